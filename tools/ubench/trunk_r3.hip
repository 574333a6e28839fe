// Scratch (GPU): the production trunk kernels (k_trunk_x16 with pair publishing) at 10 x 128 and 20 x 256,
// 4096 boards, each timed twice and compared bit for bit with itself, and the time of the split-precision
// (f16x3) kernels on a random weight image.
// (Round 3 measured three variants of the kernel with this harness and removed them again: a staging-only
// build, round 2's clumped weight-fragment reads and an L2 prefetch of the weight stream -- profiles/r03/,
// docs/history/experiments.md.)
// Round 7: the rank tiles of the 128-filter NB = 4 kernel (tower_x16.hpp, CRL_TRUNK_RANKPAIR).  The default build
// times them; -DCRL_TRUNK_RANKPAIR=0 builds the board tiles of before into a second binary.  Alternate the two
// binaries in ONE run on ONE device (MATCH selects rows by name): devices differ by up to 12 % on MFMA loops.
// Round 11: when the upper rank half of that kernel requests its weight tiles (tower_x16.hpp, CRL_TRUNK_DMA_PHASE:
// 0 = with its partner wave, directly behind the tap's sync; 1 = half a sub-step later; 2 = a whole sub-step later;
// 3 = piece by piece over four half sub-steps).  Build -DCRL_TRUNK_DMA_PHASE=0 beside the default (and 1 .. 3 to
// compare them) and alternate the binaries as above; the last column is a hash of head_out, equal across all of them.
// -DCRL_TRUNK_STAMPS (with -DCRL_TRUNK_DMA_PHASE=0 .. 2) adds a diagnostic section: in-kernel cycle stamps around the tap
// sync and around the weight requests, per rank half (tower_x16.hpp).  Read that build's shares, never its run time.
// Round 13: the partner balance of that kernel (tower_x16.hpp, ALT = 1: CRL_TRUNK_ALT_EDGE 0 / 1, CRL_TRUNK_ALT_REQ 0 .. 2).  Every
// binary holds the production kernel (ALT = 0) and ONE balance variant and times them alternately, three times each in the
// 10 x 128 section, against the production kernel's head_out; the stamps build reads both.  Build one binary per variant
// (-DCRL_TRUNK_ALT_EDGE=1 -DCRL_TRUNK_ALT_REQ=0 -o trunk_r3_e1r0, ...) and run them in one call on one device.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I chessrl_amd/csrc tools/ubench/trunk_r3.hip -o tools/ubench/trunk_r3
// hipcc ... -DCRL_TRUNK_RANKPAIR=0 tools/ubench/trunk_r3.hip -o tools/ubench/trunk_r3_boards
// hipcc ... -DCRL_TRUNK_DMA_PHASE=0 tools/ubench/trunk_r3.hip -o tools/ubench/trunk_r3_phase0
//   [MATCH="x16<128,4> pair (production)"] ./trunk_r3 [boards=4096] [reps=20]
#include "tower_x16.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace crl_tower;
typedef void (*kern_t)(const unsigned char *, const unsigned char *, const float *, float *, int,
                       const float *, const float *, float *);
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

constexpr int BAL = RankTiles<128, 4, 1, 0, 0, 0>::value ? 1 : 0;      // the partner balance exists with rank tiles only
struct Bufs { unsigned char *planes, *wts; float *bias, *head_w, *head_b, *head_out; };
static uint32_t rng_state = 12345;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static Bufs make(int F, int blocks, int boards, int image_mult)
{
    Bufs b;
    const int n_convs = 1 + 2 * blocks;
    const size_t wbytes = ((size_t)9 * 128 * F + (size_t)2 * blocks * 9 * F * F) * 2 * image_mult;
    std::vector<uint64_t> planes((size_t)boards * 128);
    for (auto &p : planes) { uint64_t v = 0; for (int i = 0; i < 64; i++) if (rnd() % 8 == 0) v |= 1ull << i; p = v; }
    std::vector<_Float16> w(wbytes / 2);
    const float scale = 1.5f / sqrtf(9.0f * F);
    for (auto &x : w) x = (_Float16)(((int)(rnd() % 2001) - 1000) * 1e-3f * scale);
    std::vector<float> bias((size_t)n_convs * F), hw(3 * F), hb(3);
    for (auto &x : bias) x = ((int)(rnd() % 201) - 100) * 1e-3f;
    for (auto &x : hw) x = ((int)(rnd() % 201) - 100) * 1e-3f;
    for (auto &x : hb) x = 0.1f;
    CK(hipMalloc(&b.planes, planes.size() * 8)); CK(hipMemcpy(b.planes, planes.data(), planes.size() * 8, hipMemcpyHostToDevice));
    CK(hipMalloc(&b.wts, wbytes)); CK(hipMemcpy(b.wts, w.data(), wbytes, hipMemcpyHostToDevice));
    CK(hipMalloc(&b.bias, bias.size() * 4)); CK(hipMemcpy(b.bias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&b.head_w, hw.size() * 4)); CK(hipMemcpy(b.head_w, hw.data(), hw.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc(&b.head_b, 12)); CK(hipMemcpy(b.head_b, hb.data(), 12, hipMemcpyHostToDevice));
    CK(hipMalloc(&b.head_out, (size_t)boards * 192 * 4));
    return b;
}

static double run(const char *name, kern_t k, int lds, int nb, int F, int blocks, int boards, int reps,
                  const Bufs &b, std::vector<float> &out, const std::vector<float> *ref)
{
    const char *match = getenv("MATCH");
    if (match && !strstr(name, match)) return 0;
    CK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    CK(hipMemset(b.head_out, 0, (size_t)boards * 192 * 4));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    double best = 1e9;
    for (int round = 0; round < 3; round++) {
        for (int i = 0; i < 2; i++)
            hipLaunchKernelGGL(k, dim3(boards / nb), dim3(512), lds, 0, b.planes, b.wts, b.bias, nullptr, blocks, b.head_w, b.head_b, b.head_out);
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0));
        for (int i = 0; i < reps; i++)
            hipLaunchKernelGGL(k, dim3(boards / nb), dim3(512), lds, 0, b.planes, b.wts, b.bias, nullptr, blocks, b.head_w, b.head_b, b.head_out);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        if (ms / reps < best) best = ms / reps;
    }
    CK(hipGetLastError());
    out.resize((size_t)boards * 192);
    CK(hipMemcpy(out.data(), b.head_out, out.size() * 4, hipMemcpyDeviceToHost));
    const double flops = 2.0 * (73152.0 * F + 1152.0 * F * F * blocks + 192.0 * F) * boards;
    const bool same = ref && memcmp(ref->data(), out.data(), out.size() * 4) == 0;
    uint64_t h = 1469598103934665603ull;                // FNV-1a of head_out: comparable across binaries
    for (size_t i = 0; i < out.size() * 4; i++) h = (h ^ reinterpret_cast<const unsigned char *>(out.data())[i]) * 1099511628211ull;
    printf("%-44s %8.4f ms  %7.1f TFLOP/s (algorithmic)  frac %.3f  %s  %016llx\n", name, best, flops / best / 1e9,
           flops / best / 1e9 / 2500.0, !ref ? "reference" : (same ? "bit-identical" : "DIFFERENT"), (unsigned long long)h);
    fflush(stdout);
    return best;
}

int main(int argc, char **argv)
{
    const int boards = argc > 1 ? atoi(argv[1]) : 4096, reps = argc > 2 ? atoi(argv[2]) : 20;
    std::vector<float> ref, out;
    char balance[96];
    snprintf(balance, sizeof balance, "x16<128,4> pair balance (ALT 1: edge %d, requests %d)", CRL_TRUNK_ALT_EDGE, CRL_TRUNK_ALT_REQ);
    for (int rep = 0; rep < 3; rep++) {
        Bufs b = make(128, 10, boards, 1);
        printf("== 10 x 128, %d boards (pass %d), production = %s tiles\n", boards, rep,
               RankTiles<128, 4, 1, 0, 0, 0>::value ? "rank" : "board");
        const int lds = Geo16<128, 4>::lds_bytes(ring_slots<4, 1, 0>());
        run("x16<128,4> pair (production)", k_trunk_x16<128, 4, 1, 0, 1>, lds, 4, 128, 10, boards, reps, b, ref, nullptr);
        if (BAL) run(balance, k_trunk_x16<128, 4, 1, BAL, 1>, lds, 4, 128, 10, boards, reps, b, out, &ref);
        run("x16<128,4> pair (production) again", k_trunk_x16<128, 4, 1, 0, 1>, lds, 4, 128, 10, boards, reps, b, out, &ref);
    }
#if defined(CRL_TRUNK_STAMPS)
    for (int alt = 0; alt <= BAL; alt++) {   // per wave [loop, sync wait, requests, syncs, one stamp]: means over the workgroups, per rank half (waves 0-3 / 4-7)
        const kern_t kern = alt ? k_trunk_x16<128, 4, 1, BAL, 1> : k_trunk_x16<128, 4, 1, 0, 1>;
        Bufs b = make(128, 10, boards, 1);
        const int lds = Geo16<128, 4>::lds_bytes(ring_slots<4, 1, 0>()), n_wg = boards / 4;
        const size_t n_dbg = (size_t)n_wg * 8 * 5;
        unsigned long long *d_dbg;
        CK(hipMalloc(&d_dbg, n_dbg * 8));
        CK(hipMemset(d_dbg, 0, n_dbg * 8));
        CK(hipMemcpyToSymbol(HIP_SYMBOL(crl_trunk_stamp_buf), &d_dbg, sizeof d_dbg));
        CK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        for (int i = 0; i < 3; i++)
            hipLaunchKernelGGL(kern, dim3(n_wg), dim3(512), lds, 0, b.planes, b.wts, b.bias, nullptr, 10, b.head_w, b.head_b, b.head_out);
        CK(hipDeviceSynchronize());
        std::vector<unsigned long long> dbg(n_dbg);
        CK(hipMemcpy(dbg.data(), d_dbg, n_dbg * 8, hipMemcpyDeviceToHost));
        for (int half = 0; half < 2; half++) {
            double sum[5] = {0, 0, 0, 0, 0};
            for (int wg = 0; wg < n_wg; wg++)
                for (int w = 4 * half; w < 4 * half + 4; w++)
                    for (int k = 0; k < 5; k++) sum[k] += (double)dbg[((size_t)wg * 8 + w) * 5 + k];
            const double nw = 4.0 * n_wg, syncs = sum[3] / nw, self = sum[4] / nw;
            printf("stamps ALT %d (edge %d, requests %d) phase %d, rank half %d, mean per wave: loop %.0f cycles, %.0f tap syncs; per sync: vmcnt wait + barrier %.0f, "
                   "weight requests %.0f (one stamp's own %.0f taken off each); per convolution of 9 taps: %.0f and %.0f of %.0f\n",
                   alt, alt ? CRL_TRUNK_ALT_EDGE : 0, alt ? CRL_TRUNK_ALT_REQ : 0, CRL_TRUNK_DMA_PHASE, half, sum[0] / nw, syncs, sum[1] / nw / syncs - self, sum[2] / nw / syncs - self, self,
                   9 * (sum[1] / nw / syncs - self), 9 * (sum[2] / nw / syncs - self), sum[0] / nw / 21);
        }
    }
#endif
    if (getenv("ONLY128")) return 0;                    // the balance variants: the 10 x 128 sections alone
    {
        Bufs b = make(256, 20, boards, 1);
        printf("== 20 x 256, %d boards\n", boards);
        const int lds = Geo16<256, 2>::lds_bytes(ring_slots<2, 1, 0>());
        run("x16<256,2> pair (production)", k_trunk_x16<256, 2, 1, 0, 1>, lds, 2, 256, 20, boards, 5, b, ref, nullptr);
        run("x16<256,2> pair (production) again", k_trunk_x16<256, 2, 1, 0, 1>, lds, 2, 256, 20, boards, 5, b, out, &ref);
    }
    {   // split precision: three MFMAs per product over a 2x weight image (random values: time only)
        Bufs b = make(128, 10, boards, 2);
        printf("== f16x3 (split operands), %d boards\n", boards);
        run("x16<128,2> pair split, 10 x 128", k_trunk_x16<128, 2, 1, 0, 1, 0, 1>, Geo16<128, 2, 1>::lds_bytes(ring_slots<2, 1, 0>()), 2, 128, 10, boards, reps, b, ref, nullptr);
        Bufs c = make(256, 20, boards, 2);
        run("x16<256,1> split, 20 x 256", k_trunk_x16<256, 1, 1, 0, 0, 0, 1>, Geo16<256, 1, 1>::lds_bytes(ring_slots<1, 0, 0>()), 1, 256, 20, boards, 3, c, ref, nullptr);
        Bufs d = make(64, 6, boards, 2);
        run("x16<64,4> split, 6 x 64", k_trunk_x16<64, 4, 1, 0, 0, 0, 1>, Geo16<64, 4, 1>::lds_bytes(ring_slots<4, 0, 0>()), 4, 64, 6, boards, reps, d, ref, nullptr);
    }
    return 0;
}
