"""Residual policy/value tower on MFMA (PyTorch-ROCm, fp16, channels-last).

Host-side mirror of the reference's ``ChessModel``
(/root/reference/src/chessrl/model.py:15-81): same topology and Keras inference
semantics, parametrised by (blocks, filters) for the
BASELINE configs; the reference's own values are (10, 256).  Inference is the hot
path (fused HIP trunk); training (model.py:69-72,83-99)
lives in chessrl_amd/train.py and hands its weights back through ``load_dict``.

MI355X design notes: the input is the encoder kernel's fp16 NHWC [B,8,8,128]
buffer used in place (channel 127 is a zero pad, so K = 9*128 is a multiple of
the MFMA K-step); BatchNorm is folded into the preceding conv in fp32 before
the cast to fp16; softmax / tanh run in fp32.  Weights are exchanged as a flat
``name -> ndarray`` dict in Keras layouts (conv HWIO, dense (in,out)), saved as
``.npz`` or as a Keras ``.h5`` weight file (chessrl_amd/keras_h5.py; no h5py needed).
"""
import logging

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, packing, precision as rules
from .packing import BN_EPS, N_POLICY, PAD_PLANES, fold as _fold  # noqa: F401  (names other modules import from here)

log = logging.getLogger("chessrl_amd.model")

IN_PLANES = 127


def init_weights(blocks, filters, seed=0):
    """Keras-default initialisation: Glorot-uniform kernels, zero biases, BN identity stats."""
    rng = np.random.default_rng(seed)
    w = {}

    def glorot(shape, fan_in, fan_out):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        return rng.uniform(-lim, lim, size=shape).astype(np.float32)

    def conv(name, k, cin, cout):
        w[name + ".kernel"] = glorot((k, k, cin, cout), k * k * cin, k * k * cout)
        w[name + ".bias"] = np.zeros(cout, np.float32)

    def bn(name, c):
        w[name + ".gamma"] = np.ones(c, np.float32)
        w[name + ".beta"] = np.zeros(c, np.float32)
        w[name + ".mean"] = np.zeros(c, np.float32)
        w[name + ".var"] = np.ones(c, np.float32)

    def dense(name, cin, cout):
        w[name + ".kernel"] = glorot((cin, cout), cin, cout)
        w[name + ".bias"] = np.zeros(cout, np.float32)

    conv("stem", 3, IN_PLANES, filters)
    for i in range(blocks):
        conv("block%d.conv1" % i, 3, filters, filters)
        bn("block%d.bn1" % i, filters)
        conv("block%d.conv2" % i, 3, filters, filters)
        bn("block%d.bn2" % i, filters)
    conv("policy.conv", 1, filters, 2)
    bn("policy.bn", 2)
    dense("policy.dense", 128, N_POLICY)
    conv("value.conv", 1, filters, 1)
    bn("value.bn", 1)
    dense("value.dense1", 64, 256)
    dense("value.dense2", 256, 1)
    w["meta.blocks"] = np.array(blocks)
    w["meta.filters"] = np.array(filters)
    return w


def _read_weights(path):
    if str(path).endswith((".h5", ".hdf5")):
        from .keras_h5 import load_keras_h5
        return load_keras_h5(path)
    return dict(np.load(path))


def _dmax(a, b):
    return float((a - b).abs().max())


_PROBE = {}


def _probe_bitplanes(device, n):
    """``n`` REAL self-play positions as plane bitboards (int64 [n,128], the encoder's compact form) for the
    precision probe of ``ChessModel(precision="auto")``: 128 complete games played once per process and
    device by a fixed tiny net (2 x 64 filters, seed 20260, 16 simulations per move, Dirichlet noise, all on
    the HIP kernels: ~1.5 s), positions drawn evenly over every game's length -- openings, middle games, the
    long endgames random play drifts into, positions after promotions.  Independent of the weights being
    probed, so every rank and every reload of a run judges its weights on the same positions.  (Rounds 3-4a
    probed 256 random-playout positions: on a trained net the maximum over real positions was 2.3x the
    probe's and "auto" kept f16 at |dpolicy| = 1.08e-3; bench.py's parity gate caught it.)"""
    key, n_all = str(device), 4096
    if n > n_all:
        raise ValueError("at most %d probe positions" % n_all)
    if key not in _PROBE:
        n_want, n = n, n_all
        from .engine import LockstepEngine
        from .selfplay import SelfPlayRunner
        dev = torch.device(device)
        tiny = ChessModel(blocks=2, filters=64, seed=20260, device=str(dev), precision="f16")
        games = 128
        side = SelfPlayRunner(tiny, games, 16, seed=20260, noise=True, total_games=games, max_plies=1024,
                              device=dev.index or 0)
        recs = side.run()
        side.close()
        rng = np.random.default_rng(20260)
        moves = [np.asarray(r.moves, dtype=np.uint16) for r in sorted(recs, key=lambda r: r.game_id) if len(r.moves) >= 8]
        total = sum(len(m) for m in moves)
        prefixes = []
        for m in moves:
            k = max(1, int(round(n * len(m) / total)))
            for ply in np.unique(rng.integers(0, len(m) + 1, size=k)):
                prefixes.append(m[:int(ply)])
        while len(prefixes) < n:
            m = moves[int(rng.integers(len(moves)))]
            prefixes.append(m[:int(rng.integers(0, len(m) + 1))])
        prefixes = prefixes[:n]
        eng = LockstepEngine(tiny, n_games=n, max_sims=2, use_graph=False, max_plies=1024, device=dev.index or 0)
        eng.load_moves(prefixes)
        eng.ctx.encode(eng.planes_s1.data_ptr())
        eng.ctx.sync()
        # (a fixed shuffle: any leading part of the set is a sample of the whole)
        order = torch.from_numpy(np.random.default_rng(20261).permutation(n)).to(dev)
        _PROBE[key] = eng.planes_s1[order].contiguous()
        eng.close()
        n = n_want
    return _PROBE[key][:n]


class _DeviceArray(object):
    """A raw device pointer as something ``torch.as_tensor`` understands (``__cuda_array_interface__``): the label /
    count lists of the search kernels are known to the host as addresses only (crl_eval_labels)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class _ClosingStamp(object):
    """What ``ChessModel._trunk_event`` hands back while stamps are on: ``record()`` issues the stamp that closes the launch."""

    def __init__(self, stamp_fn, sid):
        self._fn, self._sid = stamp_fn, sid

    def record(self):
        self._fn(self._sid)


class Tower(nn.Module):
    """Inference tower; input (B,128,8,8) channels_last fp16, i.e. NHWC memory."""

    def __init__(self, blocks, filters):
        super().__init__()
        self.blocks_n, self.filters = blocks, filters
        self.stem = nn.Conv2d(PAD_PLANES, filters, 3, padding=1)
        self.conv1 = nn.ModuleList([nn.Conv2d(filters, filters, 3, padding=1) for _ in range(blocks)])
        self.conv2 = nn.ModuleList([nn.Conv2d(filters, filters, 3, padding=1) for _ in range(blocks)])
        self.policy_conv = nn.Conv2d(filters, 2, 1)
        self.policy_fc = nn.Linear(128, N_POLICY)
        self.value_conv = nn.Conv2d(filters, 1, 1)
        self.value_fc1 = nn.Linear(64, 256)
        self.value_fc2 = nn.Linear(256, 1)

    @torch.no_grad()
    def load_keras_dict(self, w):
        k, b = _fold(w, "stem")
        kp = torch.zeros(k.shape[0], PAD_PLANES, 3, 3)
        kp[:, :IN_PLANES] = k
        self.stem.weight.copy_(kp)
        self.stem.bias.copy_(b)
        for i in range(self.blocks_n):
            for conv, name, bn in ((self.conv1[i], "block%d.conv1" % i, "block%d.bn1" % i),
                                   (self.conv2[i], "block%d.conv2" % i, "block%d.bn2" % i)):
                k, b = _fold(w, name, bn)
                conv.weight.copy_(k)
                conv.bias.copy_(b)
        for conv, name, bn in ((self.policy_conv, "policy.conv", "policy.bn"),
                               (self.value_conv, "value.conv", "value.bn")):
            k, b = _fold(w, name, bn)
            conv.weight.copy_(k)
            conv.bias.copy_(b)
        for fc, name in ((self.policy_fc, "policy.dense"), (self.value_fc1, "value.dense1"),
                         (self.value_fc2, "value.dense2")):
            fc.weight.copy_(torch.from_numpy(np.asarray(w[name + ".kernel"], np.float32)).t())
            fc.bias.copy_(torch.from_numpy(np.asarray(w[name + ".bias"], np.float32)))

    def trunk(self, x):
        x = self.stem(x)                                     # no BN / activation (model.py:33-34)
        for c1, c2 in zip(self.conv1, self.conv2):
            y = F.relu(c1(x))
            y = c2(y)
            x = F.relu(x + y)
        return x

    def forward(self, x):
        return self.heads(self.trunk(x))

    def heads(self, x):
        """Policy and value heads on the trunk activations (B,F,8,8), in fp32."""
        b = x.shape[0]
        x = x.float()                                        # heads are tiny: run them in fp32
        p = F.relu(self.policy_conv(x)).permute(0, 2, 3, 1).reshape(b, 128)   # Keras Flatten (h,w,c)
        p = torch.softmax(self.policy_fc(p), dim=-1)
        v = F.relu(self.value_conv(x)).permute(0, 2, 3, 1).reshape(b, 64)
        v = F.relu(self.value_fc1(v))
        v = torch.tanh(self.value_fc2(v))
        return p, v[:, 0]

    def cast_for_inference(self, device, dtype):
        """Trunk (stem + residual blocks) in `dtype` on MFMA, heads in fp32."""
        self.to(device)
        for m in [self.stem] + list(self.conv1) + list(self.conv2):
            m.to(dtype)
        return self.to(memory_format=torch.channels_last).eval()


class ChessModel(object):
    """Mirror of the reference ``ChessModel`` (model.py:15-99).

    ``predict(inp)`` takes (B,8,8,127) like Keras ``model.predict`` and returns
    ``[policy (B,1968), value (B,1)]`` numpy arrays.  ``__call__(planes)`` is the
    device-resident path the engine uses: fp16 NHWC [B,8,8,128] CUDA tensor in,
    (policy f32 [B,1968], value f32 [B]) CUDA tensors out.
    """

    # precision modes of the fused HIP trunk (dtype float16); errors are max |policy| / |value|
    # differences to the fp32 oracle over 4096 real self-play positions, profiles/r03/tower_sharp_probe.json:
    #   "f16"    one fp16 MFMA per product, fp32 accumulation and skip stream: BASELINE's "fp16 MFMA
    #            inference", what bench.py times.  Keras-initialised towers: 4e-4 (6x64, 20x256) to
    #            1.3e-3 (10x128, 10x256: a handful of positions in 4096 beyond 1e-3); a SHARP tower
    #            (peaked policy, values spread over (-1, 1), unit-gain layers): 6e-3 .. 2.4e-2.
    #   "f16x3"  every operand carried as a hi + lo fp16 pair, three MFMAs per product
    #            (CRL_TRUNK_SPLIT): 3e-6 .. 8e-5 on every tower and weight set, the same as PyTorch's
    #            fp32 convolutions, at 2.5x (64 filters), 3.1x (128) and 3.6x (256) the trunk time.
    #   "auto"   (default: the 1e-3 bar of the drop-in contract comes first) decided per weight set
    #            when it is loaded: both modes evaluate a fixed probe set of positions (random playouts
    #            by the rules kernels) and "f16" is kept only if it stays within PROBE_TOL of "f16x3"
    #            on all of them (the maximum over thousands of real positions is up to 1.7x the probe's).
    #   "hybrid" the 1e-3 outputs -- priors and value of S2 -- in "f16x3"; an evaluation of S1, which only
    #            chooses the opponent's reply (argmax over the legal labels, agentdistributed.py:57-58), in
    #            "f16" first, and only the boards whose two best legal moves lie closer than HYBRID_K x the
    #            f16-vs-f16x3 distance of these weights (log space, measured on the probe positions) again
    #            in "f16x3" (crl_reply_margin + crl_trunk_forward_indexed).  Measured on 1.18 M S1 positions
    #            of real searches per net (profiles/r04/hybrid_s1_probe.json): 3-7 % of the boards fall back
    #            on sharp nets, 1 % on Keras-initialised ones, and every reply equals the pure f16x3 reply.
    #            What "auto" picks when f16 misses the tolerance.
    PRECISIONS = ("auto", "f16", "f16x3", "hybrid")
    PROBE_TOL = 8e-4         # on PROBE_POSITIONS real self-play positions; f16x3 itself is within 1e-4 of fp32
    PROBE_POSITIONS = 4096
    HYBRID_K = 2.0           # margin = HYBRID_K x max |log p_f16 - log p_f16x3| on the probe positions
    HYBRID_MIN_BOARDS = 2048 # below, an S1 batch is simply evaluated in f16x3: the f16 pass + the fall-back launch
                             # are two workgroup rounds, and a batch this small is one or two rounds of the split
                             # kernel anyway (C2's 512 boards: hybrid 0.351 ms per step against 0.288 in f16x3)
    AUTO_STRICT = "hybrid"   # what "auto" runs when f16 is not within PROBE_TOL ("f16x3" = no S1 shortcut)
    STICKY_FACTOR = 0.5      # after the run-time guard has fired, f16 is re-entered only below STICKY_FACTOR x PROBE_TOL
    MARGIN_CAP = 8.0         # margin_check never widens the reply margin beyond MARGIN_CAP x the probe's
    GUARD_TOL = 9e-4         # run-time guard of an auto-kept "f16": |f16 - f16x3| on the run's OWN tree leaves beyond
                             # which the model leaves f16 for AUTO_STRICT (f16x3 is within 1e-4 of fp32: 1e-3 in all)

    def __init__(self, compile_model=False, weights=None, blocks=10, filters=256, device="cuda:0",
                 dtype=torch.float16, seed=0, fused=True, precision="auto"):
        self.compiled = bool(compile_model)      # model.py:69-72: Adam(lr=0.002), cce + mse
        self._trainer = None
        if precision not in self.PRECISIONS:
            raise ValueError("precision must be one of %s" % (self.PRECISIONS,))
        self.precision_requested = precision
        self.precision = None                    # resolved per weight set ("f16" / "f16x3"; the dtype otherwise)
        self.precision_probe = None              # what "auto" measured
        self.reply_margin = None                 # hybrid: log-margin below which an S1 board is evaluated again
        self._reply_margin_dev = None            # ... as the kernel reads it: ONE float in device memory, rewritten in
                                                 # place with every weight set (a by-value argument would stay what it
                                                 # was when a hipGraph captured the launch)
        self._fallback = {}                      # hybrid: batch size -> the device list of boards to evaluate again
        self.graph_epoch = 0                     # bumped when the kernel a captured graph holds changes
        self.trunk_events = None                 # bench.py: a list -> every trunk launch is bracketed by HIP events
        self.stamp_fn = None                     # bench.py: StampRing.stamp -> every trunk launch is bracketed by stamp
                                                 # kernels that capture into the step's hipGraph (engine.set_stamps)
        self.guard = {"checks": 0, "positions": 0, "worst": 0.0, "fired": None}   # guard_check's record
        self._scratch = {}                       # batch size -> slice statistics of the small-batch heads
        self._workspace = None                   # activation images of the layer-wise trunk (256 filters, f16x3): ONE buffer,
                                                 # sized for the largest batch seen (graph_epoch is bumped when it grows)
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("ChessModel needs an MI355X (no CPU fallback in the product path)")
        self.dtype = dtype
        self.want_fused = fused
        if isinstance(weights, str):
            weights = _read_weights(weights)
        if weights is None:
            weights = init_weights(blocks, filters, seed)
        self.load_dict(weights)

    def load_dict(self, weights):
        """(Re)load a Keras-layout weight dict.  With an unchanged (blocks, filters) every device
        tensor is overwritten IN PLACE, so hipGraphs captured over this model (LockstepEngine) stay
        valid and see the new weights at their next replay."""
        blocks, filters = int(weights["meta.blocks"]), int(weights["meta.filters"])
        same = getattr(self, "net", None) is not None and (blocks, filters) == (self.blocks, self.filters)
        self.weights = weights
        if same:
            self.net.load_keras_dict(weights)
        else:
            if getattr(self, "net", None) is not None:
                self.graph_epoch += 1                          # another architecture: captured graphs are stale
            net = Tower(blocks, filters)
            net.load_keras_dict(weights)
            self.net = net.cast_for_inference(self.device, self._torch_dtype(filters, blocks))
            self.blocks, self.filters = blocks, filters
            self._wtiles = None
        # the hand-written fused MFMA trunk (csrc/tower_x16.hpp) covers 64, 128 and 256 filters in fp16
        self.fused = self._will_fuse(filters, blocks)
        if self.fused:
            self._pack_fused(weights)
            self._resolve_precision()
        else:
            self.precision = {torch.float16: "f16", torch.bfloat16: "bf16",
                              torch.float32: "f32"}[self._torch_dtype(filters, blocks)]

    def _will_fuse(self, filters, blocks):
        return bool(self.want_fused and filters in (64, 128, 256) and self.dtype == torch.float16
                    and 1 + 2 * blocks <= 41)

    def _torch_dtype(self, filters, blocks):
        """dtype of the PyTorch-ROCm tower.  Where the fused HIP trunk does not apply (other filter
        counts, fused=False) fp16 convolutions are only run when asked for by name (precision="f16");
        "auto" and "f16x3" mean the 1e-3 bar holds whatever the weights, which there is fp32."""
        if self.dtype == torch.float16 and not self._will_fuse(filters, blocks) and self.precision_requested != "f16":
            return torch.float32
        return self.dtype

    def _pack_fused(self, w):
        """The weight images of the HIP tower (packing.pack_weights) on the device, under the ten attribute names of
        ``packing.NAMES``.  An image of unchanged shape is overwritten in place: captured graphs stay valid."""
        want_f16 = self.precision_requested in ("auto", "f16", "hybrid")
        want_x3 = self.precision_requested in ("auto", "f16x3", "hybrid")
        new = packing.pack_weights(w, self.blocks, self.filters, want_f16, want_x3)
        first = getattr(self, "_wtiles", None) is None
        if first:
            self._pad_in = None
            self._pad_bits = None
        for name, src in zip(packing.NAMES, new):
            cur = None if first else getattr(self, name, None)
            if cur is not None and cur.shape == src.shape:
                cur.copy_(src)                                 # in place: captured graphs stay valid
            else:
                setattr(self, name, src.to(self.device).contiguous())
                if cur is not None:
                    self.graph_epoch += 1                      # a captured graph holds the old tensor

    def _run_fused(self, planes, want_trunk=False, precision=None):
        """One launch of the fused trunk kernel.  ``planes``: fp16 NHWC [B,8,8,128], or int64
        [B,128] plane bitboards (the encoder's compact form; the kernel expands them on chip).
        Returns (trunk fp32 [B,8,8,F] or None, head activations fp32 [B,192] = ReLU(1x1 head
        convs): 128 policy + 64 value)."""
        b = planes.shape[0]
        _, heads, trunk = self._launch_fused(planes, want_trunk, precision)
        return (trunk[:b] if want_trunk else None), heads[:b]

    def _run_fused_padded(self, planes, precision=None):
        """(the planes as the kernel saw them -- padded to a multiple of 4 boards --, the head activations of
        all those rows): what a second launch over the same boards needs."""
        planes_p, heads, _ = self._launch_fused(planes, False, precision)
        return planes_p, heads

    def _launch_fused(self, planes, want_trunk, precision):
        b = planes.shape[0]
        bp = (b + 3) // 4 * 4
        bits = planes.dtype == torch.int64       # 128 plane bitboards per board (CRL_PLANES_BITS)
        if bits:
            if bp != b or not planes.is_contiguous():
                if self._pad_bits is None or self._pad_bits.shape[0] != bp:
                    self._pad_bits = torch.zeros((bp, PAD_PLANES), dtype=torch.int64, device=self.device)
                self._pad_bits[:b].copy_(planes)
                planes = self._pad_bits
        elif bp != b or not planes.is_contiguous() or planes.dtype != torch.float16:
            if self._pad_in is None or self._pad_in.shape[0] != bp:
                self._pad_in = torch.zeros((bp, 8, 8, PAD_PLANES), dtype=torch.float16, device=self.device)
            self._pad_in[:b].copy_(planes)
            planes = self._pad_in
        trunk = (torch.empty((bp, 8, 8, self.filters), dtype=torch.float32, device=self.device)
                 if want_trunk else None)
        heads = torch.empty((bp, 192), dtype=torch.float32, device=self.device)
        split = self._trunk_mode(precision) == "f16x3"
        image = self._wtiles3 if split else self._wtiles
        if image.numel() <= 8:                   # the placeholder: this mode's weight image was never packed
            raise _lib.HipLibraryError("the weight image of precision mode %r is not packed (model built with "
                                       "precision=%r): use set_precision() or precision='auto'"
                                       % ("f16x3" if split else "f16", self.precision_requested))
        # (TRUNK_BALANCE: the partner-balance kernel where this batch has one -- 128 filters, four boards per workgroup --
        # and nothing elsewhere; the same bits, csrc/tower_x16.hpp ALT = 1)
        flags = (_lib.TRUNK_BITPLANES if bits else 0) | (_lib.TRUNK_SPLIT if split else _lib.TRUNK_BALANCE)
        ws = self._trunk_workspace(bp) if split else None
        ev = self._trunk_event("f16x3" if split else "f16")
        _lib.trunk_forward_x(self.filters, flags, planes, image, self._wbias, trunk, bp, self.blocks, self._head_w,
                             self._head_b, heads, ws, ws.numel() if ws is not None else 0)
        if ev is not None:
            ev[2].record()
        return planes, heads, trunk

    def _trunk_workspace(self, bp):
        """The activation images the layer-wise split-precision trunk (256 filters; csrc/tower_layer.hpp) ping-pongs
        between: ONE buffer of crl_trunk_workspace_bytes for the LARGEST batch this model has evaluated (128 KiB per
        board), lent to every smaller batch as well; None where the library wants none.  Captured graphs hold its
        address: when a larger batch makes it grow, ``graph_epoch`` is bumped and engines capture again (a compacting
        run only ever shrinks its batch, so in practice it is allocated once).  Contents are undefined between calls, so
        every caller of this model -- the engine's graph, ``guard_check``, the probe -- must launch on ONE stream at a
        time (every engine of the product does)."""
        n = _lib.trunk_workspace_bytes(self.filters, bp, _lib.TRUNK_BITPLANES | _lib.TRUNK_SPLIT)
        if n == 0:
            return None
        if self._workspace is None or self._workspace.numel() < n:
            if self._workspace is not None:
                self.graph_epoch += 1                          # a captured graph holds the old address
            self._workspace = torch.empty(n, dtype=torch.uint8, device=self.device)
        return self._workspace

    def _trunk_event(self, kind):
        """Measurement hook (bench.py's in-step kernel time): with ``trunk_events`` a list, every trunk launch is
        bracketed by two HIP events recorded on the launch stream -- (kind, start, end) is appended here, the
        caller records ``end`` behind its launch.  With ``stamp_fn`` set the launch is bracketed by stamp kernels
        instead (they capture into a hipGraph; the returned object's ``record`` issues the closing stamp).  None
        (the default) costs two attribute tests."""
        if self.stamp_fn is not None:
            from .engine import STAMP_TRUNK
            b, e = STAMP_TRUNK[kind]
            self.stamp_fn(b)
            return (kind, None, _ClosingStamp(self.stamp_fn, e))
        if self.trunk_events is None:
            return None
        make = getattr(self, "trunk_event_cls", None) or torch.cuda.Event      # (bench.py: events without a system fence)
        ev = (kind, make(enable_timing=True), make(enable_timing=True))
        ev[1].record()
        self.trunk_events.append(ev)
        return ev

    def _trunk_mode(self, precision=None):
        """The trunk arithmetic of a full evaluation in mode ``precision`` (default: the resolved mode):
        "hybrid" evaluates everything but the reply choice in "f16x3"."""
        p = precision or self.precision
        return "f16x3" if p in ("f16x3", "hybrid") else p

    def set_precision(self, precision):
        """Switch the fused trunk's arithmetic mode on the loaded weights ("auto" re-runs the probe).
        Engines holding a captured hipGraph notice through ``graph_epoch`` and capture again."""
        if precision not in self.PRECISIONS:
            raise ValueError("precision must be one of %s" % (self.PRECISIONS,))
        if not self.fused:
            raise RuntimeError("precision modes belong to the fused HIP trunk")
        self.precision_requested = precision
        self._pack_fused(self.weights)           # the image of the other mode may not exist yet
        self._resolve_precision()
        return self.precision

    def probe_error(self):
        """max |policy| and |value| difference between the "f16" and "f16x3" modes on the probe
        positions (the latter is within ~1e-4 of fp32): how far the fast mode is from the reference
        arithmetic on THESE weights.  Packs both images for the measurement, leaves the mode as it was."""
        keep_req, keep = self.precision_requested, self.precision
        self.precision_requested = "auto"
        self._pack_fused(self.weights)
        planes = _probe_bitplanes(self.device, self.PROBE_POSITIONS)
        (pa, va), (pb, vb) = self._both(planes)
        self.precision_requested, self.precision = keep_req, keep
        return {"positions": int(planes.shape[0]), "dpolicy_max": _dmax(pa, pb), "dvalue_max": _dmax(va, vb)}

    def _both(self, planes):
        """``planes`` in both arithmetics: (policy, value) of "f16", then (policy, value) of "f16x3"."""
        return self._forward_fused(planes, precision="f16"), self._forward_fused(planes, precision="f16x3")

    def _auto_kept_f16(self):
        """Whether the model runs an "f16" that "auto" chose on the probe: what the run-time guard watches and leaves."""
        return bool(self.fused and self.precision == "f16" and self.precision_requested == "auto")

    def _resolve_precision(self):
        """Fix ``self.precision`` for the weights just packed.  "auto": evaluate the probe positions in
        both modes and keep the single-MFMA mode only if its outputs stay within PROBE_TOL of the
        split mode's (which is itself within ~1e-4 of fp32); otherwise AUTO_STRICT.  "hybrid" (asked for or
        picked) also fixes the reply margin from the same probe.  A changed decision invalidates captured
        hipGraphs (``graph_epoch``; LockstepEngine re-captures)."""
        before = self.precision
        if self.precision_requested not in ("auto", "hybrid"):
            self.precision = self.precision_requested
        else:
            planes = _probe_bitplanes(self.device, self.PROBE_POSITIONS)
            (pa, va), (pb, vb) = self._both(planes)
            dp, dv = _dmax(pa, pb), _dmax(va, vb)
            # the same distance in log space: a rounding error of the trunk moves a LOGIT, i.e. a probability
            # by a factor -- what decides whether an argmax over the legal moves can flip
            dlog = rules.log_distance(pa, pb)
            if dlog is None:                                 # (degenerate weights: no finite log-distance anywhere)
                dlog = float("nan")                          # a NaN margin lists every board: f16x3 everywhere
            sticky = self.guard.get("fired") is not None     # (the guard has fired in this run: precision.probe_tolerance)
            tol = rules.probe_tolerance(self.PROBE_TOL, self.STICKY_FACTOR, sticky)
            self.precision = rules.choose_mode(self.precision_requested, dp, dv, tol, self.AUTO_STRICT)
            self.reply_margin = self.HYBRID_K * dlog
            self._probe_margin = self.reply_margin
            self._publish_reply_margin()
            self.precision_probe = {"positions": int(planes.shape[0]), "dpolicy_max": dp, "dvalue_max": dv,
                                    "dlog_policy_max": dlog, "tolerance": tol, "sticky_after_guard": sticky,
                                    "chosen": self.precision,
                                    "reply_margin": self.reply_margin if self.precision == "hybrid" else None}
        if before is not None and before != self.precision:
            self.graph_epoch += 1

    @torch.no_grad()
    def guard_check(self, planes):
        """Run-time guard of a mode that "auto" chose on a PROBE: the probe is 4096 positions of a fixed tiny net's
        games, a run evaluates millions of its own (8e-4 on the probe leaves little margin for their
        maximum).  While the model runs an auto-kept "f16", the self-play runner hands over, every few moves, the
        tower inputs its search has just evaluated (the G tree leaves of the last simulation); they are evaluated
        in both arithmetics and beyond GUARD_TOL the model leaves f16 for AUTO_STRICT -- from the next step on
        (``graph_epoch``: engines capture again).  Returns max |f16 - f16x3| over policy and value, or None when
        there is nothing to guard (a mode asked for by name, a strict mode, the PyTorch tower)."""
        if self.fused and self.precision == "hybrid":
            self.margin_check(planes)
            return None
        if not self._auto_kept_f16():
            return None
        (pa, va), (pb, vb) = self._both(planes)
        d = max(_dmax(pa, pb), _dmax(va, vb))
        g = self.guard
        g["checks"] += 1
        g["positions"] += int(planes.shape[0])
        g["worst"] = max(g["worst"], d)
        if d > self.GUARD_TOL:
            self.enter_strict({"after_checks": g["checks"], "after_positions": g["positions"], "distance": d,
                               "tolerance": self.GUARD_TOL})
        return d

    def enter_strict(self, why):
        """Leave an auto-kept "f16" for AUTO_STRICT from the next step on (``graph_epoch``: engines capture again):
        the run-time guard's action, also taken when ANOTHER rank's guard fired (SelfPlayRunner._follow_strictest).
        Sticky for the run: later weight sets are kept in f16 only when the probe passes with margin
        (``_resolve_precision``).  False when there is nothing to leave (a mode asked for by name, a strict mode)."""
        if not self._auto_kept_f16():
            return False
        fired = dict(why) if isinstance(why, dict) else {"why": str(why)}
        fired.update({"from": "f16", "to": self.AUTO_STRICT})
        self.guard["fired"] = fired
        self.precision = self.AUTO_STRICT
        self.graph_epoch += 1
        if self.precision_probe is not None:
            self.precision_probe = dict(self.precision_probe, chosen=self.precision, guard=fired,
                                        reply_margin=self.reply_margin)
        return True

    @torch.no_grad()
    def margin_check(self, planes):
        """The same hand-over while the model runs "hybrid": its reply margin is HYBRID_K x the largest
        |log p_f16 - log p_f16x3| of the PROBE positions, and a run's own positions can differ by more.  Measure
        that distance on the positions handed over and, where HYBRID_K x it exceeds the margin in force, widen the
        margin -- in the device float the captured graphs read, so from the very next step and without a
        re-capture.  A wider margin only lists more boards for the second, f16x3 evaluation; results do not change.
        Returns the distance measured."""
        (pa, _), (pb, _) = self._both(planes)
        dlog = rules.log_distance(pa, pb)
        g = self.guard
        g["margin_checks"] = g.get("margin_checks", 0) + 1
        g["margin_positions"] = g.get("margin_positions", 0) + int(planes.shape[0])
        if dlog is None:                                     # nothing comparable on these positions: no decision
            return None
        g["worst_dlog"] = max(g.get("worst_dlog", 0.0), dlog)
        g.setdefault("margin_at_start", self.reply_margin)
        probe_margin = getattr(self, "_probe_margin", None) or g["margin_at_start"]
        wider, capped = rules.widened_margin(self.reply_margin, probe_margin, dlog, self.HYBRID_K, self.MARGIN_CAP)
        if capped:
            g["margin_capped"] = g.get("margin_capped", 0) + 1
            log.warning("hybrid reply margin: %.3e asked for by this run's positions, capped at %.3e (%g x the probe's)",
                        self.HYBRID_K * dlog, self.MARGIN_CAP * probe_margin, self.MARGIN_CAP)
        if wider > self.reply_margin:
            g["margin_widened"] = g.get("margin_widened", 0) + 1
            self.reply_margin = wider
            self._publish_reply_margin()
        g["margin"] = self.reply_margin
        return dlog

    _log_distance = staticmethod(rules.log_distance)

    @torch.no_grad()
    def reply_rule_check(self, planes, labels_ptr, counts_ptr):
        """The hybrid mode's reply rule, watched at run time on the run's own positions.  The rule: a board whose two best
        LEGAL moves are at least ``reply_margin`` apart in log p (in f16) keeps its f16 reply; only closer calls are
        evaluated again in f16x3.  It is an empirical rule (the margin is 2 x a SAMPLED arithmetic distance), so the same
        hand-over that re-measures that distance also checks the rule itself: the positions are evaluated in both
        arithmetics, the argmax over the legal labels (``labels_ptr`` uint16 [n,256] / ``counts_ptr`` int32 [n]: the
        device lists the search kernels wrote for these positions) is taken in both, and every board whose choice differs
        must be one the rule lists.  A board that is NOT listed and differs is a failure of the rule: it is counted
        (``guard["reply_rule"]``), logged, and the margin is widened past that board's gap at once.  Costs two legal-prior
        head passes beside margin_check's two trunk evaluations; returns the record of this check or None outside hybrid."""
        if not (self.fused and self.precision == "hybrid"):
            return None
        n = planes.shape[0]
        pri = []
        for mode in ("f16", "f16x3"):
            _, hp = self._run_fused(planes, precision=mode)
            out = torch.zeros((n, 256), dtype=torch.float32, device=self.device)
            _lib.heads_forward_legal(hp, n, *self._dense_images(), labels_ptr, counts_ptr, out, None, self._heads_scratch(n))
            pri.append(out)
        counts = torch.as_tensor(_DeviceArray(counts_ptr, (n,), "<i4"), device=self.device).clone()
        listed, differ, unlisted, gap = rules.reply_rule(pri[0], pri[1], counts, self.reply_margin)
        g = self.guard.setdefault("reply_rule", {"checks": 0, "boards": 0, "listed": 0, "replies_that_differ": 0,
                                                 "differ_but_not_listed": 0, "largest_gap_of_a_differing_reply": 0.0})
        g["checks"] += 1
        g["boards"] += int((counts >= 2).sum())
        g["listed"] += int(listed.sum())
        g["replies_that_differ"] += int(differ.sum())
        if bool(differ.any()):
            g["largest_gap_of_a_differing_reply"] = max(g["largest_gap_of_a_differing_reply"], float(gap[differ].max()))
        bad = int(unlisted.sum())
        if bad:
            g["differ_but_not_listed"] += bad
            worst = float(gap[unlisted].max())
            log.error("hybrid reply rule: %d of %d boards choose another reply in f16 than in f16x3 WITHOUT being listed "
                      "(gap up to %.3e, margin %.3e): margin widened", bad, n, worst, self.reply_margin)
            self.reply_margin = max(self.reply_margin, 1.25 * worst)
            self._publish_reply_margin()
            self.guard["margin"] = self.reply_margin
        return {"boards": int((counts >= 2).sum()), "listed": int(listed.sum()), "differ": int(differ.sum()), "unlisted": bad}

    def check_on_run(self, planes, labels_ptr=None, counts_ptr=None):
        """What a run does every few move boundaries with the tower inputs its search has just evaluated: the guard of
        an auto-kept "f16" or the margin check of "hybrid" (``guard_check``) and, in hybrid with the positions' legal
        labels at hand, the reply rule itself on the same positions; what changed is logged.  Returns guard_check's."""
        before, margin = self.precision, self.reply_margin
        d = self.guard_check(planes)
        if before == "hybrid":
            if labels_ptr is not None:
                self.reply_rule_check(planes, labels_ptr, counts_ptr)
            if self.reply_margin != margin:
                log.info("hybrid reply margin widened from %.3e to %.3e (log-policy distance of f16 on this run's own "
                         "tree leaves)", margin, self.reply_margin)
        if d is not None and self.precision != before:
            log.warning("tower precision guard: |f16 - f16x3| = %.2e on this run's own tree leaves (tolerance %.1e): "
                        "%s -> %s from the next move on", d, self.GUARD_TOL, before, self.precision)
        return d

    def _publish_reply_margin(self):
        """Write ``reply_margin`` into the device float crl_reply_margin reads (allocated once, rewritten in
        place: captured graphs hold its address and see the margin of the weights they run with)."""
        src = torch.tensor([float(self.reply_margin)], dtype=torch.float32)
        if self._reply_margin_dev is None:
            self._reply_margin_dev = src.to(self.device)
        else:
            self._reply_margin_dev.copy_(src)

    def _forward_fused(self, planes, pol_out=None, val_out=None, precision=None):
        """Fused trunk + head convs in one HIP kernel, then the dense layers (model.py:44-48,56-61)
        in one launch per head (csrc/heads.hpp), written straight into the caller's buffers."""
        _, hp = self._run_fused(planes, precision=precision)
        b = hp.shape[0]
        want_value = not (pol_out is not None and val_out is None)   # S1 evaluations only choose the reply
        p = pol_out if pol_out is not None else torch.empty((b, N_POLICY), dtype=torch.float32, device=self.device)
        v = None
        if want_value:
            v = val_out if val_out is not None else torch.empty((b,), dtype=torch.float32, device=self.device)
        _lib.heads_forward(hp, b, *self._dense_images(), p, v, self._heads_scratch(b))
        return p, v

    def _dense_images(self):
        """The dense layers of the two heads as the crl_heads_forward* entry points take them, in their order."""
        return self._pol_wp, self._pol_bias, self._val_w1p, self._val_b1, self._val_w2

    def _heads_scratch(self, n_boards):
        """Slice statistics of the small-batch heads (crl_heads_forward: float [n_boards][16]); one
        buffer per batch size, kept, so that captured graphs hold a stable address."""
        buf = self._scratch.get(n_boards)
        if buf is None:
            buf = self._scratch[n_boards] = torch.zeros((n_boards, 16), dtype=torch.float32, device=self.device)
        return buf

    @property
    def accepts_legal_labels(self):
        """The HIP heads can write just the probabilities of a position's legal moves
        (crl_heads_forward_legal): the engine then never materialises the 1968-vectors."""
        return bool(self.fused)

    @torch.no_grad()
    def forward_legal_into(self, planes, labels_ptr, counts_ptr, priors_out, val_out, stats_out=None):
        """Evaluate and write, per board, the policy at the labels listed in the device arrays
        ``labels_ptr`` (uint16 [B,256]) / ``counts_ptr`` (int32 [B]) into ``priors_out`` (fp32
        [B,256]) and the value into ``val_out`` (fp32 [B], or None: S1 evaluations need no value).
        With ``stats_out`` (fp32 [B,16]; only for batches ``raw_priors_supported``) the rows receive
        the LOGITS and ``stats_out`` the softmax statistics of the label slices: the search kernels
        normalise on read (CRL_POLICY_LEGAL_RAW) and the heads' normalising pass is not launched."""
        if not self.fused:
            raise _lib.HipLibraryError("forward_legal_into needs the fused HIP tower")

        def heads(hp):
            if stats_out is None:
                _lib.heads_forward_legal(hp, hp.shape[0], *self._dense_images(), labels_ptr, counts_ptr, priors_out, val_out,
                                         self._heads_scratch(hp.shape[0]))
            else:
                _lib.heads_forward_legal_raw(hp, hp.shape[0], *self._dense_images(), labels_ptr, counts_ptr, priors_out,
                                             val_out, stats_out)

        if self.precision == "hybrid" and val_out is None and planes.shape[0] >= self.HYBRID_MIN_BOARDS:
            # S1: the reply is an argmax over the legal labels.  Single-MFMA trunk for every board; the boards
            # whose two best legal moves are closer than the margin are listed on the device and evaluated again
            # by the split-precision kernels (a grid for the whole batch whose surplus workgroups exit at once);
            # the heads then run over all rows again (16 us) -- listed boards now carry fp32-grade activations
            if planes.dtype != torch.int64:
                raise _lib.HipLibraryError("the hybrid mode evaluates plane bitboards (the engine's default input)")
            planes_p, hp_full = self._run_fused_padded(planes, "f16")
            b, bp = planes.shape[0], planes_p.shape[0]
            heads(hp_full[:b])
            lst = self._fallback.get(bp)
            if lst is None:
                lst = self._fallback[bp] = torch.zeros(_lib.LIST_HEADER + bp, dtype=torch.int32, device=self.device)
            _lib.reply_margin(priors_out, counts_ptr, b, self._reply_margin_dev, 0 if stats_out is None else 1, lst)
            ws = self._trunk_workspace(bp)
            ev = self._trunk_event("f16x3 indexed")
            _lib.trunk_forward_indexed(self.filters, planes_p, self._wtiles3, self._wbias, bp, self.blocks, self._head_w,
                                       self._head_b, hp_full, lst, ws, ws.numel() if ws is not None else 0)
            if ev is not None:
                ev[2].record()
            heads(hp_full[:b])
            return
        _, hp = self._run_fused(planes)
        heads(hp)

    def prepare(self, n_boards):
        """Allocate what an evaluation of ``n_boards`` keeps between calls (the hybrid mode's device list with its
        running counter) NOW: LockstepEngine calls this before it captures its hipGraph, so that no buffer
        is created -- and zero-filled at every replay -- inside the captured step."""
        bp = (int(n_boards) + 3) // 4 * 4
        if self.fused and bp not in self._fallback:
            self._fallback[bp] = torch.zeros(_lib.LIST_HEADER + bp, dtype=torch.int32, device=self.device)
        if self.fused:
            self._heads_scratch(int(n_boards))
            if self._trunk_mode() == "f16x3":
                self._trunk_workspace(bp)

    def fallback_boards(self):
        """hybrid: total number of S1 boards evaluated a second time since the model was built (sum over
        the batch sizes it has served; a device-to-host read of the lists' 64-bit counters)."""
        return int(sum(int(v[2:4].view(torch.int64).item()) for v in self._fallback.values()))

    def raw_priors_supported(self, n_boards):
        """Whether a batch of ``n_boards`` is served by the sliced heads, i.e. may leave the softmax
        normalisation to the search kernels (``forward_legal_into(..., stats_out=...)``)."""
        return bool(self.fused and _lib.heads_raw_supported(n_boards))

    @torch.no_grad()
    def forward_into(self, planes, pol_out, val_out):
        """Evaluate and write policy [B,1968] / value [B] into existing fp32 tensors."""
        if self.fused:
            self._forward_fused(planes, pol_out, val_out)
        else:
            p, v = self(planes)
            pol_out.copy_(p)
            if val_out is not None:
                val_out.copy_(v)

    def load_weights(self, weights_path):
        """model.py:77-78.  ``.h5`` = a Keras weight file (chessrl_amd/keras_h5.py), else ``.npz``."""
        self.load_dict(_read_weights(weights_path))
        self._trainer = None                     # optimizer state belongs to the old weights

    def reset_optimizer(self):
        """Forget the Adam moments and step count (a fresh ``compile`` in the reference: every
        ``train_model_job`` of selfplay.py:98-108 runs in a new process with a new optimizer)."""
        self._trainer = None

    def train_generator(self, generator, epochs=1, logdir=None, val_gen=None, verbose=0):
        """model.py:83-99 (``fit_generator`` over a ``DataGameSequence``).  Where the reference
        attaches a TensorBoard callback, ``logdir`` receives one JSON line per epoch in
        ``train_log.jsonl``.  Afterwards the inference path (folded BN, fused-trunk tiles) is rebuilt
        from the trained weights."""
        if not self.compiled:
            raise RuntimeError("ChessModel was built with compile_model=False")
        from .train import Trainer
        if self._trainer is None:
            self._trainer = Trainer(self.weights, self.device)
        log = None
        if logdir is not None:
            import json
            import os
            os.makedirs(logdir, exist_ok=True)

            def log(summary):
                with open(os.path.join(logdir, "train_log.jsonl"), "a") as f:
                    f.write(json.dumps(summary) + "\n")
        history = self._trainer.fit_generator(generator, epochs=epochs, val_gen=val_gen,
                                              verbose=verbose, log=log)
        self.load_dict(self._trainer.weights())
        return history

    def save_weights(self, weights_path):
        """model.py:80-81."""
        if str(weights_path).endswith((".h5", ".hdf5")):
            from .keras_h5 import save_keras_h5
            save_keras_h5(self.weights, weights_path)
        else:
            np.savez(weights_path, **self.weights)

    @property
    def accepts_bitplanes(self):
        """The fused HIP trunk expands the encoder's 128 plane bitboards itself (engine.py)."""
        return self.fused

    @torch.no_grad()
    def __call__(self, planes):
        if self.fused:
            return self._forward_fused(planes)
        if planes.dtype == torch.int64:
            raise ValueError("plane bitboards are only understood by the fused HIP trunk")
        x = planes.to(self.net.stem.weight.dtype).permute(0, 3, 1, 2)   # NHWC memory viewed as NCHW
        return self.net(x)

    @torch.no_grad()
    def predict(self, inp):
        a = torch.as_tensor(np.asarray(inp))
        x = torch.zeros((a.shape[0], 8, 8, PAD_PLANES), dtype=self.dtype, device=self.device)
        x[..., :IN_PLANES] = a.to(self.device, self.dtype)
        p, v = self(x)
        return [p.cpu().numpy(), v.cpu().numpy()[:, None]]

    def macs_per_eval(self):
        """MACs of one forward."""
        f, b = self.filters, self.blocks
        return 73152 * f + 1152 * f * f * b + 192 * f + 268544
