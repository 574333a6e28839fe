"""GPU parity: encoder, PUCT select/expand/backup and the tower vs the CPU oracle.

Bars: encoder planes and every search statistic (visit counts, value sums as
float64 bit patterns, priors, moves, stored replies) bit-exact; tower outputs
within 1e-3 of the fp32 oracle (the tolerance BASELINE.json's north_star states).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import encoder_oracle, mcts_oracle, tower_oracle
from oracle.chess_oracle import OracleGame, move_to_uci, uci_to_move
from oracle.fakenet import FakeNet

pytestmark = pytest.mark.gpu


def random_prefix_games(n, max_len, seed):
    """n oracle games after seeded random legal move prefixes (lengths spread over 0..max_len)."""
    rng = np.random.default_rng(seed)
    games = []
    for i in range(n):
        g = OracleGame()
        want = int(round(i * max_len / max(1, n - 1)))
        while len(g) < want and g.get_result() is None:
            lm = g.legal_move_ids()
            g.move(move_to_uci(lm[int(rng.integers(len(lm)))]))
        if g.get_result() is not None:           # keep only running games
            g = OracleGame()
        games.append(g)
    return games


def move_ids(g):
    return [g.board.move_stack[i].m for i in range(len(g))]


def test_encoder_matches_oracle():
    from chessrl_amd.engine import LockstepEngine
    games = random_prefix_games(64, 90, seed=7)
    eng = LockstepEngine(lambda p: None, n_games=64, max_sims=4, use_graph=False)
    eng.load_moves([move_ids(g) for g in games])
    eng.ctx.encode(eng.planes_s1.data_ptr())
    eng.ctx.sync()
    got = eng.planes_s1.float().cpu().numpy()
    for i, g in enumerate(games):
        exp = encoder_oracle.get_game_state(g)
        assert exp.shape == (8, 8, 127)
        assert np.array_equal(got[i, :, :, :127], exp), (i, len(g))
        assert not got[i, :, :, 127].any()
    # hand-derived known answers: start position
    s = got[0]
    assert len(games[0]) == 0
    assert s[6, :, 7 + 1].all() and s[1, :, 1].all()          # white pawns row 6, black pawns row 1
    assert s[:, :, 126].all() and not s[:, :, 14:126].any()   # white to move, no history
    eng.close()


def test_encoder_matches_the_reference_encoder_vectors(golden_dir):
    """tests/golden/encoder_cases.json (the reference's own get_game_state, see
    tests/test_oracle_chess.py) through the HIP encoder: drop-in Games built from FEN + moves,
    copied into an engine, crl_encode in both plane formats."""
    import json
    import os
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.game import Game
    cases = json.load(open(os.path.join(golden_dir, "encoder_cases.json")))["cases"]
    games = []
    for c in cases:
        g = Game(board=c["fen"]) if c["fen"] else Game()
        for u in c["prefix_moves"]:
            assert g.move(u), u
        games.append(g)
    n = (len(games) + 3) // 4 * 4
    for bits in (False, True):
        eng = LockstepEngine(lambda p: None, n_games=n, max_sims=4, use_graph=False, bitplanes=bits)
        eng.load_games(games)
        eng.ctx.encode(eng.planes_s1.data_ptr())
        eng.ctx.sync()
        if bits:
            raw = eng.planes_s1.cpu().numpy().view(np.uint64)                 # [n][128] plane bitboards
            got = np.zeros((n, 8, 8, 128), np.float32)
            for ch in range(128):
                for sq in range(64):
                    got[:, 7 - sq // 8, sq % 8, ch] = (raw[:, ch] >> np.uint64(sq)) & np.uint64(1)
        else:
            got = eng.planes_s1.float().cpu().numpy()
        for i, c in enumerate(cases):
            ref = np.unpackbits(np.frombuffer(bytes.fromhex(c["planes_packbits_hex"]), np.uint8))[:8 * 8 * 127]
            assert np.array_equal(got[i, :, :, :127].reshape(-1), ref.astype(np.float32)), (bits, i)
            assert not got[i, :, :, 127].any()
        eng.close()
    for g in games:
        g.free()


@pytest.mark.parametrize("mode", ["nep50", "legacy"])
@pytest.mark.parametrize("shift,quant,sims,graph", [(24, 0, 60, False), (29, 0, 150, True),
                                                    (33, 12, 150, True), (31, 16, 90, False)])
def test_search_matches_oracle(mode, shift, quant, sims, graph):
    from chessrl_amd.engine import LockstepEngine
    G = 12
    games = random_prefix_games(G, 60, seed=100 + shift)
    net = FakeNet(seed=5 + shift, prior_shift=shift, quant=quant)
    eng = LockstepEngine(net.to("cuda:0"), n_games=G, max_sims=sims, numpy_promotion=mode,
                         use_graph=graph)
    eng.load_moves([move_ids(g) for g in games])
    eng.search(sims)
    rc = eng.root_children()
    cnt = eng.ctx.counters()
    assert cnt["sims"] == G * sims
    for i, g in enumerate(games):
        agent = mcts_oracle.OracleAgent(net)
        r = mcts_oracle.search(g, agent, sims, noise=False, mode=mode)
        n = rc["nchild"][i]
        assert n == len(r.visits), i
        assert list(rc["visits"][i, :n]) == r.visits, (i, mode)
        assert rc["root_visits"][i] == r.root_visits
        assert [move_to_uci(m) for m in rc["moves"][i, :n]] == r.child_moves
        exp_rep = [0xFFFF if u == "00000" else uci_to_move(u) for u in r.child_replies]
        assert list(rc["replies"][i, :n]) == exp_rep
        assert np.array_equal(rc["values"][i, :n].view(np.uint64),
                              np.array(r.values, dtype=np.float64).view(np.uint64)), i
        assert np.array_equal(rc["priors"][i, :n], np.array(r.priors, dtype=np.float32)), i
    eng.close()


def long_quiet_games(n, seed=77):
    """n running games of 120, 134, ... plies that shuffle pieces (non-pawn, non-capturing moves preferred): large
    halfmove clocks.  Game i does not depend on n."""
    rng = np.random.default_rng(seed)
    games = []
    while len(games) < n:
        g = OracleGame()
        want = 120 + 14 * len(games)
        while len(g) < want and g.get_result() is None:
            b = g.board_at(0)
            occ = 0
            for t in range(6):
                occ |= int(b.bb[t])
            lm = g.legal_move_ids()
            quiet = [m for m in lm if not (int(b.bb[0]) >> (m & 63)) & 1 and not (occ >> ((m >> 6) & 63)) & 1]
            pool = quiet if quiet and rng.random() < 0.97 else lm
            g.move(move_to_uci(pool[int(rng.integers(len(pool)))]))
        if g.get_result() is None:
            games.append(g)
    return games


def test_search_on_long_games_with_high_halfmove_clocks():
    """Roots 120-260 plies deep: large halfmove clocks, so the tree meets the fifty-move claim
    (terminal nodes inside the tree) and runs the repetition scan over tree path + game ring."""
    from chessrl_amd.engine import LockstepEngine
    G, sims = 10, 120
    games = long_quiet_games(G)
    clocks = [(int(g.board_at(0).state) >> 12) & 255 for g in games]
    assert max(clocks) >= 40
    net = FakeNet(seed=41, prior_shift=31)
    eng = LockstepEngine(net.to("cuda:0"), n_games=G, max_sims=sims)
    eng.load_moves([move_ids(g) for g in games])
    eng.search(sims)
    rc = eng.root_children()
    hits = eng.ctx.counters()["terminal_hits"]
    for i, g in enumerate(games):
        r = mcts_oracle.search(g, mcts_oracle.OracleAgent(net), sims, noise=False)
        n = rc["nchild"][i]
        assert list(rc["visits"][i, :n]) == r.visits, (i, len(g), clocks[i])
        assert np.array_equal(rc["values"][i, :n].view(np.uint64),
                              np.array(r.values, dtype=np.float64).view(np.uint64)), i
    print("long-game search: clocks", clocks, "terminal hits", hits)
    eng.close()


def test_search_across_the_fifty_move_claim_and_mates():
    """Set-up positions whose trees contain fifty-move claims, stalemates and checkmates after
    our move (state = S1) and after the reply (state = S2)."""
    from chessrl_amd.engine import LockstepEngine
    from oracle.chess_oracle import board_from_fen, board_to_array
    fens = ["8/8/8/4k3/8/8/4K3/7R w - - 96 80",          # claims at clock 100 two plies down
            "8/8/8/4k3/8/8/4K3/7R b - - 97 80",
            "7k/8/5KQ1/8/8/8/8/8 w - - 0 1",              # mates and stalemates one ply away
            "6k1/5ppp/8/8/8/8/5PPP/R5K1 w - - 0 1",        # back-rank mate available
            "k7/2Q5/1K6/8/8/8/8/8 b - - 10 1",             # black to move, nearly stalemated
            "r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1"]        # castling both sides in the tree
    G, sims = len(fens), 90
    games = [OracleGame(board=board_from_fen(f)) for f in fens]
    net = FakeNet(seed=13, prior_shift=30)
    eng = LockstepEngine(net.to("cuda:0"), n_games=G, max_sims=sims)
    eng.ctx.set_positions(np.stack([board_to_array(board_from_fen(f)) for f in fens]))
    eng.search(sims)
    rc = eng.root_children()
    cnt = eng.ctx.counters()
    assert cnt["terminal_hits"] > 0
    for i, g in enumerate(games):
        if g.get_result() is not None:
            assert rc["nchild"][i] == 0
            continue
        r = mcts_oracle.search(g, mcts_oracle.OracleAgent(net), sims, noise=False)
        n = rc["nchild"][i]
        assert list(rc["visits"][i, :n]) == r.visits, fens[i]
        assert [move_to_uci(m) for m in rc["moves"][i, :n]] == r.child_moves
        exp_rep = [0xFFFF if u == "00000" else uci_to_move(u) for u in r.child_replies]
        assert list(rc["replies"][i, :n]) == exp_rep, fens[i]
        assert np.array_equal(rc["values"][i, :n].view(np.uint64),
                              np.array(r.values, dtype=np.float64).view(np.uint64)), fens[i]
    eng.close()


def test_search_from_the_218_move_position_fills_the_edge_pool():
    """A root with 218 children (the worst case the edge pool ECAP = N x 218 is sized for): 240
    simulations expand all of them, apply the priors and descend again; children hold up to 80+
    replies' worth of edges each."""
    from chessrl_amd.engine import LockstepEngine
    from oracle.chess_oracle import board_from_fen, board_to_array
    from tests.util import MAX_MOVES_FEN
    sims = 240
    g = OracleGame(board=board_from_fen(MAX_MOVES_FEN))
    net = FakeNet(seed=3, prior_shift=30)
    eng = LockstepEngine(net.to("cuda:0"), n_games=4, max_sims=sims)
    eng.ctx.set_positions(np.stack([board_to_array(board_from_fen(MAX_MOVES_FEN))] * 4))
    eng.search(sims)
    rc = eng.root_children()
    r = mcts_oracle.search(g, mcts_oracle.OracleAgent(net), sims, noise=False)
    for i in (0, 3):
        assert rc["nchild"][i] == 218 == len(r.visits)
        assert list(rc["visits"][i, :218]) == r.visits
        assert np.array_equal(rc["values"][i, :218].view(np.uint64),
                              np.array(r.values, dtype=np.float64).view(np.uint64))
        assert np.array_equal(rc["priors"][i, :218], np.array(r.priors, dtype=np.float32))
    eng.close()


def test_search_then_advance_matches_oracle_game():
    """Three full moves of selfplay.play_game (search -> choose -> two pushes), noise off."""
    from chessrl_amd.engine import LockstepEngine, compute_policy
    G, sims = 6, 70
    net = FakeNet(seed=11, prior_shift=30)
    games = random_prefix_games(G, 30, seed=3)
    eng = LockstepEngine(net.to("cuda:0"), n_games=G, max_sims=sims)
    eng.load_moves([move_ids(g) for g in games])
    agent = mcts_oracle.OracleAgent(net)
    for _ in range(3):
        eng.search(sims)
        rc = eng.root_children()
        _, plies, _ = eng.ctx.records(with_moves=False)
        chosen = np.full(G, -1, dtype=np.int32)
        for i in range(G):
            n = rc["nchild"][i]
            if n:
                pol = compute_policy(rc["visits"][i, :n], rc["root_visits"][i], plies[i], noise=False)
                chosen[i] = int(np.argmax(pol))
        bm, am = eng.advance(chosen)
        for i, g in enumerate(games):
            if g.get_result() is not None:
                assert chosen[i] == -1
                continue
            r = mcts_oracle.search(g, agent, sims, noise=False)
            assert r.chosen == chosen[i]
            g.move(r.moves[0])
            g.move(r.moves[1])                     # selfplay.py:77-78 (first may fail silently)
        moves, plies, res = eng.ctx.records()
        for i, g in enumerate(games):
            assert plies[i] == len(g)
            assert list(moves[i, :plies[i]]) == move_ids(g)
            assert res[i] == (2 if g.get_result() is None else g.get_result())
    eng.close()


# Tower bar (north_star): |policy| and |value| within 1e-3 of the fp32 reference on the same weights.
# The full-size statement -- >= 4096 real self-play positions, every tower size, default-init and
# SHARP weights, what precision="auto" picks -- is tests/test_gpu_tower.py.  Here: 30 boards (not a
# multiple of 4: the padding path) through the engine's in-place path and the Keras-style predict()
# surface, in f32 (PyTorch-ROCm) and f16 (fused trunk), on the same two kinds of weights.  (Round 2
# had a "trained" leg: 3 epochs on 32 games give a collapsed net -- uniform policy, value ~ 0 -- on
# which any error is invisible; it is replaced by the calibrated sharp net.)
def _sharp_weights(blocks, filters):
    games = random_prefix_games(64, 120, seed=19)
    planes = np.stack([encoder_oracle.get_game_state(g) for g in games])
    return tower_oracle.calibrated_weights(blocks, filters, planes, seed=7)


def _tower_errors(w, dtype, n_boards=30, precision="auto"):
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.model import ChessModel
    model = ChessModel(weights=w, dtype=getattr(torch, dtype), precision=precision)
    games = random_prefix_games(n_boards, 80, seed=9)           # 30: not a multiple of 4 (padding path)
    eng = LockstepEngine(model, n_games=n_boards, max_sims=4, use_graph=False)
    eng.load_moves([move_ids(g) for g in games])
    eng.ctx.encode(eng.planes_s1.data_ptr())
    pol, val = model(eng.planes_s1)
    planes = np.stack([encoder_oracle.get_game_state(g) for g in games])
    epol, eval_ = tower_oracle.forward(w, planes)
    dp = (pol.cpu() - epol).abs().max().item()
    dv = (val.cpu() - eval_).abs().max().item()
    return model, eng, planes, (pol, val), (epol, eval_), dp, dv


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("weights", ["keras_default_init", "sharp"])
@pytest.mark.parametrize("blocks,filters", [(2, 32), (6, 64), (10, 128), (20, 256)])
def test_tower_within_1e3_of_fp32_oracle(blocks, filters, weights, dtype):
    w = (tower_oracle.init_weights(blocks, filters, seed=4) if weights == "keras_default_init"
         else _sharp_weights(blocks, filters))
    model, eng, planes, (pol, val), (epol, eval_), dp, dv = _tower_errors(w, dtype)
    assert model.fused == (filters in (64, 128, 256) and dtype == "float16")
    if model.fused and weights == "sharp":       # precision="auto": split arithmetic wherever one MFMA per product is not enough
        assert model.precision == "hybrid"
    if weights == "sharp":
        assert float(epol.max()) > 0.2 and float(eval_.abs().max()) > 0.5
    print("tower %dx%d %s %s fused=%d: max|dpolicy|=%.3g max|dvalue|=%.3g" %
          (blocks, filters, weights, dtype, model.fused, dp, dv))
    assert dp <= 1e-3 and dv <= 1e-3, (dp, dv)
    # the engine's in-place path and the Keras-style predict() surface give the same numbers
    model.forward_into(eng.planes_s1, eng.pol_s1, eng.val_s2)
    if model.fused:       # the HIP trunk is run-to-run deterministic; MIOpen's solver choice is not
        assert torch.equal(eng.pol_s1, pol) and torch.equal(eng.val_s2, val)
    else:
        assert (eng.pol_s1 - pol).abs().max() <= 1e-3 and (eng.val_s2 - val).abs().max() <= 1e-3
    kp, kv = model.predict(planes)
    assert np.abs(kp - epol.numpy()).max() <= 1e-3 and np.abs(kv[:, 0] - eval_.numpy()).max() <= 1e-3
    assert kp.shape == (30, 1968) and kv.shape == (30, 1)
    eng.close()


# NOT the 1e-3 bar: a stress case outside anything training produces.  BatchNorm statistics drawn
# at random (gamma, var in [0.5, 1.5], no weight decay) give every layer a gain of up to 2x, so a
# 20-block tower amplifies the 11-bit rounding of its fp16 operands ~60x.  The bounds below are the
# measured errors of the fused fp16 trunk on MI355X with head-room; they document how far fp16
# operands can drift on adversarial statistics (PyTorch's fp16 convolutions, which also round
# every layer OUTPUT to fp16, are 2-3x worse) and catch a regression of the BN folding.
STRESS_FP16_BOUND = {
    # (blocks, filters): (policy, value)            measured
    (6, 64): (1e-3, 1e-3),                           # 3e-7
    (10, 128): (1e-3, 3e-3),                         # 1.8e-3
    (20, 128): (5e-3, 1e-2),                         # 2.8e-3 / 6.8e-3
    (20, 256): (1e-3, 5e-3),                         # 2.1e-3
}


@pytest.mark.parametrize("blocks,filters", sorted(STRESS_FP16_BOUND))
def test_fp16_trunk_drift_under_random_batchnorm_statistics_is_bounded(blocks, filters):
    w = tower_oracle.init_weights(blocks, filters, seed=4, randomize_bn=True)
    model, eng, _, _, _, dp, dv = _tower_errors(w, "float16", precision="f16")
    ptol, vtol = STRESS_FP16_BOUND[(blocks, filters)]
    print("stress %dx%d: max|dpolicy|=%.3g max|dvalue|=%.3g (bounds %g / %g)" % (blocks, filters, dp, dv, ptol, vtol))
    assert model.fused and model.precision == "f16" and dp <= ptol and dv <= vtol
    eng.close()
    # the split mode of the fused trunk meets the bar on the same statistics
    model, eng, _, _, _, dp, dv = _tower_errors(w, "float16", precision="f16x3")
    assert model.fused and model.precision == "f16x3" and dp <= 1e-3 and dv <= 1e-3
    eng.close()
    # the f32 path stays within 1e-3 (measured 1e-5) on the same statistics
    model, eng, _, _, _, dp, dv = _tower_errors(w, "float32")
    assert dp <= 1e-3 and dv <= 1e-3
    eng.close()


@pytest.mark.parametrize("n_boards", [8, 516])
@pytest.mark.parametrize("filters", [64, 128, 256])
def test_fused_trunk_matches_pytorch_trunk_activations(filters, n_boards):
    """The fused HIP trunk's fp32 activations vs the fp32 oracle trunk, element by element, in the
    precision mode "f16" by name (fp16 operands: 4e-3; tests/test_gpu_trunk_arith.py holds every kernel
    to its own arithmetic far tighter).
    8 boards run the half-size workgroup geometry (small batches), 516 the full-size one."""
    _fused_trunk_vs_pytorch_trunk(filters, n_boards, "f16")


@pytest.mark.parametrize("n_boards", [8, 516])
@pytest.mark.parametrize("filters", [64, 128, 256])
def test_fused_split_trunk_matches_pytorch_trunk_activations(filters, n_boards):
    """As above in the precision mode "f16x3" (hi + lo pairs, three MFMAs per product): 2e-5."""
    _fused_trunk_vs_pytorch_trunk(filters, n_boards, "f16x3")


def _fused_trunk_vs_pytorch_trunk(filters, n_boards, precision):
    from chessrl_amd.model import ChessModel
    w = tower_oracle.init_weights(3, filters, seed=11, randomize_bn=True)
    model = ChessModel(weights=w, precision=precision)
    assert model.precision == precision
    ref = ChessModel(weights=w, dtype=torch.float32, fused=False)
    rng = np.random.default_rng(3)
    planes = torch.zeros((n_boards, 8, 8, 128), dtype=torch.float16, device="cuda:0")
    planes[..., :127] = torch.from_numpy((rng.random((n_boards, 8, 8, 127)) < 0.15).astype(np.float16)).cuda()
    trunk, heads = model._run_fused(planes, want_trunk=True)
    with torch.no_grad():
        exp = ref.net.trunk(planes.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    scale = exp.abs().max().item()
    tol = 4e-3 if precision == "f16" else 2e-5                          # fp16 operands / three MFMAs per product
    assert (trunk - exp).abs().max().item() <= tol * scale              # fp32 accumulate
    assert heads.shape == (n_boards, 192) and (heads >= 0).all()
    if n_boards == 8:
        # both geometries accumulate every output in the same order: identical trunk bits
        from chessrl_amd import _lib
        with _lib.trunk_set_small_batch(0):
            trunk_big, heads_big = model._run_fused(planes, want_trunk=True)
        assert torch.equal(trunk, trunk_big)
        assert (heads - heads_big).abs().max().item() <= 1e-5 * max(1.0, heads.abs().max().item())


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("n_boards", [5, 64, 1000])
def test_mfma_dense_heads_match_the_fp32_dense_layers(n_boards, sliced):
    """crl_heads_forward (csrc/heads.hpp: Dense(1968)+softmax, Dense(256)-relu-Dense(1)-tanh on
    (hi, lo)-split fp16 MFMAs) against the same layers in torch fp32 on the same head activations,
    incl. batches that are not a multiple of the 16-board blocks and the policy-only call; in the
    one-pass form and (scratch given: batches up to 1024 boards) as label slices + normalising pass
    with the value head riding along."""
    from chessrl_amd import _lib
    from chessrl_amd.model import ChessModel
    w = tower_oracle.init_weights(2, 64, seed=21, randomize_bn=True)
    rng = np.random.default_rng(n_boards)
    w["policy.dense.bias"] = rng.normal(0, 0.5, 1968).astype(np.float32)      # non-trivial biases
    w["value.dense1.bias"] = rng.normal(0, 0.2, 256).astype(np.float32)
    w["value.dense2.bias"] = np.array([0.3], np.float32)
    model = ChessModel(weights=w)
    hp = torch.from_numpy(np.abs(rng.normal(0, 1.5, (n_boards, 192))).astype(np.float32)).cuda()
    hp[:, ::7] = 0                                                              # ReLU outputs: many zeros
    n = model.net
    with torch.no_grad():
        ref_p = torch.softmax(n.policy_fc(hp[:, :128]), -1)
        ref_v = torch.tanh(n.value_fc2(F.relu(n.value_fc1(hp[:, 128:])))[:, 0])
    scratch = torch.full((n_boards + 3, 16), -7.0, device="cuda")

    def run(pol, val):
        _lib.heads_forward(hp, n_boards, model._pol_wp, model._pol_bias, model._val_w1p, model._val_b1, model._val_w2,
                           pol, val, scratch if sliced else None)
        torch.cuda.synchronize()

    pol = torch.full((n_boards + 3, 1968), -7.0, device="cuda")                 # guard rows stay untouched
    val = torch.full((n_boards + 3,), -7.0, device="cuda")
    run(pol, val)
    assert (pol[:n_boards] - ref_p).abs().max().item() <= 1e-6
    assert (val[:n_boards] - ref_v).abs().max().item() <= 1e-6
    assert (pol[:n_boards].sum(1) - 1).abs().max().item() <= 1e-5
    assert (pol[n_boards:] == -7.0).all() and (val[n_boards:] == -7.0).all()
    assert (scratch[n_boards:] == -7.0).all() and bool((scratch[:n_boards] != -7.0).all()) == sliced
    pol2 = torch.zeros_like(pol)
    run(pol2, None)                                                             # S1 evaluations: no value head
    assert torch.equal(pol2[:n_boards], pol[:n_boards])


def _bits_from_planes(planes):
    """fp16/0-1 planes [B,8,8,128] -> int64 [B,128] plane bitboards (bit sq, spatial index sq ^ 56)."""
    b = planes.shape[0]
    flat = planes.reshape(b, 64, 128).to(torch.int64)                 # [B, p, c]
    sq = torch.arange(64, device=planes.device) ^ 56                  # square of spatial index p
    w = (torch.ones(64, dtype=torch.int64, device=planes.device) << sq)
    return (flat * w.view(1, 64, 1)).sum(dim=1)                       # bit 63 wraps to the sign bit


def test_encoder_bitplane_format_holds_the_same_planes():
    """CRL_PLANES_BITS vs CRL_PLANES_F16 from the same positions (with history)."""
    from chessrl_amd.engine import LockstepEngine
    games = random_prefix_games(48, 90, seed=17)
    a = LockstepEngine(lambda p: None, n_games=48, max_sims=4, use_graph=False)
    b = LockstepEngine(lambda p: None, n_games=48, max_sims=4, use_graph=False, bitplanes=True)
    for e in (a, b):
        e.load_moves([move_ids(g) for g in games])
        e.ctx.encode(e.planes_s1.data_ptr())
        e.ctx.sync()
    assert b.planes_s1.dtype == torch.int64 and b.planes_s1.shape == (48, 128)
    assert torch.equal(_bits_from_planes(a.planes_s1), b.planes_s1)
    assert (b.planes_s1[:, 127] == 0).all()
    a.close()
    b.close()


@pytest.mark.parametrize("n_boards", [30, 516])
@pytest.mark.parametrize("filters", [64, 128, 256])
def test_fused_trunk_from_bitplanes_is_bit_identical(filters, n_boards):
    """crl_trunk_forward_bitplanes expands the bitboards on chip: same bits out as from fp16 planes."""
    from chessrl_amd.model import ChessModel
    model = ChessModel(weights=tower_oracle.init_weights(3, filters, seed=12, randomize_bn=True))
    rng = np.random.default_rng(filters + n_boards)
    planes = torch.zeros((n_boards, 8, 8, 128), dtype=torch.float16, device="cuda:0")
    planes[..., :127] = torch.from_numpy((rng.random((n_boards, 8, 8, 127)) < 0.2).astype(np.float16)).cuda()
    bits = _bits_from_planes(planes)
    t0, h0 = model._run_fused(planes, want_trunk=True)
    t1, h1 = model._run_fused(bits, want_trunk=True)
    assert torch.equal(t0, t1) and torch.equal(h0, h1)
    (p0, v0), (p1, v1) = model(planes), model(bits)
    assert torch.equal(p0, p1) and torch.equal(v0, v1)


@pytest.mark.gpu
@pytest.mark.parametrize("n_boards", [30, 516])
def test_layerwise_split_trunk_of_256_filters_both_plane_formats_trunk_output_and_batch_independence(n_boards):
    """csrc/tower_layer.hpp (256 filters, CRL_TRUNK_SPLIT: one launch per convolution, activations through the
    caller's workspace): the same bits from fp16 planes and from plane bitboards; the trunk's fp32 output and the head
    activations against the fp32 PyTorch tower at fp32-grade accuracy; and ONE arithmetic whatever the batch -- a
    board evaluated in a batch of 4 carries the bits it has in the big batch (the hybrid mode's indexed launches and
    a thinning lockstep batch rely on it)."""
    from chessrl_amd.model import ChessModel
    w = tower_oracle.init_weights(3, 256, seed=12, randomize_bn=True)
    model = ChessModel(weights=w, precision="f16x3")
    ref = ChessModel(weights=w, dtype=torch.float32, fused=False)
    rng = np.random.default_rng(256 + n_boards)
    planes = torch.zeros((n_boards, 8, 8, 128), dtype=torch.float16, device="cuda:0")
    planes[..., :127] = torch.from_numpy((rng.random((n_boards, 8, 8, 127)) < 0.2).astype(np.float16)).cuda()
    bits = _bits_from_planes(planes)
    t0, h0 = model._run_fused(planes, want_trunk=True)
    t1, h1 = model._run_fused(bits, want_trunk=True)
    assert torch.equal(t0, t1) and torch.equal(h0, h1)
    with torch.no_grad():
        exp = ref.net.trunk(planes.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    scale = exp.abs().max().item()
    assert (t0 - exp).abs().max().item() <= 2e-5 * scale                # three MFMAs per product: fp32-grade
    _, h_none = model._run_fused(bits)                                  # without the trunk output: same head rows
    assert torch.equal(h_none, h0)
    for first in (0, 4 * ((n_boards - 4) // 4)):
        _, hs = model._run_fused(bits[first:first + 4].contiguous())
        assert torch.equal(hs, h0[first:first + 4])
    (p0, v0), (p1, v1) = model(planes), model(bits)
    assert torch.equal(p0, p1) and torch.equal(v0, v1)


@pytest.mark.gpu
@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("n_boards", [5, 64, 1000])
def test_legal_priors_head_writes_the_full_policy_at_the_listed_labels(n_boards, sliced):
    """crl_heads_forward_legal: priors[b][j] == policy[b][labels[b][j]] bit for bit for j < counts[b]
    (0, 1, typical and the maximum 218 labels per board), nothing written past the count."""
    from chessrl_amd import _lib
    from chessrl_amd.model import ChessModel
    model = ChessModel(weights=tower_oracle.init_weights(2, 64, seed=22, randomize_bn=True))
    rng = np.random.default_rng(100 + n_boards)
    hp = torch.from_numpy(np.abs(rng.normal(0, 1.5, (n_boards, 192))).astype(np.float32)).cuda()
    counts = rng.integers(0, 60, n_boards).astype(np.int32)
    counts[:4] = [0, 1, 218, 35][:min(4, n_boards)]
    labels = np.zeros((n_boards, 256), np.uint16)
    for b in range(n_boards):
        labels[b, :counts[b]] = rng.permutation(1968)[:counts[b]]
    lab_d, cnt_d = torch.from_numpy(labels.view(np.int16)).cuda(), torch.from_numpy(counts).cuda()
    args = (hp, n_boards, model._pol_wp, model._pol_bias, model._val_w1p, model._val_b1, model._val_w2)
    pol = torch.zeros((n_boards, 1968), device="cuda")
    val = torch.zeros((n_boards,), device="cuda")
    scratch = torch.zeros((n_boards, 16), device="cuda")
    sc = scratch if sliced else None                     # both calls in the same form: identical values
    _lib.heads_forward(*args, pol, val, sc)
    pri = torch.full((n_boards + 2, 256), -7.0, device="cuda")
    val2 = torch.full((n_boards + 2,), -7.0, device="cuda")
    _lib.heads_forward_legal(*args, lab_d, cnt_d, pri, val2, sc)
    torch.cuda.synchronize()
    pol, pri = pol.cpu().numpy(), pri.cpu().numpy()
    for b in range(n_boards):
        n = counts[b]
        assert np.array_equal(pri[b, :n].view(np.uint32), pol[b, labels[b, :n]].view(np.uint32)), b
        assert (pri[b, n:] == -7.0).all()
    assert (pri[n_boards:] == -7.0).all()
    assert torch.equal(val2[:n_boards], val) and (val2[n_boards:] == -7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("sims,graph", [(40, False), (130, True)])
def test_search_with_legal_priors_is_identical_to_search_with_full_policies(sims, graph):
    """CRL_POLICY_LEGAL (the heads write only the legal moves' probabilities, the search kernels
    publish the label lists) and CRL_POLICY_LEGAL_RAW (the heads leave logits + slice statistics and
    the search kernels normalise on read: no normalising pass) against CRL_POLICY_FULL on the same
    games: same trees, bit for bit, through replies, terminal children, finished roots, and a second
    move after advance."""
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.model import ChessModel
    model = ChessModel(blocks=2, filters=64, seed=3)
    games = random_prefix_games(24, 70, seed=29)
    out = []
    for legal, raw in ((False, False), (True, False), (True, None)):
        eng = LockstepEngine(model, n_games=24, max_sims=sims, legal_priors=legal, use_graph=graph, raw_priors=raw)
        assert eng.legal_priors == legal and eng.raw_priors == (raw is None)
        eng.load_moves([move_ids(g) for g in games])
        eng.search(sims)
        first = eng.root_children()
        chosen = np.where(first["nchild"] > 0, np.maximum(first["visits"].argmax(1), 0), -1).astype(np.int32)
        bm, am = eng.advance(chosen)
        eng.search(sims)
        out.append((first, bm, am, eng.root_children(), eng.ctx.counters()))
        eng.close()
    (a1, abm, aam, a2, ac) = out[0]
    for (b1, bbm, bam, b2, bc) in out[1:]:
        for a, b in ((a1, b1), (a2, b2)):
            assert np.array_equal(a["nchild"], b["nchild"]) and np.array_equal(a["visits"], b["visits"])
            assert np.array_equal(a["values"].view(np.uint64), b["values"].view(np.uint64))
            assert np.array_equal(a["priors"].view(np.uint32), b["priors"].view(np.uint32))
            assert np.array_equal(a["replies"], b["replies"]) and np.array_equal(a["moves"], b["moves"])
        assert np.array_equal(abm, bbm) and np.array_equal(aam, bam)
        assert {k: int(v) for k, v in ac.items()} == {k: int(v) for k, v in bc.items()}
    assert LockstepEngine(model, n_games=4, max_sims=2).legal_priors      # the default for the HIP heads


def test_search_with_the_real_tower_is_identical_in_both_plane_formats():
    from chessrl_amd.engine import LockstepEngine
    from chessrl_amd.model import ChessModel
    model = ChessModel(blocks=2, filters=64, seed=1)
    games = random_prefix_games(16, 50, seed=23)
    out = []
    for bits in (False, True):
        eng = LockstepEngine(model, n_games=16, max_sims=40, bitplanes=bits)
        assert eng.bitplanes == bits
        eng.load_moves([move_ids(g) for g in games])
        eng.search(40)
        out.append(eng.root_children())
        eng.close()
    a, b = out
    assert np.array_equal(a["nchild"], b["nchild"]) and np.array_equal(a["visits"], b["visits"])
    assert np.array_equal(a["values"].view(np.uint64), b["values"].view(np.uint64))
    assert np.array_equal(a["priors"], b["priors"]) and np.array_equal(a["replies"], b["replies"])
    assert LockstepEngine(model, n_games=4, max_sims=2).bitplanes        # the default for a fused model


def test_search_matches_committed_golden_vectors(golden_dir):
    """HIP search vs tests/golden/mcts_cases.json: the outputs of the reference's own mctree.py
    (oracle/make_golden.py), both numpy promotion modes, incl. a case where the modes differ."""
    import json
    import os
    import struct
    from chessrl_amd.engine import LockstepEngine, compute_policy
    from chessrl_amd.game import move_to_uci as mv_uci
    cases = json.load(open(os.path.join(golden_dir, "mcts_cases.json")))["cases"]
    assert any(c["differs_from_other_mode"] for c in cases)
    for c in cases:
        net = FakeNet(seed=c["net_seed"], prior_shift=c["prior_shift"], quant=c["quant"], tie=c["tie"])
        eng = LockstepEngine(net.to("cuda:0"), n_games=1, max_sims=c["sims"], numpy_promotion=c["mode"])
        eng.load_moves([[uci_to_move(u) for u in c["prefix_moves"]]])
        eng.search(c["sims"])
        rc = eng.root_children()
        n = int(rc["nchild"][0])
        assert list(rc["visits"][0, :n]) == c["visits"], (c["prefix_seed"], c["mode"])
        assert rc["root_visits"][0] == c["root_visits"]
        assert [struct.pack(">d", v).hex() for v in rc["values"][0, :n]] == c["values"]
        assert [struct.pack(">f", p).hex() for p in rc["priors"][0, :n]] == c["priors"]
        pol = compute_policy(rc["visits"][0, :n], rc["root_visits"][0], len(c["prefix_moves"]), noise=False)
        assert [struct.pack(">d", p).hex() for p in pol] == c["policy"]
        k = int(np.argmax(pol))
        assert mv_uci(rc["moves"][0, k]) == c["bm"] and mv_uci(rc["replies"][0, k]) == c["am"]
        eng.close()


@pytest.mark.parametrize("fixture,at_least", [("mcts_cases_r2.json", 30), ("mcts_cases_r5.json", 6)])
def test_dropin_tree_matches_round2_golden_vectors(golden_dir, fixture, at_least):
    """tests/golden/mcts_cases_r2.json -- the reference's own mctree.py on roots set up from FENs
    (fifty-move claims, mates / stalemates / fivefold repetition reached by our move or by the
    reply, terminal nodes re-selected, mctree.py:216-229,241-246,266-268), the two shapes of the
    ``move_stack[-2:]`` tuple when the chosen child ends the game (mctree.py:185-194), the 218-move
    root, long quiet games and 800-simulation trees -- through the drop-in objects: ``Game`` (FEN +
    pushed moves), ``Agent``, ``SelfPlayTree.search_move``.  The engine slot is a device copy of
    the Game's slot (crl_copy_game_from), so a game that did not start from the standard position
    is searched from its real root.
    tests/golden/mcts_cases_r5.json (round 5): FEN roots that claim castling rights the position does not hold --
    ``Game(board=fen)`` keeps what ``chess.Board(fen).clean_castling_rights()`` keeps, so the root counts as an
    occurrence in the fivefold rule exactly as it does for the reference."""
    import json
    import os
    import struct
    from chessrl_amd import mctree
    from chessrl_amd.agent import Agent
    from chessrl_amd.engine import compute_policy
    from chessrl_amd.game import Game
    cases = json.load(open(os.path.join(golden_dir, fixture)))["cases"]
    assert len(cases) >= at_least
    agents = {}
    for c in cases:
        key = (c["net_seed"], c["prior_shift"], c["quant"], c["mode"])
        if key not in agents:
            net = FakeNet(seed=c["net_seed"], prior_shift=c["prior_shift"], quant=c["quant"])
            agents[key] = Agent(True, model=net.to("cuda:0"), numpy_promotion=c["mode"])
        g = Game(board=c["fen"]) if c["fen"] else Game()
        for u in c["prefix_moves"]:
            assert g.move(u), (c["name"], u)
        assert g.get_result() is None and len(g) == len(c["prefix_moves"])
        tree = mctree.SelfPlayTree(g, threads=1)
        mv = tree.search_move(agents[key], max_iters=c["sims"], noise=False, ai_move=True)
        kids = tree.root.children
        tag = (c["name"], c["mode"])
        assert [k.visits for k in kids] == c["visits"], tag
        assert tree.root.visits == c["root_visits"] == c["sims"] + 1
        assert [struct.pack(">d", k.value).hex() for k in kids] == c["values"], tag
        assert [struct.pack(">f", k.prior).hex() for k in kids] == c["priors"], tag
        pol = compute_policy([k.visits for k in kids], tree.root.visits, len(g), noise=False)
        assert [struct.pack(">d", p).hex() for p in pol] == c["policy"], tag
        assert int(np.argmax(pol)) == c["chosen"]
        assert mv == (c["bm"], c["am"]), tag
        best = kids[c["chosen"]]
        assert best.state.get_result() == c["chosen_child_result"]        # Node.state, built lazily
        assert len(best.state) == c["chosen_child_stack"]
        best.state.free()
        g.free()


def test_dropin_tree_with_noise_returns_the_moves_of_the_seeded_reference(golden_dir):
    """tests/golden/mcts_noise_cases.json: the reference's search_move(noise=True) after
    np.random.seed(s).  The drop-in SelfPlayTree draws its Dirichlet noise on the host from the same
    global np.random stream (mctree.py:317-321), so with the same seed it returns the same move --
    incl. the cases where the noise overturns the visit-count argmax."""
    import json
    import os
    from chessrl_amd import mctree
    from chessrl_amd.agent import Agent
    from chessrl_amd.game import Game
    cases = json.load(open(os.path.join(golden_dir, "mcts_noise_cases.json")))["cases"]
    assert len(cases) >= 20 and any(c["chosen"] != c["chosen_without_noise"] for c in cases)
    agents = {}
    for c in cases:
        key = (c["net_seed"], c["prior_shift"], c["quant"])
        if key not in agents:
            net = FakeNet(seed=c["net_seed"], prior_shift=c["prior_shift"], quant=c["quant"])
            agents[key] = Agent(True, model=net.to("cuda:0"))
        g = Game(board=c["fen"]) if c["fen"] else Game()
        for u in c["prefix_moves"]:
            assert g.move(u), (c["name"], u)
        tree = mctree.SelfPlayTree(g, threads=1)
        np.random.seed(c["noise_seed"])
        mv = tree.search_move(agents[key], max_iters=c["sims"], noise=True, ai_move=True)
        assert [k.visits for k in tree.root.children] == c["visits"], c["name"]
        assert mv == (c["bm"], c["am"]), (c["name"], c["noise_seed"])
        g.free()


def test_f64_sqrt_and_divide_are_correctly_rounded():
    """The PUCT contract leans on IEEE float64 sqrt/divide on the device: check them against
    numpy through the tower-free path (a torch kernel uses the same hardware ops)."""
    n = torch.arange(0, 200000, dtype=torch.float64, device="cuda:0")
    assert np.array_equal(torch.sqrt(n).cpu().numpy(), np.sqrt(n.cpu().numpy()))
    rng = np.random.default_rng(0)
    a = rng.standard_normal(200000)
    b = rng.integers(1, 900, 200000).astype(np.float64)
    got = (torch.from_numpy(a).cuda() / torch.from_numpy(b).cuda()).cpu().numpy()
    assert np.array_equal(got, a / b)
