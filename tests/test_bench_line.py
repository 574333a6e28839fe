"""CPU tests of bench.py's own arithmetic (no GPU, no HIP call): the defects VERDICT r5 found on the bench
line (weak #10 - #12) and the summary of the in-graph stamps that replaced the eager step_fit (weak #5)."""
import importlib.util
import json
import os
import types
import warnings

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class FakeModel(object):
    """A hybrid model whose fall-back counter advances by ``per_step`` boards per lockstep step."""
    fused, precision, reply_margin = True, "hybrid", 1.5e-3

    def __init__(self, run, per_step):
        self.run, self.per_step = run, per_step

    def fallback_boards(self):
        return self.run.steps_run * self.per_step


class FakeRun(object):
    """SelfPlayRunner's surface as timed_window drives it; every step completes ``G`` simulations."""
    GUARD_EVERY = 8

    def __init__(self, G=64, sims=800):
        self.G, self.sims, self.steps_run, self.moves_played, self._sims_in_move = G, sims, 0, 0, None
        self.guard_seen = []
        ctx = types.SimpleNamespace(counters=lambda: {"sims": self.steps_run * self.G, "nodes": 0, "depth_sum": 0,
                                                      "branch_sum": 0, "evals": 0, "terminal_hits": 0})
        self.engine = types.SimpleNamespace(ctx=ctx, prepare_graphs=lambda n=None: None, run_steps=self._raw_steps)
        self.opening = []

    def _raw_steps(self, n):
        self.steps_run += n

    def begin_move(self):
        self._sims_in_move = 0

    def step(self):
        self.steps(1)

    def steps(self, n):
        self.guard_seen.append(self.GUARD_EVERY)
        self.steps_run += n
        self._sims_in_move = (self._sims_in_move or 0) + n

    def end_move(self):
        self.opening.append(self._sims_in_move)
        self._sims_in_move = None
        self.moves_played += self.G


@pytest.mark.parametrize("steps", [20, 40, 80, 400])
def test_hybrid_fraction_on_the_bench_line_does_not_depend_on_the_window_length(bench, steps):
    """the counter of S1 boards evaluated twice was read in front of ~409 un-timed steps and
    divided by the K timed steps' simulations: 0.508 / 0.254 / 0.127 for 20 / 40 / 80 steps.  Read inside the window
    the fraction is per_step / G whatever K is."""
    run = FakeRun(G=64)
    model = FakeModel(run, per_step=4)
    a = types.SimpleNamespace(steps=steps, sims=800, warmup=5, opening_moves=6, opening_sims=32)
    w = bench.timed_window(run, a, lambda: None, model, sync=lambda: None)
    assert run.opening[:6] == [32] * 6                       # six shortened, noisy opening moves in front of everything
    assert w["sims"] == steps * 64
    assert w["twice"] == pytest.approx(4 / 64)
    assert w["pre"] + a.warmup > 100 or steps >= 400          # (un-timed steps really ran in front of the window)
    entry = bench.hybrid_entry({}, model, w)
    assert entry == {"s1_boards_evaluated_twice": pytest.approx(4 / 64), "reply_margin": 1.5e-3}
    # the runner's precision guard is off inside the window and back afterwards
    assert set(run.guard_seen) == {0} and run.GUARD_EVERY == 8


def test_non_hybrid_windows_carry_no_hybrid_fields(bench):
    run = FakeRun()
    model = FakeModel(run, 3)
    model.precision = "f16"
    w = bench.timed_window(run, types.SimpleNamespace(steps=10, sims=800, warmup=0), lambda: None, model, sync=lambda: None)
    assert bench.hybrid_entry({"x": 1}, model, w) == {"x": 1}


def _probe_file(root, rnd, name, tower, mode_at_start=None, train=False, gph=1000.0, plies=300.0):
    d = os.path.join(root, "profiles", rnd)
    os.makedirs(d, exist_ok=True)
    body = {"games_in_lockstep": 4096, "sims_per_move": 800, "tower": tower, "rounds": [{"plies_mean": plies}],
            "games_per_hour_overall": gph, "seconds_total": 10.0, "games_total": 4096, "training_in_the_loop": train}
    if mode_at_start is not None:
        body["tower_precision_at_start"] = mode_at_start
    json.dump(body, open(os.path.join(d, name), "w"))
    return os.path.join(d, name)


def test_whole_run_figures_are_only_read_from_a_run_of_the_same_mode(bench, tmp_path):
    """the lexicographically last rolling_probe*.json won -- a hybrid run of another net beside an
    f16 headline.  Now: same configuration AND same mode, newest round first, no training runs, else None."""
    root = str(tmp_path)
    _probe_file(root, "r03", "rolling_probe.json", "10x128 f16", gph=45000.0)
    _probe_file(root, "r05", "rolling_probe.json", "10x128 f16", "f16", gph=43600.0)
    _probe_file(root, "r05", "rolling_probe_hybrid_seed1.json", "10x128 hybrid", "hybrid", gph=18300.0, plies=320.0)
    _probe_file(root, "r04", "rolling_probe_train.json", "10x128 f16", train=True, gph=99999.0)
    _probe_file(root, "r05", "rolling_probe_switched.json", "10x128 hybrid", "f16", gph=77777.0)     # changed its mode mid-run
    cfg = (4096, 800, "10x128")
    f16 = bench.tracked_whole_run(cfg, "f16", root=root)
    assert f16["games_per_hour"] == 43600.0 and f16["tower_precision"] == "f16" and "r05" in f16["source"]
    hyb = bench.tracked_whole_run(cfg, "hybrid", root=root)
    assert hyb["games_per_hour"] == 18300.0 and hyb["moves_per_game"] == 160.0
    assert bench.tracked_whole_run(cfg, "f16x3", root=root) is None
    assert bench.tracked_whole_run((4096, 800, "20x256"), "hybrid", root=root) is None
    # a newer round beats an older one whatever the file names
    _probe_file(root, "r06", "a.json", "10x128 f16", "f16", gph=50000.0)
    os.rename(os.path.join(root, "profiles", "r06", "a.json"), os.path.join(root, "profiles", "r06", "rolling_probe_a.json"))
    assert bench.tracked_whole_run(cfg, "f16", root=root)["games_per_hour"] == 50000.0


def test_whole_run_lookup_on_the_tree_itself(bench):
    """On the tracked profiles: the f16 headline of C3 reads an f16 run, a hybrid line a hybrid run, never the other's."""
    cfg = (4096, 800, "10x128")
    for mode in ("f16", "hybrid"):
        w = bench.tracked_whole_run(cfg, mode)
        assert w is not None and w["tower_precision"] == mode and w["config"] == cfg, mode
    assert bench.tracked_whole_run(cfg, "f16")["games_per_hour"] > 2 * bench.tracked_whole_run(cfg, "hybrid")["games_per_hour"]


def test_stamp_summary_telescopes_to_the_step():
    """summarise_stamps: every interval between consecutive stamps is attributed to a part, the parts add up to the
    stamped step, trunk launches are told apart by arithmetic and by phase."""
    from chessrl_amd.engine import (STAMP_GRAPH_END, STAMP_REPLIED, STAMP_S1_DONE, STAMP_SELECTED, STAMP_STEP, STAMP_TRUNK,
                                    summarise_stamps)
    t, stamps = 0.0, []

    def at(sid, dt):
        nonlocal t
        t += dt
        stamps.append((sid, t))

    b16, e16 = STAMP_TRUNK["f16"]
    b48, e48 = STAMP_TRUNK["f16x3"]
    bi, ei = STAMP_TRUNK["f16x3 indexed"]
    for g in range(3):                                   # three graph launches of two hybrid steps each
        for k in range(2):
            at(STAMP_STEP, 0.010 if k == 0 else 0.002)   # (graph launch gap / end of the previous tower_s2)
            at(STAMP_SELECTED, 0.050)
            at(b16, 0.002)
            at(e16, 9.0)
            at(bi, 0.040)                                # heads + margin kernel
            at(ei, 1.4)
            at(STAMP_S1_DONE, 0.020)
            at(STAMP_REPLIED, 0.025)
            at(b48, 0.002)
            at(e48, 24.0)
        at(STAMP_GRAPH_END, 0.030)
    out = summarise_stamps(stamps)
    assert out["steps"] == 6
    total = stamps[-1][1] - stamps[0][1]
    assert out["ms_per_step"] == pytest.approx(total / 6)
    assert sum(out["parts"].values()) == pytest.approx(out["ms_per_step"])
    assert out["trunk"]["f16"]["launch_ms"] == pytest.approx(9.0) and out["trunk"]["f16"]["launches_per_step"] == 1
    assert out["trunk"]["f16x3"]["launch_ms"] == pytest.approx(24.0)
    assert out["trunk"]["f16x3 indexed"]["launch_ms"] == pytest.approx(1.4)
    assert out["parts"]["select_expand"] == pytest.approx(0.050)
    assert out["parts"]["reply"] == pytest.approx(0.025)
    assert out["parts"]["trunk f16 (s1)"] == pytest.approx(9.0) and out["parts"]["trunk f16x3 (s2)"] == pytest.approx(24.0)
    assert out["parts"]["tower_s1 other"] == pytest.approx(0.002 + 0.040 + 0.020)
    # tower_s2's tail: the heads up to the next step's stamp (0.002, 5 of 6 steps... the last of a graph ends at GRAPH_END)
    assert out["parts"]["tower_s2 other"] == pytest.approx(0.002 + (3 * 0.002 + 3 * 0.030) / 6)
    assert out["parts"]["graph_launch_gap"] == pytest.approx(2 * 0.010 / 6)
    with pytest.raises(RuntimeError):
        summarise_stamps([(b16, 0.0), (STAMP_S1_DONE, 1.0)])          # a trunk begin without its end


def test_multiprocess_env_is_set_by_the_entry_points_not_at_import(monkeypatch):
    """importing the package must not change ROCm IPC behaviour of the host process; the multi-process
    entry points set HSA_ENABLE_IPC_MODE_LEGACY=0 themselves, an explicit setting wins."""
    import importlib
    import chessrl_amd
    monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)
    importlib.reload(chessrl_amd)
    assert "HSA_ENABLE_IPC_MODE_LEGACY" not in os.environ
    with warnings.catch_warnings():
        warnings.simplefilter("error")                    # (no GPU initialised here: no warning)
        assert chessrl_amd.multiprocess_env() == "0"
    assert os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "1")
    assert chessrl_amd.multiprocess_env() == "1"


def test_dumped_outputs_are_float_arrays_within_the_cap_and_a_fixed_sample(bench, monkeypatch, tmp_path):
    """--dump-outputs: last_step_outputs hands over float32 / float64 arrays only; a batch beyond DUMP_BYTES is cut to
    a fixed, seeded sample of games (the same rows every run, listed in ``games``) that fits the cap."""
    import numpy as np
    import torch
    G = 96
    rng = np.random.default_rng(1)
    rc = {"nchild": rng.integers(0, 40, G).astype(np.int32), "visits": rng.integers(0, 800, (G, 256)).astype(np.int32),
          "values": rng.standard_normal((G, 256)), "priors": rng.random((G, 256)).astype(np.float32),
          "moves": rng.integers(0, 4096, (G, 256)).astype(np.uint16), "replies": np.zeros((G, 256), np.uint16),
          "root_visits": rng.integers(1, 800, G).astype(np.int32)}
    eng = types.SimpleNamespace(root_children=lambda: rc, val_s2=torch.linspace(-1, 1, G))
    run = types.SimpleNamespace(engine=eng)
    monkeypatch.setattr(bench.torch.cuda, "synchronize", lambda: None)
    whole = bench.last_step_outputs(run)
    assert "games" not in whole and all(v.dtype in (np.float32, np.float64) for v in whole.values())
    assert np.array_equal(whole["root_child_visits"], rc["visits"]) and np.array_equal(whole["root_child_value_sums"], rc["values"])
    assert np.array_equal(whole["root_child_moves"], rc["moves"]) and whole["leaf_value_s2"].shape == (G,)
    cap = sum(v.nbytes for v in whole.values()) // 3
    monkeypatch.setattr(bench, "DUMP_BYTES", cap)
    a, b = bench.last_step_outputs(run), bench.last_step_outputs(run)
    assert sum(v.nbytes for v in a.values()) <= cap and 0 < len(a["games"]) < G
    rows = a["games"].astype(np.int64)
    assert np.array_equal(rows, b["games"]) and np.array_equal(a["root_child_visits"], rc["visits"][rows])
    bench.write_outputs(str(tmp_path / "out"), a)
    assert sorted(os.listdir(str(tmp_path / "out"))) == sorted(k + ".npy" for k in a)
