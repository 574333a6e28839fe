"""Lockstep search engine: G independent self-play games advance one MCTS
simulation per step on one MI355X.

This is the host-side driver of the HIP kernels behind the reference's
``SelfPlayTree.search_move`` (/root/reference/src/chessrl/mctree.py:159-214).
One *step* = one ``explore_tree`` for every game:

    crl_sim_select_expand   backprop(previous sim) + select + expand up to S1
    evaluator(planes S1)    tower forward #1  -> policy(S1)      (opponent reply)
    crl_sim_reply           greedy reply, S2, Node(S2), encode S2
    evaluator(planes S2)    tower forward #2  -> policy(S2), value(S2)

``LockstepEngine(..., reply=MinimaxPlayer(...))`` searches against the built-in opponent (csrc/opponent.hpp) instead:
the reply stored in a node is that opponent's move from S1 -- a function of the board alone, so it is the move the
real opponent plays there and ``advance`` plays a real game against it.  Such a step is three phases,

    crl_sim_select_expand   as above
    crl_sim_reply_opponent  alpha-beta from S1, S2, Node(S2), encode S2
    evaluator(planes S2)    the only tower forward

and S1 is never evaluated.

All four are enqueued on one HIP stream with no host synchronisation and are
captured once into a hipGraph (torch.cuda.CUDAGraph) that is replayed S times
per move.  Tensors never leave HBM: the encoder kernels write the tower's input
in place -- 128 plane bitboards per position for the fused HIP trunk, which
expands them on chip, or fp16 NHWC planes for any other evaluator -- and the
search kernels read the tower's fp32 outputs in place
(``torch.Tensor.data_ptr()`` across the C-ABI).

Sequential ``threads=1`` semantics of the reference by default: per game,
simulations are strictly ordered.

``LockstepEngine(..., threads=T)`` with T > 1 runs the reference's ``threads``
workers per tree in the WAVE schedule (csrc/search_wave.hpp) -- the deterministic
one among the legal schedules of its virtual-loss thread pool (mctree.py:12,
173-176,226-227,289-293): a step selects up to T leaves per game, the two tower
calls evaluate G*T rows (row = game * T + thread), and the leaves are backed up
in thread order.  Waves may end short, so the number of steps of a search is
data-dependent, between ceil(n/T) and n; a game whose budget is spent idles.
The step is the same list of phases: the engine picks its kernel triple once
(crl_sim_* or crl_wave_* select / reply / backup) and the tower calls see more rows.
"""
import gc

import numpy as np
import torch

from . import _lib
from .searchmode import REPLY_REFUSED, SearchMode        # (REPLY_REFUSED: importable from here as ever)
from .simulation import stream_keys


def compute_policy(visits, root_visits, nb_moves, noise=True, rng=None):
    """SelfPlayTree.compute_policy (mctree.py:305-322) on host numpy.

    ``visits`` in children order.  ``rng``: a numpy Generator/RandomState or
    None for the global ``np.random`` stream the reference draws from.
    """
    tau = 1
    if nb_moves >= 30:
        tau = nb_moves / (1 + np.power(nb_moves, 1.3))
    policy = np.array([np.power(v, 1 / tau) for v in visits]) / np.power(root_visits, 1 / tau)
    if noise:
        epsilon = 0.25
        policy = (1 - epsilon) * policy + (rng or np.random).dirichlet([0.03] * len(visits))
    return policy


_ALPHA = {}


def dirichlet_row(src, n):
    """``np.random.dirichlet([0.03] * n)`` (mctree.py:319-320) from the stream ``src``."""
    a = _ALPHA.get(n)
    if a is None:
        a = _ALPHA[n] = np.full(n, 0.03)
    return src.dirichlet(a)


def choose_children(visits, nchild, root_visits, plies, noise=True, rngs=None, noise_rows=None):
    """``np.argmax(compute_policy(...))`` for every game at once (-1 where nchild == 0).

    Same arithmetic as ``compute_policy`` element for element (numpy's array ``power``, multiply, add
    and division are the scalar ones applied per element), so the chosen child is identical; only
    the per-game Dirichlet draw stays a loop because every game owns its random stream.
    ``visits`` [G, >=max(nchild)] int, children order; ``rngs`` one generator per game (or None
    for the global ``np.random`` stream, drawn in game order); ``noise_rows``: the draws already
    made for this move (``SelfPlayRunner`` makes them while the GPU searches) -- either a list with
    one row of ``nchild[g]`` entries per game with children, or a pair (matrix float64 [G, >=max
    nchild] holding the rows left-aligned, counts int [G]): the latter is consumed without a Python
    loop (4096 per-game argmax calls were most of a move boundary).
    """
    G = len(nchild)
    nchild = np.asarray(nchild)
    plies_f = np.asarray(plies, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = np.where(plies_f >= 30, plies_f / (1 + np.power(plies_f, 1.3)), 1.0)
        inv_tau = 1 / tau
        w = int(nchild.max()) if G else 0
        pol = (np.power(np.asarray(visits)[:, :w].astype(np.float64), inv_tau[:, None]) /
               np.power(np.asarray(root_visits, dtype=np.float64), inv_tau)[:, None])
    chosen = np.full(G, -1, dtype=np.int32)
    cols = np.arange(w)
    live = nchild > 0
    if noise and isinstance(noise_rows, tuple):
        mat, cnt = noise_rows
        bad = np.nonzero(live & (np.asarray(cnt)[:G] != nchild))[0]
        if len(bad):
            g = int(bad[0])
            raise RuntimeError("noise drawn ahead for %d children, game %d has %d" % (int(cnt[g]), g, int(nchild[g])))
        if mat.shape[1] < w:
            raise RuntimeError("noise matrix narrower than the widest root")
        with np.errstate(invalid="ignore"):
            noisy = (1 - 0.25) * pol + mat[:G, :w]
        masked = np.where(cols[None, :] < nchild[:, None], noisy, -np.inf)
        chosen[live] = np.argmax(masked[live], axis=1)
    elif noise:
        for g in range(G):
            n = int(nchild[g])
            if n:
                if noise_rows is not None:
                    row = noise_rows[g]
                    if row is None or len(row) != n:
                        raise RuntimeError("noise drawn ahead for %s children, game %d has %d"
                                           % (None if row is None else len(row), g, n))
                else:
                    row = dirichlet_row(rngs[g] if rngs is not None else np.random, n)
                chosen[g] = int(np.argmax((1 - 0.25) * pol[g, :n] + row))
    else:
        masked = np.where(cols[None, :] < nchild[:, None], pol, -np.inf)
        chosen[live] = np.argmax(masked[live], axis=1)
    return chosen


def resolve_numpy_promotion(mode="auto"):
    """Which arithmetic ``Node.get_value``'s ``C * self.prior`` (mctree.py:79-87: python int x
    ``np.float32`` scalar) has.  Under the reference's pinned numpy==1.17.2 (requirements.txt:6;
    any numpy < 2) value-based scalar promotion makes it a float64 product: ``"legacy"``; under
    numpy >= 2 (NEP 50) it is rounded to float32: ``"nep50"``.  ``"auto"`` (the default
    everywhere) asks the numpy this process runs on -- the same numpy the reference would run on
    if it were started in this interpreter, so a drop-in replacement computes what the code it
    replaces computed there."""
    if mode == "auto":
        return "legacy" if (10 * np.float32(0.1)).dtype == np.float64 else "nep50"
    if mode not in ("nep50", "legacy"):
        raise ValueError("numpy_promotion must be 'auto', 'nep50' or 'legacy'")
    return mode


# stamp ids (StampRing): the engine's phase boundaries and the evaluator's trunk launches
STAMP_STEP, STAMP_SELECTED, STAMP_S1_DONE, STAMP_REPLIED, STAMP_GRAPH_END = 0, 1, 2, 3, 4
STAMP_ROLLOUT = 5                    # only with LockstepEngine(simulate=...): the playouts behind the second tower call
STAMP_TRUNK = {"f16": (8, 9), "f16x3": (10, 11), "f16x3 indexed": (12, 13)}      # (begin, end) per trunk arithmetic


class StampRing(object):
    """Device ring of (id, device wall clock) pairs written by ``crl_stamp`` (include/chessrl_hip.h): one-thread
    kernels that capture into a hipGraph like any other, so the time of every phase of a step and of every trunk
    launch comes from the REPLAYED graph -- consecutive stamps telescope to the step -- instead of from eager
    launches timed beside it (C5's eager phases added up to 1.03-1.10 x its graph-replayed step)."""

    def __init__(self, capacity, device):
        self.capacity = int(capacity)
        self.dev = torch.device(device)
        self.ring = torch.zeros(2 + 2 * self.capacity, dtype=torch.int64, device=self.dev)
        khz = _lib.lib().crl_stamp_clock_khz(self.dev.index or 0)
        if khz <= 0:
            raise _lib.HipLibraryError("crl_stamp_clock_khz failed (%d)" % khz)
        self.ticks_per_ms = float(khz)

    def stamp(self, sid):
        _lib.stamp(self.ring, self.capacity, sid)

    def clear(self):
        self.ring.zero_()

    def read(self):
        """[(id, milliseconds since the first stamp)] in the order written (synchronises)."""
        torch.cuda.synchronize(self.dev)
        host = self.ring.cpu().numpy()
        n = int(host[0])
        if n > self.capacity:
            raise RuntimeError("stamp ring overflowed (%d stamps, capacity %d)" % (n, self.capacity))
        ids, clk = host[2:2 + 2 * n:2], host[3:3 + 2 * n:2]
        return [(int(i), float(c - clk[0]) / self.ticks_per_ms) for i, c in zip(ids, clk)]


def summarise_stamps(stamps):
    """Per-phase means of a stamped run (``StampRing.read()``).  Every interval between two consecutive stamps is
    attributed to what ran in it -- so the parts add up to the wall time between the first and the last stamp BY
    CONSTRUCTION; what the comparison with the un-stamped timed step then shows is the cost of the stamps themselves
    (one launch gap each).  An interval that starts at a trunk-begin stamp is that trunk launch (one kernel for the
    fused trunk, the 42 of a layer-wise forward); the rest of a tower phase (heads, the hybrid mode's margin kernel,
    the stamps' own gaps) is "tower_s1 other" / "tower_s2 other".
    Returns {steps, ms_per_step, stamps_per_step, parts: {name: ms per step}, trunk: {kind: {launch_ms,
    launches_per_step, min_ms, max_ms}}}."""
    phase_of = {STAMP_STEP: "select_expand", STAMP_SELECTED: "tower_s1", STAMP_S1_DONE: "reply",
                STAMP_REPLIED: "tower_s2", STAMP_GRAPH_END: "graph_launch_gap", STAMP_ROLLOUT: "rollout"}
    begin = {b: k for k, (b, e) in STAMP_TRUNK.items()}
    parts, trunk, steps, phase = {}, {}, 0, None
    first = next((k for k, (i, _) in enumerate(stamps) if i == STAMP_STEP), len(stamps))
    stamps = stamps[first:]                  # (evaluations in front of the first step -- warm-up, the root -- are not steps)
    for (i0, t0), (i1, t1) in zip(stamps[:-1], stamps[1:]):
        dt = t1 - t0
        if i0 == STAMP_STEP:
            steps += 1
        phase = phase_of.get(i0, phase)
        if i0 in begin:
            kind = begin[i0]
            if i1 != STAMP_TRUNK[kind][1]:
                raise RuntimeError("stamp %d (trunk begin) followed by %d" % (i0, i1))
            trunk.setdefault(kind, []).append(dt)
            key = "trunk %s (%s)" % (kind, "s1" if phase == "tower_s1" else "s2")
        elif phase in ("tower_s1", "tower_s2"):
            key = phase + " other"
        else:
            key = phase or "before the first step"
        parts[key] = parts.get(key, 0.0) + dt
    if steps == 0:
        raise RuntimeError("no complete step among the stamps")
    total = stamps[-1][1] - stamps[0][1]
    return {"steps": steps, "ms_per_step": total / steps, "stamps_per_step": (len(stamps) - 1) / steps,
            "parts": {k: v / steps for k, v in sorted(parts.items())},
            "trunk": {k: {"launch_ms": sum(v) / len(v), "launches_per_step": len(v) / steps,
                          "min_ms": min(v), "max_ms": max(v)} for k, v in trunk.items()}}


class LockstepEngine(object):
    """G games x one search tree each on one GPU.

    evaluator(planes[G,8,8,128] fp16 cuda) -> (policy[G,1968] f32, value[G] f32) cuda tensors; an
    evaluator with ``accepts_bitplanes`` is given int64 [G,128] plane bitboards instead.

    ``reply``: None -- the reply stored in a node is the net's greedy move -- or a ``chessrl_amd.opponent.MinimaxPlayer``:
    the built-in opponent's move, searched with the player's ``search_depth``, ``quiescence`` and ``node_limit`` (its colour is
    ignored: the side to move after our move replies).  A player with a ``node_budget`` replies by iterative deepening
    under that budget (csrc/opponent.hpp ``k_reply_opponent_id``); one without launches the fixed-depth kernel as before.
    The player's other options (``MinimaxPlayer.options``: ``ordering``, ``repetition``, ``evaluation``, ``selective``,
    ``exchange``) choose the instantiation of that kernel template, eager and captured.  With ``repetition`` a reply
    search scores a position it has had, in its own line, on the tree path or in the game, a draw.
    """

    def __init__(self, evaluator, n_games, max_sims, device=0, max_plies=4096,
                 numpy_promotion="auto", use_graph=True, bitplanes=None, legal_priors=None, raw_priors=None,
                 steps_per_graph=None, max_nodes=None, simulate=None, threads=1, reply=None):
        numpy_promotion = resolve_numpy_promotion(numpy_promotion)
        # what kind of step this is, and -- by name, before anything touches the device -- what that kind does not cover
        mode = SearchMode(threads, simulate, reply)
        if legal_priors:
            mode.require("legal_priors", "legal_priors")
        if raw_priors:
            mode.require("raw_priors", "raw_priors")
        if max_nodes is not None and max_nodes != max_sims + 1:
            mode.require("tree_reuse", "max_nodes")
        if not mode.covers("legal_priors"):      # the search reads the full policy vectors
            legal_priors, raw_priors = False, False
        threads = mode.threads
        self.threads, self.simulate, self.reply = threads, simulate, reply
        # node budget of every tree (default max_sims + 1: a fresh tree per move never needs more); a larger
        # one leaves room for the subtree ``reroot`` keeps across a move boundary
        if max_nodes is None:
            max_nodes = max_sims + 1
        if not max_sims + 1 <= max_nodes <= 32000:
            raise ValueError("max_nodes must lie in [max_sims + 1, 32000]")
        self.max_nodes = max_nodes
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("LockstepEngine needs an MI355X: no CPU fallback exists")
        self.numpy_promotion = numpy_promotion
        self.G, self.max_sims = n_games, max_sims
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        self.ctx = _lib.Context(n_games, max_nodes - 1, max_plies=max_plies, device=device,
                                numpy_legacy=(numpy_promotion == "legacy"))
        self.evaluator = evaluator
        # the kernel triple of a step -- select, reply and the last backup -- chosen once: one leaf per game or a wave
        if threads > 1:
            self.ctx.wave_config(threads)
        self._select, self._reply, self._backup = (getattr(self.ctx, name) for name in mode.kernels)
        G = n_games * mode.rows_per_game         # evaluator rows: one per game, or game-major one per (game, thread)
        # An evaluator that runs the fused HIP trunk takes the encoder's compact form -- 128 plane
        # bitboards (1 KiB) per position -- and expands it on chip: the 16-KiB fp16 planes are then
        # never written to HBM.  Any other evaluator gets the fp16 NHWC planes.
        if bitplanes is None:
            bitplanes = bool(getattr(evaluator, "accepts_bitplanes", False))
        self.bitplanes = bitplanes
        # every tensor with one row per evaluator row, by attribute name, at full size (``shrink`` re-slices from here)
        rows = self._rows = {}
        if bitplanes:
            self.ctx.set_plane_format(True)
            rows["planes_s1"] = torch.zeros((G, _lib.PLANES), dtype=torch.int64, device=self.dev)
            rows["planes_s2"] = torch.zeros((G, _lib.PLANES), dtype=torch.int64, device=self.dev)
        else:
            rows["planes_s1"] = torch.zeros((G, 8, 8, _lib.PLANES), dtype=torch.float16, device=self.dev)
            rows["planes_s2"] = torch.zeros((G, 8, 8, _lib.PLANES), dtype=torch.float16, device=self.dev)
        rows["pol_s1"] = torch.zeros((G, _lib.N_LABELS), dtype=torch.float32, device=self.dev)
        rows["pol_s2"] = torch.zeros((G, _lib.N_LABELS), dtype=torch.float32, device=self.dev)
        rows["val_s2"] = torch.zeros((G,), dtype=torch.float32, device=self.dev)
        # An evaluator with ``accepts_legal_labels`` (the HIP heads) is told which labels the search
        # will read -- the legal moves of S1 / S2, listed by the kernel that generated them -- and
        # writes only those probabilities: priors [G,256] instead of policy [G,1968] per call
        # (CRL_POLICY_LEGAL).  Root priors and greedy openings still use the full vectors.
        if legal_priors is None:
            legal_priors = bool(getattr(evaluator, "accepts_legal_labels", False))
        self.legal_priors = legal_priors
        self.raw_priors = False
        self._want_raw = raw_priors              # None: wherever the heads support it; False: never
        if legal_priors:
            rows["pri_s1"] = torch.zeros((G, _lib.MAX_MOVES), dtype=torch.float32, device=self.dev)
            rows["pri_s2"] = torch.zeros((G, _lib.MAX_MOVES), dtype=torch.float32, device=self.dev)
            self._lab_s1 = self.ctx.eval_labels(0)
            self._lab_s2 = self.ctx.eval_labels(1)
            # small batches: the heads leave logits + the softmax statistics of their label slices and
            # the search kernels normalise on read (CRL_POLICY_LEGAL_RAW): one launch fewer per tower
            # call.  Each evaluation slot owns its statistics (S2's are read by the NEXT step's select).
            self.stats_s1 = torch.zeros((G, 16), dtype=torch.float32, device=self.dev)
            self.stats_s2 = torch.zeros((G, 16), dtype=torch.float32, device=self.dev)
            self.ctx.set_policy_stats(0, self.stats_s1.data_ptr())
            self.ctx.set_policy_stats(1, self.stats_s2.data_ptr())
            self._pick_policy_format()
        else:                                    # (always so with threads > 1) the search reads the full policy vectors
            rows["pri_s1"], rows["pri_s2"] = rows["pol_s1"], rows["pol_s2"]
        if reply is not None:
            # the engine owns the per-slot depths and the two accumulators the captured step reads and writes
            rows["reply_depths"] = torch.full((G,), reply.search_depth, dtype=torch.int32, device=self.dev)
            rows["reply_nodes"] = torch.zeros((G,), dtype=torch.int64, device=self.dev)
            rows["reply_cuts"] = torch.zeros((G,), dtype=torch.int32, device=self.dev)
            if reply.node_budget is not None:    # iterative deepening: the sum of the depths the replies completed
                rows["reply_depth_sum"] = torch.zeros((G,), dtype=torch.int64, device=self.dev)
        self._take_rows(G)
        # simulate=Rollouts(...): leaves are valued by random playouts (simulation.py:19-34, the alternative
        # mctree.py:272-274 names) instead of the value head -- a fifth phase that overwrites val_s2.  The
        # tower still runs: its priors are needed.  The engine owns the stream keys (set_stream_keys).
        if simulate is not None:
            self.stream_keys = torch.from_numpy(stream_keys(simulate.seed, G).view(np.int64)).to(self.dev)
            self.roll_results = torch.zeros((G, simulate.repetitions), dtype=torch.int8, device=self.dev)
            self.roll_plies = torch.zeros((G, simulate.repetitions), dtype=torch.int16, device=self.dev)
        # one step: (the stamp in front of a phase when a StampRing is attached, the phase method by name)
        self._plan = mode.plan
        self.use_graph = use_graph
        if steps_per_graph is not None:
            if int(steps_per_graph) < 1:
                raise ValueError("steps_per_graph must be >= 1")
            self.STEPS_PER_GRAPH = int(steps_per_graph)      # (instance override of the class default)
        self.stamps = None                   # measurement: a StampRing -> every phase of a step is stamped (bench.py)
        self._stamped_ring = None            # ... the ring the cached stamped graphs write into
        self._graphs = {}                    # (steps per graph, stamped?) -> captured hipGraph
        self._graph_epoch = 0
        self._bind_stream()

    # ---- plumbing ---------------------------------------------------------------------
    def _pick_policy_format(self):
        """CRL_POLICY_LEGAL_RAW where the evaluator's heads can skip their normalising pass for this
        batch size, else CRL_POLICY_LEGAL.  Only called while no simulation is pending (construction,
        ``shrink`` at a move boundary): priors written in one format are never read in the other."""
        sup = getattr(self.evaluator, "raw_priors_supported", None)
        self.raw_priors = bool(self._want_raw is not False and sup is not None and sup(self.G))
        self.ctx.set_policy_format(_lib.POLICY_LEGAL_RAW if self.raw_priors else _lib.POLICY_LEGAL)

    @property
    def mode(self):
        """The ``SearchMode`` of this engine: what kind of step it runs and what that kind covers."""
        return SearchMode.of(self)

    def _bind_stream(self):
        self.ctx.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)

    def close(self):
        self._graph = None
        self.ctx.close()

    def _take_rows(self, n):
        """self.planes_s1 ... self.pri_s2: the first ``n`` rows of every registered row tensor."""
        for name, t in self._rows.items():
            setattr(self, name, t[:n])

    def shrink(self, n):
        """Keep only slots [0, n) in the lockstep batch (finite runs: the batch thins out as games
        end; the caller compacts the running games into the first slots with ``ctx.copy_game``).
        Every later launch, tower batch and the re-captured hipGraph cover n games."""
        if not 0 < n <= self._rows["val_s2"].shape[0] // self.threads or n % 4:
            raise ValueError("shrink: n must be a multiple of 4 within the engine's capacity")
        self.ctx.set_window(0, n)
        self.G = n
        self._take_rows(n * self.threads)
        if self.legal_priors:
            self._pick_policy_format()
        self._graph = None

    def _eval_into(self, planes, pol_out, val_out):
        fi = getattr(self.evaluator, "forward_into", None)
        if fi is not None:                       # ChessModel: no extra copy of the 32 MB policy
            fi(planes, pol_out, val_out)
            return
        pol, val = self.evaluator(planes)
        pol_out.copy_(pol)
        if val_out is not None:
            val_out.copy_(val)

    def _root_rows(self, t):
        """The rows of ``t`` that belong to the roots: with ``threads`` > 1 the first G of its G*T rows."""
        return t if self.threads == 1 else t[:self.G]

    # the four phases of one step (bench.py times them one by one); with threads > 1 the same four on G*T rows, the
    # two kernel phases being the wave kernels
    def phase_select_expand(self):
        self._select(self.pri_s2.data_ptr(), self.val_s2.data_ptr(), self.planes_s1.data_ptr())

    def phase_tower_s1(self):
        if self.legal_priors:
            self.evaluator.forward_legal_into(self.planes_s1, self._lab_s1[0], self._lab_s1[1], self.pri_s1, None,
                                              **({"stats_out": self.stats_s1} if self.raw_priors else {}))
        else:
            self._eval_into(self.planes_s1, self.pol_s1, None)

    def phase_reply(self):
        self._reply(self.pri_s1.data_ptr(), self.planes_s2.data_ptr())

    def phase_reply_opponent(self):
        """Only with ``reply``: the built-in opponent's move from S1 becomes the node's reply."""
        opts = self.reply.options
        self.ctx.sim_reply_opponent(self.reply_depths.data_ptr(), self.reply.node_limit, self.planes_s2.data_ptr(),
                                    self.reply_nodes.data_ptr(), self.reply_cuts.data_ptr(),
                                    dev_depth_sum=None if opts.node_budget is None else self.reply_depth_sum.data_ptr(),
                                    **opts.kwargs)

    def phase_tower_s2(self):
        if self.legal_priors:
            self.evaluator.forward_legal_into(self.planes_s2, self._lab_s2[0], self._lab_s2[1], self.pri_s2, self.val_s2,
                                              **({"stats_out": self.stats_s2} if self.raw_priors else {}))
        else:
            self._eval_into(self.planes_s2, self.pol_s2, self.val_s2)

    def phase_rollout(self):
        """Only with ``simulate``: val_s2 of every slot whose pending leaf is a running S2 becomes the mean of
        its playouts (slots without one get 0, which the backup does not read)."""
        sim = self.simulate
        self.ctx.rollout(_lib.ROLLOUT_LEAVES, sim.repetitions, sim.max_moves, self.stream_keys.data_ptr(),
                         self.val_s2.data_ptr(), self.roll_results.data_ptr(), self.roll_plies.data_ptr())

    def set_stream_keys(self, keys):
        """The 64-bit stream key of every slot (default: seed * 2^32 + slot index), copied into the tensor the
        captured step reads: int64 / uint64 tensor or array of n_games entries."""
        if self.simulate is None:
            raise ValueError("set_stream_keys: the engine was created without simulate")
        if not torch.is_tensor(keys):
            keys = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))
        if keys.numel() != self.stream_keys.numel():
            raise ValueError("set_stream_keys: one key per slot (%d)" % self.stream_keys.numel())
        self.stream_keys.copy_(keys.to(self.dev).view(torch.int64).reshape(-1))

    def set_reply_depths(self, depths):
        """The opponent's search depth of every slot (default: the player's ``search_depth``), copied into the tensor
        the captured step reads: n_games values in 1 .. 5."""
        if self.reply is None:
            raise ValueError("set_reply_depths: the engine was created without reply")
        d = np.ascontiguousarray(depths, dtype=np.int32).reshape(-1)
        if d.size != self.reply_depths.numel():
            raise ValueError("set_reply_depths: one depth per slot (%d)" % self.reply_depths.numel())
        if d.size and (d.min() < 1 or d.max() > _lib.OPP_MAX_DEPTH):
            raise ValueError("set_reply_depths: depths must lie in [1, %d]" % _lib.OPP_MAX_DEPTH)
        self.reply_depths.copy_(torch.from_numpy(d).to(self.dev))

    def reply_stats(self):
        """(nodes int64 [G], cuts int32 [G]) as numpy: what the opponent's replies of the current search cost per
        slot -- nodes searched and replies ended by the node limit (synchronises).  A ``reply`` with a ``node_budget``
        adds a third array, depth sums int64 [G]: the completed depths of the replies, summed (a cut reply is then one
        that did not complete its maximum depth)."""
        if self.reply is None:
            raise ValueError("reply_stats: the engine was created without reply")
        out = (self.reply_nodes.cpu().numpy(), self.reply_cuts.cpu().numpy())
        if self.reply.node_budget is not None:
            out += (self.reply_depth_sum.cpu().numpy(),)
        return out

    def _step_body(self):
        # with a StampRing attached this is the measurement build of the same step (bench.py): a one-thread stamp
        # kernel in front of every phase, captured into the graph with them; the evaluator stamps its own trunk
        # launches (ChessModel.stamp_fn)
        st = self.stamps
        for stamp_id, phase in self._plan:
            if st is not None:
                st.stamp(stamp_id)
            getattr(self, phase)()

    def set_stamps(self, ring):
        """Attach (or with None detach) a StampRing: ``run_steps`` then replays the STAMPED build of the step (captured
        on first use, cached beside the plain graphs: switching between the two costs nothing, so a stamped leg can
        follow a timed window without a capture in between).  Stamped graphs write into the ring they were captured
        with: another ring drops them."""
        if ring is not None:
            self.mode.require("stamps", "set_stamps")
        if ring is not None and ring is not self._stamped_ring:
            self._graphs = {k: g for k, g in self._graphs.items() if not k[1]}
            self._stamped_ring = ring
        self.stamps = ring
        if hasattr(self.evaluator, "stamp_fn"):
            self.evaluator.stamp_fn = ring.stamp if ring is not None else None

    def drop_stamped_graphs(self):
        self.set_stamps(None)
        self._graphs = {k: g for k, g in self._graphs.items() if not k[1]}
        self._stamped_ring = None

    # One hipGraph launch costs ~12 us between the last kernel of one graph and the first of the next (measured,
    # tools/graph_unroll_probe.py): nothing at C3 (0.5 %), 9 % of a C2 step.  So the engine also keeps a graph of
    # STEPS_PER_GRAPH consecutive steps and ``run_steps(n)`` replays that one for as long as n allows
    # (C2: 133 -> 119 us per step, 3.84 -> 4.29 M simulations/s).
    STEPS_PER_GRAPH = 8

    def _capture(self, k=1):
        # warm the evaluator (library handles, autotuning, buffers it keeps between calls) outside of capture
        prepare = getattr(self.evaluator, "prepare", None)
        if prepare is not None:
            prepare(self.G * self.threads)
        if not self._graphs:
            side = torch.cuda.Stream(self.dev)
            side.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(side):
                for _ in range(3):
                    self.evaluator(self.planes_s1)
            torch.cuda.current_stream(self.dev).wait_stream(side)
        torch.cuda.synchronize(self.dev)
        g = torch.cuda.CUDAGraph()
        # thread_local: another thread of this process (rank 0's background trainer) may allocate and launch
        # on its own stream while this thread captures
        # No cyclic garbage collection inside the capture: torch.cuda.graph no longer collects before it begins, and a
        # finalizer that runs in here -- an engine dropped earlier and still held by its last tree
        # (mctree: tree._engine <-> engine._tree_owner), whose Context.__del__ is crl_destroy -- would synchronise
        # the device and free memory on the capturing thread.  What is garbage now is collected after the capture.
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._bind_stream()              # kernels must land on the capturing stream
                for _ in range(k):
                    self._step_body()
                if self.stamps is not None:
                    self.stamps.stamp(STAMP_GRAPH_END)
        finally:
            if gc_was_on:
                gc.enable()
        self._bind_stream()
        self._graphs[(k, self.stamps is not None)] = g
        self._graph_epoch = getattr(self.evaluator, "graph_epoch", 0)
        return g

    @property
    def _graph(self):
        """the one-step graph (None until captured); assigning None drops every captured graph"""
        return self._graphs.get((1, False))

    @_graph.setter
    def _graph(self, value):
        if value is not None:
            raise ValueError("graphs are captured by the engine")
        self._graphs = {}

    def _graph_of(self, k):
        # an evaluator whose kernel choice changed (ChessModel precision "auto" after new weights)
        # says so through graph_epoch: the captured launches are stale, capture again
        if self._graphs and self._graph_epoch != getattr(self.evaluator, "graph_epoch", 0):
            self._graphs = {}
        g = self._graphs.get((k, self.stamps is not None))
        return g if g is not None else self._capture(k)

    def prepare_graphs(self, n_steps=None):
        """Capture now what ``run_steps(n_steps)`` will replay (bench.py: no capture inside a timed region).
        Capturing launches nothing: the search state is untouched."""
        if self.use_graph:
            if n_steps is None or n_steps >= self.STEPS_PER_GRAPH > 1:
                self._graph_of(self.STEPS_PER_GRAPH)
            self._graph_of(1)

    def run_steps(self, n):
        """``n`` steps for every game (enqueue only, no host sync): a step is one simulation per game, or with
        ``threads`` > 1 one wave of up to ``threads`` simulations per game."""
        if not self.use_graph:
            for _ in range(n):
                self._step_body()
            return
        K = self.STEPS_PER_GRAPH
        while K > 1 and n >= K:
            self._graph_of(K).replay()
            n -= K
        while n > 0:
            self._graph_of(1).replay()
            n -= 1

    def step(self):
        """One step for every game (enqueue only, no host sync): one simulation, or with ``threads`` > 1 one wave."""
        self.run_steps(1)

    # ---- SelfPlayTree surface -------------------------------------------------------------
    def search_begin(self, keep_root=False):
        """Tree.__init__ for every slot + the root's policy (priors of its children).  ``keep_root``: slots whose
        root ``reroot`` kept go on with that tree (Tree(Node), mctree.py:98-111); the others start a fresh one."""
        if keep_root:
            self.mode.require("tree_reuse", "keep_root")
        self._bind_stream()
        if keep_root:
            self.ctx.search_begin_kept(self.planes_s2.data_ptr())
        else:
            self.ctx.search_begin(self.planes_s2.data_ptr())
        self._eval_into(self._root_rows(self.planes_s2), self._root_rows(self.pol_s2), self._root_rows(self.val_s2))
        self.ctx.search_root_priors(self.pol_s2.data_ptr())
        if self.reply is not None:
            self.reply_nodes.zero_()
            self.reply_cuts.zero_()
            if self.reply.node_budget is not None:
                self.reply_depth_sum.zero_()

    def search(self, n_sims, keep_root=False):
        """search_begin + n_sims lockstep simulations + the last backprop.  A kept tree that would not fit n_sims
        more nodes was already turned into a fresh one by ``reroot(chosen, n_sims)``."""
        if n_sims > self.max_sims:
            raise ValueError("n_sims exceeds the max_sims this engine was created with")
        self.search_begin(keep_root=keep_root)
        if self.threads > 1:
            self.run_waves(n_sims)
            return
        self.run_steps(n_sims)
        self._backup(self.pri_s2.data_ptr(), self.val_s2.data_ptr())

    def run_waves(self, n_sims, while_enqueued=None):
        """After ``search_begin``: exactly ``n_sims`` simulations for every live game in waves of up to ``threads``,
        the last backprop included.  ceil(n/T) steps are enqueued blind; a wave that ended short leaves budget
        behind, so the largest remaining budget of the batch is then polled (one int) and at least the steps it
        still needs are enqueued, until it is 0.  ``while_enqueued``: called once the blind steps are enqueued and
        before the first poll synchronises -- host work that overlaps the GPU (the runner's noise draws).
        Returns the number of steps (also kept in ``wave_steps``)."""
        if n_sims > self.max_sims:
            raise ValueError("n_sims exceeds the max_sims this engine was created with")
        T = self.threads
        self.ctx.wave_begin(n_sims)
        steps = -(-n_sims // T)
        self.run_steps(steps)
        if while_enqueued is not None:
            while_enqueued()
        while True:
            left = self.ctx.wave_remaining()
            if left == 0:
                break
            more = -(-left // T)
            self.run_steps(more)
            steps += more
        self._backup(self.pri_s2.data_ptr(), self.val_s2.data_ptr())
        self.wave_steps = steps
        return steps

    def root_children(self):
        return self.ctx.root_children()

    def advance(self, chosen, plies=2):
        """Play the chosen root children.  ``plies=2`` (default): our move and the reply stored in the tree,
        returns (bm, am).  ``plies=1``: our move alone -- the other side moves for itself and its move arrives
        through ``ctx.push_moves`` -- returns bm; only on a plain leaf-mode engine with a fresh tree per move."""
        if plies == 2:
            return self.ctx.advance(chosen)
        if plies != 1:
            raise ValueError("advance: plies must be 1 or 2")
        self._require_one_ply()
        return self.ctx.advance_one(chosen)

    def _require_one_ply(self):
        # the one-ply boundary belongs to a game whose other side searches for itself: nothing that answers for it
        # (reply=), keeps a tree rooted two plies on (max_nodes above max_sims + 1) or runs waves is covered
        if self.reply is not None:
            raise ValueError("advance(plies=1): the engine was created with reply=, which plays the reply itself")
        if self.max_nodes != self.max_sims + 1:
            raise ValueError("advance(plies=1): max_nodes above max_sims + 1 is tree reuse, which stays two-ply")
        if self.threads > 1:
            raise ValueError("advance(plies=1): not with threads > 1")

    def advance_argmax(self, mover_white, ply_limit):
        """``root_children()``, ``choose_children(noise=False)`` and ``advance(chosen, plies=1)`` in one kernel and
        without the host (``crl_advance_one_argmax``).  A slot moves iff its tree is alive, its game has no result,
        it has played fewer than ``ply_limit[slot]`` plies (int32 per slot; a device tensor is taken as it is), the
        side to move is ``mover_white`` and its root has an expanded child; it plays the first maximum of the root
        children's visits in children order.  Returns ``(bm, chosen)`` as DEVICE tensors on the current stream --
        int16 [G] holding the uint16 move ids (``NO_MOVE`` where the slot did not move) and int32 [G] (-1 there) --
        and does not synchronise.  Refuses the engines ``advance(plies=1)`` refuses."""
        self._require_one_ply()
        if not torch.is_tensor(ply_limit):
            ply_limit = torch.from_numpy(np.ascontiguousarray(ply_limit, dtype=np.int32)).to(self.dev)
        if ply_limit.dtype != torch.int32 or tuple(ply_limit.shape) != (self.G,) or ply_limit.device != self.dev:
            raise ValueError("advance_argmax: ply_limit must be int32 [%d] on %s" % (self.G, self.dev))
        self._bind_stream()
        bm = torch.empty((self.G,), dtype=torch.int16, device=self.dev)
        chosen = torch.empty((self.G,), dtype=torch.int32, device=self.dev)
        self.ctx.advance_one_argmax(bool(mover_white), ply_limit.contiguous(), bm, chosen)
        return bm, chosen

    def reroot(self, chosen, next_sims):
        """``advance`` that keeps the chosen child's subtree in every slot where kept nodes + ``next_sims`` fit
        ``max_nodes``; ``search(next_sims, keep_root=True)`` then continues on it."""
        self.mode.require("tree_reuse", "reroot")
        if next_sims > self.max_sims:
            raise ValueError("next_sims exceeds the max_sims this engine was created with")
        self._bind_stream()
        return self.ctx.reroot(chosen, next_sims)

    # ---- Game surface (batched) --------------------------------------------------------------
    def reset(self, mask=None):
        self._bind_stream()
        self.ctx.reset_games(mask)

    def greedy_move(self, mask=None, push=True):
        """agent.best_move(game, real_game=True) for the masked slots (+ gam.move(...))."""
        self._bind_stream()
        self.ctx.encode(self.planes_s1.data_ptr())
        self._eval_into(self._root_rows(self.planes_s1), self._root_rows(self.pol_s1), None)
        return self.ctx.greedy_moves(self.pol_s1.data_ptr(), mask=mask, push=push)

    def load_games(self, games):
        """Slot i becomes a deep copy of ``games[i]`` (chessrl_amd ``Game`` objects: position,
        move stack and history as they stand, whatever position they started from)."""
        from .game import arena
        self._bind_stream()
        src = arena().ctx
        for i, g in enumerate(games):
            self.ctx.copy_game_from(i, src, g._slot)

    def load_moves(self, move_lists):
        """Replay per-slot move id sequences from the start position (tests / Game copies)."""
        self.reset()
        n = max((len(m) for m in move_lists), default=0)
        if n == 0:
            return
        table = np.full((self.G, n), _lib.NO_MOVE, dtype=np.uint16)
        counts = np.zeros(self.G, dtype=np.int32)
        for g, ml in enumerate(move_lists):
            table[g, :len(ml)] = ml
            counts[g] = len(ml)
        pushed = self.ctx.push_sequences(table, counts)
        for g, ml in enumerate(move_lists):
            if pushed[g] != len(ml):
                raise ValueError("illegal move %d in sequence of slot %d" % (int(pushed[g]), g))
