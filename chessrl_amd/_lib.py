"""ctypes binding of libchessrl_hip.so (the C-ABI in include/chessrl_hip.h).

There is deliberately NO CPU fallback: if the HIP library is missing or no GPU
is visible, every entry point raises.  ``build()`` compiles the library in-tree
with hipcc for gfx950 (works without a GPU: hipcc cross-compiles).
"""
import collections
import ctypes
import hashlib
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
_CSRC = os.path.join(_PKG, "csrc")
SO_PATH = os.path.join(_PKG, "libchessrl_hip.so")
HEADER = os.path.join(_ROOT, "include", "chessrl_hip.h")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]


def sources():
    """Every file the library is compiled from (all of csrc/ and the public header)."""
    files = sorted(os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".hpp", ".h")))
    return files + [HEADER]


def source_hash():
    h = hashlib.sha256(" ".join(HIPCC_FLAGS).encode())
    for f in sources():
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


MAX_MOVES = 256
N_LABELS = 1968
PLANES = 128
NO_MOVE = 0xFFFF
RESULT_NONE = 2
ROLLOUT_GAMES, ROLLOUT_LEAVES, ROLLOUT_SKIPPED = 0, 1, 0xFFFF
OPP_MAX_DEPTH, OPP_CUT, OPP_SKIPPED = 5, 1, 2     # include/chessrl_hip.h: CRL_OPP_*
OPP_MAX_QUIESCENCE = 6    # include/chessrl_hip.h: CRL_OPP_MAX_QUIESCENCE
OPP_EVALUATIONS = {"material": 0, "positional": 1}    # include/chessrl_hip.h: CRL_OPP_EVAL_*
OPP_NODE_LIMIT = 200000   # default node limit per slot of Context.opponent_moves (a first choice)
FLAG_NUMPY_LEGACY = 1
WAVE_MAX_THREADS = 64     # include/chessrl_hip.h: CRL_WAVE_MAX_THREADS
POLICY_FULL, POLICY_LEGAL, POLICY_LEGAL_RAW = 0, 1, 2
TRUNK_BITPLANES = 1
TRUNK_SPLIT = 2
TRUNK_BALANCE = 4        # include/chessrl_hip.h: CRL_TRUNK_BALANCE (rank-tile cell: the partner-balance kernel)
LIST_HEADER = 4          # include/chessrl_hip.h: CRL_LIST_HEADER (int32 words in front of a board list)

# every symbol include/chessrl_hip.h declares (tests check the .so exports all of them)
SYMBOLS = [
    "crl_create", "crl_destroy", "crl_set_stream", "crl_sync", "crl_last_error", "crl_max_games",
    "crl_max_sims", "crl_set_window", "crl_set_plane_format", "crl_set_policy_format", "crl_eval_labels",
    "crl_copy_game", "crl_copy_game_from", "crl_uci_label_moves", "crl_reset_games", "crl_set_positions",
    "crl_get_positions", "crl_legal_moves", "crl_push_moves", "crl_push_sequences", "crl_results", "crl_records",
    "crl_encode", "crl_greedy_moves", "crl_search_begin", "crl_search_root_priors",
    "crl_sim_select_expand", "crl_sim_reply", "crl_sim_backup", "crl_root_children",
    "crl_advance", "crl_counters", "crl_trunk_forward",
    "crl_trunk_forward_bitplanes", "crl_trunk_forward_x", "crl_trunk_set_small_batch", "crl_trunk_kernel_name", "crl_heads_forward",
    "crl_heads_forward_legal", "crl_heads_forward_legal_raw", "crl_heads_raw_supported", "crl_heads_set_sliced_max",
    "crl_set_policy_stats", "crl_abi_version", "crl_source_hash", "crl_reply_margin", "crl_trunk_forward_indexed", "crl_trunk_workspace_bytes",
    "crl_end_move_fetch", "crl_advance_fetch",
    "crl_reroot", "crl_reroot_fetch", "crl_search_begin_kept", "crl_copy_game_tree", "crl_fetch_tree",
    "crl_im2col3x3_f32", "crl_col2im3x3_f32", "crl_stamp", "crl_stamp_clock_khz",
    "crl_rollout_games", "crl_rollout", "crl_opponent_moves", "crl_sim_reply_opponent",
    "crl_opponent_moves_q", "crl_sim_reply_opponent_q", "crl_opponent_moves_id", "crl_sim_reply_opponent_id",
    "crl_opponent_moves_ord", "crl_sim_reply_opponent_ord",
    "crl_opponent_moves_rep", "crl_sim_reply_opponent_rep",
    "crl_opponent_moves_ev", "crl_sim_reply_opponent_ev", "crl_opponent_evaluate",
    "crl_opponent_moves_sel", "crl_sim_reply_opponent_sel",
    "crl_opponent_moves_exc", "crl_sim_reply_opponent_exc", "crl_opponent_exchange",
    "crl_wave_config", "crl_wave_begin", "crl_wave_select", "crl_wave_reply", "crl_wave_backup", "crl_wave_remaining",
    "crl_wave_stats",
    "crl_advance_one",
    "crl_advance_one_argmax", "crl_push_moves_dev",
]


class HipLibraryError(RuntimeError):
    pass


def evaluation_name(evaluation):
    """``evaluation`` if it names an evaluation of the built-in opponent; a ValueError otherwise."""
    if not isinstance(evaluation, str) or evaluation not in OPP_EVALUATIONS:
        raise ValueError("evaluation must be one of %s" % ", ".join('"%s"' % k for k in OPP_EVALUATIONS))
    return evaluation


class OpponentOptions(collections.namedtuple(
        "OpponentOptions", "quiescence node_budget ordering repetition evaluation selective exchange")):
    """The options of the built-in opponent's search (csrc/opponent.hpp) as one value, and the one statement in Python
    of which of them combine: ``quiescence`` plies past the depth; ``node_budget`` (None: the fixed-depth search);
    ``ordering`` (ORDERING), ``repetition`` (REPETITION) and ``evaluation`` = "positional" (EVALUATION) on top of a
    budget; ``selective`` (SELECTIVE) on top of ordering; ``exchange`` (EXCHANGE) on top of ordering and quiescence
    plies.  A ValueError names the first rule broken, in the order below.  ``ranges=False`` leaves the first two rules
    to the library, which refuses such a value itself (``Context``'s methods: their callers expect its refusal)."""
    __slots__ = ()

    def __new__(cls, quiescence=0, node_budget=None, ordering=False, repetition=False, evaluation="material",
                selective=False, exchange=False, ranges=True):
        quiescence = int(quiescence)
        node_budget = None if node_budget is None else int(node_budget)
        if ranges and not 0 <= quiescence <= OPP_MAX_QUIESCENCE:
            raise ValueError("quiescence must lie in [0, %d]" % OPP_MAX_QUIESCENCE)
        if ranges and node_budget is not None and node_budget < 1:
            raise ValueError("node_budget must be None or at least 1")
        if ordering and node_budget is None:
            raise ValueError("ordering needs a node_budget")
        if repetition and node_budget is None:
            raise ValueError("repetition needs a node_budget")
        if evaluation_name(evaluation) != "material" and node_budget is None:
            raise ValueError("evaluation needs a node_budget")
        if selective and not ordering:
            raise ValueError("selective needs ordering")
        if exchange and not ordering:
            raise ValueError("exchange needs ordering")
        if exchange and quiescence < 1:
            raise ValueError("exchange needs quiescence >= 1")
        return super().__new__(cls, quiescence, node_budget, bool(ordering), bool(repetition), evaluation,
                               bool(selective), bool(exchange))

    @property
    def kwargs(self):
        """The options as the keywords of ``Context.opponent_moves`` and ``Context.sim_reply_opponent``."""
        return self._asdict()

    def budgeted_args(self, node_limit):
        """What a ``crl_*_exc`` entry takes between ``quiescence`` and its arrays: the node budget and the five flags."""
        return (min(self.node_budget, int(node_limit)), int(self.ordering), int(self.repetition),
                OPP_EVALUATIONS[self.evaluation], int(self.selective), int(self.exchange))


ABI_VERSION = 9          # include/chessrl_hip.h: CRL_ABI_VERSION (checked against the loaded library)
_HASH_MARK = b"CRL_SRC_HASH="


def embedded_hash(so=SO_PATH):
    """The source hash compiled INTO the library (csrc/api.hip: g_source_hash), read from the file
    without loading it; None when the file is missing or carries no marker."""
    try:
        data = open(so, "rb").read()
    except OSError:
        return None
    i = data.find(_HASH_MARK)
    if i < 0:
        return None
    tail = data[i + len(_HASH_MARK):i + len(_HASH_MARK) + 64]
    return tail.split(b"\0")[0].decode("ascii", "replace")


def have_sources():
    return os.path.isdir(_CSRC) and os.path.exists(HEADER)


def is_stale(so=SO_PATH):
    """True when `so` is missing or was compiled from other sources than the ones present: the
    library carries the sha256 of its sources inside (no side file that a deploy can lose or an
    interrupted build can leave behind).  A deploy of the library WITHOUT csrc/ has nothing to be
    compared with and is taken as shipped."""
    if not os.path.exists(so):
        return True
    if not have_sources():
        return False
    return embedded_hash(so) != source_hash()


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -> chessrl_amd/libchessrl_hip.so (in-tree; works without a GPU).
    Recompiles whenever any file of csrc/ or the header changed since the library was built
    (``force`` recompiles regardless).  The sources' hash is compiled in (``crl_source_hash``)."""
    so = SO_PATH
    if not force and not is_stale(so):
        return so
    # several ranks of one node may arrive here together (torchrun starts one process per GPU):
    # one compiles, the others wait on the lock and find the library fresh; the library appears
    # atomically (rename), so nobody ever loads a half-written file
    import fcntl
    with open(so + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not is_stale(so):
            return so
        tmp = "%s.tmp.%d" % (so, os.getpid())
        cmd = (["hipcc"] + HIPCC_FLAGS + ['-DCRL_SOURCE_HASH="%s"' % source_hash()] +
               ["-o", tmp, os.path.join(_CSRC, "api.hip")])
        if verbose:
            print(" ".join(cmd))
        try:
            subprocess.check_call(cmd)
            os.replace(tmp, so)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return so


_lib = None


def lib():
    """Load the shared library.  It is compiled first when it is missing or was built from other
    sources than the csrc/ present; a stale library that cannot be rebuilt is REFUSED (its entry points
    may have other signatures than this binding's), and so is a library of another ABI version.  No
    CPU fallback: without a loadable library this raises."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64; it must be the copy this process binds, or the tower and
    # the search kernels would sit on two HIP runtimes (and the second one sees no device)
    import torch  # noqa: F401
    so = SO_PATH
    if is_stale(so):
        try:
            build()
        except Exception as e:  # pragma: no cover
            raise HipLibraryError(
                "%s is %s and could not be built with hipcc (%s); the HIP path has no CPU fallback and a "
                "library built from other sources is not loaded"
                % (os.path.basename(so), "missing" if not os.path.exists(so) else "older than csrc/", e))
    try:
        L = ctypes.CDLL(so)
    except OSError as e:
        raise HipLibraryError("cannot load %s: %s" % (so, e))
    try:
        L.crl_abi_version.restype = ctypes.c_int
        L.crl_source_hash.restype = ctypes.c_char_p
        abi, built_from = L.crl_abi_version(), (L.crl_source_hash() or b"").decode()
    except AttributeError:
        raise HipLibraryError("%s exports no crl_abi_version: it predates this binding" % so)
    if abi != ABI_VERSION:
        raise HipLibraryError("%s has ABI version %d, this binding needs %d" % (so, abi, ABI_VERSION))
    if have_sources() and built_from != source_hash():
        raise HipLibraryError("%s was built from other sources (%s...) than csrc/ (%s...)"
                              % (so, built_from[:12], source_hash()[:12]))
    vp, i32, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    L.crl_create.argtypes = [ctypes.POINTER(vp), i32, i32, i32, i32, u32]
    L.crl_destroy.argtypes = [vp]
    L.crl_destroy.restype = None
    L.crl_set_stream.argtypes = [vp, vp]
    L.crl_sync.argtypes = [vp]
    L.crl_last_error.argtypes = [vp]
    L.crl_last_error.restype = ctypes.c_char_p
    L.crl_max_games.argtypes = [vp]
    L.crl_max_sims.argtypes = [vp]
    L.crl_set_window.argtypes = [vp, i32, i32]
    L.crl_copy_game.argtypes = [vp, i32, i32]
    L.crl_copy_game_from.argtypes = [vp, i32, vp, i32]
    L.crl_uci_label_moves.argtypes = [vp]
    L.crl_reset_games.argtypes = [vp, vp]
    L.crl_set_positions.argtypes = [vp, vp, i32]
    L.crl_get_positions.argtypes = [vp, vp, i32]
    L.crl_legal_moves.argtypes = [vp, vp, vp]
    L.crl_push_moves.argtypes = [vp, vp, vp]
    L.crl_push_sequences.argtypes = [vp, vp, vp, i32, vp]
    L.crl_results.argtypes = [vp, vp]
    L.crl_records.argtypes = [vp, vp, vp, vp]
    L.crl_encode.argtypes = [vp, vp]
    L.crl_greedy_moves.argtypes = [vp, vp, vp, i32, vp]
    L.crl_search_begin.argtypes = [vp, vp]
    L.crl_search_root_priors.argtypes = [vp, vp]
    L.crl_sim_select_expand.argtypes = [vp, vp, vp, vp]
    L.crl_sim_reply.argtypes = [vp, vp, vp]
    L.crl_sim_backup.argtypes = [vp, vp, vp]
    L.crl_root_children.argtypes = [vp] * 8
    L.crl_advance.argtypes = [vp, vp, vp, vp]
    L.crl_advance_one.argtypes = [vp, vp, vp]
    L.crl_advance_one_argmax.argtypes = [vp, i32, vp, vp, vp]
    L.crl_push_moves_dev.argtypes = [vp, vp, vp]
    L.crl_counters.argtypes = [vp, vp]
    L.crl_end_move_fetch.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.crl_advance_fetch.argtypes = [vp, vp, vp, vp, vp, vp]
    L.crl_reroot.argtypes = [vp, vp, i32, vp, vp]
    L.crl_reroot_fetch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.crl_search_begin_kept.argtypes = [vp, vp]
    L.crl_copy_game_tree.argtypes = [vp, i32, i32]
    L.crl_fetch_tree.argtypes = [vp, i32, vp, i32, vp, i32, vp]
    L.crl_trunk_forward.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp]
    L.crl_trunk_forward_bitplanes.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp]
    L.crl_trunk_forward_x.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, ctypes.c_size_t]
    L.crl_trunk_workspace_bytes.argtypes = [i32, i32, i32]
    L.crl_trunk_workspace_bytes.restype = ctypes.c_size_t
    L.crl_set_plane_format.argtypes = [vp, i32]
    L.crl_reply_margin.argtypes = [vp, vp, vp, i32, vp, i32, vp]
    L.crl_trunk_forward_indexed.argtypes = [vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, ctypes.c_size_t]
    L.crl_trunk_set_small_batch.argtypes = [i32]
    L.crl_trunk_kernel_name.argtypes = [i32, i32, i32, ctypes.c_char_p, i32]
    L.crl_heads_forward.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.crl_heads_forward_legal.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.crl_heads_forward_legal_raw.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.crl_heads_raw_supported.argtypes = [i32]
    L.crl_heads_set_sliced_max.argtypes = [i32]
    L.crl_set_policy_format.argtypes = [vp, i32]
    L.crl_set_policy_stats.argtypes = [vp, i32, vp]
    L.crl_eval_labels.argtypes = [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.crl_im2col3x3_f32.argtypes = [vp, vp, vp, i32, i32]
    L.crl_col2im3x3_f32.argtypes = [vp, vp, vp, i32, i32]
    L.crl_stamp.argtypes = [vp, vp, u32, u32]
    L.crl_rollout_games.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp]
    L.crl_rollout.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    L.crl_opponent_moves.argtypes = [vp, vp, i32, ctypes.c_int64, vp, vp, vp, vp]
    L.crl_sim_reply_opponent.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp]
    L.crl_opponent_moves_q.argtypes = [vp, vp, i32, i32, ctypes.c_int64, vp, vp, vp, vp]
    L.crl_sim_reply_opponent_q.argtypes = [vp, vp, i32, ctypes.c_int64, vp, vp, vp]
    L.crl_opponent_moves_id.argtypes = [vp, vp, i32, i32, ctypes.c_int64, vp, vp, vp, vp, vp]
    L.crl_sim_reply_opponent_id.argtypes = [vp, vp, i32, ctypes.c_int64, vp, vp, vp, vp]
    L.crl_opponent_moves_ord.argtypes = [vp, vp, i32, i32, ctypes.c_int64, i32, vp, vp, vp, vp, vp]
    L.crl_sim_reply_opponent_ord.argtypes = [vp, vp, i32, ctypes.c_int64, i32, vp, vp, vp, vp]
    L.crl_opponent_moves_rep.argtypes = [vp, vp, i32, i32, ctypes.c_int64, i32, i32, vp, vp, vp, vp, vp]
    L.crl_sim_reply_opponent_rep.argtypes = [vp, vp, i32, ctypes.c_int64, i32, i32, vp, vp, vp, vp]
    L.crl_opponent_moves_ev.argtypes = [vp, vp, i32, i32, ctypes.c_int64, i32, i32, i32, vp, vp, vp, vp, vp]
    L.crl_sim_reply_opponent_ev.argtypes = [vp, vp, i32, ctypes.c_int64, i32, i32, i32, vp, vp, vp, vp]
    L.crl_opponent_moves_sel.argtypes = [vp, vp, i32, i32, ctypes.c_int64, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.crl_sim_reply_opponent_sel.argtypes = [vp, vp, i32, ctypes.c_int64, i32, i32, i32, i32, vp, vp, vp, vp]
    L.crl_opponent_moves_exc.argtypes = [vp, vp, i32, i32, ctypes.c_int64, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.crl_sim_reply_opponent_exc.argtypes = [vp, vp, i32, ctypes.c_int64, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    L.crl_opponent_exchange.argtypes = [vp, vp, vp]
    L.crl_opponent_evaluate.argtypes = [vp, i32, vp]
    L.crl_stamp_clock_khz.argtypes = [i32]
    L.crl_wave_config.argtypes = [vp, i32]
    L.crl_wave_begin.argtypes = [vp, i32]
    L.crl_wave_select.argtypes = [vp, vp, vp, vp]
    L.crl_wave_reply.argtypes = [vp, vp, vp]
    L.crl_wave_backup.argtypes = [vp, vp, vp]
    L.crl_wave_remaining.argtypes = [vp, vp]
    L.crl_wave_stats.argtypes = [vp, vp, vp, vp]
    for name in SYMBOLS:
        if name not in ("crl_destroy", "crl_last_error", "crl_source_hash"):
            getattr(L, name).restype = ctypes.c_int
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def uci_label_moves():
    out = np.zeros(N_LABELS, dtype=np.uint16)
    rc = lib().crl_uci_label_moves(_ptr(out))
    if rc != 0:
        raise HipLibraryError("crl_uci_label_moves failed (%d)" % rc)
    return out


# ---- the stream-level (stateless) entry points, typed --------------------------------------------------------------
# Parameters carry the names of include/chessrl_hip.h.  A pointer argument is a tensor (anything with data_ptr();
# it must be contiguous), an int address, or None where the header allows NULL; ``hip_stream`` is a
# torch.cuda.Stream, an int, or None = the current stream of ``on``'s device.  Everything is checked before the
# library is reached; dtypes and shapes are the C side's business.
class _Dev(object):
    """One pointer argument, checked: ``_Dev(x, "name")`` must be given, ``_Dev(x, "name", None)`` may be NULL."""

    def __init__(self, x, name, *null_ok):
        if x is None and not null_ok:
            raise ValueError("%s must not be NULL" % name)
        if hasattr(x, "data_ptr"):
            if not x.is_contiguous():
                raise ValueError("%s is not contiguous" % name)
            x = x.data_ptr()
        self.p = ctypes.c_void_p(None if x is None else int(x))


def _call(name, hip_stream, on, *args):
    if hip_stream is None:
        import torch
        hip_stream = torch.cuda.current_stream(getattr(on, "device", None))
    rc = getattr(lib(), name)(ctypes.c_void_p(int(getattr(hip_stream, "cuda_stream", hip_stream))),
                              *[a.p if isinstance(a, _Dev) else int(a) for a in args])
    if rc != 0:
        raise HipLibraryError("%s failed (%d)" % (name, rc))


def trunk_forward_x(filters, flags, dev_planes, dev_wtiles_f16, dev_bias_f32, dev_out_f32, n_boards, n_blocks,
                    dev_head_w_f32, dev_head_b_f32, dev_head_out_f32, dev_workspace=None, workspace_bytes=0,
                    hip_stream=None):
    _call("crl_trunk_forward_x", hip_stream, dev_planes, filters, flags, _Dev(dev_planes, "dev_planes"),
          _Dev(dev_wtiles_f16, "dev_wtiles_f16"), _Dev(dev_bias_f32, "dev_bias_f32"), _Dev(dev_out_f32, "dev_out_f32", None),
          n_boards, n_blocks, _Dev(dev_head_w_f32, "dev_head_w_f32"), _Dev(dev_head_b_f32, "dev_head_b_f32"),
          _Dev(dev_head_out_f32, "dev_head_out_f32", None), _Dev(dev_workspace, "dev_workspace", None), workspace_bytes)


def trunk_forward_indexed(filters, dev_bitplanes_u64, dev_wtiles_f16x3, dev_bias_f32, n_boards, n_blocks, dev_head_w_f32,
                          dev_head_b_f32, dev_head_out_f32, dev_list, dev_workspace=None, workspace_bytes=0,
                          hip_stream=None):
    _call("crl_trunk_forward_indexed", hip_stream, dev_bitplanes_u64, filters, _Dev(dev_bitplanes_u64, "dev_bitplanes_u64"),
          _Dev(dev_wtiles_f16x3, "dev_wtiles_f16x3"), _Dev(dev_bias_f32, "dev_bias_f32"), n_boards, n_blocks,
          _Dev(dev_head_w_f32, "dev_head_w_f32"), _Dev(dev_head_b_f32, "dev_head_b_f32"),
          _Dev(dev_head_out_f32, "dev_head_out_f32"), _Dev(dev_list, "dev_list"),
          _Dev(dev_workspace, "dev_workspace", None), workspace_bytes)


def _heads_weights(dev_policy_wp_f16, dev_policy_bias_f32, dev_value_w1p_f16, dev_value_b1_f32, dev_value_w2b2_f32):
    return (_Dev(dev_policy_wp_f16, "dev_policy_wp_f16"), _Dev(dev_policy_bias_f32, "dev_policy_bias_f32"),
            _Dev(dev_value_w1p_f16, "dev_value_w1p_f16"), _Dev(dev_value_b1_f32, "dev_value_b1_f32"),
            _Dev(dev_value_w2b2_f32, "dev_value_w2b2_f32"))


def heads_forward(dev_head_act_f32, n_boards, dev_policy_wp_f16, dev_policy_bias_f32, dev_value_w1p_f16,
                  dev_value_b1_f32, dev_value_w2b2_f32, dev_policy_out_f32, dev_value_out_f32=None,
                  dev_scratch_f32=None, hip_stream=None):
    _call("crl_heads_forward", hip_stream, dev_head_act_f32, _Dev(dev_head_act_f32, "dev_head_act_f32"), n_boards,
          *_heads_weights(dev_policy_wp_f16, dev_policy_bias_f32, dev_value_w1p_f16, dev_value_b1_f32, dev_value_w2b2_f32),
          _Dev(dev_policy_out_f32, "dev_policy_out_f32"), _Dev(dev_value_out_f32, "dev_value_out_f32", None),
          _Dev(dev_scratch_f32, "dev_scratch_f32", None))


def heads_forward_legal(dev_head_act_f32, n_boards, dev_policy_wp_f16, dev_policy_bias_f32, dev_value_w1p_f16,
                        dev_value_b1_f32, dev_value_w2b2_f32, dev_labels, dev_counts, dev_priors_out_f32,
                        dev_value_out_f32=None, dev_scratch_f32=None, hip_stream=None):
    _call("crl_heads_forward_legal", hip_stream, dev_head_act_f32, _Dev(dev_head_act_f32, "dev_head_act_f32"), n_boards,
          *_heads_weights(dev_policy_wp_f16, dev_policy_bias_f32, dev_value_w1p_f16, dev_value_b1_f32, dev_value_w2b2_f32),
          _Dev(dev_labels, "dev_labels"), _Dev(dev_counts, "dev_counts"), _Dev(dev_priors_out_f32, "dev_priors_out_f32"),
          _Dev(dev_value_out_f32, "dev_value_out_f32", None), _Dev(dev_scratch_f32, "dev_scratch_f32", None))


def heads_forward_legal_raw(dev_head_act_f32, n_boards, dev_policy_wp_f16, dev_policy_bias_f32, dev_value_w1p_f16,
                            dev_value_b1_f32, dev_value_w2b2_f32, dev_labels, dev_counts, dev_logits_out_f32,
                            dev_value_out_f32, dev_stats_out_f32, hip_stream=None):
    _call("crl_heads_forward_legal_raw", hip_stream, dev_head_act_f32, _Dev(dev_head_act_f32, "dev_head_act_f32"), n_boards,
          *_heads_weights(dev_policy_wp_f16, dev_policy_bias_f32, dev_value_w1p_f16, dev_value_b1_f32, dev_value_w2b2_f32),
          _Dev(dev_labels, "dev_labels"), _Dev(dev_counts, "dev_counts"), _Dev(dev_logits_out_f32, "dev_logits_out_f32"),
          _Dev(dev_value_out_f32, "dev_value_out_f32", None), _Dev(dev_stats_out_f32, "dev_stats_out_f32"))


def reply_margin(dev_priors_f32, dev_counts, n_boards, dev_log_margin_f32, rows_are_logits, dev_list, hip_stream=None):
    _call("crl_reply_margin", hip_stream, dev_priors_f32, _Dev(dev_priors_f32, "dev_priors_f32"),
          _Dev(dev_counts, "dev_counts"), n_boards, _Dev(dev_log_margin_f32, "dev_log_margin_f32"), rows_are_logits,
          _Dev(dev_list, "dev_list"))


def stamp(dev_ring, capacity, id, hip_stream=None):
    _call("crl_stamp", hip_stream, dev_ring, _Dev(dev_ring, "dev_ring"), capacity, id)


def trunk_workspace_bytes(filters, n_boards, flags):
    return int(lib().crl_trunk_workspace_bytes(int(filters), int(n_boards), int(flags)))


def heads_raw_supported(n_boards):
    return bool(lib().crl_heads_raw_supported(int(n_boards)))


def trunk_kernel_name(filters, n_boards, flags):
    """The kernel crl_trunk_forward_x launches for this filter count, batch and flags, as rocprofv3 prints it."""
    buf = ctypes.create_string_buffer(256)
    rc = lib().crl_trunk_kernel_name(int(filters), int(n_boards), int(flags), buf, len(buf))
    if rc != 0:
        raise HipLibraryError("crl_trunk_kernel_name failed (%d)" % rc)
    return buf.value.decode()


class _Setting(object):
    """A process-global tuning value, set when this object is made; as a context manager it restores the default."""

    def __init__(self, name, value, default):
        self._set = lambda v: getattr(lib(), name)(int(v))
        self._default = default
        if self._set(value) != 0:
            raise HipLibraryError("%s failed" % name)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._set(self._default)


def trunk_set_small_batch(enabled):
    return _Setting("crl_trunk_set_small_batch", 1 if enabled else 0, 1)


def heads_set_sliced_max(boards):
    return _Setting("crl_heads_set_sliced_max", boards, 2048)


class Context(object):
    """One crl_ctx (one GPU).  Thin, numpy-in/numpy-out; device pointers are ints."""

    def __init__(self, max_games, max_sims, max_plies=4096, device=0, numpy_legacy=False):
        self._h = ctypes.c_void_p()
        self._L = lib()
        flags = FLAG_NUMPY_LEGACY if numpy_legacy else 0
        rc = self._L.crl_create(ctypes.byref(self._h), device, max_games, max_sims, max_plies, flags)
        if rc != 0:
            msg = self._L.crl_last_error(None)
            self._h = None
            raise HipLibraryError("crl_create failed (%d): %s" % (rc, (msg or b"").decode()))
        self.G, self.max_sims, self.max_plies, self.device = max_games, max_sims, max_plies, device
        self.n_slots = max_games

    def close(self):
        if getattr(self, "_h", None):
            self._L.crl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            msg = self._L.crl_last_error(self._h)
            raise HipLibraryError("%s failed (%d): %s" % (what, rc, (msg or b"").decode()))

    def set_stream(self, stream_ptr):
        self._ck(self._L.crl_set_stream(self._h, ctypes.c_void_p(stream_ptr)), "crl_set_stream")

    def set_window(self, first, count):
        """Later calls act on slots [first, first+count); arrays become `count` rows."""
        self._ck(self._L.crl_set_window(self._h, first, count), "crl_set_window")
        self.G = count

    def set_policy_format(self, legal):
        """What the simulation entry points take as "policy": False / 0 = full policy[row][1968] rows,
        True / 1 = priors[row][256] of the legal moves (CRL_POLICY_LEGAL), 2 = the same rows holding
        logits that the kernels normalise on read (CRL_POLICY_LEGAL_RAW; ``set_policy_stats`` first)."""
        self._ck(self._L.crl_set_policy_format(self._h, int(legal)), "crl_set_policy_format")

    def set_policy_stats(self, which, dev_stats):
        """Device address of the slice statistics (float [rows][16]) of tower call ``which`` (0: S1, 1: S2)."""
        self._ck(self._L.crl_set_policy_stats(self._h, which, ctypes.c_void_p(dev_stats)), "crl_set_policy_stats")

    def eval_labels(self, which):
        """(labels, counts) device addresses for the position tower call `which` evaluates
        (0: S1 after sim_select_expand, 1: S2 after sim_reply); rows are window-relative."""
        lab, cnt = ctypes.c_void_p(), ctypes.c_void_p()
        self._ck(self._L.crl_eval_labels(self._h, which, ctypes.byref(lab), ctypes.byref(cnt)), "crl_eval_labels")
        return lab.value, cnt.value

    def set_plane_format(self, bits):
        """Encoders write fp16 NHWC planes (False, default) or 128 plane bitboards per position (True)."""
        self._ck(self._L.crl_set_plane_format(self._h, 1 if bits else 0), "crl_set_plane_format")

    def copy_game(self, dst, src):
        self._ck(self._L.crl_copy_game(self._h, dst, src), "crl_copy_game")

    def copy_game_from(self, dst, src_ctx, src):
        """Slot ``dst`` becomes a deep copy of slot ``src`` of another context on the same GPU."""
        self._ck(self._L.crl_copy_game_from(self._h, dst, src_ctx._h, src), "crl_copy_game_from")

    def copy_game_tree(self, dst, src):
        """``copy_game`` that carries the slot's live search tree along."""
        self._ck(self._L.crl_copy_game_tree(self._h, dst, src), "crl_copy_game_tree")

    def sync(self):
        self._ck(self._L.crl_sync(self._h), "crl_sync")

    # ---- Game seam -----------------------------------------------------------------
    def reset_games(self, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self._ck(self._L.crl_reset_games(self._h, _ptr(m)), "crl_reset_games")

    def set_positions(self, boards):
        """boards: np.uint64 [n][8] rows (bb0..5, white, state)."""
        b = np.ascontiguousarray(boards, dtype=np.uint64).reshape(-1, 8)
        self._ck(self._L.crl_set_positions(self._h, _ptr(b), b.shape[0]), "crl_set_positions")

    def get_positions(self, n=None):
        n = self.G if n is None else n
        b = np.zeros((n, 8), dtype=np.uint64)
        self._ck(self._L.crl_get_positions(self._h, _ptr(b), n), "crl_get_positions")
        return b

    def legal_moves(self):
        moves = np.zeros((self.G, MAX_MOVES), dtype=np.uint16)
        counts = np.zeros(self.G, dtype=np.int32)
        self._ck(self._L.crl_legal_moves(self._h, _ptr(moves), _ptr(counts)), "crl_legal_moves")
        return moves, counts

    def legal_counts(self):
        """len(get_legal_moves()) per game without copying the move lists back."""
        counts = np.zeros(self.G, dtype=np.int32)
        self._ck(self._L.crl_legal_moves(self._h, None, _ptr(counts)), "crl_legal_moves")
        return counts

    def push_moves(self, moves):
        m = np.ascontiguousarray(moves, dtype=np.uint16)
        assert m.shape == (self.G,)
        ok = np.zeros(self.G, dtype=np.uint8)
        self._ck(self._L.crl_push_moves(self._h, _ptr(m), _ptr(ok)), "crl_push_moves")
        return ok

    def push_moves_dev(self, dev_moves, dev_ok=None):
        """``push_moves`` with the moves in device memory (uint16 [G], a tensor or an address) and no synchronisation;
        ``dev_ok`` (uint8 [G], device) may be None.  A refused move is a device error at the next synchronising call."""
        self._ck(self._L.crl_push_moves_dev(self._h, _Dev(dev_moves, "dev_moves").p, _Dev(dev_ok, "dev_ok", None).p),
                 "crl_push_moves_dev")

    def push_sequences(self, moves, counts):
        """Every game replays its own move list (one launch); returns the number applied per game."""
        m = np.ascontiguousarray(moves, dtype=np.uint16)
        c = np.ascontiguousarray(counts, dtype=np.int32)
        assert m.ndim == 2 and m.shape[0] == self.G and c.shape == (self.G,)
        pushed = np.zeros(self.G, dtype=np.int32)
        self._ck(self._L.crl_push_sequences(self._h, _ptr(m), _ptr(c), m.shape[1], _ptr(pushed)),
                 "crl_push_sequences")
        return pushed

    def results(self):
        r = np.zeros(self.G, dtype=np.int8)
        self._ck(self._L.crl_results(self._h, _ptr(r)), "crl_results")
        return r

    def records(self, with_moves=True):
        moves = np.zeros((self.G, self.max_plies), dtype=np.uint16) if with_moves else None
        plies = np.zeros(self.G, dtype=np.int32)
        res = np.zeros(self.G, dtype=np.int8)
        self._ck(self._L.crl_records(self._h, _ptr(moves), _ptr(plies), _ptr(res)), "crl_records")
        return moves, plies, res

    # ---- encoder / agent seam (device pointers) ----------------------------------------
    def encode(self, dev_planes):
        self._ck(self._L.crl_encode(self._h, ctypes.c_void_p(dev_planes)), "crl_encode")

    def greedy_moves(self, dev_policy, mask=None, push=False, want_moves=True):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        out = np.zeros(self.G, dtype=np.uint16) if want_moves else None
        self._ck(self._L.crl_greedy_moves(self._h, ctypes.c_void_p(dev_policy), _ptr(m),
                                          1 if push else 0, _ptr(out)), "crl_greedy_moves")
        return out

    # ---- SelfPlayTree seam -------------------------------------------------------------
    def search_begin(self, dev_planes):
        self._ck(self._L.crl_search_begin(self._h, ctypes.c_void_p(dev_planes)), "crl_search_begin")

    def search_begin_kept(self, dev_planes):
        """``search_begin`` that leaves the roots ``reroot`` kept as they are."""
        self._ck(self._L.crl_search_begin_kept(self._h, ctypes.c_void_p(dev_planes)), "crl_search_begin_kept")

    def search_root_priors(self, dev_policy):
        self._ck(self._L.crl_search_root_priors(self._h, ctypes.c_void_p(dev_policy)),
                 "crl_search_root_priors")

    def sim_select_expand(self, dev_policy_s2, dev_value_s2, dev_planes_s1):
        self._ck(self._L.crl_sim_select_expand(
            self._h, ctypes.c_void_p(dev_policy_s2), ctypes.c_void_p(dev_value_s2),
            ctypes.c_void_p(dev_planes_s1)), "crl_sim_select_expand")

    def sim_reply(self, dev_policy_s1, dev_planes_s2):
        self._ck(self._L.crl_sim_reply(self._h, ctypes.c_void_p(dev_policy_s1),
                                       ctypes.c_void_p(dev_planes_s2)), "crl_sim_reply")

    def sim_reply_opponent(self, dev_depths, node_limit, dev_planes_s2, dev_nodes, dev_cuts, quiescence=0,
                           node_budget=None, dev_depth_sum=None, ordering=False, repetition=False,
                           evaluation="material", selective=False, exchange=False):
        """``sim_reply`` with the built-in opponent's move as the reply: device pointers to int32 [count] depths, the
        planes of S2 and the int64 / int32 [count] accumulators of nodes and cut replies.  The search is the one the
        ``OpponentOptions`` of the seven keywords name: without a ``node_budget`` the fixed-depth one
        (``crl_sim_reply_opponent_q``), with one iterative deepening up to the depths under ``min(node_budget,
        node_limit)`` nodes per reply (``crl_sim_reply_opponent_exc``), ``dev_depth_sum`` the int64 [count] accumulator
        of the completed depths."""
        opts = OpponentOptions(quiescence, node_budget, ordering, repetition, evaluation, selective, exchange,
                               ranges=False)
        vp = ctypes.c_void_p
        if opts.node_budget is None:
            self._ck(self._L.crl_sim_reply_opponent_q(self._h, vp(dev_depths), opts.quiescence, int(node_limit),
                                                      vp(dev_planes_s2), vp(dev_nodes), vp(dev_cuts)),
                     "crl_sim_reply_opponent_q")
        else:
            self._ck(self._L.crl_sim_reply_opponent_exc(self._h, vp(dev_depths), opts.quiescence,
                                                        *opts.budgeted_args(node_limit), vp(dev_planes_s2),
                                                        vp(dev_nodes), vp(dev_cuts), vp(dev_depth_sum)),
                     "crl_sim_reply_opponent_exc")

    def sim_backup(self, dev_policy_s2, dev_value_s2):
        self._ck(self._L.crl_sim_backup(self._h, ctypes.c_void_p(dev_policy_s2),
                                        ctypes.c_void_p(dev_value_s2)), "crl_sim_backup")

    def root_children(self, fields=None):
        """Root children statistics in CHILDREN order; ``fields`` limits what is copied back."""
        G = self.G
        spec = {
            "nchild": ((G,), np.int32), "visits": ((G, MAX_MOVES), np.int32),
            "values": ((G, MAX_MOVES), np.float64), "priors": ((G, MAX_MOVES), np.float32),
            "moves": ((G, MAX_MOVES), np.uint16), "replies": ((G, MAX_MOVES), np.uint16),
            "root_visits": ((G,), np.int32),
        }
        out = {k: (np.zeros(sh, dt) if (fields is None or k in fields) else None)
               for k, (sh, dt) in spec.items()}
        self._ck(self._L.crl_root_children(
            self._h, _ptr(out["nchild"]), _ptr(out["visits"]), _ptr(out["values"]), _ptr(out["priors"]),
            _ptr(out["moves"]), _ptr(out["replies"]), _ptr(out["root_visits"])), "crl_root_children")
        return out

    def advance(self, chosen):
        c = np.ascontiguousarray(chosen, dtype=np.int32)
        assert c.shape == (self.G,)
        bm = np.zeros(self.G, np.uint16)
        am = np.zeros(self.G, np.uint16)
        self._ck(self._L.crl_advance(self._h, _ptr(c), _ptr(bm), _ptr(am)), "crl_advance")
        return bm, am

    def advance_one(self, chosen):
        """``advance`` by ONE ply: our move is played and the stored reply is not (the other side moves for itself);
        returns bm."""
        c = np.ascontiguousarray(chosen, dtype=np.int32)
        assert c.shape == (self.G,)
        bm = np.zeros(self.G, np.uint16)
        self._ck(self._L.crl_advance_one(self._h, _ptr(c), _ptr(bm)), "crl_advance_one")
        return bm

    def advance_one_argmax(self, mover_white, dev_ply_limit, dev_bm, dev_chosen):
        """The noise-free one-ply boundary on the device (``crl_advance_one_argmax``): device int32 [G] ply limits in,
        device uint16 [G] moves and int32 [G] chosen children out; asynchronous."""
        self._ck(self._L.crl_advance_one_argmax(
            self._h, 1 if mover_white else 0, _Dev(dev_ply_limit, "dev_ply_limit").p, _Dev(dev_bm, "dev_bm").p,
            _Dev(dev_chosen, "dev_chosen").p), "crl_advance_one_argmax")

    def end_move_fetch(self, dev_policy_s2, dev_value_s2):
        """sim_backup + root children (nchild, visits, root_visits) + plies in one synchronising call."""
        G = self.G
        nchild, root_visits, plies = (np.zeros(G, np.int32) for _ in range(3))
        visits = np.zeros((G, MAX_MOVES), np.int32)
        self._ck(self._L.crl_end_move_fetch(self._h, ctypes.c_void_p(dev_policy_s2), ctypes.c_void_p(dev_value_s2),
                                            _ptr(nchild), _ptr(visits), _ptr(root_visits), _ptr(plies)),
                 "crl_end_move_fetch")
        return nchild, visits, root_visits, plies

    def advance_fetch(self, chosen):
        """advance + results + legal-move counts of the next roots in one synchronising call."""
        c = np.ascontiguousarray(chosen, dtype=np.int32)
        assert c.shape == (self.G,)
        res = np.zeros(self.G, np.int8)
        counts = np.zeros(self.G, np.int32)
        self._ck(self._L.crl_advance_fetch(self._h, _ptr(c), None, None, _ptr(res), _ptr(counts)), "crl_advance_fetch")
        return res, counts

    def reroot(self, chosen, next_sims):
        """``advance`` that keeps the chosen child's subtree where it fits ``next_sims`` more simulations."""
        c = np.ascontiguousarray(chosen, dtype=np.int32)
        assert c.shape == (self.G,)
        bm = np.zeros(self.G, np.uint16)
        am = np.zeros(self.G, np.uint16)
        self._ck(self._L.crl_reroot(self._h, _ptr(c), int(next_sims), _ptr(bm), _ptr(am)), "crl_reroot")
        return bm, am

    def reroot_fetch(self, chosen, next_sims):
        """reroot + results + legal-move counts of the next roots + kept nodes / kept children per slot
        in one synchronising call; returns a dict."""
        c = np.ascontiguousarray(chosen, dtype=np.int32)
        assert c.shape == (self.G,)
        out = {"bm": np.zeros(self.G, np.uint16), "am": np.zeros(self.G, np.uint16),
               "results": np.zeros(self.G, np.int8), "legal_counts": np.zeros(self.G, np.int32),
               "kept_nodes": np.zeros(self.G, np.int32), "kept_children": np.zeros(self.G, np.int32)}
        self._ck(self._L.crl_reroot_fetch(self._h, _ptr(c), int(next_sims), _ptr(out["bm"]), _ptr(out["am"]),
                                          _ptr(out["results"]), _ptr(out["legal_counts"]), _ptr(out["kept_nodes"]),
                                          _ptr(out["kept_children"])), "crl_reroot_fetch")
        return out

    NODE_DTYPE = np.dtype([("edge0", "<i4"), ("nmoves", "<u2"), ("nexp", "<u2"), ("result", "i1"), ("has_s2", "u1"),
                           ("parent", "<u2"), ("parent_edge", "<i4"), ("rest", "V160")])
    EDGE_DTYPE = np.dtype([("value", "<f8"), ("visits", "<i4"), ("prior", "<f4"), ("move", "<u2"), ("child", "<u2"),
                           ("hint", "<u4")])

    def fetch_tree(self, slot):
        """Debug read-back of one slot's tree (csrc/state.hpp records): (nodes, edges, info) with
        info = {n_nodes, edge_top, root_visits, kept}; empty arrays when the slot has no live tree."""
        cap_n = self.max_sims + 1
        nodes = np.zeros(cap_n, self.NODE_DTYPE)
        edges = np.zeros(cap_n * 218, self.EDGE_DTYPE)
        info = np.zeros(4, np.int32)
        self._ck(self._L.crl_fetch_tree(self._h, int(slot), _ptr(nodes), cap_n, _ptr(edges), len(edges), _ptr(info)),
                 "crl_fetch_tree")
        self.sync()
        return (nodes[:info[0]], edges[:info[1]],
                {"n_nodes": int(info[0]), "edge_top": int(info[1]), "root_visits": int(info[2]), "kept": int(info[3])})

    # ---- random playouts (simulation.py:19-34, mctree.py:272-274) ------------------------------
    def rollout_games(self, words, counts, chunks, max_moves, played=None):
        """The in-slot form: every slot of the window plays its own game on with the 32-bit words of its row;
        returns (played, used, chunk_results) -- plies of the run so far, words consumed by this call, and
        Game.get_result() after every chunk of ``max_moves`` plies.  ``played``: what an earlier call of the
        same run returned (a slot that ran out of words is resumed with the following words)."""
        w = np.ascontiguousarray(words, dtype=np.uint32)
        c = np.ascontiguousarray(counts, dtype=np.int32)
        assert w.ndim == 2 and w.shape[0] == self.G and w.shape[1] >= 1 and c.shape == (self.G,)
        played = np.zeros(self.G, np.int32) if played is None else np.array(played, dtype=np.int32)
        assert played.shape == (self.G,)
        used = np.zeros(self.G, np.int32)
        res = np.zeros((self.G, max(int(chunks), 1)), np.int8)
        self._ck(self._L.crl_rollout_games(self._h, _ptr(w), _ptr(c), w.shape[1], int(chunks), int(max_moves),
                                           _ptr(played), _ptr(used), _ptr(res)), "crl_rollout_games")
        return played, used, res

    def rollout(self, root_source, repetitions, max_moves, dev_keys, dev_value, dev_results=None, dev_plies=None):
        """The private form (enqueue only): ``repetitions`` independent playouts from every root; all arguments
        but the three integers are device addresses (keys uint64 [G], value f32 [G], results int8 / plies
        uint16 [G][repetitions], optional)."""
        vp = ctypes.c_void_p
        self._ck(self._L.crl_rollout(self._h, int(root_source), int(repetitions), int(max_moves), vp(dev_keys),
                                     vp(dev_value), vp(dev_results), vp(dev_plies)), "crl_rollout")

    # ---- the built-in opponent (csrc/opponent.hpp; stockfish.py:23-31, gamestockfish.py:27-41) ------
    def opponent_moves(self, depths, push=False, node_limit=OPP_NODE_LIMIT, quiescence=0, node_budget=None,
                       ordering=False, repetition=False, evaluation="material", selective=False, exchange=False):
        """Alpha-beta per slot of the window: ``depths[g]`` = 0 leaves slot g alone, 1..5 searches it, with the search
        the ``OpponentOptions`` of the seven keywords name (one value of each per call).  Without a ``node_budget``:
        the fixed-depth search (``crl_opponent_moves_q``); returns (moves u16, scores i32, nodes i64, flags u8).  With
        one: iterative deepening, ``depths`` the maximum depths, under ``min(node_budget, node_limit)`` nodes per slot
        (``crl_opponent_moves_exc``); returns (moves, scores, nodes, flags, depths_done i32).  With ``push`` the moves
        are played."""
        opts = OpponentOptions(quiescence, node_budget, ordering, repetition, evaluation, selective, exchange,
                               ranges=False)
        dp = np.ascontiguousarray(depths, dtype=np.int32)
        assert dp.shape == (self.G,)
        moves = np.zeros(self.G, np.uint16)
        scores = np.zeros(self.G, np.int32)
        nodes = np.zeros(self.G, np.int64)
        flags = np.zeros(self.G, np.uint8)
        if opts.node_budget is None:
            self._ck(self._L.crl_opponent_moves_q(self._h, _ptr(dp), opts.quiescence, 1 if push else 0,
                                                  int(node_limit), _ptr(moves), _ptr(scores), _ptr(nodes),
                                                  _ptr(flags)), "crl_opponent_moves_q")
            return moves, scores, nodes, flags
        done = np.zeros(self.G, np.int32)
        self._ck(self._L.crl_opponent_moves_exc(self._h, _ptr(dp), opts.quiescence, 1 if push else 0,
                                                *opts.budgeted_args(node_limit), _ptr(moves), _ptr(scores),
                                                _ptr(nodes), _ptr(flags), _ptr(done)), "crl_opponent_moves_exc")
        return moves, scores, nodes, flags, done

    def opponent_evaluate(self, evaluation="material"):
        """The static evaluation (int32 [G], from the side to move) of every window slot's current position:
        "material" is STATIC EVALUATION of csrc/opponent.hpp, "positional" its EVALUATION.  No search."""
        kind = OPP_EVALUATIONS[evaluation_name(evaluation)]
        scores = np.zeros(self.G, np.int32)
        self._ck(self._L.crl_opponent_evaluate(self._h, kind, _ptr(scores)), "crl_opponent_evaluate")
        return scores

    def opponent_exchange(self):
        """The exchange test of csrc/opponent.hpp, EXCHANGE, alone and without a search, for every legal move of every
        window slot's current position: (bits uint8 [G][MAX_MOVES], counts int32 [G]).  ``bits[g, i]`` belongs to move
        i of ``legal_moves()``: bit 0 = the move is tactical, bit 1 = the test keeps it (static exchange value >= 0;
        always set for a move that is not tactical); entries from ``counts[g]`` on are 0."""
        bits = np.zeros((self.G, MAX_MOVES), np.uint8)
        counts = np.zeros(self.G, np.int32)
        self._ck(self._L.crl_opponent_exchange(self._h, _ptr(bits), _ptr(counts)), "crl_opponent_exchange")
        return bits, counts

    # ---- threads > 1: virtual-loss waves (csrc/search_wave.hpp) -----------------------------------
    def wave_config(self, threads):
        """Allocate the wave arrays for ``threads`` leaves per game and wave (1..64)."""
        self._ck(self._L.crl_wave_config(self._h, int(threads)), "crl_wave_config")

    def wave_begin(self, n_sims):
        """After search_begin + search_root_priors: every live slot gets a budget of ``n_sims`` simulations."""
        self._ck(self._L.crl_wave_begin(self._h, int(n_sims)), "crl_wave_begin")

    def wave_select(self, dev_policy_s2, dev_value_s2, dev_planes_s1):
        vp = ctypes.c_void_p
        self._ck(self._L.crl_wave_select(self._h, vp(dev_policy_s2), vp(dev_value_s2), vp(dev_planes_s1)), "crl_wave_select")

    def wave_reply(self, dev_policy_s1, dev_planes_s2):
        self._ck(self._L.crl_wave_reply(self._h, ctypes.c_void_p(dev_policy_s1), ctypes.c_void_p(dev_planes_s2)), "crl_wave_reply")

    def wave_backup(self, dev_policy_s2, dev_value_s2):
        self._ck(self._L.crl_wave_backup(self._h, ctypes.c_void_p(dev_policy_s2), ctypes.c_void_p(dev_value_s2)), "crl_wave_backup")

    def wave_remaining(self):
        """The largest budget not yet selected over the window (synchronises); 0: only wave_backup is left."""
        n = np.zeros(1, np.int32)
        self._ck(self._L.crl_wave_remaining(self._h, _ptr(n)), "crl_wave_remaining")
        return int(n[0])

    def wave_stats(self):
        """Per window slot since wave_begin: {waves, short_waves, leaves} (synchronises)."""
        out = {k: np.zeros(self.G, np.int32) for k in ("waves", "short_waves", "leaves")}
        self._ck(self._L.crl_wave_stats(self._h, _ptr(out["waves"]), _ptr(out["short_waves"]), _ptr(out["leaves"])), "crl_wave_stats")
        return out

    def counters(self):
        c = np.zeros(6, dtype=np.uint64)
        self._ck(self._L.crl_counters(self._h, _ptr(c)), "crl_counters")
        return dict(zip(("sims", "nodes", "depth_sum", "branch_sum", "evals", "terminal_hits"),
                        (int(x) for x in c)))
