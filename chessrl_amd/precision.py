"""The precision rules of ``ChessModel`` as pure functions of numbers and small tensors (CPU or device): which
arithmetic a weight set runs in, how far the hybrid mode's reply margin is widened, which boards its reply rule
lists.  The thresholds are ``ChessModel``'s class attributes, read there at decision time and passed in; the state
(``precision``, ``reply_margin``, ``guard`` ...) stays on the model."""
import numpy as np
import torch


def log_distance(pa, pb):
    """max |log pa - log pb| over the entries both arithmetics can speak about: pb above 1e-12 AND pa > 0 (an f16
    policy entry that underflowed to 0 has log -inf: the distance would be infinite, the margin with it, and every
    S1 board would be evaluated twice until the next weight set).  None when no entry qualifies."""
    ok = (pb > 1e-12) & (pa > 0)
    if not bool(ok.any()):
        return None
    d = float((pa[ok].log() - pb[ok].log()).abs().max())
    return d if np.isfinite(d) else None


def probe_tolerance(tol, sticky_factor, guard_fired):
    """A run whose guard has fired once stays strict across reloads unless a later weight set passes the probe WITH
    margin (``sticky_factor`` x the tolerance): a net at the edge would otherwise flip f16 <-> hybrid -- and
    re-capture every engine's graphs -- at each reload."""
    return tol * (sticky_factor if guard_fired else 1.0)


def choose_mode(requested, dp, dv, tol, strict):
    """The mode a weight set runs in: the one asked for by name, or for "auto" the single-MFMA "f16" only if its
    policy and value distances to "f16x3" on the probe (``dp``, ``dv``) both stay within ``tol``; ``strict``
    otherwise (a NaN distance is not within anything)."""
    if requested != "auto":
        return requested
    return "f16" if (dp <= tol and dv <= tol) else strict


def widened_margin(margin, probe_margin, dlog, k, cap):
    """(the reply margin after a run's own positions measured ``dlog``, whether the cap cut it): ``k`` x dlog where
    that exceeds the margin in force, but never beyond ``cap`` x the probe's margin -- a margin that wide lists most
    boards anyway, and one outlier (a policy entry at the edge of fp32 underflow in one arithmetic) must not turn
    every S1 evaluation of the rest of the run into f16 + f16x3.  The margin never shrinks."""
    asked = k * dlog
    if not asked > margin:
        return margin, False
    limit = cap * probe_margin
    wider = min(asked, limit)
    return (wider if wider > margin else margin), asked > limit


def reply_rule(p16, p48, counts, margin):
    """The hybrid mode's reply rule on legal priors [n,256] of both arithmetics and the boards' legal-move counts [n]:
    masks ``listed`` (at least two legal moves and the two best closer than ``margin`` in log p of f16: evaluated
    again in f16x3; a NaN gap is listed, as in k_reply_margin), ``differ`` (the argmax over the legal moves is another
    in f16x3), ``unlisted`` (differs without being listed: a failure of the rule), and ``gap`` itself."""
    legal = torch.arange(p16.shape[1], device=p16.device)[None, :] < counts[:, None]
    p16 = torch.where(legal, p16, torch.full_like(p16, -1.0))
    p48 = torch.where(legal, p48, torch.full_like(p48, -1.0))
    a16, a48 = p16.argmax(dim=1), p48.argmax(dim=1)              # (first maximum, as np.argmax / the kernels take it)
    top2 = p16.topk(2, dim=1).values
    gap = torch.log(top2[:, 0].clamp_min(1e-38)) - torch.log(top2[:, 1].clamp_min(1e-38))
    listed = (counts >= 2) & ~(gap >= float(margin))
    differ = (a16 != a48) & (counts >= 2)
    return listed, differ, differ & ~listed, gap
