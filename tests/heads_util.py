"""Weight sets and head-activation sets shared by tests/test_heads_reference.py (CPU) and
tests/test_gpu_heads_arith.py (GPU): every set is a plain function of its seed, built with numpy float64 on the host."""
import numpy as np

from oracle import tower_oracle

SEED = 21
ROWS = 37                    # activation rows of the kernel-local tests (x 8 label windows = 296 boards: 18.5 blocks)
PEAKED_SPREAD = 42.0         # min over boards of (max logit - min logit): "peaked" >= 40, and all of fp32's normal range
HUGE_SPREAD = 210.0          # "huge" >= 200: most labels underflow
VALUE_Z = 12.5               # "spread-value": max |z| >= 12 (tanh saturates at +-1 in fp32 from |z| ~ 9)


def flat_weights(seed=SEED):
    """Keras-initialised 2 x 64 tower with the non-trivial dense biases of
    test_gpu_search.py::test_mfma_dense_heads_match_the_fp32_dense_layers."""
    w = tower_oracle.init_weights(2, 64, seed=seed, randomize_bn=True)
    rng = np.random.default_rng(1000)
    w["policy.dense.bias"] = rng.normal(0, 0.5, 1968).astype(np.float32)
    w["value.dense1.bias"] = rng.normal(0, 0.2, 256).astype(np.float32)
    w["value.dense2.bias"] = np.array([0.3], np.float32)
    return w


def activations(n, kind="base", seed=5):
    """fp32 [n][192] head activations (ReLU outputs): |N(0, 1.5)| with every 7th column zero ("base"), the same
    scaled to ~1e-3 ("tiny": lo, and the smaller hi, in fp16 subnormals) or to ~1e3 ("big")."""
    rng = np.random.default_rng(seed)
    a = np.abs(rng.normal(0, 1.5, (n, 192)))
    a[:, ::7] = 0
    a *= {"base": 1.0, "tiny": 1e-3, "big": 1e3}[kind]
    return a.astype(np.float32)


def logit_spread(w, act):
    """[n] max - min of the float64 logits of fp32 activations act [n][192] under weights w."""
    lg = act[:, :128].astype(np.float64) @ np.asarray(w["policy.dense.kernel"], np.float64) \
        + np.asarray(w["policy.dense.bias"], np.float64)
    return lg.max(1) - lg.min(1)


def scaled_policy(w, act, min_spread, stat=np.min):
    """A copy of w whose policy.dense.kernel is scaled so that every row of act has a logit spread >= min_spread
    (and the least peaked row about that); with another ``stat`` (np.median) that statistic of the rows' spreads."""
    out = dict(w)
    k0 = np.asarray(w["policy.dense.kernel"], np.float64)
    scale = 1.0
    for _ in range(20):
        out["policy.dense.kernel"] = (k0 * scale).astype(np.float32)
        s = stat(logit_spread(out, act))
        if min_spread <= s <= 1.02 * min_spread:
            break
        scale *= 1.01 * min_spread / s
    assert stat(logit_spread(out, act)) >= min_spread
    return out


def value_z(w, act):
    """[n] float64 argument of the value head's tanh."""
    h = act[:, 128:].astype(np.float64) @ np.asarray(w["value.dense1.kernel"], np.float64) \
        + np.asarray(w["value.dense1.bias"], np.float64)
    return np.maximum(h, 0) @ np.asarray(w["value.dense2.kernel"], np.float64).reshape(-1) \
        + float(np.asarray(w["value.dense2.bias"]).reshape(-1)[0])


def spread_value(w, act, max_z=VALUE_Z):
    """A copy of w whose value.dense2.kernel is scaled, and its bias set, so that z over act runs from -max_z to
    +max_z (the head activations are ReLU outputs: unshifted, z is mostly of one sign)."""
    out = dict(w)
    out["value.dense2.bias"] = np.zeros(1, np.float32)
    z = value_z(out, act)
    k = 2 * max_z / (z.max() - z.min())
    out["value.dense2.kernel"] = (np.asarray(w["value.dense2.kernel"], np.float64) * k).astype(np.float32)
    out["value.dense2.bias"] = np.array([-k * (z.max() + z.min()) / 2], np.float32)
    return out
