"""Cases and float64 numpy references of the gradient quantizer, shared by
test_quantize_reference_cpu.py (the host learner, device_type=cpu) and test_quantize_kernels.py
(k_qmax, k_quantize and k_leaf_true_sums, src/device/seq_hist_kernels.hip and
seq_vote_kernels.hip, through ops.quantize_gradients and device_type=gpu).

The quantizer's definition (reference gradient_discretizer.cpp), everything in float64:

    mg = float64(max |g| as float32)            gs = mg / (bins // 2)
    mh = float64(max |h| as float32)            hs = mh if the hessian is constant else mh / bins
    x  = float64(g) * (1 / gs)
    deterministic level    sign(g) * floor(|x| + 0.5)
    stochastic level       sign(g) * (floor(|x|) + 1 with probability frac(|x|), else floor(|x|))
    de-quantized value     float32(level * gs)                       (h likewise, never negative)

tests/cpp/test_native.cpp TestGradientQuantizerLevels holds the same formulas against the host's
GradientQuantizer. This module imports no library: the test files hand over their
`lambdagap_amd` module. Data is built once per process (lru_cache) and never changed.

Kernel shapes the sizes are chosen around:
  * k_qmax reads two rows per 16-byte load: one tail row when n is odd, and one leading row when
    the class slice starts 8-byte but not 16-byte aligned (class 1 of a multiclass model with n
    odd); its four-deep unrolled loop runs only when n > 8 * 256 * grid with
    grid = min(ceil(n / 256), 4 * CUs);
  * k_quantize packs the levels as int8 g << 8 | uint8 h: -127, 127 and 254 at 254 bins.
"""
import functools

import numpy as np

N = 100_001
DATASET_PARAMS = {"max_bin": 15, "min_data_in_bin": 1, "verbosity": -1}
DETERMINISTIC_BINS = (4, 5, 16, 254)
STOCHASTIC_BINS = (4, 16, 254)
# a level is compared only where the scaled value's fractional part is at least this far from the
# rounding tie: the kernel may fuse x * (1 / gs) + 0.5, which differs from the reference's
# separately rounded product by half an ulp of x (< 2^-45 at |x| <= 254)
TIE_MARGIN = 1e-9
MAX_TIE_SHARE = 1e-3
SIGMA = 6.0


@functools.lru_cache(maxsize=None)
def features(n):
    """[n, 2] feature matrix for the Dataset the device learner is built on (never read by the
    quantizer; two columns so that the learner has something to lay out)."""
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, 2))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def logistic_gradients(n, seed=0):
    """(g, h) float32 of a logistic model: p - y and p (1 - p)."""
    rng = np.random.default_rng(1000 + seed)
    p = 1.0 / (1.0 + np.exp(-1.5 * rng.standard_normal(n)))
    y = (rng.random(n) < 0.5).astype(np.float64)
    g = (p - y).astype(np.float32)
    h = (p * (1.0 - p)).astype(np.float32)
    g.setflags(write=False)
    h.setflags(write=False)
    return g, h


def with_maxima(g, h, g_row, h_row, scale=1.0):
    """Copies of (g, h) whose max |g| sits at g_row alone and whose max |h| at h_row alone
    (logistic |g| < 1 and h <= 0.25)."""
    g, h = g.copy(), h.copy()
    g[g_row] = np.float32(-1.37 * scale if g_row % 2 else 1.37 * scale)
    h[h_row] = np.float32(0.31 * scale)
    return g, h


def scales(g, h, bins, const_hess=False):
    """(mg, mh, gs, hs) in float64 from float32 inputs."""
    mg = float(np.abs(np.asarray(g, dtype=np.float32)).max()) if len(g) else 0.0
    mh = float(np.abs(np.asarray(h, dtype=np.float32)).max()) if len(h) else 0.0
    return mg, mh, mg / (bins // 2), (mh if const_hess else mh / bins)


def scaled(v, s):
    """|x| = |float64(v) * (1 / s)| (0 where the scale is 0)."""
    inv = 1.0 / s if s > 0 else 0.0
    return np.abs(np.asarray(v, dtype=np.float32).astype(np.float64) * inv)


def sign(v):
    return np.where(np.asarray(v) < 0, -1, 1).astype(np.int64)


def deterministic_levels(v, s):
    """(levels int64, clear) where clear marks the rows at least TIE_MARGIN away from a tie."""
    x = scaled(v, s)
    fl = np.floor(x)
    clear = np.abs((x - fl) - 0.5) > TIE_MARGIN
    return sign(v) * np.floor(x + 0.5).astype(np.int64), clear


def dequantized(levels, s):
    return (np.asarray(levels, dtype=np.float64) * s).astype(np.float32)


def packed(g_levels, h_levels):
    """int8(g level) << 8 | uint8(h level) as uint16."""
    return (((np.asarray(g_levels, dtype=np.int64) & 0xFF) << 8) | (np.asarray(h_levels, dtype=np.int64) & 0xFF)
            ).astype(np.uint16)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


# ------------------------------------------------------------------ stochastic rounding
def rounding_residuals(v, levels, s):
    """(f, up): the fractional part of |x| and whether the level was rounded away from zero.
    Asserts that every level is floor(|x|) or floor(|x|) + 1 with the value's sign."""
    x = scaled(v, s)
    fl = np.floor(x)
    mag = np.abs(np.asarray(levels, dtype=np.int64))
    up = mag - fl.astype(np.int64)
    bad = np.flatnonzero((up != 0) & (up != 1))
    assert bad.size == 0, (bad[:5], x[bad[:5]], np.asarray(levels)[bad[:5]])
    wrong_sign = np.flatnonzero((mag > 0) & (np.sign(levels) != sign(v)))
    assert wrong_sign.size == 0, wrong_sign[:5]
    return x - fl, up.astype(np.float64)


def z_score(resid, var):
    """sum(resid) / sqrt(sum(var)); 0 when nothing can vary."""
    tot = float(np.sum(var))
    return float(np.sum(resid)) / np.sqrt(tot) if tot > 0 else 0.0


def unbiased_statistics(f, up):
    """{name: z} of sum(up - f) / sqrt(sum f (1 - f)) over all rows and over the ten deciles of f
    that hold at least 100 rows: each is a sum of independent zero-mean terms under unbiased
    stochastic rounding, so |z| stays within a few units."""
    r, var = up - f, f * (1.0 - f)
    out = {"all": z_score(r, var)}
    dec = np.minimum((f * 10).astype(np.int64), 9)
    for d in range(10):
        m = dec == d
        if m.sum() >= 100:
            out[f"decile{d}"] = z_score(r[m], var[m])
    return out


def product_statistic(fa, upa, fb, upb):
    """z of sum (upa - fa)(upb - fb): independent draws make the products zero-mean with variance
    fa (1 - fa) fb (1 - fb)."""
    return z_score((upa - fa) * (upb - fb), fa * (1 - fa) * fb * (1 - fb))


def changed_statistic(f, levels_a, levels_b):
    """z of the number of rows whose level differs between two independent draws of the same
    input: Bernoulli(2 f (1 - f)) per row."""
    p = 2.0 * f * (1.0 - f)
    changed = (np.asarray(levels_a) != np.asarray(levels_b)).astype(np.float64)
    return z_score(changed - p, p * (1.0 - p))


# ------------------------------------------------------------------ renewed leaves (true sums)
RENEW_N = 30_001


@functools.lru_cache(maxsize=None)
def renew_data():
    rng = np.random.default_rng(77)
    X = rng.standard_normal((RENEW_N, 4))
    y = (X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.3 * rng.standard_normal(RENEW_N)).astype(np.float32)
    cls = np.clip(np.floor(1.5 + 0.8 * X[:, 0] + 0.5 * rng.standard_normal(RENEW_N)), 0, 2).astype(np.float32)
    for a in (X, y, cls):
        a.setflags(write=False)
    return X, y, cls


def check_renewed_leaves(lgb, device, bins, objective="regression", extra=None):
    """One tree with use_quantized_grad, quant_train_renew_leaf, boost_from_average=false and
    lambda_l2 = 1: whatever the quantized gradients made of the tree's structure, every leaf value
    is learning_rate * -sum(g) / (sum(h) + lambda_l2) over the true gradients of the leaf's rows.
    regression: g = -y and h = 1 exactly; multiclass (softmax at score 0, three classes):
    g = 1/3 - [y == class] and h = 3/2 * 1/3 * 2/3 = 1/3, both up to their fp32 rounding.
    Tolerance: fp32 gradients (2^-24 relative each, g and h) summed in fp64:
    2^-23 * sum|g| / (sum(h) + lambda_l2) * learning_rate. Returns the booster."""
    X, y, cls = renew_data()
    lr, l2 = 0.1, 1.0
    params = {"objective": objective, "boost_from_average": False, "use_quantized_grad": True,
              "quant_train_renew_leaf": True, "num_grad_quant_bins": bins, "lambda_l2": l2, "learning_rate": lr,
              "num_leaves": 15, "min_data_in_leaf": 20, "device_type": device, "verbosity": -1, "seed": 5}
    if objective == "multiclass":
        params["num_class"] = 3
    params.update(extra or {})
    label = cls if objective == "multiclass" else y
    b = lgb.train(params, lgb.Dataset(X, label, params=params), 1, keep_training_booster=True)
    leaves = np.asarray(b.predict(X, pred_leaf=True)).reshape(RENEW_N, -1)
    ntree = 3 if objective == "multiclass" else 1
    assert b.num_trees() == ntree and leaves.shape[1] == ntree
    for t in range(ntree):
        if objective == "multiclass":
            g = 1.0 / 3.0 - (cls == t).astype(np.float64)
            h = np.full(RENEW_N, 1.0 / 3.0)
        else:
            g = -y.astype(np.float64)
            h = np.ones(RENEW_N)
        ids = np.unique(leaves[:, t])
        assert ids.size > 4, "the tree has leaves to check"
        for leaf in ids:
            m = leaves[:, t] == leaf
            want = -lr * g[m].sum() / (h[m].sum() + l2)
            tol = 2.0 ** -23 * np.abs(g[m]).sum() / (h[m].sum() + l2) * lr
            got = b.get_leaf_output(t, int(leaf))
            assert abs(got - want) <= tol, (t, int(leaf), int(m.sum()), got, want, abs(got - want), tol)
    return b
