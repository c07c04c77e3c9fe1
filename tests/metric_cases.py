"""Cases and float64 / long double numpy references of the metrics that are evaluated on given
scores, shared by test_metric_reference_cpu.py (the host metrics, device_type=cpu) and
test_metric_kernels.py (the HIP kernels k_metric_partial / k_multi_metric_partial / k_metric_fold of
src/device/grad_kernels.hip, k_auc_prep / k_auc_terms / k_auc_fold / k_aucmu_pair and the rocPRIM
passes of src/device/metric_kernels.hip, device_type=gpu).

The references are written from the definitions: the reference project's regression_metric.hpp,
binary_metric.hpp, xentropy_metric.hpp, multiclass_metric.hpp and the objectives' ConvertOutput;
not from include/lgap/pointwise_metric.h, which the host metric and the kernel share. Row terms
are computed in np.longdouble over the float32 labels and weights the library stores and the float64
scores, and summed exactly (math.fsum over the high and low halves of every term).

This module imports no library: the test files hand their `lambdagap_amd` module to the check_*
functions. Data and references are built once per process (lru_cache) and never changed. The scores
are handed in as init_score and evaluated before any tree, as rank_cases._booster does.

Row counts: every family at 1, 255, 256, 257 and 4099 rows (one block less one row, one block, one
block and a row, seventeen blocks), and one case per family across its grid: 600 011 and 262 145
rows for the pointwise and multiclass kernels (1024 blocks of 256), 1 048 577 + 313 rows of distinct
scores for AUC / average precision (k_auc_prep's 4096 x 256, k_auc_terms' 512 x 256). auc_mu needs a
row of every class (an empty class is not this module's subject), so its smallest case has one row
per class where the others have one row.

Error bounds
  Sums of non-negative terms (AUC, average precision, auc_mu, weighted error rates): any summation
  order errs by at most (n - 1) * 2^-53 relative, three nested sums (the tie group's aggregate, the
  prefix, the terms) by 3 * n * 2^-53. With unit weights every AUC accumulator is an integer or a
  half-integer below 2^53 and only the final division and product round: 4 * 2^-53.
  Pointwise and multiclass losses:
      |got - ref| * sumw <= C * 2^-53 * sum_i w_i * m_i + n * 2^-53 * sum_i w_i * |term_i|
  m_i, the row's magnitude, is the sum of the absolute values of the addends of the row's loss before
  they cancel, times the factor by which a rounding of an intermediate value is amplified (below,
  next to every loss); the second term is the summation in any order. C is the cost of the libm
  calls per row in roundings, measured on the host (C_HOST).
  The amplification factors make m_i larger than the plain sum of absolute addends, and the bound
  wider by as much: p / (1 - p) for log(1 - p) of a rounded sigmoid (binary_logloss, the cross
  entropies), 1 / p and 1 / (1 - p) for cross_entropy_lambda's p = 1 - exp(-w h), 1 + |e| for
  tweedie's exp(e), + 1 for the log of a probability that carries a relative rounding. Without them
  the definition evaluated in float64 would miss its own bound: at sigmoid 2.5 and a raw score of 4,
  1 - p = 4.5e-5 is known to 2^-53 / 4.5e-5 only. A single saturated row (raw 40, label 1: a loss of
  4e-18 beside a rounding of 1e-16) has m_i / |term_i| up to 5e17; over the sets of 255 rows and
  more sum w m / sum w |term| is at most 3.7 for binary_logloss, 2.6 cross_entropy, 3.0
  kullback_leibler, 43 cross_entropy_lambda, 7.3 tweedie, 2.0 multi_logloss.
"""
import contextlib
import fractions
import functools
import math
import os

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
METRIC_RTOL = 1e-12  # device against host on the same booster (test_device_metrics.py, rank_cases.METRIC_RTOL)

# constants of the reference, with the types they have there
K_EPSILON = LD(np.float32(1e-15))  # meta.h: const score_t kEpsilon = 1e-15f, promoted in `p > kEpsilon`
# `return -std::log(kEpsilon)`: the float overload of a float argument, its float result widened
CLAMP_LOSS = LD(np.float32(-np.log(np.float32(1e-15))))
EPS_1E10F = LD(np.float32(1e-10))  # regression_metric.hpp: const double eps = 1e-10f
XENT_EPS = LD(1.0e-12)  # xentropy_metric.hpp: log_arg_epsilon
GAMMA_DEV_EPS = LD(1.0e-9)

SIZES = (1, 255, 256, 257, 4099)
# the validation set of the case with SIZES[i] training rows
VALID_SIZES = (4099, 1, 255, 256, 257)
GRID_TRAIN, GRID_VALID = 600_011, 262_145
AUC_GRID = 1_048_577 + 313

ALPHA, FAIR_C, TWEEDIE_RHO = 0.75, 1.5, 1.3  # non-default, exact in binary

POINTWISE_KINDS = ["l2", "rmse", "l1", "quantile", "huber", "fair", "poisson", "mape", "gamma", "gamma_deviance",
                   "tweedie", "binary_logloss", "binary_error", "cross_entropy", "cross_entropy_lambda",
                   "kullback_leibler"]

_REG = {"alpha": ALPHA, "fair_c": FAIR_C}
# setting -> (objective parameters, output transform, sigmoid, metrics, labels)
SETTINGS = {
    "regression": ({"objective": "regression", **_REG}, "identity", 1.0,
                   ["l2", "rmse", "l1", "quantile", "huber", "fair", "mape"], "real"),
    "reg_sqrt": ({"objective": "regression", "reg_sqrt": True, **_REG}, "signed_square", 1.0,
                 ["l2", "rmse", "l1", "quantile", "huber", "fair", "mape"], "real"),
    "binary1": ({"objective": "binary", "sigmoid": 1.0}, "sigmoid", 1.0, ["binary_logloss", "binary_error"], "binary"),
    "binary2.5": ({"objective": "binary", "sigmoid": 2.5}, "sigmoid", 2.5, ["binary_logloss", "binary_error"], "binary"),
    "poisson": ({"objective": "poisson"}, "exp", 1.0, ["poisson"], "count"),
    "gamma": ({"objective": "gamma"}, "exp", 1.0, ["gamma", "gamma_deviance"], "positive"),
    "tweedie": ({"objective": "tweedie", "tweedie_variance_power": TWEEDIE_RHO}, "exp", 1.0, ["tweedie"], "count"),
    "cross_entropy": ({"objective": "cross_entropy"}, "sigmoid", 1.0, ["cross_entropy", "kullback_leibler"], "unit"),
    "cross_entropy_lambda": ({"objective": "cross_entropy_lambda"}, "log1pexp", 1.0, ["cross_entropy_lambda"], "unit"),
}
assert {m for s in SETTINGS.values() for m in s[3]} == set(POINTWISE_KINDS)


def exact_sum(t):
    """The sum of long double values, rounded once: fsum over their high and low float64 halves."""
    t = np.asarray(t, dtype=LD).ravel()
    hi = t.astype(np.float64)
    lo = (t - hi.astype(LD)).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist())


def _seed(name):
    return 9000 + sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100000


# ------------------------------------------------------------------ pointwise reference
def convert_output(transform, raw, sigmoid):
    """The objectives' ConvertOutput in long double."""
    r = np.asarray(raw, dtype=np.float64).astype(LD)
    with np.errstate(over="ignore"):
        if transform == "identity":
            return r
        if transform == "signed_square":  # RegressionL2loss with sqrt: Sign(x) * x * x
            return np.sign(r) * r * r
        if transform == "sigmoid":  # BinaryLogloss / CrossEntropy: 1 / (1 + exp(-sigmoid * x))
            return 1 / (1 + np.exp(-LD(sigmoid) * r))
        if transform == "exp":  # Poisson / Gamma / Tweedie
            return np.exp(r)
        if transform == "log1pexp":  # CrossEntropyLambda
            return np.log1p(np.exp(r))
    raise KeyError(transform)


def _safe_log(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x > 0, np.log(np.where(x > 0, x, 1)), -np.inf)


def _xent(y, p, amp_p, amp_q):
    """XentLoss(label, prob) -> (loss, magnitude). a and b are both <= 0 and do not cancel; a rounding
    of p (2^-53 * amp_p absolute) moves log p by 2^-53 * amp_p / p, one of 1 - p moves log(1 - p) by
    2^-53 * amp_q / (1 - p)."""
    q = 1 - p
    pa, qa = p > XENT_EPS, q > XENT_EPS
    a = y * np.where(pa, _safe_log(np.where(pa, p, 1)), np.log(XENT_EPS))
    b = (1 - y) * np.where(qa, _safe_log(np.where(qa, q, 1)), np.log(XENT_EPS))
    m = np.abs(a) + np.abs(b) + y * np.where(pa, amp_p / np.where(pa, p, 1), 0) + (1 - y) * np.where(qa, amp_q / np.where(qa, q, 1), 0)
    return -(a + b), m


def row_loss(kind, y, s, w):
    """(loss, magnitude) per row in long double: LossOnPoint of `kind` at the converted score s.
    w only enters cross_entropy_lambda."""
    one = LD(1)
    if kind in ("l2", "rmse"):  # (s - y)^2 = s^2 - 2 s y + y^2
        d = s - y
        return d * d, (np.abs(s) + np.abs(y)) ** 2
    if kind == "l1":
        return np.abs(s - y), np.abs(s) + np.abs(y)
    if kind == "quantile":
        delta = y - s
        coef = np.where(delta < 0, LD(ALPHA) - 1, LD(ALPHA))
        return coef * delta, np.abs(coef) * (np.abs(s) + np.abs(y))
    if kind == "huber":
        d = s - y
        a = LD(ALPHA)
        quad = np.abs(d) <= a
        size = np.abs(s) + np.abs(y)
        return (np.where(quad, LD(0.5) * d * d, a * (np.abs(d) - LD(0.5) * a)),
                np.where(quad, LD(0.5) * size * size, a * size + LD(0.5) * a * a))
    if kind == "fair":  # c x and c^2 log1p(x / c) cancel to x^2 / 2 for a small x
        x, c = np.abs(s - y), LD(FAIR_C)
        lg = c * c * np.log1p(x / c)
        return c * x - lg, c * (np.abs(s) + np.abs(y)) + lg
    if kind == "poisson":
        s = np.where(s < EPS_1E10F, EPS_1E10F, s)
        t = y * np.log(s)
        return s - t, np.abs(s) + np.abs(t)
    if kind == "mape":
        den = np.maximum(one, np.abs(y))
        return np.abs(y - s) / den, (np.abs(y) + np.abs(s)) / den
    if kind == "gamma":  # psi = 1
        theta = -one / s
        b = -_safe_log(-theta)
        c = _safe_log(y) - _safe_log(y)
        return -((y * theta - b) + c), np.abs(y * theta) + np.abs(b)
    if kind == "gamma_deviance":
        t = y / (s + GAMMA_DEV_EPS)
        lt = _safe_log(t)
        return t - lt - 1, np.abs(t) + np.abs(lt) + 1
    if kind == "tweedie":  # a rounding of the exponent e moves exp(e) by |e| roundings
        rho = LD(TWEEDIE_RHO)
        s = np.where(s < EPS_1E10F, EPS_1E10F, s)
        ea, eb = (1 - rho) * np.log(s), (2 - rho) * np.log(s)
        a = y * np.exp(ea) / (1 - rho)
        b = np.exp(eb) / (2 - rho)
        return -a + b, np.abs(a) * (1 + np.abs(ea)) + np.abs(b) * (1 + np.abs(eb))
    if kind == "binary_logloss":  # a rounding of p moves log(1 - p) by 2^-53 * p / (1 - p)
        q = 1 - s
        neg, qa, pa = y <= 0, q > K_EPSILON, s > K_EPSILON
        clamp = CLAMP_LOSS
        ln = np.where(qa, -_safe_log(np.where(qa, q, 1)), clamp)
        lp = np.where(pa, -_safe_log(np.where(pa, s, 1)), clamp)
        mn = np.where(qa, np.abs(ln) + s / np.where(qa, q, 1), clamp)
        mp = np.where(pa, np.abs(lp) + 1, clamp)
        return np.where(neg, ln, lp), np.where(neg, mn, mp)
    if kind == "binary_error":
        t = np.where(s <= LD(0.5), y > 0, y <= 0).astype(LD)
        return t, t
    if kind in ("cross_entropy", "kullback_leibler"):
        return _xent(y, s, s, s)
    if kind == "cross_entropy_lambda":  # XentLambdaLoss: prob = 1 - exp(-weight * hhat), rounded at size 1
        return _xent(y, 1 - np.exp(-w * s), one, one)
    raise KeyError(kind)


def _yent(y):
    """YentLoss: p log p + (1 - p) log(1 - p), each where its argument is positive."""
    q = 1 - y
    return y * _safe_log(np.where(y > 0, y, 1)) + q * _safe_log(np.where(q > 0, q, 1))


def pointwise_reference(kind, setting, y, raw, w):
    """-> dict(value, sum, scale_m, scale_t, sumw, n): `sum` the weighted loss sum the value is
    finished from, scale_m = sum w_i m_i, scale_t = sum w_i |term_i|."""
    _, transform, sigmoid, _, _ = SETTINGS[setting]
    n = len(raw)
    yl = np.asarray(y, dtype=np.float32).astype(LD)
    wl = np.ones(n, dtype=LD) if w is None else np.asarray(w, dtype=np.float32).astype(LD)
    s = convert_output(transform, raw, sigmoid)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        if kind == "cross_entropy_lambda":  # the weight enters the loss, not the sum
            term, m = row_loss(kind, yl, s, wl)
            wt, wm = term, m
        else:
            term, m = row_loss(kind, yl, s, None)
            wt, wm = term * wl, m * wl
    assert np.all(np.isfinite(wt.astype(np.float64))) and np.all(m >= np.abs(term) * (1 - 1e-15)), (kind, setting)
    total = exact_sum(wt)
    sumw = exact_sum(wl)
    scale_m, scale_t = exact_sum(wm), exact_sum(np.abs(wt))
    ent = 0.0
    if kind == "rmse":
        value = math.sqrt(total / sumw)
    elif kind == "gamma_deviance":
        value = total * 2
    elif kind == "cross_entropy_lambda":
        value = total / n
    elif kind == "kullback_leibler":  # the label entropy is part of the value: its addends join the magnitude
        ye = _yent(yl) * wl
        ent = exact_sum(ye) / sumw
        value = ent + total / sumw
        scale_m += exact_sum(np.abs(ye))
    else:
        value = total / sumw
    return {"value": value, "sum": total, "scale_m": scale_m, "scale_t": scale_t, "sumw": sumw, "n": n, "ent": ent,
            "kind": kind}


def loss_units(ref, got):
    """The deviation of a metric value from its reference in units of 2^-53 * sum w_i m_i, after the
    summation's share n * 2^-53 * sum w_i |term_i| is taken off (0 where that covers it)."""
    kind = ref.get("kind")
    if kind == "rmse":
        total = got * got * ref["sumw"]
    elif kind == "gamma_deviance":
        total = got / 2
    elif kind == "cross_entropy_lambda":
        total = got * ref["n"]
    elif kind == "kullback_leibler":
        total = (got - ref["ent"]) * ref["sumw"]
    else:
        total = got * ref["sumw"]
    assert math.isfinite(got), got
    excess = abs(total - ref["sum"]) - ref["n"] * U * ref["scale_t"]
    if excess <= 0:
        return 0.0
    return excess / (U * ref["scale_m"]) if ref["scale_m"] > 0 else math.inf


# C_HOST: the largest loss_units of the HOST metric (device_type=cpu) over every case of this
# module, per metric kind. Measured on 2026-10-21 with
#   pytest tests/test_metric_reference_cpu.py::test_report_c_host -s
# (x86-64, glibc libm) and rounded up to one decimal; 0.0 where the summation's share covers every
# case, which it does from a few rows on, so the figures come from the sets of one row. The CPU
# tests assert the next power of two, at least 1; the device gets 4 x C_HOST with a floor of 4
# (another libm, another summation order), the margin of rank_cases.device_bound. A wrong branch,
# clamp or sign moves a row by about its own loss: 2^53 of these units.
# (On an MI355X the same day the kernels' largest values were the host's to the last digit: fair
# 0.25, gamma 0.05, tweedie 0.43, multi_logloss 1.50 of their bounds of 4, 4, 4 and 6, every other kind
# 0.0; AUC, average precision and auc_mu reached 0.004 of their bounds, the weighted error rates 0.0.)
C_HOST = {
    "l2": 0.0, "rmse": 0.0, "l1": 0.0, "quantile": 0.0, "huber": 0.0, "fair": 0.3, "poisson": 0.0, "mape": 0.0,
    "gamma": 0.1, "gamma_deviance": 0.0, "tweedie": 0.5, "binary_logloss": 0.0, "binary_error": 0.0,
    "cross_entropy": 0.0, "cross_entropy_lambda": 0.0, "kullback_leibler": 0.0, "multi_logloss": 1.5,
}


def cpu_bound(kind):
    c = C_HOST[kind]
    return 1.0 if c <= 1.0 else 2.0 ** int(np.ceil(np.log2(c)))


def device_bound(kind):
    return max(4.0, 4.0 * C_HOST[kind])


def loss_bound(device, kind):
    return cpu_bound(kind) if device == "cpu" else device_bound(kind)


# ------------------------------------------------------------------ pointwise cases
def _nx(x, up):
    return float(np.nextafter(x, np.inf if up else -np.inf))


# planted rows (label, raw score) per setting
_PLANTED = {
    "regression": [
        (1.5, 2.25), (1.5, _nx(2.25, True)), (1.5, _nx(2.25, False)),  # huber: s - y = alpha and one ulp either side
        (1.5, 0.75), (1.5, _nx(0.75, True)), (1.5, _nx(0.75, False)),  # ... = -alpha
        (0.5, 0.5), (-3.0, -3.0),  # quantile: y == s
        (0.25, 3.0), (-0.5, 1.0), (0.0, 2.0),  # mape: |y| < 1
        (1.0, 1.0 + 1e-9), (1.0, 1.0 + 1e6), (1.0, 1.0 - 1e6),  # fair: |s - y| of 1e-9 and 1e6
        (2.0, 0.5), (0.5, 2.0),  # quantile: both signs
    ],
    "binary": [(0.0, 0.0), (1.0, 0.0), (0.0, -0.0),  # p == 0.5
               (1.0, 40.0), (0.0, 40.0), (1.0, -40.0), (0.0, -40.0),  # p or 1 - p rounds to 0
               (1.0, 800.0), (0.0, 800.0), (1.0, -800.0), (0.0, -800.0)],  # exp overflows: p is exactly 0 or 1
    "count": [(0.0, -30.0), (2.0, -30.0), (0.0, 3.0), (3.0, -23.5)],  # exp(-30) < 1e-10: the clamp
    "positive": [(1.0, 0.0), (2.0, math.log(2.0)), (0.5, math.log(0.5)), (3.0, -2.0)],  # y / s within 1e-8 of 1
    "unit": [(0.0, 0.0), (1.0, 0.0), (0.5, 0.0), (0.0, 40.0), (1.0, 40.0), (0.25, 40.0), (0.0, -40.0), (1.0, -40.0),
             (0.75, -40.0), (0.0, 800.0), (1.0, 800.0), (0.5, 800.0), (0.0, -800.0), (1.0, -800.0), (0.5, -800.0)],
}
_PLANTED["reg_sqrt"] = _PLANTED["regression"]


def _pointwise_data(setting, n, weighted, rng):
    labels = SETTINGS[setting][4]
    z = rng.standard_normal(n)
    raw = rng.standard_normal(n)
    if labels == "real":
        y, raw = 2.0 * z, 2.0 * raw
        y[rng.random(n) < 0.3] *= 0.2  # |y| < 1
    elif labels == "binary":
        y = (z + raw > 0).astype(np.float64)
    elif labels == "count":
        y = rng.poisson(1.5, n).astype(np.float64)
    elif labels == "positive":
        y = np.exp(0.5 * z + raw) + 0.01
        close = rng.random(n) < 0.1  # y / s within 1e-8 of 1, after the label is rounded to float32
        y[close] = np.exp(raw[close])
    else:
        y = rng.random(n)
        y[rng.random(n) < 0.2] = 0.0
        y[rng.random(n) < 0.2] = 1.0
    y = np.asarray(y, dtype=np.float32)
    if labels == "positive":
        raw[close] = np.log(y[close].astype(np.float64)) + rng.uniform(-1e-8, 1e-8, int(close.sum()))
    planted = _PLANTED["reg_sqrt" if setting == "reg_sqrt" else "regression" if labels == "real" else labels]
    k = min(n, len(planted))
    # a set of one row takes a planted row of its own
    first = (n * 7) % len(planted) if n == 1 else 0
    for i in range(k):
        y[i], raw[i] = planted[(first + i) % len(planted)]
    # cross_entropy_lambda wants positive weights; the others take exact zeros too
    w = None
    if weighted:
        w = rng.uniform(0.25, 4.0, n).astype(np.float32)
        if setting != "cross_entropy_lambda":
            w[rng.random(n) < 0.05] = 0.0
            w[0] = 1.5
    X = rng.standard_normal((n, 2)).astype(np.float32)
    return {"X": X, "y": y, "w": w, "s": raw}


def _two_sets(name, make, n_train, n_valid, idx):
    """Training and validation set of a case: different n, scores and weights (one of the two
    weighted, which one alternates with the size)."""
    rng = np.random.default_rng(_seed(name))
    return make(n_train, idx % 2 == 0, rng), make(n_valid, idx % 2 == 1, rng)


POINTWISE_CASES = [f"{s}:{n}" for s in SETTINGS for n in SIZES] + ["regression:grid", "binary2.5:grid"]


@functools.lru_cache(maxsize=None)
def pointwise_case(name):
    """-> dict(params, train, valid, ref_train, ref_valid); ref_*: {metric: pointwise_reference}."""
    setting, size = name.split(":")
    if size == "grid":
        n_train, n_valid, idx = GRID_TRAIN, GRID_VALID, 0
    else:
        idx = SIZES.index(int(size))
        n_train, n_valid = SIZES[idx], VALID_SIZES[idx]
    params, _, _, metrics, _ = SETTINGS[setting]
    train, valid = _two_sets("pointwise" + name, lambda n, wt, rng: _pointwise_data(setting, n, wt, rng), n_train,
                             n_valid, idx)
    out = {"params": dict(params, metric=list(metrics)), "train": train, "valid": valid, "family": "pointwise"}
    for part in ("train", "valid"):
        d = out[part]
        out["ref_" + part] = {m: pointwise_reference(m, setting, d["y"], d["s"], d["w"]) for m in metrics}
    return out


# ------------------------------------------------------------------ multiclass reference
def multiclass_probabilities(objective, raw, sigmoid):
    """ConvertOutput of multiclass (Common::Softmax) / multiclassova in long double; raw is (n, K)."""
    r = np.asarray(raw, dtype=np.float64).astype(LD)
    with np.errstate(over="ignore", under="ignore"):
        if objective == "multiclass":
            e = np.exp(r - r.max(axis=1, keepdims=True))
            return e / e.sum(axis=1, keepdims=True)
        return 1 / (1 + np.exp(-LD(sigmoid) * r))


def multiclass_reference(metric, objective, sigmoid, top_k, y, raw, w):
    """multi_logloss: -log(p_y), clamped at kEpsilon; its magnitude |log p_y| + 1 (p_y carries a few
    roundings of its own size). multi_error@k: 1 where `p_k >= p_y` holds for more than top_k classes
    k, the true class among them."""
    n = len(y)
    yi = np.asarray(y, dtype=np.float32).astype(np.int64)
    wl = np.ones(n, dtype=LD) if w is None else np.asarray(w, dtype=np.float32).astype(LD)
    p = multiclass_probabilities(objective, raw, sigmoid)
    py = p[np.arange(n), yi]
    if metric == "multi_logloss":
        ok = py > K_EPSILON
        term = np.where(ok, -_safe_log(np.where(ok, py, 1)), CLAMP_LOSS)
        m = np.abs(term) + 1
    else:
        larger = (p >= py[:, None]).sum(axis=1)
        term = (larger > top_k).astype(LD)
        m = term
    total, sumw = exact_sum(term * wl), exact_sum(wl)
    return {"value": total / sumw, "sum": total, "scale_m": exact_sum(m * wl), "scale_t": exact_sum(np.abs(term * wl)),
            "sumw": sumw, "n": n, "kind": metric, "unit_weights": w is None}


MULTI_OVA_SIGMOID = 2.0
MULTI_CONFIGS = [(o, k, t) for o in ("multiclass", "multiclassova") for k in (2, 3, 7) for t in sorted({1, 2, k})]
MULTI_CASES = [f"{o}:{k}:{t}:{n}" for o, k, t in MULTI_CONFIGS for n in SIZES] + ["multiclass:7:2:grid", "multiclassova:3:1:grid"]


def _multi_data(K, n, weighted, rng):
    raw = rng.standard_normal((n, K)) * 1.5
    y = rng.integers(0, K, n)
    planted = []
    two = np.zeros(K)
    two[:2] = 1.0
    two[2:] = -1.0
    planted.append((0, two))  # two classes tied at the top, the true one among them
    planted.append((K - 1, np.zeros(K)))  # every class tied, the last one true
    low = np.zeros(K)
    low[0] = 800.0
    planted.append((1, low))  # the true class 800 below the maximum: its softmax probability is 0
    planted.append((1, two))
    planted.append((K - 1, two))  # (K > 2: the true class below a tied pair)
    planted.append((0, low))
    for c in range(K):  # every class is a label
        planted.append((c, rng.standard_normal(K)))
    first = (K * 5) % len(planted) if n == 1 else 0
    for i in range(min(n, len(planted))):
        y[i], raw[i] = planted[(first + i) % len(planted)]
    w = None
    if weighted:
        w = rng.uniform(0.25, 4.0, n).astype(np.float32)
        w[rng.random(n) < 0.05] = 0.0
        w[0] = 1.5
    return {"X": rng.standard_normal((n, 2)).astype(np.float32), "y": y.astype(np.float32), "w": w, "s": raw}


@functools.lru_cache(maxsize=None)
def multi_case(name):
    objective, K, top_k, size = name.split(":")
    K, top_k = int(K), int(top_k)
    if size == "grid":
        n_train, n_valid, idx = GRID_TRAIN, GRID_VALID, 1
    else:
        idx = SIZES.index(int(size))
        n_train, n_valid = SIZES[idx], VALID_SIZES[idx]
    train, valid = _two_sets("multi" + name, lambda n, wt, rng: _multi_data(K, n, wt, rng), n_train, n_valid, idx + K)
    error = "multi_error" if top_k == 1 else f"multi_error@{top_k}"
    params = {"objective": objective, "num_class": K, "metric": ["multi_logloss", "multi_error"], "multi_error_top_k": top_k}
    if objective == "multiclassova":
        params["sigmoid"] = MULTI_OVA_SIGMOID
    out = {"params": params, "train": train, "valid": valid, "family": "multi"}
    for part in ("train", "valid"):
        d = out[part]
        out["ref_" + part] = {
            "multi_logloss": multiclass_reference("multi_logloss", objective, MULTI_OVA_SIGMOID, top_k, d["y"], d["s"], d["w"]),
            error: multiclass_reference("multi_error", objective, MULTI_OVA_SIGMOID, top_k, d["y"], d["s"], d["w"])}
    return out


# ------------------------------------------------------------------ AUC / average precision reference
PAIR_LIMIT = 257  # the O(n^2) pair definition up to here, the grouped form above


def auc_pairs(y, s, w):
    """AUC by its definition: the weight of the (positive, negative) pairs the score orders right,
    half of the tied ones, over the weight of all such pairs; 1 for a single class. Exact (Fraction)
    without weights."""
    pos, neg = np.asarray(y) > 0, ~(np.asarray(y) > 0)
    sp, sn = s[pos], s[neg]
    gt = sp[:, None] > sn[None, :]
    eq = sp[:, None] == sn[None, :]
    if w is None:
        if pos.sum() == 0 or neg.sum() == 0:
            return fractions.Fraction(1)
        return fractions.Fraction(2 * int(gt.sum()) + int(eq.sum()), 2 * int(pos.sum()) * int(neg.sum()))
    wl = np.asarray(w, dtype=np.float32).astype(LD)
    wp, wn = wl[pos], wl[neg]
    if not (wp > 0).any() or not (wn > 0).any():
        return 1.0
    num = exact_sum((gt + LD(0.5) * eq) * wp[:, None] * wn[None, :])
    return float(LD(num) / (LD(exact_sum(wp)) * LD(exact_sum(wn))))


def average_precision_thresholds(y, s, w):
    """Average precision by its definition: over the distinct scores t, the positive weight at t
    times the precision among the rows scored >= t, over the positive weight; 1 for a single class.
    Exact (Fraction) without weights."""
    pos = np.asarray(y) > 0
    if w is None:
        if pos.sum() == 0 or pos.all():
            return fractions.Fraction(1)
        acc = fractions.Fraction(0)
        for t in np.unique(s):
            here, above = s == t, s >= t
            acc += fractions.Fraction(int((here & pos).sum()) * int((above & pos).sum()), int(above.sum()))
        return acc / int(pos.sum())
    wl = np.asarray(w, dtype=np.float32).astype(LD)
    if not (wl[pos] > 0).any() or not (wl[~pos] > 0).any():
        return 1.0
    terms = []
    for t in np.unique(s):
        here, above = s == t, s >= t
        den = LD(exact_sum(wl[above]))
        if den > 0:
            terms.append(LD(exact_sum(wl[here & pos])) * LD(exact_sum(wl[above & pos])) / den)
    return float(LD(exact_sum(np.array(terms, dtype=LD))) / LD(exact_sum(wl[pos])))


def auc_ap_grouped(y, s, w):
    """(AUC, average precision) from the groups of equal scores in descending order, in long double:
    AUC = sum_g neg_g * (pos above g + pos_g / 2) / (pos * neg), AP = sum_g pos_g * (pos through g /
    weight through g) / pos."""
    pos = np.asarray(y) > 0
    wl = np.ones(len(s), dtype=LD) if w is None else np.asarray(w, dtype=np.float32).astype(LD)
    uniq, inv = np.unique(s, return_inverse=True)  # ascending; -0.0 == +0.0
    inv = (len(uniq) - 1) - inv.ravel()  # descending
    gp, gn = np.zeros(len(uniq), dtype=LD), np.zeros(len(uniq), dtype=LD)
    np.add.at(gp, inv[pos], wl[pos])
    np.add.at(gn, inv[~pos], wl[~pos])
    tp, tn = gp.sum(), gn.sum()
    if not tp > 0 or not tn > 0:
        return 1.0, 1.0
    cp = np.cumsum(gp)
    ct = np.cumsum(gp + gn)
    auc = exact_sum(gn * (cp - gp + gp / 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        ap = exact_sum(np.where(ct > 0, gp * (cp / np.where(ct > 0, ct, 1)), 0))
    return float(LD(auc) / (tp * tn)), float(LD(ap) / tp)


def auc_ap_reference(y, s, w):
    if len(s) <= PAIR_LIMIT:
        return float(auc_pairs(y, s, w)), float(average_precision_thresholds(y, s, w))
    return auc_ap_grouped(y, s, w)


def nonneg_bound(n):
    """Three nested sums of non-negative terms in any order, and the final quotient."""
    return (3 * n + 4) * U


AUC_PATTERNS = ("all_equal", "distinct", "rounded", "zeros", "extreme", "only_pos", "only_neg")


def _auc_data(pattern, n, weighted, rng):
    y = (rng.random(n) < 0.4).astype(np.float32)
    if pattern == "all_equal":
        s = np.full(n, 0.375)
    elif pattern == "distinct":
        s = np.argsort(np.argsort(rng.standard_normal(n) + 0.7 * y)).astype(np.float64) * 0.37 - 11.0
        assert len(np.unique(s)) == n
    elif pattern == "rounded":
        s = np.round(rng.standard_normal(n) + 0.7 * y, 1)
    elif pattern == "zeros":  # -0.0 and +0.0 with different labels must tie
        s = rng.choice(np.array([-1.0, -0.0, 0.0, 0.0, 2.0]), size=n)
        z = np.flatnonzero(s == 0.0)
        s[z[y[z] > 0]] = -0.0
        s[z[y[z] <= 0]] = 0.0
        if n >= 2:
            s[:2], y[:2] = (-0.0, 0.0), (1.0, 0.0)
    elif pattern == "extreme":  # +-inf, subnormals, values near +-1e300 through the radix sort
        pool = np.array([np.inf, -np.inf, 1e300, -1e300, 9.9e299, -9.9e299, 5e-324, -5e-324, 1e-310, -1e-310, 2e-310, 0.0,
                         -0.0, 1.0, -1.0, 2.2250738585072014e-308])
        s = rng.choice(pool, size=n)
        k = min(n, len(pool))
        s[:k] = pool[:k]
    else:
        s = np.round(rng.standard_normal(n), 1)
        y[:] = 1.0 if pattern == "only_pos" else 0.0
    if n >= 2 and pattern in ("all_equal", "distinct", "rounded", "extreme"):
        y[0], y[1] = 1.0, 0.0
    w = None
    if weighted:
        w = rng.uniform(0.25, 4.0, n).astype(np.float32)
        w[rng.random(n) < 0.1] = 0.0
        # never a top-score group of zero total weight (0 / 0 on the host and in the reference project)
        w[s == s.max()] = np.float32(1.25)
        if n >= 2:
            w[:2] = np.float32(0.75)
    return {"X": rng.standard_normal((n, 2)).astype(np.float32), "y": y, "w": w, "s": s}


def _wide_weight_positives(n, rng):
    """Only positives, float32 weights from 2^-20 to 2^20: two sums of them in different orders need
    not agree to the last bit."""
    w = (2.0 ** rng.uniform(-20, 20, n)).astype(np.float32)
    return {"X": rng.standard_normal((n, 2)).astype(np.float32), "y": np.ones(n, dtype=np.float32), "w": w,
            "s": rng.standard_normal(n)}


AUC_CASES = [f"{p}:{n}" for p in AUC_PATTERNS for n in SIZES] + ["distinct:grid", "single_class_wide_weights"]


@functools.lru_cache(maxsize=None)
def auc_case(name):
    """-> dict(params, train, valid, ref_*: {"auc": v, "average_precision": v}, exact)."""
    rng = np.random.default_rng(_seed("auc" + name))
    exact = False
    if name == "single_class_wide_weights":
        train, valid = _wide_weight_positives(100_000, rng), _wide_weight_positives(60_000, rng)
    elif name == "distinct:grid":  # unit weights: every AUC accumulator is an integer or half-integer
        train, valid = _auc_data("distinct", AUC_GRID, False, rng), _auc_data("distinct", GRID_VALID, False, rng)
        exact = True
    else:
        pattern, size = name.split(":")
        idx = SIZES.index(int(size))
        train, valid = _two_sets("auc" + name, lambda n, wt, r: _auc_data(pattern, n, wt, r), SIZES[idx], VALID_SIZES[idx],
                                 idx + AUC_PATTERNS.index(pattern))
    out = {"params": {"objective": "binary", "metric": ["auc", "average_precision"]}, "train": train, "valid": valid,
           "family": "auc", "exact": exact}
    for part in ("train", "valid"):
        d = out[part]
        auc, ap = auc_ap_reference(d["y"], d["s"], d["w"])
        out["ref_" + part] = {"auc": auc, "average_precision": ap}
    return out


# ------------------------------------------------------------------ auc_mu reference
def default_class_weights(K):
    return 1.0 - np.eye(K)


def auc_mu_reference(y, raw, w, cw):
    """auc_mu (Kleiman & Page 2019) by its pair definition: for classes i < j, v = cw[i] - cw[j],
    d(a) = (v_i - v_j) * (v . score_a); S_ij = the weight of the (a in i, b in j) pairs with
    d_b < d_a, half of those with d_b == d_a; the mean of S_ij / (W_i W_j). The cases' scores and
    class weights are dyadic, so every d is exact and a tie is an exact tie."""
    yi = np.asarray(y, dtype=np.float32).astype(np.int64)
    K = cw.shape[0]
    raw = np.asarray(raw, dtype=np.float64)
    wl = np.ones(len(yi), dtype=LD) if w is None else np.asarray(w, dtype=np.float32).astype(LD)
    ans = LD(0)
    for i in range(K):
        for j in range(i + 1, K):
            v = cw[i] - cw[j]
            t1 = v[i] - v[j]
            d = t1 * (raw @ v)
            assert np.all(d * 65536.0 == np.round(d * 65536.0))  # exact: multiples of 2^-16
            a, b = yi == i, yi == j
            m = (d[b][None, :] < d[a][:, None]) + LD(0.5) * (d[b][None, :] == d[a][:, None])
            S = exact_sum(wl[a] * (m * wl[b][None, :]).sum(axis=1))  # (the inner sums in long double)
            ans += LD(S) / LD(exact_sum(wl[a])) / LD(exact_sum(wl[b]))
    return float(2 * ans / K / (K - 1))


def auc_mu_bound(n, K):
    """Per pair three nested sums over at most n rows and two quotients, K (K - 1) / 2 non-negative
    pair values summed, three more operations."""
    return (3 * n + K * K + 8) * U


AUC_MU_KINDS = ("k2", "k5", "k5custom", "k5equal", "k5pair11")
AUC_MU_SIZES = ("min", 255, 256, 257, 4099)
AUC_MU_CASES = [f"{k}:{n}" for k in AUC_MU_KINDS for n in AUC_MU_SIZES]
CUSTOM_CW = np.array([[0, 1, 2, 0.5, 1], [0.25, 0, 1, 3, 1], [1, 1, 0, 1, 0.125], [2, 1, 0.5, 0, 1], [1, 0.75, 1, 1.5, 0]])


def _auc_mu_data(kind, n, weighted, rng):
    K = 2 if kind == "k2" else 5
    y = rng.integers(0, K, n)
    y[:K] = np.arange(K)  # no empty class
    if kind == "k5pair11":  # classes 3 and 4 have one row each
        y[y >= 3] = rng.integers(0, 3, int((y >= 3).sum()))
        y[3], y[4] = 3, 4
    raw = np.round(rng.standard_normal((n, K)) * 4.0 + 2.0 * np.eye(K)[y]) / 8.0 if kind != "k5equal" else np.full((n, K), 0.625)
    if kind != "k5equal":
        fine = rng.random(n) < 0.5  # the 2^-10 grid on half the rows, heavy ties on the others
        raw[fine] += rng.integers(-16, 16, (int(fine.sum()), K)) / 1024.0
    w = None
    if weighted:
        w = rng.uniform(0.25, 4.0, n).astype(np.float32)
    return {"X": rng.standard_normal((n, 2)).astype(np.float32), "y": y.astype(np.float32), "w": w, "s": raw}


@functools.lru_cache(maxsize=None)
def auc_mu_case(name):
    kind, size = name.split(":")
    K = 2 if kind == "k2" else 5
    idx = AUC_MU_SIZES.index(size if size == "min" else int(size))
    sizes = (K,) + SIZES[1:]
    valid_sizes = (4099, K) + SIZES[1:4]
    train, valid = _two_sets("aucmu" + name, lambda n, wt, r: _auc_mu_data(kind, n, wt, r), sizes[idx], valid_sizes[idx],
                             idx + AUC_MU_KINDS.index(kind))
    cw = CUSTOM_CW if kind == "k5custom" else default_class_weights(K)
    params = {"objective": "multiclass", "num_class": K, "metric": ["auc_mu"]}
    if kind == "k5custom":
        params["auc_mu_weights"] = [float(x) for x in cw.ravel()]
    out = {"params": params, "train": train, "valid": valid, "family": "auc_mu", "K": K, "kind": kind}
    for part in ("train", "valid"):
        d = out[part]
        out["ref_" + part] = {"auc_mu": auc_mu_reference(d["y"], d["s"], d["w"], cw)}
        if kind == "k5equal":
            assert out["ref_" + part]["auc_mu"] == 0.5
        if kind == "k2":  # the binary AUC of class 0 against class 1 at s_0 - s_1
            binary = auc_ap_grouped((d["y"] == 0).astype(np.float32), d["s"][:, 0] - d["s"][:, 1], d["w"])[0]
            assert abs(binary - out["ref_" + part]["auc_mu"]) <= 4 * U
    return out


@functools.lru_cache(maxsize=None)
def auc_mu_fallback_case():
    """num_class = 65, one above the device path's kAucMuMaxClass: evaluated on the host."""
    K, n = 65, 400
    rng = np.random.default_rng(_seed("aucmu65"))
    out = {"params": {"objective": "multiclass", "num_class": K, "metric": ["auc_mu"]}, "family": "auc_mu", "K": K}
    for part, m in (("train", n), ("valid", n - 70)):
        y = rng.integers(0, K, m)
        y[:K] = np.arange(K)
        raw = np.round(rng.standard_normal((m, K)) * 4.0 + 2.0 * np.eye(K)[y]) / 8.0
        out[part] = {"X": rng.standard_normal((m, 2)).astype(np.float32), "y": y.astype(np.float32), "w": None, "s": raw}
        out["ref_" + part] = {"auc_mu": auc_mu_reference(y, raw, None, default_class_weights(K))}
    return out


# ------------------------------------------------------------------ running a case
FAMILIES = {"pointwise": (POINTWISE_CASES, pointwise_case), "multi": (MULTI_CASES, multi_case),
            "auc": (AUC_CASES, auc_case), "auc_mu": (AUC_MU_CASES, auc_mu_case)}
# the phase timers a device evaluation of each family counts in: (training set, validation set)
FAMILY_TIMERS = {"pointwise": ("Device::EvalMetric", "Device::EvalValid"),
                 "multi": ("Device::EvalMultiMetric", "Device::EvalMultiMetric"),
                 "auc": ("Device::EvalRankMetric", "Device::EvalRankMetric"),
                 "auc_mu": ("Device::EvalAucMu", "Device::EvalAucMu")}
TIMERS = ("Device::EvalMetric", "Device::EvalValid", "Device::EvalMultiMetric", "Device::EvalAucMu", "Device::EvalRankMetric")


def get_case(family, name):
    return FAMILIES[family][1](name)


def booster(lgb, device, case):
    p = {"verbosity": -1, "device_type": device, "num_leaves": 7, "num_threads": 4, "seed": 1}
    p.update(case["params"])
    t, v = case["train"], case["valid"]
    ds = lgb.Dataset(t["X"], t["y"], weight=t["w"], init_score=t["s"], params=p)
    b = lgb.Booster(p, ds)
    b.add_valid(lgb.Dataset(v["X"], v["y"], weight=v["w"], init_score=v["s"], reference=ds, params=p), "valid")
    return b


def evaluate(b):
    """({metric: value} of the training set, of the validation set) at the init scores, before any tree."""
    return {m: v for _, m, v, _ in b.eval_train()}, {m: v for _, m, v, _ in b.eval_valid()}


@contextlib.contextmanager
def host_metrics():
    old = os.environ.get("LGAP_DEVICE_METRICS")
    os.environ["LGAP_DEVICE_METRICS"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["LGAP_DEVICE_METRICS"]
        else:
            os.environ["LGAP_DEVICE_METRICS"] = old


def deviation(case, part, metric, got):
    """(figure, bound name, within): the deviation of `got` from the case's reference in the family's
    units, without the device / host distinction: loss units for losses, relative error over the
    bound (so <= 1 passes) for sums of non-negative terms, |difference| for exact counts."""
    ref = case["ref_" + part][metric]
    n = len(case[part]["y"])
    if isinstance(ref, dict):
        if ref["kind"] in ("binary_error", "multi_error"):
            if case[part]["w"] is None:  # a count over n: exact up to the division
                return abs(got - ref["value"]) / (2 * U * max(ref["value"], U)), "count"
            return abs(got - ref["value"]) / (nonneg_bound(n) * max(ref["value"], 1e-300)), "nonneg"
        return loss_units(ref, got), "loss"
    if case["family"] == "auc_mu":
        return abs(got - ref) / (auc_mu_bound(n, case["K"]) * max(ref, 1e-300)), "nonneg"
    if case.get("exact") and metric == "auc":
        return abs(got - ref) / (4 * U * ref), "nonneg"
    return abs(got - ref) / (nonneg_bound(n) * max(ref, 1e-300)), "nonneg"


def check_values(case, part, values, device, what, seen=None):
    """Every metric of one set against the reference within its bound; `seen` collects the largest
    loss units per metric kind."""
    assert set(values) == set(case["ref_" + part]), f"{what}: {sorted(values)}"
    for metric, got in values.items():
        figure, how = deviation(case, part, metric, got)
        ref = case["ref_" + part][metric]
        kind = ref["kind"] if isinstance(ref, dict) else metric
        bound = loss_bound(device, kind) if how == "loss" else 1.0
        refv = ref["value"] if isinstance(ref, dict) else ref
        print(f"{what} {part} {metric}: {got!r} reference {refv!r}: {figure:.3f} of {bound:.1f} ({how})")
        if seen is not None and how == "loss":
            seen[kind] = max(seen.get(kind, 0.0), figure)
        assert figure <= bound, f"{what} {part} {metric} = {got!r}, reference {refv!r}: {figure:.3f} > {bound:.1f} ({how})"


def check_case_cpu(lgb, family, name, seen=None):
    case = get_case(family, name)
    train, valid = evaluate(booster(lgb, "cpu", case))
    check_values(case, "train", train, "cpu", f"{family} {name} on cpu", seen)
    check_values(case, "valid", valid, "cpu", f"{family} {name} on cpu", seen)


# ------------------------------------------------------------------ the device run (one child process)
def timer_counts(lgb):
    """{timer: calls} of the metric timer families, from phase_timer_report()."""
    out = dict.fromkeys(TIMERS, 0)
    for line in lgb.phase_timer_report().splitlines():
        p = line.split()
        if len(p) >= 5 and p[0] in out and p[-1] == "calls":
            out[p[0]] = int(p[-2])
    return out


def _expect_counts(before, after, want, what):
    grew = {t: after[t] - before[t] for t in TIMERS}
    assert grew == want, f"{what}: the device timers grew by {grew}, expected {want}"


def _close(a, b, what):
    assert set(a) == set(b), what
    for m in a:
        assert abs(a[m] - b[m]) <= METRIC_RTOL * abs(b[m]), f"{what}: {m} = {a[m]!r} on the device, {b[m]!r} on the host"


def run_case_device(lgb, family, name, seen):
    """One case with device_type=gpu: device values against the reference, against the host metric
    on the same booster, two evaluations bit-identical, and the timer counts that prove which of the
    two evaluated."""
    case = auc_mu_fallback_case() if name == "fallback65" else get_case(family, name)
    what = f"{family} {name} on gpu"
    b = booster(lgb, "gpu", case)
    nm = len(case["ref_train"])
    c0 = timer_counts(lgb)
    train, valid = evaluate(b)
    again = evaluate(b)
    c1 = timer_counts(lgb)
    want = dict.fromkeys(TIMERS, 0)
    if name != "fallback65":
        want[FAMILY_TIMERS[family][0]] += 2 * nm
        want[FAMILY_TIMERS[family][1]] += 2 * nm
    _expect_counts(c0, c1, want, what)
    assert (train, valid) == again, f"{what}: two evaluations differ: {(train, valid)} and {again}"
    with host_metrics():
        host_train, host_valid = evaluate(b)
    _expect_counts(c1, timer_counts(lgb), dict.fromkeys(TIMERS, 0), what + " with LGAP_DEVICE_METRICS=0")
    check_values(case, "train", train, "gpu", what, seen)
    check_values(case, "valid", valid, "gpu", what, seen)
    if name == "fallback65":
        assert (train, valid) == (host_train, host_valid)
    else:
        _close(train, host_train, what + " train, device against host")
        _close(valid, host_valid, what + " valid, device against host")


def main():
    """Every case of every family in this process (started with LGAP_TIMETAG=1, which PhaseTimer
    reads once): prints `RESULT {"verdicts": {"<family>/<case>": null | "<failure>"}, "seen": {...}}`,
    `seen` the largest loss units per metric kind. A failed assertion is a verdict; a library error
    ends the run there, and the cases after it have no verdict."""
    import json
    import traceback

    import lambdagap_amd as lgb

    assert os.environ.get("LGAP_TIMETAG") == "1" and "LGAP_DEVICE_METRICS" not in os.environ
    verdicts, seen = {}, {}
    todo = [(f, n) for f, (names, _) in FAMILIES.items() for n in names] + [("auc_mu", "fallback65")]
    for family, name in todo:
        try:
            run_case_device(lgb, family, name, seen)
            verdicts[f"{family}/{name}"] = None
        except AssertionError as e:
            verdicts[f"{family}/{name}"] = str(e)[:1500] or "assert"
        except Exception:
            verdicts[f"{family}/{name}"] = traceback.format_exc()[-1500:]
            break
    print("RESULT " + json.dumps({"verdicts": verdicts, "seen": seen}))
