"""Cases and float64 numpy references of the ranking family, shared by test_rank_reference_cpu.py
(the host objectives and metrics, device_type=cpu) and test_rank_kernels.py (the HIP kernels
k_lambdarank, k_pos_accum / k_pos_update, k_xendcg of src/device/grad_kernels.hip and k_query_metric of
src/device/metric_kernels.hip, device_type=gpu).

The references are written from the definitions: the reference project's rank_objective.hpp
(LambdarankNDCG::GetGradientsForOneQuery with its 18 targets, GetSigmoid / ConstructSigmoidTable,
UpdatePositionBiasFactors, RankXENDCG), dcg_calculator.cpp, rank_metric.hpp, map_metric.hpp and
precision_metric.hpp, and this project's README for the LambdaGap targets; not from
include/lgap/rank_math.h or src/objective/rank_objective.cpp, which the host objective and the kernel
share. Everything is float64 over the float32 labels and weights the library stores.

This module imports no library: the test files hand their `lambdagap_amd` module to the check_*
functions. Data and references are built once per process (lru_cache) and never changed.

Query lengths are chosen around the paths of k_lambdarank:
  cnt <= 1            early out                                   1
  cnt <= 128          rank sort, two threads per document          2, 3, 63, 64, 65, 127, 128
  129 .. 256          rank sort, one thread per document           129, 255, 256
  257 .. 2048         LDS bitonic sort + the register permutation  257, 511, 1024, 2047, 2048
  > 2048              the kGlobal launch, global scratch           2049, 3000
and, for NDCG, the register pair loop (truncation <= 32) against the general loop (truncation 33
and above, and every other target). The LDS arrays have the length Pmax of the dataset's longest
query: `mixed` gives Pmax = 2048 with every shorter P below it (Pa != P), `short_array` Pmax = 256,
`tiny` Pmax = 2, and `no_long` is `mixed` without the kGlobal launch.
"""
import contextlib
import functools
import importlib
import os

import numpy as np

TARGETS = ["ndcg", "lambdaloss-ndcg", "lambdaloss-ndcg-plus-plus", "bndcg", "lambdaloss-bndcg",
           "lambdaloss-bndcg-plus-plus", "precision", "arpk", "lambdaloss-arp1", "lambdaloss-arp2", "ranknet",
           "bin-ranknet", "lambdagap-s", "lambdagap-x", "lambdagap-s-plus", "lambdagap-x-plus",
           "lambdagap-s-plus-plus", "lambdagap-x-plus-plus"]
# targets that skip a pair of two relevant documents
BINARY_TARGETS = {"precision", "bndcg", "lambdaloss-bndcg", "lambdaloss-bndcg-plus-plus", "arpk", "bin-ranknet",
                  "lambdagap-s", "lambdagap-x", "lambdagap-s-plus", "lambdagap-x-plus", "lambdagap-s-plus-plus",
                  "lambdagap-x-plus-plus"}
# the pair weight depends on no rank: the reference does not sort, pairs run in document order
_ORDER_FREE = {"ranknet", "bin-ranknet", "lambdaloss-arp1", "lambdaloss-arp2"}
# the outer rank stops at the truncation level
_I_TRUNCATED = {"ndcg", "lambdaloss-ndcg", "lambdaloss-ndcg-plus-plus", "bndcg", "lambdaloss-bndcg",
                "lambdaloss-bndcg-plus-plus", "precision"}
# the inner rank starts at max(i + 1, truncation level)
_J_FROM_K = {"arpk", "lambdagap-s-plus", "lambdagap-x-plus", "lambdagap-s-plus-plus", "lambdagap-x-plus-plus"}

MIXED_SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 1024, 2047, 2048, 2049, 3000)
_SIZES = {
    "mixed": MIXED_SIZES,
    # Pmax = 256 and a query of every P below it
    "short_array": (200, 2, 3, 5, 9, 17, 33, 65, 129, 1, 64, 128),
    "tiny": (2, 1, 2, 2, 1, 2),
    "no_long": MIXED_SIZES[:-2],
}
PATTERNS = ("distinct", "ties", "all_equal", "one_minus_inf", "neg_zero")

# The reference's `0.01f + fabs(delta_score)`: a float constant in a double sum
_F001 = float(np.float32(0.01))


def f32(a):
    """Rounded to float32, held as float64."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def default_label_gain():
    return np.array([2.0 ** i - 1.0 for i in range(31)])


def _discounts(n):
    """1 / log2(2 + r) for r = 0 .. n."""
    return 1.0 / np.log2(2.0 + np.arange(n + 1, dtype=np.float64))


# ------------------------------------------------------------------ lambdarank reference
def quantised_sigmoid(ds, sigmoid):
    """The objective's sigmoid: 2^20 bins over [-25 / sigmoid, 25 / sigmoid], the bin's left edge
    through 1 / (1 + exp(s_bin * sigmoid)), everything in float64."""
    bins = 1 << 20
    lo = -50.0 / sigmoid / 2
    hi = -lo
    factor = bins / (hi - lo)
    idx = ((np.clip(ds, lo, hi) - lo) * factor).astype(np.int64)
    idx = np.where(ds <= lo, 0, np.where(ds >= hi, bins - 1, idx))
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp((idx / factor + lo) * sigmoid))


def _delta_pair(target, pi, pj, hr, lr, L, gain, D, inv_dcg, inv_bdcg, k, w):
    """delta_pair of the pairs of ranks (pi < pj); hr / lr: the rank of the higher / lower label."""
    if target in ("ndcg", "lambdaloss-ndcg", "lambdaloss-ndcg-plus-plus", "bndcg", "lambdaloss-bndcg",
                  "lambdaloss-bndcg-plus-plus"):
        swap = np.abs(D[hr] - D[lr])  # |discount(high rank) - discount(low rank)|
        loss = D[pj - pi] - D[pj - pi + 1]  # the LambdaLoss rank-difference weight
        paired = {"ndcg": swap, "bndcg": swap, "lambdaloss-ndcg": loss, "lambdaloss-bndcg": loss,
                  "lambdaloss-ndcg-plus-plus": swap + w * loss, "lambdaloss-bndcg-plus-plus": swap + w * loss}[target]
        if target in BINARY_TARGETS:
            return paired * inv_bdcg
        return (gain[hr] - gain[lr]) * paired * inv_dcg
    if target in ("precision", "lambdagap-s", "lambdagap-x", "ranknet", "bin-ranknet"):
        return np.ones(len(pi))
    beyond = (pj + 1 - k) - (pi >= k) * (pi + 1 - k)  # ranks the pair spans beyond the top k
    if target == "lambdagap-s-plus":
        return (pj - pi == k) * w + (pi < k)
    if target == "lambdagap-x-plus":
        return (pj - pi >= k) * w + (pi < k)
    if target == "lambdagap-s-plus-plus":
        return (pj - pi == k) * w + beyond
    if target == "lambdagap-x-plus-plus":
        return (pj - pi >= k) * w + beyond
    if target == "arpk":
        return beyond.astype(np.float64)
    if target == "lambdaloss-arp1":
        return L[hr]
    if target == "lambdaloss-arp2":
        return L[hr] - L[lr]
    raise KeyError(target)


def _lambdarank_query(target, s, lab, k, sigmoid, norm, w, label_gain, block):
    """One query: (lambda, hessian, W) per document, unweighted. `s` float64 scores (position bias
    added), `lab` float32 labels."""
    n = len(s)
    lam, hes, wd = np.zeros(n), np.zeros(n), np.zeros(n)
    if n <= 1:
        return lam, hes, wd
    binary = target in BINARY_TARGETS
    # ranking: a stable descending sort; precision only needs its top-k set, ties to the lower index
    order = np.arange(n) if target in _ORDER_FREE else np.argsort(-s, kind="stable")
    S, L = s[order], lab[order].astype(np.float64)
    alive = S != -np.inf  # kMinScore documents take part in no pair
    Sf = np.where(alive, S, 0.0)
    if target in _ORDER_FREE or target == "precision":
        best, worst = s.max(), s.min()
    else:
        best = S[0]
        wi = n - 1
        if wi > 0 and S[wi] == -np.inf:
            wi -= 1
        worst = S[wi]
    gain = np.asarray(label_gain, dtype=np.float64)[L.astype(np.int64)]
    D = _discounts(n)
    kk = min(k, n)
    top = np.sort(lab.astype(np.int64))[::-1][:kk]
    max_dcg = float(np.sum(np.asarray(label_gain, dtype=np.float64)[top] * D[:kk]))
    inv_dcg = 1.0 / max_dcg if max_dcg > 0 else max_dcg
    max_bdcg = float(np.sum(D[:min(kk, int((lab > 0).sum()))]))
    inv_bdcg = 1.0 / max_bdcg if max_bdcg > 0 else max_bdcg
    i_end = min(n - 1, k) if target in _I_TRUNCATED else n - 1
    jj = np.arange(n)[None, :]
    total = 0.0
    for i0 in range(0, i_end, block):
        ii = np.arange(i0, min(i0 + block, i_end))[:, None]
        if target == "precision":
            m = jj >= k
        elif target in _J_FROM_K:
            m = jj >= np.maximum(ii + 1, k)
        elif target == "lambdagap-s":
            m = jj == ii + k
        elif target == "lambdagap-x":
            m = jj >= ii + k
        else:
            m = jj > ii
        m = m & alive[ii] & alive[jj] & (L[ii] != L[jj])
        if binary:
            m &= ~((L[ii] > 0) & (L[jj] > 0))
        pi, pj = np.nonzero(m)
        pi = pi + i0
        i_high = L[pi] > L[pj]
        hr, lr = np.where(i_high, pi, pj), np.where(i_high, pj, pi)
        ds = Sf[hr] - Sf[lr]
        dp = np.asarray(_delta_pair(target, pi, pj, hr, lr, L, gain, D, inv_dcg, inv_bdcg, k, w), dtype=np.float64)
        if norm and best != worst:
            dp = dp / (_F001 + np.abs(ds))
        p = quantised_sigmoid(ds, sigmoid)
        pl = p * (-sigmoid * dp)
        ph = p * (1.0 - p) * (sigmoid * sigmoid * dp)
        lam += np.bincount(hr, pl, n) - np.bincount(lr, pl, n)
        hes += np.bincount(hr, ph, n) + np.bincount(lr, ph, n)
        wd += np.bincount(hr, dp, n) + np.bincount(lr, dp, n)
        total -= 2.0 * float(pl.sum())
    if norm and total > 0:
        f = np.log2(1.0 + total) / total
        lam, hes, wd = lam * f, hes * f, wd * f
    out = [np.empty(n), np.empty(n), np.empty(n)]
    for o, v in zip(out, (lam, hes, wd)):
        o[order] = v
    return tuple(out)


def lambdarank_reference(target, score, label, sizes, weight=None, k=30, sigmoid=1.0, norm=True, gap_weight=1.0,
                         label_gain=None, block=512):
    """(G, H, W) per document in float64. W_d is the sum of the (normalised) delta_pair of the
    document's pairs times the query's final factor times its weight: every pair term is at most
    sigmoid * delta_pair in the lambda and sigmoid^2 * delta_pair / 4 in the hessian, so W_d is the
    scale an error of the summation is measured in. The i axis runs in blocks of `block` ranks."""
    score = np.asarray(score, dtype=np.float64)
    label = np.asarray(label, dtype=np.float32)
    gains = default_label_gain() if label_gain is None else np.asarray(label_gain, dtype=np.float64)
    G, H, W = np.zeros(len(score)), np.zeros(len(score)), np.zeros(len(score))
    b = 0
    for n in sizes:
        n = int(n)
        G[b:b + n], H[b:b + n], W[b:b + n] = _lambdarank_query(target, score[b:b + n], label[b:b + n], int(k),
                                                             float(sigmoid), bool(norm), float(gap_weight), gains, block)
        b += n
    if weight is not None:
        wt = f32(weight)
        G, H, W = G * wt, H * wt, W * wt
    return G, H, W


# c_host: the largest |got - ref| / (2^-23 * sigmoid * W_d) (lambdas) or / (2^-23 * sigmoid^2 * W_d)
# (hessians) of the HOST objective against lambdarank_reference over every gradient case of this
# module (GRADIENT_CASES, the position-bias cases included under ndcg), per target. The host sums
# float pair terms in rank order and rounds the normalised and the weighted value to float once more.
# Measured on 2026-10-21 with test_rank_reference_cpu.py::test_report_c_host (run with -s; x86-64,
# glibc exp) and rounded up to one decimal. The CPU tests assert the next power of two; the device
# gets 4 x c_host (fp32 sigmoid of the bin through __expf and v_rcp, fp32 1 / (0.01 + |ds|), another
# summation order) and no more: a structural error (a wrong pair, rank, tie order or permutation)
# moves a document by about one delta_pair, more than 1000 of these units even among 3000 pairs.
# (On an MI355X the same day the kernel stayed below 6 units wherever a wave's lanes share the sum,
# and reached 80 units = 2.9 x c_host at most, for the order-free targets on tied scores, where one
# lane adds up to 750 equal terms in a row: ranknet 77.3, lambdaloss-arp2 80.1, lambdaloss-arp1 55.3,
# bin-ranknet 34.8, lambdagap-x / -x-plus 27.7; lambdagap-s, the tightest bound, 1.5 of 4.0.)
C_HOST = {
    "ndcg": 57.0, "lambdaloss-ndcg": 68.5, "lambdaloss-ndcg-plus-plus": 19.1, "bndcg": 32.0, "lambdaloss-bndcg": 63.3,
    "lambdaloss-bndcg-plus-plus": 19.6, "precision": 87.7, "arpk": 17.9, "lambdaloss-arp1": 30.9,
    "lambdaloss-arp2": 29.9, "ranknet": 26.4, "bin-ranknet": 28.8, "lambdagap-s": 1.0, "lambdagap-x": 91.5,
    "lambdagap-s-plus": 101.8, "lambdagap-x-plus": 171.5, "lambdagap-s-plus-plus": 14.8, "lambdagap-x-plus-plus": 12.3,
}


def cpu_bound(target):
    c = C_HOST[target]
    return 2.0 ** int(np.ceil(np.log2(c)))


def device_bound(target):
    return 4.0 * C_HOST[target]


def gradient_ratio(got, ref, sigmoid, what):
    """The largest deviation of (g, h) from (G, H) in units of 2^-23 * sigmoid^(1|2) * W_d over every
    document; a document with W_d == 0 (no live pair) must be exactly (0, 0)."""
    g, h = (np.asarray(a) for a in got)
    G, H, W = ref
    assert g.dtype == np.float32 and h.dtype == np.float32 and g.shape == G.shape and h.shape == H.shape, what
    zero = W == 0
    bad = np.flatnonzero(zero & ((g != 0) | (h != 0)))
    assert bad.size == 0, f"{what}: documents {bad[:8]} have no live pair but (g, h) = ({g[bad[:8]]}, {h[bad[:8]]})"
    if zero.all():
        return 0.0
    unit = 2.0 ** -23 * W[~zero]
    rg = np.abs(g.astype(np.float64) - G)[~zero] / (unit * sigmoid)
    rh = np.abs(h.astype(np.float64) - H)[~zero] / (unit * sigmoid * sigmoid)
    return float(max(rg.max(), rh.max()))


# ------------------------------------------------------------------ data
def _scores(pattern, sizes, rng, labels=None):
    n = int(np.sum(sizes))
    if pattern in ("distinct", "one_minus_inf"):
        s = rng.standard_normal(n)
    elif pattern in ("ties", "neg_zero"):
        s = rng.choice(np.array([-1.0, -0.5, 0.0, 0.5, 1.0]), size=n)
    elif pattern == "all_equal":
        s = np.zeros(n)
    else:
        raise KeyError(pattern)
    if pattern == "neg_zero":
        # -0.0 next to +0.0: they compare equal, so the tie goes to the lower index
        z = np.flatnonzero(s == 0.0)
        s[z[::2]] = -0.0
        assert np.signbit(s).any() and (s == 0.0).sum() > 2
    if pattern == "one_minus_inf":
        # one document of every query at kMinScore, labelled into the top of the ideal ranking
        b = 0
        for c in sizes:
            if c >= 2:
                d = b + int(rng.integers(0, c))
                s[d] = -np.inf
                if labels is not None:
                    labels[d] = 4.0
            b += c
    return s


def _features(y, n, rng):
    X = rng.standard_normal((n, 4)).astype(np.float32)
    X[:, 0] += 0.5 * np.asarray(y, dtype=np.float32)
    return X


def _grad_spec(name):
    """name -> (dataset, pattern, target, objective parameters, weighted, labels)"""
    p = name.split(":")
    if p[0] == "paths":  # paths:<k>:<pattern>[:<dataset>]
        return {"sizes": p[3] if len(p) > 3 else "mixed", "pattern": p[2], "target": "ndcg",
                "params": {"lambdarank_truncation_level": int(p[1])}, "weighted": False, "labels": "graded"}
    if p[0] == "target":  # target:<name>:<weighted|ties>
        params = {"lambdarank_truncation_level": 12 if p[2] == "weighted" else 3, "lambdagap_weight": 0.5}
        return {"sizes": "mixed", "pattern": "distinct" if p[2] == "weighted" else "ties", "target": p[1], "params": params,
                "weighted": p[2] == "weighted", "labels": "binary" if p[1] in BINARY_TARGETS else "graded"}
    if p[0] == "option":
        params = {"nonorm": {"lambdarank_norm": False}, "sigmoid2": {"sigmoid": 2.0},
                  "gain71": {"label_gain": [0.5 * i * i for i in range(71)]}}[p[1]]
        return {"sizes": "mixed", "pattern": "distinct", "target": "ndcg", "params": params, "weighted": False,
                "labels": "to70" if p[1] == "gain71" else "graded"}
    if p[0] == "probe":  # probe:<target>
        return {"sizes": "probe", "pattern": "probe", "target": p[1], "params": {"lambdarank_truncation_level": 30},
                "weighted": False, "labels": "probe"}
    raise KeyError(name)


PROBE_LENGTHS = (64, 65, 256, 257, 2048, 2049)
PROBE_RANKS = (0, 29, 30, 63, 64, 255, 256)  # and cnt - 1; truncation level 30: k - 1 and k


def _probe_data(rng):
    """Queries of the boundary lengths, every label 0 except one relevant document placed by score
    at one of PROBE_RANKS (where that rank exists) or last."""
    sizes, scores, labels = [], [], []
    for cnt in PROBE_LENGTHS:
        for r in sorted({r for r in PROBE_RANKS if r < cnt} | {cnt - 1}):
            s = rng.standard_normal(cnt)
            assert len(np.unique(s)) == cnt
            lab = np.zeros(cnt, dtype=np.float32)
            lab[np.argsort(-s, kind="stable")[r]] = 2.0
            sizes.append(cnt)
            scores.append(s)
            labels.append(lab)
    return np.array(sizes), np.concatenate(scores), np.concatenate(labels)


GRADIENT_CASES = (
    [f"paths:{k}:{pat}" for k in (1, 30, 32, 33, 100000) for pat in PATTERNS]
    + [f"paths:30:distinct:{d}" for d in ("short_array", "tiny", "no_long")]
    + [f"target:{t}:{v}" for t in TARGETS for v in ("weighted", "ties")]
    + ["option:nonorm", "option:sigmoid2", "option:gain71"]
    + ["probe:ndcg", "probe:lambdagap-x", "probe:precision"]
)
DETERMINISM_CASES = ["paths:30:ties", "paths:33:distinct", "target:lambdagap-x-plus-plus:weighted", "target:ranknet:ties"]


def _seed(name):
    return 7000 + sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100000


@functools.lru_cache(maxsize=None)
def gradient_case(name):
    """-> dict(params, X, y, w, s, sizes, target, ref=(G, H, W)). Cached: callers must not modify it."""
    spec = _grad_spec(name)
    rng = np.random.default_rng(_seed(name))
    if spec["sizes"] == "probe":
        sizes, s, y = _probe_data(rng)
    else:
        sizes = np.array(_SIZES[spec["sizes"]])
        n = int(sizes.sum())
        if spec["labels"] == "to70":
            y = rng.integers(0, 71, n).astype(np.float32)
            assert y.max() >= 64  # gains at and above the kernel's LDS table of 64
        else:
            y = rng.integers(0, 5, n).astype(np.float32)
        if spec["labels"] == "binary":
            y = (y >= 3).astype(np.float32)
        s = _scores(spec["pattern"], sizes, rng, labels=y)
    n = len(s)
    X = _features(y, n, rng)
    w = rng.uniform(0.25, 3.0, size=n).astype(np.float32) if spec["weighted"] else None
    params = {"objective": "lambdarank", "lambdarank_target": spec["target"]}
    params.update(spec["params"])
    ref = lambdarank_reference(spec["target"], s, y, sizes, weight=w, k=params.get("lambdarank_truncation_level", 30),
                               sigmoid=params.get("sigmoid", 1.0), norm=params.get("lambdarank_norm", True),
                               gap_weight=params.get("lambdagap_weight", 1.0), label_gain=params.get("label_gain"))
    assert all(np.all(np.isfinite(a)) for a in ref)
    return {"params": params, "X": X, "y": y, "w": w, "s": s, "sizes": sizes, "target": spec["target"], "ref": ref,
            "position": None}


def _ops(lgb):
    return importlib.import_module(lgb.__name__ + ".ops")


def _booster(lgb, device, case, extra=None, valid=None):
    p = {"verbosity": -1, "device_type": device, "num_leaves": 7, "num_threads": 4, "seed": 1}
    p.update(case["params"])
    p.update(extra or {})
    ds = lgb.Dataset(case["X"], case["y"], weight=case["w"], group=case["sizes"], init_score=case["s"],
                     position=case.get("position"), params=p)
    b = lgb.Booster(p, ds)
    if valid is not None:
        b.add_valid(lgb.Dataset(valid["X"], valid["y"], weight=valid["w"], group=valid["sizes"], init_score=valid["s"],
                                reference=ds, params=p), "valid")
    return b


def _bound(device, target):
    return cpu_bound(target) if device == "cpu" else device_bound(target)


@functools.lru_cache(maxsize=None)
def _host_gradients(lgb, name):
    b = _booster(lgb, "cpu", gradient_case(name))
    b.update()
    return _ops(lgb).booster_gradients(b)


def assert_close_to_host(got, host, what):
    """The comparison of test_gpu_kernels.py::test_lambdarank_gradient_kernel_all_targets."""
    for a, b in zip(got, host):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5 * (np.abs(b).max() + 1e-12), err_msg=what)


def measure_gradients(lgb, device, name):
    case = gradient_case(name)
    b = _booster(lgb, device, case)
    b.update()
    got = _ops(lgb).booster_gradients(b)
    return got, gradient_ratio(got, case["ref"], case["params"].get("sigmoid", 1.0), f"{name} on {device}")


def check_gradients(lgb, device, name):
    """First round: one update at the given init score; every document within c * 2^-23 * sigmoid * W_d
    (sigmoid^2 for the hessian) of the reference, documents without a live pair exactly zero; on the
    device also the 1e-4 comparison with the host objective."""
    case = gradient_case(name)
    got, ratio = measure_gradients(lgb, device, name)
    print(f"{name} on {device}: ratio {ratio:.2f} (bound {_bound(device, case['target']):.1f})")
    assert ratio <= _bound(device, case["target"]), f"{name} on {device}: {ratio:.2f} units"
    if name.startswith("probe"):
        # one relevant document: pairs only with it, every other document in at most one
        assert (case["ref"][2] != 0).sum() < len(case["s"])
    if device != "cpu":
        assert_close_to_host(got, _host_gradients(lgb, name), name)
    return ratio


def check_deterministic(lgb, device, name):
    """Two boosters on the same case: bit-identical gradients (k_lambdarank sums in a fixed order)."""
    case = gradient_case(name)
    out = []
    for _ in range(2):
        b = _booster(lgb, device, case)
        b.update()
        out.append(_ops(lgb).booster_gradients(b))
    for a, b in zip(out[0], out[1]):
        assert a.tobytes() == b.tobytes(), f"{name}: two runs differ in some bit"


# ------------------------------------------------------------------ position bias
POSITION_CASES = [f"{p}:{r}" for p in (7, 1025) for r in ("noreg", "reg")]
_POS_LR = 0.1


@functools.lru_cache(maxsize=None)
def position_case(name):
    """`mixed` with positions arange % num_pos: 7 positions accumulate in LDS (k_pos_accum's
    num_pos <= 1024 branch), 1025 through global atomics; the queries of 2047 documents and more hold
    every one of the 1025 positions."""
    num_pos, reg = name.split(":")
    num_pos = int(num_pos)
    rng = np.random.default_rng(_seed("position" + name))
    sizes = np.array(MIXED_SIZES)
    n = int(sizes.sum())
    y = rng.integers(0, 5, n).astype(np.float32)
    s = rng.standard_normal(n)
    pos = np.concatenate([np.arange(c) % num_pos for c in sizes]).astype(np.int32)
    assert len(np.unique(pos)) == num_pos
    params = {"objective": "lambdarank", "lambdarank_target": "ndcg", "learning_rate": _POS_LR,
              "lambdarank_position_bias_regularization": 0.5 if reg == "reg" else 0.0}
    return {"params": params, "X": _features(y, n, rng), "y": y, "w": None, "s": s, "sizes": sizes, "position": pos,
            "num_pos": num_pos, "reg": params["lambdarank_position_bias_regularization"], "target": "ndcg"}


def newton_step(g, h, pos, num_pos, bias, lr, reg):
    """The position-bias update of UpdatePositionBiasFactors in float64 from the gradients (g, h):
    (new biases, the bound of their error when every row's -g and -h is first rounded to a 2^-24
    grid, as k_pos_accum's fixed point does)."""
    d1 = -np.bincount(pos, g.astype(np.float64), num_pos)
    d2 = -np.bincount(pos, h.astype(np.float64), num_pos)
    cnt = np.bincount(pos, minlength=num_pos).astype(np.float64)
    a = d1 - bias * reg * cnt
    den = np.abs(d2 - reg * cnt) + 0.001
    step = lr * a / den
    # |delta d1|, |delta d2| <= cnt * 2^-25 each, |x| is 1-Lipschitz: d(step) <= lr * e / den + lr * |a| * e / den^2;
    # plus 8 fp64 ulps of the sums' own size (the fixed-point sums are exact, the float64 sums here are not)
    e = cnt * 2.0 ** -25
    ulp = 8 * 2.0 ** -52 * (np.bincount(pos, np.abs(g).astype(np.float64), num_pos) + np.abs(bias) * reg * cnt)
    err = lr * (e + ulp) / den + lr * np.abs(a) * (e + ulp) / (den * den) + 4 * 2.0 ** -52 * (np.abs(bias) + np.abs(step))
    return bias + step, err


def check_position_bias(lgb, device, name):
    """Round 1: the biases equal the Newton step of the booster's own round-1 gradients from bias 0.
    Round 2: the gradients equal the reference at init + tree 1 + bias[position] (non-zero biases
    reach k_lambdarank), and the biases take the second Newton step (with regularization the
    `b * reg * cnt` term is then non-zero). The host keeps float biases: 2^-24 relative more per step."""
    case = position_case(name)
    ops = _ops(lgb)
    b = _booster(lgb, device, case)
    pos, num_pos, reg = case["position"], case["num_pos"], case["reg"]
    assert ops.position_biases(b).shape == (num_pos,) and not ops.position_biases(b).any()
    b.update()
    g1, h1 = ops.booster_gradients(b)
    b1 = ops.position_biases(b)
    assert b1.dtype == np.float64 and b1.shape == (num_pos,) and b1.all()
    want, err = newton_step(g1, h1, pos, num_pos, np.zeros(num_pos), _POS_LR, reg)
    if device == "cpu":
        err = err + 2.0 ** -24 * np.abs(want)
    assert np.all(np.abs(b1 - want) <= err), f"{name}: round 1 off by up to {np.abs(b1 - want).max():.3e}"
    b.update()
    g2, h2 = ops.booster_gradients(b)
    b2 = ops.position_biases(b)
    score = case["s"] + b.predict(case["X"], raw_score=True, num_iteration=1) + b1[pos]
    ref = lambdarank_reference("ndcg", score, case["y"], case["sizes"])
    ratio = gradient_ratio((g2, h2), ref, 1.0, f"{name} round 2 on {device}")
    print(f"position {name} on {device}: round-2 ratio {ratio:.2f}")
    assert ratio <= _bound(device, "ndcg"), f"{name} round 2 on {device}: {ratio:.2f} units"
    want, err = newton_step(g2, h2, pos, num_pos, b1, _POS_LR, reg)
    if device == "cpu":
        err = err + 2.0 ** -24 * (np.abs(want) + np.abs(want - b1) + np.abs(b1))
    assert np.all(np.abs(b2 - want) <= err), f"{name}: round 2 off by up to {np.abs(b2 - want).max():.3e}"
    return ratio


def check_no_positions(lgb, device):
    """A booster without positions has no biases."""
    b = _booster(lgb, device, gradient_case("paths:30:distinct:tiny"))
    b.update()
    assert _ops(lgb).position_biases(b).shape == (0,)


# ------------------------------------------------------------------ rank_xendcg
XENDCG_SIZES = (1, 2, 255, 256, 257, 2047, 2048, 2049, 3000)
XENDCG_CASES = [f"{p}:{w}" for p in ("distinct", "ties") for w in ("plain", "weighted")]
# the tolerance of test_gpu_kernels.py::test_xendcg_gradient_kernel_matches_torch
XENDCG_RTOL, XENDCG_ATOL = 1e-4, 1e-6
# The host objective's largest |got - ref| / (XENDCG_ATOL + XENDCG_RTOL * |ref|) over XENDCG_CASES, both
# rounds (2026-10-21, test_rank_reference_cpu.py::test_report_c_host). The device gets 4 x this
# where that is below 1, that is, where it tightens the tolerance above.
XENDCG_HOST_RATIO = 0.001


def xendcg_reference(score, label, sizes, seed, weight=None, rounds_before=0):
    """rank_xendcg lambdas / hessians (RankXENDCG::GetGradientsForOneQuery) in float64, each query's
    Random(seed + q) NextFloat draws reproduced. `rounds_before`: earlier calls, each of which drew
    once per document of every query of two documents or more."""
    score = np.asarray(score, dtype=np.float64)
    g, h = np.zeros(len(score)), np.zeros(len(score))
    b = 0
    for q, cnt in enumerate(sizes):
        cnt = int(cnt)
        if cnt > 1:
            s = score[b:b + cnt]
            e = np.exp(s - s.max())
            rho = e / e.sum()
            x = (seed + q) & 0xFFFFFFFF
            draws = np.empty(cnt * (rounds_before + 1))
            for i in range(len(draws)):
                x = (214013 * x + 2531011) & 0xFFFFFFFF
                draws[i] = float(np.float32((x >> 16) & 0x7FFF) / np.float32(32768.0))
            params = 2.0 ** np.asarray(label[b:b + cnt]).astype(np.int64) - draws[cnt * rounds_before:]
            inv_den = 1.0 / max(1e-15, float(params.sum()))
            t1 = -params * inv_den + rho
            p1 = t1 / (1 - rho)
            t2 = rho * (p1.sum() - p1)
            p2 = t2 / (1 - rho)
            t3 = rho * (p2.sum() - p2)
            g[b:b + cnt] = t1 + t2 + t3
            h[b:b + cnt] = rho * (1 - rho)
        b += cnt
    if weight is not None:
        g, h = g * np.asarray(weight, dtype=np.float64), h * np.asarray(weight, dtype=np.float64)
    return g, h


@functools.lru_cache(maxsize=None)
def xendcg_case(name):
    """Single-document queries (no draw), queries up to 2048 documents in k_xendcg<false>'s LDS and
    two longer ones in k_xendcg<true>'s global scratch."""
    pattern, variant = name.split(":")
    rng = np.random.default_rng(_seed("xendcg" + name))
    sizes = np.array(XENDCG_SIZES)
    n = int(sizes.sum())
    y = rng.integers(0, 5, n).astype(np.float32)
    w = rng.uniform(0.5, 2.0, n).astype(np.float32) if variant == "weighted" else None
    return {"params": {"objective": "rank_xendcg", "objective_seed": 11}, "X": _features(y, n, rng), "y": y, "w": w,
            "s": _scores(pattern, sizes, rng), "sizes": sizes, "position": None}


def _xendcg_ratio(got, ref):
    return max(float((np.abs(a.astype(np.float64) - r) / (XENDCG_ATOL + XENDCG_RTOL * np.abs(r))).max())
               for a, r in zip(got, ref))


def measure_xendcg(lgb, device, name):
    """(round-1 ratio, round-2 ratio) in units of the XENDCG_RTOL / XENDCG_ATOL tolerance."""
    case = xendcg_case(name)
    b = _booster(lgb, device, case)
    b.update()
    got1 = _ops(lgb).booster_gradients(b)
    b.update()
    got2 = _ops(lgb).booster_gradients(b)
    ref1 = xendcg_reference(case["s"], case["y"], case["sizes"], 11, case["w"])
    score = case["s"] + b.predict(case["X"], raw_score=True, num_iteration=1)
    ref2 = xendcg_reference(score, case["y"], case["sizes"], 11, case["w"], rounds_before=1)
    first = int(case["sizes"][0])
    assert first == 1 and not got1[0][:first].any() and not got2[1][:first].any()
    return _xendcg_ratio(got1, ref1), _xendcg_ratio(got2, ref2)


def check_xendcg(lgb, device, name):
    """Two rounds: the second round's draws continue every query's generator after cnt draws."""
    r1, r2 = measure_xendcg(lgb, device, name)
    bound = 1.0 if device == "cpu" else min(1.0, 4.0 * XENDCG_HOST_RATIO)
    print(f"xendcg {name} on {device}: ratios {r1:.4f} {r2:.4f} (bound {bound:.4f})")
    assert r1 <= bound and r2 <= bound, f"xendcg {name} on {device}: {r1:.4f}, {r2:.4f} of the tolerance"
    return max(r1, r2)


# ------------------------------------------------------------------ query metrics
EVAL_AT = [1, 3, 10, 63, 64, 65, 100, 128, 129, 1000, 5000]
# kMaxEvalAt positions, on and around the 64-document chunk boundaries
EVAL_AT_32 = [1, 2, 3, 5, 8, 13, 21, 34, 55, 63, 64, 65, 89, 127, 128, 129, 144, 191, 192, 193, 255, 256, 257, 300, 511,
              512, 513, 1000, 2048, 2049, 3000, 5000]
METRIC_CASES = ([f"mixed:{p}:{w}" for p in ("distinct", "ties", "all_equal", "neg_zero") for w in ("plain", "qweights")]
                + [f"single{n}:{p}:plain" for n in (64, 65, 129, 2049, 5000) for p in ("distinct", "ties")]
                + ["mixed:ties:qweights:eval32"])
METRIC_RTOL = 1e-12  # the tolerance of test_device_metrics.py


def query_metrics_reference(score, label, sizes, eval_at, weight=None, label_gain=None):
    """{"ndcg@k" | "map@k" | "precision@k": value} in float64 over a stable descending order.
    NDCG and MAP count 1 for a query without a relevant row; MAP divides by min(npos, min(k, n));
    precision@k divides the hits among the first min(k, n) by min(k, n - previous k), or by min(k, n)
    where that is not positive; queries weigh by the float32 mean of their rows' float32 weights."""
    score = np.asarray(score, dtype=np.float64)
    gains = default_label_gain() if label_gain is None else np.asarray(label_gain, dtype=np.float64)
    ks = sorted(int(k) for k in eval_at)
    acc = {m: np.zeros(len(ks)) for m in ("ndcg", "map", "precision")}
    sum_w = 0.0
    b = 0
    for n in sizes:
        n = int(n)
        s, lab = score[b:b + n], np.asarray(label[b:b + n], dtype=np.float32)
        qw = 1.0
        if weight is not None:
            qw = float(np.float32(np.asarray(weight[b:b + n], dtype=np.float32).astype(np.float64).sum() / n))
        sum_w += qw
        b += n
        L = lab[np.argsort(-s, kind="stable")]
        D = _discounts(n)[:n]
        dcg = np.concatenate([[0.0], np.cumsum(gains[L.astype(np.int64)] * D)])
        ideal = np.concatenate([[0.0], np.cumsum(gains[np.sort(lab.astype(np.int64))[::-1]] * D)])
        rel = L > 0.5
        hits = np.concatenate([[0], np.cumsum(rel)])
        ap = np.concatenate([[0.0], np.cumsum(np.where(rel, hits[1:] / (np.arange(n) + 1.0), 0.0))])
        npos = int(rel.sum())
        prev = 0
        for e, k in enumerate(ks):
            kk = min(k, n)
            acc["ndcg"][e] += qw * (dcg[kk] / ideal[kk] if ideal[min(ks[0], n)] > 0 else 1.0)
            acc["map"][e] += qw * (ap[kk] / min(npos, kk) if npos > 0 else 1.0)
            den = min(k, n - prev)
            if den <= 0:
                den = kk
            acc["precision"][e] += qw * (hits[kk] / den if den > 0 else 0.0)
            prev = k
    return {f"{m}@{k}": acc[m][e] / sum_w for m in acc for e, k in enumerate(ks)}


def _metric_data(kind, pattern, weighted, rng):
    sizes = np.array(MIXED_SIZES if kind == "mixed" else (int(kind[len("single"):]),))
    n = int(sizes.sum())
    y = rng.integers(0, 5, n).astype(np.float32)
    if kind == "mixed":
        starts = np.concatenate([[0], np.cumsum(sizes)])
        q63, q129 = list(sizes).index(63), list(sizes).index(129)
        y[starts[q63]:starts[q63 + 1]] = 0.0  # a query without a relevant document
        y[starts[q129]:starts[q129 + 1]] = np.maximum(y[starts[q129]:starts[q129 + 1]], 1.0)  # and one of only relevant ones
    # (per-row weights, constant inside a query: the metric's query weights)
    w = np.repeat(rng.uniform(0.5, 2.0, len(sizes)), sizes).astype(np.float32) if weighted else None
    return {"X": _features(y, n, rng), "y": y, "w": w, "s": _scores(pattern, sizes, rng), "sizes": sizes, "position": None}


@functools.lru_cache(maxsize=None)
def metric_case(name):
    """-> dict(train, valid, eval_at, ref_train, ref_valid). Queries of up to 5000 documents: up to 79
    64-document chunks per eval position in k_query_metric, eval positions that straddle chunks
    (63 | 64 | 65, 128 | 129), that lie beyond the query, and every rocPRIM segment-size regime."""
    p = name.split(":")
    eval_at = EVAL_AT_32 if len(p) > 3 else EVAL_AT
    assert len(EVAL_AT_32) == 32
    rng = np.random.default_rng(_seed("metric" + name))
    out = {"eval_at": eval_at}
    for part in ("train", "valid"):
        d = _metric_data(p[0], p[1], p[2] == "qweights", rng)
        d["params"] = {"objective": "lambdarank", "metric": ["ndcg", "map", "precision"], "eval_at": eval_at}
        out[part] = d
        out["ref_" + part] = query_metrics_reference(d["s"], d["y"], d["sizes"], eval_at, d["w"])
    return out


@contextlib.contextmanager
def _host_metrics():
    old = os.environ.get("LGAP_DEVICE_METRICS")
    os.environ["LGAP_DEVICE_METRICS"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["LGAP_DEVICE_METRICS"]
        else:
            os.environ["LGAP_DEVICE_METRICS"] = old


def _evaluate(lgb, device, case):
    b = _booster(lgb, device, case["train"], valid=case["valid"])
    train = {m: v for _, m, v, _ in b.eval_train()}  # the init scores, before any tree
    valid = {m: v for _, m, v, _ in b.eval_valid()}
    return train, valid


def _assert_metrics(got, ref, what):
    assert set(got) == set(ref), what
    for m in ref:
        assert abs(got[m] - ref[m]) <= METRIC_RTOL * abs(ref[m]), f"{what}: {m} = {got[m]!r}, reference {ref[m]!r}"


def check_metrics(lgb, device, name):
    """NDCG / MAP / precision at every eval position of the training set's and a validation set's
    init scores: equal to the reference within 1e-12 relative, and on the device equal to the host
    metric (LGAP_DEVICE_METRICS=0) on the same booster set-up within the same."""
    case = metric_case(name)
    train, valid = _evaluate(lgb, device, case)
    assert len(train) == 3 * len(case["eval_at"])
    _assert_metrics(train, case["ref_train"], f"{name} train on {device}")
    _assert_metrics(valid, case["ref_valid"], f"{name} valid on {device}")
    if device != "cpu":
        with _host_metrics():
            host_train, host_valid = _evaluate(lgb, device, case)
        _assert_metrics(train, host_train, f"{name} train, device against host")
        _assert_metrics(valid, host_valid, f"{name} valid, device against host")
