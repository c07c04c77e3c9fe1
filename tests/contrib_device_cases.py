"""Shared by test_contrib_device_cpu.py (the path pack and per-row function in a host loop) and
test_contrib_device.py (the same function in the HIP kernel): the hook, the error measure and
tolerance, and chain models for long paths. The trained models are predict_device_cases.py's.

Thresholds of the launch plan (src/device/contrib_kernels.h, PlanContribShape), with m the most
unique features on any path of the model and width = k * (num_features + 1):
  * a path holds at most 64 unique features (kCMaxPathFeatures), longer ones are refused;
  * a block has 256 lanes (= rows of a tile) while 8 B * lanes * (m + 1) <= 34 KiB, that is up
    to m = 16; 128 lanes up to m = 33; 64 lanes beyond;
  * the tile's contributions stay in LDS while 8 B * lanes * (m + 1 + width) <= 64 KiB, else each
    lane adds into its own output row in global memory. For a chain of m features (width m + 1)
    that is m <= 15 at 256 lanes, m <= 31 at 128 lanes and m <= 63 at 64 lanes;
  * rows are staged in LDS when they fit in what is left of the 64 KiB;
  * host input is uploaded in chunks of at most 256 MiB of the larger of input and output.
"""
import ctypes
import functools

import numpy as np

import lambdagap_amd as lgb
from lambdagap_amd.basic import _LIB, _c_str, _check

from predict_device_cases import CASES

C_API_DTYPE_FLOAT32, C_API_DTYPE_FLOAT64 = 0, 1
PREDICT_CONTRIB = 3

MAX_PATH_FEATURES = 64
TILE_ROWS = 256  # kCMaxThreads: the tile of every model whose paths have at most 16 unique features
UPLOAD_CHUNK_BYTES = 256 << 20

# Worst err() of hook against Booster.predict(pred_contrib=True) over every case of CONTRIB_CASES,
# float64 and float32 rows, measured on the CPU (profiles/predict_contrib_device.md): 8.3e-15
# (leaves_below, 200-leaf trees). Asserted at 8x: both sides are deterministic IEEE + * /, the
# factor only absorbs another compiler's association of the host's own sums. Far inside the
# 1e-9 cap.
CONTRIB_TOL = 8 * 8.3e-15
assert CONTRIB_TOL <= 1e-9

CONTRIB_CASES = [c for c in CASES if c != "linear"]

# chain lengths on both sides of every threshold of the plan, and the longest supported one
CHAIN_LENGTHS = [15, 16, 17, 31, 32, 33, 34, 63, 64]
# Unwinding m features amplifies rounding with m in both algorithms: measured on these chains, the
# contributions' sum misses the raw score by up to 2.4e-14 for m <= 17 but 5.5e-12 at m = 31 and
# 1.3e-4 at m = 64 (profiles/predict_contrib_device.md). Additivity is asserted up to here.
CHAIN_ADDITIVE_UP_TO = 17


def lanes(max_path):
    """Lanes (= tile rows) PlanContribShape picks for a model whose longest path has max_path features."""
    return 256 if max_path <= 16 else 128 if max_path <= 33 else 64


def hook(booster, X, start_iteration=0, num_iteration=-1, params=""):
    """LGBM_BoosterTestPackedContrib: the device path's pack and per-row function in a host loop."""
    X = np.ascontiguousarray(X)
    dtype = C_API_DTYPE_FLOAT32 if X.dtype == np.float32 else C_API_DTYPE_FLOAT64
    n = ctypes.c_int64(0)
    _check(_LIB.LGBM_BoosterCalcNumPredict(booster.handle, ctypes.c_int(X.shape[0]), ctypes.c_int(PREDICT_CONTRIB),
                                           ctypes.c_int(start_iteration), ctypes.c_int(num_iteration),
                                           ctypes.byref(n)))
    out = np.full(n.value, -12345.0, dtype=np.float64)
    out_len = ctypes.c_int64(0)
    _check(_LIB.LGBM_BoosterTestPackedContrib(
        booster.handle, X.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(dtype), ctypes.c_int32(X.shape[0]),
        ctypes.c_int32(X.shape[1]), ctypes.c_int(start_iteration), ctypes.c_int(num_iteration), _c_str(params),
        ctypes.byref(out_len), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    assert out_len.value == n.value
    return out.reshape(X.shape[0], -1)


def err(got, ref):
    """max over rows of max|got - ref| / max(1, max|ref| in that row)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    if ref.size == 0:
        return 0.0
    scale = np.maximum(1.0, np.abs(ref).max(axis=1))
    return float((np.abs(got - ref).max(axis=1) / scale).max())


def additivity_err(contrib, raw, k):
    """The class blocks' sums against the raw scores (nrow x k), on err()'s scale."""
    contrib = np.asarray(contrib)
    blocks = contrib.reshape(contrib.shape[0], k, -1)
    scale = np.maximum(1.0, np.abs(contrib).max(axis=1))
    return float((np.abs(blocks.sum(axis=2) - np.asarray(raw).reshape(contrib.shape[0], k)).max(axis=1) / scale).max())


def raw_scores(booster, X, name="", **kw):
    """predict(raw_score=True) as the sum contributions add up to: rf's average times its iterations."""
    raw = booster.predict(X, raw_score=True, **kw).reshape(X.shape[0], -1)
    if name == "rf":
        raw = raw * booster.current_iteration()
    return raw


def chain_model_string(m, seed=0):
    """A v4 model text with one tree: a chain of m splits on features 0 .. m-1 (node i sends
    x[i] <= 0 to leaf i and the rest on to node i + 1), data counts shrinking by a fifth per level."""
    rng = np.random.default_rng(1000 + 31 * m + seed)
    counts = [2_000_000_000]
    for _ in range(m):
        counts.append(counts[-1] * 4 // 5)
    leaf_count = [counts[i] - counts[i + 1] for i in range(m)] + [counts[m]]
    leaf_value = rng.normal(size=m + 1)
    left = [-(i + 1) for i in range(m)]
    right = [i + 1 for i in range(m - 1)] + [-(m + 1)]

    def join(v, fmt="{}"):
        return " ".join(fmt.format(x) for x in v)

    tree = "\n".join([
        "Tree=0", f"num_leaves={m + 1}", "num_cat=0",
        "split_feature=" + join(range(m)),
        "split_gain=" + join([1] * m),
        "threshold=" + join([0.0] * m, "{!r}"),
        "decision_type=" + join([2] * m),
        "left_child=" + join(left), "right_child=" + join(right),
        "leaf_value=" + join(leaf_value.tolist(), "{!r}"),
        "leaf_weight=" + join(leaf_count), "leaf_count=" + join(leaf_count),
        "internal_value=" + join([0] * m),
        "internal_weight=" + join(counts[:m]), "internal_count=" + join(counts[:m]),
        "is_linear=0", "shrinkage=1", "", "",
    ])
    head = "\n".join([
        "tree", "version=v4", "num_class=1", "num_tree_per_iteration=1", "label_index=0",
        f"max_feature_idx={m - 1}", "objective=regression",
        "feature_names=" + join(range(m), "Column_{}"),
        "feature_infos=" + join(["[-1:1]"] * m),
        f"tree_sizes={len(tree)}", "", "",
    ])
    return head + tree + "end of trees\n\nfeature_importances:\n\nparameters:\n[boosting: gbdt]\n[objective: regression]\nend of parameters\n"


@functools.lru_cache(maxsize=None)
def chain(m):
    """-> (booster, rows as float64): random rows, the rows that go all the way down and leave at
    every level, and a few special values. Cached: callers must not modify the rows."""
    booster = lgb.Booster(model_str=chain_model_string(m))
    rng = np.random.default_rng(m)
    rows = [rng.normal(size=(40, m)), np.ones((1, m)), -np.ones((1, m)), np.zeros((1, m))]
    down = np.ones((m, m))
    down[np.arange(m), np.arange(m)] = -1.0  # row i leaves the chain at node i
    rows.append(down)
    sp = rng.normal(size=(3, m))
    sp[0, m // 2] = np.nan
    sp[1, 0] = np.inf
    sp[2, m - 1] = -1e-36
    rows.append(sp)
    return booster, np.ascontiguousarray(np.vstack(rows), dtype=np.float64)
