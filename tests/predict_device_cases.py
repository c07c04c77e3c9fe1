"""Models and probe rows shared by test_predict_device_cpu.py (the packed walk in a host loop)
and test_predict_device.py (the same walk in the HIP kernels). Every model is trained on the CPU
learner, so both files test only the prediction path. Built once per process and never changed.

Thresholds of the kernels that the shapes are chosen around (src/device/predict_kernels.h):
  * a block's tile is 512 rows (256 lanes x 2 rows);
  * a tile's rows are staged in LDS while 512 * ncol * sizeof(value) <= 56 KiB: up to 28 fp32
    or 14 fp64 columns, wider rows are read from global memory;
  * trees are staged in LDS while nodes * 24 B (padded to 16) + leaves * 8 B <= 8 KiB: a tree
    of up to 256 leaves, larger trees are walked from global memory;
  * up to 4 trees per iteration accumulate in registers, more classes in LDS;
  * host input is uploaded in chunks of at most 256 MiB.
"""
import functools

import numpy as np

import lambdagap_amd as lgb

TILE_ROWS = 512
STAGED_COLS_F32 = 28
STAGED_COLS_F64 = 14
STAGED_TREE_LEAVES = 256
REG_CLASSES = 4
UPLOAD_CHUNK_BYTES = 256 << 20

SPECIALS = [0.0, -0.0, 1e-36, -1e-36, np.inf, -np.inf, np.nan]

CASES = [
    "binary", "linear", "multiclass", "multiclassova", "multiclass6", "rf", "one_leaf", "leaves_below",
    "leaves_above", "missing_nan", "zero_as_missing", "no_missing", "categorical", "one_column", "wide",
]


def _splits(booster):
    """(feature, threshold) of every numerical split, (feature, categories) of every categorical one."""
    num, cat = [], []

    def walk(node):
        if "split_feature" not in node:
            return
        if node["decision_type"] == "==":
            cat.append((node["split_feature"], [int(c) for c in str(node["threshold"]).split("||")]))
        else:
            num.append((node["split_feature"], float(node["threshold"])))
        walk(node["left_child"])
        walk(node["right_child"])

    for tree in booster.dump_model()["tree_info"]:
        walk(tree["tree_structure"])
    return num, cat


def max_leaves(booster):
    return max(t["num_leaves"] for t in booster.dump_model()["tree_info"])


def min_leaves(booster):
    return min(t["num_leaves"] for t in booster.dump_model()["tree_info"])


def _probes(booster, X, cat_cols=()):
    """Training rows plus rows built to sit on every decision boundary."""
    rng = np.random.default_rng(7)
    ncol = X.shape[1]
    rows = [X[:300]]
    num, cat = _splits(booster)
    base = X[rng.integers(0, X.shape[0], size=len(num))].copy() if num else np.empty((0, ncol))
    for i, (f, thr) in enumerate(num):  # every split's exact threshold in its feature
        base[i, f] = thr
    rows.append(base)
    used = sorted({f for f, _ in num} | {f for f, _ in cat})
    feats = range(ncol) if ncol <= 64 else used
    for v in SPECIALS:
        rows.append(np.full((1, ncol), v))
        for f in feats:
            r = X[rng.integers(0, X.shape[0])].copy()
            r[f] = v
            rows.append(r[None, :])
    for f in cat_cols:
        words = max((max(c) // 32 + 1 for ff, c in cat if ff == f), default=1)
        # negative, non-integer, unseen categories at and past the end of the widest bitset, values
        # outside int's range, NaN
        for v in [-1.0, -3.0, -0.5, 3.7, 32.0 * words - 1, 32.0 * words, 32.0 * (words + 1), 1000.0, 3e9, 1e30,
                  -1e30, np.inf, -np.inf, np.nan]:
            r = X[rng.integers(0, X.shape[0], size=8)].copy()
            r[:, f] = v
            rows.append(r)
    return np.ascontiguousarray(np.vstack(rows), dtype=np.float64)


def _train(params, X, y, rounds, **ds_kw):
    p = {"verbosity": -1, "device_type": "cpu", "num_threads": 4, "seed": 1, "deterministic": True}
    p.update(params)
    return lgb.train(p, lgb.Dataset(X, y, params=p, **ds_kw), num_boost_round=rounds)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (booster, probe rows as float64). Cached: callers must not modify the rows."""
    rng = np.random.default_rng(sum(map(ord, name)))
    n, ncol, cat_cols = 2000, 28, ()
    if name == "binary":
        X = rng.normal(size=(n, ncol))
        y = (X[:, 0] + X[:, 1] * X[:, 2] + 0.3 * rng.normal(size=n) > 0).astype(np.float64)
        b = _train({"objective": "binary", "num_leaves": 31}, X, y, 20)
    elif name == "linear":
        ncol = 10
        X = rng.normal(size=(n, ncol))
        y = 2.0 * X[:, 0] - X[:, 1] + np.where(X[:, 2] > 0, X[:, 3], -X[:, 4]) + 0.1 * rng.normal(size=n)
        b = _train({"objective": "regression", "linear_tree": True, "num_leaves": 15}, X, y, 10)
    elif name in ("multiclass", "multiclassova", "multiclass6"):
        ncol = 10
        k = 6 if name == "multiclass6" else 3
        X = rng.normal(size=(n, ncol))
        y = np.floor((np.tanh(X[:, 0] + 0.5 * X[:, 1]) + 1.0) / 2.0 * k).clip(0, k - 1)
        obj = "multiclassova" if name == "multiclassova" else "multiclass"
        b = _train({"objective": obj, "num_class": k, "num_leaves": 15}, X, y, 8)
    elif name == "rf":
        X = rng.normal(size=(n, ncol))
        y = (X[:, 0] - X[:, 3] + 0.3 * rng.normal(size=n) > 0).astype(np.float64)
        b = _train({"objective": "binary", "boosting": "rf", "bagging_freq": 1, "bagging_fraction": 0.7,
                    "feature_fraction": 0.8, "num_leaves": 15}, X, y, 7)
    elif name == "one_leaf":
        n, ncol = 400, 5
        X = rng.normal(size=(n, ncol))
        y = X[:, 0] + rng.normal(size=n)
        b = _train({"objective": "regression", "min_data_in_leaf": 10 * n}, X, y, 3)
        assert b.num_trees() >= 1 and min_leaves(b) == 1
    elif name in ("leaves_below", "leaves_above"):
        n, ncol = 4000, 12
        X = rng.normal(size=(n, ncol))
        y = np.sin(3.0 * X[:, 0]) * X[:, 1] + rng.normal(size=n)
        leaves = 200 if name == "leaves_below" else 400
        b = _train({"objective": "regression", "num_leaves": leaves, "min_data_in_leaf": 1,
                    "min_sum_hessian_in_leaf": 0.0}, X, y, 3)
        if name == "leaves_below":
            assert 128 < max_leaves(b) <= STAGED_TREE_LEAVES
        else:
            assert min_leaves(b) > STAGED_TREE_LEAVES
    elif name in ("missing_nan", "zero_as_missing", "no_missing"):
        ncol = 8
        X = rng.normal(size=(n, ncol))
        y = (np.nan_to_num(X[:, 0]) + X[:, 1] > 0).astype(np.float64)
        if name == "zero_as_missing":
            X[rng.random(size=X.shape) < 0.3] = 0.0
            extra = {"zero_as_missing": True}
        else:
            X[rng.random(size=X.shape) < 0.2] = np.nan
            extra = {"use_missing": name == "missing_nan"}
        b = _train(dict({"objective": "binary", "num_leaves": 15}, **extra), X, y, 10)
    elif name == "categorical":
        ncol, cat_cols = 6, (0,)
        X = rng.normal(size=(n, ncol))
        X[:, 0] = rng.integers(0, 80, size=n)  # more than 32 categories: multi-word bitsets
        effect = rng.normal(size=80)
        y = effect[X[:, 0].astype(int)] + 0.5 * X[:, 1] + 0.1 * rng.normal(size=n)
        b = _train({"objective": "regression", "num_leaves": 15, "min_data_per_group": 5, "cat_smooth": 1.0,
                    "max_cat_to_onehot": 4, "max_cat_threshold": 64}, X, y, 10, categorical_feature=[0])
        _, cat = _splits(b)
        assert cat and max(max(c) for _, c in cat) >= 32, "no multi-word categorical split in the model"
    elif name == "one_column":
        ncol = 1
        X = rng.normal(size=(n, ncol))
        y = np.sin(2.0 * X[:, 0]) + 0.1 * rng.normal(size=n)
        b = _train({"objective": "regression", "num_leaves": 15}, X, y, 10)
    elif name == "wide":
        n, ncol = 500, 600  # above both staged-row limits
        X = rng.normal(size=(n, ncol))
        y = X[:, 0] + X[:, 299] - X[:, 599] + 0.1 * rng.normal(size=n)
        b = _train({"objective": "regression", "num_leaves": 15, "min_data_in_leaf": 5}, X, y, 5)
    else:
        raise KeyError(name)
    return b, _probes(b, X, cat_cols)


def same(a, b):
    """Equal element for element; NaN (a linear leaf's 0 * inf) equals NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
