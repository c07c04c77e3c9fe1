"""The fixtures behind tests/test_blend_score_kernel.py (GPU) and the part of
tests/test_rf_reference_cpu.py that checks them on the CPU: per row layout of
test_traverse_forest_kernel.py one training set, a three-tree booster trained on the CPU (a
one-leaf tree, a tree of at most 15 leaves, a tree of more than 256), every tree's leaf value of
every row (the oracle's input, computed once and left unchanged), and a score vector that holds
the values a blend must get right: either zero, subnormals, values whose products overflow."""
from __future__ import annotations

import numpy as np

import lambdagap_amd as lgb
from test_traverse_forest_kernel import LAYOUTS, N, _data

ONE_LEAF, SMALL, BIG = 0, 1, 2

# (pre, post, divide): the first iteration, the eighth, a rollback from the eighth, the identity
BLENDS = [(0.0, 1.0, False), (7.0, 1.0 / 8.0, False), (8.0, 7.0, True), (1.0, 1.0, False)]


def oracle(score, leaf, pre, post, divide):
    """(score * pre + leaf) * post, or / post: three numpy operations, each rounded on its own."""
    with np.errstate(over="ignore"):
        t = score * np.float64(pre)
        t = t + leaf
        return t / np.float64(post) if divide else t * np.float64(post)


class Layout:
    def __init__(self, kind):
        rng = np.random.default_rng(sorted(LAYOUTS).index(kind) + 31)
        self.X, y = _data(kind, rng)
        extra = dict(LAYOUTS[kind])
        self.cat = extra.pop("categorical_feature", "auto")
        self.params = dict({"objective": "regression", "num_leaves": 15, "min_data_in_leaf": 5, "verbosity": -1,
                            "boost_from_average": False, "device_type": "cpu", "learning_rate": 0.2,
                            "num_threads": 4}, **extra)
        self.ds = lgb.Dataset(self.X, y, params=self.params, categorical_feature=self.cat, free_raw_data=False)
        b = lgb.Booster(dict(self.params, min_gain_to_split=1e30), self.ds)
        b.update()  # no split passes: a one-leaf tree
        b.reset_parameter({"min_gain_to_split": 0.0})
        b.update()
        b.reset_parameter({"num_leaves": 2000, "min_data_in_leaf": 1, "min_sum_hessian_in_leaf": 0.0})
        b.update()
        self.booster = b
        self.leaf = np.stack([b.predict(self.X, start_iteration=j, num_iteration=1, raw_score=True) for j in range(3)])
        self.leaf.setflags(write=False)
        score = rng.normal(size=N) * 5
        # in the first rows, so that every row count down to 1 holds some: -0.0 first
        special = [-0.0, 5e-324, -3e-310, 1e300, -1e300, 1.7e308, 0.0, 2.2250738585072014e-308]
        for rep in range(3):  # again past rows 512 and 1024: other tiles, other lanes
            score[rep * 517: rep * 517 + len(special)] = special
        self.score = score
        self.score.setflags(write=False)
        self._subsets = {N: self.ds}

    def subset(self, n):
        if n not in self._subsets:
            self._subsets[n] = lgb.Dataset(self.X[:n], reference=self.ds, categorical_feature=self.cat).construct()
        return self._subsets[n]

    def num_leaves(self):
        return [t["num_leaves"] for t in self.booster.dump_model()["tree_info"]]


_LAYOUTS = {}


def layout(kind) -> Layout:
    if kind not in _LAYOUTS:
        _LAYOUTS[kind] = Layout(kind)
    return _LAYOUTS[kind]
