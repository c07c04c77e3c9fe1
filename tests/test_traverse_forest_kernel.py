"""k_traverse_forest (ops.forest_score) against a NumPy oracle, bit for bit.

The oracle starts from ``score`` and does ``s += scales[j] * leaf_j`` for each tree j in list order,
``leaf_j`` being the row's leaf value of tree j from ``Booster.predict(X, start_iteration=j,
num_iteration=1, raw_score=True)`` of a one-class regression booster trained without
boost_from_average (so a tree's leaf values are its raw predictions). The product is the IEEE fp64
product that Tree::Shrinkage makes on the host, the sums are the kernel's fp64 adds in the same
order: the comparison is np.array_equal, no tolerance. Every case also runs the per-tree loop
(mode="tree") and the forest kernel a second time, both bit-identical to the first result.

Forest sizes come from ops.forest_runs (the host's run split and byte budget), not from constants:
the largest prefix that is one run, that plus one tree, and a list of at least three runs."""
from __future__ import annotations

import numpy as np
import pytest

import lambdagap_amd as lgb
from lambdagap_amd import ops

pytestmark = pytest.mark.gpu

N = 3000  # rows of every layout's training set; smaller row counts are its leading rows
ROUNDS = 190  # trees of <= 15 leaves: more than three runs of the 20 KiB budget


def _data(kind, rng):
    if kind == "efb":
        # three sparse one-hot blocks (bundled by EFB) and two dense columns
        cols = [np.eye(12)[rng.integers(0, 12, N)] * (rng.random((N, 1)) < 0.5) for _ in range(3)]
        X = np.hstack(cols + [rng.normal(size=(N, 2))])
    elif kind == "wide":
        X = rng.normal(size=(N, 80))  # 80 one-byte groups: 20 dwords per row, past the staged width
    else:
        X = rng.normal(size=(N, 10))
    y = X[:, 0] * 2 + np.sin(X[:, 1] * 3) + X[:, -1] * X[:, 2] + rng.normal(size=N) * 0.3 + 3.0
    if kind in ("bits8", "bits4", "bits16"):
        # NaN where the target runs high (feature 3) and where it runs low (feature 4): default
        # directions on both sides; exact zeros in feature 5
        X[y > np.quantile(y, 0.8), 3] = np.nan
        X[y < np.quantile(y, 0.2), 4] = np.nan
        X[rng.random(N) < 0.3, 5] = 0.0
    if kind == "zero_missing":
        X[y > np.quantile(y, 0.75), 3] = 0.0
        X[y < np.quantile(y, 0.25), 4] = 0.0
        X[rng.random(N) < 0.3, 5] = 0.0
    if kind == "cat":
        X[:, 0] = rng.integers(0, 40, N)
        X[:, 1] = rng.integers(0, 7, N)
        y = y + np.where(X[:, 0] % 3 == 0, 2.0, -1.0) + (X[:, 1] == 4) * 1.5
    return X, y


LAYOUTS = {
    "bits8": {},
    "bits4": {"max_bin": 15},
    "bits16": {"max_bin": 1023, "min_data_in_bin": 1},
    "efb": {},
    "wide": {},
    "zero_missing": {"zero_as_missing": True},
    "cat": {"categorical_feature": [0, 1], "min_data_per_group": 5, "cat_smooth": 1.0},
}


class Layout:
    """One training set, a booster on it, and every tree's leaf value of every row (the oracle's
    input, computed once). Tree 0 is a one-leaf tree (no split passes min_gain_to_split); the last
    tree is larger than the run budget."""

    def __init__(self, kind):
        rng = np.random.default_rng(sorted(LAYOUTS).index(kind) + 11)
        self.X, y = _data(kind, rng)
        extra = dict(LAYOUTS[kind])
        cat = extra.pop("categorical_feature", "auto")
        self.params = dict({"objective": "regression", "num_leaves": 15, "min_data_in_leaf": 5, "verbosity": -1,
                            "boost_from_average": False, "device_type": "cpu", "learning_rate": 0.2,
                            "num_threads": 4}, **extra)
        self.cat = cat
        self.ds = lgb.Dataset(self.X, y, params=self.params, categorical_feature=cat, free_raw_data=False)
        b = lgb.Booster(dict(self.params, min_gain_to_split=1e30), self.ds)
        b.update()
        b.reset_parameter({"min_gain_to_split": 0.0})
        for _ in range(ROUNDS):
            b.update()
        b.reset_parameter({"num_leaves": 2000, "min_data_in_leaf": 1, "min_sum_hessian_in_leaf": 0.0})
        b.update()
        self.booster = b
        self.num_trees = b.num_trees()
        self.big = self.num_trees - 1
        self.leaf = np.stack([b.predict(self.X, start_iteration=j, num_iteration=1, raw_score=True)
                              for j in range(self.num_trees)])
        self.leaf.setflags(write=False)
        self.score = rng.normal(size=N) * 5
        self.score.setflags(write=False)
        self._subsets = {N: self.ds}

    def subset(self, n):
        if n not in self._subsets:
            self._subsets[n] = lgb.Dataset(self.X[:n], reference=self.ds, categorical_feature=self.cat).construct()
        return self._subsets[n]

    def sizes(self):
        """(trees of the largest one-run prefix of trees 1.., a count of >= 3 runs)."""
        budget = ops.forest_runs(self.booster, [])[2]
        fill = 1
        while ops.forest_runs(self.booster, range(1, fill + 2))[0] == [fill + 1]:
            fill += 1
        runs, nbytes, _ = ops.forest_runs(self.booster, range(1, fill + 1))
        assert runs == [fill] and nbytes[0] <= budget
        three = 2 * fill + 2
        assert len(ops.forest_runs(self.booster, range(1, three + 1))[0]) >= 3
        assert three < self.big
        return fill, three


_LAYOUTS = {}


def layout(kind) -> Layout:
    if kind not in _LAYOUTS:
        _LAYOUTS[kind] = Layout(kind)
    return _LAYOUTS[kind]


def _scales(count):
    """-1, 1 / (k + 1) and -k for k = count: DART's three Shrinkage factors, cycled."""
    k = float(max(count, 1))
    return np.array([(-1.0, 1.0 / (k + 1.0), -k)[j % 3] for j in range(count)], dtype=np.float64)


def _check(lay, trees, n, grid=None):
    trees = list(trees)
    scales = _scales(len(trees))
    ds = lay.subset(n)
    score = lay.score[:n]
    want = score.copy()
    for j, t in enumerate(trees):
        want += scales[j] * lay.leaf[t, :n]
    got = ops.forest_score(ds, lay.booster, trees, scales, score, grid=grid)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"forest: {np.count_nonzero(got != want)} of {n} rows differ"
    per_tree = ops.forest_score(ds, lay.booster, trees, scales, score, grid=grid, mode="tree")
    assert np.array_equal(per_tree, got), "the per-tree loop differs from the forest pass"
    again = ops.forest_score(ds, lay.booster, trees, scales, score, grid=grid)
    assert np.array_equal(again, got), "two runs of the same call differ"
    return got


def _forest(lay, which):
    fill, three = lay.sizes()
    return {
        "none": [],
        "one": [3],
        "two": [3, 9],
        "fill": range(1, fill + 1),
        "fill_plus_one": range(1, fill + 2),
        "three_runs": range(1, three + 1),
        "big_tree": [2, lay.big, 4],
        "big_tree_alone": [lay.big],
        "one_leaf_middle": [5, 0, 7],
        "one_leaf_alone": [0],
        "repeated": [6, 6, 0, 6],
    }[which]


FORESTS = ["none", "one", "two", "fill", "fill_plus_one", "three_runs", "big_tree", "big_tree_alone", "one_leaf_middle",
           "one_leaf_alone", "repeated"]


def test_fixture_trees():
    lay = layout("bits8")
    runs, nbytes, budget = ops.forest_runs(lay.booster, [2, lay.big, 4])
    assert runs == [1, 1, 1] and nbytes[1] > budget  # the big tree is a run of its own, past the budget
    assert np.unique(lay.leaf[0]).size == 1 and lay.leaf[0, 0] != 0.0  # tree 0: one leaf
    assert ops.forest_runs(lay.booster, [5, 0, 7])[0] == [3]


@pytest.mark.parametrize("which", FORESTS)
def test_forest_sizes(which):
    lay = layout("bits8")
    got = _check(lay, _forest(lay, which), 1025)
    if which == "none":
        assert np.array_equal(got, lay.score[:1025])


@pytest.mark.parametrize("n,grid", [(1, None), (511, None), (512, None), (513, None), (1025, None), (N, 2)])
def test_row_counts(n, grid):
    lay = layout("bits8")
    _check(lay, _forest(lay, "fill_plus_one"), n, grid)


@pytest.mark.parametrize("kind", [k for k in sorted(LAYOUTS) if k != "bits8"])
@pytest.mark.parametrize("n,grid", [(513, None), (N, 2)])
def test_row_layouts(kind, n, grid):
    lay = layout(kind)
    _check(lay, _forest(lay, "three_runs"), n, grid)
    _check(lay, _forest(lay, "big_tree"), n, grid)


@pytest.mark.parametrize("kind,bits", [("bits4", 4), ("bits8", 8), ("bits16", 16), ("wide", 8)])
def test_rows_the_kernel_reads(kind, bits):
    """The learner hands the forest kernel the row format the layout is named for: 4-bit rows for
    max_bin=15 (k_traverse_forest<0>), and rows past the staged 16 dwords for the wide layout."""
    lay = layout(kind)
    info = {}
    ops.forest_score(lay.ds, lay.booster, [3, 9], [1.0, -1.0], lay.score, info=info)
    assert info["row_bits"] == bits
    assert (info["stride_dw"] > 16) == (kind == "wide")


def test_layouts_are_what_they_claim():
    assert ops.group_layout(layout("bits16").ds)[2] == 2
    assert ops.group_layout(layout("bits8").ds)[2] == 1
    ng = ops.group_layout(layout("efb").ds)[0]
    assert ng < layout("efb").X.shape[1]  # bundles
    assert ops.group_layout(layout("wide").ds)[0] > 64  # more than 16 dwords of one-byte groups
    assert "cat_threshold" in layout("cat").booster.model_to_string()
    model = layout("bits8").booster.dump_model()
    kinds = set()

    def walk(node):
        if "split_index" in node:
            kinds.add((node["missing_type"], node["default_left"]))
            walk(node["left_child"])
            walk(node["right_child"])

    for t in model["tree_info"]:
        walk(t["tree_structure"])
    assert ("NaN", True) in kinds and ("NaN", False) in kinds
    zkinds = set()

    def zwalk(node):
        if "split_index" in node:
            zkinds.add((node["missing_type"], node["default_left"]))
            zwalk(node["left_child"])
            zwalk(node["right_child"])

    for t in layout("zero_missing").booster.dump_model()["tree_info"]:
        zwalk(t["tree_structure"])
    assert ("Zero", True) in zkinds and ("Zero", False) in zkinds
