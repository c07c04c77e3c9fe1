"""The blended score-update kernels (ops.blend_score) against a NumPy oracle, bit for bit.

boosting=rf keeps a running average of its trees: s = (s * pre + leaf) * post, or / post when an
iteration is rolled back, three separately rounded fp64 operations on the host. The kernels under
test (blend_kernels.hip: the blended k_traverse for 4-, 8- and 16-bit rows, the blended
k_traverse_col for rows past the staged width, the blended constant for a one-leaf tree) make the
same three roundings, so the comparison is on the int64 view of the result, no tolerance. The
oracle is blend_score_cases.oracle: three numpy operations on ``leaf``, the row's raw prediction
of that one tree (test_rf_reference_cpu.py checks that extraction on the CPU).

Scores hold -0.0, subnormals, 1e300 and a value whose product overflows, at the head of three
different row tiles. Every call runs twice; the second result must be the first, bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

from lambdagap_amd import ops

from blend_score_cases import BIG, BLENDS, N, ONE_LEAF, SMALL, layout, oracle
from test_traverse_forest_kernel import LAYOUTS

pytestmark = pytest.mark.gpu

ROWS = [(1, None), (511, None), (512, None), (513, None), (N, None), (N, 2)]  # grid=2: several tiles per block


def _check(lay, n, grid):
    ds = lay.subset(n)
    score = lay.score[:n]
    for tree in (ONE_LEAF, SMALL, BIG):
        for pre, post, divide in BLENDS:
            want = lay_oracle(lay, tree, n, pre, post, divide)
            got = ops.blend_score(ds, lay.booster, tree, score, pre, post, divide=divide, grid=grid)
            what = f"tree {tree}, blend ({pre}, {post}, divide={divide}), {n} rows, grid {grid}"
            assert got.shape == want.shape, what
            bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
            assert bad.size == 0, (f"{what}: {bad.size} rows differ, first row {bad[0]}: score {score[bad[0]]!r}, "
                                   f"got {got[bad[0]]!r}, want {want[bad[0]]!r}")
            again = ops.blend_score(ds, lay.booster, tree, score, pre, post, divide=divide, grid=grid)
            assert np.array_equal(again.view(np.int64), got.view(np.int64)), f"{what}: two runs differ"


def lay_oracle(lay, tree, n, pre, post, divide):
    return oracle(lay.score[:n], lay.leaf[tree, :n], pre, post, divide)


def test_fixture():
    lay = layout("bits8")
    nl = lay.num_leaves()
    assert nl[ONE_LEAF] == 1 and 1 < nl[SMALL] <= 15 and nl[BIG] > 256
    assert np.unique(lay.leaf[ONE_LEAF]).size == 1 and lay.leaf[ONE_LEAF, 0] != 0.0
    s = lay.score
    assert np.signbit(s[0]) and s[0] == 0.0  # -0.0
    assert 0.0 < abs(s[1]) < 2.2250738585072014e-308 and s[3] == 1e300  # a subnormal, 1e300
    assert np.isinf(lay_oracle(lay, SMALL, 8, 8.0, 7.0, True)[5])  # the product overflows
    # the oracle's first-iteration blend is the tree itself, whatever the score was
    assert np.array_equal(lay_oracle(lay, SMALL, N, 0.0, 1.0, False), lay.leaf[SMALL] + 0.0)


@pytest.mark.parametrize("n,grid", ROWS)
def test_row_counts(n, grid):
    _check(layout("bits8"), n, grid)


@pytest.mark.parametrize("kind", [k for k in sorted(LAYOUTS) if k != "bits8"])
@pytest.mark.parametrize("n,grid", [(513, None), (N, 2)])
def test_row_layouts(kind, n, grid):
    _check(layout(kind), n, grid)
