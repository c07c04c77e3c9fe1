"""k_linear_gram<1|2|4> and k_linear_fold (src/device/linear_kernels.hip) against the
extended-precision Gram systems of linear_gram_cases.py: ops.linear_gram hands host arrays to the
production LaunchLinearGram, one launch per case. Each tile instantiation runs alone (the widest
leaf of the launch picks it), at 1, 3 and 8 row chunks per leaf; one mixed launch puts leaves
without features and with 15 into the four-tile kernel. test_linear_gram_reference_cpu.py checks
the same reference against the host linear learner."""
import numpy as np
import pytest

import linear_gram_cases as lc

pytestmark = pytest.mark.gpu


def _launch(name, chunks):
    from lambdagap_amd import ops

    (raw, g, h), groups = lc.cases()
    leaves = groups[name]
    return ops.linear_gram(raw, g, h, [rows for _, rows, _ in leaves], [feats for _, _, feats in leaves], chunks)


@pytest.mark.parametrize("chunks", lc.CHUNKS)
@pytest.mark.parametrize("name", ["one_tile", "two_tiles", "four_tiles", "mixed"])
def test_gram_systems(gpu_required, name, chunks):
    leaves = lc.cases()[1][name]
    assert (max(k for k, _, _ in leaves) + 2 + 15) // 16 == {"one_tile": 1, "two_tiles": 2}.get(name, 4)
    out, usable = _launch(name, chunks)
    refs = lc.group_reference(name)
    worst = 0.0
    for i, ((k, rows, _), ref) in enumerate(zip(leaves, refs)):
        kind = "range" if isinstance(rows, range) else "list"
        worst = max(worst, lc.worst_ratio(out[i], ref, len(rows), k))
        lc.check_slot(out[i], usable[i], ref, len(rows), k, label=f"{name} chunks={chunks} leaf {i}: k={k} n={len(rows)} {kind}")
    print(f"{name} chunks={chunks}: worst error / bound = {worst:.3g}")
    # the fold order is fixed: a second launch repeats every bit
    out2, usable2 = _launch(name, chunks)
    assert np.array_equal(out.view(np.uint64), out2.view(np.uint64)) and np.array_equal(usable, usable2)


@pytest.mark.parametrize("k", [14, 30, 62])
def test_leaf_of_nan_rows_only_is_zero(gpu_required, k):
    """Every row of the leaf holds a NaN in one of its features (in the first one, the last one
    or in between): an all-zero system, and the usable count of the values before those NaNs."""
    from lambdagap_amd import ops

    (raw, g, h), _ = lc.cases()
    feats = np.arange(3, 3 + k, dtype=np.int32)
    bad = np.flatnonzero(np.isnan(raw[:, feats]).any(axis=1))[:37]
    assert bad.size == 37
    first = np.isnan(raw[np.ix_(bad, feats)]).argmax(axis=1)
    assert first.min() < first.max()
    out, usable = ops.linear_gram(raw, g, h, [bad, range(0, 0)], [feats, feats], 3)
    ref = lc.gram_reference(raw, g, h, bad, feats)
    assert ref[2] == int(first.sum()) and not ref[3].any()
    assert not out.any()
    assert usable.tolist() == [int(first.sum()), 0]
