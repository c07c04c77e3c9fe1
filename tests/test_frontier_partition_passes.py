"""k_f_partition with blocks that own many tiles (LGAP_KERNEL=part_grid caps the grid).

A block of the frontier partition takes the tiles b, b + G, ...: it counts them all, publishing
every count, and only then looks back and scatters them one by one. At test sizes the learner's
grid gives every block a single tile, so these cases cap the grid at 1, 2, 3 and 7 blocks: a block
then owns 9 to 60 tiles (several chunks of them), an expansion ends and the next begins inside one
block's run of tiles, and every look-back has predecessors of its own and of other blocks. The
children lists and left counts are compared with the host learner's stable partition, as in
test_frontier_kernels.py::test_frontier_partition_matches_host (the hook launches the kernel a
second time with every look-back self-counted and checks it places the rows identically).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS = 60_000


def _data(rng, n, nf=10):
    X = rng.standard_normal((n, nf))
    X[rng.random(n) < 0.05, 1] = np.nan          # NaN missing values
    X[rng.random(n) < 0.3, 2] = 0.0              # zero-heavy column
    X[:, 3] = rng.integers(0, 20, n)             # categorical
    y = (X[:, 0] + 0.3 * rng.standard_normal(n) > 0).astype(float)
    return X, y


@pytest.mark.parametrize("part_iters,part_grid", [(4, 1), (4, 3), (4, 7), (16, 2)])
def test_partition_many_tiles_per_block_matches_host(lgb, gpu_required, rng, monkeypatch, part_iters, part_grid):
    from lambdagap_amd import ops

    monkeypatch.setenv("LGAP_KERNEL", f"part_iters={part_iters},part_grid={part_grid}")
    X, y = _data(rng, N_ROWS)
    base = {"objective": "binary", "num_leaves": 31, "verbosity": -1, "device_type": "gpu"}
    ds = lgb.Dataset(X, y, params=base, categorical_feature=[3]).construct()
    n = len(y)
    tile = 256 * part_iters
    # parents: 1 row, exactly one tile, one tile + 1, 5 tiles + 777, the rest
    sizes = [1, tile, tile + 1, 5 * tile + 777]
    sizes.append(n - sum(sizes))
    assert sizes[-1] > tile
    # the parent whose split sends every row right takes rows far above feature 0's lowest bin
    perm = rng.permutation(n)
    high = perm[X[perm, 0] > -1.0]
    right_rows = high[:sizes[2]]
    rest = perm[~np.isin(perm, right_rows)]
    cuts = np.cumsum([0, sizes[0], sizes[1], sizes[3], sizes[4]])
    parts = [rest[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    subsets = [parts[0], parts[1], right_rows, parts[2], parts[3]]
    subsets = [np.sort(s).astype(np.int32) for s in subsets]
    assert [len(s) for s in subsets] == sizes
    nb = [ds.feature_num_bin(f) for f in range(X.shape[1])]
    splits = [
        (3, 0, False, [1, 4, 5, 9, 13]),   # categorical bins to the left
        (0, nb[0] - 1, False, None),       # threshold at the last bin: every row left
        (0, 0, False, None),               # threshold at bin 0: every row right
        (1, nb[1] // 3, False, None),      # NaN rows go right
        (1, nb[1] // 3, True, None),       # NaN rows go left
    ]
    dev_rows, dev_left, host_rows, host_left = ops.frontier_partition(ds, subsets, splits, base)
    np.testing.assert_array_equal(dev_left, host_left)
    assert host_left[1] == sizes[1] and host_left[2] == 0
    assert 0 < host_left[3] < sizes[3] and 0 < host_left[4] < sizes[4]
    # lefts from the front in row order, rights from the back (the host's right list reversed)
    off = np.cumsum([0] + sizes)
    for e, s in enumerate(subsets):
        seg, ref, nl = dev_rows[off[e]:off[e + 1]], host_rows[off[e]:off[e + 1]], dev_left[e]
        np.testing.assert_array_equal(seg[:nl], ref[:nl])
        np.testing.assert_array_equal(seg[nl:][::-1], ref[nl:])
        assert np.array_equal(np.sort(seg), s)  # nothing lost or duplicated


def test_partition_grid_does_not_change_trees(lgb, gpu_required, monkeypatch):
    """The grid only decides which block takes which tile: the children lists, and so the trees,
    are the same with two blocks as with the learner's own grid."""
    rng = np.random.default_rng(31)
    n = 50_000
    X = rng.standard_normal((n, 10))
    y = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.3 * rng.standard_normal(n)
    params = {"objective": "regression", "num_leaves": 31, "min_data_in_leaf": 5, "device_type": "gpu",
              "verbosity": -1, "seed": 4, "deterministic": True}

    def model(kernel):
        monkeypatch.delenv("LGAP_KERNEL", raising=False)
        if kernel:
            monkeypatch.setenv("LGAP_KERNEL", kernel)
        b = lgb.train(params, lgb.Dataset(X, y, params=params), 5, keep_training_booster=True)
        assert "frontier engine" in b.device_name()
        return b.model_to_string()

    assert model("part_grid=2") == model(None)
