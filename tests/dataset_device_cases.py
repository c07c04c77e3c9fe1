"""Shared builders for the Dataset-from-GPU-tensors tests (test_dataset_device*.py).

The data follows the recipe of test_device_binning_matches_host_bit_for_bit: NaN, exact zeros
and 1e-40 (below the zero threshold), a categorical column with negative and unseen codes,
few-distinct-value columns and six 93 %-zero columns that EFB bundles. 5,000 rows by default
and bin_construct_sample_cnt=1000, so the bin mappers come from a real sample.
"""
import ctypes

import numpy as np

import lambdagap_amd as lgb
from lambdagap_amd import ops
from lambdagap_amd.basic import _LIB, _c_str, _check, param_dict_to_str

N_ROWS = 5000
SAMPLE_CNT = 1000
CHUNK_ROWS = (1, 700, 2299)  # the chunk list: a one-row chunk, a short one and the rest of 3,000 rows

# thresholds of src/device/bin_kernels.hip
PACK_TILE_BYTES = 32 * 1024   # kPackTileBytes: wider rows take k_pack_rows
PACK_TABLE_BYTES = 96 * 1024  # kPackTableBytes: larger bound tables stay in global memory


def tile_rows(ncol, itemsize):
    """R of LaunchPack: the rows of one LDS tile."""
    return min(1024, PACK_TILE_BYTES // (ncol * itemsize))


def make_matrix(n=N_ROWS, ncol=12, seed=7, dtype=np.float64):
    """The recipe on the first 12 columns (as many as exist); further columns are plain normal."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, ncol))

    def col(j):
        return j < ncol

    if col(0):
        X[rng.random(n) < 0.1, 0] = np.nan                  # NaN -> missing bin
    if col(1):
        X[rng.random(n) < 0.3, 1] = 0.0                     # zero-heavy
        X[rng.random(n) < 0.05, 1] = 1e-40                  # below the zero threshold
    if col(2):
        X[:, 2] = rng.integers(-1, 40, n)                   # categorical (negative -> bin 0)
        X[rng.random(n) < 0.02, 2] = np.nan
    if col(3):
        X[:, 3] = np.round(X[:, 3] * 3)                     # few distinct values
    # sparse columns EFB bundles together: 93 % zero each and mutually exclusive, since a sample
    # of 1,000 rows admits no conflict (max_conflict = sample / 10000); a few rows outside the
    # sample's reach hold two non-zeros, so the packer's first-column-wins rule is exercised
    if ncol >= 12:
        owner = np.where(rng.random(n) < 0.42, rng.integers(6, 12, n), -1)
        for j in range(6, 12):
            X[owner != j, j] = 0.0
        clash = rng.choice(n, max(1, n // 1000), replace=False)
        X[clash, 6:12] = 0.0
        X[clash, 7] = 1.5
        X[clash, 10] = -0.5
    if col(5):
        X[rng.random(n) < 0.05, 5] = np.nan
    return X.astype(dtype)


def make_label(X):
    Z = np.nan_to_num(X.astype(np.float64))
    s = Z[:, 0] + (Z[:, 1] if Z.shape[1] > 1 else 0.0) - (Z[:, 4] if Z.shape[1] > 4 else 0.0)
    return (s > 0).astype(np.float64)


def params_for(ncol, **over):
    p = {"objective": "binary", "num_leaves": 15, "max_bin": 255, "verbosity": -1, "enable_bundle": True,
         "use_missing": True, "bin_construct_sample_cnt": SAMPLE_CNT, "min_data_in_leaf": 5, "device_type": "cpu"}
    if ncol > 2:
        p["categorical_feature"] = [2]
    p.update(over)
    return p


def signature(ds):
    """What "the same Dataset" means here: group layout and every packed group bin."""
    ng, tb, bw, starts = ops.group_layout(ds)
    return (ng, tb, bw), np.asarray(starts).copy(), ops.group_bins(ds)


def same_signature(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def model_text(ds, params, rounds=5, **kw):
    return lgb.train(params, ds, num_boost_round=rounds, **kw).model_to_string()


def strided_args(mats):
    """ctypes arguments (pointers, row counts, element strides) of a list of 2-D numpy views."""
    n = len(mats)
    ptrs = (ctypes.c_void_p * n)(*[ctypes.c_void_p(m.ctypes.data) for m in mats])
    nrows = (ctypes.c_int32 * n)(*[m.shape[0] for m in mats])
    rs = (ctypes.c_int64 * n)(*[m.strides[0] // m.itemsize for m in mats])
    cs = (ctypes.c_int64 * n)(*[m.strides[1] // m.itemsize for m in mats])
    return ptrs, nrows, rs, cs


def hook_dataset(mats, params, label=None, reference=None, entry="LGBM_DatasetTestCreateFromSampledMats"):
    """A Dataset built by the strided-chunk entry points from host numpy views, read in place."""
    mats = [mats] if isinstance(mats, np.ndarray) else list(mats)
    assert all(m.ndim == 2 and m.dtype == mats[0].dtype for m in mats)
    dtype = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}[mats[0].dtype]
    ptrs, nrows, rs, cs = strided_args(mats)
    out = ctypes.c_void_p()
    if reference is not None:
        reference.construct()
    _check(getattr(_LIB, entry)(ctypes.c_int32(len(mats)), ptrs, ctypes.c_int(dtype), nrows,
                                ctypes.c_int32(mats[0].shape[1]), rs, cs, _c_str(param_dict_to_str(params)),
                                reference.handle if reference is not None else None, ctypes.byref(out)))
    ds = lgb.Dataset(None, params=params, reference=reference)
    ds.handle = out
    if label is not None:
        ds.set_label(label)
    return ds


def views_of(X):
    """name -> (a view with the values of X, read in place). X is C-contiguous."""
    n, ncol = X.shape
    big = np.full((n, ncol + 7), 123.0, dtype=X.dtype)
    big[:, 3:3 + ncol] = X
    doubled = np.full((2 * n, ncol), -5.0, dtype=X.dtype)
    doubled[::2] = X
    feature_major = np.ascontiguousarray(X.T)
    sparse2 = np.full((2 * n, 2 * ncol), 9.0, dtype=X.dtype)
    sparse2[::2, ::2] = X
    return {
        "contiguous": X,
        "column_slice": big[:, 3:3 + ncol],
        "row_step": doubled[::2],
        "transposed": feature_major.T,
        "no_unit_stride": sparse2[::2, ::2],
    }
