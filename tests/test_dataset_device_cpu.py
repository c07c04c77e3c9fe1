"""The construction logic of Dataset-from-GPU-tensors, checked where there is no GPU.

LGBM_DatasetTestCreateFromSampledMats runs the strided-chunk source of the device path over host
matrices: the bin-construction sample goes through the same compact gathered buffer, the rows
through the host packer over a strided accessor. Its Dataset must equal lgb.Dataset(numpy) on the
same values: group layout, every group bin, and the model text after 5 CPU boosting rounds.
"""
import numpy as np
import pytest

import lambdagap_amd as lgb

from dataset_device_cases import (CHUNK_ROWS, N_ROWS, SAMPLE_CNT, hook_dataset, make_label, make_matrix, model_text,
                                  params_for, same_signature, signature, views_of)


@pytest.fixture(scope="module")
def numpy_ref():
    """The numpy path's dataset signature and model text per dtype, computed once."""
    cache = {}

    def get(dtype):
        key = np.dtype(dtype).name
        if key not in cache:
            X = make_matrix(dtype=dtype)
            y = make_label(X)
            p = params_for(X.shape[1])
            ds = lgb.Dataset(X, y, params=p).construct()
            cache[key] = (X, y, p, signature(ds), model_text(lgb.Dataset(X, y, params=p), p))
        return cache[key]

    return get


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("view", ["contiguous", "column_slice", "transposed", "row_step", "no_unit_stride"])
def test_hook_equals_numpy_path(view, dtype, numpy_ref):
    X, y, p, sig, text = numpy_ref(dtype)
    v = views_of(X)[view]
    assert np.array_equal(v, X, equal_nan=True)
    if view != "contiguous":
        assert not v.flags.c_contiguous
    ds = hook_dataset(v, p, label=y)
    assert ds.num_data() == N_ROWS > SAMPLE_CNT
    assert same_signature(signature(ds), sig)
    assert model_text(ds, p) == text


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hook_chunk_list(dtype):
    n = sum(CHUNK_ROWS)
    X = make_matrix(n=n, dtype=dtype)
    y = make_label(X)
    p = params_for(X.shape[1])
    cuts = np.cumsum((0,) + CHUNK_ROWS)
    # each chunk with strides of its own
    chunks = [np.ascontiguousarray(X[cuts[0]:cuts[1]]), views_of(X[cuts[1]:cuts[2]].copy())["column_slice"],
              views_of(X[cuts[2]:cuts[3]].copy())["transposed"]]
    assert [c.shape[0] for c in chunks] == list(CHUNK_ROWS)
    ref = lgb.Dataset(X, y, params=p).construct()
    ds = hook_dataset(chunks, p, label=y)
    assert same_signature(signature(ds), signature(ref))
    assert model_text(ds, p) == model_text(lgb.Dataset(X, y, params=p), p)
    # the list-of-numpy path agrees as well
    lst = lgb.Dataset([np.ascontiguousarray(c) for c in chunks], y, params=p).construct()
    assert same_signature(signature(lst), signature(ref))


def test_hook_sample_covers_every_row(numpy_ref):
    X, y, _, _, _ = numpy_ref(np.float64)
    p = params_for(X.shape[1], bin_construct_sample_cnt=N_ROWS + 5)
    ref = lgb.Dataset(X, y, params=p).construct()
    ds = hook_dataset(views_of(X)["transposed"], p, label=y)
    assert same_signature(signature(ds), signature(ref))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hook_reference_set(dtype, numpy_ref):
    X, y, p, _, _ = numpy_ref(dtype)
    Xv = make_matrix(n=1237, seed=11, dtype=dtype)
    Xv[5, 2] = 77  # a category the training set has not seen
    yv = make_label(Xv)
    train = lgb.Dataset(X, y, params=p)
    ref = lgb.Dataset(Xv, yv, reference=train).construct()
    ds = hook_dataset(views_of(Xv)["column_slice"], p, label=yv, reference=train)
    assert same_signature(signature(ds), signature(ref))
    # the hook-built training set serves as a reference too
    train_h = hook_dataset(views_of(X)["row_step"], p, label=y)
    ds_h = hook_dataset(views_of(Xv)["transposed"], p, label=yv, reference=train_h)
    assert same_signature(signature(ds_h), signature(ref))


def test_hook_linear_tree_keeps_raw_values(numpy_ref):
    X, y, _, _, _ = numpy_ref(np.float32)
    p = params_for(X.shape[1], linear_tree=True)
    p.pop("categorical_feature")
    ds = hook_dataset(views_of(X)["column_slice"], p, label=y)
    assert model_text(ds, p) == model_text(lgb.Dataset(X, y, params=p), p)


def test_no_gpu_error(numpy_ref):
    if lgb.device_count() >= 1:
        pytest.skip("a GPU is visible")
    X, y, p, _, _ = numpy_ref(np.float32)
    # a host pointer: the entry point must fail before it touches it
    with pytest.raises(lgb.LightGBMError, match="no gfx950 GPU is visible"):
        hook_dataset(X, p, label=y, entry="LGBM_DatasetCreateFromDeviceMats")


def test_host_torch_tensor_takes_the_numpy_path(numpy_ref):
    import torch

    X, y, p, sig, _ = numpy_ref(np.float32)
    t = torch.from_numpy(X)
    assert not t.is_cuda
    ds = lgb.Dataset(t, y, params=p).construct()
    assert same_signature(signature(ds), sig)
    # host tensors as metadata keep working too
    ds2 = lgb.Dataset(X, torch.from_numpy(y), params=p).construct()
    np.testing.assert_array_equal(ds2.get_label(), y.astype(np.float32))
