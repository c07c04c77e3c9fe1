"""Booster.device_predictor without a GPU: the tree-parallel algorithm of its small-batch kernels
(every (row, tree) pair into a [tree][row] array, then the shared fold per row and class), run in
host loops by the library's test hook, against Booster.predict; the no-device error; the inputs
and arguments the predictor refuses."""
import ctypes

import numpy as np
import pytest

import lambdagap_amd as lgb
from lambdagap_amd.basic import _LIB, _c_str, _check

from predict_device_cases import CASES, case, same

C_API_DTYPE_FLOAT32, C_API_DTYPE_FLOAT64 = 0, 1
PREDICT_NORMAL, PREDICT_RAW, PREDICT_LEAF = 0, 1, 2

no_gpu = lgb.device_count() < 1


def hook(booster, X, ptype, start_iteration=0, num_iteration=-1, params=""):
    """LGBM_BoosterTestPackedPredictTreeParallel: pairs, then fold, in plain host loops."""
    X = np.ascontiguousarray(X)
    dtype = C_API_DTYPE_FLOAT32 if X.dtype == np.float32 else C_API_DTYPE_FLOAT64
    n = ctypes.c_int64(0)
    _check(_LIB.LGBM_BoosterCalcNumPredict(booster.handle, ctypes.c_int(X.shape[0]), ctypes.c_int(ptype),
                                           ctypes.c_int(start_iteration), ctypes.c_int(num_iteration),
                                           ctypes.byref(n)))
    out = np.full(n.value, -12345.0, dtype=np.float64)
    out_len = ctypes.c_int64(0)
    _check(_LIB.LGBM_BoosterTestPackedPredictTreeParallel(
        booster.handle, X.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(dtype), ctypes.c_int32(X.shape[0]),
        ctypes.c_int32(X.shape[1]), ctypes.c_int(ptype), ctypes.c_int(start_iteration), ctypes.c_int(num_iteration),
        _c_str(params), ctypes.byref(out_len), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    assert out_len.value == n.value
    return out.reshape(X.shape[0], -1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", CASES)
def test_tree_parallel_hook_equals_predict(name, dtype):
    booster, X64 = case(name)
    X = X64.astype(dtype)
    raw = booster.predict(X, raw_score=True)
    assert same(hook(booster, X, PREDICT_RAW), raw.reshape(X.shape[0], -1))
    if name != "linear":
        assert np.all(np.isfinite(raw))
    assert same(hook(booster, X, PREDICT_LEAF), booster.predict(X, pred_leaf=True))
    assert same(hook(booster, X, PREDICT_NORMAL), booster.predict(X).reshape(X.shape[0], -1))


def test_tree_parallel_hook_one_row():
    for name in ("binary", "multiclass6", "rf"):
        booster, X = case(name)
        raw = booster.predict(X[:1], raw_score=True)
        assert same(hook(booster, X[:1], PREDICT_RAW), raw.reshape(1, -1))


def test_tree_parallel_hook_iteration_slice():
    booster, X = case("binary")
    ref = booster.predict(X, raw_score=True, start_iteration=3, num_iteration=5)
    assert same(hook(booster, X, PREDICT_RAW, 3, 5)[:, 0], ref)
    ref = booster.predict(X, pred_leaf=True, start_iteration=3, num_iteration=5)
    got = hook(booster, X, PREDICT_LEAF, 3, 5)
    assert got.shape[1] == 5 and same(got, ref)
    # multiclass: the fold's stride over the trees of one class starts inside the slice
    booster, X = case("multiclass6")
    ref = booster.predict(X, raw_score=True, start_iteration=3, num_iteration=5)
    assert same(hook(booster, X, PREDICT_RAW, 3, 5), ref)


def test_tree_parallel_hook_shape_check():
    booster, X = case("binary")
    wide = np.ascontiguousarray(np.hstack([X, X[:, :2]]))
    with pytest.raises(lgb.LightGBMError, match="number of features"):
        hook(booster, wide, PREDICT_RAW)
    got = hook(booster, wide, PREDICT_RAW, params="predict_disable_shape_check=true")
    assert same(got[:, 0], booster.predict(X, raw_score=True))
    # fewer columns: the missing ones read as zero, as in Booster.predict
    narrow = np.ascontiguousarray(X[:, :20])
    ref = booster.predict(narrow, raw_score=True, predict_disable_shape_check=True)
    assert same(hook(booster, narrow, PREDICT_RAW, params="predict_disable_shape_check=true")[:, 0], ref)


def test_no_gpu_error():
    if not no_gpu:
        pytest.skip("a GPU is visible: the no-device error cannot be raised")
    booster, _ = case("binary")
    with pytest.raises(lgb.LightGBMError, match="no gfx950 GPU is visible"):
        booster.device_predictor()


def test_tree_parallel_rows_range():
    booster, _ = case("binary")
    for bad in (65537, -1, 1 << 20):
        with pytest.raises(ValueError, match="tree_parallel_rows"):
            booster.device_predictor(tree_parallel_rows=bad)


def test_refused_at_creation():
    booster, _ = case("binary")
    with pytest.raises(lgb.LightGBMError, match="pred_contrib.*Booster.predict"):
        booster.device_predictor(pred_contrib=True)
    with pytest.raises(lgb.LightGBMError, match="pred_early_stop.*Booster.predict"):
        booster.device_predictor(pred_early_stop=True)


class _Unopened(lgb.DevicePredictor):
    """A predictor whose native handle was never made: its input checks run before the library is called."""

    def __init__(self, booster):
        self.booster = booster
        self.handle = ctypes.c_void_p(1)
        self._per_row = {PREDICT_NORMAL: 1, PREDICT_RAW: 1, PREDICT_LEAF: 1}

    def free(self):
        self.handle = None


def test_type_errors(tmp_path):
    booster, X = case("binary")
    import pandas as pd
    import scipy.sparse as sp
    import torch

    path = tmp_path / "rows.txt"
    path.write_text("1 2 3\n")
    pred = booster.device_predictor() if not no_gpu else _Unopened(booster)
    for bad in (pd.DataFrame(X[:5]), sp.csr_matrix(X[:5]), str(path), path, lgb.Dataset(X[:5]), X[:5].tolist(),
                torch.from_numpy(X[:5])):
        with pytest.raises(TypeError, match="Booster.predict"):
            pred.predict(bad)
    pred.free()
    with pytest.raises(lgb.LightGBMError, match="after free"):
        pred.predict(X[:5])
