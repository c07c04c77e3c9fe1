"""Booster.predict_device on the GPU against Booster.predict on the host.

Models are trained on the CPU learner (predict_device_cases.py), so this file tests only the
prediction kernels; one test at the end trains with device_type=gpu. The kernel thresholds the
shapes are chosen around are stated in predict_device_cases.py: a 512-row tile, rows staged in
LDS up to 28 fp32 / 14 fp64 columns, trees staged in LDS up to 256 leaves, more than 4 trees
per iteration accumulated in LDS, host input uploaded in chunks of at most 256 MiB.
"""
import numpy as np
import pytest

import lambdagap_amd as lgb

from predict_device_cases import (CASES, STAGED_COLS_F32, STAGED_COLS_F64, TILE_ROWS, UPLOAD_CHUNK_BYTES, case,
                                  same)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_required):
    return gpu_required


@pytest.fixture(scope="module")
def host_ref():
    """Booster.predict's results per (case, dtype), computed once."""
    cache = {}

    def get(name, dtype):
        key = (name, np.dtype(dtype).name)
        if key not in cache:
            booster, X64 = case(name)
            X = X64.astype(dtype)
            cache[key] = (booster, X, booster.predict(X, raw_score=True), booster.predict(X, pred_leaf=True),
                          booster.predict(X))
        return cache[key]

    return get


# ---------------------------------------------------------------- exactness, numpy input
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", CASES)
def test_numpy_equals_predict(name, dtype, host_ref):
    booster, X, raw, leaf, normal = host_ref(name, dtype)
    if name != "linear":
        assert np.all(np.isfinite(raw))
    got = booster.predict_device(X, raw_score=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    assert same(got, raw)
    got_leaf = booster.predict_device(X, pred_leaf=True)
    assert got_leaf.dtype == leaf.dtype and same(got_leaf, leaf)
    assert same(booster.predict_device(X), normal)


def test_row_staging_limits():
    """28 columns are the last staged fp32 width and above the fp64 limit; the wide model is above both."""
    assert case("binary")[1].shape[1] == STAGED_COLS_F32 > STAGED_COLS_F64
    assert case("wide")[1].shape[1] > STAGED_COLS_F32
    assert case("one_column")[1].shape[1] == 1
    assert case("linear")[1].shape[1] <= STAGED_COLS_F64


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nrow", [1, 63, 65, TILE_ROWS, 2 * TILE_ROWS + 313])
def test_row_counts(nrow, dtype, host_ref):
    for name in ("binary", "multiclass6"):
        booster, X, raw, leaf, _ = host_ref(name, dtype)
        idx = (np.arange(nrow) + 300) % X.shape[0]  # from the first boundary probe on, wrapping
        Xs = np.ascontiguousarray(X[idx])
        assert same(booster.predict_device(Xs, raw_score=True), raw[idx])
        assert same(booster.predict_device(Xs, pred_leaf=True), leaf[idx])


def test_more_than_one_upload_chunk(host_ref):
    """600 fp64 columns: 55,924 rows fill a 256 MiB chunk; 57,157 rows are neither a multiple of
    that nor of the tile."""
    booster, X, raw, _, _ = host_ref("wide", np.float64)
    chunk_rows = UPLOAD_CHUNK_BYTES // (X.shape[1] * 8)
    nrow = chunk_rows + 1233
    assert nrow % TILE_ROWS != 0 and nrow % chunk_rows != 0
    idx = np.arange(nrow) % X.shape[0]
    big = np.ascontiguousarray(X[idx])
    assert big.nbytes > UPLOAD_CHUNK_BYTES
    assert same(booster.predict_device(big, raw_score=True), raw[idx])


def test_iteration_slice(host_ref):
    booster, X, _, _, _ = host_ref("binary", np.float64)
    kw = dict(start_iteration=3, num_iteration=5)
    assert same(booster.predict_device(X, raw_score=True, **kw), booster.predict(X, raw_score=True, **kw))
    leaf = booster.predict(X, pred_leaf=True, **kw)
    assert leaf.shape[1] == 5 and same(booster.predict_device(X, pred_leaf=True, **kw), leaf)
    assert same(booster.predict_device(X, **kw), booster.predict(X, **kw))


def test_other_numpy_dtypes(host_ref):
    booster, X, _, _, _ = host_ref("binary", np.float64)
    Xi = np.round(X[:200] * 4).astype(np.int32)
    assert same(booster.predict_device(Xi, raw_score=True), booster.predict(Xi, raw_score=True))
    Xf = np.asfortranarray(X[:200])
    assert same(booster.predict_device(Xf, raw_score=True), booster.predict(Xf, raw_score=True))


# ---------------------------------------------------------------- device tensors
# torch wheels bundle a ROCm runtime of their own. A process whose first GPU call came from this
# library (as the test session's has, from other modules) no longer lets torch's runtime see the
# device, while a process where torch came first serves both. So the tensor checks run in one
# fresh interpreter in which torch creates its context before the library's first GPU call: the
# order a user holding a GPU tensor has. It reports one verdict per check.
_TENSOR_CHILD = r"""
import json, sys
import numpy as np
import torch
assert torch.cuda.is_available(), "torch sees no GPU"
torch.zeros(1, device="cuda")
torch.cuda.synchronize()
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import lambdagap_amd as lgb
from predict_device_cases import CASES, case, same
assert lgb.device_count() >= 1, "the library sees no GPU"


def tensor_case(name, dtype):
    booster, X64 = case(name)
    X = X64.astype(dtype)
    raw, leaf, normal = booster.predict(X, raw_score=True), booster.predict(X, pred_leaf=True), booster.predict(X)
    t = torch.from_numpy(X).cuda()
    got = booster.predict_device(t, raw_score=True)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.device == t.device
    assert tuple(got.shape) == raw.shape
    # raw scores and leaves equal the numpy path (and so Booster.predict) exactly
    assert same(got.cpu().numpy(), booster.predict_device(X, raw_score=True)) and same(got.cpu().numpy(), raw)
    got_leaf = booster.predict_device(t, pred_leaf=True)
    assert got_leaf.dtype == torch.float64 and got_leaf.device == t.device
    assert same(got_leaf.cpu().numpy(), booster.predict_device(X, pred_leaf=True)) and same(got_leaf.cpu().numpy(), leaf)
    # transformed on the device: the bound of tests/test_device_metrics.py for device-versus-host
    # transcendental results
    conv = booster.predict_device(t)
    assert conv.dtype == torch.float64 and conv.device == t.device and tuple(conv.shape) == normal.shape
    np.testing.assert_allclose(conv.cpu().numpy(), normal, rtol=1e-12, atol=1e-12)


def non_contiguous():
    booster, X64 = case("binary")
    X = X64.astype(np.float32)
    raw = booster.predict(X, raw_score=True)
    pad = np.zeros((X.shape[0], 2 * X.shape[1]), dtype=np.float32)
    pad[:, ::2] = X
    view = torch.from_numpy(pad).cuda()[:, ::2]
    assert not view.is_contiguous()
    got = booster.predict_device(view, raw_score=True).cpu().numpy()
    assert same(got, booster.predict_device(view.contiguous(), raw_score=True).cpu().numpy())
    assert same(got, raw)


def other_dtype():
    booster, X64 = case("binary")
    half = torch.from_numpy(np.round(X64[:100] * 4) / 4).cuda().to(torch.float16)
    ref = booster.predict(half.cpu().numpy().astype(np.float64), raw_score=True)
    assert same(booster.predict_device(half, raw_score=True).cpu().numpy(), ref)


def host_tensor_refused():
    booster, X64 = case("binary")
    try:
        booster.predict_device(torch.from_numpy(X64[:5]))
    except TypeError as e:
        assert "Booster.predict" in str(e)
    else:
        raise AssertionError("a host tensor was accepted")


checks = {f"{name}-{dtype}": (lambda n=name, d=dtype: tensor_case(n, d))
          for name in CASES for dtype in ("float64", "float32")}
checks.update(non_contiguous=non_contiguous, other_dtype=other_dtype, host_tensor_refused=host_tensor_refused)
res = {}
for key, fn in checks.items():
    try:
        fn()
        res[key] = "ok"
    except Exception as e:  # the verdict travels to the parent test
        res[key] = f"{type(e).__name__}: {e}"[:1500]
print("RESULT " + json.dumps(res), flush=True)
"""


@pytest.fixture(scope="module")
def tensor_verdicts():
    import json
    import os
    import subprocess
    import sys

    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _TENSOR_CHILD, os.path.dirname(tests), tests], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", CASES)
def test_tensor_equals_numpy_path(name, dtype, tensor_verdicts):
    assert tensor_verdicts[f"{name}-{dtype}"] == "ok"


@pytest.mark.parametrize("check", ["non_contiguous", "other_dtype", "host_tensor_refused"])
def test_tensor_inputs(check, tensor_verdicts):
    assert tensor_verdicts[check] == "ok"


# ---------------------------------------------------------------- refusals
def test_refusals():
    booster, X = case("binary")
    with pytest.raises(lgb.LightGBMError, match="pred_contrib.*Booster.predict"):
        booster.predict_device(X[:10], pred_contrib=True)
    with pytest.raises(lgb.LightGBMError, match="pred_early_stop.*Booster.predict"):
        booster.predict_device(X[:10], pred_early_stop=True)
    extra = np.ascontiguousarray(np.hstack([X, X[:, :2]]))
    with pytest.raises(lgb.LightGBMError, match="number of features"):
        booster.predict_device(extra)
    got = booster.predict_device(extra, raw_score=True, predict_disable_shape_check=True)
    assert same(got, booster.predict(X, raw_score=True))


# ---------------------------------------------------------------- the real workflow
def test_model_trained_on_the_gpu():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(3000, 28)).astype(np.float32)
    y = (X[:, 0] + X[:, 1] * X[:, 2] > 0).astype(np.float64)
    params = {"objective": "binary", "num_leaves": 31, "device_type": "gpu", "verbosity": -1}
    booster = lgb.train(params, lgb.Dataset(X, y, params=params), num_boost_round=5)
    assert booster.num_trees() == 5
    assert same(booster.predict_device(X, raw_score=True), booster.predict(X, raw_score=True))
    assert same(booster.predict_device(X, pred_leaf=True), booster.predict(X, pred_leaf=True))
    assert same(booster.predict_device(X), booster.predict(X))
