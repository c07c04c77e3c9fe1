"""Booster.predict_contrib_device on the GPU against the library's host hook (the same per-row
function in a host loop: bit for bit) and against Booster.predict(pred_contrib=True) (within
CONTRIB_TOL, see contrib_device_cases.py, which also states the plan's thresholds).

Models are trained on the CPU learner (predict_device_cases.py) or written as text (the chains),
so this file tests only the SHAP kernel; one test at the end trains with device_type=gpu.
"""
import numpy as np
import pytest

import lambdagap_amd as lgb

from contrib_device_cases import (CHAIN_ADDITIVE_UP_TO, CHAIN_LENGTHS, CONTRIB_CASES, CONTRIB_TOL,
                                  MAX_PATH_FEATURES, TILE_ROWS, UPLOAD_CHUNK_BYTES, additivity_err, chain, chain_model_string,
                                  err, hook, lanes, raw_scores)
from predict_device_cases import case, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_required):
    return gpu_required


@pytest.fixture(scope="module")
def refs():
    """Per (case, dtype): booster, rows, the hook's and Booster.predict's SHAP values, computed once."""
    cache = {}

    def get(name, dtype):
        key = (name, np.dtype(dtype).name)
        if key not in cache:
            booster, X64 = case(name)
            X = X64.astype(dtype)
            cache[key] = (booster, X, hook(booster, X), booster.predict(X, pred_contrib=True))
        return cache[key]

    return get


# ---------------------------------------------------------------- numpy input
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", CONTRIB_CASES)
def test_numpy_equals_hook(name, dtype, refs):
    booster, X, hooked, host = refs(name, dtype)
    got = booster.predict_contrib_device(X)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == host.shape
    assert same(got, hooked)
    e = err(got, host)
    a = additivity_err(got, raw_scores(booster, X, name), booster.num_model_per_iteration())
    print(f"{name} {np.dtype(dtype).name}: err {e:.3e} additivity {a:.3e}")
    assert e <= CONTRIB_TOL and a <= CONTRIB_TOL


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nrow", [1, 63, 65, TILE_ROWS, 2 * TILE_ROWS + 313])
def test_row_counts(nrow, dtype, refs):
    assert lanes(14) == TILE_ROWS  # at most 14 unique features on a path of these models
    for name in ("binary", "multiclass6"):
        booster, X, hooked, _ = refs(name, dtype)
        idx = (np.arange(nrow) + 300) % X.shape[0]  # from the first boundary probe on, wrapping
        assert same(booster.predict_contrib_device(np.ascontiguousarray(X[idx])), hooked[idx])


@pytest.mark.parametrize("m", CHAIN_LENGTHS)
def test_long_chain(m):
    booster, X64 = chain(m)
    reps = 2 * lanes(m) // X64.shape[0] + 1  # more than two tiles
    for dtype in (np.float64, np.float32):
        X = np.ascontiguousarray(np.tile(X64, (reps, 1)).astype(dtype))
        got = booster.predict_contrib_device(X)
        assert same(got, hook(booster, X)) and np.all(np.isfinite(got))
        if m <= CHAIN_ADDITIVE_UP_TO:
            assert additivity_err(got, raw_scores(booster, X), 1) <= CONTRIB_TOL


def test_more_than_one_upload_chunk(refs):
    """600 fp64 columns, 601 output columns: 55,830 rows fill a 256 MiB chunk of output; 57,063
    rows are neither a multiple of that nor of the tile. Rows this wide are not staged and their
    contributions are not kept in LDS."""
    booster, X, hooked, _ = refs("wide", np.float64)
    chunk_rows = UPLOAD_CHUNK_BYTES // ((X.shape[1] + 1) * 8)
    nrow = chunk_rows + 1233
    assert nrow % TILE_ROWS != 0 and nrow % chunk_rows != 0
    idx = np.arange(nrow) % X.shape[0]
    big = np.ascontiguousarray(X[idx])
    assert big.nbytes > UPLOAD_CHUNK_BYTES
    assert same(booster.predict_contrib_device(big), hooked[idx])


def test_iteration_slice(refs):
    booster, X, _, _ = refs("binary", np.float64)
    kw = dict(start_iteration=3, num_iteration=5)
    got = booster.predict_contrib_device(X, **kw)
    assert same(got, hook(booster, X, 3, 5))
    assert err(got, booster.predict(X, pred_contrib=True, **kw)) <= CONTRIB_TOL


def test_determinism(refs):
    for name in ("binary", "multiclass6", "leaves_above"):
        booster, X, _, _ = refs(name, np.float32)
        assert same(booster.predict_contrib_device(X), booster.predict_contrib_device(X))


# ---------------------------------------------------------------- device tensors
# One fresh interpreter in which torch creates its GPU context before the library's first GPU
# call (see test_predict_device.py); it reports one verdict per check.
_TENSOR_CHILD = r"""
import json, sys
import numpy as np
import torch
assert torch.cuda.is_available(), "torch sees no GPU"
torch.zeros(1, device="cuda")
torch.cuda.synchronize()
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import lambdagap_amd as lgb
from predict_device_cases import case, same
from contrib_device_cases import CONTRIB_CASES
assert lgb.device_count() >= 1, "the library sees no GPU"


def tensor_case(name, dtype):
    booster, X64 = case(name)
    X = X64.astype(dtype)
    ref = booster.predict_contrib_device(X)
    t = torch.from_numpy(X).cuda()
    got = booster.predict_contrib_device(t)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.device == t.device
    assert tuple(got.shape) == ref.shape == (X.shape[0], booster.num_model_per_iteration() * (booster.num_feature() + 1))
    assert same(got.cpu().numpy(), ref)


def non_contiguous():
    booster, X64 = case("binary")
    X = X64.astype(np.float32)
    pad = np.zeros((X.shape[0], 2 * X.shape[1]), dtype=np.float32)
    pad[:, ::2] = X
    view = torch.from_numpy(pad).cuda()[:, ::2]
    assert not view.is_contiguous()
    assert same(booster.predict_contrib_device(view).cpu().numpy(), booster.predict_contrib_device(X))


def other_dtype():
    booster, X64 = case("binary")
    half = torch.from_numpy(np.round(X64[:100] * 4) / 4).cuda().to(torch.float16)
    ref = booster.predict_contrib_device(half.cpu().numpy().astype(np.float64))
    assert same(booster.predict_contrib_device(half).cpu().numpy(), ref)


def host_tensor_refused():
    booster, X64 = case("binary")
    try:
        booster.predict_contrib_device(torch.from_numpy(X64[:5]))
    except TypeError as e:
        assert "Booster.predict" in str(e)
    else:
        raise AssertionError("a host tensor was accepted")


checks = {f"{name}-{dtype}": (lambda n=name, d=dtype: tensor_case(n, d))
          for name in ("binary", "multiclass6", "wide") for dtype in ("float64", "float32")}
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
@pytest.mark.parametrize("name", ["binary", "multiclass6", "wide"])
def test_tensor_equals_numpy_path(name, dtype, tensor_verdicts):
    assert tensor_verdicts[f"{name}-{dtype}"] == "ok"


@pytest.mark.parametrize("check", ["non_contiguous", "other_dtype", "host_tensor_refused"])
def test_tensor_inputs(check, tensor_verdicts):
    assert tensor_verdicts[check] == "ok"


# ---------------------------------------------------------------- refusals
def test_refusals():
    booster, X = case("linear")
    with pytest.raises(lgb.LightGBMError, match="linear trees.*Booster.predict"):
        booster.predict_contrib_device(X[:10])
    booster, X = case("binary")
    with pytest.raises(lgb.LightGBMError, match="pred_early_stop.*Booster.predict"):
        booster.predict_contrib_device(X[:10], pred_early_stop=True)
    with pytest.raises(lgb.LightGBMError, match="pred_contrib.*Booster.predict"):
        booster.predict_device(X[:10], pred_contrib=True)
    extra = np.ascontiguousarray(np.hstack([X, X[:, :2]]))
    with pytest.raises(lgb.LightGBMError, match="number of features"):
        booster.predict_contrib_device(extra)
    got = booster.predict_contrib_device(extra, predict_disable_shape_check=True)
    assert same(got, hook(booster, X))
    narrow = np.ascontiguousarray(X[:, :20])
    got = booster.predict_contrib_device(narrow, predict_disable_shape_check=True)
    assert same(got, hook(booster, narrow, params="predict_disable_shape_check=true"))
    long_chain = lgb.Booster(model_str=chain_model_string(MAX_PATH_FEATURES + 1))
    with pytest.raises(lgb.LightGBMError, match=f"distinct features.*{MAX_PATH_FEATURES}.*Booster.predict"):
        long_chain.predict_contrib_device(np.ones((3, MAX_PATH_FEATURES + 1)))


# ---------------------------------------------------------------- the real workflow
def test_model_trained_on_the_gpu():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(3000, 28)).astype(np.float32)
    y = (X[:, 0] + X[:, 1] * X[:, 2] > 0).astype(np.float64)
    params = {"objective": "binary", "num_leaves": 31, "device_type": "gpu", "verbosity": -1}
    booster = lgb.train(params, lgb.Dataset(X, y, params=params), num_boost_round=5)
    assert booster.num_trees() == 5
    got = booster.predict_contrib_device(X)
    assert same(got, hook(booster, X))
    assert err(got, booster.predict(X, pred_contrib=True)) <= CONTRIB_TOL
    assert additivity_err(got, booster.predict_device(X, raw_score=True).reshape(-1, 1), 1) <= CONTRIB_TOL
