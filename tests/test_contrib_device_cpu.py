"""Booster.predict_contrib_device without a GPU: the path pack and the shared per-row function,
run in a host loop by the library's test hook, against Booster.predict(pred_contrib=True) and
against the raw score; the refusals; the no-device error; the inputs the method refuses."""
import numpy as np
import pytest

import lambdagap_amd as lgb

from contrib_device_cases import (CHAIN_ADDITIVE_UP_TO, CHAIN_LENGTHS, CONTRIB_CASES, CONTRIB_TOL,
                                  MAX_PATH_FEATURES, additivity_err, chain, chain_model_string, err, hook,
                                  raw_scores)
from predict_device_cases import case, same


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", CONTRIB_CASES)
def test_hook_against_predict(name, dtype):
    booster, X64 = case(name)
    X = X64.astype(dtype)
    k = booster.num_model_per_iteration()
    ref = booster.predict(X, pred_contrib=True)
    got = hook(booster, X)
    assert got.shape == ref.shape == (X.shape[0], k * (booster.num_feature() + 1))
    assert np.all(np.isfinite(got))
    e = err(got, ref)
    a = additivity_err(got, raw_scores(booster, X, name), k)
    print(f"{name} {np.dtype(dtype).name}: err {e:.3e} additivity {a:.3e}")
    assert e <= CONTRIB_TOL
    assert a <= CONTRIB_TOL
    # the expected values: the host's formula, added in the host's order
    block = booster.num_feature() + 1
    assert same(got[:, block - 1::block], ref[:, block - 1::block])
    if name == "one_leaf":  # the bias only
        assert not got[:, :block - 1].any()


def test_hook_iteration_slice():
    booster, X = case("binary")
    ref = booster.predict(X, pred_contrib=True, start_iteration=3, num_iteration=5)
    got = hook(booster, X, 3, 5)
    assert err(got, ref) <= CONTRIB_TOL and same(got[:, -1], ref[:, -1])
    assert additivity_err(got, raw_scores(booster, X, start_iteration=3, num_iteration=5), 1) <= CONTRIB_TOL
    assert err(got, hook(booster, X)) > 1e-3  # a slice, not the whole model


def test_hook_shape_check():
    booster, X = case("binary")
    wide = np.ascontiguousarray(np.hstack([X, X[:, :2]]))
    with pytest.raises(lgb.LightGBMError, match="number of features"):
        hook(booster, wide)
    got = hook(booster, wide, params="predict_disable_shape_check=true")
    assert same(got, hook(booster, X))
    assert err(got, booster.predict(X, pred_contrib=True)) <= CONTRIB_TOL
    # fewer columns: the missing ones read as zero, as in Booster.predict
    narrow = np.ascontiguousarray(X[:, :20])
    ref = booster.predict(narrow, pred_contrib=True, predict_disable_shape_check=True)
    got = hook(booster, narrow, params="predict_disable_shape_check=true")
    assert got.shape == ref.shape and err(got, ref) <= CONTRIB_TOL


def test_refusals():
    booster, X = case("linear")
    with pytest.raises(lgb.LightGBMError, match="linear trees.*Booster.predict"):
        hook(booster, X)
    booster, X = case("binary")
    with pytest.raises(lgb.LightGBMError, match="pred_early_stop.*Booster.predict"):
        hook(booster, X, params="pred_early_stop=true")


@pytest.mark.parametrize("m", CHAIN_LENGTHS)
def test_long_chain(m):
    booster, X = chain(m)
    got = hook(booster, X)
    assert got.shape == (X.shape[0], m + 1) and np.all(np.isfinite(got))
    a = additivity_err(got, raw_scores(booster, X), 1)
    print(f"chain {m}: additivity {a:.3e}")
    if m <= CHAIN_ADDITIVE_UP_TO:
        assert a <= CONTRIB_TOL
    # no feature repeats on a chain, so the host runs the same recurrences in another order
    ref = booster.predict(X, pred_contrib=True)
    assert err(got, ref) <= CONTRIB_TOL and same(got[:, -1], ref[:, -1])


def test_chain_past_the_limit():
    booster = lgb.Booster(model_str=chain_model_string(MAX_PATH_FEATURES + 1))
    X = np.ones((3, MAX_PATH_FEATURES + 1))
    with pytest.raises(lgb.LightGBMError, match=f"{MAX_PATH_FEATURES + 1} distinct features.*{MAX_PATH_FEATURES}.*Booster.predict"):
        hook(booster, X)
    assert np.all(np.isfinite(booster.predict(X, pred_contrib=True)))  # the host has no such limit


def test_no_gpu_error():
    if lgb.device_count() >= 1:
        pytest.skip("a GPU is visible: the no-device error cannot be raised")
    booster, X = case("binary")
    with pytest.raises(lgb.LightGBMError, match="no gfx950 GPU is visible"):
        booster.predict_contrib_device(X)


def test_predict_device_still_refuses_contrib():
    booster, X = case("binary")
    with pytest.raises(lgb.LightGBMError, match="pred_contrib.*Booster.predict"):
        booster.predict_device(X, pred_contrib=True)


def test_type_errors(tmp_path):
    booster, X = case("binary")
    import pandas as pd
    import scipy.sparse as sp

    path = tmp_path / "rows.txt"
    path.write_text("1 2 3\n")
    for bad in (pd.DataFrame(X[:5]), sp.csr_matrix(X[:5]), str(path), path, lgb.Dataset(X[:5]), X[:5].tolist()):
        with pytest.raises(TypeError, match="Booster.predict"):
            booster.predict_contrib_device(bad)
