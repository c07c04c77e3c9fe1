"""update_device / raw_score_device without a GPU: the markers, and the refusals of a booster
whose scores live on the host. Nothing here falls back to the host path silently."""
import numpy as np
import pytest

import lambdagap_amd as lgb


def _cpu_booster(n=200, extra=None):
    r = np.random.default_rng(0)
    X = r.normal(size=(n, 4))
    y = X[:, 0] + r.normal(size=n) * 0.1
    params = {"objective": "none", "device_type": "cpu", "verbosity": -1, "num_leaves": 7, "min_data_in_leaf": 5}
    params.update(extra or {})
    return lgb.Booster(params, lgb.Dataset(X, y, params=params)), X, y


def test_markers_return_the_same_function_marked():
    def obj(preds, ds):
        return preds, preds

    def metric(preds, ds):
        return "m", 0.0, False

    from lambdagap_amd.basic import _is_device_callable

    assert not _is_device_callable(obj) and not _is_device_callable(metric)
    assert lgb.device_objective(obj) is obj
    assert lgb.device_metric(metric) is metric
    assert _is_device_callable(obj) and _is_device_callable(metric)
    assert not _is_device_callable(lambda p, d: None)


def test_cpu_booster_refuses_and_names_update():
    b, _, _ = _cpu_booster()
    called = []

    def fobj(preds, ds):
        called.append(1)
        return preds, preds

    with pytest.raises(lgb.LightGBMError, match="update"):
        b.update_device(fobj)
    with pytest.raises(lgb.LightGBMError, match="update"):
        b.raw_score_device(0)
    assert not called and b.num_trees() == 0
    # the host path still works on the same booster
    b.update(fobj=lambda preds, ds: (preds - ds.get_label(), np.ones_like(preds)))
    assert b.num_trees() == 1


def test_train_with_a_marked_objective_on_cpu_raises():
    _, X, y = _cpu_booster()

    @lgb.device_objective
    def obj(preds, ds):  # never reached: the library refuses first
        raise AssertionError("a device objective must not run on a host booster")

    with pytest.raises(lgb.LightGBMError, match="update"):
        lgb.train({"objective": obj, "device_type": "cpu", "verbosity": -1}, lgb.Dataset(X, y), num_boost_round=2)


def test_train_with_a_marked_metric_on_cpu_raises():
    _, X, y = _cpu_booster()

    @lgb.device_metric
    def metric(preds, ds):
        raise AssertionError("a device metric must not run on a host booster")

    ds = lgb.Dataset(X, y)
    with pytest.raises(lgb.LightGBMError, match="update"):
        lgb.train({"objective": "regression", "device_type": "cpu", "verbosity": -1}, ds, num_boost_round=2,
                  valid_sets=[ds], feval=metric)


def test_numpy_gradients_raise_type_error():
    b, _, y = _cpu_booster()
    with pytest.raises(TypeError, match="update"):
        b._boost_device(np.zeros(len(y), dtype=np.float32), np.ones(len(y), dtype=np.float32))
    with pytest.raises(TypeError, match="update"):
        b._boost_device(list(np.zeros(len(y))), list(np.ones(len(y))))
    assert b.num_trees() == 0
