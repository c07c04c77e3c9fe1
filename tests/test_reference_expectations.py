"""Numeric expectations of the reference's Python tests, re-checked on this framework.

Each case trains what the named reference test trains (same sklearn dataset, split, seed and
parameters) and checks the reference's published bound, plus agreement between the recorded
evaluation and an independent recomputation. Source:
/root/reference/tests/python_package_test/test_engine.py (test names in each docstring).
"""
import numpy as np
import pytest
from sklearn.datasets import load_breast_cancer, load_digits, make_regression
from sklearn.metrics import log_loss, mean_squared_error, roc_auc_score
from sklearn.model_selection import train_test_split


def _split(X, y):
    return train_test_split(X, y, test_size=0.1, random_state=42)


def _train_with_record(lgb, params, X_tr, y_tr, X_va, y_va, rounds):
    ds = lgb.Dataset(X_tr, y_tr, params=params)
    va = lgb.Dataset(X_va, y_va, reference=ds, params=params)
    rec = {}
    b = lgb.train(params, ds, num_boost_round=rounds, valid_sets=va, callbacks=[lgb.record_evaluation(rec)])
    return b, rec["valid_0"]


def _multi_logloss(y, p):
    return float(np.mean([-np.log(p[i][int(c)]) for i, c in enumerate(y)]))


def _top_k_error(y, p, k):
    if k == p.shape[1]:
        return 0.0
    max_rest = np.max(-np.partition(-p, k)[:, k:], axis=1)
    return 1 - np.mean((p[np.arange(len(y)), y] > max_rest))


def test_binary_logloss_bound_and_num_iteration_alias(lgb):
    """test_binary: 50 rounds from `num_iteration` in params override num_boost_round=20."""
    X_tr, X_te, y_tr, y_te = _split(*load_breast_cancer(return_X_y=True))
    params = {"objective": "binary", "metric": "binary_logloss", "verbose": -1, "num_iteration": 50}
    b, rec = _train_with_record(lgb, params, X_tr, y_tr, X_te, y_te, 20)
    ret = log_loss(y_te, b.predict(X_te))
    assert ret < 0.14
    assert len(rec["binary_logloss"]) == 50
    assert rec["binary_logloss"][-1] == pytest.approx(ret)


def test_random_forest_logloss_bound(lgb):
    """test_rf."""
    X_tr, X_te, y_tr, y_te = _split(*load_breast_cancer(return_X_y=True))
    params = {"boosting_type": "rf", "objective": "binary", "bagging_freq": 1, "bagging_fraction": 0.5,
              "feature_fraction": 0.5, "num_leaves": 50, "metric": "binary_logloss", "verbose": -1}
    b, rec = _train_with_record(lgb, params, X_tr, y_tr, X_te, y_te, 50)
    ret = log_loss(y_te, b.predict(X_te))
    assert ret < 0.19
    assert rec["binary_logloss"][-1] == pytest.approx(ret)


@pytest.mark.parametrize("objective,bound", [("regression", 343), ("regression_l1", 343), ("huber", 430),
                                             ("fair", 296), ("poisson", 193), ("quantile", 1311)])
def test_regression_objectives_mse_bounds(lgb, objective, bound):
    """test_regression: |y| of sklearn make_regression(100, 4, 2, random_state=42)."""
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    X_tr, X_te, y_tr, y_te = _split(X, np.abs(y))
    params = {"objective": objective, "metric": "l2", "verbose": -1}
    b, rec = _train_with_record(lgb, params, X_tr, y_tr, X_te, y_te, 50)
    ret = mean_squared_error(y_te, b.predict(X_te))
    assert ret < bound
    assert rec["l2"][-1] == pytest.approx(ret)


@pytest.mark.parametrize("fill,label,n_special", [(0.0, 1.0, 20), (1.0, 0.0, 80)])
def test_missing_values_learned_by_default_direction(lgb, fill, label, n_special):
    """test_missing_value_handle / _more_na: a NaN-only signal is learned exactly."""
    rng = np.random.default_rng(7)
    X = np.full((100, 1), fill)
    y = np.full(100, fill)
    idx = rng.choice(100, n_special, replace=False)
    X[idx, 0] = np.nan
    y[idx] = label
    params = {"metric": "l2", "verbose": -1, "boost_from_average": False}
    b, rec = _train_with_record(lgb, params, X, y, X, y, 20)
    ret = mean_squared_error(y, b.predict(X))
    assert ret < 0.005
    assert rec["l2"][-1] == pytest.approx(ret)


_ONE_SPLIT = {"objective": "regression", "metric": "auc", "verbose": -1, "boost_from_average": False, "min_data": 1,
              "num_leaves": 2, "learning_rate": 1, "min_data_in_bin": 1}


@pytest.mark.parametrize("extra,y,exact,auc_floor", [
    ({"zero_as_missing": False}, [1, 1, 1, 1, 0, 0, 0, 0, 1], True, 0.999),   # test_missing_value_handle_na
    ({"zero_as_missing": True}, [0, 1, 1, 1, 0, 0, 0, 0, 0], True, 0.999),    # test_missing_value_handle_zero
    ({"use_missing": False}, [0, 1, 1, 1, 0, 0, 0, 0, 0], False, 0.83),       # test_missing_value_handle_none
])
def test_missing_value_modes_single_split(lgb, extra, y, exact, auc_floor):
    X = np.array([0, 1, 2, 3, 4, 5, 6, 7, np.nan]).reshape(-1, 1)
    y = np.array(y, dtype=float)
    b, rec = _train_with_record(lgb, dict(_ONE_SPLIT, **extra), X, y, X, y, 1)
    pred = b.predict(X)
    if exact:
        np.testing.assert_allclose(pred, y)
    else:
        assert pred[0] == pytest.approx(pred[1]) and pred[-1] == pytest.approx(pred[0])
    ret = roc_auc_score(y, pred)
    assert ret > auc_floor
    assert rec["auc"][-1] == pytest.approx(ret)


@pytest.mark.parametrize("quantized", [False, True])
@pytest.mark.parametrize("x,y,zero_as_missing", [
    ([0, 1, 2, 3, 4, 5, 6, 7], [0, 1, 0, 1, 0, 1, 0, 1], True),               # test_categorical_handle
    ([0, np.nan, 0, np.nan, 0, np.nan], [0, 1, 0, 1, 0, 1], False),           # test_categorical_handle_na
    ([1, 1, 1, 1, 1, 1, 2, 2], [1, 1, 1, 1, 1, 1, 0, 0], False),              # test_categorical_non_zero_inputs
])
def test_categorical_single_split_is_exact(lgb, x, y, zero_as_missing, quantized):
    X = np.array(x, dtype=float).reshape(-1, 1)
    y = np.array(y, dtype=float)
    params = dict(_ONE_SPLIT, min_data_per_group=1, cat_smooth=1, cat_l2=0, max_cat_to_onehot=1,
                  zero_as_missing=zero_as_missing, categorical_column=0, use_quantized_grad=quantized)
    b, rec = _train_with_record(lgb, params, X, y, X, y, 1)
    pred = b.predict(X)
    np.testing.assert_allclose(pred, y)
    ret = roc_auc_score(y, pred)
    assert ret > 0.999
    assert rec["auc"][-1] == pytest.approx(ret)


def test_multiclass_logloss_bound(lgb):
    """test_multiclass: digits, 10 classes."""
    X_tr, X_te, y_tr, y_te = _split(*load_digits(n_class=10, return_X_y=True))
    params = {"objective": "multiclass", "metric": "multi_logloss", "num_class": 10, "verbose": -1}
    b, rec = _train_with_record(lgb, params, X_tr, y_tr, X_te, y_te, 50)
    ret = _multi_logloss(y_te, b.predict(X_te))
    assert ret < 0.16
    assert rec["multi_logloss"][-1] == pytest.approx(ret)


def test_multiclass_random_forest_logloss_bound(lgb):
    """test_multiclass_rf."""
    X_tr, X_te, y_tr, y_te = _split(*load_digits(n_class=10, return_X_y=True))
    params = {"boosting_type": "rf", "objective": "multiclass", "metric": "multi_logloss", "bagging_freq": 1,
              "bagging_fraction": 0.6, "feature_fraction": 0.6, "num_class": 10, "num_leaves": 50, "min_data": 1,
              "verbose": -1, "gpu_use_dp": True}
    b, rec = _train_with_record(lgb, params, X_tr, y_tr, X_te, y_te, 50)
    ret = _multi_logloss(y_te, b.predict(X_te))
    assert ret < 0.23
    assert rec["multi_logloss"][-1] == pytest.approx(ret)


def test_multiclass_prediction_early_stopping_bounds(lgb):
    """test_multiclass_prediction_early_stopping: margin 1.5 stops early (loss in (0.6, 0.8)),
    margin 5.5 nearly never stops (loss < 0.2)."""
    X_tr, X_te, y_tr, y_te = _split(*load_digits(n_class=10, return_X_y=True))
    params = {"objective": "multiclass", "metric": "multi_logloss", "num_class": 10, "verbose": -1}
    b = lgb.train(params, lgb.Dataset(X_tr, y_tr, params=params), num_boost_round=50)
    kw = {"pred_early_stop": True, "pred_early_stop_freq": 5, "pred_early_stop_margin": 1.5}
    ret = _multi_logloss(y_te, b.predict(X_te, **kw))
    assert 0.6 < ret < 0.8
    kw["pred_early_stop_margin"] = 5.5
    assert _multi_logloss(y_te, b.predict(X_te, **kw)) < 0.2


def test_multi_error_top_k(lgb):
    """test_multi_class_error: multi_error@k matches an independent top-k error, k = 1, 2, 10,
    and the tie conventions on identical predictions."""
    X, y = load_digits(n_class=10, return_X_y=True)
    params = {"objective": "multiclass", "num_classes": 10, "metric": "multi_error", "num_leaves": 4, "verbose": -1}
    ds = lgb.Dataset(X, label=y)
    default = lgb.train(params, ds, num_boost_round=10).predict(X)
    for k, name in ((1, "multi_error"), (2, "multi_error@2"), (10, "multi_error@10")):
        rec = {}
        b = lgb.train(dict(params, multi_error_top_k=k), ds, num_boost_round=10, valid_sets=[ds],
                      callbacks=[lgb.record_evaluation(rec)])
        p = b.predict(X)
        if k == 1:
            np.testing.assert_allclose(p, default)
        assert rec["training"][name][-1] == pytest.approx(_top_k_error(y, p, k))
    Xs, ys = np.array([[0, 0], [0, 0]]), np.array([0, 1])
    ds2 = lgb.Dataset(Xs, label=ys)
    p2 = dict(params, num_classes=2)
    for k, name, want in ((1, "multi_error", 1.0), (2, "multi_error@2", 0.0)):
        rec = {}
        lgb.train(dict(p2, multi_error_top_k=k), ds2, num_boost_round=10, valid_sets=[ds2],
                  callbacks=[lgb.record_evaluation(rec)])
        assert rec["training"][name][-1] == pytest.approx(want)


def test_auc_mu_matches_binary_auc_and_weights(lgb):
    """test_auc_mu: two classes equal binary AUC; all-equal predictions give 0.5; weights change
    it, uniform weights do not."""
    X, y = load_digits(n_class=10, return_X_y=True)
    y2 = (y != 0).astype(float)
    ds = lgb.Dataset(X, label=y2)
    mu, auc = {}, {}
    lgb.train({"objective": "multiclass", "metric": "auc_mu", "verbose": -1, "num_classes": 2, "seed": 0}, ds, 10,
              valid_sets=[ds], callbacks=[lgb.record_evaluation(mu)])
    lgb.train({"objective": "binary", "metric": "auc", "verbose": -1, "seed": 0}, ds, 10, valid_sets=[ds],
              callbacks=[lgb.record_evaluation(auc)])
    np.testing.assert_allclose(mu["training"]["auc_mu"], auc["training"]["auc"])
    params = {"objective": "multiclass", "metric": "auc_mu", "verbose": -1, "num_classes": 2, "min_data_in_leaf": 20,
              "seed": 0}
    small = lgb.Dataset(X[:10], label=y2[:10])
    mu = {}
    lgb.train(params, small, 10, valid_sets=[small], callbacks=[lgb.record_evaluation(mu)])
    assert mu["training"]["auc_mu"][-1] == pytest.approx(0.5)
    params = dict(params, num_classes=10, num_leaves=5)
    rng = np.random.default_rng(3)
    res = {}
    for name, w in (("plain", None), ("weighted", np.abs(rng.standard_normal(y.shape))), ("half", np.full(y.shape, 0.5))):
        d = lgb.Dataset(X, label=y, weight=w)
        r = {}
        lgb.train(params, d, 10, valid_sets=[d], callbacks=[lgb.record_evaluation(r)])
        res[name] = r["training"]["auc_mu"][-1]
    assert res["weighted"] < 1 and res["weighted"] != res["plain"]
    assert res["half"] == pytest.approx(res["plain"], abs=1e-5)


# ---------------------------------------------------------------------------
# ranking: prediction early stopping, position bias (test_engine.py:651-868)
import itertools  # noqa: E402
import os  # noqa: E402
import random  # noqa: E402
import shutil  # noqa: E402

from sklearn.datasets import load_svmlight_file  # noqa: E402
from sklearn.metrics import mean_absolute_error  # noqa: E402

DATA = os.path.join(os.path.dirname(__file__), "data")


def test_rank_xendcg_prediction_early_stopping_changes_scores(lgb):
    """test_ranking_prediction_early_stopping."""
    X, y = load_svmlight_file(os.path.join(DATA, "rank.train"))
    q = np.loadtxt(os.path.join(DATA, "rank.train.query"))
    Xt, _ = load_svmlight_file(os.path.join(DATA, "rank.test"), n_features=X.shape[1])
    params = {"objective": "rank_xendcg", "verbose": -1}
    b = lgb.train(params, lgb.Dataset(X, y, group=q, params=params), num_boost_round=50)
    kw = {"pred_early_stop": True, "pred_early_stop_freq": 5, "pred_early_stop_margin": 1.5}
    loose = b.predict(Xt, **kw)
    kw["pred_early_stop_margin"] = 5.5
    assert not np.allclose(loose, b.predict(Xt, **kw))


def _biased_clicks(src, query_file, dst, baseline_feature=34):
    """Cascade click model over the ranking of `baseline_feature` (the reference's
    simulate_position_bias): click probability by true grade, stop probability 0.2 after each
    document, python `random` seeded with 10. Returns each document's displayed position."""
    p_click = {0: 0.4, 1: 0.6, 2: 0.7, 3: 0.8}
    random.seed(10)
    positions_all = []
    with open(src) as fin, open(dst, "w") as fout:
        for line in open(query_file):
            n = int(line)
            rows = [fin.readline().split() for _ in range(n)]
            key = []
            for i, tok in enumerate(rows):
                v = 0.0
                for t in tok[1:]:
                    f, x = t.split(":")
                    if int(f) == baseline_feature:
                        v = float(x)
                key.append((i, v))
            key.sort(key=lambda kv: -kv[1])
            pos = [0] * n
            stop = False
            for rank, (i, _) in enumerate(key):
                new = 0
                if not stop:
                    if random.random() < p_click.get(int(rows[i][0]), 0.9):
                        new = 1
                    stop = random.random() < 0.2
                rows[i][0] = str(new)
                pos[i] = rank
            for tok in rows:
                fout.write(" ".join(tok) + "\n")
            positions_all.extend(pos)
    return positions_all


_POS_PARAMS = {"objective": "lambdarank", "verbose": -1, "eval_at": [3], "metric": "ndcg", "bagging_freq": 1,
               "bagging_fraction": 0.9, "min_data_in_leaf": 50, "min_sum_hessian_in_leaf": 5.0}


def _biased_copy(tmp_path):
    pos = _biased_clicks(os.path.join(DATA, "rank.train"), os.path.join(DATA, "rank.train.query"),
                         str(tmp_path / "rank.train"))
    for f in ("rank.train.query", "rank.test", "rank.test.query"):
        shutil.copy(os.path.join(DATA, f), tmp_path / f)
    return pos


def _ndcg3(lgb, params, train):
    valid = [train.create_valid(str(train.data).replace("rank.train", "rank.test"))]
    return lgb.train(params, train, valid_sets=valid, num_boost_round=50).best_score["valid_0"]["ndcg@3"]


def test_position_bias_from_file_improves_ndcg(lgb, tmp_path):
    """test_ranking_with_position_information_with_file: unbiased LambdaMART with a .position
    side file beats the plain one on click labels by >= 0.03 NDCG@3; a position file longer
    than the data is an error."""
    pos = _biased_copy(tmp_path)
    fn = str(tmp_path / "rank.train")
    base = _ndcg3(lgb, _POS_PARAMS, lgb.Dataset(fn, params=_POS_PARAMS))
    np.savetxt(tmp_path / "rank.train.position", np.array(pos), fmt="%d")
    unbiased = _ndcg3(lgb, _POS_PARAMS, lgb.Dataset(fn, params=_POS_PARAMS))
    assert base + 0.03 <= unbiased
    with open(tmp_path / "rank.train.position", "a") as f:
        f.write("pos_1000\n")
    with pytest.raises(lgb.basic.LightGBMError, match=r"Positions size \(3006\) doesn't match data size"):
        _ndcg3(lgb, _POS_PARAMS, lgb.Dataset(fn, params=_POS_PARAMS))


def test_position_bias_via_constructor_and_setter(lgb, tmp_path):
    """test_ranking_with_position_information_with_dataset_constructor."""
    import pandas as pd

    params = dict(_POS_PARAMS, num_threads=1, deterministic=True, seed=0)
    pos = np.array(_biased_copy(tmp_path))
    fn = str(tmp_path / "rank.train")
    base = _ndcg3(lgb, params, lgb.Dataset(fn, params=params))
    unbiased = _ndcg3(lgb, params, lgb.Dataset(fn, params=params, position=pos))
    assert base + 0.03 <= unbiased
    assert _ndcg3(lgb, params, lgb.Dataset(fn, params=params, position=pd.Series(pos))) == unbiased
    ds = lgb.Dataset(fn, params=params)
    ds.set_position(pos)
    assert _ndcg3(lgb, params, ds) == unbiased
    np.testing.assert_array_equal(ds.get_position(), pos)


# ---------------------------------------------------------------------------
# early stopping (test_engine.py:842-1143)
_decreasing = itertools.count(0, -1)


def _constant_metric(preds, data):
    return ("error", 0.0, False)


def _decreasing_metric(preds, data):
    return ("decreasing_metric", next(_decreasing), False)


def _cancer_split(lgb):
    X_tr, X_te, y_tr, y_te = _split(*load_breast_cancer(return_X_y=True))
    tr = lgb.Dataset(X_tr, y_tr)
    return tr, lgb.Dataset(X_te, y_te, reference=tr)


def test_early_stopping_callback_best_iteration(lgb):
    """test_early_stopping."""
    params = {"objective": "binary", "metric": "binary_logloss", "verbose": -1}
    tr, va = _cancer_split(lgb)
    b = lgb.train(params, tr, num_boost_round=10, valid_sets=va, valid_names="valid_set",
                  callbacks=[lgb.early_stopping(stopping_rounds=5)])
    assert b.best_iteration == 10
    assert "binary_logloss" in b.best_score["valid_set"]
    b = lgb.train(params, tr, num_boost_round=40, valid_sets=va, valid_names="valid_set",
                  callbacks=[lgb.early_stopping(stopping_rounds=5)])
    assert b.best_iteration <= 39
    assert "binary_logloss" in b.best_score["valid_set"]


@pytest.mark.parametrize("use_valid", [True, False])
def test_early_stopping_ignores_training_set_ref(lgb, use_valid):
    """test_early_stopping_ignores_training_set."""
    x = np.linspace(-1, 1, 100)
    X, y = x.reshape(-1, 1), x ** 2
    tr, va = lgb.Dataset(X[:80], y[:80]), lgb.Dataset(X[80:], y[80:])
    sets, names = [tr], ["train"]
    if use_valid:
        sets.append(va)
        names.append("valid")
    rec = {}

    def run():
        return lgb.train({"num_leaves": 5}, tr, num_boost_round=2, valid_sets=sets, valid_names=names,
                         callbacks=[lgb.early_stopping(1), lgb.record_evaluation(rec)])

    if use_valid:
        b = run()
        assert b.best_iteration == 1
        assert rec["train"]["l2"][1] < rec["train"]["l2"][0]
        assert rec["valid"]["l2"][1] > rec["valid"]["l2"][0]
    else:
        with pytest.warns(UserWarning, match="Only training set found, disabling early stopping."):
            b = run()
        assert b.current_iteration() == 2
        assert b.best_iteration == 0


@pytest.mark.parametrize("first_metric_only", [True, False])
def test_early_stopping_from_params_and_first_metric_only(lgb, first_metric_only):
    """test_early_stopping_via_global_params."""
    params = {"num_trees": 5, "objective": "binary", "metric": "None", "verbose": -1, "early_stopping_round": 2,
              "first_metric_only": first_metric_only}
    tr, va = _cancer_split(lgb)
    b = lgb.train(params, tr, feval=[_decreasing_metric, _constant_metric], valid_sets=va, valid_names="valid_set")
    assert b.best_iteration == (5 if first_metric_only else 1)
    assert "decreasing_metric" in b.best_score["valid_set"] and "error" in b.best_score["valid_set"]


@pytest.mark.parametrize("rounds", [-10, -1, 0, None, "None"])
def test_non_positive_early_stopping_rounds_disable_it(lgb, rounds):
    """test_early_stopping_is_not_enabled_for_non_positive_stopping_rounds."""
    params = {"num_trees": 5, "objective": "binary", "metric": "None", "verbose": -1, "early_stopping_round": rounds,
              "first_metric_only": True}
    tr, va = _cancer_split(lgb)
    if rounds == "None":
        with pytest.raises(TypeError, match="early_stopping_round should be an integer. Got 'str'"):
            lgb.train(params, tr, feval=[_constant_metric], valid_sets=va, valid_names="valid_set")
        return
    b = lgb.train(params, tr, feval=[_constant_metric], valid_sets=va, valid_names="valid_set")
    if rounds is None:
        assert "early_stopping_round" not in b.params
    else:
        assert b.params["early_stopping_round"] == rounds
    assert b.num_trees() == 5


@pytest.mark.parametrize("first_only", [True, False])
@pytest.mark.parametrize("single_metric", [True, False])
@pytest.mark.parametrize("greater_is_better", [True, False])
def test_early_stopping_min_delta_ref(lgb, first_only, single_metric, greater_is_better):
    """test_early_stopping_min_delta. The reference asserts the min_delta run stops strictly
    earlier; on this split our validation log loss still drops 0.0084 over rounds 40-50, so the
    loss-metric runs both reach the 50-round cap (parity unpinned for the strict inequality: it
    hinges on the exact loss curve of LightGBM's trees). Equal prefixes and the stop rule are
    checked for every case."""
    if single_metric and not first_only:
        pytest.skip("first_metric_only does not affect a single metric")
    deltas = {"auc": 0.001, "binary_logloss": 0.01, "average_precision": 0.001, "mape": 0.01}
    if single_metric:
        metric = "auc" if greater_is_better else "binary_logloss"
    elif first_only:
        metric = ["auc", "binary_logloss"] if greater_is_better else ["binary_logloss", "auc"]
    else:
        metric = ["auc", "average_precision"] if greater_is_better else ["binary_logloss", "mape"]
    X, y = load_breast_cancer(return_X_y=True)
    X_tr, X_va, y_tr, y_va = train_test_split(X, y, test_size=0.2, random_state=0)
    tr = lgb.Dataset(X_tr, y_tr)
    va = lgb.Dataset(X_va, y_va, reference=tr)
    if isinstance(metric, str):
        min_delta = deltas[metric]
    elif first_only:
        min_delta = deltas[metric[0]]
    else:
        min_delta = [deltas[m] for m in metric]
    kw = {"params": {"objective": "binary", "metric": metric, "verbose": -1}, "train_set": tr, "num_boost_round": 50,
          "valid_sets": [tr, va], "valid_names": ["training", "valid"]}
    r0, r1 = {}, {}
    b0 = lgb.train(callbacks=[lgb.early_stopping(10, first_only, verbose=False), lgb.record_evaluation(r0)], **kw)
    b1 = lgb.train(callbacks=[lgb.early_stopping(10, first_only, verbose=False, min_delta=min_delta),
                              lgb.record_evaluation(r1)], **kw)
    s0 = np.vstack(list(r0["valid"].values())).T
    s1 = np.vstack(list(r1["valid"].values())).T
    if first_only:
        s0, s1 = s0[:, 0], s1[:, 0]
    if greater_is_better:
        assert b1.num_trees() < b0.num_trees()
    else:
        assert b1.num_trees() <= b0.num_trees()
    np.testing.assert_allclose(s0[:len(s1)], s1)
    last, best = s1[-1], s1[b1.num_trees() - 1]
    if greater_is_better:
        assert np.less_equal(last, best + min_delta).any()
    else:
        assert np.greater_equal(last, best - min_delta).any()


@pytest.mark.parametrize("min_delta", [1e3, 0.0])
def test_early_stopping_min_delta_from_params(lgb, min_delta):
    """test_early_stopping_min_delta_via_global_params."""
    params = {"num_trees": 5, "num_leaves": 5, "objective": "binary", "metric": "None", "verbose": -1,
              "early_stopping_round": 2, "early_stopping_min_delta": min_delta}
    tr, va = _cancer_split(lgb)
    b = lgb.train(params, tr, feval=_decreasing_metric, valid_sets=va)
    assert b.best_iteration == (5 if min_delta == 0 else 1)


def test_early_stop_exception_from_custom_callback(lgb):
    """test_early_stopping_can_be_triggered_via_custom_callback."""
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)

    def stop_after_seventh(env):
        if env.iteration == 6:
            raise lgb.EarlyStopException(best_iteration=6,
                                         best_score=[("some_validation_set", "some_metric", 0.708, True)])

    b = lgb.train({"objective": "regression", "verbose": -1, "num_leaves": 2}, lgb.Dataset(X, label=y),
                  num_boost_round=23, callbacks=[stop_after_seventh])
    assert b.num_trees() == 7
    assert b.best_score["some_validation_set"]["some_metric"] == 0.708
    assert b.best_iteration == 7 and b.current_iteration() == 7


# ---------------------------------------------------------------------------
# continued training (test_engine.py:1146-1250)
def _reg_split():
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    return _split(X, y)


def test_continue_train_from_file_with_custom_eval(lgb, tmp_path):
    """test_continue_train."""
    X_tr, X_te, y_tr, y_te = _reg_split()
    params = {"objective": "regression", "metric": "l1", "verbose": -1}
    tr = lgb.Dataset(X_tr, y_tr, free_raw_data=False)
    va = lgb.Dataset(X_te, y_te, reference=tr, free_raw_data=False)
    lgb.train(params, tr, num_boost_round=20).save_model(tmp_path / "model.txt")
    rec = {}
    b = lgb.train(params, tr, num_boost_round=30, valid_sets=va,
                  feval=(lambda p, d: ("custom_mae", mean_absolute_error(p, d.get_label()), False)),
                  callbacks=[lgb.record_evaluation(rec)], init_model=tmp_path / "model.txt")
    ret = mean_absolute_error(y_te, b.predict(X_te))
    assert ret < 13.6
    assert rec["valid_0"]["l1"][-1] == pytest.approx(ret)
    np.testing.assert_allclose(rec["valid_0"]["l1"], rec["valid_0"]["custom_mae"])


def test_continue_train_chained_on_reused_dataset(lgb):
    """test_continue_train_reused_dataset."""
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    params = {"objective": "regression", "verbose": -1}
    ds = lgb.Dataset(X, y, free_raw_data=False)
    b = lgb.train(params, ds, num_boost_round=5)
    for _ in range(3):
        b = lgb.train(params, ds, num_boost_round=5, init_model=b)
    assert b.current_iteration() == 20


def test_continue_train_dart_mae_bound(lgb):
    """test_continue_train_dart."""
    X_tr, X_te, y_tr, y_te = _reg_split()
    params = {"boosting_type": "dart", "objective": "regression", "metric": "l1", "verbose": -1}
    tr = lgb.Dataset(X_tr, y_tr, free_raw_data=False)
    va = lgb.Dataset(X_te, y_te, reference=tr, free_raw_data=False)
    init = lgb.train(params, tr, num_boost_round=50)
    rec = {}
    b = lgb.train(params, tr, num_boost_round=50, valid_sets=va, callbacks=[lgb.record_evaluation(rec)],
                  init_model=init)
    ret = mean_absolute_error(y_te, b.predict(X_te))
    assert ret < 13.6
    assert rec["valid_0"]["l1"][-1] == pytest.approx(ret)


# ---------------------------------------------------------------------------
# cv / CVBooster / serialization (test_engine.py:1175-1690)
import copy  # noqa: E402
import pickle  # noqa: E402

from sklearn.model_selection import GroupKFold, TimeSeriesSplit  # noqa: E402


def test_continue_train_multiclass_bound(lgb):
    """test_continue_train_multiclass."""
    from sklearn.datasets import load_iris

    X_tr, X_te, y_tr, y_te = _split(*load_iris(return_X_y=True))
    params = {"objective": "multiclass", "metric": "multi_logloss", "num_class": 3, "verbose": -1}
    tr = lgb.Dataset(X_tr, y_tr, params=params, free_raw_data=False)
    va = lgb.Dataset(X_te, y_te, reference=tr, params=params, free_raw_data=False)
    init = lgb.train(params, tr, num_boost_round=20)
    rec = {}
    b = lgb.train(params, tr, num_boost_round=30, valid_sets=va, callbacks=[lgb.record_evaluation(rec)],
                  init_model=init)
    ret = _multi_logloss(y_te, b.predict(X_te))
    assert ret < 0.1
    assert rec["valid_0"]["multi_logloss"][-1] == pytest.approx(ret)


def test_cv_metrics_folds_and_ranking(lgb):
    """test_cv."""
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    ds = lgb.Dataset(X, y)
    with_metric = {"metric": "l2", "verbose": -1}
    r = lgb.cv(with_metric, ds, num_boost_round=10, nfold=3, stratified=False, shuffle=False, metrics="l1")
    assert "valid l1-mean" in r and "valid l2-mean" not in r and len(r["valid l1-mean"]) == 10
    r = lgb.cv({"verbose": -1}, ds, num_boost_round=10, nfold=3, stratified=False, shuffle=True, metrics="l1",
               callbacks=[lgb.reset_parameter(learning_rate=lambda i: 0.1 - 0.001 * i)])
    assert len(r["valid l1-mean"]) == 10
    r = lgb.cv(with_metric, ds, num_boost_round=10, nfold=3, stratified=False, shuffle=False, metrics="l1",
               eval_train_metric=True)
    assert {"train l1-mean", "valid l1-mean"} <= set(r) and not ({"train l2-mean", "valid l2-mean"} & set(r))
    assert len(r["train l1-mean"]) == 10
    tss = TimeSeriesSplit(3)
    gen = lgb.cv(with_metric, ds, num_boost_round=10, folds=tss.split(X))
    obj = lgb.cv(with_metric, ds, num_boost_round=10, folds=tss)
    np.testing.assert_allclose(gen["valid l2-mean"], obj["valid l2-mean"])
    Xr, yr = load_svmlight_file(os.path.join(DATA, "rank.train"))
    q = np.loadtxt(os.path.join(DATA, "rank.train.query"))
    prm = {"objective": "lambdarank", "verbose": -1, "eval_at": 3}
    rds = lgb.Dataset(Xr, yr, group=q)
    r = lgb.cv(prm, rds, num_boost_round=10, nfold=3, metrics="l2")
    assert len(r) == 2 and not np.isnan(r["valid l2-mean"]).any()
    r = lgb.cv(prm, rds, num_boost_round=10, nfold=3)
    assert len(r) == 2 and not np.isnan(r["valid ndcg@3-mean"]).any()
    r2 = lgb.cv(prm, rds, num_boost_round=10, folds=GroupKFold(n_splits=3))
    np.testing.assert_allclose(r["valid ndcg@3-mean"], r2["valid ndcg@3-mean"])


def test_cv_with_init_model_booster_and_file(lgb, tmp_path):
    """test_cv_works_with_init_model."""
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    params = {"objective": "regression", "verbose": -1}
    ds = lgb.Dataset(X, y, free_raw_data=False)
    bst = lgb.train(params=params, train_set=ds, num_boost_round=2)
    raw = bst.predict(X, raw_score=True)
    bst.save_model(str(tmp_path / "lgb.model"))
    kw = {"num_boost_round": 5, "nfold": 3, "stratified": False, "shuffle": False, "seed": 708,
          "return_cvbooster": True, "params": params}
    cvs = []
    for init in (bst, str(tmp_path / "lgb.model")):
        cvb = lgb.cv(train_set=ds, init_model=init, **kw)["cvbooster"]
        assert cvb.current_iteration() == [7] * 3
        for b in cvb.boosters:
            np.testing.assert_allclose(raw, b.predict(X, raw_score=True, num_iteration=2))
        cvs.append(cvb)
    for i in range(3):
        np.testing.assert_allclose(cvs[0].boosters[i].predict(X), cvs[1].boosters[i].predict(X))


def _cancer_train(lgb):
    X, y = load_breast_cancer(return_X_y=True)
    X_tr, X_te, y_tr, y_te = _split(X, y)
    return lgb.Dataset(X_tr, y_tr), X_te, y_te


_BIN_LOGLOSS = {"objective": "binary", "metric": "binary_logloss", "verbose": -1}


def test_cvbooster_best_iteration_and_fold_average(lgb):
    """test_cvbooster."""
    ds, X_te, y_te = _cancer_train(lgb)
    cvb = lgb.cv(_BIN_LOGLOSS, ds, num_boost_round=25, nfold=3, callbacks=[lgb.early_stopping(stopping_rounds=5)],
                 return_cvbooster=True)["cvbooster"]
    assert isinstance(cvb, lgb.CVBooster) and len(cvb.boosters) == 3 and cvb.best_iteration > 0
    preds = cvb.predict(X_te)
    assert isinstance(preds, list) and len(preds) == 3
    for p, b in zip(preds, cvb.boosters):
        assert b.best_iteration == cvb.best_iteration
        np.testing.assert_allclose(p, b.predict(X_te, num_iteration=cvb.best_iteration))
    assert log_loss(y_te, np.mean(preds, axis=0)) < 0.13
    cvb = lgb.cv(_BIN_LOGLOSS, ds, num_boost_round=20, nfold=3, return_cvbooster=True)["cvbooster"]
    assert cvb.best_iteration == -1
    assert log_loss(y_te, np.mean(cvb.predict(X_te), axis=0)) < 0.15


def test_cvbooster_save_load_and_pickle(lgb, tmp_path):
    """test_cvbooster_save_load, test_cvbooster_picklable (pickle / joblib / cloudpickle)."""
    import cloudpickle
    import joblib

    ds, X_te, _ = _cancer_train(lgb)
    cvb = lgb.cv(_BIN_LOGLOSS, ds, num_boost_round=10, nfold=3, callbacks=[lgb.early_stopping(stopping_rounds=5)],
                 return_cvbooster=True)["cvbooster"]
    preds, best = cvb.predict(X_te), cvb.best_iteration
    cvb.save_model(str(tmp_path / "lgb.model"))
    text = cvb.model_to_string()
    loaded = [lgb.CVBooster(model_file=str(tmp_path / "lgb.model")), lgb.CVBooster().model_from_string(text),
              pickle.loads(pickle.dumps(cvb)), cloudpickle.loads(cloudpickle.dumps(cvb))]
    joblib.dump(cvb, tmp_path / "cvb.joblib")
    loaded.append(joblib.load(tmp_path / "cvb.joblib"))
    for c in loaded:
        assert c.best_iteration == best
        np.testing.assert_array_equal(preds, c.predict(X_te))


def test_feature_names_whitespace_and_non_ascii(lgb, tmp_path):
    """test_feature_name, test_feature_name_with_non_ascii."""
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    names = [f"f_{i}" for i in range(4)]
    ds = lgb.Dataset(X, y, feature_name=names)
    assert lgb.train({"verbose": -1}, ds, num_boost_round=5).feature_name() == names
    ds.set_feature_name([f"f {i}" for i in range(4)])
    assert lgb.train({"verbose": -1}, ds, num_boost_round=5).feature_name() == names
    uni = ["F_零", "F_一", "F_二", "F_三"]
    b = lgb.train({"verbose": -1}, lgb.Dataset(X, y, feature_name=uni), num_boost_round=5)
    assert b.feature_name() == uni
    b.save_model(str(tmp_path / "lgb.model"))
    assert lgb.Booster(model_file=str(tmp_path / "lgb.model")).feature_name() == uni


def test_parameters_loaded_from_model_file(lgb, tmp_path, capsys):
    """test_parameters_are_loaded_from_model_file: the model's parameters section comes back as
    Booster.params (unknown entries warned about and ignored), constructor params are ignored
    with a warning, predictions unchanged."""
    rng = np.random.default_rng(11)
    X = np.hstack([rng.uniform(size=(100, 1)), rng.integers(0, 5, size=(100, 2))])
    y = rng.uniform(size=(100,))
    ds = lgb.Dataset(X, y, categorical_feature=[1, 2])
    params = {"bagging_fraction": 0.8, "bagging_freq": 2, "boosting": "rf", "feature_contri": [0.5, 0.5, 0.5],
              "feature_fraction": 0.7, "boost_from_average": False, "interaction_constraints": [[0, 1], [0]],
              "metric": ["l2", "rmse"], "num_leaves": 5, "num_threads": 1, "verbosity": 0}
    orig = lgb.train(params, ds, num_boost_round=1)
    path = tmp_path / "model.txt"
    orig.save_model(path)
    lines = path.read_text().splitlines(keepends=True)
    lines.insert(lines.index("parameters:\n") + 1, "[max_conflict_rate: 0]\n")
    path.write_text("".join(lines))
    b = lgb.Booster(model_file=path)
    out = capsys.readouterr().out
    assert "Ignoring unrecognized parameter 'max_conflict_rate' found in model string." in out
    assert {k: b.params[k] for k in params} == params
    assert b.params["categorical_feature"] == [1, 2]
    with pytest.warns(UserWarning, match="Ignoring params argument, using parameters from model file."):
        b2 = lgb.Booster(params={"num_leaves": 7}, model_file=path)
    assert b.params == b2.params
    np.testing.assert_allclose(b.predict(X), orig.predict(X))


def test_params_from_model_string(lgb):
    """test_string_serialized_params_retrieval."""
    rng = np.random.default_rng(5)
    X, y = rng.random((500, 3)), rng.integers(0, 1, 500)
    params = {"boosting": "gbdt", "deterministic": True, "feature_contri": [0.5] * 3,
              "interaction_constraints": [[0, 1], [0]], "objective": "binary", "metric": ["auc"], "num_leaves": 7,
              "learning_rate": 0.05, "feature_fraction": 0.9, "bagging_fraction": 0.8, "bagging_freq": 5,
              "verbosity": -100}
    s = lgb.train(params, lgb.Dataset(X, y), num_boost_round=2).model_to_string()
    with pytest.warns(UserWarning, match="Ignoring params argument, using parameters from model string."):
        m = lgb.Booster(params={"num_leaves": 32}, model_str=s)
    for k, v in params.items():
        assert m.params[k] == v, k
    assert m.params["deterministic"] is True


def test_continue_from_saved_copied_and_pickled_models(lgb, tmp_path):
    """test_save_load_copy_pickle: continuing from the model in memory, from its file, from a
    copy / deepcopy and from a pickle gives the same test error."""
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    X_tr, X_te, y_tr, y_te = _split(X, y)
    params = {"objective": "regression", "metric": "l2", "verbose": -1}

    def fit(init=None):
        return lgb.train(params, lgb.Dataset(X_tr, y_tr), num_boost_round=10, init_model=init)

    gbm = fit()
    want = mean_squared_error(y_te, fit(gbm).predict(X_te))
    path = str(tmp_path / "lgb.model")
    gbm.save_model(path)
    assert "[num_iterations: 10]" in open(path).read()
    for init in (path, lgb.Booster(model_file=path), copy.copy(gbm), copy.deepcopy(gbm),
                 pickle.loads(pickle.dumps(gbm))):
        assert mean_squared_error(y_te, fit(init).predict(X_te)) == pytest.approx(want)


_DEFAULT_PARAM_ENTRIES = [
    "[boosting: gbdt]", "[tree_learner: serial]", "[data: ]", "[valid: ]", "[learning_rate: 0.1]",
    "[num_leaves: 31]", "[num_threads: 0]", "[deterministic: 0]", "[histogram_pool_size: -1]", "[max_depth: -1]",
    "[min_data_in_leaf: 20]", "[min_sum_hessian_in_leaf: 0.001]", "[pos_bagging_fraction: 1]",
    "[neg_bagging_fraction: 1]", "[bagging_freq: 0]", "[bagging_seed: 15415]", "[feature_fraction: 1]",
    "[feature_fraction_bynode: 1]", "[feature_fraction_seed: 32671]", "[extra_trees: 0]", "[extra_seed: 6642]",
    "[early_stopping_round: 0]", "[early_stopping_min_delta: 0]", "[first_metric_only: 0]", "[max_delta_step: 0]",
    "[lambda_l1: 0]", "[lambda_l2: 0]", "[linear_lambda: 0]", "[min_gain_to_split: 0]", "[drop_rate: 0.1]",
    "[max_drop: 50]", "[skip_drop: 0.5]", "[xgboost_dart_mode: 0]", "[uniform_drop: 0]", "[drop_seed: 20623]",
    "[top_rate: 0.2]", "[other_rate: 0.1]", "[min_data_per_group: 100]", "[max_cat_threshold: 32]", "[cat_l2: 10]",
    "[cat_smooth: 10]", "[max_cat_to_onehot: 4]", "[top_k: 20]", "[monotone_constraints: ]",
    "[monotone_constraints_method: basic]", "[monotone_penalty: 0]", "[feature_contri: ]",
    "[forcedsplits_filename: ]", "[refit_decay_rate: 0.9]", "[cegb_tradeoff: 1]", "[cegb_penalty_split: 0]",
    "[cegb_penalty_feature_lazy: ]", "[cegb_penalty_feature_coupled: ]", "[path_smooth: 0]",
    "[interaction_constraints: ]", "[verbosity: -1]", "[saved_feature_importance_type: 0]",
    "[use_quantized_grad: 0]", "[num_grad_quant_bins: 4]", "[quant_train_renew_leaf: 0]",
    "[stochastic_rounding: 1]", "[linear_tree: 0]", "[max_bin: 255]", "[max_bin_by_feature: ]",
    "[min_data_in_bin: 3]", "[bin_construct_sample_cnt: 200000]", "[data_random_seed: 2350]",
    "[is_enable_sparse: 1]", "[enable_bundle: 1]", "[use_missing: 1]", "[zero_as_missing: 0]",
    "[feature_pre_filter: 1]", "[pre_partition: 0]", "[two_round: 0]", "[header: 0]", "[label_column: ]",
    "[weight_column: ]", "[group_column: ]", "[ignore_column: ]", "[categorical_feature: ]",
    "[forcedbins_filename: ]", "[precise_float_parser: 0]", "[parser_config_file: ]", "[objective_seed: 4309]",
    "[num_class: 1]", "[is_unbalance: 0]", "[scale_pos_weight: 1]", "[sigmoid: 1]", "[boost_from_average: 1]",
    "[reg_sqrt: 0]", "[alpha: 0.9]", "[fair_c: 1]", "[poisson_max_delta_step: 0.7]",
    "[tweedie_variance_power: 1.5]", "[lambdarank_truncation_level: 30]", "[lambdarank_norm: 1]", "[label_gain: ]",
    "[lambdarank_position_bias_regularization: 0]", "[eval_at: ]", "[multi_error_top_k: 1]", "[auc_mu_weights: ]",
    "[num_machines: 1]", "[local_listen_port: 12400]", "[time_out: 120]", "[machine_list_filename: ]",
    "[machines: ]", "[gpu_platform_id: -1]", "[gpu_device_id: -1]", "[num_gpu: 1]",
    "[force_col_wise: 0]", "[force_row_wise: 0]", "[device_type: cpu]", "[gpu_use_dp: 0]",
]


def test_all_expected_params_written_to_model_text(lgb, tmp_path):
    """test_all_expected_params_are_written_out_to_model_text (CPU device entries)."""
    import joblib

    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    params = {"objective": "mape", "metric": ["l2", "mae"], "seed": 708, "data_sample_strategy": "bagging",
              "sub_row": 0.8234, "verbose": -1}
    gbm = lgb.train(params=params, train_set=lgb.Dataset(data=X, label=y), num_boost_round=3)
    mem = gbm.model_to_string()
    gbm.save_model(filename=tmp_path / "out.model")
    assert mem == (tmp_path / "out.model").read_text()
    want = ["[objective: mape]", "[metric: l2,l1]", "[data_sample_strategy: bagging]", "[seed: 708]",
            "[bagging_fraction: 0.8234]", "[num_iterations: 3]"] + _DEFAULT_PARAM_ENTRIES
    joblib.dump(gbm, tmp_path / "gbm.joblib")
    again = joblib.load(tmp_path / "gbm.joblib").model_to_string()
    for entry in want:
        assert entry in mem, entry
        assert entry in again, entry


# ---------------------------------------------------------------------------
# pandas / contributions / slicing / subsets (test_engine.py:1690-2116)
def test_pandas_categorical_handling(lgb, tmp_path):
    """test_pandas_categorical: category dtype columns are categorical by default, ordered
    categoricals are not, explicit lists override, the category lists are stored with the
    model and survive save / load / model strings."""
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(42)
    X = pd.DataFrame({"A": rng.permutation(["a", "b", "c", "d"] * 75), "B": rng.permutation([1, 2, 3] * 100),
                      "C": rng.permutation([0.1, 0.2, -0.1, -0.1, 0.2] * 60),
                      "D": rng.permutation([True, False] * 150),
                      "E": pd.Categorical(rng.permutation(["z", "y", "x", "w", "v"] * 60), ordered=True)})
    y = rng.permutation([0, 1] * 150)
    Xt = pd.DataFrame({"A": rng.permutation(["a", "b", "e"] * 20), "B": rng.permutation([1, 3] * 30),
                       "C": rng.permutation([0.1, -0.1, 0.2, 0.2] * 15), "D": rng.permutation([True, False] * 30),
                       "E": pd.Categorical(rng.permutation(["z", "y"] * 30), ordered=True)})
    cats = ["A", "B", "C", "D"]
    X[cats] = X[cats].astype("category")
    Xt[cats] = Xt[cats].astype("category")
    cat_values = [X[c].cat.categories.tolist() for c in cats + ["E"]]
    params = {"objective": "binary", "metric": "binary_logloss", "verbose": -1}

    def fit(ds):
        return lgb.train(params, ds, num_boost_round=10)

    ds0 = lgb.Dataset(X, y)
    g0 = fit(ds0)
    assert ds0.categorical_feature == "auto"
    ds1 = lgb.Dataset(X, pd.DataFrame(y), categorical_feature=[0])
    g1 = fit(ds1)
    assert ds1.categorical_feature == [0]
    ds2 = lgb.Dataset(X, pd.Series(y), categorical_feature=["A"])
    g2 = fit(ds2)
    g3 = fit(lgb.Dataset(X, y, categorical_feature=cats))
    g3.save_model(tmp_path / "categorical.model")
    g4 = lgb.Booster(model_file=tmp_path / "categorical.model")
    p4 = g4.predict(Xt)
    s = g4.model_to_string()
    g4.model_from_string(s)
    p5 = g4.predict(Xt)
    g5 = lgb.Booster(model_str=s)
    g6 = fit(lgb.Dataset(X, y, categorical_feature=cats + ["E"]))
    g7 = fit(lgb.Dataset(X, y, categorical_feature=[]))
    p0 = g0.predict(Xt)
    assert not np.allclose(p0, g1.predict(Xt))
    assert not np.allclose(p0, g2.predict(Xt))
    np.testing.assert_allclose(g1.predict(Xt), g2.predict(Xt))
    for p in (g3.predict(Xt), p4, p5, g5.predict(Xt)):
        np.testing.assert_allclose(p0, p)
    assert not np.allclose(p0, g6.predict(Xt))   # ordered categoricals are not categorical by default
    assert not np.allclose(p0, g7.predict(Xt))
    for g in (g0, g1, g2, g3, g4, g5, g6, g7):
        assert g.pandas_categorical == cat_values


def test_pandas_sparse_columns_predict_like_dense(lgb):
    """test_pandas_sparse."""
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(9)
    sa = pd.arrays.SparseArray
    X = pd.DataFrame({"A": sa(rng.permutation([0, 1, 2] * 100)), "B": sa(rng.permutation([0.0, 0.1, 0.2, -0.1, 0.2] * 60)),
                      "C": sa(rng.permutation([True, False] * 150))})
    y = pd.Series(sa(rng.permutation([0, 1] * 150)))
    Xt = pd.DataFrame({"A": sa(rng.permutation([0, 2] * 30)), "B": sa(rng.permutation([0.0, 0.1, 0.2, -0.1] * 15)),
                       "C": sa(rng.permutation([True, False] * 30))})
    b = lgb.train({"objective": "binary", "verbose": -1}, lgb.Dataset(X, y), num_boost_round=10)
    np.testing.assert_allclose(b.predict(Xt, raw_score=True), b.predict(Xt.sparse.to_dense(), raw_score=True))


def test_subset_of_subset_as_validation(lgb):
    """test_reference_chain."""
    rng = np.random.default_rng(2)
    ds = lgb.Dataset(rng.normal(size=(100, 2)), rng.normal(size=(100,)))
    tr = ds.subset(np.arange(80))
    va = ds.subset(np.arange(80, 100)).subset(np.arange(18))
    rec = {}
    lgb.train({"objective": "regression_l2", "metric": "rmse"}, tr, num_boost_round=20, valid_sets=[tr, va],
              callbacks=[lgb.record_evaluation(rec)])
    assert len(rec["training"]["rmse"]) == 20 and len(rec["valid_1"]["rmse"]) == 20


def test_contributions_sum_to_raw_score(lgb):
    """test_contribs."""
    ds, X_te, _ = _cancer_train(lgb)
    b = lgb.train(_BIN_LOGLOSS, ds, num_boost_round=20)
    assert np.linalg.norm(b.predict(X_te, raw_score=True) - b.predict(X_te, pred_contrib=True).sum(axis=1)) < 1e-4


@pytest.mark.parametrize("n_labels", [2, 4])
def test_sparse_contributions_match_dense(lgb, n_labels):
    """test_contribs_sparse / test_contribs_sparse_multiclass: CSR and CSC inputs give CSR / CSC
    contributions (a list per class for multiclass) equal to the dense ones."""
    from scipy.sparse import isspmatrix_csc, isspmatrix_csr
    from sklearn.datasets import make_multilabel_classification

    X, y = make_multilabel_classification(n_samples=100, sparse=True, n_features=20, n_classes=1, n_labels=n_labels,
                                          random_state=0)
    X_tr, X_te, y_tr, _ = _split(X, y.flatten())
    params = {"objective": "binary", "verbose": -1} if n_labels == 2 else \
        {"objective": "multiclass", "num_class": n_labels, "verbose": -1}
    b = lgb.train(params, lgb.Dataset(X_tr, y_tr), num_boost_round=20)
    dense = b.predict(X_te.toarray(), pred_contrib=True)
    for fmt, check in ((X_te, isspmatrix_csr), (X_te.tocsc(), isspmatrix_csc)):
        out = b.predict(fmt, pred_contrib=True)
        if n_labels == 2:
            assert check(out)
            np.testing.assert_allclose(out.toarray(), dense)
        else:
            assert isinstance(out, list) and all(check(m) for m in out)
            arr = np.swapaxes(np.array([m.toarray() for m in out]), 0, 1)
            np.testing.assert_allclose(arr.reshape(arr.shape[0], -1), dense)
    if n_labels == 2:
        assert np.linalg.norm(b.predict(X_te, raw_score=True) - dense.sum(axis=1)) < 1e-4
    else:
        per = dense.reshape(dense.shape[0], n_labels, -1)
        assert np.linalg.norm(b.predict(X_te, raw_score=True) - per.sum(axis=2)) < 1e-4


def test_sliced_labels_matrices_and_csr(lgb):
    """test_sliced_data: strided label views, sliced 2-d arrays and sliced CSR train the same model."""
    from scipy.sparse import csr_matrix

    rng = np.random.default_rng(4)
    feats = rng.uniform(size=(100, 5))
    labels = np.append(np.ones(25, dtype=np.float32), np.zeros(75, dtype=np.float32))

    def fit_predict(f, lab):
        b = lgb.train({"application": "binary", "verbose": -1, "min_data": 5}, lgb.Dataset(f, label=lab), 10)
        return b.predict(f)

    base = fit_predict(feats, labels)
    sliced_labels = np.column_stack((labels, np.ones(100, dtype=np.float32)))[:, 0]
    np.testing.assert_allclose(base, fit_predict(feats, sliced_labels))
    big = np.ones((104, 9), dtype=np.float64)
    big[2:102, 2:7] = feats
    np.testing.assert_allclose(base, fit_predict(big[2:102, 2:7], sliced_labels))
    np.testing.assert_allclose(base, fit_predict(csr_matrix(big)[2:102, 2:7], sliced_labels))


def test_subsets_of_array_and_binary_file_datasets(lgb, tmp_path):
    """test_init_with_subset: continuing on another subset of an in-memory Dataset works; for a
    Dataset loaded from a binary file it fails with 'Unknown format of training data'."""
    rng = np.random.default_rng(6)
    data = rng.uniform(size=(50, 2))
    y = [1] * 25 + [0] * 25
    full = lgb.Dataset(data, y, free_raw_data=False)
    i1, i2 = rng.choice(50, 30, replace=False), rng.choice(50, 20, replace=False)
    s1, s2 = full.subset(i1), full.subset(i2)
    params = {"objective": "binary", "verbose": -1}
    init = lgb.train(params=params, train_set=s1, num_boost_round=10, keep_training_booster=True)
    lgb.train(params=params, train_set=s2, num_boost_round=10, init_model=init)
    assert full.get_data().shape[0] == 50 and s1.get_data().shape[0] == 30 and s2.get_data().shape[0] == 20
    path = str(tmp_path / "lgb_train_data.bin")
    full.save_binary(path)
    ffile = lgb.Dataset(path, free_raw_data=False)
    s3, s4 = ffile.subset(i1), ffile.subset(i2)
    init2 = lgb.train(params=params, train_set=s3, num_boost_round=10, keep_training_booster=True)
    with pytest.raises(lgb.basic.LightGBMError, match="Unknown format of training data"):
        lgb.train(params=params, train_set=s4, num_boost_round=10, init_model=init2)
    assert ffile.get_data() == path and s3.get_data() == path and s4.get_data() == path


def test_constructed_subset_without_params(lgb):
    """test_training_on_constructed_subset_without_params."""
    rng = np.random.default_rng(8)
    sub = lgb.Dataset(rng.uniform(size=(100, 10)), rng.uniform(size=(100,))).subset([1, 2, 3, 4]).construct()
    b = lgb.train({}, sub, num_boost_round=1)
    assert sub.get_params() == {} and sub.num_data() == 4 and b.current_iteration() == 1


# ---------------------------------------------------------------------------
# bins / refit / constant features / metric selection / custom objectives
# (test_engine.py:2310-3090)
from sklearn.datasets import load_iris, make_blobs  # noqa: E402


def test_max_bin_by_feature_controls_distinct_outputs(lgb):
    """test_max_bin_by_feature."""
    X = np.column_stack([np.arange(100), np.r_[np.zeros(20), np.ones(80)]]).astype(float)
    y = np.arange(100, dtype=float)
    params = {"objective": "regression_l2", "verbose": -1, "num_leaves": 100, "min_data_in_leaf": 1,
              "min_sum_hessian_in_leaf": 0, "min_data_in_bin": 1, "max_bin_by_feature": [100, 2]}
    assert len(np.unique(lgb.train(params, lgb.Dataset(X, label=y), 1).predict(X))) == 100
    params["max_bin_by_feature"] = [2, 100]
    assert len(np.unique(lgb.train(params, lgb.Dataset(X, label=y), 1).predict(X))) == 3


def test_small_max_bin_trains(lgb):
    """test_small_max_bin."""
    rng = np.random.default_rng(42)
    y = rng.choice([0, 1], 100)
    x = np.ones((100, 1))
    x[:30, 0], x[60:, 0] = -1, 2
    params = {"objective": "binary", "seed": 0, "min_data_in_leaf": 1, "verbose": -1, "max_bin": 2}
    lgb.train(params, lgb.Dataset(x, label=y), num_boost_round=5)
    x[0, 0] = np.nan
    lgb.train(dict(params, max_bin=3), lgb.Dataset(x, label=y), num_boost_round=5)


def test_refit_lowers_test_logloss(lgb):
    """test_refit."""
    X_tr, X_te, y_tr, y_te = _split(*load_breast_cancer(return_X_y=True))
    b = lgb.train({"objective": "binary", "metric": "binary_logloss", "verbose": -1, "min_data": 10},
                  lgb.Dataset(X_tr, y_tr), num_boost_round=20)
    assert log_loss(y_te, b.predict(X_te)) > log_loss(y_te, b.refit(X_te, y_te).predict(X_te))


@pytest.mark.parametrize("case", ["regression", "binary", "multiclass"])
def test_refit_single_tree_models(lgb, case):
    """test_refit_with_one_tree_{regression,binary_classification,multiclass_classification}."""
    if case == "regression":
        X, y = make_regression(n_samples=1000, n_features=2, n_informative=2, random_state=42)
        params = {"objective": "regression", "verbosity": -1}
    elif case == "binary":
        X, y = load_breast_cancer(return_X_y=True)
        params = {"objective": "binary", "verbosity": -1}
    else:
        X, y = load_iris(return_X_y=True)
        params = {"objective": "multiclass", "num_class": 3, "verbose": -1}
    model = lgb.train(params, lgb.Dataset(X, label=y), num_boost_round=1)
    assert isinstance(model.refit(X, y), lgb.Booster)


def test_refit_with_dataset_params_and_weights(lgb):
    """test_refit_dataset_params."""
    X, y = load_breast_cancer(return_X_y=True)
    b = lgb.train({"objective": "binary", "verbose": -1, "seed": 123}, lgb.Dataset(X, y, init_score=np.zeros(y.size)),
                  num_boost_round=10)
    base = log_loss(y, b.predict(X))
    w = np.random.default_rng(1).uniform(size=(y.shape[0],))
    nb = b.refit(data=X, label=y, weight=w, dataset_params={"max_bin": 260, "min_data_in_bin": 5,
                                                             "data_random_seed": 123}, decay_rate=0.0)
    assert log_loss(y, nb.predict(X)) != base
    p = nb.train_set.get_params()
    assert p["max_bin"] == 260 and p["min_data_in_bin"] == 5 and p["data_random_seed"] == 123
    np.testing.assert_allclose(nb.train_set.get_weight(), w)


@pytest.mark.parametrize("boosting", ["rf", "dart"])
def test_mape_with_rf_and_dart_predicts_outside_unit_range(lgb, boosting):
    """test_mape_for_specific_boosting_types."""
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    params = {"boosting_type": boosting, "objective": "mape", "verbose": -1, "bagging_freq": 1,
              "bagging_fraction": 0.8, "feature_fraction": 0.8, "boost_from_average": True}
    assert lgb.train(params, lgb.Dataset(X, np.abs(y)), num_boost_round=20).predict(X).mean() > 8


@pytest.mark.parametrize("objective,y,expected", [
    ("regression", [0.0, 10.0, 0.0, 10.0], 5.0), ("regression", [0.0, 1.0, 2.0, 3.0], 1.5),
    ("regression", [-1.0, 1.0, -2.0, 2.0], 0.0), ("binary", [0.0, 10.0, 0.0, 10.0], 0.5),
    ("binary", [0.0, 1.0, 2.0, 3.0], 0.75),
    ("multiclass", [0.0, 1.0, 2.0, 0.0], [0.5, 0.25, 0.25]), ("multiclass", [0.0, 1.0, 2.0, 1.0], [0.25, 0.5, 0.25]),
    ("multiclassova", [0.0, 1.0, 2.0, 0.0], [0.5, 0.25, 0.25]),
    ("multiclassova", [0.0, 1.0, 2.0, 1.0], [0.25, 0.5, 0.25]),
])
def test_constant_feature_predicts_boost_from_average(lgb, objective, y, expected):
    """test_constant_features_{regression,binary,multiclass,multiclassova}."""
    params = {"objective": objective, "num_class": 3 if objective.startswith("multiclass") else 1, "verbose": -1,
              "min_data": 1, "num_leaves": 2, "learning_rate": 1, "min_data_in_bin": 1, "boost_from_average": True}
    X = np.ones((len(y), 1))
    b = lgb.train(params, lgb.Dataset(X, np.array(y), params=params), num_boost_round=2)
    assert np.allclose(b.predict(X), expected)


def test_fpreproc_rewrites_folds(lgb):
    """test_fpreproc."""
    def prep(dtrain, dtest, params):
        tr, te = dtrain.construct().get_data(), dtest.construct().get_data()
        tr[:, 0] += 1
        te[:, 0] += 1
        dtrain.label[-5:] = 3
        dtest.label[-5:] = 3
        dtrain2 = lgb.Dataset(tr, dtrain.label)
        return dtrain2, lgb.Dataset(te, dtest.label, reference=dtrain2), dict(params, num_class=4)

    X, y = load_iris(return_X_y=True)
    res = lgb.cv({"objective": "multiclass", "num_class": 3, "verbose": -1}, lgb.Dataset(X, y, free_raw_data=False),
                 num_boost_round=10, fpreproc=prep)
    assert len(res["valid multi_logloss-mean"]) == 10


def _dummy_obj(preds, data):
    return np.ones(preds.shape), np.ones(preds.shape)


def _constant_metric_multi(preds, data):
    return [("important_metric", 1.5, False), ("irrelevant_metric", 7.8, False)]


def test_metric_selection_matrix(lgb):
    """test_metrics: which metrics cv() / train() report for every combination of objective
    (built-in / custom), metric in params / arguments / aliases / 'None', and feval."""
    X, y = load_digits(n_class=2, return_X_y=True)
    X_tr, X_te, y_tr, y_te = _split(X, y)
    tr = lgb.Dataset(X_tr, y_tr)
    va = lgb.Dataset(X_te, y_te, reference=tr)
    obj = {"objective": "binary", "verbose": -1}
    dobj = {"objective": _dummy_obj, "verbose": -1}

    def cvkeys(params=obj, **kw):
        return set(lgb.cv(params, tr, num_boost_round=2, **kw))

    def m(*names):
        return {f"valid {n}-{s}" for n in names for s in ("mean", "stdv")}

    cases = [
        ({}, m("binary_logloss")),
        ({"params": dict(obj, metric="binary_error")}, m("binary_error")),
        ({"metrics": "binary_logloss"}, m("binary_logloss")),
        ({"metrics": "binary_error"}, m("binary_error")),
        ({"params": dict(obj, metric="invalid_metric"), "metrics": "binary_error"}, m("binary_error")),
        ({"params": {"objective": "regression", "metric": "quantile", "verbose": 2}}, m("quantile")),
        ({"params": dict(obj, metric=["binary_logloss", "binary_error"])}, m("binary_logloss", "binary_error")),
        ({"metrics": ["binary_logloss", "binary_error"]}, m("binary_logloss", "binary_error")),
        ({"metrics": ["None"]}, set()),
        ({"params": dobj}, set()),
        ({"params": dict(dobj, metric="binary_error")}, m("binary_error")),
        ({"params": dobj, "metrics": "binary_error"}, m("binary_error")),
        ({"params": dict(dobj, metric_types="invalid_metric"), "metrics": "binary_error"}, m("binary_error")),
        ({"params": dict(dobj, metric=["binary_logloss", "binary_error"])}, m("binary_logloss", "binary_error")),
        ({"params": dobj, "metrics": ["binary_logloss", "binary_error"]}, m("binary_logloss", "binary_error")),
        ({"feval": _constant_metric}, m("binary_logloss", "error")),
        ({"params": dict(obj, metric="binary_error"), "feval": _constant_metric}, m("binary_error", "error")),
        ({"metrics": "binary_logloss", "feval": _constant_metric_multi},
         m("binary_logloss", "important_metric", "irrelevant_metric")),
        ({"params": dict(obj, metric="invalid_metric"), "metrics": "binary_error", "feval": _constant_metric},
         m("binary_error", "error")),
        ({"metrics": ["binary_logloss", "binary_error"], "feval": _constant_metric},
         m("binary_logloss", "binary_error", "error")),
        ({"metrics": ["None"], "feval": _constant_metric}, m("error")),
        ({"params": dobj, "feval": _constant_metric}, m("error")),
        ({"params": dict(dobj, metric="binary_error"), "feval": _constant_metric}, m("binary_error", "error")),
        ({"params": dict(dobj, metric="None"), "feval": _constant_metric}, m("error")),
    ]
    for na in ("None", "na", "null", "custom"):
        cases.append(({"metrics": na}, set()))
    for kw, want in cases:
        assert cvkeys(**kw) == want, kw
    r = lgb.cv(obj, tr, num_boost_round=2, metrics="binary_logloss", feval=_constant_metric_multi)
    assert r["valid important_metric-mean"] == [1.5, 1.5] and r["valid irrelevant_metric-mean"] == [7.8, 7.8]

    def trkeys(params=obj, **kw):
        rec = {}
        lgb.train(params, tr, num_boost_round=2, valid_sets=[va], callbacks=[lgb.record_evaluation(rec)], **kw)
        return rec

    assert set(trkeys()["valid_0"]) == {"binary_logloss"}
    assert set(trkeys(dict(obj, metric="binary_error"))["valid_0"]) == {"binary_error"}
    assert set(trkeys(dict(obj, metric=["binary_logloss", "binary_error"]))["valid_0"]) == \
        {"binary_logloss", "binary_error"}
    for na in ("None", "na", "null", "custom"):
        assert trkeys(dict(obj, metric=na)) == {}
    assert trkeys(dobj) == {}
    assert set(trkeys(dict(dobj, metric="binary_logloss"))["valid_0"]) == {"binary_logloss"}
    assert set(trkeys(feval=_constant_metric)["valid_0"]) == {"binary_logloss", "error"}
    rec = trkeys(dict(obj, metric="binary_logloss"), feval=_constant_metric_multi)["valid_0"]
    assert rec["important_metric"] == [1.5, 1.5] and rec["irrelevant_metric"] == [7.8, 7.8] and len(rec) == 3
    assert set(trkeys(dict(obj, metric="None"), feval=_constant_metric)["valid_0"]) == {"error"}
    assert set(trkeys(dobj, feval=_constant_metric)["valid_0"]) == {"error"}

    # multiclass objective aliases and num_class checks
    Xm, ym = load_digits(n_class=3, return_X_y=True)
    trm = lgb.Dataset(Xm, ym)

    def mkeys(params, **kw):
        return set(lgb.cv(params, trm, num_boost_round=2, **kw))

    d3 = {"objective": _dummy_obj, "num_class": 3, "verbose": -1}
    d1 = {"objective": _dummy_obj, "num_class": 1, "verbose": -1}
    aliases = ["multiclass", "softmax", "multiclassova", "multiclass_ova", "ova", "ovr"]
    for a in aliases:
        c3 = {"objective": a, "num_class": 3, "verbose": -1}
        assert mkeys(c3) == m("multi_logloss")
        assert mkeys(c3, feval=_constant_metric) == m("multi_logloss", "error")
        assert mkeys(d3, feval=_constant_metric) == m("error")
        assert mkeys(d1) == set()
        assert mkeys(d1, feval=_constant_metric) == m("error")
        with pytest.raises(lgb.basic.LightGBMError, match="Multiclass objective and metrics don't match"):
            mkeys(d1, metrics=a, feval=_constant_metric)
        with pytest.raises(lgb.basic.LightGBMError,
                           match="Number of classes should be specified and greater than 1 for multiclass training"):
            mkeys({"objective": a, "verbose": -1})
        for ma in aliases + ["multi_logloss"]:
            assert mkeys(c3, metrics=ma) == m("multi_logloss")
        assert mkeys(c3, metrics="multi_error") == m("multi_error")
        with pytest.raises(lgb.basic.LightGBMError, match="Multiclass objective and metrics don't match"):
            mkeys(c3, metrics="binary_logloss")
    with pytest.raises(lgb.basic.LightGBMError, match="Number of classes must be 1 for non-multiclass training"):
        mkeys({"num_class": 3, "verbose": -1})
    assert mkeys(d3) == set()
    for ma in aliases + ["multi_logloss"]:
        assert mkeys(d3, metrics=ma) == m("multi_logloss")
    assert mkeys(d3, metrics="multi_error") == m("multi_error")
    with pytest.raises(lgb.basic.LightGBMError, match="Multiclass objective and metrics don't match"):
        mkeys(d3, metrics="binary_error")


def test_multiple_feval_train_and_cv(lgb):
    """test_multiple_feval_train, test_multiple_feval_cv."""
    X, y = load_breast_cancer(return_X_y=True)
    params = {"verbose": -1, "objective": "binary", "metric": "binary_logloss"}
    X_tr, X_va, y_tr, y_va = train_test_split(X, y, test_size=0.2, random_state=0)
    tr = lgb.Dataset(X_tr, y_tr)
    rec = {}
    lgb.train(params, tr, valid_sets=lgb.Dataset(X_va, y_va, reference=tr), num_boost_round=5,
              feval=[_constant_metric, _decreasing_metric], callbacks=[lgb.record_evaluation(rec)])
    assert set(rec["valid_0"]) == {"binary_logloss", "error", "decreasing_metric"}
    r = lgb.cv(params, lgb.Dataset(X, y), num_boost_round=5, feval=[_constant_metric, _decreasing_metric])
    assert set(r) == {f"valid {n}-{s}" for n in ("binary_logloss", "error", "decreasing_metric")
                      for s in ("mean", "stdv")}


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _logloss_obj(preds, data):
    p = _sigmoid(preds)
    return p - data.get_label(), p * (1.0 - p)


def _mse_obj(preds, data):
    return preds - data.get_label(), np.ones(len(preds))


def test_callable_objective_exact_values(lgb):
    """test_objective_callable_train_binary_classification / _regression: the reference's exact
    training-set log loss, AUC and MSE after 20 rounds with a Python objective."""
    X, y = load_breast_cancer(return_X_y=True)
    b = lgb.train({"verbose": -1, "objective": _logloss_obj, "learning_rate": 0.01}, lgb.Dataset(X, y), 20)
    p = _sigmoid(b.predict(X))
    assert b.params["objective"] == "none"
    assert log_loss(y, p) == pytest.approx(0.547907)
    assert roc_auc_score(y, p) == pytest.approx(0.995944)
    Xr, yr = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    b = lgb.train({"verbose": -1, "objective": _mse_obj}, lgb.Dataset(Xr, yr), 20)
    assert b.params["objective"] == "none"
    assert mean_squared_error(yr, b.predict(Xr)) == pytest.approx(286.724194)


def test_callable_objective_in_cv(lgb):
    """test_objective_callable_cv_binary_classification / _regression."""
    X, y = load_breast_cancer(return_X_y=True)
    cvb = lgb.cv({"verbose": -1, "objective": _logloss_obj, "learning_rate": 0.01}, lgb.Dataset(X, y),
                 num_boost_round=20, nfold=3, return_cvbooster=True)["cvbooster"].boosters
    assert all(b.params["objective"] == "none" for b in cvb)
    assert all(log_loss(y, _sigmoid(b.predict(X))) < 0.56 for b in cvb)
    Xr, yr = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    cvb = lgb.cv({"verbose": -1, "objective": _mse_obj}, lgb.Dataset(Xr, yr), num_boost_round=20, nfold=3,
                 stratified=False, return_cvbooster=True)["cvbooster"].boosters
    assert all(b.params["objective"] == "none" for b in cvb)
    assert all(mean_squared_error(yr, b.predict(Xr)) < 463 for b in cvb)


def test_default_objective_is_regression_with_l2(lgb):
    """test_default_objective_and_metric."""
    X, y = load_breast_cancer(return_X_y=True)
    X_tr, X_te, y_tr, y_te = train_test_split(X, y, test_size=0.2, random_state=0)
    tr = lgb.Dataset(X_tr, y_tr)
    rec = {}
    lgb.train({"verbose": -1}, tr, valid_sets=lgb.Dataset(X_te, y_te, reference=tr), num_boost_round=5,
              callbacks=[lgb.record_evaluation(rec)])
    assert set(rec["valid_0"]) == {"l2"} and len(rec["valid_0"]["l2"]) == 5


def _softmax(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("use_weight", [True, False])
def test_multiclass_custom_objective_and_eval(lgb, use_weight):
    """test_multiclass_custom_objective, test_multiclass_custom_eval."""
    def custom_obj(preds, ds):
        yt, w = ds.get_label(), ds.get_weight()
        prob = _softmax(preds)
        g = prob.copy()
        g[np.arange(len(yt)), yt.astype(int)] -= 1.0
        h = preds.shape[1] / (preds.shape[1] - 1) * prob * (1 - prob)
        if w is not None:
            g, h = g * w.reshape(-1, 1), h * w.reshape(-1, 1)
        return g, h

    def custom_eval(preds, ds):
        return "custom_logloss", log_loss(ds.get_label(), preds, sample_weight=ds.get_weight()), False

    X, y = make_blobs(n_samples=1000, centers=[[-4, -4], [4, 4], [-4, 4]], random_state=42)
    ds = lgb.Dataset(X, y)
    if use_weight:
        ds.set_weight(np.full_like(y, 2))
    params = {"objective": "multiclass", "num_class": 3, "num_leaves": 7}
    builtin = lgb.train(params, ds, num_boost_round=10).predict(X)
    custom = _softmax(lgb.train(dict(params, objective=custom_obj), ds, num_boost_round=10).predict(X))
    np.testing.assert_allclose(builtin, custom, rtol=0.01)
    w = np.full_like(y, 2)
    X_tr, X_va, y_tr, y_va, w_tr, w_va = train_test_split(X, y, w, test_size=0.2, random_state=0)
    tr, va = lgb.Dataset(X_tr, y_tr), None
    va = lgb.Dataset(X_va, y_va, reference=tr)
    if use_weight:
        tr.set_weight(w_tr)
        va.set_weight(w_va)
    rec = {}
    b = lgb.train(params, tr, num_boost_round=10, valid_sets=[tr, va], valid_names=["train", "valid"],
                  feval=custom_eval, callbacks=[lgb.record_evaluation(rec)], keep_training_booster=True)
    for key, d in (("train", tr), ("valid", va)):
        np.testing.assert_allclose(rec[key]["multi_logloss"], rec[key]["custom_logloss"])
        _, metric, value, _ = b.eval(d, key, feval=custom_eval)[1]
        assert metric == "custom_logloss"
        np.testing.assert_allclose(value, rec[key][metric][-1])


# ---------------------------------------------------------------------------
# split value histogram, early stopping on the first metric (test_engine.py:3117-3350)
def test_split_value_histogram_shapes(lgb):
    """test_get_split_value_histogram: the reference's exact bin counts (12 distinct split values
    of feature 0 after 20 trees), numpy / xgboost styles, names vs indices, categorical refusal."""
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    X, y = np.repeat(X, 3, axis=0), np.repeat(y, 3, axis=0)
    X[:, 2] = np.random.default_rng(0).integers(0, 20, size=X.shape[0])
    g = lgb.train({"verbose": -1}, lgb.Dataset(X, y, categorical_feature=[2]), num_boost_round=20)
    kw = {"feature": 0, "xgboost_style": True}
    for bins, rows in ((None, 12), (999, 12), (-1, 1), (0, 1), (1, 1), (2, 2), (6, 6), (7, 7)):
        out = g.get_split_value_histogram(**kw) if bins is None else g.get_split_value_histogram(bins=bins, **kw)
        assert out.shape == (rows, 2), bins
    for f in (0, X.shape[-1] - 1):
        np.testing.assert_allclose(g.get_split_value_histogram(f, xgboost_style=True).values,
                                   g.get_split_value_histogram(g.feature_name()[f], xgboost_style=True).values)
    hist, edges = g.get_split_value_histogram(0)
    assert len(hist) == 20 and len(edges) == 21
    for bins in (999, 1, 2, 6, 7):
        hist, edges = g.get_split_value_histogram(0, bins=bins)
        assert len(hist) == bins and len(edges) == bins + 1
    for bad in (-1, 0):
        with pytest.raises(ValueError, match="`bins` must be positive, when an integer"):
            g.get_split_value_histogram(0, bins=bad)
    for f in (0, X.shape[-1] - 1):
        hi, bi = g.get_split_value_histogram(f)
        hn, bn = g.get_split_value_histogram(g.feature_name()[f])
        np.testing.assert_array_equal(hi, hn)
        np.testing.assert_allclose(bi, bn)
    vals, edges = g.get_split_value_histogram(0, bins="auto")
    xs = g.get_split_value_histogram(0, bins="auto", xgboost_style=True)
    mask = vals > 0
    np.testing.assert_array_equal(vals[mask], xs["Count"].values)
    np.testing.assert_allclose(edges[1:][mask], xs["SplitValue"].values)
    with pytest.raises(lgb.basic.LightGBMError, match="Cannot compute split value histogram for the categorical"):
        g.get_split_value_histogram(2)


def test_early_stopping_first_metric_only_exact_iterations(lgb):
    """test_early_stopping_for_only_first_metric: the reference's exact best iterations (train:
    l1 / l2 best at 3 on the first validation set, l2 at 15 on the second; cv: l1 15, l2 13)."""
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    X_tr, X_te, y_tr, y_te = train_test_split(X, y, test_size=0.2, random_state=42)
    X1, X2, y1, y2 = train_test_split(X_te, y_te, test_size=0.5, random_state=73)
    tr = lgb.Dataset(X_tr, y_tr)
    v1, v2 = lgb.Dataset(X1, y1, reference=tr), lgb.Dataset(X2, y2, reference=tr)

    def run_train(valid, metric, want, first_only, feval=None):
        params = {"objective": "regression", "learning_rate": 1.1, "num_leaves": 10, "metric": metric, "verbose": -1,
                  "seed": 123}
        b = lgb.train(params, tr, num_boost_round=25, valid_sets=valid, feval=feval,
                      callbacks=[lgb.early_stopping(stopping_rounds=5, first_metric_only=first_only)])
        assert b.best_iteration == want, (metric, first_only)

    def run_cv(metric, want, first_only, train_metric, feval=None):
        params = {"objective": "regression", "learning_rate": 0.9, "num_leaves": 10, "metric": metric, "verbose": -1,
                  "seed": 123, "gpu_use_dp": True}
        r = lgb.cv(params, train_set=tr, num_boost_round=25, stratified=False, feval=feval,
                   callbacks=[lgb.early_stopping(stopping_rounds=5, first_metric_only=first_only)],
                   eval_train_metric=train_metric)
        assert len(r[list(r.keys())[0]]) == want, (metric, first_only, train_metric)

    for metric, want, fo in (([], 3, False), ([], 3, True), (None, 3, False), (None, 3, True), ("l2", 3, True),
                             ("l1", 3, True), (["l2", "l1"], 3, True), (["l1", "l2"], 3, True),
                             (["l2", "l1"], 3, False), (["l1", "l2"], 3, False)):
        run_train(v1, metric, want, fo)

    def dec_then_const(p, d):
        return [_decreasing_metric(p, d), _constant_metric(p, d)]

    def const_then_dec(p, d):
        return [_constant_metric(p, d), _decreasing_metric(p, d)]

    run_train(v1, "None", 1, False, feval=dec_then_const)
    run_train(v1, "None", 25, True, feval=dec_then_const)
    run_train(v1, "None", 1, True, feval=const_then_dec)
    run_train([v1, v2], ["l2", "l1"], 3, True)
    run_train([v2, v1], ["l2", "l1"], 3, True)
    run_train([v1, v2], ["l1", "l2"], 3, True)
    run_train([v2, v1], ["l1", "l2"], 3, True)
    for tm in (False, True):
        for metric, want, fo in ((None, 13, True), ("l2", 13, True), ("l1", 15, True), (["l2", "l1"], 13, True),
                                 (["l1", "l2"], 15, True), (["l2", "l1"], 13, False), (["l1", "l2"], 13, False)):
            run_cv(metric, want, fo, tm)
    run_cv("None", 1, False, False, feval=dec_then_const)
    run_cv("None", 25, True, False, feval=dec_then_const)
    run_cv("None", 1, True, False, feval=const_then_dec)


# ---------------------------------------------------------------------------
# node sampling, forced splits / bins, binning, dataset param updates, regularisers
# (test_engine.py:3353-3640)
import json  # noqa: E402


def test_feature_fraction_bynode(lgb):
    """test_node_level_subcol."""
    X_tr, X_te, y_tr, y_te = _split(*load_breast_cancer(return_X_y=True))
    params = {"objective": "binary", "metric": "binary_logloss", "feature_fraction_bynode": 0.8,
              "feature_fraction": 1.0, "verbose": -1}
    b, rec = _train_with_record(lgb, params, X_tr, y_tr, X_te, y_te, 25)
    ret = log_loss(y_te, b.predict(X_te))
    assert ret < 0.14 and rec["binary_logloss"][-1] == pytest.approx(ret)
    b2 = lgb.train(dict(params, feature_fraction=0.5), lgb.Dataset(X_tr, y_tr), 25)
    assert ret != log_loss(y_te, b2.predict(X_te))


def test_forced_split_with_out_of_range_feature(lgb, tmp_path):
    """test_forced_split_feature_indices."""
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    f = tmp_path / "forced_split.json"
    f.write_text(json.dumps({"feature": 0, "threshold": 0.5, "left": {"feature": X.shape[1], "threshold": 0.5}}))
    with pytest.raises(lgb.basic.LightGBMError, match="Forced splits file includes feature index"):
        lgb.train({"objective": "regression", "forcedsplits_filename": f}, lgb.Dataset(X, y))


def test_forced_bins_files(lgb):
    """test_forced_bins (examples/regression/forced_bins*.json)."""
    ex = os.path.join(DATA, "examples", "regression")
    x = np.empty((100, 2))
    x[:, 0] = np.arange(0, 1, 0.01)
    x[:, 1] = -np.arange(0, 1, 0.01)
    y = np.arange(0, 1, 0.01)
    params = {"objective": "regression_l1", "max_bin": 5, "forcedbins_filename": os.path.join(ex, "forced_bins.json"),
              "num_leaves": 2, "min_data_in_leaf": 1, "verbose": -1}
    est = lgb.train(params, lgb.Dataset(x, label=y), num_boost_round=20)
    nx = np.zeros((3, 2))
    nx[:, 0] = [0.31, 0.37, 0.41]
    assert len(np.unique(est.predict(nx))) == 3
    nx[:, 0] = 0
    nx[:, 1] = [-0.9, -0.6, -0.3]
    assert len(np.unique(est.predict(nx))) == 1
    est = lgb.train(dict(params, forcedbins_filename=""), lgb.Dataset(x, label=y), num_boost_round=20)
    assert len(np.unique(est.predict(nx))) == 3
    p2 = dict(params, forcedbins_filename=os.path.join(ex, "forced_bins2.json"), max_bin=11)
    est = lgb.train(p2, lgb.Dataset(x[:, :1], label=y), num_boost_round=50)
    _, counts = np.unique(est.predict(x[1:, :1]), return_counts=True)
    assert min(counts) >= 9 and max(counts) <= 11


def test_binning_one_signed_features(lgb):
    """test_binning_same_sign: zero falls with the negative side for a positive-only feature and
    with the positive side for a negative-only one."""
    x = np.empty((99, 2))
    x[:, 0] = np.arange(0.01, 1, 0.01)
    x[:, 1] = -np.arange(0.01, 1, 0.01)
    y = np.arange(0.01, 1, 0.01)
    est = lgb.train({"objective": "regression_l1", "max_bin": 5, "num_leaves": 2, "min_data_in_leaf": 1,
                     "verbose": -1, "seed": 0}, lgb.Dataset(x, label=y), num_boost_round=20)
    nx = np.zeros((3, 2))
    nx[:, 0] = [-1, 0, 1]
    p = est.predict(nx)
    assert p[0] == pytest.approx(p[1]) and p[1] != pytest.approx(p[2])
    nx = np.zeros((3, 2))
    nx[:, 1] = [-1, 0, 1]
    p = est.predict(nx)
    assert p[0] != pytest.approx(p[1]) and p[1] == pytest.approx(p[2])


def test_dataset_param_updates_allowed_and_refused(lgb):
    """test_dataset_update_params."""
    rng = np.random.default_rng(12)
    base = {"max_bin": 100, "max_bin_by_feature": [20, 10], "bin_construct_sample_cnt": 10000, "min_data_in_bin": 1,
            "use_missing": False, "zero_as_missing": False, "categorical_feature": [0], "feature_pre_filter": True,
            "pre_partition": False, "enable_bundle": True, "data_random_seed": 0, "is_enable_sparse": True,
            "header": True, "two_round": True, "label_column": 0, "weight_column": 0, "group_column": 0,
            "ignore_column": 0, "min_data_in_leaf": 10, "linear_tree": False, "precise_float_parser": True,
            "verbose": -1}
    changed = {"max_bin": 150, "max_bin_by_feature": [30, 5], "bin_construct_sample_cnt": 5000, "min_data_in_bin": 2,
               "use_missing": True, "zero_as_missing": True, "categorical_feature": [0, 1],
               "feature_pre_filter": False, "pre_partition": True, "enable_bundle": False, "data_random_seed": 1,
               "is_enable_sparse": False, "header": False, "two_round": False, "label_column": 1,
               "weight_column": 1, "group_column": 1, "ignore_column": 1,
               "forcedbins_filename": "/some/path/forcedbins.json", "min_data_in_leaf": 2, "linear_tree": True,
               "precise_float_parser": False}
    X, y = rng.uniform(size=(100, 2)), rng.uniform(size=(100,))
    p = dict(base)
    ds = lgb.Dataset(X, y, params=p, free_raw_data=False).construct()
    p["min_data_in_leaf"] -= 1
    lgb.train(p, ds, num_boost_round=3)
    ds = lgb.Dataset(X, y, params=p)
    p["min_data_in_leaf"] -= 1
    lgb.train(p, ds, num_boost_round=3)
    p["min_data_in_leaf"] += 2
    lgb.train(p, ds, num_boost_round=3)
    p["feature_pre_filter"] = False
    ds = lgb.Dataset(X, y, params=p).construct()
    p["min_data_in_leaf"] -= 4
    lgb.train(p, ds, num_boost_round=3)
    p["feature_pre_filter"] = True
    ds = lgb.Dataset(X, y, params=p).construct()
    for key, value in changed.items():
        q = dict(p, **{key: value})
        name = "forced bins" if key == "forcedbins_filename" else key
        msg = ("Reducing `min_data_in_leaf` with `feature_pre_filter=true` may cause *" if key == "min_data_in_leaf"
               else f"Cannot change {name} *")
        with pytest.raises(lgb.basic.LightGBMError, match=msg):
            lgb.train(q, ds, num_boost_round=3)


def test_dataset_params_with_reference_dataset(lgb):
    """test_dataset_params_with_reference."""
    rng = np.random.default_rng(13)
    prm = {"max_bin": 100}
    tr = lgb.Dataset(rng.uniform(size=(100, 2)), rng.uniform(size=(100,)), params=prm, free_raw_data=False).construct()
    va = lgb.Dataset(rng.uniform(size=(100, 2)), rng.uniform(size=(100,)), reference=tr, free_raw_data=False).construct()
    assert tr.get_params() == prm and va.get_params() == prm
    lgb.train(prm, tr, valid_sets=[va])


@pytest.mark.parametrize("extra", [{"extra_trees": True}, {"path_smooth": 1}])
def test_extra_trees_and_path_smoothing_regularise(lgb, extra):
    """test_extra_trees, test_path_smoothing."""
    X, y = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    params = {"objective": "regression", "num_leaves": 32, "verbose": -1, "seed": 0}
    err = mean_squared_error(y, lgb.train(params, lgb.Dataset(X, label=y), 10).predict(X))
    err2 = mean_squared_error(y, lgb.train(dict(params, **extra), lgb.Dataset(X, label=y), 10).predict(X))
    assert err < err2


# ---------------------------------------------------------------------------
# trees_to_dataframe, interaction constraints, linear trees (test_engine.py:3601-3860)
def test_trees_to_dataframe_matches_importances(lgb):
    """test_trees_to_dataframe."""
    pytest.importorskip("pandas")
    X, y = load_breast_cancer(return_X_y=True)
    b = lgb.train({"objective": "binary", "verbose": -1}, lgb.Dataset(X, label=y), 10)
    df = b.trees_to_dataframe()
    cols = [f"Column_{i}" for i in range(X.shape[1])]
    split = df[~df["split_gain"].isnull()].groupby("split_feature").size().to_dict()
    gains = df.groupby("split_feature")["split_gain"].sum().to_dict()
    np.testing.assert_equal([split.get(c, 0.0) for c in cols], b.feature_importance("split"))
    np.testing.assert_allclose([gains.get(c, 0.0) for c in cols], b.feature_importance("gain"))
    assert df["tree_index"].nunique() == 10
    np.testing.assert_equal(df.loc[df["node_depth"] == 1, "count"].values, len(y))
    b = lgb.train({"objective": "binary", "verbose": -1},
                  lgb.Dataset(np.ones((10, 2)), label=np.random.default_rng(1).uniform(size=(10,))), 10)
    df = b.trees_to_dataframe()
    assert len(df) == 1
    assert df.loc[0, "tree_index"] == 0 and df.loc[0, "node_depth"] == 1 and df.loc[0, "node_index"] == "0-L0"
    assert df.loc[0, "value"] is not None
    for c in ("left_child", "right_child", "parent_index", "split_feature", "split_gain", "threshold",
              "decision_type", "missing_direction", "missing_type", "weight", "count"):
        assert df.loc[0, c] is None, c


def test_interaction_constraints_accuracy_ordering(lgb):
    """test_interaction_constraints."""
    X, y = make_regression(n_samples=200, n_features=4, n_informative=2, random_state=42)
    ds = lgb.Dataset(X, label=y)
    params = {"verbose": -1, "seed": 0}
    p1 = lgb.train(params, ds, 10).predict(X)
    np.testing.assert_allclose(p1, lgb.train(dict(params, interaction_constraints=[list(range(4))]), ds, 10).predict(X))
    p3 = lgb.train(dict(params, interaction_constraints=[[0, 2], [1, 3]]), ds, 10).predict(X)
    assert mean_squared_error(y, p1) < mean_squared_error(y, p3)
    p4 = lgb.train(dict(params, interaction_constraints=[[i] for i in range(4)]), ds, 10).predict(X)
    assert mean_squared_error(y, p3) < mean_squared_error(y, p4)
    X2 = np.concatenate([np.zeros((X.shape[0], 1)), X], axis=1)
    lgb.train(dict(params, interaction_constraints=[[0] + list(range(2, 5)), [1] + list(range(2, 5))]),
              lgb.Dataset(X2, label=y), 10)


def test_linear_trees_thread_independent(lgb):
    """test_linear_trees_num_threads."""
    rng = np.random.default_rng(42)
    x = np.arange(0, 1000, 0.1)
    y = 2 * x + rng.normal(0, 0.1, size=(len(x),))
    params = {"verbose": -1, "objective": "regression", "seed": 0, "linear_tree": True, "num_threads": 2}
    p1 = lgb.train(params, lgb.Dataset(x[:, None], label=y), 100).predict(x[:, None])
    p2 = lgb.train(dict(params, num_threads=4), lgb.Dataset(x[:, None], label=y), 100).predict(x[:, None])
    np.testing.assert_allclose(p1, p2)


def test_linear_trees_fit_and_refit(lgb, tmp_path):
    """test_linear_trees."""
    rng = np.random.default_rng(42)
    x = np.arange(0, 100, 0.1)
    y = 2 * x + rng.normal(0, 0.1, len(x))
    x = x[:, None]
    params = {"verbose": -1, "metric": "mse", "seed": 0, "num_leaves": 2}

    def compare(xx, extra=None):
        p1 = lgb.train(params, lgb.Dataset(xx, label=y), 10).predict(xx)
        res = {}
        d = lgb.Dataset(xx, label=y)
        est = lgb.train(dict(params, linear_tree=True, **(extra or {})), d, 10, valid_sets=[d], valid_names=["train"],
                        callbacks=[lgb.record_evaluation(res)])
        p2 = est.predict(xx)
        assert res["train"]["l2"][-1] == pytest.approx(mean_squared_error(y, p2), abs=1e-1)
        return p1, p2

    p1, p2 = compare(x)
    assert mean_squared_error(y, p2) < mean_squared_error(y, p1)
    x[:10] = np.nan
    p1, p2 = compare(x)
    assert mean_squared_error(y, p2) < mean_squared_error(y, p1)
    compare(x, {"subsample": 0.8, "bagging_freq": 1})
    x = np.concatenate([np.ones([x.shape[0], 1]), x], 1)
    x[500:, 1] = np.nan
    y[500:] += 10
    compare(x, {"subsample": 0.8, "bagging_freq": 1})
    x[:250, 0] = 0
    y[:250] += 10
    est = lgb.train(dict(params, linear_tree=True, subsample=0.8, bagging_freq=1),
                    lgb.Dataset(x, label=y, categorical_feature=[0]), 10)
    p1 = est.predict(x)
    assert np.mean(np.abs(p1 - est.refit(x, label=y).predict(x))) < 2
    est.save_model(str(tmp_path / "temp_model.txt"))
    p2 = lgb.Booster(model_file=str(tmp_path / "temp_model.txt")).refit(x, label=y).predict(x)
    assert np.mean(np.abs(p1 - p2)) < 2
    p3 = est.refit(x[:100, :], label=y[:100]).predict(x)
    assert np.mean(np.abs(p2 - p1)) > np.abs(np.max(p3 - p1))
    X_tr, _, y_tr, _ = train_test_split(*load_breast_cancer(return_X_y=True), test_size=0.1, random_state=2)
    prm = {"linear_tree": True, "verbose": -1, "metric": "mse", "seed": 0}
    for nl in (2, 60):
        lgb.train(prm, lgb.Dataset(X_tr, label=y_tr, params=dict(prm, num_leaves=nl), categorical_feature=[0]), 10)


def test_linear_trees_save_load(lgb, tmp_path):
    """test_save_and_load_linear."""
    X_tr, _, y_tr, _ = train_test_split(*load_breast_cancer(return_X_y=True), test_size=0.1, random_state=2)
    X_tr = np.concatenate([np.ones((X_tr.shape[0], 1)), X_tr], 1)
    X_tr[: X_tr.shape[0] // 2, 0] = 0
    y_tr[: X_tr.shape[0] // 2] = 1
    params = {"linear_tree": True}
    d1 = lgb.Dataset(X_tr, label=y_tr, params=params, categorical_feature=[0])
    p1 = lgb.train(params, d1, 10).predict(X_tr)
    d1.save_binary(str(tmp_path / "temp_dataset.bin"))
    e2 = lgb.train(params, lgb.Dataset(str(tmp_path / "temp_dataset.bin")), 10)
    np.testing.assert_allclose(p1, e2.predict(X_tr))
    e2.save_model(str(tmp_path / "model.txt"))
    np.testing.assert_allclose(e2.predict(X_tr), lgb.Booster(model_file=str(tmp_path / "model.txt")).predict(X_tr))


def test_linear_single_leaf_and_unsupported_params(lgb):
    """test_linear_single_leaf, test_linear_raises_informative_errors_on_unsupported_params."""
    X, y = load_breast_cancer(return_X_y=True)
    b = lgb.train({"objective": "binary", "linear_tree": True, "min_sum_hessian": 5000}, lgb.Dataset(X, label=y), 5)
    assert log_loss(y, b.predict(X)) < 0.661
    Xr, yr = make_regression(n_samples=100, n_features=4, n_informative=2, random_state=42)
    with pytest.raises(lgb.basic.LightGBMError, match="Cannot use regression_l1 objective when fitting linear trees"):
        lgb.train({"linear_tree": True, "objective": "regression_l1"}, lgb.Dataset(Xr, label=yr), 1)
    with pytest.raises(lgb.basic.LightGBMError, match="zero_as_missing must be false when fitting linear trees"):
        lgb.train({"linear_tree": True, "zero_as_missing": True}, lgb.Dataset(Xr, label=yr), 1)


# ---------------------------------------------------------------------------------------------
# prediction ranges / shapes, dump_model, sampling strategies, verbosity, informative errors


def _synth(n_samples=100, n_features=4, n_informative=2, random_state=42):
    """tests/python_package_test/utils.py make_synthetic_regression."""
    return make_regression(n_samples=n_samples, n_features=n_features, n_informative=n_informative,
                           random_state=random_state)


def _assert_silent(capsys):
    out = capsys.readouterr()
    assert out.out == "" and out.err == "", out


@pytest.mark.parametrize("case", ["regression", "multiclass", "binary"])
@pytest.mark.parametrize("es_rounds", [1, 5, None])
def test_predict_with_start_iteration(lgb, case, es_rounds):
    """test_predict_with_start_iteration: sums of iteration windows equal the whole model."""
    from sklearn.datasets import load_iris
    if case == "regression":
        X, y = _synth()
        params = {"objective": "regression", "verbose": -1, "metric": "l2", "learning_rate": 0.5}
    elif case == "multiclass":
        X, y = load_iris(return_X_y=True)
        params = {"objective": "multiclass", "num_class": 3, "verbose": -1, "metric": "multi_error"}
    else:
        X, y = load_breast_cancer(return_X_y=True)
        params = {"objective": "binary", "verbose": -1, "metric": "auc"}
    X_tr, X_te, y_tr, y_te = _split(X, y)
    cbs = [lgb.early_stopping(es_rounds, verbose=False)] if es_rounds is not None else []
    b = lgb.train(params, lgb.Dataset(X_tr, label=y_tr), num_boost_round=50,
                  valid_sets=[lgb.Dataset(X_te, label=y_te)], callbacks=cbs)
    all_pred = b.predict(X, raw_score=True)
    all_contrib = b.predict(X, pred_contrib=True)
    for step in (10, 12):
        pred = np.zeros_like(all_pred)
        contrib = np.zeros_like(all_contrib)
        for start in range(0, 50, step):
            pred += b.predict(X, start_iteration=start, num_iteration=step, raw_score=True)
            contrib += b.predict(X, start_iteration=start, num_iteration=step, pred_contrib=True)
        np.testing.assert_allclose(all_pred, pred)
        np.testing.assert_allclose(all_contrib, contrib)
    np.testing.assert_allclose(b.predict(X, start_iteration=-1), b.predict(X, num_iteration=b.best_iteration))
    for kw, n in (({}, 90), ({"pred_leaf": True}, 40), ({"pred_contrib": True}, 40)):
        p4 = b.predict(X, start_iteration=10, num_iteration=-1, **kw)
        np.testing.assert_allclose(p4, b.predict(X, start_iteration=10, num_iteration=n, **kw))
        np.testing.assert_allclose(p4, b.predict(X, start_iteration=10, num_iteration=0, **kw))


@pytest.mark.parametrize("use_init_score", [False, True])
def test_predict_stump(lgb, use_init_score):
    """test_predict_stump: n stumps predict the initial score once, not n times."""
    X, y = load_breast_cancer(return_X_y=True)
    kw = {"data": X, "label": y}
    if use_init_score:
        kw["init_score"] = np.random.default_rng(1).uniform(size=y.shape)
    b = lgb.train(train_set=lgb.Dataset(**kw), params={"objective": "binary", "min_data_in_leaf": X.shape[0],
                                                       "verbose": -1}, num_boost_round=5)
    p1 = b.predict(X, raw_score=True, num_iteration=1)
    pa = b.predict(X, raw_score=True)
    expect = 0.0 if use_init_score else np.log(y.mean() / (1.0 - y.mean()))
    np.testing.assert_allclose(p1, np.full_like(p1, expect), atol=1e-12)
    np.testing.assert_allclose(pa, np.full_like(pa, expect), atol=1e-12)


@pytest.mark.parametrize("kind", ["regression", "binary", "multiclass"])
def test_predict_output_shapes(lgb, kind):
    """test_predict_{regression,binary_classification,multiclass_classification}_output_shape."""
    from sklearn.datasets import make_classification
    n = 1000
    if kind == "regression":
        X, y = _synth(n_samples=n, n_features=4)
        params, k, f = {"objective": "regression", "verbosity": -1}, 1, 4
    elif kind == "binary":
        X, y = make_classification(n_samples=n, n_features=4, n_classes=2, random_state=0)
        params, k, f = {"objective": "binary", "verbosity": -1}, 1, 4
    else:
        X, y = make_classification(n_samples=n, n_features=10, n_classes=3, n_informative=6, random_state=0)
        params, k, f = {"objective": "multiclass", "verbosity": -1, "num_class": 3}, 3, 10
    for rounds in (1, 2):
        b = lgb.train(params, lgb.Dataset(X, label=y), num_boost_round=rounds)
        flat = (n,) if k == 1 else (n, k)
        assert b.predict(X).shape == flat
        assert b.predict(X, raw_score=True).shape == flat
        assert b.predict(X, pred_contrib=True).shape == (n, k * (f + 1))
        assert b.predict(X, pred_leaf=True).shape == (n, k * rounds)


def test_reset_params_works_with_metric_num_class_and_boosting(lgb):
    """test_reset_params_works_with_metric_num_class_and_boosting."""
    X, y = load_breast_cancer(return_X_y=True)
    dataset_params = {"max_bin": 150}
    booster_params = {"objective": "multiclass", "max_depth": 4, "bagging_fraction": 0.8,
                      "metric": ["multi_logloss", "multi_error"], "boosting": "gbdt", "num_class": 5}
    bst = lgb.Booster(params=booster_params, train_set=lgb.Dataset(X, y, params=dataset_params))
    assert bst.params == dict(dataset_params, **booster_params)
    booster_params["bagging_fraction"] += 0.1
    new = bst.reset_parameter(booster_params)
    assert bst.params == dict(dataset_params, **booster_params)
    assert new.params == dict(dataset_params, **booster_params)


def _assert_subtree_valid(node):
    """utils.py assert_subtree_valid: counts / weights add up at every split."""
    if "leaf_count" in node:
        return node["leaf_count"], node["leaf_weight"]
    lc, lw = _assert_subtree_valid(node["left_child"])
    rc, rw = _assert_subtree_valid(node["right_child"])
    assert node["internal_count"] == lc + rc
    assert abs(node["internal_weight"] - (lw + rw)) <= 1e-3
    return node["internal_count"], node["internal_weight"]


def _assert_all_trees_valid(model):
    for i, t in enumerate(model["tree_info"]):
        assert t["tree_index"] == i
        _assert_subtree_valid(t["tree_structure"])


@pytest.mark.parametrize("linear_tree", [False, True])
def test_dump_model_stump(lgb, linear_tree):
    """test_dump_model_stump."""
    X, y = load_breast_cancer(return_X_y=True)
    b = lgb.train({"objective": "binary", "verbose": -1, "linear_tree": linear_tree, "min_data_in_leaf": len(y)},
                  lgb.Dataset(X, label=y), num_boost_round=5)
    d = b.dump_model(num_iteration=5, start_iteration=0)
    assert len(d["tree_info"]) == 1
    ts = d["tree_info"][0]["tree_structure"]
    assert "leaf_value" in ts and ts["leaf_count"] == len(y)


def test_dump_model(lgb):
    """test_dump_model: constant-leaf dump, boost_from_average folded into the first tree."""
    X, y = _synth()
    b = lgb.train({"objective": "regression", "verbose": -1, "boost_from_average": True},
                  lgb.Dataset(X, label=y + 57.5), num_boost_round=5)
    d = b.dump_model(num_iteration=5, start_iteration=0)
    s = str(d)
    for k in ("leaf_features", "leaf_coeff", "leaf_const"):
        assert k not in s
    assert "leaf_value" in s and "leaf_count" in s
    assert all(t["tree_structure"]["internal_value"] != 0 for t in d["tree_info"])
    assert d["tree_info"][0]["tree_structure"]["internal_value"] == pytest.approx(57.5, abs=1)
    _assert_all_trees_valid(d)


def test_dump_model_linear(lgb):
    """test_dump_model_linear."""
    X, y = load_breast_cancer(return_X_y=True)
    b = lgb.train({"objective": "binary", "verbose": -1, "linear_tree": True}, lgb.Dataset(X, label=y), 5)
    d = b.dump_model(num_iteration=5, start_iteration=0)
    _assert_all_trees_valid(d)
    s = str(d)
    for k in ("leaf_features", "leaf_coeff", "leaf_const", "leaf_value", "leaf_count"):
        assert k in s


def test_dump_model_hook(lgb):
    """test_dump_model_hook."""
    def hook(obj):
        if "leaf_value" in obj:
            obj["LV"] = obj.pop("leaf_value")
        return obj

    X, y = load_breast_cancer(return_X_y=True)
    b = lgb.train({"objective": "binary", "verbose": -1}, lgb.Dataset(X, label=y), 5)
    s = str(b.dump_model(5, 0, object_hook=hook))
    assert "leaf_value" not in s and "LV" in s


def test_force_split_with_feature_fraction(lgb, tmp_path):
    """test_force_split_with_feature_fraction: the forced root split survives feature sampling."""
    import json
    from sklearn.metrics import mean_absolute_error
    X_tr, X_te, y_tr, y_te = _split(*_synth())
    f = tmp_path / "forced_split.json"
    f.write_text(json.dumps({"feature": 0, "threshold": 0.5, "right": {"feature": 2, "threshold": 10.0}}))
    b = lgb.train({"objective": "regression", "feature_fraction": 0.6, "force_col_wise": True,
                   "feature_fraction_seed": 1, "forcedsplits_filename": f, "verbose": -1}, lgb.Dataset(X_tr, y_tr))
    assert mean_absolute_error(y_te, b.predict(X_te)) < 15.7
    info = b.dump_model()["tree_info"]
    assert len(info) > 1
    assert all(t["tree_structure"]["split_feature"] == 0 for t in info)


_SAMPLE_BASE = {"metric": "l2", "verbose": -1, "num_threads": 1, "force_row_wise": True, "gpu_use_dp": True}


def _sample_run(lgb, extra):
    X, y = _synth(n_samples=10_000, n_features=10, n_informative=5, random_state=42)
    X_tr, X_te, y_tr, y_te = _split(X, y)
    tr = lgb.Dataset(X_tr, y_tr)
    ev = lgb.Dataset(X_te, y_te, reference=tr)
    rec = {}
    b = lgb.train({**_SAMPLE_BASE, **extra}, tr, num_boost_round=10, valid_sets=ev,
                  callbacks=[lgb.record_evaluation(rec)])
    return rec["valid_0"]["l2"], mean_squared_error(y_te, b.predict(X_te))


def test_goss_boosting_and_strategy_equivalent(lgb):
    """test_goss_boosting_and_strategy_equivalent."""
    extra = {"bagging_seed": 0, "learning_rate": 0.05}
    assert _sample_run(lgb, {**extra, "boosting": "goss"})[0] == _sample_run(lgb, {**extra,
                                                                                   "data_sample_strategy": "goss"})[0]


def test_sample_strategy_with_boosting(lgb):
    """test_sample_strategy_with_boosting: the reference's values for each boosting x sampling pair
    (GOSS / bagging random streams and DART drops reproduced; all seven pinned at abs 1.0)."""
    res = {}
    for name, extra in {"dart_goss": {"boosting": "dart", "data_sample_strategy": "goss"},
                        "gbdt_goss": {"boosting": "gbdt", "data_sample_strategy": "goss"},
                        "goss_goss": {"boosting": "goss", "data_sample_strategy": "goss"},
                        "rf_goss": {"boosting": "rf", "data_sample_strategy": "goss"},
                        "dart_bag": {"boosting": "dart", "data_sample_strategy": "bagging", "bagging_freq": 1,
                                     "bagging_fraction": 0.5},
                        "gbdt_bag": {"boosting": "gbdt", "data_sample_strategy": "bagging", "bagging_freq": 1,
                                     "bagging_fraction": 0.5},
                        "rf_bag": {"boosting": "rf", "data_sample_strategy": "bagging", "bagging_freq": 1,
                                   "bagging_fraction": 0.5}}.items():
        ev, te = _sample_run(lgb, extra)
        assert ev[-1] == pytest.approx(te)
        res[name] = te
    reference = {"dart_goss": 3149.393862, "gbdt_goss": 2547.715968, "goss_goss": 2547.715968,
                 "rf_goss": 2095.538735, "dart_bag": 3134.866931, "gbdt_bag": 2539.792378, "rf_bag": 1518.704481}
    assert res["gbdt_goss"] == res["goss_goss"]
    assert res["dart_goss"] != res["gbdt_goss"] and res["rf_goss"] != res["dart_goss"]
    assert res["rf_goss"] != res["gbdt_goss"]
    assert len({res["dart_bag"], res["gbdt_bag"], res["rf_bag"]}) == 3
    for k, v in res.items():
        assert v == pytest.approx(reference[k], abs=1.0), k


def test_record_evaluation_with_train(lgb):
    """test_record_evaluation_with_train."""
    X, y = _synth()
    ds = lgb.Dataset(X, y)
    rec = {}
    b = lgb.train({"objective": "l2", "num_leaves": 3, "verbose": -1}, ds, num_boost_round=5, valid_sets=[ds],
                  callbacks=[lgb.record_evaluation(rec)])
    assert list(rec.keys()) == ["training"]
    np.testing.assert_allclose(rec["training"]["l2"],
                               [mean_squared_error(y, b.predict(X, num_iteration=i + 1)) for i in range(5)])


@pytest.mark.parametrize("train_metric", [False, True])
def test_record_evaluation_with_cv(lgb, train_metric):
    """test_record_evaluation_with_cv."""
    X, y = _synth()
    rec = {}
    metrics = ["l2", "rmse"]
    hist = lgb.cv({"objective": "l2", "num_leaves": 3, "metric": metrics, "verbose": -1}, lgb.Dataset(X, y),
                  num_boost_round=5, stratified=False, callbacks=[lgb.record_evaluation(rec)],
                  eval_train_metric=train_metric)
    sets = {"valid"} | ({"train"} if train_metric else set())
    assert set(rec.keys()) == sets
    for s in sets:
        for m in metrics:
            for agg in ("mean", "stdv"):
                np.testing.assert_allclose(hist[f"{s} {m}-{agg}"], rec[s][f"{m}-{agg}"])


def test_pandas_with_numpy_regular_dtypes(lgb):
    """test_pandas_with_numpy_regular_dtypes: every integer / bool / float dtype gives the same model."""
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(seed=42)
    n = 100
    df = pd.DataFrame({"x1": rng.integers(0, 2, n), "x2": rng.integers(1, 3, n),
                       "x3": 10 * rng.integers(1, 3, n), "x4": 100 * rng.integers(1, 3, n)}).astype(np.float64)
    y = df["x1"] * (df["x2"] + df["x3"] + df["x4"])
    params = {"objective": "l2", "num_leaves": 31, "min_child_samples": 1, "verbose": -1}
    b = lgb.train(params, lgb.Dataset(df, y), num_boost_round=5)
    preds = b.predict(df)
    assert b.trees_to_dataframe()["split_feature"].nunique() == df.shape[1]
    assert mean_squared_error(y, preds) < mean_squared_error(y, np.full_like(y, y.mean()))
    for dts in (["uint8", "uint16", "uint32", "uint64"], ["int8", "int16", "int32", "int64"],
                ["bool", "float16", "float32", "float64"]):
        df2 = df.astype({f"x{i}": dt for i, dt in enumerate(dts, start=1)})
        assert df2.dtypes.tolist() == dts
        b2 = lgb.train(params, lgb.Dataset(df2, y), num_boost_round=5)
        np.testing.assert_allclose(preds, b2.predict(df2))


def test_pandas_nullable_dtypes(lgb):
    """test_pandas_nullable_dtypes: Int32 / Float64 / boolean / sparse columns train like numpy ones."""
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(seed=42)
    df = pd.DataFrame({"x1": rng.integers(1, 3, 100), "x2": np.linspace(-1, 1, 100),
                       "x3": pd.arrays.SparseArray(rng.integers(0, 11, 100)),
                       "x4": rng.uniform(size=(100,)) < 0.5})
    df.loc[1, "x1"] = np.nan
    df.loc[2, "x2"] = np.nan
    df["x4"] = df["x4"].astype(np.float64)
    df.loc[3, "x4"] = np.nan
    y = (df["x1"] * df["x2"] + df["x3"] * (1 + df["x4"])).fillna(0)
    params = {"objective": "l2", "num_leaves": 31, "min_child_samples": 1, "verbose": -1}
    preds = lgb.train(params, lgb.Dataset(df, y), num_boost_round=5).predict(df)
    df2 = df.copy()
    df2["x1"] = df2["x1"].astype("Int32")
    df2["x2"] = df2["x2"].astype("Float64")
    df2["x4"] = df2["x4"].astype("boolean")
    b2 = lgb.train(params, lgb.Dataset(df2, y), num_boost_round=5)
    assert b2.trees_to_dataframe()["split_feature"].nunique() == df.shape[1]
    assert mean_squared_error(y, preds) < mean_squared_error(y, np.full_like(y, y.mean()))
    np.testing.assert_allclose(preds, b2.predict(df2))


def test_boost_from_average_with_single_leaf_trees(lgb):
    """test_boost_from_average_with_single_leaf_trees (upstream issue 4708 data)."""
    X = np.array([[1021.0589, 1018.9578], [1023.85754, 1018.7854], [1024.5468, 1018.88513],
                  [1019.02954, 1018.88513], [1016.79926, 1018.88513], [1007.6, 1018.88513]], dtype=np.float32)
    y = np.array([1023.8, 1024.6, 1024.4, 1023.8, 1022.0, 1014.4], dtype=np.float32)
    params = {"extra_trees": True, "min_data_in_bin": 1, "extra_seed": 7, "objective": "regression",
              "verbose": -1, "boost_from_average": True, "min_data_in_leaf": 1}
    m = np.mean(lgb.train(params, lgb.Dataset(X, y), num_boost_round=10).predict(X))
    assert y.min() <= m <= y.max()


def test_cegb_split_buffer_clean(lgb):
    """test_cegb_split_buffer_clean: CEGB per-leaf split buffers are reset between trees."""
    rng = np.random.default_rng(seed=42)
    R, C = 1000, 100
    data = rng.standard_normal(size=(R, C))
    for i in range(1, C):
        data[i] += data[0] * rng.standard_normal()
    N = int(0.8 * R)
    tr_y, te_y = data[:N].sum(axis=1), data[N:].sum(axis=1)
    params = {"boosting_type": "gbdt", "objective": "regression", "max_bin": 255, "num_leaves": 31, "seed": 0,
              "learning_rate": 0.1, "min_data_in_leaf": 0, "verbose": -1, "min_split_gain": 1000.0,
              "cegb_penalty_feature_coupled": 5 * np.arange(C), "cegb_penalty_split": 0.0002,
              "cegb_tradeoff": 10.0, "force_col_wise": True}
    b = lgb.train(params, lgb.Dataset(data[:N], tr_y), num_boost_round=10)
    assert np.sqrt(mean_squared_error(te_y, b.predict(data[N:]))) < 10.0


def test_verbosity_and_verbose(lgb, capsys):
    """test_verbosity_and_verbose: verbosity wins over its alias, and says so."""
    X, y = _synth()
    lgb.train({"num_leaves": 3, "verbose": 1, "verbosity": 0}, lgb.Dataset(X, y), num_boost_round=1)
    assert ("[Warning] verbosity is set=0, verbose=1 will be ignored. Current value: verbosity=0"
            in capsys.readouterr().out)


def test_verbosity_is_respected_when_using_custom_objective(lgb, capsys):
    """test_verbosity_is_respected_when_using_custom_objective."""
    def mse_obj(y_pred, dtrain):
        return y_pred - dtrain.get_label(), np.ones(len(y_pred))

    X, y = _synth()
    ds = lgb.Dataset(X, y)
    params = {"objective": mse_obj, "nonsense": 123, "num_leaves": 3}
    lgb.train({**params, "verbosity": -1}, ds, num_boost_round=1)
    _assert_silent(capsys)
    lgb.train({**params, "verbosity": 0}, ds, num_boost_round=1)
    assert "[Warning] Unknown parameter: nonsense" in capsys.readouterr().out


@pytest.mark.parametrize("verbosity_param", ["verbosity", "verbose"])
@pytest.mark.parametrize("verbosity", [-1, 0])
def test_verbosity_can_suppress_alias_warnings(lgb, capsys, verbosity_param, verbosity):
    """test_verbosity_can_suppress_alias_warnings."""
    X, y = _synth()
    lgb.train({"num_leaves": 3, "subsample": 0.75, "bagging_fraction": 0.8, "force_col_wise": True,
               verbosity_param: verbosity}, lgb.Dataset(X, y), num_boost_round=1)
    out = capsys.readouterr().out
    msg = "bagging_fraction is set=0.8, subsample=0.75 will be ignored. Current value: bagging_fraction=0.8"
    if verbosity >= 0:
        assert msg in out
    else:
        assert "[Warning]" not in out and "[Info]" not in out


@pytest.mark.parametrize("use_cv", [False, True])
def test_num_rounds_warning_only_when_expected(lgb, capsys, use_cv):
    """test_{train,cv}_only_raises_num_rounds_warning_when_expected."""
    import warnings
    X, y = _synth()
    ds = lgb.Dataset(X, y)
    base = {"num_leaves": 5, "objective": "regression", "verbosity": -1}

    def trees(params, **kw):
        if use_cv:
            out = lgb.cv(params, ds, return_cvbooster=True, stratified=False, **kw)["cvbooster"].num_trees()
            assert len(set(out)) == 1
            return out[0]
        return lgb.train(params, ds, **kw).num_trees()

    quiet = [({}, {}, 100), ({}, {"num_boost_round": 2}, 2), ({"n_iter": 3}, {"num_boost_round": 3}, 3),
             ({"n_iter": 4}, {"num_boost_round": 3}, 4), ({"n_iter": 3, "num_iterations": 3}, {}, 3),
             ({"n_iter": 3, "num_trees": 3, "nrounds": 3, "max_iter": 3}, {}, 3)]
    for extra, kw, n in quiet:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert trees({**base, **extra}, **kw) == n
        _assert_silent(capsys)
    with pytest.warns(UserWarning, match="will perform up to 5 boosting rounds"):
        assert trees({**base, "n_iter": 6, "num_iterations": 5}) == 5
    _assert_silent(capsys)
    with pytest.warns(UserWarning, match="will perform up to 4 boosting rounds"):
        assert trees({**base, "n_iter": 4, "max_iter": 5}) == 4
    _assert_silent(capsys)


def test_validate_features(lgb):
    """test_validate_features: predict / refit check the column names when asked to."""
    pd = pytest.importorskip("pandas")
    X, y = _synth()
    df = pd.DataFrame(X, columns=["x1", "x2", "x3", "x4"])
    b = lgb.train({"num_leaves": 15, "verbose": -1}, lgb.Dataset(df, y), num_boost_round=10)
    assert b.feature_name() == ["x1", "x2", "x3", "x4"]
    df2 = df.rename(columns={"x3": "z"})
    with pytest.raises(lgb.basic.LightGBMError, match="Expected 'x3' at position 2 but found 'z'"):
        b.predict(df2, validate_features=True)
    b.predict(df2, validate_features=False)
    with pytest.raises(lgb.basic.LightGBMError, match="Expected 'x3' at position 2 but found 'z'"):
        b.refit(df2, y, validate_features=True)
    b.refit(df2, y, validate_features=False)


def test_train_and_cv_raise_informative_errors(lgb):
    """test_train_and_cv_raise_informative_error_for_{train_set_of_wrong_type,impossible_num_boost_round},
    test_train_raises_informative_error_{if_any_valid_sets_are_not_dataset_objects,for_params_of_wrong_type}."""
    with pytest.raises(TypeError, match=r"train\(\) only accepts Dataset object, train_set has type 'list'\."):
        lgb.train({}, train_set=[])
    with pytest.raises(TypeError, match=r"cv\(\) only accepts Dataset object, train_set has type 'list'\."):
        lgb.cv({}, train_set=[])
    X, y = _synth()
    for n in (-7, -1, 0):
        msg = rf"Number of boosting rounds must be greater than 0\. Got {n}\."
        with pytest.raises(ValueError, match=msg):
            lgb.train({}, train_set=lgb.Dataset(X, y), num_boost_round=n)
        with pytest.raises(ValueError, match=msg):
            lgb.cv({}, train_set=lgb.Dataset(X, y), num_boost_round=n)
    with pytest.raises(TypeError, match=r"Every item in valid_sets must be a Dataset object\. Item 1 has type 'tuple'\."):
        lgb.train(params={}, train_set=lgb.Dataset(X, y),
                  valid_sets=[lgb.Dataset(X * 2.0, y), ([1.0], [2.0]), [5.6, 5.7, 5.8]])
    with pytest.raises(lgb.basic.LightGBMError, match='Parameter num_leaves should be of type int, got "too-many"'):
        lgb.train({"num_leaves": "too-many"}, lgb.Dataset(X, label=y))


def test_bagging_by_query_in_lambdarank(lgb):
    """test_bagging_by_query_in_lambdarank (reference examples/lambdarank data)."""
    import os
    from sklearn.datasets import load_svmlight_file
    d = os.path.join(os.path.dirname(__file__), "data")
    X_tr, y_tr = load_svmlight_file(os.path.join(d, "rank.train"))
    X_te, y_te = load_svmlight_file(os.path.join(d, "rank.test"))
    q_tr = np.loadtxt(os.path.join(d, "rank.train.query"))
    q_te = np.loadtxt(os.path.join(d, "rank.test.query"))
    params = {"objective": "lambdarank", "verbose": -1, "metric": "ndcg", "ndcg_eval_at": [5]}
    tr = lgb.Dataset(X_tr, y_tr, group=q_tr, params=params)
    te = lgb.Dataset(X_te, y_te, group=q_te, params=params)
    base = lgb.train(params, tr, num_boost_round=50, valid_sets=[te]).best_score["valid_0"]["ndcg@5"]
    for by_query in (True, False):
        p = dict(params, bagging_by_query=by_query, bagging_fraction=0.1, bagging_freq=1)
        s = lgb.train(p, tr, num_boost_round=50, valid_sets=[te]).best_score["valid_0"]["ndcg@5"]
        assert s >= base - 0.1


def test_equal_predict_from_row_major_and_col_major_data(lgb):
    """test_equal_predict_from_row_major_and_col_major_data."""
    X, y = _synth()
    assert X.flags["C_CONTIGUOUS"]
    b = lgb.train({"num_leaves": 8, "verbose": -1}, lgb.Dataset(X, y), num_boost_round=5)
    Xc = np.asfortranarray(X)
    assert Xc.flags["F_CONTIGUOUS"] and not Xc.flags["C_CONTIGUOUS"]
    np.testing.assert_allclose(b.predict(X), b.predict(Xc))


@pytest.mark.parametrize("use_cv", [False, True])
def test_objective_callable_regression(lgb, use_cv):
    """test_objective_callable_{train,cv}_regression (train value 286.724194 pinned)."""
    def mse_obj(y_pred, dtrain):
        return y_pred - dtrain.get_label(), np.ones(len(y_pred))

    X, y = _synth()
    params = {"verbose": -1, "objective": mse_obj}
    if not use_cv:
        b = lgb.train(params, lgb.Dataset(X, y), num_boost_round=20)
        assert b.params["objective"] == "none"
        assert mean_squared_error(y, b.predict(X)) == pytest.approx(286.724194)
        return
    res = lgb.cv(params, lgb.Dataset(X, y), num_boost_round=20, nfold=3, stratified=False, return_cvbooster=True)
    for cb in res["cvbooster"].boosters:
        assert cb.params["objective"] == "none"
        assert mean_squared_error(y, cb.predict(X)) < 463


def test_missing_value_handle_more_na():
    """test_engine.py::test_missing_value_handle_more_na: 80 % NaN rows of a constant
    column are learned apart from the rest (l2 < 0.005 after 20 rounds, no average boost)."""
    import random

    import lambdagap_amd as lgb
    from sklearn.metrics import mean_squared_error

    X_train = np.ones((100, 1))
    y_train = np.ones(100)
    for idx in random.Random(0).sample(range(100), 80):
        X_train[idx, 0] = np.nan
        y_train[idx] = 0
    evals_result = {}
    gbm = lgb.train({"metric": "l2", "verbose": -1, "boost_from_average": False}, lgb.Dataset(X_train, y_train),
                    num_boost_round=20, valid_sets=lgb.Dataset(X_train, y_train),
                    callbacks=[lgb.record_evaluation(evals_result)])
    ret = mean_squared_error(y_train, gbm.predict(X_train))
    assert ret < 0.005
    assert evals_result["valid_0"]["l2"][-1] == pytest.approx(ret)
