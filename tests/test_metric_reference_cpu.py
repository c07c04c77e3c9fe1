"""The host metrics on given scores (device_type=cpu) against the references of metric_cases.py,
and the references against values worked out by hand and against sklearn. Runs anywhere; the same
cases run on the HIP kernels in test_metric_kernels.py.
"""
import fractions
import math

import numpy as np
import pytest

import metric_cases as mc

LN2 = 0.6931471805599453
# `-std::log(kEpsilon)` of the float kEpsilon = 1e-15f: the float logarithm. ln(1.0000000036e-15) =
# -15 ln 10 + 3.6e-9 = -34.5387763913; floats are 2^-18 = 3.8e-6 apart there, and the nearest one is
# 9054133 * 2^-18 = 34.538776397705078 (9054133 / 262144; the next ones are 34.5387726 and 34.5387802)
CLAMP = 9054133 / 262144
LOG_1E12 = 27.631021115928547  # -log(1e-12)


@pytest.mark.parametrize("name", mc.POINTWISE_CASES)
def test_pointwise_metrics(lgb, name):
    mc.check_case_cpu(lgb, "pointwise", name)


@pytest.mark.parametrize("name", mc.MULTI_CASES)
def test_multiclass_metrics(lgb, name):
    mc.check_case_cpu(lgb, "multi", name)


@pytest.mark.parametrize("name", mc.AUC_CASES)
def test_auc_average_precision(lgb, name):
    """single_class_wide_weights: only positives with weights from 2^-20 to 2^20. The reference
    project's `sum_pos != sumw` compares two sums taken in different orders there and AUC came out as
    0 / (sum_pos * (sumw - sum_pos)) = 0; a class is absent iff its weight total is exactly 0."""
    mc.check_case_cpu(lgb, "auc", name)


@pytest.mark.parametrize("name", mc.AUC_MU_CASES)
def test_auc_mu(lgb, name):
    mc.check_case_cpu(lgb, "auc_mu", name)


def test_auc_mu_65_classes(lgb):
    case = mc.auc_mu_fallback_case()
    train, valid = mc.evaluate(mc.booster(lgb, "cpu", case))
    mc.check_values(case, "train", train, "cpu", "auc_mu 65 classes")
    mc.check_values(case, "valid", valid, "cpu", "auc_mu 65 classes")


def test_report_c_host(lgb):
    """Prints the table metric_cases.C_HOST is copied from (run with -s)."""
    seen = {}
    for family in ("pointwise", "multi"):
        for name in mc.FAMILIES[family][0]:
            case = mc.get_case(family, name)
            train, valid = mc.evaluate(mc.booster(lgb, "cpu", case))
            for part, values in (("train", train), ("valid", valid)):
                for metric, got in values.items():
                    figure, how = mc.deviation(case, part, metric, got)
                    if how == "loss":
                        kind = case["ref_" + part][metric]["kind"]
                        seen[kind] = max(seen.get(kind, 0.0), figure)
    assert set(seen) == set(mc.C_HOST) - {"binary_error"}
    print("\nC_HOST = {" + ", ".join(f'"{k}": {math.ceil(v * 10 - 1e-9) / 10:.1f}' for k, v in seen.items()) + "}")
    for kind, v in seen.items():
        assert v <= mc.cpu_bound(kind), f"{kind}: {v:.2f} units on the host, C_HOST says {mc.C_HOST[kind]}"


# ------------------------------------------------------------------ the references against hand-worked values
def _pw(kind, setting, y, raw, w=None):
    return mc.pointwise_reference(kind, setting, np.array(y, dtype=np.float32), np.array(raw, dtype=np.float64),
                                  None if w is None else np.array(w, dtype=np.float32))["value"]


@pytest.mark.parametrize("kind, setting, y, raw, w, want", [
    ("l2", "regression", [1.0, 0.0], [3.0, 1.0], None, (4.0 + 1.0) / 2),
    ("l2", "reg_sqrt", [1.0, 0.0], [-2.0, 3.0], None, (25.0 + 81.0) / 2),  # -4 and 9
    ("rmse", "regression", [1.0, 0.0], [4.0, 4.0], None, math.sqrt(12.5)),
    ("rmse", "regression", [1.0, 0.0], [4.0, 4.0], [3.0, 1.0], math.sqrt(43.0 / 4)),
    ("l1", "regression", [1.0, -2.0], [3.0, 1.0], [1.0, 3.0], (2.0 + 9.0) / 4),
    ("quantile", "regression", [2.0, 0.5, 1.0], [0.5, 2.0, 1.0], None, (0.75 * 1.5 + 0.25 * 1.5 + 0.0) / 3),
    ("huber", "regression", [0.0, 0.0, 0.0], [0.5, 2.0, -0.75], None, (0.125 + 0.75 * (2.0 - 0.375) + 0.28125) / 3),
    ("fair", "regression", [0.0], [1.5], None, 2.25 * (1.0 - LN2)),
    ("mape", "regression", [0.25, -4.0], [3.0, -2.0], None, (2.75 + 0.5) / 2),
    ("poisson", "poisson", [2.0], [0.0], None, 1.0),
    ("poisson", "poisson", [2.0], [-30.0], None,
     1.00000001335143196e-10 + 2 * (23.025850929940457 - 1.3351431871e-8)),  # clamped at 1e-10f: 10 ln 10 - ln(1.0000000134)
    ("gamma", "gamma", [2.0], [0.0], None, 2.0),
    ("gamma", "gamma", [1.0], [LN2], None, 0.5 + LN2),
    # t = 2 / (1 + 1e-9): t - log t - 1 = 1 - ln 2 - 1e-9 + O(1e-18), times 2 and not divided by n
    ("gamma_deviance", "gamma", [2.0, 2.0], [0.0, 0.0], None, 2 * 2 * (1 - LN2 - 1e-9)),
    ("tweedie", "tweedie", [2.0], [0.0], None, 2 / 0.3 + 1 / 0.7),
    ("binary_logloss", "binary1", [1.0, 0.0], [0.0, 0.0], None, LN2),
    ("binary_logloss", "binary2.5", [1.0, 0.0, 1.0, 0.0], [-800.0, 800.0, 800.0, -800.0], None, 2 * CLAMP / 4),
    ("binary_logloss", "binary2.5", [0.0], [0.4 * math.log(3.0)], None, math.log(4.0)),  # p = 3 / 4
    ("binary_error", "binary1", [1.0, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, 1.0], None, 2 / 4),  # p == 0.5 predicts 0
    ("binary_error", "binary1", [1.0, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, 1.0], [1.0, 2.0, 4.0, 8.0], 9 / 15),
    ("cross_entropy", "cross_entropy", [0.5, 1.0, 0.0], [0.0, 800.0, 800.0], None, (LN2 + 0.0 + LOG_1E12) / 3),
    ("cross_entropy_lambda", "cross_entropy_lambda", [0.5, 1.0], [0.0, 0.0], None, (LN2 + LN2) / 2),
    # weight 2: p = 1 - exp(-2 ln 2) = 3 / 4; divided by n, not by the weight sum
    ("cross_entropy_lambda", "cross_entropy_lambda", [1.0, 0.0], [0.0, 0.0], [2.0, 1.0], (math.log(4 / 3) + LN2) / 2),
    ("kullback_leibler", "cross_entropy", [0.5, 0.5], [0.0, 0.0], None, 0.0),
    ("kullback_leibler", "cross_entropy", [1.0, 0.25], [0.0, 0.0], [1.0, 3.0],
     (LN2 + 3 * LN2) / 4 + 3 * (0.25 * math.log(0.25) + 0.75 * math.log(0.75)) / 4),
])
def test_pointwise_reference_by_hand(kind, setting, y, raw, w, want):
    got = _pw(kind, setting, y, raw, w)
    assert got == pytest.approx(want, rel=4e-15, abs=1e-300)


def test_fair_reference_small_residual_by_hand():
    """c x - c^2 log1p(x / c) = x^2 / 2 - x^3 / (3 c) + O(x^4): the series is cut there, hence 1e-9."""
    x = 2.0 ** -30
    assert _pw("fair", "regression", [1.0], [1.0 + x]) == pytest.approx(x * x / 2 * (1 - x / 2.25), rel=1e-9)


def test_multiclass_reference_by_hand():
    def ref(metric, objective, top_k, y, raw, w=None):
        return mc.multiclass_reference(metric, objective, 2.0, top_k, np.array(y, dtype=np.float32), np.array(raw),
                                       None if w is None else np.array(w, dtype=np.float32))["value"]

    raw = [[0.0, 0.0, 0.0], [800.0, 0.0, 0.0], [math.log(2.0), 0.0, 0.0]]
    y = [2, 1, 0]
    # p_y: 1 / 3, exp(-800) (clamped), 2 / 4
    assert ref("multi_logloss", "multiclass", 1, y, raw) == pytest.approx((math.log(3) + CLAMP + LN2) / 3, rel=4e-15)
    # one-vs-all, sigmoid 2: 1 / 2, 1 / 2, 1 / (1 + 1 / 4)
    assert ref("multi_logloss", "multiclassova", 1, y, raw) == pytest.approx((LN2 + LN2 + math.log(1.25)) / 3, rel=4e-15)
    # classes with p >= p_y, the true one included: 3, 3 (two tied at 0 below 800), 1
    assert ref("multi_error", "multiclass", 1, y, raw) == 2 / 3
    assert ref("multi_error", "multiclass", 2, y, raw) == 2 / 3
    assert ref("multi_error", "multiclass", 3, y, raw) == 0.0
    assert ref("multi_error", "multiclassova", 2, y, raw, w=[1.0, 2.0, 5.0]) == 3 / 8
    # a true class tied for the top counts as an error at top_k = 1, not at 2
    assert ref("multi_error", "multiclass", 1, [0], [[1.0, 1.0, 0.0]]) == 1.0
    assert ref("multi_error", "multiclass", 2, [0], [[1.0, 1.0, 0.0]]) == 0.0


def test_auc_reference_by_hand():
    y = np.array([1, 0, 1, 0], dtype=np.float32)
    s = np.array([2.0, 1.0, 1.0, 0.0])
    w = np.array([1.0, 2.0, 3.0, 0.5], dtype=np.float32)
    # pairs (positive, negative): 2 > 1, 2 > 0, 1 == 1 (half), 1 > 0
    assert mc.auc_pairs(y, s, None) == 7 / 8
    assert mc.auc_pairs(y, s, w) == pytest.approx((1 * 2 + 1 * 0.5 + 3 * 2 * 0.5 + 3 * 0.5) / (4 * 2.5), rel=4e-16)
    # thresholds 2, 1: precision 1 / 1 and 2 / 3
    assert mc.average_precision_thresholds(y, s, None) == fractions.Fraction(5, 6)
    assert mc.average_precision_thresholds(y, s, w) == pytest.approx((1 * (1 / 1) + 3 * (4 / 6)) / 4, rel=4e-16)
    for f in (mc.auc_ap_grouped, mc.auc_ap_reference):
        assert f(y, s, None) == pytest.approx((7 / 8, 5 / 6), rel=4e-16)
        assert f(y, s, w) == pytest.approx((0.7, 0.75), rel=4e-16)
    # -0.0 ties with +0.0; a single class is 1
    z = np.array([-0.0, 0.0])
    assert mc.auc_pairs(np.array([1, 0], dtype=np.float32), z, None) == 0.5
    assert mc.auc_ap_grouped(np.array([1, 0], dtype=np.float32), z, None) == (0.5, 0.5)
    assert mc.auc_ap_reference(np.array([1, 1], dtype=np.float32), z, None) == (1.0, 1.0)
    assert mc.auc_ap_grouped(np.array([0, 0], dtype=np.float32), z, np.array([1, 2], dtype=np.float32)) == (1.0, 1.0)


def test_auc_mu_reference_by_hand():
    cw = mc.default_class_weights(2)
    # d = 2 (s_0 - s_1): class 0 at 2, class 1 at -2 and 1
    assert mc.auc_mu_reference([0, 1, 1], [[1.0, 0.0], [0.0, 1.0], [1.0, 0.5]], None, cw) == 1.0
    # class 0 at 1, class 1 at 1 (a tie, half) and -2
    assert mc.auc_mu_reference([0, 1, 1], [[0.5, 0.0], [1.0, 0.5], [0.0, 1.0]], None, cw) == 0.75
    assert mc.auc_mu_reference([0, 1, 1], [[0.5, 0.0], [1.0, 0.5], [0.0, 1.0]], [2.0, 3.0, 1.0], cw) == (0.5 * 3 + 1) / 4
    # three classes, every row scored alike: every pair ties
    assert mc.auc_mu_reference([0, 1, 2, 2], np.full((4, 3), 0.25), None, mc.default_class_weights(3)) == 0.5
    # three classes separated along their own score: every pair ordered
    assert mc.auc_mu_reference([0, 1, 2], np.eye(3), None, mc.default_class_weights(3)) == 1.0


def test_grouped_form_equals_pair_definition():
    """The two forms of the AUC / average-precision reference agree where both apply."""
    for name in ("rounded:257", "zeros:257", "extreme:257", "distinct:255", "all_equal:256"):
        d = mc.auc_case(name)["train"]
        pair = (float(mc.auc_pairs(d["y"], d["s"], d["w"])), float(mc.average_precision_thresholds(d["y"], d["s"], d["w"])))
        assert mc.auc_ap_grouped(d["y"], d["s"], d["w"]) == pytest.approx(pair, rel=8 * mc.U)


@pytest.mark.parametrize("name", [f"{p}:{n}" for p in ("all_equal", "distinct", "rounded", "zeros") for n in mc.SIZES[1:]]
                         + ["distinct:grid"])
def test_auc_reference_against_sklearn(name):
    """Where sklearn defines the value (two classes, finite scores): its float64 cumulative sums and
    trapezoid are three sums of non-negative terms as well."""
    from sklearn.metrics import average_precision_score, roc_auc_score

    case = mc.auc_case(name)
    for part in ("train", "valid"):
        d = case[part]
        if len(np.unique(d["y"])) < 2:
            continue
        ref = case["ref_" + part]
        bound = mc.nonneg_bound(len(d["y"]))
        assert roc_auc_score(d["y"], d["s"], sample_weight=d["w"]) == pytest.approx(ref["auc"], rel=bound)
        assert average_precision_score(d["y"], d["s"], sample_weight=d["w"]) == pytest.approx(ref["average_precision"], rel=bound)
