"""The float64 references of rank_cases.py against the host objectives and metrics (device_type=cpu):
lambdarank gradients of all 18 targets at every query-length class and score pattern, the
position-bias Newton step, rank_xendcg over two rounds, and NDCG / MAP / precision at real query
lengths. ops.booster_gradients returns the host objective's gradients here, so this validates the
references themselves, and include/lgap/rank_math.h and src/objective/rank_objective.cpp against
the reference project's definitions, before test_rank_kernels.py lets them judge the HIP kernels.

It is also where rank_cases.C_HOST and XENDCG_HOST_RATIO come from: test_report_c_host prints, per
target, the largest deviation of the host objective the tests before it measured (run with -s)."""
import numpy as np
import pytest

import lambdagap_amd as lgb

import rank_cases as rc

_measured = {}


@pytest.mark.parametrize("name", rc.GRADIENT_CASES)
def test_lambdarank_gradients(name):
    _measured[name] = (rc.gradient_case(name)["target"], rc.check_gradients(lgb, "cpu", name))


def test_gradient_cases_reach_every_path():
    """The case list itself: every query-length class, both NDCG loops, Pa != P, -inf, ties."""
    sizes = rc.gradient_case("paths:30:distinct")["sizes"]
    for lo, hi in ((1, 1), (2, 128), (129, 256), (257, 2048), (2049, 10 ** 9)):
        assert ((sizes >= lo) & (sizes <= hi)).any()
    assert {64, 65, 128, 129, 256, 257, 2048, 2049} <= set(sizes.tolist())
    assert max(rc.gradient_case("paths:30:distinct:short_array")["sizes"]) == 200
    assert max(rc.gradient_case("paths:30:distinct:no_long")["sizes"]) == 2048
    s = rc.gradient_case("paths:30:one_minus_inf")["s"]
    assert np.isneginf(s).sum() == (sizes >= 2).sum()
    assert len(np.unique(rc.gradient_case("paths:30:ties")["s"])) == 5
    for t in rc.TARGETS:
        assert f"target:{t}:weighted" in rc.GRADIENT_CASES and f"target:{t}:ties" in rc.GRADIENT_CASES


def test_quantised_sigmoid_bins():
    """The clamps and the bin edges of the 2^20-bin table."""
    q = rc.quantised_sigmoid(np.array([-30.0, -25.0, 0.0, 25.0, 30.0, 50.0 / 2 ** 20 * 0.999]), 1.0)
    assert q[0] == q[1] == 1.0 / (1.0 + np.exp(-25.0))
    assert q[2] == 0.5 and q[5] == 0.5
    assert q[3] == q[4] == 1.0 / (1.0 + np.exp(25.0 - 50.0 / 2 ** 20))


@pytest.mark.parametrize("name", rc.DETERMINISM_CASES)
def test_lambdarank_deterministic(name):
    rc.check_deterministic(lgb, "cpu", name)


@pytest.mark.parametrize("name", rc.POSITION_CASES)
def test_position_bias(name):
    _measured["position:" + name] = ("ndcg", rc.check_position_bias(lgb, "cpu", name))


def test_no_positions_no_biases():
    rc.check_no_positions(lgb, "cpu")


@pytest.mark.parametrize("name", rc.XENDCG_CASES)
def test_xendcg_two_rounds(name):
    _measured["xendcg:" + name] = ("xendcg", rc.check_xendcg(lgb, "cpu", name))


@pytest.mark.parametrize("name", rc.METRIC_CASES)
def test_query_metrics(name):
    rc.check_metrics(lgb, "cpu", name)


def test_report_c_host():
    """Prints what the tests above measured on the host (run with -s) and holds the tables of
    rank_cases.py to it: the measurement stays within the power of two the CPU tests assert, and, when
    every case of this file has run, no entry is inflated (the device bounds are 4 x the entries):
    at most a quarter above the measurement."""
    worst = {}
    for target, ratio in _measured.values():
        worst[target] = max(worst.get(target, 0.0), ratio)
    for target, ratio in sorted(worst.items()):
        print(f"measured on the host: {target} {ratio:.5f}")
    complete = len(_measured) == len(rc.GRADIENT_CASES) + len(rc.POSITION_CASES) + len(rc.XENDCG_CASES)
    for target, ratio in worst.items():
        if target == "xendcg":
            table, limit = rc.XENDCG_HOST_RATIO, 1.0
        else:
            table, limit = rc.C_HOST[target], rc.cpu_bound(target)
        assert ratio <= limit, f"{target}: measured {ratio}, limit {limit}"
        if complete:
            assert table <= 1.25 * ratio, f"{target}: table {table}, measured {ratio}"
