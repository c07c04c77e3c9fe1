"""The oracles of the RF device tests, checked on the CPU (no GPU needed).

test_rf_device.py holds the device-scored running average to predict(raw_score=True) within
rf_device_cases.bound; here device_type=cpu (the host arithmetic the device path reproduces) meets
the same bound at the same shapes, before and after a rollback. test_blend_score_kernel.py takes a
row's leaf value of one tree from predict(start_iteration=j, num_iteration=1); here those values,
added in tree order, are predict(raw_score=True) of the whole booster, bit for bit."""
import numpy as np
import pytest

import lambdagap_amd as lgb

import blend_score_cases
import rf_device_cases as rf

REGRESSION = [c for c in rf.CASES if "num_class" not in rf.CASES[c].get("params", {})]


@pytest.mark.parametrize("case", REGRESSION)
def test_bound_holds_on_the_cpu(case):
    got = rf.bitwise_run(lgb, case, device=False, device_type="cpu")
    assert got["trees"] == rf.ITERS and got["bound"] > 0
    print(f"{case}: train diff {got['train_diff']:.3e}, valid diff {got.get('valid_diff', 0.0):.3e} (bound {got['bound']:.3e})")
    assert got["train_diff"] <= got["bound"]
    if rf.CASES[case].get("valid"):
        assert got["valid_diff"] <= got["bound"]
    # the averaged score is not the sum: the bound is a statement about RF
    assert "average_output" in got["model"]


def test_bound_holds_after_a_rollback_on_the_cpu():
    got = rf.rollback_run(lgb, device_type="cpu")
    assert got["trees_after_rollback"] == rf.ITERS - 1 and got["trees"] == rf.ITERS
    print(f"train diff {got['train_diff']:.3e} (bound {got['bound']:.3e})")
    assert got["train_diff"] <= got["bound"]


def test_bound_is_tight_enough_to_see_a_wrong_average():
    """A score averaged over one tree too many misses the bound by orders of magnitude."""
    m, t = 1.0, rf.ITERS
    assert rf.bound(t, m) < 1e-3 * m / (t + 1)


@pytest.mark.parametrize("kind", sorted(blend_score_cases.LAYOUTS))
def test_leaf_extraction_reproduces_predict(kind):
    lay = blend_score_cases.layout(kind)
    nl = lay.num_leaves()
    assert nl[blend_score_cases.ONE_LEAF] == 1 and 1 < nl[blend_score_cases.SMALL] <= 15
    assert nl[blend_score_cases.BIG] > 256
    total = np.zeros(blend_score_cases.N)
    for j in range(3):
        total = total + lay.leaf[j]
    want = lay.booster.predict(lay.X, raw_score=True)
    assert np.array_equal(total.view(np.int64), want.view(np.int64))
    # every row's value of a tree is one of that tree's leaf values
    for j, t in enumerate(lay.booster.dump_model()["tree_info"]):
        values = set()

        def walk(node):
            if "leaf_value" in node:
                values.add(node["leaf_value"])
            else:
                walk(node["left_child"])
                walk(node["right_child"])

        walk(t["tree_structure"])
        assert set(np.unique(lay.leaf[j]).tolist()) <= values
