"""boosting=dart with the score on the GPU (device_type=gpu), next to the host-scored path.

LGAP_DEVICE_DART selects the path and is read once per process: "forest" keeps the score on the
device and rescoring the dropped trees is one forest traversal (k_traverse_forest), unset (the
default, the same as "tree") keeps it there with one single-tree traversal per dropped tree, "0"
is the earlier behaviour (score and objective on the host). Each path runs in a fresh child interpreter (dart_device_cases.py).

Bit for bit: with a numpy objective through Booster.update(fobj=...) the gradients are the same
host arrays on every path, so the model text, the preds handed to the objective at every
iteration and the host-read validation score must be identical across the three; "0" is the
reference. (Under bagging and GOSS the "0" path used to add a new tree twice to its out-of-bag
rows, the device learner's host-side add already covering every row; these cases caught it.)

Metrics (objective=binary, device mode): every iteration's training binary_logloss and validation
auc next to the same metrics recomputed in numpy from the raw scores read back through
raw_score_device, within the 1e-12 of test_device_metrics.py. The reads go through DART's
drop-on-first-read like the metric itself; before the last one skip_drop is set to 1, so that the
final scores can be compared with predictions of the final model.

The incremental score against fresh predictions, in raw-score space. A row's incremental score is
the init score plus E edits e_1 .. e_E (a tree added, a dropped tree subtracted, a dropped tree
re-added at its new weight), each add rounded to fp64; predict(raw_score=True) sums the T final
trees, each add rounded too. Every partial sum of either is bounded by S = sum |e_i| <= sum over
the edits of the edited tree's largest |leaf|, so each rounding errs by at most 2^-53 * S, and the
two sums, E + T <= 2 E roundings together, differ by at most 2^-52 * E * S. The run recovers E and
S itself (dart_device_cases.EditTracker). With objective=binary the device modes read the raw
scores through raw_score_device; the "0" run can only read probabilities, inverts them, and is
held to the same bound after each row's inversion error is taken off
(dart_device_cases._logit_with_slack). The numpy-objective runs read raw scores on every path, and
hold the same check for every option set, the sampled ones (bagging, GOSS on the host and on the
device sampler) included: a tree added twice to its out-of-bag rows misses it by a leaf value.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dart_device_cases import BITWISE_CASES, CUSTOM_CASES, ITERS

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
_CHILD = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import dart_device_cases as c; c.main(sys.argv[3])"
MODES = {"forest": "forest", "tree": None, "host": "0"}  # None: unset, the default


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_required):
    return gpu_required


def _run_child(what, mode, **extra_env):
    env = dict(os.environ, **extra_env)
    env.pop("LGAP_DEVICE_DART", None)
    if MODES[mode] is not None:
        env["LGAP_DEVICE_DART"] = MODES[mode]
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(TESTS), TESTS, what], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def custom():
    return {mode: _run_child("custom", mode) for mode in MODES}


@pytest.fixture(scope="module")
def builtin():
    # device mode starts with torch (raw_score_device hands the raw scores back), as test_update_device.py does
    return {"forest": _run_child("builtin_torch", "forest", LGAP_TIMETAG="1"),
            "tree": _run_child("builtin_torch", "tree", LGAP_TIMETAG="1"),
            "host": _run_child("builtin", "host", LGAP_TIMETAG="1")}


@pytest.mark.parametrize("case", BITWISE_CASES)
def test_three_paths_bit_for_bit(case, custom):
    ref = custom["host"][case]
    assert ref["trees"] == ITERS * CUSTOM_CASES[case].get("num_class", 1)
    assert len(ref["preds"]) == ITERS and len(set(ref["preds"])) == ITERS
    if case == "valid":
        assert len(ref["valid"]) == ITERS
    for mode in ("forest", "tree"):
        got = custom[mode][case]
        assert got["preds"] == ref["preds"], f"{mode}: the preds handed to the objective differ"
        assert got["valid"] == ref["valid"], f"{mode}: the validation score differs"
        assert got["model"] == ref["model"], f"{mode}: the model text differs"


def test_rollback_then_update(custom):
    assert custom["host"]["rollback"]["trees"] == 8
    for mode in ("forest", "tree"):
        assert custom[mode]["rollback"]["model"] == custom["host"]["rollback"]["model"]


@pytest.mark.parametrize("mode", list(MODES))
def test_linear_tree_dart_is_host_scored(mode, custom):
    got = custom[mode]["linear"]
    assert got["trees"] == 5 and got["finite"]
    assert any("host" in ln for ln in got["log"]), got["log"]


def test_builtin_objective_runs_on_the_device(builtin):
    assert "GBDT::Boosting(device)" in builtin["forest"]["report"]
    assert "GBDT::Boosting(device)" in builtin["tree"]["report"]
    assert "GBDT::Boosting(device)" not in builtin["host"]["report"]


@pytest.mark.parametrize("mode", ["forest", "tree"])
def test_builtin_metrics_match_host_recomputation(mode, builtin):
    got = builtin[mode]
    assert got["trees"] == ITERS and len(got["recomputed"]) == ITERS
    np.testing.assert_allclose(np.array(got["reported"]), np.array(got["recomputed"]), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("mode", ["forest", "tree", "host"])
def test_incremental_score_against_fresh_predictions(mode, builtin):
    got = builtin[mode]
    assert got["edits"] > ITERS  # trees were dropped
    print(f"{mode}: train diff {got['train_diff']:.3e} (less inversion error {got['train_excess']:.3e}, bound "
          f"{got['bound']:.3e}), valid diff {got['valid_diff']:.3e} ({got['valid_excess']:.3e}, bound {got['v_bound']:.3e})")
    # device modes: raw scores, no inversion error (excess == diff); "0": the inverted probabilities
    assert got["train_excess"] <= got["bound"]
    assert got["valid_excess"] <= got["v_bound"]
    if mode != "host":
        assert got["train_excess"] == got["train_diff"] and got["valid_excess"] == got["valid_diff"]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(CUSTOM_CASES))
def test_final_score_equals_predict(case, mode, custom):
    """Every option set, every path: the training (and validation) score after the last iteration
    against predict(raw_score=True), within 2^-52 * E * S."""
    got = custom[mode][case]
    assert got["trees"] == ITERS * CUSTOM_CASES[case].get("num_class", 1) and got["edits"] > ITERS
    print(f"{case} {mode}: train diff {got['train_diff']:.3e} (bound {got['bound']:.3e})")
    assert got["train_diff"] <= got["bound"]
    if case == "valid":
        assert got["valid_diff"] <= got["v_bound"]


def test_unknown_switch_value_is_fatal():
    env = dict(os.environ, LGAP_DEVICE_DART="forrest")
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(TESTS), TESTS, "unknown_value"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert "LGAP_DEVICE_DART" in got["error"] and "forrest" in got["error"]


@pytest.mark.parametrize("mode", ["forest", "tree"])
def test_raw_score_device_and_update_device_refusal(mode, builtin):
    got = builtin[mode]["torch"]
    assert got["same"] == [True] * len(got["same"]) and len(got["same"]) == 12
    assert "update" in got["refused"] and "dart" in got["refused"]
    assert got["trees"] == 12
