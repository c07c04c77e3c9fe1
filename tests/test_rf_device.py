"""boosting=rf with the averaged scores on the GPU (device_type=gpu), next to the host-scored path.

LGAP_DEVICE_RF selects the path and is read once per process: unset (the default, the same as
"1") keeps the training score, the validation scores and the metrics on the device, a tree blended
into the running average by one kernel, s = (s * iter + tree(row)) * (1 / (iter + 1)); "0" is the
earlier behaviour (three fp64 passes over the scores and a traversal on the host). Each path runs
in a fresh child interpreter (rf_device_cases.py), one after the other.

Bit for bit (objective=regression, whose output is the raw score, so both paths can read it): the
blend kernels round exactly as the host's three passes do, the device sampler draws the host's
bags, and the gradients are the same fp32 values, so the model text, the training score after
every iteration and every validation score after every iteration are identical across the two
paths, for every option set of rf_device_cases.CASES. On the device path the scores are also read
through raw_score_device, which must agree with eval's host read.

The path is proven, not assumed: the device child's phase timers count Device::BlendLeafMap where
the tree just grown scores the training set through its leaf map and Device::BlendTraverse where a
validation set or a walked training set is present; the "0" child counts neither.

Against a definition: after the last iteration every score equals predict(raw_score=True) of the
final model within (4 T + 6) 2^-53 M (rf_device_cases.bound derives it), T and M read from the run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from rf_device_cases import BLEND_TIMERS, CASES, GATED, ITERS

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
_CHILD = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import rf_device_cases as c; c.main(sys.argv[3])"


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_required):
    return gpu_required


def _run_child(what, switch):
    env = dict(os.environ, LGAP_TIMETAG="1")
    env.pop("LGAP_DEVICE_RF", None)
    env.pop("LGAP_FRONTIER", None)
    if switch is not None:
        env["LGAP_DEVICE_RF"] = switch
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(TESTS), TESTS, what], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def runs():
    return {"device": _run_child("device", None), "host": _run_child("host", "0")}


def _of(runs, path, key):
    got = runs[path][key]
    assert "error" not in got, f"{path} path, {key}: {got['error']}"
    return got


@pytest.fixture(scope="module")
def metrics():
    return _run_child("metrics", None)


@pytest.mark.parametrize("case", list(CASES))
def test_two_paths_bit_for_bit(case, runs):
    ref, got = _of(runs, "host", case), _of(runs, "device", case)
    classes = CASES[case].get("params", {}).get("num_class", 1)
    assert ref["trees"] == ITERS * classes
    assert len(ref["train"]) == ITERS and len(set(ref["train"])) == ITERS
    assert got["model"] == ref["model"], "the model text differs"
    assert got["train"] == ref["train"], "the training score differs"
    assert got["valid"] == ref["valid"], "the validation score differs"
    if CASES[case].get("valid"):
        assert len(ref["valid"]) == ITERS
    if classes == 1:
        # raw_score_device against eval's host read, training and validation, every iteration
        assert len(got["same"]) == ITERS * (2 if CASES[case].get("valid") else 1)
        assert all(got["same"])


@pytest.mark.parametrize("case", list(CASES))
def test_the_blend_kernels_ran(case, runs):
    grew = _of(runs, "device", case)["grew"]
    if CASES[case]["leaf_map"]:
        assert grew["Device::BlendLeafMap"] > 0, grew
    else:
        assert grew["Device::BlendLeafMap"] == 0, grew
    if CASES[case].get("valid") or not CASES[case]["leaf_map"]:
        assert grew["Device::BlendTraverse"] > 0, grew
    # the gradients were computed once, in Init: no host gradient pass per iteration
    assert grew["GBDT::Boosting"] == 0, grew
    host = _of(runs, "host", case)["grew"]
    assert all(host[t] == 0 for t in BLEND_TIMERS), host


@pytest.mark.parametrize("path", ["device", "host"])
@pytest.mark.parametrize("case", [c for c in CASES if "num_class" not in CASES[c].get("params", {})])
def test_final_score_equals_predict(case, path, runs):
    got = _of(runs, path, case)
    print(f"{case} {path}: train diff {got['train_diff']:.3e}, valid diff {got.get('valid_diff', 0.0):.3e} "
          f"(bound {got['bound']:.3e})")
    assert got["bound"] > 0
    assert got["train_diff"] <= got["bound"]
    if CASES[case].get("valid"):
        assert got["valid_diff"] <= got["bound"]


def test_rollback(runs):
    ref, got = _of(runs, "host", "rollback"), _of(runs, "device", "rollback")
    assert ref["trees_after_rollback"] == got["trees_after_rollback"] == ITERS - 1
    assert got["train"] == ref["train"], "the training score after the rollback differs"
    print(f"after the rollback: train diff {got['train_diff']:.3e}, valid diff {got['valid_diff']:.3e} "
          f"(bound {got['bound']:.3e})")
    assert got["train_diff"] <= got["bound"]
    # the device path rolls the validation scores back too (the host path leaves them)
    assert got["valid_diff"] <= got["bound"]
    assert got["trees"] == ref["trees"] == ITERS
    assert got["model"] == ref["model"], "the model text after one more iteration differs"


def test_metrics_match_host_recomputation(metrics):
    assert metrics["trees"] == ITERS and len(metrics["recomputed"]) == ITERS
    np.testing.assert_allclose(np.array(metrics["reported"]), np.array(metrics["recomputed"]), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", list(GATED) + ["init_model"])
def test_host_path_configurations_say_why(name, runs):
    got = _of(runs, "device", "gated_" + name)
    assert got["trees"] > 0 and got["finite"]
    reason = {"regression_l1": "renews leaf outputs", "linear_tree": "linear_tree", "goss": "goss",
              "init_model": "init model"}[name]
    assert any("host" in ln and reason in ln for ln in got["log"]), got["log"]
    assert all(got["grew"][t] == 0 for t in BLEND_TIMERS), got["grew"]
    assert "raw_score_device" in got["refused"], got["refused"]


def test_unknown_switch_value_is_fatal():
    got = _run_child("bad_value", "2")
    assert "LGAP_DEVICE_RF" in got["error"] and "'2'" in got["error"]
