"""The device metric kernels on given scores against the float64 / long double references of
metric_cases.py: k_metric_partial / k_multi_metric_partial / k_metric_fold (src/device/grad_kernels.hip),
k_auc_prep / k_auc_terms / k_auc_fold / k_aucmu_pair and the rocPRIM sort, reduce-by-key and scan
(src/device/metric_kernels.hip), through the training and the validation score view.

Every case runs in one child process started with LGAP_TIMETAG=1 (PhaseTimer reads it once, at first
use), which for each case checks (metric_cases.run_case_device)
  - the device value against the reference within the device bound,
  - the device value against the host metric (LGAP_DEVICE_METRICS=0) on the same booster within 1e-12,
  - two evaluations bit-identical (fixed-order folds, rocPRIM's deterministic_* calls),
  - the call counts of Device::EvalMetric / EvalValid / EvalMultiMetric / EvalAucMu / EvalRankMetric:
    they grow by exactly the number of metric evaluations of the case, and not at all under
    LGAP_DEVICE_METRICS=0, so a silent fallback to the host fails the case,
and returns a verdict per case. auc_mu with 65 classes is above the device path's class limit: no
device evaluation is counted and the value still equals the reference.
"""
import json
import os
import subprocess
import sys

import pytest

import metric_cases as mc

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
_CHILD = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import metric_cases as c; c.main()"


@pytest.fixture(scope="module")
def verdicts(gpu_required):
    env = dict(os.environ, LGAP_TIMETAG="1")
    env.pop("LGAP_DEVICE_METRICS", None)
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(TESTS), TESTS], capture_output=True, text=True,
                       timeout=900, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    print("largest loss units on the device:", out["seen"])
    return out["verdicts"]


def _verdict(verdicts, key):
    assert key in verdicts, f"{key} did not run"
    assert verdicts[key] is None, verdicts[key]


@pytest.mark.parametrize("name", mc.POINTWISE_CASES)
def test_pointwise_metrics(verdicts, name):
    _verdict(verdicts, f"pointwise/{name}")


@pytest.mark.parametrize("name", mc.MULTI_CASES)
def test_multiclass_metrics(verdicts, name):
    _verdict(verdicts, f"multi/{name}")


@pytest.mark.parametrize("name", mc.AUC_CASES)
def test_auc_average_precision(verdicts, name):
    _verdict(verdicts, f"auc/{name}")


@pytest.mark.parametrize("name", mc.AUC_MU_CASES)
def test_auc_mu(verdicts, name):
    _verdict(verdicts, f"auc_mu/{name}")


def test_auc_mu_above_the_class_limit_is_evaluated_on_the_host(verdicts):
    _verdict(verdicts, "auc_mu/fallback65")
