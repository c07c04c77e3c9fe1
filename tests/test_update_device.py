"""Booster.update_device / raw_score_device: custom objectives and metrics on GPU tensors.

The checks are in update_device_cases.py; every comparison there is bit for bit (model text,
``ops.booster_gradients``, raw scores), with no tolerance. The shapes sit around the gradient
kernels' thresholds (src/device/set_grad_kernels.hip): 4 rows per thread and 256 threads per
block in the row-streaming kernel, a 256-row LDS tile in the (N, K) kernel, 16-byte alignment
for the wide loads.

torch wheels bundle a ROCm runtime of their own, and a process serves both torch and this
library only when torch created its context first (tests/test_predict_device.py). So the checks
run in one fresh interpreter that starts with torch and reports one verdict per check; a second
one repeats the score export with validation sets scored on the host (LGAP_DEVICE_VALID=0).
"""
import json
import os
import subprocess
import sys

import pytest

from update_device_cases import CHECK_NAMES, SCORE_EXPORT_NAMES

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
_CHILD = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import update_device_cases as c; "
          "c.main(sys.argv[3])")


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_required):
    return gpu_required


def _run_child(prefix, env=None):
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(TESTS), TESTS, prefix], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def verdicts():
    return _run_child("")


@pytest.fixture(scope="module")
def host_valid_verdicts():
    return _run_child("score_export-", dict(os.environ, LGAP_DEVICE_VALID="0"))


@pytest.mark.parametrize("check", CHECK_NAMES)
def test_update_device(check, verdicts):
    assert verdicts.get(check, "not run: an earlier check ended with a HIP error") == "ok"


@pytest.mark.parametrize("check", SCORE_EXPORT_NAMES)
def test_score_export_with_host_scored_validation(check, host_valid_verdicts):
    assert host_valid_verdicts.get(check, "not run") == "ok"
