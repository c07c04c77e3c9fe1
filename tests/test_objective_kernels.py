"""The HIP gradient, leaf renewal and refit kernels against the float64 references of
objective_cases.py (validated against the host objectives by test_objective_reference_cpu.py):

  * first-round gradients at a given init score: k_pointwise2, k_ova, k_softmax
    (src/device/grad_kernels.hip);
  * second-round gradients through the deferred score add, k_leaf_add<uint8_t | uint16_t, GRAD=true>
    (src/device/traverse_kernels.hip), bit-identical to a twin whose score was flushed in between
    (k_leaf_add<T, false>, then k_pointwise2);
  * renewed leaf values: k_renew_gather, the segmented sort, k_renew_pick (src/device/leaf_kernels.hip);
  * refit leaf values: k_refit_partial, k_refit_fold, k_add_leaf_delta."""
import pytest

import lambdagap_amd as lgb

from objective_cases import (FIRST_ROUND_CASES, RENEW_CASES, SECOND_ROUND_CASES, check_first_round, check_refit,
                             check_renewal, check_second_round)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_required):
    return gpu_required


@pytest.mark.parametrize("name", FIRST_ROUND_CASES)
def test_first_round_gradients(name):
    check_first_round(lgb, "gpu", name)


@pytest.mark.parametrize("name", SECOND_ROUND_CASES)
def test_second_round_gradients(name):
    check_second_round(lgb, "gpu", name)


@pytest.mark.parametrize("name", RENEW_CASES)
def test_renewed_leaf_values(name):
    check_renewal(lgb, "gpu", name)


def test_refit_leaf_values():
    check_refit(lgb, "gpu")
