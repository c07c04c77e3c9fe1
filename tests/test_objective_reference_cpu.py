"""The float64 references of objective_cases.py against the host objectives (device_type=cpu):
first-round gradients of every pointwise, one-vs-all and softmax case, second-round gradients,
renewed leaf values and refit leaf values. ops.booster_gradients returns the host objective's
gradients here, so this validates the references themselves, and include/lgap/pointwise.h and
src/objective/objectives.cpp against the reference project's definitions, before
test_objective_kernels.py lets them judge the HIP kernels."""
import pytest

import lambdagap_amd as lgb

from objective_cases import (FIRST_ROUND_CASES, RENEW_CASES, SECOND_ROUND_CASES, check_first_round, check_refit,
                             check_renewal, check_second_round)


@pytest.mark.parametrize("name", FIRST_ROUND_CASES)
def test_first_round_gradients(name):
    check_first_round(lgb, "cpu", name)


@pytest.mark.parametrize("name", SECOND_ROUND_CASES)
def test_second_round_gradients(name):
    check_second_round(lgb, "cpu", name)


@pytest.mark.parametrize("name", RENEW_CASES)
def test_renewed_leaf_values(name):
    check_renewal(lgb, "cpu", name)


def test_refit_leaf_values():
    check_refit(lgb, "cpu")
