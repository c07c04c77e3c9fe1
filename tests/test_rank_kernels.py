"""The HIP ranking kernels against the float64 references of rank_cases.py (validated against the
host objectives and metrics by test_rank_reference_cpu.py):

  * k_lambdarank (src/device/grad_kernels.hip), first-round gradients at a given init score, every
    document within 4 x c_host x 2^-23 x sigmoid x W_d of the reference (rank_cases.C_HOST) and, as
    before, within 1e-4 of the host objective. By query length the `mixed` cases run the early out
    (1 document), the two-thread rank sort (2 .. 128), the one-thread rank sort (129, 255, 256), the
    LDS bitonic sort with the register permutation (257 .. 2048) and the kGlobal launch (2049, 3000)
    in one dataset, so the LDS arrays have Pa = 2048 for every shorter P; `short_array` gives
    Pa = 256, `tiny` Pa = 2, `no_long` no kGlobal launch.
      - paths:<k>:<pattern>: NDCG at truncation 1 / 30 / 32 (the register pair loop) and 33 / 100000
        (the general loop under TGT == kTgtNdcg), with distinct scores, ties (five values), all-equal
        scores (best == worst: no |ds| division), one -inf document per query and -0.0 next to +0.0;
      - target:<t>:weighted | ties: all 18 targets through k_lambdarank<false, -1> and <true, -1>,
        with row weights and lambdagap_weight, and with tied scores;
      - option:*: lambdarank_norm=false, sigmoid=2, label gains at and above kRankLdsGains;
      - probe:*: one relevant document at rank 0, k - 1, k, 63, 64, 255, 256, cnt - 1 of queries of
        64 / 65 / 256 / 257 / 2048 / 2049 documents; every document without a pair exactly zero;
  * k_pos_accum / k_pos_update: 7 positions (the LDS branch) and 1025 (global atomics), with and
    without regularization; the Newton step from the device's own gradients, and second-round
    gradients ranked by score + non-zero bias;
  * k_xendcg<false> and <true>: two rounds, single-document queries, ties;
  * k_query_metric<NDCG | MAP | precision> with rocPRIM's segmented sort: queries of up to 5000
    documents (79 chunks of 64), eval positions on both sides of the chunk boundaries and beyond the
    query, up to kMaxEvalAt of them; single-query datasets, so nothing averages an error away."""
import pytest

import lambdagap_amd as lgb

import rank_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_required):
    return gpu_required


@pytest.mark.parametrize("name", rc.GRADIENT_CASES)
def test_lambdarank_gradients(name):
    rc.check_gradients(lgb, "gpu", name)


@pytest.mark.parametrize("name", rc.DETERMINISM_CASES)
def test_lambdarank_deterministic(name):
    rc.check_deterministic(lgb, "gpu", name)


@pytest.mark.parametrize("name", rc.POSITION_CASES)
def test_position_bias(name):
    rc.check_position_bias(lgb, "gpu", name)


def test_no_positions_no_biases():
    rc.check_no_positions(lgb, "gpu")


@pytest.mark.parametrize("name", rc.XENDCG_CASES)
def test_xendcg_two_rounds(name):
    rc.check_xendcg(lgb, "gpu", name)


@pytest.mark.parametrize("name", rc.METRIC_CASES)
def test_query_metrics(name):
    rc.check_metrics(lgb, "gpu", name)
