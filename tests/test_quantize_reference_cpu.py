"""quantize_cases.py's renewed-leaf reference against the host learner (device_type=cpu): with
quant_train_renew_leaf every leaf of a quantized tree is the Newton step of the TRUE gradients of
its rows, at 4 levels and at 254 (where the host quantizer's levels pass int8). This validates the
reference before test_quantize_kernels.py lets it judge k_leaf_true_sums. The quantizer's level
formulas themselves are checked against the host in tests/cpp/test_native.cpp
(TestGradientQuantizerLevels)."""
import numpy as np
import pytest

import lambdagap_amd as lgb

import quantize_cases as qc


@pytest.mark.parametrize("bins", [4, 254])
def test_renewed_leaves_are_true_newton_steps(bins):
    qc.check_renewed_leaves(lgb, "cpu", bins)


def test_renewed_leaves_softmax():
    qc.check_renewed_leaves(lgb, "cpu", 4, objective="multiclass")


def test_reference_levels_and_packing():
    """The numpy reference on values worked out by hand: 4 bins, max |g| = 1 -> gs = 0.5;
    max h = 0.25 -> hs = 0.0625."""
    g = np.array([1.0, -1.0, 0.26, -0.26, 0.24, 0.0, -0.74, 0.76], dtype=np.float32)
    h = np.array([0.25, 0.0, 0.1, 0.03, 0.032, 0.2, 0.22, 0.01], dtype=np.float32)
    mg, mh, gs, hs = qc.scales(g, h, 4)
    assert (mg, mh, gs, hs) == (1.0, 0.25, 0.5, 0.0625)
    lg, _ = qc.deterministic_levels(g, gs)
    lh, _ = qc.deterministic_levels(h, hs)
    assert lg.tolist() == [2, -2, 1, -1, 0, 0, -1, 2]
    assert lh.tolist() == [4, 0, 2, 0, 1, 3, 4, 0]
    assert qc.packed([-127, 127, -1, 0], [254, 1, 0, 255]).tolist() == [0x81FE, 0x7F01, 0xFF00, 0x00FF]
    assert qc.dequantized(lg, gs).tolist() == [1.0, -1.0, 0.5, -0.5, 0.0, 0.0, -0.5, 1.0]
    # constant hessian: the scale is the value itself
    assert qc.scales(g, np.full(8, 0.25, dtype=np.float32), 4, const_hess=True)[3] == 0.25
    # an exactly unbiased rounding has z = 0; always rounding to nearest is far outside 6 sigma
    f, up = qc.rounding_residuals(g, lg, gs)
    rng = np.random.default_rng(0)
    v = rng.uniform(-1, 1, 50_000).astype(np.float32)
    x = qc.scaled(v, 0.01)
    nearest = qc.sign(v) * np.floor(x + 0.5).astype(np.int64)
    drawn = qc.sign(v) * (np.floor(x) + (rng.random(v.size) < x - np.floor(x))).astype(np.int64)
    fn, upn = qc.rounding_residuals(v, nearest, 0.01)
    fd, upd = qc.rounding_residuals(v, drawn, 0.01)
    assert max(abs(z) for z in qc.unbiased_statistics(fd, upd).values()) < qc.SIGMA
    assert max(abs(z) for z in qc.unbiased_statistics(fn, upn).values()) > 5 * qc.SIGMA
    assert abs(qc.product_statistic(fd, upd, fd, upd)) > 5 * qc.SIGMA  # one draw used twice
    assert abs(qc.changed_statistic(fd, drawn, nearest)) > 5 * qc.SIGMA
