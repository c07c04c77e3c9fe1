"""The gradient quantizer's kernels against the float64 definition of quantize_cases.py.

ops.quantize_gradients runs the device learner's own QuantizeGradients (k_qmax then k_quantize,
src/device/seq_hist_kernels.hip, with its grid, seed and round counter) and reads back what it
left: the maxima, the de-quantized (g, h), the packed integer levels and the kept true gradients.
k_leaf_true_sums (quant_train_renew_leaf) is checked through one trained tree, on the frontier
engine and on the sequential chain. test_quantize_reference_cpu.py and test_native.cpp validate
the same references against the host code."""
import functools

import numpy as np
import pytest

import quantize_cases as qc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _dataset(n):
    import lambdagap_amd as lgb

    ds = lgb.Dataset(qc.features(n), np.zeros(n), params=dict(qc.DATASET_PARAMS))
    ds.construct()
    return ds


def _quantize(n, g, h, params, **kw):
    from lambdagap_amd import ops

    return ops.quantize_gradients(_dataset(n), g, h, {"verbosity": -1, **params}, **kw)


def _assert_maxima(q, g, h, num_class):
    n = g.size // num_class
    for c in range(num_class):
        gs, hs = g[c * n:(c + 1) * n], h[c * n:(c + 1) * n]
        assert q["max_g"][0, c].view(np.uint32) == np.abs(gs).max().astype(np.float32).view(np.uint32), (c, q["max_g"][0, c])
        assert q["max_h"][0, c].view(np.uint32) == np.abs(hs).max().astype(np.float32).view(np.uint32), (c, q["max_h"][0, c])


# ------------------------------------------------------------------ k_qmax
@pytest.mark.parametrize("num_class", [1, 3])
@pytest.mark.parametrize("where", ["0", "1", "mid", "n-2", "n-1"])
def test_qmax_is_exact_wherever_the_maximum_sits(gpu_required, num_class, where):
    """max |g| at the named row and max |h| at the mirrored row, of every class (three classes
    with n odd: class 1 starts at an odd row offset, its first row read on its own)."""
    n = qc.N
    row = {"0": 0, "1": 1, "mid": n // 2, "n-2": n - 2, "n-1": n - 1}[where]
    gs, hs = [], []
    for c in range(num_class):
        g, h = qc.with_maxima(*qc.logistic_gradients(n, c), row, n - 1 - row, scale=1.0 + 0.25 * c)
        gs.append(g)
        hs.append(h)
    g, h = np.concatenate(gs), np.concatenate(hs)
    q = _quantize(n, g, h, {"num_grad_quant_bins": 4, "stochastic_rounding": False}, num_class=num_class)
    _assert_maxima(q, g, h, num_class)


@pytest.mark.parametrize("n", [1, 2, 7])
def test_qmax_tiny(gpu_required, n):
    """Fewer rows than one 16-byte load pair, three classes, the maxima at every row in turn."""
    base_g, base_h = qc.logistic_gradients(64, 9)
    for row in range(n):
        g = np.concatenate([qc.with_maxima(base_g[:n], base_h[:n], row, n - 1 - row, 1.0 + c)[0] for c in range(3)])
        h = np.concatenate([qc.with_maxima(base_g[:n], base_h[:n], row, n - 1 - row, 1.0 + c)[1] for c in range(3)])
        q = _quantize(n, g, h, {"num_grad_quant_bins": 4, "stochastic_rounding": False}, num_class=3)
        _assert_maxima(q, g, h, 3)


def test_qmax_unrolled_loop(gpu_required):
    """n just above 8 * 256 * grid (grid = 4 * CUs): every thread takes the four-deep unrolled
    loop once over rows [0, 8 * 256 * grid), the rest falls to the remainder loop and the odd
    tail row. The maxima inside the unrolled range (a different one of the four loads for g and
    h), then in the remainder."""
    import subprocess
    import sys

    # (torch serves a process together with this library only when it created its context first,
    # tests/test_predict_device.py: the CU count comes from an interpreter of its own)
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    cus = int(r.stdout.strip().splitlines()[-1])
    assert 1 <= cus <= 1024, cus
    stride = 256 * 4 * cus  # 16-byte loads per grid sweep, two rows each
    n = 8 * stride + 200_001
    assert min(-(-n // 256), 4 * cus) == 4 * cus and n > 8 * 256 * 4 * cus
    rng = np.random.default_rng(3)
    base_g = rng.uniform(-1, 1, n).astype(np.float32)
    base_h = rng.uniform(0, 0.25, n).astype(np.float32)
    for g_row, h_row in ((2 * (3 * stride + 12345) + 1, 2 * (1 * stride + 777)), (8 * stride + 4321, n - 1)):
        g, h = qc.with_maxima(base_g, base_h, g_row, h_row)
        q = _quantize(n, g, h, {"num_grad_quant_bins": 4, "stochastic_rounding": False})
        _assert_maxima(q, g, h, 1)


# ------------------------------------------------------------------ deterministic rounding
def _check_deterministic(q, g, h, bins, const_hess=False):
    mg, mh, gs, hs = qc.scales(g, h, bins, const_hess)
    lg, clear_g = qc.deterministic_levels(g, gs)
    lh, clear_h = qc.deterministic_levels(h, hs)
    if const_hess:
        lh, clear_h = np.ones_like(lh), np.ones_like(clear_h)
    clear = clear_g & clear_h
    assert (~clear).sum() <= qc.MAX_TIE_SHARE * g.size, int((~clear).sum())
    got_g, got_h = q["g_level"][0, 0], q["h_level"][0, 0]
    np.testing.assert_array_equal(got_g[clear], lg[clear])
    np.testing.assert_array_equal(got_h[clear], lh[clear])
    np.testing.assert_array_equal(q["packed"][0, 0][clear], qc.packed(lg, lh)[clear])
    # the de-quantized values are the kernel's own levels times the scale, to the bit, in every row
    assert qc.same_bits(q["g"][0, 0], qc.dequantized(got_g, gs))
    assert qc.same_bits(q["h"][0, 0], qc.dequantized(got_h, hs))
    # a row at the tie may go either way, but no further
    assert np.abs(got_g - lg).max() <= 1 and np.abs(got_h - lh).max() <= 1
    return lg, lh


@pytest.mark.parametrize("bins", qc.DETERMINISTIC_BINS)
def test_deterministic_levels(gpu_required, bins):
    n = qc.N
    g, h = qc.with_maxima(*qc.logistic_gradients(n, 0), n // 3, 2 * n // 3)
    g[n // 3 + 1] = -g[n // 3]  # both extreme g levels
    q = _quantize(n, g, h, {"num_grad_quant_bins": bins, "stochastic_rounding": False, "quant_train_renew_leaf": True})
    lg, lh = _check_deterministic(q, g, h, bins)
    assert lg.min() == -(bins // 2) and lg.max() == bins // 2 and lh.max() == bins
    assert q["g_level"].min() == -(bins // 2) and q["g_level"].max() == bins // 2 and q["h_level"].max() == bins
    assert qc.same_bits(q["true_g"][0, 0], g) and qc.same_bits(q["true_h"][0, 0], h)


def test_deterministic_constant_hessian(gpu_required):
    n = qc.N
    g = qc.logistic_gradients(n, 1)[0]
    h = np.full(n, 0.25, dtype=np.float32)
    q = _quantize(n, g, h, {"num_grad_quant_bins": 16, "stochastic_rounding": False}, const_hess=True)
    _check_deterministic(q, g, h, 16, const_hess=True)
    assert np.all(q["h_level"] == 1)
    assert qc.same_bits(q["h"][0, 0], h)


def test_all_zero_gradients(gpu_required):
    n = qc.N
    z = np.zeros(n, dtype=np.float32)
    for stochastic in (False, True):
        q = _quantize(n, z, z, {"num_grad_quant_bins": 16, "stochastic_rounding": stochastic})
        assert np.all(q["packed"] == 0)
        assert qc.same_bits(q["g"][0, 0], z) and qc.same_bits(q["h"][0, 0], z)
        assert q["max_g"][0, 0] == 0 and q["max_h"][0, 0] == 0


# ------------------------------------------------------------------ stochastic rounding
def _residuals(q, r, c, g, h, bins):
    _, _, gs, hs = qc.scales(g, h, bins)
    fg, ug = qc.rounding_residuals(g, q["g_level"][r, c], gs)
    fh, uh = qc.rounding_residuals(h, q["h_level"][r, c], hs)
    assert np.all(q["h_level"][r, c] >= 0)
    assert qc.same_bits(q["g"][r, c], qc.dequantized(q["g_level"][r, c], gs))
    assert qc.same_bits(q["h"][r, c], qc.dequantized(q["h_level"][r, c], hs))
    return fg, ug, fh, uh


@pytest.mark.parametrize("seed", [0, 11])
@pytest.mark.parametrize("bins", qc.STOCHASTIC_BINS)
def test_stochastic_rounding_is_unbiased_and_independent(gpu_required, bins, seed):
    """Two classes holding the same gradients, two rounds: four draws of the same input."""
    n = qc.N
    g, h = qc.logistic_gradients(n, 2)
    p = {"num_grad_quant_bins": bins, "stochastic_rounding": True, "seed": seed}
    q = _quantize(n, np.tile(g, 2), np.tile(h, 2), p, num_class=2, rounds=2)
    stats = {}
    for r in range(2):
        for c in range(2):
            fg, ug, fh, uh = _residuals(q, r, c, g, h, bins)
            for k, z in qc.unbiased_statistics(fg, ug).items():
                stats[f"g r{r} c{c} {k}"] = z
            for k, z in qc.unbiased_statistics(fh, uh).items():
                stats[f"h r{r} c{c} {k}"] = z
            stats[f"g x h r{r} c{c}"] = qc.product_statistic(fg, ug, fh, uh)
            stats[f"g x next g r{r} c{c}"] = qc.product_statistic(fg[:-1], ug[:-1], fg[1:], ug[1:])
            stats[f"h x next h r{r} c{c}"] = qc.product_statistic(fh[:-1], uh[:-1], fh[1:], uh[1:])
            stats[f"h x next g r{r} c{c}"] = qc.product_statistic(fh[:-1], uh[:-1], fg[1:], ug[1:])
    # a later round and another class draw afresh
    for name, (ra, ca, rb, cb) in {"round": (0, 0, 1, 0), "class": (0, 0, 0, 1), "round, class 1": (0, 1, 1, 1)}.items():
        stats[f"g changed by {name}"] = qc.changed_statistic(fg, q["g_level"][ra, ca], q["g_level"][rb, cb])
        stats[f"h changed by {name}"] = qc.changed_statistic(fh, q["h_level"][ra, ca], q["h_level"][rb, cb])
    # another seed draws afresh, the same seed on a fresh learner repeats itself
    other = _quantize(n, np.tile(g, 2), np.tile(h, 2), {**p, "seed": seed + 1}, num_class=2, rounds=1)
    stats["g changed by seed"] = qc.changed_statistic(fg, q["g_level"][0, 0], other["g_level"][0, 0])
    stats["h changed by seed"] = qc.changed_statistic(fh, q["h_level"][0, 0], other["h_level"][0, 0])
    worst = max(stats, key=lambda k: abs(stats[k]))
    print(f"bins={bins} seed={seed}: {len(stats)} statistics, worst {worst} = {stats[worst]:.2f}")
    bad = {k: round(z, 2) for k, z in stats.items() if not abs(z) <= qc.SIGMA}
    assert not bad, bad
    assert not np.array_equal(q["packed"][0, 0], other["packed"][0, 0])
    again = _quantize(n, np.tile(g, 2), np.tile(h, 2), p, num_class=2, rounds=2)
    np.testing.assert_array_equal(again["packed"], q["packed"])


# ------------------------------------------------------------------ k_leaf_true_sums
@pytest.mark.parametrize("engine", ["frontier", "sequential"])
@pytest.mark.parametrize("objective,bins", [("regression", 4), ("regression", 254), ("multiclass", 4)])
def test_renewed_leaves_are_true_newton_steps(lgb, gpu_required, monkeypatch, engine, objective, bins):
    if engine == "sequential":
        monkeypatch.setenv("LGAP_FRONTIER", "0")
    b = qc.check_renewed_leaves(lgb, "gpu", bins, objective=objective)
    assert ("frontier engine" in b.device_name()) == (engine == "frontier"), b.device_name()
