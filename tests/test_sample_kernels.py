"""k_sample_count, k_sample_scatter and k_sample_advance_units (src/device/sample_kernels.hip) against
the references of sample_cases.py, bit for bit: ops.device_sample_test runs the production launches
over host arrays, with the out-of-bag list, with bagging by query, and with both index buffers filled
with -1 beforehand and returned whole. On every case the kept rows, the out-of-bag rows, the count
and the int32 views of g and h equal the reference, nothing is written past the counts, and a second
run repeats the first. test_sample_reference_cpu.py checks the same references against the host
sampler, so the device equals the host on every case as well."""
import numpy as np
import pytest

import sample_cases as sc

pytestmark = pytest.mark.gpu


def _run(name):
    from lambdagap_amd import ops

    return ops.device_sample_test(**sc.device_kwargs(name))


def _check(name):
    ref = sc.reference(name)
    n = sc.CASES[name]["n"]
    out, oob, total, g, h = _run(name)
    assert out.size == n and oob.size == n
    assert total == ref["kept"].size
    assert np.array_equal(out[:total], ref["kept"])
    assert np.array_equal(oob[:n - total], ref["oob"])
    assert np.array_equal(out[total:], np.full(n - total, -1, dtype=np.int32)), "written past the kept count"
    assert np.array_equal(oob[n - total:], np.full(total, -1, dtype=np.int32)), "written past the out-of-bag count"
    assert np.array_equal(sc.bits(g), sc.bits(ref["g"]))
    assert np.array_equal(sc.bits(h), sc.bits(ref["h"]))
    out2, oob2, total2, g2, h2 = _run(name)
    assert total2 == total and np.array_equal(out2, out) and np.array_equal(oob2, oob)
    assert np.array_equal(sc.bits(g2), sc.bits(g)) and np.array_equal(sc.bits(h2), sc.bits(h))


@pytest.mark.parametrize("name", list(sc.BAGGING_CASES))
def test_bagging(gpu_required, name):
    _check(name)


@pytest.mark.parametrize("name", list(sc.QUERY_CASES))
def test_bagging_by_query(gpu_required, name):
    _check(name)


@pytest.mark.parametrize("name", list(sc.GOSS_CASES))
def test_goss(gpu_required, name):
    _check(name)


def test_without_the_out_of_bag_list(gpu_required):
    """The learner passes no out-of-bag list unless the frontier walks it: the bag is the same."""
    from lambdagap_amd import ops

    for name in ("bag/n4097/r2", "goss/n4097/k3"):
        ref = sc.reference(name)
        out, oob, total, g, _ = ops.device_sample_test(**{**sc.device_kwargs(name), "oob": False})
        assert oob is None and total == ref["kept"].size
        assert np.array_equal(out[:total], ref["kept"]) and (out[total:] == -1).all()
        assert np.array_equal(sc.bits(g), sc.bits(ref["g"]))
