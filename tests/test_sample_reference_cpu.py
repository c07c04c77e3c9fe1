"""sample_cases.bagging_reference / goss_reference against the host sampler (ops.host_sample_rows:
SampleStrategy::Bagging over a Dataset, no GPU): on every case the kept rows, the out-of-bag rows and
the gradient bits are equal. This validates the references before test_sample_kernels.py lets them
judge the HIP kernels. A few values are worked by hand, and the conditions a case is named for
(a draw equal to the fraction, ties above top_k, the GOSS branch taken) are asserted here, where the
reference shows them."""
import functools

import numpy as np
import pytest

import lambdagap_amd as lgb
from lambdagap_amd import ops

import sample_cases as sc


@functools.lru_cache(maxsize=8)
def _dataset(n, labels, queries):
    """A Dataset of n rows; the sampler reads only its row count, labels and query boundaries."""
    x = (np.arange(n, dtype=np.float64) % 7).reshape(n, 1)
    return lgb.Dataset(x, label=np.asarray(labels, dtype=np.float32) if labels is not None else np.zeros(n, np.float32),
                       group=None if queries is None else np.asarray(queries),
                       params={"verbosity": -1, "min_data_in_bin": 1}).construct()


def _host(name):
    c, x = sc.CASES[name], sc.inputs(name)
    ds = _dataset(c["n"], None if x["label"] is None else tuple(x["label"].tolist()),
                  None if x["query_sizes"] is None else tuple(x["query_sizes"].tolist()))
    params, iters = sc.host_params(name)
    return ops.host_sample_rows(ds, params, x["g"], x["h"], iters, c.get("num_class", 1))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_reference_equals_the_host_sampler(name):
    ref = sc.reference(name)
    n = sc.CASES[name]["n"]
    bag, oob, drawn, g, h = _host(name)
    assert ref["kept"].size + ref["oob"].size == n
    if not drawn:
        # bagging_fraction = 1: the host draws no bag and trains on every row
        assert sc.CASES[name].get("fraction") == 1.0 and ref["kept"].size == n and ref["oob"].size == 0
    else:
        assert np.array_equal(bag, ref["kept"])
        assert np.array_equal(oob, ref["oob"])
    assert np.array_equal(sc.bits(g), sc.bits(ref["g"]))
    assert np.array_equal(sc.bits(h), sc.bits(ref["h"]))


def test_first_draws_of_seed_11():
    # 214013 * 11 + 2531011 = 4885154 -> (x >> 16) & 0x7FFF = 74
    x1 = sc.lcg_next(11)
    assert x1 == 4885154 and float(sc.lcg_draw(x1)) == 74 / 32768
    # 214013 * 4885154 + 2531011 = 1045488994013 = 243 * 2^32 + 1811941085 -> 27648
    x2 = sc.lcg_next(x1)
    assert x2 == 1811941085 and float(sc.lcg_draw(x2)) == 27648 / 32768
    # 214013 * 1811941085 + 2531011 = 387778949955116 = 90286 * 2^32 + 3532668460 -> 53904 & 0x7FFF = 21136
    x3 = sc.lcg_next(x2)
    assert x3 == 3532668460 and float(sc.lcg_draw(x3)) == 21136 / 32768
    r = sc.bagging_reference(3, 11, 1, fraction=0.37)
    assert r["draws"].tolist() == [74 / 32768, 27648 / 32768, 21136 / 32768]
    assert r["kept"].tolist() == [0] and r["oob"].tolist() == [1, 2]
    # a one-row block consumes one draw per round: its third round sees the stream's third draw
    assert sc.bagging_reference(1, 11, 3, fraction=0.37)["draws"].tolist() == [21136 / 32768]


def _hash32_by_hand(seed, i):
    m = sc.M32
    x = ((i * 0x9E3779B1) & m) ^ ((seed * 0x85EBCA77 + 0x165667B1) & m)
    x ^= x >> 16
    x = (x * 0x7FEB352D) & m
    x ^= x >> 15
    x = (x * 0x846CA68B) & m
    x ^= x >> 16
    return x


def test_hash_and_seed_of_fixed_inputs():
    # Hash32(0, 0): 0x165667B1, ^ >> 16 -> 0x165671E7, * 0x7FEB352D -> 0xFAD3D89B, ^ >> 15 -> 0xFAD22D3C,
    # * 0x846CA68B -> 0x7EC37794, ^ >> 16 -> 0x7EC30957
    assert int(sc.hash32(0, [0])[0]) == _hash32_by_hand(0, 0) == 0x7EC30957
    # Hash32(1, 2): 2 * 0x9E3779B1 ^ (0x85EBCA77 + 0x165667B1) = 0xA02CC14A, ... -> 0x5992DBE6
    assert int(sc.hash32(1, [2])[0]) == _hash32_by_hand(1, 2) == 0x5992DBE6
    big = sc.hash32(sc.M32, np.array([0, 1, 4095, 4096, 0x7FFFFFFF]))
    assert big.dtype == np.uint32
    assert big.tolist() == [_hash32_by_hand(sc.M32, i) for i in (0, 1, 4095, 4096, 0x7FFFFFFF)]
    # GossSeed(3, 2) = 3 * 0x9E3779B9 + 2 * 0x85EBCA6B mod 2^32
    assert sc.goss_seed(3, 2) == (3 * 0x9E3779B9 + 2 * 0x85EBCA6B) % 2 ** 32 == 0xE67E0201
    assert sc.goss_seed(-1, 0) == 2 ** 32 - 0x9E3779B9
    assert sc.CASES["goss/seed0"]["goss_seed"] == 0 and sc.CASES["goss/seedmax"]["goss_seed"] == sc.M32


def test_goss_tile_of_eight_rows_by_hand():
    """top_rate 0.25, other_rate 0.5 on 8 rows: top_k = 2, other_k = 4, multiplier fp32(6) / 4 = 1.5.
    Importances 8 7 7 1 2 3 4 5: the second largest is 7, so rows 0, 1, 2 are kept unscaled (a tie:
    three rows for top_k = 2); of the five others the four with the smallest keys are scaled by 1.5."""
    g = np.array([8, -7, 7, 1, -2, 3, 4, 5], dtype=np.float32)
    h = np.ones(8, dtype=np.float32)
    seed = 12345
    r = sc.goss_reference(g, h, 1, 0.25, 0.5, seed)
    t = r["tiles"][0]
    assert (t["top_k"], t["other_k"], t["big"], t["rest"], t["branch"]) == (2, 4, 3, 5, "threshold")
    # Hash32(12345, 3 .. 7): row 5 holds the largest key and is the one left out
    keys = [2027853665, 126511961, 3837652618, 2797628325, 2928705559]
    assert [_hash32_by_hand(seed, i) for i in range(3, 8)] == keys
    assert r["kept"].tolist() == [0, 1, 2, 3, 4, 6, 7] and r["oob"].tolist() == [5]
    assert r["g"].tolist() == [8, -7, 7, 1.5, -3, 3, 6, 7.5]
    assert r["h"].tolist() == [1, 1, 1, 1.5, 1.5, 1, 1.5, 1.5]


def test_a_draw_equal_to_the_fraction_is_not_kept():
    c, r = sc.CASES["bag/big"], sc.reference("bag/big")
    at = np.flatnonzero(r["draws"] == c["fraction"])
    print("rows whose draw equals the fraction:", at.size)
    assert at.size >= 10
    assert not r["keep"][at].any() and np.isin(at, r["oob"]).all()
    assert c["n"] > 256 * sc.TILE  # the scatter's prefix loop loops again from tile 256 on


def test_small_fraction_leaves_tiles_and_a_whole_bag_empty():
    for r in (1, 2):
        assert sc.reference(f"bag/few/n255/r{r}")["kept"].size == 0
    n = 2 * sc.TILE + sc.BLOCK + 1
    kept = sc.reference(f"bag/few/n{n}/r1")["kept"]
    per_tile = np.bincount(kept // sc.TILE, minlength=3)
    assert kept.size > 0 and (per_tile == 0).any(), per_tile
    for name in ("bag/all/n1", "bag/all/n4097"):
        assert sc.reference(name)["oob"].size == 0


def test_balanced_label_rule_is_label_above_zero():
    name = f"balanced/pos1/n{2 * sc.TILE + sc.BLOCK + 1}"
    x, r = sc.inputs(name), sc.reference(name)
    lab = x["label"]
    assert (lab == 0).any() and (lab < 0).any() and (lab > 0).any()
    assert r["keep"][lab > 0].all()  # pos_fraction = 1 keeps every positive row
    assert 0 < r["keep"][lab <= 0].sum() < 0.05 * (lab <= 0).sum()


def test_query_cases_have_the_named_shapes():
    s = sc.inputs("query/mixed/r3")["query_sizes"]
    b = np.concatenate([[0], np.cumsum(s)])
    assert s.size == 1030 and s[0] == 1 and s.max() > sc.TILE
    straddle = [(q, b[q], b[q + 1]) for q in range(s.size) if b[q] // sc.TILE != (b[q + 1] - 1) // sc.TILE]
    assert any(s[q] <= 8 for q, _, _ in straddle), straddle  # a short query across a tile boundary
    assert sc.inputs("query/exact/r3")["query_sizes"].size == sc.BLOCK
    # all rows of a query share its fate, and both fates occur
    r = sc.reference("query/mixed/r3")
    keep_q = [r["keep"][b[q]:b[q + 1]] for q in range(s.size)]
    assert all(k.all() or not k.any() for k in keep_q)
    assert 0 < sum(bool(k[0]) for k in keep_q) < s.size


@pytest.mark.parametrize("name", list(sc.GOSS_BRANCHES))
def test_goss_cases_take_their_branches(name):
    taken = {t["branch"] for t in sc.reference(name)["tiles"]}
    assert sc.GOSS_BRANCHES[name] <= taken, taken


@pytest.mark.parametrize("name", sc.GOSS_TIES)
def test_goss_tie_cases_keep_more_than_top_k(name):
    t = sc.reference(name)["tiles"][0]
    assert t["big"] > t["top_k"], t


def test_goss_named_cases():
    t = sc.reference("goss/tie_top")["tiles"][0]
    assert (t["big"], t["rest"], t["sampled"], t["branch"]) == (4000, 96, 96, "all") and t["other_k"] >= t["rest"]
    t = sc.reference("goss/half/n4096/k1")["tiles"][0]
    assert t["branch"] == "all" and t["cnt"] - t["top_k"] == t["other_k"]  # multiplier exactly 1
    t = sc.reference("goss/half/n1001/k1")["tiles"][0]
    assert (t["other_k"], t["rest"], t["sampled"]) == (500, 501, 500)
    assert sc.reference("goss/top1/n4097")["tiles"][0]["top_k"] == 1
    assert sc.reference(f"goss/n{sc.TILE + 9}/k1")["tiles"][1]["cnt"] == 9
    assert sc.reference("goss/n4097/k1")["tiles"][1]["cnt"] == 1
    # subnormal importances, some of them zero
    imp = sc.reference("goss/subnormal/k1")["importance"]
    tiny = np.finfo(np.float32).tiny
    assert ((imp > 0) & (imp < tiny)).sum() > 3000 and (imp == 0).any()
    # the two-value, low-digit and exponent cases differ where they say
    b = sc.reference("goss/two_values")["importance"].view(np.uint32)
    assert set(np.unique(b)) == {0x3F800000, 0x3F800001}
    b = sc.reference("goss/low_digit")["importance"].view(np.uint32)
    assert np.unique(b >> 8).size == 1 and np.unique(b & 0xFF).size > 200
    b = sc.reference("goss/exponent")["importance"].view(np.uint32)
    assert not (b & 0x7FFFFF).any() and np.unique(b >> 23).size > 200
    # -0.0 stays -0.0 in the all-zero case
    r, x = sc.reference("goss/zeros/k1"), sc.inputs("goss/zeros/k1")
    assert np.signbit(x["g"]).any() and np.array_equal(sc.bits(r["g"]), sc.bits(x["g"]))


def test_two_seeds_share_the_top_set_and_differ_in_the_sample():
    a, b = sc.reference("goss/seed0"), sc.reference("goss/seedmax")
    assert np.array_equal(sc.inputs("goss/seed0")["g"], sc.inputs("goss/seedmax")["g"])
    assert np.array_equal(a["tiles"][0]["top"], b["tiles"][0]["top"])
    assert a["tiles"][0]["picked"].size == b["tiles"][0]["picked"].size == a["tiles"][0]["other_k"]
    assert not np.array_equal(a["tiles"][0]["picked"], b["tiles"][0]["picked"])
