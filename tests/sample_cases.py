"""References and cases of the row sampling tests (no GPU code here).

test_sample_reference_cpu.py checks the references below against the host sampler
(ops.host_sample_rows: SampleStrategy::Bagging), test_sample_kernels.py lets them judge the HIP
kernels k_sample_count / k_sample_scatter / k_sample_advance_units (ops.device_sample_test). Every
comparison is exact: row lists and gradient bits.

The references are written from the definitions, in numpy and Python integers.

Bagging (the reference project's bagging.hpp): the units (rows, or queries when bagging by query)
are cut into blocks of 1024. Block b owns the LCG x <- 214013 x + 2531011 (mod 2^32) started at
bagging_seed + b and stepped once per unit, in unit order, in every round; so unit i consumes the
(i % 1024 + 1)-th draw its block makes in that round, and a round moves a block on by exactly its
unit count. A draw is float32(((x >> 16) & 0x7FFF) / 32768); the unit is kept if the draw, as a
float64, is < the fraction (balanced: pos_fraction where label > 0, neg_fraction elsewhere). All
rows of a query share the query's draw.

GOSS (goss.hpp, with this project's documented deviation: fixed 4096-row tiles, and the rest is
sampled by the other_k smallest Hash32(seed, row) keys instead of a sequential scan). Per tile of
cnt rows: importance = fp32 running sum over the classes, in class order, of |fp32(g * h)|; top_k =
max(1, int(cnt * top_rate)), other_k = int(cnt * other_rate); every row whose importance is >= the
top_k-th largest is kept unscaled; of the rest none are kept (other_k == 0 or no rest), all of them
(other_k >= their number) or those whose key is <= the other_k-th smallest key among them; the rows
so sampled have g and h of every class multiplied in fp32 by fp32(cnt - top_k) / other_k.
"""
import functools
import math

import numpy as np

TILE = 4096    # rows per GOSS tile
BLOCK = 1024   # units per bagging stream
M32 = 0xFFFFFFFF
F32 = np.float32


# ---------------------------------------------------------------------------------------------
# integer pieces

def lcg_next(x):
    """One step of the bagging LCG on a Python integer state."""
    return (214013 * x + 2531011) & M32


def lcg_draw(x):
    """The float32 draw of a state (after the step)."""
    return F32((x >> 16) & 0x7FFF) / F32(32768.0)


def hash32(seed, rows):
    """Hash32(seed, row) for an array of rows, in uint32 arithmetic (wrapping)."""
    with np.errstate(over="ignore"):
        i = np.atleast_1d(np.asarray(rows, dtype=np.uint32))
        s = np.atleast_1d(np.asarray(seed & M32, dtype=np.uint32))
        x = (i * np.uint32(0x9E3779B1)) ^ (s * np.uint32(0x85EBCA77) + np.uint32(0x165667B1))
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846CA68B)
        x = x ^ (x >> np.uint32(16))
    return x


def goss_seed(bagging_seed, it):
    """GossSeed(bagging_seed, iter): uint32(bagging_seed) * 0x9E3779B9 + uint32(iter) * 0x85EBCA6B."""
    with np.errstate(over="ignore"):
        b = np.atleast_1d(np.asarray(bagging_seed & M32, dtype=np.uint32))
        i = np.atleast_1d(np.asarray(it & M32, dtype=np.uint32))
        return int((b * np.uint32(0x9E3779B9) + i * np.uint32(0x85EBCA6B))[0])


def bagging_seed_for(target, it):
    """The int32 bagging_seed whose GossSeed at iteration `it` is `target`."""
    b = ((target - it * 0x85EBCA6B) * pow(0x9E3779B9, -1, 1 << 32)) & M32
    b = b - (1 << 32) if b >= (1 << 31) else b
    assert goss_seed(b, it) == target
    return b


# ---------------------------------------------------------------------------------------------
# references

def bagging_reference(n, seed, rounds, fraction=1.0, label=None, pos_fraction=1.0, neg_fraction=1.0,
                      query_sizes=None):
    """The bag of the last of `rounds` rounds. `label` given: balanced bagging. `query_sizes` given:
    one draw per query. Returns kept / oob (ascending int32), the keep mask and the rows' draws."""
    units = n if query_sizes is None else len(query_sizes)
    nb = (units + BLOCK - 1) // BLOCK
    state = ((seed + np.arange(nb, dtype=np.int64)) & M32).astype(np.uint64)
    per = np.minimum(BLOCK, units - BLOCK * np.arange(nb))
    draws = None
    for _ in range(rounds):
        draws = np.full((nb, BLOCK), np.nan, dtype=np.float32)
        for j in range(BLOCK):
            live = per > j  # a block makes exactly one draw per unit it holds
            if not live.any():
                break
            s = (np.uint64(214013) * state[live] + np.uint64(2531011)) & np.uint64(M32)
            state[live] = s
            draws[live, j] = ((s >> np.uint64(16)) & np.uint64(0x7FFF)).astype(np.float32) / F32(32768.0)
    r = draws.reshape(-1)[:units].astype(np.float64)
    assert not np.isnan(r).any()
    if query_sizes is not None:
        r = np.repeat(r, np.asarray(query_sizes, dtype=np.int64))
        assert r.size == n
    if label is not None:
        keep = np.where(np.asarray(label) > 0, r < float(pos_fraction), r < float(neg_fraction))
    else:
        keep = r < float(fraction)
    rows = np.arange(n, dtype=np.int32)
    return {"kept": rows[keep], "oob": rows[~keep], "keep": keep, "draws": r}


def goss_reference(g, h, num_class, top_rate, other_rate, seed):
    """One GOSS pass over class-major g / h [num_class * n]. Returns kept / oob (ascending int32),
    the scaled g / h, and per tile (branch, top_k, other_k, big, rest, sampled, top set, sampled set)."""
    g = np.array(g, dtype=np.float32).reshape(num_class, -1)
    h = np.array(h, dtype=np.float32).reshape(num_class, -1)
    n = g.shape[1]
    imp = np.zeros(n, dtype=np.float32)
    for k in range(num_class):
        imp = (imp + np.abs((g[k] * h[k]).astype(np.float32))).astype(np.float32)
    keep = np.zeros(n, dtype=bool)
    tiles = []
    for start in range(0, n, TILE):
        cnt = min(TILE, n - start)
        rows = np.arange(start, start + cnt)
        v = imp[start:start + cnt]
        top_k = max(1, int(cnt * top_rate))
        other_k = int(cnt * other_rate)
        thr = np.sort(v)[::-1][top_k - 1]
        big = v >= thr
        rest_rows = rows[~big]
        rest = rest_rows.size
        branch, sampled = "none", rest_rows[:0]
        if other_k > 0 and rest > 0:
            if other_k >= rest:
                branch, sampled = "all", rest_rows
            else:
                keys = hash32(seed, rest_rows)
                kthr = np.sort(keys)[other_k - 1]
                branch, sampled = "threshold", rest_rows[keys <= kthr]
        keep[rows[big]] = True
        keep[sampled] = True
        if sampled.size:
            mul = F32(cnt - top_k) / F32(other_k)
            g[:, sampled] = (g[:, sampled] * mul).astype(np.float32)
            h[:, sampled] = (h[:, sampled] * mul).astype(np.float32)
        tiles.append({"branch": branch, "cnt": cnt, "top_k": top_k, "other_k": other_k, "big": int(big.sum()),
                      "rest": int(rest), "sampled": int(sampled.size), "top": rows[big], "picked": sampled})
    rows = np.arange(n, dtype=np.int32)
    return {"kept": rows[keep], "oob": rows[~keep], "g": g.reshape(-1), "h": h.reshape(-1), "tiles": tiles,
            "importance": imp}


# ---------------------------------------------------------------------------------------------
# cases

BIG = 257 * TILE + 5  # the tile-prefix loop of the scatter takes a second trip from tile 256 on
BAG_ROWS = [1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 2 * TILE + BLOCK + 1]
ROUNDS = [1, 2, 5]
FEW = 2e-4  # keeps the draws 0 .. 6 of 32768: about 0.9 rows per tile


def _bagging_cases():
    c = {}
    for n in BAG_ROWS:
        for r in ROUNDS:
            c[f"bag/n{n}/r{r}"] = dict(mode="bagging", n=n, rounds=r, fraction=0.37, seed=11)
            c[f"balanced/mixed/n{n}/r{r}"] = dict(mode="balanced", n=n, rounds=r, pos=0.9, neg=0.2, seed=5,
                                                  labels="mixed")
    for n in (1, 1024, 4097, 2 * TILE + BLOCK + 1):
        c[f"bag/all/n{n}"] = dict(mode="bagging", n=n, rounds=1, fraction=1.0, seed=11)
    for n in (255, 4097, 2 * TILE + BLOCK + 1):
        for r in (1, 2):
            c[f"bag/few/n{n}/r{r}"] = dict(mode="bagging", n=n, rounds=r, fraction=FEW, seed=11)
    for labels in ("positive", "negative"):
        for n in (1025, 2 * TILE + BLOCK + 1):
            c[f"balanced/{labels}/n{n}"] = dict(mode="balanced", n=n, rounds=2, pos=0.9, neg=0.2, seed=5,
                                                labels=labels)
    for n in (1, 2 * TILE + BLOCK + 1):
        c[f"balanced/pos1/n{n}"] = dict(mode="balanced", n=n, rounds=2, pos=1.0, neg=0.01, seed=5, labels="mixed")
    # about BIG / 32768 = 32 rows draw exactly 16384 / 32768 = the fraction, and are not kept
    c["bag/big"] = dict(mode="bagging", n=BIG, rounds=1, fraction=0.5, seed=11)
    return c


def _query_sizes(kind):
    rng = np.random.default_rng(77)
    if kind == "mixed":
        # 1030 queries: a second stream and a partial last stream block; the first query one row,
        # query 400 longer than a tile, and (asserted by the CPU test) queries that straddle tiles
        s = rng.integers(1, 8, 1030)
        s[0] = 1
        s[400] = TILE + 904
        s[1029] = 1
        return s.astype(np.int32)
    if kind == "exact":
        return rng.integers(1, 4, BLOCK).astype(np.int32)  # exactly one full stream block
    raise KeyError(kind)


def _query_cases():
    c = {}
    for kind in ("mixed", "exact"):
        for r in (1, 3):
            c[f"query/{kind}/r{r}"] = dict(mode="query", queries=kind, n=int(_query_sizes(kind).sum()), rounds=r,
                                           fraction=0.5, seed=9)
    return c


GOSS_ROWS = [1, 9, 10, 255, 4095, 4096, 4097, TILE + 9]
GOSS_IT = 1  # with learning_rate = 1 the host samples from iteration 1 on


def _goss(n, k, top, other, data="normal", target=None, bs=7):
    if target is not None:
        bs = bagging_seed_for(target, GOSS_IT)
    return dict(mode="goss", n=n, num_class=k, top=top, other=other, data=data, bagging_seed=bs, it=GOSS_IT,
                goss_seed=goss_seed(bs, GOSS_IT))


def _goss_cases():
    c = {}
    for n in GOSS_ROWS:
        for k in (1, 3):
            c[f"goss/n{n}/k{k}"] = _goss(n, k, 0.2, 0.1)
    # (0.5, 0.5): every rest row at 4096 rows (multiplier 1), 500 of 501 by the key threshold at 1001
    for n in (10, 1001, 4096, 4097):
        c[f"goss/half/n{n}/k1"] = _goss(n, 1, 0.5, 0.5)
    c["goss/half/n1001/k3"] = _goss(1001, 3, 0.5, 0.5)
    c["goss/big"] = _goss(BIG, 1, 0.2, 0.1)
    c["goss/top1/n4097"] = _goss(4097, 1, 1e-4, 0.1)  # cnt * top_rate < 1: top_k = 1
    for k in (1, 3):
        c[f"goss/zeros/k{k}"] = _goss(4097, k, 0.2, 0.1, "zeros")
        c[f"goss/subnormal/k{k}"] = _goss(4097, k, 0.2, 0.1, "subnormal")
    c["goss/tie_top"] = _goss(TILE, 1, 0.2, 0.1, "tie_top")
    c["goss/two_values"] = _goss(4097, 1, 0.2, 0.1, "two_values")
    c["goss/low_digit"] = _goss(4097, 1, 0.2, 0.1, "low_digit")
    c["goss/exponent"] = _goss(4097, 1, 0.2, 0.1, "exponent")
    c["goss/seed0"] = _goss(4097, 1, 0.2, 0.1, target=0)
    c["goss/seedmax"] = _goss(4097, 1, 0.2, 0.1, target=M32)
    return c


BAGGING_CASES = _bagging_cases()
QUERY_CASES = _query_cases()
GOSS_CASES = _goss_cases()
CASES = {**BAGGING_CASES, **QUERY_CASES, **GOSS_CASES}

# what only the reference can show about a case (test_sample_reference_cpu.py asserts it)
GOSS_BRANCHES = {
    "goss/n1/k1": {"none"}, "goss/n9/k1": {"none"}, "goss/n10/k1": {"threshold"},
    f"goss/n{TILE + 9}/k1": {"threshold", "none"}, f"goss/n{TILE + 9}/k3": {"threshold", "none"},
    "goss/half/n4096/k1": {"all"}, "goss/half/n1001/k1": {"threshold"}, "goss/half/n1001/k3": {"threshold"},
    "goss/half/n4097/k1": {"all", "none"}, "goss/half/n10/k1": {"all"}, "goss/tie_top": {"all"}, "goss/zeros/k1": {"none"},
    "goss/zeros/k3": {"none"}, "goss/big": {"threshold"}, "goss/two_values": {"threshold"},
}
GOSS_TIES = ["goss/tie_top", "goss/two_values", "goss/zeros/k1", "goss/zeros/k3"]  # big > top_k


def _frozen(a):
    if a is not None:
        a.setflags(write=False)
    return a


def _goss_data(kind, n, k):
    rng = np.random.default_rng([n, k, sum(map(ord, kind))])  # the data does not depend on the seed
    if kind == "normal":
        g = rng.standard_normal(k * n).astype(np.float32)
        h = (rng.random(k * n) + 0.1).astype(np.float32)
    elif kind == "zeros":
        g = np.where(rng.random(k * n) < 0.5, 0.0, -0.0).astype(np.float32)
        h = (rng.random(k * n) + 0.1).astype(np.float32)
        h[::7] = -0.0
    elif kind == "subnormal":
        # products around 1e-40, under the smallest normal fp32 (1.18e-38); some round to zero
        g = (rng.standard_normal(k * n) * 1e-20).astype(np.float32)
        h = (rng.random(k * n) * 1e-20).astype(np.float32)
        h[rng.random(k * n) < 0.05] = 1e-26
    elif kind == "tie_top":
        # 4000 rows tied at the top value, 96 below it: big = 4000 > top_k, other_k >= rest
        assert n == TILE and k == 1
        g = np.full(n, 2.0, dtype=np.float32)
        low = rng.choice(n, 96, replace=False)
        g[low] = rng.random(96).astype(np.float32) + 0.25
        h = np.ones(n, dtype=np.float32)
    elif kind == "two_values":
        # importances 1 and 1 + 2^-23 only: they differ in the last mantissa bit
        bits = np.uint32(0x3F800000) + rng.integers(0, 2, k * n).astype(np.uint32)
        g, h = bits.view(np.float32).copy(), np.ones(k * n, dtype=np.float32)
    elif kind == "low_digit":
        # importances in [1, 1 + 255 * 2^-23]: only the lowest radix digit (mantissa byte) differs
        bits = np.uint32(0x3F800000) + rng.integers(0, 256, k * n).astype(np.uint32)
        g, h = bits.view(np.float32).copy(), np.ones(k * n, dtype=np.float32)
    elif kind == "exponent":
        # powers of two from 2^-126 to 2^127: only the exponent differs
        bits = rng.integers(1, 255, k * n).astype(np.uint32) << np.uint32(23)
        g, h = bits.view(np.float32).copy(), np.ones(k * n, dtype=np.float32)
        g[::2] = -g[::2]
    else:
        raise KeyError(kind)
    return g, h


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The (read-only) inputs of a case: g, h (class-major float32), label, query_sizes."""
    c = CASES[name]
    n = c["n"]
    label = sizes = None
    if c["mode"] == "goss":
        g, h = _goss_data(c["data"], n, c["num_class"])
    else:
        rng = np.random.default_rng(n)
        g = rng.standard_normal(n).astype(np.float32)
        h = np.ones(n, dtype=np.float32)
        if c["mode"] == "balanced":
            label = {"mixed": rng.integers(-1, 3, n), "positive": rng.integers(1, 4, n),
                     "negative": -rng.integers(0, 3, n)}[c["labels"]].astype(np.float32)
        if c["mode"] == "query":
            sizes = _query_sizes(c["queries"])
    return {"g": _frozen(g), "h": _frozen(h), "label": _frozen(label), "query_sizes": _frozen(sizes)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The (read-only) reference result of a case: kept, oob, g, h and the reference's own detail."""
    c, x = CASES[name], inputs(name)
    if c["mode"] == "goss":
        r = goss_reference(x["g"], x["h"], c["num_class"], c["top"], c["other"], c["goss_seed"])
    else:
        r = bagging_reference(c["n"], c["seed"], c["rounds"], c.get("fraction", 1.0), x["label"], c.get("pos", 1.0),
                              c.get("neg", 1.0), x["query_sizes"])
        r["g"], r["h"] = x["g"], x["h"]  # bagging leaves the gradients alone
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def device_kwargs(name):
    """Arguments of ops.device_sample_test for a case."""
    c, x = CASES[name], inputs(name)
    kw = dict(mode=c["mode"], grad=x["g"], hess=x["h"], label=x["label"], query_sizes=x["query_sizes"],
              rounds=c.get("rounds", 1), oob=True)
    if c["mode"] == "goss":
        kw.update(num_class=c["num_class"], top_rate=c["top"], other_rate=c["other"], goss_seed=c["goss_seed"])
    else:
        kw.update(fraction=c.get("fraction", 1.0), pos_fraction=c.get("pos", 1.0), neg_fraction=c.get("neg", 1.0),
                  bagging_seed=c["seed"])
    return kw


def host_params(name):
    """(parameters, iterations) that make the host SampleStrategy draw the case."""
    c = CASES[name]
    if c["mode"] == "goss":
        # learning_rate 1: GOSS samples from iteration int(1 / learning_rate) = 1 on
        return ({"data_sample_strategy": "goss", "top_rate": repr(c["top"]), "other_rate": repr(c["other"]),
                 "bagging_seed": c["bagging_seed"], "learning_rate": 1.0, "verbosity": -1}, [c["it"]])
    p = {"bagging_freq": 1, "bagging_seed": c["seed"], "verbosity": -1}
    if c["mode"] == "balanced":
        p.update(pos_bagging_fraction=repr(c["pos"]), neg_bagging_fraction=repr(c["neg"]))
    else:
        p.update(bagging_fraction=repr(c["fraction"]))
    if c["mode"] == "query":
        p["bagging_by_query"] = True
    return p, list(range(c["rounds"]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


assert math.isclose(FEW * 32768, 6.5536)
