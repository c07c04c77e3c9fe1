"""Cases and the extended-precision numpy reference of the linear-leaf Gram systems, shared by
test_linear_gram_reference_cpu.py (the host linear learner, device_type=cpu) and
test_linear_gram_kernel.py (k_linear_gram<1|2|4> and k_linear_fold,
src/device/linear_kernels.hip, through ops.linear_gram).

Per leaf with rows R and sorted features f_0 .. f_{k-1} (m = k + 1 unknowns):

    kept rows   those of R without a NaN in any of the leaf's features
    X1 = [raw[kept][:, feats], 1]          A = X1' diag(h) X1  (m x m)          c = X1' g  (m)
    usable      the sum over R of the number of non-NaN values before the row's first NaN
                (k for a clean row), SolveLeaf's count in src/learner/linear_tree_learner.cpp

accumulated in np.longdouble. The kernel's 64 x 64 slot holds A in rows / columns [0, m) and c in
column m. This module imports no library; data and references are built once per process.

Kernel shapes the sizes are chosen around: one MFMA takes four rows, a block's four waves take
sixteen per sweep (row counts 0, 1, 3, 4, 5, 15, 16, 17, 64 and two long ones); a leaf's rows are
cut into `chunks` blocks (some empty when chunks exceeds the rows); the tile count is chosen by the
widest leaf of the launch: [A | c] has m + 1 columns, so k <= 14 runs one 16-wide tile per
dimension, k = 15 .. 30 two and k = 31 .. 62 four.
"""
import functools

import numpy as np

N, F = 6000, 70
DIM = 64
ROW_COUNTS = (0, 1, 3, 4, 5, 15, 16, 17, 64, 1000, 4097)
CHUNKS = (1, 3, 8)
GROUPS = {"one_tile": (0, 1, 14), "two_tiles": (15, 16, 30), "four_tiles": (31, 47, 62)}
CLEAN_ROWS = range(5800, N)  # rows without random NaNs, handed out to the leaves' special rows
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def data():
    """(raw [N, F] float32, g, h float32): columns scaled by 1e3 (every 7th from 1) and 1e-3
    (every 7th from 4), 2 % NaN outside CLEAN_ROWS, h >= 0 with a tenth exact zeros, g signed."""
    rng = np.random.default_rng(2024)
    raw = rng.standard_normal((N, F))
    raw[:, 1::7] *= 1e3
    raw[:, 4::7] *= 1e-3
    raw = raw.astype(np.float32)
    nan = rng.random((N, F)) < 0.02
    nan[CLEAN_ROWS.start:] = False
    raw[nan] = np.nan
    g = rng.standard_normal(N).astype(np.float32)
    h = rng.uniform(0.0, 1.0, N).astype(np.float32)
    h[rng.random(N) < 0.1] = 0.0
    return raw, g, h


def _build():
    """The leaves of every group: (k, rows, feats), rows an int32 array (a row list) or a range
    (contiguous rows). Row-list leaves of at least four rows and one feature start with three
    rows of their own from CLEAN_ROWS whose only NaN sits in the leaf's first feature, in its
    last feature and in a column the leaf does not use (that row stays in the system). Every leaf
    ends in rows that count (no NaN in its features, h > 0), so that a lost tail row shows."""
    raw, g, h = (a.copy() for a in data())
    rng = np.random.default_rng(7)
    special = iter(CLEAN_ROWS)
    groups = {}
    for name, ks in GROUPS.items():
        leaves = []
        for k in ks:
            for j, cnt in enumerate(ROW_COUNTS):
                feats = np.sort(rng.choice(F, size=k, replace=False)).astype(np.int32)
                if (j + k) % 2 == 0:
                    # (a range that ends in a row that counts: no NaN in the leaf's features, h > 0)
                    for _ in range(1000):
                        start = int(rng.integers(0, CLEAN_ROWS.start - cnt + 1))
                        last = start + cnt - 1
                        if cnt == 0 or (h[last] > 0 and not np.isnan(raw[last, feats]).any()):
                            break
                    rows = range(start, start + cnt)
                else:
                    rows = rng.choice(CLEAN_ROWS.start, size=cnt, replace=False).astype(np.int32)
                    # the list ends in rows that count: no NaN in the leaf's features, h > 0
                    ok = np.flatnonzero(~np.isnan(raw[:CLEAN_ROWS.start][:, feats]).any(axis=1) &
                                        (h[:CLEAN_ROWS.start] > 0))
                    ok = np.setdiff1d(ok, rows)[:min(3, cnt)]
                    rows[cnt - ok.size:] = ok
                    if cnt >= 4 and 1 <= k < F:
                        unused = int(np.setdiff1d(np.arange(F), feats)[0])
                        for slot, col in enumerate((int(feats[0]), int(feats[-1]), unused)):
                            r = next(special)
                            raw[r, col] = np.nan
                            rows[slot] = r
                leaves.append((k, rows, feats))
        groups[name] = leaves
    # one launch in which leaves without features and with 15 ride in the four-tile kernel
    groups["mixed"] = [lf for name in ("one_tile", "two_tiles", "four_tiles") for lf in groups[name]
                       if lf[0] in (0, 15, 62)]
    for a in (raw, g, h):
        a.setflags(write=False)
    return (raw, g, h), groups


@functools.lru_cache(maxsize=None)
def cases():
    """((raw, g, h), {group: [(k, rows, feats)]}) with the special rows' NaNs placed in raw."""
    return _build()


def gram_reference(raw, g, h, rows, feats):
    """(A [m, m], c [m], usable, bound_A [m, m], bound_c [m]) in np.longdouble: the system and
    sum_i |h_i x_ia x_ib|, sum_i |g_i x_ia| over the kept rows."""
    rows = np.asarray(rows, dtype=np.int64)
    feats = np.asarray(feats, dtype=np.int64)
    k = feats.size
    x = raw[np.ix_(rows, feats)] if k else np.zeros((rows.size, 0), dtype=np.float32)
    isnan = np.isnan(x)
    has = isnan.any(axis=1) if k else np.zeros(rows.size, dtype=bool)
    first = np.where(has, isnan.argmax(axis=1), k) if k else np.zeros(rows.size, dtype=np.int64)
    usable = int(first.sum())
    keep = ~has
    X1 = np.concatenate([x[keep].astype(np.longdouble), np.ones((int(keep.sum()), 1), dtype=np.longdouble)], axis=1)
    hh = h[rows][keep].astype(np.longdouble)[:, None]
    gg = g[rows][keep].astype(np.longdouble)[:, None]
    A = X1.T @ (hh * X1)
    c = (X1 * gg).sum(axis=0)
    bound_A = np.abs(X1).T @ (np.abs(hh) * np.abs(X1))
    bound_c = (np.abs(X1) * np.abs(gg)).sum(axis=0)
    return A, c, usable, bound_A, bound_c


@functools.lru_cache(maxsize=None)
def group_reference(name):
    (raw, g, h), groups = cases()
    return [gram_reference(raw, g, h, rows, feats) for _, rows, feats in groups[name]]


def check_slot(out, usable, ref, n_rows, k, label=""):
    """One leaf's 64 x 64 slot against its reference. Every element of A and c within
    4 (n + 4) 2^-53 sum_i |terms|: the any-order summation bound (n - 1 additions, each term a
    product rounded once or fused), doubled for the fold over chunks and waves; n the leaf's row
    count. Nothing absolute: an element whose bound is 0 must be exactly 0, as everything outside
    rows [0, m) and columns [0, m]."""
    A, c, want_usable, bA, bc = ref
    m = k + 1
    assert out.shape == (DIM, DIM)
    assert int(usable) == want_usable, (label, int(usable), want_usable)
    got = out.astype(np.longdouble)
    factor = np.longdouble(4 * (n_rows + 4) * U)
    errA = np.abs(got[:m, :m] - A)
    errc = np.abs(got[:m, m] - c)
    badA = np.argwhere(errA > factor * bA)
    badc = np.flatnonzero(errc > factor * bc)
    assert badA.size == 0, (label, "A", badA[:4].tolist(), [float(errA[tuple(i)]) for i in badA[:4]],
                            [float(factor * bA[tuple(i)]) for i in badA[:4]])
    assert badc.size == 0, (label, "c", badc[:4].tolist(), errc[badc[:4]].astype(float).tolist())
    pad = out.copy()
    pad[:m, :m + 1] = 0.0
    assert not pad.any(), (label, "outside the system", np.argwhere(pad != 0)[:4].tolist())


def worst_ratio(out, ref, n_rows, k):
    """max error / bound over the slot's elements with a non-zero bound (for reporting)."""
    A, c, _, bA, bc = ref
    m = k + 1
    got = out.astype(np.longdouble)
    factor = np.longdouble(4 * (n_rows + 4) * U)
    r = [0.0]
    if (bA > 0).any():
        r.append(float((np.abs(got[:m, :m] - A)[bA > 0] / (factor * bA[bA > 0])).max()))
    if (bc > 0).any():
        r.append(float((np.abs(got[:m, m] - c)[bc > 0] / (factor * bc[bc > 0])).max()))
    return max(r)
