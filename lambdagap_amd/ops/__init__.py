"""Kernel-level entry points of the native library.

These expose single HIP kernels (histogram construction, gradients) and the
packed bin layout they consume, so numerics can be checked against a plain
PyTorch / NumPy reference of the same op (tests/test_gpu_kernels.py).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from ..basic import _LIB, Booster, Dataset, _check

__all__ = ["group_layout", "group_bins", "device_histogram", "device_sample_rows", "booster_gradients",
           "frontier_histogram", "frontier_partition", "quantize_gradients", "linear_gram", "forest_score",
           "forest_runs", "blend_score", "device_sample_test", "host_sample_rows"]


def group_layout(ds: Dataset) -> Tuple[int, int, int, np.ndarray]:
    """(num_groups, num_total_bin, bin_width_bytes, hist_start[num_groups]) of a constructed Dataset."""
    ds.construct()
    ng, tb, bw = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _check(_LIB.LGBM_DatasetGetGroupLayout(ds.handle, ctypes.byref(ng), ctypes.byref(tb), ctypes.byref(bw), None))
    starts = np.zeros(max(ng.value, 1), dtype=np.int32)
    _check(_LIB.LGBM_DatasetGetGroupLayout(ds.handle, ctypes.byref(ng), ctypes.byref(tb), ctypes.byref(bw),
                                           starts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    return ng.value, tb.value, bw.value, starts[:ng.value]


def group_bins(ds: Dataset) -> np.ndarray:
    """[num_data, num_groups] uint16 packed group bins (0 = every feature of the group at its most frequent bin)."""
    ng = group_layout(ds)[0]
    out = np.zeros((ds.num_data(), ng), dtype=np.uint16)
    _check(_LIB.LGBM_DatasetGetGroupBins(ds.handle, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))))
    return out


def device_histogram(ds: Dataset, grad: np.ndarray, hess: np.ndarray, rows: Optional[np.ndarray] = None
                     ) -> np.ndarray:
    """[num_total_bin, 2] (sum_grad, sum_hess) histogram built by the HIP kernel on the GPU."""
    ds.construct()
    tb = group_layout(ds)[1]
    g = np.ascontiguousarray(grad, dtype=np.float32)
    h = np.ascontiguousarray(hess, dtype=np.float32)
    out = np.zeros(2 * tb, dtype=np.float64)
    if rows is not None:
        r = np.ascontiguousarray(rows, dtype=np.int32)
        rp, n = r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), r.size
    else:
        rp, n = None, ds.num_data()
    _check(_LIB.LGBM_DeviceHistogram(ds.handle, g.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                     h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), rp, ctypes.c_int32(n),
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return out.reshape(tb, 2)


_SAMPLE_MODES = {"bagging": 1, "balanced": 2, "goss": 3}


def device_sample_rows(mode: str, grad: np.ndarray, hess: np.ndarray, label: Optional[np.ndarray] = None,
                       num_class: int = 1, fraction: float = 1.0, pos_fraction: float = 1.0,
                       neg_fraction: float = 1.0, top_rate: float = 0.2, other_rate: float = 0.1,
                       bagging_seed: int = 3, goss_seed: int = 0, rounds: int = 1
                       ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Run the HIP bagging / GOSS sampling kernels once (``rounds`` re-bags for bagging).

    Returns (kept rows ascending, grad, hess) where GOSS has scaled the sampled rows."""
    g = np.array(grad, dtype=np.float32, copy=True).ravel()
    h = np.array(hess, dtype=np.float32, copy=True).ravel()
    n = g.size // num_class
    lab = None if label is None else np.ascontiguousarray(label, dtype=np.float32)
    rows = np.zeros(max(n, 1), dtype=np.int32)
    cnt = ctypes.c_int32(0)
    fp = ctypes.POINTER(ctypes.c_float)
    _check(_LIB.LGBM_DeviceSampleRows(
        ctypes.c_int(_SAMPLE_MODES[mode]), ctypes.c_int32(n), ctypes.c_int(num_class), g.ctypes.data_as(fp),
        h.ctypes.data_as(fp), None if lab is None else lab.ctypes.data_as(fp), ctypes.c_double(fraction),
        ctypes.c_double(pos_fraction), ctypes.c_double(neg_fraction), ctypes.c_double(top_rate),
        ctypes.c_double(other_rate), ctypes.c_int(bagging_seed), ctypes.c_uint32(goss_seed), ctypes.c_int(rounds),
        rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(cnt)))
    return rows[:cnt.value].copy(), g, h


def device_sample_test(mode: str, grad: np.ndarray, hess: np.ndarray, label: Optional[np.ndarray] = None,
                       query_sizes: Optional[np.ndarray] = None, num_class: int = 1, fraction: float = 1.0,
                       pos_fraction: float = 1.0, neg_fraction: float = 1.0, top_rate: float = 0.2,
                       other_rate: float = 0.1, bagging_seed: int = 3, goss_seed: int = 0, rounds: int = 1,
                       oob: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray], int, np.ndarray, np.ndarray]:
    """The HIP sampling kernels for a direct test: ``device_sample_rows`` plus ``mode="query"`` (bagging
    by query with ``query_sizes``, the query streams advanced after every round) and the out-of-bag list.

    Returns (out [n], oob [n] or None, total, grad, hess): both index buffers whole, filled with -1
    before every round, so the kept rows are ``out[:total]``, the others ``oob[:n - total]`` and
    everything behind them is -1 unless a kernel wrote past its count."""
    g = np.array(grad, dtype=np.float32, copy=True).ravel()
    h = np.array(hess, dtype=np.float32, copy=True).ravel()
    n = g.size // num_class
    lab = None if label is None else np.ascontiguousarray(label, dtype=np.float32)
    qs = None if query_sizes is None else np.ascontiguousarray(query_sizes, dtype=np.int32)
    out = np.zeros(max(n, 1), dtype=np.int32)
    out_oob = np.zeros(max(n, 1), dtype=np.int32) if oob else None
    total = ctypes.c_int32(0)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    _check(_LIB.LGBM_DeviceTestSampleRows(
        ctypes.c_int({**_SAMPLE_MODES, "query": 4}[mode]), ctypes.c_int32(n), ctypes.c_int(num_class),
        g.ctypes.data_as(fp), h.ctypes.data_as(fp), None if lab is None else lab.ctypes.data_as(fp),
        None if qs is None else qs.ctypes.data_as(ip), ctypes.c_int32(0 if qs is None else qs.size),
        ctypes.c_double(fraction), ctypes.c_double(pos_fraction), ctypes.c_double(neg_fraction),
        ctypes.c_double(top_rate), ctypes.c_double(other_rate), ctypes.c_int(bagging_seed),
        ctypes.c_uint32(goss_seed), ctypes.c_int(rounds), ctypes.c_int(int(oob)), out.ctypes.data_as(ip),
        None if out_oob is None else out_oob.ctypes.data_as(ip), ctypes.byref(total)))
    return out[:n], None if out_oob is None else out_oob[:n], total.value, g, h


def host_sample_rows(ds: Dataset, params: dict, grad: np.ndarray, hess: np.ndarray, iters, num_class: int = 1
                     ) -> Tuple[np.ndarray, np.ndarray, bool, np.ndarray, np.ndarray]:
    """The host sampler (SampleStrategy) with ``params`` over a constructed Dataset: ``Bagging(iter, grad,
    hess)`` for every iteration of ``iters``, no GPU needed.

    Returns (bag, out-of-bag, drawn, grad, hess): the rows of the last bag and the others, both as the
    sampler lists them, whether the last call drew a bag (False: every row is used, both lists empty),
    and the gradients, which GOSS has scaled."""
    ds.construct()
    n = ds.num_data()
    g = np.array(grad, dtype=np.float32, copy=True).ravel()
    h = np.array(hess, dtype=np.float32, copy=True).ravel()
    if g.size != num_class * n or h.size != num_class * n:
        raise ValueError(f"host_sample_rows: {g.size} gradients for {num_class} x {n} rows")
    it = np.ascontiguousarray(iters, dtype=np.int32).ravel()
    idx = np.zeros(max(n, 1), dtype=np.int32)
    cnt, drawn = ctypes.c_int32(0), ctypes.c_int(0)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    _check(_LIB.LGBM_TestHostSampleRows(ds.handle, ctypes.c_char_p(_param_str(params)), ctypes.c_int(num_class),
                                        it.ctypes.data_as(ip), ctypes.c_int(it.size), g.ctypes.data_as(fp),
                                        h.ctypes.data_as(fp), idx.ctypes.data_as(ip), ctypes.byref(cnt),
                                        ctypes.byref(drawn)))
    if not drawn.value:
        return idx[:0].copy(), idx[:0].copy(), False, g, h
    return idx[:cnt.value].copy(), idx[cnt.value:n].copy(), True, g, h


def booster_gradients(booster: Booster) -> Tuple[np.ndarray, np.ndarray]:
    """Gradients / hessians of the booster's last round (class-major), read back from the device."""
    n = ctypes.c_int64(0)
    _check(_LIB.LGBM_BoosterGetGradients(booster.handle, ctypes.byref(n), None, None))
    g = np.zeros(n.value, dtype=np.float32)
    h = np.zeros(n.value, dtype=np.float32)
    _check(_LIB.LGBM_BoosterGetGradients(booster.handle, ctypes.byref(n), g.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                         h.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return g, h


def position_biases(booster: Booster) -> np.ndarray:
    """Learned position biases of a lambdarank booster trained with positions (unbiased LTR), by position
    id, as float64: the device learner's when it computes the gradients, else the host objective's (held as
    float32 there). Empty without positions. Read-only."""
    n = ctypes.c_int64(0)
    _check(_LIB.LGBM_BoosterGetPositionBiases(booster.handle, ctypes.byref(n), None))
    out = np.zeros(n.value, dtype=np.float64)
    if n.value:
        _check(_LIB.LGBM_BoosterGetPositionBiases(booster.handle, ctypes.byref(n),
                                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return out


def _param_str(params: Optional[dict]) -> bytes:
    return " ".join(f"{k}={v}" for k, v in (params or {}).items()).encode()


def _subsets(subsets):
    rows = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32) for s in subsets]), dtype=np.int32)
    offsets = np.zeros(len(subsets) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(s) for s in subsets])
    return rows, offsets


def frontier_histogram(ds: Dataset, grad: np.ndarray, hess: np.ndarray, subsets, params: Optional[dict] = None
                       ) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """One launch of the frontier engine's production histogram kernel (k_f_hist) over several row
    subsets at once, one expansion each, with a device learner set up by ``params``.

    Returns ([k, num_total_bin, 2] sums at the kernel's fixed-point scale -- integer level sums under
    use_quantized_grad --, and for quantized training the per-row levels as (g_level, h_level))."""
    ds.construct()
    tb = group_layout(ds)[1]
    rows, offsets = _subsets(subsets)
    k = len(subsets)
    g = np.ascontiguousarray(grad, dtype=np.float32)
    h = np.ascontiguousarray(hess, dtype=np.float32)
    out = np.zeros(k * tb * 2, dtype=np.float64)
    levels = np.zeros(ds.num_data(), dtype=np.uint16)
    i32 = ctypes.POINTER(ctypes.c_int32)
    _check(_LIB.LGBM_DeviceTestFrontierHist(
        ds.handle, ctypes.c_char_p(_param_str(params)), g.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), rows.ctypes.data_as(i32), offsets.ctypes.data_as(i32),
        ctypes.c_int(k), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
        levels.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))))
    lv = None
    if (params or {}).get("use_quantized_grad"):
        lv = np.stack([(levels >> 8).astype(np.uint8).view(np.int8).astype(np.int64),
                       (levels & 0xFF).astype(np.int64)], axis=1)
    return out.reshape(k, tb, 2), lv


def frontier_scan(ds: Dataset, grad: np.ndarray, hess: np.ndarray, params: Optional[dict] = None
                  ) -> Tuple[np.ndarray, np.ndarray]:
    """The frontier engine's production split scan (k_f_scan) of the root round over all rows, next
    to the host learner's split_math.h scan of the same rows' exact histogram.

    Returns (device, host) arrays [num_features, 8]: gain, threshold, left count, default_left,
    left sum g, left sum h, valid (a split exists), categorical thresholds."""
    ds.construct()
    nf = ds.num_feature()
    g = np.ascontiguousarray(grad, dtype=np.float32)
    h = np.ascontiguousarray(hess, dtype=np.float32)
    out = np.zeros(nf * 8, dtype=np.float64)
    ref = np.zeros(nf * 8, dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    _check(_LIB.LGBM_DeviceTestFrontierScan(
        ds.handle, ctypes.c_char_p(_param_str(params)), g.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.ctypes.data_as(dp), ref.ctypes.data_as(dp)))
    return out.reshape(nf, 8), ref.reshape(nf, 8)


def frontier_partition(ds: Dataset, subsets, splits, params: Optional[dict] = None):
    """One launch of the frontier engine's production partition kernel (k_f_partition) over several
    parents at once. ``splits``: per parent (inner feature, threshold bin, default_left, categorical
    bins or None). Returns (device children lists, device left counts, host learner's lists, host
    left counts); each parent's list holds its lefts in order, then its rights."""
    ds.construct()
    rows, offsets = _subsets(subsets)
    k = len(subsets)
    feats = np.array([s[0] for s in splits], dtype=np.int32)
    thr = np.array([s[1] for s in splits], dtype=np.int32)
    dleft = np.array([int(s[2]) for s in splits], dtype=np.int32)
    bits = np.zeros((k, 32), dtype=np.uint32)  # kMaxCatWords (split_math.h) words per parent
    for e, s in enumerate(splits):
        for b in (s[3] if len(s) > 3 and s[3] is not None else []):
            bits[e, b >> 5] |= np.uint32(1 << (b & 31))
    out_rows = np.zeros(max(rows.size, 1), dtype=np.int32)
    exp_rows = np.zeros(max(rows.size, 1), dtype=np.int32)
    out_left = np.zeros(k, dtype=np.int32)
    exp_left = np.zeros(k, dtype=np.int32)
    i32 = ctypes.POINTER(ctypes.c_int32)
    _check(_LIB.LGBM_DeviceTestFrontierPartition(
        ds.handle, ctypes.c_char_p(_param_str(params)), rows.ctypes.data_as(i32), offsets.ctypes.data_as(i32),
        ctypes.c_int(k), feats.ctypes.data_as(i32), thr.ctypes.data_as(i32), dleft.ctypes.data_as(i32),
        bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), out_rows.ctypes.data_as(i32),
        out_left.ctypes.data_as(i32), exp_rows.ctypes.data_as(i32), exp_left.ctypes.data_as(i32)))
    return out_rows[:rows.size], out_left, exp_rows[:rows.size], exp_left


def quantize_gradients(ds: Dataset, grad: np.ndarray, hess: np.ndarray, params: dict, num_class: int = 1,
                       rounds: int = 1, const_hess: bool = False) -> dict:
    """The gradient quantizer of a device learner set up by ``params`` (k_qmax, k_quantize), run as
    training runs it: class-major ``grad`` / ``hess`` uploaded every round and quantized class by
    class, ``rounds`` times, with the learner's own grid, seed and round counter.

    Returns arrays indexed [round, class]: ``g`` / ``h`` [.., n] float32 the de-quantized values left
    in place, ``g_level`` / ``h_level`` [.., n] int64 and ``packed`` [.., n] uint16 (None unless the
    learner keeps integer levels: bins <= 254), ``max_g`` / ``max_h`` float32, and ``true_g`` /
    ``true_h`` [.., n] float32 (None unless quant_train_renew_leaf)."""
    ds.construct()
    n = ds.num_data()
    g = np.ascontiguousarray(grad, dtype=np.float32).ravel()
    h = np.ascontiguousarray(hess, dtype=np.float32).ravel()
    if g.size != num_class * n or h.size != num_class * n:
        raise ValueError(f"quantize_gradients: {g.size} gradients for {num_class} x {n} rows")
    p = {"use_quantized_grad": True, **params}
    gh = np.zeros((rounds, num_class, n, 2), dtype=np.float32)
    packed = np.zeros((rounds, num_class, n), dtype=np.uint16)
    qmax = np.zeros((rounds, num_class, 2), dtype=np.uint32)
    true = np.zeros((rounds, num_class, n, 2), dtype=np.float32)
    has = ctypes.c_int(0)
    fp = ctypes.POINTER(ctypes.c_float)
    _check(_LIB.LGBM_DeviceTestQuantize(
        ds.handle, ctypes.c_char_p(_param_str(p)), ctypes.c_int(int(const_hess)), g.ctypes.data_as(fp),
        h.ctypes.data_as(fp), ctypes.c_int(num_class), ctypes.c_int(rounds), gh.ctypes.data_as(fp),
        packed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), qmax.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
        true.ctypes.data_as(fp), ctypes.byref(has)))
    mx = qmax.view(np.float32)
    renew = str(p.get("quant_train_renew_leaf", False)).lower() in ("true", "1")
    out = {"g": gh[..., 0], "h": gh[..., 1], "max_g": mx[..., 0], "max_h": mx[..., 1],
           "packed": None, "g_level": None, "h_level": None,
           "true_g": true[..., 0] if renew else None, "true_h": true[..., 1] if renew else None}
    if has.value:
        out["packed"] = packed
        out["g_level"] = (packed >> 8).astype(np.uint8).view(np.int8).astype(np.int64)
        out["h_level"] = (packed & 0xFF).astype(np.int64)
    return out


def linear_gram(raw: np.ndarray, grad: np.ndarray, hess: np.ndarray, leaves, feats, chunks: int = 1
                ) -> Tuple[np.ndarray, np.ndarray]:
    """One launch of the linear-leaf Gram kernels (k_linear_gram, k_linear_fold) over host arrays.

    ``raw`` [n, f] float32; ``leaves``: per leaf an array of row numbers, or a ``range`` for the
    contiguous rows the kernel reads without an index list; ``feats``: per leaf its sorted feature
    columns. Returns (out [leaves, 64, 64]: A in rows / columns [0, m) and c in column m, with
    m = features + 1; usable [leaves] int64)."""
    x = np.ascontiguousarray(raw, dtype=np.float32)
    n, f = x.shape
    g = np.ascontiguousarray(grad, dtype=np.float32)
    h = np.ascontiguousarray(hess, dtype=np.float32)
    if g.size != n or h.size != n or len(leaves) != len(feats):
        raise ValueError("linear_gram: inconsistent inputs")
    nl = len(leaves)
    segs = np.zeros((nl, 3), dtype=np.int32)
    lists = []
    pos = 0
    for l, rows in enumerate(leaves):
        if isinstance(rows, range):
            if rows.step != 1:
                raise ValueError("linear_gram: contiguous ranges only")
            segs[l] = (-1, rows.start, len(rows))
        else:
            r = np.asarray(rows, dtype=np.int32)
            segs[l] = (0, pos, r.size)
            lists.append(r)
            pos += r.size
    rows = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), dtype=np.int32)
    off = np.zeros(nl + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(c) for c in feats])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.int32) for c in feats]), dtype=np.int32)
    out = np.zeros((nl, 64, 64), dtype=np.float64)
    usable = np.zeros(nl, dtype=np.int64)
    i32, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    _check(_LIB.LGBM_DeviceTestLinearGram(
        x.ctypes.data_as(fp), ctypes.c_int32(n), ctypes.c_int32(f), g.ctypes.data_as(fp), h.ctypes.data_as(fp),
        rows.ctypes.data_as(i32), ctypes.c_int32(rows.size), segs.ctypes.data_as(i32), ctypes.c_int(nl),
        off.ctypes.data_as(i32), flat.ctypes.data_as(i32), ctypes.c_int(chunks),
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), usable.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    return out, usable


def forest_score(ds: Dataset, booster: Booster, trees, scales, score: np.ndarray, grid: Optional[int] = None,
                 mode: str = "forest", info: Optional[dict] = None) -> np.ndarray:
    """The forest traversal kernel (k_traverse_forest) over the packed rows of a constructed Dataset.

    For tree ``trees[j]`` of ``booster`` its leaf values times ``scales[j]`` (the fp64 product of
    ``Tree::Shrinkage``) are added, in list order, into a copy of ``score`` (float64, num_data), which
    is returned. ``mode="tree"`` runs one single-tree traversal per tree instead; ``grid`` caps the
    forest kernel's grid, so one block owns several row tiles at small row counts. A dict passed as
    ``info`` receives the row format the traversal read: ``row_bits`` (4, 8 or 16 per group bin) and
    ``stride_dw`` (dwords per row)."""
    if mode not in ("forest", "tree"):
        raise ValueError(f"mode must be 'forest' or 'tree', got {mode!r}")
    ds.construct()
    idx = np.ascontiguousarray(trees, dtype=np.int32).ravel()
    sc = np.ascontiguousarray(scales, dtype=np.float64).ravel()
    if idx.size != sc.size:
        raise ValueError("one scale per tree")
    s = np.ascontiguousarray(score, dtype=np.float64).ravel()
    if s.size != ds.num_data():
        raise ValueError(f"score has {s.size} values for {ds.num_data()} rows")
    out = np.zeros(max(s.size, 1), dtype=np.float64)
    fmt = np.zeros(2, dtype=np.int32)
    dp = ctypes.POINTER(ctypes.c_double)
    _check(_LIB.LGBM_DeviceTestForestScore(
        ds.handle, booster.handle, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), sc.ctypes.data_as(dp),
        ctypes.c_int(idx.size), s.ctypes.data_as(dp), ctypes.c_int(int(grid or 0)),
        ctypes.c_int(1 if mode == "tree" else 0), out.ctypes.data_as(dp),
        fmt.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    if info is not None:
        info["row_bits"] = (4, 8, 16)[int(fmt[0])]
        info["stride_dw"] = int(fmt[1])
    return out[:s.size]


def blend_score(ds: Dataset, booster: Booster, tree: int, score: np.ndarray, pre: float, post: float,
                divide: bool = False, grid: Optional[int] = None) -> np.ndarray:
    """The blended score update (boosting=rf's running average on the GPU) over the packed rows of a
    constructed Dataset.

    Tree ``tree`` of ``booster`` is blended into a copy of ``score`` (float64, num_data), which is
    returned: ``(score * pre + leaf) * post``, or ``/ post`` with ``divide``, each operation rounded
    on its own. A tree with splits takes the blended traversal kernel of the dataset's row format, a
    one-leaf tree the blended constant. ``grid`` caps the kernel's grid, so one block owns several
    row tiles at small row counts."""
    ds.construct()
    s = np.ascontiguousarray(score, dtype=np.float64).ravel()
    if s.size != ds.num_data():
        raise ValueError(f"score has {s.size} values for {ds.num_data()} rows")
    out = np.zeros(max(s.size, 1), dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    _check(_LIB.LGBM_DeviceTestBlendScore(
        ds.handle, booster.handle, ctypes.c_int(int(tree)), s.ctypes.data_as(dp), ctypes.c_double(float(pre)),
        ctypes.c_double(float(post)), ctypes.c_int(1 if divide else 0), ctypes.c_int(int(grid or 0)),
        out.ctypes.data_as(dp)))
    return out[:s.size]


def forest_runs(booster: Booster, trees) -> Tuple[list, list, int]:
    """How ``forest_score`` splits these trees into LDS runs: (trees per run, bytes per run, the run
    byte budget). A run over the budget is one tree that the kernel walks from global memory."""
    idx = np.ascontiguousarray(trees, dtype=np.int32).ravel()
    cnt = np.zeros(max(idx.size, 1), dtype=np.int32)
    nbytes = np.zeros(max(idx.size, 1), dtype=np.int32)
    nruns, budget = ctypes.c_int(0), ctypes.c_int(0)
    i32 = ctypes.POINTER(ctypes.c_int32)
    _check(_LIB.LGBM_DeviceTestForestRuns(booster.handle, idx.ctypes.data_as(i32), ctypes.c_int(idx.size),
                                          cnt.ctypes.data_as(i32), nbytes.ctypes.data_as(i32), ctypes.byref(nruns),
                                          ctypes.byref(budget)))
    return cnt[:nruns.value].tolist(), nbytes[:nruns.value].tolist(), budget.value
