"""The checks of tests/test_update_device.py. They run in one fresh interpreter that starts with
torch (main() below), one verdict per check; this module imports neither torch nor the library
when it is only read for the names of the checks.

Exactness rests on one device. Every test objective computes its gradients on the host in numpy
from ``preds.cpu().numpy()`` and uploads them as tensors, so ``update_device`` and
``update(fobj)`` see identical values (float64 narrowed to float32 to nearest even on both
paths). Model text, ``ops.booster_gradients`` and raw scores are compared bit for bit: there is
no tolerance in this file.
"""
import contextlib
import json
import re
import sys

import numpy as np

torch = lgb = ops = None  # set by main()

BASE = {"objective": "none", "device_type": "gpu", "verbosity": -1, "min_data_in_leaf": 1, "min_data_in_bin": 1,
        "num_leaves": 7}

LAYOUT_NS = [2, 63, 64, 65, 257, 4097]
LAYOUT_KS = [1, 3, 5]
LAYOUTS = ["contig", "kn_t", "flat", "colslice", "rowstep", "offset1"]
NON_FINITE = {
    "beyond_float_range": ("grad", 100, 1, 1e39, "gradient"),  # finite as fp64
    "nan_first_row": ("hess", 0, 0, float("nan"), "hessian"),
    "nan_last_row": ("hess", 256, 1, float("nan"), "hessian"),
    "nan_last_class": ("grad", 17, 2, float("nan"), "gradient"),
    "inf_last_element": ("grad", 256, 2, float("-inf"), "gradient"),
}
NON_FINITE_LAYOUTS = ["contig", "kn_t", "rowstep"]  # the tile, the row-streaming and again the tile kernel
PARITY = {
    "regression": (1, {}),
    "softmax3": (3, {}),
    "bagging": (1, {"bagging_fraction": 0.7, "bagging_freq": 1}),
    "goss": (1, {"data_sample_strategy": "goss"}),
    "goss_host_sampler": (1, {"data_sample_strategy": "goss", "device_sampling": False}),
    "goss_host_sampler_3class": (3, {"data_sample_strategy": "goss", "device_sampling": False}),
    "quantized": (1, {"use_quantized_grad": True}),
    "no_graph": (1, {"device_use_graph": False}),
}
REFUSALS = {
    "dart": {"boosting": "dart"},
    "host_route": {"monotone_constraints": [1, 0, 0], "monotone_constraints_method": "advanced"},
    "builtin_objective": {"objective": "regression"},
}


@contextlib.contextmanager
def _raises(exc, match=None):
    """The block must end with an ``exc`` whose message holds ``match`` (a regular expression)."""
    try:
        yield
    except exc as e:
        assert match is None or re.search(match, str(e)), f"{type(e).__name__} without {match!r}: {e}"
    else:
        raise AssertionError(f"no {exc.__name__} was raised")


def _booster(n, k, seed=0, extra=None, ncol=3, valid=False):
    r = np.random.default_rng(seed)
    X = r.normal(size=(n, ncol))
    y = r.normal(size=n) if k == 1 else r.integers(0, k, size=n).astype(np.float64)
    params = dict(BASE)
    if k > 1:
        params["num_class"] = k
    params.update(extra or {})
    ds = lgb.Dataset(X, y, params=params)
    b = lgb.Booster(params, ds)
    if valid:
        Xv = r.normal(size=(max(2, n // 3), ncol))
        yv = r.normal(size=Xv.shape[0]) if k == 1 else r.integers(0, k, size=Xv.shape[0]).astype(np.float64)
        b.add_valid(lgb.Dataset(Xv, yv, reference=ds, params=params), "valid")
    return b, y


# ---------------------------------------------------------------- layouts
def _present(a, how, dtype):
    """The (N, K) float64 array ``a`` as a GPU tensor of ``dtype`` in the layout ``how``."""
    n, k = a.shape
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    t = torch.from_numpy(np.ascontiguousarray(a.astype(dtype))).cuda()  # (N, K) contiguous
    if how == "contig":  # (N,) / (N, K) contiguous
        return t.reshape(n) if k == 1 else t
    if how == "kn_t":  # the transpose of a (K, N) buffer: unit row stride
        return t.T.contiguous().T
    if how == "flat":  # class-major 1-D
        return t.T.contiguous().reshape(n * k)
    if how == "colslice":  # columns 2 .. 2 + K of a wider tensor
        big = torch.full((n, k + 5), 7.0, dtype=tdt, device="cuda")
        big[:, 2:2 + k] = t
        return big[:, 2] if k == 1 else big[:, 2:2 + k]
    if how == "rowstep":  # every second row of a taller tensor
        big = torch.full((2 * n, k), 7.0, dtype=tdt, device="cuda")
        big[::2] = t
        return big[::2, 0] if k == 1 else big[::2]
    if how == "offset1":  # class-major 1-D, one element past an aligned allocation
        buf = torch.full((n * k + 1,), 7.0, dtype=tdt, device="cuda")
        buf[1:] = t.T.contiguous().reshape(n * k)
        out = buf[1:]
        assert out.data_ptr() % 16 != 0
        return out
    raise AssertionError(how)


def layouts(n, k):
    """After update_device, the learner's gradients are astype(float32) of the inputs, class-major."""
    b, _ = _booster(n, k, seed=n * 7 + k)
    r = np.random.default_rng(n + 100 * k)
    round_no = 0

    def check(g_how, g_dt, h_how, h_dt):
        nonlocal round_no
        round_no += 1
        g = r.normal(size=(n, k)) * 3.0
        h = r.uniform(0.5, 2.0, size=(n, k))
        tg, th = _present(g, g_how, g_dt), _present(h, h_how, h_dt)
        b.update_device(lambda preds, ds: (tg, th))
        got_g, got_h = ops.booster_gradients(b)
        want_g = g.astype(g_dt).astype(np.float32).T.ravel()
        want_h = h.astype(h_dt).astype(np.float32).T.ravel()
        tag = f"n={n} k={k} round {round_no}: grad {g_how}/{np.dtype(g_dt).name}, hess {h_how}/{np.dtype(h_dt).name}"
        assert got_g.dtype == np.float32 and got_g.tobytes() == want_g.tobytes(), tag
        assert got_h.dtype == np.float32 and got_h.tobytes() == want_h.tobytes(), tag

    for dt in (np.float32, np.float64):
        for how in LAYOUTS:
            check(how, dt, how, dt)
    # grad and hess in different layouts and dtypes in one call
    check("contig", np.float32, "kn_t", np.float64)
    check("flat", np.float64, "rowstep", np.float32)
    check("offset1", np.float32, "flat", np.float64)


def other_dtypes():
    n = 65
    b, _ = _booster(n, 1)
    g = np.random.default_rng(3).normal(size=n)
    tg = torch.from_numpy(g).cuda().to(torch.float16)
    th = torch.ones(n, dtype=torch.int32, device="cuda")
    b.update_device(lambda preds, ds: (tg, th))
    got_g, got_h = ops.booster_gradients(b)
    assert got_g.tobytes() == tg.to(torch.float32).cpu().numpy().tobytes()
    assert got_h.tobytes() == np.ones(n, dtype=np.float32).tobytes()


def non_finite(case, how):
    which, row, col, value, word = NON_FINITE[case]
    n, k = 257, 3
    b, _ = _booster(n, k)
    r = np.random.default_rng(5)
    g, h = r.normal(size=(n, k)), r.uniform(0.5, 2.0, size=(n, k))
    # ("mixed": the gradient (N, K), the hessian (K, N).T, which takes the gather kernel)
    g_how, h_how = ("contig", "kn_t") if how == "mixed" else (how, how)
    b.update_device(lambda preds, ds: (_present(g, g_how, np.float64), _present(h, h_how, np.float64)))
    trees = b.num_trees()
    assert trees == k
    (g if which == "grad" else h)[row, col] = value
    tg, th = _present(g, g_how, np.float64), _present(h, h_how, np.float64)
    with _raises(lgb.LightGBMError, match=word):
        b.update_device(lambda preds, ds: (tg, th))
    assert b.num_trees() == trees


# ---------------------------------------------------------------- training parity
def _np_objective(k, y):
    """A numpy objective (preds (N,) or (N, K) float64 -> float64 grad, hess)."""
    if k == 1:
        def fobj(preds, ds):
            return preds - y, np.ones_like(preds)
        return fobj
    onehot = np.eye(k)[y.astype(int)]

    def fobj(preds, ds):
        e = np.exp(preds - preds.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
        return p - onehot, 2.0 * p * (1.0 - p)
    return fobj


def _on_device(fobj_np):
    """The same objective on GPU tensors: the values are computed on the host from a download."""
    def fobj(preds, ds):
        assert isinstance(preds, torch.Tensor) and preds.is_cuda and preds.dtype == torch.float64
        g, h = fobj_np(preds.cpu().numpy(), ds)
        return torch.from_numpy(np.ascontiguousarray(g)).cuda(), torch.from_numpy(np.ascontiguousarray(h)).cuda()
    return fobj


def parity(name):
    k, extra = PARITY[name]
    extra = dict(extra, num_leaves=15, min_data_in_leaf=20, min_data_in_bin=3)
    host, y = _booster(3000, k, seed=11, extra=extra, ncol=10)
    dev, _ = _booster(3000, k, seed=11, extra=extra, ncol=10)
    f_np = _np_objective(k, y)
    f_dev = _on_device(f_np)
    for it in range(5):
        fin_h = host.update(fobj=f_np)
        fin_d = dev.update_device(f_dev)
        assert fin_h == fin_d
        if name in ("regression", "softmax3", "no_graph"):  # (no sampling: the gradients are the objective's)
            gh, gd = ops.booster_gradients(host), ops.booster_gradients(dev)
            assert gh[0].tobytes() == gd[0].tobytes() and gh[1].tobytes() == gd[1].tobytes(), it
    assert dev.num_trees() == 5 * k
    assert dev.model_to_string() == host.model_to_string()


# ---------------------------------------------------------------- score export
def _host_raw(b, idx):
    """LGBM_BoosterGetPredict's values (objective none: raw), shaped as update's preds."""
    return np.array(b._Booster__inner_predict(idx))


def score_export(k):
    b, y = _booster(1500, k, seed=21, extra={"num_leaves": 15}, ncol=6, valid=True)
    f_dev = _on_device(_np_objective(k, y))
    n_valid = b.valid_sets[0].num_data()
    for it in range(3):
        b.update_device(f_dev)
        for idx, rows in ((0, 1500), (1, n_valid)):
            t = b.raw_score_device(idx)
            assert t.is_cuda and t.dtype == torch.float64
            assert tuple(t.shape) == ((rows,) if k == 1 else (rows, k))
            want = np.ascontiguousarray(_host_raw(b, idx)).tobytes()
            assert t.cpu().numpy().tobytes() == want, (it, idx)
            assert any(want)
            t.zero_()  # the tensor is a copy: the next call is unchanged
            assert b.raw_score_device(idx).cpu().numpy().tobytes() == want, (it, idx)


def preds_is_a_copy():
    b, y = _booster(500, 1, seed=4)
    f_np = _np_objective(1, y)

    def fobj(preds, ds):
        g, h = f_np(preds.cpu().numpy(), ds)
        preds.fill_(123.0)
        return torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda()

    b.update_device(fobj)
    first = _host_raw(b, 0).copy()
    assert not np.any(first == 123.0)
    assert b.raw_score_device(0).cpu().numpy().tobytes() == first.tobytes()


# ---------------------------------------------------------------- train()
def _train_data():
    r = np.random.default_rng(31)
    X = r.normal(size=(2000, 8))
    y = X[:, 0] + 0.5 * X[:, 1] ** 2 + r.normal(size=2000)
    Xv = r.normal(size=(600, 8))
    yv = Xv[:, 0] + 0.5 * Xv[:, 1] ** 2 + r.normal(size=600) * 2.0
    return X, y, Xv, yv


def train_marked():
    X, y, Xv, yv = _train_data()
    params = {"device_type": "gpu", "verbosity": -1, "num_leaves": 31, "learning_rate": 0.5, "min_data_in_leaf": 5,
              "early_stopping_round": 3, "metric": "None"}
    seen = {"obj": 0, "metric": 0}

    def np_obj(preds, ds):
        assert isinstance(preds, np.ndarray)
        return preds - ds.get_label(), np.ones_like(preds)

    def np_metric(preds, ds):
        assert isinstance(preds, np.ndarray)
        return "my_l2", float(np.mean((preds - ds.get_label()) ** 2)), False

    @lgb.device_objective
    def dev_obj(preds, ds):
        assert isinstance(preds, torch.Tensor) and preds.is_cuda
        seen["obj"] += 1
        g, h = np_obj(preds.cpu().numpy(), ds)
        return torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda()

    @lgb.device_metric
    def dev_metric(preds, ds):
        assert isinstance(preds, torch.Tensor) and preds.is_cuda
        seen["metric"] += 1
        return np_metric(preds.cpu().numpy(), ds)

    def run(obj, metric):
        ds = lgb.Dataset(X, y)
        dv = lgb.Dataset(Xv, yv, reference=ds)
        rec = {}
        b = lgb.train(dict(params, objective=obj), ds, num_boost_round=40, valid_sets=[dv], valid_names=["v"],
                      feval=metric, callbacks=[lgb.record_evaluation(rec)])
        return b, rec

    host, rec_h = run(np_obj, np_metric)
    dev, rec_d = run(dev_obj, dev_metric)
    assert seen["obj"] > 0 and seen["metric"] > 0
    assert 0 < host.best_iteration < 40, host.best_iteration  # (early stopping did stop)
    assert dev.best_iteration == host.best_iteration
    assert rec_d == rec_h
    assert dev.model_to_string() == host.model_to_string()


def train_unmarked():
    X, y, Xv, yv = _train_data()
    calls = []

    def np_obj(preds, ds):
        assert isinstance(preds, np.ndarray)
        calls.append("obj")
        return preds - ds.get_label(), np.ones_like(preds)

    def np_metric(preds, ds):
        assert isinstance(preds, np.ndarray)
        calls.append("metric")
        return "my_l2", float(np.mean((preds - ds.get_label()) ** 2)), False

    ds = lgb.Dataset(X, y)
    b = lgb.train({"device_type": "gpu", "verbosity": -1, "objective": np_obj, "metric": "None"}, ds, num_boost_round=2,
                  valid_sets=[lgb.Dataset(Xv, yv, reference=ds)], feval=np_metric)
    assert b.num_trees() == 2 and calls.count("obj") == 2 and calls.count("metric") == 2


def device_metric_raw_scores():
    r = np.random.default_rng(8)
    X = r.normal(size=(800, 5))
    y = (X[:, 0] > 0).astype(np.float64)
    got = {}

    @lgb.device_metric
    def raw_mean(preds, ds):
        got["preds"] = preds.cpu().numpy().copy()
        return "raw_mean", float(preds.mean()), False

    ds = lgb.Dataset(X, y)
    b = lgb.train({"device_type": "gpu", "verbosity": -1, "objective": "binary", "metric": "None"}, ds,
                  num_boost_round=3, valid_sets=[ds], feval=raw_mean, keep_training_booster=True)
    assert got["preds"].tobytes() == b.raw_score_device(0).cpu().numpy().tobytes()
    assert got["preds"].min() < 0.0  # raw margins, not probabilities


# ---------------------------------------------------------------- refusals
def _good(n, k=1):
    return torch.zeros(n * k, dtype=torch.float32, device="cuda"), torch.ones(n * k, dtype=torch.float32, device="cuda")


def library_refusal(name):
    n = 300
    b, _ = _booster(n, 1, extra=REFUSALS[name])
    with _raises(lgb.LightGBMError, match="update"):
        b.update_device(lambda preds, ds: _good(n))
    with _raises(lgb.LightGBMError, match="update"):
        b._boost_device(*_good(n))
    assert b.num_trees() == 0


def python_refusals():
    n = 300
    b, _ = _booster(n, 1)
    with _raises(TypeError, match="update"):
        b.update_device(lambda preds, ds: (torch.zeros(n), torch.ones(n)))  # host tensors
    with _raises(TypeError, match="update"):
        b.update_device(lambda preds, ds: (np.zeros(n), np.ones(n)))
    with _raises(ValueError, match="don't match"):
        b.update_device(lambda preds, ds: _good(n - 1))
    with _raises(ValueError, match="don't match"):
        b.update_device(lambda preds, ds: (_good(n)[0], _good(n + 1)[1]))
    with _raises(ValueError):
        b.update_device(lambda preds, ds: tuple(t.reshape(2, n // 2) for t in _good(n)))
    assert b.num_trees() == 0
    assert b.update_device(lambda preds, ds: _good(n)) in (True, False)


# ---------------------------------------------------------------- the list of checks
def _checks():
    c = {}
    for n in LAYOUT_NS:
        for k in LAYOUT_KS:
            c[f"layouts-{n}-{k}"] = lambda n=n, k=k: layouts(n, k)
    c["other_dtypes"] = other_dtypes
    for case in NON_FINITE:
        for how in NON_FINITE_LAYOUTS + ["mixed"]:
            c[f"non_finite-{case}-{how}"] = lambda case=case, how=how: non_finite(case, how)
    for name in PARITY:
        c[f"parity-{name}"] = lambda name=name: parity(name)
    for k in (1, 3):
        c[f"score_export-{k}"] = lambda k=k: score_export(k)
    c["preds_is_a_copy"] = preds_is_a_copy
    c["train_marked"] = train_marked
    c["train_unmarked"] = train_unmarked
    c["device_metric_raw_scores"] = device_metric_raw_scores
    for name in REFUSALS:
        c[f"refusal-{name}"] = lambda name=name: library_refusal(name)
    c["python_refusals"] = python_refusals
    return c


CHECK_NAMES = list(_checks())
SCORE_EXPORT_NAMES = [n for n in CHECK_NAMES if n.startswith("score_export-")]


def main(prefix=""):
    """Run the checks whose names start with ``prefix``; torch creates its context before the
    library's first GPU call (a process serves both only in that order)."""
    global torch, lgb, ops
    import torch as _torch

    assert _torch.cuda.is_available(), "torch sees no GPU"
    _torch.zeros(1, device="cuda")
    _torch.cuda.synchronize()
    import lambdagap_amd as _lgb
    from lambdagap_amd import ops as _ops

    torch, lgb, ops = _torch, _lgb, _ops
    assert lgb.device_count() >= 1, "the library sees no GPU"
    res = {}
    for key, fn in _checks().items():
        if not key.startswith(prefix):
            continue
        try:
            fn()
            res[key] = "ok"
        except Exception as e:  # the verdict travels to the parent test
            res[key] = f"{type(e).__name__}: {e}"[:1500]
            if "HIP error" in res[key]:  # nothing more runs on a device that reported an error
                break
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "")
