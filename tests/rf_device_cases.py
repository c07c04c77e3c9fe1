"""The runs behind tests/test_rf_device.py (GPU) and tests/test_rf_reference_cpu.py (CPU).

LGAP_DEVICE_RF is read once per process, so each path (unset: the averaged scores on the device,
"0": on the host) runs in a child interpreter that calls main() and prints one ``RESULT <json>``
line; the parent compares the children's reports. LGAP_FRONTIER is read when a learner is
created, so the child sets it around the one case that needs it."""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

F, ITERS, NV = 10, 12, 700

BASE = {"boosting": "rf", "device_type": "gpu", "objective": "regression", "num_leaves": 15, "min_data_in_leaf": 5,
        "verbosity": -1, "seed": 3, "bagging_freq": 1, "bagging_fraction": 0.632, "feature_fraction": 0.8}

# option sets of the bit-for-bit comparison: "n" rows, "valid" a validation set, "env" set while the
# booster is built, "leaf_map" whether the training score takes the leaf map on the device path
CASES = {
    # the 4-row vector body of the blended leaf add and each tail length; device bagging
    "n3000": {"n": 3000, "leaf_map": True},
    "n3001": {"n": 3001, "leaf_map": True, "valid": True},
    "n3002": {"n": 3002, "leaf_map": True},
    "n3003": {"n": 3003, "leaf_map": True},
    # no bag: the leaf map without an out-of-bag list
    "feature_fraction_only": {"n": 3001, "leaf_map": True, "params": {"bagging_freq": 0, "bagging_fraction": 1.0}},
    # the host sampler: no out-of-bag list on the device, every row is walked
    "bagging_host_sampler": {"n": 3001, "leaf_map": False, "params": {"device_sampling": False}},
    # more than 256 leaves: the uint16 map
    "leaves300": {"n": 3001, "leaf_map": True, "params": {"num_leaves": 300, "min_data_in_leaf": 1}},
    # 4-bit training rows: under the leaf map, and walked by the blended 4-bit traversal
    "max_bin15": {"n": 3001, "leaf_map": True, "valid": True, "params": {"max_bin": 15}},
    "max_bin15_walked": {"n": 3001, "leaf_map": False, "params": {"max_bin": 15, "device_sampling": False}},
    # classes 1 and 2 start at unaligned slices of the score: the scalar path
    "multiclass": {"n": 2999, "leaf_map": True, "params": {"objective": "multiclass", "num_class": 3}},
    "quantized": {"n": 3001, "leaf_map": True, "params": {"use_quantized_grad": True}},
    # no leaf map, every tree traversed
    "no_frontier": {"n": 3001, "leaf_map": False, "env": {"LGAP_FRONTIER": "0"}},
}
GATED = {
    "regression_l1": {"objective": "regression_l1"},
    "linear_tree": {"linear_tree": True},
    "goss": {"data_sample_strategy": "goss", "bagging_freq": 0, "bagging_fraction": 1.0},
}
BLEND_TIMERS = ("Device::BlendLeafMap", "Device::BlendTraverse")
TIMERS = BLEND_TIMERS + ("GBDT::Boosting",)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_data(n, classes=1, seed=5, binary=False):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F))
    z = X[:, 1] + 0.5 * X[:, 2] * X[:, 3] + np.sin(2 * X[:, 0]) + rng.normal(size=n) * 0.5
    if binary:
        return X, (z > np.median(z)).astype(np.float64)
    if classes > 1:
        return X, np.digitize(z, np.quantile(z, np.linspace(0, 1, classes + 1)[1:-1])).astype(np.float64)
    return X, z + 3.0


def timer_counts(lgb):
    """{timer: calls} from phase_timer_report() (the process runs with LGAP_TIMETAG=1)."""
    out = dict.fromkeys(TIMERS, 0)
    for line in lgb.phase_timer_report().splitlines():
        p = line.split()
        if len(p) >= 3 and p[0] in out and p[-1] == "calls":
            out[p[0]] = int(p[-2])
    return out


def leaf_max(model_text):
    """the largest |leaf value| of any tree of a model text."""
    return max(float(np.max(np.abs(np.array(ln.split("=", 1)[1].split(), dtype=np.float64))))
               for ln in model_text.splitlines() if ln.startswith("leaf_value="))


def bound(iters, m):
    """How far RF's running average may be from predict(raw_score=True) of the same trees. Blend i
    (i = 0 .. T - 1) makes three roundings on values bounded by (i + 1) M, each at most 2^-53 of
    that, and the later blends scale what it left by 1 / (i + 1) overall: 3 T roundings of 2^-53 M
    on the average. predict makes T adds on partial sums bounded by T M and one division: T + 1
    more. A rollback adds three roundings. (4 T + 6) 2^-53 M covers them with room."""
    return (4 * iters + 6) * 2.0 ** -53 * m


class _Env:
    def __init__(self, env):
        self.env, self.old = env or {}, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _booster(lgb, case, device_type=None):
    params = dict(BASE, **case.get("params", {}))
    if device_type is not None:
        params["device_type"] = device_type
    classes = params.get("num_class", 1)
    X, y = make_data(case["n"], classes)
    train = lgb.Dataset(X, y, params=params)
    with _Env(case.get("env")):
        bst = lgb.Booster(params, train)
        Xv = None
        if case.get("valid"):
            Xv, yv = make_data(NV, classes, seed=6)
            bst.add_valid(lgb.Dataset(Xv, yv, reference=train), "v")
    return bst, X, Xv, classes


def _raw_dev(bst, idx, classes):
    """the class-major raw score raw_score_device hands back, in __inner_predict's order."""
    return bst.raw_score_device(idx).cpu().numpy().reshape(-1)


def bitwise_run(lgb, name, device, torch=None, device_type=None):
    """model text, the sha256 of the training score and of the validation score after every
    iteration (eval's host read), whether raw_score_device agrees with that read (device path),
    the final scores next to predict(raw_score=True), and how the blend timers grew."""
    case = CASES[name]
    before = timer_counts(lgb)
    bst, X, Xv, classes = _booster(lgb, case, device_type)
    train_sha, valid_sha, same = [], [], []
    for _ in range(ITERS):
        bst.update()
        if device and torch is not None:
            dev = _raw_dev(bst, 0, classes)
        host = bst._Booster__inner_predict(0)
        train_sha.append(_sha(host))
        if device and torch is not None and classes == 1:
            same.append(dev.tobytes() == np.ascontiguousarray(host).tobytes())
        if Xv is not None:
            hv = bst._Booster__inner_predict(1)
            valid_sha.append(_sha(hv))
            if device and torch is not None and classes == 1:
                same.append(_raw_dev(bst, 1, classes).tobytes() == np.ascontiguousarray(hv).tobytes())
    after = timer_counts(lgb)
    model = bst.model_to_string()
    out = {"model": model, "train": train_sha, "valid": valid_sha, "same": same, "trees": bst.num_trees(),
           "grew": {t: after[t] - before[t] for t in TIMERS}}
    if classes == 1:
        m = leaf_max(model)
        out["bound"] = bound(ITERS, m)
        out["train_diff"] = float(np.max(np.abs(bst._Booster__inner_predict(0) - bst.predict(X, raw_score=True))))
        if Xv is not None:
            out["valid_diff"] = float(np.max(np.abs(bst._Booster__inner_predict(1) - bst.predict(Xv, raw_score=True))))
    return out


def rollback_run(lgb, device_type=None):
    """12 iterations, a rollback, one more iteration: the training score after the rollback, every
    score next to the remaining model, the model text at the end."""
    case = {"n": 3001, "valid": True}
    bst, X, Xv, _ = _booster(lgb, case, device_type)
    for _ in range(ITERS):
        bst.update()
    b = bound(ITERS, leaf_max(bst.model_to_string()))
    bst.rollback_one_iter()
    out = {"trees_after_rollback": bst.num_trees(), "bound": b,
           "train": _sha(bst._Booster__inner_predict(0)),
           "train_diff": float(np.max(np.abs(bst._Booster__inner_predict(0) - bst.predict(X, raw_score=True)))),
           "valid_diff": float(np.max(np.abs(bst._Booster__inner_predict(1) - bst.predict(Xv, raw_score=True))))}
    bst.update()
    out["model"] = bst.model_to_string()
    out["trees"] = bst.num_trees()
    return out


def _logloss(y, p):
    eps = 1e-15
    p = np.clip(p, eps, 1.0 - eps)
    return float(np.mean(np.where(y > 0, -np.log(p), -np.log(1.0 - p))))


def _auc(y, s):
    order = np.argsort(s, kind="mergesort")
    s, y = s[order], y[order]
    ranks = np.empty(len(s))  # average ranks over ties
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        ranks[i:j + 1] = 0.5 * (i + j) + 1.0
        i = j + 1
    pos = y > 0
    npos, nneg = int(pos.sum()), int((~pos).sum())
    return float((ranks[pos].sum() - npos * (npos + 1) / 2.0) / (npos * nneg))


def metrics_run(lgb):
    """objective=binary on the device path: every iteration's training binary_logloss and
    validation auc next to the same metrics recomputed in numpy from raw_score_device."""
    params = dict(BASE, objective="binary", metric=["binary_logloss", "auc"])
    X, y = make_data(3001, binary=True)
    Xv, yv = make_data(NV, seed=6, binary=True)
    train = lgb.Dataset(X, y, params=params)
    bst = lgb.Booster(params, train)
    bst.add_valid(lgb.Dataset(Xv, yv, reference=train), "v")
    reported, recomputed = [], []
    for _ in range(ITERS):
        bst.update()
        ev = {(d, m): v for d, m, v, _ in bst.eval_train() + bst.eval_valid()}
        reported.append([ev[("training", "binary_logloss")], ev[("v", "auc")]])
        raw_train = bst.raw_score_device(0).cpu().numpy()
        raw_valid = bst.raw_score_device(1).cpu().numpy()
        recomputed.append([_logloss(y, 1.0 / (1.0 + np.exp(-raw_train))), _auc(yv, raw_valid)])
    return {"reported": reported, "recomputed": recomputed, "trees": bst.num_trees()}


class _ListLogger:
    def __init__(self, lines):
        self.lines = lines

    def info(self, msg):
        self.lines.append(str(msg))

    def warning(self, msg):
        self.lines.append(str(msg))


def gated_run(lgb, name):
    """A configuration RF keeps on the host: it trains, says why, runs no blend kernel, and
    raw_score_device refuses it."""
    lines = []
    lgb.register_logger(_ListLogger(lines))
    before = timer_counts(lgb)
    X, y = make_data(2000)
    if name == "init_model":
        params = dict(BASE, verbosity=1)
        first = lgb.train(dict(BASE), lgb.Dataset(X, y, params=dict(BASE)), num_boost_round=3)
        del lines[:]
        holder = []
        bst = lgb.train(params, lgb.Dataset(X, y, params=params), num_boost_round=3, init_model=first,
                        callbacks=[_keep(holder)])
        before = holder[0]  # (the first booster ran on the device)
    else:
        params = dict(BASE, verbosity=1, **GATED[name])
        bst = lgb.train(params, lgb.Dataset(X, y, params=params), num_boost_round=5)
    refused = ""
    try:
        bst.raw_score_device(0)
    except lgb.LightGBMError as e:
        refused = str(e)
    after = timer_counts(lgb)
    p = bst.predict(X)
    return {"trees": bst.num_trees(), "finite": bool(np.all(np.isfinite(p))), "refused": refused,
            "log": [ln for ln in lines if "RF:" in ln], "grew": {t: after[t] - before[t] for t in BLEND_TIMERS}}


def _keep(holder):
    """a callback that records the timer counts before the continued booster's first iteration."""
    def cb(env):
        if not holder:
            import lambdagap_amd as lgb
            holder.append(timer_counts(lgb))
    cb.before_iteration = True
    cb.order = 0
    return cb


def main(what):
    torch = None
    if what in ("device", "metrics"):
        import torch  # before the library's first GPU call (tests/test_update_device.py)

        torch.zeros(1, device="cuda")
        torch.cuda.synchronize()
    import lambdagap_amd as lgb

    out = {}

    def run(key, fn, *args):
        # one failing run is reported under its own key; the others still report
        try:
            out[key] = fn(lgb, *args)
        except Exception as e:  # noqa: BLE001
            out[key] = {"error": f"{type(e).__name__}: {e}"}

    if what in ("device", "host"):
        for name in CASES:
            run(name, bitwise_run, name, what == "device", torch)
        run("rollback", rollback_run)
        if what == "device":
            for name in list(GATED) + ["init_model"]:
                run("gated_" + name, gated_run, name)
    elif what == "metrics":
        out = metrics_run(lgb)
    elif what == "bad_value":
        try:
            _booster(lgb, CASES["n3000"])[0].update()
            out = {"error": ""}
        except lgb.LightGBMError as e:
            out = {"error": str(e)}
    else:
        raise SystemExit(f"unknown run {what!r}")
    print("RESULT " + json.dumps(out))
    sys.stdout.flush()
