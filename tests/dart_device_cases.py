"""The runs behind tests/test_dart_device.py. LGAP_DEVICE_DART is read once per process, so each
path ("forest", unset: one traversal per tree, "0": host score) runs in a child interpreter that calls main() and
prints one ``RESULT <json>`` line; the parent compares the children's reports."""
from __future__ import annotations

import hashlib
import json
import sys

import numpy as np

N, F, LEAVES, ITERS = 2000, 10, 15, 30

BASE = {"boosting": "dart", "device_type": "gpu", "num_leaves": LEAVES, "min_data_in_leaf": 5, "verbosity": -1,
        "seed": 3, "drop_seed": 9, "objective": "none"}

# GOSS: the host sampler on every path (device_sampling=false). The device GOSS draws the host's
# bag but rescales the kept gradients in its own kernel, so only the host sampler hands the same
# fp32 gradients to the learner whether or not the boosting loop is device-resident. Device
# bagging draws the host's bags bit for bit and changes no gradient: it runs as configured.
CUSTOM_CASES = {
    "default": {},
    "uniform_drop": {"uniform_drop": True},
    "xgboost_dart_mode": {"xgboost_dart_mode": True},
    "skip0_max3": {"skip_drop": 0.0, "max_drop": 3},
    "drop_rate_half": {"drop_rate": 0.5},
    "three_classes": {"num_class": 3},
    "bagging": {"bagging_fraction": 0.7, "bagging_freq": 1},
    "goss": {"data_sample_strategy": "goss", "device_sampling": False},
    "categorical": {"categorical_feature": [0]},
    "valid": {"valid": True},
    # not compared bit for bit (see above): the device GOSS sampler with device-scored DART
    "goss_device": {"data_sample_strategy": "goss"},
}
BITWISE_CASES = [c for c in CUSTOM_CASES if c != "goss_device"]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_data(classes=1, categorical=False, n=N, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F))
    if categorical:
        X[:, 0] = rng.integers(0, 12, n)
    z = X[:, 1] + 0.5 * X[:, 2] * X[:, 3] + (X[:, 0] % 3 == 0) + rng.normal(size=n) * 0.5
    if classes == 1:
        y = (z > np.median(z)).astype(np.float64)
    else:
        y = np.digitize(z, np.quantile(z, np.linspace(0, 1, classes + 1)[1:-1])).astype(np.float64)
    return X, y


def objective(y, classes):
    """Logistic / softmax gradients in numpy from the raw score the library hands over."""
    if classes == 1:
        def fobj(preds, _):
            p = 1.0 / (1.0 + np.exp(-preds))
            return p - y, p * (1.0 - p)
        return fobj
    onehot = np.eye(classes)[y.astype(int)]

    def fobj(preds, _):  # preds: (N, K)
        e = np.exp(preds - preds.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
        return (p - onehot).T.ravel(), (2.0 * p * (1.0 - p)).T.ravel()
    return fobj


def _booster(lgb, extra, n=N):
    extra = dict(extra)
    classes = extra.get("num_class", 1)
    cat = extra.pop("categorical_feature", "auto")
    with_valid = extra.pop("valid", False)
    params = dict(BASE, **extra)
    X, y = make_data(classes, cat != "auto", n)
    train = lgb.Dataset(X, y, params=params, categorical_feature=cat)
    bst = lgb.Booster(params, train)
    if with_valid:
        Xv, yv = make_data(classes, cat != "auto", 700, seed=6)
        bst.add_valid(lgb.Dataset(Xv, yv, reference=train), "v")
    return bst, X, y, classes, with_valid


def custom_run(lgb, name):
    """model text, and the sha256 of the preds handed to the objective (and of the validation
    score read on the host) at every iteration."""
    bst, X, y, classes, with_valid = _booster(lgb, CUSTOM_CASES[name])
    inner = objective(y, classes)
    preds_sha, valid_sha = [], []

    def fobj(preds, ds):
        preds_sha.append(_sha(preds))
        return inner(preds, ds)

    track = EditTracker(classes)
    for _ in range(ITERS):
        bst.update(fobj=fobj)
        track.step(bst)
        if with_valid:
            valid_sha.append(_sha(bst._Booster__inner_predict(1)))
    out = {"model": bst.model_to_string(), "preds": preds_sha, "valid": valid_sha, "trees": bst.num_trees()}
    # the final scores next to predictions of the final model (no objective: the reads are raw); the
    # read must not drop trees for an iteration that never comes
    bst.reset_parameter({"skip_drop": 1.0})
    out.update(track.report())
    out["train_diff"] = float(np.max(np.abs(bst._Booster__inner_predict(0) - bst.predict(X, raw_score=True))))
    if with_valid:
        Xv, _ = make_data(classes, CUSTOM_CASES[name].get("categorical_feature") is not None, 700, seed=6)
        out["valid_diff"] = float(np.max(np.abs(bst._Booster__inner_predict(1) - bst.predict(Xv, raw_score=True))))
    return out


def rollback_run(lgb):
    bst, X, y, classes, _ = _booster(lgb, {})
    fobj = objective(y, classes)
    for _ in range(8):
        bst.update(fobj=fobj)
    bst.rollback_one_iter()
    bst.update(fobj=fobj)
    return {"model": bst.model_to_string(), "trees": bst.num_trees()}


def linear_run(lgb):
    """DART with linear leaves trains; the library says where the score lives."""
    lines = []
    lgb.register_logger(_ListLogger(lines))
    X, y = make_data()
    params = dict(BASE, objective="regression", linear_tree=True, verbosity=1)
    bst = lgb.train(params, lgb.Dataset(X, y, params=params), num_boost_round=5)
    p = bst.predict(X)
    return {"trees": bst.num_trees(), "finite": bool(np.all(np.isfinite(p))),
            "log": [ln for ln in lines if "DART" in ln]}


class _ListLogger:
    def __init__(self, lines):
        self.lines = lines

    def info(self, msg):
        self.lines.append(str(msg))

    def warning(self, msg):
        self.lines.append(str(msg))


def _leaf_max(model_text):
    """max |leaf value| of every tree of a model text."""
    return [float(np.max(np.abs(np.array(ln.split("=", 1)[1].split(), dtype=np.float64))))
            for ln in model_text.splitlines() if ln.startswith("leaf_value=")]


def _logloss(y, p):
    eps = 1e-15
    p = np.clip(p, eps, 1.0 - eps)
    return float(np.mean(np.where(y > 0, -np.log(p), -np.log(1.0 - p))))


def _auc(y, s):
    order = np.argsort(s, kind="mergesort")
    s, y = s[order], y[order]
    # average ranks over ties
    ranks = np.empty(len(s))
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


class EditTracker:
    """The score edits of a DART run, recovered from the model text after every iteration: a tree
    whose leaf values changed over the iteration was dropped in it. Per class, E counts the edits
    applied to a row of the training score (each dropped tree subtracted and re-added, the new tree
    added) and S sums the edited tree's largest |leaf| over them (a re-added tree's k / (k + 1) of
    it is bounded by the same); v_E / v_S are the same for a validation score (each dropped tree's
    correction, below its old |leaf|, and the new tree)."""

    def __init__(self, classes=1):
        self.k = classes
        self.before = []
        self.E, self.S = [0] * classes, [0.0] * classes
        self.v_E, self.v_S = [0] * classes, [0.0] * classes

    def step(self, bst):
        after = _leaf_max(bst.model_to_string())
        for j in range(len(after)):
            c = j % self.k
            if j >= len(self.before):  # this iteration's tree
                self.E[c] += 1
                self.S[c] += after[j]
                self.v_E[c] += 1
                self.v_S[c] += after[j]
            elif after[j] != self.before[j]:
                self.E[c] += 2
                self.S[c] += 2.0 * self.before[j]
                self.v_E[c] += 1
                self.v_S[c] += self.before[j]
        self.before = after

    def report(self):
        """2^-52 * E * S of the worst class (test_dart_device.py derives the bound), and the edits."""
        return {"bound": max(2.0 ** -52 * e * s for e, s in zip(self.E, self.S)),
                "v_bound": max(2.0 ** -52 * e * s for e, s in zip(self.v_E, self.v_S)),
                "edits": max(self.E), "trees": len(self.before)}


def _logit_with_slack(p):
    """The raw score behind a probability the binary objective handed out, and how far that
    inversion can be off. The library's p = 1 / (1 + exp(-s)) carries a few roundings (exp, add,
    divide: taken as 4 ulp of p and of 1 - p), which ds/dp = 1 / (p (1 - p)) turns into at most
    4 * 2^-53 / (p (1 - p)) of s; numpy's log(p) - log1p(-p) adds an ulp of each logarithm and of
    their difference, at most 2^-52 * (|log p| + |log(1 - p)|)."""
    lp, lq = np.log(p), np.log1p(-p)
    return lp - lq, 4 * 2.0 ** -53 / (p * (1.0 - p)) + 2.0 ** -52 * (np.abs(lp) + np.abs(lq))


def builtin_run(lgb, torch=None):
    """objective=binary: the phase report, every iteration's metrics next to the same metrics
    recomputed on the host from the raw scores read back (through raw_score_device, so in device
    mode only: the host read hands out probabilities, whose rounding ties scores that the raw
    order separates), and the final incremental raw scores next to predict(raw_score=True), with
    the rounding bound of the run. In device mode the raw scores come from raw_score_device; the
    host-scored run inverts the probabilities it reads and reports each row's difference less the
    inversion's own error (_logit_with_slack)."""
    params = dict(BASE, objective="binary", metric=["binary_logloss", "auc"], boost_from_average=False)
    X, y = make_data()
    Xv, yv = make_data(n=700, seed=6)
    train = lgb.Dataset(X, y, params=params)
    bst = lgb.Booster(params, train)
    bst.add_valid(lgb.Dataset(Xv, yv, reference=train), "v")
    reported, recomputed = [], []
    track = EditTracker()
    for it in range(ITERS):
        bst.update()
        track.step(bst)
        if it == ITERS - 1:
            # the read below must not drop trees for an iteration that never comes
            bst.reset_parameter({"skip_drop": 1.0})
        ev = {(d, m): v for d, m, v, _ in bst.eval_train() + bst.eval_valid()}
        reported.append([ev[("training", "binary_logloss")], ev[("v", "auc")]])
        if torch is not None:
            raw_train = bst.raw_score_device(0).cpu().numpy()
            raw_valid = bst.raw_score_device(1).cpu().numpy()
            recomputed.append([_logloss(y, 1.0 / (1.0 + np.exp(-raw_train))), _auc(yv, raw_valid)])
    fresh_train, fresh_valid = bst.predict(X, raw_score=True), bst.predict(Xv, raw_score=True)
    if torch is not None:
        slack_t = slack_v = 0.0
    else:
        raw_train, slack_t = _logit_with_slack(bst._Booster__inner_predict(0))
        raw_valid, slack_v = _logit_with_slack(bst._Booster__inner_predict(1))
    out = track.report()
    out.update({"report": lgb.phase_timer_report(), "reported": reported, "recomputed": recomputed,
                "train_diff": float(np.max(np.abs(raw_train - fresh_train))),
                "valid_diff": float(np.max(np.abs(raw_valid - fresh_valid))),
                "train_excess": float(np.max(np.abs(raw_train - fresh_train) - slack_t)),
                "valid_excess": float(np.max(np.abs(raw_valid - fresh_valid) - slack_v))})
    return out


def torch_run(lgb, torch):
    """raw_score_device(0) of a DART booster next to the host read of the training score."""
    bst, X, y, classes, _ = _booster(lgb, {})
    fobj = objective(y, classes)
    same = []
    for _ in range(12):
        bst.update(fobj=fobj)
        dev = bst.raw_score_device(0).cpu().numpy()  # the first read of the iteration: it drops
        host = bst._Booster__inner_predict(0)
        same.append(dev.tobytes() == host.tobytes())
    refused = ""
    try:
        bst.update_device(lambda preds, ds: (torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")))
    except lgb.LightGBMError as e:
        refused = str(e)
    return {"same": same, "refused": refused, "trees": bst.num_trees()}


def main(what):
    torch = None
    if what == "builtin_torch":
        import torch  # before the library's first GPU call (tests/test_update_device.py)

        torch.zeros(1, device="cuda")
        torch.cuda.synchronize()
    import lambdagap_amd as lgb

    out = {}
    if what == "custom":
        for name in CUSTOM_CASES:
            out[name] = custom_run(lgb, name)
        out["rollback"] = rollback_run(lgb)
        out["linear"] = linear_run(lgb)
    elif what == "builtin":
        out = builtin_run(lgb)
    elif what == "builtin_torch":
        out = builtin_run(lgb, torch)
        out["torch"] = torch_run(lgb, torch)
    elif what == "unknown_value":
        try:
            bst = _booster(lgb, {})[0]
            bst.update(fobj=lambda preds, ds: (preds, np.ones_like(preds)))
            out = {"error": ""}
        except lgb.LightGBMError as e:
            out = {"error": str(e)}
    else:
        raise SystemExit(f"unknown run {what!r}")
    print("RESULT " + json.dumps(out))
    sys.stdout.flush()
