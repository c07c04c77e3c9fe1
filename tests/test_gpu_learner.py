"""HIP tree learner vs the CPU oracle learner (same data, same parameters)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _auc(y, p):
    from sklearn.metrics import roc_auc_score

    return roc_auc_score(y, p)


def _train(lgb, X, y, device, rounds=1, **kw):
    params = {"objective": "binary", "num_leaves": 31, "device_type": device, "verbosity": -1,
              "min_data_in_leaf": 20, "seed": 1, "deterministic": True}
    params.update(kw)
    ds = lgb.Dataset(X, y, params=params)
    return lgb.train(params, ds, rounds, keep_training_booster=True)  # device_name() needs the live learner


def _trees(b):
    return b.dump_model()["tree_info"]


def _splits(node, out):
    if "split_index" in node:
        out.append((node["split_feature"], node["threshold"], node["default_left"]))
        _splits(node["left_child"], out)
        _splits(node["right_child"], out)
    return out


@pytest.mark.parametrize("extra", [{}, {"lambda_l1": 1.0, "lambda_l2": 2.0},
                                   {"max_depth": 4}, {"path_smooth": 5.0},
                                   {"min_sum_hessian_in_leaf": 5.0, "max_delta_step": 0.7}])
@pytest.mark.parametrize("use_dp", [True, False])
def test_first_tree_matches_cpu(lgb, gpu_required, rng, extra, use_dp):
    from lambdagap_amd.utils import make_higgs_like

    X, y = make_higgs_like(40000, seed=5)
    bc = _train(lgb, X, y, "cpu", **extra)
    bg = _train(lgb, X, y, "gpu", gpu_use_dp=use_dp, **extra)
    assert "gfx950" in bg.device_name() or "MI3" in bg.device_name()
    tc, tg = _trees(bc)[0], _trees(bg)[0]
    assert tc["num_leaves"] == tg["num_leaves"]
    assert _splits(tc["tree_structure"], []) == _splits(tg["tree_structure"], [])
    pc, pg = bc.predict(X[:5000], raw_score=True), bg.predict(X[:5000], raw_score=True)
    # fp32 LDS histograms (the reference GPU learner's default) vs fp64 (gpu_use_dp)
    tol = 1e-7 if use_dp else 5e-3 * np.abs(pc).max()
    np.testing.assert_allclose(pg, pc, rtol=0, atol=tol)


def test_missing_values_and_categorical(lgb, gpu_required, rng):
    n = 30000
    X = rng.standard_normal((n, 6))
    X[rng.random(n) < 0.2, 0] = np.nan
    X[rng.random(n) < 0.5, 1] = 0.0
    X[:, 2] = rng.integers(0, 12, n)
    # majority of three effects (missing-aware numeric, categorical, zero-heavy numeric): every
    # effect has a clear main-effect gain, unlike an XOR target whose early splits are noise ties
    votes = (np.nan_to_num(X[:, 0]) > 0.3).astype(int) + (X[:, 2] % 3 == 0) + (X[:, 1] > 0.5)
    y = (votes >= 2).astype(float)
    kw = {"categorical_feature": [2], "max_cat_to_onehot": 4}
    bc = _train(lgb, X, y, "cpu", rounds=3, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=3, gpu_use_dp=True, **kw)
    tc, tg = _trees(bc)[0], _trees(bg)[0]
    # the first three pre-order splits resolve the three effects; deeper splits of the (then
    # pure) leaves have ~0 gain and are decided by summation-order rounding
    sc = [s[:2] for s in _splits(tc["tree_structure"], [])][:3]
    sg = [s[:2] for s in _splits(tg["tree_structure"], [])][:3]
    assert sc == sg
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=0, atol=2e-2)


def test_auc_parity_with_cpu_oracle(lgb, gpu_required):
    """BASELINE.md accuracy criterion: |AUC_gpu - AUC_cpu| <= 1e-3 on identical synthetic data."""
    from lambdagap_amd.utils import make_higgs_like

    X, y = make_higgs_like(200000, seed=11)
    Xv, yv = make_higgs_like(50000, seed=12)
    kw = {"num_leaves": 63, "learning_rate": 0.1, "min_data_in_leaf": 1, "min_sum_hessian_in_leaf": 100}
    bc = _train(lgb, X, y, "cpu", rounds=40, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=40, **kw)
    ac, ag = _auc(yv, bc.predict(Xv)), _auc(yv, bg.predict(Xv))
    assert abs(ac - ag) <= 1e-3, (ac, ag)


def test_fixed_point_vs_fp64_histograms_auc_1m(lgb, gpu_required):
    """Precision of the default fixed-point histograms at scale: 1M Higgs-shape rows, 63 leaves,
    30 iterations; held-out AUC of the fixed-point learner, of gpu_use_dp=true (fp64) and of the
    CPU oracle on the same bins agree within 1e-3 (docs/GPU-Performance.rst:136 tolerance)."""
    from lambdagap_amd.utils import make_higgs_like

    X, y = make_higgs_like(1_000_000, seed=21)
    Xv, yv = make_higgs_like(200_000, seed=22)
    base = {"objective": "binary", "num_leaves": 63, "learning_rate": 0.1, "min_data_in_leaf": 1,
            "min_sum_hessian_in_leaf": 100, "verbosity": -1}
    ds = lgb.Dataset(X, y, params=dict(base, device_type="cpu"), free_raw_data=False).construct()
    aucs = {}
    for name, extra in (("fixed", {"device_type": "gpu"}), ("fp64", {"device_type": "gpu", "gpu_use_dp": True}),
                        ("cpu", {"device_type": "cpu"})):
        b = lgb.train(dict(base, **extra), ds, 30, keep_training_booster=True)
        aucs[name] = _auc(yv, b.predict(Xv))
    assert abs(aucs["fixed"] - aucs["fp64"]) < 1e-3, aucs
    assert abs(aucs["fixed"] - aucs["cpu"]) < 1e-3, aucs
    assert abs(aucs["fp64"] - aucs["cpu"]) < 1e-3, aucs


def _heavy_tailed(rng, n, nf=8):
    X = rng.standard_normal((n, nf)).astype(np.float32)
    f = np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1] * X[:, 2] + np.where(X[:, 3] > 0.5, 1.0, -0.3)
    return X, f


def test_fixed_point_heavy_tailed_regression_10m(lgb, gpu_required):
    """Fixed-point precision at scale with heavy-tailed gradients: 10M rows of L2 regression
    whose target carries Student-t(1.5) noise (infinite variance) and rare 1e4-times outliers,
    so max|g| is ~1e5 times the typical |g|. The held-out L2 (against the noise-free target)
    of the default fixed-point learner and of gpu_use_dp=true (fp64-equivalent accumulation)
    agree within 0.1%. The per-block scale is bounded by sum|g| as well as rows * max|g|
    (frontier.h FixedPointExp), so one outlier does not set every row's quantum."""
    rng = np.random.default_rng(31)
    n = 10_000_000
    X, f = _heavy_tailed(rng, n)
    y = f + rng.standard_t(1.5, n)
    out = rng.random(n) < 1e-5
    y[out] *= 1e4
    Xv, fv = _heavy_tailed(rng, 500_000)
    base = {"objective": "regression", "num_leaves": 63, "learning_rate": 0.1, "min_data_in_leaf": 100,
            "verbosity": -1, "device_type": "gpu"}
    ds = lgb.Dataset(X, y, params=base, free_raw_data=False).construct()
    del X
    l2 = {}
    for name, extra in (("fixed", {}), ("fp64", {"gpu_use_dp": True})):
        b = lgb.train(dict(base, **extra), ds, 30, keep_training_booster=True)
        l2[name] = float(np.mean((b.predict(Xv) - fv) ** 2))
    assert abs(l2["fixed"] - l2["fp64"]) <= 1e-3 * l2["fp64"], l2


@pytest.mark.parametrize("objective,extra", [("regression", {}), ("huber", {"alpha": 0.8}),
                                             ("poisson", {}), ("multiclass", {"num_class": 3}),
                                             ("multiclassova", {"num_class": 3}),
                                             ("multiclassova", {"num_class": 3, "is_unbalance": True}),
                                             ("regression_l1", {}), ("quantile", {"alpha": 0.3}),
                                             ("mape", {}), ("regression_l1", {"weighted": True}),
                                             ("quantile", {"alpha": 0.8, "bagging_fraction": 0.7,
                                                           "bagging_freq": 1})])
def test_objectives_on_device(lgb, gpu_required, rng, objective, extra):
    """Device gradients (pointwise, softmax, one-vs-all) and the device leaf renewal of L1 /
    quantile / MAPE (segment-sorted residual percentiles) against the CPU oracle."""
    n = 20000
    extra = dict(extra)
    weighted = extra.pop("weighted", False)
    X = rng.standard_normal((n, 8))
    if objective in ("multiclass", "multiclassova"):
        y = (np.digitize(X[:, 0] + 0.3 * X[:, 1], [-0.5, 0.5])).astype(float)
    elif objective == "poisson":
        y = rng.poisson(np.exp(0.5 * X[:, 0])).astype(float)
    else:
        y = 2 * X[:, 0] - X[:, 1] ** 2 + 0.1 * rng.standard_normal(n)
    if objective == "mape":
        y = np.abs(y) + 0.5
    w = rng.random(n) + 0.5 if weighted else None
    params = {"objective": objective, "num_leaves": 15, "verbosity": -1, "seed": 3, **extra}
    bc = lgb.train({**params, "device_type": "cpu"}, lgb.Dataset(X, y, weight=w), 5)
    bg = lgb.train({**params, "device_type": "gpu"}, lgb.Dataset(X, y, weight=w), 5)
    np.testing.assert_allclose(bg.predict(X[:2000], raw_score=True), bc.predict(X[:2000], raw_score=True),
                               rtol=1e-3, atol=1e-4)


def test_device_refit_matches_cpu(lgb, gpu_required, rng):
    """Booster.refit on the device (leaf sums of the device gradients over the leaf assignment,
    score delta applied on the device) equals the CPU refit."""
    n = 30000
    X = rng.standard_normal((n, 6))
    y = (X[:, 0] - 0.5 * X[:, 1] + 0.3 * rng.standard_normal(n) > 0).astype(float)
    X2 = rng.standard_normal((n, 6))
    y2 = (X2[:, 0] - 0.5 * X2[:, 1] + 0.3 * rng.standard_normal(n) > 0.2).astype(float)
    out = {}
    for dev in ("cpu", "gpu"):
        b = lgb.train({"objective": "binary", "num_leaves": 15, "verbosity": -1, "device_type": dev},
                      lgb.Dataset(X, y), 8)
        r = b.refit(X2, y2, decay_rate=0.5)
        out[dev] = r.predict(X2[:3000], raw_score=True)
    np.testing.assert_allclose(out["gpu"], out["cpu"], rtol=1e-4, atol=1e-4)


def test_device_position_bias_lambdarank(lgb, gpu_required, rng):
    """Unbiased LambdaRank (positions): position-adjusted scores and the Newton bias update run
    on the device; the model tracks the CPU learner's."""
    from lambdagap_amd.utils import make_ranking

    X, y, sizes = make_ranking(400, num_features=20, seed=4)
    pos = np.concatenate([np.arange(s) % 10 for s in sizes]).astype(np.int32)
    params = {"objective": "lambdarank", "num_leaves": 15, "verbosity": -1, "lambdarank_truncation_level": 10}
    bc = lgb.train({**params, "device_type": "cpu"}, lgb.Dataset(X, y, group=sizes, position=pos), 5)
    bg = lgb.train({**params, "device_type": "gpu"}, lgb.Dataset(X, y, group=sizes, position=pos), 5)
    pc, pg = bc.predict(X, raw_score=True), bg.predict(X, raw_score=True)
    assert np.corrcoef(pc, pg)[0, 1] > 0.999
    assert np.mean(np.abs(pc - pg)) < 5e-3 * np.mean(np.abs(pc))


@pytest.mark.parametrize("objective", ["lambdarank", "rank_xendcg"])
def test_device_long_queries(lgb, gpu_required, rng, objective):
    """Queries longer than the LDS-resident limit (2048 documents) run on the device in global
    scratch (reference cuda_rank_objective.cu:190,506) and match the CPU objective."""
    sizes = np.array([40, 3000, 77, 5001, 2049, 120], dtype=np.int32)
    n = int(sizes.sum())
    X = rng.standard_normal((n, 10))
    y = np.clip(np.round(1.5 + X[:, 0] + 0.5 * X[:, 1] + 0.3 * rng.standard_normal(n)), 0, 4)
    params = {"objective": objective, "num_leaves": 15, "verbosity": -1, "lambdarank_truncation_level": 20,
              "min_data_in_leaf": 50}
    bc = lgb.train({**params, "device_type": "cpu"}, lgb.Dataset(X, y, group=sizes), 3)
    bg = lgb.train({**params, "device_type": "gpu"}, lgb.Dataset(X, y, group=sizes), 3)
    pc, pg = bc.predict(X, raw_score=True), bg.predict(X, raw_score=True)
    assert np.corrcoef(pc, pg)[0, 1] > 0.999, objective
    assert np.mean(np.abs(pc - pg)) < 5e-3 * np.mean(np.abs(pc)) + 1e-6


ALL_TARGETS = ["ndcg", "lambdaloss-ndcg", "lambdaloss-ndcg-plus-plus", "bndcg", "lambdaloss-bndcg",
               "lambdaloss-bndcg-plus-plus", "precision", "arpk", "lambdaloss-arp1", "lambdaloss-arp2", "ranknet",
               "bin-ranknet", "lambdagap-s", "lambdagap-x", "lambdagap-s-plus", "lambdagap-x-plus",
               "lambdagap-s-plus-plus", "lambdagap-x-plus-plus"]
BINARY_TARGETS = {"bndcg", "lambdaloss-bndcg", "lambdaloss-bndcg-plus-plus", "precision", "arpk", "bin-ranknet",
                  "lambdagap-s", "lambdagap-x", "lambdagap-s-plus", "lambdagap-x-plus", "lambdagap-s-plus-plus",
                  "lambdagap-x-plus-plus"}


@pytest.mark.parametrize("target", ALL_TARGETS)
def test_lambdarank_targets_on_device(lgb, gpu_required, rng, target):
    from lambdagap_amd.utils import make_ranking

    X, y, sizes = make_ranking(300, num_features=20, seed=3)
    if target in BINARY_TARGETS:
        y = (y >= 3).astype(np.float32)
    params = {"objective": "lambdarank", "lambdarank_target": target, "num_leaves": 15, "verbosity": -1,
              "lambdarank_truncation_level": 10}
    bc = lgb.train({**params, "device_type": "cpu"}, lgb.Dataset(X, y, group=sizes), 3)
    # fp64 histograms: this test pins the objective; histogram precision is pinned elsewhere
    bg = lgb.train({**params, "device_type": "gpu", "gpu_use_dp": True}, lgb.Dataset(X, y, group=sizes), 3)
    pc, pg = bc.predict(X, raw_score=True), bg.predict(X, raw_score=True)
    # exact ties (empty bins) are broken as on the host; what remains is a rare near-tie (gains
    # ~1e-7 apart) flipped by 1-ulp float differences of the device lambdas
    # (test_gpu_kernels.py pins the gradients of all 18 targets against torch)
    assert np.corrcoef(pc, pg)[0, 1] > 0.9999
    assert np.mean(np.abs(pc - pg)) < 1e-3 * np.mean(np.abs(pc)), (np.mean(np.abs(pc - pg)), np.mean(np.abs(pc)))


def test_bagging_goss_feature_fraction_on_device(lgb, gpu_required):
    from lambdagap_amd.utils import make_higgs_like

    X, y = make_higgs_like(60000, seed=21)
    # device bagging draws the host's bags bit for bit (same per-1024-row LCG streams, also
    # across re-bags); GOSS with device_sampling=false runs the host sampler
    for kw in ({"bagging_fraction": 0.7, "bagging_freq": 1},
               {"pos_bagging_fraction": 0.8, "neg_bagging_fraction": 0.5, "bagging_freq": 2},
               {"data_sample_strategy": "goss", "learning_rate": 0.5, "device_sampling": False},
               {"feature_fraction": 0.6}, {"extra_trees": True}):
        bc = _train(lgb, X, y, "cpu", rounds=5, **kw)
        bg = _train(lgb, X, y, "gpu", rounds=5, **kw)
        np.testing.assert_allclose(bg.predict(X[:3000], raw_score=True), bc.predict(X[:3000], raw_score=True),
                                   rtol=1e-3, atol=1e-4)


def test_device_goss(lgb, gpu_required):
    """GOSS drawn on the device (fixed 4096-row tiles: exact top-k by |g*h| + the other_k smallest
    hash keys of the rest, rescaled) draws the host sampler's bag: same models either way."""
    from lambdagap_amd.utils import make_higgs_like

    X, y = make_higgs_like(100000, seed=23)
    Xv, yv = make_higgs_like(40000, seed=24)
    kw = {"data_sample_strategy": "goss", "learning_rate": 0.25, "top_rate": 0.2, "other_rate": 0.1}
    bc = _train(lgb, X, y, "cpu", rounds=20, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=20, **kw)
    bh = _train(lgb, X, y, "gpu", rounds=20, device_sampling=False, **kw)
    pg, ph = bg.predict(Xv, raw_score=True), bh.predict(Xv, raw_score=True)
    np.testing.assert_allclose(pg, ph, rtol=1e-5, atol=1e-5)
    ac, ag = _auc(yv, bc.predict(Xv)), _auc(yv, bg.predict(Xv))
    assert abs(ag - ac) < 1e-3, (ag, ac)


@pytest.mark.parametrize("features", [28, 100])
@pytest.mark.parametrize("kw", [{"bagging_fraction": 0.6, "bagging_freq": 1},
                                {"data_sample_strategy": "goss", "learning_rate": 0.5},
                                {"bagging_fraction": 0.5, "bagging_freq": 2, "objective": "multiclass", "num_class": 3}],
                         ids=["bagging", "goss", "multiclass-bagging"])
def test_bagged_score_update_walks_only_out_of_bag_rows(lgb, gpu_required, features, kw):
    """A bagged / GOSS frontier tree scores its in-bag rows from the partition's leaf segments and
    walks only the out-of-bag list the device sampler wrote (LeafMapScore + LaunchLeafMapList;
    reference gbdt.cpp:495-516). The host-sampled run draws the same bags but has no out-of-bag
    list, so every row walks the tree: the two must train the same model (a wrong score on any
    row changes the next trees' gradients). Narrow rows walk the packed rows, 100 features the
    group-major copy."""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((30000, features)).astype(np.float32)
    X[rng.random(X.shape) < 0.05] = np.nan
    y = (X[:, 0] + 0.5 * np.nan_to_num(X[:, 1]) ** 2 - X[:, 2] * (X[:, 3] > 0) > 0.3).astype(np.float32)
    if kw.get("objective") == "multiclass":
        y = (np.nan_to_num(X[:, 0]) > 0).astype(np.float32) + (np.nan_to_num(X[:, 1]) > 0.5)
    bd = _train(lgb, X, y, "gpu", rounds=12, **kw)
    bh = _train(lgb, X, y, "gpu", rounds=12, device_sampling=False, **kw)
    sd, sh = [], []
    for t in _trees(bd):
        _splits(t["tree_structure"], sd)
    for t in _trees(bh):
        _splits(t["tree_structure"], sh)
    assert sd == sh
    np.testing.assert_allclose(bd.predict(X[:5000], raw_score=True), bh.predict(X[:5000], raw_score=True),
                               rtol=1e-6, atol=1e-7)
    # the training score the device kept (every row: in-bag from the segments, out-of-bag walked)
    # equals the model's prediction (both transformed: the inner predict is the objective's output)
    inner = bd._Booster__inner_predict(0).reshape(-1)
    pred = bd.predict(X).reshape(-1)  # (multiclass: row-major, as the inner predict)
    np.testing.assert_allclose(inner, pred, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("transport", ["collective", "xgmi", "collective-quantized"])
def test_data_parallel_path_single_rank(lgb, gpu_required, transport):
    """The owner-computes data-parallel learner path (owner exchange of the histogram, owned-feature
    scan, candidate table, global counts) on a one-rank communicator must reproduce the
    single-device model, over RCCL collectives and over the xGMI in-kernel exchange."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LGAP_DP_TRANSPORT=transport.replace("-quantized", ""), LGAP_XGMI_TIMEOUT_S="20",
               DP_SELFTEST_QUANTIZED="1" if transport.endswith("quantized") else "0")
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "dp_selftest.py")], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["num_trees"] == [8, 8]
    assert res["dp_path"] and res["single_path"], res
    assert ("xGMI" in res["dp_name"]) == (transport == "xgmi"), res
    assert res["root_features_equal"]
    assert res["max_abs_diff"] < 1e-3, res
    # exact integer all-reduce: the pipelined exchange grows the bit-identical model
    assert res["pipeline_vs_serial_equal"], res


@pytest.mark.parametrize("world,transport", [(2, "collective"), (3, "collective"), (4, "collective"),
                                             (3, "allreduce"), (2, "collective-seq"), (2, "xgmi"), (3, "xgmi"),
                                             (4, "xgmi"), (3, "collective-quantized")])
def test_data_parallel_multirank_rehearsal(lgb, gpu_required, world, transport):
    """P ranks share the one GPU. "collective": the data-parallel FRONTIER engine, owner-computes
    (per-round exact reduce-scatter of the fixed-point histograms by feature-group owner through
    host-staged collectives, owner-only scans, per-child bests all-gathered, redundant select on
    every rank); "allreduce": the same engine with the per-round all-reduce and redundant scans
    of every feature; "collective-seq": the sequential chain's owner histogram exchange over
    the same collectives; "xgmi": the frontier engine's in-kernel exchange over IPC-mapped
    buffers (here all on one device): k_f_reduce adds every bin into its owner's receive chunk,
    k_f_pair_best pushes the per-child bests, the root sums are exchanged by k_fx_root, and no
    collective runs while a tree grows. Every rank must grow the identical model, and it must match
    the host data-parallel learner trained by the same ranks on the same bins."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    quantized = transport.endswith("-quantized")
    transport = transport.replace("-quantized", "")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", LGAP_DP_TRANSPORT=transport.replace("-seq", ""),
               LGAP_XGMI_TIMEOUT_S="20", DP_QUANTIZED="1" if quantized else "0")
    if transport == "collective-seq":
        env["LGAP_FRONTIER_DP"] = "0"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1",
                        "--nproc-per-node", str(world), os.path.join(root, "scripts", "dp_multirank.py")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["world"] == world
    assert "data-parallel" in res["device_name"], res
    assert ("xGMI" in res["device_name"]) == (transport == "xgmi"), res
    assert ("frontier engine" in res["device_name"]) == (transport in ("collective", "allreduce", "xgmi")), res
    if transport == "collective":
        assert "owner reduce-scatter" in res["device_name"], res
    if transport == "xgmi":
        assert "owner histogram chunks" in res["device_name"], res
    if transport == "allreduce":
        assert "all-reduce per round" in res["device_name"], res
    assert res["ranks_identical"], res
    assert res["num_trees"] == 10
    if quantized:
        # device and host quantizers round stochastically with different streams: the models
        # agree in quality, not split for split
        assert abs(res["auc_gpu"] - res["auc_cpu"]) < 5e-3, res
        return
    # unit hessians (l2): the split structure must match the host learner tree for tree
    assert res["identical_leading_trees"] == 10, res
    assert res["max_abs_diff_vs_cpu_dp"] < 1e-3, res
    assert abs(res["auc_gpu"] - res["auc_cpu"]) < 1e-3, res


@pytest.mark.parametrize("transport", ["collective", "xgmi"])
def test_feature_parallel_multirank_rehearsal(lgb, gpu_required, transport):
    """Device feature-parallel (every rank holds all rows, scans the features of the groups it
    owns, candidates exchanged into one table) on 3 ranks sharing the GPU: identical models on all
    ranks, equal to the host feature-parallel learner tree for tree."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", LGAP_DP_TRANSPORT=transport, LGAP_XGMI_TIMEOUT_S="20",
               DP_LEARNER="feature")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1",
                        "--nproc-per-node", "3", os.path.join(root, "scripts", "dp_multirank.py")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert "feature-parallel" in res["device_name"], res
    # the frontier engine (per-child bests all-gathered each round, or pushed over xGMI)
    assert "frontier engine" in res["device_name"], res
    assert ("xGMI" in res["device_name"]) == (transport == "xgmi"), res
    assert res["ranks_identical"], res
    assert res["identical_leading_trees"] == 10, res
    assert res["max_abs_diff_vs_cpu_dp"] < 1e-3, res


@pytest.mark.parametrize("world,transport,topk", [(2, "collective", 3), (3, "collective", 20), (4, "collective", 2),
                                                  (3, "xgmi", 3), (2, "xgmi", 20), (4, "xgmi", 2),
                                                  (3, "xgmi-wavescan", 3)])
def test_voting_parallel_multirank_rehearsal(lgb, gpu_required, world, transport, topk):
    """Device voting-parallel (PV-Tree: local scan, top-k vote all-gathered, elected features'
    histograms summed, global scan of the elected features only), P ranks sharing the GPU: every
    rank grows the identical model, equal to the host voting learner tree for tree. Both transports
    run on the frontier engine (all expansions of a round voted at once)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # "-wavescan": the local pass on the wave-per-item scan (the wide-data kernel; forced here)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", LGAP_DP_TRANSPORT=transport.replace("-wavescan", ""),
               LGAP_XGMI_TIMEOUT_S="20", DP_LEARNER="voting", DP_TOPK=str(topk))
    if transport.endswith("-wavescan"):
        env["LGAP_KERNEL"] = "scan_wave=1"
    transport = transport.replace("-wavescan", "")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1",
                        "--nproc-per-node", str(world), os.path.join(root, "scripts", "dp_multirank.py")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert "voting-parallel" in res["device_name"], res
    assert ("xGMI" in res["device_name"]) == (transport == "xgmi"), res
    # the frontier engine (local pass, top-k votes exchanged, elected rows summed exactly, global
    # pass per round): over collectives (all-gather + all-reduce) or pushed in-kernel over xGMI
    assert "frontier engine" in res["device_name"], res
    assert res["ranks_identical"], res
    assert res["num_trees"] == 10
    assert res["identical_leading_trees"] == 10, res
    assert res["max_abs_diff_vs_cpu_dp"] < 1e-3, res


@pytest.mark.parametrize("world,transport,extra", [
    (2, "xgmi", {"extra_trees": True}),
    (3, "xgmi", {"extra_trees": True, "top_k": 3}),
    (3, "xgmi", {"cegb_penalty_split": 0.002, "cegb_tradeoff": 0.5}),
    (2, "collective", {"cegb_penalty_split": 0.001, "top_k": 3}),
    (4, "xgmi", {"extra_trees": True, "top_k": 2}),
])
def test_voting_parallel_extra_trees_and_cegb_split(lgb, gpu_required, world, transport, extra):
    """Voting parallel with extra trees (the global pass redraws each elected feature's threshold
    from its stream in the host's order: smaller child's elected features, then the larger's) and
    with the CEGB split penalty (at the leaf's global count, as the reference's global pass) on the
    device frontier, P ranks sharing the GPU: identical models on every rank, equal to the host
    voting learner tree for tree. (Extra trees run over the in-kernel xGMI exchange; over
    collectives the factory keeps the host policy.)"""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    extra = dict(extra)
    topk = extra.pop("top_k", 20)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", LGAP_DP_TRANSPORT=transport, LGAP_XGMI_TIMEOUT_S="20",
               DP_LEARNER="voting", DP_TOPK=str(topk), DP_EXTRA=json.dumps(extra))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1",
                        "--nproc-per-node", str(world), os.path.join(root, "scripts", "dp_multirank.py")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert "voting-parallel" in res["device_name"] and "frontier engine" in res["device_name"], res
    assert "host split policy" not in res["device_name"], res
    assert res["ranks_identical"], res
    assert res["identical_leading_trees"] == 10, res
    assert res["max_abs_diff_vs_cpu_dp"] < 1e-3, res


def _policy_data(rng, n=20000):
    X = rng.standard_normal((n, 6))
    z = 1.5 * X[:, 0] - X[:, 1] + 0.7 * X[:, 2] * X[:, 3] + 0.3 * rng.standard_normal(n)
    return X, z


@pytest.mark.parametrize("extra", [{"interaction_constraints": [[0, 1], [1, 2, 3]]},
                                   {"interaction_constraints": [[0], [2, 3, 4], [1, 5]], "num_leaves": 15},
                                   # 100 sets (two 64-set words), the binding ones at positions 70 and 90
                                   {"interaction_constraints": [[5]] * 70 + [[0, 1]] + [[4]] * 19 + [[1, 2, 3]]
                                    + [[5]] * 9}])
def test_device_interaction_constraints(lgb, gpu_required, rng, extra):
    """Device-resident interaction constraints (per-leaf set masks, 64 sets per word) against the
    CPU learner."""
    X, z = _policy_data(rng)
    y = (z > 0).astype(float)
    bc = _train(lgb, X, y, "cpu", rounds=5, **extra)
    bg = _train(lgb, X, y, "gpu", rounds=5, gpu_use_dp=True, **extra)
    assert "host split policy" not in bg.device_name()
    sets = [set(c) for c in extra["interaction_constraints"]]

    def paths(n, acc):
        if "split_index" in n:
            f = n["split_feature"]
            yield from paths(n["left_child"], acc | {f})
            yield from paths(n["right_child"], acc | {f})
        else:
            yield acc
    for t in _trees(bg):
        for feats in paths(t["tree_structure"], set()):
            assert any(feats <= s for s in sets), feats
    tc, tg = _trees(bc)[0], _trees(bg)[0]
    assert [s[:2] for s in _splits(tc["tree_structure"], [])][:3] == [s[:2] for s in _splits(tg["tree_structure"], [])][:3]
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=0, atol=5e-2)


@pytest.mark.parametrize("renew", [False, True])
def test_device_quantized_training(lgb, gpu_required, rng, renew):
    """use_quantized_grad on the device-resident learner: integer-level gradients through the
    fixed-point histograms; accuracy tracks the full-precision model."""
    X, z = _policy_data(rng)
    y = (z > 0).astype(float)
    q = {"use_quantized_grad": True, "num_grad_quant_bins": 4, "quant_train_renew_leaf": renew}
    full = _train(lgb, X, y, "gpu", rounds=30)
    bq = _train(lgb, X, y, "gpu", rounds=30, **q)
    bq_cpu = _train(lgb, X, y, "cpu", rounds=30, **q)
    a_full, a_q, a_qc = _auc(y, full.predict(X)), _auc(y, bq.predict(X)), _auc(y, bq_cpu.predict(X))
    assert a_q > a_full - 0.01, (a_q, a_full)
    assert abs(a_q - a_qc) < 0.01, (a_q, a_qc)
    # deterministic rounding: the first split matches the host quantizer
    d = dict(q, stochastic_rounding=False)
    tc = _trees(_train(lgb, X, y, "cpu", rounds=1, **d))[0]["tree_structure"]
    tg = _trees(_train(lgb, X, y, "gpu", rounds=1, gpu_use_dp=True, **d))[0]["tree_structure"]
    assert (tc["split_feature"], tc["threshold"]) == (tg["split_feature"], tg["threshold"])


@pytest.mark.parametrize("bins", [4, 16, 254])
def test_device_quantized_integer_histograms(lgb, gpu_required, rng, bins, monkeypatch):
    """Quantized training on the frontier engine builds integer-level histograms (int8 g /
    uint8 h per row, packed g32|h32 sums): with deterministic rounding the whole first tree
    matches the host quantized learner, and the model matches the float-histogram path
    (LGAP_KERNEL=quant_hist=off) in accuracy. 254 bins: the widest levels the packing holds
    (h levels up to 254, beyond int8 on the host too)."""
    X, z = _policy_data(rng)
    y = (z > 0).astype(float)
    d = {"use_quantized_grad": True, "num_grad_quant_bins": bins, "stochastic_rounding": False}
    tc = _trees(_train(lgb, X, y, "cpu", rounds=1, **d))[0]["tree_structure"]
    bg = _train(lgb, X, y, "gpu", rounds=1, **d)
    assert "frontier" in bg.device_name()
    tg = _trees(bg)[0]["tree_structure"]
    assert [s[:2] for s in _splits(tc, [])] == [s[:2] for s in _splits(tg, [])]
    q = {"use_quantized_grad": True, "num_grad_quant_bins": bins}
    a_int = _auc(y, _train(lgb, X, y, "gpu", rounds=30, **q).predict(X))
    a_cpu = _auc(y, _train(lgb, X, y, "cpu", rounds=30, **q).predict(X))
    monkeypatch.setenv("LGAP_KERNEL", "quant_hist=off")
    a_flt = _auc(y, _train(lgb, X, y, "gpu", rounds=30, **q).predict(X))
    assert abs(a_int - a_cpu) < 5e-3, (a_int, a_cpu)
    assert abs(a_int - a_flt) < 5e-3, (a_int, a_flt)


def test_device_quantized_regression_tracks_cpu(lgb, gpu_required):
    """Integer-level histograms on a regression (non-constant range of gradients, 255 leaves):
    the held-out l2 of the device quantized model tracks the host quantized learner's (4 levels
    cost both the same accuracy against fp gradients)."""
    from lambdagap_amd.utils import make_regression

    X, y = make_regression(60000, num_features=40, seed=7)
    Xv, yv = make_regression(20000, num_features=40, seed=8)
    p = {"objective": "regression", "num_leaves": 255, "max_bin": 63, "verbosity": -1,
         "use_quantized_grad": True, "num_grad_quant_bins": 4, "seed": 3}
    l2 = {}
    for dev in ("cpu", "gpu"):
        b = lgb.train({**p, "device_type": dev}, lgb.Dataset(X, y), 30)
        l2[dev] = float(np.mean((b.predict(Xv) - yv) ** 2))
    assert abs(l2["gpu"] - l2["cpu"]) < 0.03 * l2["cpu"], l2


@pytest.mark.parametrize("extra", [{"cegb_penalty_split": 0.05, "feature_fraction_bynode": 0.8,
                                    "cegb_penalty_feature_lazy": [0.01, 0.02, 0.03, 0.04, 0.05, 0.06]}])
def test_host_policy_over_device_histograms(lgb, gpu_required, rng, extra):
    """Options only the host learners implement run the host split policy over HIP histograms
    (the reference's GPUTreeLearner arrangement); the model matches the CPU learner."""
    X, z = _policy_data(rng)
    y = z if extra.get("objective") == "regression" else (z > 0).astype(float)
    bc = _train(lgb, X, y, "cpu", rounds=4, **extra)
    bg = _train(lgb, X, y, "gpu", rounds=4, gpu_use_dp=True, **extra)
    assert "host split policy" in bg.device_name()
    tc, tg = _trees(bc)[0], _trees(bg)[0]
    assert [s[:2] for s in _splits(tc["tree_structure"], [])][:4] == [s[:2] for s in _splits(tg["tree_structure"], [])][:4]
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=1e-3, atol=1e-3)


def _monotone_reference_xy(rng, x3_to_category, n=3000):
    """the data of test_policies._reference_monotone_set (reference test_engine.py:2118-2146)"""
    x1, x2, x3 = rng.uniform(size=n), rng.uniform(size=n), rng.uniform(size=n)
    X = np.column_stack((x1, x2, np.digitize(x3, bins=np.arange(0, 1, 0.01)) if x3_to_category else x3))
    s = 10.0 * (rng.uniform(size=6) + 0.5)
    y = (s[0] * x1 + np.sin(s[1] * np.pi * x1) - s[2] * x2 - np.cos(s[3] * np.pi * x2) - s[4] * x3
         - np.cos(s[5] * np.pi * x3) + rng.normal(0.0, 0.01, size=n))
    return X, y


@pytest.mark.parametrize("x3_to_category", [True, False])
@pytest.mark.parametrize("interactions", [True, False])
@pytest.mark.parametrize("method", ["intermediate", "advanced"])
def test_device_monotone_constraints_reference_cases(lgb, gpu_required, rng, x3_to_category, interactions, method):
    """Intermediate / advanced monotone constraints with device_type=gpu: the leaves' histograms
    stay on the device and every scan (children and the constraint walk's rescans, with flat or
    per-threshold bounds) runs there (device/policy_scan.h). The reference's test_monotone_constraints
    cases hold, and the trees equal the CPU learner's split for split."""
    from lambdagap_amd.basic import Dataset

    X, y = _monotone_reference_xy(rng, x3_to_category)
    params = {"objective": "regression", "min_data": 20, "num_leaves": 20, "monotone_constraints": [1, -1, 0],
              "monotone_constraints_method": method, "use_missing": False, "verbosity": -1, "gpu_use_dp": True,
              "deterministic": True}
    if interactions:
        params["interaction_constraints"] = [[0], [1], [2]]
    cat = [2] if x3_to_category else []
    models = {}
    for dev in ("cpu", "gpu"):
        p = dict(params, device_type=dev)
        models[dev] = lgb.train(p, Dataset(X, y, categorical_feature=cat, params=p), 30, keep_training_booster=True)
    bg, bc = models["gpu"], models["cpu"]
    # intermediate: the frontier select walks the constraints; advanced: device scans, host walk
    want = "intermediate monotone walk" if method == "intermediate" else "split scans"
    assert "host split policy" not in bg.device_name() and want in bg.device_name(), bg.device_name()
    n = 1000
    v = np.linspace(0, 1, n).reshape((n, 1))
    for fixed in np.linspace(0, 1, n)[:10]:
        fx = fixed * np.ones((n, 1))
        assert (np.diff(bg.predict(np.column_stack((v, fx, fx)))) >= 0).all()
        assert (np.diff(bg.predict(np.column_stack((fx, v, fx)))) <= 0).all()
    tc, tg = _trees(bc), _trees(bg)
    assert [t["num_leaves"] for t in tc] == [t["num_leaves"] for t in tg]
    for a, b in zip(tc[:5], tg[:5]):
        assert [s[:2] for s in _splits(a["tree_structure"], [])] == [s[:2] for s in _splits(b["tree_structure"], [])]
    np.testing.assert_allclose(bg.predict(X), bc.predict(X), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("extra", [
    {},
    {"num_leaves": 63, "objective": "regression"},
    # (a regression target: a binary one at 127 leaves leaves pure nodes whose gains are rounding
    # noise, ~1e-14, where CPU and device sums legitimately order differently -- basic too)
    {"num_leaves": 127, "objective": "regression", "n": 60000},
    {"path_smooth": 1.5, "lambda_l1": 0.3, "max_depth": 8},
    {"monotone_penalty": 0.5, "lambda_l2": 1.0},
    {"interaction_constraints": [[0, 1, 2], [1, 3, 4, 5]], "num_leaves": 47},
    # (max_delta_step puts this data's gains at rounding-noise level, ~1e-13, for basic too)
    {"bagging_fraction": 0.6, "bagging_freq": 1, "objective": "regression"},
])
def test_frontier_intermediate_monotone_matches_cpu(lgb, gpu_required, rng, extra):
    """Intermediate monotone constraints in the frontier engine's select (FMonoCommit: the host's
    constraint walk per committed split, stale leaves re-scanned from their slots): the trees equal
    the CPU learner's split for split, in the same order, and the model is monotone."""
    extra = dict(extra)
    n = extra.pop("n", 20000)
    X, z = _policy_data(rng, n)
    obj = extra.pop("objective", "binary")
    y = z if obj == "regression" else (z > 0).astype(float)
    kw = dict(extra, objective=obj, monotone_constraints=[1, -1, 1, 0, -1, 0],
              monotone_constraints_method="intermediate")
    kw.setdefault("num_leaves", 31)
    bc = _train(lgb, X, y, "cpu", rounds=8, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=8, gpu_use_dp=True, **kw)
    assert "frontier engine, intermediate monotone walk" in bg.device_name(), bg.device_name()
    tc, tg = _trees(bc), _trees(bg)
    assert [t["num_leaves"] for t in tc] == [t["num_leaves"] for t in tg]
    for a, b in zip(tc, tg):
        sa, sb = _splits_in_order(a["tree_structure"]), _splits_in_order(b["tree_structure"])
        assert [x[:2] for x in sa] == [x[:2] for x in sb]
        np.testing.assert_allclose([x[2] for x in sa], [x[2] for x in sb], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=1e-6, atol=1e-6)
    grid = np.linspace(-3, 3, 60)
    for row in X[:8]:
        for f, sign in ((0, 1), (1, -1), (2, 1), (4, -1)):
            Z = np.repeat(row[None, :], len(grid), 0)
            Z[:, f] = grid
            assert np.all(sign * np.diff(bg.predict(Z, raw_score=True)) >= -1e-10)


@pytest.mark.parametrize("extra", [{"use_quantized_grad": True, "num_grad_quant_bins": 4},
                                   {"categorical": True, "num_leaves": 63},
                                   {"max_delta_step": 0.6, "objective": "regression", "num_leaves": 63}])
def test_frontier_intermediate_monotone_other_modes(lgb, gpu_required, rng, extra):
    """Intermediate monotone constraints on the frontier with quantized gradients (integer-level
    histograms in the slots the rescans read), a categorical feature (bounds clamp its outputs),
    and max_delta_step (no gain bound for stale records: every stale leaf is re-scanned before the
    next commit): the model is monotone in the constrained features and tracks the CPU learner."""
    extra = dict(extra)
    X, z = _policy_data(rng, 30000)
    cat = extra.pop("categorical", False)
    if cat:
        X[:, 5] = rng.integers(0, 12, len(X))
        z = z + 0.3 * (X[:, 5] % 4)
    obj = extra.pop("objective", "binary")
    y = z if obj == "regression" else (z > 0).astype(float)
    kw = dict(extra, objective=obj, monotone_constraints=[1, -1, 1, 0, -1, 0],
              monotone_constraints_method="intermediate")
    if cat:
        kw["categorical_feature"] = [5]
    bc = _train(lgb, X, y, "cpu", rounds=8, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=8, **kw)
    assert "frontier engine, intermediate monotone walk" in bg.device_name(), bg.device_name()
    pc, pg = bc.predict(X), bg.predict(X)
    if obj == "regression":
        lc, lg_ = float(np.mean((pc - y) ** 2)), float(np.mean((pg - y) ** 2))
    else:
        eps = 1e-12
        lc = float(-np.mean(y * np.log(pc + eps) + (1 - y) * np.log(1 - pc + eps)))
        lg_ = float(-np.mean(y * np.log(pg + eps) + (1 - y) * np.log(1 - pg + eps)))
    # (quantized gradients: the device and host quantizers draw differently; same loss level)
    assert abs(lg_ - lc) < 0.03 * lc, (lg_, lc)
    grid = np.linspace(-3, 3, 60)
    for row in X[:8]:
        for f, sign in ((0, 1), (1, -1), (2, 1), (4, -1)):
            Z = np.repeat(row[None, :], len(grid), 0)
            Z[:, f] = grid
            assert np.all(sign * np.diff(bg.predict(Z, raw_score=True)) >= -1e-10)


@pytest.mark.parametrize("method", ["intermediate", "advanced"])
def test_device_monotone_scans_default_precision(lgb, gpu_required, rng, method):
    """The default device_type=gpu setup (gpu_use_dp unset: fp32 (g, h) with fixed-point histogram
    sums) routes intermediate / advanced monotone constraints to the device-resident scans too. Sums
    differ from the CPU learner's doubles in the last bits, so the check is the constraint itself
    plus agreement in prediction, not split-for-split equality."""
    X, z = _policy_data(rng)
    y = (z > 0).astype(float)
    kw = {"objective": "binary", "monotone_constraints": [1, -1, 0, 0, 0, 0], "monotone_constraints_method": method}
    bc = _train(lgb, X, y, "cpu", rounds=10, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=10, **kw)
    want = "intermediate monotone walk" if method == "intermediate" else "split scans"
    assert want in bg.device_name(), bg.device_name()
    pc, pg = bc.predict(X), bg.predict(X)
    assert np.mean(np.abs(pg - pc)) < 5e-3, np.mean(np.abs(pg - pc))
    grid = np.linspace(-3, 3, 50)
    for row in X[:10]:
        r = np.tile(row, (50, 1))
        r[:, 0] = grid
        assert (np.diff(bg.predict(r)) >= -1e-12).all()
        r = np.tile(row, (50, 1))
        r[:, 1] = grid
        assert (np.diff(bg.predict(r)) <= 1e-12).all()


@pytest.mark.parametrize("extra", [
    {"monotone_constraints_method": "advanced", "bagging_fraction": 0.7, "bagging_freq": 1, "lambda_l1": 0.5,
     "path_smooth": 2.0, "max_depth": 7},
    {"monotone_constraints_method": "intermediate", "cegb_penalty_split": 0.02, "min_data_in_leaf": 40,
     "monotone_penalty": 1.0},
    {"monotone_constraints_method": "advanced", "objective": "regression", "max_delta_step": 0.5, "num_leaves": 63},
])
def test_device_monotone_scans_with_other_policies(lgb, gpu_required, rng, extra):
    """The device scans of the monotone policies combined with bagging, L1 / path smoothing /
    max_delta_step, the CEGB split penalty (applied on the host to the device's records) and the
    monotone split penalty: trees equal the CPU learner's, outputs monotone in the constrained
    features."""
    X, z = _policy_data(rng)
    extra = dict(extra)
    obj = extra.pop("objective", "binary")
    y = z if obj == "regression" else (z > 0).astype(float)
    kw = dict(extra, objective=obj, monotone_constraints=[1, -1, 0, 0, 0, 0])
    bc = _train(lgb, X, y, "cpu", rounds=6, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=6, gpu_use_dp=True, **kw)
    # (the CEGB split penalty keeps intermediate on the host walk over device scans)
    assert "split scans" in bg.device_name(), bg.device_name()
    tc, tg = _trees(bc), _trees(bg)
    assert [t["num_leaves"] for t in tc] == [t["num_leaves"] for t in tg]
    for a, b in zip(tc, tg):
        assert [s[:2] for s in _splits(a["tree_structure"], [])] == [s[:2] for s in _splits(b["tree_structure"], [])]
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=1e-6, atol=1e-6)
    grid = np.linspace(-3, 3, 50)
    for row in X[:10]:
        Z = np.repeat(row[None, :], len(grid), 0)
        Z[:, 0] = grid
        assert np.all(np.diff(bg.predict(Z, raw_score=True)) >= -1e-10)
        Z = np.repeat(row[None, :], len(grid), 0)
        Z[:, 1] = grid
        assert np.all(np.diff(bg.predict(Z, raw_score=True)) <= 1e-10)


@pytest.mark.parametrize("extra", [{"cegb_penalty_split": 0.1},
                                   {"cegb_penalty_split": 0.05, "cegb_tradeoff": 0.5, "num_leaves": 63},
                                   {"cegb_penalty_split": 0.02, "extra_trees": True}])
def test_device_cegb_split_penalty(lgb, gpu_required, rng, extra):
    """CEGB's split penalty (tradeoff x penalty_split x rows of the leaf) is applied by the device
    scans (frontier engine, and the sequential chain with extra_trees): no host split policy, and
    the model matches the CPU learner's, whose penalty prunes splits of small leaves."""
    X, z = _policy_data(rng)
    y = (z > 0).astype(float)
    bc = _train(lgb, X, y, "cpu", rounds=4, **extra)
    bg = _train(lgb, X, y, "gpu", rounds=4, gpu_use_dp=True, **extra)
    assert "host split policy" not in bg.device_name()
    tc, tg = _trees(bc), _trees(bg)
    assert [t["num_leaves"] for t in tc] == [t["num_leaves"] for t in tg]
    assert [s[:2] for s in _splits(tc[0]["tree_structure"], [])] == [s[:2] for s in _splits(tg[0]["tree_structure"], [])]
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=1e-3, atol=1e-3)
    # the penalty bites: fewer leaves than without it
    b0 = _train(lgb, X, y, "gpu", rounds=1, gpu_use_dp=True, **{k: v for k, v in extra.items() if "cegb" not in k})
    assert _trees(b0)[0]["num_leaves"] >= tg[0]["num_leaves"]


@pytest.mark.parametrize("extra", [{"cegb_penalty_feature_coupled": [500, 300, 100, 100, 30, 30]},
                                   {"cegb_penalty_feature_coupled": [0, 0, 40, 40, 10, 10], "cegb_penalty_split": 0.002,
                                    "cegb_tradeoff": 0.7, "num_leaves": 63},
                                   {"cegb_penalty_feature_coupled": [3000, 100, 60, 60, 20, 40],
                                    "monotone_constraints": [1, -1, 0, 0, 0, 0]},
                                   {"cegb_penalty_split": 0.05,
                                    "cegb_penalty_feature_lazy": [0.01, 0.02, 0.03, 0.04, 0.05, 0.06]},
                                   {"cegb_penalty_feature_lazy": [0.05, 0.1, 0.1, 0.1, 0.1, 0.1],
                                    "cegb_penalty_feature_coupled": [0, 0, 40, 40, 10, 10], "bagging_fraction": 0.8,
                                    "bagging_freq": 1},
                                   {"cegb_penalty_feature_lazy": [0.02, 0.02, 0.05, 0.05, 0.1, 0.1],
                                    "min_data_in_leaf": 300, "num_leaves": 63}])
def test_device_cegb_coupled_penalties(lgb, gpu_required, rng, extra):
    """CEGB feature penalties in the frontier engine. Coupled: raw candidates kept per node, the
    penalty of a feature not yet used by any split subtracted, and a feature's first use in the
    replay refunding every other leaf's stored candidate (leaf-index chain) and voiding the
    speculative expansions grown under the old gains. Lazy: per-row feature marks (a final
    leaf's rows marked for its path after each tree), each node's unmarked-row counts (smaller
    child counted, larger = parent - smaller). Trees equal the host CegbPenalty learner's split
    for split, over several trees (used flags and marks persist across trees)."""
    X, z = _policy_data(rng)
    y = (z > 0).astype(float)
    bc = _train(lgb, X, y, "cpu", rounds=4, **extra)
    bg = _train(lgb, X, y, "gpu", rounds=4, gpu_use_dp=True, **extra)
    assert "host split policy" not in bg.device_name() and "frontier" in bg.device_name()
    tc, tg = _trees(bc), _trees(bg)
    for a, b in zip(tc, tg):
        assert [s[:2] for s in _splits(a["tree_structure"], [])] == [s[:2] for s in _splits(b["tree_structure"], [])]
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=1e-4, atol=1e-4)


def test_histogram_pool_bound_routes_to_pooled_learner(lgb, gpu_required, rng, monkeypatch):
    """num_leaves per-leaf device histograms above the device budget (half the HBM; here a small
    budget through LGAP_DEVICE_HIST_BUDGET_MB): training takes the host learner's LRU histogram
    pool (evicted histograms rebuilt from rows by the HIP kernels) instead of the device learner's
    one-slot-per-leaf store; the model equals the pooled CPU learner's. A user-set
    histogram_pool_size bounds only the host cache, as in the reference: the device learner stays."""
    X, z = _policy_data(rng)
    y = (z > 0).astype(float)
    # 6 features x 255 bins x 16 B ~ 24 KB per leaf: 63 leaves ~ 1.5 MB > 1 MB
    extra = {"num_leaves": 63, "histogram_pool_size": 1.0}
    bc = _train(lgb, X, y, "cpu", rounds=3, **extra)
    monkeypatch.setenv("LGAP_DEVICE_HIST_BUDGET_MB", "1")
    bg = _train(lgb, X, y, "gpu", rounds=3, gpu_use_dp=True, **extra)
    assert "host split policy" in bg.device_name()
    assert [s[:2] for s in _splits(_trees(bc)[0]["tree_structure"], [])] == \
        [s[:2] for s in _splits(_trees(bg)[0]["tree_structure"], [])]
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=1e-3, atol=1e-3)
    monkeypatch.delenv("LGAP_DEVICE_HIST_BUDGET_MB")
    # a small user histogram_pool_size alone keeps the device learner
    bd = _train(lgb, X, y, "gpu", rounds=1, num_leaves=63, histogram_pool_size=1.0)
    assert "host split policy" not in bd.device_name()


def test_frontier_only_options_fall_back_when_the_frontier_cannot_hold_them(lgb, gpu_required, rng, tmp_path):
    """Forced splits and CEGB feature penalties run on the frontier engine only. A tree the
    frontier's select cannot hold in LDS (num_leaves=400: ~169 KB node image) takes the host split
    policy over HIP histograms instead of failing at allocation (device::FrontierServes)."""
    import json

    X, z = _policy_data(rng)
    y = (z > 0).astype(float)
    f = tmp_path / "forced.json"
    f.write_text(json.dumps({"feature": 4, "threshold": 0.1, "left": {"feature": 5, "threshold": -0.2}}))
    kw = {"num_leaves": 400, "min_data_in_leaf": 2, "forcedsplits_filename": str(f)}
    bg = _train(lgb, X, y, "gpu", rounds=2, gpu_use_dp=True, **kw)
    assert "host split policy" in bg.device_name()
    root = _trees(bg)[0]["tree_structure"]
    assert root["split_feature"] == 4 and root["left_child"]["split_feature"] == 5
    bc = _train(lgb, X, y, "cpu", rounds=2, **kw)
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=1e-3, atol=1e-3)
    pen = [0.5] * X.shape[1]
    bp = _train(lgb, X, y, "gpu", rounds=1, num_leaves=400, min_data_in_leaf=2, cegb_penalty_feature_coupled=pen)
    assert "host split policy" in bp.device_name()


FORCED_TREES = [
    {"feature": 4, "threshold": 0.1, "left": {"feature": 5, "threshold": -0.2}},
    # two levels on both sides, children pushed left then right (breadth-first order)
    {"feature": 0, "threshold": 0.0,
     "left": {"feature": 1, "threshold": 0.3, "left": {"feature": 2, "threshold": -0.5}},
     "right": {"feature": 3, "threshold": -0.1, "right": {"feature": 2, "threshold": 0.5}}},
    # the left child's forced split cannot gain (every row goes left): forced splitting stops
    # there and the right child's forced split is never applied
    {"feature": 4, "threshold": 0.0, "left": {"feature": 5, "threshold": 1e9},
     "right": {"feature": 3, "threshold": 0.2}},
    # a node without a feature inside the tree: that node and its subtree are skipped
    {"feature": 1, "threshold": 0.0, "left": {"threshold": 0.0, "left": {"feature": 0, "threshold": 0}},
     "right": {"feature": 2, "threshold": 0.1}},
]


@pytest.mark.parametrize("case", range(len(FORCED_TREES)))
def test_forced_splits_on_device(lgb, gpu_required, rng, tmp_path, case):
    """Forced splits on the device-resident frontier engine (no host split policy): the select
    applies the flattened forced list first, each forced split computed by the scan at its
    threshold; the first tree matches the host learner split for split."""
    import json

    X, z = _policy_data(rng)
    y = (z > 0).astype(float)
    f = tmp_path / "forced.json"
    f.write_text(json.dumps(FORCED_TREES[case]))
    bc = _train(lgb, X, y, "cpu", rounds=3, forcedsplits_filename=str(f))
    bg = _train(lgb, X, y, "gpu", rounds=3, gpu_use_dp=True, forcedsplits_filename=str(f))
    assert "host split policy" not in bg.device_name() and "frontier engine" in bg.device_name()
    for t in range(3):
        tc, tg = _trees(bc)[t]["tree_structure"], _trees(bg)[t]["tree_structure"]
        sc, sg = _splits(tc, []), _splits(tg, [])
        assert [s[0] for s in sc] == [s[0] for s in sg], (t, sc[:6], sg[:6])
        np.testing.assert_allclose([s[1] for s in sg], [s[1] for s in sc], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=1e-4, atol=1e-4)


def test_forced_splits_over_device_histograms(lgb, gpu_required, rng, tmp_path):
    """Forced splits where the device frontier does not apply (feature_fraction_bynode): the
    host split policy over HIP histograms."""
    import json

    X, z = _policy_data(rng)
    y = (z > 0).astype(float)
    f = tmp_path / "forced.json"
    f.write_text(json.dumps({"feature": 4, "threshold": 0.1, "left": {"feature": 5, "threshold": -0.2}}))
    kw = {"feature_fraction_bynode": 0.999, "forcedsplits_filename": str(f)}
    bc = _train(lgb, X, y, "cpu", rounds=2, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=2, gpu_use_dp=True, **kw)
    assert "host split policy" in bg.device_name()
    for b in (bc, bg):
        root = _trees(b)[0]["tree_structure"]
        assert root["split_feature"] == 4 and root["left_child"]["split_feature"] == 5
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=1e-3, atol=1e-3)


def test_collective_watchdog_aborts_on_timeout(lgb, gpu_required):
    """The RCCL watchdog (runtime.hip WatchedStreamSync): a collective wait that outlives the
    timeout aborts the communicator and raises on the rank instead of hanging."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LGAP_DP_TRANSPORT="collective")
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "watchdog_selftest.py")], capture_output=True,
                       env=env,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["raised"], res
    assert "communicator aborted" in res["message"], res


def test_xgmi_exchange_timeout_raises(lgb, gpu_required):
    """xGMI transport failure detection: a rank that stops signalling (LGAP_FAULT_INJECT=xgmi drops
    every flag after the set-up self-test) makes the in-kernel exchange wait run into its bound;
    the learner raises instead of hanging the GPU."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LGAP_DP_TRANSPORT="xgmi", LGAP_FAULT_INJECT="xgmi", LGAP_XGMI_TIMEOUT_S="0.5",
               LGAP_COMM_TIMEOUT_S="120")
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "watchdog_selftest.py")], capture_output=True,
                       env=env, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["raised"], res
    assert "xGMI exchange" in res["message"] and "timed out" in res["message"], res


def test_device_bagging_by_query_matches_host(lgb, gpu_required):
    """bagging_by_query drawn on the device (one draw per query from the per-1024-query LCG
    streams, every row of a kept query kept, streams advanced across re-bags) trains the
    host sampler's model."""
    from lambdagap_amd.utils import make_ranking

    X, y, sizes = make_ranking(400, num_features=20, seed=9)
    params = {"objective": "lambdarank", "num_leaves": 15, "verbosity": -1, "bagging_by_query": True,
              "bagging_fraction": 0.6, "bagging_freq": 2, "bagging_seed": 5}
    bc = lgb.train({**params, "device_type": "cpu"}, lgb.Dataset(X, y, group=sizes), 6)
    bg = lgb.train({**params, "device_type": "gpu"}, lgb.Dataset(X, y, group=sizes), 6)
    bh = lgb.train({**params, "device_type": "gpu", "device_sampling": False}, lgb.Dataset(X, y, group=sizes), 6)
    pc, pg, ph = (b.predict(X, raw_score=True) for b in (bc, bg, bh))
    # device draw == host draw: the device-sampled model has the host-sampled device model's
    # splits (leaf values agree to float rounding)
    def splits(b):
        return [ln for ln in b.model_to_string().splitlines() if ln.startswith(("split_feature=", "threshold="))]

    assert splits(bg) == splits(bh)
    np.testing.assert_allclose(pg, ph, rtol=1e-4, atol=1e-5)
    assert np.corrcoef(pc, pg)[0, 1] > 0.999


@pytest.mark.parametrize("objective,metrics,extra", [
    ("binary", ["binary_logloss", "binary_error", "l2", "l1", "mape"], {}),
    ("regression", ["l2", "rmse", "l1", "huber", "fair", "quantile", "mape"], {"reg_sqrt": True}),
    ("poisson", ["poisson", "l2", "gamma", "gamma_deviance", "tweedie"], {}),
    ("cross_entropy", ["cross_entropy", "kullback_leibler", "cross_entropy_lambda"], {}),
    ("cross_entropy_lambda", ["cross_entropy_lambda", "cross_entropy"], {}),
])
@pytest.mark.parametrize("weighted", [False, True])
def test_device_training_metrics_match_host(lgb, gpu_required, objective, metrics, extra, weighted):
    """Pointwise training metrics evaluated on the device score (k_metric_partial + fold, row loss
    shared with the host metric through lgap/pointwise_metric.h) equal the host evaluation of the
    same booster (LGAP_DEVICE_METRICS=0 forces the host path)."""
    import os

    rng = np.random.default_rng(31)
    n = 50000
    X = rng.standard_normal((n, 8))
    if objective == "binary":
        y = (X[:, 0] + 0.5 * rng.standard_normal(n) > 0).astype(float)
    elif objective == "regression":
        y = X[:, 0] * 3 + rng.standard_normal(n)
    elif objective == "poisson":
        y = rng.poisson(np.exp(0.3 * X[:, 0] + 0.5)).astype(float) + 0.5
    else:
        y = 1 / (1 + np.exp(-X[:, 0] - 0.3 * rng.standard_normal(n)))
    w = rng.uniform(0.5, 2.0, n) if weighted else None
    params = {"objective": objective, "metric": metrics, "device_type": "gpu", "verbosity": -1, "num_leaves": 15,
              **extra}
    b = lgb.Booster(params, lgb.Dataset(X, y, weight=w, params=params))
    for _ in range(3):
        b.update()
    dev = b.eval_train()
    os.environ["LGAP_DEVICE_METRICS"] = "0"
    try:
        host = b.eval_train()
    finally:
        del os.environ["LGAP_DEVICE_METRICS"]
    assert [r[1] for r in dev] == [r[1] for r in host]
    for d, h in zip(dev, host):
        assert d[2] == pytest.approx(h[2], rel=1e-9, abs=1e-12), (d, h)


@pytest.mark.parametrize("objective,metrics", [("binary", ["binary_logloss", "auc", "binary_error"]),
                                               ("regression", ["l2", "l1", "huber"]),
                                               ("multiclass", ["multi_logloss", "multi_error"])])
def test_device_validation_scoring(lgb, gpu_required, rng, objective, metrics):
    """Validation sets scored on the device (packed rows uploaded once, each tree traversed on
    the device, pointwise metrics reduced there; AUC / multiclass read the refreshed host copy):
    every recorded metric, early stopping and predictions equal the host-scored run."""
    import os
    import subprocess
    import sys
    import json

    code = f"""
import json, os, sys, numpy as np
sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})
import lambdagap_amd as lgb
rng = np.random.default_rng(5)
X = rng.standard_normal((30000, 8)); Xv = rng.standard_normal((7000, 8))
def lab(X):
    z = X[:, 0] - 0.7 * X[:, 1] + 0.3 * X[:, 2] * X[:, 3]
    if {objective!r} == "binary": return (z + 0.3 * rng.standard_normal(len(X)) > 0).astype(float)
    if {objective!r} == "multiclass": return np.digitize(z, [-0.5, 0.5]).astype(float)
    return z + 0.2 * rng.standard_normal(len(X))
y, yv = lab(X), lab(Xv)
p = {{"objective": {objective!r}, "metric": {metrics!r}, "num_leaves": 15, "device_type": "gpu", "verbosity": -1,
     "early_stopping_round": 5}}
if {objective!r} == "multiclass": p["num_class"] = 3
ds = lgb.Dataset(X, y); dv = ds.create_valid(Xv, yv)
ev = {{}}
b = lgb.train(p, ds, 40, valid_sets=[dv], valid_names=["v"], callbacks=[lgb.record_evaluation(ev)],
              keep_training_booster=True)
print(json.dumps({{"ev": ev["v"], "best": b.best_iteration, "pred": b.predict(Xv[:500]).ravel().tolist(),
                  "inner": b._Booster__inner_predict(1).ravel()[:500].tolist()}}))
"""
    runs = {}
    for mode in ("1", "0"):
        env = dict(os.environ, LGAP_DEVICE_VALID=mode)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        runs[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    dev, host = runs["1"], runs["0"]
    assert dev["best"] == host["best"]
    for name in host["ev"]:
        np.testing.assert_allclose(dev["ev"][name], host["ev"][name], rtol=1e-9, atol=1e-12, err_msg=name)
    np.testing.assert_allclose(dev["pred"], host["pred"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dev["inner"], host["inner"], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("ncat,onehot", [(1500, 4), (40, 64), (300, 4)])
def test_device_categorical_wide(lgb, gpu_required, rng, ncat, onehot):
    """Categorical features between max_cat_to_onehot and the 1024-bin bitset cap (1500 distinct
    categories fold their rarest into bin 0): the wave-parallel one-hot / bitonic ctr-sorted device
    scan picks the CPU learner's splits."""
    n = 200_000
    X = rng.standard_normal((n, 4))
    X[:, 0] = rng.integers(0, ncat, n)
    eff = rng.standard_normal(ncat)
    y = (eff[X[:, 0].astype(int)] + 0.5 * X[:, 1] + 0.3 * rng.standard_normal(n) > 0).astype(float)
    kw = {"categorical_feature": [0], "max_cat_to_onehot": onehot, "max_bin": 2047, "min_data_per_group": 20,
          "cat_smooth": 5.0, "max_cat_threshold": 64, "num_leaves": 15}
    bc = _train(lgb, X, y, "cpu", rounds=3, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=3, gpu_use_dp=True, **kw)
    nb = lgb.Dataset(X, y, params={"categorical_feature": [0], "max_bin": 2047, "verbosity": -1}).construct() \
        .feature_num_bin(0)
    assert nb <= 1024 and (nb > onehot) == (ncat > onehot), nb  # ctr-sorted vs one-hot path
    sc = [s[:2] for s in _splits(_trees(bc)[0]["tree_structure"], [])][:4]
    sg = [s[:2] for s in _splits(_trees(bg)[0]["tree_structure"], [])][:4]
    assert sc == sg
    np.testing.assert_allclose(bg.predict(X[:5000], raw_score=True), bc.predict(X[:5000], raw_score=True),
                               rtol=0, atol=2e-3)


def test_device_max_bin_8191_global_scan(lgb, gpu_required, rng):
    """max_bin=8191: the split scan works in global scratch (features wider than the LDS budget)
    and matches the CPU learner; the same global path forced on ordinary bins (LGAP_KERNEL=scan_global=1)
    grows the model of the sequential chain's LDS path."""
    import os
    import subprocess
    import sys

    n = 300_000
    X = rng.standard_normal((n, 5))
    y = (X[:, 0] + 0.5 * np.sin(3 * X[:, 1]) + 0.2 * rng.standard_normal(n) > 0).astype(float)
    kw = {"max_bin": 8191, "num_leaves": 15, "min_data_in_bin": 1}
    bc = _train(lgb, X, y, "cpu", rounds=2, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=2, gpu_use_dp=True, **kw)
    assert _splits(_trees(bc)[0]["tree_structure"], []) == _splits(_trees(bg)[0]["tree_structure"], [])
    np.testing.assert_allclose(bg.predict(X[:5000], raw_score=True), bc.predict(X[:5000], raw_score=True),
                               rtol=0, atol=1e-6)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import lambdagap_amd as lgb; "
            "from lambdagap_amd.utils import make_higgs_like; X, y = make_higgs_like(100000, seed=2); "
            "p = {'objective': 'binary', 'num_leaves': 31, 'device_type': 'gpu', 'verbosity': -1}; "
            "print(lgb.train(p, lgb.Dataset(X, y, params=p), 5).model_to_string().split('end of trees')[0])"
            ) % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    # the global-memory scan is a variant of the sequential device chain (the frontier engine has
    # no global-scan variant): compare it with that chain's LDS scan
    for env in ({"LGAP_FRONTIER": "0"}, {"LGAP_FRONTIER": "0", "LGAP_KERNEL": "scan_global=1"}):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]


def test_reset_training_data_keeps_device_validation(lgb, gpu_required, rng):
    """ResetTrainingData builds a new device learner: validation sets scored on the old one are
    pulled back and registered again, so training and evaluation continue."""
    X = rng.standard_normal((20000, 6))
    y = (X[:, 0] - 0.5 * X[:, 1] > 0).astype(float)
    Xv = rng.standard_normal((5000, 6))
    yv = (Xv[:, 0] - 0.5 * Xv[:, 1] > 0).astype(float)
    p = {"objective": "binary", "metric": "binary_logloss", "num_leaves": 15, "device_type": "gpu",
         "verbosity": -1}
    outs = []
    for dev in ("gpu", "cpu"):
        q = dict(p, device_type=dev)
        ds = lgb.Dataset(X, y, params=q, free_raw_data=False)
        b = lgb.Booster(q, ds)
        b.add_valid(ds.create_valid(Xv, yv), "v")
        for _ in range(3):
            b.update()
        ds2 = lgb.Dataset(X[:15000], y[:15000], params=q, reference=ds)
        b.update(train_set=ds2)
        for _ in range(2):
            b.update()
        outs.append((b.eval_valid()[0][2], b.predict(Xv[:1000], raw_score=True)))
    assert np.isfinite(outs[0][0])
    assert abs(outs[0][0] - outs[1][0]) < 1e-3, (outs[0][0], outs[1][0])
    np.testing.assert_allclose(outs[0][1], outs[1][1], rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("extra", [{}, {"max_depth": 6}, {"monotone_constraints": [1, -1, 0, 0, 0, 0]},
                                   {"interaction_constraints": [[0, 1], [1, 2, 3]]},
                                   {"categorical_feature": [4], "max_cat_to_onehot": 4},
                                   {"bagging_fraction": 0.7, "bagging_freq": 1}, {"num_leaves": 255, "min_data_in_leaf": 5}])
def test_frontier_engine_matches_sequential_chain(lgb, gpu_required, rng, extra):
    """The frontier engine (batched rounds + replay of best-first order, src/device/frontier.h)
    grows the trees of the one-split-at-a-time device chain: identical split structure with fp64
    histograms, for the options the frontier covers."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json, numpy as np; sys.path.insert(0, %r); import lambdagap_amd as lgb; "
            "rng = np.random.default_rng(3); X = rng.standard_normal((60000, 6)); "
            "X[:, 4] = rng.integers(0, 9, 60000); X[rng.random(60000) < 0.1, 0] = np.nan; "
            "y = (X[:, 0] - 0.7 * X[:, 1] + 0.4 * X[:, 2] * X[:, 3] + 0.3 * (X[:, 4] %% 3) + 0.3 * rng.standard_normal(60000) > 0).astype(float); "
            "p = dict({'objective': 'binary', 'num_leaves': 31, 'device_type': 'gpu', 'verbosity': -1, 'gpu_use_dp': True, "
            "'seed': 2}, **json.loads(sys.argv[1])); "
            "b = lgb.train(p, lgb.Dataset(X, y, params=p), 6, keep_training_booster=True); "
            "print(json.dumps({'model': b.model_to_string().split('end of trees')[0], 'name': b.device_name()}))") % root
    outs = []
    for fr in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", code, json.dumps(extra)], capture_output=True, text=True,
                           timeout=300, env=dict(os.environ, LGAP_FRONTIER=fr))
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))

    def structure(model):
        return [ln for ln in model.splitlines() if ln.startswith(("split_feature=", "threshold=", "left_child=",
                                                                   "right_child=", "decision_type=", "num_leaves="))]
    assert "frontier engine" in outs[0]["name"] and "frontier" not in outs[1]["name"], outs[0]["name"]
    assert structure(outs[0]["model"]) == structure(outs[1]["model"])


@pytest.mark.parametrize("max_bin", [15, 7])
def test_four_bit_rows_match_byte_rows(lgb, gpu_required, rng, monkeypatch, max_bin):
    """max_bin <= 15: the frontier histograms and the training score update read 4-bit rows
    (8 groups per dword, traverse_kernels.hip LaunchPackNibbles); the model is identical to the
    one grown from the 8-bit rows (LGAP_KERNEL=nibble=0), trees and training predictions."""
    n = 30000
    X = rng.standard_normal((n, 11))
    X[rng.random(n) < 0.05, 3] = np.nan
    y = (X[:, 0] - 0.6 * X[:, 1] + 0.4 * X[:, 2] * X[:, 4] + 0.3 * rng.standard_normal(n) > 0).astype(float)
    params = {"objective": "binary", "num_leaves": 31, "max_bin": max_bin, "device_type": "gpu", "verbosity": -1}
    models = []
    for nib in ("1", "0"):
        monkeypatch.setenv("LGAP_KERNEL", f"nibble={nib}")
        b = lgb.train(params, lgb.Dataset(X, y, params=params), 10)
        models.append((b.model_to_string().split("end of trees")[0], b.predict(X, raw_score=True)))
    assert models[0][0] == models[1][0]
    np.testing.assert_array_equal(models[0][1], models[1][1])


def test_wide_rows_training_score(lgb, gpu_required, rng):
    """Rows wider than 16 dwords (120 features): with bagging the training score update walks the
    group-major copy (traverse_kernels.hip, k_traverse_col), without it it comes from the leaf
    ranges; both equal the model's prediction and the boosted model tracks the CPU learner's."""
    n, f = 30000, 120
    X = rng.standard_normal((n, f))
    X[:, 3] = rng.integers(0, 7, n)
    y = X[:, 0] - 0.5 * X[:, 1] + 0.3 * X[:, 2] * X[:, 5] + 0.2 * (X[:, 3] == 2) + 0.1 * rng.standard_normal(n)
    params = {"objective": "regression", "num_leaves": 31, "verbosity": -1, "categorical_feature": [3],
              "min_data_in_leaf": 40}
    bc = lgb.train({**params, "device_type": "cpu"}, lgb.Dataset(X, y), 8)
    for extra in ({}, {"bagging_fraction": 0.8, "bagging_freq": 1}):  # leaf-range update / column walk
        bg = lgb.train({**params, "device_type": "gpu", "gpu_use_dp": True, **extra}, lgb.Dataset(X, y), 8,
                       keep_training_booster=True)
        np.testing.assert_allclose(bg._Booster__inner_predict(0), bg.predict(X), rtol=0, atol=1e-9)
        if not extra:
            np.testing.assert_allclose(bg.predict(X[:3000]), bc.predict(X[:3000]), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("extra", [{}, {"objective": "multiclass", "num_class": 3},
                                   {"num_leaves": 1100, "min_data_in_leaf": 2, "min_sum_hessian_in_leaf": 0},
                                   {"num_leaves": 300, "min_data_in_leaf": 5},
                                   {"bagging_fraction": 0.7, "bagging_freq": 1}, {"data_sample_strategy": "goss"}])
def test_leaf_range_score_update_matches_predict(lgb, gpu_required, rng, extra):
    """The training score update from the final leaf ranges (traverse_kernels.hip k_leaf_bounds /
    k_leaf_tile_add: per-tile runs of every leaf's ascending rows, an LDS row -> leaf map) equals
    the model's prediction on the training rows. n = 20001 is not a multiple of the 4096-row tile
    and makes the multiclass class slices 8-byte (not 16-byte) aligned; 1100 leaves exceed the
    path's 1024-leaf limit and bagging / GOSS leave rows out of the leaves: those take the
    traversal."""
    n = 20001
    X = rng.standard_normal((n, 10))
    z = X[:, 0] - 0.6 * X[:, 1] + 0.4 * X[:, 2] * X[:, 3] + 0.3 * rng.standard_normal(n)
    y = np.digitize(z, [-0.5, 0.5]).astype(float) if extra.get("objective") == "multiclass" else (z > 0).astype(float)
    params = {"objective": "binary", "num_leaves": 63, "device_type": "gpu", "verbosity": -1, **extra}
    b = lgb.train(params, lgb.Dataset(X, y), 6, keep_training_booster=True)
    # (the inner scores come back through the objective's output transform, as predict's)
    np.testing.assert_allclose(b._Booster__inner_predict(0), b.predict(X), rtol=0, atol=1e-9)


_IC70 = [[(7 * i) % 12, (7 * i + 3) % 12, (5 * i + 1) % 12] for i in range(70)]


@pytest.mark.parametrize("extra", [{"feature_fraction_bynode": 0.6},
                                   {"feature_fraction_bynode": 0.5, "feature_fraction": 0.8, "num_leaves": 31},
                                   {"feature_fraction_bynode": 0.7, "max_depth": 3, "min_data_in_leaf": 50},
                                   {"feature_fraction_bynode": 0.6,
                                    "interaction_constraints": [[0, 1, 2], [2, 3, 4, 5], [6, 7, 8, 9, 10, 11]]},
                                   {"feature_fraction_bynode": 0.5, "feature_fraction": 0.8, "num_leaves": 31,
                                    "interaction_constraints": [[0, 1], [1, 2, 3], [0, 4, 5, 6], [7, 8, 9, 10, 11]]},
                                   {"feature_fraction_bynode": 0.3, "num_leaves": 31, "interaction_constraints": _IC70}],
                         ids=["bynode", "bytree", "depth", "ic", "ic-bytree", "ic-70sets"])
def test_bynode_sampling_on_frontier_matches_cpu(lgb, gpu_required, rng, extra):
    """feature_fraction_bynode on the frontier engine: the tree's masks in the host's draw order
    (root, then smaller / larger child of every scanned split), each child scored when its parent
    commits in the replay, and the sampler rewound to the draws the tree used, so every tree (not
    only the first) equals the CPU learner's. Under interaction constraints each node's pool is the
    features its sets allow, so the select draws the masks itself (Random::Sample's Bernoulli and
    Floyd branches over the pool, the sampler's state handed back to the host after each tree)."""
    X = rng.standard_normal((30000, 12))
    z = X[:, 0] - 0.8 * X[:, 1] + 0.5 * X[:, 2] * X[:, 3] + 0.3 * X[:, 4] + 0.2 * rng.standard_normal(30000)
    y = (z > 0).astype(float)
    kw = {"num_leaves": 15, "feature_fraction_seed": 5}
    kw.update(extra)
    bc = _train(lgb, X, y, "cpu", rounds=6, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=6, gpu_use_dp=True, **kw)
    assert "frontier engine" in bg.device_name(), bg.device_name()
    for t in range(6):
        sc = _splits(_trees(bc)[t]["tree_structure"], [])
        sg = _splits(_trees(bg)[t]["tree_structure"], [])
        assert [s[0] for s in sc] == [s[0] for s in sg], (t, sc[:6], sg[:6])
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("extra", [{}, {"num_leaves": 31, "extra_seed": 11}, {"max_depth": 4, "min_data_in_leaf": 40}])
def test_extra_trees_on_frontier_matches_cpu(lgb, gpu_required, rng, extra):
    """extra_trees on the frontier engine: per-feature random streams drawn in the host's order
    (each scanned node's smaller child, then its larger one), kept by expanding only the node the
    replay waits for; numerical and categorical (one-hot and ctr-sorted) thresholds; every tree
    equals the CPU learner's."""
    n = 30000
    X = rng.standard_normal((n, 8))
    X[:, 6] = rng.integers(0, 3, n)    # one-hot categorical
    X[:, 7] = rng.integers(0, 25, n)   # many-category categorical
    z = X[:, 0] - 0.8 * X[:, 1] + 0.4 * (X[:, 7] % 5 == 1) + 0.3 * (X[:, 6] == 2) + 0.3 * rng.standard_normal(n)
    y = (z > 0).astype(float)
    kw = {"num_leaves": 15, "extra_trees": True, "categorical_feature": [6, 7], "min_data_per_group": 20,
          "cat_smooth": 5}
    kw.update(extra)
    bc = _train(lgb, X, y, "cpu", rounds=5, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=5, gpu_use_dp=True, **kw)
    assert "frontier engine" in bg.device_name(), bg.device_name()
    for t in range(5):
        sc = _splits(_trees(bc)[t]["tree_structure"], [])
        sg = _splits(_trees(bg)[t]["tree_structure"], [])
        assert [s[0] for s in sc] == [s[0] for s in sg], (t, sc[:6], sg[:6])
    np.testing.assert_allclose(bg.predict(X, raw_score=True), bc.predict(X, raw_score=True), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("extra", [{}, {"linear_lambda": 0.5, "num_leaves": 15}, {"nan": True}])
def test_linear_tree_on_device_matches_cpu(lgb, gpu_required, rng, extra):
    """linear_tree on the device learner: the structure from the frontier engine, each leaf's
    Gram system [X'HX | X'g] accumulated by the fp64 MFMA kernel over the leaf's rows, solved on
    the host; the training score updated by the traversal's linear leaf evaluation. Equal to the
    host linear learner within fp64 round-off (rows with NaN features keep the constant)."""
    extra = dict(extra)
    nan = extra.pop("nan", False)
    n = 20000
    X = rng.standard_normal((n, 6))
    z = 1.5 * X[:, 0] - X[:, 1] + 0.7 * X[:, 2] * X[:, 3] + 0.3 * rng.standard_normal(n)
    if nan:
        X[rng.random(X.shape) < 0.02] = np.nan
    kw = {"objective": "regression", "linear_tree": True, "num_leaves": 7}
    kw.update(extra)
    bc = _train(lgb, X, z, "cpu", rounds=5, **kw)
    bg = _train(lgb, X, z, "gpu", rounds=5, gpu_use_dp=True, **kw)
    assert "host split policy" not in bg.device_name() and "frontier engine" in bg.device_name()
    tc, tg = _trees(bc), _trees(bg)
    for t in range(5):
        assert [s[:2] for s in _splits(tc[t]["tree_structure"], [])] == [s[:2] for s in _splits(tg[t]["tree_structure"], [])]
    np.testing.assert_allclose(bg.predict(X), bc.predict(X), rtol=1e-4, atol=1e-4)
    # the device-resident training score (traversal with linear leaves) equals the model's prediction
    ev = {}
    p2 = {**kw, "device_type": "gpu", "gpu_use_dp": True, "verbosity": -1, "metric": "l2", "seed": 1,
          "min_data_in_leaf": 20, "deterministic": True}
    ds = lgb.Dataset(X, z, params=p2)
    bg2 = lgb.train(p2, ds, 5, valid_sets=[ds], valid_names=["train"], callbacks=[lgb.record_evaluation(ev)])
    np.testing.assert_allclose(ev["train"]["l2"][-1], float(np.mean((bg2.predict(X) - z) ** 2)), rtol=1e-9)


def test_linear_tree_wide_branches_on_device_and_beyond(lgb, gpu_required, rng):
    """Leaves that can carry 31-62 branch features use the Gram kernel's four-tile instantiation
    (64 x 64 [A | c], 284 VGPRs) and match the host linear learner; more than 62 train under the
    host linear learner over HIP histograms."""
    n = 6000
    X = rng.standard_normal((n, 40))
    z = X[:, :5].sum(axis=1) + 0.3 * X[:, 7] * X[:, 11] + 0.1 * rng.standard_normal(n)
    kw = {"objective": "regression", "linear_tree": True, "num_leaves": 48, "min_data_in_leaf": 10}
    bc = _train(lgb, X, z, "cpu", rounds=3, **kw)
    bg = _train(lgb, X, z, "gpu", rounds=3, gpu_use_dp=True, **kw)
    assert "host split policy" not in bg.device_name() and "frontier engine" in bg.device_name(), bg.device_name()
    tc, tg = _trees(bc), _trees(bg)
    for t in range(3):
        assert [s[:2] for s in _splits(tc[t]["tree_structure"], [])] == [s[:2] for s in _splits(tg[t]["tree_structure"], [])]
    np.testing.assert_allclose(bg.predict(X), bc.predict(X), rtol=1e-4, atol=1e-4)
    X2 = rng.standard_normal((n, 70))
    z2 = X2[:, :5].sum(axis=1) + 0.1 * rng.standard_normal(n)
    bg2 = _train(lgb, X2, z2, "gpu", rounds=2, **dict(kw, num_leaves=80))
    assert "host split policy" in bg2.device_name()


@pytest.mark.parametrize("extra", [{}, {"num_leaves": 63, "monotone_constraints": [1] + [0] * 79},
                                   {"max_bin": 63, "lambda_l2": 1.0}])
def test_wide_data_wave_scan_matches_cpu(lgb, gpu_required, rng, extra):
    """Wide numerical data (80 features, so the frontier scans one (expansion, feature) item per
    wave: k_f_scan_w) grows the CPU learner's trees; the row-aligned multi-tile layout (a narrow
    LDS budget forces several tiles) keeps the histograms exact."""
    n, nf = 20000, 80
    X = rng.standard_normal((n, nf))
    X[rng.random((n, nf)) < 0.05] = np.nan
    z = X[:, 0] - 0.7 * np.nan_to_num(X[:, 1]) + 0.4 * np.nan_to_num(X[:, 5]) * np.nan_to_num(X[:, 9])
    y = (z + 0.3 * rng.standard_normal(n) > 0).astype(float)
    kw = {"num_leaves": 31, "min_data_in_leaf": 20}
    kw.update(extra)
    bc = _train(lgb, X, y, "cpu", rounds=4, **kw)
    bg = _train(lgb, X, y, "gpu", rounds=4, gpu_use_dp=True, **kw)
    assert "frontier engine" in bg.device_name(), bg.device_name()
    for t in range(4):
        sc = _splits_in_order(_trees(bc)[t]["tree_structure"])
        sg = _splits_in_order(_trees(bg)[t]["tree_structure"])
        for a, b in zip(sc, sg):
            if a[1] != b[1]:
                # two features whose gains agree to float32 (the model's split_gain): which one
                # wins depends on the last bits of differently ordered fp64 sums, not on the scan
                assert a[2] == b[2] and a[3] == b[3], (t, a, b)
                return
        assert len(sc) == len(sg)
    np.testing.assert_allclose(bg.predict(X[:2000], raw_score=True), bc.predict(X[:2000], raw_score=True),
                               rtol=1e-4, atol=1e-4)


def _splits_in_order(node, out=None):
    """(split_index, feature, split_gain, internal_count) in the order the learner split them."""
    out = [] if out is None else out
    if "split_index" in node:
        out.append((node["split_index"], node["split_feature"], node["split_gain"], node["internal_count"]))
        _splits_in_order(node["left_child"], out)
        _splits_in_order(node["right_child"], out)
    return sorted(out)


@pytest.mark.parametrize("quantized", [False, True])
def test_interleaved_root_histogram_rows_4m(lgb, gpu_required, quantized, monkeypatch):
    """From 4M rows the single-tile plan reserves LDS for the interleaved root histogram
    (k_f_hist il); fixed-point and quantized (MODE 3 sub-chunk folding) training launch within
    the LDS budget and grow the same trees as with the interleave off (integer sums)."""
    rng = np.random.default_rng(17)
    n = 4_200_000
    X = rng.standard_normal((n, 10)).astype(np.float32)
    y = (X[:, 0] - 0.6 * X[:, 1] + 0.3 * rng.standard_normal(n) > 0).astype(np.float32)
    params = {"objective": "binary", "num_leaves": 31, "device_type": "gpu", "verbosity": -1, "seed": 3,
              "deterministic": True, "use_quantized_grad": quantized, "num_grad_quant_bins": 4}

    def model():
        b = lgb.train(params, lgb.Dataset(X, y, params=params), 3, keep_training_booster=True)
        assert "frontier engine" in b.device_name()
        return b.model_to_string()

    with_il = model()
    monkeypatch.setenv("LGAP_KERNEL", "hist_il=0")
    assert model() == with_il


def test_speculation_budget_does_not_change_trees(lgb, gpu_required, monkeypatch):
    """The frontier's speculation budget (fixed alpha, the timed tuner, the waste throttle) only
    decides which nodes are expanded ahead of the replay: the committed split sequence, and so
    the model, is the same under every budget."""
    rng = np.random.default_rng(23)
    n = 60000
    X = rng.standard_normal((n, 12))
    y = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.3 * rng.standard_normal(n)
    params = {"objective": "regression", "num_leaves": 255, "min_data_in_leaf": 5, "device_type": "gpu",
              "verbosity": -1, "seed": 4, "deterministic": True}

    def model(**env):
        monkeypatch.delenv("LGAP_FRONTIER_SPEC", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        b = lgb.train(params, lgb.Dataset(X, y, params=params), 30, keep_training_booster=True)
        assert "frontier engine" in b.device_name()
        return b.model_to_string()

    base = model(LGAP_FRONTIER_SPEC="fixed")
    assert model() == base  # timed tuner (>= 128 leaves, one process)
    assert model(LGAP_FRONTIER_SPEC="3") == base
    assert model(LGAP_FRONTIER_SPEC="adapt") == base


@pytest.mark.parametrize("extra", [{}, {"use_quantized_grad": True, "num_grad_quant_bins": 4},
                                   {"num_leaves": 300, "min_data_in_leaf": 2},
                                   {"monotone_constraints": [1, -1, 0, 1] + [0] * 12,
                                    "monotone_constraints_method": "intermediate"}])
def test_select_merged_alive_order_does_not_change_trees(lgb, gpu_required, monkeypatch, extra):
    """Beyond 256 alive nodes the select merges the previous round's alive order with the last
    round's children (and, under intermediate monotone constraints, the nodes it re-scanned)
    instead of re-sorting (FState::nsal, FArgs::salive): the same expansions and the same model as
    the full sort (LGAP_KERNEL=select_merge=0)."""
    rng = np.random.default_rng(29)
    n = 80000
    X = rng.standard_normal((n, 16))
    y = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] - 0.4 * np.abs(X[:, 3]) + 0.3 * rng.standard_normal(n)
    params = {"objective": "regression", "num_leaves": 255, "min_data_in_leaf": 5, "device_type": "gpu",
              "verbosity": -1, "seed": 4, "deterministic": True, **extra}

    # (a fixed speculation budget: the timed tuner's budget follows measured tree times; 300 leaves
    # is about the largest tree whose node image fits the select's LDS)
    monkeypatch.setenv("LGAP_FRONTIER_SPEC", "fixed")

    def model(merge):
        if merge:
            monkeypatch.delenv("LGAP_KERNEL", raising=False)
        else:
            monkeypatch.setenv("LGAP_KERNEL", "select_merge=0")
        b = lgb.train(params, lgb.Dataset(X, y, params=params), 12, keep_training_booster=True)
        assert "frontier engine" in b.device_name()
        return b.model_to_string()

    assert model(True) == model(False)


_GPU_LOAD = r"""
import sys, time
import torch
a = torch.randn(6144, 6144, device="cuda")
b = torch.empty_like(a)
torch.cuda.synchronize()
print("ready", flush=True)
t0 = time.time()
while time.time() - t0 < float(sys.argv[1]):
    for _ in range(8):
        torch.matmul(a, a, out=b)
    torch.cuda.synchronize()
"""


def test_training_under_concurrent_gpu_load(lgb, gpu_required):
    """The frontier partition assumes nothing about co-residency: with another process's long
    matmul kernels occupying CUs (fewer of the partition's blocks resident, look-backs waiting on
    blocks that have not started), training completes and grows the same trees as without the
    load (profiles/r05/ab_notes.md, resident partition grid)."""
    import subprocess
    import sys
    import time

    from lambdagap_amd.utils import make_higgs_like

    X, y = make_higgs_like(2_000_000, seed=11)
    params = {"objective": "binary", "num_leaves": 63, "device_type": "gpu", "verbosity": -1}

    def model():
        b = lgb.train(params, lgb.Dataset(X, y, params=params), 8)
        s = b.model_to_string()
        return s[:s.index("parameters:")]

    ref = model()
    load = subprocess.Popen([sys.executable, "-c", _GPU_LOAD, "60"], stdout=subprocess.PIPE, text=True)
    try:
        import select

        t0 = time.time()
        line = ""
        while time.time() - t0 < 90 and load.poll() is None:
            ready, _, _ = select.select([load.stdout], [], [], 1.0)
            if ready:
                line = load.stdout.readline()
                if line.startswith("ready"):
                    break
        if not line.startswith("ready"):
            pytest.skip("the GPU load process did not start (torch import / device unavailable)")
        time.sleep(1.0)
        t1 = time.time()
        got = model()
        assert load.poll() is None, "the load ended before training did"
        assert got == ref
        assert time.time() - t1 < 60
    finally:
        load.kill()
        load.wait()
