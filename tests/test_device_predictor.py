"""Booster.device_predictor on the GPU against Booster.predict on the host and against
Booster.predict_device: both kernel families of the resident predictor.

Models are trained on the CPU learner (predict_device_cases.py, which also states the thresholds
of the row-parallel kernels), so this file tests only the prediction path.

Thresholds of the tree-parallel kernels that the shapes are chosen around
(src/device/predict_kernels.h):
  * a block has 256 lanes, owns one staged run of trees and one row tile, and spreads its lanes
    over the tile's rows x the run's trees;
  * the row tile is 64 rows for batches of up to 1,024 rows and 256 rows above;
  * a tile's rows are staged in LDS while tile * ncol * sizeof(value) <= 32 KiB: with the 64-row
    tile up to 128 fp32 / 64 fp64 columns, with the 256-row tile up to 32 fp32 / 16 fp64 columns
    (28 fp64 columns are read from global memory there), the 600-column model never;
  * trees are staged in LDS within the 8 KiB budget of the row-parallel kernels, larger trees are
    walked from global memory;
  * tree_parallel_rows is at most 65,536.
"""
import numpy as np
import pytest

import lambdagap_amd as lgb

from predict_device_cases import CASES, case, same

pytestmark = pytest.mark.gpu

PAIR_LANES = 256
PAIR_SMALL_TILE = 64
PAIR_LARGE_TILE = 256
PAIR_SMALL_TILE_MAX_ROWS = 1024
MAX_TREE_PARALLEL_ROWS = 65536

# the issue's counts, then the edges of the two row tiles and of the switch between them
ROW_COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025,
              PAIR_SMALL_TILE - 1, 2 * PAIR_SMALL_TILE, 2 * PAIR_SMALL_TILE + 1, PAIR_SMALL_TILE_MAX_ROWS - 1,
              PAIR_SMALL_TILE_MAX_ROWS, PAIR_SMALL_TILE_MAX_ROWS + PAIR_LARGE_TILE,
              PAIR_SMALL_TILE_MAX_ROWS + PAIR_LARGE_TILE + 1]
ROW_COUNTS = sorted(set(ROW_COUNTS))


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_required):
    return gpu_required


@pytest.fixture(scope="module")
def host_ref():
    """Booster.predict's results per (case, dtype), computed once."""
    cache = {}

    def get(name, dtype):
        key = (name, np.dtype(dtype).name)
        if key not in cache:
            booster, X64 = case(name)
            X = X64.astype(dtype)
            cache[key] = (booster, X, booster.predict(X, raw_score=True), booster.predict(X, pred_leaf=True),
                          booster.predict(X))
        return cache[key]

    return get


# ---------------------------------------------------------------- exactness, numpy input
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", CASES)
def test_numpy_equals_predict(name, dtype, host_ref):
    booster, X, raw, leaf, normal = host_ref(name, dtype)
    assert X.shape[0] <= MAX_TREE_PARALLEL_ROWS
    dev_raw = booster.predict_device(X, raw_score=True)
    dev_leaf = booster.predict_device(X, pred_leaf=True)
    for rows, path in ((MAX_TREE_PARALLEL_ROWS, "tree"), (0, "row")):
        with booster.device_predictor(tree_parallel_rows=rows) as pred:
            got = pred.predict(X, raw_score=True)
            assert pred.last_path == path
            assert isinstance(got, np.ndarray) and got.dtype == np.float64
            assert same(got, raw) and same(got, dev_raw)
            got_leaf = pred.predict(X, pred_leaf=True)
            assert pred.last_path == path
            assert got_leaf.dtype == leaf.dtype and same(got_leaf, leaf) and same(got_leaf, dev_leaf)
            assert same(pred.predict(X), normal)
            assert pred.last_path == path


@pytest.mark.parametrize("nrow", ROW_COUNTS)
def test_row_counts(nrow, host_ref):
    for name in ("binary", "multiclass6"):
        for dtype in (np.float64, np.float32):
            booster, X, raw, leaf, _ = host_ref(name, dtype)
            idx = np.arange(nrow) % X.shape[0]  # a leading slice; the longest counts wrap around
            Xs = np.ascontiguousarray(X[idx])
            for rows, path in ((MAX_TREE_PARALLEL_ROWS, "tree"), (0, "row")):
                with booster.device_predictor(tree_parallel_rows=rows) as pred:
                    assert same(pred.predict(Xs, raw_score=True), raw[idx])
                    assert pred.last_path == path
                    assert same(pred.predict(Xs, pred_leaf=True), leaf[idx])
                    assert pred.last_path == path


def test_threshold_between_the_paths(host_ref):
    for name in ("binary", "multiclass6"):
        booster, X, raw, leaf, normal = host_ref(name, np.float32)
        with booster.device_predictor(tree_parallel_rows=256) as pred:
            for nrow, path in ((256, "tree"), (257, "row"), (256, "tree")):
                Xs = np.ascontiguousarray(X[:nrow])
                assert same(pred.predict(Xs, raw_score=True), raw[:nrow])
                assert pred.last_path == path
                assert same(pred.predict(Xs, pred_leaf=True), leaf[:nrow])
                assert same(pred.predict(Xs), normal[:nrow])
                assert pred.last_path == path


def test_default_threshold_serves_every_size(host_ref):
    booster, X, raw, _, _ = host_ref("binary", np.float32)
    with booster.device_predictor() as pred:
        for nrow in (1, 300, X.shape[0]):
            assert same(pred.predict(np.ascontiguousarray(X[:nrow]), raw_score=True), raw[:nrow])
            assert pred.last_path in ("row", "tree")


def test_iteration_slice_and_shape_check(host_ref):
    booster, X, _, _, _ = host_ref("binary", np.float64)
    kw = dict(start_iteration=3, num_iteration=5)
    leaf = booster.predict(X, pred_leaf=True, **kw)
    for rows in (MAX_TREE_PARALLEL_ROWS, 0):
        with booster.device_predictor(tree_parallel_rows=rows, **kw) as pred:
            assert same(pred.predict(X, raw_score=True), booster.predict(X, raw_score=True, **kw))
            assert leaf.shape[1] == 5 and same(pred.predict(X, pred_leaf=True), leaf)
            assert same(pred.predict(X), booster.predict(X, **kw))
            extra = np.ascontiguousarray(np.hstack([X, X[:, :2]]))
            with pytest.raises(lgb.LightGBMError, match="number of features"):
                pred.predict(extra)
        with booster.device_predictor(tree_parallel_rows=rows, predict_disable_shape_check=True) as pred:
            assert same(pred.predict(extra, raw_score=True), booster.predict(X, raw_score=True))
            narrow = np.ascontiguousarray(X[:, :20])
            ref = booster.predict(narrow, raw_score=True, predict_disable_shape_check=True)
            assert same(pred.predict(narrow, raw_score=True), ref)


# ---------------------------------------------------------------- the predictor is a snapshot
def test_snapshot_and_coexistence():
    rng = np.random.default_rng(11)
    X = rng.normal(size=(1500, 12))
    y = (X[:, 0] * X[:, 1] + 0.2 * rng.normal(size=1500) > 0).astype(np.float64)
    params = {"objective": "binary", "num_leaves": 15, "device_type": "cpu", "verbosity": -1, "num_threads": 4,
              "seed": 1, "deterministic": True}
    booster = lgb.Booster(params, lgb.Dataset(X, y, params=params))
    for _ in range(12):
        booster.update()
    ref10 = booster.predict(X, raw_score=True, num_iteration=10)
    ref10_prob = booster.predict(X, num_iteration=10)
    ref_mid = booster.predict(X, raw_score=True, start_iteration=4, num_iteration=6)
    ref_all = booster.predict(X, raw_score=True)
    first = booster.device_predictor(num_iteration=10, tree_parallel_rows=MAX_TREE_PARALLEL_ROWS)
    mid = booster.device_predictor(start_iteration=4, num_iteration=6, tree_parallel_rows=0)
    whole = booster.device_predictor(tree_parallel_rows=MAX_TREE_PARALLEL_ROWS)
    assert same(first.predict(X, raw_score=True), ref10) and same(mid.predict(X, raw_score=True), ref_mid)
    # the booster moves on: more trees, one taken back, a leaf of the first tree rewritten
    for _ in range(3):
        booster.update()
    booster.rollback_one_iter()
    booster.set_leaf_output(0, 0, booster.get_leaf_output(0, 0) + 1.0)
    assert not same(booster.predict(X, raw_score=True, num_iteration=10), ref10)
    assert same(first.predict(X, raw_score=True), ref10)
    assert same(first.predict(X), ref10_prob)
    assert same(mid.predict(X, raw_score=True), ref_mid)
    assert same(whole.predict(X, raw_score=True), ref_all)
    assert (first.last_path, mid.last_path, whole.last_path) == ("tree", "row", "tree")
    for pred in (first, mid, whole):
        pred.free()


def test_free_and_context_manager(host_ref):
    booster, X, raw, _, _ = host_ref("binary", np.float64)
    pred = booster.device_predictor()
    assert same(pred.predict(X[:10], raw_score=True), raw[:10])
    pred.free()
    pred.free()  # harmless
    with pytest.raises(lgb.LightGBMError, match="after free"):
        pred.predict(X[:10])
    with booster.device_predictor() as held:
        assert same(held.predict(X[:10], raw_score=True), raw[:10])
    with pytest.raises(lgb.LightGBMError, match="after free"):
        held.predict(X[:10])


def test_refusals():
    booster, X = case("binary")
    with pytest.raises(lgb.LightGBMError, match="pred_contrib.*Booster.predict"):
        booster.device_predictor(pred_contrib=True)
    with pytest.raises(lgb.LightGBMError, match="pred_early_stop.*Booster.predict"):
        booster.device_predictor(pred_early_stop=True)
    with pytest.raises(ValueError, match="tree_parallel_rows"):
        booster.device_predictor(tree_parallel_rows=MAX_TREE_PARALLEL_ROWS + 1)
    with booster.device_predictor() as pred:
        with pytest.raises(TypeError, match="Booster.predict"):
            pred.predict(X[:5].tolist())


# ---------------------------------------------------------------- device tensors
# As in test_predict_device.py, the tensor checks run in one fresh interpreter in which torch
# creates its context before the library's first GPU call, and report one verdict per check.
_TENSOR_CHILD = r"""
import json, sys
import numpy as np
import torch
assert torch.cuda.is_available(), "torch sees no GPU"
torch.zeros(1, device="cuda")
torch.cuda.synchronize()
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import lambdagap_amd as lgb
from predict_device_cases import CASES, case, same
assert lgb.device_count() >= 1, "the library sees no GPU"
PATHS = ((65536, "tree"), (0, "row"))


def tensor_case(name, dtype):
    booster, X64 = case(name)
    X = X64.astype(dtype)
    raw, leaf, normal = booster.predict(X, raw_score=True), booster.predict(X, pred_leaf=True), booster.predict(X)
    t = torch.from_numpy(X).cuda()
    dev_raw = booster.predict_device(t, raw_score=True).cpu().numpy()
    dev_leaf = booster.predict_device(t, pred_leaf=True).cpu().numpy()
    for rows, path in PATHS:
        with booster.device_predictor(tree_parallel_rows=rows) as pred:
            got = pred.predict(t, raw_score=True)
            assert pred.last_path == path
            assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.device == t.device
            assert tuple(got.shape) == raw.shape
            assert same(got.cpu().numpy(), raw) and same(got.cpu().numpy(), dev_raw)
            got_leaf = pred.predict(t, pred_leaf=True)
            assert pred.last_path == path
            assert got_leaf.dtype == torch.float64 and got_leaf.device == t.device
            assert same(got_leaf.cpu().numpy(), leaf) and same(got_leaf.cpu().numpy(), dev_leaf)
            # transformed on the device: predict_device's bound for device-versus-host transcendentals
            conv = pred.predict(t)
            assert conv.dtype == torch.float64 and conv.device == t.device and tuple(conv.shape) == normal.shape
            np.testing.assert_allclose(conv.cpu().numpy(), normal, rtol=1e-12, atol=1e-12)


def reuse(name):
    # 513 rows, then 1, then 513 again, numpy and tensor input in turn, raw / leaf / normal in turn:
    # every result equals the first of its kind, whatever the buffers held before
    booster, X64 = case(name)
    X = X64.astype(np.float32)
    kinds = (dict(raw_score=True), dict(pred_leaf=True), dict())
    for rows, path in PATHS + ((300, None),):
        first = {}
        with booster.device_predictor(tree_parallel_rows=rows) as pred:
            previous = None
            call = 0
            for rnd in range(3):  # the third round repeats the first's pairing of size, kind and input
                for nrow in (513, 1, 513):
                    for kind in range(3):
                        as_tensor = call % 2 == 1
                        call += 1
                        if previous is not None:  # the last result is ours: scribble over it
                            if isinstance(previous, torch.Tensor):
                                previous.fill_(-7.25)
                                torch.cuda.synchronize()
                            else:
                                previous.fill(-7)
                        data = torch.from_numpy(X[:nrow]).cuda() if as_tensor else np.ascontiguousarray(X[:nrow])
                        got = pred.predict(data, **kinds[kind])
                        if path is not None:
                            assert pred.last_path == path
                        else:
                            assert pred.last_path == ("tree" if nrow <= rows else "row")
                        previous = got
                        val = got.cpu().numpy().copy() if as_tensor else got.copy()
                        key = (nrow, kind, as_tensor)
                        if key in first:
                            assert same(val, first[key]), key
                        else:
                            first[key] = val
                        if kind < 2:  # raw and leaf: the host's bits, from either input
                            ref = booster.predict(X[:nrow], **kinds[kind])
                            assert same(val.reshape(ref.shape).astype(ref.dtype), ref), key
            assert len(first) == 12


def non_contiguous():
    booster, X64 = case("binary")
    X = X64.astype(np.float32)
    raw = booster.predict(X, raw_score=True)
    pad = np.zeros((X.shape[0], 2 * X.shape[1]), dtype=np.float32)
    pad[:, ::2] = X
    view = torch.from_numpy(pad).cuda()[:, ::2]
    assert not view.is_contiguous()
    for rows, path in PATHS:
        with booster.device_predictor(tree_parallel_rows=rows) as pred:
            got = pred.predict(view, raw_score=True).cpu().numpy()
            assert same(got, pred.predict(view.contiguous(), raw_score=True).cpu().numpy())
            assert same(got, raw) and pred.last_path == path


def other_dtype():
    booster, X64 = case("binary")
    half = torch.from_numpy(np.round(X64[:100] * 4) / 4).cuda().to(torch.float16)
    ref = booster.predict(half.cpu().numpy().astype(np.float64), raw_score=True)
    for rows, path in PATHS:
        with booster.device_predictor(tree_parallel_rows=rows) as pred:
            assert same(pred.predict(half, raw_score=True).cpu().numpy(), ref) and pred.last_path == path


def host_tensor_refused():
    booster, X64 = case("binary")
    with booster.device_predictor() as pred:
        try:
            pred.predict(torch.from_numpy(X64[:5]))
        except TypeError as e:
            assert "Booster.predict" in str(e)
        else:
            raise AssertionError("a host tensor was accepted")


checks = {f"{name}-{dtype}": (lambda n=name, d=dtype: tensor_case(n, d))
          for name in CASES for dtype in ("float64", "float32")}
checks.update({"reuse-binary": lambda: reuse("binary"), "reuse-multiclass6": lambda: reuse("multiclass6")})
checks.update(non_contiguous=non_contiguous, other_dtype=other_dtype, host_tensor_refused=host_tensor_refused)
res = {}
for key, fn in checks.items():
    try:
        fn()
        res[key] = "ok"
    except Exception as e:  # the verdict travels to the parent test
        res[key] = f"{type(e).__name__}: {e}"[:1500]
print("RESULT " + json.dumps(res), flush=True)
"""


@pytest.fixture(scope="module")
def tensor_verdicts():
    import json
    import os
    import subprocess
    import sys

    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _TENSOR_CHILD, os.path.dirname(tests), tests], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", CASES)
def test_tensor_equals_predict(name, dtype, tensor_verdicts):
    assert tensor_verdicts[f"{name}-{dtype}"] == "ok"


@pytest.mark.parametrize("check", ["reuse-binary", "reuse-multiclass6", "non_contiguous", "other_dtype",
                                   "host_tensor_refused"])
def test_tensor_inputs(check, tensor_verdicts):
    assert tensor_verdicts[check] == "ok"
