"""lgb.Dataset from feature tensors that already live on the GPU, against the numpy path.

The rule of every check: a Dataset built from torch.from_numpy(X).cuda(), or from a view with
X's values, equals the Dataset built from X as a numpy array: group layout, every group bin and
model_to_string() after 5 rounds with device_type=gpu. These are exact equalities.

The shapes sit at the kernels' thresholds (src/device/bin_kernels.hip, restated in
dataset_device_cases.py): an LDS tile of R = min(1024, 32 KiB / row bytes) rows, so row counts
1, 63, R and 2R + 313; 29 fp32 columns put row bases off 16-byte alignment; max_bin=1023 gives
two-byte bins; 60 x 255 bins exceed the 96 KiB the bound tables may take in LDS; 4,100 fp64
columns exceed the 32 KiB tile and take the per-(row, group) kernel.
"""
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(gpu_required):
    return gpu_required


# torch wheels bundle a ROCm runtime of their own, and a process serves both torch and this
# library only when torch created its context first (tests/test_predict_device.py). So all
# tensor work runs in one fresh interpreter that starts with torch, and reports one verdict per
# check. A HIP error ends it: nothing is caught past the first one.
_CHILD = r"""
import json, sys
import numpy as np
import torch
assert torch.cuda.is_available(), "torch sees no GPU"
torch.zeros(1, device="cuda")
torch.cuda.synchronize()
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import lambdagap_amd as lgb
from dataset_device_cases import (CHUNK_ROWS, N_ROWS, PACK_TABLE_BYTES, PACK_TILE_BYTES, SAMPLE_CNT, make_label,
                                  make_matrix, params_for, same_signature, signature, tile_rows)
assert lgb.device_count() >= 1, "the library sees no GPU"


class Lines:
    def __init__(self):
        self.lines = []

    def info(self, m):
        self.lines.append(m)

    def warning(self, m):
        self.lines.append(m)

    def take(self):
        out, self.lines = self.lines, []
        return out


LOG = Lines()
lgb.register_logger(LOG)


def gpu_params(ncol, **over):
    return params_for(ncol, **dict({"device_type": "gpu"}, **over))


def outcome(fn):
    # the value, or the error it ends with (a one-row set may refuse to train: then both must)
    try:
        return fn()
    except lgb.LightGBMError as e:
        return "LightGBMError: " + str(e)


def train_text(data, y, p, rounds=5, **kw):
    return outcome(lambda: lgb.train(p, lgb.Dataset(data, y, params=p), num_boost_round=rounds, **kw).model_to_string())


def assert_same_dataset(t, X, y, p, train=True):
    assert tuple(t.shape) == X.shape and t.is_cuda
    ref = signature(lgb.Dataset(X, y, params=p).construct())
    got = signature(lgb.Dataset(t, y, params=p).construct())
    assert got[0] == ref[0], (got[0], ref[0])
    assert same_signature(got, ref), "group bins differ in %d places" % int((got[2] != ref[2]).sum())
    if train:
        a, b = train_text(t, y, p), train_text(X, y, p)
        assert a == b, (a[:200], b[:200])
    return ref


def tensor_views(X):
    # name -> a GPU view with X's values and the strides the name says
    t = torch.from_numpy(X).cuda()
    n, ncol = X.shape
    big = torch.full((n, ncol + 7), 123.0, dtype=t.dtype, device="cuda")
    big[:, 3:3 + ncol] = t
    doubled = torch.full((2 * n, ncol), -5.0, dtype=t.dtype, device="cuda")
    doubled[::2] = t
    feature_major = t.T.contiguous()
    spread = torch.full((2 * n, 2 * ncol), 9.0, dtype=t.dtype, device="cuda")
    spread[::2, ::2] = t
    views = {"contiguous": t, "column_slice": big[:, 3:3 + ncol], "row_step": doubled[::2],
             "transposed": feature_major.T, "no_unit_stride": spread[::2, ::2]}
    assert views["column_slice"].stride() == (ncol + 7, 1)
    assert views["row_step"].stride() == (2 * ncol, 1)
    assert views["transposed"].stride() == (1, n)
    assert views["no_unit_stride"].stride() == (4 * ncol, 2)
    for v in views.values():
        assert np.array_equal(v.cpu().numpy(), X, equal_nan=True)
    return views


def shapes(dtype, ncol):
    item = np.dtype(dtype).itemsize
    R = tile_rows(ncol, item)
    if ncol == 29 and item == 4:
        assert (ncol * item) % 16 != 0  # row bases off 16-byte alignment
    for nrow in (1, 63, R, 2 * R + 313):
        X = make_matrix(n=nrow, ncol=ncol, seed=nrow, dtype=dtype)
        y = make_label(X)
        assert_same_dataset(torch.from_numpy(X).cuda(), X, y, gpu_params(ncol))


def wide_bins():
    X = make_matrix(dtype=np.float32)
    y = make_label(X)
    ref = assert_same_dataset(torch.from_numpy(X).cuda(), X, y, gpu_params(12, max_bin=1023))
    assert ref[0][2] == 2  # two-byte bins
    v = tensor_views(X)
    for name in ("column_slice", "transposed"):
        assert_same_dataset(v[name], X, y, gpu_params(12, max_bin=1023), train=False)


def unstaged_tables():
    X = np.ascontiguousarray(make_matrix(n=2361, ncol=72, seed=3, dtype=np.float32)[:, 12:])
    y = make_label(X)
    p = gpu_params(60, enable_bundle=False, min_data_in_bin=1)
    p.pop("categorical_feature")
    ref = assert_same_dataset(torch.from_numpy(X).cuda(), X, y, p)
    assert ref[0][0] == 60 and ref[0][1] * 8 > PACK_TABLE_BYTES, ref[0]
    v = tensor_views(X)
    for name in ("column_slice", "transposed"):
        assert_same_dataset(v[name], X, y, p, train=False)


def wide_rows():
    X = make_matrix(n=300, ncol=4100, seed=4, dtype=np.float64)
    assert X.shape[1] * 8 > PACK_TILE_BYTES
    y = make_label(X)
    p = gpu_params(4100, max_bin=15)
    assert_same_dataset(torch.from_numpy(X).cuda(), X, y, p)
    v = tensor_views(X)
    for name in ("column_slice", "transposed", "no_unit_stride"):
        assert_same_dataset(v[name], X, y, p, train=False)


def strided(dtype, name):
    item = np.dtype(dtype).itemsize
    for nrow in (N_ROWS, 2 * tile_rows(12, item) + 313):
        X = make_matrix(n=nrow, dtype=dtype)
        y = make_label(X)
        v = tensor_views(X)[name]
        assert not v.is_contiguous()
        assert_same_dataset(v, X, y, gpu_params(12))


def chunk_list():
    n = sum(CHUNK_ROWS)
    X = make_matrix(n=n, dtype=np.float32)
    y = make_label(X)
    cuts = np.cumsum((0,) + CHUNK_ROWS)
    parts = [np.ascontiguousarray(X[cuts[i]:cuts[i + 1]]) for i in range(3)]
    chunks = [torch.from_numpy(parts[0]).cuda(), tensor_views(parts[1])["column_slice"],
              tensor_views(parts[2])["transposed"]]
    assert [int(c.shape[0]) for c in chunks] == list(CHUNK_ROWS)
    p = gpu_params(12)
    ref = signature(lgb.Dataset(X, y, params=p).construct())
    assert same_signature(signature(lgb.Dataset(chunks, y, params=p).construct()), ref)
    assert train_text(chunks, y, p) == train_text(X, y, p)
    bad = [chunks[0], torch.zeros((4, 11), dtype=torch.float32, device="cuda")]
    try:
        lgb.Dataset(bad, None, params=p).construct()
    except ValueError as e:
        assert "same number of columns" in str(e)
    else:
        raise AssertionError("chunks of 12 and 11 columns were accepted")


def num_bins(ds):
    return [ds.feature_num_bin(j) for j in range(ds.num_feature())]


def sampling():
    X = make_matrix(dtype=np.float64)
    y = make_label(X)
    t = torch.from_numpy(X).cuda()
    for cnt in (SAMPLE_CNT, N_ROWS + 5):  # a real sample of 1,000 of 5,000 rows; every row
        p = gpu_params(12, bin_construct_sample_cnt=cnt)
        a = lgb.Dataset(t, y, params=p).construct()
        b = lgb.Dataset(X, y, params=p).construct()
        assert num_bins(a) == num_bins(b)
        assert same_signature(signature(a), signature(b))
    full = num_bins(lgb.Dataset(X, y, params=gpu_params(12, bin_construct_sample_cnt=N_ROWS)).construct())
    part = num_bins(lgb.Dataset(X, y, params=gpu_params(12)).construct())
    assert full != part  # the sample matters at this size


def validation_set():
    X, Xv = make_matrix(dtype=np.float32), make_matrix(n=1237, seed=11, dtype=np.float32)
    Xv[5, 2] = 77  # a category the training set has not seen
    y, yv = make_label(X), make_label(Xv)
    p = gpu_params(12, metric=["binary_logloss", "auc"])
    hist = {}
    for kind in ("numpy", "tensor"):
        conv = (lambda a: a) if kind == "numpy" else (lambda a: torch.from_numpy(a).cuda())
        train = lgb.Dataset(conv(X), y, params=p)
        valid = lgb.Dataset(conv(Xv), yv, reference=train)
        rec = {}
        bst = lgb.train(p, train, num_boost_round=5, valid_sets=[valid], valid_names=["v"],
                        callbacks=[lgb.record_evaluation(rec)])
        hist[kind] = (signature(valid), json.dumps(rec, sort_keys=True), bst.model_to_string())
    assert same_signature(hist["numpy"][0], hist["tensor"][0])
    assert hist["numpy"][1] == hist["tensor"][1] and len(json.loads(hist["numpy"][1])["v"]["auc"]) == 5
    assert hist["numpy"][2] == hist["tensor"][2]
    # a view as the validation set, on a constructed reference
    train = lgb.Dataset(X, y, params=p).construct()
    v = lgb.Dataset(tensor_views(Xv)["transposed"], yv, reference=train).construct()
    assert same_signature(signature(v), hist["numpy"][0])


def parameters_do_not_matter():
    X = make_matrix(dtype=np.float32)
    y = make_label(X)
    t = torch.from_numpy(X).cuda()
    for over in ({"device_type": "cpu"}, {"device_type": "cpu", "device_binning": False},
                 {"device_type": "gpu", "device_binning": False}):
        assert_same_dataset(t, X, y, params_for(12, **over))


def fallback():
    X = make_matrix(dtype=np.float32)
    y = make_label(X)
    p = gpu_params(12, linear_tree=True, verbosity=1)
    p.pop("categorical_feature")
    t = tensor_views(X)["column_slice"]
    LOG.take()
    ds = lgb.Dataset(t, y, params=p).construct()
    lines = [ln for ln in LOG.take() if "copying the matrix to the host" in ln]
    assert len(lines) == 1 and "linear_tree" in lines[0], lines
    assert same_signature(signature(ds), signature(lgb.Dataset(X, y, params=p).construct()))
    LOG.take()
    assert train_text(t, y, p) == train_text(X, y, p)
    assert "Device::CopyRowsToHost" in lgb.phase_timer_report()


def metadata():
    X = make_matrix(dtype=np.float32)
    y = make_label(X)
    rng = np.random.default_rng(2)
    w = rng.uniform(0.5, 2.0, len(y)).astype(np.float32)
    init = rng.normal(size=len(y))
    p = gpu_params(12)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    t = cuda(X)
    ref = lgb.train(p, lgb.Dataset(X, y, weight=w, init_score=init, params=p), 5).model_to_string()
    got = lgb.train(p, lgb.Dataset(t, cuda(y), weight=cuda(w), init_score=cuda(init), params=p), 5).model_to_string()
    assert got == ref
    ds = lgb.Dataset(t, params=p).construct()  # through the setters of a constructed Dataset
    ds.set_label(cuda(y)).set_weight(cuda(w)).set_init_score(cuda(init))
    assert lgb.train(p, ds, 5).model_to_string() == ref
    np.testing.assert_array_equal(ds.get_label(), y.astype(np.float32))
    # ranking: query sizes and positions as GPU tensors
    n = 1200
    Xr = make_matrix(n=n, seed=6, dtype=np.float32)
    yr = rng.integers(0, 4, n).astype(np.float64)
    group = np.array([100] * 6 + [50] * 12, dtype=np.int32)
    pr = gpu_params(12, objective="lambdarank", metric="ndcg")
    a = lgb.train(pr, lgb.Dataset(Xr, yr, group=group, params=pr), 5).model_to_string()
    b = lgb.train(pr, lgb.Dataset(cuda(Xr), cuda(yr), group=cuda(group), params=pr), 5).model_to_string()
    assert a == b
    d = lgb.Dataset(cuda(Xr), cuda(yr), group=cuda(group), position=cuda((np.arange(n) % 7).astype(np.int32)),
                    params=pr).construct()
    np.testing.assert_array_equal(d.get_position(), np.arange(n) % 7)


def continued_training():
    X = make_matrix(dtype=np.float32)
    y = make_label(X)
    p = gpu_params(12)
    first = lgb.train(p, lgb.Dataset(X, y, params=p), 3)
    t = torch.from_numpy(X).cuda()
    a = lgb.train(p, lgb.Dataset(X, y, params=p), 4, init_model=first).model_to_string()
    b = lgb.train(p, lgb.Dataset(t, y, params=p), 4, init_model=first).model_to_string()
    assert a == b
    kept = lgb.Dataset(t, y, params=p, free_raw_data=False).construct()
    assert kept.get_data() is t
    try:
        kept.subset([0, 5, 9]).construct()
    except lgb.LightGBMError as e:
        assert "free_raw_data" in str(e)
    else:
        raise AssertionError("raw rows of a tensor-backed Dataset were subset")
    sub = lgb.Dataset(t, y, params=p).construct().subset([0, 5, 9]).construct()  # binned rows subset as ever
    assert sub.num_data() == 3


def adoption():
    # runs first: the phase timer must not yet hold a host-fallback copy
    X = make_matrix(dtype=np.float32)
    y = make_label(X)
    p = gpu_params(12, verbosity=2)
    p.pop("categorical_feature")  # the plain case of test_device_binned_dataset_trains_like_host_binned
    t = torch.from_numpy(X).cuda()
    ds = lgb.Dataset(t, y, params=p).construct()
    report = lgb.phase_timer_report()
    assert "Device::PackResident" in report and "Device::GatherRows" in report, report
    assert "Device::CopyRowsToHost" not in report and "Device::PackRows" not in report, report
    LOG.take()
    lgb.Booster(p, ds).update()
    assert any("adopted the device-binned rows" in ln for ln in LOG.take())
    # a validation set keeps no device copy: nothing for a learner to adopt by mistake
    lgb.Dataset(t, y, reference=ds).construct()


def end_to_end():
    X = make_matrix(dtype=np.float32)
    y = make_label(X)
    p = gpu_params(12)
    t, y_t = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    bst = lgb.train(p, lgb.Dataset(t, y_t), num_boost_round=5)
    ref = lgb.train(p, lgb.Dataset(X, y), num_boost_round=5)
    assert bst.model_to_string() == ref.model_to_string()
    got = bst.predict_device(t)
    assert got.is_cuda and tuple(got.shape) == (len(y),)
    # raw scores equal the all-numpy run bit for bit; the transformed scores of a device tensor are
    # computed on the device, so they equal the numpy model's on the same tensor exactly and the
    # host's within the device-versus-host bound of tests/test_predict_device.py
    assert np.array_equal(bst.predict_device(t, raw_score=True).cpu().numpy(), ref.predict(X, raw_score=True))
    assert np.array_equal(got.cpu().numpy(), ref.predict_device(t).cpu().numpy())
    np.testing.assert_allclose(got.cpu().numpy(), ref.predict(X), rtol=1e-12, atol=1e-12)


def other_dtype():
    X = np.round(make_matrix(dtype=np.float32) * 4) / 4  # exact in float16
    X[np.isnan(X)] = 0
    y = make_label(X)
    half = torch.from_numpy(X).cuda().to(torch.float16)
    assert_same_dataset(half, X, y, gpu_params(12))
    ints = torch.from_numpy(X * 4).cuda().to(torch.int32)
    assert_same_dataset(ints, (X * 4).astype(np.float32), y, gpu_params(12))


checks = {"adoption": adoption}
for dtype in ("float32", "float64"):
    for ncol in (1, 12, 29):
        checks["shapes-%s-%d" % (dtype, ncol)] = (lambda d=dtype, c=ncol: shapes(d, c))
    for name in ("column_slice", "row_step", "transposed", "no_unit_stride"):
        checks["strided-%s-%s" % (dtype, name)] = (lambda d=dtype, v=name: strided(d, v))
checks.update(wide_bins=wide_bins, unstaged_tables=unstaged_tables, wide_rows=wide_rows, chunk_list=chunk_list,
              sampling=sampling, validation_set=validation_set, parameters_do_not_matter=parameters_do_not_matter,
              metadata=metadata, continued_training=continued_training, end_to_end=end_to_end,
              other_dtype=other_dtype, fallback=fallback)
res = {}
for key, fn in checks.items():
    try:
        fn()
        res[key] = "ok"
    except Exception as e:  # the verdict travels to the parent test
        if "HIP error" in str(e):
            raise
        res[key] = f"{type(e).__name__}: {e}"[:1500]
print("RESULT " + json.dumps(res), flush=True)
"""

_SHAPES = [f"shapes-{d}-{c}" for d in ("float32", "float64") for c in (1, 12, 29)]
_STRIDED = [f"strided-{d}-{v}" for d in ("float32", "float64")
            for v in ("column_slice", "row_step", "transposed", "no_unit_stride")]
_OTHER = ["wide_bins", "unstaged_tables", "wide_rows", "chunk_list", "sampling", "validation_set",
          "parameters_do_not_matter", "fallback", "metadata", "continued_training", "adoption", "end_to_end",
          "other_dtype"]


@pytest.fixture(scope="module")
def verdicts():
    import json
    import os
    import subprocess
    import sys

    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(tests), tests], capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, LGAP_TIMETAG="1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.parametrize("check", _SHAPES)
def test_row_and_column_counts(check, verdicts):
    assert verdicts[check] == "ok"


@pytest.mark.parametrize("check", _STRIDED)
def test_strided_views(check, verdicts):
    assert verdicts[check] == "ok"


@pytest.mark.parametrize("check", _OTHER)
def test_tensor_dataset(check, verdicts):
    assert verdicts[check] == "ok"
