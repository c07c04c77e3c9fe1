"""bench.py contract: `python bench.py --gpus N` outside torchrun launches N rank processes
itself (torch.distributed.run, 127.0.0.1 rendezvous) and relays exactly one JSON line from
rank 0, as the driver's multi-GPU scaling run invokes it. The CPU learner over gloo stands in
for the GPUs here."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_bench_spawns_ranks_and_relays_rank0_line():
    out = _run(["--gpus", "2", "--device", "cpu", "--rows", "20000", "--valid-rows", "4000", "--steps", "2",
                "--warmup", "1", "--full"])
    assert out["n_gpus"] == 2
    assert out["steps"] == 2 and out["warmup"] == 1
    assert out["config"]["parallelism"] == "dp2"
    assert out["config"]["transport"] == "gloo (host collectives)"
    assert out["value"] > 0 and 0.5 < out["auc"] <= 1.0


def test_bench_single_process_cpu():
    out = _run(["--device", "cpu", "--rows", "20000", "--valid-rows", "4000", "--steps", "2", "--warmup", "1"])
    assert out["n_gpus"] == 1 and out["config"]["transport"] is None
    for key in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert key in out
    # a plain run stops at the headline figure; the held-out AUC belongs to --full
    assert out["auc"] is None
    assert out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] - 1000.0) < 1.0


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the model's raw scores on a fixed sample of the training rows as
    float64 .npy files; the same arguments give the same inputs, hence (CPU learner) the same files."""
    import numpy as np

    dumps = []
    for d in ("a", "b"):
        _run(["--device", "cpu", "--rows", "20000", "--steps", "3", "--warmup", "1",
              "--dump-outputs", str(tmp_path / d)])
        files = sorted(p.name for p in (tmp_path / d).iterdir())
        assert files == ["last_step_raw_score.npy", "raw_score.npy"]
        dumps.append({f: np.load(tmp_path / d / f) for f in files})
    for f, a in dumps[0].items():
        assert a.dtype == np.float64 and a.shape == (20000,) and np.all(np.isfinite(a))
        np.testing.assert_array_equal(a, dumps[1][f])
    # 4 trees at learning rate 0.1: the last one alone is a strict part of the whole score
    assert np.ptp(dumps[0]["raw_score.npy"]) > np.ptp(dumps[0]["last_step_raw_score.npy"]) > 0
