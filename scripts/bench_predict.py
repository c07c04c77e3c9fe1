"""Times Booster.predict (host loop) against Booster.predict_device on one MI355X.

The model has the headline shape: 28 features, 63 leaves, binary objective, trained on the GPU.
For each row count it times raw-score prediction three ways: the host loop, predict_device on a
numpy array (upload + kernel + download) and predict_device on a float32 tensor already on the
GPU (kernel only, output left on the device). Every timing ends in a completed call (the library
synchronises its stream before returning); each variant is warmed up once per shape and the
minimum and median of the repeats are printed. Results are checked equal before they are timed.

    python scripts/bench_predict.py --rows 100000 1000000 10000000 --trees 100 --out profiles/predict_device.md

torch is imported and creates its GPU context first: a torch wheel that bundles its own ROCm
runtime cannot see the device once the library's runtime has initialised it.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats):
    fn()  # warm-up: code objects, allocations
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100_000, 1_000_000, 10_000_000])
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--train-rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-tensor", action="store_true", help="skip the device-tensor variant (no torch)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    torch = None
    if not args.no_tensor:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench_predict: torch sees no GPU (use --no-tensor to time numpy input only)")
        torch.zeros(1, device="cuda")
        torch.cuda.synchronize()

    import lambdagap_amd as lgb
    from lambdagap_amd.utils import make_higgs_like

    if lgb.device_count() < 1:
        raise SystemExit("bench_predict: no gfx950 GPU visible")
    X, y = make_higgs_like(max(max(args.rows), args.train_rows), seed=11)
    X = np.ascontiguousarray(X, dtype=np.float32)
    params = {"objective": "binary", "num_leaves": 63, "learning_rate": 0.1, "max_bin": 255, "device_type": "gpu",
              "verbosity": -1}
    nt = min(args.train_rows, X.shape[0])
    booster = lgb.train(params, lgb.Dataset(X[:nt], y[:nt], params=params), num_boost_round=args.trees)
    lines = [
        "# Booster.predict_device vs Booster.predict on one MI355X (scripts/bench_predict.py)",
        "",
        f"Model: binary, 28 features, 63 leaves, {booster.num_trees()} trees; raw scores, float32 rows; host loop with "
        f"{os.environ.get('OMP_NUM_THREADS', 'all')} OpenMP threads; min / median of {args.repeats} calls after one "
        "warm-up call, seconds; Mrow/s from the minimum.",
        "",
        "| rows | predict (host) | predict_device, numpy in / numpy out | predict_device, GPU tensor in / out | equal |",
        "|---:|---:|---:|---:|---|",
    ]
    for n in args.rows:
        Xn = X[:n]
        ref = booster.predict(Xn, raw_score=True)
        got = booster.predict_device(Xn, raw_score=True)
        equal = bool(np.array_equal(ref, got))
        cells = []
        for fn in (lambda: booster.predict(Xn, raw_score=True), lambda: booster.predict_device(Xn, raw_score=True)):
            lo, med = timed(fn, args.repeats)
            cells.append(f"{lo:.4f} / {med:.4f} ({n / lo / 1e6:.1f} Mrow/s)")
        if torch is not None:
            t = torch.from_numpy(Xn).cuda()
            torch.cuda.synchronize()
            out = booster.predict_device(t, raw_score=True)
            equal = equal and bool(np.array_equal(ref, out.cpu().numpy()))
            lo, med = timed(lambda: booster.predict_device(t, raw_score=True), args.repeats)
            cells.append(f"{lo:.4f} / {med:.4f} ({n / lo / 1e6:.1f} Mrow/s)")
            del t, out
        else:
            cells.append("not measured")
        lines.append(f"| {n:,} | {cells[0]} | {cells[1]} | {cells[2]} | {'yes' if equal else 'NO'} |")
        print(lines[-1], flush=True)
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)


if __name__ == "__main__":
    main()
