"""Times Booster.predict(pred_contrib=True) (host recursion) against Booster.predict_contrib_device
on one MI355X.

The model has the headline shape: 28 features, 63 leaves, binary objective, trained on the GPU.
For each row count it times SHAP values three ways: the host's OpenMP row loop, predict_contrib_device
on a numpy array (upload + kernel + download) and on a float32 tensor already on the GPU (kernel
only, output left on the device). Every device timing ends in a completed call (the library
synchronises its stream before returning, and the clock stops after torch.cuda.synchronize());
each variant is warmed up once per shape and the minimum and median of the repeats are printed.

The host loop is tens of seconds per million rows, so it is given a time budget: at a row count
where warm-up plus repeats would not fit (projected from the rate at the previous row count), it is
timed with one call, or skipped when even that does not fit; the table says which.

    python scripts/bench_contrib.py --rows 100000 1000000 10000000 --trees 100 --out profiles/contrib.md

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


def timed(fn, repeats, warm=True, sync=None):
    if warm:
        fn()  # warm-up: code objects, allocations
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        if sync is not None:
            sync()
        ts.append(time.perf_counter() - t0)
        print(f"  call {len(ts)}/{repeats}: {ts[-1]:.4f} s", file=sys.stderr, flush=True)
    return min(ts), statistics.median(ts)


def err(got, ref):
    scale = np.maximum(1.0, np.abs(ref).max(axis=1))
    return float((np.abs(got - ref).max(axis=1) / scale).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100_000, 1_000_000, 10_000_000])
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--train-rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-budget", type=float, default=600.0, help="seconds the host column may take per row count")
    ap.add_argument("--no-tensor", action="store_true", help="skip the device-tensor variant (no torch)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    torch = None
    if not args.no_tensor:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench_contrib: torch sees no GPU (use --no-tensor to time numpy input only)")
        torch.zeros(1, device="cuda")
        torch.cuda.synchronize()

    import lambdagap_amd as lgb
    from lambdagap_amd.utils import make_higgs_like

    if lgb.device_count() < 1:
        raise SystemExit("bench_contrib: no gfx950 GPU visible")
    X, y = make_higgs_like(max(max(args.rows), args.train_rows), seed=11)
    X = np.ascontiguousarray(X, dtype=np.float32)
    params = {"objective": "binary", "num_leaves": 63, "learning_rate": 0.1, "max_bin": 255, "device_type": "gpu",
              "verbosity": -1}
    nt = min(args.train_rows, X.shape[0])
    booster = lgb.train(params, lgb.Dataset(X[:nt], y[:nt], params=params), num_boost_round=args.trees)
    threads = os.environ.get("OMP_NUM_THREADS", "all")
    lines = [
        "# Booster.predict_contrib_device vs Booster.predict(pred_contrib=True) on one MI355X (scripts/bench_contrib.py)",
        "",
        f"Model: binary, 28 features, 63 leaves, {booster.num_trees()} trees; SHAP values (29 doubles per row), float32 "
        f"rows; host loop with {threads} OpenMP threads; min / median of {args.repeats} calls after one warm-up call, "
        "seconds; krow/s from the minimum.",
        "",
        "| rows | predict(pred_contrib=True) (host) | predict_contrib_device, numpy in / numpy out | "
        "predict_contrib_device, GPU tensor in / out | max err vs host |",
        "|---:|---:|---:|---:|---:|",
    ]
    host_rate = None  # rows per second of the host loop, from the last row count it ran at
    probe = min(10_000, min(args.rows))
    t0 = time.perf_counter()
    booster.predict(X[:probe], pred_contrib=True)
    host_rate = probe / (time.perf_counter() - t0)
    for n in args.rows:
        Xn = X[:n]
        cells = []
        ref = None
        projected = n / host_rate
        if projected * (args.repeats + 1) <= args.host_budget:
            ref = booster.predict(Xn, pred_contrib=True)  # the warm-up call
            print(f"  host warm-up done at {n} rows", file=sys.stderr, flush=True)
            lo, med = timed(lambda: booster.predict(Xn, pred_contrib=True), args.repeats, warm=False)
            cells.append(f"{lo:.3f} / {med:.3f} ({n / lo / 1e3:.1f} krow/s)")
            host_rate = n / lo
        elif projected <= args.host_budget:
            t0 = time.perf_counter()
            ref = booster.predict(Xn, pred_contrib=True)
            lo = time.perf_counter() - t0
            cells.append(f"{lo:.3f} (one call, no warm-up) ({n / lo / 1e3:.1f} krow/s)")
            host_rate = n / lo
        else:
            cells.append(f"skipped (projected {projected:.0f} s per call)")
        got = booster.predict_contrib_device(Xn)
        worst = err(got, ref) if ref is not None else None
        lo, med = timed(lambda: booster.predict_contrib_device(Xn), args.repeats)
        cells.append(f"{lo:.4f} / {med:.4f} ({n / lo / 1e3:.1f} krow/s)")
        if torch is not None:
            t = torch.from_numpy(Xn).cuda()
            torch.cuda.synchronize()
            out = booster.predict_contrib_device(t)
            same = bool(np.array_equal(got, out.cpu().numpy()))
            del out
            lo, med = timed(lambda: booster.predict_contrib_device(t), args.repeats, sync=torch.cuda.synchronize)
            cells.append(f"{lo:.4f} / {med:.4f} ({n / lo / 1e3:.1f} krow/s)" + ("" if same else " DIFFERS FROM NUMPY PATH"))
            del t
        else:
            cells.append("not measured")
        del got, ref
        lines.append(f"| {n:,} | {cells[0]} | {cells[1]} | {cells[2]} | "
                     f"{'not measured' if worst is None else format(worst, '.2e')} |")
        print(lines[-1], flush=True)
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)


if __name__ == "__main__":
    main()
