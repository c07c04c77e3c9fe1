"""Times a boosting iteration with a custom objective on the host, on the GPU, and with the built-in one.

For each row count (make_higgs_like: 28 float32 features, device_type=gpu, 63 leaves) three
boosters train the same logistic loss:

  update(fobj)    the objective in numpy: the score is downloaded, the gradients are uploaded
  update_device   the same objective in torch on GPU tensors: nothing leaves the device
  built-in        objective=binary (the library's gradient kernel)

Each booster runs `--warmup` iterations, then `--repeats` batches of `--iters` iterations; a
batch's clock stops after a device synchronisation. The report gives iterations per second from
the fastest and the median batch, and what each custom path costs per iteration over the
built-in one.

    python scripts/bench_custom_objective.py --rows 1000000 10000000 --out profiles/update_device.md

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--num-leaves", type=int, default=63)
    ap.add_argument("--iters", type=int, default=20, help="iterations per timed batch")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--note", default="", help="commit and machine, copied into the report")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_custom_objective: torch sees no GPU")
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()

    import lambdagap_amd as lgb
    from lambdagap_amd.basic import _LIB, _check
    from lambdagap_amd.utils import make_higgs_like

    if lgb.device_count() < 1:
        raise SystemExit("bench_custom_objective: no gfx950 GPU visible")

    def sync():
        torch.cuda.synchronize()
        _check(_LIB.LGBM_DeviceSynchronize())

    def batches(step):
        for _ in range(args.warmup):
            step()
        sync()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for _ in range(args.iters):
                step()
            sync()
            ts.append((time.perf_counter() - t0) / args.iters)
        return {"min": min(ts), "median": statistics.median(ts)}

    X, y = make_higgs_like(max(args.rows), seed=11)
    X = np.ascontiguousarray(X, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float64)
    results = {}
    for n in args.rows:
        Xn, yn = X[:n], y[:n]

        def booster(objective):
            p = {"objective": objective, "num_leaves": args.num_leaves, "max_bin": 255, "device_type": "gpu",
                 "verbosity": -1, "boost_from_average": False}
            return lgb.Booster(p, lgb.Dataset(Xn, yn, params=p))

        def np_logistic(preds, ds):
            p = 1.0 / (1.0 + np.exp(-preds))
            return p - yn, p * (1.0 - p)

        y_dev = torch.from_numpy(yn).cuda()

        def torch_logistic(preds, ds):
            p = torch.sigmoid(preds)
            return p - y_dev, p * (1.0 - p)

        res = {}
        b = booster("none")
        res["update(fobj), numpy"] = batches(lambda: b.update(fobj=np_logistic))
        del b
        b = booster("none")
        res["update_device, torch"] = batches(lambda: b.update_device(torch_logistic))
        del b
        b = booster("binary")
        res["built-in binary"] = batches(lambda: b.update())
        del b, y_dev
        results[n] = res

    def its(m):
        return f"{1.0 / m['min']:.1f} / {1.0 / m['median']:.1f}"

    lines = [
        "# A custom objective on the host, on the GPU, and the built-in one (scripts/bench_custom_objective.py)",
        "",
        f"{args.note}".strip(),
        "",
        f"28 float32 features (make_higgs_like), max_bin=255, {args.num_leaves} leaves, device_type=gpu, logistic loss. "
        f"Iterations per second from the fastest / the median of {args.repeats} batches of {args.iters} iterations after "
        f"{args.warmup} warm-up iterations; a batch's clock stops after a device synchronisation. The last column is the "
        "median batch's milliseconds per iteration above the built-in objective's.",
        "",
        "| rows | path | it/s (best / median) | ms per iteration (median) | ms over built-in |",
        "|---:|---|---:|---:|---:|",
    ]
    for n in args.rows:
        base = results[n]["built-in binary"]["median"]
        for name, m in results[n].items():
            lines.append(f"| {n:,} | {name} | {its(m)} | {m['median'] * 1e3:.2f} | {(m['median'] - base) * 1e3:.2f} |")
    lines.append("")
    for n in args.rows:
        r = results[n]
        base, host, dev = (r[k]["median"] for k in ("built-in binary", "update(fobj), numpy", "update_device, torch"))
        removed = (host - dev) / (host - base) * 100.0 if host > base else float("nan")
        lines.append(f"- {n:,} rows: update(fobj) costs {host / base:.1f}x the built-in objective's iteration, "
                     f"update_device {dev / base:.2f}x; update_device removes {removed:.1f} % of what update(fobj) adds.")
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)


if __name__ == "__main__":
    main()
