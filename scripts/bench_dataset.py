"""Times lgb.Dataset(...).construct() with device_type=gpu from host and from GPU-resident features.

The matrix has the headline shape (make_higgs_like: 28 float32 features). For each row count the
Dataset is constructed from a numpy array (sample on the host, upload in 256 MiB chunks, pack on
the device), from a contiguous float32 tensor on the GPU and from the transposed view of a
feature-major tensor (both sampled and packed where they lie). Each variant is warmed up once,
then timed `--repeats` times; the clock stops after a device synchronisation. With LGAP_TIMETAG=1
the phase timer's share of one construction is printed per variant.

    python scripts/bench_dataset.py --rows 1000000 10000000 --out profiles/dataset_from_device.md
    python scripts/bench_dataset.py --baseline-lib /path/to/parent/lib_lambdagap.so ...

--baseline-lib times the numpy variant again in a child process that loads another build of the
native library (the parent commit's), so the baseline comes from the same machine and the same
run rather than from the code under test.

torch is imported and creates its GPU context first: a torch wheel that bundles its own ROCm
runtime cannot see the device once the library's runtime has initialised it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("Dataset::Construct", "Dataset::GatherSample", "Device::GatherRows", "Device::PackRows",
          "Device::PackResident", "Device::CopyRowsToHost")


def phase_seconds(lgb):
    out = {}
    for line in lgb.phase_timer_report().splitlines():
        parts = line.split()
        if len(parts) >= 5 and parts[0] in PHASES:
            out[parts[0]] = float(parts[1])
    return out


def measure(lgb, torch, make_data, params, repeats):
    def once():
        ds = lgb.Dataset(make_data(), params=params).construct()
        torch.cuda.synchronize()
        return ds

    once()  # warm-up: code objects, allocations
    before = phase_seconds(lgb)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        once()
        ts.append(time.perf_counter() - t0)
    after = phase_seconds(lgb)
    phases = {k: (after[k] - before.get(k, 0.0)) / repeats for k in after if after[k] - before.get(k, 0.0) > 0}
    return {"min": min(ts), "median": statistics.median(ts), "phases": phases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inputs", nargs="+", default=["numpy", "tensor", "transposed"],
                    choices=["numpy", "tensor", "transposed"])
    ap.add_argument("--baseline-lib", default=None, help="another build of the native library for the numpy baseline")
    ap.add_argument("--json", action="store_true", help="print one JSON line instead of the report")
    ap.add_argument("--note", default="", help="commit and machine, copied into the report")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    baseline = None
    if args.baseline_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--json", "--inputs", "numpy", "--repeats", str(args.repeats),
               "--rows"] + [str(n) for n in args.rows]
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, LAMBDAGAP_LIB=args.baseline_lib))
        if r.returncode != 0:
            raise SystemExit("bench_dataset: the baseline run failed\n" + (r.stdout + r.stderr)[-2000:])
        baseline = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_dataset: torch sees no GPU")
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()

    import lambdagap_amd as lgb
    from lambdagap_amd.utils import make_higgs_like

    if lgb.device_count() < 1:
        raise SystemExit("bench_dataset: no gfx950 GPU visible")
    X, _ = make_higgs_like(max(args.rows), seed=11)
    X = np.ascontiguousarray(X, dtype=np.float32)
    params = {"max_bin": 255, "device_type": "gpu", "verbosity": -1}
    results = {}
    for n in args.rows:
        Xn = X[:n]
        res = {}
        if "numpy" in args.inputs:
            res["numpy"] = measure(lgb, torch, lambda: Xn, params, args.repeats)
        if "tensor" in args.inputs:
            t = torch.from_numpy(Xn).cuda()
            res["tensor"] = measure(lgb, torch, lambda: t, params, args.repeats)
            del t
        if "transposed" in args.inputs:
            fm = torch.from_numpy(Xn).cuda().T.contiguous()
            res["transposed"] = measure(lgb, torch, lambda: fm.T, params, args.repeats)
            del fm
        results[str(n)] = res
    if args.json:
        print(json.dumps(results), flush=True)
        return

    def cell(m):
        return "not measured" if m is None else f"{m['min']:.3f} / {m['median']:.3f}"

    lines = [
        "# lgb.Dataset(...).construct() from host and from GPU-resident features (scripts/bench_dataset.py)",
        "",
        f"{args.note}".strip(),
        "",
        f"28 float32 features (make_higgs_like), max_bin=255, device_type=gpu; wall seconds of one construct(), "
        f"min / median of {args.repeats} after one warm-up, the clock stopped after a device synchronisation. The "
        "baseline column is the numpy input on the parent commit's library, timed in the same run.",
        "",
        "| rows | numpy, parent commit | numpy | GPU tensor, contiguous | GPU tensor, transposed view |",
        "|---:|---:|---:|---:|---:|",
    ]
    for n in args.rows:
        res = results[str(n)]
        base = baseline[str(n)]["numpy"] if baseline else None
        lines.append(f"| {n:,} | {cell(base)} | {cell(res.get('numpy'))} | {cell(res.get('tensor'))} | "
                     f"{cell(res.get('transposed'))} |")
    if any(m["phases"] for res in results.values() for m in res.values()):
        lines += ["", "Phase timer, seconds per construct() (phases nest: Construct holds the others; FindBin and the "
                  "bundle plan are its remainder; PackRows / PackResident include the copy-back of the packed rows):", ""]
        for n in args.rows:
            for name, m in results[str(n)].items():
                ph = ", ".join(f"{k} {v:.3f}" for k, v in sorted(m["phases"].items()))
                lines.append(f"- {n:,} rows, {name}: {ph}")
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)


if __name__ == "__main__":
    main()
