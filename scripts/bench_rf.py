"""Times boosting=rf on the GPU: averaged scores on the host and on the device.

For each row count (make_higgs_like: 28 float32 features; objective=binary, 63 leaves,
device_type=gpu, bagging_freq=1, bagging_fraction=0.632, feature_fraction=0.8) one booster per
column trains `--stop` iterations:

  parent        boosting=rf with another build of the library (--parent-lib, the parent commit's)
  host          this library, LGAP_DEVICE_RF=0: gradients uploaded per tree, the scores averaged on
                the host (should match parent)
  device        the default: gradients uploaded once, the scores averaged by the blend kernels
  gbdt          boosting=gbdt with this library and the same sampling, the ceiling

The clock covers iterations `--start` to `--stop` in `--repeats` equal batches; a batch's clock
stops after a device synchronisation. The report gives iterations per second from the fastest and
the median batch. An RF iteration costs the same at every iteration (no score feeds back into the
gradients), so a short run measures it.

LGAP_DEVICE_RF is read once per process and the parent's library is another file, so every column
is a child process. Each runs under its own time limit, and the first one that fails or runs out
of time ends the script: nothing more is started on the GPU after it.

    python scripts/bench_rf.py --rows 1000000 10000000 --parent-lib /path/to/parent/lib_lambdagap.so \\
        --out profiles/rf_device.md
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLUMNS = {  # name -> (boosting, LGAP_DEVICE_RF, the parent's library)
    "parent": ("rf", None, True),
    "host": ("rf", "0", False),
    "device": ("rf", None, False),
    "gbdt": ("gbdt", None, False),
}


def worker(args):
    import lambdagap_amd as lgb
    from lambdagap_amd.basic import _LIB, _check
    from lambdagap_amd.utils import make_higgs_like

    if lgb.device_count() < 1:
        raise SystemExit("bench_rf: no gfx950 GPU visible")
    X, y = make_higgs_like(args.rows, seed=1)
    params = {"objective": "binary", "num_leaves": args.num_leaves, "boosting": args.boosting, "device_type": "gpu",
              "verbosity": -1, "learning_rate": 0.1, "bagging_freq": 1, "bagging_fraction": 0.632,
              "feature_fraction": 0.8}
    bst = lgb.Booster(params, lgb.Dataset(X, y, params=params))
    del X

    def sync():
        _check(_LIB.LGBM_DeviceSynchronize())

    for _ in range(args.start):
        bst.update()
    sync()
    per = (args.stop - args.start) // args.repeats
    rates = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(per):
            bst.update()
        sync()
        rates.append(per / (time.perf_counter() - t0))
    print("RESULT " + json.dumps({"best": max(rates), "median": statistics.median(rates), "device": bst.device_name()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--num-leaves", type=int, default=63)
    ap.add_argument("--start", type=int, default=10, help="first timed iteration")
    ap.add_argument("--stop", type=int, default=70, help="end of the timed iterations")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--columns", nargs="+", default=list(COLUMNS), choices=list(COLUMNS))
    ap.add_argument("--parent-lib", default=None, help="lib_lambdagap.so of the parent commit (column 'parent')")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds per column and row count")
    ap.add_argument("--note", default="", help="commits and machine, copied into the report")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--boosting", default="rf", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        args.rows = args.rows[0]
        return worker(args)

    lines = ["# boosting=rf on the GPU", ""]
    if args.note:
        lines += [args.note, ""]
    lines += [f"objective=binary, {args.num_leaves} leaves, bagging_freq=1, bagging_fraction=0.632, feature_fraction=0.8, "
              f"28 float32 features; iterations per second over iterations {args.start}-{args.stop}, fastest / median "
              f"of {args.repeats} batches.", "",
              "| rows | " + " | ".join(args.columns) + " |",
              "|---|" + "---|" * len(args.columns)]

    def report():
        text = "\n".join(lines) + "\n"
        if args.out:
            with open(args.out, "w") as f:
                f.write(text)
        return text

    for rows in args.rows:
        cells = []
        for col in args.columns:
            boosting, mode, parent = COLUMNS[col]
            if parent and not args.parent_lib:
                cells.append("-")
                continue
            env = dict(os.environ)
            env.pop("LGAP_DEVICE_RF", None)
            env.pop("LAMBDAGAP_LIB", None)
            if mode is not None:
                env["LGAP_DEVICE_RF"] = mode
            if parent:
                env["LAMBDAGAP_LIB"] = args.parent_lib
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--rows", str(rows), "--boosting", boosting,
                   "--num-leaves", str(args.num_leaves), "--start", str(args.start), "--stop", str(args.stop),
                   "--repeats", str(args.repeats)]
            try:
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"bench_rf: column {col} at {rows} rows ran past {args.step_timeout} s; stopping")
            if r.returncode != 0:
                raise SystemExit(f"bench_rf: column {col} at {rows} rows ended with {r.returncode}; stopping\n"
                                 + (r.stdout + r.stderr)[-2000:])
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            cells.append(f"{res['best']:.1f} / {res['median']:.1f}")
            print(f"{rows} rows, {col}: {cells[-1]} it/s ({res['device']})", flush=True)
        lines.append(f"| {rows:,} | " + " | ".join(cells) + " |")
        report()  # (after every row count: a later time limit keeps what was measured)
    print(report())


if __name__ == "__main__":
    main()
