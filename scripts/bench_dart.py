"""Times boosting=dart on the GPU: host-scored, device-scored per tree, device-scored by forest.

For each row count (make_higgs_like: 28 float32 features; objective=binary, 63 leaves,
device_type=gpu, default drop_rate=0.1) one booster per column trains 200 iterations:

  parent        boosting=dart with another build of the library (--parent-lib, the parent commit's)
  host          this library, LGAP_DEVICE_DART=0: score and objective on the host (should match parent)
  tree          the default: score on the device, one traversal per dropped tree
  forest        LGAP_DEVICE_DART=forest: score on the device, the dropped trees in one forest traversal
  gbdt          boosting=gbdt with this library, the ceiling

The clock covers iterations 100-200 (about 10 to 20 trees dropped in each) in `--repeats` equal
batches; a batch's clock stops after a device synchronisation. The report gives iterations per
second from the fastest and the median batch, and the mean number of trees dropped per iteration,
counted over 30 further, untimed iterations from the new tree's shrinkage (learning_rate / (1 + k)).

LGAP_DEVICE_DART is read once per process and the parent's library is another file, so every
column is a child process. Each runs under its own time limit, and the first one that fails or
runs out of time ends the script: nothing more is started on the GPU after it.

    python scripts/bench_dart.py --rows 1000000 10000000 --parent-lib /path/to/parent/lib_lambdagap.so \\
        --out profiles/dart_device.md
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

COLUMNS = {  # name -> (boosting, LGAP_DEVICE_DART, the parent's library)
    "parent": ("dart", None, True),
    "host": ("dart", "0", False),
    "tree": ("dart", None, False),
    "forest": ("dart", "forest", False),
    "gbdt": ("gbdt", None, False),
}


def worker(args):
    import lambdagap_amd as lgb
    from lambdagap_amd.basic import _LIB, _check
    from lambdagap_amd.utils import make_higgs_like

    if lgb.device_count() < 1:
        raise SystemExit("bench_dart: no gfx950 GPU visible")
    X, y = make_higgs_like(args.rows, seed=1)
    params = {"objective": "binary", "num_leaves": args.num_leaves, "boosting": args.boosting, "device_type": "gpu",
              "verbosity": -1, "learning_rate": 0.1}
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
    dropped = []
    if args.boosting == "dart":
        for _ in range(30):
            bst.update()
            it = bst.current_iteration() - 1
            text = bst.model_to_string(start_iteration=it, num_iteration=1)
            shrink = float([ln for ln in text.splitlines() if ln.startswith("shrinkage=")][-1].split("=")[1])
            dropped.append(params["learning_rate"] / shrink - 1.0)
    print("RESULT " + json.dumps({"best": max(rates), "median": statistics.median(rates),
                                  "dropped": statistics.mean(dropped) if dropped else 0.0,
                                  "device": bst.device_name()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--num-leaves", type=int, default=63)
    ap.add_argument("--start", type=int, default=100, help="first timed iteration")
    ap.add_argument("--stop", type=int, default=200, help="end of the timed iterations")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--columns", nargs="+", default=list(COLUMNS), choices=list(COLUMNS))
    ap.add_argument("--parent-lib", default=None, help="lib_lambdagap.so of the parent commit (column 'parent')")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds per column and row count")
    ap.add_argument("--note", default="", help="commits and machine, copied into the report")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--boosting", default="dart", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        args.rows = args.rows[0]
        return worker(args)

    lines = ["# boosting=dart on the GPU", ""]
    if args.note:
        lines += [args.note, ""]
    lines += [f"objective=binary, {args.num_leaves} leaves, drop_rate=0.1, 28 float32 features; iterations per second "
              f"over iterations {args.start}-{args.stop}, fastest / median of {args.repeats} batches.", "",
              "| rows | " + " | ".join(args.columns) + " | dropped trees / iteration |",
              "|---|" + "---|" * (len(args.columns) + 1)]
    for rows in args.rows:
        cells, dropped = [], 0.0
        for col in args.columns:
            boosting, mode, parent = COLUMNS[col]
            if parent and not args.parent_lib:
                cells.append("-")
                continue
            env = dict(os.environ)
            env.pop("LGAP_DEVICE_DART", None)
            env.pop("LAMBDAGAP_LIB", None)
            if mode is not None:
                env["LGAP_DEVICE_DART"] = mode
            if parent:
                env["LAMBDAGAP_LIB"] = args.parent_lib
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--rows", str(rows), "--boosting", boosting,
                   "--num-leaves", str(args.num_leaves), "--start", str(args.start), "--stop", str(args.stop),
                   "--repeats", str(args.repeats)]
            try:
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"bench_dart: column {col} at {rows} rows ran past {args.step_timeout} s; stopping")
            if r.returncode != 0:
                raise SystemExit(f"bench_dart: column {col} at {rows} rows ended with {r.returncode}; stopping\n"
                                 + (r.stdout + r.stderr)[-2000:])
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            cells.append(f"{res['best']:.1f} / {res['median']:.1f}")
            if col == "forest" or (boosting == "dart" and dropped == 0.0):
                dropped = res["dropped"]
            print(f"{rows} rows, {col}: {cells[-1]} it/s, {res['dropped']:.1f} dropped ({res['device']})", flush=True)
        lines.append(f"| {rows:,} | " + " | ".join(cells) + f" | {dropped:.1f} |")
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        with open(args.out, "w") as f:
            f.write(report)


if __name__ == "__main__":
    main()
