"""Times repeated prediction of one trained model on one MI355X: Booster.predict_device per call
against a resident Booster.device_predictor, and the predictor's two kernel families against
each other. The table decides the default of tree_parallel_rows.

The model has the headline shape: 28 float32 features, 63 leaves, 100 trees, binary objective;
raw scores. Variants, per row count and for numpy in / numpy out and GPU tensor in / out:

  a  predict_device of the parent commit's library (--parent-lib), the baseline
  b  predict_device of this library
  c  device_predictor(tree_parallel_rows=0): the row-parallel kernels
  d  device_predictor(tree_parallel_rows=65536): the tree-parallel kernels, up to 65,536 rows
  e  Booster.predict on the host's OpenMP threads (numpy only), for scale

Every timed call ends in a device synchronisation (the library synchronises its stream before it
returns; the tensor variants also synchronise torch's stream inside the timed span). Per variant
and shape: 20 warm-up calls, then the fastest and the median of 200 calls (fewer at 1,000,000
rows). One repeat is one fresh process per library, the parent's and this one in turn; the
default is three repeats. Results are checked equal to Booster.predict before they are timed.

    python scripts/bench_predictor.py --parent-lib variants/lib_parent.so --out profiles/device_predictor.md

torch is imported and creates its GPU context first: a torch wheel that bundles its own ROCm
runtime cannot see the device once the library's runtime has initialised it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = [1, 16, 256, 1024, 4096, 16384, 65536, 1_000_000]
MAX_TREE_PARALLEL_ROWS = 65536
INPUTS = ("numpy", "tensor")


def calls_for(n, calls):
    """(warm-up calls, timed calls): fewer for the one shape that takes milliseconds per call."""
    return (3, max(10, calls // 10)) if n > MAX_TREE_PARALLEL_ROWS else (20, calls)


def timed(fn, warm, calls):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), statistics.median(ts)


def worker(args):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_predictor: torch sees no GPU")
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    import lambdagap_amd as lgb
    from lambdagap_amd.utils import make_higgs_like

    if lgb.device_count() < 1:
        raise SystemExit("bench_predictor: no gfx950 GPU visible")
    booster = lgb.Booster(model_file=args.model)
    X, _ = make_higgs_like(max(args.rows), seed=11)
    X = np.ascontiguousarray(X, dtype=np.float32)
    variants = args.worker.split(",")
    preds = {}
    if "c" in variants:
        preds["c"] = booster.device_predictor(tree_parallel_rows=0)
    if "d" in variants:
        preds["d"] = booster.device_predictor(tree_parallel_rows=MAX_TREE_PARALLEL_ROWS)
    for n in args.rows:
        Xn = X[:n]
        t = torch.from_numpy(Xn).cuda()
        torch.cuda.synchronize()
        ref = booster.predict(Xn, raw_score=True)
        warm, calls = calls_for(n, args.calls)
        for v in variants:
            if v == "d" and n > MAX_TREE_PARALLEL_ROWS:
                continue
            for inp in INPUTS:
                if v == "e":
                    if inp == "tensor":
                        continue
                    fn = lambda: booster.predict(Xn, raw_score=True)  # noqa: E731
                elif v in ("a", "b"):
                    fn = (lambda: booster.predict_device(Xn, raw_score=True)) if inp == "numpy" else \
                        (lambda: (booster.predict_device(t, raw_score=True), torch.cuda.synchronize())[0])
                else:
                    p = preds[v]
                    fn = (lambda: p.predict(Xn, raw_score=True)) if inp == "numpy" else \
                        (lambda: (p.predict(t, raw_score=True), torch.cuda.synchronize())[0])
                got = fn()
                got = got.cpu().numpy() if inp == "tensor" else got
                equal = bool(np.array_equal(ref, got))
                if v in preds:
                    assert preds[v].last_path == ("row" if v == "c" else "tree")
                w, c = (warm, calls) if v != "e" else (2, max(5, calls // (20 if n >= 16384 else 4)))
                lo, med = timed(fn, w, c)
                print("TIMING " + json.dumps({"variant": v, "input": inp, "rows": n, "min": lo, "median": med,
                                              "calls": c, "equal": equal}), flush=True)
        del t


def run_worker(args, model, variants, lib):
    env = dict(os.environ)
    env.pop("LAMBDAGAP_LIB", None)
    if lib:
        env["LAMBDAGAP_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", variants, "--model", model, "--calls",
           str(args.calls), "--rows"] + [str(n) for n in args.rows]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise SystemExit(f"bench_predictor: worker {variants} failed\n{(r.stdout + r.stderr)[-3000:]}")
    return [json.loads(ln[len("TIMING "):]) for ln in r.stdout.splitlines() if ln.startswith("TIMING ")]


def fmt(sec):
    return f"{sec * 1e6:,.0f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=ROWS)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--train-rows", type=int, default=500_000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's library: variant a")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--model", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    import lambdagap_amd as lgb
    from lambdagap_amd.utils import make_higgs_like

    if lgb.device_count() < 1:
        raise SystemExit("bench_predictor: no gfx950 GPU visible")
    X, y = make_higgs_like(args.train_rows, seed=11)
    params = {"objective": "binary", "num_leaves": 63, "learning_rate": 0.1, "max_bin": 255, "device_type": "gpu",
              "verbosity": -1}
    booster = lgb.train(params, lgb.Dataset(X, y, params=params), num_boost_round=args.trees)
    tmp = tempfile.mkdtemp(prefix="bench_predictor_")
    model = os.path.join(tmp, "model.txt")
    booster.save_model(model)
    ntrees = booster.num_trees()
    del booster, X, y

    # results[(variant, input, rows)] -> one (min, median) per repeat
    results, all_equal = {}, True
    for rep in range(args.repeats):
        runs = []
        if args.parent_lib:
            runs += run_worker(args, model, "a", args.parent_lib)
        runs += run_worker(args, model, "b,c,d,e", None)
        for r in runs:
            results.setdefault((r["variant"], r["input"], r["rows"]), []).append((r["min"], r["median"]))
            all_equal = all_equal and r["equal"]
        print(f"repeat {rep + 1} of {args.repeats} done", flush=True)

    def cell(v, inp, n):
        got = results.get((v, inp, n))
        if not got:
            return "not measured"
        meds = [m for _, m in got]
        return f"{fmt(min(lo for lo, _ in got))} / {fmt(statistics.median(meds))} ({fmt(max(meds) - min(meds))})"

    def wins(inp, n):
        c, d = results.get(("c", inp, n)), results.get(("d", inp, n))
        if not c or not d:
            return False
        mc, md = [m for _, m in c], [m for _, m in d]
        spread = max(max(mc) - min(mc), max(md) - min(md))
        return statistics.median(mc) - statistics.median(md) > spread

    lines = [
        "# Booster.device_predictor on one MI355X (scripts/bench_predictor.py)",
        "",
        f"Model: binary, 28 float32 features, 63 leaves, {ntrees} trees; raw scores. Wall time per call in "
        "microseconds, the clock stopped after a device synchronisation: fastest call / median call (spread of the "
        f"repeats' medians). {args.repeats} repeats, each a fresh process per library, the parent's and this one in "
        f"turn; per repeat 20 warm-up calls and {args.calls} timed calls per variant and shape "
        f"({calls_for(max(args.rows), args.calls)[1]} above 65,536 rows; the host loop fewer), the fastest taken over "
        "all repeats, the median that of the repeats' medians. No hardware counters were taken.",
        "",
        "a: predict_device, parent commit. b: predict_device, this commit. c: device_predictor, "
        "tree_parallel_rows=0 (row-parallel kernels). d: device_predictor, tree_parallel_rows=65536 (tree-parallel "
        f"kernels). e: Booster.predict on {os.environ.get('OMP_NUM_THREADS', 'all')} host threads.",
        "",
    ]
    for inp, title in (("numpy", "numpy in / numpy out"), ("tensor", "GPU tensor in / GPU tensor out")):
        lines += [f"## {title}", "", "| rows | a | b | c | d | e | d below c by more than the spread |",
                  "|---:|---:|---:|---:|---:|---:|---|"]
        for n in args.rows:
            verdict = "-" if n > MAX_TREE_PARALLEL_ROWS else ("yes" if wins(inp, n) else "no")
            lines.append(f"| {n:,} | " + " | ".join(cell(v, inp, n) for v in "abcde") + f" | {verdict} |")
        lines.append("")
    both = [n for n in args.rows if n <= MAX_TREE_PARALLEL_ROWS and all(wins(inp, n) for inp in INPUTS)]
    default = max(both) if both else 0
    lines += [
        "## The default of tree_parallel_rows",
        "",
        "The rule: the largest row count of the grid at which d's median is below c's by more than the spread of "
        "the repeats' medians (the larger of c's and d's), for numpy and for tensor input alike; 0 if there is none.",
        "",
        f"By this table: **{default}**" + (" (row counts that qualify: " + ", ".join(f"{n:,}" for n in both) + ")."
                                          if both else " (no row count qualifies)."),
        "",
        f"All timed variants returned Booster.predict's raw scores bit for bit: {'yes' if all_equal else 'NO'}.",
        "",
    ]
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)


if __name__ == "__main__":
    main()
