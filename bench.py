#!/usr/bin/env python3
"""Headline benchmark: boosting iterations/sec + AUC on synthetic Higgs-shape
10M x 28 binary data, 255 bins, 63 leaves (BASELINE.json), HIP learner on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

N>1 runs under torchrun, one process per GPU: the 10M training rows are split
evenly across ranks (strong scaling: the job always trains on the same 10M x 28
dataset) and every tree is grown data-parallel with the smaller child's
histogram all-reduced over RCCL. A "step" is one full boosting iteration
(gradients, tree growth, score update). W untimed iterations, then exactly K
timed iterations between barrier + device synchronisation on both sides; the
max over ranks is reported. A plain run does only that: set up, warm up, time the K
steps, print the result line. `--dump-outputs DIR` also writes what the last timed step left
behind (see _dump_outputs); `--full` adds the checks that take work of their own, today the
AUC of the trained model on a held-out set (null in the result line of a plain run).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# Published like-for-like numbers exist only for num_leaves=255: Higgs 500
# iterations, 255 bins, lr 0.1, min_sum_hessian_in_leaf=100 -> GTX 1080 OpenCL 4.31 it/s
# (docs/GPU-Performance.rst:99). The BASELINE.json driver config (63 leaves) has no published
# number, so vs_baseline is null there; `--num-leaves 255` reports the comparison.
BASELINE_IT_S = {255: 4.31}
METRIC = "boosting iters/sec + AUC, synthetic Higgs-shape 10M×28, 255 bins, 63 leaves"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--valid-rows", type=int, default=500_000)
    ap.add_argument("--num-leaves", type=int, default=63)
    ap.add_argument("--max-bin", type=int, default=255)
    ap.add_argument("--device", default="gpu")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--graph", type=int, default=None, help="device_use_graph override (1/0)")
    ap.add_argument("--use-dp", action="store_true", help="gpu_use_dp=true: fp64 histogram accumulation")
    ap.add_argument("--quantized", action="store_true",
                    help="use_quantized_grad=true (4 gradient levels, integer histograms); a secondary line")
    ap.add_argument("--rehearse-dp", action="store_true",
                    help="1 GPU: run the RCCL data-parallel learner path on a one-rank communicator")
    ap.add_argument("--dp-host-transport", action="store_true",
                    help="N>1 ranks sharing one GPU: stage the data-parallel collectives through host "
                         "memory over gloo (multi-rank rehearsal; not a performance configuration)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the trained model's outputs to DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the checks beyond the headline figure: AUC on a held-out set")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world == 1 and args.gpus > 1 and "RANK" not in os.environ:
        # `python bench.py --gpus N` outside torchrun: launch the N rank processes here, before
        # this process touches the GPU, and relay their output (rank 0 prints the JSON line)
        return _spawn_ranks(args.gpus)
    if world != args.gpus:
        print(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus}", file=sys.stderr)
        return 2

    import lambdagap_amd as lgb
    from lambdagap_amd.parallel import device_synchronize, init_device_comm, shard_range
    from lambdagap_amd.utils import make_higgs_like

    dist = None
    if world > 1 and args.device == "cpu":
        # host learners: data-parallel over the torch (gloo) collectives
        import torch.distributed as dist  # noqa: F811

        from lambdagap_amd.parallel.torch_network import init_torch_network

        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        init_torch_network()
    elif world > 1 and args.dp_host_transport:
        import torch.distributed as dist  # noqa: F811

        from lambdagap_amd.parallel.torch_network import init_torch_network

        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        init_torch_network()
        os.environ["LGAP_DEVICE_DP_TRANSPORT"] = "host"
    elif world > 1:
        import torch.distributed as dist  # noqa: F811

        init_device_comm()
    elif args.rehearse_dp:
        import ctypes

        from lambdagap_amd.parallel import distributed as dd

        uid = dd.get_unique_id()
        dd._check(dd._LIB.LGBM_DeviceCommInit(dd._c_str(uid), ctypes.c_int64(len(uid)), ctypes.c_int(1),
                                              ctypes.c_int(0), ctypes.c_int(0)))
        os.environ["LGAP_FORCE_DEVICE_DP"] = "1"
    t_data = time.time()
    start, stop = shard_range(args.rows, rank, world)
    X, y = make_higgs_like(args.rows, seed=args.seed, start=start, stop=stop)
    params = {
        "objective": "binary",
        "num_leaves": args.num_leaves,
        "max_bin": args.max_bin,
        "learning_rate": 0.1,
        "min_data_in_leaf": 1,
        "min_sum_hessian_in_leaf": 100,
        "device_type": args.device,
        "verbosity": -1,
        "seed": args.seed,
    }
    if world > 1:
        params.update({"tree_learner": "data", "num_machines": world, "pre_partition": True})
    if args.use_dp:
        params["gpu_use_dp"] = True
    if args.quantized:
        params["use_quantized_grad"] = True
        params["num_grad_quant_bins"] = 4
    if args.graph is not None:
        params["device_use_graph"] = bool(args.graph)
    train_set = lgb.Dataset(X, y, params=params, free_raw_data=True)
    booster = lgb.Booster(params=params, train_set=train_set)
    del X
    t_data = time.time() - t_data

    def barrier_sync():
        device_synchronize()
        if dist is not None:
            dist.barrier()

    for _ in range(args.warmup):
        booster.update()
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        booster.update()
    barrier_sync()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        import torch

        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank == 0 and args.dump_outputs:
        _dump_outputs(booster, args)
    auc = None
    if rank == 0 and args.full:
        Xv, yv = make_higgs_like(args.valid_rows, seed=args.seed + 1000)
        pred = booster.predict(Xv)
        auc = _auc(yv, pred)
    if rank == 0:
        it_s = args.steps / elapsed
        out = {
            "metric": METRIC.replace("63 leaves", f"{args.num_leaves} leaves"),
            "value": round(it_s, 4),
            "unit": "iters/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1000.0 * elapsed / args.steps, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": (round(it_s / BASELINE_IT_S[args.num_leaves], 3)
                            if args.num_leaves in BASELINE_IT_S and args.max_bin == 255 else None),
            "dtype": "fp32",  # fp32 (g, h); fixed-point histogram sums (gpu_use_dp: fp64)
            "data": "synthetic",
            "auc": round(auc, 6) if auc is not None else None,
            "config": {
                "model": f"gbdt binary, {args.num_leaves} leaves, {args.max_bin} bins, lr 0.1"
                         + (", gpu_use_dp" if args.use_dp else "")
                         + (", use_quantized_grad (4 levels)" if args.quantized else ""),
                "global_batch": args.rows,
                "seq_len": 28,
                "parallelism": f"dp{world}",
                "device": booster.device_name(),
                "setup_s": round(t_data, 2),
                "transport": _transport(booster.device_name(), args) if world > 1 else None,
            },
        }
        print(json.dumps(out), flush=True)
    if dist is not None:
        # orderly teardown: the device learner, then the native collectives, then the process
        # group (left to static destructors, gloo's threads can abort the exiting process)
        dist.barrier()
        del booster, train_set
        if args.dp_host_transport or args.device == "cpu":
            from lambdagap_amd.parallel.torch_network import free_torch_network

            free_torch_network()
        else:
            from lambdagap_amd.parallel.distributed import free_device_comm

            free_device_comm()
        dist.barrier()
        dist.destroy_process_group()
    return 0


def _dump_outputs(booster, args, sample_rows: int = 200_000) -> None:
    """What the timed path computed, as a caller of Booster.update() receives it: the model after
    the last timed step. Written as the raw scores (float64) of the first `sample_rows` training
    rows, which are regenerated from the seed and so identical from run to run, under the whole
    model and under the trees of the last timed step alone. 2 x 1.6 MB at the default sizes."""
    from lambdagap_amd.utils import make_higgs_like

    os.makedirs(args.dump_outputs, exist_ok=True)
    Xs, _ = make_higgs_like(args.rows, seed=args.seed, start=0, stop=min(args.rows, sample_rows))
    it = booster.current_iteration()
    outputs = {"raw_score": booster.predict(Xs, raw_score=True)}
    if it > 0:
        outputs["last_step_raw_score"] = booster.predict(Xs, start_iteration=it - 1, num_iteration=1, raw_score=True)
    for name, a in outputs.items():
        np.save(os.path.join(args.dump_outputs, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def _spawn_ranks(n: int) -> int:
    """Run this benchmark as N ranks under torch.distributed.run (one process per GPU)."""
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    return subprocess.run(cmd, env=env).returncode


def _transport(device_name: str, args) -> str:
    """The exchange the learner actually selected (from its device_name())."""
    if args.device == "cpu":
        return "gloo (host collectives)"
    if "xGMI" in device_name:
        return "xgmi (in-kernel IPC exchange)"
    if "host-staged" in device_name or args.dp_host_transport:
        return "host-staged (rehearsal)"
    if "owner reduce-scatter" in device_name:
        return "rccl reduce-scatter by feature owner + best-split all-gather"
    if "all-reduce" in device_name:
        return "rccl all-reduce"
    return "rccl"


def _auc(y: np.ndarray, p: np.ndarray) -> float:
    order = np.argsort(p, kind="mergesort")
    ps = p[order]
    ys = y[order]
    # average ranks for ties
    ranks = np.empty(len(p), dtype=np.float64)
    i = 0
    n = len(p)
    idx = np.flatnonzero(np.diff(ps)) + 1
    bounds = np.concatenate([[0], idx, [n]])
    for a, b in zip(bounds[:-1], bounds[1:]):
        ranks[a:b] = (a + b + 1) / 2.0
    npos = ys.sum()
    nneg = n - npos
    return float((ranks[ys > 0].sum() - npos * (npos + 1) / 2.0) / (npos * nneg))


if __name__ == "__main__":
    sys.exit(main())
