#!/usr/bin/env python3
"""Benchmark: training cross-sections/sec (BASELINE.json headline metric).

Measures the flagship FactorVAE training step — forward + backward +
Adam + LR-scheduler per trading-day cross-section — on synthetic
Alpha158-shaped data (N=300 stocks, T=20, C=158 features, K=20 factors;
BASELINE.json config) with random-init weights.

Usage:
  python bench.py [--gpus N] [--steps K] [--warmup W] [--engine fused|eager]
                  [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times exactly K steps and prints one JSON
result line; `ms_per_step` is the wall time of one timed step.
--dump-outputs DIR additionally writes what the last timed step produced
(loss terms, reconstruction, and the trained parameters) as float32
DIR/<name>.npy; inputs and weights are seeded, so equal arguments give
comparable dumps across builds. --full is where measurements beyond the
headline figure belong; the benchmark has none today, so it changes
nothing yet.
Multi-GPU (driver contract): launched under torch.distributed.run with
one rank per GPU; ranks read RANK/LOCAL_RANK/WORLD_SIZE from the env.
Weak scaling: each rank trains its own shard of day cross-sections
(day-level DP, gradient all-reduced over RCCL each step), so the
whole-job aggregate is steps * N_gpus cross-sections.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

from factorvae_amd.models.modules import build_factorvae
from factorvae_amd.parallel.ddp import (
    FlatGradBucket,
    get_rank,
    get_world_size,
    init_distributed,
    is_distributed,
)
from factorvae_amd.utils import set_seed


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--engine", type=str, default="auto",
                   choices=["auto", "fused", "eager"])
    p.add_argument("--n_stocks", type=int, default=300)
    p.add_argument("--seq_len", type=int, default=20)
    p.add_argument("--num_latent", type=int, default=158)
    p.add_argument("--num_factor", type=int, default=20)
    p.add_argument("--hidden_size", type=int, default=64)
    p.add_argument("--num_portfolio", type=int, default=128)
    p.add_argument("--dtype", type=str, default="fp32",
                   choices=["fp32", "bf16", "fp8"])
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--n_days", type=int, default=32,
                   help="distinct synthetic day tensors cycled through")
    p.add_argument("--dump-outputs", dest="dump_outputs", type=str,
                   default=None, metavar="DIR",
                   help="after the timed steps, write the last step's "
                        "outputs and the trained parameters to DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run every measurement beyond the headline "
                        "figure (none today; a plain run stays lean)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be >= 1")
    if args.warmup < 0:
        p.error("--warmup must be >= 0")
    return args


def dump_outputs(out_dir, arrays):
    """Write each named tensor as float32 out_dir/<name>.npy. The dump
    stays under 64 MB in all: an array over its share is replaced by a
    fixed seeded sample of its elements (same indices every run)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    max_elems = (64 << 20) // 4 // len(arrays)
    for name, t in arrays.items():
        a = t.detach().to(torch.float32).cpu().numpy()
        if a.size > max_elems:
            idx = np.random.default_rng(0).choice(a.size, max_elems,
                                                  replace=False)
            a = a.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def main():
    args = parse_args()
    rank = init_distributed()
    world = get_world_size()
    set_seed(args.seed + rank)

    if torch.cuda.is_available():
        device = torch.device("cuda", torch.cuda.current_device())
    else:
        device = torch.device("cpu")

    N, T, C = args.n_stocks, args.seq_len, args.num_latent
    H, M, K = args.hidden_size, args.num_portfolio, args.num_factor

    model = build_factorvae(num_latent=C, hidden_size=H, num_portfolio=M,
                            num_factor=K).to(device)

    from factorvae_amd.engine.trainer import resolve_engine
    engine_name = resolve_engine(args.engine, H, device.type)

    # synthetic device-resident day tensors (weak scaling: each rank its own days)
    g = torch.Generator(device=device)
    g.manual_seed(args.seed * 1000 + rank)
    days = [(torch.randn(N, T, C, device=device, generator=g),
             torch.randn(N, 1, device=device, generator=g))
            for _ in range(args.n_days)]

    total_steps = args.warmup + args.steps

    if engine_name == "fused":
        from factorvae_amd.engine.fused import FusedTrainer
        trainer = FusedTrainer(model, lr=args.lr, t_max=total_steps,
                               device=device, dtype=args.dtype)
        # multi-step graph: capture G = gcd-ish steps per replay so the
        # timed region is exactly `steps` cross-sections
        G = 1
        for d in range(min(args.n_days, args.steps), 0, -1):
            if args.steps % d == 0 and args.warmup % d == 0:
                G = d
                break
        if is_distributed() or os.environ.get("FV_PRINT_CAPS") == "1":
            rng_ok, comm_ok = trainer._probe_caps()
            print(f"[bench rank {rank}] probe_caps: rng_in_graph={rng_ok} "
                  f"comm_in_graph={comm_ok} world={world} "
                  f"backend={torch.distributed.get_backend() if is_distributed() else 'none'}",
                  file=sys.stderr, flush=True)
        runner, _ = trainer.make_bench_runner(days[:G])

        class _Multi:
            pass

        multi = _Multi()
        multi.runner, multi.G = runner, G
        step_fn = None
    else:
        multi = None
        bucket = FlatGradBucket(model.parameters()) if is_distributed() else None
        opt = torch.optim.Adam(model.parameters(), lr=args.lr)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=total_steps)
        model.train()

        def step_fn(x, y):
            if bucket is not None:
                bucket.zero_()
            else:
                opt.zero_grad(set_to_none=True)
            loss, *_ = model(x, y)
            loss.backward()
            if bucket is not None:
                bucket.all_reduce_()
            opt.step()
            sched.step()
            return loss

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    def barrier():
        if is_distributed():
            torch.distributed.barrier()

    # warmup
    if multi is not None:
        for _ in range(max(1, args.warmup // multi.G)):
            multi.runner()
    else:
        for i in range(args.warmup):
            step_fn(*days[i % len(days)])
    barrier()
    sync()

    t0 = time.perf_counter()
    if multi is not None:
        for _ in range(args.steps // multi.G):
            multi.runner()
    else:
        for i in range(args.steps):
            last_loss = step_fn(*days[(args.warmup + i) % len(days)])
    barrier()
    sync()
    t1 = time.perf_counter()

    elapsed = t1 - t0
    # max over ranks (report the slowest rank's wall time)
    if is_distributed():
        t = torch.tensor([elapsed], device=device if device.type == "cuda" else None,
                         dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    ms_per_step = elapsed / args.steps * 1000.0
    # whole-job aggregate: each rank processes one cross-section per step
    value = args.steps * world / elapsed
    # The reference publishes NO training throughput; its only speed
    # datum is 6.54 cross-sections/s *inference* (eager, unnamed CUDA
    # GPU, backtest.ipynb cell 4). vs_baseline divides our TRAINING
    # rate by that inference datum — see baseline_note in the output.
    baseline = 6.54
    result = {
        "metric": "training cross-sections/sec",
        "value": value,
        "unit": "cross-sections/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": value / baseline,
        "baseline_note": ("reference publishes no training throughput; "
                          "6.54 cs/s is its eager INFERENCE rate on an "
                          "unnamed CUDA GPU (backtest.ipynb cell 4) — "
                          "vs_baseline is training-vs-inference, not "
                          "like-for-like"),
        # effective compute dtype: the eager oracle path always runs fp32
        "dtype": args.dtype if engine_name == "fused" else "fp32",
        "data": "synthetic",
        "config": {
            "model": "FactorVAE",
            "global_batch": N * world,
            "seq_len": T,
            "parallelism": f"dp{world}",
            "n_stocks": N,
            "num_latent": C,
            "num_factor": K,
            "hidden_size": H,
            "num_portfolio": M,
            "engine": engine_name,
        },
    }
    if rank == 0 and args.dump_outputs:
        # what the last timed step computed, plus the weights all timed
        # steps trained (about 1 MB at the benchmark shapes)
        with torch.no_grad():
            arrays = {"params": torch.cat([p.reshape(-1)
                                           for p in model.parameters()])}
            if multi is not None:
                w = trainer.ws
                arrays.update(loss=w["loss"], mse=w["mse"], kl=w["kl"],
                              recon=w["recon"])
            else:
                arrays["loss"] = last_loss.reshape(1)
            dump_outputs(args.dump_outputs, arrays)
    if rank == 0:
        print(json.dumps(result))
    if is_distributed():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
