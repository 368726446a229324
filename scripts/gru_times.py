"""GRU recurrence kernel times at H = 64: the fp32 kernels by variant (0 = f32
MFMA, 1 = wave per stock where the router allows it) beside the bf16 MFMA
kernels. Above ext.gru_wave_max_n() variant 1 IS the MFMA kernel, so the two
columns agree there by construction; to measure the wave kernels past the
cut-over, build gru_wave.hip with a larger -DGW_MAX_N.

    python scripts/gru_times.py [--shapes 300x20,1000x20,...] [--reps 5]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from factorvae_amd.ops import get_extension

ext = get_extension()
dev = torch.device("cuda:0")


def timeit(fn, iters=50):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def med(fn, reps):
    xs = sorted(timeit(fn) for _ in range(reps))
    return statistics.median(xs), xs[0], xs[-1]


def fmt(m):
    return f"{m[0]:7.1f} ({m[1]:.1f}-{m[2]:.1f})"


ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="300x20,300x60,1000x20,1000x60,"
                                    "3500x20,3500x60")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
print(f"gru_wave_max_n = {ext.gru_wave_max_n()}; us per launch, back-to-back "
      f"launches, median (min-max) of {args.reps} x 50", flush=True)
for shape in args.shapes.split(","):
    N, T = (int(v) for v in shape.split("x"))
    H = 64
    gi = torch.randn(N, T, 3 * H, device=dev)
    whh = torch.randn(3 * H, H, device=dev) * 0.1
    whh_bf = whh.to(torch.bfloat16)
    bhh = torch.randn(3 * H, device=dev) * 0.1
    hf = torch.empty(N, H, device=dev)
    hp = torch.empty(N, T, H, device=dev)
    g4 = torch.empty(N, T, 4 * H, device=dev)
    dh = torch.randn(N, H, device=dev)
    dgi = torch.empty(N, T, 3 * H, device=dev)
    dgh = torch.empty(N, T, 3 * H, device=dev)
    dgib = torch.empty(N, T, 3 * H, device=dev, dtype=torch.bfloat16)
    dghb = torch.empty_like(dgib)
    row = [f"N={N} T={T}:"]
    for v in (0, 1):
        f = med(lambda: ext.gru_fwd(gi, whh, bhh, hf, None, hp, g4, N, T, H,
                                    variant=v), args.reps)
        i = med(lambda: ext.gru_fwd_infer(gi, whh, bhh, hf, N, T, H,
                                          variant=v), args.reps)
        b = med(lambda: ext.gru_bwd(dh, hp, g4, whh, dgi, dgh, N, T, H,
                                    variant=v), args.reps)
        row.append(f"f32 v{v} fwd {fmt(f)} infer {fmt(i)} bwd {fmt(b)} |")
    f = med(lambda: ext.gru_fwd_mfma(gi, whh_bf, bhh, hf, None, hp, g4, N, T,
                                     H), args.reps)
    b = med(lambda: ext.gru_bwd_mfma(dh, hp, g4, whh_bf, dgi, dgh, N, T, H,
                                     dgib, dghb), args.reps)
    row.append(f"bf16 fwd {fmt(f)} bwd {fmt(b)}")
    print(" ".join(row), flush=True)
