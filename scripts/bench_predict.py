"""Scoring throughput: per-day FusedTrainer.predict against the batched
FusedTrainer.predict_many, same model and data, one process.

Per-day path = what generate_prediction_scores does for every loader day:
predict(x) (one hipGraph replay) and the scores brought to the host.
Batched path = predict_many over all D days (packed chunks, one
device-to-host copy per chunk). Inputs are device resident for both.

Method: every shape is warmed up first; then `--windows` timed windows per
path, alternating between the two paths, each window long enough
(`--min-seconds`) to be far above timer and scheduler noise and closed by
a device synchronise. Reported per path: median days/s and the min..max
spread over the windows; the ratio is median over median.

Configs: CSI300 shape (N=300, T=20, C=158, H=64, K=20, D in 8/64/256) and
A-share shape (N=3500, T=60, C=158, H=64, K=96, D=8).

  python scripts/bench_predict.py [--configs csi300,ashare] [--dtype fp32]
      [--per-day-only] [--out results.jsonl]

--per-day-only measures only predict (also what happens on a tree that
has no predict_many), for a baseline from another checkout:
  PYTHONPATH=/path/to/other/checkout python scripts/bench_predict.py \
      --per-day-only --no-repo-path
"""
import argparse
import json
import os
import statistics
import sys
import time

CONFIGS = {
    "csi300": dict(N=300, T=20, C=158, H=64, M=128, K=20, D=(8, 64, 256)),
    "ashare": dict(N=3500, T=60, C=158, H=64, M=128, K=96, D=(8,)),
}


def timed_windows(fn, days_per_call, windows, min_seconds, sync):
    """days/s of `windows` windows of repeated fn() calls."""
    fn()
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = max(1, int(min_seconds / one + 0.999))
    rates = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        rates.append(reps * days_per_call / (time.perf_counter() - t0))
    return rates


def summarize(rates):
    return {"median": statistics.median(rates), "min": min(rates),
            "max": max(rates), "windows": len(rates)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", type=str, default="csi300,ashare")
    p.add_argument("--dtype", type=str, default="fp32",
                   choices=["fp32", "bf16"])
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--min-seconds", type=float, default=0.5)
    p.add_argument("--per-day-only", action="store_true")
    p.add_argument("--no-repo-path", action="store_true",
                   help="import factorvae_amd from PYTHONPATH, not from "
                        "this script's checkout")
    p.add_argument("--label", type=str, default="")
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args()

    if not args.no_repo_path:
        sys.path.insert(0, os.path.dirname(os.path.dirname(
            os.path.abspath(__file__))))
    import torch

    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    if not torch.cuda.is_available():
        raise SystemExit("bench_predict.py needs a GPU: no timing without one")
    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)
    lines = []
    for name in args.configs.split(","):
        cfg = CONFIGS[name]
        N, T, C = cfg["N"], cfg["T"], cfg["C"]
        set_seed(0)
        model = build_factorvae(num_latent=C, hidden_size=cfg["H"],
                                num_portfolio=cfg["M"],
                                num_factor=cfg["K"]).to(dev)
        tr = FusedTrainer(model, lr=0.0, t_max=1, device=dev, train=False,
                          dtype=args.dtype)
        batched = hasattr(tr, "predict_many") and not args.per_day_only
        for D in cfg["D"]:
            g = torch.Generator().manual_seed(D)
            xs = [torch.randn(N, T, C, generator=g).to(dev)
                  for _ in range(D)]

            def per_day():
                for x in xs:
                    tr.predict(x).cpu()

            def many():
                tr.predict_many(xs)

            rates = {"per_day": [], "predict_many": []}
            # alternate the two paths window by window
            for _ in range(args.windows):
                rates["per_day"] += timed_windows(per_day, D, 1,
                                                  args.min_seconds, sync)
                if batched:
                    rates["predict_many"] += timed_windows(
                        many, D, 1, args.min_seconds, sync)
            rec = {"config": name, "label": args.label, "dtype": args.dtype,
                   "N": N, "T": T, "C": C, "H": cfg["H"], "K": cfg["K"],
                   "D": D,
                   "per_day_days_per_s": summarize(rates["per_day"])}
            if batched:
                rec["predict_many_days_per_s"] = summarize(
                    rates["predict_many"])
                rec["ratio"] = (rec["predict_many_days_per_s"]["median"]
                                / rec["per_day_days_per_s"]["median"])
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del xs
        del tr, model
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
