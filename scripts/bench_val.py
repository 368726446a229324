"""Validation throughput: the batched multi-day posterior pass against the
per-day validation forward, same model and data, one process.

Routes:
  a  validate_epoch(days)                  one graph replay per day
  b  validate_epoch(days, batched=True)    loss_many over packed days
  c  validate_epoch + validate_metrics     today's --val_metrics epoch tail
  d  validate_metrics(with_loss=True)      loss and ranking metrics, one pass
Inputs and labels are device resident for all four.

Method: as scripts/bench_eval.py — every route warmed up, then `--windows`
timed windows per route, alternating between the routes, each at least
`--min-seconds` long and closed by a device synchronise. Reported per
route: median days/s and the min..max spread; the ratios b/a and d/c are
median over median. The validation losses of the routes are printed next
to each other as a sanity check (they differ by their decoder noise).

Configs: CSI300 shape (N=300, T=20, C=158, H=64, K=20, D=256) and A-share
shape (N=3500, T=60, C=158, H=64, K=96, D=16).

  python scripts/bench_val.py [--configs csi300,ashare] [--dtype fp32]
      [--device-only] [--out results.jsonl]

--device-only runs route d alone (a few calls per config), for a kernel
trace of that route, taken in a run of its own.
"""
import argparse
import json
import os
import sys

CONFIGS = {
    "csi300": dict(N=300, T=20, C=158, H=64, M=128, K=20, D=256),
    "ashare": dict(N=3500, T=60, C=158, H=64, M=128, K=96, D=16),
}
ROUTES = ("a", "b", "c", "d")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", type=str, default="csi300,ashare")
    p.add_argument("--dtype", type=str, default="fp32",
                   choices=["fp32", "bf16"])
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--min-seconds", type=float, default=0.5)
    p.add_argument("--topk", type=int, default=50)
    p.add_argument("--device-only", action="store_true")
    p.add_argument("--calls", type=int, default=5,
                   help="route d calls of --device-only")
    p.add_argument("--label", type=str, default="")
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args()

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    import torch
    from bench_predict import summarize, timed_windows

    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    if not torch.cuda.is_available():
        raise SystemExit("bench_val.py needs a GPU: no timing without one")
    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)
    lines = []
    for name in args.configs.split(","):
        cfg = CONFIGS[name]
        N, T, C, D = cfg["N"], cfg["T"], cfg["C"], cfg["D"]
        set_seed(0)
        model = build_factorvae(num_latent=C, hidden_size=cfg["H"],
                                num_portfolio=cfg["M"],
                                num_factor=cfg["K"]).to(dev)
        tr = FusedTrainer(model, lr=0.0, t_max=1, device=dev, train=False,
                          dtype=args.dtype)
        g = torch.Generator().manual_seed(D)
        xs = [torch.randn(N, T, C, generator=g).to(dev) for _ in range(D)]
        ys = [(torch.randn(N, 1, generator=g) * 0.1).to(dev)
              for _ in range(D)]
        days = list(zip(xs, ys))
        last = {}

        def route_a():
            last["a"] = tr.validate_epoch(days)

        def route_b():
            last["b"] = tr.validate_epoch(days, batched=True)

        def route_c():
            last["c"] = tr.validate_epoch(days)
            last["c_RankIC"] = tr.validate_metrics(
                days, topk=args.topk)["RankIC"]

        def route_d():
            vm = tr.validate_metrics(days, topk=args.topk, with_loss=True)
            last["d"], last["d_RankIC"] = vm["loss"], vm["RankIC"]

        if args.device_only:
            for _ in range(args.calls):
                route_d()
            sync()
            print(json.dumps({"config": name, "dtype": args.dtype,
                              "calls": args.calls, "loss": last["d"],
                              "RankIC": last["d_RankIC"]}), flush=True)
            del tr, model, xs, ys, days
            torch.cuda.empty_cache()
            continue

        fns = {"a": route_a, "b": route_b, "c": route_c, "d": route_d}
        rates = {r: [] for r in ROUTES}
        for _ in range(args.windows):  # alternate the routes
            for r in ROUTES:
                rates[r] += timed_windows(fns[r], D, 1, args.min_seconds,
                                          sync)
        rec = {"config": name, "label": args.label, "dtype": args.dtype,
               "N": N, "T": T, "C": C, "H": cfg["H"], "K": cfg["K"], "D": D}
        for r in ROUTES:
            rec[f"{r}_days_per_s"] = summarize(rates[r])
            rec[f"{r}_val_loss"] = last[r]
        rec["RankIC_c"], rec["RankIC_d"] = last["c_RankIC"], last["d_RankIC"]
        rec["ratio_b_over_a"] = (rec["b_days_per_s"]["median"]
                                 / rec["a_days_per_s"]["median"])
        rec["ratio_d_over_c"] = (rec["d_days_per_s"]["median"]
                                 / rec["c_days_per_s"]["median"])
        # the ranking metrics do not depend on the noise: the same value
        assert rec["RankIC_c"] == rec["RankIC_d"], rec
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del tr, model, xs, ys, days
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
