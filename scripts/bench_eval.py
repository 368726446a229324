"""Evaluation throughput: on-device FusedTrainer.validate_metrics against
the host route it replaces, same model and data, one process.

Host route = what a tree without the evaluation kernel can do:
predict_many(return_dist=True) over all D days, the per-stock mu joined
with the labels in a (datetime, instrument) DataFrame, utils.RankIC (one
scipy.spearmanr per day). Device route = validate_metrics: the same
packed kernel sequence, then daily_ic_seg, and only the per-day
statistics brought to the host. Inputs and labels are device resident for
both.

Method: as scripts/bench_predict.py — both routes warmed up, then
`--windows` timed windows per route, alternating between the routes, each
at least `--min-seconds` long and closed by a device synchronise.
Reported per route: median days/s and the min..max spread; the ratio is
median over median. The two RankIC values are printed next to each other
as a sanity check.

Configs: CSI300 shape (N=300, T=20, C=158, H=64, K=20, D=256) and A-share
shape (N=3500, T=60, C=158, H=64, K=96, D=16).

  python scripts/bench_eval.py [--configs csi300,ashare] [--dtype fp32]
      [--device-only] [--out results.jsonl]

--device-only runs validate_metrics alone (a few calls per config), for a
kernel trace of that route.
"""
import argparse
import json
import os
import sys

CONFIGS = {
    "csi300": dict(N=300, T=20, C=158, H=64, M=128, K=20, D=256),
    "ashare": dict(N=3500, T=60, C=158, H=64, M=128, K=96, D=16),
}


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
                   help="validate_metrics calls of --device-only")
    p.add_argument("--label", type=str, default="")
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args()

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    import numpy as np
    import pandas as pd
    import torch
    from bench_predict import summarize, timed_windows

    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import RankIC, set_seed

    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py needs a GPU: no timing without one")
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
        ys = [torch.randn(N, 1, generator=g).to(dev) for _ in range(D)]
        days = list(zip(xs, ys))
        index = pd.MultiIndex.from_product(
            [pd.bdate_range("2020-01-01", periods=D), range(N)],
            names=["datetime", "instrument"])
        last = {}

        def device_route():
            last["device"] = tr.validate_metrics(days, topk=args.topk)

        def host_route():
            outs = tr.predict_many(xs, return_dist=True)
            mu = torch.cat([o[1] for o in outs]).numpy().reshape(-1)
            lab = torch.cat(ys).cpu().numpy().reshape(-1)
            df = pd.DataFrame({"LABEL0": lab, "Pred": mu}, index=index)
            last["host"] = RankIC(df)

        if args.device_only:
            for _ in range(args.calls):
                device_route()
            sync()
            print(json.dumps({"config": name, "dtype": args.dtype,
                              "calls": args.calls,
                              "RankIC": last["device"]["RankIC"]}),
                  flush=True)
            del tr, model, xs, ys, days
            torch.cuda.empty_cache()
            continue

        rates = {"host": [], "device": []}
        for _ in range(args.windows):  # alternate the routes
            rates["host"] += timed_windows(host_route, D, 1,
                                           args.min_seconds, sync)
            rates["device"] += timed_windows(device_route, D, 1,
                                             args.min_seconds, sync)
        host_ric = float(last["host"]["RankIC"].iloc[0])
        rec = {"config": name, "label": args.label, "dtype": args.dtype,
               "N": N, "T": T, "C": C, "H": cfg["H"], "K": cfg["K"], "D": D,
               "host_route_days_per_s": summarize(rates["host"]),
               "validate_metrics_days_per_s": summarize(rates["device"]),
               "RankIC_host": host_ric,
               "RankIC_device": last["device"]["RankIC"]}
        rec["ratio"] = (rec["validate_metrics_days_per_s"]["median"]
                        / rec["host_route_days_per_s"]["median"])
        assert np.isclose(host_ric, last["device"]["RankIC"], atol=1e-9), rec
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
