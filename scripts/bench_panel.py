"""Batched scoring and evaluation on windows against the same calls on a
PanelDays of the same days, same model, one process.

Dense route = FusedTrainer.predict_many / evaluate_many(with_loss=True) on
D consecutive days held as (N, T, C) windows. Panel route = the same calls
on a data.panel.PanelDays of those days: (D + T - 1) * N feature rows and
one (N, T) index matrix per day; the extractor head runs once per row and
the GRU gathers. Inputs are device resident for both, and with --host also
measured from host memory (windows against panel).

Method: every shape is warmed up first; then `--windows` timed windows per
route, alternating between the routes, each window long enough
(`--min-seconds`) to be far above timer and scheduler noise and closed by
a device synchronise. Reported per route: median days/s and the min..max
spread over the windows; the ratio is median over median.

Configs: CSI300 shape (N=300, T=20, C=158, H=64, K=20, D=256) and A-share
shape (N=3500, T=60, C=158, H=64, K=96, D in 8/64).

  python scripts/bench_panel.py [--configs csi300,ashare] [--dtype fp32]
      [--host] [--calls predict_many,evaluate_many] [--out results.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_predict import summarize, timed_windows  # noqa: E402

CONFIGS = {
    "csi300": dict(N=300, T=20, C=158, H=64, M=128, K=20, D=(256,)),
    "ashare": dict(N=3500, T=60, C=158, H=64, M=128, K=96, D=(8, 64)),
}


def make_panel(torch, PanelDays, N, T, C, D, seed):
    """D consecutive days of a full (date, stock) frame in frame order."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn((D + T - 1) * N, C, generator=g)
    stocks = torch.arange(N, dtype=torch.int32)[:, None]
    ids = [(torch.arange(d, d + T, dtype=torch.int32)[None, :] * N + stocks)
           for d in range(D)]
    labels = [torch.randn(N, generator=g) for _ in range(D)]
    return PanelDays(rows, ids, labels)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", type=str, default="csi300,ashare")
    p.add_argument("--dtype", type=str, default="fp32",
                   choices=["fp32", "bf16"])
    p.add_argument("--calls", type=str, default="predict_many,evaluate_many")
    p.add_argument("--days", type=str, default="",
                   help="comma-separated D values instead of the config's")
    p.add_argument("--host", action="store_true",
                   help="also time both routes from host inputs")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--min-seconds", type=float, default=0.5)
    p.add_argument("--label", type=str, default="")
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args()

    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    import torch

    from factorvae_amd.data.panel import PanelDays
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    if not torch.cuda.is_available():
        raise SystemExit("bench_panel.py needs a GPU: no timing without one")
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
        Ds = ([int(d) for d in args.days.split(",")] if args.days
              else cfg["D"])
        for D in Ds:
            host_panel = make_panel(torch, PanelDays, N, T, C, D, seed=D)
            inputs = {"device": host_panel.to(dev)}
            if args.host:
                inputs["host"] = host_panel
            for where, panel in inputs.items():
                days = [panel.windows(d) for d in range(D)]
                xs = [x for x, _ in days]
                routes = {
                    "predict_many": (lambda: tr.predict_many(xs),
                                     lambda: tr.predict_many(panel)),
                    "evaluate_many": (
                        lambda: tr.evaluate_many(days, with_loss=True),
                        lambda: tr.evaluate_many(panel, with_loss=True)),
                }
                for call in args.calls.split(","):
                    dense, pan = routes[call]
                    rates = {"dense": [], "panel": []}
                    for _ in range(args.windows):
                        rates["dense"] += timed_windows(
                            dense, D, 1, args.min_seconds, sync)
                        rates["panel"] += timed_windows(
                            pan, D, 1, args.min_seconds, sync)
                    rec = {"config": name, "label": args.label,
                           "dtype": args.dtype, "call": call,
                           "inputs": where, "N": N, "T": T, "C": C,
                           "H": cfg["H"], "K": cfg["K"], "D": D,
                           "window_rows": D * N * T,
                           "panel_rows": int(panel.rows.shape[0]),
                           "dense_days_per_s": summarize(rates["dense"]),
                           "panel_days_per_s": summarize(rates["panel"])}
                    rec["ratio"] = (rec["panel_days_per_s"]["median"]
                                    / rec["dense_days_per_s"]["median"])
                    line = json.dumps(rec)
                    print(line, flush=True)
                    lines.append(line)
                del days, xs
            del inputs, host_panel
            torch.cuda.empty_cache()
        del tr, model
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
