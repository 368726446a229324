"""Risk-model throughput: FusedTrainer.risk_many against the scoring floor
and against the host route it replaces, same model and data, one process.

Routes, all over the same D device-resident days:
  predict   predict_many(return_dist=True): the floor, nothing of the risk
            model is computed
  risk      risk_many with equal weights
  solve     risk_many(solve=("minvar", "mv"))
  host      what a tree without the risk kernels can do:
            predict_many(return_dist=True, return_beta=True) brings mu,
            sigma and beta (N*K floats per day) to the host, then
            risk.portfolio_risk per day in float64 with the specific
            variance by subtraction, sigma^2 - beta^2 . factor_sigma^2.
            The prior factors it needs are handed to it for free (they are
            read once from risk_many outside the timed region).

Method: as scripts/bench_predict.py — every route warmed up, then
`--windows` timed windows per route, alternating between the routes, each
at least `--min-seconds` long and closed by a device synchronise.
Reported per route: median days/s and the min..max spread.

Configs: CSI300 shape (N=300, T=20, C=158, H=64, K=20, D=256) and A-share
shape (N=3500, T=60, C=158, H=64, K=96, D=64).

  python scripts/bench_risk.py [--configs csi300,ashare] [--dtype fp32]
      [--device-only risk|solve] [--out results.jsonl]

--device-only runs one route alone (a few calls per config), for a kernel
trace of that route.
"""
import argparse
import json
import os
import sys

CONFIGS = {
    "csi300": dict(N=300, T=20, C=158, H=64, M=128, K=20, D=256),
    "ashare": dict(N=3500, T=60, C=158, H=64, M=128, K=96, D=64),
}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", type=str, default="csi300,ashare")
    p.add_argument("--dtype", type=str, default="fp32",
                   choices=["fp32", "bf16"])
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--min-seconds", type=float, default=0.5)
    p.add_argument("--device-only", type=str, default=None,
                   choices=["risk", "solve"])
    p.add_argument("--calls", type=int, default=5,
                   help="risk_many calls of --device-only")
    p.add_argument("--label", type=str, default="")
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args()

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    import torch
    from bench_predict import summarize, timed_windows

    from factorvae_amd import risk
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    if not torch.cuda.is_available():
        raise SystemExit("bench_risk.py needs a GPU: no timing without one")
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
        g = torch.Generator(device=dev).manual_seed(D)
        xs = [torch.randn(N, T, C, generator=g, device=dev)
              for _ in range(D)]
        last = {}

        def predict_route():
            last["predict"] = tr.predict_many(xs, return_dist=True)

        def risk_route():
            last["risk"] = tr.risk_many(xs)

        def solve_route():
            last["solve"] = tr.risk_many(xs, solve=("minvar", "mv"))

        if args.device_only:
            fn = risk_route if args.device_only == "risk" else solve_route
            for _ in range(args.calls):
                fn()
            sync()
            r = last[args.device_only]
            print(json.dumps({"config": name, "dtype": args.dtype,
                              "route": args.device_only, "calls": args.calls,
                              "vol_mean": float(r["vol"].mean())}),
                  flush=True)
            del tr, model, xs
            torch.cuda.empty_cache()
            continue

        comp0 = tr.risk_many(xs, return_components=True)
        fmu = comp0["factor_mu"].double()
        fsig = comp0["factor_sigma"].double()
        w = torch.full((N,), 1.0 / N, dtype=torch.float64)

        def host_route():
            outs = tr.predict_many(xs, return_dist=True, return_beta=True)
            vols = []
            for d, (_, mu, sigma, beta) in enumerate(outs):
                beta = beta.double()
                s2 = (sigma.double().view(-1) ** 2
                      - (beta ** 2) @ (fsig[d] ** 2))
                comp = {"mu": mu.double().view(-1), "beta": beta,
                        "specific_var": s2, "factor_mu": fmu[d],
                        "factor_sigma": fsig[d]}
                vols.append(risk.portfolio_risk(comp, w)["vol"])
            last["host"] = torch.stack(vols)

        routes = {"predict": predict_route, "risk": risk_route,
                  "solve": solve_route, "host": host_route}
        rates = {k: [] for k in routes}
        for _ in range(args.windows):  # alternate the routes
            for k, fn in routes.items():
                rates[k] += timed_windows(fn, D, 1, args.min_seconds, sync)
        rec = {"config": name, "label": args.label, "dtype": args.dtype,
               "N": N, "T": T, "C": C, "H": cfg["H"], "K": cfg["K"], "D": D}
        for k in routes:
            rec[f"{k}_days_per_s"] = summarize(rates[k])
        med = lambda k: rec[f"{k}_days_per_s"]["median"]
        rec["risk_over_predict"] = med("risk") / med("predict")
        rec["solve_over_predict"] = med("solve") / med("predict")
        rec["risk_over_host"] = med("risk") / med("host")
        # sanity: the two routes' vol agree (the host one cancels in s2)
        dv = (last["host"].float() - last["risk"]["vol"]).abs().max()
        rec["vol_max_abs_diff_host_vs_device"] = float(dv)
        rec["solve_info_nonzero"] = int(
            (last["solve"]["solve_info"] != 0).sum())
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del tr, model, xs
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
