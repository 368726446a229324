"""Scoring / backtest CLI — the reference's backtest.ipynb cells 2-9 as
a command-line entry point.

checkpoint -> prediction scores over a date range -> optional CSV dump
(same schema as the reference's released artifacts:
`{run_name}_{K}_{normalize}_{select_feature}_{C}_{H}.csv`, columns
datetime,instrument,score — /root/reference/scores/readme.md) ->
optional top-k dropout backtest + risk report + RankIC.

Run:  python -m factorvae_amd.score --checkpoint best_models/x.pt \
          --dataset data/synthetic.pkl --run_name demo [--backtest]
"""

from __future__ import annotations

import argparse
import json
import os

import pandas as pd
import torch

from .backtest import BacktestConfig, backtest_report, topk_dropout_backtest
from .data.panel import PanelDays
from .data.sampler import init_data_loader
from .utils import RankIC, generate_prediction_scores, load_model, test_args


def build_argparser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Score a test range with a "
                                            "trained FactorVAE checkpoint")
    p.add_argument("--checkpoint", type=str, required=True)
    p.add_argument("--dataset", type=str, required=True, help="data pickle")
    p.add_argument("--run_name", type=str, default="scores")
    p.add_argument("--num_factor", type=int, default=96)
    p.add_argument("--hidden_size", type=int, default=64)
    p.add_argument("--num_latent", type=int, default=158)
    p.add_argument("--num_portfolio", type=int, default=128)
    p.add_argument("--seq_length", type=int, default=20)
    p.add_argument("--start", type=str, default=None)
    p.add_argument("--end", type=str, default=None)
    p.add_argument("--out_dir", type=str, default="./scores")
    p.add_argument("--normalize", action=argparse.BooleanOptionalAction,
                   default=True)
    p.add_argument("--select_feature", action=argparse.BooleanOptionalAction,
                   default=False)
    p.add_argument("--engine", type=str, default="auto",
                   choices=["auto", "fused", "eager"],
                   help="auto = fused HIP predict path on GPU, eager "
                        "module path otherwise")
    p.add_argument("--batch_days", type=int, default=1,
                   help="score this many consecutive days per call of the "
                        "batched path (1 = one day at a time)")
    p.add_argument("--dist", action="store_true",
                   help="also write the predictive mean and risk as mu and "
                        "sigma columns")
    p.add_argument("--risk_aversion", type=float, default=0.0,
                   help="eta != 0: score = mu - eta * sigma (deterministic; "
                        "implies --dist)")
    p.add_argument("--backtest", action="store_true",
                   help="run the top-k dropout backtest + risk report")
    p.add_argument("--report", action="store_true",
                   help="with --backtest: also write backtest.png and the "
                        "plotly HTML report (the reference notebook's "
                        "backtest.png / backtest_plotly/ artifacts)")
    p.add_argument("--metrics", action="store_true",
                   help="also evaluate the range's daily IC / RankIC and "
                        "top-k long/short spread on the predictive mean and "
                        "write them as JSON next to the score CSV")
    p.add_argument("--metrics_topk", type=int, default=50,
                   help="k of the --metrics long/short spread")
    p.add_argument("--factors", action="store_true",
                   help="also write each day's posterior and prior factors "
                        "(<stem>_factors.csv) and its validation loss terms "
                        "(<stem>_daily.csv) next to the score CSV; decoder "
                        "noise off, so the files are reproducible")
    p.add_argument("--panel", action="store_true",
                   help="hold the range once per (stock, date) row and send "
                        "the scores, --dist, --metrics and --factors through "
                        "the panel route (faster on the fused engine, the "
                        "same files on the eager one)")
    p.add_argument("--risk", action="store_true",
                   help="with --dist: also write the factor risk model's "
                        "view of the equal-weight portfolio of the --topk "
                        "stocks by predictive mean: <stem>_risk.csv (mean, "
                        "factor and "
                        "specific variance, vol per day) and "
                        "<stem>_risk_factors.csv (exposure and variance per "
                        "day and factor)")
    p.add_argument("--risk_weights", type=str, default=None,
                   choices=["minvar", "mv"],
                   help="with --risk: also write <stem>_weights.csv, the "
                        "minimum-variance or mean-variance weights of every "
                        "day's stocks under the model's covariance")
    p.add_argument("--topk", type=int, default=50)
    p.add_argument("--n_drop", type=int, default=10)
    return p


def _panel_windows(panel):
    """The days of a PanelDays as the eager code takes them."""
    return [panel.windows(d) for d in range(len(panel))]


def range_metrics(model, loader, seq_length: int, engine: str = "auto",
                  topk: int = 50, panel: bool = False):
    """Summary of the loader's days ranked on the predictive mean: the
    fused engine's on-device evaluation on a GPU (engine "auto"/"fused"),
    metrics.py's oracle on the eager module otherwise. panel=True takes
    the days as a PanelDays (the fused engine's panel route; the eager
    engine evaluates its windows())."""
    from .engine.trainer import resolve_engine
    from .metrics import evaluate_days_eager, summarize_ic

    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model.to(device)
    hidden = model.feature_extractor.gru.hidden_size
    fused = resolve_engine(engine, hidden, device.type, warn=False) == "fused"
    if panel:
        days = PanelDays.from_loader(loader)
        if not fused:
            days = _panel_windows(days)
    else:
        days = []
        for char_with_label, _ in loader:
            if char_with_label.shape[1] != seq_length:
                continue
            days.append((char_with_label[:, :, :-1].float(),
                         char_with_label[:, -1, -1].float()))
    if fused:
        from .engine.fused import FusedTrainer

        trainer = FusedTrainer(model, lr=0.0, t_max=1, device=device,
                               train=False)
        return trainer.validate_metrics(days, topk=topk)
    return summarize_ic(evaluate_days_eager(model, days, on=("mu",),
                                            topk=topk))


def range_factors(model, loader, seq_length: int, engine: str = "auto",
                  panel: bool = False):
    """The factors and the validation loss of every day of the loader, with
    the decoder noise off (the reconstruction is the posterior mean), so
    the result is reproducible: (factors, daily) DataFrames —
      factors: one row per (day, factor): datetime, factor, post_mu,
               post_sigma, prior_mu, prior_sigma (the posterior is the
               realised factor return given that day's labels);
      daily:   one row per day: datetime, n_stocks, loss, mse, kl.
    The fused engine's loss_many on a GPU (engine "auto"/"fused"),
    metrics.loss_days_eager on the eager module otherwise. Dates come from
    the dataset's (datetime, instrument) index, walked in loader order as
    generate_prediction_scores does. panel=True takes days and dates from
    a PanelDays (the fused engine's panel route; the eager engine works on
    its windows())."""
    from .engine.trainer import resolve_engine
    from .metrics import FACTOR_KEYS, loss_days_eager

    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model.to(device)
    hidden = model.feature_extractor.gru.hidden_size
    fused = resolve_engine(engine, hidden, device.type, warn=False) == "fused"
    if panel:
        # a loader day always has rows, so none is left out here either
        days = PanelDays.from_loader(loader)
        dates = days.dates
        if not fused:
            days = _panel_windows(days)
    else:
        index = loader.dataset.get_index()
        days, dates, row = [], [], 0
        for char_with_label, _ in loader:
            n = int(char_with_label.shape[0])
            if char_with_label.shape[1] == seq_length and n > 0:
                days.append((char_with_label[:, :, :-1].float(),
                             char_with_label[:, -1, -1].float()))
                dates.append(index[row][0])
            row += n
    if fused:
        from .engine.fused import FusedTrainer

        trainer = FusedTrainer(model, lr=0.0, t_max=1, device=device,
                               train=False)
        r = trainer.loss_many(days, sample=False, return_factors=True)
    else:
        r = loss_days_eager(model, days, sample=False, return_factors=True)
    D = len(days)
    K = r["post_mu"].shape[1] if D else 0
    factors = pd.DataFrame({
        "datetime": [d for d in dates for _ in range(K)],
        "factor": list(range(K)) * D,
        **{k: r[k].reshape(-1).numpy() for k in FACTOR_KEYS}})
    daily = pd.DataFrame({
        "datetime": dates, "n_stocks": r["n"].numpy(),
        **{k: r[k].numpy() for k in ("loss", "mse", "kl")}})
    return factors, daily


def range_risk(model, loader, seq_length: int, scores, engine: str = "auto",
               topk: int = 50, risk_weights=None, panel: bool = False):
    """The factor risk model (factorvae_amd.risk) of every day of the
    loader for the equal-weight portfolio of the topk stocks by predictive
    mean, taken from the `mu` column of `scores` (the frame
    generate_prediction_scores returned for this loader, in its row
    order): (risk, factors, weights) DataFrames —
      risk:    one row per day: datetime, n_stocks, mean, mean_factor,
               var_factor, var_specific, vol;
      factors: one row per (day, factor): datetime, factor, exposure,
               factor_var;
      weights: None, or with risk_weights in ("minvar", "mv") one row per
               (day, stock): datetime, instrument, weight.
    The fused engine's risk_many on a GPU (engine "auto"/"fused"),
    risk.risk_days_eager on the eager module otherwise; panel=True takes
    the days from a PanelDays."""
    from .engine.trainer import resolve_engine
    from .risk import STAT_KEYS, risk_days_eager

    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model.to(device)
    hidden = model.feature_extractor.gru.hidden_size
    fused = resolve_engine(engine, hidden, device.type, warn=False) == "fused"
    index = loader.dataset.get_index()
    mu_all = torch.as_tensor(scores["mu"].to_numpy())
    days, dates, spans, row = [], [], [], 0
    for char_with_label, _ in loader:
        n = int(char_with_label.shape[0])
        if char_with_label.shape[1] == seq_length and n > 0:
            days.append(char_with_label[:, :, :-1].float())
            dates.append(index[row][0])
            spans.append((row, n))
        row += n
    if panel:
        # the loader's days, held once per (stock, date) row
        pdays = PanelDays.from_loader(loader)
        days = pdays if fused else [pdays.windows(d)[0]
                                    for d in range(len(pdays))]
    weights = []
    for r0, n in spans:
        k = max(1, min(int(topk), n))
        w = torch.zeros(n)
        w[torch.topk(mu_all[r0:r0 + n], k).indices] = 1.0 / k
        weights.append(w)
    solve = (risk_weights,) if risk_weights else ()
    if fused:
        from .engine.fused import FusedTrainer

        trainer = FusedTrainer(model, lr=0.0, t_max=1, device=device,
                               train=False)
        r = trainer.risk_many(days, weights=weights, solve=solve)
    else:
        r = risk_days_eager(model, days, weights=weights, solve=solve)
    D = len(dates)
    K = r["exposure"].shape[1] if D else 0
    risk = pd.DataFrame({
        "datetime": dates, "n_stocks": r["n"].numpy(),
        **{k: r[k].numpy() for k in STAT_KEYS}})
    factors = pd.DataFrame({
        "datetime": [d for d in dates for _ in range(K)],
        "factor": list(range(K)) * D,
        "exposure": r["exposure"].reshape(-1).numpy(),
        "factor_var": r["factor_var"].reshape(-1).numpy()})
    wdf = None
    if risk_weights:
        rows = [index[i] for r0, n in spans for i in range(r0, r0 + n)]
        wdf = pd.DataFrame({
            "datetime": [t[0] for t in rows],
            "instrument": [t[1] for t in rows],
            "weight": (torch.cat(r[risk_weights]).numpy() if D
                       else torch.empty(0).numpy())})
    return risk, factors, wdf


def main(argv=None):
    parser = build_argparser()
    args = parser.parse_args(argv)
    if args.risk and not args.dist:
        parser.error("--risk needs --dist (the portfolio is built from the "
                     "predictive mean)")
    if args.risk_weights and not args.risk:
        parser.error("--risk_weights needs --risk")
    targs = test_args(
        run_name=args.run_name, num_factor=args.num_factor,
        hidden_size=args.hidden_size, num_latent=args.num_latent,
        num_portfolio=args.num_portfolio, seq_length=args.seq_length,
    )
    model = load_model(targs)
    state = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
    model.load_state_dict(state)
    model.eval()

    df = pd.read_pickle(args.dataset)
    loader = init_data_loader(df, step_len=args.seq_length, shuffle=False,
                              start=args.start, end=args.end)
    scores = generate_prediction_scores(model, loader, loader.dataset,
                                        targs, engine=args.engine,
                                        batch_days=args.batch_days,
                                        return_dist=args.dist,
                                        risk_aversion=args.risk_aversion,
                                        panel=args.panel)

    os.makedirs(args.out_dir, exist_ok=True)
    # reference artifact name schema (scores/readme.md)
    fname = (f"{args.run_name}_{args.num_factor}_{args.normalize}_"
             f"{args.select_feature}_{args.num_latent}_{args.hidden_size}.csv")
    out_csv = os.path.join(args.out_dir, fname)
    scores.to_csv(out_csv)
    print(f"wrote {out_csv}: {len(scores)} rows")

    if args.metrics:
        summary = range_metrics(model, loader, args.seq_length,
                                engine=args.engine, topk=args.metrics_topk,
                                panel=args.panel)
        print("\nmetrics on mu:")
        for k in ("IC", "ICIR", "RankIC", "RankIC_IR", "long_short",
                  "n_days"):
            print(f"  {k}: {summary[k]}")
        out_json = os.path.splitext(out_csv)[0] + "_metrics.json"
        with open(out_json, "w") as f:
            json.dump(dict(summary, topk=args.metrics_topk), f, indent=1)
        print(f"wrote {out_json}")

    if args.factors:
        factors, daily = range_factors(model, loader, args.seq_length,
                                       engine=args.engine, panel=args.panel)
        stem = os.path.splitext(out_csv)[0]
        factors.to_csv(stem + "_factors.csv", index=False)
        daily.to_csv(stem + "_daily.csv", index=False)
        print(f"wrote {stem}_factors.csv ({len(factors)} rows) and "
              f"{stem}_daily.csv ({len(daily)} days)")

    if args.risk:
        risk, rfac, wdf = range_risk(model, loader, args.seq_length, scores,
                                     engine=args.engine, topk=args.topk,
                                     risk_weights=args.risk_weights,
                                     panel=args.panel)
        stem = os.path.splitext(out_csv)[0]
        risk.to_csv(stem + "_risk.csv", index=False)
        rfac.to_csv(stem + "_risk_factors.csv", index=False)
        print(f"wrote {stem}_risk.csv ({len(risk)} days) and "
              f"{stem}_risk_factors.csv ({len(rfac)} rows)")
        if wdf is not None:
            wdf.to_csv(stem + "_weights.csv", index=False)
            print(f"wrote {stem}_weights.csv ({len(wdf)} rows)")

    if args.backtest:
        merged = scores.join(df[["LABEL0"]], how="inner")
        result = topk_dropout_backtest(
            merged, config=BacktestConfig(topk=args.topk, n_drop=args.n_drop))
        report = backtest_report(result)
        print("\nexcess_return_without_cost:")
        print(report["excess_return_without_cost"])
        print("\nexcess_return_with_cost:")
        print(report["excess_return_with_cost"])
        print(f"\nNOTE: {report['note']}")
        print("\nRankIC:")
        print(RankIC(merged, column1="LABEL0", column2="score"))
        if args.report:
            from .report import write_backtest_png, write_plotly_report

            png = write_backtest_png(
                result, os.path.join(args.out_dir, "backtest.png"),
                title=f"{args.run_name} backtest")
            html = write_plotly_report(
                result, os.path.join(args.out_dir, "backtest_plotly"))
            print(f"wrote {png} and {html}")
    return scores


if __name__ == "__main__":
    main()
