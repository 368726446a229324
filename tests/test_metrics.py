"""Daily IC / RankIC / top-k oracle (factorvae_amd.metrics) against scipy
and direct references, its summary against utils.RankIC, and the opt-in
validation metrics / RankIC checkpoint selection of train_main (CPU)."""

import json
import math

import numpy as np
import pandas as pd
import pytest
import scipy.stats
import torch

from factorvae_amd.data.synthetic import make_synthetic_frame
from factorvae_amd.engine.trainer import train_main
from factorvae_amd.metrics import (daily_ic, evaluate_days_eager,
                                   summarize_ic)
from factorvae_amd.utils import DataArgument, RankIC, checkpoint_path

SIZES = [2, 3, 5, 64, 257, 1000]
TOL = 1e-12


def _inputs(n, kind, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    l = (0.3 * p + rng.standard_normal(n)).astype(np.float32)
    if kind == "tied":
        p = (np.round(p * 4) / 4).astype(np.float32)
        l = (np.round(l * 200) / 200).astype(np.float32)
        # both zeros present: they must tie
        if n >= 5:
            p[0], p[n // 2] = 0.0, -0.0
            l[1], l[n - 1] = -0.0, 0.0
    return p, l


def _scipy(p, l):
    """(pearson, spearman) of float64 copies; NaN where scipy's input is
    constant."""
    p, l = p.astype(np.float64), l.astype(np.float64)
    if p.size < 2 or np.ptp(p) == 0 or np.ptp(l) == 0:
        return math.nan, math.nan
    return (float(scipy.stats.pearsonr(p, l)[0]),
            float(scipy.stats.spearmanr(p, l)[0]))


def _close(a, b, tol=TOL):
    if math.isnan(b):
        return math.isnan(a)
    return abs(a - b) <= tol


@pytest.mark.parametrize("kind", ["continuous", "tied"])
@pytest.mark.parametrize("n", SIZES)
def test_daily_ic_matches_scipy(n, kind):
    p, l = _inputs(n, kind, seed=n)
    ic, ric, lg, sh, nv = daily_ic(p, l)
    ref_ic, ref_ric = _scipy(p, l)
    assert nv == n
    assert _close(ic, ref_ic), (ic, ref_ic)
    assert _close(ric, ref_ric), (ric, ref_ric)
    assert math.isnan(lg) and math.isnan(sh)  # topk = 0


@pytest.mark.parametrize("kind", ["continuous", "tied"])
def test_ranks_match_rankdata(kind):
    from factorvae_amd.metrics import _avg_ranks

    p, _ = _inputs(1000, kind, seed=3)
    r = _avg_ranks(p.astype(np.float64) + 0.0)
    assert np.array_equal(r, scipy.stats.rankdata(p.astype(np.float64)))
    assert np.array_equal(r, pd.Series(p).rank().to_numpy())


@pytest.mark.parametrize("n", [5, 64, 257, 1000])
def test_non_finite_rows_are_masked(n):
    p, l = _inputs(n, "tied", seed=100 + n)
    rng = np.random.default_rng(n)
    bad = [np.nan, np.inf, -np.inf]
    for arr, frac in ((l, 0.10), (p, 0.05)):
        for i in np.flatnonzero(rng.random(n) < frac):
            arr[i] = bad[i % 3]
    keep = np.isfinite(p) & np.isfinite(l)
    ic, ric, lg, sh, nv = daily_ic(p, l, topk=3)
    assert nv == int(keep.sum())
    ref_ic, ref_ric = _scipy(p[keep], l[keep])
    assert _close(ic, ref_ic) and _close(ric, ref_ric)
    ic2, ric2, lg2, sh2, _ = daily_ic(p[keep], l[keep], topk=3)
    assert (ic, ric, lg, sh) == (ic2, ric2, lg2, sh2)


def test_degenerate_days_give_nan():
    for n in (0, 1):
        p, l = _inputs(n, "continuous", seed=7)
        ic, ric, lg, sh, nv = daily_ic(p, l, topk=5)
        assert nv == n and math.isnan(ic) and math.isnan(ric)
        assert math.isnan(lg) == (n == 0)
    p, l = _inputs(64, "continuous", seed=8)
    for const_p, const_l in ((True, False), (False, True), (True, True)):
        pc = np.full_like(p, 0.37) if const_p else p
        lc = np.full_like(l, -1.25) if const_l else l
        ic, ric, *_ = daily_ic(pc, lc)
        assert math.isnan(ic) and math.isnan(ric)
    ic, ric, lg, sh, nv = daily_ic(np.full(9, np.nan, np.float32), l[:9], 4)
    assert nv == 0 and all(math.isnan(v) for v in (ic, ric, lg, sh))
    # one side invalid everywhere a row could count
    p2, l2 = p[:4].copy(), l[:4].copy()
    p2[:2], l2[2:] = np.inf, np.nan
    assert daily_ic(p2, l2)[4] == 0


@pytest.mark.parametrize("kind", ["continuous", "tied"])
@pytest.mark.parametrize("n", [5, 64, 257])
def test_topk_against_lexsort(n, kind):
    p, l = _inputs(n, kind, seed=200 + n)
    order = np.lexsort((np.arange(n), p.astype(np.float64) + 0.0))
    l64 = l.astype(np.float64)
    for k in (1, 50, n, n + 7):
        _, _, lg, sh, _ = daily_ic(p, l, topk=k)
        kk = min(k, n)
        assert abs(lg - l64[order[n - kk:]].mean()) <= TOL
        assert abs(sh - l64[order[:kk]].mean()) <= TOL


def test_topk_tie_rule_higher_index_is_higher():
    p = np.array([1.0, 1.0, 1.0, 0.0, -0.0], np.float32)
    l = np.array([10.0, 20.0, 30.0, 40.0, 50.0], np.float32)
    _, _, lg, sh, _ = daily_ic(p, l, topk=1)
    assert lg == 30.0 and sh == 40.0
    _, _, lg, sh, _ = daily_ic(p, l, topk=2)
    assert lg == 25.0 and sh == 45.0


def test_summarize_ic_equals_utils_rankic():
    rng = np.random.default_rng(5)
    days = pd.bdate_range("2020-01-01", periods=6)
    names = [f"s{i}" for i in range(15)]
    idx = pd.MultiIndex.from_product([days, names],
                                     names=["datetime", "instrument"])
    pred = np.round(rng.standard_normal(len(idx)), 1).astype(np.float32)
    lab = (0.5 * pred + rng.standard_normal(len(idx))).astype(np.float32)
    df = pd.DataFrame({"LABEL0": lab, "Pred": pred}, index=idx)
    ref = RankIC(df)
    per = [daily_ic(df.loc[d]["Pred"].to_numpy(), df.loc[d]["LABEL0"].to_numpy(),
                    topk=3) for d in days]
    # two more days that carry no RankIC: skipped by the summary
    per.append(daily_ic(np.ones(4, np.float32), np.arange(4.0), topk=3))
    per.append(daily_ic(np.zeros(0, np.float32), np.zeros(0, np.float32)))
    a = np.array([r[:4] for r in per])
    out = summarize_ic({"ic": a[:, 0], "rank_ic": a[:, 1], "long": a[:, 2],
                        "short": a[:, 3]})
    assert out["n_days"] == 6
    assert abs(out["RankIC"] - float(ref["RankIC"].iloc[0])) <= TOL
    assert abs(out["RankIC_IR"] - float(ref["RankIC_IR"].iloc[0])) <= 1e-9
    fin = a[np.isfinite(a[:, 2])]
    assert abs(out["long_short"] - np.mean(fin[:, 2] - fin[:, 3])) <= TOL
    assert abs(out["ICIR"] - np.mean(a[:6, 0]) / np.std(a[:6, 0])) <= 1e-9
    empty = summarize_ic({"ic": [], "rank_ic": [], "long": [], "short": []})
    assert empty["n_days"] == 0 and math.isnan(empty["RankIC"])
    one = summarize_ic({"ic": [0.1], "rank_ic": [0.2], "long": [1.0],
                        "short": [0.5]})
    assert math.isnan(one["RankIC_IR"]) and one["RankIC"] == 0.2


def test_evaluate_days_eager_is_the_oracle_on_its_own_mu():
    from factorvae_amd.models.modules import build_factorvae

    torch.manual_seed(0)
    model = build_factorvae(num_latent=10, hidden_size=8, num_portfolio=12,
                            num_factor=4)
    g = torch.Generator().manual_seed(1)
    days = [(torch.randn(n, 5, 10, generator=g), torch.randn(n, 1, generator=g))
            for n in (7, 1, 0, 30)]
    days[3][1][4] = float("nan")
    state = torch.get_rng_state()
    out = evaluate_days_eager(model, days, on=("mu",), topk=2)
    assert torch.equal(state, torch.get_rng_state())  # mu draws nothing
    assert out["columns"] == ("mu",) and out["ic"].shape == (4, 1)
    assert out["count"].reshape(-1).tolist() == [7, 1, 0, 29]
    model.eval()
    for d in (0, 3):
        mu, _ = model.prediction_dist(days[d][0])
        ref = daily_ic(mu.numpy(), days[d][1].numpy(), topk=2)
        got = tuple(float(out[k][d, 0])
                    for k in ("ic", "rank_ic", "long", "short"))
        assert got == ref[:4]
    both = evaluate_days_eager(model, days, on=("score", "mu"), topk=2)
    assert both["ic"].shape == (4, 2)
    assert np.array_equal(both["rank_ic"][:, 1], out["rank_ic"][:, 0],
                          equal_nan=True)


# ------------------------------------------------------------ train_main
class Args:
    num_epochs = 2
    lr = 1e-3
    num_latent = 10
    num_portfolio = 12
    seq_len = 5
    num_factor = 4
    hidden_size = 8
    seed = 42
    run_name = "unit"
    num_workers = 0
    wandb = False
    engine = "eager"


NEW_LOG_KEYS = ("Validation IC", "Validation RankIC", "Validation RankIC_IR")


def _run(tmp_path, **extra):
    df = make_synthetic_frame(n_days=40, n_stocks=12, n_features=10, seed=0,
                              start="2015-01-01")
    args = Args()
    args.save_dir = str(tmp_path)
    args.dataset = None
    for k, v in extra.items():
        setattr(args, k, v)
    data_args = DataArgument(start_time="2015-01-01", fit_end_time="2015-02-10",
                             val_start_time="2015-02-11", val_end_time="2015-02-25",
                             end_time="2015-02-25", seq_len=5)
    best = train_main(args, data_args, df=df)
    ckpt = checkpoint_path(str(tmp_path), "unit", 4, 8, 12, 42)
    recs = [json.loads(line)
            for line in open(tmp_path / "unit_metrics.jsonl")]
    return best, ckpt, recs, df, data_args


def test_train_main_select_by_rankic(tmp_path):
    import os

    from factorvae_amd.data.sampler import init_data_loader
    from factorvae_amd.models.modules import build_factorvae

    best, ckpt, recs, df, da = _run(tmp_path, select_by="rankic", val_topk=3)
    assert np.isfinite(best)
    assert os.path.exists(ckpt) and os.path.exists(ckpt + ".opt")
    side = torch.load(ckpt + ".opt", map_location="cpu", weights_only=True)
    assert side["select_by"] == "rankic"
    assert np.isfinite(side["best_val_rankic"])
    epochs = [r for r in recs if "Train Loss" in r]
    assert len(epochs) == 2
    for r in epochs:
        for k in NEW_LOG_KEYS + ("Validation long_short",):
            assert k in r
    assert side["best_val_rankic"] == max(r["Validation RankIC"]
                                          for r in epochs)
    assert best == min(r["Validation Loss"] for r in epochs)
    assert recs[-1]["Best Validation RankIC"] == side["best_val_rankic"]
    # the saved weights are the ones that scored the best RankIC
    model = build_factorvae(num_latent=10, hidden_size=8, num_portfolio=12,
                            num_factor=4)
    model.load_state_dict(torch.load(ckpt, weights_only=True))
    loader = init_data_loader(df, shuffle=False, step_len=5,
                              start=da.val_start_time, end=da.val_end_time)
    days = [(c[:, :, :-1].float(), c[:, -1, -1].float()) for c, _ in loader]
    again = summarize_ic(evaluate_days_eager(model, days, topk=3))
    assert abs(again["RankIC"] - side["best_val_rankic"]) <= 1e-9


def test_train_main_val_metrics_only_logs(tmp_path):
    _, ckpt, recs, _, _ = _run(tmp_path, val_metrics=True)
    side = torch.load(ckpt + ".opt", map_location="cpu", weights_only=True)
    assert "select_by" not in side and "best_val_rankic" not in side
    epochs = [r for r in recs if "Train Loss" in r]
    assert all(k in r for r in epochs for k in NEW_LOG_KEYS)
    assert all("Validation long_short" not in r for r in epochs)


def test_train_main_defaults_carry_no_new_keys(tmp_path):
    _, ckpt, recs, _, _ = _run(tmp_path)
    side = torch.load(ckpt + ".opt", map_location="cpu", weights_only=True)
    assert set(side) == {"epoch", "best_val_loss", "optimizer", "scheduler"}
    for r in recs:
        assert not any("IC" in k or "long_short" in k for k in r), r
    assert set(recs[-1]) == {"Best Validation Loss", "ts"}


def test_score_cli_metrics_json(tmp_path):
    """score.py --metrics writes the summary next to an unchanged CSV."""
    from factorvae_amd import score

    _, ckpt, _, df, _ = _run(tmp_path)
    data = tmp_path / "d.pkl"
    df.to_pickle(data)
    base = ["--checkpoint", ckpt, "--dataset", str(data), "--run_name", "m",
            "--num_factor", "4", "--hidden_size", "8", "--num_latent", "10",
            "--num_portfolio", "12", "--seq_length", "5",
            "--start", "2015-02-11"]
    torch.manual_seed(0)
    plain = score.main(base + ["--out_dir", str(tmp_path / "a")])
    torch.manual_seed(0)
    with_m = score.main(base + ["--out_dir", str(tmp_path / "b"), "--metrics",
                                "--metrics_topk", "3"])
    assert plain.equals(with_m)
    name = "m_4_True_False_10_8"
    assert (tmp_path / "a" / f"{name}.csv").read_bytes() == \
        (tmp_path / "b" / f"{name}.csv").read_bytes()
    assert not (tmp_path / "a" / f"{name}_metrics.json").exists()
    out = json.load(open(tmp_path / "b" / f"{name}_metrics.json"))
    assert set(out) == {"IC", "ICIR", "RankIC", "RankIC_IR", "long_short",
                        "n_days", "topk"}
    assert out["topk"] == 3 and out["n_days"] > 0
    assert np.isfinite(out["RankIC"]) and np.isfinite(out["long_short"])


def test_resume_restores_rankic_selection(tmp_path):
    _, ckpt, recs, _, _ = _run(tmp_path, select_by="rankic", num_epochs=1)
    first = torch.load(ckpt + ".opt", map_location="cpu", weights_only=True)
    assert first["epoch"] == 1
    # no select_by on the resumed run: the side-car's carries over
    _, _, recs, _, _ = _run(tmp_path, resume=True, num_epochs=3)
    epochs = [r for r in recs if "Train Loss" in r]
    assert [r["epoch"] for r in epochs] == [0, 1, 2]
    assert all("Validation RankIC" in r for r in epochs)
    side = torch.load(ckpt + ".opt", map_location="cpu", weights_only=True)
    assert side["select_by"] == "rankic"
    assert side["best_val_rankic"] == max(r["Validation RankIC"]
                                          for r in epochs)
    assert side["best_val_rankic"] >= first["best_val_rankic"]
