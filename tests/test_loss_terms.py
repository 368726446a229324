"""The posterior pass on the eager engine: FactorVAE.loss_terms (forward's
math with the noise as an argument and every term named),
metrics.loss_days_eager over ragged days, the score CLI's --factors files
and train_main's --val_batched flag."""

import json

import numpy as np
import pandas as pd
import pytest
import torch

from factorvae_amd.data.sampler import init_data_loader
from factorvae_amd.data.synthetic import make_synthetic_frame
from factorvae_amd.metrics import FACTOR_KEYS, loss_days_eager
from factorvae_amd.models.modules import build_factorvae

C, H, M, K, T = 6, 8, 4, 3, 4


def _model(seed=0):
    torch.manual_seed(seed)
    return build_factorvae(num_latent=C, hidden_size=H, num_portfolio=M,
                           num_factor=K).eval()


def _day(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, T, C, generator=g),
            torch.randn(n, 1, generator=g) * 0.1)


@pytest.fixture(scope="module")
def frame():
    return make_synthetic_frame(n_days=14, n_stocks=9, n_features=C, seed=3,
                                ragged=True)


@pytest.mark.parametrize("N", [1, 13])
def test_loss_terms_is_forward_with_the_noise_as_an_argument(N):
    model = _model()
    x, y = _day(N, 1)
    with torch.no_grad():
        torch.manual_seed(7)
        loss, recon, fmu, fsig, pmu, psig = model(x, y)
        torch.manual_seed(7)
        t = model.loss_terms(x, y, eps=torch.randn(N, 1))
        torch.manual_seed(7)
        drawn = model.loss_terms(x, y.view(-1))  # eps=None draws it itself
    assert set(t) == {"loss", "mse", "kl", "recon"} | set(FACTOR_KEYS)
    for got in (t, drawn):
        assert torch.equal(got["loss"], loss)
        assert torch.equal(got["recon"], recon) and recon.shape == (N, 1)
        assert torch.equal(got["post_mu"], fmu)
        assert torch.equal(got["post_sigma"], fsig)
        assert torch.equal(got["prior_mu"], pmu)
        assert torch.equal(got["prior_sigma"], psig)
        assert torch.equal(got["loss"], got["mse"] + got["kl"])
    assert t["post_mu"].shape == t["prior_sigma"].shape == (K,)
    # the terms are what they are called
    assert torch.equal(t["mse"], torch.nn.functional.mse_loss(recon, y))
    assert torch.equal(t["kl"], model.KL_Divergence(fmu, fsig, pmu, psig))


def test_post_sigma_keeps_the_zero_clamp():
    """A posterior sigma of exactly zero enters the decoder and the KL term
    as 1e-6 and is returned as such."""
    model = _model()
    with torch.no_grad():
        model.factor_encoder.linear_sigma.weight.zero_()
        model.factor_encoder.linear_sigma.bias.fill_(-200.0)
        x, y = _day(7, 2)
        assert bool((model.factor_encoder(model.feature_extractor(x), y)[1]
                     == 0).all())
        t = model.loss_terms(x, y, eps=torch.zeros(7, 1))
    assert torch.equal(t["post_sigma"], torch.full((K,), 1e-6))
    assert bool(torch.isfinite(t["kl"])) and bool(torch.isfinite(t["loss"]))
    with torch.no_grad():
        mu, _ = model.factor_decoder.dist(model.feature_extractor(x),
                                          t["post_mu"], t["post_sigma"])
    assert torch.equal(t["recon"], mu)


def test_loss_days_eager_over_ragged_days():
    model = _model()
    lens = [5, 0, 1, 11]
    days = [_day(n, 10 + i) for i, n in enumerate(lens)]
    eps = [torch.randn(n, generator=torch.Generator().manual_seed(20 + i))
           for i, n in enumerate(lens)]
    r = loss_days_eager(model, days, eps=eps, return_factors=True)
    assert set(r) == {"loss", "mse", "kl", "n"} | set(FACTOR_KEYS)
    assert r["n"].dtype == torch.int32 and r["n"].tolist() == lens
    assert r["loss"].dtype == torch.float32 and r["loss"].shape == (4,)
    assert r["post_mu"].shape == (4, K)
    for d, (x, y) in enumerate(days):
        if lens[d] == 0:
            assert all(bool(torch.isnan(r[k][d]).all()) for k in r
                       if k != "n")
            continue
        with torch.no_grad():
            t = model.loss_terms(x, y, eps=eps[d].view(-1, 1))
        for k in r:
            if k != "n":
                assert torch.equal(r[k][d], t[k]), (d, k)
    plain = loss_days_eager(model, days, eps=eps)
    assert set(plain) == {"loss", "mse", "kl", "n"}
    assert torch.equal(plain["loss"][[0, 2, 3]], r["loss"][[0, 2, 3]])
    # sample=False is eps = 0 and draws nothing
    state = torch.random.get_rng_state()
    zero = loss_days_eager(model, days, sample=False)
    assert torch.equal(torch.random.get_rng_state(), state)
    with torch.no_grad():
        t = model.loss_terms(*days[3], eps=torch.zeros(11, 1))
    assert torch.equal(zero["loss"][3], t["loss"])
    assert not model.training


def test_score_cli_factors_files(frame, tmp_path):
    from factorvae_amd import score

    model = _model()
    ckpt = tmp_path / "m.pt"
    torch.save(model.state_dict(), ckpt)
    data = tmp_path / "d.pkl"
    frame.to_pickle(data)
    base = ["--checkpoint", str(ckpt), "--dataset", str(data), "--run_name",
            "r", "--num_factor", str(K), "--hidden_size", str(H),
            "--num_latent", str(C), "--num_portfolio", str(M),
            "--seq_length", str(T), "--engine", "eager"]
    stem = f"r_{K}_True_False_{C}_{H}"
    score.main(base + ["--out_dir", str(tmp_path / "plain")])
    assert not (tmp_path / "plain" / f"{stem}_factors.csv").exists()
    for out in ("a", "b"):
        score.main(base + ["--out_dir", str(tmp_path / out), "--factors"])
    fa = tmp_path / "a" / f"{stem}_factors.csv"
    da = tmp_path / "a" / f"{stem}_daily.csv"
    # no noise in the files: two runs are byte-identical
    assert fa.read_bytes() == (tmp_path / "b" / fa.name).read_bytes()
    assert da.read_bytes() == (tmp_path / "b" / da.name).read_bytes()

    factors, daily = pd.read_csv(fa), pd.read_csv(da)
    assert list(factors.columns) == ["datetime", "factor", *FACTOR_KEYS]
    assert list(daily.columns) == ["datetime", "n_stocks", "loss", "mse",
                                   "kl"]
    loader = init_data_loader(frame, step_len=T, shuffle=False, start=None,
                              end=None)
    days = [(c[:, :, :-1].float(), c[:, -1, -1].float()) for c, _ in loader]
    dates = sorted(set(str(d) for d, _ in loader.dataset.get_index()))
    assert len(daily) == len(days) > 0 and len(factors) == K * len(days)
    assert [str(pd.Timestamp(d)) for d in daily["datetime"]] == \
        [str(pd.Timestamp(d)) for d in dates]
    assert daily["n_stocks"].tolist() == [x.shape[0] for x, _ in days]
    assert factors["factor"].tolist() == list(range(K)) * len(days)
    model.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))
    dev = next(model.parameters()).device
    for d, (x, y) in enumerate(days):
        n = x.shape[0]
        with torch.no_grad():
            t = model.loss_terms(x.to(dev), y.to(dev).view(n, 1),
                                 eps=torch.zeros(n, 1, device=dev))
        for k in ("loss", "mse", "kl"):
            assert np.float32(daily[k][d]) == np.float32(t[k].item()), (d, k)
        rows = factors.iloc[d * K:(d + 1) * K]
        assert (rows["datetime"] == daily["datetime"][d]).all()
        for k in FACTOR_KEYS:
            assert np.array_equal(rows[k].to_numpy(np.float32),
                                  t[k].cpu().numpy()), (d, k)


def test_train_main_eager_accepts_val_batched(tmp_path):
    from factorvae_amd.engine.trainer import train_main
    from factorvae_amd.main import build_argparser
    from factorvae_amd.utils import DataArgument

    assert build_argparser().parse_args([]).val_batched is False
    assert build_argparser().parse_args(["--val_batched"]).val_batched is True

    class Args:
        num_epochs = 1
        lr = 1e-3
        num_latent = 10
        num_portfolio = 12
        seq_len = 5
        num_factor = 4
        hidden_size = 8
        seed = 42
        run_name = "vb"
        num_workers = 0
        wandb = False
        engine = "eager"
        val_batched = True
        val_metrics = True
        dataset = None

    args = Args()
    args.save_dir = str(tmp_path)
    df = make_synthetic_frame(n_days=40, n_stocks=12, n_features=10, seed=0,
                              start="2015-01-01")
    data_args = DataArgument(
        start_time="2015-01-01", fit_end_time="2015-02-10",
        val_start_time="2015-02-11", val_end_time="2015-02-25",
        end_time="2015-02-25", seq_len=5)
    best = train_main(args, data_args, df=df)
    assert np.isfinite(best)
    recs = [json.loads(line) for line in open(tmp_path / "vb_metrics.jsonl")]
    epoch = [r for r in recs if "Train Loss" in r]
    assert len(epoch) == 1
    assert np.isfinite(epoch[0]["Validation Loss"])
    assert "Validation RankIC" in epoch[0]
