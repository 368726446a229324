"""Predictive mean / risk outputs and multi-day scoring on the eager
(CPU) engine: FactorVAE.prediction_dist, generate_prediction_scores'
batch_days / return_dist / risk_aversion, and the score CLI flags."""

import numpy as np
import pandas as pd
import pytest
import torch

from factorvae_amd.data.sampler import init_data_loader
from factorvae_amd.data.synthetic import make_synthetic_frame
from factorvae_amd.models.modules import build_factorvae
from factorvae_amd.utils import generate_prediction_scores, test_args

C, H, M, K, T = 6, 8, 4, 3, 4


def _model(seed=0):
    torch.manual_seed(seed)
    return build_factorvae(num_latent=C, hidden_size=H, num_portfolio=M,
                           num_factor=K).eval()


@pytest.fixture(scope="module")
def frame():
    # ragged universe: the stock count changes from day to day
    return make_synthetic_frame(n_days=14, n_stocks=9, n_features=C, seed=3,
                                ragged=True)


def _score(frame, **kw):
    loader = init_data_loader(frame, step_len=T, shuffle=False, start=None,
                              end=None)
    args = test_args(run_name="t", num_factor=K, hidden_size=H, num_latent=C,
                     num_portfolio=M, seq_length=T)
    torch.manual_seed(11)
    return generate_prediction_scores(_model(), loader, loader.dataset, args,
                                      engine="eager", **kw)


def test_prediction_is_a_sample_of_prediction_dist():
    model = _model()
    x = torch.randn(13, T, C, generator=torch.Generator().manual_seed(1))
    mu, sigma = model.prediction_dist(x)
    assert mu.shape == sigma.shape == (13, 1)
    assert mu.dtype == sigma.dtype == torch.float32
    assert bool((sigma > 0).all())
    torch.manual_seed(5)
    pred = model.prediction(x)
    torch.manual_seed(5)
    eps = torch.randn_like(sigma)
    assert torch.equal(pred, mu + eps * sigma)


def test_prediction_dist_keeps_the_zero_clamp():
    """A prior sigma of exactly zero enters as 1e-6, as in the decoder's
    forward."""
    model = _model()
    h = torch.randn(5, H, generator=torch.Generator().manual_seed(2))
    fmu = torch.randn(K, generator=torch.Generator().manual_seed(3))
    fsig = torch.tensor([0.0, 0.5, 0.0])
    mu, sigma = model.factor_decoder.dist(h, fmu, fsig)
    mu2, sigma2 = model.factor_decoder.dist(h, fmu,
                                            torch.tensor([1e-6, 0.5, 1e-6]))
    assert torch.equal(mu, mu2) and torch.equal(sigma, sigma2)


def test_scorer_batched_dist_matches_per_day(frame):
    default = _score(frame)
    assert list(default.columns) == ["score"]
    one = _score(frame, batch_days=1, return_dist=True)
    four = _score(frame, batch_days=4, return_dist=True)
    assert list(four.columns) == ["score", "mu", "sigma"]
    assert four.index.equals(default.index)
    assert one.index.equals(default.index)
    assert len(four) > 0
    for col in ("mu", "sigma"):
        assert np.array_equal(four[col].to_numpy(), one[col].to_numpy())
    # same generator state, same draws: the stochastic score is the
    # default scorer's
    assert np.array_equal(one["score"].to_numpy(),
                          default["score"].to_numpy())
    # grouping alone (no dist) keeps the frame
    grouped = _score(frame, batch_days=5)
    pd.testing.assert_frame_equal(grouped, default)


def test_scorer_risk_aversion_is_mu_minus_eta_sigma(frame):
    df = _score(frame, batch_days=4, risk_aversion=0.5)
    assert list(df.columns) == ["score", "mu", "sigma"]
    mu = torch.from_numpy(df["mu"].to_numpy())
    sigma = torch.from_numpy(df["sigma"].to_numpy())
    assert np.array_equal(df["score"].to_numpy(),
                          (mu - 0.5 * sigma).numpy())
    ref = _score(frame, batch_days=1, return_dist=True)
    assert np.array_equal(df["mu"].to_numpy(), ref["mu"].to_numpy())


def test_score_cli_dist_columns(frame, tmp_path):
    from factorvae_amd import score

    ckpt = tmp_path / "m.pt"
    torch.save(_model().state_dict(), ckpt)
    data = tmp_path / "d.pkl"
    frame.to_pickle(data)
    base = ["--checkpoint", str(ckpt), "--dataset", str(data), "--run_name",
            "r", "--num_factor", str(K), "--hidden_size", str(H),
            "--num_latent", str(C), "--num_portfolio", str(M),
            "--seq_length", str(T), "--engine", "eager"]
    name = f"r_{K}_True_False_{C}_{H}.csv"

    score.main(base + ["--out_dir", str(tmp_path / "a")])
    with open(tmp_path / "a" / name) as f:
        assert f.readline().strip() == "datetime,instrument,score"

    score.main(base + ["--out_dir", str(tmp_path / "b"), "--dist",
                       "--risk_aversion", "0.25", "--batch_days", "3"])
    out = pd.read_csv(tmp_path / "b" / name)
    assert list(out.columns) == ["datetime", "instrument", "score", "mu",
                                 "sigma"]
    assert len(out) > 0
    assert np.allclose(out["score"], out["mu"] - 0.25 * out["sigma"],
                       rtol=1e-6, atol=1e-7)
