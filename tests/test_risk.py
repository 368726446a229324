"""The factor risk model on the eager engine: FactorVAE.risk_model, the
plain-torch functions of factorvae_amd.risk against the dense covariance
in float64, risk_days_eager over ragged days and the score CLI's --risk /
--risk_weights files."""

import pandas as pd
import pytest
import torch

from factorvae_amd import risk
from factorvae_amd.data.sampler import init_data_loader
from factorvae_amd.data.synthetic import make_synthetic_frame
from factorvae_amd.models.modules import build_factorvae

# (N, H, K); the last has fewer stocks than factors
SHAPES = [(1, 20, 3), (37, 64, 20), (257, 64, 96), (40, 64, 128)]
C_, T_ = 10, 5


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "N%d_H%d_K%d" % s)
def case(request):
    """(float64 model, x, float64 components, dense Sigma, w) of one shape,
    computed once."""
    N, H, K = request.param
    torch.manual_seed(N + K)
    model = build_factorvae(num_latent=C_, hidden_size=H, num_portfolio=16,
                            num_factor=K).double().eval()
    x = torch.randn(N, T_, C_, dtype=torch.float64)
    comp = model.risk_model(x)
    w = torch.randn(N, dtype=torch.float64) / N
    return model, x, comp, risk.dense_cov(comp), w


def test_risk_model_components(case):
    model, x, comp, cov, _ = case
    N, K = comp["beta"].shape
    assert set(comp) == set(risk.COMPONENT_KEYS)
    assert comp["mu"].shape == comp["specific_var"].shape == (N,)
    assert comp["factor_mu"].shape == comp["factor_sigma"].shape == (K,)
    mu, sigma = model.prediction_dist(x)
    # the diagonal is the predictive variance, to float32 rounding
    assert torch.allclose(cov.diagonal(), sigma.view(-1) ** 2, rtol=1e-6,
                          atol=0)
    assert torch.allclose(comp["mu"], mu.view(-1), rtol=1e-6, atol=1e-9)
    h = model.feature_extractor(x)
    _, asig = model.factor_decoder.alpha_layer(h)
    assert torch.equal(comp["specific_var"], asig.view(-1) ** 2 + 1e-6)
    assert bool((comp["factor_sigma"] > 0).all())


def test_portfolio_risk_is_the_dense_quadratic_form(case):
    _, _, comp, cov, w = case
    r = risk.portfolio_risk(comp, w)
    rt = dict(rtol=1e-10, atol=0)
    var = w @ cov @ w
    assert torch.allclose(r["var_factor"] + r["var_specific"], var, **rt)
    assert torch.allclose(r["vol"], var.sqrt(), **rt)
    assert torch.allclose(r["mcr"], cov @ w / var.sqrt(), rtol=1e-10,
                          atol=1e-10 * float((cov @ w).abs().max()
                                             / var.sqrt()))
    assert torch.allclose((w * r["mcr"]).sum(), r["vol"], **rt)
    assert torch.allclose(r["mean"], w @ comp["mu"], **rt)
    f = comp["beta"].t() @ w
    assert torch.allclose(r["exposure"], f, rtol=1e-10, atol=1e-300)
    assert torch.allclose(r["mean_factor"], f @ comp["factor_mu"], **rt)
    assert torch.allclose(r["factor_var"],
                          (f * comp["factor_sigma"]) ** 2, **rt)
    assert torch.allclose(r["var_factor"], r["factor_var"].sum(), **rt)
    assert torch.allclose(r["var_specific"],
                          (w * w * comp["specific_var"]).sum(), **rt)
    zero = risk.portfolio_risk(comp, torch.zeros_like(w))
    assert float(zero["vol"]) == 0.0 and bool(zero["mcr"].isnan().all())


def test_solve_cov_matches_the_dense_solve(case):
    _, _, comp, cov, _ = case
    N = cov.shape[0]
    g = torch.Generator().manual_seed(5)
    b = torch.randn(N, 3, dtype=torch.float64, generator=g)
    ref = torch.linalg.solve(cov, b)
    x = risk.solve_cov(comp, b)
    assert x.shape == (N, 3)
    err = float((x - ref).abs().max() / ref.abs().max())
    assert err <= 1e-10, err
    x1 = risk.solve_cov(comp, b[:, 0])
    assert x1.shape == (N,)
    assert float((x1 - ref[:, 0]).abs().max() / ref.abs().max()) <= 1e-10


def test_minvar_and_mv_weights(case):
    _, _, comp, cov, _ = case
    wm = risk.minvar_weights(comp)
    assert abs(float(wm.sum()) - 1.0) <= 1e-12
    # stationary point of w' Sigma w on sum w = 1: Sigma w is constant
    g = cov @ wm
    assert float((g - g.mean()).abs().max() / g.abs().max()) <= 1e-9
    wv = risk.mv_weights(comp)
    assert abs(float(wv.abs().sum()) - 1.0) <= 1e-12
    d = torch.linalg.solve(cov, comp["mu"])
    assert torch.allclose(wv, d / d.abs().sum(), rtol=1e-8, atol=1e-12)
    flat = dict(comp, mu=torch.zeros_like(comp["mu"]))
    assert bool((risk.mv_weights(flat) == 0).all())


# ---------------------------------------------------------- ragged days
H, K, M = 8, 3, 4


def _model(seed=0):
    torch.manual_seed(seed)
    return build_factorvae(num_latent=C_, hidden_size=H, num_portfolio=M,
                           num_factor=K).eval()


def test_risk_days_eager_layout_empty_day_and_errors():
    model = _model()
    lens = [5, 0, 1, 11]
    g = torch.Generator().manual_seed(1)
    days = [torch.randn(n, T_, C_, generator=g) for n in lens]
    ws = [torch.randn(n, generator=g) for n in lens]
    state = torch.random.get_rng_state()
    r = risk.risk_days_eager(model, days, weights=ws,
                             solve=("minvar", "mv"), return_components=True)
    assert torch.equal(torch.random.get_rng_state(), state)
    assert r["n"].tolist() == lens and r["n"].dtype == torch.int32
    for k in risk.STAT_KEYS:
        assert r[k].shape == (4,) and r[k].dtype == torch.float32
    assert r["exposure"].shape == r["factor_var"].shape == (4, K)
    assert r["factor_mu"].shape == r["factor_sigma"].shape == (4, K)
    assert r["solve_info"].tolist() == [0, 0, 0, 0]
    for k in ("mcr", "minvar", "mv", "mu", "specific_var"):
        assert [t.shape for t in r[k]] == [(n,) for n in lens], k
    assert [t.shape for t in r["beta"]] == [(n, K) for n in lens]
    for d, n in enumerate(lens):
        if n == 0:
            for k in risk.STAT_KEYS + ("exposure", "factor_var", "factor_mu",
                                       "factor_sigma"):
                assert bool(torch.isnan(r[k][d]).all()), k
            continue
        comp = model.risk_model(days[d])
        p = risk.portfolio_risk(comp, ws[d])
        for k in risk.STAT_KEYS:
            assert torch.equal(r[k][d], p[k]), (d, k)
        assert torch.equal(r["mcr"][d], p["mcr"])
        assert torch.equal(r["minvar"][d], risk.minvar_weights(comp))
        assert torch.equal(r["mv"][d], risk.mv_weights(comp))
        assert torch.equal(r["beta"][d], comp["beta"])
    # equal weights by default
    eq = risk.risk_days_eager(model, days)
    assert set(eq) == {"n", "mcr", "exposure", "factor_var", *risk.STAT_KEYS}
    p = risk.portfolio_risk(model.risk_model(days[3]),
                            torch.full((11,), 1.0 / 11))
    assert torch.equal(eq["vol"][3], p["vol"])
    with pytest.raises(ValueError):
        risk.risk_days_eager(model, days, weights=ws[:3])
    with pytest.raises(ValueError):
        risk.risk_days_eager(model, days, weights=[ws[0]] * 4)
    with pytest.raises(ValueError):
        risk.risk_days_eager(model, days, solve=("maxvar",))
    assert not model.training


def test_score_cli_risk_files(tmp_path):
    from factorvae_amd import score

    frame = make_synthetic_frame(n_days=12, n_stocks=9, n_features=C_, seed=3,
                                 ragged=True)
    model = _model()
    ckpt = tmp_path / "m.pt"
    torch.save(model.state_dict(), ckpt)
    data = tmp_path / "d.pkl"
    frame.to_pickle(data)
    base = ["--checkpoint", str(ckpt), "--dataset", str(data), "--run_name",
            "r", "--num_factor", str(K), "--hidden_size", str(H),
            "--num_latent", str(C_), "--num_portfolio", str(M),
            "--seq_length", str(T_), "--engine", "eager", "--topk", "3"]
    stem = f"r_{K}_True_False_{C_}_{H}"
    with pytest.raises(SystemExit):   # --risk needs --dist
        score.main(base + ["--out_dir", str(tmp_path / "x"), "--risk"])
    score.main(base + ["--out_dir", str(tmp_path / "plain"), "--dist"])
    assert not (tmp_path / "plain" / f"{stem}_risk.csv").exists()
    scores = score.main(base + ["--out_dir", str(tmp_path / "a"), "--dist",
                                "--risk"])
    assert not (tmp_path / "a" / f"{stem}_weights.csv").exists()
    rk = pd.read_csv(tmp_path / "a" / f"{stem}_risk.csv")
    fc = pd.read_csv(tmp_path / "a" / f"{stem}_risk_factors.csv")
    assert list(rk.columns) == ["datetime", "n_stocks", "mean", "mean_factor",
                                "var_factor", "var_specific", "vol"]
    assert list(fc.columns) == ["datetime", "factor", "exposure",
                                "factor_var"]
    loader = init_data_loader(frame, step_len=T_, shuffle=False, start=None,
                              end=None)
    days = [c[:, :, :-1].float() for c, _ in loader]
    assert len(rk) == len(days) > 0 and len(fc) == K * len(days)
    assert rk["n_stocks"].tolist() == [x.shape[0] for x in days]
    assert fc["factor"].tolist() == list(range(K)) * len(days)
    # the portfolio: equal weight on the 3 largest predictive means
    model.to(torch.device("cuda" if torch.cuda.is_available() else "cpu"))
    dev = next(model.parameters()).device
    mu = torch.as_tensor(scores["mu"].to_numpy())
    row = 0
    for d, x in enumerate(days):
        n = x.shape[0]
        k = min(3, n)
        w = torch.zeros(n)
        w[torch.topk(mu[row:row + n], k).indices] = 1.0 / k
        p = risk.portfolio_risk(model.risk_model(x.to(dev)), w.to(dev))
        assert abs(rk["vol"][d] - float(p["vol"])) <= 1e-6 * float(p["vol"])
        assert abs(rk["mean"][d] - float(p["mean"])) <= 1e-6
        row += n
    for which in ("minvar", "mv"):
        out = tmp_path / which
        score.main(base + ["--out_dir", str(out), "--dist", "--risk",
                           "--risk_weights", which, "--panel"])
        wd = pd.read_csv(out / f"{stem}_weights.csv")
        assert list(wd.columns) == ["datetime", "instrument", "weight"]
        assert len(wd) == sum(x.shape[0] for x in days)
        per_day = wd.groupby("datetime", sort=False)["weight"]
        tot = per_day.sum() if which == "minvar" else per_day.apply(
            lambda s: s.abs().sum())
        assert len(tot) == len(days)
        assert ((tot - 1.0).abs() < 1e-4).all()
        assert len(pd.read_csv(out / f"{stem}_risk.csv")) == len(days)
