"""The factor risk model on the device: dec_seg_fwd's svar output, the
risk_seg / risk_solve_seg kernels against factorvae_amd.risk in float64,
and FusedTrainer.risk_many against risk_days_eager, predict_many's
components, its own chunking and the panel route. Outputs start as garbage.

Tolerances. u = 2^-24 is the unit roundoff of float32.

risk_seg is compared with risk.portfolio_risk in float64 fed the very
float32 inputs the kernel read, so only the kernel's arithmetic is under
test. A float32 sum of n rounded products, in any order, differs from the
exact sum by at most e(n, terms) = 2 (n - 1) u sum|terms| to first order
(n - 1 additions and one product rounding per term). For n = 1 that
expression is 0, which no rounded product can meet, so n - 1 is taken as at
least 1. With that (risk_bounds below):
  mean          e(N, w_i mu_i)
  var_specific  e(N, w_i^2 s2_i)
  exposure f_k  df_k = e(N, B_ik w_i)
  factor_var_k  dv_k = 2 |f_k| sz_k^2 df_k + 4 u f_k^2 sz_k^2
                (df through the square; three product roundings)
  var_factor    sum_k dv_k + e(K, factor_var_k)
  mean_factor   sum_k |pmu_k| df_k + e(K, f_k pmu_k)
  vol           (d var_factor + d var_specific) / (2 vol) + 2 u vol
                (through the square root; the addition and the root round)
  mcr_i         g_k = sz_k^2 f_k has dg_k = sz_k^2 df_k + 2 u |g_k|;
                num_i = sum_k B_ik g_k + w_i s2_i has
                dnum_i = sum_k |B_ik| dg_k + e(K + 1, its terms);
                d mcr_i = dnum_i / vol + |num_i| dvol / vol^2 + 2 u |mcr_i|
risk_bounds can add a component tolerance tol on top: every component c is
then taken as known to tol (1 + |c|) (the fused-vs-eager forward tolerance
of test_gpu_predict_batched, 1e-4) and that is pushed through the same
first-order formulas. The engine test compares risk_many with
risk_days_eager under the sum of both.

risk_solve_seg is compared with torch.linalg.solve on the float64 dense
Sigma built from the same inputs. Its tolerance is measured inside the test
from a reference, never from the kernel: 8 x the error risk.solve_cov makes
in float32 on the CPU on the same inputs, relative to max|x_ref|, per
right-hand side, with a floor of 1e-6; the factor 8 covers a different summation order. The float64
residual |Sigma x - b|_inf / |b|_inf is held to the same bound. Against
the eager engine the weights also carry the component tolerance amplified
by the solve, bounded by 4 cond(Sigma) tol (matrix and right-hand side each
perturbed by tol, twice for the normalisation)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from factorvae_amd.ops import get_extension
    ext = get_extension()
from factorvae_amd import risk

DEV = torch.device("cuda:0")
U = 2.0 ** -24
T_, C_, M_ = 5, 10, 8
HK = [(64, 20), (20, 3), (64, 96), (64, 128)]
# a single stock, N < K, an empty day, more rows than threads, full waves
LENS = [1, 37, 0, 257, 64]
TOL = 1e-4  # fused vs eager forward, as test_gpu_predict_batched


def t(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def garbage(shape, seed, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, 12345 + seed, dtype=dtype, device=DEV)
    return t(*shape, seed=seed) + 3.0


def bits(a):
    return a.contiguous().view(torch.int32)


def assert_same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    n = int((bits(a) != bits(b)).sum())
    assert n == 0, f"{what}: {n} of {b.numel()} bit patterns differ"


def seg_tensor(lens):
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    return torch.tensor(offs, dtype=torch.int32, device=DEV)


def offsets(lens):
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    return offs


# ------------------------------------------------------------ the bounds
def e_sum(terms, dim=None):
    """2 max(n - 1, 1) u sum|terms| over dim (all elements if None)."""
    n = terms.numel() if dim is None else terms.shape[dim]
    s = terms.abs().sum() if dim is None else terms.abs().sum(dim)
    return 2.0 * max(n - 1, 1) * U * s


def risk_bounds(comp, w, tol=0.0):
    """Per-quantity error bounds of the module docstring, in float64, for
    the float64 components comp and weights w; tol > 0 adds the
    first-order effect of components known to tol (1 + |c|)."""
    B, s2, mu = comp["beta"], comp["specific_var"], comp["mu"]
    sz, pm = comp["factor_sigma"], comp["factor_mu"]
    N, K = B.shape
    d = lambda c: tol * (1.0 + c.abs())
    r = risk.portfolio_risk(comp, w)
    f, vol = r["exposure"], r["vol"]
    bd = {"mean": e_sum(w * mu) + (w.abs() * d(mu)).sum(),
          "var_specific": e_sum(w * w * s2) + (w * w * d(s2)).sum()}
    df = e_sum(B * w[:, None], 0) + (w.abs()[:, None] * d(B)).sum(0)
    bd["exposure"] = df
    bd["factor_var"] = (2 * f.abs() * sz ** 2 * df + 4 * U * r["factor_var"]
                        + 2 * f ** 2 * sz * d(sz))
    bd["var_factor"] = bd["factor_var"].sum() + e_sum(r["factor_var"])
    bd["mean_factor"] = ((pm.abs() * df).sum() + e_sum(f * pm)
                         + (f.abs() * d(pm)).sum())
    dvol = ((bd["var_factor"] + bd["var_specific"]) / (2 * vol)
            + 2 * U * vol)
    bd["vol"] = dvol
    g = sz ** 2 * f
    dg = sz ** 2 * df + 2 * U * g.abs() + 2 * sz * d(sz) * f.abs()
    terms = torch.cat([B * g, (w * s2)[:, None]], dim=1)
    num = terms.sum(1)
    dnum = ((B.abs() * dg).sum(1) + e_sum(terms, 1)
            + (d(B) * g.abs()).sum(1) + w.abs() * d(s2))
    bd["mcr"] = (dnum / vol + num.abs() * dvol / vol ** 2
                 + 2 * U * r["mcr"].abs())
    return r, bd


def check_risk(got, comp, w, what, tol=0.0, ref=None):
    """got: float32 results of one day; comp, w: float64 inputs of the
    bounds; ref: the values to compare with (default: the float64 oracle
    on comp)."""
    r, bd = risk_bounds(comp, w, tol)
    ref = r if ref is None else ref
    for k in bd:
        err = (got[k].double().cpu() - ref[k].double().cpu()).abs()
        over = err - bd[k].cpu()
        print(f"{what} {k}: max err {float(err.max()):.3e} "
              f"bound {float(bd[k].max()):.3e}")
        assert bool((over <= 0).all()), (what, k, float(err.max()),
                                         float(bd[k].max()))


# --------------------------------------------------------- packed inputs
def packed_inputs(K, lens, seed):
    """Random float32 components of the packed days, on the device, with
    the scales the model gives them: those of a randomly initialised
    FactorVAE on random days (eager, on the CPU), and random weights.
    (Uniformly random variances spread over a factor of 25 make the
    residual check meaningless: risk.solve_cov's own float32 residual is
    then up to 100 x its error, measured on the CPU.)"""
    from factorvae_amd.models.modules import build_factorvae

    torch.manual_seed(seed)
    H = 20 if K < 20 else 64
    model = build_factorvae(num_latent=C_, hidden_size=H, num_portfolio=M_,
                            num_factor=K).eval()
    g = torch.Generator(device="cpu").manual_seed(seed)
    N, D = sum(lens), len(lens)
    i = {"beta": torch.zeros(N, K), "svar": torch.ones(N),
         "mu": torch.zeros(N), "pmu": torch.zeros(D, K),
         "psig_c": torch.ones(D, K)}
    o = 0
    for d, n in enumerate(lens):
        if n:
            c = model.risk_model(torch.randn(n, T_, C_, generator=g))
            i["beta"][o:o + n], i["svar"][o:o + n] = c["beta"], c["specific_var"]
            i["mu"][o:o + n] = c["mu"]
            i["pmu"][d], i["psig_c"][d] = c["factor_mu"], c["factor_sigma"]
        o += n
    i = {k: v.to(DEV) for k, v in i.items()}
    i["w"] = t(N, seed=seed + 3, scale=0.1)
    return i


def day_comp(i, d, o, n, dtype=torch.float64, device="cpu"):
    c = {"beta": i["beta"][o:o + n], "specific_var": i["svar"][o:o + n],
         "mu": i["mu"][o:o + n], "factor_mu": i["pmu"][d],
         "factor_sigma": i["psig_c"][d]}
    return {k: v.to(device=device, dtype=dtype) for k, v in c.items()}


def run_risk_seg(i, lens, seed):
    N, D, K = sum(lens), len(lens), i["beta"].size(1)
    o = {"stats": garbage((D, 5), seed), "exposure": garbage((D, K), seed + 1),
         "factor_var": garbage((D, K), seed + 2), "mcr": garbage((N,), seed + 3)}
    ext.risk_seg(i["beta"], i["svar"], i["mu"], i["w"], seg_tensor(lens),
                 i["pmu"], i["psig_c"], o["stats"], o["exposure"],
                 o["factor_var"], o["mcr"])
    torch.cuda.synchronize()
    return o


def run_solve(i, lens, b, seed, norms=True):
    N, D, R = sum(lens), len(lens), b.size(1)
    o = {"x": garbage((N, R), seed), "info": garbage((D,), seed, torch.int32),
         "norms": garbage((D, 2, R), seed + 1)}
    ext.risk_solve_seg(i["beta"], i["svar"], seg_tensor(lens), i["psig_c"],
                       b, o["x"], o["info"], o["norms"] if norms else None)
    torch.cuda.synchronize()
    return o


def stats_of(o, d, a, n):
    got = {k: o["stats"][d, j] for j, k in enumerate(risk.STAT_KEYS)}
    got["exposure"], got["factor_var"] = o["exposure"][d], o["factor_var"][d]
    got["mcr"] = o["mcr"][a:a + n]
    return got


# ------------------------------------------------------------- decoder
def dec_weights(H, K):
    from factorvae_amd.models.modules import build_factorvae

    torch.manual_seed(4)
    model = build_factorvae(num_latent=C_, hidden_size=H, num_portfolio=M_,
                            num_factor=K).to(DEV)
    dec = model.factor_decoder
    al = dec.alpha_layer
    wt = [al.linear1.weight, al.linear1.bias, al.mu_layer.weight,
          al.mu_layer.bias, al.sigma_layer.weight, al.sigma_layer.bias,
          dec.beta_layer.linear1.weight, dec.beta_layer.linear1.bias]
    return dec, [w.detach().contiguous() for w in wt]


@pytest.mark.parametrize("H,K", HK)
def test_dec_seg_svar_output(H, K):
    dec, wt = dec_weights(H, K)
    N, D = sum(LENS), len(LENS)
    h, eps = t(N, H, seed=31), t(N, seed=32)
    fmu = t(D, K, seed=33)
    fsig = t(D, K, seed=34).abs() + 0.1

    def run(seed, svar):
        o = {"mu": garbage((N,), seed), "sigma": garbage((N,), seed + 1),
             "sample": garbage((N,), seed + 2),
             "beta": garbage((N, K), seed + 3)}
        # the positional form of test_gpu_predict_batched, then svar
        ext.dec_seg_fwd(h, seg_tensor(LENS), *wt, fmu, fsig, eps, o["mu"],
                        o["sigma"], o["sample"], o["beta"], *svar)
        return o

    plain = run(400, ())
    sv = garbage((N,), 410)
    with_sv = run(400, (sv,))
    kw = garbage((N,), 411)
    ext.dec_seg_fwd(h, seg_tensor(LENS), *wt, fmu, fsig, None,
                    garbage((N,), 1), garbage((N,), 2), svar=kw)
    torch.cuda.synchronize()
    for k in plain:
        assert_same_bits(with_sv[k], plain[k], k)
    assert_same_bits(kw, sv, "svar by keyword, without eps and beta")
    # the per-day decoder's asig_pre is this kernel's (its sigma has the same
    # bits, test_gpu_predict_batched), so torch's softplus of it isolates
    # the arithmetic behind svar
    pre = garbage((N,), 420)
    ext.dec_fwd(h, *wt, fmu[0], fsig[0], eps, garbage((N,), 421),
                garbage((N, H), 422), garbage((N, K), 423), pre,
                garbage((N,), 424))
    torch.cuda.synchronize()
    a64 = torch.nn.functional.softplus(pre.double())
    ref = (a64 ** 2 + 1e-6).float()
    with torch.no_grad():
        _, asig_e = dec.alpha_layer(h)
    assert torch.allclose(sv, asig_e.view(-1) ** 2 + 1e-6, atol=TOL, rtol=TOL)
    # 4 ulp of the float32 result
    ulp = torch.abs(torch.nextafter(ref, ref * 2) - ref)
    err = (sv - ref).abs()
    print(f"svar: max err {float((err / ulp).max()):.2f} ulp")
    assert bool((err <= 4 * ulp).all())
    # and it is not sigma^2 minus the factor part
    assert bool((sv > 0).all())


# ------------------------------------------------------------ risk_seg
@pytest.mark.parametrize("K", [k for _, k in HK])
def test_risk_seg_against_float64(K):
    i = packed_inputs(K, LENS, seed=100 + K)
    o = run_risk_seg(i, LENS, 500)
    offs = offsets(LENS)
    for d, n in enumerate(LENS):
        a = offs[d]
        if n == 0:
            assert bool(torch.isnan(o["stats"][d]).all())
            assert bool(torch.isnan(o["exposure"][d]).all())
            assert bool(torch.isnan(o["factor_var"][d]).all())
            continue
        comp = day_comp(i, d, a, n)
        w = i["w"][a:a + n].double().cpu()
        check_risk(stats_of(o, d, a, n), comp, w, f"K={K} N={n}")
        # sum_i w_i mcr_i = vol
        wm = w * o["mcr"][a:a + n].double().cpu()
        assert abs(float(wm.sum()) - float(o["stats"][d, 4])) <= \
            1e-5 * float(wm.abs().sum())


def test_risk_seg_zero_portfolio_and_batch_invariance():
    K = 20
    i = packed_inputs(K, LENS, seed=7)
    i["w"][1:38] = 0.0  # day 1: vol = 0 -> mcr NaN
    o = run_risk_seg(i, LENS, 510)
    assert float(o["stats"][1, 4]) == 0.0
    assert bool(torch.isnan(o["mcr"][1:38]).all())
    assert bool(torch.isfinite(o["mcr"][38:]).all())
    # every day alone: the same bits as in the pack
    offs = offsets(LENS)
    for d, n in enumerate(LENS):
        if n == 0:
            continue
        a = offs[d]
        one = {k: (v[d:d + 1] if k in ("pmu", "psig_c") else v[a:a + n])
               .contiguous() for k, v in i.items()}
        alone = run_risk_seg(one, [n], 520)
        assert_same_bits(alone["stats"][0], o["stats"][d], f"stats {d}")
        assert_same_bits(alone["exposure"][0], o["exposure"][d], f"f {d}")
        assert_same_bits(alone["mcr"], o["mcr"][a:a + n], f"mcr {d}")


# ------------------------------------------------------ risk_solve_seg
def solve_reference(comp64, b64):
    """(cov, x_ref, tolerance, cpu error) of one right-hand side b64 (n,):
    the float64 dense solve, and 8 x the relative error of risk.solve_cov
    in float32 on the CPU on the same inputs (floor 1e-6)."""
    cov = risk.dense_cov(comp64)
    ref = torch.linalg.solve(cov, b64)
    c32 = {k: v.float() for k, v in comp64.items()}
    x32 = risk.solve_cov(c32, b64.float()).double()
    cpu_err = float((x32 - ref).abs().max() / ref.abs().max())
    return cov, ref, max(8.0 * cpu_err, 1e-6), cpu_err


@pytest.mark.parametrize("K", [k for _, k in HK])
@pytest.mark.parametrize("R", [1, 2, 4])
def test_risk_solve_seg_against_dense_float64(K, R):
    """Right-hand sides: the two risk_many solves for, b = 1 and b = mu,
    and for R = 4 two combinations of them of comparable size,
    1 +- 10 mu. Every column is held to its own reference error and its
    own residual: the columns differ in scale, and a tolerance pooled over
    them would be set by the largest one. (Generic random right-hand sides
    are no use for the residual check: x is then b / s2 to within 1e-7 and
    the residual, amplified by |Sigma|, is up to 29 x the error for
    risk.solve_cov in float32 on the CPU itself; for the columns used here
    that ratio is 0.1 to 3.6 on these inputs.)"""
    i = packed_inputs(K, LENS, seed=200 + K)
    N = sum(LENS)
    one, mu = torch.ones(N, 1, device=DEV), i["mu"][:, None]
    b = torch.cat([one, mu, one + 10 * mu, one - 10 * mu],
                  dim=1)[:, :R].contiguous()
    o = run_solve(i, LENS, b, 600)
    offs = offsets(LENS)
    for d, n in enumerate(LENS):
        a = offs[d]
        if n == 0:
            assert int(o["info"][d]) == 0
            assert bool(torch.isnan(o["norms"][d]).all())
            continue
        assert int(o["info"][d]) == 0, (K, n)
        comp = day_comp(i, d, a, n)
        x = o["x"][a:a + n].double().cpu()
        for c in range(R):
            b64 = b[a:a + n, c].double().cpu()
            cov, ref, tol, cpu_err = solve_reference(comp, b64)
            err = float((x[:, c] - ref).abs().max() / ref.abs().max())
            res = float((cov @ x[:, c] - b64).abs().max() / b64.abs().max())
            print(f"solve K={K} N={n} R={R} col {c}: cpu fp32 err "
                  f"{cpu_err:.2e} tol {tol:.2e} kernel err {err:.2e} "
                  f"residual {res:.2e}")
            assert err <= tol, (K, n, R, c, err, tol)
            assert res <= tol, (K, n, R, c, res, tol)
        nm = o["norms"][d].double().cpu()
        assert torch.allclose(nm[0], x.sum(0), rtol=1e-5,
                              atol=1e-5 * float(x.abs().sum(0).max()))
        assert torch.allclose(nm[1], x.abs().sum(0), rtol=1e-5, atol=0)
    bare = run_solve(i, LENS, b, 600, norms=False)
    assert_same_bits(bare["x"], o["x"], "x without norms")


def test_risk_solve_seg_isolates_a_failed_day():
    """A NaN in one day's svar (data, not a fault): that day reports
    info = 1 and NaN x, the others keep the bits of a run without it."""
    K = 20
    lens = [37, 64, 5]
    i = packed_inputs(K, lens, seed=11)
    b = torch.ones(sum(lens), 2, device=DEV)
    b[:, 1] = i["mu"]
    good = run_solve(i, lens, b, 700)
    bad_in = dict(i, svar=i["svar"].clone())
    bad_in["svar"][37 + 10] = float("nan")
    bad = run_solve(bad_in, lens, b, 700)
    assert bad["info"].tolist() == [0, 1, 0]
    assert good["info"].tolist() == [0, 0, 0]
    assert bool(torch.isnan(bad["x"][37:101]).all())
    assert_same_bits(bad["x"][:37], good["x"][:37], "day 0")
    assert_same_bits(bad["x"][101:], good["x"][101:], "day 2")
    # without the failed day at all
    keep = torch.cat([torch.arange(37), torch.arange(101, 106)]).to(DEV)
    two = {k: (v[[0, 2]] if k in ("pmu", "psig_c") else v[keep]).contiguous()
           for k, v in i.items()}
    alone = run_solve(two, [37, 5], b[keep].contiguous(), 710)
    assert_same_bits(alone["x"], bad["x"][keep], "days 0 and 2 alone")
    assert_same_bits(alone["norms"], bad["norms"][[0, 2]], "norms")


def test_binding_checks():
    """Wrong dtype, short seg_off, R = 5 and K = 129 are refused on the
    host, with an exception and no launch."""
    K, lens = 4, [3, 2]
    i = packed_inputs(K, lens, seed=1)
    N, D = 5, 2
    seg = seg_tensor(lens)
    outs = lambda: (garbage((D, 5), 1), garbage((D, K), 2),
                    garbage((D, K), 3), garbage((N,), 4))

    def rs(**kw):
        a = dict(i, seg_off=seg)
        a.update(kw)
        ext.risk_seg(a["beta"], a["svar"], a["mu"], a["w"], a["seg_off"],
                     a["pmu"], a["psig_c"], *outs())

    def sv(b=None, **kw):
        a = dict(i, seg_off=seg)
        a.update(kw)
        b = torch.ones(N, 1, device=DEV) if b is None else b
        ext.risk_solve_seg(a["beta"], a["svar"], a["seg_off"], a["psig_c"], b,
                           garbage(tuple(b.shape), 5),
                           garbage((D,), 6, torch.int32), None)

    rs()
    sv()
    for call in (rs, sv):
        with pytest.raises(RuntimeError, match="svar"):
            call(svar=i["svar"].double())
        with pytest.raises(RuntimeError, match="seg_off"):
            call(seg_off=seg[:D])
        with pytest.raises(RuntimeError, match="seg_off"):
            call(seg_off=seg.long())
        with pytest.raises(RuntimeError, match="K <= 128"):
            call(beta=t(N, 129), pmu=t(D, 129), psig_c=t(D, 129).abs())
    with pytest.raises(RuntimeError, match="R <= 4"):
        sv(b=torch.ones(N, 5, device=DEV))
    with pytest.raises(RuntimeError, match="info"):
        ext.risk_solve_seg(i["beta"], i["svar"], seg, i["psig_c"],
                           torch.ones(N, 1, device=DEV), garbage((N, 1), 5),
                           garbage((D,), 6), None)
    torch.cuda.synchronize()


# --------------------------------------------------- through the engine
def _trainer(H, K, dtype="fp32", seed=0):
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    set_seed(seed)
    model = build_factorvae(num_latent=C_, hidden_size=H, num_portfolio=M_,
                            num_factor=K).to(DEV)
    return FusedTrainer(model, lr=1e-3, t_max=100, device=DEV,
                        use_graph=False, train=False, dtype=dtype)


def _days(lens, seed=0):
    xs = [t(n, T_, C_, seed=seed + i) for i, n in enumerate(lens)]
    ws = [t(n, seed=seed + 100 + i, scale=0.1) for i, n in enumerate(lens)]
    return xs, ws


def own_comp(r, d, dtype=torch.float64):
    return {"mu": r["mu"][d].to(dtype), "beta": r["beta"][d].to(dtype),
            "specific_var": r["specific_var"][d].to(dtype),
            "factor_mu": r["factor_mu"][d].to(dtype),
            "factor_sigma": r["factor_sigma"][d].to(dtype)}


def assert_same_result(a, b, what, order=None):
    order = list(range(len(a["n"]))) if order is None else order
    for k, v in a.items():
        for i, j in enumerate(order):
            x, y = v[i], b[k][j]
            if x.numel() == 0:
                assert y.numel() == 0, (what, k, i)
            elif x.dtype == torch.int32:
                assert torch.equal(x, y), (what, k, i)
            else:
                assert_same_bits(x, y, f"{what} {k} day {i}")


@pytest.mark.parametrize("H,K", HK)
def test_risk_many_against_eager_and_float64(H, K):
    tr = _trainer(H, K)
    xs, ws = _days(LENS, seed=200)
    state = torch.cuda.get_rng_state()
    cpu_state = torch.random.get_rng_state()
    r = tr.risk_many(xs, weights=ws, solve=("minvar", "mv"),
                     return_components=True)
    assert torch.equal(torch.cuda.get_rng_state(), state)
    assert torch.equal(torch.random.get_rng_state(), cpu_state)
    e = risk.risk_days_eager(tr.model, xs, weights=ws,
                             solve=("minvar", "mv"), return_components=True)
    assert r["n"].tolist() == LENS and r["n"].dtype == torch.int32
    assert r["solve_info"].tolist() == [0] * len(LENS)
    assert set(r) == set(e)
    for k in e:
        if isinstance(e[k], list):
            assert [tuple(v.shape) for v in r[k]] == \
                [tuple(v.shape) for v in e[k]], k
        else:
            assert r[k].shape == e[k].shape and r[k].dtype == e[k].dtype, k
    # the components are predict_many's, bit for bit
    pm = tr.predict_many(xs, return_dist=True, return_beta=True)
    for d, n in enumerate(LENS):
        if n == 0:
            for k in risk.STAT_KEYS + ("exposure", "factor_var", "factor_mu",
                                       "factor_sigma"):
                assert bool(torch.isnan(r[k][d]).all()), k
            continue
        assert_same_bits(r["mu"][d], pm[d][1].view(-1).cpu(), "mu")
        assert_same_bits(r["beta"][d], pm[d][3].cpu(), "beta")
        for k in ("mu", "beta", "specific_var", "factor_mu", "factor_sigma"):
            assert torch.allclose(r[k][d], e[k][d], atol=TOL, rtol=TOL), k
        sig2 = (r["beta"][d].double() ** 2
                @ r["factor_sigma"][d].double() ** 2
                + r["specific_var"][d].double())
        assert torch.allclose(sig2.sqrt().float(), pm[d][2].view(-1).cpu(),
                              rtol=TOL, atol=0)
        got = {k: r[k][d] for k in risk.STAT_KEYS + ("exposure", "factor_var",
                                                     "mcr")}
        comp = own_comp(r, d)
        w = ws[d].double().cpu()
        # the kernel's arithmetic on its own components
        check_risk(got, comp, w, f"own H={H} K={K} N={n}")
        # against the eager engine: plus the component tolerance
        check_risk(got, comp, w, f"eager H={H} K={K} N={n}", tol=TOL,
                   ref={k: e[k][d] for k in got})
        # the weights against the float64 dense solve on the same components
        cov = risk.dense_cov(comp)
        cond = float(torch.linalg.cond(cov))
        for which, fn in (("minvar", risk.minvar_weights),
                          ("mv", risk.mv_weights)):
            ref = fn(comp)
            c32 = {k: v.float() for k, v in comp.items()}
            cpu_err = float((fn(c32).double() - ref).abs().max()
                            / ref.abs().max())
            tol = max(8.0 * cpu_err, 1e-6)
            err = float((r[which][d].double() - ref).abs().max()
                        / ref.abs().max())
            err_e = float((r[which][d].double() - e[which][d].double())
                          .abs().max() / ref.abs().max())
            print(f"{which} H={H} K={K} N={n}: cpu fp32 err {cpu_err:.2e} "
                  f"tol {tol:.2e} err {err:.2e} vs eager {err_e:.2e} "
                  f"cond {cond:.1f}")
            assert err <= tol, (which, n, err, tol)
            assert err_e <= tol + 4.0 * cond * TOL, (which, n, err_e)
    # equal weights by default
    eq = tr.risk_many(xs)
    assert set(eq) == {"n", "mcr", "exposure", "factor_var", *risk.STAT_KEYS}
    ones = [torch.full((n,), 1.0 / n if n else 0.0) for n in LENS]
    assert_same_result(eq, tr.risk_many(xs, weights=ones), "equal weights")
    with pytest.raises(ValueError):
        tr.risk_many(xs, weights=ws[:3])
    with pytest.raises(ValueError):
        tr.risk_many(xs, weights=[ws[1]] * len(xs))
    with pytest.raises(ValueError):
        tr.risk_many(xs, solve=("maxvar",))


@pytest.mark.parametrize("H,K", HK)
def test_risk_many_chunks_and_order(H, K):
    tr = _trainer(H, K)
    xs, ws = _days(LENS, seed=300)
    kw = dict(solve=("minvar", "mv"), return_components=True)
    one = tr.risk_many(xs, weights=ws, **kw)
    # every day its own chunk
    split = tr.risk_many(xs, weights=ws, max_rows=1, **kw)
    assert_same_result(one, split, "one day per chunk")
    # host inputs, reversed order
    rev = tr.risk_many([x.cpu() for x in xs[::-1]],
                       weights=[w.cpu() for w in ws[::-1]], **kw)
    D = len(xs)
    assert_same_result(one, rev, "reversed", order=list(range(D))[::-1])


def make_panel():
    """Ragged days on consecutive dates of a full (date, stock) table."""
    from factorvae_amd.data.panel import PanelDays

    S = 300
    n_dates = len(LENS) + T_ - 1
    g = torch.Generator(device="cpu").manual_seed(3)
    rows = torch.randn(n_dates * S, C_, generator=g)
    ids = []
    for d, n in enumerate(LENS):
        stocks = torch.randperm(S, generator=g)[:n].sort().values
        dates = torch.arange(d, d + T_)
        ids.append((dates[None, :] * S + stocks[:, None]).to(torch.int32)
                   .reshape(n, T_))
    return PanelDays(rows, ids)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_risk_many_panel_and_bf16(dtype):
    """The panel route gives the bits of its windows(); the bf16 engine
    runs and its components are its own predict_many's."""
    tr = _trainer(64, 20, dtype=dtype)
    panel = make_panel().to(DEV)
    days = [panel.windows(d)[0] for d in range(len(panel))]
    kw = dict(solve=("minvar", "mv"), return_components=True)
    a = tr.risk_many(panel, **kw)
    b = tr.risk_many(days, **kw)
    assert_same_result(a, b, f"panel {dtype}")
    pm = tr.predict_many(days, return_dist=True, return_beta=True)
    for d, n in enumerate(LENS):
        if n:
            assert_same_bits(b["mu"][d], pm[d][1].view(-1).cpu(), "mu")
            assert_same_bits(b["beta"][d], pm[d][3].cpu(), "beta")
    assert b["solve_info"].tolist() == [0] * len(LENS)
    assert bool(torch.isfinite(b["vol"][[0, 1, 3, 4]]).all())


def test_fp8_engine_is_refused():
    tr = _trainer(64, 20, dtype="fp8")
    xs, _ = _days([5], seed=700)
    with pytest.raises(ValueError, match="fp8"):
        tr.risk_many(xs)
