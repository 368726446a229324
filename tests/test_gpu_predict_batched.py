"""Batched multi-day scoring: the segmented prior-attention and decoder
kernels, the GRU forward without backward state, FusedTrainer.predict_many
and the scorer's batch_days path — against the per-day kernels / per-day
predict (bit patterns where the arithmetic order is the same) and the
eager module (1e-4, the forward tolerance of test_full_step_grad_parity)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from factorvae_amd.ops import get_extension
    ext = get_extension()
DEV = torch.device("cuda:0")
KEEP_INV = 1.0 / (1.0 - 0.1)
HK = [(20, 3), (64, 20)]
T_, C_, M_ = 4, 24, 8
TOL = 1e-4


def t(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def garbage(shape, seed, dtype=torch.float32):
    # garbage-filled outputs: a store a kernel misses shows as a difference
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


# ------------------------------------------------------------ attention
def attn_weights(H, K):
    return {"qk": t(K, H, seed=2, scale=H ** -0.5), "cb": t(K, seed=3),
            "Wv": t(K, H, H, seed=5, scale=H ** -0.5), "bv": t(K, H, seed=6),
            "Wl": t(H, H, seed=7, scale=H ** -0.5), "bl": t(H, seed=8),
            "wmu": t(H, seed=9, scale=H ** -0.5), "bmu": t(1, seed=10),
            "wsig": t(H, seed=11, scale=H ** -0.5), "bsig": t(1, seed=12)}


def run_attn_seg(h, lens, wt, seed):
    D, K = len(lens), wt["qk"].size(0)
    o = {"pmu": garbage((D, K), seed), "psig_c": garbage((D, K), seed + 1),
         "guard": garbage((D, K), seed + 2, torch.int32)}
    ext.attn_seg_fwd(h, seg_tensor(lens), max(lens) if lens else 0, wt["qk"],
                     wt["cb"], wt["Wv"], wt["bv"], wt["Wl"], wt["bl"],
                     wt["wmu"], wt["bmu"], wt["wsig"], wt["bsig"], o["pmu"],
                     o["psig_c"], o["guard"], h.size(1) ** -0.5)
    return o


def run_attn_day(h, wt, seed):
    """The existing per-day kernel, original variant, no dropout."""
    N, H = h.shape
    K = wt["qk"].size(0)
    g = lambda *s: garbage(s, seed)
    o = {"a": g(N, K), "sd": g(N, K),
         "guard": garbage((K,), seed, torch.int32), "u": g(K, H),
         "ctx": g(K, H), "hm2": g(K, H), "pmu": g(K), "psig_pre": g(K),
         "psig": g(K), "psig_c": g(K)}
    ext.attn_fused_fwd(h, wt["qk"], wt["cb"], None, wt["Wv"], wt["bv"],
                       wt["Wl"], wt["bl"], wt["wmu"], wt["bmu"], wt["wsig"],
                       wt["bsig"], o["a"], o["sd"], o["guard"], o["u"],
                       o["ctx"], o["hm2"], o["pmu"], o["psig_pre"], o["psig"],
                       o["psig_c"], H ** -0.5, KEEP_INV, 0)
    return o


def attn_reference(h, wt):
    """The predictor's math in float64 torch ops."""
    d = lambda x: x.double()
    H = h.size(1)
    s = (d(h) @ d(wt["qk"]).T + d(wt["cb"])) * (H ** -0.5)
    a = torch.softmax(torch.relu(s), dim=0)
    u = a.T @ d(h)                                        # (K,H)
    ctx = torch.einsum("kji,ki->kj", d(wt["Wv"]), u) + d(wt["bv"])
    hm2 = torch.nn.functional.leaky_relu(ctx @ d(wt["Wl"]).T + d(wt["bl"]))
    pmu = hm2 @ d(wt["wmu"]) + d(wt["bmu"])
    psig = torch.nn.functional.softplus(hm2 @ d(wt["wsig"]) + d(wt["bsig"]))
    return pmu.float(), psig.float()


@pytest.mark.parametrize("H,K", HK)
@pytest.mark.parametrize("N", [1, 37, 257, 448])
def test_attn_seg_one_day_bits(N, H, K):
    wt = attn_weights(H, K)
    h = t(N, H, seed=1)
    old = run_attn_day(h, wt, 100)
    new = run_attn_seg(h, [N], wt, 200)
    torch.cuda.synchronize()
    assert int(old["guard"].abs().sum()) == 0
    for name in ("pmu", "psig_c", "guard"):
        assert_same_bits(new[name][0], old[name], f"N={N} H={H} K={K} {name}")


@pytest.mark.parametrize("H,K", HK)
def test_attn_seg_long_day_in_the_same_launch(H, K):
    """A 4096-stock day (h re-read from L2, only the scores in LDS) next to
    a short staged one, against the float64 math."""
    wt = attn_weights(H, K)
    lens = [5, 4096, 300]
    h = t(sum(lens), H, seed=21)
    o = run_attn_seg(h, lens, wt, 300)
    torch.cuda.synchronize()
    assert int(o["guard"].abs().sum()) == 0
    r0 = 0
    for d, n in enumerate(lens):
        pmu, psig = attn_reference(h[r0:r0 + n], wt)
        assert torch.allclose(o["pmu"][d], pmu, atol=TOL, rtol=TOL), (d, n)
        assert torch.allclose(o["psig_c"][d], psig, atol=TOL, rtol=TOL), (d, n)
        r0 += n


def test_attn_seg_refuses_a_segment_outside_the_buffer():
    """Offsets that run past the packed rows (or past the longest day the
    launch was sized for) are not read: the day comes back marked."""
    H, K = 20, 3
    wt = attn_weights(H, K)
    h = t(8, H, seed=22)
    o = {"pmu": garbage((2, K), 1), "psig_c": garbage((2, K), 2),
         "guard": garbage((2, K), 3, torch.int32)}
    seg = torch.tensor([0, 5, 999], dtype=torch.int32, device=DEV)
    ext.attn_seg_fwd(h, seg, 5, wt["qk"], wt["cb"], wt["Wv"], wt["bv"],
                     wt["Wl"], wt["bl"], wt["wmu"], wt["bmu"], wt["wsig"],
                     wt["bsig"], o["pmu"], o["psig_c"], o["guard"],
                     H ** -0.5)
    good = run_attn_seg(h[:5], [5], wt, 10)
    torch.cuda.synchronize()
    assert_same_bits(o["pmu"][0], good["pmu"][0], "valid day")
    assert o["guard"][0].eq(0).all() and o["guard"][1].eq(2).all()
    assert torch.isnan(o["pmu"][1]).all() and torch.isnan(o["psig_c"][1]).all()


# -------------------------------------------------------------- decoder
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


def run_dec_seg(h, lens, wt, fmu, fsig, eps, seed, with_beta):
    N, K = h.size(0), wt[6].size(0)
    o = {"mu": garbage((N,), seed), "sigma": garbage((N,), seed + 1),
         "sample": garbage((N,), seed + 2), "beta": garbage((N, K), seed + 3)}
    ext.dec_seg_fwd(h, seg_tensor(lens), *wt, fmu, fsig, eps, o["mu"],
                    o["sigma"], o["sample"], o["beta"] if with_beta else None)
    return o


@pytest.mark.parametrize("H,K", HK)
@pytest.mark.parametrize("N", [1, 5, 300])
def test_dec_seg_one_day_bits(N, H, K):
    dec, wt = dec_weights(H, K)
    h, eps = t(N, H, seed=31), t(N, seed=32)
    fmu = t(1, K, seed=33)
    fsig = t(1, K, seed=34).abs() + 0.1
    old = {"recon": garbage((N,), 1), "a1": garbage((N, H), 2),
           "beta": garbage((N, K), 3), "asig_pre": garbage((N,), 4),
           "sigma": garbage((N,), 5)}
    ext.dec_fwd(h, *wt, fmu[0], fsig[0], eps, old["recon"], old["a1"],
                old["beta"], old["asig_pre"], old["sigma"])
    new = run_dec_seg(h, [N], wt, fmu, fsig, eps, 400, True)
    bare = run_dec_seg(h, [N], wt, fmu, fsig, eps, 400, False)
    untouched = garbage((N, K), 403)
    torch.cuda.synchronize()
    for o in (new, bare):
        assert_same_bits(o["sigma"], old["sigma"], "sigma")
        assert_same_bits(o["sample"], old["recon"], "sample")
    assert_same_bits(new["beta"], old["beta"], "beta")
    assert_same_bits(bare["beta"], untouched, "beta not requested")
    with torch.no_grad():
        mu, sigma = dec.dist(h, fmu[0], fsig[0])
    assert torch.allclose(new["mu"], mu.view(-1), atol=TOL, rtol=TOL)
    assert torch.allclose(new["sigma"], sigma.view(-1), atol=TOL, rtol=TOL)
    # without eps nothing is sampled
    o = run_dec_seg(h, [N], wt, fmu, fsig, None, 400, False)
    torch.cuda.synchronize()
    assert_same_bits(o["mu"], new["mu"], "mu without eps")
    assert_same_bits(o["sample"], garbage((N,), 402), "sample without eps")


# ------------------------------------------------------------------ GRU
@pytest.mark.parametrize("H", [7, 20, 64])
@pytest.mark.parametrize("N", [1, 17, 70])
def test_gru_infer_matches_training_forward(N, H):
    T = 5
    gi = t(N, T, 3 * H, seed=41)
    Whh = t(3 * H, H, seed=42, scale=H ** -0.5)
    bhh = t(3 * H, seed=43)
    h0, h1 = garbage((N, H), 1), garbage((N, H), 2)
    ext.gru_fwd(gi, Whh, bhh, h0, None, garbage((N, T, H), 3),
                garbage((N, T, 4 * H), 4), N, T, H)
    ext.gru_fwd_infer(gi, Whh, bhh, h1, N, T, H)
    torch.cuda.synchronize()
    assert_same_bits(h1, h0, f"gru_fwd_infer N={N} H={H}")
    if H == 64:
        wb = Whh.to(torch.bfloat16)
        h2, h3 = garbage((N, H), 5), garbage((N, H), 6)
        ext.gru_fwd_mfma(gi, wb, bhh, h2, None, garbage((N, T, H), 7),
                         garbage((N, T, 4 * H), 8), N, T, H)
        ext.gru_fwd_mfma_infer(gi, wb, bhh, h3, N, T, H)
        torch.cuda.synchronize()
        assert_same_bits(h3, h2, f"gru_fwd_mfma_infer N={N}")


# ------------------------------------------------- segments in one batch
LENS = [1, 3, 64, 65, 257, 300, 600]  # 600 exceeds the LDS-staged limit


def packed_kernels(hs, order, wt_a, wt_d, eps, seed):
    """Attention + decoder over the days of `order`, packed; per-day
    slices of pmu / mu / sigma keyed by day."""
    lens = [hs[d].size(0) for d in order]
    h = torch.cat([hs[d] for d in order])
    e = torch.cat([eps[d] for d in order])
    a = run_attn_seg(h, lens, wt_a, seed)
    o = run_dec_seg(h, lens, wt_d, a["pmu"], a["psig_c"], e, seed + 10,
                    False)
    torch.cuda.synchronize()
    res, r0 = {}, 0
    for j, d in enumerate(order):
        n = lens[j]
        res[d] = {"pmu": a["pmu"][j].clone(),
                  "psig_c": a["psig_c"][j].clone(),
                  "mu": o["mu"][r0:r0 + n].clone(),
                  "sigma": o["sigma"][r0:r0 + n].clone(),
                  "sample": o["sample"][r0:r0 + n].clone()}
        r0 += n
    return res


@pytest.mark.parametrize("H,K", HK)
def test_batch_invariance(H, K):
    wt_a = attn_weights(H, K)
    _, wt_d = dec_weights(H, K)
    hs = [t(n, H, seed=50 + i) for i, n in enumerate(LENS)]
    eps = [t(n, seed=70 + i) for i, n in enumerate(LENS)]
    days = list(range(len(LENS)))
    packed = packed_kernels(hs, days, wt_a, wt_d, eps, 500)
    rev = packed_kernels(hs, days[::-1], wt_a, wt_d, eps, 600)
    for d in days:
        alone = packed_kernels(hs, [d], wt_a, wt_d, eps, 700)[d]
        for name in alone:
            what = f"day {d} (N={LENS[d]}) {name}"
            assert_same_bits(packed[d][name], alone[name], what + " packed")
            assert_same_bits(rev[d][name], alone[name], what + " reversed")


@pytest.mark.parametrize("H,K", HK)
def test_empty_segments_and_batches(H, K):
    wt_a = attn_weights(H, K)
    _, wt_d = dec_weights(H, K)
    hs = {0: t(3, H, seed=80), 1: t(0, H, seed=81), 2: t(5, H, seed=82)}
    eps = {0: t(3, seed=83), 1: t(0, seed=84), 2: t(5, seed=85)}
    with_empty = packed_kernels(hs, [0, 1, 2], wt_a, wt_d, eps, 800)
    without = packed_kernels(hs, [0, 2], wt_a, wt_d, eps, 800)
    for d in (0, 2):
        for name in without[d]:
            assert_same_bits(with_empty[d][name], without[d][name],
                             f"day {d} {name}")
    # the empty day's per-day outputs are not written
    assert_same_bits(with_empty[1]["pmu"], garbage((3, K), 800)[1], "pmu")
    # D = 0 and an all-empty batch launch nothing and return
    for lens in ([], [0, 0]):
        a = run_attn_seg(t(0, H), lens, wt_a, 900)
        o = run_dec_seg(t(0, H), lens, wt_d, a["pmu"], a["psig_c"], t(0),
                        910, True)
        torch.cuda.synchronize()
        assert_same_bits(a["pmu"], garbage((len(lens), K), 900), "pmu")
        assert o["mu"].numel() == 0


# --------------------------------------------------- through the engine
def _trainer(H, K, dtype="fp32", train=False, use_graph=False, seed=0):
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    set_seed(seed)
    model = build_factorvae(num_latent=C_, hidden_size=H, num_portfolio=M_,
                            num_factor=K).to(DEV)
    return FusedTrainer(model, lr=1e-3, t_max=100, device=DEV,
                        use_graph=use_graph, train=train, dtype=dtype)


def _days(lens, seed=0):
    xs = [t(n, T_, C_, seed=seed + i) for i, n in enumerate(lens)]
    eps = [t(n, seed=seed + 100 + i) for i, n in enumerate(lens)]
    return xs, eps


def _per_day(tr, x, eps):
    """tr.predict's kernel sequence with a given eps: (score, sigma, guard)."""
    N, T, _ = x.shape
    tr._ensure_ws(N, T)
    w = tr.ws
    w["x"].copy_(x)
    w["y"].zero_()
    w["eps"].copy_(eps)
    was, tr.training = tr.training, False
    try:
        tr._launch_predict(N, T)
    finally:
        tr.training = was
    torch.cuda.synchronize()
    return (w["recon"].view(N, 1).cpu(), w["sigma"].view(N, 1).cpu(),
            w["guard"].cpu())


def _cpu(entries):
    return [tuple(x.cpu() for x in e) for e in entries]


ENGINE_LENS = [1, 37, 300, 448, 600]


@pytest.mark.parametrize("H,K", HK)
def test_predict_many_matches_per_day_and_eager(H, K):
    tr = _trainer(H, K)
    xs, eps = _days(ENGINE_LENS, seed=200)
    many = _cpu(tr.predict_many(xs, eps=eps, return_dist=True))
    assert len(many) == len(xs)
    for x, e, (score, mu, sigma), n in zip(xs, eps, many, ENGINE_LENS):
        assert score.shape == mu.shape == sigma.shape == (n, 1)
        s_ref, sig_ref, guard = _per_day(tr, x, e)
        assert int(guard.abs().sum()) == 0
        assert torch.allclose(score, s_ref, atol=TOL, rtol=TOL), n
        assert torch.allclose(sigma, sig_ref, atol=TOL, rtol=TOL), n
        if n <= 448:
            assert_same_bits(score, s_ref, f"score N={n}")
            assert_same_bits(sigma, sig_ref, f"sigma N={n}")
        mu_e, sig_e = tr.model.prediction_dist(x)
        assert torch.allclose(mu, mu_e.cpu(), atol=TOL, rtol=TOL), n
        assert torch.allclose(sigma, sig_e.cpu(), atol=TOL, rtol=TOL), n
        assert torch.allclose(score, mu + e.cpu().view(n, 1) * sigma,
                              atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("H,K", HK)
def test_predict_many_outputs_and_host_inputs(H, K):
    tr = _trainer(H, K)
    xs, eps = _days([5, 37], seed=300)
    full = tr.predict_many(xs, eps=eps, return_dist=True, return_beta=True)
    plain = tr.predict_many([x.cpu() for x in xs],
                            eps=[e.cpu() for e in eps])
    only_beta = tr.predict_many(xs, eps=eps, return_beta=True)
    for d, n in enumerate([5, 37]):
        score, mu, sigma, beta = full[d]
        assert beta.shape == (n, K)
        assert_same_bits(plain[d].cpu(), score.cpu(), "host inputs")
        assert len(only_beta[d]) == 2
        assert_same_bits(only_beta[d][1].cpu(), beta.cpu(), "beta")
        beta_e = tr.model.factor_decoder.beta_layer(
            tr.model.feature_extractor(xs[d]))
        assert torch.allclose(beta.cpu(), beta_e.detach().cpu(), atol=TOL,
                              rtol=TOL)
    assert tr.predict_many([]) == []
    # eps drawn by the generator: reproducible under a seed
    torch.manual_seed(9)
    a = tr.predict_many(xs)
    torch.manual_seed(9)
    b = tr.predict_many(xs)
    for u, v in zip(a, b):
        assert_same_bits(u.cpu(), v.cpu(), "seeded eps")


@pytest.mark.parametrize("H,K", HK)
def test_predict_many_chunks_and_order(H, K):
    tr = _trainer(H, K)
    lens = [3, 64, 65, 257, 300, 600, 1]
    xs, eps = _days(lens, seed=400)
    one = _cpu(tr.predict_many(xs, eps=eps, return_dist=True))
    # 600*T rows per chunk: [3,64,65,257] [300] [600,1]... three or more
    budget = 600 * T_
    chunked = _cpu(tr.predict_many(xs, eps=eps, return_dist=True,
                                   max_rows=budget))
    rev = _cpu(tr.predict_many(xs[::-1], eps=eps[::-1],
                               return_dist=True))[::-1]
    for d, n in enumerate(lens):
        alone = _cpu(tr.predict_many([xs[d]], eps=[eps[d]],
                                     return_dist=True))[0]
        for j, name in enumerate(("score", "mu", "sigma")):
            what = f"day {d} (N={n}) {name}"
            assert_same_bits(chunked[d][j], one[d][j], what + " chunked")
            assert_same_bits(rev[d][j], one[d][j], what + " reversed")
            assert_same_bits(alone[j], one[d][j], what + " alone")


def test_chunking_respects_the_row_budget(monkeypatch):
    tr = _trainer(20, 3)
    calls = []
    real = tr._launch_predict_many
    monkeypatch.setattr(
        tr, "_launch_predict_many",
        lambda iw, R, Nn, D, *a: (calls.append((R, D)), real(iw, R, Nn, D, *a)))
    xs, eps = _days([10, 10, 10, 50, 10], seed=450)
    tr.predict_many(xs, eps=eps, max_rows=25 * T_)
    # greedy: [10,10] [10] [50 alone, over budget] [10]
    assert calls == [(20 * T_, 2), (10 * T_, 1), (50 * T_, 1), (10 * T_, 1)]
    calls.clear()
    monkeypatch.setenv("FV_PREDICT_ROWS", str(30 * T_))
    tr.predict_many(xs, eps=eps)
    assert calls == [(30 * T_, 3), (50 * T_, 1), (10 * T_, 1)]


@pytest.mark.parametrize("H,K", HK)
def test_guard_isolation(H, K):
    tr = _trainer(H, K)
    lens = [5, 37, 70]
    xs, eps = _days(lens, seed=500)
    clean = _cpu(tr.predict_many([xs[0], xs[2]], eps=[eps[0], eps[2]],
                                 return_dist=True))
    xs[1] = xs[1].clone()
    xs[1][11, 2, 3] = float("nan")
    got = _cpu(tr.predict_many(xs, eps=eps, return_dist=True))
    guard = tr._iws["guard"][:3].cpu()
    assert guard[1].eq(1).all() and guard[0].eq(0).all() \
        and guard[2].eq(0).all()
    for j, d in enumerate((0, 2)):
        for a, b, name in zip(got[d], clean[j], ("score", "mu", "sigma")):
            assert_same_bits(a, b, f"day {d} {name} next to a guarded day")
    # the poisoned day itself: what per-day predict gives
    s_ref, sig_ref, g_ref = _per_day(tr, xs[1], eps[1])
    assert g_ref.eq(1).all()
    score, mu, sigma = got[1]
    ok = torch.ones(37, dtype=torch.bool)
    ok[11] = False
    assert torch.isnan(score[11]).all() and torch.isnan(s_ref[11]).all()
    assert torch.isfinite(score[ok]).all()
    assert_same_bits(score[ok], s_ref[ok], "guarded day score")
    assert_same_bits(sigma[ok], sig_ref[ok], "guarded day sigma")


@pytest.mark.parametrize("H,K", HK)
def test_bf16_engine_close_to_fp32(H, K):
    xs, eps = _days([37, 300], seed=600)
    outs = {}
    for dtype in ("fp32", "bf16"):
        tr = _trainer(H, K, dtype=dtype)
        outs[dtype] = _cpu(tr.predict_many(xs, eps=eps, return_dist=True))
    for a, b in zip(outs["bf16"], outs["fp32"]):
        for u, v in zip(a, b):
            # test_bf16_full_step_vs_fp32's forward bound, per element
            assert bool(((u - v).abs() < 0.02 * (v.abs() + 1.0)).all())
    # the bf16 engine too is batch invariant
    tr = _trainer(H, K, dtype="bf16")
    alone = _cpu(tr.predict_many([xs[0]], eps=[eps[0]], return_dist=True))[0]
    both = _cpu(tr.predict_many(xs[::-1], eps=eps[::-1],
                                return_dist=True))[1]
    for u, v in zip(alone, both):
        assert_same_bits(u, v, "bf16 alone vs packed")


def test_fp8_engine_is_refused():
    tr = _trainer(64, 20, dtype="fp8")
    xs, eps = _days([5], seed=700)
    with pytest.raises(ValueError, match="fp8"):
        tr.predict_many(xs, eps=eps)


@pytest.mark.parametrize("H,K", HK)
def test_no_interference_with_training(H, K):
    x, y = t(40, T_, C_, seed=800), t(40, 1, seed=801)
    xs, eps = _days([7, 40, 90], seed=810)
    params = {}
    for with_scoring in (False, True):
        tr = _trainer(H, K, train=True, use_graph=True, seed=5)
        tr.step(x, y)
        if with_scoring:
            n_graphs = len(tr._graphs)
            assert tr.use_graph and n_graphs >= 1
            ws = tr.ws
            # eps from the caller: the generator the training step draws
            # its noise from is not advanced
            tr.predict_many(xs, eps=eps, return_dist=True)
            assert len(tr._graphs) == n_graphs
            assert tr.ws is ws
        tr.step(x, y)
        torch.cuda.synchronize()
        params[with_scoring] = tr.params.flat.clone()
    assert_same_bits(params[True], params[False], "parameters")


@pytest.mark.parametrize("H,K", HK)
def test_scorer_batch_days_end_to_end(H, K):
    from factorvae_amd.data.sampler import init_data_loader
    from factorvae_amd.data.synthetic import make_synthetic_frame
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import generate_prediction_scores, test_args

    df = make_synthetic_frame(n_days=40, n_stocks=30, n_features=C_, seed=6,
                              ragged=True)
    args = test_args(run_name="t", num_factor=K, hidden_size=H,
                     num_latent=C_, num_portfolio=M_, seq_length=T_)
    frames = {}
    for key, kw in (("b16", dict(engine="auto", batch_days=16,
                                 return_dist=True)),
                    ("b1", dict(engine="auto", batch_days=1,
                                return_dist=True)),
                    ("eager", dict(engine="eager", batch_days=16,
                                   return_dist=True)),
                    ("default", dict(engine="auto"))):
        torch.manual_seed(0)
        model = build_factorvae(num_latent=C_, hidden_size=H,
                                num_portfolio=M_, num_factor=K).to(DEV)
        loader = init_data_loader(df, step_len=T_, shuffle=False, start=None,
                                  end=None)
        frames[key] = generate_prediction_scores(model, loader,
                                                 loader.dataset, args, **kw)
    b16 = frames["b16"]
    assert list(b16.columns) == ["score", "mu", "sigma"]
    assert list(frames["default"].columns) == ["score"]
    assert len(b16) > 0
    for key in ("b1", "eager", "default"):
        assert b16.index.equals(frames[key].index), key
    for key in ("b1", "eager"):
        for col in ("mu", "sigma"):
            a = torch.from_numpy(b16[col].to_numpy())
            b = torch.from_numpy(frames[key][col].to_numpy())
            assert torch.allclose(a, b, atol=TOL, rtol=TOL), (key, col)


def test_serving_engine_scores_many_days_in_one_call():
    from factorvae_amd.serve import ScoringEngine

    torch.manual_seed(0)
    eng = ScoringEngine(None, num_latent=C_, hidden_size=64,
                        num_portfolio=M_, num_factor=20, seq_length=T_,
                        device="cuda")
    assert eng.engine == "fused"
    xs, _ = _days([5, 37, 300], seed=900)
    out = eng.score_many([x.cpu() for x in xs], dist=True)
    assert [len(o["scores"]) for o in out] == [5, 37, 300]
    for x, o in zip(xs, out):
        mu, sigma = eng.model.prediction_dist(x)
        assert torch.allclose(torch.tensor(o["mu"]), mu.view(-1).cpu(),
                              atol=TOL, rtol=TOL)
        assert torch.allclose(torch.tensor(o["sigma"]), sigma.view(-1).cpu(),
                              atol=TOL, rtol=TOL)
