"""Batched multi-day posterior pass: the segmented encoder, its heads and
the segmented loss, FusedTrainer.loss_many, evaluate_many / validate_metrics
with_loss, validate_epoch(batched=True) and train_main --val_batched —
against the per-day kernels / the per-day forward (bit patterns where the
arithmetic order is the same), float64 math and the eager module's
loss_terms (1e-4, the project's forward tolerance)."""

import json
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from factorvae_amd.ops import get_extension
    ext = get_extension()
DEV = torch.device("cuda:0")
HK = [(20, 3), (64, 20)]
T_, C_, M_ = 4, 24, 8
TOL = 1e-4
FACTORS = ("post_mu", "post_sigma", "prior_mu", "prior_sigma")
SCALARS = ("loss", "mse", "kl")


def t(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def garbage(shape, seed):
    # garbage-filled outputs: a store a kernel misses shows as a difference
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


def close_rel(a, b):
    """|a - b| <= TOL * (1 + |b|), element-wise."""
    return bool(((a - b).abs() <= TOL * (1.0 + b.abs())).all())


# -------------------------------------------------------------- encoder
def enc_weights(H, K):
    return {"Wenc": t(M_, H, seed=2, scale=H ** -0.5), "benc": t(M_, seed=3),
            "Wmu": t(K, M_, seed=4, scale=M_ ** -0.5), "bmu": t(K, seed=5),
            "Wsig": t(K, M_, seed=6, scale=M_ ** -0.5), "bsig": t(K, seed=7)}


def run_enc_seg(h, y, lens, wt, seed, max_n=None):
    D, K = len(lens), wt["Wmu"].size(0)
    o = {"yp": garbage((D, M_), seed), "fmu": garbage((D, K), seed + 1),
         "fsig_c": garbage((D, K), seed + 2)}
    ext.enc_seg_fwd(h, seg_tensor(lens),
                    (max(lens) if lens else 0) if max_n is None else max_n,
                    wt["Wenc"], wt["benc"], y, o["yp"])
    ext.enc_seg_heads(o["yp"], wt["Wmu"], wt["bmu"], wt["Wsig"], wt["bsig"],
                      o["fmu"], o["fsig_c"])
    return o


def run_enc_day(h, y, wt, seed):
    """The per-day kernel, original variant, heads on its last workgroup."""
    N, K = h.size(0), wt["Wmu"].size(0)
    g = lambda *s: garbage(s, seed)
    o = {"scores": g(N, M_), "a": g(N, M_), "yp": g(M_), "fmu": g(K),
         "fsig_pre": g(K), "fsig": g(K), "fsig_c": g(K)}
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    ext.enc_fused_fwd(h, wt["Wenc"], wt["benc"], y, o["scores"], o["a"],
                      o["yp"], wt["Wmu"], wt["bmu"], wt["Wsig"], wt["bsig"],
                      o["fmu"], o["fsig_pre"], o["fsig"], o["fsig_c"], done,
                      0)
    return o


def enc_reference(h, y, wt):
    """The encoder's portfolio returns in float64 torch ops."""
    d = lambda x: x.double()
    a = torch.softmax(d(h) @ d(wt["Wenc"]).T + d(wt["benc"]), dim=0)
    return (a.T @ d(y).view(-1)).float()


@pytest.mark.parametrize("H,K", HK)
@pytest.mark.parametrize("N", [1, 37, 257, 448])
def test_enc_seg_one_day_bits(N, H, K):
    wt = enc_weights(H, K)
    h, y = t(N, H, seed=1), t(N, seed=8, scale=0.1)
    old = run_enc_day(h, y, wt, 100)
    new = run_enc_seg(h, y, [N], wt, 200)
    torch.cuda.synchronize()
    for name in ("yp", "fmu", "fsig_c"):
        assert_same_bits(new[name][0], old[name], f"N={N} H={H} K={K} {name}")


def packed_enc(hs, ys, order, wt, seed):
    lens = [hs[d].size(0) for d in order]
    o = run_enc_seg(torch.cat([hs[d] for d in order]),
                    torch.cat([ys[d] for d in order]), lens, wt, seed)
    torch.cuda.synchronize()
    return {d: {k: v[j].clone() for k, v in o.items()}
            for j, d in enumerate(order)}


@pytest.mark.parametrize("H,K", HK)
def test_enc_seg_several_days(H, K):
    """A 4096-stock day (h re-read from L2, only the scores in LDS) between
    two short staged ones against the float64 math; every day keeps its bits
    in the reverse order and alone. The fourth day is staged when it runs
    alone and not staged next to the long one."""
    wt = enc_weights(H, K)
    lens = [5, 4096, 300, {20: 1600, 64: 520}[H]]
    hs = [t(n, H, seed=21 + i) for i, n in enumerate(lens)]
    ys = [t(n, seed=31 + i, scale=0.1) for i, n in enumerate(lens)]
    days = list(range(len(lens)))
    packed = packed_enc(hs, ys, days, wt, 300)
    rev = packed_enc(hs, ys, days[::-1], wt, 310)
    for d, n in enumerate(lens):
        ref = enc_reference(hs[d], ys[d], wt)
        assert torch.allclose(packed[d]["yp"], ref, atol=TOL, rtol=TOL), (d, n)
        alone = packed_enc(hs, ys, [d], wt, 320)[d]
        for name in alone:
            what = f"day {d} (N={n}) {name}"
            assert_same_bits(packed[d][name], alone[name], what + " packed")
            assert_same_bits(rev[d][name], alone[name], what + " reversed")


@pytest.mark.parametrize("H,K", HK)
def test_enc_seg_empty_day_in_the_middle(H, K):
    wt = enc_weights(H, K)
    hs = {0: t(5, H, seed=40), 1: t(0, H, seed=41), 2: t(37, H, seed=42)}
    ys = {0: t(5, seed=43), 1: t(0, seed=44), 2: t(37, seed=45)}
    with_empty = packed_enc(hs, ys, [0, 1, 2], wt, 400)
    without = packed_enc(hs, ys, [0, 2], wt, 400)
    for d in (0, 2):
        for name in without[d]:
            assert_same_bits(with_empty[d][name], without[d][name],
                             f"day {d} {name}")
    # the empty day's yp is not written
    assert_same_bits(with_empty[1]["yp"], garbage((3, M_), 400)[1], "yp")
    # D = 0 and an all-empty batch launch nothing and return
    for lens in ([], [0, 0]):
        o = run_enc_seg(t(0, H), t(0), lens, wt, 410)
        torch.cuda.synchronize()
        assert_same_bits(o["yp"], garbage((len(lens), M_), 410), "yp")


@pytest.mark.parametrize("seg,max_n", [([0, 5, 12], 8),   # runs past total
                                       ([0, 5, 999], 5),  # far past total
                                       ([0, 2, 8], 2)])   # longer than max_n
def test_enc_seg_refuses_a_segment_outside_the_buffer(seg, max_n):
    """Offsets that run past the packed rows (or past the longest day the
    launch was sized for) are not read: the day comes back as NaN."""
    H, K = 20, 3
    wt = enc_weights(H, K)
    h, y = t(8, H, seed=50), t(8, seed=51)
    n0 = seg[1]
    yp = garbage((2, M_), 1)
    ext.enc_seg_fwd(h, torch.tensor(seg, dtype=torch.int32, device=DEV),
                    max_n, wt["Wenc"], wt["benc"], y, yp)
    good = run_enc_seg(h[:n0], y[:n0], [n0], wt, 10)
    torch.cuda.synchronize()
    assert_same_bits(yp[0], good["yp"][0], "valid day")
    assert torch.isnan(yp[1]).all()


# ----------------------------------------------------------------- loss
def loss_inputs(lens, K, seed):
    D, N = len(lens), sum(lens)
    return {"recon": t(N, seed=seed), "y": t(N, seed=seed + 1),
            "fmu": t(D, K, seed=seed + 2),
            "fsig_c": t(D, K, seed=seed + 3).abs() + 0.1,
            "pmu": t(D, K, seed=seed + 4),
            "psig_c": t(D, K, seed=seed + 5).abs() + 0.1}


def run_loss_seg(i, lens, seed):
    D = len(lens)
    o = {k: garbage((D,), seed + j) for j, k in enumerate(SCALARS)}
    ext.loss_seg(i["recon"], i["y"], seg_tensor(lens), i["fmu"], i["fsig_c"],
                 i["pmu"], i["psig_c"], o["loss"], o["mse"], o["kl"])
    return o


@pytest.mark.parametrize("K", [3, 20])
@pytest.mark.parametrize("N", [1, 37, 300, 600])
def test_loss_seg_one_day_bits(N, K):
    i = loss_inputs([N], K, 60)
    old = {k: garbage((1,), 70 + j) for j, k in enumerate(SCALARS)}
    ext.loss_scalars(i["recon"], i["y"], i["fmu"][0], i["fsig_c"][0],
                     i["pmu"][0], i["psig_c"][0], old["loss"], old["mse"],
                     old["kl"])
    new = run_loss_seg(i, [N], 80)
    torch.cuda.synchronize()
    for k in SCALARS:
        assert_same_bits(new[k], old[k], f"N={N} K={K} {k}")


@pytest.mark.parametrize("K", [3, 20])
def test_loss_seg_ragged_days_and_an_empty_one(K):
    lens = [5, 0, 600, 37]
    i = loss_inputs(lens, K, 90)
    o = run_loss_seg(i, lens, 95)
    torch.cuda.synchronize()
    d64 = lambda x: x.double()
    r0 = 0
    for d, n in enumerate(lens):
        if n == 0:
            assert all(bool(torch.isnan(o[k][d])) for k in SCALARS)
            continue
        mse = ((d64(i["recon"][r0:r0 + n]) - d64(i["y"][r0:r0 + n])) ** 2
               ).mean()
        fs, ps = d64(i["fsig_c"][d]), d64(i["psig_c"][d])
        kl = (torch.log(ps / fs) + (fs ** 2 + (d64(i["fmu"][d])
              - d64(i["pmu"][d])) ** 2) / (2 * ps ** 2) - 0.5).sum()
        for k, ref in (("mse", mse), ("kl", kl), ("loss", mse + kl)):
            assert close_rel(o[k][d].double(), ref), (d, k, o[k][d], ref)
        r0 += n
    # a segment outside the packed rows is not read either
    bad = {k: garbage((2,), 99) for k in SCALARS}
    two = loss_inputs([5, 3], K, 97)
    ext.loss_seg(two["recon"], two["y"],
                 torch.tensor([0, 5, 999], dtype=torch.int32, device=DEV),
                 two["fmu"], two["fsig_c"], two["pmu"], two["psig_c"],
                 bad["loss"], bad["mse"], bad["kl"])
    good = run_loss_seg(two, [5, 3], 98)
    torch.cuda.synchronize()
    for k in SCALARS:
        assert_same_bits(bad[k][0], good[k][0], k)
        assert bool(torch.isnan(bad[k][1]))


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
    days = [(t(n, T_, C_, seed=seed + i), t(n, seed=seed + 50 + i, scale=0.1))
            for i, n in enumerate(lens)]
    eps = [t(n, seed=seed + 100 + i) for i, n in enumerate(lens)]
    return days, eps


def assert_day_bits(a, b, i, j, what):
    """Day i of result a against day j of result b, every output."""
    for k in a:
        assert_same_bits(a[k][i], b[k][j], f"{what} {k}")


ENGINE_LENS = [1, 37, 300, 448, 600]


@pytest.mark.parametrize("H,K", HK)
def test_loss_many_matches_eager_and_per_day(H, K):
    tr = _trainer(H, K)
    days, eps = _days(ENGINE_LENS, seed=200)
    r = tr.loss_many(days, eps=eps, return_factors=True)
    assert set(r) == set(SCALARS) | set(FACTORS) | {"n"}
    assert r["n"].dtype == torch.int32 and r["n"].tolist() == ENGINE_LENS
    assert r["loss"].dtype == torch.float32 and r["loss"].shape == (5,)
    assert r["post_mu"].shape == (5, K) and not r["loss"].is_cuda
    plain = tr.loss_many(days, eps=eps)
    assert set(plain) == set(SCALARS) | {"n"}
    for k in SCALARS:
        assert_same_bits(plain[k], r[k], f"{k} without factors")
    for d, ((x, y), e) in enumerate(zip(days, eps)):
        n = x.shape[0]
        with torch.no_grad():
            ref = tr.model.loss_terms(x, y.view(n, 1), eps=e.view(n, 1))
        for k in FACTORS:
            assert torch.allclose(r[k][d], ref[k].cpu(), atol=TOL,
                                  rtol=TOL), (n, k)
        for k in SCALARS:
            assert close_rel(r[k][d], ref[k].cpu()), (n, k, r[k][d], ref[k])
        if n <= 448:
            # the per-day route with the eps it drew itself
            loss = tr.forward_only(x, y)
            torch.cuda.synchronize()
            drawn = tr.ws["eps"].reshape(-1)[:n].clone()
            want = loss.reshape(-1)[:1].cpu()
            got = tr.loss_many([(x, y)], eps=[drawn])["loss"]
            assert_same_bits(got, want, f"loss N={n} against forward_only")


@pytest.mark.parametrize("H,K", HK)
def test_loss_many_chunks_and_order(H, K):
    tr = _trainer(H, K)
    lens = [3, 64, 65, 257, 300, 600, 1]
    days, eps = _days(lens, seed=400)
    kw = dict(return_factors=True)
    one = tr.loss_many(days, eps=eps, **kw)
    calls = []
    real = tr._launch_predict_many
    tr._launch_predict_many = lambda *a: (calls.append(a[3]), real(*a))
    try:
        chunked = tr.loss_many(days, eps=eps, max_rows=600 * T_, **kw)
    finally:
        del tr._launch_predict_many
    assert len(calls) >= 3 and sum(calls) == len(lens)
    rev = tr.loss_many(days[::-1], eps=eps[::-1], **kw)
    D = len(lens)
    for d, n in enumerate(lens):
        alone = tr.loss_many([days[d]], eps=[eps[d]], **kw)
        what = f"day {d} (N={n})"
        assert_day_bits(chunked, one, d, d, what + " chunked")
        assert_day_bits(rev, one, D - 1 - d, d, what + " reversed")
        assert_day_bits(alone, one, 0, d, what + " alone")


def test_loss_many_empty_days_and_edges():
    tr = _trainer(20, 3)
    r = tr.loss_many([], return_factors=True)
    assert r["loss"].shape == (0,) and r["post_mu"].shape == (0, 3)
    days, eps = _days([5, 0, 37], seed=450)
    r = tr.loss_many(days, eps=eps, return_factors=True)
    ref = tr.loss_many([days[0], days[2]], eps=[eps[0], eps[2]],
                       return_factors=True)
    assert r["n"].tolist() == [5, 0, 37]
    assert_day_bits(r, ref, 0, 0, "day 0")
    assert_day_bits(r, ref, 2, 1, "day 2")
    for k in SCALARS + FACTORS:
        assert bool(torch.isnan(r[k][1]).all()), k
    # a batch of empty days launches nothing
    days0, _ = _days([0, 0], seed=460)
    r = tr.loss_many(days0, return_factors=True)
    assert r["n"].tolist() == [0, 0] and bool(torch.isnan(r["loss"]).all())
    assert bool(torch.isnan(r["prior_sigma"]).all())
    with pytest.raises(ValueError, match="labels"):
        tr.loss_many([(days[0][0], days[2][1])])


@pytest.mark.parametrize("H,K", HK)
def test_loss_many_bf16_close_to_fp32(H, K):
    days, eps = _days([37, 300], seed=600)
    outs = {}
    for dtype in ("fp32", "bf16"):
        tr = _trainer(H, K, dtype=dtype)
        outs[dtype] = tr.loss_many(days, eps=eps, return_factors=True)
    for k in SCALARS + FACTORS:
        u, v = outs["bf16"][k], outs["fp32"][k]
        # test_bf16_engine_close_to_fp32's bound, per element
        assert bool(((u - v).abs() < 0.02 * (v.abs() + 1.0)).all()), k
    # the bf16 engine too is batch invariant
    tr = _trainer(H, K, dtype="bf16")
    alone = tr.loss_many([days[0]], eps=[eps[0]], return_factors=True)
    both = tr.loss_many(days[::-1], eps=eps[::-1], return_factors=True)
    assert_day_bits(alone, both, 0, 1, "bf16 alone vs packed")


def test_loss_many_refuses_the_fp8_engine():
    tr = _trainer(64, 20, dtype="fp8")
    days, eps = _days([5], seed=700)
    with pytest.raises(ValueError, match="fp8"):
        tr.loss_many(days, eps=eps)


def test_sample_false_is_zero_eps_and_draws_nothing():
    tr = _trainer(64, 20)
    days, _ = _days([5, 37], seed=710)
    zeros = [torch.zeros(n, device=DEV) for n in (5, 37)]
    ref = tr.loss_many(days, eps=zeros, return_factors=True)
    cpu_state = torch.random.get_rng_state()
    gpu_state = torch.cuda.get_rng_state(DEV)
    got = tr.loss_many(days, sample=False, return_factors=True)
    assert torch.equal(torch.random.get_rng_state(), cpu_state)
    assert torch.equal(torch.cuda.get_rng_state(DEV), gpu_state)
    for d in range(2):
        assert_day_bits(got, ref, d, d, f"day {d}")
    # eps drawn by the generator: reproducible under a seed, and not zero
    torch.manual_seed(9)
    a = tr.loss_many(days)
    torch.manual_seed(9)
    b = tr.loss_many(days)
    assert_same_bits(a["loss"], b["loss"], "seeded eps")
    assert not torch.equal(a["mse"], ref["mse"])


@pytest.mark.parametrize("H,K", HK)
def test_evaluate_many_with_loss(H, K):
    tr = _trainer(H, K)
    days, eps = _days([5, 64, 0, 257, 600], seed=800)
    on = ("score", "mu")
    base = tr.evaluate_many(days, on=on, topk=3, eps=eps)
    both = tr.evaluate_many(days, on=on, topk=3, eps=eps, with_loss=True)
    assert set(base) == {"columns", "ic", "rank_ic", "long", "short", "count"}
    assert set(both) == set(base) | set(SCALARS)
    for k in ("ic", "rank_ic", "long", "short"):
        assert torch.equal(both[k].view(torch.int64),
                           base[k].view(torch.int64)), k
    assert torch.equal(both["count"], base["count"])
    ref = tr.loss_many(days, eps=eps)
    for k in SCALARS:
        assert_same_bits(both[k], ref[k], k)
    assert bool(torch.isnan(both["loss"][2]))
    # chunked: the same bits
    chunked = tr.evaluate_many(days, on=on, topk=3, eps=eps, with_loss=True,
                               max_rows=260 * T_)
    for k in SCALARS:
        assert_same_bits(chunked[k], ref[k], k + " chunked")


def test_validate_metrics_and_validate_epoch_batched(monkeypatch):
    tr = _trainer(64, 20)
    days, eps = _days([40, 64, 0, 37, 1, 90], seed=900)
    plain = tr.validate_metrics(days, topk=5)
    torch.manual_seed(3)
    got = tr.validate_metrics(days, topk=5, with_loss=True)
    torch.manual_seed(3)
    per_day = tr.loss_many(days)
    assert set(got) == set(plain) | {"loss"}
    for k in plain:
        assert got[k] == plain[k] or (got[k] != got[k]
                                      and plain[k] != plain[k]), k
    finite = per_day["loss"][torch.isfinite(per_day["loss"])].double()
    assert finite.numel() == 5
    assert got["loss"] == float(finite.mean())
    torch.manual_seed(3)
    assert tr.validate_epoch(days, batched=True) == float(finite.mean())
    # the per-day route is still there
    v = tr.validate_epoch([d for d in days if d[0].shape[0]])
    assert v == v
    # the fp8 engine keeps the per-day loop
    tr8 = _trainer(64, 20, dtype="fp8")
    called = []
    monkeypatch.setattr(tr8, "loss_many",
                        lambda *a, **k: called.append(1))
    v = tr8.validate_epoch([days[0]], batched=True)
    assert v == v and not called


@pytest.mark.parametrize("H,K", HK)
def test_no_interference_with_training(H, K):
    x, y = t(40, T_, C_, seed=800), t(40, 1, seed=801)
    days, eps = _days([7, 40, 90], seed=810)
    params = {}
    for with_loss in (False, True):
        tr = _trainer(H, K, train=True, use_graph=True, seed=5)
        tr.step(x, y)
        if with_loss:
            n_graphs = len(tr._graphs)
            assert tr.use_graph and n_graphs >= 1
            ws = tr.ws
            # eps from the caller: the generator the training step draws
            # its noise from is not advanced
            tr.loss_many(days, eps=eps, return_factors=True)
            tr.evaluate_many(days, eps=eps, with_loss=True)
            assert len(tr._graphs) == n_graphs
            assert tr.ws is ws
        tr.step(x, y)
        torch.cuda.synchronize()
        params[with_loss] = tr.params.flat.clone()
    assert_same_bits(params[True], params[False], "parameters")


def test_score_cli_factors_fused_matches_eager(tmp_path, monkeypatch):
    """score.py --factors through loss_many (engine auto on a GPU) against
    the eager engine's files: same rows, values within the forward
    tolerance; the fused route is reproducible byte for byte too."""
    import pandas as pd

    from factorvae_amd import score
    from factorvae_amd.data.synthetic import make_synthetic_frame
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae

    H, K = 64, 20
    used = []
    real = FusedTrainer.loss_many
    monkeypatch.setattr(
        FusedTrainer, "loss_many",
        lambda self, *a, **k: (used.append(k), real(self, *a, **k))[1])
    df = make_synthetic_frame(n_days=20, n_stocks=30, n_features=C_, seed=6,
                              ragged=True)
    data = tmp_path / "d.pkl"
    df.to_pickle(data)
    torch.manual_seed(0)
    ckpt = tmp_path / "m.pt"
    torch.save(build_factorvae(num_latent=C_, hidden_size=H,
                               num_portfolio=M_, num_factor=K).state_dict(),
               ckpt)
    base = ["--checkpoint", str(ckpt), "--dataset", str(data), "--run_name",
            "r", "--num_factor", str(K), "--hidden_size", str(H),
            "--num_latent", str(C_), "--num_portfolio", str(M_),
            "--seq_length", str(T_), "--factors"]
    stem = f"r_{K}_True_False_{C_}_{H}"
    for out, engine in (("f1", "auto"), ("f2", "auto"), ("e", "eager")):
        score.main(base + ["--out_dir", str(tmp_path / out), "--engine",
                           engine])
    assert len(used) == 2 and all(k == dict(sample=False,
                                            return_factors=True)
                                  for k in used)
    for kind, cols in (("factors", FACTORS), ("daily", SCALARS)):
        name = f"{stem}_{kind}.csv"
        assert (tmp_path / "f1" / name).read_bytes() == \
            (tmp_path / "f2" / name).read_bytes()
        fused = pd.read_csv(tmp_path / "f1" / name)
        eager = pd.read_csv(tmp_path / "e" / name)
        assert len(fused) == len(eager) > 0
        assert list(fused.columns) == list(eager.columns)
        for c in ("datetime", "factor", "n_stocks"):
            if c in fused:
                assert fused[c].equals(eager[c]), (kind, c)
        for c in cols:
            a = torch.from_numpy(fused[c].to_numpy())
            b = torch.from_numpy(eager[c].to_numpy())
            assert close_rel(a, b), (kind, c)


@pytest.mark.timeout(300)
def test_train_main_fused_val_batched(tmp_path, monkeypatch):
    from factorvae_amd.data.synthetic import make_synthetic_frame
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.engine.trainer import train_main
    from factorvae_amd.utils import DataArgument

    calls = {"extractor": 0, "per_day": 0, "epochs": 0}
    real_pm = FusedTrainer._launch_predict_many
    real_fo = FusedTrainer.forward_only
    real_vm = FusedTrainer.validate_metrics

    def spy_pm(self, *a, **k):
        calls["extractor"] += 1
        return real_pm(self, *a, **k)

    def spy_fo(self, *a, **k):
        calls["per_day"] += 1
        return real_fo(self, *a, **k)

    def spy_vm(self, days, **k):
        calls["epochs"] += 1
        calls["rows"] = sum(x.shape[0] * x.shape[1] for x, _ in days)
        return real_vm(self, days, **k)

    monkeypatch.setattr(FusedTrainer, "_launch_predict_many", spy_pm)
    monkeypatch.setattr(FusedTrainer, "forward_only", spy_fo)
    monkeypatch.setattr(FusedTrainer, "validate_metrics", spy_vm)
    df = make_synthetic_frame(n_days=60, n_stocks=64, seed=11,
                              signal_strength=1.0, label_from_features=True)
    args = SimpleNamespace(
        num_epochs=2, lr=1e-3, num_latent=158, num_portfolio=32,
        seq_len=8, num_factor=8, hidden_size=64, seed=0,
        run_name="gpu_vb", save_dir=str(tmp_path), dataset=None,
        engine="fused", dtype="fp32", wandb=False, resume=False,
        val_batched=True, val_metrics=True,
    )
    data_args = DataArgument(
        start_time="2015-01-01", end_time="2015-12-31",
        fit_end_time="2015-03-01", val_start_time="2015-03-02",
        val_end_time="2015-03-25", seq_len=8,
    )
    best = train_main(args, data_args, df=df)
    assert best == best and best < 1e6
    recs = [json.loads(line) for line in
            open(os.path.join(str(tmp_path), "gpu_vb_metrics.jsonl"))]
    epochs = [r for r in recs if "Train Loss" in r]
    assert len(epochs) == 2
    for r in epochs:
        assert r["Validation Loss"] == r["Validation Loss"]
        assert abs(r["Validation Loss"]) < 1e6
        assert r["Validation RankIC"] == r["Validation RankIC"]
    assert best == min(r["Validation Loss"] for r in epochs)
    # one validate_metrics pass per epoch; the validation range fits one
    # chunk, so the extractor is launched once per epoch and the per-day
    # validation forward never
    assert calls["epochs"] == 2 and calls["per_day"] == 0
    assert calls["rows"] <= FusedTrainer.PREDICT_ROWS
    assert calls["extractor"] == 2
