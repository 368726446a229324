"""The training step's middle chain (FV_MID_CHAIN, docs/KERNELS.md) against
the kernel sequence it replaces, on the same inputs: every output equal by
bit pattern, at the kernels and over whole steps (FV_MID_CHAIN=0 against
the default)."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from factorvae_amd.ops import get_extension
    ext = get_extension()
DEV = torch.device("cuda:0")
KEEP_INV = 1.0 / (1.0 - 0.1)


def t(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def garbage(*shape, seed=0):
    # garbage-filled outputs: a store a kernel misses shows as a difference
    return t(*shape, seed=1000 + seed) + 3.0


def assert_bits(new, old, what):
    assert set(new) == set(old)
    for name in sorted(old):
        a, b = new[name], old[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        ai = a.contiguous().view(torch.int32)
        bi = b.contiguous().view(torch.int32)
        assert torch.equal(ai, bi), (
            f"{what} {name}: {(ai != bi).sum().item()} of {bi.numel()} "
            f"bit patterns differ")


def dec_nblk(N):
    # decoder.hip owns the block count (test_gpu_binding_checks.py holds it
    # against literals; NBLK_ROWS below does for the counts used here)
    return ext.dec_nblk(N)


def kl_inputs(K, seed=0):
    """fmu, fsig_c, pmu, psig_c of K factors: the sigmas positive, one
    fsig_c and one psig_c at the 1e-6 clamp."""
    fsig_c = t(K, seed=seed + 31).abs() + 0.05
    psig_c = t(K, seed=seed + 33).abs() + 0.05
    fsig_c[K // 2] = 1e-6
    psig_c[(K // 3 + 1) % K] = 1e-6
    return {"fmu": t(K, seed=seed + 30), "fsig_c": fsig_c,
            "pmu": t(K, seed=seed + 32), "psig_c": psig_c}


def run_loss_fused(recon, y, kl, seed=0):
    N, K = recon.numel(), kl["fmu"].numel()
    o = {"loss": garbage(1, seed=seed), "mse": garbage(1, seed=seed + 1),
         "kl": garbage(1, seed=seed + 2), "drecon": garbage(N, seed=seed + 3),
         "dfmu": garbage(K, seed=seed + 4),
         "dfsig_c": garbage(K, seed=seed + 5),
         "dpmu": garbage(K, seed=seed + 6),
         "dpsig_c": garbage(K, seed=seed + 7)}
    ext.loss_fused(recon, y, kl["fmu"], kl["fsig_c"], kl["pmu"],
                   kl["psig_c"], o["loss"], o["mse"], o["kl"], o["drecon"],
                   o["dfmu"], o["dfsig_c"], o["dpmu"], o["dpsig_c"], 1.0)
    return o


# ---------------------------------------------------------------- decoder
DEC_ROW_OUTS = (("recon", "N"), ("a1", "NH"), ("beta", "NK"),
                ("asig_pre", "N"), ("sigma", "N"), ("drecon", "N"),
                ("dh", "NH"), ("dz1", "NH"), ("dbeta", "NK"))
DEC_HEAD_OUTS = ("dwmu", "dbmu", "dwsig", "dbsig")


def dec_inputs(N, K, H, zero_eps=False):
    i = {"h": t(N, H, seed=1), "W1": t(H, H, seed=2, scale=H ** -0.5),
         "b1": t(H, seed=3), "wmu": t(H, seed=4, scale=H ** -0.5),
         "bmu": t(1, seed=5), "wsig": t(H, seed=6, scale=H ** -0.5),
         "bsig": t(1, seed=7), "Wb": t(K, H, seed=8, scale=H ** -0.5),
         "bb": t(K, seed=9), "y": t(N, 1, seed=10),
         "eps": torch.zeros(N, device=DEV) if zero_eps else t(N, seed=11)}
    i.update(kl_inputs(K))
    return i


def dec_shape(code, N, K, H):
    return {"N": (N,), "NH": (N, H), "NK": (N, K)}[code]


def run_dec_old(i, N, K, H, seed):
    """dec_fwd -> loss_fused -> dec_bwd (+ its reduce)."""
    o = {name: garbage(*dec_shape(code, N, K, H), seed=seed + j)
         for j, (name, code) in enumerate(DEC_ROW_OUTS)}
    o["part"] = garbage(dec_nblk(N) * (2 * K + 2 * H + 2), seed=seed + 20)
    o["dwmu"], o["dwsig"] = garbage(H, seed=seed + 21), garbage(H, seed=seed + 22)
    o["dbmu"], o["dbsig"] = garbage(1, seed=seed + 23), garbage(1, seed=seed + 24)
    ext.dec_fwd(i["h"], i["W1"], i["b1"], i["wmu"], i["bmu"], i["wsig"],
                i["bsig"], i["Wb"], i["bb"], i["fmu"], i["fsig_c"], i["eps"],
                o["recon"], o["a1"], o["beta"], o["asig_pre"], o["sigma"])
    lo = run_loss_fused(o["recon"], i["y"], i, seed + 30)
    o["drecon"] = lo["drecon"]
    ext.dec_bwd(o["drecon"], i["h"], o["a1"], o["beta"], o["asig_pre"],
                o["sigma"], i["eps"], i["fmu"], i["fsig_c"], i["W1"],
                i["wmu"], i["wsig"], i["Wb"], o["dh"], o["dz1"], o["dbeta"],
                o["part"], lo["dfmu"], lo["dfsig_c"], o["dwmu"], o["dbmu"],
                o["dwsig"], o["dbsig"])
    # what the sequence hands on: the final factor gradients, the loss
    # scalars and the predictor's KL gradients
    extra = {k: lo[k] for k in ("loss", "mse", "kl", "dfmu", "dfsig_c",
                                "dpmu", "dpsig_c")}
    return o, extra


def run_dec_new(i, N, K, H, seed):
    """dec_fwd_bwd, then the head-gradient reduce."""
    o = {name: garbage(*dec_shape(code, N, K, H), seed=seed + j)
         for j, (name, code) in enumerate(DEC_ROW_OUTS)}
    o["part"] = garbage(dec_nblk(N) * (2 * K + 2 * H + 2), seed=seed + 20)
    o["dwmu"], o["dwsig"] = garbage(H, seed=seed + 21), garbage(H, seed=seed + 22)
    o["dbmu"], o["dbsig"] = garbage(1, seed=seed + 23), garbage(1, seed=seed + 24)
    ext.dec_fwd_bwd(i["h"], i["W1"], i["b1"], i["wmu"], i["bmu"], i["wsig"],
                    i["bsig"], i["Wb"], i["bb"], i["fmu"], i["fsig_c"],
                    i["eps"], i["y"], o["recon"], o["a1"], o["beta"],
                    o["asig_pre"], o["sigma"], o["drecon"], o["dh"], o["dz1"],
                    o["dbeta"], o["part"], 1.0)
    ext.dec_bwd_reduce_heads(o["part"], o["dwmu"], o["dbmu"], o["dwsig"],
                             o["dbsig"], N, K)
    return o


# N: one row; short of / exactly / one past one block's four rows; two
# blocks' worth plus one; the benchmark's; iters = 2; the iters = 8 cap with
# 129 blocks. K = 65 uses the k >= 64 accumulators.
@pytest.mark.parametrize("zero_eps", [False, True])
@pytest.mark.parametrize("H", [64, 20])
@pytest.mark.parametrize("K", [1, 20, 65, 128])
@pytest.mark.parametrize("N", [1, 3, 4, 5, 257, 300, 513, 4100])
def test_dec_fwd_bwd_bits(N, K, H, zero_eps):
    i = dec_inputs(N, K, H, zero_eps)
    assert float(i["fsig_c"].min()) == pytest.approx(1e-6)
    old, _ = run_dec_old(i, N, K, H, 100)
    new = run_dec_new(i, N, K, H, 200)
    torch.cuda.synchronize()
    assert_bits(new, old, f"dec N={N} K={K} H={H} zero_eps={zero_eps}")


def test_dec_fwd_bwd_unaligned_weights():
    """W1 and Wb 4 bytes off a 16-byte boundary, as views into the packed
    parameter arena may be: the scalar path of the staging loads."""
    N, K, H = 300, 20, 64
    i = dec_inputs(N, K, H)
    for name in ("W1", "Wb"):
        buf = torch.empty(i[name].numel() + 1, device=DEV)
        v = buf[1:].view(i[name].shape)
        v.copy_(i[name])
        assert v.data_ptr() % 16 == 4
        i[name] = v
    old, _ = run_dec_old(i, N, K, H, 100)
    new = run_dec_new(i, N, K, H, 200)
    torch.cuda.synchronize()
    assert_bits(new, old, "dec unaligned")


# ---------------------------------------------------------------- encoder
# decoder rows that give each block count
NBLK_ROWS = {1: 4, 63: 252, 64: 256, 65: 260, 75: 300, 129: 4100}


@functools.lru_cache(maxsize=None)
def dec_reference(nblk, K):
    """The old decoder sequence once per (nblk, K): its block partials and
    what loss_fused and dec_bwd_reduce made of them. Read-only."""
    Nd, H = NBLK_ROWS[nblk], 64
    assert dec_nblk(Nd) == nblk
    i = dec_inputs(Nd, K, H)
    old, extra = run_dec_old(i, Nd, K, H, 100)
    torch.cuda.synchronize()
    return i, old["part"], extra


@pytest.mark.parametrize("N", [1, 257, 300])
@pytest.mark.parametrize("K", [1, 20, 128])
@pytest.mark.parametrize("M", [1, 3, 128])
@pytest.mark.parametrize("nblk", sorted(NBLK_ROWS))
def test_enc_bwd_mid_bits(nblk, M, K, N):
    di, part, extra = dec_reference(nblk, K)
    fsig = di["fsig_c"].clone()
    fsig[K // 2] = 0.0  # the factor whose fsig_c is the 1e-6 clamp
    i = {"fsig": fsig, "fsig_pre": t(K, seed=40), "yp": t(M, seed=41),
         "Wmu": t(K, M, seed=42, scale=M ** -0.5),
         "Wsig": t(K, M, seed=43, scale=M ** -0.5),
         "a": torch.softmax(t(N, M, seed=44), dim=0).contiguous(),
         "y": t(N, 1, seed=45)}

    def outs(seed):
        return {"dscores": garbage(N, M, seed=seed),
                "dWmu": garbage(K, M, seed=seed + 1),
                "dbmu": garbage(K, seed=seed + 2),
                "dWsig": garbage(K, M, seed=seed + 3),
                "dbsig": garbage(K, seed=seed + 4)}

    old = outs(300)
    ext.enc_bwd_fused(extra["dfmu"], extra["dfsig_c"], i["fsig"],
                      i["fsig_pre"], i["yp"], i["Wmu"], i["Wsig"], i["a"],
                      i["y"], old["dscores"], old["dWmu"], old["dbmu"],
                      old["dWsig"], old["dbsig"])
    old["dfmu"], old["dfsig_c"] = extra["dfmu"], extra["dfsig_c"]
    new = outs(400)
    new["dfmu"], new["dfsig_c"] = garbage(K, seed=405), garbage(K, seed=406)
    ext.enc_bwd_mid(part, nblk, di["fmu"], di["fsig_c"], di["pmu"],
                    di["psig_c"], i["fsig"], i["fsig_pre"], i["yp"], i["Wmu"],
                    i["Wsig"], i["a"], i["y"], new["dscores"], new["dWmu"],
                    new["dbmu"], new["dWsig"], new["dbsig"], new["dfmu"],
                    new["dfsig_c"], 1.0)
    torch.cuda.synchronize()
    assert_bits(new, old, f"enc nblk={nblk} M={M} K={K} N={N}")


# -------------------------------------------------------------- attention
ATT_BWD_OUTS = (("dz2", "KH"), ("du", "KH"), ("ds", "NK"), ("dc", "K"),
                ("dWv", "KHH"), ("dbv", "KH"), ("dq", "KH"), ("dWk", "KHH"),
                ("dbk", "KH"), ("hpart", "E"), ("dwmu", "H"), ("dbmu", "1"),
                ("dwsig", "H"), ("dbsig", "1"))


def att_shape(code, N, H, K):
    return {"NK": (N, K), "KH": (K, H), "K": (K,), "KHH": (K, H, H),
            "E": (K * (2 * H + 2),), "H": (H,), "1": (1,)}[code]


def attn_state(N, H, K, with_mask):
    """Inputs of the attention backward and its forward's outputs."""
    g = torch.Generator(device="cpu").manual_seed(4)
    i = {"h": t(N, H, seed=1), "qk": t(K, H, seed=2, scale=H ** -0.5),
         "cb": t(K, seed=3),
         "mask": ((torch.rand(N, K, generator=g) >= 0.1).float().to(DEV)
                  if with_mask else None),
         "Wv": t(K, H, H, seed=5, scale=H ** -0.5), "bv": t(K, H, seed=6),
         "Wl": t(H, H, seed=7, scale=H ** -0.5), "bl": t(H, seed=8),
         "wmu": t(H, seed=9, scale=H ** -0.5), "bmu": t(1, seed=10),
         "wsig": t(H, seed=11, scale=H ** -0.5), "bsig": t(1, seed=12),
         "q": t(K, H, seed=13), "Wk": t(K, H, H, seed=14, scale=H ** -0.5),
         "bk": t(K, H, seed=15)}
    f = {"a": garbage(N, K, seed=50), "sd": garbage(N, K, seed=51),
         "guard": torch.full((K,), 777, dtype=torch.int32, device=DEV),
         "u": garbage(K, H, seed=52), "ctx": garbage(K, H, seed=53),
         "hm2": garbage(K, H, seed=54), "pmu": garbage(K, seed=55),
         "psig_pre": garbage(K, seed=56), "psig": garbage(K, seed=57),
         "psig_c": garbage(K, seed=58)}
    ext.attn_fused_fwd(i["h"], i["qk"], i["cb"], i["mask"], i["Wv"], i["bv"],
                       i["Wl"], i["bl"], i["wmu"], i["bmu"], i["wsig"],
                       i["bsig"], f["a"], f["sd"], f["guard"], f["u"],
                       f["ctx"], f["hm2"], f["pmu"], f["psig_pre"], f["psig"],
                       f["psig_c"], H ** -0.5, KEEP_INV, 1)
    return i, f


def run_attn_bwd(i, f, dpmu, dpsig_c, N, H, K, seed, kl=None):
    o = {name: garbage(*att_shape(code, N, H, K), seed=seed + j)
         for j, (name, code) in enumerate(ATT_BWD_OUTS)}
    extra = () if kl is None else (kl["fmu"], kl["fsig_c"], kl["pmu"],
                                   kl["psig_c"], 1.0)
    ext.attn_fused_bwd(dpmu, dpsig_c, f["psig"], f["psig_pre"], f["hm2"],
                       i["wmu"], i["wsig"], i["Wl"], i["h"], f["a"], f["sd"],
                       i["mask"], f["guard"], f["u"], i["Wv"], i["q"],
                       i["Wk"], i["bk"], o["dz2"], o["du"], o["ds"], o["dc"],
                       o["dWv"], o["dbv"], o["dq"], o["dWk"], o["dbk"],
                       o["hpart"], o["dwmu"], o["dbmu"], o["dwsig"],
                       o["dbsig"], H ** -0.5, KEEP_INV, 1, *extra)
    o["dpmu"], o["dpsig_c"] = dpmu, dpsig_c
    return o


def check_attn_kl(N, H, K, with_mask, zero_psig=None, guarded=None):
    i, f = attn_state(N, H, K, with_mask)
    if zero_psig is not None:
        f["psig"][zero_psig] = 0.0
        f["psig_c"][zero_psig] = 1e-6
    if guarded is not None:
        f["guard"][guarded] = 1
    kl = kl_inputs(K)
    kl["pmu"], kl["psig_c"] = f["pmu"], f["psig_c"]
    recon, y = t(N, seed=60), t(N, 1, seed=61)
    lo = run_loss_fused(recon, y, kl, 70)
    old = run_attn_bwd(i, f, lo["dpmu"], lo["dpsig_c"], N, H, K, 300)
    new = run_attn_bwd(i, f, garbage(K, seed=80), garbage(K, seed=81), N, H,
                       K, 400, kl=kl)
    torch.cuda.synchronize()
    assert_bits(new, old, f"attn N={N} H={H} K={K} mask={with_mask} "
                f"zero_psig={zero_psig} guarded={guarded}")


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("H", [64, 20])
@pytest.mark.parametrize("N", [1, 3, 256, 257, 300, 384])
def test_attn_bwd_kl_in_kernel_bits(N, H, K, with_mask):
    check_attn_kl(N, H, K, with_mask)


@pytest.mark.parametrize("with_mask", [False, True])
def test_attn_bwd_kl_zero_psig_and_guard(with_mask):
    check_attn_kl(300, 64, 20, with_mask, zero_psig=3)
    check_attn_kl(300, 64, 20, with_mask, guarded=7)
    check_attn_kl(257, 20, 20, with_mask, zero_psig=0, guarded=19)


def test_attn_bwd_kl_needs_the_latency_kernel():
    """variant 0 has no in-kernel KL gradients: an error, not a fallback."""
    N, H, K = 33, 64, 2
    i, f = attn_state(N, H, K, False)
    kl = kl_inputs(K)
    o = {name: garbage(*att_shape(code, N, H, K), seed=j)
         for j, (name, code) in enumerate(ATT_BWD_OUTS)}
    with pytest.raises(RuntimeError):
        ext.attn_fused_bwd(garbage(K), garbage(K), f["psig"], f["psig_pre"],
                           f["hm2"], i["wmu"], i["wsig"], i["Wl"], i["h"],
                           f["a"], f["sd"], None, f["guard"], f["u"], i["Wv"],
                           i["q"], i["Wk"], i["bk"], o["dz2"], o["du"],
                           o["ds"], o["dc"], o["dWv"], o["dbv"], o["dq"],
                           o["dWk"], o["dbk"], o["hpart"], o["dwmu"],
                           o["dbmu"], o["dwsig"], o["dbsig"], H ** -0.5,
                           KEEP_INV, 0, kl["fmu"], kl["fsig_c"], kl["pmu"],
                           kl["psig_c"], 1.0)


# ------------------------------------------------ KL helper, loss scalars
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_kl_helper_matches_loss_fused(seed):
    """kl_grad_ as enc_bwd_mid (dfmu, dfsig_c: zero partials, so the sum
    adds +0) and attn_fused_bwd (dpmu, dpsig_c) use it, K = 128 factors."""
    K, N, M, H = 128, 5, 2, 64
    kl = kl_inputs(K, seed=100 * seed)
    assert float(kl["fsig_c"].min()) == pytest.approx(1e-6)
    assert float(kl["psig_c"].min()) == pytest.approx(1e-6)
    lo = run_loss_fused(t(N, seed=1), t(N, 1, seed=2), kl, 10)
    # a zero-filled partial array: s_k = +0, and x + 0 == x
    nblk = 2
    part = torch.zeros(nblk * (2 * K + 2 * H + 2), device=DEV)
    new = {"dfmu": garbage(K, seed=20), "dfsig_c": garbage(K, seed=21)}
    ext.enc_bwd_mid(part, nblk, kl["fmu"], kl["fsig_c"], kl["pmu"],
                    kl["psig_c"], kl["fsig_c"], t(K, seed=3), t(M, seed=4),
                    t(K, M, seed=5), t(K, M, seed=6),
                    torch.softmax(t(N, M, seed=7), dim=0).contiguous(),
                    t(N, 1, seed=8), garbage(N, M), garbage(K, M),
                    garbage(K), garbage(K, M), garbage(K), new["dfmu"],
                    new["dfsig_c"], 1.0)
    torch.cuda.synchronize()
    # -0 + +0 = +0: compare values where loss_fused gave a signed zero
    for name in ("dfmu", "dfsig_c"):
        ref = lo[name] + 0.0
        assert_bits({name: new[name]}, {name: ref}, f"kl helper seed={seed}")

    # dpmu / dpsig_c through one head-per-factor attention backward launch
    Na, Ha = 3, 20
    i, f = attn_state(Na, Ha, K, False)
    got = run_attn_bwd(i, f, garbage(K, seed=30), garbage(K, seed=31), Na, Ha,
                       K, 400, kl=kl)
    torch.cuda.synchronize()
    assert_bits({"dpmu": got["dpmu"], "dpsig_c": got["dpsig_c"]},
                {"dpmu": lo["dpmu"], "dpsig_c": lo["dpsig_c"]},
                f"kl helper seed={seed}")


@pytest.mark.parametrize("N,K", [(1, 1), (300, 20), (4100, 128)])
def test_loss_scalars_match_loss_fused(N, K):
    kl = kl_inputs(K)
    recon, y = t(N, seed=1), t(N, 1, seed=2)
    lo = run_loss_fused(recon, y, kl, 10)
    new = {k: garbage(1, seed=20 + j)
           for j, k in enumerate(("loss", "mse", "kl"))}
    ext.loss_scalars(recon, y, kl["fmu"], kl["fsig_c"], kl["pmu"],
                     kl["psig_c"], new["loss"], new["mse"], new["kl"])
    torch.cuda.synchronize()
    assert_bits(new, {k: lo[k] for k in new}, f"loss scalars N={N} K={K}")


# ------------------------------------------------------ through the engine
def _trainer(monkeypatch, chain, dtype, train, use_graph=False):
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    if chain is None:
        monkeypatch.delenv("FV_MID_CHAIN", raising=False)
    else:
        monkeypatch.setenv("FV_MID_CHAIN", chain)
    monkeypatch.delenv("FV_MID", raising=False)
    set_seed(0)
    model = build_factorvae(num_latent=158, hidden_size=64, num_portfolio=128,
                            num_factor=20).to(DEV)
    tr = FusedTrainer(model, lr=1e-4, t_max=100, device=DEV,
                      use_graph=use_graph, train=train, dtype=dtype)
    assert tr._mid_chain == (chain != "0")
    return tr


STEP_WS = ("loss", "mse", "kl", "recon", "drecon", "dfmu", "dfsig_c", "dpmu",
           "dpsig_c", "a1", "beta", "asig_pre", "sigma", "dscores")


def _one_step(tr, x, y, noise, expect_chain):
    """Forward, backward and Adam with fixed inputs and noise, launched as
    the training step launches them; everything the step produces."""
    N, T, _ = x.shape
    tr._ensure_ws(N, T)
    w = tr.ws
    w["x"].copy_(x)
    w["y"].copy_(y)
    if not noise:
        tr._fill_rng(N)
        noise["eps"], noise["mask"] = w["eps"].clone(), w["mask"].clone()
    w["eps"].copy_(noise["eps"])
    w["mask"].copy_(noise["mask"])
    tr.grads.zero_()
    for k in STEP_WS:
        w[k].fill_(7.0)
    tr._launch_forward(N, T, train=True)
    assert tr._chain_pending == expect_chain
    tr._launch_backward(N, T)
    assert not tr._chain_pending
    torch.cuda.synchronize()
    out = {f"ws {k}": w[k].clone() for k in STEP_WS}
    out.update({f"grad {name}": tr.g(name).clone()
                for name, _, _ in tr._param_specs()})
    tr._launch_optimizer()
    torch.cuda.synchronize()
    out["params after adam"] = tr.params.flat.clone()
    return out


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("N,T", [(33, 3), (300, 20)])
def test_chain_matches_old_sequence_over_a_step(monkeypatch, N, T, dtype,
                                                train):
    """FV_MID_CHAIN=0 against the default over one whole step (losses,
    recon, the loss gradients, every gradient slot, parameters after Adam),
    then forward_only and predict."""
    x, y = t(N, T, 158, seed=50), t(N, 1, seed=51)
    noise = {}
    tr_off = _trainer(monkeypatch, "0", dtype, train)
    off = _one_step(tr_off, x, y, noise, False)
    tr_on = _trainer(monkeypatch, None, dtype, train)
    on = _one_step(tr_on, x, y, noise, True)
    assert_bits(on, off, f"step N={N} {dtype} train={train}")

    res = {}
    for key, tr in (("off", tr_off), ("on", tr_on)):
        torch.manual_seed(7)
        val = tr.forward_only(x, y).clone()
        val_recon = tr.ws["recon"].clone()
        torch.manual_seed(8)
        res[key] = {"forward_only loss": val, "forward_only recon": val_recon,
                    "predict": tr.predict(x)}
    torch.cuda.synchronize()
    assert_bits(res["on"], res["off"], f"N={N} {dtype} train={train}")


def test_old_call_order_still_takes_the_old_sequence(monkeypatch):
    """_launch_forward without train=True runs dec_fwd and loss_fused
    itself, and the backward that follows must not run the chain."""
    N, T = 33, 3
    x, y = t(N, T, 158, seed=50), t(N, 1, seed=51)
    noise = {}
    tr = _trainer(monkeypatch, None, "fp32", True)
    on = _one_step(tr, x, y, noise, True)
    tr2 = _trainer(monkeypatch, None, "fp32", True)
    tr2._ensure_ws(N, T)
    w = tr2.ws
    w["x"].copy_(x)
    w["y"].copy_(y)
    w["eps"].copy_(noise["eps"])
    w["mask"].copy_(noise["mask"])
    tr2._launch_forward(N, T)
    assert not tr2._chain_pending
    tr2._launch_backward(N, T)
    torch.cuda.synchronize()
    got = {f"grad {name}": tr2.g(name).clone()
           for name, _, _ in tr2._param_specs()}
    got["ws loss"] = w["loss"].clone()
    assert_bits(got, {k: on[k] for k in got}, "old call order")


def test_larger_days_keep_the_old_sequence(monkeypatch):
    """N = 385 is past the fused attention backward: old sequence, equal
    to FV_MID_CHAIN=0."""
    N, T = 385, 2
    x, y = t(N, T, 158, seed=52), t(N, 1, seed=53)
    noise = {}
    off = _one_step(_trainer(monkeypatch, "0", "fp32", True), x, y, noise,
                    False)
    on = _one_step(_trainer(monkeypatch, None, "fp32", True), x, y, noise,
                   False)
    assert_bits(on, off, "N=385")


def test_five_graph_steps_are_deterministic(monkeypatch):
    """Two identically seeded runs of 5 captured steps: identical
    parameter bits and losses, and the loss is the chain's own."""
    N, T = 300, 20
    x, y = t(N, T, 158, seed=54), t(N, 1, seed=55)
    runs = []
    for _ in range(2):
        tr = _trainer(monkeypatch, None, "fp32", True, use_graph=True)
        torch.manual_seed(11)
        losses = [tr.step(x, y).clone() for _ in range(5)]
        torch.cuda.synchronize()
        runs.append({"params": tr.params.flat.clone(),
                     "losses": torch.cat(losses)})
    assert_bits(runs[1], runs[0], "5 steps")
    assert torch.isfinite(runs[0]["losses"]).all()
