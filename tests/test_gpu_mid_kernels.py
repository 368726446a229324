"""The latency-oriented attn_fused_fwd / attn_fused_bwd / enc_fused_fwd
kernels (variant=1, the default) against the original kernels
(variant=0) on the same inputs: every output equal by bit pattern, at the
kernels and over one whole step (FV_MID=0 against the default)."""

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


def garbage(shape, seed, dtype=torch.float32):
    # garbage-filled outputs: a store a kernel misses shows as a difference
    if dtype == torch.int32:
        return torch.full(shape, 12345 + seed, dtype=dtype, device=DEV)
    return t(*shape, seed=seed) + 3.0


def assert_bits(new, old, what):
    assert set(new) == set(old)
    for name in sorted(old):
        a, b = new[name], old[name]
        assert a.dtype == b.dtype and a.shape == b.shape
        ai = a.contiguous().view(torch.int32)
        bi = b.contiguous().view(torch.int32)
        assert torch.equal(ai, bi), (
            f"{what} {name}: {(ai != bi).sum().item()} of {bi.numel()} "
            f"bit patterns differ")


def dropout_mask(N, K, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(N, K, generator=g) >= 0.1).float().to(DEV)


# ------------------------------------------------------------ attention
def attn_inputs(N, H, K, with_mask, special=None):
    """special: None or (head, value) written to cb[head] — +inf / NaN
    there makes every score of that head, and of no other, inf / NaN."""
    i = {"h": t(N, H, seed=1), "qk": t(K, H, seed=2, scale=H ** -0.5),
         "cb": t(K, seed=3),
         "mask": dropout_mask(N, K, 4) if with_mask else None,
         "Wv": t(K, H, H, seed=5, scale=H ** -0.5), "bv": t(K, H, seed=6),
         "Wl": t(H, H, seed=7, scale=H ** -0.5), "bl": t(H, seed=8),
         "wmu": t(H, seed=9, scale=H ** -0.5), "bmu": t(1, seed=10),
         "wsig": t(H, seed=11, scale=H ** -0.5), "bsig": t(1, seed=12),
         "q": t(K, H, seed=13), "Wk": t(K, H, H, seed=14, scale=H ** -0.5),
         "bk": t(K, H, seed=15), "dpmu": t(K, seed=16),
         "dpsig_c": t(K, seed=17)}
    if special is not None:
        i["cb"][special[0]] = special[1]
    return i


FWD_OUTS = (("a", "NK"), ("sd", "NK"), ("guard", "Ki"), ("u", "KH"),
            ("ctx", "KH"), ("hm2", "KH"), ("pmu", "K"), ("psig_pre", "K"),
            ("psig", "K"), ("psig_c", "K"))


def shape_of(code, N, H, K):
    return {"NK": (N, K), "KH": (K, H), "K": (K,), "Ki": (K,),
            "KHH": (K, H, H), "E": (K * (2 * H + 2),), "H": (H,),
            "1": (1,)}[code]


def run_attn_fwd(i, N, H, K, variant, seed):
    o = {name: garbage(shape_of(code, N, H, K), seed + j,
                       torch.int32 if code == "Ki" else torch.float32)
         for j, (name, code) in enumerate(FWD_OUTS)}
    ext.attn_fused_fwd(i["h"], i["qk"], i["cb"], i["mask"], i["Wv"], i["bv"],
                       i["Wl"], i["bl"], i["wmu"], i["bmu"], i["wsig"],
                       i["bsig"], o["a"], o["sd"], o["guard"], o["u"],
                       o["ctx"], o["hm2"], o["pmu"], o["psig_pre"], o["psig"],
                       o["psig_c"], H ** -0.5, KEEP_INV, variant)
    return o


BWD_OUTS = (("dz2", "KH"), ("du", "KH"), ("ds", "NK"), ("dc", "K"),
            ("dWv", "KHH"), ("dbv", "KH"), ("dq", "KH"), ("dWk", "KHH"),
            ("dbk", "KH"), ("hpart", "E"), ("dwmu", "H"), ("dbmu", "1"),
            ("dwsig", "H"), ("dbsig", "1"))


def run_attn_bwd(i, f, N, H, K, variant, seed):
    o = {name: garbage(shape_of(code, N, H, K), seed + j)
         for j, (name, code) in enumerate(BWD_OUTS)}
    ext.attn_fused_bwd(i["dpmu"], i["dpsig_c"], f["psig"], f["psig_pre"],
                       f["hm2"], i["wmu"], i["wsig"], i["Wl"], i["h"], f["a"],
                       f["sd"], i["mask"], f["guard"], f["u"], i["Wv"],
                       i["q"], i["Wk"], i["bk"], o["dz2"], o["du"], o["ds"],
                       o["dc"], o["dWv"], o["dbv"], o["dq"], o["dWk"],
                       o["dbk"], o["hpart"], o["dwmu"], o["dbmu"], o["dwsig"],
                       o["dbsig"], H ** -0.5, KEEP_INV, variant)
    return o


# N: one row; fewer rows than one wave's four-way split; exactly the 256
# first rows; one row in the second set; the benchmark's; the forward limit
FWD_N = [1, 3, 256, 257, 300, 448]
BWD_N = [1, 3, 256, 257, 300, 384]


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("H", [64, 32, 20])
@pytest.mark.parametrize("N", FWD_N)
def test_attn_fwd_bits(N, H, K, with_mask):
    i = attn_inputs(N, H, K, with_mask)
    old = run_attn_fwd(i, N, H, K, 0, 100)
    new = run_attn_fwd(i, N, H, K, 1, 200)
    torch.cuda.synchronize()
    assert int(old["guard"].abs().sum()) == 0
    assert_bits(new, old, f"fwd N={N} H={H} K={K} mask={with_mask}")


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
@pytest.mark.parametrize("with_mask", [False, True])
def test_attn_fwd_guarded_head(value, with_mask):
    """One head's scores +inf or NaN: guard set for that head only."""
    N, H, K, head = 300, 64, 20, 7
    i = attn_inputs(N, H, K, with_mask, special=(head, value))
    old = run_attn_fwd(i, N, H, K, 0, 100)
    new = run_attn_fwd(i, N, H, K, 1, 200)
    torch.cuda.synchronize()
    want = torch.zeros(K, dtype=torch.int32, device=DEV)
    want[head] = 1
    assert torch.equal(old["guard"], want)
    assert torch.equal(new["guard"], want)
    assert_bits(new, old, f"fwd guarded {value} mask={with_mask}")


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("H", [64, 32, 20])
@pytest.mark.parametrize("N", BWD_N)
def test_attn_bwd_bits(N, H, K, with_mask):
    i = attn_inputs(N, H, K, with_mask)
    f = run_attn_fwd(i, N, H, K, 0, 100)
    old = run_attn_bwd(i, f, N, H, K, 0, 300)
    new = run_attn_bwd(i, f, N, H, K, 1, 400)
    torch.cuda.synchronize()
    assert_bits(new, old, f"bwd N={N} H={H} K={K} mask={with_mask}")


@pytest.mark.parametrize("N,H", [(300, 64), (257, 20)])
@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_attn_bwd_guarded_head(value, N, H):
    K, head = 20, 7
    i = attn_inputs(N, H, K, True, special=(head, value))
    f = run_attn_fwd(i, N, H, K, 0, 100)
    old = run_attn_bwd(i, f, N, H, K, 0, 300)
    new = run_attn_bwd(i, f, N, H, K, 1, 400)
    torch.cuda.synchronize()
    assert int(f["guard"][head]) == 1 and int(f["guard"].sum()) == 1
    assert float(old["ds"][:, head].abs().sum()) == 0.0
    assert_bits(new, old, f"bwd guarded {value} N={N} H={H}")


@pytest.mark.parametrize("N,H,K", [(5, 6, 3), (257, 63, 2), (300, 1, 2)])
def test_attn_h_not_multiple_of_four(N, H, K):
    """H % 4 != 0: the element-wise staging path."""
    i = attn_inputs(N, H, K, True)
    fo = run_attn_fwd(i, N, H, K, 0, 100)
    fn = run_attn_fwd(i, N, H, K, 1, 200)
    old = run_attn_bwd(i, fo, N, H, K, 0, 300)
    new = run_attn_bwd(i, fo, N, H, K, 1, 400)
    torch.cuda.synchronize()
    assert_bits(fn, fo, f"fwd N={N} H={H}")
    assert_bits(new, old, f"bwd N={N} H={H}")


def test_attn_unaligned_views():
    """Weights and gradient slots that start 4 bytes off a 16-byte
    boundary (as views into a packed arena may): the scalar load / store
    paths of the staging helpers."""
    N, H, K = 300, 64, 3
    i = attn_inputs(N, H, K, True)

    def off1(x):
        buf = torch.empty(x.numel() + 1, device=DEV)
        v = buf[1:].view(x.shape)
        v.copy_(x)
        assert v.data_ptr() % 16 == 4
        return v

    for name in ("h", "Wv", "Wl", "Wk"):
        i[name] = off1(i[name])
    fo = run_attn_fwd(i, N, H, K, 0, 100)
    fn = run_attn_fwd(i, N, H, K, 1, 200)
    res = {}
    for variant, seed in ((0, 300), (1, 400)):
        o = {name: garbage(shape_of(code, N, H, K), seed + j)
             for j, (name, code) in enumerate(BWD_OUTS)}
        o["dWv"], o["dWk"] = off1(o["dWv"]), off1(o["dWk"])
        ext.attn_fused_bwd(i["dpmu"], i["dpsig_c"], fo["psig"],
                           fo["psig_pre"], fo["hm2"], i["wmu"], i["wsig"],
                           i["Wl"], i["h"], fo["a"], fo["sd"], i["mask"],
                           fo["guard"], fo["u"], i["Wv"], i["q"], i["Wk"],
                           i["bk"], o["dz2"], o["du"], o["ds"], o["dc"],
                           o["dWv"], o["dbv"], o["dq"], o["dWk"], o["dbk"],
                           o["hpart"], o["dwmu"], o["dbmu"], o["dwsig"],
                           o["dbsig"], H ** -0.5, KEEP_INV, variant)
        res[variant] = o
    torch.cuda.synchronize()
    assert_bits(fn, fo, "fwd unaligned")
    assert_bits(res[1], res[0], "bwd unaligned")


# -------------------------------------------------------------- encoder
ENC_OUTS = ("scores", "a", "yp", "fmu", "fsig_pre", "fsig", "fsig_c")


def run_enc(i, N, M, K, variant, seed, heads, done):
    o = {"scores": garbage((N, M), seed), "a": garbage((N, M), seed + 1),
         "yp": garbage((M,), seed + 2)}
    for j, name in enumerate(ENC_OUTS[3:]):
        o[name] = garbage((K,), seed + 3 + j)
    if heads:
        ext.enc_fused_fwd(i["h"], i["Wenc"], i["benc"], i["y"], o["scores"],
                          o["a"], o["yp"], i["Wmu"], i["bmu"], i["Wsig"],
                          i["bsig"], o["fmu"], o["fsig_pre"], o["fsig"],
                          o["fsig_c"], done, variant)
    else:
        ext.enc_fused_fwd(i["h"], i["Wenc"], i["benc"], i["y"], o["scores"],
                          o["a"], o["yp"], variant=variant)
    return o


ENC_GRID = [(N, M, K, H) for N in (1, 257, 300) for M in (1, 3, 128)
            for K in (1, 20) for H in (64, 20)]
# H % 4 != 0 (runs the original kernel under either variant); K*M above
# 4096, where Wmu / Wsig are loaded in the heads tail, not prefetched
ENC_GRID += [(257, 5, 3, 63), (3, 128, 20, 6), (300, 128, 40, 32)]


@pytest.mark.parametrize("heads", [True, False])
@pytest.mark.parametrize("N,M,K,H", ENC_GRID)
def test_enc_fwd_bits(N, M, K, H, heads):
    i = {"h": t(N, H, seed=1), "Wenc": t(M, H, seed=2, scale=H ** -0.5),
         "benc": t(M, seed=3), "y": t(N, 1, seed=4),
         "Wmu": t(K, M, seed=5, scale=M ** -0.5), "bmu": t(K, seed=6),
         "Wsig": t(K, M, seed=7, scale=M ** -0.5), "bsig": t(K, seed=8)}
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    what = f"enc N={N} M={M} K={K} H={H} heads={heads}"
    old = run_enc(i, N, M, K, 0, 100, heads, done)
    torch.cuda.synchronize()
    assert int(done) == 0
    new1 = run_enc(i, N, M, K, 1, 200, heads, done)
    torch.cuda.synchronize()
    assert int(done) == 0, what
    # back to back, no host synchronisation between the two launches
    new2 = run_enc(i, N, M, K, 1, 300, heads, done)
    new3 = run_enc(i, N, M, K, 1, 400, heads, done)
    torch.cuda.synchronize()
    assert int(done) == 0, what
    if not heads:
        # the head outputs are not written: drop the garbage
        for o in (old, new1, new2, new3):
            for name in ENC_OUTS[3:]:
                del o[name]
    assert_bits(new1, old, what)
    assert_bits(new2, new1, what + " second launch")
    assert_bits(new3, new1, what + " third launch")


# -------------------------------------------------- through the engine
def _trainer(monkeypatch, mid, dtype, train, C=158, H=64, M=128, K=20):
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    if mid is None:
        monkeypatch.delenv("FV_MID", raising=False)
    else:
        monkeypatch.setenv("FV_MID", mid)
    set_seed(0)
    model = build_factorvae(num_latent=C, hidden_size=H, num_portfolio=M,
                            num_factor=K).to(DEV)
    tr = FusedTrainer(model, lr=1e-4, t_max=100, device=DEV, use_graph=False,
                      train=train, dtype=dtype)
    assert tr._mid == (0 if mid == "0" else 1)
    return tr


def _one_step(tr, x, y, noise):
    """Forward, backward and Adam with fixed inputs and noise; everything
    the step produces."""
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
    tr._launch_forward(N, T)
    tr._launch_backward(N, T)
    torch.cuda.synchronize()
    out = {f"out {k}": w[k].clone() for k in ("loss", "mse", "kl", "recon")}
    out.update({f"grad {name}": tr.g(name).clone()
                for name, _, _ in tr._param_specs()})
    tr._launch_optimizer()
    torch.cuda.synchronize()
    out["params after adam"] = tr.params.flat.clone()
    return out


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_mid_matches_old_kernels_over_a_step(monkeypatch, dtype, train):
    """FV_MID=0 against the default over one whole step (losses, recon,
    every gradient slot, parameters after Adam), then forward_only and
    predict."""
    N, T, C = 33, 3, 158
    x, y = t(N, T, C, seed=50), t(N, 1, seed=51)
    noise = {}
    tr_off = _trainer(monkeypatch, "0", dtype, train)
    off = _one_step(tr_off, x, y, noise)
    tr_on = _trainer(monkeypatch, None, dtype, train)
    on = _one_step(tr_on, x, y, noise)
    assert_bits(on, off, f"step {dtype} train={train}")

    res = {}
    for key, tr in (("off", tr_off), ("on", tr_on)):
        torch.manual_seed(7)
        val = tr.forward_only(x, y).clone()
        val_recon = tr.ws["recon"].clone()
        torch.manual_seed(8)
        res[key] = {"forward_only loss": val, "forward_only recon": val_recon,
                    "predict": tr.predict(x)}
    torch.cuda.synchronize()
    assert_bits(res["on"], res["off"], f"{dtype} train={train}")
