"""The fused middle (FV_MID_FUSE, docs/KERNELS.md) against the separate
kernels it is made of, on the same inputs, every output equal by bit pattern:
mid_fwd against attn_fused_fwd + enc_fused_fwd, mid_bwd (+ pred_head_reduce)
against attn_fused_bwd + dec_fwd_bwd, gru_bwd with the dh_combine operands
against dh_combine -> gru_bwd, whole steps with FV_MID_FUSE=0 against the
default, and the argument checks of the new bindings."""

import re

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


def off16(x):
    """x's values in storage that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(x.numel() + 1, device=DEV, dtype=x.dtype)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4
    return v


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


# ------------------------------------------------------ mid_fwd / mid_bwd
def mid_inputs(N, K, M, H, with_mask, zero_eps=False):
    g = torch.Generator(device="cpu").manual_seed(4)
    s = H ** -0.5
    return {
        "h": t(N, H, seed=1), "qk": t(K, H, seed=2, scale=s),
        "cb": t(K, seed=3),
        "mask": ((torch.rand(N, K, generator=g) >= 0.1).float().to(DEV)
                 if with_mask else None),
        "Wv": t(K, H, H, seed=5, scale=s), "bv": t(K, H, seed=6),
        "Wl": t(H, H, seed=7, scale=s), "bl": t(H, seed=8),
        "wmu_p": t(H, seed=9, scale=s), "bmu_p": t(1, seed=10),
        "wsig_p": t(H, seed=11, scale=s), "bsig_p": t(1, seed=12),
        "q": t(K, H, seed=13), "Wk": t(K, H, H, seed=14, scale=s),
        "bk": t(K, H, seed=15),
        "Wenc": t(M, H, seed=16, scale=s), "benc": t(M, seed=17),
        "y": t(N, 1, seed=18),
        "Wmu_e": t(K, M, seed=19, scale=M ** -0.5), "bmu_e": t(K, seed=20),
        "Wsig_e": t(K, M, seed=21, scale=M ** -0.5), "bsig_e": t(K, seed=22),
        "W1": t(H, H, seed=23, scale=s), "b1": t(H, seed=24),
        "wmu_d": t(H, seed=25, scale=s), "bmu_d": t(1, seed=26),
        "wsig_d": t(H, seed=27, scale=s), "bsig_d": t(1, seed=28),
        "Wb": t(K, H, seed=29, scale=s), "bb": t(K, seed=30),
        "eps": torch.zeros(N, device=DEV) if zero_eps else t(N, seed=31),
    }


def mid_outputs(N, K, M, H, seed):
    shapes = {
        # forward, attention role
        "a": (N, K), "sd": (N, K), "u": (K, H), "ctx": (K, H), "hm2": (K, H),
        "pmu": (K,), "psig_pre": (K,), "psig": (K,), "psig_c": (K,),
        # forward, encoder role
        "scores": (N, M), "a_enc": (N, M), "yp": (M,), "fmu": (K,),
        "fsig_pre": (K,), "fsig": (K,), "fsig_c": (K,),
        # backward, attention role
        "dz2": (K, H), "du": (K, H), "ds": (N, K), "dc": (K,),
        "dWv": (K, H, H), "dbv": (K, H), "dq": (K, H), "dWk": (K, H, H),
        "dbk": (K, H), "hpart": (K * (2 * H + 2),), "dwmu": (H,),
        "dbmu": (1,), "dwsig": (H,), "dbsig": (1,), "dpmu": (K,),
        "dpsig_c": (K,),
        # backward, decoder role
        "recon": (N,), "a1": (N, H), "beta": (N, K), "asig_pre": (N,),
        "sigma": (N,), "drecon": (N,), "dh": (N, H), "dz1": (N, H),
        "dbeta": (N, K),
        "part": (ext.dec_nblk(N) * (2 * K + 2 * H + 2),),
    }
    o = {name: garbage(*shape, seed=seed + j)
         for j, (name, shape) in enumerate(sorted(shapes.items()))}
    o["guard"] = torch.full((K,), 777, dtype=torch.int32, device=DEV)
    o["done"] = torch.zeros(1, dtype=torch.int32, device=DEV)
    return o


def fwd_separate(i, o, H):
    ext.attn_fused_fwd(i["h"], i["qk"], i["cb"], i["mask"], i["Wv"], i["bv"],
                       i["Wl"], i["bl"], i["wmu_p"], i["bmu_p"], i["wsig_p"],
                       i["bsig_p"], o["a"], o["sd"], o["guard"], o["u"],
                       o["ctx"], o["hm2"], o["pmu"], o["psig_pre"], o["psig"],
                       o["psig_c"], H ** -0.5, KEEP_INV, 1)
    ext.enc_fused_fwd(i["h"], i["Wenc"], i["benc"], i["y"], o["scores"],
                      o["a_enc"], o["yp"], i["Wmu_e"], i["bmu_e"],
                      i["Wsig_e"], i["bsig_e"], o["fmu"], o["fsig_pre"],
                      o["fsig"], o["fsig_c"], o["done"], 1)


def fwd_fused(i, o, H):
    return ext.mid_fwd(
        i["h"], i["qk"], i["cb"], i["mask"], i["Wv"], i["bv"], i["Wl"],
        i["bl"], i["wmu_p"], i["bmu_p"], i["wsig_p"], i["bsig_p"], o["a"],
        o["sd"], o["guard"], o["u"], o["ctx"], o["hm2"], o["pmu"],
        o["psig_pre"], o["psig"], o["psig_c"], i["Wenc"], i["benc"], i["y"],
        o["scores"], o["a_enc"], o["yp"], i["Wmu_e"], i["bmu_e"],
        i["Wsig_e"], i["bsig_e"], o["fmu"], o["fsig_pre"], o["fsig"],
        o["fsig_c"], o["done"], H ** -0.5, KEEP_INV)


def bwd_separate(i, o, H):
    ext.attn_fused_bwd(o["dpmu"], o["dpsig_c"], o["psig"], o["psig_pre"],
                       o["hm2"], i["wmu_p"], i["wsig_p"], i["Wl"], i["h"],
                       o["a"], o["sd"], i["mask"], o["guard"], o["u"],
                       i["Wv"], i["q"], i["Wk"], i["bk"], o["dz2"], o["du"],
                       o["ds"], o["dc"], o["dWv"], o["dbv"], o["dq"],
                       o["dWk"], o["dbk"], o["hpart"], o["dwmu"], o["dbmu"],
                       o["dwsig"], o["dbsig"], H ** -0.5, KEEP_INV, 1,
                       o["fmu"], o["fsig_c"], o["pmu"], o["psig_c"], 1.0)
    ext.dec_fwd_bwd(i["h"], i["W1"], i["b1"], i["wmu_d"], i["bmu_d"],
                    i["wsig_d"], i["bsig_d"], i["Wb"], i["bb"], o["fmu"],
                    o["fsig_c"], i["eps"], i["y"], o["recon"], o["a1"],
                    o["beta"], o["asig_pre"], o["sigma"], o["drecon"],
                    o["dh"], o["dz1"], o["dbeta"], o["part"], 1.0)


def bwd_fused(i, o, H, K):
    ran = ext.mid_bwd(
        o["psig"], o["psig_pre"], o["hm2"], i["wmu_p"], i["wsig_p"], i["Wl"],
        i["h"], o["a"], o["sd"], i["mask"], o["guard"], o["u"], i["Wv"],
        i["q"], i["Wk"], i["bk"], o["dz2"], o["du"], o["ds"], o["dc"],
        o["dWv"], o["dbv"], o["dq"], o["dWk"], o["dbk"], o["hpart"],
        o["fmu"], o["fsig_c"], o["pmu"], o["psig_c"], o["dpmu"],
        o["dpsig_c"], i["W1"], i["b1"], i["wmu_d"], i["bmu_d"], i["wsig_d"],
        i["bsig_d"], i["Wb"], i["bb"], i["eps"], i["y"], o["recon"], o["a1"],
        o["beta"], o["asig_pre"], o["sigma"], o["drecon"], o["dh"], o["dz1"],
        o["dbeta"], o["part"], H ** -0.5, KEEP_INV, 1.0)
    if ran:
        ext.pred_head_reduce(o["hpart"], o["dwmu"], o["dbmu"], o["dwsig"],
                             o["dbsig"], K, H)
    return ran


def check_mid(i, N, K, M, H, what):
    """Both launches against the separate kernels; returns the fused
    outputs."""
    old = mid_outputs(N, K, M, H, 100)
    fwd_separate(i, old, H)
    bwd_separate(i, old, H)
    new = mid_outputs(N, K, M, H, 300)
    assert fwd_fused(i, new, H)
    assert int(new["done"]) == 0
    assert bwd_fused(i, new, H, K)
    torch.cuda.synchronize()
    assert_bits(new, old, what)
    return new


# N: one row; short of / exactly / one past the decoder's four rows per
# block; one past a thread's first row (256); the benchmark's; the largest.
# H = 32, 20: rows narrower than a wave. M = 1, 3: the encoder's last
# arriver is the first or third; K = 1: one attention workgroup.
@pytest.mark.parametrize("H", [64, 32, 20])
@pytest.mark.parametrize("M", [1, 3, 128])
@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("N", [1, 3, 4, 5, 257, 300, 384])
def test_mid_bits(N, K, M, H):
    for with_mask in (False, True):
        i = mid_inputs(N, K, M, H, with_mask)
        check_mid(i, N, K, M, H,
                  f"mid N={N} K={K} M={M} H={H} mask={with_mask}")


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_mid_one_guarded_head(bad):
    """One head's scores +inf / NaN: the guard is set for that head only,
    and the backward's guarded path runs for it."""
    N, K, M, H = 300, 20, 128, 64
    i = mid_inputs(N, K, M, H, True)
    i["cb"][7] = bad
    new = check_mid(i, N, K, M, H, f"guarded {bad}")
    want = torch.zeros(K, dtype=torch.int32, device=DEV)
    want[7] = 1
    assert torch.equal(new["guard"], want)


def test_mid_unaligned_operands():
    N, K, M, H = 300, 20, 128, 64
    i = mid_inputs(N, K, M, H, True)
    for name in ("h", "Wv", "Wl", "Wk", "Wenc", "Wmu_e", "Wsig_e", "W1",
                 "Wb", "qk"):
        i[name] = off16(i[name])
    check_mid(i, N, K, M, H, "unaligned")


def test_mid_zero_eps_and_clamped_fsig():
    """All-zero eps (the decoder's dsig = 0), and one factor whose softplus
    underflows to 0 so that its fsig_c is the 1e-6 clamp."""
    N, K, M, H = 257, 20, 3, 64
    i = mid_inputs(N, K, M, H, False, zero_eps=True)
    i["bsig_e"][5] = -200.0
    new = check_mid(i, N, K, M, H, "zero eps, clamp")
    assert float(new["fsig"][5]) == 0.0
    assert float(new["fsig_c"][5]) == pytest.approx(1e-6)
    assert float(new["fsig_c"].min()) == pytest.approx(1e-6)


def test_mid_fwd_twice_resets_done():
    N, K, M, H = 300, 20, 128, 64
    i = mid_inputs(N, K, M, H, True)
    old = mid_outputs(N, K, M, H, 100)
    fwd_separate(i, old, H)
    new = mid_outputs(N, K, M, H, 300)
    for rep in range(2):
        for k in ("fmu", "fsig_pre", "fsig", "fsig_c", "yp"):
            new[k].fill_(9.0)
        assert fwd_fused(i, new, H)
        assert int(new["done"]) == 0, rep
        torch.cuda.synchronize()
        fw = ("a", "sd", "guard", "u", "ctx", "hm2", "pmu", "psig_pre",
              "psig", "psig_c", "scores", "a_enc", "yp", "fmu", "fsig_pre",
              "fsig", "fsig_c", "done")
        assert_bits({k: new[k] for k in fw}, {k: old[k] for k in fw},
                    f"launch {rep}")


@pytest.mark.parametrize("N,H", [(300, 18), (385, 64)])
def test_mid_refuses_and_launches_nothing(N, H):
    """H no multiple of 4, N past the chain: False, and no output touched."""
    K, M = 20, 128
    i = mid_inputs(N, K, M, H, True)
    new = mid_outputs(N, K, M, H, 300)
    before = {k: v.clone() for k, v in new.items()}
    assert fwd_fused(i, new, H) is False
    assert bwd_fused(i, new, H, K) is False
    torch.cuda.synchronize()
    assert_bits(new, before, f"refused N={N} H={H}")


# ------------------------------------------- gru_bwd with dh_combine fused
def gru_inputs(N, T, K, M):
    H = 64
    return {
        "dh": t(N, H, seed=40), "h_prev": t(N, T, H, seed=41).tanh(),
        "gates4": torch.sigmoid(t(N, T, 4 * H, seed=42)) * 2.0 - 0.5,
        "Whh": t(3 * H, H, seed=43, scale=H ** -0.5),
        "ds": t(N, K, seed=44), "qk": t(K, H, seed=45),
        "a": torch.softmax(t(N, K, seed=46), dim=0).contiguous(),
        "du": t(K, H, seed=47), "dscores": t(N, M, seed=48),
        "Wenc": t(M, H, seed=49, scale=H ** -0.5),
    }


def run_gru(i, N, T, fused, seed):
    H = 64
    o = {"dh": i["dh"].clone(), "dgi": garbage(N, T, 3 * H, seed=seed),
         "dgh": garbage(N, T, 3 * H, seed=seed + 1)}
    comb = (i["ds"], i["qk"], i["a"], i["du"], i["dscores"], i["Wenc"])
    if fused:
        ran = ext.gru_bwd(o["dh"], i["h_prev"], i["gates4"], i["Whh"],
                          o["dgi"], o["dgh"], N, T, H, None, None, 1, *comb)
    else:
        ext.dh_combine(o["dh"], *comb)
        ran = ext.gru_bwd(o["dh"], i["h_prev"], i["gates4"], i["Whh"],
                          o["dgi"], o["dgh"], N, T, H, variant=1)
        assert ran is False
    return o, ran


def check_gru(i, N, T, what):
    old, _ = run_gru(i, N, T, False, 100)
    new, ran = run_gru(i, N, T, True, 200)
    assert ran is True
    torch.cuda.synchronize()
    assert_bits(new, old, what)


# N around a workgroup's four waves and past several workgroups; T = 1 has
# no step to prefetch
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("N", [1, 3, 4, 5, 17, 33])
def test_gru_combine_bits(N, T):
    check_gru(gru_inputs(N, T, 20, 128), N, T, f"gru N={N} T={T}")


def test_gru_combine_bits_benchmark_shape():
    check_gru(gru_inputs(300, 20, 20, 128), 300, 20, "gru 300x20")


# K, M against the prologue's unroll factors (4 and 8): below, off and on
@pytest.mark.parametrize("M", [1, 3, 128])
@pytest.mark.parametrize("K", [1, 20, 128])
def test_gru_combine_bits_k_m(K, M):
    check_gru(gru_inputs(33, 3, K, M), 33, 3, f"gru K={K} M={M}")


def test_gru_combine_unaligned_whh():
    i = gru_inputs(33, 3, 20, 128)
    i["Whh"] = off16(i["Whh"])
    check_gru(i, 33, 3, "gru unaligned Whh")


def test_gru_combine_not_fused_past_the_wave_route():
    """One N past gru_wave_max_n(): False, and nothing is written."""
    N, T = ext.gru_wave_max_n() + 1, 1
    i = gru_inputs(N, T, 2, 3)
    new, ran = run_gru(i, N, T, True, 200)
    assert ran is False
    torch.cuda.synchronize()
    assert_bits(new, {"dh": i["dh"], "dgi": garbage(N, T, 192, seed=200),
                      "dgh": garbage(N, T, 192, seed=201)}, "not fused")


# ------------------------------------------------------ through the engine
def _trainer(monkeypatch, fuse, dtype, use_graph=False, rng_side="0",
             hidden=64, whh_fused=None):
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    if fuse is None:
        monkeypatch.delenv("FV_MID_FUSE", raising=False)
    else:
        monkeypatch.setenv("FV_MID_FUSE", fuse)
    monkeypatch.setenv("FV_RNG_SIDE", rng_side)
    for k in ("FV_MID", "FV_MID_CHAIN", "FV_F32_GRU", "FV_WHH_FUSED"):
        monkeypatch.delenv(k, raising=False)
    if whh_fused is not None:
        monkeypatch.setenv("FV_WHH_FUSED", whh_fused)
    set_seed(0)
    model = build_factorvae(num_latent=158, hidden_size=hidden,
                            num_portfolio=128, num_factor=20).to(DEV)
    tr = FusedTrainer(model, lr=1e-4, t_max=100, device=DEV,
                      use_graph=use_graph, train=True, dtype=dtype)
    assert tr._mid_chain and tr._mid_fuse == (fuse != "0")
    return tr


STEP_WS = ("loss", "mse", "kl", "recon", "drecon", "dfmu", "dfsig_c", "dpmu",
           "dpsig_c", "a1", "beta", "asig_pre", "sigma", "dscores", "dh")


def _one_step(tr, x, y, noise):
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
    assert tr._chain_pending and tr._fuse_pending == tr._mid_fuse
    tr._launch_backward(N, T)
    assert not tr._chain_pending and not tr._fuse_pending
    # fp32 at H = 64 is on the wave route: dh_combine ran as gru_bwd's
    # prologue if and only if the middle is fused
    if not tr.bf16 and tr.H == 64:
        assert tr._combine_ran == tr._mid_fuse
    torch.cuda.synchronize()
    out = {f"ws {k}": w[k].clone() for k in STEP_WS}
    out.update({f"grad {name}": tr.g(name).clone()
                for name, _, _ in tr._param_specs()})
    tr._launch_optimizer()
    torch.cuda.synchronize()
    out["params after adam"] = tr.params.flat.clone()
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("N,T", [(33, 3), (300, 20)])
def test_fused_middle_matches_the_chain_over_a_step(monkeypatch, N, T, dtype):
    x, y = t(N, T, 158, seed=50), t(N, 1, seed=51)
    noise = {}
    off = _one_step(_trainer(monkeypatch, "0", dtype), x, y, noise)
    on = _one_step(_trainer(monkeypatch, None, dtype), x, y, noise)
    assert_bits(on, off, f"step N={N} T={T} {dtype}")


@pytest.mark.parametrize("hidden,whh_fused", [(64, "0"), (32, None)])
def test_bf16_step_with_the_h_prev_cast_on_its_own_stream(monkeypatch, hidden,
                                                          whh_fused):
    """bf16 without the fused Whh weight gradient (FV_WHH_FUSED=0, or
    H < 64): h_prev's bf16 image is cast on the second side stream and read
    by the Whh weight gradient, which therefore has to stay on that stream
    (or wait for it) with the fused middle too. Run three times from a
    stale image: a missing edge between the two would show as a difference
    from FV_MID_FUSE=0 sooner or later, not necessarily every time."""
    N, T = 300, 20
    x, y = t(N, T, 158, seed=56), t(N, 1, seed=57)
    noise = {}
    kw = {"hidden": hidden, "whh_fused": whh_fused}
    tr_off = _trainer(monkeypatch, "0", "bf16", **kw)
    assert not tr_off._whh_fused
    off = _one_step(tr_off, x, y, noise)
    for rep in range(3):
        tr_on = _trainer(monkeypatch, None, "bf16", **kw)
        tr_on._ensure_ws(N, T)
        tr_on.ws["h_prev_bf"].fill_(3.0)  # a stale image must not be read
        on = _one_step(tr_on, x, y, noise)
        assert_bits(on, off, f"bf16 H={hidden} whh_fused={whh_fused} {rep}")


def test_five_graph_steps_deterministic_and_equal_to_the_chain(monkeypatch):
    """Five captured steps, twice with the fused middle, once with
    FV_MID_FUSE=0 and once with the RNG fills on the side stream
    (FV_RNG_SIDE=1: the same draws), identically seeded: the same parameter
    bits and losses."""
    N, T = 300, 20
    x, y = t(N, T, 158, seed=54), t(N, 1, seed=55)
    runs = []
    for fuse, rng_side in ((None, "0"), (None, "0"), ("0", "0"), (None, "1")):
        tr = _trainer(monkeypatch, fuse, "fp32", use_graph=True,
                      rng_side=rng_side)
        assert tr._rng_side == (rng_side == "1")
        torch.manual_seed(11)
        losses = [tr.step(x, y).clone() for _ in range(5)]
        torch.cuda.synchronize()
        runs.append({"params": tr.params.flat.clone(),
                     "losses": torch.cat(losses)})
    assert torch.isfinite(runs[0]["losses"]).all()
    assert_bits(runs[1], runs[0], "5 steps, run to run")
    assert_bits(runs[0], runs[2], "5 steps, against FV_MID_FUSE=0")
    assert_bits(runs[3], runs[0], "5 steps, FV_RNG_SIDE=1")


# ------------------------------------------------------- argument checks
# one valid argument set per binding; then one property of one tensor
# argument is broken and the refusal must name it (the manner and the
# allocation rules of test_gpu_binding_checks.py: refused on the host, and
# a launch that slipped through would stay inside its allocations)
BN, BT, BH, BK, BM = 5, 2, 8, 2, 4
F32, I32 = torch.float32, torch.int32


class A:
    def __init__(self, name, shape, dtype=F32):
        self.name, self.shape, self.dtype = name, tuple(shape), dtype

    @property
    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def valid(self):
        return torch.zeros(self.shape, dtype=self.dtype, device=DEV)

    def broken(self, how):
        if how == "dtype":
            wider = torch.float64 if self.dtype == F32 else torch.int64
            return torch.zeros(self.shape, dtype=wider, device=DEV)
        if how == "noncontig":
            if self.numel == 1:
                return None
            wide = self.shape[:-1] + (2 * self.shape[-1],)
            v = torch.zeros(wide, dtype=self.dtype, device=DEV)[..., ::2]
            assert v.shape == self.shape and not v.is_contiguous()
            return v
        if how == "cpu":
            return torch.zeros(self.shape, dtype=self.dtype).pin_memory()
        assert how == "short"
        return self.valid().view(-1)[:self.numel - 1]


def binding_specs():
    N, T, H, K, M = BN, BT, BH, BK, BM
    G3 = (N, T, 3 * H)
    attn_w = [A("Wv", (K, H, H)), A("bv", (K, H)), A("Wl", (H, H)),
              A("bl", (H,)), A("wmu", (H,)), A("bmu", (1,)), A("wsig", (H,)),
              A("bsig", (1,))]
    return {
        "mid_fwd": [
            A("h", (N, H)), A("qk", (K, H)), A("cb", (K,)), A("mask", (N, K)),
            *attn_w, A("a", (N, K)), A("sd", (N, K)), A("guard", (K,), I32),
            A("u", (K, H)), A("ctx", (K, H)), A("hm2", (K, H)),
            A("pmu", (K,)), A("psig_pre", (K,)), A("psig", (K,)),
            A("psig_c", (K,)), A("Wenc", (M, H)), A("benc", (M,)),
            A("y", (N, 1)), A("scores", (N, M)), A("a_enc", (N, M)),
            A("yp", (M,)), A("Wmu_e", (K, M)), A("bmu_e", (K,)),
            A("Wsig_e", (K, M)), A("bsig_e", (K,)), A("fmu", (K,)),
            A("fsig_pre", (K,)), A("fsig", (K,)), A("fsig_c", (K,)),
            A("done", (1,), I32), H ** -0.5, 1.0],
        "mid_bwd": [
            A("psig", (K,)), A("psig_pre", (K,)), A("hm2", (K, H)),
            A("wmu", (H,)), A("wsig", (H,)), A("Wl", (H, H)), A("h", (N, H)),
            A("a", (N, K)), A("sd", (N, K)), A("mask", (N, K)),
            A("guard", (K,), I32), A("u", (K, H)), A("Wv", (K, H, H)),
            A("q", (K, H)), A("Wk", (K, H, H)), A("bk", (K, H)),
            A("dz2", (K, H)), A("du", (K, H)), A("ds", (N, K)),
            A("dc", (K,)), A("dWv", (K, H, H)), A("dbv", (K, H)),
            A("dq", (K, H)), A("dWk", (K, H, H)), A("dbk", (K, H)),
            A("hpart", (K * (2 * H + 2),)), A("fmu", (K,)),
            A("fsig_c", (K,)), A("pmu", (K,)), A("psig_c", (K,)),
            A("dpmu", (K,)), A("dpsig_c", (K,)), A("W1", (H, H)),
            A("b1", (H,)), A("wmu_d", (H,)), A("bmu_d", (1,)),
            A("wsig_d", (H,)), A("bsig_d", (1,)), A("Wb", (K, H)),
            A("bb", (K,)), A("eps", (N,)), A("y", (N, 1)), A("recon", (N,)),
            A("a1", (N, H)), A("beta", (N, K)), A("asig_pre", (N,)),
            A("sigma", (N,)), A("drecon", (N,)), A("dh", (N, H)),
            A("dz1", (N, H)), A("dbeta", (N, K)),
            A("part", (ext.dec_nblk(N) * (2 * K + 2 * H + 2),)),
            H ** -0.5, 1.0, 1.0],
        "pred_head_reduce": [
            A("hpart", (K * (2 * H + 2),)), A("dwmu", (H,)), A("dbmu", (1,)),
            A("dwsig", (H,)), A("dbsig", (1,)), K, H],
        "gru_bwd": [
            A("dh_final", (N, H)), A("h_prev", (N, T, H)),
            A("gates4", (N, T, 4 * H)), A("Whh", (3 * H, H)), A("dgi", G3),
            A("dgh", G3), N, T, H, None, None, 1, A("ds", (N, K)),
            A("qk", (K, H)), A("a", (N, K)), A("du", (K, H)),
            A("dscores", (N, M)), A("Wenc", (M, H))],
    }


@pytest.mark.parametrize("how", ["dtype", "noncontig", "cpu", "short"])
@pytest.mark.parametrize("op", ["mid_fwd", "mid_bwd", "pred_head_reduce",
                                "gru_bwd"])
def test_one_broken_argument_is_refused_by_name(op, how):
    spec = binding_specs()[op]
    fn = getattr(ext, op)
    tried = 0
    for pos, arg in enumerate(spec):
        if not isinstance(arg, A):
            continue
        bad = arg.broken(how)
        if bad is None:
            continue
        args = [x.valid() if isinstance(x, A) else x for x in spec]
        args[pos] = bad
        want = rf"{op}: (\w+ and )?{re.escape(arg.name)} "
        with pytest.raises(RuntimeError, match=want):
            fn(*args)
        tried += 1
    assert tried >= 2, (op, how, tried)


def test_gru_bwd_combine_operands_come_as_a_set():
    spec = binding_specs()["gru_bwd"]
    args = [x.valid() if isinstance(x, A) else x for x in spec]
    args[-1] = None
    with pytest.raises(RuntimeError, match="gru_bwd: .*set of six"):
        ext.gru_bwd(*args)
