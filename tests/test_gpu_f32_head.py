"""The fused fp32 extractor head (extractor_head_fwd: LayerNorm + W1x
projection with LeakyReLU + GRU input projection in one launch) against
the three-kernel sequence it replaces (ln_fwd -> gemm_nt -> gemm_nt):
every output bit-equal, at the kernel, through the unsupported-shape
fallback, and over the whole step (FV_F32_HEAD=0 against the default)."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from factorvae_amd.ops import get_extension
    ext = get_extension()
DEV = torch.device("cuda:0")

OUTS = ("xln", "mean", "rstd", "xp", "gi")


def t(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def head_inputs(R, C, H, offset=0.0):
    G = 3 * H
    gamma = t(C, seed=2)  # both signs
    gamma[0] = 0.0
    return {"x": t(R, C, seed=1) + offset, "gamma": gamma,
            "beta": t(C, seed=3) + 0.5,
            "W1x": t(C, C, seed=4, scale=C ** -0.5), "b1x": t(C, seed=5),
            "Wih": t(G, C, seed=6, scale=C ** -0.5), "bih": t(G, seed=7)}


def garbage_outputs(R, C, G, seed):
    # garbage-filled: a store the kernel misses shows as a difference
    return {"xln": t(R, C, seed=seed), "mean": t(R, seed=seed + 1),
            "rstd": t(R, seed=seed + 2), "xp": t(R, C, seed=seed + 3),
            "gi": t(R, G, seed=seed + 4)}


def run_old(i, o):
    ext.ln_fwd(i["x"], i["gamma"], i["beta"], o["xln"], o["mean"], o["rstd"],
               1e-5)
    ext.gemm_nt(o["xln"], i["W1x"], i["b1x"], o["xp"], 1.0, False, True)
    ext.gemm_nt(o["xp"], i["Wih"], i["bih"], o["gi"], 1.0, False, False)


def run_new(i, o, strip=0, with_xln=True):
    return ext.extractor_head_fwd(
        i["x"], i["gamma"], i["beta"], i["W1x"], i["b1x"], i["Wih"], i["bih"],
        o["xln"] if with_xln else None, o["mean"], o["rstd"], o["xp"],
        o["gi"], 1e-5, strip)


def assert_same(new, old, names, what):
    for name in names:
        a, b = new[name], old[name]
        assert torch.equal(a, b), (
            f"{what} {name}: {(a != b).sum().item()} of {b.numel()} differ, "
            f"max abs diff {(a - b).abs().max().item():.3e}")


# (R, C, H): single row / odd C below one k-group / tiny G; one row past a
# 32-row strip with k % 4 = 1 and ln_fwd's scalar path; the benchmark's C
# and G, one row past a 64-row strip; C a multiple of 32 (no k tail); C
# one past a k-tile with G = 60, not a multiple of 16
SHAPES = [(1, 3, 4), (33, 5, 4), (65, 158, 64), (130, 160, 64), (47, 33, 20)]


# ------------------------------------------------ kernel vs three kernels
@pytest.mark.parametrize("strip", [0, 16, 32, 64])
@pytest.mark.parametrize("R,C,H", SHAPES)
def test_head_matches_three_kernels(R, C, H, strip):
    i = head_inputs(R, C, H)
    old, new = garbage_outputs(R, C, 3 * H, 10), garbage_outputs(R, C, 3 * H,
                                                                 20)
    run_old(i, old)
    assert run_new(i, new, strip) is True
    torch.cuda.synchronize()
    assert_same(new, old, OUTS, f"R={R} C={C} H={H} strip={strip}")


@pytest.mark.parametrize("strip", [0, 16, 64])
def test_head_large_mean(strip):
    """x at mean 100, std 1: the case the two-pass variance exists for."""
    R, C, H = 65, 158, 64
    i = head_inputs(R, C, H, offset=100.0)
    old, new = garbage_outputs(R, C, 3 * H, 10), garbage_outputs(R, C, 3 * H,
                                                                 20)
    run_old(i, old)
    assert run_new(i, new, strip) is True
    torch.cuda.synchronize()
    assert (old["mean"] - 100.0).abs().max() < 1.0
    assert_same(new, old, OUTS, f"mean 100 strip={strip}")


def test_head_without_xln():
    """xln=None: the other four outputs unchanged, the buffer untouched."""
    R, C, H = 47, 33, 20
    i = head_inputs(R, C, H)
    old, new = garbage_outputs(R, C, 3 * H, 10), garbage_outputs(R, C, 3 * H,
                                                                 20)
    untouched = new["xln"].clone()
    run_old(i, old)
    assert run_new(i, new, with_xln=False) is True
    torch.cuda.synchronize()
    assert_same(new, old, ("mean", "rstd", "xp", "gi"), "xln=None")
    assert torch.equal(new["xln"], untouched)


def test_three_kernels_against_float64():
    """The yardstick itself: the old sequence against a float64 torch
    reference, at the tolerance test_gemm_tn_pair uses for fp32 MFMA."""
    R, C, H = 65, 158, 64
    i = head_inputs(R, C, H)
    old = garbage_outputs(R, C, 3 * H, 10)
    run_old(i, old)
    torch.cuda.synchronize()
    d = {k: v.double() for k, v in i.items()}
    xln = F.layer_norm(d["x"], (C,), d["gamma"], d["beta"], 1e-5)
    xp = F.leaky_relu(F.linear(xln, d["W1x"], d["b1x"]), 0.01)
    gi = F.linear(xp, d["Wih"], d["bih"])
    mean = d["x"].mean(-1)
    rstd = (d["x"].var(-1, unbiased=False) + 1e-5).rsqrt()
    ref = {"xln": xln, "mean": mean, "rstd": rstd, "xp": xp, "gi": gi}
    for name in OUTS:
        torch.testing.assert_close(
            old[name], ref[name].float(), atol=5e-4, rtol=5e-4,
            msg=lambda m, name=name: f"{name}: {m}")


def test_head_reports_unsupported():
    """Outside the limits nothing is launched and False comes back."""
    R, C, H = 5, 300, 4
    i = head_inputs(R, C, H)
    new = garbage_outputs(R, C, 3 * H, 20)
    before = {k: v.clone() for k, v in new.items()}
    assert run_new(i, new) is False
    torch.cuda.synchronize()
    assert_same(new, before, OUTS, "unsupported C")


# -------------------------------------------------- through the engine
def _trainer(monkeypatch, head, tail, C, H=64, M=128, K=20):
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    for name, val in (("FV_F32_HEAD", head), ("FV_F32_TAIL", tail)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    set_seed(0)
    model = build_factorvae(num_latent=C, hidden_size=H, num_portfolio=M,
                            num_factor=K).to(DEV)
    tr = FusedTrainer(model, lr=1e-4, t_max=100, device=DEV, use_graph=False)
    assert tr._f32_head == (head != "0")
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


def test_unsupported_shape_falls_back(monkeypatch):
    """C = 300 is outside the fused kernel's range: the step runs on the
    three old kernels and matches the knob-off run bit for bit."""
    N, T, C = 9, 3, 300
    x, y = t(N, T, C, seed=50), t(N, 1, seed=51)
    noise = {}
    off = _one_step(_trainer(monkeypatch, "0", None, C), x, y, noise)
    on = _one_step(_trainer(monkeypatch, None, None, C), x, y, noise)
    assert set(on) == set(off)
    assert_same(on, off, sorted(off), "C=300")


@pytest.mark.parametrize("tail", [None, "2"])
def test_f32_head_matches_old_sequence(monkeypatch, tail):
    """FV_F32_HEAD=0 against the default over one whole step, at the
    default tail level and at FV_F32_TAIL=2 (which passes xln=None), then
    forward_only and predict."""
    N, T, C = 33, 3, 158
    x, y = t(N, T, C, seed=50), t(N, 1, seed=51)
    noise = {}
    tr_off = _trainer(monkeypatch, "0", tail, C)
    off = _one_step(tr_off, x, y, noise)
    tr_on = _trainer(monkeypatch, None, tail, C)
    assert tr_on._f32_tail == (2 if tail == "2" else 1)
    on = _one_step(tr_on, x, y, noise)
    assert set(on) == set(off)
    assert_same(on, off, sorted(off), f"tail={tail}")

    res = {}
    for key, tr in (("off", tr_off), ("on", tr_on)):
        torch.manual_seed(7)
        val = tr.forward_only(x, y).clone()
        val_recon = tr.ws["recon"].clone()
        torch.manual_seed(8)
        res[key] = {"forward_only loss": val, "forward_only recon": val_recon,
                    "predict": tr.predict(x)}
    torch.cuda.synchronize()
    assert_same(res["on"], res["off"], sorted(res["off"]), f"tail={tail}")
