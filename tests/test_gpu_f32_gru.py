"""The wave-per-stock fp32 GRU kernels (FV_F32_GRU, docs/KERNELS.md): every
output of variant=1 against variant=0 as bit patterns, then whole steps,
validation and scoring with FV_F32_GRU=0 against the default. Outputs start
as garbage."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from factorvae_amd.ops import get_extension
    ext = get_extension()
DEV = torch.device("cuda:0")
H = 64


def t(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def off16(n, seed, scale=1.0):
    """t(n, seed, scale)'s values, one float past a 16-byte boundary."""
    flat = torch.empty(n + 1, device=DEV)
    assert flat.data_ptr() % 16 == 0
    flat[1:].copy_(t(n, seed=seed, scale=scale))
    return flat[1:]


def assert_bits(got, ref, what):
    assert set(got) == set(ref), what
    for k in sorted(ref):
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k}"
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), \
            f"{what}: {k}: {(a != b).sum().item()} of {b.numel()} differ"


def weights(scale=0.125, unaligned=False):
    if unaligned:
        return (off16(3 * H * H, 2, scale).view(3 * H, H),
                off16(3 * H, 3, 0.1))
    return t(3 * H, H, seed=2, scale=scale), t(3 * H, seed=3, scale=0.1)


def run_fwd(variant, gi, Whh, bhh, N, T, with_seq=True):
    o = {"h_final": t(N, H, seed=10), "h_prev": t(N, T, H, seed=11),
         "gates4": t(N, T, 4 * H, seed=12)}
    if with_seq:
        o["h_seq"] = t(N, T, H, seed=13)
    ext.gru_fwd(gi, Whh, bhh, o["h_final"], o.get("h_seq"), o["h_prev"],
                o["gates4"], N, T, H, variant=variant)
    return o


def run_bwd(variant, dh, h_prev, gates4, Whh, N, T):
    o = {"dgi": t(N, T, 3 * H, seed=20), "dgh": t(N, T, 3 * H, seed=21)}
    ext.gru_bwd(dh, h_prev, gates4, Whh, o["dgi"], o["dgh"], N, T, H,
                variant=variant)
    return o


def check_fwd_bwd(N, T, what, scale=0.125, unaligned=False, with_seq=True,
                  dh_zero=False, z_one=False):
    gi = t(N, T, 3 * H, seed=1)
    Whh, bhh = weights(scale, unaligned)
    f0 = run_fwd(0, gi, Whh, bhh, N, T, with_seq)
    f1 = run_fwd(1, gi, Whh, bhh, N, T, with_seq)
    hi = t(N, H, seed=14)
    ext.gru_fwd_infer(gi, Whh, bhh, hi, N, T, H, variant=1)
    torch.cuda.synchronize()
    assert_bits(f1, f0, f"fwd {what}")
    assert_bits({"h_final": hi}, {"h_final": f0["h_final"]}, f"infer {what}")
    dh = torch.zeros(N, H, device=DEV) if dh_zero else t(N, H, seed=4)
    g4 = f0["gates4"]
    if z_one:
        g4 = g4.clone()
        g4[:, :, H:2 * H][:, :, ::3] = 1.0
    b0 = run_bwd(0, dh, f0["h_prev"], g4, Whh, N, T)
    b1 = run_bwd(1, dh, f0["h_prev"], g4, Whh, N, T)
    torch.cuda.synchronize()
    assert_bits(b1, b0, f"bwd {what}")
    return f0, b0


# --------------------------------------------------------------- the kernels
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("N", [1, 3, 4, 5, 17, 33])
def test_wave_kernels_match_mfma_kernels(N, T):
    for with_seq in (True, False):
        f0, b0 = check_fwd_bwd(N, T, f"N={N} T={T} h_seq={with_seq}",
                               with_seq=with_seq)
    assert torch.isfinite(f0["h_final"]).all()
    assert b0["dgi"].abs().max() > 0


def test_benchmark_shape():
    f0, b0 = check_fwd_bwd(300, 20, "N=300 T=20", with_seq=False)
    assert torch.isfinite(b0["dgh"]).all() and f0["h_final"].abs().max() > 0


@pytest.mark.parametrize("N,T", [(5, 3), (33, 2)])
def test_weights_one_float_past_a_16_byte_boundary(N, T):
    ref, _ = check_fwd_bwd(N, T, "aligned")
    got, _ = check_fwd_bwd(N, T, "unaligned", unaligned=True)
    # the same values at another address: the same bits again
    assert_bits(got, ref, "unaligned against aligned")


@pytest.mark.parametrize("scale", [1e-30, 1e-38])
def test_tiny_recurrent_weights(scale):
    """Whh * 1e-30 as the issue sets it; at 1e-38 the weights, every product
    and every partial sum of both chains are subnormal."""
    Whh, _ = weights(0.125 * scale)
    assert (Whh != 0).any()
    if scale == 1e-38:
        assert Whh.abs().max() < 1.1754944e-38
    check_fwd_bwd(17, 3, f"Whh * {scale}", scale=0.125 * scale)


def test_bwd_zero_dh_final_and_saturated_z():
    check_fwd_bwd(17, 3, "dh_final = 0", dh_zero=True)
    check_fwd_bwd(17, 3, "z = 1", z_one=True)
    check_fwd_bwd(5, 2, "dh_final = 0, z = 1", dh_zero=True, z_one=True)


def test_router_falls_back_above_the_cut_over():
    """One stock more than gru_wave_max_n(): variant=1 runs the MFMA
    kernels, so nothing can differ; one stock fewer runs the wave kernels."""
    n_max = ext.gru_wave_max_n()
    assert n_max >= 300
    check_fwd_bwd(n_max + 1, 1, "above the cut-over", with_seq=False)
    check_fwd_bwd(n_max, 1, "at the cut-over", with_seq=False)


def test_bad_variant_is_named():
    gi = t(4, 1, 3 * H, seed=1)
    Whh, bhh = weights()
    o = [t(4, H), None, t(4, 1, H), t(4, 1, 4 * H)]
    with pytest.raises(RuntimeError, match="gru_fwd: variant = 7"):
        ext.gru_fwd(gi, Whh, bhh, *o, 4, 1, H, variant=7)
    with pytest.raises(RuntimeError, match="gru_fwd_infer: variant = 2"):
        ext.gru_fwd_infer(gi, Whh, bhh, o[0], 4, 1, H, variant=2)
    with pytest.raises(RuntimeError, match="gru_bwd: variant = -1"):
        ext.gru_bwd(o[0], o[2], o[3], Whh, t(4, 1, 3 * H), t(4, 1, 3 * H),
                    4, 1, H, variant=-1)
    torch.cuda.synchronize()


# -------------------------------------------------------- through the engine
def _trainer(monkeypatch, gru, use_graph=False):
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    if gru is None:
        monkeypatch.delenv("FV_F32_GRU", raising=False)
    else:
        monkeypatch.setenv("FV_F32_GRU", gru)
    set_seed(0)
    model = build_factorvae(num_latent=158, hidden_size=64, num_portfolio=128,
                            num_factor=20).to(DEV)
    tr = FusedTrainer(model, lr=1e-4, t_max=100, device=DEV,
                      use_graph=use_graph, dtype="fp32")
    assert tr._gru_v == (0 if gru == "0" else 1)
    return tr


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
    tr._launch_forward(N, T, train=True)
    tr._launch_backward(N, T)
    torch.cuda.synchronize()
    out = {f"out {k}": w[k].clone() for k in ("loss", "mse", "kl", "recon")}
    out.update({f"grad {name}": tr.g(name).clone()
                for name, _, _ in tr._param_specs()})
    tr._launch_optimizer()
    torch.cuda.synchronize()
    out["params after adam"] = tr.params.flat.clone()
    return out


@pytest.mark.parametrize("N,T", [(33, 3), (300, 20)])
def test_f32_gru_matches_mfma_kernels_over_a_step(monkeypatch, N, T):
    """FV_F32_GRU=0 against the default: one whole step (losses, recon,
    every gradient slot, parameters after Adam), then forward_only, predict
    and predict_many / loss_many on two packed days."""
    x, y = t(N, T, 158, seed=50), t(N, 1, seed=51)
    noise = {}
    tr_off = _trainer(monkeypatch, "0")
    off = _one_step(tr_off, x, y, noise)
    tr_on = _trainer(monkeypatch, None)
    on = _one_step(tr_on, x, y, noise)
    assert_bits(on, off, f"step N={N} T={T}")

    n2 = max(1, N // 2 - 1)
    days = [(x, y), (x[:n2].contiguous(), y[:n2].contiguous())]
    eps = [t(N, seed=60), t(n2, seed=61)]
    res = {}
    for key, tr in (("off", tr_off), ("on", tr_on)):
        torch.manual_seed(7)
        val = tr.forward_only(x, y).clone()
        r = {"forward_only loss": val,
             "forward_only recon": tr.ws["recon"].clone()}
        torch.manual_seed(8)
        r["predict"] = tr.predict(x)
        many = tr.predict_many([d[0] for d in days], eps=eps,
                               return_dist=True)
        for d, entry in enumerate(many):
            for name, v in zip(("score", "mu", "sigma"), entry):
                r[f"predict_many day {d} {name}"] = v
        for k, v in tr.loss_many(days, eps=eps, return_factors=True).items():
            r[f"loss_many {k}"] = v
        res[key] = r
    torch.cuda.synchronize()
    assert_bits(res["on"], res["off"], f"N={N} T={T}")


def test_five_graph_steps(monkeypatch):
    """5 captured steps: two default runs and one with FV_F32_GRU=0, all
    with identical parameter bits and losses."""
    N, T = 300, 20
    x, y = t(N, T, 158, seed=54), t(N, 1, seed=55)
    runs = []
    for gru in (None, None, "0"):
        tr = _trainer(monkeypatch, gru, use_graph=True)
        torch.manual_seed(11)
        losses = [tr.step(x, y).clone() for _ in range(5)]
        torch.cuda.synchronize()
        runs.append({"params": tr.params.flat.clone(),
                     "losses": torch.cat(losses)})
    assert_bits(runs[1], runs[0], "5 steps, default twice")
    assert_bits(runs[2], runs[0], "5 steps, FV_F32_GRU=0")
    assert torch.isfinite(runs[0]["losses"]).all()
