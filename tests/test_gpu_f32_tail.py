"""The shortened fp32 backward tail: gemm_nn's LeakyReLU-backward
epilogue, the paired Whh/Wih weight-gradient launch, the LayerNorm + W1x
gradients formed without dxln (gemm_tn_xhat -> ln_w1x_finish), the fp32
GRU backward's dgi, and the whole step against the old kernel sequence
(FV_F32_TAIL=0)."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from factorvae_amd.ops import get_extension
    ext = get_extension()
DEV = torch.device("cuda:0")


def t(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def assert_close(a, b, atol, rtol, what=""):
    torch.testing.assert_close(a, b, atol=atol, rtol=rtol,
                               msg=lambda m: f"{what}: {m}")


# ------------------------------------------- gemm_nn + lrelu_bwd epilogue
@pytest.mark.parametrize("R,Ci,Co", [(1, 3, 5), (65, 192, 158),
                                     (130, 33, 64)])
def test_gemm_nn_lrelu_bwd_epilogue(R, Ci, Co):
    A, B = t(R, Ci, seed=1), t(Ci, Co, seed=2)
    Y = F.leaky_relu(t(R, Co, seed=3), 0.01)
    Y.view(-1)[::3] = 0.0  # exact zeros next to both signs
    Y.view(-1)[1] = 0.5
    Y.view(-1)[2] = -0.005
    assert (Y == 0).any() and (Y > 0).any() and (Y < 0).any()

    dxp = torch.empty(R, Co, device=DEV)
    two = torch.empty(R, Co, device=DEV)
    ext.gemm_nn(A, B, None, dxp, 1.0, False, False)
    ext.lrelu_bwd(dxp, Y, two)
    one = torch.empty(R, Co, device=DEV)
    ext.gemm_nn(A, B, None, one, 1.0, False, False, lrelu_bwd_of=Y)
    torch.cuda.synchronize()
    assert torch.equal(one, two), \
        f"{(one != two).sum().item()} of {one.numel()} elements differ"


# ------------------------------------------------------------ gemm_tn_pair
@pytest.mark.parametrize("R,M,N0,N1", [(33, 192, 64, 158),
                                       (1100, 192, 64, 158),
                                       (513, 40, 7, 33)])
def test_gemm_tn_pair(R, M, N0, N1):
    chunks = 4  # asks for slicing; the launcher's rule picks the count
    A0, B0 = t(R, M, seed=4), t(R, N0, seed=5)
    A1, B1 = t(R, M, seed=6), t(R, N1, seed=7)

    def bufs(N, seed):
        # garbage-filled outputs and workspaces: every word must be written
        return (t(M, N, seed=seed), t(32 * M * N, seed=seed + 1),
                t(M, seed=seed + 2), t(32 * M, seed=seed + 3))

    o0, p0, d0, q0 = bufs(N0, 10)
    o1, p1, d1, q1 = bufs(N1, 20)
    ext.gemm_tn(A0, B0, o0, p0, chunks, False, d0, q0)
    ext.gemm_tn(A1, B1, o1, p1, chunks, False, d1, q1)
    po0, pp0, pd0, pq0 = bufs(N0, 30)
    po1, pp1, pd1, pq1 = bufs(N1, 40)
    ext.gemm_tn_pair(A0, B0, po0, A1, B1, po1, pp0, pp1, chunks, False,
                     pd0, pd1, pq0, pq1)
    torch.cuda.synchronize()
    for got, ref, what in ((po0, o0, "out0"), (po1, o1, "out1"),
                           (pd0, d0, "db0"), (pd1, d1, "db1")):
        assert torch.equal(got, ref), \
            f"{what}: {(got != ref).sum().item()} of {ref.numel()} differ"
    # and the separate calls are themselves right
    assert_close(o1, A1.t() @ B1, 5e-4, 5e-4, "gemm_tn ref")


# ------------------------------------------- gemm_tn_xhat + ln_w1x_finish
@pytest.mark.parametrize("R,C", [(33, 5), (513, 33), (1100, 158)])
def test_ln_w1x_grads_without_dxln(R, C):
    """All four gradients of layer_norm -> linear from G = dzx^T @ xhat and
    gb = colsum(dzx). The reference is float64 autograd, so the measured
    error is this path's own. W1x has nn.Linear's init scale."""
    x = t(R, C, seed=50) + 100.0  # large common offset, std 1
    dzx = t(R, C, seed=51)
    W = t(C, C, seed=52, scale=C ** -0.5)
    b1 = t(C, seed=53)
    gamma = t(C, seed=54)  # both signs
    gamma[0] = 0.0
    gamma[C - 1] = 1e-4
    beta = t(C, seed=55) + 0.5
    assert (gamma > 0).any() and (gamma < 0).any() and (beta != 0).all()

    leaves = [v.double().requires_grad_(True) for v in (gamma, beta, W, b1)]
    gd, bd, Wd, b1d = leaves
    zx = F.linear(F.layer_norm(x.double(), (C,), gd, bd, 1e-5), Wd, b1d)
    zx.backward(dzx.double())
    ref = {"ln_g": gd.grad, "ln_b": bd.grad, "W1x": Wd.grad, "b1x": b1d.grad}

    xln = torch.empty(R, C, device=DEV)
    mean = torch.empty(R, device=DEV)
    rstd = torch.empty(R, device=DEV)
    ext.ln_fwd(x, gamma, beta, xln, mean, rstd, 1e-5)
    part = t(32 * C * C, seed=56)   # garbage: only nz slices are read
    db_part = t(32 * C, seed=57)
    nz = ext.gemm_tn_xhat(dzx, x, mean, rstd, part, db_part)
    assert nz == max(1, min(32, (R + 511) // 512))
    got = {"ln_g": t(C, seed=58), "ln_b": t(C, seed=59),
           "W1x": t(C, C, seed=60), "b1x": t(C, seed=61)}
    ext.ln_w1x_finish(part, db_part, nz, W, gamma, beta, got["W1x"],
                      got["b1x"], got["ln_g"], got["ln_b"])
    torch.cuda.synchronize()
    for name in ("b1x", "W1x", "ln_b", "ln_g"):
        r = ref[name].float()
        err = (got[name] - r).abs()
        print(f"R={R} C={C} {name}: max abs err {err.max().item():.3e}, "
              f"max |ref| {r.abs().max().item():.3e}")
    for name in ("b1x", "W1x", "ln_b", "ln_g"):
        assert_close(got[name], ref[name].float(), 5e-4, 5e-4, name)


# ----------------------------------------------------- gru_bwd, fp32, H=64
@pytest.mark.parametrize("N,T", [(1, 1), (16, 2), (17, 3), (300, 20)])
def test_gru_bwd_f32_dgi(N, T):
    """dgi against torch.nn.GRU autograd at the shapes where a step-input
    prefetch in the backward kernel could go wrong: a single step, a full
    16-stock block, a block with 15 dead rows, the benchmark shape (the
    prefetch itself was measured and left out, profiles/f32_tail.md; the
    cases guard the next attempt). The GRU's input projection is the
    identity (input size 3H, weight_ih = I, bias_ih = 0), so gi is the
    input itself and the input gradient is dgi."""
    H = 64
    torch.manual_seed(20)
    gru = torch.nn.GRU(3 * H, H, 1, batch_first=True).to(DEV)
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.eye(3 * H, device=DEV))
        gru.bias_ih_l0.zero_()
    gi = t(N, T, 3 * H, seed=21)

    gi_r = gi.clone().requires_grad_(True)
    out, _ = gru(gi_r)
    dh = t(N, H, seed=22)
    out[:, -1, :].backward(dh)

    h_final = torch.empty(N, H, device=DEV)
    h_seq = torch.empty(N, T, H, device=DEV)
    h_prev = torch.empty(N, T, H, device=DEV)
    gates4 = torch.empty(N, T, 4 * H, device=DEV)
    ext.gru_fwd(gi, gru.weight_hh_l0.detach(), gru.bias_hh_l0.detach(),
                h_final, h_seq, h_prev, gates4, N, T, H)
    dgi = torch.full((N, T, 3 * H), float("nan"), device=DEV)
    dgh = torch.full((N, T, 3 * H), float("nan"), device=DEV)
    ext.gru_bwd(dh, h_prev, gates4, gru.weight_hh_l0.detach(), dgi, dgh,
                N, T, H)
    dWhh = torch.zeros(3 * H, H, device=DEV)
    ext.gemm_tn(dgh.view(N * T, 3 * H), h_prev.view(N * T, H), dWhh, None, 1,
                False)
    torch.cuda.synchronize()
    assert_close(dgi, gi_r.grad, 1e-3, 1e-3, "dgi")
    assert_close(dWhh, gru.weight_hh_l0.grad, 1e-3, 1e-3, "dWhh (via dgh)")


# ------------------------------------------------------- old vs new step
@pytest.mark.parametrize("level", [None, "2"])
def test_f32_tail_matches_old_sequence(monkeypatch, level):
    """FV_F32_TAIL=0 against the default (None) and against the opt-in
    level 2 (LayerNorm/W1x gradients without dxln). The default keeps the
    old kernels for those four slots, so there it is bit-equal too."""
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    N, T, C, H, M, K = 33, 3, 158, 64, 128, 20
    x, y = t(N, T, C, seed=50), t(N, 1, seed=51)
    noise = {}

    def grads(env, expect):
        if env is None:
            monkeypatch.delenv("FV_F32_TAIL", raising=False)
        else:
            monkeypatch.setenv("FV_F32_TAIL", env)
        set_seed(0)
        model = build_factorvae(num_latent=C, hidden_size=H, num_portfolio=M,
                                num_factor=K).to(DEV)
        tr = FusedTrainer(model, lr=1e-4, t_max=100, device=DEV,
                          use_graph=False)
        assert tr._f32_tail == expect
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
        return {name: tr.g(name).clone() for name, _, _ in tr._param_specs()}

    old = grads("0", 0)
    new = grads(level, 2 if level == "2" else 1)
    changed = {"ln_g", "ln_b", "W1x", "b1x"}
    assert changed <= set(old)
    for name in old:
        if name in changed:
            print(f"{name}: max abs diff "
                  f"{(new[name] - old[name]).abs().max().item():.3e}")
            assert_close(new[name], old[name], 2e-3, 2e-3, f"grad {name}")
            if level is None:
                assert torch.equal(new[name], old[name]), \
                    f"grad {name} differs"
        else:
            assert torch.equal(new[name], old[name]), f"grad {name} differs"
