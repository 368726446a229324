"""The pipelined fp32 GEMM kernels (FV_F32_GEMM, docs/KERNELS.md): every
output of variant=1 against variant=0 as bit patterns, the one-launch
reduce against the reduces it replaces, the dxln GEMM's LayerNorm epilogue
against gemm_nn -> ln_bwd_params, and whole steps with FV_F32_GEMM=0
against the default. Outputs and workspaces start as garbage."""

import itertools

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


def assert_bits(got, ref, what):
    assert set(got) == set(ref), what
    for k in sorted(ref):
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k}"
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), \
            f"{what}: {k}: {(a != b).sum().item()} of {b.numel()} differ"


# ------------------------------------------------- gemm_tn / pair / xhat
TN_R = [1, 31, 32, 33, 65, 513, 1100]
TN_MN = [(1, 1), (33, 7), (192, 64), (158, 158)]
TN_OPTS = list(itertools.product([False, True], [False, True], [1, 4]))


@pytest.mark.parametrize("R", TN_R)
def test_gemm_tn_new_vs_old(R):
    for (M, N), (with_db, acc, chunks) in itertools.product(TN_MN, TN_OPTS):
        A, B = t(R, M, seed=1), t(R, N, seed=2)
        res = {}
        for variant in (0, 1):
            out, part = t(M, N, seed=3), t(32 * M * N, seed=4)
            db, dbp = t(M, seed=5), t(32 * M, seed=6)
            ext.gemm_tn(A, B, out, part, chunks, acc,
                        db if with_db else None, dbp if with_db else None,
                        variant=variant)
            res[variant] = {"out": out, "part": part, "db": db, "db_part": dbp}
        torch.cuda.synchronize()
        assert_bits(res[1], res[0], f"gemm_tn R={R} M={M} N={N} db={with_db} "
                                    f"acc={acc} chunks={chunks}")


@pytest.mark.parametrize("R", TN_R)
def test_gemm_tn_pair_new_vs_old(R):
    for (M, N0), (with_db, acc, chunks) in itertools.product(TN_MN, TN_OPTS):
        N1 = 7 if N0 != 7 else 64
        A0, B0 = t(R, M, seed=1), t(R, N0, seed=2)
        A1, B1 = t(R, M, seed=3), t(R, N1, seed=4)
        res = {}
        for variant in (0, 1):
            b = {"out0": t(M, N0, seed=5), "out1": t(M, N1, seed=6),
                 "part0": t(32 * M * N0, seed=7),
                 "part1": t(32 * M * N1, seed=8),
                 "db0": t(M, seed=9), "db1": t(M, seed=10),
                 "db_part0": t(32 * M, seed=11),
                 "db_part1": t(32 * M, seed=12)}
            d = (b["db0"], b["db1"], b["db_part0"], b["db_part1"])
            ext.gemm_tn_pair(A0, B0, b["out0"], A1, B1, b["out1"], b["part0"],
                             b["part1"], chunks, acc,
                             *(d if with_db else (None,) * 4),
                             variant=variant)
            res[variant] = b
        torch.cuda.synchronize()
        assert_bits(res[1], res[0], f"gemm_tn_pair R={R} M={M} N0={N0} "
                                    f"db={with_db} acc={acc} chunks={chunks}")


@pytest.mark.parametrize("R", TN_R)
def test_gemm_tn_xhat_new_vs_old(R):
    for M, N in TN_MN:
        A, x = t(R, M, seed=1), t(R, N, seed=2) + 100.0
        mean = x.mean(1).contiguous()
        rstd = (x.var(1, unbiased=False) + 1e-5).rsqrt().contiguous() \
            if N > 1 else torch.ones(R, device=DEV)
        res = {}
        for variant in (0, 1):
            part, dbp = t(32 * M * N, seed=3), t(32 * M, seed=4)
            nz = ext.gemm_tn_xhat(A, x, mean, rstd, part, dbp,
                                  variant=variant)
            assert nz == max(1, min(32, (R + 511) // 512))
            res[variant] = {"part": part, "db_part": dbp}
        torch.cuda.synchronize()
        assert_bits(res[1], res[0], f"gemm_tn_xhat R={R} M={M} N={N}")


# ---------------------------------------------------- the combined reduce
@pytest.mark.parametrize("R,z", [(300, 1), (1024, 2), (2100, 5)])
@pytest.mark.parametrize("acc", [False, True])
def test_tn_reduce_list_matches_separate_reduces(R, z, acc):
    """pair + gemm_tn with reduce=False, then one tn_reduce_list, against
    the same calls reducing on their own (tn_reduce_pair + tn_reduce)."""
    M, N0, N1, M2, N2 = 192, 64, 158, 33, 7
    chunks = 4
    A0, B0 = t(R, M, seed=1), t(R, N0, seed=2)
    A1, B1 = t(R, M, seed=3), t(R, N1, seed=4)
    A2, B2 = t(R, M2, seed=5), t(R, N2, seed=6)
    res = {}
    for reduce in (True, False):
        o = [t(M, N0, seed=7), t(M, N1, seed=8), t(M2, N2, seed=9)]
        p = [t(32 * M * N0, seed=10), t(32 * M * N1, seed=11),
             t(32 * M2 * N2, seed=12)]
        d = [t(M, seed=13), t(M, seed=14), t(M2, seed=15)]
        q = [t(32 * M, seed=16), t(32 * M, seed=17), t(32 * M2, seed=18)]
        ext.gemm_tn_pair(A0, B0, o[0], A1, B1, o[1], p[0], p[1], chunks, acc,
                         d[0], d[1], q[0], q[1], variant=1, reduce=reduce)
        ext.gemm_tn(A2, B2, o[2], p[2], chunks, acc, d[2], q[2], variant=1,
                    reduce=reduce)
        if not reduce:
            assert ext.tn_reduce_list(o, p, d, q, R, chunks, acc) == z
        res[reduce] = {f"{n}{i}": v[i] for n, v in
                       (("out", o), ("part", p), ("db", d), ("db_part", q))
                       for i in range(3)}
    torch.cuda.synchronize()
    assert_bits(res[False], res[True], f"reduce list R={R} acc={acc}")


def test_tn_reduce_list_without_bias_gradients():
    R, chunks = 1100, 4
    A, B = t(R, 40, seed=1), t(R, 33, seed=2)
    ref, got = t(40, 33, seed=3), t(40, 33, seed=4)
    pr, pg = t(32 * 40 * 33, seed=5), t(32 * 40 * 33, seed=6)
    ext.gemm_tn(A, B, ref, pr, chunks, False, variant=0)
    ext.gemm_tn(A, B, got, pg, chunks, False, variant=1, reduce=False)
    assert ext.tn_reduce_list([got], [pg], [None], [None], R, chunks,
                              False) == 3
    torch.cuda.synchronize()
    assert_bits({"out": got}, {"out": ref}, "reduce list, no db")


# ------------------------------------------------------------------ gemm_nn
NN_R = [1, 63, 64, 65, 130]
NN_CC = [(3, 5), (32, 64), (33, 64), (192, 158), (158, 158)]
# (bias, act, lrelu_bwd_of, accumulate)
NN_FLAGS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0),
            (0, 0, 0, 1), (1, 1, 1, 1)]


def _offset_view(R, Co, seed, offset):
    """An (R,Co) tensor that starts `offset` elements into its buffer."""
    flat = t(R * Co + offset, seed=seed)
    return flat[offset:].view(R, Co)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("R", NN_R)
def test_gemm_nn_new_vs_old(R, offset):
    for (Ci, Co), (bias, act, lb, acc) in itertools.product(NN_CC, NN_FLAGS):
        A, B = t(R, Ci, seed=1), t(Ci, Co, seed=2)
        bv = t(Co, seed=3)
        Y = _offset_view(R, Co, 4, offset)
        Y.copy_(F.leaky_relu(Y, 0.01))
        Y.view(-1)[::3] = 0.0  # exact zeros next to both signs
        res = {}
        for variant in (0, 1):
            out = _offset_view(R, Co, 5, offset)
            ext.gemm_nn(A, B, bv if bias else None, out, 0.75, bool(acc),
                        bool(act), lrelu_bwd_of=Y if lb else None,
                        variant=variant)
            res[variant] = {"out": out}
        torch.cuda.synchronize()
        assert_bits(res[1], res[0], f"gemm_nn R={R} Ci={Ci} Co={Co} "
                                    f"flags={(bias, act, lb, acc)}")


# ------------------------------------------------------ the ln-epilogue mode
def _ln_inputs(R, C):
    x = t(R, C, seed=1) + 100.0  # mean 100, std 1
    dzx = t(R, C, seed=2)
    W = t(C, C, seed=3, scale=C ** -0.5)
    mean = x.mean(1).contiguous()
    rstd = (x.var(1, unbiased=False) + 1e-5).rsqrt().contiguous() \
        if C > 1 else torch.ones(R, device=DEV)
    return x, dzx, W, mean, rstd


@pytest.mark.parametrize("R", [1, 64, 65, 300])
@pytest.mark.parametrize("C", [5, 64, 65, 158])
def test_gemm_nn_ln_epilogue(R, C):
    x, dzx, W, mean, rstd = _ln_inputs(R, C)
    nwords = (ext.ln_bwd_yblocks(R, C) + 1) * 2 * C
    ref = {"part": t(nwords, seed=4), "ln_g": t(C, seed=5),
           "ln_b": t(C, seed=6)}
    got = {k: v.clone() for k, v in ref.items()}
    dxln = t(R, C, seed=7)
    ext.gemm_nn(dzx, W, None, dxln, 1.0, False, False, variant=0)
    ext.ln_bwd_params(x, dxln, mean, rstd, ref["part"], ref["ln_g"],
                      ref["ln_b"], 4)
    assert ext.gemm_nn_ln(dzx, W, x, mean, rstd, got["part"]) is True
    ext.ln_bwd_reduce(got["part"], got["ln_g"], got["ln_b"], R, C)
    torch.cuda.synchronize()
    assert_bits(got, ref, f"ln epilogue R={R} C={C}")


def test_gemm_nn_ln_not_run_outside_its_geometry():
    """R = 44,000 at C = 158: ln_bwd_params works on more than 64 rows per
    block, so nothing is launched and False comes back."""
    R, C = 44000, 158
    x, dzx, W, mean, rstd = _ln_inputs(R, C)
    part = t((ext.ln_bwd_yblocks(R, C) + 1) * 2 * C, seed=4)
    before = part.clone()
    assert ext.gemm_nn_ln(dzx, W, x, mean, rstd, part) is False
    torch.cuda.synchronize()
    assert_bits({"part": part}, {"part": before}, "not run")


# ------------------------------------------------------------ bad arguments
def test_bad_arguments_are_named():
    R, C = 65, 33
    x, dzx, W, mean, rstd = _ln_inputs(R, C)
    part = t((ext.ln_bwd_yblocks(R, C) + 1) * 2 * C, seed=4)
    with pytest.raises(RuntimeError, match="gemm_nn_ln: rstd has"):
        ext.gemm_nn_ln(dzx, W, x, mean, rstd[:-1].contiguous(), part)
    with pytest.raises(RuntimeError, match="ln_bwd_reduce: dgamma has"):
        ext.ln_bwd_reduce(part, t(C + 1), t(C), R, C)
    o, p = t(40, 33), t(2 * 40 * 33)
    with pytest.raises(RuntimeError, match=r"tn_reduce_list: parts\[i\] has"):
        ext.tn_reduce_list([o], [p], [None], [None], 1100, 4, False)
    with pytest.raises(RuntimeError, match="gemm_nn: variant = 7"):
        ext.gemm_nn(dzx, W, None, t(R, C), 1.0, False, False, variant=7)
    with pytest.raises(RuntimeError, match="gemm_tn: reduce = false needs"):
        ext.gemm_tn(dzx, x, t(C, C), None, 4, False, reduce=False)
    torch.cuda.synchronize()


# -------------------------------------------------------- through the engine
def _trainer(monkeypatch, gemm, tail, dtype="fp32", use_graph=False):
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    for name, val in (("FV_F32_GEMM", gemm), ("FV_F32_TAIL", tail)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    set_seed(0)
    model = build_factorvae(num_latent=158, hidden_size=64, num_portfolio=128,
                            num_factor=20).to(DEV)
    tr = FusedTrainer(model, lr=1e-4, t_max=100, device=DEV,
                      use_graph=use_graph, dtype=dtype)
    assert tr._gv == (0 if gemm == "0" else 1)
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


@pytest.mark.parametrize("N,T,dtype,tail", [
    (33, 3, "fp32", None), (33, 3, "fp32", "2"), (300, 20, "fp32", None),
    (300, 20, "fp32", "2"), (300, 20, "bf16", None),
    # R = 44,000: the ln epilogue is not run, the old pair of kernels is
    (220, 200, "fp32", None)])
def test_f32_gemm_matches_old_kernels_over_a_step(monkeypatch, N, T, dtype,
                                                  tail):
    x, y = t(N, T, 158, seed=50), t(N, 1, seed=51)
    noise = {}
    off = _one_step(_trainer(monkeypatch, "0", tail, dtype), x, y, noise)
    on = _one_step(_trainer(monkeypatch, None, tail, dtype), x, y, noise)
    assert_bits(on, off, f"step N={N} T={T} {dtype} tail={tail}")


def test_five_graph_steps(monkeypatch):
    """5 captured steps: two default runs and one with FV_F32_GEMM=0, all
    with identical parameter bits and losses."""
    N, T = 300, 20
    x, y = t(N, T, 158, seed=54), t(N, 1, seed=55)
    runs = []
    for gemm in (None, None, "0"):
        tr = _trainer(monkeypatch, gemm, None, use_graph=True)
        torch.manual_seed(11)
        losses = [tr.step(x, y).clone() for _ in range(5)]
        torch.cuda.synchronize()
        runs.append({"params": tr.params.flat.clone(),
                     "losses": torch.cat(losses)})
    assert_bits(runs[1], runs[0], "5 steps, default twice")
    assert_bits(runs[2], runs[0], "5 steps, FV_F32_GEMM=0")
    assert torch.isfinite(runs[0]["losses"]).all()
