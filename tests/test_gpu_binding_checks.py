"""Argument checks of the bindings: every tensor a binding hands to a launcher
is checked for device, dtype, contiguity and element count, and the error
names the op and the argument.

For each binding one valid argument set is built; then, once per tensor
argument, exactly one property is broken and the call must raise a
RuntimeError that names that argument. The calls are refused on the host, so
nothing is launched. Should a check be missing, the launch still stays inside
its allocations:
  - a tensor with too few elements is a leading slice of a full-size one;
  - a tensor of the wrong dtype has at least as many bytes as the right one;
  - a non-contiguous tensor is a strided view of a buffer twice the size;
  - a CPU tensor is in pinned host memory, which the GPU can address.

Where a property cannot be broken, the case does not exist:
  - a one-element tensor is always contiguous;
  - `out` and `db` of wgrad_reduce alone give the counts the call works on, so
    shorter ones are a valid smaller call.
An argument that gives the call a dimension (h gives N and H) is shortened to
a flat slice, one element short of the full tensor. Two arguments that give
a count together (recon and y, fmu and fsig_c, p and g) are reported together.
"""

import re

import pytest
import torch

from factorvae_amd.ops import get_extension

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    ext = get_extension()
    DEV = torch.device("cuda:0")

N, T, C, H, K, M = 5, 2, 8, 8, 2, 4
F32, BF16, I32, FP8 = (torch.float32, torch.bfloat16, torch.int32,
                       torch.float8_e4m3fn)
# a dtype that is wrong and at least as wide
WIDER = {F32: torch.float64, BF16: torch.float32, I32: torch.int64,
         FP8: torch.float32}


class A:
    """One tensor argument: name, shape, dtype; count=True marks the two
    wgrad_reduce arguments that have no 'too few' case."""

    def __init__(self, name, shape, dtype=F32, count=False):
        self.name, self.shape, self.dtype = name, tuple(shape), dtype
        self.count = count

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
            return torch.zeros(self.shape, dtype=WIDER[self.dtype],
                               device=DEV)
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
        if self.count:
            return None
        v = self.valid().view(-1)[:self.numel - 1]
        assert v.numel() == self.numel - 1
        return v


def dec_part():
    return ext.dec_nblk(N) * (2 * K + 2 * H + 2)


ATTN_W = [A("Wv", (K, H, H)), A("bv", (K, H)), A("Wl", (H, H)), A("bl", (H,)),
          A("wmu", (H,)), A("bmu", (1,)), A("wsig", (H,)), A("bsig", (1,))]
DEC_W = [A("W1", (H, H)), A("b1", (H,)), A("wmu", (H,)), A("bmu", (1,)),
         A("wsig", (H,)), A("bsig", (1,)), A("Wb", (K, H)), A("bb", (K,))]
LOSS_IN = [A("recon", (N,)), A("y", (N, 1)), A("fmu", (K,)),
           A("fsig_c", (K,)), A("pmu", (K,)), A("psig_c", (K,)),
           A("loss", (1,)), A("mse", (1,)), A("kl", (1,))]
GRU_FWD = [A("h_final", (N, H)), A("h_seq", (N, T, H)),
           A("h_prev", (N, T, H)), A("gates4", (N, T, 4 * H)), N, T, H]
GRU_BWD_IN = [A("dh_final", (N, H)), A("h_prev", (N, T, H)),
              A("gates4", (N, T, 4 * H))]
G3 = (N, T, 3 * H)


def specs():
    """op -> argument list, tensors as A and everything else as it is."""
    return {
        "attn_fused_fwd": [
            A("h", (N, H)), A("qk", (K, H)), A("cb", (K,)),
            A("mask", (N, K)), *ATTN_W, A("a", (N, K)), A("sd", (N, K)),
            A("guard", (K,), I32), A("u", (K, H)), A("ctx", (K, H)),
            A("hm2", (K, H)), A("pmu", (K,)), A("psig_pre", (K,)),
            A("psig", (K,)), A("psig_c", (K,)), H ** -0.5, 1.0, 1],
        "attn_fused_bwd": [
            A("dpmu", (K,)), A("dpsig_c", (K,)), A("psig", (K,)),
            A("psig_pre", (K,)), A("hm2", (K, H)), A("wmu", (H,)),
            A("wsig", (H,)), A("Wl", (H, H)), A("h", (N, H)), A("a", (N, K)),
            A("sd", (N, K)), A("mask", (N, K)), A("guard", (K,), I32),
            A("u", (K, H)), A("Wv", (K, H, H)), A("q", (K, H)),
            A("Wk", (K, H, H)), A("bk", (K, H)), A("dz2", (K, H)),
            A("du", (K, H)), A("ds", (N, K)), A("dc", (K,)),
            A("dWv", (K, H, H)), A("dbv", (K, H)), A("dq", (K, H)),
            A("dWk", (K, H, H)), A("dbk", (K, H)),
            A("hpart", (K * (2 * H + 2),)), A("dwmu", (H,)), A("dbmu", (1,)),
            A("dwsig", (H,)), A("dbsig", (1,)), H ** -0.5, 1.0, 1,
            A("kl_fmu", (K,)), A("kl_fsig_c", (K,)), A("kl_pmu", (K,)),
            A("kl_psig_c", (K,)), 1.0],
        "dec_fwd": [
            A("h", (N, H)), *DEC_W, A("fmu", (K,)), A("fsig_c", (K,)),
            A("eps", (N,)), A("recon", (N,)), A("a1", (N, H)),
            A("beta", (N, K)), A("asig_pre", (N,)), A("sigma", (N,))],
        "dec_bwd": [
            A("drecon", (N,)), A("h", (N, H)), A("a1", (N, H)),
            A("beta", (N, K)), A("asig_pre", (N,)), A("sigma", (N,)),
            A("eps", (N,)), A("fmu", (K,)), A("fsig_c", (K,)),
            A("W1", (H, H)), A("wmu", (H,)), A("wsig", (H,)),
            A("Wb", (K, H)), A("dh", (N, H)), A("dz1", (N, H)),
            A("dbeta", (N, K)), A("part", (dec_part(),)), A("dfmu", (K,)),
            A("dfsig_c", (K,)), A("dwmu", (H,)), A("dbmu", (1,)),
            A("dwsig", (H,)), A("dbsig", (1,))],
        "loss_fused": [
            *LOSS_IN, A("drecon", (N,)), A("dfmu", (K,)), A("dfsig_c", (K,)),
            A("dpmu", (K,)), A("dpsig_c", (K,)), 1.0],
        "loss_scalars": list(LOSS_IN),
        "adam": [
            A("p", (37,)), A("g", (37,)), A("m", (37,)), A("v", (37,)),
            A("step_t", (1,), I32), 1e-3, 0.0, 10.0, 0.9, 0.999, 1e-8],
        "wgrad_reduce": [
            A("part", (3 * 3 * H * H,)), A("out", (3 * H, H), count=True),
            A("db_part", (3 * 3 * H,)), A("db", (3 * H,), count=True), 3,
            False],
        "attn_ctx_fwd": [
            A("u", (K, H)), A("Wv", (K, H, H)), A("bv", (K, H)),
            A("guard", (K,), I32), A("ctx", (K, H))],
        "attn_head_bwd": [
            A("dctx", (K, H)), A("u", (K, H)), A("Wv", (K, H, H)),
            A("guard", (K,), I32), A("du", (K, H)), A("dWv", (K, H, H)),
            A("dbv", (K, H))],
        "attn_softmax_bwd": [
            A("da", (N, K)), A("a", (N, K)), A("sd", (N, K)),
            A("mask", (N, K)), A("guard", (K,), I32), A("ds", (N, K)),
            A("dc", (K,)), 1.0, H ** -0.5],
        "gru_fwd": [
            A("gi", G3), A("Whh", (3 * H, H)), A("bhh", (3 * H,)), *GRU_FWD],
        "gru_fwd_mfma": [
            A("gi", G3), A("whh_bf", (3 * H, H), BF16), A("bhh", (3 * H,)),
            *GRU_FWD],
        "gru_bwd": [
            *GRU_BWD_IN, A("Whh", (3 * H, H)), A("dgi", G3), A("dgh", G3),
            N, T, H, A("dgi_bf", G3, BF16), A("dgh_bf", G3, BF16)],
        "gru_bwd_mfma": [
            *GRU_BWD_IN, A("whh_bf", (3 * H, H), BF16), A("dgi", G3),
            A("dgh", G3), N, T, H, A("dgi_bf", G3, BF16),
            A("dgh_bf", G3, BF16), A("dgi_f8", (N * T, 3 * H), FP8),
            A("s_dgi", (1,)), A("amax_dgi", (1,)),
            A("whh_part", (ext.gru_wgrad_blocks(N) * 3 * H * H,)),
            A("bhh_part", (ext.gru_wgrad_blocks(N) * 3 * H,))],
    }


OPS = ["attn_fused_fwd", "attn_fused_bwd", "dec_fwd", "dec_bwd", "loss_fused",
       "loss_scalars", "adam", "wgrad_reduce", "attn_ctx_fwd",
       "attn_head_bwd", "attn_softmax_bwd", "gru_fwd", "gru_fwd_mfma",
       "gru_bwd", "gru_bwd_mfma"]


def test_every_listed_binding_has_a_spec():
    assert sorted(specs()) == sorted(OPS)


@pytest.mark.parametrize("how", ["dtype", "noncontig", "cpu", "short"])
@pytest.mark.parametrize("op", OPS)
def test_one_broken_argument_is_refused_by_name(op, how):
    spec = specs()[op]
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


@pytest.mark.parametrize("op", ["dec_bwd", "gru_bwd_mfma"])
def test_geometry_sized_partials_are_one_short(op):
    """part and whh_part have exactly the size the exported block counts
    give, so their 'short' case above is one element short of it."""
    by_name = {a.name: a for a in specs()[op] if isinstance(a, A)}
    if op == "dec_bwd":
        assert by_name["part"].numel == ext.dec_nblk(N) * (2 * K + 2 * H + 2)
        assert by_name["part"].broken("short").numel() == dec_part() - 1
    else:
        want = ext.gru_wgrad_blocks(N) * 3 * H * H
        assert by_name["whh_part"].numel == want
        assert by_name["whh_part"].broken("short").numel() == want - 1


def test_exported_geometry():
    """The block counts against the formulas they replace, as literals."""
    assert [ext.dec_nblk(n) for n in (1, 4, 5, 512, 513, 4096, 4097)] == [
        1, 1, 2, 128, 65, 128, 129]
    assert [ext.gru_wgrad_blocks(n) for n in (1, 16, 17)] == [1, 1, 2]
