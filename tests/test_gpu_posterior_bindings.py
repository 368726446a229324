"""Argument checks of the posterior-pass bindings (enc_seg_fwd,
enc_seg_heads, loss_seg), by the method of test_gpu_binding_checks: one
valid argument set per binding; then, once per tensor argument, exactly one
property is broken and the call must raise a RuntimeError that names that
argument. The calls are refused on the host, so nothing is launched. Should
a check be missing, the launch still stays inside its allocations:
  - a tensor with too few elements is a leading slice of a full-size one;
  - a tensor of the wrong dtype has at least as many bytes as the right one;
  - a non-contiguous tensor is a strided view of a buffer twice the size;
  - a CPU tensor is in pinned host memory, which the GPU can address.
A one-element tensor is always contiguous, so that case does not exist. The
day count comes from an output (yp, fmu), never from seg_off, so a shorter
seg_off is refused too. recon and y give the row count together and are
reported together."""

import re

import pytest
import torch

from factorvae_amd.ops import get_extension

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    ext = get_extension()
    DEV = torch.device("cuda:0")

D, N, H, K, M = 2, 5, 8, 3, 4
F32, I32 = torch.float32, torch.int32
# a dtype that is wrong and at least as wide
WIDER = {F32: torch.float64, I32: torch.int64}


class A:
    """One tensor argument: name, shape, dtype."""

    def __init__(self, name, shape, dtype=F32):
        self.name, self.shape, self.dtype = name, tuple(shape), dtype

    @property
    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def valid(self):
        if self.name == "seg_off":
            return torch.tensor([0, 2, N], dtype=I32, device=DEV)
        return torch.ones(self.shape, dtype=self.dtype, device=DEV)

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
        v = self.valid().view(-1)[:self.numel - 1]
        assert v.numel() == self.numel - 1
        return v


def specs():
    """op -> argument list, tensors as A and everything else as it is."""
    return {
        "enc_seg_fwd": [
            A("h", (N, H)), A("seg_off", (D + 1,), I32), 3,
            A("Wenc", (M, H)), A("benc", (M,)), A("y", (N,)),
            A("yp", (D, M))],
        "enc_seg_heads": [
            A("yp", (D, M)), A("Wmu", (K, M)), A("bmu", (K,)),
            A("Wsig", (K, M)), A("bsig", (K,)), A("fmu", (D, K)),
            A("fsig_c", (D, K))],
        "loss_seg": [
            A("recon", (N,)), A("y", (N,)), A("seg_off", (D + 1,), I32),
            A("fmu", (D, K)), A("fsig_c", (D, K)), A("pmu", (D, K)),
            A("psig_c", (D, K)), A("loss", (D,)), A("mse", (D,)),
            A("kl", (D,))],
    }


OPS = ["enc_seg_fwd", "enc_seg_heads", "loss_seg"]


@pytest.mark.parametrize("op", OPS)
def test_the_valid_argument_set_runs(op):
    args = [x.valid() if isinstance(x, A) else x for x in specs()[op]]
    getattr(ext, op)(*args)
    torch.cuda.synchronize()
    outs = {"enc_seg_fwd": args[-1:], "enc_seg_heads": args[-2:],
            "loss_seg": args[-3:]}[op]
    assert all(bool(torch.isfinite(o).all()) for o in outs)


@pytest.mark.parametrize("how", ["dtype", "noncontig", "cpu", "short"])
@pytest.mark.parametrize("op", OPS)
def test_one_broken_argument_is_refused_by_name(op, how):
    spec = specs()[op]
    fn = getattr(ext, op)
    tensors = [a for a in spec if isinstance(a, A)]
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
    # every tensor argument has every case here
    assert tried == len(tensors), (op, how, tried)
