"""On-device daily IC / RankIC / top-k evaluation: the daily_ic_seg kernel,
FusedTrainer.evaluate_many / validate_metrics and the RankIC checkpoint
selection of train_main, against the float64 oracle factorvae_amd.metrics.

Tolerance 1e-9 (absolute) on finite statistics: the inputs have unit-scale
variance, the two float64 summation orders differ by at most N * 2^-53
(about 1e-12 at N = 8192), and the ranks are exact on both sides; `count`
and the NaN positions must agree exactly."""

import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from factorvae_amd.ops import get_extension
    ext = get_extension()
from factorvae_amd.metrics import daily_ic, summarize_ic

DEV = torch.device("cuda:0")
HK = [(20, 3), (64, 20)]
T_, C_, M_ = 4, 24, 8
TOL = 1e-9
LENS = [1, 2, 0, 3, 63, 64, 65, 255, 256, 257, 300, 511, 512, 513]
STATS = ("ic", "rank_ic", "long", "short")


# ------------------------------------------------------------- helpers
def make_case(lens, kind, seed):
    """Host (3, total) prediction buffer and (total,) labels."""
    rng = np.random.default_rng(seed)
    total = sum(lens)
    buf = rng.standard_normal((3, total)).astype(np.float32)
    lab = (0.3 * buf[1] + rng.standard_normal(total)).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    if kind in ("tied", "nonfinite"):
        buf = (np.round(buf * 4) / 4).astype(np.float32)
        lab = (np.round(lab * 200) / 200).astype(np.float32)
        big = [d for d, n in enumerate(lens) if n >= 63]
        for d in big:  # both zeros in every longer day
            o, n = offs[d], lens[d]
            buf[:, o], buf[:, o + n // 2] = 0.0, -0.0
            lab[o + 1], lab[o + n - 1] = -0.0, 0.0
        if len(big) > 1:  # one all-equal day
            d = big[len(big) // 2]
            buf[:, offs[d]:offs[d + 1]] = 0.75
    if kind == "nonfinite":
        bad = np.array([np.nan, np.inf, -np.inf], np.float32)
        m = rng.random(total) < 0.10
        lab[m] = bad[np.flatnonzero(m) % 3]
        for r in range(3):
            m = rng.random(total) < 0.05
            buf[r, m] = bad[(np.flatnonzero(m) + r) % 3]
        big = [d for d, n in enumerate(lens) if n >= 63]
        if len(big) > 1:  # one day without a valid row
            d = big[0]
            lab[offs[d]:offs[d + 1]] = np.nan
    return buf, lab


def run_kernel(pred, lab, lens, topk=0, max_n=None):
    """pred: a (P, total) device view. Outputs start as garbage, so a
    store the kernel misses shows."""
    D, P = len(lens), pred.shape[0]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    seg = torch.from_numpy(offs).to(DEV)
    stats = torch.full((D, P, 4), 1234.5, dtype=torch.float64, device=DEV)
    count = torch.full((D, P), 12345, dtype=torch.int32, device=DEV)
    if max_n is None:
        max_n = max(lens) if lens else 0
    ext.daily_ic_seg(pred, lab, seg, max_n, topk, stats, count)
    torch.cuda.synchronize()
    return stats.cpu().numpy(), count.cpu().numpy()


def oracle(rows, lab, lens, topk=0):
    """rows: list of host (total,) prediction rows -> (D,P,4), (D,P)."""
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    st = np.empty((len(lens), len(rows), 4))
    cn = np.empty((len(lens), len(rows)), np.int32)
    for d in range(len(lens)):
        for p, row in enumerate(rows):
            r = daily_ic(row[offs[d]:offs[d + 1]], lab[offs[d]:offs[d + 1]],
                         topk)
            st[d, p], cn[d, p] = r[:4], r[4]
    return st, cn


def check(st, cn, ref_st, ref_cn, what):
    assert np.array_equal(cn, ref_cn), f"{what}: count {cn} vs {ref_cn}"
    nan, ref_nan = np.isnan(st), np.isnan(ref_st)
    assert np.array_equal(nan, ref_nan), \
        f"{what}: NaN positions differ at {np.argwhere(nan != ref_nan)}"
    err = np.abs(np.where(nan, 0.0, st) - np.where(nan, 0.0, ref_st))
    print(f"{what}: max abs error {err.max():.3e}")
    assert err.max() <= TOL, f"{what}: max abs error {err.max():.3e}"


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64),
                          np.ascontiguousarray(b).view(np.int64))


# -------------------------------------------------------------- kernel
@pytest.mark.parametrize("kind", ["continuous", "tied", "nonfinite"])
def test_kernel_against_oracle(kind):
    """P = 2 prediction columns taken as row views of a (3, total) buffer
    (torch has no negative strides, so the pair is rows 0 and 1 at row
    stride total, then rows 0 and 2 at row stride 2 * total)."""
    buf, lab = make_case(LENS, kind, seed=1)
    dbuf, dlab = torch.from_numpy(buf).to(DEV), torch.from_numpy(lab).to(DEV)
    for rows, view in (((0, 1), dbuf[0:2]), ((0, 2), dbuf[0::2])):
        assert view.data_ptr() == dbuf.data_ptr()  # a view, not a copy
        st, cn = run_kernel(view, dlab, LENS)
        ref_st, ref_cn = oracle([buf[r] for r in rows], lab, LENS)
        check(st, cn, ref_st, ref_cn, f"{kind} rows {rows}")
    assert cn[2, 0] == 0  # the empty day
    if kind == "nonfinite":
        assert (cn[4] == 0).all() and np.isnan(st[4]).all()


@pytest.mark.parametrize("n", [3500, 8192])
def test_kernel_single_long_day(n):
    buf, lab = make_case([n], "tied", seed=2)
    dbuf, dlab = torch.from_numpy(buf).to(DEV), torch.from_numpy(lab).to(DEV)
    st, cn = run_kernel(dbuf[0:2], dlab, [n], topk=50)
    ref_st, ref_cn = oracle([buf[0], buf[1]], lab, [n], topk=50)
    check(st, cn, ref_st, ref_cn, f"N={n}")


@pytest.mark.parametrize("k", [1, 50, 10000])
def test_kernel_topk(k):
    buf, lab = make_case(LENS, "tied", seed=3)
    dbuf, dlab = torch.from_numpy(buf).to(DEV), torch.from_numpy(lab).to(DEV)
    st, cn = run_kernel(dbuf[0:2], dlab, LENS, topk=k)
    ref_st, ref_cn = oracle([buf[0], buf[1]], lab, LENS, topk=k)
    check(st, cn, ref_st, ref_cn, f"topk={k}")
    assert np.isfinite(st[-1, :, 2:]).all()


def test_kernel_position_independence():
    """A day alone and as the first, middle and last segment of a batch:
    identical float64 bit patterns for all four statistics."""
    n = 300
    day, dlab_day = make_case([n], "tied", seed=4)
    other, olab = make_case([513, 65], "continuous", seed=5)
    alone, cn = run_kernel(torch.from_numpy(day).to(DEV)[0:2],
                           torch.from_numpy(dlab_day).to(DEV), [n], topk=50)
    assert cn[0, 0] == n and np.isfinite(alone).all()
    for pos in range(3):
        lens = [513, 65]
        lens.insert(pos, n)
        parts, lparts = [other[:, :513], other[:, 513:]], [olab[:513], olab[513:]]
        parts.insert(pos, day)
        lparts.insert(pos, dlab_day)
        buf = np.ascontiguousarray(np.concatenate(parts, axis=1))
        lab = np.concatenate(lparts)
        st, _ = run_kernel(torch.from_numpy(buf).to(DEV)[0:2],
                           torch.from_numpy(lab).to(DEV), lens, topk=50)
        assert same_bits(st[pos], alone[0]), f"position {pos}"


def test_kernel_refusals():
    """A day longer than the launch's plan is not read: count -1, NaN; the
    other days are unchanged bit for bit. Above the 8192 cap the wrapper
    raises."""
    lens = [5, 300, 64, 0]
    buf, lab = make_case(lens, "continuous", seed=6)
    dbuf, dlab = torch.from_numpy(buf).to(DEV), torch.from_numpy(lab).to(DEV)
    full, cn_full = run_kernel(dbuf[0:2], dlab, lens, topk=3)
    st, cn = run_kernel(dbuf[0:2], dlab, lens, topk=3, max_n=64)
    assert (cn[1] == -1).all() and np.isnan(st[1]).all()
    for d in (0, 2, 3):
        assert same_bits(st[d], full[d]) and (cn[d] == cn_full[d]).all()
    # offsets that leave the packed rows
    seg = torch.tensor([0, 5, 9999, 5, 400], dtype=torch.int32, device=DEV)
    stats = torch.full((4, 2, 4), 1.5, dtype=torch.float64, device=DEV)
    count = torch.full((4, 2), 7, dtype=torch.int32, device=DEV)
    ext.daily_ic_seg(dbuf[0:2], dlab, seg, 8192, 3, stats, count)
    torch.cuda.synchronize()
    assert count[:, 0].tolist() == [5, -1, -1, -1]
    assert same_bits(stats[0].cpu().numpy(), full[0])
    assert torch.isnan(stats[1:]).all()
    with pytest.raises(RuntimeError):
        ext.daily_ic_seg(dbuf[0:2], dlab, seg, 8193, 3, stats, count)


# --------------------------------------------------- through the engine
def _trainer(H, K, dtype="fp32", seed=0):
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    set_seed(seed)
    model = build_factorvae(num_latent=C_, hidden_size=H, num_portfolio=M_,
                            num_factor=K).to(DEV)
    return FusedTrainer(model, lr=1e-3, t_max=100, device=DEV,
                        use_graph=False, train=False, dtype=dtype)


def _days(lens, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    xs = [torch.randn(n, T_, C_, generator=g).to(DEV) for n in lens]
    ys = [torch.randn(n, 1, generator=g) for n in lens]
    eps = [torch.randn(n, generator=g).to(DEV) for n in lens]
    return xs, ys, eps


def _oracle_days(outs, ys, on, topk):
    """daily_ic on predict_many(return_dist=True) host outputs."""
    col = {"score": 0, "mu": 1}
    D, P = len(outs), len(on)
    st = np.empty((D, P, 4))
    cn = np.empty((D, P), np.int32)
    for d, (o, y) in enumerate(zip(outs, ys)):
        for p, c in enumerate(on):
            r = daily_ic(o[col[c]].numpy(), y.numpy(), topk)
            st[d, p], cn[d, p] = r[:4], r[4]
    return st, cn


def _stack(res):
    return np.stack([res[k].numpy() for k in STATS], axis=-1)


EVAL_LENS = [5, 64, 1, 0, 257]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("H,K", HK)
def test_evaluate_many_matches_oracle(H, K, dtype):
    tr = _trainer(H, K, dtype)
    xs, ys, eps = _days(EVAL_LENS, seed=900)
    ys[1][3] = float("nan")
    ys[4][::9] = float("inf")
    on = ("score", "mu")
    before = tr.predict_many(xs, eps=eps, return_dist=True, return_beta=True)
    res = tr.evaluate_many(list(zip(xs, ys)), on=on, topk=3, eps=eps)
    assert res["columns"] == on
    assert res["count"].dtype == torch.int32 and res["ic"].dtype == torch.float64
    ref_st, ref_cn = _oracle_days(before, ys, on, 3)
    check(_stack(res), res["count"].numpy(), ref_st, ref_cn,
          f"H={H} K={K} {dtype}")
    assert res["count"][:, 0].tolist() == [5, 63, 1, 0, 257 - 29]
    # columns in the other order, and a single one
    swapped = tr.evaluate_many(list(zip(xs, ys)), on=("mu", "score"), topk=3,
                               eps=eps)
    assert same_bits(_stack(swapped)[:, ::-1], _stack(res))
    only_mu = tr.evaluate_many(list(zip(xs, ys)), topk=3)
    assert same_bits(_stack(only_mu)[:, 0], _stack(res)[:, 1])

    # three chunks: same bits
    calls = []
    real = tr._launch_predict_many
    tr._launch_predict_many = lambda *a, **k: (calls.append(a[2]), real(*a, **k))
    try:
        chunked = tr.evaluate_many(list(zip(xs, ys)), on=on, topk=3, eps=eps,
                                   max_rows=260)
    finally:
        del tr._launch_predict_many
    assert calls == [5, 65, 257]
    assert same_bits(_stack(chunked), _stack(res))
    assert torch.equal(chunked["count"], res["count"])

    # a larger evaluation grows the workspace; predict_many is undisturbed
    xs2, ys2, _ = _days([600, 7], seed=950)
    grown = tr.evaluate_many(list(zip(xs2, ys2)))
    assert grown["count"].reshape(-1).tolist() == [600, 7]
    after = tr.predict_many(xs, eps=eps, return_dist=True, return_beta=True)
    for b, a in zip(before, after):
        for tb, ta in zip(b, a):
            assert torch.equal(tb.view(torch.int32), ta.view(torch.int32))


def test_evaluate_many_edges():
    tr = _trainer(20, 3)
    assert tr.evaluate_many([])["ic"].shape == (0, 1)
    xs, ys, _ = _days([0, 0], seed=960)
    res = tr.evaluate_many(list(zip(xs, ys)), topk=2)
    assert res["count"].reshape(-1).tolist() == [0, 0]
    assert torch.isnan(res["rank_ic"]).all()
    with pytest.raises(ValueError):
        tr.evaluate_many(list(zip(xs, ys)), on=("sigma",))
    state = torch.cuda.get_rng_state(DEV)
    xs, ys, _ = _days([9], seed=961)
    tr.evaluate_many(list(zip(xs, ys)))
    assert torch.equal(state, torch.cuda.get_rng_state(DEV))
    tr8 = _trainer(64, 20, dtype="fp8")
    with pytest.raises(ValueError, match="fp8"):
        tr8.evaluate_many(list(zip(xs, ys)))


@pytest.mark.parametrize("H,K", HK)
def test_validate_metrics_matches_oracle_summary(H, K):
    tr = _trainer(H, K)
    lens = [40, 64, 0, 37, 1, 90, 65]
    xs, ys, eps = _days(lens, seed=970)
    ys[3][5] = float("nan")
    outs = tr.predict_many(xs, eps=eps, return_dist=True)
    st, _ = _oracle_days(outs, ys, ("mu",), 5)
    ref = summarize_ic({k: st[:, 0, i] for i, k in enumerate(STATS)})
    got = tr.validate_metrics(list(zip(xs, ys)), topk=5)
    assert set(got) == {"IC", "ICIR", "RankIC", "RankIC_IR", "long_short",
                        "n_days"}
    assert got["n_days"] == ref["n_days"] == 5
    for k in ("IC", "ICIR", "RankIC", "RankIC_IR", "long_short"):
        assert abs(got[k] - ref[k]) <= TOL, (k, got[k], ref[k])


@pytest.mark.timeout(300)
def test_train_main_fused_select_by_rankic(tmp_path, monkeypatch):
    from factorvae_amd.data.synthetic import make_synthetic_frame
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.engine.trainer import train_main
    from factorvae_amd.utils import DataArgument, checkpoint_path

    seen = {}
    real = FusedTrainer.validate_metrics

    def spy(self, days, topk=0):
        seen["trainer"], seen["days"] = self, days
        return real(self, days, topk=topk)

    monkeypatch.setattr(FusedTrainer, "validate_metrics", spy)
    df = make_synthetic_frame(n_days=60, n_stocks=64, seed=11,
                              signal_strength=1.0, label_from_features=True)
    args = SimpleNamespace(
        num_epochs=2, lr=1e-3, num_latent=158, num_portfolio=32,
        seq_len=8, num_factor=8, hidden_size=64, seed=0,
        run_name="gpu_rankic", save_dir=str(tmp_path), dataset=None,
        engine="fused", dtype="fp32", wandb=False, resume=False,
        select_by="rankic", val_topk=5,
    )
    data_args = DataArgument(
        start_time="2015-01-01", end_time="2015-12-31",
        fit_end_time="2015-03-01", val_start_time="2015-03-02",
        val_end_time="2015-03-25", seq_len=8,
    )
    best = train_main(args, data_args, df=df)
    assert best == best and best < 1e6
    ckpt = checkpoint_path(str(tmp_path), args.run_name, 8, 64, 32, 0)
    assert os.path.exists(ckpt) and os.path.exists(ckpt + ".opt")
    side = torch.load(ckpt + ".opt", map_location="cpu", weights_only=True)
    assert side["select_by"] == "rankic" and "fused_opt" in side
    recs = [json.loads(line) for line in
            open(os.path.join(str(tmp_path), "gpu_rankic_metrics.jsonl"))]
    epochs = [r for r in recs if "Train Loss" in r]
    assert len(epochs) == 2
    for r in epochs:
        for k in ("Validation IC", "Validation RankIC",
                  "Validation RankIC_IR", "Validation long_short"):
            assert k in r
    assert side["best_val_rankic"] == max(r["Validation RankIC"]
                                          for r in epochs)
    assert recs[-1]["Best Validation RankIC"] == side["best_val_rankic"]

    # the last epoch's logged RankIC, recomputed from the final weights
    tr, days = seen["trainer"], seen["days"]
    again = real(tr, days, topk=5)
    assert abs(again["RankIC"] - epochs[-1]["Validation RankIC"]) <= TOL
    outs = tr.predict_many([x for x, _ in days], return_dist=True)
    st, _ = _oracle_days(outs, [y.cpu() for _, y in days], ("mu",), 5)
    ref = summarize_ic({k: st[:, 0, i] for i, k in enumerate(STATS)})
    assert abs(ref["RankIC"] - epochs[-1]["Validation RankIC"]) <= TOL
    assert abs(ref["long_short"] - epochs[-1]["Validation long_short"]) <= TOL
