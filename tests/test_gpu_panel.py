"""The panel route (docs/KERNELS.md, "Gather recurrence and panel route"):
every gather GRU kernel against its dense kernel as bit patterns, the
missing-row rule, the extractor head's independence of a row's position, and
predict_many / evaluate_many / loss_many on a PanelDays against the same
calls on its windows(), bit for bit. Outputs start as garbage."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from factorvae_amd.ops import get_extension
    ext = get_extension()
DEV = torch.device("cuda:0")
T, C, K, M = 5, 10, 4, 6


def t(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def bits(a):
    a = a.detach().cpu()
    if a.dtype == torch.float32:
        return a.view(torch.int32)
    if a.dtype == torch.float64:
        return a.view(torch.int64)
    return a


def same(got, ref, what=""):
    """Equal as bit patterns, so NaN-aware; walks tuples, lists, dicts."""
    if isinstance(ref, dict):
        assert set(got) == set(ref), what
        for k in ref:
            same(got[k], ref[k], f"{what}[{k}]")
    elif isinstance(ref, (tuple, list)):
        assert len(got) == len(ref), what
        for i, (a, b) in enumerate(zip(got, ref)):
            same(a, b, f"{what}[{i}]")
    elif torch.is_tensor(ref):
        assert got.shape == ref.shape and got.dtype == ref.dtype, what
        a, b = bits(got), bits(ref)
        assert torch.equal(a, b), \
            f"{what}: {(a != b).sum().item()} of {b.numel()} differ"
    else:
        assert got == ref, what


# --------------------------------------------------------------- the kernels
def wave_max_n():
    return ext.gru_wave_max_n()


# name -> (H, variant, bf16, stocks per workgroup)
KERNELS = {
    "wave": (64, 1, False, 4),
    "f32_mfma": (64, 0, False, 16),
    "fast": (20, 1, False, 8),
    "generic": (18, 1, False, 4),
    "bf16_mfma": (64, 1, True, 16),
}


def indices(N, Tn, U, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    idx = torch.randint(0, U, (N, Tn), generator=g, dtype=torch.int32)
    if Tn > 1:
        idx[::2, 1] = idx[::2, 0]   # a row repeated inside a window
    return idx


def run_pair(name, N, Tn, U, idx, variant=None):
    """h_final of the dense kernel on gi_rows[idx] and of the gather kernel;
    rows of idx outside [0, U) are taken as row 0 by the dense run."""
    H, v, bf16, _ = KERNELS[name]
    v = v if variant is None else variant
    gi_rows = t(U, 3 * H, seed=1)
    Whh, bhh = t(3 * H, H, seed=2, scale=0.125), t(3 * H, seed=3, scale=0.1)
    idx_d = idx.to(DEV)
    ok = (idx_d >= 0) & (idx_d < U)
    gi = gi_rows[torch.where(ok, idx_d, 0).long()].contiguous()
    hd, hg = t(N, H, seed=10), t(N, H, seed=11)
    if bf16:
        whh_bf = Whh.bfloat16()
        ext.gru_fwd_mfma_infer(gi, whh_bf, bhh, hd, N, Tn, H)
        ext.gru_fwd_mfma_infer_gather(gi_rows, U, idx_d, whh_bf, bhh, hg, N,
                                      Tn, H)
    else:
        ext.gru_fwd_infer(gi, Whh, bhh, hd, N, Tn, H, variant=v)
        ext.gru_fwd_infer_gather(gi_rows, U, idx_d, Whh, bhh, hg, N, Tn, H,
                                 variant=v)
    torch.cuda.synchronize()
    return hd, hg


@pytest.mark.parametrize("N", [1, 70])
@pytest.mark.parametrize("name", list(KERNELS))
def test_gather_kernel_matches_dense_kernel(name, N):
    assert N == 1 or N % KERNELS[name][3] != 0
    U = 23
    hd, hg = run_pair(name, N, T, U, indices(N, T, U, seed=N))
    assert torch.isfinite(hd).all() and hd.abs().max() > 0
    same(hg, hd, f"{name} N={N}")


def test_f32_mfma_past_the_wave_cut_over():
    """variant=1 above gru_wave_max_n() stocks runs the f32 MFMA kernel."""
    N, U = wave_max_n() + 37, 301
    hd, hg = run_pair("f32_mfma", N, 3, U, indices(N, 3, U, seed=5),
                      variant=1)
    same(hg, hd, "past the cut-over")


@pytest.mark.parametrize("name", ["wave", "fast"])
def test_more_than_64_steps(name):
    """The wave and fast kernels hold a stock's row numbers 64 at a time;
    70 steps cross into the second batch."""
    N, Tn, U = 3, 70, 50
    hd, hg = run_pair(name, N, Tn, U, indices(N, Tn, U, seed=6))
    assert torch.isfinite(hd).all()
    same(hg, hd, f"{name} T=70")


@pytest.mark.parametrize("name", list(KERNELS))
def test_missing_rows(name):
    """An index of -1 and one of U: exactly those two stocks are NaN, the
    rest as without them."""
    N, U = 9, 23
    idx = indices(N, T, U, seed=7)
    clean, _ = run_pair(name, N, T, U, idx)
    bad = idx.clone()
    bad[2, 1] = -1
    bad[5, 3] = U
    _, hg = run_pair(name, N, T, U, bad)
    nan_rows = torch.isnan(hg).all(dim=1).cpu()
    assert nan_rows.tolist() == [n in (2, 5) for n in range(N)]
    keep = [n for n in range(N) if n not in (2, 5)]
    same(hg[keep], clean[keep], f"{name}: the other stocks")


def test_first_and_last_step_missing():
    """Step 0 is loaded in the prologue and the last step ahead of time."""
    N, U = 6, 23
    idx = indices(N, T, U, seed=8)
    bad = idx.clone()
    bad[1, 0] = -7
    bad[4, T - 1] = U + 5
    for name in ("wave", "fast"):
        ref, _ = run_pair(name, N, T, U, idx)
        _, hg = run_pair(name, N, T, U, bad)
        assert torch.isnan(hg).all(dim=1).cpu().tolist() == [
            n in (1, 4) for n in range(N)]
        assert torch.isfinite(ref).all()
        same(hg[[0, 2, 3, 5]], ref[[0, 2, 3, 5]], name)


# ------------------------------------------------------------ binding checks
def gather_args(bf16):
    H, N, U = 64, 5, 7
    Whh = torch.zeros(3 * H, H, device=DEV)
    a = {"gi_rows": torch.zeros(U, 3 * H, device=DEV), "U": U,
         "idx": torch.zeros(N, T, dtype=torch.int32, device=DEV),
         "Whh": Whh.bfloat16() if bf16 else Whh,
         "bhh": torch.zeros(3 * H, device=DEV),
         "h_final": torch.zeros(N, H, device=DEV), "N": N, "T": T, "H": H}
    return a


@pytest.mark.parametrize("op", ["gru_fwd_infer_gather",
                                "gru_fwd_mfma_infer_gather"])
@pytest.mark.parametrize("how", ["idx dtype", "idx short", "gi_rows short",
                                 "device"])
def test_binding_refuses_by_name(op, how):
    a = gather_args(op == "gru_fwd_mfma_infer_gather")
    if how == "idx dtype":
        a["idx"], arg = a["idx"].long(), "idx"
    elif how == "idx short":
        a["idx"], arg = a["idx"].view(-1)[:-1], "idx"
    elif how == "gi_rows short":
        a["gi_rows"], arg = a["gi_rows"].view(-1)[:-1], "gi_rows"
    else:
        a["idx"], arg = a["idx"].cpu().pin_memory(), "idx"
    with pytest.raises(RuntimeError, match=rf"{op}: {arg} "):
        getattr(ext, op)(*a.values())
    torch.cuda.synchronize()


# -------------------------------------------------------- through the engine
def make_trainer(monkeypatch, dtype, head=None, H=64):
    from factorvae_amd.engine.fused import FusedTrainer
    from factorvae_amd.models.modules import build_factorvae
    from factorvae_amd.utils import set_seed

    if head is None:
        monkeypatch.delenv("FV_F32_HEAD", raising=False)
    else:
        monkeypatch.setenv("FV_F32_HEAD", head)
    set_seed(0)
    model = build_factorvae(num_latent=C, hidden_size=H, num_portfolio=M,
                            num_factor=K).to(DEV)
    return FusedTrainer(model, lr=1e-3, t_max=100, device=DEV,
                        use_graph=False, dtype=dtype)


S = 70                               # stocks of the synthetic frame
DAY_N = [17, 1, 0, 70, 5, 70, 17]    # rows per day; day d is date d + T - 1


def make_panel(missing=None):
    """A full (date, stock) frame in frame order and ragged days on
    consecutive dates; missing = (day, stock row, step) gets id -1."""
    from factorvae_amd.data.panel import PanelDays

    n_dates = len(DAY_N) + T - 1
    g = torch.Generator(device="cpu").manual_seed(3)
    rows = torch.randn(n_dates * S, C, generator=g)
    ids, labels = [], []
    for d, n in enumerate(DAY_N):
        stocks = torch.randperm(S, generator=g)[:n].sort().values
        dates = torch.arange(d, d + T)
        m = (dates[None, :] * S + stocks[:, None]).to(torch.int32)
        if missing is not None and missing[0] == d:
            m[missing[1], missing[2]] = -1
        ids.append(m.reshape(n, T))
        labels.append(torch.randn(n, generator=g))
    return PanelDays(rows, ids, labels)


def dense_days(panel):
    return [panel.windows(d) for d in range(len(panel))]


HEADS = [("fp32", None), ("fp32", "0"), ("bf16", None)]


@pytest.mark.parametrize("dtype,head", HEADS)
def test_head_is_independent_of_row_position(monkeypatch, dtype, head):
    """gi over the row table, whole and in two uneven slices, gathered,
    against gi over the materialised windows."""
    tr = make_trainer(monkeypatch, dtype, head)
    assert tr._f32_head == (dtype == "fp32" and head is None)
    panel = make_panel().to(DEV)
    H, U = tr.H, panel.rows.shape[0]
    x2d = torch.cat([panel.windows(d)[0] for d in range(len(panel))]
                    ).reshape(-1, C).contiguous()
    idx = torch.cat(panel.ids).reshape(-1).long()
    iw = tr._alloc_infer_ws(max(U, x2d.shape[0]), 1, 1, False)
    if tr._f32_head:
        f = lambda n: torch.empty(n, device=DEV)
        p = tr.p
        assert ext.extractor_head_fwd(
            x2d, p("ln_g"), p("ln_b"), p("W1x"), p("b1x"), p("Wih"), p("bih"),
            None, f(x2d.shape[0]), f(x2d.shape[0]),
            torch.empty(x2d.shape[0], C, device=DEV),
            torch.empty(x2d.shape[0], 3 * H, device=DEV), 1e-5), \
            "the fused head does not run at this shape"
    gi_dense = t(x2d.shape[0], 3 * H, seed=20)
    tr._launch_infer_head(iw, x2d, gi_dense)
    gi_rows = t(U, 3 * H, seed=21)
    tr._launch_infer_head(iw, panel.rows, gi_rows)
    cut = 201                        # no multiple of any tile
    gi_cut = t(U, 3 * H, seed=22)
    tr._launch_infer_head(iw, panel.rows[:cut], gi_cut[:cut])
    tr._launch_infer_head(iw, panel.rows[cut:], gi_cut[cut:])
    torch.cuda.synchronize()
    assert torch.isfinite(gi_dense).all()
    same(gi_rows[idx], gi_dense, "rows, one launch")
    same(gi_cut[idx], gi_dense, "rows, two slices")


def run_calls(tr, days_or_panel, eps, max_rows):
    pm = tr.predict_many(
        days_or_panel if not isinstance(days_or_panel, list)
        else [x for x, _ in days_or_panel],
        eps=eps, return_dist=True, return_beta=True, max_rows=max_rows)
    ev = tr.evaluate_many(days_or_panel, on=("score", "mu"), topk=3, eps=eps,
                          max_rows=max_rows, with_loss=True)
    lm = tr.loss_many(days_or_panel, eps=eps, return_factors=True,
                      max_rows=max_rows)
    return {"predict_many": pm, "evaluate_many": ev, "loss_many": lm}


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_engine_panel_equals_dense(monkeypatch, dtype, where):
    tr = make_trainer(monkeypatch, dtype)
    panel = make_panel()
    if where == "device":
        panel = panel.to(DEV)
    days = dense_days(panel)
    g = torch.Generator(device="cpu").manual_seed(9)
    eps = [torch.randn(n, generator=g) for n in DAY_N]
    # 360 rows: chunks [0,1,2] [3] [4] [5] [6], head slices of 360 rows;
    # 500 panel rows: three day blocks
    max_rows = 360
    monkeypatch.setenv("FV_PANEL_ROWS", "500")
    ref = run_calls(tr, days, eps, max_rows)
    got = run_calls(tr, panel, eps, max_rows)
    same(got, ref, f"{dtype} {where}")
    assert torch.isfinite(ref["evaluate_many"]["loss"][3])
    assert ref["loss_many"]["n"].tolist() == DAY_N
    # one block and one chunk for everything: the same bits again
    monkeypatch.delenv("FV_PANEL_ROWS")
    same(tr.predict_many(panel, eps=eps, return_dist=True),
         [e[:3] for e in ref["predict_many"]], "one block")
    # eps drawn: the same chunks, so the same draws
    torch.manual_seed(5)
    drawn_ref = tr.predict_many([x for x, _ in days], max_rows=max_rows)
    torch.manual_seed(5)
    drawn = tr.predict_many(panel, max_rows=max_rows)
    same(drawn, drawn_ref, "eps=None")
    assert not torch.equal(bits(drawn[3]), bits(ref["predict_many"][3][0]))


def test_day_block_budget(monkeypatch):
    tr = make_trainer(monkeypatch, "fp32")
    panel = make_panel().to(DEV)
    monkeypatch.setenv("FV_PANEL_ROWS", "100")
    with pytest.raises(ValueError, match="FV_PANEL_ROWS"):
        tr.predict_many(panel, max_rows=360)


def test_engine_refuses_what_the_dense_calls_refuse(monkeypatch):
    from factorvae_amd.data.panel import PanelDays

    tr = make_trainer(monkeypatch, "fp32")
    ids = [torch.zeros(2, T, dtype=torch.int32)]
    with pytest.raises(ValueError, match=f"{C + 1} features"):
        tr.predict_many(PanelDays(torch.zeros(3, C + 1), ids))
    panel = PanelDays(torch.zeros(3, C), ids)
    with pytest.raises(ValueError, match="eps must have 2 entries"):
        tr.predict_many(panel, eps=[torch.zeros(3)])
    with pytest.raises(ValueError, match="needs a panel with labels"):
        tr.loss_many(panel)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_missing_row_inside_a_day(monkeypatch, dtype):
    tr = make_trainer(monkeypatch, dtype)
    day, stock = 4, 2
    panel = make_panel(missing=(day, stock, 1)).to(DEV)
    days = dense_days(panel)
    assert torch.isnan(days[day][0][stock, 1]).all()
    eps = [torch.zeros(n) for n in DAY_N]
    got = tr.predict_many(panel, eps=eps, return_dist=True, return_beta=True)
    ref = tr.predict_many([x for x, _ in days], eps=eps, return_dist=True,
                          return_beta=True)
    if dtype == "fp32":
        same(got, ref, "against the NaN window")
    else:
        # gemm_nt_bf16_rs reads a row as ceil32(C) elements against zero
        # weights, so behind a NaN x row the dense bf16 head also turns the
        # rows in front of it NaN (0 * NaN), here stock 1; the panel never
        # sends a NaN row through the head. Where the dense call is
        # finite, the bits agree.
        for d in range(len(DAY_N)):
            for a, b in zip(got[d], ref[d]):
                ok = torch.isfinite(b).all(dim=1)
                same(a[ok], b[ok], f"day {d}, where the dense call is finite")
    for out in got[day]:
        assert torch.isnan(out[stock]).all()
        assert torch.isfinite(out[[0, 1, 3, 4]]).all()
    ev = tr.evaluate_many(panel, on=("mu",), eps=eps)
    assert ev["count"][:, 0].tolist() == [
        n - (d == day) for d, n in enumerate(DAY_N)]


def test_training_is_undisturbed(monkeypatch):
    panel = make_panel().to(DEV)
    x, y = panel.windows(3)
    eps = [torch.zeros(n) for n in DAY_N]
    arenas = []
    for with_panel in (False, True):
        tr = make_trainer(monkeypatch, "fp32")
        torch.manual_seed(11)
        tr.step(x, y.view(-1, 1))
        if with_panel:
            state = torch.cuda.get_rng_state(DEV)
            run_calls(tr, panel, eps, 360)
            assert torch.equal(state, torch.cuda.get_rng_state(DEV))
        tr.step(x, y.view(-1, 1))
        torch.cuda.synchronize()
        arenas.append(tr.params.flat.clone())
    same(arenas[1], arenas[0], "parameters after two steps")
