"""PanelDays (data/panel.py): the sampler's gather ids in public, a date
range held once per (stock, date) row, and the --panel / --val_panel
switches, which on the eager engine must change nothing."""

import filecmp
import json

import numpy as np
import pytest
import torch

from factorvae_amd.data.panel import PanelDays
from factorvae_amd.data.sampler import TSDataSampler, init_data_loader
from factorvae_amd.data.synthetic import make_synthetic_frame


def frame(n_features=10):
    return make_synthetic_frame(n_days=40, n_stocks=30, n_features=n_features,
                                seed=2, ragged=True)


# --------------------------------------------------------------- window_ids
@pytest.mark.parametrize("fill", ["none", "ffill", "ffill+bfill"])
@pytest.mark.parametrize("T", [1, 6])
def test_window_ids_gather_what_the_sampler_returns(T, fill):
    df = frame()
    dates = df.index.levels[0]
    s = TSDataSampler(df, dates[10], dates[-1], step_len=T, fillna_type=fill)
    idx = list(range(0, len(s), 7)) + [len(s) - 1]
    ids = s.window_ids(idx)
    assert ids.shape == (len(idx), T) and ids.dtype == np.int64
    assert ids.min() >= -1 and ids.max() < len(s.data_arr) - 1
    if fill == "none" and T > 1:
        assert (ids < 0).any()      # the ragged frame does have gaps
    if fill == "ffill+bfill":
        assert (ids >= 0).all()
    data, _ = s[idx]
    np.testing.assert_array_equal(s.data_arr[ids], data)   # NaN == NaN
    one, _ = s[idx[3]]
    np.testing.assert_array_equal(s.data_arr[ids[3]], one)
    with pytest.raises(KeyError):
        s.window_ids([len(s)])


# -------------------------------------------------------------- from_loader
def loader_and_panel(T=6):
    df = frame()
    dates = df.index.levels[0]
    loader = init_data_loader(df, step_len=T, shuffle=False, start=dates[10],
                              end=dates[-1])
    return loader, PanelDays.from_loader(loader)


def test_from_loader_reproduces_the_loader():
    loader, panel = loader_and_panel()
    batches = [b for b, _ in loader]
    assert len(panel) == len(batches) == 30
    index = loader.dataset.get_index()
    row = 0
    for d, b in enumerate(batches):
        x, y = panel.windows(d)
        assert x.dtype == torch.float32 and y.dtype == torch.float32
        assert torch.equal(x.view(torch.int32),
                           b[:, :, :-1].float().view(torch.int32))
        assert torch.equal(y.view(torch.int32),
                           b[:, -1, -1].float().view(torch.int32))
        assert panel.dates[d] == index[row][0]
        row += b.shape[0]
    assert panel.lens() == [b.shape[0] for b in batches]


def test_rows_hold_every_referenced_row_once_in_frame_order():
    loader, panel = loader_and_panel()
    s = loader.dataset.sampler
    every = np.concatenate([s.window_ids(g).reshape(-1)
                            for g in loader.batch_sampler])
    frame_rows = np.unique(every[every >= 0])     # sorted: frame order
    assert panel.rows.shape == (len(frame_rows), 10)
    np.testing.assert_array_equal(panel.rows.numpy(),
                                  s.data_arr[frame_rows, :-1])
    used = torch.cat([m.reshape(-1) for m in panel.ids])
    assert torch.equal(torch.unique(used),
                       torch.arange(len(frame_rows), dtype=torch.int32))
    assert len(panel.rows) < sum(n * panel.T for n in panel.lens())
    # six consecutive days reference one range of at most 6 + T - 1 dates
    lo = min(s_[0] for s_ in panel.span[3:9])
    hi = max(s_[1] for s_ in panel.span[3:9])
    assert hi - lo + 1 <= (6 + panel.T - 1) * 30
    assert hi - lo + 1 < len(panel.rows) // 2


# -------------------------------------------------------------- constructor
def small(**over):
    a = {"rows": torch.zeros(7, 3),
         "ids": [torch.zeros(2, 4, dtype=torch.int32),
                 torch.full((3, 4), 6, dtype=torch.int32)],
         "labels": [torch.zeros(2), torch.zeros(3)]}
    a.update(over)
    return a


def test_constructor_accepts_and_refuses():
    p = PanelDays(**small())
    assert len(p) == 2 and p.T == 4 and p.C == 3 and p.span == [(0, 0), (6, 6)]
    assert PanelDays(**small(labels=None)).windows(1)[1] is None
    bad = {
        "rows must be": small(rows=torch.zeros(7, 3, dtype=torch.float64)),
        "ids must be": small(ids=[torch.zeros(2, 4, dtype=torch.int64)],
                             labels=None),
        "T = 5": small(ids=[torch.zeros(2, 4, dtype=torch.int32),
                            torch.zeros(3, 5, dtype=torch.int32)]),
        "id 7 is outside the 7 rows": small(
            ids=[torch.zeros(2, 4, dtype=torch.int32),
                 torch.full((3, 4), 7, dtype=torch.int32)]),
        "labels must be": small(labels=[torch.zeros(2), torch.zeros(4)]),
        "1 label vectors": small(labels=[torch.zeros(2)]),
    }
    for msg, args in bad.items():
        with pytest.raises(ValueError, match=msg):
            PanelDays(**args)


def test_row_table_without_a_feature_axis_is_refused():
    """rows must be (U, C); that C is the model's is the engine's check
    (tests/test_gpu_panel.py)."""
    with pytest.raises(ValueError, match="rows must be"):
        PanelDays(torch.zeros(7), [torch.zeros(2, 4, dtype=torch.int32)])


def test_negative_id_is_a_nan_row():
    ids = torch.tensor([[0, -1, 2], [1, 1, -5]], dtype=torch.int32)
    rows = torch.arange(9, dtype=torch.float32).view(3, 3)
    p = PanelDays(rows, [ids, torch.zeros(0, 3, dtype=torch.int32)])
    x, y = p.windows(0)
    assert y is None and x.shape == (2, 3, 3)
    assert torch.isnan(x[0, 1]).all() and torch.isnan(x[1, 2]).all()
    assert torch.equal(x[0, 0], rows[0]) and torch.equal(x[1, 1], rows[1])
    assert torch.equal(rows, torch.arange(9.).view(3, 3))   # rows untouched
    assert p.span == [(0, 2), None]
    assert p.windows(1)[0].shape == (0, 3, 3)


# ------------------------------------------------------------ command lines
def test_score_panel_writes_the_same_files(tmp_path):
    from factorvae_amd import score as score_mod
    from factorvae_amd.models.modules import build_factorvae

    pkl = tmp_path / "d.pkl"
    frame(n_features=158).to_pickle(pkl)
    torch.manual_seed(0)
    ckpt = tmp_path / "m.pt"
    torch.save(build_factorvae(num_latent=158, hidden_size=16,
                               num_portfolio=8, num_factor=4).state_dict(),
               ckpt)
    names = set()
    for sub, extra in (("dense", []), ("panel", ["--panel"])):
        score_mod.main([
            "--checkpoint", str(ckpt), "--dataset", str(pkl),
            "--run_name", "t", "--num_factor", "4", "--hidden_size", "16",
            "--num_latent", "158", "--num_portfolio", "8",
            "--seq_length", "6", "--out_dir", str(tmp_path / sub),
            "--engine", "eager", "--dist", "--risk_aversion", "0.5",
            "--factors", "--metrics", "--metrics_topk", "5"] + extra)
        names = {p.name for p in (tmp_path / sub).iterdir()}
        assert len([n for n in names if n.endswith(".csv")]) == 3
    for name in names:
        assert filecmp.cmp(tmp_path / "dense" / name,
                           tmp_path / "panel" / name, shallow=False), name


def test_val_panel_is_ignored_by_the_eager_engine(tmp_path):
    from factorvae_amd import main as main_mod

    pkl = tmp_path / "d.pkl"
    make_synthetic_frame(n_days=40, n_stocks=12, n_features=10, seed=0,
                         start="2015-01-01").to_pickle(pkl)
    keys = []
    for sub, extra in (("a", []), ("b", ["--val_panel"])):
        main_mod.main([
            "--num_epochs", "1", "--num_latent", "10", "--num_portfolio",
            "12", "--seq_len", "5", "--num_factor", "4", "--hidden_size",
            "8", "--dataset", str(pkl), "--start_time", "2015-01-01",
            "--fit_end_time", "2015-02-10", "--val_start_time", "2015-02-11",
            "--val_end_time", "2015-02-25", "--end_time", "2015-02-25",
            "--run_name", "u", "--save_dir", str(tmp_path / sub),
            "--num_workers", "0", "--engine", "eager", "--val_metrics"]
            + extra)
        with open(tmp_path / sub / "u_metrics.jsonl") as f:
            rec = json.loads(f.readline())
        assert np.isfinite(rec["Validation Loss"])
        keys.append(sorted(rec))
    assert keys[0] == keys[1] and "Validation RankIC" in keys[0]
