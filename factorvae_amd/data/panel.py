"""Trading days as one row table plus per-day index matrices.

A day reaches the model as an (N, T, C) block of windows, and the sampler
builds that block as ``data_arr[ids]`` with an (N, T) matrix of row numbers
into the sorted (datetime, instrument) frame. Consecutive days share T - 1
of their T rows per stock, so a date range held as windows repeats every
feature row up to T times. `PanelDays` keeps each referenced row once and
the index matrices beside it; `windows(d)` materialises a day exactly as
the loader would have delivered it.

Whatever is computed row by row under fixed weights (the extractor head in
front of the GRU) can then run once per row instead of once per window
position: FusedTrainer.predict_many / evaluate_many / loss_many take a
PanelDays in place of their list of days.
"""

from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch


class PanelDays:
    """rows (U, C) float32, each referenced (stock, date) feature row once;
    ids: one (N_d, T) int32 matrix of row numbers into `rows` per day, a
    negative entry meaning "no row" (the sampler's NaN sentinel); labels:
    one (N_d,) float32 vector per day, or None; dates: optional, one per
    day. Host or device; `to()` moves all of it."""

    def __init__(self, rows, ids: Sequence, labels: Optional[Sequence] = None,
                 dates: Optional[Sequence] = None):
        rows = torch.as_tensor(rows)
        if rows.ndim != 2 or rows.dtype != torch.float32:
            raise ValueError("rows must be (U, C) float32, got "
                             f"{tuple(rows.shape)} {rows.dtype}")
        ids = [torch.as_tensor(m) for m in ids]
        U = rows.shape[0]
        T = None
        span = []
        for d, m in enumerate(ids):
            if m.dtype != torch.int32 or m.ndim != 2:
                raise ValueError(f"day {d}: ids must be (N, T) int32, got "
                                 f"{tuple(m.shape)} {m.dtype}")
            if T is None:
                T = m.shape[1]
            if m.shape[1] != T:
                raise ValueError(f"day {d}: ids have T = {m.shape[1]}, the "
                                 f"days before it T = {T}")
            valid = m[m >= 0]
            if valid.numel() == 0:
                span.append(None)
                continue
            lo, hi = int(valid.min()), int(m.max())
            if hi >= U:
                raise ValueError(f"day {d}: id {hi} is outside the {U} rows")
            span.append((lo, hi))
        if labels is not None:
            labels = [torch.as_tensor(y).reshape(-1) for y in labels]
            if len(labels) != len(ids):
                raise ValueError(f"{len(labels)} label vectors for "
                                 f"{len(ids)} days")
            for d, (y, m) in enumerate(zip(labels, ids)):
                if y.dtype != torch.float32 or y.numel() != m.shape[0]:
                    raise ValueError(
                        f"day {d}: labels must be ({m.shape[0]},) float32, "
                        f"got {tuple(y.shape)} {y.dtype}")
        if dates is not None and len(dates) != len(ids):
            raise ValueError(f"{len(dates)} dates for {len(ids)} days")
        self.rows = rows.contiguous()
        self.ids = [m.contiguous() for m in ids]
        self.labels = labels
        self.dates = list(dates) if dates is not None else None
        self.T = T
        # (lowest, highest) row number each day references, None without any
        self.span = span

    @classmethod
    def from_loader(cls, loader) -> "PanelDays":
        """The days of a day-batched loader (init_data_loader), in the
        order of its batch sampler. Features are data_arr[:, :-1], the
        label is the last column of each window's last row, as the engines
        take them from the loader's batch."""
        sampler = loader.dataset.sampler
        index = sampler.get_index()
        per_day, dates = [], []
        for group in loader.batch_sampler:
            per_day.append(sampler.window_ids(group))
            dates.append(index[group[0]][0] if len(group) else None)
        T = sampler.step_len
        every = (np.concatenate([m.reshape(-1) for m in per_day])
                 if per_day else np.empty(0, dtype=np.int64))
        # sorted, so the table keeps frame order: consecutive days then
        # reference one contiguous range of it
        uniq = np.unique(every[every >= 0])
        arr = sampler.data_arr
        rows = np.ascontiguousarray(arr[uniq, :-1], dtype=np.float32)
        ids, labels = [], []
        for m in per_day:
            m = m.reshape(-1, T)
            local = np.where(m >= 0, np.searchsorted(uniq, m), -1)
            ids.append(torch.from_numpy(local.astype(np.int32)))
            # a window's last row; -1 picks the trailing all-NaN row
            labels.append(torch.from_numpy(
                arr[m[:, -1], -1].astype(np.float32)))
        return cls(torch.from_numpy(rows), ids, labels, dates)

    def __len__(self) -> int:
        return len(self.ids)

    @property
    def C(self) -> int:
        return self.rows.shape[1]

    @property
    def device(self) -> torch.device:
        return self.rows.device

    def lens(self) -> List[int]:
        return [int(m.shape[0]) for m in self.ids]

    def windows(self, d: int):
        """Day d as the dense calls take it: (x (N_d, T, C), y (N_d,) or
        None), x = rows[ids[d]] with NaN rows where the id is negative."""
        m = self.ids[d].long()
        x = self.rows[m.clamp(min=0)]
        x[m < 0] = float("nan")
        return x, (self.labels[d] if self.labels is not None else None)

    def to(self, device) -> "PanelDays":
        new = object.__new__(PanelDays)
        new.rows = self.rows.to(device)
        new.ids = [m.to(device) for m in self.ids]
        new.labels = (None if self.labels is None
                      else [y.to(device) for y in self.labels])
        new.dates, new.T, new.span = self.dates, self.T, self.span
        return new
