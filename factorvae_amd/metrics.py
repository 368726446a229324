"""Daily ranking metrics (IC, RankIC, top-k long/short) in numpy float64.

The eager/CPU implementation of the evaluation feature, and the oracle of
the on-device kernel `daily_ic_seg` (ops/hip/metrics.hip), which follows
the same definitions:

- a row is valid when its prediction and its label are both finite; all
  statistics run over the valid rows only (`n_valid`);
- `ic`: Pearson correlation, two-pass (means, then centred sums); fewer
  than two valid rows or zero variance on either side give NaN;
- ranks: 1-based average ranks (ties share the mean of their positions,
  as scipy.stats.rankdata / pandas.Series.rank; -0.0 ties +0.0);
- `rank_ic`: Pearson correlation of the two rank vectors, centred on the
  exact mean (n_valid + 1) / 2;
- `long` / `short`: mean label of the k = min(topk, n_valid) valid rows
  with the highest / lowest prediction; among equal predictions the
  higher row index counts as higher. topk == 0 or no valid row gives NaN.
"""

from __future__ import annotations

from typing import Dict, Iterable, Sequence, Tuple

import numpy as np

COLUMNS = ("score", "mu")
NAN = float("nan")


def _avg_ranks(v: np.ndarray) -> np.ndarray:
    """1-based average ranks: a value's tie group occupies the sorted
    positions [lo, hi), its rank is (lo + hi + 1) / 2."""
    s = np.sort(v)
    lo = np.searchsorted(s, v, side="left")
    hi = np.searchsorted(s, v, side="right")
    return (lo + hi + 1) * 0.5


def _corr(a: np.ndarray, b: np.ndarray, ma: float, mb: float) -> float:
    da, db = a - ma, b - mb
    saa, sbb, sab = float(da @ da), float(db @ db), float(da @ db)
    if not (saa > 0.0 and sbb > 0.0):
        return NAN
    return sab / float(np.sqrt(saa * sbb))


def daily_ic(pred, label, topk: int = 0
             ) -> Tuple[float, float, float, float, int]:
    """(ic, rank_ic, long, short, n_valid) of one day's cross-section."""
    p32 = np.asarray(pred).reshape(-1)
    l32 = np.asarray(label).reshape(-1)
    if p32.shape != l32.shape:
        raise ValueError(f"pred has {p32.size} rows, label {l32.size}")
    ok = np.isfinite(p32) & np.isfinite(l32)
    # + 0.0 turns -0.0 into +0.0, so the two tie in every ordering below
    p = p32[ok].astype(np.float64) + 0.0
    l = l32[ok].astype(np.float64) + 0.0
    n = int(p.size)
    ic = rank_ic = long_ret = short_ret = NAN
    if n >= 2:
        with np.errstate(over="ignore", invalid="ignore"):
            ic = _corr(p, l, float(p.sum() / n), float(l.sum() / n))
        mr = 0.5 * (n + 1)
        rank_ic = _corr(_avg_ranks(p), _avg_ranks(l), mr, mr)
    k = min(int(topk), n)
    if k > 0:
        order = np.lexsort((np.arange(n), p))  # ascending, index breaks ties
        long_ret = float(l[order[n - k:]].sum() / k)
        short_ret = float(l[order[:k]].sum() / k)
    return ic, rank_ic, long_ret, short_ret, n


def _finite_mean(v: np.ndarray) -> float:
    v = v[np.isfinite(v)]
    return float(np.mean(v)) if v.size else NAN


def _ir(v: np.ndarray) -> float:
    v = v[np.isfinite(v)]
    if not v.size:
        return NAN
    std = float(np.std(v))  # ddof=0, as utils.RankIC
    return float(np.mean(v)) / std if std != 0 else NAN


def summarize_ic(per_day: Dict) -> Dict[str, float]:
    """Summary of per-day values (a dict with 1-D or (D,1) arrays `ic`,
    `rank_ic`, `long`, `short`): means over the days whose value is finite,
    IR = mean / std(ddof=0) (utils.RankIC's convention; zero std -> NaN),
    long_short = mean of long - short, n_days = days with finite RankIC."""
    g = lambda name: np.asarray(per_day[name], dtype=np.float64).reshape(-1)
    ic, ric = g("ic"), g("rank_ic")
    return {
        "IC": _finite_mean(ic),
        "ICIR": _ir(ic),
        "RankIC": _finite_mean(ric),
        "RankIC_IR": _ir(ric),
        "long_short": _finite_mean(g("long") - g("short")),
        "n_days": int(np.isfinite(ric).sum()),
    }


def evaluate_preds(preds: Iterable[Sequence], labels: Iterable,
                   columns: Sequence[str], topk: int = 0) -> Dict:
    """daily_ic over days: preds[d] holds one array per column. Returns the
    per-day dict FusedTrainer.evaluate_many returns (numpy arrays)."""
    rows = [[daily_ic(c, y, topk) for c in cols]
            for cols, y in zip(preds, labels)]
    D, P = len(rows), len(columns)
    a = np.array([[r[:4] for r in day] for day in rows],
                 dtype=np.float64).reshape(D, P, 4)
    cnt = np.array([[r[4] for r in day] for day in rows],
                   dtype=np.int32).reshape(D, P)
    return {"columns": tuple(columns), "ic": a[:, :, 0], "rank_ic": a[:, :, 1],
            "long": a[:, :, 2], "short": a[:, :, 3], "count": cnt}


def check_columns(on) -> Tuple[str, ...]:
    on = (on,) if isinstance(on, str) else tuple(on)
    if not on or len(set(on)) != len(on) or any(c not in COLUMNS for c in on):
        raise ValueError(f"on must be a non-empty subset of {COLUMNS}, "
                         f"got {on}")
    return on


FACTOR_KEYS = ("post_mu", "post_sigma", "prior_mu", "prior_sigma")


def loss_days_eager(model, days, eps=None, sample: bool = True,
                    return_factors: bool = False) -> Dict:
    """Per-day validation loss and factors of the eager module, from
    FactorVAE.loss_terms with dropout off: the dict of host tensors
    FusedTrainer.loss_many returns ("loss", "mse", "kl": (D,) float32,
    "n": (D,) int32, with return_factors also the four (D, K) factor
    arrays), and its oracle. days: (x_d (N_d,T,C), y_d) pairs; eps: optional
    per-day (N_d,) draws, None draws them with torch's generator unless
    sample=False, which uses zeros. A day without rows is NaN with n = 0."""
    import torch

    days = list(days)
    dev = next(model.parameters()).device
    K = model.factor_encoder.num_factors
    D = len(days)
    res = {k: torch.full((D,), NAN) for k in ("loss", "mse", "kl")}
    res["n"] = torch.tensor([int(x.shape[0]) for x, _ in days],
                            dtype=torch.int32)
    if return_factors:
        for k in FACTOR_KEYS:
            res[k] = torch.full((D, K), NAN)
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            for d, (x, y) in enumerate(days):
                n = int(x.shape[0])
                if n == 0:
                    continue
                if eps is not None:
                    e = torch.as_tensor(eps[d]).to(dev).float().reshape(n, 1)
                elif sample:
                    e = None
                else:
                    e = torch.zeros(n, 1, device=dev)
                t = model.loss_terms(
                    x.to(dev).float(),
                    torch.as_tensor(y).to(dev).float().reshape(n, 1), e)
                for k in res:
                    if k != "n":
                        res[k][d] = t[k].float().cpu()
    finally:
        model.train(was)
    return res


def evaluate_days_eager(model, days, on=("mu",), topk: int = 0) -> Dict:
    """Per-day metrics of the eager module: model.prediction_dist gives
    (mu, sigma); "score" is the stochastic sample mu + eps * sigma with
    eps from torch's generator. days: (x_d (N_d,T,C), y_d) pairs."""
    import torch

    on = check_columns(on)
    dev = next(model.parameters()).device
    was = model.training
    model.eval()
    preds, labels = [], []
    try:
        with torch.no_grad():
            for x, y in days:
                y = torch.as_tensor(y).reshape(-1).float().cpu().numpy()
                if x.shape[0] == 0:
                    cols = {c: np.zeros(0, np.float32) for c in COLUMNS}
                else:
                    mu, sigma = model.prediction_dist(x.to(dev).float())
                    cols = {"mu": mu.reshape(-1).cpu().numpy()}
                    if "score" in on:
                        score = mu + torch.randn_like(sigma) * sigma
                        cols["score"] = score.reshape(-1).cpu().numpy()
                preds.append([cols[c] for c in on])
                labels.append(y)
    finally:
        model.train(was)
    return evaluate_preds(preds, labels, on, topk)
