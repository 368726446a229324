"""The factor risk model the prior decoder implies, in plain torch.

For one trading day the decoder under the prior gives the covariance

    Sigma = B diag(sz^2) B^T + diag(s2)

with B = beta (N, K), sz = the prior sigma after its zero clamp (K,) and
s2 = alpha_sigma^2 + 1e-6 (N,) — FactorVAE.risk_model(x) returns these
components, and Sigma's diagonal is prediction_dist's sigma^2. The
functions here work on such a component dict in the dtype they are given
(float64 for the tests' oracle) and are the definition the HIP kernels
risk_seg / risk_solve_seg (ops/hip/risk.hip) follow;
FusedTrainer.risk_many is the batched device route, risk_days_eager its
eager counterpart with the same return layout.
"""

from __future__ import annotations

from typing import Dict, Sequence

import torch

NAN = float("nan")
STAT_KEYS = ("mean", "mean_factor", "var_factor", "var_specific", "vol")
SOLVE_KEYS = ("minvar", "mv")
COMPONENT_KEYS = ("mu", "beta", "specific_var", "factor_mu", "factor_sigma")


def components_to(comp: Dict, dtype=None, device=None) -> Dict:
    """The component dict with every tensor cast / moved."""
    return {k: v.to(dtype=dtype, device=device) for k, v in comp.items()}


def check_solve(solve) -> tuple:
    solve = tuple(solve)
    for s in solve:
        if s not in SOLVE_KEYS:
            raise ValueError(f"solve entries must be among {SOLVE_KEYS}, "
                             f"got {s!r}")
    return solve


def portfolio_risk(comp: Dict, w: torch.Tensor) -> Dict:
    """Risk decomposition of the portfolio w (N,), used as given (no
    normalisation): mean = w.mu, exposure f = B^T w (K,), mean_factor =
    f.factor_mu, factor_var_k = f_k^2 sz_k^2 (K,), var_factor = their sum,
    var_specific = sum w_i^2 s2_i, vol = sqrt(var_factor + var_specific)
    and mcr (N,) = (B (sz^2 f) + w s2) / vol, the marginal contribution to
    risk: sum_i w_i mcr_i = vol. mcr is NaN when vol == 0."""
    B, s2 = comp["beta"], comp["specific_var"]
    w = w.reshape(-1).to(B.dtype)
    sz2 = comp["factor_sigma"] ** 2
    f = B.t() @ w
    factor_var = f * f * sz2
    var_factor = factor_var.sum()
    var_specific = (w * w * s2).sum()
    vol = torch.sqrt(var_factor + var_specific)
    num = B @ (sz2 * f) + w * s2
    mcr = torch.where(vol == 0, torch.full_like(num, NAN), num / vol)
    return {"mean": (w * comp["mu"]).sum(), "exposure": f,
            "mean_factor": (f * comp["factor_mu"]).sum(),
            "factor_var": factor_var, "var_factor": var_factor,
            "var_specific": var_specific, "vol": vol, "mcr": mcr}


def dense_cov(comp: Dict) -> torch.Tensor:
    """Sigma as an (N, N) matrix. For tests and small exports only."""
    B = comp["beta"]
    return (B * comp["factor_sigma"] ** 2) @ B.t() + torch.diag(
        comp["specific_var"])


def solve_cov(comp: Dict, b: torch.Tensor) -> torch.Tensor:
    """x = Sigma^-1 b for b (N,) or (N, R) through the factor structure,
    never the dense matrix: C = diag(1/s) B diag(sz), M = I_K + C^T C (SPD,
    eigenvalues >= 1), Cholesky of M, u = M^-1 C^T (b/s),
    x = b/s2 - (C u)/s. (The diag(1/sz^2) + B^T diag(1/s2) B form is
    hopeless in float32 once a factor sigma sits at its 1e-6 clamp.)"""
    B, s2 = comp["beta"], comp["specific_var"]
    vec = b.dim() == 1
    b2 = b.reshape(B.shape[0], -1).to(B.dtype)
    s = torch.sqrt(s2).unsqueeze(1)
    C = B * comp["factor_sigma"] / s
    M = torch.eye(B.shape[1], dtype=B.dtype, device=B.device) + C.t() @ C
    L = torch.linalg.cholesky(M)
    u = torch.cholesky_solve(C.t() @ (b2 / s), L)
    x = b2 / s2.unsqueeze(1) - (C @ u) / s
    return x.reshape(-1) if vec else x


def minvar_weights(comp: Dict) -> torch.Tensor:
    """Fully invested minimum-variance weights Sigma^-1 1 / (1^T Sigma^-1 1)."""
    x = solve_cov(comp, torch.ones_like(comp["specific_var"]))
    return x / x.sum()


def mv_weights(comp: Dict) -> torch.Tensor:
    """Mean-variance direction Sigma^-1 mu scaled to gross exposure 1
    (long-short, L1 norm 1); all-zero when the norm is 0."""
    x = solve_cov(comp, comp["mu"])
    norm = x.abs().sum()
    return torch.where(norm == 0, torch.zeros_like(x), x / norm)


def empty_result(lens: Sequence[int], K: int, solve=(),
                 return_components: bool = False) -> Dict:
    """The return layout of risk_many / risk_days_eager before any day is
    filled in: NaN per-day values, per-stock entries None."""
    D = len(lens)
    res = {"n": torch.tensor(list(lens), dtype=torch.int32)}
    for k in STAT_KEYS:
        res[k] = torch.full((D,), NAN)
    res["exposure"] = torch.full((D, K), NAN)
    res["factor_var"] = torch.full((D, K), NAN)
    res["mcr"] = [torch.empty(0)] * D
    for s in solve:
        res[s] = [torch.empty(0)] * D
    if solve:
        res["solve_info"] = torch.zeros(D, dtype=torch.int32)
    if return_components:
        res["mu"] = [torch.empty(0)] * D
        res["specific_var"] = [torch.empty(0)] * D
        res["beta"] = [torch.empty(0, K)] * D
        res["factor_mu"] = torch.full((D, K), NAN)
        res["factor_sigma"] = torch.full((D, K), NAN)
    return res


def check_weights(weights, lens: Sequence[int]):
    """weights as a list with one (N_d,) tensor per day, or None."""
    if weights is None:
        return None
    weights = list(weights)
    if len(weights) != len(lens):
        raise ValueError(f"weights must hold one (N_d,) tensor per day: got "
                         f"{len(weights)} for {len(lens)} days")
    for i, (wt, n) in enumerate(zip(weights, lens)):
        if wt.numel() != n:
            raise ValueError(f"day {i}: weights must have {n} entries, got "
                             f"{wt.numel()}")
    return weights


def risk_days_eager(model, days, weights=None, solve=(),
                    return_components: bool = False) -> Dict:
    """FusedTrainer.risk_many on the eager module, day by day, and its
    oracle: days is a list of x_d (N_d, T, C); weights None (equal weight
    1/N_d) or one (N_d,) tensor per day, used as given; solve a subset of
    ("minvar", "mv"). Returns host float32 tensors in day order: "n" (D,)
    int32; "mean", "mean_factor", "var_factor", "var_specific", "vol" (D,);
    "exposure", "factor_var" (D, K); "mcr" a list of (N_d,); with solve the
    weight lists "minvar" / "mv" and "solve_info" (D,) int32 (1 where the
    solution is not finite); with return_components the lists "mu",
    "specific_var" (N_d,), "beta" (N_d, K) and "factor_mu", "factor_sigma"
    (D, K). A day without rows has n = 0, NaN per-day values and empty
    per-stock tensors."""
    days = list(days)
    solve = check_solve(solve)
    lens = [int(x.shape[0]) for x in days]
    weights = check_weights(weights, lens)
    dev = next(model.parameters()).device
    K = model.factor_predictor.num_factor
    res = empty_result(lens, K, solve, return_components)
    was = model.training
    model.eval()
    try:
        for d, x in enumerate(days):
            n = lens[d]
            if n == 0:
                continue
            comp = model.risk_model(x.to(dev).float())
            if weights is None:
                w = torch.full((n,), 1.0 / n, device=dev)
            else:
                w = torch.as_tensor(weights[d]).to(dev).float().reshape(n)
            r = portfolio_risk(comp, w)
            for k in STAT_KEYS:
                res[k][d] = r[k].float().cpu()
            res["exposure"][d] = r["exposure"].float().cpu()
            res["factor_var"][d] = r["factor_var"].float().cpu()
            res["mcr"][d] = r["mcr"].float().cpu()
            for s in solve:
                wt = (minvar_weights if s == "minvar" else mv_weights)(comp)
                res[s][d] = wt.float().cpu()
                if not bool(torch.isfinite(wt).all()):
                    res["solve_info"][d] = 1
            if return_components:
                for k in ("mu", "specific_var", "beta"):
                    res[k][d] = comp[k].float().cpu()
                res["factor_mu"][d] = comp["factor_mu"].float().cpu()
                res["factor_sigma"][d] = comp["factor_sigma"].float().cpu()
    finally:
        model.train(was)
    return res
