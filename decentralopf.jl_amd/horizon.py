"""Moving a window of the decentral OPF by k timesteps: the rule of dopf_roll_horizon (include/dopf.h) in NumPy.

``shift_window`` is the specification in executable form: the library's device path is tested against it, and ``Engine.roll``
uses it on a backend that has no dopf_roll_horizon of its own (getters -> shift_window -> a new context with the setters and
dopf_set_state). Not in the reference, which builds a new ADMM(...) per window (src/structures/admm.jl:23-62).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np


def _mat(a, rows: int, T: int) -> np.ndarray:
    return np.asarray(a, dtype=np.float64).reshape(rows, T)


def _persist(a: np.ndarray, k: int) -> np.ndarray:
    """new[:, t] = old[:, t + k] for t < T - k, behind it the old last column"""
    T = a.shape[-1]
    return np.concatenate([a[..., k:], np.repeat(a[..., T - 1:T], k, axis=-1)], axis=-1)


def _zeros(a: np.ndarray, k: int) -> np.ndarray:
    """new[:, t] = old[:, t + k] for t < T - k, behind it zeros"""
    return np.concatenate([a[..., k:], np.zeros(a.shape[:-1] + (k,))], axis=-1)


def shift_window(k: int, demand_tail, *, demand, P, D, C, E, lam, mu, rho, avg_U, avg_K, sto_emax,
                 used: Optional[dict] = None, line_rating=None) -> Dict[str, np.ndarray]:
    """The state of the window that starts k steps later, 1 <= k <= T - 1. Matrices in Julia shape (rows, T): demand (N, T),
    P (G, T), D / C / E (S, T), mu / rho / avg_U / avg_K (L, T); lam (T,); demand_tail (N, k); sto_emax (S,). E is what
    get_primal returned for the old window (it includes that window's initial levels).

    "Kept": the new value at t is the old one at t + k, for t < T - k. Behind it: demand = demand_tail; P = the old last column
    (persistence; the next x-update clamps it to the cap); D = C = 0; the duals and avg_U / avg_K = their old last column.
    e0[s] = min(max(E[s, k - 1], 0), max_level[s]): the level the old window reached where the new one starts.

    line_rating (L, T), the table of DOPF_F_LINE_RATING, moves like the duals: behind the kept part its old last column (a derating
    persists until the caller sets a new table).

    Returns demand, P, D, C, lam, mu, rho, avg_U, avg_K, e0 (and line_rating when given); with `used` (a dict with any of lam, mu, rho, avg_U, avg_K: what the
    last solve read) also a dict `used`, moved like the duals."""
    lam = np.asarray(lam, dtype=np.float64).reshape(-1)
    T = lam.size
    k = int(k)
    if not 1 <= k <= T - 1:
        raise ValueError(f"k = {k} outside [1, T - 1 = {T - 1}]")
    em = np.asarray(sto_emax, dtype=np.float64).reshape(-1)
    S = em.size
    demand = np.asarray(demand, dtype=np.float64)
    N = demand.size // T
    tail = np.asarray(demand_tail, dtype=np.float64).reshape(N, k)
    if not np.all(np.isfinite(tail)):
        raise ValueError("demand_tail holds a NaN or Inf")
    rows = lambda a: _mat(a, np.asarray(a).size // T, T)
    out = dict(
        demand=np.concatenate([_mat(demand, N, T)[:, k:], tail], axis=1),
        P=_persist(rows(P), k), D=_zeros(rows(D), k), C=_zeros(rows(C), k),
        lam=_persist(lam, k), mu=_persist(rows(mu), k), rho=_persist(rows(rho), k),
        avg_U=_persist(rows(avg_U), k), avg_K=_persist(rows(avg_K), k),
        e0=np.minimum(np.maximum(_mat(E, S, T)[:, k - 1], 0.0), em) + 0.0)
    if line_rating is not None:
        out["line_rating"] = _persist(rows(line_rating), k)
    if used is not None:
        out["used"] = {name: _persist(np.asarray(a, dtype=np.float64).reshape(-1) if name == "lam" else rows(a), k)
                       for name, a in used.items()}
    return out


def shift_coupled(k: int, P, *, budget: Optional[Tuple] = None) -> Dict[str, object]:
    """What couples a generator's timesteps, for the window that starts k steps later: the rule of dopf_roll_horizon_coupled
    (include/dopf.h) in NumPy, the specification the device is tested against. P (G, T): the rows of the old window.

    gen_prev = P[:, k - 1], the output of the step before the new window (the ramps' anchor). With budget = (e_min, e_max) (G values
    each; either may be None: 0 / inf) also gen_budget = (lo', hi'): what the k steps that leave the window delivered,
    spent[g] = ((P[g, 0] + P[g, 1]) + ...) + P[g, k - 1] — summed left to right from P[g, 0]; the order is part of the rule — comes off
    both bounds, floored at 0 (inf stays inf)."""
    P = np.asarray(P, dtype=np.float64)
    P = P.reshape(P.shape[0], -1) if P.ndim == 2 else P.reshape(1, -1)
    G, T = P.shape
    k = int(k)
    if not 1 <= k <= T - 1:
        raise ValueError(f"k = {k} outside [1, T - 1 = {T - 1}]")
    out: Dict[str, object] = dict(gen_prev=P[:, k - 1].copy())
    if budget is not None:
        lo, hi = budget
        lo = np.zeros(G) if lo is None else np.asarray(lo, dtype=np.float64).reshape(G)
        hi = np.full(G, np.inf) if hi is None else np.asarray(hi, dtype=np.float64).reshape(G)
        spent = np.cumsum(P[:, :k], axis=1)[:, -1]
        out["gen_budget"] = (np.maximum(0.0, lo - spent) + 0.0, np.maximum(0.0, hi - spent) + 0.0)
    return out
