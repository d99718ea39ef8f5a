"""The central reference: the whole multi-period DC-OPF as ONE LP (host side, SciPy/HiGHS).

Mirrors the reference's second script, src/opf_central_reference.jl:1-81 — there a JuMP model handed to Gurobi, here the
same LP handed to HiGHS (the LP solver that ships with SciPy; no licence):

    variables     P[g,t] in [0, max_generation], D[s,t], C[s,t] in [0, max_power], E[s,t] in [0, max_level],
                  U[l,t], K[l,t] >= 0                                                            (:21-31)
    injection     I[n,t] = sum of the node's P + D - C - demand                                  (:34-38)
    objective     sum mc P + sum mc (D + C)                                                      (:41-44)
    EB[t]         sum_n I[n,t] = 0                                                               (:47)
    FlowUpper     ptdf I + U = f_max,   FlowLower   K - ptdf I = f_max                           (:49-51)
    StorageBalance  E[s,t] = E[s,t-1] - D + C, E[s,0] = 0                                        (:53)
                  (here E[s,0] = initial_level[s] if given: DOPF_F_STO_INITIAL_LEVEL's target; 0 as in the reference by default;
                  E[s,T] in [lo[s], hi[s]] if a terminal band is given: DOPF_F_STO_TERMINAL_LEVEL's; [0, max_level] by default;
                  E[s,t] = E[s,t-1] - D / eta_d + eta_c C if efficiencies are given: DOPF_F_STO_EFFICIENCY's; lossless by default)
    outputs       objective, P, D, C, line utilisation ptdf I, system price lambda = dual(EB),
                  nodal price = lambda + sum_l (dual(FlowUpper) + dual(FlowLower))[l,t] ptdf[l,:]  (:57-81)

It is the parity target of the decentral ADMM ("converged objective within 1e-3 of opf_central_reference.jl") and, like in
the reference, NOT part of the hot path: a one-off host solve. The injections are explicit LP variables, so a flow row
has N non-zeros instead of one per unit (what makes the 118-node cases tractable); duals come back in the reference's
sign convention (d objective / d right-hand side).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from .network import Generator, Line, Node, PackedProblem, Storage, pack


@dataclass
class CentralResult:
    objective: float
    generation: np.ndarray          # (G, T)  value.(P)
    discharge: np.ndarray           # (S, T)  value.(D)
    charge: np.ndarray              # (S, T)  value.(C)
    level: np.ndarray               # (S, T)  value.(E)
    injection: np.ndarray           # (N, T)  value.(I)
    line_utilization: np.ndarray    # (L, T)  ptdf * I
    system_price: np.ndarray        # (T,)    dual.(EB)
    flow_upper_dual: np.ndarray     # (L, T)  dual.(FlowUpper)
    flow_lower_dual: np.ndarray     # (L, T)  dual.(FlowLower)
    nodal_price: np.ndarray         # (N, T)
    budget_window_dual: Optional[np.ndarray] = None     # (G, n_win) with gen_budget_windows: d objective / d right-hand side of the window rows


def _efficiencies(pp: PackedProblem, efficiency):
    """(eta_c, eta_d) as float64 (S,): the argument, else the packed case's, else all 1."""
    ec, ed = pp.efficiency() if efficiency is None else efficiency
    ec, ed = np.asarray(ec, dtype=np.float64).reshape(pp.S), np.asarray(ed, dtype=np.float64).reshape(pp.S)
    if np.any(~(ec > 0.0)) or np.any(ec > 1.0) or np.any(~(ed > 0.0)) or np.any(ed > 1.0):
        raise ValueError("storage efficiencies must lie in (0, 1]")
    return ec, ed


def solve_central_packed(pp: PackedProblem, *, duals: bool = True, initial_level=None, terminal_level=None,
                         availability=None, efficiency=None, line_rating=None, gen_ramp=None, gen_prev=None, gen_budget=None,
                         gen_min_output=None, gen_budget_windows=None) -> CentralResult:
    """The LP on a packed case (any size HiGHS can take; synthetic cases with 1e5 agents go through
    tests/central_lp.aggregate_* first). initial_level: (S,) level of each storage before the first timestep, the right-hand
    side of its storage-balance row at t = 0 (None: the packed case's sto_e0, else 0 as in the reference). terminal_level:
    (lo, hi), (S,) each, the bounds of the level after the last timestep E[:, T-1] (None: the packed case's band, else
    [0, max_level] as in the reference). availability: (profiles (K, T), profile_of (G,)), the upper bound of P[g,t] becomes
    gen_pmax[g] * profiles[profile_of[g], t] (gen_pmax for -1; None: the packed case's profiles, else gen_pmax as in the reference).
    efficiency: (eta_c, eta_d), (S,) each in (0, 1]: the storage-balance rows read E[t] - E[t-1] + D / eta_d - eta_c C = 0 (None:
    the packed case's efficiencies, else all 1 as in the reference). line_rating: (L, T), the right-hand sides of the two flow rows
    become rating[l,t] (None: the packed case's table, else f_max in every timestep as in the reference). gen_ramp: (up, down), (G,)
    each, inf = no limit: the rows -down[g] <= P[g,t] - P[g,t-1] <= up[g] for t >= 1 (None: the packed case's ramps, else none as in
    the reference); gen_prev: (G,) outputs of the step before the window, the same rows at t = 0 against them (None: no such rows). gen_budget:
    (e_min, e_max), (G,) each: the rows e_min[g] <= sum_t P[g,t] <= e_max[g], one per generator with an e_min above 0 and one per finite
    e_max (None: the packed case's budgets, else none as in the reference). gen_min_output: (G,) must-run floors: the lower bound of
    P[g,t] becomes min(p_min[g], its upper bound) — the floor follows an outage down (None: the packed case's floors, else 0 as in the
    reference). The parity target of dopf_set_generator_min_output. gen_budget_windows: (win_end (n_win,), e_min, e_max (G, n_win) each or
    None): one inequality pair per generator and window, e_min[g,j] <= sum_{win_end[j-1] <= t < win_end[j]} P[g,t] <= e_max[g,j] (a row
    per e_min above 0 and per finite e_max; None: the packed case's table, else none). The result's budget_window_dual[g,j] is then
    d objective / d right-hand side of that pair: negative where e_max binds, positive where e_min does, as
    _capi.central_solve_coupled's budget_dual — minus dopf_get_generator_budget_window_price at convergence. An infeasible table
    raises RuntimeError, as every infeasible case. The parity target of dopf_set_generator_energy_budget_windows."""
    from scipy import sparse
    from scipy.optimize import linprog
    if pp.has_quadratic_cost():
        raise ValueError("solve_central_packed: the central problem here is an LP; a case with Generator.quadratic_costs is a QP and "
                         "would be solved with the marginal costs alone")
    N, L, T, G, S = pp.N, pp.L, pp.T, pp.G, pp.S
    nP, nS, nI, nL = G * T, S * T, N * T, L * T
    oD, oC, oE, oI, oU, oK = nP, nP + nS, nP + 2 * nS, nP + 3 * nS, nP + 3 * nS + nI, nP + 3 * nS + nI + nL
    nv = oK + nL
    c = np.zeros(nv)
    c[:nP] = np.repeat(pp.gen_mc, T)
    c[oD:oD + nS] = np.repeat(pp.sto_mc, T)
    c[oC:oC + nS] = np.repeat(pp.sto_mc, T)
    lb = np.zeros(nv)
    ub = np.concatenate([np.repeat(pp.gen_pmax, T), np.repeat(pp.sto_pmax, T), np.repeat(pp.sto_pmax, T),
                         np.repeat(pp.sto_emax, T), np.full(nI, np.inf), np.full(2 * nL, np.inf)])
    lb[oI:oI + nI] = -np.inf
    if availability is None and pp.has_availability():
        availability = pp.availability()
    if availability is not None and G > 0:
        prof = np.asarray(availability[0], dtype=np.float64).reshape(-1, T)
        of = np.asarray(availability[1], dtype=np.int64).reshape(G)
        pm = np.asarray(pp.gen_pmax, dtype=np.float64)
        f = np.ones((G, T))
        f[of >= 0] = prof[of[of >= 0]]
        ub[:nP] = np.where((of >= 0)[:, None], pm[:, None] * f, pm[:, None]).reshape(-1)      # one multiply, as the kernels
    if gen_min_output is None and pp.has_min_output():
        gen_min_output = pp.min_output()
    if gen_min_output is None and getattr(pp, "gen_budget_min_output", None) is not None:
        gen_min_output = pp.gen_budget_min_output          # (floors on a budget context are the same lower bounds to the LP)
    if gen_min_output is not None and G > 0:
        lb = np.array(lb, dtype=np.float64)
        lb[:nP] = np.minimum(np.repeat(np.asarray(gen_min_output, dtype=np.float64).reshape(G), T), ub[:nP])
    tt = np.arange(T)
    rows, cols, vals, beq = [], [], [], []
    # I[n,t] - sum of the node's units = -demand[n,t]          rows n*T + t
    gi = np.repeat(np.asarray(pp.gen_node, dtype=np.int64), T) * T + np.tile(tt, G)
    si = np.repeat(np.asarray(pp.sto_node, dtype=np.int64), T) * T + np.tile(tt, S)
    rows += [gi, si, si, np.arange(nI)]
    cols += [np.arange(nP), oD + np.arange(nS), oC + np.arange(nS), oI + np.arange(nI)]
    vals += [-np.ones(nP), -np.ones(nS), np.ones(nS), np.ones(nI)]
    beq.append(-np.asarray(pp.demand, dtype=np.float64).reshape(N, T).reshape(-1))
    r0 = nI
    rEB = r0                                                   # EB[t]: sum_n I[n,t] = 0
    rows.append(r0 + np.tile(tt, N)); cols.append(oI + np.arange(nI)); vals.append(np.ones(nI))
    beq.append(np.zeros(T)); r0 += T
    k = np.arange(nS)                                          # E[t] - E[t-1] + al D - be C = 0   (t = 0: E[0] + al D - be C = e0)
    eta_c, eta_d = _efficiencies(pp, efficiency)               # (al = 1 / eta_d, be = eta_c; all 1: the reference's rows, bit for bit)
    rows += [r0 + k, r0 + k, r0 + k]; cols += [oE + k, oD + k, oC + k]
    vals += [np.ones(nS), np.repeat(1.0 / eta_d, T), -np.repeat(eta_c, T)]
    k1 = k[(k % T) > 0]
    rows.append(r0 + k1); cols.append(oE + k1 - 1); vals.append(-np.ones(k1.size))
    if initial_level is None:
        initial_level = pp.sto_e0
    rhs = np.zeros(nS)
    if initial_level is not None:
        rhs[::T] = np.asarray(initial_level, dtype=np.float64).reshape(S)
    beq.append(rhs); r0 += nS
    Aeq = sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(r0, nv))
    rUp = rLo = r0
    if L > 0:
        flow = sparse.kron(sparse.csr_matrix(np.asarray(pp.ptdf, dtype=np.float64)), sparse.identity(T, format="csr"), format="csr")
        eyeL = sparse.identity(nL, format="csr")
        z = lambda n_: sparse.csr_matrix((nL, n_))
        up = sparse.hstack([z(oI), flow, eyeL, z(nL)], format="csr")          # ptdf I + U = f_max      rows l*T + t
        lo = sparse.hstack([z(oI), -flow, z(nL), eyeL], format="csr")         # K - ptdf I = f_max
        rUp, rLo = r0, r0 + nL
        Aeq = sparse.vstack([Aeq, up, lo], format="csr")
        if line_rating is None:
            line_rating = pp.line_rating
        if line_rating is None:
            beq += [np.repeat(pp.f_max, T), np.repeat(pp.f_max, T)]
        else:
            cap = np.asarray(line_rating, dtype=np.float64).reshape(L, T).reshape(-1)
            beq += [cap, cap]
    if terminal_level is None and (pp.sto_end_lo is not None or pp.sto_end_hi is not None):
        terminal_level = pp.terminal_band()
    if terminal_level is not None and S > 0:
        lb, ub = np.array(lb, dtype=np.float64), np.array(ub, dtype=np.float64)
        last = oE + np.arange(S) * T + (T - 1)
        lb[last] = np.asarray(terminal_level[0], dtype=np.float64).reshape(S)
        ub[last] = np.asarray(terminal_level[1], dtype=np.float64).reshape(S)
    Aub = bub = None
    ur, uc, uv, bub = [], [], [], []
    if gen_ramp is None and pp.has_ramp():
        gen_ramp = pp.ramp()
    if (gen_ramp is not None or gen_prev is not None) and G > 0:
        up, down = (np.full(G, np.inf),) * 2 if gen_ramp is None else (np.asarray(r, dtype=np.float64).reshape(G) for r in gen_ramp)
        def ramp_rows(sign, limit):          # sign (P[g,t] - P[g,t-1]) <= limit[g], the generators with a finite limit; t = 0: against gen_prev
            nonlocal Aub
            for g in np.flatnonzero(np.isfinite(limit)):
                for t in range(0 if gen_prev is not None else 1, T):
                    r = len(bub)
                    ur.append(r); uc.append(g * T + t); uv.append(sign)
                    if t > 0:
                        ur.append(r); uc.append(g * T + t - 1); uv.append(-sign)
                    bub.append(limit[g] + (sign * float(np.asarray(gen_prev, dtype=np.float64).reshape(G)[g]) if t == 0 else 0.0))
        ramp_rows(1.0, up)
        ramp_rows(-1.0, down)
    if gen_budget is None and pp.has_budget():
        gen_budget = pp.budget()
    if gen_budget is not None and G > 0:
        e_min = np.zeros(G) if gen_budget[0] is None else np.asarray(gen_budget[0], dtype=np.float64).reshape(G)
        e_max = np.full(G, np.inf) if gen_budget[1] is None else np.asarray(gen_budget[1], dtype=np.float64).reshape(G)
        for sign, bound, rowsof in ((1.0, e_max, np.flatnonzero(np.isfinite(e_max))), (-1.0, e_min, np.flatnonzero(e_min > 0.0))):
            for g in rowsof:          # sign sum_t P[g,t] <= sign bound[g]
                r = len(bub)
                ur += [r] * T; uc += list(range(g * T, g * T + T)); uv += [sign] * T
                bub.append(sign * bound[g])
    if gen_budget_windows is None and pp.has_budget_windows():
        gen_budget_windows = pp.budget_windows()
    win_rows = []          # (row of A_ub, g, j, sign)
    if gen_budget_windows is not None and G > 0:
        ends = np.asarray(gen_budget_windows[0], dtype=np.int64).reshape(-1)
        nw = ends.size
        if nw < 1 or ends[-1] != T or np.any(np.diff(np.concatenate([[0], ends])) <= 0):
            raise ValueError(f"gen_budget_windows: the ends {ends.tolist()} are not strictly increasing from above 0 up to T = {T}")
        w_min = np.zeros((G, nw)) if gen_budget_windows[1] is None else np.asarray(gen_budget_windows[1], dtype=np.float64).reshape(G, nw)
        w_max = np.full((G, nw), np.inf) if gen_budget_windows[2] is None else np.asarray(gen_budget_windows[2], dtype=np.float64).reshape(G, nw)
        for sign, bound, wanted in ((1.0, w_max, np.isfinite(w_max)), (-1.0, w_min, w_min > 0.0)):
            for g, j in zip(*np.nonzero(wanted)):          # sign sum_{t in window j} P[g,t] <= sign bound[g,j]
                t0, t1 = (0 if j == 0 else int(ends[j - 1])), int(ends[j])
                r = len(bub)
                ur += [r] * (t1 - t0); uc += list(range(g * T + t0, g * T + t1)); uv += [sign] * (t1 - t0)
                bub.append(sign * bound[g, j])
                win_rows.append((r, g, j, sign))
    if bub:
        Aub = sparse.csr_matrix((uv, (ur, uc)), shape=(len(bub), nv))
        bub = np.asarray(bub)
    res = linprog(c, A_ub=Aub, b_ub=bub if Aub is not None else None, A_eq=Aeq, b_eq=np.concatenate(beq),
                  bounds=np.stack([lb, ub], axis=1), method="highs")
    if res.status != 0:
        raise RuntimeError(f"central LP: {res.message}")
    x = res.x
    inj = x[oI:oI + nI].reshape(N, T)
    lam = np.zeros(T)
    fu = np.zeros((L, T))
    fl = np.zeros((L, T))
    if duals:
        m = res.eqlin.marginals
        lam = m[rEB:rEB + T].copy()
        if L > 0:
            fu = m[rUp:rUp + nL].reshape(L, T)
            fl = m[rLo:rLo + nL].reshape(L, T)
    ptdf = np.asarray(pp.ptdf, dtype=np.float64).reshape(L, N)
    nodal = lam[None, :] + ptdf.T @ (fu + fl) if L > 0 else np.tile(lam, (N, 1))      # opf_central_reference.jl:71-79
    wdual = None
    if gen_budget_windows is not None and G > 0:
        wdual = np.zeros((G, nw))
        if duals:
            for r, g, j, sign in win_rows:          # (a <= row's marginal is d objective / d its right-hand side, sign x the bound)
                wdual[g, j] += sign * res.ineqlin.marginals[r]
    return CentralResult(budget_window_dual=wdual, objective=float(res.fun), generation=x[:nP].reshape(G, T), discharge=x[oD:oD + nS].reshape(S, T),
                         charge=x[oC:oC + nS].reshape(S, T), level=x[oE:oE + nS].reshape(S, T), injection=inj,
                         line_utilization=ptdf @ inj if L > 0 else np.zeros((0, T)), system_price=lam,
                         flow_upper_dual=fu, flow_lower_dual=fl, nodal_price=nodal)


def central_reference(nodes: Sequence[Node], generators: Sequence[Generator], storages: Sequence[Storage],
                      lines: Sequence[Line], *, verbose: bool = False, initial_level=None,
                      terminal_level=None, efficiency=None) -> CentralResult:
    """src/opf_central_reference.jl for a case given as the reference's element vectors; `verbose` prints what the
    script prints (:60-81). initial_level: (S,) storage levels before the first timestep (None: Storage.initial_level).
    terminal_level: (lo, hi) bounds of the level after the last timestep (None: Storage.terminal_level_min / _max).
    efficiency: (eta_c, eta_d) (None: Storage.charge_efficiency / discharge_efficiency)."""
    r = solve_central_packed(pack(nodes, generators, storages, lines), initial_level=initial_level,
                             terminal_level=terminal_level, efficiency=efficiency)
    if verbose:
        print(f"Objective value: {r.objective}\n")
        print(f"Generator results:\n{r.generation}\n")
        print(f"Discharge results:\n{r.discharge}\n")
        print(f"Charge results:\n{r.charge}\n")
        print(f"Line utilization:\n{r.line_utilization}\n")
        print(f"System price:\n{r.system_price}\n")
        print(f"Nodal price:\n{r.nodal_price}\n")
    return r


def central_reference_on_device(nodes: Sequence[Node], generators: Sequence[Generator], storages: Sequence[Storage],
                                lines: Sequence[Line], *, tol: float = 1e-9, max_iters: int = 200000, device: int = -1,
                                initial_level=None, terminal_level=None, efficiency=None, lossy: bool = False) -> CentralResult:
    """The same LP solved on the GPU by libdopf_hip (dopf_central_solve / dopf_central_solve_ex / dopf_central_solve_lossy:
    first-order primal-dual method, csrc/kernels_central.hip) — for cases beyond a host LP solver, and as a cross-check that shares
    no code with HiGHS. The elements' initial levels, terminal bands and availability series are part of the LP, as in
    central_reference; initial_level / terminal_level override the storages' own, as there. Without lossy=True the device LP is
    lossless: efficiencies other than 1 (the argument's, or the storages' own) raise ValueError. With lossy=True they (the
    argument's, else the storages' own) are part of the LP (dopf_central_solve_lossy), as in central_reference. Any horizon is taken,
    beyond 512 timesteps too; no flag is needed for it."""
    from . import _capi
    pp = pack(nodes, generators, storages, lines)
    if pp.has_quadratic_cost():
        raise ValueError("central_reference_on_device: the device LP (dopf_central_solve, _ex, _lossy) takes no quadratic generator "
                         "costs and would solve with the marginal costs alone")
    if pp.has_min_output():
        raise ValueError("central_reference_on_device: the device LP (dopf_central_solve, _ex, _lossy) takes no generator minimum "
                         "output and would let every generator go down to 0; use central_reference for a case with Generator.min_generation")
    if pp.has_ramp():
        raise ValueError("central_reference_on_device: the device LP (dopf_central_solve, _ex, _lossy) takes no generator ramp limits "
                         "and would let every generator move freely; use central_reference_coupled_on_device, or central_reference, "
                         "for a case with Generator.ramp_up / ramp_down")
    if pp.has_budget():
        raise ValueError("central_reference_on_device: the device LP (dopf_central_solve, _ex, _lossy) takes no generator energy budgets "
                         "and would bound no generator's sum over the window; use central_reference for a case with Generator.energy_min / energy_max")
    if pp.line_rating is not None:
        raise ValueError("central_reference_on_device: the device LP (dopf_central_solve, _ex, _lossy) takes no line ratings and would "
                         "solve with max_capacity in every timestep; use central_reference for a case with Line.rating")
    ec, ed = _efficiencies(pp, efficiency)
    if not lossy and (np.any(ec != 1.0) or np.any(ed != 1.0)):
        raise ValueError("central_reference_on_device: the device LP (dopf_central_solve_ex) has no storage efficiencies; "
                         "pass lossy=True (dopf_central_solve_lossy) or use central_reference for a case with charge / discharge "
                         "efficiencies other than 1")
    kw = pp.engine_kwargs()
    kw.pop("sto_eta", None)
    if lossy:
        kw["sto_eta"] = (ec, ed)
    if initial_level is not None:
        kw["sto_e0"] = np.asarray(initial_level, dtype=np.float64).reshape(pp.S)
    if terminal_level is not None:
        kw["sto_end_lo"] = np.asarray(terminal_level[0], dtype=np.float64).reshape(pp.S)
        kw["sto_end_hi"] = np.asarray(terminal_level[1], dtype=np.float64).reshape(pp.S)
    r = _capi.central_solve(_capi.hip_api(), tol=tol, max_iters=max_iters, params=_capi.default_params(device=device), **kw)
    if not r["converged"]:
        raise RuntimeError(f"central LP on the device: gap {r['gap']:.2e} after {r['iterations']} iterations (infeasible case?)")
    inj = -np.asarray(pp.demand, dtype=np.float64).copy()
    np.add.at(inj, pp.gen_node, r["P"])
    np.add.at(inj, pp.sto_node, r["D"] - r["C"])
    return CentralResult(objective=r["objective"], generation=r["P"], discharge=r["D"], charge=r["C"], level=r["E"], injection=inj,
                         line_utilization=r["line_utilization"], system_price=r["system_price"], flow_upper_dual=r["flow_upper_dual"],
                         flow_lower_dual=r["flow_lower_dual"], nodal_price=r["nodal_price"])


def central_reference_coupled_on_device(nodes: Sequence[Node], generators: Sequence[Generator], storages: Sequence[Storage],
                                        lines: Sequence[Line], *, tol: float = 1e-9, max_iters: int = 200000, device: int = -1,
                                        initial_level=None, terminal_level=None, efficiency=None, gen_ramp=None, gen_prev=None,
                                        gen_budget=None, line_rating=None, duals: bool = False):
    """central_reference_on_device for a case whose elements carry ramp limits (Generator.ramp_up / ramp_down), energy budgets
    (Generator.energy_min / energy_max) or line ratings (Line.rating): the LP central_reference solves on the host, solved on the GPU
    by dopf_central_solve_coupled (csrc/kernels_central.hip, kc_gen_rows). The storages' efficiencies are always part of it. gen_ramp =
    (up, down), gen_budget = (e_min, e_max) and line_rating (L, T) override the elements' own; gen_prev (G,) are the outputs of the step
    before the window, the anchor of the ramp rows at t = 0 (None: no anchor — the elements carry none). Quadratic costs are refused:
    the device solve is an LP. Returns a CentralResult; with duals=True a pair of it and dict(ramp_dual (G, T), budget_dual (G,)),
    d objective / d right-hand side of the ramp and budget rows (budget_dual: minus the water value of a capped generator). Any horizon
    is taken, beyond 512 timesteps too (kc_gen_rows_long, kc_sto_long); no flag is needed for it."""
    from . import _capi
    pp = pack(nodes, generators, storages, lines)
    if pp.has_quadratic_cost():
        raise ValueError("central_reference_coupled_on_device: the device LP (dopf_central_solve_coupled) takes no quadratic generator "
                         "costs and would solve with the marginal costs alone")
    if pp.has_min_output():
        raise ValueError("central_reference_coupled_on_device: the device LP (dopf_central_solve_coupled) takes no generator minimum "
                         "output and would let every generator go down to 0; use central_reference for a case with Generator.min_generation")
    kw = pp.engine_kwargs()
    kw["sto_eta"] = _efficiencies(pp, efficiency)
    if initial_level is not None:
        kw["sto_e0"] = np.asarray(initial_level, dtype=np.float64).reshape(pp.S)
    if terminal_level is not None:
        kw["sto_end_lo"] = np.asarray(terminal_level[0], dtype=np.float64).reshape(pp.S)
        kw["sto_end_hi"] = np.asarray(terminal_level[1], dtype=np.float64).reshape(pp.S)
    for key, val in (("gen_ramp", gen_ramp), ("gen_prev", gen_prev), ("gen_budget", gen_budget), ("line_rating", line_rating)):
        if val is not None:
            kw[key] = val
    r = _capi.central_solve_coupled(_capi.hip_api(), tol=tol, max_iters=max_iters, params=_capi.default_params(device=device), **kw)
    if not r["converged"]:
        raise RuntimeError(f"central LP on the device: gap {r['gap']:.2e} after {r['iterations']} iterations (infeasible case?)")
    inj = -np.asarray(pp.demand, dtype=np.float64).copy()
    np.add.at(inj, pp.gen_node, r["P"])
    np.add.at(inj, pp.sto_node, r["D"] - r["C"])
    out = CentralResult(objective=r["objective"], generation=r["P"], discharge=r["D"], charge=r["C"], level=r["E"], injection=inj,
                        line_utilization=r["line_utilization"], system_price=r["system_price"], flow_upper_dual=r["flow_upper_dual"],
                        flow_lower_dual=r["flow_lower_dual"], nodal_price=r["nodal_price"])
    return (out, dict(ramp_dual=r["ramp_dual"], budget_dual=r["budget_dual"])) if duals else out
