"""Helpers of the storage-efficiency tests (DOPF_F_STO_EFFICIENCY), CPU and GPU: an optimality certificate of the
copper-plate storage QP with charge / discharge efficiencies in NumPy, an independent solve of that QP (SciPy) for the
certificate's own test, and the draws of efficiencies, initial levels and terminal bands the GPU tests share."""
import numpy as np


def levels_eff(e0, eta_c, eta_d, D, C):
    """E = e0 + cumsum(eta_c C - D / eta_d), (S, T)."""
    return np.asarray(e0)[:, None] + np.cumsum(np.asarray(eta_c)[:, None] * C - D / np.asarray(eta_d)[:, None], axis=1)


def reachable_eff(pp, e0, eta_c, eta_d):
    """End levels reachable from e0: [max(0, e0 - T pmax / eta_d), min(emax, e0 + T eta_c pmax)]."""
    return (np.maximum(0.0, e0 - pp.T * pp.sto_pmax / eta_d), np.minimum(pp.sto_emax, e0 + pp.T * eta_c * pp.sto_pmax))


def draw_eta(S, rng):
    """eta_c, eta_d uniform in [0.6, 1]; every fourth storage (1, 1), one (0.6, 1), one (1, 0.6)."""
    ec, ed = rng.uniform(0.6, 1.0, S), rng.uniform(0.6, 1.0, S)
    ec[::4] = 1.0
    ed[::4] = 1.0
    if S > 1:
        ec[1], ed[1] = 0.6, 1.0
    if S > 2:
        ec[2], ed[2] = 1.0, 0.6
    return ec, ed


def draw_band_eff(pp, e0, eta_c, eta_d, kind, rng):
    """helpers.draw_band's kinds default / eq / cyclic / mix over the efficiency-aware reachable range (mix: an equality target,
    lo = hi = e0, the highest reachable level as an equality, a band around the target, the default, in turn)."""
    rlo, rhi = reachable_eff(pp, e0, eta_c, eta_d)
    x = rlo + rng.uniform(0.0, 1.0, pp.S) * (rhi - rlo)
    if kind == "mix":
        k = np.arange(pp.S) % 5
        mid = 0.5 * (rlo + rhi)
        lo = np.select([k == 0, k == 1, k == 2, k == 3], [x, e0, rhi, np.minimum(x, mid)], 0.0)
        hi = np.select([k == 0, k == 1, k == 2, k == 3], [x, e0, rhi, np.maximum(x, mid)], pp.sto_emax)
        return lo, hi
    return {"default": (np.zeros(pp.S), pp.sto_emax.copy()), "eq": (x, x.copy()), "cyclic": (e0.copy(), e0.copy())}[kind]


def psi_at(pp, lam, mu, rho, inj, flow, avg_U, avg_K, gamma, w_flow, dlt):
    """Psi_{n,t}(dlt) of DESIGN.md section 3 for every storage (at its node n) and timestep, in NumPy from the closed forms: the
    derivative of everything that couples an agent to the network with respect to a change dlt (S, T) of its net injection,
        Psi = pi + gamma (s + dlt) + sum_l w2 h_l [(f + h_l dlt + U_l - F_l) - (K_l - f - h_l dlt - F_l)],
        U_l = max(0, (gamma a_l - w2 (f_l + h_l dlt - F_l)) / (w2 + gamma)),  K_l = max(0, (gamma b_l + w2 (f_l + h_l dlt + F_l)) / (w2 + gamma)),
    pi = lam_t + sum_l h_l (mu - rho), h_l = ptdf[l, n], w2 = 2 w_flow, s_t = sum_n inj[n, t], f = flow, a = avg_U, b = avg_K:
    the consensus state (get_consensus) and the duals (get_duals) the solve read. Without lines: lam + gamma (s + dlt)."""
    w2 = 2.0 * w_flow
    h = np.asarray(pp.ptdf, dtype=np.float64).reshape(pp.L, pp.N)[:, np.asarray(pp.sto_node, dtype=np.int64)]      # (L, S)
    psi = lam[None, :] + gamma * (inj.sum(axis=0)[None, :] + dlt)
    if pp.L > 0:
        psi = psi + h.T @ (mu - rho)
        fl = flow[None, :, :] + h.T[:, :, None] * dlt[:, None, :]                    # (S, L, T)
        F = np.asarray(pp.f_max, dtype=np.float64)[None, :, None]
        U = np.maximum(0.0, (gamma * avg_U[None] - w2 * (fl - F)) / (w2 + gamma))
        K = np.maximum(0.0, (gamma * avg_K[None] + w2 * (fl + F)) / (w2 + gamma))
        psi = psi + w2 * np.einsum("ls,slt->st", h, (fl + U - F) - (K - fl - F))
    return psi


def theta_of(pp, before, duals, D, C, gamma, w_flow):
    """The linear coefficient the certificate takes: Psi at the solution's injection change minus gamma (D - C), so that
    theta + gamma q is the gradient of the coupling terms at the solution (the QP is convex: KKT there is optimality).
    before: helpers.state_of before the iteration; duals: (lam, mu, rho) the solve read. Copper plate: lam + gamma (s - q0)."""
    q = D - C
    dlt = q - (before["D"] - before["C"])
    # (the flows the solve reads are ptdf . injection: what get_consensus reports once an iteration has run, and what the solve
    # derives in the zero state, where the getter still reports 0)
    flow = np.asarray(pp.ptdf, dtype=np.float64).reshape(pp.L, pp.N) @ before["inj"]
    psi = psi_at(pp, duals[0], duals[1], duals[2], before["inj"], flow, before["avg_U"], before["avg_K"], gamma, w_flow, dlt)
    return psi - gamma * q


def storage_kkt_violation_eff(pp, D0, C0, D, C, theta, gamma, e0, lo_end, hi_end, eta_c, eta_d, w=1.0, tol=1e-7):
    """helpers.storage_kkt_violation_band with efficiencies. The step problem is J_t(D, C) - nu_t (be C - al D) with al = 1 / eta_d,
    be = eta_c, so with gD = mc + theta + gamma q + w (D - D0), gC = mc - theta - gamma q + w (C - C0), q = D - C:
        gD + al nu_t  >= 0 at D = 0, = 0 inside, <= 0 at D = pmax;    gC - be nu_t likewise;
    nu_{t+1} - nu_t >= 0 where the level E_t = e0 + cumsum(be C - al D) sits on its upper bound, <= 0 on its lower bound, = 0
    inside, nu past the horizon 0; the bounds of E_{T-1} are [lo_end, hi_end]. The feasible nu_t form an interval, propagated
    backwards exactly. theta[s, t] = price_t + gamma (s_t - (D0 - C0)) on a copper plate, theta_of(...) in general. Returns the largest amount by which an
    interval is empty (0 = optimal within tol)."""
    mc = pp.sto_mc[:, None]
    pm = pp.sto_pmax[:, None]
    em = pp.sto_emax
    al, be = 1.0 / np.asarray(eta_d)[:, None], np.asarray(eta_c)[:, None]
    E = levels_eff(e0, eta_c, eta_d, D, C)
    q = D - C
    gD = mc + theta + gamma * q + w * (D - D0)
    gC = mc - theta - gamma * q + w * (C - C0)
    inf = np.inf
    nD, nC = -gD / al, gC / be          # the price at which D resp. C is stationary
    lo = np.where(D <= tol, nD, np.where(D >= pm - tol, -inf, nD))
    hi = np.where(D <= tol, inf, np.where(D >= pm - tol, nD, nD))
    lo = np.maximum(lo, np.where(C <= tol, -inf, np.where(C >= pm - tol, nC, nC)))
    hi = np.minimum(hi, np.where(C <= tol, nC, np.where(C >= pm - tol, inf, nC)))
    degenerate = pm <= tol
    lo = np.where(degenerate, -inf, lo)
    hi = np.where(degenerate, inf, hi)
    T = D.shape[1]
    flo = np.zeros(D.shape[0])
    fhi = np.zeros(D.shape[0])
    worst = 0.0
    for t in range(T - 1, -1, -1):
        blo, bhi = (lo_end, hi_end) if t == T - 1 else (np.zeros_like(em), em)
        at_hi = E[:, t] >= bhi - tol
        at_lo = E[:, t] <= blo + tol
        both = at_hi & at_lo          # a band of one point: any jump allowed
        nlo = np.where(both, -inf, np.where(at_hi, -inf, flo))      # E on its upper bound: nu_t <= nu_{t+1}
        nhi = np.where(both, inf, np.where(at_lo, inf, fhi))        # E on its lower bound: nu_t >= nu_{t+1}
        nlo = np.where(at_lo & ~both, flo, nlo)
        nhi = np.where(at_hi & ~both, fhi, nhi)
        flo = np.maximum(nlo, lo[:, t])
        fhi = np.minimum(nhi, hi[:, t])
        worst = max(worst, float(np.max(flo - fhi)))
        with np.errstate(invalid="ignore"):     # (an unbounded interval: -inf + inf, never used — `bad` is False there)
            mid = 0.5 * (flo + fhi)
        bad = flo > fhi
        flo = np.where(bad, mid, flo)
        fhi = np.where(bad, mid, fhi)
    return max(worst, 0.0)


def solve_storage_qp(mc, pm, em, e0, lo_end, hi_end, eta_c, eta_d, D0, C0, theta, gamma, w=1.0):
    """One storage's copper-plate step QP solved without any of the library's code: SLSQP on
        sum_t mc (D + C) + theta_t (D - C) + gamma/2 (D - C)^2 + w/2 ((D - D0)^2 + (C - C0)^2)
    over 0 <= D, C <= pm, 0 <= e0 + cumsum(eta_c C - D / eta_d) <= em (last level in [lo_end, hi_end]), then polished: the active
    set SLSQP ends on (variables and levels within 1e-6 of a bound) is imposed as equalities and the KKT system of that
    equality-constrained QP is solved exactly. Returns (D, C)."""
    from scipy.optimize import minimize
    T = len(theta)
    al, be = 1.0 / eta_d, eta_c
    Lm = np.tril(np.ones((T, T)))
    A = np.hstack([-al * Lm, be * Lm])                      # levels = e0 + A x, x = (D, C)
    H = np.zeros((2 * T, 2 * T))
    for t in range(T):
        H[t, t] = H[T + t, T + t] = w + gamma
        H[t, T + t] = H[T + t, t] = -gamma
    g = np.concatenate([mc + theta - w * D0, mc - theta - w * C0])
    f = lambda x: 0.5 * x @ H @ x + g @ x
    blo = np.zeros(T)
    bhi = np.full(T, float(em))
    blo[-1], bhi[-1] = lo_end, hi_end
    cons = [dict(type="ineq", fun=lambda x: e0 + A @ x - blo, jac=lambda x: A),
            dict(type="ineq", fun=lambda x: bhi - e0 - A @ x, jac=lambda x: -A)]
    r = minimize(f, np.zeros(2 * T), jac=lambda x: H @ x + g, bounds=[(0.0, pm)] * (2 * T), constraints=cons, method="SLSQP",
                 options=dict(ftol=1e-15, maxiter=500))
    x = np.clip(r.x, 0.0, pm)
    lev = e0 + A @ x
    rows, rhs = [], []
    for i in range(2 * T):
        if x[i] <= 1e-6 or x[i] >= pm - 1e-6:
            e = np.zeros(2 * T)
            e[i] = 1.0
            rows.append(e)
            rhs.append(0.0 if x[i] <= 1e-6 else pm)
    for t in range(T):
        if lev[t] <= blo[t] + 1e-6 or lev[t] >= bhi[t] - 1e-6:
            rows.append(A[t])
            rhs.append((blo[t] if lev[t] <= blo[t] + 1e-6 else bhi[t]) - e0)
    if rows:
        Ae, be_ = np.asarray(rows), np.asarray(rhs)
        K = np.block([[H, Ae.T], [Ae, np.zeros((len(rows), len(rows)))]])
        sol = np.linalg.lstsq(K, np.concatenate([-g, be_]), rcond=None)[0]
        x = sol[:2 * T]
    else:
        x = np.linalg.solve(H, -g)
    return x[:T], x[T:]
