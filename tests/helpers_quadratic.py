"""Helpers of the quadratic-cost tests (DOPF_F_GEN_QUADRATIC_COST), CPU and GPU: the oracle pin (an iteration with
quadratic costs assembled from T = 1 oracle problems with linear costs), an optimality certificate of the generator step in NumPy,
the central QP (SciPy) and the draws the GPU tests share."""
import copy

import numpy as np

from decentralopf_jl_amd import _capi, synth
from helpers_efficiency import psi_at
from helpers_line_rating import psi_at_rated

QC = getattr(_capi, "F_GEN_QUADRATIC_COST", 0)
CHAIN = _capi.F_NO_FUSE | _capi.F_NO_TAIL_FUSE          # the chain a context with the flag runs
STATE_KEYS = ("P", "lam", "mu", "rho", "avg_U", "avg_K", "inj")

# the oracle-pinned cases: (synthetic_case arguments, c2, steps); gamma = 1 / agents as in the free runs of the parity tests
COPPER_ODD = (dict(n_gen=7, n_sto=0, T=5, seed=3), 0.5, 30)
COPPER_EVEN = (dict(n_gen=7, n_sto=0, T=4, seed=3), 0.5, 30)
NETWORK = (dict(n_gen=12, n_sto=0, T=4, N=6, L=8, seed=2), 2.0, 40)


def case(kw):
    return synth.synthetic_case(**kw)


def params_of(pp):
    """the parameters every test of a case shares: gamma = 1 / agents (and the flow weight scaled alike on networks), no stop test"""
    A = pp.G + pp.S
    return dict(eps=0.0, gamma=1.0 / A) if pp.L == 0 else dict(eps=0.0, gamma=1.0 / A, w_flow=0.3 / A)


def total_cost(pp, c2, P, D=None, C=None):
    """sum mc P + c2 P^2 / 2 (+ the storages' mc (D + C))"""
    c2 = np.broadcast_to(np.asarray(c2, dtype=np.float64), (pp.G,))
    cost = float((pp.gen_mc[:, None] * P + 0.5 * c2[:, None] * P * P).sum())
    if D is not None and pp.S:
        cost += float((pp.sto_mc[:, None] * (D + C)).sum())
    return cost


def quad_engine(api, pp, c2=None, flags=0, **params):
    """a context with the flag; c2: set after create (None: the setter is not called)"""
    e = _capi.Engine(api, params=_capi.default_params(flags=flags | QC, **params), **pp.engine_kwargs())
    if c2 is not None:
        e.set_quadratic_cost(np.broadcast_to(np.asarray(c2, dtype=np.float64), (pp.G,)))
    return e


def zero_state(pp):
    """the state of a new context"""
    z = lambda r: np.zeros((r, pp.T))
    return dict(P=z(pp.G), D=z(pp.S), C=z(pp.S), lam=np.zeros(pp.T), mu=z(pp.L), rho=z(pp.L), avg_U=z(pp.L), avg_K=z(pp.L),
                inj=-np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T))


def slice_reference(oracle_api, pp, c2, state, iteration, rating=None, **params):
    """The oracle pin: one iteration with the common quadratic coefficient c2 from `state` (helpers.state_of: P, lam, mu, rho,
    avg_U, avg_K), for problems without storages, where an iteration separates over t. Around p0 = P[g,t] the generator's step with
    cost mc P + c2 P^2 / 2 and proximal weight w is the step with cost (mc + c2 p0) P and weight w + c2, so for each t
    an oracle context (exact mode) of the T = 1 problem with demand[:, t], gen_mc + c2 P[:, t], w_prox + c2 (rating: f_max =
    rating[:, t]) is set to column t of the state, iterates once, and the columns are assembled. params: those of
    _capi.default_params (gamma, w_flow, w_prox, ...). Returns P, lam, mu, rho, avg_U, avg_K, inj, flow and the cost
    sum mc P + c2 P^2 / 2."""
    assert pp.S == 0 and np.ndim(c2) == 0
    c2 = float(c2)
    w = float(params.get("w_prox", 1.0))
    out = {k: np.zeros_like(np.asarray(state[k], dtype=np.float64)) for k in STATE_KEYS}
    out["flow"] = np.zeros((pp.L, pp.T))
    for t in range(pp.T):
        q = copy.copy(pp)
        q.T = 1
        q.demand = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, t:t + 1].copy()
        q.gen_mc = pp.gen_mc + c2 * state["P"][:, t]
        q.gen_c2 = q.gen_avail = q.gen_avail_of = q.line_rating = None
        if rating is not None:
            q.f_max = np.asarray(rating, dtype=np.float64).reshape(pp.L, pp.T)[:, t].copy()
        e = _capi.Engine(oracle_api, params=_capi.default_params(**dict(params, w_prox=w + c2)), mode=1, **q.engine_kwargs())
        col = lambda a: np.asarray(a, dtype=np.float64)[:, t:t + 1]
        e.set_state(P=col(state["P"]), D=np.zeros((0, 1)), C_=np.zeros((0, 1)), avg_U=col(state["avg_U"]), avg_K=col(state["avg_K"]),
                    lam=np.asarray(state["lam"], dtype=np.float64)[t:t + 1], mu=col(state["mu"]), rho=col(state["rho"]),
                    iteration=int(iteration))
        e.iterate(1)
        P, _, _, _ = e.get_primal()
        lam, mu, rho = e.get_duals()
        inj, aU, aK, flow, _ = e.get_consensus()
        for k, a in (("P", P), ("mu", mu), ("rho", rho), ("avg_U", aU), ("avg_K", aK), ("inj", inj), ("flow", flow)):
            out[k][:, t] = a[:, 0]
        out["lam"][t] = lam[0]
        e.close()
    out["cost"] = np.asarray([total_cost(pp, c2, out["P"])])
    return out


def interior_fraction(pp, P, cap=None):
    """share of the (g, t) strictly inside their box [0, cap] (cap: gen_pmax)"""
    cap = pp.gen_pmax[:, None] if cap is None else cap
    return float(np.mean((P > 0.0) & (P < cap)))


def gen_kkt_violation(pp, c2, cap, before, duals, P_new, gamma, w_flow, w=1.0, rating=None, tol=1e-9):
    """Optimality certificate of the generators' step. With p0 = before["P"], the step minimises
    mc P + c2 P^2 / 2 + Phi_{n,t}(P - p0) + w (P - p0)^2 / 2 over [0, cap], Phi' = Psi, so
        r = mc + c2 P + Psi(P - p0) + w (P - p0)
    is >= 0 where P = 0, <= 0 where P = cap and 0 inside. Psi: helpers_efficiency.psi_at at the generators' nodes, from the state
    the solve read (before: helpers.state_of before the iteration; duals: its lam, mu, rho; rating: the (L, T) table of
    DOPF_F_LINE_RATING). c2: (G,) or a number; cap: (G, T) or (G,). Returns the largest violation."""
    c2 = np.broadcast_to(np.asarray(c2, dtype=np.float64), (pp.G,))[:, None]
    cap = np.asarray(cap, dtype=np.float64)
    cap = np.broadcast_to(cap[:, None] if cap.ndim == 1 else cap, (pp.G, pp.T))
    p0 = before["P"]
    q = copy.copy(pp)
    q.sto_node = pp.gen_node            # (psi_at evaluates Psi at sto_node)
    flow = np.asarray(pp.ptdf, dtype=np.float64).reshape(pp.L, pp.N) @ before["inj"]
    args = (q, duals[0], duals[1], duals[2], before["inj"], flow, before["avg_U"], before["avg_K"], gamma, w_flow, P_new - p0)
    psi = psi_at(*args) if rating is None else psi_at_rated(*args, rating)
    r = pp.gen_mc[:, None] + c2 * P_new + psi + w * (P_new - p0)
    at0, atc = P_new <= tol, P_new >= cap - tol
    viol = np.where(at0 & atc, 0.0, np.where(at0, np.maximum(0.0, -r), np.where(atc, np.maximum(0.0, r), np.abs(r))))
    viol = np.maximum(viol, np.maximum(0.0, np.maximum(-P_new, P_new - cap)))          # (and inside the box)
    return float(viol.max()) if viol.size else 0.0


def solve_qp(pp, c2):
    """The central QP, min sum mc P + c2 P^2 / 2 + sum sto_mc (D + C) over the generators' and storages' boxes, the balance
    sum_n injection = 0 per timestep, |ptdf injection| <= f_max and 0 <= cumsum(C - D) <= emax, by SciPy's SLSQP; then polished: the
    active set SLSQP ends on is imposed as equalities and the KKT system of that equality-constrained QP is solved exactly (kept
    when it is feasible and no worse). Returns (objective, P, D, C)."""
    from scipy.optimize import minimize
    N, L, T, G, S = pp.N, pp.L, pp.T, pp.G, pp.S
    c2 = np.broadcast_to(np.asarray(c2, dtype=np.float64), (G,))
    nP, nS = G * T, S * T
    n = nP + 2 * nS
    h = np.concatenate([np.repeat(c2, T), np.zeros(2 * nS)])
    g = np.concatenate([np.repeat(pp.gen_mc, T), np.repeat(pp.sto_mc, T), np.repeat(pp.sto_mc, T)])
    ub = np.concatenate([np.repeat(pp.gen_pmax, T), np.repeat(pp.sto_pmax, T), np.repeat(pp.sto_pmax, T)])
    # injection[n, t] = M x - demand
    M = np.zeros((N * T, n))
    for i in range(G):
        for t in range(T):
            M[pp.gen_node[i] * T + t, i * T + t] = 1.0
    for i in range(S):
        for t in range(T):
            M[pp.sto_node[i] * T + t, nP + i * T + t] = 1.0
            M[pp.sto_node[i] * T + t, nP + nS + i * T + t] = -1.0
    dem = np.asarray(pp.demand, dtype=np.float64).reshape(N, T).reshape(-1)
    Aeq = np.kron(np.ones((1, N)), np.eye(T)) @ M
    beq = np.kron(np.ones((1, N)), np.eye(T)) @ dem
    rows, rhs = [], []                                       # A x <= b
    if L > 0:
        F = np.kron(np.asarray(pp.ptdf, dtype=np.float64).reshape(L, N), np.eye(T))
        fm = np.repeat(pp.f_max, T)
        rows += [F @ M, -F @ M]
        rhs += [fm + F @ dem, fm - F @ dem]
    if S > 0:
        Lm = np.kron(np.eye(S), np.tril(np.ones((T, T))))
        E = np.hstack([np.zeros((nS, nP)), -Lm, Lm])
        rows += [E, -E]
        rhs += [np.repeat(pp.sto_emax, T), np.zeros(nS)]
    A = np.vstack(rows) if rows else np.zeros((0, n))
    b = np.concatenate(rhs) if rhs else np.zeros(0)
    f = lambda x: 0.5 * x @ (h * x) + g @ x
    cons = [dict(type="eq", fun=lambda x: Aeq @ x - beq, jac=lambda x: Aeq)]
    if A.shape[0]:
        cons.append(dict(type="ineq", fun=lambda x: b - A @ x, jac=lambda x: -A))
    x0 = np.concatenate([np.repeat(pp.gen_pmax, T) * np.tile(beq / pp.gen_pmax.sum(), G), np.zeros(2 * nS)])
    r = minimize(f, x0, jac=lambda x: h * x + g, bounds=list(zip(np.zeros(n), ub)), constraints=cons, method="SLSQP",
                 options=dict(ftol=1e-15, maxiter=1000))
    x = np.clip(r.x, 0.0, ub)
    # polish on the active set
    act, val = [], []
    for i in range(n):
        if x[i] <= 1e-6 or x[i] >= ub[i] - 1e-6:
            e = np.zeros(n)
            e[i] = 1.0
            act.append(e)
            val.append(0.0 if x[i] <= 1e-6 else ub[i])
    for k in range(A.shape[0]):
        if A[k] @ x >= b[k] - 1e-6:
            act.append(A[k])
            val.append(b[k])
    Ae = np.vstack([Aeq] + ([np.asarray(act)] if act else []))
    be = np.concatenate([beq, np.asarray(val)])
    K = np.block([[np.diag(h), Ae.T], [Ae, np.zeros((Ae.shape[0], Ae.shape[0]))]])
    y = np.linalg.lstsq(K, np.concatenate([-g, be]), rcond=None)[0][:n]
    feas = (np.all(y >= -1e-9) and np.all(y <= ub + 1e-9) and np.abs(Aeq @ y - beq).max() <= 1e-8 and
            (A.shape[0] == 0 or np.all(A @ y <= b + 1e-8)))
    if feas and f(y) <= f(x) + 1e-9 * max(1.0, abs(f(x))):
        x = np.clip(y, 0.0, ub)
    return float(f(x)), x[:nP].reshape(G, T), x[nP:nP + nS].reshape(S, T), x[nP + nS:].reshape(S, T)


def draw_c2(G, rng):
    """c2 uniform in [0, 1], every fourth value 0, one value 50"""
    c2 = rng.uniform(0.0, 1.0, G)
    c2[::4] = 0.0
    if G > 1:
        c2[1] = 50.0
    return c2
