"""Helpers of the ramp-limit tests (DOPF_F_GEN_RAMP), CPU and GPU: the value reference of the generator step under
ramps (a NumPy dynamic programme), its optimality certificate (multipliers from an LP), and the draws and engines the GPU tests share."""
import numpy as np

from decentralopf_jl_amd import _capi

RAMP = getattr(_capi, "F_GEN_RAMP", 0)
CHAIN = _capi.F_NO_FUSE | _capi.F_NO_TAIL_FUSE          # the chain a context with the flag runs


def _interp(xa, va, xb, vb, x):
    return va if va == vb else va + (x - xa) * ((vb - va) / (xb - xa))


def _argmin(kx, kv):
    """the smallest x with h'(x) >= 0, clamped to the knots' range"""
    n = len(kx)
    k = 0
    while k < n and kv[k] < 0.0:
        k += 1
    if k == 0:
        return kx[0]
    if k == n:
        return kx[-1]
    xa, va, xb, vb = kx[k - 1], kv[k - 1], kx[k], kv[k]
    if xb == xa:
        return xb
    return min(max(xa + (-va) * ((xb - xa) / (vb - va)), xa), xb)


def ramp_project(c, q, cap, up, down, prev=None, knots=None):
    """The minimiser of q / 2 |x - c|^2 over 0 <= x_t <= cap_t, -down <= x_t - x_{t-1} <= up (t >= 1, and t = 0 against prev where
    one is given), exactly: a forward dynamic programme over h_t', the derivative of the cost-to-go as a function of x_t — non-decreasing,
    piecewise linear, kept as knots (x, v); two knots may share an x (a jump) — and a backward pass. Per step: y*_{t-1} = the smallest
    x with h' >= 0; the knots with v < 0 move to x - down, those with v > 0 to x + up (split by the sign of v, not by position: that
    keeps a jump's one-sided values), v == 0 is dropped, (y* - down, 0) and (y* + up, 0) go between; clip to [max(0, first x),
    min(cap_t, last x)], interpolating at the new ends; add q (x - c_t). c: (T,); cap: (T,) or a number; up, down >= 0 (inf: no limit).
    knots: a list that receives the largest knot count."""
    c = np.asarray(c, dtype=np.float64)
    T = c.size
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    pm = float(cap.max()) if prev is None else max(float(cap.max()), float(prev))
    up, down = min(float(up), pm), min(float(down), pm)      # (a ramp of the box's width or more never binds: no infinities below)
    lo, hi = 0.0, float(cap[0])
    if prev is not None:
        lo, hi = max(lo, prev - down), min(hi, prev + up)
    assert lo <= hi, "infeasible anchor"
    kx, kv = [lo, hi], [q * (lo - c[0]), q * (hi - c[0])]
    ys = np.zeros(T)
    most = 2
    for t in range(1, T):
        y = ys[t - 1] = _argmin(kx, kv)
        neg = [(x - down, v) for x, v in zip(kx, kv) if v < 0.0]
        pos = [(x + up, v) for x, v in zip(kx, kv) if v > 0.0]
        kn = neg + [(y - down, 0.0), (y + up, 0.0)] + pos
        most = max(most, len(kn))
        lo, hi = max(0.0, kn[0][0]), min(float(cap[t]), kn[-1][0])
        assert lo <= hi, f"infeasible at t = {t}"
        a = max(j for j in range(len(kn)) if kn[j][0] <= lo)            # the value at lo from the right
        b = min(j for j in range(len(kn)) if kn[j][0] >= hi)            # at hi from the left
        vlo = kn[a][1] if kn[a][0] == lo else _interp(*kn[a], *kn[a + 1], lo)
        vhi = kn[b][1] if kn[b][0] == hi else _interp(*kn[b - 1], *kn[b], hi)
        if not lo < hi:
            vlo = vhi = 0.0
        kn = [(lo, vlo)] + kn[a + 1:b] + [(hi, vhi)]
        kx = [x for x, _ in kn]
        kv = [v + q * (x - c[t]) for x, v in kn]
    if knots is not None:
        knots.append(most)
    x = np.zeros(T)
    x[T - 1] = _argmin(kx, kv)
    for t in range(T - 1, 0, -1):
        x[t - 1] = min(max(ys[t - 1], x[t] - up), x[t] + down)
    return x


def ramp_infeasibility(P, cap, up, down, prev=None):
    """the largest violation of the box and the ramps (>= 0)"""
    P = np.asarray(P, dtype=np.float64)
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), P.shape)
    v = max(0.0, float((-P).max()), float((P - cap).max()))
    d = np.diff(P) if prev is None else np.diff(np.concatenate([[prev], P]))
    if d.size:
        v = max(v, float((d - up).max()), float((-d - down).max()))
    return v


def ramp_active(P, up, down, prev=None, tol=1e-9):
    """some ramp of the row holds with equality"""
    P = np.asarray(P, dtype=np.float64)
    d = np.diff(P) if prev is None else np.diff(np.concatenate([[prev], P]))
    return bool(d.size and (np.any(d >= up - tol) or np.any(-d >= down - tol)))


def ramp_kkt_violation(P, g, cap, up, down, prev=None, tol=1e-9):
    """(infeasibility, stationarity) of one row P (T,) as the minimiser of a convex f with gradient g (T,) at P over
    0 <= P_t <= cap_t, -down <= P_t - P_{t-1} <= up (t >= 1; t = 0 against prev where given). Multipliers >= 0 are allowed on the
    active sides only — a-_t (P_t = 0), a+_t (P_t = cap_t), u_t (P_t - P_{t-1} = up), d_t (= -down) — and with nu = u - d the
    stationarity residual is r_t = g_t + a+_t - a-_t + nu_t - nu_{t+1}. They come from an LP (HiGHS) that minimises max |r_t|; the
    residual is then formed again in float64 from the multipliers clipped at 0 (HiGHS alone resolves ~1e-7)."""
    from scipy.optimize import linprog
    P, g = np.asarray(P, dtype=np.float64), np.asarray(g, dtype=np.float64)
    T = P.size
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    infeas = ramp_infeasibility(P, cap, up, down, prev)
    before = np.concatenate([[np.nan if prev is None else prev], P[:-1]])
    d = P - before                                                   # (NaN: no constraint in front of t = 0)
    act = np.stack([P >= cap - tol, P <= tol, d >= up - tol, -d >= down - tol])        # a+, a-, u, d
    act[2:] &= ~np.isnan(d)
    # x = [a+ (T) | a- (T) | u (T) | d (T) | z]; r = g + M x[:4T]
    M = np.zeros((T, 4 * T))
    for t in range(T):
        M[t, t], M[t, T + t], M[t, 2 * T + t], M[t, 3 * T + t] = 1.0, -1.0, 1.0, -1.0
        if t + 1 < T:
            M[t, 2 * T + t + 1], M[t, 3 * T + t + 1] = -1.0, 1.0
    scale = max(1.0, float(np.abs(g).max()))
    A = np.block([[M, -np.ones((T, 1))], [-M, -np.ones((T, 1))]])
    b = np.concatenate([-g, g]) / scale
    bounds = [(0.0, None if on else 0.0) for on in act.reshape(-1)] + [(0.0, None)]
    res = linprog(np.concatenate([np.zeros(4 * T), [1.0]]), A_ub=A, b_ub=b, bounds=bounds, method="highs")
    if res.status != 0:
        return infeas, float("inf")
    x = np.where(act.reshape(-1), np.maximum(res.x[:4 * T], 0.0), 0.0) * scale
    return infeas, float(np.abs(g + M @ x).max())


def draw_ramps(pp, rng):
    """(up, down) per generator from {inf, 0, 2 % .. 30 % of pmax}: every fifth pair unlimited, one generator at 0"""
    G = pp.G
    up = rng.uniform(0.02, 0.30, G) * pp.gen_pmax
    down = rng.uniform(0.02, 0.30, G) * pp.gen_pmax
    up[::5] = down[::5] = np.inf
    if G > 2:
        up[2] = down[2] = 0.0
    if G > 3:
        down[3] = np.inf
    return up, down


def ramp_engine(api, pp, ramp=None, prev=None, flags=0, **params):
    """a context with the flag; ramp = (up, down): set after create (None with prev None: the setter is not called)"""
    e = _capi.Engine(api, params=_capi.default_params(flags=flags | RAMP, **params), **pp.engine_kwargs())
    if ramp is not None or prev is not None:
        e.set_ramp(*(ramp if ramp is not None else (None, None)), prev)
    return e


def step_centres(pp, c2, before, gamma, w=1.0):
    """(c, q) of the copper-plate generator step from the state `before` (helpers.state_of): q = w + gamma + c2 per row and
    c = p0 - (mc + c2 p0 + price + gamma s) / q with price[n,t] = lam[t] and s = sum of the injections (DESIGN.md 3, L = 0)."""
    c2 = np.broadcast_to(np.asarray(c2, dtype=np.float64), (pp.G,))[:, None]
    p0 = before["P"]
    s = before["inj"].sum(axis=0)
    q = w + gamma + c2
    c = p0 - (pp.gen_mc[:, None] + c2 * p0 + before["lam"][None, :] + gamma * s[None, :]) / q
    return c, np.broadcast_to(q, (pp.G, 1))[:, 0]
