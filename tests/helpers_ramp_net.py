"""Helpers of the tests of ramp limits on networks (DOPF_F_GEN_RAMP_NETWORK), CPU and GPU: the NumPy twin of
csrc/ramp_dp.h — the dynamic programme of helpers_ramp.ramp_project with a piecewise-linear increasing derivative phi_t per step — and
the steps' derivatives of a network's generators from the closed forms of DESIGN.md section 3 (never from the device's tables)."""
import types

import numpy as np

from decentralopf_jl_amd import _capi
from helpers_line_rating import psi_at_rated
from helpers_ramp import RAMP, _argmin, _interp

RAMP_NET = getattr(_capi, "F_GEN_RAMP_NETWORK", 0)
NET = RAMP | RAMP_NET                                   # what a ramped context on a network is created with
CHAIN_NET = _capi.F_NO_FUSE                             # the chain such a context runs


def line_step(q, c):
    """the step phi(x) = q (x - c) in the form ramp_project_pwl takes: no kink, one line of slope q through (c, 0)"""
    return [float(c)], [0.0], [float(q)]


def _phi(step, x, piece):
    """(phi(x), piece): step = (xk, vk, sl), m = len(sl) - 1 kinks xk (ascending) with values vk and the slopes of the m + 1 pieces;
    m == 0: the line of slope sl[0] through (xk[0], vk[0]). piece: a cursor that only moves up while x does."""
    xk, vk, sl = step
    m = len(sl) - 1
    while piece < m and xk[piece] < x:
        piece += 1
    a = piece if piece < m else (m - 1 if m > 0 else 0)
    return vk[a] + sl[piece] * (x - xk[a]), piece


def _add_phi(step, kx, kv, K):
    """dp_add_phi of csrc/ramp_dp.h, statement by statement: the kinks strictly inside (kx[0], kx[-1]) become knots (backward merge,
    values interpolated), then phi is added at every knot. Returns the number of kinks merged, or -1 (nothing changed) beyond K."""
    xk = step[0]
    m = len(step[2]) - 1
    n = len(kx)
    cnt = 0
    if m > 0:
        lo, hi = kx[0], kx[n - 1]
        j0 = 0
        while j0 < m and not xk[j0] > lo:
            j0 += 1
        j1 = j0
        while j1 < m and xk[j1] < hi:
            j1 += 1
        cnt = j1 - j0
        if K is not None and n + cnt > K:
            return -1
        kx.extend([0.0] * cnt)
        kv.extend([0.0] * cnt)
        i, w, j = n - 1, n + cnt - 1, j1 - 1
        while j >= j0:
            x = xk[j]
            if kx[i] > x:
                kx[w], kv[w] = kx[i], kv[i]
                i -= 1
            else:
                kv[w] = _interp(kx[i], kv[i], kx[w + 1], kv[w + 1], x)
                kx[w] = x
                j -= 1
            w -= 1
    piece = 0
    for k in range(len(kx)):
        f, piece = _phi(step, kx[k], piece)
        kv[k] += f
    return cnt


def ramp_project_pwl(phi_knots, cap, up, down, prev=None, info=None, K=None):
    """The minimiser of sum_t f_t(x_t), f_t' = phi_t, over 0 <= x_t <= cap_t, -down <= x_t - x_{t-1} <= up (t >= 1; t = 0 against
    prev where given): helpers_ramp.ramp_project with its step (4), "add q (x - c_t)", replaced by "merge phi_t's kinks into the
    knots, add phi_t" — ramp_repair_pwl of csrc/ramp_dp.h in NumPy, the same statements in the same order. phi_knots: T steps
    (xk, vk, sl) as _phi takes them (line_step(q, c): the copper-plate step). info: a dict that receives the largest knot count
    ("most") and the kinks merged per step ("merged", T values). K: the knot capacity (None: unbounded); returns None where the
    programme needs more."""
    T = len(phi_knots)
    steps = [tuple([float(v) for v in part] for part in st) for st in phi_knots]
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    pm = float(cap.max()) if prev is None else max(float(cap.max()), float(prev))
    up, down = min(float(up), pm), min(float(down), pm)      # (a ramp of the box's width or more never binds: no infinities below)
    if K is not None and K < 2:
        return None
    lo, hi = 0.0, float(cap[0])
    if prev is not None:
        lo, hi = max(lo, prev - down), min(hi, prev + up)
    hi = max(hi, lo)
    kx, kv = [lo, hi], [0.0, 0.0]
    merged = [_add_phi(steps[0], kx, kv, K)]
    if merged[0] < 0:
        return None
    ys = np.zeros(T)
    most = len(kx)
    for t in range(1, T):
        n = len(kx)
        y = ys[t - 1] = _argmin(kx, kv)
        k = 0
        while k < n and kv[k] < 0.0:
            k += 1
        p = k
        while p < n and kv[p] <= 0.0:
            p += 1
        if K is not None and k + 2 + (n - p) > K:
            return None
        nx = [x - down for x in kx[:k]] + [y - down, y + up] + [x + up for x in kx[p:]]
        nv = kv[:k] + [0.0, 0.0] + kv[p:]
        n2 = len(nx)
        most = max(most, n2)
        lo = max(0.0, nx[0])
        hi = max(min(float(cap[t]), nx[n2 - 1]), lo)
        a, b = 0, n2 - 1
        while a + 1 < n2 and nx[a + 1] <= lo:
            a += 1
        while b > 0 and nx[b - 1] >= hi:
            b -= 1
        vlo = nv[a] if nx[a] == lo else _interp(nx[a], nv[a], nx[a + 1], nv[a + 1], lo)
        vhi = nv[b] if nx[b] == hi else _interp(nx[b - 1], nv[b - 1], nx[b], nv[b], hi)
        if not lo < hi:
            vlo = vhi = 0.0
        kx = [lo] + nx[a + 1:b] + [hi]
        kv = [vlo] + nv[a + 1:b] + [vhi]
        merged.append(_add_phi(steps[t], kx, kv, K))
        if merged[-1] < 0:
            return None
        most = max(most, len(kx))
    if info is not None:
        info["most"], info["merged"] = most, merged
    x = np.zeros(T)
    x[T - 1] = _argmin(kx, kv)
    for t in range(T - 1, 0, -1):
        x[t - 1] = min(max(ys[t - 1], x[t] - up), x[t] + down)
    return x


def phi_at(step, x):
    return _phi(tuple(list(map(float, part)) for part in step), float(x), 0)[0]


# ---- a network's generators: phi_t from the closed forms -----------------------------------------------------------------------------

def _as_storages(pp):
    """the case as psi_at_rated reads it, with the generators' nodes where it looks for the agents'"""
    return types.SimpleNamespace(ptdf=pp.ptdf, L=pp.L, N=pp.N, T=pp.T, f_max=pp.f_max, sto_node=pp.gen_node)


def _limits(pp, F):
    return np.repeat(np.asarray(pp.f_max, dtype=np.float64)[:, None], pp.T, axis=1) if F is None else np.asarray(F, dtype=np.float64).reshape(pp.L, pp.T)


def psi_gen(pp, before, gamma, w_flow, dlt, F=None):
    """Psi_{n,t}(dlt) for every generator (at its node) and timestep, dlt (G, T), from the state the solve read (helpers.state_of
    before the iteration; the flows are ptdf . injection, as helpers_efficiency.theta_of takes them). F: the (L, T) rating table."""
    flow = np.asarray(pp.ptdf, dtype=np.float64).reshape(pp.L, pp.N) @ before["inj"]
    return psi_at_rated(_as_storages(pp), before["lam"], before["mu"], before["rho"], before["inj"], flow, before["avg_U"],
                        before["avg_K"], gamma, w_flow, dlt, _limits(pp, F))


def phi_gen(pp, c2, before, gamma, w_flow, P, F=None, w=1.0):
    """the gradient of a generator row's step objective at P (G, T): mc + c2 P + Psi(P - p0) + w (P - p0)"""
    c2 = np.broadcast_to(np.asarray(c2, dtype=np.float64), (pp.G,))[:, None]
    d = P - before["P"]
    return pp.gen_mc[:, None] + c2 * P + psi_gen(pp, before, gamma, w_flow, d, F) + w * d


def net_step_pieces(pp, c2, before, gamma, w_flow, F=None, w=1.0):
    """pieces[g][t] = (xk, vk, sl): phi_t of generator g as ramp_project_pwl takes it, from the closed forms of DESIGN.md section 3.
    The kinks of Psi in the change d of the row's injection are those of the lines' slacks, for every line l with h = ptdf[l, n] != 0:
    U_l switches at d = (gamma a / w2 - f + F) / h, K_l at d = (-gamma b / w2 - f - F) / h; those with p0 + d within one unit of the
    row's box [0, pmax] are kept (phi is asked for inside the box only). Their values come from psi_at_rated, the slopes of the
    pieces between them from the slacks that are on at the pieces' midpoints: gamma + sum_l w2 h^2 (2 - (U on + K on) w2 / (w2 + gamma))
    for Psi, plus c2 + w."""
    G, T, L = pp.G, pp.T, pp.L
    c2 = np.broadcast_to(np.asarray(c2, dtype=np.float64), (G,))
    w2 = 2.0 * w_flow
    H = np.asarray(pp.ptdf, dtype=np.float64).reshape(L, pp.N)[:, np.asarray(pp.gen_node, dtype=np.int64)]          # (L, G)
    flow = np.asarray(pp.ptdf, dtype=np.float64).reshape(L, pp.N) @ before["inj"]
    Fl = _limits(pp, F)
    aU, aK, p0 = before["avg_U"], before["avg_K"], before["P"]
    kinks = [[None] * T for _ in range(G)]
    most = 1
    for g in range(G):
        h = H[:, g]
        on = h != 0.0
        for t in range(T):
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.concatenate([((gamma * aU[:, t] / w2 - flow[:, t] + Fl[:, t]) / h)[on],
                                    ((-gamma * aK[:, t] / w2 - flow[:, t] - Fl[:, t]) / h)[on]])
            x = np.unique(p0[g, t] + d[np.isfinite(d)])
            kinks[g][t] = x[(x > -1.0) & (x < pp.gen_pmax[g] + 1.0)]
            most = max(most, kinks[g][t].size)
    # the values at the kinks, rank by rank (one vectorised Psi per rank; rows with fewer kinks: their reference point p0)
    X = np.repeat(p0[:, :, None], most, axis=2).astype(np.float64)
    for g in range(G):
        for t in range(T):
            X[g, t, :kinks[g][t].size] = kinks[g][t]
    V = np.stack([phi_gen(pp, c2, before, gamma, w_flow, X[:, :, k], F, w) for k in range(most)], axis=2)

    def slope(g, t, x):
        d = x - p0[g, t]
        h, f = H[:, g], flow[:, t]
        u_on = gamma * aU[:, t] - w2 * (f + h * d - Fl[:, t]) > 0.0
        k_on = gamma * aK[:, t] + w2 * (f + h * d + Fl[:, t]) > 0.0
        return c2[g] + w + gamma + float(np.sum(w2 * h * h * (2.0 - (u_on.astype(float) + k_on) * w2 / (w2 + gamma))))

    pieces = [[None] * T for _ in range(G)]
    for g in range(G):
        for t in range(T):
            x = kinks[g][t]
            m = x.size
            if m == 0:
                pieces[g][t] = ([float(p0[g, t])], [float(V[g, t, 0])], [slope(g, t, p0[g, t])])
                continue
            mids = np.concatenate([[x[0] - 1.0], 0.5 * (x[:-1] + x[1:]), [x[-1] + 1.0]])
            pieces[g][t] = (x.tolist(), V[g, t, :m].tolist(), [slope(g, t, v) for v in mids])
    return pieces


# ---- seeded rows for the CPU tests ---------------------------------------------------------------------------------------------------

def draw_step(rng, pm, m):
    """an increasing piecewise-linear phi with m kinks in [-0.2 pm, 1.2 pm], slopes in [0.3, 3], and a zero near c in [-0.5 pm, 1.5 pm]"""
    sl = rng.uniform(0.3, 3.0, m + 1)
    c = float(rng.uniform(-0.5 * pm, 1.5 * pm))
    if m == 0:
        return line_step(sl[0], c)
    xk = np.sort(rng.uniform(-0.2 * pm, 1.2 * pm, m))
    vk = np.zeros(m)
    vk[0] = sl[0] * (xk[0] - c)
    for j in range(1, m):
        vk[j] = vk[j - 1] + sl[j] * (xk[j] - xk[j - 1])
    return xk.tolist(), vk.tolist(), sl.tolist()


def pwl_cases(n, seed, tmax=24):
    """seeded rows (steps, cap, up, down, prev): T = 1 .. tmax (every tenth T = 1), caps that drop to 0, ramps from {inf, 0, 2 % .. 30 % of
    pmax}, every second row anchored (where the anchor can come down under the caps), steps with 0, 1, 3 or 6 kinks — every fourth
    row without any"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        T = 1 if k % 10 == 9 else int(rng.integers(2, tmax + 1))
        pm = float(rng.uniform(10.0, 100.0))
        cap = np.full(T, pm)
        if k % 3 == 0:
            cap = pm * rng.uniform(0.0, 1.0, T)
            cap[rng.random(T) < 0.25] = 0.0
        steps = [draw_step(rng, pm, 0 if k % 4 == 0 else int(rng.choice([0, 1, 3, 6]))) for _ in range(T)]
        draw = lambda: float(rng.uniform(0.02, 0.30) * pm)
        up = (np.inf, 0.0, draw())[k % 3] if k % 7 else draw()
        down = (draw(), np.inf, 0.0)[k % 3] if k % 5 else draw()
        prev = None
        if k % 2 == 0:
            prev, fits = float(rng.uniform(0.0, pm)), True
            lo = prev
            for t in range(T):
                lo = max(0.0, lo - down)
                fits = fits and lo <= cap[t]
            prev = prev if fits else None
        yield steps, cap, up, down, prev


def primitive(step, x):
    """f(x) = the integral of phi from the step's first knot to x (phi is piecewise linear: the trapezoid rule over its kinks is exact)"""
    xk = step[0]
    x0 = xk[0]
    a, b = min(x0, x), max(x0, x)
    pts = [a] + [v for v in xk if a < v < b] + [b]
    s = sum(0.5 * (phi_at(step, u) + phi_at(step, v)) * (v - u) for u, v in zip(pts[:-1], pts[1:]))
    return s if x >= x0 else -s
