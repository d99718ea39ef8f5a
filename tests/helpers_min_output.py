"""Helpers of the minimum-output tests (dopf_set_generator_min_output), CPU and GPU: the NumPy twins of the two ramp
programmes with a floor vector — helpers_ramp.ramp_project and helpers_ramp_net.ramp_project_pwl, statement by statement, with the
lower end of step t's box at lo_t in 0's place —, an independent dense QP for them (the oracle's generic QP solver, which shares no
code with either), the certificate with the floor as the lower bound, the setter's forward-interval check, and seeded rows."""
import ctypes as C

import numpy as np

from helpers_ramp import _argmin, _interp
from helpers_ramp_net import _add_phi, draw_step, phi_at

_dp = C.POINTER(C.c_double)


def floor_of(p_min, cap):
    """floor[t] = min(p_min, cap[t]): the floor follows the cap down (one fmin, as the kernels form it)"""
    return np.minimum(float(p_min), np.asarray(cap, dtype=np.float64))


def path_exists(lo, cap, up, down, prev=None):
    """The setter's check: the forward intervals F_0 = [max(lo_0, prev - down), min(cap_0, prev + up)] ([lo_0, cap_0] without an
    anchor), F_t = [max(lo_t, a_{t-1} - down), min(cap_t, b_{t-1} + up)]; returns the first t with an empty one, or None."""
    a = b = 0.0
    for t in range(len(cap)):
        if t == 0:
            a, b = (lo[0], cap[0]) if prev is None else (max(lo[0], prev - down), min(cap[0], prev + up))
        else:
            a, b = max(lo[t], a - down), min(cap[t], b + up)
        if a > b:
            return t
    return None


def ramp_project_floor(c, q, lo, cap, up, down, prev=None, knots=None):
    """helpers_ramp.ramp_project over lo_t <= x_t <= cap_t: the same statements in the same order, lo_t where that one has 0.0 (at
    lo = 0 the same bits). lo: (T,) or a number, lo_t <= cap_t; the caller has made sure that a path exists (path_exists)."""
    c = np.asarray(c, dtype=np.float64)
    T = c.size
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    lov = np.broadcast_to(np.asarray(lo, dtype=np.float64), (T,))
    pm = float(cap.max()) if prev is None else max(float(cap.max()), float(prev))
    up, down = min(float(up), pm), min(float(down), pm)      # (a ramp of the box's width or more never binds: no infinities below)
    lo, hi = float(lov[0]), float(cap[0])
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
        lo, hi = max(float(lov[t]), kn[0][0]), min(float(cap[t]), kn[-1][0])
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


def ramp_project_pwl_floor(phi_knots, lo, cap, up, down, prev=None, info=None, K=None):
    """helpers_ramp_net.ramp_project_pwl over lo_t <= x_t <= cap_t — ramp_repair_pwl<true> of csrc/ramp_dp.h in NumPy, the same
    statements in the same order (at lo = 0 the bits of ramp_project_pwl). info also receives "on_floor": the row's result touches
    its floor somewhere."""
    T = len(phi_knots)
    steps = [tuple([float(v) for v in part] for part in st) for st in phi_knots]
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    lov = np.broadcast_to(np.asarray(lo, dtype=np.float64), (T,))
    pm = float(cap.max()) if prev is None else max(float(cap.max()), float(prev))
    up, down = min(float(up), pm), min(float(down), pm)
    if K is not None and K < 2:
        return None
    lo, hi = float(lov[0]), float(cap[0])
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
        lo = max(float(lov[t]), nx[0])
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
    x = np.zeros(T)
    x[T - 1] = _argmin(kx, kv)
    for t in range(T - 1, 0, -1):
        x[t - 1] = min(max(ys[t - 1], x[t] - up), x[t] + down)
    if info is not None:
        info["most"], info["merged"] = most, merged
        info["on_floor"] = bool(np.any((x == lov) & (lov > 0.0)))
    return x


# ---- an independent dense QP -----------------------------------------------------------------------------------------------------------

def _qp(api, Q, c, A, b, lb, ub):
    """the oracle's generic QP solver: min x'Qx / 2 + c'x, A x = b, lb <= x <= ub (Q PSD, row-major)"""
    n, m = len(c), A.shape[0]
    x, y, it = np.zeros(n), np.zeros(max(m, 1)), C.c_int32(0)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (Q, c, A, b, lb, ub)]
    rc = api.qp_solve(n, m, *(a.ctypes.data_as(_dp) for a in arrs), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), C.byref(it))
    assert rc == 0, rc
    return x


def qp_row(api, steps, lo, cap, up, down, prev=None):
    """The row's problem as one dense QP with no dynamic programme in it. Step t's convex cost, whose derivative phi_t is piecewise
    linear, is written over segment variables: x_t = lo_t + sum_j z_tj, 0 <= z_tj <= the length of piece j of [lo_t, cap_t] between
    phi_t's kinks, cost phi_t(start of the piece) z + slope_j z^2 / 2 — the marginal cost rises from piece to piece, so the pieces
    fill in order on their own. The ramps are equalities with a bounded slack: x_t - x_{t-1} - s_t = 0, -down <= s_t <= up (t = 0:
    x_0 - s_0 = prev). steps[t] = (xk, vk, sl) as ramp_project_pwl takes them (line_step(q, c): the copper plate's)."""
    T = len(steps)
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    lov = np.broadcast_to(np.asarray(lo, dtype=np.float64), (T,))
    pm = float(cap.max()) if prev is None else max(float(cap.max()), float(prev))
    up, down = min(float(up), pm), min(float(down), pm)
    seg = []                                                    # (t, start, length, phi at the start from the right, slope)
    for t, (xk, vk, sl) in enumerate(steps):
        m = len(sl) - 1
        pts = [float(lov[t])] + [float(v) for v in xk[:m] if lov[t] < v < cap[t]] + [float(cap[t])]
        for u, v in zip(pts[:-1], pts[1:]):
            mid = 0.5 * (u + v)
            j = sum(1 for z in xk[:m] if z < mid)
            seg.append((t, u, v - u, phi_at((xk, vk, sl), mid) - sl[j] * (mid - u), sl[j]))
    nz = len(seg)
    first = 0 if prev is not None else 1
    ns = T - first
    n = nz + ns
    Q, c = np.zeros((n, n)), np.zeros(n)
    lb, ub = np.zeros(n), np.zeros(n)
    X = np.zeros((T, n))                                        # x_t - lo_t as a row over the variables
    for k, (t, u, ln, v0, s) in enumerate(seg):
        Q[k, k], c[k], ub[k] = s, v0, ln
        X[t, k] = 1.0
    A, b = np.zeros((max(ns, 1), n)), np.zeros(max(ns, 1))
    for r, t in enumerate(range(first, T)):
        A[r] = X[t] - (X[t - 1] if t > 0 else 0.0)
        A[r, nz + r] = -1.0
        b[r] = (lov[t - 1] if t > 0 else prev) - lov[t]
        lb[nz + r], ub[nz + r] = -down, up
    z = _qp(api, Q, c, A[:ns], b[:ns], lb, ub)
    return lov + X @ z


# ---- the certificate with a floor ------------------------------------------------------------------------------------------------------

def floor_infeasibility(P, lo, cap, up, down, prev=None):
    """the largest violation of the box [lo, cap] and the ramps (>= 0)"""
    P = np.asarray(P, dtype=np.float64)
    v = max(0.0, float((np.broadcast_to(lo, P.shape) - P).max()), float((P - np.broadcast_to(cap, P.shape)).max()))
    d = np.diff(P) if prev is None else np.diff(np.concatenate([[prev], P]))
    if d.size:
        v = max(v, float((d - up).max()), float((-d - down).max()))
    return v


def floor_kkt_violation(P, g, lo, cap, up, down, prev=None, tol=1e-9):
    """helpers_ramp.ramp_kkt_violation with lo_t as the lower bound: (infeasibility, stationarity) of the row P as the minimiser of
    a convex f with gradient g at P over lo_t <= P_t <= cap_t and the ramps; multipliers >= 0 on the active sides only, from an LP
    that minimises max |r_t|, the residual formed again in float64 from the multipliers clipped at 0."""
    from scipy.optimize import linprog
    P, g = np.asarray(P, dtype=np.float64), np.asarray(g, dtype=np.float64)
    T = P.size
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    lov = np.broadcast_to(np.asarray(lo, dtype=np.float64), (T,))
    infeas = floor_infeasibility(P, lov, cap, up, down, prev)
    before = np.concatenate([[np.nan if prev is None else prev], P[:-1]])
    d = P - before
    act = np.stack([P >= cap - tol, P <= lov + tol, d >= up - tol, -d >= down - tol])
    act[2:] &= ~np.isnan(d)
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


# ---- seeded rows -----------------------------------------------------------------------------------------------------------------------

def draw_row(rng, k, T):
    """(p_min, cap, up, down, prev) of seeded row k, a path guaranteed (path_exists): every third row under caps that drop to 0 and
    rise again (the floor rises behind a zero cap), every fourth with up = 0, every second anchored, every fifth a must-take row
    (p_min = pmax); a draw without a path gives up its anchor first, then its finite ramps"""
    pm = float(rng.uniform(10.0, 100.0))
    cap = np.full(T, pm)
    if k % 3 == 0:
        cap = pm * rng.uniform(0.3, 1.0, T)
        if T >= 3:
            z = int(rng.integers(0, T - 1))
            cap[z:z + int(rng.integers(1, 3))] = 0.0
    p_min = pm if k % 5 == 4 else float(rng.uniform(0.05, 0.7) * pm)
    draw = lambda: float(rng.uniform(0.05, 0.5) * pm)
    up = 0.0 if k % 4 == 1 else (np.inf if k % 4 == 3 else draw())
    down = np.inf if k % 6 == 2 else draw()
    prev = float(rng.uniform(0.0, pm)) if k % 2 == 0 else None
    lo = floor_of(p_min, cap)
    if path_exists(lo, cap, up, down, prev) is not None:
        prev = None
    if path_exists(lo, cap, up, down, prev) is not None:
        up = down = np.inf
    assert path_exists(lo, cap, up, down, prev) is None
    return p_min, cap, up, down, prev


def floor_cases(n, seed, tmax=8):
    """seeded copper-plate rows (c, q, lo, cap, up, down, prev), T = 1 .. tmax; the centres lie below the floor for a stretch in every
    second row (the row then rests on its floor)"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        T = 1 if k % 10 == 9 else int(rng.integers(2, tmax + 1))
        p_min, cap, up, down, prev = draw_row(rng, k, T)
        q = float(rng.uniform(0.5, 3.0))
        pm = float(cap.max())
        c = rng.uniform(-0.5 * pm, 1.5 * pm, T)
        if k % 2 == 1:
            a = int(rng.integers(0, T))
            c[a:] = rng.uniform(-0.5 * pm, 0.1 * p_min, T - a)
        yield c, q, floor_of(p_min, cap), cap, up, down, prev


def pwl_floor_cases(n, seed, tmax=8):
    """seeded network rows (steps, lo, cap, up, down, prev): floor_cases' boxes with steps of 0, 1, 3 or 6 kinks (every fourth row
    none); in every second row the steps' zeros lie below the floor from some t on"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        T = 1 if k % 10 == 9 else int(rng.integers(2, tmax + 1))
        p_min, cap, up, down, prev = draw_row(rng, k, T)
        pm = float(cap.max())
        steps = [draw_step(rng, pm, 0 if k % 4 == 0 else int(rng.choice([0, 1, 3, 6]))) for _ in range(T)]
        if k % 2 == 1:
            a = int(rng.integers(0, T))
            for t in range(a, T):                              # phi_t moved up until its zero lies below the floor
                xk, vk, sl = steps[t]
                shift = max(0.0, -phi_at(steps[t], 0.05 * p_min)) + float(rng.uniform(0.1, 2.0))
                steps[t] = (xk, [v + shift for v in vk], sl)
        yield steps, floor_of(p_min, cap), cap, up, down, prev


# ---- the GPU tests' engines ------------------------------------------------------------------------------------------------------------

def set_floor_raw(e, p_min):
    """dopf_set_generator_min_output with the array as given (Engine.set_min_output hands all zeros on as NULL): (rc, message)"""
    a = None if p_min is None else np.ascontiguousarray(p_min, dtype=np.float64)
    rc = e.api.set_generator_min_output(e._ctx, None if a is None else a.ctypes.data_as(_dp))
    msg = e.api.last_error(e._ctx)
    return rc, (msg.decode() if msg else "")


def all_state(e):
    """every getter of the context as one flat list of arrays (bitwise comparisons)"""
    res = e.get_residuals()
    return list(e.get_primal()) + list(e.get_duals()) + list(e.get_consensus()[:4]) + [np.asarray(res[:3], dtype=np.float64)]


def same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- the plates' step on the CPU: what the GPU tests compare against and settle their coverage with --------------------------------

def swing(pp, lo=0.4, hi=1.6):
    """the case with its demand alternating between lo and hi times itself (the ramp tests'): neighbouring steps of a row differ"""
    f = np.where(np.arange(pp.T) % 2 == 0, lo, hi)
    pp.demand = np.round(np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T) * f[None, :])
    return pp


def drawn_state(pp, p_min, rng, gamma):
    """a state that needs no device to be known: P between floor and capacity, the storages at rest, the line vectors at
    zero, and lambda such that the price a row sees, lambda + gamma s with s = sum P - demand, is minus a target that alternates
    between a high and a low quantile of the generators' costs — in the even steps most rows want to run, in the odd ones most want
    to stop, which is what sends a ramped row onto its floor; set with iteration = 2"""
    P = p_min[:, None] + rng.uniform(0.0, 1.0, (pp.G, pp.T)) * (pp.gen_pmax - p_min)[:, None]
    near = np.arange(pp.G) % 2 == 1                              # every second row starts within a step's reach of its floor
    P[near] = p_min[near, None] + rng.uniform(0.0, 0.05, (int(near.sum()), pp.T)) * (pp.gen_pmax - p_min)[near, None]
    s = P.sum(axis=0) - np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T).sum(axis=0)
    mc = np.sort(pp.gen_mc)[:-1] if pp.G > 1 else pp.gen_mc
    hi, lo = np.quantile(mc, 0.9) + 1.0, np.quantile(mc, 0.1) - 1.0
    target = np.where(np.arange(pp.T) % 2 == 0, hi, lo) + rng.uniform(-0.5, 0.5, pp.T)
    lam = -gamma * s - target
    z = np.zeros((pp.S, pp.T))
    return dict(P=P, D=z, C=z.copy(), lam=lam, mu=np.zeros((pp.L, pp.T)), rho=np.zeros((pp.L, pp.T)), avg_U=np.zeros((pp.L, pp.T)),
                avg_K=np.zeros((pp.L, pp.T)))


def plate_rows(c, q, p_min, cap, up, down, prev):
    """per row of a copper plate, from its centres (helpers_ramp.step_centres): (ramp_project_floor's answer, it is repaired — the
    clamp of its centres breaks a ramp —, its answer touches the floor, it sits on its floor throughout, a floor that is not 0 everywhere)"""
    out = []
    for g in range(c.shape[0]):
        pv = None if prev is None else float(prev[g])
        lo = floor_of(p_min[g], cap[g])
        want = ramp_project_floor(c[g], q[g], lo, cap[g], up[g], down[g], pv)
        repaired = floor_infeasibility(np.clip(c[g], lo, cap[g]), lo, cap[g], min(up[g], 1e300), min(down[g], 1e300), pv) > 0.0
        on = (want == lo) & (lo > 0.0)
        out.append((want, repaired, bool(on.any()), bool(np.all(want == lo) and np.any(lo > 0.0))))
    return out


def floor_profiles(pp, p_min, up, down, prev, rng):
    """(profiles, profile_of, cap) for a case with floors: one profile that stays within [0.6, 1] (a floor of at most 0.4 pmax stays
    below the cap), one with a zero stretch and a rise behind it (the floor follows it down to 0 and up again); every third row has
    none. up, down and prev (None: no anchors) are changed in place: the anchors come under the first cap, and a row that is left
    without a path (path_exists) gives up its finite ramps"""
    G, T = pp.G, pp.T
    prof = np.stack([rng.uniform(0.6, 1.0, T), rng.uniform(0.5, 1.0, T)])
    z = max(1, T // 3)
    prof[1, z:z + max(1, T // 5)] = 0.0
    of = (np.arange(G) % 3 - 1).astype(np.int32)                   # -1, 0, 1, -1, ..
    cap = np.where((of >= 0)[:, None], pp.gen_pmax[:, None] * prof[np.maximum(of, 0)], np.repeat(pp.gen_pmax[:, None], T, axis=1))
    for g in range(G):
        lo = floor_of(p_min[g], cap[g])
        if prev is not None:
            prev[g] = max(float(lo[0]), min(float(prev[g]), float(cap[g, 0])))
        if path_exists(lo, cap[g], up[g], down[g], None if prev is None else prev[g]) is not None:
            up[g] = down[g] = np.inf
    return prof, of, cap


PLATES = {"7x5": lambda: (7, 0, 5, 3), "9+4x6": lambda: (9, 4, 6, 5), "3x70": lambda: (3, 0, 70, 4), "3x130": lambda: (3, 0, 130, 9)}


def plate_draw(name, quad, seed, avail=False):
    """One seeded copper plate of the GPU tests with everything the step needs, known without a device: the case (its last generator
    a must-run unit nobody would dispatch: 20 times its cost, which keeps it on its floor), ramps, floors of 10 % .. 40 % of the
    capacity, c2, anchors between floor and capacity, a state (drawn_state). avail: profiles too (floor_profiles), and the caps under
    them."""
    from decentralopf_jl_amd import synth
    from helpers_quadratic import draw_c2, params_of
    from helpers_ramp import draw_ramps
    G, S, T, case_seed = PLATES[name]()
    pp = swing(synth.synthetic_case(G, S, T, seed=case_seed))
    pp.gen_mc = pp.gen_mc.copy()
    pp.gen_mc[-1] = 20.0 * float(pp.gen_mc.max())
    rng = np.random.default_rng(seed)
    up, down = draw_ramps(pp, rng)
    p_min = rng.uniform(0.1, 0.4, G) * pp.gen_pmax
    c2 = draw_c2(G, rng) if quad else np.zeros(G)
    prev = p_min + rng.uniform(0.0, 1.0, G) * (pp.gen_pmax - p_min)
    prev[-1] = p_min[-1]
    st = drawn_state(pp, p_min, rng, params_of(pp)["gamma"])
    cap = np.repeat(pp.gen_pmax[:, None], T, axis=1)
    prof = of = None
    if avail:
        prof, of, cap = floor_profiles(pp, p_min, up, down, prev, rng)
    return dict(pp=pp, prm=params_of(pp), up=up, down=down, p_min=p_min, c2=c2, prev=prev, st=st, cap=cap, prof=prof, of=of)
