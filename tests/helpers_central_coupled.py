"""The coupled device LP (dopf_central_solve_coupled) in NumPy.

1. The twin of csrc/central_rows.h: the same statements in the same order over IEEE doubles (NumPy fuses nothing), for one generator row
   at a time (row_step, row_metrics) — what tests/central_rows_main.cpp prints, bit for bit.
2. The whole primal-dual iteration (pdhg) with the step sizes of kernels_central.hip and the restart scheme of dopf_central.hip
   (batches of 200, restart to the better of last iterate and average when its gap has halved or after 4000 iterations; at every
   restart the primal weight follows the iterates, w <- sqrt(w |dy| / |dx|), as the coupled entry's does), on the pattern of
   scripts/proto_pdlp.py: the signs and step sizes of the new rows, checked against HiGHS without a GPU.
3. The drawing rule of the GPU tests' inputs (draw_inputs) and the checks they share.

Multipliers are positive where a row's upper end binds. The returned duals are d objective / d right-hand side, the reference's
convention (central.py): ramp_dual = -yR, budget_dual = -yQ — negative where the upper end binds (more room is cheaper), positive
where the lower end does."""
import numpy as np

INF = np.inf


# ---- 1. the twin of central_rows.h -------------------------------------------------------------------------------------------------
def clamp(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def anchored(prev):
    return prev == prev


def has_ramp(ru, rd, prev):
    return (ru < INF) | (rd < INF) | anchored(prev)


def has_budget(e_min, e_max):
    return (e_min > 0.0) | (e_max < INF)


def ramp_rows_at(t, T, ramp, anch):
    return np.where(ramp, np.where((t >= 1) | anch, 1, 0) + np.where(t + 1 < T, 1, 0), 0)


def tau(absH, a, b, w):
    return 1.0 / ((1.0 + absH + (a + b).astype(np.float64)) * w)


def ramp_lo(t, rd, prev):
    with np.errstate(invalid="ignore"):
        return np.where(t >= 1, -rd, prev - rd)


def ramp_hi(t, ru, prev):
    with np.errstate(invalid="ignore"):
        return np.where(t >= 1, ru, prev + ru)


def sigma_ramp(t, w):
    return np.where(t >= 1, w / 2.0, w)


def sigma_budget(T, w):
    return w / float(T)


def reduced_cost(mc, pi, yR, yR_next, yQ):
    return mc + pi + yR - yR_next + yQ


def column_step(x0, tau_, rc, cap):
    return clamp(x0 - tau_ * rc, 0.0, cap)


def prox(y, sigma, row, lo, hi):
    z = y + sigma * row
    q = z / sigma
    with np.errstate(invalid="ignore"):
        return np.where(q < lo, z - sigma * lo, np.where(q > hi, z - sigma * hi, 0.0))


def support(y, lo, hi):
    with np.errstate(invalid="ignore"):
        up = np.where(y > 0.0, y * hi, 0.0)
        dn = np.where(y < 0.0, y * lo, 0.0)
    return -(up + dn)


def rc_term(rc, cap):
    return np.where(rc < 0.0, rc, 0.0) * cap


def violation(row, lo, hi):
    a, b = lo - row, row - hi
    m = np.where(a > b, a, b)
    return np.where(m > 0.0, m, 0.0)


def _seq_sum(x):
    """x[0] + x[1] + ... in this order (np.sum adds pairwise)"""
    return float(np.cumsum(np.asarray(x, dtype=np.float64))[-1]) if len(x) else 0.0


def row_step(mc, absH, w, ru, rd, prev, e_min, e_max, pi, cap, x0, yR, yQ):
    """One primal-dual step of one generator row, as tests/central_rows_main.cpp forms it: (x+, yR+, yQ+)."""
    pi, cap, x0, yR = (np.asarray(a, dtype=np.float64) for a in (pi, cap, x0, yR))
    T = x0.size
    t = np.arange(T)
    ramp, anch, bud = bool(has_ramp(ru, rd, prev)), bool(anchored(prev)), bool(has_budget(e_min, e_max))
    a = ramp_rows_at(t, T, ramp, anch)
    yn = np.append(yR[1:], 0.0)
    rc = reduced_cost(mc, pi, yR, yn, yQ)
    xn = column_step(x0, tau(absH, a, np.full(T, int(bud)), w), rc, cap)
    xb = 2.0 * xn - x0
    row = np.where(t >= 1, xb - np.append(0.0, xb[:-1]), xb)
    live = ramp & ((t >= 1) | anch)
    yRn = np.where(live, prox(yR, sigma_ramp(t, w), row, ramp_lo(t, rd, prev), ramp_hi(t, ru, prev)), 0.0)
    yQn = float(prox(yQ, sigma_budget(T, w), _seq_sum(xb), e_min, e_max)) if bud else 0.0
    return xn, yRn, yQn


def row_metrics(mc, ru, rd, prev, e_min, e_max, pi, cap, x, yR, yQ):
    """The row's parts of the metrics: (cost, reduced-cost term, support term, worst violation), sums in t order, ramp rows first."""
    pi, cap, x, yR = (np.asarray(a, dtype=np.float64) for a in (pi, cap, x, yR))
    T = x.size
    t = np.arange(T)
    ramp, anch, bud = bool(has_ramp(ru, rd, prev)), bool(anchored(prev)), bool(has_budget(e_min, e_max))
    rc = reduced_cost(mc, pi, yR, np.append(yR[1:], 0.0), yQ)
    cost, rct = _seq_sum(mc * x), _seq_sum(rc_term(rc, cap))
    row = np.where(t >= 1, x - np.append(0.0, x[:-1]), x)
    live = ramp & ((t >= 1) | anch)
    lo, hi = ramp_lo(t, rd, prev), ramp_hi(t, ru, prev)
    sup = _seq_sum(np.where(live, support(yR, lo, hi), 0.0))
    viol = float(np.max(np.where(live, violation(row, lo, hi), 0.0)))
    if bud:
        s = _seq_sum(x)
        sup = sup + float(support(yQ, e_min, e_max))
        viol = max(viol, float(violation(s, e_min, e_max)))
    return cost, rct, sup, viol


# ---- 2. the whole iteration ----------------------------------------------------------------------------------------------------------
def _coupling(pp, gen_ramp, gen_prev, gen_budget):
    G = pp.G
    ru, rd = (np.full(G, INF), np.full(G, INF)) if gen_ramp is None else (np.asarray(r, dtype=np.float64).reshape(G) for r in gen_ramp)
    prev = np.full(G, np.nan) if gen_prev is None else np.asarray(gen_prev, dtype=np.float64).reshape(G)
    lo, hi = (None, None) if gen_budget is None else gen_budget
    e_min = np.zeros(G) if lo is None else np.asarray(lo, dtype=np.float64).reshape(G)
    e_max = np.full(G, INF) if hi is None else np.asarray(hi, dtype=np.float64).reshape(G)
    return ru, rd, prev, e_min, e_max


def pdhg(pp, *, gen_ramp=None, gen_prev=None, gen_budget=None, line_rating=None, tol=1e-9, max_iters=200000):
    """dict(objective, dual_objective, primal_infeasibility, gap, iterations, converged, P, D, C, ramp_dual, budget_dual) of the lossless
    LP of pp (no initial levels, bands or availability) with the coupling inputs, by the iteration the device runs."""
    G, S, T, N, L = pp.G, pp.S, pp.T, pp.N, pp.L
    gn, sn = np.asarray(pp.gen_node, dtype=np.int64), np.asarray(pp.sto_node, dtype=np.int64)
    H = np.asarray(pp.ptdf, dtype=np.float64).reshape(L, N)
    dem = np.asarray(pp.demand, dtype=np.float64).reshape(N, T)
    ru, rd, prev, e_min, e_max = (a[:, None] for a in _coupling(pp, gen_ramp, gen_prev, gen_budget))
    ramp, anch, bud = has_ramp(ru, rd, prev), anchored(prev), has_budget(e_min, e_max)
    tt = np.arange(T)[None, :]
    live = ramp & ((tt >= 1) | anch)
    rlo, rhi = ramp_lo(tt, rd, prev), ramp_hi(tt, ru, prev)
    cP, cS = np.repeat(pp.gen_mc[:, None], T, 1), np.repeat(pp.sto_mc[:, None], T, 1)
    uP, uS = np.repeat(pp.gen_pmax[:, None], T, 1), np.repeat(pp.sto_pmax[:, None], T, 1)
    em = pp.sto_emax[:, None]
    absH = np.abs(H)
    w = 1.0          # the step sizes at weight 1; an iteration divides the primal ones by the current weight and multiplies the dual ones
    weight = [1.0]
    tauP = tau(absH.sum(0)[gn][:, None], ramp_rows_at(tt, T, ramp, anch), np.where(bud, 1, 0) * np.ones((1, T), dtype=np.int64), w)
    tauS = 1.0 / ((1.0 + absH.sum(0)[sn][:, None] + (T - tt)) * w)
    cnt = np.bincount(gn, minlength=N) + 2 * np.bincount(sn, minlength=N)
    sig_b = w / max(1, G + 2 * S)
    sig_f = w / np.maximum(1e-300, absH @ cnt)[:, None]
    sig_E = w / (2.0 * (tt + 1))
    sig_R, sig_Q = sigma_ramp(tt, w), sigma_budget(T, w)
    F = (np.asarray(pp.f_max, dtype=np.float64)[:, None] * np.ones((1, T)) if line_rating is None
         else np.asarray(line_rating, dtype=np.float64).reshape(L, T))
    dmax = np.abs(dem).max()

    def Kx(P, D, C):
        inj = -dem.copy()
        np.add.at(inj, gn, P)
        np.add.at(inj, sn, D - C)
        diff = np.where(tt >= 1, P - np.concatenate([np.zeros((G, 1)), P[:, :-1]], axis=1), P)
        return inj.sum(0), H @ inj, np.cumsum(C - D, axis=1), diff, P.sum(1, keepdims=True)

    def reduced(yb, yf, yE, yR, yQ):
        pi = yb[None, :] + H.T @ yf
        suf = np.cumsum(yE[:, ::-1], axis=1)[:, ::-1]
        yn = np.concatenate([yR[:, 1:], np.zeros((G, 1))], axis=1)
        return reduced_cost(cP, pi[gn], yR, yn, yQ), cS + pi[sn] - suf, cS - pi[sn] + suf

    def step(P, D, C, yb, yf, yE, yR, yQ):
        rP, rD, rC = reduced(yb, yf, yE, yR, yQ)
        wt = weight[0]
        Pn, Dn, Cn = column_step(P, tauP / wt, rP, uP), np.clip(D - tauS / wt * rD, 0, uS), np.clip(C - tauS / wt * rC, 0, uS)
        b, f, E, diff, tot = Kx(2 * Pn - P, 2 * Dn - D, 2 * Cn - C)
        sf, sE = sig_f * wt, sig_E * wt
        z = yf + sf * f
        zE = yE + sE * E
        return (Pn, Dn, Cn, yb + sig_b * wt * b, z - sf * np.clip(z / sf, -F, F), zE - sE * np.clip(zE / sE, 0.0, em),
                np.where(live, prox(yR, sig_R * wt, diff, rlo, rhi), 0.0), np.where(bud, prox(yQ, sig_Q * wt, tot, e_min, e_max), 0.0))

    def metrics(P, D, C, yb, yf, yE, yR, yQ):
        b, f, E, diff, tot = Kx(P, D, C)
        pobj = (cP * P).sum() + (cS * (D + C)).sum()
        pinf = max(np.abs(b).max(), (np.abs(f) - F).max() if L else 0.0, (-E).max() if S else 0.0, (E - em).max() if S else 0.0,
                   np.where(live, violation(diff, rlo, rhi), 0.0).max(), np.where(bud, violation(tot, e_min, e_max), 0.0).max(), 0.0)
        rP, rD, rC = reduced(yb, yf, yE, yR, yQ)
        dobj = (rc_term(rP, uP).sum() + (np.minimum(rD, 0) * uS).sum() + (np.minimum(rC, 0) * uS).sum() - (yb * dem.sum(0)).sum()
                - (np.abs(yf) * F).sum() - (yf * (H @ dem)).sum() - (np.maximum(yE, 0) * em).sum()
                + np.where(live, support(yR, rlo, rhi), 0.0).sum() + np.where(bud, support(yQ, e_min, e_max), 0.0).sum())
        return pobj, dobj, pinf, abs(pobj - dobj) / (1.0 + abs(pobj)) + pinf / (1.0 + dmax)

    x = [np.zeros((G, T)), np.zeros((S, T)), np.zeros((S, T)), np.zeros(T), np.zeros((L, T)), np.zeros((S, T)), np.zeros((G, T)),
         np.zeros((G, 1))]
    avg, navg, last_gap, it, done = [np.zeros_like(a) for a in x], 0, np.inf, 0, False
    anchor = [a.copy() for a in x]          # the last restart point
    while it < max_iters and not done:
        nb = min(200, max_iters - it)
        for _ in range(nb):
            x = list(step(*x))
            for a, b_ in zip(avg, x):
                a += b_
        it += nb
        navg += nb
        cand = [a / navg for a in avg]
        cand[0], cand[1], cand[2] = np.minimum(cand[0], uP), np.minimum(cand[1], uS), np.minimum(cand[2], uS)
        mc_, ma = metrics(*x), metrics(*cand)
        use_avg = ma[3] < mc_[3]
        best = ma if use_avg else mc_
        done = best[3] <= tol
        if done or best[3] < 0.5 * last_gap or navg >= 4000:
            if use_avg:
                x = cand
            last_gap = best[3]
            dx = np.sqrt(sum(((a - b_) ** 2).sum() for a, b_ in zip(x[:3], anchor[:3])))
            dy = np.sqrt(sum(((a - b_) ** 2).sum() for a, b_ in zip(x[3:], anchor[3:])))
            if dx > 1e-10 and dy > 1e-10:
                weight[0] = float(np.exp(0.5 * np.log(dy / dx) + 0.5 * np.log(weight[0])))
            anchor = [np.array(a, copy=True) for a in x]
            avg, navg = [np.zeros_like(a) for a in x], 0
    m = metrics(*x)
    return dict(objective=float(m[0]), dual_objective=float(m[1]), primal_infeasibility=float(m[2]), gap=float(m[3]), iterations=it,
                converged=bool(m[3] <= tol), P=x[0], D=x[1], C=x[2], ramp_dual=-x[6], budget_dual=-x[7][:, 0])


# ---- 3. the GPU tests' inputs and checks ----------------------------------------------------------------------------------------------
def draw_inputs(pp, solve):
    """The drawing rule of tests/test_gpu_central_coupled.py. solve(pp, **kw) -> host LP result (central.solve_central_packed).
    Returns dict(ramp=(up, dn), prev, budget=(e_min, e_max), rating | None)."""
    G, T, L = pp.G, pp.T, pp.L
    pmax = np.asarray(pp.gen_pmax, dtype=np.float64)
    P = solve(pp).generation
    step = np.abs(np.diff(P, axis=1)).max(axis=1) if T > 1 else np.zeros(G)
    up = np.maximum(0.1 * step, pmax / 50.0)
    dn = up.copy()
    up[::3] = dn[::3] = INF
    dn[1::6] = INF
    prev = np.maximum(P[:, 0] - 2.0 * np.where(np.isfinite(up), up, 0.0), 0.0)
    e = solve(pp, gen_ramp=(up, dn), gen_prev=prev).generation.sum(axis=1)
    e_min, e_max = np.zeros(G), np.full(G, INF)
    e_max[3::6] = np.where(e[3::6] > 0.0, 0.8 * e[3::6], INF)
    e_min[0::6] = e[0::6] + 0.2 * (T * pmax[0::6] - e[0::6])
    rating = None
    if L > 0:
        rating = np.asarray(pp.f_max, dtype=np.float64)[:, None] * np.random.default_rng(11).uniform(0.9, 1.3, (L, T))
    return dict(ramp=(up, dn), prev=prev, budget=(e_min, e_max), rating=rating)


def ramp_row_values(P, prev):
    """(G, T) values of the ramp rows: P[:, 0] (the anchor's row; it exists only with an anchor) and the differences"""
    return np.concatenate([P[:, :1], np.diff(P, axis=1)], axis=1)


def ramp_row_bounds(T, up, dn, prev):
    """((G, T) lo, (G, T) hi, (G, T) live) of the ramp rows; prev None: no anchors"""
    G = up.size
    pv = np.full(G, np.nan) if prev is None else np.asarray(prev, dtype=np.float64)
    tt = np.arange(T)[None, :]
    live = has_ramp(up, dn, pv)[:, None] & ((tt >= 1) | anchored(pv)[:, None])
    return ramp_lo(tt, dn[:, None], pv[:, None]), ramp_hi(tt, up[:, None], pv[:, None]), live


def complementarity(y_dual, value, lo, hi, live):
    """sum over rows of |y| * distance(row value, the bound y's sign names). y_dual: d objective / d right-hand side (negative: the
    upper end binds, positive: the lower end)."""
    with np.errstate(invalid="ignore"):
        dist = np.where(y_dual < 0.0, np.abs(hi - value), np.where(y_dual > 0.0, np.abs(value - lo), 0.0))
        term = np.where(live & (y_dual != 0.0), np.abs(y_dual) * dist, 0.0)
    return float(term.sum())
