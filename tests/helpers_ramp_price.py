"""Helpers of the ramp-price tests (dopf_get_generator_ramp_price), CPU and GPU: the NumPy twin of csrc/ramp_price.h,
statement by statement; a certificate for a vector of ramp multipliers that shares nothing with the pass but the optimality system;
the duals of the dense QP of helpers_min_output.qp_row (the oracle's generic solver); and seeded rows."""
import ctypes as C

import numpy as np

from helpers_min_output import draw_row, floor_of, qp_row, ramp_project_floor

INF = float("inf")


def _min(a, b):
    return a if a < b else b


def _max(a, b):
    return a if a > b else b


def _near(il, ih, sl, sh):
    """rp_near: I ∩ S, or the end of S nearest to I"""
    l, h = _max(il, sl), _min(ih, sh)
    if l <= h:
        return l, h
    if ih < sl:
        return sl, sl
    return sh, sh


def ramp_multipliers(x, c, q, floor, cap, up, down, prev=None, pm=None, shift=0.0):
    """ramp_price of csrc/ramp_price.h in Python floats (IEEE doubles, no contraction): a[t], the multiplier of the ramp row between
    t-1 and t (t = 0: the anchor's). up, down: the stored ramps (inf allowed); pm: gen_pmax (None: the largest cap)."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    T = x.size
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    floor = np.broadcast_to(np.asarray(floor, dtype=np.float64), (T,))
    q, up, down, shift = float(q), float(up), float(down), float(shift)
    pm = float(cap.max()) if pm is None else float(pm)
    tol = pm * 2.0 ** -40
    lo, hi = [0.0] * T, [0.0] * T
    al = ah = 0.0
    for t in range(T):
        xt = float(x[t])
        before = float(x[t - 1]) if t else (None if prev is None or prev != prev else float(prev))
        sl = sh = 0.0
        if before is not None:
            if before - xt >= down - tol:
                sl = -INF
            if xt - before >= up - tol:
                sh = INF
        if t == 0:
            al, ah = sl, sh
        else:
            al, ah = _near(al, ah, sl, sh)
        lo[t], hi[t] = al, ah
        g = q * (xt - (float(c[t]) - shift))
        bl = -INF if xt <= float(floor[t]) + tol else 0.0
        bh = INF if xt >= float(cap[t]) - tol else 0.0
        al = (al + g) + bl
        ah = (ah + g) + bh
    a = np.zeros(T)
    an = 0.0
    for t in range(T - 1, -1, -1):
        xt = float(x[t])
        g = q * (xt - (float(c[t]) - shift))
        bl = -INF if xt <= float(floor[t]) + tol else 0.0
        bh = INF if xt >= float(cap[t]) - tol else 0.0
        l, h = _near((an - g) - bh, (an - g) - bl, lo[t], hi[t])
        an = _min(_max(0.0, l), h)
        a[t] = an
    return a


def ramp_price_violation(x, c, q, floor, cap, up, down, prev, a, shift=0.0, rel=1e-9):
    """The certificate: the largest breach, in units of q max(1, max cap), of
      - stationarity with a correctly signed box multiplier: b_t = a_{t+1} - a_t - q (x_t - c_t + shift), a_T = 0, must be >= 0 at the
        cap alone, <= 0 at the floor alone, 0 inside, free where both ends are touched;
      - the signs of a_t: >= 0 where ramp-up alone is tight, <= 0 where ramp-down alone is, free where both are;
      - a_t = 0 off tight rows (and at t = 0 without an anchor).
    "Tight" and "at" are taken within rel max(1, max cap): the one-step bound, which the pass's own tolerance stays below."""
    x, c, a = (np.asarray(v, dtype=np.float64) for v in (x, c, a))
    T = x.size
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    floor = np.broadcast_to(np.asarray(floor, dtype=np.float64), (T,))
    size = max(1.0, float(cap.max()))
    tol = rel * size
    nxt = np.concatenate([a[1:], [0.0]])
    b = nxt - a - float(q) * (x - (c - shift))
    at_cap, at_floor = x >= cap - tol, x <= floor + tol
    worst = 0.0
    for t in range(T):
        if at_cap[t] and at_floor[t]:
            v = 0.0
        elif at_cap[t]:
            v = max(0.0, -b[t])
        elif at_floor[t]:
            v = max(0.0, b[t])
        else:
            v = abs(b[t])
        before = x[t - 1] if t else (None if prev is None or prev != prev else float(prev))
        tu = before is not None and x[t] - before >= up - tol
        td = before is not None and before - x[t] >= down - tol
        if tu and td:
            s = 0.0
        elif tu:
            s = max(0.0, -a[t])
        elif td:
            s = max(0.0, a[t])
        else:
            s = abs(a[t])
        worst = max(worst, v, s)
    return worst / (float(q) * size)


def tied(x, floor, cap, up, down, prev, rel=1e-9):
    """a step sits on a box end and a ramp reach at once (the multipliers need not be unique there); the ramps as the programme and
    the QP cap them (at the largest cap, or the anchor where that is larger)"""
    x = np.asarray(x, dtype=np.float64)
    T = x.size
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    floor = np.broadcast_to(np.asarray(floor, dtype=np.float64), (T,))
    pm = float(cap.max()) if prev is None else max(float(cap.max()), float(prev))
    up, down = min(float(up), pm), min(float(down), pm)
    tol = rel * max(1.0, float(cap.max()))
    box = (x >= cap - tol) | (x <= floor + tol)
    d = np.diff(x) if prev is None else np.diff(np.concatenate([[prev], x]))
    reach = (d >= up - tol) | (-d >= down - tol)
    reach = np.concatenate([[False], reach]) if prev is None else reach
    touch = reach.copy()                                        # a tight row touches both of its steps
    touch[:-1] |= reach[1:]
    return bool(np.any(box & touch))


class _Spy:
    """the API with qp_solve's y kept: qp_row drops it"""

    def __init__(self, api):
        self.api, self.y = api, None

    def qp_solve(self, n, m, *args):
        rc = self.api.qp_solve(n, m, *args)
        self.y = np.ctypeslib.as_array(args[7], shape=(max(m, 1),))[:m].copy()
        return rc


def qp_ramp_duals(api, steps, lo, cap, up, down, prev=None):
    """(x, y) of helpers_min_output.qp_row: y[t] the solver's multiplier of the equality x_t - x_{t-1} - s_t = 0 (T values; y[0] = 0
    without an anchor, which has no such row). The sign against a_t is settled by the tests' hand case."""
    spy = _Spy(api)
    x = qp_row(spy, steps, lo, cap, up, down, prev)
    y = np.asarray(spy.y, dtype=np.float64)
    return x, (y if prev is not None else np.concatenate([[0.0], y]))


def long_rows(T, n, seed):
    """seeded rows (c, q, lo, cap, up, down, prev) at one T (the GPU kernels' horizons: 64, 65, 130), helpers_min_output.draw_row's
    boxes and ramps with centres that swing"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        p_min, cap, up, down, prev = draw_row(rng, k, T)
        q = float(rng.uniform(0.5, 3.0))
        pm = float(cap.max())
        c = rng.uniform(-0.5 * pm, 1.5 * pm, T)
        yield c, q, floor_of(p_min, cap), cap, up, down, prev


def priced_row(row):
    """(x, a) of a seeded row: the twin's projection and the twin's prices"""
    c, q, lo, cap, up, down, prev = row
    x = ramp_project_floor(c, q, lo, cap, up, down, prev)
    return x, ramp_multipliers(x, c, q, lo, cap, up, down, prev)


# ---- the GPU tests' plates: what a step prices, known without a device ------------------------------------------------------------------

def drawn_before(d):
    """the drawn state of helpers_min_output.plate_draw as helpers_ramp.step_centres takes it (the storages rest: the injections' sum
    is the generators' less the demand)"""
    pp, st = d["pp"], d["st"]
    s = st["P"].sum(axis=0) - np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T).sum(axis=0)
    return dict(P=st["P"], lam=st["lam"], inj=s[None, :])


def plate_prices(d, floors, before, P=None, shift=None):
    """per row of a drawn plate (x, a, c, q, lo, shift): the twin's prices of the rows P (None: of the twin's own projection of the step's
    centres from `before`); floors: the drawn p_min apply (else 0); shift: per row (the pair's nu / q), None = 0"""
    from helpers_ramp import step_centres
    pp = d["pp"]
    c, q = step_centres(pp, d["c2"], before, d["prm"]["gamma"])
    out = []
    for g in range(pp.G):
        lo = floor_of(d["p_min"][g] if floors else 0.0, d["cap"][g])
        pv = None if d["prev"] is None else float(d["prev"][g])
        sh = 0.0 if shift is None else float(shift[g])
        x = ramp_project_floor(c[g] - sh, q[g], lo, d["cap"][g], d["up"][g], d["down"][g], pv) if P is None else np.asarray(P[g])
        a = ramp_multipliers(x, c[g], q[g], lo, d["cap"][g], d["up"][g], d["down"][g], pv, pm=float(pp.gen_pmax[g]), shift=sh)
        out.append((x, a, c[g], float(q[g]), lo, sh))
    return out


def coverage(rows):
    """(rows with a price, some a > 0, some a < 0)"""
    return (sum(bool(np.any(r[1] != 0.0)) for r in rows), any(bool(np.any(r[1] > 0.0)) for r in rows),
            any(bool(np.any(r[1] < 0.0)) for r in rows))


def price_plate(name, quad, seed, avail=False):
    """helpers_min_output.plate_draw, with one change on the plates of three generators ("3x70", "3x130"): there the draw leaves ONE row
    with finite ramps above 0 — row 0 is every fifth (unlimited), row 2 the one at 0 — and with c2 that row's coefficient is the
    draw's 50, which flattens its centres: it comes down from its anchor and never meets ramp-up, so no seed gives both signs. Row 0,
    the cheap unit that follows the swinging price, gets ramps of 10 % of its capacity in every variant (it has no profile and its
    anchor lies in its box: a path exists)."""
    from helpers_min_output import path_exists, plate_draw
    d = plate_draw(name, quad, seed, avail)
    pp = d["pp"]
    if pp.G == 3:
        d["up"][0] = d["down"][0] = 0.1 * float(pp.gen_pmax[0])
        assert path_exists(floor_of(d["p_min"][0], d["cap"][0]), d["cap"][0], d["up"][0], d["down"][0], float(d["prev"][0])) is None
    return d
