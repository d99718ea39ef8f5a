"""Helpers of the tests of ramp limits and energy budgets on the same generators (DOPF_F2_GEN_RAMP_BUDGET), CPU and
GPU: the value reference of the step (a bisection on the budget's multiplier over helpers_ramp.ramp_project), the extreme feasible
paths of a row, and the draws the tests share."""
import numpy as np

from decentralopf_jl_amd import _capi
from helpers_ramp import ramp_active, ramp_project

RAMP = _capi.F_GEN_RAMP
BUDGET = _capi.F2_GEN_ENERGY_BUDGET
PAIR = getattr(_capi, "F2_GEN_RAMP_BUDGET", 0)
HOST_T = (1, 2, 5, 24, 64, 65, 130)


def extreme_paths(cap, up, down, prev=None):
    """(lo, hi): the pointwise-smallest and pointwise-largest paths under caps, ramps and anchor, by the rule of the setters' joint
    check — forward, then backward. The feasible paths form a lattice: both are feasible where any path is (lo <= hi everywhere)."""
    cap = np.asarray(cap, dtype=np.float64)
    T = cap.size
    hi, lo = np.zeros(T), np.zeros(T)
    for t in range(T):
        if t == 0:
            hi[0] = cap[0] if prev is None else min(cap[0], prev + up)
            lo[0] = 0.0 if prev is None else max(0.0, prev - down)
        else:
            hi[t] = min(cap[t], hi[t - 1] + up)
            lo[t] = max(0.0, lo[t - 1] - down)
    for t in range(T - 2, -1, -1):
        hi[t] = min(hi[t], hi[t + 1] + down)
        lo[t] = max(lo[t], lo[t + 1] - up)
    return lo, hi


def path_sum(x):
    """a row's sum in t order (the setters' order)"""
    s = 0.0
    for v in np.asarray(x, dtype=np.float64):
        s += float(v)
    return s


def ramp_budget_project(c, q, cap, up, down, prev=None, e_min=0.0, e_max=np.inf, info=None):
    """The minimiser of q / 2 |x - c|^2 over the box, the ramps (anchor included) and e_min <= sum x <= e_max: x(nu) =
    ramp_project(c - nu / q, ...) with nu bisected until no double is left between the two ends that bracket the broken bound, then
    interpolated between them. info (a dict) receives nu, side (+1: e_max binds, -1: e_min, 0: neither) and evals."""
    c = np.asarray(c, dtype=np.float64)
    T = c.size
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    x_at = lambda nu: ramp_project(c - nu / q, q, cap, up, down, prev)
    x0 = x_at(0.0)
    s0 = float(x0.sum())
    info = {} if info is None else info
    info.update(nu=0.0, side=0, evals=1)
    if e_min <= s0 <= e_max:
        return x0
    side = 1 if s0 > e_max else -1
    target = e_max if side > 0 else e_min
    beyond = (lambda f: f > target) if side > 0 else (lambda f: f < target)
    a, xa, b = 0.0, x0, side * max(abs(s0 - target) * q / T, 1e-12)
    for _ in range(1100):
        xb = x_at(b)
        info["evals"] += 1
        if not beyond(float(xb.sum())):
            break
        a, xa, b = b, xb, 2.0 * b
    else:
        raise AssertionError("the bound is out of reach")
    while True:
        m = a + 0.5 * (b - a)
        if m == a or m == b:
            break
        xm = x_at(m)
        info["evals"] += 1
        if beyond(float(xm.sum())):
            a, xa = m, xm
        else:
            b, xb = m, xm
    fa, fb = float(xa.sum()), float(xb.sum())
    th = 1.0 if fa == fb else min(max((fa - target) / (fa - fb), 0.0), 1.0)
    info.update(nu=a + th * (b - a), side=side)
    return xa + th * (xb - xa)


def draw_row(rng, T, k, pm=None):
    """Row k of a seeded draw: (c, q, cap, up, down, prev, e_min, e_max, pm). Ramps 2-30 % of pmax, every other row anchored, every
    third with caps 0.2-1.0 of pmax; centres that swing across the box, so that ramps bind; e_max between the smallest feasible sum
    and the ramp-only step's sum (even k // 2), or e_min between that sum and the largest feasible sum."""
    pm = float(rng.uniform(20.0, 400.0)) if pm is None else float(pm)
    cap = pm * rng.uniform(0.2, 1.0, T) if k % 3 == 0 else np.full(T, pm)
    up, down, prev = draw_limits(rng, k, cap, pm)
    q = float(rng.uniform(1.0, 2.0))
    c = pm * (0.5 + 0.9 * np.where(np.arange(T) % 2 == 0, -1.0, 1.0) * rng.uniform(0.2, 1.0, T) + rng.uniform(-0.2, 0.2))
    e_min, e_max = draw_budget(rng, k, c, q, cap, up, down, prev)
    return c, q, cap, up, down, prev, e_min, e_max, pm


def draw_limits(rng, k, cap, pm, anchored=None):
    """(up, down, prev) of row k under its caps: ramps 2-30 % of pmax, even rows (anchored: every row, or none) anchored at a point
    under cap[0] from which the row has a path (drawn again until it has)"""
    while True:
        up, down = (float(v) for v in rng.uniform(0.02, 0.30, 2) * pm)
        prev = float(rng.uniform(0.0, 1.0) * cap[0]) if (k % 2 == 0 if anchored is None else anchored) else None
        lo, hi = extreme_paths(cap, up, down, prev)
        if np.all(lo <= hi):
            return up, down, prev


def draw_budget(rng, k, c, q, cap, up, down, prev, exact=False):
    """(e_min, e_max) of row k from the sum s of its ramp-only step: e_max between the smallest feasible sum and s (k // 2 even), or
    e_min between s and the largest feasible sum; the other kind where s sits on that end already, none where both ends are one. exact: the bound is the extreme
    sum itself (the row's only feasible path: where one timestep leaves no other way for ramp and budget to bind together)"""
    lo, hi = extreme_paths(cap, up, down, prev)
    s = float(ramp_project(c, q, cap, up, down, prev).sum())
    slo, shi = path_sum(lo), path_sum(hi)
    th = 0.0 if exact else float(rng.uniform(0.2, 0.8))
    # (a step within a thousandth of an end sits on it: a bound drawn in the rounding of two sums would be out of reach)
    at_lo, at_hi = s - slo <= 1e-3 * (shi - slo), shi - s <= 1e-3 * (shi - slo)
    if ((k // 2) % 2 == 0 or at_hi) and not at_lo:
        return 0.0, slo + th * (s - slo)
    if not at_hi:
        return shi - th * (shi - s), np.inf
    return 0.0, np.inf


def host_rows(seed=41, per_T=12):
    rng = np.random.default_rng(seed)
    return [draw_row(rng, T, k) for T in HOST_T for k in range(per_T)]


def both_bind(x, up, down, prev, info):
    """the reference's row has a tight ramp and a multiplier on its budget"""
    return bool(info["nu"] != 0.0 and ramp_active(x, up, down, prev))
