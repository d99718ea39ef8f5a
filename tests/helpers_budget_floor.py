"""Helpers of the tests of must-run floors on budget contexts (dopf_set_generator_budget_min_output), CPU and GPU: the
NumPy reference of the budget row's step with the clip [floor_t, cap_t]. It is helpers_budget.budget_project with that clip: it sorts
every breakpoint of phi(nu) = sum_t x_t(nu), evaluates phi at each and solves on the one linear segment that holds the bound — no
bracket, no bisection, nothing of csrc/budget_root.h's search. For plate rows there is an independent dense QP as well (the oracle's
generic QP solver, as helpers_min_output calls it), and the one-multiplier certificate with the floors as the lower ends.

A row's step at timestep t is described as helpers_ramp_net describes it: (xk, vk, sl), the increasing piecewise-linear derivative
phi_t of the step's objective. With the multiplier nu on the budget row, x_t(nu) = clip(phi_t^{-1}(-nu), floor_t, cap_t)."""
import numpy as np

from helpers_budget import _floats, budget_violation, plate_steps
from helpers_min_output import _qp, floor_of
from helpers_ramp_net import _phi


def x_of(step, lo, cap, nu):
    """x_t(nu): the zero of phi_t + nu, clipped to [lo, cap]"""
    xk, vk, sl = step
    m = len(sl) - 1
    want = -float(nu)
    j = 0
    while j < m and vk[j] < want:
        j += 1
    a = j if j < m else (m - 1 if m > 0 else 0)
    return min(max(xk[a] + (want - vk[a]) / sl[j], float(lo)), float(cap))


def breakpoints(step, lo, cap):
    """the nu at which x_t(nu) changes its linear piece: where it reaches its floor, where it reaches cap, and phi_t's kinks between"""
    xk, vk, sl = step
    m = len(sl) - 1
    out = [-_phi(step, float(lo), 0)[0], -_phi(step, float(cap), 0)[0]]
    out += [-vk[j] for j in range(m) if lo < xk[j] < cap]
    return out


def budget_project_floor(steps, lo, cap, e_min=0.0, e_max=np.inf, info=None):
    """The row's step under lo_t <= x_t <= cap_t and e_min <= sum_t x_t <= e_max: x(0) where its sum keeps the budget, else x(nu*) with
    phi(nu*) on the broken bound. info: a dict that receives nu ("nu"), the bound met ("side": 0 free, +1 e_max, -1 e_min), whether nu
    is the only multiplier ("unique": the bound lies strictly inside phi's range and phi is strictly decreasing there), the breakpoint
    count, the sum at nu = 0 and "moved_onto_floor": some step sits on a floor > 0 at nu* and was above it at nu = 0."""
    T = len(steps)
    steps = [_floats(s) for s in steps]
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (T,))
    at = lambda nu: np.array([x_of(steps[t], lo[t], cap[t], nu) for t in range(T)])
    x0 = at(0.0)
    s0 = float(sum(x0.tolist()))
    side = 1 if s0 > e_max else -1 if s0 < e_min else 0
    nu, nb, unique = 0.0, 0, False
    if side:
        target = float(e_max if side > 0 else e_min)
        bps = sorted({b for t in range(T) for b in breakpoints(steps[t], lo[t], cap[t])})
        nb = len(bps)
        vals = [float(sum(at(b).tolist())) for b in bps]     # non-increasing along bps; added in t order, as the bounds are
        if target >= vals[0]:
            nu = bps[0]                                     # everything at its cap: the most the box gives
        elif target <= vals[-1]:
            nu = bps[-1]                                    # everything on its floor: the least the box gives
        else:
            i = 0
            while not (vals[i] >= target >= vals[i + 1]):
                i += 1
            flat = vals[i] == vals[i + 1]
            nu = bps[i] if flat else bps[i] + (vals[i] - target) * ((bps[i + 1] - bps[i]) / (vals[i] - vals[i + 1]))
            tiny = 1e-9 * max(1.0, float(np.max(cap))) * T      # (a bound within rounding of the box's own sums has no one multiplier)
            unique = not flat and vals[i] > target > vals[i + 1] and vals[-1] + tiny < target < vals[0] - tiny
    x = at(nu) if side else x0
    if info is not None:
        info["nu"], info["side"], info["breakpoints"], info["sum0"], info["unique"] = nu, side, nb, s0, unique
        info["moved_onto_floor"] = bool(side and np.any((x == lo) & (lo > 0.0) & (x0 > lo)))
    return x


def qp_plate_row(api, c, q, lo, cap, e_min, e_max):
    """A plate row as one dense QP with no search in it: min q/2 sum (x_t - c_t)^2 over lo <= x <= cap with sum x - s = 0 and the budget
    as the bounds of s"""
    c = np.asarray(c, dtype=np.float64)
    T = c.size
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (T,))
    n = T + 1
    Q = np.zeros((n, n))
    Q[np.arange(T), np.arange(T)] = q
    lin = np.concatenate([-q * c, [0.0]])
    A = np.concatenate([np.ones(T), [-1.0]])[None, :]
    lb = np.concatenate([lo, [max(float(e_min), float(lo.sum()))]])
    ub = np.concatenate([cap, [min(float(e_max), float(cap.sum()))]])
    return _qp(api, Q, lin, A, np.zeros(1), lb, ub)[:T]


def budget_kkt_violation(P, grad, lo, cap, e_min, e_max, tol=1e-9):
    """helpers_budget.budget_kkt_violation with lo_t as the lower end of step t's box: (infeasibility, stationarity, nu) — the smallest
    max-violation over ONE multiplier nu of  grad_t + nu = 0 inside the box, >= 0 on the floor, <= 0 at the cap, with nu >= 0 only
    where the sum sits on e_max, nu <= 0 only where it sits on e_min (both where they coincide), nu = 0 where on neither."""
    P, grad = np.asarray(P, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), P.shape)
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), P.shape)
    scale = max(1.0, float(np.max(cap)))
    infeas = max(float(np.max(np.maximum(P - cap, 0.0))), float(np.max(np.maximum(lo - P, 0.0))), budget_violation(P, e_min, e_max))
    at_lo, at_hi = P <= lo + tol * scale, P >= cap - tol * scale
    ge, le = ~at_hi, ~at_lo
    Lb = float(np.max(-grad[ge])) if np.any(ge) else -np.inf
    Ub = float(np.min(-grad[le])) if np.any(le) else np.inf
    s = float(np.sum(P))
    on_hi, on_lo = s >= e_max - tol * scale * P.size, s <= e_min + tol * scale * P.size
    A, B = (0.0 if not on_lo else -np.inf), (0.0 if not on_hi else np.inf)
    mid = 0.5 * (Lb + Ub) if np.isfinite(Lb) and np.isfinite(Ub) else (Lb if np.isfinite(Lb) else Ub if np.isfinite(Ub) else 0.0)
    nu = min(max(mid, A), B)
    return infeas, max(Lb - nu, nu - Ub, 0.0), nu


def stationarity_at(P, grad, lo, cap, nu, tol=1e-9):
    """the largest violation of  grad_t + nu = 0 inside the box, >= 0 on the floor, <= 0 at the cap  with nu GIVEN; a box of one point
    asks nothing"""
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), np.shape(P))
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), np.shape(P))
    scale = max(1.0, float(np.max(cap)))
    r = np.asarray(grad, dtype=np.float64) + nu
    at_lo, at_hi = P <= lo + tol * scale, P >= cap - tol * scale
    worst = 0.0
    if np.any(~at_hi):
        worst = max(worst, float(np.max(-r[~at_hi])))            # may not want to go up
    if np.any(~at_lo):
        worst = max(worst, float(np.max(r[~at_lo])))             # may not want to go down
    return max(worst, 0.0)


def budget_floor_rows(n, seed, sizes=(1, 2, 5, 64, 65, 130), pwl=False):
    """seeded rows (steps, floor, cap, e_min, e_max) in the style of helpers_budget.budget_rows, by class (k // len(sizes)) % 8: binding
    above, binding below, an equality, e_max = sum floor, e_min = sum cap, free, every box one point (p_min = pmax: must-take, the
    budget on the only sum there is), binding above with the bound a little above the floor sum (most steps end on their floors) —
    every third row with caps that drop to 0 inside the row (the floor follows them). The floors: p_min in [0.1, 0.6] pmax, every
    fifth row 0. The bounds of the binding classes lie between the floor sum and the clamped step's sum (or that and the cap sum)."""
    from helpers_ramp_net import draw_step
    rng = np.random.default_rng(seed)
    for k in range(n):
        T = int(sizes[k % len(sizes)])
        kind = (k // len(sizes)) % 8
        pm = float(rng.uniform(10.0, 100.0))
        cap = np.full(T, pm)
        if k % 3 == 0:
            cap = pm * rng.uniform(0.0, 1.0, T)
            cap[rng.random(T) < 0.25] = 0.0
        p_min = 0.0 if k % 5 == 4 else float(rng.uniform(0.1, 0.6)) * pm
        if kind == 6:
            p_min = pm
        lo = floor_of(p_min, cap)
        if pwl:
            steps = [draw_step(rng, pm, int(rng.choice([0, 1, 3, 6]))) for _ in range(T)]
        else:
            steps = plate_steps(rng.uniform(-0.5 * pm, 1.5 * pm, T), float(rng.uniform(0.5, 3.0)))
        s0 = float(sum(budget_project_floor(steps, lo, cap).tolist()))
        room, least = float(sum(cap.tolist())), float(sum(lo.tolist()))
        e_min, e_max = 0.0, np.inf
        if kind == 0:
            e_max = least + 0.6 * (s0 - least)
        elif kind == 1:
            e_min = s0 + 0.4 * (room - s0)
        elif kind == 2:
            e_min = e_max = least + 0.8 * (s0 - least)
        elif kind == 3:
            e_max = least
        elif kind == 4:
            e_min = room
        elif kind == 6:
            e_min = e_max = least
        elif kind == 7:
            e_max = least + 0.05 * (s0 - least)
        yield steps, lo, cap, e_min, e_max


# ---- the GPU tests' side ---------------------------------------------------------------------------------------------------------------

def set_floor_raw(e, p_min):
    """dopf_set_generator_budget_min_output with the array as given: (rc, message)"""
    import ctypes as C
    a = None if p_min is None else np.ascontiguousarray(p_min, dtype=np.float64)
    rc = e.api.set_generator_budget_min_output(e._ctx, None if a is None else a.ctypes.data_as(C.POINTER(C.c_double)))
    msg = e.api.last_error(e._ctx)
    return rc, (msg.decode() if msg else "")
