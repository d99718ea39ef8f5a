"""Helpers of the tests of generator energy budgets (DOPF_F2_GEN_ENERGY_BUDGET), CPU and GPU: the NumPy reference of
the budget row's step. It shares nothing with csrc/budget_root.h's search (no bracket, no bisection): it sorts every breakpoint of
phi(nu) = sum_t x_t(nu), evaluates phi at each, and solves on the one linear segment that holds the bound.

A row's step at timestep t is described as helpers_ramp_net describes it: (xk, vk, sl), the increasing piecewise-linear derivative
phi_t of the step's objective (line_step(q, c): the copper-plate step q (x - c)). With the multiplier nu on the budget row,
x_t(nu) = clip(phi_t^{-1}(-nu), 0, cap_t)."""
import numpy as np

from decentralopf_jl_amd import _capi
from helpers_ramp_net import _phi

BUDGET = getattr(_capi, "F2_GEN_ENERGY_BUDGET", 0)
CHAIN = _capi.F_NO_FUSE | _capi.F_NO_TAIL_FUSE          # the chain a budget context runs


def _floats(step):
    return tuple([float(v) for v in part] for part in step)


def x_of(step, cap, nu):
    """x_t(nu): the zero of phi_t + nu, clipped to [0, cap]"""
    xk, vk, sl = step
    m = len(sl) - 1
    want = -float(nu)
    j = 0
    while j < m and vk[j] < want:
        j += 1
    a = j if j < m else (m - 1 if m > 0 else 0)
    return min(max(xk[a] + (want - vk[a]) / sl[j], 0.0), float(cap))


def breakpoints(step, cap):
    """the nu at which x_t(nu) changes its linear piece: where it reaches 0, where it reaches cap, and phi_t's kinks between"""
    xk, vk, sl = step
    m = len(sl) - 1
    out = [-_phi(step, 0.0, 0)[0], -_phi(step, float(cap), 0)[0]]
    out += [-vk[j] for j in range(m) if 0.0 < xk[j] < cap]
    return out


def budget_project(steps, cap, e_min=0.0, e_max=np.inf, info=None):
    """The row's step under e_min <= sum_t x_t <= e_max: x(0) where its sum keeps the budget, else x(nu*) with phi(nu*) on the broken
    bound. info: a dict that receives nu ("nu"), the bound met ("side": 0 free, +1 e_max, -1 e_min) and the breakpoint count."""
    T = len(steps)
    steps = [_floats(s) for s in steps]
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), (T,))
    at = lambda nu: np.array([x_of(steps[t], cap[t], nu) for t in range(T)])
    x0 = at(0.0)
    s0 = float(np.sum(x0))
    side = 1 if s0 > e_max else -1 if s0 < e_min else 0
    nu = 0.0
    nb = 0
    if side:
        target = float(e_max if side > 0 else e_min)
        bps = sorted({b for t in range(T) for b in breakpoints(steps[t], cap[t])})
        nb = len(bps)
        vals = [float(np.sum(at(b))) for b in bps]          # non-increasing along bps
        if target >= vals[0]:
            nu = bps[0]                                     # everything at its cap: the most the box gives
        elif target <= vals[-1]:
            nu = bps[-1]                                    # everything at 0
        else:
            i = 0
            while not (vals[i] >= target >= vals[i + 1]):
                i += 1
            nu = bps[i] if vals[i] == vals[i + 1] else bps[i] + (vals[i] - target) * ((bps[i + 1] - bps[i]) / (vals[i] - vals[i + 1]))
    if info is not None:
        info["nu"], info["side"], info["breakpoints"], info["sum0"] = nu, side, nb, s0
    return at(nu) if side else x0


def plate_steps(c, q):
    """the copper-plate steps of a row: phi_t(x) = q (x - c_t)"""
    return [([float(ct)], [0.0], [float(q)]) for ct in c]


def budget_rows(n, seed, sizes=(1, 2, 5, 64, 65, 130), pwl=False):
    """seeded rows (steps, cap, e_min, e_max) by class k % 6: binding above, binding below, an equality, e_max = 0, e_min = sum cap,
    free — every third row with caps that drop to 0 inside the row; pwl: steps with 0, 1, 3 or 6 kinks (helpers_ramp_net.draw_step)"""
    from helpers_ramp_net import draw_step
    rng = np.random.default_rng(seed)
    for k in range(n):
        T = int(sizes[k % len(sizes)])
        pm = float(rng.uniform(10.0, 100.0))
        cap = np.full(T, pm)
        if k % 3 == 0:
            cap = pm * rng.uniform(0.0, 1.0, T)
            cap[rng.random(T) < 0.25] = 0.0
        if pwl:
            steps = [draw_step(rng, pm, int(rng.choice([0, 1, 3, 6]))) for _ in range(T)]
        else:
            steps = plate_steps(rng.uniform(-0.5 * pm, 1.5 * pm, T), float(rng.uniform(0.5, 3.0)))
        s0 = float(np.sum(budget_project(steps, cap)))
        room = float(np.sum(cap))
        kind = (k // len(sizes)) % 6
        lo, hi = 0.0, np.inf
        if kind == 0:
            hi = 0.6 * s0
        elif kind == 1:
            lo = s0 + 0.4 * (room - s0)
        elif kind == 2:
            lo = hi = 0.8 * s0
        elif kind == 3:
            hi = 0.0
        elif kind == 4:
            lo = room
        yield steps, cap, lo, hi


# ---- the GPU tests' side ---------------------------------------------------------------------------------------------------------------

def budget_engine(api, pp, budget=None, flags=0, **params):
    """a context with the flag of the second word; budget = (e_min, e_max): set after create (None: the setter is not called)"""
    e = _capi.Engine(api, params=_capi.default_params(flags=flags, **params), flags2=BUDGET, **pp.engine_kwargs())
    if budget is not None:
        e.set_energy_budget(*budget)
    return e


def row_sums(X):
    """the rows' sums added in t order, as the library's own check adds a row's caps (NumPy's pairwise sum may differ in the last bit,
    which matters where a budget is drawn exactly on sum_t cap)"""
    return np.array([sum(r) for r in np.asarray(X, dtype=np.float64).tolist()])


def draw_budgets(S, room):
    """(e_min, e_max) from the rows' clamped-step sums S and the sums of their caps, by row class g mod 4: free, e_max = 0.6 S,
    e_min = S + 0.4 (room - S), equality at 0.8 S"""
    S, room = np.asarray(S, dtype=np.float64), np.asarray(room, dtype=np.float64)
    lo, hi = np.zeros(S.size), np.full(S.size, np.inf)
    g = np.arange(S.size)
    hi[g % 4 == 1] = 0.6 * S[g % 4 == 1]
    lo[g % 4 == 2] = (S + 0.4 * (room - S))[g % 4 == 2]
    lo[g % 4 == 3] = hi[g % 4 == 3] = 0.8 * S[g % 4 == 3]
    return lo, hi


def draw_budgets_by_state(S, room):
    """(e_min, e_max, classes) with each row's class chosen from its own state, so that the shares hold whatever the state is: a row can
    bind above (e_max = 0.6 S) only with S > 0, below (e_min = S + 0.4 (room - S)) only with S < room, and be an equality (0.8 S, which
    binds above) only with S > 0; a row whose box is one point can only be free. Rows are taken in order and get, of the classes
    open to them, the one with the fewest rows so far (ties: above, below, free, equality)."""
    S, room = np.asarray(S, dtype=np.float64), np.asarray(room, dtype=np.float64)
    lo, hi = np.zeros(S.size), np.full(S.size, np.inf)
    count = {"above": 0, "below": 0, "free": 0, "equality": 0}
    classes = []
    for g in range(S.size):
        tiny = 1e-6 * max(1.0, float(room[g]))
        can = [k for k in count if k == "free" or (k == "below" and S[g] < room[g] - tiny) or (k in ("above", "equality") and S[g] > tiny)]
        k = min(can, key=lambda name: count[name])
        count[k] += 1
        classes.append(k)
        if k == "above":
            hi[g] = 0.6 * S[g]
        elif k == "below":
            lo[g] = S[g] + 0.4 * (room[g] - S[g])
        elif k == "equality":
            lo[g] = hi[g] = 0.8 * S[g]
    return lo, hi, classes


def budget_violation(P, e_min, e_max):
    s = float(np.sum(P))
    return max(0.0, s - e_max, e_min - s)


def budget_kkt_violation(P, grad, cap, e_min, e_max, tol=1e-9):
    """(infeasibility, stationarity, nu) of a row at P under box and budget, with the gradient grad of its step objective at P: the
    smallest max-violation over ONE multiplier nu of  grad_t + nu = 0 inside the box, >= 0 at 0, <= 0 at the cap, with nu >= 0 only
    where the sum sits on e_max, nu <= 0 only where it sits on e_min (both where they coincide), nu = 0 where on neither."""
    P, grad = np.asarray(P, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    cap = np.broadcast_to(np.asarray(cap, dtype=np.float64), P.shape)
    scale = max(1.0, float(np.max(cap)))
    infeas = max(float(np.max(np.maximum(P - cap, 0.0))), float(np.max(np.maximum(-P, 0.0))), budget_violation(P, e_min, e_max))
    at_lo, at_hi = P <= tol * scale, P >= cap - tol * scale
    # at 0: grad + nu >= 0 (nu >= -grad); at the cap: grad + nu <= 0 (nu <= -grad); inside: both; a box of one point asks nothing
    ge, le = ~at_hi, ~at_lo
    Lb = float(np.max(-grad[ge])) if np.any(ge) else -np.inf
    Ub = float(np.min(-grad[le])) if np.any(le) else np.inf
    s = float(np.sum(P))
    on_hi, on_lo = s >= e_max - tol * scale * P.size, s <= e_min + tol * scale * P.size
    A, B = (0.0 if not on_lo else -np.inf), (0.0 if not on_hi else np.inf)
    mid = 0.5 * (Lb + Ub) if np.isfinite(Lb) and np.isfinite(Ub) else (Lb if np.isfinite(Lb) else Ub if np.isfinite(Ub) else 0.0)
    nu = min(max(mid, A), B)
    return infeas, max(Lb - nu, nu - Ub, 0.0), nu


def stationarity_at(P, grad, cap, nu, tol=1e-9):
    """the largest violation of  grad_t + nu = 0 inside the box, >= 0 at 0, <= 0 at the cap  with nu GIVEN (helpers_budget's
    budget_kkt_violation fits a nu; this one does not); a box of one point asks nothing"""
    scale = max(1.0, float(np.max(cap)))
    r = np.asarray(grad, dtype=np.float64) + nu
    at_lo, at_hi = P <= tol * scale, P >= cap - tol * scale
    worst = 0.0
    if np.any(~at_hi):
        worst = max(worst, float(np.max(-r[~at_hi])))            # may not want to go up
    if np.any(~at_lo):
        worst = max(worst, float(np.max(r[~at_lo])))             # may not want to go down
    return max(worst, 0.0)


# ---- budgets per sub-window ---------------------------------------------------------------------------------------------------------------

def _slices(ends):
    return [slice(0 if j == 0 else ends[j - 1], ends[j]) for j in range(len(ends))]


def _unit_budgets(pp, steps, cap, ends):
    """(e_min, e_max) of shape (G, n_win): every (row, window) unit's class dealt by draw_budgets_by_state from the unit's own clamped-step
    sum and cap sum (both added in t order). Two deals are formed — one over all units, rows outermost, and one window by window — and
    the one whose smallest class (binding above, binding below, free: by the reference alone) is larger is taken. Neither serves every
    shape: one deal over six units gives 3xT600 a single free unit whatever the state, and window by window the one-step windows of 7x5
    leave six of 35 units to bind below (the CPU oracle's warm-up state gives the same counts as the device's)"""
    sl = _slices(ends)
    x0 = [budget_project(steps[g], cap[g]) for g in range(pp.G)]
    S = np.array([[row_sums([x0[g][s]])[0] for s in sl] for g in range(pp.G)])
    room = np.array([[row_sums([cap[g][s]])[0] for s in sl] for g in range(pp.G)])
    lo, hi, _ = draw_budgets_by_state(S.ravel(), room.ravel())
    deals = [(lo.reshape(S.shape), hi.reshape(S.shape)), (np.zeros(S.shape), np.full(S.shape, np.inf))]
    for j in range(len(ends)):
        deals[1][0][:, j], deals[1][1][:, j], _ = draw_budgets_by_state(S[:, j], room[:, j])

    def smallest_class(deal):
        sides = []
        for g in range(pp.G):
            for j, s in enumerate(sl):
                info = {}
                budget_project(steps[g][s], cap[g][s], deal[0][g, j], deal[1][g, j], info)
                sides.append(info["side"])
        return min(sides.count(k) for k in (1, -1, 0))
    return max(deals, key=smallest_class)
