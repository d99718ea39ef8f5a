"""dopf_roll_horizon_coupled / dopf_get_generator_coupling on the GPU: contexts with ramp limits, energy budgets or both
roll in place. Per case: (1) the moved arrays are horizon.shift_window of what the getters returned before, and the anchor and the
budgets horizon.shift_coupled of them, bit for bit; (2) the context then behaves like a second one that took Engine.roll's host route
(a new context of the next window: the definition of the rule) — tolerances those of tests/test_gpu_horizon_roll.py, "same state,
node sums formed in another order": one step 1e-9 on copper plates, 1e-8 on networks, twelve steps 1e-8 / 1e-7, cost 1e-9 / 1e-8;
(3) the next iteration keeps the ramps against the old P[:, k-1] and the new budgets. Then the refusals (which leave every getter
as it was), the graphs, three rolls in a row and the debug allocator. Needs a real MI355X: pytest -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

from decentralopf_jl_amd import _capi, shift_coupled, shift_window, synth
from helpers import max_diff, set_from, state_of
from helpers_budget import draw_budgets, row_sums
from helpers_ramp_budget import extreme_paths, path_sum

pytestmark = pytest.mark.gpu

IL, AV, QC = _capi.F_STO_INITIAL_LEVEL, _capi.F_GEN_AVAILABILITY, _capi.F_GEN_QUADRATIC_COST
RAMP, RAMP_NET = _capi.F_GEN_RAMP, _capi.F_GEN_RAMP_NETWORK
BUDGET, PAIR = _capi.F2_GEN_ENERGY_BUDGET, _capi.F2_GEN_RAMP_BUDGET
E_INVALID, E_UNSUPPORTED = -1, -4
MOVED = ("P", "D", "C", "lam", "mu", "rho", "avg_U", "avg_K")
COUPLING = ("ramp_up", "ramp_down", "p_prev", "e_min", "e_max")


# ---- the cases and helpers of tests/test_gpu_horizon_roll.py (copied) ------------------------------------------------------------------

def copper(T, G=40, S=12, seed=801):
    return synth.synthetic_case(G, S, T, seed=seed)


def network(T, seed=802):
    return synth.synthetic_case(30, 10, T, N=6, L=8, seed=seed, fmax_factor=0.7, fmax_min=5)


def kw_of(pp):
    return dict(eps=0.0, gamma=0.02) if pp.L == 0 else dict(eps=0.0, gamma=0.03)


def tail_of(pp, k):
    """the demand of the k new steps: the window's first k steps again, a little higher (integers, like the case's own)"""
    return np.round(pp.demand[:, :k] * 1.05) + 1.0


def scaled(sa, sb):
    scale = max(1.0, float(np.abs(sb["lam"]).max()))
    worst, where = max_diff(sa, sb, keys=[k for k in sa if k != "cost"])
    cost = abs(float(sa["cost"][0] - sb["cost"][0])) / max(1.0, abs(float(sb["cost"][0])))
    return worst / scale, where, cost


def full_state(e):
    """every getter, the new one included"""
    s = state_of(e)
    lu, mu_u, ru = e.get_duals_used()
    s.update(lam_used=lu, mu_used=mu_u, rho_used=ru, price0=e.get_nodal_price(0), price1=e.get_nodal_price(1),
             res=np.asarray(e.get_residuals(), dtype=np.float64), sync=np.asarray(e.sync(), dtype=np.float64))
    s.update(e.generator_coupling())
    return s


def same_bits(a, b, keys=None):
    for k in (keys or a.keys()):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- building a coupled context ----------------------------------------------------------------------------------------------------

def draw_ramps(pp, seed):
    """ramps at 10-15 % of gen_pmax"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.10, 0.15, pp.G) * pp.gen_pmax, rng.uniform(0.10, 0.15, pp.G) * pp.gen_pmax


def build(api, pp, flags, flags2, ramp=None, budget=None, prof=None, c2=None, extra=0):
    e = _capi.Engine(api, params=_capi.default_params(flags=IL | flags | extra, **kw_of(pp)), flags2=flags2, **pp.engine_kwargs())
    e.set_initial_levels(np.zeros(pp.S))
    if prof is not None:
        e.set_availability(*prof)
    if c2 is not None:
        e.set_quadratic_cost(c2)
    if ramp is not None:
        e.set_ramp(*ramp)
    if budget is not None:
        e.set_energy_budget(*budget)
    return e


def budgets_for(api, pp, flags, flags2, ramp, widen=1.0):
    """as tests/test_gpu_gen_budget.py draws them: helpers_budget.draw_budgets on the row sums of a warm state (4 iterations of the
    same context with its budgets at their defaults) and the sums of the caps; widen: every finite e_max times it"""
    warm = build(api, pp, flags, flags2, ramp)
    warm.iterate(4)
    lo, hi = draw_budgets(row_sums(warm.get_primal()[0]), row_sums(np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)))
    warm.close()
    return lo, np.where(np.isfinite(hi), hi * widen, hi)


def rows_fit(pp, up, down, prev, lo, hi, cap=None):
    """the joint check of DOPF_F2_GEN_RAMP_BUDGET (ramp_budget_fits) in NumPy: the rows that have a path under caps, ramps and anchor
    whose sum meets the budget — lo_t <= hi_t, e_min <= sum hi_t, sum lo_t <= e_max"""
    ok = np.zeros(pp.G, dtype=bool)
    for g in range(pp.G):
        c = np.full(pp.T, pp.gen_pmax[g]) if cap is None else cap[g]
        plo, phi = extreme_paths(c, up[g], down[g], None if np.isnan(prev[g]) else float(prev[g]))
        ok[g] = bool(np.all(plo <= phi)) and lo[g] <= path_sum(phi) and path_sum(plo) <= hi[g]
    return ok


def coupled_case(api, pp, flags, flags2, k, prof=None, new_prof=None, c2=None):
    ramp = draw_ramps(pp, 31) if flags & RAMP else None
    has_budget, pair = bool(flags2 & BUDGET), bool(flags2 & PAIR)
    one, many = (1e-9, 1e-8) if pp.L == 0 else (1e-8, 1e-7)
    widen = 1.0
    while True:
        budget = budgets_for(api, pp, flags, flags2, ramp, widen) if has_budget else None
        h = build(api, pp, flags, flags2, ramp, budget, prof, c2)
        h.iterate(7)
        before = full_state(h)
        want = shift_coupled(k, before["P"], budget=(before["e_min"], before["e_max"]) if has_budget else None)
        if not pair:
            break
        # the pair's precondition: the roll is admissible — every row of the next window is jointly feasible under the new anchor
        # and what is left of its budgets (the lattice rule, evaluated here before the call). Where it is not, e_max is drawn wider
        # (x 1.5 per round) and the case starts over, so that a refusal by the library is a failure of the library, not of the draw.
        # Needed on an MI355X: no widening at k = 1 and k = 5 (printed below).
        fit = rows_fit(pp, before["ramp_up"], before["ramp_down"], want["gen_prev"], *want["gen_budget"])
        print(f"pair k={k}: e_max x {widen}: {int(fit.sum())}/{pp.G} rows of the next window jointly feasible")
        if fit.all():
            break
        h.close()
        widen *= 1.5
        assert widen < 20.0, "no admissible draw"
    assert h.solver_failures() == 0
    ref = build(api, pp, flags, flags2, ramp, budget, prof, c2)
    ref.iterate(7)
    same_bits(before, full_state(ref))
    tail = tail_of(pp, k)
    w = shift_window(k, tail, demand=pp.demand, sto_emax=pp.sto_emax, E=before["E"], **{n: before[n] for n in MOVED},
                     used=dict(lam=before["lam_used"], mu=before["mu_used"], rho=before["rho_used"]))
    h.roll_coupled(k, tail, availability=new_prof)
    after = full_state(h)
    # (1) bits
    assert after["res"][3] == 2 and after["sync"].tolist() == [2.0, 0.0]
    same_bits(after, w, MOVED)
    for n in ("lam", "mu", "rho"):
        assert np.array_equal(after[n + "_used"], w["used"][n]), n
    assert np.array_equal(h.demand(), w["demand"])
    same_bits(after, before, ("ramp_up", "ramp_down"))
    if flags & RAMP:
        assert np.array_equal(after["p_prev"], want["gen_prev"]) and np.array_equal(h._mirror["gen_prev"], want["gen_prev"])
        assert np.all(np.isnan(before["p_prev"]))                   # (no anchor was stored before)
    else:
        assert np.all(np.isnan(after["p_prev"]))
    if has_budget:
        assert np.array_equal(after["e_min"], want["gen_budget"][0]) and np.array_equal(after["e_max"], want["gen_budget"][1])
        assert np.array_equal(h._mirror["gen_budget"][1], want["gen_budget"][1])
    else:
        assert np.all(after["e_min"] == 0.0) and np.all(after["e_max"] == np.inf)
    # (2) the reference route: Engine.roll rebuilds the next window's context on the host
    if new_prof is not None:
        ref._mirror.update(gen_avail=np.asarray(new_prof[0], dtype=np.float64), gen_avail_of=np.asarray(new_prof[1], dtype=np.int32))
    ref.roll(k, tail)
    d, where, _ = scaled(state_of(h), state_of(ref))
    print(f"after the roll vs the host route: {d:.2e} ({where})")
    assert d <= one, (where, d)
    h.iterate(1)
    ref.iterate(1)
    d, where, cost = scaled(state_of(h), state_of(ref))
    print(f"one iteration vs the host route: {d:.2e} ({where}), cost {cost:.2e}")
    assert d <= one and cost <= 1e-9, (where, d, cost)
    # (3) the constraints of the new window in the first iteration
    P1 = h.get_primal()[0]
    tol = 1e-9 * float(pp.gen_pmax.max())
    if flags & RAMP:
        step = P1[:, 0] - before["P"][:, k - 1]
        assert np.all(step <= after["ramp_up"] + tol) and np.all(-step <= after["ramp_down"] + tol), (float(step.max()), float(step.min()))
    if has_budget:
        sums = P1.sum(axis=1)
        assert np.all(sums >= after["e_min"] - tol) and np.all(sums <= after["e_max"] + tol), float(np.max(np.maximum(after["e_min"] - sums, sums - after["e_max"])))
    h.iterate(11)
    ref.iterate(11)
    d, where, cost = scaled(state_of(h), state_of(ref))
    print(f"12 iterations vs the host route: {d:.2e} ({where}), cost {cost:.2e}")
    assert d <= many and cost <= 1e-8, (where, d, cost)
    assert h.solver_failures() == 0
    return h


GRID = [
    ("copper-ramp-T24-k1", lambda: copper(24), RAMP, 0, 1),
    ("copper-ramp-T24-k5", lambda: copper(24), RAMP, 0, 5),
    ("copper-ramp-T24-k23", lambda: copper(24), RAMP, 0, 23),
    ("copper-ramp-T100-k37", lambda: copper(100), RAMP, 0, 37),
    ("copper-ramp-G300-k5", lambda: copper(24, G=300), RAMP, 0, 5),          # the generators cross a 256-thread block
    ("net-ramp-k1", lambda: network(12), RAMP | RAMP_NET, 0, 1),
    ("net-ramp-k7", lambda: network(12), RAMP | RAMP_NET, 0, 7),
    ("copper-budget-k1", lambda: copper(24), 0, BUDGET, 1),
    ("copper-budget-k5", lambda: copper(24), 0, BUDGET, 5),
    ("copper-budget-k23", lambda: copper(24), 0, BUDGET, 23),
    ("net-budget-k7", lambda: network(12), 0, BUDGET, 7),
    ("pair-T41-k1", lambda: copper(41), RAMP, BUDGET | PAIR, 1),
    ("pair-T41-k5", lambda: copper(41), RAMP, BUDGET | PAIR, 5),
]


@pytest.mark.parametrize("name,case,flags,flags2,k", GRID, ids=[g[0] for g in GRID])
def test_roll_coupled_on_every_context(hip_api, name, case, flags, flags2, k):
    coupled_case(hip_api, case(), flags, flags2, k)


def test_roll_coupled_with_a_new_availability_table(hip_api):
    """copper ramp + availability + quadratic costs, the new window's table handed to the roll: the stored one moved by k. The
    profiles are a day's sine, 0.6 + 0.3 sin(2 pi (t + 3 j) / T): a cap moves by less than 8 % of gen_pmax per step, under every
    ramp_down (10 % and more), so the new anchor can come down under the new window's caps — under a table of independent draws it
    cannot, and the library rightly refuses such a window."""
    pp = copper(24)
    k = 5
    rng = np.random.default_rng(803)
    t = np.arange(pp.T)
    prof = np.round((0.6 + 0.3 * np.sin(2.0 * np.pi * (t[None, :] + 3.0 * np.arange(2)[:, None]) / pp.T)) * 1024.0) / 1024.0
    of = (np.arange(pp.G) % 3 - 1).astype(np.int32)             # -1, 0, 1, ...
    moved = np.concatenate([prof[:, k:], prof[:, :k]], axis=1)
    h = coupled_case(hip_api, pp, RAMP | AV | QC, 0, k, prof=(prof, of), new_prof=(moved, of), c2=rng.uniform(0.0, 0.05, pp.G))
    assert np.array_equal(h._mirror["gen_avail"], moved) and np.array_equal(h._mirror["gen_avail_of"], of)
    cap = np.where((of >= 0)[:, None], pp.gen_pmax[:, None] * moved[np.maximum(of, 0)], pp.gen_pmax[:, None])
    assert np.all(h.get_primal()[0] <= cap + 1e-9 * pp.gen_pmax.max())          # the iterations ran under the new caps


def test_without_a_flag_it_is_roll_horizon_bit_for_bit(hip_api):
    pp = copper(24)
    states = []
    for coupled in (True, False):
        e = build(hip_api, pp, 0, 0)
        e.iterate(7)
        (e.roll_coupled if coupled else e.roll)(5, tail_of(pp, 5))
        states.append(full_state(e))
        e.iterate(3)
        states.append(full_state(e))
    same_bits(states[0], states[2])
    same_bits(states[1], states[3])
    assert np.all(np.isnan(states[0]["p_prev"])) and np.all(states[0]["ramp_up"] == np.inf) and np.all(states[0]["e_max"] == np.inf)


# ---- refusals leave everything as it was ---------------------------------------------------------------------------------------------

def refused(e, rc, want, snap, *words):
    msg = e.api.last_error(e._ctx).decode()
    assert rc == want, (rc, msg)
    for word in words:
        assert word in msg, msg
    same_bits(snap, full_state(e))


def call(e, k, tail, K=-1, prof=None, of=None, set_budget=0, lo=None, hi=None):
    dp = _capi._dp
    return e.api.roll_horizon_coupled(e._ctx, k, None if tail is None else dp(_capi._f64(np.asarray(tail).T)), K,
                                      None if prof is None else dp(_capi._f64(prof)), None if of is None else of.ctypes.data_as(_capi.c_int32_p),
                                      set_budget, None if lo is None else dp(_capi._f64(lo)), None if hi is None else dp(_capi._f64(hi)))


def test_refusal_of_the_stored_table_under_the_new_anchor(hip_api):
    """(a) generator g's stored profile is 0 before t = k - 1 and 1 from there on, and its ramp_down is below the output it holds at
    k - 1: under the stored table the new anchor cannot come down to the cap 0 at t = 0. With the table moved by k it can."""
    pp = copper(24)
    k, g = 3, 4
    prof = np.ones((1, pp.T))
    prof[0, :k - 1] = 0.0
    of = np.full(pp.G, -1, dtype=np.int32)
    of[g] = 0
    up, down = np.full(pp.G, np.inf), np.full(pp.G, np.inf)
    up[g], down[g] = pp.gen_pmax[g], 0.05 * pp.gen_pmax[g]
    h = build(hip_api, pp, RAMP | AV, 0, (up, down), prof=(prof, of))
    h.iterate(7)
    st = state_of(h)
    st["P"][g] = np.where(np.arange(pp.T) >= k - 1, 0.5 * pp.gen_pmax[g], 0.0)      # (a state handed in is the next step's centre)
    set_from(h, st, 8)
    snap = full_state(h)
    assert snap["P"][g, k - 1] > down[g]                                            # the precondition
    tail = tail_of(pp, k)
    refused(h, call(h, k, tail), E_INVALID, snap, "dopf_roll_horizon_coupled", f"g = {g} ", "t = 0")
    with pytest.raises(_capi.DopfError, match="cannot come down"):
        h.roll_coupled(k, tail)
    same_bits(snap, full_state(h))
    h.roll_coupled(k, tail, availability=(np.ones((1, pp.T)), of))                  # the stored profile moved by k: all ones
    now = h.generator_coupling()
    assert now["p_prev"][g] == snap["P"][g, k - 1] and h.sync() == (2, False)
    h.iterate(3)
    assert h.solver_failures() == 0


def test_refusal_of_what_is_left_of_a_budget_under_the_new_anchor(hip_api):
    """(b) a pair context, generator g with both ramps 0 and e_max binding on its constant path: after k steps e_max - spent is less
    than the only path from the new anchor delivers. With the new window's own budget (the old e_max) the roll is accepted."""
    pp = copper(41)
    k, g = 5, int(np.argmin(copper(41).gen_mc))
    T = pp.T
    c = 0.25 * float(pp.gen_pmax[g])
    up, down = np.full(pp.G, np.inf), np.full(pp.G, np.inf)
    up[g] = down[g] = 0.0
    hi = np.full(pp.G, np.inf)
    hi[g] = path_sum(np.full(T, c))
    h = build(hip_api, pp, RAMP, BUDGET | PAIR, (up, down), (None, hi))
    h.iterate(7)
    st = state_of(h)
    st["P"][g] = c
    set_from(h, st, 8)
    snap = full_state(h)
    tail = tail_of(pp, k)
    refused(h, call(h, k, tail), E_INVALID, snap, "dopf_roll_horizon_coupled", f"g = {g} ", "cannot stay under e_max")
    assert call(h, k, tail, set_budget=1, hi=hi) == 0, h.api.last_error(h._ctx)
    now = h.generator_coupling()
    assert now["p_prev"][g] == c and now["e_max"][g] == hi[g] and np.all(now["e_min"] == 0.0)
    h.iterate(3)
    assert h.solver_failures() == 0


def test_refusals_of_the_arguments(hip_api):
    """(c)"""
    pp = copper(24)
    ramp = draw_ramps(pp, 31)
    h = build(hip_api, pp, RAMP, 0, ramp)
    h.iterate(7)
    snap = full_state(h)
    good = tail_of(pp, 3)
    prof, of = np.ones((1, pp.T)), np.zeros(pp.G, dtype=np.int32)
    refused(h, call(h, 3, good, K=-2), E_INVALID, snap, "n_profiles = -2")
    refused(h, call(h, 3, good, K=1, prof=prof, of=of), E_UNSUPPORTED, snap, "DOPF_F_GEN_AVAILABILITY")
    refused(h, call(h, 3, good, K=0), E_UNSUPPORTED, snap, "DOPF_F_GEN_AVAILABILITY")
    refused(h, call(h, 3, good, set_budget=1), E_UNSUPPORTED, snap, "DOPF_F2_GEN_ENERGY_BUDGET")
    refused(h, call(h, 0, good), E_INVALID, snap, "k = 0")
    refused(h, call(h, pp.T, good), E_INVALID, snap, "k = %d" % pp.T)
    refused(h, call(h, 3, None), E_INVALID, snap, "NULL")
    bad = good.copy()
    bad[0, 1] = np.nan                              # node 0 of the second new step
    refused(h, call(h, 3, bad), E_INVALID, snap, "demand_tail[%d] (node 0, t = %d)" % (pp.N, pp.T - 2))
    # a budget context: the new window's budgets are checked as their setter checks them
    b = build(hip_api, pp, 0, BUDGET)
    b.iterate(3)
    snap_b = full_state(b)
    lo = np.zeros(pp.G)
    lo[2] = -1.0
    refused(b, call(b, 3, good, set_budget=1, lo=lo), E_INVALID, snap_b, "dopf_roll_horizon_coupled", "e_min[2]")
    # an availability context: the table's form
    a = build(hip_api, pp, RAMP | AV, 0, ramp)
    a.iterate(3)
    snap_a = full_state(a)
    refused(a, call(a, 3, good, K=1, prof=2.0 * prof, of=of), E_INVALID, snap_a, "outside [0, 1]")
    refused(a, call(a, 3, good, K=1, prof=prof, of=of + 1), E_INVALID, snap_a, "profile_of[0] = 1")
    # storages in a context without DOPF_F_STO_INITIAL_LEVEL
    s = _capi.Engine(hip_api, params=_capi.default_params(flags=RAMP, **kw_of(pp)), **pp.engine_kwargs())
    s.iterate(3)
    refused(s, call(s, 3, good), E_UNSUPPORTED, full_state(s), "DOPF_F_STO_INITIAL_LEVEL")
    # a context on DOPF_F_COMM_HOST shards
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(flags=_capi.F_COMM_HOST | IL, **kw_of(pp)), **pp.engine_kwargs())
    m.iterate(2)
    shard = m.shard(0)
    rc = call(shard, 3, good[:shard.N])
    assert rc == E_UNSUPPORTED and "communicator" in shard.api.last_error(shard._ctx).decode()
    m.close()


# ---- graphs ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,flags", [(lambda: copper(24), RAMP), (lambda: network(12), RAMP | RAMP_NET)], ids=["copper", "net"])
def test_captured_graphs_stay_valid_across_two_rolls(hip_api, case, flags):
    pp = case()
    ramp = draw_ramps(pp, 31)
    states = []
    for extra in (0, _capi.F_NO_GRAPH):
        h = build(hip_api, pp, flags, 0, ramp, extra=extra)
        h.iterate(21)                       # graphs of 16, 4 and 1 iterations
        h.roll_coupled(5, tail_of(pp, 5))
        h.iterate(21)
        h.roll_coupled(1, tail_of(pp, 1))
        h.iterate(21)
        states.append(full_state(h))
        assert h.solver_failures() == 0
    same_bits(*states)


# ---- three rolls in a row ---------------------------------------------------------------------------------------------------------

def test_three_rolls_in_a_row(hip_api):
    """copper pair, T = 41, k = 1: after each roll the anchor and the budgets are shift_coupled of the getters before it. The
    budgets: e_max alone, on every second generator 1.5 times the warm state's row sum plus 6 gen_pmax — the slowest way down from any
    anchor delivers at most pmax^2 / (2 ramp_down) <= 5 gen_pmax at ramps of 10 % and more, so every roll is admissible (asserted
    before each call by the lattice rule)."""
    pp = copper(41)
    ramp = draw_ramps(pp, 31)
    warm = build(hip_api, pp, RAMP, BUDGET | PAIR, ramp)
    warm.iterate(4)
    hi = np.where(np.arange(pp.G) % 2 == 0, 1.5 * row_sums(warm.get_primal()[0]) + 6.0 * pp.gen_pmax, np.inf)
    h = build(hip_api, pp, RAMP, BUDGET | PAIR, ramp, (None, hi))
    h.iterate(7)
    for n in range(3):
        before = full_state(h)
        want = shift_coupled(1, before["P"], budget=(before["e_min"], before["e_max"]))
        assert rows_fit(pp, before["ramp_up"], before["ramp_down"], want["gen_prev"], *want["gen_budget"]).all(), n
        h.roll_coupled(1, tail_of(pp, 1))
        now = h.generator_coupling()
        assert np.array_equal(now["p_prev"], want["gen_prev"]), n
        assert np.array_equal(now["e_min"], want["gen_budget"][0]) and np.array_equal(now["e_max"], want["gen_budget"][1]), n
        same_bits(now, before, ("ramp_up", "ramp_down"))
        h.iterate(5)
        assert h.solver_failures() == 0
    assert np.all(now["e_max"][::2] <= hi[::2]) and np.any(now["e_max"][::2] < hi[::2]) and np.all(now["e_max"][1::2] == np.inf)


# ---- the debug allocator --------------------------------------------------------------------------------------------------------

def test_roll_coupled_under_the_debug_allocator():
    """DOPF_GUARD=1: every device array ends on the last byte of its own mapping, so an access past an end is a GPU memory fault in
    the child (tests/roll_coupled_worker.py) instead of a silent read of a neighbour."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "roll_coupled_worker.py")
    r = subprocess.run([sys.executable, worker], env=dict(os.environ, DOPF_GUARD="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "roll coupled worker: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
