"""dopf_get_generator_budget_price on the GPU: the multiplier nu the last x-update put on every budget row, as
k_gen_budget and k_gen_ramp_budget store it. One step on plates, networks and the pair against the row's optimality system with the
device's nu FIXED (no multiplier is fitted), the sign rule, and the NumPy twins' nu where the multiplier is unique; the getter moves
nothing else; the status rules; two shards against one context; and convergence of nu to the water value of the central LP."""
import copy

import numpy as np
import pytest

from conftest import pkg
from decentralopf_jl_amd import _capi, central, synth
from helpers import draw_profiles, make_engine, set_from, state_of
from helpers_budget import (BUDGET, CHAIN, budget_engine, budget_project, draw_budgets, draw_budgets_by_state, plate_steps, row_sums,
                            stationarity_at)
from helpers_min_output import all_state, same_bits
from helpers_quadratic import QC, draw_c2, params_of
from helpers_ramp import ramp_infeasibility, ramp_project, step_centres
from helpers_ramp_budget import PAIR, RAMP, draw_budget, draw_limits, extreme_paths, path_sum, ramp_budget_project
from helpers_ramp_net import net_step_pieces, phi_gen

pytestmark = pytest.mark.gpu
AV = _capi.F_GEN_AVAILABILITY
WIDE = _capi.F_DEBUG_WIDE_NET
GAMMA, W_FLOW = 0.3, 10.0                    # networks: the reference's parameters (what net_step_pieces is given)
NET_PRM = dict(eps=0.0, gamma=GAMMA)
NET_CHAIN = _capi.F_NO_FUSE
EXTRAS = {"plain": (False, False), "availability": (True, False), "c2": (False, True), "availability+c2": (True, True)}


def swing(pp, lo=0.4, hi=1.6):
    """the case with its demand alternating between lo and hi times itself (the budget tests'): a row's timesteps differ"""
    f = np.where(np.arange(pp.T) % 2 == 0, lo, hi)
    pp.demand = np.round(np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T) * f[None, :])
    return pp


def pair_engine(api, pp, ramp=None, prev=None, budget=None, flags=0, **params):
    e = _capi.Engine(api, params=_capi.default_params(flags=flags | RAMP, **params), flags2=BUDGET | PAIR, **pp.engine_kwargs())
    if ramp is not None or prev is not None:
        e.set_ramp(*(ramp if ramp is not None else (None, None)), prev)
    if budget is not None:
        e.set_energy_budget(*budget)
    return e


def _profiles(pp, rng):
    """helpers.draw_profiles' three profiles (zeros every fourth step and a fifth of the others: caps that drop to 0 inside a row); on
    a one-step horizon those zeros would leave every row with a profile a box of one point: a value in [0.2, 1] there"""
    prof, of = draw_profiles(pp, "K3", rng)
    if pp.T == 1:
        prof = np.where(prof == 0.0, rng.uniform(0.2, 1.0, prof.shape), prof)
    return prof, of


def _grad(pp, c2, before, prm, P):
    """the derivative of a row's step objective at P, without the budget's term (copper plate: DESIGN.md 3 with w = 1)"""
    if pp.L:
        return phi_gen(pp, c2, before, GAMMA, W_FLOW, P)
    d = P - before["P"]
    return pp.gen_mc[:, None] + np.asarray(c2)[:, None] * P + before["lam"][None, :] + prm["gamma"] * (before["inj"].sum(axis=0)[None, :] + d) + d


def check_sign(nu, P, lo, hi, cap, free):
    """nu > 0 only with the sum on e_max, nu < 0 only on e_min, exactly 0.0 for a row with default budgets"""
    tol = 1e-9 * max(1.0, float(np.max(cap))) * P.size
    s = float(np.sum(P))
    if free:
        assert nu == 0.0 and not np.signbit(nu)
    if nu > 0.0:
        assert abs(s - hi) <= tol, (nu, s, hi)
    if nu < 0.0:
        assert abs(s - lo) <= tol, (nu, s, lo)


def _one_step_setup(hip_api, pp, prm, extra, flags, chain, warm=3):
    """(budget engine, c2, cap, steps, e_min, e_max, classes, state before): the engine in the state of `warm` iterations of the flagless twin on
    the chain, the budgets drawn from the clamped step's sums there by helpers_budget.draw_budgets_by_state"""
    avail, quad = EXTRAS[extra]
    rng = np.random.default_rng(17)
    c2 = draw_c2(pp.G, rng) if quad else np.zeros(pp.G)
    flags |= (AV if avail else 0) | (QC if quad else 0)
    h = budget_engine(hip_api, pp, flags=flags, **prm)
    twin = make_engine(hip_api, pp, flags=flags | chain, **prm)
    cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
    if avail:
        prof, of = _profiles(pp, rng)
        for e in (h, twin):
            e.set_availability(prof, of)
        cap = np.where((of >= 0)[:, None], pp.gen_pmax[:, None] * prof[np.maximum(of, 0)], cap)
    if quad:
        for e in (h, twin):
            e.set_quadratic_cost(c2)
    twin.iterate(warm)
    set_from(h, state_of(twin), twin.get_residuals()[3])
    before = state_of(h)
    if pp.L:
        steps = net_step_pieces(pp, c2, before, GAMMA, W_FLOW)
    else:
        c, q = step_centres(pp, c2, before, prm["gamma"])
        steps = [plate_steps(c[g], q[g]) for g in range(pp.G)]
    S = row_sums([budget_project(steps[g], cap[g]) for g in range(pp.G)])
    lo, hi, classes = draw_budgets_by_state(S, row_sums(cap))
    h.set_energy_budget(lo, hi)
    return h, c2, cap, steps, lo, hi, classes, before


def _certify(pp, prm, h, c2, cap, lo, hi, classes, before, what):
    """one step, then per row the certificate with the device's nu and the sign rule; returns (P, nu)"""
    assert np.array_equal(h.budget_price(), np.zeros(pp.G))
    h.iterate(1)
    P, nu = state_of(h)["P"], h.budget_price()
    grad = _grad(pp, c2, before, prm, P)
    price = float(np.abs(before["lam"]).max()) if before["lam"].size else 0.0
    worst = 0.0
    for g in range(pp.G):
        bound = 1e-9 * (1.0 + abs(float(pp.gen_mc[g])) + price)
        stat = stationarity_at(P[g], grad[g], cap[g], nu[g])
        worst = max(worst, stat / bound)
        assert stat <= bound, (what, g, stat, bound, nu[g])
        check_sign(nu[g], P[g], lo[g], hi[g], cap[g], classes[g] == "free")
    assert h.solver_failures() == 0
    print(f"{what}: stationarity with the device's nu at most {worst:.2e} of its bound; nu {np.array2string(nu, precision=4)}")
    return P, nu


# ---- 1. one step, plates -----------------------------------------------------------------------------------------------------------------

PLATE_CASES = [(T, x) for T in (1, 5, 64, 65, 130) for x in EXTRAS]


@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
@pytest.mark.parametrize("T,extra", PLATE_CASES, ids=[f"T{T}-{x}" for T, x in PLATE_CASES])
def test_one_step_on_a_plate(hip_api, T, extra, eager):
    """12 generators. Every row: stationarity at the stored P with the device's nu, bound 1e-9 (1 + |mc| + max |lambda|); the sign rule.
    Rows with a timestep strictly inside its box (by 1e-9 pmax) have one multiplier only: there nu equals budget_project's to 1e-9
    relative, and at least half of the budgeted rows are such rows."""
    pp = swing(synth.synthetic_case(12, 0, T, seed=30 + T))
    prm = params_of(pp)
    h, c2, cap, steps, lo, hi, classes, before = _one_step_setup(hip_api, pp, prm, extra, _capi.F_NO_GRAPH if eager else 0, CHAIN)
    P, nu = _certify(pp, prm, h, c2, cap, lo, hi, classes, before, f"plate T={T} {extra} {'eager' if eager else 'graphs'}")
    budgeted = unique = 0
    worst = 0.0
    for g in range(pp.G):
        if classes[g] == "free":
            continue
        budgeted += 1
        info = {}
        budget_project(steps[g], cap[g], lo[g], hi[g], info)
        assert info["side"] != 0, (g, classes[g])
        inside = 1e-9 * float(pp.gen_pmax[g])
        if np.any((P[g] > inside) & (P[g] < cap[g] - inside)):
            unique += 1
            rel = abs(nu[g] - info["nu"]) / abs(info["nu"])
            worst = max(worst, rel)
            assert rel <= 1e-9, (g, nu[g], info["nu"])
        assert np.sign(nu[g]) == info["side"], (g, nu[g], info)
    print(f"   {unique}/{budgeted} budgeted rows with a unique multiplier, |nu - twin| / |twin| at most {worst:.2e}")
    assert 2 * budgeted >= pp.G and 2 * unique >= budgeted, (unique, budgeted)


# ---- 2. one step, network ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wide", [0, WIDE], ids=["net", "wide-chain"])
@pytest.mark.parametrize("T", [5, 65])
def test_one_step_on_a_network(hip_api, T, wide):
    """12 generators on 6 nodes and 8 lines: the same certificate with the derivative of the closed forms of DESIGN.md section 3
    (helpers_ramp_net.phi_gen), never the device's tables; the sign rule; at least a quarter of the rows bind."""
    pp = swing(synth.synthetic_case(12, 0, T, N=6, L=8, seed=2))
    h, c2, cap, steps, lo, hi, classes, before = _one_step_setup(hip_api, pp, NET_PRM, "plain", wide, NET_CHAIN)
    assert h.wide_net() == (1 if wide else 0)
    P, nu = _certify(pp, NET_PRM, h, c2, cap, lo, hi, classes, before, f"network T={T} {'wide' if wide else ''}")
    assert 4 * int(np.count_nonzero(nu)) >= pp.G, nu


# ---- 3. the pair -------------------------------------------------------------------------------------------------------------------------

def _pair_rows(pp, c, q, cap, rng):
    """ramps and budgets by row class g mod 4, so that every branch of k_gen_ramp_budget's cascade occurs: 0 — ramps of pmax (never
    broken) under a finite budget with room: the clamped step; 1 — ramps of pmax, e_max = 0.6 of the clamped step's sum: the budget
    alone; 2 — drawn ramps under a budget that holds what any path delivers: the ramps alone; 3 — drawn ramps and
    helpers_ramp_budget.draw_budget: the pair search. No anchors."""
    G, T = pp.G, pp.T
    up, down, lo, hi = np.zeros(G), np.zeros(G), np.zeros(G), np.full(G, np.inf)
    for g in range(G):
        pm = float(pp.gen_pmax[g])
        s0 = path_sum(np.clip(c[g], 0.0, cap[g]))
        if g % 4 <= 1:
            up[g] = down[g] = pm
            hi[g] = T * pm + 1.0 if g % 4 == 0 else 0.6 * s0
            if g % 4 == 1 and not s0 > 1e-6 * pm:                         # (a row at rest has nothing to give: its e_min binds instead)
                lo[g], hi[g] = 0.4 * T * pm, np.inf
        else:
            up[g], down[g], _ = draw_limits(rng, g, cap[g], pm, False)
            if g % 4 == 2:
                hi[g] = T * pm + 1.0
            else:
                lo[g], hi[g] = draw_budget(rng, g, c[g], q[g], cap[g], up[g], down[g], None)
    return up, down, lo, hi


def _branch(c, q, cap, up, down, lo, hi):
    """the branch of the cascade that stores the row, from the NumPy pieces alone"""
    x0 = np.clip(c, 0.0, cap)
    bad0 = ramp_infeasibility(x0, cap, up, down) > 0.0
    in0 = lo <= path_sum(x0) <= hi
    if not bad0:
        if in0:
            return 1
        x = budget_project(plate_steps(c, q), cap, lo, hi)
        return 2 if ramp_infeasibility(x, cap, up, down) <= 0.0 else 4
    s = path_sum(ramp_project(c, q, cap, up, down, None))
    return 3 if lo <= s <= hi else 4


@pytest.mark.parametrize("T", [6, 70, 130])
def test_one_step_of_the_pair(hip_api, T):
    """DOPF_F2_GEN_RAMP_BUDGET (T = 130: beyond kRampLdsT = 128, the centres and the repair's arrays in scratch). Every branch of the
    cascade occurs (from the twin). Branches 1 and 3 store exactly 0.0. Branches 2 and 4: where the twin's phi(nu) = sum_t x_t(nu)
    falls strictly on both sides of nu* — one multiplier only — nu equals ramp_budget_project's to 1e-9 relative; elsewhere its sign
    is that of the bound met. P is the twin's row to 1e-9 scaled, as the pair's own test asks."""
    G = 24 if T < 130 else 16
    pp = swing(synth.synthetic_case(G, 0, T, seed=20 + T))
    prm = params_of(pp)
    rng = np.random.default_rng(100 + T)
    h = pair_engine(hip_api, pp, **prm)
    twin = make_engine(hip_api, pp, flags=_capi.F_NO_FUSE | _capi.F_NO_TAIL_FUSE, **prm)
    twin.iterate(4)
    set_from(h, state_of(twin), twin.get_residuals()[3])
    before = state_of(h)
    c, q = step_centres(pp, np.zeros(pp.G), before, prm["gamma"])
    cap = np.repeat(pp.gen_pmax[:, None], T, axis=1)
    up, down, lo, hi = _pair_rows(pp, c, q, cap, rng)
    h.set_ramp(up, down, None)
    h.set_energy_budget(lo, hi)
    assert np.array_equal(h.budget_price(), np.zeros(pp.G))
    h.iterate(1)
    P, nu = state_of(h)["P"], h.budget_price()
    seen = {1: 0, 2: 0, 3: 0, 4: 0}
    unique = 0
    worst = 0.0
    for g in range(pp.G):
        b = _branch(c[g], q[g], cap[g], up[g], down[g], lo[g], hi[g])
        seen[b] += 1
        if b in (1, 3):
            assert nu[g] == 0.0 and not np.signbit(nu[g]), (g, b, nu[g])
            continue
        info = {}
        want = ramp_budget_project(c[g], q[g], cap[g], up[g], down[g], None, lo[g], hi[g], info)
        assert np.abs(P[g] - want).max() <= 1e-9 * max(1.0, float(pp.gen_pmax[g])), (g, b)
        assert info["side"] != 0 and np.sign(nu[g]) == info["side"], (g, b, nu[g], info)
        target = hi[g] if info["side"] > 0 else lo[g]
        d = 1e-6 * abs(info["nu"])
        f = lambda x: path_sum(ramp_project(c[g] - x / q[g], q[g], cap[g], up[g], down[g], None))
        # one free timestep moves by d / q: a thousandth of that on both sides says phi is not flat at nu*
        if f(info["nu"] - d) - target >= 1e-3 * d / q[g] and target - f(info["nu"] + d) >= 1e-3 * d / q[g]:
            unique += 1
            rel = abs(nu[g] - info["nu"]) / abs(info["nu"])
            worst = max(worst, rel)
            assert rel <= 1e-9, (g, b, nu[g], info["nu"])
    print(f"pair T={T}: rows by branch {seen}, {unique} with a unique multiplier, |nu - twin| / |twin| at most {worst:.2e}")
    assert min(seen.values()) >= 1, seen
    assert 2 * unique >= seen[2] + seen[4], (unique, seen)
    assert h.solver_failures() == 0


# ---- 4. nothing else moved ---------------------------------------------------------------------------------------------------------------

def _moved_case(hip_api):
    pp = swing(synth.synthetic_case(41, 3, 5, seed=6))
    prm = params_of(pp)
    warm = make_engine(hip_api, pp, flags=CHAIN, **prm)
    warm.iterate(4)
    budget = draw_budgets(row_sums(warm.get_primal()[0]), row_sums(np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)))
    return pp, prm, budget


@pytest.mark.parametrize("which", ["budget", "pair"])
def test_the_getter_moves_nothing(hip_api, which):
    """Three contexts of the same problem: a is asked for its prices between any two iterations, b once before the first (the call
    that starts the recording) and then only at the end, c never — a budget context that never asks runs the instantiations
    without the store. After 1, 4 and 7 iterations every getter the other tests pin (primal, duals, consensus, residuals:
    helpers_min_output.all_state) gives the same bits in all three, and the prices read late equal the prices read all along."""
    pp, prm, budget = _moved_case(hip_api)
    if which == "budget":
        a, b, c = (budget_engine(hip_api, pp, budget, **prm) for _ in range(3))
    else:
        ramp = (0.2 * pp.gen_pmax, 0.25 * pp.gen_pmax)
        a, b, c = (pair_engine(hip_api, pp, ramp, None, budget, **prm) for _ in range(3))
    assert np.array_equal(b.budget_price(), np.zeros(pp.G))
    done = 0
    for upto in (1, 4, 7):
        while done < upto:
            a.budget_price()
            a.iterate(1)
            b.iterate(1)
            c.iterate(1)
            done += 1
        last = a.budget_price()
        assert same_bits(all_state(a), all_state(b)) and same_bits(all_state(a), all_state(c)), (which, upto)
        assert np.array_equal(last, b.budget_price()) and np.any(last != 0.0)
    assert a.solver_failures() == 0 and b.solver_failures() == 0 and c.solver_failures() == 0
    # c asks now, for the first time: a pair context has recorded all along; a budget context starts recording with this call —
    # zeros now, the next iteration's prices after it, and nothing else moves
    first = c.budget_price()
    assert np.array_equal(first, last if which == "pair" else np.zeros(pp.G))
    for e in (a, c):
        e.iterate(1)
    assert same_bits(all_state(a), all_state(c)) and np.array_equal(a.budget_price(), c.budget_price()) and np.any(c.budget_price() != 0.0)


# ---- 5. the status rules -----------------------------------------------------------------------------------------------------------------

def _small():
    return swing(synth.synthetic_case(7, 0, 5, seed=3))


@pytest.mark.parametrize("which", ["budget", "pair"])
def test_values_are_those_of_the_last_x_update(hip_api, which):
    pp = _small()
    prm = params_of(pp)
    warm = make_engine(hip_api, pp, flags=CHAIN, **prm)
    warm.iterate(6)
    cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
    budget = draw_budgets(row_sums(warm.get_primal()[0]), row_sums(cap))
    make = (lambda **kw: budget_engine(hip_api, pp, budget, **kw)) if which == "budget" else \
           (lambda **kw: pair_engine(hip_api, pp, (0.3 * pp.gen_pmax, 0.3 * pp.gen_pmax), None, budget, **kw))
    h = make(**prm)
    assert np.array_equal(h.budget_price(), np.zeros(pp.G))                       # zeros before the first iteration, budgets set
    h.trace_begin(_capi.TRACE_ALL, 8)                                             # the getter works while a trace is active
    h.iterate(3)
    nu = h.budget_price()
    assert np.count_nonzero(nu) >= 2 and h.trace_info()[3] >= 1
    h.trace_end()
    # the setters leave the values alone
    h.set_energy_budget(None, None)
    assert np.array_equal(h.budget_price(), nu)
    st = state_of(h)
    h.set_state(P=0.5 * st["P"], lam=st["lam"], iteration=4)
    assert np.array_equal(h.budget_price(), nu)
    h.set_demand(0.9 * np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T))
    assert np.array_equal(h.budget_price(), nu)
    h.roll_coupled(1, np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, :1], budget=(None, None))
    assert np.array_equal(h.budget_price(), nu)
    # ... until the next iteration: every budget is at its default now
    h.iterate(1)
    assert np.array_equal(h.budget_price(), np.zeros(pp.G))
    # a halted context computes nothing: the values stay, although the budgets are gone
    e = make(max_iters=3, **prm)
    e.budget_price()                                                              # (starts the recording)
    assert 0 < e.iterate(5)[0] < 5                                                 # (halted at max_iters)
    nu = e.budget_price()
    assert np.count_nonzero(nu) >= 2
    e.set_energy_budget(None, None)
    it = e.sync()[0]
    assert e.iterate(2)[0] == 0 and e.sync()[0] == it
    assert np.array_equal(e.budget_price(), nu)


def test_refusals(hip_api):
    pp = _small()
    prm = params_of(pp)
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*dopf_get_generator_budget_price.*DOPF_F2_GEN_ENERGY_BUDGET"):    # DOPF_E_UNSUPPORTED
        make_engine(hip_api, pp, **prm).budget_price()
    with pytest.raises(_capi.DopfError, match=r"\(-4\)"):
        _capi.Engine(hip_api, params=_capi.default_params(flags=RAMP, **prm), **pp.engine_kwargs()).budget_price()
    h = budget_engine(hip_api, pp, **prm)
    assert hip_api.get_generator_budget_price(h._ctx, None) == -1                 # DOPF_E_INVALID
    assert b"dopf_get_generator_budget_price: nu is NULL" in hip_api.last_error(h._ctx)
    nogen = synth.synthetic_case(0, 3, 5, seed=3)
    e = budget_engine(hip_api, nogen, **params_of(nogen))
    assert hip_api.get_generator_budget_price(e._ctx, None) == 0 and e.budget_price().size == 0


# ---- 6. shards ---------------------------------------------------------------------------------------------------------------------------

def _sharding_case(hip_api):
    pp = swing(synth.synthetic_case(41, 7, 6, seed=4))
    g = 1.0 / (pp.G + pp.S)
    warm = make_engine(hip_api, pp, eps=0.0, gamma=g, flags=CHAIN)
    warm.iterate(4)
    lo, hi = draw_budgets(row_sums(warm.get_primal()[0]), row_sums(np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)))
    return pp, g, lo, hi


def _same_prices(got, want, first, who):
    """Bit for bit after the first iteration, where every rank's rows read the inputs one context reads. From the first dual step on
    the shards' lambda and injections differ from one context's in the last bits (their sums are added in another order: measured on
    an MI355X on the parent commit, |lambda| apart by 4e-14 after one iteration and 31 of 41 rows of P with other bits after two), and
    a price is formed from them: there the bound is the one the budget tests hold two chains to, 1e-9 scaled (observed: 2e-13)."""
    diff = float(np.abs(got - want).max())
    print(f"{who}: {np.count_nonzero(want)} priced rows, largest |difference| {diff:.2e}")
    assert np.count_nonzero(want) >= want.size // 4
    if first:
        assert np.array_equal(got, want), who
    assert diff <= 1e-9 * max(1.0, float(np.abs(want).max())), (who, diff)


def test_multi_two_shards_equal_one_context(hip_api):
    pp, g, lo, hi = _sharding_case(hip_api)
    ref = budget_engine(hip_api, pp, (lo, hi), eps=0.0, gamma=g)
    ref.budget_price()                                                            # (starts the recording, as m's first call below does on every shard)
    q = copy.copy(pp)
    q.gen_budget = (lo, hi)
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(eps=0.0, gamma=g, flags=_capi.F_COMM_HOST), **q.engine_kwargs())
    assert np.array_equal(m.budget_price(), np.zeros(pp.G))
    for k in (1, 3):
        ref.iterate(k)
        assert m.iterate(k) == (k, False)
        got = m.budget_price()
        _same_prices(got, ref.budget_price(), k == 1, "multi")
    # each shard's own getter is its slice
    n0 = m.shard(0).G
    assert np.array_equal(np.concatenate([m.shard(i).budget_price() for i in range(2)]), got) and 0 < n0 < pp.G
    assert hip_api.multi_get_generator_budget_price(m._m, None) == -1
    m.close()


def test_sharded_admm_two_ranks_equal_one_context(hip_api):
    """Two ranks against a plain context (bits after the first iteration, _same_prices' bound later) and, at every iteration, bit
    for bit against ONE context on equal inputs: a one-rank ShardedADMM of the whole case whose consensus vector is, like the two
    ranks', the ranks' sum — so all three derive lambda, injections and prices from the same bits, and every row's step and price must
    agree to the last bit after 1, 4 and 7 iterations. (Copying the shards' state into a context with set_state does not give equal
    inputs: that context forms the injections again from P in its own order of additions — measured 1.8e-12 apart, and 11 of 28
    prices with other bits after the next step.)"""
    import torch
    pp, g, lo, hi = _sharding_case(hip_api)
    ref = budget_engine(hip_api, pp, (lo, hi), eps=0.0, gamma=g)
    q = copy.copy(pp)
    q.gen_budget = (lo, hi)
    ranks = [pkg.ShardedADMM(q, r, 2, all_reduce=lambda: None, eps=0.0, gamma=g) for r in range(2)]
    whole = pkg.ShardedADMM(q, 0, 1, all_reduce=lambda: None, eps=0.0, gamma=g)
    for e in [ref, whole] + ranks:                                                # (every context's first call starts its recording)
        assert not np.any(e.budget_price(all_reduce=lambda x: x) if e is not ref else e.budget_price())
    done = 0
    for upto in (1, 4, 7):
        while done < upto:
            done += 1
            for sh in ranks + [whole]:
                sh.engine.local_update()
            for sh in ranks + [whole]:
                sh.sync()
            total = ranks[0]._tensor.cpu() + ranks[1]._tensor.cpu()          # (summed on the host: no PyTorch kernel has to load)
            for sh in ranks + [whole]:
                sh._tensor.copy_(total)
            torch.cuda.synchronize()
            for sh in ranks + [whole]:
                sh.engine.apply_consensus()
            for sh in ranks + [whole]:
                sh.sync()
            ref.iterate(1)
        # every rank's vector holds its own slice and zeros: their sum is the gather (the all-reduce of the product path)
        parts = [sh.budget_price(all_reduce=lambda x: x) for sh in ranks]
        for sh, part in zip(ranks, parts):
            a, b = sh.shard.meta["gen_range"]
            assert not np.any(part[:a]) and not np.any(part[b:])
        _same_prices(parts[0] + parts[1], ref.budget_price(), upto == 1, "sharded")
        one = whole.budget_price()
        rows = np.concatenate([sh.engine.get_primal()[0] for sh in ranks])
        print(f"sharded, equal inputs, iteration {upto}: {np.count_nonzero(one)} priced rows, {int(np.sum(parts[0] + parts[1] != one))} with other bits")
        assert np.array_equal(rows, whole.engine.get_primal()[0]), upto                 # the rows read the same inputs ...
        assert np.array_equal(parts[0] + parts[1], one) and np.count_nonzero(one) >= pp.G // 4, upto      # ... and store the same prices


# ---- 7. convergence to the LP's water value ----------------------------------------------------------------------------------------------

def _water_case():
    node = pkg.Node("plate", [55, 75, 95, 125, 85, 65], True)
    gens = [pkg.Generator(f"g{i}", mc, pm, "k", node) for i, (mc, pm) in enumerate(zip([5, 20, 40, 70], [50, 60, 40, 60]))]
    return [node], gens


@pytest.mark.parametrize("which", ["budget", "pair"])
def test_converged_price_is_the_lps_water_value(hip_api, which):
    """One plate, T = 6, the cheapest unit (5 per MWh, 50 MW) with 100 MWh for the window. The host LP: objective 9400, and the
    objective's one-sided slopes in e_max are -35 on both sides (repeated here with e_max = 99 and 101), so the budget dual -35 is
    unique: the water value is 35. The run stops at eps = 1e-6. The bound on |nu[0] - 35| is 10 x the largest |lambda[t] - LP price|
    of the same run — the row's price cannot be known better than the prices it is formed from — and the same bound holds against
    -budget_dual[0] of the device LP (dopf_central_solve_coupled). pair: the same case in a DOPF_F2_GEN_RAMP_BUDGET context with ramps
    of 30 on the budgeted unit; both LPs take the ramps too (their slopes are -35 as well). Measured on an MI355X, both contexts: 112
    iterations to the stop test, |nu[0] - 35| = 1.3e-6 (1.3e-6 against the device LP's dual too), largest price gap 8.1e-6, cost
    9399.9994."""
    nodes, gens = _water_case()
    pp = pkg.pack(nodes, gens, [], [])
    lo, hi = np.zeros(4), np.array([100.0, np.inf, np.inf, np.inf])
    ramp = (np.array([30.0, np.inf, np.inf, np.inf]),) * 2 if which == "pair" else None
    solve = lambda e: central.solve_central_packed(pp, gen_budget=(lo, np.array([e, np.inf, np.inf, np.inf])), gen_ramp=ramp)
    want, below, above = solve(100.0), solve(99.0), solve(101.0)
    assert abs(want.objective - 9400.0) <= 1e-6
    assert abs((want.objective - below.objective) + 35.0) <= 1e-6 and abs((above.objective - want.objective) + 35.0) <= 1e-6
    dev, duals = central.central_reference_coupled_on_device(nodes, gens, [], [], gen_budget=(lo, hi), gen_ramp=ramp, duals=True)
    prm = dict(eps=1e-6, max_iters=200000)
    h = budget_engine(hip_api, pp, (lo, hi), **prm) if which == "budget" else pair_engine(hip_api, pp, ramp, None, (lo, hi), **prm)
    assert not np.any(h.budget_price())                                          # (starts the recording on the budget context)
    done, conv = h.iterate(200000)
    nu, st = h.budget_price(), state_of(h)
    # the iteration's lambda is minus the LP's price: a unit inside its box has mc + lambda + nu = 0 at the fixed point
    price_gap = float(np.abs(-st["lam"] - want.system_price).max())
    gap, gap_dev = abs(nu[0] - 35.0), abs(nu[0] + duals["budget_dual"][0])
    print(f"{which}: converged {conv} after {done} iterations, nu[0] = {nu[0]:.9f}, |nu[0] - 35| = {gap:.3e}, against the device LP's "
          f"budget_dual {duals['budget_dual'][0]:.9f}: {gap_dev:.3e}, largest price gap {price_gap:.3e} (bound {10 * price_gap:.3e}), "
          f"cost {float(st['cost'][0]):.6f} (LP {want.objective:.6f}, device LP {dev.objective:.6f})")
    assert conv and done < 200000
    assert np.array_equal(nu[1:], np.zeros(3))
    assert gap <= 10.0 * price_gap, (gap, price_gap)
    assert gap_dev <= 10.0 * price_gap, (gap_dev, price_gap)
    assert h.solver_failures() == 0
