"""DOPF_F2_GEN_RAMP_BUDGET on the GPU: the generators' step under ramp limits and energy budgets at once
(k_gen_ramp_budget) against the bisecting NumPy reference row by row; the bits of the three older chains where a constraint is at its
default; the setters' joint-feasibility check and the create rules; convergence to the host LP with ramp and budget rows; two shards
against one context and the packed route through admm.ADMM."""
import copy
import ctypes

import numpy as np
import pytest

from decentralopf_jl_amd import _capi, admm, central, synth
from helpers import make_engine, set_from, state_of
from helpers_budget import budget_violation, draw_budgets, row_sums
from helpers_quadratic import QC, draw_c2, params_of
from helpers_ramp import CHAIN, draw_ramps, ramp_infeasibility, step_centres
from helpers_ramp_budget import BUDGET, PAIR, RAMP, both_bind, draw_budget, draw_limits, extreme_paths, path_sum, ramp_budget_project

pytestmark = pytest.mark.gpu
AV = _capi.F_GEN_AVAILABILITY
EXTRAS = {"plain": (False, False), "availability": (True, False), "c2": (False, True), "availability+c2": (True, True)}
# T -> generators: 41, so that on the short horizons (one item) a block's wave loops over several rows; 21 at T = 130, where the
# reference's bisection takes a fifth of a second per row (64 / 65: the wave edge; 130: beyond kRampLdsT, the centres and
# ramp_repair's arrays in scratch)
SHAPES = {1: 41, 2: 41, 5: 41, 64: 41, 65: 41, 130: 21}


def swing(pp, lo=0.4, hi=1.6):
    """the case with its demand alternating between lo and hi times itself (the ramp tests'): a row's timesteps differ"""
    f = np.where(np.arange(pp.T) % 2 == 0, lo, hi)
    pp.demand = np.round(np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T) * f[None, :])
    return pp


def pair_engine(api, pp, ramp=None, prev=None, budget=None, flags=0, flags2=BUDGET | PAIR, **params):
    """a context with the three flags; ramps, anchor and budgets set after create (None: that setter is not called)"""
    e = _capi.Engine(api, params=_capi.default_params(flags=flags | RAMP, **params), flags2=flags2, **pp.engine_kwargs())
    if ramp is not None or prev is not None:
        e.set_ramp(*(ramp if ramp is not None else (None, None)), prev)
    if budget is not None:
        e.set_energy_budget(*budget)
    return e


CASES = [(T, x) for T in SHAPES for x in EXTRAS]


@pytest.mark.parametrize("T,extra", CASES, ids=[f"T{T}-{x}" for T, x in CASES])
def test_one_step_against_the_bisecting_reference(hip_api, T, extra):
    """One step from the state of 4 flagless iterations: P against helpers_ramp_budget.ramp_budget_project row by row, 1e-9 scaled by
    max(1, gen_pmax) (the suite's bound for a primal value); box, ramps and budget kept to the same bound; no solver failure; and in
    the reference at least a quarter of the rows have a tight ramp and a multiplier on the budget. T = 1: a row's one ramp is its
    anchor's, and it binds together with the budget only where the budget leaves one path — the anchored rows' bounds are drawn on
    that path's sum. The setter anchors every row or none: every row in the plain and the availability+c2 variants and at T = 1."""
    avail, quad = EXTRAS[extra]
    anchored = T == 1 or avail == quad
    pp = swing(synth.synthetic_case(SHAPES[T], 0, T, seed=20 + T))
    prm = params_of(pp)
    rng = np.random.default_rng(100 + T)
    c2 = draw_c2(pp.G, rng) if quad else np.zeros(pp.G)
    flags = (AV if avail else 0) | (QC if quad else 0)
    h = pair_engine(hip_api, pp, flags=flags, **prm)
    twin = make_engine(hip_api, pp, flags=flags | CHAIN, **prm)
    cap = np.repeat(pp.gen_pmax[:, None], T, axis=1)
    if avail:
        prof = rng.uniform(0.2, 1.0, (3, T))
        of = rng.integers(0, 3, pp.G).astype(np.int32)
        of[::3] = -1
        for e in (h, twin):
            e.set_availability(prof, of)
        cap = np.where((of >= 0)[:, None], pp.gen_pmax[:, None] * prof[np.maximum(of, 0)], cap)
    if quad:
        for e in (h, twin):
            e.set_quadratic_cost(c2)
    twin.iterate(4)
    st, it = state_of(twin), twin.get_residuals()[3]
    set_from(h, st, it)
    before = state_of(h)
    c, q = step_centres(pp, c2, before, prm["gamma"])
    lim = [draw_limits(rng, g, cap[g], float(pp.gen_pmax[g]), anchored) for g in range(pp.G)]
    up, down = np.array([l[0] for l in lim]), np.array([l[1] for l in lim])
    prev = [l[2] for l in lim]
    bud = [draw_budget(rng, g, c[g], q[g], cap[g], up[g], down[g], prev[g], exact=(T == 1 and prev[g] is not None)) for g in range(pp.G)]
    lo, hi = np.array([b[0] for b in bud]), np.array([b[1] for b in bud])
    h.set_ramp(up, down, np.array(prev) if anchored else None)
    h.set_energy_budget(lo, hi)
    h.iterate(1)
    P = state_of(h)["P"]
    worst = viol = 0.0
    bind = 0
    for g in range(pp.G):
        info = {}
        want = ramp_budget_project(c[g], q[g], cap[g], up[g], down[g], prev[g], lo[g], hi[g], info)
        bind += both_bind(want, up[g], down[g], prev[g], info)
        scale = max(1.0, float(pp.gen_pmax[g]))
        worst = max(worst, float(np.abs(P[g] - want).max()) / scale)
        viol = max(viol, ramp_infeasibility(P[g], cap[g], up[g], down[g], prev[g]) / scale, budget_violation(P[g], lo[g], hi[g]) / scale)
    print(f"T={T} {extra}: |P - reference| {worst:.2e} (scaled), box / ramp / budget violation {viol:.2e} (scaled), ramp and budget "
          f"both bind in {bind}/{pp.G} rows, solver failures {h.solver_failures()}")
    assert 4 * bind >= pp.G, (bind, pp.G)
    assert worst <= 1e-9, worst
    assert viol <= 1e-9, viol
    assert h.solver_failures() == 0


# ---- a constraint at its default: the bits of the older chains -----------------------------------------------------------------------------

def _free_case():
    return swing(synth.synthetic_case(41, 3, 5, seed=6))


@pytest.mark.parametrize("which", ["ramps-only", "budgets-only", "neither"])
def test_defaults_give_the_bits_of_the_older_chains(hip_api, which):
    """After 1, 4 and 7 iterations the whole state equals (i) a DOPF_F_GEN_RAMP context's when every budget is default, (ii) a
    DOPF_F2_GEN_ENERGY_BUDGET context's when every ramp is +inf with no anchor, (iii) the flagless context's on that chain when both
    are default (odd T: it runs k_gen_update itself)."""
    pp = _free_case()
    prm = params_of(pp)
    rng = np.random.default_rng(3)
    warm = make_engine(hip_api, pp, flags=CHAIN, **prm)
    warm.iterate(4)
    P0 = warm.get_primal()[0]
    ramp = draw_ramps(pp, rng) if which == "ramps-only" else None
    anchor = 0.5 * pp.gen_pmax if which == "ramps-only" else None
    budget = draw_budgets(row_sums(P0), row_sums(np.repeat(pp.gen_pmax[:, None], pp.T, axis=1))) if which == "budgets-only" else None
    h = pair_engine(hip_api, pp, ramp, anchor, budget, **prm)
    if which == "ramps-only":
        ref = _capi.Engine(hip_api, params=_capi.default_params(flags=RAMP, **prm), **pp.engine_kwargs())
        ref.set_ramp(*ramp, anchor)
    elif which == "budgets-only":
        ref = _capi.Engine(hip_api, params=_capi.default_params(**prm), flags2=BUDGET, **pp.engine_kwargs())
        ref.set_energy_budget(*budget)
    else:
        ref = make_engine(hip_api, pp, flags=CHAIN, **prm)
    for k in (1, 3, 3):
        h.iterate(k)
        ref.iterate(k)
        a, b = state_of(h), state_of(ref)
        for key in a:
            assert np.array_equal(a[key], b[key]), (which, key)
    assert h.solver_failures() == 0 and ref.solver_failures() == 0


# ---- the setters and create ------------------------------------------------------------------------------------------------------------

def _small():
    return swing(synth.synthetic_case(7, 0, 5, seed=3))


def _create_ex(api, pp, flags, flags2, **params):
    keys = ("N", "L", "T", "demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax", "sto_node")
    kw = pp.engine_kwargs()
    prob, keep, G, S = _capi._problem(**{k: kw[k] for k in keys})
    ctx = ctypes.c_void_p()
    q = _capi.default_params(flags=flags, **params)
    rc = api.create_ex(ctypes.byref(ctx), ctypes.byref(prob), ctypes.byref(q), flags2)
    msg = (api.last_error(None) or b"").decode()
    if ctx.value:
        api.destroy(ctx)
    return rc, msg


def test_joint_feasibility_refusals_name_the_row_and_store_nothing(hip_api):
    pp = _small()
    prm = params_of(pp)
    G, T, pm = pp.G, pp.T, pp.gen_pmax
    up, down = 0.1 * pm, 0.1 * pm
    prev = 0.5 * pm
    lo, hi = 0.5 * pm, 3.0 * pm
    prof, of = np.full((1, T), 0.9), np.zeros(G, dtype=np.int32)
    h, twin = (pair_engine(hip_api, pp, (up, down), prev, (lo, hi), flags=AV, **prm) for _ in range(2))
    for e in (h, twin):
        e.set_availability(prof, of)
        e.iterate(3)

    def bad(a, g, v):
        x = a.copy()
        x[g] = v
        return x
    # every generator is anchored at 0.5 pmax and moves 0.1 pmax a step under caps of 0.9 pmax: its window delivers between 1.0 pmax
    # (0.4 + 0.3 + 0.2 + 0.1 + 0) and 3.9 pmax (0.6 + 0.7 + 0.8 + 0.9 + 0.9). The caps alone leave room for 4.5 pmax: the older check passes
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_energy_budget.*g = 2 .*e_min.*largest path"):
        h.set_energy_budget(bad(lo, 2, 4.0 * pm[2]), bad(hi, 2, 4.4 * pm[2]))
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_energy_budget.*g = 2 .*e_max.*smallest path"):
        h.set_energy_budget(bad(lo, 2, 0.0), bad(hi, 2, 0.9 * pm[2]))
    # the ramp setter repeats it: from 0.5 pmax at 0.01 pmax a step generator 4 delivers at least 2.35 pmax, above its e_max = 2.3 pmax
    lo2, hi2 = bad(lo, 1, 3.09 * pm[1]), bad(bad(hi, 4, 2.3 * pm[4]), 1, 4.0 * pm[1])
    for e in (h, twin):
        e.set_energy_budget(lo2, hi2)
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_ramp.*g = 4 .*e_max"):
        h.set_ramp(up, bad(down, 4, 0.01 * pm[4]), prev)
    # ... and the availability setter: under caps of 0.62 pmax generator 1 delivers at most 0.6 + 4 x 0.62 = 3.08 pmax, under its
    # e_min = 3.09 pmax — which the caps alone (3.1 pmax) and the anchor alone would allow
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_availability.*g = 1 .*e_min.*largest path"):
        h.set_availability(np.vstack([prof, np.full((1, T), 0.62)]), bad(of, 1, 1))
    # (caps of 0.3 pmax leave generator 0 no first step down from its anchor: the ramp check's own refusal, as before)
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_availability.*g = 0 "):
        h.set_availability(np.vstack([prof, np.full((1, T), 0.3)]), bad(of, 0, 1))
    assert h.iterate(5) == twin.iterate(5)
    a, b = state_of(h), state_of(twin)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_create_rules(hip_api):
    pp = _small()
    for flags, flags2 in ((RAMP, PAIR), (0, BUDGET | PAIR), (0, PAIR)):
        rc, msg = _create_ex(hip_api, pp, flags, flags2)
        assert rc == -4 and "DOPF_F2_GEN_RAMP_BUDGET means nothing without" in msg, (flags, flags2, msg)          # DOPF_E_UNSUPPORTED
    net = synth.synthetic_case(12, 0, 4, N=6, L=8, seed=2)
    rc, msg = _create_ex(hip_api, net, RAMP | _capi.F_GEN_RAMP_NETWORK, BUDGET | PAIR)
    assert rc == -4 and "DOPF_F2_GEN_RAMP_BUDGET" in msg and "copper plates" in msg
    rc, msg = _create_ex(hip_api, pp, RAMP, BUDGET)                                     # the two older flags without the bit: as before
    assert rc == -4 and "DOPF_F2_GEN_ENERGY_BUDGET" in msg and "DOPF_F_GEN_RAMP" in msg and "RAMP_BUDGET" not in msg
    assert _create_ex(hip_api, pp, RAMP, BUDGET | PAIR)[0] == 0
    nogen = synth.synthetic_case(0, 3, 5, seed=3)                                       # no generators: accepted and ignored
    assert _create_ex(hip_api, nogen, RAMP, BUDGET | PAIR)[0] == 0
    h = pair_engine(hip_api, pp, **params_of(pp))
    h.iterate(2)
    tail = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, :1]
    rc = h.api.roll_horizon(h._ctx, 1, _capi._dp(_capi._f64(tail.T)))
    assert rc == -4 and b"dopf_roll_horizon" in h.api.last_error(h._ctx)


# ---- convergence to the host LP with ramp and budget rows -------------------------------------------------------------------------------

def test_converged_run_against_the_host_lp(hip_api):
    """swing(synthetic_case(7, 0, 5, seed=3), 0.85, 1.15) with the budgets of test_gpu_gen_budget's convergence test and ramps of
    30 % of pmax per step on every generator, which bind at the LP optimum (asserted: the objective moves by more than 1e-6 relative
    against budgets alone; on the host LP it moves by 3.1 %, 73 028 -> 75 298, and ramps of 20 % leave the case infeasible). That test's bounds: converged, cost within 1e-3 of the LP, budgets and
    ramps kept to 1e-9 scaled, no solver failures. Measured on an MI355X: 134 iterations to the stop test, cost within 6.7e-7 of the LP's."""
    pp = swing(synth.synthetic_case(7, 0, 5, seed=3), 0.85, 1.15)
    free = central.solve_central_packed(pp)
    E = free.generation.sum(axis=1)
    room = pp.T * pp.gen_pmax
    lo, hi = np.zeros(pp.G), np.full(pp.G, np.inf)
    big = int(np.argmax(E))
    hi[big] = 0.7 * E[big]
    small = int(np.argmin(np.where(np.arange(pp.G) == big, np.inf, E / room)))
    lo[small] = E[small] + 0.1 * room[small]
    alone = central.solve_central_packed(pp, gen_budget=(lo, hi))
    up = down = 0.3 * pp.gen_pmax
    want = central.solve_central_packed(pp, gen_ramp=(up, down), gen_budget=(lo, hi))
    assert want.objective > alone.objective * (1.0 + 1e-6)                         # the ramps bind at the optimum
    h = pair_engine(hip_api, pp, (up, down), None, (lo, hi), max_iters=20000, gamma=0.3)
    done, conv = h.iterate(20000)
    st = state_of(h)
    gap = abs(float(st["cost"][0]) - want.objective) / want.objective
    cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
    viol = max(max(budget_violation(st["P"][g], lo[g], hi[g]), ramp_infeasibility(st["P"][g], cap[g], up[g], down[g]))
               / max(1.0, float(pp.gen_pmax[g])) for g in range(pp.G))
    print(f"converged {conv} after {done} iterations, relative cost gap {gap:.2e}, largest budget / ramp violation {viol:.2e} (scaled), "
          f"LP {want.objective:.4f} (budgets alone {alone.objective:.4f}, neither {free.objective:.4f})")
    assert conv
    assert viol <= 1e-9, viol
    assert gap <= 1e-3, gap
    assert h.solver_failures() == 0


# ---- two shards against one context; the packed route -------------------------------------------------------------------------------------

def _close(got, want, keys, who):
    for key in keys:
        if want[key].size:
            assert np.abs(got[key] - want[key]).max() <= 1e-9 * max(1.0, np.abs(want[key]).max()), (key, who)


def test_multi_two_shards_equal_one_context(hip_api):
    pp = swing(synth.synthetic_case(41, 7, 6, seed=4))
    g = 1.0 / (pp.G + pp.S)
    warm = make_engine(hip_api, pp, eps=0.0, gamma=g, flags=CHAIN)
    warm.iterate(4)
    lo, hi = draw_budgets(row_sums(warm.get_primal()[0]), row_sums(np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)))
    up = down = 0.15 * pp.gen_pmax
    ref = pair_engine(hip_api, pp, (up, down), None, (lo, hi), eps=0.0, gamma=g)
    q = copy.copy(pp)
    q.gen_budget, q.gen_ramp = (lo, hi), (up, down)              # (through engine_kwargs: both words and both setters from the constructor)
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(eps=0.0, gamma=g, flags=_capi.F_COMM_HOST), **q.engine_kwargs())
    assert m.flags2 == BUDGET | PAIR
    for k in (1, 4, 7):
        ref.iterate(k)
        assert m.iterate(k) == (k, False)
        want = state_of(ref)
        P, D, C, E = m.get_primal()
        _close(dict(P=P, D=D, C=C, E=E), want, ("P", "D", "C", "E"), "primal")
        for i in range(2):
            _close(state_of(m.shard(i)), want, ("lam", "inj", "cost"), i)
    cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
    assert max(max(budget_violation(P[i], lo[i], hi[i]), ramp_infeasibility(P[i], cap[i], up[i], down[i])) for i in range(pp.G)) \
        <= 1e-9 * float(pp.gen_pmax.max())
    assert ref.solver_failures() == 0
    m.close()


def test_a_packed_case_with_both_constraints_builds_through_admm(hip_api):
    from conftest import pkg
    n = pkg.Node("N", [10, 10, 50, 10, 30], True)
    gens = [pkg.Generator("A", 1, 100, "k", n, energy_max=60.0, ramp_up=15.0, ramp_down=15.0),
            pkg.Generator("B", 5, 100, "k", n, ramp_up=30.0, ramp_down=30.0)]
    a = admm.ADMM(0.5, [n], gens, [], [], backend=hip_api, record=False, max_iters=5000)
    assert a.engine.flags2 == BUDGET | PAIR == 9 and a.engine.params.flags & RAMP
    a.engine.iterate(5000)
    P = a.engine.get_primal()[0]
    assert budget_violation(P[0], 0.0, 60.0) <= 1e-7 and ramp_infeasibility(P[0], 100.0, 15.0, 15.0) <= 1e-7
    assert a.engine.solver_failures() == 0
    # Engine.roll, the host route of ramp and budget contexts, keeps working: the anchor and what is left of the budget move on
    e = a.engine
    used = P[:, :1].sum(axis=1)
    e.roll(1, np.array([[20.0]]))
    assert e.flags2 == 9 and np.array_equal(e._mirror["gen_prev"], P[:, 0])
    assert np.array_equal(e._mirror["gen_budget"][1], np.maximum(0.0, np.array([60.0, np.inf]) - used))
    e.iterate(3)
    assert e.solver_failures() == 0
