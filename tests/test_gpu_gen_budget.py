"""DOPF_F2_GEN_ENERGY_BUDGET on the GPU: the generators' step under energy budgets (k_gen_budget) against the NumPy
reference row by row and against its one-multiplier optimality certificate, on copper plates and networks; the bits of the flagless
chain with every budget at its default; the setter and the create rules of the second flag word; convergence to the host LP with
budget rows; two shards against one context; and Engine.roll's host route. On networks the steps' derivatives come from the closed
forms of DESIGN.md section 3 (helpers_ramp_net.net_step_pieces), never from the device's tables."""
import copy
import ctypes

import numpy as np
import pytest

from decentralopf_jl_amd import _capi, central, synth
from helpers import draw_profiles, make_engine, set_from, state_of
from helpers_budget import (BUDGET, CHAIN, budget_engine, budget_kkt_violation, budget_project, budget_violation, draw_budgets,
                            draw_budgets_by_state, plate_steps, row_sums)
from helpers_quadratic import QC, draw_c2, params_of
from helpers_ramp import step_centres
from helpers_ramp_net import net_step_pieces, phi_gen

pytestmark = pytest.mark.gpu
AV = _capi.F_GEN_AVAILABILITY
LONG = _capi.F_LONG_HORIZON
WIDE = _capi.F_DEBUG_WIDE_NET
RAMP = _capi.F_GEN_RAMP
GAMMA, W_FLOW = 0.3, 10.0                    # networks: the reference's parameters (what net_step_pieces is given)
NET_PRM = dict(eps=0.0, gamma=GAMMA)
NET_CHAIN = _capi.F_NO_FUSE                  # the chain a network runs under the flag (plan_chain: no k_net_agents)


def swing(pp, lo=0.4, hi=1.6):
    """the case with its demand alternating between lo and hi times itself (the ramp tests'): a row's timesteps differ"""
    f = np.where(np.arange(pp.T) % 2 == 0, lo, hi)
    pp.demand = np.round(np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T) * f[None, :])
    return pp


# name -> (case, flags, warm-up iterations of the flagless twin)
# The warm-up runs on the flagless twin, so the state of the compared step is the one a CPU oracle run reaches (plain runs: settled
# there). 7x5: six iterations — until then two of the seven rows sit at their caps, where no e_min can bind.
SHAPES = {
    "7x5": (lambda: swing(synth.synthetic_case(7, 0, 5, seed=3)), 0, 6),
    "9xT1": (lambda: synth.synthetic_case(9, 0, 1, seed=4), 0, 2),
    "70+6xT96-3-nodes": (lambda: swing(synth.synthetic_case(70, 6, 96, N=3, seed=8)), 0, 3),
    "11+2xT130": (lambda: swing(synth.synthetic_case(11, 2, 130, seed=9)), 0, 3),
    "3xT600-long": (lambda: swing(synth.synthetic_case(3, 0, 600, seed=7)), LONG, 3),
    "net-12xT4-N6-L8": (lambda: swing(synth.synthetic_case(12, 0, 4, N=6, L=8, seed=2)), 0, 3),
    "net-12+3xT70-N6-L8": (lambda: swing(synth.synthetic_case(12, 3, 70, N=6, L=8, seed=2)), 0, 3),
    "net-12xT4-wide-chain": (lambda: swing(synth.synthetic_case(12, 0, 4, N=6, L=8, seed=2)), WIDE, 3),
}
EXTRAS = {"plain": (False, False), "availability": (True, False), "c2": (False, True), "availability+c2": (True, True)}


def _profiles(pp, rng):
    """helpers.draw_profiles' three profiles; on a one-step horizon its zeros (every fourth step, so t = 0, and a fifth of the others)
    would leave every row with a profile a box of one point, with nothing to project: those get a value in [0.2, 1] instead"""
    prof, of = draw_profiles(pp, "K3", rng)
    if pp.T == 1:
        prof = np.where(prof == 0.0, rng.uniform(0.2, 1.0, prof.shape), prof)
    return prof, of


def _prm(pp):
    return NET_PRM if pp.L else params_of(pp)


def _chain(pp):
    return NET_CHAIN if pp.L else CHAIN


def _steps(pp, c2, before, prm):
    """steps[g][t] = (xk, vk, sl) of every generator row from the state the solve reads"""
    if pp.L:
        return net_step_pieces(pp, c2, before, GAMMA, W_FLOW)
    c, q = step_centres(pp, c2, before, prm["gamma"])
    return [plate_steps(c[g], q[g]) for g in range(pp.G)]


def _grad(pp, c2, before, prm, P):
    if pp.L:
        return phi_gen(pp, c2, before, GAMMA, W_FLOW, P)
    d = P - before["P"]
    return pp.gen_mc[:, None] + np.asarray(c2)[:, None] * P + before["lam"][None, :] + prm["gamma"] * (before["inj"].sum(axis=0)[None, :] + d) + d


def _setup(hip_api, name, extra, eager):
    """(pp, prm, budget engine, flagless twin on the chain, c2, cap, steps, e_min, e_max, state before): both engines in the twin's
    warm-up state (a warm-up with default budgets is a flagless run), the budgets drawn from the clamped step's sums there: the four
    classes (free, e_max = 0.6 S, e_min = S + 0.4 (sum cap - S), equality at 0.8 S) dealt to the rows from their own state
    (helpers_budget.draw_budgets_by_state), so that the shares the test asserts hold with availability and c2 too"""
    make, flags, warm = SHAPES[name]
    avail, quad = EXTRAS[extra]
    pp = make()
    prm = _prm(pp)
    rng = np.random.default_rng(17)
    c2 = draw_c2(pp.G, rng) if quad else np.zeros(pp.G)
    flags |= (AV if avail else 0) | (QC if quad else 0) | (_capi.F_NO_GRAPH if eager else 0)
    h = budget_engine(hip_api, pp, flags=flags, **prm)
    twin = make_engine(hip_api, pp, flags=flags | _chain(pp), **prm)
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
    st, it = state_of(twin), twin.get_residuals()[3]
    for e in (h, twin):
        set_from(e, st, it)
    before = state_of(h)
    steps = _steps(pp, c2, before, prm)
    S = row_sums([budget_project(steps[g], cap[g]) for g in range(pp.G)])
    lo, hi, _ = draw_budgets_by_state(S, row_sums(cap))
    h.set_energy_budget(lo, hi)
    return pp, prm, h, twin, c2, cap, steps, lo, hi, before


CASES = [(n, x) for n in SHAPES for x in EXTRAS]


@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
@pytest.mark.parametrize("name,extra", CASES, ids=[f"{n}-{x}" for n, x in CASES])
def test_one_step_against_the_reference_and_the_certificate(hip_api, name, extra, eager):
    """One step from the twin's warm-up state: P against budget_project row by row (1e-9 scaled by max(1, gen_pmax), the parity tests'
    bound for a primal value), the certificate of every row at 1e-8 (one nu per row, its sign against the bound met), the budget
    itself within 1e-9 scaled, D and C the bits of the flagless twin on the chain, no solver failure. At least a fifth of the rows
    bind above, a fifth below and a fifth are free, according to the reference, on every run."""
    pp, prm, h, twin, c2, cap, steps, lo, hi, before = _setup(hip_api, name, extra, eager)
    h.iterate(1)
    twin.iterate(1)
    after, other = state_of(h), state_of(twin)
    grad = _grad(pp, c2, before, prm, after["P"])
    worst = cert = viol = 0.0
    sides = []
    for g in range(pp.G):
        info = {}
        want = budget_project(steps[g], cap[g], lo[g], hi[g], info)
        sides.append(info["side"])
        scale = max(1.0, float(pp.gen_pmax[g]))
        worst = max(worst, float(np.abs(after["P"][g] - want).max()) / scale)
        infeas, stat, nu = budget_kkt_violation(after["P"][g], grad[g], cap[g], lo[g], hi[g])
        cert = max(cert, stat)
        viol = max(viol, budget_violation(after["P"][g], lo[g], hi[g]) / scale)
        assert infeas <= 1e-9 * scale, (g, infeas)
        if info["side"] == 0:
            assert np.array_equal(after["P"][g], other["P"][g]), g          # a row that keeps its budget: the clamped step's bits
    above, below, free = sides.count(1), sides.count(-1), sides.count(0)
    print(f"{name} {extra}: |P - reference| {worst:.2e} (scaled), certificate {cert:.2e}, budget violation {viol:.2e} (scaled), rows "
          f"binding above {above}/{pp.G}, below {below}/{pp.G}, free {free}/{pp.G}")
    assert 5 * above >= pp.G and 5 * below >= pp.G and 5 * free >= pp.G, (above, below, free, pp.G)
    assert worst <= 1e-9, worst
    assert cert <= 1e-8, cert
    assert viol <= 1e-9, viol
    assert np.array_equal(after["D"], other["D"]) and np.array_equal(after["C"], other["C"])      # the storages do not see the budgets
    assert h.solver_failures() == 0


def test_projected_steps_reach_the_deltas_the_slack_sums_read(hip_api):
    """DOPF_F_KEEP_DELTAS on the network: the slack sums then walk the agents through P - p0 of the PROJECTED step (dltG). The run must
    agree with the one that forms those sums without the deltas, within the bound for two chains (1e-9 scaled)"""
    pp = SHAPES["net-12xT4-N6-L8"][0]()
    runs = []
    for keep in (0, _capi.F_KEEP_DELTAS):
        h = budget_engine(hip_api, pp, flags=keep, **NET_PRM)
        h.iterate(3)
        cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
        S = row_sums([budget_project(s, cap[g]) for g, s in enumerate(_steps(pp, np.zeros(pp.G), state_of(h), NET_PRM))])
        h.set_energy_budget(*draw_budgets(S, row_sums(cap)))
        h.iterate(6)
        assert h.solver_failures() == 0
        runs.append(state_of(h))
    for k in ("P", "lam", "mu", "rho", "inj"):
        scale = max(1.0, float(np.abs(runs[0][k]).max()))
        assert float(np.abs(runs[0][k] - runs[1][k]).max()) <= 1e-9 * scale, k


# ---- every budget at its default: the bits of the flagless chain ---------------------------------------------------------------------

FREE = [("copper-odd-T25", lambda: synth.synthetic_case(200, 16, 25, seed=702), 0, True),
        ("copper-odd-T5", lambda: synth.synthetic_case(9, 4, 5, seed=5), 0, True),
        ("copper-even-T24", lambda: synth.synthetic_case(300, 24, 24, seed=701), 0, False),
        ("copper-T600-long", lambda: synth.synthetic_case(3, 0, 600, seed=7), LONG, False),
        ("net-12+3xT70", lambda: synth.synthetic_case(12, 3, 70, N=6, L=8, seed=2), 0, True),
        ("net-12xT4-wide", lambda: synth.synthetic_case(12, 0, 4, N=6, L=8, seed=2), WIDE, True)]


@pytest.mark.parametrize("extra", list(EXTRAS))
@pytest.mark.parametrize("name,make,flags,bitwise", FREE, ids=[r[0] for r in FREE])
def test_default_budgets_are_the_flagless_chain(hip_api, name, make, flags, bitwise, extra):
    """One step from the same state: the same bits of P on every shape. 25 iterations: every array's bits where the flagless context
    runs k_gen_update itself on that chain (odd T, networks); on an even-T plate it runs the pair kernels, whose sums add in another
    order: 1e-9 scaled there, as in the ramp tests."""
    avail, quad = EXTRAS[extra]
    pp = make()
    prm = _prm(pp)
    rng = np.random.default_rng(5)
    flags |= (AV if avail else 0) | (QC if quad else 0)
    h = budget_engine(hip_api, pp, flags=flags, **prm)
    ref = make_engine(hip_api, pp, flags=flags | _chain(pp), **prm)
    if avail:
        prof, of = draw_profiles(pp, "K3", rng)
        for e in (h, ref):
            e.set_availability(prof, of)
    if quad:
        c2 = draw_c2(pp.G, rng)
        for e in (h, ref):
            e.set_quadratic_cost(c2)
    ref.iterate(3)
    st, it = state_of(ref), ref.get_residuals()[3]
    for e in (h, ref):
        set_from(e, st, it)
    h.iterate(1)
    ref.iterate(1)
    assert np.array_equal(state_of(h)["P"], state_of(ref)["P"])
    h.iterate(24)
    ref.iterate(24)
    a, b = state_of(h), state_of(ref)
    if bitwise or quad:                          # (DOPF_F_GEN_QUADRATIC_COST contexts run k_gen_update on every shape)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    else:
        for k in ("P", "D", "C", "lam", "inj"):
            if b[k].size:
                scale = max(1.0, float(np.abs(b[k]).max()))
                assert float(np.abs(a[k] - b[k]).max()) <= 1e-9 * scale, k
    assert h.solver_failures() == 0


# ---- the setter -------------------------------------------------------------------------------------------------------------------------

def _small():
    return swing(synth.synthetic_case(7, 0, 5, seed=3))


def test_setter_refusals_store_nothing(hip_api):
    pp = _small()
    prm = params_of(pp)
    G, T = pp.G, pp.T
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*DOPF_F2_GEN_ENERGY_BUDGET"):        # DOPF_E_UNSUPPORTED
        make_engine(hip_api, pp, **prm).set_energy_budget(np.zeros(G), np.ones(G))
    lo, hi = 0.5 * pp.gen_pmax, 3.0 * pp.gen_pmax
    prof, of = np.full((1, T), 0.75), np.zeros(G, dtype=np.int32)
    h, twin = (budget_engine(hip_api, pp, (lo, hi), flags=AV, **prm) for _ in range(2))
    for e in (h, twin):
        e.set_availability(prof, of)
        e.iterate(3)

    def bad(a, g, v):
        x = a.copy()
        x[g] = v
        return x
    for args, what in (((bad(lo, 2, np.nan), hi), r"e_min\[2\]"), ((bad(lo, 5, -1e-3), hi), r"e_min\[5\]"),
                       ((bad(lo, 1, np.inf), None), r"e_min\[1\]"), ((lo, bad(hi, 4, np.nan)), r"e_max\[4\]"),
                       ((None, bad(hi, 3, -1.0)), r"e_max\[3\]"), ((lo, bad(hi, 0, 0.4 * pp.gen_pmax[0])), r"e_min\[0\].*e_max\[0\]"),
                       ((bad(lo, 6, 0.76 * T * pp.gen_pmax[6]), None), r"g = 6 ")):        # above sum_t cap = 0.75 T pmax
        with pytest.raises(_capi.DopfError, match=r"\(-1\).*" + what):                     # DOPF_E_INVALID, naming the entry
            h.set_energy_budget(*args)
    # the availability setter's re-check: generator 6's caps drop to 0.05 pmax in every step, 0.25 pmax over the window, under its
    # e_min = 0.5 pmax
    low = np.vstack([prof, np.full((1, T), 0.05)])
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_availability.*g = 6 "):
        h.set_availability(low, bad(of, 6, 1))
    assert h.iterate(5) == twin.iterate(5)
    a, b = state_of(h), state_of(twin)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_setter_between_graph_replays_resets_converged_and_null_restores_the_defaults(hip_api):
    pp = _small()
    prm = params_of(pp)
    h = budget_engine(hip_api, pp, **prm)
    h.iterate(16)
    P = h.get_primal()[0]
    for budget in (draw_budgets(row_sums(P), row_sums(np.repeat(pp.gen_pmax[:, None], pp.T, axis=1))), (None, None)):                            # None: back to 0 and +inf
        st, it = state_of(h), h.get_residuals()[3]
        h.set_energy_budget(*budget)
        assert h.get_residuals()[3] == it                                           # the iteration counter is kept
        now = state_of(h)
        for k in ("P", "lam", "inj"):
            assert np.array_equal(now[k], st[k]), k
        fresh = budget_engine(hip_api, pp, None if budget[0] is None else budget, **prm)
        for e in (h, fresh):                                                        # (both from the getters' values: the same node sums)
            set_from(e, st, it)
        h.iterate(4)
        fresh.iterate(4)
        a, b = state_of(h), state_of(fresh)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    ref = make_engine(hip_api, pp, flags=CHAIN, **prm)                              # the defaults again: the flagless chain's bits (odd T)
    st, it = state_of(h), h.get_residuals()[3]
    for e in (h, ref):
        set_from(e, st, it)
    h.iterate(3)
    ref.iterate(3)
    assert np.array_equal(state_of(h)["P"], state_of(ref)["P"])
    # converged is reset
    pp = synth.synthetic_case(7, 0, 5, seed=3)                                      # (the case without the swing: it converges)
    e = budget_engine(hip_api, pp, gamma=1.0 / pp.G, max_iters=20000)
    done, conv = e.iterate(20000)
    assert conv and e.iterate(5) == (0, True)
    it = e.get_residuals()[3]
    e.set_energy_budget(None, 0.5 * e.get_primal()[0].sum(axis=1))
    assert e.sync() == (it, False)


# ---- create -----------------------------------------------------------------------------------------------------------------------------

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


def test_create_rules_of_the_second_word(hip_api):
    pp = _small()
    rc, msg = _create_ex(hip_api, pp, 0, 4)
    assert rc == -1 and "unknown bit 4" in msg                                      # DOPF_E_INVALID, naming the bit
    rc, msg = _create_ex(hip_api, pp, RAMP, BUDGET)
    assert rc == -4 and "DOPF_F2_GEN_ENERGY_BUDGET" in msg and "DOPF_F_GEN_RAMP" in msg          # DOPF_E_UNSUPPORTED
    net = synth.synthetic_case(12, 0, 4, N=6, L=8, seed=2)
    rc, msg = _create_ex(hip_api, net, RAMP | _capi.F_GEN_RAMP_NETWORK, BUDGET)
    assert rc == -4 and "DOPF_F2_GEN_ENERGY_BUDGET" in msg
    assert _create_ex(hip_api, pp, 0, BUDGET)[0] == 0 and _create_ex(hip_api, net, 0, BUDGET)[0] == 0
    h = budget_engine(hip_api, pp, **params_of(pp))
    h.iterate(2)
    tail = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, :1]
    rc = h.api.roll_horizon(h._ctx, 1, _capi._dp(_capi._f64(tail.T)))
    assert rc == -4 and b"DOPF_F2_GEN_ENERGY_BUDGET" in h.api.last_error(h._ctx)


@pytest.mark.parametrize("name", ["9+4xT6", "net-12+3xT4"])
def test_create_and_create_ex_with_a_zero_word_give_equal_bits(hip_api, name):
    """dopf_create is dopf_create_ex(..., 0): the chains with the fused launches and the one-launch tail included"""
    pp = synth.synthetic_case(9, 4, 6, seed=5) if name == "9+4xT6" else synth.synthetic_case(12, 3, 4, N=6, L=8, seed=2)
    prm = _prm(pp)
    a = make_engine(hip_api, pp, **prm)
    api = copy.copy(hip_api)                 # the constructor's create, through the new entry with a zero word
    api._create = lambda *args: hip_api.create_ex(*args, 0)
    b = _capi.Engine(api, params=_capi.default_params(**prm), **pp.engine_kwargs())
    assert b.flags2 == 0
    a.iterate(5)
    b.iterate(5)
    sa, sb = state_of(a), state_of(b)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k


# ---- convergence to the host LP with budget rows ------------------------------------------------------------------------------------------

def _net_conv():
    from conftest import pkg
    nodes, lines, gens, stos = pkg.three_node_case()
    return pkg.pack(nodes, gens, stos, lines)


# name -> (case, parameters, the generator whose energy is held (None: the one that delivers most in the free optimum), to which share)
# three-node network: the wind unit to 90 % — coal, the largest, cannot be cut at all: the lines leave t = 2 no other supply (the LP
# with 0.97 of its energy is infeasible)
CONV = {"7x5": (lambda: swing(synth.synthetic_case(7, 0, 5, seed=3), 0.85, 1.15), dict(gamma=0.3), None, 0.7),
        "three-node-network": (_net_conv, dict(), 1, 0.9)}


@pytest.mark.parametrize("name", list(CONV))
def test_converged_run_against_the_host_lp(hip_api, name):
    """The cost bound of the ramp and quadratic-cost convergence tests (within 1e-3 of the central optimum), 1e-9 scaled for the
    budgets, which the projection keeps in every iteration. The budgets: one generator is held to a share of the energy it delivers in
    the free optimum (e_max), and the one that uses least of its capacity there (of the others) must deliver a tenth of its
    capacity's energy more (e_min) — both change the optimum (asserted: more than 1e-6 relative). Default parameters but for gamma on
    the plate (0.3, as the ramp test's). Iterations to the stop test, measured on an MI355X: the plate 51 (cost within 2.5e-6 of the LP's 73 028; 72 730 without budgets), the three-node
    network 469 (within 2.0e-5 of 14 675; 14 035 without)."""
    make, prm, held, share = CONV[name]
    pp = make()
    free = central.solve_central_packed(pp)
    E = free.generation.sum(axis=1)
    room = pp.T * pp.gen_pmax
    lo, hi = np.zeros(pp.G), np.full(pp.G, np.inf)
    big = int(np.argmax(E)) if held is None else held
    hi[big] = share * E[big]
    small = int(np.argmin(np.where(np.arange(pp.G) == big, np.inf, E / room)))
    lo[small] = E[small] + 0.1 * room[small]
    want = central.solve_central_packed(pp, gen_budget=(lo, hi))
    assert want.objective > free.objective * (1.0 + 1e-6)                          # the budgets bind at the optimum
    h = budget_engine(hip_api, pp, (lo, hi), max_iters=20000, **prm)               # (eps: the reference's 1e-3)
    done, conv = h.iterate(20000)
    st = state_of(h)
    gap = abs(float(st["cost"][0]) - want.objective) / want.objective
    viol = max(budget_violation(st["P"][g], lo[g], hi[g]) / max(1.0, float(pp.gen_pmax[g])) for g in range(pp.G))
    print(f"{name}: converged {conv} after {done} iterations, relative cost gap {gap:.2e}, largest budget violation {viol:.2e} (scaled), "
          f"LP {want.objective:.4f} (without budgets {free.objective:.4f})")
    assert conv
    assert viol <= 1e-9, viol
    assert gap <= 1e-3, gap
    assert h.solver_failures() == 0


# ---- two shards against one context -------------------------------------------------------------------------------------------------------

def _close(got, want, keys, who):
    for key in keys:
        if want[key].size:
            assert np.abs(got[key] - want[key]).max() <= 1e-9 * max(1.0, np.abs(want[key]).max()), (key, who)


def _sharding_case(hip_api):
    pp = swing(synth.synthetic_case(41, 7, 6, seed=4))
    g = 1.0 / (pp.G + pp.S)
    warm = make_engine(hip_api, pp, eps=0.0, gamma=g, flags=CHAIN)
    warm.iterate(4)
    lo, hi = draw_budgets(row_sums(warm.get_primal()[0]), row_sums(np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)))
    return pp, g, lo, hi


def test_multi_two_shards_equal_one_context(hip_api):
    pp, g, lo, hi = _sharding_case(hip_api)
    ref = budget_engine(hip_api, pp, (lo, hi), eps=0.0, gamma=g)
    q = copy.copy(pp)
    q.gen_budget = (lo, hi)                                      # (through engine_kwargs: the second word and the setter from the constructor)
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(eps=0.0, gamma=g, flags=_capi.F_COMM_HOST), **q.engine_kwargs())
    assert m.flags2 & BUDGET
    for k in (1, 4, 7):
        ref.iterate(k)
        assert m.iterate(k) == (k, False)
        want = state_of(ref)
        P, D, C, E = m.get_primal()
        _close(dict(P=P, D=D, C=C, E=E), want, ("P", "D", "C", "E"), "primal")
        for i in range(2):
            _close(state_of(m.shard(i)), want, ("lam", "inj", "cost"), i)
    assert max(budget_violation(P[i], lo[i], hi[i]) for i in range(pp.G)) <= 1e-9 * float(pp.gen_pmax.max())
    bad = lo.copy()
    bad[pp.G - 1] = -1.0                                         # the second shard's last entry: nothing stored on the first either
    with pytest.raises(_capi.DopfError, match="shard 1"):
        m.set_energy_budget(bad, hi)
    ref.iterate(3)
    assert m.iterate(3) == (3, False)
    _close(state_of(m.shard(0)), state_of(ref), ("lam", "inj", "cost"), "after a refusal")
    m.set_energy_budget(None, None)
    ref.set_energy_budget(None, None)
    ref.iterate(3)
    m.iterate(3)
    _close(state_of(m.shard(1)), state_of(ref), ("lam", "inj", "cost"), "reset")
    m.close()


def test_sharded_admm_two_ranks_equal_one_context(hip_api):
    import torch
    from conftest import pkg
    pp, g, lo, hi = _sharding_case(hip_api)
    ref = budget_engine(hip_api, pp, (lo, hi), eps=0.0, gamma=g)
    q = copy.copy(pp)
    q.gen_budget = (lo, hi)                                      # every rank's engine gets the word and its slice from engine_kwargs
    ranks = [pkg.ShardedADMM(q, r, 2, all_reduce=lambda: None, eps=0.0, gamma=g) for r in range(2)]
    for sh in ranks:
        assert sh.engine.flags2 & BUDGET
        sh.set_energy_budget(lo, hi)                             # all G values: each rank takes its slice
    for _ in range(12):
        for sh in ranks:
            sh.engine.local_update()
        for sh in ranks:
            sh.sync()
        total = ranks[0]._tensor.cpu() + ranks[1]._tensor.cpu()          # (summed on the host: no PyTorch kernel has to load)
        for sh in ranks:
            sh._tensor.copy_(total)
        torch.cuda.synchronize()
        for sh in ranks:
            sh.engine.apply_consensus()
        for sh in ranks:
            sh.sync()
    ref.iterate(12)
    want = state_of(ref)
    got = [state_of(sh.engine) for sh in ranks]
    for i, s in enumerate(got):
        _close(s, want, ("lam", "inj", "cost"), i)
    assert np.abs(np.concatenate([s["P"] for s in got]) - want["P"]).max() <= 1e-9 * max(1.0, np.abs(want["P"]).max())


# ---- Engine.roll on a budget context: the host route --------------------------------------------------------------------------------------

def test_engine_roll_carries_the_remaining_budgets(hip_api):
    pp = _small()
    prm = params_of(pp)
    warm = make_engine(hip_api, pp, flags=CHAIN, **prm)
    warm.iterate(20)
    lo, hi = draw_budgets(row_sums(warm.get_primal()[0]), row_sums(np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)))
    h = budget_engine(hip_api, pp, (lo, hi), **prm)
    h.iterate(20)
    P = h.get_primal()[0]
    k = 2
    tail = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, :k]
    h.roll(k, tail)
    used = P[:, :k].sum(axis=1)
    assert h.flags2 & BUDGET
    assert np.array_equal(h._mirror["gen_budget"][0], np.maximum(0.0, lo - used))
    assert np.array_equal(h._mirror["gen_budget"][1], np.maximum(0.0, hi - used))
    assert np.array_equal(h.get_primal()[0][:, :pp.T - k], P[:, k:])           # the window moved
    h.iterate(1)
    P1 = h.get_primal()[0]
    nlo, nhi = h._mirror["gen_budget"]
    assert max(budget_violation(P1[g], nlo[g], nhi[g]) for g in range(pp.G)) <= 1e-9 * float(pp.gen_pmax.max())
    # a remaining minimum the new window's caps cannot deliver (a table put into the mirror by hand: the engine itself would have
    # refused it): the rebuilt context's setter refuses, and the call says so
    h2 = budget_engine(hip_api, pp, (np.where(np.arange(pp.G) == 0, 0.99 * pp.T * pp.gen_pmax, 0.0), None), flags=AV, **prm)
    h2.iterate(3)
    h2._mirror["gen_avail"], h2._mirror["gen_avail_of"] = np.full((1, pp.T), 0.5), np.zeros(pp.G, dtype=np.int32)
    with pytest.raises(_capi.DopfError, match=r"g = 0 "):
        h2.roll(1, tail[:, :1])
