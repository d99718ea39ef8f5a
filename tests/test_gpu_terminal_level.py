"""Storage terminal levels (DOPF_F_STO_TERMINAL_LEVEL, dopf_set_storage_terminal_level): the flag alone changes nothing against
DOPF_F_STO_GENERAL (nor, with DOPF_F_STO_INITIAL_LEVEL, against that flag alone), the setters' refusals, exactness of every
storage body with a band on the level after the last timestep (certificate after every iteration), the bodies against each other,
the optimum against the central LP with the same band, a rolling horizon, the Python front end and the multi-context form.
Needs a real MI355X: pytest -m gpu."""
import numpy as np
import pytest

import decentralopf_jl_amd as pkg
from decentralopf_jl_amd import _capi, synth
from decentralopf_jl_amd.central import solve_central_packed
from helpers import make_engine, max_diff, state_of, storage_kkt_violation_band

pytestmark = pytest.mark.gpu

TL, IL, GEN, LH = _capi.F_STO_TERMINAL_LEVEL, _capi.F_STO_INITIAL_LEVEL, _capi.F_STO_GENERAL, _capi.F_LONG_HORIZON
NET = dict(N=4, L=5, seed=50, fmax_factor=0.7, fmax_min=5)


def bitwise_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def set_from(e, st, iteration):
    e.set_state(P=st["P"], D=st["D"], C_=st["C"], avg_U=st["avg_U"], avg_K=st["avg_K"], lam=st["lam"], mu=st["mu"],
                rho=st["rho"], iteration=iteration)


def reachable(pp, e0):
    span = pp.T * pp.sto_pmax
    return np.maximum(0.0, e0 - span), np.minimum(pp.sto_emax, e0 + span)


def draw_levels(pp, seed):
    """A third of the storages at 0, a third full, a third inside the band."""
    rng = np.random.default_rng(seed)
    kind = rng.permutation(np.arange(pp.S) % 3)
    return np.where(kind == 0, 0.0, np.where(kind == 1, pp.sto_emax, rng.uniform(0.05, 0.95, pp.S) * pp.sto_emax))


def draw_bands(pp, e0, seed):
    """A mix, each reachable from e0: ">= target" bands [x, emax], equalities lo = hi, caps [0, x] below emax, bands inside, and
    the default band; storages with emax = 0 get [0, 0]."""
    rng = np.random.default_rng(seed)
    rlo, rhi = reachable(pp, e0)
    em = pp.sto_emax
    kind = rng.permutation(np.arange(pp.S) % 5)
    u = lambda a, b: a + rng.uniform(0.0, 1.0, pp.S) * (b - a)
    x = u(rlo, rhi)
    y = u(rlo, rhi)
    lo = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [u(0.0, rhi), x, 0.0, np.minimum(x, y)], 0.0)
    hi = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [em, x, u(rlo, em), np.maximum(x, y)], em)
    lo = np.where(em == 0.0, 0.0, lo)
    hi = np.where(em == 0.0, 0.0, hi)
    assert np.all((lo <= np.minimum(rhi, hi)) & (hi >= rlo)), "a drawn band is unreachable"
    return lo, hi


def with_empty_storages(pp, every=5):
    """Every `every`-th storage gets max_level 0 (it can only pass energy through within a timestep)."""
    em = pp.sto_emax.copy()
    em[::every] = 0.0
    pp.sto_emax = em
    return pp


def certify_steps(e, pp, e0, lo, hi, gamma, n):
    """n single iterations; after each, every storage passes the QP certificate under e0 and the band, E = e0 + cumsum(C - D) and
    E[:, T-1] lies in [lo, hi]."""
    for k in range(n):
        before = state_of(e)
        e.iterate(1)
        after = state_of(e)
        lam_used = e.get_duals_used()[0]
        s_prev = before["inj"].sum(axis=0)
        D, C, E = after["D"], after["C"], after["E"]
        em = pp.sto_emax[:, None]
        assert np.abs(E - (e0[:, None] + np.cumsum(C - D, axis=1))).max() <= 1e-9, k
        assert E.min() >= -1e-9 and (E - em).max() <= 1e-9, k
        assert (lo - E[:, -1]).max() <= 1e-9 and (E[:, -1] - hi).max() <= 1e-9, k
        theta = lam_used[None, :] + gamma * (s_prev[None, :] - (before["D"] - before["C"]))
        viol = storage_kkt_violation_band(pp, before["D"], before["C"], D, C, E, theta, gamma, lo, hi)
        assert viol <= 1e-7, (k, viol)
    assert e.solver_failures() == 0


# ---- 1. the flag alone is DOPF_F_STO_GENERAL; with the initial level, the default band is that flag alone --------------------

CHAIN = [("copper-T24", dict(n_gen=40, n_sto=12, T=24, seed=401), 0, 0.02),
         ("copper-T96", dict(n_gen=40, n_sto=12, T=96, seed=402), 0, 0.02),
         ("net-4x5-T24", dict(n_gen=20, n_sto=8, T=24, **NET), 0, 0.03),
         ("copper-T600-long", dict(n_gen=20, n_sto=6, T=600, seed=403), LH, 0.02)]


@pytest.mark.parametrize("name,case,extra,gamma", CHAIN, ids=[c[0] for c in CHAIN])
def test_flag_without_setter_is_the_general_body_bit_for_bit(hip_api, name, case, extra, gamma):
    pp = synth.synthetic_case(**case)
    runs = []
    for flags, call in ((GEN | extra, None), (TL | extra, None), (TL | extra, "null"), (TL | extra, "explicit")):
        e = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=flags)
        if call == "null":
            e.set_terminal_levels(None, None)
        elif call == "explicit":
            e.set_terminal_levels(np.zeros(pp.S), pp.sto_emax)
        e.iterate(10)
        runs.append(state_of(e))
        assert e.solver_failures() == 0
    for r in runs[1:]:
        assert bitwise_equal(runs[0], r)


@pytest.mark.parametrize("name,case,extra,gamma", CHAIN, ids=[c[0] for c in CHAIN])
def test_both_flags_with_the_default_band_are_the_initial_level_flag_bit_for_bit(hip_api, name, case, extra, gamma):
    pp = synth.synthetic_case(**case)
    e0 = draw_levels(pp, seed=404)
    runs = []
    for flags, explicit in ((IL | extra, False), (IL | TL | extra, False), (IL | TL | extra, True)):
        e = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=flags)
        e.set_initial_levels(e0)
        if explicit:
            e.set_terminal_levels(np.zeros(pp.S), pp.sto_emax)
        e.iterate(10)
        runs.append(state_of(e))
        assert e.solver_failures() == 0
    for r in runs[1:]:
        assert bitwise_equal(runs[0], r)


# ---- 2. refusals --------------------------------------------------------------------------------------------------------

def test_setter_refusals(hip_api):
    pp = synth.synthetic_case(30, 6, 24, seed=411)
    pp.sto_emax = pp.sto_emax.copy()
    pp.sto_emax[3] = 100.0 * pp.sto_pmax[3]             # beyond what 24 steps of pmax reach from either end
    S, em, pm = pp.S, pp.sto_emax, pp.sto_pmax
    e = make_engine(hip_api, pp, eps=0.0, gamma=0.02)
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*DOPF_F_STO_TERMINAL_LEVEL"):
        e.set_terminal_levels(np.zeros(S), em)
    e0 = 0.5 * em
    e0[3] = 80.0 * pm[3]
    lo, hi = 0.25 * em, 0.75 * em
    lo[3], hi[3] = 90.0 * pm[3], em[3]                  # reachable from 80 pmax, not from 0
    a, b = (make_engine(hip_api, pp, eps=0.0, gamma=0.02, flags=IL | TL) for _ in range(2))
    for x in (a, b):
        x.set_initial_levels(e0)
        x.set_terminal_levels(lo, hi)
        x.iterate(3)

    def bad(which, value):
        l2, h2 = lo.copy(), hi.copy()
        (l2 if which == "lo" else h2)[2] = value
        return l2, h2

    for l2, h2 in (bad("lo", np.nan), bad("hi", np.nan), bad("lo", -1.0), bad("hi", em[2] + 1.0), bad("lo", hi[2] + 1.0)):
        with pytest.raises(_capi.DopfError, match=r"\(-1\)"):
            a.set_terminal_levels(l2, h2)
    l2, h2 = lo.copy(), hi.copy()
    l2[3], h2[3] = 0.0, 50.0 * pm[3]                     # below the lowest end level reachable from 80 pmax (56 pmax)
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*unreachable"):
        a.set_terminal_levels(l2, h2)
    with pytest.raises(_capi.DopfError, match=r"\(-1\)"):
        a.set_terminal_levels(lo, None)
    e2 = e0.copy()
    e2[3] = 0.0                                          # the stored band [90, 100] pmax is out of reach from 0
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*unreachable"):
        a.set_initial_levels(e2)
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*unreachable"):
        a.set_initial_levels(None)
    a.iterate(5)
    b.iterate(5)
    assert bitwise_equal(state_of(a), state_of(b))


def test_initial_level_setter_without_the_terminal_flag_is_unchanged(hip_api):
    pp = synth.synthetic_case(30, 6, 24, seed=412)
    pp.sto_emax = pp.sto_emax.copy()
    pp.sto_emax[3] = 100.0 * pp.sto_pmax[3]
    e = make_engine(hip_api, pp, eps=0.0, gamma=0.02, flags=IL)
    e0 = 0.5 * pp.sto_emax
    e.set_initial_levels(e0)                              # any level in [0, emax]: no band to reach
    e.set_initial_levels(None)
    with pytest.raises(_capi.DopfError, match=r"\(-4\)"):
        e.set_terminal_levels(None, None)


# ---- 3. exactness of every body ----------------------------------------------------------------------------------------

EXACT = [("warm-T24", 24, 0), ("warm-T96", 96, 0), ("scan-T96-no-warm", 96, _capi.F_NO_WARM_START),
         ("scan-T24-leave", 24, _capi.F_DEBUG_LEAVE), ("scan-T96-leave", 96, _capi.F_DEBUG_LEAVE),
         ("long-T96", 96, _capi.F_DEBUG_LONG_STO), ("long-T600", 600, LH)]


@pytest.mark.parametrize("name,T,extra", EXACT, ids=[x[0] for x in EXACT])
@pytest.mark.parametrize("with_e0", [True, False], ids=["e0", "empty-start"])
def test_every_iteration_is_certified_under_the_band(hip_api, name, T, extra, with_e0):
    pp = with_empty_storages(synth.synthetic_case(40, 15, T, seed=420 + T))
    e0 = draw_levels(pp, seed=T) if with_e0 else np.zeros(pp.S)
    lo, hi = draw_bands(pp, e0, seed=T + 1)
    gamma = 0.02
    e = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=TL | (IL if with_e0 else 0) | extra)
    if with_e0:
        e.set_initial_levels(e0)
    e.set_terminal_levels(lo, hi)
    certify_steps(e, pp, e0, lo, hi, gamma, 12)


def test_a_band_that_moves_between_iterations_stays_certified(hip_api):
    pp = with_empty_storages(synth.synthetic_case(40, 15, 48, seed=425))
    e0 = draw_levels(pp, seed=426)
    gamma = 0.02
    e = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=TL | IL)
    e.set_initial_levels(e0)
    for k in range(4):
        lo, hi = draw_bands(pp, e0, seed=427 + k)
        e.set_terminal_levels(lo, hi)
        certify_steps(e, pp, e0, lo, hi, gamma, 3)


# ---- 4. the bodies agree --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,case,gamma", [("copper-T96", dict(n_gen=40, n_sto=12, T=96, seed=431), 0.02),
                                             ("net-4x5-T96", dict(n_gen=20, n_sto=8, T=96, **NET), 0.03)],
                         ids=["copper-T96", "net-4x5-T96"])
def test_warm_scan_and_long_bodies_agree(hip_api, name, case, gamma):
    """From the same state (the warm body's run) one step of each body, 20 times."""
    pp = synth.synthetic_case(**case)
    e0 = draw_levels(pp, seed=432)
    lo, hi = draw_bands(pp, e0, seed=433)
    engines = [make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=IL | TL | f)
               for f in (0, _capi.F_NO_WARM_START, _capi.F_DEBUG_LONG_STO)]
    for e in engines:
        e.set_initial_levels(e0)
        e.set_terminal_levels(lo, hi)
    ref = engines[0]
    for k in range(20):
        it = ref.get_residuals()[3]
        st = state_of(ref)
        for e in engines[1:]:
            set_from(e, st, it)
        for e in engines:
            e.iterate(1)
        a = state_of(ref)
        scale = max(1.0, float(np.abs(a["lam"]).max()))
        for e in engines[1:]:
            b = state_of(e)
            worst, where = max_diff(a, b, keys=[x for x in a if x != "cost"])
            assert worst <= 1e-9 * scale, (k, where, worst)
    assert engines[2].iterate_timed(1)["sto_long"] == 1
    assert all(e.solver_failures() == 0 for e in engines)


# ---- 5. the optimum -------------------------------------------------------------------------------------------------------

def check_levels(e, pp, e0, lo, hi):
    _, D, C, E = e.get_primal()
    assert E.min() >= -1e-9 and (E - pp.sto_emax[:, None]).max() <= 1e-9
    assert np.abs(E[:, 0] - (e0 + C[:, 0] - D[:, 0])).max() <= 1e-9
    assert (lo - E[:, -1]).max() <= 1e-9 and (E[:, -1] - hi).max() <= 1e-9


# The three-node case with the parameters DESIGN.md section 5h found for a charged battery (gamma 0.02, flow weight 3).
THREE_NODE = dict(gamma=0.02, w_flow=3.0)
LP = [(0.0, 0.0, 20.0, 14035.0), (0.0, 5.0, 20.0, 14440.0), (0.0, 10.0, 20.0, 14845.0), (0.0, 20.0, 20.0, 15675.0),
      (7.0, 7.0, 7.0, 14035.0), (20.0, 20.0, 20.0, 14805.0), (20.0, 10.0, 10.0, 13995.0)]


@pytest.mark.parametrize("e0,lo,hi,objective", LP, ids=[f"e0={x[0]:g}-[{x[1]:g},{x[2]:g}]" for x in LP])
def test_three_node_case_reaches_the_lp_with_a_band(hip_api, three_node, e0, lo, hi, objective):
    *_, pp = three_node
    e0a, loa, hia = np.array([e0]), np.array([lo]), np.array([hi])
    want = solve_central_packed(pp, initial_level=e0a, terminal_level=(loa, hia)).objective
    assert abs(want - objective) <= 1e-6 * objective
    e = _capi.Engine(hip_api, params=_capi.default_params(max_iters=5000, **THREE_NODE), sto_e0=e0a if e0 else None,
                     sto_end_lo=loa, sto_end_hi=hia, **pp.engine_kwargs())
    done, conv = e.iterate(5000)
    assert conv, done
    cost = e.get_consensus()[4]
    assert abs(cost - want) / want < 1e-3, (cost, want, done)
    check_levels(e, pp, e0a, loa, hia)
    assert e.solver_failures() == 0


@pytest.mark.parametrize("name", ["copper-T24", "network-12x18-T12"])
def test_synthetic_cases_reach_the_lp_with_bands(hip_api, name):
    if name == "copper-T24":
        pp = synth.synthetic_case(300, 30, 24, seed=441)
        kw = {}
    else:
        pp = synth.synthetic_case(300, 30, 12, N=12, L=18, seed=23, fmax_factor=1.5, fmax_min=20)
        kw = dict(w_flow=0.3 / (pp.G + pp.S))
    e0 = draw_levels(pp, seed=442)
    lo, hi = draw_bands(pp, e0, seed=443)
    want = solve_central_packed(pp, duals=False, initial_level=e0, terminal_level=(lo, hi)).objective
    A = pp.G + pp.S
    e = make_engine(hip_api, pp, gamma=1.0 / A, max_iters=5000, flags=IL | TL, **kw)
    e.set_initial_levels(e0)
    e.set_terminal_levels(lo, hi)
    done, conv = e.iterate(5000)
    assert conv, done
    cost = e.get_consensus()[4]
    assert abs(cost - want) / want < 1e-3, (cost, want, done)
    check_levels(e, pp, e0, lo, hi)
    assert e.solver_failures() == 0


# ---- 6. rolling horizon ---------------------------------------------------------------------------------------------------

def test_rolling_horizon_with_an_end_target_and_a_cyclic_window(hip_api):
    pp = synth.synthetic_case(300, 30, 24, seed=451)
    A = pp.G + pp.S
    gamma = 1.0 / A
    target = 0.5 * pp.sto_emax
    lo1, hi1 = target, pp.sto_emax.copy()
    e = make_engine(hip_api, pp, gamma=gamma, max_iters=0, flags=IL | TL)
    e.set_terminal_levels(lo1, hi1)                       # window 1: from empty, end at least half full
    done, conv = e.iterate(5000)
    assert conv, done
    zero = np.zeros(pp.S)
    want = solve_central_packed(pp, duals=False, initial_level=zero, terminal_level=(lo1, hi1)).objective
    assert want > solve_central_packed(pp, duals=False).objective      # the target binds
    cost = e.get_consensus()[4]
    assert abs(cost - want) / want < 1e-3, (cost, want, done)
    check_levels(e, pp, zero, lo1, hi1)
    e1 = np.clip(e.get_primal()[3][:, -1], 0.0, pp.sto_emax)            # window 2 starts where window 1 ended ...
    assert np.all(e1 >= target - 1e-9)
    e.set_terminal_levels(None, None)                     # (the old band may be out of reach of the new start: reset first)
    e.set_initial_levels(e1)
    e.set_terminal_levels(e1, e1)                         # ... and ends there again: a cyclic horizon
    e.set_state(iteration=1)
    certify_steps(e, pp, e1, e1, e1, gamma, 1)
    done, conv = e.iterate(5000)
    assert conv, done
    want = solve_central_packed(pp, duals=False, initial_level=e1, terminal_level=(e1, e1)).objective
    cost = e.get_consensus()[4]
    assert abs(cost - want) / want < 1e-3, (cost, want, done)
    check_levels(e, pp, e1, e1, e1)
    assert e.solver_failures() == 0


# ---- 7. the Python front end and the multi-context form --------------------------------------------------------------------

def test_python_front_end_takes_the_band_from_the_storages(hip_api, three_node):
    nodes, lines, gens, _, _ = three_node
    stos = [pkg.Storage("battery", 1, 10, 20, "purple", nodes[0], terminal_level_min=10.0)]
    mk = lambda: pkg.ADMM(THREE_NODE["gamma"], nodes, gens, stos, lines, record=False, max_iters=5000, w_flow=THREE_NODE["w_flow"])
    admm = mk()
    assert admm.engine.params.flags & TL
    e = _capi.Engine(hip_api, params=_capi.default_params(max_iters=5000, **THREE_NODE), sto_end_lo=[10.0], sto_end_hi=[20.0],
                     **pkg.pack(nodes, gens, [pkg.Storage("battery", 1, 10, 20, "purple", nodes[0])], lines).engine_kwargs())
    for _ in range(3):
        admm.engine.iterate(7)
        e.iterate(7)
        assert bitwise_equal(state_of(admm.engine), state_of(e))
    admm = mk()
    pkg.run(admm)
    want = solve_central_packed(admm.packed).objective
    assert abs(want - 14845.0) <= 1e-6 * 14845.0
    assert abs(admm.results[-1].total_costs - want) / want < 1e-3
    assert admm.results[-1].of(stos[0]).level[-1] >= 10.0 - 1e-9
    admm.set_terminal_levels([0.0], [20.0])               # back to the reference's free end
    admm.set_terminal_levels(None, None)


@pytest.mark.parametrize("n", [2, 3])
def test_multi_context_matches_one_context(hip_api, n):
    pp = synth.synthetic_case(40, 11, 24, seed=471)
    e0 = draw_levels(pp, seed=472)
    lo, hi = draw_bands(pp, e0, seed=473)
    kw = dict(eps=0.0, gamma=1.0 / (pp.G + pp.S))
    ref = make_engine(hip_api, pp, flags=IL | TL, **kw)
    ref.set_initial_levels(e0)
    ref.set_terminal_levels(lo, hi)
    ref.iterate(12)
    want = state_of(ref)
    runs = []
    for _ in range(2):
        m = _capi.MultiEngine(hip_api, n, params=_capi.default_params(flags=IL | TL | _capi.F_COMM_HOST, **kw),
                              **pp.engine_kwargs())
        m.set_initial_levels(e0)
        m.set_terminal_levels(lo, hi)
        assert m.iterate(12) == (12, False)
        runs.append(m.get_primal())
        m.close()
    for a, b in zip(runs[0], (want["P"], want["D"], want["C"], want["E"])):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    # a refusal on any shard leaves every shard as it was
    m = _capi.MultiEngine(hip_api, n, params=_capi.default_params(flags=IL | TL | _capi.F_COMM_HOST, **kw), **pp.engine_kwargs())
    m.set_initial_levels(e0)
    m.set_terminal_levels(lo, hi)
    bad = hi.copy()
    bad[-1] = pp.sto_emax[-1] + 1.0
    with pytest.raises(_capi.DopfError, match=r"\(-1\)"):
        m.set_terminal_levels(lo, bad)
    m.iterate(12)
    P, D, C, E = m.get_primal()
    assert np.abs(E - want["E"]).max() <= 1e-12 * max(1.0, np.abs(want["E"]).max())
    m.close()
