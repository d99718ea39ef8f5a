"""Storage initial levels (DOPF_F_STO_INITIAL_LEVEL, dopf_set_storage_initial_level): the flag alone changes nothing against
DOPF_F_STO_GENERAL, the setter's refusals, exactness of every storage body with a level before timestep 0 (certificate after
every iteration), the bodies against each other, the optimum against the central LP with the same level, a rolling horizon,
dopf_set_state and the multi-context form. Needs a real MI355X: pytest -m gpu."""
import numpy as np
import pytest

import decentralopf_jl_amd as pkg
from decentralopf_jl_amd import _capi, synth
from decentralopf_jl_amd.central import solve_central_packed
from helpers import make_engine, max_diff, state_of, storage_kkt_violation

pytestmark = pytest.mark.gpu

IL, GEN, LH = _capi.F_STO_INITIAL_LEVEL, _capi.F_STO_GENERAL, _capi.F_LONG_HORIZON
NET = dict(N=4, L=5, seed=50, fmax_factor=0.7, fmax_min=5)


def bitwise_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def set_from(e, st, iteration):
    e.set_state(P=st["P"], D=st["D"], C_=st["C"], avg_U=st["avg_U"], avg_K=st["avg_K"], lam=st["lam"], mu=st["mu"],
                rho=st["rho"], iteration=iteration)


def draw_levels(pp, seed):
    """A third of the storages at 0, a third full, a third inside the band."""
    rng = np.random.default_rng(seed)
    kind = rng.permutation(np.arange(pp.S) % 3)
    return np.where(kind == 0, 0.0, np.where(kind == 1, pp.sto_emax, rng.uniform(0.05, 0.95, pp.S) * pp.sto_emax))


def with_empty_storages(pp, every=5):
    """Every `every`-th storage gets max_level 0 (it can only pass energy through within a timestep)."""
    em = pp.sto_emax.copy()
    em[::every] = 0.0
    pp.sto_emax = em
    return pp


def certify_steps(e, pp, e0, gamma, n):
    """n single iterations; after each, every storage passes the QP certificate under e0 and E = e0 + cumsum(C - D)."""
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
        theta = lam_used[None, :] + gamma * (s_prev[None, :] - (before["D"] - before["C"]))
        viol = storage_kkt_violation(pp, np.arange(pp.S), before["D"], before["C"], D, C, E, theta, gamma)
        assert viol <= 1e-7, (k, viol)
    assert e.solver_failures() == 0


# ---- 1. the flag alone is DOPF_F_STO_GENERAL ------------------------------------------------------------------------------

CHAIN = [("copper-T24", dict(n_gen=40, n_sto=12, T=24, seed=301), 0, 0.02),
         ("copper-T96", dict(n_gen=40, n_sto=12, T=96, seed=302), 0, 0.02),
         ("net-4x5-T24", dict(n_gen=20, n_sto=8, T=24, **NET), 0, 0.03),
         ("copper-T600-long", dict(n_gen=20, n_sto=6, T=600, seed=303), LH, 0.02)]


@pytest.mark.parametrize("name,case,extra,gamma", CHAIN, ids=[c[0] for c in CHAIN])
def test_flag_without_setter_is_the_general_body_bit_for_bit(hip_api, name, case, extra, gamma):
    pp = synth.synthetic_case(**case)
    runs = []
    for flags, zero_call in ((GEN | extra, False), (IL | extra, False), (IL | extra, True)):
        e = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=flags)
        if zero_call:
            e.set_initial_levels(np.zeros(pp.S))
        e.iterate(10)
        runs.append(state_of(e))
        assert e.solver_failures() == 0
    assert bitwise_equal(runs[0], runs[1])
    assert bitwise_equal(runs[0], runs[2])


# ---- 2. refusals --------------------------------------------------------------------------------------------------------

def test_setter_refusals(hip_api):
    pp = synth.synthetic_case(30, 6, 24, seed=311)
    e = make_engine(hip_api, pp, eps=0.0, gamma=0.02)
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*DOPF_F_STO_INITIAL_LEVEL"):
        e.set_initial_levels(np.zeros(pp.S))
    good = 0.5 * pp.sto_emax
    a = make_engine(hip_api, pp, eps=0.0, gamma=0.02, flags=IL)
    b = make_engine(hip_api, pp, eps=0.0, gamma=0.02, flags=IL)
    a.set_initial_levels(good)
    b.set_initial_levels(good)
    a.iterate(3)
    b.iterate(3)
    for bad_value in (np.nan, -1.0, None):
        bad = good.copy()
        bad[2] = pp.sto_emax[2] + 1.0 if bad_value is None else bad_value
        with pytest.raises(_capi.DopfError, match=r"\(-1\)"):
            a.set_initial_levels(bad)
    a.iterate(5)
    b.iterate(5)
    assert bitwise_equal(state_of(a), state_of(b))


# ---- 3. exactness of every body ----------------------------------------------------------------------------------------

EXACT = [("warm-T24", 24, 0), ("warm-T96", 96, 0), ("scan-T250", 250, 0), ("scan-T512", 512, 0),
         ("scan-T96-no-warm", 96, _capi.F_NO_WARM_START), ("long-T96", 96, _capi.F_DEBUG_LONG_STO), ("long-T600", 600, LH)]


@pytest.mark.parametrize("name,T,extra", EXACT, ids=[x[0] for x in EXACT])
def test_every_iteration_is_certified_under_the_initial_level(hip_api, name, T, extra):
    pp = with_empty_storages(synth.synthetic_case(40, 15, T, seed=320 + T))
    e0 = draw_levels(pp, seed=T)
    gamma = 0.02
    e = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=IL | extra)
    e.set_initial_levels(e0)
    certify_steps(e, pp, e0, gamma, 12)


# ---- 4. the bodies agree --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,case,gamma", [("copper-T96", dict(n_gen=40, n_sto=12, T=96, seed=331), 0.02),
                                             ("net-4x5-T96", dict(n_gen=20, n_sto=8, T=96, **NET), 0.03)],
                         ids=["copper-T96", "net-4x5-T96"])
def test_warm_scan_and_long_bodies_agree(hip_api, name, case, gamma):
    """From the same state (the warm body's run) one step of each body, 20 times."""
    pp = synth.synthetic_case(**case)
    e0 = draw_levels(pp, seed=332)
    engines = [make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=IL | f)
               for f in (0, _capi.F_NO_WARM_START, _capi.F_DEBUG_LONG_STO)]
    for e in engines:
        e.set_initial_levels(e0)
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

def check_levels(e, pp, e0):
    _, D, C, E = e.get_primal()
    assert E.min() >= -1e-9 and (E - pp.sto_emax[:, None]).max() <= 1e-9
    assert np.abs(E[:, 0] - (e0 + C[:, 0] - D[:, 0])).max() <= 1e-9


# The three-node case: with the reference's literals (gamma 0.3, flow weight 10) the ADMM converges from an empty battery (476
# iterations) but cycles once the battery starts with energy (lambda residual ~19 at e0 = 20 after 20 000 iterations; the warm
# and the scan body give the same bits, so the x-updates are not the cause); so does gamma 0.01 .. 0.05 with weight 10. gamma 0.02
# with flow weight 3 converges at e0 = 0, 7 and 20 alike (2 156 iterations each). DESIGN.md section 5h.
THREE_NODE = dict(gamma=0.02, w_flow=3.0)


@pytest.mark.parametrize("level", [20.0, 7.0, 0.0])
def test_three_node_case_reaches_the_lp_with_an_initial_level(hip_api, three_node, level):
    *_, pp = three_node
    e0 = np.array([level])
    want = solve_central_packed(pp, initial_level=e0).objective
    e = _capi.Engine(hip_api, params=_capi.default_params(max_iters=5000, **THREE_NODE), sto_e0=e0, **pp.engine_kwargs())
    done, conv = e.iterate(5000)
    assert conv, done
    cost = e.get_consensus()[4]
    assert abs(cost - want) / want < 1e-3, (cost, want, done)
    check_levels(e, pp, e0)
    assert e.solver_failures() == 0


@pytest.mark.parametrize("name", ["copper-T24", "network-12x18-T12"])
def test_synthetic_cases_reach_the_lp_with_initial_levels(hip_api, name):
    if name == "copper-T24":
        pp = synth.synthetic_case(300, 30, 24, seed=341)
        kw = {}
    else:
        pp = synth.synthetic_case(300, 30, 12, N=12, L=18, seed=23, fmax_factor=1.5, fmax_min=20)
        kw = dict(w_flow=0.3 / (pp.G + pp.S))
    e0 = draw_levels(pp, seed=342)
    want = solve_central_packed(pp, duals=False, initial_level=e0).objective
    assert want < solve_central_packed(pp, duals=False).objective        # the stored energy is worth something
    A = pp.G + pp.S
    e = make_engine(hip_api, pp, gamma=1.0 / A, max_iters=5000, flags=IL, **kw)
    e.set_initial_levels(e0)
    done, conv = e.iterate(5000)
    assert conv, done
    cost = e.get_consensus()[4]
    assert abs(cost - want) / want < 1e-3, (cost, want, done)
    check_levels(e, pp, e0)
    assert e.solver_failures() == 0


# ---- 6. rolling horizon ---------------------------------------------------------------------------------------------------

def test_rolling_horizon_continues_from_the_level_reached(hip_api):
    pp = synth.synthetic_case(300, 30, 24, seed=351)
    A = pp.G + pp.S
    gamma = 1.0 / A
    e = make_engine(hip_api, pp, gamma=gamma, max_iters=0, flags=IL)
    done, conv = e.iterate(5000)
    assert conv, done
    _, D, C, E = e.get_primal()
    e1 = np.clip(E[:, 11], 0.0, pp.sto_emax)             # the level reached at step 12 starts the next window
    assert np.ptp(e1) > 0.0
    e.set_initial_levels(e1)
    e.set_state(iteration=1)                             # a new window: the stop test starts again (primal and duals kept)
    certify_steps(e, pp, e1, gamma, 1)
    done, conv = e.iterate(5000)
    assert conv, done
    want = solve_central_packed(pp, duals=False, initial_level=e1).objective
    cost = e.get_consensus()[4]
    assert abs(cost - want) / want < 1e-3, (cost, want, done)
    check_levels(e, pp, e1)
    assert e.solver_failures() == 0


# ---- 7. set_state, the Python front end and the multi-context form ------------------------------------------------------------

def test_set_state_levels_start_from_the_initial_level(hip_api):
    pp = synth.synthetic_case(30, 8, 48, seed=361)
    e0 = draw_levels(pp, seed=362)
    src = make_engine(hip_api, pp, eps=0.0, gamma=0.02, flags=IL)
    src.set_initial_levels(e0)
    src.iterate(6)
    st = state_of(src)
    dst = make_engine(hip_api, pp, eps=0.0, gamma=0.02, flags=IL)
    dst.set_initial_levels(e0)
    set_from(dst, st, src.get_residuals()[3])
    E = dst.get_primal()[3]
    assert np.abs(E - (e0[:, None] + np.cumsum(st["C"] - st["D"], axis=1))).max() <= 1e-12
    assert np.array_equal(E, st["E"])


def test_python_front_end_takes_the_level_from_the_storages(hip_api, three_node):
    nodes, lines, gens, _, _ = three_node
    stos = [pkg.Storage("battery", 1, 10, 20, "purple", nodes[0], initial_level=20.0)]
    admm = pkg.ADMM(THREE_NODE["gamma"], nodes, gens, stos, lines, record=False, max_iters=5000, w_flow=THREE_NODE["w_flow"])
    pkg.run(admm)
    want = solve_central_packed(admm.packed).objective
    assert abs(admm.results[-1].total_costs - want) / want < 1e-3
    assert admm.results[-1].of(stos[0]).level[0] == pytest.approx(20.0 + admm.results[-1].of(stos[0]).charge[0]
                                                                   - admm.results[-1].of(stos[0]).discharge[0], abs=1e-9)
    admm.set_initial_levels([0.0])                        # back to the reference's empty start
    admm.set_initial_levels(None)


@pytest.mark.parametrize("n", [2, 3])
def test_multi_context_matches_one_context(hip_api, n):
    pp = synth.synthetic_case(40, 11, 24, seed=371)
    e0 = draw_levels(pp, seed=372)
    kw = dict(eps=0.0, gamma=1.0 / (pp.G + pp.S))
    ref = make_engine(hip_api, pp, flags=IL, **kw)
    ref.set_initial_levels(e0)
    ref.iterate(12)
    want = state_of(ref)
    runs = []
    for _ in range(2):
        m = _capi.MultiEngine(hip_api, n, params=_capi.default_params(flags=IL | _capi.F_COMM_HOST, **kw), **pp.engine_kwargs())
        m.set_initial_levels(e0)
        assert m.iterate(12) == (12, False)
        runs.append(m.get_primal())
        m.close()
    for a, b in zip(runs[0], (want["P"], want["D"], want["C"], want["E"])):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    # a refusal on any shard leaves every shard as it was
    m = _capi.MultiEngine(hip_api, n, params=_capi.default_params(flags=IL | _capi.F_COMM_HOST, **kw), **pp.engine_kwargs())
    bad = e0.copy()
    bad[-1] = -1.0
    with pytest.raises(_capi.DopfError, match=r"\(-1\)"):
        m.set_initial_levels(bad)
    m.close()
