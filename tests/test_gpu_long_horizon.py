"""Storages on horizons beyond 512 timesteps (DOPF_F_LONG_HORIZON, csrc/sto_long.h): the refusal without the flag, the flag as
a no-op below 513, the long body against the one-wave bodies (DOPF_F_DEBUG_LONG_STO) and against the oracle, an hourly and a
half-hourly year, the launch chains, determinism, the getters and the failure path. Needs a real MI355X: pytest -m gpu."""
import numpy as np
import pytest

import decentralopf_jl_amd as pkg
from decentralopf_jl_amd import _capi, synth
from decentralopf_jl_amd.network import Generator, Node, Storage
from helpers import make_engine, max_diff, state_of, storage_kkt_violation

pytestmark = pytest.mark.gpu

LH, DBG = _capi.F_LONG_HORIZON, _capi.F_DEBUG_LONG_STO
NET = dict(N=4, L=5, seed=50, fmax_factor=0.7, fmax_min=5)


def bitwise_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def set_from(e, st, iteration):
    e.set_state(P=st["P"], D=st["D"], C_=st["C"], avg_U=st["avg_U"], avg_K=st["avg_K"], lam=st["lam"], mu=st["mu"],
                rho=st["rho"], iteration=iteration)


def test_refusal_without_the_flag_is_kept(hip_api):
    with pytest.raises(_capi.DopfError, match="T <= 512") as ei:
        make_engine(hip_api, synth.synthetic_case(4, 2, 600))
    assert "DOPF_F_LONG_HORIZON" in str(ei.value)


@pytest.mark.parametrize("T", [24, 96, 250, 512])
def test_flag_changes_nothing_up_to_512(hip_api, T):
    pp = synth.synthetic_case(40, 8, T, seed=60 + T)
    runs = []
    for flags in (0, LH):
        e = make_engine(hip_api, pp, eps=0.0, gamma=0.02, flags=flags)
        e.iterate(10)
        runs.append(state_of(e))
        assert e.iterate_timed(1)["sto_long"] == 0
    assert bitwise_equal(*runs)


BODIES = [("copper-T24", dict(n_gen=30, n_sto=10, T=24, seed=71), 0.02),
          ("copper-T96", dict(n_gen=30, n_sto=10, T=96, seed=72), 0.02),
          ("copper-T168", dict(n_gen=30, n_sto=10, T=168, seed=73), 0.02),
          ("copper-T500", dict(n_gen=30, n_sto=10, T=500, seed=74), 0.02),
          ("net-4x5-T250", dict(n_gen=20, n_sto=6, T=250, **NET), 0.03)]


@pytest.mark.parametrize("name,case,gamma", BODIES, ids=[b[0] for b in BODIES])
def test_long_body_matches_the_one_wave_bodies(hip_api, name, case, gamma):
    """From the same state (the default bodies' free run), one step of each side."""
    pp = synth.synthetic_case(**case)
    ref = make_engine(hip_api, pp, eps=0.0, gamma=gamma)
    lng = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=DBG)
    for k in range(8):
        it = ref.get_residuals()[3]
        set_from(lng, state_of(ref), it)
        ref.iterate(1)
        lng.iterate(1)
        a, b = state_of(ref), state_of(lng)
        scale = max(1.0, float(np.abs(a["lam"]).max()))
        worst, where = max_diff(a, b, keys=[x for x in a if x != "cost"])
        assert worst <= 1e-9 * scale, (k, where, worst)
        assert abs(a["cost"][0] - b["cost"][0]) <= 1e-9 * max(1.0, abs(a["cost"][0]))
    assert lng.solver_failures() == 0 and ref.solver_failures() == 0
    assert lng.iterate_timed(1)["sto_long"] == 1


ORACLE = [("copper-T513", dict(n_gen=20, n_sto=6, T=513, seed=81), 0.02),
          ("copper-T600", dict(n_gen=20, n_sto=6, T=600, seed=82), 0.02),
          ("copper-T1000", dict(n_gen=20, n_sto=8, T=1000, seed=83), 0.02),
          ("copper-T2048-whole-tiles", dict(n_gen=20, n_sto=6, T=2048, seed=84), 0.02),
          ("copper-T2190-ragged-tile", dict(n_gen=20, n_sto=6, T=2190, seed=85), 0.02),
          ("storages-only-T1000", dict(n_gen=0, n_sto=8, T=1000, seed=86), 0.05),
          ("net-4x5-T600", dict(n_gen=20, n_sto=6, T=600, **NET), 0.03),
          ("net-4x5-T1000", dict(n_gen=20, n_sto=6, T=1000, **NET), 0.03),
          ("net-40x60-T700", dict(n_gen=60, n_sto=8, T=700, N=40, L=60, seed=51, fmax_factor=0.8, fmax_min=5), 0.02)]


@pytest.mark.parametrize("name,case,gamma", ORACLE, ids=[o[0] for o in ORACLE])
def test_long_body_one_step_parity_with_the_oracle(hip_api, oracle_api, name, case, gamma):
    """test_hip_one_step_parity's protocol from a state in which the storages cycle: 12 free iterations of the library, then
    every step from the oracle's state."""
    pp = synth.synthetic_case(**case)
    h = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=LH)
    o = make_engine(oracle_api, pp, mode=1, eps=0.0, gamma=gamma)
    h.iterate(12)
    set_from(o, state_of(h), h.get_residuals()[3])
    touched = np.zeros(2, dtype=bool)
    for k in range(4):
        h.iterate(1)
        o.iterate(1)
        sh, so = state_of(h), state_of(o)
        scale = max(1.0, float(np.abs(so["lam"]).max()))
        worst, where = max_diff(sh, so, keys=[x for x in sh if x != "cost"])
        assert worst <= 1e-8 * scale, (k, where, worst)
        assert abs(sh["cost"][0] - so["cost"][0]) <= 1e-9 * max(1.0, abs(so["cost"][0]))
        E, em = so["E"], pp.sto_emax[:, None]
        touched |= [bool((E <= 1e-9).any()), bool((E >= em - 1e-9).any())]
        set_from(h, so, o.get_residuals()[3])
    assert h.solver_failures() == 0
    # the storages cycled: both bounds were met (storages alone cannot fill up against the demand: empty contacts only)
    assert touched.all() if pp.G > 0 else touched[0], touched


@pytest.mark.parametrize("T", [8760, 17520])
def test_hourly_and_half_hourly_year(hip_api, T):
    pp = synth.synthetic_case(40, 6, T, seed=91)
    gamma = 0.02
    e = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=LH)
    e.iterate(20)
    before = state_of(e)
    e.iterate(1)
    after = state_of(e)
    assert e.solver_failures() == 0
    lam_used = e.get_duals_used()[0]
    s_prev = before["inj"].sum(axis=0)
    D, C, E = after["D"], after["C"], after["E"]
    em = pp.sto_emax[:, None]
    assert E.min() >= -1e-9 and (E - em).max() <= 1e-9
    assert np.abs(np.cumsum(C - D, axis=1) - E).max() < 1e-8
    theta = lam_used[None, :] + gamma * (s_prev[None, :] - (before["D"] - before["C"]))
    assert storage_kkt_violation(pp, np.arange(pp.S), before["D"], before["C"], D, C, E, theta, gamma) < 1e-6
    contacts = ((E <= 1e-9) | (E >= em - 1e-9)).sum(axis=1)
    assert contacts.min() >= 100, contacts


@pytest.mark.parametrize("case", [dict(n_gen=30, n_sto=8, T=1000, seed=95), dict(n_gen=20, n_sto=6, T=1000, **NET)],
                         ids=["copper", "net-4x5"])
def test_chains_determinism_and_resume(hip_api, case):
    pp = synth.synthetic_case(**case)
    kw = dict(eps=0.0, gamma=0.03)
    runs = []
    for flags in (LH, LH, LH | _capi.F_NO_GRAPH, LH | _capi.F_OVERLAP_AGENTS):
        e = make_engine(hip_api, pp, flags=flags, **kw)
        e.iterate(9)
        runs.append(state_of(e))
    for r in runs[1:]:
        assert bitwise_equal(runs[0], r)
    # set_state + iterate continues the run
    a = make_engine(hip_api, pp, flags=LH, **kw)
    a.iterate(6)
    mid, it = state_of(a), a.get_residuals()[3]
    b = make_engine(hip_api, pp, flags=LH, **kw)
    set_from(b, mid, it)
    a.iterate(3)
    b.iterate(3)
    sa, sb = state_of(a), state_of(b)
    worst, where = max_diff(sa, sb, keys=[x for x in sa if x != "cost"])
    assert worst <= 1e-9 * max(1.0, float(np.abs(sa["lam"]).max())), (where, worst)
    assert a.solver_failures() == 0 and b.solver_failures() == 0


def test_getters_on_a_long_network(hip_api):
    pp = synth.synthetic_case(n_gen=20, n_sto=6, T=1000, **NET)
    h = make_engine(hip_api, pp, eps=0.0, gamma=0.03, flags=LH | _capi.F_KEEP_DELTAS)
    h.iterate(7)
    eb_s, up_s, lo_s = h.get_penalty_sums()
    acc = np.zeros((3, pp.T))
    for a in range(pp.G + pp.S):
        acc += np.asarray(h.get_agent_penalty(a))
    for got, want in zip((eb_s, up_s, lo_s), acc):
        assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
    U, K = h.get_agent_slacks(pp.G)                 # a storage's slacks
    assert U.shape == (pp.L, pp.T) and K.shape == (pp.L, pp.T)
    assert h.solver_failures() == 0


def test_root_cap_surfaces_as_an_error(hip_api):
    pp = synth.synthetic_case(20, 6, 1000, seed=97)
    e = make_engine(hip_api, pp, eps=0.0, gamma=0.02, flags=LH | _capi.F_DEBUG_ROOT_CAP)
    with pytest.raises(_capi.DopfError, match="tolerance"):
        for _ in range(30):
            e.iterate(1)
    assert e.solver_failures() > 0


def test_python_front_end_runs_an_hourly_year(hip_api):
    T = 8760
    t = np.arange(1, T + 1)
    node = Node("n1", [int(v) for v in np.round(900.0 * (1.0 + 0.3 * np.sin(2.0 * np.pi * t / 24.0)))], True)
    gens = [Generator(f"g{i}", 5 + 7 * i, 150 + 40 * i, "black", node) for i in range(8)]
    stos = [Storage(f"s{i}", 1 + i % 3, 10 + 3 * i, 2 * (10 + 3 * i), "blue", node) for i in range(6)]
    admm = pkg.ADMM(0.02, [node], gens, stos, [], record=False, max_iters=5, flags=LH)
    pkg.run(admm)
    assert admm.iteration == 6
    assert admm.engine.solver_failures() == 0
    E = np.asarray([admm.results[-1].of(s).level for s in stos])
    assert E.shape == (6, T) and E.min() >= -1e-9
    assert (E - np.asarray([s.max_level for s in stos])[:, None]).max() <= 1e-9
