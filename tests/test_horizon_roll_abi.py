"""dopf_set_demand / dopf_roll_horizon without a GPU: the library exports both, horizon.shift_window — the rule in
executable form — gives the documented table entry by entry, and a backend without the entries (the CPU oracle) rolls by the host
route: getters -> shift_window -> a new context with the setters and set_state(iteration = 2)."""
import ctypes

import numpy as np
import pytest

from conftest import build_oracle
from decentralopf_jl_amd import ADMM, _capi, calculate_iteration, shift_window, synth
from decentralopf_jl_amd.network import Generator, Node, Storage
from helpers import engine, set_from, state_of


def test_library_exports_both_entries_and_the_binding_knows_them():
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    assert hasattr(lib, "dopf_set_demand") and hasattr(lib, "dopf_roll_horizon")
    api = _capi.CApi(_capi.HIP_LIB_PATH, "dopf_")
    assert api.roll_horizon.argtypes == [ctypes.c_void_p, ctypes.c_int32, _capi.c_double_p]
    assert api.set_demand.argtypes == [ctypes.c_void_p, _capi.c_double_p]


def test_the_oracle_has_no_counterpart():
    from oracle.binding import OracleApi
    api = OracleApi(build_oracle(), features=True)
    assert not hasattr(api, "roll_horizon") and not hasattr(api, "set_demand")


def hand_made():
    """T = 5, N = 2, L = 1, G = 2, S = 1: every entry distinct"""
    T = 5
    t = np.arange(T, dtype=np.float64)
    return dict(demand=np.array([100.0 + t, 200.0 + t]), P=np.array([10.0 + t, 20.0 + t]), D=np.array([1.0 + t]),
                C=np.array([0.5 + t]), E=np.array([[3.0, 7.5, -0.25, 9.0, 4.0]]), lam=-1.0 - t, mu=np.array([0.1 * (t + 1)]),
                rho=np.array([0.2 * (t + 1)]), avg_U=np.array([0.3 * (t + 1)]), avg_K=np.array([0.4 * (t + 1)]),
                sto_emax=np.array([7.0]))


def test_shift_window_gives_the_table_entry_by_entry():
    s = hand_made()
    k, T = 2, 5
    tail = np.array([[1000.0, 1001.0], [2000.0, 2001.0]])
    w = shift_window(k, tail, **s)
    for t in range(T):
        old = t + k
        for n in range(2):
            assert w["demand"][n, t] == (s["demand"][n, old] if t < T - k else tail[n, t - (T - k)])
        for g in range(2):
            assert w["P"][g, t] == (s["P"][g, old] if t < T - k else s["P"][g, T - 1])          # persistence
        assert w["D"][0, t] == (s["D"][0, old] if t < T - k else 0.0)
        assert w["C"][0, t] == (s["C"][0, old] if t < T - k else 0.0)
        assert w["lam"][t] == (s["lam"][old] if t < T - k else s["lam"][T - 1])
        for name in ("mu", "rho", "avg_U", "avg_K"):
            assert w[name][0, t] == (s[name][0, old] if t < T - k else s[name][0, T - 1]), name
    assert w["e0"].tolist() == [7.0]                        # E[0, k-1] = 7.5 clamped to max_level
    assert shift_window(3, np.zeros((2, 3)), **s)["e0"].tolist() == [0.0]     # E[0, 2] = -0.25 clamped to 0
    assert shift_window(1, np.zeros((2, 1)), **s)["e0"].tolist() == [3.0]
    u = shift_window(k, tail, used=dict(lam=s["lam"] * 2, mu=s["mu"] * 2), **s)["used"]
    assert u["lam"].tolist() == (2 * np.array([-3.0, -4.0, -5.0, -5.0, -5.0])).tolist() and u["mu"][0, 3] == s["mu"][0, 4] * 2


def test_shift_window_reads_the_c_layouts_as_the_getters_reshape_them():
    """[n + N*t] (demand, tail) and [t + T*g] (rows): flat buffers of the C ABI, brought to Julia shape the way Engine does"""
    s = hand_made()
    N, T, k = 2, 5, 2
    flat_demand = s["demand"].T.ravel()                    # [n + N*t]
    flat_tail = np.array([1000.0, 2000.0, 1001.0, 2001.0])  # [n + N*j]
    flat_P = s["P"].ravel()                                # [t + T*g]
    w = shift_window(k, flat_tail.reshape(k, N).T, **dict(s, demand=flat_demand.reshape(T, N).T, P=flat_P))
    assert w["demand"].T.ravel().tolist() == [102.0, 202.0, 103.0, 203.0, 104.0, 204.0, 1000.0, 2000.0, 1001.0, 2001.0]
    assert w["P"].ravel().tolist() == [12.0, 13.0, 14.0, 14.0, 14.0, 22.0, 23.0, 24.0, 24.0, 24.0]


@pytest.mark.parametrize("k", [0, 5, -1])
def test_shift_window_refuses_k_outside_the_window(k):
    with pytest.raises(ValueError):
        shift_window(k, np.zeros((2, max(k, 0))), **hand_made())


def test_shift_window_refuses_a_nan_tail():
    with pytest.raises(ValueError):
        shift_window(1, np.array([[np.nan], [0.0]]), **hand_made())


@pytest.fixture(scope="module")
def fapi():
    from oracle.binding import OracleApi
    return OracleApi(build_oracle(), features=True)


@pytest.mark.parametrize("case,k", [(dict(n_gen=9, n_sto=3, T=6, seed=11), 2),
                                    (dict(n_gen=8, n_sto=3, T=5, N=3, L=3, seed=12, fmax_factor=0.7, fmax_min=5), 1)],
                         ids=["copper", "net"])
def test_engine_roll_on_the_oracle_takes_the_host_route(fapi, case, k):
    """bit for bit a fresh oracle engine of the shifted problem with the same set_state"""
    pp = synth.synthetic_case(**case)
    IL = _capi.F_STO_INITIAL_LEVEL
    a = engine(fapi, pp, 1, flags=IL, eps=0.0, gamma=0.05)
    a.iterate(7)
    before = state_of(a)
    tail = np.arange(pp.N * k, dtype=np.float64).reshape(pp.N, k) + 50.0
    w = shift_window(k, tail, demand=pp.demand, sto_emax=pp.sto_emax,
                     **{n: before[n] for n in ("P", "D", "C", "E", "lam", "mu", "rho", "avg_U", "avg_K")})
    a.roll(k, tail)
    assert np.array_equal(a.demand(), w["demand"]) and a.get_residuals()[3] == 2
    pp2 = synth.synthetic_case(**case)
    pp2.demand = w["demand"]
    b = engine(fapi, pp2, 1, flags=IL, eps=0.0, gamma=0.05)
    b.set_initial_levels(w["e0"])
    set_from(b, w, 2)
    for n in (0, 1):
        sa, sb = state_of(a), state_of(b)
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), (n, key)
        a.iterate(1)
        b.iterate(1)
    assert np.array_equal(state_of(a)["E"][:, 0], w["e0"] + state_of(a)["C"][:, 0] - state_of(a)["D"][:, 0])


def test_the_host_route_refuses_storages_without_the_flag_as_the_entry_does(fapi):
    pp = synth.synthetic_case(n_gen=4, n_sto=2, T=4, seed=2)
    e = engine(fapi, pp, 1, eps=0.0, gamma=0.05)
    e.iterate(3)
    before = state_of(e)
    with pytest.raises(_capi.DopfError, match="DOPF_F_STO_INITIAL_LEVEL"):
        e.roll(1, np.full((pp.N, 1), 50.0))
    for key, val in state_of(e).items():
        assert np.array_equal(val, before[key]), key


def little_case(T=4):
    n = Node("N", [float(60 + 10 * t) for t in range(T)], True)
    gens = [Generator("a", 3, 50, "x", n), Generator("b", 30, 100, "x", n)]
    stos = [Storage("s", 1, 10, 20, "x", n, initial_level=5.0)]
    return [n], gens, stos, []


def test_admm_roll_on_the_oracle_keeps_the_host_mirrors_in_step(fapi):
    nodes, gens, stos, lines = little_case()
    admm = ADMM(0.3, nodes, gens, stos, lines, backend=fapi, backend_mode=1, max_iters=50)
    for _ in range(5):
        calculate_iteration(admm)
    E = admm.results[-1].of(stos[0]).level
    lam_last = admm.lambdas[-1].copy()
    admm.roll(1, [[123.0]])
    assert nodes[0].demand == [70.0, 80.0, 90.0, 123.0] and admm.total_demand.tolist() == [70.0, 80.0, 90.0, 123.0]
    assert admm.node_id_to_demand == {1: [70.0, 80.0, 90.0, 123.0]}
    assert admm.iteration == 2 and admm.results == [] and not admm.convergence.all and len(admm.lambdas) == 1
    assert admm.lambdas[0].tolist() == lam_last[1:].tolist() + [lam_last[-1]]
    # a fresh ADMM of the shifted problem with the same state gives the same next iteration, bit for bit
    n2 = Node("N", [70.0, 80.0, 90.0, 123.0], True)
    g2 = [Generator("a", 3, 50, "x", n2), Generator("b", 30, 100, "x", n2)]
    s2 = [Storage("s", 1, 10, 20, "x", n2)]
    fresh = ADMM(0.3, [n2], g2, s2, [], backend=fapi, backend_mode=1, max_iters=50, flags=_capi.F_STO_INITIAL_LEVEL)
    fresh.set_initial_levels([float(min(max(E[0], 0.0), 20.0))])
    set_from(fresh.engine, state_of(admm.engine), 2)
    calculate_iteration(admm)
    calculate_iteration(fresh)
    for key, val in state_of(admm.engine).items():
        assert np.array_equal(val, state_of(fresh.engine)[key]), key
    assert len(admm.results) == 1 and admm.iteration == 3


def test_engine_set_demand_needs_the_entry(fapi):
    pp = synth.synthetic_case(n_gen=4, n_sto=0, T=3, seed=1)
    e = engine(fapi, pp, 1)
    with pytest.raises(_capi.DopfError, match="no set_demand"):
        e.set_demand(pp.demand)
