"""dopf_trace_*  on the GPU: slot i of a trace equals, bit for bit, what the getters return when called after that
iteration. Every comparison is np.array_equal. A case's reference — twelve single steps with every getter after each, under an
active trace — is computed once per problem and shared. Needs a real MI355X: pytest -m gpu."""
import functools
import re

import numpy as np
import pytest

from conftest import pkg
from decentralopf_jl_amd import ADMM, _capi, export_results, run, run_recorded, synth
from helpers import engine, state_of
from test_trace_layout_host import layout_twin

pytestmark = pytest.mark.gpu

K = 12
ALL = _capi.TRACE_ALL
NO_GRAPH, NO_QUIET = _capi.F_NO_GRAPH, _capi.F_NO_QUIET
SECTIONS = ("lam", "mu", "rho", "inj", "avg_U", "avg_K", "flow", "P", "D", "C", "E")
ROW = ("lam_res", "mu_res", "rho_res", "total_cost", "iteration", "converged")


def three_node():
    nodes, lines, gens, stos = pkg.three_node_case()
    return pkg.pack(nodes, gens, stos, lines)


def storages_only():
    """G = 0. The synthetic demand is a share of the generators' capacity, 0 here: a demand that changes sign over the day takes its
    place, so that the storages — and the duals — move"""
    pp = synth.synthetic_case(0, 6, 24, seed=904)
    pp.demand = np.round(10.0 * np.cos(2.0 * np.pi * np.arange(24) / 24.0))[None, :]
    return pp


# name -> (problem, parameters). net: 20 * 168 = 3360 node entries and 30 * 168 = 5040 line entries, beyond the 4096 of the one-block
# dual step: the one-launch dual kernel leaves the residuals as bit patterns, and the quiet chain may run
CASES = {
    "three": (three_node, dict()),
    "cp24": (lambda: synth.synthetic_case(40, 8, 24, seed=901), dict(eps=0.0, gamma=0.02)),
    "cp5": (lambda: synth.synthetic_case(40, 8, 5, seed=902), dict(eps=0.0, gamma=0.02)),
    "net": (lambda: synth.synthetic_case(60, 6, 168, N=20, L=30, seed=903, fmax_factor=0.7, fmax_min=5), dict(eps=0.0, gamma=0.03)),
    "g0": (lambda: storages_only(), dict(eps=0.0, gamma=0.02)),
    "s0": (lambda: synth.synthetic_case(40, 0, 24, seed=905), dict(eps=0.0, gamma=0.02)),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    return CASES[name][0]()


def make(hip_api, name, flags=0, **over):
    return engine(hip_api, problem(name), None, flags=flags, **dict(CASES[name][1], **over))


def getters(e):
    """every getter, in the trace's names"""
    s = state_of(e)
    a, b, c, it = e.get_residuals()
    conv = int(e.sync()[1])
    s.pop("cost")
    s.update(lam_res=a, mu_res=b, rho_res=c, total_cost=e.get_consensus()[4], iteration=it if conv else it - 1, converged=conv)
    return s


def same_slot(sl, i, want, keys=ROW + SECTIONS):
    for k in keys:
        assert np.array_equal(np.asarray(sl[k][i]), np.asarray(want[k])), (i, k)


_REF = {}


def reference(hip_api, name):
    """(the getters after each of K single steps, the K slots of the trace that was active meanwhile): once per problem"""
    if name not in _REF:
        e = make(hip_api, name)
        e.trace_begin(ALL, K)
        states = []
        for _ in range(K):
            assert e.iterate(1)[0] == 1
            states.append(getters(e))
        assert e.trace_info() == (ALL, K, K, K)
        _REF[name] = (states, e.trace_read(0, K))
        e.trace_end()
        e.close()
    return _REF[name]


# ---- 1. the same context, step by step -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_slots_are_the_getters_step_by_step(hip_api, name):
    states, sl = reference(hip_api, name)
    pp = problem(name)
    assert sl["P"].shape == (K, pp.G, pp.T) and sl["mu"].shape == (K, pp.L, pp.T) and sl["inj"].shape == (K, pp.N, pp.T)
    for i in range(K):
        same_slot(sl, i, states[i])
    assert sl["iteration"].tolist() == list(range(1, K + 1))
    assert any(np.any(sl["lam"][i] != sl["lam"][i + 1]) for i in range(K - 1))          # (the run moves)


@pytest.mark.parametrize("name", list(CASES))
def test_step_by_step_without_graphs(hip_api, name):
    _, ref = reference(hip_api, name)
    e = make(hip_api, name, flags=NO_GRAPH)
    e.trace_begin(ALL, K)
    for i in range(K):
        e.iterate(1)
        same_slot(e.trace_read(i, 1), 0, getters(e))
    sl = e.trace_read(0, K)
    for i in range(K):          # (and the eager chain's history is the graphs')
        same_slot(sl, i, {k: ref[k][i] for k in ROW + SECTIONS})
    e.close()          # (dopf_destroy frees the active trace)


# ---- 2. one call ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_one_call_records_the_same_history(hip_api, name):
    _, ref = reference(hip_api, name)
    e = make(hip_api, name, flags=NO_QUIET if problem(name).L else 0)
    e.trace_begin(ALL, K)
    assert e.iterate(K)[0] == K and e.trace_info() == (ALL, K, K, K)
    sl = e.trace_read(0, K)
    for i in range(K):
        same_slot(sl, i, {k: ref[k][i] for k in ROW + SECTIONS})
    same_slot(sl, K - 1, getters(e))
    e.trace_end()
    e.close()


@pytest.mark.parametrize("name", ["three", "net"])
def test_one_call_with_the_quiet_chain_allowed_ends_on_the_getters(hip_api, name):
    e = make(hip_api, name)
    e.trace_begin(ALL, K)
    assert e.iterate(K)[0] == K and e.trace_info()[2:] == (K, K)
    same_slot(e.trace_read(K - 1, 1), 0, getters(e))
    e.iterate(K)
    assert e.trace_info()[2:] == (K, 2 * K)
    same_slot(e.trace_read(K - 1, 1), 0, getters(e))
    e.trace_end()
    e.close()


@pytest.mark.parametrize("what", [0, _capi.TRACE_DUALS | _capi.TRACE_CONSENSUS, _capi.TRACE_PRIMAL])
def test_a_trace_of_some_sections(hip_api, what):
    _, ref = reference(hip_api, "cp5")
    e = make(hip_api, "cp5")
    e.trace_begin(what, K)
    e.iterate(K)
    sl = e.trace_read(0, K)
    have = [k for k in SECTIONS if k in sl]
    assert have == [k for k, bit in zip(SECTIONS, [1] * 3 + [2] * 4 + [4] * 4) if what & bit]
    for i in range(K):
        same_slot(sl, i, {k: ref[k][i] for k in ROW + SECTIONS}, keys=ROW + tuple(have))
    e.trace_end()
    e.close()


# ---- 3. the ring ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,one_call", [("three", True), ("cp5", False), ("net", True)])
def test_the_ring_keeps_the_last_slots(hip_api, name, one_call):
    _, ref = reference(hip_api, name)
    e = make(hip_api, name, flags=NO_QUIET if problem(name).L else 0)
    e.trace_begin(ALL, 5)
    if one_call:
        e.iterate(K)
    else:
        for _ in range(K):
            e.iterate(1)
    assert e.trace_info() == (ALL, 5, 5, K)
    sl = e.trace_read(0, 5)
    assert sl["iteration"].tolist() == [8, 9, 10, 11, 12]
    for i in range(5):
        same_slot(sl, i, {k: ref[k][7 + i] for k in ROW + SECTIONS})
    same_slot(e.trace_read(3, 2), 1, {k: ref[k][11] for k in ROW + SECTIONS})
    for first, n in ((0, 6), (5, 1), (4, 2), (-1, 1)):
        with pytest.raises(_capi.DopfError, match=r"\(-1\).*outside the 5 held"):
            e.trace_read(first, n)
    assert e.trace_read(5, 0)["iteration"].size == 0
    e.trace_end()
    e.close()


# ---- 4. a stop inside a call ---------------------------------------------------------------------------------------------------------
def test_a_converging_call_records_every_iteration_once(hip_api):
    e = make(hip_api, "three")
    e.trace_begin(0, 600)
    done, conv = e.iterate(600)
    assert (done, conv) == (476, True) and e.trace_info() == (0, 600, 476, 476)
    sl = e.trace_read(0, 476)
    assert sl["iteration"].tolist() == list(range(1, 477))          # (no slot twice, none missing)
    assert sl["converged"].tolist() == [0] * 475 + [1]
    a, b, c, it = e.get_residuals()
    assert (sl["lam_res"][-1], sl["mu_res"][-1], sl["rho_res"][-1], int(sl["iteration"][-1])) == (a, b, c, it) and it == 476
    assert sl["total_cost"][-1] == e.get_consensus()[4]
    assert e.iterate(5)[0] == 0 and e.trace_info()[3] == 476          # (halted: the no-ops rewrite the last slot with its own bytes)
    again = e.trace_read(0, 476)
    for k in ROW:
        assert np.array_equal(again[k], sl[k]), k
    e.trace_end()
    e.close()


def test_a_capped_call_stops_recording_at_the_cap(hip_api):
    _, ref = reference(hip_api, "three")
    e = make(hip_api, "three", max_iters=7)
    e.trace_begin(ALL, 600)
    assert e.iterate(600)[0] == 7 and e.trace_info() == (ALL, 600, 7, 7)
    sl = e.trace_read(0, 7)
    for i in range(7):
        same_slot(sl, i, {k: ref[k][i] for k in ROW + SECTIONS})
    e.trace_end()
    e.close()


# ---- 5. levels -----------------------------------------------------------------------------------------------------------------------
def test_levels_follow_the_stored_initial_levels_and_efficiencies(hip_api):
    pp = problem("cp24")
    rng = np.random.default_rng(5)
    e = engine(hip_api, pp, None, flags=_capi.F_STO_INITIAL_LEVEL | _capi.F_STO_EFFICIENCY, eps=0.0, gamma=0.02)
    e.set_efficiency(rng.uniform(0.8, 1.0, pp.S), rng.uniform(0.8, 1.0, pp.S))
    e0 = rng.uniform(0.1, 0.9, pp.S) * pp.sto_emax
    e.set_initial_levels(e0)
    e.trace_begin(_capi.TRACE_PRIMAL, 6)
    for i in range(6):
        e.iterate(1)
        P, D, Cc, E = e.get_primal()
        sl = e.trace_read(i, 1)
        assert np.array_equal(sl["E"][0], E) and np.array_equal(sl["D"][0], D) and np.array_equal(sl["P"][0], P)
    assert np.any(E[:, 0] != Cc[:, 0] - D[:, 0])          # (the stored levels and efficiencies are in E)
    # E is formed when read: under other initial levels the same slot's D and C give dopf_get_primal's recursion from those
    e.set_initial_levels(0.5 * e0)
    now = e.get_primal()[3]
    assert np.array_equal(e.trace_read(5, 1)["E"][0], now) and np.any(now != E)
    e.trace_end()
    e.close()


# ---- 6. begin late, end early --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three", "cp24", "net"])
def test_a_trace_leaves_the_run_alone(hip_api, name):
    twin = make(hip_api, name)
    twin.iterate(15)
    e = make(hip_api, name)
    e.iterate(5)
    e.trace_begin(ALL, 8)
    e.iterate(2)
    assert e.trace_info()[2:] == (2, 2)
    e.trace_reset()
    assert e.trace_info() == (ALL, 8, 0, 0)
    with pytest.raises(_capi.DopfError, match=r"\(-1\)"):
        e.trace_read(0, 1)
    e.iterate(3)
    assert e.trace_info()[2:] == (3, 3)
    sl = e.trace_read(0, 3)
    assert sl["iteration"].tolist() == [8, 9, 10]
    same_slot(sl, 2, getters(e))
    e.trace_end()
    assert e.trace_info() == (0, 0, 0, 0)
    e.iterate(5)
    a, b = getters(e), getters(twin)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    e.close()
    twin.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def raw_read(e, **given):
    """dopf_trace_read of slot 0 with the named section pointers given (T * whatever doubles is more than any of them needs here)"""
    names = ("lambda", "mu", "rho", "injection", "avg_U", "avg_K", "line_util", "P", "D", "C", "E")
    buf = np.zeros(4096)
    args = [buf.ctypes.data_as(_capi.c_double_p) if n in given else None for n in names]
    rc = e.api.trace_read(e._ctx, 0, 1, None, None, None, *args)
    return rc, e.api.last_error(e._ctx).decode()


def test_refusals(hip_api):
    e = make(hip_api, "three")
    invalid = lambda: pytest.raises(_capi.DopfError, match=r"\(-1\)")
    for call in (e.trace_end, e.trace_reset, lambda: e.trace_read(0, 0)):          # no trace
        with invalid():
            call()
    for what, cap in ((8, 4), (-1, 4), (ALL, 0), (ALL, -3)):
        with invalid():
            e.trace_begin(what, cap)
    assert e.trace_info() == (0, 0, 0, 0)
    e.trace_begin(_capi.TRACE_DUALS, 4)
    with invalid():
        e.trace_begin(_capi.TRACE_DUALS, 4)          # a second begin
    e.iterate(2)
    for name, bit in (("P", "DOPF_TRACE_PRIMAL"), ("E", "DOPF_TRACE_PRIMAL"), ("avg_K", "DOPF_TRACE_CONSENSUS"), ("injection", "DOPF_TRACE_CONSENSUS")):
        rc, msg = raw_read(e, **{name: True})
        assert rc == -1 and re.search(r"\b%s is given" % name, msg) and bit in msg, (name, rc, msg)
    assert raw_read(e, **{"lambda": True, "rho": True})[0] == 0
    # while a trace is active dopf_iterate alone advances the context
    for call in (lambda: e.iterate_timed(1), e.local_update, e.apply_consensus, lambda: e.xchg_export(1),
                 lambda: e.comm_init(1, 0, bytes(_capi.COMM_ID_BYTES)), lambda: e.xchg_init(1, 0, bytes(_capi.XCHG_HANDLE_BYTES))):
        with invalid():
            call()
    assert e.trace_info()[2:] == (2, 2)
    # ... and the setters keep working: the rows' iteration shows what they did to the counter
    lam, mu, rho = e.get_duals()
    e.set_state(lam=lam, mu=mu, rho=rho, iteration=40)
    e.iterate(1)
    assert e.trace_read(0, 3)["iteration"].tolist() == [1, 2, 40]
    e.trace_end()
    e.iterate_timed(1)
    e.close()


def test_a_context_on_a_peer_exchange_is_refused(hip_api):
    e = make(hip_api, "cp5")
    e.xchg_export(1)
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*communicator or a peer exchange"):
        e.trace_begin(ALL, 4)
    assert e.trace_info() == (0, 0, 0, 0)
    e.close()


def test_a_ring_beyond_the_device_is_refused_with_its_bytes(hip_api):
    pp = problem("cp24")
    slot = layout_twin(pp.N, pp.L, pp.T, pp.G, pp.S, ALL)[0]
    cap = (1 << 42) // slot + 1          # 4 TiB of slots: beyond any device's memory, and nothing of it is allocated
    assert cap < 2 ** 31
    e = make(hip_api, "cp24")
    with pytest.raises(_capi.DopfError, match=r"\(-2\)") as err:
        e.trace_begin(ALL, cap)
    m = re.search(r"ring of (\d+) slots of (\d+) bytes needs (\d+) bytes, the device has (\d+) free", str(err.value))
    assert m and int(m.group(1)) == cap and int(m.group(2)) == slot and int(m.group(3)) >= cap * slot > int(m.group(4))
    assert e.trace_info() == (0, 0, 0, 0)
    e.trace_begin(ALL, 2)          # (and the context is as it was)
    e.iterate(1)
    same_slot(e.trace_read(0, 1), 0, getters(e))
    e.close()


# ---- 8. the hosts --------------------------------------------------------------------------------------------------------------------
def same_history(a, b):
    assert len(a.results) == len(b.results) == 12 and a.iteration == b.iteration
    for name in ("lambdas", "mues", "rhos"):
        ha, hb = getattr(a, name), getattr(b, name)
        assert len(ha) == len(hb) == 13 and all(np.array_equal(x, y) for x, y in zip(ha, hb)), name
    ca, cb = a.convergence, b.convergence
    assert (ca.lambda_, ca.mue, ca.rho, ca.all) == (cb.lambda_, cb.mue, cb.rho, cb.all)
    for name in ("lambda_res", "mue_res", "rho_res"):
        ha, hb = getattr(ca, name), getattr(cb, name)
        assert len(ha) == len(hb) == 11 and all(np.array_equal(x, y) for x, y in zip(ha, hb)), name
    for ra, rb in zip(a.results, b.results):
        for f in ("generation", "discharge", "charge", "avg_U", "avg_K", "injection", "line_utilization"):
            assert np.array_equal(getattr(ra, f), getattr(rb, f)), f
        assert ra.total_costs == rb.total_costs and ra.penalty_term is None and rb.penalty_term is None
        for ga, gb in zip(a.generators, b.generators):
            assert np.array_equal(ra.of(ga).generation, rb.of(gb).generation)
        for sa, sb in zip(a.storages, b.storages):
            for f in ("discharge", "charge", "level"):
                assert np.array_equal(getattr(ra.of(sa), f), getattr(rb.of(sb), f)), f
        for na, nb in zip(a.nodes, b.nodes):
            for f in ("generation", "discharge", "charge"):
                assert np.array_equal(getattr(ra.of_node(na), f), getattr(rb.of_node(nb), f)), f


@pytest.mark.parametrize("chunk", [5, 64])
def test_run_recorded_fills_the_history_run_fills(hip_api, tmp_path, chunk):
    def fresh():
        nodes, lines, gens, stos = pkg.three_node_case()
        return ADMM(0.3, nodes, gens, stos, lines, backend=hip_api, eps=0.0, max_iters=12)
    a, b = run(fresh()), run_recorded(fresh(), chunk=chunk)
    same_history(a, b)
    assert b.engine.trace_info() == (0, 0, 0, 0)          # (ended on the way out)
    export_results(a, "case", parent_dir=str(tmp_path / "run"))
    export_results(b, "case", parent_dir=str(tmp_path / "recorded"))
    for f in ("case_duals.csv", "case_generators.csv", "case_storages.csv"):
        assert (tmp_path / "run" / f).read_bytes() == (tmp_path / "recorded" / f).read_bytes(), f


def test_run_recorded_leaves_a_trace_that_is_not_its_own(hip_api):
    nodes, lines, gens, stos = pkg.three_node_case()
    admm = ADMM(0.3, nodes, gens, stos, lines, backend=hip_api, eps=0.0, max_iters=12)
    admm.engine.trace_begin(0, 1)          # (run_recorded's own begin is refused ...)
    with pytest.raises(_capi.DopfError):
        run_recorded(admm)
    assert admm.engine.trace_info() == (0, 1, 0, 0)          # (... and it leaves a trace that is not its own)
    admm.engine.trace_end()
