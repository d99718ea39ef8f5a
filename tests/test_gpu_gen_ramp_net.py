"""DOPF_F_GEN_RAMP | DOPF_F_GEN_RAMP_NETWORK on the GPU: the generators' step under ramp limits on a network
(k_gen_ramp_net) against the NumPy programme row by row and against its optimality certificate, the deltas the slack sums read after
a repair, the bits of the flagless chain with every ramp at +inf, the create rules and the setter, convergence of the three-node case
to the host LP with ramp rows, and two shards against one context. The steps' derivatives come from the closed forms of DESIGN.md
section 3 (helpers_ramp_net.net_step_pieces), never from the device's tables."""
import copy

import numpy as np
import pytest

from conftest import pkg
from decentralopf_jl_amd import _capi, central, synth
from helpers import draw_profiles, make_engine, set_from, state_of
from helpers_line_rating import draw_table
from helpers_quadratic import QC, draw_c2
from helpers_ramp import RAMP, draw_ramps, ramp_active, ramp_infeasibility, ramp_kkt_violation
from helpers_ramp_net import CHAIN_NET, NET, RAMP_NET, net_step_pieces, phi_gen, ramp_project_pwl

pytestmark = pytest.mark.gpu
AV = _capi.F_GEN_AVAILABILITY
RATING = _capi.F_LINE_RATING
WIDE = _capi.F_DEBUG_WIDE_NET
KEEP = _capi.F_KEEP_DELTAS
GAMMA, W_FLOW = 0.3, 10.0                    # the reference's parameters
PRM = dict(eps=0.0, gamma=GAMMA)


def swing(pp, lo=0.4, hi=1.6):
    """the case with its demand alternating between lo and hi times itself (the copper-plate test's): neighbouring steps of a row differ"""
    f = np.where(np.arange(pp.T) % 2 == 0, lo, hi)
    pp.demand = np.round(np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T) * f[None, :])
    return pp


def net(G, S, T, N, L, seed, node=None):
    pp = swing(synth.synthetic_case(G, S, T, N=N, L=L, seed=seed, fmax_factor=0.8, fmax_min=5))
    if node is not None:
        pp.gen_node = np.full(pp.G, node, dtype=np.int32)
    return pp


def net_engine(api, pp, ramp=None, prev=None, flags=0, **params):
    """a context with both flags; ramp = (up, down): set after create"""
    e = _capi.Engine(api, params=_capi.default_params(flags=flags | NET, **params), **pp.engine_kwargs())
    if ramp is not None or prev is not None:
        e.set_ramp(*(ramp if ramp is not None else (None, None)), prev)
    return e


# name -> (case, flags, warm-up iterations of the flagless twin, anchored, rated, congested)
# The warm-up runs on the flagless twin, so the state of the compared step is the one a ramp-free CPU oracle run reaches and the
# coverage conditions below could be settled on the CPU. 12xT6 after 2 iterations: 4 of 12 rows with an active ramp, 8 with none, 4
# repaired rows with a kink inside, up to 31 knots (the copper-plate bound is 14). 19+3xT8, all generators on node 1 (one item of 19
# rows: more than the block has waves): the issue's seed 6 leaves 1 active row of 19 for the first 20 iterations and no kink in a
# repaired row later, so seed 7 after 25 iterations (the compared step is iteration 26, an even one): 15 rows active, 4 with none —
# the 4 whose ramps draw_ramps leaves at +inf — 15 repaired rows with a kink inside.
SHAPES = {
    "12xT6-N6-L8": (lambda: net(12, 0, 6, 6, 8, 2), 0, 2, False, False, True),
    "19+3xT8-N3-L3-one-node": (lambda: net(19, 3, 8, 3, 3, 7, node=1), 0, 25, False, False, True),
    "9xT1-anchored": (lambda: net(9, 0, 1, 3, 3, 4), 0, 2, True, False, False),
    "7xT2-anchored": (lambda: net(7, 0, 2, 3, 3, 3), 0, 3, True, False, False),
    "6xT70-N3-L3": (lambda: net(6, 0, 70, 3, 3, 8), 0, 3, False, False, False),
    "5xT130-anchored": (lambda: net(5, 0, 130, 3, 3, 9), 0, 3, True, False, False),
    "12xT6-wide-chain": (lambda: net(12, 0, 6, 6, 8, 2), WIDE, 2, False, False, False),
    "12xT6-line-rating": (lambda: net(12, 0, 6, 6, 8, 2), RATING, 2, False, True, False),
}
EXTRAS = {"plain": (False, False), "availability": (True, False), "c2": (False, True), "availability+c2": (True, True)}
CASES = [(n, x) for n in SHAPES for x in EXTRAS if x == "plain" or n in list(SHAPES)[:2]]


def _setup(hip_api, name, extra, eager, more=0):
    make, flags, warm, anchored, rated, congested = SHAPES[name]
    avail, quad = EXTRAS[extra]
    pp = make()
    rng = np.random.default_rng(17)
    up, down = draw_ramps(pp, rng)
    c2 = draw_c2(pp.G, rng) if quad else np.zeros(pp.G)
    flags |= (AV if avail else 0) | (QC if quad else 0) | (_capi.F_NO_GRAPH if eager else 0) | more
    h = net_engine(hip_api, pp, flags=flags, **PRM)
    twin = make_engine(hip_api, pp, flags=flags | CHAIN_NET, **PRM)
    cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
    F = None
    if rated:
        F = draw_table(pp)
        for e in (h, twin):
            e.set_line_rating(F)
    if avail:
        prof, of = draw_profiles(pp, "K3", rng)
        for e in (h, twin):
            e.set_availability(prof, of)
        cap = np.where((of >= 0)[:, None], pp.gen_pmax[:, None] * prof[np.maximum(of, 0)], cap)
    if quad:
        for e in (h, twin):
            e.set_quadratic_cost(c2)
    prev = rng.uniform(0.0, 1.0, pp.G) * cap.min(axis=1) if anchored else None
    h.set_ramp(up, down, prev)
    twin.iterate(warm)
    st, it = state_of(twin), twin.get_residuals()[3]
    for e in (h, twin):
        set_from(e, st, it)
    return pp, h, twin, c2, cap, up, down, prev, F, congested


def _rows(pp, c2, cap, up, down, prev, F, before):
    """per row: (the programme's answer, a ramp is active, it is repaired — differs from the step without ramps — and merged a kink of
    Psi strictly inside (lo, hi) at some step, its largest knot count, it is repaired)"""
    pieces = net_step_pieces(pp, c2, before, GAMMA, W_FLOW, F)
    out = []
    for g in range(pp.G):
        pv = None if prev is None else float(prev[g])
        info = {}
        want = ramp_project_pwl(pieces[g], cap[g], up[g], down[g], pv, info)
        free = ramp_project_pwl(pieces[g], cap[g], np.inf, np.inf, None)
        repaired = bool(np.any(want != free))
        out.append((want, ramp_active(want, up[g], down[g], pv), repaired and sum(info["merged"]) > 0, info["most"], repaired))
    return out


@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
@pytest.mark.parametrize("name,extra", CASES, ids=[f"{n}-{x}" for n, x in CASES])
def test_one_step_against_the_programme_and_the_certificate(hip_api, name, extra, eager):
    """(a) One step from the device's own state: P against ramp_project_pwl row by row (1e-9 scaled by max(1, gen_pmax)) and the
    certificate of every row at 1e-8 with the gradient mc + c2 P + Psi(P - p0) + w (P - p0) — the bounds of the copper-plate test;
    D and C the bits of the flagless twin on the chain; no solver failure. The coverage conditions are asserted on the plain runs of
    the two congested shapes (what the CPU oracle run settled; with availability or c2 the state is another) and printed for all."""
    pp, h, twin, c2, cap, up, down, prev, F, congested = _setup(hip_api, name, extra, eager)
    before = state_of(h)
    h.iterate(1)
    twin.iterate(1)
    after, other = state_of(h), state_of(twin)
    rows = _rows(pp, c2, cap, up, down, prev, F, before)
    grad = phi_gen(pp, c2, before, GAMMA, W_FLOW, after["P"], F)
    worst = cert = 0.0
    for g, (want, on, kinked, most, repaired) in enumerate(rows):
        pv = None if prev is None else float(prev[g])
        worst = max(worst, float(np.abs(after["P"][g] - want).max()) / max(1.0, float(pp.gen_pmax[g])))
        infeas, stat = ramp_kkt_violation(after["P"][g], grad[g], cap[g], up[g], down[g], pv)
        cert = max(cert, stat)
        assert infeas <= 1e-9, (g, infeas)
    active, kinked, most = sum(r[1] for r in rows), sum(r[2] for r in rows), max(r[3] for r in rows)
    free = pp.G - active
    print(f"{name} {extra}: |P - programme| {worst:.2e} (scaled), certificate {cert:.2e}, rows with an active ramp {active}/{pp.G}, with "
          f"none {free}/{pp.G}, repaired rows with a kink of Psi inside {kinked}, most knots {most} (2T + 2 = {2 * pp.T + 2})")
    if congested and extra == "plain":
        assert 5 * active >= pp.G and 5 * free >= pp.G, (active, free, pp.G)
        assert kinked >= 3, kinked
    assert worst <= 1e-9, worst
    assert cert <= 1e-8, cert
    assert np.array_equal(after["D"], other["D"]) and np.array_equal(after["C"], other["C"])      # the storages do not see the ramps
    assert h.solver_failures() == 0


@pytest.mark.parametrize("keep", [False, True], ids=["walked-only", "keep-deltas"])
def test_the_deltas_after_a_repair_feed_the_slack_sums(hip_api, keep):
    """(b) 12xT6 (no storages): after the compared step avg_U and avg_K are the means over all agents of the closed forms U_l(d_a),
    K_l(d_a) at d_a = P_after - P_before — a delta left from the clamped step of a repaired row would show here, not
    in P. 1e-9 scaled by the largest mean."""
    pp, h, twin, c2, cap, up, down, prev, F, _ = _setup(hip_api, "12xT6-N6-L8", "plain", False, more=KEEP if keep else 0)
    before = state_of(h)
    h.iterate(1)
    after = state_of(h)
    w2 = 2.0 * W_FLOW
    Hm = np.asarray(pp.ptdf, dtype=np.float64).reshape(pp.L, pp.N)
    flow = Hm @ before["inj"]
    d = after["P"] - before["P"]
    fl = flow[:, None, :] + Hm[:, pp.gen_node][:, :, None] * d[None]                              # (L, G, T)
    Fm = pp.f_max[:, None, None]
    U = np.maximum(0.0, (GAMMA * before["avg_U"][:, None, :] - w2 * (fl - Fm)) / (w2 + GAMMA)).mean(axis=1)
    K = np.maximum(0.0, (GAMMA * before["avg_K"][:, None, :] + w2 * (fl + Fm)) / (w2 + GAMMA)).mean(axis=1)
    repaired = sum(r[4] for r in _rows(pp, c2, cap, up, down, prev, F, before))
    eu = float(np.abs(after["avg_U"] - U).max()) / max(1.0, float(np.abs(U).max()))
    ek = float(np.abs(after["avg_K"] - K).max()) / max(1.0, float(np.abs(K).max()))
    print(f"keep {keep}: avg_U {eu:.2e}, avg_K {ek:.2e} (scaled), repaired rows {repaired}/{pp.G}")
    assert repaired >= 3
    assert eu <= 1e-9 and ek <= 1e-9, (eu, ek)


# ---- (c) every ramp +inf, no anchor: the bits of the flagless chain ------------------------------------------------------------------

def _three_node_packed():
    nodes, lines, gens, stos = pkg.three_node_case()
    return pkg.pack(nodes, gens, stos, lines)


FREE = {"three-node": _three_node_packed, "12xT6": lambda: net(12, 0, 6, 6, 8, 2)}


@pytest.mark.parametrize("quad", [False, True], ids=["linear", "c2"])
@pytest.mark.parametrize("name", list(FREE))
def test_all_ramps_inf_is_the_flagless_chain(hip_api, name, quad):
    pp = FREE[name]()
    c2 = draw_c2(pp.G, np.random.default_rng(5))
    h = net_engine(hip_api, pp, flags=QC if quad else 0, **PRM)
    ref = make_engine(hip_api, pp, flags=CHAIN_NET | (QC if quad else 0), **PRM)
    if quad:
        for e in (h, ref):
            e.set_quadratic_cost(c2)
    ref.iterate(3)
    st, it = state_of(ref), ref.get_residuals()[3]
    for e in (h, ref):
        set_from(e, st, it)
    h.iterate(1)
    ref.iterate(1)
    assert np.array_equal(state_of(h)["P"], state_of(ref)["P"])          # one step from the same state: the same bits
    h.iterate(24)
    ref.iterate(24)
    a, b = state_of(h), state_of(ref)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert h.solver_failures() == 0


# ---- (d) create and setter --------------------------------------------------------------------------------------------------------------

def test_the_create_rules(hip_api):
    pp = net(12, 0, 4, 6, 8, 2)
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*copper plates.*DOPF_F_GEN_RAMP_NETWORK"):      # DOPF_E_UNSUPPORTED
        make_engine(hip_api, pp, flags=RAMP, **PRM)
    plate = swing(synth.synthetic_case(7, 0, 5, seed=3))
    for case in (pp, plate):
        with pytest.raises(_capi.DopfError, match=r"\(-4\).*DOPF_F_GEN_RAMP"):
            make_engine(hip_api, case, flags=RAMP_NET, **PRM)
    # L == 0: accepted and ignored — the copper-plate kernel, the same bits
    rng = np.random.default_rng(3)
    ramp = draw_ramps(plate, rng)
    runs = []
    for flags in (RAMP, NET):
        e = make_engine(hip_api, plate, flags=flags, eps=0.0, gamma=1.0 / plate.G)
        e.set_ramp(*ramp)
        e.iterate(12)
        runs.append(state_of(e))
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    # the bindings add the bit where the problem has lines
    q = copy.copy(pp)
    q.gen_ramp = draw_ramps(pp, rng)
    e = _capi.Engine(hip_api, params=_capi.default_params(**PRM), **q.engine_kwargs())
    assert e.params.flags & RAMP and (e.params.flags & RAMP_NET) != 0
    assert e.iterate(3) == (3, False)


def test_setter_between_graph_replays_null_converged_and_roll(hip_api):
    pp = net(12, 0, 6, 6, 8, 2)
    rng = np.random.default_rng(3)
    h = net_engine(hip_api, pp, draw_ramps(pp, rng), **PRM)
    h.iterate(6)
    prev = rng.uniform(0.0, 1.0, pp.G) * pp.gen_pmax
    for ramp, pv in ((draw_ramps(pp, rng), prev), ((None, None), None)):        # None: back to +inf, no anchor
        st, it = state_of(h), h.get_residuals()[3]
        h.set_ramp(*ramp, pv)
        assert h.get_residuals()[3] == it                                       # the iteration counter is kept
        now = state_of(h)
        for k in ("P", "lam", "mu", "rho", "inj"):
            assert np.array_equal(now[k], st[k]), k
        fresh = net_engine(hip_api, pp, None if ramp[0] is None else ramp, pv, **PRM)
        for e in (h, fresh):                                                    # (both from the getters' values: the same node sums)
            set_from(e, st, it)
        h.iterate(4)
        fresh.iterate(4)
        a, b = state_of(h), state_of(fresh)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    ref = make_engine(hip_api, pp, flags=CHAIN_NET, **PRM)                      # +inf again: the flagless chain's bits
    st, it = state_of(h), h.get_residuals()[3]
    for e in (h, ref):
        set_from(e, st, it)
    h.iterate(3)
    ref.iterate(3)
    assert np.array_equal(state_of(h)["P"], state_of(ref)["P"])
    # dopf_roll_horizon is still refused
    tail = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, :1]
    rc = h.api.roll_horizon(h._ctx, 1, _capi._dp(_capi._f64(tail.T)))
    assert rc == -4 and b"DOPF_F_GEN_RAMP" in h.api.last_error(h._ctx)
    # converged is reset
    e = net_engine(hip_api, _three_node_packed(), max_iters=20000)              # (the reference's parameters: it converges)
    done, conv = e.iterate(20000)
    assert conv and e.iterate(5) == (0, True)
    it = e.get_residuals()[3]
    e.set_ramp(np.full(4, 50.0), np.full(4, 50.0))
    assert e.sync() == (it, False)


# ---- (e) convergence on the three-node case ----------------------------------------------------------------------------------------------

def _ramped_three_node():
    """the ramps of test_gen_ramp_abi._ramped_three_node"""
    nodes, lines, gens, stos = pkg.three_node_case()
    gens[2].ramp_up, gens[2].ramp_down = 40.0, 25.0
    gens[3].ramp_down = 10.0
    return nodes, lines, gens, stos


def test_the_three_node_case_converges_to_the_ramped_lp(hip_api):
    """The reference's parameters (gamma 0.3, eps 1e-3). The cost bound of the existing convergence tests (within 1e-3 of the
    central optimum), 1e-9 for the ramps, which the exact step keeps in every iteration, eps / gamma for the balance (what the stop
    test bounds). The LP's ramps bind with these values: 18 650 against 14 035 without."""
    nodes, lines, gens, stos = _ramped_three_node()
    pp = pkg.pack(nodes, gens, stos, lines)
    want = central.solve_central_packed(pp)
    free = central.solve_central_packed(_three_node_packed())
    assert want.objective > free.objective * (1.0 + 1e-6)                      # the ramps bind at the optimum
    h = _capi.Engine(hip_api, params=_capi.default_params(max_iters=20000), **pp.engine_kwargs())
    assert (h.params.flags & RAMP_NET) != 0
    done, conv = h.iterate(20000)
    st = state_of(h)
    up, down = pp.ramp()
    gap = abs(float(st["cost"][0]) - want.objective) / want.objective
    bal = float(np.abs(st["inj"].sum(axis=0)).max())
    viol = max(ramp_infeasibility(st["P"][g], pp.gen_pmax[g], up[g], down[g]) for g in range(pp.G))
    print(f"three-node: converged {conv} after {done} iterations, relative cost gap {gap:.2e}, balance {bal:.1e}, largest ramp violation "
          f"{viol:.2e}, LP {want.objective:.4f} (without ramps {free.objective:.4f})")
    assert conv
    assert viol <= 1e-9, viol
    assert gap <= 1e-3 and bal <= h.params.eps / h.params.gamma, (gap, bal)
    assert h.solver_failures() == 0


# ---- (f) two shards against one context ------------------------------------------------------------------------------------------------

def test_multi_two_shards_equal_one_context(hip_api):
    pp = net(12, 0, 6, 6, 8, 2)
    rng = np.random.default_rng(4)
    up, down = draw_ramps(pp, rng)
    ref = net_engine(hip_api, pp, (up, down), **PRM)
    q = copy.copy(pp)
    q.gen_ramp = (up, down)                                      # (through engine_kwargs: both flags and the setter from the constructor)
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(flags=_capi.F_COMM_HOST, **PRM), **q.engine_kwargs())
    assert m.params.flags & RAMP and (m.params.flags & RAMP_NET) != 0
    for k in (1, 4, 7):
        ref.iterate(k)
        assert m.iterate(k) == (k, False)
        want = state_of(ref)
        P = m.get_primal()[0]
        assert np.abs(P - want["P"]).max() <= 1e-9 * max(1.0, np.abs(want["P"]).max())
        for i in range(2):
            got = state_of(m.shard(i))
            for key in ("lam", "mu", "rho", "inj", "cost"):
                assert np.abs(got[key] - want[key]).max() <= 1e-9 * max(1.0, np.abs(want[key]).max()), (key, i)
    m.close()
