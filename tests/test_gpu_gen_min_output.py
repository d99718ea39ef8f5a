"""dopf_set_generator_min_output on the GPU: the MN instantiations of k_gen_ramp and k_gen_ramp_net. One step of a
floor context against a twin on the trusted kernels (a ramp context without floors of the shifted problem), one step against the
NumPy programmes with availability (floors that follow their caps) and their certificate, zero floors against the context that never
called the setter (bit for bit), the setter's refusals and timing, convergence to the host LP with must-run units, two shards against
one context, and Engine.roll. The states the one-step tests start from are drawn on the host (helpers_min_output.drawn_state) or
reached by the flagless chain, so their coverage — rows repaired, rows on their floor — was settled on the CPU and is asserted here."""
import copy

import numpy as np
import pytest

from decentralopf_jl_amd import _capi, central, synth
from helpers import make_engine, set_from, state_of
from helpers_min_output import (PLATES, all_state, floor_infeasibility, floor_kkt_violation, floor_of, floor_profiles, path_exists,
                                plate_draw, plate_rows, ramp_project_pwl_floor, same_bits, set_floor_raw, swing)
from helpers_quadratic import QC, params_of
from helpers_ramp import RAMP, draw_ramps, ramp_engine, step_centres
from helpers_ramp_net import CHAIN_NET, NET, net_step_pieces, phi_gen

pytestmark = pytest.mark.gpu
AV = _capi.F_GEN_AVAILABILITY
KEEP = _capi.F_KEEP_DELTAS
EAGER = _capi.F_NO_GRAPH
GAMMA, W_FLOW = 0.3, 10.0                    # the reference's parameters (the network tests')
SEEDS = {("7x5", False): 14, ("7x5", True): 13}          # (default 11) the seeds whose coverage the CPU emulation settled


def _plate(name, quad, avail=False):
    return plate_draw(name, quad, SEEDS.get((name, quad), 11), avail)


def _floor_plate(hip_api, d, flags=0, floor=True):
    """the ramp context of a drawn plate with everything set, the floors last"""
    pp = d["pp"]
    h = ramp_engine(hip_api, pp, flags=flags, **d["prm"])
    if d["prof"] is not None:
        h.set_availability(d["prof"], d["of"])
    if flags & QC:
        h.set_quadratic_cost(d["c2"])
    h.set_ramp(d["up"], d["down"], d["prev"])
    if floor:
        h.set_min_output(d["p_min"])
    return h


def _coverage(rows, G):
    rep = sum(r[1] for r in rows)
    touch = sum(r[1] and r[2] for r in rows)
    rest = sum(r[3] for r in rows)
    return rep, touch, rest


# ---- 5. one step against a twin on the trusted kernels -------------------------------------------------------------------------------

@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
@pytest.mark.parametrize("quad", [False, True], ids=["linear", "c2"])
@pytest.mark.parametrize("name", list(PLATES))
def test_one_step_equals_the_shifted_problem_without_floors(hip_api, name, quad, eager):
    """Without availability the substitution P = P' + p_min turns the floor context's step into the step of a ramp context without
    floors: pmax' = pmax - p_min, demand' = demand - sum of the node's p_min, prev' = prev - p_min, mc' = mc + c2 p_min, from the
    state P' = P - p_min (the injections, and with them every price, are the same numbers up to the rounding of the sums). After one
    step P against P' + p_min at 1e-9 scaled by the row's capacity — the suite's bound for a primal value —, D and C at 1e-9 scaled by
    the storage's power, lambda and the residuals at 1e-9 scaled by max(1, largest value). The twin runs k_gen_ramp<., ., false>."""
    d = _plate(name, quad)
    pp, prm, p_min, c2 = d["pp"], d["prm"], d["p_min"], d["c2"]
    flags = (QC if quad else 0) | (EAGER if eager else 0)
    h = _floor_plate(hip_api, d, flags)
    q = copy.copy(pp)
    q.gen_pmax = pp.gen_pmax - p_min
    q.gen_mc = pp.gen_mc + c2 * p_min
    q.demand = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T) - np.bincount(pp.gen_node, weights=p_min, minlength=pp.N)[:, None]
    twin = _floor_plate(hip_api, dict(d, pp=q, prev=d["prev"] - p_min), flags, floor=False)
    set_from(h, d["st"], 2)
    set_from(twin, dict(d["st"], P=d["st"]["P"] - p_min[:, None]), 2)
    before = state_of(h)
    c, qq = step_centres(pp, c2, before, prm["gamma"])
    rows = plate_rows(c, qq, p_min, d["cap"], d["up"], d["down"], d["prev"])
    rep, touch, rest = _coverage(rows, pp.G)
    h.iterate(1)
    twin.iterate(1)
    a, b = state_of(h), state_of(twin)
    eP = float((np.abs(a["P"] - (b["P"] + p_min[:, None])).max(axis=1) / np.maximum(1.0, pp.gen_pmax)).max())
    eW = float((np.abs(a["P"] - np.stack([r[0] for r in rows])).max(axis=1) / np.maximum(1.0, pp.gen_pmax)).max())
    eS = max([float((np.abs(a[k] - b[k]).max(axis=1) / np.maximum(1.0, pp.sto_pmax)).max()) for k in ("D", "C")] if pp.S else [0.0])
    eL = float(np.abs(a["lam"] - b["lam"]).max()) / max(1.0, float(np.abs(b["lam"]).max()))
    ra, rb = np.asarray(h.get_residuals()[:3]), np.asarray(twin.get_residuals()[:3])
    eR = float(np.abs(ra - rb).max()) / max(1.0, float(np.abs(rb).max()))
    print(f"{name} c2={quad}: |P - (P' + p_min)| {eP:.2e}, |P - programme| {eW:.2e}, D/C {eS:.2e}, lambda {eL:.2e}, residuals {eR:.2e} "
          f"(scaled); repaired {rep}/{pp.G}, of those on the floor {touch}, rows resting on the floor {rest}")
    assert 4 * rep >= pp.G and 4 * touch >= rep and touch >= 1 and rest >= 1, (rep, touch, rest, pp.G)
    assert eP <= 1e-9 and eS <= 1e-9 and eL <= 1e-9 and eR <= 1e-9, (eP, eS, eL, eR)
    assert eW <= 1e-9, eW
    assert h.solver_failures() == 0 and twin.solver_failures() == 0


# ---- 6. one step against the programmes, with availability ---------------------------------------------------------------------------

AVAIL_PLATES = [(n, q) for n in PLATES for q in (False, True) if not q or n in ("7x5", "9+4x6")]


@pytest.mark.parametrize("name,quad", AVAIL_PLATES, ids=[f"{n}-{'c2' if q else 'linear'}" for n, q in AVAIL_PLATES])
def test_one_step_with_availability_against_the_projection_and_the_certificate(hip_api, name, quad):
    """Floors that follow their caps (one profile drops to 0 and rises again): P against ramp_project_floor on the step's centres
    row by row at 1e-9 scaled by max(1, pmax), and the ramp tests' certificate with the floor as the lower bound at 1e-8."""
    d = _plate(name, quad, avail=True)
    pp, prm, p_min, c2, cap = d["pp"], d["prm"], d["p_min"], d["c2"], d["cap"]
    assert np.any((cap[:, :-1] == 0.0) & (floor_of(1.0, cap[:, 1:]) > 0.0) & (p_min[:, None] > 0.0))      # a floor rises behind a zero cap
    h = _floor_plate(hip_api, d, AV | (QC if quad else 0))
    set_from(h, d["st"], 2)
    before = state_of(h)
    c, qq = step_centres(pp, c2, before, prm["gamma"])
    rows = plate_rows(c, qq, p_min, cap, d["up"], d["down"], d["prev"])
    rep, touch, rest = _coverage(rows, pp.G)
    h.iterate(1)
    after = state_of(h)
    worst = cert = 0.0
    gamma = prm["gamma"]
    for g in range(pp.G):
        lo = floor_of(p_min[g], cap[g])
        worst = max(worst, float(np.abs(after["P"][g] - rows[g][0]).max()) / max(1.0, float(pp.gen_pmax[g])))
        grad = pp.gen_mc[g] + c2[g] * after["P"][g] + before["lam"] + gamma * (before["inj"].sum(axis=0) + after["P"][g] - before["P"][g]) \
            + (after["P"][g] - before["P"][g])
        infeas, stat = floor_kkt_violation(after["P"][g], grad, lo, cap[g], d["up"][g], d["down"][g], float(d["prev"][g]))
        assert infeas <= 1e-9 * max(1.0, float(pp.gen_pmax[g])), (g, infeas)
        cert = max(cert, stat)
    print(f"{name} c2={quad}: |P - programme| {worst:.2e} (scaled), certificate {cert:.2e}; repaired {rep}/{pp.G}, of those on the floor "
          f"{touch}, rows resting on the floor {rest}")
    assert rep >= 1 and touch >= 1 and rest >= 1, (rep, touch, rest)
    assert worst <= 1e-9, worst
    assert cert <= 1e-8, cert
    assert h.solver_failures() == 0


def _net_case():
    return swing(synth.synthetic_case(12, 0, 6, N=6, L=8, seed=2, fmax_factor=0.8, fmax_min=5))


def _net_draw(seed=19):
    pp = _net_case()
    rng = np.random.default_rng(seed)
    up, down = draw_ramps(pp, rng)
    p_min = rng.uniform(0.1, 0.4, pp.G) * pp.gen_pmax
    prof, of, cap = floor_profiles(pp, p_min, up, down, None, rng)
    return pp, up, down, p_min, prof, of, cap


def _net_engine(hip_api, pp, flags, up, down, prof=None, of=None, p_min=None):
    e = _capi.Engine(hip_api, params=_capi.default_params(flags=flags | NET, eps=0.0, gamma=GAMMA), **pp.engine_kwargs())
    if prof is not None:
        e.set_availability(prof, of)
    e.set_ramp(up, down, None)
    if p_min is not None:
        e.set_min_output(p_min)
    return e


@pytest.mark.parametrize("keep", [False, True], ids=["walked-only", "keep-deltas"])
def test_one_step_on_a_network_against_the_programme_and_the_slack_sums(hip_api, keep):
    """12 generators on 6 nodes and 8 lines, T = 6, with availability, from the state the flagless chain reaches after 3 iterations
    (on the CPU oracle: 6 rows repaired, 2 of them onto their floor): P against ramp_project_pwl_floor on the closed forms' pieces at
    1e-9 scaled by max(1, pmax), the certificate at 1e-8, and avg_U / avg_K the means of the closed forms at d = P_after - P_before
    (1e-9 scaled by the largest mean), as the network ramp test checks them: a delta left from the clamped step would show there."""
    pp, up, down, p_min, prof, of, cap = _net_draw()
    more = AV | (KEEP if keep else 0)
    h = _net_engine(hip_api, pp, more, up, down, prof, of, p_min)
    twin = make_engine(hip_api, pp, flags=more | CHAIN_NET, eps=0.0, gamma=GAMMA)
    twin.set_availability(prof, of)
    twin.iterate(3)
    st, it = state_of(twin), twin.get_residuals()[3]
    set_from(h, st, it)
    before = state_of(h)
    h.iterate(1)
    after = state_of(h)
    c2 = np.zeros(pp.G)
    pieces = net_step_pieces(pp, c2, before, GAMMA, W_FLOW, None)
    grad = phi_gen(pp, c2, before, GAMMA, W_FLOW, after["P"], None)
    worst = cert = 0.0
    rep = touch = 0
    for g in range(pp.G):
        lo, info = floor_of(p_min[g], cap[g]), {}
        want = ramp_project_pwl_floor(pieces[g], lo, cap[g], up[g], down[g], None, info)
        free = ramp_project_pwl_floor(pieces[g], lo, cap[g], np.inf, np.inf, None)
        repaired = bool(np.any(want != free))
        rep, touch = rep + repaired, touch + (repaired and info["on_floor"])
        worst = max(worst, float(np.abs(after["P"][g] - want).max()) / max(1.0, float(pp.gen_pmax[g])))
        infeas, stat = floor_kkt_violation(after["P"][g], grad[g], lo, cap[g], up[g], down[g], None)
        assert infeas <= 1e-9 * max(1.0, float(pp.gen_pmax[g])), (g, infeas)
        cert = max(cert, stat)
    w2 = 2.0 * W_FLOW
    Hm = np.asarray(pp.ptdf, dtype=np.float64).reshape(pp.L, pp.N)
    flow = Hm @ before["inj"]
    dl = after["P"] - before["P"]
    fl = flow[:, None, :] + Hm[:, pp.gen_node][:, :, None] * dl[None]                              # (L, G, T)
    Fm = pp.f_max[:, None, None]
    U = np.maximum(0.0, (GAMMA * before["avg_U"][:, None, :] - w2 * (fl - Fm)) / (w2 + GAMMA)).mean(axis=1)
    K = np.maximum(0.0, (GAMMA * before["avg_K"][:, None, :] + w2 * (fl + Fm)) / (w2 + GAMMA)).mean(axis=1)
    eu = float(np.abs(after["avg_U"] - U).max()) / max(1.0, float(np.abs(U).max()))
    ek = float(np.abs(after["avg_K"] - K).max()) / max(1.0, float(np.abs(K).max()))
    print(f"keep {keep}: |P - programme| {worst:.2e} (scaled), certificate {cert:.2e}, avg_U {eu:.2e}, avg_K {ek:.2e}; repaired "
          f"{rep}/{pp.G}, of those on the floor {touch}")
    assert rep >= 3 and touch >= 1, (rep, touch)
    assert worst <= 1e-9 and cert <= 1e-8, (worst, cert)
    assert eu <= 1e-9 and ek <= 1e-9, (eu, ek)
    assert h.solver_failures() == 0


# ---- 7. zero floors change nothing ---------------------------------------------------------------------------------------------------

def _in_step(a, b, what):
    for n in (1, 3, 3):                                        # after 1, 4 and 7 iterations
        assert a.iterate(n) == b.iterate(n)
        assert same_bits(all_state(a), all_state(b)), what


def test_zero_floors_are_the_ramp_context_bit_for_bit_on_a_plate(hip_api):
    """The setter with an array of zeros switches to the MN instantiation, whose box [fmin(0, cap), cap] is [0, cap]: the bits of the
    context that never called it; and again after the NULL call, which switches back. (The twin's ramp setter is called at the same
    points: the same values, and the same fresh start of the stop test.)"""
    d = _plate("9+4x6", False)
    pp = d["pp"]
    a, b = (_floor_plate(hip_api, d, 0, floor=False) for _ in range(2))
    for e in (a, b):
        set_from(e, d["st"], 2)
    assert set_floor_raw(b, np.zeros(pp.G))[0] == 0
    a.set_ramp(d["up"], d["down"], d["prev"])
    _in_step(a, b, "zeros")
    assert set_floor_raw(b, None)[0] == 0
    a.set_ramp(d["up"], d["down"], d["prev"])
    _in_step(a, b, "NULL")


def test_zero_floors_are_the_ramp_context_bit_for_bit_on_a_network(hip_api):
    pp, up, down, p_min, prof, of, cap = _net_draw()
    a, b = (_net_engine(hip_api, pp, AV, up, down, prof, of) for _ in range(2))
    twin = make_engine(hip_api, pp, flags=AV | CHAIN_NET, eps=0.0, gamma=GAMMA)
    twin.set_availability(prof, of)
    twin.iterate(3)
    st, it = state_of(twin), twin.get_residuals()[3]
    for e in (a, b):
        set_from(e, st, it)
    assert set_floor_raw(b, np.zeros(pp.G))[0] == 0
    a.set_ramp(up, down, None)
    _in_step(a, b, "zeros")
    assert set_floor_raw(b, None)[0] == 0
    a.set_ramp(up, down, None)
    _in_step(a, b, "NULL")


# ---- 8. the setter -------------------------------------------------------------------------------------------------------------------

def _small():
    return swing(synth.synthetic_case(7, 0, 5, seed=3))


def test_refusals_store_nothing(hip_api):
    pp = _small()
    prm = params_of(pp)
    G = pp.G
    floor = 0.3 * pp.gen_pmax
    # without the ramp flag, and with budgets (the pair included): DOPF_E_UNSUPPORTED
    rc, msg = set_floor_raw(make_engine(hip_api, pp, **prm), floor)
    assert rc == -4 and "ramp kernels" in msg and "DOPF_F_GEN_RAMP " in msg and "DOPF_F_GEN_RAMP_NETWORK" in msg, (rc, msg)
    for flags, flags2 in ((0, _capi.F2_GEN_ENERGY_BUDGET), (RAMP, _capi.F2_GEN_ENERGY_BUDGET | _capi.F2_GEN_RAMP_BUDGET)):
        e = _capi.Engine(hip_api, params=_capi.default_params(flags=flags, **prm), flags2=flags2, **pp.engine_kwargs())
        rc, msg = set_floor_raw(e, floor)
        assert rc == -4 and ("DOPF_F2_GEN_ENERGY_BUDGET" in msg or "DOPF_F_GEN_RAMP" in msg), (flags, rc, msg)
        assert np.array_equal(e.min_output(), np.zeros(G))
    up, down, prev = 0.1 * pp.gen_pmax, 0.2 * pp.gen_pmax, 0.5 * pp.gen_pmax
    h, twin = (ramp_engine(hip_api, pp, (up, down), prev, **prm) for _ in range(2))
    for e in (h, twin):
        e.set_min_output(floor)
        e.iterate(3)
    def bad(g, v):
        x = floor.copy()
        x[g] = v
        return x
    for arr, what in ((bad(2, np.nan), r"p_min[2]"), (bad(5, np.inf), r"p_min[5]"), (bad(1, -1e-3), r"p_min[1]"),
                      (bad(4, np.nextafter(pp.gen_pmax[4], np.inf)), r"p_min[4]")):
        rc, msg = set_floor_raw(h, arr)
        assert rc == -1 and "dopf_set_generator_min_output" in msg and what in msg, (rc, msg)
    # a row without a path: generator 3 anchored at 0.5 pmax climbs 0.1 pmax per step at the most and is asked to be at 0.9 pmax
    rc, msg = set_floor_raw(h, bad(3, 0.9 * pp.gen_pmax[3]))
    assert rc == -1 and "dopf_set_generator_min_output" in msg and "g = 3 " in msg and "t = 0 " in msg, (rc, msg)
    assert np.array_equal(h.min_output(), floor) and np.array_equal(twin.min_output(), floor)
    assert h.iterate(1) == twin.iterate(1)
    assert same_bits(all_state(h), all_state(twin))


def test_the_other_setters_refuse_an_unreachable_floor_and_leave_every_getter(hip_api):
    pp = _small()
    prm = params_of(pp)
    G, T = pp.G, pp.T
    floor = np.zeros(G)
    floor[3] = 0.4 * pp.gen_pmax[3]
    up, down = np.full(G, np.inf), np.full(G, np.inf)
    up[3] = 0.05 * pp.gen_pmax[3]
    down[1] = 0.1 * pp.gen_pmax[1]
    prev = 0.45 * pp.gen_pmax
    prof, of = np.ones((1, T)), np.zeros(G, dtype=np.int32)
    only3 = np.full(G, -1, dtype=np.int32)
    only3[3] = 0
    h = ramp_engine(hip_api, pp, flags=AV, **prm)
    h.set_availability(prof, of)
    h.set_ramp(up, down, prev)
    h.set_min_output(floor)
    h.iterate(4)
    def getters():
        c = h.generator_coupling()
        return all_state(h) + [h.min_output()] + [c[k] for k in sorted(c)]
    was = getters()
    # the ramp setter: anchored below its floor with no way up
    low, still = prev.copy(), up.copy()
    low[3], still[3] = 0.1 * pp.gen_pmax[3], 0.0
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_ramp.*g = 3 .*t = 0 "):
        h.set_ramp(still, down, low)
    assert same_bits(getters(), was)
    # the availability setter: the cap drops to 0 at t = 1, and from there the floor is 0.4 pmax away, 0.05 pmax per step
    drop = np.where(np.arange(T) == 1, 0.0, 1.0)[None, :]
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_availability.*g = 3 .*t = 2 "):
        h.set_availability(drop, only3)
    assert same_bits(getters(), was)
    # the roll, with the table that will be in force (the new anchor is P[:, k - 1])
    tail = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, T)[:, :1]
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_roll_horizon_coupled.*g = 3 .*t = 2 "):
        h.roll_coupled(1, tail, availability=(drop, only3))
    assert same_bits(getters(), was)
    # a row without a floor keeps the check and the text it had: generator 1, anchored at 0.45 pmax, comes down 0.1 pmax per step
    only1 = np.full(G, -1, dtype=np.int32)
    only1[1] = 0
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_availability: generator g = 1 cannot come down from p_prev"):
        h.set_availability(drop, only1)
    assert same_bits(getters(), was)


def test_a_set_between_graph_replays_equals_a_fresh_context_and_resets_converged(hip_api):
    d = _plate("7x5", False)
    pp, prm = d["pp"], d["prm"]
    h = _floor_plate(hip_api, d, 0, floor=False)
    h.iterate(16)                                              # (graphs of the MN = false kernel are in place)
    for floor in (d["p_min"], 0.5 * d["p_min"], None):         # the switch, a second array (the graphs stay), the switch back
        st, it = state_of(h), h.get_residuals()[3]
        h.set_min_output(floor)
        assert h.get_residuals()[3] == it                      # the iteration counter is kept
        now = state_of(h)
        for k in ("P", "lam", "inj"):
            assert np.array_equal(now[k], st[k]), k
        fresh = _floor_plate(hip_api, d, 0, floor=False)
        fresh.set_min_output(floor)                            # before its first iteration
        for e in (h, fresh):
            set_from(e, st, it)
        h.iterate(4)
        fresh.iterate(4)
        assert same_bits(all_state(h), all_state(fresh)), floor is None
        want = np.zeros(pp.G) if floor is None else floor
        assert np.array_equal(h.min_output(), want)
        assert (h.get_primal()[0] >= want[:, None]).all()
    # converged is reset
    pp = synth.synthetic_case(7, 0, 5, seed=3)                 # (the case without the swing: it converges)
    e = ramp_engine(hip_api, pp, gamma=1.0 / pp.G, max_iters=20000)
    done, conv = e.iterate(20000)
    assert conv and e.iterate(5) == (0, True)
    it = e.get_residuals()[3]
    e.set_min_output(0.05 * pp.gen_pmax)
    assert e.sync() == (it, False)


# ---- 9. convergence ------------------------------------------------------------------------------------------------------------------

def test_must_run_units_converge_to_the_host_lp(hip_api):
    """A plate whose two most expensive units must run at 30 % and whose cheapest is must-take at 10 %: the floors bind at the optimum
    (the LP's objective rises by more than 1e-6 of itself), the run stops within 1e-3 of the host LP with floors, and floors and
    ramps, which the exact projection keeps in every iteration, hold to 1e-9."""
    pp = swing(synth.synthetic_case(7, 0, 5, seed=3), 0.85, 1.15)
    order = np.argsort(pp.gen_mc)
    floor = np.zeros(pp.G)
    floor[order[-2:]] = 0.3 * pp.gen_pmax[order[-2:]]
    floor[order[0]] = 0.1 * pp.gen_pmax[order[0]]
    up, down = 0.2 * pp.gen_pmax, 0.2 * pp.gen_pmax
    up[::3] = np.inf
    assert floor.sum() < np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T).sum(axis=0).min()       # not over-committed
    want = central.solve_central_packed(pp, gen_ramp=(up, down), gen_min_output=floor)
    free = central.solve_central_packed(pp, gen_ramp=(up, down))
    assert want.objective > free.objective * (1.0 + 1e-6)
    h = ramp_engine(hip_api, pp, (up, down), gamma=0.3, max_iters=20000)
    h.set_min_output(floor)
    done, conv = h.iterate(20000)
    st = state_of(h)
    gap = abs(float(st["cost"][0]) - want.objective) / want.objective
    bal = float(np.abs(st["inj"].sum(axis=0)).max())
    viol = max(floor_infeasibility(st["P"][g], floor[g], pp.gen_pmax[g], up[g], down[g]) for g in range(pp.G))
    print(f"converged {conv} after {done} iterations, relative cost gap {gap:.2e}, balance {bal:.1e}, largest floor / ramp violation "
          f"{viol:.2e}, LP {want.objective:.4f} (without floors {free.objective:.4f})")
    assert conv
    assert viol <= 1e-9 * float(pp.gen_pmax.max()), viol
    assert gap <= 1e-3 and bal <= h.params.eps / h.params.gamma, (gap, bal)


# ---- 10. shards and rolls ------------------------------------------------------------------------------------------------------------

def _close(got, want, keys, who):
    for key in keys:
        if want[key].size:
            assert np.abs(got[key] - want[key]).max() <= 1e-9 * max(1.0, np.abs(want[key]).max()), (key, who)


def _sharded_case():
    pp = swing(synth.synthetic_case(41, 7, 6, seed=4))
    rng = np.random.default_rng(4)
    up, down = draw_ramps(pp, rng)
    floor = rng.uniform(0.0, 0.3, pp.G) * pp.gen_pmax
    floor[::4] = 0.0
    prev = floor + rng.uniform(0.0, 1.0, pp.G) * (pp.gen_pmax - floor)
    for g in range(pp.G):
        assert path_exists(np.full(pp.T, floor[g]), np.full(pp.T, pp.gen_pmax[g]), up[g], down[g], prev[g]) is None
    return pp, up, down, floor, prev


def test_multi_two_shards_equal_one_context(hip_api):
    pp, up, down, floor, prev = _sharded_case()
    g = 1.0 / (pp.G + pp.S)
    ref = ramp_engine(hip_api, pp, (up, down), prev, eps=0.0, gamma=g)
    ref.set_min_output(floor)
    q = copy.copy(pp)
    q.gen_ramp, q.gen_min_output = (up, down), floor             # (through engine_kwargs: the flag and the setters from the constructor)
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(eps=0.0, gamma=g, flags=_capi.F_COMM_HOST), gen_prev=prev,
                          **q.engine_kwargs())
    assert m.params.flags & RAMP
    for k in (1, 4, 7):
        ref.iterate(k)
        assert m.iterate(k) == (k, False)
        want = state_of(ref)
        P, D, C, E = m.get_primal()
        _close(dict(P=P, D=D, C=C, E=E), want, ("P", "D", "C", "E"), "primal")
        assert (P >= floor[:, None]).all()
        for i in range(2):
            _close(state_of(m.shard(i)), want, ("lam", "inj", "cost"), i)
    bad = floor.copy()
    bad[pp.G - 1] = -1.0                                         # the second shard's last entry: nothing stored on the first either
    with pytest.raises(_capi.DopfError, match="shard 1"):
        m.set_min_output(bad)
    assert np.array_equal(m.shard(0).min_output(), floor[:m.shard(0).G])
    ref.iterate(3)
    assert m.iterate(3) == (3, False)
    _close(state_of(m.shard(0)), state_of(ref), ("lam", "inj", "cost"), "after a refusal")
    m.close()


def test_sharded_admm_two_ranks_equal_one_context(hip_api):
    import torch
    from conftest import pkg
    pp, up, down, floor, prev = _sharded_case()
    g = 1.0 / (pp.G + pp.S)
    ref = ramp_engine(hip_api, pp, (up, down), prev, eps=0.0, gamma=g)
    ref.set_min_output(floor)
    ranks = [pkg.ShardedADMM(pp, r, 2, all_reduce=lambda: None, eps=0.0, gamma=g, flags=RAMP) for r in range(2)]
    for sh in ranks:
        sh.set_ramp(up, down, prev)                              # all G values: each rank takes its slice
        sh.set_min_output(floor)
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


def test_engine_roll_over_two_windows_keeps_floors_and_anchor(hip_api):
    pp = _small()
    prm = params_of(pp)
    up, down = 0.1 * pp.gen_pmax, 0.1 * pp.gen_pmax
    floor = 0.2 * pp.gen_pmax
    floor[::3] = 0.0
    h = ramp_engine(hip_api, pp, (up, down), **prm)
    h.set_min_output(floor)
    h.iterate(20)
    k = 2
    tail = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, :k]
    for window in range(2):
        P = h.get_primal()[0]
        assert (P >= floor[:, None]).all()
        h.roll(k, tail)
        assert h.params.flags & RAMP
        assert np.array_equal(h._mirror["gen_min_output"], floor) and np.array_equal(h.min_output(), floor)
        assert np.array_equal(h._mirror["gen_prev"], P[:, k - 1]) and np.array_equal(h._mirror["gen_ramp"][0], up)
        assert np.array_equal(h.get_primal()[0][:, :pp.T - k], P[:, k:])           # the window moved
        h.iterate(5)
        P1 = h.get_primal()[0]
        assert max(floor_infeasibility(P1[g], floor[g], pp.gen_pmax[g], up[g], down[g], float(P[g, k - 1])) for g in range(pp.G)) <= 1e-9
