"""dopf_get_generator_ramp_price on the GPU: the multipliers the last x-update put on every generator's ramp rows, as
the RP instantiations of k_gen_ramp and k_gen_ramp_budget store them. One step on plates and in pair contexts against the certificate
(helpers_ramp_price.ramp_price_violation) on the device's own rows and against the NumPy twin of csrc/ramp_price.h on those rows; the
getter moves nothing else; the status rules and the refusals; two shards against one context; and convergence of the prices to the
ramp duals of the central LP. What a step prices is counted by the twin from the drawn state before a device is touched."""
import copy

import numpy as np
import pytest

from conftest import pkg
from decentralopf_jl_amd import _capi, central, synth
from helpers import make_engine, set_from, state_of
from helpers_budget import draw_budgets, row_sums
from helpers_min_output import PLATES, all_state, same_bits, swing
from helpers_quadratic import QC, params_of
from helpers_ramp import RAMP, draw_ramps, ramp_engine, ramp_infeasibility, ramp_project, step_centres
from helpers_ramp_budget import BUDGET, PAIR, draw_budget, extreme_paths, path_sum, ramp_budget_project
from helpers_ramp_net import NET
from helpers_ramp_price import coverage, drawn_before, plate_prices, price_plate, ramp_price_violation

pytestmark = pytest.mark.gpu
AV = _capi.F_GEN_AVAILABILITY
EAGER = _capi.F_NO_GRAPH
BOUND = 1e-9
# (c2, floors, availability)
VARIANTS = {"plain": (False, False, False), "c2": (True, False, False), "floors": (False, True, False),
            "availability": (False, False, True), "floors+availability+c2": (True, True, True)}
SEEDS = {("7x5", "floors"): 12, ("7x5", "floors+availability+c2"): 12}       # (default 11) the seeds whose coverage the twin settled


def pair_engine(api, pp, ramp=None, prev=None, budget=None, flags=0, **params):
    e = _capi.Engine(api, params=_capi.default_params(flags=flags | RAMP, **params), flags2=BUDGET | PAIR, **pp.engine_kwargs())
    if ramp is not None or prev is not None:
        e.set_ramp(*(ramp if ramp is not None else (None, None)), prev)
    if budget is not None:
        e.set_energy_budget(*budget)
    return e


def _engine(hip_api, d, quad, floors, flags=0):
    """the ramp context of a drawn plate with everything set, the floors last"""
    h = ramp_engine(hip_api, d["pp"], flags=flags | (QC if quad else 0) | (AV if d["prof"] is not None else 0), **d["prm"])
    if d["prof"] is not None:
        h.set_availability(d["prof"], d["of"])
    if quad:
        h.set_quadratic_cost(d["c2"])
    h.set_ramp(d["up"], d["down"], d["prev"])
    if floors:
        h.set_min_output(d["p_min"])
    return h


def _check_rows(d, rows, rp, what):
    """per row: the certificate with the device's prices on the device's row, and the twin's prices of that row; (both figures, rows
    the device priced)"""
    pp = d["pp"]
    cert = apart = 0.0
    for g, (x, a, c, q, lo, shift) in enumerate(rows):
        v = ramp_price_violation(x, c, q, lo, d["cap"][g], d["up"][g], d["down"][g], float(d["prev"][g]), rp[g], shift=shift)
        assert v <= BOUND, (what, g, v)
        e = float(np.abs(rp[g] - a).max()) / (q * float(pp.gen_pmax[g]))
        assert e <= BOUND, (what, g, e)
        cert, apart = max(cert, v), max(apart, e)
    return cert, apart, int(np.count_nonzero(np.any(rp != 0.0, axis=1)))


# ---- 1. one step on a plate --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(PLATES))
def test_one_step_on_a_plate(hip_api, name, variant, eager):
    """T = 5, 6, 70 and 130: below and beyond one wave of lanes, and beyond kRampLdsT = 128 (the intervals in scratch). After one step
    from the drawn state the device's prices pass the certificate on the device's own rows at 1e-9 (of q max(1, max cap)) and equal
    the twin's prices of those rows within 1e-9 q pmax. From the drawn state alone the twin prices at least a quarter of the rows,
    with both signs. (On the plates of three generators row 0 carries ramps: helpers_ramp_price.price_plate says why.)"""
    quad, floors, avail = VARIANTS[variant]
    d = price_plate(name, quad, SEEDS.get((name, variant), 11), avail)
    pp = d["pp"]
    n, pos, neg = coverage(plate_prices(d, floors, drawn_before(d)))              # before a device is touched
    assert 4 * n >= pp.G and pos and neg, (n, pp.G, pos, neg)
    h = _engine(hip_api, d, quad, floors, EAGER if eager else 0)
    assert np.array_equal(h.ramp_price(), np.zeros((pp.G, pp.T)))                  # the first call: zeros, and the recording starts
    set_from(h, d["st"], 2)
    before = state_of(h)
    h.iterate(1)
    P, rp = state_of(h)["P"], h.ramp_price()
    assert rp.shape == (pp.G, pp.T)
    cert, apart, priced = _check_rows(d, plate_prices(d, floors, before, P=P), rp, (name, variant))
    print(f"{name} {variant} {'eager' if eager else 'graphs'}: certificate {cert:.2e}, |rp - twin| {apart:.2e} of q pmax; the device "
          f"priced {priced}/{pp.G} rows (the twin, from the drawn state: {n}), {int(np.sum(rp > 0.0))} values > 0, {int(np.sum(rp < 0.0))} < 0")
    assert 4 * priced >= pp.G and np.any(rp > 0.0) and np.any(rp < 0.0)
    assert h.solver_failures() == 0


# ---- 2. one step of the pair -------------------------------------------------------------------------------------------------------------

def _branch(c, q, cap, up, down, prev, lo, hi):
    """the branch of k_gen_ramp_budget's cascade that stores the row, from the NumPy pieces alone"""
    from helpers_budget import budget_project, plate_steps
    x0 = np.clip(c, 0.0, cap)
    bad0 = ramp_infeasibility(x0, cap, up, down, prev) > 0.0
    in0 = lo <= path_sum(x0) <= hi
    if not bad0:
        if in0:
            return 1
        x = budget_project(plate_steps(c, q), cap, lo, hi)
        return 2 if ramp_infeasibility(x, cap, up, down, prev) <= 0.0 else 4
    s = path_sum(ramp_project(c, q, cap, up, down, prev))
    return 3 if lo <= s <= hi else 4


def _pair_draw(name, seed):
    """a drawn plate (no floors: budget contexts refuse them) with budgets by row: of the rows whose clamped step breaks a ramp every
    second one keeps its default budgets (branch 3), the others get helpers_ramp_budget.draw_budget's (branch 4); the rows whose
    clamped step keeps its ramps get e_max = 0.6 of its sum (branch 2, or 4 where the relaxed row breaks a ramp)"""
    d = price_plate(name, False, seed)
    pp = d["pp"]
    c, q = step_centres(pp, d["c2"], drawn_before(d), d["prm"]["gamma"])
    rng = np.random.default_rng(1000 + seed)
    lo, hi = np.zeros(pp.G), np.full(pp.G, np.inf)
    k = 0
    for g in range(pp.G):
        cap, up, down, prev = d["cap"][g], d["up"][g], d["down"][g], float(d["prev"][g])
        x0 = np.clip(c[g], 0.0, cap)
        if ramp_infeasibility(x0, cap, up, down, prev) > 0.0:
            if k % 2 == 0:
                lo[g], hi[g] = draw_budget(rng, k, c[g], q[g], cap, up, down, prev)
            k += 1
        elif path_sum(x0) > 1e-6 * float(pp.gen_pmax[g]) and up > 0.0:
            hi[g] = max(0.6 * path_sum(x0), 1.05 * path_sum(extreme_paths(cap, up, down, prev)[0]))      # (above the smallest feasible sum)
    branch = [_branch(c[g], q[g], d["cap"][g], d["up"][g], d["down"][g], float(d["prev"][g]), lo[g], hi[g]) for g in range(pp.G)]
    nu = np.zeros(pp.G)
    for g in range(pp.G):
        if branch[g] in (2, 4):
            info = {}
            ramp_budget_project(c[g], q[g], d["cap"][g], d["up"][g], d["down"][g], float(d["prev"][g]), lo[g], hi[g], info)
            nu[g] = info["nu"]
    return d, lo, hi, branch, nu, q


@pytest.mark.parametrize("name,seed", [("7x5", 11), ("3x70", 11)])
def test_one_step_of_the_pair(hip_api, name, seed):
    """DOPF_F2_GEN_RAMP_BUDGET at T = 5 and 70, budgets that send rows through branches 3 (the ramps alone) and 4 (the pair search):
    the certificate and the twin with shift = nu / q, nu from budget_price(), at the bounds of the plate test. Branches 3 and 4 both
    occur, a quarter of the rows are priced and both signs occur — counted by the twins from the drawn state."""
    d, lo, hi, branch, nu_twin, q = _pair_draw(name, seed)
    pp = d["pp"]
    n, pos, neg = coverage(plate_prices(d, False, drawn_before(d), shift=nu_twin / q))
    assert 3 in branch and 4 in branch and 4 * n >= pp.G and pos and neg, (branch, n, pos, neg)
    h = pair_engine(hip_api, pp, (d["up"], d["down"]), d["prev"], (lo, hi), **d["prm"])
    assert np.array_equal(h.ramp_price(), np.zeros((pp.G, pp.T)))
    set_from(h, d["st"], 2)
    before = state_of(h)
    h.iterate(1)
    P, rp, nu = state_of(h)["P"], h.ramp_price(), h.budget_price()
    cert, apart, priced = _check_rows(d, plate_prices(d, False, before, P=P, shift=nu / q), rp, name)
    for g in range(pp.G):
        if branch[g] in (1, 2):
            assert np.array_equal(rp[g], np.zeros(pp.T)), (g, branch[g])          # the ramps kept: exact zeros
    print(f"pair {name}: rows by branch {branch}, certificate {cert:.2e}, |rp - twin| {apart:.2e} of q pmax, {priced}/{pp.G} rows priced, "
          f"nu {np.array2string(nu, precision=3)}")
    assert 4 * priced >= pp.G and np.any(rp > 0.0) and np.any(rp < 0.0)
    assert h.solver_failures() == 0


# ---- 3. nothing else moved ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["ramp", "ramp+floors", "pair"])
def test_the_getter_moves_nothing(hip_api, which):
    """Three contexts of the same problem: a is asked for its prices between any two iterations, b once before the first (the call
    that starts the recording) and then only at the end, c never — it runs the instantiations of before. After 1, 4 and 7 iterations
    every getter (helpers_min_output.all_state) gives the same bits in all three, and the prices read late equal the prices read
    all along. Then c asks for the first time: zeros, the next iteration's prices after it, and nothing else moves."""
    pp = swing(synth.synthetic_case(41, 3, 5, seed=6))
    prm = params_of(pp)
    ramp = (0.2 * pp.gen_pmax, 0.25 * pp.gen_pmax)
    if which == "pair":
        warm = make_engine(hip_api, pp, flags=_capi.F_NO_FUSE | _capi.F_NO_TAIL_FUSE, **prm)
        warm.iterate(4)
        budget = draw_budgets(row_sums(warm.get_primal()[0]), row_sums(np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)))
        a, b, c = (pair_engine(hip_api, pp, ramp, None, budget, **prm) for _ in range(3))
    else:
        a, b, c = (ramp_engine(hip_api, pp, ramp, None, **prm) for _ in range(3))
        if which == "ramp+floors":
            for e in (a, b, c):
                e.set_min_output(0.1 * pp.gen_pmax)
    zeros = np.zeros((pp.G, pp.T))
    assert np.array_equal(b.ramp_price(), zeros)
    done = 0
    for upto in (1, 4, 7):
        while done < upto:
            a.ramp_price()
            a.iterate(1)
            b.iterate(1)
            c.iterate(1)
            done += 1
        last = a.ramp_price()
        assert same_bits(all_state(a), all_state(b)) and same_bits(all_state(a), all_state(c)), (which, upto)
        assert np.array_equal(last, b.ramp_price()) and np.any(last != 0.0)
    assert a.solver_failures() == 0 and b.solver_failures() == 0 and c.solver_failures() == 0
    assert np.array_equal(c.ramp_price(), zeros)
    for e in (a, c):
        e.iterate(1)
    assert same_bits(all_state(a), all_state(c)) and np.array_equal(a.ramp_price(), c.ramp_price()) and np.any(c.ramp_price() != 0.0)


@pytest.mark.parametrize("name", ["7x5", "3x130"])
def test_the_first_call_returns_zeros_in_a_block_that_held_prices(hip_api, name):
    """Four contexts of one shape, one after the other: each records a step's prices and is destroyed, so the next one's first call
    is handed a block of the size just freed. Its zeros must be the call's own — ordered on the context's stream before the copy that
    returns them. (scripts/fuzz_gen_coupling.py's floor-plate slice found the first call returning what the block held before: the
    array was zeroed on the null stream, which the context's non-blocking stream does not wait for.)"""
    d = price_plate(name, False, 11)
    pp = d["pp"]
    for k in range(4):
        h = _engine(hip_api, d, False, True)
        first = h.ramp_price()
        assert np.array_equal(first, np.zeros((pp.G, pp.T))), (k, int(np.count_nonzero(first)))
        set_from(h, d["st"], 2)
        h.iterate(1)
        assert np.any(h.ramp_price() != 0.0)
        h.close()


# ---- 4. the status rules -----------------------------------------------------------------------------------------------------------------

def _small():
    return swing(synth.synthetic_case(7, 0, 5, seed=3))


@pytest.mark.parametrize("which", ["ramp", "pair"])
def test_values_are_those_of_the_last_x_update(hip_api, which):
    pp = _small()
    prm = params_of(pp)
    demand = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)
    ramp = (0.1 * pp.gen_pmax, 0.1 * pp.gen_pmax)
    make = (lambda **kw: ramp_engine(hip_api, pp, ramp, None, **kw)) if which == "ramp" else \
           (lambda **kw: pair_engine(hip_api, pp, ramp, None, None, **kw))
    zeros = np.zeros((pp.G, pp.T))
    h = make(**prm)
    assert np.array_equal(h.ramp_price(), zeros)                                   # the first call returns zeros ...
    assert np.array_equal(h.ramp_price(), zeros)                                   # ... and so does every call before the first iteration
    h.trace_begin(_capi.TRACE_ALL, 8)                                             # the getter works while a trace is active
    h.iterate(3)
    rp = h.ramp_price()
    assert np.count_nonzero(np.any(rp != 0.0, axis=1)) >= 2 and h.trace_info()[3] >= 1
    h.trace_end()
    # the setters leave the values alone
    h.set_ramp(None, None, None)
    assert np.array_equal(h.ramp_price(), rp)
    st = state_of(h)
    h.set_state(P=0.5 * st["P"], lam=st["lam"], iteration=4)
    assert np.array_equal(h.ramp_price(), rp)
    h.set_demand(0.9 * demand)
    assert np.array_equal(h.ramp_price(), rp)
    h.roll_coupled(1, demand[:, :1])
    assert np.array_equal(h.ramp_price(), rp)
    if which == "ramp":
        h.set_min_output(0.05 * pp.gen_pmax)                                      # a floor set after the recording began ...
        assert np.array_equal(h.ramp_price(), rp)
    # ... until the next iteration: the ramps are unlimited now and the roll's anchor is within reach, so nothing is priced
    h.set_ramp(None, None, None)
    h.iterate(1)
    assert np.array_equal(h.ramp_price(), zeros)
    h.set_ramp(*ramp, None)                                                       # ... keeps it recording
    h.iterate(2)
    assert np.any(h.ramp_price() != 0.0)
    # a halted context computes nothing: the values stay, although the ramps are gone
    e = make(max_iters=3, **prm)
    e.ramp_price()                                                                # (starts the recording)
    assert 0 < e.iterate(5)[0] < 5                                                 # (halted at max_iters)
    rp = e.ramp_price()
    assert np.any(rp != 0.0)
    e.set_ramp(None, None, None)
    it = e.sync()[0]
    assert e.iterate(2)[0] == 0 and e.sync()[0] == it
    assert np.array_equal(e.ramp_price(), rp)


def _raw(api, e, out):
    rc = api.get_generator_ramp_price(e._ctx, None if out is None else out.ctypes.data_as(_capi.C.POINTER(_capi.C.c_double)))
    msg = api.last_error(e._ctx)
    return rc, (msg.decode() if msg else "")


def test_refusals(hip_api):
    pp = _small()
    prm = params_of(pp)
    # no ramp flag (a budget context included): DOPF_E_UNSUPPORTED, and the context runs on as before
    plain, twin = (make_engine(hip_api, pp, **prm) for _ in range(2))
    plain.iterate(2)
    twin.iterate(2)
    before = all_state(plain)
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*dopf_get_generator_ramp_price.*without DOPF_F_GEN_RAMP"):
        plain.ramp_price()
    assert same_bits(all_state(plain), before)
    plain.iterate(1)
    twin.iterate(1)
    assert same_bits(all_state(plain), all_state(twin))
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*without DOPF_F_GEN_RAMP"):
        _capi.Engine(hip_api, params=_capi.default_params(**prm), flags2=BUDGET, **pp.engine_kwargs()).ramp_price()
    # a network ramp context: 12 generators / 6 nodes / 8 lines
    net = swing(synth.synthetic_case(12, 0, 6, N=6, L=8, seed=2, fmax_factor=0.8, fmax_min=5))
    mk = lambda: _capi.Engine(hip_api, params=_capi.default_params(flags=RAMP | NET, eps=0.0, gamma=0.3), **net.engine_kwargs())
    e, t = mk(), mk()
    for x in (e, t):
        x.set_ramp(0.2 * net.gen_pmax, 0.2 * net.gen_pmax, None)
        x.iterate(2)
    before = all_state(e)
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*network rows are not priced.*L = 8"):
        e.ramp_price()
    assert same_bits(all_state(e), before)
    e.iterate(1)
    t.iterate(1)
    assert same_bits(all_state(e), all_state(t))
    # NULL with G > 0: DOPF_E_INVALID, nothing switched (the next call is still the first: zeros after two iterations)
    h, t = (ramp_engine(hip_api, pp, (0.1 * pp.gen_pmax, 0.1 * pp.gen_pmax), None, **prm) for _ in range(2))
    h.iterate(2)
    t.iterate(2)
    rc, msg = _raw(hip_api, h, None)
    assert rc == -1 and "dopf_get_generator_ramp_price: rp is NULL" in msg
    assert same_bits(all_state(h), all_state(t))
    h.iterate(1)
    t.iterate(1)
    assert same_bits(all_state(h), all_state(t))
    assert np.array_equal(h.ramp_price(), np.zeros((pp.G, pp.T)))
    # G == 0: DOPF_OK, nothing done
    nogen = synth.synthetic_case(0, 3, 5, seed=3)
    z = ramp_engine(hip_api, nogen, None, None, **params_of(nogen))
    assert _raw(hip_api, z, None)[0] == 0 and z.ramp_price().shape == (0, 5)


# ---- 5. shards ---------------------------------------------------------------------------------------------------------------------------

def _sharded_case():
    pp = swing(synth.synthetic_case(41, 7, 6, seed=4))
    rng = np.random.default_rng(4)
    up, down = draw_ramps(pp, rng)
    prev = rng.uniform(0.0, 1.0, pp.G) * pp.gen_pmax
    return pp, up, down, prev


def _same_prices(pp, got, want, q, first, who):
    """Bit for bit after the first iteration, where every rank's rows read the inputs one context reads; later the shards' lambda and
    injections differ from one context's in the last bits (their sums are added in another order), and a price is
    formed from them: 1e-9 q pmax, the bound of the one-step tests."""
    diff = float((np.abs(got - want).max(axis=1) / (q * pp.gen_pmax)).max())
    priced = int(np.count_nonzero(np.any(want != 0.0, axis=1)))
    print(f"{who}: {priced} priced rows, largest |difference| {diff:.2e} of q pmax")
    assert 4 * priced >= pp.G
    if first:
        assert np.array_equal(got, want), who
    assert diff <= BOUND, (who, diff)


def test_multi_two_shards_equal_one_context(hip_api):
    pp, up, down, prev = _sharded_case()
    g = 1.0 / (pp.G + pp.S)
    ref = ramp_engine(hip_api, pp, (up, down), prev, eps=0.0, gamma=g)
    ref.ramp_price()                                                              # (starts the recording, as m's first call does on every shard)
    p = copy.copy(pp)
    p.gen_ramp = (up, down)
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(eps=0.0, gamma=g, flags=_capi.F_COMM_HOST), gen_prev=prev,
                          **p.engine_kwargs())
    assert np.array_equal(m.ramp_price(), np.zeros((pp.G, pp.T)))
    for k in (1, 3):
        ref.iterate(k)
        assert m.iterate(k) == (k, False)
        got = m.ramp_price()
        _same_prices(pp, got, ref.ramp_price(), 1.0 + g, k == 1, "multi")
    n0 = m.shard(0).G
    assert np.array_equal(np.concatenate([m.shard(i).ramp_price() for i in range(2)]), got) and 0 < n0 < pp.G
    assert hip_api.multi_get_generator_ramp_price(m._m, None) == -1
    m.close()


def test_sharded_admm_two_ranks_equal_one_context(hip_api):
    import torch
    pp, up, down, prev = _sharded_case()
    g = 1.0 / (pp.G + pp.S)
    ref = ramp_engine(hip_api, pp, (up, down), prev, eps=0.0, gamma=g)
    ranks = [pkg.ShardedADMM(pp, r, 2, all_reduce=lambda: None, eps=0.0, gamma=g, flags=RAMP) for r in range(2)]
    for sh in ranks:
        sh.set_ramp(up, down, prev)                                               # all G values: each rank takes its slice
        assert not np.any(sh.ramp_price(all_reduce=lambda x: x))                  # (every context's first call starts its recording)
    assert not np.any(ref.ramp_price())
    done = 0
    for upto in (1, 4):
        while done < upto:
            done += 1
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
            ref.iterate(1)
        parts = [sh.ramp_price(all_reduce=lambda x: x) for sh in ranks]
        for sh, part in zip(ranks, parts):
            a, b = sh.shard.meta["gen_range"]
            assert part.shape == (pp.G, pp.T) and not np.any(part[:a]) and not np.any(part[b:])
        _same_prices(pp, parts[0] + parts[1], ref.ramp_price(), 1.0 + g, upto == 1, "sharded")


# ---- 6. convergence to the LP's ramp duals -----------------------------------------------------------------------------------------------

def _ramp_case():
    node = pkg.Node("plate", [55, 75, 95, 125, 85, 65], True)
    gens = [pkg.Generator(f"g{i}", mc, pm, "k", node) for i, (mc, pm) in enumerate(zip([5, 20, 40, 70], [50, 60, 40, 60]))]
    return [node], gens


def test_converged_prices_are_the_lps_ramp_duals(hip_api):
    """One plate, T = 6, demand (55, 75, 95, 125, 85, 65), units (mc, pmax) = (5, 50), (20, 60), (40, 40), (70, 60); unit 0 has
    ramp_up = 12, an unlimited ramp_down and starts from p_prev = 0; the others have unlimited ramps and the anchor 0. The host LP:
    objective 7040, P0 = (12, 24, 36, 48, 50, 50), prices (20, 20, 20, 40, 20, 20); the objective's slope in ramp_up is -230 on both
    sides (+-0.1) and in p_prev -80, so the duals are unique and rp[0, :] = (80, 65, 50, 35, 0, 0). The run stops at eps = 1e-6. The
    bound on max_t |rp[0,t] - want_t| is 10 T x the largest |lambda_t + LP price_t| of the same run — the row's price is a sum of up
    to T price differences; the 10 is test_converged_price_is_the_lps_water_value's — and holds against -ramp_dual of the device LP
    too. The other units' prices are exactly 0. Measured on an MI355X: 129 iterations to the stop test, rp[0] = (80.0000554,
    65.0000541, 50.0000542, 34.9999998, 0, 0), largest gap 5.5e-5 (5.5e-5 against the device LP's duals too), largest price gap
    4.2e-5 (bound 2.5e-3), cost 7039.99997."""
    nodes, gens = _ramp_case()
    pp = pkg.pack(nodes, gens, [], [])
    inf = np.inf
    ramp = lambda u: (np.array([u, inf, inf, inf]), np.full(4, inf))
    solve = lambda u, p0: central.solve_central_packed(pp, gen_ramp=ramp(u), gen_prev=np.array([p0, 0.0, 0.0, 0.0]))
    want, below, above, later = solve(12.0, 0.0), solve(11.9, 0.0), solve(12.1, 0.0), solve(12.0, 0.1)
    assert abs(want.objective - 7040.0) <= 1e-6
    assert np.abs(want.generation[0] - [12, 24, 36, 48, 50, 50]).max() <= 1e-6
    assert np.abs(want.system_price - [20, 20, 20, 40, 20, 20]).max() <= 1e-6
    assert abs((want.objective - below.objective) / 0.1 + 230.0) <= 1e-5 and abs((above.objective - want.objective) / 0.1 + 230.0) <= 1e-5
    assert abs((later.objective - want.objective) / 0.1 + 80.0) <= 1e-5
    target = np.array([80.0, 65.0, 50.0, 35.0, 0.0, 0.0])
    dev, duals = central.central_reference_coupled_on_device(nodes, gens, [], [], gen_ramp=ramp(12.0), gen_prev=np.zeros(4), duals=True)
    h = ramp_engine(hip_api, pp, ramp(12.0), np.zeros(4), eps=1e-6, max_iters=200000)
    assert not np.any(h.ramp_price())                                            # (starts the recording)
    done, conv = h.iterate(200000)
    rp, st = h.ramp_price(), state_of(h)
    price_gap = float(np.abs(-st["lam"] - want.system_price).max())
    gap, gap_dev = float(np.abs(rp[0] - target).max()), float(np.abs(rp[0] + duals["ramp_dual"][0]).max())
    bound = 10.0 * pp.T * price_gap
    print(f"converged {conv} after {done} iterations, rp[0] = {np.array2string(rp[0], precision=7)}, largest gap {gap:.3e}, against the "
          f"device LP's -ramp_dual {np.array2string(-duals['ramp_dual'][0], precision=7)}: {gap_dev:.3e}; largest price gap {price_gap:.3e} "
          f"(bound {bound:.3e}), cost {float(st['cost'][0]):.6f} (LP {want.objective:.6f}, device LP {dev.objective:.6f})")
    assert conv and done < 200000
    assert np.array_equal(rp[1:], np.zeros((3, pp.T)))
    assert gap <= bound, (gap, bound)
    assert gap_dev <= bound, (gap_dev, bound)
    assert h.solver_failures() == 0
