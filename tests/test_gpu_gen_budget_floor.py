"""dopf_set_generator_budget_min_output on the GPU: the budget kernels' step with the clip [floor, cap] (the MN
instantiations of k_gen_budget and k_gen_budget_win) against the NumPy reference that sorts every breakpoint
(helpers_budget_floor.budget_project_floor) and the one-multiplier certificate with the floors as the lower ends; the bits of the
kernels without floors; the setter's rules and the four entries that repeat its feasibility test; setting between graph replays;
convergence to the host LP with budgets and floors; two shards against one context; the coupled roll. Shapes, set-up and tolerances
are tests/test_gpu_gen_budget.py's and tests/test_gpu_gen_budget_windows.py's: 1e-9 scaled by max(1, gen_pmax) for a primal value,
1e-8 for the certificate, 1e-9 scaled for a budget's violation, 1e-9 relative for a price, 1e-3 relative for a converged cost."""
import copy
import re

import numpy as np
import pytest

from decentralopf_jl_amd import _capi, central, synth
from helpers import make_engine, set_from, state_of
from helpers_budget import BUDGET, CHAIN, _slices, budget_engine, budget_violation, draw_budgets_by_state, row_sums
from helpers_budget_floor import budget_kkt_violation, budget_project_floor, set_floor_raw, stationarity_at, x_of
from helpers_min_output import all_state, floor_of, same_bits
from helpers_quadratic import params_of
from test_gpu_gen_budget import EXTRAS, SHAPES, _close, _grad, _sharding_case, swing
from test_gpu_gen_budget_windows import WINDOWS, _setup

pytestmark = pytest.mark.gpu
AV = _capi.F_GEN_AVAILABILITY
RAMP = _capi.F_GEN_RAMP
PAIRS = ("plain", "availability+c2")
WHOLE = ["7x5", "9xT1", "11+2xT130", "70+6xT96-3-nodes", "3xT600-long", "net-12xT4-N6-L8", "net-12+3xT70-N6-L8", "net-12xT4-wide-chain"]
TABLES = {"7x5-2-5": WINDOWS["7x5-2-5"], "7x5-every-step": WINDOWS["7x5-every-step"], "11+2xT130": WINDOWS["11+2xT130"],
          "net-12+3xT70-N6-L8": WINDOWS["net-12+3xT70-N6-L8"]}


def floors_of(pp):
    """p_min = 0.5 gen_pmax for g % 4 != 3, else 0"""
    return np.where(np.arange(pp.G) % 4 != 3, 0.5 * pp.gen_pmax, 0.0)


def _shift(lo, hi, least):
    """budgets drawn above the floor sum, moved back by it; an end at its default stays the default (the row then runs the
    default-budget path of the kernel, and no bound sits within rounding of the floor sum)"""
    return np.where(lo > 0.0, lo + least, 0.0), np.where(np.isfinite(hi), hi + least, np.inf)


def row_budgets(pp, steps, fl, cap):
    """the four classes of helpers_budget.draw_budgets_by_state, dealt from the clamped-to-[floor, cap] step's sums above the floor sum"""
    S = row_sums([budget_project_floor(steps[g], fl[g], cap[g]) for g in range(pp.G)])
    least, room = row_sums(fl), row_sums(cap)
    lo, hi, _ = draw_budgets_by_state(S - least, room - least)
    return _shift(lo, hi, least)


def unit_budgets(pp, steps, fl, cap, ends):
    """helpers_budget._unit_budgets with floors: (e_min, e_max) of shape (G, n_win), every (row, window) unit's class dealt from the
    unit's own sums above its floor sum; of the two deals (all units in one, window by window) the one whose smallest class is larger"""
    sl = _slices(ends)
    x0 = [budget_project_floor(steps[g], fl[g], cap[g]) for g in range(pp.G)]
    sums = lambda X: np.array([[row_sums([X[g][s]])[0] for s in sl] for g in range(pp.G)])
    S, room, least = sums(x0), sums(cap), sums(fl)
    lo, hi, _ = draw_budgets_by_state((S - least).ravel(), (room - least).ravel())
    deals = [_shift(lo.reshape(S.shape), hi.reshape(S.shape), least), (np.zeros(S.shape), np.full(S.shape, np.inf))]
    for j in range(len(ends)):
        a, b, _ = draw_budgets_by_state(S[:, j] - least[:, j], room[:, j] - least[:, j])
        deals[1][0][:, j], deals[1][1][:, j] = _shift(a, b, least[:, j])

    def smallest_class(deal):
        sides = []
        for g in range(pp.G):
            for j, s in enumerate(sl):
                info = {}
                budget_project_floor(steps[g][s], fl[g][s], cap[g][s], deal[0][g, j], deal[1][g, j], info)
                sides.append(info["side"])
        return min(sides.count(k) for k in (1, -1, 0))
    return max(deals, key=smallest_class)


def _floor_setup(hip_api, shape, extra, eager, ends=None):
    """test_gpu_gen_budget_windows._setup (both engines in the flagless twin's warm-up state), then the floors, the budgets drawn above
    the floor sums (whole-horizon, or per window with ends), and both set on the budget engine — the floors last"""
    pp, prm, h, twin, c2, cap, steps, before, env = _setup(hip_api, shape, extra, eager, ends or ())
    p_min = floors_of(pp)
    fl = np.array([floor_of(p_min[g], cap[g]) for g in range(pp.G)])
    if ends is None:
        lo, hi = row_budgets(pp, steps, fl, cap)
        h.set_energy_budget(lo, hi)
        lo, hi = lo[:, None], hi[:, None]
    else:
        lo, hi = unit_budgets(pp, steps, fl, cap, ends)
        h.set_energy_budget_windows(ends, lo, hi)
    h.set_budget_min_output(p_min)
    return pp, prm, h, twin, c2, cap, steps, before, env, p_min, fl, lo, hi


# (shape, window ends or None for whole-horizon budgets)
ONE_STEP = [(n, None) for n in WHOLE] + [(n, TABLES[n][1]) for n in TABLES]


@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
@pytest.mark.parametrize("extra", PAIRS)
@pytest.mark.parametrize("name,ends", ONE_STEP, ids=[n if e is None else "win-" + n for n, e in ONE_STEP])
def test_one_step_against_the_reference_and_the_certificate(hip_api, name, ends, extra, eager):
    """One step from the twin's warm-up state, row by row (unit by unit with a table): P against budget_project_floor (1e-9 scaled), the
    one-multiplier certificate with the floors as the lower ends (1e-8) and with the stored price (1e-9 (1 + |mc| + max |lambda|), the
    price tests' bound), the budget within 1e-9 scaled, no step below its floor, the stored price against the reference's nu (1e-9
    relative to max(1, |nu|)) wherever the unit has one multiplier only, a free row or unit the bits of clampd(the flagless twin's
    centre, floor, cap), D and C the twin's bits, no solver failure. At least a fifth of the units bind above, a fifth below and a fifth
    are free, according to the reference; wherever a unit has more than one step at least one searched unit holds a step that sits on a
    floor > 0 and was above it at nu = 0, on 70+6xT96 and 11+2xT130 (whole-horizon) a tenth of all rows. What the reference alone gives
    (counted by the NumPy reference from the flagless twin's warm-up state): 7x5 3 / 2 / 2 of 7 and 1 such row, 9xT1 5 / 2 / 2 of 9
    and none, 70+6xT96 35 / 18 / 17 of 70 and 16 (19 with availability + c2), 11+2xT130 5 / 3 / 3 of 11 and 3 (4), 3xT600 1 / 1 / 1
    and 1, the networks 6 / 3 / 3 of 12 and 1 (12+3xT70 with availability + c2: 3); with tables 7x5-2-5 6 / 4 / 4 of 14 units and 1
    (2), 11+2xT130 18 / 14 / 12 of 44 and 6 (8), 12+3xT70 18 / 9 / 9 of 36 and 7 (10), 7x5-every-step 16 / 10 / 9 of 35 (14 / 9 / 12)
    and none: a one-step unit has nothing to redistribute (as 9xT1's rows), so the condition is not asked of a table of one-step
    windows — the one share lowered, to what the reference gives there. The multiplier is the only one in every searched unit on the
    plates and in all but one or two of 9 and 27 on 12+3xT70, whose rows can sit on flats of the node's table.
    Observed on an MI355X, the largest over all cases: |P - reference| 2.0e-14, certificate 1.8e-12, budget violation 1.8e-14, price
    7.1e-14, the certificate with the stored price 8.3e-6 of its bound."""
    shape = name if ends is None else TABLES[name][0]
    pp, prm, h, twin, c2, cap, steps, before, _, p_min, fl, lo, hi = _floor_setup(hip_api, shape, extra, eager, ends)
    assert np.array_equal(h.budget_min_output(), p_min)
    price_of = h.budget_price if ends is None else h.budget_window_price
    assert not np.any(price_of())                                 # (whole-horizon: starts the recording)
    h.iterate(1)
    twin.iterate(1)
    after, other = state_of(h), state_of(twin)
    nu = price_of().reshape(pp.G, -1)
    grad = _grad(pp, c2, before, prm, after["P"])
    worst = cert = viol = price = own = 0.0
    lam_max = float(np.abs(before["lam"]).max())
    unique = moved = 0
    sides = []
    for g in range(pp.G):
        scale = max(1.0, float(pp.gen_pmax[g]))
        for j, s in enumerate(_slices(ends or (pp.T,))):
            info = {}
            want = budget_project_floor(steps[g][s], fl[g][s], cap[g][s], lo[g, j], hi[g, j], info)
            got = after["P"][g][s]
            sides.append(info["side"])
            moved += info["moved_onto_floor"]
            worst = max(worst, float(np.abs(got - want).max()) / scale)
            infeas, stat, _ = budget_kkt_violation(got, grad[g][s], fl[g][s], cap[g][s], lo[g, j], hi[g, j])
            cert = max(cert, stat)
            viol = max(viol, budget_violation(got, lo[g, j], hi[g, j]) / scale)
            assert infeas <= 1e-9 * scale, (g, j, infeas)
            assert np.all(got >= fl[g][s]) and np.all(got <= cap[g][s]), (g, j)          # the box itself: exactly
            bound = 1e-9 * (1.0 + abs(float(pp.gen_mc[g])) + lam_max)
            own = max(own, stationarity_at(got, grad[g][s], fl[g][s], cap[g][s], nu[g, j]) / bound)
            if info["side"] != 0:
                # one multiplier only: phi strictly decreasing through nu* (the test of tests/test_gpu_gen_budget_windows.py)
                d = 1e-6 * max(1.0, abs(info["nu"]))
                target = hi[g, j] if info["side"] > 0 else lo[g, j]
                f = lambda v: sum(x_of(st, a, c, v) for st, a, c in zip(steps[g][s], fl[g][s], cap[g][s]))
                if f(info["nu"] - d) - target >= 1e-12 * scale and target - f(info["nu"] + d) >= 1e-12 * scale:
                    unique += 1
                    price = max(price, abs(nu[g, j] - info["nu"]) / max(1.0, abs(info["nu"])))
                assert (nu[g, j] > 0.0) == (info["side"] > 0), (g, j, nu[g, j])
            else:
                assert nu[g, j] == 0.0, (g, j)
                assert np.array_equal(got, np.maximum(other["P"][g][s], fl[g][s])), (g, j)      # clampd(centre, floor, cap), bit for bit
    n = len(sides)
    above, below, free = sides.count(1), sides.count(-1), sides.count(0)
    print(f"{name} {'whole' if ends is None else ends} {extra}: |P - reference| {worst:.2e} (scaled), certificate {cert:.2e}, budget "
          f"violation {viol:.2e} (scaled), price {price:.2e} (relative; {unique}/{above + below} searched units with one multiplier), "
          f"certificate with the device's nu {own:.2e} of its bound, units binding above {above}/{n}, below {below}/{n}, free {free}/{n}, "
          f"searched units with a step moved onto a floor > 0: {moved}")
    assert 5 * above >= n and 5 * below >= n and 5 * free >= n, (above, below, free, n)
    if max(s.stop - s.start for s in _slices(ends or (pp.T,))) > 1:
        assert moved >= 1, moved
    if ends is None and name in ("70+6xT96-3-nodes", "11+2xT130"):
        assert 10 * moved >= pp.G, (moved, pp.G)
    assert worst <= 1e-9, worst
    assert cert <= 1e-8, cert
    assert viol <= 1e-9, viol
    assert price <= 1e-9, price
    assert own <= 1.0, own
    assert np.array_equal(after["D"], other["D"]) and np.array_equal(after["C"], other["C"])      # the storages do not see any of it
    assert h.solver_failures() == 0


# ---- bits ---------------------------------------------------------------------------------------------------------------------------------

def _second(hip_api, pp, prm, h, c2, extra, env):
    """a second budget engine in the state and with the availability and c2 of h (its budgets and floors are the caller's to set)"""
    st, it, flags = env
    e = budget_engine(hip_api, pp, flags=flags, **prm)
    if EXTRAS[extra][0]:
        e.set_availability(h._mirror["gen_avail"], h._mirror["gen_avail_of"])
    if EXTRAS[extra][1]:
        e.set_quadratic_cost(c2)
    set_from(e, st, it)
    return e


BITS = [("7x5", None), ("11+2xT130", None), ("net-12+3xT70-N6-L8", None), ("7x5-2-5", (2, 5)), ("11+2xT130", (1, 64, 65, 130)),
        ("net-12+3xT70-N6-L8", (10, 35, 70))]


@pytest.mark.parametrize("extra", PAIRS)
@pytest.mark.parametrize("name,ends", BITS, ids=[n if e is None else "win-" + n for n, e in BITS])
def test_floors_of_zero_and_null_give_the_bits_of_the_kernels_without_floors(hip_api, name, ends, extra):
    """an all-zero array runs the floor instantiations: P, the duals, the sums and the prices over 3 iterations are the bits of the same
    context without the call; a NULL call goes back to the kernels of before: the same bits again"""
    shape = name if ends is None else TABLES[name][0]
    pp, prm, h, twin, c2, cap, steps, before, env = _setup(hip_api, shape, extra, False, ends or ())
    twin.close()
    fl = np.zeros(cap.shape)
    plain = _second(hip_api, pp, prm, h, c2, extra, env)
    if ends is None:
        lo, hi = row_budgets(pp, steps, fl, cap)
        for e in (h, plain):
            e.set_energy_budget(lo, hi)
            assert not np.any(e.budget_price())
    else:
        lo, hi = unit_budgets(pp, steps, fl, cap, ends)
        for e in (h, plain):
            e.set_energy_budget_windows(ends, lo, hi)
    price = (lambda e: e.budget_price()) if ends is None else (lambda e: e.budget_window_price())
    # (the same budgets again: the status reset the floor setter makes on h)
    touch = (lambda e: e.set_energy_budget(lo, hi)) if ends is None else (lambda e: e.set_energy_budget_windows(ends, lo, hi))
    h.set_budget_min_output(np.zeros(pp.G))
    touch(plain)
    for k in range(3):
        h.iterate(1)
        plain.iterate(1)
        assert same_bits(all_state(h), all_state(plain)) and np.array_equal(price(h), price(plain)), k
    assert np.any(price(h) != 0.0)
    h.set_budget_min_output(None)
    assert not np.any(h.budget_min_output())
    touch(plain)
    for k in range(3):
        h.iterate(1)
        plain.iterate(1)
        assert same_bits(all_state(h), all_state(plain)) and np.array_equal(price(h), price(plain)), k
    assert h.solver_failures() == 0


@pytest.mark.parametrize("extra", PAIRS)
@pytest.mark.parametrize("name", ["7x5", "11+2xT130", "net-12+3xT70-N6-L8"])
def test_one_window_with_floors_is_the_whole_horizon_budget_with_floors(hip_api, name, extra):
    pp, prm, whole, twin, c2, cap, steps, before, env, p_min, fl, lo, hi = _floor_setup(hip_api, name, extra, False)
    twin.close()
    assert not np.any(whole.budget_price())
    win = _second(hip_api, pp, prm, whole, c2, extra, env)
    win.set_energy_budget_windows([pp.T], lo, hi)
    win.set_budget_min_output(p_min)
    for k in (1, 3, 3):
        whole.iterate(k)
        win.iterate(k)
        assert same_bits(all_state(win), all_state(whole)), k
        assert np.array_equal(win.budget_window_price()[:, 0], whole.budget_price())
    assert np.any(whole.budget_price() != 0.0)
    assert win.solver_failures() == 0 and whole.solver_failures() == 0


# ---- the setter ---------------------------------------------------------------------------------------------------------------------------

def _small():
    return swing(synth.synthetic_case(7, 0, 5, seed=3))


def test_refusals_store_nothing(hip_api):
    """every refusal of include/dopf.h, then the repeat checks of the budget, windows, availability and coupled-roll entries; after all
    of them the stored floors, the budgets and the next iterations' bits are those of an untouched twin"""
    pp = _small()
    prm = params_of(pp)
    G, T = pp.G, pp.T
    pm = pp.gen_pmax
    # DOPF_E_UNSUPPORTED: no budget flag; a ramp context; and the old setter on a budget context, as before
    plain = make_engine(hip_api, pp, **prm)
    assert set_floor_raw(plain, 0.1 * pm)[0] == -4 and "dopf_set_generator_budget_min_output" in set_floor_raw(plain, 0.1 * pm)[1]
    ramp = make_engine(hip_api, pp, flags=RAMP, **prm)
    rc, msg = set_floor_raw(ramp, 0.1 * pm)
    assert rc == -4 and "dopf_set_generator_budget_min_output" in msg
    pair = _capi.Engine(hip_api, params=_capi.default_params(flags=RAMP, **prm), flags2=BUDGET | _capi.F2_GEN_RAMP_BUDGET, **pp.engine_kwargs())
    rc, msg = set_floor_raw(pair, 0.1 * pm)
    assert rc == -4 and "dopf_set_generator_budget_min_output" in msg and "DOPF_F_GEN_RAMP" in msg
    p_min = np.where(np.arange(G) % 2 == 0, 0.4 * pm, 0.0)
    hi = np.where(np.arange(G) == 2, 0.5 * T * pm, np.inf)           # generator 2 (a floor of 0.4 pmax): 2.0 pmax needed, 2.5 allowed
    lo = np.where(np.arange(G) == 4, 0.3 * T * pm, 0.0)
    prof, of = np.full((1, T), 0.75), np.zeros(G, dtype=np.int32)
    h, twin = (budget_engine(hip_api, pp, (lo, hi), flags=AV, **prm) for _ in range(2))
    for e in (h, twin):
        e.set_availability(prof, of)
        e.set_budget_min_output(p_min)
        e.iterate(3)
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*minimum output"):
        h.set_min_output(0.1 * pm)                                    # dopf_set_generator_min_output keeps refusing budget contexts

    def bad(a, g, v):
        x = np.array(a, dtype=np.float64)
        x[g] = v
        return x
    # DOPF_E_INVALID, naming the entry and g: the values, then the floor sum against e_max
    for arr, what in ((bad(p_min, 1, np.nan), r"g = 1\]"), (bad(p_min, 3, np.inf), r"g = 3\]"), (bad(p_min, 5, -1e-3), r"g = 5\]"),
                      (bad(p_min, 6, 1.01 * pm[6]), r"g = 6\]"),
                      (bad(p_min, 2, 0.51 * pm[2]), r"g = 2 cannot stay under e_max")):          # 5 x 0.51 pmax > 2.5 pmax
        rc, msg = set_floor_raw(h, arr)
        assert rc == -1 and "dopf_set_generator_budget_min_output" in msg and re.search(what, msg), (what, msg)
    # the repeat checks, each naming the calling entry
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_energy_budget: generator g = 2 cannot stay under e_max"):
        h.set_energy_budget(lo, bad(hi, 2, 0.39 * T * pm[2]))         # below 5 x 0.4 pmax
    # the availability entry: floors only fall with the caps, so its refusal comes with caps that rise — generator 2 out for two steps
    # (its floors sum to 3 x 0.4 pmax), e_max = 1.3 pmax set under that outage, then the outage ends: 2.0 pmax needed
    out = np.vstack([prof, np.concatenate([[0.0, 0.0], np.full(T - 2, 0.75)])[None, :]])
    av, avtwin = (budget_engine(hip_api, pp, flags=AV, **prm) for _ in range(2))
    for e in (av, avtwin):
        e.set_availability(out, bad(of, 2, 1).astype(np.int32))
        e.set_energy_budget(lo, bad(hi, 2, 1.3 * pm[2]))
        e.set_budget_min_output(p_min)
        e.iterate(3)
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_availability: generator g = 2 cannot stay under e_max"):
        av.set_availability(prof, of)
    assert np.array_equal(np.asarray(av._mirror["gen_avail"]).reshape(out.shape), out)
    # the coupled roll: what is left of e_max after k steps, and a stated new budget
    P = h.get_primal()[0]
    k = 2
    tail = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, T)[:, :k]
    tight = budget_engine(hip_api, pp, (None, bad(hi, 2, P[2, :k].sum() + 0.39 * T * pm[2])), flags=AV, **prm)
    tight.set_availability(prof, of)
    tight.set_budget_min_output(p_min)
    set_from(tight, state_of(h), h.get_residuals()[3])
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_roll_horizon_coupled: generator g = 2 cannot stay under e_max"):
        tight.roll_coupled(k, tail)                                    # left: 0.39 T pmax < 0.4 T pmax
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_roll_horizon_coupled: generator g = 2 cannot stay under e_max"):
        h.roll_coupled(k, tail, budget=(lo, bad(hi, 2, 0.39 * T * pm[2])))
    # with a table: the windows entry's own repeat check, naming g and j
    ends = (2, T)
    wlo, whi = np.zeros((G, 2)), np.full((G, 2), np.inf)
    win, wtwin = (budget_engine(hip_api, pp, flags=AV, **prm) for _ in range(2))
    for e in (win, wtwin):
        e.set_availability(prof, of)
        e.set_energy_budget_windows(ends, wlo, whi)
        e.set_budget_min_output(p_min)
        e.iterate(2)
    whi_bad = whi.copy()
    whi_bad[4, 1] = 0.39 * (T - 2) * pm[4]
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_energy_budget_windows: generator g = 4 cannot stay under e_max.*window j = 1"):
        win.set_energy_budget_windows(ends, wlo, whi_bad)
    whi_ok = whi.copy()
    whi_ok[4, 1] = 0.41 * (T - 2) * pm[4]
    for e in (win, wtwin):
        e.set_energy_budget_windows(ends, wlo, whi_ok)
    rc, msg = set_floor_raw(win, bad(p_min, 4, 0.42 * pm[4]))
    assert rc == -1 and "dopf_set_generator_budget_min_output" in msg and "g = 4" in msg and "window j = 1" in msg, msg
    for a, b in ((h, twin), (av, avtwin), (win, wtwin)):
        assert np.array_equal(a.budget_min_output(), p_min) and np.array_equal(b.budget_min_output(), p_min)
        assert a.generator_coupling()["e_max"].tolist() == b.generator_coupling()["e_max"].tolist()
        assert a.iterate(4) == b.iterate(4)
        assert same_bits(all_state(a), all_state(b))
    assert np.array_equal(win.energy_budget_windows()[2], whi_ok)


def test_setting_between_graph_replays(hip_api):
    """array, another array, NULL, array: after each the next iterations equal those of a fresh context given that state and those
    floors; the iteration counter and the state stay, converged is reset"""
    pp = _small()
    prm = params_of(pp)
    warm = make_engine(hip_api, pp, flags=CHAIN, **prm)
    warm.iterate(6)
    cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
    S = row_sums(warm.get_primal()[0])
    hi = np.where(np.arange(pp.G) % 2 == 0, np.maximum(0.7 * S, 0.45 * row_sums(cap)), np.inf)
    lo = np.zeros(pp.G)
    h = budget_engine(hip_api, pp, (lo, hi), **prm)
    h.iterate(6)
    for p_min in (0.4 * pp.gen_pmax, np.where(np.arange(pp.G) % 3 == 0, 0.2 * pp.gen_pmax, 0.0), None, 0.3 * pp.gen_pmax):
        st, it = state_of(h), h.get_residuals()[3]
        h.set_budget_min_output(p_min)
        assert h.get_residuals()[3] == it and h.sync() == (it, False)
        now = state_of(h)
        for k in ("P", "lam", "inj"):
            assert np.array_equal(now[k], st[k]), k
        fresh = budget_engine(hip_api, pp, (lo, hi), **prm)
        if p_min is not None:
            fresh.set_budget_min_output(p_min)
        for e in (h, fresh):                                           # (both from the getters' values: the same node sums)
            set_from(e, st, it)
        for k in (1, 3):
            h.iterate(k)
            fresh.iterate(k)
            assert same_bits(all_state(h), all_state(fresh)), k
        want = np.zeros(pp.G) if p_min is None else p_min
        assert np.array_equal(h.budget_min_output(), want)
        P = h.get_primal()[0]
        assert np.all(P >= want[:, None]) and np.all(P.sum(axis=1) <= hi + 1e-9 * pp.gen_pmax)
    assert h.solver_failures() == 0


# ---- convergence to the host LP with budgets and floors -------------------------------------------------------------------------------------

def test_converged_run_against_the_host_lp(hip_api):
    """7x5 with swing(0.85, 1.15) and gamma = 0.3: the largest unit that sits at its cap throughout the free optimum is held to 70 % of
    its energy (e_max) and must run at half its capacity at least; the dearest unit must run at a fifth of its capacity. The four LPs
    (free 72 730, floors only 73 326, budgets only 80 482, both 81 078) differ pairwise by more than 1e-6 relative; the run converges
    with its cost within 1e-3 of the LP with both, budgets and floors within 1e-9 scaled. Measured on an MI355X: 59 iterations to the
    stop test, cost within 9.1e-6 of the LP's 81 078, budget violation 4.2e-16 scaled, no step under its floor."""
    pp = swing(synth.synthetic_case(7, 0, 5, seed=3), 0.85, 1.15)
    free = central.solve_central_packed(pp)
    full = np.all(free.generation >= pp.gen_pmax[:, None] * (1.0 - 1e-9), axis=1)
    assert np.any(full)
    held = int(np.argmax(np.where(full, pp.gen_pmax, -np.inf)))
    dear = int(np.argmax(pp.gen_mc))
    assert held != dear
    hi = np.full(pp.G, np.inf)
    hi[held] = 0.7 * free.generation[held].sum()
    p_min = np.zeros(pp.G)
    p_min[held], p_min[dear] = 0.5 * pp.gen_pmax[held], 0.2 * pp.gen_pmax[dear]
    floors = central.solve_central_packed(pp, gen_min_output=p_min)
    budgets = central.solve_central_packed(pp, gen_budget=(None, hi))
    want = central.solve_central_packed(pp, gen_budget=(None, hi), gen_min_output=p_min)
    obj = [free.objective, floors.objective, budgets.objective, want.objective]
    on_floor = int(np.sum(np.abs(want.generation[held] - p_min[held]) <= 1e-7 * pp.gen_pmax[held]))
    print(f"LP objectives: free {obj[0]:.1f}, floors only {obj[1]:.1f}, budgets only {obj[2]:.1f}, both {obj[3]:.1f}; the held unit sits "
          f"on its floor in {on_floor} steps")
    for i in range(4):
        for k in range(i + 1, 4):
            assert abs(obj[i] - obj[k]) > 1e-6 * max(obj[i], obj[k]), (i, k, obj)
    assert on_floor == 3
    for got, stated in zip(obj, (72730.0, 73326.0, 80482.0, 81078.0)):
        assert abs(got - stated) < 1.0, obj
    h = budget_engine(hip_api, pp, (None, hi), max_iters=20000, gamma=0.3)
    h.set_budget_min_output(p_min)
    done, conv = h.iterate(20000)
    st = state_of(h)
    gap = abs(float(st["cost"][0]) - want.objective) / want.objective
    scale = np.maximum(1.0, pp.gen_pmax)
    viol = max(budget_violation(st["P"][g], 0.0, hi[g]) / scale[g] for g in range(pp.G))
    under = float(np.max((p_min[:, None] - st["P"]) / scale[:, None]))
    print(f"converged {conv} after {done} iterations, relative cost gap {gap:.2e}, largest budget violation {viol:.2e}, largest shortfall "
          f"under a floor {under:.2e} (both scaled)")
    assert conv
    assert viol <= 1e-9 and under <= 1e-9, (viol, under)
    assert gap <= 1e-3, gap
    assert h.solver_failures() == 0


# ---- two shards against one context ---------------------------------------------------------------------------------------------------------

def _sharded_floors(hip_api):
    pp, g, lo, hi = _sharding_case(hip_api)
    p_min = floors_of(pp)
    least = pp.T * p_min                                               # (no availability: floor = p_min in every step)
    hi = np.where(np.isfinite(hi), np.maximum(hi, 1.05 * least), np.inf)
    lo = np.minimum(lo, hi)
    return pp, g, lo, hi, p_min


def test_multi_two_shards_equal_one_context(hip_api):
    pp, g, lo, hi, p_min = _sharded_floors(hip_api)
    ref = budget_engine(hip_api, pp, (lo, hi), eps=0.0, gamma=g)
    ref.set_budget_min_output(p_min)
    q = copy.copy(pp)
    q.gen_budget, q.gen_budget_min_output = (lo, hi), p_min            # (through engine_kwargs: the constructor applies the floors last)
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
    assert np.all(P >= p_min[:, None])
    assert np.array_equal(np.concatenate([m.shard(i).budget_min_output() for i in range(2)]), p_min)
    bad = p_min.copy()
    bad[pp.G - 1] = -1.0                                               # the second shard's last entry: nothing stored on the first either
    with pytest.raises(_capi.DopfError, match="shard 1"):
        m.set_budget_min_output(bad)
    assert np.array_equal(m.shard(0).budget_min_output(), p_min[:m.shard(0).G])
    m.set_budget_min_output(None)
    ref.set_budget_min_output(None)
    ref.iterate(3)
    m.iterate(3)
    _close(state_of(m.shard(1)), state_of(ref), ("lam", "inj", "cost"), "floors removed")
    m.close()


def test_sharded_admm_two_ranks_equal_one_context(hip_api):
    import torch
    from conftest import pkg
    pp, g, lo, hi, p_min = _sharded_floors(hip_api)
    ref = budget_engine(hip_api, pp, (lo, hi), eps=0.0, gamma=g)
    ref.set_budget_min_output(p_min)
    q = copy.copy(pp)
    q.gen_budget = (lo, hi)
    ranks = [pkg.ShardedADMM(q, r, 2, all_reduce=lambda: None, eps=0.0, gamma=g) for r in range(2)]
    for sh in ranks:
        sh.set_energy_budget(lo, hi)
        sh.set_budget_min_output(p_min)                                # all G values: each rank takes its slice
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
    P = np.concatenate([s["P"] for s in got])
    assert np.abs(P - want["P"]).max() <= 1e-9 * max(1.0, np.abs(want["P"]).max())
    assert np.all(P >= p_min[:, None])


# ---- the coupled roll -------------------------------------------------------------------------------------------------------------------------

def test_roll_coupled_with_floors_equals_the_host_route(hip_api):
    """k = 2 on 7x5: the in-place roll of a budget context with floors against Engine.roll's host route (a new context with what is left
    of the budgets, then the floors), at the tolerances of tests/test_gpu_roll_coupled.py: 1e-9 scaled after the roll and after one
    iteration, 1e-8 after twelve; the floors are left alone"""
    from test_gpu_roll_coupled import scaled
    pp = _small()
    prm = params_of(pp)
    p_min = floors_of(pp)
    cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
    hi = np.where(np.arange(pp.G) % 2 == 0, 0.95 * row_sums(cap), np.inf)            # what is left after two steps holds five steps' floors
    engines = []
    for _ in range(2):
        e = budget_engine(hip_api, pp, (None, hi), **prm)
        e.set_budget_min_output(p_min)
        e.iterate(7)
        engines.append(e)
    h, ref = engines
    k = 2
    tail = np.round(np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, :k] * 1.05) + 1.0
    used = h.get_primal()[0][:, :k].sum(axis=1)
    h.roll_coupled(k, tail)
    ref.roll(k, tail)
    assert np.array_equal(h.budget_min_output(), p_min) and np.array_equal(ref.budget_min_output(), p_min)
    assert np.array_equal(h.generator_coupling()["e_max"], np.maximum(0.0, hi - used))
    d, where, _ = scaled(state_of(h), state_of(ref))
    assert d <= 1e-9, (where, d)
    h.iterate(1)
    ref.iterate(1)
    d1, where, cost = scaled(state_of(h), state_of(ref))
    assert d1 <= 1e-9 and cost <= 1e-9, (where, d1, cost)
    assert np.all(h.get_primal()[0] >= p_min[:, None])
    h.iterate(11)
    ref.iterate(11)
    d12, where, cost = scaled(state_of(h), state_of(ref))
    print(f"roll with floors vs the host route: {d:.2e} after the roll, {d1:.2e} after one iteration, {d12:.2e} after twelve (scaled)")
    assert d12 <= 1e-8 and cost <= 1e-8, (where, d12, cost)
    assert h.solver_failures() == 0
