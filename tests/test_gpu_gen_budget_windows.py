"""dopf_set_generator_energy_budget_windows on the GPU: k_gen_budget_win's step window by window against the NumPy
reference (helpers_budget.budget_project on the slices) and each window's one-multiplier certificate; one window against the
whole-horizon budget and free windows against default budgets, bit for bit; one-step windows against their closed form; a window against
the truncated problem; the setter's rules; convergence to the host LP with window rows; two shards against one context. Shapes, set-up
and tolerances are tests/test_gpu_gen_budget.py's: 1e-9 scaled by max(1, gen_pmax) for a primal value, 1e-8 for the certificate, 1e-9
scaled for a budget's violation, 1e-3 relative for a converged cost."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from decentralopf_jl_amd import _capi, central, synth
from helpers import make_engine, set_from, state_of
from helpers_budget import (BUDGET, CHAIN, _slices, _unit_budgets, budget_engine, budget_kkt_violation, budget_project, budget_violation,
                            draw_budgets_by_state, row_sums, stationarity_at)
from helpers_quadratic import QC, draw_c2, params_of
from helpers_budget import x_of
from test_gpu_gen_budget import CONV, EXTRAS, SHAPES, _chain, _close, _grad, _prm, _profiles, _steps, swing

pytestmark = pytest.mark.gpu
AV = _capi.F_GEN_AVAILABILITY

# name -> (shape of test_gpu_gen_budget.SHAPES, window ends)
WINDOWS = {
    "7x5-2-5": ("7x5", (2, 5)),
    "7x5-every-step": ("7x5", (1, 2, 3, 4, 5)),
    "9xT1": ("9xT1", (1,)),
    "70+6xT96-3-nodes": ("70+6xT96-3-nodes", (24, 48, 72, 96)),
    "11+2xT130": ("11+2xT130", (1, 64, 65, 130)),          # the 65-step window takes a second trip of the lane loop
    "3xT600-long": ("3xT600-long", (300, 600)),
    "net-12+3xT70-N6-L8": ("net-12+3xT70-N6-L8", (10, 35, 70)),
    "net-12xT4": ("net-12xT4-N6-L8", (1, 4)),
    "net-12xT4-wide-chain": ("net-12xT4-wide-chain", (1, 4)),
}
PAIRS = ("plain", "availability+c2")


def _window_profiles(pp, rng, ends):
    """test_gpu_gen_budget._profiles, whose remedy for a one-step horizon is applied to one-step windows too: draw_profiles' zeros
    (every fourth step and a fifth of the others) would leave every row with a profile a box of one point in such a window, with
    nothing to project: at those steps the zeros get a value in [0.2, 1] instead"""
    prof, of = _profiles(pp, rng)
    for s in _slices(ends):
        if s.stop - s.start == 1 and pp.T > 1:
            col = prof[:, s.start]
            prof[:, s.start] = np.where(col == 0.0, rng.uniform(0.2, 1.0, col.shape), col)
    return prof, of


def _setup(hip_api, shape, extra, eager, ends=()):
    """test_gpu_gen_budget._setup without its budgets: (pp, prm, budget engine, flagless twin on the chain, c2, cap, steps, state
    before, (state, iteration, flags)), both engines in the twin's warm-up state"""
    make, flags, warm = SHAPES[shape]
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
        prof, of = _window_profiles(pp, rng, ends)
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
    return pp, prm, h, twin, c2, cap, steps, before, (st, it, flags)


CASES = [(n, x) for n in WINDOWS for x in PAIRS]


@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
@pytest.mark.parametrize("name,extra", CASES, ids=[f"{n}-{x}" for n, x in CASES])
def test_one_step_against_the_reference_and_the_certificate(hip_api, name, extra, eager):
    """One step from the twin's warm-up state, unit by unit: P against budget_project on the window's slice (1e-9 scaled), the window's
    certificate with its own nu (1e-8) and with the stored price (1e-9 (1 + |mc| + max |lambda|), the price tests' bound), the budget
    within 1e-9 scaled, the stored price against the reference's nu (1e-9 relative to max(1, |nu|)) wherever the window has one
    multiplier only (at least half of the searched units on a plate), a free unit the bits of the flagless twin, D and C its bits, no solver failure. At least a fifth of the units bind
    above, a fifth below and a fifth are free, according to the reference (9xT1: the shares it gives, one unit of each class at least).
    Observed on an MI355X, the largest over all cases: |P - reference| 2.0e-14, certificate 1.7e-12, budget violation 8.3e-15,
    price 7.1e-14."""
    shape, ends = WINDOWS[name]
    pp, prm, h, twin, c2, cap, steps, before, _ = _setup(hip_api, shape, extra, eager, ends)
    lo, hi = _unit_budgets(pp, steps, cap, ends)
    h.set_energy_budget_windows(ends, lo, hi)
    assert not np.any(h.budget_window_price())                    # zeros after the allocation
    h.iterate(1)
    twin.iterate(1)
    after, other = state_of(h), state_of(twin)
    nu = h.budget_window_price()
    grad = _grad(pp, c2, before, prm, after["P"])
    worst = cert = viol = price = own = 0.0
    lam_max = float(np.abs(before["lam"]).max())
    unique = 0
    sides = []
    for g in range(pp.G):
        scale = max(1.0, float(pp.gen_pmax[g]))
        for j, s in enumerate(_slices(ends)):
            info = {}
            want = budget_project(steps[g][s], cap[g][s], lo[g, j], hi[g, j], info)
            sides.append(info["side"])
            worst = max(worst, float(np.abs(after["P"][g][s] - want).max()) / scale)
            infeas, stat, _ = budget_kkt_violation(after["P"][g][s], grad[g][s], cap[g][s], lo[g, j], hi[g, j])
            cert = max(cert, stat)
            viol = max(viol, budget_violation(after["P"][g][s], lo[g, j], hi[g, j]) / scale)
            assert infeas <= 1e-9 * scale, (g, j, infeas)
            # the window's certificate with the DEVICE's nu, the bound of tests/test_gpu_gen_budget_price.py for it
            bound = 1e-9 * (1.0 + abs(float(pp.gen_mc[g])) + lam_max)
            own = max(own, stationarity_at(after["P"][g][s], grad[g][s], cap[g][s], nu[g, j]) / bound)
            # ... and the reference's nu wherever the window has one multiplier only: phi strictly decreasing through nu* (on a network
            # x_t(nu) is flat across a kink of the node's table, and a window whose steps all sit on flats or box ends meets its bound
            # on a whole interval of nu: any point of it is a multiplier)
            if info["side"] != 0:
                d = 1e-6 * max(1.0, abs(info["nu"]))
                target = hi[g, j] if info["side"] > 0 else lo[g, j]
                f = lambda v: sum(x_of(st, c, v) for st, c in zip(steps[g][s], cap[g][s]))
                if f(info["nu"] - d) - target >= 1e-12 * scale and target - f(info["nu"] + d) >= 1e-12 * scale:
                    unique += 1
                    price = max(price, abs(nu[g, j] - info["nu"]) / max(1.0, abs(info["nu"])))
            if info["side"] == 0:
                assert nu[g, j] == 0.0, (g, j)
                assert np.array_equal(after["P"][g][s], other["P"][g][s]), (g, j)          # the clamped step's bits
            else:
                assert (nu[g, j] > 0.0) == (info["side"] > 0), (g, j, nu[g, j])
    n = len(sides)
    above, below, free = sides.count(1), sides.count(-1), sides.count(0)
    print(f"{name} {extra}: |P - reference| {worst:.2e} (scaled), certificate {cert:.2e}, budget violation {viol:.2e} (scaled), price "
          f"{price:.2e} (relative; {unique}/{above + below} searched units with one multiplier only), certificate with the device's nu "
          f"{own:.2e} of its bound, units binding above {above}/{n}, below {below}/{n}, free {free}/{n}")
    if shape == "9xT1":
        assert above >= 1 and below >= 1 and free >= 1, (above, below, free)
    else:
        assert 5 * above >= n and 5 * below >= n and 5 * free >= n, (above, below, free, n)
    assert worst <= 1e-9, worst
    assert cert <= 1e-8, cert
    assert viol <= 1e-9, viol
    assert price <= 1e-9, price
    assert own <= 1.0, own
    if pp.L == 0:                                                 # (a network's tables leave fewer: reported above)
        assert 2 * unique >= above + below, (unique, above, below)
    assert np.array_equal(after["D"], other["D"]) and np.array_equal(after["C"], other["C"])      # the storages do not see the budgets
    assert h.solver_failures() == 0


THREE = ["7x5-2-5", "11+2xT130", "net-12+3xT70-N6-L8"]


@pytest.mark.parametrize("extra", PAIRS)
@pytest.mark.parametrize("name", THREE)
def test_one_window_is_the_whole_horizon_budget_bit_for_bit(hip_api, name, extra):
    """the same state and budgets in a context with dopf_set_generator_energy_budget and in one with one window: every array's bits
    after 1, 4 and 7 iterations, and the window price the bits of dopf_get_generator_budget_price"""
    shape, _ = WINDOWS[name]
    pp, prm, h, twin, c2, cap, steps, before, (st, it, flags) = _setup(hip_api, shape, extra, False)
    S = row_sums([budget_project(steps[g], cap[g]) for g in range(pp.G)])
    lo, hi, _ = draw_budgets_by_state(S, row_sums(cap))
    twin.close()
    whole = h
    whole.set_energy_budget(lo, hi)
    assert not np.any(whole.budget_price())                       # (starts the recording)
    win = budget_engine(hip_api, pp, flags=flags, **prm)
    if EXTRAS[extra][0]:
        win.set_availability(whole._mirror["gen_avail"], whole._mirror["gen_avail_of"])
    if EXTRAS[extra][1]:
        win.set_quadratic_cost(c2)
    set_from(win, st, it)
    win.set_energy_budget_windows([pp.T], lo[:, None], hi[:, None])
    for k in (1, 3, 3):
        whole.iterate(k)
        win.iterate(k)
        a, b = state_of(win), state_of(whole)
        for key in a:
            assert np.array_equal(a[key], b[key]), (key, k)
        assert np.array_equal(win.budget_window_price()[:, 0], whole.budget_price())
    assert np.any(win.budget_window_price() != 0.0)
    assert win.solver_failures() == 0 and whole.solver_failures() == 0


@pytest.mark.parametrize("extra", PAIRS)
@pytest.mark.parametrize("name", THREE)
def test_every_window_free_is_the_budget_context_with_default_budgets(hip_api, name, extra):
    shape, ends = WINDOWS[name]
    pp, prm, h, twin, c2, cap, steps, before, (st, it, flags) = _setup(hip_api, shape, extra, False)
    twin.close()
    win = budget_engine(hip_api, pp, flags=flags, **prm)
    if EXTRAS[extra][0]:
        win.set_availability(h._mirror["gen_avail"], h._mirror["gen_avail_of"])
    if EXTRAS[extra][1]:
        win.set_quadratic_cost(c2)
    set_from(win, st, it)
    win.set_energy_budget_windows(ends)                           # e_min None, e_max None: all 0, all +inf
    for k in (1, 3, 3):
        h.iterate(k)
        win.iterate(k)
        a, b = state_of(win), state_of(h)
        for key in a:
            assert np.array_equal(a[key], b[key]), (key, k)
    assert not np.any(win.budget_window_price()) and win.solver_failures() == 0


@pytest.mark.parametrize("extra", PAIRS)
def test_windows_of_one_step_are_a_clamp(hip_api, extra):
    """T windows of one step on 7x5: P[g,t] = clamp(clamped step, e_min[g,t], min(e_max[g,t], cap[g,t])), exactly — the clamped step
    being the flagless twin's bits"""
    pp, prm, h, twin, c2, cap, steps, before, _ = _setup(hip_api, "7x5", extra, False, tuple(range(1, 6)))
    rng = np.random.default_rng(23)
    lo = np.where(rng.random(cap.shape) < 0.5, 0.0, rng.uniform(0.0, 1.0, cap.shape) * cap)
    hi = np.where(rng.random(cap.shape) < 0.4, np.inf, lo + rng.uniform(0.0, 1.0, cap.shape) * (cap - lo))
    h.set_energy_budget_windows(np.arange(1, pp.T + 1), lo, hi)
    h.iterate(1)
    twin.iterate(1)
    got, x0 = state_of(h)["P"], state_of(twin)["P"]
    want = np.minimum(np.maximum(x0, lo), np.minimum(hi, cap))
    moved = int(np.sum(want != x0))
    print(f"one-step windows {extra}: {moved}/{want.size} units moved by their budget, largest |P - clamp| {float(np.abs(got - want).max()):.2e}")
    assert moved >= want.size // 4
    assert np.array_equal(got, want)
    nu = h.budget_window_price()
    assert np.all((nu > 0.0) == (want < x0)) and np.all((nu < 0.0) == (want > x0))
    assert h.solver_failures() == 0


def test_a_window_against_the_truncated_problem(hip_api):
    """11+2xT130 with ends (64, 130): the rows' steps in window 0 are those of a budget context of the first 64 steps of the same case,
    with the same state slices (dopf_set_state) and the same budgets. 1e-9 scaled; the arithmetic is the same, so bits are expected and
    printed. A unit that read outside its window would see other prices, other centres and other caps here."""
    pp, prm, h, twin, c2, cap, steps, before, (st, it, flags) = _setup(hip_api, "11+2xT130", "availability+c2", False)
    twin.close()
    ends, T0 = (64, 130), 64
    lo, hi = _unit_budgets(pp, steps, cap, ends)
    h.set_energy_budget_windows(ends, lo, hi)
    short = copy.copy(pp)
    short.T = T0
    short.demand = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, :T0].copy()
    cut = budget_engine(hip_api, short, flags=flags, **prm)          # (the parameters do not depend on T)
    cut.set_availability(h._mirror["gen_avail"][:, :T0], h._mirror["gen_avail_of"])
    cut.set_quadratic_cost(c2)
    cut.set_state(P=st["P"][:, :T0], D=st["D"][:, :T0], C_=st["C"][:, :T0], avg_U=st["avg_U"][:, :T0], avg_K=st["avg_K"][:, :T0],
                  lam=st["lam"][:T0], mu=st["mu"][:, :T0], rho=st["rho"][:, :T0], iteration=it)
    cut.set_energy_budget(lo[:, 0], hi[:, 0])
    assert not np.any(cut.budget_price())
    h.iterate(1)
    cut.iterate(1)
    a, b = state_of(h)["P"][:, :T0], state_of(cut)["P"]
    diff = float(np.max(np.abs(a - b) / np.maximum(1.0, pp.gen_pmax)[:, None]))
    print(f"window 0 against the truncated problem: largest difference {diff:.2e} (scaled), bits equal: {np.array_equal(a, b)}; prices "
          f"equal: {np.array_equal(h.budget_window_price()[:, 0], cut.budget_price())}")
    assert diff <= 1e-9, diff
    assert np.count_nonzero(h.budget_window_price()[:, 0]) >= pp.G // 3
    assert h.solver_failures() == 0 and cut.solver_failures() == 0


# ---- the setter -------------------------------------------------------------------------------------------------------------------------

def _small():
    return swing(synth.synthetic_case(7, 0, 5, seed=3))


def _same(a, b):
    sa, sb = state_of(a), state_of(b)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k


def test_setter_refusals_store_nothing(hip_api):
    pp = _small()
    prm = params_of(pp)
    G, T = pp.G, pp.T
    ends = np.array([2, 5], dtype=np.int32)
    entry = "dopf_set_generator_energy_budget_windows"
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*" + entry + ".*DOPF_F2_GEN_ENERGY_BUDGET"):          # DOPF_E_UNSUPPORTED
        make_engine(hip_api, pp, **prm).set_energy_budget_windows(ends)
    pair = _capi.Engine(hip_api, params=_capi.default_params(flags=_capi.F_GEN_RAMP, **prm), flags2=BUDGET | _capi.F2_GEN_RAMP_BUDGET,
                        **pp.engine_kwargs())
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*" + entry + ".*DOPF_F2_GEN_RAMP_BUDGET"):
        pair.set_energy_budget_windows(ends)
    lo = np.repeat(0.2 * pp.gen_pmax[:, None], 2, axis=1)
    hi = np.repeat(1.5 * pp.gen_pmax[:, None], 2, axis=1)
    prof, of = np.full((1, T), 0.75), np.zeros(G, dtype=np.int32)
    h, twin = (budget_engine(hip_api, pp, flags=AV, **prm) for _ in range(2))
    for e in (h, twin):
        e.set_availability(prof, of)
        e.set_energy_budget_windows(ends, lo, hi)
        e.iterate(3)

    def bad(a, g, j, v):
        x = a.copy()
        x[g, j] = v
        return x

    def call(n, e, a, b):
        f = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)
        e, a, b = None if e is None else np.ascontiguousarray(e, dtype=np.int32), f(a), f(b)
        rc = hip_api.set_generator_energy_budget_windows(h._ctx, n, None if e is None else e.ctypes.data_as(_capi.c_int32_p), _capi._dp(a), _capi._dp(b))
        return rc, (hip_api.last_error(h._ctx) or b"").decode()
    for args, code, what in (((-1, ends, lo, hi), -1, "n_win = -1"), ((T + 1, np.arange(1, T + 2), None, None), -1, "n_win = 6"),
                             ((2, None, lo, hi), -1, "win_end is NULL"), ((0, ends, None, None), -1, "n_win = 0"),
                             ((2, [2, 2], lo, hi), -1, r"win_end\[j = 1\]"), ((2, [0, 5], lo, hi), -1, r"win_end\[j = 0\]"),
                             ((2, [2, 4], lo, hi), -1, r"win_end\[j = 1\] = 4 is not T = 5"),
                             ((2, ends, bad(lo, 2, 1, np.nan), hi), -1, "e_min of g = 2, j = 1"),
                             ((2, ends, bad(lo, 5, 0, -1e-3), hi), -1, "e_min of g = 5, j = 0"),
                             ((2, ends, bad(lo, 1, 1, np.inf), None), -1, "e_min of g = 1, j = 1"),
                             ((2, ends, lo, bad(hi, 4, 0, np.nan)), -1, "e_max of g = 4, j = 0"),
                             ((2, ends, None, bad(hi, 3, 1, -1.0)), -1, "e_max of g = 3, j = 1"),
                             ((2, ends, lo, bad(hi, 0, 1, 0.1 * pp.gen_pmax[0])), -1, "at g = 0, j = 1"),
                             # above the window's sum of caps: 0.75 x 2 pmax in window 0
                             ((2, ends, bad(lo, 6, 0, 1.51 * pp.gen_pmax[6]), None), -1, "g = 6 .*window j = 0")):
        rc, msg = call(*args)
        assert rc == code and entry in msg and re.search(what, msg), (args[0], rc, msg)
    # the mutual exclusion, this direction: the whole-horizon setter with an array, its price getter and the coupled roll
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_energy_budget:.*sub-window"):
        h.set_energy_budget(None, 3.0 * pp.gen_pmax)
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_get_generator_budget_window_price"):
        h.budget_price()
    tail = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, :1]
    for roll in (h.roll_coupled, h.roll):
        with pytest.raises(_capi.DopfError, match=r"\(-4\).*dopf_roll_horizon_coupled.*sub-window"):
            roll(1, tail)
    for e in (h, twin):
        e.set_energy_budget(None, None)                           # (NULL, NULL) stays allowed
    # the availability setter's re-check, window by window: generator 6's caps drop to 0.05 pmax, 0.1 pmax over window 0, under its 0.2
    low = np.vstack([prof, np.full((1, T), 0.05)])
    of6 = of.copy()
    of6[6] = 1
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*dopf_set_generator_availability.*g = 6 .*window j = 0"):
        h.set_availability(low, of6)
    got = h.energy_budget_windows()
    assert np.array_equal(got[0], ends) and np.array_equal(got[1], lo) and np.array_equal(got[2], hi)
    assert np.array_equal(h.budget_window_price(), twin.budget_window_price())
    assert h.iterate(5) == twin.iterate(5)
    _same(h, twin)
    assert np.array_equal(h.budget_window_price(), twin.budget_window_price())
    # ... and the other direction: a stored whole-horizon budget refuses the table
    other = budget_engine(hip_api, pp, (None, 3.0 * pp.gen_pmax), **prm)
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*" + entry + r".*dopf_set_generator_energy_budget\(ctx, NULL, NULL\)"):
        other.set_energy_budget_windows(ends)
    assert other.energy_budget_windows() is None
    other.set_energy_budget(None, None)
    other.set_energy_budget_windows(ends)


def test_set_between_graph_replays_changed_n_win_and_removal(hip_api):
    """a set with the same n_win between two graph replays matches a fresh context; a changed n_win and n_win = 0 match eager contexts,
    bitwise; after the removal the whole-horizon getter and the coupled roll work again"""
    pp = _small()
    prm = params_of(pp)
    cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
    h = budget_engine(hip_api, pp, **prm)
    h.iterate(16)

    def table(ends):
        P = h.get_primal()[0]
        S = np.array([[row_sums([P[g][s]])[0] for s in _slices(ends)] for g in range(pp.G)])
        room = np.array([[row_sums([cap[g][s]])[0] for s in _slices(ends)] for g in range(pp.G)])
        lo, hi, _ = draw_budgets_by_state(S.ravel(), room.ravel())
        return lo.reshape(S.shape), hi.reshape(S.shape)
    for ends, eager in (((2, 5), False), ((3, 5), False), ((1, 3, 5), True), (None, True), ((2, 5), True), (None, True)):
        st, it = state_of(h), h.get_residuals()[3]
        lo, hi = (None, None) if ends is None else table(ends)
        h.set_energy_budget_windows(ends, lo, hi)
        assert h.get_residuals()[3] == it and h.sync() == (it, False)          # the counter is kept, converged is 0
        now = state_of(h)
        for k in ("P", "lam", "inj"):
            assert np.array_equal(now[k], st[k]), k
        fresh = budget_engine(hip_api, pp, flags=_capi.F_NO_GRAPH if eager else 0, **prm)
        if ends is not None:
            fresh.set_energy_budget_windows(ends, lo, hi)
        for e in (h, fresh):
            set_from(e, st, it)
        h.iterate(4)
        fresh.iterate(4)
        _same(h, fresh)
        if ends is None:
            assert h.energy_budget_windows() is None
            with pytest.raises(_capi.DopfError, match=r"\(-1\).*no table is set"):
                h.budget_window_price()
        else:
            assert np.array_equal(h.budget_window_price(), fresh.budget_window_price())
            assert h.budget_window_price().shape == (pp.G, len(ends))
    assert h.solver_failures() == 0
    # with the table removed the whole-horizon price getter and the coupled roll work again
    assert h.budget_price().shape == (pp.G,)
    P = h.get_primal()[0]
    h.roll_coupled(1, np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, :1])
    assert np.array_equal(h.get_primal()[0][:, :pp.T - 1], P[:, 1:])


def test_guard_mode(hip_api):
    """DOPF_GUARD=1: every device array ends on the last byte of its own mapping, so an access past an end is a GPU memory fault in a
    child process (tests/budget_windows_worker.py), not a silent read of a neighbour"""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "budget_windows_worker.py")
    r = subprocess.run([sys.executable, worker], env=dict(os.environ, DOPF_GUARD="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "budget windows worker: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---- convergence to the host LP with window rows ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CONV))
def test_converged_run_against_the_host_lp(hip_api, name):
    """test_gpu_gen_budget.CONV's two cases with ends (2, 5) on the plate and (midpoint, T) on the three-node network. The generator
    that delivers most in the free optimum (network: the wind unit) is held in the LAST window to a share of what it delivers there:
    0.7 on the plate, 0.9 on the network. On the plate that unit (g = 5, 49 per MWh) has a twin of the same marginal cost with spare
    capacity (g = 0), which would take over at no cost — the LP's objective would not rise at any share; so every unit of the held
    unit's marginal cost with spare capacity in that window is held there at what it delivers in the free optimum. The LP then
    rises from 72 730 to 73 381.6 and the held row's dual is -4 on both sides (the 53 per MWh unit steps in). Cost within 1e-3, budgets within 1e-9 scaled, no solver failure, within 20 000 iterations;
    the held window's price against minus the LP's dual within 10 x the largest |lambda[t] - LP price| of the same run, the bound of
    tests/test_gpu_gen_budget_price.py for that comparison. Observed on an MI355X: the plate 73 iterations, cost gap 4.0e-6, nu 3.996435
    against 4 (price gap 2.7e-3); the network 438 iterations, 2.0e-5, nu 15.9994 against 16 (price gap 1.7e-4)."""
    make, prm, held, share = CONV[name]
    pp = make()
    ends = (2, 5) if name == "7x5" else (pp.T // 2, pp.T)
    last = _slices(ends)[-1]
    free = central.solve_central_packed(pp)
    big = int(np.argmax(free.generation.sum(axis=1))) if held is None else held
    hi = np.full((pp.G, 2), np.inf)
    E_last = free.generation[:, last].sum(axis=1)
    hi[big, 1] = share * E_last[big]
    for g in range(pp.G):                                         # the held unit's twins (docstring)
        if g != big and pp.gen_mc[g] == pp.gen_mc[big] and E_last[g] < (last.stop - last.start) * pp.gen_pmax[g]:
            hi[g, 1] = E_last[g]
    want = central.solve_central_packed(pp, gen_budget_windows=(ends, None, hi))          # (infeasible: RuntimeError)
    assert want.objective > free.objective * (1.0 + 1e-6)                                # the budget binds at the optimum
    h = budget_engine(hip_api, pp, max_iters=20000, **prm)
    h.set_energy_budget_windows(ends, None, hi)
    done, conv = h.iterate(20000)
    st, nu = state_of(h), h.budget_window_price()
    gap = abs(float(st["cost"][0]) - want.objective) / want.objective
    viol = max(budget_violation(st["P"][g][s], 0.0, hi[g, j]) / max(1.0, float(pp.gen_pmax[g]))
               for g in range(pp.G) for j, s in enumerate(_slices(ends)))
    price_gap = float(np.abs(-st["lam"] - want.system_price).max())
    dual_gap = abs(nu[big, 1] + want.budget_window_dual[big, 1])
    print(f"{name}: converged {conv} after {done} iterations, relative cost gap {gap:.2e}, largest budget violation {viol:.2e} (scaled), "
          f"LP {want.objective:.4f} (without budgets {free.objective:.4f}), nu {nu[big, 1]:.6f} against -dual {-want.budget_window_dual[big, 1]:.6f}: "
          f"{dual_gap:.2e} (largest price gap {price_gap:.2e})")
    assert conv and done <= 20000
    assert viol <= 1e-9, viol
    assert gap <= 1e-3, gap
    assert dual_gap <= 10.0 * price_gap, (dual_gap, price_gap)
    assert h.solver_failures() == 0


# ---- two shards against one context -------------------------------------------------------------------------------------------------------

def _sharding_case(hip_api):
    pp = swing(synth.synthetic_case(41, 7, 6, seed=4))
    g = 1.0 / (pp.G + pp.S)
    ends = (2, 6)
    warm = make_engine(hip_api, pp, eps=0.0, gamma=g, flags=CHAIN)
    warm.iterate(4)
    P = warm.get_primal()[0]
    cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
    S = np.array([[row_sums([P[i][s]])[0] for s in _slices(ends)] for i in range(pp.G)])
    room = np.array([[row_sums([cap[i][s]])[0] for s in _slices(ends)] for i in range(pp.G)])
    lo, hi, _ = draw_budgets_by_state(S.ravel(), room.ravel())
    return pp, g, ends, lo.reshape(S.shape), hi.reshape(S.shape)


def test_multi_two_shards_equal_one_context(hip_api):
    pp, g, ends, lo, hi = _sharding_case(hip_api)
    ref = budget_engine(hip_api, pp, eps=0.0, gamma=g)
    ref.set_energy_budget_windows(ends, lo, hi)
    q = copy.copy(pp)
    q.gen_budget_windows = (ends, lo, hi)                        # (through engine_kwargs: the second word and the setter from the constructor)
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
        _close(dict(nu=m.budget_window_price()), dict(nu=ref.budget_window_price()), ("nu",), "price")
    bad = lo.copy()
    bad[pp.G - 1, 1] = -1.0                                      # the second shard's last entry: nothing stored on the first either
    with pytest.raises(_capi.DopfError, match="shard 1"):
        m.set_energy_budget_windows(ends, bad, hi)
    ref.iterate(3)
    assert m.iterate(3) == (3, False)
    _close(state_of(m.shard(0)), state_of(ref), ("lam", "inj", "cost"), "after a refusal")
    m.set_energy_budget_windows(None)
    ref.set_energy_budget_windows(None)
    ref.iterate(3)
    m.iterate(3)
    _close(state_of(m.shard(1)), state_of(ref), ("lam", "inj", "cost"), "removed")
    m.close()


def test_sharded_admm_two_ranks_equal_one_context(hip_api):
    import torch
    from conftest import pkg
    pp, g, ends, lo, hi = _sharding_case(hip_api)
    ref = budget_engine(hip_api, pp, eps=0.0, gamma=g)
    ref.set_energy_budget_windows(ends, lo, hi)
    q = copy.copy(pp)
    q.gen_budget_windows = (ends, lo, hi)                        # every rank's engine gets the word and its rows from engine_kwargs
    ranks = [pkg.ShardedADMM(q, r, 2, all_reduce=lambda: None, eps=0.0, gamma=g) for r in range(2)]
    for sh in ranks:
        assert sh.engine.flags2 & BUDGET
        a, b = sh.shard.meta["gen_range"]
        assert np.array_equal(sh.energy_budget_windows()[1], lo[a:b])
        sh.set_energy_budget_windows(ends, lo, hi)               # all G rows: each rank takes its own
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
    nu = sum(sh.budget_window_price(all_reduce=lambda x: x) for sh in ranks)
    _close(dict(nu=nu), dict(nu=ref.budget_window_price()), ("nu",), "price")
