"""The device LP on horizons beyond 512 timesteps (csrc/kernels_central.hip, kc_sto_long and kc_gen_rows_long; csrc/central_long.h;
DESIGN.md 5v): a block walks a row in tiles of 2048 timesteps, and what the one-wave sweeps pass between lanes crosses threads, waves
and tiles. The reference for every number is the host LP (central.solve_central_packed, HiGHS) with the same inputs, never the device
solver itself. TOL, MAX_ITERS and the 1e-5 bounds are those of test_gpu_central_coupled.py.

The horizons: 513 and 600 (one tile, partly filled), 2048 (one tile, full), 2049 (one step in the second tile: every carry between
tiles feeds exactly one slot, and T - 1 is the only slot of its tile), 4100 (two whole tiles and a rest). Below 513 the long sweeps run
behind DOPF_F_DEBUG_LONG_STO (group 5): tiles with 1, 12, 65, 70 and 130 live slots."""
import functools
import time

import numpy as np
import pytest

from decentralopf_jl_amd import _capi, synth
from decentralopf_jl_amd.central import solve_central_packed
from helpers import draw_band, draw_e0
from helpers_central_coupled import INF, complementarity, draw_inputs, ramp_row_bounds, ramp_row_values, violation
from helpers_efficiency import draw_band_eff, draw_eta, levels_eff
import test_gpu_central_coupled as small
import test_gpu_central_lossy as small_lossy

pytestmark = pytest.mark.gpu

TOL = 1e-7
MAX_ITERS = 200000
CASES = {
    "copper-T513": lambda: synth.synthetic_case(8, 2, 513, seed=11),          # one tile, partly filled
    "copper-T600": lambda: synth.synthetic_case(8, 2, 600, seed=12),          # one tile, partly filled
    "net-4x5-T600": lambda: synth.synthetic_case(8, 2, 600, N=4, L=5, seed=14),
    "copper-T2048": lambda: synth.synthetic_case(6, 2, 2048, seed=13),        # one tile, full: nothing is handed over
    "copper-T2049": lambda: synth.synthetic_case(6, 2, 2049, seed=13),        # one step in the second tile: every carry
    "copper-T4100": lambda: synth.synthetic_case(6, 1, 4100, seed=15),        # two whole tiles and a rest
}
LEVEL_CASES = ("copper-T600", "copper-T2049")
LEVEL_SETS = ("e0", "e0+band", "all")                                       # kc_sto_long<., 1>, <., 2>, <., 3>
ROW_PAIRS = [("copper-T513", "both"), ("copper-T600", "ramp+prev"), ("copper-T600", "budget"), ("copper-T2049", "ramp"),
             ("copper-T2049", "ramp+prev"), ("copper-T2049", "budget"), ("net-4x5-T600", "ramp"), ("net-4x5-T600", "budget"),
             ("net-4x5-T600", "both")]
# (copper-T2049 "both" is no case: the NumPy twin of the iteration stood at a gap of 7.8e-5 after MAX_ITERS, the objective within 1.7e-8)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def _host(pp, **kw):
    return solve_central_packed(pp, duals=False, **kw)


def bounds_hold(pp, r, want):
    assert r["converged"], {k: r[k] for k in ("objective", "dual_objective", "primal_infeasibility", "gap", "iterations")}
    assert abs(r["objective"] - want) <= 1e-5 * abs(want)
    assert abs(r["dual_objective"] - want) <= 1e-5 * abs(want)
    assert r["primal_infeasibility"] <= 1e-5 * (1.0 + np.abs(pp.demand).max())


_device = {}


def solved(key, call):
    """One device solve per key, shared by the tests that look at it; (result, seconds)."""
    if key not in _device:
        t0 = time.perf_counter()
        r = call()
        _device[key] = (r, time.perf_counter() - t0)
    return _device[key]


# ---- 1. storages, no rows ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_plain(name):
    return _host(case(name)).objective


def device_plain(api, name, flags=0):
    return solved((name, "plain", flags), lambda: _capi.central_solve(api, tol=TOL, max_iters=MAX_ITERS, params=_capi.default_params(flags=flags),
                                                                      **case(name).engine_kwargs()))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", list(CASES))
def test_storages_match_the_host_lp(hip_api, name):
    """kc_sto_long<., 0> through dopf_central_solve with default flags. Iterations to TOL / seconds of the whole call on an MI355X:
    copper-T513 13 600 / 0.59, copper-T600 10 200 / 0.28, net-4x5-T600 14 200 / 0.41, copper-T2048 61 800 / 2.09, copper-T2049 61 600 /
    2.27, copper-T4100 72 600 / 4.14 — the counts of the NumPy twin of the iteration (helpers_central_coupled.pdhg with the weight
    fixed at 1), case for case; on copper-T2048 the twin was run before the device: 61 800."""
    pp, want = case(name), host_plain(name)
    r, sec = device_plain(hip_api, name)
    print(f"{name}: host {want!r} device {r['objective']!r} dual {r['dual_objective']!r} pinf {r['primal_infeasibility']:.3e} "
          f"iterations {r['iterations']} seconds {sec:.2f}")
    bounds_hold(pp, r, want)
    E = r["E"]
    assert np.abs(np.cumsum(r["C"] - r["D"], axis=1) - E).max() <= 1e-9 * (1.0 + np.abs(E).max())


@pytest.mark.timeout(120)
def test_the_callers_long_horizon_flag_changes_no_bit(hip_api):
    a, _ = device_plain(hip_api, "copper-T600")
    b, sec = device_plain(hip_api, "copper-T600", _capi.F_LONG_HORIZON)
    print(f"copper-T600 with DOPF_F_LONG_HORIZON: iterations {b['iterations']} seconds {sec:.2f}")
    assert a["iterations"] == b["iterations"]
    for k in ("objective", "dual_objective", "primal_infeasibility", "gap"):
        assert a[k] == b[k], k
    for k in small.OUT_KEYS:
        assert np.array_equal(a[k], b[k]), k


# ---- 2. levels, bands and efficiencies ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def level_inputs(name, which):
    """(eta | None, e0, band | None): e0 a mix of empty, full and half full; the band an equality target inside the reachable levels
    (under the efficiencies with "all") for every storage — the row of T - 1."""
    pp = case(name)
    rng = np.random.default_rng(11)
    ec, ed = draw_eta(pp.S, rng)
    e0 = draw_e0(pp, "mix", rng)
    if which == "e0":
        return None, e0, None
    if which == "e0+band":
        return None, e0, draw_band(pp, e0, "eq", rng)
    return (ec, ed), e0, draw_band_eff(pp, e0, ec, ed, "eq", rng)


@functools.lru_cache(maxsize=None)
def host_levels(name, which):
    eta, e0, band = level_inputs(name, which)
    return _host(case(name), initial_level=e0, terminal_level=band, efficiency=eta).objective


@pytest.mark.timeout(120)
@pytest.mark.parametrize("which", LEVEL_SETS)
@pytest.mark.parametrize("name", LEVEL_CASES)
def test_levels_bands_and_efficiencies_match_the_host_lp(hip_api, name, which):
    """kc_sto_long<., 1 .. 3>. The band's slot is T - 1: the last live slot of a partly filled tile, and at 2049 the only one of its tile.
    HiGHS is feasible on all six (checked on the CPU first). Iterations / seconds on an MI355X, e0 / e0+band / all: copper-T600
    11 200 / 0.31, 10 000 / 0.28, 9 800 / 0.27; copper-T2049 62 000 / 2.29, 47 800 / 1.75, 40 200 / 1.48."""
    pp, want = case(name), host_levels(name, which)
    eta, e0, band = level_inputs(name, which)
    r, sec = solved((name, "levels", which), lambda: _capi.central_solve(hip_api, tol=TOL, max_iters=MAX_ITERS, **pp.engine_kwargs(),
                                                                         **small_lossy.feature_kwargs(eta, e0, band)))
    print(f"{name} {which}: host {want!r} (plain {host_plain(name)!r}) device {r['objective']!r} dual {r['dual_objective']!r} "
          f"pinf {r['primal_infeasibility']:.3e} iterations {r['iterations']} seconds {sec:.2f}")
    bounds_hold(pp, r, want)
    ec, ed = (np.ones(pp.S), np.ones(pp.S)) if eta is None else eta
    E = r["E"]
    assert np.abs(levels_eff(e0, ec, ed, r["D"], r["C"]) - E).max() <= 1e-9 * (1.0 + np.abs(E).max())
    slack = 1e-5 * (1.0 + np.abs(pp.demand).max())
    assert E.min() >= -slack and (E - pp.sto_emax[:, None]).max() <= slack
    if band is not None:
        assert (band[0] - E[:, -1]).max() <= slack and (E[:, -1] - band[1]).max() <= slack


# ---- 3. ramp and budget rows -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def drawn(name):
    """Copper plates: the drawing rule of test_gpu_central_coupled.py. net-4x5-T600 (that rule is infeasible there, on the anchors):
    ramps of max(a quarter of the free optimum's largest step, pmax / 20), every third generator free, no anchor; e_max = 0.9 of the
    free optimum's energy for the generators 1::4, e_min = 0."""
    pp = case(name)
    if not name.startswith("net"):
        return draw_inputs(pp, _host)
    P = _host(pp).generation
    pmax = np.asarray(pp.gen_pmax, dtype=np.float64)
    up = np.maximum(0.25 * np.abs(np.diff(P, axis=1)).max(axis=1), pmax / 20.0)
    up[::3] = INF
    e = P.sum(axis=1)
    e_max = np.full(pp.G, INF)
    e_max[1::4] = np.where(e[1::4] > 0.0, 0.9 * e[1::4], INF)
    return dict(ramp=(up, up.copy()), prev=None, budget=(np.zeros(pp.G), e_max), rating=None)


def row_inputs(name, which):
    d = drawn(name)
    kw = {}
    if which in ("ramp", "ramp+prev", "both"):
        kw["gen_ramp"] = d["ramp"]
    if which in ("ramp+prev", "both") and d["prev"] is not None:
        kw["gen_prev"] = d["prev"]
    if which in ("budget", "both"):
        kw["gen_budget"] = d["budget"]
    return kw


@functools.lru_cache(maxsize=None)
def host_rows(name, which):
    return _host(case(name), **row_inputs(name, which)).objective


def device_rows(api, name, which, max_iters=MAX_ITERS):
    return solved((name, "rows", which, max_iters), lambda: _capi.central_solve_coupled(api, tol=TOL, max_iters=max_iters, **case(name).engine_kwargs(),
                                                                                        **row_inputs(name, which)))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,which", ROW_PAIRS)
def test_objective_matches_the_host_lp_with_the_same_rows(hip_api, name, which):
    """kc_gen_rows_long next to kc_sto_long. Iterations to TOL / seconds of the whole call on an MI355X: copper-T513 both 6 200 / 0.21;
    copper-T600 ramp+prev 14 800 / 0.49, budget 16 000 / 0.51; copper-T2049 ramp 66 000 / 2.84, ramp+prev 57 200 / 2.47, budget 32 800 /
    1.33; net-4x5-T600 ramp 31 000 / 1.06, budget 8 800 / 0.29, both 28 600 / 1.01 — the NumPy twin's counts, case for case."""
    pp, want = case(name), host_rows(name, which)
    r, sec = device_rows(hip_api, name, which)
    print(f"{name} {which}: host {want!r} device {r['objective']!r} dual {r['dual_objective']!r} pinf {r['primal_infeasibility']:.3e} "
          f"iterations {r['iterations']} seconds {sec:.2f}")
    bounds_hold(pp, r, want)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,which", ROW_PAIRS)
def test_device_objective_lies_on_the_rows_side(hip_api, name, which):
    with_set, base = host_rows(name, which), host_plain(name)
    print(f"{name} {which}: host with the set {with_set!r} base {base!r} relative difference {(with_set - base) / base:.3e}")
    assert abs(with_set - base) > 1e-4 * abs(base)                     # ten times the bound below
    r, _ = device_rows(hip_api, name, which)
    assert abs(r["objective"] - with_set) <= 1e-5 * abs(with_set)
    assert abs(r["objective"] - base) > 1e-5 * abs(base)


def row_violations(pp, kw, P):
    """(worst ramp-row violation, worst budget-row violation) of P under the inputs kw"""
    vr = vq = 0.0
    if "gen_ramp" in kw:
        lo, hi, live = ramp_row_bounds(pp.T, *kw["gen_ramp"], kw.get("gen_prev"))
        vr = float(np.where(live, violation(ramp_row_values(P, kw.get("gen_prev")), lo, hi), 0.0).max())
    if "gen_budget" in kw:
        vq = float(violation(P.sum(axis=1), kw["gen_budget"][0], kw["gen_budget"][1]).max())
    return vr, vq


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,which", ROW_PAIRS)
def test_returned_point_is_feasible_in_its_own_right(hip_api, name, which):
    pp, kw = case(name), row_inputs(name, which)
    r, _ = device_rows(hip_api, name, which)
    P, D, Cc = r["P"], r["D"], r["C"]
    slack = 1e-5 * (1.0 + np.abs(pp.demand).max())
    assert P.min() >= 0 and (P - pp.gen_pmax[:, None]).max() <= 0
    assert D.min() >= 0 and Cc.min() >= 0 and (D - pp.sto_pmax[:, None]).max() <= 0 and (Cc - pp.sto_pmax[:, None]).max() <= 0
    E = np.cumsum(Cc - D, axis=1)
    assert E.min() >= -slack and (E - pp.sto_emax[:, None]).max() <= slack
    vr, vq = row_violations(pp, kw, P)
    assert vr <= slack and vq <= slack
    if "gen_ramp" in kw and pp.T == 2049:
        # the row between the two tiles, t = 2048: it exists, and it holds
        lo, hi, live = ramp_row_bounds(pp.T, *kw["gen_ramp"], kw.get("gen_prev"))
        assert live[:, 2048].any()
        step = P[:, 2048] - P[:, 2047]
        assert np.where(live[:, 2048], np.maximum(lo[:, 2048] - step, step - hi[:, 2048]), 0.0).max() <= slack
    inj = -np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T).copy()
    np.add.at(inj, pp.gen_node, P)
    np.add.at(inj, pp.sto_node, D - Cc)
    assert np.abs(inj.sum(axis=0)).max() <= slack
    if pp.L:
        flow = np.asarray(pp.ptdf, dtype=np.float64).reshape(pp.L, pp.N) @ inj
        assert (np.abs(flow) - np.asarray(pp.f_max)[:, None]).max() <= slack
        assert np.abs(flow - r["line_utilization"]).max() <= 1e-9 * (1.0 + np.abs(flow).max())
    cost = float(pp.gen_mc @ P.sum(axis=1) + pp.sto_mc @ (D + Cc).sum(axis=1))
    assert abs(cost - r["objective"]) <= 1e-10 * cost


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,which", ROW_PAIRS)
def test_duals_follow_the_binding_side_and_are_complementary(hip_api, name, which):
    pp, kw = case(name), row_inputs(name, which)
    r, _ = device_rows(hip_api, name, which)
    G, T = pp.G, pp.T
    yr, yq = r["ramp_dual"], r["budget_dual"]
    assert yr.shape == (G, T) and yq.shape == (G,)
    bound = 1e-5 * (1.0 + abs(r["objective"]))
    up, dn = kw.get("gen_ramp", (np.full(G, np.inf), np.full(G, np.inf)))
    lo, hi, live = ramp_row_bounds(T, up, dn, kw.get("gen_prev"))
    assert np.all(yr[~live] == 0.0)                                    # no row, no dual
    assert np.all(np.isfinite(hi[yr < 0.0])) and np.all(np.isfinite(lo[yr > 0.0]))      # the sign names an end that exists
    comp_r = complementarity(yr, ramp_row_values(r["P"], kw.get("gen_prev")), lo, hi, live)
    e_min, e_max = kw.get("gen_budget", (np.zeros(G), np.full(G, np.inf)))
    has = (e_min > 0.0) | np.isfinite(e_max)
    assert np.all(yq[~has] == 0.0)
    assert np.all(np.isfinite(e_max[yq < 0.0]))
    comp_q = complementarity(yq, r["P"].sum(axis=1), e_min, e_max, has)
    print(f"{name} {which}: ramp rows with a dual {int((yr != 0).sum())}, budget rows {int((yq != 0).sum())}, "
          f"complementarity {comp_r:.3e} / {comp_q:.3e} (bound {bound:.3e})")
    assert comp_r <= bound and comp_q <= bound
    assert (yr != 0).any() or (yq != 0).any()                          # the set binds somewhere (it moves the optimum)


# ---- 4. the carries in the metrics pass: no convergence needed ---------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", ["copper-T2049", "copper-T4100"])
def test_metrics_of_an_unconverged_point_are_its_own(hip_api, name):
    """400 iterations of "both": whatever point comes back, E is its cumsum, the objective its cost and primal_infeasibility its worst
    violation, recomputed here — levels, ramp rows and budget sums across the tile boundaries."""
    pp, kw = case(name), row_inputs(name, "both")
    r, sec = device_rows(hip_api, name, "both", max_iters=400)
    print(f"{name} both, 400 iterations: objective {r['objective']!r} pinf {r['primal_infeasibility']:.6e} seconds {sec:.2f}")
    assert r["iterations"] == 400
    P, D, Cc, E = r["P"], r["D"], r["C"], r["E"]
    assert np.abs(np.cumsum(Cc - D, axis=1) - E).max() <= 1e-9 * (1.0 + np.abs(E).max())
    cost = float(pp.gen_mc @ P.sum(axis=1) + pp.sto_mc @ (D + Cc).sum(axis=1))
    assert abs(cost - r["objective"]) <= 1e-10 * cost
    inj = -np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T).copy()
    np.add.at(inj, pp.gen_node, P)
    np.add.at(inj, pp.sto_node, D - Cc)
    lev = np.cumsum(Cc - D, axis=1)
    vr, vq = row_violations(pp, kw, P)
    worst = max(np.abs(inj.sum(axis=0)).max(), (-lev).max(), (lev - pp.sto_emax[:, None]).max(), vr, vq, 0.0)
    print(f"  recomputed {worst:.6e}: balance {np.abs(inj.sum(axis=0)).max():.3e} ramp {vr:.3e} budget {vq:.3e}")
    assert worst > 0.0
    assert abs(worst - r["primal_infeasibility"]) <= 1e-9 * (1.0 + np.abs(pp.demand).max())
    _, _, live = ramp_row_bounds(pp.T, *kw["gen_ramp"], kw.get("gen_prev"))
    assert np.all(r["ramp_dual"][~live] == 0.0)


# ---- 5. the long sweeps at small T -------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", ["copper-T1", "copper-T12", "copper-T65", "copper-T130"])
def test_long_sweeps_at_small_T_reach_the_host_lp(hip_api, name):
    """test_gpu_central_coupled.py's cases and inputs ("both") with DOPF_F_DEBUG_LONG_STO in the parameters: a tile with 1, 12, 65 and
    130 live slots. (It cannot tell which sweep ran; group 1 can: the one-wave sweeps do not reach T = 513.) Iterations on an MI355X:
    1 200 / 1 400 / 4 800 / 5 800, the one-wave sweeps' counts in test_gpu_central_coupled.py; under half a second each."""
    pp, want = small.case(name), small.host_lp(name, "both")
    r, sec = solved((name, "debug"), lambda: _capi.central_solve_coupled(hip_api, tol=TOL, max_iters=MAX_ITERS,
                                                                         params=_capi.default_params(flags=_capi.F_DEBUG_LONG_STO),
                                                                         **pp.engine_kwargs(), **small.inputs(name, "both")))
    print(f"{name} both, long sweeps: host {want!r} device {r['objective']!r} dual {r['dual_objective']!r} iterations {r['iterations']} "
          f"seconds {sec:.2f}")
    bounds_hold(pp, r, want)


@pytest.mark.timeout(120)
def test_long_storage_sweep_at_T_70_with_levels_band_and_efficiencies(hip_api):
    """test_gpu_central_lossy.py's copper-T70 "all" (kc_sto_long<., 3>: e0, an equality band, efficiencies) behind the same flag."""
    name = "copper-T70"
    pp, want = small_lossy.case(name), small_lossy.host_lp(name, "all")
    r, sec = solved((name, "debug-levels"), lambda: _capi.central_solve(hip_api, tol=TOL, max_iters=MAX_ITERS,
                                                                        params=_capi.default_params(flags=_capi.F_DEBUG_LONG_STO),
                                                                        **pp.engine_kwargs(),
                                                                        **small_lossy.feature_kwargs(*small_lossy.inputs(name, "all"))))
    print(f"{name} all, long sweep: host {want!r} device {r['objective']!r} dual {r['dual_objective']!r} iterations {r['iterations']} "
          f"seconds {sec:.2f}")
    bounds_hold(pp, r, want)


# ---- 6. a decentral run lands on the device optimum ------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_decentral_run_at_T_600_lands_on_the_device_optimum(hip_api):
    """The pattern of test_gpu_central_coupled.py's landing on copper-T600: the ADMM run behind DOPF_F_LONG_HORIZON within 1e-3 of
    dopf_central_solve's objective, which is within 1e-5 of HiGHS. On an MI355X: converged after 175 iterations, 1.07e-5 from the
    device optimum."""
    pp = case("copper-T600")
    r, _ = device_plain(hip_api, "copper-T600")
    assert r["converged"]
    e = _capi.Engine(hip_api, params=_capi.default_params(gamma=1.0 / (pp.G + pp.S), max_iters=20000, flags=_capi.F_LONG_HORIZON),
                     **pp.engine_kwargs())
    done, conv = e.iterate(20000)
    cost = e.get_consensus()[4]
    print(f"decentral cost {cost!r} after {done} iterations (converged {conv}), device LP {r['objective']!r}")
    assert conv, done
    assert abs(cost - r["objective"]) / r["objective"] <= 1e-3, (cost, r["objective"], done)
