"""dopf_central_solve_coupled: the device LP with generator ramp limits, an anchor, energy budgets and a line-rating table
(csrc/kernels_central.hip, kc_gen_rows and kc_dual<., true>). The reference for every number is the host LP
(central.solve_central_packed, HiGHS) with the same inputs, never the device solver itself. The cases are those of
test_gpu_central_lossy.py plus a copper plate with T = 130 (three timesteps per lane, a partly filled last lane); TOL and the 1e-5
bounds are that file's.

Duals (ramp_dual, budget_dual) are d objective / d right-hand side, the reference's convention (central.py): negative where a row's
upper end binds — more room there lowers the cost — positive where its lower end binds, 0 elsewhere.

The inputs follow one drawing rule (helpers_central_coupled.draw_inputs): ramps of max(a tenth of the free optimum's largest step,
pmax / 50), every third generator free and every sixth one-sided; anchors two ramps below the free optimum's first step; budgets that
cut the ramped optimum's energy of every sixth generator to 80 % and lift another sixth's a fifth of the way to its capacity; ratings
of 0.9 to 1.3 f_max. Every set is feasible on every case and moves the optimum by at least 3e-3 relative (checked with HiGHS)."""
import ctypes as C
import functools

import numpy as np
import pytest

from decentralopf_jl_amd import _capi, synth
from decentralopf_jl_amd.central import solve_central_packed
from helpers_central_coupled import complementarity, draw_inputs, ramp_row_bounds, ramp_row_values

pytestmark = pytest.mark.gpu

INVALID = -1                    # DOPF_E_INVALID
TOL = 1e-7
MAX_ITERS = 200000
CASES = {
    "copper-T12": lambda: synth.synthetic_case(40, 6, 12, seed=3),
    "copper-T70": lambda: synth.synthetic_case(60, 9, 70, seed=5),      # two timesteps per lane, a partly filled wave
    "copper-T1": lambda: synth.synthetic_case(20, 5, 1, seed=9),        # the anchor's row is the only ramp row
    "copper-T65": lambda: synth.synthetic_case(60, 9, 65, seed=5),      # lane 32 holds one timestep, its second slot is empty
    "net-6x9-T24": lambda: synth.synthetic_case(60, 15, 24, N=6, L=9, seed=7, fmax_factor=1.0, fmax_min=5),      # line limits bind
    "copper-T130": lambda: synth.synthetic_case(30, 4, 130, seed=5),    # K = 3, the last lane partly filled
}
COPPER_SETS = ("ramp", "ramp+prev", "budget", "both")
NET_SETS = COPPER_SETS + ("rated", "all")
PAIRS = [(n, w) for n in CASES for w in (NET_SETS if n.startswith("net") else COPPER_SETS)]
TELLING = [(n, w) for n, w in PAIRS if (n, w) != ("copper-T1", "ramp")]      # (T = 1 without an anchor: no ramp row exists)
OUT_KEYS = ("P", "D", "C", "E", "system_price", "nodal_price", "line_utilization", "flow_upper_dual", "flow_lower_dual")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def _host(pp, **kw):
    return solve_central_packed(pp, duals=False, **kw)


@functools.lru_cache(maxsize=None)
def drawn(name):
    return draw_inputs(case(name), _host)


def inputs(name, which):
    """the keyword arguments of one set, as both solve_central_packed and _capi.central_solve_coupled take them"""
    d = drawn(name)
    kw = {}
    if which in ("ramp", "ramp+prev", "both", "all"):
        kw["gen_ramp"] = d["ramp"]
    if which in ("ramp+prev", "both", "all"):
        kw["gen_prev"] = d["prev"]
    if which in ("budget", "both", "all"):
        kw["gen_budget"] = d["budget"]
    if which in ("rated", "all"):
        kw["line_rating"] = d["rating"]
    return kw


@functools.lru_cache(maxsize=None)
def host_lp(name, which):
    return _host(case(name), **(inputs(name, which) if which else {})).objective


_device = {}


def device_lp(api, name, which):
    """One device solve per (case, set), shared by the tests that look at it."""
    if (name, which) not in _device:
        _device[name, which] = _capi.central_solve_coupled(api, tol=TOL, max_iters=MAX_ITERS, **case(name).engine_kwargs(),
                                                           **inputs(name, which))
    return _device[name, which]


# ---- 1. the objective ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,which", PAIRS)
def test_objective_matches_the_host_lp_with_the_same_inputs(hip_api, name, which):
    """Iterations to TOL on an MI355X (ramp / ramp+prev / budget / both): copper-T12 2 000 / 1 400 / 1 200 / 1 400, copper-T70 2 200 /
    2 800 / 2 200 / 6 200, copper-T65 4 000 / 4 400 / 2 400 / 4 800, copper-T130 7 400 / 10 000 / 6 600 / 5 800, copper-T1 1 000 / 1 600 /
    800 / 1 200, net-6x9-T24 8 200 / 9 200 / 7 800 / 39 200, rated 11 000, all 115 600 — with the primal weight that follows the
    iterates. With the weight fixed at 1, net-6x9-T24 "both" stalled at a gap of 2.26e-7 from iteration 60 000 to
    MAX_ITERS, and the rating table alone took 84 200."""
    pp, want = case(name), host_lp(name, which)
    r = device_lp(hip_api, name, which)
    print(f"{name} {which}: host {want!r} device {r['objective']!r} dual {r['dual_objective']!r} "
          f"pinf {r['primal_infeasibility']:.3e} iterations {r['iterations']}")
    assert r["converged"], {k: r[k] for k in ("objective", "dual_objective", "primal_infeasibility", "gap", "iterations")}
    assert abs(r["objective"] - want) <= 1e-5 * abs(want)
    assert abs(r["dual_objective"] - want) <= 1e-5 * abs(want)
    assert r["primal_infeasibility"] <= 1e-5 * (1.0 + np.abs(pp.demand).max())


# ---- 2. the test can tell the set from the base case -----------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,which", TELLING)
def test_device_objective_lies_on_the_sets_side(hip_api, name, which):
    with_set, base = host_lp(name, which), host_lp(name, "")
    print(f"{name} {which}: host with the set {with_set!r} base {base!r} relative difference {(with_set - base) / base:.3e}")
    assert abs(with_set - base) > 1e-4 * abs(base)                     # ten times the bound below
    r = device_lp(hip_api, name, which)
    assert abs(r["objective"] - with_set) <= 1e-5 * abs(with_set)
    assert abs(r["objective"] - base) > 1e-5 * abs(base)


# ---- 3. the returned point in its own right --------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,which", PAIRS)
def test_returned_point_is_feasible_in_its_own_right(hip_api, name, which):
    pp, kw = case(name), inputs(name, which)
    r = device_lp(hip_api, name, which)
    P, D, Cc = r["P"], r["D"], r["C"]
    slack = 1e-5 * (1.0 + np.abs(pp.demand).max())
    assert P.min() >= 0 and (P - pp.gen_pmax[:, None]).max() <= 0
    assert D.min() >= 0 and Cc.min() >= 0 and (D - pp.sto_pmax[:, None]).max() <= 0 and (Cc - pp.sto_pmax[:, None]).max() <= 0
    E = np.cumsum(Cc - D, axis=1)
    assert E.min() >= -slack and (E - pp.sto_emax[:, None]).max() <= slack
    if "gen_ramp" in kw:
        lo, hi, live = ramp_row_bounds(pp.T, *kw["gen_ramp"], kw.get("gen_prev"))
        val = ramp_row_values(P, kw.get("gen_prev"))
        assert np.where(live, np.maximum(lo - val, val - hi), 0.0).max() <= slack
    if "gen_budget" in kw:
        e = P.sum(axis=1)
        assert (kw["gen_budget"][0] - e).max() <= slack and (e - kw["gen_budget"][1]).max() <= slack
    inj = -np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T).copy()
    np.add.at(inj, pp.gen_node, P)
    np.add.at(inj, pp.sto_node, D - Cc)
    assert np.abs(inj.sum(axis=0)).max() <= slack
    if pp.L:
        limit = kw.get("line_rating", np.asarray(pp.f_max)[:, None] * np.ones((pp.L, pp.T)))
        flow = np.asarray(pp.ptdf, dtype=np.float64).reshape(pp.L, pp.N) @ inj
        assert (np.abs(flow) - limit).max() <= slack
        assert np.abs(flow - r["line_utilization"]).max() <= 1e-9 * (1.0 + np.abs(flow).max())
    cost = float(pp.gen_mc @ P.sum(axis=1) + pp.sto_mc @ (D + Cc).sum(axis=1))
    assert abs(cost - r["objective"]) <= 1e-10 * cost


# ---- 4. the rows' duals ----------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,which", PAIRS)
def test_duals_follow_the_binding_side_and_are_complementary(hip_api, name, which):
    pp, kw = case(name), inputs(name, which)
    r = device_lp(hip_api, name, which)
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
    assert np.all(np.isfinite(e_max[yq < 0.0]))                        # (the lower end always exists: a positive dual on a row with
                                                                       # e_min = 0 belongs to a generator that stays off, sum_t P = 0)
    comp_q = complementarity(yq, r["P"].sum(axis=1), e_min, e_max, has)
    print(f"{name} {which}: ramp rows with a dual {int((yr != 0).sum())}, budget rows {int((yq != 0).sum())}, "
          f"complementarity {comp_r:.3e} / {comp_q:.3e} (bound {bound:.3e})")
    assert comp_r <= bound and comp_q <= bound
    if which != "rated" and (name, which) in TELLING:
        assert (yr != 0).any() or (yq != 0).any()                      # the set binds somewhere (it moves the optimum)


# ---- the raw entry -----------------------------------------------------------------------------------------------------------------
def raw(api, pp, *, rating=None, up=None, down=None, prev=None, e_min=None, e_max=None, avail=None, fill=0.0):
    """dopf_central_solve_coupled called as C would, every pointer as given (None = NULL), lossless storages from empty.
    avail: (profiles (K, T), profile_of (G,)). Returns (rc, message, result dict); the outputs start at `fill`."""
    kw = pp.engine_kwargs()
    keep = {k: np.ascontiguousarray(np.asarray(kw[k], dtype=np.int32 if k.endswith("_node") else np.float64).reshape(-1))
            for k in ("demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax", "sto_node")}
    prob = _capi.DopfProblem(N=pp.N, L=pp.L, T=pp.T, G=pp.G, S=pp.S)
    for k, v in keep.items():
        setattr(prob, k, v.ctypes.data_as(C.POINTER(C.c_int32 if v.dtype == np.int32 else C.c_double)))
    q, res = _capi.default_params(), _capi.DopfCentralResult()
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    f64 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    rating = None if rating is None else f64(np.asarray(rating, dtype=np.float64).reshape(pp.L, pp.T).T)
    up, down, prev, e_min, e_max = f64(up), f64(down), f64(prev), f64(e_min), f64(e_max)
    K, prof, of = 0, None, None
    if avail is not None:
        prof, of = f64(avail[0]), np.ascontiguousarray(np.asarray(avail[1], dtype=np.int32))
        K = prof.size // pp.T
    sizes = dict(P=pp.G * pp.T, D=pp.S * pp.T, C=pp.S * pp.T, E=pp.S * pp.T, system_price=pp.T, nodal_price=pp.N * pp.T,
                 line_utilization=pp.L * pp.T, flow_upper_dual=pp.L * pp.T, flow_lower_dual=pp.L * pp.T, ramp_dual=pp.G * pp.T,
                 budget_dual=pp.G)
    out = {k: np.full(n, fill) for k, n in sizes.items()}
    rc = api.central_solve_coupled(C.byref(prob), C.byref(q), None, None, None, None, None, K, dp(prof),
                                   None if of is None else of.ctypes.data_as(C.POINTER(C.c_int32)), dp(rating), dp(up), dp(down), dp(prev),
                                   dp(e_min), dp(e_max), TOL, MAX_ITERS, C.byref(res), *[dp(out[k]) for k in sizes])
    msg = api.last_error(None)
    out.update(objective=res.objective, dual_objective=res.dual_objective, iterations=res.iterations, converged=res.converged)
    return rc, (msg.decode() if msg else ""), out


# ---- 5. nothing given changes nothing ----------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", ["copper-T12", "net-6x9-T24"])
def test_without_the_new_inputs_it_is_central_solve(hip_api, name):
    """All six NULL: the _lossy body, the bits of central_solve. All six given at their defaults (kc_gen_rows without a row, kc_dual
    reading a table of f_max): another sweep, the same optimum."""
    pp = case(name)
    want = _capi.central_solve(hip_api, tol=TOL, max_iters=MAX_ITERS, **pp.engine_kwargs())
    rc, msg, null = raw(hip_api, pp)
    assert rc == 0, msg
    assert null["iterations"] == want["iterations"] and null["objective"] == want["objective"]
    assert null["dual_objective"] == want["dual_objective"]
    for k in OUT_KEYS:
        shape = want[k].shape
        have = null[k].reshape(shape[::-1]).T if len(shape) == 2 and k not in ("P", "D", "C", "E") else null[k].reshape(shape)
        assert np.array_equal(have, want[k]), k
    assert np.all(null["ramp_dual"] == 0.0) and np.all(null["budget_dual"] == 0.0)
    G = pp.G
    rating = np.asarray(pp.f_max)[:, None] * np.ones((pp.L, pp.T)) if pp.L else None
    rc, msg, dflt = raw(hip_api, pp, rating=rating, up=np.full(G, np.inf), down=np.full(G, np.inf), e_min=np.zeros(G), e_max=np.full(G, np.inf))
    assert rc == 0 and dflt["converged"], msg
    print(f"{name}: central_solve {want['objective']!r} ({want['iterations']} iterations), defaults {dflt['objective']!r} ({dflt['iterations']})")
    assert abs(dflt["objective"] - want["objective"]) <= 1e-5 * abs(want["objective"])
    assert np.all(dflt["ramp_dual"] == 0.0) and np.all(dflt["budget_dual"] == 0.0)


# ---- 6. refusals are the setters' --------------------------------------------------------------------------------------------------
REFUSALS = ("a NaN ramp", "p_prev above pmax", "an anchor that cannot come down", "e_min above the caps under availability",
            "a negative rating")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_are_the_setters(hip_api, what):
    pp = case("net-6x9-T24")
    G, T = pp.G, pp.T
    a = {}
    if what == "a NaN ramp":
        a["up"], a["down"] = np.full(G, 5.0), np.full(G, 5.0)
        a["down"][3] = np.nan
    elif what == "p_prev above pmax":
        a["prev"] = 0.5 * pp.gen_pmax
        a["prev"][G - 1] = 1.01 * pp.gen_pmax[G - 1] + 1.0
    elif what == "an anchor that cannot come down":
        # generator 2 starts at its capacity, comes down by a hundredth of it per step, and is unavailable from the second step on
        prof = np.ones((1, T))
        prof[0, 1:] = 0.0
        a["avail"] = (prof, np.where(np.arange(G) == 2, 0, -1))
        a["up"], a["down"] = np.full(G, np.inf), np.full(G, np.inf)
        a["down"][2] = 0.01 * pp.gen_pmax[2]
        a["prev"] = np.zeros(G)
        a["prev"][2] = pp.gen_pmax[2]
    elif what == "e_min above the caps under availability":
        # a minimum that fits under T pmax but not under the half-available profile of the same call
        prof = np.full((1, T), 0.5)
        a["avail"] = (prof, np.where(np.arange(G) == 4, 0, -1))
        a["e_min"] = np.zeros(G)
        a["e_min"][4] = 0.75 * T * pp.gen_pmax[4]
        rc, msg, out = raw(hip_api, pp, e_min=0.1 * a["e_min"], avail=a["avail"])
        assert rc == 0 and out["converged"], (rc, msg)                  # ... a tenth of it does: the entry takes that
    else:
        a["rating"] = np.asarray(pp.f_max)[:, None] * np.ones((pp.L, T))
        a["rating"][4, 7] = -1.0
    rc, msg, out = raw(hip_api, pp, fill=np.nan, **a)
    assert rc == INVALID, (rc, msg)
    assert "dopf_central_solve_coupled" in msg, msg
    for k in OUT_KEYS + ("ramp_dual", "budget_dual"):
        assert np.all(np.isnan(out[k])), k
    assert out["iterations"] == 0 and out["converged"] == 0


# ---- 7. a decentral run lands on the device optimum ------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_decentral_run_with_budgets_lands_on_the_device_optimum(hip_api):
    """The case of test_gpu_central_lossy.py's landing with budgets from the drawing rule: the ADMM cost within 1e-3 of
    dopf_central_solve_coupled's objective, which is within 1e-5 of HiGHS."""
    pp = synth.synthetic_case(n_gen=12, n_sto=4, T=24, seed=892)
    pp.sto_pmax, pp.sto_emax = pp.sto_pmax * 8.0, pp.sto_emax * 8.0
    budget = draw_inputs(pp, _host)["budget"]
    r = _capi.central_solve_coupled(hip_api, tol=TOL, max_iters=MAX_ITERS, gen_budget=budget, **pp.engine_kwargs())
    assert r["converged"]
    lp, base = _host(pp, gen_budget=budget).objective, _host(pp).objective
    print(f"device {r['objective']!r} host {lp!r} (without budgets {base!r}) iterations {r['iterations']}")
    assert abs(lp - base) > 1e-3 * abs(base)
    assert abs(r["objective"] - lp) <= 1e-5 * abs(lp)
    e = _capi.Engine(hip_api, params=_capi.default_params(gamma=1.0 / (pp.G + pp.S), max_iters=20000), gen_budget=budget, **pp.engine_kwargs())
    done, conv = e.iterate(20000)
    assert conv, done
    cost = e.get_consensus()[4]
    print(f"decentral cost {cost!r} after {done} iterations")
    assert abs(cost - r["objective"]) / r["objective"] <= 1e-3, (cost, r["objective"], done)
