"""dopf_central_solve_lossy: the device LP with storage charge / discharge efficiencies (csrc/kernels_central.hip, kc_sto<., 3>; DESIGN.md
5n). The reference for every number is the host LP (central.solve_central_packed(..., efficiency=...), HiGHS) with the same inputs,
never the device solver itself. The cases are those of test_gpu_central_features.py (the smallest shapes at which kc_sto can go wrong)."""
import ctypes as C
import functools

import numpy as np
import pytest

from decentralopf_jl_amd import _capi, synth
from decentralopf_jl_amd.central import central_reference, central_reference_on_device, solve_central_packed
from helpers import draw_band, draw_e0, reachable
from helpers_efficiency import draw_band_eff, draw_eta, levels_eff

pytestmark = pytest.mark.gpu

INVALID = -1                    # DOPF_E_INVALID
TOL = 1e-7
CASES = {
    "copper-T12": lambda: synth.synthetic_case(40, 6, 12, seed=3),
    "copper-T70": lambda: synth.synthetic_case(60, 9, 70, seed=5),      # two timesteps per lane, a partly filled wave: the band's slot
                                                                        # is k = 1 of lane 34, not the wave's last lane
    "copper-T1": lambda: synth.synthetic_case(20, 5, 1, seed=9),        # first step = last step: e0 and the band meet in one row
    "copper-T65": lambda: synth.synthetic_case(60, 9, 65, seed=5),      # the band's slot is k = 0 of lane 32, whose second slot is empty
    "net-6x9-T24": lambda: synth.synthetic_case(60, 15, 24, N=6, L=9, seed=7, fmax_factor=1.0, fmax_min=5),      # line limits bind
}
SETS = ("eta", "all")
TELLING = ("copper-T70", "copper-T65", "net-6x9-T24")      # (on copper-T12 / copper-T1 the storages stay idle from the empty start under
                                                            # "eta": the lossy and the lossless optimum coincide)
OUT_KEYS = ("P", "D", "C", "E", "system_price", "nodal_price", "line_utilization", "flow_upper_dual", "flow_lower_dual")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def inputs(name, which):
    """((eta_c, eta_d), e0 | None, (lo, hi) | None) of one set. "all": an equality target inside the levels reachable under the
    efficiencies for every odd-indexed storage, [0, emax] for the even-indexed ones."""
    pp = case(name)
    rng = np.random.default_rng(11)
    ec, ed = draw_eta(pp.S, rng)
    if which == "eta":
        return (ec, ed), None, None
    e0 = draw_e0(pp, "mix", rng)
    lo, hi = draw_band_eff(pp, e0, ec, ed, "eq", rng)
    lo, hi = lo.copy(), hi.copy()
    lo[::2], hi[::2] = 0.0, pp.sto_emax[::2]
    return (ec, ed), e0, (lo, hi)


def feature_kwargs(eta, e0, band):
    kw = {}
    if eta is not None:
        kw["sto_eta"] = eta
    if e0 is not None:
        kw["sto_e0"] = e0
    if band is not None:
        kw["sto_end_lo"], kw["sto_end_hi"] = band
    return kw


@functools.lru_cache(maxsize=None)
def host_lp(name, which):
    eta, e0, band = inputs(name, which)
    return solve_central_packed(case(name), duals=False, initial_level=e0, terminal_level=band, efficiency=eta).objective


@functools.lru_cache(maxsize=None)
def host_lp_lossless(name):
    return solve_central_packed(case(name), duals=False).objective


_device = {}


def device_lp(api, name, which):
    """One device solve per (case, set), shared by the tests that look at it."""
    if (name, which) not in _device:
        _device[name, which] = _capi.central_solve(api, tol=TOL, **case(name).engine_kwargs(), **feature_kwargs(*inputs(name, which)))
    return _device[name, which]


# ---- 1. the objective ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name", list(CASES))
def test_objective_matches_the_host_lp_with_the_same_inputs(hip_api, name, which):
    pp, want = case(name), host_lp(name, which)
    r = device_lp(hip_api, name, which)
    print(f"{name} {which}: host {want!r} device {r['objective']!r} dual {r['dual_objective']!r} "
          f"pinf {r['primal_infeasibility']:.3e} iterations {r['iterations']}")
    assert r["converged"], {k: r[k] for k in ("objective", "dual_objective", "primal_infeasibility", "gap", "iterations")}
    assert abs(r["objective"] - want) <= 1e-5 * abs(want)
    assert abs(r["dual_objective"] - want) <= 1e-5 * abs(want)
    assert r["primal_infeasibility"] <= 1e-5 * (1.0 + np.abs(pp.demand).max())


# ---- 2. the test can tell lossy from lossless ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TELLING)
def test_device_objective_lies_on_the_lossy_side(hip_api, name):
    lossy, lossless = host_lp(name, "eta"), host_lp_lossless(name)
    print(f"{name}: host lossy {lossy!r} lossless {lossless!r} relative difference {(lossy - lossless) / lossless:.3e}")
    assert abs(lossy - lossless) > 1e-4 * abs(lossless)                # ten times the bound below
    r = device_lp(hip_api, name, "eta")
    assert abs(r["objective"] - lossy) <= 1e-5 * abs(lossy)
    assert abs(r["objective"] - lossless) > 1e-5 * abs(lossless)


# ---- 3. the returned point in its own right --------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name", list(CASES))
def test_returned_point_is_feasible_in_its_own_right(hip_api, name, which):
    pp = case(name)
    (ec, ed), e0, band = inputs(name, which)
    r = device_lp(hip_api, name, which)
    assert r["P"].min() >= 0 and (r["P"] - pp.gen_pmax[:, None]).max() <= 0
    assert r["D"].min() >= 0 and r["C"].min() >= 0 and (r["D"] - pp.sto_pmax[:, None]).max() <= 0 and (r["C"] - pp.sto_pmax[:, None]).max() <= 0
    start = np.zeros(pp.S) if e0 is None else e0
    E = r["E"]
    assert np.abs(levels_eff(start, ec, ed, r["D"], r["C"]) - E).max() < 1e-9 * (1 + np.abs(E).max())
    slack = r["primal_infeasibility"] + 1e-9 * (1 + np.abs(E).max())
    assert E.min() >= -slack and (E - pp.sto_emax[:, None]).max() <= slack
    lo, hi = (np.zeros(pp.S), pp.sto_emax) if band is None else band
    assert (lo - E[:, -1]).max() <= slack and (E[:, -1] - hi).max() <= slack
    cost = float(pp.gen_mc @ r["P"].sum(axis=1) + pp.sto_mc @ (r["D"] + r["C"]).sum(axis=1))
    assert abs(cost - r["objective"]) <= 1e-10 * cost


# ---- the raw entry: what the Python host does not let through --------------------------------------------------------------------
def raw(api, pp, e0=None, lo=None, hi=None, eta_c=None, eta_d=None, *, ex=False, fill=0.0):
    """dopf_central_solve_lossy called as C would (ex: dopf_central_solve_ex, which has no efficiency arguments), every pointer as
    given (None = NULL), no availability. Returns (rc, message, result dict); the outputs start at `fill`."""
    kw = pp.engine_kwargs()
    keep = {k: np.ascontiguousarray(np.asarray(kw[k], dtype=np.int32 if k.endswith("_node") else np.float64).reshape(-1))
            for k in ("demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax", "sto_node")}
    prob = _capi.DopfProblem(N=pp.N, L=pp.L, T=pp.T, G=pp.G, S=pp.S)
    for k, v in keep.items():
        setattr(prob, k, v.ctypes.data_as(C.POINTER(C.c_int32 if v.dtype == np.int32 else C.c_double)))
    q, res = _capi.default_params(), _capi.DopfCentralResult()
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    f64 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    e0, lo, hi, eta_c, eta_d = f64(e0), f64(lo), f64(hi), f64(eta_c), f64(eta_d)
    sizes = dict(P=pp.G * pp.T, D=pp.S * pp.T, C=pp.S * pp.T, E=pp.S * pp.T, system_price=pp.T, nodal_price=pp.N * pp.T,
                 line_utilization=pp.L * pp.T, flow_upper_dual=pp.L * pp.T, flow_lower_dual=pp.L * pp.T)
    out = {k: np.full(n, fill) for k, n in sizes.items()}
    outs = [dp(out[k]) for k in sizes]
    if ex:
        assert eta_c is None and eta_d is None
        rc = api.central_solve_ex(C.byref(prob), C.byref(q), dp(e0), dp(lo), dp(hi), 0, None, None, TOL, 200000, C.byref(res), *outs)
    else:
        rc = api.central_solve_lossy(C.byref(prob), C.byref(q), dp(e0), dp(lo), dp(hi), dp(eta_c), dp(eta_d), 0, None, None, TOL, 200000,
                                     C.byref(res), *outs)
    msg = api.last_error(None)
    out.update(objective=res.objective, dual_objective=res.dual_objective, iterations=res.iterations, converged=res.converged)
    return rc, (msg.decode() if msg else ""), out


# ---- 4. all ones change nothing --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["copper-T12", "net-6x9-T24"])
def test_unit_efficiencies_change_nothing(hip_api, name):
    """_ex with an initial level and a band, _lossy with the same and both arrays NULL, _lossy with both arrays all 1 (kc_sto<., 3>
    instead of kc_sto<., 2>): the same iterations and the same bits — every new operation multiplies by exactly 1.0 or adds 1 + 1,
    and a fused multiply-add with a factor of 1 rounds once, like the addition it replaces."""
    pp = case(name)
    rng = np.random.default_rng(7)
    e0 = draw_e0(pp, "mix", rng)
    lo, hi = draw_band(pp, e0, "mix", rng)
    rc0, _, ex = raw(hip_api, pp, e0, lo, hi, ex=True)
    rc1, _, null = raw(hip_api, pp, e0, lo, hi)
    rc2, _, ones = raw(hip_api, pp, e0, lo, hi, np.ones(pp.S), np.ones(pp.S))
    assert rc0 == rc1 == rc2 == 0
    assert ex["converged"] and ex["iterations"] > 0
    for other in (null, ones):
        assert other["iterations"] == ex["iterations"] and other["objective"] == ex["objective"]
        assert other["dual_objective"] == ex["dual_objective"]
        for k in OUT_KEYS:
            assert np.array_equal(other[k], ex[k]), k


# ---- 5. refusals are the setters' ------------------------------------------------------------------------------------------------
REFUSALS = ("eta_c of 0", "eta_d of 0", "eta_c of 1.1", "eta_d of 1.1", "a NaN", "only eta_c", "only eta_d",
            "band unreachable under eta_c")


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_are_the_setters(hip_api, what):
    pp = case("copper-T12")
    S = pp.S
    a = dict(e0=None, lo=None, hi=None, eta_c=np.ones(S), eta_d=np.ones(S))
    if what == "eta_c of 0":
        a["eta_c"][3] = 0.0
    elif what == "eta_d of 0":
        a["eta_d"][3] = 0.0
    elif what == "eta_c of 1.1":
        a["eta_c"][0] = 1.1
    elif what == "eta_d of 1.1":
        a["eta_d"][S - 1] = 1.1
    elif what == "a NaN":
        a["eta_d"][2] = np.nan
    elif what == "only eta_c":
        a["eta_d"] = None
    elif what == "only eta_d":
        a["eta_c"] = None
    else:
        # a target that a lossless storage reaches from empty and one with eta_c = 0.6 does not: 0.9 min(emax, T pmax) > 0.6 T pmax
        pp = case("copper-T1")
        S, span = pp.S, pp.T * pp.sto_pmax
        target = 0.9 * np.minimum(pp.sto_emax, span)
        s = int(np.flatnonzero((target > 0.6 * span * (1 + 1e-9)) & (span > 0.0))[0])
        e0, lo, hi = np.zeros(S), np.zeros(S), pp.sto_emax.copy()
        lo[s] = hi[s] = target[s]
        rlo, rhi = reachable(pp, e0)
        assert rlo[s] <= target[s] <= rhi[s]                            # reachable losslessly ...
        rc, msg, out = raw(hip_api, pp, e0, lo, hi, ex=True)
        assert rc == 0 and out["converged"], (rc, msg)                  # ... so the lossless entry takes it
        a = dict(e0=e0, lo=lo, hi=hi, eta_c=np.where(np.arange(S) == s, 0.6, 1.0), eta_d=np.ones(S))
    rc, msg, out = raw(hip_api, pp, a["e0"], a["lo"], a["hi"], a["eta_c"], a["eta_d"], fill=np.nan)
    assert rc == INVALID, (rc, msg)
    assert "dopf_central_solve_lossy" in msg, msg
    for k in OUT_KEYS:
        assert np.all(np.isnan(out[k])), k
    assert out["iterations"] == 0 and out["converged"] == 0
    # ... and the Python host hands the same message on (it always passes both arrays)
    if a["eta_c"] is not None and a["eta_d"] is not None:
        with pytest.raises(_capi.DopfError, match="dopf_central_solve_lossy"):
            kw = feature_kwargs((a["eta_c"], a["eta_d"]), a["e0"], None if a["lo"] is None else (a["lo"], a["hi"]))
            _capi.central_solve(hip_api, tol=TOL, **pp.engine_kwargs(), **kw)


# ---- 6. a decentral run lands on the device optimum ------------------------------------------------------------------------------
def test_decentral_run_with_lossy_storages_lands_on_the_device_optimum(hip_api):
    """The case of test_gpu_sto_efficiency.test_copper_plate_with_lossy_storages_reaches_the_lp, with the device LP as the target:
    the ADMM cost within that test's 1e-3 of dopf_central_solve_lossy's objective, which is within 1e-5 of HiGHS."""
    pp = synth.synthetic_case(n_gen=12, n_sto=4, T=24, seed=892)
    pp.sto_pmax, pp.sto_emax = pp.sto_pmax * 8.0, pp.sto_emax * 8.0
    eta = (np.full(4, 0.9), np.full(4, 0.9))
    r = _capi.central_solve(hip_api, tol=TOL, sto_eta=eta, **pp.engine_kwargs())
    assert r["converged"]
    lp = solve_central_packed(pp, duals=False, efficiency=eta).objective
    print(f"device {r['objective']!r} host {lp!r} iterations {r['iterations']}")
    assert abs(r["objective"] - lp) <= 1e-5 * abs(lp)
    e = _capi.Engine(hip_api, params=_capi.default_params(gamma=1.0 / (pp.G + pp.S), max_iters=20000), sto_eta=eta, **pp.engine_kwargs())
    done, conv = e.iterate(20000)
    assert conv, done
    cost = e.get_consensus()[4]
    assert abs(cost - r["objective"]) / r["objective"] <= 1e-3, (cost, r["objective"], done)


# ---- 7. central_reference_on_device(..., lossy=True) -----------------------------------------------------------------------------
def test_central_reference_on_device_takes_the_storages_efficiencies():
    from conftest import pkg
    nodes, lines, gens, stos = pkg.three_node_case()
    stos[0].charge_efficiency, stos[0].discharge_efficiency = 0.9, 0.9
    host = central_reference(nodes, gens, stos, lines)
    r = central_reference_on_device(nodes, gens, stos, lines, lossy=True)
    print(f"device {r.objective!r} host {host.objective!r}")
    assert abs(r.objective - host.objective) <= 1e-6 * abs(host.objective)
    assert np.abs(r.level - levels_eff(np.zeros(1), np.full(1, 0.9), np.full(1, 0.9), r.discharge, r.charge)).max() <= 1e-9
    # ... and the keyword overrides the storages' own, as in central_reference
    eta = (np.full(1, 0.8), np.full(1, 1.0))
    host = central_reference(nodes, gens, stos, lines, efficiency=eta)
    r = central_reference_on_device(nodes, gens, stos, lines, efficiency=eta, lossy=True)
    assert abs(r.objective - host.objective) <= 1e-6 * abs(host.objective)
