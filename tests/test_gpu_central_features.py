"""dopf_central_solve_ex: the device LP with storage initial levels, terminal bands and generator availability (csrc/kernels_central.hip,
kc_gen<., AV> and kc_sto<., LV>). The reference for every number is the host LP (central.solve_central_packed, HiGHS) with the same
inputs, never the device solver itself."""
import ctypes as C
import functools

import numpy as np
import pytest

from decentralopf_jl_amd import _capi, synth
from decentralopf_jl_amd.central import central_reference_on_device, solve_central_packed
from helpers import draw_band, draw_e0, engine

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
SETS = ("e0", "band", "avail", "all")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def inputs(name, which):
    """(e0 | None, (lo, hi) | None, (profiles, profile_of) | None) of one feature set."""
    pp = case(name)
    rng = np.random.default_rng(7)
    e0 = draw_e0(pp, "mix", rng)
    band = draw_band(pp, e0, "mix", rng)
    if which == "band":
        band = draw_band(pp, np.zeros(pp.S), "mix", np.random.default_rng(7))
    prof = synth.availability_profiles(pp.T, seed=8)
    of = np.full(pp.G, -1, dtype=np.int32)
    of[::4] = np.arange(pp.G)[::4] % 3
    return (e0 if which in ("e0", "all") else None, band if which in ("band", "all") else None,
            (prof, of) if which in ("avail", "all") else None)


def feature_kwargs(e0, band, avail):
    kw = {}
    if e0 is not None:
        kw["sto_e0"] = e0
    if band is not None:
        kw["sto_end_lo"], kw["sto_end_hi"] = band
    if avail is not None:
        kw["gen_avail"], kw["gen_avail_of"] = avail
    return kw


@functools.lru_cache(maxsize=None)
def host_lp(name, which):
    e0, band, avail = inputs(name, which)
    return solve_central_packed(case(name), duals=False, initial_level=e0, terminal_level=band, availability=avail).objective


_device = {}


def device_lp(api, name, which):
    """One device solve per (case, feature set), shared by the tests that look at it."""
    if (name, which) not in _device:
        _device[name, which] = _capi.central_solve(api, tol=TOL, **case(name).engine_kwargs(), **feature_kwargs(*inputs(name, which)))
    return _device[name, which]


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


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name", list(CASES))
def test_returned_point_is_feasible_in_its_own_right(hip_api, name, which):
    pp = case(name)
    e0, band, avail = inputs(name, which)
    r = device_lp(hip_api, name, which)
    cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
    if avail is not None:
        prof, of = avail
        cap = np.where((of >= 0)[:, None], pp.gen_pmax[:, None] * prof[np.maximum(of, 0)], cap)      # one multiply, as the kernels
    assert r["P"].min() >= 0 and (r["P"] - cap).max() <= 0
    assert r["D"].min() >= 0 and r["C"].min() >= 0 and (r["D"] - pp.sto_pmax[:, None]).max() <= 0 and (r["C"] - pp.sto_pmax[:, None]).max() <= 0
    start = np.zeros(pp.S) if e0 is None else e0
    E = r["E"]
    assert np.abs(start[:, None] + np.cumsum(r["C"] - r["D"], axis=1) - E).max() < 1e-9 * (1 + np.abs(E).max())
    slack = r["primal_infeasibility"] + 1e-9 * (1 + np.abs(E).max())
    assert E.min() >= -slack and (E - pp.sto_emax[:, None]).max() <= slack
    lo, hi = (np.zeros(pp.S), pp.sto_emax) if band is None else band
    assert (lo - E[:, -1]).max() <= slack and (E[:, -1] - hi).max() <= slack
    cost = float(pp.gen_mc @ r["P"].sum(axis=1) + pp.sto_mc @ (r["D"] + r["C"]).sum(axis=1))
    assert abs(cost - r["objective"]) <= 1e-10 * cost


# ---- the raw entry: what the Python host does not let through -------------------------------------------------------------

def raw_ex(api, pp, e0=None, lo=None, hi=None, K=0, prof=None, of=None, *, plain=False, fill=0.0):
    """dopf_central_solve_ex called as C would (plain: dopf_central_solve), every pointer as given (None = NULL). Returns
    (rc, message, result dict); the outputs start at `fill`."""
    kw = pp.engine_kwargs()
    keep = {k: np.ascontiguousarray(np.asarray(kw[k], dtype=np.int32 if k.endswith("_node") else np.float64).reshape(-1))
            for k in ("demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax", "sto_node")}
    prob = _capi.DopfProblem(N=pp.N, L=pp.L, T=pp.T, G=pp.G, S=pp.S)
    for k, v in keep.items():
        setattr(prob, k, v.ctypes.data_as(C.POINTER(C.c_int32 if v.dtype == np.int32 else C.c_double)))
    q, res = _capi.default_params(), _capi.DopfCentralResult()
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    f64 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    e0, lo, hi, prof = f64(e0), f64(lo), f64(hi), f64(prof)
    of = None if of is None else np.ascontiguousarray(np.asarray(of, dtype=np.int32))
    sizes = dict(P=pp.G * pp.T, D=pp.S * pp.T, C=pp.S * pp.T, E=pp.S * pp.T, system_price=pp.T, nodal_price=pp.N * pp.T,
                 line_utilization=pp.L * pp.T, flow_upper_dual=pp.L * pp.T, flow_lower_dual=pp.L * pp.T)
    out = {k: np.full(n, fill) for k, n in sizes.items()}
    outs = [dp(out[k]) for k in sizes]
    if plain:
        rc = api.central_solve(C.byref(prob), C.byref(q), TOL, 200000, C.byref(res), *outs)
    else:
        rc = api.central_solve_ex(C.byref(prob), C.byref(q), dp(e0), dp(lo), dp(hi), int(K), dp(prof),
                                  None if of is None else of.ctypes.data_as(C.POINTER(C.c_int32)), TOL, 200000, C.byref(res), *outs)
    msg = api.last_error(None)
    out.update(objective=res.objective, dual_objective=res.dual_objective, iterations=res.iterations, converged=res.converged)
    return rc, (msg.decode() if msg else ""), out


@pytest.mark.parametrize("name", ["copper-T12", "net-6x9-T24"])
def test_defaults_change_nothing(hip_api, name):
    """dopf_central_solve, _ex with every input NULL, _ex with the defaults spelled out: the same iterations and the same bits (the
    default inputs add exact zeros and multiply by exact ones)."""
    pp = case(name)
    rc0, _, plain = raw_ex(hip_api, pp, plain=True)
    rc1, _, null = raw_ex(hip_api, pp)
    ones = np.ones((2, pp.T))
    of = np.full(pp.G, -1, dtype=np.int32)
    of[::2] = np.arange(pp.G)[::2] % 2                  # half on an all-ones profile, half on -1
    rc2, _, dflt = raw_ex(hip_api, pp, np.zeros(pp.S), np.zeros(pp.S), pp.sto_emax.copy(), 2, ones, of)
    assert rc0 == rc1 == rc2 == 0
    assert plain["converged"] and plain["iterations"] > 0
    for other in (null, dflt):
        assert other["iterations"] == plain["iterations"] and other["objective"] == plain["objective"]
        assert other["dual_objective"] == plain["dual_objective"]
        for k in ("P", "D", "C", "E", "system_price", "line_utilization"):
            assert np.array_equal(other[k], plain[k]), k


REFUSALS = ("e0 above max_level", "lo > hi", "only lo", "only hi", "band unreachable from e0", "profile value 1.5",
            "index >= n_profiles", "n_profiles > 0 with a NULL table")


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_are_the_setters(hip_api, what):
    pp = case("copper-T12")
    S, G, T, em = pp.S, pp.G, pp.T, pp.sto_emax
    assert np.all(T * pp.sto_pmax > 0.0)
    a = dict(e0=None, lo=None, hi=None, K=0, prof=None, of=None)
    if what == "e0 above max_level":
        a["e0"] = np.where(np.arange(S) == 2, 1.5 * em, 0.0)
    elif what == "lo > hi":
        a["lo"], a["hi"] = np.where(np.arange(S) == 1, 0.75 * em, 0.0), np.where(np.arange(S) == 1, 0.25 * em, em)
    elif what == "only lo":
        a["lo"] = np.zeros(S)
    elif what == "only hi":
        a["hi"] = em.copy()
    elif what == "band unreachable from e0":
        pp = case("copper-T1")                      # one step of at most pmax < emax: from full down to empty is out of reach
        S, em = pp.S, pp.sto_emax
        assert np.all(pp.sto_pmax < em)
        a["e0"], a["lo"], a["hi"] = em.copy(), np.zeros(S), np.zeros(S)
    elif what == "profile value 1.5":
        prof = np.ones((2, T))
        prof[1, 3] = 1.5
        a.update(K=2, prof=prof, of=np.zeros(G, dtype=np.int32))
    elif what == "index >= n_profiles":
        of = np.zeros(G, dtype=np.int32)
        of[5] = 2
        a.update(K=2, prof=np.ones((2, T)), of=of)
    else:
        a.update(K=2, prof=None, of=np.zeros(G, dtype=np.int32))
    rc, msg, out = raw_ex(hip_api, pp, a["e0"], a["lo"], a["hi"], a["K"], a["prof"], a["of"], fill=np.nan)
    assert rc == INVALID, (rc, msg)
    assert "dopf_central_solve_ex" in msg, msg
    for k in ("P", "D", "C", "E", "system_price", "nodal_price", "line_utilization", "flow_upper_dual", "flow_lower_dual"):
        assert np.all(np.isnan(out[k])), k
    assert out["iterations"] == 0 and out["converged"] == 0
    # ... and the Python host hands the same message on
    with pytest.raises(_capi.DopfError, match="dopf_central_solve_ex"):
        kw = feature_kwargs(a["e0"], None if a["lo"] is None and a["hi"] is None else (a["lo"], a["hi"]),
                            None if a["K"] == 0 else (a["prof"], a["of"]))
        _capi.central_solve(hip_api, tol=TOL, **pp.engine_kwargs(), **kw)


def test_decentral_run_lands_on_the_device_optimum_with_every_feature(hip_api):
    """The parity target without any host LP: ADMM with all three flags against dopf_central_solve_ex (the inputs of
    test_oracle_features.test_exact_oracle_reaches_the_lp_with_every_feature, where the CPU oracle meets the same bound)."""
    pp = synth.synthetic_case(100, 12, 24, seed=441)
    rng = np.random.default_rng(7)
    e0 = draw_e0(pp, "mix", rng)
    lo, hi = draw_band(pp, e0, "mix", rng)
    prof = synth.availability_profiles(pp.T, seed=8)
    of = np.full(pp.G, -1, dtype=np.int32)
    of[::10] = np.arange(pp.G)[::10] % 3
    r = _capi.central_solve(hip_api, tol=TOL, **pp.engine_kwargs(), **feature_kwargs(e0, (lo, hi), (prof, of)))
    assert r["converged"]
    flags = _capi.F_STO_INITIAL_LEVEL | _capi.F_STO_TERMINAL_LEVEL | _capi.F_GEN_AVAILABILITY
    e = engine(hip_api, pp, None, flags=flags, gamma=1.0 / (pp.G + pp.S), max_iters=6000)
    e.set_initial_levels(e0)
    e.set_terminal_levels(lo, hi)
    e.set_availability(prof, of)
    done, conv = e.iterate(6000)
    assert conv, done
    cost = e.get_consensus()[4]
    assert abs(cost - r["objective"]) / r["objective"] < 1e-3, (cost, r["objective"], done)


def test_central_reference_on_device_takes_the_elements_inputs():
    """The three-node case with the PV profile [1, 0.875] (LP 14825): the packed case's engine_kwargs() carry the
    profile, which the device entry used to refuse."""
    from conftest import pkg
    nodes, lines, gens, stos = pkg.three_node_case()
    gens[0].availability = [1.0, 0.875]
    host = solve_central_packed(pkg.pack(nodes, gens, stos, lines))
    assert abs(host.objective - 14825.0) <= 1e-6 * host.objective
    r = central_reference_on_device(nodes, gens, stos, lines)
    assert abs(r.objective - host.objective) < 1e-4
    assert np.abs(r.generation - host.generation).max() < 1e-4
    # ... and the keyword overrides, as central_reference has them
    e0, band = np.array([5.0]), (np.array([5.0]), np.array([20.0]))
    host = solve_central_packed(pkg.pack(nodes, gens, stos, lines), initial_level=e0, terminal_level=band)
    r = central_reference_on_device(nodes, gens, stos, lines, initial_level=e0, terminal_level=band)
    assert abs(r.objective - host.objective) < 1e-4
    assert r.level[0, -1] >= 5.0 - 1e-6
