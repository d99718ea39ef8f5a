"""dopf_set_generator_min_output without a GPU: the header's three prototypes and what its text promises, the
bindings, the Julia shim, the fourth extension table (the three older ones as they were), the host route of the floors
(Generator.min_generation -> pack -> engine_kwargs -> shard), the refusals of the device LP, the host LP's lower bounds on the
three-node case, and the two NumPy twins the GPU tests stand on — against an independent dense QP and, at a zero floor, against the
helpers they were written from, bit for bit."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT, pkg
from decentralopf_jl_amd import _capi, admm, central, sharded
from helpers_min_output import (floor_cases, floor_kkt_violation, path_exists, pwl_floor_cases, qp_row, ramp_project_floor,
                                ramp_project_pwl_floor)
from helpers_ramp import ramp_project
from helpers_ramp_net import line_step, phi_at, pwl_cases, ramp_project_pwl

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
ENTRY = ("dopf_set_generator_min_output", "dopf_multi_set_generator_min_output")
BASE_KEYS = {"N", "L", "T", "demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax",
             "sto_node"}
DP = ctypes.POINTER(ctypes.c_double)


# ---- the header ------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_three_entries():
    assert re.search(r"^int dopf_set_generator_min_output\(dopf_ctx \*ctx, const double \*p_min /\* G; NULL = all 0 \*/\);$", HDR, re.M)
    assert re.search(r"^int dopf_get_generator_min_output\(dopf_ctx \*ctx, double \*p_min /\* G \*/\);", HDR, re.M)
    assert re.search(r"^int dopf_multi_set_generator_min_output\(dopf_multi \*m, const double \*p_min\);$", HDR, re.M)


def test_header_text_states_the_rule_the_flag_the_refusals_and_the_recapture():
    at = HDR.index("int dopf_set_generator_min_output(")
    text = " ".join(HDR[HDR.rindex("/*", 0, at):at].replace(" * ", " ").split())
    for phrase in ("floor[g,t] = fmin(p_min[g], cap[g,t])", "floor[g,t] <= P[g,t] <= cap[g,t]", "DOPF_F_GEN_RAMP", "DOPF_F_GEN_RAMP_NETWORK",
                   "DOPF_F2_GEN_ENERGY_BUDGET", "DOPF_F2_GEN_RAMP_BUDGET", "captured again at the next dopf_iterate",
                   "does NOT check that the floors", "does not converge", "dopf_roll_horizon_coupled leaves p_min alone",
                   "dopf_central_solve* ignore it", "F_t = [max(floor_t, lo_{t-1} - ramp_down), min(cap_t, hi_{t-1} + ramp_up)]",
                   "With G == 0 the call returns DOPF_OK"):
        assert phrase in text, phrase


def test_header_adds_no_flag_to_either_word():
    assert dict(re.findall(r"#define\s+(DOPF_F2_\w+)\s+(\d+)", HDR)) == {"DOPF_F2_GEN_ENERGY_BUDGET": "1", "DOPF_F2_GEN_RAMP_BUDGET": "8"}
    assert not re.search(r"#define\s+DOPF_F\w*(MIN_OUT|FLOOR|MUST_RUN)", HDR)


# ---- the bindings ----------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_entries_and_the_argtypes_match():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for name in ("set_generator_min_output", "multi_set_generator_min_output", "get_generator_min_output"):
        f = getattr(api, name)
        assert f.restype is ctypes.c_int and list(f.argtypes) == [ctypes.c_void_p, DP], name


def test_julia_shim_has_the_setter_and_the_ccalls():
    assert re.search(r"^function set_min_output!\(admm::ADMM, p_min::Union\{Nothing, Vector\{Float64\}\}\)", JL, re.M)
    for name in ENTRY + ("dopf_get_generator_min_output",):
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cdouble\}\)" % name, JL), name
    doc = JL[JL.index("    set_min_output!(admm, p_min)"):JL.index("function set_min_output!")]
    assert "DOPF_F_GEN_RAMP" in doc and "DOPF_F2_GEN_ENERGY_BUDGET" in doc


def test_the_fourth_table_and_the_four_hosts_setters():
    assert [x.setter for x in _capi.EXTENSIONS_FLOOR] == ["set_min_output"]
    x = _capi.EXTENSIONS_FLOOR[0]
    assert (x.flag, x.word, x.entry, x.keys, x.optional) == (_capi.F_GEN_RAMP, 1, "set_generator_min_output", ("gen_min_output",), True)
    assert tuple(x.argtypes) == (DP,)
    assert _capi._ALL_EXTENSIONS == _capi.EXTENSIONS + _capi.EXTENSIONS_MORE + _capi.EXTENSIONS_WORD2 + _capi.EXTENSIONS_FLOOR
    assert list(_capi._BY_SETTER)[-1] == "set_min_output" and _capi._BY_SETTER["set_min_output"] is x
    order = list(_capi._BY_SETTER)
    assert order.index("set_min_output") > order.index("set_ramp") > order.index("set_availability")      # its check reads both
    for cls in (_capi.Engine, _capi.MultiEngine, admm.ADMM, sharded.ShardedADMM):
        assert callable(getattr(cls, "set_min_output")), cls


def test_the_three_older_tables_are_what_they_were():
    assert [x.setter for x in _capi.EXTENSIONS] == ["set_efficiency", "set_initial_levels", "set_terminal_levels", "set_availability",
                                                    "set_line_rating", "set_quadratic_cost"]
    assert [x.setter for x in _capi.EXTENSIONS_MORE] == ["set_ramp"] and [x.setter for x in _capi.EXTENSIONS_WORD2] == ["set_energy_budget"]
    assert [(x.flag, x.word) for x in _capi.EXTENSIONS_MORE + _capi.EXTENSIONS_WORD2] == [(_capi.F_GEN_RAMP, 1), (_capi.F2_GEN_ENERGY_BUDGET, 2)]


def _extensions(L, **kw):
    api = types.SimpleNamespace(prefix="dopf_", set_generator_min_output=object(), set_generator_ramp=object())
    d = types.SimpleNamespace(N=2, L=L, T=3, G=4, S=0)
    params, todo = _capi._extensions(api, None, d, {}, kw)
    return (0 if params is None else params.flags & 0xFFFFFFFF), [x.setter for x, _ in todo], todo


def test_a_floor_alone_asks_for_the_ramp_flag_and_a_default_floor_for_nothing():
    floor = np.array([0.0, 5.0, 0.0, 1.0])
    flags, setters, todo = _extensions(0, gen_min_output=floor)
    assert flags == _capi.F_GEN_RAMP and setters == ["set_min_output"] and np.array_equal(todo[0][1][0], floor)
    flags, setters, _ = _extensions(2, gen_min_output=floor)
    assert flags == _capi.F_GEN_RAMP | _capi.F_GEN_RAMP_NETWORK and setters == ["set_min_output"]
    for L in (0, 2):
        assert _extensions(L, gen_min_output=np.zeros(4))[:2] == (0, [])
        assert _extensions(L, gen_min_output=None)[:2] == (0, [])
    flags, setters, _ = _extensions(0, gen_min_output=floor, gen_ramp=(np.full(4, 3.0), np.full(4, 3.0)))
    assert flags == _capi.F_GEN_RAMP and setters == ["set_ramp", "set_min_output"]          # behind the ramps
    assert _capi._flags2(_extensions(0, gen_min_output=floor)[2], 0) == 0


# ---- the host route --------------------------------------------------------------------------------------------------------------------

def _floored_three_node():
    nodes, lines, gens, stos = pkg.three_node_case()
    gens[2].min_generation = 120.0
    return nodes, lines, gens, stos


def test_generator_default_pack_and_shard(three_node):
    nodes, lines, gens, stos, pp = three_node
    assert all(g.min_generation == 0.0 for g in gens)
    assert not pp.has_min_output() and set(pp.engine_kwargs()) == BASE_KEYS             # yesterday's arguments while every floor is 0
    nodes, lines, gens, stos = _floored_three_node()
    pq = pkg.pack(nodes, gens, stos, lines)
    want = np.array([0.0, 0.0, 120.0, 0.0])
    assert pq.has_min_output() and np.array_equal(pq.gen_min_output, want) and not pq.has_ramp()
    kw = pq.engine_kwargs()
    assert set(kw) == BASE_KEYS | {"gen_min_output"} and np.array_equal(kw["gen_min_output"], want)
    a, b = pq.shard(0, 2), pq.shard(1, 2)
    assert np.array_equal(a.gen_min_output, want[:2]) and np.array_equal(b.gen_min_output, want[2:])
    # every rank runs with the ramp flag: the shard without a floor of its own asks for it through its (infinite) ramps
    assert set(a.engine_kwargs()) == BASE_KEYS | {"gen_ramp"} and set(b.engine_kwargs()) == BASE_KEYS | {"gen_ramp", "gen_min_output"}
    assert "gen_ramp" not in pp.shard(0, 2).engine_kwargs()
    for bad in (-1.0, np.nan, 301.0):
        gens[2].min_generation = bad
        with pytest.raises(ValueError):
            pkg.pack(nodes, gens, stos, lines)


def test_the_device_lp_front_ends_refuse_a_floor(three_node):
    nodes, lines, gens, stos = _floored_three_node()
    pq = pkg.pack(nodes, gens, stos, lines)
    with pytest.raises(ValueError, match="minimum output"):
        central.central_reference_on_device(nodes, gens, stos, lines)
    with pytest.raises(ValueError, match="minimum output"):
        central.central_reference_coupled_on_device(nodes, gens, stos, lines)
    with pytest.raises(_capi.DopfError, match="minimum output"):
        _capi.central_solve(None, **pq.engine_kwargs())
    with pytest.raises(_capi.DopfError, match="minimum output"):
        _capi.central_solve_coupled(None, **pq.engine_kwargs())


def test_an_api_without_the_entry_refuses_with_the_tables_texts(three_node, oracle_api):
    x, pp = _capi.EXTENSIONS_FLOOR[0], three_node[4]
    assert not hasattr(oracle_api, x.entry)
    build = lambda **kw: _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, **kw, **pp.engine_kwargs())
    e = build(gen_min_output=np.zeros(pp.G))
    assert e.params.flags == 0
    with pytest.raises(_capi.DopfError) as err:
        build(gen_min_output=np.full(pp.G, 1.0))
    assert str(err.value) == f"oracle_*: this API has no {x.what} ({x.why})"
    with pytest.raises(_capi.DopfError) as err:
        e.set_min_output()
    assert str(err.value) == f"oracle_*: this API has no {x.what} (unsupported)"


# ---- the host LP -----------------------------------------------------------------------------------------------------------------------

def test_host_lp_with_floors_on_the_three_node_case(three_node):
    pp = three_node[4]
    base = central.solve_central_packed(pp)
    zero = central.solve_central_packed(pp, gen_min_output=np.zeros(pp.G))
    assert zero.objective == base.objective and np.array_equal(zero.generation, base.generation)
    floor = np.array([0.0, 0.0, 0.0, 60.0])                   # gas (50 per MWh) must run at 60
    assert base.generation[3].min() < 60.0 - 1.0
    r = central.solve_central_packed(pp, gen_min_output=floor)
    assert r.objective > base.objective * (1.0 + 1e-6)
    assert (floor[:, None] - r.generation).max() <= 1e-9 * pp.gen_pmax.max()
    nodes, lines, gens, stos = pkg.three_node_case()
    gens[3].min_generation = 60.0
    packed = central.solve_central_packed(pkg.pack(nodes, gens, stos, lines))          # the packed case's own floors
    assert packed.objective == r.objective
    # the floor follows an outage down: lb = min(p_min, ub)
    prof, of = np.array([[0.0, 1.0]]), np.array([-1, -1, -1, 0], dtype=np.int32)
    out = central.solve_central_packed(pp, availability=(prof, of), gen_min_output=floor)
    assert out.generation[3, 0] == 0.0 and out.generation[3, 1] >= 60.0 - 1e-9 * 120.0


# ---- the twins -------------------------------------------------------------------------------------------------------------------------

def test_ramp_project_floor_against_a_dense_qp_and_the_certificate(oracle_api):
    n = rest = rise = anchored = up0 = repaired = 0
    worst = 0.0
    for c, q, lo, cap, up, down, prev in floor_cases(240, 31):
        assert c.size <= 8 and path_exists(lo, cap, up, down, prev) is None
        x = ramp_project_floor(c, q, lo, cap, up, down, prev)
        y = qp_row(oracle_api, [line_step(q, ct) for ct in c], lo, cap, up, down, prev)
        err = float(np.abs(x - y).max())
        assert err <= 1e-9 * max(1.0, float(cap.max())), (n, err)
        worst = max(worst, err / max(1.0, float(cap.max())))
        infeas, stat = floor_kkt_violation(x, q * (x - c), lo, cap, up, down, prev)
        assert infeas <= 1e-12 and stat <= 1e-8, (n, infeas, stat)
        n += 1
        rest += bool(np.any((x == lo) & (lo > 0.0)))
        rise += bool(np.any((cap[:-1] == 0.0) & (lo[1:] > 0.0)))
        anchored, up0 = anchored + (prev is not None), up0 + (up == 0.0)
        repaired += not np.array_equal(x, np.clip(c, lo, cap))
    print(f"{n} rows against the QP, worst {worst:.1e} of the capacity: {rest} rest on the floor, {rise} with a floor that rises behind "
          f"a zero cap, {anchored} anchored, {up0} with up = 0, {repaired} repaired")
    assert n >= 200 and min(rest, repaired) >= n // 4 and min(rise, anchored, up0) >= n // 10, (n, rest, rise, anchored, up0, repaired)


def test_ramp_project_pwl_floor_against_a_dense_qp_and_the_certificate(oracle_api):
    n = rest = rise = anchored = up0 = kinked = 0
    worst = 0.0
    for steps, lo, cap, up, down, prev in pwl_floor_cases(240, 32):
        assert len(steps) <= 8 and path_exists(lo, cap, up, down, prev) is None
        info = {}
        x = ramp_project_pwl_floor(steps, lo, cap, up, down, prev, info)
        y = qp_row(oracle_api, steps, lo, cap, up, down, prev)
        err = float(np.abs(x - y).max())
        assert err <= 1e-9 * max(1.0, float(cap.max())), (n, err)
        worst = max(worst, err / max(1.0, float(cap.max())))
        grad = np.array([phi_at(s, v) for s, v in zip(steps, x)])
        infeas, stat = floor_kkt_violation(x, grad, lo, cap, up, down, prev)
        assert infeas <= 1e-12 and stat <= 1e-8, (n, infeas, stat)
        n += 1
        rest += info["on_floor"]
        rise += bool(np.any((cap[:-1] == 0.0) & (lo[1:] > 0.0)))
        anchored, up0, kinked = anchored + (prev is not None), up0 + (up == 0.0), kinked + (sum(info["merged"]) >= 1)
    print(f"{n} rows against the QP, worst {worst:.1e} of the capacity: {rest} rest on the floor, {rise} with a floor that rises behind "
          f"a zero cap, {anchored} anchored, {up0} with up = 0, {kinked} with kinks merged")
    assert n >= 200 and rest >= n // 4 and min(rise, anchored, up0, kinked) >= n // 10, (n, rest, rise, anchored, up0, kinked)


def test_at_a_zero_floor_the_twins_are_the_old_helpers_bit_for_bit():
    rng = np.random.default_rng(7)
    n = 0
    for steps, cap, up, down, prev in pwl_cases(160, 33, tmax=24):
        T = len(steps)
        info, info0 = {}, {}
        a, b = ramp_project_pwl(steps, cap, up, down, prev, info), ramp_project_pwl_floor(steps, np.zeros(T), cap, up, down, prev, info0)
        assert np.array_equal(a, b) and info["most"] == info0["most"] and info["merged"] == info0["merged"]
        assert np.array_equal(a, ramp_project_pwl_floor(steps, 0.0, cap, up, down, prev))
        q, pm = float(rng.uniform(0.5, 3.0)), float(cap.max()) + 1.0
        c = rng.uniform(-0.5 * pm, 1.5 * pm, T)
        if prev is None or max(0.0, prev - min(down, max(pm - 1.0, prev))) <= min(cap[0], prev + up):
            try:
                want = ramp_project(c, q, cap, up, down, prev)
            except AssertionError:              # (ramp_project asserts feasibility where the pwl form widens: not a row of this test)
                continue
            assert np.array_equal(want, ramp_project_floor(c, q, np.zeros(T), cap, up, down, prev))
            assert np.array_equal(want, ramp_project_floor(c, q, 0.0, cap, up, down, prev))
            n += 1
    assert n >= 100, n


def test_path_exists_is_the_anchor_check_at_a_zero_floor():
    """F_t at lo = 0: the lower ends are lo_t = max(0, lo_{t-1} - down) from prev, the upper ends never fall below them while
    lo_t <= cap_t — dopf_set_generator_ramp's check"""
    for steps, cap, up, down, prev in pwl_cases(200, 34, tmax=12):
        if prev is None:
            assert path_exists(np.zeros(len(cap)), cap, up, down, None) is None
            continue
        lo, fits = prev, True
        for t in range(len(cap)):
            lo = max(0.0, lo - down)
            fits = fits and lo <= cap[t]
        assert (path_exists(np.zeros(len(cap)), cap, up, down, prev) is None) == fits
