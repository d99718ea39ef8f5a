"""DOPF_F_GEN_RAMP without a GPU: the header, the bindings, the host route of the ramps (Generator.ramp_up / ramp_down ->
pack -> engine_kwargs -> shard), the refusals of the device LP and of an API without the entries, the ramp rows of the host LP, and
the two helpers the GPU tests stand on — the NumPy projection (the value reference) and its optimality certificate."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg
from decentralopf_jl_amd import _capi, admm, central, sharded, synth
from helpers_ramp import ramp_active, ramp_infeasibility, ramp_kkt_violation, ramp_project

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
ENTRY = ("dopf_set_generator_ramp", "dopf_multi_set_generator_ramp")
BASE_KEYS = {"N", "L", "T", "demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax",
             "sto_node"}
DP = ctypes.POINTER(ctypes.c_double)


def test_header_defines_the_flag_on_the_free_bit():
    m = re.search(r"#define\s+DOPF_F_GEN_RAMP\s+(\d+)", HDR)
    assert m and int(m.group(1)) == 32 == _capi.F_GEN_RAMP
    others = [int(v) for k, v in re.findall(r"#define\s+(DOPF_F_\w+)\s+(\d+)", HDR) if k != "DOPF_F_GEN_RAMP"]
    assert others and all(v & 32 == 0 for v in others)
    flag = HDR[HDR.index("#define DOPF_F_GEN_RAMP"):]
    assert "ignore the flag" in flag[:flag.index("*/")]


def test_header_declares_both_entry_points():
    assert re.search(r"^int dopf_set_generator_ramp\(dopf_ctx \*ctx, const double \*ramp_up[^)]*const double \*ramp_down[^)]*"
                     r"const double \*p_prev[^)]*\);$", HDR, re.M | re.S)
    assert re.search(r"^int\s+dopf_multi_set_generator_ramp\(dopf_multi \*m, const double \*ramp_up, const double \*ramp_down, "
                     r"const double \*p_prev\);$", HDR, re.M)


def test_library_exports_both_entry_points():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    for name in ENTRY:
        assert hasattr(lib, name), name


def test_ctypes_signatures_match_the_header():
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for name in ("set_generator_ramp", "multi_set_generator_ramp"):
        f = getattr(api, name)
        assert f.restype is ctypes.c_int
        assert list(f.argtypes) == [ctypes.c_void_p, DP, DP, DP]


def test_julia_shim_defines_the_flag_and_the_setter():
    m = re.search(r"^const DOPF_F_GEN_RAMP = (\d+)", JL, re.M)
    assert m and int(m.group(1)) == _capi.F_GEN_RAMP
    assert re.search(r"^function set_ramp!\(admm::ADMM", JL, re.M)
    for name in ENTRY:
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cdouble\}, Ptr\{Cdouble\}, Ptr\{Cdouble\}\)" % name, JL), name


def test_the_table_keeps_its_six_rows_and_the_new_row_is_behind_them():
    assert len(_capi.EXTENSIONS) == 6 and [x.setter for x in _capi.EXTENSIONS_MORE] == ["set_ramp"]
    x = _capi.EXTENSIONS_MORE[0]
    assert x.flag == _capi.F_GEN_RAMP and x.entry == "set_generator_ramp" and x.keys == ("gen_ramp", "gen_prev")
    assert _capi._BY_SETTER["set_ramp"] is x and list(_capi._BY_SETTER)[:6] == [y.setter for y in _capi.EXTENSIONS]
    order = [y.setter for y in _capi.EXTENSIONS + _capi.EXTENSIONS_MORE]
    assert order.index("set_ramp") > order.index("set_availability")          # its check reads the caps
    for cls in (_capi.Engine, _capi.MultiEngine, admm.ADMM, sharded.ShardedADMM):
        assert callable(getattr(cls, "set_ramp")), cls


def _ramped_three_node():
    nodes, lines, gens, stos = pkg.three_node_case()
    gens[2].ramp_up, gens[2].ramp_down = 40.0, 25.0
    gens[3].ramp_down = 10.0
    return nodes, lines, gens, stos


def test_generator_default_pack_and_shard(three_node):
    nodes, lines, gens, stos, pp = three_node
    assert all(g.ramp_up == np.inf and g.ramp_down == np.inf for g in gens)
    assert not pp.has_ramp() and set(pp.engine_kwargs()) == BASE_KEYS             # yesterday's arguments while every ramp is inf
    nodes, lines, gens, stos = _ramped_three_node()
    pq = pkg.pack(nodes, gens, stos, lines)
    up, down = np.array([np.inf, np.inf, 40.0, np.inf]), np.array([np.inf, np.inf, 25.0, 10.0])
    assert pq.has_ramp() and np.array_equal(pq.gen_ramp[0], up) and np.array_equal(pq.gen_ramp[1], down)
    kw = pq.engine_kwargs()
    assert set(kw) == BASE_KEYS | {"gen_ramp"} and np.array_equal(kw["gen_ramp"][0], up) and np.array_equal(kw["gen_ramp"][1], down)
    a, b = pq.shard(0, 2), pq.shard(1, 2)
    assert np.array_equal(a.gen_ramp[0], up[:2]) and np.array_equal(b.gen_ramp[1], down[2:])
    assert "gen_ramp" in a.engine_kwargs() and "gen_ramp" in b.engine_kwargs()   # every rank runs with the flag, its slice all inf or not
    assert "gen_ramp" not in pp.shard(0, 2).engine_kwargs()
    for bad in (-1.0, np.nan):
        gens[0].ramp_up = bad
        with pytest.raises(ValueError):
            pkg.pack(nodes, gens, stos, lines)


def test_an_api_without_the_entry_refuses_with_the_tables_texts(three_node, oracle_api):
    x, pp = _capi.EXTENSIONS_MORE[0], three_node[4]
    assert not hasattr(oracle_api, x.entry)
    build = lambda **kw: _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, **kw, **pp.engine_kwargs())
    e = build(gen_ramp=(np.full(pp.G, np.inf), np.full(pp.G, np.inf)))          # the default value: nothing to set, and no flag
    assert e.params.flags == 0 and all(v is None for v in e._mirror.values())
    for other in (dict(gen_ramp=(np.full(pp.G, 5.0), np.full(pp.G, np.inf))), dict(gen_prev=np.zeros(pp.G))):
        with pytest.raises(_capi.DopfError) as err:
            build(**other)
        assert str(err.value) == f"oracle_*: this API has no {x.what} ({x.why})"
    with pytest.raises(_capi.DopfError) as err:
        e.set_ramp()
    assert str(err.value) == f"oracle_*: this API has no {x.what} (unsupported)"


def test_the_device_lp_refuses_a_ramped_case(three_node):
    nodes, lines, gens, stos = _ramped_three_node()
    pq = pkg.pack(nodes, gens, stos, lines)
    with pytest.raises(ValueError, match="ramp"):
        central.central_reference_on_device(nodes, gens, stos, lines)
    with pytest.raises(_capi.DopfError, match="ramp"):
        _capi.central_solve(None, **pq.engine_kwargs())
    with pytest.raises(_capi.DopfError, match="ramp"):
        _capi.central_solve(None, gen_prev=np.zeros(pq.G), **three_node[4].engine_kwargs())


# ---- the host LP with ramp rows ---------------------------------------------------------------------------------------------------

def test_host_lp_with_ramp_rows_on_a_case_known_by_hand():
    """One node, T = 4, demand 10 10 50 10; A (cost 1, 100 MW, ramps 20 up and down) and B (cost 5, 100 MW, free). Without ramps A
    serves everything: 80. The balance ties A + B to the demand, so A <= 10 at t = 0, 1, 3 and, from 10, A <= 30 at t = 2: A = 10 10
    30 10, B = 0 0 20 0, 60 + 100 = 160. Anchored at 0 before the window A reaches 10 at t = 0 all the same: 160. Anchored at 40 it
    must stay at or above 20 there, over the demand: infeasible."""
    n = pkg.Node("N", [10, 10, 50, 10], True)
    gens = [pkg.Generator("A", 1, 100, "k", n, ramp_up=20.0, ramp_down=20.0), pkg.Generator("B", 5, 100, "k", n)]
    pp = pkg.pack([n], gens, [], [])
    free = central.solve_central_packed(pp, gen_ramp=(np.full(2, np.inf), np.full(2, np.inf)))
    assert abs(free.objective - 80.0) <= 1e-9
    r = central.solve_central_packed(pp)                            # the packed case's ramps
    assert abs(r.objective - 160.0) <= 1e-9
    assert np.allclose(r.generation, [[10, 10, 30, 10], [0, 0, 20, 0]], atol=1e-9)
    r = central.solve_central_packed(pp, gen_prev=np.zeros(2))
    assert abs(r.objective - 160.0) <= 1e-9
    with pytest.raises(RuntimeError):
        central.solve_central_packed(pp, gen_prev=np.array([40.0, 0.0]))


# ---- the helpers --------------------------------------------------------------------------------------------------------------------

def _cases(n, seed):
    """seeded rows: T = 1 .. 40, caps that drop to 0, ramps from {inf, 0, 2 % .. 30 % of pmax}, every second one anchored (where
    the anchor can come down under the caps)"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        T = 1 if k % 10 == 9 else int(rng.integers(2, 41))
        q, pm = float(rng.uniform(0.5, 3.0)), float(rng.uniform(10.0, 100.0))
        cap = np.full(T, pm)
        if k % 3 == 0:
            cap = pm * rng.uniform(0.0, 1.0, T)
            cap[rng.random(T) < 0.25] = 0.0
        c = rng.uniform(-0.5 * pm, 1.5 * pm, T)
        draw = lambda: float(rng.uniform(0.02, 0.30) * pm)
        up = (np.inf, 0.0, draw())[k % 3] if k % 7 else draw()
        down = (draw(), np.inf, 0.0)[k % 3] if k % 5 else draw()
        prev = None
        if k % 2 == 0:
            prev, lo, fits = float(rng.uniform(0.0, pm)), None, True
            lo = prev
            for t in range(T):
                lo = max(0.0, lo - down)
                fits = fits and lo <= cap[t]
            prev = prev if fits else None
        yield c, q, cap, up, down, prev


def _slsqp(c, q, cap, up, down, prev):
    from scipy.optimize import minimize
    T = c.size
    D = np.eye(T) - np.eye(T, k=-1)
    off = np.zeros(T)
    if prev is None:
        D, off = D[1:], off[1:]
    else:
        off[0] = -prev
    cons = []
    if np.isfinite(up) and D.shape[0]:
        cons.append(dict(type="ineq", fun=lambda x: up - (D @ x + off), jac=lambda x: -D))
    if np.isfinite(down) and D.shape[0]:
        cons.append(dict(type="ineq", fun=lambda x: down + (D @ x + off), jac=lambda x: D))
    f = lambda x: 0.5 * q * float((x - c) @ (x - c))
    x0 = np.zeros(T) if prev is None else np.minimum(cap, np.maximum(0.0, prev - down * np.arange(1, T + 1)))
    r = minimize(f, x0, jac=lambda x: q * (x - c), bounds=list(zip(np.zeros(T), cap)), constraints=cons, method="SLSQP",
                 options=dict(ftol=1e-14, maxiter=500))
    return f(r.x), r.x


def test_ramp_project_against_slsqp_and_the_certificate():
    n = active = anchored = 0
    worst = [0.0, 0.0]
    for c, q, cap, up, down, prev in _cases(240, 5):
        knots = []
        x = ramp_project(c, q, cap, up, down, prev, knots)
        assert knots[0] <= 2 * c.size + 2
        assert ramp_infeasibility(x, cap, up, down, prev) <= 1e-12
        f = 0.5 * q * float((x - c) @ (x - c))
        fs, xs = _slsqp(c, q, cap, up, down, prev)
        if ramp_infeasibility(xs, cap, up, down, prev) <= 1e-9:
            assert f <= fs + 1e-9 * max(1.0, abs(fs)), (n, f, fs)                # never above SLSQP's
        infeas, stat = ramp_kkt_violation(x, q * (x - c), cap, up, down, prev)
        assert infeas <= 1e-12 and stat <= 1e-8, (n, infeas, stat)
        worst = [max(worst[0], infeas), max(worst[1], stat)]
        n, active, anchored = n + 1, active + ramp_active(x, up, down, prev), anchored + (prev is not None)
    assert n >= 200 and active >= n // 2 and anchored >= n // 5, (n, active, anchored)
    print(f"{n} cases, {active} with an active ramp, {anchored} anchored: infeasibility {worst[0]:.1e}, stationarity {worst[1]:.1e}")


def test_the_certificate_catches_a_wrong_ramp():
    """the projection under a ramp_up off by 10 %: wherever it differs from the right one, the certificate says so"""
    differ = caught = 0
    for c, q, cap, up, down, prev in _cases(240, 5):
        if not np.isfinite(up) or up == 0.0:
            continue
        x, y = ramp_project(c, q, cap, up, down, prev), ramp_project(c, q, cap, 1.1 * up, down, prev)
        if np.abs(x - y).max() <= 1e-6:
            continue
        differ += 1
        infeas, stat = ramp_kkt_violation(y, q * (y - c), cap, up, down, prev)
        caught += max(infeas, stat) > 1e-6
    print(f"caught {caught} of the {differ} that differ")
    assert differ >= 40 and caught == differ, (differ, caught)


def test_ramp_project_without_ramps_is_the_clamp():
    rng = np.random.default_rng(2)
    c, cap = rng.uniform(-50.0, 150.0, 30), rng.uniform(0.0, 100.0, 30)
    assert np.abs(ramp_project(c, 1.3, cap, np.inf, np.inf) - np.clip(c, 0.0, cap)).max() <= 1e-12      # (the zero crossing is interpolated)


def test_synthetic_cases_carry_no_ramp():
    assert not synth.synthetic_case(7, 0, 5, seed=3).has_ramp()
