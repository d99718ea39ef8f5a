"""DOPF_F_LINE_RATING without a GPU: the header, the bindings, the host route of the table (Line.rating -> pack ->
engine_kwargs), the host LP with a table, horizon.shift_window, and the NumPy Psi of the GPU tests' certificate."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, build_oracle, pkg
from decentralopf_jl_amd import _capi, central, shift_window, synth
from helpers_efficiency import psi_at
from helpers_line_rating import STOC, case, constant_table, draw_table, psi_at_rated

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
ENTRY = ("dopf_set_line_rating", "dopf_multi_set_line_rating")
BASE_KEYS = {"N", "L", "T", "demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax",
             "sto_node"}


def test_header_defines_the_flag():
    m = re.search(r"#define\s+DOPF_F_LINE_RATING\s+(\d+)", HDR)
    assert m and int(m.group(1)) == 1 << 29 == 536870912 == _capi.F_LINE_RATING
    others = [int(v) for k, v in re.findall(r"#define\s+(DOPF_F_\w+)\s+(\d+)", HDR) if k != "DOPF_F_LINE_RATING"]
    assert others and all(v & (1 << 29) == 0 for v in others)


def test_header_declares_both_entry_points():
    assert re.search(r"^int dopf_set_line_rating\(dopf_ctx \*ctx, const double \*rating[^)]*\);$", HDR, re.M)
    assert re.search(r"^int\s+dopf_multi_set_line_rating\(dopf_multi \*m, const double \*rating[^)]*\);$", HDR, re.M)
    assert "does NOT take the line out of the PTDF" in HDR          # a rating of 0 is not an outage


def test_library_exports_both_entry_points():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    for name in ENTRY:
        assert hasattr(lib, name), name


def test_ctypes_signatures_match_the_header():
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for name in ("set_line_rating", "multi_set_line_rating"):
        f = getattr(api, name)
        assert f.restype is ctypes.c_int
        assert len(f.argtypes) == 2 and f.argtypes[0] is ctypes.c_void_p and f.argtypes[1] is ctypes.POINTER(ctypes.c_double)


def test_julia_shim_defines_the_flag_and_the_setter():
    m = re.search(r"^const DOPF_F_LINE_RATING = (\d+)", JL, re.M)
    assert m and int(m.group(1)) == _capi.F_LINE_RATING
    assert re.search(r"^function set_line_rating!\(admm::ADMM", JL, re.M)
    for name in ENTRY:
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cdouble\}\)" % name, JL), name


def _derated_three_node():
    """the shipped case with line 0 at 0.75 f_max (15 instead of 20) in the second timestep only"""
    nodes, lines, gens, stos = pkg.three_node_case()
    lines[0].rating = [20, 15]
    return nodes, lines, gens, stos


def test_pack_and_engine_kwargs_carry_the_table_only_when_a_line_has_one(three_node):
    nodes, lines, gens, stos, pp = three_node
    assert all(l.rating is None for l in lines) and pp.line_rating is None
    assert set(pp.engine_kwargs()) == BASE_KEYS                      # yesterday's arguments
    nodes, lines, gens, stos = _derated_three_node()
    pr = pkg.pack(nodes, gens, stos, lines)
    want = np.array([[20.0, 15.0], [45.0, 45.0], [70.0, 70.0]])      # lines without a rating: max_capacity throughout
    assert np.array_equal(pr.line_rating, want)
    kw = pr.engine_kwargs()
    assert set(kw) == BASE_KEYS | {"line_rating"} and np.array_equal(kw["line_rating"], want)
    assert np.array_equal(pr.shard(1, 2).line_rating, want)          # replicated state: every shard carries the whole table
    for bad in ([20.0], [20.0, -1.0], [20.0, np.nan], [np.inf, 20.0]):
        lines[0].rating = bad
        with pytest.raises(ValueError):
            pkg.pack(nodes, gens, stos, lines)


def test_rating_buffer_is_line_major_within_a_timestep():
    r = np.arange(6.0).reshape(3, 2)                                 # (L, T)
    buf = _capi._rating_buffer(r, 3, 2)
    assert np.array_equal(buf, [0.0, 2.0, 4.0, 1.0, 3.0, 5.0])       # [l + L*t]


def test_oracle_backend_refuses_a_table_other_than_f_max(three_node):
    from oracle.binding import OracleApi
    nodes, lines, gens, stos, pp = three_node
    api = OracleApi(build_oracle())
    assert not hasattr(api, "set_line_rating")                       # loads without the symbols
    e = _capi.Engine(api, params=_capi.default_params(), mode=0, **pp.engine_kwargs())
    with pytest.raises(_capi.DopfError, match="unsupported"):
        e.set_line_rating(constant_table(pp))
    with pytest.raises(_capi.DopfError, match="no line ratings"):
        _capi.Engine(api, params=_capi.default_params(), mode=0, line_rating=0.5 * constant_table(pp), **pp.engine_kwargs())
    _capi.Engine(api, params=_capi.default_params(), mode=0, line_rating=constant_table(pp), **pp.engine_kwargs())   # f_max: nothing to set


def test_central_lp_with_a_table(three_node):
    nodes, lines, gens, stos, pp = three_node
    base = central.solve_central_packed(pp)
    assert abs(base.objective - 14035.0) <= 1e-6 * 14035.0
    same = central.solve_central_packed(pp, line_rating=constant_table(pp))
    for name in ("objective", "generation", "discharge", "charge", "level", "injection", "line_utilization", "system_price",
                 "flow_upper_dual", "flow_lower_dual", "nodal_price"):
        assert np.array_equal(getattr(base, name), getattr(same, name)), name
    nodes, lines, gens, stos = _derated_three_node()
    pr = pkg.pack(nodes, gens, stos, lines)
    for r in (central.solve_central_packed(pr), central.solve_central_packed(pp, line_rating=pr.line_rating),
              central.central_reference(nodes, gens, stos, lines)):
        assert abs(r.objective - 14685.0) <= 1e-6 * 14685.0, r.objective
        assert abs(r.line_utilization[0, 1]) <= 15.0 + 1e-9 and np.all(np.abs(r.line_utilization) <= pr.line_rating + 1e-9)
    with pytest.raises(ValueError, match="no line ratings"):
        central.central_reference_on_device(nodes, gens, stos, lines)
    with pytest.raises(_capi.DopfError, match="no line ratings"):
        _capi.central_solve(None, **pr.engine_kwargs())


def test_shift_window_moves_the_table_by_the_rolls_rule():
    pp = case(STOC)
    T, k = pp.T, 5
    rng = np.random.default_rng(7)
    rating = draw_table(pp)
    z = lambda r: rng.uniform(0.0, 1.0, (r, T))
    kw = dict(demand=pp.demand, P=z(pp.G), D=z(pp.S), C=z(pp.S), E=z(pp.S), lam=rng.uniform(1, 9, T), mu=z(pp.L), rho=z(pp.L),
              avg_U=z(pp.L), avg_K=z(pp.L), sto_emax=pp.sto_emax)
    tail = np.ones((pp.N, k))
    w = shift_window(k, tail, line_rating=rating, **kw)
    assert np.array_equal(w["line_rating"][:, :T - k], rating[:, k:])
    assert np.array_equal(w["line_rating"][:, T - k:], np.repeat(rating[:, T - 1:T], k, axis=1))      # a derating persists
    plain = shift_window(k, tail, **kw)
    assert "line_rating" not in plain and all(np.array_equal(plain[n], w[n]) for n in plain)


def test_psi_under_a_constant_table_is_the_psi_of_the_efficiency_tests():
    """helpers_line_rating.psi_at_rated against helpers_efficiency.psi_at, which is pinned against the oracle"""
    pp = case(STOC)
    rng = np.random.default_rng(11)
    z = lambda r, hi: rng.uniform(0.0, hi, (r, pp.T))
    lam, mu, rho, inj = rng.uniform(1, 30, pp.T), z(pp.L, 1), z(pp.L, 1), rng.uniform(-40, 40, (pp.N, pp.T))
    flow = pp.f_max[:, None] * rng.choice([-1.2, 0.5, 1.2], (pp.L, pp.T))      # (F cancels where both slacks are active: overload some)
    aU, aK, dlt = z(pp.L, 3), z(pp.L, 3), rng.uniform(-10, 10, (pp.S, pp.T))
    a = psi_at(pp, lam, mu, rho, inj, flow, aU, aK, 0.03, 10.0, dlt)
    b = psi_at_rated(pp, lam, mu, rho, inj, flow, aU, aK, 0.03, 10.0, dlt, constant_table(pp))
    assert np.array_equal(a, b)
    c = psi_at_rated(pp, lam, mu, rho, inj, flow, aU, aK, 0.03, 10.0, dlt, draw_table(pp))
    assert np.abs(c - a).max() > 1.0                 # (and a real table moves it)
