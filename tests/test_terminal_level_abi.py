"""Storage terminal levels (DOPF_F_STO_TERMINAL_LEVEL) at the boundary: the header, the exports, the ctypes signatures, the
Julia shim, network.Storage / pack / engine_kwargs / shard, the oracle API's refusal, and the central LP with a band on the level
after the last timestep. No compute calls on a device (runs without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg
from decentralopf_jl_amd import _capi, central
from decentralopf_jl_amd.network import Storage

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
ENTRY = ("dopf_set_storage_terminal_level", "dopf_multi_set_storage_terminal_level")
BASE_KEYS = {"N", "L", "T", "demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax",
             "sto_node"}


def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_defines_the_flag():
    m = re.search(r"#define\s+DOPF_F_STO_TERMINAL_LEVEL\s+(\d+)", HDR)
    assert m and int(m.group(1)) == 1 << 26 == _capi.F_STO_TERMINAL_LEVEL
    # a bit of its own
    others = [int(v) for k, v in re.findall(r"#define\s+(DOPF_F_\w+)\s+(\d+)", HDR) if k != "DOPF_F_STO_TERMINAL_LEVEL"]
    assert all(v & (1 << 26) == 0 for v in others)


def test_header_declares_both_entry_points():
    assert _prototype("dopf_set_storage_terminal_level") == ["dopf_ctx *ctx", "const double *lo", "const double *hi"]
    assert _prototype("dopf_multi_set_storage_terminal_level") == ["dopf_multi *m", "const double *lo", "const double *hi"]


def test_library_exports_both_entry_points():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    for name in ENTRY:
        assert hasattr(lib, name), name


def test_ctypes_signatures_match_the_header():
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for name in ("set_storage_terminal_level", "multi_set_storage_terminal_level"):
        f = getattr(api, name)
        assert f.restype is ctypes.c_int
        assert len(f.argtypes) == 3
        assert f.argtypes[1] is ctypes.POINTER(ctypes.c_double) and f.argtypes[2] is ctypes.POINTER(ctypes.c_double)


def test_oracle_api_refuses_a_non_default_band(three_node, oracle_api):
    *_, pp = three_node
    assert not hasattr(oracle_api, "set_storage_terminal_level")
    for lo, hi in (([5.0], [20.0]), ([0.0], [10.0]), ([7.0], [7.0])):
        with pytest.raises(_capi.DopfError, match="terminal level"):
            _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, sto_end_lo=lo, sto_end_hi=hi, **pp.engine_kwargs())
    # the default band is what the oracle computes anyway: accepted, no flag
    e = _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, sto_end_lo=[0.0], sto_end_hi=[20.0],
                     **pp.engine_kwargs())
    assert e.params.flags & _capi.F_STO_TERMINAL_LEVEL == 0
    e.close()


def test_julia_shim_defines_the_flag_and_the_setter():
    m = re.search(r"^const DOPF_F_STO_TERMINAL_LEVEL = (\d+)", JL, re.M)
    assert m and int(m.group(1)) == _capi.F_STO_TERMINAL_LEVEL
    assert re.search(r"^function set_terminal_levels!\(admm::ADMM", JL, re.M)
    for name in ENTRY:
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cdouble\}, Ptr\{Cdouble\}\)" % name, JL), name


def test_storage_defaults_leave_the_engine_arguments_unchanged(three_node):
    nodes, lines, gens, stos, pp = three_node
    s = Storage("s", 1, 10, 20, "purple", nodes[0])
    assert s.terminal_level_min == 0.0 and s.terminal_level_max is None
    assert np.array_equal(pp.sto_end_lo, [0.0]) and np.array_equal(pp.sto_end_hi, [20.0])
    assert not pp.has_terminal_band()
    assert set(pp.engine_kwargs()) == BASE_KEYS
    # an explicit band equal to the default is still the default
    stos2 = [Storage("battery", 1, 10, 20, "purple", nodes[0], terminal_level_min=0.0, terminal_level_max=20.0)]
    assert set(pkg.pack(nodes, gens, stos2, lines).engine_kwargs()) == BASE_KEYS


def test_pack_carries_the_band_and_engine_kwargs_pass_it_only_when_not_default(three_node):
    nodes, lines, gens, _, _ = three_node
    stos = [Storage("battery", 1, 10, 20, "purple", nodes[0], terminal_level_min=5.0)]
    pp = pkg.pack(nodes, gens, stos, lines)
    assert np.array_equal(pp.sto_end_lo, [5.0]) and np.array_equal(pp.sto_end_hi, [20.0])
    kw = pp.engine_kwargs()
    assert np.array_equal(kw["sto_end_lo"], [5.0]) and np.array_equal(kw["sto_end_hi"], [20.0])
    stos = [Storage("battery", 1, 10, 20, "purple", nodes[0], terminal_level_max=12.0)]
    kw = pkg.pack(nodes, gens, stos, lines).engine_kwargs()
    assert np.array_equal(kw["sto_end_lo"], [0.0]) and np.array_equal(kw["sto_end_hi"], [12.0])


def test_shard_slices_the_band():
    from decentralopf_jl_amd import synth
    pp = synth.synthetic_case(20, 7, 24, seed=5)
    pp.sto_end_lo = np.arange(pp.S, dtype=np.float64) * 0.01
    pp.sto_end_hi = pp.sto_emax.copy()
    for world in (2, 3):
        parts = [pp.shard(r, world) for r in range(world)]
        assert np.array_equal(np.concatenate([p.sto_end_lo for p in parts]), pp.sto_end_lo)
        assert np.array_equal(np.concatenate([p.sto_end_hi for p in parts]), pp.sto_end_hi)
        for p in parts:
            s0, s1 = p.meta["sto_range"]
            assert np.array_equal(p.sto_end_lo, pp.sto_end_lo[s0:s1])


# HiGHS on the three-node case (T = 2, battery pmax 10, emax 20)
LP = [(0.0, 0.0, 20.0, 14035.0, None), (0.0, 5.0, 20.0, 14440.0, None), (0.0, 10.0, 20.0, 14845.0, None),
      (0.0, 20.0, 20.0, 15675.0, None), (7.0, 7.0, 7.0, 14035.0, [17.0, 7.0]), (20.0, 20.0, 20.0, 14805.0, None),
      (20.0, 10.0, 10.0, 13995.0, None)]


@pytest.mark.parametrize("e0,lo,hi,objective,levels", LP, ids=[f"e0={x[0]:g}-[{x[1]:g},{x[2]:g}]" for x in LP])
def test_central_lp_bounds_the_last_level(three_node, e0, lo, hi, objective, levels):
    *_, pp = three_node
    r = central.solve_central_packed(pp, initial_level=[e0], terminal_level=([lo], [hi]))
    assert abs(r.objective - objective) <= 1e-6 * objective, r.objective
    E = r.level
    assert lo - 1e-9 <= E[0, -1] <= hi + 1e-9
    assert np.allclose(E, e0 + np.cumsum(r.charge - r.discharge, axis=1), atol=1e-9)
    if levels is not None:
        assert np.allclose(E[0], levels, atol=1e-9)


def test_central_reference_takes_the_band_from_the_storages(three_node):
    nodes, lines, gens, _, _ = three_node
    stos = [Storage("battery", 1, 10, 20, "purple", nodes[0], terminal_level_min=10.0)]
    assert abs(central.central_reference(nodes, gens, stos, lines).objective - 14845.0) <= 1e-6 * 14845.0
    # an explicit band wins over the storages'
    r = central.central_reference(nodes, gens, stos, lines, terminal_level=([0.0], [20.0]))
    assert abs(r.objective - 14035.0) <= 1e-6 * 14035.0
    # the default band is the reference's problem
    stos = [Storage("battery", 1, 10, 20, "purple", nodes[0])]
    assert abs(central.central_reference(nodes, gens, stos, lines).objective - 14035.0) <= 1e-6 * 14035.0
