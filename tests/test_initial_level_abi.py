"""Storage initial levels (DOPF_F_STO_INITIAL_LEVEL) at the boundary: the header, the exports, the ctypes signatures, the
Julia shim, network.Storage / pack / engine_kwargs, and the central LP with a level before the first timestep. No compute
calls on a device (runs without a GPU)."""
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
ENTRY = ("dopf_set_storage_initial_level", "dopf_multi_set_storage_initial_level")


def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_defines_the_flag():
    m = re.search(r"#define\s+DOPF_F_STO_INITIAL_LEVEL\s+(\d+)", HDR)
    assert m and int(m.group(1)) == 1 << 25 == _capi.F_STO_INITIAL_LEVEL


def test_header_declares_both_entry_points():
    assert _prototype("dopf_set_storage_initial_level") == ["dopf_ctx *ctx", "const double *e0"]
    assert _prototype("dopf_multi_set_storage_initial_level") == ["dopf_multi *m", "const double *e0"]


def test_header_cites_the_reference_lines():
    assert "subproblems.jl:154" in HDR and "opf_central_reference.jl:53" in HDR


def test_library_exports_both_entry_points():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    for name in ENTRY:
        assert hasattr(lib, name), name


def test_ctypes_signatures_match_the_header():
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for name in ("set_storage_initial_level", "multi_set_storage_initial_level"):
        f = getattr(api, name)
        assert f.restype is ctypes.c_int
        assert len(f.argtypes) == 2
        assert f.argtypes[1] is ctypes.POINTER(ctypes.c_double)


def test_oracle_api_has_no_initial_level_and_refuses_non_zero_levels(three_node, oracle_api):
    *_, pp = three_node
    assert not hasattr(oracle_api, "set_storage_initial_level")
    with pytest.raises(_capi.DopfError, match="initial level"):
        _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, sto_e0=[7.0], **pp.engine_kwargs())
    # all zeros is what the oracle computes anyway: accepted, no flag
    e = _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, sto_e0=[0.0], **pp.engine_kwargs())
    e.close()


def test_julia_shim_defines_the_flag_and_the_setter():
    m = re.search(r"^const DOPF_F_STO_INITIAL_LEVEL = (\d+)", JL, re.M)
    assert m and int(m.group(1)) == _capi.F_STO_INITIAL_LEVEL
    assert re.search(r"^function set_initial_levels!\(admm::ADMM", JL, re.M)
    for name in ENTRY:
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cdouble\}\)" % name, JL), name


def test_storage_defaults_to_an_empty_start(three_node):
    nodes, lines, gens, stos, pp = three_node
    assert Storage("s", 1, 10, 20, "purple", nodes[0]).initial_level == 0.0
    assert [s.initial_level for s in stos] == [0.0]
    assert "sto_e0" not in pp.engine_kwargs()
    assert np.array_equal(pp.sto_e0, [0.0])


def test_pack_carries_the_level_and_engine_kwargs_pass_it_only_when_non_zero(three_node):
    nodes, lines, gens, _, _ = three_node
    stos = [Storage("battery", 1, 10, 20, "purple", nodes[0], initial_level=7.0)]
    pp = pkg.pack(nodes, gens, stos, lines)
    assert np.array_equal(pp.sto_e0, [7.0])
    kw = pp.engine_kwargs()
    assert np.array_equal(kw["sto_e0"], [7.0])
    assert np.array_equal(pp.shard(0, 1).sto_e0, [7.0])


@pytest.mark.parametrize("e0,objective", [(None, 14035.0), ([0.0], 14035.0), ([7.0], 14007.0), ([20.0], 13975.0)])
def test_central_lp_starts_from_the_initial_level(three_node, e0, objective):
    *_, pp = three_node
    r = central.solve_central_packed(pp, initial_level=e0)
    assert abs(r.objective - objective) <= 1e-6 * objective, r.objective
    start = 0.0 if e0 is None else e0[0]
    D, C, E = r.discharge, r.charge, r.level
    assert np.allclose(E[:, 0], start + C[:, 0] - D[:, 0], atol=1e-9)
    assert np.allclose(E, start + np.cumsum(C - D, axis=1), atol=1e-9)
    assert E.min() >= -1e-9 and (E - pp.sto_emax[:, None]).max() <= 1e-9


def test_central_reference_takes_the_level_from_the_storages(three_node):
    nodes, lines, gens, _, _ = three_node
    stos = [Storage("battery", 1, 10, 20, "purple", nodes[0], initial_level=20.0)]
    assert abs(central.central_reference(nodes, gens, stos, lines).objective - 13975.0) <= 1e-6 * 13975.0
    # an explicit level wins over the storages'
    assert abs(central.central_reference(nodes, gens, stos, lines, initial_level=[7.0]).objective - 14007.0) <= 1e-6 * 14007.0
