"""dopf_central_solve_lossy (the device LP with storage charge / discharge efficiencies) at the boundary: the header, the export, the
ctypes signature, the Python host's keywords and the Julia shim. No compute calls on a device (runs without a GPU)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg
from decentralopf_jl_amd import _capi, central

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
OUTS = ["double *P", "double *D", "double *C", "double *E", "double *system_price", "double *nodal_price",
        "double *line_utilization", "double *flow_upper_dual", "double *flow_lower_dual"]


def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry_as_ex_plus_the_two_efficiency_arrays():
    ex, lossy = _prototype("dopf_central_solve_ex"), _prototype("dopf_central_solve_lossy")
    at = ex.index("const double *sto_end_hi") + 1
    assert lossy == ex[:at] + ["const double *sto_eta_c", "const double *sto_eta_d"] + ex[at:]
    assert lossy[-9:] == OUTS


def test_header_says_which_entry_takes_the_efficiencies():
    flag = re.search(r"#define DOPF_F_STO_EFFICIENCY .*?\*/", HDR, re.S).group(0)
    flag = " ".join(flag.replace("*", " ").split())
    assert flag.endswith("dopf_central_solve(_ex) ignores the flag; dopf_central_solve_lossy takes the efficiencies. /")


def test_library_exports_the_entry():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    assert hasattr(lib, "dopf_central_solve_lossy")


def test_ctypes_signature_matches_the_header():
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    f = api.central_solve_lossy
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == ([ctypes.POINTER(_capi.DopfProblem), ctypes.POINTER(_capi.DopfParams), dp, dp, dp, dp, dp, ctypes.c_int32,
                                 dp, ip, ctypes.c_double, ctypes.c_int32, ctypes.POINTER(_capi.DopfCentralResult)] + [dp] * 9)
    assert len(f.argtypes) == len(_prototype("dopf_central_solve_lossy")) == len(api.central_solve_ex.argtypes) + 2


def test_python_host_takes_sto_eta_and_the_lossy_keyword():
    par = inspect.signature(_capi.central_solve).parameters
    assert "sto_eta" in par and par["sto_eta"].default is None and par["sto_eta"].kind is inspect.Parameter.KEYWORD_ONLY
    par = inspect.signature(central.central_reference_on_device).parameters
    assert "lossy" in par and par["lossy"].default is False and par["lossy"].kind is inspect.Parameter.KEYWORD_ONLY


def _three_node_with(eta_c, eta_d):
    nodes, lines, gens, stos = pkg.three_node_case()
    stos[0].charge_efficiency, stos[0].discharge_efficiency = eta_c, eta_d
    return nodes, lines, gens, stos


def test_every_engine_kwarg_of_a_lossy_case_is_a_central_solve_keyword():
    """What used to raise TypeError: a packed case with efficiencies, handed over as engine_kwargs()."""
    nodes, lines, gens, stos = _three_node_with(0.9, 0.8)
    kw = pkg.pack(nodes, gens, stos, lines).engine_kwargs()
    assert "sto_eta" in kw
    assert set(kw) <= set(inspect.signature(_capi.central_solve).parameters)


def test_device_reference_still_refuses_efficiencies_without_the_keyword():
    nodes, lines, gens, stos = _three_node_with(0.9, 0.9)
    with pytest.raises(ValueError, match="no storage efficiencies"):
        central.central_reference_on_device(nodes, gens, stos, lines)
    with pytest.raises(ValueError, match="no storage efficiencies"):
        central.central_reference_on_device(nodes, gens, stos, lines, lossy=False)
    nodes, lines, gens, stos = pkg.three_node_case()
    with pytest.raises(ValueError, match="no storage efficiencies"):
        central.central_reference_on_device(nodes, gens, stos, lines, efficiency=(np.full(1, 0.9), np.ones(1)))
    with pytest.raises(ValueError, match=r"\(0, 1\]"):              # (checked on the host before any device call, lossy or not)
        central.central_reference_on_device(nodes, gens, stos, lines, efficiency=(np.full(1, 1.1), np.ones(1)), lossy=True)


def test_julia_shim_calls_the_entry_only_under_the_keyword():
    m = re.search(r"ccall\(\(:dopf_central_solve_lossy, DOPF_LIB\), Cint,\s*\(([^)]*)\)", JL)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == (["Ref{CProblem}", "Ref{CParams}"] + ["Ptr{Cdouble}"] * 5 + ["Cint", "Ptr{Cdouble}", "Ptr{Cint}",
                     "Cdouble", "Cint", "Ref{CCentralResult}"] + ["Ptr{Cdouble}"] * 9)
    sig = re.search(r"^function central_reference\((.*?)\)\n", JL, re.S | re.M).group(1)
    assert re.search(r"\befficiency::Union\{Nothing, Tuple\{Vector\{Float64\}, Vector\{Float64\}\}\}=nothing", sig)
    body = JL[JL.index("function central_reference("):]
    guard, call = body.index("if efficiency !== nothing"), body.index(":dopf_central_solve_lossy")
    assert guard < call < body.index(":dopf_central_solve_ex")      # the lossy ccall sits in the keyword's branch, _ex in its else
    assert JL.count(":dopf_central_solve_lossy") == 1
