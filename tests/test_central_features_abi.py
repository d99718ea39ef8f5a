"""dopf_central_solve_ex (the device LP with storage initial levels, terminal bands and generator availability) at the boundary: the
header, the export, the ctypes signature, the Python host's keywords and the Julia shim. No compute calls on a device (runs
without a GPU)."""
import ctypes
import inspect
import os
import re

from conftest import ROOT
from decentralopf_jl_amd import _capi, central

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
FEATURE_KW = ("sto_e0", "sto_end_lo", "sto_end_hi", "gen_avail", "gen_avail_of")


def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry_with_flat_arguments():
    outs = ["double *P", "double *D", "double *C", "double *E", "double *system_price", "double *nodal_price",
            "double *line_utilization", "double *flow_upper_dual", "double *flow_lower_dual"]
    assert _prototype("dopf_central_solve_ex") == (
        ["const dopf_problem *p", "const dopf_params *q", "const double *sto_e0", "const double *sto_end_lo",
         "const double *sto_end_hi", "int32_t n_profiles", "const double *profiles", "const int32_t *profile_of",
         "double tol", "int32_t max_iters", "dopf_central_result *res"] + outs)
    # the entry without the inputs keeps its prototype
    assert _prototype("dopf_central_solve") == (["const dopf_problem *p", "const dopf_params *q", "double tol", "int32_t max_iters",
                                                 "dopf_central_result *res"] + outs)


def test_library_exports_the_entry():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    assert hasattr(lib, "dopf_central_solve_ex") and hasattr(lib, "dopf_central_solve")


def test_ctypes_signature_matches_the_header():
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    f = api.central_solve_ex
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == ([ctypes.POINTER(_capi.DopfProblem), ctypes.POINTER(_capi.DopfParams), dp, dp, dp, ctypes.c_int32,
                                 dp, ip, ctypes.c_double, ctypes.c_int32, ctypes.POINTER(_capi.DopfCentralResult)] + [dp] * 9)
    assert len(f.argtypes) == len(_prototype("dopf_central_solve_ex"))


def test_python_host_accepts_the_inputs_engine_kwargs_emits():
    par = inspect.signature(_capi.central_solve).parameters
    for k in FEATURE_KW:
        assert k in par and par[k].default is None and par[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    par = inspect.signature(central.central_reference_on_device).parameters
    ref = inspect.signature(central.central_reference).parameters
    for k in ("initial_level", "terminal_level"):
        assert k in par and par[k].default is None and k in ref, k


def test_every_engine_kwarg_of_a_featured_case_is_a_central_solve_keyword():
    """What used to raise TypeError: a packed case with an initial level, a band and a profile, handed over as engine_kwargs()."""
    import numpy as np
    from conftest import pkg
    nodes, lines, gens, stos = pkg.three_node_case()
    gens[0].availability = [1.0, 0.875]
    stos[0].initial_level = 5.0
    stos[0].terminal_level_min = 5.0
    kw = pkg.pack(nodes, gens, stos, lines).engine_kwargs()
    assert set(FEATURE_KW) <= set(kw)
    assert set(kw) <= set(inspect.signature(_capi.central_solve).parameters)
    assert np.asarray(kw["gen_avail"]).shape == (1, 2)


def test_julia_shim_calls_both_entries():
    assert re.search(r"ccall\(\(:dopf_central_solve, DOPF_LIB\), Cint,", JL)
    m = re.search(r"ccall\(\(:dopf_central_solve_ex, DOPF_LIB\), Cint,\s*\(([^)]*)\)", JL)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == (["Ref{CProblem}", "Ref{CParams}", "Ptr{Cdouble}", "Ptr{Cdouble}", "Ptr{Cdouble}", "Cint", "Ptr{Cdouble}", "Ptr{Cint}",
                     "Cdouble", "Cint", "Ref{CCentralResult}"] + ["Ptr{Cdouble}"] * 9)
    sig = re.search(r"^function central_reference\((.*?)\)\n", JL, re.S | re.M).group(1)
    for k in ("initial_level", "terminal_level", "availability"):
        assert re.search(r"\b%s::Union\{Nothing, " % k, sig), k
