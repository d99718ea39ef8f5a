"""dopf_central_solve_coupled without a GPU: the header's prototype, the library's export, the ctypes and Julia signatures, the Python
functions on top, the refusals that need no device, and that the older entries' hosts go on refusing ramped, budgeted and rated
cases (the new entry is an addition, not a change)."""
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
ENTRY = "dopf_central_solve_coupled"
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
INVALID = -1
BASE_KEYS = ("N", "L", "T", "demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax", "sto_node")


def _proto(name):
    text = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    m = re.search(r"^int %s\(([^;]*?)\);" % name, text, re.M)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry_as_lossy_plus_the_coupling_arguments():
    lossy, coupled = _proto("dopf_central_solve_lossy"), _proto(ENTRY)
    new_in = ["const double *line_rating", "const double *gen_ramp_up", "const double *gen_ramp_down", "const double *gen_prev",
              "const double *gen_e_min", "const double *gen_e_max"]
    at = lossy.index("double tol")
    assert coupled == lossy[:at] + new_in + lossy[at:] + ["double *ramp_dual", "double *budget_dual"]
    # the older entries' sentences in the flag comments stand, with the new entry named next to them
    for flag, old in (("DOPF_F_LINE_RATING", "take no ratings"), ("DOPF_F_GEN_RAMP ", "ignore the flag"),
                      ("DOPF_F_GEN_RAMP_NETWORK", "ignore the flag"), ("DOPF_F2_GEN_ENERGY_BUDGET", "ignore the bit")):
        text = HDR[HDR.index("#define " + flag):]
        text = text[:text.index("*/")]
        assert old in text and ENTRY in text, flag


def test_library_exports_the_entry():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    assert hasattr(ctypes.CDLL(_capi.HIP_LIB_PATH), ENTRY)


def test_ctypes_signature_matches_the_header():
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    P = ctypes.POINTER
    f = api.central_solve_coupled
    want = {"const dopf_problem *": P(_capi.DopfProblem), "const dopf_params *": P(_capi.DopfParams), "const double *": DP, "double *": DP,
            "const int32_t *": IP, "int32_t": ctypes.c_int32, "double": ctypes.c_double, "dopf_central_result *": P(_capi.DopfCentralResult)}
    types = [want[re.sub(r"\w+$", "", a).strip()] for a in _proto(ENTRY)]
    assert f.restype is ctypes.c_int and list(f.argtypes) == types and len(types) == 30


def test_julia_shim_calls_the_entry_with_the_headers_types():
    m = re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint,\s*\(([^)]*)\)" % ENTRY, JL)
    assert m
    got = [a.strip() for a in m.group(1).split(",")]
    jl = {"const dopf_problem *": "Ref{CProblem}", "const dopf_params *": "Ref{CParams}", "const double *": "Ptr{Cdouble}",
          "double *": "Ptr{Cdouble}", "const int32_t *": "Ptr{Cint}", "int32_t": "Cint", "double": "Cdouble",
          "dopf_central_result *": "Ref{CCentralResult}"}
    assert got == [jl[re.sub(r"\w+$", "", a).strip()] for a in _proto(ENTRY)]
    assert re.search(r"^function central_reference_coupled\(nodes::Vector\{Node\}", JL, re.M)
    assert len(re.findall(r"ccall\(\(:%s," % ENTRY, JL)) == 1


def test_python_functions_exist_with_the_coupling_keywords():
    sig = inspect.signature(_capi.central_solve_coupled)
    for k in ("line_rating", "gen_ramp", "gen_prev", "gen_budget", "sto_eta", "gen_avail", "tol", "max_iters"):
        assert k in sig.parameters and sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    sig = inspect.signature(central.central_reference_coupled_on_device)
    for k in ("gen_ramp", "gen_prev", "gen_budget", "line_rating", "efficiency", "duals"):
        assert k in sig.parameters, k
    assert pkg.central_reference_coupled_on_device is central.central_reference_coupled_on_device
    nodes, lines, gens, stos = pkg.three_node_case()
    gens[0].quadratic_costs = 0.1
    with pytest.raises(ValueError, match="quadratic"):
        central.central_reference_coupled_on_device(nodes, gens, stos, lines)
    with pytest.raises(_capi.DopfError, match="quadratic"):
        _capi.central_solve_coupled(None, gen_c2=np.ones(4), **{k: v for k, v in pkg.pack(*_order(pkg.three_node_case())).engine_kwargs().items()
                                                               if k in BASE_KEYS})


def _order(case):
    nodes, lines, gens, stos = case
    return nodes, gens, stos, lines


def _raw(api, pp, *, up=None, down=None, tol=1e-7, max_iters=1000, fill=np.nan):
    kw = pp.engine_kwargs()
    prob, keep, G, S = _capi._problem(**{k: kw[k] for k in BASE_KEYS})
    q, res = _capi.default_params(), _capi.DopfCentralResult()
    sizes = (G * pp.T, S * pp.T, S * pp.T, S * pp.T, pp.T, pp.N * pp.T, pp.L * pp.T, pp.L * pp.T, pp.L * pp.T, G * pp.T, G)
    out = [np.full(n, fill) for n in sizes]
    dp = lambda a: None if a is None else a.ctypes.data_as(DP)
    rc = api.central_solve_coupled(ctypes.byref(prob), ctypes.byref(q), None, None, None, None, None, 0, None, None, None, dp(up), dp(down),
                                   None, None, None, tol, max_iters, ctypes.byref(res), *[dp(a) for a in out])
    msg = api.last_error(None)
    return rc, (msg.decode() if msg else ""), out, res


@pytest.mark.parametrize("what", ["only ramp_up", "only ramp_down", "tol of 0", "a negative tol", "a NaN tol", "max_iters of 0"])
def test_pairing_refusals_need_no_device(three_node, what, monkeypatch):
    """ramp_up without ramp_down, tol <= 0 and max_iters < 1 come before the temporary context: DOPF_E_INVALID with this entry's name
    whether or not a GPU is there (here none is visible to the call), and no output is written."""
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "-1")
    api = _capi.hip_api()
    pp = three_node[4]
    a = dict(up=np.full(pp.G, 5.0), down=np.full(pp.G, 5.0))
    if what == "only ramp_up":
        a["down"] = None
    elif what == "only ramp_down":
        a["up"] = None
    elif what == "tol of 0":
        a["tol"] = 0.0
    elif what == "a negative tol":
        a["tol"] = -1e-7
    elif what == "a NaN tol":
        a["tol"] = float("nan")
    else:
        a["max_iters"] = 0
    rc, msg, out, res = _raw(api, pp, **a)
    assert rc == INVALID and ENTRY in msg, (rc, msg)
    assert all(np.all(np.isnan(o)) for o in out)
    assert res.iterations == 0 and res.converged == 0


def test_the_older_hosts_still_refuse_coupled_cases(three_node):
    nodes, lines, gens, stos, pp = three_node
    base = {k: v for k, v in pp.engine_kwargs().items() if k in BASE_KEYS}
    with pytest.raises(_capi.DopfError, match="ramp"):
        _capi.central_solve(None, gen_ramp=(np.full(pp.G, 5.0), np.full(pp.G, 5.0)), **base)
    with pytest.raises(_capi.DopfError, match="ramp"):
        _capi.central_solve(None, gen_prev=np.zeros(pp.G), **base)
    with pytest.raises(_capi.DopfError, match="budget"):
        _capi.central_solve(None, gen_budget=(None, np.full(pp.G, 100.0)), **base)
    with pytest.raises(_capi.DopfError, match="no line ratings"):
        _capi.central_solve(None, line_rating=0.5 * np.asarray(pp.f_max)[:, None] * np.ones((pp.L, pp.T)), **base)
    for field, value, word in (("ramp_up", 5.0, "ramp"), ("energy_max", 300.0, "budget")):
        n2, l2, g2, s2 = pkg.three_node_case()
        setattr(g2[2], field, value)
        with pytest.raises(ValueError, match=word):
            central.central_reference_on_device(n2, g2, s2, l2)
    # ... and their messages point at the new function
    with pytest.raises(_capi.DopfError, match="central_solve_coupled"):
        _capi.central_solve(None, gen_prev=np.zeros(pp.G), **base)
