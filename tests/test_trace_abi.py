"""dopf_trace_*  without a GPU: the header declares the five entries and the three constants, the library exports
them, the ctypes signatures say what the header says, the Julia shim calls them, and run_recorded refuses what a trace cannot
record before it touches a device."""
import ctypes
import os
import re

import pytest

from conftest import ROOT, build_oracle
from decentralopf_jl_amd import ADMM, _capi, run_recorded
from decentralopf_jl_amd.network import Generator, Node, Storage

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
ENTRIES = ("trace_begin", "trace_end", "trace_reset", "trace_info", "trace_read")
C2CTYPES = {"dopf_ctx*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int32_t*": _capi.c_int32_p, "double*": _capi.c_double_p}


def header_args(name):
    text = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    m = re.search(r"^int\s+dopf_%s\s*\(([^;{]*?)\)\s*;" % name, text, re.M)
    assert m, name
    out = []
    for a in " ".join(m.group(1).split()).split(","):
        mm = re.match(r"([\w]+)\s*(\**)\s*\w*$", a.strip())
        assert mm, (name, a)
        out.append(mm.group(1) + mm.group(2))
    return out


def test_header_declares_the_entries_and_the_constants():
    for name, value in (("DOPF_TRACE_DUALS", 1), ("DOPF_TRACE_CONSENSUS", 2), ("DOPF_TRACE_PRIMAL", 4)):
        assert re.search(r"^#define %s\s+%d\b" % (name, value), HDR, re.M), name
    assert header_args("trace_begin") == ["dopf_ctx*", "int32_t", "int32_t"]
    assert header_args("trace_end") == ["dopf_ctx*"] and header_args("trace_reset") == ["dopf_ctx*"]
    assert header_args("trace_info") == ["dopf_ctx*"] + ["int32_t*"] * 4
    assert header_args("trace_read") == ["dopf_ctx*", "int32_t", "int32_t", "double*", "int32_t*", "int32_t*"] + ["double*"] * 11
    # only the argument types the Julia shim's type table knows
    for e in ENTRIES:
        assert set(header_args(e)) <= set(C2CTYPES), e


def test_library_exports_them_and_the_binding_says_what_the_header_says():
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    api = _capi.CApi(_capi.HIP_LIB_PATH, "dopf_")
    for e in ENTRIES:
        assert hasattr(lib, "dopf_" + e), e
        fn = getattr(api, e)
        assert fn.restype == ctypes.c_int
        assert fn.argtypes == [C2CTYPES[t] for t in header_args(e)], e
    assert (_capi.TRACE_DUALS, _capi.TRACE_CONSENSUS, _capi.TRACE_PRIMAL, _capi.TRACE_ALL) == (1, 2, 4, 7)
    for m in ("trace_begin", "trace_end", "trace_reset", "trace_info", "trace_read"):
        assert callable(getattr(_capi.Engine, m))


def test_julia_shim_has_the_constants_the_ccalls_and_run_recorded():
    for name, value in (("DOPF_TRACE_DUALS", 1), ("DOPF_TRACE_CONSENSUS", 2), ("DOPF_TRACE_PRIMAL", 4)):
        assert re.search(r"^const %s = %d\b" % (name, value), JL, re.M), name
    for e in ENTRIES:
        assert re.search(r"ccall\(\(:dopf_%s, DOPF_LIB\), Cint," % e, JL), e
    assert re.search(r"^function run_recorded!\(admm::ADMM; chunk::Int=64\)", JL, re.M)
    body = JL.split("function run_recorded!(admm::ADMM", 1)[1].split("\nend\n", 1)[0]
    assert "admm.record || error" in body and "finally" in body and ":dopf_trace_end" in body.split("finally", 1)[1]
    assert "DOPF_TRACE_DUALS | DOPF_TRACE_CONSENSUS | DOPF_TRACE_PRIMAL" in body


class NoDevice:
    """an engine that fails the test at the first call of any kind"""

    def __getattr__(self, name):
        raise AssertionError(f"run_recorded touched the engine ({name}) before refusing")


def little(**kw):
    from oracle.binding import OracleApi
    n = Node("N", [60.0, 70.0, 80.0], True)
    gens = [Generator("a", 3, 50, "x", n), Generator("b", 30, 100, "x", n)]
    stos = [Storage("s", 1, 10, 20, "x", n)]
    admm = ADMM(0.3, [n], gens, stos, [], backend=OracleApi(build_oracle()), backend_mode=1, max_iters=5, **kw)
    real = admm.engine
    admm.engine = NoDevice()
    return admm, real


def test_run_recorded_refuses_before_any_device_call():
    admm, _ = little(record=False)
    with pytest.raises(ValueError, match="record=True"):
        run_recorded(admm)
    admm, _ = little(record=True)
    admm.record_slacks = True
    with pytest.raises(ValueError, match="record_slacks"):
        run_recorded(admm)
    admm.record_slacks = False
    with pytest.raises(ValueError, match="chunk"):
        run_recorded(admm, chunk=0)


def test_run_recorded_on_a_backend_without_the_entries_says_so():
    admm, real = little(record=True)
    admm.engine = real
    with pytest.raises(_capi.DopfError, match="no trace"):
        run_recorded(admm)
    assert admm.results == [] and len(admm.lambdas) == 1
