"""DOPF_F_LONG_HORIZON / DOPF_F_DEBUG_LONG_STO at the boundary: the header, the ctypes constants, the timing mirror and the
Julia shim agree. No compute calls (runs without a GPU)."""
import ctypes
import os
import re

from conftest import ROOT
from decentralopf_jl_amd import _capi

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()


def header_flags():
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+DOPF_F_(\w+)\s+(\d+)", HDR)}


def test_header_defines_the_long_horizon_flags_as_capi_does():
    f = header_flags()
    assert f["LONG_HORIZON"] == 1 << 21 == _capi.F_LONG_HORIZON
    assert f["DEBUG_LONG_STO"] == 1 << 22 == _capi.F_DEBUG_LONG_STO


def test_every_header_flag_is_one_bit_used_once():
    f = header_flags()
    vals = list(f.values())
    assert all(v > 0 and v & (v - 1) == 0 for v in vals), f
    assert len(set(vals)) == len(vals), f
    for name, v in f.items():                    # the ctypes module mirrors every one of them
        assert getattr(_capi, "F_" + name) == v, name


def test_timing_mirror_ends_with_sto_long():
    body = re.search(r"typedef struct dopf_timing \{(.*?)\} dopf_timing;", HDR, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(double|int32_t)\s+", "", " ".join(decl.split())).split(",")]
    assert names[-1] == "sto_long"
    assert [n for n, _ in _capi.DopfTiming._fields_] == names
    assert ctypes.sizeof(_capi.DopfTiming) == 8 * 8 + 8 * 4


def test_julia_shim_defines_the_long_horizon_flag():
    m = re.search(r"^const DOPF_F_LONG_HORIZON = (\d+)", JL, re.M)
    assert m and int(m.group(1)) == _capi.F_LONG_HORIZON
