"""dopf_roll_horizon_coupled / dopf_get_generator_coupling without a GPU: the library exports both and the bindings
say what the header says, horizon.shift_coupled — the rule in NumPy, which the device is tested against — entry by entry on a
hand-made P, Engine.roll's routing on an API that has the new entry (unchanged: the host route for ramp and budget contexts), and
the Julia shim's two functions."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from decentralopf_jl_amd import _capi, horizon, shift_coupled

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
LIB = _capi.HIP_LIB_PATH

C2CTYPES = {"dopf_ctx*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "double*": ctypes.POINTER(ctypes.c_double),
            "int32_t*": ctypes.POINTER(ctypes.c_int32)}


def header_args(name):
    """the C argument types of a prototype in include/dopf.h (comments, const and parameter names stripped, '*' attached)"""
    text = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    m = re.search(r"^\s*int\s+%s\s*\(([^;{]*?)\)\s*;" % name, text, re.M)
    assert m, f"{name} is not declared in include/dopf.h"
    out = []
    for a in " ".join(m.group(1).split()).split(","):
        mm = re.match(r"([\w]+)\s*(\**)\s*\w*$", a.strip().replace("const ", ""))
        assert mm, (name, a)
        out.append(mm.group(1) + mm.group(2))
    return out


def test_the_library_exports_both_entries_and_the_bindings_match_the_header():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "dopf_roll_horizon_coupled") and hasattr(lib, "dopf_get_generator_coupling")
    api = _capi.CApi(LIB)
    for name in ("roll_horizon_coupled", "get_generator_coupling"):
        fn = getattr(api, name)
        want = [C2CTYPES[t] for t in header_args("dopf_" + name)]
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want, (name, fn.argtypes, want)
    assert len(header_args("dopf_roll_horizon_coupled")) == 9 and len(header_args("dopf_get_generator_coupling")) == 6
    # the older entry's prototype is as it was, and its comment and the two flags' point to the new one
    assert header_args("dopf_roll_horizon") == ["dopf_ctx*", "int32_t", "double*"]
    for start in ("#define DOPF_F_GEN_RAMP ", "#define DOPF_F2_GEN_ENERGY_BUDGET", "#define DOPF_F2_GEN_RAMP_BUDGET", "/* dopf_roll_horizon:"):
        text = HDR[HDR.index(start):]
        assert "dopf_roll_horizon_coupled" in text[:text.index("*/")], start


def test_a_null_context_is_invalid():
    """(no device is touched: both entries look at the context first)"""
    api = _capi.CApi(LIB)
    assert api.roll_horizon_coupled(None, 1, None, -1, None, None, 0, None, None) == -1
    assert api.get_generator_coupling(None, None, None, None, None, None) == -1


# ---- horizon.shift_coupled -------------------------------------------------------------------------------------------------------

# distinct entries, none of them a sum of others in binary; row 1's sums are not exact in double, so the order of the sum shows
P_HAND = np.array([[1.0, 2.5, 4.25, 8.125, 16.0625],
                   [0.1, 0.7, 1e16, -1e16 + 2.0, 0.3],
                   [3.0, 5.0, 7.0, 11.0, 13.0]])
LO_HAND = np.array([0.5, 0.25, 2.0])
HI_HAND = np.array([np.inf, 40.0, 7.0])           # row 0: no upper bound; row 2 goes negative before the floor from k = 2 on


@pytest.mark.parametrize("k", [1, 2, 4])
def test_shift_coupled_entry_by_entry(k):
    assert shift_coupled is horizon.shift_coupled
    out = shift_coupled(k, P_HAND, budget=(LO_HAND, HI_HAND))
    assert set(out) == {"gen_prev", "gen_budget"}
    lo, hi = out["gen_budget"]
    for g in range(3):
        assert out["gen_prev"][g] == P_HAND[g, k - 1]
        spent = float(P_HAND[g, 0])
        for t in range(1, k):                     # left to right from P[g, 0]
            spent = spent + float(P_HAND[g, t])
        assert lo[g] == max(0.0, float(LO_HAND[g]) - spent) and hi[g] == max(0.0, float(HI_HAND[g]) - spent), (g, k)
    assert hi[0] == np.inf                        # +inf stays +inf
    if k >= 2:
        assert HI_HAND[2] - P_HAND[2, :k].sum() < 0.0 and hi[2] == 0.0 and lo[2] == 0.0          # floored
    if k == 4:                                    # the order matters here: 0.1 + 0.7 is lost in 1e16, another order keeps it
        assert lo[1] == 0.0 and hi[1] == 40.0 - ((0.1 + 0.7 + 1e16) + (-1e16 + 2.0))
        assert ((0.1 + 0.7) + (1e16 + (-1e16 + 2.0))) != ((0.1 + 0.7 + 1e16) + (-1e16 + 2.0))
    assert out["gen_prev"] is not P_HAND and not np.shares_memory(out["gen_prev"], P_HAND)


def test_shift_coupled_without_budgets_and_with_defaults():
    assert set(shift_coupled(2, P_HAND)) == {"gen_prev"}
    lo, hi = shift_coupled(2, P_HAND, budget=(None, None))["gen_budget"]
    assert np.array_equal(lo, np.zeros(3)) and np.all(hi == np.inf)
    for k in (0, 5):
        with pytest.raises(ValueError, match="outside"):
            shift_coupled(k, P_HAND)


# ---- Engine.roll's routing -------------------------------------------------------------------------------------------------------

class HostRoute(Exception):
    pass


class FakeApi:
    """an API object that has every roll entry (no library, no device): it records which one Engine.roll calls"""
    prefix = "dopf_"

    def __init__(self):
        self.calls = []

    def roll_horizon(self, ctx, k, tail):
        self.calls.append("roll_horizon")
        return 0

    def roll_horizon_coupled(self, *args):
        self.calls.append("roll_horizon_coupled")
        return 0

    def get_generator_coupling(self, *args):
        self.calls.append("get_generator_coupling")
        return 0


def fake_engine(flags, flags2):
    e = object.__new__(_capi.Engine)
    e.api, e.N, e.L, e.T, e.G, e.S = FakeApi(), 2, 0, 4, 3, 0
    e.params, e.flags2 = _capi.default_params(flags=flags), flags2
    e._keep, e._mirror, e._mode, e._ctx = dict(demand=np.zeros(8)), {}, None, ctypes.c_void_p()

    def host_route():
        raise HostRoute()
    e.get_primal = host_route                    # the host route's first step
    return e


@pytest.mark.parametrize("flags,flags2", [(_capi.F_GEN_RAMP, 0), (0, _capi.F2_GEN_ENERGY_BUDGET),
                                          (_capi.F_GEN_RAMP, _capi.F2_GEN_ENERGY_BUDGET | _capi.F2_GEN_RAMP_BUDGET)])
def test_engine_roll_keeps_the_host_route_for_ramp_and_budget_contexts(flags, flags2):
    e = fake_engine(flags, flags2)
    with pytest.raises(HostRoute):
        e.roll(1, np.ones((2, 1)))
    assert e.api.calls == []                     # neither native entry


def test_engine_roll_takes_the_native_entry_without_the_flags():
    e = fake_engine(0, 0)
    e.roll(1, np.ones((2, 1)))
    assert e.api.calls == ["roll_horizon"]
    assert np.array_equal(e.demand(), np.concatenate([np.zeros((2, 3)), np.ones((2, 1))], axis=1))


def test_engine_roll_coupled_calls_the_entry_and_refreshes_the_mirrors():
    e = fake_engine(_capi.F_GEN_RAMP, _capi.F2_GEN_ENERGY_BUDGET)
    e._mirror["line_rating"] = np.arange(8.0).reshape(2, 4)
    e.roll_coupled(1, np.ones((2, 1)), availability=(np.full((1, 4), 0.5), np.zeros(3, dtype=np.int32)))
    assert e.api.calls == ["roll_horizon_coupled", "get_generator_coupling"]
    assert {"gen_prev", "gen_budget", "gen_avail", "gen_avail_of"} <= set(e._mirror)
    assert np.array_equal(e._mirror["gen_avail"], np.full((1, 4), 0.5)) and e._mirror["gen_avail_of"].tolist() == [0, 0, 0]
    assert np.array_equal(e._mirror["line_rating"], np.array([[1.0, 2.0, 3.0, 3.0], [5.0, 6.0, 7.0, 7.0]]))
    assert np.array_equal(e.demand()[:, -1], np.ones(2))


def test_engine_roll_coupled_needs_the_entry():
    e = fake_engine(_capi.F_GEN_RAMP, 0)
    e.api = type("Old", (), {"prefix": "dopf_", "roll_horizon": None})()
    with pytest.raises(_capi.DopfError, match="no roll_horizon_coupled"):
        e.roll_coupled(1, np.ones((2, 1)))


def test_admm_has_the_thin_wrapper():
    from decentralopf_jl_amd import ADMM
    assert callable(ADMM.roll_coupled) and callable(ADMM.roll)


# ---- the Julia shim --------------------------------------------------------------------------------------------------------------

def test_the_julia_shim_names_both_functions():
    assert re.search(r"^function roll_horizon_coupled!\(admm::ADMM, k::Int, demand_tail::Matrix\{Float64\}; availability=nothing, budget=nothing\)", JL, re.M)
    assert re.search(r"^function generator_coupling\(admm::ADMM\)", JL, re.M)
    assert ":dopf_roll_horizon_coupled, DOPF_LIB" in JL and ":dopf_get_generator_coupling, DOPF_LIB" in JL
    for fn in ("roll_horizon_coupled!", "generator_coupling"):
        body = JL[JL.index("function " + fn):]
        assert "one GPU only" in body[:body.index("\nend\n")], fn
