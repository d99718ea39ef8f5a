"""dopf_get_generator_ramp_price without a GPU: the header's two prototypes and what its text promises, the library's
exports, the bindings and the hosts' methods, the Julia shim, the refusal of an API without the entry, that no create-time flag came
with it, and that nothing of the gen_pmax block or of DevView moved: the prices live in an array of the context's own, which reaches
the kernels as their second argument (tests/budget_price_layout_main.cpp must print what it printed before this entry:
tests/golden/gen_pmax_layout.txt)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from decentralopf_jl_amd import _capi, admm, sharded

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
DP = ctypes.POINTER(ctypes.c_double)
FLAGS = """DOPF_F_NO_GRAPH DOPF_F_OVERLAP_AGENTS DOPF_F_NO_ROW_SKIP DOPF_F_NO_WARM_START DOPF_F_NO_FUSE DOPF_F_COMM_HOST DOPF_F_KEEP_DELTAS
DOPF_F_COMM_GRAPH DOPF_F_COMM_P2P DOPF_F_NO_TAIL_FUSE DOPF_F_TIME_CALLS DOPF_F_STO_GENERAL DOPF_F_NO_QUIET DOPF_F_XCHG_OWNER
DOPF_F_XCHG_ALLGATHER DOPF_F_NO_TAIL_XCHG DOPF_F_NET_SMALL_ITEMS DOPF_F_PERSIST DOPF_F_LONG_HORIZON DOPF_F_WIDE_NETWORK
DOPF_F_STO_INITIAL_LEVEL DOPF_F_STO_TERMINAL_LEVEL DOPF_F_GEN_AVAILABILITY DOPF_F_STO_EFFICIENCY DOPF_F_LINE_RATING
DOPF_F_GEN_QUADRATIC_COST DOPF_F_GEN_RAMP DOPF_F_GEN_RAMP_NETWORK DOPF_F2_GEN_ENERGY_BUDGET DOPF_F2_GEN_RAMP_BUDGET DOPF_F_DEBUG_LEAVE
DOPF_F_DEBUG_ROOT_CAP DOPF_F_DEBUG_LONG_STO DOPF_F_DEBUG_WIDE_NET""".split()


# ---- the header --------------------------------------------------------------------------------------------------------------------------

def test_header_declares_both_entries_and_no_flag():
    assert re.search(r"^int dopf_get_generator_ramp_price\(dopf_ctx \*ctx, double \*rp /\* T\*G, \[t \+ T\*g\] \*/\);$", HDR, re.M)
    assert re.search(r"^int dopf_multi_get_generator_ramp_price\(dopf_multi \*m, double \*rp /\* T\*G, \[t \+ T\*g\] \*/\);$", HDR, re.M)
    assert re.findall(r"#define\s+(DOPF_F\w+)", HDR) == FLAGS


def test_header_text_states_the_sign_the_lp_relation_and_the_status_rules():
    at = HDR.index("int dopf_get_generator_ramp_price(")
    text = " ".join(HDR[HDR.rindex("/*", 0, at):at].replace(" * ", " ").split())
    for phrase in ("rp[t + T*g] is the multiplier the last computed x-update put on generator g's ramp row", "t = 0: the anchor's row",
                   "0 without an anchor", "in the unit of gen_mc", "caller's generator order", "rp > 0 where ramp-up held the unit back",
                   "rp < 0 where ramp-down held it up", "whose clamped step kept its ramps", "whose pair search gave up",
                   "rp = -ramp_dual of dopf_central_solve_coupled", "wherever the LP's dual is unique", "the sign rule of the budget price",
                   "On a DOPF_F2_GEN_RAMP_BUDGET context it is the ramp rows' multiplier under that row's nu", "dopf_set_generator_min_output",
                   "Recording is opt-in", "the FIRST call of this entry allocates T*G doubles", "DOPF_E_NOMEM, naming the bytes",
                   "captured again at the next dopf_iterate", "and returns what is stored: zeros", "there is no way back",
                   "a floor set afterwards keeps the context recording", "A context that never calls the entry runs the kernels of before",
                   "dopf_set_state, dopf_set_demand, dopf_roll_horizon_coupled", "leave them alone", "halted context",
                   "Before the first iteration the values are zeros", "while a trace is active", "communicator or a peer exchange",
                   "DOPF_E_UNSUPPORTED without DOPF_F_GEN_RAMP", "with L > 0: network rows are not priced",
                   "DOPF_E_INVALID for a NULL pointer with G > 0", "with G == 0 the call returns DOPF_OK"):
        assert phrase in text, phrase
    at = HDR.index("int dopf_multi_get_generator_ramp_price(")
    text = " ".join(HDR[HDR.rindex("/*", 0, at):at].replace(" * ", " ").split())
    assert "caller's order" in text and "dopf_multi_get_primal" in text


# ---- the library, the bindings, the hosts ------------------------------------------------------------------------------------------------

def test_library_exports_the_entries_and_the_argtypes_match():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    assert hasattr(lib, "dopf_get_generator_ramp_price") and hasattr(lib, "dopf_multi_get_generator_ramp_price")
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for name in ("get_generator_ramp_price", "multi_get_generator_ramp_price"):
        f = getattr(api, name)
        assert f.restype is ctypes.c_int and list(f.argtypes) == [ctypes.c_void_p, DP], name


def test_the_four_hosts_have_the_method():
    for cls in (_capi.Engine, _capi.MultiEngine, admm.ADMM, sharded.ShardedADMM):
        assert callable(getattr(cls, "ramp_price")), cls
        assert "ramp" in getattr(cls, "ramp_price").__doc__


def test_julia_shim_has_the_getter_and_both_ccalls():
    assert re.search(r"^function ramp_price\(admm::ADMM\)", JL, re.M)
    for name in ("dopf_get_generator_ramp_price", "dopf_multi_get_generator_ramp_price"):
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cdouble\}\)" % name, JL), name
    doc = JL[JL.index("    ramp_price(admm)"):JL.index("function ramp_price")]
    assert "DOPF_F_GEN_RAMP" in doc and "-ramp_dual" in doc and "`> 0` where\n`ramp_up`" in doc and "`G x T`" in doc
    body = JL[JL.index("function ramp_price"):]
    assert "permutedims(reshape(out, T, G))" in body[:body.index("\nend\n")]     # the ABI's [t + T*g] as a G x T matrix


def test_an_api_without_the_entry_refuses_with_a_clear_text(three_node, oracle_api):
    pp = three_node[4]
    assert not hasattr(oracle_api, "get_generator_ramp_price") and not hasattr(oracle_api, "multi_get_generator_ramp_price")
    e = _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, **pp.engine_kwargs())
    with pytest.raises(_capi.DopfError) as err:
        e.ramp_price()
    assert str(err.value) == "oracle_*: this API has no get_generator_ramp_price"
    m = _capi.MultiEngine.__new__(_capi.MultiEngine)              # (no device: the method looks at the API before anything else)
    m.api, m.G, m.T = oracle_api, pp.G, pp.T
    with pytest.raises(_capi.DopfError) as err:
        m.ramp_price()
    assert str(err.value) == "oracle_*: this API has no multi_get_generator_ramp_price"


def test_sharded_ramp_price_places_the_ranks_rows_and_sums():
    """ShardedADMM.ramp_price without a device: the rank's rows in an array of zeros, handed to the caller's sum"""
    class Shard:
        meta = {"gen_range": (1, 3)}

    class Engine:
        def ramp_price(self):
            return np.array([[1.5, -0.0], [-2.0, 0.25]])
    sh = sharded.ShardedADMM.__new__(sharded.ShardedADMM)
    sh.shard, sh.engine, sh.world, sh._tensor = Shard(), Engine(), 2, None
    sh.problem = type("P", (), {"G": 4})()
    seen = []
    other = np.array([[7.0, 8.0], [0, 0], [0, 0], [9.0, 1.0]])
    out = sh.ramp_price(all_reduce=lambda x: (seen.append(x.copy()), x + other)[1])
    assert np.array_equal(seen[0], [[0, 0], [1.5, 0], [-2.0, 0.25], [0, 0]])
    assert np.array_equal(out, [[7.0, 8.0], [1.5, 0], [-2.0, 0.25], [9.0, 1.0]])
    with pytest.raises(ValueError, match="all_reduce"):
        sh.ramp_price()
    sh.world = 1
    assert np.array_equal(sh.ramp_price(), seen[0])


# ---- where the prices live ---------------------------------------------------------------------------------------------------------------

def test_the_pass_is_plain_cpp_and_the_plan_entry_is_the_getters_alone():
    src = open(os.path.join(CSRC, "ramp_price.h")).read()
    assert "#include" not in src                                                          # no HIP include, nor any other
    assert "#pragma clang fp contract(off)" in src
    plan = open(os.path.join(CSRC, "dopf_plan.h")).read()
    assert "double *genRampPrice;" in plan and plan.count("genRampPrice") == 1           # plan_chain never sets it
    api = open(os.path.join(CSRC, "dopf_api.hip")).read()
    assert api.count("c->plan.genRampPrice = ") == 1
    for name, kernel in (("gen_ramp.h", "k_gen_ramp"), ("gen_ramp_budget.h", "k_gen_ramp_budget")):
        text = open(os.path.join(CSRC, name)).read()
        assert "with_bool(p.genRampPrice != nullptr" in text and re.search(r"bool RP>\n__global__[^\n]*void %s\(DevView v, double \*rpv\)" % kernel, text)
    internal = open(os.path.join(CSRC, "dopf_internal.h")).read()
    assert 'static_assert(sizeof(DevView) == 832, "DevView must keep its size");' in internal
    assert "ramp_price" not in internal                                                  # no accessor, no offset: the block is as it was


def test_the_gen_pmax_block_is_where_it_was(tmp_path):
    """the layout program of tests/test_gen_budget_price_abi.py prints what it printed on the commit before this entry"""
    exe = str(tmp_path / "layout")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O0", "-Wno-unused-value", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "budget_price_layout_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    assert r.stdout == open(os.path.join(ROOT, "tests", "golden", "gen_pmax_layout.txt")).read()
    assert ["view", "832"] in [ln.split() for ln in r.stdout.splitlines()]
