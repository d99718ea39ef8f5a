"""dopf_get_generator_budget_price without a GPU: the header's two prototypes and what its text promises, the
library's exports, the bindings and the hosts' methods, the Julia shim, the refusal of an API without the entry, and where the prices
live: behind everything the two layouts held before them, every older offset in its place (a host-only build of
csrc/dopf_internal.h around tests/budget_price_layout_main.cpp prints the offsets), DevView at its size."""
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
INTERNAL = open(os.path.join(CSRC, "dopf_internal.h")).read()
DP = ctypes.POINTER(ctypes.c_double)


# ---- the header --------------------------------------------------------------------------------------------------------------------------

def test_header_declares_both_entries():
    assert re.search(r"^int dopf_get_generator_budget_price\(dopf_ctx \*ctx, double \*nu /\* G \*/\);$", HDR, re.M)
    assert re.search(r"^int dopf_multi_get_generator_budget_price\(dopf_multi \*m, double \*nu /\* G \*/\);$", HDR, re.M)
    # ... and no create-time flag came with them
    assert dict(re.findall(r"#define\s+(DOPF_F2_\w+)\s+(\d+)", HDR)) == {"DOPF_F2_GEN_ENERGY_BUDGET": "1", "DOPF_F2_GEN_RAMP_BUDGET": "8"}
    assert not re.search(r"#define\s+DOPF_F\w*(PRICE|WATER)", HDR)


def test_header_text_states_the_sign_the_lp_relation_and_the_status_rules():
    at = HDR.index("int dopf_get_generator_budget_price(")
    text = " ".join(HDR[HDR.rindex("/*", 0, at):at].replace(" * ", " ").split())
    for phrase in ("nu[g] > 0 where e_max held the row down", "nu[g] < 0 where e_min pushed it up", "nu[g] = 0 for a row with default budgets",
                   "whose search gave up", "dopf_solver_failures", "nu[g] = -budget_dual[g] of dopf_central_solve_coupled",
                   "wherever the LP's dual is unique", "the number the generator kernels add to gen_mc[g]", "last computed x-update",
                   "synchronises the context's stream", "while a trace is active", "Before the first iteration the values are zeros",
                   "dopf_set_generator_energy_budget, dopf_set_state, dopf_set_demand, dopf_roll_horizon_coupled",
                   "leave them alone", "halted context", "Recording is opt-in on a context without DOPF_F2_GEN_RAMP_BUDGET",
                   "until the FIRST call of this entry", "captured again at the next dopf_iterate", "and returns what is stored: zeros", "does not record the budget prices",
                   "multipliers of the ramp rows are not returned", "DOPF_E_UNSUPPORTED without DOPF_F2_GEN_ENERGY_BUDGET",
                   "DOPF_E_INVALID for a NULL pointer with G > 0", "with G == 0 the call returns DOPF_OK"):
        assert phrase in text, phrase
    at = HDR.index("int dopf_multi_get_generator_budget_price(")
    text = " ".join(HDR[HDR.rindex("/*", 0, at):at].replace(" * ", " ").split())
    assert "caller's order" in text and "dopf_multi_get_primal" in text


# ---- the library, the bindings, the hosts ------------------------------------------------------------------------------------------------

def test_library_exports_the_entries_and_the_argtypes_match():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    assert hasattr(lib, "dopf_get_generator_budget_price") and hasattr(lib, "dopf_multi_get_generator_budget_price")
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for name in ("get_generator_budget_price", "multi_get_generator_budget_price"):
        f = getattr(api, name)
        assert f.restype is ctypes.c_int and list(f.argtypes) == [ctypes.c_void_p, DP], name


def test_the_four_hosts_have_the_method():
    for cls in (_capi.Engine, _capi.MultiEngine, admm.ADMM, sharded.ShardedADMM):
        assert callable(getattr(cls, "budget_price")), cls
        assert "budget" in getattr(cls, "budget_price").__doc__


def test_julia_shim_has_the_getter_and_both_ccalls():
    assert re.search(r"^function budget_price\(admm::ADMM\)", JL, re.M)
    for name in ("dopf_get_generator_budget_price", "dopf_multi_get_generator_budget_price"):
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cdouble\}\)" % name, JL), name
    doc = JL[JL.index("    budget_price(admm)"):JL.index("function budget_price")]
    assert "DOPF_F2_GEN_ENERGY_BUDGET" in doc and "-budget_dual" in doc and "`> 0` where `e_max`" in doc


def test_an_api_without_the_entry_refuses_with_a_clear_text(three_node, oracle_api):
    pp = three_node[4]
    assert not hasattr(oracle_api, "get_generator_budget_price") and not hasattr(oracle_api, "multi_get_generator_budget_price")
    e = _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, **pp.engine_kwargs())
    with pytest.raises(_capi.DopfError) as err:
        e.budget_price()
    assert str(err.value) == "oracle_*: this API has no get_generator_budget_price"
    m = _capi.MultiEngine.__new__(_capi.MultiEngine)              # (no device: the method looks at the API before anything else)
    m.api, m.G = oracle_api, pp.G
    with pytest.raises(_capi.DopfError) as err:
        m.budget_price()
    assert str(err.value) == "oracle_*: this API has no multi_get_generator_budget_price"


def test_sharded_budget_price_places_the_ranks_slice_and_sums():
    """ShardedADMM.budget_price without a device: the rank's slice in a vector of zeros, handed to the caller's sum"""
    class Shard:
        meta = {"gen_range": (2, 5)}

    class Engine:
        def budget_price(self):
            return np.array([1.5, -0.0, -2.0])
    sh = sharded.ShardedADMM.__new__(sharded.ShardedADMM)
    sh.shard, sh.engine, sh.world, sh._tensor = Shard(), Engine(), 2, None
    sh.problem = type("P", (), {"G": 6})()
    seen = []
    out = sh.budget_price(all_reduce=lambda x: (seen.append(x.copy()), x + np.array([7.0, 8.0, 0, 0, 0, 9.0]))[1])
    assert np.array_equal(seen[0], [0, 0, 1.5, 0, -2.0, 0]) and np.array_equal(out, [7.0, 8.0, 1.5, 0.0, -2.0, 9.0])
    with pytest.raises(ValueError, match="all_reduce"):
        sh.budget_price()
    sh.world = 1
    assert np.array_equal(sh.budget_price(), [0, 0, 1.5, 0, -2.0, 0])


# ---- where the prices live ---------------------------------------------------------------------------------------------------------------

def test_only_the_price_and_the_floor_sit_behind_a_scratch():
    """every pointer accessor of dopf_internal.h whose place depends on a scratch's size: those two and no other"""
    behind = set()
    for m in re.finditer(r"inline (?:const )?double \*(\w+)\(const DevView &v[^)]*\)\s*\{(.*?)\n?\}", INTERNAL, re.S):
        name, body = m.groups()
        if re.search(r"scratch_doubles\(|wave_doubles\(|row_doubles\(", body):
            behind.add(name)
    assert behind == {"gen_min_output", "gen_budget_price"}, behind
    assert 'static_assert(sizeof(DevView) == 832, "DevView must keep its size");' in INTERNAL
    # the host states the layout in one place: the context's accessor takes it from the plan, and dopf_api.hip goes through it
    ctx = open(os.path.join(CSRC, "dopf_ctx.h")).read()
    assert "double *gen_budget_price_d() const { return dopf::gen_budget_price(v, plan.genRampBudget); }" in ctx
    api = open(os.path.join(CSRC, "dopf_api.hip")).read()
    # ... and the store is an instantiation of its own, switched by the getter alone: plan_chain never sets it
    plan = open(os.path.join(CSRC, "dopf_plan.h")).read()
    assert "bool genBudgetPrice;" in plan and plan.count("genBudgetPrice") == 1
    assert api.count("c->plan.genBudgetPrice = true;") == 1 and "with_bool(p.genBudgetPrice" in open(os.path.join(CSRC, "gen_budget.h")).read()
    assert api.count("gen_budget_price_d()") == 2 and "gen_budget_price(" not in api.replace("dopf_get_generator_budget_price(", "")


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("layout") / "budget_price_layout")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O0", "-Wno-unused-value", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "budget_price_layout_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return [line.split() for line in r.stdout.splitlines()]


def test_the_prices_sit_behind_both_layouts_and_every_older_offset_stays(layout):
    wave = lambda T: T + 64 * (5 * T + 4)                        # ramp_budget_wave_doubles: c[T] | 64 x ramp_row_doubles(T)
    seen = {"budget": 0, "pair": 0, "ramp": 0, "view": 0}
    for row in layout:
        kind, num = row[0], [int(x) for x in row[1:]]
        seen[kind] += 1
        if kind == "view":
            assert num == [832]
        elif kind == "budget":
            G, T, items, lo, hi, price, total = num
            assert (lo, hi, price, total) == (G, 2 * G, 3 * G, 4 * G)
        elif kind == "pair":
            G, T, items, up, down, prev, lo, hi, scratch, price, total = num
            assert (up, down, prev, lo, hi, scratch) == (G, 2 * G, 3 * G, 4 * G, 5 * G, 6 * G)
            assert price == 6 * G + items * 8 * wave(T) and total == price + G
        else:
            G, T, items, L, up, down, prev, scratch, floor, total = num
            assert (up, down, prev, scratch) == (G, 2 * G, 3 * G, 4 * G)
            assert floor == total - G and floor >= 4 * G            # behind the scratch, the last G doubles of the block
            if L == 0:
                assert floor == 4 * G + (items * 8 * (5 * T + 4) if T > 128 else 0)
    assert seen["view"] == 1 and min(seen.values()) >= 1 and seen["budget"] == seen["pair"] == seen["ramp"] >= 5
