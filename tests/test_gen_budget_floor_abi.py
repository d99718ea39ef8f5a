"""dopf_set_generator_budget_min_output without a GPU: the header's three prototypes and their comment, the library's
exports and the bindings' argtypes, no new flag and no new row of the extension tables, the plan entry, the hosts' methods, the Julia
shim's ccalls, and the packed problem's field on its way to the engines and the shards."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from decentralopf_jl_amd import _capi, admm, central, sharded

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
DP, VP = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p

ENTRIES = {"set_generator_budget_min_output": ("dopf_ctx *", "const double *"),
           "get_generator_budget_min_output": ("dopf_ctx *", "double *"),
           "multi_set_generator_budget_min_output": ("dopf_multi *", "const double *")}


def test_header_declares_the_three_entries():
    for name, want in ENTRIES.items():
        m = re.search(r"^int dopf_%s\((.*?)\);" % name, HDR, re.M | re.S)
        assert m, name
        args = [re.sub(r"\w+$", "", a.strip()).strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        assert tuple(args) == want, (name, args)


def test_no_flag_came_with_the_entries_and_the_tables_are_unchanged():
    assert dict(re.findall(r"#define\s+(DOPF_F2_\w+)\s+(\d+)", HDR)) == {"DOPF_F2_GEN_ENERGY_BUDGET": "1", "DOPF_F2_GEN_RAMP_BUDGET": "8"}
    assert {getattr(_capi, n) for n in dir(_capi) if n.startswith("F2_")} == {1, 8}
    assert _capi._ALL_EXTENSIONS == _capi.EXTENSIONS + _capi.EXTENSIONS_MORE + _capi.EXTENSIONS_WORD2 + _capi.EXTENSIONS_FLOOR
    assert not any("budget_min_output" in x.entry for x in _capi._ALL_EXTENSIONS)


def test_header_text_states_the_rules():
    at = HDR.index("int dopf_set_generator_budget_min_output(")
    text = " ".join(HDR[HDR.rindex("/* Must-run floors on a budget context", 0, at):at].replace(" * ", " ").split())
    for phrase in ("DOPF_F2_GEN_ENERGY_BUDGET and without DOPF_F_GEN_RAMP", "floor[g,t] = min(p_min[g], cap[g,t])", "the floor follows an outage down",
                   "p_min = gen_pmax means must-take", "rows with default budgets and free windows included", "keep their definitions and sign rule",
                   "take effect at the next x-update", "converged becomes 0 and the residual maxima are cleared", "DOPF_E_NOMEM, naming the bytes",
                   "drops the captured graphs", "a NULL call switches back", "between two arrays the graphs stay valid",
                   "names this entry and stores nothing", "sum_t floor[g,t] > e_max[g]", "the test is exact",
                   "dopf_roll_horizon_coupled repeat that test", "the roll leaves p_min alone", "With G == 0 the call returns DOPF_OK"):
        assert phrase in text, phrase
    # the old setter's comment still says what it refuses
    at = HDR.index("int dopf_set_generator_min_output(")
    assert "DOPF_F2_GEN_ENERGY_BUDGET" in HDR[HDR.rindex("/*", 0, at):at]


def test_library_exports_the_entries_and_the_argtypes_match():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, "dopf_" + name), name
        f = getattr(api, name)
        assert f.restype is ctypes.c_int and list(f.argtypes) == [VP, DP], name


def test_the_plan_entry_is_never_set_by_plan_chain_and_the_launches_dispatch_on_it():
    plan = open(os.path.join(CSRC, "dopf_plan.h")).read()
    assert "double *genBudgetMinOut;" in plan and plan.count("genBudgetMinOut") == 1          # declared, never assigned in plan_chain
    assert 'static_assert(sizeof(DevView) == 832, "DevView must keep its size");' in open(os.path.join(CSRC, "dopf_internal.h")).read()
    for header, kernel in (("gen_budget.h", "k_gen_budget"), ("gen_budget_win.h", "k_gen_budget_win")):
        src = open(os.path.join(CSRC, header)).read()
        assert "with_bool(p.genBudgetMinOut != nullptr" in src, header
        assert re.search(r"template <bool LINES, bool AV, bool QC,( bool PR,)? bool MN>\s*__global__ __launch_bounds__\(512\) void %s\(" % kernel, src)
        assert "if constexpr (MN) pmn = mnv[g];" in src, header
    root = open(os.path.join(CSRC, "budget_root.h")).read()
    assert "DOPF_BR_FN int budget_piece(double u, double cap, int interval)" in root                      # the old one stays
    assert "DOPF_BR_FN int budget_piece(double u, double floor, double cap, int interval)" in root
    assert "hip" not in root.split("#pragma once")[1].lower().replace("__hipcc__", "").replace("no hip include", "")


def test_the_hosts_have_the_methods():
    for cls in (_capi.Engine, _capi.MultiEngine, admm.ADMM, sharded.ShardedADMM):
        assert callable(cls.set_budget_min_output) and cls.set_budget_min_output.__doc__, cls
    for cls in (_capi.Engine, admm.ADMM):
        assert callable(cls.budget_min_output) and cls.budget_min_output.__doc__, cls


def test_julia_shim_has_the_functions_and_the_ccalls():
    assert re.search(r"^function set_budget_min_output!\(admm::ADMM, p_min::Union\{Nothing, Vector\{Float64\}\}\)", JL, re.M)
    assert re.search(r"^function budget_min_output\(admm::ADMM\)", JL, re.M)
    for name in ("dopf_set_generator_budget_min_output", "dopf_multi_set_generator_budget_min_output", "dopf_get_generator_budget_min_output"):
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint,\s*\(Ptr\{Cvoid\}, Ptr\{Cdouble\}\)" % name, JL), name
    body = JL[JL.index("function set_budget_min_output!"):JL.index("function budget_min_output")]
    assert "admm.multi != C_NULL" in body and "dopf_check_multi" in body          # the multi branch of set_min_output!


def test_an_api_without_the_entries_refuses_with_a_clear_text(three_node, oracle_api):
    pp = three_node[4]
    e = _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, **pp.engine_kwargs())
    with pytest.raises(_capi.DopfError) as err:
        e.set_budget_min_output(np.zeros(pp.G))
    assert str(err.value) == "oracle_*: this API has no set_generator_budget_min_output"
    with pytest.raises(_capi.DopfError) as err:
        e.budget_min_output()
    assert str(err.value) == "oracle_*: this API has no get_generator_budget_min_output"


def test_packed_problem_carries_the_field_to_engines_and_shards(three_node):
    pp = copy.copy(three_node[4])
    assert pp.gen_budget_min_output is None and "gen_budget_min_output" not in pp.engine_kwargs()
    p_min = 0.25 * np.asarray(pp.gen_pmax, dtype=np.float64) + np.arange(pp.G)
    pp.gen_budget_min_output = p_min
    got = pp.engine_kwargs()["gen_budget_min_output"]
    assert got.dtype == np.float64 and np.array_equal(got, p_min)
    assert "gen_min_output" not in pp.engine_kwargs()                  # not the ramp contexts' floors: no ramp flag comes with it
    rows = 0
    for r in range(2):
        sh = pp.shard(r, 2)
        g0, g1 = sh.meta["gen_range"]
        assert np.array_equal(sh.engine_kwargs()["gen_budget_min_output"], p_min[g0:g1])
        rows += g1 - g0
    assert rows == pp.G
    for solve in (_capi.central_solve, _capi.central_solve_coupled):   # the device LP's front ends keep refusing floors
        with pytest.raises(_capi.DopfError, match="no generator minimum output"):
            solve(None, **pp.engine_kwargs())
    # the host LP takes them as its generators' lower bounds
    a = central.solve_central_packed(pp)
    b = central.solve_central_packed(three_node[4], gen_min_output=p_min)
    assert a.objective == b.objective and np.all(a.generation >= np.minimum(p_min[:, None], pp.gen_pmax[:, None]) - 1e-9)


def test_engine_constructor_asks_for_the_flag_and_applies_the_floors_last(three_node):
    """without a device: an API object that records the calls"""
    pp = copy.copy(three_node[4])
    ends = np.array([pp.T // 2, pp.T], dtype=np.int32)
    pp.gen_budget_windows = (ends, None, np.full((pp.G, 2), 1e9))
    pp.gen_budget_min_output = 0.5 * np.asarray(pp.gen_pmax, dtype=np.float64)
    calls = []

    class Api:
        prefix, has_mode = "fake_", False

        def create_ex(self, ctx, prob, params, flags2):
            calls.append(("create_ex", flags2.value))
            return 0

        def set_generator_energy_budget_windows(self, ctx, n, ends, lo, hi):
            calls.append(("windows", n))
            return 0

        def set_generator_budget_min_output(self, ctx, p):
            calls.append(("floors", None if not p else [p[g] for g in range(pp.G)]))
            return 0

        def destroy(self, ctx):
            pass
    e = _capi.Engine(Api(), params=_capi.default_params(), **pp.engine_kwargs())
    assert e.flags2 == _capi.F2_GEN_ENERGY_BUDGET and not e.params.flags & _capi.F_GEN_RAMP
    assert calls == [("create_ex", 1), ("windows", 2), ("floors", pp.gen_budget_min_output.tolist())]
    assert np.array_equal(e._mirror["gen_budget_min_output"], pp.gen_budget_min_output)
    e.set_budget_min_output(np.zeros(pp.G))                            # zeros are an array, not NULL: the floor kernels stay
    assert calls[-1] == ("floors", [0.0] * pp.G) and np.array_equal(e._mirror["gen_budget_min_output"], np.zeros(pp.G))
    e.set_budget_min_output(None)
    assert calls[-1] == ("floors", None) and "gen_budget_min_output" not in e._mirror
    # floors alone ask for the budget flag too
    del calls[:]
    q = copy.copy(three_node[4])
    q.gen_budget_min_output = pp.gen_budget_min_output
    e = _capi.Engine(Api(), params=_capi.default_params(), **q.engine_kwargs())
    assert e.flags2 == _capi.F2_GEN_ENERGY_BUDGET and [c[0] for c in calls] == ["create_ex", "floors"]


def test_sharded_setter_hands_on_the_ranks_slice():
    got = []

    class Engine:
        def set_budget_min_output(self, p):
            got.append(p)
    sh = sharded.ShardedADMM.__new__(sharded.ShardedADMM)
    sh.shard = type("S", (), {"meta": {"gen_range": (1, 3), "sto_range": (0, 0)}})()
    sh.engine, sh.problem = Engine(), type("P", (), {"G": 4, "S": 0})()
    sh.set_budget_min_output(np.arange(4.0))
    sh.set_budget_min_output(None)
    assert np.array_equal(got[0], [1.0, 2.0]) and got[1] is None
