"""dopf_set_generator_energy_budget_windows without a GPU: the header's five prototypes, the library's exports and the
bindings' argtypes, no new flag and no new row of the extension tables, the Julia shim's ccalls, the packed problem's table on its way
to the engines and the shards, and the host LP with one inequality pair per generator and window."""
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
DP, IP, I32, VP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_void_p

# name -> the argument types behind the handle, as include/dopf.h declares them
ENTRIES = {
    "set_generator_energy_budget_windows": [I32, IP, DP, DP],
    "get_generator_energy_budget_windows": [IP, IP, DP, DP],
    "get_generator_budget_window_price": [DP],
    "multi_set_generator_energy_budget_windows": [I32, IP, DP, DP],
    "multi_get_generator_budget_window_price": [DP],
}
CTYPE = {"int32_t": I32, "const int32_t *": IP, "int32_t *": IP, "const double *": DP, "double *": DP}


def _prototype(name):
    m = re.search(r"^int dopf_%s\((.*?)\);" % name, HDR, re.M | re.S)
    assert m, name
    args = [re.sub(r"/\*.*?\*/", "", a, flags=re.S).strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    return [re.sub(r"\w+$", "", a).strip() for a in args]


def test_header_declares_the_five_entries_with_the_bound_argument_types():
    for name, want in ENTRIES.items():
        types = _prototype(name)
        assert types[0] == ("dopf_multi *" if name.startswith("multi_") else "dopf_ctx *"), name
        assert [CTYPE[t] for t in types[1:]] == want, (name, types)


def test_no_flag_came_with_the_entries():
    assert dict(re.findall(r"#define\s+(DOPF_F2_\w+)\s+(\d+)", HDR)) == {"DOPF_F2_GEN_ENERGY_BUDGET": "1", "DOPF_F2_GEN_RAMP_BUDGET": "8"}
    assert not re.search(r"#define\s+DOPF_F\w*WIN", HDR)
    assert {getattr(_capi, n) for n in dir(_capi) if n.startswith("F2_")} == {1, 8}


def test_header_text_states_the_rules():
    at = HDR.index("int dopf_set_generator_energy_budget_windows(")
    text = " ".join(HDR[HDR.rindex("/* Energy budgets per sub-window", 0, at):at].replace(" * ", " ").split())
    for phrase in ("win_end[j-1] <= t < win_end[j]", "strictly increasing", "1 <= n_win <= T", "[j + n_win*g]", "exact minimiser",
                   "One window with end T is dopf_set_generator_energy_budget, bit for bit", "DOPF_E_NOMEM, naming the bytes",
                   "drops the captured graphs", "the graphs stay valid", "n_win == 0 with all pointers NULL removes the table",
                   "One description of the budgets at a time", "dopf_set_generator_energy_budget(ctx, NULL, NULL)",
                   "dopf_roll_horizon_coupled DOPF_E_UNSUPPORTED", "names the entry, g and j and stores nothing",
                   "DOPF_F2_GEN_RAMP_BUDGET context", "dopf_set_generator_availability repeats that check window by window",
                   "With G == 0 the call returns DOPF_OK"):
        assert phrase in text, phrase
    # one added sentence each in the comments of the flag, the whole-horizon setter, its price getter and the coupled roll
    for anchor, phrase in (("#define DOPF_F2_GEN_RAMP_BUDGET", "dopf_set_generator_energy_budget_windows, k_gen_budget_win"),
                           ("int dopf_set_generator_energy_budget(", "(NULL, NULL) stays allowed"),
                           ("int dopf_get_generator_budget_price(", "dopf_get_generator_budget_window_price"),
                           ("int dopf_roll_horizon_coupled(", "remove the table, roll, and set the next window's table")):
        at = HDR.index(anchor)
        assert phrase in " ".join(HDR[HDR.rindex("/*", 0, at) if anchor.startswith("int") else at - 900:at].replace(" * ", " ").split()), anchor


def test_library_exports_the_entries_and_the_argtypes_match():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for name, want in ENTRIES.items():
        assert hasattr(lib, "dopf_" + name), name
        f = getattr(api, name)
        assert f.restype is ctypes.c_int and list(f.argtypes) == [VP] + want, name


def test_the_extension_tables_are_unchanged():
    assert [x.setter for x in _capi.EXTENSIONS] == ["set_efficiency", "set_initial_levels", "set_terminal_levels", "set_availability",
                                                    "set_line_rating", "set_quadratic_cost"]
    assert [x.setter for x in _capi.EXTENSIONS_MORE] == ["set_ramp"] and [x.setter for x in _capi.EXTENSIONS_WORD2] == ["set_energy_budget"]
    assert [x.setter for x in _capi.EXTENSIONS_FLOOR] == ["set_min_output"]
    assert _capi._ALL_EXTENSIONS == _capi.EXTENSIONS + _capi.EXTENSIONS_MORE + _capi.EXTENSIONS_WORD2 + _capi.EXTENSIONS_FLOOR
    assert not any("window" in x.entry for x in _capi._ALL_EXTENSIONS)


def test_the_plan_entry_is_never_set_by_plan_chain_and_the_view_keeps_its_size():
    plan = open(os.path.join(CSRC, "dopf_plan.h")).read()
    assert "BudgetWinView genBudgetWin;" in plan and plan.count("genBudgetWin") == 1
    assert 'static_assert(sizeof(DevView) == 832, "DevView must keep its size");' in open(os.path.join(CSRC, "dopf_internal.h")).read()
    agents = open(os.path.join(CSRC, "kernels_agents.hip")).read()
    assert agents.index('#include "gen_budget.h"') < agents.index('#include "gen_budget_win.h"')
    assert agents.index("if (p.genBudgetWin.n_win > 0) { launch_gen_budget_win(v, p, s); return; }") < agents.index("if (p.genBudget) {")
    # the mapping helper is plain C++ (tests/budget_windows_main.cpp builds it with g++)
    assert "hip" not in open(os.path.join(CSRC, "budget_win_map.h")).read().split("#pragma once")[1].lower().replace("no hip include", "")


def test_the_hosts_have_the_methods():
    for cls in (_capi.Engine, _capi.MultiEngine, admm.ADMM, sharded.ShardedADMM):
        for name in ("set_energy_budget_windows", "energy_budget_windows", "budget_window_price"):
            assert callable(getattr(cls, name)) and getattr(cls, name).__doc__, (cls, name)


def test_julia_shim_has_the_functions_and_the_ccalls():
    assert re.search(r"^function set_energy_budget_windows!\(admm::ADMM, win_end", JL, re.M)
    assert re.search(r"^function energy_budget_windows\(admm::ADMM\)", JL, re.M)
    assert re.search(r"^function budget_window_price\(admm::ADMM, n_win::Int\)", JL, re.M)
    sig = {"dopf_set_generator_energy_budget_windows": r"\(Ptr\{Cvoid\}, Cint, Ptr\{Cint\}, Ptr\{Cdouble\}, Ptr\{Cdouble\}\)",
           "dopf_multi_set_generator_energy_budget_windows": r"\(Ptr\{Cvoid\}, Cint, Ptr\{Cint\}, Ptr\{Cdouble\}, Ptr\{Cdouble\}\)",
           "dopf_get_generator_energy_budget_windows": r"\(Ptr\{Cvoid\}, Ptr\{Cint\}, Ptr\{Cint\}, Ptr\{Cdouble\}, Ptr\{Cdouble\}\)",
           "dopf_get_generator_budget_window_price": r"\(Ptr\{Cvoid\}, Ptr\{Cdouble\}\)",
           "dopf_multi_get_generator_budget_window_price": r"\(Ptr\{Cvoid\}, Ptr\{Cdouble\}\)"}
    for name, args in sig.items():
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint,\s*%s" % (name, args), JL), name


def test_an_api_without_the_entries_refuses_with_a_clear_text(three_node, oracle_api):
    pp = three_node[4]
    e = _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, **pp.engine_kwargs())
    with pytest.raises(_capi.DopfError) as err:
        e.set_energy_budget_windows([pp.T])
    assert str(err.value) == "oracle_*: this API has no set_generator_energy_budget_windows"
    with pytest.raises(_capi.DopfError, match="no get_generator_budget_window_price"):
        e.budget_window_price()
    with pytest.raises(_capi.DopfError, match="no get_generator_energy_budget_windows"):
        e.energy_budget_windows()


# ---- the packed problem ------------------------------------------------------------------------------------------------------------------

def _table(pp):
    ends = np.array([pp.T // 2, pp.T], dtype=np.int32)
    lo = np.arange(pp.G * 2, dtype=np.float64).reshape(pp.G, 2)
    hi = lo + 100.0
    return ends, lo, hi


def test_packed_problem_carries_the_table_to_engines_and_shards(three_node):
    import copy
    pp = copy.copy(three_node[4])
    assert not pp.has_budget_windows() and "gen_budget_windows" not in pp.engine_kwargs()
    ends, lo, hi = _table(pp)
    pp.gen_budget_windows = (ends, lo, None)
    assert pp.has_budget_windows()
    e, a, b = pp.engine_kwargs()["gen_budget_windows"]
    assert e.dtype == np.int32 and np.array_equal(e, ends) and np.array_equal(a, lo) and np.all(b == np.inf) and b.shape == (pp.G, 2)
    pp.gen_budget_windows = (ends, lo, hi)
    rows = 0
    for r in range(2):
        sh = pp.shard(r, 2)
        g0, g1 = sh.meta["gen_range"]
        assert sh.has_budget_windows()
        e, a, b = sh.engine_kwargs()["gen_budget_windows"]
        assert np.array_equal(e, ends) and np.array_equal(a, lo[g0:g1]) and np.array_equal(b, hi[g0:g1])
        rows += g1 - g0
    assert rows == pp.G
    # the engines ask for the budgets' flag and set the table behind everything else; the device LP's front ends refuse it, as floors
    for solve in (_capi.central_solve, _capi.central_solve_coupled):
        with pytest.raises(_capi.DopfError, match="no energy budgets per sub-window"):
            solve(None, **pp.engine_kwargs())


def test_engine_constructor_asks_for_the_flag_and_applies_the_table_last(three_node):
    """without a device: an API object that records the calls"""
    import copy
    pp = copy.copy(three_node[4])
    pp.gen_budget_windows = _table(pp)
    calls = []

    class Api:
        prefix, has_mode = "fake_", False

        def create_ex(self, ctx, prob, params, flags2):
            calls.append(("create_ex", flags2.value))
            return 0

        def set_generator_energy_budget_windows(self, ctx, n, ends, lo, hi):
            calls.append(("windows", n, [ends[j] for j in range(n)], [lo[k] for k in range(n * pp.G)], [hi[k] for k in range(n * pp.G)]))
            return 0

        def destroy(self, ctx):
            pass
    e = _capi.Engine(Api(), params=_capi.default_params(), **pp.engine_kwargs())
    ends, lo, hi = pp.gen_budget_windows
    assert e.flags2 == _capi.F2_GEN_ENERGY_BUDGET
    assert calls == [("create_ex", 1), ("windows", 2, ends.tolist(), lo.ravel().tolist(), hi.ravel().tolist())]          # C order: [j + n_win*g]
    m = e._mirror["gen_budget_windows"]
    assert np.array_equal(m[0], ends) and np.array_equal(m[1], lo) and np.array_equal(m[2], hi)
    e.set_energy_budget_windows(None)
    assert "gen_budget_windows" not in e._mirror and calls[-1] == ("windows", 0, [], [], [])


def test_sharded_window_price_places_the_ranks_rows_and_sums():
    class Shard:
        meta = {"gen_range": (1, 3)}

    class Engine:
        def budget_window_price(self):
            return np.array([[1.5, 0.0], [-2.0, 3.0]])
    sh = sharded.ShardedADMM.__new__(sharded.ShardedADMM)
    sh.shard, sh.engine, sh.world, sh._tensor = Shard(), Engine(), 2, None
    sh.problem = type("P", (), {"G": 4})()
    out = sh.budget_window_price(all_reduce=lambda x: x + 1.0)
    assert np.array_equal(out, np.array([[0, 0], [1.5, 0], [-2, 3], [0, 0]]) + 1.0)
    assert np.array_equal(sh._mine_rows(np.arange(8.0).reshape(4, 2)), [[2, 3], [4, 5]])


# ---- the host LP -------------------------------------------------------------------------------------------------------------------------

def test_host_lp_one_window_is_the_whole_horizon_budget(three_node):
    pp = three_node[4]
    free = central.solve_central_packed(pp)
    E = free.generation.sum(axis=1)
    hi = np.full(pp.G, np.inf)
    hi[1] = 0.9 * E[1]                                            # the wind unit, as tests/test_gpu_gen_budget.py's CONV
    lo = np.zeros(pp.G)
    a = central.solve_central_packed(pp, gen_budget=(lo, hi))
    b = central.solve_central_packed(pp, gen_budget_windows=([pp.T], lo[:, None], hi[:, None]))
    assert abs(a.objective - b.objective) <= 1e-9 * abs(a.objective)
    assert np.abs(a.generation - b.generation).max() <= 1e-9 * float(pp.gen_pmax.max())
    assert b.budget_window_dual.shape == (pp.G, 1) and a.budget_window_dual is None
    assert b.budget_window_dual[1, 0] < 0.0 and np.all(np.delete(b.budget_window_dual[:, 0], 1) == 0.0)          # e_max binds: negative


def test_host_lp_two_windows_bind_and_the_duals_have_the_documented_sign(three_node):
    pp = three_node[4]
    T, G = pp.T, pp.G
    free = central.solve_central_packed(pp)
    ends = [T // 2, T]
    Ew = np.stack([free.generation[:, :ends[0]].sum(axis=1), free.generation[:, ends[0]:].sum(axis=1)], axis=1)          # (G, 2)
    hi = np.full((G, 2), np.inf)
    held = []
    for j in range(2):                                            # each window holds one unit to 0.8 of its free energy there
        cands = [g for g in np.argsort(-Ew[:, j]) if g not in held and Ew[g, j] > 0.0]
        for g in cands:
            trial = hi.copy()
            trial[g, j] = 0.8 * Ew[g, j]
            try:
                central.solve_central_packed(pp, gen_budget_windows=(ends, None, trial), duals=False)
            except RuntimeError:
                continue                                          # (a unit the lines leave no substitute for)
            hi, held = trial, held + [g]
            break
    assert len(held) == 2
    want = central.solve_central_packed(pp, gen_budget_windows=(ends, None, hi))
    rel = (want.objective - free.objective) / free.objective
    print(f"two windows: units {held} held to 0.8 of {[float(Ew[g, j]) for j, g in enumerate(held)]}, objective {free.objective:.4f} -> "
          f"{want.objective:.4f} ({rel:.2e} relative), duals {[float(want.budget_window_dual[g, j]) for j, g in enumerate(held)]}")
    assert rel > 1e-6
    for j, g in enumerate(held):
        assert abs(want.generation[g, (0 if j == 0 else ends[0]):ends[j]].sum() - hi[g, j]) <= 1e-7 * max(1.0, hi[g, j])          # binds
        assert want.budget_window_dual[g, j] < 0.0                # an upper end that binds: d objective / d e_max < 0
    mask = np.ones((G, 2), dtype=bool)
    for j, g in enumerate(held):
        mask[g, j] = False
    assert np.all(want.budget_window_dual[mask] == 0.0)
    # a lower end that binds: positive. The cheapest-to-raise unit of the first window must deliver a tenth of its room more there
    room = ends[0] * pp.gen_pmax
    g = int(np.argmin(np.where(Ew[:, 0] < room, Ew[:, 0] / room, np.inf)))
    lo = np.zeros((G, 2))
    lo[g, 0] = Ew[g, 0] + 0.1 * (room[g] - Ew[g, 0])
    up = central.solve_central_packed(pp, gen_budget_windows=(ends, lo, None))
    assert up.objective > free.objective * (1.0 + 1e-6) and up.budget_window_dual[g, 0] > 0.0
    assert up.generation[g, :ends[0]].sum() >= lo[g, 0] - 1e-7 * max(1.0, lo[g, 0])
    # the packed case's own table is taken where none is given
    import copy
    q = copy.copy(pp)
    q.gen_budget_windows = (ends, None, hi)
    assert abs(central.solve_central_packed(q).objective - want.objective) <= 1e-9 * want.objective


def test_host_lp_reports_an_infeasible_table(three_node):
    pp = three_node[4]
    hi = np.full((pp.G, 2), np.inf)
    hi[:, 1] = 0.0                                                # nobody may generate in the second half: the demand there cannot be met
    with pytest.raises(RuntimeError, match="central LP"):
        central.solve_central_packed(pp, gen_budget_windows=([pp.T // 2, pp.T], None, hi))
    with pytest.raises(ValueError, match="strictly increasing"):
        central.solve_central_packed(pp, gen_budget_windows=([pp.T, pp.T], None, None))
