"""DOPF_F2_GEN_ENERGY_BUDGET and the second flag word without a GPU: the header, the bindings, the third table of the
host side, the host route of the budgets (Generator.energy_min / energy_max -> pack -> engine_kwargs -> shard), the refusals of the
device LP and of an API without the entries, and the budget rows of the host LP."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg
from decentralopf_jl_amd import _capi, admm, central, sharded

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
ENTRY = ("dopf_create_ex", "dopf_multi_create_ex", "dopf_set_generator_energy_budget", "dopf_multi_set_generator_energy_budget")
BASE_KEYS = {"N", "L", "T", "demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax",
             "sto_node"}
DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int32)


def test_header_defines_the_flag_in_the_second_word():
    m = re.search(r"^#define\s+(DOPF_F2_GEN_ENERGY_BUDGET)\s+(\d+)", HDR, re.M)
    assert m and int(m.group(2)) == 1 == _capi.F2_GEN_ENERGY_BUDGET
    assert not re.fullmatch(r"DOPF_F_\w+", m.group(1))                 # the first word's macros are collected by that pattern
    first = {k: int(v) for k, v in re.findall(r"#define\s+(DOPF_F_\w+)\s+(\d+)", HDR)}
    assert "DOPF_F2_GEN_ENERGY_BUDGET" not in first and sum(first.values()) == 2 ** 32 - 1      # the first word: full, untouched
    last = HDR[HDR.index("#define DOPF_F_GEN_RAMP_NETWORK"):]
    last = last[:last.index("*/")]
    assert "LAST bit" in last and "second flag word" in last and "dopf_create_ex" in last
    flag = HDR[HDR.index("#define DOPF_F2_GEN_ENERGY_BUDGET"):]
    assert "ignore the bit" in flag[:flag.index("*/")]


def test_header_declares_the_four_entry_points():
    assert re.search(r"^int dopf_create_ex\(dopf_ctx \*\*out, const dopf_problem \*p, const dopf_params \*q, int32_t flags2\);$", HDR, re.M)
    assert re.search(r"^int dopf_multi_create_ex\(dopf_multi \*\*out, const dopf_problem \*p, const dopf_params \*q, int32_t n_gpus,\s*"
                     r"const int32_t \*devices, int32_t flags2\);$", HDR, re.M)
    assert re.search(r"^int dopf_set_generator_energy_budget\(dopf_ctx \*ctx, const double \*e_min[^)]*const double \*e_max[^)]*\);$",
                     HDR, re.M | re.S)
    assert re.search(r"^int dopf_multi_set_generator_energy_budget\(dopf_multi \*m, const double \*e_min, const double \*e_max\);$", HDR, re.M)


def test_library_exports_the_four_entry_points():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    for name in ENTRY:
        assert hasattr(lib, name), name


def test_ctypes_signatures_match_the_header():
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    P = ctypes.POINTER
    assert list(api.create_ex.argtypes) == [P(ctypes.c_void_p), P(_capi.DopfProblem), P(_capi.DopfParams), ctypes.c_int32]
    assert list(api.multi_create_ex.argtypes) == [P(ctypes.c_void_p), P(_capi.DopfProblem), P(_capi.DopfParams), ctypes.c_int32, IP,
                                                  ctypes.c_int32]
    for name in ("set_generator_energy_budget", "multi_set_generator_energy_budget"):
        f = getattr(api, name)
        assert f.restype is ctypes.c_int and list(f.argtypes) == [ctypes.c_void_p, DP, DP]
    assert api.create_ex.restype is ctypes.c_int and api.multi_create_ex.restype is ctypes.c_int


def test_create_ex_refuses_an_unknown_bit_before_it_looks_for_a_device(three_node):
    """the second word is checked first: no GPU is needed to see the refusal, and the message names the bit"""
    api = _capi.hip_api()
    pp = three_node[4]
    prob, keep, G, S = _capi._problem(**{k: v for k, v in pp.engine_kwargs().items() if k in BASE_KEYS})
    ctx = ctypes.c_void_p()
    q = _capi.default_params()
    for word, bit in ((2, 2), (1 | 64, 64), (-2147483648, 2147483648)):
        rc = api.create_ex(ctypes.byref(ctx), ctypes.byref(prob), ctypes.byref(q), word)
        msg = api.last_error(None).decode()
        assert rc == -1 and not ctx.value and f"unknown bit {bit}" in msg and "flags2" in msg, (rc, msg)


def test_julia_shim_defines_the_flag_the_setter_and_the_creates():
    m = re.search(r"^const DOPF_F2_GEN_ENERGY_BUDGET = (\d+)", JL, re.M)
    assert m and int(m.group(1)) == _capi.F2_GEN_ENERGY_BUDGET
    assert re.search(r"^function set_energy_budget!\(admm::ADMM", JL, re.M)
    for name in ENTRY[2:]:
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cdouble\}, Ptr\{Cdouble\}\)" % name, JL), name
    assert re.search(r"ccall\(\(:dopf_create_ex, DOPF_LIB\), Cint, \(Ref\{Ptr\{Cvoid\}\}, Ref\{CProblem\}, Ref\{CParams\}, Cint\)", JL)
    assert re.search(r"ccall\(\(:dopf_multi_create_ex, DOPF_LIB\), Cint, \(Ref\{Ptr\{Cvoid\}\}, Ref\{CProblem\}, Ref\{CParams\}, Cint, "
                     r"Ptr\{Cint\}, Cint\)", JL)
    assert re.search(r"flags2::Int=0", JL)


def test_the_three_tables_and_the_hosts():
    assert len(_capi.EXTENSIONS) == 6 and [x.setter for x in _capi.EXTENSIONS_MORE] == ["set_ramp"]
    assert [x.setter for x in _capi.EXTENSIONS_WORD2] == ["set_energy_budget"]
    x = _capi.EXTENSIONS_WORD2[0]
    assert x.flag == _capi.F2_GEN_ENERGY_BUDGET and x.word == 2 and x.entry == "set_generator_energy_budget"
    assert x.keys == ("gen_budget",) and x.packed and x.optional
    assert all(y.word == 1 for y in _capi.EXTENSIONS + _capi.EXTENSIONS_MORE)
    assert _capi._BY_SETTER["set_energy_budget"] is x and list(_capi._BY_SETTER)[:6] == [y.setter for y in _capi.EXTENSIONS]
    order = list(_capi._BY_SETTER)
    assert order.index("set_energy_budget") > order.index("set_availability")          # its check reads the caps
    for cls in (_capi.Engine, _capi.MultiEngine, admm.ADMM, sharded.ShardedADMM):
        assert callable(getattr(cls, "set_energy_budget")), cls


class _Sizes:
    N, L, T, G, S = 3, 3, 2, 4, 1


def test_extensions_keeps_its_pair_and_the_second_word_is_derived_from_todo():
    api = _capi.hip_api()
    lo, hi = np.zeros(4), np.array([np.inf, 50.0, np.inf, np.inf])
    out = _capi._extensions(api, None, _Sizes, {}, dict(gen_budget=(lo, hi)))
    assert isinstance(out, tuple) and len(out) == 2
    params, todo = out
    assert params is None and [x.setter for x, _ in todo] == ["set_energy_budget"] and _capi._flags2(todo) == 1     # no bit of the first word
    params, todo = _capi._extensions(api, None, _Sizes, {}, dict(gen_budget=(None, hi), gen_c2=np.ones(4)))
    assert params.flags == _capi.F_GEN_QUADRATIC_COST and _capi._flags2(todo) == 1
    params, todo = _capi._extensions(api, None, _Sizes, {}, dict(gen_c2=np.ones(4)))
    assert _capi._flags2(todo) == 0
    params, todo = _capi._extensions(api, None, _Sizes, {}, dict(gen_budget=(None, None)))
    assert params is None and todo == []


def _budgeted_three_node():
    nodes, lines, gens, stos = pkg.three_node_case()
    gens[2].energy_max = 300.0
    gens[3].energy_min, gens[3].energy_max = 20.0, 150.0
    return nodes, lines, gens, stos


def test_generator_default_pack_and_shard(three_node):
    nodes, lines, gens, stos, pp = three_node
    assert all(g.energy_min == 0.0 and g.energy_max == np.inf for g in gens)
    assert not pp.has_budget() and set(pp.engine_kwargs()) == BASE_KEYS             # yesterday's arguments while every budget is at its default
    nodes, lines, gens, stos = _budgeted_three_node()
    pq = pkg.pack(nodes, gens, stos, lines)
    lo, hi = np.array([0.0, 0.0, 0.0, 20.0]), np.array([np.inf, np.inf, 300.0, 150.0])
    assert pq.has_budget() and np.array_equal(pq.gen_budget[0], lo) and np.array_equal(pq.gen_budget[1], hi)
    kw = pq.engine_kwargs()
    assert set(kw) == BASE_KEYS | {"gen_budget"} and np.array_equal(kw["gen_budget"][0], lo) and np.array_equal(kw["gen_budget"][1], hi)
    a, b = pq.shard(0, 2), pq.shard(1, 2)
    assert np.array_equal(a.gen_budget[1], hi[:2]) and np.array_equal(b.gen_budget[0], lo[2:])
    assert "gen_budget" in a.engine_kwargs() and "gen_budget" in b.engine_kwargs()   # every rank runs with the flag, its slice default or not
    assert "gen_budget" not in pp.shard(0, 2).engine_kwargs()
    for bad in (dict(energy_min=-1.0), dict(energy_min=np.nan), dict(energy_min=np.inf), dict(energy_max=np.nan),
                dict(energy_min=5.0, energy_max=4.0), dict(energy_max=-1.0)):
        nodes, lines, gens, stos = pkg.three_node_case()
        for k, v in bad.items():
            setattr(gens[0], k, v)
        with pytest.raises(ValueError):
            pkg.pack(nodes, gens, stos, lines)


def test_an_api_without_the_entry_refuses_with_the_tables_texts(three_node, oracle_api):
    x, pp = _capi.EXTENSIONS_WORD2[0], three_node[4]
    assert not hasattr(oracle_api, x.entry)
    build = lambda **kw: _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, **kw, **pp.engine_kwargs())
    e = build(gen_budget=(np.zeros(pp.G), np.full(pp.G, np.inf)))          # the default value: nothing to set, no flag in either word
    assert e.params.flags == 0 and e.flags2 == 0 and all(v is None for v in e._mirror.values())
    for other in ((np.full(pp.G, 1.0), None), (None, np.full(pp.G, 100.0))):
        with pytest.raises(_capi.DopfError) as err:
            build(gen_budget=other)
        assert str(err.value) == f"oracle_*: this API has no {x.what} ({x.why})"
    with pytest.raises(_capi.DopfError) as err:
        e.set_energy_budget()
    assert str(err.value) == f"oracle_*: this API has no {x.what} (unsupported)"
    with pytest.raises(_capi.DopfError, match=r"oracle_\*: this API has no second flag word"):          # the word itself, given by hand
        build(flags2=_capi.F2_GEN_ENERGY_BUDGET)
    assert build(flags2=0).flags2 == 0


def test_the_device_lp_refuses_a_budgeted_case(three_node):
    nodes, lines, gens, stos = _budgeted_three_node()
    pq = pkg.pack(nodes, gens, stos, lines)
    with pytest.raises(ValueError, match="budget"):
        central.central_reference_on_device(nodes, gens, stos, lines)
    with pytest.raises(_capi.DopfError, match="budget"):
        _capi.central_solve(None, **pq.engine_kwargs())
    with pytest.raises(_capi.DopfError, match="budget"):
        _capi.central_solve(None, gen_budget=(np.ones(pq.G), None), **three_node[4].engine_kwargs())


def test_host_lp_with_budget_rows_on_a_case_known_by_hand():
    """One node, T = 4, demand 10 10 50 10; A (cost 1, 100 MW, energy_max 40) and B (cost 5, 100 MW). Without budgets A serves
    everything: 80. With A held to 40 over the window B delivers the other 40: 40 + 200 = 240. With energy_min = 90 on B alone the
    case is infeasible: the window's demand is 80."""
    n = pkg.Node("N", [10, 10, 50, 10], True)
    gens = [pkg.Generator("A", 1, 100, "k", n, energy_max=40.0), pkg.Generator("B", 5, 100, "k", n)]
    pp = pkg.pack([n], gens, [], [])
    free = central.solve_central_packed(pp, gen_budget=(np.zeros(2), np.full(2, np.inf)))
    assert abs(free.objective - 80.0) <= 1e-9
    r = central.solve_central_packed(pp)                            # the packed case's budgets
    assert abs(r.objective - 240.0) <= 1e-9
    assert np.allclose(r.generation.sum(axis=1), [40.0, 40.0], atol=1e-9)
    r = central.solve_central_packed(pp, gen_budget=(np.array([0.0, 40.0]), None))          # B's minimum take says the same
    assert abs(r.objective - 240.0) <= 1e-9
    with pytest.raises(RuntimeError):
        central.solve_central_packed(pp, gen_budget=(np.array([0.0, 90.0]), None))
