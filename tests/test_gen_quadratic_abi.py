"""DOPF_F_GEN_QUADRATIC_COST without a GPU: the header, the bindings, the host route of the coefficients
(Generator.quadratic_costs -> pack -> engine_kwargs -> shard), the refusals of the central LP, and the three helpers the GPU tests
stand on — the oracle pin assembled from T = 1 problems, the generators' optimality certificate and the central QP."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg
from decentralopf_jl_amd import _capi, central
from helpers import state_of
from helpers_quadratic import (COPPER_EVEN, COPPER_ODD, NETWORK, STATE_KEYS, case, gen_kkt_violation, interior_fraction, params_of,
                               slice_reference, solve_qp, total_cost, zero_state)

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
ENTRY = ("dopf_set_generator_quadratic_cost", "dopf_multi_set_generator_quadratic_cost")
BASE_KEYS = {"N", "L", "T", "demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax",
             "sto_node"}


def test_header_defines_the_flag():
    m = re.search(r"#define\s+DOPF_F_GEN_QUADRATIC_COST\s+(\d+)", HDR)
    assert m and int(m.group(1)) == 1 << 30 == 1073741824 == _capi.F_GEN_QUADRATIC_COST
    others = [int(v) for k, v in re.findall(r"#define\s+(DOPF_F_\w+)\s+(\d+)", HDR) if k != "DOPF_F_GEN_QUADRATIC_COST"]
    assert others and all(v & (1 << 30) == 0 for v in others)


def test_header_declares_both_entry_points():
    assert re.search(r"^int dopf_set_generator_quadratic_cost\(dopf_ctx \*ctx, const double \*c2[^)]*\);$", HDR, re.M)
    assert re.search(r"^int\s+dopf_multi_set_generator_quadratic_cost\(dopf_multi \*m, const double \*c2[^)]*\);$", HDR, re.M)
    flag = HDR[HDR.index("#define DOPF_F_GEN_QUADRATIC_COST"):]
    assert "ignore the flag" in flag[:flag.index("*/")]          # the central LP says so, as for the rating table


def test_library_exports_both_entry_points():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    for name in ENTRY:
        assert hasattr(lib, name), name


def test_ctypes_signatures_match_the_header():
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for name in ("set_generator_quadratic_cost", "multi_set_generator_quadratic_cost"):
        f = getattr(api, name)
        assert f.restype is ctypes.c_int
        assert len(f.argtypes) == 2 and f.argtypes[0] is ctypes.c_void_p and f.argtypes[1] is ctypes.POINTER(ctypes.c_double)


def test_julia_shim_defines_the_flag_and_the_setter():
    m = re.search(r"^const DOPF_F_GEN_QUADRATIC_COST = (\d+)", JL, re.M)
    assert m and int(m.group(1)) == _capi.F_GEN_QUADRATIC_COST
    assert re.search(r"^function set_quadratic_cost!\(admm::ADMM", JL, re.M)
    for name in ENTRY:
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cdouble\}\)" % name, JL), name


def test_hosts_have_the_setter():
    from decentralopf_jl_amd import admm, sharded
    for cls in (_capi.Engine, _capi.MultiEngine, admm.ADMM, sharded.ShardedADMM):
        assert callable(getattr(cls, "set_quadratic_cost")), cls


def _curved_three_node():
    nodes, lines, gens, stos = pkg.three_node_case()
    gens[2].quadratic_costs = 0.02
    return nodes, lines, gens, stos


def test_generator_default_pack_and_shard(three_node):
    nodes, lines, gens, stos, pp = three_node
    assert all(g.quadratic_costs == 0.0 for g in gens)
    assert np.array_equal(pp.gen_c2, np.zeros(pp.G)) and not pp.has_quadratic_cost()
    assert set(pp.engine_kwargs()) == BASE_KEYS                      # yesterday's arguments while every value is 0
    nodes, lines, gens, stos = _curved_three_node()
    pq = pkg.pack(nodes, gens, stos, lines)
    want = np.array([0.0, 0.0, 0.02, 0.0])
    assert np.array_equal(pq.gen_c2, want) and pq.has_quadratic_cost()
    kw = pq.engine_kwargs()
    assert set(kw) == BASE_KEYS | {"gen_c2"} and np.array_equal(kw["gen_c2"], want)
    a, b = pq.shard(0, 2), pq.shard(1, 2)
    assert np.array_equal(a.gen_c2, want[:2]) and np.array_equal(b.gen_c2, want[2:])
    assert "gen_c2" in a.engine_kwargs() and "gen_c2" in b.engine_kwargs()      # every rank runs with the flag, its slice all 0 or not
    assert "gen_c2" not in pp.shard(0, 2).engine_kwargs()
    for bad in (-1.0, np.nan, np.inf):
        gens[0].quadratic_costs = bad
        with pytest.raises(ValueError):
            pkg.pack(nodes, gens, stos, lines)


def test_oracle_backend_refuses_a_coefficient_other_than_0(three_node, oracle_api):
    nodes, lines, gens, stos, pp = three_node
    assert not hasattr(oracle_api, "set_generator_quadratic_cost")   # loads without the symbols
    e = _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, **pp.engine_kwargs())
    with pytest.raises(_capi.DopfError, match="unsupported"):
        e.set_quadratic_cost(np.zeros(pp.G))
    with pytest.raises(_capi.DopfError, match="no quadratic generator costs"):
        _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, gen_c2=np.full(pp.G, 0.1), **pp.engine_kwargs())
    _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, gen_c2=np.zeros(pp.G), **pp.engine_kwargs())   # zeros: nothing to set


def test_central_refuses_a_quadratic_case(three_node):
    nodes, lines, gens, stos, pp = three_node
    assert abs(central.solve_central_packed(pp).objective - 14035.0) <= 1e-6 * 14035.0       # zeros: the LP of before
    nodes, lines, gens, stos = _curved_three_node()
    pq = pkg.pack(nodes, gens, stos, lines)
    with pytest.raises(ValueError, match="quadratic"):
        central.solve_central_packed(pq)
    with pytest.raises(ValueError, match="quadratic"):
        central.central_reference_on_device(nodes, gens, stos, lines)
    with pytest.raises(_capi.DopfError, match="quadratic"):
        _capi.central_solve(None, **pq.engine_kwargs())


# ---- the helpers ---------------------------------------------------------------------------------------------------------------

def _emulate(api, pp, c2, steps, prm, st=None, it=1):
    """`steps` iterations of slice_reference from st (the zero state); yields (before, after)"""
    st = zero_state(pp) if st is None else st
    for _ in range(steps):
        new = dict(slice_reference(api, pp, c2, st, it, **prm), D=st["D"], C=st["C"])
        yield st, new
        st, it = new, it + 1


def test_slice_reference_at_c2_0_is_the_oracle_bit_for_bit(oracle_api):
    pp = case(NETWORK[0])
    prm = params_of(pp)
    o = _capi.Engine(oracle_api, params=_capi.default_params(**prm), mode=1, **pp.engine_kwargs())
    for k, (_, new) in enumerate(_emulate(oracle_api, pp, 0.0, 50, prm)):
        o.iterate(1)
        so = state_of(o)
        for key in STATE_KEYS + ("flow",):
            assert np.array_equal(new[key], so[key]), (k, key)
        assert abs(float(new["cost"][0] - so["cost"][0])) <= 1e-12 * abs(float(so["cost"][0]))      # (NumPy's sum, another order)


@pytest.mark.parametrize("which", [COPPER_ODD, COPPER_EVEN, NETWORK], ids=["copper-T5", "copper-T4", "net-6x8"])
def test_certificate_on_the_slice_reference(oracle_api, which):
    kw, c2, steps = which
    pp = case(kw)
    prm = params_of(pp)
    wf = prm.get("w_flow", 10.0)
    worst, inside = 0.0, []
    for before, new in _emulate(oracle_api, pp, c2, steps, prm):
        duals = (before["lam"], before["mu"], before["rho"])
        v = gen_kkt_violation(pp, c2, pp.gen_pmax, before, duals, new["P"], prm["gamma"], wf)
        assert v <= 1e-10, v
        worst = max(worst, v)
        inside.append(interior_fraction(pp, new["P"]))
    assert gen_kkt_violation(pp, 1.1 * c2, pp.gen_pmax, before, duals, new["P"], prm["gamma"], wf) > 1e-3      # (it can fail)
    assert np.mean(inside) >= 0.25, np.mean(inside)              # rows inside their box are where c2 shows
    print(f"certificate {worst:.1e}, interior {np.mean(inside):.2f}")


def test_certificate_on_a_plain_oracle_step(oracle_api):
    pp = case(NETWORK[0])
    prm = params_of(pp)
    o = _capi.Engine(oracle_api, params=_capi.default_params(**prm), mode=1, **pp.engine_kwargs())
    o.iterate(7)
    before = state_of(o)
    o.iterate(1)
    v = gen_kkt_violation(pp, 0.0, pp.gen_pmax, before, (before["lam"], before["mu"], before["rho"]), state_of(o)["P"], prm["gamma"],
                          prm["w_flow"])
    assert v <= 1e-10, v


@pytest.mark.parametrize("which", [COPPER_ODD, COPPER_EVEN], ids=["copper-T5", "copper-T4"])
def test_emulated_iterations_reach_the_central_qp(oracle_api, which):
    kw, c2, _ = which
    pp = case(kw)
    for _, st in _emulate(oracle_api, pp, c2, 400, params_of(pp)):
        pass
    obj, P, _, _ = solve_qp(pp, c2)
    assert abs(obj - total_cost(pp, c2, P)) <= 1e-9 * obj
    assert abs(float(st["cost"][0]) - obj) <= 1e-8 * obj, (float(st["cost"][0]), obj)
    assert np.abs(st["inj"].sum(axis=0)).max() <= 1e-9


def test_solve_qp_with_storages_and_lines_is_the_lp_at_c2_0(three_node):
    nodes, lines, gens, stos, pp = three_node
    obj, P, D, C = solve_qp(pp, 0.0)
    assert abs(obj - 14035.0) <= 1e-6 * 14035.0, obj
    assert abs(obj - total_cost(pp, 0.0, P, D, C)) <= 1e-9 * obj
    curved = solve_qp(pp, 0.02)[0]
    assert curved > obj                                          # (a convex term on top: dearer)
