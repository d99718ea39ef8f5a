"""Storage efficiencies (DOPF_F_STO_EFFICIENCY) at the boundary: the header, the exports, the ctypes signatures, the Julia shim,
network.Storage / pack / engine_kwargs / shard, the oracle API's refusal, the central LP with lossy storage-balance rows, and the
self-test of the NumPy certificate the GPU tests rely on. No compute calls on a device (runs without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, build_oracle, pkg
from decentralopf_jl_amd import _capi, central, synth
from helpers_efficiency import levels_eff, solve_storage_qp, storage_kkt_violation_eff

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
ENTRY = ("dopf_set_storage_efficiency", "dopf_multi_set_storage_efficiency")
BASE_KEYS = {"N", "L", "T", "demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax",
             "sto_node"}


def test_header_defines_the_flag():
    m = re.search(r"#define\s+DOPF_F_STO_EFFICIENCY\s+(\d+)", HDR)
    assert m and int(m.group(1)) == 1 << 28 == 268435456 == _capi.F_STO_EFFICIENCY
    others = [int(v) for k, v in re.findall(r"#define\s+(DOPF_F_\w+)\s+(\d+)", HDR) if k != "DOPF_F_STO_EFFICIENCY"]
    assert others and all(v & (1 << 28) == 0 for v in others)


def test_header_declares_both_entry_points():
    assert re.search(r"^int dopf_set_storage_efficiency\(dopf_ctx \*ctx, const double \*eta_c, const double \*eta_d\);$", HDR, re.M)
    assert re.search(r"^int\s+dopf_multi_set_storage_efficiency\(dopf_multi \*m, const double \*eta_c, const double \*eta_d\);$", HDR, re.M)


def test_library_exports_both_entry_points():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    for name in ENTRY:
        assert hasattr(lib, name), name


def test_ctypes_signatures_match_the_header():
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for name in ("set_storage_efficiency", "multi_set_storage_efficiency"):
        f = getattr(api, name)
        assert f.restype is ctypes.c_int
        assert len(f.argtypes) == 3 and f.argtypes[0] is ctypes.c_void_p
        assert f.argtypes[1] is ctypes.POINTER(ctypes.c_double) and f.argtypes[2] is ctypes.POINTER(ctypes.c_double)


def test_julia_shim_defines_the_flag_and_the_setter():
    m = re.search(r"^const DOPF_F_STO_EFFICIENCY = (\d+)", JL, re.M)
    assert m and int(m.group(1)) == _capi.F_STO_EFFICIENCY
    assert re.search(r"^function set_efficiency!\(admm::ADMM", JL, re.M)
    for name in ENTRY:
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cdouble\}, Ptr\{Cdouble\}\)" % name, JL), name


def _three_node_with(eta_c, eta_d):
    nodes, lines, gens, stos = pkg.three_node_case()
    stos[0].charge_efficiency, stos[0].discharge_efficiency = eta_c, eta_d
    return nodes, lines, gens, stos


def test_storage_default_leaves_the_engine_arguments_unchanged(three_node):
    nodes, lines, gens, stos, pp = three_node
    assert all(s.charge_efficiency == 1.0 and s.discharge_efficiency == 1.0 for s in stos)
    assert not pp.has_efficiency() and set(pp.engine_kwargs()) == BASE_KEYS
    ec, ed = pp.efficiency()
    assert np.array_equal(ec, [1.0]) and np.array_equal(ed, [1.0])


def test_pack_and_engine_kwargs_carry_the_efficiencies():
    for ec, ed in ((0.9, 1.0), (1.0, 0.8), (0.9, 0.8)):
        nodes, lines, gens, stos = _three_node_with(ec, ed)
        pp = pkg.pack(nodes, gens, stos, lines)
        assert pp.has_efficiency() and np.array_equal(pp.sto_eta_c, [ec]) and np.array_equal(pp.sto_eta_d, [ed])
        kw = pp.engine_kwargs()
        assert set(kw) == BASE_KEYS | {"sto_eta"}
        assert np.array_equal(kw["sto_eta"][0], [ec]) and np.array_equal(kw["sto_eta"][1], [ed])


def test_shard_slices_the_efficiencies():
    pp = synth.synthetic_case(20, 7, 24, seed=5)
    pp.sto_eta_c, pp.sto_eta_d = np.linspace(0.6, 1.0, 7), np.linspace(1.0, 0.7, 7)
    for world in (2, 3):
        parts = [pp.shard(r, world) for r in range(world)]
        assert np.array_equal(np.concatenate([p.sto_eta_c for p in parts]), pp.sto_eta_c)
        assert np.array_equal(np.concatenate([p.sto_eta_d for p in parts]), pp.sto_eta_d)
        assert all("sto_eta" in p.engine_kwargs() for p in parts if p.S)
    plain = synth.synthetic_case(20, 7, 24, seed=5)
    assert all("sto_eta" not in plain.shard(r, 2).engine_kwargs() for r in range(2))


def test_oracle_backend_refuses_efficiencies(three_node):
    from oracle.binding import OracleApi
    nodes, lines, gens, stos, pp = three_node
    api = OracleApi(build_oracle())
    assert not hasattr(api, "set_storage_efficiency")                    # loads without the symbols
    e = _capi.Engine(api, params=_capi.default_params(), mode=0, **pp.engine_kwargs())
    with pytest.raises(_capi.DopfError, match="unsupported"):
        e.set_efficiency([0.9], [0.9])
    with pytest.raises(_capi.DopfError, match="no storage efficiencies"):
        _capi.Engine(api, params=_capi.default_params(), mode=0, sto_eta=([0.9], [1.0]), **pp.engine_kwargs())
    _capi.Engine(api, params=_capi.default_params(), mode=0, sto_eta=([1.0], [1.0]), **pp.engine_kwargs())   # all ones: nothing to set


def test_central_lp_with_efficiencies(three_node):
    nodes, lines, gens, stos, pp = three_node
    base = central.solve_central_packed(pp)
    ones = central.solve_central_packed(pp, efficiency=(np.ones(1), np.ones(1)))
    assert ones.objective == base.objective
    for a, b in ((ones.generation, base.generation), (ones.discharge, base.discharge), (ones.charge, base.charge), (ones.level, base.level)):
        assert np.array_equal(a, b)
    eta = (np.full(1, 0.9), np.full(1, 0.9))
    lossy = central.solve_central_packed(pp, efficiency=eta)
    assert np.abs(lossy.level - levels_eff(np.zeros(1), eta[0], eta[1], lossy.discharge, lossy.charge)).max() <= 1e-9
    assert lossy.level.min() >= -1e-9 and (lossy.level - pp.sto_emax[:, None]).max() <= 1e-9
    assert lossy.objective >= base.objective - 1e-9
    # the packed case's own efficiencies are the default, and central_reference passes them on
    n2, l2, g2, s2 = _three_node_with(0.9, 0.9)
    assert abs(central.central_reference(n2, g2, s2, l2).objective - lossy.objective) <= 1e-9 * abs(lossy.objective)
    with pytest.raises(ValueError, match="no storage efficiencies"):
        central.central_reference_on_device(n2, g2, s2, l2)
    with pytest.raises(ValueError):
        central.solve_central_packed(pp, efficiency=(np.full(1, 1.1), np.ones(1)))


def _qp_case(seed, T, eta_c, eta_d, band):
    rng = np.random.default_rng(seed)
    pp = synth.synthetic_case(4, 1, T, seed=seed)
    pp.sto_pmax, pp.sto_emax = np.array([3.0]), np.array([5.0])
    D0, C0 = rng.uniform(0.0, 3.0, (1, T)), rng.uniform(0.0, 3.0, (1, T))
    theta = rng.uniform(-8.0, 8.0, (1, T))
    e0 = np.array([2.0])
    lo, hi = band
    D, C = solve_storage_qp(pp.sto_mc[0], 3.0, 5.0, 2.0, lo, hi, eta_c, eta_d, D0[0], C0[0], theta[0], 0.3)
    return pp, D0, C0, D[None, :], C[None, :], theta, e0, np.array([lo]), np.array([hi]), np.array([eta_c]), np.array([eta_d])


@pytest.mark.parametrize("seed,T,band", [(1, 6, (0.0, 5.0)), (2, 5, (2.0, 2.0)), (3, 6, (1.0, 4.0)), (4, 4, (0.0, 5.0))])
def test_certificate_accepts_an_independent_solution_and_rejects_a_moved_one(seed, T, band):
    """The certificate on a storage QP solved by SciPy's SLSQP (polished on the active set it ends on, a linear solve):
    eta_c = 0.8, eta_d = 0.9, T <= 6, one storage. It must return <= 1e-7 there and > 1e-4 once one D entry is moved by 1e-3
    (the QP is strictly convex with curvature w = 1: a move of 1e-3 shifts a gradient by >= 1e-3)."""
    pp, D0, C0, D, C, theta, e0, lo, hi, ec, ed = _qp_case(seed, T, 0.8, 0.9, band)
    E = levels_eff(e0, ec, ed, D, C)
    assert D.min() >= -1e-9 and C.min() >= -1e-9 and D.max() <= 3.0 + 1e-9 and C.max() <= 3.0 + 1e-9
    assert E.min() >= -1e-9 and E.max() <= 5.0 + 1e-9 and lo[0] - 1e-9 <= E[0, -1] <= hi[0] + 1e-9
    v = storage_kkt_violation_eff(pp, D0, C0, D, C, theta, 0.3, e0, lo, hi, ec, ed)
    print(f"certificate on the polished SLSQP solution: {v:.2e}")
    assert v <= 1e-7, v
    free = np.flatnonzero((D[0] > 1e-3) & (D[0] < 3.0 - 2e-3))
    t = int(free[0]) if free.size else int(np.argmax(D[0] + C[0] > -1.0))
    D2 = D.copy()
    D2[0, t] += 1e-3 if D2[0, t] < 3.0 - 2e-3 else -1e-3
    v2 = storage_kkt_violation_eff(pp, D0, C0, D2, C, theta, 0.3, e0, lo, hi, ec, ed)
    assert v2 > 1e-4, v2


def test_certificate_at_unit_efficiency_is_the_band_certificate():
    """With eta = 1 the new certificate is helpers.storage_kkt_violation_band, number for number."""
    from helpers import storage_kkt_violation_band
    pp, D0, C0, D, C, theta, e0, lo, hi, ec, ed = _qp_case(7, 6, 1.0, 1.0, (0.0, 5.0))
    E = levels_eff(e0, ec, ed, D, C)
    rng = np.random.default_rng(0)
    for Dx in (D, D + rng.uniform(0, 1e-2, D.shape)):
        a = storage_kkt_violation_eff(pp, D0, C0, Dx, C, theta, 0.3, e0, lo, hi, ec, ed)
        b = storage_kkt_violation_band(pp, D0, C0, Dx, C, levels_eff(e0, ec, ed, Dx, C), theta, 0.3, lo, hi)
        assert a == b, (a, b)
    assert storage_kkt_violation_eff(pp, D0, C0, D, C, theta, 0.3, e0, lo, hi, ec, ed) <= 1e-7


def test_network_theta_from_psi_certifies_the_oracle_at_unit_efficiency():
    """helpers_efficiency.theta_of (Psi_{n,t} from the closed forms of DESIGN.md section 3, in NumPy) against code that shares
    nothing with it: the CPU oracle's exact mode on the 4x5 grid, lossless, from the zero state and from a seeded state. The
    certificate must accept the oracle's storages (<= 1e-7) and reject them under a wrong flow weight (> 1e-4)."""
    from oracle.binding import OracleApi
    from helpers import engine, set_from, state_of
    from helpers_efficiency import theta_of
    pp = synth.synthetic_case(n_gen=24, n_sto=8, T=12, seed=823, N=4, L=5, fmax_factor=0.7, fmax_min=5)
    g, one, zero = 0.03, np.ones(pp.S), np.zeros(pp.S)
    e = engine(OracleApi(build_oracle(), features=True), pp, 1, flags=0, eps=0.0, gamma=g)
    rng = np.random.default_rng(6)
    seeded = dict(P=rng.uniform(0, 1, (pp.G, pp.T)) * pp.gen_pmax[:, None], D=rng.uniform(0, 0.4, (pp.S, pp.T)) * pp.sto_pmax[:, None],
                  C=rng.uniform(0, 0.4, (pp.S, pp.T)) * pp.sto_pmax[:, None], avg_U=rng.uniform(0, 1, (pp.L, pp.T)),
                  avg_K=rng.uniform(0, 1, (pp.L, pp.T)), lam=rng.uniform(1, 30, pp.T), mu=rng.uniform(0, 1, (pp.L, pp.T)),
                  rho=rng.uniform(0, 1, (pp.L, pp.T)))
    rejected = 0
    for phase, n in (("zero", 3), ("seeded", 2)):
        if phase == "seeded":
            set_from(e, seeded, 2)
        for k in range(n):
            b = state_of(e)
            e.iterate(1)
            a = state_of(e)
            v = [storage_kkt_violation_eff(pp, b["D"], b["C"], a["D"], a["C"], theta_of(pp, b, e.get_duals_used(), a["D"], a["C"], g, wf),
                                           g, zero, zero, pp.sto_emax, one, one) for wf in (10.0, 5.0)]
            assert v[0] <= 1e-7, (phase, k, v)
            rejected += v[1] > 1e-4
    assert rejected >= 3
