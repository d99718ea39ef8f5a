"""Generator availability (DOPF_F_GEN_AVAILABILITY) at the boundary: the header, the exports, the ctypes signatures, the Julia
shim, network.Generator / pack / engine_kwargs / shard, the synthetic profiles, the oracle API's refusal, and the central LP with
per-timestep generator caps. No compute calls on a device (runs without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg
from decentralopf_jl_amd import _capi, central, synth
from decentralopf_jl_amd.network import Generator

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
ENTRY = ("dopf_set_generator_availability", "dopf_multi_set_generator_availability")
BASE_KEYS = {"N", "L", "T", "demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax",
             "sto_node"}


def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_defines_the_flag():
    m = re.search(r"#define\s+DOPF_F_GEN_AVAILABILITY\s+(\d+)", HDR)
    assert m and int(m.group(1)) == 1 << 27 == 134217728 == _capi.F_GEN_AVAILABILITY
    others = [int(v) for k, v in re.findall(r"#define\s+(DOPF_F_\w+)\s+(\d+)", HDR) if k != "DOPF_F_GEN_AVAILABILITY"]
    assert others and all(v & (1 << 27) == 0 for v in others)


def test_header_declares_both_entry_points():
    rest = ["int32_t n_profiles", "const double *profiles", "const int32_t *profile_of"]
    assert _prototype("dopf_set_generator_availability") == ["dopf_ctx *ctx"] + rest
    assert _prototype("dopf_multi_set_generator_availability") == ["dopf_multi *m"] + rest
    for name in ENTRY:          # exactly as the issue of the feature spells them
        assert re.search(r"^int %s\(%s \*\w+, int32_t n_profiles, const double \*profiles, const int32_t \*profile_of\);$"
                         % (name, "dopf_multi" if "multi" in name else "dopf_ctx"), HDR, re.M), name


def test_library_exports_both_entry_points():
    assert os.path.exists(_capi.HIP_LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_capi.HIP_LIB_PATH)
    for name in ENTRY:
        assert hasattr(lib, name), name


def test_ctypes_signatures_match_the_header():
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for name in ("set_generator_availability", "multi_set_generator_availability"):
        f = getattr(api, name)
        assert f.restype is ctypes.c_int
        assert len(f.argtypes) == 4
        assert f.argtypes[1] is ctypes.c_int32
        assert f.argtypes[2] is ctypes.POINTER(ctypes.c_double) and f.argtypes[3] is ctypes.POINTER(ctypes.c_int32)


def test_julia_shim_defines_the_flag_and_the_setter():
    m = re.search(r"^const DOPF_F_GEN_AVAILABILITY = (\d+)", JL, re.M)
    assert m and int(m.group(1)) == _capi.F_GEN_AVAILABILITY
    assert re.search(r"^function set_availability!\(admm::ADMM", JL, re.M)
    for name in ENTRY:
        assert re.search(r"ccall\(\(:%s, DOPF_LIB\), Cint, \(Ptr\{Cvoid\}, Cint, Ptr\{Cdouble\}, Ptr\{Cint\}\)" % name, JL), name


def test_generator_default_leaves_the_engine_arguments_unchanged(three_node):
    nodes, lines, gens, stos, pp = three_node
    assert all(g.availability is None for g in gens)
    assert pp.gen_avail is None and pp.gen_avail_of is None and not pp.has_availability()
    assert set(pp.engine_kwargs()) == BASE_KEYS
    prof, of = pp.availability()
    assert prof.shape == (0, 2) and np.array_equal(of, [-1, -1, -1, -1])


def _three_node_with(profiles):
    nodes, lines, gens, stos = pkg.three_node_case()
    for g in gens:
        if g.name in profiles:
            g.availability = profiles[g.name]
    return nodes, lines, gens, stos


def test_pack_deduplicates_identical_series():
    nodes, lines, gens, stos = _three_node_with({"pv": [1.0, 0.25], "wind": [0.5, 0.75], "gas": [1.0, 0.25]})
    pp = pkg.pack(nodes, gens, stos, lines)
    assert pp.gen_avail.shape == (2, 2)                      # three generators, two distinct series
    assert np.array_equal(pp.gen_avail, [[1.0, 0.25], [0.5, 0.75]])
    assert np.array_equal(pp.gen_avail_of, [0, 1, -1, 0]) and pp.gen_avail_of.dtype == np.int32
    kw = pp.engine_kwargs()
    assert set(kw) == BASE_KEYS | {"gen_avail", "gen_avail_of"}
    assert np.array_equal(kw["gen_avail"], pp.gen_avail) and np.array_equal(kw["gen_avail_of"], pp.gen_avail_of)


def test_pack_refuses_bad_series():
    for bad in ([1.0], [1.0, 1.5], [-0.1, 1.0], [float("nan"), 1.0]):
        nodes, lines, gens, stos = _three_node_with({"pv": bad})
        with pytest.raises(ValueError):
            pkg.pack(nodes, gens, stos, lines)


def test_shard_slices_the_indices_and_replicates_the_table():
    pp = synth.synthetic_case(20, 7, 24, seed=5, availability=0.25)
    assert pp.gen_avail.shape == (3, 24) and np.any(pp.gen_avail_of >= 0) and np.any(pp.gen_avail_of == -1)
    for world in (2, 3):
        parts = [pp.shard(r, world) for r in range(world)]
        assert np.array_equal(np.concatenate([p.gen_avail_of for p in parts]), pp.gen_avail_of)
        for p in parts:
            g0, g1 = p.meta["gen_range"]
            assert np.array_equal(p.gen_avail_of, pp.gen_avail_of[g0:g1])
            assert np.array_equal(p.gen_avail, pp.gen_avail)


def test_synthetic_profiles_are_seeded_and_leave_the_case_of_before():
    a = synth.synthetic_case(300, 30, 48, seed=9, availability=0.25)
    b = synth.synthetic_case(300, 30, 48, seed=9, availability=0.25)
    plain = synth.synthetic_case(300, 30, 48, seed=9)
    assert np.array_equal(a.gen_avail, b.gen_avail) and np.array_equal(a.gen_avail_of, b.gen_avail_of)
    for k in ("gen_mc", "gen_pmax", "sto_mc", "sto_pmax", "demand"):
        assert np.array_equal(getattr(a, k), getattr(plain, k)), k
    assert plain.gen_avail is None and set(plain.engine_kwargs()) == BASE_KEYS
    solar = a.gen_avail[0]
    assert solar[(np.arange(48) % 24) <= 6].max() == 0.0 and solar.max() == 1.0        # 0 at night
    assert a.gen_avail.min() >= 0.0 and a.gen_avail.max() <= 1.0
    assert abs((a.gen_avail_of >= 0).mean() - 0.25) < 0.01
    f = np.ones((a.G, a.T))
    f[a.gen_avail_of >= 0] = a.gen_avail[a.gen_avail_of[a.gen_avail_of >= 0]]
    assert np.all((a.gen_pmax[:, None] * f).sum(axis=0) >= a.demand.sum(axis=0))      # feasible at every timestep


def test_oracle_api_refuses_a_non_default_profile(three_node, oracle_api):
    *_, pp = three_node
    assert not hasattr(oracle_api, "set_generator_availability")
    for prof, of in (([[1.0, 0.25]], [0, -1, -1, -1]), ([[0.5, 0.5]], [-1, 0, -1, -1]), ([[1.0, 1.0], [0.0, 0.0]], [1, -1, -1, -1])):
        with pytest.raises(_capi.DopfError, match="availability"):
            _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, gen_avail=prof, gen_avail_of=of, **pp.engine_kwargs())
    # all-ones profiles and unused profiles are what the oracle computes anyway: accepted, no flag
    for prof, of in (([[1.0, 1.0]], [0, 0, -1, 0]), ([[0.5, 0.5]], [-1, -1, -1, -1])):
        e = _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, gen_avail=prof, gen_avail_of=of, **pp.engine_kwargs())
        assert e.params.flags & _capi.F_GEN_AVAILABILITY == 0
        e.close()


def test_central_lp_all_ones_is_the_reference_optimum(three_node):
    *_, pp = three_node
    ones = (np.ones((1, 2)), np.zeros(4, dtype=np.int32))
    r = central.solve_central_packed(pp, availability=ones)
    assert abs(r.objective - 14035.0) <= 1e-6 * 14035.0, r.objective
    assert abs(central.solve_central_packed(pp).objective - 14035.0) <= 1e-6 * 14035.0


def test_central_lp_constant_pv_profile_is_a_smaller_nameplate():
    # independent construction: pv at 7/8 of its availability is pv with max_generation 70 (at one half, 40, node N1 cannot meet
    # its demand of 250 at t = 2 through lines L1 and L2: the LP is infeasible either way)
    nodes, lines, gens, stos = pkg.three_node_case()
    pp = pkg.pack(nodes, gens, stos, lines)
    half = central.solve_central_packed(pp, availability=(np.full((1, 2), 0.875), np.array([0, -1, -1, -1], dtype=np.int32)))
    gens[0].max_generation = 70
    small = central.solve_central_packed(pkg.pack(nodes, gens, stos, lines))
    assert abs(half.objective - small.objective) <= 1e-9 * small.objective, (half.objective, small.objective)
    assert half.objective > 14035.0 + 1.0
    assert half.generation[0].max() <= 70.0 + 1e-9


def test_central_lp_takes_the_profiles_from_the_generators():
    nodes, lines, gens, stos = _three_node_with({"pv": [1.0, 0.875]})
    pp = pkg.pack(nodes, gens, stos, lines)
    r = central.solve_central_packed(pp)
    assert abs(r.objective - 14825.0) <= 1e-6 * 14825.0, r.objective          # (HiGHS; 14035 without the profile)
    assert r.generation[0, 1] <= 80.0 * 0.875 + 1e-9
    # an explicit availability wins over the packed one
    ones = (np.ones((1, 2)), np.zeros(4, dtype=np.int32))
    assert abs(central.solve_central_packed(pp, availability=ones).objective - 14035.0) <= 1e-6 * 14035.0
