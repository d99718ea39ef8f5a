"""Generator availability (DOPF_F_GEN_AVAILABILITY, dopf_set_generator_availability): the flag alone and all-ones profiles change
nothing on any chain, one x-update is min(P_unflagged, pmax * f) bit for bit, row skipping stays exact across a change of the caps,
the optimum against the central LP with the same caps, the refusals, a rolling horizon against the eager chain, and the multi-context
form. Needs a real MI355X: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import decentralopf_jl_amd as pkg
from decentralopf_jl_amd import _capi, synth
from decentralopf_jl_amd.central import solve_central_packed
from helpers import make_engine, state_of

pytestmark = pytest.mark.gpu

AV = _capi.F_GEN_AVAILABILITY
IL, TL, GEN, LH = _capi.F_STO_INITIAL_LEVEL, _capi.F_STO_TERMINAL_LEVEL, _capi.F_STO_GENERAL, _capi.F_LONG_HORIZON
NET = dict(N=4, L=5, seed=50, fmax_factor=0.7, fmax_min=5)
CP = dict(n_gen=600, n_sto=40, T=24, seed=601)
NETC = dict(n_gen=200, n_sto=40, T=24, **NET)

# (name, case, flags, gamma): every chain the generator bodies run on
CHAINS = [
    ("copper-one-launch-lean", CP, 0, 0.02),
    ("copper-one-launch-general", CP, GEN, 0.02),
    ("copper-no-tail-fuse", CP, _capi.F_NO_TAIL_FUSE, 0.02),
    ("copper-no-fuse", CP, _capi.F_NO_FUSE, 0.02),
    ("copper-no-fuse-no-skip", CP, _capi.F_NO_FUSE | _capi.F_NO_ROW_SKIP, 0.02),
    ("copper-generators-only", dict(n_gen=600, n_sto=0, T=24, seed=602), 0, 0.02),
    ("copper-odd-T", dict(n_gen=300, n_sto=20, T=25, seed=603), 0, 0.02),
    ("net", NETC, 0, 0.03),
    ("net-small-items", NETC, _capi.F_NET_SMALL_ITEMS, 0.03),
    ("net-no-quiet", NETC, _capi.F_NO_QUIET, 0.03),
    ("net-overlap", NETC, _capi.F_OVERLAP_AGENTS, 0.03),
    ("net-wide", NETC, _capi.F_DEBUG_WIDE_NET, 0.03),
    ("copper-long-T600", dict(n_gen=60, n_sto=6, T=600, seed=604), LH, 0.02),
    ("copper-levels", CP, IL | TL, 0.02),
]
IDS = [c[0] for c in CHAINS]


def bitwise(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, float(np.nanmax(np.abs(a[k] - b[k]))) if a[k].size else 0.0)


def draw_profiles(pp, K, seed, ones=False):
    """K profiles (K, T) in [0, 1] (exact binary fractions, some 0 and 1 entries) and an index per generator, some -1."""
    rng = np.random.default_rng(seed)
    prof = np.ones((K, pp.T)) if ones else np.round(rng.uniform(-0.2, 1.2, (K, pp.T)).clip(0.0, 1.0) * 64.0) / 64.0
    if K == pp.G:
        of = np.arange(pp.G, dtype=np.int32)
        of[::7] = -1
    else:
        of = rng.integers(-1, K, size=pp.G).astype(np.int32)
    return prof, of


def caps(pp, prof, of):
    f = np.ones((pp.G, pp.T))
    f[of >= 0] = prof[of[of >= 0]]
    return np.where((of >= 0)[:, None], pp.gen_pmax[:, None] * f, pp.gen_pmax[:, None])


def set_from(e, st, iteration):
    e.set_state(P=st["P"], D=st["D"], C_=st["C"], avg_U=st["avg_U"], avg_K=st["avg_K"], lam=st["lam"], mu=st["mu"],
                rho=st["rho"], iteration=iteration)


# ---- 1. the flag alone, and all-ones profiles, are the flagless run -------------------------------------------------------------

@pytest.mark.parametrize("name,case,flags,gamma", CHAINS, ids=IDS)
def test_flag_and_all_ones_are_the_flagless_run_bit_for_bit(hip_api, name, case, flags, gamma):
    pp = synth.synthetic_case(**case)
    runs = []
    for extra, ones in ((0, None), (AV, None), (AV, 3)):
        e = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=flags | extra)
        if ones:
            e.set_availability(*draw_profiles(pp, ones, 1, ones=True))
        e.iterate(200)
        runs.append(state_of(e))
        assert e.solver_failures() == 0
        e.close()
    bitwise(runs[0], runs[1], "flag")
    bitwise(runs[0], runs[2], "all ones")


# ---- 2. one x-update: P = min(P_unflagged, pmax * f), storages untouched -------------------------------------------------------

@pytest.mark.parametrize("name,case,flags,gamma", CHAINS, ids=IDS)
def test_one_x_update_is_the_clamped_flagless_update(hip_api, name, case, flags, gamma):
    pp = synth.synthetic_case(**case)
    src = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=flags)
    src.iterate(60)
    st = state_of(src)
    it = src.get_residuals()[3]
    src.close()
    a = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=flags)
    b = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=flags | AV)
    for K in (1, 3, pp.G):
        prof, of = draw_profiles(pp, K, 10 + K)
        b.set_availability(prof, of)
        set_from(a, st, it)
        set_from(b, st, it)
        a.iterate(1)
        b.iterate(1)
        sa, sb = state_of(a), state_of(b)
        cap = caps(pp, prof, of)
        assert np.array_equal(sb["P"], np.minimum(sa["P"], cap)), K
        assert np.all(sb["P"] <= cap) and np.all(sb["P"] >= 0.0)
        for k in ("D", "C", "E"):
            assert np.array_equal(sa[k], sb[k]), (K, k)
    assert a.solver_failures() == 0 and b.solver_failures() == 0


# ---- 3. row skipping stays exact when the caps change mid-run --------------------------------------------------------------------

@pytest.mark.parametrize("scale", [0.25, 1.0], ids=["fused-skip", "separate-skip"])
def test_row_skipping_stays_exact_across_a_change_of_the_caps(hip_api, scale):
    a_ = int(1000000 * scale)
    pp = synth.synthetic_case(a_ - a_ // 11, a_ // 11, 24, availability=0.25)
    g = 1.0 / (pp.G + pp.S)
    a = make_engine(hip_api, pp, eps=0.0, gamma=g)
    b = make_engine(hip_api, pp, eps=0.0, gamma=g, flags=_capi.F_NO_ROW_SKIP)
    assert a.params.flags & AV and b.params.flags & AV
    prof2 = pp.gen_avail.copy()
    prof2[0] = np.roll(prof2[0], 3)                         # the sun three hours later,
    prof2[1:] = np.round(prof2[1:] * 0.75 * 1024.0) / 1024.0   # less wind
    for step, (n, change) in enumerate(((1, None), (40, None), (1, prof2), (20, None), (1, pp.gen_avail), (20, None))):
        if change is not None:
            Pa = a.get_primal()[0]
            at_cap = (Pa == caps(pp, pp.gen_avail if change is prof2 else prof2, pp.gen_avail_of)).all(axis=1)
            assert at_cap.mean() > 0.05, at_cap.mean()       # rows whose summary is "all at cap" exist when the caps change
            a.set_availability(change, pp.gen_avail_of)
            b.set_availability(change, pp.gen_avail_of)
        a.iterate(n)
        b.iterate(n)
        sa, sb = state_of(a), state_of(b)
        bitwise(sa, sb, step)
        assert a.get_residuals() == b.get_residuals()
    assert a.solver_failures() == 0 and b.solver_failures() == 0


# ---- 4. the optimum -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,share,wf", [(dict(n_gen=300, n_sto=30, T=24, seed=611), 0.25, None),
                                           (dict(n_gen=300, n_sto=30, T=12, N=12, L=18, seed=23, fmax_factor=2.0, fmax_min=20), 0.1, 0.3)],
                         ids=["copper", "net"])
def test_optimum_matches_the_central_lp_with_the_same_caps(hip_api, case, share, wf):
    pp = synth.synthetic_case(**case, availability=share)
    A = pp.G + pp.S
    kw = dict(eps=1e-3, gamma=1.0 / A)
    if wf is not None:
        kw["w_flow"] = wf / A
    e = make_engine(hip_api, pp, **kw)
    assert e.params.flags & AV
    done, conv = e.iterate(20000)
    assert conv, (done, e.get_residuals())
    cost = e.get_consensus()[4]
    lp = solve_central_packed(pp).objective
    assert abs(cost - lp) <= 1e-3 * abs(lp), (cost, lp)
    P = e.get_primal()[0]
    assert np.all(P <= caps(pp, pp.gen_avail, pp.gen_avail_of)) and np.all(P >= 0.0)
    assert e.solver_failures() == 0


def test_three_node_with_a_pv_profile_converges_to_its_lp(hip_api):
    nodes, lines, gens, stos = pkg.three_node_case()
    gens[0].availability = [1.0, 0.875]
    lp = solve_central_packed(pkg.pack(nodes, gens, stos, lines)).objective
    assert abs(lp - 14825.0) <= 1e-6 * lp
    admm = pkg.ADMM(0.3, nodes, gens, stos, lines, record=False, max_iters=20000, w_flow=10.0)
    assert admm.engine.params.flags & AV
    pkg.run(admm)
    assert admm.convergence.all, admm.iteration
    cost = admm.engine.get_consensus()[4]
    assert abs(cost - lp) <= 1e-3 * lp, (cost, lp)
    assert admm.engine.get_primal()[0][0, 1] <= 70.0


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_store_nothing(hip_api):
    pp = synth.synthetic_case(n_gen=60, n_sto=6, T=24, seed=621)
    plain = make_engine(hip_api, pp, eps=0.0, gamma=0.02)
    prof, of = draw_profiles(pp, 2, 5)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    flat = np.ascontiguousarray(prof).ravel()
    assert hip_api.set_generator_availability(plain._ctx, 2, dp(flat), ip(of)) == -4          # DOPF_E_UNSUPPORTED
    a = make_engine(hip_api, pp, eps=0.0, gamma=0.02, flags=AV)
    b = make_engine(hip_api, pp, eps=0.0, gamma=0.02, flags=AV)
    a.set_availability(prof, of)
    b.set_availability(prof, of)
    a.iterate(30)
    b.iterate(30)
    bad = []
    for v in (np.nan, 1.5, -0.25):
        p = flat.copy()
        p[7] = v
        bad.append((2, p, of))
    for k in (2, -2):
        o = of.copy()
        o[3] = k
        bad.append((2, flat, o))
    for K, p, o in bad:
        assert hip_api.set_generator_availability(a._ctx, K, dp(p), ip(o)) == -1              # DOPF_E_INVALID
    assert hip_api.set_generator_availability(a._ctx, -1, None, None) == -1
    assert hip_api.set_generator_availability(a._ctx, 2, None, ip(of)) == -1
    assert hip_api.set_generator_availability(a._ctx, 2, dp(flat), None) == -1
    msg = hip_api.last_error(a._ctx).decode()
    assert "profile_of" in msg, msg
    a.iterate(30)
    b.iterate(30)
    bitwise(state_of(a), state_of(b), "refusals")
    # the multi form refuses before it stores anything, in any shard
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(eps=0.0, gamma=0.02, flags=_capi.F_COMM_HOST | AV),
                          **pp.engine_kwargs())
    o = of.copy()
    o[-1] = 9
    assert hip_api.multi_set_generator_availability(m._m, 2, dp(flat), ip(o)) == -1
    m.close()


# ---- 6. a rolling horizon: profiles set between calls, the table grown, against the eager chain -------------------------------

@pytest.mark.parametrize("case,gamma", [(CP, 0.02), (NETC, 0.03)], ids=["copper", "net"])
def test_rolling_horizon_matches_the_eager_chain(hip_api, case, gamma):
    pp = synth.synthetic_case(**case)
    a = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=AV)
    b = make_engine(hip_api, pp, eps=0.0, gamma=gamma, flags=AV | _capi.F_NO_GRAPH)
    plan = [(1, 30), (2, 25), (2, 25), (5, 40), (0, 20), (3, 30)]     # K = 5 grows the table beyond its allocation of 2
    for i, (K, n) in enumerate(plan):
        if K:
            prof, of = draw_profiles(pp, K, 100 + i)
            a.set_availability(prof, of)
            b.set_availability(prof, of)
        else:
            a.set_availability(None, None)
            b.set_availability(None, None)
        a.iterate(n)
        b.iterate(n)
        bitwise(state_of(a), state_of(b), i)
    assert a.solver_failures() == 0 and b.solver_failures() == 0


# ---- 7. the multi-context form ---------------------------------------------------------------------------------------------------

def test_multi_context_matches_one_context(hip_api):
    pp = synth.synthetic_case(n_gen=300, n_sto=30, T=24, seed=631, availability=0.25)
    g = 1.0 / (pp.G + pp.S)
    ref = make_engine(hip_api, pp, eps=0.0, gamma=g)
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(eps=0.0, gamma=g, flags=_capi.F_COMM_HOST), **pp.engine_kwargs())
    assert m.params.flags & AV
    prof2, of2 = draw_profiles(pp, 4, 7)
    for k, change in ((1, None), (7, None), (30, (prof2, of2)), (30, None)):
        if change is not None:
            ref.set_availability(*change)
            m.set_availability(*change)
        ref.iterate(k)
        assert m.iterate(k) == (k, False)
        want = state_of(ref)
        P, D, C, E = m.get_primal()
        for x, y in zip((P, D, C, E), (want["P"], want["D"], want["C"], want["E"])):
            assert np.abs(x - y).max() <= 1e-9 * max(1.0, np.abs(y).max())
        got = state_of(m.shard(1))
        for key in ("lam", "inj", "cost"):
            assert np.abs(got[key] - want[key]).max() <= 1e-9 * max(1.0, np.abs(want[key]).max()), key
    m.close()
