"""Storage charge / discharge efficiencies (DOPF_F_STO_EFFICIENCY) on the device. The CPU oracle takes efficiencies
since (oracle_set_storage_efficiency), and every chain is compared with it value for value at eta < 1 in
tests/test_gpu_lossy_rated_parity.py; this file, written before, pins the ground four ways without them: (i) the oracle's exact mode at eta = 1, one step at a time; (ii) an exact KKT certificate
in NumPy at eta < 1 (helpers_efficiency.storage_kkt_violation_eff; on networks its theta comes from Psi_{n,t} evaluated in NumPy
from the closed forms of DESIGN.md section 3, helpers_efficiency.theta_of); (iii) the identity that normalises the discharge efficiency away (copper plate and network); (iv) the HiGHS LP with
lossy balance rows at convergence. Bounds: test 1 the one-step bound of tests/test_gpu_feature_parity.py (1e-9 scaled on copper
plates, 1e-8 on networks), the bodies and the normalisation 1e-9 scaled everywhere, the roll's of tests/test_gpu_horizon_roll.py, the shards' of tests/test_gpu_multi.py, 1e-3 relative to the LP.
Needs a real MI355X: pytest -m gpu."""
import copy

import numpy as np
import pytest

from conftest import build_oracle, pkg
from decentralopf_jl_amd import _capi, central, synth
from decentralopf_jl_amd.horizon import shift_window
from helpers import Features, degenerate, draw_e0, engine, max_diff, set_from, state_of
from helpers_efficiency import draw_band_eff, draw_eta, levels_eff, storage_kkt_violation_eff, theta_of

pytestmark = pytest.mark.gpu

EF, IL, TL, AV = _capi.F_STO_EFFICIENCY, _capi.F_STO_INITIAL_LEVEL, _capi.F_STO_TERMINAL_LEVEL, _capi.F_GEN_AVAILABILITY
NET = dict(N=4, L=5, fmax_factor=0.7, fmax_min=5)


@pytest.fixture(scope="module")
def fapi():
    from oracle.binding import OracleApi
    return OracleApi(build_oracle(), features=True)


def three_node_pp():
    nodes, lines, gens, stos = pkg.three_node_case()
    return pkg.pack(nodes, gens, stos, lines)


def case_pp(case):
    return three_node_pp() if case == "three-node" else synth.synthetic_case(**case)


def scaled(sh, so):
    scale = max(1.0, float(np.abs(so["lam"]).max()))
    worst, where = max_diff(sh, so, keys=[k for k in sh if k != "cost"])
    return worst / scale, where, abs(float(sh["cost"][0] - so["cost"][0])) / max(1.0, abs(float(so["cost"][0])))


def seeded_state(pp, seed):
    """a state for dopf_set_state that no run produced: (D, C) inside their boxes, random duals"""
    rng = np.random.default_rng(seed)
    return dict(P=rng.uniform(0, 1, (pp.G, pp.T)) * pp.gen_pmax[:, None], D=rng.uniform(0, 0.4, (pp.S, pp.T)) * pp.sto_pmax[:, None],
                C=rng.uniform(0, 0.4, (pp.S, pp.T)) * pp.sto_pmax[:, None], avg_U=rng.uniform(0, 1, (pp.L, pp.T)),
                avg_K=rng.uniform(0, 1, (pp.L, pp.T)), lam=rng.uniform(1, 30, pp.T), mu=rng.uniform(0, 1, (pp.L, pp.T)),
                rho=rng.uniform(0, 1, (pp.L, pp.T)))


def step(e, pair=False):
    if pair:        # the sharded form at world 1
        e.local_update()
        e.apply_consensus()
    else:
        e.iterate(1)


# ---- 1. the oracle anchor at eta = 1 ------------------------------------------------------------------------------------------
CP24 = dict(n_gen=40, n_sto=24, T=24, seed=801)
N45 = dict(n_gen=24, n_sto=8, T=12, seed=806, **NET)
ANCHOR = [
    # name, case, extra flags, (e0, band, profiles), degenerate, gamma, setter called with ones, local_update/apply_consensus pair
    ("copper-T24", CP24, 0, ("mix", "mix", "K3"), "emax0", 0.02, False, False),
    ("copper-T24-flag-alone", CP24, 0, (None, None, None), "pmax0", 0.02, True, False),
    ("copper-T13-ragged", dict(n_gen=16, n_sto=11, T=13, seed=802), 0, ("inside", "eq", None), "", 0.02, True, False),
    ("copper-T96", dict(n_gen=16, n_sto=9, T=96, seed=803), 0, ("mix", "cyclic", "K1"), "", 0.02, False, False),
    ("copper-T200-scan", dict(n_gen=12, n_sto=5, T=200, seed=804), 0, ("mix", "mix", None), "emax0", 0.02, True, False),
    ("three-node", "three-node", 0, (None, None, None), "", 0.3, True, False),
    ("net-4x5-T12", N45, 0, ("mix", "mix", "K3"), "emax0", 0.03, False, False),
    ("copper-no-fuse", CP24, _capi.F_NO_FUSE, ("inside", "eq", None), "", 0.02, True, False),
    ("copper-no-tail-fuse", CP24, _capi.F_NO_TAIL_FUSE, ("mix", "cyclic", None), "", 0.02, False, False),
    ("net-no-quiet", N45, _capi.F_NO_QUIET, ("inside", "eq", None), "", 0.03, True, False),
    ("net-debug-wide", N45, _capi.F_DEBUG_WIDE_NET, ("mix", "mix", None), "", 0.03, False, False),
    ("copper-local-update-pair", CP24, 0, ("mix", "mix", None), "", 0.02, True, True),
    ("net-local-update-pair", N45, 0, ("inside", "cyclic", None), "", 0.03, False, True),
]


@pytest.mark.parametrize("name,case,extra,feat,degen,gamma,ones,pair", ANCHOR, ids=[r[0] for r in ANCHOR])
def test_unit_efficiency_follows_the_oracle(hip_api, fapi, name, case, extra, feat, degen, gamma, ones, pair):
    """Contexts with the flag (setter not called / called with ones) against the oracle's exact mode with the same e0, band and
    profiles: 4 iterations from the zero state, 2 from a seeded dopf_set_state, the HIP state reset to the oracle's after each."""
    pp = degenerate(case_pp(case), degen)
    feats = Features(pp, *feat, seed=11)
    h = engine(hip_api, pp, None, flags=feats.flags | EF | extra, eps=0.0, gamma=gamma)
    o = engine(fapi, pp, 1, flags=feats.flags, eps=0.0, gamma=gamma)
    for e in (h, o):
        feats.apply(e)
    if ones:
        h.set_efficiency(np.ones(pp.S), np.ones(pp.S))
    tol = 1e-9 if pp.L == 0 else 1e-8
    worst = 0.0
    for phase, iters in (("zero", 4), ("seeded", 2)):
        if phase == "seeded":
            st = seeded_state(pp, 5)
            set_from(h, st, 2)
            set_from(o, st, 2)
        for k in range(iters):
            step(h, pair)
            o.iterate(1)
            w, where, cost = scaled(state_of(h), state_of(o))
            assert w <= tol and cost <= 1e-9, (phase, k, where, w, cost)
            worst = max(worst, w)
            set_from(h, state_of(o), o.get_residuals()[3])
    assert h.solver_failures() == 0
    print(f"{name}: worst one-step difference {worst:.2e} (scaled)")


# ---- 2. the certificate at eta < 1 ---------------------------------------------------------------------------------------------
def lossy_setup(pp, e0kind, bandkind, seed):
    rng = np.random.default_rng(seed)
    ec, ed = draw_eta(pp.S, rng)
    if pp.S == 1:                       # (the three-node case's one battery: not the draw's (1, 1))
        ec, ed = np.array([0.8]), np.array([0.9])
    e0 = draw_e0(pp, e0kind, rng)
    lo, hi = draw_band_eff(pp, e0, ec, ed, bandkind, rng)
    return ec, ed, e0, lo, hi


def lossy_engine(api, pp, ec, ed, e0, lo, hi, extra=0, gamma=0.02):
    e = engine(api, pp, None, flags=EF | IL | TL | extra, eps=0.0, gamma=gamma)
    e.set_efficiency(ec, ed)
    e.set_initial_levels(e0)
    e.set_terminal_levels(lo, hi)
    return e


def certified_steps(e, pp, n, gamma, ec, ed, e0, lo, hi, pair=False, w_flow=10.0):
    for k in range(n):
        before = state_of(e)
        step(e, pair)
        after = state_of(e)
        D, C, E = after["D"], after["C"], after["E"]
        assert np.abs(E - levels_eff(e0, ec, ed, D, C)).max() <= 1e-9, k
        assert E.min() >= -1e-9 and (E - pp.sto_emax[:, None]).max() <= 1e-9, k
        assert (lo - E[:, -1]).max() <= 1e-9 and (E[:, -1] - hi).max() <= 1e-9, k
        theta = theta_of(pp, before, e.get_duals_used(), D, C, gamma, w_flow)
        if pp.L == 0:                   # (the copper plate's closed form, as the other certificates' tests build it)
            closed = e.get_duals_used()[0][None, :] + gamma * (before["inj"].sum(axis=0)[None, :] - (before["D"] - before["C"]))
            assert np.abs(theta - closed).max() <= 1e-9 * max(1.0, np.abs(closed).max())
        viol = storage_kkt_violation_eff(pp, before["D"], before["C"], D, C, theta, gamma, e0, lo, hi, ec, ed)
        assert viol <= 1e-7, (k, viol)
    assert e.solver_failures() == 0


CERT = [
    ("copper-T24", dict(n_gen=40, n_sto=24, T=24, seed=811), 0, "inside", "eq", "emax0"),
    ("copper-T24-full-cyclic", dict(n_gen=40, n_sto=24, T=24, seed=812), 0, "full", "cyclic", "pmax0"),
    ("copper-T13-ragged", dict(n_gen=16, n_sto=11, T=13, seed=813), 0, "0", "default", ""),
    ("copper-T96", dict(n_gen=16, n_sto=9, T=96, seed=814), 0, "inside", "cyclic", "emax0+pmax0"),
    ("copper-T200-scan", dict(n_gen=12, n_sto=5, T=200, seed=815), 0, "inside", "eq", ""),
    ("copper-no-fuse", dict(n_gen=40, n_sto=24, T=24, seed=816), _capi.F_NO_FUSE, "0", "eq", ""),
    ("copper-no-tail-fuse", dict(n_gen=40, n_sto=24, T=24, seed=817), _capi.F_NO_TAIL_FUSE, "full", "default", ""),
    ("copper-no-warm", dict(n_gen=40, n_sto=24, T=24, seed=818), _capi.F_NO_WARM_START, "inside", "eq", "emax0"),
    ("copper-debug-leave", dict(n_gen=40, n_sto=24, T=24, seed=819), _capi.F_DEBUG_LEAVE, "inside", "cyclic", ""),
    ("copper-T24-debug-long", dict(n_gen=40, n_sto=24, T=24, seed=820), _capi.F_DEBUG_LONG_STO, "inside", "eq", "pmax0"),
    ("copper-T70-debug-long", dict(n_gen=16, n_sto=7, T=70, seed=821), _capi.F_DEBUG_LONG_STO, "0", "default", ""),
    ("copper-local-update-pair", dict(n_gen=40, n_sto=24, T=24, seed=822), 0, "inside", "eq", ""),
    # networks: theta from Psi_{n,t} in NumPy
    ("three-node", "three-node", 0, "0", "default", ""),
    ("three-node-inside-eq", "three-node", 0, "inside", "eq", ""),
    ("net-4x5-T12", dict(n_gen=24, n_sto=8, T=12, seed=823, **NET), 0, "inside", "eq", "emax0"),
    ("net-4x5-T12-cyclic", dict(n_gen=24, n_sto=8, T=12, seed=824, **NET), 0, "full", "cyclic", "pmax0"),
    ("net-no-fuse", dict(n_gen=24, n_sto=8, T=12, seed=825, **NET), _capi.F_NO_FUSE, "0", "default", ""),
    ("net-no-tail-fuse", dict(n_gen=24, n_sto=8, T=12, seed=826, **NET), _capi.F_NO_TAIL_FUSE, "inside", "eq", ""),
    ("net-no-quiet", dict(n_gen=24, n_sto=8, T=12, seed=827, **NET), _capi.F_NO_QUIET, "inside", "eq", ""),
    ("net-debug-wide", dict(n_gen=24, n_sto=8, T=12, seed=828, **NET), _capi.F_DEBUG_WIDE_NET, "inside", "cyclic", ""),
    ("net-no-warm", dict(n_gen=24, n_sto=8, T=12, seed=829, **NET), _capi.F_NO_WARM_START, "inside", "eq", ""),
    ("net-debug-leave", dict(n_gen=24, n_sto=8, T=12, seed=831, **NET), _capi.F_DEBUG_LEAVE, "inside", "eq", ""),
    ("net-debug-long", dict(n_gen=24, n_sto=8, T=12, seed=832, **NET), _capi.F_DEBUG_LONG_STO, "inside", "eq", ""),
    ("net-local-update-pair", dict(n_gen=24, n_sto=8, T=12, seed=833, **NET), 0, "inside", "eq", ""),
]


@pytest.mark.parametrize("name,case,extra,e0kind,bandkind,degen", CERT, ids=[r[0] for r in CERT])
def test_lossy_storages_pass_the_certificate(hip_api, name, case, extra, e0kind, bandkind, degen):
    pp = degenerate(case_pp(case), degen)
    seed = 810 if case == "three-node" else case["seed"]
    gamma = 0.3 if case == "three-node" else (0.02 if pp.L == 0 else 0.03)
    pair = name.endswith("pair")
    ec, ed, e0, lo, hi = lossy_setup(pp, e0kind, bandkind, seed)
    e = lossy_engine(hip_api, pp, ec, ed, e0, lo, hi, extra, gamma)
    certified_steps(e, pp, 4, gamma, ec, ed, e0, lo, hi, pair)
    set_from(e, seeded_state(pp, 6), 2)
    certified_steps(e, pp, 2, gamma, ec, ed, e0, lo, hi, pair)


def test_lossy_long_horizon_crosses_a_tile(hip_api):
    """DOPF_F_LONG_HORIZON, T = 2100 (past the long body's 2048-step tile), 3 storages, 2 iterations, the certificate."""
    pp = synth.synthetic_case(n_gen=8, n_sto=3, T=2100, seed=830)
    ec, ed, e0, lo, hi = lossy_setup(pp, "inside", "eq", 830)
    e = lossy_engine(hip_api, pp, ec, ed, e0, lo, hi, _capi.F_LONG_HORIZON)
    certified_steps(e, pp, 2, 0.02, ec, ed, e0, lo, hi)


# ---- 3. the bodies agree --------------------------------------------------------------------------------------------------------
BODIES = [("copper-T24", dict(n_gen=40, n_sto=24, T=24, seed=840), 0.02, (_capi.F_NO_WARM_START, _capi.F_DEBUG_LEAVE, _capi.F_DEBUG_LONG_STO)),
          ("copper-T70", dict(n_gen=16, n_sto=7, T=70, seed=841), 0.02, (_capi.F_NO_WARM_START, _capi.F_DEBUG_LEAVE, _capi.F_DEBUG_LONG_STO)),
          ("net-4x5-T12", dict(n_gen=24, n_sto=8, T=12, seed=842, **NET), 0.03, (_capi.F_NO_WARM_START, _capi.F_DEBUG_LEAVE, _capi.F_DEBUG_LONG_STO)),
          ("net-4x5-T24-wide", dict(n_gen=24, n_sto=8, T=24, seed=843, **NET), 0.03, (_capi.F_DEBUG_WIDE_NET, _capi.F_NO_QUIET))]


@pytest.mark.parametrize("name,case,gamma,variants", BODIES, ids=[r[0] for r in BODIES])
def test_the_storage_bodies_agree(hip_api, name, case, gamma, variants):
    """the scan body alone, the hand-over in every variant, the long body and the other chains against the default of the flag:
    P, D, C, E and the duals after 3 iterations"""
    pp = synth.synthetic_case(**case)
    ec, ed, e0, lo, hi = lossy_setup(pp, "inside", "eq", case["seed"])
    ref = lossy_engine(hip_api, pp, ec, ed, e0, lo, hi, 0, gamma)
    ref.iterate(3)
    want = state_of(ref)
    tol = 1e-9
    for extra in variants:
        e = lossy_engine(hip_api, pp, ec, ed, e0, lo, hi, extra, gamma)
        e.iterate(3)
        w, where, cost = scaled(state_of(e), want)
        assert w <= tol and cost <= 1e-9, (extra, where, w, cost)
        assert e.solver_failures() == 0


# ---- 4. normalising the discharge efficiency away ------------------------------------------------------------------------------
@pytest.mark.parametrize("case,gamma", [(dict(n_gen=40, n_sto=24, T=24, seed=850), 0.02), (dict(n_gen=24, n_sto=8, T=12, seed=851, **NET), 0.03)],
                         ids=["copper-T24", "net-4x5-T12"])
def test_discharge_efficiency_normalises_away(hip_api, case, gamma):
    """(eta_c, eta_d, emax, e0, lo, hi) and (eta_c eta_d, 1, emax eta_d, e0 eta_d, lo eta_d, hi eta_d) — the balance divided by
    al = 1 / eta_d — give the same D, C, P and duals over 5 iterations, and levels that differ by the factor eta_d."""
    pp = synth.synthetic_case(**case)
    ec, ed, e0, lo, hi = lossy_setup(pp, "inside", "eq", case["seed"])
    a = lossy_engine(hip_api, pp, ec, ed, e0, lo, hi, 0, gamma)
    pp2 = copy.copy(pp)
    pp2.sto_emax = pp.sto_emax * ed
    b = lossy_engine(hip_api, pp2, ec * ed, np.ones(pp.S), e0 * ed, lo * ed, hi * ed, 0, gamma)
    tol = 1e-9
    for k in range(5):
        a.iterate(1)
        b.iterate(1)
        sa, sb = state_of(a), state_of(b)
        sb["E"] = sb["E"] / ed[:, None]
        w, where, cost = scaled(sa, sb)
        assert w <= tol and cost <= 1e-9, (k, where, w, cost)
    assert a.solver_failures() == 0 and b.solver_failures() == 0


# ---- 5. the setter ---------------------------------------------------------------------------------------------------------------
def test_setter_refusals_store_nothing(hip_api):
    pp = synth.synthetic_case(n_gen=20, n_sto=6, T=24, seed=860)
    ec, ed, e0, lo, hi = lossy_setup(pp, "inside", "eq", 860)
    e = lossy_engine(hip_api, pp, ec, ed, e0, lo, hi)
    twin = lossy_engine(hip_api, pp, ec, ed, e0, lo, hi)
    e.iterate(2)
    twin.iterate(2)
    bad = []
    for i, x in ((0, float("nan")), (1, 0.0), (2, -0.5), (3, 1.0 + 1e-12)):
        v = ec.copy()
        v[i] = x
        bad += [(v, ed, "eta_c[%d]" % i), (ed, v, "eta_d[%d]" % i)]
    def unchanged():                    # the refusal stored nothing: the next iteration is the twin's, bit for bit
        e.iterate(1)
        twin.iterate(1)
        sa, sb = state_of(e), state_of(twin)
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), k

    for a, b, what in bad:
        with pytest.raises(_capi.DopfError, match=what.replace("[", r"\[").replace("]", r"\]")):
            e.set_efficiency(a, b)
        unchanged()
    for a, b in ((ec, None), (None, ed)):
        with pytest.raises(_capi.DopfError, match="both"):
            e.set_efficiency(a, b)
        unchanged()
    # a band that the efficiencies leave unreachable: the highest level only a lossless storage reaches
    # (slow storages: T pmax = 0.9 emax, so that a charge efficiency of 0.6 shortens the reach of those that start low)
    pp3 = copy.copy(pp)
    pp3.sto_pmax = 0.9 * pp.sto_emax / pp.T
    top = np.minimum(pp3.sto_emax, e0 + pp3.T * pp3.sto_pmax)
    assert np.any(e0 + pp3.T * 0.6 * pp3.sto_pmax < top - 1e-6)
    e2 = lossy_engine(hip_api, pp3, np.ones(pp.S), np.ones(pp.S), e0, top, top)
    with pytest.raises(_capi.DopfError, match="unreachable"):
        e2.set_efficiency(np.full(pp.S, 0.6), np.ones(pp.S))
    e3 = lossy_engine(hip_api, pp3, np.full(pp.S, 0.6), np.ones(pp.S), e0, np.zeros(pp.S), pp3.sto_emax)
    e3b = lossy_engine(hip_api, pp3, np.full(pp.S, 0.6), np.ones(pp.S), e0, np.zeros(pp.S), pp3.sto_emax)
    for x in (e3, e3b):
        x.iterate(1)
    with pytest.raises(_capi.DopfError, match="unreachable"):      # and the level setters see the stored efficiencies
        e3.set_terminal_levels(top, top)
    e3.iterate(1)
    e3b.iterate(1)
    for k, v in state_of(e3).items():
        assert np.array_equal(v, state_of(e3b)[k]), k
    e3.set_terminal_levels()
    e3.set_initial_levels(np.zeros(pp.S))
    with pytest.raises(_capi.DopfError, match="unreachable"):
        e3.set_terminal_levels(0.7 * pp3.sto_emax, pp3.sto_emax)     # from 0 only 0.54 emax is in reach
    plain = engine(hip_api, pp, None, flags=0, eps=0.0, gamma=0.02)
    with pytest.raises(_capi.DopfError, match="DOPF_F_STO_EFFICIENCY"):
        plain.set_efficiency(ec, ed)
    unchanged()


def test_setter_between_iterations_equals_a_fresh_context(hip_api):
    """efficiencies changed between two dopf_iterate calls act at the next x-update (no re-capture): the result equals a fresh
    context given the same state and the new efficiencies; NULL, NULL restores eta = 1"""
    pp = synth.synthetic_case(n_gen=40, n_sto=24, T=24, seed=861)
    ec, ed, e0, lo, hi = lossy_setup(pp, "inside", "default", 861)
    e = lossy_engine(hip_api, pp, ec, ed, e0, lo, hi)
    e.iterate(3)
    for new in ((np.full(pp.S, 0.9), np.full(pp.S, 0.85)), (None, None)):
        st, it = state_of(e), e.get_residuals()[3]
        e.set_efficiency(*new)
        fresh = lossy_engine(hip_api, pp, *(new if new[0] is not None else (np.ones(pp.S), np.ones(pp.S))), e0, lo, hi)
        set_from(fresh, st, it)
        e.iterate(1)
        fresh.iterate(1)
        w, where, cost = scaled(state_of(e), state_of(fresh))
        assert w <= 1e-9 and cost <= 1e-9, (where, w, cost)
    D, C, E = state_of(e)["D"], state_of(e)["C"], state_of(e)["E"]
    assert np.abs(E - (e0[:, None] + np.cumsum(C - D, axis=1))).max() <= 1e-9         # lossless again


# ---- 6. rolling ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 12])
def test_roll_with_efficiencies_equals_a_fresh_shifted_context(hip_api, k):
    pp = synth.synthetic_case(n_gen=40, n_sto=12, T=24, seed=870)
    rng = np.random.default_rng(870)
    ec, ed = draw_eta(pp.S, rng)
    e0 = draw_e0(pp, "inside", rng)
    h = engine(hip_api, pp, None, flags=EF | IL, eps=0.0, gamma=0.02)
    h.set_efficiency(ec, ed)
    h.set_initial_levels(e0)
    h.iterate(7)
    before = state_of(h)
    assert np.abs(before["E"] - levels_eff(e0, ec, ed, before["D"], before["C"])).max() <= 1e-9
    tail = rng.uniform(0.8, 1.2, (pp.N, k)) * pp.demand[:, :k]
    w = shift_window(k, tail, demand=pp.demand, sto_emax=pp.sto_emax, E=before["E"],
                     **{n: before[n] for n in ("P", "D", "C", "lam", "mu", "rho", "avg_U", "avg_K")})
    h.roll(k, tail)
    assert np.abs(w["e0"] - np.clip(before["E"][:, k - 1], 0.0, pp.sto_emax)).max() <= 1e-12 * pp.sto_emax.max()
    pp2 = copy.copy(pp)
    pp2.demand = w["demand"]
    twin = engine(hip_api, pp2, None, flags=EF | IL, eps=0.0, gamma=0.02)
    twin.set_efficiency(ec, ed)
    twin.set_initial_levels(w["e0"])
    set_from(twin, w, 2)
    d, where, _ = scaled(state_of(h), state_of(twin))
    assert d <= 1e-9, (where, d)                         # (the roll test's one-step bound on copper plates)
    assert np.abs(state_of(h)["E"][:, 0] - (w["e0"] + ec * w["C"][:, 0] - w["D"][:, 0] / ed)).max() <= 1e-9
    h.iterate(1)
    twin.iterate(1)
    d, where, cost = scaled(state_of(h), state_of(twin))
    assert d <= 1e-9 and cost <= 1e-9, (where, d, cost)
    h.iterate(11)
    twin.iterate(11)
    d, where, cost = scaled(state_of(h), state_of(twin))
    assert d <= 1e-8 and cost <= 1e-8, (where, d, cost)
    assert h.solver_failures() == 0


# ---- 7. shards -------------------------------------------------------------------------------------------------------------------
def test_multi_engine_shards_equal_one_context(hip_api):
    pp = synth.synthetic_case(n_gen=40, n_sto=13, T=24, seed=880)
    ec, ed, e0, lo, hi = lossy_setup(pp, "inside", "eq", 880)
    g = 1.0 / (pp.G + pp.S)
    ref = lossy_engine(hip_api, pp, ec, ed, e0, lo, hi, 0, g)
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(eps=0.0, gamma=g, flags=_capi.F_COMM_HOST | EF | IL | TL),
                          **pp.engine_kwargs())
    m.set_efficiency(ec, ed)
    m.set_initial_levels(e0)
    m.set_terminal_levels(lo, hi)
    bad = ec.copy()
    bad[-1] = 1.5                                         # the last shard refuses: nothing stored on the first either
    with pytest.raises(_capi.DopfError, match="shard 1"):
        m.set_efficiency(bad, ed)
    for k in (1, 7):
        ref.iterate(k)
        assert m.iterate(k) == (k, False)
        want = state_of(ref)
        for a, b in zip(m.get_primal(), (want["P"], want["D"], want["C"], want["E"])):
            assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
        for i in range(2):
            got = state_of(m.shard(i))
            for key in ("lam", "inj", "cost"):
                assert np.abs(got[key] - want[key]).max() <= 1e-9 * max(1.0, np.abs(want[key]).max()), (key, i)
    m.close()


def test_sharded_admm_slices_the_efficiencies(hip_api):
    """ShardedADMM (world 1: what one GPU allows, as tests/test_gpu_host.py runs it) given the GLOBAL arrays: equal to the
    single context within the bound of tests/test_gpu_multi.py; both None restores eta = 1. Its slicing for world 2 against
    PackedProblem.shard's ranges, through the engines' stored copies."""
    pp = synth.synthetic_case(n_gen=40, n_sto=13, T=24, seed=881)
    ec, ed, e0, lo, hi = lossy_setup(pp, "inside", "eq", 881)
    g = 1.0 / (pp.G + pp.S)
    ref = lossy_engine(hip_api, pp, ec, ed, e0, lo, hi, 0, g)
    sh = pkg.ShardedADMM(pp, 0, 1, eps=0.0, gamma=g, flags=EF | IL | TL)
    sh.set_efficiency(ec, ed)
    sh.set_initial_levels(e0)
    sh.set_terminal_levels(lo, hi)
    assert np.array_equal(sh.engine._eta[0], ec) and np.array_equal(sh.engine._eta[1], ed)
    for k in (1, 7):
        ref.iterate(k)
        sh.step(k)
        sh.sync()
        want, got = state_of(ref), state_of(sh.engine)
        for key in want:
            if want[key].size:
                assert np.abs(got[key] - want[key]).max() <= 1e-9 * max(1.0, np.abs(want[key]).max()), key
    for rank in range(2):               # world 2: each rank keeps its slice of the global arrays
        s2 = pkg.ShardedADMM(pp, rank, 2, eps=0.0, gamma=g, flags=EF, all_reduce=lambda: None)
        s2.set_efficiency(ec, ed)
        s0, s1 = s2.shard.meta["sto_range"]
        assert np.array_equal(s2.engine._eta[0], ec[s0:s1]) and np.array_equal(s2.engine._eta[1], ed[s0:s1])
        s2.set_efficiency()
        assert s2.engine._eta is None
    # both None: lossless again — equal to a context that never had efficiencies set
    sh.set_terminal_levels()
    sh.set_efficiency(None, None)
    st, it = state_of(sh.engine), sh.engine.get_residuals()[3]
    fresh = lossy_engine(hip_api, pp, np.ones(pp.S), np.ones(pp.S), e0, np.zeros(pp.S), pp.sto_emax, 0, g)
    set_from(fresh, st, it)
    sh.step(1)
    sh.sync()
    fresh.iterate(1)
    w, where, cost = scaled(state_of(sh.engine), state_of(fresh))
    assert w <= 1e-9 and cost <= 1e-9, (where, w, cost)


def test_admm_class_carries_and_sets_efficiencies(hip_api):
    """Storage.charge_efficiency / discharge_efficiency through ADMM(...) (the flag set for it), and ADMM.set_efficiency."""
    nodes, lines, gens, stos = pkg.three_node_case()
    stos[0].charge_efficiency, stos[0].discharge_efficiency = 0.9, 0.8
    a = pkg.ADMM(0.3, nodes, gens, stos, lines, eps=0.0)
    assert a.engine.params.flags & EF
    ref = _capi.Engine(hip_api, params=_capi.default_params(eps=0.0, gamma=0.3, flags=EF), **three_node_pp().engine_kwargs())
    ref.set_efficiency([0.9], [0.8])
    a.engine.iterate(5)
    ref.iterate(5)
    for k, v in state_of(ref).items():
        assert np.array_equal(state_of(a.engine)[k], v), k
    a.set_efficiency([0.7], [1.0])
    ref.set_efficiency([0.7], [1.0])
    a.engine.iterate(3)
    ref.iterate(3)
    for k, v in state_of(ref).items():
        assert np.array_equal(state_of(a.engine)[k], v), k
    D, C, E = state_of(ref)["D"], state_of(ref)["C"], state_of(ref)["E"]
    assert np.abs(E - levels_eff(np.zeros(1), np.array([0.7]), np.array([1.0]), D, C)).max() <= 1e-9


# ---- 8. to the optimum -----------------------------------------------------------------------------------------------------------
def test_three_node_with_a_lossy_battery_reaches_the_lp(hip_api):
    pp = three_node_pp()
    eta = (np.full(1, 0.9), np.full(1, 0.9))
    lp, lossless = central.solve_central_packed(pp, efficiency=eta), central.solve_central_packed(pp)
    assert (lp.objective - lossless.objective) / lossless.objective > 2e-3          # the test can tell the two apart
    e = _capi.Engine(hip_api, params=_capi.default_params(), sto_eta=eta, **pp.engine_kwargs())
    done, conv = e.iterate(5000)
    assert conv, done
    cost = e.get_consensus()[4]
    assert abs(cost - lp.objective) / lp.objective <= 1e-3, (cost, lp.objective)
    P, D, C, E = e.get_primal()
    assert np.abs(E - levels_eff(np.zeros(1), eta[0], eta[1], D, C)).max() <= 1e-9
    assert e.solver_failures() == 0


def test_copper_plate_with_lossy_storages_reaches_the_lp(hip_api):
    pp = synth.synthetic_case(n_gen=12, n_sto=4, T=24, seed=892)
    pp.sto_pmax, pp.sto_emax = pp.sto_pmax * 8.0, pp.sto_emax * 8.0      # (storages large enough for their losses to show: checked
    eta = (np.full(4, 0.9), np.full(4, 0.9))                              # on the CPU, the two LP optima differ by 7e-3)
    lp, lossless = central.solve_central_packed(pp, efficiency=eta), central.solve_central_packed(pp)
    assert (lp.objective - lossless.objective) / lossless.objective > 2e-3
    e = _capi.Engine(hip_api, params=_capi.default_params(gamma=1.0 / (pp.G + pp.S), max_iters=20000), sto_eta=eta, **pp.engine_kwargs())
    done, conv = e.iterate(20000)
    assert conv, done
    cost = e.get_consensus()[4]
    assert abs(cost - lp.objective) / lp.objective <= 1e-3, (cost, lp.objective)
    P, D, C, E = e.get_primal()
    assert np.abs(E - levels_eff(np.zeros(4), eta[0], eta[1], D, C)).max() <= 1e-9
