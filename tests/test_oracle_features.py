"""The CPU oracle with the three problem extensions (storage initial levels, terminal bands, generator availability; DESIGN.md
sections 5h-5j): their defaults change no bit, the exact mode equals the literal QP one step at a time over a table of horizons,
levels, bands, degenerate storages and profiles, the exact storages pass the QP certificate, free runs reach the central LP with the
same inputs, and a shift of 1e-6 in any one input moves the result by more than the tolerances used here. CPU only."""
import numpy as np
import pytest

from conftest import build_oracle
from decentralopf_jl_amd import _capi, synth
from decentralopf_jl_amd.central import solve_central_packed
from helpers import (Features, degenerate, draw_band, draw_e0, engine, max_diff, set_from, state_of,
                     storage_kkt_violation_band)

IL, TL, AV = _capi.F_STO_INITIAL_LEVEL, _capi.F_STO_TERMINAL_LEVEL, _capi.F_GEN_AVAILABILITY
ALL = IL | TL | AV
NET = dict(N=4, L=5, fmax_factor=0.7, fmax_min=5)


@pytest.fixture(scope="module")
def fapi():
    """The oracle with the three setters bound (the session's oracle_api has none of them)."""
    from oracle.binding import OracleApi
    return OracleApi(build_oracle(), features=True)


def make(api, pp, mode, feats, **params):
    e = engine(api, pp, mode, flags=feats.flags, eps=0.0, **params)
    feats.apply(e)
    return e


def one_step_worst(a, b, iters, between=None):
    """a and b one iteration each, b restarted from a's state after each; `between(k)` may call setters on both. Worst absolute
    difference of any array of state_of but the cost, or relative difference of the cost (a sum over every agent and timestep)."""
    worst, where = 0.0, None
    for k in range(iters):
        if between is not None:
            between(k)
        a.iterate(1)
        b.iterate(1)
        sa, sb = state_of(a), state_of(b)
        w, wh = max_diff(sa, sb, keys=[k for k in sa if k != "cost"])
        c = abs(float(sa["cost"][0] - sb["cost"][0])) / max(1.0, abs(float(sa["cost"][0])))    # the cost: relative
        w, wh = (w, wh) if w >= c else (c, "cost")
        if w > worst:
            worst, where = w, (k, wh)
        set_from(b, sa, a.get_residuals()[3])
    return worst, where


# ---- no-op: each flag with its default values is the flagless run, bit for bit, in both modes --------------------------------

NOOP = [("copper-T12", dict(n_gen=12, n_sto=6, T=12, seed=3), dict(gamma=0.1)),
        ("net-4x5-T5", dict(n_gen=12, n_sto=4, T=5, seed=5, **NET), dict(gamma=0.1))]


@pytest.mark.parametrize("name,case,params", NOOP, ids=[c[0] for c in NOOP])
@pytest.mark.parametrize("mode", [0, 1])
def test_defaults_are_the_flagless_run_bit_for_bit(fapi, name, case, params, mode):
    pp = synth.synthetic_case(**case)
    ref = engine(fapi, pp, mode, eps=0.0, **params)
    ones = np.ones((2, pp.T))
    runs = []
    for flags, setup in [(IL, lambda e: e.set_initial_levels(np.zeros(pp.S))),
                         (TL, lambda e: e.set_terminal_levels(np.zeros(pp.S), pp.sto_emax)),
                         (AV, lambda e: e.set_availability(np.full((2, pp.T), 0.5), np.full(pp.G, -1))),
                         (AV, lambda e: e.set_availability(ones, np.arange(pp.G) % 2)),
                         (ALL, lambda e: None)]:
        e = engine(fapi, pp, mode, flags=flags, eps=0.0, **params)
        setup(e)
        runs.append(e)
    for _ in range(6):
        ref.iterate(1)
        want = state_of(ref)
        for e in runs:
            e.iterate(1)
            got = state_of(e)
            assert all(np.array_equal(want[k], got[k]) for k in want), e.params.flags


def test_setter_refusals_store_nothing(fapi):
    """The refusals of include/dopf.h: DOPF_E_UNSUPPORTED without the flag, DOPF_E_INVALID (and nothing stored) for the inputs
    the header lists."""
    INVALID, UNSUPPORTED = -1, -4
    pp = synth.synthetic_case(n_gen=6, n_sto=3, T=4, seed=8)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_capi.c_double_p)
    ip = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(_capi.c_int32_p)
    e = engine(fapi, pp, 1)
    assert fapi.set_storage_initial_level(e._ctx, dp(np.zeros(3))) == UNSUPPORTED
    assert fapi.set_storage_terminal_level(e._ctx, dp(np.zeros(3)), dp(pp.sto_emax)) == UNSUPPORTED
    assert fapi.set_generator_availability(e._ctx, 1, dp(np.ones(4)), ip(np.zeros(6))) == UNSUPPORTED
    e = engine(fapi, pp, 1, flags=ALL)
    ctx, em, span = e._ctx, pp.sto_emax, 4 * pp.sto_pmax
    for e0 in ([0.0, -1e-9, 0.0], [0.0, np.nextafter(em[1], np.inf), 0.0], [np.nan, 0.0, 0.0]):
        assert fapi.set_storage_initial_level(ctx, dp(e0)) == INVALID, e0
    top = np.minimum(em, span)                                        # the highest level reachable from the empty start
    for lo, hi in ((np.zeros(3), None), (None, em), ([1.0, 0.0, 0.0], [0.5, 1.0, 1.0]), (np.zeros(3), em + 1.0),
                   ([np.nan, 0.0, 0.0], em), (np.nextafter(top, np.inf), em)):
        assert fapi.set_storage_terminal_level(ctx, dp(lo), dp(hi)) == INVALID, (lo, hi)
    assert fapi.set_storage_terminal_level(ctx, dp(top), dp(top)) == 0
    for K, prof, of in ((1, [1.0, 0.5, 1.5, 0.0], np.zeros(6)), (1, [1.0, np.nan, 1.0, 0.0], np.zeros(6)),
                        (1, [1.0, 0.5, -0.0 - 1e-300, 0.0], np.zeros(6)), (1, np.ones(4), np.ones(6)),
                        (1, np.ones(4), np.full(6, -2)), (1, np.ones(4), None), (1, None, np.zeros(6)), (-1, None, None)):
        assert fapi.set_generator_availability(ctx, K, dp(prof), ip(of)) == INVALID, (K, prof, of)
    # nothing of the refused calls was stored: the run equals one with the accepted band alone
    ref = engine(fapi, pp, 1, flags=TL)
    ref.set_terminal_levels(top, top)
    e.iterate(3)
    ref.iterate(3)
    a, b = state_of(e), state_of(ref)
    assert all(np.array_equal(a[k], b[k]) for k in a)


# ---- the exact mode equals the literal QP, one step at a time --------------------------------------------------------------
# name, case, params, e0, band, profiles, degenerate storages, iterations, tolerance. Halfway through, every row draws new
# inputs and sets them on both engines. The tolerances are measured (the row's worst, times 2-10; the cost compares relatively):
# 1.1e-13, 2.3e-13, 1.5e-11, 4.9e-8, 7.1e-7, 3.7e-8 on the copper plates, 2.3e-13, 2.0e-12, 2.1e-10, 7.5e-9, 2.5e-6, 4.0e-8 on
# the networks. The rows above 1e-9 have a storage on a degenerate vertex (its level on a bound while D or C sits on one too, a
# contact next to an idle step), where the interior-point QP of the literal mode stops short of the vertex; the exact mode's point
# passes the QP certificate there (test_exact_storages_pass_the_certificate_under_every_feature).

TABLE = [
    ("copper-T1", dict(n_gen=10, n_sto=8, T=1, seed=31), dict(gamma=0.1), "inside", "eq", "K1", "emax0", 6, 1e-11),
    ("copper-T2", dict(n_gen=10, n_sto=8, T=2, seed=32), dict(gamma=0.1), "full", "edge-lo", "K3", "", 6, 1e-11),
    ("copper-T5", dict(n_gen=12, n_sto=8, T=5, seed=33), dict(gamma=0.1), "0", "edge", "KG", "pmax0", 8, 1e-10),
    ("copper-T12", dict(n_gen=12, n_sto=8, T=12, seed=34), dict(gamma=0.1), "inside", "cyclic", "K3", "emax0+pmax0", 8, 2e-7),
    ("copper-T24", dict(n_gen=20, n_sto=10, T=24, seed=35), dict(gamma=0.05), "mix", "mix", "KG", "", 8, 3e-6),
    ("copper-T48", dict(n_gen=20, n_sto=8, T=48, seed=36), dict(gamma=0.05), "full", "eq", "K1", "pmax0", 6, 2e-7),
    ("net-T1", dict(n_gen=12, n_sto=4, T=1, seed=41, **NET), dict(gamma=0.1), "inside", "default", "K3", "", 6, 1e-11),
    ("net-T2", dict(n_gen=12, n_sto=4, T=2, seed=42, **NET), dict(gamma=0.1), "full", "cyclic", "KG", "emax0", 6, 1e-11),
    ("net-T5", dict(n_gen=12, n_sto=8, T=5, seed=43, **NET), dict(gamma=0.1), "mix", "mix", "K1", "pmax0", 8, 1e-9),
    ("net-T12", dict(n_gen=12, n_sto=4, T=12, seed=44, **NET), dict(gamma=0.1), "0", "edge", "K3", "", 6, 3e-8),
    ("net-T24", dict(n_gen=12, n_sto=4, T=24, seed=45, **NET), dict(gamma=0.1), "inside", "eq", "KG", "emax0", 4, 1e-5),
    ("net-T48", dict(n_gen=8, n_sto=3, T=48, seed=46, **NET), dict(gamma=0.1), "mix", "edge-lo", "K3", "emax0", 3, 2e-7),
]


def literal_and_exact(fapi, pp, feats, params, threads=4):
    from oracle.binding import set_threads
    a, b = make(fapi, pp, 0, feats, **params), make(fapi, pp, 1, feats, **params)
    set_threads(a, threads)
    return a, b


@pytest.mark.parametrize("name,case,params,e0,band,prof,degen,iters,tol", TABLE, ids=[r[0] for r in TABLE])
def test_exact_mode_equals_literal_qp_with_features(fapi, name, case, params, e0, band, prof, degen, iters, tol):
    pp = degenerate(synth.synthetic_case(**case), degen)
    feats = Features(pp, e0, band, prof, seed=case["seed"])
    again = Features(pp, e0, band, prof, seed=case["seed"] + 1000)
    a, b = literal_and_exact(fapi, pp, feats, params)

    def between(k):
        if k == iters // 2:
            again.apply(a)
            again.apply(b)

    worst, where = one_step_worst(a, b, iters, between)
    print(f"{name}: worst one-step difference {worst:.2e} at {where}")
    assert worst < tol, (where, worst)


# ---- the exact storages pass the QP certificate under every feature (copper plates) -----------------------------------------

@pytest.mark.parametrize("e0,band", [("mix", "mix"), ("inside", "cyclic"), ("0", "edge"), ("full", "edge-lo")])
def test_exact_storages_pass_the_certificate_under_every_feature(fapi, e0, band):
    gamma = 0.02
    pp = degenerate(synth.synthetic_case(40, 25, 24, seed=21), "emax0")
    feats = Features(pp, e0, band, "K3", seed=22)
    e = make(fapi, pp, 1, feats, gamma=gamma)
    for k in range(12):
        before = state_of(e)
        e.iterate(1)
        after = state_of(e)
        theta = e.get_duals_used()[0][None, :] + gamma * (before["inj"].sum(axis=0)[None, :] - (before["D"] - before["C"]))
        D, C, E = after["D"], after["C"], after["E"]
        assert np.abs(E - (feats.e0[:, None] + np.cumsum(C - D, axis=1))).max() <= 1e-9
        assert (feats.band[0] - E[:, -1]).max() <= 1e-9 and (E[:, -1] - feats.band[1]).max() <= 1e-9
        v = storage_kkt_violation_band(pp, before["D"], before["C"], D, C, E, theta, gamma, *feats.band)
        assert v < 1e-7, (k, v)
    # the certificate sees the band: the same point against a band shifted off its last level fails
    lo, hi = feats.band
    moved = np.where(hi - lo < 1e-3, 0.5 * (lo + hi), lo)
    shifted = (np.minimum(moved + 1e-3, pp.sto_emax), np.minimum(moved + 1e-3, pp.sto_emax))
    if np.any(np.abs(E[:, -1] - shifted[0]) > 1e-4):
        assert storage_kkt_violation_band(pp, before["D"], before["C"], D, C, E, theta, gamma, *shifted) > 0 or \
            np.any(E[:, -1] < shifted[0] - 1e-7)


# ---- free runs reach the central LP with the same inputs ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["copper-T24", "network-12x18-T12"])
def test_exact_oracle_reaches_the_lp_with_every_feature(fapi, name):
    if name == "copper-T24":
        pp = synth.synthetic_case(100, 12, 24, seed=441)
        kw = {}
    else:
        pp = synth.synthetic_case(300, 30, 12, N=12, L=18, seed=23, fmax_factor=2.0, fmax_min=20)
        kw = dict(w_flow=0.3 / (pp.G + pp.S))
    rng = np.random.default_rng(7)
    e0 = draw_e0(pp, "mix", rng)
    lo, hi = draw_band(pp, e0, "mix", rng)
    prof = synth.availability_profiles(pp.T, seed=8)
    of = np.full(pp.G, -1, dtype=np.int32)
    of[::10] = np.arange(pp.G)[::10] % 3
    want = solve_central_packed(pp, duals=False, initial_level=e0, terminal_level=(lo, hi), availability=(prof, of)).objective
    A = pp.G + pp.S
    e = engine(fapi, pp, 1, flags=ALL, gamma=1.0 / A, max_iters=6000, **kw)
    e.set_initial_levels(e0)
    e.set_terminal_levels(lo, hi)
    e.set_availability(prof, of)
    from oracle.binding import set_threads
    set_threads(e, 4)
    done, conv = e.iterate(6000)
    assert conv, done
    cost = e.get_consensus()[4]
    assert abs(cost - want) / want < 1e-3, (cost, want, done)


# ---- negative controls: a shift of 1e-6 in one input on one side is seen ---------------------------------------------------

CONTROL = dict(n_gen=12, n_sto=8, T=5, seed=33)


@pytest.mark.parametrize("what", ["e0", "lo", "profile"])
def test_a_one_sided_shift_of_one_input_fails_the_tolerance(fapi, what):
    """The literal mode with the inputs, the exact mode with one of them moved by 1e-6 emax (levels) or 1e-6 (a profile entry):
    the one-step difference must exceed this row's tolerance of the table above (copper-T5, 1e-10) many times over."""
    pp = synth.synthetic_case(**CONTROL)
    feats = Features(pp, "inside", "eq", "K3", seed=5)
    prof, of = feats.prof
    feats.prof = (np.maximum(prof, 0.5), np.where(of < 0, 0, of).astype(np.int32))   # every generator on a profile, none at 0
    a, b = literal_and_exact(fapi, pp, feats, dict(gamma=0.1))
    moved = Features(pp, "inside", "eq", "K3", seed=5)
    moved.prof = (feats.prof[0].copy(), feats.prof[1])
    d = 1e-6 * pp.sto_emax
    if what == "e0":
        moved.e0 = feats.e0 + np.where(np.arange(pp.S) == 2, d, 0.0)
    elif what == "lo":
        moved.band = (feats.band[0] + np.where(np.arange(pp.S) == 2, d, 0.0), feats.band[1] + np.where(np.arange(pp.S) == 2, d, 0.0))
    else:
        moved.prof[0][0, 3] -= 1e-6
    moved.apply(b)
    worst, where = one_step_worst(a, b, 4)
    assert worst > 100 * 1e-10, (what, worst, where)
    # and without the shift the same pair agrees within the tolerance
    a, b = literal_and_exact(fapi, pp, feats, dict(gamma=0.1))
    assert one_step_worst(a, b, 4)[0] < 1e-10
