"""The CPU oracle with storage efficiencies and line ratings per timestep (DESIGN.md sections 5m, 5o), alone, together and with the
three earlier extensions: their defaults change no bit, the setters refuse what include/dopf.h refuses and store nothing then, the
exact mode equals the literal QP one step at a time over a table of horizons, efficiencies, rating tables, levels, bands, degenerate
storages and profiles, free runs reach the central LP with the same inputs, and a shift of 1e-6 in one efficiency or one binding
rating on one side moves the result by more than the tolerances used here. CPU only."""
import numpy as np
import pytest

from conftest import build_oracle
from decentralopf_jl_amd import _capi, synth
from decentralopf_jl_amd.central import solve_central_packed
from helpers import LossyRated, degenerate, draw_e0, engine, max_diff, set_from, state_of
from helpers_efficiency import draw_band_eff, draw_eta, storage_kkt_violation_eff
from helpers_line_rating import constant_table, draw_table, theta_of_rated

IL, TL, AV = _capi.F_STO_INITIAL_LEVEL, _capi.F_STO_TERMINAL_LEVEL, _capi.F_GEN_AVAILABILITY
EF, LR = _capi.F_STO_EFFICIENCY, _capi.F_LINE_RATING
NET = dict(N=4, L=5, fmax_factor=0.7, fmax_min=5)
INVALID, UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def fapi():
    """The oracle with the five setters bound (the session's oracle_api has none of them)."""
    from oracle.binding import OracleApi
    return OracleApi(build_oracle(), features=True)


def make(api, pp, mode, feats, **params):
    e = engine(api, pp, mode, flags=feats.flags, eps=0.0, **params)
    feats.apply(e)
    return e


def literal_and_exact(fapi, pp, feats, params, threads=4):
    from oracle.binding import set_threads
    a, b = make(fapi, pp, 0, feats, **params), make(fapi, pp, 1, feats, **params)
    set_threads(a, threads)
    return a, b


def one_step_worst(a, b, iters, between=None, certify=None):
    """tests/test_oracle_features.py's: a (literal) and b (exact) one iteration each, b restarted from a's state after each;
    `between(k)` may call setters on both; `certify(before, b)` sees b's state before and b itself after every step. Worst absolute
    difference of any array of state_of but the cost, or relative difference of the cost."""
    worst, where = 0.0, None
    for k in range(iters):
        if between is not None:
            between(k)
        before = state_of(b)
        a.iterate(1)
        b.iterate(1)
        sa, sb = state_of(a), state_of(b)
        w, wh = max_diff(sa, sb, keys=[k for k in sa if k != "cost"])
        c = abs(float(sa["cost"][0] - sb["cost"][0])) / max(1.0, abs(float(sa["cost"][0])))    # the cost: relative
        w, wh = (w, wh) if w >= c else (c, "cost")
        if w > worst:
            worst, where = w, (k, wh)
        if certify is not None:
            certify(k, before, b, sb)
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
    ones = np.ones(pp.S)
    runs = []
    for flags, setup in [(EF, lambda e: None), (LR, lambda e: None),
                         (EF, lambda e: e.set_efficiency(ones, ones)),
                         (LR, lambda e: e.set_line_rating(constant_table(pp))),
                         (EF | LR, lambda e: None),
                         (EF | LR, lambda e: (e.set_efficiency(ones, ones), e.set_line_rating(constant_table(pp)))),
                         (EF | LR | IL | TL | AV, lambda e: None),
                         (EF | LR | IL | TL | AV, lambda e: (e.set_efficiency(), e.set_line_rating(), e.set_initial_levels(np.zeros(pp.S)),
                                                            e.set_terminal_levels(np.zeros(pp.S), pp.sto_emax)))]:
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


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_setter_refusals_store_nothing(fapi):
    """The refusals of include/dopf.h: DOPF_E_UNSUPPORTED without the flag, DOPF_E_INVALID (and nothing stored) for a NaN, an eta
    <= 0 or > 1, only one array NULL, an Inf or negative rating, and, with DOPF_F_STO_TERMINAL_LEVEL, a band, an initial level or a
    pair of efficiencies under which the band is out of reach — among them bands that are reachable at eta = 1."""
    pp = synth.synthetic_case(n_gen=6, n_sto=3, T=4, seed=8, **NET)
    S, L, T = pp.S, pp.L, pp.T
    dp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_capi.c_double_p)
    one, em, pm = np.ones(S), pp.sto_emax, pp.sto_pmax
    assert np.all(T * pm > em)                                        # (the synthetic storages fill in 2 steps at eta = 1)
    buf = lambda r: _capi._rating_buffer(r, L, T)
    e = engine(fapi, pp, 1)
    assert fapi.set_storage_efficiency(e._ctx, dp(one), dp(one)) == UNSUPPORTED
    assert fapi.set_storage_efficiency(e._ctx, None, None) == UNSUPPORTED
    assert fapi.set_line_rating(e._ctx, dp(buf(constant_table(pp)))) == UNSUPPORTED
    assert fapi.set_line_rating(e._ctx, None) == UNSUPPORTED
    e = engine(fapi, pp, 1, flags=EF | LR | IL | TL)
    ctx = e._ctx
    for ec, ed in ((one, None), (None, one), ([np.nan, 1.0, 1.0], one), (one, [1.0, np.nan, 1.0]), ([0.0, 1.0, 1.0], one),
                   (one, [1.0, 1.0, -0.5]), ([1.0, np.nextafter(1.0, 2.0), 1.0], one), (one, [np.inf, 1.0, 1.0])):
        assert fapi.set_storage_efficiency(ctx, dp(ec), dp(ed)) == INVALID, (ec, ed)
    for l, t, v in ((0, 0, np.nan), (L - 1, T - 1, np.inf), (2, 1, -1e-300), (1, 3, -np.inf)):
        r = draw_table(pp)
        r[l, t] = v
        assert fapi.set_line_rating(ctx, dp(buf(r))) == INVALID, (l, t, v)
    # reachability that only eta < 1 takes away. The top of the reachable range from the empty start is min(emax, T eta_c pmax):
    # emax at eta_c = 1, less under an eta_c so small that T eta_c pmax < emax
    small = 0.5 * em / (T * pm)                                       # T small pmax = emax / 2
    low = np.array([small[0], 1.0, 1.0])
    assert fapi.set_storage_terminal_level(ctx, dp(em), dp(em)) == 0  # reachable at eta = 1 ...
    assert fapi.set_storage_efficiency(ctx, dp(low), dp(one)) == INVALID          # ... not under the small eta_c: refused
    assert fapi.set_storage_terminal_level(ctx, None, None) == 0
    assert fapi.set_storage_efficiency(ctx, dp(low), dp(one)) == 0    # under the default band the small eta_c is fine,
    assert fapi.set_storage_terminal_level(ctx, dp(em), dp(em)) == INVALID        # and now the band is the one refused,
    top = np.minimum(em, T * low * pm)
    over = top.copy()
    over[0] = np.nextafter(top[0], np.inf)
    assert fapi.set_storage_terminal_level(ctx, dp(over), dp(em)) == INVALID
    assert fapi.set_storage_terminal_level(ctx, dp(top), dp(top)) == 0            # while the top of the smaller range passes.
    # The bottom: from a full start the lowest level is max(0, e0 - T pmax / eta_d), which a small eta_d lowers (never refuses), so
    # the refusal with eta_d comes through e0: [top, top] is reachable from 0, and from emax only by discharging
    assert fapi.set_storage_terminal_level(ctx, None, None) == 0
    assert fapi.set_storage_efficiency(ctx, dp(one), dp(one)) == 0
    half = 0.5 * em
    assert fapi.set_storage_initial_level(ctx, dp(em)) == 0
    assert fapi.set_storage_terminal_level(ctx, dp(half), dp(half)) == 0
    # (eta_d < 1 only widens the reach downwards: accepted. eta_c so small that the band is out of reach from below: e0 = 0)
    assert fapi.set_storage_efficiency(ctx, dp(one), dp(np.full(S, 0.5))) == 0
    assert fapi.set_storage_efficiency(ctx, dp(one), dp(one)) == 0
    tiny = 0.25 * em / (T * pm)                                       # T tiny pmax = emax / 4 < half
    assert fapi.set_storage_initial_level(ctx, dp(np.zeros(S))) == 0  # at eta = 1 the band [half, half] is reachable from 0,
    assert fapi.set_storage_efficiency(ctx, dp(np.array([1.0, tiny[1], 1.0])), dp(one)) == INVALID     # not under tiny eta_c
    assert fapi.set_storage_terminal_level(ctx, None, None) == 0
    assert fapi.set_storage_efficiency(ctx, dp(np.array([1.0, tiny[1], 1.0])), dp(one)) == 0
    assert fapi.set_storage_initial_level(ctx, dp(em)) == 0
    assert fapi.set_storage_terminal_level(ctx, dp(half), dp(half)) == 0          # from emax the band is reached by discharging
    assert fapi.set_storage_initial_level(ctx, dp(np.zeros(S))) == INVALID        # and e0 = 0 is now the one refused
    # nothing of the refused calls was stored: the run equals one that made the accepted calls alone
    table = draw_table(pp)
    assert fapi.set_line_rating(ctx, dp(buf(table))) == 0
    bad = table.copy()
    bad[0, 0] = -1.0
    assert fapi.set_line_rating(ctx, dp(buf(bad))) == INVALID
    ref = engine(fapi, pp, 1, flags=EF | LR | IL | TL)
    ref.set_efficiency(np.array([1.0, tiny[1], 1.0]), one)
    ref.set_initial_levels(em)
    ref.set_terminal_levels(half, half)
    ref.set_line_rating(table)
    e.iterate(3)
    ref.iterate(3)
    a, b = state_of(e), state_of(ref)
    assert all(np.array_equal(a[k], b[k]) for k in a)


# ---- the exact mode equals the literal QP, one step at a time --------------------------------------------------------------
# name, case, params, (e0, band, profiles), (eta, table, zero entry), degenerate storages, iterations, tolerance. Halfway through,
# every row draws new inputs (new efficiencies and a new table among them) and sets them on both engines. Every draw of
# efficiencies has storages at (1, 1) among the lossy ones (helpers_efficiency.draw_eta). The tolerances are measured (the row's
# worst with the literal mode as the reference, times 2-10; the cost compares relatively; none looser than 1e-5):
# 2.6e-13, 1.1e-13, 4.8e-12, 3.8e-12, 2.6e-7 on the copper plates, 7.8e-14, 1.1e-13, 1.8e-11, 3.9e-12, 3.4e-12 on the networks
# T = 1 to 24, 1.0e-10 with the table alone, 2.0e-12 with the efficiencies alone, 4.6e-13 with everything.
# The rows above 1e-9 (copper-T24) must also pass the QP certificate (helpers_efficiency.storage_kkt_violation_eff <= 1e-7, theta from
# helpers_line_rating.theta_of_rated) on the exact mode's point at every step: there a storage sits on a degenerate vertex (its
# level on a bound while D or C sits on one too), where the interior-point QP of the literal mode stops short of the vertex.

TABLE = [
    ("copper-T1", dict(n_gen=10, n_sto=8, T=1, seed=61), dict(gamma=0.1), ("inside", "eq", "K1"), (True, False, False), "emax0", 6, 1e-12),
    ("copper-T2", dict(n_gen=10, n_sto=8, T=2, seed=62), dict(gamma=0.1), ("full", "cyclic", "K3"), (True, False, False), "", 6, 1e-12),
    ("copper-T5", dict(n_gen=12, n_sto=8, T=5, seed=63), dict(gamma=0.1), ("0", "eq", "KG"), (True, False, False), "pmax0", 8, 2e-11),
    ("copper-T12", dict(n_gen=12, n_sto=8, T=12, seed=64), dict(gamma=0.1), ("inside", "cyclic", "K3"), (True, False, False), "emax0+pmax0", 8, 2e-11),
    ("copper-T24", dict(n_gen=20, n_sto=10, T=24, seed=65), dict(gamma=0.05), ("mix", "mix", "KG"), (True, False, False), "", 8, 1e-6),
    ("net-T1", dict(n_gen=12, n_sto=4, T=1, seed=71, **NET), dict(gamma=0.1), ("inside", "default", "K3"), (True, True, True), "", 6, 5e-13),
    ("net-T2", dict(n_gen=12, n_sto=4, T=2, seed=72, **NET), dict(gamma=0.1), ("full", "cyclic", "KG"), (True, True, False), "emax0", 6, 1e-12),
    ("net-T5", dict(n_gen=12, n_sto=8, T=5, seed=73, **NET), dict(gamma=0.1), ("mix", "mix", "K1"), (True, True, True), "pmax0", 8, 1e-10),
    ("net-T12", dict(n_gen=12, n_sto=4, T=12, seed=74, **NET), dict(gamma=0.1), ("0", "eq", "K3"), (True, True, False), "", 6, 2e-11),
    ("net-T24", dict(n_gen=12, n_sto=4, T=24, seed=75, **NET), dict(gamma=0.1), ("inside", "eq", "KG"), (True, True, True), "emax0", 4, 2e-11),
    ("net-T5-table-alone", dict(n_gen=12, n_sto=6, T=5, seed=76, **NET), dict(gamma=0.1), (None, None, None), (False, True, True), "", 8, 5e-10),
    ("net-T5-eta-alone", dict(n_gen=12, n_sto=6, T=5, seed=77, **NET), dict(gamma=0.1), (None, None, None), (True, False, False), "", 8, 1e-11),
    ("net-T12-everything", dict(n_gen=12, n_sto=5, T=12, seed=78, **NET), dict(gamma=0.1), ("mix", "mix", "K3"), (True, True, True), "emax0+pmax0", 6, 3e-12),
]


def certifier(pp, feats_at, gamma, w_flow=10.0):
    """the QP certificate on the exact mode's storages after a step; feats_at(k): the inputs in force at step k"""
    def certify(k, before, b, after):
        e0, lo, hi, ec, ed, F = feats_at(k).cert_inputs()
        theta = theta_of_rated(pp, before, b.get_duals_used(), after["D"], after["C"], gamma, w_flow, F)
        v = storage_kkt_violation_eff(pp, before["D"], before["C"], after["D"], after["C"], theta, gamma, e0, lo, hi, ec, ed)
        assert v <= 1e-7, (k, v)
    return certify


@pytest.mark.parametrize("name,case,params,feat,extra,degen,iters,tol", TABLE, ids=[r[0] for r in TABLE])
def test_exact_mode_equals_literal_qp_lossy_and_rated(fapi, name, case, params, feat, extra, degen, iters, tol):
    pp = degenerate(synth.synthetic_case(**case), degen)
    eta, table, zero = extra
    feats = LossyRated(pp, *feat, seed=case["seed"], eta=eta, table=table, zero=zero)
    again = LossyRated(pp, *feat, seed=case["seed"] + 1000, eta=eta, table=table, zero=zero)
    assert tol <= 1e-5
    if eta:
        assert np.any((feats.eta[0] == 1.0) & (feats.eta[1] == 1.0)) and np.any(feats.eta[0] < 1.0) and np.any(feats.eta[1] < 1.0)
    if zero:
        assert feats.rating[0, 0] == 0.0 and again.rating[0, 0] == 0.0
    a, b = literal_and_exact(fapi, pp, feats, params)

    def between(k):
        if k == iters // 2:
            again.apply(a)
            again.apply(b)

    certify = certifier(pp, lambda k: again if k >= iters // 2 else feats, params["gamma"]) if tol > 1e-9 else None
    worst, where = one_step_worst(a, b, iters, between, certify)
    print(f"{name}: worst one-step difference {worst:.2e} at {where}")
    assert worst < tol, (where, worst)


# ---- free runs reach the central LP with the same inputs ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["copper-T24", "network-12x18-T12"])
def test_exact_oracle_reaches_the_lossy_rated_lp(fapi, name):
    """The cases, the other three inputs and the bound of test_oracle_features.test_exact_oracle_reaches_the_lp_with_every_feature,
    with efficiencies below 1 and (on the network) a rating table."""
    if name == "copper-T24":
        pp = synth.synthetic_case(100, 12, 24, seed=441)
        kw = {}
    else:
        pp = synth.synthetic_case(300, 30, 12, N=12, L=18, seed=23, fmax_factor=2.0, fmax_min=20)
        kw = dict(w_flow=0.3 / (pp.G + pp.S))
    rng = np.random.default_rng(7)
    ec, ed = draw_eta(pp.S, rng)
    e0 = draw_e0(pp, "mix", rng)
    lo, hi = draw_band_eff(pp, e0, ec, ed, "mix", rng)
    prof = synth.availability_profiles(pp.T, seed=8)
    of = np.full(pp.G, -1, dtype=np.int32)
    of[::10] = np.arange(pp.G)[::10] % 3
    # The table: helpers_line_rating.draw_table's deratings, but no entry below 1.05 times the flow that the LP without a table
    # puts on that line in that timestep. Limits that bind at the optimum keep this case from settling at these parameters with
    # or without the new code: with a constant 0.5 f_max and no new flag (the code path of before, 21 binding pairs) the dual
    # residual still stands at 0.27 after 6000 iterations, and under draw_table as it is (where the LP is feasible at all) at
    # 0.3-0.5 after 20000. So the table here derates 91 of the network's 216 entries without binding at the optimum, the LP is
    # solved with it all the same, and the run differs from the one without a table on the way (1012 iterations against 551).
    lp = dict(duals=False, initial_level=e0, terminal_level=(lo, hi), availability=(prof, of), efficiency=(ec, ed))
    rating = np.maximum(draw_table(pp, seed=9), 1.05 * np.abs(solve_central_packed(pp, **lp).line_utilization))
    if pp.L:
        assert (rating < pp.f_max[:, None]).sum() > pp.L * pp.T // 3
    want = solve_central_packed(pp, line_rating=rating, **lp).objective
    A = pp.G + pp.S
    e = engine(fapi, pp, 1, flags=IL | TL | AV | EF | LR, gamma=1.0 / A, max_iters=6000, **kw)
    e.set_efficiency(ec, ed)
    e.set_initial_levels(e0)
    e.set_terminal_levels(lo, hi)
    e.set_availability(prof, of)
    e.set_line_rating(rating)
    from oracle.binding import set_threads
    set_threads(e, 4)
    done, conv = e.iterate(6000)
    assert conv, done
    cost = e.get_consensus()[4]
    print(f"{name}: converged after {done} iterations, cost {cost:.4f} against the LP's {want:.4f}")
    assert abs(cost - want) / want < 1e-3, (cost, want, done)


# ---- negative controls: a shift of 1e-6 in one input on one side is seen ---------------------------------------------------

CONTROL = "net-T5"


@pytest.mark.parametrize("what", ["eta_c", "eta_d", "rating"])
def test_a_one_sided_shift_of_one_input_fails_the_tolerance(fapi, what):
    """The literal mode with the inputs, the exact mode with one of them moved: one eta_c or one eta_d by 1e-6, or one rating by
    1e-6 f_max. The moved entry is a binding one in the unshifted run: a storage that charges (eta_c) resp. discharges (eta_d), a
    (line, timestep) whose mu is non-zero. The one-step difference must exceed this row's tolerance of the table above 100 times
    over, and the unshifted pair stays inside it."""
    row = next(r for r in TABLE if r[0] == CONTROL)
    _, case, params, feat, (eta, table, zero), degen, iters, tol = row
    pp = degenerate(synth.synthetic_case(**case), degen)
    feats = LossyRated(pp, *feat, seed=case["seed"], eta=eta, table=table, zero=zero)
    a, b = literal_and_exact(fapi, pp, feats, params)
    n = 4
    assert one_step_worst(a, b, n)[0] < tol
    st = state_of(a)
    moved = LossyRated(pp, *feat, seed=case["seed"], eta=eta, table=table, zero=zero)
    if what == "rating":
        l, t = np.unravel_index(np.argmax(np.abs(st["mu"])), st["mu"].shape)
        assert st["mu"][l, t] != 0.0
        moved.rating[l, t] += 1e-6 * pp.f_max[l]
    else:
        moved_through = st["C"] if what == "eta_c" else st["D"]
        arr = moved.eta[0] if what == "eta_c" else moved.eta[1]
        s = int(np.argmax(np.where(arr < 1.0, moved_through.sum(axis=1), -1.0)))       # (a lossy one: eta + 1e-6 must stay <= 1)
        assert moved_through[s].sum() > 0.0 and arr[s] + 1e-6 <= 1.0
        arr[s] += 1e-6
    a, b = literal_and_exact(fapi, pp, feats, params)
    moved.apply(b)
    worst, where = one_step_worst(a, b, n)
    print(f"{what}: one-step difference {worst:.2e} at {where} against the tolerance {tol:.0e}")
    assert worst > 100 * tol, (what, worst, where)
