"""Line ratings per timestep (DOPF_F_LINE_RATING, dopf_set_line_rating) on the device. The references here are: the
flagless context, bit for bit, wherever the table's columns all equal f_max; without storages the oracle's exact mode column by
column with one f_max per line (timestep t of a run under a table is the T = 1 problem with f_max = rating[:, t]); with storages the
breakpoint tables of a flagless context with f_max = rating[:, t] and a NumPy KKT certificate whose theta comes from Psi under the
table; and the HiGHS LP for the optimum. The CPU oracle takes the table itself since (oracle_set_line_rating): the slack getters'
last leg uses it, and every chain is compared with it value for value, with storages, in tests/test_gpu_lossy_rated_parity.py.
Needs a real MI355X: pytest -m gpu."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library loads RCCL: one copy per process)

from conftest import pkg
from decentralopf_jl_amd import _capi, shift_window, synth
from helpers import engine, set_from, state_of, storage_kkt_violation_band
from helpers_line_rating import (GAMMA, GENC, LR, NETC, STOC, case, column_problem, constant_table, debug_table, draw_table,
                                 quiet_state, rated_engine, theta_of_rated, with_f_max)

pytestmark = pytest.mark.gpu

IL, TL, EF, AV = _capi.F_STO_INITIAL_LEVEL, _capi.F_STO_TERMINAL_LEVEL, _capi.F_STO_EFFICIENCY, _capi.F_GEN_AVAILABILITY
E_INVALID, E_UNSUPPORTED = -1, -4
KW = dict(eps=0.0, gamma=GAMMA)
COLS = ("P", "lam", "mu", "rho", "avg_U", "avg_K", "flow", "inj")       # what has a column per timestep (without storages)


def same_bits(a, b, keys=None, what=""):
    for k in (keys or a.keys()):
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k] - b[k]).max()))


def col(st, key, t):
    return st[key][t] if key == "lam" else st[key][:, t]


def seeded_state(pp, seed):
    """a state for dopf_set_state that no run produced (tests/test_gpu_sto_efficiency.py)"""
    rng = np.random.default_rng(seed)
    return dict(P=rng.uniform(0, 1, (pp.G, pp.T)) * pp.gen_pmax[:, None], D=rng.uniform(0, 0.4, (pp.S, pp.T)) * pp.sto_pmax[:, None],
                C=rng.uniform(0, 0.4, (pp.S, pp.T)) * pp.sto_pmax[:, None], avg_U=rng.uniform(0, 1, (pp.L, pp.T)),
                avg_K=rng.uniform(0, 1, (pp.L, pp.T)), lam=rng.uniform(1, 30, pp.T), mu=rng.uniform(0, 1, (pp.L, pp.T)),
                rho=rng.uniform(0, 1, (pp.L, pp.T)))


# ---- 1. the flag alone and a constant table are the flagless run, bit for bit ---------------------------------------------------
T1024C = dict(n_gen=200, n_sto=40, T=144, N=20, L=30, seed=51, fmax_factor=0.7, fmax_min=5)     # L*T > 4096: the one-launch dual/price kernel
CHAINS = [("default", NETC, 0), ("net-small-items", NETC, _capi.F_NET_SMALL_ITEMS), ("no-quiet", NETC, _capi.F_NO_QUIET),
          ("overlap-agents", NETC, _capi.F_OVERLAP_AGENTS), ("no-fuse", NETC, _capi.F_NO_FUSE), ("no-graph", NETC, _capi.F_NO_GRAPH),
          ("debug-wide-net", NETC, _capi.F_DEBUG_WIDE_NET), ("debug-long-sto", NETC, _capi.F_DEBUG_LONG_STO),
          ("feature-flags-at-defaults", NETC, IL | TL | EF | AV),
          ("copper-plate", dict(n_gen=40, n_sto=8, T=12, seed=52), 0),
          ("one-launch-dual-kernel", T1024C, 0), ("one-launch-dual-kernel-no-quiet", T1024C, _capi.F_NO_QUIET)]


@pytest.mark.parametrize("name,kw,extra", CHAINS, ids=[c[0] for c in CHAINS])
def test_flag_alone_and_constant_table_are_the_flagless_run(hip_api, name, kw, extra):
    pp = case(kw)
    plain = engine(hip_api, pp, None, flags=extra, **KW)
    plain.iterate(200)
    want = state_of(plain)
    alone = rated_engine(hip_api, pp, extra, **KW)
    alone.iterate(200)
    same_bits(state_of(alone), want, what="flag alone")
    const = rated_engine(hip_api, pp, extra, rating=constant_table(pp), **KW)
    const.iterate(200)
    same_bits(state_of(const), want, what="constant table")
    assert alone.get_residuals()[3] == const.get_residuals()[3] == plain.get_residuals()[3]
    assert alone.solver_failures() == 0 and const.solver_failures() == 0


# ---- 2. generators only: every column follows the oracle -------------------------------------------------------------------------
STEPS = 25


@pytest.fixture(scope="module")
def gen_case():
    pp = case(GENC)
    return pp, draw_table(pp)


@pytest.fixture(scope="module")
def oracle_columns(oracle_api, gen_case):
    """the oracle's exact mode on the T = 1 problem of every column, f_max = rating[:, t]: the state after each of STEPS steps"""
    pp, rating = gen_case
    out = []
    for t in range(pp.T):
        o = engine(oracle_api, column_problem(pp, t, rating[:, t]), 1, **KW)
        steps = []
        for _ in range(STEPS):
            o.iterate(1)
            steps.append(state_of(o))
        out.append(steps)
    return out


GEN_CHAINS = [("default", 0), ("no-quiet", _capi.F_NO_QUIET), ("net-small-items", _capi.F_NET_SMALL_ITEMS),
              ("debug-wide-net", _capi.F_DEBUG_WIDE_NET), ("no-graph", _capi.F_NO_GRAPH)]


@pytest.mark.parametrize("name,extra", GEN_CHAINS, ids=[c[0] for c in GEN_CHAINS])
def test_generators_only_every_column_follows_the_oracle(hip_api, gen_case, oracle_columns, name, extra):
    pp, rating = gen_case
    h = rated_engine(hip_api, pp, extra, rating=rating, **KW)
    twins = None
    if extra == _capi.F_NO_QUIET:           # flagless T = 4 contexts with the constant f_max = rating[:, t]: column t, bit for bit
        twins = [engine(hip_api, with_f_max(pp, rating[:, t]), None, flags=extra, **KW) for t in range(pp.T)]
    binding = np.zeros(pp.T, dtype=bool)
    worst = 0.0
    for k in range(STEPS):
        h.iterate(1)
        st = state_of(h)
        binding |= np.any(st["mu"] != 0.0, axis=0)
        for t in range(pp.T):
            ref = oracle_columns[t][k]
            for key in COLS:
                d = float(np.abs(col(st, key, t) - col(ref, key, 0)).max())
                worst = max(worst, d)
                assert d <= 1e-9, (k, t, key, d)
        if twins:
            for t, tw in enumerate(twins):
                tw.iterate(1)
                sw = state_of(tw)
                for key in COLS:
                    assert np.array_equal(col(st, key, t), col(sw, key, t)), (k, t, key)
    assert binding.all(), binding           # in every column some line binds at some step
    print(f"{name}: worst column difference to the oracle {worst:.2e}")


# ---- 3. the storages' input: tables bit for bit ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sto_case(hip_api):
    """the case with storages, its table, and a state after 30 iterations of the rated context"""
    pp = case(STOC)
    rating = draw_table(pp)
    e = rated_engine(hip_api, pp, 0, rating=rating, **KW)
    e.iterate(30)
    return pp, rating, state_of(e), e.get_residuals()[3]


@pytest.mark.parametrize("extra", [0, _capi.F_DEBUG_WIDE_NET], ids=["default", "debug-wide-net"])
def test_tables_are_those_of_a_flagless_context_with_the_columns_limits(hip_api, sto_case, extra):
    pp, rating, st, it = sto_case
    r = rated_engine(hip_api, pp, extra, rating=rating, **KW)
    set_from(r, st, it)
    r.iterate(1)
    for t in (0, pp.T // 2, pp.T - 1):
        f = engine(hip_api, with_f_max(pp, rating[:, t]), None, flags=extra, **KW)
        set_from(f, st, it)
        f.iterate(1)
        for n in range(pp.N):
            a, b = debug_table(hip_api, r, n, t), debug_table(hip_api, f, n, t)
            for key in ("m", "beta", "psi", "slope", "psi0"):
                assert np.array_equal(a[key], b[key]), (t, n, key, a[key], b[key])


# ---- 4. storages under ratings pass the KKT certificate --------------------------------------------------------------------------
def certified_steps(e, pp, n, rating, w_flow=10.0):
    for k in range(n):
        before = state_of(e)
        e.iterate(1)
        after = state_of(e)
        D, C, E = after["D"], after["C"], after["E"]
        assert np.abs(E - np.cumsum(C - D, axis=1)).max() <= 1e-9, k
        theta = theta_of_rated(pp, before, e.get_duals_used(), D, C, GAMMA, w_flow, rating)
        viol = storage_kkt_violation_band(pp, before["D"], before["C"], D, C, E, theta, GAMMA, np.zeros(pp.S), pp.sto_emax)
        print(f"step {k}: KKT violation {viol:.2e}")
        assert viol <= 1e-7, (k, viol)
    assert e.solver_failures() == 0


CERT = [("default", 0), ("no-quiet", _capi.F_NO_QUIET), ("debug-wide-net", _capi.F_DEBUG_WIDE_NET),
        ("debug-long-sto", _capi.F_DEBUG_LONG_STO), ("sto-general", _capi.F_STO_GENERAL)]


@pytest.mark.parametrize("name,extra", CERT, ids=[c[0] for c in CERT])
def test_storages_under_ratings_pass_the_certificate(hip_api, name, extra):
    pp = case(STOC)
    rating = draw_table(pp)
    e = rated_engine(hip_api, pp, extra, rating=rating, **KW)
    certified_steps(e, pp, 4, rating)
    set_from(e, seeded_state(pp, 6), 2)
    certified_steps(e, pp, 2, rating)


# ---- 5. a set between iterations -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, _capi.F_DEBUG_WIDE_NET], ids=["default", "debug-wide-net"])
def test_set_between_iterations(hip_api, extra):
    pp = case(NETC)
    first, second = constant_table(pp), draw_table(pp)
    g = rated_engine(hip_api, pp, extra, rating=first, **KW)                         # captured graphs
    n = rated_engine(hip_api, pp, extra | _capi.F_NO_GRAPH, rating=first, **KW)      # the same launches, eagerly
    for e in (g, n):
        assert e.iterate(20) == (20, False)
    before = state_of(g)
    it = g.get_residuals()[3]
    for e in (g, n):
        e.set_line_rating(second)
        assert e.sync() == (it, False) and e.get_residuals()[3] == it               # not converged, the counter unchanged
    same_bits(state_of(g), before, what="kept by the set")
    fresh = rated_engine(hip_api, pp, extra, rating=second, **KW)
    set_from(fresh, before, it)
    for e in (g, n, fresh):
        assert e.iterate(20) == (20, False)
    after = state_of(g)
    assert not np.array_equal(after["mu"], before["mu"])
    same_bits(after, state_of(n), what="graphs vs eager launches")
    d = {k: float(np.abs(after[k] - v).max()) for k, v in state_of(fresh).items()}
    print("set mid-run vs a fresh context handed the state:", d)
    same_bits(after, state_of(fresh), what="fresh context with the table, handed the state before the set")


# ---- 6. the quiet chain ----------------------------------------------------------------------------------------------------------
def test_a_tighter_table_leaves_the_quiet_chain(hip_api):
    """The 118-node share (the one-launch dual/price kernel; tests/p2p_worker.py runs its quiet chain): generous limits, the quiet
    chain runs; then 0.3 f_max — the flags must be formed again and the stale "no line flagged" dropped."""
    pp = synth.baseline_config(3, scale=0.02)
    A = pp.G + pp.S
    kw = dict(eps=0.0, gamma=1.0 / A, w_flow=0.3 / A)
    q = rated_engine(hip_api, pp, 0, rating=constant_table(pp, 4.0), **kw)
    nq = rated_engine(hip_api, pp, _capi.F_NO_QUIET, rating=constant_table(pp, 4.0), **kw)
    for e in (q, nq):
        e.iterate(20)
    assert quiet_state(hip_api, q)[:2] == (1, 1)                    # allowed, and in use for the next call
    assert quiet_state(hip_api, nq)[:2] == (0, 0)
    same_bits(state_of(q), state_of(nq), what="generous limits")
    for e in (q, nq):
        e.set_line_rating(constant_table(pp, 0.3))
    assert quiet_state(hip_api, q)[1] == 0                          # right after the set
    for e in (q, nq):
        e.iterate(20)
    a = state_of(q)
    same_bits(a, state_of(nq), what="tight limits")
    assert np.any(a["mu"] != 0.0) or np.any(a["rho"] != 0.0)        # (the tight table binds)


# ---- 7. refusals store nothing -----------------------------------------------------------------------------------------------------
def full_state(e):
    s = state_of(e)
    lu, mu_u, ru = e.get_duals_used()
    s.update(lam_used=lu, mu_used=mu_u, rho_used=ru, price0=e.get_nodal_price(0), price1=e.get_nodal_price(1),
             res=np.asarray(e.get_residuals(), dtype=np.float64), sync=np.asarray(e.sync(), dtype=np.float64))
    return s


def test_refusals_store_nothing(hip_api):
    pp = case(NETC)
    plain = engine(hip_api, pp, None, **KW)
    plain.iterate(5)
    snap = full_state(plain)
    buf = _capi._rating_buffer(constant_table(pp), pp.L, pp.T)
    assert hip_api.set_line_rating(plain._ctx, _capi._dp(buf)) == E_UNSUPPORTED
    assert b"DOPF_F_LINE_RATING" in hip_api.last_error(plain._ctx)
    same_bits(full_state(plain), snap, what="no flag")
    e = rated_engine(hip_api, pp, 0, rating=draw_table(pp), **KW)
    e.iterate(5)
    snap = full_state(e)
    l, t = 3, 7
    for bad in (np.nan, np.inf, -1.0):
        tab = draw_table(pp)
        tab[l, t] = bad
        buf = _capi._rating_buffer(tab, pp.L, pp.T)
        assert hip_api.set_line_rating(e._ctx, _capi._dp(buf)) == E_INVALID, bad
        msg = hip_api.last_error(e._ctx).decode()
        assert f"l = {l}" in msg and f"t = {t}" in msg, msg
        same_bits(full_state(e), snap, what=f"refused {bad}")
    # nothing of a refused table was stored: the run goes on under the table of before
    twin = rated_engine(hip_api, pp, 0, rating=draw_table(pp), **KW)
    twin.iterate(5)
    e.iterate(5)
    twin.iterate(5)
    same_bits(state_of(e), state_of(twin), what="after the refusals")
    # NULL restores f_max: from a common state the next 20 iterations are the flagless context's
    st, it = state_of(e), e.get_residuals()[3]
    e.set_line_rating(None)
    set_from(e, st, it)
    flagless = engine(hip_api, pp, None, **KW)
    set_from(flagless, st, it)
    e.iterate(20)
    flagless.iterate(20)
    same_bits(state_of(e), state_of(flagless), what="NULL = f_max")
    # a copper plate: the flag is accepted, the call does nothing
    cp = synth.synthetic_case(n_gen=20, n_sto=4, T=6, seed=53)
    c = rated_engine(hip_api, cp, 0, **KW)
    c.iterate(3)
    snap = full_state(c)
    c.set_line_rating(None)
    assert hip_api.set_line_rating(c._ctx, _capi._dp(np.zeros(1))) == 0
    same_bits(full_state(c), snap, what="L == 0")


# ---- 8. roll ---------------------------------------------------------------------------------------------------------------------
MOVED = ("P", "D", "C", "lam", "mu", "rho", "avg_U", "avg_K")


def scaled(sa, sb):
    scale = max(1.0, float(np.abs(sb["lam"]).max()))
    worst, where = 0.0, None
    for k in sa:
        if k != "cost" and sa[k].size:
            d = float(np.abs(sa[k] - sb[k]).max())
            if d > worst:
                worst, where = d, k
    cost = abs(float(sa["cost"][0] - sb["cost"][0])) / max(1.0, abs(float(sb["cost"][0])))
    return worst / scale, where, cost


@pytest.mark.parametrize("k", [1, 5])
def test_roll_moves_the_table(hip_api, k):
    """tests/test_gpu_horizon_roll.py's comparison (networks: one step 1e-8, twelve 1e-7, scaled) against a fresh context of the
    shifted problem with the shifted table, whose tail repeats the last column"""
    pp = case(STOC)
    rating = draw_table(pp)
    one, many = 1e-8, 1e-7
    h = rated_engine(hip_api, pp, IL, rating=rating, **KW)
    h.set_initial_levels(np.zeros(pp.S))
    h.iterate(7)
    before = state_of(h)
    tail = np.round(pp.demand[:, :k] * 1.05) + 1.0
    w = shift_window(k, tail, demand=pp.demand, sto_emax=pp.sto_emax, E=before["E"], line_rating=rating,
                     **{n: before[n] for n in MOVED})
    assert np.array_equal(w["line_rating"][:, pp.T - k:], np.repeat(rating[:, -1:], k, axis=1))
    h.roll(k, tail)
    after = state_of(h)
    same_bits(after, w, MOVED, what="moved arrays")
    assert h.sync() == (2, False)

    def twin_of(table):
        pp2 = copy.copy(pp)
        pp2.demand = w["demand"]
        e = rated_engine(hip_api, pp2, IL, rating=table, **KW)
        e.set_initial_levels(w["e0"])
        set_from(e, w, 2)
        return e
    twin = twin_of(w["line_rating"])
    d, where, _ = scaled(state_of(h), state_of(twin))
    assert d <= one, (where, d)
    h.iterate(1)
    twin.iterate(1)
    d, where, cost = scaled(state_of(h), state_of(twin))
    print(f"k = {k}: one iteration after the roll vs the fresh context: {d:.2e} ({where}), cost {cost:.2e}")
    assert d <= one and cost <= 1e-9, (where, d, cost)
    h.iterate(11)
    twin.iterate(11)
    d, where, cost = scaled(state_of(h), state_of(twin))
    assert d <= many and cost <= 1e-8, (where, d, cost)
    # a new table after the roll = the same table on the fresh context
    new = draw_table(pp, seed=4)
    h.set_line_rating(new)
    twin.set_line_rating(new)
    h.iterate(5)
    twin.iterate(5)
    d, where, cost = scaled(state_of(h), state_of(twin))
    assert d <= many and cost <= 1e-8, (where, d, cost)
    assert h.solver_failures() == 0


# ---- 9. slack and penalty getters ------------------------------------------------------------------------------------------------
def test_slack_and_penalty_getters_follow_the_table(hip_api, oracle_api, gen_case):
    pp, rating = gen_case
    h = rated_engine(hip_api, pp, _capi.F_KEEP_DELTAS, rating=rating, **KW)
    cols = [engine(oracle_api, column_problem(pp, t, rating[:, t]), 1, **KW) for t in range(pp.T)]
    dp = _capi.c_double_p
    tol = lambda want: 1e-10 * max(1.0, float(np.abs(want).max()))
    worst = 0.0
    for it in range(6):
        h.iterate(1)
        befores = [state_of(o) for o in cols]
        for o in cols:
            o.iterate(1)
        afters = [state_of(o) for o in cols]
        sums = np.zeros((3, pp.T))
        for a in range(pp.G):
            U, K = h.get_agent_slacks(a)
            eb, up, lo = h.get_agent_penalty(a)
            hcol = pp.ptdf[:, pp.gen_node[a]]
            for t, o in enumerate(cols):
                Uo, Ko = np.zeros(pp.L), np.zeros(pp.L)
                assert oracle_api.get_agent_slacks(o._ctx, a, Uo.ctypes.data_as(dp), Ko.ctypes.data_as(dp)) == 0
                d = afters[t]["P"][a, 0] - befores[t]["P"][a, 0]
                # (the flows the solve read are ptdf . injection: in the zero state the getter still reports 0)
                fl = pp.ptdf @ befores[t]["inj"][:, 0] + hcol * d
                want = ((befores[t]["inj"][:, 0].sum() + d) ** 2, ((fl + Uo - rating[:, t]) ** 2).sum(), ((Ko - fl - rating[:, t]) ** 2).sum())
                sums[:, t] += want
                if a in (0, 7, pp.G - 1):
                    for got, ref in ((U[:, t], Uo), (K[:, t], Ko), (eb[t], want[0]), (up[t], want[1]), (lo[t], want[2])):
                        dd = float(np.abs(got - ref).max())
                        worst = max(worst, dd / max(1.0, float(np.abs(ref).max())))
                        assert dd <= tol(ref), (it, a, t, dd)
        for got, want in zip(h.get_penalty_sums(), sums):
            dd = float(np.abs(got - want).max())
            worst = max(worst, dd / max(1.0, float(np.abs(want).max())))
            assert dd <= tol(want), (it, dd)
    print(f"slack and penalty getters vs the oracle's columns: worst relative difference {worst:.2e}")
    # with storages the columns are coupled, and the reference is the oracle's exact mode under the same table: one step at a time
    # (from the zero state, the HIP state reset to the oracle's after each), generators and storages
    from conftest import build_oracle
    from oracle.binding import OracleApi
    fapi = OracleApi(build_oracle(), features=True)
    pp = case(STOC)
    rating = draw_table(pp)
    h = rated_engine(hip_api, pp, _capi.F_KEEP_DELTAS, rating=rating, **KW)
    o = _capi.Engine(fapi, params=_capi.default_params(flags=LR, **KW), mode=1, **pp.engine_kwargs())
    o.set_line_rating(rating)
    worst, active = 0.0, 0
    for it in range(5):
        h.iterate(1)
        o.iterate(1)
        for a in (0, 7, pp.G - 1, pp.G, pp.G + 3, pp.G + pp.S - 1):
            U, K = h.get_agent_slacks(a)
            Uo, Ko = np.zeros(pp.L * pp.T), np.zeros(pp.L * pp.T)
            assert fapi.get_agent_slacks(o._ctx, a, Uo.ctypes.data_as(dp), Ko.ctypes.data_as(dp)) == 0
            for got, ref in ((U, Uo.reshape(pp.T, pp.L).T), (K, Ko.reshape(pp.T, pp.L).T)):
                dd = float(np.abs(got - ref).max())
                worst = max(worst, dd / max(1.0, float(np.abs(ref).max())))
                active += int(np.count_nonzero(ref))
                assert dd <= tol(ref), (it, a, dd)
        set_from(h, state_of(o), o.get_residuals()[3])
    assert active > 0
    print(f"slack getters with storages vs the oracle under the table: worst relative difference {worst:.2e}")


# ---- 10. shards --------------------------------------------------------------------------------------------------------------------
def test_multi_shards_equal_one_context_with_a_table_changed_mid_run(hip_api):
    """tests/test_gpu_multi.py::test_multi_shards_equal_one_context's comparison (host transport, 2 shards on one device)"""
    kw = dict(n_gen=300, n_sto=40, T=24, N=3, L=3, seed=4, fmax_factor=0.8, fmax_min=5)
    pp = case(kw)
    g = 0.01
    first, second = draw_table(pp), draw_table(pp, seed=4)
    ref = rated_engine(hip_api, pp, 0, rating=first, eps=0.0, gamma=g)
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(eps=0.0, gamma=g, flags=_capi.F_COMM_HOST | LR), line_rating=first,
                          **pp.engine_kwargs())
    for k in (1, 4, None, 7):
        if k is None:
            ref.set_line_rating(second)
            m.set_line_rating(second)
            continue
        ref.iterate(k)
        assert m.iterate(k) == (k, False)
        want = state_of(ref)
        for a, b in zip(m.get_primal(), (want["P"], want["D"], want["C"], want["E"])):
            assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
        for i in range(2):
            got = state_of(m.shard(i))
            for key in ("lam", "mu", "rho", "inj", "avg_U", "avg_K", "flow", "cost"):
                assert np.abs(got[key] - want[key]).max() <= 1e-9 * max(1.0, np.abs(want[key]).max()), (key, i, k)
    bad = second.copy()
    bad[1, 2] = -3.0
    with pytest.raises(_capi.DopfError, match="shard 0.*l = 1.*t = 2"):
        m.set_line_rating(bad)
    m.close()


def test_peer_exchange_shards_with_ratings(hip_api):
    """DOPF_F_COMM_P2P, two shards on one device, in a process of its own (as tests/test_gpu_multi.py::
    test_peer_exchange_shards_on_one_device): a table changed mid-run, and the generous-then-tight change on the chain without
    k_reduce — both shards take the same chain decisions. tests/line_rating_p2p_worker.py."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "line_rating_p2p_worker.py")
    r = subprocess.run([sys.executable, worker], env=dict(os.environ, DOPF_XCHG_TIMEOUT_MS="5000"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "line rating p2p worker: ok" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    for line in ("table changed mid-run ok", "generous then tight ok"):
        assert line in r.stdout, (line, r.stdout[-1500:])


# ---- 11. optimum -------------------------------------------------------------------------------------------------------------------
def test_derated_three_node_case_reaches_the_lp(hip_api):
    """Line 0 of the shipped case at 15 instead of 20 in the second timestep only: LP optimum 14685.0 (tests/test_line_rating_abi.py).
    With the reference's literals (eps 1e-3) the run converges, its cost within 1e-3 of the LP. The stop test lets mu move by less
    than eps in the last step, mu' - mu = gamma (flow + avg_U - rating), so a converged flow may stand above its rating by up to
    eps / gamma = 3.3e-3: measured |flow[0, 1]| = 15.0033 at eps 1e-3. The bound 15 + 1e-6 on the flow therefore needs
    eps <= 1e-6 gamma = 3e-7, and is asserted on a second run with that eps (same case, same max_iters)."""
    nodes, lines, gens, stos = pkg.three_node_case()
    lines[0].rating = [20, 15]
    for eps in (1e-3, 3e-7):
        admm = pkg.ADMM(0.3, nodes, gens, stos, lines, max_iters=20000, record=False, eps=eps)
        assert admm.engine.params.flags & LR
        done, conv = admm.engine.iterate(20000)
        inj, aU, aK, flow, cost = admm.engine.get_consensus()
        print(f"derated three-node case, eps {eps:g}: converged {conv} after {done} iterations, cost {cost:.4f} (LP 14685.0), "
              f"|flow[0, 1]| = {abs(flow[0, 1]):.9f}")
        assert conv, (eps, done)
        assert abs(cost - 14685.0) <= 1e-3 * 14685.0, (eps, cost)
        assert abs(flow[0, 1]) <= 15.0 + eps / 0.3 + 1e-9, (eps, flow[0, 1])
    assert abs(flow[0, 1]) <= 15.0 + 1e-6, flow[0, 1]
