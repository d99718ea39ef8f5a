"""dopf_set_demand / dopf_roll_horizon on every single-GPU chain. Three checks per case: (1) the moved arrays are
horizon.shift_window of what the getters returned before, bit for bit; (2) the context then behaves like a fresh one of the shifted
problem after the same setters and dopf_set_state(shifted, iteration = 2) — the route the entry is defined by; (3) and like the
oracle's exact mode from the same state. Tolerances: those of tests/test_gpu_feature_parity.py (scaled as there): one step 1e-9
on copper plates, 1e-8 on networks; several steps 1e-8 / 1e-7. Needs a real MI355X: pytest -m gpu."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import build_oracle
from decentralopf_jl_amd import _capi, shift_window, synth
from helpers import engine, max_diff, set_from, state_of

pytestmark = pytest.mark.gpu

IL, TL, AV = _capi.F_STO_INITIAL_LEVEL, _capi.F_STO_TERMINAL_LEVEL, _capi.F_GEN_AVAILABILITY
E_INVALID, E_UNSUPPORTED = -1, -4
MOVED = ("P", "D", "C", "lam", "mu", "rho", "avg_U", "avg_K")


@pytest.fixture(scope="module")
def fapi():
    from oracle.binding import OracleApi
    return OracleApi(build_oracle(), features=True)


def copper(T, S=12, seed=801):
    return synth.synthetic_case(40, S, T, seed=seed)


def network(T, seed=802):
    return synth.synthetic_case(30, 10, T, N=6, L=8, seed=seed, fmax_factor=0.7, fmax_min=5)


def kw_of(pp):
    return dict(eps=0.0, gamma=0.02) if pp.L == 0 else dict(eps=0.0, gamma=0.03)


def tail_of(pp, k):
    """the demand of the k new steps: the window's first k steps again, a little higher (integers, like the case's own)"""
    return np.round(pp.demand[:, :k] * 1.05) + 1.0


def scaled(sa, sb):
    scale = max(1.0, float(np.abs(sb["lam"]).max()))
    worst, where = max_diff(sa, sb, keys=[k for k in sa if k != "cost"])
    cost = abs(float(sa["cost"][0] - sb["cost"][0])) / max(1.0, abs(float(sb["cost"][0])))
    return worst / scale, where, cost


def full_state(e):
    """every getter"""
    s = state_of(e)
    lu, mu_u, ru = e.get_duals_used()
    s.update(lam_used=lu, mu_used=mu_u, rho_used=ru, price0=e.get_nodal_price(0), price1=e.get_nodal_price(1),
             res=np.asarray(e.get_residuals(), dtype=np.float64), sync=np.asarray(e.sync(), dtype=np.float64))
    return s


def same_bits(a, b, keys=None):
    for k in (keys or a.keys()):
        assert np.array_equal(a[k], b[k]), k


class Setup:
    """the inputs of the three feature flags for a case (None: not used), applied to any engine with a given e0"""

    def __init__(self, pp, band=None, prof=None):
        self.band, self.prof = band, prof

    def apply(self, e, e0):
        if self.band is not None:
            e.set_terminal_levels()
        e.set_initial_levels(e0)
        if self.band is not None:
            e.set_terminal_levels(*self.band)
        if self.prof is not None:
            e.set_availability(*self.prof)


def shifted_twin(api, pp, w, flags, setup, mode, iteration=2):
    """the reference route: a fresh context of the shifted problem, the setters, set_state(shifted arrays)"""
    pp2 = copy.copy(pp)
    pp2.demand = w["demand"]
    e = engine(api, pp2, mode, flags=flags, **kw_of(pp))
    setup.apply(e, w["e0"])
    set_from(e, w, iteration)
    return e


def roll_case(hip_api, fapi, pp, extra, k, checks, setup=None, e0=None):
    setup = setup or Setup(pp)
    flags = IL | extra
    one, many = (1e-9, 1e-8) if pp.L == 0 else (1e-8, 1e-7)
    h = engine(hip_api, pp, None, flags=flags, **kw_of(pp))
    setup.apply(h, np.zeros(pp.S) if e0 is None else e0)
    h.iterate(7)
    before = full_state(h)
    tail = tail_of(pp, k)
    w = shift_window(k, tail, demand=pp.demand, sto_emax=pp.sto_emax, E=before["E"], **{n: before[n] for n in MOVED},
                     used=dict(lam=before["lam_used"], mu=before["mu_used"], rho=before["rho_used"]))
    h.roll(k, tail)
    after = full_state(h)
    assert after["res"][3] == 2 and after["sync"].tolist() == [2.0, 0.0]
    T = pp.T
    if 1 in checks:
        same_bits(after, w, MOVED)
        for n in ("lam", "mu", "rho"):
            assert np.array_equal(after[n + "_used"], w["used"][n]), n
        lim = 1e-12 * pp.sto_emax[:, None]
        assert np.all(np.abs(after["E"][:, :T - k] - before["E"][:, k:]) <= lim), float(np.abs(after["E"][:, :T - k] - before["E"][:, k:]).max())
        assert np.array_equal(after["E"][:, T - k:], np.repeat(after["E"][:, T - k - 1:T - k], k, axis=1))
        assert np.all(np.abs(after["inj"] - (h.get_node_results()[0] + h.get_node_results()[1] - h.get_node_results()[2] - w["demand"])) <= 1e-9 * np.abs(w["demand"]).max())
    twin = shifted_twin(hip_api, pp, w, flags, setup, None) if 2 in checks else None
    ora = shifted_twin(fapi, pp, w, flags & (IL | TL | AV), setup, 1) if 3 in checks else None
    if twin is not None:                    # the derived state, before any iteration
        d, where, _ = scaled(state_of(h), state_of(twin))
        print(f"after the roll vs the reference route: {d:.2e} ({where})")
        assert d <= one, (where, d)
    h.iterate(1)
    for other, name in ((twin, "reference route"), (ora, "oracle")):
        if other is None:
            continue
        other.iterate(1)
        d, where, cost = scaled(state_of(h), state_of(other))
        print(f"one iteration vs the {name}: {d:.2e} ({where}), cost {cost:.2e}")
        assert d <= one and cost <= 1e-9, (name, where, d, cost)
    if twin is not None:
        h.iterate(11)
        twin.iterate(11)
        d, where, cost = scaled(state_of(h), state_of(twin))
        print(f"12 iterations vs the reference route: {d:.2e} ({where}), cost {cost:.2e}")
        assert d <= many and cost <= 1e-8, (where, d, cost)
    assert h.solver_failures() == 0
    return h


GRID = [
    ("copper-T24-k1", lambda: copper(24), 0, 1, (1, 2, 3)),
    ("copper-T24-k5", lambda: copper(24), 0, 5, (1, 2, 3)),
    ("copper-T24-k23", lambda: copper(24), 0, 23, (1, 2, 3)),
    ("copper-T100-k37", lambda: copper(100), 0, 37, (1, 2, 3)),
    ("copper-T192-k64", lambda: copper(192), 0, 64, (1, 2, 3)),
    ("copper-no-tail-fuse", lambda: copper(24), _capi.F_NO_TAIL_FUSE, 5, (2,)),
    ("copper-no-fuse", lambda: copper(24), _capi.F_NO_FUSE, 5, (2,)),
    ("net-k1", lambda: network(12), 0, 1, (1, 2, 3)),
    ("net-k7", lambda: network(12), 0, 7, (1, 2, 3)),
    ("net-no-quiet-k1", lambda: network(12), _capi.F_NO_QUIET, 1, (1, 2, 3)),
    ("net-no-quiet-k7", lambda: network(12), _capi.F_NO_QUIET, 7, (1, 2, 3)),
    ("net-debug-wide", lambda: network(12), _capi.F_DEBUG_WIDE_NET, 7, (2,)),
    ("copper-debug-long-sto", lambda: copper(24), _capi.F_DEBUG_LONG_STO, 5, (1, 2, 3)),
    ("copper-long-horizon-T2100-k70", lambda: copper(2100, S=3), _capi.F_LONG_HORIZON, 70, (2, 3)),
]


@pytest.mark.parametrize("name,case,extra,k,checks", GRID, ids=[g[0] for g in GRID])
def test_roll_on_every_chain(hip_api, fapi, name, case, extra, k, checks):
    roll_case(hip_api, fapi, case(), extra, k, checks)


def test_roll_with_every_feature_flag(hip_api, fapi):
    pp = copper(24)
    rng = np.random.default_rng(803)
    prof = np.round(rng.uniform(0.2, 1.0, (2, pp.T)) * 1024.0) / 1024.0
    of = (np.arange(pp.G) % 3 - 1).astype(np.int32)             # -1, 0, 1, ...
    setup = Setup(pp, band=(0.3 * pp.sto_emax, 0.8 * pp.sto_emax), prof=(prof, of))
    roll_case(hip_api, fapi, pp, TL | AV, 5, (2, 3), setup=setup, e0=0.5 * pp.sto_emax)


# ---- dopf_set_demand ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [lambda: copper(24), lambda: network(12)], ids=["copper", "net"])
def test_set_demand(hip_api, fapi, case):
    pp = case()
    one, many = (1e-9, 1e-8) if pp.L == 0 else (1e-8, 1e-7)
    h = engine(hip_api, pp, None, flags=IL, **kw_of(pp))
    h.iterate(7)
    before = full_state(h)
    demand = pp.demand * 1.1
    h.set_demand(demand)
    after = full_state(h)
    derived = ("inj", "flow", "price0", "price1")
    same_bits(before, after, [k for k in before if k not in derived])        # (incl. the iteration counter; s is inj summed)
    assert after["sync"].tolist() == [8.0, 0.0]
    assert np.all(np.abs((before["inj"] - after["inj"]) - (demand - pp.demand)) <= 1e-9 * np.abs(demand).max())
    h.set_demand(demand)
    same_bits(after, full_state(h))
    w = dict(before, demand=demand, e0=np.zeros(pp.S))
    twin = shifted_twin(hip_api, pp, w, IL, Setup(pp), None, iteration=8)
    ora = shifted_twin(fapi, pp, w, IL, Setup(pp), 1, iteration=8)
    h.iterate(1)
    for other, name in ((twin, "reference route"), (ora, "oracle")):
        other.iterate(1)
        d, where, cost = scaled(state_of(h), state_of(other))
        print(f"set_demand, one iteration vs the {name}: {d:.2e} ({where}), cost {cost:.2e}")
        assert d <= one and cost <= 1e-9, (name, where, d, cost)
    h.iterate(11)
    twin.iterate(11)
    d, where, cost = scaled(state_of(h), state_of(twin))
    assert d <= many and cost <= 1e-8, (where, d, cost)
    assert h.get_residuals()[3] == 20


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def refused(e, rc, want, snap, word=None):
    assert rc == want, (rc, e.api.last_error(e._ctx))
    if word:
        assert word in e.api.last_error(e._ctx).decode(), e.api.last_error(e._ctx)
    same_bits(snap, full_state(e))


@pytest.mark.parametrize("case", [lambda: copper(24), lambda: network(12)], ids=["copper", "net"])
def test_refusals_leave_every_getter_as_it_was(hip_api, case):
    pp = case()
    h = engine(hip_api, pp, None, flags=IL, **kw_of(pp))
    h.iterate(7)
    snap = full_state(h)
    api, ctx, dp = h.api, h._ctx, _capi._dp
    good = _capi._f64(tail_of(pp, 3).T)
    refused(h, api.roll_horizon(ctx, 0, dp(good)), E_INVALID, snap, "k = 0")
    refused(h, api.roll_horizon(ctx, pp.T, dp(good)), E_INVALID, snap, "k = %d" % pp.T)
    refused(h, api.roll_horizon(ctx, 3, None), E_INVALID, snap, "NULL")
    for bad in (np.nan, np.inf):
        arr = good.copy()
        arr[pp.N + 0] = bad                 # node 0 of the second new step
        refused(h, api.roll_horizon(ctx, 3, dp(arr)), E_INVALID, snap, "demand_tail[%d] (node 0, t = %d)" % (pp.N, pp.T - 2))
        dem = _capi._f64(pp.demand.T)
        dem[2 * pp.N] = bad
        refused(h, api.set_demand(ctx, dp(dem)), E_INVALID, snap, "demand[%d] (node 0, t = 2)" % (2 * pp.N))
    refused(h, api.set_demand(ctx, None), E_INVALID, snap, "NULL")
    # storages in a context without DOPF_F_STO_INITIAL_LEVEL
    g = engine(hip_api, pp, None, flags=0, **kw_of(pp))
    g.iterate(3)
    snap_g = full_state(g)
    refused(g, g.api.roll_horizon(g._ctx, 3, dp(good)), E_UNSUPPORTED, snap_g, "DOPF_F_STO_INITIAL_LEVEL")
    # a context joined to a peer exchange
    g.xchg_export(1)
    refused(g, g.api.roll_horizon(g._ctx, 3, dp(good)), E_UNSUPPORTED, snap_g, "communicator")
    refused(g, g.api.set_demand(g._ctx, dp(_capi._f64(pp.demand.T))), E_UNSUPPORTED, snap_g, "communicator")


def test_refusal_of_an_unreachable_band(hip_api):
    """lo = hi = max_level, T * pmax = max_level / 2, and the storages emptied within the first k steps: from the new initial level
    0 the band cannot be reached"""
    pp = copper(24)
    pp.sto_pmax = pp.sto_emax / (2.0 * pp.T)
    h = engine(hip_api, pp, None, flags=IL | TL, **kw_of(pp))
    h.set_initial_levels(pp.sto_emax)
    h.set_terminal_levels(pp.sto_emax, pp.sto_emax)
    h.iterate(3)
    k = 4
    st = state_of(h)
    st["D"] = np.repeat((pp.sto_emax / k)[:, None], pp.T, axis=1)       # (a state handed in is not clamped until the next x-update)
    st["C"] = np.zeros_like(st["D"])
    set_from(h, st, 4)
    snap = full_state(h)
    assert np.all(snap["E"][:, k - 1] <= 1e-9)
    refused(h, h.api.roll_horizon(h._ctx, k, _capi._dp(_capi._f64(tail_of(pp, k).T))), E_INVALID, snap, "unreachable")
    with pytest.raises(_capi.DopfError, match="unreachable"):
        h.roll(k, tail_of(pp, k))
    same_bits(snap, full_state(h))


def test_refusal_of_a_level_that_is_not_a_number(hip_api):
    """a diverged state: shift_window keeps a NaN level NaN, and so does the device (a bare fmin / fmax would make it 0 and accept
    the roll); the roll is refused before anything is overwritten"""
    pp = copper(24)
    h = engine(hip_api, pp, None, flags=IL, **kw_of(pp))
    h.iterate(3)
    st = state_of(h)
    st["D"][2, 1] = np.nan
    set_from(h, st, 4)
    snap = full_state(h)
    assert np.isnan(shift_window(4, tail_of(pp, 4), demand=pp.demand, sto_emax=pp.sto_emax, E=snap["E"], **{n: snap[n] for n in MOVED})["e0"][2])
    rc = h.api.roll_horizon(h._ctx, 4, _capi._dp(_capi._f64(tail_of(pp, 4).T)))
    msg = h.api.last_error(h._ctx).decode()
    assert rc == E_INVALID and "initial level of storage 2 is" in msg and "nan" in msg, (rc, msg)
    after = full_state(h)
    for key in snap:
        assert np.array_equal(snap[key], after[key], equal_nan=True), key


# ---- graphs ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [lambda: copper(24), lambda: network(12)], ids=["copper", "net"])
def test_captured_graphs_stay_valid_across_a_roll(hip_api, case):
    pp = case()
    states = []
    for extra in (0, _capi.F_NO_GRAPH):
        h = engine(hip_api, pp, None, flags=IL | extra, **kw_of(pp))
        h.iterate(21)                       # graphs of 16, 4 and 1 iterations
        h.roll(5, tail_of(pp, 5))
        h.iterate(21)
        h.set_demand(h.demand() * 1.02)
        h.iterate(5)
        states.append(full_state(h))
    same_bits(*states)


# ---- a receding-horizon run -----------------------------------------------------------------------------------------------------

# The three-node case with the reference's literals (gamma 0.3, flow weight 10) converges only from an empty battery: once a window
# starts with stored energy the ADMM cycles, a cold fresh context as much as a rolled one (the CPU oracle shows the same
# on these windows, 5l). gamma 0.02 with flow weight 3 converges from every level, and the three-node tests with levels use it.
THREE_NODE = dict(gamma=0.02, w_flow=3.0)
LIMIT = 20000                                   # (a window takes about 2 000 iterations)


def test_receding_horizon_on_the_three_node_case(hip_api, three_node):
    """T = 2 extended to T = 6 by repeating the demand; run to convergence, roll by one step three times. Every window converges,
    and its cost is as near the central LP's as a cold run's on the same window: the allowed relative difference is twice the cold
    run's own plus 1e-6 (both stop on the same eps rule, from different starts)."""
    pp = copy.copy(three_node[4])
    pp.T = 6
    pp.demand = np.tile(three_node[4].demand, (1, 3))
    pp.sto_e0 = None
    h = engine(hip_api, pp, None, flags=IL, max_iters=LIMIT, **THREE_NODE)
    _, conv = h.iterate(LIMIT)
    assert conv
    demand = pp.demand
    for window in range(1, 4):
        E = h.get_primal()[3]
        e0 = np.minimum(np.maximum(E[:, 0], 0.0), pp.sto_emax)
        tail = demand[:, :1].copy()                         # the pattern of period 2 goes on
        demand = np.concatenate([demand[:, 1:], tail], axis=1)
        h.roll(1, tail)
        done, conv = h.iterate(LIMIT)
        assert conv and h.sync() == (h.get_residuals()[3], True), (window, done)
        warm = h.get_consensus()[4]
        pw = copy.copy(pp)
        pw.demand = demand
        cold_e = engine(hip_api, pw, None, flags=IL, max_iters=LIMIT, **THREE_NODE)
        cold_e.set_initial_levels(e0)
        done_cold, conv_cold = cold_e.iterate(LIMIT)
        assert conv_cold
        cold = cold_e.get_consensus()[4]
        ref = _capi.central_solve(hip_api, **pw.engine_kwargs(), sto_e0=e0, tol=1e-9, max_iters=400000)
        assert ref["converged"]
        obj = ref["objective"]
        d_warm, d_cold = abs(warm - obj) / abs(obj), abs(cold - obj) / abs(obj)
        print(f"window {window}: warm {warm:.4f} in {done} iterations ({d_warm:.2e}), cold {cold:.4f} in {done_cold} ({d_cold:.2e}), "
              f"central {obj:.4f}")
        assert d_warm <= 2.0 * d_cold + 1e-6, (window, d_warm, d_cold)


# ---- the debug allocator --------------------------------------------------------------------------------------------------------

def test_roll_under_the_debug_allocator():
    """DOPF_GUARD=1: every device array ends on the last byte of its own mapping, so an access past an end is a GPU memory fault in
    the child (tests/horizon_roll_worker.py) instead of a silent read of a neighbour."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "horizon_roll_worker.py")
    r = subprocess.run([sys.executable, worker], env=dict(os.environ, DOPF_GUARD="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "horizon roll worker: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
