"""DOPF_F_GEN_RAMP on the GPU: the generators' step under ramp limits (k_gen_ramp) against the NumPy projection row by
row and against its optimality certificate, the bits of the flagless chain with every ramp at +inf, the setter, convergence to the
host LP with ramp rows, two shards against one context, and Engine.roll's host route."""
import copy

import numpy as np
import pytest

from decentralopf_jl_amd import _capi, central, synth
from helpers import draw_profiles, make_engine, set_from, state_of
from helpers_quadratic import QC, draw_c2, params_of
from helpers_ramp import (CHAIN, RAMP, draw_ramps, ramp_active, ramp_engine, ramp_infeasibility, ramp_kkt_violation, ramp_project,
                          step_centres)

pytestmark = pytest.mark.gpu
AV = _capi.F_GEN_AVAILABILITY
LONG = _capi.F_LONG_HORIZON


def swing(pp, lo=0.4, hi=1.6):
    """the case with its demand alternating between lo and hi times itself: what makes neighbouring steps of a row differ"""
    f = np.where(np.arange(pp.T) % 2 == 0, lo, hi)
    pp.demand = np.round(np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T) * f[None, :])
    return pp


# name -> (case, flags, warm-up iterations, anchored)
SHAPES = {
    "7x5": (lambda: swing(synth.synthetic_case(7, 0, 5, seed=3)), 0, 3, False),
    "7x4": (lambda: swing(synth.synthetic_case(7, 0, 4, seed=3)), 0, 3, False),
    "9xT1-anchored": (lambda: synth.synthetic_case(9, 0, 1, seed=4), 0, 2, True),
    "7xT2": (lambda: swing(synth.synthetic_case(7, 0, 2, seed=3)), 0, 3, True),
    "70+6xT96-3-nodes": (lambda: swing(synth.synthetic_case(70, 6, 96, N=3, seed=8)), 0, 3, False),
    "11xT130": (lambda: swing(synth.synthetic_case(11, 2, 130, seed=9)), 0, 3, True),
    "3xT600-long": (lambda: swing(synth.synthetic_case(3, 0, 600, seed=7)), LONG, 3, False),
}
EXTRAS = {"plain": (False, False), "availability": (True, False), "c2": (False, True), "availability+c2": (True, True)}


def _setup(hip_api, name, extra, eager):
    """(pp, prm, ramped engine, flagless twin on the chain, c2, cap, up, down, prev) of a shape with its extras set"""
    make, flags, warm, anchored = SHAPES[name]
    avail, quad = EXTRAS[extra]
    pp = make()
    prm = params_of(pp)
    rng = np.random.default_rng(17)
    up, down = draw_ramps(pp, rng)
    c2 = draw_c2(pp.G, rng) if quad else np.zeros(pp.G)
    flags |= (AV if avail else 0) | (QC if quad else 0) | (_capi.F_NO_GRAPH if eager else 0)
    h = ramp_engine(hip_api, pp, flags=flags, **prm)
    twin = make_engine(hip_api, pp, flags=flags | CHAIN, **prm)
    cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
    if avail:
        prof, of = draw_profiles(pp, "K3", rng)
        for e in (h, twin):
            e.set_availability(prof, of)
        cap = np.where((of >= 0)[:, None], pp.gen_pmax[:, None] * prof[np.maximum(of, 0)], cap)
    if quad:
        for e in (h, twin):
            e.set_quadratic_cost(c2)
    prev = None
    if anchored:            # anchors that can come down under the caps: at or below the smallest cap of the row
        prev = rng.uniform(0.0, 1.0, pp.G) * cap.min(axis=1)
    h.set_ramp(up, down, prev)
    return pp, prm, h, twin, c2, cap, up, down, prev, warm


@pytest.mark.parametrize("eager", [False, True], ids=["graphs", "eager"])
@pytest.mark.parametrize("extra", list(EXTRAS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_one_step_against_the_projection_and_the_certificate(hip_api, name, extra, eager):
    """One step from the device's own state: P against ramp_project row by row (1e-9 scaled by the row's capacity, the parity
    tests' bound for a primal value), the certificate of every row at 1e-8, D and C the bits of the flagless twin on the chain."""
    pp, prm, h, twin, c2, cap, up, down, prev, warm = _setup(hip_api, name, extra, eager)
    gamma = prm["gamma"]
    h.iterate(warm)
    st, it = state_of(h), h.get_residuals()[3]
    for e in (h, twin):
        set_from(e, st, it)
    before = state_of(h)
    h.iterate(1)
    twin.iterate(1)
    after, other = state_of(h), state_of(twin)
    c, q = step_centres(pp, c2, before, gamma)
    active = free = 0
    worst = cert = 0.0
    for g in range(pp.G):
        pv = None if prev is None else float(prev[g])
        want = ramp_project(c[g], q[g], cap[g], up[g], down[g], pv)
        on = ramp_active(want, up[g], down[g], pv)
        active, free = active + on, free + (not on)
        worst = max(worst, float(np.abs(after["P"][g] - want).max()) / max(1.0, float(pp.gen_pmax[g])))
        grad = pp.gen_mc[g] + c2[g] * after["P"][g] + before["lam"] + gamma * (before["inj"].sum(axis=0) + after["P"][g] - before["P"][g]) \
            + (after["P"][g] - before["P"][g])
        infeas, stat = ramp_kkt_violation(after["P"][g], grad, cap[g], up[g], down[g], pv)
        cert = max(cert, stat)
        assert infeas <= 1e-9, (g, infeas)
    print(f"{name} {extra}: |P - projection| {worst:.2e} (scaled), certificate {cert:.2e}, rows with an active ramp {active}/{pp.G}, "
          f"with none {free}/{pp.G}")
    assert 5 * active >= pp.G and 5 * free >= pp.G, (active, free, pp.G)
    assert worst <= 1e-9, worst
    assert cert <= 1e-8, cert
    assert np.array_equal(after["D"], other["D"]) and np.array_equal(after["C"], other["C"])      # the storages do not see the ramps
    assert h.solver_failures() == 0


# ---- 3. every ramp +inf, no anchor: the bits of the flagless chain -------------------------------------------------------------------

FREE = [("copper-odd-T25", lambda: synth.synthetic_case(200, 16, 25, seed=702), True),
        ("copper-odd-T5", lambda: synth.synthetic_case(9, 4, 5, seed=5), True),
        ("copper-even-T24", lambda: synth.synthetic_case(300, 24, 24, seed=701), False),
        ("copper-even-T6", lambda: synth.synthetic_case(9, 4, 6, seed=5), False)]


@pytest.mark.parametrize("quad", [False, True], ids=["linear", "c2"])
@pytest.mark.parametrize("name,make,bitwise", FREE, ids=[r[0] for r in FREE])
def test_all_ramps_inf_is_the_flagless_chain(hip_api, name, make, bitwise, quad):
    pp = make()
    prm = params_of(pp)
    c2 = draw_c2(pp.G, np.random.default_rng(5))
    h = ramp_engine(hip_api, pp, flags=QC if quad else 0, **prm)
    ref = make_engine(hip_api, pp, flags=CHAIN | (QC if quad else 0), **prm)
    if quad:
        for e in (h, ref):
            e.set_quadratic_cost(c2)
    ref.iterate(3)
    st, it = state_of(ref), ref.get_residuals()[3]
    for e in (h, ref):
        set_from(e, st, it)
    h.iterate(1)
    ref.iterate(1)
    assert np.array_equal(state_of(h)["P"], state_of(ref)["P"])          # one step from the same state: the same bits on every T
    h.iterate(24)
    ref.iterate(24)
    a, b = state_of(h), state_of(ref)
    if bitwise:
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    else:
        for k in ("P", "D", "C", "lam", "inj"):
            scale = max(1.0, float(np.abs(b[k]).max()))
            assert float(np.abs(a[k] - b[k]).max()) <= 1e-9 * scale, k


# ---- 4. the setter --------------------------------------------------------------------------------------------------------------------

def _small():
    return swing(synth.synthetic_case(7, 0, 5, seed=3))


def test_setter_refusals_store_nothing(hip_api):
    pp = _small()
    prm = params_of(pp)
    G = pp.G
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*DOPF_F_GEN_RAMP"):        # DOPF_E_UNSUPPORTED
        make_engine(hip_api, pp, **prm).set_ramp(np.ones(G), np.ones(G))
    up, down = 0.1 * pp.gen_pmax, 0.2 * pp.gen_pmax
    prev = 0.5 * pp.gen_pmax
    prof, of = np.full((1, pp.T), 0.75), np.zeros(G, dtype=np.int32)
    h, twin = (ramp_engine(hip_api, pp, (up, down), prev, flags=AV, **prm) for _ in range(2))
    for e in (h, twin):
        e.set_availability(prof, of)
        e.iterate(3)
    def bad(a, g, v):
        x = a.copy()
        x[g] = v
        return x
    for args, what in (((bad(up, 2, np.nan), down, prev), r"ramp_up\[2\]"), ((up, bad(down, 5, -1e-3), prev), r"ramp_down\[5\]"),
                       ((bad(up, 1, -1.0), down, None), r"ramp_up\[1\]"), ((up, down, bad(prev, 4, np.nan)), r"p_prev\[4\]"),
                       ((up, down, bad(prev, 3, 1.01 * pp.gen_pmax[3])), r"p_prev\[3\]"), ((up, down, bad(prev, 0, -1.0)), r"p_prev\[0\]")):
        with pytest.raises(_capi.DopfError, match=r"\(-1\).*" + what):                # DOPF_E_INVALID, naming the entry
            h.set_ramp(*args)
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*both"):
        h._chk(h.api.set_generator_ramp(h._ctx, _capi._dp(up), None, None))
    # an anchor that cannot come down under its cap: generator 6 at 0.5 pmax with ramp_down 0.2 pmax is still at 0.1 pmax at t = 1,
    # under a cap that drops to 0 there
    drop = np.vstack([prof, np.where(np.arange(pp.T) == 1, 0.0, 1.0)[None, :]])
    of2 = bad(of, 6, 1)
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*g = 6 .*t = 1"):              # the availability setter's re-check
        h.set_availability(drop, of2)
    with pytest.raises(_capi.DopfError, match=r"\(-1\).*g = 1 .*t = 0"):              # 0.75 pmax + 0.1 pmax < 0.95 pmax
        h.set_ramp(up, 0.1 * pp.gen_pmax, bad(prev, 1, 0.95 * pp.gen_pmax[1]))
    assert h.iterate(5) == twin.iterate(5)
    a, b = state_of(h), state_of(twin)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_create_refuses_lines_and_roll_horizon_is_refused(hip_api):
    net = synth.synthetic_case(12, 0, 4, N=6, L=8, seed=2)
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*copper plates"):
        ramp_engine(hip_api, net, **params_of(net))
    pp = _small()
    h = ramp_engine(hip_api, pp, **params_of(pp))
    h.iterate(2)
    tail = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, :1]
    rc = h.api.roll_horizon(h._ctx, 1, _capi._dp(_capi._f64(tail.T)))
    assert rc == -4 and b"DOPF_F_GEN_RAMP" in h.api.last_error(h._ctx)


def test_setter_between_graph_replays_resets_converged_and_null_restores_inf(hip_api):
    pp = _small()
    prm = params_of(pp)
    rng = np.random.default_rng(3)
    h = ramp_engine(hip_api, pp, draw_ramps(pp, rng), **prm)
    h.iterate(16)
    prev = rng.uniform(0.0, 1.0, pp.G) * pp.gen_pmax
    for ramp, pv in ((draw_ramps(pp, rng), prev), ((None, None), None)):        # None: back to +inf, no anchor
        st, it = state_of(h), h.get_residuals()[3]
        h.set_ramp(*ramp, pv)
        assert h.get_residuals()[3] == it                                       # the iteration counter is kept
        now = state_of(h)
        for k in ("P", "lam", "inj"):
            assert np.array_equal(now[k], st[k]), k
        fresh = ramp_engine(hip_api, pp, None if ramp[0] is None else ramp, pv, **prm)
        for e in (h, fresh):                                                    # (both from the getters' values: the same node sums)
            set_from(e, st, it)
        h.iterate(4)
        fresh.iterate(4)
        a, b = state_of(h), state_of(fresh)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    ref = make_engine(hip_api, pp, flags=CHAIN, **prm)                          # +inf again: the flagless chain's bits (odd T)
    st, it = state_of(h), h.get_residuals()[3]
    for e in (h, ref):
        set_from(e, st, it)
    h.iterate(3)
    ref.iterate(3)
    assert np.array_equal(state_of(h)["P"], state_of(ref)["P"])
    # converged is reset
    pp = synth.synthetic_case(7, 0, 5, seed=3)                                  # (the case without the swing: it converges)
    e = ramp_engine(hip_api, pp, gamma=1.0 / pp.G, max_iters=20000)
    done, conv = e.iterate(20000)
    assert conv and e.iterate(5) == (0, True)
    it = e.get_residuals()[3]
    e.set_ramp(0.05 * pp.gen_pmax, 0.05 * pp.gen_pmax)
    assert e.sync() == (it, False)


# ---- 5. convergence to the host LP with ramp rows -------------------------------------------------------------------------------------

# name -> (case, gamma). The plate with storages runs at gamma = 1 / agents: at the reference's 0.3 the flagless problem itself does not
# converge (the CPU oracle, no ramps: 20 000 iterations and an imbalance of 269; at 1 / 13 it stops after 136)
CONV = {"7x5": (lambda: swing(synth.synthetic_case(7, 0, 5, seed=3), 0.85, 1.15), 0.3),
        "9+4xT6": (lambda: swing(synth.synthetic_case(9, 4, 6, seed=5), 0.85, 1.15), 1.0 / 13)}


@pytest.mark.parametrize("name", list(CONV))
def test_converged_run_against_the_host_lp(hip_api, name):
    """The cost bound of the quadratic-cost convergence tests (within 1e-3 of the central optimum), 1e-9 for the ramps, which the
    exact projection keeps in every iteration, and for the balance what the stop test gives: it bounds the change of lambda,
    gamma * |imbalance|, by eps, so |imbalance| < eps / gamma at the stop (not eps: gamma < 1 here). Measured figures: DESIGN.md 5r."""
    make, gamma = CONV[name]
    pp = make()
    up, down = 0.2 * pp.gen_pmax, 0.2 * pp.gen_pmax
    up[::3] = np.inf
    want = central.solve_central_packed(pp, gen_ramp=(up, down))
    free = central.solve_central_packed(pp)
    assert want.objective > free.objective * (1.0 + 1e-6)                      # the ramps bind at the optimum
    h = ramp_engine(hip_api, pp, (up, down), gamma=gamma, max_iters=20000)     # (eps: the reference's 1e-3)
    done, conv = h.iterate(20000)
    st = state_of(h)
    gap = abs(float(st["cost"][0]) - want.objective) / want.objective
    bal = float(np.abs(st["inj"].sum(axis=0)).max())
    viol = max(ramp_infeasibility(st["P"][g], pp.gen_pmax[g], up[g], down[g]) for g in range(pp.G))
    print(f"{name}: converged {conv} after {done} iterations, relative cost gap {gap:.2e}, balance {bal:.1e}, largest ramp violation "
          f"{viol:.2e}, LP {want.objective:.4f} (without ramps {free.objective:.4f})")
    assert conv
    assert viol <= 1e-9, viol
    assert gap <= 1e-3 and bal <= h.params.eps / h.params.gamma, (gap, bal)


# ---- 6. two shards against one context ------------------------------------------------------------------------------------------------

def _close(got, want, keys, who):
    for key in keys:
        if want[key].size:
            assert np.abs(got[key] - want[key]).max() <= 1e-9 * max(1.0, np.abs(want[key]).max()), (key, who)


def test_multi_two_shards_equal_one_context(hip_api):
    pp = swing(synth.synthetic_case(41, 7, 6, seed=4))
    g = 1.0 / (pp.G + pp.S)
    rng = np.random.default_rng(4)
    up, down = draw_ramps(pp, rng)
    prev = rng.uniform(0.0, 1.0, pp.G) * pp.gen_pmax
    ref = ramp_engine(hip_api, pp, (up, down), prev, eps=0.0, gamma=g)
    q = copy.copy(pp)
    q.gen_ramp = (up, down)                                      # (through engine_kwargs: the flag and the setter from the constructor)
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(eps=0.0, gamma=g, flags=_capi.F_COMM_HOST), gen_prev=prev,
                          **q.engine_kwargs())
    assert m.params.flags & RAMP
    for k in (1, 4, 7):
        ref.iterate(k)
        assert m.iterate(k) == (k, False)
        want = state_of(ref)
        P, D, C, E = m.get_primal()
        _close(dict(P=P, D=D, C=C, E=E), want, ("P", "D", "C", "E"), "primal")
        for i in range(2):
            _close(state_of(m.shard(i)), want, ("lam", "inj", "cost"), i)
    bad = up.copy()
    bad[pp.G - 1] = -1.0                                         # the second shard's last entry: nothing stored on the first either
    with pytest.raises(_capi.DopfError, match="shard 1"):
        m.set_ramp(bad, down, prev)
    ref.iterate(3)
    assert m.iterate(3) == (3, False)
    _close(state_of(m.shard(0)), state_of(ref), ("lam", "inj", "cost"), "after a refusal")
    m.set_ramp(None, None, None)
    ref.set_ramp(None, None, None)
    ref.iterate(3)
    m.iterate(3)
    _close(state_of(m.shard(1)), state_of(ref), ("lam", "inj", "cost"), "reset")
    m.close()


def test_sharded_admm_two_ranks_equal_one_context(hip_api):
    import torch
    from conftest import pkg
    pp = swing(synth.synthetic_case(41, 7, 6, seed=4))
    g = 1.0 / (pp.G + pp.S)
    rng = np.random.default_rng(4)
    up, down = draw_ramps(pp, rng)
    prev = rng.uniform(0.0, 1.0, pp.G) * pp.gen_pmax
    ref = ramp_engine(hip_api, pp, (up, down), prev, eps=0.0, gamma=g)
    ranks = [pkg.ShardedADMM(pp, r, 2, all_reduce=lambda: None, eps=0.0, gamma=g, flags=RAMP) for r in range(2)]
    for sh in ranks:
        sh.set_ramp(up, down, prev)                              # all G values: each rank takes its slice
    for _ in range(12):
        for sh in ranks:
            sh.engine.local_update()
        for sh in ranks:
            sh.sync()
        total = ranks[0]._tensor.cpu() + ranks[1]._tensor.cpu()          # (summed on the host: no PyTorch kernel has to load)
        for sh in ranks:
            sh._tensor.copy_(total)
        torch.cuda.synchronize()
        for sh in ranks:
            sh.engine.apply_consensus()
        for sh in ranks:
            sh.sync()
    ref.iterate(12)
    want = state_of(ref)
    got = [state_of(sh.engine) for sh in ranks]
    for i, s in enumerate(got):
        _close(s, want, ("lam", "inj", "cost"), i)
    assert np.abs(np.concatenate([s["P"] for s in got]) - want["P"]).max() <= 1e-9 * max(1.0, np.abs(want["P"]).max())


# ---- 7. Engine.roll on a ramp context: the host route -------------------------------------------------------------------------------

def test_engine_roll_carries_the_anchor(hip_api):
    pp = _small()
    prm = params_of(pp)
    up, down = 0.1 * pp.gen_pmax, 0.1 * pp.gen_pmax
    h = ramp_engine(hip_api, pp, (up, down), **prm)
    h.iterate(20)
    P = h.get_primal()[0]
    k = 2
    tail = np.asarray(pp.demand, dtype=np.float64).reshape(pp.N, pp.T)[:, :k]
    h.roll(k, tail)
    assert h.params.flags & RAMP
    assert np.array_equal(h._mirror["gen_prev"], P[:, k - 1]) and np.array_equal(h._mirror["gen_ramp"][0], up)
    assert np.array_equal(h.get_primal()[0][:, :pp.T - k], P[:, k:])           # the window moved
    h.iterate(1)
    P1 = h.get_primal()[0]
    d0 = P1[:, 0] - P[:, k - 1]
    assert np.all(d0 <= up + 1e-9) and np.all(-d0 <= down + 1e-9)              # the first step obeys the ramps against the anchor
    assert max(ramp_infeasibility(P1[g], pp.gen_pmax[g], up[g], down[g], float(P[g, k - 1])) for g in range(pp.G)) <= 1e-9
