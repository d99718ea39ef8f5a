"""DOPF_F_GEN_QUADRATIC_COST on the device: the generator step with quadratic costs against the CPU oracle one step
at a time (helpers_quadratic.slice_reference), its optimality certificate with heterogeneous coefficients, storages and
availability, the bits of the flagless kernels at c2 = 0, the setter, the total cost, convergence to the central QP and two
shards. Needs a real MI355X: pytest -m gpu."""
import copy

import numpy as np
import pytest
import torch  # noqa: F401  (before the library loads: ShardedADMM below runs on PyTorch's streams, and a process must hold one HIP runtime)

from decentralopf_jl_amd import _capi, synth
from helpers import draw_profiles, make_engine, max_diff, set_from, state_of
from helpers_line_rating import draw_table
from helpers_quadratic import (CHAIN, COPPER_EVEN, COPPER_ODD, NETWORK, QC, STATE_KEYS, case, draw_c2, gen_kkt_violation,
                               interior_fraction, params_of, quad_engine, slice_reference, solve_qp, total_cost)

pytestmark = pytest.mark.gpu

AV, LR = _capi.F_GEN_AVAILABILITY, _capi.F_LINE_RATING


def scaled_diff(got, want, keys):
    scale = max(1.0, float(np.abs(want["lam"]).max()))
    worst, where = max_diff(got, want, keys=keys)
    return worst / scale, where


# ---- 1. the oracle pin, one step at a time ---------------------------------------------------------------------------------------

PIN = [("copper-T5", COPPER_ODD, 0, False), ("copper-T5-eager", COPPER_ODD, _capi.F_NO_GRAPH, False),
       ("copper-T4", COPPER_EVEN, 0, False), ("copper-T4-eager", COPPER_EVEN, _capi.F_NO_GRAPH, False),
       ("net-6x8", NETWORK, 0, False), ("net-6x8-eager", NETWORK, _capi.F_NO_GRAPH, False),
       ("net-6x8-wide", NETWORK, _capi.F_DEBUG_WIDE_NET, False), ("net-6x8-rated", NETWORK, LR, True)]


@pytest.mark.parametrize("name,which,flags,rated", PIN, ids=[r[0] for r in PIN])
def test_one_step_against_the_oracle(hip_api, oracle_api, name, which, flags, rated):
    kw, c2, steps = which
    pp = case(kw)
    prm = params_of(pp)
    h = quad_engine(hip_api, pp, c2, flags=flags, **prm)
    rating = draw_table(pp) if rated else None
    if rated:
        h.set_line_rating(rating)
    assert h.wide_net() == (1 if flags & _capi.F_DEBUG_WIDE_NET else 0)
    tol = 1e-9 if pp.L == 0 else 1e-8
    worst, inside = 0.0, []
    for k in range(steps):
        before, it = state_of(h), h.get_residuals()[3]
        h.iterate(1)
        got = state_of(h)
        want = slice_reference(oracle_api, pp, c2, before, it, rating=rating, **prm)
        w, where = scaled_diff(got, want, STATE_KEYS)
        cost = abs(float(got["cost"][0] - want["cost"][0])) / max(1.0, abs(float(want["cost"][0])))
        print(f"{name} step {k}: {w:.2e} ({where}), cost {cost:.1e}")
        assert w <= tol and cost <= 1e-9, (k, where, w, cost)
        worst = max(worst, w)
        inside.append(interior_fraction(pp, got["P"]))
    assert np.mean(inside) >= 0.25, np.mean(inside)              # rows inside their box are where c2 shows
    assert h.solver_failures() == 0
    print(f"{name}: worst one-step difference {worst:.2e} (scaled), interior {np.mean(inside):.2f}")


# ---- 2. the certificate with heterogeneous c2, storages and availability ---------------------------------------------------------

def _one_node_network():
    """3 nodes / 3 lines, T = 128, all 19 generators on node 1: 4 agent lanes, more rows than the 16 in flight and no multiple"""
    pp = synth.synthetic_case(19, 3, 128, N=3, L=3, seed=6, fmax_factor=0.8, fmax_min=5)
    pp.gen_node = np.full(pp.G, 1, dtype=np.int32)
    return pp


def _three_node():
    from conftest import pkg
    nodes, lines, gens, stos = pkg.three_node_case()
    return pkg.pack(nodes, gens, stos, lines)


CERT = {"copper-9x4-T6": lambda: synth.synthetic_case(9, 4, 6, seed=5), "three-node": _three_node,
        "net-19-on-one-node-T128": _one_node_network, "copper-3x0-T600": lambda: synth.synthetic_case(3, 0, 600, seed=7)}


@pytest.mark.parametrize("avail", [False, True], ids=["pmax", "availability"])
@pytest.mark.parametrize("name", list(CERT))
def test_certificate_with_heterogeneous_c2(hip_api, name, avail):
    pp = CERT[name]()
    prm = dict(eps=0.0) if name == "three-node" else params_of(pp)
    gamma, wf = prm.get("gamma", 0.3), prm.get("w_flow", 10.0)
    rng = np.random.default_rng(11)
    c2 = draw_c2(pp.G, rng)
    extra = AV if avail else 0
    h = quad_engine(hip_api, pp, c2, flags=extra, **prm)
    twin = make_engine(hip_api, pp, flags=CHAIN | extra, **prm)        # no flag: the storages' launch of the same chain
    cap = np.repeat(pp.gen_pmax[:, None], pp.T, axis=1)
    if avail:
        prof, of = draw_profiles(pp, "K3", rng)
        for e in (h, twin):
            e.set_availability(prof, of)
        cap = np.where((of >= 0)[:, None], pp.gen_pmax[:, None] * prof[np.maximum(of, 0)], cap)
    worst = 0.0
    for k in range(10):
        st, it = state_of(h), h.get_residuals()[3]
        for e in (h, twin):
            set_from(e, st, it)
        before = state_of(h)
        h.iterate(1)
        twin.iterate(1)
        after, other = state_of(h), state_of(twin)
        v = gen_kkt_violation(pp, c2, cap, before, (before["lam"], before["mu"], before["rho"]), after["P"], gamma, wf)
        print(f"{name} step {k}: certificate {v:.2e}")
        assert v <= 1e-8, (k, v)
        worst = max(worst, v)
        assert np.array_equal(after["D"], other["D"]) and np.array_equal(after["C"], other["C"]), k      # the storages do not see c2
    assert h.solver_failures() == 0
    print(f"{name}: worst certificate {worst:.2e}")


# ---- 3. c2 = 0: the bits of the flagless kernels ----------------------------------------------------------------------------------

ZERO = [("copper-odd-T25", lambda: synth.synthetic_case(200, 16, 25, seed=702), 0, True),
        ("copper-odd-T5", lambda: synth.synthetic_case(9, 4, 5, seed=5), 0, True),
        ("three-node", _three_node, _capi.F_NO_FUSE, True),
        ("copper-even-T24", lambda: synth.synthetic_case(300, 24, 24, seed=701), 0, False),
        ("copper-even-T6", lambda: synth.synthetic_case(9, 4, 6, seed=5), 0, False)]


@pytest.mark.parametrize("name,make,other_flags,bitwise", ZERO, ids=[r[0] for r in ZERO])
@pytest.mark.parametrize("set_zeros", [False, True], ids=["until-the-first-call", "zeros-set"])
def test_c2_0_is_the_flagless_context(hip_api, name, make, other_flags, bitwise, set_zeros):
    pp = make()
    prm = dict(eps=0.0) if name == "three-node" else params_of(pp)
    h = quad_engine(hip_api, pp, np.zeros(pp.G) if set_zeros else None, **prm)
    ref = make_engine(hip_api, pp, flags=other_flags, **prm)
    for n in (1, 4, 20):
        h.iterate(n)
        ref.iterate(n)
        a, b = state_of(h), state_of(ref)
        if bitwise:
            for k in a:
                assert np.array_equal(a[k], b[k]), (n, k)
        else:
            w, where = scaled_diff(a, b, [k for k in a if k != "cost"])
            assert w <= 1e-9, (n, where, w)
            assert abs(float(a["cost"][0] - b["cost"][0])) <= 1e-9 * max(1.0, abs(float(b["cost"][0])))


# ---- 4. the setter ----------------------------------------------------------------------------------------------------------------

def test_setter_refusals_store_nothing(hip_api):
    pp = case(COPPER_ODD[0])
    prm = params_of(pp)
    with pytest.raises(_capi.DopfError, match=r"\(-4\).*DOPF_F_GEN_QUADRATIC_COST"):      # DOPF_E_UNSUPPORTED
        make_engine(hip_api, pp, **prm).set_quadratic_cost(np.zeros(pp.G))
    c2 = np.linspace(0.1, 0.7, pp.G)
    h, twin = quad_engine(hip_api, pp, c2, **prm), quad_engine(hip_api, pp, c2, **prm)
    h.iterate(3)
    twin.iterate(3)
    for g, bad in ((2, np.nan), (5, np.inf), (0, -1e-3)):
        x = c2.copy()
        x[g] = bad
        with pytest.raises(_capi.DopfError, match=r"\(-1\).*c2\[%d\]" % g):              # DOPF_E_INVALID, naming the entry
            h.set_quadratic_cost(x)
    assert h.iterate(5) == twin.iterate(5)
    a, b = state_of(h), state_of(twin)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("which", [COPPER_EVEN, NETWORK], ids=["copper-T4", "net-6x8"])
def test_setter_between_graph_replays(hip_api, which):
    kw, c2, _ = which
    pp = case(kw)
    prm = params_of(pp)
    rng = np.random.default_rng(3)
    h = quad_engine(hip_api, pp, c2, **prm)
    h.iterate(16)
    new = draw_c2(pp.G, rng)
    for vals in (new, None):                                     # None: back to 0
        st, it = state_of(h), h.get_residuals()[3]
        h.set_quadratic_cost(vals)
        assert h.get_residuals()[3] == it                        # the iteration counter is kept
        now = state_of(h)
        for k in ("P", "lam", "mu", "rho", "avg_U", "avg_K", "inj"):
            assert np.array_equal(now[k], st[k]), k
        fresh = quad_engine(hip_api, pp, vals, **prm)
        set_from(fresh, st, it)
        h.iterate(4)
        fresh.iterate(4)
        a, b = state_of(h), state_of(fresh)
        w, where = scaled_diff(a, b, STATE_KEYS)
        assert w <= (1e-9 if pp.L == 0 else 1e-8), (where, w)
        want = total_cost(pp, np.zeros(pp.G) if vals is None else vals, a["P"])
        assert abs(float(a["cost"][0]) - want) <= 1e-9 * max(1.0, abs(want))


def test_setter_resets_converged(hip_api):
    kw, c2, _ = COPPER_ODD
    pp = case(kw)
    h = quad_engine(hip_api, pp, c2, gamma=1.0 / pp.G, max_iters=20000)
    done, conv = h.iterate(20000)
    assert conv and h.iterate(5) == (0, True)
    it = h.get_residuals()[3]
    h.set_quadratic_cost(np.full(pp.G, 2.0 * c2))
    assert h.sync() == (it, False)
    done, conv = h.iterate(20000)
    assert done > 0 and conv


# ---- 5. the total cost ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["copper-9x4-T6", "three-node", "net-19-on-one-node-T128", "copper-3x0-T600"])
def test_total_cost_is_the_quadratic_cost(hip_api, name):
    pp = CERT[name]()
    prm = dict(eps=0.0) if name == "three-node" else params_of(pp)
    c2 = draw_c2(pp.G, np.random.default_rng(5))
    h = quad_engine(hip_api, pp, c2, **prm)
    for n in (1, 7):
        h.iterate(n)
        st = state_of(h)
        want = total_cost(pp, c2, st["P"], st["D"], st["C"])
        assert abs(float(st["cost"][0]) - want) <= 1e-9 * abs(want), (n, float(st["cost"][0]), want)
    assert abs(want - total_cost(pp, 0.0, st["P"], st["D"], st["C"])) > 1e-3 * abs(want)      # (the quadratic part is visible)


# ---- 6. convergence ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", [COPPER_ODD, COPPER_EVEN], ids=["copper-T5", "copper-T4"])
def test_copper_plates_converge_to_the_central_qp(hip_api, which):
    """The reference's parameters (gamma 0.3, eps 1e-3). The stop test bounds gamma * |imbalance|, so the balance at the stop is not
    below eps by construction; the CPU emulation (slice_reference) of these two cases stops after 18 iterations with an imbalance of
    5.9e-4 resp. 5.7e-4 and a cost within 9e-7 of the QP's."""
    kw, c2, _ = which
    pp = case(kw)
    h = quad_engine(hip_api, pp, c2, max_iters=20000)
    done, conv = h.iterate(20000)
    st = state_of(h)
    obj = solve_qp(pp, c2)[0]
    rel = abs(float(st["cost"][0]) - obj) / obj
    bal = float(np.abs(st["inj"].sum(axis=0)).max())
    print(f"converged {conv} after {done}: cost {float(st['cost'][0]):.6f}, QP {obj:.6f} ({rel:.1e}), balance {bal:.1e}")
    assert conv
    assert rel <= 1e-3 and bal <= h.params.eps, (rel, bal)


def test_three_node_case_converges_to_the_central_qp(hip_api):
    """The shipped case with c2 = 0.02 on every generator, the reference's parameters, at most 20 000 iterations. No CPU reference
    reaches it (the oracle takes no c2 with storages). Measured on an MI355X: converged after 506 iterations (476 at c2 = 0), cost
    14984.99 against the QP's 14985.50 (3.4e-5), imbalance 8.6e-8."""
    pp = _three_node()
    h = quad_engine(hip_api, pp, 0.02, max_iters=20000)
    hist, done, conv = [], 0, False
    while done < 20000 and not conv:
        d, conv = h.iterate(1000)
        done += d
        hist.append((done,) + tuple(float(x) for x in h.get_residuals()[:3]))
        if d == 0:
            break
    st = state_of(h)
    obj = solve_qp(pp, 0.02)[0]
    rel = abs(float(st["cost"][0]) - obj) / obj
    bal = float(np.abs(st["inj"].sum(axis=0)).max())
    print(f"residuals (iterations, lambda, mu, rho): {hist}")
    print(f"converged {conv} after {done}: cost {float(st['cost'][0]):.6f}, QP {obj:.6f} ({rel:.1e}), balance {bal:.1e}")
    assert conv
    assert rel <= 1e-3 and bal <= h.params.eps, (rel, bal)


# ---- 7. two shards ----------------------------------------------------------------------------------------------------------------

SHARDS = {"network": lambda: synth.synthetic_case(30, 6, 6, N=3, L=3, seed=4, fmax_factor=0.8, fmax_min=5),
          "copper plate": lambda: synth.synthetic_case(41, 7, 6, seed=4)}


def _close(got, want, keys, who):
    for key in keys:
        if want[key].size:
            assert np.abs(got[key] - want[key]).max() <= 1e-9 * max(1.0, np.abs(want[key]).max()), (key, who)


@pytest.mark.parametrize("name", list(SHARDS))
def test_multi_two_shards_equal_one_context(hip_api, name):
    pp = SHARDS[name]()
    g = 0.01 if name == "network" else 1.0 / (pp.G + pp.S)
    c2 = draw_c2(pp.G, np.random.default_rng(9))
    ref = quad_engine(hip_api, pp, c2, eps=0.0, gamma=g)
    q = copy.copy(pp)
    q.gen_c2 = c2                                                # (through engine_kwargs: the flag and the setter from the constructor)
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(eps=0.0, gamma=g, flags=_capi.F_COMM_HOST), **q.engine_kwargs())
    assert m.params.flags & QC
    for k in (1, 4, 7):
        ref.iterate(k)
        assert m.iterate(k) == (k, False)
        want = state_of(ref)
        P, D, C, E = m.get_primal()
        _close(dict(P=P, D=D, C=C, E=E), want, ("P", "D", "C", "E"), "primal")
        for i in range(2):
            _close(state_of(m.shard(i)), want, ("lam", "mu", "rho", "inj", "avg_U", "avg_K", "flow", "cost"), i)
    bad = c2.copy()
    bad[pp.G - 1] = -1.0                                         # the second shard's last entry: nothing stored on the first either
    with pytest.raises(_capi.DopfError, match="shard 1"):
        m.set_quadratic_cost(bad)
    ref.iterate(3)
    assert m.iterate(3) == (3, False)
    _close(state_of(m.shard(0)), state_of(ref), ("lam", "inj", "cost"), "after a refusal")
    m.set_quadratic_cost(None)
    ref.set_quadratic_cost(None)
    ref.iterate(3)
    m.iterate(3)
    _close(state_of(m.shard(1)), state_of(ref), ("lam", "inj", "cost"), "reset")
    m.close()


@pytest.mark.parametrize("name", list(SHARDS))
def test_sharded_admm_two_ranks_equal_one_context(hip_api, name):
    import torch
    from conftest import pkg
    pp = SHARDS[name]()
    g = 0.01 if name == "network" else 1.0 / (pp.G + pp.S)
    c2 = draw_c2(pp.G, np.random.default_rng(9))
    ref = quad_engine(hip_api, pp, c2, eps=0.0, gamma=g)
    ranks = [pkg.ShardedADMM(pp, r, 2, all_reduce=lambda: None, eps=0.0, gamma=g, flags=QC) for r in range(2)]
    for sh in ranks:
        sh.set_quadratic_cost(c2)                                # all G values: each rank takes its slice
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
        _close(s, want, ("lam", "mu", "rho", "inj", "avg_U", "avg_K", "flow", "cost"), i)
    assert np.abs(np.concatenate([s["P"] for s in got]) - want["P"]).max() <= 1e-9 * max(1.0, np.abs(want["P"]).max())
