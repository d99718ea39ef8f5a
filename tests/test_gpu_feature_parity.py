"""Storage initial levels, terminal bands and generator availability (DESIGN.md sections 5h-5j) on every chain, against the
oracle's exact mode with the same inputs: one step at a time (the HIP state reset to the oracle's after every iteration), the
setters between iterate(n) calls of graph-replayed chains, free runs, and negative controls. Needs a real MI355X: pytest -m gpu."""
import numpy as np
import pytest

from conftest import build_oracle
from decentralopf_jl_amd import _capi, synth
from helpers import Features, degenerate, draw_band, draw_e0, draw_profiles, engine, max_diff, set_from, state_of

pytestmark = pytest.mark.gpu

IL, TL, AV = _capi.F_STO_INITIAL_LEVEL, _capi.F_STO_TERMINAL_LEVEL, _capi.F_GEN_AVAILABILITY
ALL = IL | TL | AV
LH = _capi.F_LONG_HORIZON
NET = dict(N=4, L=5, fmax_factor=0.7, fmax_min=5)
NET30 = dict(N=30, L=45, fmax_factor=0.7, fmax_min=10)


@pytest.fixture(scope="module")
def fapi():
    from oracle.binding import OracleApi
    return OracleApi(build_oracle(), features=True)


def compare(sh, so, tol):
    scale = max(1.0, float(np.abs(so["lam"]).max()))
    worst, where = max_diff(sh, so, keys=[k for k in sh if k != "cost"])
    cost = abs(float(sh["cost"][0] - so["cost"][0])) / max(1.0, abs(float(so["cost"][0])))
    return worst / scale, where, cost


def one_step(h, o, iters, tol, expect=None):
    """HIP and oracle one iteration each from the oracle's state; the first HIP iteration through dopf_iterate_timed, whose
    fields must show `expect`. Returns the worst scaled difference."""
    worst = 0.0
    for k in range(iters):
        if k == 0 and expect:
            got = h.iterate_timed(1)
            for f, v in expect.items():
                assert got[f] == v, (f, got[f], v)
        else:
            h.iterate(1)
        o.iterate(1)
        w, where, cost = compare(state_of(h), state_of(o), tol)
        assert w <= tol and cost <= 1e-9, (k, where, w, cost)
        worst = max(worst, w)
        set_from(h, state_of(o), o.get_residuals()[3])
    assert h.solver_failures() == 0
    return worst


# ---- one step at a time, every chain that carries LV 1 / 2 and every generator body with availability -----------------------
# name, case, extra flags, features (e0, band, profiles), degenerate storages, gamma, iterations, expected dopf_timing fields.
# The comment names the kernels the row reaches with the levels (LV 1 / 2) or the profiles (_av).

CP = dict(n_gen=300, n_sto=24, T=24, seed=701)
ONE = [
    # k_agents<..., LV 2> (the fused copper plate on the general body) and k_agents<..., AV>
    ("copper-fused", CP, 0, ("mix", "mix", "K3"), "emax0", 0.02, 8, dict(agents_fused=1, sto_lean=0, sto_long=0)),
    # k_agents<..., LV 1> without a band, the lean body's chain otherwise
    ("copper-fused-e0-only", CP, 0, ("inside", None, None), "", 0.02, 6, dict(agents_fused=1, sto_lean=0)),
    # k_agents<..., LV 2> with the band alone (e0 slot all zeros)
    ("copper-fused-band-only", CP, 0, (None, "eq", None), "pmax0", 0.02, 6, dict(agents_fused=1, sto_lean=0)),
    # k_sto<..., LV 2> + k_gen_update_pair<MODE, AV>: separate launches
    ("copper-no-fuse", CP, _capi.F_NO_FUSE, ("mix", "cyclic", "KG"), "emax0+pmax0", 0.02, 6, dict(agents_fused=0, sto_long=0)),
    # k_sto<..., LV 2> + k_gen_update<LINES, AV> (no row skipping)
    ("copper-no-fuse-no-skip", CP, _capi.F_NO_FUSE | _capi.F_NO_ROW_SKIP, ("full", "edge-lo", "K1"), "", 0.02, 5, dict(agents_fused=0)),
    # odd T: the separate-launch chain with k_gen_update<LINES, AV>
    ("copper-odd-T25", dict(n_gen=200, n_sto=16, T=25, seed=702), 0, ("mix", "mix", "K3"), "emax0", 0.02, 5, dict(agents_fused=0)),
    # k_sto_update<..., LV 2> (the scan body: 193 <= T <= 512)
    ("copper-T250-scan", dict(n_gen=30, n_sto=6, T=250, seed=703), 0, ("mix", "mix", "K3"), "emax0", 0.02, 4, dict(sto_long=0)),
    ("copper-T512-scan", dict(n_gen=30, n_sto=6, T=512, seed=704), 0, ("inside", "eq", "K1"), "", 0.02, 3, dict(sto_long=0)),
    # k_sto_update<..., LV 2> at T <= 192: the cold scan body for every storage
    ("copper-T24-no-warm", CP, _capi.F_NO_WARM_START, ("mix", "mix", "K3"), "pmax0", 0.02, 5, dict(sto_long=0)),
    # k_agents<..., LV 2> handing every third storage to k_sto_update<..., LV 2>
    ("copper-debug-leave", CP, _capi.F_DEBUG_LEAVE, ("mix", "mix", "K3"), "emax0", 0.02, 5, dict(sto_long=0)),
    # k_sto_long<copper, LV 2>
    ("copper-T600-long", dict(n_gen=20, n_sto=4, T=600, seed=705), LH, ("mix", "mix", "K3"), "emax0", 0.02, 3, dict(sto_long=1)),
    ("copper-T2048-long-one-tile", dict(n_gen=8, n_sto=3, T=2048, seed=706), LH, ("inside", "eq", "K1"), "", 0.02, 2, dict(sto_long=1)),
    ("copper-T2049-long-tile-edge", dict(n_gen=8, n_sto=3, T=2049, seed=707), LH, ("mix", "cyclic", "K1"), "", 0.02, 2, dict(sto_long=1)),
    ("copper-T24-debug-long", CP, _capi.F_DEBUG_LONG_STO, ("mix", "mix", "K3"), "emax0", 0.02, 4, dict(sto_long=1)),
    # small networks (5 launches): k_net_agents<..., LV 2> / k_net_agents_av
    ("net-4x5-T24", dict(n_gen=60, n_sto=12, T=24, seed=708, **NET), 0, ("mix", "mix", "K3"), "emax0", 0.03, 8, dict(wide_net=0)),
    # k_sto_warm<..., lines, LV 2> beside the generator launch (overlap on a side stream)
    ("net-4x5-overlap", dict(n_gen=60, n_sto=12, T=24, seed=709, **NET), _capi.F_OVERLAP_AGENTS, ("inside", "cyclic", "KG"), "pmax0", 0.03, 6, dict(agents_fused=0)),
    # k_sto_update<..., lines, LV 2>
    ("net-4x5-T250-scan", dict(n_gen=20, n_sto=6, T=250, seed=710, **NET), 0, ("mix", "mix", "K3"), "", 0.03, 3, dict(sto_long=0)),
    # k_sto_long<lines, LV 2>
    ("net-4x5-T600-long", dict(n_gen=20, n_sto=4, T=600, seed=711, **NET), LH, ("mix", "edge", "K1"), "", 0.03, 2, dict(sto_long=1)),
    # 30 nodes / 45 lines x 96: k_net_agents<..., LV 2> + the quiet / slack chains; lines get flagged in the first iterations
    ("net-30x45-T96", dict(n_gen=120, n_sto=24, T=96, seed=41, **NET30), 0, ("mix", "mix", "K3"), "emax0", 0.01, 5, dict(agents_fused=1, wide_net=0)),
    ("net-30x45-no-quiet", dict(n_gen=120, n_sto=24, T=96, seed=41, **NET30), _capi.F_NO_QUIET, ("inside", "eq", "KG"), "", 0.01, 4, dict(quiet=0)),
    ("net-30x45-small-items", dict(n_gen=120, n_sto=24, T=96, seed=41, **NET30), _capi.F_NET_SMALL_ITEMS, ("mix", "cyclic", "K3"), "pmax0", 0.01, 4, dict(wide_net=0)),
    ("net-30x45-overlap", dict(n_gen=120, n_sto=24, T=96, seed=41, **NET30), _capi.F_OVERLAP_AGENTS, ("full", "edge-lo", "K3"), "", 0.01, 4, dict(agents_fused=0)),
    # the wide chain with k_net_agents / k_sto_warm at LV 2
    ("net-30x45-debug-wide", dict(n_gen=120, n_sto=24, T=96, seed=41, **NET30), _capi.F_DEBUG_WIDE_NET, ("mix", "mix", "K3"), "emax0", 0.01, 4, dict(wide_net=1)),
    # generators alone: k_gen_update_pair_skip<MODE, AV> / the generator launch without storages
    ("copper-generators-only", dict(n_gen=400, n_sto=0, T=24, seed=712), 0, (None, None, "KG"), "", 0.02, 5, dict()),
    # the lean copper body (no level flag): k_agents_l<..., AV>
    ("copper-lean-av", CP, 0, (None, None, "K3"), "", 0.02, 6, dict(agents_fused=1, sto_lean=1)),
    ("copper-lean-no-tail-fuse-av", CP, _capi.F_NO_TAIL_FUSE, (None, None, "K3"), "", 0.02, 5, dict(sto_lean=1)),
]


@pytest.mark.parametrize("name,case,extra,feat,degen,gamma,iters,expect", ONE, ids=[r[0] for r in ONE])
def test_one_step_parity_with_features(hip_api, fapi, name, case, extra, feat, degen, gamma, iters, expect):
    pp = degenerate(synth.synthetic_case(**case), degen)
    feats = Features(pp, *feat, seed=case["seed"])
    h = engine(hip_api, pp, None, flags=feats.flags | extra, eps=0.0, gamma=gamma)
    o = engine(fapi, pp, 1, flags=feats.flags, eps=0.0, gamma=gamma)
    from oracle.binding import set_threads
    set_threads(o, 8)
    for e in (h, o):
        feats.apply(e)
    tol = 1e-9 if pp.L == 0 else 1e-8
    worst = one_step(h, o, iters, tol, expect)
    print(f"{name}: worst one-step difference {worst:.2e} (scaled)")


LITERAL = [("copper-T8", dict(n_gen=20, n_sto=8, T=8, seed=721), 0, ("mix", "mix", "K3"), "emax0", 0.05),
           ("net-4x5-T5", dict(n_gen=12, n_sto=4, T=5, seed=722, **NET), 0, ("inside", "eq", "KG"), "", 0.1)]


@pytest.mark.parametrize("name,case,extra,feat,degen,gamma", LITERAL, ids=[r[0] for r in LITERAL])
def test_one_step_parity_against_the_literal_mode(hip_api, fapi, name, case, extra, feat, degen, gamma):
    pp = degenerate(synth.synthetic_case(**case), degen)
    feats = Features(pp, *feat, seed=case["seed"])
    h = engine(hip_api, pp, None, flags=feats.flags | extra, eps=0.0, gamma=gamma)
    o = engine(fapi, pp, 0, flags=feats.flags, eps=0.0, gamma=gamma)
    for e in (h, o):
        feats.apply(e)
    print(f"{name}: worst {one_step(h, o, 6, 1e-6):.2e}")


# ---- the setters between iterate(n) calls: graphs of 16, 4 and 1 iterations replayed with the new values --------------------

@pytest.mark.parametrize("case,extra", [(dict(n_gen=100, n_sto=10, T=24, seed=731), 0),
                                        (dict(n_gen=60, n_sto=12, T=24, seed=732, **NET), 0)], ids=["copper", "net-4x5"])
def test_setters_between_graph_replays(hip_api, fapi, case, extra):
    pp = synth.synthetic_case(**case)
    A = pp.G + pp.S
    kw = dict(eps=0.0, gamma=1.0 / A) if pp.L == 0 else dict(eps=0.0, gamma=1.0 / A, w_flow=0.3 / A)
    h = engine(hip_api, pp, None, flags=ALL | extra, **kw)
    o = engine(fapi, pp, 1, flags=ALL, **kw)
    rng = np.random.default_rng(case["seed"])
    tol = 1e-8 if pp.L == 0 else 1e-7
    worst = 0.0
    e0 = np.zeros(pp.S)
    for step, n in enumerate((1, 4, 16, 37, 1, 16, 4, 37)):
        what = ("e0", "band", "profiles")[step % 3]
        for e in (h, o):
            if what == "e0":                    # a new e0 under the default band, then a band reachable from it
                e0 = draw_e0(pp, ("mix", "inside", "full")[(step // 3) % 3], rng) if e is h else e0
                e.set_terminal_levels()
                e.set_initial_levels(e0)
            elif what == "band":
                band = draw_band(pp, e0, ("mix", "eq", "cyclic")[(step // 3) % 3], rng) if e is h else band
                e.set_terminal_levels(*band)
            else:                               # step 5: a larger table (K = G), so the graphs are captured again
                prof = draw_profiles(pp, "KG" if step == 5 else "K3", rng) if e is h else prof
                e.set_availability(*prof)
        h.iterate(n)
        o.iterate(n)
        w, where, cost = compare(state_of(h), state_of(o), tol)
        assert w <= tol, (step, n, where, w)
        worst = max(worst, w)
    assert h.solver_failures() == 0
    print(f"setters between replays: worst {worst:.2e}")


# ---- free runs ----------------------------------------------------------------------------------------------------------------

def test_free_running_copper_plate_with_every_feature(hip_api, fapi):
    pp = synth.synthetic_case(100, 10, 24, seed=741)
    g = 1.0 / (pp.G + pp.S)
    feats = Features(pp, "mix", "mix", "K3", seed=742)
    h = engine(hip_api, pp, None, flags=ALL, eps=0.0, gamma=g)
    o = engine(fapi, pp, 1, flags=ALL, eps=0.0, gamma=g)
    for e in (h, o):
        feats.apply(e)
    h.iterate(200)
    o.iterate(200)
    w = max_diff(state_of(h), state_of(o), keys=["P", "D", "C", "E", "lam", "inj"])[0]
    print(f"free run copper: {w:.2e}")
    assert w < 1e-8


def test_free_running_network_with_every_feature(hip_api, fapi):
    pp = synth.synthetic_case(120, 24, 96, N=30, L=45, seed=43, fmax_factor=0.8, fmax_min=10)
    A = pp.G + pp.S
    kw = dict(eps=0.0, gamma=1.0 / A, w_flow=0.3 / A)
    feats = Features(pp, "mix", "mix", "K3", seed=744)
    h = engine(hip_api, pp, None, flags=ALL, **kw)
    o = engine(fapi, pp, 1, flags=ALL, **kw)
    for e in (h, o):
        feats.apply(e)
    from oracle.binding import set_threads
    set_threads(o, 8)
    assert h.iterate_timed(1)["agents_fused"] == 1
    o.iterate(1)
    for n in (1, 3, 10, 15):
        h.iterate(n)
        o.iterate(n)
        w, where, _ = compare(state_of(h), state_of(o), 1e-7)
        assert w <= 1e-7, (n, where, w)
    assert h.solver_failures() == 0


# ---- negative controls: HIP with a feature against the oracle without it fails the tolerance ---------------------------------

@pytest.mark.parametrize("what", ["e0", "band", "profiles"])
def test_negative_controls(hip_api, fapi, what):
    pp = synth.synthetic_case(**CP)
    feats = Features(pp, "inside" if what == "e0" else None, "eq" if what == "band" else None,
                     "K3" if what == "profiles" else None, seed=751)
    h = engine(hip_api, pp, None, flags=feats.flags, eps=0.0, gamma=0.02)
    feats.apply(h)
    o = engine(fapi, pp, 1, flags=feats.flags, eps=0.0, gamma=0.02)       # the flag, but the defaults
    with pytest.raises(AssertionError):
        one_step(h, o, 4, 1e-9)
