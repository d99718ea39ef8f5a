"""Storage efficiencies and line ratings (DOPF_F_STO_EFFICIENCY, DOPF_F_LINE_RATING) beside initial levels, terminal bands and
availability, against the oracle's exact mode with the same inputs: fuzz_levels.py with the case drawn through helpers.LossyRated
in place of helpers.Features. Random shapes (fuzz_levels' ranges: T = 1, 2, 250 and 600 with DOPF_F_LONG_HORIZON, storage shapes
varied, storages with emax = 0 or pmax = 0), a random non-empty subset of the five inputs e0, band, profiles, eta, table (the table
only where the case has lines; on some cases with an entry of exactly 0), one chain flag; one-step comparisons (HIP restarted from
the oracle's state) mixed with short free runs of iterate(n), and a few setter calls mid-run, the same draw on both sides.
usage: python scripts/fuzz_lossy_rated.py [n_cases] [seed]"""
import sys, os, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np, dopf_pkg
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth
from helpers import LossyRated, degenerate, engine, max_diff, set_from, state_of
import __graft_entry__ as ge
hip = _capi.CApi(os.environ["DOPF_LIB"], "dopf_") if os.environ.get("DOPF_LIB") else _capi.hip_api()
from oracle.binding import OracleApi, set_threads
ora = OracleApi(ge.ORACLE_LIB, features=True)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
CHAIN = {"copper": [0, _capi.F_NO_FUSE, _capi.F_NO_WARM_START, _capi.F_DEBUG_LEAVE, _capi.F_DEBUG_LONG_STO, _capi.F_NO_TAIL_FUSE],
         "net": [0, _capi.F_NO_QUIET, _capi.F_NET_SMALL_ITEMS, _capi.F_OVERLAP_AGENTS, _capi.F_DEBUG_WIDE_NET]}
worst, bad = 0.0, 0
t0 = time.time()
for k in range(n_cases):
    T = int(rng.choice([1, 2, 3, 5, 8, 12, 24, 24, 31, 48, 96, 250, 600]))
    net = rng.random() < 0.5
    G, S = int(rng.integers(2, 60)), int(rng.integers(1, 16))
    case = dict(n_gen=G, n_sto=S, T=T, seed=int(rng.integers(1, 10**6)))
    if net:
        N = int(rng.integers(2, 12))
        case.update(N=N, L=int(rng.integers(N - 1, min(2 * N + 1, N * (N - 1) // 2) + 1)), fmax_factor=float(rng.uniform(0.5, 1.0)), fmax_min=1.0)
    elif rng.random() < 0.2:
        case.update(N=int(rng.integers(2, 6)))                  # several nodes without lines
    pp = synth.synthetic_case(**case)
    if rng.random() < 0.6:                                      # storage shapes: not only emax = 2 pmax
        pp.sto_emax = pp.sto_pmax * rng.choice([0.7, 1.0, 2.0, 3.3, 5.0], size=S)
    if rng.random() < 0.3:
        pp.sto_pmax = pp.sto_pmax * rng.uniform(0.6, 1.4, size=S)
    pp = degenerate(pp, str(rng.choice(["", "", "emax0", "pmax0", "emax0+pmax0"])))
    pick = lambda *opts: str(rng.choice(opts))
    feats = lambda seed: LossyRated(pp, pick("0", "full", "inside", "mix") if use[0] else None,
                                    pick("default", "eq", "cyclic", "mix") if use[1] else None,      # (helpers_efficiency.draw_band_eff's kinds)
                                    pick("K1", "K3", "KG") if use[2] and pp.G > 0 else None, seed,
                                    eta=use[3], table=use[4], zero=zero)
    use = [False] * 5
    while not any(use):
        use = [bool(x) for x in rng.random(5) < 0.5]
        use[4] = use[4] and pp.L > 0                            # the table applies only where the case has lines
    zero = bool(rng.random() < 0.25)
    f = feats(int(rng.integers(1, 10**6)))
    extra = int(rng.choice(CHAIN["net" if pp.L else "copper"]))
    if T > 512:
        extra |= _capi.F_LONG_HORIZON
    A = pp.G + pp.S
    params = dict(gamma=float(rng.choice([1.0, 0.3, 2.0])) / A, w_flow=float(rng.choice([10.0, 0.3 / A])) if pp.L else 10.0)
    try:
        h = engine(hip, pp, None, flags=f.flags | extra, eps=0.0, **params)
        o = engine(ora, pp, 1, flags=f.flags, eps=0.0, **params)
    except _capi.DopfError as err:             # a shape no chain takes (e.g. an odd T with the long body's flag): not a finding
        print("skip", case, err, flush=True)
        continue
    set_threads(o, 8)
    f.apply(h); f.apply(o)
    w_case, it, iters = 0.0, 0, int(rng.integers(6, 30))
    while it < iters:
        if rng.random() < 0.15:                # setters mid-run, the same draw on both
            g = feats(int(rng.integers(1, 10**6)))
            if g.flags == f.flags:
                g.apply(h); g.apply(o)
        one = rng.random() < 0.5
        n = 1 if one else int(rng.choice([1, 4, 5, 16, 17]))
        h.iterate(n); o.iterate(n)
        it += n
        sh, so = state_of(h), state_of(o)
        scale = max(1.0, float(np.abs(so["lam"]).max()))
        w, where = max_diff(sh, so, keys=["P", "D", "C", "E", "lam", "mu", "rho", "inj"])
        tol = (1e-9 if one else 1e-7) * scale * (10 if pp.L else 1)
        w_case = max(w_case, w / scale)
        if w > tol:
            bad += 1
            print("MISMATCH", case, params, "flags", f.flags | extra, "features", use, "zero", zero, "iteration", it, "step", n, where, w, flush=True)
            break
        if one:
            set_from(h, so, o.get_residuals()[3])
    if h.solver_failures():
        bad += 1
        print("SOLVER FAILURES", case, params, h.solver_failures(), flush=True)
    worst = max(worst, w_case)
    h.close(); o.close()
    if k % 10 == 9:
        print(f"{k+1} cases, worst relative difference {worst:.2e}, bad {bad}, {time.time()-t0:.0f}s", flush=True)
print(f"done: {n_cases} cases, worst relative difference {worst:.2e}, bad {bad}")
