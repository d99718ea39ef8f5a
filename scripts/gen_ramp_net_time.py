"""Per-iteration time with generator ramp limits on a network (DOPF_F_GEN_RAMP | DOPF_F_GEN_RAMP_NETWORK; bench.py cannot
set them): one workload shape, the settings below in ONE process, each timed as the device-side span of a settled dopf_iterate call
(DOPF_F_TIME_CALLS):
  (i)   no flag, DOPF_F_NO_FUSE — the flagless problem on the launches a context with the flags runs;
  (ii)  the flags with every ramp +inf: k_gen_ramp_net's fast path alone;
  (iii) the flags with ramps of 10 % of pmax per step, up and down; with it the share of rows that the last timed iteration repaired
        (formed on the host: from the state before it, one more iteration of (iii) and one of a flagless context from the same state —
        a row whose values differ left the fast path) and the context's solver failures (rows beyond the knot capacity).
(ii) against (i) is the cost of the feature's kernel on rows that need no repair, (iii) against (ii) the repairs'. No threshold is fixed
in advance.
usage: python scripts/gen_ramp_net_time.py [workload: config3-share] [rounds]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

import dopf_pkg  # noqa: E402
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth  # noqa: E402
import bench  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "config3-share"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
settle, timed = 200, 200
pp = bench.make_problem(synth, wl)
assert pp.L > 0, "a workload with lines (copper plates: scripts/gen_ramp_time.py)"
A = pp.G + pp.S
NET = _capi.F_GEN_RAMP | _capi.F_GEN_RAMP_NETWORK
runs = {"(i) flagless, DOPF_F_NO_FUSE": (_capi.F_NO_FUSE, None), "(ii) ramps +inf": (NET, None),
        "(iii) ramps 10 % of pmax": (NET, 0.1 * pp.gen_pmax)}
api = _capi.hip_api()


def engine(flags, ramp):
    e = _capi.Engine(api, params=_capi.default_params(gamma=1.0 / A, w_flow=0.3 / A, eps=0.0, flags=flags | _capi.F_TIME_CALLS),
                     **pp.engine_kwargs())
    if ramp is not None:
        e.set_ramp(ramp, ramp)
    return e


def state(e):
    P, D, C, _ = e.get_primal()
    lam, mu, rho = e.get_duals()
    _, aU, aK, _, _ = e.get_consensus()
    return dict(P=P, D=D, C_=C, avg_U=aU, avg_K=aK, lam=lam, mu=mu, rho=rho, iteration=e.get_residuals()[3])


def iterate(e, n):
    """dopf_iterate; a DOPF_E_SOLVER (rows beyond the knot capacity kept their clamped step) is reported once and counted below"""
    try:
        e.iterate(n)
    except _capi.DopfError as err:
        if not e.solver_failures():
            raise
        print(f"  ({err})")


res, share, fails = {}, [], []
for rnd in range(rounds):
    for name, (flags, ramp) in runs.items():
        e = engine(flags, ramp)
        iterate(e, settle)
        iterate(e, timed)
        res.setdefault(name, []).append(1000.0 * e.last_call_ms() / timed)
        if ramp is not None and rnd == 0:
            st = state(e)
            twin = engine(_capi.F_NO_FUSE, None)
            for x in (e, twin):
                x.set_state(**st)
                iterate(x, 1)
            share.append(float(np.mean(np.any(e.get_primal()[0] != twin.get_primal()[0], axis=1))))
            twin.close()
        if ramp is not None:
            fails.append(e.solver_failures())
        else:
            assert e.solver_failures() == 0
        e.close()
print(f"{wl}: G={pp.G} S={pp.S} T={pp.T} N={pp.N} L={pp.L}, median of {rounds} rounds [min..max], microseconds per iteration over {timed} "
      f"settled iterations")
base = sorted(res["(i) flagless, DOPF_F_NO_FUSE"])[rounds // 2]
for name, v in res.items():
    v = sorted(v)
    print(f"  {name:34s} {v[rounds // 2]:9.2f} us [{v[0]:.2f}..{v[-1]:.2f}] ({100.0 * (v[rounds // 2] / base - 1.0):+.1f} % of (i))")
print(f"  rows repaired in (iii): {100.0 * share[0]:.1f} % of {pp.G}; solver failures per run {fails}")
