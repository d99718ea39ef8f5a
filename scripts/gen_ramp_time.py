"""Per-iteration time with generator ramp limits (DOPF_F_GEN_RAMP; bench.py cannot set them): one workload shape, the
settings below in ONE process, each timed as the device-side span of a settled dopf_iterate call (DOPF_F_TIME_CALLS):
  (a) no flag, DOPF_F_NO_FUSE | DOPF_F_NO_TAIL_FUSE — the flagless problem on the launches a context with the flag runs (on an even
      T its generators still run in the pair kernels; run on the parent commit this is the parent's figure);
  (b) DOPF_F_GEN_RAMP with every ramp +inf: the fast path alone;
  (c) DOPF_F_GEN_RAMP with ramps of 10 % of pmax per step, up and down; with it the share of rows whose clamped step breaks a ramp
      in the iteration behind the timed ones (formed on the host from the state: those rows left the fast path);
  (d) no flag at all — the default chain (fused launch, one-launch tail): (a) against (d) is what the chain costs.
(b) against (a) is the cost of the feature's kernel on rows that need no repair, (c) against (b) the repairs'. No threshold is fixed
in advance.
usage: python scripts/gen_ramp_time.py <workload: config1 | config2> [rounds]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

import dopf_pkg  # noqa: E402
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth  # noqa: E402
import bench  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "config1"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
pp = bench.make_problem(synth, wl)
A = pp.G + pp.S
APART = _capi.F_NO_FUSE | _capi.F_NO_TAIL_FUSE
RAMP = getattr(_capi, "F_GEN_RAMP", 0)
runs = {"(a) flagless, launches apart": (APART, None), "(d) flagless, default chain": (0, None)}
if RAMP:      # (the parent commit has no such flag: there the script reports (a) and (d) alone)
    runs["(b) ramps +inf"] = (RAMP, None)
    runs["(c) ramps 10 % of pmax"] = (RAMP, 0.1 * pp.gen_pmax)


def left_fast_path(e, ramp):
    """share of the generators whose clamped step from the engine's state breaks a ramp (copper plate, no c2, no availability)"""
    gamma = 1.0 / A
    P = e.get_primal()[0]
    lam = e.get_duals()[0]
    s = e.get_consensus()[0].sum(axis=0)
    c = P - (pp.gen_mc[:, None] + lam[None, :] + gamma * s[None, :]) / (1.0 + gamma)
    d = np.abs(np.diff(np.clip(c, 0.0, pp.gen_pmax[:, None]), axis=1))
    return float(np.mean(d.max(axis=1) > ramp))


api = _capi.hip_api()
res, share = {}, []
for rnd in range(rounds):
    for name, (flags, ramp) in runs.items():
        e = _capi.Engine(api, params=_capi.default_params(gamma=1.0 / A, eps=0.0, flags=flags | _capi.F_TIME_CALLS), **pp.engine_kwargs())
        if ramp is not None:
            e.set_ramp(ramp, ramp)
        e.iterate(200)                               # settle (row summaries, warm starts)
        e.iterate(400)
        res.setdefault(name, []).append(1000.0 * e.last_call_ms() / 400)
        if ramp is not None:
            share.append(left_fast_path(e, ramp))
        assert e.solver_failures() == 0
        e.close()
print(f"{wl}: G={pp.G} S={pp.S} T={pp.T}, median of {rounds} rounds [min..max], microseconds per iteration")
base = sorted(res["(a) flagless, launches apart"])[rounds // 2]
for name, v in res.items():
    v = sorted(v)
    print(f"  {name:34s} {v[rounds // 2]:9.2f} us [{v[0]:.2f}..{v[-1]:.2f}] ({100.0 * (v[rounds // 2] / base - 1.0):+.1f} % of (a))")
if share:
    print(f"  rows that left the fast path in (c): {100.0 * float(np.median(share)):.1f} % of {pp.G}")
