"""Per-iteration time with quadratic generator costs (DOPF_F_GEN_QUADRATIC_COST; bench.py cannot set them): one
workload shape, the settings below in ONE process, each timed as the device-side span of a settled dopf_iterate call
(DOPF_F_TIME_CALLS):
  (a) no flag, DOPF_F_NO_FUSE | DOPF_F_NO_TAIL_FUSE — the flagless problem on the launches a context with the flag runs (on an even
      T its generators still run in the pair kernels; run on the parent commit this is the parent's figure);
  (b) DOPF_F_GEN_QUADRATIC_COST with every c2 = 0;
  (c) DOPF_F_GEN_QUADRATIC_COST with c2 uniform in [0.01, 0.1];
  (d) no flag at all — the default chain (fused launch, one-launch tail): (a) against (d) is what the chain costs.
(b) against (a) is the cost of the feature's kernel. No threshold is fixed in advance.
usage: python scripts/gen_quadratic_time.py <workload: config1 | config2> [rounds]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

import dopf_pkg  # noqa: E402
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth  # noqa: E402
import bench  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "config1"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
pp = bench.make_problem(synth, wl)
A = pp.G + pp.S
APART = _capi.F_NO_FUSE | _capi.F_NO_TAIL_FUSE
QC = getattr(_capi, "F_GEN_QUADRATIC_COST", 0)
runs = {"(a) flagless, launches apart": (APART, None), "(d) flagless, default chain": (0, None)}
if QC:      # (the parent commit has no such flag: there the script reports (a) and (d) alone)
    runs["(b) quadratic, c2 = 0"] = (QC, None)
    runs["(c) quadratic, c2 in [0.01, 0.1]"] = (QC, np.random.default_rng(1).uniform(0.01, 0.1, pp.G))
api = _capi.hip_api()
res = {}
for rnd in range(rounds):
    for name, (flags, c2) in runs.items():
        e = _capi.Engine(api, params=_capi.default_params(gamma=1.0 / A, eps=0.0, flags=flags | _capi.F_TIME_CALLS), **pp.engine_kwargs())
        if c2 is not None:
            e.set_quadratic_cost(c2)
        e.iterate(200)                               # settle (row summaries, warm starts)
        e.iterate(400)
        res.setdefault(name, []).append(1000.0 * e.last_call_ms() / 400)
        assert e.solver_failures() == 0
        e.close()
print(f"{wl}: G={pp.G} S={pp.S} T={pp.T}, median of {rounds} rounds [min..max], microseconds per iteration")
base = sorted(res["(a) flagless, launches apart"])[rounds // 2]
for name, v in res.items():
    v = sorted(v)
    print(f"  {name:34s} {v[rounds // 2]:9.2f} us [{v[0]:.2f}..{v[-1]:.2f}] ({100.0 * (v[rounds // 2] / base - 1.0):+.1f} % of (a))")
