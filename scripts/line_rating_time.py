"""Per-iteration time with line ratings (DOPF_F_LINE_RATING; bench.py cannot set them): one network workload, the
settings in ONE process, each timed as the device-side span of a settled dopf_iterate call (DOPF_F_TIME_CALLS):
  (b) no flag — the L limits of dopf_create, read through the leading dimension 0;
  (c) DOPF_F_LINE_RATING with a table whose columns all equal f_max (the same iterates, bit for bit; L*T doubles more to read).
Run on the parent commit the script reports (b) alone, and that figure is (a), the yardstick for both: the parent has no flag and
no leading dimension. (b2) / (c2): the same with DOPF_F_NO_QUIET, the chain with k_slack in every iteration.
usage: python scripts/line_rating_time.py [workload: config3-share | config3] [rounds]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

import dopf_pkg  # noqa: E402
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth  # noqa: E402
import bench  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "config3-share"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
pp = bench.make_problem(synth, wl)
A = pp.G + pp.S
LR = getattr(_capi, "F_LINE_RATING", 0)
runs = {"(b) no flag": 0, "(b2) (b), no quiet chain": _capi.F_NO_QUIET}
if LR:      # (the parent commit has no such flag: there the script reports the flagless figures alone — (a))
    runs["(c) rating table = f_max"] = LR
    runs["(c2) (c), no quiet chain"] = LR | _capi.F_NO_QUIET
api = _capi.hip_api()
res = {}
for rnd in range(rounds):
    for name, flags in runs.items():
        e = _capi.Engine(api, params=_capi.default_params(gamma=1.0 / A, w_flow=0.3 / A, eps=0.0, flags=flags | _capi.F_TIME_CALLS),
                         **pp.engine_kwargs())
        if flags & LR:
            e.set_line_rating(np.repeat(np.asarray(pp.f_max, dtype=np.float64)[:, None], pp.T, axis=1))
        e.iterate(200)                               # settle (row summaries, warm starts, the flags of the slack sums)
        e.iterate(400)
        res.setdefault(name, []).append(1000.0 * e.last_call_ms() / 400)
        assert e.solver_failures() == 0
        e.close()
print(f"{wl}: N={pp.N} L={pp.L} G={pp.G} S={pp.S} T={pp.T}, median of {rounds} rounds [min..max], us per iteration")
base = sorted(res["(b) no flag"])[rounds // 2]
for name, v in res.items():
    v = sorted(v)
    print(f"  {name:28s} {v[rounds // 2]:9.3f} us [{v[0]:.3f}..{v[-1]:.3f}] ({100.0 * (v[rounds // 2] / base - 1.0):+.1f} % of (b))")
