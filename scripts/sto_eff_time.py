"""Per-iteration time with storage efficiencies (DOPF_F_STO_EFFICIENCY; bench.py cannot set them): one workload
shape, three settings in ONE process, each timed as the device-side span of a settled dopf_iterate call (DOPF_F_TIME_CALLS):
  (a) DOPF_F_STO_INITIAL_LEVEL | DOPF_F_STO_TERMINAL_LEVEL — the general body at level mode 2, the baseline (run on the parent
      commit this is the parent's figure: those instantiations are untouched);
  (b) DOPF_F_STO_EFFICIENCY with all efficiencies 1;
  (c) DOPF_F_STO_EFFICIENCY with eta_c = eta_d = 0.9.
All three run the same chain; (a2) times (a) with DOPF_F_NO_FUSE | DOPF_F_NO_TAIL_FUSE and (b2) (b) likewise: the storage
launch of its own.
usage: python scripts/sto_eff_time.py <workload: config2 | config4> [rounds]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

import dopf_pkg  # noqa: E402
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth  # noqa: E402
import bench  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "config2"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
pp = bench.make_problem(synth, wl)
A, S = pp.G + pp.S, pp.S
LV2 = _capi.F_STO_INITIAL_LEVEL | _capi.F_STO_TERMINAL_LEVEL
EF = getattr(_capi, "F_STO_EFFICIENCY", 0)
runs = {"(a) levels + band": (LV2, None),
        "(a2) (a), launches apart": (LV2 | _capi.F_NO_FUSE | _capi.F_NO_TAIL_FUSE, None)}
if EF:      # (the parent commit has no such flag: there the script reports (a) alone)
    runs["(b) efficiency, eta = 1"] = (EF, None)
    runs["(c) efficiency, eta = 0.9"] = (EF, 0.9)
    runs["(b2) (b), launches apart"] = (EF | _capi.F_NO_FUSE | _capi.F_NO_TAIL_FUSE, None)
api = _capi.hip_api()
res = {}
for rnd in range(rounds):
    for name, (flags, eta) in runs.items():
        e = _capi.Engine(api, params=_capi.default_params(gamma=1.0 / A, eps=0.0, flags=flags | _capi.F_TIME_CALLS), **pp.engine_kwargs())
        if eta is not None:
            e.set_efficiency(np.full(S, eta), np.full(S, eta))
        e.iterate(200)                               # settle (row summaries, warm starts)
        e.iterate(400)
        res.setdefault(name, []).append(e.last_call_ms() / 400)
        assert e.solver_failures() == 0
        e.close()
print(f"{wl}: G={pp.G} S={S} T={pp.T}, median of {rounds} rounds [min..max], ms per iteration")
base = sorted(res["(a) levels + band"])[rounds // 2]
for name, v in res.items():
    v = sorted(v)
    print(f"  {name:28s} {v[rounds // 2]:9.5f} ms [{v[0]:.5f}..{v[-1]:.5f}] ({100.0 * (v[rounds // 2] / base - 1.0):+.1f} % of (a))")
