"""Per-iteration time with the ramp prices recorded (dopf_get_generator_ramp_price; bench.py cannot ask for them): one
workload shape in a ramp context and in the pair's context (DOPF_F2_GEN_RAMP_BUDGET, default budgets) with the ramps of
scripts/gen_ramp_time.py (10 % of pmax per step, up and down), each setting timed as the device-side span of a settled dopf_iterate
call (DOPF_F_TIME_CALLS):
  (a/b) the entry never called — k_gen_ramp<AV, QC, MN, false> / k_gen_ramp_budget<AV, QC, false>. Run with a library of the commit
        before (third argument) this is (a), that commit's figure; with this commit's library it is (b), which launches the same code
        and must lie inside (a)'s own min..max spread;
  (c)   the entry called once before the first iteration — the RP = true instantiations: zeros for the rows that keep their ramps, the
        pass of csrc/ramp_price.h behind every repair. Reported, not bounded. (A library without the entry reports the first lines alone.)
usage: python scripts/gen_ramp_price_time.py <workload: config1 | config2> [rounds] [library: a libdopf_hip.so of another commit]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import dopf_pkg  # noqa: E402
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth  # noqa: E402
import bench  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "config2"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
if len(sys.argv) > 3:
    _capi._pin_hip_runtime()
    api = _capi.CApi(sys.argv[3], "dopf_")
else:
    api = _capi.hip_api()
pp = bench.make_problem(synth, wl)
A = pp.G + pp.S
ramp = 0.1 * pp.gen_pmax
PAIR2 = _capi.F2_GEN_ENERGY_BUDGET | _capi.F2_GEN_RAMP_BUDGET
runs = {"(a/b) ramps, entry never called": (0, False), "(a/b) the pair, entry never called": (PAIR2, False)}
if hasattr(api, "get_generator_ramp_price"):
    runs["(c) ramps, prices recorded"] = (0, True)
    runs["(c) the pair, prices recorded"] = (PAIR2, True)
res, priced = {}, {}
for rnd in range(rounds):
    for name, (flags2, record) in runs.items():
        e = _capi.Engine(api, params=_capi.default_params(gamma=1.0 / A, eps=0.0, flags=_capi.F_GEN_RAMP | _capi.F_TIME_CALLS),
                         flags2=flags2, **pp.engine_kwargs())
        e.set_ramp(ramp, ramp)
        if record:
            assert not np.any(e.ramp_price())
        e.iterate(200)                               # settle (warm starts)
        e.iterate(400)
        res.setdefault(name, []).append(1000.0 * e.last_call_ms() / 400)
        assert e.solver_failures() == 0
        if record:
            priced[name] = float(np.mean(np.any(e.ramp_price() != 0.0, axis=1)))
        e.close()
print(f"{wl}: G={pp.G} S={pp.S} T={pp.T}, library {api.path}, median of {rounds} rounds [min..max], microseconds per iteration")
for name, v in res.items():
    v = sorted(v)
    more = f"  ({100.0 * priced[name]:.1f} % of the rows priced in the last iteration)" if name in priced else ""
    print(f"  {name:36s} {v[rounds // 2]:9.2f} us [{v[0]:.2f}..{v[-1]:.2f}]{more}")
