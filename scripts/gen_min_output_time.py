"""Per-iteration time with must-run floors (dopf_set_generator_min_output; bench.py cannot set them): one workload shape
in a ramp context with the ramps of scripts/gen_ramp_time.py (10 % of pmax per step, up and down), each setting timed as the
device-side span of a settled dopf_iterate call (DOPF_F_TIME_CALLS):
  (a/b) DOPF_F_GEN_RAMP, the floor setter never called — k_gen_ramp<AV, QC, false>. Run with a library of the commit before (third
        argument) this is (a), that commit's figure; with this commit's library it is (b), which runs the same instantiations and must
        lie inside (a)'s own min..max spread;
  (c)   every row's floor at 30 % of its capacity — k_gen_ramp<AV, QC, true>. Reported, not bounded. (A library without the entry
        reports the first line alone.)
usage: python scripts/gen_min_output_time.py <workload: config1 | config2> [rounds] [library: a libdopf_hip.so of another commit]"""
import os
import sys

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
runs = {"(a/b) ramps, no floor set": None}
if hasattr(api, "set_generator_min_output"):
    runs["(c) floors at 30 % of pmax"] = 0.3 * pp.gen_pmax
res = {}
for rnd in range(rounds):
    for name, floor in runs.items():
        e = _capi.Engine(api, params=_capi.default_params(gamma=1.0 / A, eps=0.0, flags=_capi.F_GEN_RAMP | _capi.F_TIME_CALLS),
                         **pp.engine_kwargs())
        e.set_ramp(ramp, ramp)
        if floor is not None:
            e.set_min_output(floor)
        e.iterate(200)                               # settle (warm starts)
        e.iterate(400)
        res.setdefault(name, []).append(1000.0 * e.last_call_ms() / 400)
        assert e.solver_failures() == 0
        if floor is not None:
            assert float((floor[:, None] - e.get_primal()[0]).max()) <= 1e-9 * float(pp.gen_pmax.max())
        e.close()
print(f"{wl}: G={pp.G} S={pp.S} T={pp.T}, library {api.path}, median of {rounds} rounds [min..max], microseconds per iteration")
for name, v in res.items():
    v = sorted(v)
    print(f"  {name:30s} {v[rounds // 2]:9.2f} us [{v[0]:.2f}..{v[-1]:.2f}]")
