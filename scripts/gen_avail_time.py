"""Per-iteration time with generator availability profiles (DOPF_F_GEN_AVAILABILITY; bench.py cannot set profiles): one workload
shape, four runs in ONE process — no flag, the flag without profiles, K = 3 shared profiles on every generator, and a dense profile
per generator (K = G) — each timed as the device-side span of a settled dopf_iterate call (DOPF_F_TIME_CALLS), plus the generator
kernel's time and achieved bandwidth from dopf_iterate_timed (eager launches; bytes: P read + written, 16 B per element, and with
K = G the profile read, 8 B more).
usage: python scripts/gen_avail_time.py <workload: config4 | config4x2 | config2> [rounds]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

import dopf_pkg  # noqa: E402
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth  # noqa: E402
import bench  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "config4"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
pp = bench.make_problem(synth, wl)
A, G, T = pp.G + pp.S, pp.G, pp.T
shapes = synth.availability_profiles(T)
rng = np.random.default_rng(7)
runs = {
    "no flag": (0, None),
    "flag, no profiles": (_capi.F_GEN_AVAILABILITY, None),
    "K=3 shared": (_capi.F_GEN_AVAILABILITY, (shapes, rng.integers(0, 3, size=G).astype(np.int32))),
    "K=G dense": (_capi.F_GEN_AVAILABILITY, (np.round(rng.uniform(0.3, 1.0, (G, T)) * 1024.0) / 1024.0, np.arange(G, dtype=np.int32))),
}
api = _capi.hip_api()
res = {}
for rnd in range(rounds):
    for name, (flags, prof) in runs.items():
        e = _capi.Engine(api, params=_capi.default_params(gamma=1.0 / A, eps=0.0, flags=flags | _capi.F_TIME_CALLS), **pp.engine_kwargs())
        if prof is not None:
            e.set_availability(*prof)
        e.iterate(200)                               # settle (row summaries, warm starts)
        e.iterate(400)
        it_us = e.last_call_ms() / 400 * 1e3
        tm = e.iterate_timed(50)
        gen_bytes = 16.0 * G * T + (8.0 * G * T if name == "K=G dense" else 0.0)
        res.setdefault(name, []).append((it_us, tm["gen_ms"] * 1e3, gen_bytes / (tm["gen_ms"] * 1e-3) / 1e9 if tm["gen_ms"] > 0 else 0.0))
        e.close()
print(f"{wl}: G={G} S={pp.S} T={T}, median of {rounds} rounds (us per iteration of the default chain; generator kernel of the eager chain)")
base = sorted(x[0] for x in res["no flag"])[rounds // 2]
for name, v in res.items():
    it = sorted(x[0] for x in v)
    gk = sorted(x[1] for x in v)
    bw = sorted(x[2] for x in v)
    print(f"  {name:18s} {it[rounds // 2]:8.2f} us [{it[0]:.2f}..{it[-1]:.2f}] ({100.0 * (it[rounds // 2] / base - 1.0):+.1f} %)   "
          f"generator kernel {gk[rounds // 2]:7.2f} us, {bw[rounds // 2]:6.0f} GB/s of the model's bytes")
