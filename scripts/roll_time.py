"""What a window change costs: dopf_roll_horizon against the host route the library offered before it — getters,
horizon.shift_window in NumPy, dopf_set_state and dopf_set_storage_initial_level on an existing context of the shifted demand
(creating that context is timed separately). Median wall time of each, host sync included, and the bytes the row kernel moves
(P, D, C read and written once: 16 B per element, plus the items' sums) against the time of a roll. The kernels' device time:
run this script under `rocprofv3 --kernel-trace --stats -- python scripts/roll_time.py <workload>` and read the k_roll_* rows.
usage: python scripts/roll_time.py <workload: config2 | config3-share> [k] [rounds]"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

import dopf_pkg  # noqa: E402
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, shift_window, synth  # noqa: E402
import bench  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "config2"
k = int(sys.argv[2]) if len(sys.argv) > 2 else 4
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
pp = bench.make_problem(synth, wl)
A, T = pp.G + pp.S, pp.T
kw = dict(gamma=1.0 / A, eps=0.0, flags=_capi.F_STO_INITIAL_LEVEL)
if pp.L:
    kw["w_flow"] = 0.3 / A
api = _capi.hip_api()
e = _capi.Engine(api, params=_capi.default_params(**kw), **pp.engine_kwargs())
e.iterate(200)
tail = pp.demand[:, :k].copy()
roll_ms, host_ms, create_ms = [], [], []
for r in range(rounds):
    # the host route first (it reads the state the roll then moves)
    t0 = time.perf_counter()
    P, D, C, E = e.get_primal()
    lam, mu, rho = e.get_duals()
    _, aU, aK, _, _ = e.get_consensus()
    w = shift_window(k, tail, demand=e.demand(), P=P, D=D, C=C, E=E, lam=lam, mu=mu, rho=rho, avg_U=aU, avg_K=aK, sto_emax=pp.sto_emax)
    t1 = time.perf_counter()
    kwargs = dict(pp.engine_kwargs(), demand=_capi._f64(w["demand"].T))
    other = _capi.Engine(api, params=_capi.default_params(**kw), **kwargs)
    t2 = time.perf_counter()
    other.set_initial_levels(w["e0"])
    other.set_state(P=w["P"], D=w["D"], C_=w["C"], avg_U=w["avg_U"], avg_K=w["avg_K"], lam=w["lam"], mu=w["mu"], rho=w["rho"], iteration=2)
    other.sync()
    t3 = time.perf_counter()
    other.close()
    host_ms.append(((t1 - t0) + (t3 - t2)) * 1e3)
    create_ms.append((t2 - t1) * 1e3)
    t0 = time.perf_counter()
    e.roll(k, tail)
    roll_ms.append((time.perf_counter() - t0) * 1e3)
    e.iterate(20)
med = lambda v: sorted(v)[len(v) // 2]
moved = 16.0 * (pp.G + 2 * pp.S) * T
print(f"{wl}: G={pp.G} S={pp.S} T={T} N={pp.N} L={pp.L}, k={k}, median of {rounds}")
print(f"  dopf_roll_horizon        {med(roll_ms):9.3f} ms [{min(roll_ms):.3f}..{max(roll_ms):.3f}] (host sync included)")
print(f"  host route               {med(host_ms):9.3f} ms [{min(host_ms):.3f}..{max(host_ms):.3f}] (getters + shift_window + set_initial_levels + set_state)")
print(f"  ... plus dopf_create     {med(create_ms):9.3f} ms")
print(f"  rows moved: {moved / 1e6:.1f} MB read + written; at the roll's whole wall time that is {moved / (med(roll_ms) * 1e-3) / 1e9:.1f} GB/s "
      f"(the k_roll_rows kernels' own time: rocprofv3 --kernel-trace --stats)")
