"""What a window change costs on a context with ramp limits or energy budgets: dopf_roll_horizon_coupled
(Engine.roll_coupled: the context, its scratch and its graphs stay) against Engine.roll's host route on the same kind of context —
getters, horizon.shift_window, a new context with every setter, dopf_set_state — which was the only route before. The host route's
time is split into the context's creation (dopf_create / dopf_create_ex) and the rest. Ramps of 10 % of gen_pmax; the ramp context
and, on a copper plate, the pair context (DOPF_F2_GEN_RAMP_BUDGET) with its budgets at their defaults; dopf_roll_horizon on the
flagless context of the same shape beside them. Median wall time of each, host sync included.
usage: python scripts/roll_coupled_time.py <workload: config2 | config3-share> [k] [rounds]"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

import dopf_pkg  # noqa: E402
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth  # noqa: E402
import bench  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "config2"
k = int(sys.argv[2]) if len(sys.argv) > 2 else 4
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
pp = bench.make_problem(synth, wl)
A, T = pp.G + pp.S, pp.T
kw = dict(gamma=1.0 / A, eps=0.0)
if pp.L:
    kw["w_flow"] = 0.3 / A
api = _capi.hip_api()
IL, RAMP, RAMP_NET = _capi.F_STO_INITIAL_LEVEL, _capi.F_GEN_RAMP, _capi.F_GEN_RAMP_NETWORK
BUDGET, PAIR = _capi.F2_GEN_ENERGY_BUDGET, _capi.F2_GEN_RAMP_BUDGET
tail = pp.demand[:, :k].copy()
med = lambda v: sorted(v)[len(v) // 2]

create_s = [0.0]


def timed(fn):
    def call(*args):
        t0 = time.perf_counter()
        rc = fn(*args)
        create_s[0] += time.perf_counter() - t0
        return rc
    return call


api._create, api.create_ex = timed(api._create), timed(api.create_ex)


def context(flags, flags2):
    e = _capi.Engine(api, params=_capi.default_params(flags=IL | flags, **kw), flags2=flags2, **pp.engine_kwargs())
    e.set_initial_levels(np.zeros(pp.S))
    if flags & RAMP:
        e.set_ramp(0.1 * pp.gen_pmax, 0.1 * pp.gen_pmax)
    e.iterate(200)
    return e


def line(name, v, note=""):
    print(f"  {name:34s}{med(v):9.3f} ms [{min(v):.3f}..{max(v):.3f}]{note}")


print(f"{wl}: G={pp.G} S={pp.S} T={T} N={pp.N} L={pp.L}, k={k}, median of {rounds}, host sync included")
plain = context(0, 0)
ms = []
for r in range(rounds):
    t0 = time.perf_counter()
    plain.roll(k, tail)
    ms.append((time.perf_counter() - t0) * 1e3)
    plain.iterate(20)
line("flagless: dopf_roll_horizon", ms)
plain.close()
kinds = [("ramp", RAMP | (RAMP_NET if pp.L else 0), 0)] + ([("ramp + budget", RAMP, BUDGET | PAIR)] if pp.L == 0 else [])
for name, flags, flags2 in kinds:
    native, host = context(flags, flags2), context(flags, flags2)
    roll_ms, host_ms, create_ms = [], [], []
    for r in range(rounds):
        t0 = time.perf_counter()
        native.roll_coupled(k, tail)
        roll_ms.append((time.perf_counter() - t0) * 1e3)
        create_s[0] = 0.0
        t0 = time.perf_counter()
        host.roll(k, tail)                  # (the host route on this API: the context is rebuilt)
        total = time.perf_counter() - t0
        host_ms.append((total - create_s[0]) * 1e3)
        create_ms.append(create_s[0] * 1e3)
        native.iterate(20)
        host.iterate(20)
    line(f"{name}: dopf_roll_horizon_coupled", roll_ms)
    line(f"{name}: host route, creation", create_ms)
    line(f"{name}: host route, the rest", host_ms, " (getters + shift_window + the setters + set_state)")
    native.close()
    host.close()
