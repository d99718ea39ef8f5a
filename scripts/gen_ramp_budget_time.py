"""Per-iteration time with ramp limits and energy budgets on the same generators (DOPF_F2_GEN_RAMP_BUDGET; bench.py
cannot set them): one workload shape with the ramps of scripts/gen_ramp_time.py (10 % of pmax per step, up and down), the settings
below in ONE process, each timed as the device-side span of a settled dopf_iterate call (DOPF_F_TIME_CALLS):
  (a) DOPF_F_GEN_RAMP alone — k_gen_ramp, the figure of the commit before the pair (run there, the script reports (a) alone);
  (b) the three flags with every budget at its default: by the cascade every row takes k_gen_ramp's path, so (b) against (a) is what
      the new kernel's own shape costs — it must stay within the rounds' spread;
  (c) the three flags with every tenth row held to 70 % of the energy it delivers in (a)'s settled state; with it the share of rows
      whose ramp-only step breaks the budget is not formed on the host (it would need the ramp programme there): the solver failures
      are reported instead.
Also printed: the bytes of the pair search's scratch for the shape (dopf_internal.h: gen_ramp_budget_doubles).
usage: python scripts/gen_ramp_budget_time.py <workload: config1 | config2> [rounds]"""
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
RAMP = _capi.F_GEN_RAMP
BUDGET = _capi.F2_GEN_ENERGY_BUDGET
PAIR = getattr(_capi, "F2_GEN_RAMP_BUDGET", 0)
ramp = 0.1 * pp.gen_pmax
runs = {"(a) ramps alone (k_gen_ramp)": (0, False)}
if PAIR:      # (the commit before has no such flag: there the script reports (a) alone)
    runs["(b) the pair, default budgets"] = (BUDGET | PAIR, False)
    runs["(c) the pair, a tenth of the rows at 0.7"] = (BUDGET | PAIR, True)


def scratch_bytes():
    """plan_chain's generator items on a one-node plate (2048 wanted, whole tiles of 512 / min(T, 512) rows), 8 waves each, T centres
    and 64 x (5T + 4) work doubles per wave, behind the 6 G doubles of capacities, ramps, anchor and budgets (the G budget prices
    behind the scratch are not counted)"""
    R = 512 // min(pp.T, 512)
    chunk = -(-max(R, -(-pp.G // 2048)) // R) * R
    items = -(-pp.G // chunk)
    return 8 * (6 * pp.G + items * 8 * (pp.T + 64 * (5 * pp.T + 4))), items


api = _capi.hip_api()
res, energy, fails = {}, None, {}
for rnd in range(rounds):
    for name, (flags2, bind) in runs.items():
        kw = dict(flags2=flags2) if flags2 else {}
        e = _capi.Engine(api, params=_capi.default_params(gamma=1.0 / A, eps=0.0, flags=RAMP | _capi.F_TIME_CALLS), **kw, **pp.engine_kwargs())
        e.set_ramp(ramp, ramp)
        if bind:
            hi = np.full(pp.G, np.inf)
            hi[::10] = 0.7 * energy[::10]
            e.set_energy_budget(None, hi)
        try:
            e.iterate(200)                               # settle (row summaries, warm starts)
            e.iterate(400)
        except _capi.DopfError as err:                   # (DOPF_E_SOLVER: counted below; the time of the call stands)
            print(f"  {name}: {err}")
        res.setdefault(name, []).append(1000.0 * e.last_call_ms() / 400)
        if energy is None:
            energy = e.get_primal()[0].sum(axis=1)       # (a), first round: the rows' energies in the settled run under ramps
        fails[name] = fails.get(name, 0) + e.solver_failures()
        e.close()
print(f"{wl}: G={pp.G} S={pp.S} T={pp.T}, ramps 10 % of pmax, median of {rounds} rounds [min..max], microseconds per iteration")
base = sorted(res["(a) ramps alone (k_gen_ramp)"])[rounds // 2]
for name, v in res.items():
    v = sorted(v)
    print(f"  {name:42s} {v[rounds // 2]:9.2f} us [{v[0]:.2f}..{v[-1]:.2f}] ({100.0 * (v[rounds // 2] / base - 1.0):+.1f} % of (a)), "
          f"solver failures {fails[name]}")
if PAIR:
    b, items = scratch_bytes()
    print(f"  scratch of the pair search: {b} bytes ({b / 2 ** 30:.2f} GiB) for {items} generator items")
