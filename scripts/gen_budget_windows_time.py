"""Per-iteration time with energy budgets per sub-window (dopf_set_generator_energy_budget_windows; bench.py cannot set
them): one workload shape, the settings below in ONE process, each timed as the device-side span of a settled dopf_iterate call
(DOPF_F_TIME_CALLS: 200 iterations to settle, 400 timed):
  (a) whole-horizon budgets, every tenth row held to 60 % of the energy it delivers in the settled run without budgets: k_gen_budget,
      scripts/gen_budget_time.py's (c), the yardstick (the kernel of the commit before, which has no window entry);
  (b) the same budgets as one window with end T: k_gen_budget_win on k_gen_budget's work;
  (c) four windows of T / 4 steps, all free: the fast path alone, four units per row;
  (d) four windows, every tenth row held in every window to 60 % of the energy it delivers there in the settled run: four searches
      per held row, each over a quarter of the row.
No threshold is fixed in advance.
usage: python scripts/gen_budget_windows_time.py <workload: config1 | config2> [rounds]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

import dopf_pkg  # noqa: E402
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth  # noqa: E402
import bench  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "config2"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
pp = bench.make_problem(synth, wl)
A = pp.G + pp.S
BUDGET = _capi.F2_GEN_ENERGY_BUDGET
QUARTERS = [pp.T * (j + 1) // 4 for j in range(4)]
api = _capi.hip_api()
runs = {"(a) whole horizon, a tenth of the rows bind": "whole", "(b) the same budgets as one window": "one",
        "(c) four windows, all free": "free", "(d) four windows, a tenth of the rows bind": "four"}


def engine():
    return _capi.Engine(api, params=_capi.default_params(gamma=1.0 / A, eps=0.0, flags=_capi.F_TIME_CALLS), flags2=BUDGET, **pp.engine_kwargs())


e = engine()                                         # the settled run without budgets: the rows' energies, whole and per quarter
e.iterate(600)
P = e.get_primal()[0]
e.close()
cuts = [0] + QUARTERS
whole = np.full(pp.G, np.inf)
whole[::10] = 0.6 * P.sum(axis=1)[::10]
four = np.full((pp.G, 4), np.inf)
four[::10] = 0.6 * np.stack([P[::10, a:b].sum(axis=1) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)

res, fails = {}, 0
for rnd in range(rounds):
    for name, kind in runs.items():
        e = engine()
        if kind == "whole":
            e.set_energy_budget(None, whole)
        elif kind == "one":
            e.set_energy_budget_windows([pp.T], None, whole[:, None])
        else:
            e.set_energy_budget_windows(QUARTERS, None, four if kind == "four" else None)
        e.iterate(200)                               # settle (row summaries, warm starts)
        e.iterate(400)
        res.setdefault(name, []).append(1000.0 * e.last_call_ms() / 400)
        fails += e.solver_failures()
        e.close()
print(f"{wl}: G={pp.G} S={pp.S} T={pp.T}, windows end at {QUARTERS}, median of {rounds} rounds [min..max], microseconds per iteration")
base = sorted(res["(a) whole horizon, a tenth of the rows bind"])[rounds // 2]
for name, v in res.items():
    v = sorted(v)
    print(f"  {name:44s} {v[rounds // 2]:9.2f} us [{v[0]:.2f}..{v[-1]:.2f}] ({100.0 * (v[rounds // 2] / base - 1.0):+.1f} % of (a))")
print(f"  solver failures in all runs: {fails}")
