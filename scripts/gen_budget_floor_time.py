"""Per-iteration time with must-run floors on a budget context (dopf_set_generator_budget_min_output; bench.py cannot
set them): one workload shape, the settings below in ONE process, each timed as the device-side span of a settled dopf_iterate call
(DOPF_F_TIME_CALLS: 200 iterations to settle, 400 timed):
  (a) whole-horizon budgets, every tenth row held to 60 % of the energy it delivers in the settled run without budgets, no floor
      call: the MN = false instantiations of k_gen_budget — scripts/gen_budget_time.py's (c), the yardstick against the commit before;
  (b) four windows of T / 4 steps, every tenth row held in every window to 60 % of the energy it delivers there, no floor call:
      scripts/gen_budget_windows_time.py's (d), the MN = false instantiations of k_gen_budget_win;
  (c) (a) with floors of 30 % of gen_pmax on every row: the MN instantiations of k_gen_budget;
  (d) (b) with the same floors: the MN instantiations of k_gen_budget_win.
In (c) and (d) a held row whose floors sum above its bound gets the floor sum plus 2 % as its bound (the setter would refuse it
otherwise); the count is printed. No threshold is fixed in advance.
With a third argument the library of another commit is loaded in this one's place (the commit before has no floor entry: (c) and (d)
are left out), so that the two can be run in turn in one session.
usage: python scripts/gen_budget_floor_time.py <workload: config1 | config2> [rounds] [library]"""
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
lib = sys.argv[3] if len(sys.argv) > 3 else None
pp = bench.make_problem(synth, wl)
A = pp.G + pp.S
BUDGET = _capi.F2_GEN_ENERGY_BUDGET
QUARTERS = [pp.T * (j + 1) // 4 for j in range(4)]
api = _capi.hip_api() if lib is None else _capi.CApi(lib, "dopf_")
has_floors = hasattr(api, "set_generator_budget_min_output")
runs = {"(a) whole horizon, a tenth of the rows bind, no floor call": ("whole", False),
        "(b) four windows, a tenth of the rows bind, no floor call": ("four", False)}
if has_floors:
    runs.update({"(c) (a) with floors of 30 % of gen_pmax": ("whole", True), "(d) (b) with floors of 30 % of gen_pmax": ("four", True)})


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
p_min = 0.3 * np.asarray(pp.gen_pmax, dtype=np.float64)
need_whole = 1.02 * pp.T * p_min
need_four = 1.02 * np.stack([(b - a) * p_min for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
whole_f = np.where(np.isfinite(whole), np.maximum(whole, need_whole), np.inf)
four_f = np.where(np.isfinite(four), np.maximum(four, need_four), np.inf)
raised = (int(np.sum(whole_f != whole)), int(np.sum(four_f != four)))

res, fails, on_floor = {}, 0, {}
for rnd in range(rounds):
    for name, (kind, floors) in runs.items():
        e = engine()
        if kind == "whole":
            e.set_energy_budget(None, whole_f if floors else whole)
        else:
            e.set_energy_budget_windows(QUARTERS, None, four_f if floors else four)
        if floors:
            e.set_budget_min_output(p_min)
        e.iterate(200)                               # settle (row summaries, warm starts)
        e.iterate(400)
        res.setdefault(name, []).append(1000.0 * e.last_call_ms() / 400)
        fails += e.solver_failures()
        if floors and rnd == 0:
            on_floor[name] = float(np.mean(e.get_primal()[0] <= p_min[:, None]))
        e.close()
print(f"{wl}: G={pp.G} S={pp.S} T={pp.T}, windows end at {QUARTERS}, library {lib or 'of this tree'}, median of {rounds} rounds [min..max], "
      f"microseconds per iteration")
for name, v in res.items():
    v = sorted(v)
    base = sorted(res[[n for n in res if n.startswith("(a)" if runs[name][0] == "whole" else "(b)")][0]])[rounds // 2]
    print(f"  {name:60s} {v[rounds // 2]:9.2f} us [{v[0]:.2f}..{v[-1]:.2f}] ({100.0 * (v[rounds // 2] / base - 1.0):+.1f} % of the case without floors)")
if has_floors:
    print(f"  bounds raised to the floor sum + 2 %: {raised[0]} rows (whole horizon), {raised[1]} windows; steps on their floors in the settled "
          f"run: " + ", ".join(f"{n[:3]} {100.0 * s:.1f} %" for n, s in on_floor.items()))
print(f"  solver failures in all runs: {fails}")
