"""Per-iteration time with generator energy budgets (DOPF_F2_GEN_ENERGY_BUDGET; bench.py cannot set them): one workload
shape, the settings below in ONE process, each timed as the device-side span of a settled dopf_iterate call (DOPF_F_TIME_CALLS):
  (a) no flag, DOPF_F_NO_FUSE | DOPF_F_NO_TAIL_FUSE — the flagless problem on the launches a context with the flag runs (on an even
      T its generators still run in the pair kernels; run on the parent commit this is the parent's figure, the yardstick);
  (b) the flag with every budget at its default: the fast path alone;
  (c) the flag with every tenth row held to 60 % of the energy it delivers in (a)'s settled state, so that its budget binds; with it
      the share of rows whose clamped step breaks the budget in the iteration behind the timed ones (formed on the host from the state:
      those rows ran the search);
  (e) as (b), (f) as (c), with the budget prices recorded: dopf_get_generator_budget_price called once before the first iteration, which
      switches the context to the price-storing instantiations of k_gen_budget; (b) and (c) never call it;
  (d) no flag at all — the default chain (fused launch, one-launch tail): (a) against (d) is what the chain costs.
(b) against (a) is the cost of the feature's kernel on rows that need no search, (c) against (a) with a tenth of the rows searched. No
threshold is fixed in advance.
usage: python scripts/gen_budget_time.py <workload: config1 | config2> [rounds]"""
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
APART = _capi.F_NO_FUSE | _capi.F_NO_TAIL_FUSE
BUDGET = getattr(_capi, "F2_GEN_ENERGY_BUDGET", 0)
runs = {"(a) flagless, launches apart": (APART, 0, False, False), "(d) flagless, default chain": (0, 0, False, False)}
if BUDGET:      # (the parent commit has no such flag: there the script reports (a) and (d) alone)
    runs["(b) default budgets"] = (0, BUDGET, False, False)
    runs["(c) a tenth of the rows bind"] = (0, BUDGET, True, False)
    if hasattr(_capi.Engine, "budget_price"):
        runs["(e) (b) with prices recorded"] = (0, BUDGET, False, True)
        runs["(f) (c) with prices recorded"] = (0, BUDGET, True, True)


def searched(e, hi):
    """share of the generators whose clamped step from the engine's state breaks e_max (copper plate, no c2, no availability)"""
    gamma = 1.0 / A
    P = e.get_primal()[0]
    lam = e.get_duals()[0]
    s = e.get_consensus()[0].sum(axis=0)
    c = P - (pp.gen_mc[:, None] + lam[None, :] + gamma * s[None, :]) / (1.0 + gamma)
    return float(np.mean(np.clip(c, 0.0, pp.gen_pmax[:, None]).sum(axis=1) > hi))


api = _capi.hip_api()
res, share, energy, fails = {}, [], None, 0
for rnd in range(rounds):
    for name, (flags, flags2, bind, price) in runs.items():
        kw = dict(flags2=flags2) if flags2 else {}
        e = _capi.Engine(api, params=_capi.default_params(gamma=1.0 / A, eps=0.0, flags=flags | _capi.F_TIME_CALLS), **kw, **pp.engine_kwargs())
        hi = None
        if bind:
            hi = np.full(pp.G, np.inf)
            hi[::10] = 0.6 * energy[::10]
            e.set_energy_budget(None, hi)
        if price:
            e.budget_price()
        e.iterate(200)                               # settle (row summaries, warm starts)
        e.iterate(400)
        res.setdefault(name, []).append(1000.0 * e.last_call_ms() / 400)
        if energy is None:
            energy = e.get_primal()[0].sum(axis=1)   # (a), first round: the rows' energies in the settled flagless run
        if bind:
            share.append(searched(e, hi))
        fails += e.solver_failures()
        e.close()
print(f"{wl}: G={pp.G} S={pp.S} T={pp.T}, median of {rounds} rounds [min..max], microseconds per iteration")
base = sorted(res["(a) flagless, launches apart"])[rounds // 2]
for name, v in res.items():
    v = sorted(v)
    print(f"  {name:34s} {v[rounds // 2]:9.2f} us [{v[0]:.2f}..{v[-1]:.2f}] ({100.0 * (v[rounds // 2] / base - 1.0):+.1f} % of (a))")
if share:
    print(f"  rows that ran the search in (c): {100.0 * float(np.median(share)):.1f} % of {pp.G}; solver failures in all runs: {fails}")
