"""Cost per iteration of the device LP's long sweeps (kc_sto_long, kc_gen_rows_long) against the one-wave sweeps, on a
copper plate of 8 generators and 2 storages (the shape of tests/test_gpu_central_long.py). A solve that cannot converge (tol 1e-300)
runs exactly max_iters iterations and ends in a device synchronise. Three kinds of solve:
  (a) the one-wave sweeps at T = 512 — the code as it was before the long sweeps, the yardstick for (b);
  (b) the long sweeps at T = 512, behind DOPF_F_DEBUG_LONG_STO;
  (c) the long sweeps at T = 2048 (one full tile) and T = 8760 (an hourly year: five tiles).
<case> storages: dopf_central_solve (kc_gen next to kc_sto / kc_sto_long). rows: dopf_central_solve_coupled with a ramp of pmax / 20 on
every generator, an anchor and a budget of half the capacity's energy on every second one (kc_gen_rows / kc_gen_rows_long too).
Reported per solve, in milliseconds per iteration: wall clock of the whole call over res.iterations at max_iters = N2 ("whole": the
context's set-up is in it), and (t(N2) - t(N1)) / (N2 - N1) ("marginal": the iteration alone, with its metrics pass every 200
iterations). Host clock, the solves alternating, best of `reps`. No threshold: the figures go to DESIGN.md.

    python scripts/central_long_time.py <storages | rows> [reps]        ->  one JSON line
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import dopf_pkg

pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth

N1, N2 = 1000, 5000


def solver(api, kind, T, flags):
    pp = synth.synthetic_case(8, 2, T, seed=12)
    base = pp.engine_kwargs()
    params = _capi.default_params(flags=flags)
    if kind == "storages":
        return lambda n: _capi.central_solve(api, tol=1e-300, max_iters=n, params=params, **base)
    pmax = np.asarray(pp.gen_pmax, dtype=np.float64)
    ramp = pmax / 20.0
    e_max = np.full(pp.G, np.inf)
    e_max[::2] = 0.5 * T * pmax[::2]
    return lambda n: _capi.central_solve_coupled(api, tol=1e-300, max_iters=n, params=params, gen_ramp=(ramp, ramp.copy()),
                                                 gen_prev=0.5 * pmax, gen_budget=(np.zeros(pp.G), e_max), **base)


def main():
    kind = sys.argv[1] if len(sys.argv) > 1 else "storages"
    assert kind in ("storages", "rows"), kind
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    api = _capi.hip_api()
    solves = {"(a) one-wave T=512": solver(api, kind, 512, 0), "(b) long T=512": solver(api, kind, 512, _capi.F_DEBUG_LONG_STO),
              "(c) long T=2048": solver(api, kind, 2048, 0), "(c) long T=8760": solver(api, kind, 8760, 0)}
    for f in solves.values():
        f(200)                                      # warm-up: code objects, allocations
    best = {k: {N1: np.inf, N2: np.inf} for k in solves}
    for _ in range(reps):
        for n in (N1, N2):
            for k, f in solves.items():
                t0 = time.perf_counter()
                r = f(n)
                best[k][n] = min(best[k][n], time.perf_counter() - t0)
                assert r["iterations"] == n
    out = {k: {"whole": round(v[N2] / N2 * 1e3, 5), "marginal": round((v[N2] - v[N1]) / (N2 - N1) * 1e3, 5)} for k, v in best.items()}
    print(json.dumps({"case": f"{kind}: copper plate, G 8, S 2", "ms_per_iteration": out, "iterations": [N1, N2], "reps": reps}))


if __name__ == "__main__":
    main()
