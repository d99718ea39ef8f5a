"""Cost per iteration of the coupled device LP's generator sweep (kc_gen_rows) against kc_gen, on the copper plate with T = 70 of
tests/test_gpu_central_coupled.py. A solve that cannot converge (tol 1e-300) runs exactly max_iters iterations and ends in a
device synchronise, so (time at n2 - time at n1) / (n2 - n1) is the cost of one iteration of the whole chain (kc_price, the generator
sweep, kc_sto, k_reduce, kc_dual, and the metrics pass every 200 iterations) without the context's set-up; the three chains differ
in the generator sweep alone. Host clock around the calls, the variants alternating, best of `reps`.

    python scripts/central_coupled_time.py [reps]        ->  one JSON line
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import dopf_pkg

pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth
from decentralopf_jl_amd.central import solve_central_packed
from helpers_central_coupled import draw_inputs

N1, N2 = 2000, 12000


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    api = _capi.hip_api()
    pp = synth.synthetic_case(60, 9, 70, seed=5)
    d = draw_inputs(pp, lambda q, **kw: solve_central_packed(q, duals=False, **kw))
    G = pp.G
    base = pp.engine_kwargs()
    variants = {
        "kc_gen": lambda n: _capi.central_solve(api, tol=1e-300, max_iters=n, **base),
        "kc_gen_rows_no_rows": lambda n: _capi.central_solve_coupled(api, tol=1e-300, max_iters=n, gen_ramp=(np.full(G, np.inf),) * 2, **base),
        "kc_gen_rows_both": lambda n: _capi.central_solve_coupled(api, tol=1e-300, max_iters=n, gen_ramp=d["ramp"], gen_prev=d["prev"],
                                                                 gen_budget=d["budget"], **base),
    }
    for f in variants.values():
        f(200)                                      # warm-up: code objects, allocations
    best = {k: {N1: np.inf, N2: np.inf} for k in variants}
    for _ in range(reps):
        for n in (N1, N2):
            for k, f in variants.items():
                t0 = time.perf_counter()
                r = f(n)
                best[k][n] = min(best[k][n], time.perf_counter() - t0)
                assert r["iterations"] == n
    out = {k: round((v[N2] - v[N1]) / (N2 - N1) * 1e6, 3) for k, v in best.items()}
    print(json.dumps({"case": "copper-T70 (G 60, S 9)", "us_per_iteration": out, "iterations": [N1, N2], "reps": reps}))


if __name__ == "__main__":
    main()
