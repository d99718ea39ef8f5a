"""Started by tests/test_gpu_horizon_roll.py with DOPF_GUARD=1: every device array of the library then ends on the last byte of
its own mapping, so that a read or write of dopf_roll_horizon / dopf_set_demand past an array's end is a GPU memory fault (the
process dies) instead of a silent access to a neighbour. The copper and network cases of that file's grid, every k."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dopf_pkg  # noqa: E402

dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth  # noqa: E402
from helpers import engine  # noqa: E402

assert os.environ.get("DOPF_GUARD")
hip = _capi.hip_api()
NET = dict(N=6, L=8, fmax_factor=0.7, fmax_min=5)
cases = [(dict(n_gen=40, n_sto=12, T=24, seed=801), (1, 5, 23)), (dict(n_gen=40, n_sto=12, T=100, seed=801), (37,)),
         (dict(n_gen=40, n_sto=12, T=192, seed=801), (64,)), (dict(n_gen=30, n_sto=10, T=12, seed=802, **NET), (1, 7))]
for case, ks in cases:
    pp = synth.synthetic_case(**case)
    for k in ks:
        e = engine(hip, pp, None, flags=_capi.F_STO_INITIAL_LEVEL, eps=0.0, gamma=0.02 if pp.L == 0 else 0.03)
        e.iterate(7)
        e.roll(k, np.round(pp.demand[:, :k] * 1.05) + 1.0)
        e.iterate(3)
        e.set_demand(e.demand() * 1.1)
        e.iterate(3)
        P, D, C, E = e.get_primal()
        assert np.all(np.isfinite(P)) and np.all(np.isfinite(E)) and e.solver_failures() == 0
        e.close()
print("horizon roll worker: ok")
