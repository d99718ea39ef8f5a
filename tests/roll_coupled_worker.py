"""Started by tests/test_gpu_roll_coupled.py with DOPF_GUARD=1: every device array of the library then ends on the last byte of its
own mapping, so that a read or write of dopf_roll_horizon_coupled past an array's end is a GPU memory fault (the process dies) instead
of a silent access to a neighbour. One copper-plate context with ramps and budgets together and one network context with ramps."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dopf_pkg  # noqa: E402

dopf_pkg.load()
from decentralopf_jl_amd import _capi, shift_coupled, synth  # noqa: E402

assert os.environ.get("DOPF_GUARD")
hip = _capi.hip_api()
IL, RAMP, RAMP_NET = _capi.F_STO_INITIAL_LEVEL, _capi.F_GEN_RAMP, _capi.F_GEN_RAMP_NETWORK
BUDGET, PAIR = _capi.F2_GEN_ENERGY_BUDGET, _capi.F2_GEN_RAMP_BUDGET
cases = [(synth.synthetic_case(40, 12, 41, seed=801), RAMP, BUDGET | PAIR, (1, 5)),
         (synth.synthetic_case(30, 10, 12, N=6, L=8, seed=802, fmax_factor=0.7, fmax_min=5), RAMP | RAMP_NET, 0, (1, 7))]
for pp, flags, flags2, ks in cases:
    for k in ks:
        e = _capi.Engine(hip, params=_capi.default_params(flags=IL | flags, eps=0.0, gamma=0.02 if pp.L == 0 else 0.03), flags2=flags2,
                         **pp.engine_kwargs())
        e.set_initial_levels(np.zeros(pp.S))
        e.set_ramp(0.12 * pp.gen_pmax, 0.12 * pp.gen_pmax)
        if flags2:
            e.set_energy_budget(None, np.where(np.arange(pp.G) % 2 == 0, 0.8 * pp.T * pp.gen_pmax, np.inf))
        e.iterate(7)
        P = e.get_primal()[0]
        now = e.generator_coupling()
        want = shift_coupled(k, P, budget=(now["e_min"], now["e_max"]))
        e.roll_coupled(k, np.round(pp.demand[:, :k] * 1.05) + 1.0)
        now = e.generator_coupling()
        assert np.array_equal(now["p_prev"], want["gen_prev"])
        if flags2:
            assert np.array_equal(now["e_max"], want["gen_budget"][1])
        e.iterate(3)
        e.roll_coupled(1, np.round(pp.demand[:, :1] * 1.05) + 1.0)
        e.iterate(3)
        P, D, C, E = e.get_primal()
        assert np.all(np.isfinite(P)) and np.all(np.isfinite(E)) and e.solver_failures() == 0
        e.close()
print("roll coupled worker: ok")
