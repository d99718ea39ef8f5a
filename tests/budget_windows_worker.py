"""Started by tests/test_gpu_gen_budget_windows.py with DOPF_GUARD=1: every device array of the library then ends on the last byte of
its own mapping, so that a read or write of k_gen_budget_win or of dopf_set_generator_energy_budget_windows past an array's end — the
ends, the two budget tables, the prices, a row of P behind a window's last step — is a GPU memory fault (the process dies) instead of a
silent access to a neighbour. A copper plate and a network, each through a first table, a table of another n_win (a new allocation),
one window per step and the removal."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dopf_pkg  # noqa: E402

dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth  # noqa: E402

assert os.environ.get("DOPF_GUARD")
hip = _capi.hip_api()
BUDGET = _capi.F2_GEN_ENERGY_BUDGET
cases = [(synth.synthetic_case(40, 12, 41, seed=801), 0.02, [(7, 41), (1, 20, 21, 41), tuple(range(1, 42))]),
         (synth.synthetic_case(30, 10, 12, N=6, L=8, seed=802, fmax_factor=0.7, fmax_min=5), 0.03, [(6, 12), (1, 12), tuple(range(1, 13))])]
for pp, gamma, tables in cases:
    e = _capi.Engine(hip, params=_capi.default_params(eps=0.0, gamma=gamma), flags2=BUDGET, **pp.engine_kwargs())
    e.iterate(5)
    for ends in tables:
        P = e.get_primal()[0]
        cuts = np.concatenate([[0], ends])
        S = np.stack([P[:, a:b].sum(axis=1) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
        room = np.stack([(b - a) * pp.gen_pmax for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
        k = np.arange(S.size).reshape(S.shape) % 3
        hi = np.where(k == 1, 0.6 * S, np.inf)
        lo = np.where(k == 2, S + 0.4 * (room - S), 0.0)
        e.set_energy_budget_windows(ends, lo, hi)
        e.iterate(7)
        P = e.get_primal()[0]
        now = np.stack([P[:, a:b].sum(axis=1) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
        tol = 1e-9 * np.maximum(1.0, pp.gen_pmax)[:, None] * np.diff(cuts)[None, :]
        assert np.all(now <= hi + tol) and np.all(now >= lo - tol)
        nu = e.budget_window_price()
        assert nu.shape == S.shape and np.all(np.isfinite(nu)) and np.all(nu[k == 0] == 0.0)
        assert e.solver_failures() == 0
    e.set_energy_budget_windows(None)
    e.iterate(3)
    assert np.all(np.isfinite(e.get_primal()[0])) and e.energy_budget_windows() is None
    e.close()
print("budget windows worker: ok")
