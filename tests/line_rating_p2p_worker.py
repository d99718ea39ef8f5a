"""Started by tests/test_gpu_line_rating.py (nothing else alive in the process): dopf_multi_set_line_rating on the peer exchange
(DOPF_F_COMM_P2P), two shards on ONE device. See the test's docstring."""
import gc
import os
import sys

import numpy as np
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dopf_pkg  # noqa: E402

dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth  # noqa: E402
from helpers import state_of  # noqa: E402
from helpers_line_rating import LR, constant_table, draw_table, quiet_state, rated_engine  # noqa: E402

hip = _capi.hip_api()
KEYS = ("lam", "mu", "rho", "inj", "avg_U", "avg_K", "flow", "cost")


def run(pp, plan, kw, tol, xflags=0):
    """plan: iteration counts and tables, in order, for a single context and for two shards on the exchange; after every call
    that iterates: the shards against the single context (to rounding), the replicated state bitwise equal on both shards, and
    both shards' chain decisions. Returns those decisions (dopf_debug_quiet), one per entry of the plan."""
    ref = rated_engine(hip, pp, xflags, **kw)
    wants = []
    for step in plan:
        if isinstance(step, int):
            ref.iterate(step)
            wants.append(state_of(ref))
        else:
            ref.set_line_rating(step)
            wants.append(None)
    ref.close()
    gc.collect()
    m = _capi.MultiEngine(hip, 2, params=_capi.default_params(flags=_capi.F_COMM_P2P | LR | xflags, **kw), devices=[0, 0], **pp.engine_kwargs())
    seen = []
    for step, want in zip(plan, wants):
        if isinstance(step, int):
            assert m.iterate(step) == (step, False)
            for a, b in zip(m.get_primal(), (want["P"], want["D"], want["C"], want["E"])):
                assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())
            first = state_of(m.shard(0))
            for i in range(2):
                got = state_of(m.shard(i))
                for key in KEYS:
                    assert np.abs(got[key] - want[key]).max() <= tol * max(1.0, np.abs(want[key]).max()), (key, i, step)
                    assert np.array_equal(got[key], first[key]), (key, i)        # rank-order sums: bitwise the same
        else:
            m.set_line_rating(step)
        qs = [quiet_state(hip, m.shard(i)) for i in range(2)]
        assert qs[0] == qs[1], qs                                                # every shard takes the same decision
        seen.append(qs[0])
    m.close()
    gc.collect()
    return seen


# the network of tests/p2p_worker.py (the three-launch chain on the exchange), the table changed once mid-run
pp = synth.synthetic_case(300, 40, 24, N=3, L=3, seed=4, fmax_factor=0.8, fmax_min=5)
run(pp, (draw_table(pp), 1, 4, draw_table(pp, seed=4), 7), dict(eps=0.0, gamma=0.01), 1e-9)
print("table changed mid-run ok", flush=True)

# the 118-node share: generous limits — the chain without k_reduce comes into use — then tight ones: the stale "no line flagged"
# is dropped on both shards alike, and the trajectory stays the single context's
ppq = synth.baseline_config(3, scale=0.02)
A = ppq.G + ppq.S
seen = run(ppq, (constant_table(ppq, 4.0), 20, constant_table(ppq, 0.3), 20), dict(eps=0.0, gamma=1.0 / A, w_flow=0.3 / A), 1e-9)
assert seen[1][:2] == (1, 1), seen              # allowed, and in use after the generous 20
assert seen[2][1] == 0, seen                    # right after the set
print("generous then tight ok", seen, flush=True)
print("line rating p2p worker: ok")
