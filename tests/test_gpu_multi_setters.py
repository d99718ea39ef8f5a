"""The two passes the six dopf_multi_set_* entries share (multi_set in csrc/dopf_comm.hip): every shard is checked before any is set,
so a value that one shard refuses leaves every shard as it was, and the refusal names the shard."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library loads: one HIP runtime per process)

from decentralopf_jl_amd import _capi, synth

pytestmark = pytest.mark.gpu

ALL_SIX = (_capi.F_STO_EFFICIENCY | _capi.F_STO_INITIAL_LEVEL | _capi.F_STO_TERMINAL_LEVEL | _capi.F_GEN_AVAILABILITY |
           _capi.F_LINE_RATING | _capi.F_GEN_QUADRATIC_COST)
SETTERS = [x.setter for x in _capi.EXTENSIONS]


def _valid(pp):
    """arguments every shard accepts, per setter, in the constructors' order"""
    S, G, T = pp.S, pp.G, pp.T
    return {
        "set_efficiency": (np.full(S, 0.9), np.full(S, 0.95)),
        "set_initial_levels": (0.25 * pp.sto_emax,),
        "set_terminal_levels": (0.1 * pp.sto_emax, 0.9 * pp.sto_emax),
        "set_availability": (np.stack([np.ones(T), np.full(T, 0.5)]), np.arange(G, dtype=np.int32) % 3 - 1),
        "set_line_rating": (0.9 * np.tile(pp.f_max[:, None], (1, T)),),
        "set_quadratic_cost": (np.full(G, 0.01),),
    }


def _invalid(pp, setter, good):
    """the valid arguments with one entry that one shard refuses, and that shard: the last storage or generator (shard 1's); the
    table of ratings is replicated, so shard 0 refuses it first"""
    bad = [np.array(a, copy=True) for a in good]
    if setter == "set_efficiency":
        bad[0][-1] = 1.5
    elif setter == "set_initial_levels":
        bad[0][-1] = 2.0 * pp.sto_emax[-1]
    elif setter == "set_terminal_levels":
        bad[0][-1], bad[1][-1] = 0.9 * pp.sto_emax[-1], 0.1 * pp.sto_emax[-1]          # lo > hi
    elif setter == "set_availability":
        bad[1][-1] = bad[0].shape[0]                                                     # profile_of = K
    elif setter == "set_line_rating":
        bad[0][1, 2] = -1.0
        return bad, 0
    elif setter == "set_quadratic_cost":
        bad[0][-1] = -1.0
    return bad, 1


@pytest.mark.parametrize("setter", SETTERS)
def test_a_refusal_from_one_shard_leaves_every_shard_as_it_was(hip_api, setter):
    """synthetic_case(n_gen=8, n_sto=4, T=4), 2 shards on device 0 over the host sum, all six flags: the smallest shapes at which both
    shards own a storage and a generator and T - 1 >= 2. The rating's case has 3 nodes and 2 lines on top: its entry (l = 1, t = 2)
    needs a second line (a copper plate has no table to refuse). After the refused call 3 iterations equal a single context's, which
    was given the valid values alone, within the bound of test_multi_engine_shards_equal_one_context."""
    net = dict(N=3, L=2) if setter == "set_line_rating" else {}
    pp = synth.synthetic_case(n_gen=8, n_sto=4, T=4, **net)
    g = 0.01 if net else 1.0 / (pp.G + pp.S)
    twin = _capi.Engine(hip_api, params=_capi.default_params(eps=0.0, gamma=g, device=0, flags=ALL_SIX), **pp.engine_kwargs())
    m = _capi.MultiEngine(hip_api, 2, params=_capi.default_params(eps=0.0, gamma=g, flags=_capi.F_COMM_HOST | ALL_SIX),
                          devices=[0, 0], **pp.engine_kwargs())
    valid = _valid(pp)
    for name in SETTERS:
        getattr(twin, name)(*valid[name])
        getattr(m, name)(*valid[name])
    bad, shard = _invalid(pp, setter, valid[setter])
    with pytest.raises(_capi.DopfError, match=f"shard {shard}"):
        getattr(m, setter)(*bad)
    twin.iterate(3)
    assert m.iterate(3) == (3, False)
    for a, b in zip(m.get_primal(), twin.get_primal()):
        assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
    m.close()
