"""DOPF_F2_GEN_RAMP_BUDGET without a GPU: the header, the bindings' constant and the Julia shim's, the second word's
unknown bits, and the rule by which the hosts add the bit."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT
from decentralopf_jl_amd import _capi

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
BASE_KEYS = {"N", "L", "T", "demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax",
             "sto_node"}


def _comment(name):
    text = HDR[HDR.index("#define " + name):]
    return text[:text.index("*/")]


def test_the_define_is_eight_here_in_the_bindings_and_in_the_shim():
    m = re.search(r"^#define\s+DOPF_F2_GEN_RAMP_BUDGET\s+(\d+)", HDR, re.M)
    assert m and int(m.group(1)) == 8 == _capi.F2_GEN_RAMP_BUDGET
    m = re.search(r"^const DOPF_F2_GEN_RAMP_BUDGET = (\d+)", JL, re.M)
    assert m and int(m.group(1)) == 8
    assert re.search(r"flags2 \|= DOPF_F2_GEN_RAMP_BUDGET", JL) and re.search(r"DOPF_F2_GEN_ENERGY_BUDGET\) != 0 && L == 0", JL)
    second = {k: int(v) for k, v in re.findall(r"^#define\s+(DOPF_F2_\w+)\s+(\d+)", HDR, re.M)}
    assert second == {"DOPF_F2_GEN_ENERGY_BUDGET": 1, "DOPF_F2_GEN_RAMP_BUDGET": 8}


def test_the_header_text_holds():
    new = _comment("DOPF_F2_GEN_RAMP_BUDGET")
    for words in ("copper plates", "DOPF_F_GEN_RAMP", "DOPF_F2_GEN_ENERGY_BUDGET", "exact minimiser", "DOPF_E_NOMEM", "DOPF_E_SOLVER",
                  "jointly feasible", "DOPF_E_INVALID", "accepted and ignored", "dopf_roll_horizon", "ignore the bit"):
        assert words in new, words
    ramp, budget = _comment("DOPF_F_GEN_RAMP "), _comment("DOPF_F2_GEN_ENERGY_BUDGET")
    assert "DOPF_F2_GEN_RAMP_BUDGET" in ramp and "DOPF_F2_GEN_RAMP_BUDGET" in budget
    assert "ignore the bit" in budget and "refused (DOPF_E_UNSUPPORTED" in budget           # what the older tests quote stays
    last = _comment("DOPF_F_GEN_RAMP_NETWORK")
    assert "LAST bit" in last and "second flag word" in last


def test_bits_two_four_and_sixty_four_are_still_unknown(three_node):
    api = _capi.hip_api()
    pp = three_node[4]
    prob, keep, G, S = _capi._problem(**{k: v for k, v in pp.engine_kwargs().items() if k in BASE_KEYS})
    q = _capi.default_params()
    for word, bit in ((2, 2), (4, 4), (8 | 64, 64), (1 | 8 | 2, 2)):
        ctx = ctypes.c_void_p()
        rc = api.create_ex(ctypes.byref(ctx), ctypes.byref(prob), ctypes.byref(q), word)
        msg = api.last_error(None).decode()
        assert rc == -1 and not ctx.value and f"unknown bit {bit}" in msg and "flags2" in msg, (rc, msg)


class _Plate:
    N, L, T, G, S = 1, 0, 2, 4, 1


class _Net:
    N, L, T, G, S = 3, 3, 2, 4, 1


def test_flags2_adds_the_bit_for_ramps_and_budgets_on_a_plate():
    api = _capi.hip_api()
    hi = np.array([np.inf, 50.0, np.inf, np.inf])
    ramp = (np.full(4, 5.0), np.full(4, 5.0))
    params, todo = _capi._extensions(api, None, _Plate, {}, dict(gen_budget=(None, hi), gen_ramp=ramp))
    assert _capi._flags2(todo) == 9 and _capi._flags2(todo, 0) == 9 and params.flags == _capi.F_GEN_RAMP
    params, todo = _capi._extensions(api, None, _Plate, {}, dict(gen_budget=(None, hi)))
    assert _capi._flags2(todo) == 1
    params, todo = _capi._extensions(api, None, _Plate, {}, dict(gen_ramp=ramp))
    assert _capi._flags2(todo) == 0
    params, todo = _capi._extensions(api, None, _Plate, {}, dict(gen_budget=(None, hi), gen_prev=np.zeros(4)))        # an anchor alone: ramps too
    assert _capi._flags2(todo, 0) == 9
    # with lines the bit is not added: the library's refusal of the two older flags together surfaces as it is
    params, todo = _capi._extensions(api, None, _Net, {}, dict(gen_budget=(None, hi), gen_ramp=ramp))
    assert _capi._flags2(todo, _Net.L) == 1 and params.flags & _capi.F_GEN_RAMP_NETWORK
