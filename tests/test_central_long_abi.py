"""The device LP beyond T = 512 without a GPU: dopf_central_solve_coupled with ramps and dopf_central_solve with storages
no longer refuse a horizon of 600 — with no device visible the calls now get as far as looking for one — the header says so, and the
refusals that need no values still come first."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from decentralopf_jl_amd import _capi, synth

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
DP = ctypes.POINTER(ctypes.c_double)
INVALID, UNSUPPORTED = -1, -4
BASE_KEYS = ("N", "L", "T", "demand", "ptdf", "f_max", "gen_mc", "gen_pmax", "gen_node", "sto_mc", "sto_pmax", "sto_emax", "sto_node")


@pytest.fixture(scope="module")
def pp():
    return synth.synthetic_case(8, 2, 600, seed=12)


@pytest.fixture()
def api(monkeypatch):
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "-1")          # no device is visible to the calls below
    return _capi.hip_api()


def _coupled(api, pp, up, down):
    kw = pp.engine_kwargs()
    prob, keep, G, S = _capi._problem(**{k: kw[k] for k in BASE_KEYS})
    q, res = _capi.default_params(), _capi.DopfCentralResult()
    dp = lambda a: None if a is None else a.ctypes.data_as(DP)
    rc = api.central_solve_coupled(ctypes.byref(prob), ctypes.byref(q), None, None, None, None, None, 0, None, None, None, dp(up), dp(down),
                                   None, None, None, 1e-7, 1000, ctypes.byref(res), *([None] * 11))
    msg = api.last_error(None)
    return rc, (msg.decode() if msg else "")


def test_coupled_entry_takes_ramps_at_T_600(api, pp):
    assert pp.T == 600
    rc, msg = _coupled(api, pp, np.full(pp.G, 5.0), np.full(pp.G, 5.0))
    print(rc, msg)
    assert rc != 0 and rc != UNSUPPORTED, (rc, msg)                     # (no device: the call fails, but not as unsupported)
    assert "supports T <= 512" not in msg


def test_plain_entry_takes_storages_at_T_600_with_default_flags(api, pp):
    kw = pp.engine_kwargs()
    prob, keep, G, S = _capi._problem(**{k: kw[k] for k in BASE_KEYS})
    assert S > 0
    q, res = _capi.default_params(), _capi.DopfCentralResult()
    assert not q.flags & (_capi.F_LONG_HORIZON | _capi.F_DEBUG_LONG_STO)
    rc = api.central_solve(ctypes.byref(prob), ctypes.byref(q), 1e-7, 1000, ctypes.byref(res), *([None] * 9))
    msg = api.last_error(None)
    msg = msg.decode() if msg else ""
    print(rc, msg)
    assert rc != 0 and rc != UNSUPPORTED, (rc, msg)
    assert "need DOPF_F_LONG_HORIZON" not in msg


def test_header_no_longer_says_long_horizons_are_refused():
    assert "are refused with ramps or budgets" not in HDR
    at = HDR.index("the central reference on the device")
    assert "any horizon" in HDR[at:HDR.index("typedef struct dopf_central_result")]


def test_pairing_refusal_still_comes_before_any_device_at_T_600(api, pp):
    rc, msg = _coupled(api, pp, np.full(pp.G, 5.0), None)
    assert rc == INVALID and "dopf_central_solve_coupled" in msg and "ramp_up and ramp_down" in msg, (rc, msg)
