"""_capi.EXTENSIONS, the one host-side description of the six problem extensions, row by row against what it
describes: the header, the library's bindings, the four hosts' setters and the refusals of an API without the entries. Keeps the
table honest; the per-feature files (tests/test_*_abi.py) pin each extension's behaviour."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from decentralopf_jl_amd import _capi, admm, sharded

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
ROWS = {x.setter: x for x in _capi.EXTENSIONS}


def _values(pp):
    """per setter: (constructor keywords at the default value, at another value)"""
    S, G, T = pp.S, pp.G, pp.T
    table = np.tile(pp.f_max[:, None], (1, T))
    return {
        "set_efficiency": (dict(sto_eta=(np.ones(S), np.ones(S))), dict(sto_eta=(np.full(S, 0.9), np.ones(S)))),
        "set_initial_levels": (dict(sto_e0=np.zeros(S)), dict(sto_e0=0.5 * pp.sto_emax)),
        "set_terminal_levels": (dict(sto_end_lo=np.zeros(S), sto_end_hi=pp.sto_emax.copy()), dict(sto_end_lo=0.5 * pp.sto_emax)),
        "set_availability": (dict(gen_avail=np.ones((1, T)), gen_avail_of=np.zeros(G, dtype=np.int32)),
                             dict(gen_avail=np.full((1, T), 0.5), gen_avail_of=np.zeros(G, dtype=np.int32))),
        "set_line_rating": (dict(line_rating=table), dict(line_rating=0.5 * table)),
        "set_quadratic_cost": (dict(gen_c2=np.zeros(G)), dict(gen_c2=np.full(G, 0.1))),
    }


def test_the_order_is_the_constructors():
    # the efficiencies before the levels (their reachability checks see them), the two replace-in-place setters last
    assert list(ROWS) == ["set_efficiency", "set_initial_levels", "set_terminal_levels", "set_availability", "set_line_rating",
                          "set_quadratic_cost"]
    assert [x.keys for x in _capi.EXTENSIONS] == [("sto_eta",), ("sto_e0",), ("sto_end_lo", "sto_end_hi"),
                                                  ("gen_avail", "gen_avail_of"), ("line_rating",), ("gen_c2",)]


@pytest.mark.parametrize("setter", list(ROWS))
def test_row_matches_the_header_and_the_library(setter):
    x = ROWS[setter]
    name = [k for k, v in vars(_capi).items() if k.startswith("F_") and v == x.flag]
    assert len(name) == 1
    m = re.search(r"#define\s+DOPF_%s\s+(\d+)" % name[0], HDR)
    assert m and int(m.group(1)) == x.flag
    assert re.search(r"^int\s+dopf_%s\(dopf_ctx \*ctx, " % x.entry, HDR, re.M)
    assert re.search(r"^int\s+dopf_multi_%s\(dopf_multi \*m, " % x.entry, HDR, re.M)
    api = _capi.CApi(_capi.HIP_LIB_PATH)
    for entry in (x.entry, "multi_" + x.entry):
        f = getattr(api, entry)
        assert f.restype is ctypes.c_int
        assert list(f.argtypes) == [ctypes.c_void_p] + list(x.argtypes)


@pytest.mark.parametrize("setter", list(ROWS))
def test_every_host_has_the_setter(setter):
    for cls in (_capi.Engine, _capi.MultiEngine, admm.ADMM, sharded.ShardedADMM):
        assert callable(getattr(cls, setter)), cls


@pytest.mark.parametrize("setter", list(ROWS))
def test_an_api_without_the_entry(three_node, oracle_api, setter):
    x, pp = ROWS[setter], three_node[4]
    default, other = _values(pp)[setter]
    assert set(default) == set(x.keys) and set(other) <= set(x.keys)
    assert not hasattr(oracle_api, x.entry)
    build = lambda **kw: _capi.Engine(oracle_api, params=_capi.default_params(), mode=0, **kw, **pp.engine_kwargs())
    e = build(**default)                                    # the default value: nothing to set, and no flag
    assert e.params.flags == 0 and all(v is None for v in e._mirror.values())
    with pytest.raises(_capi.DopfError) as err:
        build(**other)
    assert str(err.value) == f"oracle_*: this API has no {x.what} ({x.why})"
    with pytest.raises(_capi.DopfError) as err:
        getattr(e, setter)()
    assert str(err.value) == f"oracle_*: this API has no {x.what}" + (" (unsupported)" if x.optional else "")
