"""csrc/ramp_budget.h and plan_chain's DOPF_F2_GEN_RAMP_BUDGET as a host program (the pattern of tests/test_budget_host.py):
neither header has a HIP include, so tests/ramp_budget_main.cpp — its own main, those two headers only — is built with g++ under the
address and undefined-behaviour sanitizers (static runtimes) and fed plan cases and seeded rows as hexadecimal doubles. The
candidates' work arrays have the device's interleaved layout at its exact size, so an index out of a lane's share is a sanitizer report.

The search a wave of k_gen_ramp_budget runs must give the step of helpers_ramp_budget.ramp_budget_project, which bisects the
multiplier until no double is left. Bound: 1e-9 times max(1, pmax), the suite's bound for a primal value. The reference itself is
checked by helpers_ramp.ramp_kkt_violation with the budget's multiplier added to the gradient."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from decentralopf_jl_amd import _capi
from helpers_ramp import ramp_infeasibility, ramp_kkt_violation, ramp_project
from helpers_ramp_budget import HOST_T, PAIR, both_bind, host_rows, ramp_budget_project

CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
MAX_ROUNDS = 32                                        # kRampBudgetMaxRounds
RAMP, RAMP_NET, BUDGET = _capi.F_GEN_RAMP, _capi.F_GEN_RAMP_NETWORK, _capi.F2_GEN_ENERGY_BUDGET


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ramp_budget") / "ramp_budget")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "ramp_budget_main.cpp"), "-o", out], check=True)
    return out


def _run(exe, lines):
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])          # (a sanitizer report lands here)
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


# ---- plan_chain ---------------------------------------------------------------------------------------------------------------------

PLATE = "1 0 24 1000 100 %d 256 34 25 1000 100"
NET = "3 3 8 40 4 %d 256 34 25 20 10 10 2 1 1"


def _plan(exe, flags2, inp):
    ln, = _run(exe, [f"plan {flags2} {inp}\n"])
    f = dict(kv.split("=", 1) for kv in ln.split()[1:])
    f["text"] = f["text"].replace("~", " ")
    return f


def test_the_pair_is_accepted_on_a_plate_with_the_own_launch_chain(exe):
    f = _plan(exe, BUDGET | PAIR, PLATE % RAMP)
    assert PAIR == 8 and (f["genRampBudget"], f["genRamp"], f["genBudget"], f["refusal"], f["text"]) == ("1", "1", "1", "0", "-")
    assert (f["genTT2"], f["fuseAgents"], f["fuseNet"], f["tail"]) == ("0", "0", "0", "0")
    g = _plan(exe, 0, PLATE % RAMP)                     # ... the chain of a ramp context
    assert g["genRampBudget"] == "0" and all(f[k] == g[k] for k in ("genTT2", "fuseAgents", "fuseNet", "tail"))
    f = _plan(exe, BUDGET | PAIR, "1 0 24 0 100 %d 256 34 25 0 100" % RAMP)        # no generators: accepted and ignored
    assert (f["genRampBudget"], f["refusal"]) == ("0", "0")


def test_the_three_refusals_and_the_one_of_the_two_older_flags(exe):
    for flags, flags2 in ((RAMP, PAIR), (0, BUDGET | PAIR), (0, PAIR)):
        f = _plan(exe, flags2, PLATE % flags)
        assert f["refusal"] == "1" and f["genRampBudget"] == "0", (flags, flags2)
        assert "DOPF_F2_GEN_RAMP_BUDGET means nothing without" in f["text"] and "DOPF_F_GEN_RAMP" in f["text"] and \
            "DOPF_F2_GEN_ENERGY_BUDGET" in f["text"]
    f = _plan(exe, BUDGET | PAIR, NET % (RAMP | RAMP_NET))
    assert f["refusal"] == "1" and f["genRampBudget"] == "0" and "DOPF_F2_GEN_RAMP_BUDGET" in f["text"] and "copper plates" in f["text"]
    for inp in (PLATE % RAMP, NET % (RAMP | RAMP_NET)):                          # without the bit: the refusal of before
        f = _plan(exe, BUDGET, inp)
        assert f["refusal"] == "1" and f["text"].startswith("DOPF_F2_GEN_ENERGY_BUDGET does not combine with DOPF_F_GEN_RAMP")


# ---- the search against the bisecting reference ---------------------------------------------------------------------------------------

def _line(row, max_rounds=MAX_ROUNDS):
    c, q, cap, up, down, prev, e_min, e_max, pm = row
    h = lambda v: float(v).hex()
    return (f"row {len(c)} {h(q)} {h(up)} {h(down)} {h(np.nan if prev is None else prev)} {h(e_min)} {h(e_max)} {h(pm)} {max_rounds} "
            + " ".join(h(v) for v in cap) + " " + " ".join(h(v) for v in c) + "\n")


def _rows(exe, rows, max_rounds=MAX_ROUNDS):
    out = []
    for ln in _run(exe, [_line(r, max_rounds) for r in rows]):
        f = ln.split()
        assert f[0] == "row"
        out.append((int(f[1][3:]), int(f[2][7:]), float.fromhex(f[3][3:]), np.array([float.fromhex(v) for v in f[4:]])))
    return out


@pytest.fixture(scope="module")
def reference():
    """the 84 seeded rows with the reference's step and what it says of each (computed once)"""
    rows = host_rows()
    want = []
    for c, q, cap, up, down, prev, e_min, e_max, pm in rows:
        info = {}
        want.append((ramp_budget_project(c, q, cap, up, down, prev, e_min, e_max, info), info))
    return rows, want


def test_the_reference_is_optimal_by_its_certificate(reference):
    """stationarity of q (x - c) + nu under box and ramps (multipliers from HiGHS), the budget met, the sign of nu"""
    rows, want = reference
    stat = infe = 0.0
    for (c, q, cap, up, down, prev, e_min, e_max, pm), (x, info) in zip(rows, want):
        nu = info["nu"]
        i, s = ramp_kkt_violation(x, q * (x - c) + nu, cap, up, down, prev)
        scale = max(1.0, pm)
        stat, infe = max(stat, s / (scale * q)), max(infe, i / scale)
        total = float(x.sum())
        assert e_min - 1e-9 * scale * len(c) <= total <= e_max + 1e-9 * scale * len(c)
        assert info["side"] == 0 or (nu > 0) == (info["side"] > 0)
    print(f"{len(rows)} rows: stationarity {stat:.2e} relative, infeasibility {infe:.2e} relative")
    assert stat <= 1e-9 and infe <= 1e-12


def test_the_search_gives_the_step_of_the_bisecting_reference(exe, reference):
    rows, want = reference
    worst, most, bind = 0.0, 0, 0
    for (rc, rounds, nu, x), row, (xr, info) in zip(_rows(exe, rows), rows, want):
        c, q, cap, up, down, prev, e_min, e_max, pm = row
        scale = max(1.0, pm)
        assert rc == (1 if info["side"] else 0) and (rc == 1 or (rounds == 0 and nu == 0.0)), (len(c), rc, info)
        err = float(np.abs(x - xr).max()) / scale
        worst, most = max(worst, err), max(most, rounds)
        bind += both_bind(xr, up, down, prev, info)
        print(f"T={len(c)} side={info['side']} rounds={rounds} |x - reference| {err:.2e} (scaled)")
        assert err <= 1e-9, (len(c), err)
        assert ramp_infeasibility(x, cap, up, down, prev) <= 1e-9 * scale
        assert e_min - 1e-9 * scale <= float(x.sum()) <= e_max + 1e-9 * scale
    print(f"{len(rows)} rows: worst difference {worst:.2e} (scaled), at most {most} rounds, ramp and budget both bind in {bind}")
    assert 4 * bind >= len(rows) and {len(r[0]) for r in rows} == set(HOST_T)
    assert most < MAX_ROUNDS


def test_a_row_that_runs_out_of_rounds_keeps_its_step_at_zero(exe, reference):
    rows, want = reference
    pick = [r for r, (x, info) in zip(rows, want) if info["side"] and len(r[0]) >= 5][:12]
    assert len(pick) >= 8
    gave_up = 0
    for (rc, rounds, nu, x), (c, q, cap, up, down, prev, e_min, e_max, pm) in zip(_rows(exe, pick, 1), pick):
        if rc == 1:
            continue                                   # (the first round may already meet the bound)
        gave_up += 1
        assert rc == -1 and nu == 0.0 and rounds == 1
        assert float(np.abs(x - ramp_project(c, q, cap, up, down, prev)).max()) <= 1e-9 * max(1.0, pm)
    assert gave_up >= 4
