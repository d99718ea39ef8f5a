"""csrc/budget_root.h and plan_chain's second flag word as a host program (the pattern of tests/test_ramp_net_host.py):
neither header has a HIP include, so tests/budget_main.cpp — its own main, those two headers only — is built with g++ under the
address and undefined-behaviour sanitizers (static runtimes) and fed plan cases and seeded rows as hexadecimal doubles.

The search a wave of k_gen_budget runs must give the step of helpers_budget.budget_project, which sorts every breakpoint instead of
bracketing. Bound: 1e-9 times the row's capacity, the suite's bound for a primal value (the two divide at different points of the
same linear segment, so the bits may differ)."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from decentralopf_jl_amd import _capi
from helpers_budget import budget_project, budget_rows

CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_chain.json")
MAX_EVALS = 192                                        # kBudgetMaxEvals


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("budget") / "budget")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "budget_main.cpp"), "-o", out], check=True)
    return out


def _run(exe, lines):
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])          # (a sanitizer report lands here)
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


# ---- plan_chain(shape, flags, cus, flags2) ---------------------------------------------------------------------------------------------

def _plan(exe, flags2, inputs):
    out = []
    for ln in _run(exe, [f"plan {flags2} {i}\n" for i in inputs]):
        head, rest = ln.split(" | ", 1)
        f = dict(kv.split("=", 1) for kv in head.split()[1:])
        out.append((int(f["genBudget"]), f["text"].replace("~", " "), rest, dict(kv.split("=") for kv in rest.split() if "=" in kv)))
    return out


def _with_flags(inp, flags):
    f = inp.split()
    f[5] = str(flags)
    return " ".join(f)


def test_the_second_word_at_zero_reproduces_the_pinned_plans(exe):
    cases = [c for c in json.load(open(GOLDEN))["cases"] if "env" not in c]
    got = _plan(exe, 0, [c["input"] for c in cases])
    bad = [c["name"] for c, (gb, text, rest, _) in zip(cases, got) if rest != c["output"] or gb != 0]
    assert not bad and len(cases) >= 140, bad[:5]


def test_the_budget_flag_gives_the_own_launch_chain(exe):
    cases = {c["name"]: c["input"] for c in json.load(open(GOLDEN))["cases"]}
    names = ["config1 cus=256", "config2 cus=256", "config3 cus=256", "config4 cus=256", "config3-share cus=256"]
    for (gb, text, rest, f), name in zip(_plan(exe, 1, [cases[n] for n in names]), names):
        assert gb == 1 and f["refusal"] == "0" and text == "-", name
        assert (f["genTT2"], f["fuseAgents"], f["fuseNet"], f["tail"]) == ("0", "0", "0", "0"), (name, f)
    # ... which is the chain DOPF_F_GEN_QUADRATIC_COST contexts run: the same plan, field by field, but for genQuad itself
    quad = _plan(exe, 0, [_with_flags(cases[n], _capi.F_GEN_QUADRATIC_COST) for n in names])
    both = _plan(exe, 1, [_with_flags(cases[n], _capi.F_GEN_QUADRATIC_COST) for n in names])
    for (_, _, _, fq), (gb, _, _, fb), (_, _, _, f1), name in zip(quad, both, _plan(exe, 1, [cases[n] for n in names]), names):
        assert gb == 1 and fq == fb, name
        assert {k: v for k, v in f1.items() if k != "genQuad"} == {k: v for k, v in fq.items() if k != "genQuad"}, name


def test_budgets_with_ramps_are_refused_and_no_generators_means_no_budget_kernel(exe):
    (gb, text, rest, f), = _plan(exe, 1, ["1 0 24 1000 100 %d 256 34 25 1000 100" % _capi.F_GEN_RAMP])
    assert f["refusal"] == "1" and "DOPF_F2_GEN_ENERGY_BUDGET" in text and "DOPF_F_GEN_RAMP" in text
    (gb, text, rest, f), = _plan(exe, 1, ["3 3 8 40 4 %d 256 34 25 20 10 10 2 1 1" % (_capi.F_GEN_RAMP | _capi.F_GEN_RAMP_NETWORK)])
    assert f["refusal"] == "1" and "DOPF_F2_GEN_ENERGY_BUDGET" in text
    (gb, text, rest, f), = _plan(exe, 1, ["1 0 24 0 100 0 256 34 25 0 100"])
    (gb0, _, rest0, _), = _plan(exe, 0, ["1 0 24 0 100 0 256 34 25 0 100"])
    assert gb == 0 and gb0 == 0 and f["refusal"] == "0" and rest == rest0


# ---- budget_root against the sorted-breakpoint reference ---------------------------------------------------------------------------------

def _hex(values):
    return " ".join(float(v).hex() for v in values)


def _line(steps, cap, lo, hi, max_evals=MAX_EVALS):
    body = " ".join(f"{float(c).hex()} {len(sl) - 1} {_hex(xk)} {_hex(vk)} {_hex(sl)}" for c, (xk, vk, sl) in zip(cap, steps))
    return f"root {len(steps)} {float(lo).hex()} {float(hi).hex()} {max_evals} {body}\n"


def _roots(exe, rows, max_evals=MAX_EVALS):
    out = []
    for ln in _run(exe, [_line(*row, max_evals) for row in rows]):
        f = ln.split()
        assert f[0] == "root"
        out.append((int(f[1][3:]), int(f[2][6:]), float.fromhex(f[3][3:]), np.array([float.fromhex(v) for v in f[4:]])))
    return out


@pytest.mark.parametrize("pwl", [False, True], ids=["clamp-only", "piecewise-linear"])
def test_the_search_gives_the_step_of_the_sorted_breakpoint_reference(exe, pwl):
    rows = list(budget_rows(144, 31 + pwl, pwl=pwl))
    sides, worst, most, spent = [], 0.0, 0, []
    for (rc, evals, nu, x), (steps, cap, lo, hi) in zip(_roots(exe, rows), rows):
        info = {}
        want = budget_project(steps, cap, lo, hi, info)
        scale = max(1.0, float(np.max(cap)))
        assert rc == (1 if info["side"] else 0) and (rc == 1 or (evals == 0 and nu == 0.0))
        err = float(np.max(np.abs(x - want))) / scale
        worst, most = max(worst, err), max(most, evals)
        assert err <= 1e-9, (len(steps), lo, hi, err)
        assert float(np.sum(x)) <= hi + 1e-9 * scale * len(steps) and float(np.sum(x)) >= lo - 1e-9 * scale * len(steps)
        assert info["side"] == 0 or (nu > 0) == (info["side"] > 0) or nu == 0.0
        sides.append(info["side"])
        spent += [evals] if rc == 1 else []
    assert min(sides.count(s) for s in (-1, 0, 1)) >= len(rows) // 6 and {len(r[0]) for r in rows} == {1, 2, 5, 64, 65, 130}
    assert most < MAX_EVALS
    print(f"{len(rows)} rows: worst difference {worst:.2e} of the capacity, {np.mean(spent):.1f} evaluations per searched row, at most {most}")


def test_a_row_that_runs_out_of_evaluations_keeps_its_clamped_step(exe):
    rows = [r for r in budget_rows(72, 33) if budget_project(r[0], r[1]).sum() > r[3] or budget_project(r[0], r[1]).sum() < r[2]]
    rows = [r for r in rows if len(r[0]) >= 5][:12]
    assert len(rows) >= 8
    for (rc, evals, nu, x), (steps, cap, lo, hi) in zip(_roots(exe, rows, 1), rows):
        if rc == 1:
            continue                                   # (the first probe may already end the search: a saturated or one-piece row)
        assert rc == -1 and nu == 0.0 and evals == 1 and np.array_equal(x, budget_project(steps, cap))
    assert sum(rc == -1 for rc, _, _, _ in _roots(exe, rows, 1)) >= 4
