"""csrc/budget_root.h with floors as a host program (dopf_set_generator_budget_min_output; the pattern of
tests/test_budget_host.py): tests/budget_floor_main.cpp — its own main, that header only — is built with g++ under the address and
undefined-behaviour sanitizers (static runtimes) and fed seeded rows as hexadecimal doubles.

The search a wave of k_gen_budget<.., MN = true> runs — budget_root with the pieces of the four-argument budget_piece and the clip
[floor_t, cap_t] — must give the step of helpers_budget_floor.budget_project_floor, which sorts every breakpoint instead of
bracketing, and on plate rows that of a dense QP. Bound: 1e-9 times the row's capacity, the suite's bound for a primal value (the
two divide at different points of the same linear segment, so the bits may differ). With every floor at 0 the program prints the
bits of tests/budget_main.cpp's root request."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers_budget import budget_rows
from helpers_budget_floor import budget_floor_rows, budget_project_floor, qp_plate_row

CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
MAX_EVALS = 192                                        # kBudgetMaxEvals


def _build(tmp, source, name):
    out = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", source), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("budget_floor"), "budget_floor_main.cpp", "budget_floor")


@pytest.fixture(scope="module")
def exe_plain(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("budget_plain"), "budget_main.cpp", "budget")


def _run(exe, lines):
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])          # (a sanitizer report lands here)
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def _hex(values):
    return " ".join(float(v).hex() for v in values)


def _line(steps, floor, cap, lo, hi, max_evals=MAX_EVALS):
    """floor None: a request of tests/budget_main.cpp (no floor per step)"""
    fl = [""] * len(steps) if floor is None else [float(f).hex() + " " for f in floor]
    body = " ".join(f"{f}{float(c).hex()} {len(sl) - 1} {_hex(xk)} {_hex(vk)} {_hex(sl)}" for f, c, (xk, vk, sl) in zip(fl, cap, steps))
    return f"root {len(steps)} {float(lo).hex()} {float(hi).hex()} {max_evals} {body}\n"


def _roots(exe, rows, max_evals=MAX_EVALS):
    out = []
    for ln in _run(exe, [_line(*row, max_evals) for row in rows]):
        f = ln.split()
        assert f[0] == "root"
        out.append((int(f[1][3:]), int(f[2][6:]), float.fromhex(f[3][3:]), np.array([float.fromhex(v) for v in f[4:]])))
    return out


@pytest.mark.parametrize("pwl", [False, True], ids=["clamp-only", "piecewise-linear"])
def test_the_search_with_floors_gives_the_step_of_the_sorted_breakpoint_reference(exe, oracle_api, pwl):
    """192 seeded rows of the sizes 1, 2, 5, 64, 65, 130 in eight classes (helpers_budget_floor.budget_floor_rows): x within 1e-9 of the
    capacity of the reference, rc and the sign of nu, floors and budget kept; plate rows of up to 65 steps also against the dense QP
    (the same bound, as tests/test_gen_min_output_abi.py holds that solver to). Largest observed difference to the reference: 1.31e-15 of
    the capacity (clamp-only), 5.44e-15 (piecewise-linear); to the QP 9.81e-13; at most 21 and 29 evaluations per row; 52 and 53 rows in
    which the search moves a step onto a floor > 0."""
    rows = list(budget_floor_rows(192, 41 + pwl, pwl=pwl))
    sides, worst, worst_qp, most, on_floor = [], 0.0, 0.0, 0, 0
    for k, ((rc, evals, nu, x), (steps, fl, cap, lo, hi)) in enumerate(zip(_roots(exe, rows), rows)):
        info = {}
        want = budget_project_floor(steps, fl, cap, lo, hi, info)
        scale = max(1.0, float(np.max(cap)))
        assert rc == (1 if info["side"] else 0) and (rc == 1 or (evals == 0 and nu == 0.0)), (k, rc, info)
        err = float(np.max(np.abs(x - want))) / scale
        worst, most = max(worst, err), max(most, evals)
        assert err <= 1e-9, (k, len(steps), lo, hi, err)
        assert np.all(x >= fl) and np.all(x <= cap), k
        assert float(np.sum(x)) <= hi + 1e-9 * scale * len(steps) and float(np.sum(x)) >= lo - 1e-9 * scale * len(steps), k
        assert info["side"] == 0 or (nu > 0) == (info["side"] > 0) or nu == 0.0, k
        if info["unique"]:
            assert abs(nu - info["nu"]) <= 1e-9 * max(1.0, abs(info["nu"])), (k, nu, info["nu"])
        sides.append(info["side"])
        on_floor += info["moved_onto_floor"]
        if not pwl and len(steps) <= 65:
            c, q = [s[0][0] for s in steps], steps[0][2][0]
            worst_qp = max(worst_qp, float(np.max(np.abs(qp_plate_row(oracle_api, c, q, fl, cap, lo, hi) - x))) / scale)
    assert min(sides.count(s) for s in (-1, 0, 1)) >= len(rows) // 8 and {len(r[0]) for r in rows} == {1, 2, 5, 64, 65, 130}
    assert on_floor >= len(rows) // 8, on_floor            # rows in which the search itself puts a step onto a floor > 0
    assert most < MAX_EVALS
    assert worst_qp <= 1e-9, worst_qp
    print(f"{len(rows)} rows: worst difference {worst:.2e} of the capacity (dense QP: {worst_qp:.2e}), at most {most} evaluations, "
          f"{on_floor} rows with a step moved onto its floor")


def test_the_two_new_row_classes(exe):
    """e_max = sum floor: the search going up ends with every step on its floor, on the bound itself (rc = 1, nu > 0) unless the
    clamped step is there already; every box one point: nothing to search (rc = 0), the step is the floor = the cap"""
    rows = list(budget_floor_rows(192, 43))
    least = [r for k, r in enumerate(rows) if (k // 6) % 8 == 3]
    point = [r for k, r in enumerate(rows) if (k // 6) % 8 == 6]
    assert len(least) >= 12 and len(point) >= 12
    searched = 0
    for (rc, evals, nu, x), (steps, fl, cap, lo, hi) in zip(_roots(exe, least), least):
        assert np.array_equal(x, fl) and sum(x.tolist()) == hi
        assert (rc == 1 and nu > 0.0) or (rc == 0 and nu == 0.0)
        searched += rc
    assert searched >= len(least) // 2
    for (rc, evals, nu, x), (steps, fl, cap, lo, hi) in zip(_roots(exe, point), point):
        assert rc == 0 and evals == 0 and nu == 0.0 and np.array_equal(x, cap) and np.array_equal(fl, cap)


def test_a_row_that_runs_out_of_evaluations_keeps_its_clamped_step(exe):
    rows = [r for r in budget_floor_rows(96, 45) if len(r[0]) >= 5]
    rows = [r for r in rows if not r[3] <= sum(budget_project_floor(r[0], r[1], r[2]).tolist()) <= r[4]][:16]
    assert len(rows) >= 8
    got = _roots(exe, rows, 2)
    for (rc, evals, nu, x), (steps, fl, cap, lo, hi) in zip(got, rows):
        if rc == 1:
            continue                                   # (two probes may already end the search: a saturated or one-piece row)
        assert rc == -1 and nu == 0.0 and evals == 2 and np.array_equal(x, budget_project_floor(steps, fl, cap))
    assert sum(rc == -1 for rc, _, _, _ in got) >= 4


@pytest.mark.parametrize("pwl", [False, True], ids=["clamp-only", "piecewise-linear"])
def test_floors_of_zero_give_the_bits_of_the_search_without_floors(exe, exe_plain, pwl):
    rows = list(budget_rows(72, 31 + pwl, pwl=pwl))
    with_floor = _run(exe, [_line(steps, np.zeros(len(steps)), cap, lo, hi) for steps, cap, lo, hi in rows])
    plain = _run(exe_plain, [_line(steps, None, cap, lo, hi) for steps, cap, lo, hi in rows])
    assert with_floor == plain
