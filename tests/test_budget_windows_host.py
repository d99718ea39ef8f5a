"""csrc/budget_win_map.h with csrc/budget_root.h as a host program (the pattern of tests/test_budget_host.py): neither
header has a HIP include, so tests/budget_windows_main.cpp — its own main, those two headers only — is built with g++ under the address
and undefined-behaviour sanitizers (static runtimes) and fed seeded rows as hexadecimal doubles.

A row under one budget per sub-window is one budget_root search per window, over the window's timesteps alone: what a wave of
k_gen_budget_win runs for a (row, window) unit. Each must give helpers_budget.budget_project on the slice. Bound: 1e-9 times the row's
capacity, test_budget_host.py's. The unit mapping must enumerate every (row, window) exactly once, rows outermost."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers_budget import budget_project, budget_rows

CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
MAX_EVALS = 192                                        # kBudgetMaxEvals


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("budget_windows") / "budget_windows")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "budget_windows_main.cpp"), "-o", out], check=True)
    return out


def _run(exe, lines):
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])          # (a sanitizer report lands here)
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def _hex(values):
    return " ".join(float(v).hex() for v in values)


def _line(steps, cap, ends, lo, hi, max_evals=MAX_EVALS):
    body = " ".join(f"{float(c).hex()} {len(sl) - 1} {_hex(xk)} {_hex(vk)} {_hex(sl)}" for c, (xk, vk, sl) in zip(cap, steps))
    return f"row {len(steps)} {len(ends)} {max_evals} {' '.join(str(int(e)) for e in ends)} {_hex(lo)} {_hex(hi)} {body}\n"


def _window_budgets(steps, cap, ends, kind):
    """one budget per window by class (kind + j) % 6, budget_rows' classes on the window's own clamped-step sum and cap sum: binding
    above, binding below, an equality, e_max = 0, e_min = the window's sum of caps, free"""
    lo, hi = np.zeros(len(ends)), np.full(len(ends), np.inf)
    t0 = 0
    for j, t1 in enumerate(ends):
        s0 = float(np.sum(budget_project(steps[t0:t1], cap[t0:t1])))
        room = sum(float(c) for c in cap[t0:t1])          # (added in t order)
        k = (kind + j) % 6
        if k == 0:
            hi[j] = 0.6 * s0
        elif k == 1:
            lo[j] = s0 + 0.4 * (room - s0)
        elif k == 2:
            lo[j] = hi[j] = 0.8 * s0
        elif k == 3:
            hi[j] = 0.0
        elif k == 4:
            lo[j] = room
        t0 = t1
    return lo, hi


def _cuts(T, rng):
    """the cuts of a row of T steps: none; 1, 63, 1, 65 (T = 130); every step its own window; random"""
    out = [("none", [T])]
    if T == 130:
        out.append(("1-63-1-65", [1, 64, 65, 130]))
    if T > 1:
        out.append(("every-step", list(range(1, T + 1))))
        n = int(rng.integers(2, min(T, 9) + 1))
        out.append(("random", sorted(set(rng.choice(np.arange(1, T), size=n - 1, replace=False).tolist())) + [T]))
    return out


@pytest.mark.parametrize("pwl", [False, True], ids=["clamp-only", "piecewise-linear"])
def test_per_window_searches_give_the_reference_on_the_slices(exe, pwl):
    rng = np.random.default_rng(77 + pwl)
    cases, seen = [], set()
    for k, (steps, cap, lo, hi) in enumerate(budget_rows(120, 41 + pwl, pwl=pwl)):          # 2 x 120 = 240 rows over the two parametrisations
        for name, ends in _cuts(len(steps), rng):
            wl, wh = (np.array([lo]), np.array([hi])) if name == "none" else _window_budgets(steps, cap, ends, k)
            cases.append((steps, cap, ends, wl, wh))
            seen.add(name)
    assert seen == {"none", "1-63-1-65", "every-step", "random"}
    worst, sides, units = 0.0, [], 0
    for ln, (steps, cap, ends, wl, wh) in zip(_run(exe, [_line(*c) for c in cases]), cases):
        f = ln.split()
        assert f[0] == "row" and f[1] == "fails=0", f[:2]
        nu = np.array([float.fromhex(v) for v in f[2:2 + len(ends)]])
        x = np.array([float.fromhex(v) for v in f[2 + len(ends):]])
        scale = max(1.0, float(np.max(cap)))
        t0 = 0
        for j, t1 in enumerate(ends):
            info = {}
            want = budget_project(steps[t0:t1], cap[t0:t1], wl[j], wh[j], info)
            err = float(np.max(np.abs(x[t0:t1] - want))) / scale
            worst = max(worst, err)
            assert err <= 1e-9, (len(steps), ends, j, err)
            s = float(np.sum(x[t0:t1]))
            assert wl[j] - 1e-9 * scale * (t1 - t0) <= s <= wh[j] + 1e-9 * scale * (t1 - t0)
            assert info["side"] != 0 or nu[j] == 0.0
            assert info["side"] == 0 or nu[j] == 0.0 or (nu[j] > 0) == (info["side"] > 0)
            sides.append(info["side"])
            units += 1
            t0 = t1
    assert min(sides.count(s) for s in (-1, 0, 1)) >= units // 8
    print(f"{len(cases)} rows, {units} (row, window) units: worst difference {worst:.2e} of the capacity")


def test_a_unit_out_of_evaluations_keeps_its_clamped_step_in_its_window_alone(exe):
    rng = np.random.default_rng(5)
    done = 0
    for k, (steps, cap, lo, hi) in enumerate(budget_rows(36, 43)):
        if len(steps) != 130:
            continue
        ends = [1, 64, 65, 130]
        wl, wh = _window_budgets(steps, cap, ends, k)
        f = _run(exe, [_line(steps, cap, ends, wl, wh, 1)])[0].split()
        fails = int(f[1][6:])
        nu = np.array([float.fromhex(v) for v in f[2:6]])
        x = np.array([float.fromhex(v) for v in f[6:]])
        t0 = 0
        for j, t1 in enumerate(ends):
            if nu[j] == 0.0:          # free, kept or given up: the clamped step of that window, bit for bit
                assert np.array_equal(x[t0:t1], budget_project(steps[t0:t1], cap[t0:t1])), (k, j)
            else:                     # a neighbour that gave up changes nothing here (the first probe may end a search: saturated, one piece)
                want = budget_project(steps[t0:t1], cap[t0:t1], wl[j], wh[j])
                assert np.abs(x[t0:t1] - want).max() <= 1e-9 * max(1.0, float(np.max(cap))), (k, j)
            t0 = t1
        done += fails
    assert done >= 4


@pytest.mark.parametrize("rows", [1, 7, 8, 9, 300])
@pytest.mark.parametrize("n_win", [1, 2, 7, 130])
def test_the_mapping_enumerates_every_unit_once(exe, rows, n_win):
    T, a0 = 130, 11
    ends = [T] if n_win == 1 else sorted(np.random.default_rng(n_win).choice(np.arange(1, T), size=n_win - 1, replace=False).tolist()) + [T]
    f = _run(exe, [f"map {rows} {n_win} {a0} {' '.join(map(str, ends))}\n"])[0].split()
    assert f[0] == "map" and f[1] == f"units={rows * n_win}"
    units = np.array(f[2:], dtype=np.int64).reshape(rows * n_win, 4)
    want = [(a0 + r, j, 0 if j == 0 else ends[j - 1], ends[j]) for r in range(rows) for j in range(n_win)]          # rows outermost
    assert [tuple(u) for u in units.tolist()] == want
    assert len({(g, j) for g, j, _, _ in want}) == rows * n_win
    # the kernel's waves: wave w takes u = w, w + 8, ..: together every unit once
    taken = sorted(u for w in range(8) for u in range(w, rows * n_win, 8))
    assert taken == list(range(rows * n_win))
