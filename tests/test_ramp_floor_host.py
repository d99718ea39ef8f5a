"""csrc/ramp_dp.h with floors as a host program (the pattern of tests/test_ramp_net_host.py): tests/ramp_floor_main.cpp
— its own main, that header only — is built with g++ under the address and undefined-behaviour sanitizers and fed seeded rows as
hexadecimal doubles; ramp_repair_pwl<true>, the routine a lane of k_gen_ramp_net<.., .., true> runs, must give the bits of
helpers_min_output.ramp_project_pwl_floor. Tolerance 0: the same statements in the same order over IEEE doubles, built with
-ffp-contract=off. The knots live in heap arrays of exactly K doubles: with K below a row's need the routine must return false with
the output row untouched, and a write beyond K would be the sanitizer's report (stderr must stay empty)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers_min_output import pwl_floor_cases, ramp_project_pwl_floor
from helpers_ramp_net import phi_at

CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rampfloor") / "ramp_floor")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "ramp_floor_main.cpp"), "-o", out], check=True)
    return out


def _hex(values):
    return " ".join(float(v).hex() for v in values)


def _line(steps, lo, cap, up, down, prev, K):
    """the request of one row; the ramps capped as ramp_project_pwl_floor caps them (the routine takes finite ramps)"""
    pm = float(np.max(cap)) if prev is None else max(float(np.max(cap)), float(prev))
    head = f"row {len(steps)} {K} {_hex([min(float(up), pm), min(float(down), pm)])} {'nan' if prev is None else float(prev).hex()}"
    body = " ".join(f"{float(f).hex()} {float(c).hex()} {len(sl) - 1} {_hex(xk)} {_hex(vk)} {_hex(sl)}"
                    for f, c, (xk, vk, sl) in zip(lo, cap, steps))
    return head + " " + body + "\n"


def _run(exe, lines):
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])          # (a sanitizer report lands here)
    out = []
    for ln in r.stdout.splitlines():
        f = ln.split()
        assert f[0] == "row"
        out.append((f[1] == "ok=1", f[2] == "guard=1", np.array([float.fromhex(v) for v in f[3:]])))
    assert len(out) == len(lines)
    return out


def _repaired(steps, lo, cap, x):
    """the row left the fast path: it is not the clamp of every step's own minimiser"""
    for st, f, c, v in zip(steps, lo, cap, x):
        g = phi_at(st, v)
        if not ((v == f and g >= 0.0) or (v == c and g <= 0.0) or abs(g) <= 1e-9 * max(1.0, abs(v))):
            return True
    return False


def test_the_host_build_gives_the_bits_of_ramp_project_pwl_floor(exe):
    rows = list(pwl_floor_cases(260, 41, tmax=24))
    want, need, floor_repairs = [], [], 0
    for steps, lo, cap, up, down, prev in rows:
        info = {}
        x = ramp_project_pwl_floor(steps, lo, cap, up, down, prev, info)
        want.append(x)
        need.append(info["most"])
        floor_repairs += info["on_floor"] and _repaired(steps, lo, cap, x)
    got = _run(exe, [_line(*row, 2 * len(row[0]) + 2 + sum(len(s[2]) - 1 for s in row[0])) for row in rows])
    differ = [i for i, ((ok, guard, x), w) in enumerate(zip(got, want)) if not ok or not np.array_equal(x, w)]
    assert not differ, (len(differ), differ[:5])
    assert len(rows) >= 200 and floor_repairs >= 40, (len(rows), floor_repairs)          # repairs that end on the floor somewhere
    print(f"{len(rows)} rows bit for bit, {floor_repairs} repaired onto their floor; largest knot count {max(need)}")


def test_a_small_capacity_is_refused_without_a_write_beyond_it(exe):
    rows = list(pwl_floor_cases(120, 42, tmax=24))
    need = []
    for row in rows:
        info = {}
        ramp_project_pwl_floor(*row, info)
        need.append(info["most"])
    exact = _run(exe, [_line(*row, n) for row, n in zip(rows, need)])                    # K at the need: still the answer
    for (ok, guard, x), row in zip(exact, rows):
        assert ok and np.array_equal(x, ramp_project_pwl_floor(*row))
    for less in (1, 2):                                                                  # one and two below: false, the row untouched
        short = _run(exe, [_line(*row, max(n - less, 0)) for row, n in zip(rows, need)])
        for (ok, guard, x), row in zip(short, rows):
            assert not ok and guard and np.array_equal(x, -1.0 - np.arange(len(row[0])))
    tiny = _run(exe, [_line(*row, k) for row in rows[:20] for k in (0, 1, 2, 3)])
    assert all(guard or ok for ok, guard, x in tiny)
