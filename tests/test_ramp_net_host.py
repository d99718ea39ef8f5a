"""csrc/ramp_dp.h as a host program (the pattern of tests/test_plan_chain.py): the header has no HIP include, so
tests/ramp_net_main.cpp — its own main, that header and dopf_plan.h only — is built with g++ under the address and
undefined-behaviour sanitizers and fed seeded rows as hexadecimal doubles; the routine a lane of k_gen_ramp_net runs must give the
bits of helpers_ramp_net.ramp_project_pwl. Tolerance 0: the two are the same statements in the same order over IEEE doubles, and the
program is built with -ffp-contract=off, so no multiply-add is fused on the host. The knots live in heap arrays of exactly K
doubles: with K below a row's need the routine must return false with the output row untouched, and a write beyond K would be the
sanitizer's report (stderr must stay empty)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers_ramp_net import pwl_cases, ramp_project_pwl

CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rampnet") / "ramp_net")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "ramp_net_main.cpp"), "-o", out], check=True)
    return out


def _hex(values):
    return " ".join(float(v).hex() for v in values)


def _line(steps, cap, up, down, prev, K):
    """the request of one row; the ramps capped as ramp_project_pwl caps them (the routine takes finite ramps)"""
    pm = float(np.max(cap)) if prev is None else max(float(np.max(cap)), float(prev))
    head = f"row {len(steps)} {K} {_hex([min(float(up), pm), min(float(down), pm)])} {'nan' if prev is None else float(prev).hex()}"
    body = " ".join(f"{float(c).hex()} {len(sl) - 1} {_hex(xk)} {_hex(vk)} {_hex(sl)}" for c, (xk, vk, sl) in zip(cap, steps))
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


def test_the_host_build_gives_the_bits_of_ramp_project_pwl(exe):
    rows = list(pwl_cases(260, 21))
    want, need = [], []
    for steps, cap, up, down, prev in rows:
        info = {}
        want.append(ramp_project_pwl(steps, cap, up, down, prev, info))
        need.append(info["most"])
    got = _run(exe, [_line(*row, 2 * len(row[0]) + 2 + sum(len(s[2]) - 1 for s in row[0])) for row in rows])
    differ = [i for i, ((ok, guard, x), w) in enumerate(zip(got, want)) if not ok or not np.array_equal(x, w)]
    assert not differ, (len(differ), differ[:5])
    assert sum(n > 2 * len(r[0]) + 2 for n, r in zip(need, rows)) >= 20                  # rows beyond the copper-plate bound 2T + 2
    print(f"{len(rows)} rows bit for bit; largest knot count {max(need)}")


def test_a_small_capacity_is_refused_without_a_write_beyond_it(exe):
    rows = list(pwl_cases(120, 22))
    need = []
    for steps, cap, up, down, prev in rows:
        info = {}
        ramp_project_pwl(steps, cap, up, down, prev, info)
        need.append(info["most"])
    exact = _run(exe, [_line(*row, n) for row, n in zip(rows, need)])                    # K at the need: still the answer
    for (ok, guard, x), row in zip(exact, rows):
        assert ok and np.array_equal(x, ramp_project_pwl(*row))
    for less in (1, 2):                                                                  # one and two below: false, the row untouched
        short = _run(exe, [_line(*row, max(n - less, 0)) for row, n in zip(rows, need)])
        for (ok, guard, x), row in zip(short, rows):
            assert not ok and guard and np.array_equal(x, -1.0 - np.arange(len(row[0])))
    tiny = _run(exe, [_line(*row, k) for row in rows[:20] for k in (0, 1, 2, 3)])
    assert all(guard or ok for ok, guard, x in tiny)
