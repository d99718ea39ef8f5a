"""csrc/central_rows.h on the CPU (the pattern of tests/test_ramp_net_host.py). The header has no HIP include, so
tests/central_rows_main.cpp — its own main around that header alone — is built with g++ under the address and undefined-behaviour
sanitizers and fed seeded generator rows as hexadecimal doubles; what it prints must be the bits of the NumPy twin in
helpers_central_coupled.py. Tolerance 0: the two are the same statements in the same order over IEEE doubles, and the program is built
with -ffp-contract=off, so no multiply-add is fused on the host. stderr must stay empty (a sanitizer report lands there).

Then the whole primal-dual iteration in NumPy (helpers_central_coupled.pdhg: the device's step sizes and restart scheme) against
HiGHS: the signs and step sizes of the ramp and budget rows, checked before any GPU run."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg
from decentralopf_jl_amd import synth
from decentralopf_jl_amd.central import solve_central_packed
from helpers_central_coupled import draw_inputs, pdhg, row_metrics, row_step

CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
INF, NAN = np.inf, np.nan


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("centralrows") / "central_rows")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "central_rows_main.cpp"), "-o", out], check=True)
    return out


def _hex(values):
    return " ".join(float(v).hex() for v in np.atleast_1d(values))


def rows(n, seed):
    """Seeded rows: (T, mc, absH, w, ru, rd, prev, e_min, e_max, yQ, pi, cap, x0, yR). Every third has one-sided ramps, some have no
    rows at all, the multipliers are 0 on a share of the slots, and the fixed ones in front hold the corners."""
    rng = np.random.default_rng(seed)
    z = np.zeros
    out = [
        (1, 3.0, 0.0, 1.0, 2.0, 1.0, 5.0, 0.0, INF, 0.0, z(1) - 4.0, z(1) + 9.0, z(1) + 5.0, z(1)),            # T = 1 with an anchor
        (1, 3.0, 0.5, 1.0, INF, INF, 5.0, 0.0, INF, 0.0, z(1) - 4.0, z(1) + 9.0, z(1) + 5.0, z(1) + 0.25),     # ... whose row is free
        (1, 3.0, 0.0, 2.0, INF, INF, NAN, 4.0, 4.0, -1.5, z(1) - 4.0, z(1) + 9.0, z(1) + 5.0, z(1)),           # e_min = e_max, T = 1
        (5, 2.0, 1.5, 1.0, INF, INF, NAN, 7.0, 7.0, 0.0, z(5) - 3.0, z(5) + 4.0, z(5) + 1.0, z(5)),            # e_min = e_max, y = 0
        (5, 2.0, 1.5, 1.0, INF, 0.5, NAN, 0.0, 6.0, 0.0, np.array([-9.0, 0, -9, 0, -9]), z(5) + 4.0, z(5), z(5)),      # one-sided, y = 0
        (5, 2.0, 1.5, 1.0, 0.5, INF, 1.0, 2.0, INF, 0.0, np.array([-9.0, 0, -9, 0, -9]), z(5) + 4.0, z(5), z(5)),      # the other side
        (4, 1.0, 0.0, 1.0, 0.0, 0.0, 2.0, 0.0, INF, 0.0, z(4) - 5.0, z(4) + 4.0, z(4) + 2.0, z(4)),            # ramps of 0: a pinned row
    ]
    for i in range(n):
        T = int(rng.choice([1, 2, 3, 7, 24, 65, 130]))
        cap = rng.uniform(0.0, 50.0, T) * (rng.random(T) > 0.1)
        ru, rd = rng.uniform(0.0, 20.0, 2)
        if i % 3 == 0:
            ru = INF
        elif i % 3 == 1 and i % 2 == 0:
            rd = INF
        if i % 7 == 0:
            ru = rd = INF
        prev = float(rng.uniform(0.0, 50.0)) if i % 2 else NAN
        e_min = float(rng.uniform(0.0, 10.0 * T)) if i % 4 == 0 else 0.0
        e_max = e_min + float(rng.uniform(0.0, 10.0 * T)) if i % 5 < 2 else INF
        if i % 11 == 0:
            e_max = e_min
        ramp = np.isfinite(ru) or np.isfinite(rd) or prev == prev
        yR = rng.normal(0.0, 5.0, T) * (rng.random(T) > 0.4) * ramp
        if ru == INF:
            yR = np.minimum(yR, 0.0)          # (what the iteration keeps: no positive multiplier on a row without an upper end)
        if rd == INF:
            yR = np.maximum(yR, 0.0)
        if prev != prev:
            yR[0] = 0.0
        yQ = float(rng.normal(0.0, 5.0)) * (i % 3 != 2) * bool(e_min > 0.0 or e_max < INF)
        if e_max == INF:
            yQ = min(yQ, 0.0)
        out.append((T, float(rng.uniform(0.0, 60.0)), float(rng.uniform(0.0, 3.0)), float(rng.choice([1.0, 0.5, 3.0])), float(ru), float(rd),
                    prev, e_min, e_max, yQ, rng.normal(-30.0, 30.0, T), cap, rng.uniform(0.0, 1.0, T) * cap, yR))
    return out


def _word(v):
    return "nan" if v != v else float(v).hex()


def _run(exe, lines):
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    out = [ln.split() for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return [(f[0], np.array([float.fromhex(v) for v in f[1:]])) for f in out]


def test_the_host_build_gives_the_bits_of_the_numpy_twin(exe):
    cases = rows(300, 5)
    lines = []
    for T, mc, absH, w, ru, rd, prev, e_min, e_max, yQ, pi, cap, x0, yR in cases:
        tail = f"{_hex(pi)} {_hex(cap)} {_hex(x0)} {_hex(yR)}\n"
        lines.append(f"step {T} {_hex([mc, absH, w, ru, rd])} {_word(prev)} {_hex([e_min, e_max, yQ])} {tail}")
        lines.append(f"metrics {T} {_hex([mc, ru, rd])} {_word(prev)} {_hex([e_min, e_max, yQ])} {tail}")
    got = _run(exe, lines)
    differ, moved = [], 0
    for i, (T, mc, absH, w, ru, rd, prev, e_min, e_max, yQ, pi, cap, x0, yR) in enumerate(cases):
        xn, yRn, yQn = row_step(mc, absH, w, ru, rd, prev, e_min, e_max, pi, cap, x0, yR, yQ)
        want = np.concatenate([xn, yRn, [yQn]])
        kind, have = got[2 * i]
        if kind != "step" or not np.array_equal(have, want):
            differ.append(("step", i))
        moved += int(np.any(yRn != 0.0)) + int(yQn != 0.0)
        kind, have = got[2 * i + 1]
        want = np.array(row_metrics(mc, ru, rd, prev, e_min, e_max, pi, cap, x0, yR, yQ))
        assert not np.any(np.isnan(want)), (i, want)          # (one-sided rows: no 0 * inf in the support term)
        if kind != "metrics" or not np.array_equal(have, want):
            differ.append(("metrics", i))
    assert not differ, (len(differ), differ[:6])
    assert moved >= 100          # (the rows' proximal steps are exercised, not only their zeros)
    print(f"{len(cases)} rows bit for bit")


def test_a_row_inside_its_interval_gets_a_multiplier_of_exactly_zero():
    """what the dual objective needs of a one-sided row: never a rounding error of the wrong sign times an infinite end"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        T = 6
        cap = rng.uniform(1.0, 9.0, T)
        x0 = rng.uniform(0.0, 1.0, T) * cap
        xn, yRn, yQn = row_step(0.0, 0.3, 1.0, INF, 100.0, NAN, 0.0, 1e6, np.zeros(T), cap, x0, np.zeros(T), 0.0)
        assert np.all(yRn == 0.0) and yQn == 0.0
        cost, rct, sup, viol = row_metrics(0.0, INF, 100.0, NAN, 0.0, 1e6, np.zeros(T), cap, xn, yRn, yQn)
        assert sup == 0.0 and viol == 0.0


# ---- the whole iteration against HiGHS -----------------------------------------------------------------------------------------------
def _three_node_inputs(pp):
    """tests/test_gen_budget_abi.py's budgets (generator 2 at most 300, generator 3 in [20, 150]) plus a ramp that makes them bind"""
    G = pp.G
    lo, hi = np.zeros(G), np.full(G, INF)
    hi[2] = 300.0
    lo[3], hi[3] = 20.0, 150.0
    up, dn = np.full(G, INF), np.full(G, INF)
    up[2] = dn[2] = 150.0
    dn[0] = 2.0
    return dict(gen_ramp=(up, dn), gen_budget=(lo, hi))


def test_numpy_iteration_reaches_highs_on_the_three_node_case(three_node):
    pp = three_node[4]
    base = solve_central_packed(pp, duals=False).objective
    kw = _three_node_inputs(pp)
    prev = np.maximum(solve_central_packed(pp, duals=False, gen_ramp=kw["gen_ramp"]).generation[:, 0] - 30.0, 0.0)
    for extra in (dict(), dict(gen_prev=prev)):
        want = solve_central_packed(pp, duals=False, **kw, **extra).objective
        assert abs(want - base) > 1e-3 * base          # (the rows bind)
        r = pdhg(pp, tol=1e-9, **kw, **extra)
        print(f"three-node {sorted(extra)}: host {want!r} numpy {r['objective']!r} dual {r['dual_objective']!r} iterations {r['iterations']}")
        assert r["converged"]
        assert abs(r["objective"] - want) <= 1e-6 * abs(want) and abs(r["dual_objective"] - want) <= 1e-6 * abs(want)


def test_numpy_iteration_reaches_highs_on_a_drawn_case():
    pp = synth.synthetic_case(8, 2, 6, seed=3)
    d = draw_inputs(pp, lambda q, **kw: solve_central_packed(q, duals=False, **kw))
    base = solve_central_packed(pp, duals=False).objective
    for name, kw in (("ramp", dict(gen_ramp=d["ramp"])), ("ramp+prev", dict(gen_ramp=d["ramp"], gen_prev=d["prev"])),
                     ("budget", dict(gen_budget=d["budget"])),
                     ("both", dict(gen_ramp=d["ramp"], gen_prev=d["prev"], gen_budget=d["budget"]))):
        want = solve_central_packed(pp, duals=False, **kw).objective
        assert abs(want - base) > 1e-4 * base
        r = pdhg(pp, tol=1e-9, **kw)
        print(f"{name}: host {want!r} numpy {r['objective']!r} dual {r['dual_objective']!r} iterations {r['iterations']}")
        assert r["converged"]
        assert abs(r["objective"] - want) <= 1e-6 * abs(want) and abs(r["dual_objective"] - want) <= 1e-6 * abs(want)
