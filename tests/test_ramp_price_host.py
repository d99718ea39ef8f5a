"""csrc/ramp_price.h on the CPU: the NumPy twin helpers_ramp_price.ramp_multipliers against the certificate
(stationarity with a correctly signed box multiplier, the signs of a_t, a_t = 0 off tight rows) and against the duals of an
independent dense QP, and tests/ramp_price_main.cpp — its own main, that header only — built with g++ under the address and
undefined-behaviour sanitizers, which must give the twin's bits: the same statements in the same order over IEEE doubles, built with
-ffp-contract=off."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers_min_output import floor_cases, ramp_project_floor
from helpers_ramp_net import line_step
from helpers_ramp_price import long_rows, priced_row, qp_ramp_duals, ramp_multipliers, ramp_price_violation, tied

CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
BOUND = 1e-9            # the project's one-step bound, carried to the price's unit (q max(1, max cap))
QP_SIGN = -1.0          # a_t = QP_SIGN * y_t of the oracle's qp_solve (test_the_sign_of_the_qps_duals_on_a_hand_case settles it)


def _seeded():
    rows = [r for seed in (1, 2, 3) for r in floor_cases(400, seed, 12)]
    rows += [r for T, seed in ((64, 11), (65, 12), (130, 13)) for r in long_rows(T, 8, seed)]
    return rows


@pytest.fixture(scope="module")
def seeded():
    rows = _seeded()
    return rows, [priced_row(r) for r in rows]


def test_the_twins_prices_pass_the_certificate(seeded):
    rows, priced = seeded
    worst, n_priced, pos, neg = 0.0, 0, 0, 0
    for (c, q, lo, cap, up, down, prev), (x, a) in zip(rows, priced):
        v = ramp_price_violation(x, c, q, lo, cap, up, down, prev, a)
        assert v <= BOUND, (len(c), v)
        worst = max(worst, v)
        n_priced += bool(np.any(a != 0.0))
        pos, neg = pos + bool(np.any(a > 0.0)), neg + bool(np.any(a < 0.0))
    print(f"{len(rows)} rows, {n_priced} priced ({pos} with a > 0, {neg} with a < 0), worst violation {worst:.1e}")
    assert 3 * n_priced >= len(rows) and pos > 0 and neg > 0, (len(rows), n_priced, pos, neg)
    assert {64, 65, 130} <= {len(r[0]) for r in rows}


def test_the_certificate_refuses_wrong_prices(seeded):
    """the certificate is no rubber stamp: a priced row with its prices zeroed, negated or moved by 1e-6 of q max cap fails it"""
    rows, priced = seeded
    seen = 0
    for (c, q, lo, cap, up, down, prev), (x, a) in zip(rows, priced):
        if not np.any(a != 0.0) or tied(x, lo, cap, up, down, prev):
            continue
        seen += 1
        big = 1e-6 * q * max(1.0, float(cap.max()))
        for wrong in (np.zeros_like(a), -a, a + big * (a != 0.0)):
            if np.abs(wrong - a).max() <= 100.0 * BOUND * q * max(1.0, float(cap.max())):
                continue
            assert ramp_price_violation(x, c, q, lo, cap, up, down, prev, wrong) > BOUND
    assert seen >= 100, seen


def test_the_sign_of_the_qps_duals_on_a_hand_case(oracle_api):
    """q = 1, c = (0, 10), box [0, 100], up = 2, no anchor: x = (4, 6), g = (4, -4), so a_1 = 4 > 0 — ramp-up holds the row back"""
    c, q, lo, cap = np.array([0.0, 10.0]), 1.0, np.zeros(2), np.full(2, 100.0)
    x = ramp_project_floor(c, q, lo, cap, 2.0, np.inf, None)
    assert np.array_equal(x, [4.0, 6.0])
    a = ramp_multipliers(x, c, q, lo, cap, 2.0, np.inf, None)
    assert np.array_equal(a, [0.0, 4.0])
    xq, y = qp_ramp_duals(oracle_api, [line_step(q, ct) for ct in c], lo, cap, 2.0, np.inf, None)
    assert np.abs(xq - x).max() <= 1e-9 * 100.0
    assert abs(QP_SIGN * y[1] - 4.0) <= 1e-9 * 100.0, y
    # ... and ramp-down: the mirror image
    c2 = np.array([10.0, 0.0])
    x2 = ramp_project_floor(c2, q, lo, cap, np.inf, 2.0, None)
    a2 = ramp_multipliers(x2, c2, q, lo, cap, np.inf, 2.0, None)
    assert np.array_equal(x2, [6.0, 4.0]) and np.array_equal(a2, [0.0, -4.0])
    _, y2 = qp_ramp_duals(oracle_api, [line_step(q, ct) for ct in c2], lo, cap, np.inf, 2.0, None)
    assert abs(QP_SIGN * y2[1] + 4.0) <= 1e-9 * 100.0, y2


def test_the_twin_equals_the_dense_qps_duals_where_they_are_unique(oracle_api):
    """On the rows of floor_cases(400, seed, 12), seeds 1..3, with no step on a box end and a ramp reach at once, the twin's prices
    equal the multipliers the oracle's qp_solve puts on the QP's ramp equalities within the bound tests/test_gen_min_output_abi.py
    uses for that solver's primal, 1e-9 max(1, max cap), times q."""
    n = priced = 0
    worst = 0.0
    for seed in (1, 2, 3):
        for c, q, lo, cap, up, down, prev in floor_cases(400, seed, 12):
            x = ramp_project_floor(c, q, lo, cap, up, down, prev)
            if tied(x, lo, cap, up, down, prev):
                continue
            a = ramp_multipliers(x, c, q, lo, cap, up, down, prev)
            xq, y = qp_ramp_duals(oracle_api, [line_step(q, ct) for ct in c], lo, cap, up, down, prev)
            size = max(1.0, float(cap.max()))
            assert np.abs(xq - x).max() <= 1e-9 * size
            err = float(np.abs(a - QP_SIGN * y).max()) / (q * size)
            worst = max(worst, err)
            assert err <= BOUND, (seed, n, err, a, y)
            n += 1
            priced += bool(np.any(a != 0.0))
    print(f"{n} rows with unique multipliers against the QP's duals, {priced} priced, worst {worst:.1e} of q max cap")
    assert n >= 600 and priced >= 100, (n, priced)


# ---- the header as a host program ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rampprice") / "ramp_price")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "ramp_price_main.cpp"), "-o", out], check=True)
    return out


def _h(v):
    return float(v).hex()


def _line(kind, x, c, q, lo, cap, up, down, prev, shift=0.0):
    T = len(x)
    cap, lo = np.broadcast_to(cap, (T,)), np.broadcast_to(lo, (T,))
    head = f"{kind} {T} {_h(shift)} {_h(q)} {_h(up)} {_h(down)} {'nan' if prev is None else _h(prev)} {_h(cap.max()) if T else _h(1.0)}"
    return head + "".join(f" {_h(x[t])} {_h(c[t])} {_h(lo[t])} {_h(cap[t])}" for t in range(T)) + "\n"


def _run(exe, lines):
    r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])          # (a sanitizer report lands here)
    out = [np.array([float.fromhex(v) for v in ln.split()[1:]]) for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def test_the_host_build_gives_the_twins_bits(exe, seeded):
    rows, priced = seeded
    got = _run(exe, [_line("row", x, c, q, lo, cap, up, down, prev) for (c, q, lo, cap, up, down, prev), (x, a) in zip(rows, priced)])
    differ = [i for i, (g, (x, a)) in enumerate(zip(got, priced)) if not np.array_equal(g, a)]
    assert not differ, (len(differ), differ[:5])
    alias = _run(exe, [_line("alias", x, c, q, lo, cap, up, down, prev) for (c, q, lo, cap, up, down, prev), (x, a) in zip(rows, priced)])
    assert all(np.array_equal(g, a) for g, (x, a) in zip(alias, priced))                 # in place over the centres: the same bits
    print(f"{len(rows)} rows bit for bit, {sum(bool(np.any(a != 0.0)) for x, a in priced)} priced")


def test_the_host_build_under_a_shift(exe, seeded):
    """shift = nu / q (the pair's rows): the row projected from c - shift, priced with the centres c and the shift"""
    rows, _ = seeded
    lines, want = [], []
    for k, (c, q, lo, cap, up, down, prev) in enumerate(rows[:300]):
        shift = (0.3 if k % 2 else -0.2) * float(np.max(cap))
        x = ramp_project_floor(c - shift, q, lo, cap, up, down, prev)
        a = ramp_multipliers(x, c, q, lo, cap, up, down, prev, shift=shift)
        assert ramp_price_violation(x, c, q, lo, cap, up, down, prev, a, shift=shift) <= BOUND
        lines.append(_line("row", x, c, q, lo, cap, up, down, prev, shift))
        want.append(a)
    got = _run(exe, lines)
    assert all(np.array_equal(g, a) for g, a in zip(got, want))
