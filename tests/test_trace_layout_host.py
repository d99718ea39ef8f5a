"""csrc/trace_layout.h on the CPU (the pattern of tests/test_central_rows_host.py). The header has no HIP include, so
tests/trace_layout_main.cpp — its own main around that header alone — is built with g++ under the address and undefined-behaviour
sanitizers; what it prints — slot sizes and section offsets for a list of shapes and every mask, and the ring arithmetic — must be
what the NumPy twin below gives. stderr must stay empty (a sanitizer report lands there)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
DUALS, CONSENSUS, PRIMAL = 1, 2, 4
SHAPES = [(3, 3, 2, 4, 1), (3, 3, 2, 4, 0), (3, 3, 2, 0, 1), (3, 0, 2, 4, 1), (3, 3, 5, 4, 1), (1, 0, 5, 3, 3), (1, 0, 1, 1, 1),
          (20, 30, 168, 60, 6)]
CAPS = [1, 2, 5, 64]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tracelayout") / "trace_layout")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-I" + CSRC, os.path.join(ROOT, "tests", "trace_layout_main.cpp"), "-o", out],
                   check=True)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return [ln.split() for ln in r.stdout.splitlines()]


def layout_twin(N, L, T, G, S, what):
    """(slot_bytes, offsets, lengths): the 64-byte row, then the selected sections in slot order, each on a 16-byte boundary"""
    full = np.array([T, L * T, L * T, N * T, L * T, L * T, L * T, G * T, S * T, S * T], dtype=np.int64)
    bit = np.array([DUALS] * 3 + [CONSENSUS] * 4 + [PRIMAL] * 3)
    n = np.where(bit & what, full, 0)
    padded = (n * 8 + 15) // 16 * 16
    off = 64 + np.concatenate([[0], np.cumsum(padded)[:-1]])
    return int(64 + padded.sum()), off, n


def test_slot_layout_is_the_numpy_twin(printed):
    lines = [f for f in printed if f[0] == "layout"]
    assert len(lines) == len(SHAPES) * 8
    seen = set()
    for f in lines:
        N, L, T, G, S, what = (int(x) for x in f[1:7])
        seen.add((N, L, T, G, S, what))
        slot, off, n = layout_twin(N, L, T, G, S, what)
        got_off, got_n = np.array(f[8::2], dtype=np.int64), np.array(f[9::2], dtype=np.int64)
        assert int(f[7]) == slot and np.array_equal(got_off, off) and np.array_equal(got_n, n), f
        assert slot % 16 == 0 and np.all(got_off % 16 == 0)
        # a section that is not selected, or empty (G, S or L = 0), has size 0 and takes no space
        full = [T, L * T, L * T, N * T, L * T, L * T, L * T, G * T, S * T, S * T]
        for k in range(10):
            selected = bool(what & (DUALS if k < 3 else CONSENSUS if k < 7 else PRIMAL))
            assert got_n[k] == (full[k] if selected else 0)
            nxt = got_off[k + 1] if k < 9 else slot
            assert nxt - got_off[k] >= 8 * got_n[k] and (got_n[k] > 0 or nxt == got_off[k])
        if what == 0:
            assert slot == 64
    assert seen == {s + (w,) for s in SHAPES for w in range(8)}


def test_ring_arithmetic(printed):
    lines = [f for f in printed if f[0] == "ring"]
    assert len(lines) == len(CAPS) * 6
    for f in lines:
        cap, rec, slot, held, oldest = (int(x) for x in f[1:])
        assert held == min(rec, cap)
        assert slot == ((rec - 1) % cap if rec else -1)
        # replay: write slots one by one and see which ring slot holds the oldest kept iteration
        ring = {}
        for i in range(rec):
            ring[i % cap] = i
        if rec:
            assert ring[slot] == rec - 1
            assert ring[oldest] == rec - held
            assert [ring[(oldest + i) % cap] for i in range(held)] == list(range(rec - held, rec))
        else:
            assert oldest == 0
    assert {(int(f[1]), int(f[2])) for f in lines} == {(c, r) for c in CAPS for r in (0, 1, c - 1, c, c + 1, 3 * c + 2)}
