"""csrc/central_long.h on the CPU (the pattern of tests/test_central_rows_host.py). The header has no HIP include, so
tests/central_long_main.cpp — its own main around that header alone — is built with g++ under the address and undefined-behaviour
sanitizers. For each horizon it prints, per tile and thread of the long sweeps (kc_sto_long, kc_gen_rows_long), the first owned
timestep, the live mask, the slot of T - 1 and the slot handed to the next tile; the NumPy twin below must match exactly, and every
t in [0, T) must be owned once, in order. stderr must stay empty (a sanitizer report lands there)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
THREADS, SLOTS = 256, 8
TILE = THREADS * SLOTS
HORIZONS = (1, 8, 2047, 2048, 2049, 4096, 4100, 8760)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("centrallong") / "central_long")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "central_long_main.cpp"), "-o", out], check=True)
    return out


def twin(T):
    """((tiles * 256, 6) rows of tile, thread, first, mask, last_slot, hand_slot; (tiles, last tile, last thread, last slot))"""
    tiles = -(-T // TILE)
    tile, th = np.divmod(np.arange(tiles * THREADS, dtype=np.int64), THREADS)
    first = tile * TILE + th * SLOTS
    t = first[:, None] + np.arange(SLOTS)[None, :]
    live = t < T
    mask = (live << np.arange(SLOTS)[None, :]).sum(axis=1)
    is_last = live & (t == T - 1)
    last = np.where(is_last.any(axis=1), is_last.argmax(axis=1), -1)
    hand = np.where((th == THREADS - 1) & (tile + 1 < tiles), SLOTS - 1, -1)
    return np.stack([tile, th, first, mask, last, hand], axis=1), (tiles, (T - 1) // TILE, ((T - 1) % TILE) // SLOTS, (T - 1) % SLOTS)


@pytest.fixture(scope="module")
def printed(exe):
    r = subprocess.run([exe] + [str(T) for T in HORIZONS], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    rows, closed = {T: [] for T in HORIZONS}, {}
    for ln in r.stdout.splitlines():
        f = ln.split()
        if f[0] == "tiles":
            closed[int(f[1])] = tuple(int(x) for x in f[2:])
        else:
            rows[int(f[0])].append([int(x) for x in f[1:]])
    return {T: np.array(rows[T], dtype=np.int64) for T in HORIZONS}, closed


@pytest.mark.parametrize("T", HORIZONS)
def test_the_host_build_prints_the_numpy_twins_tiling(printed, T):
    rows, closed = printed
    want, want_closed = twin(T)
    assert rows[T].shape == want.shape and np.array_equal(rows[T], want)
    assert closed[T] == want_closed


@pytest.mark.parametrize("T", HORIZONS)
def test_every_timestep_is_owned_once_and_in_order(printed, T):
    rows, closed = printed
    got = rows[T]
    owned = []
    for tile, th, first, mask, last, hand in got:
        ks = [k for k in range(SLOTS) if mask >> k & 1]
        assert ks == list(range(len(ks)))                               # a thread's live slots are a prefix of its eight
        owned.extend(first + k for k in ks)
    assert owned == list(range(T))
    # T - 1: one slot, the one the closed forms name, and it is that thread's last live slot
    at = np.flatnonzero(got[:, 4] >= 0)
    assert at.size == 1
    tile, th, first, mask, last, hand = got[at[0]]
    assert (tile, th, last) == closed[T][1:] and first + last == T - 1 and mask == (1 << (last + 1)) - 1
    # hand-over: the last slot of the last thread of every tile but the last one, live, and followed by the next tile's first step
    hands = got[got[:, 5] >= 0]
    assert hands.shape[0] == closed[T][0] - 1
    for tile, th, first, mask, last, hand in hands:
        assert th == THREADS - 1 and hand == SLOTS - 1 and mask == 255
        nxt = got[(got[:, 0] == tile + 1) & (got[:, 1] == 0)][0]
        assert nxt[2] == first + hand + 1 and nxt[3] & 1
