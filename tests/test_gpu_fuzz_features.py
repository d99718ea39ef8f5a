"""Bounded, seeded slices of the two fuzzers of the later features in guard mode (DOPF_GUARD=1: every device array of the library
ends on the last bytes of its own mapping, so an access past an array's end is a fault that names it): scripts/fuzz_lossy_rated.py
(storage efficiencies and line ratings against the oracle) and scripts/fuzz_gen_coupling.py (quadratic costs, ramps on plates and
networks, energy budgets, ramps with budgets, must-run floors and budgets per sub-window, with the budget and ramp prices recorded in
every second case: rows against the NumPy references, the prices against their certificates and NumPy twins, the whole state against
a forced-step oracle twin, iterate(n) against single steps, shards against one context). Each slice runs in a fresh child process with fixed seeds, as
tests/test_gpu_fuzz.py's do, and passes when the script exits 0 and reports `bad 0` with no MISMATCH and no SOLVER FAILURES line.
tests/test_fuzz_reference_only.py settles on the CPU that the coupling slices' first steps leave and keep the kernels' fast paths
often enough."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# script, families (fuzz_gen_coupling's --families), cases, seed, seconds measured on an MI355X (library load included)
SLICES = [
    ("fuzz_lossy_rated", None, 30, 431, 5.2),
    ("fuzz_gen_coupling", "c2", 12, 456, 2.1),
    ("fuzz_gen_coupling", "ramp-plate", 12, 442, 4.6),
    ("fuzz_gen_coupling", "ramp-net", 12, 443, 4.3),
    ("fuzz_gen_coupling", "budget-plate", 12, 444, 3.6),
    ("fuzz_gen_coupling", "budget-net", 12, 445, 6.1),
    ("fuzz_gen_coupling", "pair", 4, 446, 8.0),            # (the pair's twelve cases in three slices: its reference bisects)
    ("fuzz_gen_coupling", "pair", 4, 447, 6.5),
    ("fuzz_gen_coupling", "pair", 4, 448, 9.1),
    ("fuzz_gen_coupling", "ramp-plate", 12, 500, 4.3),     # (ramp prices at T = 1, 2 and 127..130, which seed 442 does not draw)
    ("fuzz_gen_coupling", "floor-plate", 12, 549, 5.5),
    ("fuzz_gen_coupling", "floor-net", 12, 500, 3.3),
    ("fuzz_gen_coupling", "window-plate", 12, 500, 4.0),
    ("fuzz_gen_coupling", "window-net", 12, 501, 3.4),
]
COUPLING = [s for s in SLICES if s[0] == "fuzz_gen_coupling"]


def slice_command(script, families, n, seed, *more):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", script + ".py"), str(n), str(seed)]
    return cmd + ([f"--families={families}"] if families else []) + list(more)


def check_output(r, what):
    """exit status 0, a `done:` line with `bad 0`, no MISMATCH, no SOLVER FAILURES; returns the stdout"""
    tail = (r.stdout or "")[-1500:] + (r.stderr or "")[-1500:]
    assert r.returncode == 0, f"{what}\n{tail}"
    done = [l for l in r.stdout.splitlines() if l.startswith("done:")]
    assert done, tail
    assert "MISMATCH" not in r.stdout and "SOLVER FAILURES" not in r.stdout, tail
    m = re.search(r"bad (\d+)", done[-1])
    assert m and int(m.group(1)) == 0, done[-1]
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("script,families,n,seed,seconds", SLICES, ids=[f"{s[0]}-{s[1] or 'all'}-{s[3]}" for s in SLICES])
def test_fuzz_slice_in_guard_mode(script, families, n, seed, seconds):
    r = subprocess.run(slice_command(script, families, n, seed), cwd=ROOT, capture_output=True, text=True,
                       timeout=max(60, 10 * seconds), env=dict(os.environ, DOPF_GUARD="1"))
    check_output(r, f"{script} {families or ''} {n} {seed}")
