"""scripts/fuzz_gen_coupling.py --reference-only on the seeds of the GPU suite's slices (tests/test_gpu_fuzz_features.py), on the
CPU: the oracle warm-up, the draws and the NumPy references of each case's first compared step, and the forced-step oracle twin
("The forced-step twin") against a plain oracle step. Two things are asserted: the twin reproduces the plain step on
every case, and the slices' first steps exercise the kernels — in every constrained family at least a fifth of the rows leave the
fast path (active ramp, binding budget, both for the pair) and at least a fifth stay on it, the `5 * active >= G and 5 * free >= G`
of the fixed-shape tests; the c2 family has at least a quarter of its (g, t) strictly inside the box."""
import re
import subprocess

import pytest

from test_gpu_fuzz_features import COUPLING, ROOT, check_output, slice_command

CONSTRAINED = ("ramp-plate", "ramp-net", "budget-plate", "budget-net", "pair")


@pytest.fixture(scope="module")
def coverage():
    """family -> [rows, leave, stay] over the slices (one child process per slice: the script runs as the GPU slices run it); the
    script itself counts a case whose twin misses 1e-11 scaled, or whose P is not the plain step's to 1e-12 relative, as bad"""
    total = {}
    for script, families, n, seed, _ in COUPLING:
        r = subprocess.run(slice_command(script, families, n, seed, "--reference-only"), cwd=ROOT, capture_output=True, text=True,
                           timeout=600)
        out = check_output(r, f"{families} {n} {seed}")
        worst = float(re.search(r"worst relative difference (\S+),", out.splitlines()[-1]).group(1))
        assert worst <= 1e-11, (families, seed, worst)
        for fam, rows, leave, stay in re.findall(r"^coverage (\S+): rows (\d+) leave (\d+) stay (\d+)$", out, re.M):
            t = total.setdefault(fam, [0, 0, 0])
            for i, v in enumerate((rows, leave, stay)):
                t[i] += int(v)
    for fam, (rows, leave, stay) in total.items():
        print(f"{fam}: rows compared {rows}, leave the fast path {leave}, stay on it {stay}")
    return total


def test_the_twin_reproduces_a_plain_oracle_step_on_every_family(coverage):
    assert set(coverage) == set(CONSTRAINED) | {"c2"}, sorted(coverage)


@pytest.mark.parametrize("family", CONSTRAINED)
def test_first_steps_leave_and_keep_the_fast_path(coverage, family):
    rows, leave, stay = coverage[family]
    assert rows > 0 and 5 * leave >= rows and 5 * stay >= rows, (family, rows, leave, stay)


def test_a_quarter_of_the_c2_entries_are_inside_the_box(coverage):
    rows, inside, _ = coverage["c2"]
    assert rows > 0 and 4 * inside >= rows, (rows, inside)
