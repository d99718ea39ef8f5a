"""scripts/fuzz_gen_coupling.py --reference-only on the seeds of the GPU suite's slices (tests/test_gpu_fuzz_features.py), on the
CPU: the oracle warm-up, the draws and the NumPy references of each case's first compared step, and the forced-step oracle twin
("The forced-step twin") against a plain oracle step. Two things are asserted: the twin reproduces the plain step on
every case, and the slices' first steps exercise the kernels — in every constrained family at least a fifth of the rows leave the
fast path (active ramp, binding budget, both for the pair; a floor row: it touches a floor above 0; the window families count their
(row, window) units) and at least a fifth stay on it, the `5 * active >= G and 5 * free >= G` of the fixed-shape tests; the c2 family
has at least a quarter of its (g, t) strictly inside the box. Of the floor rows at least a tenth touch their floor and leave it; of
the windows' units at least a fifth bind above and a fifth below; where ramp prices are drawn the NumPy twin prices at least a
quarter of the reference's rows, with both signs, and some priced case has no anchor, some T in {127, 128, 129, 130} and some T in
{1, 2}; where budget prices are drawn the leave/stay rule holds on the priced cases alone and both sides bind. These conditions
stand as they are: a slice that misses one gets other seeds or more cases, here on the CPU."""
import re
import subprocess

import pytest

from test_gpu_fuzz_features import COUPLING, ROOT, check_output, slice_command

CONSTRAINED = ("ramp-plate", "ramp-net", "budget-plate", "budget-net", "pair", "floor-plate", "floor-net", "window-plate", "window-net")
FLOORS = ("floor-plate", "floor-net")
WINDOWS = ("window-plate", "window-net")
RAMP_PRICED = ("ramp-plate", "floor-plate", "pair")
BUDGET_PRICED = ("budget-plate", "budget-net", "pair")


@pytest.fixture(scope="module")
def runs():
    """(family -> [rows, leave, stay], (line, family) -> {counter: sum}) over the slices (one child process per slice: the script runs as the GPU slices run it); the
    script itself counts a case whose twin misses 1e-11 scaled, or whose P is not the plain step's to 1e-12 relative, as bad"""
    total, more = {}, {}
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
        for name, fam, rest in re.findall(r"^(floors|windows|ramp-priced|budget-priced) (\S+): (.*)$", out, re.M):
            t = more.setdefault((name, fam), {})
            for key, v in re.findall(r"(\w+) (\d+)", rest):
                t[key] = t.get(key, 0) + int(v)
    for fam, (rows, leave, stay) in total.items():
        print(f"{fam}: rows compared {rows}, leave the fast path {leave}, stay on it {stay}")
    for (name, fam), t in sorted(more.items()):
        print(f"{name} {fam}: {t}")
    return total, more


@pytest.fixture(scope="module")
def coverage(runs):
    return runs[0]


@pytest.fixture(scope="module")
def more(runs):
    """the lines of the later features: ("floors" | "windows" | "ramp-priced" | "budget-priced", family) -> {counter: sum}"""
    return runs[1]


def test_the_twin_reproduces_a_plain_oracle_step_on_every_family(coverage):
    assert set(coverage) == set(CONSTRAINED) | {"c2"}, sorted(coverage)


@pytest.mark.parametrize("family", CONSTRAINED)
def test_first_steps_leave_and_keep_the_fast_path(coverage, family):
    rows, leave, stay = coverage[family]
    assert rows > 0 and 5 * leave >= rows and 5 * stay >= rows, (family, rows, leave, stay)


def test_a_quarter_of_the_c2_entries_are_inside_the_box(coverage):
    rows, inside, _ = coverage["c2"]
    assert rows > 0 and 4 * inside >= rows, (rows, inside)


@pytest.mark.parametrize("family", FLOORS)
def test_floor_rows_touch_their_floor_stay_off_it_and_do_both(more, family):
    t = more[("floors", family)]
    assert t["rows"] > 0 and 5 * t["touch"] >= t["rows"] and 5 * t["never"] >= t["rows"] and 10 * t["both"] >= t["rows"], (family, t)


@pytest.mark.parametrize("family", WINDOWS)
def test_window_units_bind_above_bind_below_and_are_free(more, family):
    t = more[("windows", family)]
    n = t["units"]
    assert n > 0 and 5 * t["above"] >= n and 5 * t["below"] >= n and 5 * t["free"] >= n, (family, t)


@pytest.mark.parametrize("family", RAMP_PRICED)
def test_ramp_priced_cases_price_rows_with_both_signs_at_the_edges(more, family):
    t = more[("ramp-priced", family)]
    assert t["rows"] > 0 and 4 * t["priced"] >= t["rows"] and t["positive"] >= 1 and t["negative"] >= 1, (family, t)
    assert t["no_anchor"] >= 1 and t["long_edge"] >= 1 and t["short_edge"] >= 1, (family, t)


@pytest.mark.parametrize("family", BUDGET_PRICED)
def test_budget_priced_cases_leave_and_keep_the_fast_path_on_both_sides(more, family):
    t = more[("budget-priced", family)]
    assert t["rows"] > 0 and 5 * t["leave"] >= t["rows"] and 5 * t["stay"] >= t["rows"] and t["above"] >= 1 and t["below"] >= 1, (family, t)
