"""csrc/central_sto.h on the CPU (the pattern of tests/test_central_rows_host.py). The header has no HIP include, so
tests/central_sto_main.cpp — its own main around that header alone — is built with g++ under the address and undefined-behaviour
sanitizers and fed seeded storage rows as hexadecimal doubles. It steps a row one timestep after the other, the sums sequential: the
order in which a wave or a block of kc_sto / kc_sto_long adds is the kernels' business, the statements per timestep are the header's,
and those are what this pins. The program is built with -ffp-contract=off, so no multiply-add is fused on the host, and stderr must
stay empty (a sanitizer report lands there). Tolerance 0 throughout, with one exception that is stated where it is made:

  (a) LV 0 gives the bits of a NumPy twin written from helpers_central_coupled.pdhg's storage formulas;
  (b) LV 3 with al = be = 1 gives LV 2's bits (every new operation multiplies by exactly 1);
  (c) LV 2 with the band [0, em] gives LV 1's bits;
  (d) LV 1 with e0 = 0 gives LV 0's bits but for the support term."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
HORIZONS = (1, 2, 7, 65)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("centralsto") / "central_sto")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "central_sto_main.cpp"), "-o", out], check=True)
    return out


def _hex(values):
    return " ".join(float(v).hex() for v in np.atleast_1d(values))


def rows(per_horizon, seed):
    """Seeded rows: dict(T, mc, pm, em, e0, elo, ehi, al, be, absH, w, pi, yE, d, c). The multipliers have both signs and zeros (the last
    one too: the terminal band's slot), the columns sit inside their boxes with a share at either end, e0 and the band lie in [0, em]."""
    rng = np.random.default_rng(seed)
    out = []
    for T in HORIZONS:
        for i in range(per_horizon):
            pm, em = float(rng.uniform(1.0, 40.0)), float(rng.uniform(5.0, 200.0))
            lo = float(rng.uniform(0.0, 0.6)) * em
            yE = rng.normal(0.0, 4.0, T) * (rng.random(T) > 0.35)
            if i % 3 == 0:
                yE[-1] = 0.0
            elif i % 3 == 1:
                yE[-1] = -abs(yE[-1]) - 0.5
            d, c = (np.clip(rng.uniform(-0.3, 1.3, T), 0.0, 1.0) * pm for _ in range(2))
            out.append(dict(T=T, mc=float(rng.uniform(0.0, 5.0)), pm=pm, em=em, e0=float(rng.uniform(0.0, 1.0)) * em, elo=lo,
                            ehi=lo + float(rng.uniform(0.0, 1.0)) * (em - lo), al=1.0 / float(rng.uniform(0.7, 1.0)),
                            be=float(rng.uniform(0.7, 1.0)), absH=float(rng.uniform(0.0, 3.0)), w=float(rng.choice([1.0, 0.5, 3.0])),
                            pi=rng.normal(-30.0, 30.0, T), yE=yE, d=d, c=c))
    return out


def _lines(lv, r):
    head = f"{lv} {r['T']} {_hex([r[k] for k in ('mc', 'pm', 'em', 'e0', 'elo', 'ehi', 'al', 'be')])}"
    tail = f"{_hex(r['pi'])} {_hex(r['yE'])} {_hex(r['d'])} {_hex(r['c'])}\n"
    return [f"step {head} {_hex([r['absH'], r['w']])} {tail}", f"metrics {head} {tail}"]


def _run(exe, cases):
    """cases: [(LV, row)] -> [(step output, metrics output)] as arrays"""
    lines = [ln for lv, r in cases for ln in _lines(lv, r)]
    p = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    out = [ln.split() for ln in p.stdout.splitlines()]
    assert len(out) == len(lines) and all(f[0] == ("step", "metrics")[i % 2] for i, f in enumerate(out))
    got = [np.array([float.fromhex(v) for v in f[1:]]) for f in out]
    return list(zip(got[0::2], got[1::2]))


def _seq(x):
    """cumulative sums 0 + x[0] + x[1] + ... in this order (np.sum adds pairwise)"""
    return np.cumsum(np.concatenate([[0.0], np.asarray(x, dtype=np.float64)]))


def twin_lv0(r):
    """helpers_central_coupled.pdhg's storage formulas for one row (its reduced(), step() and metrics(): no e0, no band, no
    efficiencies), with the sums taken as the program takes them — the suffix sum as total minus prefix — and in the device's grouping
    where pdhg's differs by a rounding: the primal weight inside the step size (1 / ((...) w), pdhg divides tau by it), the two columns'
    reduced-cost terms added before the product with pmax."""
    T, mc, pm, em, absH, w = r["T"], r["mc"], r["pm"], r["em"], r["absH"], r["w"]
    pi, yE, d, c = r["pi"], r["yE"], r["d"], r["c"]
    t = np.arange(T)
    acc = _seq(yE)
    suf = acc[-1] - acc[:-1]
    rD, rC = mc + pi - suf, mc - pi + suf
    tau = 1.0 / ((1.0 + absH + (T - t).astype(np.float64)) * w)
    dn, cn = np.clip(d - tau * rD, 0.0, pm), np.clip(c - tau * rC, 0.0, pm)
    E = _seq((2.0 * cn - c) - (2.0 * dn - d))[1:]
    sg = w / (2.0 * (t + 1).astype(np.float64))
    z = yE + sg * E
    step = np.concatenate([dn, cn, z - sg * np.clip(z / sg, 0.0, em)])
    lev = _seq(c - d)[1:]
    viol = max(0.0, float(np.max(np.maximum(-lev, lev - em))))
    metrics = np.concatenate([[_seq(mc * (d + c))[-1], _seq((np.minimum(rD, 0.0) + np.minimum(rC, 0.0)) * pm)[-1], viol,
                               _seq(np.maximum(yE, 0.0) * em)[-1]], lev])
    return step, metrics


def _differing(got, want):
    return [i for i, (g, w) in enumerate(zip(got, want)) if not (np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]))]


def test_lv0_gives_the_bits_of_the_numpy_twin(exe):
    cases = rows(40, 7)
    got = _run(exe, [(0, r) for r in cases])
    want = [twin_lv0(r) for r in cases]
    assert not _differing(got, want), _differing(got, want)[:6]
    moved = sum(int(np.any(g[0][2 * r["T"]:] != 0.0)) for g, r in zip(got, cases))
    assert moved >= len(cases) // 2          # (the multipliers' proximal steps are exercised, not only their zeros)
    assert {r["T"] for r in cases} == set(HORIZONS)


def test_lv3_without_losses_gives_the_bits_of_lv2(exe):
    cases = [dict(r, al=1.0, be=1.0) for r in rows(25, 11)]
    got3, got2 = _run(exe, [(3, r) for r in cases]), _run(exe, [(2, r) for r in cases])
    assert not _differing(got3, got2), _differing(got3, got2)[:6]
    lossy = _run(exe, [(3, r) for r in rows(25, 11)])
    assert len(_differing(lossy, got2)) == len(cases)          # (and with losses LV 3 is another problem: the inputs reach it)


def test_lv2_with_the_default_band_gives_the_bits_of_lv1(exe):
    cases = [dict(r, elo=0.0, ehi=r["em"]) for r in rows(25, 13)]
    got2, got1 = _run(exe, [(2, r) for r in cases]), _run(exe, [(1, r) for r in cases])
    assert not _differing(got2, got1), _differing(got2, got1)[:6]
    banded = _run(exe, [(2, r) for r in rows(25, 13)])
    assert len(_differing(banded, got1)) >= len(cases) // 2


def test_lv1_from_an_empty_level_gives_the_bits_of_lv0_but_for_the_support_term(exe):
    """The support term is metrics value 3. LV 1 forms it with explicit fused multiply-adds, sum = fma(max(y, 0), em - e0, sum), which
    round once per timestep; LV 0's sum + max(y, 0) * em rounds the product and the sum on a host without contraction (on the device
    the compiler fuses it, and the two agree there). Every term is non-negative and with e0 = 0 the second fused step adds a zero, so
    the two sums differ by at most one rounding of the running sum per timestep: T * 2^-53 <= 65 * 1.2e-16 = 7.3e-15 relative. 1e-12
    leaves room for that and for nothing else."""
    cases = [dict(r, e0=0.0) for r in rows(25, 17)]
    got1, got0 = _run(exe, [(1, r) for r in cases]), _run(exe, [(0, r) for r in cases])
    for i, (a, b) in enumerate(zip(got1, got0)):
        assert np.array_equal(a[0], b[0]), i
        assert np.array_equal(np.delete(a[1], 3), np.delete(b[1], 3)), i
        assert abs(a[1][3] - b[1][3]) <= 1e-12 * abs(b[1][3]), (i, a[1][3], b[1][3])
    started = _run(exe, [(1, r) for r in rows(25, 17)])
    assert len(_differing(started, got0)) == len(cases)
