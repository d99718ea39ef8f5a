"""DOPF_F_GEN_RAMP_NETWORK without a GPU: the header's last bit and its twins in the bindings, the three create-time
rules through plan_chain, the bindings adding the bit only where the problem has lines, and the helper the GPU tests stand on —
ramp_project_pwl, the dynamic programme with a piecewise-linear derivative per step — against SLSQP, against its certificate and,
without kinks, against the bits of ramp_project."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg
from decentralopf_jl_amd import _capi, synth
from helpers_ramp import ramp_active, ramp_infeasibility, ramp_kkt_violation, ramp_project
from helpers_ramp_net import line_step, phi_at, primitive, pwl_cases, ramp_project_pwl

HDR = open(os.path.join(ROOT, "include", "dopf.h")).read()
JL = open(os.path.join(ROOT, "decentralopf.jl_amd", "julia", "DecentralOPFHip.jl")).read()
CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
BIT = 2147483648


def test_header_defines_the_flag_on_the_last_bit():
    m = re.search(r"#define\s+DOPF_F_GEN_RAMP_NETWORK\s+(\d+)u", HDR)
    assert m and int(m.group(1)) == BIT == _capi.F_GEN_RAMP_NETWORK
    flags = {k: int(v) for k, v in re.findall(r"#define\s+(DOPF_F_\w+)\s+(\d+)", HDR)}
    assert all(v & BIT == 0 for k, v in flags.items() if k != "DOPF_F_GEN_RAMP_NETWORK")
    union = 0
    for v in flags.values():
        assert v & union == 0 or v == 0
        union |= v
    assert union == 2 ** 32 - 1                                     # the word is full
    text = HDR[HDR.index("#define DOPF_F_GEN_RAMP_NETWORK"):]
    text = text[:text.index("*/")]
    for word in ("LAST bit", "second flag word", "DOPF_F_GEN_RAMP", "DOPF_E_SOLVER", "DOPF_E_NOMEM"):
        assert word in text, word
    assert "DOPF_F_GEN_RAMP_NETWORK" in HDR[HDR.index("#define DOPF_F_GEN_RAMP "):HDR.index("#define DOPF_F_GEN_RAMP_NETWORK")]


def test_the_bindings_carry_the_bit_as_the_sign_bit():
    q = _capi.default_params(flags=_capi.F_GEN_RAMP | _capi.F_GEN_RAMP_NETWORK)
    assert q.flags < 0 and (q.flags & _capi.F_GEN_RAMP_NETWORK) != 0 and q.flags & 32 and not q.flags & _capi.F_NO_FUSE
    assert q.flags & 0xFFFFFFFF == BIT | 32
    m = re.search(r"^const DOPF_F_GEN_RAMP_NETWORK = typemin\(Int32\)", JL, re.M)
    assert m and -2 ** 31 & 0xFFFFFFFF == BIT                       # Int32's smallest value is that bit pattern
    assert re.search(r"flags \|= DOPF_F_GEN_RAMP_NETWORK", JL)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rampnet") / "ramp_net")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "ramp_net_main.cpp"), "-o", exe], check=True)
    return exe


def _plan(exe, N, L, T, G, S, flags):
    r = subprocess.run([exe], input=f"plan {N} {L} {T} {G} {S} {flags & 0xFFFFFFFF}\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    head, text = r.stdout.strip().split(" | ") if " | " in r.stdout.strip() else (r.stdout.strip().rstrip(" |"), "")
    return dict(kv.split("=") for kv in head.split()[1:]), text


def test_the_three_create_rules_in_plan_chain(host_exe):
    RAMP, NETB = _capi.F_GEN_RAMP, _capi.F_GEN_RAMP_NETWORK
    f, text = _plan(host_exe, 6, 8, 4, 12, 0, RAMP)                 # the old refusal, with its words
    assert f["refusal"] == "1" and "copper plates" in text and "DOPF_F_GEN_RAMP_NETWORK" in text
    f, text = _plan(host_exe, 6, 8, 4, 12, 0, NETB)                 # the new flag alone: refused, on a network ...
    assert f["refusal"] == "1" and "DOPF_F_GEN_RAMP" in text
    f, text = _plan(host_exe, 1, 0, 4, 12, 0, NETB)                 # ... and on a copper plate
    assert f["refusal"] == "1"
    f, text = _plan(host_exe, 1, 0, 4, 12, 0, RAMP | NETB)          # L == 0: accepted and ignored, the copper-plate kernel
    assert (f["refusal"], f["genRamp"], f["genRampNet"]) == ("0", "1", "0")
    f, text = _plan(host_exe, 6, 8, 4, 12, 3, RAMP | NETB)
    assert (f["refusal"], f["genRamp"], f["genRampNet"]) == ("0", "1", "1") and int(f["knots"]) == 2 * 4 + 2 + 2 * 8 * 4
    f, text = _plan(host_exe, 6, 8, 4, 0, 3, RAMP | NETB)           # no generators: nothing to ramp
    assert (f["refusal"], f["genRamp"], f["genRampNet"]) == ("0", "0", "0")
    f, text = _plan(host_exe, 118, 186, 168, 1000, 0, RAMP | NETB)  # the capacity's cap
    assert int(f["knots"]) == 2 * 168 + 2 + 4096


def test_the_constructor_adds_the_bit_only_with_lines(oracle_api):
    """_extensions: what Engine, MultiEngine, ADMM, ShardedADMM and Engine.roll's rebuild all go through. An API object that has the
    entry stands in for the library (no context is created here)."""
    api = type("Api", (), {"set_generator_ramp": None, "prefix": "dopf_"})()
    for pp, lines in ((synth.synthetic_case(12, 0, 4, N=6, L=8, seed=2), True), (synth.synthetic_case(7, 0, 5, seed=3), False)):
        d = type("D", (), dict(G=pp.G, S=pp.S, T=pp.T, L=pp.L, N=pp.N))()
        up = np.full(pp.G, 5.0)
        params, todo = _capi._extensions(api, None, d, {}, dict(gen_ramp=(up, up)))
        assert [x.setter for x, _ in todo] == ["set_ramp"] and params.flags & _capi.F_GEN_RAMP
        assert ((params.flags & _capi.F_GEN_RAMP_NETWORK) != 0) == lines
        params, todo = _capi._extensions(api, None, d, {}, {})
        assert params is None and not todo                                       # no ramp keyword: no flag of either kind
    # a flag handed in by the caller stays as it is: F_GEN_RAMP alone on a network is the library's to refuse
    q = _capi.default_params(flags=_capi.F_GEN_RAMP)
    params, todo = _capi._extensions(api, q, d, {}, {})
    assert params is q and (q.flags & _capi.F_GEN_RAMP_NETWORK) == 0


# ---- ramp_project_pwl ------------------------------------------------------------------------------------------------------------------

def _slsqp(steps, cap, up, down, prev):
    from scipy.optimize import minimize
    T = len(steps)
    D = np.eye(T) - np.eye(T, k=-1)
    off = np.zeros(T)
    if prev is None:
        D, off = D[1:], off[1:]
    else:
        off[0] = -prev
    cons = []
    if np.isfinite(up) and D.shape[0]:
        cons.append(dict(type="ineq", fun=lambda x: up - (D @ x + off), jac=lambda x: -D))
    if np.isfinite(down) and D.shape[0]:
        cons.append(dict(type="ineq", fun=lambda x: down + (D @ x + off), jac=lambda x: D))
    f = lambda x: float(sum(primitive(s, v) for s, v in zip(steps, x)))
    jac = lambda x: np.array([phi_at(s, v) for s, v in zip(steps, x)])
    x0 = np.zeros(T) if prev is None else np.minimum(cap, np.maximum(0.0, prev - down * np.arange(1, T + 1)))
    r = minimize(f, x0, jac=jac, bounds=list(zip(np.zeros(T), cap)), constraints=cons, method="SLSQP", options=dict(ftol=1e-14, maxiter=500))
    return f(r.x), r.x


def test_ramp_project_pwl_against_slsqp_and_the_certificate():
    n = active = anchored = kinked = plain = 0
    worst = [0.0, 0.0]
    for steps, cap, up, down, prev in pwl_cases(220, 11):
        info = {}
        x = ramp_project_pwl(steps, cap, up, down, prev, info)
        T = len(steps)
        assert info["most"] <= 2 * T + 2 + sum(len(s[2]) - 1 for s in steps)          # the capacity rule of DESIGN.md 5s
        assert ramp_infeasibility(x, cap, up, down, prev) <= 1e-12
        f = float(sum(primitive(s, v) for s, v in zip(steps, x)))
        fs, xs = _slsqp(steps, cap, up, down, prev)
        if ramp_infeasibility(xs, cap, up, down, prev) <= 1e-9:
            assert f <= fs + 1e-9 * max(1.0, abs(fs)), (n, f, fs)                       # never above SLSQP's
        grad = np.array([phi_at(s, v) for s, v in zip(steps, x)])
        infeas, stat = ramp_kkt_violation(x, grad, cap, up, down, prev)
        assert infeas <= 1e-12 and stat <= 1e-8, (n, infeas, stat)
        worst = [max(worst[0], infeas), max(worst[1], stat)]
        n, active, anchored = n + 1, active + ramp_active(x, up, down, prev), anchored + (prev is not None)
        kinked, plain = kinked + (sum(info["merged"]) >= 3), plain + all(len(s[2]) == 1 for s in steps)
    print(f"{n} rows, {active} with an active ramp, {anchored} anchored, {kinked} with 3 or more kinks merged, {plain} without a kink: "
          f"infeasibility {worst[0]:.1e}, stationarity {worst[1]:.1e}")
    assert n >= 200 and active >= n // 2 and anchored >= n // 5 and kinked >= n // 4 and plain >= n // 5, (n, active, anchored, kinked, plain)


def test_without_kinks_and_with_one_q_it_is_ramp_project_bit_for_bit():
    rng = np.random.default_rng(5)
    n = 0
    for steps, cap, up, down, prev in pwl_cases(120, 12, tmax=40):
        T = len(steps)
        q, pm = float(rng.uniform(0.5, 3.0)), float(cap.max()) + 1.0
        c = rng.uniform(-0.5 * pm, 1.5 * pm, T)
        want = ramp_project(c, q, cap, up, down, prev)
        got = ramp_project_pwl([line_step(q, v) for v in c], cap, up, down, prev)
        assert np.array_equal(got, want), n
        n += 1
    assert n == 120


def test_the_certificate_catches_a_wrong_ramp():
    """the projection under a ramp_up off by 10 %: wherever it differs from the right one, the certificate says so"""
    differ = caught = 0
    for steps, cap, up, down, prev in pwl_cases(220, 11):
        if not np.isfinite(up) or up == 0.0:
            continue
        x, y = ramp_project_pwl(steps, cap, up, down, prev), ramp_project_pwl(steps, cap, 1.1 * up, down, prev)
        if np.abs(x - y).max() <= 1e-6:
            continue
        differ += 1
        grad = np.array([phi_at(s, v) for s, v in zip(steps, y)])
        infeas, stat = ramp_kkt_violation(y, grad, cap, up, down, prev)
        caught += max(infeas, stat) > 1e-6
    print(f"caught {caught} of the {differ} that differ")
    assert differ >= 40 and caught == differ, (differ, caught)


def test_the_capacity_is_kept():
    """with K one below what a row needs the programme gives up; with K at its need it gives the unbounded answer"""
    n = 0
    for steps, cap, up, down, prev in pwl_cases(40, 13):
        info = {}
        x = ramp_project_pwl(steps, cap, up, down, prev, info)
        assert np.array_equal(ramp_project_pwl(steps, cap, up, down, prev, K=info["most"]), x)
        assert ramp_project_pwl(steps, cap, up, down, prev, K=info["most"] - 1) is None
        n += 1
    assert n == 40
