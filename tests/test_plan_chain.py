"""The launch plan and the layout, pinned on the CPU (csrc/dopf_plan.h: plan_chain, make_layout).

plan_chain decides which kernels a context runs — lean or general storage body, fused launches, one-launch tail, quiet chain, item
sizes, block counts — and a slipped condition there gives the same numbers at another speed: no other test would see it. The
header has no HIP include, so a small program (tests/plan_chain_main.cpp: its own main, that header only) is built with g++ under the
address and undefined-behaviour sanitizers and fed the cases of tests/golden/plan_chain.json; its lines must equal the golden's, which
were written by the same program built against the plan and layout code of the commit before the header existed. One build serves
every case: -DDOPF_EXPERIMENTS only makes the sizing knobs readable, and a case runs with them unset unless it names some ("env") —
the two cases at the one-launch tail's 1000-arrival cap do, since no shipped build cuts that many items on one node."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "decentralopf.jl_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_chain.json")
KNOBS = ("DOPF_GEN_TARGET_ITEMS", "DOPF_STO_TARGET_ITEMS", "DOPF_GEN_BLOCKS")


@pytest.fixture(scope="module")
def plan_cases():
    return json.load(open(GOLDEN))["cases"]


@pytest.fixture(scope="module")
def outputs(plan_cases, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_chain")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-DDOPF_EXPERIMENTS", "-I" + CSRC, os.path.join(ROOT, "tests", "plan_chain_main.cpp"), "-o", exe], check=True)
    groups = {}
    for i, c in enumerate(plan_cases):
        groups.setdefault(json.dumps(c.get("env", {}), sort_keys=True), []).append(i)
    out = {}
    for key, idx in groups.items():
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(json.loads(key))
        r = subprocess.run([exe], input="".join(plan_cases[i]["input"] + "\n" for i in idx), capture_output=True, text=True, env=env)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])       # (a sanitizer report lands here)
        lines = r.stdout.splitlines()
        assert len(lines) == len(idx)
        out.update(zip(idx, lines))
    return out


def test_the_plan_and_layout_of_every_case_are_the_pinned_ones(plan_cases, outputs):
    bad = []
    for i, c in enumerate(plan_cases):
        if outputs[i] != c["output"]:
            want, got = c["output"].split(), outputs[i].split()
            bad.append((c["name"], [(w, g) for w, g in zip(want, got) if w != g]))
    assert not bad, bad[:5]


def _fields(line):
    return dict(kv.split("=") for kv in line.split() if "=" in kv)


def test_the_golden_covers_the_chains_the_bench_workloads_run(plan_cases):
    """What the figures of bench.py rest on, spelled out (the golden holds them; this names them)."""
    by = {c["name"]: _fields(c["output"].split("|")[0]) for c in plan_cases}
    c2, c4, c3, c3s, q2 = (by[k] for k in ("config2 cus=256", "config4 cus=256", "config3 cus=256", "config3-share cus=256",
                                             "config2 GEN_QUADRATIC_COST"))
    assert (c2["fuseAgents"], c2["tail"], c2["stoLean"], c2["nGenItems"], c2["genItem"], c2["nStoItems"], c2["stoItem"], c2["genBlocks"]) == \
        ("1", "1", "1", "1516", "30", "569", "8", "198")
    assert (c4["fuseAgents"], c4["tail"], c4["genSkip"], c4["nGenItems"], c4["genItem"], c4["nStoItems"], c4["stoItem"]) == \
        ("0", "1", "1", "1968", "462", "711", "128")
    assert (c3["consensus"], c3["fuseNet"], c3["quiet"], c3["stoLean"]) == ("1", "1", "1", "1")
    assert (c3s["stoLean"], c3s["fuseNet"], c3s["quiet"], c3s["rowsT"]) == ("0", "1", "1", "1280")
    assert (q2["fuseAgents"], q2["tail"], q2["nGenItems"], q2["genItem"]) == ("0", "0", "1819", "25")
    assert len(plan_cases) >= 150 and sum("env" in c for c in plan_cases) == 2
