"""What recording the iteration history costs (dopf_trace_*; bench.py cannot begin a trace).
Device side: one workload shape, the settings below in ONE process, alternating, each timed as the device-side span of a settled
dopf_iterate call (DOPF_F_TIME_CALLS, dopf_last_call_ms):
  (a) no trace — the chain of a context that never traced (run on the parent commit this is the parent's figure: the untraced time
      must not move beyond the spread of the rounds);
  (b) what = 0: the row alone, i.e. the cost of the extra launch;
  (c) duals + consensus;
  (d) everything.
Next to each: the slot's bytes (read once and written once per iteration) and the rate that is of the time added over (a).
Host side (`three` only): the wall time of the 476 recorded iterations of the three-node case through run — the per-iteration host
route — against run_recorded, history filled either way. No threshold is fixed in advance.
usage: python scripts/trace_time.py <workload: three | config1 | config2> [rounds] [iterations per timed call]"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import dopf_pkg  # noqa: E402
pkg = dopf_pkg.load()
from decentralopf_jl_amd import ADMM, _capi, run, synth  # noqa: E402
import bench  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "three"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 400
TRACE = hasattr(_capi, "TRACE_ALL")          # (the parent commit has no trace: there the script reports (a) alone)
if wl == "three":
    nodes, lines, gens, stos = pkg.three_node_case()
    pp = pkg.pack(nodes, gens, stos, lines)
    kw = dict(eps=0.0)
else:
    pp = bench.make_problem(synth, wl)
    kw = dict(gamma=1.0 / (pp.G + pp.S), eps=0.0)
runs = {"(a) no trace": None}
if TRACE:
    runs.update({"(b) what = 0": 0, "(c) duals + consensus": _capi.TRACE_DUALS | _capi.TRACE_CONSENSUS, "(d) everything": _capi.TRACE_ALL})


def slot_bytes(what):
    """csrc/trace_layout.h: the 64-byte row, then the selected sections on 16-byte boundaries"""
    N, L, T, G, S = pp.N, pp.L, pp.T, pp.G, pp.S
    full = [T, L * T, L * T, N * T, L * T, L * T, L * T, G * T, S * T, S * T]
    bit = [1] * 3 + [2] * 4 + [4] * 3
    return 64 + sum((8 * n + 15) // 16 * 16 for n, b in zip(full, bit) if what & b)


api = _capi.hip_api()
res = {}
for rnd in range(rounds):
    for name, what in runs.items():
        e = _capi.Engine(api, params=_capi.default_params(flags=_capi.F_TIME_CALLS, **kw), **pp.engine_kwargs())
        if what is not None:
            e.trace_begin(what, 8)
        e.iterate(200)                               # settle (row summaries, warm starts, the graphs)
        e.iterate(iters)
        res.setdefault(name, []).append(1000.0 * e.last_call_ms() / iters)
        e.close()
med = lambda v: sorted(v)[len(v) // 2]
print(f"{wl}: G={pp.G} S={pp.S} T={pp.T} N={pp.N} L={pp.L}, median of {rounds} rounds [min..max], microseconds per iteration, "
      f"{iters} iterations per timed call")
base = med(res["(a) no trace"])
for name, v in res.items():
    what = runs[name]
    line = f"  {name:24s} {med(v):9.2f} us [{min(v):.2f}..{max(v):.2f}]"
    if what is not None:
        b, add = slot_bytes(what), med(v) - base
        rate = f"{2.0 * b / (add * 1e-6) / 1e9:.3g} GB/s read + written over the time added" if add > 0 else "no time added"
        line += f"  {add:+8.2f} us over (a); slot {b} B per iteration ({rate})"
    print(line)

if wl == "three" and TRACE:
    from decentralopf_jl_amd import run_recorded  # noqa: E402

    def fresh():
        n, l, g, s = pkg.three_node_case()
        return ADMM(0.3, n, g, s, l, backend=api)
    wall = {"run (per-iteration host route)": [], "run_recorded (chunks of 64)": []}
    for rnd in range(rounds):
        for name, fn in (("run (per-iteration host route)", run), ("run_recorded (chunks of 64)", run_recorded)):
            a = fresh()
            t0 = time.perf_counter()
            fn(a)
            wall[name].append((time.perf_counter() - t0) * 1e3)
            assert len(a.results) == 476 and a.convergence.all
            a.engine.close()
    print(f"three-node case, 476 recorded iterations, wall time, median of {rounds} [min..max]; slot {slot_bytes(7)} B per iteration")
    for name, v in wall.items():
        print(f"  {name:34s} {med(v):9.2f} ms [{min(v):.2f}..{max(v):.2f}] = {1000.0 * med(v) / 476:.1f} us per iteration")
