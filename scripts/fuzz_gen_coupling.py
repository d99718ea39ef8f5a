"""The five generator features (DOPF_F_GEN_QUADRATIC_COST, DOPF_F_GEN_RAMP, DOPF_F_GEN_RAMP_NETWORK, DOPF_F2_GEN_ENERGY_BUDGET,
DOPF_F2_GEN_RAMP_BUDGET) on random shapes, against the NumPy references of tests/ row by row and against a forced-step oracle twin
for the whole state. Each case draws one family:

  c2            QC                            step_centres then clamp (plate), ramp_project_pwl with every ramp +inf (network); gen_kkt_violation
  ramp-plate    RAMP                          ramp_project, ramp_kkt_violation
  ramp-net      RAMP | RAMP_NETWORK           net_step_pieces, ramp_project_pwl, ramp_kkt_violation with phi_gen
  budget-plate  F2 BUDGET                     budget_project over plate_steps, budget_kkt_violation
  budget-net    F2 BUDGET                     budget_project over net_step_pieces, budget_kkt_violation
  pair          RAMP + F2 BUDGET + F2 PAIR    ramp_budget_project, ramp_infeasibility, budget_violation (L = 0)

with availability (1/2), heterogeneous draw_c2 (1/2), S = 0..8 storages that carry a random subset of initial level, terminal band and
efficiency (helpers.LossyRated), a rating table on networks (1/2), one chain flag of {0, NO_GRAPH, KEEP_DELTAS, DEBUG_WIDE_NET
(networks)}, gamma of {1/A, 0.3}, w_flow of {10, 0.3/A}. T comes from the edges of the kernels' 64-lane chunks and of kRampLdsT = 128
(1, 2, 3, 5, 8, 24, 63, 64, 65, 96, 127, 128, 129, 130; networks 1, 2, 5, 8, 24, 70, 129: the two scratch paths of k_gen_ramp_net),
one case in twelve (not the pair: its bisecting reference is too slow) runs T = 513 under DOPF_F_LONG_HORIZON with G <= 4; G from
{1, 2, 7, 8, 9, 16, 17, 19} or 2..40 (pair: <= 24); with probability 1/4 every generator sits on one node. Demand goes through the
tests' swing.

Per case the oracle (exact mode, with the storage, rating and availability inputs; it knows neither c2 nor the couplings) warms up for
2-5 iterations, its state is set into the HIP context, and ramps, anchors and budgets are drawn from that state with the tests' own
draws (draw_ramps, draw_limits, draw_budgets_by_state, draw_budget) — so the coverage of the first compared step is settled on the
CPU (--reference-only). Then 3-6 single steps along the device's own trajectory, each checked from its own state before:
  (a) P against the family's reference row by row (1e-9 scaled by max(1, gen_pmax)), certificate <= 1e-8, feasibility <= 1e-9, no
      solver failure;
  (b) the whole state by the forced-step twin: an oracle context with DOPF_F_GEN_AVAILABILITY, every generator on its own profile
      P_after[g] / gen_pmax[g] and gen_mc = -1e9, so that every generator's step ends on its cap, seeded with the state before. Its
      one iteration is the iteration with the generators' rows forced to the device's; D, C, E, inj, flow, avg_U, avg_K, lam, mu,
      rho are the oracle's own. All keys but cost, 1e-9 on plates and 1e-8 on networks (test_gpu_feature_parity.compare); the twin's
      P equals the device's to 1e-12 relative;
  (c) cost against helpers_quadratic.total_cost of the device's own primal, 1e-9 relative;
then (d) iterate(n), n of {4, 5, 16, 17}, in a second context seeded alike against n single steps, np.array_equal on every key
(every sum has a fixed order, graph or eager — no chain is excepted), and (e) every third case K = 2 or 3 shards
(MultiEngine, DOPF_F_COMM_HOST) with the same setters against a single context over n iterations from the zero state, 1e-7 scaled
(fuzz_sharded's bound).

--reference-only draws the same cases without loading the HIP library: the warm-up, the draws, the references of the first step, and
the forced twin against a plain oracle step (all keys but cost, 1e-11 scaled); it prints per family the rows compared, those that
leave the fast path (active ramp, binding budget, both for the pair; c2: the (g, t) strictly inside the box) and those that stay.
--families=a,b restricts the draw to those families (the suite's slices).
usage: python scripts/fuzz_gen_coupling.py [n_cases] [seed] [--families=...] [--reference-only]"""
import sys, os, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np, dopf_pkg
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth
from helpers import LossyRated, draw_profiles, engine, set_from, state_of
from helpers_budget import budget_kkt_violation, budget_project, budget_violation, draw_budgets_by_state, plate_steps, row_sums
from helpers_quadratic import draw_c2, gen_kkt_violation, total_cost
from helpers_ramp import draw_ramps, ramp_active, ramp_infeasibility, ramp_kkt_violation, ramp_project, step_centres
from helpers_ramp_budget import both_bind, draw_budget, draw_limits, ramp_budget_project
from helpers_ramp_net import net_step_pieces, phi_gen, ramp_project_pwl
from test_gpu_feature_parity import compare
from test_gpu_gen_budget import swing
import __graft_entry__ as ge
from oracle.binding import OracleApi, set_threads

FAMILIES = ("c2", "ramp-plate", "ramp-net", "budget-plate", "budget-net", "pair")
REF_ONLY = "--reference-only" in sys.argv
families = FAMILIES
for a in sys.argv[1:]:
    if a.startswith("--families="):
        families = tuple(a.split("=", 1)[1].split(","))
        assert all(f in FAMILIES for f in families), families
args = [a for a in sys.argv[1:] if not a.startswith("--")]
n_cases = int(args[0]) if len(args) > 0 else 40
seed = int(args[1]) if len(args) > 1 else 1
rng = np.random.default_rng(seed)
ora = OracleApi(ge.ORACLE_LIB, features=True)
hip = None
if not REF_ONLY:
    hip = _capi.CApi(os.environ["DOPF_LIB"], "dopf_") if os.environ.get("DOPF_LIB") else _capi.hip_api()
AV, QC, RAMP, RAMP_NET = _capi.F_GEN_AVAILABILITY, _capi.F_GEN_QUADRATIC_COST, _capi.F_GEN_RAMP, _capi.F_GEN_RAMP_NETWORK
BUDGET, PAIR = _capi.F2_GEN_ENERGY_BUDGET, _capi.F2_GEN_RAMP_BUDGET
PLATE_T = [1, 2, 3, 5, 8, 24, 63, 64, 65, 96, 127, 128, 129, 130]
NET_T = [1, 2, 5, 8, 24, 70, 129]
G_EDGES = [1, 2, 7, 8, 9, 16, 17, 19]
INF = np.inf


class Case:
    """One drawn case: the problem, its family, flags, parameters and the inputs that do not depend on the warm-up state. Every draw
    comes from the case's own generator, so a case is the same whatever ran before it and in either mode."""

    def __init__(self, cseed, families):
        r = self.rng = np.random.default_rng(cseed)
        self.cseed = cseed
        fam = self.family = str(r.choice(families))
        net = fam in ("ramp-net", "budget-net") or (fam == "c2" and r.random() < 0.5)
        long = fam != "pair" and not net and r.random() < 1.0 / 12.0
        T = 513 if long else int(r.choice(NET_T if net else PLATE_T))
        G = int(r.choice(G_EDGES)) if r.random() < 0.5 else int(r.integers(2, 41))
        G = min(G, 24) if fam == "pair" else min(G, 4) if long else G
        S = int(r.integers(0, 9))
        N, L = 1, 0
        if net:
            N = int(r.integers(2, 7))
            L = int(r.integers(N - 1, min(2 * N, N * (N - 1) // 2) + 1))
        elif r.random() < 0.2:
            N = int(r.integers(2, 6))                                  # several nodes without lines
        kw = dict(n_gen=G, n_sto=S, T=T, N=N, L=L, seed=int(r.integers(1, 10**6)))
        if net:
            kw.update(fmax_factor=0.8, fmax_min=5)
        self.kw = kw
        pp = self.pp = swing(synth.synthetic_case(**kw))
        self.one_node = bool(r.random() < 0.25)
        if self.one_node:                                              # one item of G rows: more than the block has waves
            pp.gen_node = np.full(G, int(r.integers(0, N)), dtype=np.int32)
        A = G + S
        self.gamma = float(r.choice([1.0 / A, 0.3]))
        self.w_flow = float(r.choice([10.0, 0.3 / A])) if L else 10.0
        self.params = dict(eps=0.0, gamma=self.gamma, w_flow=self.w_flow)
        # storages: a random subset of initial level, terminal band, efficiency; networks: a rating table
        use = [bool(x) for x in r.random(3) < 0.5] if S else [False] * 3
        pick = lambda *opts: str(r.choice(opts))
        self.feat = LossyRated(pp, pick("0", "full", "inside", "mix") if use[0] else None,
                               pick("default", "eq", "cyclic", "mix") if use[1] else None, None, int(r.integers(1, 10**6)),
                               eta=use[2], table=bool(L and r.random() < 0.5))
        self.F = self.feat.rating
        self.avail = bool(r.random() < 0.5)
        self.cap = np.repeat(pp.gen_pmax[:, None], T, axis=1)
        self.prof = None
        if self.avail:
            if fam == "pair":                                          # (the pair test's profiles: no zeros, a row keeps a path)
                prof, of = r.uniform(0.2, 1.0, (3, T)), r.integers(0, 3, G).astype(np.int32)
                of[::3] = -1
            else:
                prof, of = draw_profiles(pp, "K3", r)
                if T == 1:                                             # (draw_profiles' zero at t = 0 would leave boxes of one point only)
                    prof = np.where(prof == 0.0, r.uniform(0.2, 1.0, prof.shape), prof)
            self.prof = (prof, of)
            self.cap = np.where((of >= 0)[:, None], pp.gen_pmax[:, None] * prof[np.maximum(of, 0)], self.cap)
        het = bool(r.random() < 0.5)
        self.quad = het or fam == "c2"
        self.c2 = draw_c2(G, r) if het else np.full(G, float(r.choice([0.5, 2.0])) if fam == "c2" else 0.0)
        self.extra = int(r.choice([0, _capi.F_NO_GRAPH, _capi.F_KEEP_DELTAS] + ([_capi.F_DEBUG_WIDE_NET] if L else [])))
        self.flags = (self.feat.flags | (AV if self.avail else 0) | (QC if self.quad else 0) | self.extra
                      | (_capi.F_LONG_HORIZON if T > 512 else 0)
                      | (RAMP if fam in ("ramp-plate", "ramp-net", "pair") else 0) | (RAMP_NET if fam == "ramp-net" else 0))
        self.flags2 = (BUDGET if fam in ("budget-plate", "budget-net", "pair") else 0) | (PAIR if fam == "pair" else 0)
        self.warm = int(r.integers(2, 6))
        self.steps = int(r.integers(3, 7))
        self.n = int(r.choice([4, 5, 16, 17]))
        self.K = int(r.choice([2, 3]))
        self.up = self.down = self.prev = self.lo = self.hi = None

    def describe(self):
        return (f"case seed {self.cseed} {self.kw} family {self.family} flags {self.flags} flags2 {self.flags2} gamma {self.gamma:.4g} "
                f"w_flow {self.w_flow:.4g} avail {self.avail} c2 {self.quad} one-node {self.one_node}")

    def oracle(self, forced=False):
        """an oracle context in exact mode with the storage and rating inputs and the case's availability; forced: the twin — gen_mc
        so low that every generator's step ends on its cap, the profiles set per step"""
        import copy
        pp = self.pp
        if forced:
            pp = copy.copy(pp)
            pp.gen_mc = np.full(self.pp.G, -1e9)
        o = engine(ora, pp, 1, flags=self.feat.flags | (AV if self.avail or forced else 0), **self.params)
        set_threads(o, 8)
        self.feat.apply(o)
        if self.avail and not forced:
            o.set_availability(*self.prof)
        return o

    def set_inputs(self, e):
        """everything but ramps and budgets"""
        self.feat.apply(e)
        if self.avail:
            e.set_availability(*self.prof)
        if self.quad:
            e.set_quadratic_cost(self.c2)

    def set_couplings(self, e):
        if self.up is not None:
            e.set_ramp(self.up, self.down, self.prev)
        if self.lo is not None:
            e.set_energy_budget(self.lo, self.hi)

    def context(self):
        e = _capi.Engine(hip, params=_capi.default_params(flags=self.flags, **self.params), flags2=self.flags2, **self.pp.engine_kwargs())
        self.set_inputs(e)
        return e

    def steps_of(self, before):
        """what the references read of the state: (c, q) on a plate, the pieces of net_step_pieces on a network"""
        if self.pp.L:
            return net_step_pieces(self.pp, self.c2, before, self.gamma, self.w_flow, self.F)
        return step_centres(self.pp, self.c2, before, self.gamma)

    def row_steps(self, st, g):
        return st[g] if self.pp.L else plate_steps(st[0][g], st[1][g])

    def draw_couplings(self, before):
        """ramps, anchors and budgets from the warm-up state, with the tests' own draws"""
        pp, r, fam, cap = self.pp, self.rng, self.family, self.cap
        G, T = pp.G, pp.T
        if fam in ("ramp-plate", "ramp-net"):
            self.up, self.down = draw_ramps(pp, r)
            if r.random() < 0.5:                   # anchors that can come down under the caps: at or below the smallest cap of the row
                self.prev = r.uniform(0.0, 1.0, G) * cap.min(axis=1)
        elif fam in ("budget-plate", "budget-net"):
            st = self.steps_of(before)
            S = row_sums([budget_project(self.row_steps(st, g), cap[g]) for g in range(G)])
            self.lo, self.hi, _ = draw_budgets_by_state(S, row_sums(cap))
        elif fam == "pair":
            c, q = self.steps_of(before)
            anchored = T == 1 or bool(r.random() < 0.5)                # (the setter anchors every row or none)
            lim = [draw_limits(r, g, cap[g], float(pp.gen_pmax[g]), anchored) for g in range(G)]
            self.up, self.down = np.array([l[0] for l in lim]), np.array([l[1] for l in lim])
            prev = [l[2] for l in lim]
            bud = [draw_budget(r, g, c[g], q[g], cap[g], self.up[g], self.down[g], prev[g], exact=(T == 1 and prev[g] is not None))
                   for g in range(G)]
            self.lo, self.hi = np.array([b[0] for b in bud]), np.array([b[1] for b in bud])
            self.lo[2::3], self.hi[2::3] = 0.0, INF                    # every third row without a budget: draw_budget alone leaves none free
            self.prev = np.array(prev) if anchored else None

    def pv(self, g):
        return None if self.prev is None else float(self.prev[g])

    def reference(self, before):
        """(want (G, T), leaves): the family's reference of the step from `before`, and per row whether it leaves the fast path
        (c2: the number of its timesteps strictly inside the box)"""
        pp, fam, cap = self.pp, self.family, self.cap
        st = self.steps_of(before)
        want, leaves = np.zeros((pp.G, pp.T)), []
        for g in range(pp.G):
            info = {}
            if fam == "c2":
                x = ramp_project_pwl(st[g], cap[g], INF, INF, None) if pp.L else np.minimum(np.maximum(st[0][g], 0.0), cap[g])
                leaves.append(int(np.sum((x > 0.0) & (x < cap[g]))))
            elif fam == "ramp-plate":
                x = ramp_project(st[0][g], st[1][g], cap[g], self.up[g], self.down[g], self.pv(g))
                leaves.append(ramp_active(x, self.up[g], self.down[g], self.pv(g)))
            elif fam == "ramp-net":
                x = ramp_project_pwl(st[g], cap[g], self.up[g], self.down[g], self.pv(g))
                leaves.append(ramp_active(x, self.up[g], self.down[g], self.pv(g)))
            elif fam in ("budget-plate", "budget-net"):
                x = budget_project(self.row_steps(st, g), cap[g], self.lo[g], self.hi[g], info)
                leaves.append(info["side"] != 0)
            else:
                x = ramp_budget_project(st[0][g], st[1][g], cap[g], self.up[g], self.down[g], self.pv(g), self.lo[g], self.hi[g], info)
                leaves.append(both_bind(x, self.up[g], self.down[g], self.pv(g), info))
            want[g] = x
        return want, leaves

    def gradient(self, before, P):
        """the gradient of every row's step objective at P: mc + c2 P + Psi(P - p0) + w (P - p0)"""
        pp = self.pp
        if pp.L:
            return phi_gen(pp, self.c2, before, self.gamma, self.w_flow, P, self.F)
        d = P - before["P"]
        return pp.gen_mc[:, None] + self.c2[:, None] * P + before["lam"][None, :] + self.gamma * (before["inj"].sum(axis=0)[None, :] + d) + d

    def check_rows(self, before, P):
        """(a): None, or (what, value) of the first bound missed"""
        pp, fam, cap = self.pp, self.family, self.cap
        want, _ = self.reference(before)
        scale = np.maximum(1.0, pp.gen_pmax)
        w = float((np.abs(P - want).max(axis=1) / scale).max())
        if not w <= 1e-9:
            return "P", w
        if fam == "c2":
            v = gen_kkt_violation(pp, self.c2, cap, before, (before["lam"], before["mu"], before["rho"]), P, self.gamma, self.w_flow, rating=self.F)
            return None if v <= 1e-8 else ("certificate", v)
        grad = self.gradient(before, P)
        for g in range(pp.G):
            if fam in ("ramp-plate", "ramp-net"):
                infeas, stat = ramp_kkt_violation(P[g], grad[g], cap[g], self.up[g], self.down[g], self.pv(g))
            elif fam in ("budget-plate", "budget-net"):
                infeas, stat, _ = budget_kkt_violation(P[g], grad[g], cap[g], self.lo[g], self.hi[g])
                infeas /= scale[g]
            else:
                infeas = max(ramp_infeasibility(P[g], cap[g], self.up[g], self.down[g], self.pv(g)), budget_violation(P[g], self.lo[g], self.hi[g])) / scale[g]
                stat = 0.0
            if not infeas <= 1e-9:
                return f"feasibility of row {g}", infeas
            if not stat <= 1e-8:
                return f"certificate of row {g}", stat
        return None

    def forced_step(self, twin, before, iteration, P_after):
        """(b): the twin's state after the iteration from `before` with the generators' rows forced to P_after"""
        pm = self.pp.gen_pmax[:, None]
        prof = np.where(pm > 0.0, P_after / np.where(pm > 0.0, pm, 1.0), 0.0)
        twin.set_availability(np.minimum(np.maximum(prof, 0.0), 1.0), np.arange(self.pp.G, dtype=np.int32))
        set_from(twin, before, iteration)
        twin.iterate(1)
        return state_of(twin)


def same_rows(a, b):
    return float(np.abs(a - b).max()) <= 1e-12 * max(1.0, float(np.abs(b).max())) if b.size else True


def run_reference_only(c, cover):
    """the warm-up, the draws, the first step's references, and the forced twin against a plain oracle step"""
    o, twin = c.oracle(), c.oracle(forced=True)
    o.iterate(c.warm)
    before, it = state_of(o), o.get_residuals()[3]
    c.draw_couplings(before)
    _, leaves = c.reference(before)
    rows = c.pp.G * c.pp.T if c.family == "c2" else c.pp.G
    cv = cover.setdefault(c.family, [0, 0, 0])
    cv[0] += rows
    cv[1] += int(sum(leaves))
    cv[2] += rows - int(sum(leaves))
    o.iterate(1)
    plain = state_of(o)
    got = c.forced_step(twin, before, it, plain["P"])
    w, where, _ = compare(got, plain, 0.0)
    o.close(); twin.close()
    if not same_rows(got["P"], plain["P"]):
        return ("first", "twin P", float(np.abs(got["P"] - plain["P"]).max())), w
    return (("first", f"twin {where}", w) if not w <= 1e-11 else None), w


def run_device(c, k):
    """(a)-(e) of one case; returns (None or (step, key, value), the worst scaled difference of (b))"""
    o, twin = c.oracle(), c.oracle(forced=True)
    o.iterate(c.warm)
    so, it = state_of(o), o.get_residuals()[3]
    o.close()
    h = c.context()
    set_from(h, so, it)
    c.draw_couplings(state_of(h))
    c.set_couplings(h)
    tol = 1e-9 if c.pp.L == 0 else 1e-8
    worst = 0.0
    try:
        for step in range(c.steps):
            before, it = state_of(h), h.get_residuals()[3]
            h.iterate(1)
            after = state_of(h)
            miss = c.check_rows(before, after["P"])
            if miss:
                return (step,) + miss, worst
            want = c.forced_step(twin, before, it, after["P"])
            if not same_rows(want["P"], after["P"]):
                return (step, "twin P", float(np.abs(want["P"] - after["P"]).max())), worst
            w, where, _ = compare(after, want, tol)
            worst = max(worst, w)
            if not w <= tol:
                return (step, where, w), worst
            cost = total_cost(c.pp, c.c2, after["P"], after["D"], after["C"])
            rel = abs(float(after["cost"][0]) - cost) / max(1.0, abs(cost))
            if not rel <= 1e-9:
                return (step, "cost", rel), worst
        if h.solver_failures():
            return ("-", "solver failures", h.solver_failures()), worst
        # (d) iterate(n) against n single steps, both seeded from the getters' values
        st, it = state_of(h), h.get_residuals()[3]
        h2 = c.context()
        c.set_couplings(h2)
        for e in (h, h2):
            set_from(e, st, it)
        h2.iterate(c.n)
        for _ in range(c.n):
            h.iterate(1)
        a, b = state_of(h2), state_of(h)
        fails = h2.solver_failures()
        h2.close()
        for key in a:
            if not np.array_equal(a[key], b[key]):
                return (f"iterate({c.n})", key, float(np.abs(a[key] - b[key]).max())), worst
        if fails:
            return (f"iterate({c.n})", "solver failures", fails), worst
        # (e) shards against a single context from the zero state
        if k % 3 == 2 and c.pp.G >= c.K:
            ref = c.context()
            c.set_couplings(ref)
            try:
                m = _capi.MultiEngine(hip, c.K, params=_capi.default_params(flags=c.flags | _capi.F_COMM_HOST, **c.params), flags2=c.flags2,
                                      **c.pp.engine_kwargs())
            except _capi.DopfError as err:
                if "(-4)" not in str(err):
                    raise
                print("no shards:", c.describe(), err, flush=True)      # a chain flag the sharded create refuses: (a)-(d) stand
                ref.close()
                return None, worst
            c.set_inputs(m)
            c.set_couplings(m)
            ref.iterate(c.n)
            m.iterate(c.n)
            want = state_of(ref)
            P, D, C_, E = m.get_primal()
            got = [dict(P=P, D=D, C=C_, E=E)] + [{key: v for key, v in state_of(m.shard(i)).items() if key in ("lam", "mu", "rho", "inj", "flow")}
                                                 for i in range(c.K)]
            w = 0.0
            for part in got:
                for key, v in part.items():
                    if v.size:
                        w = max(w, float(np.abs(v - want[key]).max()) / max(1.0, float(np.abs(want[key]).max())))
            m.close(); ref.close()
            if not w <= 1e-7:
                return (f"{c.K} shards", "state", w), worst
        return None, worst
    finally:
        h.close(); twin.close()


worst, bad, skipped = 0.0, 0, 0
cover = {}
t0 = time.time()
for k in range(n_cases):
    c = Case(int(rng.integers(1, 2**31 - 1)), families)
    try:
        miss, w = run_reference_only(c, cover) if REF_ONLY else run_device(c, k)
    except _capi.DopfError as err:
        if "create" not in str(err) or "(-4)" not in str(err):
            raise
        print("skip", c.describe(), err, flush=True)       # a combination create refuses as unsupported: not a finding
        skipped += 1
        continue
    worst = max(worst, w)
    if miss:
        bad += 1
        what = "SOLVER FAILURES" if "solver failures" in str(miss) else "MISMATCH"
        print(what, c.describe(), "step", miss[0] if len(miss) > 2 else "-", *miss[-2:], flush=True)
    if k % 10 == 9:
        print(f"{k+1} cases, worst relative difference {worst:.2e}, bad {bad}, {time.time()-t0:.0f}s", flush=True)
if REF_ONLY:
    for fam in FAMILIES:
        if fam in cover:
            rows, leave, stay = cover[fam]
            print(f"coverage {fam}: rows {rows} leave {leave} stay {stay}")
print(f"done: {n_cases} cases, worst relative difference {worst:.2e}, bad {bad}, skipped {skipped}")
