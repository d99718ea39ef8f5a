"""The generator features (DOPF_F_GEN_QUADRATIC_COST, DOPF_F_GEN_RAMP, DOPF_F_GEN_RAMP_NETWORK, DOPF_F2_GEN_ENERGY_BUDGET,
DOPF_F2_GEN_RAMP_BUDGET, dopf_set_generator_min_output, dopf_set_generator_energy_budget_windows, and the prices of
dopf_get_generator_budget_price, dopf_get_generator_ramp_price and dopf_get_generator_budget_window_price) on random shapes, against
the NumPy references of tests/ row by row and against a forced-step oracle twin for the whole state. Each case draws one family:

  c2            QC                            step_centres then clamp (plate), ramp_project_pwl with every ramp +inf (network); gen_kkt_violation
  ramp-plate    RAMP                          ramp_project, ramp_kkt_violation
  ramp-net      RAMP | RAMP_NETWORK           net_step_pieces, ramp_project_pwl, ramp_kkt_violation with phi_gen
  budget-plate  F2 BUDGET                     budget_project over plate_steps, budget_kkt_violation
  budget-net    F2 BUDGET                     budget_project over net_step_pieces, budget_kkt_violation
  pair          RAMP + F2 BUDGET + F2 PAIR    ramp_budget_project, ramp_infeasibility, budget_violation (L = 0)
  floor-plate   RAMP + set_min_output         helpers_min_output.ramp_project_floor, floor_kkt_violation, floor_infeasibility
  floor-net     RAMP | RAMP_NETWORK + floors  ramp_project_pwl_floor over net_step_pieces, the same certificate with phi_gen
  window-plate  F2 BUDGET + a window table    budget_project on each window's slice of plate_steps, budget_kkt_violation per unit
  window-net    F2 BUDGET + a window table    budget_project on slices of net_step_pieces, the same

with availability (1/2), heterogeneous draw_c2 (1/2), S = 0..8 storages that carry a random subset of initial level, terminal band and
efficiency (helpers.LossyRated), a rating table on networks (1/2), one chain flag of {0, NO_GRAPH, KEEP_DELTAS, DEBUG_WIDE_NET
(networks)}, gamma of {1/A, 0.3}, w_flow of {10, 0.3/A}. T comes from the edges of the kernels' 64-lane chunks and of kRampLdsT = 128
(1, 2, 3, 5, 8, 24, 63, 64, 65, 96, 127, 128, 129, 130; networks 1, 2, 5, 8, 24, 70, 129: the two scratch paths of k_gen_ramp_net),
one case in twelve (not the pair: its bisecting reference is too slow; not networks) runs T = 513 under DOPF_F_LONG_HORIZON with
G <= 4; G from {1, 2, 7, 8, 9, 16, 17, 19} or 2..40 (pair: <= 24); with probability 1/4 every generator sits on one node. Demand goes
through the tests' swing.

Everything of the later features comes from a second generator per case (default_rng([case seed, 1])), so the first six families'
cases are the cases they were:
  floors   per row one of: 0, 10-40 % of gen_pmax, gen_pmax itself (must take), a value above the row's smallest cap (the floor is then
           fmin(p_min, cap)); half of the cases keep every ramp infinite (the header's must-take unit), the others take draw_ramps';
           an anchor (1/2) is clipped into [floor_0, cap_0]; a row without a path (helpers_min_output.path_exists) gives up its finite
           ramps, so the setter is never refused (a refusal counts as bad);
  windows  n_win of {1, 2, 3, 4..6, T where T <= 24}; the ends from {1, 2, 63, 64, 65, 127, 128, 129, T - 1} inside (0, T), filled up
           at random: one-step windows next to long ones, windows of 64 and 65 steps, starts off a multiple of 64, and with one-node
           cases rows x n_win far above kBudgetWaves; the budgets dealt by helpers_budget._unit_budgets from the warm-up state;
  prices   in every second case the context records: ramp-plate, floor-plate and the pair call ramp_price() once before the first
           step, budget-plate, budget-net and the pair budget_price() (the pair records those anyway); the call must return zeros
           and switches the context to the RP / PR = true kernels. The window families always read budget_window_price(). Only
           combinations include/dopf.h documents are drawn (no floors on budgets, no ramp prices on networks, no windows on the pair).

Per case the oracle (exact mode, with the storage, rating and availability inputs; it knows neither c2 nor the couplings) warms up for
2-5 iterations, its state is set into the HIP context, and ramps, anchors and budgets are drawn from that state with the tests' own
draws (draw_ramps, draw_limits, draw_budgets_by_state, draw_budget, _unit_budgets) — so the coverage of the first compared step is
settled on the CPU (--reference-only). Then 3-6 single steps along the device's own trajectory, each checked from its own state before:
  (a) P against the family's reference row by row (1e-9 scaled by max(1, gen_pmax)), certificate <= 1e-8, feasibility <= 1e-9, no
      solver failure;
  (b) the whole state by the forced-step twin: an oracle context with DOPF_F_GEN_AVAILABILITY, every generator on its own profile
      P_after[g] / gen_pmax[g] and gen_mc = -1e9, so that every generator's step ends on its cap, seeded with the state before. Its
      one iteration is the iteration with the generators' rows forced to the device's — whatever rule produced them, floors and
      windows included; D, C, E, inj, flow, avg_U, avg_K, lam, mu, rho are the oracle's own. All keys but cost, 1e-9 on plates and
      1e-8 on networks (test_gpu_feature_parity.compare); the twin's P equals the device's to 1e-12 relative;
  (c) cost against helpers_quadratic.total_cost of the device's own primal, 1e-9 relative;
  (p) the prices of that x-update, at the bounds of the fixed-shape tests. Ramp prices (tests/test_gpu_gen_ramp_price.py's _check_rows):
      helpers_ramp_price.ramp_price_violation of the device's prices on the device's own row <= 1e-9, |rp - ramp_multipliers(that
      row)| <= 1e-9 q gen_pmax (the pair: shift = nu / q, nu from budget_price(); prev = None without an anchor), exact zeros on a row
      whose clamped step keeps its ramps. Budget and window prices, per row or per (row, window) unit: stationarity with the device's
      nu <= 1e-9 (1 + |mc| + max |lambda|), nu within 1e-9 relative to max(1, |nu|) of the reference's where the multiplier is unique
      (phi falls strictly through the bound), the sign of a binding row its side, exactly 0 on a free one. A free unit of a window
      context stores the bits of a flagless context on the same chain from the same state, a searched one-step window of a table
      with several windows the closed-form clamp of them, and with n_win = 1 a second context with dopf_set_generator_energy_budget
      takes the same steps, np.array_equal on every key (and on the prices where it records). The window families seed all their
      contexts from the getters' values before every step, so that they read equal inputs;
then (d) iterate(n), n of {4, 5, 16, 17}, in a second context seeded alike against n single steps, np.array_equal on every key
(every sum has a fixed order, graph or eager — no chain is excepted); the second context records its prices exactly
when the first does not, so the RP / PR = true kernels are shown to store the state of the plain ones, and where both record (window
prices, the pair's budget prices) the prices are compared the same way; and (e) every third case K = 2 or 3 shards (MultiEngine,
DOPF_F_COMM_HOST) with the same setters against a single context over n iterations from the zero state, the prices included, 1e-7
scaled (fuzz_sharded's bound); of the budget and window prices the rows that are free or have one multiplier only, by the tests of
(p) on the state before the single context's last iteration — a row that meets its bound on a whole interval of nu (the pair's row
with one feasible path at T = 1) ends its search where the last bits of lambda send it, and those differ between shards and one
context; on the pair such a row's ramp prices, formed under its nu, are left out too. The rows left out are checked on each run's
own row instead: the sign rule for nu, stationarity with that nu, on the pair ramp_price_violation under shift = nu / q. A -4 from create is a skip; a refusal from any other entry is a finding, counts as bad and ends the run.

--reference-only draws the same cases without loading the HIP library: the warm-up, the draws, the references of the first step, and
the forced twin against a plain oracle step (all keys but cost, 1e-11 scaled); it prints per family the rows compared, those that
leave the fast path (active ramp, binding budget, both for the pair; c2: the (g, t) strictly inside the box; a floor row: it touches
a floor above 0; the window families count (row, window) units) and those that stay, and on lines of their own the floor rows that
touch, never touch and both touch and leave their floor, the units by side, and over the priced cases the rows the NumPy twin
prices, the signs, the cases without an anchor and at the T edges, and the budget rows by side. Both modes end with the largest
figure of every check per family (`figures`).
--families=a,b restricts the draw to those families (the suite's slices).
usage: python scripts/fuzz_gen_coupling.py [n_cases] [seed] [--families=...] [--reference-only]"""
import sys, os, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np, dopf_pkg
pkg = dopf_pkg.load()
from decentralopf_jl_amd import _capi, synth
from helpers import LossyRated, draw_profiles, engine, set_from, state_of
from helpers_budget import (CHAIN, budget_kkt_violation, budget_project, budget_violation, draw_budgets_by_state, plate_steps, row_sums,
                            x_of)
try:
    from helpers_budget import _slices, _unit_budgets, stationarity_at
except ImportError:                                # a tests/ of before the three moved into helpers_budget: where they were written
    from test_gpu_gen_budget_windows import _slices, _unit_budgets
    from test_gpu_gen_budget_price import stationarity_at
from helpers_min_output import floor_infeasibility, floor_kkt_violation, floor_of, path_exists, ramp_project_floor, ramp_project_pwl_floor
from helpers_quadratic import draw_c2, gen_kkt_violation, total_cost
from helpers_ramp import draw_ramps, ramp_active, ramp_infeasibility, ramp_kkt_violation, ramp_project, step_centres
from helpers_ramp_budget import both_bind, draw_budget, draw_limits, path_sum, ramp_budget_project
from helpers_ramp_net import net_step_pieces, phi_gen, ramp_project_pwl
from helpers_ramp_price import ramp_multipliers, ramp_price_violation
from test_gpu_feature_parity import compare
from test_gpu_gen_budget import swing
import __graft_entry__ as ge
from oracle.binding import OracleApi, set_threads

FAMILIES = ("c2", "ramp-plate", "ramp-net", "budget-plate", "budget-net", "pair", "floor-plate", "floor-net", "window-plate", "window-net")
NETS = ("ramp-net", "budget-net", "floor-net", "window-net")
RAMPED = ("ramp-plate", "ramp-net", "floor-plate", "floor-net")                # the ramp kernels alone
FLOORS = ("floor-plate", "floor-net")
BUDGETED = ("budget-plate", "budget-net", "window-plate", "window-net")         # k_gen_budget, k_gen_budget_win
WINDOWS = ("window-plate", "window-net")
RAMP_PRICED = ("ramp-plate", "floor-plate", "pair")                             # (the header refuses ramp prices on a network)
BUDGET_PRICED = ("budget-plate", "budget-net", "pair")
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
WIN_EDGES = [1, 2, 63, 64, 65, 127, 128, 129]
INF = np.inf


class Unexpected(Exception):
    """a getter's first call that does not return zeros: a finding"""


class Case:
    """One drawn case: the problem, its family, flags, parameters and the inputs that do not depend on the warm-up state. Every draw
    comes from the case's own generator, so a case is the same whatever ran before it and in either mode."""

    def __init__(self, cseed, families):
        r = self.rng = np.random.default_rng(cseed)
        self.cseed = cseed
        fam = self.family = str(r.choice(families))
        r2 = self.rng2 = np.random.default_rng([cseed, 1])             # the price axis, floors and windows: nothing of them from r
        net = fam in NETS or (fam == "c2" and r.random() < 0.5)
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
                      | (RAMP if fam in RAMPED + ("pair",) else 0) | (RAMP_NET if fam in ("ramp-net", "floor-net") else 0))
        self.flags2 = (BUDGET if fam in BUDGETED + ("pair",) else 0) | (PAIR if fam == "pair" else 0)
        self.warm = int(r.integers(2, 6))
        self.steps = int(r.integers(3, 7))
        self.n = int(r.choice([4, 5, 16, 17]))
        self.K = int(r.choice([2, 3]))
        self.up = self.down = self.prev = self.lo = self.hi = self.p_min = self.ends = None
        # the price axis: h records its prices in every second case ((d)'s second context then does not, and the other way round)
        self.priced = bool(r2.random() < 0.5)
        self.rp = fam in RAMP_PRICED
        self.bp = fam in BUDGET_PRICED
        if fam in WINDOWS:
            self.ends = self.draw_ends(r2, T)
        self.ref = None                                                # (want, leaves, infos) of the last reference

    @staticmethod
    def draw_ends(r2, T):
        """n_win of {1, 2, 3, 4..6, T itself where T <= 24} and the ends: of the edges {1, 2, 63, 64, 65, 127, 128, 129, T - 1} inside
        (0, T) as many as fit, the rest at random — one-step windows next to long ones, windows of 64 and 65 steps, starts off a
        multiple of 64"""
        opts = [1, 2, 3, int(r2.integers(4, 7))] + ([T] if T <= 24 else [])
        n_win = min(int(r2.choice(opts)), T)
        if n_win == T:
            return np.arange(1, T + 1, dtype=np.int32)
        edges = sorted({e for e in WIN_EDGES + [T - 1] if 0 < e < T})
        take = [int(e) for e in r2.choice(edges, size=min(n_win - 1, len(edges)), replace=False)] if edges and n_win > 1 else []
        rest = [t for t in range(1, T) if t not in take]
        take += [int(e) for e in r2.choice(rest, size=n_win - 1 - len(take), replace=False)] if n_win - 1 > len(take) else []
        return np.array(sorted(take) + [T], dtype=np.int32)

    def describe(self):
        return (f"case seed {self.cseed} {self.kw} family {self.family} flags {self.flags} flags2 {self.flags2} gamma {self.gamma:.4g} "
                f"w_flow {self.w_flow:.4g} avail {self.avail} c2 {self.quad} one-node {self.one_node} priced {self.priced}"
                + ("" if self.ends is None else f" ends {self.ends.tolist()}") + ("" if self.p_min is None else f" anchored {self.prev is not None}"))

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

    def set_couplings(self, e, record=None, whole=False, who="the first context"):
        """ramps, floors, budgets or the window table; record (None: the case's draw): the first call of the price getters, which
        switches the context to the recording kernels and must return zeros. whole: a one-window table as a whole-horizon budget"""
        if self.up is not None:
            e.set_ramp(self.up, self.down, self.prev)
        if self.p_min is not None:
            e.set_min_output(self.p_min)
        if self.ends is not None and not whole:
            e.set_energy_budget_windows(self.ends, self.lo, self.hi)
            self.zeros(e.budget_window_price(), "budget_window_price() after the allocation", who)
        elif self.lo is not None:
            e.set_energy_budget(*((self.lo[:, 0], self.hi[:, 0]) if whole else (self.lo, self.hi)))
        if self.priced if record is None else record:
            if self.rp:
                self.zeros(e.ramp_price(), "the first ramp_price()", who)
            if self.bp or whole:
                self.zeros(e.budget_price(), "the first budget_price()", who)

    @staticmethod
    def zeros(a, what, who):
        if np.any(a != 0.0) or np.any(np.isnan(a)):
            raise Unexpected(f"{what} of {who} is not zeros: {int(np.count_nonzero(a))} of {a.size} values, {int(np.isnan(a).sum())} NaN, "
                             f"largest {float(np.nanmax(np.abs(a))):.3e}, rows {np.flatnonzero(np.any(a.reshape(a.shape[0], -1) != 0.0, axis=1)).tolist()[:12]}")

    def context(self, flagless=False):
        """flagless: the context without budgets on the chain a budget context runs (the window families' clamped step)"""
        flags, flags2 = (self.flags | (_capi.F_NO_FUSE if self.pp.L else CHAIN), 0) if flagless else (self.flags, self.flags2)
        e = _capi.Engine(hip, params=_capi.default_params(flags=flags, **self.params), flags2=flags2, **self.pp.engine_kwargs())
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
        elif fam in FLOORS:
            self.draw_floors()
        elif fam in WINDOWS:
            st = self.steps_of(before)
            self.lo, self.hi = _unit_budgets(pp, [self.row_steps(st, g) for g in range(G)], cap, self.ends)
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

    def draw_floors(self):
        """floors by row of four kinds — none, 10-40 % of gen_pmax, gen_pmax itself (must take), a value above the row's smallest cap
        (the floor is then fmin(p_min, cap)) —, in half of the cases under infinite ramps (the header's must-take unit), else under
        draw_ramps'; an anchor (half of the cases) is clipped into [floor_0, cap_0]; a row without a path (path_exists) gives up its
        finite ramps, the remedy of helpers_min_output.floor_profiles"""
        pp, r2, cap = self.pp, self.rng2, self.cap
        G, pm = pp.G, pp.gen_pmax
        kind = r2.integers(0, 4, G)
        low = cap.min(axis=1)
        self.p_min = np.select([kind == 0, kind == 1, kind == 2], [np.zeros(G), r2.uniform(0.1, 0.4, G) * pm, pm],
                               low + r2.uniform(0.0, 1.0, G) * (pm - low))
        self.p_min = np.minimum(np.maximum(self.p_min, 0.0), pm)
        up, down = draw_ramps(pp, r2)
        if r2.random() < 0.5:
            up, down = np.full(G, INF), np.full(G, INF)
        prev = r2.uniform(0.0, 1.0, G) * pm if r2.random() < 0.5 else None
        for g in range(G):
            lo = floor_of(self.p_min[g], cap[g])
            if prev is not None:
                prev[g] = max(float(lo[0]), min(float(prev[g]), float(cap[g, 0])))
            if path_exists(lo, cap[g], up[g], down[g], None if prev is None else float(prev[g])) is not None:
                up[g] = down[g] = INF
        self.up, self.down, self.prev = up, down, prev

    def floor(self, g):
        return floor_of(0.0 if self.p_min is None else self.p_min[g], self.cap[g])

    def pv(self, g):
        return None if self.prev is None else float(self.prev[g])

    def reference(self, before):
        """(want (G, T), leaves): the family's reference of the step from `before`, and per row whether it leaves the fast path
        (c2: the number of its timesteps strictly inside the box)"""
        pp, fam, cap = self.pp, self.family, self.cap
        st = self.steps_of(before)
        want, leaves, infos = np.zeros((pp.G, pp.T)), [], []
        for g in range(pp.G):
            info = {}
            infos.append(info)
            if fam == "c2":
                x = ramp_project_pwl(st[g], cap[g], INF, INF, None) if pp.L else np.minimum(np.maximum(st[0][g], 0.0), cap[g])
                leaves.append(int(np.sum((x > 0.0) & (x < cap[g]))))
            elif fam == "ramp-plate":
                x = ramp_project(st[0][g], st[1][g], cap[g], self.up[g], self.down[g], self.pv(g))
                leaves.append(ramp_active(x, self.up[g], self.down[g], self.pv(g)))
            elif fam == "ramp-net":
                x = ramp_project_pwl(st[g], cap[g], self.up[g], self.down[g], self.pv(g))
                leaves.append(ramp_active(x, self.up[g], self.down[g], self.pv(g)))
            elif fam == "floor-plate":
                x = ramp_project_floor(st[0][g], st[1][g], self.floor(g), cap[g], self.up[g], self.down[g], self.pv(g))
                leaves.append(ramp_active(x, self.up[g], self.down[g], self.pv(g)))
            elif fam == "floor-net":
                x = ramp_project_pwl_floor(st[g], self.floor(g), cap[g], self.up[g], self.down[g], self.pv(g))
                leaves.append(ramp_active(x, self.up[g], self.down[g], self.pv(g)))
            elif fam in ("budget-plate", "budget-net"):
                x = budget_project(self.row_steps(st, g), cap[g], self.lo[g], self.hi[g], info)
                leaves.append(info["side"] != 0)
            elif fam in WINDOWS:
                steps, units = self.row_steps(st, g), []
                x = np.zeros(pp.T)
                for j, s in enumerate(_slices(self.ends)):
                    units.append({})
                    x[s] = budget_project(steps[s], cap[g][s], self.lo[g, j], self.hi[g, j], units[-1])
                info["units"], info["steps"] = units, steps
                leaves.append(any(u["side"] != 0 for u in units))
            else:
                x = ramp_budget_project(st[0][g], st[1][g], cap[g], self.up[g], self.down[g], self.pv(g), self.lo[g], self.hi[g], info)
                leaves.append(both_bind(x, self.up[g], self.down[g], self.pv(g), info))
            if fam in ("budget-plate", "budget-net"):
                info["steps"] = self.row_steps(st, g)
            want[g] = x
        self.ref = (want, leaves, infos)
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
            elif fam in FLOORS:
                up, down = min(self.up[g], 1e300), min(self.down[g], 1e300)
                infeas, stat = floor_kkt_violation(P[g], grad[g], self.floor(g), cap[g], up, down, self.pv(g))
                infeas /= scale[g]
            elif fam in WINDOWS:
                infeas = stat = 0.0
                for j, s in enumerate(_slices(self.ends)):
                    i, v, _ = budget_kkt_violation(P[g][s], grad[g][s], cap[g][s], self.lo[g, j], self.hi[g, j])
                    infeas, stat = max(infeas, i / scale[g]), max(stat, v)
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


    # ---- the prices -------------------------------------------------------------------------------------------------------------------

    def pair_branch(self, c, q, g):
        """the branch of k_gen_ramp_budget's cascade that stores row g (tests/test_gpu_gen_ramp_price.py's _branch)"""
        cap, up, down, pv, lo, hi = self.cap[g], self.up[g], self.down[g], self.pv(g), self.lo[g], self.hi[g]
        x0 = np.clip(c, 0.0, cap)
        if not ramp_infeasibility(x0, cap, up, down, pv) > 0.0:
            if lo <= path_sum(x0) <= hi:
                return 1
            x = budget_project(plate_steps(c, q), cap, lo, hi)
            return 2 if ramp_infeasibility(x, cap, up, down, pv) <= 0.0 else 4
        return 3 if lo <= path_sum(ramp_project(c, q, cap, up, down, pv)) <= hi else 4

    def ramp_price_rows(self, before, P, nu=None):
        """per row (x, a, c, q, floor, shift, zeros): the NumPy twin's prices a of the rows P (None: of the reference's own rows); on
        the pair under shift = nu / q; zeros: the row's clamped step keeps its ramps (the pair: branches 1 and 2), so the kernel
        stores exact zeros"""
        pp = self.pp
        c, q = step_centres(pp, self.c2, before, self.gamma)
        out = []
        for g in range(pp.G):
            lo, sh = self.floor(g), 0.0 if nu is None else float(nu[g]) / float(q[g])
            x = self.ref[0][g] if P is None else P[g]
            a = ramp_multipliers(x, c[g], q[g], lo, self.cap[g], self.up[g], self.down[g], self.pv(g), pm=float(pp.gen_pmax[g]), shift=sh)
            if self.family == "pair":
                zeros = self.pair_branch(c[g], q[g], g) in (1, 2)
            else:
                zeros = not floor_infeasibility(np.clip(c[g], lo, self.cap[g]), lo, self.cap[g], min(self.up[g], 1e300),
                                                min(self.down[g], 1e300), self.pv(g)) > 0.0
            out.append((x, a, c[g], float(q[g]), lo, sh, zeros))
        return out

    def check_ramp_prices(self, before, P, rp, nu):
        """tests/test_gpu_gen_ramp_price.py's _check_rows on the device's own rows: (None or (what, value), the worst certificate)"""
        worst = 0.0
        for g, (x, a, c, q, lo, sh, zeros) in enumerate(self.ramp_price_rows(before, P, nu)):
            v = ramp_price_violation(x, c, q, lo, self.cap[g], self.up[g], self.down[g], self.pv(g), rp[g], shift=sh)
            worst = max(worst, v)
            if not v <= 1e-9:
                return (f"ramp-price certificate of row {g}", v), worst
            e = float(np.abs(rp[g] - a).max()) / (q * float(self.pp.gen_pmax[g]))
            if not e <= 1e-9:
                return (f"ramp price of row {g} against the twin", e), worst
            if zeros and np.any(rp[g] != 0.0):
                return (f"ramp price of row {g}, whose clamped step keeps its ramps", float(np.abs(rp[g]).max())), worst
        return None, worst

    @staticmethod
    def unique_multiplier(steps, cap, info, target, scale):
        """tests/test_gpu_gen_budget_windows.py's test: phi(nu) = sum_t x_t(nu) falls strictly through the bound at nu*"""
        d = 1e-6 * max(1.0, abs(info["nu"]))
        f = lambda v: sum(x_of(st, c, v) for st, c in zip(steps, cap))
        return f(info["nu"] - d) - target >= 1e-12 * scale and target - f(info["nu"] + d) >= 1e-12 * scale

    def check_unit_price(self, what, P, grad, cap, steps, lo, hi, info, nu, bound, scale):
        """one budget row (a whole row or a window's unit) with the device's nu: stationarity within `bound`, the reference's nu
        where the multiplier is unique, the sign of a binding row, exactly 0 on a free one"""
        v = stationarity_at(P, grad, cap, nu)
        if not v <= bound:
            return (f"stationarity of {what} with the device's nu (of its bound)", v / bound), v / bound
        if info["side"] == 0:
            return ((f"price of the free {what}", float(nu)) if nu != 0.0 else None), v / bound
        if (nu > 0.0) != (info["side"] > 0) or nu == 0.0:
            return (f"sign of the price of {what} (side {info['side']})", float(nu)), v / bound
        if self.unique_multiplier(steps, cap, info, hi if info["side"] > 0 else lo, scale):
            rel = abs(nu - info["nu"]) / max(1.0, abs(info["nu"]))
            if not rel <= 1e-9:
                return (f"price of {what} against the reference's", rel), v / bound
        return None, v / bound

    def pair_unique(self, c, q, g, info):
        """tests/test_gpu_gen_budget_price.py's test on the pair: the ramp-constrained sum falls strictly through the bound at nu*
        (one free timestep moves by d / q: a thousandth of that on both sides says phi is not flat there)"""
        target = self.hi[g] if info["side"] > 0 else self.lo[g]
        d = 1e-6 * abs(info["nu"])
        f = lambda v: path_sum(ramp_project(c - v / q, q, self.cap[g], self.up[g], self.down[g], self.pv(g)))
        return f(info["nu"] - d) - target >= 1e-3 * d / q and target - f(info["nu"] + d) >= 1e-3 * d / q

    def one_multiplier(self, before):
        """per budget row ((G,); window families: per unit, (G, n_win)) of the step from `before`: the row is free or its multiplier is
        unique, by the references and the tests of check_budget_prices — the rows whose price two runs can be asked to agree on"""
        pp, fam = self.pp, self.family
        self.reference(before)
        infos = self.ref[2]
        if fam == "pair":
            c, q = step_centres(pp, self.c2, before, self.gamma)
            return np.array([infos[g]["side"] == 0 or self.pair_unique(c[g], q[g], g, infos[g]) for g in range(pp.G)])
        one = lambda steps, cap, info, lo, hi, g: info["side"] == 0 or self.unique_multiplier(
            steps, cap, info, hi if info["side"] > 0 else lo, max(1.0, float(pp.gen_pmax[g])))
        if fam in WINDOWS:
            return np.array([[one(infos[g]["steps"][s], self.cap[g][s], infos[g]["units"][j], self.lo[g, j], self.hi[g, j], g)
                              for j, s in enumerate(_slices(self.ends))] for g in range(pp.G)])
        return np.array([one(infos[g]["steps"], self.cap[g], infos[g], self.lo[g], self.hi[g], g) for g in range(pp.G)])

    def check_left_out(self, before, P, prices, one):
        """The rows (units) that one_multiplier leaves out of a comparison of two runs' prices, checked on one run's own row instead: nu
        carries the sign of the bound its sum sits on (tests/test_gpu_gen_budget_price.py's check_sign), and it is a multiplier of that
        row — stationarity with nu given, bound 1e-9 (1 + |mc| + max |lambda|); on the pair ramp_price_violation of the run's ramp
        prices on the run's own row under shift = nu / q, <= 1e-9, where they are recorded. None or (what, value)"""
        pp, fam, cap = self.pp, self.family, self.cap
        nu = prices["window price"] if fam in WINDOWS else prices["budget price"]
        units = _slices(self.ends) if fam in WINDOWS else [slice(0, pp.T)]
        lo, hi = (self.lo, self.hi) if fam in WINDOWS else (self.lo[:, None], self.hi[:, None])
        nu, one = nu.reshape(pp.G, len(units)), one.reshape(pp.G, len(units))
        grad = None if fam == "pair" else self.gradient(before, P)
        c, q = step_centres(pp, self.c2, before, self.gamma) if fam == "pair" else (None, None)
        lam_max = float(np.abs(before["lam"]).max()) if before["lam"].size else 0.0
        for g, j in zip(*np.nonzero(~one)):
            sl = units[j]
            x, v = P[g][sl], float(nu[g, j])
            tol = 1e-9 * max(1.0, float(np.max(cap[g][sl]))) * x.size
            total = path_sum(x)
            if (v > 0.0 and abs(total - hi[g, j]) > tol) or (v < 0.0 and abs(total - lo[g, j]) > tol):
                return f"sign of the price of unit ({g}, {j}), whose sum is {total:.6g} in [{lo[g, j]:.6g}, {hi[g, j]:.6g}]", v
            if fam != "pair":
                bound = 1e-9 * (1.0 + abs(float(pp.gen_mc[g])) + lam_max)
                r = stationarity_at(x, grad[g][sl], cap[g][sl], v)
                if not r <= bound:
                    return f"stationarity of unit ({g}, {j}) with its own nu (of its bound)", r / bound
            elif "ramp price" in prices:
                r = ramp_price_violation(x, c[g], q[g], self.floor(g), cap[g], self.up[g], self.down[g], self.pv(g), prices["ramp price"][g],
                                         shift=v / float(q[g]))
                if not r <= 1e-9:
                    return f"ramp-price certificate of row {g} under its own nu", r
        return None

    def check_budget_prices(self, before, P, nu, clamped=None):
        """tests/test_gpu_gen_budget_price.py's and tests/test_gpu_gen_budget_windows.py's checks on the device's own rows, the
        reference's (side, nu) from the last check_rows. nu: (G,), or (G, n_win) of a window context, where clamped is the flagless
        context's P of the same step: a free unit stores its bits, a searched one-step window the closed-form clamp of them.
        (None or (what, value), the worst stationarity in units of its bound)"""
        pp, fam, cap = self.pp, self.family, self.cap
        infos = self.ref[2]
        worst = 0.0
        lam_max = float(np.abs(before["lam"]).max()) if before["lam"].size else 0.0
        if fam == "pair":
            c, q = step_centres(pp, self.c2, before, self.gamma)
            for g in range(pp.G):
                info = infos[g]
                if info["side"] == 0:
                    if nu[g] != 0.0:
                        return (f"price of the free row {g}", float(nu[g])), worst
                    continue
                if np.sign(nu[g]) != info["side"]:
                    return (f"sign of the price of row {g} (side {info['side']})", float(nu[g])), worst
                if self.pair_unique(c[g], q[g], g, info):
                    rel = abs(nu[g] - info["nu"]) / max(1.0, abs(info["nu"]))
                    if not rel <= 1e-9:
                        return (f"price of row {g} against the reference's", rel), worst
            return None, worst
        grad = self.gradient(before, P)
        for g in range(pp.G):
            scale = max(1.0, float(pp.gen_pmax[g]))
            bound = 1e-9 * (1.0 + abs(float(pp.gen_mc[g])) + lam_max)
            if fam not in WINDOWS:
                miss, v = self.check_unit_price(f"row {g}", P[g], grad[g], cap[g], infos[g]["steps"], self.lo[g], self.hi[g], infos[g], nu[g],
                                                bound, scale)
                worst = max(worst, v)
                if miss:
                    return miss, worst
                continue
            for j, s in enumerate(_slices(self.ends)):
                info, lo, hi = infos[g]["units"][j], self.lo[g, j], self.hi[g, j]
                miss, v = self.check_unit_price(f"unit ({g}, {j})", P[g][s], grad[g][s], cap[g][s], infos[g]["steps"][s], lo, hi, info,
                                                nu[g, j], bound, scale)
                worst = max(worst, v)
                if miss:
                    return miss, worst
                if info["side"] == 0 and not np.array_equal(P[g][s], clamped[g][s]):
                    return (f"free unit ({g}, {j}) against the flagless context", float(np.abs(P[g][s] - clamped[g][s]).max())), worst
                if info["side"] != 0 and s.stop - s.start == 1 and self.ends.size > 1:   # (one window of one step is k_gen_budget's search)
                    want = min(max(clamped[g, s.start], lo), min(hi, cap[g, s.start]))
                    if P[g, s.start] != want:
                        return (f"one-step unit ({g}, {j}) against its clamp", abs(float(P[g, s.start]) - want)), worst
        return None, worst


def twin_distance(a, b):
    """the largest |a - b| relative to max(1, max |b|)"""
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max())) if b.size else 0.0


def same_rows(a, b):
    return twin_distance(a, b) <= 1e-12


def note(table, fam, **worst):
    """keeps the largest of each figure per family"""
    t = table.setdefault(fam, {})
    for key, v in worst.items():
        t[key] = max(t.get(key, 0.0), float(v))


def count(table, fam, **n):
    t = table.setdefault(fam, {})
    for key, v in n.items():
        t[key] = t.get(key, 0) + int(v)


def cover_new(c, before, leaves):
    """what the first step's reference says about the new families and the price axis (the coverage lines of --reference-only)"""
    pp, fam = c.pp, c.family
    want, _, infos = c.ref
    if fam in FLOORS:
        touch = leaves
        off = [bool(np.any(want[g] > c.floor(g))) for g in range(pp.G)]
        count(floors, fam, rows=pp.G, touch=sum(touch), never=pp.G - sum(touch), both=sum(t and o for t, o in zip(touch, off)))
    if fam in WINDOWS:
        sides = [u["side"] for info in infos for u in info["units"]]
        count(windows, fam, units=len(sides), above=sides.count(1), below=sides.count(-1), free=sides.count(0))
    if c.rp and c.priced:
        nu = np.array([info.get("nu", 0.0) for info in infos]) if fam == "pair" else None
        rows = c.ramp_price_rows(before, None, nu)
        count(ramp_priced, fam, cases=1, rows=pp.G, priced=sum(bool(np.any(r[1] != 0.0)) for r in rows),
              positive=sum(bool(np.any(r[1] > 0.0)) for r in rows), negative=sum(bool(np.any(r[1] < 0.0)) for r in rows),
              no_anchor=c.prev is None, long_edge=pp.T in (127, 128, 129, 130), short_edge=pp.T in (1, 2))
    if c.bp and (c.priced or fam == "pair"):                           # (the pair always records its budget prices)
        sides = [info["side"] for info in infos]
        count(budget_priced, fam, cases=1, rows=pp.G, leave=sum(leaves), stay=pp.G - sum(leaves), above=sides.count(1), below=sides.count(-1))


def run_reference_only(c, cover):
    """the warm-up, the draws, the first step's references, and the forced twin against a plain oracle step"""
    o, twin = c.oracle(), c.oracle(forced=True)
    o.iterate(c.warm)
    before, it = state_of(o), o.get_residuals()[3]
    c.draw_couplings(before)
    _, leaves = c.reference(before)
    rows = c.pp.G * c.pp.T if c.family == "c2" else c.pp.G
    if c.family in FLOORS:                                             # a floor row leaves the fast path where it touches a floor above 0
        leaves = [bool(np.any((c.ref[0][g] == c.floor(g)) & (c.floor(g) > 0.0))) for g in range(c.pp.G)]
    if c.family in WINDOWS:                                            # the windows' rows are their (row, window) units
        leaves = [u["side"] != 0 for info in c.ref[2] for u in info["units"]]
        rows = len(leaves)
    cv = cover.setdefault(c.family, [0, 0, 0])
    cv[0] += rows
    cv[1] += int(sum(leaves))
    cv[2] += rows - int(sum(leaves))
    cover_new(c, before, leaves)
    o.iterate(1)
    plain = state_of(o)
    got = c.forced_step(twin, before, it, plain["P"])
    w, where, _ = compare(got, plain, 0.0)
    o.close(); twin.close()
    note(figures, c.family, b=w, twin=twin_distance(got["P"], plain["P"]))
    if not same_rows(got["P"], plain["P"]):
        return ("first", "twin P", float(np.abs(got["P"] - plain["P"]).max())), w
    return (("first", f"twin {where}", w) if not w <= 1e-11 else None), w


def read_prices(c, e, recording):
    """the prices the context records: {name: array}"""
    out = {}
    if c.ends is not None:
        out["window price"] = e.budget_window_price()
    if recording and c.rp:
        out["ramp price"] = e.ramp_price()
    if (recording and c.bp) or c.family == "pair":
        out["budget price"] = e.budget_price()
    return out


def run_device(c, k):
    """(a)-(e) of one case and the price checks; returns (None or (step, key, value), the worst scaled difference of (b))"""
    o, twin = c.oracle(), c.oracle(forced=True)
    o.iterate(c.warm)
    so, it = state_of(o), o.get_residuals()[3]
    o.close()
    h = c.context()
    others = []                                                        # window families: the flagless context, the whole-horizon one
    set_from(h, so, it)
    c.draw_couplings(state_of(h))
    tol = 1e-9 if c.pp.L == 0 else 1e-8
    worst = 0.0
    try:
        c.set_couplings(h)
        flagless = whole = None
        if c.ends is not None:
            flagless = c.context(flagless=True)
            others.append(flagless)
            if c.ends.size == 1:                                       # "one window with end T is dopf_set_generator_energy_budget, bit for bit"
                whole = c.context()
                others.append(whole)
                c.set_couplings(whole, whole=True, who="the whole-horizon context")
        for step in range(c.steps):
            before, it = state_of(h), h.get_residuals()[3]
            if c.ends is not None:                                     # equal inputs for the contexts compared bit for bit: all seeded by the getters' values
                for e in [h] + others:
                    set_from(e, before, it)
                before = state_of(h)
            h.iterate(1)
            after = state_of(h)
            miss = c.check_rows(before, after["P"])
            if miss:
                return (step,) + miss, worst
            want = c.forced_step(twin, before, it, after["P"])
            note(figures, c.family, twin=twin_distance(want["P"], after["P"]))
            if not same_rows(want["P"], after["P"]):
                return (step, "twin P", float(np.abs(want["P"] - after["P"]).max())), worst
            w, where, _ = compare(after, want, tol)
            worst = max(worst, w)
            note(figures, c.family, b=w)
            if not w <= tol:
                return (step, where, w), worst
            cost = total_cost(c.pp, c.c2, after["P"], after["D"], after["C"])
            rel = abs(float(after["cost"][0]) - cost) / max(1.0, abs(cost))
            if not rel <= 1e-9:
                return (step, "cost", rel), worst
            # the prices of this x-update
            prices = read_prices(c, h, c.priced)
            if "budget price" in prices:                               # (the pair's kernel always stores them: checked on every case)
                miss, v = c.check_budget_prices(before, after["P"], prices["budget price"])
                note(figures, c.family, budget_price=v)
                if miss:
                    return (step,) + miss, worst
            if "ramp price" in prices:
                miss, v = c.check_ramp_prices(before, after["P"], prices["ramp price"], prices.get("budget price"))
                note(figures, c.family, ramp_price=v)
                if miss:
                    return (step,) + miss, worst
            if c.ends is not None:
                for e in others:
                    e.iterate(1)
                miss, v = c.check_budget_prices(before, after["P"], prices["window price"], state_of(flagless)["P"])
                note(figures, c.family, budget_price=v)
                if miss:
                    return (step,) + miss, worst
                if whole is not None:
                    b = state_of(whole)
                    for key in after:
                        if not np.array_equal(after[key], b[key]):
                            return (step, f"{key} against the whole-horizon budget", float(np.abs(after[key] - b[key]).max())), worst
                    if c.priced and not np.array_equal(prices["window price"][:, 0], whole.budget_price()):
                        return (step, "window price against the whole-horizon budget's", 0.0), worst
        if h.solver_failures() or any(e.solver_failures() for e in others):
            return ("-", "solver failures", h.solver_failures()), worst
        # (d) iterate(n) against n single steps, both seeded from the getters' values; the second context records its prices exactly
        # when the first does not
        st, it = state_of(h), h.get_residuals()[3]
        h2 = c.context()
        others.append(h2)
        c.set_couplings(h2, record=not c.priced, who="the context of iterate(n)")
        for e in (h, h2):
            set_from(e, st, it)
        h2.iterate(c.n)
        for _ in range(c.n):
            h.iterate(1)
        a, b = state_of(h2), state_of(h)
        fails = h2.solver_failures()
        for key in a:
            if not np.array_equal(a[key], b[key]):
                return (f"iterate({c.n})", key, float(np.abs(a[key] - b[key]).max())), worst
        pa, pb = read_prices(c, h2, not c.priced), read_prices(c, h, c.priced)
        for key in pa:                                                 # where both record: the window prices, the pair's budget prices
            if key in pb and not np.array_equal(pa[key], pb[key]):
                return (f"iterate({c.n})", key, float(np.abs(pa[key] - pb[key]).max())), worst
        if fails:
            return (f"iterate({c.n})", "solver failures", fails), worst
        # (e) shards against a single context from the zero state
        if k % 3 == 2 and c.pp.G >= c.K:
            ref = c.context()
            others.append(ref)
            c.set_couplings(ref, who="the shards' reference context")
            try:
                m = _capi.MultiEngine(hip, c.K, params=_capi.default_params(flags=c.flags | _capi.F_COMM_HOST, **c.params), flags2=c.flags2,
                                      **c.pp.engine_kwargs())
            except _capi.DopfError as err:
                if "(-4)" not in str(err):
                    raise
                print("no shards:", c.describe(), err, flush=True)      # a chain flag the sharded create refuses: (a)-(d) stand
                return None, worst
            try:
                c.set_inputs(m)
                c.set_couplings(m, who="the shards")
                ref.iterate(c.n - 1)
                last = state_of(ref)
                ref.iterate(1)
                m.iterate(c.n - 1)
                P, D, C_, E = m.get_primal()
                last_m = dict(state_of(m.shard(0)), P=P, D=D, C=C_, E=E)          # (duals and consensus are replicated: shard 0's)
                m.iterate(1)
                want = state_of(ref)
                P, D, C_, E = m.get_primal()
                got = [dict(P=P, D=D, C=C_, E=E)] + [{key: v for key, v in state_of(m.shard(i)).items() if key in ("lam", "mu", "rho", "inj", "flow")}
                                                     for i in range(c.K)]
                w, where = 0.0, None
                for part in got:
                    for key, v in part.items():
                        if v.size and float(np.abs(v - want[key]).max()) / max(1.0, float(np.abs(want[key]).max())) > w:
                            w, where = float(np.abs(v - want[key]).max()) / max(1.0, float(np.abs(want[key]).max())), key
                # the prices of the last x-update. A budget row that meets its bound on a whole interval of nu (a window whose steps all sit
                # on box ends or flats; the pair's row with one feasible path) has no one price: the search ends where the last bits of
                # lambda send it, and those differ between the shards and one context. Such rows, by the per-step checks' own test on the
                # state before the reference context's last iteration, are left out; on the pair their ramp prices too (formed under nu).
                # What is left out is checked on each run's own rows instead (check_left_out)
                pw, pg = read_prices(c, ref, c.priced), read_prices(c, m, c.priced)
                one = c.one_multiplier(last) if ("budget price" in pw or "window price" in pw) else None
                for key, v in pg.items():
                    keep = np.ones(v.shape, dtype=bool) if one is None else one if key != "ramp price" else np.repeat(one[:, None], c.pp.T, axis=1)
                    d = np.where(keep, np.abs(v - pw[key]), 0.0)
                    if d.size and float(d.max()) / max(1.0, float(np.abs(pw[key]).max())) > w:
                        w, where = float(d.max()) / max(1.0, float(np.abs(pw[key]).max())), key
                miss = None
                if one is not None and not np.all(one):
                    miss = c.check_left_out(last_m, P, pg, one) or c.check_left_out(last, want["P"], pw, one)
            finally:
                m.close()
            if miss:
                return (f"{c.K} shards",) + miss, worst
            if not w <= 1e-7:
                return (f"{c.K} shards", where, w), worst
        return None, worst
    finally:
        h.close(); twin.close()
        for e in others:
            e.close()


worst, bad, skipped = 0.0, 0, 0
cover, floors, windows, ramp_priced, budget_priced, figures = {}, {}, {}, {}, {}, {}
t0 = time.time()
for k in range(n_cases):
    c = Case(int(rng.integers(1, 2**31 - 1)), families)
    try:
        miss, w = run_reference_only(c, cover) if REF_ONLY else run_device(c, k)
    except Unexpected as err:
        miss, w = ("-", str(err), 0.0), 0.0
    except _capi.DopfError as err:
        if "create" not in str(err) or "(-4)" not in str(err):
            bad += 1                                           # an entry refuses a combination the header allows: a finding, and the
            print("MISMATCH", c.describe(), "refused:", err, flush=True)      # run ends here (the error may be the device's)
            break
        else:
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
    for name, table in (("floors", floors), ("windows", windows), ("ramp-priced", ramp_priced), ("budget-priced", budget_priced)):
        for fam in FAMILIES:
            if fam in table:
                print(f"{name} {fam}: " + " ".join(f"{key} {v}" for key, v in table[fam].items()))
for fam in FAMILIES:
    if fam in figures:
        print(f"figures {fam}: " + " ".join(f"{key} {v:.2e}" for key, v in sorted(figures[fam].items())))
print(f"done: {n_cases} cases, worst relative difference {worst:.2e}, bad {bad}, skipped {skipped}")
