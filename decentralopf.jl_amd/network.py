"""Network element types, PTDF set-up and the shipped three-node case (host side, CPU by design).

Mirrors, for the Python host (Julia is not in this image; the Julia shim is julia/DecentralOPFHip.jl):
  Node / Generator / Storage / Line      src/structures/network_elements.jl:1-30
  calculate_ptdf(nodes, lines)           src/helpers/ptdf.jl:1-41   (one-off O(N^3) set-up, stays on host)
  three_node_case()                      src/cases/three_node.jl:1-21
Numeric struct fields are Int in the reference and are promoted to Float64 when packed.
Storage.initial_level is not in the reference (which starts every storage empty, src/optimization/subproblems.jl:154): the
level before the first timestep, for runs that continue a previous horizon (DOPF_F_STO_INITIAL_LEVEL).
Storage.terminal_level_min / terminal_level_max are not in the reference either (which lets the level after the last timestep
lie anywhere in [0, max_level]): a band for that level, e.g. "end at least at X" or a cyclic horizon (DOPF_F_STO_TERMINAL_LEVEL).
Generator.availability is not in the reference either (one nameplate max_generation for the whole horizon,
src/optimization/subproblems.jl:26): T per-unit values in [0, 1], the box of P[t] becomes [0, max_generation * availability[t]] —
a solar or wind profile, or a rolling horizon's renewable forecast (DOPF_F_GEN_AVAILABILITY).
Storage.charge_efficiency / discharge_efficiency are not in the reference either (whose storages are lossless,
src/optimization/subproblems.jl:150-156): eta_c, eta_d in (0, 1], the level follows E_t = E_{t-1} + eta_c C_t - D_t / eta_d
(DOPF_F_STO_EFFICIENCY).
Line.rating is not in the reference either (one max_capacity per line for the whole horizon, src/optimization/subproblems.jl:77-78):
T limits >= 0, |flow[t]| <= rating[t] — a planned derating, a dynamic rating or a security margin per timestep (DOPF_F_LINE_RATING).
Generator.quadratic_costs is not in the reference either (one constant marginal_costs per unit, src/optimization/subproblems.jl:26-40):
c2 >= 0, the cost of output P is marginal_costs * P + c2 * P^2 / 2 — a polynomial cost curve (DOPF_F_GEN_QUADRATIC_COST).
Generator.ramp_up / ramp_down are not in the reference either (its generators move freely between steps, src/optimization/subproblems.jl:26-40):
-ramp_down <= P[t] - P[t-1] <= ramp_up, the limit on how fast a unit's output changes (DOPF_F_GEN_RAMP; on a case with lines the engines add DOPF_F_GEN_RAMP_NETWORK).
Generator.energy_min / energy_max are not in the reference either: energy_min <= sum_t P[t] <= energy_max, the energy a unit delivers
over the window — a reservoir's water, a minimum take, a fuel or emission cap (DOPF_F2_GEN_ENERGY_BUDGET, the second flag word).
Generator.min_generation is not in the reference either (its generators' lower bound is 0): min(min_generation, cap[t]) <= P[t] — a
must-run floor that follows an outage down; min_generation = max_generation is a must-take unit (dopf_set_generator_min_output, on
the ramp kernels: the engines create the context with DOPF_F_GEN_RAMP).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np


@dataclass(eq=False)
class Node:
    name: str
    demand: List[int]
    slack: bool


@dataclass(eq=False)
class Generator:
    name: str
    marginal_costs: int
    max_generation: int
    plot_color: str
    node: Node
    availability: Optional[Sequence[float]] = None      # T per-unit values in [0, 1]; None = always max_generation (not in the reference)
    quadratic_costs: float = 0.0                        # c2 >= 0: the cost is marginal_costs * P + c2 * P^2 / 2 (not in the reference)
    ramp_up: float = float("inf")                       # >= 0: P[t] - P[t-1] <= ramp_up; inf = no limit (not in the reference)
    ramp_down: float = float("inf")                     # >= 0: P[t-1] - P[t] <= ramp_down; inf = no limit (not in the reference)
    energy_min: float = 0.0                             # >= 0, finite: sum_t P[t] >= energy_min (not in the reference)
    energy_max: float = float("inf")                    # >= energy_min: sum_t P[t] <= energy_max; inf = no limit (not in the reference)
    min_generation: float = 0.0                         # in [0, max_generation]: P[t] >= min(min_generation, cap[t]) (not in the reference)


@dataclass(eq=False)
class Storage:
    name: str
    marginal_costs: int
    max_power: int
    max_level: int
    plot_color: str
    node: Node
    initial_level: float = 0.0      # level before the first timestep, 0 <= initial_level <= max_level (not in the reference)
    terminal_level_min: float = 0.0                 # band of the level after the last timestep (not in the reference)
    terminal_level_max: Optional[float] = None      # (None: max_level)
    charge_efficiency: float = 1.0                  # eta_c in (0, 1]: the level gains eta_c * C (not in the reference)
    discharge_efficiency: float = 1.0               # eta_d in (0, 1]: the level loses D / eta_d (not in the reference)


@dataclass(eq=False)
class Line:
    name: str
    from_: Node          # `from` is a Python keyword; Julia field: from
    to: Node
    max_capacity: int
    susceptance: int
    rating: Optional[Sequence[float]] = None        # T limits >= 0, one per timestep; None = max_capacity throughout (not in the reference)


def calculate_ptdf(nodes: Sequence[Node], lines: Sequence[Line]) -> np.ndarray:
    """PTDF (L x N). Incidence from=+1, to=-1; Bl = B A; Bn = A' B A; invert without the first
    slack node's row/column; PTDF = Bl * B_inv (src/helpers/ptdf.jl:1-41)."""
    N, L = len(nodes), len(lines)
    if L == 0:
        return np.zeros((0, N))
    slack = next((i for i, n in enumerate(nodes) if n.slack), None)
    if slack is None:
        raise ValueError("no slack node")
    idx = {id(n): i for i, n in enumerate(nodes)}
    inc = np.zeros((L, N))
    for l, line in enumerate(lines):
        inc[l, idx[id(line.from_)]] = 1.0
        inc[l, idx[id(line.to)]] = -1.0
    B = np.diag([float(line.susceptance) for line in lines])
    Bl = B @ inc
    Bn = inc.T @ B @ inc
    keep = [i for i in range(N) if i != slack]
    B_inv = np.zeros((N, N))
    B_inv[np.ix_(keep, keep)] = np.linalg.inv(Bn[np.ix_(keep, keep)])
    return Bl @ B_inv


def three_node_case():
    """The shipped case study: 3 nodes, 3 lines, 4 generators, 1 battery, T = 2."""
    n1 = Node("N1", [10, 250], False)
    n2 = Node("N2", [50, 70], False)
    n3 = Node("N3", [120, 200], True)
    nodes = [n1, n2, n3]
    lines = [Line("L1", n2, n1, 20, 1), Line("L2", n3, n1, 45, 1), Line("L3", n2, n3, 70, 2)]
    generators = [
        Generator("pv", 3, 80, "yellow", n1),
        Generator("wind", 4, 120, "lightblue", n2),
        Generator("coal", 30, 300, "brown", n3),
        Generator("gas", 50, 120, "grey", n1),
    ]
    storages = [Storage("battery", 1, 10, 20, "purple", n1)]
    return nodes, lines, generators, storages


@dataclass
class PackedProblem:
    """Flat SoA view of a case in the layouts include/dopf.h documents."""
    N: int
    L: int
    T: int
    demand: np.ndarray      # (N, T)
    ptdf: np.ndarray        # (L, N)
    f_max: np.ndarray       # (L,)
    gen_mc: np.ndarray
    gen_pmax: np.ndarray
    gen_node: np.ndarray    # int32, 0-based
    sto_mc: np.ndarray
    sto_pmax: np.ndarray
    sto_emax: np.ndarray
    sto_node: np.ndarray
    meta: dict = field(default_factory=dict)
    sto_e0: Optional[np.ndarray] = None     # (S,) Storage.initial_level; None = all 0
    sto_end_lo: Optional[np.ndarray] = None     # (S,) Storage.terminal_level_min; None = all 0
    sto_end_hi: Optional[np.ndarray] = None     # (S,) Storage.terminal_level_max; None = sto_emax
    gen_avail: Optional[np.ndarray] = None      # (K, T) the distinct Generator.availability series; None = no generator has one
    gen_avail_of: Optional[np.ndarray] = None   # (G,) int32 row of gen_avail per generator, -1 = always gen_pmax
    sto_eta_c: Optional[np.ndarray] = None      # (S,) Storage.charge_efficiency; None = all 1
    sto_eta_d: Optional[np.ndarray] = None      # (S,) Storage.discharge_efficiency; None = all 1
    line_rating: Optional[np.ndarray] = None    # (L, T) Line.rating (max_capacity where a line has none); None = no line has one
    gen_c2: Optional[np.ndarray] = None         # (G,) Generator.quadratic_costs; None = all 0
    gen_ramp: Optional[tuple] = None            # ((G,), (G,)) Generator.ramp_up, ramp_down; None = all inf
    gen_budget: Optional[tuple] = None          # ((G,), (G,)) Generator.energy_min, energy_max; None = all (0, inf)
    gen_min_output: Optional[np.ndarray] = None     # (G,) Generator.min_generation; None = all 0
    gen_budget_windows: Optional[tuple] = None  # (win_end (n_win,), e_min (G, n_win) or None, e_max (G, n_win) or None): energy budgets per
                                                # sub-window of the horizon (window j: win_end[j-1] <= t < win_end[j]); None = no table
    gen_budget_min_output: Optional[np.ndarray] = None  # (G,) must-run floors on a budget context (dopf_set_generator_budget_min_output); None = not set

    @property
    def G(self):
        return int(self.gen_mc.size)

    @property
    def S(self):
        return int(self.sto_mc.size)

    def engine_kwargs(self):
        """Arguments of _capi.Engine in the C ABI's memory order (column-major matrices). sto_e0 only when some storage
        starts above 0 (engines then run with F_STO_INITIAL_LEVEL; everything else sees the arguments of before)."""
        kw = dict(
            N=self.N, L=self.L, T=self.T,
            demand=np.asarray(self.demand, dtype=np.float64).reshape(self.N, self.T).T.ravel(),
            ptdf=np.asarray(self.ptdf, dtype=np.float64).reshape(self.L, self.N).T.ravel(),
            f_max=self.f_max, gen_mc=self.gen_mc, gen_pmax=self.gen_pmax, gen_node=self.gen_node,
            sto_mc=self.sto_mc, sto_pmax=self.sto_pmax, sto_emax=self.sto_emax, sto_node=self.sto_node)
        if self.sto_e0 is not None and np.any(np.asarray(self.sto_e0) != 0.0):
            kw["sto_e0"] = np.asarray(self.sto_e0, dtype=np.float64)
        if self.has_terminal_band():      # (engines then run with F_STO_TERMINAL_LEVEL)
            kw["sto_end_lo"], kw["sto_end_hi"] = self.terminal_band()
        if self.has_availability():      # (engines then run with F_GEN_AVAILABILITY)
            kw["gen_avail"], kw["gen_avail_of"] = self.availability()
        if self.has_efficiency():      # (engines then run with F_STO_EFFICIENCY)
            kw["sto_eta"] = self.efficiency()
        if self.line_rating is not None:      # (engines then run with F_LINE_RATING)
            kw["line_rating"] = np.asarray(self.line_rating, dtype=np.float64).reshape(self.L, self.T)
        if self.has_quadratic_cost():      # (engines then run with F_GEN_QUADRATIC_COST)
            kw["gen_c2"] = self.quadratic_cost()
        if self.has_ramp():      # (engines then run with F_GEN_RAMP)
            kw["gen_ramp"] = self.ramp()
        if self.has_budget():      # (engines then run with F2_GEN_ENERGY_BUDGET, through dopf_create_ex)
            kw["gen_budget"] = self.budget()
        if self.gen_min_output is not None and np.any(np.asarray(self.gen_min_output) != 0.0):
            kw["gen_min_output"] = self.min_output()      # (engines then run with F_GEN_RAMP: the floors run on the ramp kernels)
        if self.has_budget_windows():      # (engines then run with F2_GEN_ENERGY_BUDGET and set the table behind everything else)
            kw["gen_budget_windows"] = self.budget_windows()
        if self.gen_budget_min_output is not None:      # (engines then run with F2_GEN_ENERGY_BUDGET and set the floors last of all)
            kw["gen_budget_min_output"] = np.asarray(self.gen_budget_min_output, dtype=np.float64)
        return kw

    def budget_windows(self):
        """(win_end int32 (n_win,), e_min, e_max float64 (G, n_win)), the defaults filled in: all 0, all inf. Needs a table."""
        ends, lo, hi = self.gen_budget_windows
        ends = np.asarray(ends, dtype=np.int32).reshape(-1)
        lo = np.zeros((self.G, ends.size)) if lo is None else np.asarray(lo, dtype=np.float64).reshape(self.G, ends.size)
        hi = np.full((self.G, ends.size), np.inf) if hi is None else np.asarray(hi, dtype=np.float64).reshape(self.G, ends.size)
        return ends, lo, hi

    def has_budget_windows(self) -> bool:
        """The problem carries a table of energy budgets per sub-window (a shard: the whole problem does, and the shard holds its rows)."""
        return self.gen_budget_windows is not None

    def min_output(self):
        """min_generation, float64 (G,), the default filled in: all 0."""
        return np.zeros(self.G) if self.gen_min_output is None else np.asarray(self.gen_min_output, dtype=np.float64)

    def has_min_output(self) -> bool:
        """Some generator has a floor (a shard: some generator of the whole problem, so that every rank runs with the ramp flag)."""
        return bool(self.meta.get("min_output")) or bool(np.any(self.min_output() != 0.0))

    def budget(self):
        """(energy_min, energy_max), float64 (G,) each, the defaults filled in: all 0, all inf."""
        if self.gen_budget is None:
            return np.zeros(self.G), np.full(self.G, np.inf)
        return tuple(np.asarray(b, dtype=np.float64) for b in self.gen_budget)

    def has_budget(self) -> bool:
        """Some generator has an energy budget (a shard: some generator of the whole problem, so that every rank runs with the flag)."""
        lo, hi = self.budget()
        return bool(self.meta.get("budget")) or bool(np.any(lo != 0.0) or np.any(hi != np.inf))

    def ramp(self):
        """(ramp_up, ramp_down), float64 (G,) each, the default filled in: all inf."""
        if self.gen_ramp is None:
            return np.full(self.G, np.inf), np.full(self.G, np.inf)
        return tuple(np.asarray(r, dtype=np.float64) for r in self.gen_ramp)

    def has_ramp(self) -> bool:
        """Some generator has a finite ramp limit (a shard: some generator of the whole problem, so that every rank runs with the flag)."""
        if self.meta.get("ramp") or self.meta.get("min_output"):      # (a floor runs on the ramp kernels: the shards of such a problem all take the flag)
            return True
        return self.gen_ramp is not None and any(bool(np.any(np.isfinite(r))) for r in self.ramp())

    def quadratic_cost(self):
        """c2, float64 (G,), the default filled in: all 0."""
        return np.zeros(self.G) if self.gen_c2 is None else np.asarray(self.gen_c2, dtype=np.float64)

    def has_quadratic_cost(self) -> bool:
        """Some generator has a quadratic cost term (a shard: some generator of the whole problem, so that every rank runs with the flag)."""
        return bool(self.meta.get("quadratic_cost")) or (self.gen_c2 is not None and bool(np.any(np.asarray(self.gen_c2) != 0.0)))

    def efficiency(self):
        """(eta_c, eta_d), float64 (S,) each, the defaults filled in: all 1."""
        ec = np.ones(self.S) if self.sto_eta_c is None else np.asarray(self.sto_eta_c, dtype=np.float64)
        ed = np.ones(self.S) if self.sto_eta_d is None else np.asarray(self.sto_eta_d, dtype=np.float64)
        return ec, ed

    def has_efficiency(self) -> bool:
        """Some storage's charge or discharge efficiency differs from 1."""
        ec, ed = self.efficiency()
        return bool(np.any(ec != 1.0) or np.any(ed != 1.0))

    def availability(self):
        """(profiles (K, T) float64, profile_of (G,) int32): the generators' availability, K = 0 and all -1 when none has one."""
        prof = np.zeros((0, self.T)) if self.gen_avail is None else np.asarray(self.gen_avail, dtype=np.float64).reshape(-1, self.T)
        of = (np.full(self.G, -1, dtype=np.int32) if self.gen_avail_of is None
              else np.asarray(self.gen_avail_of, dtype=np.int32))
        return prof, of

    def has_availability(self) -> bool:
        """Some generator has an availability profile."""
        return self.gen_avail_of is not None and bool(np.any(np.asarray(self.gen_avail_of) >= 0))

    def terminal_band(self):
        """(lo, hi) of the level after the last timestep, float64 (S,) each, the defaults filled in: [0, sto_emax]."""
        lo = np.zeros(self.S) if self.sto_end_lo is None else np.asarray(self.sto_end_lo, dtype=np.float64)
        hi = np.asarray(self.sto_emax if self.sto_end_hi is None else self.sto_end_hi, dtype=np.float64)
        return lo, hi

    def has_terminal_band(self) -> bool:
        """Some storage's band differs from the default [0, max_level]."""
        lo, hi = self.terminal_band()
        return bool(np.any(lo != 0.0) or np.any(hi != np.asarray(self.sto_emax, dtype=np.float64)))

    def shard(self, rank: int, world: int) -> "PackedProblem":
        """Contiguous slice of the agent lists for one rank (network data replicated)."""
        def cut(n):
            base, rem = divmod(n, world)
            lo = rank * base + min(rank, rem)
            return lo, lo + base + (1 if rank < rem else 0)
        g0, g1 = cut(self.G)
        s0, s1 = cut(self.S)
        return PackedProblem(
            N=self.N, L=self.L, T=self.T, demand=self.demand, ptdf=self.ptdf, f_max=self.f_max,
            gen_mc=self.gen_mc[g0:g1], gen_pmax=self.gen_pmax[g0:g1], gen_node=self.gen_node[g0:g1],
            sto_mc=self.sto_mc[s0:s1], sto_pmax=self.sto_pmax[s0:s1], sto_emax=self.sto_emax[s0:s1],
            sto_node=self.sto_node[s0:s1],
            meta=dict(self.meta, rank=rank, world=world, gen_range=(g0, g1), sto_range=(s0, s1),
                      n_agents_global=self.G + self.S, quadratic_cost=self.has_quadratic_cost(), ramp=self.has_ramp(),
                      budget=self.has_budget(), min_output=self.has_min_output()),
            sto_e0=None if self.sto_e0 is None else self.sto_e0[s0:s1],
            sto_end_lo=None if self.sto_end_lo is None else self.sto_end_lo[s0:s1],
            sto_end_hi=None if self.sto_end_hi is None else self.sto_end_hi[s0:s1],
            gen_avail=self.gen_avail,
            gen_avail_of=None if self.gen_avail_of is None else self.gen_avail_of[g0:g1],
            sto_eta_c=None if self.sto_eta_c is None else self.sto_eta_c[s0:s1],
            sto_eta_d=None if self.sto_eta_d is None else self.sto_eta_d[s0:s1],
            line_rating=self.line_rating,
            gen_c2=None if self.gen_c2 is None else self.gen_c2[g0:g1],
            gen_ramp=None if self.gen_ramp is None else tuple(np.asarray(r)[g0:g1] for r in self.gen_ramp),
            gen_budget=None if self.gen_budget is None else tuple(np.asarray(b)[g0:g1] for b in self.gen_budget),
            gen_min_output=None if self.gen_min_output is None else np.asarray(self.gen_min_output)[g0:g1],
            gen_budget_windows=None if self.gen_budget_windows is None else tuple(
                b if i == 0 or b is None else np.asarray(b).reshape(self.G, -1)[g0:g1] for i, b in enumerate(self.gen_budget_windows)),
            gen_budget_min_output=None if self.gen_budget_min_output is None else np.asarray(self.gen_budget_min_output)[g0:g1])


def pack(nodes: Sequence[Node], generators: Sequence[Generator], storages: Sequence[Storage],
         lines: Sequence[Line]) -> PackedProblem:
    """What ADMM(...) derives from the element vectors (src/structures/admm.jl:28-60)."""
    idx = {id(n): i for i, n in enumerate(nodes)}
    T = len(nodes[0].demand)
    for n in nodes:
        if len(n.demand) != T:
            raise ValueError("all nodes need a demand series of the same length")
    f64 = lambda xs: np.asarray(list(xs), dtype=np.float64)
    i32 = lambda xs: np.asarray(list(xs), dtype=np.int32)
    # availability: identical series share one row of the table (one solar shape for many units)
    rows, of, seen = [], [], {}
    for g in generators:
        if g.availability is None:
            of.append(-1)
            continue
        a = f64(g.availability)
        if a.shape != (T,):
            raise ValueError(f"generator {g.name}: availability needs {T} values, got {a.size}")
        if np.any(np.isnan(a)) or np.any(a < 0.0) or np.any(a > 1.0):
            raise ValueError(f"generator {g.name}: availability values must lie in [0, 1]")
        key = a.tobytes()
        if key not in seen:
            seen[key] = len(rows)
            rows.append(a)
        of.append(seen[key])
    has_avail = bool(rows)
    c2 = f64(g.quadratic_costs for g in generators)
    if not np.all(np.isfinite(c2)) or np.any(c2 < 0.0):
        raise ValueError("generator quadratic_costs must be finite and >= 0")
    ramp = (f64(g.ramp_up for g in generators), f64(g.ramp_down for g in generators))
    if any(np.any(np.isnan(r)) or np.any(r < 0.0) for r in ramp):
        raise ValueError("generator ramp_up / ramp_down must be >= 0 (inf: no limit)")
    budget = (f64(g.energy_min for g in generators), f64(g.energy_max for g in generators))
    if not np.all(np.isfinite(budget[0])) or np.any(budget[0] < 0.0) or np.any(np.isnan(budget[1])) or np.any(budget[1] < budget[0]):
        raise ValueError("generator energy_min must be finite and >= 0, energy_max >= energy_min (inf: no limit)")
    pmin = f64(g.min_generation for g in generators)
    if not np.all(np.isfinite(pmin)) or np.any(pmin < 0.0) or np.any(pmin > f64(g.max_generation for g in generators)):
        raise ValueError("generator min_generation must lie in [0, max_generation]")
    # line ratings: a table only when some line has one (the others keep max_capacity in every timestep)
    rating = None
    if any(l.rating is not None for l in lines):
        rating = np.empty((len(lines), T))
        for i, l in enumerate(lines):
            r = np.full(T, float(l.max_capacity)) if l.rating is None else f64(l.rating)
            if r.shape != (T,):
                raise ValueError(f"line {l.name}: rating needs {T} values, got {r.size}")
            if not np.all(np.isfinite(r)) or np.any(r < 0.0):
                raise ValueError(f"line {l.name}: rating values must be finite and >= 0")
            rating[i] = r
    return PackedProblem(
        N=len(nodes), L=len(lines), T=T,
        demand=np.asarray([n.demand for n in nodes], dtype=np.float64).reshape(len(nodes), T),
        ptdf=calculate_ptdf(nodes, lines),
        f_max=f64(l.max_capacity for l in lines),
        gen_mc=f64(g.marginal_costs for g in generators),
        gen_pmax=f64(g.max_generation for g in generators),
        gen_node=i32(idx[id(g.node)] for g in generators),
        sto_mc=f64(s.marginal_costs for s in storages),
        sto_pmax=f64(s.max_power for s in storages),
        sto_emax=f64(s.max_level for s in storages),
        sto_node=i32(idx[id(s.node)] for s in storages),
        sto_e0=f64(s.initial_level for s in storages),
        sto_end_lo=f64(s.terminal_level_min for s in storages),
        sto_end_hi=f64(s.max_level if s.terminal_level_max is None else s.terminal_level_max for s in storages),
        gen_avail=np.asarray(rows, dtype=np.float64).reshape(len(rows), T) if has_avail else None,
        gen_avail_of=i32(of) if has_avail else None,
        sto_eta_c=f64(s.charge_efficiency for s in storages),
        sto_eta_d=f64(s.discharge_efficiency for s in storages),
        line_rating=rating,
        gen_c2=c2,
        gen_ramp=ramp,
        gen_budget=budget,
        gen_min_output=pmin)
