"""Host-side mirror of the reference's ADMM driver API, on top of the C ABI (include/dopf.h).

Julia is not available in this image, so this Python module is the runnable host; the thin Julia
shim with the same calls lives in julia/DecentralOPFHip.jl. Names, argument meaning and stopping
behaviour follow the reference:

  ADMM(gamma, nodes, generators, storages, lines)   src/structures/admm.jl:1-63
  run(admm)                  ~ run!(admm)            src/optimization/run.jl:1-5
  calculate_iteration(admm)  ~ calculate_iteration!  src/optimization/run.jl:7-16
  Result / ResultGenerator / ResultStorage           src/structures/results.jl:1-117
  Convergence                                        src/structures/convergence.jl:1-20
  get_nodal_price(admm, iteration)                   src/helpers/network_elements.jl:16-25
  export_results(admm, filename)                     src/helpers/output.jl:1-85

Differences, all deliberate: no console printing per iteration; an optional
iteration cap (the reference loops forever on a non-convergent case); history recording can be
switched off (`record=False`) because the reference's whole-history vectors are O(iterations x
agents) and would dominate at 1e6 agents — then only the last state is fetched.
All compute happens in libdopf_hip; this file only marshals.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _capi
from .network import Generator, Line, Node, Storage, pack


@dataclass
class PenaltyTerm:
    """src/structures/penalty_terms.jl:1-5 (diagnostics: never read back by the algorithm)"""
    energy_balance: np.ndarray
    upper_flow: np.ndarray
    lower_flow: np.ndarray


@dataclass
class ResultGenerator:
    generator: Generator
    generation: np.ndarray
    penalty_term: Optional[PenaltyTerm] = None      # filled with ADMM(..., record_slacks=True)
    U: Optional[np.ndarray] = None                  # (L, T)
    K: Optional[np.ndarray] = None


@dataclass
class ResultStorage:
    storage: Storage
    discharge: np.ndarray
    charge: np.ndarray
    level: np.ndarray
    penalty_term: Optional[PenaltyTerm] = None
    U: Optional[np.ndarray] = None
    K: Optional[np.ndarray] = None


@dataclass
class ResultNode:
    """src/structures/results.jl:19-35: what the units of one node produce, discharge and charge per timestep."""
    node: Node
    generation: np.ndarray
    discharge: np.ndarray
    charge: np.ndarray


@dataclass
class Result:
    unit_to_result: Dict[int, object]
    generation: np.ndarray
    discharge: np.ndarray
    charge: np.ndarray
    avg_U: np.ndarray
    avg_K: np.ndarray
    total_costs: float
    injection: np.ndarray
    line_utilization: np.ndarray
    node_to_result: Dict[int, ResultNode] = field(default_factory=dict)
    penalty_term: Optional[PenaltyTerm] = None      # results.jl:66-70 (sum over the units); filled with record_slacks=True

    def of(self, unit):
        return self.unit_to_result[id(unit)]

    def of_node(self, node):
        return self.node_to_result[id(node)]


@dataclass
class Convergence:
    """src/structures/convergence.jl:1-20. With history recording the *_res lists hold the reference's vectors /
    matrices |dual change| per entry; without it their inf-norms (floats)."""
    lambda_: bool = False
    lambda_res: list = field(default_factory=list)
    mue: bool = False
    mue_res: list = field(default_factory=list)
    rho: bool = False
    rho_res: list = field(default_factory=list)
    all: bool = False


class ADMM:
    """State of one decentral OPF run. `backend` is a loaded C-ABI library (default: the HIP one)."""

    def __init__(self, gamma: float, nodes: Sequence[Node], generators: Sequence[Generator],
                 storages: Sequence[Storage], lines: Sequence[Line], *, backend: Optional[_capi.CApi] = None,
                 record: bool = True, max_iters: int = 0, backend_mode: Optional[int] = None,
                 record_slacks: bool = False, **params):
        self.iteration = 1
        self.gamma = float(gamma)
        self.nodes, self.generators = list(nodes), list(generators)
        self.storages, self.lines = list(storages), list(lines)
        self.packed = pack(self.nodes, self.generators, self.storages, self.lines)
        p = self.packed
        self.T = list(range(1, p.T + 1))
        self.N = list(range(1, p.N + 1))
        self.L = list(range(1, p.L + 1))
        self.lambdas = [np.zeros(p.T)]
        self.mues = [np.zeros((p.L, p.T))]
        self.rhos = [np.zeros((p.L, p.T))]
        self.results: List[Result] = []
        self.convergence = Convergence()
        self.ptdf = p.ptdf
        self.f_max = p.f_max
        self.total_demand = p.demand.sum(axis=0)
        self.node_id_to_demand = {i + 1: list(n.demand) for i, n in enumerate(self.nodes)}
        self.node_to_id = {id(n): i + 1 for i, n in enumerate(self.nodes)}
        self.node_to_units: Dict[int, list] = {}
        for u in self.generators + self.storages:
            self.node_to_units.setdefault(id(u.node), []).append(u)
        self.record = record
        self.record_slacks = record_slacks        # also fetch every unit's U, K and PenaltyTerm (diagnostics, HIP backend)
        if record_slacks:
            params["flags"] = int(params.get("flags", 0)) | _capi.F_KEEP_DELTAS
        self.params = _capi.default_params(gamma=self.gamma, max_iters=max_iters, **params)
        self.engine = _capi.Engine(backend if backend is not None else _capi.hip_api(),
                                   params=self.params, mode=backend_mode, **p.engine_kwargs())

    def set_initial_levels(self, e0=None) -> None:
        """The level of each storage before the first timestep (S values in the order of `storages`; None = all 0), for a
        horizon that continues where the last one ended. Not in the reference, which starts every storage empty
        (src/optimization/subproblems.jl:154). Needs flags=F_STO_INITIAL_LEVEL (set for you when a Storage has a non-zero
        initial_level); takes effect at the next iteration."""
        self.engine.set_initial_levels(e0)

    def set_terminal_levels(self, lo=None, hi=None) -> None:
        """The band [lo, hi] of each storage's level after the last timestep (S values each in the order of `storages`; both
        None = [0, max_level]): "end at least at X" is [X, max_level], a cyclic horizon lo = hi = the initial level. Not in the
        reference, which leaves that level free. Needs flags=F_STO_TERMINAL_LEVEL (set for you when a Storage has a band other
        than the default); takes effect at the next iteration."""
        self.engine.set_terminal_levels(lo, hi)

    def set_efficiency(self, eta_c=None, eta_d=None) -> None:
        """Each storage's charge and discharge efficiency in (0, 1] (S values each in the order of `storages`; both None = all 1):
        the level follows E_t = E_{t-1} + eta_c C_t - D_t / eta_d. Not in the reference, whose storages are lossless
        (src/optimization/subproblems.jl:150-156). Needs flags=F_STO_EFFICIENCY (set for you when a Storage has an efficiency
        other than 1); takes effect at the next iteration."""
        self.engine.set_efficiency(eta_c, eta_d)

    def set_availability(self, profiles=None, profile_of=None) -> None:
        """The generators' availability: K profiles (K x T, values in [0, 1]) and each generator's profile (G indices in the order
        of `generators`, -1 = always max_generation); both None = every generator at max_generation. The box of P[g,t] becomes
        [0, max_generation * profiles[k][t]]. Not in the reference (one nameplate value per generator). Needs
        flags=F_GEN_AVAILABILITY (set for you when a Generator has an availability series); takes effect at the next iteration."""
        self.engine.set_availability(profiles, profile_of)

    def set_line_rating(self, rating=None) -> None:
        """The lines' limits per timestep, an (L, T) array in the order of `lines` (None = max_capacity in every timestep):
        |flow[l,t]| <= rating[l,t]. A rating of 0 pins the flow to 0; it does not take the line out of the PTDF. Not in the
        reference (one max_capacity per line). Needs flags=F_LINE_RATING (set for you when a Line has a rating); the state and
        the iteration counter stay, the run is no longer converged; takes effect at the next iteration."""
        self.engine.set_line_rating(rating)
        self._replaced("line_rating", rating, (self.packed.L, self.packed.T))

    def set_quadratic_cost(self, c2=None) -> None:
        """Each generator's quadratic cost coefficient (G values >= 0 in the order of `generators`; None = all 0): the cost of
        output P is marginal_costs * P + c2 * P^2 / 2, and Result.total_costs follows it. Not in the reference (one constant
        marginal_costs per unit, src/optimization/subproblems.jl:26-40). Needs flags=F_GEN_QUADRATIC_COST (set for you when a
        Generator has quadratic_costs); the state and the iteration counter stay, the run is no longer converged; takes effect at
        the next iteration."""
        self.engine.set_quadratic_cost(c2)
        self._replaced("gen_c2", c2, (self.packed.G,))

    def set_ramp(self, up=None, down=None, prev=None) -> None:
        """Each generator's ramp limits (G values >= 0 each in the order of `generators`, inf = no limit; both None = all inf) and
        optionally the outputs of the step before the window (prev; None = no anchor): -down <= P[t] - P[t-1] <= up, at t = 0 against
        prev. Not in the reference (its generators move freely, src/optimization/subproblems.jl:26-40); copper plates only. Needs
        flags=F_GEN_RAMP (set for you when a Generator has a finite ramp_up or ramp_down); the state and the iteration counter stay,
        the run is no longer converged; takes effect at the next iteration."""
        self.engine.set_ramp(up, down, prev)
        G = self.packed.G
        self.packed.gen_ramp = None if up is None else tuple(np.asarray(r, dtype=np.float64).reshape(G).copy() for r in (up, down))
        self.convergence = Convergence()

    def set_energy_budget(self, e_min=None, e_max=None) -> None:
        """Each generator's energy budget over the window (G values each in the order of `generators`; e_min None = all 0, e_max None
        = all inf): e_min <= sum_t P[t] <= e_max. Not in the reference (its generators have no budget over the window). Needs the
        second flag word's F2_GEN_ENERGY_BUDGET (set for you when a Generator has an energy_min or energy_max); the state and the
        iteration counter stay, the run is no longer converged; takes effect at the next iteration."""
        self.engine.set_energy_budget(e_min, e_max)
        G = self.packed.G
        lo = np.zeros(G) if e_min is None else np.asarray(e_min, dtype=np.float64).reshape(G).copy()
        hi = np.full(G, np.inf) if e_max is None else np.asarray(e_max, dtype=np.float64).reshape(G).copy()
        self.packed.gen_budget = None if e_min is None and e_max is None else (lo, hi)
        self.convergence = Convergence()

    def budget_price(self) -> np.ndarray:
        """The water values of the run: nu[g], the multiplier the last computed iteration put on generator g's energy budget (G values
        in the order of `generators`, in the unit of marginal_cost): > 0 where energy_max holds the unit down, < 0 where energy_min
        pushes it up, 0 for a unit without a budget or with room in it. Not in the reference. Recording starts with the FIRST call (it
        switches the generator kernel and returns zeros): call it once before iterating. Zeros before the first iteration; the
        setters leave the values alone until the next iteration. At convergence minus the budget dual of the central LP
        (_capi.central_solve_coupled's budget_dual) where that dual is unique. Needs F2_GEN_ENERGY_BUDGET, as set_energy_budget."""
        return self.engine.budget_price()

    def set_energy_budget_windows(self, win_end=None, e_min=None, e_max=None) -> None:
        """One energy budget per generator and sub-window of the horizon: win_end are the windows' ends (strictly increasing, the last
        one T; window j covers win_end[j-1] <= t < win_end[j]), e_min / e_max (G, n_win) in the order of `generators` (None = all 0 /
        all inf): e_min[g,j] <= sum_{t in window j} P[t] <= e_max[g,j] — a daily allotment inside a weekly horizon. win_end None removes
        the table. Not in the reference. Needs F2_GEN_ENERGY_BUDGET (set for you when the packed problem carries a table) and no
        whole-horizon budget at the same time; the state and the iteration counter stay, the run is no longer converged; roll and
        roll_coupled are refused while a table is set (remove it, roll, set the next window's)."""
        self.engine.set_energy_budget_windows(win_end, e_min, e_max)
        self.packed.gen_budget_windows = None if win_end is None else tuple(
            None if a is None else a.copy() for a in self.engine._mirror["gen_budget_windows"])
        self.convergence = Convergence()

    def energy_budget_windows(self):
        """(win_end, e_min, e_max) as the context holds them, or None while no table is set."""
        return self.engine.energy_budget_windows()

    def budget_window_price(self) -> np.ndarray:
        """The water values per sub-window: nu[g, j], the multiplier the last computed iteration put on generator g's budget of window j,
        (G, n_win), with budget_price's sign convention. Always recorded while a table is set. At convergence minus the window rows'
        duals of the host LP (central.solve_central_packed(gen_budget_windows=)) where they are unique."""
        return self.engine.budget_window_price()

    def ramp_price(self) -> np.ndarray:
        """The ramp prices of the run: rp[g, t], the multiplier the last computed iteration put on generator g's ramp row between t-1
        and t (t = 0: the row against the anchor), (G, T) in the order of `generators` and the unit of marginal_cost — what one more
        unit per step of flexibility of g is worth at t: > 0 where ramp_up holds the unit back, < 0 where ramp_down holds it up, 0
        where no ramp binds. Not in the reference. Recording starts with the FIRST call (it switches the generator kernel and
        returns zeros): call it once before iterating. Zeros before the first iteration; the setters leave the values alone until
        the next iteration. At convergence minus the ramp dual of the central LP (_capi.central_solve_coupled's ramp_dual) where
        that dual is unique. Needs F_GEN_RAMP on a copper plate, as set_ramp."""
        return self.engine.ramp_price()

    def set_min_output(self, p_min=None) -> None:
        """Each generator's must-run floor (G values in [0, max_generation] in the order of `generators`; None = all 0):
        min(p_min, cap[t]) <= P[t], a floor that follows an availability profile down; p_min = max_generation is a must-take unit.
        Not in the reference (its generators go down to 0). Runs on the ramp kernels: needs flags=F_GEN_RAMP (set for you when a
        Generator has a min_generation), and does not combine with energy budgets; the state and the iteration counter stay, the
        run is no longer converged; takes effect at the next iteration."""
        self.engine.set_min_output(p_min)
        self._replaced("gen_min_output", p_min, (self.packed.G,))

    def set_budget_min_output(self, p_min=None) -> None:
        """Must-run floors on a run with energy budgets (G values in [0, max_generation] in the order of `generators`; None removes
        them): min(p_min, cap[t]) <= P[t] <= cap[t] inside the budgets' own step — a reservoir's minimum flow beside its water
        allotment. The floor holds for every generator, budgeted or not, whole-horizon budgets and budgets per sub-window alike. Not in
        the reference. Needs F2_GEN_ENERGY_BUDGET and no F_GEN_RAMP (there set_min_output serves); a generator whose floors sum above
        its energy_max (or a window's) is refused. The state and the iteration counter stay, the run is no longer converged; takes
        effect at the next iteration. budget_price and budget_window_price keep their meaning."""
        self.engine.set_budget_min_output(p_min)
        self._replaced("gen_budget_min_output", p_min, (self.packed.G,))

    def budget_min_output(self) -> np.ndarray:
        """The floors of set_budget_min_output as the context holds them, G values (zeros while none are set)."""
        return self.engine.budget_min_output()

    def _replaced(self, field_: str, value, shape) -> None:
        """the packed problem follows an input that was replaced under a kept state, and the run is no longer converged"""
        setattr(self.packed, field_, None if value is None else np.asarray(value, dtype=np.float64).reshape(shape).copy())
        self.convergence = Convergence()

    # -- a receding horizon ----------------------------------------------------------------------
    def _new_window(self, demand: np.ndarray) -> None:
        """the host's mirrors of the demand follow the engine's, and the recorded history starts anew for the new window"""
        for i, n in enumerate(self.nodes):
            n.demand = [float(x) for x in demand[i]]
        self.packed.demand = demand.copy()
        self.total_demand = demand.sum(axis=0)
        self.node_id_to_demand = {i + 1: list(n.demand) for i, n in enumerate(self.nodes)}
        lam, mu, rho = self.engine.get_duals()
        self.lambdas, self.mues, self.rhos = [lam], [mu], [rho]
        self.results = []
        self.convergence = Convergence()
        self.iteration = self.engine.get_residuals()[3]

    def set_demand(self, demand) -> None:
        """A new demand (N, T) for the same window, in place (dopf_set_demand): the primal state, the duals and the iteration
        counter stay, the run is no longer converged. Not in the reference, which builds a new ADMM(...) per window."""
        self.engine.set_demand(demand)
        self._new_window(self.engine.demand())

    def roll(self, k: int, demand_tail) -> None:
        """The window advances by k steps (dopf_roll_horizon; the rule is horizon.shift_window's): demand_tail (N, k) is the demand
        of the k new steps, every storage starts from the level it had after step k, the state of the kept steps warm-starts
        the new window and the iteration counter becomes 2. The availability profiles are not moved: set the new window's with
        set_availability. A line rating table moves with the window, its last column repeated: set the new window's forecast with
        set_line_rating. Not in the reference, which builds a new ADMM(...) per window (src/structures/admm.jl:23-62)."""
        self.engine.roll(k, demand_tail)
        if self.packed.line_rating is not None:          # (moved with the window: the old last column behind the kept part)
            r = np.asarray(self.packed.line_rating, dtype=np.float64)
            self.packed.line_rating = np.concatenate([r[:, int(k):], np.repeat(r[:, -1:], int(k), axis=1)], axis=1)
        self._new_window(self.engine.demand())

    def roll_coupled(self, k: int, demand_tail, *, availability=None, budget=None) -> None:
        """roll for a case with ramp limits or energy budgets, in place (dopf_roll_horizon_coupled; horizon.shift_coupled has the
        rule): the ramps' anchor becomes the output of step k - 1, and what the k leaving steps delivered comes off both budgets,
        floored at 0. availability = (profiles, profile_of): the new window's table, checked together with the new anchor;
        budget = (e_min, e_max): the new window's own budgets instead of what is left. Everything else as roll."""
        self.engine.roll_coupled(k, demand_tail, availability=availability, budget=budget)
        if self.packed.line_rating is not None:          # (moved with the window: the old last column behind the kept part)
            r = np.asarray(self.packed.line_rating, dtype=np.float64)
            self.packed.line_rating = np.concatenate([r[:, int(k):], np.repeat(r[:, -1:], int(k), axis=1)], axis=1)
        if self.packed.gen_budget is not None:           # (what the device left of them)
            self.packed.gen_budget = tuple(b.copy() for b in self.engine._mirror["gen_budget"])
        self._new_window(self.engine.demand())

    # -- one iteration -------------------------------------------------------------------------
    def _fetch_result(self) -> Result:
        P, D, C, E = self.engine.get_primal()
        inj, aU, aK, flow, cost = self.engine.get_consensus()
        u2r: Dict[int, object] = {}
        prev = self.results[-1] if self.results else None
        G = len(self.generators)

        def extras(a, delta):
            if not self.record_slacks:
                return {}
            U, K = self.engine.get_agent_slacks(a)
            return dict(U=U, K=K, penalty_term=PenaltyTerm(*self.engine.get_agent_penalty(a, delta=delta)))
        for i, g in enumerate(self.generators):
            d = P[i] - (prev.of(g).generation if prev else 0.0)
            u2r[id(g)] = ResultGenerator(g, P[i].copy(), **extras(i, d))
        for i, s in enumerate(self.storages):
            q0 = (prev.of(s).discharge - prev.of(s).charge) if prev else 0.0
            u2r[id(s)] = ResultStorage(s, D[i].copy(), C[i].copy(), E[i].copy(), **extras(G + i, (D[i] - C[i]) - q0))
        T = self.packed.T
        if hasattr(self.engine.api, "get_node_results"):        # dopf_get_node_results (the device adds the units of a node)
            ng, nd, nc = self.engine.get_node_results()
        else:                                                   # a backend without it: the same sums here
            ng, nd, nc = (np.zeros((self.packed.N, T)) for _ in range(3))
            np.add.at(ng, np.asarray(self.packed.gen_node, dtype=np.int64), P)
            np.add.at(nd, np.asarray(self.packed.sto_node, dtype=np.int64), D)
            np.add.at(nc, np.asarray(self.packed.sto_node, dtype=np.int64), C)
        n2r = {id(n): ResultNode(n, ng[i].copy(), nd[i].copy(), nc[i].copy()) for i, n in enumerate(self.nodes)}
        pen = None
        if self.record_slacks:
            # Result.penalty_term = sum_up over the units (results.jl:66-70, helpers/penalty_terms.jl:1-6): one pass on the device
            # where it holds the injection changes (networks), else the sum of the per-unit terms fetched above
            if self.packed.L > 0 and hasattr(self.engine.api, "get_penalty_sums"):
                pen = PenaltyTerm(*self.engine.get_penalty_sums())
            else:
                terms = [r.penalty_term for r in u2r.values()]
                pen = PenaltyTerm(*(sum(getattr(t_, f) for t_ in terms) for f in ("energy_balance", "upper_flow", "lower_flow")))
        return Result(u2r, P.sum(axis=0) if P.size else np.zeros(T), D.sum(axis=0) if D.size else np.zeros(T),
                      C.sum(axis=0) if C.size else np.zeros(T), aU, aK, cost, inj, flow, n2r, pen)

    def _after(self, done: int):
        lam_res, mu_res, rho_res, it = self.engine.get_residuals()
        _, conv = self.engine.sync()
        if done and (self.iteration != 1 or done > 1):
            c = self.convergence
            if self.record and len(self.lambdas) >= 2:       # the reference's per-entry residuals (convergence.jl:5-12)
                c.lambda_res.append(np.abs(self.lambdas[-1] - self.lambdas[-2]))
                c.mue_res.append(np.abs(self.mues[-1] - self.mues[-2]))
                c.rho_res.append(np.abs(self.rhos[-1] - self.rhos[-2]))
            else:
                c.lambda_res.append(lam_res)
                c.mue_res.append(mu_res)
                c.rho_res.append(rho_res)
            eps = self.params.eps
            c.lambda_, c.mue, c.rho = lam_res < eps, mu_res < eps, rho_res < eps
        self.convergence.all = bool(conv)
        self.iteration = it


def calculate_iteration(admm: ADMM) -> None:
    """One ADMM iteration: all sub-problems, dual update, stop test."""
    done, _ = admm.engine.iterate(1)
    if done and admm.record:
        admm.results.append(admm._fetch_result())
        lam, mu, rho = admm.engine.get_duals()
        admm.lambdas.append(lam)
        admm.mues.append(mu)
        admm.rhos.append(rho)
    admm._after(done)


def run(admm: ADMM, chunk: int = 64) -> ADMM:
    """run!(admm): iterate until Convergence.all (or the optional cap `max_iters`)."""
    cap = admm.params.max_iters
    while not admm.convergence.all and not (cap > 0 and admm.iteration > cap):
        if admm.record:
            calculate_iteration(admm)
        else:
            done, _ = admm.engine.iterate(chunk)
            admm._after(done)
            if done == 0:
                break
    if not admm.record:
        admm.results = [admm._fetch_result()]
        admm.lambdas = [admm.engine.get_duals_used()[0], admm.engine.get_duals()[0]]
        admm.mues = [admm.engine.get_duals_used()[1], admm.engine.get_duals()[1]]
        admm.rhos = [admm.engine.get_duals_used()[2], admm.engine.get_duals()[2]]
    return admm


def _result_of_slot(admm: ADMM, sl: dict, i: int) -> Result:
    """The Result of slot i of a trace read (Engine.trace_read with all sections): what ADMM._fetch_result builds from the getters
    after that iteration. The node results are summed here, in NumPy, from the slot's P, D and C."""
    p = admm.packed
    P, D, C, E = sl["P"][i], sl["D"][i], sl["C"][i], sl["E"][i]
    u2r: Dict[int, object] = {}
    for k, g in enumerate(admm.generators):
        u2r[id(g)] = ResultGenerator(g, P[k].copy())
    for k, s in enumerate(admm.storages):
        u2r[id(s)] = ResultStorage(s, D[k].copy(), C[k].copy(), E[k].copy())
    ng, nd, nc = (np.zeros((p.N, p.T)) for _ in range(3))
    np.add.at(ng, np.asarray(p.gen_node, dtype=np.int64), P)
    np.add.at(nd, np.asarray(p.sto_node, dtype=np.int64), D)
    np.add.at(nc, np.asarray(p.sto_node, dtype=np.int64), C)
    n2r = {id(n): ResultNode(n, ng[k].copy(), nd[k].copy(), nc[k].copy()) for k, n in enumerate(admm.nodes)}
    return Result(u2r, P.sum(axis=0) if P.size else np.zeros(p.T), D.sum(axis=0) if D.size else np.zeros(p.T),
                  C.sum(axis=0) if C.size else np.zeros(p.T), sl["avg_U"][i].copy(), sl["avg_K"][i].copy(), float(sl["total_cost"][i]),
                  sl["inj"][i].copy(), sl["flow"][i].copy(), n2r, None)


def run_recorded(admm: ADMM, chunk: int = 64) -> ADMM:
    """run(admm) with the history recorded on the device (dopf_trace_*): the iterations run `chunk` at a time, back to back, each
    writing its slot of a device ring, and the host reads a chunk's slots afterwards — one round trip per chunk where run makes
    one, and five to seven blocking copies, per iteration. Appends to admm.results, lambdas, mues, rhos and convergence exactly
    what run appends. Needs ADMM(..., record=True); the units' slacks and penalty terms are not in a trace (record_slacks=True:
    ValueError)."""
    if not admm.record:
        raise ValueError("run_recorded records the iteration history: build ADMM(..., record=True) (or call run)")
    if admm.record_slacks:
        raise ValueError("run_recorded: the units' slacks and penalty terms are not part of a trace (record_slacks=True): call run")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"run_recorded: chunk = {chunk} < 1")
    e = admm.engine
    cap, eps = admm.params.max_iters, admm.params.eps
    e.trace_begin(_capi.TRACE_ALL, chunk)
    try:
        while not admm.convergence.all and not (cap > 0 and admm.iteration > cap):
            e.trace_reset()
            done, _ = e.iterate(chunk)
            sl = e.trace_read(0, done)
            c = admm.convergence
            for i in range(done):
                admm.results.append(_result_of_slot(admm, sl, i))
                admm.lambdas.append(sl["lam"][i].copy())
                admm.mues.append(sl["mu"][i].copy())
                admm.rhos.append(sl["rho"][i].copy())
                if admm.iteration != 1:          # (as ADMM._after: the first iteration has no residuals)
                    c.lambda_res.append(np.abs(admm.lambdas[-1] - admm.lambdas[-2]))
                    c.mue_res.append(np.abs(admm.mues[-1] - admm.mues[-2]))
                    c.rho_res.append(np.abs(admm.rhos[-1] - admm.rhos[-2]))
                    c.lambda_, c.mue, c.rho = (float(sl[k][i]) < eps for k in ("lam_res", "mu_res", "rho_res"))
                conv = bool(sl["converged"][i])
                c.all = conv
                admm.iteration = int(sl["iteration"][i]) + (0 if conv else 1)
            if done == 0:           # (halted before the call: the counter and the flag as the engine has them)
                admm._after(0)
                break
    finally:
        e.trace_end()
    return admm


def get_nodal_price(admm: ADMM, iteration: Optional[int] = None) -> np.ndarray:
    """lambda_t + sum_l (mu + rho)[l,t] ptdf[l,:] with the duals of `iteration` (1-based, default
    admm.iteration = the duals the last solve used, as src/opf_admm_decentral.jl:9 does)."""
    if iteration is None or not admm.record:
        return admm.engine.get_nodal_price(0)
    lam, mu, rho = admm.lambdas[iteration - 1], admm.mues[iteration - 1], admm.rhos[iteration - 1]
    return lam[None, :] + admm.ptdf.T @ (mu + rho)


def export_results(admm: ADMM, filename: str, parent_dir: str = "results/") -> None:
    """The three long-format CSVs of src/helpers/output.jl:1-85, byte-compatible in layout:
    <name>_duals.csv (iteration,dual,timestep,line,value; duals lambda, rho, mue; row i = the dual
    USED in iteration i), <name>_generators.csv, <name>_storages.csv (charge before discharge)."""
    if not admm.record:
        raise ValueError("export_results needs the iteration history: build ADMM(..., record=True)")
    os.makedirs(parent_dir, exist_ok=True)
    n_it = min(admm.iteration, len(admm.results))
    T, L = len(admm.T), len(admm.L)
    with open(os.path.join(parent_dir, filename + "_duals.csv"), "w") as f:
        f.write("iteration,dual,timestep,line,value\n")
        for name, hist in (("lambda", admm.lambdas), ("rho", admm.rhos), ("mue", admm.mues)):
            for i in range(1, n_it + 1):
                for t in range(T):
                    if name == "lambda":
                        f.write(f"{i},lambda,{t + 1},,{float(hist[i - 1][t])!r}\n")
                    else:
                        for l in range(L):
                            f.write(f"{i},{name},{t + 1},{l + 1},{float(hist[i - 1][l, t])!r}\n")
    with open(os.path.join(parent_dir, filename + "_generators.csv"), "w") as f:
        f.write("iteration,generator,timestep,generation\n")
        for g in admm.generators:
            for i in range(1, n_it + 1):
                r = admm.results[i - 1].of(g)
                for t in range(T):
                    f.write(f"{i},{g.name},{t + 1},{float(r.generation[t])!r}\n")
    with open(os.path.join(parent_dir, filename + "_storages.csv"), "w") as f:
        f.write("iteration,storage,timestep,charge,discharge\n")
        for s in admm.storages:
            for i in range(1, n_it + 1):
                r = admm.results[i - 1].of(s)
                for t in range(T):
                    f.write(f"{i},{s.name},{t + 1},{float(r.charge[t])!r},{float(r.discharge[t])!r}\n")
