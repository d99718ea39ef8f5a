"""Agents sharded over ranks (one process per GPU), consensus by ONE all-reduce per iteration.

The reference has no parallelism at all; what shards is the agent loop of
optimize_all_subproblems! (src/optimization/subproblems.jl:1-17): every agent reads only iteration
k-1, and the only cross-agent data flow is the sum over agents of nodal injections and slacks
(Result(...), src/structures/results.jl:72-106). Each rank therefore owns a contiguous slice of the
node-sorted agent lists plus a replica of the O((N+L)T) consensus state, and per iteration does

    local_update()      x-updates of its agents + local sums  -> consensus buffer (N*T + 2*L*T + 1)
    all_reduce(SUM)     RCCL over xGMI (backend "nccl"); gloo in the CPU tests
    apply_consensus()   averages, flows, lambda/mu/rho update, residuals, stop test — replicated,
                        so duals stay identical on all ranks without a second collective

`ShardedADMM` is generic over the C-ABI library it drives: the product passes the HIP library and a
CUDA tensor bound as the consensus buffer; the CPU tests pass a host library and a numpy view.
"""
from __future__ import annotations

import ctypes
from typing import Callable, Optional

import numpy as np

from . import _capi
from .network import PackedProblem


def host_consensus_view(engine: _capi.Engine) -> np.ndarray:
    """numpy view of a HOST consensus buffer (host libraries only)."""
    n = engine.consensus_size()
    ptr = engine.consensus_ptr()
    return np.ctypeslib.as_array((ctypes.c_double * n).from_address(ptr))


class ShardedADMM:
    def __init__(self, problem: PackedProblem, rank: int, world: int, *, api: Optional[_capi.CApi] = None,
                 all_reduce: Optional[Callable[[], None]] = None, mode: Optional[int] = None,
                 device: Optional[int] = None, n_agents_global_override: Optional[int] = None, **params):
        self.rank, self.world = rank, world
        self.problem = problem
        self.shard = problem.shard(rank, world)
        self.n_agents_global = n_agents_global_override or (problem.G + problem.S)
        self._tensor = None
        kw = dict(params)
        kw["n_agents_global"] = self.n_agents_global
        if api is None:                       # product path: HIP + RCCL via torch.distributed
            import torch
            import torch.distributed as dist
            if device is None:
                device = torch.cuda.current_device()
            dev = torch.device("cuda", device)
            # one dedicated (non-null) stream carries the kernels AND, as torch's current stream, orders
            # the RCCL all-reduce between dopf_local_update and dopf_apply_consensus
            self.stream = torch.cuda.Stream(device=dev)
            kw["device"] = device
            kw["stream"] = self.stream.cuda_stream
            self.engine = _capi.Engine(_capi.hip_api(), params=_capi.default_params(**kw),
                                       **self.shard.engine_kwargs())
            self._tensor = torch.zeros(self.engine.consensus_size(), dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)
            self.engine.bind_consensus(self._tensor.data_ptr())
            if all_reduce is None:
                if world > 1:
                    t = self._tensor

                    def all_reduce():                 # runs on the engine's stream: step() makes it current
                        dist.all_reduce(t, op=dist.ReduceOp.SUM)
                else:
                    all_reduce = lambda: None
        else:
            self.engine = _capi.Engine(api, params=_capi.default_params(**kw), mode=mode,
                                       **self.shard.engine_kwargs())
            if all_reduce is None:
                if world > 1:
                    raise ValueError("a host library needs an all_reduce callable")
                all_reduce = lambda: None
        self._all_reduce = all_reduce

    def step(self, n: int = 1) -> None:
        """n iterations, enqueued without host synchronisation (converged state is frozen on device)."""
        e = self.engine
        if self._tensor is not None:          # product path: the collective must queue on the kernels' stream
            import torch
            with torch.cuda.stream(self.stream):      # entered once per call, not once per iteration
                for _ in range(n):
                    e.local_update()
                    self._all_reduce()
                    e.apply_consensus()
            return
        for _ in range(n):
            e.local_update()
            self._all_reduce()
            e.apply_consensus()

    def sync(self):
        return self.engine.sync()

    def _mine(self, x, which: str, dtype=np.float64):
        """This rank's slice of a global per-agent array (which: "sto" or "gen"); None stays None."""
        if x is None:
            return None
        a, b = self.shard.meta[which + "_range"]
        return np.asarray(x, dtype=dtype).reshape(self.problem.S if which == "sto" else self.problem.G)[a:b]

    def set_initial_levels(self, e0=None) -> None:
        """All storages' levels before the first timestep (problem.S values, global order; None = all 0): this rank sets its
        slice (dopf_set_storage_initial_level). Needs F_STO_INITIAL_LEVEL in the params; every rank calls it between steps."""
        self.engine.set_initial_levels(self._mine(e0, "sto"))

    def set_terminal_levels(self, lo=None, hi=None) -> None:
        """All storages' terminal bands (problem.S values each, global order; both None = [0, max_level]): this rank sets its
        slice (dopf_set_storage_terminal_level). Needs F_STO_TERMINAL_LEVEL in the params; every rank calls it between steps."""
        self.engine.set_terminal_levels(self._mine(lo, "sto"), self._mine(hi, "sto"))

    def set_efficiency(self, eta_c=None, eta_d=None) -> None:
        """All storages' charge and discharge efficiencies (problem.S values each, global order; both None = all 1): this rank sets
        its slice (dopf_set_storage_efficiency). Needs F_STO_EFFICIENCY in the params; every rank calls it between steps."""
        self.engine.set_efficiency(self._mine(eta_c, "sto"), self._mine(eta_d, "sto"))

    def set_line_rating(self, rating=None) -> None:
        """The lines' limits per timestep ((L, T); None = f_max in every timestep): replicated state, so this rank sets the whole
        table (dopf_set_line_rating; no sums move). Needs F_LINE_RATING in the params; every rank calls it with the same table
        between the same two steps."""
        self.engine.set_line_rating(rating)

    def set_quadratic_cost(self, c2=None) -> None:
        """All generators' quadratic cost coefficients (problem.G values >= 0, global order; None = all 0): this rank sets its slice
        (dopf_set_generator_quadratic_cost; the cost is local to the rank's agents, no sums move). Needs F_GEN_QUADRATIC_COST in the
        params; every rank calls it between the same two steps."""
        self.engine.set_quadratic_cost(self._mine(c2, "gen"))

    def set_min_output(self, p_min=None) -> None:
        """All generators' must-run floors (problem.G values, global order; None = all 0): this rank sets its slice
        (dopf_set_generator_min_output; the bound is local to the rank's agents, no exchange). Every rank must call it."""
        self.engine.set_min_output(self._mine(p_min, "gen"))

    def set_budget_min_output(self, p_min=None) -> None:
        """All generators' must-run floors on a run with energy budgets (problem.G values, global order; None removes them): this
        rank sets its slice (dopf_set_generator_budget_min_output; the bound is local to the rank's agents, no exchange). Needs
        F2_GEN_ENERGY_BUDGET in the second flag word and no F_GEN_RAMP; every rank calls it between the same two steps."""
        self.engine.set_budget_min_output(self._mine(p_min, "gen"))

    def set_ramp(self, up=None, down=None, prev=None) -> None:
        """All generators' ramp limits and (optionally) anchors (problem.G values each, global order; both ramps None = all inf,
        prev None = no anchor): this rank sets its slice (dopf_set_generator_ramp; the constraint is local to the rank's agents, no
        sums move). Needs F_GEN_RAMP in the params; every rank calls it between the same two steps."""
        self.engine.set_ramp(self._mine(up, "gen"), self._mine(down, "gen"), self._mine(prev, "gen"))

    def set_energy_budget(self, e_min=None, e_max=None) -> None:
        """All generators' energy budgets over the window (problem.G values each, global order; e_min None = all 0, e_max None = all
        inf): this rank sets its slice (dopf_set_generator_energy_budget; the constraint is local to the rank's agents, no sums
        move). Needs F2_GEN_ENERGY_BUDGET in the second flag word; every rank calls it between the same two steps."""
        self.engine.set_energy_budget(self._mine(e_min, "gen"), self._mine(e_max, "gen"))

    def set_energy_budget_windows(self, win_end=None, e_min=None, e_max=None) -> None:
        """All generators' energy budgets per sub-window (win_end: the windows' ends, the same on every rank; e_min / e_max:
        (problem.G, n_win), global order, None = all 0 / all inf; win_end None removes the table): this rank sets the ends and its rows
        (dopf_set_generator_energy_budget_windows; the constraint is local to the rank's agents, no sums move). Needs
        F2_GEN_ENERGY_BUDGET in the second flag word; every rank calls it between the same two steps."""
        self.engine.set_energy_budget_windows(win_end, self._mine_rows(e_min), self._mine_rows(e_max))

    def _mine_rows(self, x):
        """This rank's rows of a global (problem.G, n) array; None stays None."""
        if x is None:
            return None
        a, b = self.shard.meta["gen_range"]
        return np.asarray(x, dtype=np.float64).reshape(self.problem.G, -1)[a:b]

    def energy_budget_windows(self):
        """This rank's (win_end, e_min, e_max) as its context holds them (its generators' rows), or None while no table is set."""
        return self.engine.energy_budget_windows()

    def budget_window_price(self, all_reduce: Optional[Callable[[np.ndarray], np.ndarray]] = None) -> np.ndarray:
        """All generators' window prices ((problem.G, n_win), global order): this rank's rows (dopf_get_generator_budget_window_price)
        in an array of zeros, summed over the ranks as budget_price does: torch.distributed on the product path (every rank must
        call), a caller's all_reduce (array -> the ranks' sum) otherwise; one rank needs neither."""
        a, b = self.shard.meta["gen_range"]
        mine = np.asarray(self.engine.budget_window_price(), dtype=np.float64)
        out = np.zeros((self.problem.G, mine.shape[1]))
        out[a:b] = mine
        if all_reduce is not None:
            return np.asarray(all_reduce(out), dtype=np.float64)
        if self.world == 1:
            return out
        if self._tensor is None:
            raise ValueError("a host library needs an all_reduce callable")
        import torch
        import torch.distributed as dist
        t = torch.from_numpy(out).to(self._tensor.device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t.cpu().numpy()

    def budget_price(self, all_reduce: Optional[Callable[[np.ndarray], np.ndarray]] = None) -> np.ndarray:
        """All generators' budget prices (problem.G values, global order): this rank's slice (dopf_get_generator_budget_price; the
        price is local to the rank's agents) in a vector of zeros, summed over the ranks — every entry has one owner, so the sum
        gathers. On the product path the sum is a torch.distributed all-reduce on the rank's device, and every rank must call; a host
        library, or a caller that moves the data itself, passes all_reduce (vector -> the ranks' sum). One rank needs neither. As
        Engine.budget_price: the first call starts the recording and returns zeros."""
        a, b = self.shard.meta["gen_range"]
        out = np.zeros(self.problem.G)
        out[a:b] = self.engine.budget_price()
        if all_reduce is not None:
            return np.asarray(all_reduce(out), dtype=np.float64)
        if self.world == 1:
            return out
        if self._tensor is None:
            raise ValueError("a host library needs an all_reduce callable")
        import torch
        import torch.distributed as dist
        t = torch.from_numpy(out).to(self._tensor.device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t.cpu().numpy()

    def ramp_price(self, all_reduce: Optional[Callable[[np.ndarray], np.ndarray]] = None) -> np.ndarray:
        """All generators' ramp prices ((problem.G, T), global order): this rank's rows (dopf_get_generator_ramp_price; the price is
        local to the rank's rows) in an array of zeros, summed over the ranks — every entry has one owner, so the sum gathers — as
        budget_price does: torch.distributed on the product path (every rank must call), a caller's all_reduce (array -> the ranks'
        sum) otherwise; one rank needs neither. As Engine.ramp_price: the first call starts the recording and returns zeros."""
        a, b = self.shard.meta["gen_range"]
        mine = np.asarray(self.engine.ramp_price(), dtype=np.float64)
        out = np.zeros((self.problem.G, mine.shape[1]))
        out[a:b] = mine
        if all_reduce is not None:
            return np.asarray(all_reduce(out), dtype=np.float64)
        if self.world == 1:
            return out
        if self._tensor is None:
            raise ValueError("a host library needs an all_reduce callable")
        import torch
        import torch.distributed as dist
        t = torch.from_numpy(out).to(self._tensor.device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t.cpu().numpy()

    def set_availability(self, profiles=None, profile_of=None) -> None:
        """The generators' availability (K x T profiles, problem.G indices in global order; both None = every generator at
        max_generation): this rank sets the whole table and its slice of the indices (dopf_set_generator_availability). Needs
        F_GEN_AVAILABILITY in the params; every rank calls it between steps."""
        self.engine.set_availability(profiles, self._mine(profile_of, "gen", np.int32))

    def run(self, max_iters: int, check_every: int = 16):
        """Iterate until the stop test holds (checked every `check_every` iterations) or max_iters."""
        done = 0
        while done < max_iters:
            n = min(check_every, max_iters - done)
            self.step(n)
            done += n
            it, conv = self.sync()
            if conv:
                return it, True
        return self.sync()

    def gather_primal(self):
        """This rank's slice of P, D, C, E with the global index ranges it covers."""
        P, D, C, E = self.engine.get_primal()
        return dict(gen_range=self.shard.meta["gen_range"], sto_range=self.shard.meta["sto_range"],
                    P=P, D=D, C=C, E=E)
