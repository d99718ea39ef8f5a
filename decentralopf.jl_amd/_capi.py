"""ctypes binding of the C ABI declared in include/dopf.h.

The product library is csrc/libdopf_hip.so (hand-written HIP for gfx950). There is NO CPU
fallback: if the library is missing or HIP cannot start, loading raises.

``CApi`` is generic over the symbol prefix so that another library exporting the same
signatures can be driven by the same Engine class (the test suite's checker does that from
oracle/binding.py); nothing in this package knows about such a library.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, NamedTuple, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.path.join(_HERE, "csrc", "libdopf_hip.so")

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)


class DopfProblem(C.Structure):
    _fields_ = [
        ("N", C.c_int32), ("L", C.c_int32), ("T", C.c_int32), ("G", C.c_int32), ("S", C.c_int32),
        ("demand", c_double_p), ("ptdf", c_double_p), ("f_max", c_double_p),
        ("gen_mc", c_double_p), ("gen_pmax", c_double_p), ("gen_node", c_int32_p),
        ("sto_mc", c_double_p), ("sto_pmax", c_double_p), ("sto_emax", c_double_p),
        ("sto_node", c_int32_p),
    ]


class DopfParams(C.Structure):
    _fields_ = [
        ("gamma", C.c_double), ("w_flow", C.c_double), ("w_prox", C.c_double),
        ("eps", C.c_double), ("mask_thr", C.c_double),
        ("max_iters", C.c_int32), ("n_agents_global", C.c_int32),
        ("device", C.c_int32), ("flags", C.c_int32),
        ("stream", C.c_void_p),
    ]


class DopfTiming(C.Structure):
    _fields_ = [("tables_ms", C.c_double), ("gen_ms", C.c_double), ("sto_ms", C.c_double),
                ("slack_ms", C.c_double), ("reduce_ms", C.c_double), ("dual_ms", C.c_double),
                ("iter_ms", C.c_double), ("empty_ms", C.c_double), ("iters", C.c_int32),
                ("agents_fused", C.c_int32), ("tail_fused", C.c_int32),
                ("slack_in_dual", C.c_int32), ("quiet", C.c_int32), ("sto_lean", C.c_int32), ("persist", C.c_int32),
                ("sto_long", C.c_int32)]


class DopfCentralResult(C.Structure):
    _fields_ = [("objective", C.c_double), ("dual_objective", C.c_double), ("primal_infeasibility", C.c_double),
                ("gap", C.c_double), ("iterations", C.c_int32), ("converged", C.c_int32)]


F_NO_GRAPH = 1
F_OVERLAP_AGENTS = 2
F_NO_WARM_START = 4
F_NO_ROW_SKIP = 8
F_NO_TAIL_FUSE = 4096
F_TIME_CALLS = 8192
F_NO_FUSE = 16
F_COMM_HOST = 64
F_DEBUG_ROOT_CAP = 128
F_KEEP_DELTAS = 256
F_COMM_GRAPH = 512
F_COMM_P2P = 1024
F_DEBUG_LEAVE = 2048
F_STO_GENERAL = 16384
F_NO_QUIET = 32768
F_XCHG_OWNER = 65536
F_XCHG_ALLGATHER = 131072
F_NO_TAIL_XCHG = 262144
F_NET_SMALL_ITEMS = 524288
F_PERSIST = 1048576  # retired: accepted, has no effect
F_LONG_HORIZON = 2097152
F_DEBUG_LONG_STO = 4194304
F_WIDE_NETWORK = 8388608
F_DEBUG_WIDE_NET = 16777216
F_STO_INITIAL_LEVEL = 33554432
F_STO_TERMINAL_LEVEL = 67108864
F_GEN_AVAILABILITY = 134217728
F_STO_EFFICIENCY = 268435456
F_LINE_RATING = 536870912
F_GEN_QUADRATIC_COST = 1073741824
F_GEN_RAMP = 32
F_GEN_RAMP_NETWORK = 2147483648  # bit 31, the last of the int32 flag word (ctypes stores it as the sign bit; test it with `& ... != 0`)
F2_GEN_ENERGY_BUDGET = 1  # the second flag word (DOPF_F2_*): the flags2 argument of dopf_create_ex / dopf_multi_create_ex
F2_GEN_RAMP_BUDGET = 8  # ... ramp limits and energy budgets on the same generators (copper plates): the opt-in of the pair search's scratch
COMM_ID_BYTES = 128
XCHG_HANDLE_BYTES = 64
TRACE_DUALS = 1       # dopf_trace_begin's `what` (DOPF_TRACE_*): lambda, mu, rho
TRACE_CONSENSUS = 2   # injection, avg_U, avg_K, line_util
TRACE_PRIMAL = 4      # P, D, C (E is derived when read)
TRACE_ALL = 7


class DopfError(RuntimeError):
    pass


def _f64(a, n=None) -> np.ndarray:
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if n is not None and arr.size != n:
        raise ValueError(f"expected {n} doubles, got {arr.size}")
    return arr


def _i32(a, n=None) -> np.ndarray:
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
    if n is not None and arr.size != n:
        raise ValueError(f"expected {n} int32, got {arr.size}")
    return arr


def _dp(arr: Optional[np.ndarray]):
    return None if arr is None else arr.ctypes.data_as(c_double_p)


class CApi:
    """One loaded shared library exporting <prefix>create/iterate/... (include/dopf.h)."""

    def __init__(self, path: str, prefix: str = "dopf_", create_extra=()):
        if not os.path.exists(path):
            raise DopfError(
                f"{path} not found: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
                "There is no CPU fallback for the HIP path.")
        self.path = path
        self.prefix = prefix
        self.lib = C.CDLL(path)
        p = prefix
        L = self.lib
        ctxp = C.c_void_p
        self.has_mode = bool(create_extra)          # <prefix>create takes extra trailing arguments
        create = getattr(L, p + "create")
        create.restype = C.c_int
        create.argtypes = [C.POINTER(ctxp), C.POINTER(DopfProblem), C.POINTER(DopfParams)] + list(create_extra)
        self._create = create
        self._sig("destroy", None, [ctxp])
        self._sig("last_error", C.c_char_p, [ctxp])
        self._sig("iterate", C.c_int, [ctxp, C.c_int32, c_int32_p, c_int32_p])
        self._sig("local_update", C.c_int, [ctxp])
        self._sig("apply_consensus", C.c_int, [ctxp])
        self._sig("consensus_size", C.c_int64, [ctxp])
        self._sig("consensus_ptr", C.c_void_p, [ctxp])
        self._sig("sync", C.c_int, [ctxp, c_int32_p, c_int32_p])
        self._sig("get_duals", C.c_int, [ctxp, c_double_p, c_double_p, c_double_p])
        self._sig("get_duals_used", C.c_int, [ctxp, c_double_p, c_double_p, c_double_p])
        self._sig("get_primal", C.c_int, [ctxp, c_double_p, c_double_p, c_double_p, c_double_p])
        self._sig("get_consensus", C.c_int, [ctxp, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p])
        self._sig("get_residuals", C.c_int, [ctxp, c_double_p, c_double_p, c_double_p, c_int32_p])
        self._sig("get_nodal_price", C.c_int, [ctxp, C.c_int32, c_double_p])
        self._sig("set_state", C.c_int, [ctxp] + [c_double_p] * 8 + [C.c_int32])
        # the receding-horizon entries: optional — a library of the same ABI may lack them (Engine.roll then goes the host route)
        self._opt("set_demand", C.c_int, [ctxp, c_double_p])
        self._opt("roll_horizon", C.c_int, [ctxp, C.c_int32, c_double_p])
        # ... for contexts with ramp limits or energy budgets (Engine.roll_coupled), and the getter its mirrors follow
        self._opt("roll_horizon_coupled", C.c_int, [ctxp, C.c_int32, c_double_p, C.c_int32, c_double_p, c_int32_p, C.c_int32,
                                                    c_double_p, c_double_p])
        self._opt("get_generator_coupling", C.c_int, [ctxp] + [c_double_p] * 5)
        self._opt("get_generator_min_output", C.c_int, [ctxp, c_double_p])
        # the budget rows' multipliers of the last x-update (Engine.budget_price, MultiEngine.budget_price)
        self._opt("get_generator_budget_price", C.c_int, [ctxp, c_double_p])
        self._opt("multi_get_generator_budget_price", C.c_int, [ctxp, c_double_p])
        # budgets per sub-window (Engine.set_energy_budget_windows, .energy_budget_windows, .budget_window_price and MultiEngine's): no
        # flag of their own, so they travel beside the extension tables, as the price getters do
        self._opt("set_generator_energy_budget_windows", C.c_int, [ctxp, C.c_int32, c_int32_p, c_double_p, c_double_p])
        self._opt("get_generator_energy_budget_windows", C.c_int, [ctxp, c_int32_p, c_int32_p, c_double_p, c_double_p])
        self._opt("get_generator_budget_window_price", C.c_int, [ctxp, c_double_p])
        self._opt("multi_set_generator_energy_budget_windows", C.c_int, [ctxp, C.c_int32, c_int32_p, c_double_p, c_double_p])
        self._opt("multi_get_generator_budget_window_price", C.c_int, [ctxp, c_double_p])
        # must-run floors on budget contexts (Engine.set_budget_min_output, .budget_min_output and MultiEngine's): no flag of their own
        # either, and the extension tables are full — beside them, as the window entries
        self._opt("set_generator_budget_min_output", C.c_int, [ctxp, c_double_p])
        self._opt("get_generator_budget_min_output", C.c_int, [ctxp, c_double_p])
        self._opt("multi_set_generator_budget_min_output", C.c_int, [ctxp, c_double_p])
        # the ramp rows' multipliers of the last x-update (Engine.ramp_price, MultiEngine.ramp_price)
        self._opt("get_generator_ramp_price", C.c_int, [ctxp, c_double_p])
        self._opt("multi_get_generator_ramp_price", C.c_int, [ctxp, c_double_p])
        if prefix == "dopf_":
            self._sig("bind_consensus", C.c_int, [ctxp, C.c_void_p])
            self._sig("solver_failures", C.c_int64, [ctxp])
            self._sig("iterate_timed", C.c_int, [ctxp, C.c_int32, C.POINTER(DopfTiming)])
            self._sig("wide_net", C.c_int, [ctxp, c_int32_p])
            self._sig("debug_stats", C.c_int, [ctxp, C.POINTER(C.c_uint64)])
            self._sig("version", C.c_char_p, [])
            self._sig("default_params", None, [C.POINTER(DopfParams)])
            self._sig("get_agent_slacks", C.c_int, [ctxp, C.c_int32, c_double_p, c_double_p])
            self._sig("get_agent_penalty", C.c_int, [ctxp, C.c_int32, c_double_p, c_double_p])
            self._sig("get_residual_vectors", C.c_int, [ctxp, c_double_p, c_double_p, c_double_p])
            self._sig("get_penalty_sums", C.c_int, [ctxp, c_double_p])
            self._sig("central_solve", C.c_int, [C.POINTER(DopfProblem), C.POINTER(DopfParams), C.c_double, C.c_int32,
                                                 C.POINTER(DopfCentralResult)] + [c_double_p] * 9)
            self._sig("central_solve_ex", C.c_int, [C.POINTER(DopfProblem), C.POINTER(DopfParams), c_double_p, c_double_p, c_double_p,
                                                    C.c_int32, c_double_p, c_int32_p, C.c_double, C.c_int32,
                                                    C.POINTER(DopfCentralResult)] + [c_double_p] * 9)
            self._sig("central_solve_lossy", C.c_int, [C.POINTER(DopfProblem), C.POINTER(DopfParams)] + [c_double_p] * 5 +
                                                      [C.c_int32, c_double_p, c_int32_p, C.c_double, C.c_int32,
                                                       C.POINTER(DopfCentralResult)] + [c_double_p] * 9)
            # ... plus line_rating, ramp_up, ramp_down, p_prev, e_min, e_max in front of tol, and ramp_dual, budget_dual at the end
            self._sig("central_solve_coupled", C.c_int, [C.POINTER(DopfProblem), C.POINTER(DopfParams)] + [c_double_p] * 5 +
                                                        [C.c_int32, c_double_p, c_int32_p] + [c_double_p] * 6 +
                                                        [C.c_double, C.c_int32, C.POINTER(DopfCentralResult)] + [c_double_p] * 11)
            self._sig("get_node_results", C.c_int, [ctxp, c_double_p, c_double_p, c_double_p])
            self._sig("last_call_ms", C.c_double, [ctxp])
            # the iteration history on the device (Engine.trace_*)
            self._sig("trace_begin", C.c_int, [ctxp, C.c_int32, C.c_int32])
            self._sig("trace_end", C.c_int, [ctxp])
            self._sig("trace_reset", C.c_int, [ctxp])
            self._sig("trace_info", C.c_int, [ctxp] + [c_int32_p] * 4)
            self._sig("trace_read", C.c_int, [ctxp, C.c_int32, C.c_int32, c_double_p, c_int32_p, c_int32_p] + [c_double_p] * 11)
            # consensus sum across GPUs inside the library (RCCL, loaded on first use)
            self._sig("comm_unique_id", C.c_int, [C.c_void_p])
            self._sig("comm_init", C.c_int, [ctxp, C.c_int32, C.c_int32, C.c_void_p])
            self._sig("xchg_export", C.c_int, [ctxp, C.c_int32, C.c_void_p])
            self._sig("xchg_init", C.c_int, [ctxp, C.c_int32, C.c_int32, C.c_void_p])
            self._sig("comm_info", C.c_int, [ctxp, c_int32_p, c_int32_p, c_int32_p])
            self._sig("multi_create", C.c_int, [C.POINTER(ctxp), C.POINTER(DopfProblem), C.POINTER(DopfParams), C.c_int32, c_int32_p])
            self._sig("multi_destroy", None, [ctxp])
            self._sig("multi_last_error", C.c_char_p, [ctxp])
            self._sig("multi_iterate", C.c_int, [ctxp, C.c_int32, c_int32_p, c_int32_p])
            self._sig("multi_get_primal", C.c_int, [ctxp, c_double_p, c_double_p, c_double_p, c_double_p])
            self._sig("multi_size", C.c_int32, [ctxp])
            self._sig("multi_ctx", ctxp, [ctxp, C.c_int32])
            # the creates with the second flag word (Engine and MultiEngine call them only with a non-zero word)
            self._sig("create_ex", C.c_int, [C.POINTER(ctxp), C.POINTER(DopfProblem), C.POINTER(DopfParams), C.c_int32])
            self._sig("multi_create_ex", C.c_int, [C.POINTER(ctxp), C.POINTER(DopfProblem), C.POINTER(DopfParams), C.c_int32, c_int32_p,
                                                   C.c_int32])
        # the problem extensions' setters (EXTENSIONS below). The older three belong to the HIP library's ABI; the later three are bound
        # wherever the library exports them — the oracle backend loads without them (Engine's setter then refuses)
        for x in _ALL_EXTENSIONS:
            if x.optional or prefix == "dopf_":
                for name in (x.entry, "multi_" + x.entry):
                    (self._opt if x.optional else self._sig)(name, C.c_int, [ctxp] + list(x.argtypes))

    def _opt(self, name, restype, argtypes):
        if hasattr(self.lib, self.prefix + name):
            self._sig(name, restype, argtypes)

    def _sig(self, name, restype, argtypes):
        f = getattr(self.lib, self.prefix + name)
        f.restype = restype
        f.argtypes = argtypes
        setattr(self, name, f)


_hip_api: Optional[CApi] = None
_runtime_pinned = False


def _pin_hip_runtime():
    """One HIP runtime per process. PyTorch's wheels bundle their own libamdhip64.so / libhsa-runtime64.so (same SONAMEs as
    the system ROCm's, requested under another file name), so a process that loads libdopf_hip.so first (system runtime) and
    imports torch later ends up with TWO runtimes: the second one finds no GPU ("No HIP GPUs are available"), and a system
    RCCL bound to the other copy's runtime is an ABI mismatch. When PyTorch is installed but not imported yet, its copy of the
    runtime is loaded here first: libdopf_hip.so's DT_NEEDED libamdhip64.so.7 then binds to it by SONAME, and a later
    `import torch` finds its runtime already in place. Without PyTorch (a C or Julia host) nothing happens: system ROCm."""
    global _runtime_pinned
    if _runtime_pinned:
        return
    _runtime_pinned = True
    import sys
    if "torch" in sys.modules:
        return                          # its runtime is loaded already; ours will bind to it
    try:
        with open("/proc/self/maps") as f:
            if "libamdhip64" in f.read():
                return                  # a HIP runtime is mapped already (whoever loaded it): never add a second one
    except OSError:
        pass
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return                  # (an unusable bundle: leave everything to the system runtime)


def hip_api() -> CApi:
    """The product library. Raises (never falls back) if it is not built or cannot load."""
    global _hip_api
    if _hip_api is None:
        _pin_hip_runtime()
        _hip_api = CApi(HIP_LIB_PATH, "dopf_")
    return _hip_api


def default_params(**kw) -> DopfParams:
    """The reference's literals: gamma 0.3, flow weight 10, prox 1,
    eps 1e-3, mask threshold 1e-2."""
    q = DopfParams(gamma=0.3, w_flow=10.0, w_prox=1.0, eps=1e-3, mask_thr=1e-2, max_iters=0,
                   n_agents_global=0, device=-1, flags=0, stream=None)
    for k, v in kw.items():
        if not hasattr(q, k):
            raise TypeError(f"unknown parameter {k}")
        setattr(q, k, v)
    return q


def _problem(N, L, T, demand, ptdf, f_max, gen_mc, gen_pmax, gen_node, sto_mc, sto_pmax, sto_emax, sto_node):
    """(prob, keep, G, S): the dopf_problem of the ten base arrays, and the arrays its pointers point into (keep them alive)."""
    gen_mc, sto_mc = _f64(gen_mc), _f64(sto_mc)
    G, S = gen_mc.size, sto_mc.size
    keep = dict(demand=_f64(demand, N * T), ptdf=_f64(ptdf, L * N), f_max=_f64(f_max, L), gen_mc=gen_mc,
                gen_pmax=_f64(gen_pmax, G), gen_node=_i32(gen_node, G), sto_mc=sto_mc, sto_pmax=_f64(sto_pmax, S),
                sto_emax=_f64(sto_emax, S), sto_node=_i32(sto_node, S))
    prob = DopfProblem(N=N, L=L, T=T, G=G, S=S)
    for k, v in keep.items():
        setattr(prob, k, v.ctypes.data_as(c_int32_p if v.dtype == np.int32 else c_double_p))
    return prob, keep, G, S


def _rating_buffer(rating, L: int, T: int) -> np.ndarray:
    """An (L, T) table as the C ABI's [l + L*t] buffer."""
    return _f64(np.asarray(rating, dtype=np.float64).reshape(L, T).T, L * T)


def _availability_arrays(profiles, profile_of, T: int, G: int):
    """(K, profiles as float64 [t + T*k], profile_of as int32 (G,)) from a (K, T) array (or None) and G indices (or None)."""
    if profiles is None and profile_of is None:
        return 0, None, None
    prof = np.zeros((0, T)) if profiles is None else np.asarray(profiles, dtype=np.float64).reshape(-1, T)
    of = None if profile_of is None else _i32(profile_of, G)
    return int(prof.shape[0]), np.ascontiguousarray(prof).ravel(), of


# ---- the problem extensions ------------------------------------------------------------------------------------------------------
# One row per optional input of the problem; CApi, Engine and MultiEngine read everything they do about an extension from its row.
# `d` is whoever knows the sizes (an Engine or MultiEngine: d.L, d.T, d.G, d.S), `keep` the base arrays of _problem.

class Extension(NamedTuple):
    keys: tuple             # the constructor's keyword(s), and the mirror's keys
    flag: int               # the DOPF_F_* that dopf_create needs
    entry: str              # the C entry behind the prefix; "multi_" + entry is the dopf_multi form
    argtypes: tuple         # its ctypes argtypes behind the context
    setter: str             # the method of Engine, MultiEngine, ADMM and ShardedADMM
    what: str               # "this API has no <what>": the setter's refusal on an API without the entry
    why: str                # "this API has no <what> (<why>)": the constructor's refusal of a non-default value there
    norm: Callable          # (d, *values) -> the arrays the entry takes, as the mirror keeps them (None stays None)
    is_default: Callable    # (d, keep, *arrays) -> True where they say what a problem without the extension says
    cargs: Callable = lambda d, *arrays: tuple(_dp(a) for a in arrays)      # (d, *arrays) -> the entry's arguments behind the context
    fill: Optional[Callable] = None     # (d, keep, *arrays) -> arrays: how the constructor completes a value given in part
    mirror: Optional[Callable] = None   # (*arrays) -> {constructor keyword: value} where the keywords are not the arrays one to one
    optional: bool = False  # bound wherever the library exports it, under any prefix, and the setter's refusal ends in " (unsupported)";
    #                         False: part of the "dopf_" ABI, bound under that prefix alone
    word: int = 1           # the flag word `flag` lives in: 1 = dopf_params.flags, 2 = the flags2 argument of dopf_create_ex

    @property
    def packed(self) -> bool:
        """one keyword for several arrays: the constructor and the mirror hold them as a tuple"""
        return len(self.keys) == 1 and len(self.argtypes) > 1

    def refusal(self, api, setter: bool) -> str:
        tail = (" (unsupported)" if self.optional else "") if setter else f" ({self.why})"
        return f"{api.prefix}*: this API has no {self.what}{tail}"


def _per_storage(d, *values):
    return tuple(None if v is None else _f64(v, d.S) for v in values)


def _availability_norm(d, profiles, profile_of):
    K, prof, of = _availability_arrays(profiles, profile_of, d.T, d.G)
    return None if prof is None else prof.reshape(K, d.T), of


def _availability_is_default(d, keep, prof, of):
    used = [] if of is None else sorted({int(k) for k in of if k >= 0})
    return not any(k >= prof.shape[0] or np.any(prof[k] != 1.0) for k in used)


def _availability_cargs(d, prof, of):
    return (0 if prof is None else prof.shape[0], _dp(None if prof is None else prof.ravel()),
            None if of is None else of.ctypes.data_as(c_int32_p))


# in the order the constructors apply them: the efficiencies before the levels, whose reachability checks then see them
EXTENSIONS = (
    Extension(keys=("sto_eta",), flag=F_STO_EFFICIENCY, entry="set_storage_efficiency", argtypes=(c_double_p, c_double_p),
              setter="set_efficiency", optional=True,
              what="storage efficiencies", why="a value other than 1; the reference's storages are lossless",
              norm=_per_storage, is_default=lambda d, keep, ec, ed: not (np.any(ec != 1.0) or np.any(ed != 1.0))),
    Extension(keys=("sto_e0",), flag=F_STO_INITIAL_LEVEL, entry="set_storage_initial_level", argtypes=(c_double_p,),
              setter="set_initial_levels",
              what="storage initial levels", why="non-zero sto_e0; the reference starts every storage empty",
              norm=_per_storage, is_default=lambda d, keep, e0: not np.any(e0 != 0.0)),
    Extension(keys=("sto_end_lo", "sto_end_hi"), flag=F_STO_TERMINAL_LEVEL, entry="set_storage_terminal_level",
              argtypes=(c_double_p, c_double_p), setter="set_terminal_levels",
              what="storage terminal levels", why="a band other than [0, max_level]; the reference leaves the last level free",
              norm=_per_storage, is_default=lambda d, keep, lo, hi: not (np.any(lo != 0.0) or np.any(hi != keep["sto_emax"])),
              fill=lambda d, keep, lo, hi: (np.zeros(d.S) if lo is None else lo, keep["sto_emax"].copy() if hi is None else hi)),
    Extension(keys=("gen_avail", "gen_avail_of"), flag=F_GEN_AVAILABILITY, entry="set_generator_availability",
              argtypes=(C.c_int32, c_double_p, c_int32_p), setter="set_availability",
              what="generator availability",
              why="a profile other than all ones; the reference keeps every generator at max_generation",
              norm=_availability_norm, is_default=_availability_is_default, cargs=_availability_cargs),
    Extension(keys=("line_rating",), flag=F_LINE_RATING, entry="set_line_rating", argtypes=(c_double_p,),
              setter="set_line_rating", optional=True,
              what="line ratings", why="a rating other than f_max; the reference keeps one max_capacity per line",
              norm=lambda d, r: (None if r is None else np.asarray(r, dtype=np.float64).reshape(d.L, d.T),),
              is_default=lambda d, keep, r: not np.any(r != keep["f_max"][:, None]),
              cargs=lambda d, r: (_dp(None if r is None else _rating_buffer(r, d.L, d.T)),)),
    Extension(keys=("gen_c2",), flag=F_GEN_QUADRATIC_COST, entry="set_generator_quadratic_cost", argtypes=(c_double_p,),
              setter="set_quadratic_cost", optional=True,
              what="quadratic generator costs", why="a non-zero gen_c2; the reference keeps one constant marginal_costs per unit",
              norm=lambda d, c2: (None if c2 is None else _f64(c2, d.G),), is_default=lambda d, keep, c2: not np.any(c2 != 0.0)),
)


def _ramp_norm(d, ramp, prev):
    up, down = (None, None) if ramp is None else ramp
    if (up is None) != (down is None):
        raise ValueError("gen_ramp: ramp_up and ramp_down must both be given or both be None")
    return (None if up is None else _f64(up, d.G), None if down is None else _f64(down, d.G), None if prev is None else _f64(prev, d.G))


# The later extensions. EXTENSIONS keeps its six rows (tests/test_extensions_table.py pins them); everything that walks the table
# walks EXTENSIONS + EXTENSIONS_MORE. The ramps come behind the availability, whose caps their check reads.
EXTENSIONS_MORE = (
    Extension(keys=("gen_ramp", "gen_prev"), flag=F_GEN_RAMP, entry="set_generator_ramp", argtypes=(c_double_p, c_double_p, c_double_p),
              setter="set_ramp", optional=True,
              what="generator ramp limits", why="a finite ramp or an anchor; the reference's generators move freely between steps",
              norm=_ramp_norm,
              is_default=lambda d, keep, up, down, prev: prev is None and (up is None or not (np.any(np.isfinite(up)) or np.any(np.isfinite(down)))),
              mirror=lambda up, down, prev: dict(gen_ramp=None if up is None else (up, down), gen_prev=prev)),
)


def _budget_norm(d, e_min, e_max):
    return (None if e_min is None else _f64(e_min, d.G), None if e_max is None else _f64(e_max, d.G))


# The extensions whose flag lives in the second word (DOPF_F2_*: dopf_params.flags is full). The budgets come behind the availability,
# whose caps their check reads.
EXTENSIONS_WORD2 = (
    Extension(keys=("gen_budget",), flag=F2_GEN_ENERGY_BUDGET, word=2, entry="set_generator_energy_budget", argtypes=(c_double_p, c_double_p),
              setter="set_energy_budget", optional=True,
              what="generator energy budgets", why="an energy_min above 0 or a finite energy_max; the reference's generators have no budget over the window",
              norm=_budget_norm,
              is_default=lambda d, keep, lo, hi: not ((lo is not None and np.any(lo != 0.0)) or (hi is not None and np.any(hi != np.inf)))),
)

def _floor_norm(d, p_min):
    """zeros are what None says (the entry's NULL: the context runs the kernels without floors); a NaN passes on to the entry's refusal"""
    if p_min is None:
        return (None,)
    a = _f64(p_min, d.G)
    return (a if np.any(a != 0.0) else None,)


# Minimum output has no flag of its own (both words are spoken for: DESIGN.md 5z): it runs on the ramp kernels, so its row's flag is the
# ramps' — a floor alone creates a ramp context with infinite ramps. Applied behind the ramps, whose limits and anchor its check reads.
EXTENSIONS_FLOOR = (
    Extension(keys=("gen_min_output",), flag=F_GEN_RAMP, entry="set_generator_min_output", argtypes=(c_double_p,),
              setter="set_min_output", optional=True,
              what="generator minimum output", why="a min_generation above 0; the reference's generators may go down to 0",
              norm=_floor_norm, is_default=lambda d, keep, p: p is None or not np.any(p != 0.0)),
)
_ALL_EXTENSIONS = EXTENSIONS + EXTENSIONS_MORE + EXTENSIONS_WORD2 + EXTENSIONS_FLOOR
_BY_SETTER = {x.setter: x for x in _ALL_EXTENSIONS}


def _extensions(api: CApi, params: Optional[DopfParams], d, keep: dict, kw: dict):
    """(params, todo) for a context built with the extensions' constructor keywords in kw: the params with the flags of those given
    added (a copy), and todo, the (extension, arrays) to apply behind create, in the order of EXTENSIONS + EXTENSIONS_MORE + EXTENSIONS_WORD2 +
    EXTENSIONS_FLOOR.
    Nothing to set: a keyword left None, or its default value on an API without the entry (a non-default value there: DopfError). The
    flags of the second word are not in params: _flags2(todo) forms them."""
    todo = []
    for x in _ALL_EXTENSIONS:
        given = [kw.get(k) for k in x.keys]
        if all(v is None for v in given):
            continue
        arrays = x.norm(d, *(given[0] if x.packed else given))
        if all(a is None for a in arrays):
            continue
        if x.fill:
            arrays = x.fill(d, keep, *arrays)
        if not hasattr(api, x.entry):
            if not x.is_default(d, keep, *arrays):
                raise DopfError(x.refusal(api, setter=False))
            continue
        todo.append((x, arrays))
    if any(x.word == 1 for x, _ in todo):
        params = DopfParams.from_buffer_copy(params if params is not None else default_params())
        for x, _ in todo:
            if x.word != 1:
                continue
            params.flags |= x.flag
            if x.flag == F_GEN_RAMP and d.L > 0:       # ramps on a network: the opt-in of k_gen_ramp_net's knot scratch
                params.flags |= F_GEN_RAMP_NETWORK
    return params, todo


def _needs_create_ex(api: CApi, flags2: int) -> None:
    """A non-zero second word on an API without the entry that takes it: refused as the tables' rows refuse (DopfError)."""
    if flags2 and not hasattr(api, "create_ex"):
        raise DopfError(f"{api.prefix}*: this API has no second flag word (no create_ex; flags2 = {flags2})")


def _flags2(todo, L: int = 0) -> int:
    """The second flag word of a context built with todo (what _extensions returned): the flags of its word-2 extensions — and, for
    ramps and budgets together on a copper plate (L == 0), F2_GEN_RAMP_BUDGET, the opt-in of k_gen_ramp_budget's scratch,
    the way _extensions adds F_GEN_RAMP_NETWORK for ramps on a network. With lines it is not added: the library's refusal of the two
    flags together surfaces as it is."""
    word = 0
    for x, _ in todo:
        if x.word == 2:
            word |= x.flag
    setters = {x.setter for x, _ in todo}
    if "set_ramp" in setters and "set_energy_budget" in setters and L == 0:
        word |= F2_GEN_RAMP_BUDGET
    return word


class _ExtensionSetters:
    """What Engine and MultiEngine share of the extensions: the constructor's pass over EXTENSIONS and the one path of every setter.
    The class says which object the entries take (_handle) and which form of the entry (_entry_prefix)."""
    _entry_prefix = ""

    def _set(self, setter: str, *values) -> dict:
        """The extension's entry with the values normalised; returns them as the mirror holds them: {constructor keyword: value}."""
        x = _BY_SETTER[setter]
        fn = getattr(self.api, self._entry_prefix + x.entry, None)
        if fn is None:
            raise DopfError(x.refusal(self.api, setter=True))
        arrays = x.norm(self, *values)
        self._chk(fn(self._handle(), *x.cargs(self, *arrays)))
        if all(a is None for a in arrays):
            return dict.fromkeys(x.keys)
        arrays = tuple(None if a is None else a.copy() for a in arrays)
        if x.mirror:
            return x.mirror(*arrays)
        return {x.keys[0]: arrays} if x.packed else dict(zip(x.keys, arrays))

    def _apply(self, todo) -> None:
        for x, arrays in todo:
            getattr(self, x.setter)(*arrays)

    def set_energy_budget_windows(self, win_end=None, e_min=None, e_max=None):
        """dopf_set_generator_energy_budget_windows (MultiEngine: dopf_multi_...): one energy budget per generator and sub-window of
        the horizon. win_end: the windows' ends (strictly increasing, the last one T; window j covers win_end[j-1] <= t < win_end[j]);
        e_min / e_max: (G, n_win) in the caller's generator order (None = all 0 / all inf). win_end None removes the table. Needs
        F2_GEN_ENERGY_BUDGET without F2_GEN_RAMP_BUDGET, and no whole-horizon budget stored (set_energy_budget(None, None) first). P, D,
        C, the duals and the iteration counter stay; converged becomes False. While a table is set, set_energy_budget with an array,
        budget_price and roll are refused (DopfError). A backend without the entry: DopfError."""
        name = self._entry_prefix + "set_generator_energy_budget_windows"
        fn = getattr(self.api, name, None)
        if fn is None:
            raise DopfError(f"{self.api.prefix}*: this API has no {name}")
        if win_end is None:
            if e_min is not None or e_max is not None:
                raise ValueError("set_energy_budget_windows: budgets without win_end")
            self._chk(fn(self._handle(), 0, None, None, None))
            self._mirror.pop("gen_budget_windows", None)
            return
        ends = np.ascontiguousarray(np.asarray(win_end, dtype=np.int32).reshape(-1))
        n = self.G * ends.size
        lo = None if e_min is None else _f64(np.asarray(e_min, dtype=np.float64).reshape(self.G, ends.size), n)
        hi = None if e_max is None else _f64(np.asarray(e_max, dtype=np.float64).reshape(self.G, ends.size), n)
        self._chk(fn(self._handle(), int(ends.size), ends.ctypes.data_as(c_int32_p), _dp(lo), _dp(hi)))
        self._mirror["gen_budget_windows"] = (ends.copy(), None if lo is None else lo.reshape(self.G, ends.size).copy(),
                                              None if hi is None else hi.reshape(self.G, ends.size).copy())

    def set_budget_min_output(self, p_min=None):
        """dopf_set_generator_budget_min_output (MultiEngine: dopf_multi_...): must-run floors on a budget context — every row's box
        becomes min(p_min, cap) <= P <= cap, the budgets' multiplier search runs inside it, and rows and windows without a budget are
        clamped to it too. p_min: G values in [0, gen_pmax] in the caller's order; None removes the floors (the context runs the
        kernels without them again). An array of zeros is an array: the floor kernels with nothing to hold. Needs F2_GEN_ENERGY_BUDGET
        and no F_GEN_RAMP (ramp contexts have set_min_output). A row whose floors sum above its e_max (or a window's) is refused,
        here and by the budget, window, availability and coupled-roll entries under their new values. P, D, C, the duals and the
        iteration counter stay; converged becomes False. A backend without the entry: DopfError."""
        name = self._entry_prefix + "set_generator_budget_min_output"
        fn = getattr(self.api, name, None)
        if fn is None:
            raise DopfError(f"{self.api.prefix}*: this API has no {name}")
        a = None if p_min is None else _f64(p_min, self.G)
        self._chk(fn(self._handle(), _dp(a)))
        if a is None:
            self._mirror.pop("gen_budget_min_output", None)
        else:
            self._mirror["gen_budget_min_output"] = a.copy()

    def _budget_window_price(self, handle, n_win: int) -> np.ndarray:
        name = self._entry_prefix + "get_generator_budget_window_price"
        if not hasattr(self.api, name):
            raise DopfError(f"{self.api.prefix}*: this API has no {name}")
        out = np.zeros(self.G * max(n_win, 1))
        self._chk(getattr(self.api, name)(handle, _dp(out)))
        return out[:self.G * n_win].reshape(self.G, n_win)


class Engine(_ExtensionSetters):
    """A context of the C ABI with numpy in/out. Mirrors include/dopf.h one to one.
    sto_e0 (optional, S values): the storages' initial levels — sets F_STO_INITIAL_LEVEL and calls
    dopf_set_storage_initial_level after create. sto_end_lo / sto_end_hi (optional, S values each): the band of the level
    after the last timestep — sets F_STO_TERMINAL_LEVEL and calls dopf_set_storage_terminal_level (after the initial levels).
    gen_avail (optional, K x T) / gen_avail_of (optional, G indices in [-1, K)): the generators' availability profiles — sets
    F_GEN_AVAILABILITY and calls dopf_set_generator_availability. sto_eta = (eta_c, eta_d) (optional, S values each): the storages'
    charge and discharge efficiencies — sets F_STO_EFFICIENCY and calls dopf_set_storage_efficiency (before the levels: their
    reachability checks then see the efficiencies). line_rating (optional, (L, T)): the lines' limits per timestep — sets
    F_LINE_RATING and calls dopf_set_line_rating. gen_c2 (optional, G values >= 0): the generators' quadratic cost coefficients —
    sets F_GEN_QUADRATIC_COST and calls dopf_set_generator_quadratic_cost. gen_ramp = (up, down) (optional, G values >= 0 each, inf =
    no limit) / gen_prev (optional, G outputs of the step before the window): the generators' ramp limits and their anchor — sets
    F_GEN_RAMP (on a network F_GEN_RAMP_NETWORK too) and calls dopf_set_generator_ramp (after the availability: its check reads the caps).
    gen_budget = (e_min, e_max) (optional, G values each; either may be None: 0 / inf): the generators' energy budgets over the window —
    sets F2_GEN_ENERGY_BUDGET in the second flag word (self.flags2; the context is then created by dopf_create_ex) and calls
    dopf_set_generator_energy_budget (after the availability too). flags2 (optional): further bits of that word, as Engine.roll passes
    them to the context it rebuilds; on an API without create_ex a non-zero word is a DopfError. gen_min_output (optional, G values in
    [0, gen_pmax]): the generators' must-run floors — sets F_GEN_RAMP (on a network F_GEN_RAMP_NETWORK too: the floors run on the ramp
    kernels) and calls dopf_set_generator_min_output behind the ramps; all zeros is what None says. gen_budget_windows = (win_end,
    e_min, e_max) (optional; (G, n_win) budgets, either may be None): energy budgets per sub-window — sets F2_GEN_ENERGY_BUDGET and calls
    dopf_set_generator_energy_budget_windows behind everything else. gen_budget_min_output (optional, G values in [0, gen_pmax]): must-run
    floors on a budget context — sets F2_GEN_ENERGY_BUDGET and calls dopf_set_generator_budget_min_output last of all (its check reads the
    budgets and the window table)."""

    def __init__(self, api: CApi, *, N, L, T, demand, ptdf, f_max, gen_mc, gen_pmax, gen_node,
                 sto_mc, sto_pmax, sto_emax, sto_node, params: Optional[DopfParams] = None,
                 mode: Optional[int] = None, sto_e0=None, sto_end_lo=None, sto_end_hi=None, gen_avail=None, gen_avail_of=None,
                 sto_eta=None, line_rating=None, gen_c2=None, gen_ramp=None, gen_prev=None, gen_budget=None, flags2: int = 0,
                 gen_min_output=None, gen_budget_windows=None, gen_budget_min_output=None):
        self.api = api
        self.N, self.L, self.T = int(N), int(L), int(T)
        prob, keep, self.G, self.S = _problem(self.N, self.L, self.T, demand, ptdf, f_max, gen_mc, gen_pmax, gen_node,
                                              sto_mc, sto_pmax, sto_emax, sto_node)
        params, todo = _extensions(api, params, self, keep, dict(
            sto_e0=sto_e0, sto_end_lo=sto_end_lo, sto_end_hi=sto_end_hi, gen_avail=gen_avail, gen_avail_of=gen_avail_of,
            sto_eta=sto_eta, line_rating=line_rating, gen_c2=gen_c2, gen_ramp=gen_ramp, gen_prev=gen_prev, gen_budget=gen_budget,
            gen_min_output=gen_min_output))
        self.params = params if params is not None else default_params()
        # (a table of budgets per sub-window runs on a budget context: it asks for the budgets' flag)
        # (and so do floors on budget rows)
        self.flags2 = int(flags2) | _flags2(todo, self.L) | (
            F2_GEN_ENERGY_BUDGET if gen_budget_windows is not None or gen_budget_min_output is not None else 0)
        _needs_create_ex(api, self.flags2)
        # what a window change needs of the problem: the arrays as handed to create, and the inputs of the setters as they stand
        # (by constructor keyword, in the form the constructor takes them)
        self._keep, self._mode, self._mirror = keep, mode, {}
        self._ctx = C.c_void_p()
        args = [C.byref(self._ctx), C.byref(prob), C.byref(self.params)]
        if api.has_mode:
            args.append(C.c_int32(0 if mode is None else mode))
        if self.flags2:
            rc = api.create_ex(*args, C.c_int32(self.flags2))
        else:
            rc = api._create(*args)
        if rc != 0:
            msg = api.last_error(None)
            raise DopfError(f"{api.prefix}create failed ({rc}): {msg.decode() if msg else ''}")
        self._apply(todo)
        if gen_budget_windows is not None:          # (behind the tables' to-do list: its check reads the availability's caps)
            self.set_energy_budget_windows(*gen_budget_windows)
        if gen_budget_min_output is not None:       # (last: its check reads the budgets and the window table)
            self.set_budget_min_output(gen_budget_min_output)

    def _handle(self):
        return self._ctx

    @property
    def _eta(self):
        return self._mirror.get("sto_eta")

    # -- lifecycle -----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self.api.destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            msg = self.api.last_error(self._ctx)
            raise DopfError(f"{self.api.prefix}* failed ({rc}): {msg.decode() if msg else ''}")

    # -- iteration -----------------------------------------------------------------------------
    def iterate(self, n_iters: int):
        done, conv = C.c_int32(0), C.c_int32(0)
        self._chk(self.api.iterate(self._ctx, int(n_iters), C.byref(done), C.byref(conv)))
        return done.value, bool(conv.value)

    def local_update(self):
        self._chk(self.api.local_update(self._ctx))

    def apply_consensus(self):
        self._chk(self.api.apply_consensus(self._ctx))

    def consensus_size(self) -> int:
        return int(self.api.consensus_size(self._ctx))

    def consensus_ptr(self) -> int:
        return int(self.api.consensus_ptr(self._ctx) or 0)

    def bind_consensus(self, device_ptr: int):
        self._chk(self.api.bind_consensus(self._ctx, C.c_void_p(device_ptr)))

    def sync(self):
        it, conv = C.c_int32(0), C.c_int32(0)
        self._chk(self.api.sync(self._ctx, C.byref(it), C.byref(conv)))
        return it.value, bool(conv.value)

    def get_node_results(self):
        """ResultNode.{generation, discharge, charge} of the last result, each (N, T) (src/structures/results.jl:19-35)."""
        outs = [np.zeros(self.N * self.T) for _ in range(3)]
        self._chk(self.api.get_node_results(self._ctx, *[_dp(o) for o in outs]))
        return tuple(o.reshape(self.T, self.N).T.copy() for o in outs)

    def last_call_ms(self) -> float:
        """F_TIME_CALLS: device-side milliseconds of the last iterate() call's launches (-1 if not measured)."""
        return float(self.api.last_call_ms(self._ctx))

    # -- the iteration history on the device (dopf_trace_*) --------------------------------------
    def trace_begin(self, what: int = TRACE_ALL, capacity: int = 64):
        """dopf_trace_begin: from now on every computed iteration of iterate() writes one slot of a device ring of `capacity` slots:
        the row (residuals, total cost, iteration, converged) and the sections `what` selects (TRACE_DUALS | TRACE_CONSENSUS |
        TRACE_PRIMAL; 0 = the row alone). A backend without the entries: DopfError."""
        if not hasattr(self.api, "trace_begin"):
            raise DopfError(f"{self.api.prefix}*: this API has no trace (dopf_trace_*)")
        self._chk(self.api.trace_begin(self._ctx, int(what), int(capacity)))

    def trace_end(self):
        self._chk(self.api.trace_end(self._ctx))

    def trace_reset(self):
        """dopf_trace_reset: recorded = 0 again, same ring, same sections."""
        self._chk(self.api.trace_reset(self._ctx))

    def trace_info(self):
        """(what, capacity, held, recorded); zeros without a trace."""
        v = [C.c_int32(0) for _ in range(4)]
        self._chk(self.api.trace_info(self._ctx, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def trace_read(self, first: int, n: int) -> dict:
        """dopf_trace_read: held slots [first, first + n), oldest first, as a dict of arrays with the slot as the leading axis and
        the getters' shapes behind it: lam_res, mu_res, rho_res, total_cost, iteration, converged (n each), and of the sections the
        trace selected lam (n, T), mu, rho (n, L, T); inj (n, N, T), avg_U, avg_K, flow (n, L, T); P (n, G, T), D, C, E (n, S, T)."""
        what = self.trace_info()[0]
        first, n = int(first), int(n)
        m = max(n, 0)
        N, L, T, G, S = self.N, self.L, self.T, self.G, self.S
        rows = np.zeros(4 * m)
        it, conv = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
        sizes = (("lam", TRACE_DUALS, T), ("mu", TRACE_DUALS, L * T), ("rho", TRACE_DUALS, L * T),
                 ("inj", TRACE_CONSENSUS, N * T), ("avg_U", TRACE_CONSENSUS, L * T), ("avg_K", TRACE_CONSENSUS, L * T),
                 ("flow", TRACE_CONSENSUS, L * T), ("P", TRACE_PRIMAL, G * T), ("D", TRACE_PRIMAL, S * T), ("C", TRACE_PRIMAL, S * T),
                 ("E", TRACE_PRIMAL, S * T))
        buf = {k: (np.zeros(m * size) if what & bit else None) for k, bit, size in sizes}
        self._chk(self.api.trace_read(self._ctx, first, n, _dp(rows), it.ctypes.data_as(c_int32_p), conv.ctypes.data_as(c_int32_p),
                                      *[_dp(buf[k]) for k, _, _ in sizes]))
        r = rows.reshape(m, 4)
        out = dict(lam_res=r[:, 0].copy(), mu_res=r[:, 1].copy(), rho_res=r[:, 2].copy(), total_cost=r[:, 3].copy(),
                   iteration=it, converged=conv)
        cm = lambda v, rows_: v.reshape(m, T, rows_).transpose(0, 2, 1).copy()          # [r + rows*t] per slot -> (rows, T)
        am = lambda v, rows_: v.reshape(m, rows_, T)                                     # [t + T*row] per slot
        if what & TRACE_DUALS:
            out.update(lam=buf["lam"].reshape(m, T), mu=cm(buf["mu"], L), rho=cm(buf["rho"], L))
        if what & TRACE_CONSENSUS:
            out.update(inj=cm(buf["inj"], N), avg_U=cm(buf["avg_U"], L), avg_K=cm(buf["avg_K"], L), flow=cm(buf["flow"], L))
        if what & TRACE_PRIMAL:
            out.update(P=am(buf["P"], G), D=am(buf["D"], S), C=am(buf["C"], S), E=am(buf["E"], S))
        return out

    def solver_failures(self) -> int:
        return int(self.api.solver_failures(self._ctx))

    def iterate_timed(self, n_iters: int) -> dict:
        """HIP-event timing of every kernel of the chain (eager launches), averages in ms."""
        t = DopfTiming()
        self._chk(self.api.iterate_timed(self._ctx, int(n_iters), C.byref(t)))
        out = {k: getattr(t, k) for k, _ in DopfTiming._fields_}
        out["wide_net"] = self.wide_net()
        return out

    def wide_net(self) -> int:
        """1 when this context runs the wide-network chain (F_WIDE_NETWORK beyond 2048 lines, F_DEBUG_WIDE_NET)."""
        w = C.c_int32(0)
        self._chk(self.api.wide_net(self._ctx, C.byref(w)))
        return int(w.value)

    def set_initial_levels(self, e0=None):
        """dopf_set_storage_initial_level: the level of each storage before timestep 0 (S values, None = all 0); needs
        F_STO_INITIAL_LEVEL. Takes effect at the next x-update."""
        self._mirror.update(self._set("set_initial_levels", e0))

    def set_terminal_levels(self, lo=None, hi=None):
        """dopf_set_storage_terminal_level: the band [lo, hi] of each storage's level after the last timestep (S values each;
        both None = the default band [0, max_level]); needs F_STO_TERMINAL_LEVEL. Takes effect at the next x-update."""
        self._mirror.update(self._set("set_terminal_levels", lo, hi))

    def set_efficiency(self, eta_c=None, eta_d=None):
        """dopf_set_storage_efficiency: each storage's charge and discharge efficiency in (0, 1] (S values each; both None = all
        1); needs F_STO_EFFICIENCY. The level then follows E_t = E_{t-1} + eta_c C_t - D_t / eta_d. Takes effect at the next
        x-update. A backend without the entry: DopfError (unsupported)."""
        self._mirror.update(self._set("set_efficiency", eta_c, eta_d))

    def set_line_rating(self, rating=None):
        """dopf_set_line_rating: the lines' limits per timestep, an (L, T) array of finite values >= 0 (None = f_max in every
        timestep); needs F_LINE_RATING. P, D, C, the duals, flows and the iteration counter stay; converged becomes False. Takes
        effect at the next x-update. A backend without the entry: DopfError (unsupported)."""
        self._mirror.update(self._set("set_line_rating", rating))

    def set_quadratic_cost(self, c2=None):
        """dopf_set_generator_quadratic_cost: each generator's quadratic cost coefficient (G finite values >= 0, None = all 0): the
        cost of generator g at output P is gen_mc[g] P + c2[g] P^2 / 2; needs F_GEN_QUADRATIC_COST. P, D, C, the duals and the
        iteration counter stay; converged becomes False. Takes effect at the next x-update. A backend without the entry:
        DopfError (unsupported)."""
        self._mirror.update(self._set("set_quadratic_cost", c2))

    def set_availability(self, profiles=None, profile_of=None):
        """dopf_set_generator_availability: K profiles (K x T, values in [0, 1]) and each generator's profile (G indices, -1 =
        max_generation); both None resets every generator to -1. Needs F_GEN_AVAILABILITY. Takes effect at the next x-update."""
        self._mirror.update(self._set("set_availability", profiles, profile_of))

    def set_ramp(self, up=None, down=None, prev=None):
        """dopf_set_generator_ramp: each generator's ramp limits (G values >= 0 each, inf = no limit; both None = all inf) and
        optionally the outputs of the step before the window (prev, G values in [0, gen_pmax]; None = no anchor):
        -down <= P[g,t] - P[g,t-1] <= up, and at t = 0 against prev; needs F_GEN_RAMP. P, D, C, the duals and the iteration counter
        stay; converged becomes False. Takes effect at the next x-update. A backend without the entry: DopfError (unsupported)."""
        if (up is None) != (down is None):
            raise ValueError("set_ramp: up and down must both be given or both be None")
        self._mirror.update(self._set("set_ramp", None if up is None else (up, down), prev))

    def set_energy_budget(self, e_min=None, e_max=None):
        """dopf_set_generator_energy_budget: each generator's energy budget over the window, e_min <= sum_t P[g,t] <= e_max (G values
        each; e_min None = all 0, e_max None = all inf); needs F2_GEN_ENERGY_BUDGET. P, D, C, the duals and the iteration counter
        stay; converged becomes False. Takes effect at the next x-update. A backend without the entry: DopfError (unsupported)."""
        self._mirror.update(self._set("set_energy_budget", e_min, e_max))

    def set_min_output(self, p_min=None):
        """dopf_set_generator_min_output: each generator's must-run floor (G values in [0, gen_pmax]; None or all zeros = none):
        min(p_min[g], cap[g,t]) <= P[g,t] <= cap[g,t]; needs F_GEN_RAMP (the floors run on the ramp kernels; no budgets). P, D, C, the
        duals and the iteration counter stay; converged becomes False. Takes effect at the next x-update. A backend without the
        entry: DopfError (unsupported)."""
        self._mirror.update(self._set("set_min_output", p_min))

    def budget_min_output(self) -> np.ndarray:
        """dopf_get_generator_budget_min_output: the floors of set_budget_min_output as the context holds them, G values (zeros while
        none are set). A backend without the entry: DopfError."""
        if not hasattr(self.api, "get_generator_budget_min_output"):
            raise DopfError(f"{self.api.prefix}*: this API has no get_generator_budget_min_output")
        out = np.zeros(self.G)
        self._chk(self.api.get_generator_budget_min_output(self._ctx, _dp(out)))
        return out

    def min_output(self) -> np.ndarray:
        """dopf_get_generator_min_output: the floors as the context holds them, G values. A backend without the entry: DopfError."""
        if not hasattr(self.api, "get_generator_min_output"):
            raise DopfError(f"{self.api.prefix}*: this API has no get_generator_min_output")
        out = np.empty(self.G)
        self._chk(self.api.get_generator_min_output(self._ctx, _dp(out)))
        return out

    def budget_price(self) -> np.ndarray:
        """dopf_get_generator_budget_price: nu[g], the multiplier the last computed x-update put on generator g's budget row (the
        number the kernels add to gen_mc[g]; the water value of the decentral run), G values: > 0 where e_max held the row down,
        < 0 where e_min pushed it up, 0 for a free row and for one whose search gave up. Zeros before the first iteration; the
        setters leave it alone. Recording is opt-in without F2_GEN_RAMP_BUDGET: the FIRST call switches the context to the kernels
        that store the prices (graphs are captured again) and returns zeros; call it once after the constructor, then every call
        returns the last iteration's prices. At convergence -budget_dual of central_solve_coupled where that dual is unique. Needs
        F2_GEN_ENERGY_BUDGET (DopfError, unsupported, without); a backend without the entry: DopfError."""
        if not hasattr(self.api, "get_generator_budget_price"):
            raise DopfError(f"{self.api.prefix}*: this API has no get_generator_budget_price")
        out = np.zeros(self.G)
        self._chk(self.api.get_generator_budget_price(self._ctx, _dp(out)))
        return out

    def energy_budget_windows(self):
        """dopf_get_generator_energy_budget_windows: (win_end, e_min, e_max) as the context holds them — n_win ends and two (G, n_win)
        arrays — or None while no table is set. A backend without the entry: DopfError."""
        if not hasattr(self.api, "get_generator_energy_budget_windows"):
            raise DopfError(f"{self.api.prefix}*: this API has no get_generator_energy_budget_windows")
        n = C.c_int32(0)
        self._chk(self.api.get_generator_energy_budget_windows(self._ctx, C.byref(n), None, None, None))
        if n.value == 0:
            return None
        ends = np.zeros(self.T, dtype=np.int32)
        lo, hi = np.zeros(self.G * n.value), np.zeros(self.G * n.value)
        self._chk(self.api.get_generator_energy_budget_windows(self._ctx, C.byref(n), ends.ctypes.data_as(c_int32_p), _dp(lo), _dp(hi)))
        return ends[:n.value].copy(), lo.reshape(self.G, n.value), hi.reshape(self.G, n.value)

    def budget_window_price(self) -> np.ndarray:
        """dopf_get_generator_budget_window_price: nu[g, j], the multiplier the last computed x-update put on window j's budget row of
        generator g, (G, n_win), with budget_price's sign convention: 0 for a free window, one whose clamped step keeps its budget
        and one whose search gave up. Always recorded while a table is set (DopfError without one); zeros before the first iteration
        after the table's allocation. At convergence minus the host LP's dual of that row where it is unique."""
        n = C.c_int32(0)
        if hasattr(self.api, "get_generator_energy_budget_windows"):
            self._chk(self.api.get_generator_energy_budget_windows(self._ctx, C.byref(n), None, None, None))
        return self._budget_window_price(self._ctx, int(n.value))

    def ramp_price(self) -> np.ndarray:
        """dopf_get_generator_ramp_price: rp[g, t], the multiplier the last computed x-update put on generator g's ramp row between
        t-1 and t (t = 0: the anchor's row, 0 without an anchor), (G, T) in the unit of gen_mc: > 0 where ramp-up held the unit
        back, < 0 where ramp-down held it up, 0 for a row whose clamped step kept its ramps and for one whose pair search gave up.
        Recording is opt-in: the FIRST call allocates the array on the device, switches the context to the kernels that store the
        prices (graphs are captured again) and returns zeros; call it once after the constructor, then every call returns the last
        iteration's prices. Zeros before the first iteration; the setters leave it alone. At convergence -ramp_dual of
        central_solve_coupled where that dual is unique. Needs F_GEN_RAMP on a copper plate (DopfError, unsupported, without the
        flag and with lines: network rows are not priced); a backend without the entry: DopfError."""
        if not hasattr(self.api, "get_generator_ramp_price"):
            raise DopfError(f"{self.api.prefix}*: this API has no get_generator_ramp_price")
        out = np.zeros(self.G * self.T)
        self._chk(self.api.get_generator_ramp_price(self._ctx, _dp(out)))
        return out.reshape(self.G, self.T)

    # -- a receding horizon --------------------------------------------------------------------
    def demand(self) -> np.ndarray:
        """The context's demand as it stands, (N, T)."""
        return self._keep["demand"].reshape(self.T, self.N).T.copy()

    def set_demand(self, demand):
        """dopf_set_demand: the demand (N, T) replaced in place; P, D, C, the duals and the iteration counter stay, injection,
        flows and prices are derived again, converged becomes False. A backend without the entry: DopfError."""
        if not hasattr(self.api, "set_demand"):
            raise DopfError(f"{self.api.prefix}*: this API has no set_demand")
        arr = _f64(np.asarray(demand, dtype=np.float64).reshape(self.N, self.T).T, self.N * self.T)
        self._chk(self.api.set_demand(self._ctx, _dp(arr)))
        self._keep["demand"] = arr

    def roll(self, k: int, demand_tail):
        """dopf_roll_horizon: the window advances by k steps (1 <= k <= T - 1); demand_tail (N, k) is the demand of the k new
        steps. The rule is horizon.shift_window's. A backend without the entry goes the host route: getters -> shift_window -> a
        new context with the setters and set_state(iteration = 2), which replaces this engine's context; like the entry it refuses
        storages in a context without F_STO_INITIAL_LEVEL (DopfError). The availability profiles are not moved: set the new
        window's with set_availability."""
        from .horizon import shift_window
        k = int(k)
        if self._mirror.get("gen_budget_windows") is not None:       # (the library's refusal and message: a table does not roll)
            self._chk(self.api.roll_horizon_coupled(self._ctx, k, None, -1, None, None, 0, None, None))
        # (a context with ramp limits goes the host route on every API: the next window's anchor is the old P[:, k - 1])
        # (so does a context with energy budgets: what is left of them after k steps is formed below)
        native = hasattr(self.api, "roll_horizon") and not self.params.flags & F_GEN_RAMP and not self.flags2 & F2_GEN_ENERGY_BUDGET
        if not 1 <= k <= self.T - 1:
            if native:
                self._chk(self.api.roll_horizon(self._ctx, k, None))       # (the library's refusal and message)
            raise ValueError(f"roll: k = {k} outside [1, T - 1 = {self.T - 1}]")
        tail = np.asarray(demand_tail, dtype=np.float64).reshape(self.N, k)
        if native:
            # (the initial levels now live on the device only; the host route, which reads the mirror, is never taken with this API)
            self._chk(self.api.roll_horizon(self._ctx, k, _dp(_f64(tail.T, self.N * k))))
            self._keep["demand"] = _f64(np.concatenate([self.demand()[:, k:], tail], axis=1).T)
            r = self._mirror.get("line_rating")
            if r is not None:          # (the library moved its table by the same rule)
                self._mirror["line_rating"] = np.concatenate([r[:, k:], np.repeat(r[:, -1:], k, axis=1)], axis=1)
            return
        if self.S and not self.params.flags & F_STO_INITIAL_LEVEL:          # (the native entry's refusal, DOPF_E_UNSUPPORTED)
            raise DopfError(f"roll: the storages' levels after {k} steps become the next window's initial levels, which need "
                            "DOPF_F_STO_INITIAL_LEVEL at create")
        P, D, Cc, E = self.get_primal()
        lam, mu, rho = self.get_duals()
        _, aU, aK, _, _ = self.get_consensus()
        w = shift_window(k, tail, demand=self.demand(), P=P, D=D, C=Cc, E=E, lam=lam, mu=mu, rho=rho, avg_U=aU, avg_K=aK,
                         sto_emax=self._keep["sto_emax"], line_rating=self._mirror.get("line_rating"))
        kw = dict(self._keep, **self._mirror, demand=_f64(w["demand"].T))
        if self.S:
            kw["sto_e0"] = w["e0"]
        if "line_rating" in w:
            kw["line_rating"] = w["line_rating"]
        if self.params.flags & F_GEN_RAMP:
            kw["gen_prev"] = P[:, k - 1].copy()
        if self.flags2 & F2_GEN_ENERGY_BUDGET:
            # what the k steps that leave the window delivered comes off both bounds (floored at 0); the new context's setter checks
            # what is left against the caps, and its refusal is this call's
            lo, hi = self._mirror.get("gen_budget") or (None, None)
            used = P[:, :k].sum(axis=1)
            lo = np.zeros(self.G) if lo is None else np.maximum(0.0, lo - used)
            hi = np.full(self.G, np.inf) if hi is None else np.maximum(0.0, hi - used)
            kw["gen_budget"] = (lo, hi)
        new = Engine(self.api, N=self.N, L=self.L, T=self.T, params=self.params, mode=self._mode, flags2=self.flags2, **kw)
        new.set_state(P=w["P"], D=w["D"], C_=w["C"], avg_U=w["avg_U"], avg_K=w["avg_K"], lam=w["lam"], mu=w["mu"], rho=w["rho"],
                      iteration=2)
        self._adopt(new)

    def generator_coupling(self) -> dict:
        """dopf_get_generator_coupling: ramp_up, ramp_down, p_prev (NaN: no anchor), e_min, e_max as the context holds them, G values
        each (a context without the flag: inf, inf, NaN, 0, inf). A backend without the entry: DopfError."""
        if not hasattr(self.api, "get_generator_coupling"):
            raise DopfError(f"{self.api.prefix}*: this API has no get_generator_coupling")
        names = ("ramp_up", "ramp_down", "p_prev", "e_min", "e_max")
        out = {n: np.empty(self.G) for n in names}
        self._chk(self.api.get_generator_coupling(self._ctx, *(_dp(out[n]) for n in names)))
        return out

    def roll_coupled(self, k: int, demand_tail, *, availability=None, budget=None):
        """dopf_roll_horizon_coupled: roll for a context with ramp limits or energy budgets, in place — the context, its scratch
        and its graphs stay. The rule is horizon.shift_window's plus horizon.shift_coupled's: the anchor becomes P[:, k - 1], and
        what the k leaving steps delivered comes off both budgets, floored at 0. availability = (profiles, profile_of), as
        set_availability takes them ((None, None): every generator back to max_generation): the new window's table, checked together
        with the new anchor and budgets; None: the stored table stays. budget = (e_min, e_max), as set_energy_budget takes them: the
        new window's own budgets instead of what is left. A refusal (DopfError) leaves the context as it was. A backend without
        the entry: DopfError (Engine.roll's host route serves there)."""
        if not hasattr(self.api, "roll_horizon_coupled"):
            raise DopfError(f"{self.api.prefix}*: this API has no roll_horizon_coupled")
        k = int(k)
        if not 1 <= k <= self.T - 1:
            self._chk(self.api.roll_horizon_coupled(self._ctx, k, None, -1, None, None, 0, None, None))       # (the library's refusal and message)
            raise ValueError(f"roll_coupled: k = {k} outside [1, T - 1 = {self.T - 1}]")
        tail = np.asarray(demand_tail, dtype=np.float64).reshape(self.N, k)
        K, prof, of = -1, None, None
        if availability is not None:
            prof, of = _availability_norm(self, *availability)
            K = 0 if prof is None else prof.shape[0]
        lo, hi = (None, None) if budget is None else _budget_norm(self, *budget)
        self._chk(self.api.roll_horizon_coupled(
            self._ctx, k, _dp(_f64(tail.T, self.N * k)), K, _dp(None if prof is None else prof.ravel()),
            None if of is None else of.ctypes.data_as(c_int32_p), 0 if budget is None else 1, _dp(lo), _dp(hi)))
        self._keep["demand"] = _f64(np.concatenate([self.demand()[:, k:], tail], axis=1).T)
        now = self.generator_coupling()              # (the device's arithmetic, not a second evaluation of the rule)
        if self.params.flags & F_GEN_RAMP:
            self._mirror["gen_prev"] = now["p_prev"]
        if self.flags2 & F2_GEN_ENERGY_BUDGET:
            self._mirror["gen_budget"] = (now["e_min"], now["e_max"])
        if availability is not None:
            self._mirror.update(gen_avail=None if prof is None else prof.copy(), gen_avail_of=None if of is None else of.copy())
        r = self._mirror.get("line_rating")
        if r is not None:          # (the library moved its table by the same rule)
            self._mirror["line_rating"] = np.concatenate([r[:, k:], np.repeat(r[:, -1:], k, axis=1)], axis=1)

    def _adopt(self, new: "Engine"):
        """This engine goes on as `new`: its own context is destroyed, new's context and host mirrors move here, and `new` is left
        without a context (so that nothing is destroyed twice)."""
        self.close()
        self.__dict__.update(new.__dict__)
        new._ctx = C.c_void_p()

    def warm_start_stats(self):
        """(storages the warm-start kernel solved, storages it left to the scan kernel) in the LAST iteration."""
        out = (C.c_uint64 * 15)()
        self._chk(self.api.debug_stats(self._ctx, out))
        return int(out[3]), int(out[4])

    # -- consensus sum across ranks inside the library (one process per GPU) ---------------------
    def comm_unique_id(self) -> bytes:
        """128 opaque bytes (ncclUniqueId): rank 0 creates them, every rank passes them to comm_init."""
        buf = C.create_string_buffer(COMM_ID_BYTES)
        rc = self.api.comm_unique_id(buf)
        if rc != 0:
            msg = self.api.last_error(None)
            raise DopfError(f"dopf_comm_unique_id failed ({rc}): {msg.decode() if msg else ''}")
        return buf.raw

    def comm_init(self, world: int, rank: int, unique_id: bytes):
        buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        self._chk(self.api.comm_init(self._ctx, int(world), int(rank), buf))

    # -- the same sum by the peer exchange (direct stores into the peers' memory, no collective library) ----------
    def xchg_export(self, world: int) -> bytes:
        """Allocates this rank's receive area; 64 opaque bytes (hipIpcMemHandle_t) to gather over all ranks."""
        buf = C.create_string_buffer(XCHG_HANDLE_BYTES)
        self._chk(self.api.xchg_export(self._ctx, int(world), buf))
        return buf.raw

    def xchg_init(self, world: int, rank: int, handles):
        """handles: the world handles in rank order (list of bytes or one bytes object)."""
        blob = b"".join(handles) if not isinstance(handles, (bytes, bytearray)) else bytes(handles)
        if len(blob) != world * XCHG_HANDLE_BYTES:
            raise ValueError("need world x 64 bytes of handles")
        buf = C.create_string_buffer(blob, len(blob))
        self._chk(self.api.xchg_init(self._ctx, int(world), int(rank), buf))

    def comm_info(self):
        """(world, rank, collective captured in the hipGraph?)"""
        w, r, g = C.c_int32(1), C.c_int32(0), C.c_int32(0)
        self._chk(self.api.comm_info(self._ctx, C.byref(w), C.byref(r), C.byref(g)))
        return w.value, r.value, bool(g.value)

    # -- getters -------------------------------------------------------------------------------
    def _duals(self, fn):
        lam = np.zeros(self.T)
        mu = np.zeros(self.L * self.T)
        rho = np.zeros(self.L * self.T)
        self._chk(fn(self._ctx, _dp(lam), _dp(mu), _dp(rho)))
        # Julia shapes: lambda (T), mu/rho (L, T) column-major
        return lam, mu.reshape(self.T, self.L).T.copy(), rho.reshape(self.T, self.L).T.copy()

    def get_duals(self):
        return self._duals(self.api.get_duals)

    def get_duals_used(self):
        return self._duals(self.api.get_duals_used)

    def get_primal(self):
        """P (G,T), D, C, E (S,T)."""
        P = np.zeros(self.G * self.T)
        D = np.zeros(self.S * self.T)
        Cc = np.zeros(self.S * self.T)
        E = np.zeros(self.S * self.T)
        self._chk(self.api.get_primal(self._ctx, _dp(P), _dp(D), _dp(Cc), _dp(E)))
        return (P.reshape(self.G, self.T), D.reshape(self.S, self.T),
                Cc.reshape(self.S, self.T), E.reshape(self.S, self.T))

    def get_consensus(self):
        """injection (N,T), avg_U, avg_K, line_utilization (L,T), total_costs."""
        inj = np.zeros(self.N * self.T)
        aU = np.zeros(self.L * self.T)
        aK = np.zeros(self.L * self.T)
        fl = np.zeros(self.L * self.T)
        cost = C.c_double(0)
        self._chk(self.api.get_consensus(self._ctx, _dp(inj), _dp(aU), _dp(aK), _dp(fl), C.byref(cost)))
        r = lambda v, rows: v.reshape(self.T, rows).T.copy()
        return r(inj, self.N), r(aU, self.L), r(aK, self.L), r(fl, self.L), cost.value

    def get_residuals(self):
        a, b, c, it = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int32(0)
        self._chk(self.api.get_residuals(self._ctx, C.byref(a), C.byref(b), C.byref(c), C.byref(it)))
        return a.value, b.value, c.value, it.value

    def get_residual_vectors(self):
        """Convergence.{lambda_res, mue_res, rho_res}[end]: |dual change| per entry, (T), (L,T), (L,T)."""
        lam = np.zeros(self.T)
        mu = np.zeros(self.L * self.T)
        rho = np.zeros(self.L * self.T)
        self._chk(self.api.get_residual_vectors(self._ctx, _dp(lam), _dp(mu), _dp(rho)))
        return lam, mu.reshape(self.T, self.L).T.copy(), rho.reshape(self.T, self.L).T.copy()

    def get_agent_slacks(self, agent: int):
        """ResultGenerator/ResultStorage.U, .K of the last solve, (L,T) each; agent: generators first."""
        U = np.zeros(self.L * self.T)
        K = np.zeros(self.L * self.T)
        self._chk(self.api.get_agent_slacks(self._ctx, int(agent), _dp(U), _dp(K)))
        return U.reshape(self.T, self.L).T.copy(), K.reshape(self.T, self.L).T.copy()

    def get_agent_penalty(self, agent: int, delta=None):
        """PenaltyTerm(energy_balance, upper_flow, lower_flow) of the agent's last solve, (T) each. `delta`: the
        agent's injection change of that iteration; needed on a copper plate (the device keeps it only with lines)."""
        pen = np.zeros(3 * self.T)
        d = None if delta is None else _f64(delta, self.T)
        self._chk(self.api.get_agent_penalty(self._ctx, int(agent), _dp(d), _dp(pen)))
        return pen[:self.T].copy(), pen[self.T:2 * self.T].copy(), pen[2 * self.T:].copy()

    def get_penalty_sums(self):
        """Result.penalty_term (results.jl:66-70): the three penalty vectors summed over all agents, (T) each. Networks
        with F_KEEP_DELTAS (the device must hold the injection changes of the last x-update)."""
        pen = np.zeros(3 * self.T)
        self._chk(self.api.get_penalty_sums(self._ctx, _dp(pen)))
        return pen[:self.T].copy(), pen[self.T:2 * self.T].copy(), pen[2 * self.T:].copy()

    def get_nodal_price(self, which: int = 0):
        out = np.zeros(self.N * self.T)
        self._chk(self.api.get_nodal_price(self._ctx, int(which), _dp(out)))
        return out.reshape(self.T, self.N).T.copy()

    def set_state(self, *, P=None, D=None, C_=None, avg_U=None, avg_K=None, lam=None, mu=None,
                  rho=None, iteration: int = 1):
        """Matrices in Julia shape: P (G,T) etc. agent-major rows; avg_U/mu/rho (L,T)."""
        def am(a, rows):  # (rows, T) -> [t + T*row]
            return None if a is None else _f64(np.asarray(a, dtype=np.float64).reshape(rows, self.T))

        def cm(a, rows):  # (rows, T) -> column-major [r + rows*t]
            return None if a is None else _f64(np.asarray(a, dtype=np.float64).reshape(rows, self.T).T)
        bufs = [am(P, self.G), am(D, self.S), am(C_, self.S), cm(avg_U, self.L), cm(avg_K, self.L),
                None if lam is None else _f64(lam, self.T), cm(mu, self.L), cm(rho, self.L)]
        self._chk(self.api.set_state(self._ctx, *[_dp(b) for b in bufs], int(iteration)))


class _ShardView(Engine):
    """A shard's context inside a MultiEngine (owned by the dopf_multi object: never destroyed from here)."""

    def __init__(self, api: CApi, ctx, N, L, T, G, S):     # noqa: super().__init__ deliberately not called
        self.api, self._ctx = api, ctx
        self.N, self.L, self.T, self.G, self.S = N, L, T, G, S
        self._mirror = {}

    def close(self):
        self._ctx = C.c_void_p()


class MultiEngine(_ExtensionSetters):
    """One process, n GPUs: dopf_multi_* (the library shards the agents, owns the RCCL communicator and one host
    thread per device). Replicated state (duals, consensus, prices, residuals) is read from shard 0."""
    _entry_prefix = "multi_"

    def __init__(self, api: CApi, n_gpus: int, *, N, L, T, demand, ptdf, f_max, gen_mc, gen_pmax, gen_node,
                 sto_mc, sto_pmax, sto_emax, sto_node, params: Optional[DopfParams] = None, devices=None, sto_e0=None,
                 sto_end_lo=None, sto_end_hi=None, gen_avail=None, gen_avail_of=None, sto_eta=None, line_rating=None, gen_c2=None,
                 gen_ramp=None, gen_prev=None, gen_budget=None, flags2: int = 0, gen_min_output=None, gen_budget_windows=None,
                 gen_budget_min_output=None):
        self.api = api
        self.N, self.L, self.T = int(N), int(L), int(T)
        prob, keep, self.G, self.S = _problem(self.N, self.L, self.T, demand, ptdf, f_max, gen_mc, gen_pmax, gen_node,
                                              sto_mc, sto_pmax, sto_emax, sto_node)
        params, todo = _extensions(api, params, self, keep, dict(
            sto_e0=sto_e0, sto_end_lo=sto_end_lo, sto_end_hi=sto_end_hi, gen_avail=gen_avail, gen_avail_of=gen_avail_of,
            sto_eta=sto_eta, line_rating=line_rating, gen_c2=gen_c2, gen_ramp=gen_ramp, gen_prev=gen_prev, gen_budget=gen_budget,
            gen_min_output=gen_min_output))
        self.params = params if params is not None else default_params()
        # (and so do floors on budget rows)
        self.flags2 = int(flags2) | _flags2(todo, self.L) | (
            F2_GEN_ENERGY_BUDGET if gen_budget_windows is not None or gen_budget_min_output is not None else 0)
        _needs_create_ex(api, self.flags2)
        dev = None if devices is None else _i32(devices, n_gpus)
        self._m = C.c_void_p()
        args = (C.byref(self._m), C.byref(prob), C.byref(self.params), int(n_gpus), None if dev is None else dev.ctypes.data_as(c_int32_p))
        rc = api.multi_create_ex(*args, C.c_int32(self.flags2)) if self.flags2 else api.multi_create(*args)
        if rc != 0:
            msg = api.multi_last_error(None)
            raise DopfError(f"dopf_multi_create failed ({rc}): {msg.decode() if msg else ''}")
        self.n = int(api.multi_size(self._m))
        self._mirror = {}           # (of the extensions' inputs, the efficiencies and the budget windows alone)
        self._apply(todo)
        if gen_budget_windows is not None:
            self.set_energy_budget_windows(*gen_budget_windows)
        if gen_budget_min_output is not None:
            self.set_budget_min_output(gen_budget_min_output)

    def _handle(self):
        return self._m

    def set_quadratic_cost(self, c2=None):
        """dopf_multi_set_generator_quadratic_cost: all G generators' quadratic cost coefficients in the caller's order (None = all
        0); each shard gets its slice."""
        self._set("set_quadratic_cost", c2)

    def set_ramp(self, up=None, down=None, prev=None):
        """dopf_multi_set_generator_ramp: all G generators' ramp limits and (optionally) anchors in the caller's order (both ramps
        None = all inf, prev None = no anchor); each shard gets its slice."""
        if (up is None) != (down is None):
            raise ValueError("set_ramp: up and down must both be given or both be None")
        self._set("set_ramp", None if up is None else (up, down), prev)

    def set_energy_budget(self, e_min=None, e_max=None):
        """dopf_multi_set_generator_energy_budget: all G generators' energy budgets in the caller's order (e_min None = all 0, e_max
        None = all inf); each shard gets its slice."""
        self._set("set_energy_budget", e_min, e_max)

    def set_min_output(self, p_min=None):
        """dopf_multi_set_generator_min_output: all G generators' must-run floors in the caller's order (None or all zeros = none);
        every shard is checked before any stores."""
        self._set("set_min_output", p_min)

    def set_line_rating(self, rating=None):
        """dopf_multi_set_line_rating: the (L, T) table for every shard (None = f_max in every timestep)."""
        self._set("set_line_rating", rating)

    def set_availability(self, profiles=None, profile_of=None):
        """dopf_multi_set_generator_availability: K profiles (K x T) and all G generators' indices in the caller's order (every
        shard gets the whole table and its slice); both None resets every generator to -1."""
        self._set("set_availability", profiles, profile_of)

    def set_efficiency(self, eta_c=None, eta_d=None):
        """dopf_multi_set_storage_efficiency: all storages' efficiencies in the caller's order (both None = all 1)."""
        self._mirror.update(self._set("set_efficiency", eta_c, eta_d))

    def set_initial_levels(self, e0=None):
        """dopf_multi_set_storage_initial_level: all storages' initial levels in the caller's order (None = all 0)."""
        self._set("set_initial_levels", e0)

    def set_terminal_levels(self, lo=None, hi=None):
        """dopf_multi_set_storage_terminal_level: all storages' terminal bands in the caller's order (both None = [0, max_level])."""
        self._set("set_terminal_levels", lo, hi)

    def _chk(self, rc):
        if rc != 0:
            msg = self.api.multi_last_error(self._m)
            raise DopfError(f"dopf_multi_* failed ({rc}): {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_m", None) is not None and self._m.value:
            self.api.multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def iterate(self, n_iters: int):
        done, conv = C.c_int32(0), C.c_int32(0)
        self._chk(self.api.multi_iterate(self._m, int(n_iters), C.byref(done), C.byref(conv)))
        return done.value, bool(conv.value)

    def get_primal(self):
        P = np.zeros(self.G * self.T)
        D = np.zeros(self.S * self.T)
        Cc = np.zeros(self.S * self.T)
        E = np.zeros(self.S * self.T)
        self._chk(self.api.multi_get_primal(self._m, _dp(P), _dp(D), _dp(Cc), _dp(E)))
        return (P.reshape(self.G, self.T), D.reshape(self.S, self.T), Cc.reshape(self.S, self.T), E.reshape(self.S, self.T))

    def budget_price(self) -> np.ndarray:
        """dopf_multi_get_generator_budget_price: Engine.budget_price for all shards' rows in the caller's order, G values."""
        if not hasattr(self.api, "multi_get_generator_budget_price"):
            raise DopfError(f"{self.api.prefix}*: this API has no multi_get_generator_budget_price")
        out = np.zeros(self.G)
        self._chk(self.api.multi_get_generator_budget_price(self._m, _dp(out)))
        return out

    def energy_budget_windows(self):
        """(win_end, e_min, e_max) as set_energy_budget_windows stored them ((G, n_win) arrays in the caller's order; None for a
        table given as None), or None while no table is set: the host mirror."""
        return self._mirror.get("gen_budget_windows")

    def budget_window_price(self) -> np.ndarray:
        """dopf_multi_get_generator_budget_window_price: Engine.budget_window_price for all shards' rows in the caller's order,
        (G, n_win)."""
        w = self._mirror.get("gen_budget_windows")
        return self._budget_window_price(self._m, 0 if w is None else int(w[0].size))

    def ramp_price(self) -> np.ndarray:
        """dopf_multi_get_generator_ramp_price: Engine.ramp_price for all shards' rows in the caller's order, (G, T)."""
        if not hasattr(self.api, "multi_get_generator_ramp_price"):
            raise DopfError(f"{self.api.prefix}*: this API has no multi_get_generator_ramp_price")
        out = np.zeros(self.G * self.T)
        self._chk(self.api.multi_get_generator_ramp_price(self._m, _dp(out)))
        return out.reshape(self.G, self.T)

    def shard(self, i: int = 0) -> Engine:
        """Engine view of shard i's context (getters for the replicated state; do not iterate it directly)."""
        ctx = C.c_void_p(self.api.multi_ctx(self._m, int(i)))
        if not ctx.value:
            raise IndexError(i)
        def cut(total):              # the split dopf_multi_create makes (contiguous, remainder to the first shards)
            base, rem = divmod(total, self.n)
            return base + (1 if i < rem else 0)
        return _ShardView(self.api, ctx, self.N, self.L, self.T, cut(self.G), cut(self.S))


def _no_budget_floors(gen_budget_min_output) -> None:
    """The device LP's front ends refuse floors on budget rows as they refuse gen_min_output."""
    if gen_budget_min_output is not None and np.any(np.asarray(gen_budget_min_output, dtype=np.float64) != 0.0):
        raise DopfError("dopf_central_solve*: the device LP takes no generator minimum output (its generators' lower bound is 0); use "
                        "central.solve_central_packed(..., gen_budget=, gen_min_output=) for a budget case with a floor")


def _no_budget_windows(gen_budget_windows) -> None:
    """The device LP's front ends refuse a case with budgets per sub-window, as they refuse floors."""
    if gen_budget_windows is not None:
        raise DopfError("dopf_central_solve*: the device LP takes no energy budgets per sub-window (its budget rows span the whole "
                        "horizon); use central.solve_central_packed(..., gen_budget_windows=) for a case with a table")


def central_solve(api: CApi, *, N, L, T, demand, ptdf, f_max, gen_mc, gen_pmax, gen_node, sto_mc, sto_pmax, sto_emax,
                  sto_node, tol: float = 1e-8, max_iters: int = 200000, params: Optional[DopfParams] = None,
                  sto_e0=None, sto_end_lo=None, sto_end_hi=None, gen_avail=None, gen_avail_of=None, sto_eta=None,
                  line_rating=None, gen_c2=None, gen_ramp=None, gen_prev=None, gen_budget=None, gen_min_output=None,
                  gen_budget_windows=None, gen_budget_min_output=None) -> dict:
    """dopf_central_solve: the central reference (src/opf_central_reference.jl) as one LP solved on the GPU by a first-order
    primal-dual method. Arguments as Engine (PackedProblem.engine_kwargs()). Returns objective, gap, iterations and the
    reference script's outputs in Julia shapes: P (G,T), D/C/E (S,T), system_price (T), nodal_price (N,T),
    line_utilization (L,T).
    sto_e0 (S), sto_end_lo / sto_end_hi (S each, both or neither), gen_avail (K x T) / gen_avail_of (G indices in [-1, K)): the
    inputs of the three problem extensions, as Engine takes them; with any of them given the call is dopf_central_solve_ex, which
    checks them as the setters do (DopfError with the setter's message), and E holds levels that include sto_e0.
    sto_eta = (eta_c, eta_d) (S each, in (0, 1]): the storages' charge and discharge efficiencies, as Engine takes them; whenever it is
    given (all ones too) the call is dopf_central_solve_lossy, and E = sto_e0 + cumsum(eta_c C - D / eta_d).
    line_rating: the device LP takes no line ratings; a table other than f_max in every timestep raises DopfError.
    gen_c2: the device LP takes no quadratic costs either; a non-zero coefficient raises DopfError.
    gen_ramp, gen_prev: nor ramp limits; a finite ramp or an anchor raises DopfError.
    gen_budget: nor energy budgets; an e_min above 0 or a finite e_max raises DopfError.
    gen_min_output: nor must-run floors; a value above 0 raises DopfError.
    gen_budget_windows: nor budgets per sub-window; a table raises DopfError.
    gen_budget_min_output: nor floors on budget rows; a value above 0 raises DopfError.
    T: any horizon. Beyond 512 timesteps the storages run on the long sweep (kc_sto_long); the entry sets DOPF_F_LONG_HORIZON on its own
    context, so params needs no flag, and with F_LONG_HORIZON in params the result is the same bits. F_DEBUG_LONG_STO in params runs
    that sweep at T <= 512 too (tests)."""
    N, L, T = int(N), int(L), int(T)
    _no_budget_windows(gen_budget_windows)
    _no_budget_floors(gen_budget_min_output)
    if gen_min_output is not None and np.any(np.asarray(gen_min_output, dtype=np.float64) != 0.0):
        raise DopfError("dopf_central_solve*: the device LP takes no generator minimum output (its generators' lower bound is 0); use "
                        "central.solve_central_packed(..., gen_min_output=) for a case with a floor")
    if gen_budget is not None and ((gen_budget[0] is not None and np.any(np.asarray(gen_budget[0], dtype=np.float64) != 0.0)) or
                                   (gen_budget[1] is not None and np.any(np.asarray(gen_budget[1], dtype=np.float64) != np.inf))):
        raise DopfError("dopf_central_solve*: the device LP takes no generator energy budgets (it bounds no generator's sum over the "
                        "window); use central_solve_coupled, or central.solve_central_packed(..., gen_budget=), for a case with a budget")
    if gen_prev is not None or (gen_ramp is not None and any(np.any(np.isfinite(np.asarray(r, dtype=np.float64))) for r in gen_ramp)):
        raise DopfError("dopf_central_solve*: the device LP takes no generator ramp limits (it lets every generator move freely); use "
                        "central_solve_coupled, or central.solve_central_packed(..., gen_ramp=), for a case with ramps")
    if gen_c2 is not None and np.any(np.asarray(gen_c2, dtype=np.float64) != 0.0):
        raise DopfError("dopf_central_solve*: the device LP takes no quadratic generator costs (it solves with gen_mc alone)")
    if line_rating is not None and np.any(np.asarray(line_rating, dtype=np.float64).reshape(L, T) != _f64(f_max, L)[:, None]):
        raise DopfError("dopf_central_solve*: the device LP takes no line ratings (it solves with f_max in every timestep); use "
                        "central_solve_coupled, or central.solve_central_packed(..., line_rating=), for a case with ratings")
    prob, keep, G, S = _problem(N, L, T, demand, ptdf, f_max, gen_mc, gen_pmax, gen_node, sto_mc, sto_pmax, sto_emax, sto_node)
    q = params if params is not None else default_params()
    res = DopfCentralResult()
    P, D, Cc, E = np.zeros(G * T), np.zeros(S * T), np.zeros(S * T), np.zeros(S * T)
    lam, nodal, flow = np.zeros(T), np.zeros(N * T), np.zeros(L * T)
    fu, fl = np.zeros(L * T), np.zeros(L * T)
    outs = (_dp(P), _dp(D), _dp(Cc), _dp(E), _dp(lam), _dp(nodal), _dp(flow), _dp(fu), _dp(fl))
    if all(a is None for a in (sto_e0, sto_end_lo, sto_end_hi, gen_avail, gen_avail_of, sto_eta)):
        entry = "dopf_central_solve"
        rc = api.central_solve(C.byref(prob), C.byref(q), float(tol), int(max_iters), C.byref(res), *outs)
    else:
        e0 = None if sto_e0 is None else _f64(sto_e0, S)
        lo = None if sto_end_lo is None else _f64(sto_end_lo, S)
        hi = None if sto_end_hi is None else _f64(sto_end_hi, S)
        K, prof, of = _availability_arrays(gen_avail, gen_avail_of, T, G)
        tail = (K, _dp(prof), None if of is None else of.ctypes.data_as(c_int32_p), float(tol), int(max_iters), C.byref(res)) + outs
        if sto_eta is None:
            entry = "dopf_central_solve_ex"
            rc = api.central_solve_ex(C.byref(prob), C.byref(q), _dp(e0), _dp(lo), _dp(hi), *tail)
        else:
            entry = "dopf_central_solve_lossy"
            ec, ed = _f64(sto_eta[0], S), _f64(sto_eta[1], S)
            rc = api.central_solve_lossy(C.byref(prob), C.byref(q), _dp(e0), _dp(lo), _dp(hi), _dp(ec), _dp(ed), *tail)
    if rc != 0:
        msg = api.last_error(None)
        raise DopfError(f"{entry} failed ({rc}): {msg.decode() if msg else ''}")
    return dict(objective=res.objective, dual_objective=res.dual_objective, primal_infeasibility=res.primal_infeasibility,
                gap=res.gap, iterations=res.iterations, converged=bool(res.converged),
                P=P.reshape(G, T), D=D.reshape(S, T), C=Cc.reshape(S, T), E=E.reshape(S, T), system_price=lam,
                nodal_price=nodal.reshape(T, N).T.copy(), line_utilization=flow.reshape(T, L).T.copy(),
                flow_upper_dual=fu.reshape(T, L).T.copy(), flow_lower_dual=fl.reshape(T, L).T.copy())


def central_solve_coupled(api: CApi, *, N, L, T, demand, ptdf, f_max, gen_mc, gen_pmax, gen_node, sto_mc, sto_pmax, sto_emax,
                          sto_node, tol: float = 1e-8, max_iters: int = 200000, params: Optional[DopfParams] = None,
                          sto_e0=None, sto_end_lo=None, sto_end_hi=None, gen_avail=None, gen_avail_of=None, sto_eta=None,
                          line_rating=None, gen_c2=None, gen_ramp=None, gen_prev=None, gen_budget=None, gen_min_output=None,
                          gen_budget_windows=None, gen_budget_min_output=None) -> dict:
    """dopf_central_solve_coupled: central_solve's LP with the constraints that couple a generator's timesteps and with per-timestep
    line limits. Arguments as Engine (PackedProblem.engine_kwargs()); beyond central_solve's:
    line_rating (L, T): the limits of the flow rows, as Engine takes them (None: f_max in every timestep).
    gen_ramp = (ramp_up, ramp_down) (G each, inf = no limit), gen_prev (G outputs of the step before the window; None: no anchor).
    gen_budget = (e_min, e_max) (G each; either may be None: 0, inf).
    The call is always dopf_central_solve_coupled (with none of the four given it returns dopf_central_solve_lossy's bits); it checks
    the inputs as the three setters do (DopfError with the entry's name). gen_c2: the device solve is an LP; a non-zero coefficient
    raises DopfError, and so does a gen_min_output above 0 (the device LP's generators go down to 0) and a gen_budget_windows table. Returns central_solve's dict plus ramp_dual (G, T) and budget_dual (G,): d objective / d right-hand side of the
    ramp row between t - 1 and t (t = 0: the anchor's row) and of the budget row — negative where the row's upper end binds, positive
    where its lower end does.
    T: any horizon, with ramps and budgets too. Beyond 512 timesteps the rows run on the long sweeps (kc_gen_rows_long, kc_sto_long);
    params needs no flag for it. F_DEBUG_LONG_STO in params runs those sweeps at T <= 512 too (tests)."""
    N, L, T = int(N), int(L), int(T)
    _no_budget_windows(gen_budget_windows)
    _no_budget_floors(gen_budget_min_output)
    if gen_c2 is not None and np.any(np.asarray(gen_c2, dtype=np.float64) != 0.0):
        raise DopfError("dopf_central_solve_coupled: the device LP takes no quadratic generator costs (it solves with gen_mc alone)")
    if gen_min_output is not None and np.any(np.asarray(gen_min_output, dtype=np.float64) != 0.0):
        raise DopfError("dopf_central_solve_coupled: the device LP takes no generator minimum output (its generators' lower bound is "
                        "0); use central.solve_central_packed(..., gen_min_output=) for a case with a floor")
    prob, keep, G, S = _problem(N, L, T, demand, ptdf, f_max, gen_mc, gen_pmax, gen_node, sto_mc, sto_pmax, sto_emax, sto_node)
    q = params if params is not None else default_params()
    res = DopfCentralResult()
    P, D, Cc, E = np.zeros(G * T), np.zeros(S * T), np.zeros(S * T), np.zeros(S * T)
    lam, nodal, flow = np.zeros(T), np.zeros(N * T), np.zeros(L * T)
    fu, fl = np.zeros(L * T), np.zeros(L * T)
    rdual, bdual = np.zeros(G * T), np.zeros(G)
    opt = lambda a, n: None if a is None else _f64(a, n)
    e0, lo, hi = opt(sto_e0, S), opt(sto_end_lo, S), opt(sto_end_hi, S)
    ec, ed = (None, None) if sto_eta is None else (_f64(sto_eta[0], S), _f64(sto_eta[1], S))
    K, prof, of = _availability_arrays(gen_avail, gen_avail_of, T, G)
    rating = None if line_rating is None else _f64(np.asarray(line_rating, dtype=np.float64).reshape(L, T).T, L * T)      # [l + L*t]
    up, down = (None, None) if gen_ramp is None else (opt(gen_ramp[0], G), opt(gen_ramp[1], G))
    prev = opt(gen_prev, G)
    emin, emax = (None, None) if gen_budget is None else (opt(gen_budget[0], G), opt(gen_budget[1], G))
    rc = api.central_solve_coupled(C.byref(prob), C.byref(q), _dp(e0), _dp(lo), _dp(hi), _dp(ec), _dp(ed), K, _dp(prof),
                                   None if of is None else of.ctypes.data_as(c_int32_p), _dp(rating), _dp(up), _dp(down), _dp(prev),
                                   _dp(emin), _dp(emax), float(tol), int(max_iters), C.byref(res), _dp(P), _dp(D), _dp(Cc), _dp(E),
                                   _dp(lam), _dp(nodal), _dp(flow), _dp(fu), _dp(fl), _dp(rdual), _dp(bdual))
    if rc != 0:
        msg = api.last_error(None)
        raise DopfError(f"dopf_central_solve_coupled failed ({rc}): {msg.decode() if msg else ''}")
    return dict(objective=res.objective, dual_objective=res.dual_objective, primal_infeasibility=res.primal_infeasibility,
                gap=res.gap, iterations=res.iterations, converged=bool(res.converged),
                P=P.reshape(G, T), D=D.reshape(S, T), C=Cc.reshape(S, T), E=E.reshape(S, T), system_price=lam,
                nodal_price=nodal.reshape(T, N).T.copy(), line_utilization=flow.reshape(T, L).T.copy(),
                flow_upper_dual=fu.reshape(T, L).T.copy(), flow_lower_dual=fl.reshape(T, L).T.copy(),
                ramp_dual=rdual.reshape(G, T), budget_dual=bdual)
