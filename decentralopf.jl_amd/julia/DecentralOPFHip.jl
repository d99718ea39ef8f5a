# DecentralOPFHip.jl — Julia host for libdopf_hip (the MI355X-native ADMM consensus-OPF inner loop).
#
# Takes the place of `include("imports.jl")` in src/opf_admm_decentral.jl of rockstaedt/DecentralOPF.jl:
#
#     include("/path/to/DecentralOPFHip.jl")        # instead of include("imports.jl")  (no JuMP, no Gurobi, no licence)
#     include("cases/three_node.jl")
#     admm = ADMM(0.3, nodes, generators, storages, lines)
#     run!(admm)
#     np = get_nodal_price(admm.iteration)
#
# Like the reference's own imports.jl this is a plain script evaluated in `Main` — NOT a module: the element
# types Node / Generator / Storage / Line are the reference's own (its src/structures/network_elements.jl is
# included verbatim, so cases/*.jl construct exactly the types ADMM(...) accepts), calculate_ptdf is the
# reference's own (src/helpers/ptdf.jl), and ADMM / run! / calculate_iteration! / get_nodal_price keep the
# reference's names, argument lists and stopping behaviour:
#     ADMM(gamma, nodes, generators, storages, lines)      src/structures/admm.jl:23-62
#     run!(admm) / calculate_iteration!(admm)              src/optimization/run.jl:1-16
#     get_nodal_price(iteration)  (reads the global `admm`, like the reference)   src/helpers/network_elements.jl:16-25
# Everything between is a ccall into the C ABI of include/dopf.h.
#
# STATUS: written by inspection — the build image has no Julia, so this file has NOT been executed. What is
# checked mechanically (tests/test_julia_shim.py): the C struct mirrors against include/dopf.h field by field,
# every ccall's symbol and arity against the header, and the structural points above. The identical call
# sequence runs from Python ctypes and from C (examples/three_node.c) in the GPU test-suite.
#
# Where the reference's files are found: next to this file if it has been copied into the reference's src/
# directory, else ENV["DECENTRALOPF_SRC"], else ./src. The library: ENV["DOPF_LIB"] or "libdopf_hip" on the
# loader path.

using LinearAlgebra                     # calculate_ptdf uses Diagonal and inv (the reference gets it from imports.jl:3)

const DOPF_SRC = isfile(joinpath(@__DIR__, "structures", "network_elements.jl")) ? @__DIR__ :
                 get(ENV, "DECENTRALOPF_SRC", joinpath(pwd(), "src"))
include(joinpath(DOPF_SRC, "structures", "network_elements.jl"))   # Node, Generator, Storage, Line — verbatim, in Main
include(joinpath(DOPF_SRC, "helpers", "ptdf.jl"))                  # calculate_ptdf(nodes, lines)

const DOPF_LIB = get(ENV, "DOPF_LIB", "libdopf_hip")

# mirrors of struct dopf_problem / struct dopf_params (include/dopf.h): same field order, same types
struct CProblem
    N::Cint
    L::Cint
    T::Cint
    G::Cint
    S::Cint
    demand::Ptr{Cdouble}
    ptdf::Ptr{Cdouble}
    f_max::Ptr{Cdouble}
    gen_mc::Ptr{Cdouble}
    gen_pmax::Ptr{Cdouble}
    gen_node::Ptr{Cint}
    sto_mc::Ptr{Cdouble}
    sto_pmax::Ptr{Cdouble}
    sto_emax::Ptr{Cdouble}
    sto_node::Ptr{Cint}
end

struct CParams
    gamma::Cdouble
    w_flow::Cdouble
    w_prox::Cdouble
    eps::Cdouble
    mask_thr::Cdouble
    max_iters::Cint
    n_agents_global::Cint
    device::Cint
    flags::Cint
    stream::Ptr{Cvoid}
end

# Convergence of the reference (src/structures/convergence.jl): the flags and the residual history
mutable struct Convergence
    lambda::Bool
    lambda_res::Vector{Vector{Float64}}
    mue::Bool
    mue_res::Vector{Matrix{Float64}}
    rho::Bool
    rho_res::Vector{Matrix{Float64}}
    all::Bool
    Convergence() = new(false, [], false, [], false, [], false)
end

# Same field names as the reference's ADMM for everything a caller reads; `results` holds NamedTuples with the
# fields of Result (generation per unit, discharge/charge/level, injection, avg_U, avg_K, total_costs,
# line_utilization). Histories grow only with record = true (the reference always records: O(iterations x agents)
# of host memory and one device read-back per iteration); without it the last TWO dual sets are kept, which is
# what get_nodal_price(admm.iteration) needs.
mutable struct ADMM
    iteration::Int
    gamma::Float64
    lambdas::Vector{Vector{Float64}}
    mues::Vector{Matrix{Float64}}
    rhos::Vector{Matrix{Float64}}
    T::Vector{Int}
    N::Vector{Int}
    L::Vector{Int}
    nodes::Vector{Node}
    generators::Vector{Generator}
    storages::Vector{Storage}
    lines::Vector{Line}
    results::Vector{Any}
    convergence::Convergence
    ptdf::Matrix{Float64}
    total_demand::Vector{Float64}
    node_to_id::Dict{Node, Int}
    f_max::Vector{Float64}
    record::Bool
    n_gpus::Int
    ctx::Ptr{Cvoid}                 # dopf_ctx* (n_gpus == 1) ...
    multi::Ptr{Cvoid}               # ... or dopf_multi* (n_gpus > 1: the library shards the agents and owns RCCL)
end

function dopf_check(rc::Cint, ctx::Ptr{Cvoid})
    rc == 0 && return
    msg = unsafe_string(ccall((:dopf_last_error, DOPF_LIB), Cstring, (Ptr{Cvoid},), ctx))
    error("libdopf_hip error $rc: $msg")
end

function dopf_check_multi(rc::Cint, m::Ptr{Cvoid})
    rc == 0 && return
    msg = unsafe_string(ccall((:dopf_multi_last_error, DOPF_LIB), Cstring, (Ptr{Cvoid},), m))
    error("libdopf_hip error $rc: $msg")
end

const DOPF_F_COMM_P2P = 1024      # include/dopf.h
const DOPF_F_LONG_HORIZON = 2097152  # include/dopf.h
const DOPF_F_WIDE_NETWORK = 8388608  # include/dopf.h
const DOPF_F_DEBUG_WIDE_NET = 16777216  # include/dopf.h (tests)
const DOPF_F_STO_INITIAL_LEVEL = 33554432  # include/dopf.h
const DOPF_F_STO_TERMINAL_LEVEL = 67108864  # include/dopf.h
const DOPF_F_GEN_AVAILABILITY = 134217728  # include/dopf.h
const DOPF_F_STO_EFFICIENCY = 268435456  # include/dopf.h
const DOPF_F_LINE_RATING = 536870912  # include/dopf.h
const DOPF_F_GEN_QUADRATIC_COST = 1073741824  # include/dopf.h
const DOPF_F_GEN_RAMP = 32  # include/dopf.h
const DOPF_F_GEN_RAMP_NETWORK = typemin(Int32)  # include/dopf.h: 2147483648, bit 31 — the sign bit of the Cint flag word, and its last
const DOPF_F2_GEN_ENERGY_BUDGET = 1  # include/dopf.h: the second flag word (the `flags2` keyword; dopf_create_ex)
const DOPF_F2_GEN_RAMP_BUDGET = 8  # include/dopf.h: ramp limits and energy budgets on the same generators (copper plates)
const DOPF_TRACE_DUALS = 1      # include/dopf.h: dopf_trace_begin's `what` — lambda, mu, rho
const DOPF_TRACE_CONSENSUS = 2  # injection, avg_U, avg_K, line_util
const DOPF_TRACE_PRIMAL = 4     # P, D, C (E is derived when read)

"""
    ADMM(gamma, nodes, generators, storages, lines; max_iters=0, n_gpus=1, record=false, ...)

The reference's constructor (src/structures/admm.jl:23-27) with the same five positional arguments. The `Int`
struct fields are promoted to Float64 when packed; matrices go over column-major, as Julia stores them.
Keywords are additions: `max_iters` (the reference loops forever on a divergent case), `n_gpus` (> 1: agents are
sharded over that many devices inside the library, one RCCL all-reduce per iteration — or, with
`flags = DOPF_F_COMM_P2P`, the library's peer exchange: direct stores into the other devices' memory, no collective
library, a few microseconds instead of tens for the small vector of a copper plate), `record`, and the
reference's literals `w_flow = 10`, `w_prox = 1`, `eps = 1e-3`, `mask_thr = 1e-2`.
Storages on horizons beyond 512 timesteps (an hourly year: T = 8 760) need `flags = DOPF_F_LONG_HORIZON`
(the long-horizon storage body; without the flag the library refuses them). The central references on the device
(`central_reference`, `central_reference_coupled`) take such horizons without any flag. Networks of more than 2 048 lines
need `flags = DOPF_F_WIDE_NETWORK` (the wide-network chain; without it the library refuses them). Storages that start a
horizon from a given level (see `set_initial_levels!`) need `flags = DOPF_F_STO_INITIAL_LEVEL`; storages whose level after the
last timestep is bounded (see `set_terminal_levels!`) need `flags = DOPF_F_STO_TERMINAL_LEVEL`; generators that follow an
availability profile (see `set_availability!`) need `flags = DOPF_F_GEN_AVAILABILITY`; storages with charge / discharge
efficiencies below 1 (see `set_efficiency!`; the reference's `Storage` type, used verbatim, has no such fields) need
`flags = DOPF_F_STO_EFFICIENCY`, line limits per timestep (see `set_line_rating!`) `flags = DOPF_F_LINE_RATING`, and quadratic
generator cost curves (see `set_quadratic_cost!`) `flags = DOPF_F_GEN_QUADRATIC_COST`; generator ramp limits (see `set_ramp!`) `flags = DOPF_F_GEN_RAMP` — on a case
with lines the constructor adds `DOPF_F_GEN_RAMP_NETWORK`, the library's opt-in for the network step's knot scratch. Flags combine with `|`.
`flags2` is the second flag word (`dopf_params.flags` is full): generator energy budgets over the window (see `set_energy_budget!`)
need `flags2 = DOPF_F2_GEN_ENERGY_BUDGET`; a non-zero `flags2` creates the context through `dopf_create_ex` / `dopf_multi_create_ex`.
With `flags = DOPF_F_GEN_RAMP` and `flags2 = DOPF_F2_GEN_ENERGY_BUDGET` together on a case without lines the constructor adds
`DOPF_F2_GEN_RAMP_BUDGET`, the library's opt-in for the scratch of the step that keeps both (DESIGN.md 5x); with lines it adds nothing
and the library's refusal of the two together comes back as it is.
"""
function ADMM(gamma::Float64, nodes::Vector{Node}, generators::Vector{Generator}, storages::Vector{Storage},
              lines::Vector{Line}; max_iters::Int=0, device::Int=-1, n_gpus::Int=1, record::Bool=false,
              w_flow::Float64=10.0, w_prox::Float64=1.0, eps::Float64=1e-3, mask_thr::Float64=1e-2, flags::Int=0, flags2::Int=0)
    N, L, T = length(nodes), length(lines), length(nodes[1].demand)
    G, S = length(generators), length(storages)
    if (flags & DOPF_F_GEN_RAMP) != 0 && L > 0
        flags |= DOPF_F_GEN_RAMP_NETWORK         # ramps on a network: k_gen_ramp_net and its knot scratch (DESIGN.md 5s)
    end
    if (flags & DOPF_F_GEN_RAMP) != 0 && (flags2 & DOPF_F2_GEN_ENERGY_BUDGET) != 0 && L == 0
        flags2 |= DOPF_F2_GEN_RAMP_BUDGET        # ramps and budgets on a copper plate: k_gen_ramp_budget and its scratch (DESIGN.md 5x)
    end
    node_to_id = Dict{Node, Int}(n => i for (i, n) in enumerate(nodes))
    demand = Float64[nodes[n].demand[t] for n in 1:N, t in 1:T]          # N x T, column-major = [n + N*t]
    ptdf = L > 0 ? Matrix{Float64}(calculate_ptdf(nodes, lines)) : zeros(Float64, 0, N)
    f_max = Float64[l.max_capacity for l in lines]
    gen_mc = Float64[g.marginal_costs for g in generators]
    gen_pmax = Float64[g.max_generation for g in generators]
    gen_node = Cint[node_to_id[g.node] - 1 for g in generators]          # 0-based
    sto_mc = Float64[s.marginal_costs for s in storages]
    sto_pmax = Float64[s.max_power for s in storages]
    sto_emax = Float64[s.max_level for s in storages]
    sto_node = Cint[node_to_id[s.node] - 1 for s in storages]
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    multi = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve demand ptdf f_max gen_mc gen_pmax gen_node sto_mc sto_pmax sto_emax sto_node begin
        prob = Ref(CProblem(N, L, T, G, S, pointer(demand), pointer(ptdf), pointer(f_max), pointer(gen_mc),
                            pointer(gen_pmax), pointer(gen_node), pointer(sto_mc), pointer(sto_pmax),
                            pointer(sto_emax), pointer(sto_node)))
        par = Ref(CParams(gamma, w_flow, w_prox, eps, mask_thr, max_iters, 0, device, flags, C_NULL))
        if n_gpus == 1
            rc = flags2 == 0 ?
                ccall((:dopf_create, DOPF_LIB), Cint, (Ref{Ptr{Cvoid}}, Ref{CProblem}, Ref{CParams}), ctx, prob, par) :
                ccall((:dopf_create_ex, DOPF_LIB), Cint, (Ref{Ptr{Cvoid}}, Ref{CProblem}, Ref{CParams}, Cint), ctx, prob, par, flags2)
            dopf_check(rc, Ptr{Cvoid}(C_NULL))       # the library copies every input before returning
        else
            rc = flags2 == 0 ?
                ccall((:dopf_multi_create, DOPF_LIB), Cint, (Ref{Ptr{Cvoid}}, Ref{CProblem}, Ref{CParams}, Cint, Ptr{Cint}),
                      multi, prob, par, n_gpus, C_NULL) :
                ccall((:dopf_multi_create_ex, DOPF_LIB), Cint, (Ref{Ptr{Cvoid}}, Ref{CProblem}, Ref{CParams}, Cint, Ptr{Cint}, Cint),
                      multi, prob, par, n_gpus, C_NULL, flags2)
            dopf_check_multi(rc, Ptr{Cvoid}(C_NULL))
            ctx[] = ccall((:dopf_multi_ctx, DOPF_LIB), Ptr{Cvoid}, (Ptr{Cvoid}, Cint), multi[], 0)   # replicated state: shard 0
        end
    end
    total_demand = zeros(T)
    for node in nodes
        total_demand += node.demand
    end
    admm = ADMM(1, gamma, [zeros(T)], [zeros(L, T)], [zeros(L, T)], collect(1:T), collect(1:N), collect(1:L),
                nodes, generators, storages, lines, [], Convergence(), ptdf, total_demand, node_to_id, f_max,
                record, n_gpus, ctx[], multi[])
    finalizer(admm) do a
        if a.multi != C_NULL
            ccall((:dopf_multi_destroy, DOPF_LIB), Cvoid, (Ptr{Cvoid},), a.multi)
        elseif a.ctx != C_NULL
            ccall((:dopf_destroy, DOPF_LIB), Cvoid, (Ptr{Cvoid},), a.ctx)
        end
    end
    return admm
end

function dopf_duals(admm::ADMM; used::Bool=false)
    lam = zeros(length(admm.T))
    mu = zeros(length(admm.L), length(admm.T))
    rho = zeros(length(admm.L), length(admm.T))
    if used
        dopf_check(ccall((:dopf_get_duals_used, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                         admm.ctx, lam, mu, rho), admm.ctx)
    else
        dopf_check(ccall((:dopf_get_duals, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                         admm.ctx, lam, mu, rho), admm.ctx)
    end
    return lam, mu, rho
end

"""P is T x G, D / C / E are T x S: column u = ResultGenerator.generation resp. ResultStorage.discharge/charge/level of unit u."""
function dopf_primal(admm::ADMM)
    T, G, S = length(admm.T), length(admm.generators), length(admm.storages)
    P = zeros(T, G); D = zeros(T, S); C = zeros(T, S); E = zeros(T, S)
    if admm.multi != C_NULL
        dopf_check_multi(ccall((:dopf_multi_get_primal, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                               admm.multi, P, D, C, E), admm.multi)
    else
        dopf_check(ccall((:dopf_get_primal, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                         admm.ctx, P, D, C, E), admm.ctx)
    end
    return P, D, C, E
end

"""
    set_initial_levels!(admm, e0)

The level of each storage before the first timestep (`e0[s]`, in the order of `storages`, `0 <= e0[s] <= max_level`;
`nothing` = all 0), for a horizon that continues where the last one ended. The reference starts every storage empty
(src/optimization/subproblems.jl:154); the ADMM must have been created with `flags = DOPF_F_STO_INITIAL_LEVEL`. Takes
effect at the next iteration.
"""
function set_initial_levels!(admm::ADMM, e0::Union{Nothing, Vector{Float64}})
    S = length(admm.storages)
    e0 === nothing || length(e0) == S || error("set_initial_levels!: expected $S levels, got $(length(e0))")
    p = e0 === nothing ? Ptr{Cdouble}(C_NULL) : pointer(e0)
    GC.@preserve e0 begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_set_storage_initial_level, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.multi, p),
                             admm.multi)
        else
            dopf_check(ccall((:dopf_set_storage_initial_level, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.ctx, p), admm.ctx)
        end
    end
    return admm
end

"""
    set_terminal_levels!(admm, lo, hi)

The band `[lo[s], hi[s]]` of each storage's level after the last timestep (in the order of `storages`,
`0 <= lo[s] <= hi[s] <= max_level`, reachable from the initial level in T steps of at most `max_power`; `nothing` for both =
`[0, max_level]`): "end at least at X" is `[X, max_level]`, a cyclic horizon `lo = hi =` the initial level. The reference leaves
that level free; the ADMM must have been created with `flags = DOPF_F_STO_TERMINAL_LEVEL`. Takes effect at the next iteration.
"""
function set_terminal_levels!(admm::ADMM, lo::Union{Nothing, Vector{Float64}}, hi::Union{Nothing, Vector{Float64}})
    S = length(admm.storages)
    (lo === nothing) == (hi === nothing) || error("set_terminal_levels!: give both lo and hi, or neither")
    lo === nothing || (length(lo) == S && length(hi) == S) || error("set_terminal_levels!: expected $S values each")
    pl = lo === nothing ? Ptr{Cdouble}(C_NULL) : pointer(lo)
    ph = hi === nothing ? Ptr{Cdouble}(C_NULL) : pointer(hi)
    GC.@preserve lo hi begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_set_storage_terminal_level, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}),
                                   admm.multi, pl, ph), admm.multi)
        else
            dopf_check(ccall((:dopf_set_storage_terminal_level, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}),
                             admm.ctx, pl, ph), admm.ctx)
        end
    end
    return admm
end

"""
    set_line_rating!(admm, rating)

The lines' limits per timestep: `rating[l, t] >= 0`, an `L x T` matrix in the order of `lines` (`nothing` = `max_capacity` in every
timestep), so that `-rating[l, t] <= flow[l, t] <= rating[l, t]`. The reference keeps one `max_capacity` per line
(src/optimization/subproblems.jl:77-78); the ADMM must have been created with `flags = DOPF_F_LINE_RATING`. A rating of 0 pins the
flow to 0; it does not take the line out of the PTDF. The state and the iteration counter stay; takes effect at the next iteration.
"""
function set_line_rating!(admm::ADMM, rating::Union{Nothing, Matrix{Float64}})
    L, T = length(admm.L), length(admm.T)
    rating === nothing || size(rating) == (L, T) || error("set_line_rating!: expected an $L x $T matrix")
    pr = rating === nothing ? Ptr{Cdouble}(C_NULL) : pointer(rating)      # (column-major: [l + L*t], the library's layout)
    GC.@preserve rating begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_set_line_rating, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.multi, pr), admm.multi)
        else
            dopf_check(ccall((:dopf_set_line_rating, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.ctx, pr), admm.ctx)
        end
    end
    return admm
end

"""
    set_quadratic_cost!(admm, c2)

The quadratic cost coefficient of each generator (`c2[g] >= 0`, in the order of `generators`; `nothing` = all 0): the cost of output
`P` is `marginal_costs * P + c2 * P^2 / 2`. The reference keeps one constant `marginal_costs` per unit
(src/optimization/subproblems.jl:26-40; its `Generator` type, used verbatim, has no such field); the ADMM must have been created
with `flags = DOPF_F_GEN_QUADRATIC_COST`. The state and the iteration counter stay; takes effect at the next iteration.
"""
function set_quadratic_cost!(admm::ADMM, c2::Union{Nothing, Vector{Float64}})
    G = length(admm.generators)
    c2 === nothing || length(c2) == G || error("set_quadratic_cost!: expected $G coefficients, got $(length(c2))")
    p = c2 === nothing ? Ptr{Cdouble}(C_NULL) : pointer(c2)
    GC.@preserve c2 begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_set_generator_quadratic_cost, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.multi, p),
                             admm.multi)
        else
            dopf_check(ccall((:dopf_set_generator_quadratic_cost, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.ctx, p), admm.ctx)
        end
    end
    return admm
end

"""
    set_ramp!(admm, ramp_up, ramp_down, p_prev=nothing)

The ramp limits of each generator (`ramp_up[g], ramp_down[g] >= 0`, `Inf` = no limit, in the order of `generators`; both `nothing` =
all `Inf`) and optionally the outputs of the step before the window (`p_prev`, in `[0, max_generation]`; `nothing` = no anchor):
`-ramp_down <= P[g,t] - P[g,t-1] <= ramp_up`, at `t = 1` against `p_prev`. The reference's generators move freely between steps
(src/optimization/subproblems.jl:26-40); the ADMM must have been created with `flags = DOPF_F_GEN_RAMP` (with lines the constructor adds `DOPF_F_GEN_RAMP_NETWORK`).
The state and the iteration counter stay; takes effect at the next iteration.
"""
function set_ramp!(admm::ADMM, ramp_up::Union{Nothing, Vector{Float64}}, ramp_down::Union{Nothing, Vector{Float64}},
                   p_prev::Union{Nothing, Vector{Float64}}=nothing)
    G = length(admm.generators)
    for a in (ramp_up, ramp_down, p_prev)
        a === nothing || length(a) == G || error("set_ramp!: expected $G values, got $(length(a))")
    end
    (ramp_up === nothing) == (ramp_down === nothing) || error("set_ramp!: ramp_up and ramp_down must both be given or both be nothing")
    pu = ramp_up === nothing ? Ptr{Cdouble}(C_NULL) : pointer(ramp_up)
    pd = ramp_down === nothing ? Ptr{Cdouble}(C_NULL) : pointer(ramp_down)
    pp = p_prev === nothing ? Ptr{Cdouble}(C_NULL) : pointer(p_prev)
    GC.@preserve ramp_up ramp_down p_prev begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_set_generator_ramp, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                                   admm.multi, pu, pd, pp), admm.multi)
        else
            dopf_check(ccall((:dopf_set_generator_ramp, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                             admm.ctx, pu, pd, pp), admm.ctx)
        end
    end
    return admm
end

"""
    set_min_output!(admm, p_min)

The must-run floor of each generator (`0 <= p_min[g] <= max_generation`, in the order of `generators`; `nothing` = all 0):
`min(p_min[g], cap[g,t]) <= P[g,t]` — the floor follows an availability profile down, and `p_min = max_generation` is a must-take
unit. The reference's generators go down to 0. Minimum output runs on the ramp kernels: the ADMM must have been created with
`flags = DOPF_F_GEN_RAMP` (with lines the constructor adds `DOPF_F_GEN_RAMP_NETWORK`; the ramps stay `Inf` until `set_ramp!`), and
it does not combine with `DOPF_F2_GEN_ENERGY_BUDGET`. The state and the iteration counter stay; takes effect at the next iteration.
"""
function set_min_output!(admm::ADMM, p_min::Union{Nothing, Vector{Float64}})
    G = length(admm.generators)
    p_min === nothing || length(p_min) == G || error("set_min_output!: expected $G values, got $(length(p_min))")
    p = p_min === nothing ? Ptr{Cdouble}(C_NULL) : pointer(p_min)
    GC.@preserve p_min begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_set_generator_min_output, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.multi, p),
                             admm.multi)
        else
            dopf_check(ccall((:dopf_set_generator_min_output, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.ctx, p), admm.ctx)
        end
    end
    return admm
end

"""
    min_output(admm)

The floors as the context holds them (`dopf_get_generator_min_output`; a multi-GPU ADMM: not available).
"""
function min_output(admm::ADMM)
    admm.multi == C_NULL || error("min_output: not on a multi-GPU ADMM")
    out = zeros(Float64, length(admm.generators))
    GC.@preserve out dopf_check(ccall((:dopf_get_generator_min_output, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.ctx, pointer(out)), admm.ctx)
    return out
end

"""
    set_budget_min_output!(admm, p_min)

Must-run floors on an ADMM with energy budgets (`0 <= p_min[g] <= max_generation`, in the order of `generators`; `nothing` removes
them): `min(p_min[g], cap[g,t]) <= P[g,t] <= cap[g,t]` inside the budgets' own step, for every generator, budgeted or not — a
reservoir's minimum flow beside its water allotment. The ADMM must have been created with `flags2 = DOPF_F2_GEN_ENERGY_BUDGET` and
without `DOPF_F_GEN_RAMP` (there `set_min_output!` serves). A generator whose floors sum above its `energy_max` (or a window's) is
refused. The state and the iteration counter stay; takes effect at the next iteration.
"""
function set_budget_min_output!(admm::ADMM, p_min::Union{Nothing, Vector{Float64}})
    G = length(admm.generators)
    p_min === nothing || length(p_min) == G || error("set_budget_min_output!: expected $G values, got $(length(p_min))")
    p = p_min === nothing ? Ptr{Cdouble}(C_NULL) : pointer(p_min)
    GC.@preserve p_min begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_set_generator_budget_min_output, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.multi, p),
                             admm.multi)
        else
            dopf_check(ccall((:dopf_set_generator_budget_min_output, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.ctx, p), admm.ctx)
        end
    end
    return admm
end

"""
    budget_min_output(admm)

The floors of `set_budget_min_output!` as the context holds them (`dopf_get_generator_budget_min_output`; a multi-GPU ADMM: not
available).
"""
function budget_min_output(admm::ADMM)
    admm.multi == C_NULL || error("budget_min_output: not on a multi-GPU ADMM")
    out = zeros(Float64, length(admm.generators))
    GC.@preserve out dopf_check(ccall((:dopf_get_generator_budget_min_output, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.ctx, pointer(out)), admm.ctx)
    return out
end

"""
    set_energy_budget!(admm, e_min, e_max)

The energy budget of each generator over the window (`e_min[g] >= 0` finite, `e_max[g] >= e_min[g]`, `Inf` = no limit, in the order
of `generators`; `nothing` = all 0 / all `Inf`, each on its own): `e_min <= sum_t P[g,t] <= e_max` — a reservoir's water, a minimum
take, a fuel or emission cap. The reference's generators have no such row; the ADMM must have been created with
`flags2 = DOPF_F2_GEN_ENERGY_BUDGET`. The state and the iteration counter stay; takes effect at the next iteration.
"""
function set_energy_budget!(admm::ADMM, e_min::Union{Nothing, Vector{Float64}}, e_max::Union{Nothing, Vector{Float64}})
    G = length(admm.generators)
    for a in (e_min, e_max)
        a === nothing || length(a) == G || error("set_energy_budget!: expected $G values, got $(length(a))")
    end
    plo = e_min === nothing ? Ptr{Cdouble}(C_NULL) : pointer(e_min)
    phi = e_max === nothing ? Ptr{Cdouble}(C_NULL) : pointer(e_max)
    GC.@preserve e_min e_max begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_set_generator_energy_budget, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}),
                                   admm.multi, plo, phi), admm.multi)
        else
            dopf_check(ccall((:dopf_set_generator_energy_budget, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}),
                             admm.ctx, plo, phi), admm.ctx)
        end
    end
    return admm
end

"""
    budget_price(admm)

The water values of the run (`dopf_get_generator_budget_price`; a multi-GPU ADMM: `dopf_multi_get_generator_budget_price`): `nu[g]`,
the multiplier the last computed iteration put on generator g's energy budget, in the order of `generators` and the unit of the
marginal costs — `> 0` where `e_max` holds the unit down, `< 0` where `e_min` pushes it up, `0` for a unit without a budget or with
room in it. Recording starts with the FIRST call, which switches the generator kernel and returns zeros (a context with
`DOPF_F2_GEN_RAMP_BUDGET` records from the start): call it once before iterating. Zeros before the first iteration; the setters leave the values alone. At convergence `-budget_dual` of
`central_reference_coupled` where that dual is unique. The ADMM must have been created with `flags2 = DOPF_F2_GEN_ENERGY_BUDGET`.
"""
function budget_price(admm::ADMM)
    out = zeros(Float64, length(admm.generators))
    GC.@preserve out begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_get_generator_budget_price, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.multi,
                                   pointer(out)), admm.multi)
        else
            dopf_check(ccall((:dopf_get_generator_budget_price, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.ctx, pointer(out)), admm.ctx)
        end
    end
    return out
end

"""
    set_energy_budget_windows!(admm, win_end, e_min, e_max)

One energy budget per generator and sub-window of the horizon (`dopf_set_generator_energy_budget_windows`; a multi-GPU ADMM:
`dopf_multi_set_generator_energy_budget_windows`). `win_end` holds the windows' ends as the C ABI counts them: window j covers the
0-based timesteps `win_end[j-1] <= t < win_end[j]` (0 in front of the first), strictly increasing, the last one T. `e_min` and `e_max`
are `n_win x G` matrices in the order of `generators` (`nothing` = all 0 / all `Inf`): `e_min[j,g] <= sum over window j of P[g,t] <=
e_max[j,g]` — a daily allotment inside a weekly horizon. `win_end === nothing` removes the table. The ADMM must have been created with
`flags2 = DOPF_F2_GEN_ENERGY_BUDGET` (without ramps) and hold no whole-horizon budget. The state and the iteration counter stay; takes
effect at the next iteration.
"""
function set_energy_budget_windows!(admm::ADMM, win_end::Union{Nothing, Vector{Cint}}, e_min::Union{Nothing, Matrix{Float64}}=nothing,
                                    e_max::Union{Nothing, Matrix{Float64}}=nothing)
    G = length(admm.generators)
    nw = win_end === nothing ? 0 : length(win_end)
    for a in (e_min, e_max)
        a === nothing || (win_end !== nothing && size(a) == (nw, G)) || error("set_energy_budget_windows!: expected a $nw x $G matrix, got $(size(a))")
    end
    pend = win_end === nothing ? Ptr{Cint}(C_NULL) : pointer(win_end)
    plo = e_min === nothing ? Ptr{Cdouble}(C_NULL) : pointer(e_min)
    phi = e_max === nothing ? Ptr{Cdouble}(C_NULL) : pointer(e_max)
    GC.@preserve win_end e_min e_max begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_set_generator_energy_budget_windows, DOPF_LIB), Cint,
                                   (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}), admm.multi, nw, pend, plo, phi), admm.multi)
        else
            dopf_check(ccall((:dopf_set_generator_energy_budget_windows, DOPF_LIB), Cint,
                             (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}), admm.ctx, nw, pend, plo, phi), admm.ctx)
        end
    end
    return nothing
end

"""
    energy_budget_windows(admm)

The stored table (`dopf_get_generator_energy_budget_windows`, from the context's host copies): `(win_end, e_min, e_max)` with two
`n_win x G` matrices, or `nothing` while no table is set. One GPU only (`n_gpus == 1`).
"""
function energy_budget_windows(admm::ADMM)
    admm.multi == C_NULL || error("energy_budget_windows: one GPU only (no dopf_multi_* wrapper)")
    G, T = length(admm.generators), length(admm.T)
    nw = Ref{Cint}(0)
    ends = zeros(Cint, T)
    dopf_check(ccall((:dopf_get_generator_energy_budget_windows, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}),
                     admm.ctx, nw, ends, C_NULL, C_NULL), admm.ctx)
    nw[] == 0 && return nothing
    lo, hi = zeros(Float64, nw[], G), zeros(Float64, nw[], G)
    dopf_check(ccall((:dopf_get_generator_energy_budget_windows, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}),
                     admm.ctx, nw, ends, lo, hi), admm.ctx)
    return ends[1:nw[]], lo, hi
end

"""
    budget_window_price(admm, n_win)

The water values per sub-window (`dopf_get_generator_budget_window_price`; a multi-GPU ADMM:
`dopf_multi_get_generator_budget_window_price`): an `n_win x G` matrix, `nu[j,g]` the multiplier the last computed iteration put on
generator g's budget of window j, with `budget_price`'s sign convention. Always recorded while a table is set; `n_win` is the stored
table's number of windows.
"""
function budget_window_price(admm::ADMM, n_win::Int)
    out = zeros(Float64, n_win, length(admm.generators))
    GC.@preserve out begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_get_generator_budget_window_price, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.multi,
                                   pointer(out)), admm.multi)
        else
            dopf_check(ccall((:dopf_get_generator_budget_window_price, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.ctx, pointer(out)), admm.ctx)
        end
    end
    return out
end

"""
    ramp_price(admm)

The ramp prices of the run (`dopf_get_generator_ramp_price`; a multi-GPU ADMM: `dopf_multi_get_generator_ramp_price`): a `G x T`
matrix, `rp[g, t]` the multiplier the last computed iteration put on generator g's ramp row between `t-1` and `t` (the first column:
the row against the anchor `p_prev`, `0` without one), in the order of `generators` and the unit of the marginal costs — `> 0` where
`ramp_up` holds the unit back, `< 0` where `ramp_down` holds it up, `0` where no ramp binds. Recording starts with the FIRST call,
which switches the generator kernel and returns zeros: call it once before iterating. Zeros before the first iteration; the setters
leave the values alone. At convergence `-ramp_dual` of `central_reference_coupled` where that dual is unique. The ADMM must have been
created with `DOPF_F_GEN_RAMP` on a copper plate (network rows are not priced).
"""
function ramp_price(admm::ADMM)
    G = length(admm.generators)
    T = length(admm.T)
    out = zeros(Float64, T * G)
    GC.@preserve out begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_get_generator_ramp_price, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.multi,
                                   pointer(out)), admm.multi)
        else
            dopf_check(ccall((:dopf_get_generator_ramp_price, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.ctx, pointer(out)), admm.ctx)
        end
    end
    return permutedims(reshape(out, T, G))
end

"""
    set_efficiency!(admm, eta_c, eta_d)

The charge and discharge efficiency of each storage (`eta_c[s]`, `eta_d[s]` in `(0, 1]`, in the order of `storages`; `nothing`
for both = all 1): the level follows `E[t] = E[t-1] + eta_c * C[t] - D[t] / eta_d`. The reference's storages are lossless
(src/optimization/subproblems.jl:150-156); the ADMM must have been created with `flags = DOPF_F_STO_EFFICIENCY`. Takes effect at
the next iteration.
"""
function set_efficiency!(admm::ADMM, eta_c::Union{Nothing, Vector{Float64}}, eta_d::Union{Nothing, Vector{Float64}})
    S = length(admm.storages)
    (eta_c === nothing) == (eta_d === nothing) || error("set_efficiency!: give both eta_c and eta_d, or neither")
    eta_c === nothing || (length(eta_c) == S && length(eta_d) == S) || error("set_efficiency!: expected $S values each")
    pc = eta_c === nothing ? Ptr{Cdouble}(C_NULL) : pointer(eta_c)
    pd = eta_d === nothing ? Ptr{Cdouble}(C_NULL) : pointer(eta_d)
    GC.@preserve eta_c eta_d begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_set_storage_efficiency, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}),
                                   admm.multi, pc, pd), admm.multi)
        else
            dopf_check(ccall((:dopf_set_storage_efficiency, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}),
                             admm.ctx, pc, pd), admm.ctx)
        end
    end
    return admm
end

"""
    set_availability!(admm, profiles, profile_of)

The generators' availability: `profiles` is T x K (column k = one per-unit profile, values in [0, 1]), `profile_of[g]` the
profile of generator g (in the order of `generators`, 0-based, -1 = always `max_generation`); `nothing` for both = every
generator at `max_generation`. The box of generator g at t becomes `[0, max_generation * profiles[t, profile_of[g] + 1]]`. The
reference keeps one nameplate value per generator; the ADMM must have been created with `flags = DOPF_F_GEN_AVAILABILITY`.
Takes effect at the next iteration.
"""
function set_availability!(admm::ADMM, profiles::Union{Nothing, Matrix{Float64}}, profile_of::Union{Nothing, Vector{Cint}})
    T, G = length(admm.T), length(admm.generators)
    (profiles === nothing) == (profile_of === nothing) || error("set_availability!: give both profiles and profile_of, or neither")
    profiles === nothing || size(profiles, 1) == T || error("set_availability!: expected $T rows of profiles, got $(size(profiles, 1))")
    profile_of === nothing || length(profile_of) == G || error("set_availability!: expected $G profile indices")
    K = profiles === nothing ? 0 : size(profiles, 2)
    pp = profiles === nothing ? Ptr{Cdouble}(C_NULL) : pointer(profiles)        # T x K column-major = [t + T*k]
    po = profile_of === nothing ? Ptr{Cint}(C_NULL) : pointer(profile_of)
    GC.@preserve profiles profile_of begin
        if admm.multi != C_NULL
            dopf_check_multi(ccall((:dopf_multi_set_generator_availability, DOPF_LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cint}),
                                   admm.multi, K, pp, po), admm.multi)
        else
            dopf_check(ccall((:dopf_set_generator_availability, DOPF_LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cint}),
                             admm.ctx, K, pp, po), admm.ctx)
        end
    end
    return admm
end

# a new window: the recorded history starts anew from the duals the context holds now. (The nodes' own demand vectors stay as
# they were built: the reference's Node.demand is a Vector{Int}, a forecast need not be.)
function dopf_new_window!(admm::ADMM, total_demand::Vector{Float64})
    admm.total_demand = total_demand
    L, T = length(admm.L), length(admm.T)
    lam = zeros(T); mu = zeros(L, T); rho = zeros(L, T)
    dopf_check(ccall((:dopf_get_duals, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), admm.ctx, lam, mu, rho), admm.ctx)
    admm.lambdas = [lam]; admm.mues = [mu]; admm.rhos = [rho]
    admm.results = []
    admm.convergence = Convergence()
    it = Ref{Cint}(0); conv = Ref{Cint}(0)
    dopf_check(ccall((:dopf_sync, DOPF_LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}), admm.ctx, it, conv), admm.ctx)
    admm.iteration = Int(it[])
    return admm
end

"""
    set_demand!(admm, demand)

A new demand (`N x T`, row n = `admm.nodes[n]`) for the same window, replaced in place on the device: the primal state, the duals
and the iteration counter stay, injection, flows and prices are derived again, and the run is no longer converged. The reference
builds a new `ADMM(...)` per window (src/structures/admm.jl:23-62). One GPU only (`n_gpus == 1`).
"""
function set_demand!(admm::ADMM, demand::Matrix{Float64})
    N, T = length(admm.N), length(admm.T)
    size(demand) == (N, T) || error("set_demand!: expected a $N x $T demand, got $(size(demand))")
    admm.multi == C_NULL || error("set_demand!: one GPU only (no dopf_multi_* wrapper)")
    dopf_check(ccall((:dopf_set_demand, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.ctx, demand), admm.ctx)   # N x T column-major = [n + N*t]
    return dopf_new_window!(admm, vec(sum(demand, dims=1)))
end

"""
    roll_horizon!(admm, k, demand_tail)

The window advances by `k` steps, `1 <= k <= T - 1`, on the device: the state of the kept steps moves to the front and
warm-starts the new window, `demand_tail` (`N x k`) is the demand of the `k` new steps, every storage starts from the level it
had after step `k` (storages need `flags = DOPF_F_STO_INITIAL_LEVEL`), the iteration counter becomes 2. The terminal band now
applies to the new window's end; the availability profiles are not moved (`set_availability!`). The reference builds a new
`ADMM(...)` per window (src/structures/admm.jl:23-62). One GPU only (`n_gpus == 1`).
"""
function roll_horizon!(admm::ADMM, k::Int, demand_tail::Matrix{Float64})
    N, T = length(admm.N), length(admm.T)
    size(demand_tail) == (N, k) || error("roll_horizon!: expected a $N x $k demand tail, got $(size(demand_tail))")
    admm.multi == C_NULL || error("roll_horizon!: one GPU only (no dopf_multi_* wrapper)")
    dopf_check(ccall((:dopf_roll_horizon, DOPF_LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}), admm.ctx, k, demand_tail), admm.ctx)
    return dopf_new_window!(admm, vcat(admm.total_demand[k+1:end], vec(sum(demand_tail, dims=1))))
end

"""
    roll_horizon_coupled!(admm, k, demand_tail; availability=nothing, budget=nothing)

`roll_horizon!` for an ADMM with ramp limits or energy budgets, in place on the device: the ramps' anchor becomes the output of step
`k` (`P[g, k]`, 1-based), and what the `k` leaving steps delivered comes off both budgets, floored at 0. `availability =
(profiles, profile_of)` as `set_availability!` takes them (`(nothing, nothing)`: every generator back to `max_generation`) is the new
window's table, checked together with the new anchor and budgets; `nothing`: the stored table stays. `budget = (e_min, e_max)` as
`set_energy_budget!` takes them: the new window's own budgets instead of what is left. A refusal leaves the context as it was.
The reference builds a new `ADMM(...)` per window (src/structures/admm.jl:23-62). One GPU only (`n_gpus == 1`).
"""
function roll_horizon_coupled!(admm::ADMM, k::Int, demand_tail::Matrix{Float64}; availability=nothing, budget=nothing)
    N, T, G = length(admm.N), length(admm.T), length(admm.generators)
    size(demand_tail) == (N, k) || error("roll_horizon_coupled!: expected a $N x $k demand tail, got $(size(demand_tail))")
    admm.multi == C_NULL || error("roll_horizon_coupled!: one GPU only (no dopf_multi_* wrapper)")
    profiles, profile_of = availability === nothing ? (nothing, nothing) : availability
    (profiles === nothing) == (profile_of === nothing) || error("roll_horizon_coupled!: give both profiles and profile_of, or neither")
    profiles === nothing || size(profiles, 1) == T || error("roll_horizon_coupled!: expected $T rows of profiles, got $(size(profiles, 1))")
    profile_of === nothing || length(profile_of) == G || error("roll_horizon_coupled!: expected $G profile indices")
    K = availability === nothing ? -1 : (profiles === nothing ? 0 : size(profiles, 2))
    e_min, e_max = budget === nothing ? (nothing, nothing) : budget
    for a in (e_min, e_max)
        a === nothing || length(a) == G || error("roll_horizon_coupled!: expected $G values, got $(length(a))")
    end
    pp = profiles === nothing ? Ptr{Cdouble}(C_NULL) : pointer(profiles)        # T x K column-major = [t + T*k]
    po = profile_of === nothing ? Ptr{Cint}(C_NULL) : pointer(profile_of)
    plo = e_min === nothing ? Ptr{Cdouble}(C_NULL) : pointer(e_min)
    phi = e_max === nothing ? Ptr{Cdouble}(C_NULL) : pointer(e_max)
    GC.@preserve profiles profile_of e_min e_max begin
        dopf_check(ccall((:dopf_roll_horizon_coupled, DOPF_LIB), Cint,
                         (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cint}, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
                         admm.ctx, k, demand_tail, K, pp, po, budget === nothing ? 0 : 1, plo, phi), admm.ctx)
    end
    return dopf_new_window!(admm, vcat(admm.total_demand[k+1:end], vec(sum(demand_tail, dims=1))))
end

"""
    generator_coupling(admm)

`(ramp_up, ramp_down, p_prev, e_min, e_max)` as the context holds them, one value per generator in the order of `generators`
(`p_prev` is `NaN` where no anchor is stored; without the flags: `Inf`, `Inf`, `NaN`, 0, `Inf`). After `roll_horizon_coupled!` they
are what the device computed. One GPU only (`n_gpus == 1`).
"""
function generator_coupling(admm::ADMM)
    admm.multi == C_NULL || error("generator_coupling: one GPU only (no dopf_multi_* wrapper)")
    G = length(admm.generators)
    up = zeros(G); down = zeros(G); prev = zeros(G); lo = zeros(G); hi = zeros(G)
    dopf_check(ccall((:dopf_get_generator_coupling, DOPF_LIB), Cint,
                     (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), admm.ctx, up, down, prev, lo, hi), admm.ctx)
    return (ramp_up=up, ramp_down=down, p_prev=prev, e_min=lo, e_max=hi)
end

"""The fields of the reference's Result (src/structures/results.jl:37-48) for the last solved iteration."""
function dopf_result(admm::ADMM)
    N, L, T = length(admm.N), length(admm.L), length(admm.T)
    inj = zeros(N, T); aU = zeros(L, T); aK = zeros(L, T); fl = zeros(L, T)
    cost = Ref{Cdouble}(0.0)
    dopf_check(ccall((:dopf_get_consensus, DOPF_LIB), Cint,
                     (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}),
                     admm.ctx, inj, aU, aK, fl, cost), admm.ctx)
    P, D, C, E = dopf_primal(admm)
    # ResultNode.{generation, discharge, charge} (src/structures/results.jl:19-35): N x T, row n = admm.nodes[n]
    ng = zeros(N, T); nd = zeros(N, T); nc = zeros(N, T)
    dopf_check(ccall((:dopf_get_node_results, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                     admm.ctx, ng, nd, nc), admm.ctx)
    return (generation=P, discharge=D, charge=C, level=E, injection=inj, avg_U=aU, avg_K=aK,
            line_utilization=fl, total_costs=cost[], node_generation=ng, node_discharge=nd, node_charge=nc)
end

"""
Result.penalty_term of the last solved iteration (src/structures/results.jl:66-70: the units' PenaltyTerms summed,
src/helpers/penalty_terms.jl:1-6) as `(energy_balance, upper_flow, lower_flow)`, T values each — one pass on the device.
Needs lines and `flags` containing DOPF_F_KEEP_DELTAS at construction (the device then keeps every unit's injection change).
"""
function dopf_penalty_sums(admm::ADMM)
    T = length(admm.T)
    pen = zeros(3 * T)
    dopf_check(ccall((:dopf_get_penalty_sums, DOPF_LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), admm.ctx, pen), admm.ctx)
    return (energy_balance=pen[1:T], upper_flow=pen[T+1:2T], lower_flow=pen[2T+1:3T])
end

# after a batch of iterations: iteration counter, stop flags, the dual sets get_nodal_price needs
function dopf_refresh!(admm::ADMM, converged::Bool)
    a = Ref{Cdouble}(0.0); b = Ref{Cdouble}(0.0); c = Ref{Cdouble}(0.0); it = Ref{Cint}(0)
    dopf_check(ccall((:dopf_get_residuals, DOPF_LIB), Cint, (Ptr{Cvoid}, Ref{Cdouble}, Ref{Cdouble}, Ref{Cdouble}, Ref{Cint}),
                     admm.ctx, a, b, c, it), admm.ctx)
    admm.iteration = Int(it[])
    admm.convergence.all = converged
    if converged
        admm.convergence.lambda = true; admm.convergence.mue = true; admm.convergence.rho = true
    end
    return a[], b[], c[]
end

"""
    calculate_iteration!(admm; n = 1)

`n` ADMM iterations on the device (all sub-problems, consensus sums, dual update, stop test; src/optimization/run.jl:7-16
without the printing). With `admm.record` the duals and a Result-like NamedTuple are pushed per iteration like the
reference does (then n is forced to 1); otherwise only the dual sets of the last step are kept.
"""
function calculate_iteration!(admm::ADMM; n::Int=1)
    n = admm.record ? 1 : n
    done = Ref{Cint}(0); conv = Ref{Cint}(0)
    if admm.multi != C_NULL
        dopf_check_multi(ccall((:dopf_multi_iterate, DOPF_LIB), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}, Ref{Cint}), admm.multi, n, done, conv), admm.multi)
    else
        dopf_check(ccall((:dopf_iterate, DOPF_LIB), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}, Ref{Cint}), admm.ctx, n, done, conv), admm.ctx)
    end
    done[] == 0 && return 0
    dopf_refresh!(admm, conv[] != 0)
    used = dopf_duals(admm; used=true)
    now = dopf_duals(admm)
    if admm.record
        push!(admm.results, dopf_result(admm))
        push!(admm.lambdas, now[1]); push!(admm.mues, now[2]); push!(admm.rhos, now[3])     # update_duals.jl:14,26,38
        push!(admm.convergence.lambda_res, abs.(now[1] - used[1]))
        push!(admm.convergence.mue_res, abs.(now[2] - used[2]))
        push!(admm.convergence.rho_res, abs.(now[3] - used[3]))
    else
        admm.lambdas = [used[1], now[1]]; admm.mues = [used[2], now[2]]; admm.rhos = [used[3], now[3]]
    end
    return Int(done[])
end

"""run!(admm): iterate until every |dual change| < eps — tested on the device exactly like check_convergence!
(no test at iteration 1, the counter is not bumped on the converging step) — or the iteration cap is reached."""
function run!(admm::ADMM; chunk::Int=64)
    while !admm.convergence.all
        calculate_iteration!(admm; n=chunk) == 0 && break      # iteration cap reached
    end
    return admm
end

"""
    run_recorded!(admm; chunk = 64)

`run!` with the history recorded on the device (dopf_trace_*, include/dopf.h): the iterations run `chunk` at a time, back to back,
each writing its slot of a device ring, and the host reads a chunk's slots afterwards — one round trip per chunk where
`calculate_iteration!` with `admm.record` makes one, and its blocking copies, per iteration. Pushes to `admm.results`, `lambdas`,
`mues`, `rhos` and `convergence` what `run!` pushes (the residual vectors from consecutive duals; the node results summed here from
the slot's P, D and C). Needs `ADMM(...; record=true)` and a single device (`n_gpus = 1`: a sharded history is not recorded).
"""
function run_recorded!(admm::ADMM; chunk::Int=64)
    admm.record || error("run_recorded! records the iteration history (create ADMM(...; record=true))")
    admm.multi == C_NULL || error("run_recorded!: a sharded history is not recorded (n_gpus = 1)")
    chunk >= 1 || error("run_recorded!: chunk = $chunk < 1")
    N, L, T = length(admm.N), length(admm.L), length(admm.T)
    G, S = length(admm.generators), length(admm.storages)
    gen_node = Int[admm.node_to_id[g.node] for g in admm.generators]
    sto_node = Int[admm.node_to_id[s.node] for s in admm.storages]
    what = DOPF_TRACE_DUALS | DOPF_TRACE_CONSENSUS | DOPF_TRACE_PRIMAL
    dopf_check(ccall((:dopf_trace_begin, DOPF_LIB), Cint, (Ptr{Cvoid}, Cint, Cint), admm.ctx, what, chunk), admm.ctx)
    try
        while !admm.convergence.all
            dopf_check(ccall((:dopf_trace_reset, DOPF_LIB), Cint, (Ptr{Cvoid},), admm.ctx), admm.ctx)
            done = Ref{Cint}(0); conv = Ref{Cint}(0)
            dopf_check(ccall((:dopf_iterate, DOPF_LIB), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}, Ref{Cint}), admm.ctx, chunk, done, conv), admm.ctx)
            n = Int(done[])
            n == 0 && break                                   # iteration cap reached
            w = Ref{Cint}(0); cap = Ref{Cint}(0); held = Ref{Cint}(0); rec = Ref{Cint}(0)
            dopf_check(ccall((:dopf_trace_info, DOPF_LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Cint}, Ref{Cint}),
                             admm.ctx, w, cap, held, rec), admm.ctx)
            Int(held[]) == n || error("trace: $(held[]) slots held after $n iterations")
            rows = zeros(4, n); its = zeros(Cint, n); cvs = zeros(Cint, n)
            lam = zeros(T, n); mu = zeros(L, T, n); rho = zeros(L, T, n)
            inj = zeros(N, T, n); aU = zeros(L, T, n); aK = zeros(L, T, n); fl = zeros(L, T, n)
            P = zeros(T, G, n); D = zeros(T, S, n); C = zeros(T, S, n); E = zeros(T, S, n)
            dopf_check(ccall((:dopf_trace_read, DOPF_LIB), Cint,
                             (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                              Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                             admm.ctx, 0, n, rows, its, cvs, lam, mu, rho, inj, aU, aK, fl, P, D, C, E), admm.ctx)
            for i in 1:n
                # ResultNode.{generation, discharge, charge} (src/structures/results.jl:19-35): the units of a node, summed here
                ng = zeros(N, T); nd = zeros(N, T); nc = zeros(N, T)
                for g in 1:G
                    ng[gen_node[g], :] += P[:, g, i]
                end
                for s in 1:S
                    nd[sto_node[s], :] += D[:, s, i]
                    nc[sto_node[s], :] += C[:, s, i]
                end
                push!(admm.results, (generation=P[:, :, i], discharge=D[:, :, i], charge=C[:, :, i], level=E[:, :, i],
                                     injection=inj[:, :, i], avg_U=aU[:, :, i], avg_K=aK[:, :, i], line_utilization=fl[:, :, i],
                                     total_costs=rows[4, i], node_generation=ng, node_discharge=nd, node_charge=nc))
                push!(admm.lambdas, lam[:, i]); push!(admm.mues, mu[:, :, i]); push!(admm.rhos, rho[:, :, i])
                push!(admm.convergence.lambda_res, abs.(admm.lambdas[end] - admm.lambdas[end-1]))
                push!(admm.convergence.mue_res, abs.(admm.mues[end] - admm.mues[end-1]))
                push!(admm.convergence.rho_res, abs.(admm.rhos[end] - admm.rhos[end-1]))
            end
            dopf_refresh!(admm, cvs[n] != 0)
        end
    finally
        ccall((:dopf_trace_end, DOPF_LIB), Cint, (Ptr{Cvoid},), admm.ctx)
    end
    return admm
end

"""
    get_nodal_price(iteration)

The reference's signature (src/helpers/network_elements.jl:16-25): reads the GLOBAL `admm` and evaluates
`lambdas[iteration] .+ sum((mues[iteration] + rhos[iteration])[l, t] * ptdf[l, :])`. `iteration == admm.iteration`
(what src/opf_admm_decentral.jl:9 asks for) are the duals the last solve used; with `record = true` any past
iteration works, without it only the last two dual sets exist.
"""
function get_nodal_price(iteration::Int)
    a = admm                                   # the global of the driver script, as in the reference
    idx = a.record ? iteration : (iteration == a.iteration ? 1 : (iteration == a.iteration + 1 ? 2 : 0))
    (idx < 1 || idx > length(a.lambdas)) && error("duals of iteration $iteration are not kept (create ADMM(...; record=true))")
    nodal_price = zeros(length(a.N), length(a.T))
    for t in a.T
        nodal_price[:, t] .= a.lambdas[idx][t]
        for l in a.L
            nodal_price[:, t] .+= (a.mues[idx][l, t] + a.rhos[idx][l, t]) .* a.ptdf[l, :]
        end
    end
    return nodal_price
end

"""
    export_results(admm, filename; parent_dir = "results/")

The reference's export (src/helpers/output.jl:1-85): `<filename>_duals.csv` (iteration,dual,timestep,line,value; duals
lambda, rho, mue in that order; `line` empty for lambda; row i = the dual USED in iteration i), `<filename>_generators.csv`
(iteration,generator,timestep,generation) and `<filename>_storages.csv` (iteration,storage,timestep,charge,discharge), one
row per iteration 1..admm.iteration, written as plain text (no CSV.jl / DataFrames needed). Needs the iteration history:
`ADMM(...; record = true)` — which is also what any reference-style script that reads `admm.results[end]` needs.
"""
function export_results(admm::ADMM, filename::String; parent_dir::String="results/")
    admm.record || error("export_results needs the iteration history: create ADMM(...; record = true)")
    mkpath(parent_dir)
    n_it = min(admm.iteration, length(admm.results))
    open(joinpath(parent_dir, filename * "_duals.csv"), "w") do f
        println(f, "iteration,dual,timestep,line,value")
        for (name, hist) in (("lambda", admm.lambdas), ("rho", admm.rhos), ("mue", admm.mues))
            for i in 1:n_it, t in admm.T
                if name == "lambda"
                    println(f, i, ",lambda,", t, ",,", hist[i][t])
                else
                    for l in admm.L
                        println(f, i, ",", name, ",", t, ",", l, ",", hist[i][l, t])
                    end
                end
            end
        end
    end
    open(joinpath(parent_dir, filename * "_generators.csv"), "w") do f
        println(f, "iteration,generator,timestep,generation")
        for (g, gen) in enumerate(admm.generators), i in 1:n_it, t in admm.T
            println(f, i, ",", gen.name, ",", t, ",", admm.results[i].generation[t, g])
        end
    end
    open(joinpath(parent_dir, filename * "_storages.csv"), "w") do f
        println(f, "iteration,storage,timestep,charge,discharge")
        for (s, sto) in enumerate(admm.storages), i in 1:n_it, t in admm.T
            println(f, i, ",", sto.name, ",", t, ",", admm.results[i].charge[t, s], ",", admm.results[i].discharge[t, s])
        end
    end
    return nothing
end

struct CCentralResult          # == struct dopf_central_result (include/dopf.h)
    objective::Cdouble
    dual_objective::Cdouble
    primal_infeasibility::Cdouble
    gap::Cdouble
    iterations::Cint
    converged::Cint
end

"""
    central_reference(nodes, generators, storages, lines; tol = 1e-9, max_iters = 200000,
                      initial_level = nothing, terminal_level = nothing, availability = nothing, efficiency = nothing)

What src/opf_central_reference.jl computes — objective, P, D, C, line utilisation, system price `dual.(EB)`, nodal price —
from the whole problem as ONE LP, solved on the GPU by libdopf_hip's first-order method (no modelling layer, no licensed solver).
Returns a NamedTuple; matrices are units x timesteps like `value.(P).data`.

`initial_level` (S levels before the first timestep), `terminal_level = (lo, hi)` (S bounds each of the level after the last
timestep) and `availability = (profiles, profile_of)` (T x K and G 0-based indices, -1 = always `max_generation`) are the inputs of
`set_initial_levels!`, `set_terminal_levels!` and `set_availability!`: with any of them the LP of a decentral run that uses them is
solved (`dopf_central_solve_ex`, same checks as those setters), and `level` includes the initial level.

`efficiency = (eta_c, eta_d)` (S values each in (0, 1]) is the input of `set_efficiency!`: the LP with lossy storages,
`level = initial_level + cumsum(eta_c C - D / eta_d)`, solved by `dopf_central_solve_lossy` (called only when the keyword is set).
"""
function central_reference(nodes::Vector{Node}, generators::Vector{Generator}, storages::Vector{Storage}, lines::Vector{Line};
                           tol::Float64=1e-9, max_iters::Int=200000, device::Int=-1,
                           initial_level::Union{Nothing, Vector{Float64}}=nothing,
                           terminal_level::Union{Nothing, Tuple{Vector{Float64}, Vector{Float64}}}=nothing,
                           availability::Union{Nothing, Tuple{Matrix{Float64}, Vector{Cint}}}=nothing,
                           efficiency::Union{Nothing, Tuple{Vector{Float64}, Vector{Float64}}}=nothing)
    N, L, T = length(nodes), length(lines), length(nodes[1].demand)
    G, S = length(generators), length(storages)
    node_to_id = Dict{Node, Int}(n => i for (i, n) in enumerate(nodes))
    demand = Float64[nodes[n].demand[t] for n in 1:N, t in 1:T]
    ptdf = L > 0 ? Matrix{Float64}(calculate_ptdf(nodes, lines)) : zeros(Float64, 0, N)
    f_max = Float64[l.max_capacity for l in lines]
    gen_mc = Float64[g.marginal_costs for g in generators]
    gen_pmax = Float64[g.max_generation for g in generators]
    gen_node = Cint[node_to_id[g.node] - 1 for g in generators]
    sto_mc = Float64[s.marginal_costs for s in storages]
    sto_pmax = Float64[s.max_power for s in storages]
    sto_emax = Float64[s.max_level for s in storages]
    sto_node = Cint[node_to_id[s.node] - 1 for s in storages]
    P = zeros(T, G); D = zeros(T, S); C = zeros(T, S); E = zeros(T, S)
    lambda = zeros(T); nodal = zeros(N, T); util = zeros(L, T)
    flow_upper = zeros(L, T); flow_lower = zeros(L, T)          # dual.(FlowUpper), dual.(FlowLower), opf_central_reference.jl:71
    res = Ref(CCentralResult(0.0, 0.0, 0.0, 0.0, 0, 0))
    initial_level === nothing || length(initial_level) == S || error("central_reference: expected $S initial levels")
    terminal_level === nothing || (length(terminal_level[1]) == S && length(terminal_level[2]) == S) ||
        error("central_reference: expected $S terminal bounds each")
    availability === nothing || (size(availability[1], 1) == T && length(availability[2]) == G) ||
        error("central_reference: expected $T rows of profiles and $G profile indices")
    efficiency === nothing || (length(efficiency[1]) == S && length(efficiency[2]) == S) ||
        error("central_reference: expected $S efficiencies each")
    extended = initial_level !== nothing || terminal_level !== nothing || availability !== nothing || efficiency !== nothing
    GC.@preserve demand ptdf f_max gen_mc gen_pmax gen_node sto_mc sto_pmax sto_emax sto_node initial_level terminal_level availability efficiency begin
        prob = Ref(CProblem(N, L, T, G, S, pointer(demand), pointer(ptdf), pointer(f_max), pointer(gen_mc),
                            pointer(gen_pmax), pointer(gen_node), pointer(sto_mc), pointer(sto_pmax),
                            pointer(sto_emax), pointer(sto_node)))
        par = Ref(CParams(0.3, 10.0, 1.0, 1e-3, 1e-2, 0, 0, device, 0, C_NULL))
        if extended
            pe = initial_level === nothing ? Ptr{Cdouble}(C_NULL) : pointer(initial_level)
            plo = terminal_level === nothing ? Ptr{Cdouble}(C_NULL) : pointer(terminal_level[1])
            phi = terminal_level === nothing ? Ptr{Cdouble}(C_NULL) : pointer(terminal_level[2])
            K = availability === nothing ? 0 : size(availability[1], 2)
            pf = availability === nothing ? Ptr{Cdouble}(C_NULL) : pointer(availability[1])      # T x K column-major = [t + T*k]
            po = availability === nothing ? Ptr{Cint}(C_NULL) : pointer(availability[2])
            if efficiency !== nothing
                rc = ccall((:dopf_central_solve_lossy, DOPF_LIB), Cint,
                           (Ref{CProblem}, Ref{CParams}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble},
                            Ptr{Cint}, Cdouble, Cint, Ref{CCentralResult}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                            Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                           prob, par, pe, plo, phi, pointer(efficiency[1]), pointer(efficiency[2]), K, pf, po, tol, max_iters, res, P, D, C, E,
                           lambda, nodal, util, flow_upper, flow_lower)
            else
                rc = ccall((:dopf_central_solve_ex, DOPF_LIB), Cint,
                           (Ref{CProblem}, Ref{CParams}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cint}, Cdouble, Cint,
                            Ref{CCentralResult}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                            Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                           prob, par, pe, plo, phi, K, pf, po, tol, max_iters, res, P, D, C, E, lambda, nodal, util, flow_upper, flow_lower)
            end
        else
            rc = ccall((:dopf_central_solve, DOPF_LIB), Cint,
                       (Ref{CProblem}, Ref{CParams}, Cdouble, Cint, Ref{CCentralResult}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                        Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                       prob, par, tol, max_iters, res, P, D, C, E, lambda, nodal, util, flow_upper, flow_lower)
        end
        dopf_check(rc, Ptr{Cvoid}(C_NULL))
    end
    res[].converged == 0 && error("central LP: gap $(res[].gap) after $(res[].iterations) iterations")
    return (objective=res[].objective, generation=permutedims(P), discharge=permutedims(D), charge=permutedims(C),
            level=permutedims(E), line_utilization=util, system_price=lambda, nodal_price=nodal,
            flow_upper_dual=flow_upper, flow_lower_dual=flow_lower)
end

"""
    central_reference_coupled(nodes, generators, storages, lines; tol = 1e-9, max_iters = 200000,
                              initial_level = nothing, terminal_level = nothing, availability = nothing, efficiency = nothing,
                              line_rating = nothing, ramp = nothing, p_prev = nothing, energy_budget = nothing)

`central_reference` with the inputs of `set_line_rating!`, `set_ramp!` and `set_energy_budget!`: the LP of a decentral run that uses
them, solved on the GPU by `dopf_central_solve_coupled` (same checks as those setters; ramps and budgets may be given together).
`line_rating` is L x T, `ramp = (up, down)` G values each (`Inf` = no limit), `p_prev` the G outputs of the step before the window,
`energy_budget = (e_min, e_max)` G values each. Returns `central_reference`'s NamedTuple plus `ramp_dual` (G x T) and `budget_dual`
(G): d objective / d right-hand side of the ramp row between t - 1 and t (t = 1: the anchor's row) and of the budget row, negative
where the row's upper end binds and positive where its lower end does.
"""
function central_reference_coupled(nodes::Vector{Node}, generators::Vector{Generator}, storages::Vector{Storage}, lines::Vector{Line};
                                   tol::Float64=1e-9, max_iters::Int=200000, device::Int=-1,
                                   initial_level::Union{Nothing, Vector{Float64}}=nothing,
                                   terminal_level::Union{Nothing, Tuple{Vector{Float64}, Vector{Float64}}}=nothing,
                                   availability::Union{Nothing, Tuple{Matrix{Float64}, Vector{Cint}}}=nothing,
                                   efficiency::Union{Nothing, Tuple{Vector{Float64}, Vector{Float64}}}=nothing,
                                   line_rating::Union{Nothing, Matrix{Float64}}=nothing,
                                   ramp::Union{Nothing, Tuple{Vector{Float64}, Vector{Float64}}}=nothing,
                                   p_prev::Union{Nothing, Vector{Float64}}=nothing,
                                   energy_budget::Union{Nothing, Tuple{Vector{Float64}, Vector{Float64}}}=nothing)
    N, L, T = length(nodes), length(lines), length(nodes[1].demand)
    G, S = length(generators), length(storages)
    node_to_id = Dict{Node, Int}(n => i for (i, n) in enumerate(nodes))
    demand = Float64[nodes[n].demand[t] for n in 1:N, t in 1:T]
    ptdf = L > 0 ? Matrix{Float64}(calculate_ptdf(nodes, lines)) : zeros(Float64, 0, N)
    f_max = Float64[l.max_capacity for l in lines]
    gen_mc = Float64[g.marginal_costs for g in generators]
    gen_pmax = Float64[g.max_generation for g in generators]
    gen_node = Cint[node_to_id[g.node] - 1 for g in generators]
    sto_mc = Float64[s.marginal_costs for s in storages]
    sto_pmax = Float64[s.max_power for s in storages]
    sto_emax = Float64[s.max_level for s in storages]
    sto_node = Cint[node_to_id[s.node] - 1 for s in storages]
    P = zeros(T, G); D = zeros(T, S); C = zeros(T, S); E = zeros(T, S)
    lambda = zeros(T); nodal = zeros(N, T); util = zeros(L, T)
    flow_upper = zeros(L, T); flow_lower = zeros(L, T)
    ramp_dual = zeros(T, G); budget_dual = zeros(G)
    res = Ref(CCentralResult(0.0, 0.0, 0.0, 0.0, 0, 0))
    initial_level === nothing || length(initial_level) == S || error("central_reference_coupled: expected $S initial levels")
    terminal_level === nothing || (length(terminal_level[1]) == S && length(terminal_level[2]) == S) ||
        error("central_reference_coupled: expected $S terminal bounds each")
    availability === nothing || (size(availability[1], 1) == T && length(availability[2]) == G) ||
        error("central_reference_coupled: expected $T rows of profiles and $G profile indices")
    efficiency === nothing || (length(efficiency[1]) == S && length(efficiency[2]) == S) ||
        error("central_reference_coupled: expected $S efficiencies each")
    line_rating === nothing || size(line_rating) == (L, T) || error("central_reference_coupled: expected a $L x $T rating table")
    ramp === nothing || (length(ramp[1]) == G && length(ramp[2]) == G) || error("central_reference_coupled: expected $G ramps each")
    p_prev === nothing || length(p_prev) == G || error("central_reference_coupled: expected $G previous outputs")
    energy_budget === nothing || (length(energy_budget[1]) == G && length(energy_budget[2]) == G) ||
        error("central_reference_coupled: expected $G budget bounds each")
    dptr(a) = a === nothing ? Ptr{Cdouble}(C_NULL) : pointer(a)
    GC.@preserve demand ptdf f_max gen_mc gen_pmax gen_node sto_mc sto_pmax sto_emax sto_node initial_level terminal_level availability efficiency line_rating ramp p_prev energy_budget begin
        prob = Ref(CProblem(N, L, T, G, S, pointer(demand), pointer(ptdf), pointer(f_max), pointer(gen_mc),
                            pointer(gen_pmax), pointer(gen_node), pointer(sto_mc), pointer(sto_pmax),
                            pointer(sto_emax), pointer(sto_node)))
        par = Ref(CParams(0.3, 10.0, 1.0, 1e-3, 1e-2, 0, 0, device, 0, C_NULL))
        K = availability === nothing ? 0 : size(availability[1], 2)
        po = availability === nothing ? Ptr{Cint}(C_NULL) : pointer(availability[2])
        rc = ccall((:dopf_central_solve_coupled, DOPF_LIB), Cint,
                   (Ref{CProblem}, Ref{CParams}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble},
                    Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cint,
                    Ref{CCentralResult}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                    Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                   prob, par, dptr(initial_level), dptr(terminal_level === nothing ? nothing : terminal_level[1]),
                   dptr(terminal_level === nothing ? nothing : terminal_level[2]), dptr(efficiency === nothing ? nothing : efficiency[1]),
                   dptr(efficiency === nothing ? nothing : efficiency[2]), K, dptr(availability === nothing ? nothing : availability[1]), po,
                   dptr(line_rating), dptr(ramp === nothing ? nothing : ramp[1]), dptr(ramp === nothing ? nothing : ramp[2]), dptr(p_prev),
                   dptr(energy_budget === nothing ? nothing : energy_budget[1]), dptr(energy_budget === nothing ? nothing : energy_budget[2]),
                   tol, max_iters, res, P, D, C, E, lambda, nodal, util, flow_upper, flow_lower, ramp_dual, budget_dual)
        dopf_check(rc, Ptr{Cvoid}(C_NULL))
    end
    res[].converged == 0 && error("central LP: gap $(res[].gap) after $(res[].iterations) iterations")
    return (objective=res[].objective, generation=permutedims(P), discharge=permutedims(D), charge=permutedims(C),
            level=permutedims(E), line_utilization=util, system_price=lambda, nodal_price=nodal,
            flow_upper_dual=flow_upper, flow_lower_dual=flow_lower, ramp_dual=permutedims(ramp_dual), budget_dual=budget_dual)
end
