/*
 * dopf.h — C ABI of libdopf_hip: the MI355X-native ADMM consensus-OPF inner loop.
 *
 * This is the drop-in boundary for the hot path of rockstaedt/DecentralOPF.jl
 * (reference paths are relative to the reference checkout):
 *
 *   dopf_create            replaces  ADMM(gamma, nodes, generators, storages, lines)
 *                                    src/structures/admm.jl:23-62 (state, zero duals, maps)
 *   dopf_iterate           replaces  run!(admm) / calculate_iteration!(admm)
 *                                    src/optimization/run.jl:1-16
 *                                    = optimize_all_subproblems!  src/optimization/subproblems.jl:1-17
 *                                    + update_duals!              src/optimization/update_duals.jl:1-39
 *                                    + check_convergence!         src/optimization/convergence.jl:1-31
 *   dopf_local_update      replaces  optimize_subproblem.(generators|storages)
 *                                    src/optimization/subproblems.jl:19-207 (+ penalty_terms.jl:1-53)
 *                                    and the agent sums of Result(...) src/structures/results.jl:50-106
 *   dopf_apply_consensus   replaces  the rest of Result(...) (avg_U/avg_K, line_utilization,
 *                                    results.jl:108-116), update_duals! and check_convergence!
 *   dopf_get_duals         replaces  admm.lambdas[end], admm.mues[end], admm.rhos[end]
 *   dopf_get_duals_used    replaces  admm.lambdas[admm.iteration] ... (the duals the last solve used;
 *                                    these feed get_nodal_price(admm.iteration),
 *                                    src/opf_admm_decentral.jl:9)
 *   dopf_get_primal        replaces  ResultGenerator.generation / ResultStorage.{discharge,charge,level}
 *                                    src/structures/results.jl:1-17
 *   dopf_get_consensus     replaces  Result.{injection,avg_U,avg_K,line_utilization,total_costs}
 *                                    src/structures/results.jl:37-48
 *   dopf_get_residuals     replaces  Convergence.{lambda_res,mue_res,rho_res} (inf-norms)
 *                                    src/structures/convergence.jl:1-20
 *   dopf_get_nodal_price   replaces  get_nodal_price(iteration) src/helpers/network_elements.jl:16-25
 *   dopf_set_state         (no reference counterpart: resume / trajectory tests; the reference
 *                                    keeps whole histories in admm.results / admm.lambdas instead)
 *   dopf_trace_*           replaces  those histories: admm.lambdas / mues / rhos / results / convergence, one
 *                                    entry per iteration (src/structures/admm.jl, src/optimization/run.jl:1-16)
 *
 * Conventions
 *   - all matrices are Julia column-major: demand[n + N*t], ptdf[l + L*n], mu[l + L*t];
 *   - per-agent time series are agent-major: P[t + T*g], D/C/E[t + T*s];
 *   - node ids are 0-based int32; all reals are double (the reference computes in Float64);
 *   - every pointer argument is caller-owned HOST memory, copied in or out before return
 *     (no aliasing of the caller's GC memory after the call returns), except the device
 *     pointer handed to dopf_bind_consensus (see there);
 *   - return 0 = ok, negative = error (DOPF_E_*); message via dopf_last_error;
 *     no exception or longjmp crosses this boundary;
 *   - a context is driven by one host thread at a time.
 *
 * The same signatures, prefixed oracle_ instead of dopf_, are implemented by the CPU oracle
 * (oracle/dopf_oracle.c). The oracle is test infrastructure, never a fallback of this library.
 */
#ifndef DOPF_H
#define DOPF_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DOPF_OK            0
#define DOPF_E_INVALID    -1   /* bad argument / inconsistent sizes */
#define DOPF_E_NOMEM      -2
#define DOPF_E_DEVICE     -3   /* HIP runtime error (message has the hipError string) */
#define DOPF_E_UNSUPPORTED -4
#define DOPF_E_SOLVER     -5   /* an agent sub-problem did not reach its tolerance */

typedef struct dopf_ctx dopf_ctx;

/* One OPF instance (or one rank's shard of it: G and S then count the LOCAL agents,
 * everything else is the global network). Mirrors the fields ADMM(...) derives from the
 * Node/Generator/Storage/Line vectors, src/structures/admm.jl:28-60. */
typedef struct dopf_problem {
    int32_t N, L, T, G, S;
    const double  *demand;    /* N x T, [n + N*t]   (Node.demand, promoted Int -> Float64)      */
    const double  *ptdf;      /* L x N, [l + L*n]   (calculate_ptdf, src/helpers/ptdf.jl:1-41)   */
    const double  *f_max;     /* L                  (Line.max_capacity)                          */
    const double  *gen_mc;    /* G                  (Generator.marginal_costs)                   */
    const double  *gen_pmax;  /* G                  (Generator.max_generation)                   */
    const int32_t *gen_node;  /* G, 0-based                                                      */
    const double  *sto_mc;    /* S                  (Storage.marginal_costs)                     */
    const double  *sto_pmax;  /* S                  (Storage.max_power)                          */
    const double  *sto_emax;  /* S                  (Storage.max_level)                          */
    const int32_t *sto_node;  /* S, 0-based                                                      */
} dopf_problem;

/* The literals of the reference, collected (SURVEY.md section 5 "Config / flags"). */
typedef struct dopf_params {
    double  gamma;      /* 0.3   src/opf_admm_decentral.jl:5  (BASELINE.json calls it rho)      */
    double  w_flow;     /* 10    src/optimization/subproblems.jl:77-78,176-177                  */
    double  w_prox;     /* 1     (the literal 1/2 in subproblems.jl:81,180-181 is w_prox/2)     */
    double  eps;        /* 1e-3  src/optimization/convergence.jl:2                              */
    double  mask_thr;   /* 1e-2  src/optimization/update_duals.jl:24,36                         */
    int32_t max_iters;  /* cap on admm.iteration; 0 = none (the reference has none, run.jl:2-4)  */
    int32_t n_agents_global; /* divisor of avg_U/avg_K (results.jl:108-112); 0 = G+S (one shard) */
    int32_t device;     /* HIP device ordinal; -1 = current device                              */
    int32_t flags;      /* DOPF_F_* below                                                        */
    void   *stream;     /* hipStream_t to enqueue on; NULL = a stream the context creates        */
} dopf_params;

#define DOPF_F_NO_GRAPH   1   /* launch kernels eagerly instead of through a captured hipGraph   */
#define DOPF_F_OVERLAP_AGENTS 2 /* storage kernel forked onto a side stream so it overlaps the generator
                                   kernel (default: one stream, kernels back to back — the per-kernel
                                   durations then mean the same in every tool)                        */

#define DOPF_F_NO_ROW_SKIP   8  /* generators: always sweep every row of P (no skipping of saturated rows)    */
#define DOPF_F_NO_WARM_START 4  /* storages: always the cold price-threshold scan (no warm-start kernel) */
#define DOPF_F_NO_FUSE      16  /* copper plate: generator and storage x-updates as separate launches instead
                                   of the single k_agents launch                                           */
#define DOPF_F_COMM_HOST    64  /* dopf_multi_*: sum the consensus buffers through host memory instead of RCCL — a
                                   debugging transport that lets several shards share one device (tests)      */
#define DOPF_F_KEEP_DELTAS  256  /* networks: keep every agent's injection change of the last iteration on the device, so that
                                   dopf_get_agent_slacks / dopf_get_agent_penalty work without the caller passing it in (by
                                   default it is written only for timesteps whose slack sums need the agents one by one) */
#define DOPF_F_COMM_GRAPH   512  /* contexts joined to a communicator of > 1 ranks: capture the RCCL all-reduce into the iteration
                                   hipGraphs instead of launching the chain eagerly (default: eager — the host enqueues an
                                   iteration faster than the GPU retires it, and plain launches are RCCL's best-trodden path) */
#define DOPF_F_COMM_P2P    1024  /* dopf_multi_*: the consensus sum by the peer exchange (dopf_xchg_* below) instead of RCCL.
                                   (Rehearsals that put several shards on ONE device: every shard's stream then needs a hardware
                                   queue of its own (HIP's default of four covers three shards) or a waiting exchange kernel
                                   sits in front of the peer it waits for and the wait times out. One shard per device cannot
                                   run into that.)                                                                          */
#define DOPF_F_NO_TAIL_FUSE 4096  /* one node, no lines, single-GPU chain: keep the consensus sums and the dual step as launches of
                                   their own (k_reduce, k_dual_price_small) instead of finishing the iteration inside the
                                   x-update launch (integer accumulators + the last block's tail) */
#define DOPF_F_TIME_CALLS  8192  /* measurement: dopf_iterate brackets its launches with a HIP event pair on the context's stream;
                                   dopf_last_call_ms returns the device-side span of the last call's iterations (no host launch
                                   latency in front, no status read-back behind) */
#define DOPF_F_STO_GENERAL 16384 /* storages: the general active-set body (kernels_agents.hip: sto_warm_body) also where the lean
                                  * body (sto_lean.h: copper plates; networks with many storage blocks) applies — the two are
                                  * compared by the tests */
#define DOPF_F_NO_QUIET   32768 /* networks, single-GPU chain: always launch k_slack (never the "quiet" chain, in which the dual/price
                                  * kernel forms the node sums while no line is flagged); bitwise comparisons of the two chains */
#define DOPF_F_XCHG_OWNER 65536 /* peer exchange: always the reduce-scatter + all-gather form (every chunk has an owner rank that adds the
                                  * ranks' copies), also for vectors of one chunk per rank — by default the library picks it when the
                                  * vector has more chunks than ranks */
#define DOPF_F_XCHG_ALLGATHER 131072 /* peer exchange: always the all-gather form (every rank stores its vector into every peer's area) */
#define DOPF_F_NO_TAIL_XCHG 262144 /* copper plates on a peer exchange: the exchange runs inside the one-block dual kernel of the
                                  * three-launch chain instead of inside the tail block of the one-launch iteration */
#define DOPF_F_NET_SMALL_ITEMS 524288 /* networks, one launch for all agents: cut the generators into the ~1024 items the separate
                                  * launches use instead of ~512 larger ones (same partial-sum rows on both chains: bitwise comparisons) */
#define DOPF_F_PERSIST 1048576 /* retired: accepted, has no effect; the bit is not reused */
#define DOPF_F_LONG_HORIZON 2097152 /* storages on horizons beyond T = 512 (without it dopf_create refuses them): solved by the long-horizon
                                  * body (csrc/sto_long.h: one block per storage, the horizon in tiles of 2048 timesteps, no limit on T but
                                  * device memory) on the separate-launch chain. For T <= 512 the flag changes nothing. */
#define DOPF_F_WIDE_NETWORK 8388608 /* networks beyond L = 2048 lines (without it dopf_create refuses them): the wide chain (csrc/net_wide.h:
                                  * breakpoint tables, dual and price steps and line slack sums whose LDS does not grow with N or L). Limits:
                                  * L*N and L*T below 2^31, and the tables (N*T*(6L+1) doubles + 2 N*T*L doubles of slack partials) must fit
                                  * the device's free memory, else DOPF_E_NOMEM naming the bytes. For L <= 2048 the flag changes nothing. */
#define DOPF_F_STO_INITIAL_LEVEL 33554432 /* storages start from a given level: the context keeps an initial level e0[s] per storage (all 0
                                  * until dopf_set_storage_initial_level), and every storage body solves with E_t = e0 + sum_{tau<=t} (C - D) in
                                  * [0, emax] instead of the reference's empty start (src/optimization/subproblems.jl:154: E[t] == (t == 1 ? 0 :
                                  * E[t-1]) + C[t] - D[t]; src/opf_central_reference.jl:53: E[s,0] = 0). Runs on the general active-set body (as with
                                  * DOPF_F_STO_GENERAL), the scan body and the long-horizon body; with every e0 = 0 the results are bit for bit those of
                                  * DOPF_F_STO_GENERAL. */
#define DOPF_F_STO_TERMINAL_LEVEL 67108864 /* storages end inside a given band: the context keeps a band [lo[s], hi[s]] per storage
                                  * ([0, max_level] until dopf_set_storage_terminal_level), and every storage body solves with the level after
                                  * the last timestep, E_{T-1}, in [lo, hi] instead of [0, emax] (lo == hi: an equality target; lo = hi = e0: a
                                  * cyclic horizon). Nothing else changes. Works alone (from the empty start) and with DOPF_F_STO_INITIAL_LEVEL.
                                  * Runs on the general active-set body, the scan body and the long-horizon body; with the default band the
                                  * results are those of DOPF_F_STO_GENERAL (with DOPF_F_STO_INITIAL_LEVEL: of that flag alone), bit for bit
                                  * where no storage has max_level 0 (there the last contact takes any price, so the path may differ). */
#define DOPF_F_GEN_AVAILABILITY 134217728 /* generators follow availability profiles: the context keeps K profiles f[k][t] in [0, 1] and a
                                  * profile index per generator (-1 until dopf_set_generator_availability), and every generator's box becomes
                                  * 0 <= P[g,t] <= cap[g,t] = gen_pmax[g] * f[prof[g]][t] (one fp64 multiply; gen_pmax[g] for index -1) instead of
                                  * the reference's 0 <= P <= max_generation (src/optimization/subproblems.jl:26). Nothing else changes: the same
                                  * chain runs, with generator kernels that read the profiles; with every index -1, or every profile all ones, the
                                  * results are those of the context without the flag, bit for bit. */
#define DOPF_F_STO_EFFICIENCY 268435456 /* storages lose energy on the way in and out: the context keeps a charge efficiency eta_c[s] and a
                                  * discharge efficiency eta_d[s] per storage, both in (0, 1] (all 1 until dopf_set_storage_efficiency), and every
                                  * storage body solves with E_t = E_{t-1} + eta_c C_t - D_t / eta_d instead of the reference's lossless balance
                                  * (src/optimization/subproblems.jl:150-156, src/opf_central_reference.jl:53). The objective, the boxes
                                  * 0 <= D, C <= pmax, the injection D - C and the proximal terms stay. Works alone and with
                                  * DOPF_F_STO_INITIAL_LEVEL, DOPF_F_STO_TERMINAL_LEVEL, DOPF_F_GEN_AVAILABILITY, DOPF_F_LONG_HORIZON and
                                  * DOPF_F_WIDE_NETWORK, on every chain. Runs on the general active-set body with the scan body behind it
                                  * (as with DOPF_F_STO_GENERAL) and on the long-horizon body; the lean body has no efficiencies. Wherever a level is formed from D and C — dopf_get_primal's E, dopf_set_state,
                                  * dopf_roll_horizon's new initial level — it is e0 + sum (eta_c C - D / eta_d). dopf_central_solve(_ex) ignores
                                  * the flag; dopf_central_solve_lossy takes the efficiencies. */
#define DOPF_F_LINE_RATING 536870912 /* the lines follow a rating table: the context keeps a limit rating[l + L*t] per line and timestep
                                  * (f_max[l] in every timestep until dopf_set_line_rating), and every place that read f_max[l] for timestep t
                                  * reads rating[l,t]: -rating[l,t] <= flow[l,t] <= rating[l,t] instead of the reference's one max_capacity per
                                  * line (src/optimization/subproblems.jl:77-78,176-177, src/optimization/update_duals.jl:17-39). Planned
                                  * deratings, dynamic ratings and security margins that differ between the timesteps of a window
                                  * are tables. Nothing else changes: the same chain and the same kernels run, the agents see the network
                                  * through the breakpoint tables as before. With a table whose columns all equal f_max the results are those
                                  * of the context without the flag, bit for bit, on every chain. dopf_get_agent_slacks, dopf_get_agent_penalty,
                                  * dopf_get_penalty_sums and dopf_debug_table follow the table; dopf_roll_horizon moves it like mu and rho.
                                  * dopf_central_solve, _ex and _lossy take no ratings: they solve with f_max, flag or not.
                                  * dopf_central_solve_coupled takes a table as an argument. */
#define DOPF_F_GEN_QUADRATIC_COST 1073741824 /* generators have quadratic cost curves: the context keeps a coefficient c2[g] >= 0 per generator
                                  * (all 0 until dopf_set_generator_quadratic_cost), and the cost of generator g at output P is
                                  * gen_mc[g] P + c2[g] P^2 / 2 instead of the reference's one marginal_costs per unit
                                  * (src/optimization/subproblems.jl:26-40). The generator's step around p0 = P[g,t] is the linear-cost step with
                                  * gen_mc + c2 p0 for the cost and w_prox + c2 for the proximal weight, both per row. Contexts with the flag run
                                  * their generators in a launch of their own (k_gen_update) on every shape: no pair or row-skipping kernels, no
                                  * launch shared with the storages, no one-launch iteration — the chain the same problem runs under
                                  * DOPF_F_NO_FUSE | DOPF_F_NO_TAIL_FUSE at odd T. The storages, the consensus step and every other flag work as
                                  * without it (DOPF_F_WIDE_NETWORK, DOPF_F_LONG_HORIZON, DOPF_F_GEN_AVAILABILITY, DOPF_F_LINE_RATING,
                                  * DOPF_F_KEEP_DELTAS and the storage flags included). With every c2 = 0 the results are those of the flagless
                                  * context on that chain, bit for bit. dopf_get_consensus' total_cost, and everything fed from it, is
                                  * sum gen_mc P + c2 P^2 / 2 (+ the storages' costs). dopf_central_solve, _ex and _lossy solve the LP: they
                                  * ignore the flag and the coefficients. */
#define DOPF_F_GEN_RAMP 32 /* generators have ramp limits (copper plates, L == 0): the context keeps ramp_up[g], ramp_down[g] >= 0 per
                                  * generator (+inf, no limit, until dopf_set_generator_ramp) and optionally the output p_prev[g] of the step
                                  * before the window. The generator's step keeps its objective and its box and gains
                                  * -ramp_down <= P[g,t] - P[g,t-1] <= ramp_up for t = 1 .. T-1, and for t = 0 against p_prev where one is
                                  * given: the only constraint that couples a generator's timesteps. The step is the exact Euclidean
                                  * projection of the unconstrained step's centre onto {box, ramps}, by a forward dynamic programme over the
                                  * derivative of the cost-to-go and a backward pass (k_gen_ramp): O(T x knots) for a row whose
                                  * clamped step breaks a ramp, the clamped step itself (the bits of k_gen_update) for a row that does not.
                                  * Contexts with the flag run their generators in a launch of their own, as DOPF_F_GEN_QUADRATIC_COST
                                  * contexts do (no pair or row-skipping kernels, no launch shared with the storages, no one-launch
                                  * iteration); the storages, the consensus step, DOPF_F_GEN_AVAILABILITY, DOPF_F_GEN_QUADRATIC_COST,
                                  * DOPF_F_LONG_HORIZON and the storage flags work as without it. With every ramp +inf and no p_prev the
                                  * results are those of the flagless context on that chain, bit for bit. dopf_create refuses the flag with
                                  * L > 0 (DOPF_E_UNSUPPORTED) unless DOPF_F_GEN_RAMP_NETWORK is given too, dopf_roll_horizon refuses a
                                  * context with it (the anchor's roll is the host's: build the next window's context, or use
                                  * dopf_roll_horizon_coupled, which moves the anchor on the device).
                                  * dopf_central_solve, _ex and _lossy ignore the flag. dopf_central_solve_coupled ignores it too and
                                  * takes the ramps and the anchor as arguments. Energy budgets on the same generators (copper plates):
                                  * DOPF_F2_GEN_RAMP_BUDGET, in the second flag word. */
#define DOPF_F_GEN_RAMP_NETWORK 2147483648u /* ramp limits on a network (L > 0); meaningful only together with DOPF_F_GEN_RAMP, and an
                                  * opt-in of its own because the network step needs memory that grows with the tables. A row's derivative
                                  * per step is then mc + c2 x + Psi(x - p0) + w_prox (x - p0), piecewise linear with up to 2L kinks of the
                                  * node's table, and the kinks are merged into the knots of the dynamic programme (k_gen_ramp_net,
                                  * DESIGN.md 5s). A row in flight holds at most 2T + 2 + min(2 L T, 4096) knots, in a scratch allocated at
                                  * dopf_create (DOPF_E_NOMEM, naming the bytes, where it does not fit). A row whose knots would exceed
                                  * that capacity keeps its clamped step for the iteration and is counted: dopf_iterate returns
                                  * DOPF_E_SOLVER and dopf_solver_failures() grows, as for a storage whose root search gave up. The chain
                                  * is the one a network runs under DOPF_F_NO_FUSE; DOPF_F_LINE_RATING, DOPF_F_WIDE_NETWORK,
                                  * DOPF_F_GEN_AVAILABILITY, DOPF_F_GEN_QUADRATIC_COST, DOPF_F_KEEP_DELTAS and the storage flags work as
                                  * without it; with every ramp +inf and no p_prev the results are those of the flagless context on that
                                  * chain, bit for bit. dopf_create refuses (DOPF_E_UNSUPPORTED) this flag without DOPF_F_GEN_RAMP, and
                                  * DOPF_F_GEN_RAMP alone with L > 0; with L == 0 this flag is accepted and ignored (the copper-plate
                                  * kernel runs, the same bits). dopf_roll_horizon goes on refusing every ramp context, dopf_central_solve,
                                  * _ex and _lossy ignore the flag (dopf_central_solve_coupled as well: it takes ramps as arguments, on
                                  * copper plates and networks alike). This is bit 31, the LAST bit of dopf_params.flags (an int32_t whose
                                  * size the ABI pins): the next create-time option needs a second flag word, for example in a
                                  * dopf_create2. (That word exists now: the flags2 argument of dopf_create_ex below, whose options are
                                  * named DOPF_F2_*.) */
/* ---- the second flag word: the flags2 argument of dopf_create_ex / dopf_multi_create_ex (dopf_params keeps its size). Its options are
 * named DOPF_F2_*; a bit that is none of them is DOPF_E_INVALID. */
#define DOPF_F2_GEN_ENERGY_BUDGET 1 /* generators have energy budgets over the window: the context keeps e_min[g] (0 until
                                  * dopf_set_generator_energy_budget) and e_max[g] (+inf until then). The generator's step keeps its
                                  * objective and its box (cap[g,t] under DOPF_F_GEN_AVAILABILITY, the c2 term under
                                  * DOPF_F_GEN_QUADRATIC_COST) and gains e_min[g] <= sum_t P[g,t] <= e_max[g], one timestep counting 1. With a
                                  * multiplier nu on that row the step is the one the library takes with gen_mc[g] + nu for gen_mc[g];
                                  * phi(nu) = sum_t P[g,t](nu) is continuous, piecewise linear and non-increasing, and a row whose step at
                                  * nu = 0 breaks its budget takes the step at the root of phi(nu) = the broken bound (k_gen_budget,
                                  * a wave brackets the root and narrows the bracket until phi is linear on it, then solves).
                                  * A row whose search reaches its cap of evaluations keeps its clamped step for the iteration and is
                                  * counted: dopf_iterate returns DOPF_E_SOLVER and dopf_solver_failures() grows. Contexts with the flag run
                                  * their generators in a launch of their own, the chain of DOPF_F_GEN_QUADRATIC_COST contexts (no pair or
                                  * row-skipping kernels, no launch shared with the storages, no one-launch iteration), on copper plates and
                                  * networks, DOPF_F_LONG_HORIZON and the wide chain included; with every budget at its default the results
                                  * are those of the flagless context on that chain, bit for bit. dopf_get_consensus' cost is unchanged (a
                                  * budget has no price); dopf_get_agent_slacks, dopf_get_agent_penalty and DOPF_F_KEEP_DELTAS see the
                                  * projected step. Together with DOPF_F_GEN_RAMP the flag is refused (DOPF_E_UNSUPPORTED: two constraints
                                  * that couple a row's timesteps need the ramp programme inside the multiplier search); dopf_roll_horizon
                                  * refuses a context with it (what is left of a budget after k steps is the host's arithmetic, or
                                  * dopf_roll_horizon_coupled's on the device);
                                  * dopf_central_solve, _ex and _lossy take no budgets and ignore the bit. dopf_central_solve_coupled
                                  * takes the budgets as arguments, together with ramps if the caller has both. On a copper plate
                                  * DOPF_F2_GEN_RAMP_BUDGET lifts that refusal: the pair then runs in one context. A context with this flag
                                  * and without DOPF_F2_GEN_RAMP_BUDGET also takes one budget per sub-window of the horizon
                                  * (dopf_set_generator_energy_budget_windows, k_gen_budget_win). */
#define DOPF_F2_GEN_RAMP_BUDGET 8 /* ramp limits and energy budgets on the same generators (copper plates, L == 0); meaningful only together
                                  * with DOPF_F_GEN_RAMP and DOPF_F2_GEN_ENERGY_BUDGET, and an opt-in of its own because the step needs
                                  * scratch that grows with T. The generator's step keeps its objective and its box (cap[g,t] under
                                  * DOPF_F_GEN_AVAILABILITY, the c2 term under DOPF_F_GEN_QUADRATIC_COST) and obeys the ramps, the anchor
                                  * included, and e_min[g] <= sum_t P[g,t] <= e_max[g] at once: the exact minimiser, not a sequence of two
                                  * projections. With a multiplier nu on the budget row the step is the ramp projection of the centres
                                  * c_t - nu / q; its sum is continuous, piecewise linear and non-increasing in nu, and two candidates with
                                  * the same active set bracket a stretch on which it is linear (k_gen_ramp_budget). A row
                                  * whose clamped step keeps both constraints keeps the bits of k_gen_update, one that needs only the
                                  * budget's search those of k_gen_budget, one that needs only the ramps' repair those of k_gen_ramp; the
                                  * others run the pair search, 64 candidate multipliers per round, in a scratch of
                                  * 64 x (5T + 4) + T doubles per wave and 8 waves per generator item, allocated at dopf_create
                                  * (DOPF_E_NOMEM, naming the bytes, where it does not fit). A row whose search spends its rounds keeps
                                  * its step at nu = 0 for the iteration and is counted: dopf_iterate returns DOPF_E_SOLVER and
                                  * dopf_solver_failures() grows. The chain is the one DOPF_F_GEN_RAMP contexts run. The three setters
                                  * dopf_set_generator_ramp, dopf_set_generator_energy_budget and dopf_set_generator_availability keep
                                  * their meaning, timing and status rules and also check, before anything is stored, that every row is
                                  * jointly feasible: with hi_t the pointwise-largest and lo_t the pointwise-smallest path under caps, ramps
                                  * and anchor, lo_t <= hi_t for every t, e_min <= sum_t hi_t and sum_t lo_t <= e_max (DOPF_E_INVALID,
                                  * naming g and the failing sum; the feasible paths form a lattice, so the check is exact). dopf_create
                                  * refuses (DOPF_E_UNSUPPORTED) the bit without both of the other two flags, and with L > 0 (a network
                                  * row's knots are 64 times too many for this design); with G == 0 it is accepted and ignored. The two
                                  * older flags without the bit behave as before. dopf_roll_horizon goes on refusing the context
                                  * (dopf_roll_horizon_coupled rolls it, with the joint check on the next window);
                                  * dopf_central_solve* ignore the bit. */
/* Everything else that steers kernel selection is decided from the problem's shape ("which chain runs"). The
 * library reads two environment variables, neither of which changes results: DOPF_GUARD (debug allocator) and DOPF_XCHG_TIMEOUT_MS
 * (how long an exchange kernel waits for a lost peer). Tuning knobs of the experiments (item counts, block counts, launch splits)
 * exist only in builds with -DDOPF_EXPERIMENTS. */
#define DOPF_F_DEBUG_LEAVE  2048  /* tests: the active-set storage body declares every third storage uncertified, so that the
                                   hand-over to the scan body is exercised in every kernel variant                        */
#define DOPF_F_DEBUG_ROOT_CAP 128 /* tests: the scan kernel's root search gives up after 2 iterations instead of
                                   80, so that the DOPF_E_SOLVER path can be exercised                        */
#define DOPF_F_DEBUG_LONG_STO 4194304 /* tests: the storages run on the long-horizon body at every T, also T <= 512, so that it can be
                                   compared with the one-wave bodies where those are trusted                    */
#define DOPF_F_DEBUG_WIDE_NET 16777216 /* tests: the wide chain at every L > 0, so that it can be compared with the chains of L <= 2048 */

/* Fill q with the reference's defaults (values above). */
void dopf_default_params(dopf_params *q);

int  dopf_create(dopf_ctx **out, const dopf_problem *p, const dopf_params *q);
/* dopf_create with the second flag word (DOPF_F2_*): dopf_create(out, p, q) is dopf_create_ex(out, p, q, 0). DOPF_E_INVALID, naming
 * the bit, for a bit of flags2 that is no DOPF_F2_* option. */
int dopf_create_ex(dopf_ctx **out, const dopf_problem *p, const dopf_params *q, int32_t flags2);
void dopf_destroy(dopf_ctx *ctx);
/* Message of the last error on ctx; with ctx == NULL the last dopf_create error (thread-local). */
const char *dopf_last_error(const dopf_ctx *ctx);

/* Run up to n_iters ADMM iterations back to back on the device, one host sync at the end.
 * Stops exactly like check_convergence!: no test at iteration 1; on the converging step the
 * iteration counter is NOT bumped and later iterations in the same call are no-ops.
 * iters_done = iterations actually computed in this call; converged = Convergence.all.
 * Returns DOPF_E_SOLVER (outputs are still set, the state is still advanced) when a storage
 * sub-problem's root search hit its iteration cap since the last report: that row is not the
 * minimiser of its QP (the reference would surface a Gurobi failure from value.() at this point,
 * src/optimization/subproblems.jl:189-206). dopf_sync reports the same.
 * On a context joined to a communicator (dopf_comm_init / dopf_multi_create) every iteration
 * includes the all-reduce of the consensus buffer; all ranks must call with the same n_iters. */
int dopf_iterate(dopf_ctx *ctx, int32_t n_iters, int32_t *iters_done, int32_t *converged);

/* Sharded form of one iteration (one process per GPU):
 *   dopf_local_update     x-update of the local agents + local sums -> consensus buffer
 *   <all-reduce(sum) of the consensus buffer across ranks, done by the caller>
 *   dopf_apply_consensus  avg_U/avg_K, flows, dual update, residuals, convergence test
 * Both enqueue on the context's stream and return without synchronising. */
int dopf_local_update(dopf_ctx *ctx);
int dopf_apply_consensus(dopf_ctx *ctx);
/* Number of doubles in the consensus buffer: N*T injections | L*T sum U | L*T sum K | 1 cost. */
int64_t dopf_consensus_size(const dopf_ctx *ctx);
/* Device address of the context's own consensus buffer (for RCCL / a zero-copy tensor view). */
void *dopf_consensus_ptr(dopf_ctx *ctx);
/* Use caller-owned DEVICE memory (>= dopf_consensus_size doubles) as the consensus buffer,
 * e.g. the data_ptr of a torch tensor handed to torch.distributed.all_reduce. */
int dopf_bind_consensus(dopf_ctx *ctx, void *device_ptr);
/* Host sync of the context's stream + status read-back (iteration, converged). */
int dopf_sync(dopf_ctx *ctx, int32_t *iteration, int32_t *converged);

int dopf_get_duals(dopf_ctx *ctx, double *lambda /*T*/, double *mu /*L*T*/, double *rho /*L*T*/);
int dopf_get_duals_used(dopf_ctx *ctx, double *lambda, double *mu, double *rho);
int dopf_get_primal(dopf_ctx *ctx, double *P /*T*G*/, double *D, double *C, double *E /*T*S*/);
int dopf_get_consensus(dopf_ctx *ctx, double *injection /*N*T*/, double *avg_U, double *avg_K,
                       double *line_util /*L*T each*/, double *total_cost /*1*/);
int dopf_get_residuals(dopf_ctx *ctx, double *lam_res, double *mu_res, double *rho_res,
                       int32_t *iteration);
/* Convergence.{lambda_res, mue_res, rho_res}[end] as vectors (src/structures/convergence.jl:5-12):
 * |dual after the last update - dual the last solve used| per entry; any pointer may be NULL. */
int dopf_get_residual_vectors(dopf_ctx *ctx, double *lam_res /*T*/, double *mu_res /*L*T*/, double *rho_res /*L*T*/);
/* ResultGenerator/ResultStorage.{U, K} of the last solve (src/structures/results.jl:1-17), L x T each,
 * [l + L*t]; agent = caller's index, generators 0..G-1 then storages G..G+S-1 (of this context's shard).
 * The device eliminates the slacks in closed form; they are recomputed here from the agent's injection
 * change and the consensus state that solve read. Needs DOPF_F_KEEP_DELTAS. */
int dopf_get_agent_slacks(dopf_ctx *ctx, int32_t agent, double *U, double *K);
/* PenaltyTerm of the agent (src/structures/penalty_terms.jl:1-5, src/optimization/penalty_terms.jl:3-37):
 * penalty[0..T) energy_balance, [T..2T) upper_flow, [2T..3T) lower_flow — the diagnostics print_results shows
 * with print_penalty=true. delta = the agent's injection change of the last iteration (T values), or NULL to
 * use the device's copy, which exists only with lines and DOPF_F_KEEP_DELTAS (DOPF_E_UNSUPPORTED otherwise). */
int dopf_get_agent_penalty(dopf_ctx *ctx, int32_t agent, const double *delta, double *penalty /*3*T*/);
/* Result.penalty_term of the last result (src/structures/results.jl:66-70: `sum_up` of src/helpers/penalty_terms.jl:1-6 over
 * every unit's PenaltyTerm): penalty[0..T) energy_balance, [T..2T) upper_flow, [2T..3T) lower_flow, each the SUM over all
 * agents of this context of what dopf_get_agent_penalty returns for one — one pass on the device instead of one call per
 * agent. Needs lines and DOPF_F_KEEP_DELTAS (the injection changes of the last x-update must be on the device);
 * DOPF_E_UNSUPPORTED otherwise. */
int dopf_get_penalty_sums(dopf_ctx *ctx, double *penalty /*3*T*/);
/* which = 0: duals used by the last solve (what the reference's driver script evaluates),
 * which = 1: duals after the last update. out is N x T, [n + N*t]. */
int dopf_get_nodal_price(dopf_ctx *ctx, int32_t which, double *out);

/* ResultNode.{generation, discharge, charge} of the last result (src/structures/results.jl:19-35, filled by `update`,
 * src/helpers/network_elements.jl:1-14, in the agent loop of Result(...), results.jl:72-106): per node and timestep the
 * sums of its generators' output and of its storages' discharge and charge, layout [n + N*t] like the injection (which
 * is generation + discharge - charge - demand). Any pointer may be NULL. Result.{generation, discharge, charge}
 * (results.jl:37-47) are these summed over the nodes. Computed on request from the primal arrays (not on the hot path). */
int dopf_get_node_results(dopf_ctx *ctx, double *generation /*N*T*/, double *discharge /*N*T*/, double *charge /*N*T*/);
/* Any of P, D, C, avg_U, avg_K, lambda, mu, rho may be NULL (= keep). iteration >= 1 is the
 * value admm.iteration would have before the next solve; iteration == 1 means "no result yet"
 * only if all primal pointers are NULL and the state is untouched. */
int dopf_set_state(dopf_ctx *ctx, const double *P, const double *D, const double *C,
                   const double *avg_U, const double *avg_K,
                   const double *lambda, const double *mu, const double *rho, int32_t iteration);

/* Diagnostics: number of storage sub-problems whose inner root search hit its iteration cap
 * since creation (0 in every healthy run), and a version string. */
/* Measurement: n_iters iterations launched kernel by kernel (no graph) with a hipEvent pair around
 * every kernel on the stream it runs on; one host sync at the end. Average milliseconds per launch. */
typedef struct dopf_timing {
    double tables_ms, gen_ms, sto_ms, slack_ms, reduce_ms, dual_ms;  /* per-kernel averages; with agents_fused
                                                                        gen_ms is the ONE x-update launch
                                                                        (k_agents) and sto_ms an empty pair */
    double iter_ms;                                                  /* whole iteration, event to event */
    double empty_ms;    /* an event pair with nothing between: the fixed cost inside every number above */
    int32_t iters;
    int32_t agents_fused;   /* 1: generators and storages ran as one launch */
    int32_t tail_fused;     /* 1: consensus sums, dual step and stop test ran inside the x-update launch(es): reduce_ms and
                               dual_ms are empty event pairs */
    int32_t slack_in_dual;  /* 1 (networks): node sums left from k_slack, slack sums were formed by the dual/price kernel:
                               reduce_ms is an empty event pair */
    int32_t quiet;          /* 1 (networks): no line was flagged, k_slack was not launched (slack_ms is an empty event pair): the dual/price
                               kernel formed the node sums too */
    int32_t sto_lean;       /* 1: the storages of this problem are solved by the lean active-set body (csrc/sto_lean.h) */
    int32_t persist;        /* always 0 (DOPF_F_PERSIST is retired; the field keeps the layout) */
    int32_t sto_long;       /* 1: the storages ran on the long-horizon body (csrc/sto_long.h: DOPF_F_LONG_HORIZON, DOPF_F_DEBUG_LONG_STO) */
} dopf_timing;
int dopf_iterate_timed(dopf_ctx *ctx, int32_t n_iters, dopf_timing *out);
/* *out = 1 when the context runs the wide chain (DOPF_F_WIDE_NETWORK beyond L = 2048, DOPF_F_DEBUG_WIDE_NET), else 0. (A query of
 * its own rather than a field of dopf_timing: callers built against the header of an earlier release allocate that struct.) */
int dopf_wide_net(const dopf_ctx *ctx, int32_t *out);
/* DOPF_F_TIME_CALLS: milliseconds between the first launch of the last dopf_iterate call and the end of its last one, on the
 * device (-1 without the flag, or when the call ended early on a stop). */
double dopf_last_call_ms(const dopf_ctx *ctx);

int64_t dopf_solver_failures(dopf_ctx *ctx);

/* DOPF_F_STO_INITIAL_LEVEL: the level of each storage before the first timestep, e0[S] in the caller's order of this context's
 * storages (NULL = all 0), 0 <= e0[s] <= max_level[s]. The reference pins it to 0 (src/optimization/subproblems.jl:154,
 * src/opf_central_reference.jl:53); a receding-horizon caller hands the next window the level the last one reached. May be called
 * between any two calls that iterate; takes effect at the next x-update. The values are copied before the call returns, in order
 * on the context's stream (the captured iteration graphs read the same device array and stay valid). dopf_get_primal's E and
 * dopf_set_state's levels start from it. DOPF_E_UNSUPPORTED without the flag; DOPF_E_INVALID for a NaN, a negative value or one
 * above max_level (the stored levels are then unchanged). */
int dopf_set_storage_initial_level(dopf_ctx *ctx, const double *e0);

/* DOPF_F_STO_TERMINAL_LEVEL: the band of each storage's level after the last timestep, lo[S] and hi[S] in the caller's order of this
 * context's storages (both NULL = the default band [0, max_level], the reference's). Timing and copies as for
 * dopf_set_storage_initial_level. DOPF_E_UNSUPPORTED without the flag; DOPF_E_INVALID, and nothing stored, for a NaN, lo < 0,
 * hi > max_level, lo > hi, only one of the arrays NULL, or a band that the storage cannot reach from its initial level e0 in T steps of
 * at most pmax: the reachable end levels are [max(0, e0 - T pmax), min(max_level, e0 + T pmax)]. In contexts with both flags
 * dopf_set_storage_initial_level refuses (DOPF_E_INVALID) an e0 from which the stored band is unreachable. */
int dopf_set_storage_terminal_level(dopf_ctx *ctx, const double *lo, const double *hi);

/* DOPF_F_STO_EFFICIENCY: the storages' charge and discharge efficiencies, eta_c[S] and eta_d[S] in the caller's order of this
 * context's storages, every value in (0, 1] (both NULL = all 1, the reference's lossless storage; all 1 until the first call). The
 * level then follows E_t = E_{t-1} + eta_c C_t - D_t / eta_d, E_{-1} = e0, 0 <= E_t <= max_level (E_{T-1} in the terminal band). Timing
 * and copies as for dopf_set_storage_initial_level. DOPF_E_UNSUPPORTED without the flag; DOPF_E_INVALID, naming the entry and storing
 * nothing, for a NaN, a value <= 0 or > 1, only one of the arrays NULL, or (contexts with DOPF_F_STO_TERMINAL_LEVEL) efficiencies
 * under which the stored band is unreachable from the stored e0: the reachable end levels are
 * [max(0, e0 - T pmax / eta_d), min(max_level, e0 + T eta_c pmax)]. In contexts with this flag dopf_set_storage_initial_level and
 * dopf_set_storage_terminal_level check reachability over that range. */
int dopf_set_storage_efficiency(dopf_ctx *ctx, const double *eta_c, const double *eta_d);

/* DOPF_F_GEN_AVAILABILITY: the generators' availability. profiles: T x n_profiles, [t + T*k] (agent-major like P), every value in
 * [0, 1]; profile_of: G in the caller's order of this context's generators, -1 = always gen_pmax, else a profile in [0, n_profiles).
 * n_profiles == 0 with both NULL resets every generator to -1. Many generators may share a profile (one solar shape per region): the
 * kernels read the table per (row, timestep), and a small one stays in L2. Timing and copies as for dopf_set_storage_initial_level;
 * a table larger than any before is allocated anew, and the iteration graphs are then captured again at the next dopf_iterate.
 * dopf_set_state may hand in P above a cap: the next x-update clamps it. DOPF_E_UNSUPPORTED without the flag; DOPF_E_INVALID, naming
 * the entry and storing nothing, for a NaN, a value outside [0, 1], an index outside [-1, n_profiles), n_profiles < 0, or a NULL
 * array with n_profiles > 0. */
int dopf_set_generator_availability(dopf_ctx *ctx, int32_t n_profiles, const double *profiles, const int32_t *profile_of);

/* DOPF_F_LINE_RATING: the lines' limits per timestep, rating[l + L*t] (L x T, the layout of mu), every value finite and >= 0; NULL =
 * f_max[l] of dopf_create in every timestep (also the table until the first call). May be called between any two calls that iterate,
 * on every single-GPU chain (the wide chain included) and on contexts joined to a communicator or a peer exchange: the table is
 * replicated state and the call moves no sums, so the rule is dopf_iterate's — every rank calls it with the same table between the
 * same two iterations (a consensus buffer bound with dopf_bind_consensus must still hold the last summed vector). The values are
 * copied before the call returns, in order on the context's stream, into the device array the captured iteration graphs read: the
 * graphs stay valid. Then the state derived from the limits — the per-line flags that choose between the closed-form and the
 * agent-by-agent slack sums, and the breakpoint tables of the settled timesteps — is formed again under the new table, before the
 * next x-update. P, D, C, the duals, injections, flows, avg_U / avg_K and the iteration counter are kept; converged becomes 0, halt is
 * formed again from max_iters and the residual maxima are cleared, as dopf_set_demand does. A rating of 0 pins the flow of that line
 * and timestep to 0 (as far as the penalty enforces any limit); it does NOT take the line out of the PTDF — an outage that reroutes
 * flows is a new dopf_problem. DOPF_E_UNSUPPORTED without the flag; DOPF_E_INVALID, naming l and t and storing nothing, for a NaN, an
 * Inf or a negative entry. With L == 0 the call returns DOPF_OK and does nothing. */
int dopf_set_line_rating(dopf_ctx *ctx, const double *rating /* L x T, [l + L*t]; NULL = f_max in every timestep */);

/* DOPF_F_GEN_QUADRATIC_COST: the generators' quadratic cost coefficients, c2[G] in the caller's order of this context's generators,
 * every value finite and >= 0; NULL = all 0 (also the value until the first call). The cost of generator g at output P becomes
 * gen_mc[g] P + c2[g] P^2 / 2. Timing and copies as for dopf_set_storage_initial_level: callable between any two calls that iterate,
 * the values are copied before the call returns, in order on the context's stream, into the device array the captured iteration
 * graphs read (the graphs stay valid), and take effect at the next x-update. Status as for dopf_set_line_rating: P, D, C, the duals
 * and the iteration counter are kept; converged becomes 0, halt is formed again from max_iters and the residual maxima are cleared.
 * The coefficients have no time axis: dopf_roll_horizon and dopf_set_state leave them alone. Contexts joined to a communicator or a
 * peer exchange need nothing else (the cost is local to the rank's agents). DOPF_E_UNSUPPORTED without the flag; DOPF_E_INVALID,
 * naming the entry and storing nothing, for a NaN, an Inf or a negative entry. With G == 0 the call returns DOPF_OK and does nothing. */
int dopf_set_generator_quadratic_cost(dopf_ctx *ctx, const double *c2 /* G; NULL = all 0 */);

/* DOPF_F_GEN_RAMP: the generators' ramp limits, ramp_up[G] and ramp_down[G] in the caller's order of this context's generators, every
 * value >= 0 (0: constant output; +inf: no limit), both NULL or both given; both NULL = all +inf (also the value until the first
 * call). p_prev[G] (optional; NULL = no anchor): the output of the step before the window, in [0, gen_pmax[g]]; the first step then
 * obeys the ramps against it. Timing, copies and status as for dopf_set_generator_quadratic_cost: callable between any two calls that
 * iterate, the values are copied before the call returns, in order on the context's stream, into the device arrays the captured
 * iteration graphs read (the graphs stay valid), and take effect at the next x-update; P, D, C, the duals and the iteration counter
 * are kept, converged becomes 0. A P that breaks a ramp (dopf_set_state) is only the proximal centre: the next x-update projects.
 * Contexts joined to a communicator or a peer exchange need nothing else (the constraint is local to the rank's agents).
 * DOPF_E_UNSUPPORTED without the flag; DOPF_E_INVALID, naming the entry and storing nothing, for a NaN, a negative ramp, only one of
 * the two ramp arrays, a p_prev outside [0, gen_pmax], or an anchored generator g that cannot stay under its caps: with
 * lo_0 = max(0, p_prev - ramp_down), lo_t = max(0, lo_{t-1} - ramp_down), some lo_t > cap[g,t] (the message names g and t). In
 * contexts with this flag dopf_set_generator_availability repeats that check under its new table. With G == 0 the call returns
 * DOPF_OK and does nothing. */
int dopf_set_generator_ramp(dopf_ctx *ctx, const double *ramp_up /* G; NULL = +inf */, const double *ramp_down /* G; NULL = +inf */,
                            const double *p_prev /* G; NULL = no anchor */);

/* Minimum output (must-run floors): p_min[G] in the caller's order of this context's generators, 0 <= p_min[g] <=
 * gen_pmax[g], finite; NULL = all 0 (also the value until the first call). The box of row g at timestep t becomes
 *     floor[g,t] <= P[g,t] <= cap[g,t],   floor[g,t] = fmin(p_min[g], cap[g,t])
 * with cap[g,t] = gen_pmax[g], or gen_pmax[g] * f[prof[g]][t] under DOPF_F_GEN_AVAILABILITY: the floor follows an outage down (cap = 0
 * gives floor = 0), and p_min = gen_pmax means "must take whatever is available". The objective, the ramps, the anchor, the c2 term,
 * the injections and the consensus step stay as they are; p_min has no time axis. There is no create-time flag of its own: minimum
 * output runs on the ramp kernels, so the context needs DOPF_F_GEN_RAMP (on a network DOPF_F_GEN_RAMP_NETWORK too); the ramps stay
 * +inf until dopf_set_generator_ramp, so a must-take unit is a ramp context with infinite ramps. The library does NOT check that the
 * floors of a node or a plate fit under the demand: an over-committed system does not converge, exactly as an under-supplied one does
 * not. Timing, copies and status as for dopf_set_generator_ramp: callable between any two calls that iterate, the values are copied
 * before the call returns, in order on the context's stream, into a device array the kernels read, and take effect at the next
 * x-update; P, D, C, the duals and the iteration counter are kept, converged becomes 0, halt is formed again from max_iters and the
 * residual maxima are cleared. A P below its floor (dopf_set_state) is only the proximal centre: the next x-update clamps it. The
 * first call with an array switches the context to the floor instantiations of its generator kernel, a NULL call switches back; either
 * switch drops the captured iteration graphs, which are captured again at the next dopf_iterate (the rule of a grown availability
 * table); between two arrays the graphs stay valid. dopf_roll_horizon_coupled leaves p_min alone; dopf_central_solve* ignore it.
 * DOPF_E_UNSUPPORTED without DOPF_F_GEN_RAMP, and on a context with DOPF_F2_GEN_ENERGY_BUDGET (the pair DOPF_F2_GEN_RAMP_BUDGET
 * included: floors inside the multiplier search are not built). DOPF_E_INVALID, naming the entry and storing nothing, for a NaN, an
 * Inf, a negative value, a value above gen_pmax, or a row g without a path: with the forward intervals
 *     F_0 = [max(floor_0, p_prev - ramp_down), min(cap_0, p_prev + ramp_up)]   ([floor_0, cap_0] without an anchor),
 *     F_t = [max(floor_t, lo_{t-1} - ramp_down), min(cap_t, hi_{t-1} + ramp_up)]
 * the first t with lo_t > hi_t is refused (the message names g, t and both ends). The check is exact — a point of F_{T-1} traces back
 * through the intervals — and at p_min = 0 it is dopf_set_generator_ramp's. dopf_set_generator_ramp, dopf_set_generator_availability
 * and dopf_roll_horizon_coupled repeat it for every row with a stored p_min > 0 under their new ramps, anchor or table, before
 * anything is overwritten. With G == 0 the call returns DOPF_OK and does nothing. */
int dopf_set_generator_min_output(dopf_ctx *ctx, const double *p_min /* G; NULL = all 0 */);
/* The stored floors, G values in the caller's order, from the context's host copy: no device call, callable at any time. Zeros on a
 * context without DOPF_F_GEN_RAMP. */
int dopf_get_generator_min_output(dopf_ctx *ctx, double *p_min /* G */);

/* DOPF_F2_GEN_ENERGY_BUDGET: the generators' energy budgets over the window, e_min[G] and e_max[G] in the caller's order of this
 * context's generators: e_min[g] <= sum_t P[g,t] <= e_max[g]. Either array may be NULL on its own (e_min: all 0, e_max: all +inf, also
 * the values until the first call). Timing, copies and status as for dopf_set_generator_ramp: callable between any two calls that
 * iterate, the values are copied before the call returns, in order on the context's stream, into the device arrays the captured
 * iteration graphs read (the graphs stay valid), and take effect at the next x-update; P, D, C, the duals and the iteration counter
 * are kept, converged becomes 0. Contexts joined to a communicator or a peer exchange need nothing else (the constraint is local to
 * the rank's agents). DOPF_E_UNSUPPORTED without the flag; DOPF_E_INVALID, naming the entry and storing nothing, for a NaN,
 * e_min < 0, an infinite e_min, e_max < 0, e_min > e_max, or e_min[g] > sum_t cap[g,t] (the stored availability table). In contexts
 * with this flag dopf_set_generator_availability repeats the last check under its new table. With G == 0 the call returns DOPF_OK
 * and does nothing. While dopf_set_generator_energy_budget_windows holds a table a call with an array is DOPF_E_INVALID (one
 * description of the budgets at a time); (NULL, NULL) stays allowed. */
int dopf_set_generator_energy_budget(dopf_ctx *ctx, const double *e_min /* G; NULL = 0 */, const double *e_max /* G; NULL = +inf */);
/* The budget prices (water values) of the decentral run: nu[g] is the multiplier the last computed x-update put on
 * generator g's budget row e_min[g] <= sum_t P[g,t] <= e_max[g] — the number the generator kernels add to gen_mc[g] to form the
 * row, in the unit of gen_mc (cost per unit of energy). Sign convention: nu[g] > 0 where e_max held the row down, nu[g] < 0 where
 * e_min pushed it up, and nu[g] = 0 for a row with default budgets, for a row whose step at nu = 0 kept its budget, and for a row
 * whose search gave up (that row keeps its step at nu = 0 and counts in dopf_solver_failures). At a fixed point of the iteration
 * the proximal and consensus terms vanish and the row's optimality system is the central LP's, so at convergence
 * nu[g] = -budget_dual[g] of dopf_central_solve_coupled wherever the LP's dual is unique. G values in the caller's generator
 * order. The call synchronises the context's stream and copies G doubles; it works while a trace is active, as the other getters
 * do, and on contexts joined to a communicator or a peer exchange (the price is local to the rank's agents). Before the first
 * iteration the values are zeros. Recording is opt-in on a context without DOPF_F2_GEN_RAMP_BUDGET: storing the prices costs its
 * generator kernel time, so such a context records nothing until the FIRST call of this entry, which switches it
 * to the price-storing instantiations of that kernel — other kernels, so the captured iteration graphs are dropped and captured
 * again at the next dopf_iterate, the rule of the first dopf_set_generator_min_output — and returns what is stored: zeros. From the
 * next computed x-update on every call returns that x-update's prices; there is no way back. A caller who wants prices calls the
 * entry once after dopf_create_ex (dopf_multi: every shard is switched by dopf_multi_get_generator_budget_price); one who never
 * calls it runs the kernels of before. A DOPF_F2_GEN_RAMP_BUDGET context records from its first iteration on, nothing is switched.
 * The values are "of the last x-update": dopf_set_generator_energy_budget, dopf_set_state,
 * dopf_set_demand, dopf_roll_horizon_coupled and the other setters leave them alone (after a roll they still describe the window
 * before it), and so does a dopf_iterate on a halted context, whose launches compute nothing. The trace (dopf_trace_*) does not
 * record the budget prices, and the multipliers of the ramp rows are not returned (on a DOPF_F2_GEN_RAMP_BUDGET context nu is the
 * budget row's multiplier alone). DOPF_E_UNSUPPORTED without DOPF_F2_GEN_ENERGY_BUDGET; DOPF_E_INVALID for a NULL pointer with
 * G > 0; with G == 0 the call returns DOPF_OK and does nothing. While dopf_set_generator_energy_budget_windows holds a table the
 * entry returns DOPF_E_INVALID: the prices are per window then, dopf_get_generator_budget_window_price. */
int dopf_get_generator_budget_price(dopf_ctx *ctx, double *nu /* G */);
/* Energy budgets per sub-window of the horizon, on a context created with DOPF_F2_GEN_ENERGY_BUDGET and without
 * DOPF_F2_GEN_RAMP_BUDGET: copper plates, networks, the wide chain and DOPF_F_LONG_HORIZON (no flag of its own). Window j of n_win
 * covers the timesteps win_end[j-1] <= t < win_end[j] with win_end[-1] = 0; the ends are strictly increasing, the last one is T and
 * 1 <= n_win <= T. The table of ends is shared by all generators; the budgets are per generator and window, [j + n_win*g] in the
 * caller's generator order (e_min NULL: all 0, e_max NULL: all +inf). While a table is set every generator's x-update keeps its
 * objective and its box and obeys e_min[g,j] <= sum_{t in window j} P[g,t] <= e_max[g,j] for every j: the windows are disjoint, so
 * the row separates into n_win problems of dopf_set_generator_energy_budget's kind, one multiplier each, and the step is the exact
 * minimiser (k_gen_budget_win: a wave per (row, window)). One window with end T is dopf_set_generator_energy_budget, bit for bit.
 * The first call with n_win >= 1 switches the context to that kernel and allocates device arrays of the context's own (the ends,
 * the two tables and n_win x G prices, zeroed; DOPF_E_NOMEM, naming the bytes, where they do not fit). A call with another n_win
 * than the stored one synchronises the stream, reallocates and drops the captured graphs; one with the same n_win copies, in order
 * on the context's stream, into the arrays the graphs read (the graphs stay valid). n_win == 0 with all pointers NULL removes the
 * table: the context is back on k_gen_budget and the graphs are dropped. Status as for dopf_set_generator_energy_budget: P, D, C,
 * the duals and the iteration counter are kept, converged becomes 0. One description of the budgets at a time: the entry returns
 * DOPF_E_INVALID while a non-default whole-horizon budget is stored (call dopf_set_generator_energy_budget(ctx, NULL, NULL)
 * first), and while a table is set dopf_set_generator_energy_budget with an array and dopf_get_generator_budget_price return
 * DOPF_E_INVALID and dopf_roll_horizon_coupled DOPF_E_UNSUPPORTED. Every refusal names the entry, g and j and stores nothing:
 * DOPF_E_UNSUPPORTED without the flag and on a DOPF_F2_GEN_RAMP_BUDGET context (ramps couple neighbouring windows: the rows no
 * longer separate); DOPF_E_INVALID for n_win < 0 or > T, a NULL win_end with n_win > 0, pointers with n_win == 0, ends that are
 * not strictly increasing or do not end at T, a NaN, a negative or infinite e_min, e_max < 0, e_min > e_max, and
 * e_min[g,j] > sum_{t in window j} cap[g,t] (the sum formed in t order under the stored availability table;
 * dopf_set_generator_availability repeats that check window by window under its new table). With G == 0 the call returns DOPF_OK
 * and does nothing. */
int dopf_set_generator_energy_budget_windows(dopf_ctx *ctx, int32_t n_win, const int32_t *win_end /* n_win */,
                                             const double *e_min /* n_win x G, [j + n_win*g]; NULL = all 0 */,
                                             const double *e_max /* n_win x G, [j + n_win*g]; NULL = all +inf */);
/* The stored table from the context's host copies (no device call); any pointer may be NULL. *n_win is 0 while no table is set, and
 * nothing else is written then. win_end needs room for T values, e_min and e_max for n_win x G. */
int dopf_get_generator_energy_budget_windows(dopf_ctx *ctx, int32_t *n_win, int32_t *win_end /* room for T */, double *e_min,
                                             double *e_max);
/* The window prices: nu[j + n_win*g] is the multiplier the last computed x-update put on window j's row of generator g, with the
 * sign convention of dopf_get_generator_budget_price: 0 for a free window, for one whose clamped step keeps its budget and for one
 * whose search gave up. k_gen_budget_win always stores them (no opt-in); before the first iteration after a set the values are what
 * is stored, zeros after an allocation. At convergence nu[g,j] is minus the central LP's dual of that row wherever it is unique.
 * Works while a trace is active; the trace does not record the prices. DOPF_E_INVALID while no table is set and for a NULL
 * pointer; with G == 0 the call returns DOPF_OK and does nothing. */
int dopf_get_generator_budget_window_price(dopf_ctx *ctx, double *nu /* n_win x G, [j + n_win*g] */);
/* Must-run floors on a budget context: on a context created with DOPF_F2_GEN_ENERGY_BUDGET and without DOPF_F_GEN_RAMP
 * — copper plates, networks, the wide chain and DOPF_F_LONG_HORIZON, with or without a table of budgets per sub-window — every row's
 * box becomes floor[g,t] <= P[g,t] <= cap[g,t] with floor[g,t] = min(p_min[g], cap[g,t]) and cap[g,t] = gen_pmax[g] (times the
 * availability factor under DOPF_F_GEN_AVAILABILITY): the rules of dopf_set_generator_min_output — the floor follows an outage down,
 * p_min = gen_pmax means must-take. The floor holds for every row of the context, rows with default budgets and free windows
 * included; the objective, the budget rows e_min <= sum P <= e_max (whole-horizon or per window) and the consensus step are
 * untouched, and the multiplier search of the budget kernels runs with [floor, cap] for [0, cap] (the MN instantiations of
 * k_gen_budget and k_gen_budget_win). dopf_get_generator_budget_price and dopf_get_generator_budget_window_price keep their
 * definitions and sign rule: nu is the multiplier of the row whose box has the floor as its lower end, at convergence minus the dual
 * of the central LP with the same floors wherever that is unique. p_min in the caller's generator order; NULL: all 0.
 * Callable between any two calls that iterate; the values are copied in order on the context's stream and take effect at the next
 * x-update; P, D, C, the duals and the iteration counter are kept (a P below its floor handed in by dopf_set_state is only the
 * proximal centre), converged becomes 0 and the residual maxima are cleared. The floors live in a device array of the context's
 * own, allocated and zeroed at the first call with an array (DOPF_E_NOMEM, naming the bytes, where it does not fit). The first call
 * with an array switches the context to the floor instantiations and drops the captured graphs, a NULL call switches back (and
 * drops them); between two arrays the graphs stay valid. Every refusal names this entry and stores nothing: DOPF_E_UNSUPPORTED
 * without DOPF_F2_GEN_ENERGY_BUDGET and on any DOPF_F_GEN_RAMP context (plain ramp contexts have dopf_set_generator_min_output; the
 * pair DOPF_F2_GEN_RAMP_BUDGET has no floors); DOPF_E_INVALID, naming g (and j), for a NaN, an infinite or negative value,
 * p_min[g] > gen_pmax[g], and a row that cannot stay under its maximum: sum_t floor[g,t] > e_max[g], or the same over a window of the
 * stored table (sums formed in t order under the stored availability table; with e_min <= sum cap, which the budget setters check,
 * the test is exact). dopf_set_generator_energy_budget, dopf_set_generator_energy_budget_windows, dopf_set_generator_availability
 * and dopf_roll_horizon_coupled repeat that test for every row with a stored floor > 0 under their new values before they overwrite
 * anything (the roll leaves p_min alone); their messages name the calling entry. With G == 0 the call returns DOPF_OK. */
int dopf_set_generator_budget_min_output(dopf_ctx *ctx, const double *p_min /* G; NULL = all 0 */);
/* The stored floors of dopf_set_generator_budget_min_output from the context's host copy (no device call); zeros while none are set */
int dopf_get_generator_budget_min_output(dopf_ctx *ctx, double *p_min /* G */);
/* The ramp prices of the decentral run: rp[t + T*g] is the multiplier the last computed x-update put on generator
 * g's ramp row -ramp_down <= P[g,t] - P[g,t-1] <= ramp_up between t-1 and t (t = 0: the anchor's row against p_prev, 0 without an
 * anchor) — what one more unit per step of flexibility of unit g is worth at step t, in the unit of gen_mc, in the caller's
 * generator order. Sign convention: rp > 0 where ramp-up held the unit back, rp < 0 where ramp-down held it up; rp = 0 for a row
 * whose clamped step kept its ramps and for a row whose pair search gave up (dopf_solver_failures). Where a row's multipliers are
 * not unique (a step on a box end and a ramp reach at once) the vector nearest 0, step by step from the horizon's end, is returned.
 * The values are read off the stored row and its centres (csrc/ramp_price.h), not off the programme that repaired it. At a fixed
 * point of the iteration the proximal and consensus terms vanish and the row's optimality system is the central LP's, so at
 * convergence rp = -ramp_dual of dopf_central_solve_coupled wherever the LP's dual is unique: the sign rule of the budget price. On
 * a DOPF_F2_GEN_RAMP_BUDGET context it is the ramp rows' multiplier under that row's nu (dopf_get_generator_budget_price). The
 * floors of dopf_set_generator_min_output are the lower ends of the boxes the values are formed with.
 * Recording is opt-in: the FIRST call of this entry allocates T*G doubles of the context's own on the device and zeroes them
 * (DOPF_E_NOMEM, naming the bytes, where they do not fit), switches the context to the price-recording instantiations of its
 * generator kernel — other kernels, so the call synchronises the context's stream and the captured iteration graphs are dropped and
 * captured again at the next dopf_iterate, the rule of the first dopf_set_generator_min_output — and returns what is stored: zeros.
 * From the next computed x-update on every call returns that x-update's prices; there is no way back, and a floor set afterwards
 * keeps the context recording. A context that never calls the entry runs the kernels of before (dopf_multi: every shard is
 * switched by dopf_multi_get_generator_ramp_price). The values are "of the last x-update": dopf_set_generator_ramp,
 * dopf_set_generator_min_output, dopf_set_state, dopf_set_demand, dopf_roll_horizon_coupled and the other setters leave them alone
 * (after a roll they still describe the window before it), and so does a dopf_iterate on a halted context, whose launches compute
 * nothing. Before the first iteration the values are zeros. The call copies T*G doubles; it works while a trace is active (the
 * trace does not record the ramp prices) and on contexts joined to a communicator or a peer exchange (the price is local to the
 * rank's rows). DOPF_E_UNSUPPORTED without DOPF_F_GEN_RAMP, and with L > 0: network rows are not priced (k_gen_ramp_net keeps no
 * centre, and a row's gradient there needs the node's table). DOPF_E_INVALID for a NULL pointer with G > 0; with G == 0 the call
 * returns DOPF_OK and does nothing. */
int dopf_get_generator_ramp_price(dopf_ctx *ctx, double *rp /* T*G, [t + T*g] */);

/* ---- a receding horizon: the window's demand and the window itself change in place -------------------------------
 * Replace nothing in the reference, which builds a new ADMM(...) per window (src/structures/admm.jl:23-62). Both need no flag, work
 * on every single-GPU chain, keep the captured iteration graphs valid (they write the arrays the graphs read) and return after
 * their work on the context's stream is done. Both are DOPF_E_UNSUPPORTED on a context joined to a communicator or a peer exchange
 * (the shards' node sums would need an exchange); there are no dopf_multi_* wrappers.
 *
 * dopf_set_demand: the context's demand, N x T, [n + N*t], replaced in the same device array. P, D, C, the duals, avg_U / avg_K and
 * the inputs of the setters above are unchanged; injection, imbalance, flows, prices and the consensus buffer are derived again
 * from the agents' node sums (formed from P, D, C in parallel) and the new demand. converged becomes 0, halt is formed again from
 * max_iters, the residual maxima are cleared as dopf_set_state clears them; the iteration counter is kept. DOPF_E_INVALID, with
 * nothing stored, for a NULL pointer or a NaN / Inf entry (the message names it). */
int dopf_set_demand(dopf_ctx *ctx, const double *demand /* N x T, [n + N*t] */);
/* dopf_roll_horizon: the window advances by k steps, 1 <= k <= T - 1, on the device: the new value at t is the old one at t + k for
 * t < T - k ("kept"); behind it ("tail"): demand = demand_tail, N x k, [n + N*j]; P = the old P[g, T-1] (persistence; the next
 * x-update clamps it to the cap, as for dopf_set_state); D = C = 0; lambda, mu, rho, avg_U, avg_K (and what the last solve read of
 * them) and, with DOPF_F_LINE_RATING, the rating table = their old values at T - 1 (a derating persists until the caller sets a new
 * table). Each storage's initial level becomes min(max(E[s, k-1], 0), max_level[s]) with E what
 * dopf_get_primal returns just before the call. The terminal band and the availability table stay as they are: the band now
 * applies to the new window's end, and the caller sets the new window's profiles with dopf_set_generator_availability. Status:
 * iteration = 2, converged = 0, halt from max_iters, residual maxima cleared; the warm-start summaries are reset. By definition the
 * context is then in the state of a fresh context of the shifted problem after the same setters and dopf_set_state(shifted arrays,
 * iteration = 2). The new initial levels are computed and checked first: a refusal leaves the context as it was.
 * DOPF_E_INVALID for k < 1, k >= T, a NULL demand_tail, a NaN / Inf in it, or a stored terminal band that is unreachable from the
 * new initial levels; DOPF_E_UNSUPPORTED with storages in a context without DOPF_F_STO_INITIAL_LEVEL, and on a context with
 * DOPF_F_GEN_RAMP or DOPF_F2_GEN_ENERGY_BUDGET: those roll with dopf_roll_horizon_coupled below. */
int dopf_roll_horizon(dopf_ctx *ctx, int32_t k, const double *demand_tail /* N x k, [n + N*j] */);
/* dopf_roll_horizon_coupled: dopf_roll_horizon's rule, unchanged, plus a rule for the state that couples a generator's timesteps
 * (DESIGN.md 5y), so that a context with ramp limits or energy budgets keeps its arrays, its scratch and its captured graphs over a
 * receding-horizon run. With P the rows just before the call, every value in the caller's generator order:
 *   anchor p_prev[g] (DOPF_F_GEN_RAMP)            = P[g, k-1], bit for bit, also where none was stored before
 *   ramp_up, ramp_down, c2, the terminal band     unchanged
 *   budgets (DOPF_F2_GEN_ENERGY_BUDGET), set_budget == 0: spent[g] = ((P[g,0] + P[g,1]) + ..) + P[g,k-1], summed left to right from
 *                                                 P[g,0]; e_min = fmax(0, e_min - spent), e_max = fmax(0, e_max - spent); +inf stays
 *   budgets, set_budget != 0                      e_min / e_max as dopf_set_generator_energy_budget takes them (either may be NULL:
 *                                                 0 / +inf): the new window's own budgets
 *   availability, n_profiles == -1                the stored table and indices stay, as in dopf_roll_horizon
 *   availability, n_profiles >= 0                 the new window's table and indices, as dopf_set_generator_availability takes them
 *                                                 (0 with both NULL: every generator back to -1); needs DOPF_F_GEN_AVAILABILITY
 * The table and the budgets are arguments, not setter calls behind the roll, because the new anchor and what is left of the budgets
 * must be feasible under the NEW window's caps: the stored table does not move with the window, so the old table under the new
 * anchor (or the new table under the old anchor) may be refused where the new window is feasible; and with DOPF_F2_GEN_RAMP_BUDGET
 * what is left of e_max can be less than the slowest way down from the new anchor delivers, so that the caller has to state the
 * new window's budget. All checks run before anything is overwritten, and a refusal leaves every getter as it was: first
 * dopf_roll_horizon's (k, the tail, a communicator or peer exchange, storages without DOPF_F_STO_INITIAL_LEVEL, the band's
 * reachability), then those of dopf_set_generator_ramp, dopf_set_generator_energy_budget and dopf_set_generator_availability on the
 * new anchor, the new budgets and the table that will be in force, the joint check of DOPF_F2_GEN_RAMP_BUDGET included (DOPF_E_INVALID;
 * the messages name this entry and the caller's g). DOPF_E_INVALID for n_profiles < -1; DOPF_E_UNSUPPORTED for a table without
 * DOPF_F_GEN_AVAILABILITY and for set_budget != 0 without DOPF_F2_GEN_ENERGY_BUDGET. On a context with neither flag, with
 * n_profiles == -1 and set_budget == 0, the entry is dopf_roll_horizon bit for bit; with G == 0 the generator part does nothing.
 * Status, the warm-start summaries and timing as after dopf_roll_horizon; the graphs stay valid (a table larger than any before
 * follows dopf_set_generator_availability's rule: a new allocation, and the graphs are captured again). While a trace is active the
 * entry works as the setters do. There is no dopf_multi_* wrapper. While dopf_set_generator_energy_budget_windows holds a table
 * the entry returns DOPF_E_UNSUPPORTED with nothing changed: remove the table, roll, and set the next window's table. */
int dopf_roll_horizon_coupled(dopf_ctx *ctx, int32_t k, const double *demand_tail /* N x k, [n + N*j] */,
                              int32_t n_profiles /* -1: the table stays */, const double *profiles /* n_profiles x T, [t + T*p] */,
                              const int32_t *profile_of /* G */, int32_t set_budget, const double *e_min /* G; NULL = 0 */,
                              const double *e_max /* G; NULL = +inf */);
/* The stored ramp limits, anchor (NaN: none) and energy budgets, G values each in the caller's order; any pointer may be NULL. They
 * come from the context's host copies: no device call, callable at any time. Without DOPF_F_GEN_RAMP the ramps are +inf and the
 * anchor NaN, without DOPF_F2_GEN_ENERGY_BUDGET the budgets are 0 and +inf. After dopf_roll_horizon_coupled they hold what the
 * device computed, which lets a host mirror follow the device's arithmetic. */
int dopf_get_generator_coupling(dopf_ctx *ctx, double *ramp_up, double *ramp_down, double *p_prev, double *e_min, double *e_max);

/* ---- the iteration history on the device ---------------------------------------------------------------
 * The reference's data product is the history of a run: admm.lambdas, admm.mues, admm.rhos, admm.results and admm.convergence hold
 * one entry per iteration (src/structures/admm.jl, src/optimization/run.jl:1-16). A trace records it without a host round trip per
 * iteration: while one is active, dopf_iterate(n) keeps running its n iterations back to back, and every COMPUTED iteration writes
 * one slot of a ring in device memory (one more kernel per iteration). A slot always holds a row: the three residual
 * maxima and the total cost exactly as dopf_get_residuals and dopf_get_consensus return them right after that iteration, the
 * value admm.iteration had DURING that solve, and converged. `what` adds array sections (0: the row alone, the convergence curve): */
#define DOPF_TRACE_DUALS     1   /* lambda[T], mu[L*T], rho[L*T] after the iteration's update (dopf_get_duals) */
#define DOPF_TRACE_CONSENSUS 2   /* injection[N*T], avg_U, avg_K, line_util[L*T each] (dopf_get_consensus) */
#define DOPF_TRACE_PRIMAL    4   /* P[T*G], D, C[T*S] (dopf_get_primal; E is derived when read) */
/* The ring keeps the last `capacity` slots. recorded counts the slots written since begin or reset, held = min(recorded, capacity);
 * dopf_trace_read indexes the held slots oldest first, 0 <= first, first + n <= held, and does not consume them. Its outputs are
 * slot-major — rows[4*i ..] = lam_res, mu_res, rho_res, total_cost of slot first + i; lambda[t + T*i], mu[l + L*t + L*T*i],
 * P[t + T*g + T*G*i], ... in the getters' layouts and the caller's agent order — and any pointer may be NULL. By definition slot i
 * equals, bit for bit, what the getters return when called after that iteration; E is what dopf_get_primal forms from the slot's D
 * and C under the initial levels and efficiencies stored when it is READ. The copies are ordered on the context's stream behind the
 * work already queued there.
 * dopf_trace_begin and dopf_trace_end let the iteration graphs be captured again at the next dopf_iterate (the chain gains or loses a
 * launch); dopf_trace_reset (recorded = 0 again, same ring) and dopf_trace_read do not. A context that never begins a trace launches
 * what it always launched. While a trace is active dopf_iterate alone advances the context: dopf_iterate_timed, dopf_local_update,
 * dopf_apply_consensus, dopf_comm_init, dopf_xchg_export and dopf_xchg_init return DOPF_E_INVALID; the setters (dopf_set_state,
 * dopf_set_demand, dopf_roll_horizon, the extensions') keep working, and the rows' iteration shows what they did to the counter.
 * dopf_destroy frees an active trace. dopf_trace_info without a trace reports zeros.
 * DOPF_E_INVALID: an unknown bit in what, capacity < 1, a second begin without an end, read / reset / end without a trace, a read
 * range outside the held slots, a non-NULL pointer for a section that what did not select (the message names it). DOPF_E_NOMEM,
 * naming the bytes, when capacity slots do not fit on the device. DOPF_E_UNSUPPORTED on a context joined to a communicator or a
 * peer exchange (a sharded history is not recorded). */
int dopf_trace_begin(dopf_ctx *ctx, int32_t what, int32_t capacity);
int dopf_trace_end(dopf_ctx *ctx);
int dopf_trace_reset(dopf_ctx *ctx);
int dopf_trace_info(dopf_ctx *ctx, int32_t *what, int32_t *capacity, int32_t *held, int32_t *recorded);
int dopf_trace_read(dopf_ctx *ctx, int32_t first, int32_t n,
                    double *rows /* 4*n: lam_res, mu_res, rho_res, total_cost */,
                    int32_t *iteration /* n */, int32_t *converged /* n */,
                    double *lambda, double *mu, double *rho,
                    double *injection, double *avg_U, double *avg_K, double *line_util,
                    double *P, double *D, double *C, double *E);

/* ---- the central reference on the device ---------------------------------------------------------------
 * Replaces src/opf_central_reference.jl:16-81 (one JuMP model of the whole multi-period DC-OPF, solved by Gurobi): the same
 * LP — variables P, D, C, E in their boxes, energy balance per timestep, |ptdf * injection| <= f_max, storage balance —
 * solved on the GPU by a first-order primal-dual method (diagonal step sizes, averaging, restarts; csrc/kernels_central.hip).
 * It is the parity target of the decentral run and independent of it. p holds ALL agents; q supplies device and flags.
 * Stops when |primal - dual objective| / (1 + |primal|) + worst violation / (1 + max demand) <= tol, or at max_iters.
 * Outputs (any may be NULL), layouts as in dopf_get_primal / dopf_get_consensus: P, D, C, E; system_price[T] = dual.(EB);
 * nodal_price[N*T] = lambda + sum_l (dual FlowUpper + dual FlowLower)[l,t] ptdf[l,:]; line_utilization[L*T] = ptdf * I;
 * flow_upper_dual[L*T] = dual.(FlowUpper), flow_lower_dual[L*T] = dual.(FlowLower) (opf_central_reference.jl:71-79: both are
 * d objective / d max_capacity <= 0, non-zero only where that limit binds). None of the three entries below takes the rating
 * table of DOPF_F_LINE_RATING: they solve with f_max in every timestep (a DOPF_F_LINE_RATING bit in q changes nothing).
 * All four entries take any horizon and need no flag for it: beyond T = 512 the rows that couple timesteps (storage levels, ramps,
 * budgets) run on the long sweeps (csrc/central_long.h), and the entry sets DOPF_F_LONG_HORIZON on its own context itself — what counts
 * is the shape. With the flag in q and without it the results are the same bits; the horizon is bounded by device memory alone. */
typedef struct dopf_central_result {
    double objective, dual_objective, primal_infeasibility, gap;
    int32_t iterations, converged;
} dopf_central_result;
int dopf_central_solve(const dopf_problem *p, const dopf_params *q, double tol, int32_t max_iters,
                       dopf_central_result *res, double *P, double *D, double *C, double *E,
                       double *system_price, double *nodal_price, double *line_utilization,
                       double *flow_upper_dual, double *flow_lower_dual);

/* The same LP with the inputs of DOPF_F_STO_INITIAL_LEVEL, DOPF_F_STO_TERMINAL_LEVEL and DOPF_F_GEN_AVAILABILITY: the parity target
 * of a decentral run that uses them. sto_e0[S] (NULL = all 0): the level rows become e0 + sum_{tau<=t} (C - D) in [0, max_level];
 * sto_end_lo[S], sto_end_hi[S] (both or neither; NULL = [0, max_level]): the row of the last timestep lies in [lo, hi] instead;
 * profiles (T x n_profiles, [t + T*k]) and profile_of[G] (-1 = always gen_pmax): the box of P[g,t] is [0, gen_pmax[g] *
 * profiles[t + T*profile_of[g]]]. All in the caller's agent order, like p. Meaning, checks and error codes are those of
 * dopf_set_storage_initial_level, dopf_set_storage_terminal_level (incl. the band's reachability from e0) and
 * dopf_set_generator_availability: the entry sets the matching flag for every input given and calls them on its own context; a
 * refusal returns that setter's code, its message (dopf_last_error(NULL)) names this entry, and no output is written. The E output
 * holds levels that include e0, as dopf_get_primal returns them. With every input NULL / 0 this is dopf_central_solve. */
int dopf_central_solve_ex(const dopf_problem *p, const dopf_params *q,
                          const double *sto_e0,
                          const double *sto_end_lo, const double *sto_end_hi,
                          int32_t n_profiles, const double *profiles,
                          const int32_t *profile_of,
                          double tol, int32_t max_iters, dopf_central_result *res,
                          double *P, double *D, double *C, double *E,
                          double *system_price, double *nodal_price, double *line_utilization,
                          double *flow_upper_dual, double *flow_lower_dual);

/* The same LP with lossy storages: dopf_central_solve_ex's arguments plus the input of DOPF_F_STO_EFFICIENCY, the parity target of a
 * decentral run that uses it. sto_eta_c[S], sto_eta_d[S] (both or neither, in the caller's agent order, every value in (0, 1]; both NULL
 * = all 1): the level rows become e0 + sum_{tau<=t} (eta_c C - D / eta_d) in [0, max_level] (in [lo, hi] at the last timestep), and the
 * E output holds these levels. The injection D - C, the boxes and the objective stay. When the arrays are given the entry sets
 * DOPF_F_STO_EFFICIENCY on its own context (a DOPF_F_STO_EFFICIENCY bit in q is ignored here too) and calls dopf_set_storage_efficiency
 * before the other setters, so that the band's reachability from e0 is checked over
 * [max(0, e0 - T pmax / eta_d), min(max_level, e0 + T eta_c pmax)]. Checks and codes are that setter's (a NaN, a value <= 0 or > 1, only
 * one array) and, as for dopf_central_solve_ex, the other three's; the message names this entry, and no output is written. With both
 * arrays NULL this is dopf_central_solve_ex; with both all 1 it returns the same bits. */
int dopf_central_solve_lossy(const dopf_problem *p, const dopf_params *q,
                             const double *sto_e0,
                             const double *sto_end_lo, const double *sto_end_hi,
                             const double *sto_eta_c, const double *sto_eta_d,
                             int32_t n_profiles, const double *profiles,
                             const int32_t *profile_of,
                             double tol, int32_t max_iters, dopf_central_result *res,
                             double *P, double *D, double *C, double *E,
                             double *system_price, double *nodal_price, double *line_utilization,
                             double *flow_upper_dual, double *flow_lower_dual);

/* The same LP with the constraints that couple a generator's timesteps, and with per-timestep line limits: dopf_central_solve_lossy's
 * arguments plus the inputs of dopf_set_line_rating, dopf_set_generator_ramp and dopf_set_generator_energy_budget — the parity target
 * of a decentral run that uses DOPF_F_LINE_RATING, DOPF_F_GEN_RAMP (with or without DOPF_F_GEN_RAMP_NETWORK) or
 * DOPF_F2_GEN_ENERGY_BUDGET. All in the caller's agent order, each NULL = that input's default:
 *   line_rating[L*T]  [l + L*t], every entry finite and >= 0 (NULL: f_max in every timestep): -rating <= flow[l,t] <= rating.
 *   gen_ramp_up[G], gen_ramp_down[G]  both or neither, >= 0, +inf = no limit: -ramp_down <= P[g,t] - P[g,t-1] <= ramp_up for t >= 1.
 *   gen_prev[G]  the outputs of the step before the window, in [0, gen_pmax]: the same row at t = 0 against them (NULL: no such row).
 *   gen_e_min[G], gen_e_max[G]  0 <= e_min <= e_max, e_min finite (NULL: 0 and +inf): e_min <= sum_t P[g,t] <= e_max.
 * Meaning, checks and codes are the three setters' — an anchored generator must be able to come down under its caps, and a minimum
 * must fit under them, both under the availability table of this same call — except that budgets and ramps may be given together
 * (two coupling rows are nothing to an LP; only the decentral step refuses the pair). ramp_up without ramp_down (or the reverse),
 * tol <= 0 and max_iters < 1 are refused before a device is looked for. A refusal's message names this entry, and no output is written.
 * Ramps and budgets are taken on any horizon, beyond T = 512 too, with no flag in q. The flags of q that name these extensions are
 * ignored, as by the other entries: what counts is the arrays. Two more outputs, both d objective / d right-hand side like the flow
 * duals — negative where the row's upper end binds, positive where its lower end binds, 0 where neither does or the row does not exist:
 *   ramp_dual[T*G]   [t + T*g]: the ramp row between t - 1 and t (t = 0: the anchor's row)
 *   budget_dual[G]   the budget row: minus the price of generator g's energy over the window (the water value of a capped reservoir)
 * primal_infeasibility includes the worst ramp and budget violation. With all six inputs NULL this is dopf_central_solve_lossy, bit for
 * bit (the two duals are zeros). */
int dopf_central_solve_coupled(const dopf_problem *p, const dopf_params *q,
                               const double *sto_e0,
                               const double *sto_end_lo, const double *sto_end_hi,
                               const double *sto_eta_c, const double *sto_eta_d,
                               int32_t n_profiles, const double *profiles,
                               const int32_t *profile_of,
                               const double *line_rating,
                               const double *gen_ramp_up, const double *gen_ramp_down, const double *gen_prev,
                               const double *gen_e_min, const double *gen_e_max,
                               double tol, int32_t max_iters, dopf_central_result *res,
                               double *P, double *D, double *C, double *E,
                               double *system_price, double *nodal_price, double *line_utilization,
                               double *flow_upper_dual, double *flow_lower_dual,
                               double *ramp_dual, double *budget_dual);

/* ---- consensus sum across GPUs inside the library (RCCL over xGMI, loaded at run time) -------------
 * Replaces nothing in the reference (it has no parallelism); what is distributed is the agent loop of
 * optimize_all_subproblems! (src/optimization/subproblems.jl:1-17) and the agent sums of Result(...)
 * (src/structures/results.jl:72-106), summed over ranks by ONE all-reduce per iteration.
 *
 * One process per GPU: every rank creates its context from its shard (dopf_problem.G/S = local agents,
 * dopf_params.n_agents_global = all agents), rank 0 calls dopf_comm_unique_id and ships the 128 bytes to
 * the other ranks over any host channel (MPI, torch.distributed, a file), every rank calls dopf_comm_init.
 * From then on dopf_iterate runs local_update -> all-reduce -> apply_consensus per iteration with no host round
 * trip: plain launches by default, captured in its hipGraphs with DOPF_F_COMM_GRAPH (back to plain launches if RCCL
 * refuses the capture). */
#define DOPF_COMM_ID_BYTES 128
int dopf_comm_unique_id(void *id128);
int dopf_comm_init(dopf_ctx *ctx, int32_t world, int32_t rank, const void *id128);
/* world / rank of the context's communicator (1 / 0 without one); in_graph = 1 once dopf_iterate has
 * captured the collective into its graphs, 0 while it launches eagerly. Any pointer may be NULL. */
int dopf_comm_info(const dopf_ctx *ctx, int32_t *world, int32_t *rank, int32_t *in_graph);

/* ---- peer exchange: the same sum without a collective library ------------------------------------------------
 * For the sub-kilobyte consensus vector of a copper plate (776 B on BASELINE configs[2]) a library all-reduce is pure
 * latency (tens of microseconds against a 40 us iteration). Here ONE kernel per iteration stores this rank's vector
 * into every peer's receive area over xGMI, publishes a sequence number, waits for the peers' numbers and adds the
 * copies in rank order (bitwise identical sums on every rank; csrc/kernels_consensus.hip k_xchg). The kernel is part of
 * the iteration hipGraphs. One process per GPU: every rank calls dopf_xchg_export (allocates its receive area, returns
 * a 64-byte hipIpc handle), the world handles are gathered in rank order over any host channel, every rank calls
 * dopf_xchg_init (maps the peers' areas, host rendezvous). world <= 16. A peer that does not show up within
 * DOPF_XCHG_TIMEOUT_MS (default 20 000) makes dopf_iterate / dopf_sync return DOPF_E_DEVICE; the kernels always end. */
#define DOPF_XCHG_HANDLE_BYTES 64
int dopf_xchg_export(dopf_ctx *ctx, int32_t world, void *handle64);
int dopf_xchg_init(dopf_ctx *ctx, int32_t world, int32_t rank, const void *handles /* world x 64 bytes, rank order */);

/* One process, n GPUs — what a Julia `ccall` host uses (no launcher): p holds ALL agents; the library
 * cuts the agent lists into n contiguous shards, creates one context per device (devices[i], or 0..n-1
 * when NULL), joins them with ncclCommInitAll and drives each from its own host thread.
 * Replaces ADMM(...) + run!(admm) exactly like dopf_create + dopf_iterate do on one GPU. */
typedef struct dopf_multi dopf_multi;
int  dopf_multi_create(dopf_multi **out, const dopf_problem *p, const dopf_params *q, int32_t n_gpus,
                       const int32_t *devices);
/* dopf_multi_create with the second flag word, as dopf_create_ex: every shard is created with flags2 */
int dopf_multi_create_ex(dopf_multi **out, const dopf_problem *p, const dopf_params *q, int32_t n_gpus,
                         const int32_t *devices, int32_t flags2);
void dopf_multi_destroy(dopf_multi *m);
const char *dopf_multi_last_error(const dopf_multi *m);   /* m == NULL: last dopf_multi_create error */
int  dopf_multi_iterate(dopf_multi *m, int32_t n_iters, int32_t *iters_done, int32_t *converged);
/* Primal rows of all shards in the caller's agent order (layout of dopf_get_primal). */
int  dopf_multi_get_primal(dopf_multi *m, double *P, double *D, double *C, double *E);
int32_t dopf_multi_size(const dopf_multi *m);
/* dopf_set_storage_initial_level for all storages, e0[S] in the caller's order (NULL = all 0): each shard gets its slice. Every
 * shard's values are checked before any is stored. */
int  dopf_multi_set_storage_initial_level(dopf_multi *m, const double *e0);
/* dopf_set_storage_terminal_level for all storages, lo[S] and hi[S] in the caller's order (both NULL = the default band): each shard
 * gets its slice. Every shard's values are checked before any is stored. */
int  dopf_multi_set_storage_terminal_level(dopf_multi *m, const double *lo, const double *hi);
/* dopf_set_line_rating on every shard: each gets the whole table (replicated state); every shard is checked before any is stored. */
int  dopf_multi_set_line_rating(dopf_multi *m, const double *rating /* L x T, [l + L*t]; NULL = f_max */);
/* dopf_set_storage_efficiency for all storages, eta_c[S] and eta_d[S] in the caller's order (both NULL = all 1): each shard gets its
 * slice; every shard is checked before any is stored */
int  dopf_multi_set_storage_efficiency(dopf_multi *m, const double *eta_c, const double *eta_d);
/* all G generators in the caller's order; every shard gets the whole table and its slice of profile_of (checked for every shard
 * before any is stored) */
int dopf_multi_set_generator_availability(dopf_multi *m, int32_t n_profiles, const double *profiles, const int32_t *profile_of);
/* dopf_set_generator_quadratic_cost for all G generators, c2[G] in the caller's order (NULL = all 0): each shard gets its slice;
 * every shard is checked before any value is stored */
int dopf_multi_set_generator_quadratic_cost(dopf_multi *m, const double *c2);
/* dopf_set_generator_ramp for all G generators, arrays in the caller's order (NULL as there): each shard gets its slice; every shard
 * is checked before any value is stored */
int dopf_multi_set_generator_ramp(dopf_multi *m, const double *ramp_up, const double *ramp_down, const double *p_prev);
/* dopf_set_generator_energy_budget for all G generators, arrays in the caller's order (NULL as there): each shard gets its slice;
 * every shard is checked before any value is stored */
int dopf_multi_set_generator_energy_budget(dopf_multi *m, const double *e_min, const double *e_max);
/* dopf_set_generator_min_output for all G generators, p_min in the caller's order (NULL as there): each shard gets its slice; every
 * shard is checked before any stores */
int dopf_multi_set_generator_min_output(dopf_multi *m, const double *p_min);
/* dopf_set_generator_budget_min_output for all G generators, p_min in the caller's order (NULL as there): each shard gets its
 * slice; every shard is checked before any stores */
int dopf_multi_set_generator_budget_min_output(dopf_multi *m, const double *p_min);
/* dopf_get_generator_budget_price of all shards' rows in the caller's order, like dopf_multi_get_primal: G values */
int dopf_multi_get_generator_budget_price(dopf_multi *m, double *nu /* G */);
/* dopf_set_generator_energy_budget_windows for all G generators: the ends are replicated, each shard gets the rows of its
 * generators ([j + n_win*g]: a slice); all or nothing, as the other dopf_multi_set_* entries */
int dopf_multi_set_generator_energy_budget_windows(dopf_multi *m, int32_t n_win, const int32_t *win_end, const double *e_min,
                                                   const double *e_max);
/* dopf_get_generator_budget_window_price of all shards' rows in the caller's order: n_win x G values */
int dopf_multi_get_generator_budget_window_price(dopf_multi *m, double *nu /* n_win x G */);
/* dopf_get_generator_ramp_price of all shards' rows in the caller's order, like dopf_multi_get_primal: T*G values */
int dopf_multi_get_generator_ramp_price(dopf_multi *m, double *rp /* T*G, [t + T*g] */);
/* Shard i's context: duals, consensus state, residuals and prices are replicated, read them from
 * shard 0 with the dopf_get_* calls above. */
dopf_ctx *dopf_multi_ctx(dopf_multi *m, int32_t i);
/* Diagnostics, 15 counters: [0..2] scan-kernel statistics (only in -DDOPF_STATS builds), [3] storages the
 * active-set kernel certified in the LAST iteration, [4] storages it left to the scan kernel, [5..8] contact-set
 * rounds / Newton iterations (sum, max per lane group), [9..14] cycles per section (DOPF_STATS builds). */
int dopf_debug_stats(dopf_ctx *ctx, uint64_t *out15);
/* Diagnostics (-DDOPF_STATS builds; -1 otherwise): 8 wall-clock stamps (100 MHz) per wave of the storage body's last launch. */
int dopf_debug_timeline(dopf_ctx *ctx, uint64_t *out, int32_t n);
/* networks: out3 = { the quiet chain (no k_slack launch while no line is flagged) is allowed for this context, the next launches
 * would use it, times it parked itself because a line got flagged and the host went back to the chain with k_slack } */
int dopf_debug_quiet(dopf_ctx *ctx, int64_t *out3);
/* Diagnostics (L > 0): the breakpoint table of node n, timestep t that the last x-update used:
 * beta, psi: 2L doubles (first *m valid, ascending), slope: 2L+1, psi0 = Psi(0). */
int dopf_debug_table(dopf_ctx *ctx, int32_t n, int32_t t, double *beta, double *psi, double *slope,
                     double *psi0, int32_t *m);
const char *dopf_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DOPF_H */
