// dopf_ctx.h — the context behind the C ABI, shared by dopf_api.hip and dopf_comm.hip (internal).
#pragma once

#include <string>
#include <vector>

#include "dopf_internal.h"
#include "trace_layout.h"

struct dopf_comm_state;     // dopf_comm.hip: RCCL communicator of a sharded context
namespace dopf { struct TraceBlock; }   // trace.h

struct dopf_ctx {
    dopf::DevView v{};
    dopf::Plan plan{};              // the launch chain (plan_chain, dopf_create)
    dopf_params q{};
    int device = 0;
    hipStream_t main = nullptr, side = nullptr;
    bool own_main = false;
    hipEvent_t evFork = nullptr, evJoin = nullptr;
    hipEvent_t evT0 = nullptr, evT1 = nullptr;      // DOPF_F_TIME_CALLS: around the launches of the last dopf_iterate
    double last_call_ms = -1.0;
    // The iteration graphs, kUnroll, kMid and 1 iterations per launch (dopf_api.hip: kGraphIters), built when first used; [1]: the
    // quiet chain's. Networks on the three-launch chain: while no line is flagged (Status::walk_last == 0 at the last look) the "quiet"
    // chain runs — k_net_agents and the dual/price kernel, which forms the node sums itself; k_slack is not launched.
    struct Graphs {
        hipGraphExec_t g[3] = {};
        bool valid = false;
    } graphs[2];
    bool quiet = false;             // no line flagged at the last look: the next launches may use the quiet chain (if quiet_allowed)
    unsigned long long quiet_parked = 0;    // times the quiet chain parked itself (a line got flagged) and the host went back
    std::vector<void *> allocs;
    void *own_cons = nullptr;
    double *getter_scratch = nullptr;      // 3 * N * T doubles, allocated at the first getter that needs them (freed with the context)
    double *roll_scratch = nullptr;        // dopf_roll_horizon(_coupled): the moved vectors, the demand tail, the new initial levels, the new anchors and budgets
    std::vector<int> gen_perm, sto_perm;   // sorted position -> caller's index
    std::vector<double> sto_h;             // the storage block as it is on the device (dopf_internal.h: StoSlot, sto_slots(plan) slots of S
                                           // values, sorted order): the setters' bounds, and what each checks reachability against
    std::vector<double> sto_pmax_h;        // max charge / discharge per step, sorted order (reachability)
    std::vector<int> gen_prof_h;           // DOPF_F_GEN_AVAILABILITY: the generators' profile indices on the device (sorted order)
    double *gen_avail = nullptr;           // ... the profile table on the device (its address is in gen_avail_slot(v)) and the
    int gen_avail_cap = 0;                 //     profiles it has room for
    std::vector<double> gen_ramp_h;        // DOPF_F_GEN_RAMP: gen_pmax | ramp_up | ramp_down | p_prev (NaN: none) as on the device (sorted order), and
    std::vector<double> gen_avail_h;       //     with DOPF_F_GEN_AVAILABILITY the profile table: what the two setters check the anchors against
    std::vector<double> gen_min_h;         // ... and the floors p_min of dopf_set_generator_min_output as on the device (sorted order; zeros until then)
    int32_t flags2 = 0;                    // the second flag word (DOPF_F2_*, dopf_create_ex)
    std::vector<double> gen_budget_h;      // DOPF_F2_GEN_ENERGY_BUDGET: gen_pmax | e_min | e_max as on the device (sorted order); gen_avail_h is
                                           //     kept for these contexts too: what the two setters check e_min <= sum_t cap against
    std::vector<int32_t> gen_bw_end_h;     // dopf_set_generator_energy_budget_windows: the window ends (empty: no table), and
    std::vector<double> gen_bw_h;          //     e_min | e_max, n_win x G each as on the device (sorted order, [j + n_win*i])
    void *gen_bw_base = nullptr;           // ... the device block behind plan.genBudgetWin (an entry of allocs; freed when n_win changes)
    std::vector<double> gen_bmin_h;        // dopf_set_generator_budget_min_output: the floors p_min as on the device (sorted order; empty until the first
                                           //     array: no floors), behind plan.genBudgetMinOut, and that array (kept across a NULL call, zeroed)
    double *gen_bmin_d = nullptr;
    dopf::Status host_st{};
    dopf::Status *host_pin = nullptr;       // page-locked landing area of the status read-back (a pageable target is staged: slower)
    unsigned long long solver_fail_seen = 0;   // failures already reported through DOPF_E_SOLVER
    dopf_comm_state *comm = nullptr;       // non-null: dopf_iterate runs local_update -> all-reduce -> apply_consensus
    bool tail_xchg = false;                // peer exchange inside the tail block of the one-launch iteration (copper plates)
    bool level_from_primal = true;         // dopf_get_primal rebuilds E = cumsum(C - D); false while a central solve's own levels are in v.E
    // dopf_trace_* (DESIGN.md 5w): run-time state of the context, not part of the plan. While active, enqueue_iteration ends with
    // k_trace, and dopf_iterate is the only entry that advances the context.
    struct Trace {
        bool active = false;
        int what = 0, capacity = 0;
        int base = 0;                       // host_st.iters_total at begin / reset: recorded = host_st.iters_total - base
        dopf::TraceLayout lay{};
        char *ring = nullptr;               // capacity slots of lay.slot_bytes
        dopf::TraceBlock *blk = nullptr;    // the trace block in device memory (base, the segment table)
        double *level = nullptr;            // dopf_trace_read: the levels of level_slots slots at a time (S * T doubles each)
        int level_slots = 0;
    } trace;
    char err[512] = {0};
    double *sto_slot_h(int slot) { return sto_h.data() + (size_t)slot * (size_t)v.S; }                  // a held slot of the mirror
    double sto_at(int slot, int i) const { return sto_h[(size_t)slot * (size_t)v.S + (size_t)i]; }      // ... and sorted storage i of it
    // the context's budget prices on the device (dopf_internal.h: gen_budget_price(v, pair)): the layout comes from the plan here, so
    // that no host caller states it by hand
    double *gen_budget_price_d() const { return dopf::gen_budget_price(v, plan.genRampBudget); }
};

namespace dopf {

int fail(dopf_ctx *c, int code, const char *fmt, ...);
void keep_error(const dopf_ctx *c);          // the context's message becomes what dopf_last_error(NULL) returns
void drop_graphs(dopf_ctx *c);
int read_status(dopf_ctx *c);
void trace_release(dopf_ctx *c);             // frees an active trace's device memory (dopf_trace_end, dopf_destroy)
int check_initial_levels(dopf_ctx *c, const double *e0);   // the checks of dopf_set_storage_initial_level (flag, 0 <= e0 <= emax)
int check_terminal_levels(dopf_ctx *c, const double *lo, const double *hi);   // those of dopf_set_storage_terminal_level
int check_storage_efficiency(dopf_ctx *c, const double *eta_c, const double *eta_d);   // those of dopf_set_storage_efficiency
int check_generator_availability(dopf_ctx *c, int32_t K, const double *profiles, const int32_t *profile_of);   // dopf_set_generator_availability's
int check_line_rating(dopf_ctx *c, const double *rating);   // those of dopf_set_line_rating (flag, finite, >= 0)
int check_generator_quadratic_cost(dopf_ctx *c, const double *c2);   // those of dopf_set_generator_quadratic_cost (flag, finite, >= 0)
// those of dopf_set_generator_ramp (flag, no NaN, ramps >= 0 and both or neither, p_prev in [0, gen_pmax], the anchors under the caps)
int check_generator_ramp(dopf_ctx *c, const double *up, const double *down, const double *prev);
// those of dopf_set_generator_min_output (the ramp flag, no budget, 0 <= p_min <= gen_pmax, a path for every row with a floor)
int check_generator_min_output(dopf_ctx *c, const double *p_min);
// those of dopf_set_generator_energy_budget (flag, no NaN, 0 <= e_min <= e_max, e_min finite and <= sum_t cap)
int check_generator_energy_budget(dopf_ctx *c, const double *e_min, const double *e_max);
// those of dopf_set_generator_energy_budget_windows (flag, no pair, no whole-horizon budget, the ends, the values, every window's
// e_min <= the window's sum of caps)
int check_generator_energy_budget_windows(dopf_ctx *c, int32_t n_win, const int32_t *win_end, const double *e_min, const double *e_max);
// those of dopf_set_generator_budget_min_output (the budget flag, no ramps, 0 <= p_min <= gen_pmax finite, sum floor <= e_max per row or window)
int check_generator_budget_min_output(dopf_ctx *c, const double *p_min);
// the two without their flag checks, for a caller that keeps the arrays itself (dopf_central_solve_coupled; `entry`: the name the
// messages carry). pmax: capacities in sorted order; table: the availability profiles [t + T*k] the context's gen_prof_h refers to
int check_generator_ramp_values(dopf_ctx *c, const char *entry, const double *pmax, const double *table, const double *up, const double *down,
                                const double *prev);
int check_generator_energy_budget_values(dopf_ctx *c, const char *entry, const double *pmax, const double *table, const double *e_min,
                                         const double *e_max);
void launch_demote_full_rows(const DevView &v, hipStream_t s);   // gen_state 1 -> 2 (the caps changed)
// dopf_comm.hip
int check_one_runtime(dopf_ctx *c);           // DOPF_E_UNSUPPORTED when two HIP runtimes are mapped into the process
int comm_enqueue_allreduce(dopf_ctx *c);      // sum of the consensus buffer over the ranks, on the context's stream
void comm_release(dopf_ctx *c);
int comm_world(const dopf_ctx *c);             // ranks of the context's communicator (1 without one)
const XchgView *comm_xchg(const dopf_ctx *c);   // the initialised peer exchange of the context, or null
bool comm_capturable(const dopf_ctx *c);      // the chain incl. its consensus sum may go into a hipGraph by default

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { hipGetDevice(&prev); if (dev != prev) hipSetDevice(dev); else prev = -1; }
    ~DeviceGuard() { if (prev >= 0) hipSetDevice(prev); }
};

#define HIPCHK(c, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return dopf::fail((c), DOPF_E_DEVICE, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

}  // namespace dopf
