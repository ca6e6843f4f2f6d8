// ps_options.h -- the handle's user options: the members (PsOptions, a base of ps_problem), and ONE table that says for every
// option name which member it writes, how the value is parsed, what is refused (with which words) and what the change
// invalidates on the handle.  No HIP: tests/test_options_host.py compiles it with a plain C++ compiler and holds every row
// against its own transcription.  ps_set_option (ps_abi_solver.h) is the null check, the two names a caller's loop sets per
// iteration ("expect_next", "solve_horizon": no table look-up, nothing invalidated), ps_option_apply and the effects.
// include/pyslam_hip.h documents every name of the table with its default and range.
#pragma once
#include <cmath>
#include <cstring>

#include "ps_limits.h"

struct PsOptions {
    int pcg_variant = 1;            // 1 = fused single-reduction CG, 0 = classic two-launch PCG
    int pcg_chunk = 8;              // launches between host polls of the 'done' flag
    int coarse_req = -1;            // "coarse_groups": requested number of groups: -1 = auto, 0 = off
    int coarse_basis = 1;           // coarse basis P_iq = w(i,q) B_i: B_i = L_i^T Ad(T_i) (1, rigid-motion aware) or I (0)
    int coarse_lag = 1;             // the factorisation of THIS iteration's A_c on a side stream, the CG with the previous one's
    int lagx = 1;                   // "coarse_lag_x": lagged three-launch set-up (k_rows_setup)
    int lin_zero_list = 1;          // the option as set (ps_problem::lin_zero_gate: whether the handle is eligible)
    int cg_ablate = 0, schur_ablate = 0, lm_ablate = 0;   // measurement build only
    int schur_pipeline = 1;         // k_schur_pairs_db (two chunks per wave in flight) instead of k_schur_pairs
    int mo_fused = 1;               // "fused_motion_only": one launch per iteration (k_motion_only_iteration)
    int direct_fused = 1;           // the direct solve in one launch (k_direct_solve); measurement build: PS_DIRECT_3LAUNCH -> 0
    int direct_max = 90;            // "direct_max_unknowns": reduced systems up to this many unknowns are solved directly (0: never)
    int big_chol = 1;               // nc > 90: multi-workgroup blocked factorisation (0: one workgroup out of L2)
    int explicit_ok = 1;            // "cg_explicit": the explicit two-level PCG (long sparse chains) may be chosen
    int xcg_refresh_every = 1;      // "coarse_refresh_every": lagged set-ups between two refreshes of the coarse inverse
    // "coarse_auto_hold": keep the lagged coarse inverse (no assembly, no side-stream factorisation) while the solve has
    // settled -- the last whole-iteration call changed the cost by less than 1e-4 relative -- for at most 3 set-ups in a row
    int xcg_auto_hold = 1;
    int xcg_adaptive_hold = 1;      // "coarse_adaptive_hold": keep the lagged inverse while it still does its job (xcg_setup)
    int band_chol = 1;              // banded coarse matrix (ps_k_band.h): band factor by rows / columns
    int band_part = 1;              // ... by the PARTITIONED factorisation (ps_k_bandpart.h) where it applies
    int band_part_m = 0;            // "band_part_chunk": interior nodes per chunk (0: automatic, ~ sqrt(B ncb) - B)
    int hold_across_steps = 1;      // BA rows keep a coarse inverse that still converges as fast, also behind a big step
    int sync_refactor = 1;          // pose graphs factor the CURRENT coarse matrix on the solver stream behind a step that halved the cost
    int xcg_rt = 1;                 // "xcg_restrict_fused": three-launch form (restriction folded into the SpMV epilogue)
    int xcg_fused = 1;              // 0 = three launches per iteration, 1 = one (two when the coarse level is too wide), 2 = two
    int cg_lds = 1;                 // small systems: k_cg_fused_lds (whole vector through LDS)
    int cg_persist = 1;             // the folded CG in ONE launch (ps_k_cg_persist.h); also cleared by a solve whose launch timed out
    unsigned cp_spin = 200000;      // "cg_persist_spin": passes over the exchange before a workgroup gives up
    int xcg_persist = 1;            // the explicit two-level PCG as one launch per solve (ps_k_xcg_persist.h); cleared likewise
    int prof_every = 1;             // "profile_every": profiling level 1 times the Schur kernel of every n-th linearisation only
    int cg_force_restart = 0;       // tests: end the first pass of a synchronous solve at 1e-4 and restart from the true residual
    // tests: n > 0 = CG iteration n - 1 of the first pass of the NEXT reduced solve finds denom <= 0 (its delta is overwritten in front
    // of that launch: cg_fused_launch, xcg_launch) and reports a breakdown; cleared by the set-up of that solve
    int cg_force_breakdown = 0;
    int cg_margin = 4;              // CG launches enqueued beyond the previous solve's iteration count
    int cg_split_min_rows = 1024;   // split mode (coarse rows owned by k_cg_reduce_split) beyond this many reduced poses
    int cg_explicit_min_rows = -1;  // explicit two-level PCG beyond this many reduced poses (-1: 400 for pose-graph rows, 540 for BA rows)
    int lm_packed = 1;              // landmark pass / back-substitution with the lanes packed by observation (ps_k_packed.h)
    int pose_xcd = 1;               // the pose pass's items in eight contiguous ranges, one per XCD
    // lagged dense inverse of the reduced system as the CG preconditioner (ps_k_ldi.h / ps_host_ldi.h)
    int ldi_enable = 1;             // "lagged_inverse"
    int ldi_max_n = 2048;           // "ldi_max_unknowns": reduced systems up to this many unknowns
    int ldi_cap = 12;               // PCG iterations before a solve gives the inverse up
    int ldi_seed_steps = 3;         // Newton-Schulz steps of a seed
    double ldi_cost_tol = 0.05;     // try the inverse while the last step changed the cost by at most this (relative)
    int ldi_refresh_its = 7;        // solves slower than this switch the per-iteration refresh on
    // calls between a seed's start and its first use (fixed schedule).  1: the call after the seed waits for it where the solve
    // begins (~0.1 ms of the seed's GEMMs are then still ahead at C3, hidden behind this call's linearisation for most of it) and
    // takes 6 iterations instead of 18-25 -- eight-call solves 3-7 % shorter at every size from 138 to 2 034 unknowns than with 2
    int ldi_seed_lag = 1;           // (measurement build: PS_LDI_SEED_LAG)
    // direct seed (ps_host_ldi.h: ldi_direct_enqueue): "ldi_direct" -1 auto (ok, not on), 0 never, 1 always.  ldi_direct is ALSO
    // written by the solver: switched on for pose graphs from the start and for any problem after a rejected Newton-Schulz seed
    // (ldi_ensure, ldi_decide), and back off by ps_reset_solver_state
    bool ldi_direct = false, ldi_direct_ok = true;
    int expect_next = 0;            // a successor call is expected (ps_set_option's early path; ps_solve sets it per iteration)
    int fuse_cost = 1;              // 0 off, 1 on, 2 = in the tails only (not the start cost / ps_eval_cost)
};

// whether the lagged dense inverse can apply to a reduced system of n unknowns at all: decides the folded / explicit crossover
// (build_coarse), whether an option change has the coarse level rebuilt (relook_path), and is part of ldi_eligible
inline bool ps_ldi_possible(const PsOptions& o, long n) {
    return o.ldi_enable && n <= o.ldi_max_n && n <= PS_LDI_MAXN && n > o.direct_max;
}

#ifdef PS_MEASURE
constexpr bool PS_MEASURE_BUILD = true;
#else
constexpr bool PS_MEASURE_BUILD = false;
#endif

// how a row turns the caller's double into the member
enum PsOptKind {
    PS_OPT_BOOL,          // value != 0
    PS_OPT_INT,           // (int)value, nothing refused
    PS_OPT_RANGE,         // refused when value < lo || value > hi, then (int)value
    PS_OPT_BELOW,         // refused when value < lo || value >= hi, then (int)value ("coarse_groups": truncated after the check)
    PS_OPT_EXACT,         // one of the integers lo .. hi exactly
    PS_OPT_SPIN,          // as PS_OPT_RANGE into the unsigned cp_spin
    PS_OPT_COST_TOL,      // refused unless value >= 0 (so NaN is), stored as a double in ldi_cost_tol
    PS_OPT_LDI_DIRECT,    // ldi_direct_ok = value != 0, ldi_direct = value > 0
};

// what a successful change invalidates on the handle (ps_set_option)
enum : unsigned {
    PS_FX_COARSE_REBUILD = 1u,     // coarse_built = false: the next solve plans the coarse level again
    PS_FX_DROP_FACTOR = 2u,        // lci_next = -1: the lagged coarse factor was made under the old value
    PS_FX_DROP_SIDE = 4u,          // side_todo = false: ... and so would the X that is still to be formed
    PS_FX_RELOOK_PATH = 8u,        // the folded / explicit crossover may move (relook_path)
    PS_FX_LDI_OFF = 16u,           // switched off: the dense inverse in use is dropped (a seed in flight runs out on its own)
};

struct PsOptionRow {
    const char* name;
    int PsOptions::* member;       // null for the three kinds that name their members themselves
    PsOptKind kind;
    double lo, hi;
    const char* refusal;           // what ps_last_error says about a refused value
    unsigned effects;
    bool measure_only;             // product build: 0 is accepted and changes nothing, anything else is refused; measurement build: by kind
};

#define PS_ABLATION_REFUSAL(name) name ": timing experiments exist in the measurement build only (__graft_entry__.build_measure(), PYSLAM_AMD_MEASURE=1)"

static const PsOptionRow PS_OPTION_TABLE[] = {
    {"pcg_variant", &PsOptions::pcg_variant, PS_OPT_EXACT, 0, 1, "pcg_variant must be 0 or 1", 0, false},
    {"coarse_groups", &PsOptions::coarse_req, PS_OPT_BELOW, -1, PS_XCG_MAXNODES,
     "coarse_groups out of range (-1 auto, 0 off, else number of hat intervals; above 63 only for the explicit two-level PCG, at most 1023)",
     PS_FX_COARSE_REBUILD, false},
    {"cg_ablate", &PsOptions::cg_ablate, PS_OPT_INT, 0, 0, PS_ABLATION_REFUSAL("cg_ablate"), 0, true},
    {"schur_ablate", &PsOptions::schur_ablate, PS_OPT_INT, 0, 0, PS_ABLATION_REFUSAL("schur_ablate"), 0, true},
    {"lm_ablate", &PsOptions::lm_ablate, PS_OPT_INT, 0, 0, PS_ABLATION_REFUSAL("lm_ablate"), 0, true},
    {"schur_pipeline", &PsOptions::schur_pipeline, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"coarse_lag", &PsOptions::coarse_lag, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"cg_force_restart", &PsOptions::cg_force_restart, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"cg_force_breakdown", &PsOptions::cg_force_breakdown, PS_OPT_INT, 0, 0, nullptr, 0, false},
    {"xcg_restrict_fused", &PsOptions::xcg_rt, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"band_chol", &PsOptions::band_chol, PS_OPT_BOOL, 0, 0, nullptr, PS_FX_DROP_FACTOR, false},
    {"lm_packed", &PsOptions::lm_packed, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"pose_xcd", &PsOptions::pose_xcd, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"fuse_cost", &PsOptions::fuse_cost, PS_OPT_INT, 0, 0, nullptr, 0, false},
    {"sync_refactor", &PsOptions::sync_refactor, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"hold_across_steps", &PsOptions::hold_across_steps, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"band_part", &PsOptions::band_part, PS_OPT_BOOL, 0, 0, nullptr, PS_FX_DROP_FACTOR, false},
    {"band_part_chunk", &PsOptions::band_part_m, PS_OPT_RANGE, 0, 4096, "band_part_chunk must be 0 (automatic) .. 4096 nodes", PS_FX_DROP_FACTOR, false},
    {"coarse_auto_hold", &PsOptions::xcg_auto_hold, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"coarse_adaptive_hold", &PsOptions::xcg_adaptive_hold, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"xcg_fused", &PsOptions::xcg_fused, PS_OPT_EXACT, 0, 2, "xcg_fused must be 0, 1 or 2", 0, false},
    {"lagged_inverse", &PsOptions::ldi_enable, PS_OPT_BOOL, 0, 0, nullptr, PS_FX_LDI_OFF | PS_FX_RELOOK_PATH, false},
    {"ldi_max_unknowns", &PsOptions::ldi_max_n, PS_OPT_RANGE, 0, PS_LDI_MAXN, "ldi_max_unknowns out of range (0 .. 3328)", PS_FX_RELOOK_PATH, false},
    {"ldi_cap", &PsOptions::ldi_cap, PS_OPT_RANGE, 1, 64, "ldi_cap out of range (1 .. 64)", 0, false},
    {"ldi_cost_tol", nullptr, PS_OPT_COST_TOL, 0, INFINITY, "ldi_cost_tol must be >= 0", 0, false},
    {"ldi_refresh_its", &PsOptions::ldi_refresh_its, PS_OPT_RANGE, 0, 64, "ldi_refresh_its out of range (0 .. 64)", 0, false},
    {"ldi_direct", nullptr, PS_OPT_LDI_DIRECT, 0, 0, nullptr, 0, false},
    {"direct_fused", &PsOptions::direct_fused, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"ldi_seed_lag", &PsOptions::ldi_seed_lag, PS_OPT_RANGE, 1, 16, "ldi_seed_lag out of range (1 .. 16)", 0, false},
    {"ldi_seed_steps", &PsOptions::ldi_seed_steps, PS_OPT_RANGE, 1, 40, "ldi_seed_steps out of range (1 .. 40)", 0, false},
    {"coarse_refresh_every", &PsOptions::xcg_refresh_every, PS_OPT_RANGE, 1, 16, "coarse_refresh_every must be 1..16", 0, false},
    {"coarse_lag_x", &PsOptions::lagx, PS_OPT_BOOL, 0, 0, nullptr, PS_FX_DROP_FACTOR | PS_FX_DROP_SIDE, false},
    {"cg_lds", &PsOptions::cg_lds, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"cg_persist", &PsOptions::cg_persist, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"xcg_persist", &PsOptions::xcg_persist, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"cg_persist_spin", nullptr, PS_OPT_SPIN, 0, 1e7, "cg_persist_spin out of range", 0, false},
    {"cg_explicit", &PsOptions::explicit_ok, PS_OPT_BOOL, 0, 0, nullptr, PS_FX_COARSE_REBUILD, false},
    {"big_chol", &PsOptions::big_chol, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"fused_motion_only", &PsOptions::mo_fused, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
    {"direct_max_unknowns", &PsOptions::direct_max, PS_OPT_RANGE, 0, 90, "direct_max_unknowns must be 0..90", 0, false},
    {"coarse_basis", &PsOptions::coarse_basis, PS_OPT_BOOL, 0, 0, nullptr, PS_FX_DROP_FACTOR | PS_FX_DROP_SIDE, false},
    {"profile_every", &PsOptions::prof_every, PS_OPT_RANGE, 1, INFINITY, "profile_every must be >= 1", 0, false},
    {"cg_margin", &PsOptions::cg_margin, PS_OPT_RANGE, 0, 64, "cg_margin out of range", 0, false},
    {"cg_split_min_rows", &PsOptions::cg_split_min_rows, PS_OPT_INT, 0, 0, nullptr, PS_FX_COARSE_REBUILD, false},
    {"cg_explicit_min_rows", &PsOptions::cg_explicit_min_rows, PS_OPT_INT, 0, 0, nullptr, PS_FX_COARSE_REBUILD, false},
    {"pcg_chunk", &PsOptions::pcg_chunk, PS_OPT_RANGE, 1, 4096, "pcg_chunk out of range", 0, false},
    {"lin_zero_list", &PsOptions::lin_zero_list, PS_OPT_BOOL, 0, 0, nullptr, 0, false},
};
constexpr int PS_NUM_OPTIONS = (int)(sizeof(PS_OPTION_TABLE) / sizeof(PS_OPTION_TABLE[0]));

inline const PsOptionRow* ps_option_find(const char* name) {
    for (const PsOptionRow& r : PS_OPTION_TABLE)
        if (!std::strcmp(r.name, name)) return &r;
    return nullptr;
}

// (name, value) onto o.  -> the row's effects mask when the value was stored; PS_OPT_REFUSED with the row's words in *refusal
// (o untouched); PS_OPT_UNKNOWN: no such option
constexpr int PS_OPT_UNKNOWN = -1, PS_OPT_REFUSED = -2;
inline int ps_option_apply(PsOptions& o, const char* name, double value, const char** refusal) {
    const PsOptionRow* r = ps_option_find(name);
    if (!r) return PS_OPT_UNKNOWN;
    bool ok = true;
    if (r->measure_only && !PS_MEASURE_BUILD) ok = value == 0.0;
    else switch (r->kind) {
    case PS_OPT_BOOL: o.*r->member = value != 0; break;
    case PS_OPT_INT: o.*r->member = (int)value; break;
    case PS_OPT_RANGE: if ((ok = !(value < r->lo || value > r->hi))) o.*r->member = (int)value; break;
    case PS_OPT_BELOW: if ((ok = !(value < r->lo || value >= r->hi))) o.*r->member = (int)value; break;
    case PS_OPT_EXACT: if ((ok = value >= r->lo && value <= r->hi && value == std::floor(value))) o.*r->member = (int)value; break;
    case PS_OPT_SPIN: if ((ok = !(value < r->lo || value > r->hi))) o.cp_spin = (unsigned)value; break;
    case PS_OPT_COST_TOL: if ((ok = value >= r->lo)) o.ldi_cost_tol = value; break;
    case PS_OPT_LDI_DIRECT: o.ldi_direct_ok = value != 0.0; o.ldi_direct = value > 0.0; break;
    }
    if (!ok) { *refusal = r->refusal; return PS_OPT_REFUSED; }
    return (int)r->effects;
}
