// ps_core.hip -- host side of the C ABI declared in include/pyslam_hip.h:
// table upload, iteration-invariant structure (segment / pair / block lists),
// kernel sequencing on one HIP stream, hipEvent stage timers.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared \
//              -Iinclude pyslam_amd/csrc/ps_core.hip -o pyslam_amd/lib/libpyslam_hip.so
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <map>
#include <atomic>
#include <chrono>
#include <thread>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "pyslam_hip.h"
#include "ps_kernels.h"
#include "ps_ransac_core.h"
#include "ps_ransac.h"
#include "ps_k_twoview.h"
#include "ps_k_pnp.h"
#include "ps_k_sim3.h"
#include "ps_k_sim3pg.h"
#include "ps_photo.h"
#include "ps_k_dense.h"
#include "ps_k_feat.h"
#include "ps_k_feat_global.h"
#include "ps_k_feat_db.h"
#include "ps_sparse.h"
#include "ps_k_covmarg.h"
#include "ps_k_triang.h"

namespace {

// Environment switches.  ps_create_env: variants chosen when a handle is CREATED (which Schur lists are built, tile sizes: the
// parity tests hold the variants against each other) -- read once per ps_problem_create, never inside an iteration.
// ps_env: measurement and debugging switches (timing printouts, ablations, allocation guards, launch-shape experiments);
// compiled out of the product library -- they exist only in the -DPS_MEASURE build (__graft_entry__.build_measure(),
// lib/libpyslam_hip_measure.so, loaded when PYSLAM_AMD_MEASURE=1), which tools/ use.
inline const char* ps_create_env(const char* name) { return getenv(name); }
#ifdef PS_MEASURE
inline const char* ps_env(const char* name) { return getenv(name); }
#else
inline const char* ps_env(const char*) { return nullptr; }
#endif

thread_local std::string g_err;

int fail(const std::string& msg) { g_err = msg; return -1; }

#define HIP_OK(expr)                                                                   \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- process-wide cache of the fixed-cost resources of a handle -----------------------------------------------
// A per-frame Problem (reference pipelines/sparse.py:153-161: a fresh Problem for every image pair) creates and
// destroys a handle per solve; for a 45 us iteration the ~30 hipMalloc + hipMemcpy pairs, five hipHostMalloc and a
// hipStreamCreate of ps_problem_create (0.65-0.70 ms) were the latency the user saw.  So:
//   * tables of up to PS_ARENA_SMALL bytes are carved from ONE device block per handle ("arena") and staged in a pinned
//     mirror; ps_problem_create ends with a single asynchronous copy of the used part (big tables keep hipMalloc);
//   * the pinned, host-mapped result words of a handle live in one 4 KB block;
//   * arena blocks, mirrors, word blocks and streams of destroyed handles are kept (up to PS_POOL_KEEP each) and handed
//     to the next ps_problem_create.
constexpr size_t PS_ARENA_BYTES = 2u << 20, PS_ARENA_SMALL = 192u << 10, PS_WORDS_BYTES = 4096, PS_MO_HIST_WORDS = 256;
constexpr size_t PS_POOL_KEEP = 8;
struct PsPool {
    std::mutex mu;
    std::vector<void*> dev_arenas, host_arenas, host_words;
    std::vector<hipStream_t> streams;
    std::vector<hipStream_t> side_streams;     // ordinary non-blocking streams (side / lagged-inverse work)
    template <typename T> bool take(std::vector<T>& v, T* out) {
        std::lock_guard<std::mutex> lk(mu);
        if (v.empty()) return false;
        *out = v.back(); v.pop_back(); return true;
    }
    template <typename T> bool give(std::vector<T>& v, T x) {      // false: the pool is full, the caller frees
        std::lock_guard<std::mutex> lk(mu);
        if (v.size() >= PS_POOL_KEEP) return false;
        v.push_back(x); return true;
    }
};
// Events that order the solver stream against the side stream (and back).  PS_EVENT_FLAGS=<int> overrides the creation flags
// (debugging); see DESIGN.md section 3 "cross-stream visibility".
inline unsigned ps_xstream_event_flags() {
    static const unsigned f = ps_env("PS_EVENT_FLAGS") ? (unsigned)strtoul(ps_env("PS_EVENT_FLAGS"), nullptr, 0)
                                                       : (unsigned)(hipEventDisableTiming | hipEventReleaseToSystem);
    return f;
}
#define PS_XSTREAM_EVENT_FLAGS ps_xstream_event_flags()

// Dynamic LDS beyond 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize, and that attribute belongs to the KERNEL, not to
// a handle: with per-handle "already set" flags a second, smaller problem lowered the limit under a live bigger one, whose
// next launch then failed without a trace.  One process-wide high-water mark per kernel instead.
inline int ensure_dynamic_lds(const void* func, size_t bytes) {
    static std::mutex mu;
    static std::map<const void*, size_t> high;
    std::lock_guard<std::mutex> lock(mu);
    size_t& cur = high[func];
    if (bytes > cur) {
        HIP_OK(hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        cur = bytes;
    }
    return 0;
}

PsPool& ps_pool() { static PsPool* p = new PsPool(); return *p; }   // (leaked on purpose: no destructor order issues at exit)

// ---- co-residency of the one-launch solvers (k_cg_persist, k_xcg_persist) ------------------------------------------------
// Their workgroups wait for one another INSIDE the launch, in an ordinary (non-cooperative) launch: the whole grid must be
// resident at once or the first arrivals spin until the time-out.  Nothing may be left to a literal there (round-5 verdict,
// ADVICE): the compute units the solver's stream may use come from the device (hipDeviceAttributeMultiprocessorCount: a CPX /
// DPX partition reports its own count) and from the stream's CU mask (hipExtStreamCreateWithCUMask; without one
// hipExtStreamGetCUMask returns ROC_GLOBAL_CU_MASK or all units); workgroups per unit from
// hipOccupancyMaxActiveBlocksPerMultiprocessor of the very instantiation; and the units that launches of OTHER handles of this
// process hold at the same time come off a process-wide ledger per device (reserved when a solve is enqueued, released when
// the host has seen its end).  A form that cannot be resident is refused up front -- the launch-per-iteration kernels run --
// instead of being found out by a 20 ms stall.  What the ledger cannot see (another PROCESS on the same device, HSA_CU_MASK
// applied below HIP) is still answered by the bounded spins.
struct CuBudget { int cus = 0; bool masked = false; };
inline CuBudget ps_stream_cus(hipStream_t st) {
    CuBudget b;
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) { (void)hipGetLastError(); return b; }
    b.cus = ncu;
    uint32_t mask[64] = {};
    const uint32_t words = (uint32_t)std::min(64, (ncu + 31) / 32);
    if (hipExtStreamGetCUMask(st, words, mask) == hipSuccess) {
        int c = 0;
        for (int i = 0; i < ncu && i < 64 * 32; ++i) c += (mask[i >> 5] >> (i & 31)) & 1u;
        if (c > 0 && c < ncu) { b.cus = c; b.masked = true; }
    } else (void)hipGetLastError();
    // a mask applied below HIP (ROCr) is invisible here: nothing can be promised
    if (const char* e = getenv("HSA_CU_MASK")) { if (*e) { b.cus = 0; b.masked = true; } }
    return b;
}
struct PersistLedger {
    std::mutex mu;
    int held[64] = {};             // compute units held by one-launch solves in flight, per device
    bool reserve(int dev, int need, int capacity) {
        if (dev < 0 || dev >= 64) return false;
        std::lock_guard<std::mutex> lk(mu);
        if (held[dev] + need > capacity) return false;
        held[dev] += need; return true;
    }
    void release(int dev, int n) { if (dev < 0 || dev >= 64 || n <= 0) return; std::lock_guard<std::mutex> lk(mu); held[dev] = std::max(0, held[dev] - n); }
};
PersistLedger& ps_persist_ledger() { static PersistLedger* p = new PersistLedger(); return *p; }

}  // namespace

#include "ps_host_devmem.h"
#include "ps_host_bandpart.h"
#include "ps_host_bchol.h"
#include "ps_options.h"
#include "ps_coarse_band.h"
#include "ps_structure.h"

// ---- the handle by role -------------------------------------------------------------------------------------------------
// ps_problem derives from three plain structs so that the struct itself says what a member is: a user option (PsOptions,
// ps_options.h), what one whole-iteration call hands to the next (PsCostHistory, PsCarried: ps_reset_solver_state assigns
// fresh ones), and everything else -- tables and structures built at create time or by build_coarse, counters, timers, plumbing
// ("The handle": why a reset leaves each of those alone).

// costs the whole-iteration calls returned, and what the caller's stopping rule still allows: reset even on a handle that has
// not linearised anything since the last reset
struct PsCostHistory {
    double last_cost = -1.0, prev_cost = -1.0;   // costs returned by the last two ps_gn_iteration calls (-1: none / parameters replaced since)
    double snap_cost = -1.0;        // last_cost at the time of ps_snapshot_params
    // option "solve_horizon" (the one option outside PsOptions): how many MORE whole-iteration calls the caller's stopping rule allows if the step about to be
    // taken does not decrease the cost enough (reference problem.py:163-178: max_nondecreasing_steps - taken - 1, or 0 without
    // allow_nondecreasing_steps); -1 = unknown (a caller that drives ps_gn_iteration itself).  Side work that only pays back
    // over several later calls -- the seed of the lagged dense inverse -- is not started when the solve is about to stop.
    int solve_horizon = -1;
};

// what the solver carries from one whole-iteration call to the next.  A member that is added here is reset with the rest; the
// initialisers ARE the reset values
struct PsCarried {
    // lagged coarse level (folded and explicit forms)
    int lci_cur = 0;                // buffer the current augmented system was built with
    int lci_next = -1;              // buffer holding (or receiving, see side_pending) the newest factor; -1: none
    bool side_todo = false;         // the next X (from SB / the basis in buffer side_buf) is still to be formed on the side stream
    bool side_ready = false;        // the host has synchronised with the solver stream since the side stream's inputs were enqueued
    bool side_pending = false;      // a side-stream factorisation is in flight: wait for ev_chol before reuse
    bool acdone_pending = false;    // explicit PCG: the side stream may still be assembling A_c from SB / the basis (wait before they are overwritten)
    bool xcg_side_todo = false;     // explicit PCG: lagged setup whose side-stream half is not enqueued yet
    long xcg_lag_count = 0;         // lagged set-ups since the last refresh ("coarse_refresh_every")
    int xcg_held = 0;               // set-ups in a row that kept the inverse ("coarse_auto_hold")
    int xcg_its_ref = 0, xcg_good_held = 0;   // CG iterations of the first solve with the inverse in use / set-ups it has been kept for
    bool xcg_ref_pending = false;
    double xcg_tag[2] = {-1.0, -1.0}, xcg_setup_cost = -1.0;   // start cost of the call whose A_c each inverse buffer was formed from
    double xcg_tag_lambda[2] = {0.0, 0.0}, xcg_setup_lambda = 0.0;
    bool mc_active = false;         // the current system was built with a lagged factor in split mode
    bool last_setup_lagx = false;   // the current folded system was built with the lagged X~ (three-launch set-up)
    int xf_skip = 0;                // upcoming set-ups that must not use the one-launch form (a fallback after its breakdown)
    int cg_break_at = 0;            // test hook "cg_force_breakdown" as THIS pass took it (cg_break_arm): the launch index whose delta is forced, 0 none
    // lagged dense inverse
    int ldi_state = 0;              // 0 none, 1 seed in flight, 2 valid (ldi_cur), 3 valid + update in flight
    int ldi_cur = -1, ldi_next = -1;
    long ldi_iter = 0, ldi_ready_at = 0;
    bool ldi_side_todo = false, ldi_update_ok = false, ldi_sread_pending = false;
    int ldi_last_its = 0, ldi_prev_its = 0;
    int ldi_rejects = 0; long ldi_no_seed_before = 0;
    double ldi_tag = -1.0, ldi_next_tag = -1.0, ldi_call_start_cost = -1.0;   // cost at the point the inverse in use / in flight was built at
    double ldi_prev_start_cost = -2.0;   // cost the previous standard-path call started from
    bool ldi_moved = false;         // this call left the lagged inverse behind (cost jump): the standard solve's launch-count prediction is stale
    // launch-count predictions
    int last_pcg_iters = 0;
    int prev_pcg_iters = -1;        // iteration count of the solve before the last one
};

struct ps_problem : PsOptions, PsCostHistory, PsCarried {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int D = 6, PW = 12;
    int P = 0, nr = 0, L = 0, nv = 0;
    long N = 0, Nl = 0, Np = 0;     // observations: all / on variable points / on variable poses
    long F = 0;                     // pose factors (edges + priors)
    long FH = 0;                    // host rows (ps_problem_create_hybrid): pose factors after the F in fscratch, values from the caller
    bool hybrid = false;            // made by ps_problem_create_hybrid: the core's cost passes do not see every block
    double host_cost = 0.0;         // the caller's cost at the point of its last ps_set_host_rows
    long npairs = 0;
    int nnzb = 0;
    size_t dev_bytes = 0;
    std::vector<void*> allocs;
    // PS_ALLOC_GUARD=1 (debugging): every hipMalloc'd table is followed by 4 KB of 0xA5; check_guards() names the table
    // whose guard a kernel has written into
    struct Guard { char* guard; size_t table_bytes; int serial; };
    std::vector<Guard> guards;
    int check_guards(const char* where) {
        int bad = 0;
        std::vector<unsigned char> g(4096);
        for (const Guard& gd : guards) {
            if (hipMemcpy(g.data(), gd.guard, 4096, hipMemcpyDeviceToHost) != hipSuccess) return -1;
            for (int i = 0; i < 4096; ++i) if (g[i] != 0xA5) {
                fprintf(stderr, "GUARD %p %s: table #%d (%zu bytes) overrun at +%d (byte %02x)\n", (void*)this, where, gd.serial, gd.table_bytes, i, g[i]);
                ++bad; break;
            }
        }
        return bad;
    }

    // parameter tables
    double *poses = nullptr, *points = nullptr, *poses_snap = nullptr, *points_snap = nullptr;
    int32_t *pose_rid = nullptr, *point_vid = nullptr;
    // reprojection
    ObsGroup* ogroups = nullptr;
    // "wide" problems (more than 255 (camera, stiffness, loss) rows): per-observation stiffness index columns in landmark /
    // pose order + the stiffness table; the 8-bit group field then holds the (camera, loss) class
    bool wide_obs = false;
    int32_t *sidx_l = nullptr, *sidx_p = nullptr;
    double* stiff_tab = nullptr;
    LObs* lobs = nullptr;
    int32_t *lorig = nullptr, *lm_ptr = nullptr, *lm_point = nullptr;
    double *Z = nullptr, *Cinv = nullptr, *cvec = nullptr, *dxl = nullptr;
    LObs* pobs = nullptr;           // observation records in pose-sorted order (landmark slot + 1 in the pose bits)
    PItem* pitems = nullptr;
    int npitems = 0;
    int32_t* pitem_ptr = nullptr;
    double* ppartial = nullptr;
    int2* pairs = nullptr;
    int npair_items = 0, pair_per_xcd = 0;
    PairItem* pair_xitems = nullptr;   // work items in per-XCD dispatch order
    // tiled Schur (Z larger than the L2s): per-task partial blocks + per-block task lists
    int schur_tiles = 1, ncomb = 0;
    bool has_diag_tasks = false;    // some landmark is observed twice from one pose: a pair task writes a diagonal block
    double* Spart = nullptr;
    PairItem* comb_items = nullptr;     // slot, slotT, [start, end) into comb_tasks
    int32_t* comb_tasks = nullptr;
    // factors
    FactorGroup* fgroups = nullptr;
    int32_t *f_i = nullptr, *f_j = nullptr, *f_grp = nullptr;
    double *f_Tinv = nullptr, *fscratch = nullptr;
    int32_t *eslots = nullptr, *eptr = nullptr, *eslot_diag = nullptr, *gptr = nullptr, *gitems = nullptr;
    int2* eitems = nullptr;
    int nes = 0;
    // reduced system
    int32_t *row_ptr = nullptr, *col_idx = nullptr, *diag_slot = nullptr;
    double* red = nullptr;          // [S (nnzb*D*D) | g (nr*D) | cost]
    long red_count = 0;
    double *S = nullptr, *g = nullptr;
    // option "lin_zero_list": the slots of S that a linearisation ACCUMULATES into (diagonal blocks, blocks a factor or a host
    // row adds into, blocks of the pattern no pair item writes); every other slot is stored with `=` by exactly one pair item
    // of the untiled pair kernel and needs no zero in front.  Trailing workgroups of the pose pass zero these, g, the cost
    // words and the status words in place of the fill over all of [S | g | cost | status] (ps_host_cg.h: linearize)
    int32_t* zero_slots = nullptr;
    int nzero_slots = 0;
    bool has_extra_pairs = false;   // created with extra pattern blocks: a landmark shard (pyslam_amd/distributed.py)
    bool lin_zero_gate = false;     // the option is on and this handle is eligible (relook_launch_gates)
    long lin_fills = 0, lin_zero_launches = 0;   // linearisations that ran the fill / that zeroed by the list
    // option "setup_ride" (ps_set_option, ahead of the table): the block-Jacobi factor kernel that heads the fused CG's set-up
    // rides in a launch that is there anyway -- the factor of a pose is formed by the wave of the pair launch that has just finalised
    // its diagonal block (ride_gate: the handle is eligible, relook_launch_gates; ride_valid: Linv, g^, the zeroed CG vectors and the
    // basis blocks in ride_basis belong to the S and g on the device -- set by linearize(), consumed by the first set-up, cleared
    // by whatever changes S, g, the parameters or an option in between; ride_lagged / ride_use / ride_basis: the set-up plan the
    // ridden factor was run for, cg_setup_plan).
    int setup_ride = 1;
    bool ride_gate = false, ride_valid = false, ride_lagged = false;
    int ride_use = 0;
    double* ride_basis = nullptr;
    long bjf_launches = 0, bjf_ridden = 0, bjf_mismatches = 0;   // factor launches of the fused CG's set-up / linearisations that rode the factor / ridden for another plan than the set-up's
    std::vector<int32_t> h_row_ptr, h_col_idx;
    std::vector<int32_t> h_vid_of_slot;   // landmarks are stored in locality order; external order is vid
    // pcg
    double *x = nullptr, *r = nullptr, *z = nullptr, *p0 = nullptr, *p1 = nullptr, *q = nullptr, *Minv = nullptr;
    double *rz_part = nullptr, *rr_part = nullptr, *pq_part = nullptr, *hist = nullptr;
    int npartA = 0, npartB = 0, hist_cap = 0;
    // fused CG (one launch per iteration) on the block-Jacobi-scaled system
    double *Linv = nullptr, *cg_r[2] = {}, *cg_w[2] = {}, *cg_s[2] = {}, *cg_gd[2] = {}, *cg_xh = nullptr;
    int32_t* brow_of = nullptr;
    double* cg_p = nullptr;
    double* Saug = nullptr;         // scaled (and, with a coarse level, augmented) matrix the CG runs on
    int32_t* ident_slot = nullptr;
    // two-level preconditioner (coarse level), built lazily by build_coarse()
    int G = 0, ncb = 0, nc = 0, nr_aug = 0, nnzb_aug = 0;
    size_t cg_cap = 0, saug_cap = 0; // CG vectors / matrix are allocated for this many block rows / blocks
    int32_t *pnode = nullptr, *slo = nullptr, *shi = nullptr, *run_lo = nullptr, *run_hi = nullptr,
            *arow_ptr = nullptr, *acol_idx = nullptr, *aug_slot = nullptr, *fine_nnz = nullptr;
    double *pw0 = nullptr, *pw1 = nullptr, *SZ = nullptr, *Ac = nullptr, *tvec = nullptr, *chol_scratch = nullptr;
    // coarse basis P_iq = w(i,q) B_i: B_i = L_i^T Ad(T_i) (coarse_basis 1, rigid-motion aware) or I (0)
    double *Bmat = nullptr, *bgv = nullptr, *SB = nullptr, *BSZ = nullptr;   // Bmat: the basis the CURRENT system was built with
    // lagged three-launch setup (k_rows_setup): basis blocks and X = P L_c^-T double-buffered with the coarse factor
    double *Bmat2[2] = {}, *X2[2] = {}, *Mpart = nullptr;
    bool lagx_ok = false;           // the problem's shape allows it (folded, not split, nc <= 96, rows <= PS_RS_MAXROW blocks)
    int side_buf = 0;               // (PsCarried::side_todo: the buffer the next X is formed from)
    double host_wait_ns = 0.0, host_call_ns = 0.0;   // PS_HOST_TIMING
    long host_waits = 0, host_calls = 0;
    size_t rows_lds = 0;
    int rows_attr_set = 0;          // bit m: the dynamic-LDS attribute of k_rows_setup<D, m> covers rows_lds
    bool rows_lci_lds = false;
    // option "rows_regs" (ps_set_option, ahead of the table): the scaled-block products of the set-up by one thread per block
    // row in registers (scaled_block_row) -- k_rows_setup<D, PS_RS_REGS>, which also forms K_i only over the coarse nodes of
    // the row; and, where lagx_ok, the exact set-up's k_scale_blocks + k_coarse_rowsums as ONE launch of the rows kernel
    // (PS_RS_EXACT).  0: the wave-per-block form and the two launches.  Every value is the same either way.
    int rows_regs = 1;
    long rows_setups = 0, exact_row_setups = 0;      // lagged set-ups launched / exact set-ups headed by the rows kernel
    int32_t *ent_ptr = nullptr, *ent_q = nullptr, *ent_lo = nullptr, *ent_hi = nullptr;   // explicit PCG: non-empty (row, node) runs
    int32_t *seg_ptr = nullptr, *seg_ent = nullptr, *seg_row = nullptr;                     // ... grouped by (node, node') for A_c
    int max_row_ents = 0;
    int32_t* pose_of_rid = nullptr;
    // coarse factor L_c^-1 (and transpose), double-buffered: with "coarse_lag" the factorisation of THIS
    // iteration's A_c runs on a side stream while the CG iterates with the previous iteration's factor
    double *Lci2[2] = {}, *LciT2[2] = {};
    hipStream_t side = nullptr;
    int side_cus = 0;               // > 0: the side stream is confined to this many compute units (CU mask)
    hipEvent_t ev_ac = nullptr, ev_chol = nullptr, ev_acdone = nullptr;
    // PS_XCG_AC_CHECK (measurement build, tools/probes/lowprio_hunt.sh): A_c / BSZ assembled a second time on the solver stream and
    // compared bit for bit with what the side stream assembled: [entries of A_c that differ, of BSZ, comparisons]
    unsigned long long* chk_sums = nullptr; int chk_nsum = 0;      // PS_XCG_INV_SUM: bit checksums (pinned) of [inverse consumed | A_c the side job factored | inverse it produced] per set-up
    double *chk_Ac = nullptr, *chk_BSZ = nullptr, *chk_Ac_side = nullptr; int32_t* chk_cnt = nullptr; size_t chk_bsz_n = 0;
    int32_t* lag_status = nullptr;  // ST_DIAG_FAIL of the side-stream factorisation
    double* Mc = nullptr;           // split mode: dense coarse-coarse block M of the lagged system
    bool coarse_built = false;
    bool coarse_clamped = false;    // the automatic coarse level was cut back to 255 nodes: its matrix is not banded
    int max_pose_obs = 0;           // most observations on one variable pose
    double* mo_partials = nullptr;
    bool status_clean = true;       // no failure flag can be pending in the device status words
    double *dA = nullptr, *dLi = nullptr, *dLiT = nullptr;
    // explicit two-level PCG (long sparse chains)
    bool cg_explicit = false;
    double lin_lambda = 0.0;        // damping of the last linearisation
    double *xstate = nullptr, *xy = nullptr, *xp2 = nullptr;
    // ... banded coarse matrix (ps_k_band.h): block off-diagonals of A_c (-1: not banded enough), band factor by rows / columns
    int ac_bw = -1;
    std::unique_ptr<BandPart> bpart;
    double *Lrow = nullptr, *Lcol = nullptr, *rdiag = nullptr;
    // ... three-launch form (restriction folded into the SpMV epilogue + a recurrence for t)
    bool xcg_rt_ok = false;         // every SpMV workgroup touches at most PS_XCG_NSLOT coarse nodes
    int xcg_rt_rows = PS_XCG_ROWS_RT;
    int32_t *xcg_wg_out = nullptr, *xcg_nptr = nullptr;
    double *tq_part = nullptr, *tvec2 = nullptr;
    // ... one-launch form (k_xcg_fused1)
    bool xf_ok = false, xf_active = false;
    bool xf_one_ok = false, xf_two = false;   // the one-launch form fits (nc <= 2 048, even) / this solve runs the two-launch form
    int32_t *xf_cptr = nullptr, *xf_cols = nullptr, *xf_nlo = nullptr, *xf_nhi = nullptr, *xf_rec = nullptr;
    uint16_t* xf_lidx = nullptr;
    double *xf_tq[2] = {}, *xf_ts[2] = {}, *xf_t[2] = {};
    int xf_rmax = 1, xf_nwg = 0, xf_pf = 2;
    size_t xf_nrec = 0;
    long xf_solves = 0, xf_fallbacks = 0;
    // the folded CG in ONE launch (ps_k_cg_persist.h): option "cg_persist"; task table built with the coarse level
    bool cp_ok = false;             // the augmented system fits the kernel's layout
    bool cp_recovered = false;      // the launch just enqueued recovers x itself when it converges
    int cp_ntasks = 0, cg_max_launches = 0;
    void* cp_tasks = nullptr;       // CpTask[cp_ntasks]
    int32_t* cp_row_task0 = nullptr;
    unsigned long long* cp_exch = nullptr;
    unsigned cp_salt = 0;
    long cp_launches = 0, cp_failures = 0;
    // options "cg_persist_recover" / "cg_persist_recover_lds" (ps_set_option, ahead of the table): the recovery x = L^-T (x^_f + P y)
    // inside the launch, every workgroup its own slice of poses with the operands prefetched into LDS (ps_k_cg_persist.h), when
    // the largest slice's operands fit the cap; else, and with 0, the gated k_coarse_recover behind the launch.  Same bits either way.
    int cg_persist_recover = 1;
    int cg_persist_recover_lds = PS_CP_RECOVER_LDS_CAP;
    int cp_rec_pp = 0, cp_rec_cols = 0;         // poses per workgroup's slice; most columns of L_c^-1 a slice's nodes select
    size_t cp_rec_lds = 0;                      // dynamic LDS the largest slice needs (0: no slices -- pnode is not ascending)
    long cp_rec_inside = 0, cp_rec_behind = 0;  // launches that recover in the launch / that leave it to k_coarse_recover
    // co-residency (ps_stream_cus / PersistLedger above): what build_coarse found, what a solve in flight holds
    int persist_dev = 0, persist_cus = 0;       // device of the handle; compute units its stream may use (0: unknown -> no one-launch form)
    bool persist_masked = false;                // ... fewer than the device has (a CU mask)
    int cp_cus_needed = 0, xp_cus_needed = 0;   // compute units the one-launch folded CG / explicit PCG need resident
    int persist_held = 0;                       // units this handle holds on the ledger (released when the host has seen the solve's end)
    // Z, C^-1, c are rewritten by every landmark pass -- also by the one a tail runs AHEAD for its successor and by the pass that
    // sums ps_eval_cost's cost (fuse_cost): the staged entry points that read them (ps_backsub, ps_gn_finish, ps_gn_solve_finish*,
    // ps_get_landmark_factors) belong to the last ps_linearize and refuse when the buffers have since been rewritten at another point
    bool params_moved_since_lin = false;        // a tail / update / upload / restore since the last linearize()
    bool z_foreign = false;                     // ... and a landmark pass ran at the moved point (or under another damping)
    bool no_repeat = false;                     // the caller drives the collectives itself and cannot repeat a solve: no form that may time out
    long cp_refused = 0;                        // solves that wanted a one-launch form and ran launch by launch instead (not resident)
    void persist_release() { if (persist_held) { ps_persist_ledger().release(persist_dev, persist_held); persist_held = 0; } }
    // compute units a one-launch solve may count on: all of the stream's when it has the whole device; half of a masked stream's
    // (workgroups go to the XCDs round-robin whatever the mask leaves of each: an uneven mask fills one XCD first)
    int persist_capacity() const { return persist_masked ? persist_cus / 2 : persist_cus; }
    bool persist_reserve(int need) {
        if (need <= 0 || persist_cus <= 0) return false;
        if (persist_held) return true;          // (a second round of launches of the same solve: already held)
        if (!ps_persist_ledger().reserve(persist_dev, need, persist_capacity())) { ++cp_refused; return false; }
        persist_held = need; return true;
    }
    // the explicit two-level PCG's one-launch-per-iteration form as one launch per solve (ps_k_xcg_persist.h): option "xcg_persist"
    bool xp_ok = false;             // every workgroup resident at once, at most PS_XP_RB records per node
    int32_t* xf_cnt = nullptr;      // live records per coarse node
    unsigned long long* xp_exch = nullptr;
    size_t xp_words = 0;
    unsigned xp_salt = 0;
    bool xp_defer = false;          // xcg_setup left launch -1 to the one launch that runs them all
    long long* cp_dbg = nullptr;    // measurement build, PS_CP_CLOCKS: phase clocks of the kernel's first workgroup
    long long* xp_dbg = nullptr;    // measurement build, PS_XP_CLOCKS: phase clocks of three workgroups of k_xcg_persist
    long prof_tick = 0;             // linearisations so far ("profile_every" times every n-th)
    int cg_fallbacks = 0;           // solves repeated with the classic PCG after a breakdown of the pipelined CG
    bool cg_two_level_reduce = false, cg_short_rows = false;
    double* cg_tot = nullptr;
    // split mode (large systems): coarse rows are owned by k_cg_reduce_split
    bool cg_split = false;
    bool xmin_auto_ldi = false;     // build_coarse chose the folded / explicit crossover assuming the lagged inverse applies (re-decided when that changes)
    double *cg_U = nullptr, *cg_cgd[2] = {}, *cg_ab = nullptr;
    int cg_launched = 0;            // CG launches enqueued since the last setup
    long cg_kernel_launches = 0;    // kernels enqueued for CG / PCG iterations since creation (ps_problem_info)
    bool cov_ready = false;         // ps_covariance_begin has linearised and set the reduced solver up; cleared by linearize()
    std::vector<int32_t> h_slot_of_vid;
    // batched marginals (ps_abi_cov.h): one device block [S -> Sigma (n^2) | L^-1 (n^2) | L^-T (n^2) | ...], allocated by the first
    // ps_covariance_marginals, freed by the next linearisation, ps_covariance_begin or destroy; Sigma is valid for cov_epoch only
    double* cov_buf = nullptr;
    double* cov_xbuf = nullptr;     // ps_covariance_cross_blocks' fixed pair buffer: allocated by its first call, freed by destroy
    long long cov_epoch = 0, cov_sigma_epoch = -1;
    double* tri_buf = nullptr;      // ps_triangulate's result block (tri_cap doubles): grown by a call that needs more, freed by destroy
    size_t tri_cap = 0;
    int ell_wf = 0, ell_wc = 0;     // two-class ELL widths of the CG matrix (0 = CSR)
    // scalars
    double *cost_partials = nullptr, *scalars = nullptr, *h_scalars = nullptr;
    int32_t *status = nullptr, *h_status = nullptr;
    double* h_scalars_dev = nullptr;     // device-side aliases of the pinned, host-mapped result words
    int32_t* h_status_dev = nullptr;
    double *h_shard = nullptr, *h_shard_dev = nullptr;   // host-mapped copy of shard_buf (sharded iteration)
    long long *h_seq = nullptr, *h_seq_dev = nullptr;   // sequence number stamped by the last k_reduce3 workgroup
    long long seq = 0;
    long long *h_setup = nullptr, *h_setup_dev = nullptr;   // stamped by the last kernel of a lagged set-up: the side stream's inputs are complete
    long long setup_seq = 0;
    int32_t* arrivals = nullptr;
    double *h_mo_hist = nullptr, *h_mo_hist_dev = nullptr;   // pinned: k_motion_only_solve's [entries, iterations, |dx|, cost history ...]
    int ncost_obs = 0, ncost_fac = 0;
    // native RCCL: function pointer + communicator handed over by the binding (ps_set_collective)
    typedef int (*allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
    allreduce_fn nccl_allreduce = nullptr;
    void* nccl_comm = nullptr;
    // segment exchange inside the core (round 6, ps_set_segment_exchange): ncclAllGather of [tail | this rank's elements of the packed
    // system], then every destination element summed over its contributors in RANK order (the same on every rank)
    typedef int (*allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
    allgather_fn seg_allgather = nullptr;
    int seg_world = 0;
    long seg_maxlen = 0, seg_nmine = 0, seg_ndst = 0;
    int32_t *seg_mine = nullptr, *seg_dst = nullptr, *seg_src_off = nullptr, *seg_src_ptr = nullptr;   // (the plan in 32 bits on the device: 12 B per element less to read)
    double *seg_in = nullptr, *seg_all = nullptr;
    // sharded exchange buffer [upper(S) | g | cost | flag] (k_shard_pack / k_shard_unpack), built on first use
    double* shard_pack = nullptr;
    int32_t *up_slot = nullptr, *upT_slot = nullptr;
    long nup = 0, pack_count = 0;
    double* shard_buf = nullptr;    // {cost, ||dx_point||^2} of this landmark shard, for the caller's all-reduce
    bool shard_out = false;         // k_reduce3 writes cost / ||dx_point||^2 there instead of into scalars
    double *sq_part_l = nullptr, *sq_part_p = nullptr;   // per-workgroup partials of ||dx_point||^2, ||dx_pose||^2
    // adaptive LM (ps_lm_iteration): the running call's tail also sums the model decrease (csrc/ps_k_lm.h); its partials
    bool lm_md = false;
    double *md_part_p = nullptr, *md_part_l = nullptr;
    int nmd_p = 0;
    int nsq_l = 0 /* partials allocated */, nsq_l16 = 0 /* workgroups of the 16-lane back-substitution */, nsq_p = 0;
    // landmark pass / back-substitution with the lanes packed by observation (ps_k_packed.h): the first landmark of every wave's run
    // (lmw_nwaves + 1 entries; 0 waves: the 16-lane kernels -- a track longer than 16 observations, or an unobserved landmark)
    int32_t* lmw_first = nullptr;
    int lmw_nwaves = 0;
    // option "packed_prefetch" (ps_set_option, ahead of the table): the packed kernels read their run from ONE 16-byte record per
    // wave (lmw_run: lmw_nwaves records, built beside lmw_first) and ask for their operands in four dependent trips instead of
    // seven (ps_k_packed.h: PF).  0: the load order they had before.  Every value is the same either way.
    LmwRun* lmw_run = nullptr;
    int packed_prefetch = 1;
    // option "pose_prefetch" (ps_set_option, ahead of the table): the pose pass asks for both observations of a thread, their gathers
    // and the group record up front and forms its 33 sums only at the end (ps_k_linearize.h: k_pose_pass_pf) -- under 128 VGPRs
    // without damping, four waves per SIMD: the items of C3 in one resident round instead of two.  It serves items of at most
    // PS_POSE_PF_OBS observations (pose_chunk: what create_pose_segments cut; larger only in the measurement build).  0, or a
    // larger chunk: k_pose_pass.  Every value is the same either way.
    int pose_prefetch = 1;
    int pose_chunk = 256;
    // option "coarse_chol_band" (ps_set_option, ahead of the table): coarse_factor's LDS branch (nc <= 90) launches
    // k_coarse_chol_band with the block half-bandwidth of A_c -- coarse_chol_bw: what build_coarse derived from the run tables
    // (ps_coarse_band.h; the explicit form: from its segment lists), ncb - 1 where the pattern has no band.  0: k_coarse_chol.
    // Every value is the same either way.
    int coarse_chol_band = 1;
    int coarse_chol_bw = 0;
    // lagged dense inverse of the reduced system as the CG preconditioner (ps_k_ldi.h / ps_host_ldi.h)
    bool ldi_ready = false;         // buffers allocated
    int ldi_n = 0, ldi_np = 0, ldi_kp = 0;
    float *ldi_S32 = nullptr, *ldi_X32 = nullptr, *ldi_R32 = nullptr, *ldi_T32 = nullptr, *ldi_Xt = nullptr, *ldi_XtT = nullptr;
    float* ldi_Xu[2] = {};          // unscaled inverse, double-buffered against the side stream
    double *ldi_x64 = nullptr, *ldi_Linv = nullptr, *ldi_r[2] = {}, *ldi_part = nullptr, *ldi_fro_part = nullptr;
    double *h_ldi_fro = nullptr, *h_ldi_fro_dev = nullptr;   // ||R||_F^2 of the side stream's last Newton-Schulz step (pinned)
    double ldi_fro_limit = 0.1;     // ||R||_F bound the seed / refresh in flight is accepted under
    int2* ldi_krange = nullptr;
    bool side_poolable = false;            // `side` is an ordinary non-blocking stream (no CU mask, no priority)
    hipStream_t ldi_stream = nullptr;      // the direct seed's own stream: ~100 launches that must not sit in front of the coarse operator on `side`
    double *ldi_A64 = nullptr, *ldi_Li = nullptr, *ldi_LiT = nullptr, *ldi_Tinv = nullptr; int32_t* ldi_stat = nullptr;
    float* ldi_coef = nullptr;      // device: seed scale c and the two Ritz values (k_ldi_ritz)
    long ldi_solves = 0, ldi_fallbacks = 0, ldi_seeds = 0;
    hipEvent_t ev_ldi = nullptr, ev_ldi_sread = nullptr;
    bool snap_valid = false;        // a snapshot has been taken and not consumed (ps_solve's final restore exchanges the tables)
    // speculative next linearisation (ps_solve): the call's tail stamps h_early when its reduced solve has converged; the host,
    // waiting for the end of the iteration, then enqueues the linearisation of the NEXT iteration behind the tail, and the next
    // ps_gn_iteration finds it done (prelin_valid) -- the GPU does not idle while the host ends one call and starts the next
    long long *h_early = nullptr, *h_early_dev = nullptr;
    long long early_seq = 0;
    bool spec_next = false, spec_enqueued = false, early_armed = false, prelin_valid = false;
    double prelin_lambda = 0.0;
    // The landmark pass of the NEXT linearisation in place of this iteration's cost pass (k_landmark_pass_packed<.., COST>,
    // gn_tail): option "expect_next" (ps_solve sets it per iteration; a caller's own loop may) says a successor is expected.
    // prelm_pending: the running tail carries such a pass (tag prelm_tag); prelm_valid: it ran (the tail was open) and the
    // parameters have not moved since -- linearize() then skips its landmark pass.  A landmark block that was not positive
    // definite there stamps h_lmfail[tag & 1] with the tag (two pinned words: consecutive passes cannot overwrite one another's
    // report before it is read); the call whose linearisation consumed the pass reports it (lmfail_check).
    bool prelm_pending = false, prelm_valid = false;
    double prelm_lambda = 0.0;
    long long prelm_tag = 0, prelm_seq = 0, lmfail_check = 0, lin_lmfail_tag = 0;
    long long *h_lmfail = nullptr, *h_lmfail_dev = nullptr;
    long prelm_used = 0;            // linearisations that skipped their landmark pass (ps_get_counters-style diagnostics)
    bool start_cost_pending = false; // the running whole-iteration call also evaluates the cost at its linearisation point (SC_STARTCOST)
    bool solver_touched = false;    // something has been linearised since creation / the last ps_reset_solver_state
    // profiling
    int profiling = 0;              // 0 off, 1 = iteration total + Schur kernel only, 2 = every stage
    std::vector<std::pair<int, int>> pending;   // (stage, event slot) recorded, not yet read
    double stage_ms[PS_NUM_STAGES] = {};
    int64_t stage_n[PS_NUM_STAGES] = {};
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;

    // create-time arena (see PsPool): device block + pinned mirror, open only inside ps_problem_create
    char *arena_dev = nullptr, *arena_host = nullptr;
    void* words_host = nullptr;
    size_t arena_used = 0;
    bool arena_open = false, arena_poisoned = false;

    template <typename T>
    int alloc(T** out, size_t n, bool device_written = false /* filled by a kernel of the structure build: not in the arena, whose closing copy would overwrite it */) {
        *out = nullptr;
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        if (arena_open && bytes <= PS_ARENA_SMALL && !device_written) {
            const size_t off = (arena_used + 255) & ~(size_t)255;
            if (off + bytes <= PS_ARENA_BYTES) {
                std::memset(arena_host + off, 0, bytes);          // the closing copy writes the whole used range
                arena_used = off + bytes;
                dev_bytes += bytes;
                *out = (T*)(arena_dev + off);
                return 0;
            }
        }
        void* p = nullptr;
        static const bool guard_on = ps_env("PS_ALLOC_GUARD") != nullptr;
        const size_t padded = (bytes + 255) & ~(size_t)255;
        if (slab_left >= padded) {                                // inside a slab_reserve()d block: no call into the runtime
            *out = (T*)slab; slab += padded; slab_left -= padded; dev_bytes += bytes;
            return 0;
        }
        hipError_t e = hipMalloc(&p, guard_on ? padded + 4096 : bytes);
        if (e != hipSuccess) return fail(std::string("hipMalloc: ") + hipGetErrorString(e));
        if (guard_on) {
            if (hipMemset((char*)p + bytes, 0xA5, padded - bytes + 4096) != hipSuccess) return fail("hipMemset (guard) failed");
            guards.push_back({(char*)p + padded, bytes, (int)guards.size()});
            fprintf(stderr, "GUARD %p table #%d = %zu bytes (%s)\n", (void*)this, (int)guards.size() - 1, bytes, __PRETTY_FUNCTION__);
        }
        // PS_ARENA_POISON=1 (debugging): big tables start as NaN too -- recycled device memory is not zero, and a kernel that
        // reads a word nothing wrote (padding of a tile, a slot past the end) then shows instead of depending on history
        static const bool poison_all = ps_env("PS_ARENA_POISON") != nullptr;
        if (poison_all && hipMemset(p, 0xFF, bytes) != hipSuccess) return fail("hipMemset (poison) failed");
        allocs.push_back(p);
        dev_bytes += bytes;
        *out = (T*)p;
        return 0;
    }
    // One hipMalloc for a group of tables that are created together in the middle of a solve (the lagged inverse's ~20
    // buffers: 0.5 ms of hipMalloc calls inside one iteration of a problem whose iterations take 0.1 ms).  The tables that
    // follow are carved from it in 256-byte steps; what does not fit falls through to hipMalloc.
    char* slab = nullptr; size_t slab_left = 0;
    int slab_reserve(size_t bytes) {
        if (ps_env("PS_ALLOC_GUARD")) return 0;                   // guard mode wants every table on its own
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return fail(std::string("hipMalloc: ") + hipGetErrorString(e));
        if (ps_env("PS_ARENA_POISON") && hipMemset(p, 0xFF, bytes) != hipSuccess) return fail("hipMemset (poison) failed");
        allocs.push_back(p);
        slab = (char*)p; slab_left = bytes;
        return 0;
    }
    void slab_close() { slab = nullptr; slab_left = 0; }
    bool in_arena(const void* p) const {
        return arena_open && (const char*)p >= arena_dev && (const char*)p < arena_dev + PS_ARENA_BYTES;
    }
    template <typename T>
    int upload(T** out, const T* src, size_t n, bool src_resident = false) {
        if (alloc(out, n)) return -1;
        if (!n) return 0;
        if (src_resident) {     // a table the caller already holds in HBM (ps_problem_desc.flags): arena tables travel with the
                                // mirror's closing copy, so the mirror is what gets filled; anything else is device to device
            if (in_arena(*out)) HIP_OK(hipMemcpy(arena_host + ((char*)*out - arena_dev), src, n * sizeof(T), hipMemcpyDeviceToHost));
            else HIP_OK(hipMemcpy(*out, src, n * sizeof(T), hipMemcpyDeviceToDevice));
            return 0;
        }
        if (in_arena(*out)) std::memcpy(arena_host + ((char*)*out - arena_dev), src, n * sizeof(T));
        else HIP_OK(hipMemcpy(*out, src, n * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
    template <typename T>
    int upload(T** out, const std::vector<T>& v) { return upload(out, v.data(), v.size()); }
    // zero-fill on the stream; arena memory is already zero in the mirror (and must not be touched before the closing copy)
    int zero(void* p, size_t bytes) {
        if (in_arena(p)) return 0;
        HIP_OK(hipMemsetAsync(p, 0, std::max<size_t>(bytes, 1), stream));
        return 0;
    }
    int arena_begin() {
        PsPool& pool = ps_pool();
        void *d = nullptr, *m = nullptr;
        if (!pool.take(pool.dev_arenas, &d)) HIP_OK(hipMalloc(&d, PS_ARENA_BYTES));
        arena_dev = (char*)d;
        if (!pool.take(pool.host_arenas, &m)) HIP_OK(hipHostMalloc(&m, PS_ARENA_BYTES, hipHostMallocDefault));
        arena_host = (char*)m;
        // PS_ARENA_POISON=1 (debugging): the gaps between tables read as NaN, so a kernel that reads past the end of one shows
        static const bool poison = ps_env("PS_ARENA_POISON") != nullptr;
        if (poison) std::memset(arena_host, 0xFF, PS_ARENA_BYTES);
        arena_poisoned = poison;
        arena_used = 0;
        arena_open = true;
        return 0;
    }
    int arena_flush() {        // the tables staged so far, for a kernel of the structure build that reads them (the closing copy repeats it)
        if (arena_open && arena_used) HIP_OK(hipMemcpyAsync(arena_dev, arena_host, arena_used, hipMemcpyHostToDevice, stream));
        return 0;
    }
    int arena_close() {        // one copy of everything staged; the caller synchronises the stream afterwards
        arena_open = false;
        if (arena_poisoned) arena_used = PS_ARENA_BYTES;       // (the poisoned tail travels too)
        if (arena_used) HIP_OK(hipMemcpyAsync(arena_dev, arena_host, arena_used, hipMemcpyHostToDevice, stream));
        return 0;
    }
    void arena_release() {     // after the handle's streams are idle
        PsPool& pool = ps_pool();
        if (arena_dev && !pool.give(pool.dev_arenas, (void*)arena_dev)) hipFree(arena_dev);
        if (arena_host && !pool.give(pool.host_arenas, (void*)arena_host)) hipHostFree(arena_host);
        if (words_host && !pool.give(pool.host_words, words_host)) hipHostFree(words_host);
        arena_dev = arena_host = nullptr; words_host = nullptr;
    }
};

// the batched marginals' dense block (ps_abi_cov.h) goes when its reduced system does: at the next linearisation, the next
// ps_covariance_begin, destroy
inline void cov_release(ps_problem* h) {
    if (!h->cov_buf) return;
    hipStreamSynchronize(h->stream);
    hipFree(h->cov_buf);
    h->cov_buf = nullptr;
    h->cov_sigma_epoch = -1;
}

// which launches a linearisation issues is decided when an option (or the handle's role: a collective, a shard buffer)
// changes, not per call.  "lin_zero_list": only where the split of S into stored and accumulated slots holds -- the untiled
// pipelined pair kernel writes every block it owns with `=` -- and the handle is no landmark shard (a shard's system is
// packed, exchanged and summed over slots its own pairs never touch: it keeps the fill over everything)
inline void relook_launch_gates(ps_problem* h) {
    const bool shard = (h->nccl_allreduce && h->nccl_comm) || h->seg_allgather || h->shard_pack || h->has_extra_pairs;
    h->lin_zero_gate = h->lin_zero_list && h->zero_slots && !h->Spart && h->schur_pipeline && h->npitems > 0 && h->D == 6 && !shard;
    // "setup_ride": the finalisation is in the pair launch (fin_in_pairs of linearize(): untiled, pipelined, SE(3), no task writes a
    // diagonal block), nothing adds into the diagonal blocks behind that launch (pose-to-pose factors, host rows) and the system is
    // not exchanged and summed over ranks afterwards; and the fused CG takes the system -- not k_direct_solve, the classic PCG or
    // (known once the coarse level is built: linearize() looks again) the explicit PCG.
    h->ride_gate = h->setup_ride && !h->Spart && h->schur_pipeline && h->npitems > 0 && h->npair_items > 0 && !h->has_diag_tasks &&
                   h->D == 6 && h->F == 0 && h->FH == 0 && !shard && h->pcg_variant == 1 && h->nr > 0 &&
                   h->nr * h->D > h->direct_max && !(h->coarse_built && h->cg_explicit);
    h->ride_valid = false;
}

#include "ps_host_cg.h"
#include "ps_host_ldi.h"
#include "ps_host_iteration.h"
#include "ps_host_build.h"
#include "ps_host_structure.h"

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

#include "ps_abi_problem.h"
#include "ps_abi_solver.h"
#include "ps_abi_cov.h"
#include "ps_abi_triang.h"
#include "ps_host_ransac.h"
#include "ps_abi_small.h"
#include "ps_abi_twoview.h"
#include "ps_abi_pnp.h"
#include "ps_abi_sim3.h"
#include "ps_host_sim3pg.h"
#include "ps_abi_sim3pg.h"
#include "ps_abi_dense.h"
#include "ps_abi_feat.h"

}  // extern "C"
