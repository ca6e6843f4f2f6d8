/*
 * pyslam_hip.h -- C ABI of the MI355X-native Gauss-Newton / LM core.
 *
 * The reference (utiasSTARS/pyslam) has no native or FFI boundary: its hot
 * path is pure Python.  This header defines the
 * boundary a maintainer would bind instead; every entry point names the
 * reference code it replaces (paths relative to the reference repository).
 * The binding itself (ctypes) is shown in INTEGRATION.md and implemented in
 * pyslam_amd/_native.py.
 *
 * Conventions
 *   - plain C types only; the table pointers in ps_problem_desc are HOST
 *     pointers unless ps_problem_desc.flags says they are resident in HBM
 *     (PS_DESC_DEVICE_PARAMS / PS_DESC_DEVICE_TABLES); either way
 *     ps_problem_create copies them into the handle's own layout (records
 *     sorted by landmark and by pose), the handle owns that memory and the
 *     caller keeps ownership of its arrays.  ps_set_params / ps_get_params and
 *     the pose part of ps_get_dx take host OR device pointers;
 *   - every function returns 0 on success, <0 on error (message through
 *     ps_last_error()); nothing throws across the ABI;
 *   - all launches go to ONE HIP stream per handle (the `stream` argument of
 *     ps_problem_create, a hipStream_t; NULL = a stream the handle creates);
 *     functions that return host scalars synchronise that stream, the
 *     others only enqueue;
 *   - arithmetic is fp64 throughout (the reference is float64 numpy).
 *
 * Table layout: see pyslam_amd/lowering.py (LoweredProblem).
 */
#ifndef PYSLAM_HIP_H
#define PYSLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ps_problem ps_problem;

typedef struct ps_problem_desc {
    int32_t dof;                 /* 6: SE(3) poses, 3: SE(2) poses                           */
    int32_t num_poses;           /* rows of `poses` (12 doubles SE3 / 6 doubles SE2 each)     */
    const double*  poses;        /* [R row-major | t]                                         */
    const int32_t* pose_rid;     /* index in the reduced system, -1 = held constant           */
    int32_t num_points;
    const double*  points;       /* (num_points, 3)                                           */
    const int32_t* point_vid;    /* variable-landmark index, -1 = held constant               */

    /* stereo reprojection blocks (reference residuals/reprojection_residual.py:13-37,
       reprojection_motion_only_residual.py:35-113 lowered onto constant points) */
    int64_t num_obs;
    const int32_t* obs_pose;
    const int32_t* obs_point;
    const double*  obs_uvd;      /* (num_obs, 3)                                              */
    const int32_t* obs_grp;      /* row of obs_groups                                         */
    int32_t num_cams;       const double* cams;        /* (num_cams, 5) cu cv fu fv b  (b >= 0: stereo; b = -1: RGB-D camera, third coordinate is z; b = -2: monocular (u, v), third coordinate 0 and third stiffness row / column 0; any other negative b is an error) */
    int32_t num_stiff3;     const double* stiff3;      /* (num_stiff3, 9) 3x3 row-major       */
    int32_t num_obs_groups; const double* obs_groups;  /* (n, 4) cam, stiff, loss id, loss k  */

    /* pose-pose edges (reference residuals/pose_to_pose_residual.py:12-32) */
    int64_t num_edges;
    const int32_t* e_i;
    const int32_t* e_j;
    const double*  e_Tobs_inv;   /* T_2_1_obs^-1, packed like poses                           */
    const int32_t* e_grp;        /* row of edge_groups                                        */
    /* unary pose priors (reference residuals/pose_residual.py:12-27) */
    int64_t num_priors;
    const int32_t* u_i;
    const double*  u_Tobs_inv;
    const int32_t* u_grp;
    int32_t num_stiffd;      const double* stiffd;       /* (n, dof*dof) row-major            */
    int32_t num_edge_groups; const double* edge_groups;  /* (n, 3) stiff, loss id, loss k     */

    /* multi-GPU: pose pairs (reduced indices, i<j) that other landmark shards
       couple, so every rank builds the SAME block pattern for the all-reduce */
    int64_t num_extra_pairs;
    const int32_t* extra_pair_i;
    const int32_t* extra_pair_j;

    /* 0 = every pointer above is a host pointer.  PS_DESC_DEVICE_PARAMS: `poses` and `points` are device pointers (on the
       device the handle is created on) and are copied device to device.  PS_DESC_DEVICE_TABLES: EVERY other non-NULL table
       pointer above is a device pointer; the index and measurement tables come to the host once for the structure pass
       (sorting by landmark / pose, pair lists), the caller needs no host copy of them. */
    uint32_t flags;
} ps_problem_desc;

enum { PS_DESC_DEVICE_PARAMS = 1u, PS_DESC_DEVICE_TABLES = 2u };

/* sizes a binding needs to allocate result buffers */
typedef struct ps_problem_info {
    int32_t dof, num_poses, num_reduced, num_points, num_var_points;
    int64_t num_obs, num_edges, num_priors;
    int64_t reduced_nnzb;        /* blocks in the reduced (Schur) system, both triangles      */
    int64_t num_pairs;           /* off-diagonal Schur contributions (upper triangle)         */
    int64_t reduce_count;        /* doubles in the all-reduce payload [upper(S) | g | cost | flag] */
    int64_t device_bytes;        /* HBM held by the handle                                    */
    int64_t cg_restarts;         /* restarts of the pipelined CG so far: its recurrences broke down (rounding drift out of
                                    range(V^T) on the singular folded system) and the solve went on
                                    from the true residual                                    */
    int64_t cg_kernel_launches;  /* kernels enqueued for iterations of the reduced solve so far (1 per iteration for the
                                    folded CG, 3 or 4 for the explicit two-level PCG, 2 for the classic PCG)            */
    int64_t ldi_solves;          /* reduced solves preconditioned with the lagged dense inverse (option "lagged_inverse")   */
    int64_t ldi_fallbacks;       /* ... that gave the inverse up after "ldi_cap" iterations and ran the standard solver       */
    int64_t ldi_seeds;           /* inverses seeded on the side stream (after a standard solve)                             */
    int64_t xcg_fused_solves;    /* explicit two-level PCG solves set up in the one-launch form (option "xcg_fused")       */
    int64_t xcg_fused_fallbacks; /* ... repeated in the three-launch form after a breakdown of the single-reduction recurrences */
    int64_t cg_persist_solves;   /* folded CG solves run in ONE launch (option "cg_persist", csrc/ps_k_cg_persist.h)          */
    int64_t cg_persist_failures; /* ... whose in-launch exchange timed out: solved again with the launch-per-iteration kernels,
                                    and the one-launch form is not used on the handle any more                              */
    int64_t cg_persist_refused;  /* solves that wanted a one-launch form and ran launch by launch instead because its grid
                                    could not be resident at that moment: one-launch solves of OTHER handles of this process
                                    held the compute units (a form that can never be resident on the handle's stream -- device
                                    size, CU mask, occupancy -- is not even tried and does not count)                        */
    int32_t persist_cus;         /* compute units the solver's stream may use as the core found them (device count, the stream's
                                    CU mask, ROC_GLOBAL_CU_MASK; 0: unknown, e.g. HSA_CU_MASK is set: no one-launch form)     */
    int32_t persist_cus_needed;  /* units the one-launch form of this handle needs resident (0: the system does not fit the form) */
    int64_t landmark_passes_taken_over; /* linearisations that found their landmark pass done: it ran in the previous call's tail
                                    (or in ps_eval_cost) and summed that cost on its way -- options "expect_next", "fuse_cost"   */
} ps_problem_info;

enum { PS_NUM_STAGES = 12 };
/* stage ids for ps_get_stage_times (ALLREDUCE / PACK: the landmark-sharded iteration driven by the core itself,
   ps_set_collective -- both all-reduces, and k_shard_pack + k_shard_unpack; CG_KERNEL: the launch(es) that run the CG
   iterations of the reduced solve alone -- k_cg_persist / k_xcg_persist or the per-iteration kernels -- without the set-up
   kernels and the recovery that PCG also spans; recorded at profiling level 1 like SCHUR) */
enum { PS_ST_LANDMARK = 0, PS_ST_POSE = 1, PS_ST_SCHUR = 2, PS_ST_EDGES = 3, PS_ST_PCG = 4,
       PS_ST_BACKSUB = 5, PS_ST_UPDATE = 6, PS_ST_COST = 7, PS_ST_TOTAL = 8, PS_ST_CG_KERNEL = 9,
       PS_ST_ALLREDUCE = 10, PS_ST_PACK = 11 };

const char* ps_last_error(void);
int ps_device_count(void);
/* Pay the process-wide one-off costs now (code-object load at the first kernel launch, allocator set-up at the first
   hipMalloc) instead of inside the first solve.  Idempotent; the binding calls it when it first finds a device. */
int ps_warm_up(void);

/* Lower the tables to HBM and precompute the iteration-invariant structure
   (landmark / pose segment lists, Schur pair lists, block pattern).
   Replaces the per-iteration Python bookkeeping of pyslam/problem.py:294-329.
   From 200 000 observations up the observation tables and the Schur pair list are built BY THE DEVICE from the caller's
   columns (csrc/ps_host_build.h; with PS_DESC_DEVICE_TABLES the columns are read in place), bit-identical to the host
   builder that smaller problems use.  Environment, read once here: PS_CREATE_DEVICE = 0 host builder / 1 by size
   (default) / 2 always; PS_SCHUR_TILE_KB, PS_SCHUR_TILE_MIN_MB, PS_CREATE_KEYS64: list variants the
   parity tests hold against each other.
   THREADS: the host builder (below 200 000 observations, pose graphs, more than 255 observation groups) splits its
   counting sorts over up to 16 std::threads, all joined before this call returns; no other entry point of this header
   creates a host thread, and none is alive between calls.  (SURVEY section 8b asked for "no internal host threads": true
   of the iteration path; at create time the device build is the single-threaded route.) */
int ps_problem_create(const ps_problem_desc* desc, void* stream, ps_problem** out);

/* Pose factors whose blocks the CALLER evaluates (Problem with Options.hybrid_blocks: user-defined residual blocks on poses).
   Row k stands for poses (i[k], j[k]) -- pose indices, i[k] = -1 for a row on one pose -- and enters the pair structure as a
   pose-pose edge does.  Its values, one scratch row [H11 | H12 | H22 | g1 | g2] (3 D^2 + 2 D doubles, g = -J~^T e~) per row,
   come from ps_set_host_rows before each linearisation and are assembled into S and g with the edges and priors (the
   Marquardt (1 + lambda) scaling included).  A handle made here is a HYBRID handle: its own cost passes see only the typed
   blocks, so everything that would decide from a cost inside one call is off (ps_solve and ps_motion_only_solve return 1,
   option "expect_next" is ignored, the one-launch motion-only iteration and the lagged dense inverse are not used). */
typedef struct ps_host_rows_desc {
    int64_t num;
    const int32_t* i;
    const int32_t* j;
} ps_host_rows_desc;
int ps_problem_create_hybrid(const ps_problem_desc* desc, const ps_host_rows_desc* rows, void* stream, ps_problem** out);
/* Values of the host rows (num rows of 3 D^2 + 2 D doubles, host memory, num = the create call's) at the current
   parameters, and the caller's cost of its blocks at the same point (blocks whose poses are all constant excluded).  A
   following ps_gn_iteration without line search returns the typed cost plus this cost; with line search the cost after
   the step is the typed blocks' only and the caller adds its own.  Copied on the solver's stream before this returns. */
int ps_set_host_rows(ps_problem* h, const double* rows, int64_t num, double cost);
int ps_problem_destroy(ps_problem* h);
int ps_get_info(ps_problem* h, ps_problem_info* info);

/* sum_blocks sum_i rho(r_i) at the current parameters -- pyslam/problem.py:110-128
   (include_all_constant=1) or the cost term of problem.py:334,358
   (include_all_constant=0: blocks whose parameters are all constant are skipped).
   SIDE EFFECT (option "fuse_cost" = 1, the default, include_all_constant = 1, every observation on a variable landmark with
   at most 16 observations): the cost is summed by the landmark pass itself, which REWRITES Z, C^-1 and c at the current
   parameters (a linearisation that follows at this point finds its landmark pass done).  If the parameters have moved since the
   last ps_linearize those buffers then belong to the new point, and the staged entry points that read them -- ps_backsub,
   ps_gn_finish, ps_gn_solve_finish[_enqueue], ps_get_landmark_factors -- fail with "no longer belong to the last ps_linearize"
   until ps_linearize is called again.  The same holds after a whole-iteration call (ps_gn_iteration, ps_solve) that expected a
   successor: its tail has run the successor's landmark pass. */
int ps_eval_cost(ps_problem* h, int include_all_constant, double* cost);

/* Residuals + Jacobians + IRLS weights + J^T J assembly + landmark elimination:
   builds the reduced system S dx_p = g in HBM.  Replaces pyslam/problem.py:279-360
   (block.evaluate, loss.weight, sparse.bmat, HT.dot(HT.T), -HT.dot(e)).
   lambda: Marquardt damping added as lambda*diag(J^T J); 0 = the reference's GN. */
int ps_linearize(ps_problem* h, double lambda);

/* Exchange buffer of the landmark-sharded (multi-GPU) iteration: the contiguous payload
   [upper block triangle of S incl. diagonal | g | cost (2) | failure flag] a caller all-reduces (sum)
   between ps_linearize and ps_solve_reduced.  ps_shard_pack gathers it from the reduced system (S is
   exactly symmetric: only one triangle travels), ps_shard_unpack scatters the sum back, mirrors the upper
   blocks into the lower triangle and raises the landmark-failure status on EVERY rank if any shard
   reported a non-positive-definite H_ll (ranks fail together, none is left waiting in a collective).
   Enqueue-only, on the handle's stream.  SURVEY.md section 8e. */
int ps_reduce_buffer(ps_problem* h, void** dev_ptr, int64_t* count);
int ps_shard_pack(ps_problem* h);
int ps_shard_unpack(ps_problem* h);

/* Block-Jacobi PCG on the reduced system; replaces the splinalg.spsolve call of
   pyslam/problem.py:186 together with ps_backsub.  Stops when the preconditioned residual
   norm sqrt(r^T M^-1 r) has dropped by `tol` (scale-invariant; relres_out reports it).
   tol <= 0 (here and wherever this header takes a `pcg_tol` / `tol` of the reduced solve): the DEFAULT -- 1e-12 where the
   reduced system is the Schur complement of a bundle adjustment (variable landmarks), 1e-14 for pose graphs (no landmarks:
   priors of stiffness ~1e6 beside loop closures of ~1 leave cond(M^-1 S) at 1e4-1e5 after the two-level preconditioner, and
   error <= cond x relative residual): what meets |dx - dx_spsolve| <= 1e-8 |dx| without the caller knowing the
   condition number.  pyslam_amd.Options.pcg_tol = None passes 0. */
int ps_solve_reduced(ps_problem* h, double tol, int max_iters, int* iters_out, double* relres_out);

/* Landmark back-substitution dx_l = Hll^-1 (b_l - W^T dx_p). */
int ps_backsub(ps_problem* h);

/* dx in device order [reduced poses (dof each) | variable points (3 each)];
   either pointer may be NULL.  ps_step_norm2 returns ||dx||^2. */
int ps_get_dx(ps_problem* h, double* dx_pose, double* dx_point);
int ps_step_norm2(ps_problem* h, double* norm2);

/* T <- exp(step*xi) T, p <- p + step*dp -- pyslam/problem.py:155-156, 400-409. */
int ps_apply_update(ps_problem* h, double step);

/* best_params snapshot / restore of pyslam/problem.py:163-175. */
int ps_snapshot_params(ps_problem* h);
int ps_restore_params(ps_problem* h);

/* either pointer may be NULL; each may be a host or a device pointer (a torch caller keeps its parameters resident) */
int ps_get_params(ps_problem* h, double* poses, double* points);
int ps_set_params(ps_problem* h, const double* poses, const double* points);

/* One whole Gauss-Newton / LM iteration with a single host synchronisation:
   linearize -> PCG -> back-substitution -> update -> post-step cost.
   cost_out = cost after the step (linesearch != 0, pyslam/problem.py:362-398 with its
   always-full step) or cost at the linearisation point (linesearch == 0, problem.py:192). */
int ps_gn_iteration(ps_problem* h, double lambda, double pcg_tol, int pcg_max_iters,
                    int linesearch, double* cost_out, double* dx_norm_out,
                    int* pcg_iters_out, double* pcg_relres_out);

/* The loop of Problem.solve (reference pyslam/problem.py:130-178) for a problem of ONE variable SE(3) pose observing
   constant landmarks -- config 5, built per frame by pipelines/sparse.py:153-161 -- in ONE launch and one
   synchronisation: the start cost, then iterations until `iterations > max_iters`, ||dx|| < min_update_norm, cost <
   min_cost or the non-decreasing-step rules stop it (best parameters kept and restored as the reference does; the rule
   is pyslam_amd/csrc/ps_stop_rule.h, run by the kernel).
   Options carry the reference's names; linesearch != 0: an iteration's cost is the cost after its (always full) step,
   else the cost of its linearisation point (problem.py:188-192).  cost_history receives the reference's
   _cost_history (at most max_iters + 2 entries), the pose is left updated and, if pose12_out is not NULL, also returned
   ([R row-major | t]: no second copy from the device).
   Returns 0 = solved, 1 = not this kind of problem or history too long for `cap` (nothing done: iterate with
   ps_gn_iteration), <0 = error. */
typedef struct ps_solve_options {
    int32_t max_iters, allow_nondecreasing_steps, max_nondecreasing_steps, linesearch;
    double min_update_norm, min_cost, min_cost_decrease, lm_lambda;
} ps_solve_options;
int ps_motion_only_solve(ps_problem* h, const ps_solve_options* options, double* cost_history, int32_t cap,
                         int32_t* n_history, int32_t* iterations, double* last_dx_norm, double* pose12_out);

/* Start of a NEW solve on a live handle: drop every piece of state the solver carries from one whole-iteration call to
   the next (lagged coarse factors / inverses and their tags, the lagged dense inverse of S, launch-count predictions, the
   cost history), waiting for side-stream work in flight first.  Tables, parameters and options stay.  The next
   ps_gn_iteration behaves exactly like the first one of a freshly created handle -- what Problem.solve (reference
   pyslam/problem.py:130-141: every solve starts from scratch) calls before its first iteration, so that a solve is a
   function of (parameters, options) and not of what the handle did before. */
int ps_reset_solver_state(ps_problem* h);

/* Hash of the HIP sources the loaded library was compiled from (first 16 hex digits of the SHA-256 over include/pyslam_hip.h
   and pyslam_amd/csrc/, the -DPS_BUILD_SHA of __graft_entry__.build(); "unknown" for a hand build): bench.py reports THIS and
   refuses to run on a library that does not match the sources on disk. */
const char* ps_build_sha(void);

/* The loop of Problem.solve (reference pyslam/problem.py:130-178) on a resident problem, in one call: ps_reset_solver_state,
   the start cost (its pass is enqueued in front of the first iteration: no call and no synchronisation of its own), then
   whole iterations (each exactly ps_gn_iteration) until `iterations > max_iters`, ||dx|| < min_update_norm, cost < min_cost or
   the non-decreasing-step rules stop it, the best parameters kept by ps_snapshot_params / ps_restore_params as the reference
   keeps best_params.  cost_history receives the reference's _cost_history (at most max_iters + 2 entries); pcg_iters,
   pcg_relres and iter_ms (host wall clock of every iteration call, ms) receive one entry per iteration, each may be NULL.
   The same loop as pyslam_amd/problem.py: device_solve (which calls this when the device offers it), without the
   interpreter between two iterations.  The stopping rule itself has ONE definition for every loop of the core, this one, ps_solve_lm
   (its threshold tests), ps_motion_only_solve and ps_dense_track: pyslam_amd/csrc/ps_stop_rule.h, which reads ps_solve_options;
   the Python loops use its counterpart, pyslam_amd/problem.py: StopRule.  Returns 0 = solved, 1 = not offered for this handle (landmark-sharded: the caller
   loops with ps_gn_iteration) or `cap` too small, <0 = error. */
int ps_solve(ps_problem* h, const ps_solve_options* options, double pcg_tol, int pcg_max_iters, double* cost_history,
             int32_t cap, int32_t* n_history, int32_t* iterations, double* last_dx_norm, int32_t* pcg_iters,
             double* pcg_relres, double* iter_ms);

/* Adaptive Levenberg-Marquardt (Nielsen 1999; Madsen, Nielsen, Tingleff, algorithm 3.16).
   ps_lm_iteration is ps_gn_iteration at the damping `lambda` whose tail also sums, on the device,
       model_decrease = 0.5 h^T (lambda D h + g),   D = diag(J~^T J~) undamped,   (J~^T J~ + lambda D) h = g = -J~^T e~
   for the step h it has just applied; the scalar arrives with the cost and ||dx|| in the block the call's ONE synchronisation
   reads.  The caller forms rho = (cost before - cost after) / model_decrease and, to reject the step, restores a snapshot it took
   in front of the call (ps_snapshot_params / ps_restore_params); the next call linearises again at the restored point.
   linesearch must be non-zero (the cost returned is the cost AFTER the step).  For such a call the tail starts none of the next
   iteration's work ahead, and the one-launch motion-only kernel and the lagged dense inverse are not used.  A hybrid handle
   returns the typed blocks' cost, as ps_gn_iteration does; a landmark-sharded handle is an error. */
int ps_lm_iteration(ps_problem* h, double lambda, double pcg_tol, int pcg_max_iters, int linesearch, double* cost_out,
                    double* dx_norm_out, double* model_decrease_out, int* pcg_iters_out, double* pcg_relres_out);

/* The adaptive loop in one call, as ps_solve is the default loop in one call: ps_reset_solver_state, the start cost in front of
   the first iteration, then per iteration: snapshot, ps_lm_iteration at the current lambda, rho;
       rho > 0: accept, lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2;    else: reject (the parameter tables are exchanged with
       the snapshot's: no copy), lambda *= nu, nu *= 2;                   lambda clamped to [lambda_min, lambda_max];
   a model_decrease that is not positive and finite is a rejection.  cost_history receives the cost after every iteration (the
   unchanged previous cost after a rejection: it never increases).  Stops when iterations > max_iters, ||dx|| < min_update_norm,
   cost < min_cost, an ACCEPTED step has cost >= min_cost_decrease * previous cost, or a rejection asks for lambda > lambda_max.
   lambda0 <= 0 means 1e-3.  allow_nondecreasing_steps, max_nondecreasing_steps and lm_lambda are ignored; linesearch must be
   non-zero.  Outputs as ps_solve, plus lm_rows (may be NULL): (lambda used, rho, accepted 1 / 0, model_decrease) per iteration,
   4 * (max_iters + 1) doubles at most.  Returns 0 = solved, 1 = not offered for this handle (landmark-sharded; hybrid: the
   caller loops with ps_lm_iteration and adds its blocks' cost) or `cap` too small, <0 = error.
   sizeof(ps_lm_options) == 72. */
typedef struct ps_lm_options {
    int32_t max_iters, allow_nondecreasing_steps, max_nondecreasing_steps, linesearch;
    double min_update_norm, min_cost, min_cost_decrease, lm_lambda;
    double lambda0, lambda_min, lambda_max;
} ps_lm_options;
int ps_solve_lm(ps_problem* h, const ps_lm_options* options, double pcg_tol, int pcg_max_iters, double* cost_history,
                int32_t cap, int32_t* n_history, int32_t* iterations, double* last_dx_norm, int32_t* pcg_iters,
                double* pcg_relres, double* iter_ms, double* lm_rows);

/* Second half of an iteration for a landmark-sharded (multi-GPU) caller, after
   ps_linearize -> all-reduce -> ps_solve_reduced: back-substitution, update, cost, ONE
   synchronisation.  Returns this shard's cost and ||dx_pose||^2, ||dx_point||^2 separately
   (poses are replicated, landmarks are not). */
int ps_gn_finish(ps_problem* h, int linesearch, double* cost_out, double* dx_pose_norm2,
                 double* dx_point_norm2);

/* ps_solve_reduced + ps_gn_finish with ONE synchronisation (the tail is enqueued behind the CG
   launches and gated on the device-side convergence flag): the sharded caller's second half. */
int ps_gn_solve_finish(ps_problem* h, double pcg_tol, int pcg_max_iters, int linesearch, double* cost_out,
                       double* dx_pose_norm2, double* dx_point_norm2, int* pcg_iters_out,
                       double* pcg_relres_out);

/* Fully asynchronous variant for the multi-GPU driver: ps_gn_solve_finish_enqueue enqueues the
   reduced solve and the (convergence-gated) tail and leaves this shard's {cost, ||dx_point||^2}
   in the 2-double device buffer of ps_shard_buffer; the caller all-reduces that buffer on the
   same stream and calls ps_gn_result (the only synchronisation).  If *done == 0 the CG needed
   more launches: call enqueue again with first = 0 (it returns 1 on the final, ungated pass). */
int ps_shard_buffer(ps_problem* h, void** dev_ptr);

/* Native collective: hand the core RCCL's ncclAllReduce entry point and an ncclComm_t (created by
   the binding, one rank per GPU).  ps_gn_iteration then runs the whole landmark-sharded iteration
   -- both all-reduces included -- on the handle's stream with a single host synchronisation. */
int ps_set_collective(ps_problem* h, void* nccl_all_reduce_fn, void* nccl_comm);
/* The exchange of the partial reduced systems as an ALL-GATHER OF SEGMENTS inside the core's one-call sharded iteration (round 6;
   needs ps_set_collective first -- the second, two-scalar exchange stays an all-reduce).  With landmarks sharded by first observing
   pose a rank's partial system is non-zero on one band segment of S (C4 on 8 ranks: 3.2 of 23.5 MB): every rank sends
   [tail words | its elements of the packed buffer of ps_reduce_buffer] once (ncclAllGather, `maxlen` doubles per rank) and adds up
   what it receives itself -- every destination element over its contributing ranks in RANK ORDER, the same on every rank, so the
   replicated solve stays bit-identical across ranks.  The plan is the caller's (pyslam_amd/distributed.py: segment_plan, held
   against a dense sum by the CPU tests): `mine` = this rank's element positions (n_mine); `dst` (n_dst) = every position some
   rank touches, `src_ptr` (n_dst + 1) / `src_off` = for each of them the offsets rank * maxlen + 3 + k into the gathered buffer,
   ascending rank.  The three tail words (cost (2), failure flag) are summed over all ranks.  Arrays are copied.
   nccl_all_gather_fn == NULL: back to the sum all-reduce. */
int ps_set_segment_exchange(ps_problem* h, void* nccl_all_gather_fn, int32_t world, int32_t rank, int64_t maxlen,
                            int64_t n_mine, const int64_t* mine, int64_t n_dst, const int64_t* dst, const int64_t* src_ptr,
                            const int64_t* src_off);
int ps_gn_solve_finish_enqueue(ps_problem* h, double pcg_tol, int pcg_max_iters, int linesearch, int first);
int ps_gn_result(ps_problem* h, int* done, double* shard2, double* dx_pose_norm2,
                 int* pcg_iters_out, double* pcg_relres_out);

/* Covariance by columns -- pyslam/problem.py:196-216 (compute_covariance inverts the whole sparse
   precision matrix; get_covariance_block slices it).  ps_covariance_begin linearises at the current
   parameters (lambda = 0) and prepares the reduced solver.  ps_covariance_column then solves
   H x = e_k, e_k the unit vector of component `comp` of reduced pose `index` (kind 0) or of variable
   landmark `index` (kind 1), by the hot path's own Schur elimination, CG and back-substitution:
   x = column k of the covariance, left in the dx buffers (read it with ps_get_dx).  Scales to any
   problem the iteration handles; no dense n x n matrix is ever formed. */
int ps_covariance_begin(ps_problem* h);
int ps_covariance_column(ps_problem* h, int kind, int index, int comp, double tol, int max_iters,
                         int* iters_out, double* relres_out);

/* Batched marginal covariances (Problem.compute_marginal_covariances), after ps_covariance_begin:
   ps_covariance_marginals densifies the reduced system S it left behind (nr * dof unknowns, at most
   PS_COV_DENSE_MAX_UNKNOWNS: 1.2 GB per n x n buffer there, three of them), factors it and forms
   Sigma_pp = S^-1 in fp64 on the device.  pose_blocks (nr, dof, dof): the diagonal blocks of every reduced
   pose, in reduced order (rid); point_blocks (nv, 3, 3): every variable landmark's marginal
   M^T (I + sum_ij Z_i^T Sigma_pp[r_i, r_j] Z_j) M, in vid order.  Either may be NULL.  Every block is exactly
   symmetric and bit-identical from call to call.  Errors: above the limit (the column route has none), a
   non-positive or rounding-size pivot (gauge freedom: hold a pose constant or add a prior; nothing is
   written).  Sigma_pp stays on the handle until the next linearisation, ps_covariance_begin or
   ps_problem_destroy; it is not allocated unless this call is made.
   ps_covariance_pose_blocks reads out[k] = Sigma_pp[a_k, b_k] (dof x dof, reduced indices) from it. */
#define PS_COV_DENSE_MAX_UNKNOWNS 12288
int ps_covariance_marginals(ps_problem* h, double* pose_blocks /* (nr, D, D) or NULL */,
                            double* point_blocks /* (nv, 3, 3) or NULL */);
int ps_covariance_pose_blocks(ps_problem* h, int64_t n, const int32_t* a, const int32_t* b,
                              double* out /* (n, D, D) */);
/* After ps_covariance_marginals, any block of the full covariance from the same Sigma_pp:
   out[36 k ...] = Sigma[(kind_a[k], a[k]), (kind_b[k], b[k])]; kind 0 = reduced pose index (rid), 1 = variable
   landmark index (vid, the caller's order, as point_blocks); the block row-major dof_a x dof_b in the leading
   entries of a 36-double slot, the rest zero.  Pose-landmark: -sum_i Sigma_pp[a, r_i] Z_i M over the landmark's
   observations on variable poses (M: its factor, C^-1 = M^T M), landmark-pose its exact transpose; landmark-landmark
   M1^T (sum_ij Z_i^T Sigma_pp[r_i, r_j] Z_j) M2, (l2, l1) the exact transpose of (l1, l2); (l, l) bit-identical to
   point_blocks, pose-pose to ps_covariance_pose_blocks.  Any n: pairs pass through a fixed device buffer (allocated
   by the first call, freed by ps_problem_destroy), with results that do not depend on the chunking.  Errors: no
   current Sigma_pp, a kind other than 0 / 1, an index out of range, landmarks on a problem whose poses are not SE(3). */
int ps_covariance_cross_blocks(ps_problem* h, int64_t n, const int32_t* kind_a, const int32_t* a,
                               const int32_t* kind_b, const int32_t* b, double* out /* (n, 36) */);

/* Multi-view triangulation of variable landmarks from their observations and the CURRENT poses (constant poses included);
   Problem.triangulate_landmarks, pyslam_amd.triangulate_tables.  vids: n variable-landmark indices (vid, the caller's order),
   or NULL for every variable landmark (n ignored; results in vid order).  Per landmark, in the fixed slot order of the
   landmark-sorted tables (bit-identical from call to call):
     1. linear start: with x_n = (u - cu) / fu, y_n = (v - cv) / fv and the pose (R | t), rows r1 r2 r3, every observation gives
        (x_n r3 - r1) p = -(x_n t3 - t1) and (y_n r3 - r2) p = -(y_n t3 - t2); a stereo (z = fu b / d) or RGB-D (z = d) observation
        also r3 p = z - t3; the 3 x 3 normal equations are solved by Cholesky;
     2. refine_iters Gauss-Newton steps on the landmark's own robust reprojection cost (the iteration's evaluator: camera
        types, stiffness, IRLS weights), poses held; a step that does not lower the cost is not taken and ends the iteration,
        and so does a step whose 3 x 3 system cannot be solved (a pivot that is not positive, NaN -- the L1 weight of a
        residual component at zero): the landmark keeps its last accepted point and its status;
     3. status 0 ok | 1 fewer than two observations and none bearing depth | 2 no depth and the largest angle between two
        viewing rays below min_parallax_deg, or a linear start whose normal equations are not positive definite | 3 behind one
        of its cameras.
   points_out (n, 3): the new point, or the old one where the status is not 0; status_out (n).  write_back != 0: points
   with status 0 replace the handle's (as ps_set_params would).  One launch, one synchronisation. */
int ps_triangulate(ps_problem* h, int64_t n, const int32_t* vids /* (n) or NULL */, int refine_iters, double min_parallax_deg,
                   int write_back, double* points_out /* (n, 3) or NULL */, int32_t* status_out /* (n) or NULL */);

/* Parity / debug taps (device -> host). */
int ps_get_reduced_system(ps_problem* h, int32_t* row_ptr, int32_t* col_idx,
                          double* vals, double* g);       /* BSR, dof x dof blocks */
int ps_get_landmark_factors(ps_problem* h, double* cinv /* (nv,6) */, double* c /* (nv,3) */);
int ps_debug_reproj_blocks(ps_problem* h, double* r /* (N,3) */, double* jpose /* (N,18) */,
                           double* jpoint /* (N,9) */);  /* IRLS-scaled, original obs order */
/* The pose-factor kernel's own blocks (IRLS-scaled, as they enter J~^T J~): r~ (F, dof), J~_1 (F, dof, dof) and
   J~_2 (F, dof, dof), F = num_edges + num_priors in table order (edges first).  Edges: the reference's
   PoseToPoseResidual.evaluate (pyslam/residuals/pose_to_pose_residual.py:12-32: r = S log(T_2 T_1^-1 T_obs^-1),
   J_1 = -S Ad(T_2 T_1^-1), J_2 = S); priors: PoseResidual.evaluate (pose_residual.py:12-27: r = S log(T T_obs^-1),
   J = S in j2, j1 = 0).  Runs the production kernel with its tap open; S and g are not touched. */
int ps_debug_factor_blocks(ps_problem* h, double* r, double* j1, double* j2);
/* FNV-1a (64 bit) of the structure tables ps_problem_create left in HBM, in a fixed order: point slots, lobs, lorig,
   lm_ptr, lm_point, pose_of_rid, pitems, pitem_ptr, pobs, pairs, pair work items (XCD order), combine items, combine
   tasks, row_ptr, col_idx, diag_slot (16 words; 0 for a table the problem does not have).  What holds the device
   structure build against the host builder bit for bit (tests/test_gpu_create.py); no reference counterpart. */
int ps_debug_table_checksums(ps_problem* h, uint64_t* out, int capacity, int* count);
/* The run tables of the packed observation passes (csrc/ps_k_packed.h), device -> host.  *nwaves: runs on this handle (0: it keeps
   the 16-lane kernels); run (nwaves, 4): {first landmark, one past the last, first row, rows} per wave -- the record the kernels
   read under "packed_prefetch"; first (nwaves + 1): the run starts the record is made from; lm_ptr (variable landmarks + 1): first
   row of every landmark slot; sq_part (ceil(nwaves / 4)): the partial sums of ||dx_point||^2, one per workgroup, as the last packed
   back-substitution left them.  run / first / lm_ptr / sq_part may be NULL; capacity_waves: runs the caller's run / first /
   sq_part have room for (refused when too few: call with NULLs first).  No reference counterpart. */
int ps_debug_packed_runs(ps_problem* h, int32_t* nwaves, int32_t capacity_waves, int32_t* run, int32_t* first, int32_t* lm_ptr,
                         double* sq_part);
/* The work items of the pose pass (csrc/ps_k_linearize.h) and the partial sums its last launch left, device -> host.  *nitems: items
   on this handle (one workgroup each: a chunk of one variable pose's observations); items (nitems, 3): {reduced pose, first row,
   one past the last row} in the pose-ordered observation table; partial (nitems, 33): upper triangle of the 6 x 6 block (21) |
   gradient (6) | damping sums (6; zero after a linearisation with lambda = 0).  items / partial may be NULL; capacity_items: items
   the caller's tables have room for (refused when too few: call with NULLs first).  No reference counterpart. */
int ps_debug_pose_items(ps_problem* h, int32_t* nitems, int32_t capacity_items, int32_t* items, double* partial);

/* Tuning knobs.  [default; accepted values]: "0 / 1" is stored as value != 0; a range is refused outside it and truncated to
   an integer inside it; "any" is truncated and never refused.  One table holds every name with its parse rule, bounds, refusal
   and what a change invalidates on the handle: csrc/ps_options.h (checked on the CPU by tests/test_options_host.py).  Every
   name but "expect_next" and "solve_horizon" drops what was computed ahead for the next call.
     "pcg_variant"        [1; 0 or 1 exactly] fused single-launch-per-iteration CG on the block-Jacobi scaled system; 0 = classic two-launch PCG
     "coarse_groups"      [-1 auto; -1 <= value < 1024] hat-function intervals of the two-level preconditioner, 0 = off; above 63 only for the explicit
                              two-level PCG.  The coarse level is planned again by the next solve
     "coarse_basis"       [1; 0 / 1] coarse unknowns are body-frame twists (P_iq = w L_i^T Ad(T_i)); 0 = hats in scaled coordinates
     "coarse_lag"         [1; 0 / 1] whole-iteration calls build the two-level system with the previous iteration's coarse factor
     "direct_max_unknowns"[90; 0 .. 90] reduced systems up to this size are solved by a dense Cholesky instead of CG (0 = never)
     "direct_fused"       [1; 0 / 1] ... in one launch (k_direct_solve); 0: three
     "fused_motion_only"  [1; 0 / 1] problems without variable landmarks / pose factors: one launch per iteration
     "cg_explicit"        [1; 0 / 1] long sparse chains: apply the two-level preconditioner (k_xcg_*) instead of folding it in
     "coarse_lag_x"       [1; 0 / 1] ... and with the previous iteration's basis and X = P L_c^-T too: three set-up launches (k_rows_setup)
     "coarse_refresh_every" [1; 1 .. 16] explicit two-level PCG: only every k-th lagged set-up takes the newest coarse inverse and starts the
                              next side-stream factorisation (landmark-sharded runs whose iteration is shorter than that factorisation)
     "coarse_auto_hold"   [1; 0 / 1] explicit two-level PCG: while the solve has settled (last iteration changed the cost by < 1e-4
                              relative) keep the lagged coarse inverse, for at most 3 set-ups in a row (no assembly, no factorisation);
                              and for as long as the caller linearises at the point (same start cost, same lambda) the inverse in use
                              was formed from.  A call whose lambda is more than a factor of four from the newest inverse's (or zero against non-zero)
                              factors its own A_c (no lag).
     "coarse_adaptive_hold" [1; 0 / 1] explicit two-level PCG: keep the lagged coarse inverse (no assembly, no side-stream factorisation) while the
                              last solve with it took at most 3 iterations more than the first one did (at most 8 set-ups in a row)
     "xcg_restrict_fused" [1; 0 / 1] explicit two-level PCG: three launches per iteration (restriction in the SpMV epilogue, t by recurrence)
                              instead of four
     "lagged_inverse"     [1; 0 / 1] reduced systems of "direct_max_unknowns" + 1 .. "ldi_max_unknowns" [2048; 0 .. 3328: pays from ~7 iterations per solve on] unknowns (folded CG, one GPU, whole-iteration calls):
                              precondition the CG with a dense fp32 inverse of the PREVIOUS iteration's S, kept current on the side
                              stream by one Newton-Schulz step per iteration (two fp32 MFMA GEMMs) and seeded from the two-level
                              operator of the last standard solve; tried while the last step changed the cost by at most
                              "ldi_cost_tol" [0.05; any double >= 0] relative, given up (standard solver + re-seed) after "ldi_cap" [12; 1 .. 64] iterations.
                              It only preconditions: the solution is the current system's at pcg_tol either way.
     "ldi_direct"         [-1; any] ... seeded by a DIRECT fp64 factorisation of S on a stream of its own instead of Newton-Schulz
                              (below 0: pose graphs from the start, any problem after a rejected Newton-Schulz seed; 0 never; above 0 always);
                              usable a fixed 2 / 4 / 6 calls later (n <= 400 / 800 / 1 536)
     "ldi_seed_lag" [1; 1 .. 16], "ldi_seed_steps" [3; 1 .. 40], "ldi_refresh_its" [7; 0 .. 64]: schedule of the Newton-Schulz seed / refresh
     "xcg_fused"          [1; 0, 1 or 2 exactly] explicit two-level PCG: ONE launch per iteration (single-reduction recurrences; the restriction, the coarse
                              product for the nodes a workgroup needs, the prolongation and the SpMV in one kernel, the row's matrix
                              blocks requested before the scalar phase) up to 2 048 poses and 2 048 coarse unknowns, TWO beyond (scalars,
                              t and y = A_c^-1 t once, in k_xcg_f2_coarse); 2: always two; 0: three launches per iteration.
                              A breakdown of the recurrences repeats the solve in the three-launch form
     "band_chol"          [1; 0 / 1] explicit two-level PCG: banded factorisation + band substitutions for the coarse inverse when A_c
                              has at most 7 block off-diagonals (chain-like problems); 0: always the dense factorisation
     "solve_horizon"      [-1 unknown; below 0 is -1, else truncated, at most 1e6] how many more whole-iteration calls the caller's stopping rule allows if the step about to be
                              taken turns out non-decreasing (reference problem.py:163-178); side work that pays back only over
                              several later calls (the lagged inverse's seed) is not started with fewer than three to come
     "expect_next"        [0; 0 / 1, always 0 on a hybrid handle] the caller will ask for another whole iteration after the coming one unless a stopping rule on ||dx|| or
                              the cost fires (ps_solve sets it for its own loop): with "fuse_cost" the coming call's tail runs the NEXT
                              iteration's landmark pass in place of its cost pass -- every observation evaluated once per iteration;
                              the next call's linearisation takes the pass over if the parameters have not moved since.  Does not
                              invalidate what was computed ahead (every other option does)
     "fuse_cost"          [1; any] the cost of all blocks summed by the packed landmark pass itself (tails that expect a successor, the start
                              cost of ps_solve, ps_eval_cost) or by a cost-only pass in the same structure: the same number bit for bit;
                              2: in the tails only; 0: the grid-stride cost pass of rounds 1-4 everywhere (another summation order).
                              Needs every observation on a variable landmark with at most 16 observations, else 0 is what runs
     "cg_persist"         [1; 0 / 1] the folded two-level CG in ONE launch (csrc/ps_k_cg_persist.h) where the augmented system fits (<= 2 048
                              unknowns, <= 1 024 tasks); 0: one launch per CG iteration.  "cg_persist_spin" [200000; 0 .. 1e7]: passes over the
                              in-launch exchange before a workgroup gives up -- or one second, whichever comes first -- (then the solve is
                              repeated launch by launch and the form is not used on the handle any more:
                              ps_problem_info.cg_persist_failures).  The form is only used when its whole grid can be resident on the
                              compute units the handle's stream may use (device count, stream CU mask, occupancy of the kernel:
                              ps_problem_info.persist_cus / persist_cus_needed) and while one-launch solves of other handles of the
                              process leave them free (cg_persist_refused)
     "xcg_persist"        [1; 0 / 1] the explicit two-level PCG of bundle adjustments (long rows, one workgroup per compute unit of the stream: up to 2 048 poses on a whole MI355X) in ONE
                              launch per solve (csrc/ps_k_xcg_persist.h): matrix in registers / LDS, w, partials and records exchanged
                              in-launch; 0: one launch per iteration (k_xcg_fused1).  Time-outs as "cg_persist"
     "pose_xcd"           [1; 0 / 1] the pose pass's work items in eight contiguous ranges, one per XCD (0: item = workgroup); speed only
     "lin_zero_list"      [1; 0 / 1] a linearisation zeroes only what it accumulates into -- the diagonal blocks of S, blocks a factor or a host
                              row adds into, pattern blocks no Schur pair writes, g, the cost and status words -- from trailing
                              workgroups of the pose pass; every other block is stored by the pair kernel.  Live on a handle with the
                              untiled pipelined pair kernel ("schur_pipeline"), SE(3) poses and no landmark shard (ps_get_option tells);
                              every other handle, and 0, keep the fill over all of [S | g | cost | status].  Speed only
     "setup_ride"         [1; 0 / 1] the block-Jacobi factors that head the fused CG's set-up (L_i^-1, g^, the zeroed CG vectors, the coarse
                              basis blocks) are formed by the waves of the Schur pair launch that finalise the diagonal blocks, and the
                              kernel of their own is launched only for further set-ups on the same linearisation.  Live on a handle
                              whose finalisation is in the pair launch (untiled pipelined pair kernel, SE(3) poses, no landmark observed
                              twice from one pose), without pose-to-pose factors or host rows, that is no landmark shard and whose
                              reduced system the fused CG takes (not the direct solve, the explicit or the classic PCG); ps_get_option
                              tells.  Every other handle, and 0, launch the factor kernel in every set-up.  Speed only, same bits.
                              Handled ahead of the option table, as "expect_next" and "solve_horizon" are
     "rows_regs"          [1; 0 / 1] the scaled-block products of the fused CG's set-up (S^ = L_i^-1 S_ij L_j^-T, S^ B) by one thread per
                              block row in registers; the lagged set-up forms K_i only over the coarse nodes its row reaches; and where
                              the lagged set-up applies, the exact set-up's block scaling and coarse row sums are one launch of the rows
                              kernel.  0: one wave per block through LDS, the two launches.  Speed only, same bits.  Handled ahead of
                              the option table
     "cg_persist_recover" [1; 0 / 1] the one-launch folded CG ("cg_persist") recovers x = L^-T (x^_f + P y) inside the launch, every workgroup
                              its own slice of poses from operands it copied into LDS at kernel entry, when the largest slice's
                              operands fit "cg_persist_recover_lds" [146432; 0 .. 146432 bytes of dynamic LDS: what one workgroup per
                              compute unit leaves free]; else, and with 0, the gated k_coarse_recover runs behind the launch.  Speed
                              only, same bits.  Both handled ahead of the option table
     "packed_prefetch"    [1; 0 / 1] the packed landmark pass, cost pass and back-substitution ("lm_packed") read their wave's run from one
                              16-byte record (built beside the run starts at create time) and request their operands in four
                              dependent trips to memory -- record + gate word; the lane's row + the run's landmark starts; the gathers
                              the row names (x of its pose, pose, point, the whole observation-group record) + the head lane's point
                              index; the point with the head lane's C^-1 and c -- instead of seven.  0: the load order they had
                              before.  Speed only, same bits.  Handled ahead of the option table
     "pose_prefetch"      [1; 0 / 1] the pose pass (items of at most 512 observations: every handle of the product library) requests both
                              observations of a thread, then their point / C^-1 / c gathers with the whole observation-group record,
                              evaluates each down to twelve numbers and forms its 33 sums only at the end; the six damping sums are
                              compiled out of the launches with lambda = 0.  Under 128 registers there: four waves per SIMD instead of
                              three.  0: k_pose_pass, one observation after the other.  Speed only, same bits.  Handled ahead of the
                              option table
     "coarse_chol_band"   [1; 0 / 1] coarse levels of at most 90 unknowns: the factorisation of A_c = P^T S^ P leaves out the blocks that the
                              pattern makes structurally zero (k_coarse_chol_band with the block half-bandwidth the coarse-level
                              planner derived from the run tables -- ps_get_option "coarse_chol_bw"; ncb - 1, the dense matrix,
                              where a loop closure spans the trajectory), on the solver stream and on the side stream.  0:
                              k_coarse_chol on every launch.  Speed only, same bits.  Handled ahead of the option table
     "schur_pipeline"    [1; 0 / 1] the Schur pair kernel with two chunks per wave in flight (k_schur_pairs_db); 0: k_schur_pairs
     "lm_packed" [1; 0 / 1], "band_part" [1; 0 / 1], "band_part_chunk" [0 auto; 0 .. 4096 nodes], "sync_refactor" [1; 0 / 1],
     "hold_across_steps" [1; 0 / 1]: round-5 kernels and schedules against their predecessors (DESIGN.md sections 0 and 3)
     "cg_force_restart"   [0; 0 / 1] tests: end the first pass of a synchronous reduced solve at 1e-4 and restart from the true residual
     "cg_force_breakdown" [0; integer] tests: n > 0 arms ONE forced breakdown -- in the first pass of the next reduced solve that sets
                              up the folded CG or the explicit two-level PCG, CG iteration n - 1 reads a negative delta (a one-thread-
                              block kernel overwrites it in front of that launch), finds denom <= 0 through its own branch and sets
                              the breakdown flag; the host then takes its fallback.  That one pass runs launch by launch (never a
                              one-launch-per-solve form, which takes no host step between iterations).  The set-up of that solve
                              clears the option (ps_get_option reads it back), so the repeat runs untouched.  The three- and
                              four-launch forms of the explicit PCG have no such branch: they consume the option and run as usual.
                              Setting it invalidates nothing that was computed ahead
     "cg_lds"             [1; 0 / 1] small systems: the fused CG with the whole vector through LDS (k_cg_fused_lds)
     "big_chol"           [1; 0 / 1] coarse matrices of more than 90 unknowns: the blocked factorisation over many workgroups; 0: one workgroup
     "profile_every"      [1; >= 1] profiling level 1 times the Schur kernel of every n-th linearisation only
     "cg_margin"          [4; 0 .. 64] CG launches enqueued beyond the previous solve's iteration count
     "pcg_chunk"          [8; 1 .. 4096] launch-per-iteration solves: launches between two host polls of the 'done' flag
     "cg_split_min_rows"  [1024; any] more reduced poses than this: the coarse rows in a kernel of their own (split mode; the threshold
                              below is never above this one), and
     "cg_explicit_min_rows" [-1; any] ... the explicit two-level PCG instead of the folded one (-1: 400 poses for pose-graph rows, 540 for
                              bundle-adjustment rows, 250 where the lagged inverse cannot apply).  Either has the coarse level planned again
     "cg_ablate", "schur_ablate", "lm_ablate" [0; any]: timing experiments of the measurement build only (results are wrong under
                              ablation); the product build accepts 0 and refuses every other value */
int ps_set_option(ps_problem* h, const char* name, double value);
/* What an option comes to on this handle.  "lin_zero_list": 1 if linearisations zero by the list, 0 if they keep the fill;
   "lin_zero_launches" / "lin_fills": linearisations so far that did the one / the other.
   "setup_ride": 1 if the pair launch also forms the block-Jacobi factors on this handle, else 0; "factors_ridden": linearisations
   so far that did; "factor_launches": set-ups of the fused CG that launched the factor kernel themselves; "factor_plan_mismatches":
   those among them that found ridden factors made for another set-up plan (lagged / exact, coarse buffer) than their own.
   "rows_regs": the option; "rows_setups": lagged set-ups launched so far (k_rows_setup); "exact_row_setups": exact set-ups so far
   whose block scaling and row sums were the rows kernel's one launch; "rows_lci_in_lds": 1 if the rows kernel holds the lagged
   coarse factor in LDS on this handle (0 before the coarse level is built, and where the lagged set-up does not apply).
   "cg_persist_recover", "cg_persist_recover_lds": the options; "cg_persist_recover_need": bytes of LDS the largest slice's operands
   take on this handle (0 before the coarse level is built, and where the one-launch folded CG does not apply);
   "cg_persist_recovered" / "cg_persist_recover_fallbacks": one-launch solves so far (ps_problem_info.cg_persist_solves) that recover
   x inside the launch / that leave it to k_coarse_recover behind the launch.
   "packed_prefetch", "pose_prefetch", "coarse_chol_band": the options.  "coarse_chol_bw": the block half-bandwidth of the coarse
   matrix on this handle, 0 .. ncb - 1 (ncb - 1: no band; -1 before the coarse level is built and without one); "coarse_nodes": ncb,
   the coarse nodes of this handle (0 before the coarse level is built and without one). */
int ps_get_option(ps_problem* h, const char* name, double* value);

/* hipEvent stage timers on the handle's stream (the reference has no tracing). */
int ps_set_profiling(ps_problem* h, int enabled);
int ps_get_stage_times(ps_problem* h, double* ms /* PS_NUM_STAGES */, int64_t* counts, int reset);

/* Host-evaluated generic path (user-defined Python residual blocks): dense
   J (m x n, row-major) and r are uploaded, the device forms J^T J, -J^T r and
   solves by Cholesky; optionally returns the inverse (compute_covariance,
   pyslam/problem.py:196-203). */
int ps_dense_normal_solve(const double* J, const double* r, int32_t m, int32_t n,
                          double* dx, double* covariance /* n*n or NULL */);

/* The same path beyond the dense solver's size: J (m x n) and its transpose as CSR in HBM, Jacobi-preconditioned CG
   on J^T J dx = rhs without forming J^T J; rhs = -J^T r (a Gauss-Newton step; `rhs` NULL) or the caller's `rhs`
   (a unit vector: one covariance column; `r` may then be NULL).  Replaces scipy's sparse LU (pyslam/problem.py:186)
   for problems with user-defined blocks / losses / parameters and more than 2048 unknowns.  Stops at a relative
   preconditioned residual of `tol` or after max_iters iterations (the step is returned either way). */
int ps_sparse_normal_solve(int32_t m, int32_t n, const int32_t* j_row_ptr, const int32_t* j_col, const double* j_val,
                           const int32_t* jt_row_ptr, const int32_t* jt_col, const double* jt_val,
                           const double* r, const double* rhs, double tol, int32_t max_iters,
                           double* dx, int32_t* iters_out, double* relres_out);

/* The same system solved DIRECTLY (round 5): J^T J formed dense on the device, blocked multi-workgroup Cholesky, block
 * substitutions, `refine_steps` refinement steps on the residual of the original system.  n <= 8192.  What the host-evaluated path
 * uses between the single-workgroup dense solve (n <= 2048) and the CG above; stands in for scipy.sparse.linalg.spsolve
 * (reference pyslam/problem.py:186).  relres_out: ||rhs - J^T J dx|| / ||rhs||. */
int ps_sparse_normal_direct(int32_t m, int32_t n, const int32_t* j_row_ptr, const int32_t* j_col, const double* j_val,
                            const int32_t* jt_row_ptr, const int32_t* jt_col, const double* jt_val,
                            const double* r, const double* rhs, int32_t refine_steps, double* dx, double* relres_out);

/* The banded factorisation kernels of the explicit two-level PCG's coarse level on their own (csrc/ps_k_band.h: one workgroup
 * walking the block columns; csrc/ps_k_bandpart.h: the partitioned, parallel form): inverse of a symmetric positive definite
 * matrix with `bw` (1..7) block off-diagonals of dof x dof blocks.  `a`: dense, row-major, (ncb dof)^2 doubles on the host, lower
 * triangle read.  chunk_nodes < 0: serial walk; 0: partitioned, automatic chunk size; > 0: interior nodes per chunk (partitioned
 * needs 2 bw - 1 <= 7).  ainv_out: fp32, what the preconditioner keeps.  elapsed_us (or NULL): GPU time of the launches.
 * Stands in for the coarse-level part of scipy.sparse.linalg.spsolve (reference pyslam/problem.py:186); test and measurement entry. */
int ps_debug_band_inverse(const double* a, int32_t ncb, int32_t dof, int32_t bw, int32_t chunk_nodes, float* ainv_out,
                          double* elapsed_us);
/* The LDS-resident coarse factorisation kernels on their own (csrc/ps_k_coarse.h): one launch of k_coarse_chol (variant 0) or of
 * k_coarse_chol_band (variant 1: as the solver launches it; 64 .. 1024 in steps of 64: with that many threads) on a host matrix
 * `a` (dense, row-major, (ncb dof)^2 doubles, ncb dof <= 90, dof 3 or 6), on a stream of its own.  bw: block half-bandwidth handed
 * to the band kernel, 0 .. ncb - 1 (outside it `a` must hold +0.0; variant 0 ignores it).  Li, LiT: L^-1 and its transpose, whole,
 * zeros above / below the diagonal (an entry the kernel did not write comes back as NaN).  status: the 8 status words (word 1: non-
 * positive or NaN pivots).  elapsed_us (or NULL): GPU time of a second launch, between events.  Test and measurement entry; no
 * solver path calls it.  ps_debug_coarse_chol_clocks (measurement build; the product build refuses): six stamps of the kernel's
 * thread 0 in microseconds from kernel entry -- entry, band loaded, factor loop done, diagonal inverses done, doubling levels done,
 * outputs stored. */
int ps_debug_coarse_chol(const double* a, int32_t ncb, int32_t dof, int32_t bw, int32_t variant, double* Li, double* LiT,
                         int32_t* status, double* elapsed_us);
int ps_debug_coarse_chol_clocks(const double* a, int32_t ncb, int32_t dof, int32_t bw, int32_t variant, double* clocks);
/* The blocked dense factorisation chain on its own (csrc/ps_host_bchol.h: bchol_chain, the one launch sequence behind the coarse
 * level beyond 90 unknowns, the lagged inverse's direct seed, ps_covariance_marginals and ps_sparse_normal_direct; kernels
 * k_bchol_panel / k_bchol_update / k_btri_inverse / k_btri_merge / k_btri_clear and k_xcg_ainv).  Test and measurement entries;
 * no production path calls them.
 * ps_debug_dense_factor: `a` is a symmetric positive definite matrix on the host, n x n row-major, n <= 8192; the lower triangle
 *   is read.  Runs the chain as production does, on a stream of its own, and returns every stage (any out pointer may be NULL):
 *   l_out (n x n): the working matrix, L below the 24 x 24 diagonal tiles (the tiles themselves and the upper triangle keep A: the
 *   tiles' factors are never written back); tinv_out (ceil(n / 24) tiles of 24 x 24, lower triangular, zero-padded): the inverses
 *   of the diagonal tiles' factors; li_out, lit_out (n x n): L^-1 and its transpose; ainv_out (n x ld floats): A^-1 in fp32, both
 *   triangles; diag_fail: the count of non-positive (or NaN) pivots -- with diag_fail NULL such a matrix is an error instead;
 *   elapsed_us: GPU time of the chain's launches (second of two runs).
 *   flags bit 0: the folded CG's dense-output form (zero fill, k_btri_clear: the strict upper triangle of li_out and the strict
 *   lower triangle of lit_out are zero); without it the explicit PCG's form, where li_out outside its lower triangle and the
 *   192 x 192 diagonal blocks (lit_out: outside the upper triangle and those blocks) is unspecified and comes back as NaN, the
 *   entry's pre-fill.  flags bits 8..15: ld = n + that many columns; ainv_out's contents go in, and what k_xcg_ainv leaves alone
 *   (the columns from n on) comes back unchanged.
 * ps_debug_bchol_slab: host only, no device needed.  Which rows of a panel of m rows and w (1..24) columns workgroup `block` of
 *   k_bchol_panel owns, found by walking its 256 threads x 4 entries through the kernel's own mapping function (ps_bchol_slab,
 *   csrc/ps_k_coarse.h): rows [row_lo, row_hi), `entries` cells, `grid` workgroups in the launch.  A workgroup owns whole rows:
 *   the panel is factored in place, and a row shared between two workgroups would be read by one while the other overwrites it. */
int ps_debug_dense_factor(const double* a, int32_t n, int32_t flags, double* l_out, double* tinv_out, double* li_out, double* lit_out,
                          float* ainv_out, int32_t* diag_fail, double* elapsed_us);
int ps_debug_bchol_slab(int32_t m, int32_t w, int32_t block, int32_t* row_lo, int32_t* row_hi, int32_t* entries, int32_t* grid);
/* The lagged dense inverse's kernels on their own (csrc/ps_k_ldi.h; option "lagged_inverse"): test entries that run the
 * production kernels and change nothing in them; no production path calls them.
 * ps_debug_ldi_gemm: C = alpha A B + beta Dm + gamma I by the fp32 MFMA product k_ldi_gemm, launched exactly as the Newton-Schulz
 *   steps launch it.  Host arrays, row-major: A (M x lda), B (K x ldb), Dm (M x ldd, or NULL; may be the pointer A itself: the
 *   device copies alias as well), C (M x ldc; its contents go in, tiles the kernel leaves alone come back unchanged).  krange (or
 *   NULL): [k_lo, k_hi) per 32-row tile, 2 (M / 32) ints.  upper_only: tiles below the diagonal stay untouched.  dev_scale (or NULL):
 *   one float that multiplies alpha and gamma on the device.  fro_part (or NULL): (M / 32) (N / 32) doubles, pre-filled with
 *   fro_sentinel, the sum of squares of every tile written.  Refused before any launch: M or N not a multiple of 32, K or a
 *   krange bound not a multiple of 16, a leading dimension below its extent or (lda, ldb) not a multiple of 4.
 * ps_debug_ldi_ritz: the seed scale kernel k_ldi_ritz on rz[k] = r_k . z_k and alpha[k], k < m, of a CG of m iterations (the first
 *   64 are used).  out3 = c, ritz_min, ritz_max; all zero when there is no usable estimate.
 * ps_debug_ldi_read: one item of a live handle's inverse as doubles, after waiting for every stream that writes it; the state
 *   machine does not move.  PS_LDI_READ_STATE (12 doubles: state [0 none, 1 seed in flight, 2 valid, 3 valid + refresh in flight],
 *   buffer in use or -1, n, np, kp, direct seed 0 / 1, the residual bound the inverse in flight / in use was accepted under, CG
 *   iterations of the last solve with it, "ldi_seed_steps", block rows, dof, buffers allocated 0 / 1) always answers; every other
 *   item is an error until an inverse has been seeded: S32, X32, XU (the buffer in use), np x np; XT np x kp; LINV block rows x
 *   dof x dof (the frozen factors); COEF 3; FRO 1 (||I - S^ X||_F^2 of the last step); R, Z: n (the residual the last k_ldi_init /
 *   k_ldi_update stored and z = X_u r, valid straight after a call that solved with the inverse). */
enum { PS_LDI_READ_STATE = 0, PS_LDI_READ_S32 = 1, PS_LDI_READ_X32 = 2, PS_LDI_READ_XU = 3, PS_LDI_READ_XT = 4, PS_LDI_READ_LINV = 5,
       PS_LDI_READ_COEF = 6, PS_LDI_READ_FRO = 7, PS_LDI_READ_R = 8, PS_LDI_READ_Z = 9 };
int ps_debug_ldi_gemm(int32_t M, int32_t N, int32_t K, float alpha, const float* A, int32_t lda, const float* B, int32_t ldb, float beta,
                      const float* Dm, int32_t ldd, float gamma, float* C, int32_t ldc, const int32_t* krange, int32_t upper_only,
                      const float* dev_scale, double fro_sentinel, double* fro_part);
int ps_debug_ldi_ritz(const double* rz, const double* alpha, int32_t m, float* out3);
int ps_debug_ldi_read(ps_problem* h, int32_t what, double* out, int64_t capacity);
/* Stress entry behind DESIGN.md section 3 "side stream" (round 6; test and measurement infrastructure): the coarse level's
 * factorisation kernels run `launches` times on a stream of their own -- lowest priority if `lowprio` -- while, if `aggressor`,
 * streaming copy kernels keep an ordinary stream busy; every output is compared bit for bit with one produced on an idle device.
 * mode 0: serial band walk (k_band_chol + k_band_inverse_rl); 1: partitioned band factorisation (BandPart); 2: dense LDS-resident
 * k_coarse_chol + k_xcg_ainv (ncb dof <= 90); 3: the same with its matrices in global scratch; 4: the blocked chain (bchol_chain:
 * k_bchol_panel / k_bchol_update / k_btri_inverse / k_btri_merge) + k_xcg_ainv on a working copy, any ncb dof, `bw` ignored; + 8: the input is produced on the
 * same stream by a copy kernel in front of every factorisation (the buffer holds 2 A before); + 16: with an event recorded in
 * between.  `a` as ps_debug_band_inverse.
 * -> n_diff: launches whose fp32 inverse differs from the reference in any bit; n_pivot: launches that reported a non-positive
 * pivot on this positive definite input.  A kernel that is a function of its input gives 0 / 0 whatever runs beside it. */
int ps_debug_factor_stress(const double* a, int32_t ncb, int32_t dof, int32_t bw, int32_t mode, int32_t launches, int32_t lowprio,
                           int32_t aggressor, int32_t* n_diff, int32_t* n_pivot);

/* Frame-to-frame RANSAC, the step before the motion-only solve in the reference's sparse VO pipeline
   (pyslam/pipelines/sparse.py:148-150).  Stateless; host pointers in, host pointers out.
   ps_ransac_transforms   -- compute_transform_fast (pyslam/pipelines/ransac.py:13-67): `batch` rigid
                             alignments p_2 ~ C p_1 + r of n-point sets (pts: batch x n x 3), 4x4 out.
   ps_ransac_cost         -- FrameToFrameRANSAC.compute_ransac_cost (:153-165): inlier masks
                             (num_hyp x num_pts bytes) and counts of given 4x4 transforms; cam5 = cu cv fu fv b.
   ps_ransac_frame_to_frame -- perform_ransac (:113-151) without the random draw: hypotheses from the
                             caller's sample indices (num_hyp x set_size), scoring of all points, first
                             hypothesis with the most inliers, its transform and inlier mask. */
int ps_ransac_transforms(const double* pts_1, const double* pts_2, int32_t batch, int32_t n, double* T_out);
int ps_ransac_cost(const double* T, int32_t num_hyp, const double* pts_1, const double* obs_2, int32_t num_pts,
                   const double* cam5, double thresh, uint8_t* masks, int32_t* counts);
int ps_ransac_frame_to_frame(const double* pts_1, const double* pts_2, const double* obs_2, int32_t num_pts,
                             const int32_t* sample_idx, int32_t num_hyp, int32_t set_size, const double* cam5,
                             double thresh, double* T_all, int32_t* counts, int32_t* best_index,
                             int32_t* best_count, double* T_best, uint8_t* best_mask);

/* Monocular two-view initialisation: essential-matrix RANSAC on 2-D - 2-D correspondences (pyslam_amd/pipelines/twoview.py;
   the definition, the sign rule, the candidate order and the tie rules: pyslam_amd/csrc/ps_k_twoview.h, restated in numpy by
   pyslam_amd/pipelines/epipolar.py).  Stateless; host pointers in, host pointers out.  obs_1, obs_2: (num_pts, 2) pixels;
   cam5 = cu cv fu fv b (b is not read); sample_idx: (num_hyp, 8) point indices, drawn by the caller; thresh: squared Sampson
   distance in pixels^2.  Two calls on the same input are bit-identical.
   ps_twoview_hypotheses -- per sample the eight-point essential matrix E (row-major 3 x 3, x_2^T E x_1 = 0, singular values
                            1 1 0, largest entry positive), its inlier count and its degenerate flag (a repeated index or a
                            rank-deficient sample: E = 0, count 0, flag 1).
   ps_twoview_score      -- inlier masks (num_hyp x num_pts bytes) and counts of given matrices.
   ps_twoview_ransac     -- the whole chain with one synchronisation: hypotheses, the first one with the most inliers, its mask,
                            the refit over its inliers (refit != 0; kept when its count is not lower), decomposition and cheirality
                            vote.  T_21 (4 x 4, |t| = 1), E_out (9), mask (num_pts), parallax_deg (num_pts, 0 outside the inliers),
                            info (8): best index, its count, final count, refit kept, the four candidates' cheirality counts. */
int ps_twoview_hypotheses(const double* obs_1, const double* obs_2, int32_t num_pts, const int32_t* sample_idx, int32_t num_hyp,
                          const double* cam5, double thresh, double* E_all, int32_t* counts, uint8_t* degenerate);
int ps_twoview_score(const double* E, int32_t num_hyp, const double* obs_1, const double* obs_2, int32_t num_pts,
                     const double* cam5, double thresh, uint8_t* masks, int32_t* counts);
int ps_twoview_ransac(const double* obs_1, const double* obs_2, int32_t num_pts, const int32_t* sample_idx, int32_t num_hyp,
                      const double* cam5, double thresh, int32_t refit, double* T_21, double* E_out, uint8_t* mask,
                      int32_t* info, double* parallax_deg);

/* Absolute pose (PnP): registration of a monocular frame against the map by P3P RANSAC on 2-D - 3-D correspondences
   (pyslam_amd/pipelines/pnp.py; the definition, the slot order, the emptiness, degeneracy and tie rules: pyslam_amd/csrc/ps_k_pnp.h,
   restated by pyslam_amd/pipelines/absolute.py).  Stateless; host pointers in, host pointers out.  pts_w: (num_pts, 3) landmarks in
   the map frame; obs: (num_pts, 2) pixels; cam5 = cu cv fu fv b (b is not read); sample_idx: (num_hyp, 3) point indices, drawn by
   the caller; thresh: squared reprojection error in pixels^2; poses are row-major 4 x 4 with p_c = R p_w + t.  num_pts >= 3.  Two
   calls on the same input are bit-identical.
   ps_pnp_hypotheses -- per sample the four slots of Grunert's quartic in the fixed root order: T_all (num_hyp x 4 x 16), counts
                        (num_hyp x 4), empty (num_hyp x 4 bytes: bit 0 the slot is empty -- T = 0, count 0 --, bit 1 the whole
                        sample is degenerate: a repeated index, a collapsed triangle or a non-finite row).
   ps_pnp_score      -- inlier masks (num_T x num_pts bytes) and counts of given poses T (num_T x 16).
   ps_pnp_ransac     -- the whole chain with one synchronisation: hypotheses, the first one with the most inliers (its first such
                        slot), its mask, refine_iters Gauss-Newton iterations over its inliers (kept when no pivot failed, the count
                        is not lower and the pose is finite; 0: none).  T_cw (16), mask (num_pts), sq_err (num_pts: the final pose's
                        squared errors), cost_history (refine_iters + 1: before every iteration and after the last), info (8): best
                        hypothesis, its slot, raw count, final count, refinement kept, a pivot failed, iterations run, 0. */
int ps_pnp_hypotheses(const double* pts_w, const double* obs, int32_t num_pts, const int32_t* sample_idx, int32_t num_hyp,
                      const double* cam5, double thresh, double* T_all, int32_t* counts, uint8_t* empty);
int ps_pnp_score(const double* T, int32_t num_T, const double* pts_w, const double* obs, int32_t num_pts, const double* cam5,
                 double thresh, uint8_t* masks, int32_t* counts);
int ps_pnp_ransac(const double* pts_w, const double* obs, int32_t num_pts, const int32_t* sample_idx, int32_t num_hyp,
                  const double* cam5, double thresh, int32_t refine_iters, double* T_cw, uint8_t* mask, int32_t* info,
                  double* sq_err, double* cost_history);

/* Similarity (Sim(3)) alignment: robust 7-DoF alignment of two matched 3-D point sets by RANSAC over Umeyama fits of three pairs --
   a monocular map against a second map, a trajectory against ground truth, two keyframes that see the same landmarks
   (pyslam_amd/pipelines/sim3.py; the definition, the degeneracy, tie and refit rules: pyslam_amd/csrc/ps_k_sim3.h, restated by
   pyslam_amd/pipelines/similarity.py).  Stateless; host pointers in, host pointers out.  pts_1, pts_2: (num_pts, 3); the model is
   p_2 = s R p_1 + t, stored row-major 4 x 4 as [s R | t; 0 0 0 1] with the scalar s beside it.  cam5 = cu cv fu fv b (b is not read)
   selects the PIXEL mode: obs_1, obs_2 (num_pts, 2) are the pixels of the points in their own cameras, thresh is in pixels^2 on the
   larger of the two squared reprojection errors, and both depths must be positive.  cam5 == NULL selects the METRIC mode: obs_1 and
   obs_2 must be NULL, thresh is on |s R p_1 + t - p_2|^2 (+inf: every finite pair).  sample_idx: (num_hyp, 3) point indices, drawn by
   the caller; fixed_scale: 1 holds s = 1 (maps with a metric scale), else 0; num_pts >= 3; thresh > 0.  Two calls on the same input
   are bit-identical.
   ps_sim3_hypotheses -- per sample S_all (num_hyp x 16), scales, counts, flags (num_hyp bytes; 1: the sample is degenerate --
                         collinear or repeated points, a non-finite row, a scale that is not positive: S = 0, scale 0, count 0).
   ps_sim3_score      -- inlier masks (num_S x num_pts bytes) and counts of given models S (num_S x 16).
   ps_sim3_ransac     -- the whole chain with one synchronisation: hypotheses, the first one with the most inliers, its mask, up to
                         refit_iters (0..1000) rounds of a fit over all current inliers and a rescoring.  S_21 (16), scale, mask
                         (num_pts), sq_err (num_pts: the final model's errors; +inf when it is degenerate), info (8): best hypothesis,
                         raw count, final count, rounds adopted, how the loop ended (0: every round ran, 1: a round with fewer inliers
                         was discarded, 2: a round reproduced its mask, 3: a degenerate round was discarded), 1 when the result is
                         degenerate, 0, 0. */
int ps_sim3_hypotheses(const double* pts_1, const double* pts_2, const double* obs_1, const double* obs_2, int32_t num_pts,
                       const int32_t* sample_idx, int32_t num_hyp, const double* cam5, double thresh, int32_t fixed_scale,
                       double* S_all, double* scales, int32_t* counts, uint8_t* flags);
int ps_sim3_score(const double* S, int32_t num_S, const double* pts_1, const double* pts_2, const double* obs_1, const double* obs_2,
                  int32_t num_pts, const double* cam5, double thresh, uint8_t* masks, int32_t* counts);
int ps_sim3_ransac(const double* pts_1, const double* pts_2, const double* obs_1, const double* obs_2, int32_t num_pts,
                   const int32_t* sample_idx, int32_t num_hyp, const double* cam5, double thresh, int32_t fixed_scale,
                   int32_t refit_iters, double* S_21, double* scale, uint8_t* mask, int32_t* info, double* sq_err);

/* Sim(3) pose graph: what consumes a verified loop constraint (definition: DESIGN.md section 7; restatement:
   pyslam_amd/pipelines/simgraph.py; kernels: csrc/ps_k_sim3pg.h).  A stand-alone handle with kernels of its own; the core's
   D = 3 / 6 solver is not involved.
   Element: 13 doubles [R row-major (9) | t (3) | s], s > 0, p -> s R p + t.  Tangent [rho | phi | sigma]; update S <- exp(dx) S.
   Edge (i, j, S_ji, W): r = W log(S_j S_i^-1 S_ji^-1) with a 7 x 7 stiffness W (edge_stiffness49 NULL: identity; an all-zero row
   is an absent row), J_i = -W Ad(S_j S_i^-1), J_j = W, the robust loss per component as the pose factors of the core apply it,
   with one exception: L1's IRLS weight is 1 / max(|r_k|, 1e-8) here (the core's is NaN within 1e-8 of zero) -- the edges of a loop
   correction start at zero residual, and an L1 solve converges to zero components; the cost stays |r_k|.
   held[v] != 0: vertex v contributes no unknowns (at least one must be held; an edge between two held vertices adds cost only).
   The system is DENSE, n = 7 free vertices <= 8192, solved by the blocked Cholesky chain with one refinement step; a larger
   graph, an index out of range, i == j, a non-finite input and a non-positive pivot are errors.
   create:     host tables in; `stream` as everywhere (NULL: the default stream).
   eval_cost:  the cost at the current vertices, summed in a fixed order (bit-reproducible).
   linearize:  H_out (n x n, diagonal times 1 + lambda, both triangles), g_out (n; H dx = g), cost; any out pointer may be NULL.
   iteration:  linearise, factor, solve, refine, retract, cost after the step; relres: ||g - H dx|| / ||g|| after the refinement.
   solve:      the loop of Problem.solve under the linesearch != 0 meaning (an iteration's cost is the cost after its step) with
               csrc/ps_stop_rule.h and options->lm_lambda as the fixed damping; cost_history needs max_iters + 2 entries.
   debug_edges / debug_explog: test entries -- the edge kernel's tap, 105 doubles per edge: scaled residual (7), scaled J_i (49),
               scaled J_j (49); the device exp, log of that and adjoint of that on a host table of n tangent vectors.
   profile:    measurement entry -- enable != 0 times the stages of later iterations with events; stage_ms5 (or NULL): the last
               iteration's edges, assemble, factor, substitute + refine, retract + cost, in ms. */
typedef struct ps_sim3pg ps_sim3pg;
int ps_sim3pg_create(int32_t num_vertices, const double* vertices13, const uint8_t* held, int32_t num_edges, const int32_t* edge_i,
                     const int32_t* edge_j, const double* edge_obs13, const double* edge_stiffness49, int32_t loss_id, double loss_k,
                     void* stream, ps_sim3pg** out);
int ps_sim3pg_destroy(ps_sim3pg* h);
int ps_sim3pg_set_vertices(ps_sim3pg* h, const double* vertices13);
int ps_sim3pg_get_vertices(ps_sim3pg* h, double* vertices13);
int ps_sim3pg_eval_cost(ps_sim3pg* h, double* cost);
int ps_sim3pg_linearize(ps_sim3pg* h, double lambda, double* H_out, double* g_out, double* cost);
int ps_sim3pg_iteration(ps_sim3pg* h, double lambda, double* cost_after, double* dx_norm, double* relres);
int ps_sim3pg_solve(ps_sim3pg* h, const ps_solve_options* options, double* cost_history, int32_t cap, int32_t* n_history,
                    int32_t* iterations, double* last_dx_norm);
int ps_sim3pg_debug_edges(ps_sim3pg* h, double* tap105);
int ps_sim3pg_debug_explog(int32_t n, const double* xi_in, double* S13_out, double* xi_back, double* adj49_out);
int ps_sim3pg_profile(ps_sim3pg* h, int32_t enable, double* stage_ms5);

/* Dense photometric alignment: one SE(3) pose, one residual per reference pixel --
   PhotometricResidualSE3 (pyslam/residuals/photometric_residual.py:38-161) inside Problem's Gauss-Newton
   iteration with element-wise IRLS (pyslam/problem.py:279-360), as the dense VO pipeline runs it per pyramid
   level (pyslam/pipelines/dense.py:157-194).  The pixel tables are what the residual's constructor
   precomputes (:44-81); they are copied to the device at create time. */
typedef struct ps_photo ps_photo;
typedef struct ps_photo_desc {
    int32_t num_pixels;
    const double* pt_ref;        /* num_pixels x 3: triangulated reference points (:80) */
    const double* im_ref;        /* num_pixels: reference intensities */
    const double* im_jac;        /* num_pixels x 2: reference image gradient (dI/du, dI/dv) */
    const double* tri_jac_d;     /* num_pixels x 3: d point / d depth (column 2 of the triangulation Jacobian, :116) */
    int32_t height, width;       /* tracking image */
    const double* im_track;      /* height x width, row-major */
    double cam[5];               /* cu cv fu fv b */
    int32_t cam_type;            /* 0 stereo (u, v, disparity), 1 RGB-D (u, v, depth) */
    int32_t cam_w, cam_h;        /* validity bounds of the camera model (is_valid_measurement) */
    double intensity_covar, depth_covar;   /* stiffness^-2 (:57-58) */
    int32_t loss_id;             /* 0 L2, 1 L1, 2 Cauchy, 3 Huber, 4 Tukey, 5 t-distribution */
    double loss_k;
} ps_photo_desc;

int ps_photometric_create(const ps_photo_desc* desc, void* hip_stream, ps_photo** out);
int ps_photometric_destroy(ps_photo* h);
/* pose = T_track_ref as 12 doubles: R row-major, then t */
int ps_photometric_set_pose(ps_photo* h, const double* pose12);
int ps_photometric_get_pose(ps_photo* h, double* pose12);
/* sum of loss(r) over the valid pixels, and their number (evaluate() compresses invalid pixels away, :106) */
int ps_photometric_eval_cost(ps_photo* h, double* cost, int64_t* num_valid);
/* H = J~^T J~ (6 x 6, row-major), b = -J~^T r~, cost at the current pose (parity / debugging) */
int ps_photometric_normal_equations(ps_photo* h, double* H36, double* b6, double* cost, int64_t* num_valid);
/* One Gauss-Newton iteration: dx = H^-1 b in [translation; rotation] order, then
     split_params == 0: T <- exp(dx) T          (one SE3 parameter, liegroups perturb)
     split_params == 1: R <- exp(dx[3:6]) R, t += dx[0:3]   (separate SO3 / translation parameters, dense.py:185)
   cost: after the step when linesearch != 0 (Problem's degenerate line search always lands on the full step,
   pyslam/problem.py:362-398), else the cost of the linearisation point (:188-192). */
int ps_photometric_iteration(ps_photo* h, int32_t split_params, int32_t linesearch, double* dx6, double* cost);

/* Dense RGB-D visual odometry (reference pyslam/pipelines/dense.py, keyframes.py): image pyramids, keyframe pixel
   tables and the coarse-to-fine tracking of a frame against a keyframe, all on the device.  A handle holds
   num_slots frames of at most max_height x max_width, each with `levels` pyramid levels (the cv2.pyrDown chain,
   ((h+1)/2, (w+1)/2) per level); its device memory is fixed at create time.  Every frame of a handle has one size. */
typedef struct ps_dense ps_dense;
int ps_dense_create(int32_t levels, int32_t max_height, int32_t max_width, int32_t num_slots, void* hip_stream, ps_dense** out);
int ps_dense_destroy(ps_dense* h);
/* Upload a frame into a slot and build its image pyramid (dtype 0: uint8, 1: float64; row-major height x width).
   The float64 level images are raw / 255. (keyframes.py: compute_image_pyramid).  depth (float64, height x width,
   NaN / <= 0 = none) may come with the image or later with image == NULL.  No synchronisation: the caller keeps both
   buffers alive until its next synchronising call (ps_dense_track, a read). */
int ps_dense_upload(ps_dense* h, int32_t slot, int32_t dtype, int32_t height, int32_t width, const void* image, const double* depth);
/* Pixel tables of a keyframe slot for the listed levels, exactly as PhotometricResidualSE3's constructor builds them
   (ps_photo_desc): gradient 0.5 * Sobel, depth level depth[::2^l, ::2^l], RGBDCamera.is_valid_measurement on the
   level camera, |gradient| >= min_grad, kept pixels in raster order.  cams6: num_levels x (cu cv fu fv w h). */
int ps_dense_make_tables(ps_dense* h, int32_t slot, int32_t num_levels, const int32_t* levels, const double* cams6,
                         double intensity_covar, double depth_covar, double min_grad);
/* Track the frame in track_slot against the keyframe in ref_slot: for each listed level in order, Problem.solve's loop
   (options: max_iters, min_update_norm, min_cost, min_cost_decrease, allow_nondecreasing_steps, max_nondecreasing_steps,
   linesearch) on the level's PhotometricResidualSE3 with the (R, t) parameter split; rot_only[k] != 0 holds t constant
   (H[3:6,3:6] dphi = b[3:6], R <- exp(dphi) R).  The pose (T_track_ref, 12 doubles) carries from level to level on the
   device; one synchronisation per call.  iterations[k] and cost_history[k * history_cap + 0 .. iterations[k]] per level
   (history_cap >= max_iters + 2).  Errors as ps_photometric_iteration; pose12_out is then not written. */
int ps_dense_track(ps_dense* h, int32_t ref_slot, int32_t track_slot, int32_t num_levels, const int32_t* levels,
                   const int32_t* rot_only, const ps_solve_options* options, int32_t loss_id, double loss_k,
                   const double* pose12_in, double* pose12_out, int32_t* iterations, double* cost_history, int32_t history_cap);
/* Read back: level shape; a level's image (what 0, h x w), gradient (1, 2 x h x w: d/du then d/dv) or depth (2, h x w);
   the number of table pixels of a level and its tables (layout of ps_photo_desc). */
int ps_dense_level_shape(ps_dense* h, int32_t level, int32_t* height, int32_t* width);
int ps_dense_read_level(ps_dense* h, int32_t slot, int32_t level, int32_t what, double* out);
int ps_dense_num_pixels(ps_dense* h, int32_t slot, int32_t level, int32_t* num_pixels);
int ps_dense_read_tables(ps_dense* h, int32_t slot, int32_t level, int32_t num_pixels, double* pt_ref, double* im_ref,
                         double* im_jac, double* tri_jac_d);
/* device memory held by the handle */
int ps_dense_device_bytes(ps_dense* h, int64_t* bytes);

/* Feature matcher of the sparse VO pipelines (pyslam/pipelines/sparse.py; definition: DESIGN.md section 7, host
   restatement pyslam_amd/pipelines/featproc.py): corner features with 32-byte gradient descriptors and circular
   matching between the previous and the current frame, all on the device.  A handle holds three frames of at most
   max_height x max_width (one uint8 image, or a left / right pair) and at most max_features features per image; its
   device memory is fixed at create time. */
typedef struct ps_feat ps_feat;
typedef struct ps_feat_params {
    int64_t response_threshold;      /* a feature has R > response_threshold */
    int32_t nms_n;                   /* non-maximum suppression over (2 nms_n + 1)^2 pixels, 1..3 */
    int32_t max_features;            /* per image, <= the handle's; above it the strongest are kept */
    int32_t match_radius_u, match_radius_v;   /* temporal legs: |du| <= match_radius_u, |dv| <= match_radius_v */
    int32_t disp_max;                /* stereo legs: |dv| <= 1, 0 <= u_left - u_right <= disp_max */
    int32_t match_cost_max;          /* a best candidate above this sum of absolute differences is no match */
    int32_t refinement;              /* != 0: sub-pixel refinement (two-line fit of the costs at -1, 0, +1) */
    int32_t reserved;
} ps_feat_params;
int ps_feat_create(int32_t max_height, int32_t max_width, int32_t max_features, void* hip_stream, ps_feat** out);
int ps_feat_destroy(ps_feat* h);
/* The current frame becomes the previous one and (left, right or NULL) the current one.  A frame whose bytes equal a
   frame the handle holds (previous, current or the one cached beside them) is neither uploaded nor processed again.
   The images are copied before the call returns. */
int ps_feat_push(ps_feat* h, int32_t height, int32_t width, const uint8_t* left, const uint8_t* right);
/* mode 0 flow (previous left <-> current left), 1 stereo (current left <-> current right), 2 quad (previous left ->
   previous right -> current right -> current left -> previous left).  Computes the features of the frames that have
   none under these parameters, matches, and waits once for the number of matches. */
int ps_feat_match(ps_feat* h, int32_t mode, const ps_feat_params* params, int32_t* num_matches);
/* Matches of the last ps_feat_match, in the order of their first feature: matches8 = num_matches x (u1p v1p u2p v2p
   u1c v1c u2c v2c) (1 left, 2 right, p previous, c current; -1 where a mode has no such image), indices4 =
   num_matches x feature index (1p 2p 1c 2c; -1 likewise).  Either may be NULL. */
int ps_feat_read_matches(ps_feat* h, int32_t num_matches, double* matches8, int32_t* indices4);
/* Features of an image after a match (which: 0 previous left, 1 previous right, 2 current left, 3 current right), at
   most `capacity` of them: uv (2 x int32 each, raster order), response R, descriptors (32 bytes each).  Tests. */
int ps_feat_read_features(ps_feat* h, int32_t which, int32_t capacity, int32_t* num_features, int32_t* uv, int64_t* response,
                          uint8_t* descriptors);
/* Matching by projection (step 8 of the definition).  ps_feat_set_map uploads num_points (0 .. 2^20) map points -- points_w:
   num_points x 3 doubles in the world frame, descriptors: 32 bytes each, as ps_feat_read_features returns them -- to the handle,
   where they stay; its buffers are allocated at the first call and grow with num_points (a handle that never sets a map holds
   what it was created with).  ps_feat_match_map computes the features of the current frame's left image if it has none under
   these parameters, projects every point with T_cw (4 x 4, row-major) and cam5 = (cu, cv, fu, fv, b; b is not read), takes the
   best feature within `radius` pixels of the rounded projection, lets every feature go to one point only and refines the
   positions; it waits once, for the number of matched points and the results, which one copy brings to the host with it.
   ps_feat_read_map_matches hands them out without touching the device: one entry per map point, no compaction
   -- feature index or -1; status 0 matched, 1 not visible, 2 no candidate within match_cost_max, 3 lost its feature to a point
   with a lower (cost, index); cost, -1 unless the status is 0 or 3; uv (2 doubles), -1 unless the status is 0.  Any output may
   be NULL. */
int ps_feat_set_map(ps_feat* h, int32_t num_points, const double* points_w, const uint8_t* descriptors);
int ps_feat_match_map(ps_feat* h, const double* T_cw, const double* cam5, int32_t radius, const ps_feat_params* params,
                      int32_t* num_matched);
int ps_feat_read_map_matches(ps_feat* h, int32_t num_points, int32_t* feature, int32_t* status, int32_t* cost, double* uv);
/* Matching without a prior (step 9 of the definition): every point of the map against every feature of the current frame's left
   image (computed first if it has none under these parameters), no projection.  A point's best feature is the one with the lowest
   (cost, index); it is accepted when the cost is at most match_cost_max and ratio_den * cost < ratio_num * second-best cost
   (0 < ratio_num <= ratio_den <= 32768; a frame with one feature has no second-best cost and accepts).  Features then go to one
   point only and positions are refined as in ps_feat_match_map.  One wait; ps_feat_read_map_matches hands out feature / status /
   cost / uv of this match -- status 0 matched, 2 no feature within match_cost_max, 3 lost its feature, 4 ambiguous (cost kept,
   feature -1); 1 does not occur -- and ps_feat_read_map_second the second-best costs (-1 where there is none or the status is 2).
   Room for the second-best costs (4 bytes per point of the map's capacity) is allocated at the first global match
   (ps_feat_device_bytes grows by it then).
   ps_feat_read_map_second fails unless the last map match was a global one. */
int ps_feat_match_map_global(ps_feat* h, int32_t ratio_num, int32_t ratio_den, const ps_feat_params* params, int32_t* num_matched);
int ps_feat_read_map_second(ps_feat* h, int32_t num_points, int32_t* second);
/* The keyframe database (step 10 of the definition): an ordered list of entries, each num >= 0 descriptors of 32 bytes as
   ps_feat_read_features returns them.  ps_feat_db_add appends one entry and returns its index (num = 0 is allowed, descriptors may
   then be null; the caller's array is free on return); entries are never edited, ps_feat_db_clear empties the list and keeps the
   buffers.  At most 65536 entries and 2^22 descriptors.  Nothing is allocated before the first ps_feat_db_add; the buffers grow by
   doubling and are counted in ps_feat_device_bytes.
   ps_feat_db_query computes the features of the current frame's left image if it has none under `params` and writes
   scores[e - first], first <= e < last: the number of descriptors of entry e whose best cost over all features is at most
   match_cost_max and, where the frame has a second feature, satisfies ratio_den * best < ratio_num * second-best (what
   ps_feat_match_map_global gives status 0 or 3).  It counts descriptors of the entry, not distinct features of the frame.  One
   memset, one launch, one copy of last - first ints, one wait; two calls give the same bits.  first == last is a query of
   nothing.  Fails on a range outside 0 <= first <= last <= entries, on a ratio outside 0 < num <= den <= 32768, and without a
   pushed frame. */
int ps_feat_db_add(ps_feat* h, int32_t num, const uint8_t* descriptors, int32_t* entry);
int ps_feat_db_clear(ps_feat* h);
int ps_feat_db_size(ps_feat* h, int32_t* entries, int64_t* descriptors);
int ps_feat_db_query(ps_feat* h, int32_t first, int32_t last, int32_t ratio_num, int32_t ratio_den, const ps_feat_params* params,
                     int32_t* scores);
/* number of images whose features were computed since create (a recognised frame adds none) */
int ps_feat_feature_passes(ps_feat* h, int64_t* passes);
int ps_feat_device_bytes(ps_feat* h, int64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* PYSLAM_HIP_H */
