// ps_abi_problem.h -- C ABI: error state, ps_problem_create / destroy.  problem_create is the sequence of the create_* stages
// above it; the builders behind them are in ps_host_build.h (device) and ps_host_structure.h (host), the decisions that need
// neither the handle nor HIP in ps_structure.h.
// Part of ps_core.hip (one translation unit; included from there, in this order).


const char* ps_last_error(void) { return g_err.c_str(); }

int ps_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// One-off costs of a process, paid here instead of inside its first solve: the HIP runtime loads this library's code object
// at the FIRST kernel launch (5.8 ms on the MI355X box: it used to sit in the start-cost pass of the first Problem.solve,
// tools/first_call_probe.py) and sets its allocator up at the first hipMalloc (~150 ms, seen as "parameter tables" of the
// first ps_problem_create).  The binding calls this once from require_gpu().
int ps_warm_up(void) {
    static std::once_flag once;
    static int rc = 0;
    std::call_once(once, [] {
        void* p = nullptr;
        if (hipMalloc(&p, 256) != hipSuccess) { rc = fail("hipMalloc failed (no usable HIP device?)"); return; }
        hipLaunchKernelGGL(k_zero4, dim3(1), dim3(256), 0, 0, (size_t)8, (double*)p, (size_t)0, (double*)nullptr, (size_t)0,
                           (double*)nullptr, (size_t)0, (double*)nullptr);
        // (the runtime's own fill and copy kernels are resolved at their first use too: every linearisation starts with a
        //  hipMemsetAsync, the staged calls read their scalars back with hipMemcpyAsync)
        double hostw[4] = {0, 0, 0, 0};
        (void)hipMemsetAsync(p, 0, 256, 0);
        (void)hipMemcpyAsync((char*)p + 128, p, 64, hipMemcpyDeviceToDevice, 0);
        (void)hipMemcpyAsync(hostw, p, sizeof(hostw), hipMemcpyDeviceToHost, 0);
        if (hipDeviceSynchronize() != hipSuccess) rc = fail("the warm-up launch failed");
        hipFree(p);
        // The runtime also builds its object for every KERNEL lazily, at that kernel's first launch (~0.2 ms each: the first
        // whole-iteration call of a process took 6-8 ms for ~35 distinct kernels -- not under rocprofv3, which resolves them all
        // when it loads).  Asking for the attributes of the kernels of the whole-iteration paths resolves them here.
        hipFuncAttributes a;
#define PS_TOUCH(...) (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&__VA_ARGS__))
        PS_TOUCH(k_landmark_pass<false>); PS_TOUCH(k_landmark_pass_packed<false, false, true>); PS_TOUCH(k_landmark_pass_packed<false, true, true>); PS_TOUCH(k_backsub_packed<false, true>); PS_TOUCH(k_pose_pass<false>); PS_TOUCH((k_pose_pass_pf<false, false>)); PS_TOUCH(k_pose_finalize); PS_TOUCH(k_schur_pairs_db<0>);
        PS_TOUCH(k_schur_combine); PS_TOUCH(k_backsub<false>); PS_TOUCH(k_cost_reproj<false>); PS_TOUCH(k_cost_packed<false, true>); PS_TOUCH(k_reduce3); PS_TOUCH(k_reduce_partials);
        PS_TOUCH(k_copy2); PS_TOUCH(k_zero4); PS_TOUCH(k_lag_status_check);
        PS_TOUCH(k_block_jacobi_factor<6>); PS_TOUCH(k_scale_blocks<6>); PS_TOUCH(k_scale_blocks_p<6>); PS_TOUCH(k_rows_setup<6, PS_RS_REGS>); PS_TOUCH(k_rows_setup<6, PS_RS_EXACT>);
        PS_TOUCH(k_coarse_rowsums<6>); PS_TOUCH(k_coarse_matrix<6>); PS_TOUCH(k_coarse_chol<6, true>); PS_TOUCH(k_coarse_chol_band<6>); PS_TOUCH(k_coarse_border<6>);
        PS_TOUCH(k_coarse_mreduce<6>); PS_TOUCH(k_coarse_xbuild<6>); PS_TOUCH(k_coarse_recover<6>); PS_TOUCH(k_cg_fused_lds<6, 8>);
        PS_TOUCH(k_cg_fused<6, 8>); PS_TOUCH(k_cg_unscale<6>); PS_TOUCH(k_update_poses<6>); PS_TOUCH(k_update_points);
        PS_TOUCH(k_xcoarse_rowsums<6>); PS_TOUCH(k_xcoarse_matrix<6>); PS_TOUCH(k_band_chol<6>); PS_TOUCH(k_band_inverse); PS_TOUCH(k_band_inverse_rl<false>);
        PS_TOUCH(k_band_inverse_rl<true>); PS_TOUCH(k_bp_v); PS_TOUCH(k_bp_t); PS_TOUCH(k_bp_w); PS_TOUCH(k_bp_dense_sep); PS_TOUCH(k_bp_dense);
        PS_TOUCH(k_xcg_restrict<6>); PS_TOUCH(k_xcg_f2_coarse<6, 3>); PS_TOUCH(k_xcg_fused1<6, 8, false>); PS_TOUCH(k_xcg_fused1<6, 0, true>);
        PS_TOUCH(k_xcg_fused1<6, 2, false>); PS_TOUCH(k_xcg_fused1<6, 6, false>);
        PS_TOUCH(k_factor_pass<6>); PS_TOUCH(k_factor_assemble<6>); PS_TOUCH(k_cost_factors<6>);
        PS_TOUCH(k_factor_pass<3>); PS_TOUCH(k_factor_assemble<3>); PS_TOUCH(k_cost_factors<3>); PS_TOUCH(k_block_jacobi_factor<3>);
        PS_TOUCH(k_update_poses<3>); PS_TOUCH(k_direct_solve<6>); PS_TOUCH(k_direct_solve<3>);
        PS_TOUCH(k_motion_only_solve<false>); PS_TOUCH(k_motion_only_iteration<false>);
        PS_TOUCH(k_pcg_spmv<6>); PS_TOUCH(k_pcg_spmv<3>); PS_TOUCH(k_ldi_init); PS_TOUCH(k_ldi_update); PS_TOUCH(k_ldi_gemm); PS_TOUCH(k_ldi_mirror);
        PS_TOUCH(k_ldi_ritz); PS_TOUCH(k_ldi_seed_prep); PS_TOUCH(k_ldi_fro_total); PS_TOUCH(k_ldi_pad_identity);
        PS_TOUCH(k_ldi_scaled_dense<6>); PS_TOUCH(k_ldi_sym_unscale<6>); PS_TOUCH(k_ldi_scaled_dense<3>); PS_TOUCH(k_ldi_sym_unscale<3>);
        PS_TOUCH(k_shard_pack<6>); PS_TOUCH(k_shard_unpack<6>); PS_TOUCH(k_publish); PS_TOUCH(k_cov_rhs); PS_TOUCH(k_triangulate<false>);
        PS_TOUCH(k_scale_blocks<3>); PS_TOUCH(k_rows_setup<3, PS_RS_REGS>); PS_TOUCH(k_rows_setup<3, PS_RS_EXACT>); PS_TOUCH(k_coarse_rowsums<3>); PS_TOUCH(k_coarse_matrix<3>);
        PS_TOUCH(k_coarse_chol<3, true>); PS_TOUCH(k_coarse_chol_band<3>); PS_TOUCH(k_coarse_border<3>); PS_TOUCH(k_coarse_mreduce<3>); PS_TOUCH(k_coarse_xbuild<3>);
        PS_TOUCH(k_coarse_recover<3>); PS_TOUCH(k_cg_fused_lds<3, 8>); PS_TOUCH(k_cg_unscale<3>);
#undef PS_TOUCH
    });
    return rc;
}

int ps_problem_destroy(ps_problem* h) {
    if (!h) return 0;
    if (h->cp_dbg) {
        long long c[PS_CP_NCLK]; hipMemcpy(c, h->cp_dbg, sizeof c, hipMemcpyDeviceToHost);
        int khz = 100000; hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0);
        fprintf(stderr, "k_cg_persist, workgroup 0, %ld launches, us per launch: recurrences %.2f | sync %.2f | products + publish %.2f | gather + sums %.2f "
                "(%.1f failed passes) | dots + sync %.2f | exchanges %lld = %.2f per launch | prologue %.2f | recovery %.2f\n", h->cp_launches, c[0] * 1e3 / khz / h->cp_launches,
                c[1] * 1e3 / khz / h->cp_launches, c[2] * 1e3 / khz / h->cp_launches, c[3] * 1e3 / khz / h->cp_launches, (double)c[7] / h->cp_launches,
                c[5] * 1e3 / khz / h->cp_launches, c[6], (double)c[6] / h->cp_launches, c[8] * 1e3 / khz / h->cp_launches, c[4] * 1e3 / khz / h->cp_launches);
        hipFree(h->cp_dbg);
    }
    if (h->xp_dbg) {                                      // (PS_XP_CLOCKS: the LAST launch's time stamps, averaged over its passes)
        std::vector<long long> c(3 * 64 * 8); hipMemcpy(c.data(), h->xp_dbg, c.size() * 8, hipMemcpyDeviceToHost);
        int khz = 100000; hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0);
        for (int w = 0; w < 3; ++w) {
            double ph[6] = {0, 0, 0, 0, 0, 0}; int np = 0;
            for (int p = 1; p < 64; ++p) {                   // (pass 0 = launch -1: no scalars yet; skipped)
                const long long* t = &c[((size_t)w * 64 + p) * 8];
                if (!t[6] || !t[4]) break;
                ph[0] += t[0] - t[6]; ph[1] += t[1] - t[0]; ph[2] += t[2] - t[1]; ph[3] += t[5] - t[2]; ph[4] += t[3] - t[5]; ph[5] += t[4] - t[3]; ++np;
            }
            const double u = 1e3 / khz / std::max(np, 1);
            fprintf(stderr, "k_xcg_persist, workgroup %s, last launch, %d passes, us per pass: t + coarse y %.2f | columns %.2f | products + publish %.2f | "
                    "first gather pass %.2f | rest of the gather %.2f | record sums + dots %.2f | sum %.2f\n", w == 0 ? "0" : (w == 1 ? "nwg/2" : "nwg-1"), np,
                    ph[0] * u, ph[1] * u, ph[2] * u, ph[3] * u, ph[4] * u, ph[5] * u, (ph[0] + ph[1] + ph[2] + ph[3] + ph[4] + ph[5]) * u);
        }
        hipFree(h->xp_dbg);
    }
    if (h->chk_sums) {
        hipDeviceSynchronize();
        fprintf(stderr, "PS_XCG_INV_SUM %p:", (void*)h);
        for (int k = 0; k < std::min(h->chk_nsum, 64); ++k) fprintf(stderr, " [%d use %016llx | side A_c %016llx -> inv %016llx]", k, h->chk_sums[3 * k], h->chk_sums[3 * k + 1], h->chk_sums[3 * k + 2]);
        fprintf(stderr, "\n");
        hipHostFree(h->chk_sums);
    }
    if (h->chk_cnt) {
        int32_t c[4] = {}; hipDeviceSynchronize(); hipMemcpy(c, h->chk_cnt, 16, hipMemcpyDeviceToHost);
        fprintf(stderr, "PS_XCG_AC_CHECK: %d comparisons, entries that differ between the side stream's assembly and the solver stream's: A_c %d, BSZ %d; A_c behind the assembly vs at the end of the side job: %d\n", c[2], c[0], c[1], c[3]);
        hipFree(h->chk_Ac_side); hipFree(h->chk_Ac); hipFree(h->chk_BSZ); hipFree(h->chk_cnt);
    }
    if (ps_env("PS_HOST_TIMING") && h->host_calls)
        fprintf(stderr, "ps_gn_iteration: %ld calls, %.1f us per call on the host, of which %.1f us waiting for the GPU (%ld waits)\n",
                h->host_calls, h->host_call_ns * 1e-3 / h->host_calls, h->host_wait_ns * 1e-3 / h->host_calls, h->host_waits);
    hipStreamSynchronize(h->stream);
    h->persist_release();
    if (h->side) hipStreamSynchronize(h->side);
    if (h->ldi_stream) hipStreamSynchronize(h->ldi_stream);
    cov_release(h);
    if (h->cov_xbuf) hipFree(h->cov_xbuf);
    if (h->tri_buf) hipFree(h->tri_buf);
    for (void* p : h->allocs) hipFree(p);
    h->arena_release();            // arena block, its pinned mirror and the pinned result words go back to the process-wide pool
    for (hipEvent_t e : h->ev_pool) hipEventDestroy(e);
    if (h->ev_ldi) { hipEventDestroy(h->ev_ldi); hipEventDestroy(h->ev_ldi_sread); }
    if (h->ldi_stream && !ps_pool().give(ps_pool().side_streams, h->ldi_stream)) hipStreamDestroy(h->ldi_stream);
    if (h->side) { hipStreamSynchronize(h->side); if (!h->side_poolable || !ps_pool().give(ps_pool().side_streams, h->side)) hipStreamDestroy(h->side); hipEventDestroy(h->ev_ac); hipEventDestroy(h->ev_chol); hipEventDestroy(h->ev_acdone); }
    if (h->own_stream && h->stream && !ps_pool().give(ps_pool().streams, h->stream)) hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

// ps_problem_desc::flags & PS_DESC_DEVICE_TABLES: the small tables (groups, factors, index maps) are walked on the host, so they are
// brought over once (one D2H copy each, no pinned staging on the caller's side); the observation columns stay where they are when
// the structure is built on the device (csrc/ps_host_build.h reads them in place) and come over only for the host builder; the
// parameter tables (PS_DESC_DEVICE_PARAMS) never leave the device.
struct DescStage {
    ps_problem_desc d;
    std::vector<std::vector<char>> bufs;
    int pull_bytes(const void** field, size_t bytes) {
        if (!bytes || !*field) return 0;
        bufs.emplace_back(bytes);
        if (hipMemcpy(bufs.back().data(), *field, bytes, hipMemcpyDeviceToHost) != hipSuccess)
            return fail("ps_problem_create: copy of a device-resident table failed (PS_DESC_DEVICE_TABLES set on a host pointer?)");
        *field = bufs.back().data();
        return 0;
    }
    int pull(const double** f, size_t n) { return pull_bytes((const void**)f, n * sizeof(double)); }
    int pull(const int32_t** f, size_t n) { return pull_bytes((const void**)f, n * sizeof(int32_t)); }
    bool obs_pending = false;
    int pull_obs() {
        if (!obs_pending) return 0;
        obs_pending = false;
        const size_t N = (size_t)std::max<int64_t>(0, d.num_obs);
        return pull(&d.obs_pose, N) || pull(&d.obs_point, N) || pull(&d.obs_uvd, 3 * N) || pull(&d.obs_grp, N);
    }
    int stage(const ps_problem_desc* in) {
        d = *in;
        if (!(d.flags & PS_DESC_DEVICE_TABLES)) return 0;
        const size_t P = std::max(0, d.num_poses), L = std::max(0, d.num_points), N = (size_t)std::max<int64_t>(0, d.num_obs);
        const size_t E = (size_t)std::max<int64_t>(0, d.num_edges), Q = (size_t)std::max<int64_t>(0, d.num_priors);
        const size_t X = (size_t)std::max<int64_t>(0, d.num_extra_pairs), PW = d.dof == 6 ? 12 : 6, DD = (size_t)d.dof * d.dof;
        obs_pending = N > 0;       // the observation columns come over only if the HOST builder is going to walk them (pull_obs)
        return pull(&d.pose_rid, P) || pull(&d.point_vid, L) || pull(&d.cams, 5 * (size_t)std::max(0, d.num_cams)) || pull(&d.stiff3, 9 * (size_t)std::max(0, d.num_stiff3)) ||
               pull(&d.obs_groups, 4 * (size_t)std::max(0, d.num_obs_groups)) || pull(&d.e_i, E) || pull(&d.e_j, E) ||
               pull(&d.e_Tobs_inv, PW * E) || pull(&d.e_grp, E) || pull(&d.u_i, Q) || pull(&d.u_Tobs_inv, PW * Q) || pull(&d.u_grp, Q) ||
               pull(&d.stiffd, DD * (size_t)std::max(0, d.num_stiffd)) || pull(&d.edge_groups, 3 * (size_t)std::max(0, d.num_edge_groups)) ||
               pull(&d.extra_pair_i, X) || pull(&d.extra_pair_j, X);
    }
};

// ---- the stages of ps_problem_create, in the order problem_create runs them.  Each takes the handle, the staged descriptor and
// what earlier stages left for it; each returns 0 or -1 (error set).  The arena requests (upload / alloc / zero) of all stages
// together form ONE fixed sequence: a stage that moves one moves device addresses.
struct CreateIn {
    const ps_problem_desc* d;           // the descriptor with HOST tables (staged if the caller's were resident)
    const ps_problem_desc* src;         // the caller's own (its obs_* are device pointers when PS_DESC_DEVICE_TABLES is set)
    const ps_host_rows_desc* hrows;     // ps_problem_create_hybrid, else null
};

static int create_validate(const ps_problem_desc* d_in, ps_problem** out) {
    if (!d_in || !out) return fail("null argument");
    *out = nullptr;
    if (d_in->flags & ~(uint32_t)(PS_DESC_DEVICE_PARAMS | PS_DESC_DEVICE_TABLES)) return fail("unknown bits in ps_problem_desc.flags");
    if (d_in->dof != 6 && d_in->dof != 3) return fail("dof must be 6 (SE3) or 3 (SE2)");
    if (d_in->num_obs > 0 && d_in->dof != 6) return fail("reprojection blocks need SE(3) poses");
    if (d_in->num_poses >= (1 << 24)) return fail("more than 2^24 poses");
    if (d_in->num_obs >= (1L << 31) / 18) return fail("too many observations for 32-bit indexing");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device visible");
    return 0;
}

// parameter tables, the counts nr / nv, landmark index by vid
static int create_parameter_tables(ps_problem* h, const ps_problem_desc* d, std::vector<int32_t>& point_of_vid) {
    const bool params_resident = (d->flags & PS_DESC_DEVICE_PARAMS) != 0;
    const int D = h->D = d->dof;
    const int PW = h->PW = (D == 6 ? 12 : 6);
    h->P = d->num_poses; h->L = d->num_points; h->N = d->num_obs;
    const int P = h->P, L = h->L;
    if (h->upload(&h->poses, d->poses, (size_t)P * PW, params_resident)) return -1;
    if (h->upload(&h->points, d->points, (size_t)L * 3, params_resident)) return -1;
    if (h->upload(&h->pose_rid, d->pose_rid, (size_t)P)) return -1;
    if (h->alloc(&h->poses_snap, (size_t)P * PW) || h->alloc(&h->points_snap, (size_t)L * 3)) return -1;
    int nr = 0, nv = 0;
    for (int i = 0; i < P; ++i) if (d->pose_rid[i] >= 0) nr = std::max(nr, d->pose_rid[i] + 1);
    for (int i = 0; i < L; ++i) if (d->point_vid[i] >= 0) nv = std::max(nv, d->point_vid[i] + 1);
    h->nr = nr; h->nv = nv;
    point_of_vid.assign(nv, -1);
    for (int i = 0; i < L; ++i) if (d->point_vid[i] >= 0) point_of_vid[d->point_vid[i]] = i;
    for (int v = 0; v < nv; ++v) if (point_of_vid[v] < 0) return fail("point_vid is not a dense 0..nv-1 numbering");
    return 0;
}

// Structure build on the device (csrc/ps_host_build.h): the observation tables and the pair list are produced by kernels
// from the caller's observation columns; the host builder (csrc/ps_host_structure.h) stays as its test oracle and for what the
// device build does not cover.  PS_CREATE_DEVICE: 0 = host builder, 1 = device build from 200 000 observations up (default: below
// that the host builder takes a fraction of a millisecond), 2 = always.
static int create_choose_builder(ps_problem* h, DescStage& staged, const ps_problem_desc* d_in, std::unique_ptr<ObsBuilder>& ob) {
    const ps_problem_desc* d = &staged.d;
    const int create_dev_env = ps_create_env("PS_CREATE_DEVICE") ? atoi(ps_create_env("PS_CREATE_DEVICE")) : 1;
    const bool dev_build = create_dev_env != 0 && h->D == 6 && h->N > 0 && h->nr > 0 && h->nv > 0 && d->num_obs_groups <= 255 &&
                           (create_dev_env == 2 || h->N >= 200000) && !ps_create_env("PS_SCHUR_TILE_KB") && !ps_create_env("PS_PAIRS_BY_LANDMARK");
    if (dev_build) ob.reset(new DevObsBuild(h, d, d_in));
    else {
        if (staged.pull_obs()) return -1;
        ob.reset(new HostObsBuild(h, d));
    }
    return 0;
}

static int create_landmark_slots(ps_problem* h, const ps_problem_desc* d, ObsBuilder& ob, const std::vector<int32_t>& point_of_vid) {
    std::vector<char> seen(h->nr, 0);
    for (int i = 0; i < h->P; ++i) if (d->pose_rid[i] >= 0) {
        if (seen[d->pose_rid[i]]) return fail("pose_rid has duplicates");
        seen[d->pose_rid[i]] = 1;
    }
    for (int i = 0; i < h->nr; ++i) if (!seen[i]) return fail("pose_rid is not a dense 0..nr-1 numbering");
    return ob.slots(point_of_vid);
}

// Observation groups.  Up to 255 rows (camera, stiffness, loss id, loss k): one device group per row.  More --
// typically one stiffness per observation -- : the device groups are the distinct (camera, loss id, loss k) CLASSES
// (at most 255 of those) and the stiffness travels as a per-observation index into the stiffness table ("wide").
static int create_observation_groups(ps_problem* h, const ps_problem_desc* d, std::vector<int32_t>& class_of_row) {
    const bool wide = d->num_obs_groups > 255;
    class_of_row.assign(std::max(1, d->num_obs_groups), 0);
    std::vector<ObsGroup> og;
    auto fill = [&](ObsGroup& o, const double* row, bool with_s) -> int {
        const int cam = (int)row[0], st = (int)row[1];
        if (cam < 0 || cam >= d->num_cams || st < 0 || st >= d->num_stiff3) return fail("obs group index out of range");
        const double* c = d->cams + 5 * cam;
        o.cu = c[0]; o.cv = c[1]; o.fu = c[2]; o.fv = c[3];
        // cams row: baseline b >= 0 = stereo, b = -1 = RGB-D, b = -2 = monocular (u, v); any other negative value is an error
        if (c[4] < 0.0 && c[4] != -1.0 && c[4] != -2.0) return fail("cams row " + std::to_string(cam) + ": b must be >= 0 (stereo), -1 (RGB-D) or -2 (monocular)");
        o.cam_type = c[4] == -2.0 ? 2 : (c[4] < 0.0 ? 1 : 0);
        o.b = o.cam_type ? 0.0 : c[4];
        for (int k = 0; k < 9; ++k) o.S[k] = with_s ? d->stiff3[9 * st + k] : (k % 4 == 0 ? 1.0 : 0.0);
        o.loss_id = (int)row[2]; o.loss_k = row[3];
        return 0;
    };
    if (!wide) {
        og.resize(std::max(1, d->num_obs_groups));
        for (int gi = 0; gi < d->num_obs_groups; ++gi) { if (fill(og[gi], d->obs_groups + 4 * gi, true)) return -1; class_of_row[gi] = gi; }
    } else {
        std::vector<std::array<double, 3>> keys;        // (camera, loss id, loss k) of the classes found so far
        for (int gi = 0; gi < d->num_obs_groups; ++gi) {
            const double* row = d->obs_groups + 4 * gi;
            // every row's stiffness index is read on the device through the per-observation column (round-3 ADVICE: only
            // the first row of a class used to be range-checked)
            if ((int)row[1] < 0 || (int)row[1] >= d->num_stiff3) return fail("obs group index out of range");
            int c = -1;
            for (size_t q = 0; q < keys.size(); ++q)
                if (keys[q][0] == row[0] && keys[q][1] == row[2] && keys[q][2] == row[3]) { c = (int)q; break; }
            if (c < 0) {
                if (keys.size() == 255) return fail("more than 255 distinct (camera, loss) classes among the observation groups");
                keys.push_back({row[0], row[2], row[3]});
                og.emplace_back();
                if (fill(og.back(), row, false)) return -1;
                c = (int)keys.size() - 1;
            }
            class_of_row[gi] = c;
        }
        if (og.empty()) og.emplace_back();
        std::vector<double> st(d->stiff3, d->stiff3 + 9 * (size_t)d->num_stiff3);
        if (h->upload(&h->stiff_tab, st)) return -1;
    }
    h->wide_obs = wide;
    return h->upload(&h->ogroups, og);
}

// observations sorted by landmark: variable points (by slot) first, then constant points; Z and the landmark vectors
static int create_landmark_order(ps_problem* h, ObsBuilder& ob, const std::vector<int32_t>& point_of_vid, const std::vector<int32_t>& class_of_row) {
    const int nv = h->nv;
    if ((long)nv + (long)h->L + 1 >= (1L << 31)) return fail("too many landmarks for 32-bit sort keys");
    if (ob.landmark_order(point_of_vid, class_of_row)) return -1;
    h->Nl = ob.Nl;
    if (h->alloc(&h->Z, (size_t)ob.Nl * PS_ZROW) || h->alloc(&h->Cinv, (size_t)nv * 6) ||
        h->alloc(&h->cvec, (size_t)nv * 3) || h->alloc(&h->dxl, (size_t)nv * 3)) return -1;
    return h->zero(h->dxl, (size_t)nv * 3 * sizeof(double));
}

// pose segments (observations on variable poses), in chunks
static int create_pose_segments(ps_problem* h, const ps_problem_desc* d, ObsBuilder& ob) {
    const int nr = h->nr, P = h->P;
    if (h->nv >= (1 << 24) - 1) return fail("too many variable landmarks for the 24-bit slot field");
    if (ob.pose_order()) return -1;
    const std::vector<int32_t>& pcount = ob.pcount;
    const long Np = h->Np = pcount[nr];
    for (int r = 0; r < nr; ++r) h->max_pose_obs = std::max(h->max_pose_obs, pcount[r + 1] - pcount[r]);
    std::vector<PItem> pitems;
    std::vector<int32_t> pitem_ptr(nr + 1, 0);
    std::vector<int32_t> pose_of_rid(std::max(nr, 1), 0);
    for (int p = 0; p < P; ++p) if (d->pose_rid[p] >= 0) pose_of_rid[d->pose_rid[p]] = p;
    if (h->upload(&h->pose_of_rid, pose_of_rid)) return -1;
    // chunk of observations per workgroup: 512 (two per thread) once that still fills the chip
    // (measured with the LDS-transposed reduction of k_pose_pass: 256 / 512 / 1024 observations per workgroup give
    //  28.3 / 25.9 / 28.6 us at C3 and 0.218 / 0.192 / 0.202 ms at C4)
    int pchunk = Np >= 512L * 256 ? 512 : 256;
    if (const char* e = ps_env("PS_POSE_CHUNK")) pchunk = std::max(256, atoi(e) / 256 * 256);
    h->pose_chunk = pchunk;
    for (int r = 0; r < nr; ++r) {
        for (int s = pcount[r]; s < pcount[r + 1]; s += pchunk)
            pitems.push_back({r, s, std::min(s + pchunk, pcount[r + 1]), pose_of_rid[r]});
        pitem_ptr[r + 1] = (int32_t)pitems.size();
    }
    if (ob.place_sidx_p()) return -1;
    h->npitems = (int)pitems.size();
    if (h->upload(&h->pitems, pitems) || h->upload(&h->pitem_ptr, pitem_ptr) || ob.place_pobs() ||
        h->alloc(&h->ppartial, (size_t)pitems.size() * PS_NPOSE_ACC)) return -1;
    return 0;
}

// pose factors: edges then priors; host rows (ps_problem_create_hybrid) numbered after them
static int create_pose_factors(ps_problem* h, const CreateIn& in, FactorTables& fac) {
    const ps_problem_desc* d = in.d;
    const ps_host_rows_desc* hrows = in.hrows;
    const int D = h->D, DD = D * D, PW = h->PW, P = h->P;
    const long E = fac.E = d->num_edges, Q = d->num_priors, F = fac.F = h->F = E + Q;
    std::vector<FactorGroup> fg(std::max(1, d->num_edge_groups));
    for (int gi = 0; gi < d->num_edge_groups; ++gi) {
        const double* row = d->edge_groups + 3 * gi;
        const int st = (int)row[0];
        if (st < 0 || st >= d->num_stiffd) return fail("edge group stiffness index out of range");
        std::memset(&fg[gi], 0, sizeof(FactorGroup));
        for (int k = 0; k < DD; ++k) fg[gi].S[k] = d->stiffd[(size_t)DD * st + k];
        fg[gi].loss_id = (int)row[1]; fg[gi].loss_k = row[2];
    }
    std::vector<int32_t>&f_i = fac.f_i, &f_j = fac.f_j;
    std::vector<int32_t> f_grp(F);
    f_i.resize(F); f_j.resize(F);
    std::vector<double> f_T((size_t)F * PW);
    for (long f = 0; f < E; ++f) {
        f_i[f] = d->e_i[f]; f_j[f] = d->e_j[f]; f_grp[f] = d->e_grp[f];
        std::memcpy(&f_T[(size_t)f * PW], d->e_Tobs_inv + (size_t)f * PW, PW * sizeof(double));
    }
    for (long u = 0; u < Q; ++u) {
        f_i[E + u] = -1; f_j[E + u] = d->u_i[u]; f_grp[E + u] = d->u_grp[u];
        std::memcpy(&f_T[(size_t)(E + u) * PW], d->u_Tobs_inv + (size_t)u * PW, PW * sizeof(double));
    }
    for (long f = 0; f < F; ++f)
        if (f_j[f] < 0 || f_j[f] >= P || f_i[f] >= P || f_grp[f] < 0 || f_grp[f] >= d->num_edge_groups)
            return fail("pose factor index out of range");
    if (h->upload(&h->fgroups, fg) || h->upload(&h->f_i, f_i) || h->upload(&h->f_j, f_j) ||
        h->upload(&h->f_grp, f_grp) || h->upload(&h->f_Tinv, f_T)) return -1;
    // host rows (ps_problem_create_hybrid): pose pairs of the caller's blocks, numbered F, F + 1, ... after the edges and priors
    const long FH = fac.FH = h->FH = hrows ? std::max<int64_t>(0, hrows->num) : 0;
    fac.hrows = hrows;
    h->hybrid = hrows != nullptr;
    if (FH > 0 && (!hrows->i || !hrows->j)) return fail("null host row table");
    for (long k = 0; k < FH; ++k)
        if (hrows->j[k] < 0 || hrows->j[k] >= P || hrows->i[k] < -1 || hrows->i[k] >= P || hrows->i[k] == hrows->j[k])
            return fail("host row pose index out of range");
    const int FROW = 3 * DD + 2 * D;
    return h->alloc(&h->fscratch, (size_t)(F + FH) * FROW);
}

// Schur pairs per landmark (upper-triangle block keys): the tile count, then ps_pair_list_build (ps_structure.h) over the
// observation builder's pair builder
static int create_pair_list(ps_problem* h, ObsBuilder& ob, std::unique_ptr<PairBuilder>& pb) {
    PairListPolicy pol;
    pol.zbytes = 8.0 * PS_ZROW * (double)ob.Nl;
    pol.tiles_forced = ps_create_env("PS_SCHUR_TILE_KB") != nullptr;
    pol.keep_tiles = ps_env("PS_SCHUR_KEEP_TILES") != nullptr;
    pol.by_landmark = h->nr == 0 || ps_create_env("PS_PAIRS_BY_LANDMARK") != nullptr;
    double tile_kb = 9216.0, min_mb = 16.0;
    if (const char* e = ps_create_env("PS_SCHUR_TILE_KB")) tile_kb = atof(e);
    if (const char* e = ps_create_env("PS_SCHUR_TILE_MIN_MB")) min_mb = atof(e);
    const int ntiles = ps_pair_tiles(pol.zbytes, tile_kb, min_mb);
    pb = ob.pair_builder();
    if (ntiles > pb->max_tiles()) return fail("too many landmark tiles for the device pair build");
    if (pb->prepare()) return -1;
    if (pb->total >= (1L << 31)) return fail("too many Schur pairs for 32-bit indexing");
    if (ps_pair_list_build(*pb, pol, ntiles, &h->schur_tiles)) return -1;
    h->npairs = (long)pb->total;
    return 0;
}

// tasks of the pair list; block pattern of the reduced system; the reduced system itself
static int create_block_pattern(ps_problem* h, const CreateIn& in, const FactorTables& fac, PairBuilder& pb, PairTasks& tk, BlockPattern& pat) {
    const ps_problem_desc* d = in.d;
    const int nr = h->nr, D = h->D, DD = D * D;
    if (pb.tasks(tk)) return -1;
    BlockPatternIn pin;
    pin.nr = nr; pin.dof = D; pin.pose_rid = d->pose_rid;
    pin.task_key = tk.key.data(); pin.ntask = tk.key.size();
    pin.edge_i = fac.f_i.data(); pin.edge_j = fac.f_j.data(); pin.nedge = fac.E;
    if (fac.FH > 0) { pin.hrow_i = in.hrows->i; pin.hrow_j = in.hrows->j; pin.nhrow = fac.FH; }
    pin.extra_i = d->extra_pair_i; pin.extra_j = d->extra_pair_j; pin.nextra = d->num_extra_pairs;
    if (const char* refusal = ps_block_pattern(pin, pat)) return fail(refusal);
    h->h_row_ptr = pat.row_ptr; h->h_col_idx = pat.col_idx;
    const int nnzb = h->nnzb = pat.row_ptr[nr];
    if (h->upload(&h->row_ptr, pat.row_ptr) || h->upload(&h->col_idx, pat.col_idx) || h->upload(&h->diag_slot, pat.diag_slot)) return -1;
    h->red_count = (long)nnzb * DD + (long)nr * D + 2;
    if (h->alloc(&h->red, (size_t)h->red_count + ST_NWORDS / 2)) return -1;       // + the status words: one memset clears both
    h->status = reinterpret_cast<int32_t*>(h->red + h->red_count);
    h->S = h->red; h->g = h->red + (size_t)nnzb * DD;
    return 0;
}

static int create_pair_items(ps_problem* h, PairBuilder& pb, const PairTasks& tk, const BlockPattern& pat, std::vector<PairItem>& pitm) {
    return (build_pair_items(h, tk, pat, pitm) || pb.place_pairs() || build_xcd_lists(h, tk, pitm)) ? -1 : 0;
}

static int create_factor_lists(ps_problem* h, const ps_problem_desc* d, const FactorTables& fac, const BlockPattern& pat, const std::vector<PairItem>& pitm) {
    std::vector<int32_t> eslots;
    if (build_factor_lists(h, d->pose_rid, fac, pat, eslots) || build_zero_slots(h, pat, pitm, eslots)) return -1;
    h->has_extra_pairs = d->num_extra_pairs > 0;
    return 0;
}

static int create_pcg_workspace(ps_problem* h) {
    const int nr = h->nr, D = h->D, DD = D * D, nnzb = h->nnzb;
    const std::vector<int32_t>& row_ptr = h->h_row_ptr;
    const size_t nvec = (size_t)nr * D;
    h->npartA = std::max(1, nr);      // k_pcg_spmv: one workgroup (and one p.q partial) per block row
    h->npartB = std::max(1, cdiv(nr, D == 6 ? PS_PCG_BR(6) : PS_PCG_BR(3)));
    h->hist_cap = 4098;            // classic PCG uses [0,cap); the fused CG needs 2*cap (gamma | alpha)
    if (h->alloc(&h->x, nvec) || h->alloc(&h->r, nvec) || h->alloc(&h->z, nvec) || h->alloc(&h->p0, nvec) ||
        h->alloc(&h->p1, nvec) || h->alloc(&h->q, nvec) || h->alloc(&h->Minv, (size_t)nr * DD) ||
        h->alloc(&h->rz_part, h->npartB) || h->alloc(&h->rr_part, h->npartB) || h->alloc(&h->pq_part, h->npartA) ||
        h->alloc(&h->hist, 2 * (size_t)h->hist_cap)) return -1;
    {
        std::vector<int32_t> brow_of(nnzb), ident(nnzb);
        for (int r = 0; r < nr; ++r) for (int b = row_ptr[r]; b < row_ptr[r + 1]; ++b) brow_of[b] = r;
        for (int b = 0; b < nnzb; ++b) ident[b] = b;
        if (h->upload(&h->brow_of, brow_of) || h->upload(&h->ident_slot, ident)) return -1;
        if (h->alloc(&h->Linv, (size_t)nr * DD)) return -1;
    }
    if (h->zero(h->x, nvec * sizeof(double)) || h->zero(h->p0, nvec * sizeof(double)) || h->zero(h->p1, nvec * sizeof(double))) return -1;
    return 0;
}

// scalars, the runs of landmarks per wave of the packed landmark pass / back-substitution (ps_k_packed.h), result words;
// closes the arena
static int create_scalars(ps_problem* h, ObsBuilder& ob) {
    const int nr = h->nr, nv = h->nv, D = h->D, P = h->P;
    const long N = h->N, F = h->F, Nl = h->Nl;
    h->ncost_obs = N > 0 ? std::min(2048, cdiv(N, 256)) : 0;
    h->ncost_fac = F > 0 ? std::min(1024, cdiv(F, 256)) : 0;
    if (h->alloc(&h->scalars, SC_NWORDS)) return -1;
    if (h->zero(h->scalars, SC_NWORDS * sizeof(double)) || h->zero(h->status, ST_NWORDS * sizeof(int32_t))) return -1;
    h->nsq_l = h->nsq_l16 = nv > 0 ? cdiv(nv, 256 / PS_LM_GROUP) : 0;
    h->lmw_nwaves = 0;
    if (nv > 0 && Nl > 0 && D == 6) {
        int mx = 0, mn = INT_MAX;
        if (ob.landmark_extent(&mx, &mn)) return -1;
        if (mx <= PS_LMW_MAXOBS && mn >= 1) {
            const int W = 64 - (mx - 1), nw = cdiv(Nl, W);
            if (ob.place_run_starts(W, nw)) return -1;
            h->lmw_nwaves = nw;
            h->nsq_l = std::max(h->nsq_l, cdiv(nw, 4));
        }
    }
    h->nsq_p = nr > 0 ? cdiv(P, 256) : 0;
    if (h->alloc(&h->sq_part_l, (size_t)h->nsq_l) || h->alloc(&h->sq_part_p, (size_t)h->nsq_p) ||
        h->alloc(&h->shard_buf, 2)) return -1;
    // (cost partials: one per workgroup of the cost pass, or of the packed landmark pass when that sums the cost; + the factors')
    if (h->alloc(&h->cost_partials, (size_t)std::max({h->ncost_obs + h->ncost_fac, cdiv(h->lmw_nwaves, 4) + h->ncost_fac, 512}) + 8)) return -1;
    if (h->zero(h->shard_buf, 2 * sizeof(double))) return -1;
    // the pinned, host-mapped result words: one block (from the pool), five windows at 256-byte offsets
    if (!ps_pool().take(ps_pool().host_words, &h->words_host))
        HIP_OK(hipHostMalloc(&h->words_host, PS_WORDS_BYTES, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(h->words_host, 0, PS_WORDS_BYTES);
    char* wdev = nullptr;
    HIP_OK(hipHostGetDevicePointer((void**)&wdev, h->words_host, 0));
    static_assert(SC_NWORDS * sizeof(double) <= 256 && ST_NWORDS * sizeof(int32_t) <= 256, "result words outgrew their windows");
    char* whost = (char*)h->words_host;
    h->h_scalars = (double*)(whost + 0);      h->h_scalars_dev = (double*)(wdev + 0);
    h->h_status = (int32_t*)(whost + 256);    h->h_status_dev = (int32_t*)(wdev + 256);
    h->h_seq = (long long*)(whost + 512);     h->h_seq_dev = (long long*)(wdev + 512);
    h->h_shard = (double*)(whost + 768);      h->h_shard_dev = (double*)(wdev + 768);
    h->h_setup = (long long*)(whost + 1024);  h->h_setup_dev = (long long*)(wdev + 1024);
    h->h_ldi_fro = (double*)(whost + 1280);   h->h_ldi_fro_dev = (double*)(wdev + 1280);
    h->h_early = (long long*)(whost + 1536);  h->h_early_dev = (long long*)(wdev + 1536);
    h->h_lmfail = (long long*)(whost + 1792); h->h_lmfail_dev = (long long*)(wdev + 1792);
    h->h_mo_hist = (double*)(whost + 2048);   h->h_mo_hist_dev = (double*)(wdev + 2048);     // PS_MO_HIST_WORDS doubles
    if (h->alloc(&h->arrivals, 2)) return -1;
    if (h->zero(h->arrivals, 2 * sizeof(int32_t))) return -1;
    if (h->arena_close()) return -1;
    HIP_OK(hipStreamSynchronize(h->stream));
    return 0;
}

static int create_two_level(ps_problem* h, StageLap& lap) {
    // The structures of the two-level preconditioner (node lists, augmented pattern, per-workgroup column lists: host work
    // of a few milliseconds at C2 / C4) used to be built by the first solve, i.e. inside the first Gauss-Newton iteration
    // (C2: 9-10 ms against 3 ms for the later ones).  They depend on nothing but the block pattern: built here.  An option
    // that changes them (coarse_groups, cg_explicit, ...) rebuilds them on the next solve as before.
    if (h->nr >= 16 && h->nr * h->D > h->direct_max && h->pcg_variant == 1 && !ps_env("PS_LAZY_COARSE")) {
        if (build_coarse(h)) return -1;
        HIP_OK(hipStreamSynchronize(h->stream));
        lap("two-level structures");
    }
    // a pose graph that will get the direct seed of the lagged inverse (ps_host_ldi.h): its stream is taken here -- the
    // first hipStreamCreate of a process costs ~5 ms, which belongs to set-up, not into the third iteration of a 0.1 ms solve
    if (ldi_eligible(h) && h->ldi_direct_ok && h->N == 0 && h->F > 0 && !h->ldi_stream &&
        !ps_pool().take(ps_pool().side_streams, &h->ldi_stream))
        HIP_OK(hipStreamCreateWithFlags(&h->ldi_stream, hipStreamNonBlocking));
    return 0;
}

static int problem_create(const ps_problem_desc* d_in, const ps_host_rows_desc* hrows, void* stream, ps_problem** out) {
    StageLap lap("ps_problem_create", ps_env("PS_CREATE_TIMING") != nullptr);
    if (create_validate(d_in, out)) return -1;
    DescStage staged;
    if (staged.stage(d_in)) return -1;
    const CreateIn in{&staged.d, d_in, hrows};
    const ps_problem_desc* d = in.d;
    lap("device-resident tables");

    ps_problem* h = new ps_problem();
    if (ps_env("PS_DIRECT_3LAUNCH")) h->direct_fused = 0;   // (measurement build: two option defaults from the environment)
    if (ps_env("PS_LDI_SEED_LAG")) h->ldi_seed_lag = atoi(ps_env("PS_LDI_SEED_LAG"));
    struct Guard { ps_problem* h; bool ok = false; ~Guard() { if (!ok) ps_problem_destroy(h); } } guard{h};
    if (stream) h->stream = (hipStream_t)stream;
    else {
        if (!ps_pool().take(ps_pool().streams, &h->stream)) HIP_OK(hipStreamCreate(&h->stream));
        h->own_stream = true;
    }
    if (h->arena_begin()) return -1;

    // what one stage leaves for the later ones (the builders keep their scratch until the handle is complete)
    std::vector<int32_t> point_of_vid, class_of_row;
    std::unique_ptr<ObsBuilder> ob;
    std::unique_ptr<PairBuilder> pb;
    FactorTables fac;
    PairTasks tasks;
    BlockPattern pat;
    std::vector<PairItem> pitm;

    if (create_parameter_tables(h, d, point_of_vid) || create_choose_builder(h, staged, d_in, ob) ||
        create_landmark_slots(h, d, *ob, point_of_vid)) return -1;
    lap("parameter tables");
    if (create_observation_groups(h, d, class_of_row)) return -1;
    lap("observation groups");
    if (create_landmark_order(h, *ob, point_of_vid, class_of_row)) return -1;
    lap("landmark sort + lobs");
    if (create_pose_segments(h, d, *ob)) return -1;
    lap("pose segments + pobs");
    if (create_pose_factors(h, in, fac)) return -1;
    lap("pose factors");
    if (create_pair_list(h, *ob, pb)) return -1;
    lap("pair generation + sort");
    if (create_block_pattern(h, in, fac, *pb, tasks, pat)) return -1;
    lap("block pattern");
    if (create_pair_items(h, *pb, tasks, pat, pitm)) return -1;
    lap("pair items + XCD lists");
    if (create_factor_lists(h, d, fac, pat, pitm)) return -1;
    lap("factor lists");
    if (create_pcg_workspace(h)) return -1;
    lap("pcg workspace");
    if (create_scalars(h, *ob) || create_two_level(h, lap)) return -1;
    lap("scalars + final sync");
    relook_launch_gates(h);
    guard.ok = true;
    *out = h;
    return 0;
}


int ps_problem_create(const ps_problem_desc* d_in, void* stream, ps_problem** out) {
    return problem_create(d_in, nullptr, stream, out);
}

int ps_problem_create_hybrid(const ps_problem_desc* d_in, const ps_host_rows_desc* rows, void* stream, ps_problem** out) {
    if (!rows) return fail("null argument");
    return problem_create(d_in, rows, stream, out);
}

int ps_set_host_rows(ps_problem* h, const double* rows, int64_t num, double cost) {
    if (!h) return fail("null argument");
    if (!h->hybrid) return fail("ps_set_host_rows: the handle has no host rows (ps_problem_create_hybrid)");
    if (num != h->FH) return fail("ps_set_host_rows: row count differs from the create call's");
    if (num > 0 && !rows) return fail("null argument");
    const size_t FROW = 3 * (size_t)h->D * h->D + 2 * (size_t)h->D;
    if (num > 0) {
        // behind whatever the stream holds (k_factor_pass writes the rows before these, never these)
        HIP_OK(hipMemcpyAsync(h->fscratch + (size_t)h->F * FROW, rows, (size_t)num * FROW * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_OK(hipStreamSynchronize(h->stream));
    }
    h->host_cost = cost;
    h->prelin_valid = h->ride_valid = false;                 // (a linearisation enqueued ahead would lack these rows)
    h->last_cost = h->prev_cost = -1.0;                      // the core's own costs miss the caller's blocks: no cost history
    return 0;
}
