// ps_abi_small.h -- C ABI: frame-to-frame RANSAC and dense photometric alignment.
// Part of ps_core.hip (one translation unit; included from there, in this order, after ps_host_ransac.h: the host side of a
// RANSAC call that the three front ends share).

// ---- frame-to-frame RANSAC (reference pyslam/pipelines/ransac.py) -------------------------------
int ps_ransac_transforms(const double* pts_1, const double* pts_2, int32_t batch, int32_t n, double* T_out) {
    if (!pts_1 || !pts_2 || !T_out || batch < 0 || n <= 0) return fail("bad argument");
    if (batch == 0) return 0;
    if (need_device()) return -1;
    const size_t nb = (size_t)batch * n * 3 * sizeof(double);
    DevBuf a, b, t;
    if (a.get(nb) || b.get(nb) || t.get((size_t)batch * 16 * sizeof(double))) return -1;
    HIP_OK(hipMemcpy(a.p, pts_1, nb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b.p, pts_2, nb, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_ransac_transforms, dim3(cdiv(batch, 64)), dim3(64), 0, 0, batch, n, a.as<double>(), b.as<double>(),
                       t.as<double>());
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(T_out, t.p, (size_t)batch * 16 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

extern "C++" {
namespace {
struct F2fLayout {                   // the parts of a call's device block (RcBlock, ps_host_ransac.h)
    size_t pts1, pts2, obs2, cam, idx;                              // in: pts_1 | pts_2 | obs_2 (3 N each) | cam (8) doubles | samples (int32)
    size_t masks;                                                   // [H][N] bytes, only with own_masks (ps_ransac_cost's are rc_score_call's)
    size_t model, T_best, counts, best, best_mask;                  // out: T_all (16 H) | T_best (16) doubles | counts (H) | best (2) int32 | best_mask (N bytes)
    RcSpan in, out;                                                 // the upload, ps_ransac_frame_to_frame's download
    size_t total;
    F2fLayout(size_t N, size_t H, size_t set_size, bool own_masks) {
        RcBlock B;
        pts1 = B.part(3 * N * F64); pts2 = B.pack(3 * N * F64); obs2 = B.pack(3 * N * F64); cam = B.pack(8 * F64); idx = B.pack(H * set_size * I32);
        in = B.span(pts1);
        masks = B.part(own_masks ? H * N : 0);
        model = B.part(16 * H * F64); T_best = B.pack(16 * F64); counts = B.pack(H * I32); best = B.pack(2 * I32); best_mask = B.pack(N);
        out = B.span(model);
        total = B.part(0);
    }
};

// uploads pts_1 | pts_2 | obs_2 | cam | idx (pts_2 and idx may be NULL: scoring)
int f2f_begin(const F2fLayout& L, char* d, const double* pts_1, const double* pts_2, const double* obs_2, int32_t num_pts,
              const double* cam5, const int32_t* idx, size_t num_idx) {
    const RcCam cam(cam5);
    const size_t pb = 3 * F64 * num_pts;
    return rc_upload(d, L.in, {{L.pts1, pts_1, pb}, {L.pts2, pts_2, pb}, {L.obs2, obs_2, pb}, {L.cam, cam.v, sizeof(cam.v)}, {L.idx, idx, num_idx * I32}});
}

// k_ransac_hypotheses on the uploaded samples (masks == NULL: the block's own) or, scoring, on the transforms at L.model
void f2f_hypotheses(const F2fLayout& L, char* d, int32_t num_pts, int32_t set_size, int32_t num_hyp, double thresh, uint8_t* masks) {
    hipLaunchKernelGGL(k_ransac_hypotheses, dim3(num_hyp), dim3(256), 0, 0, num_pts, set_size,
                       masks ? (const int32_t*)nullptr : (const int32_t*)(d + L.idx), (const double*)(d + L.pts1),
                       masks ? (const double*)nullptr : (const double*)(d + L.pts2), (const double*)(d + L.obs2), (const double*)(d + L.cam),
                       thresh, (double*)(d + L.model), (int32_t*)(d + L.counts), masks ? masks : (uint8_t*)(d + L.masks));
}
}  // namespace
}  // extern "C++"

int ps_ransac_cost(const double* T, int32_t num_hyp, const double* pts_1, const double* obs_2, int32_t num_pts,
                   const double* cam5, double thresh, uint8_t* masks, int32_t* counts) {
    if (!T || !pts_1 || !obs_2 || !cam5 || num_hyp < 0 || num_pts < 0) return fail("bad argument");
    if (num_hyp == 0) return 0;
    const F2fLayout L((size_t)num_pts, (size_t)num_hyp, 0, false);
    return rc_score_call(
        L, T, 16 * F64 * num_hyp, num_hyp, num_pts, masks, counts,
        [&](char* d) { return f2f_begin(L, d, pts_1, nullptr, obs_2, num_pts, cam5, nullptr, 0); },
        [&](char* d, uint8_t* dmasks) { f2f_hypotheses(L, d, num_pts, 0, num_hyp, thresh, dmasks); });
}

int ps_ransac_frame_to_frame(const double* pts_1, const double* pts_2, const double* obs_2, int32_t num_pts,
                             const int32_t* sample_idx, int32_t num_hyp, int32_t set_size, const double* cam5,
                             double thresh, double* T_all, int32_t* counts, int32_t* best_index,
                             int32_t* best_count, double* T_best, uint8_t* best_mask) {
    if (!pts_1 || !pts_2 || !obs_2 || !cam5 || num_pts <= 0) return fail("bad argument");
    if (rc_check_samples(sample_idx, num_hyp, set_size, num_pts, nullptr)) return -1;
    const F2fLayout L((size_t)num_pts, (size_t)num_hyp, (size_t)set_size, true);
    DevBuf buf;
    if (need_device() || buf.get(L.total)) return -1;
    char* d = buf.as<char>();
    if (f2f_begin(L, d, pts_1, pts_2, obs_2, num_pts, cam5, sample_idx, (size_t)num_hyp * set_size)) return -1;
    f2f_hypotheses(L, d, num_pts, set_size, num_hyp, thresh, nullptr);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(k_ransac_best, dim3(1), dim3(256), 0, 0, num_hyp, num_pts, (const int32_t*)(d + L.counts), (const double*)(d + L.model),
                       (const uint8_t*)(d + L.masks), (int32_t*)(d + L.best), (double*)(d + L.T_best), (uint8_t*)(d + L.best_mask));
    HIP_OK(hipGetLastError());
    return rc_download(d, L.out, {{L.model, T_all, 16 * F64 * num_hyp}, {L.T_best, T_best, 16 * F64}, {L.counts, counts, num_hyp * I32},
                                  {L.best, best_index, I32}, {L.best + I32, best_count, I32}, {L.best_mask, best_mask, (size_t)num_pts}});
}

// ---- dense photometric alignment (reference pyslam/residuals/photometric_residual.py) ------------------
struct ps_photo {
    hipStream_t stream = nullptr;
    PhotoArgs args{};
    DevMem mem{0};
    double *pose = nullptr, *partials = nullptr, *out = nullptr;
    int nparts = 0;
    double h_out[PS_PHOTO_NOUT];
};

namespace {
int photo_pass(ps_photo* h, int with_normal, int update) {
    hipLaunchKernelGGL(k_photo_pass, dim3(h->nparts), dim3(256), 0, h->stream, h->args, (const double*)h->pose, with_normal,
                       h->partials);
    hipLaunchKernelGGL(k_photo_finish, dim3(1), dim3(256), 0, h->stream, h->nparts, (const double*)h->partials, with_normal,
                       update, h->pose, h->out);
    return 0;
}
int photo_fetch(ps_photo* h) {
    HIP_OK(hipMemcpyAsync(h->h_out, h->out, sizeof(h->h_out), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    return 0;
}
}  // namespace

int ps_photometric_create(const ps_photo_desc* d, void* stream, ps_photo** out) {
    if (!d || !out) return fail("null argument");
    *out = nullptr;
    if (d->num_pixels < 0 || d->height <= 0 || d->width <= 0) return fail("bad image or pixel count");
    if (d->num_pixels > 0 && (!d->pt_ref || !d->im_ref || !d->im_jac || !d->tri_jac_d)) return fail("null pixel table");
    if (!d->im_track) return fail("null tracking image");
    if (d->cam_type != 0 && d->cam_type != 1) return fail("cam_type must be 0 (stereo) or 1 (RGB-D)");
    if (d->loss_id < 0 || d->loss_id > 5) return fail("unknown loss id");
    if (need_device()) return -1;
    std::unique_ptr<ps_photo> h(new ps_photo);
    h->stream = (hipStream_t)stream;
    PhotoArgs& a = h->args;
    const size_t n = (size_t)d->num_pixels;
    a.n = d->num_pixels; a.h = d->height; a.w = d->width;
    DevMem& M = h->mem;
    if (M.upload(&a.pt_ref, d->pt_ref, 3 * n) || M.upload(&a.im_ref, d->im_ref, n) ||
        M.upload(&a.im_jac, d->im_jac, 2 * n) || M.upload(&a.tri_jac_d, d->tri_jac_d, 3 * n) ||
        M.upload(&a.image, d->im_track, (size_t)d->height * d->width)) return -1;
    a.cu = d->cam[0]; a.cv = d->cam[1]; a.fu = d->cam[2]; a.fv = d->cam[3]; a.b = d->cam[4];
    a.cam_type = d->cam_type; a.cam_w = (double)d->cam_w; a.cam_h = (double)d->cam_h;
    a.var_i = d->intensity_covar; a.var_d = d->depth_covar;
    a.loss_id = d->loss_id; a.loss_k = d->loss_k;
    h->nparts = std::max(1, cdiv(d->num_pixels, 256 * PS_PHOTO_PPT));
    const double ident[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    std::vector<double> zeros((size_t)h->nparts * PS_PHOTO_NACC + PS_PHOTO_NOUT, 0.0);
    if (M.upload(&h->pose, ident, 12) || M.upload(&h->partials, zeros.data(), (size_t)h->nparts * PS_PHOTO_NACC) ||
        M.upload(&h->out, zeros.data(), (size_t)PS_PHOTO_NOUT)) return -1;
    *out = h.release();
    return 0;
}

int ps_photometric_destroy(ps_photo* h) {
    if (!h) return 0;
    if (h->stream) hipStreamSynchronize(h->stream); else hipDeviceSynchronize();
    delete h;
    return 0;
}

int ps_photometric_set_pose(ps_photo* h, const double* pose12) {
    if (!h || !pose12) return fail("null argument");
    HIP_OK(hipMemcpyAsync(h->pose, pose12, 12 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    return 0;
}

int ps_photometric_get_pose(ps_photo* h, double* pose12) {
    if (!h || !pose12) return fail("null argument");
    HIP_OK(hipMemcpyAsync(pose12, h->pose, 12 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    return 0;
}

int ps_photometric_eval_cost(ps_photo* h, double* cost, int64_t* num_valid) {
    if (!h) return fail("null handle");
    if (photo_pass(h, 0, 0) || photo_fetch(h)) return -1;
    if (cost) *cost = h->h_out[42];
    if (num_valid) *num_valid = (int64_t)h->h_out[43];
    return 0;
}

int ps_photometric_normal_equations(ps_photo* h, double* H36, double* b6, double* cost, int64_t* num_valid) {
    if (!h) return fail("null handle");
    if (photo_pass(h, 1, 0) || photo_fetch(h)) return -1;
    if (H36) std::copy(h->h_out, h->h_out + 36, H36);
    if (b6) std::copy(h->h_out + 36, h->h_out + 42, b6);
    if (cost) *cost = h->h_out[42];
    if (num_valid) *num_valid = (int64_t)h->h_out[43];
    return 0;
}

int ps_photometric_iteration(ps_photo* h, int32_t split_params, int32_t linesearch, double* dx6, double* cost) {
    if (!h) return fail("null handle");
    if (photo_pass(h, 1, split_params ? 2 : 1) || photo_fetch(h)) return -1;
    if (h->h_out[43] < 6.0) return fail("photometric alignment: fewer than 6 valid pixels");
    if (h->h_out[50] != 0.0) return fail("photometric alignment: normal equations are not positive definite");
    if (dx6) std::copy(h->h_out + 44, h->h_out + 50, dx6);
    double c = h->h_out[42];
    if (linesearch) {
        if (photo_pass(h, 0, 0) || photo_fetch(h)) return -1;
        c = h->h_out[42];
    }
    if (cost) *cost = c;
    return 0;
}

// ---- the two sparse solves' input: J and J^T in CSR on the device, and the right-hand side b = rhs or -J^T r ---------------
extern "C++" {
namespace {
struct CsrPair {
    DevBuf Jr, Jc, Jv, Tr, Tc, Tv, e, b;
    static int check(int32_t m, int32_t n, const int32_t* j_row_ptr, const int32_t* j_col, const double* j_val, const int32_t* jt_row_ptr,
                     const int32_t* jt_col, const double* jt_val, const double* r, const double* rhs, const double* dx) {
        if (!j_row_ptr || !j_col || !j_val || !jt_row_ptr || !jt_col || !jt_val || !dx || m <= 0 || n <= 0 || (!r && !rhs))
            return fail("bad argument");
        return 0;
    }
    // after check(): the device, the two non-zero counts, the uploads, b (on stream st when it is formed from r)
    int load(hipStream_t st, int32_t m, int32_t n, const int32_t* j_row_ptr, const int32_t* j_col, const double* j_val,
             const int32_t* jt_row_ptr, const int32_t* jt_col, const double* jt_val, const double* r, const double* rhs) {
        if (need_device()) return -1;
        const size_t nnz = (size_t)j_row_ptr[m];
        if ((size_t)jt_row_ptr[n] != nnz) return fail("J and its transpose have different numbers of non-zeros");
        if (Jr.put(j_row_ptr, (size_t)m + 1) || Jc.put(j_col, nnz) || Jv.put(j_val, nnz) || Tr.put(jt_row_ptr, (size_t)n + 1) ||
            Tc.put(jt_col, nnz) || Tv.put(jt_val, nnz)) return -1;
        if (rhs) return b.put(rhs, (size_t)n);
        if (e.put(r, (size_t)m) || b.get((size_t)n * 8)) return -1;
        hipLaunchKernelGGL(k_sp_spmv, dim3(cdiv(n, 256)), dim3(256), 0, st, n, Tr.as<int32_t>(), Tc.as<int32_t>(), Tv.as<double>(),
                           e.as<double>(), b.as<double>(), -1.0);
        return 0;
    }
};
}  // namespace
}  // extern "C++"

// ---- host-evaluated generic path at scale: CG on J^T J dx = rhs, J sparse in HBM (csrc/ps_sparse.h) -----------------
int ps_sparse_normal_solve(int32_t m, int32_t n, const int32_t* j_row_ptr, const int32_t* j_col, const double* j_val,
                           const int32_t* jt_row_ptr, const int32_t* jt_col, const double* jt_val,
                           const double* r, const double* rhs, double tol, int32_t max_iters,
                           double* dx, int32_t* iters_out, double* relres_out) {
    if (CsrPair::check(m, n, j_row_ptr, j_col, j_val, jt_row_ptr, jt_col, jt_val, r, rhs, dx)) return -1;
    hipStream_t st = 0;
    CsrPair J;
    if (J.load(st, m, n, j_row_ptr, j_col, j_val, jt_row_ptr, jt_col, jt_val, r, rhs)) return -1;
    DevBuf bM, bx, br, bz, bp, bq, by, bpart, bsc;
    const int nb = std::max(1, std::min(1024, cdiv(n, 256)));
    if (bM.get((size_t)n * 8) || bx.get((size_t)n * 8) || br.get((size_t)n * 8) || bz.get((size_t)n * 8) || bp.get((size_t)n * 8) ||
        bq.get((size_t)n * 8) || by.get((size_t)m * 8) || bpart.get((size_t)nb * 8) || bsc.get(SPS_N * 8)) return -1;
    HIP_OK(hipMemset(bsc.p, 0, SPS_N * 8));
    const int gm = cdiv(m, 256), gn = cdiv(n, 256);
    hipLaunchKernelGGL(k_sp_diag, dim3(gn), dim3(256), 0, st, n, J.Tr.as<int32_t>(), J.Tv.as<double>(), bM.as<double>());
    hipLaunchKernelGGL(k_sp_init, dim3(nb), dim3(256), 0, st, n, J.b.as<double>(), bM.as<double>(), bx.as<double>(),
                       br.as<double>(), bz.as<double>(), bp.as<double>(), bpart.as<double>());
    hipLaunchKernelGGL(k_sp_scalars, dim3(1), dim3(256), 0, st, nb, bpart.as<double>(), bsc.as<double>(), (int)SPS_RZ, tol * tol, 1);
    double sc[SPS_N] = {};
    int launched = 0;
    while (launched < max_iters) {
        const int chunk = std::min(32, max_iters - launched);
        for (int k = 0; k < chunk; ++k, ++launched) {
            hipLaunchKernelGGL(k_sp_dir, dim3(nb), dim3(256), 0, st, n, bz.as<double>(), bp.as<double>(), bsc.as<double>());
            hipLaunchKernelGGL(k_sp_spmv, dim3(gm), dim3(256), 0, st, m, J.Jr.as<int32_t>(), J.Jc.as<int32_t>(), J.Jv.as<double>(),
                               bp.as<double>(), by.as<double>(), 1.0);
            hipLaunchKernelGGL(k_sp_spmv, dim3(gn), dim3(256), 0, st, n, J.Tr.as<int32_t>(), J.Tc.as<int32_t>(), J.Tv.as<double>(),
                               by.as<double>(), bq.as<double>(), 1.0);
            hipLaunchKernelGGL(k_sp_dot, dim3(nb), dim3(256), 0, st, n, bp.as<double>(), bq.as<double>(), bpart.as<double>());
            hipLaunchKernelGGL(k_sp_scalars, dim3(1), dim3(256), 0, st, nb, bpart.as<double>(), bsc.as<double>(), (int)SPS_PQ, tol * tol, 0);
            hipLaunchKernelGGL(k_sp_update, dim3(nb), dim3(256), 0, st, n, bp.as<double>(), bq.as<double>(), bM.as<double>(),
                               bx.as<double>(), br.as<double>(), bz.as<double>(), bsc.as<double>(), bpart.as<double>());
            hipLaunchKernelGGL(k_sp_scalars, dim3(1), dim3(256), 0, st, nb, bpart.as<double>(), bsc.as<double>(), (int)SPS_RZ, tol * tol, 0);
        }
        if (bsc.fetch(sc, (size_t)SPS_N)) return -1;
        if (sc[SPS_DONE] != 0.0) break;
    }
    if (bx.fetch(dx, (size_t)n)) return -1;
    if (iters_out) *iters_out = (int32_t)sc[SPS_ITERS];
    if (relres_out) *relres_out = sc[SPS_RZ0] > 0.0 ? std::sqrt(sc[SPS_RZ] / sc[SPS_RZ0]) : 0.0;
    if (sc[SPS_DONE] == 2.0) return fail("sparse normal-equation CG broke down (J^T J is not positive semi-definite to rounding, or a NaN in J)");
    return 0;
}

// ---- host-evaluated generic path, DIRECT: (J^T J) dx = -J^T r (or = rhs) by a dense blocked Cholesky on the device, n <= 8 192
// (csrc/ps_sparse.h "Round 5").  relres_out: ||rhs - J^T J dx|| / ||rhs|| of the ORIGINAL system after the refinement steps.
int ps_sparse_normal_direct(int32_t m, int32_t n, const int32_t* j_row_ptr, const int32_t* j_col, const double* j_val,
                            const int32_t* jt_row_ptr, const int32_t* jt_col, const double* jt_val,
                            const double* r, const double* rhs, int32_t refine_steps, double* dx, double* relres_out) {
    if (CsrPair::check(m, n, j_row_ptr, j_col, j_val, jt_row_ptr, jt_col, jt_val, r, rhs, dx)) return -1;
    if (n > PS_SPD_MAXN) return fail("ps_sparse_normal_direct: more unknowns than the dense direct solve takes (8192)");
    hipStream_t st = 0;
    CsrPair J;
    if (J.load(st, m, n, j_row_ptr, j_col, j_val, jt_row_ptr, jt_col, jt_val, r, rhs)) return -1;
    DevBuf bH, bA, bTi, bx, bres, bpart, bst;
    std::vector<double> part(spd_part_count(n));
    if (bH.get((size_t)n * n * 8) || bA.get((size_t)n * n * 8) || bTi.get(bchol_tinv_count(n) * 8) || bx.get((size_t)n * 8) ||
        bres.get((size_t)n * 8) || bpart.get(part.size() * 8) || bst.get(ST_NWORDS * 4)) return -1;
    HIP_OK(hipMemset(bst.p, 0, ST_NWORDS * 4));
    double *H = bH.as<double>(), *b = J.b.as<double>(), *x = bx.as<double>(), *res = bres.as<double>();
    hipLaunchKernelGGL(k_spd_normal, dim3(cdiv((long)n * n, 256)), dim3(256), 0, st, n, J.Jr.as<int32_t>(), J.Jc.as<int32_t>(), J.Jv.as<double>(),
                       J.Tr.as<int32_t>(), J.Tc.as<int32_t>(), J.Tv.as<double>(), H);
    HIP_OK(hipMemcpyAsync(bA.p, H, (size_t)n * n * 8, hipMemcpyDeviceToDevice, st));
    // blocked right-looking Cholesky over the whole chip (ps_host_bchol.h; substitutions through the factor, no inverse)
    const SpdSolve S{n, bA.as<double>(), bTi.as<double>(), bst.as<int32_t>()};
    if (S.factor(st)) return -1;
    HIP_OK(hipMemcpyAsync(x, b, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    S.solve_into(st, x);
    double rel = 0.0;
    for (int it = 0;; ++it) {                                  // residual of the original system; refine through the factor
        S.residual(st, H, b, x, res, bpart.as<double>());
        if (bpart.fetch(part.data(), part.size())) return -1;
        double rr = 0.0, bbn = 0.0;
        for (size_t k = 0; k < part.size(); k += 2) { rr += part[k]; bbn += part[k + 1]; }
        rel = bbn > 0.0 ? std::sqrt(rr / bbn) : 0.0;
        if (it >= refine_steps || !(rel > 1e-15)) break;
        S.solve_into(st, res);
        S.add(st, res, x);
    }
    int32_t stw[ST_NWORDS];
    if (bst.fetch(stw, (size_t)ST_NWORDS)) return -1;
    if (relres_out) *relres_out = rel;
    // (a failed factor leaves NaNs in x: dx stays as the caller gave it)
    if (stw[ST_DIAG_FAIL]) return fail("normal matrix is not positive definite to rounding (dense direct solve)");
    return bx.fetch(dx, (size_t)n);
}

// ---- the band factorisation kernels on their own (csrc/ps_k_band.h, ps_k_bandpart.h): inverse of a symmetric positive definite
// matrix with `bw` block off-diagonals of D x D blocks, A given dense on the host (row-major, nc = ncb D; the lower triangle is
// read).  chunk_nodes < 0: the one-workgroup column walk (k_band_chol + k_band_inverse_rl); 0: the partitioned form with its
// automatic chunk size; > 0: that many interior nodes per chunk.  ainv_out: nc x nc fp32 (what the explicit two-level PCG
// keeps).  elapsed_us (may be NULL): GPU time of the factorisation + inverse launches, measured with events.
int ps_debug_factor_stress(const double* a, int32_t ncb, int32_t dof, int32_t bw, int32_t mode, int32_t launches, int32_t lowprio,
                           int32_t aggressor, int32_t* n_diff, int32_t* n_pivot) {
    // mode bits: 8 = the input is PRODUCED on the victim stream in front of every factorisation (the buffer first holds 2 A, then a
    // many-workgroup copy kernel writes A: a factorisation that starts before its producer has finished reads a mix of both);
    // 16 = an event is recorded between producer and factorisation (as xcg_side_enqueue does with ev_acdone)
    const bool produce = (mode & 8) != 0, with_event = (mode & 16) != 0;
    mode &= 7;
    if (!a || !n_diff || !n_pivot || ncb <= 0 || (dof != 3 && dof != 6) || mode < 0 || mode > 4 || launches < 1) return fail("bad argument");
    if (mode <= 1 && (bw < 1 || bw > PS_BAND_MAXB)) return fail("bad band width");
    if (need_device()) return -1;
    const int nc = ncb * dof;
    if (mode == 2 && nc > 90) return fail("mode 2 (LDS-resident k_coarse_chol) needs ncb dof <= 90");
    DevBuf bA, bInv, bLr, bLc, brd, bXs, bst, bLi, bLiT, bsc, bTi, ga, gb;
    const size_t gn = (size_t)16 << 20;
    if (bA.put(a, (size_t)nc * nc) || bInv.get((size_t)nc * nc * 4) || bst.get(ST_NWORDS * 4) || bLr.get((size_t)nc * PS_BAND_W * 8) ||
        bLc.get((size_t)nc * PS_BAND_W * 8) || brd.get((size_t)nc * 8) || bXs.get((size_t)nc * nc * 8) || bLi.get((size_t)nc * nc * 8) ||
        bLiT.get((size_t)nc * nc * 8) || bsc.get((size_t)2 * nc * nc * 8) || bTi.get(bchol_tinv_count(nc) * 8) ||
        ga.get(gn * 8) || gb.get(gn * 8)) return -1;
    HIP_OK(hipMemset(ga.p, 0, gn * 8));
    DevBuf bA1, bA2;
    hipEvent_t evp = nullptr;
    if (produce) {
        std::vector<double> a2((size_t)nc * nc);
        for (size_t k = 0; k < a2.size(); ++k) a2[k] = 2.0 * a[k];
        if (bA1.put(a, a2.size()) || bA2.put(a2.data(), a2.size())) return -1;
        HIP_OK(hipEventCreateWithFlags(&evp, hipEventDisableTiming));
    }
    struct EvGuard { hipEvent_t e; ~EvGuard() { if (e) hipEventDestroy(e); } } evg{evp};
    hipStream_t vs = nullptr, as = nullptr;
    int lo = 0, hi = 0;
    HIP_OK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    if (lowprio) HIP_OK(hipStreamCreateWithPriority(&vs, hipStreamNonBlocking, lo)); else HIP_OK(hipStreamCreateWithFlags(&vs, hipStreamNonBlocking));
    HIP_OK(hipStreamCreateWithFlags(&as, hipStreamNonBlocking));
    struct Streams { hipStream_t a, b; ~Streams() { hipStreamDestroy(a); hipStreamDestroy(b); } } streams{vs, as};
    std::unique_ptr<BandPart> bp;
    if (mode == 1) {
        const int m = BandPart::auto_m(ncb, bw);
        if (!BandPart::eligible(ncb, bw, m)) return fail("mode 1: the partitioned factorisation does not apply to this shape");
        bp.reset(new BandPart());
        if (bp->build(ncb, dof, bw, m, vs)) return -1;
    }
    const size_t chol_lds = 2 * (size_t)nc * nc * sizeof(double);
    if (mode == 2 && (dof == 6 ? ensure_dynamic_lds((const void*)k_coarse_chol<6, true>, chol_lds) : ensure_dynamic_lds((const void*)k_coarse_chol<3, true>, chol_lds))) return -1;
    auto run = [&](hipStream_t st) -> int {
        if (produce) {
            copy_doubles(st, bA.as<double>(), bA2.as<double>(), (size_t)nc * nc);       // 2 A ...
            copy_doubles(st, bA.as<double>(), bA1.as<double>(), (size_t)nc * nc);       // ... then A, by a kernel of many workgroups
            if (with_event) HIP_OK(hipEventRecord(evp, st));
        }
        HIP_OK(hipMemsetAsync(bst.p, 0, ST_NWORDS * 4, st));
        HIP_OK(hipMemsetAsync(bInv.p, 0, (size_t)nc * nc * 4, st));
        if (mode == 0) {
            HIP_OK(hipMemsetAsync(bLr.p, 0, (size_t)nc * PS_BAND_W * 8, st));
            HIP_OK(hipMemsetAsync(bLc.p, 0, (size_t)nc * PS_BAND_W * 8, st));
            if (dof == 6) hipLaunchKernelGGL(k_band_chol<6>, dim3(1), dim3(256), 0, st, ncb, bw, bA.as<double>(), bLr.as<double>(), bLc.as<double>(), brd.as<double>(), bst.as<int32_t>(), nc, (const int2*)nullptr);
            else hipLaunchKernelGGL(k_band_chol<3>, dim3(1), dim3(256), 0, st, ncb, bw, bA.as<double>(), bLr.as<double>(), bLc.as<double>(), brd.as<double>(), bst.as<int32_t>(), nc, (const int2*)nullptr);
            hipLaunchKernelGGL(k_band_inverse_rl<false>, dim3(cdiv(nc, 4)), dim3(256), 0, st, nc, (const double*)bLr.as<double>(), (const double*)bLc.as<double>(),
                               (const double*)brd.as<double>(), bXs.as<double>(), bInv.as<float>(), (const BandInvItem*)nullptr, (double*)nullptr, nc);
        } else if (mode == 1) {
            if (dof == 6 ? bp->run<6>(st, bA.as<double>(), nc, bInv.as<float>(), nc, bst.as<int32_t>()) : bp->run<3>(st, bA.as<double>(), nc, bInv.as<float>(), nc, bst.as<int32_t>())) return -1;
        } else if (mode == 4) {
            // the blocked chain as xcg_coarse_inverse runs it: working copy of A by a kernel, factor, L^-1 without zero fill, A^-1
            copy_doubles(st, bsc.as<double>(), bA.as<double>(), (size_t)nc * nc);
            if (bchol_chain(st, nc, BCHOL_FACTOR | BCHOL_INVERSE | BCHOL_AINV, bsc.as<double>(), bTi.as<double>(), bst.as<int32_t>(),
                            bLi.as<double>(), bLiT.as<double>(), bInv.as<float>(), nc)) return -1;
        } else {
            if (mode == 2) {
                if (dof == 6) hipLaunchKernelGGL((k_coarse_chol<6, true>), dim3(1), dim3(1024), chol_lds, st, ncb, bA.as<double>(), bLi.as<double>(), bLiT.as<double>(), bst.as<int32_t>(), nullptr);
                else hipLaunchKernelGGL((k_coarse_chol<3, true>), dim3(1), dim3(1024), chol_lds, st, ncb, bA.as<double>(), bLi.as<double>(), bLiT.as<double>(), bst.as<int32_t>(), nullptr);
            } else {
                if (dof == 6) hipLaunchKernelGGL((k_coarse_chol<6, false>), dim3(1), dim3(1024), 0, st, ncb, bA.as<double>(), bLi.as<double>(), bLiT.as<double>(), bst.as<int32_t>(), bsc.as<double>());
                else hipLaunchKernelGGL((k_coarse_chol<3, false>), dim3(1), dim3(1024), 0, st, ncb, bA.as<double>(), bLi.as<double>(), bLiT.as<double>(), bst.as<int32_t>(), bsc.as<double>());
            }
            bchol_ainv(st, nc, bLi.as<double>(), bInv.as<float>(), nc);
        }
        return 0;
    };
    std::vector<float> ref((size_t)nc * nc), out((size_t)nc * nc);
    int32_t stw[ST_NWORDS];
    if (run(vs)) return -1;
    HIP_OK(hipStreamSynchronize(vs));
    if (bInv.fetch(ref.data(), ref.size()) || bst.fetch(stw, (size_t)ST_NWORDS)) return -1;
    if (stw[ST_DIAG_FAIL]) return fail("ps_debug_factor_stress: the input is not positive definite (idle reference run)");
    *n_diff = *n_pivot = 0;
    for (int k = 0; k < launches; ++k) {
        if (aggressor == 1) for (int q = 0; q < 3; ++q) copy_doubles(as, gb.as<double>(), ga.as<double>(), gn);
        if (aggressor == 2) {                                 // workgroups with 96 KB of LDS each, scribbling over all of it
            const size_t lds = 96 * 1024;
            if (ensure_dynamic_lds((const void*)k_lds_scribble, lds)) return -1;
            for (int q = 0; q < 2; ++q) hipLaunchKernelGGL(k_lds_scribble, dim3(1024), dim3(512), lds, as, (int)(lds / 8), 6, gb.as<double>());
        }
        if (run(vs)) return -1;
        HIP_OK(hipStreamSynchronize(vs));
        if (bInv.fetch(out.data(), out.size()) || bst.fetch(stw, (size_t)ST_NWORDS)) return -1;
        if (std::memcmp(out.data(), ref.data(), out.size() * 4)) ++*n_diff;
        if (stw[ST_DIAG_FAIL]) ++*n_pivot;
    }
    HIP_OK(hipDeviceSynchronize());
    if (bp) bp.reset();
    return 0;
}

int ps_debug_band_inverse(const double* a, int32_t ncb, int32_t dof, int32_t bw, int32_t chunk_nodes, float* ainv_out, double* elapsed_us) {
    if (!a || !ainv_out || ncb <= 0 || (dof != 3 && dof != 6) || bw < 1 || bw > PS_BAND_MAXB) return fail("bad argument");
    if (need_device()) return -1;
    const int nc = ncb * dof;
    DevBuf bA, bInv, bLr, bLc, brd, bXs, bst;
    if (bA.put(a, (size_t)nc * nc) || bInv.get((size_t)nc * nc * 4) || bst.get(ST_NWORDS * 4)) return -1;
    HIP_OK(hipMemset(bst.p, 0, ST_NWORDS * 4));
    HIP_OK(hipMemset(bInv.p, 0, (size_t)nc * nc * 4));
    hipStream_t st = 0;
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
    struct Ev { hipEvent_t a, b; ~Ev() { hipEventDestroy(a); hipEventDestroy(b); } } evs{e0, e1};
    float ms = 0.f;
    for (int rep = 0; rep < 2; ++rep) {                       // (the second run is the one timed: the first loads the kernels)
        if (chunk_nodes < 0) {
            if (rep == 0 && (bLr.get((size_t)nc * PS_BAND_W * 8) || bLc.get((size_t)nc * PS_BAND_W * 8) || brd.get((size_t)nc * 8) ||
                             bXs.get((size_t)nc * nc * 8))) return -1;
            HIP_OK(hipMemsetAsync(bLr.p, 0, (size_t)nc * PS_BAND_W * 8, st));
            HIP_OK(hipMemsetAsync(bLc.p, 0, (size_t)nc * PS_BAND_W * 8, st));
            HIP_OK(hipEventRecord(e0, st));
            if (dof == 6) hipLaunchKernelGGL(k_band_chol<6>, dim3(1), dim3(256), 0, st, ncb, bw, bA.as<double>(), bLr.as<double>(), bLc.as<double>(),
                                             brd.as<double>(), bst.as<int32_t>(), nc, (const int2*)nullptr);
            else hipLaunchKernelGGL(k_band_chol<3>, dim3(1), dim3(256), 0, st, ncb, bw, bA.as<double>(), bLr.as<double>(), bLc.as<double>(),
                                    brd.as<double>(), bst.as<int32_t>(), nc, (const int2*)nullptr);
            hipLaunchKernelGGL(k_band_inverse_rl<false>, dim3(cdiv(nc, 4)), dim3(256), 0, st, nc, (const double*)bLr.as<double>(),
                               (const double*)bLc.as<double>(), (const double*)brd.as<double>(), bXs.as<double>(), bInv.as<float>(),
                               (const BandInvItem*)nullptr, (double*)nullptr, nc);
            HIP_OK(hipEventRecord(e1, st));
        } else {
            static thread_local std::unique_ptr<BandPart> bp;
            const int m = chunk_nodes > 0 ? chunk_nodes : BandPart::auto_m(ncb, bw);
            if (rep == 0) {
                if (2 * bw - 1 > PS_BAND_MAXB || m < bw) return fail("partitioned band factorisation: needs 2 bw - 1 <= 7 and chunks of at least bw nodes");
                bp.reset(new BandPart());
                if (bp->build(ncb, dof, bw, m, st)) { bp.reset(); return -1; }
            }
            HIP_OK(hipEventRecord(e0, st));
            const int rc = dof == 6 ? bp->run<6>(st, bA.as<double>(), nc, bInv.as<float>(), nc, bst.as<int32_t>())
                                    : bp->run<3>(st, bA.as<double>(), nc, bInv.as<float>(), nc, bst.as<int32_t>());
            HIP_OK(hipEventRecord(e1, st));
            if (rc) { bp.reset(); return -1; }
            if (rep == 1) { HIP_OK(hipStreamSynchronize(st)); bp.reset(); }
        }
        HIP_OK(hipStreamSynchronize(st));
    }
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    if (elapsed_us) *elapsed_us = 1e3 * ms;
    int32_t stw[ST_NWORDS];
    if (bst.fetch(stw, (size_t)ST_NWORDS) || bInv.fetch(ainv_out, (size_t)nc * nc)) return -1;
    if (stw[ST_DIAG_FAIL]) return fail("band factorisation: the matrix is not positive definite");
    return 0;
}

// ---- the LDS-resident coarse factorisation kernels on their own (csrc/ps_k_coarse.h; tests/test_gpu_coarse_chol_band.py) ------
// One launch of k_coarse_chol<dof, true> (variant 0) or k_coarse_chol_band<dof> (variant 1: the production launch; 64 .. 1024, a
// multiple of 64: that many threads) on a host matrix (nc x nc row-major, nc = ncb dof <= 90), on a stream of its own.  Li and LiT
// are pre-filled with NaN bit patterns, so an entry a kernel failed to write would show.  status: the ST_NWORDS status words.
// clocks (may be NULL; measurement build only): six wall-clock stamps of thread 0 -- entry | loaded | factor loop done |
// diagonal inverses done | doubling done | stored -- in microseconds from the first.
static int debug_coarse_chol(const double* a, int32_t ncb, int32_t dof, int32_t bw, int32_t variant, double* Li, double* LiT,
                             int32_t* status, double* elapsed_us, double* clocks) {
    if (!a || !Li || !LiT || !status || ncb <= 0 || (dof != 3 && dof != 6)) return fail("ps_debug_coarse_chol: bad argument");
    const int nc = ncb * dof;
    if (nc > 90) return fail("ps_debug_coarse_chol: the LDS-resident kernels take ncb dof <= 90");
    if (variant != 0 && variant != 1 && (variant < 64 || variant > 1024 || variant % 64)) return fail("ps_debug_coarse_chol: bad variant");
    if (variant != 0 && (bw < 0 || bw > ncb - 1)) return fail("ps_debug_coarse_chol: bw must be 0 .. ncb - 1");
    if (clocks && !PS_MEASURE_BUILD) return fail("ps_debug_coarse_chol_clocks: phase clocks exist in the measurement build only");
    if (need_device()) return -1;
    const size_t nn = (size_t)nc * nc;
    DevBuf bA, bLi, bLiT, bst, bck;
    if (bA.put(a, nn) || bLi.get(nn * 8) || bLiT.get(nn * 8) || bst.get(ST_NWORDS * 4) || bck.get(8 * 8)) return -1;
    hipStream_t st = nullptr;
    HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct St { hipStream_t s; ~St() { hipStreamDestroy(s); } } stg{st};
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
    struct Ev { hipEvent_t a, b; ~Ev() { hipEventDestroy(a); hipEventDestroy(b); } } evs{e0, e1};
    const size_t chol_lds = 2 * nn * sizeof(double);
    const int threads = variant == 1 ? PS_CCB_THREADS : variant;
    if (variant == 0 ? (dof == 6 ? ensure_dynamic_lds((const void*)k_coarse_chol<6, true>, chol_lds) : ensure_dynamic_lds((const void*)k_coarse_chol<3, true>, chol_lds))
                     : (dof == 6 ? ensure_dynamic_lds((const void*)k_coarse_chol_band<6>, chol_lds) : ensure_dynamic_lds((const void*)k_coarse_chol_band<3>, chol_lds))) return -1;
    for (int rep = 0; rep < (elapsed_us ? 2 : 1); ++rep) {    // (a timed call: the second run is the one timed, the first loads the kernel)
        HIP_OK(hipMemsetAsync(bst.p, 0, ST_NWORDS * 4, st));
        HIP_OK(hipMemsetAsync(bck.p, 0, 8 * 8, st));
        HIP_OK(hipMemsetAsync(bLi.p, 0xff, nn * 8, st));
        HIP_OK(hipMemsetAsync(bLiT.p, 0xff, nn * 8, st));
        HIP_OK(hipEventRecord(e0, st));
        if (variant == 0) {
            double* ck = clocks ? bck.as<double>() : nullptr;       // (k_coarse_chol's measurement build stamps its scratch argument)
            if (dof == 6) hipLaunchKernelGGL((k_coarse_chol<6, true>), dim3(1), dim3(1024), chol_lds, st, ncb, bA.as<double>(), bLi.as<double>(), bLiT.as<double>(), bst.as<int32_t>(), ck);
            else hipLaunchKernelGGL((k_coarse_chol<3, true>), dim3(1), dim3(1024), chol_lds, st, ncb, bA.as<double>(), bLi.as<double>(), bLiT.as<double>(), bst.as<int32_t>(), ck);
        } else {
            long long* ck = clocks ? bck.as<long long>() : nullptr;
            if (dof == 6) hipLaunchKernelGGL(k_coarse_chol_band<6>, dim3(1), dim3(threads), chol_lds, st, ncb, bw, (const double*)bA.as<double>(), bLi.as<double>(), bLiT.as<double>(), bst.as<int32_t>(), ck);
            else hipLaunchKernelGGL(k_coarse_chol_band<3>, dim3(1), dim3(threads), chol_lds, st, ncb, bw, (const double*)bA.as<double>(), bLi.as<double>(), bLiT.as<double>(), bst.as<int32_t>(), ck);
        }
        HIP_OK(hipEventRecord(e1, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    if (elapsed_us) { float ms = 0.f; HIP_OK(hipEventElapsedTime(&ms, e0, e1)); *elapsed_us = 1e3 * ms; }
    if (bst.fetch(status, (size_t)ST_NWORDS) || bLi.fetch(Li, nn) || bLiT.fetch(LiT, nn)) return -1;
    if (clocks) {
        long long c[6];
        int khz = 100000;
        if (bck.fetch(c, (size_t)6)) return -1;
        HIP_OK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0));
        if (!c[3]) c[3] = c[2];                               // (a single block row: no doubling level stamps it)
        for (int k = 0; k < 6; ++k) clocks[k] = (double)(c[k] - c[0]) * 1e3 / khz;
    }
    return 0;
}

int ps_debug_coarse_chol(const double* a, int32_t ncb, int32_t dof, int32_t bw, int32_t variant, double* Li, double* LiT,
                         int32_t* status, double* elapsed_us) {
    return debug_coarse_chol(a, ncb, dof, bw, variant, Li, LiT, status, elapsed_us, nullptr);
}

int ps_debug_coarse_chol_clocks(const double* a, int32_t ncb, int32_t dof, int32_t bw, int32_t variant, double* clocks /* 6 */) {
    if (!clocks || !a || ncb <= 0 || (dof != 3 && dof != 6) || ncb * dof > 90) return fail("ps_debug_coarse_chol_clocks: bad argument");
    std::vector<double> li((size_t)ncb * dof * ncb * dof), lit(li.size());
    int32_t stw[ST_NWORDS];
    double us = 0.0;
    return debug_coarse_chol(a, ncb, dof, bw, variant, li.data(), lit.data(), stw, &us, clocks);
}

// ---- the blocked dense factorisation chain on its own (csrc/ps_host_bchol.h; tests/test_gpu_bchol_kernels.py) ----------------
// Every stage's output of bchol_chain on a host matrix, on a stream of its own.  flags bit 0: the folded CG's dense-output form
// (zero fill + k_btri_clear), else the explicit PCG's; bits 8..15: extra columns of ainv_out's leading dimension (ld = n + that;
// ainv_out's contents go in, what k_xcg_ainv leaves alone comes back unchanged).  Li and LiT are pre-filled with NaN bit patterns:
// what a form leaves unspecified comes back as NaN, and a kernel that read it would show.
int ps_debug_dense_factor(const double* a, int32_t n, int32_t flags, double* l_out, double* tinv_out, double* li_out, double* lit_out,
                          float* ainv_out, int32_t* diag_fail, double* elapsed_us) {
    if (!a || n <= 0 || (flags & ~0xff01)) return fail("ps_debug_dense_factor: bad argument");
    if (n > PS_SPD_MAXN) return fail("ps_debug_dense_factor: more than 8192 unknowns");
    if (need_device()) return -1;
    const int ld = n + ((flags >> 8) & 0xff);
    const size_t nn = (size_t)n * n, nti = bchol_tinv_count(n), ninv = (size_t)n * ld;
    DevBuf bA0, bA, bTi, bLi, bLiT, bInv, bInv0, bst;
    if (bA0.put(a, nn) || bA.get(nn * 8) || bTi.get(nti * 8) || bLi.get(nn * 8) || bLiT.get(nn * 8) || bInv.get(ninv * 4) ||
        (ainv_out ? bInv0.put(ainv_out, ninv) : bInv0.get(ninv * 4)) || bst.get(ST_NWORDS * 4)) return -1;
    if (!ainv_out) HIP_OK(hipMemset(bInv0.p, 0, ninv * 4));
    hipStream_t st = nullptr;
    HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct St { hipStream_t s; ~St() { hipStreamDestroy(s); } } stg{st};
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
    struct Ev { hipEvent_t a, b; ~Ev() { hipEventDestroy(a); hipEventDestroy(b); } } evs{e0, e1};
    const int stages = BCHOL_FACTOR | BCHOL_INVERSE | BCHOL_AINV | ((flags & 1) ? BCHOL_DENSE_OUT : 0);
    for (int rep = 0; rep < 2; ++rep) {                       // (the second run is the one timed: the first loads the kernels)
        HIP_OK(hipMemcpyAsync(bA.p, bA0.p, nn * 8, hipMemcpyDeviceToDevice, st));
        HIP_OK(hipMemcpyAsync(bInv.p, bInv0.p, ninv * 4, hipMemcpyDeviceToDevice, st));
        HIP_OK(hipMemsetAsync(bst.p, 0, ST_NWORDS * 4, st));
        HIP_OK(hipMemsetAsync(bTi.p, 0, nti * 8, st));
        HIP_OK(hipMemsetAsync(bLi.p, 0xff, nn * 8, st));
        HIP_OK(hipMemsetAsync(bLiT.p, 0xff, nn * 8, st));
        HIP_OK(hipEventRecord(e0, st));
        if (bchol_chain(st, n, stages, bA.as<double>(), bTi.as<double>(), bst.as<int32_t>(), bLi.as<double>(), bLiT.as<double>(),
                        bInv.as<float>(), ld)) return -1;
        HIP_OK(hipEventRecord(e1, st));
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(st));
    }
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    if (elapsed_us) *elapsed_us = 1e3 * ms;
    int32_t stw[ST_NWORDS];
    if (bst.fetch(stw, (size_t)ST_NWORDS) || (l_out && bA.fetch(l_out, nn)) || (tinv_out && bTi.fetch(tinv_out, nti)) ||
        (li_out && bLi.fetch(li_out, nn)) || (lit_out && bLiT.fetch(lit_out, nn)) || (ainv_out && bInv.fetch(ainv_out, ninv))) return -1;
    if (diag_fail) *diag_fail = stw[ST_DIAG_FAIL];
    else if (stw[ST_DIAG_FAIL]) return fail("ps_debug_dense_factor: the matrix is not positive definite");
    return 0;
}

// Host only: which rows of a panel of m rows x w columns workgroup `block` of k_bchol_panel owns -- found by walking every
// (thread, entry) of that workgroup through ps_bchol_slab, the function the kernel itself uses.  [row_lo, row_hi): the rows it
// touches; entries: the distinct (row, column) cells it owns; grid: workgroups of the launch.  Needs no device.
int ps_debug_bchol_slab(int32_t m, int32_t w, int32_t block, int32_t* row_lo, int32_t* row_hi, int32_t* entries, int32_t* grid) {
    if (m < 0 || m > (1 << 24) || w < 1 || w > PS_BC_W || block < 0 || block > (1 << 20) || !row_lo || !row_hi || !entries || !grid) return fail("ps_debug_bchol_slab: bad argument");
    int lo = INT_MAX, hi = -1, g = 0;
    std::vector<std::pair<int, int>> cells;
    for (int t = 0; t < 256; ++t)
        for (int k = 0; k < PS_BC_SLAB / 256; ++k) {
            int r, c;
            g = ps_bchol_slab(m, w, block, t, k, &r, &c);
            if (r < 0) continue;
            if (r >= m || c < 0 || c >= w) return fail("ps_debug_bchol_slab: the mapping leaves the panel");
            lo = std::min(lo, r); hi = std::max(hi, r);
            cells.emplace_back(r, c);
        }
    std::sort(cells.begin(), cells.end());
    if (std::adjacent_find(cells.begin(), cells.end()) != cells.end()) return fail("ps_debug_bchol_slab: a cell is owned twice");
    *entries = (int32_t)cells.size();
    *row_lo = hi < 0 ? 0 : lo;
    *row_hi = hi < 0 ? 0 : hi + 1;
    *grid = g;
    return 0;
}

// ---- the lagged dense inverse's kernels on their own (csrc/ps_k_ldi.h; tests/test_gpu_ldi_kernels.py) -----------------------------
// C = alpha A B + beta Dm + gamma I by k_ldi_gemm, launched through ldi_gemm() like every production product.  Host arrays in
// (A: M x lda, B: K x ldb, Dm: M x ldd or NULL, C: M x ldc with the caller's initial contents), C and the per-tile Frobenius
// parts out (fro_part: (M / 32) (N / 32) doubles pre-filled with fro_sentinel, or NULL).  Dm may be the very pointer A (or B):
// the device copies alias then too, as in ldi_ns_step.  krange: 2 (M / 32) ints or NULL; dev_scale: one float or NULL.
int ps_debug_ldi_gemm(int32_t M, int32_t N, int32_t K, float alpha, const float* A, int32_t lda, const float* B, int32_t ldb, float beta,
                      const float* Dm, int32_t ldd, float gamma, float* C, int32_t ldc, const int32_t* krange, int32_t upper_only,
                      const float* dev_scale, double fro_sentinel, double* fro_part) {
    if (!A || !B || !C) return fail("ps_debug_ldi_gemm: null argument");
    if (M <= 0 || N <= 0 || K <= 0 || M % PS_GM_BM || N % PS_GM_BN) return fail("ps_debug_ldi_gemm: M and N must be positive multiples of 32");
    if (K % PS_GM_BK) return fail("ps_debug_ldi_gemm: K must be a multiple of 16");
    if (lda < K || ldb < N || ldc < N || (Dm && ldd < N)) return fail("ps_debug_ldi_gemm: a leading dimension is smaller than its extent");
    if (lda % 4 || ldb % 4) return fail("ps_debug_ldi_gemm: lda and ldb must be multiples of 4 (16-byte loads)");
    if (beta != 0.f && !Dm) return fail("ps_debug_ldi_gemm: beta != 0 needs Dm");
    if (upper_only && M != N) return fail("ps_debug_ldi_gemm: upper_only needs a square C");
    const int mt = M / PS_GM_BM, nt = N / PS_GM_BN;
    if (krange)
        for (int t = 0; t < mt; ++t) {
            const int lo = krange[2 * t], hi = krange[2 * t + 1];
            if (lo < 0 || hi > K || lo > hi || lo % PS_GM_BK || hi % PS_GM_BK) return fail("ps_debug_ldi_gemm: krange bounds must be multiples of 16 with 0 <= lo <= hi <= K");
        }
    if (need_device()) return -1;
    DevBuf bA, bB, bD, bC, bF, bK, bS;
    const size_t na = (size_t)M * lda, nb = (size_t)K * ldb, nd = (size_t)M * ldd, nc = (size_t)M * ldc;
    if (bA.put(A, na) || bB.put(B, nb) || bC.put(C, nc)) return -1;
    const float* dD = nullptr;
    if (Dm == A && ldd == lda) dD = bA.as<float>();
    else if (Dm == B && ldd == ldb && M == K) dD = bB.as<float>();
    else if (Dm) {
        if (bD.put(Dm, nd)) return -1;
        dD = bD.as<float>();
    }
    const std::vector<double> f(fro_part ? (size_t)mt * nt : 0, fro_sentinel);
    if ((fro_part && bF.put(f.data(), f.size())) || (krange && bK.put(krange, (size_t)2 * mt)) || (dev_scale && bS.put(dev_scale, (size_t)1)))
        return -1;
    ldi_gemm(nullptr, 0, M, N, K, alpha, bA.as<float>(), lda, bB.as<float>(), ldb, beta, dD, ldd, gamma, bC.as<float>(), ldc,
             fro_part ? bF.as<double>() : nullptr, krange ? bK.as<int2>() : nullptr, upper_only ? 1 : 0, dev_scale ? bS.as<float>() : nullptr);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(0));
    return bC.fetch(C, nc) || (fro_part && bF.fetch(fro_part, f.size())) ? -1 : 0;
}

// k_ldi_ritz once on the coefficients of a CG of m iterations: rz[k] = r_k . z_k and alpha[k], what the solver's CG leaves in
// hist[k] and hist[cap + k].  out3: c = 1.9 / (ritz_min + ritz_max) and the two Ritz values (all zero: no usable estimate).
int ps_debug_ldi_ritz(const double* rz, const double* alpha, int32_t m, float* out3) {
    if (!out3 || m < 0 || (m > 0 && (!rz || !alpha))) return fail("ps_debug_ldi_ritz: bad argument");
    if (need_device()) return -1;
    const int cap = std::max(m, 1);
    std::vector<double> hist(2 * (size_t)cap, 0.0);
    for (int k = 0; k < m; ++k) { hist[k] = rz[k]; hist[cap + k] = alpha[k]; }
    int32_t stw[ST_NWORDS] = {};
    stw[ST_PCG_ITERS] = m;
    const float before[3] = {-1.f, -1.f, -1.f};               // (the kernel writes all three words whatever it finds)
    DevBuf bh, bs, bo;
    if (bh.put(hist.data(), hist.size()) || bs.put(stw, (size_t)ST_NWORDS) || bo.put(before, (size_t)3)) return -1;
    hipLaunchKernelGGL(k_ldi_ritz, dim3(1), dim3(64), 0, 0, (const double*)bh.as<double>(), cap, (const int32_t*)bs.as<int32_t>(), bo.as<float>());
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(0));
    return bo.fetch(out3, (size_t)3);
}
