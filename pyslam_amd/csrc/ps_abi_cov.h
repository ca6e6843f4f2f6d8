// ps_abi_cov.h -- C ABI: batched marginal covariances of every reduced pose and variable landmark (kernels: ps_k_covmarg.h).
// Part of ps_core.hip (inside its extern "C" block, after ps_abi_solver.h).
//
// ps_covariance_marginals densifies the reduced system that ps_covariance_begin left in S (n = nr * D unknowns, at most
// PS_COV_DENSE_MAX_UNKNOWNS), factors it, forms Sigma_pp = S^-1 in fp64 and keeps it on the handle; the pose blocks are its
// diagonal blocks, the landmark blocks follow from it and the Schur elimination's Z rows / C^-1 factors of the same
// linearisation.  ps_covariance_pose_blocks reads further D x D blocks of the kept Sigma_pp; ps_covariance_cross_blocks any
// block of the full covariance (pose-pose, pose-landmark either way, landmark-landmark) from the same Sigma_pp, Z and C^-1.

// one device block: [A: S, then Sigma (n^2) | L^-1 (n^2) | L^-T (n^2) | Tinv | diag (n) | pose out (nr D^2) | landmark out (9 nv) | stat]
static size_t cov_layout(const ps_problem* h, size_t off[8]) {
    const size_t n = (size_t)h->nr * h->D, nn = n * n;
    const size_t sizes[8] = {nn, nn, nn, bchol_tinv_count((long)n), n, (size_t)h->nr * h->D * h->D,
                             (size_t)h->nv * 9, (size_t)ST_NWORDS};
    size_t at = 0;
    for (int k = 0; k < 8; ++k) { off[k] = at; at += (sizes[k] + 31) / 32 * 32; }     // (256-byte aligned pieces)
    return at;
}

int ps_covariance_marginals(ps_problem* h, double* pose_blocks, double* point_blocks) {
    if (!h) return fail("null argument");
    if (!h->cov_ready) return fail("ps_covariance_marginals: call ps_covariance_begin first (any linearisation invalidates it)");
    const int D = h->D, nr = h->nr, nv = h->nv;
    const long n = (long)nr * D;
    if (n > PS_COV_DENSE_MAX_UNKNOWNS)
        return fail("ps_covariance_marginals: the reduced system has " + std::to_string(n) + " unknowns, above the dense limit "
                    "PS_COV_DENSE_MAX_UNKNOWNS = " + std::to_string(PS_COV_DENSE_MAX_UNKNOWNS) +
                    " (nr * dof); use get_covariance_block (ps_covariance_column), which has no such limit");
    if (nv > 0 && D != 6) return fail("ps_covariance_marginals: landmarks on a problem whose poses are not SE(3)");
    hipStream_t st = h->stream;
    size_t off[8];
    const size_t total = cov_layout(h, off);
    if (!h->cov_buf) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, total * sizeof(double));
        if (e != hipSuccess)
            return fail(std::string("ps_covariance_marginals: hipMalloc of the dense block (") + std::to_string(total * 8 >> 20) +
                        " MiB): " + hipGetErrorString(e));
        h->cov_buf = (double*)p;
    }
    double* A = h->cov_buf + off[0];
    double* Li = h->cov_buf + off[1];
    double* LiT = h->cov_buf + off[2];
    double* Tinv = h->cov_buf + off[3];
    double* diag = h->cov_buf + off[4];
    double* pose_out = h->cov_buf + off[5];
    double* lm_out = h->cov_buf + off[6];
    int32_t* stat = reinterpret_cast<int32_t*>(h->cov_buf + off[7]);
    HIP_OK(hipMemsetAsync(stat, 0, ST_NWORDS * sizeof(int32_t), st));
    if (n > 0) {
        // S -> dense, Cholesky (the lagged inverse's direct-seed chain, on the handle's stream), pivots checked before going on
        HIP_OK(hipMemsetAsync(A, 0, (size_t)n * n * sizeof(double), st));
        if (D == 6) hipLaunchKernelGGL(k_ldi_dense64<6>, dim3(h->nnzb), dim3(64), 0, st, h->brow_of, h->col_idx, h->S, A, (int)n);
        else hipLaunchKernelGGL(k_ldi_dense64<3>, dim3(h->nnzb), dim3(64), 0, st, h->brow_of, h->col_idx, h->S, A, (int)n);
        hipLaunchKernelGGL(k_cov_diag_save, dim3(cdiv(n, 256)), dim3(256), 0, st, (int)n, A, diag);
        if (bchol_chain(st, (int)n, BCHOL_FACTOR, A, Tinv, stat, nullptr, nullptr, nullptr, 0)) return -1;
        hipLaunchKernelGGL(k_cov_pivot_check, dim3(cdiv(n, 256)), dim3(256), 0, st, (int)n, diag, Tinv, stat);
        int32_t hstat[ST_NWORDS];
        HIP_OK(hipMemcpyAsync(hstat, stat, sizeof(hstat), hipMemcpyDeviceToHost, st));
        if (sync(h)) return -1;
        if (hstat[ST_DIAG_FAIL])
            return fail("ps_covariance_marginals: the reduced system is singular or not positive definite (gauge freedom? hold a "
                        "pose constant or add a prior)");
        // L^-1 and L^-T, then Sigma = L^-T L^-1 into A's place (A is not read after the merges), mirrored
        // (k_cov_sigma reads the lower triangle of L^-1 only: the chain's form without zero fill, ps_host_bchol.h)
        if (bchol_chain(st, (int)n, BCHOL_INVERSE, A, Tinv, stat, Li, LiT, nullptr, 0)) return -1;
        const int nt = cdiv(n, PS_CS_T);
        hipLaunchKernelGGL(k_cov_sigma, dim3(nt * (nt + 1) / 2), dim3(256), 0, st, (int)n, Li, A);
        hipLaunchKernelGGL(k_cov_mirror, dim3(cdiv(n, 32), cdiv(n, 32)), dim3(256), 0, st, (int)n, A);
        if (pose_blocks) {
            hipLaunchKernelGGL(k_cov_gather, dim3(cdiv((long)nr * D * D, 256)), dim3(256), 0, st, nr, D, (int)n,
                               (const int32_t*)nullptr, (const int32_t*)nullptr, A, pose_out);
            HIP_OK(hipMemcpyAsync(pose_blocks, pose_out, (size_t)nr * D * D * sizeof(double), hipMemcpyDeviceToHost, st));
        }
    }
    std::vector<double> lm;
    if (point_blocks && nv > 0) {
        hipLaunchKernelGGL(k_cov_landmarks, dim3(cdiv(nv, 256 / PS_LM_GROUP)), dim3(256), 0, st, nv, (int)n, h->lm_ptr, h->Z,
                           h->Cinv, n > 0 ? A : (const double*)nullptr, lm_out);
        lm.resize((size_t)nv * 9);
        HIP_OK(hipMemcpyAsync(lm.data(), lm_out, lm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (sync(h)) return -1;
    for (int s2 = 0; !lm.empty() && s2 < nv; ++s2)       // internal slot order -> the caller's vid order
        std::memcpy(point_blocks + 9 * (size_t)h->h_vid_of_slot[s2], &lm[9 * (size_t)s2], 9 * sizeof(double));
    h->cov_sigma_epoch = h->cov_epoch;
    return 0;
}

int ps_covariance_pose_blocks(ps_problem* h, int64_t n, const int32_t* a, const int32_t* b, double* out) {
    if (!h) return fail("null argument");
    if (!h->cov_ready || !h->cov_buf || h->cov_sigma_epoch != h->cov_epoch)
        return fail("ps_covariance_pose_blocks: no dense inverse on the handle (call ps_covariance_marginals after ps_covariance_begin; "
                    "any linearisation invalidates it)");
    if (n < 0 || (n > 0 && (!a || !b || !out))) return fail("ps_covariance_pose_blocks: null argument");
    if (n == 0) return 0;
    for (int64_t k = 0; k < n; ++k)
        if (a[k] < 0 || a[k] >= h->nr || b[k] < 0 || b[k] >= h->nr)
            return fail("ps_covariance_pose_blocks: reduced pose index out of range");
    const int D = h->D;
    const size_t DD = (size_t)D * D;
    // chunks of at most as many blocks as the pose output piece holds: indices and results pass through it
    size_t off[8];
    cov_layout(h, off);
    const size_t cap = ((size_t)h->nr * DD + 31) / 32 * 32;                  // doubles in the pose output piece
    const long chunk = (long)std::max<size_t>(1, cap / (DD + 1));           // DD results + two int32 indices per block
    double* buf = h->cov_buf + off[5];
    for (int64_t k0 = 0; k0 < n; k0 += chunk) {
        const int m = (int)std::min<int64_t>(chunk, n - k0);
        int32_t* da = reinterpret_cast<int32_t*>(buf + (size_t)m * DD);
        int32_t* db = da + m;
        HIP_OK(hipMemcpyAsync(da, a + k0, m * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIP_OK(hipMemcpyAsync(db, b + k0, m * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_cov_gather, dim3(cdiv((long)m * DD, 256)), dim3(256), 0, h->stream, m, D, h->nr * D, da, db,
                           h->cov_buf + off[0], buf);
        HIP_OK(hipMemcpyAsync(out + (size_t)k0 * DD, buf, m * DD * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (sync(h)) return -1;
    }
    return 0;
}

// pairs per pass of ps_covariance_cross_blocks through its fixed buffer (36 doubles of result + four int32 per pair: 10 MiB)
#define PS_COV_CROSS_CHUNK 32768

int ps_covariance_cross_blocks(ps_problem* h, int64_t n, const int32_t* kind_a, const int32_t* a, const int32_t* kind_b,
                               const int32_t* b, double* out) {
    if (!h) return fail("null argument");
    if (!h->cov_ready || !h->cov_buf || h->cov_sigma_epoch != h->cov_epoch)
        return fail("ps_covariance_cross_blocks: no dense inverse on the handle (call ps_covariance_marginals after "
                    "ps_covariance_begin; any linearisation invalidates it)");
    if (n < 0 || (n > 0 && (!kind_a || !a || !kind_b || !b || !out))) return fail("ps_covariance_cross_blocks: null argument");
    for (int64_t k = 0; k < n; ++k) {
        const int32_t kinds[2] = {kind_a[k], kind_b[k]}, ix[2] = {a[k], b[k]};
        for (int s2 = 0; s2 < 2; ++s2) {
            if (kinds[s2] != 0 && kinds[s2] != 1)
                return fail("ps_covariance_cross_blocks: pair " + std::to_string(k) + ": kind " + std::to_string(kinds[s2]) +
                            " (0 = reduced pose, 1 = variable landmark)");
            if (kinds[s2] == 1 && h->D != 6)
                return fail("ps_covariance_cross_blocks: landmarks on a problem whose poses are not SE(3)");
            if (ix[s2] < 0 || ix[s2] >= (kinds[s2] == 0 ? h->nr : h->nv))
                return fail("ps_covariance_cross_blocks: pair " + std::to_string(k) + ": " +
                            (kinds[s2] == 0 ? "reduced pose" : "landmark") + " index " + std::to_string(ix[s2]) + " out of range");
        }
    }
    if (n == 0) return 0;
    if (!h->cov_xbuf) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, (size_t)PS_COV_CROSS_CHUNK * (36 + 2) * sizeof(double));
        if (e != hipSuccess) return fail(std::string("ps_covariance_cross_blocks: hipMalloc: ") + hipGetErrorString(e));
        h->cov_xbuf = (double*)p;
    }
    size_t off[8];
    cov_layout(h, off);
    const double* Sigma = h->cov_buf + off[0];
    double* dres = h->cov_xbuf;
    int32_t* drec = reinterpret_cast<int32_t*>(h->cov_xbuf + (size_t)PS_COV_CROSS_CHUNK * 36);
    std::vector<int32_t> rec((size_t)4 * std::min<int64_t>(n, PS_COV_CROSS_CHUNK));
    for (int64_t k0 = 0; k0 < n; k0 += PS_COV_CROSS_CHUNK) {
        const int m = (int)std::min<int64_t>(PS_COV_CROSS_CHUNK, n - k0);
        for (int k = 0; k < m; ++k) {                    // landmarks: the caller's vid -> the internal slot
            rec[4 * k] = kind_a[k0 + k];
            rec[4 * k + 1] = kind_a[k0 + k] ? h->h_slot_of_vid[a[k0 + k]] : a[k0 + k];
            rec[4 * k + 2] = kind_b[k0 + k];
            rec[4 * k + 3] = kind_b[k0 + k] ? h->h_slot_of_vid[b[k0 + k]] : b[k0 + k];
        }
        HIP_OK(hipMemcpyAsync(drec, rec.data(), (size_t)4 * m * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_cov_cross, dim3(cdiv(m, 256 / PS_LM_GROUP)), dim3(256), 0, h->stream, m, h->nr * h->D, h->D, drec,
                           h->lm_ptr, h->Z, h->Cinv, Sigma, dres);
        HIP_OK(hipMemcpyAsync(out + (size_t)k0 * 36, dres, (size_t)m * 36 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (sync(h)) return -1;
    }
    return 0;
}
