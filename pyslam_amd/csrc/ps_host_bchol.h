// ps_host_bchol.h -- the ONE launch sequence of the blocked dense factorisation chain (kernels: ps_k_coarse.h k_bchol_panel /
// k_bchol_update / k_btri_inverse / k_btri_merge / k_btri_clear, ps_k_xcg.h k_xcg_ainv).  Part of ps_core.hip.
//
// Callers: the coarse level beyond 90 unknowns (coarse_factor, ps_host_cg.h: side stream), the lagged inverse's direct seed
// (ldi_direct_enqueue, ps_host_ldi.h: its own stream), ps_covariance_marginals (ps_abi_cov.h: the handle's stream, with its
// pivot check and a synchronisation between BCHOL_FACTOR and BCHOL_INVERSE), the test entries ps_debug_dense_factor /
// ps_debug_factor_stress mode 4, and -- through SpdSolve below: BCHOL_FACTOR only, substitutions instead of an inverse --
// ps_sparse_normal_direct (ps_abi_small.h) and the Sim(3) pose graph's s3g_iteration (ps_host_sim3pg.h).  Streams, buffers
// and what runs between the stages stay with the caller; the order of launches and their grids are here and nowhere else.
#pragma once

enum {
    BCHOL_FACTOR = 1,      // A (n x n, lower triangle read) -> L below the 24 x 24 diagonal tiles, in place; Tinv: the tiles' inverses
    BCHOL_INVERSE = 2,     // -> Li = L^-1 (lower triangle and the diagonal blocks' upper parts written) and LiT = its transpose
    BCHOL_DENSE_OUT = 4,   // with BCHOL_INVERSE: Li and LiT zero-filled first, the merge intermediates cleared from LiT after
                           // (the folded CG reads both as dense matrices; without it everything outside the lower triangle of Li /
                           // the upper triangle of LiT beyond the 192 x 192 diagonal blocks is unspecified)
    BCHOL_AINV = 8         // -> Ainv = Li^T Li in fp32, leading dimension ld >= n, both triangles
};

inline void bchol_ainv(hipStream_t st, int n, const double* Li, float* Ainv, int ld) {
    const int nt = cdiv(n, PS_AI_T);
    hipLaunchKernelGGL(k_xcg_ainv, dim3(nt * (nt + 1) / 2), dim3(256), 0, st, n, Li, Ainv, ld);
}

// workgroups of step (j0, w)'s panel launch: whole rows per workgroup (ps_bchol_slab)
inline int bchol_panel_grid(int m, int w) {
    int row, col;
    return ps_bchol_slab(m, w, 0, 0, 0, &row, &col);
}

inline int bchol_chain(hipStream_t st, int n, int stages, double* A, double* Tinv, int32_t* stat, double* Li, double* LiT,
                       float* Ainv, int ld) {
    if (stages & BCHOL_FACTOR) {                           // blocked right-looking Cholesky over the whole chip
        const int nsteps = cdiv(n, PS_BC_W);
        for (int s2 = 0; s2 < nsteps; ++s2) {
            const int j0 = s2 * PS_BC_W, w = std::min(PS_BC_W, n - j0), m = n - j0 - w;
            hipLaunchKernelGGL(k_bchol_panel, dim3(bchol_panel_grid(m, w)), dim3(256), 0, st, n, j0, A,
                               Tinv + (size_t)s2 * PS_BC_W * PS_BC_W, stat);
            if (m > 0) {
                const int nt = cdiv(m, 32);
                hipLaunchKernelGGL(k_bchol_update, dim3(nt * (nt + 1) / 2), dim3(256), 0, st, n, j0, w, A);
            }
        }
    }
    if (stages & BCHOL_INVERSE) {
        // L^-1: diagonal blocks by substitution, the rest merged level by level with triangular products
        const bool dense_out = (stages & BCHOL_DENSE_OUT) != 0;
        if (dense_out) {
            HIP_OK(hipMemsetAsync(Li, 0, (size_t)n * n * sizeof(double), st));
            HIP_OK(hipMemsetAsync(LiT, 0, (size_t)n * n * sizeof(double), st));
        }
        const size_t inv_lds = ((size_t)PS_BI_S0 + PS_BC_W) * PS_BI_CW * sizeof(double);
        hipLaunchKernelGGL(k_btri_inverse, dim3(cdiv(n, PS_BI_CW)), dim3(256), inv_lds, st, n, A, Tinv, Li, LiT);
        for (int s2 = PS_BI_S0; s2 < n; s2 *= 2) {
            const int pairs = cdiv(n, 2 * s2), nt = cdiv(s2, PS_BM_T);
            for (int stage = 0; stage < 2; ++stage)
                hipLaunchKernelGGL(k_btri_merge, dim3(pairs * nt * nt), dim3(256), 0, st, n, s2, stage, A, Li, LiT);
        }
        if (dense_out)
            hipLaunchKernelGGL(k_btri_clear, dim3(cdiv((long)n * n, 256)), dim3(256), 0, st, n, LiT);
    }
    if (stages & BCHOL_AINV) bchol_ainv(st, n, Li, Ainv, ld);
    return 0;
}

// doubles of Tinv (the inverses of the diagonal tiles) and of k_spd_residual's partials (r.r, b.b per workgroup) for n unknowns
inline size_t bchol_tinv_count(long n) { return (size_t)cdiv(n, PS_BC_W) * PS_BC_W * PS_BC_W; }
inline size_t spd_part_count(long n) { return (size_t)2 * cdiv(n, 4); }

// The dense direct solve through the factor (kernels: ps_sparse.h): a view of the caller's buffers.  What is solved, how often
// it is refined and who reads the residual's partials stay with the caller.
struct SpdSolve {
    int n;
    double *A, *Tinv;              // A: factored in place; Tinv: bchol_tinv_count(n)
    int32_t* stat;
    int factor(hipStream_t st) const { return bchol_chain(st, n, BCHOL_FACTOR, A, Tinv, stat, nullptr, nullptr, nullptr, 0); }
    void solve_into(hipStream_t st, double* v) const {     // v <- (L L^T)^-1 v
        hipLaunchKernelGGL(k_spd_subst, dim3(1), dim3(512), 0, st, n, (const double*)A, (const double*)Tinv, v, 0);
        hipLaunchKernelGGL(k_spd_subst, dim3(1), dim3(512), 0, st, n, (const double*)A, (const double*)Tinv, v, 1);
    }
    // res = b - H x with H the unfactored matrix; part: spd_part_count(n)
    void residual(hipStream_t st, const double* H, const double* b, const double* x, double* res, double* part) const {
        hipLaunchKernelGGL(k_spd_residual, dim3(cdiv(n, 4)), dim3(256), 0, st, n, H, b, x, res, part);
    }
    void add(hipStream_t st, const double* d, double* x) const {   // x += d
        hipLaunchKernelGGL(k_spd_axpy, dim3(cdiv(n, 256)), dim3(256), 0, st, n, d, x);
    }
};
