// ps_k_lm.h -- adaptive Levenberg-Marquardt: the predicted decrease of the quadratic model, summed on the device in the tail.
// Part of ps_core.hip (one translation unit; included from ps_kernels.h in front of the tail's kernels, which call the helper).
//
//   model_decrease = 0.5 h^T (lambda D h + g),   D = diag(J~^T J~) (undamped),   (H + lambda D) h = g
//
// In Schur form, with C_l = H_ll + lambda diag(H_ll) = L L^T, M = L^-1 (the six words of `Cinv`) and cvec = M b_l:
//   h^T g   = h_p^T g_red + sum_l |cvec_l|^2                        (b_l^T C_l^-1 b_l = |M b_l|^2)
//   h^T D h = sum_p D_p h_p^2 + sum_l diag(C_l) / (1 + lambda) . h_l^2,   diag(C_l)_k = sum_j L_kj^2,  L = M^-1 (3 x 3, lower)
// The landmark sums are formed by the back-substitution's head lanes (k_backsub<true>, k_backsub_packed<true>: one partial per
// workgroup), the pose sums by k_lm_pose_sums (D_p from the pose pass's undamped diagonal sums, still in its partials, and the
// diagonal entries of the factor blocks, still in their scratch rows), and k_lm_total adds the partials in a fixed order.

PS_DEV double strided_sum8(const double* __restrict__ p, int n);      // (ps_k_tail.h)

// a landmark's terms of 2 model_decrease from M = (M00 M10 M11 M20 M21 M22), cvec and its step d:
// |cvec|^2 + lambda / (1 + lambda) . sum_k diag(C)_k d_k^2
PS_DEV double lm_landmark_terms(const double* __restrict__ m, const double* __restrict__ cv, double d0, double d1, double d2,
                                double lam_ratio) {
    const double l00 = 1.0 / m[0], l11 = 1.0 / m[2], l22 = 1.0 / m[5];
    const double l10 = -m[1] * l00 * l11;
    const double l21 = -m[4] * l11 * l22;
    const double l20 = -(m[3] * l00 + m[4] * l10) * l22;
    const double c0 = l00 * l00, c1 = l10 * l10 + l11 * l11, c2 = (l20 * l20 + l21 * l21) + l22 * l22;
    return ((cv[0] * cv[0] + cv[1] * cv[1]) + cv[2] * cv[2]) + lam_ratio * ((c0 * d0 * d0 + c1 * d1 * d1) + c2 * d2 * d2);
}

// pose terms: thread (rid, r) of the first nr D adds h (lambda D_reproj h + g_red); thread (slot, r) of the touched DIAGONAL
// factor slots adds lambda D_factor h^2.  One partial per workgroup.
template <int D>
__global__ __launch_bounds__(256) void k_lm_pose_sums(
    int nr, const double* __restrict__ x, const double* __restrict__ g,
    const int32_t* __restrict__ pitem_ptr /* NULL: no reprojection terms */, const double* __restrict__ ppartial,
    int nslots, const int32_t* __restrict__ eslots, const int32_t* __restrict__ eptr, const int2* __restrict__ eitems,
    const int32_t* __restrict__ slot_is_diag, const int32_t* __restrict__ brow_of, const double* __restrict__ scratch,
    double lambda, const int32_t* __restrict__ gate, double* __restrict__ part)
{
    __shared__ double lds[16];
    if (gate && gate[ST_PCG_DONE] != 1) return;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    double term = 0.0;
    if (t < nr * D) {
        const int rid = t / D, r = t - rid * D;
        double d = 0.0;
        if (pitem_ptr != nullptr && D == 6)
            for (int it = pitem_ptr[rid]; it < pitem_ptr[rid + 1]; ++it) d += ppartial[(size_t)it * 33 + 27 + r];   // (PS_NPOSE_ACC; 27..32: the damping sums)
        const double xv = x[t];
        term = xv * (lambda * d * xv + g[t]);
    } else if (t - nr * D < nslots * D) {
        const int u = t - nr * D, si = u / D, r = u - si * D;
        if (slot_is_diag[si]) {
            double d = 0.0;
            for (int k = eptr[si]; k < eptr[si + 1]; ++k) d += scratch[(size_t)eitems[k].x + r * D + r];
            const double xv = x[(size_t)brow_of[eslots[si]] * D + r];
            term = lambda * d * xv * xv;
        }
    }
    term = block_sum(term, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = term;
}

// model_decrease = 0.5 (sum of the pose partials + sum of the landmark partials) into its scalar slot, in front of the
// reduction that publishes the slots (k_reduce3).  One workgroup, fixed order.
__global__ __launch_bounds__(256) void k_lm_total(int np, const double* __restrict__ pp, int nl, const double* __restrict__ pl,
                                                  const int32_t* __restrict__ gate, double* __restrict__ out)
{
    __shared__ double lds[16];
    if (gate && gate[ST_PCG_DONE] != 1) return;
    double a = strided_sum8(pp, np), b = strided_sum8(pl, nl);
    a = block_sum(a, lds);
    b = block_sum(b, lds);
    if (threadIdx.x == 0) out[0] = 0.5 * (a + b);
}
