// ps_k_twoview.h -- monocular two-view initialisation: essential-matrix RANSAC on the device (gfx950, fp64).
// Part of ps_core.hip (one translation unit; included after ps_ransac_core.h and ps_ransac.h).  pyslam_amd/pipelines/epipolar.py is the same
// definition in numpy; this project has no reference counterpart for it (as for MonoCamera and the matcher).
//
// Input: N correspondences obs_1, obs_2 (pixels), a pinhole camera (cu, cv, fu, fv), H minimal sets of 8 point indices.
//   x = ((u - cu) / fu, (v - cv) / fv, 1)                      normalised coordinates, once per call (k_tv_normalise: 32 B per point)
//   hypothesis h: the 8 x 9 matrix A with rows kron(x_2, x_1); its null vector f by Gaussian elimination with COMPLETE pivoting on A
//     itself (A^T A is never formed: that would square sigma_1 / sigma_8); F = f as 3 x 3, row-major, so that x_2^T F x_1 = 0.
//     A sample with a repeated index, or with a pivot whose magnitude is not above 1e-12 of the first (largest) pivot, is
//     DEGENERATE: flag 1, E = 0, count 0.  So is an F of rank < 2.
//   projection: F = U S V^T by a one-sided Jacobi SVD of the 3 x 3 (rc_jacobi3, ps_ransac_core.h), E = u_1 v_1^T + u_2 v_2^T
//     (= U diag(1, 1, 0) V^T, Frobenius norm sqrt 2).
//   SIGN RULE: the entry of E with the largest absolute value is positive; of equal magnitudes the one with the lowest row-major
//     index decides.
//   score: r = x_2^T E x_1, l = E x_1, l' = E^T x_2; squared Sampson distance in pixel units
//     d = r^2 / ((l_1^2 + l'_1^2) / fu^2 + (l_2^2 + l'_2^2) / fv^2);  inlier: denominator > 0 and d < thresh.
//   best: the FIRST hypothesis with the maximal count (np.argmax); its mask by one rescoring pass.
//   refit over the inliers of the best hypothesis: Hartley normalisation of either image's normalised coordinates (centroid c,
//     s = sqrt 2 / mean distance to c, x~ = s (x - c)), M = sum a a^T with a = kron(x~_2, x~_1), the eigenvector of M's smallest
//     eigenvalue by cyclic Jacobi, F = T_2^T F~ T_1, projection and sign as above, rescoring.  The refit is kept if it is not
//     degenerate and its count is not lower than the raw hypothesis'.
//   decomposition of the winner: u_3 the unit left null vector of E, largest component positive (lowest index decides);
//     (u_1, v_1), (u_2, v_2) its singular pairs with u_1 x u_2 = u_3; v_3 = v_1 x v_2; U = [u_1 u_2 u_3], V = [v_1 v_2 v_3] (both of
//     determinant +1, hence det R = +1), W = [0 -1 0; 1 0 0; 0 0 1].  Candidates in this order:
//       0: (U W V^T, +u_3)   1: (U W V^T, -u_3)   2: (U W^T V^T, +u_3)   3: (U W^T V^T, -u_3)
//     For every inlier the two rays t + lambda R x_1 and mu x_2 (camera-2 frame) are intersected by the midpoint formula; the
//     candidate's count is the number of inliers with det > 0, lambda > 0 and mu > 0.  Highest count wins, lowest index first.
//     T_21 = [R | t], |t| = 1; parallax of an inlier = angle between R x_1 and x_2 in degrees.
//
// No atomics; every sum is reduced in a fixed order (rc_block_sum: lane tree, then waves 0..3; then workgroups in slot order), so two calls on the
// same input are bit-identical.  The small dense solves run in lane 0 on matrices kept in LDS (runtime-indexed pivoting on a
// private array would go through scratch); the scoring pass is one coalesced 32 B read per point and hypothesis.
#pragma once
#include "ps_ransac_core.h"

// ---- scalar building blocks (no thread indices: pointers may address LDS or private memory) ----------------------------------

PS_DEV void tv_fix_sign(double* __restrict__ E) {
    double big = E[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) if (fabs(E[k]) > fabs(big)) big = E[k];       // the first of equal magnitudes stays
    if (big < 0.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = -E[k];
    }
}

// The two leading singular pairs of the row-major 3 x 3 F (rc_jacobi3 on the columns of F, sorted).
// false: rank < 2 (sigma_2 <= 1e-12 sigma_1) or a non-finite entry.
PS_DEV bool tv_svd2(const double* __restrict__ F, double* __restrict__ u1, double* __restrict__ u2, double* __restrict__ v1,
                    double* __restrict__ v2)
{
    double A[3][3], V[3][3], sg[3];                                    // A[col][row], V[col][row]
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) A[c][r] = F[3 * r + c];
    rc_jacobi3<false>(A, V, sg);                                       // (a non-finite column pair is skipped)
    rc_sort3(sg, A, V);
    if (!(sg[0] > 0.0) || !(sg[1] > 1e-12 * sg[0]) || !(sg[0] < 1e300)) return false;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        u1[r] = A[0][r] / sg[0]; u2[r] = A[1][r] / sg[1];
        v1[r] = V[0][r]; v2[r] = V[1][r];
    }
    return true;
}

// E = U diag(1, 1, 0) V^T of the row-major F, with the sign rule.  false (E = 0): F has rank < 2.
PS_DEV bool tv_project(const double* __restrict__ F, double* __restrict__ E) {
    double u1[3], u2[3], v1[3], v2[3];
    if (!tv_svd2(F, u1, u2, v1, v2)) {
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = 0.0;
        return false;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) E[3 * r + c] = u1[r] * v1[c] + u2[r] * v2[c];
    tv_fix_sign(E);
    return true;
}

// Unit null vector f (9) of the 8 x 9 row-major A (destroyed) by elimination with complete pivoting.  cp (9 ints) and x (9)
// are work space.  false: a pivot not above 1e-12 of the first one.
PS_DEV bool tv_null8x9(double* __restrict__ A, int* __restrict__ cp, double* __restrict__ x, double* __restrict__ f) {
    for (int c = 0; c < 9; ++c) cp[c] = c;
    double p0 = 0.0;
    for (int k = 0; k < 8; ++k) {
        int pr = k, pc = k;
        double best = -1.0;
        for (int r = k; r < 8; ++r)
            for (int c = k; c < 9; ++c) {
                const double a = fabs(A[9 * r + c]);
                if (a > best) { best = a; pr = r; pc = c; }       // the first maximum in row-major order
            }
        if (pr != k)
            for (int c = 0; c < 9; ++c) { const double w = A[9 * k + c]; A[9 * k + c] = A[9 * pr + c]; A[9 * pr + c] = w; }
        if (pc != k) {
            for (int r = 0; r < 8; ++r) { const double w = A[9 * r + k]; A[9 * r + k] = A[9 * r + pc]; A[9 * r + pc] = w; }
            const int w = cp[k]; cp[k] = cp[pc]; cp[pc] = w;
        }
        const double piv = A[9 * k + k];
        if (k == 0) p0 = fabs(piv);
        if (!(fabs(piv) > 0.0) || !(fabs(piv) > 1e-12 * p0) || !(p0 < 1e300)) return false;
        for (int r = k + 1; r < 8; ++r) {
            const double m = A[9 * r + k] / piv;
            for (int c = k + 1; c < 9; ++c) A[9 * r + c] -= m * A[9 * k + c];
        }
    }
    x[8] = 1.0;
    double n2 = 1.0;
    for (int k = 7; k >= 0; --k) {
        double s = 0.0;
        for (int c = k + 1; c < 9; ++c) s += A[9 * k + c] * x[c];
        x[k] = -s / A[9 * k + k];
        n2 += x[k] * x[k];
    }
    const double inv = 1.0 / sqrt(n2);
    for (int c = 0; c < 9; ++c) f[cp[c]] = x[c] * inv;
    return true;
}

// Eigenvector f (9) of the smallest eigenvalue of the symmetric 9 x 9 M (row-major, destroyed) by cyclic Jacobi; Q (81) is work space.
PS_DEV void tv_eig9_smallest(double* __restrict__ M, double* __restrict__ Q, double* __restrict__ f) {
    double fro = 0.0;
    for (int k = 0; k < 81; ++k) { Q[k] = (k % 10 == 0) ? 1.0 : 0.0; fro += M[k] * M[k]; }
    fro = sqrt(fro);
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double apq = M[9 * p + q];
                if (!(fabs(apq) > 1e-19 * fro)) continue;
                rotated = true;
                const double theta = (M[9 * q + q] - M[9 * p + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < 9; ++r) {                  // columns p, q:  M <- M J
                    const double mp = M[9 * r + p], mq = M[9 * r + q];
                    M[9 * r + p] = c * mp - s * mq; M[9 * r + q] = s * mp + c * mq;
                }
                for (int r = 0; r < 9; ++r) {                  // rows p, q:  M <- J^T M
                    const double mp = M[9 * p + r], mq = M[9 * q + r];
                    M[9 * p + r] = c * mp - s * mq; M[9 * q + r] = s * mp + c * mq;
                }
                M[9 * p + q] = 0.0; M[9 * q + p] = 0.0;
                for (int r = 0; r < 9; ++r) {
                    const double qp = Q[9 * r + p], qq = Q[9 * r + q];
                    Q[9 * r + p] = c * qp - s * qq; Q[9 * r + q] = s * qp + c * qq;
                }
            }
        if (!rotated) break;
    }
    int m = 0;
    for (int k = 1; k < 9; ++k) if (M[10 * k] < M[10 * m]) m = k;
    for (int r = 0; r < 9; ++r) f[r] = Q[9 * r + m];
}

// F = T_2^T F~ T_1 with T_k = [s_k 0 -s_k cx_k; 0 s_k -s_k cy_k; 0 0 1]  (hn = cx_1 cy_1 s_1 cx_2 cy_2 s_2)
PS_DEV void tv_denormalise(const double* __restrict__ Fn, const double* __restrict__ hn, double* __restrict__ F) {
    double G[9];                                               // G = F~ T_1
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        G[3 * r] = Fn[3 * r] * hn[2];
        G[3 * r + 1] = Fn[3 * r + 1] * hn[2];
        G[3 * r + 2] = Fn[3 * r + 2] - hn[2] * (Fn[3 * r] * hn[0] + Fn[3 * r + 1] * hn[1]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        F[c] = hn[5] * G[c];
        F[3 + c] = hn[5] * G[3 + c];
        F[6 + c] = G[6 + c] - hn[5] * (hn[3] * G[c] + hn[4] * G[3 + c]);
    }
}

// inlier test of one correspondence (the operations of epipolar.sampson in the same order, no contraction)
PS_DEV bool tv_inlier(const double* __restrict__ E, double x1, double y1, double x2, double y2, double ifu2, double ifv2,
                      double thresh)
{
#pragma clang fp contract(off)
    const double l0 = E[0] * x1 + E[1] * y1 + E[2];
    const double l1 = E[3] * x1 + E[4] * y1 + E[5];
    const double l2 = E[6] * x1 + E[7] * y1 + E[8];
    const double r = x2 * l0 + y2 * l1 + l2;
    const double m0 = E[0] * x2 + E[3] * y2 + E[6];
    const double m1 = E[1] * x2 + E[4] * y2 + E[7];
    const double den = (l0 * l0 + m0 * m0) * ifu2 + (l1 * l1 + m1 * m1) * ifv2;
    const double d = (r * r) / den;
    return den > 0.0 && d < thresh;                              // NaN compares false
}

// The rotations of candidates 0 / 1 (Ra) and 2 / 3 (Rb) and the translation direction t = +u_3 of the essential matrix E.
PS_DEV bool tv_decompose(const double* __restrict__ E, double* __restrict__ Ra, double* __restrict__ Rb, double* __restrict__ t) {
    double u1[3], u2[3], v1[3], v2[3];
    if (!tv_svd2(E, u1, u2, v1, v2)) return false;
    double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    double big = u3[0];
    if (fabs(u3[1]) > fabs(big)) big = u3[1];
    if (fabs(u3[2]) > fabs(big)) big = u3[2];
    if (big < 0.0) {                                           // the other orientation: (u_1, v_1) -> (-u_1, -v_1)
#pragma unroll
        for (int r = 0; r < 3; ++r) { u1[r] = -u1[r]; v1[r] = -v1[r]; u3[r] = -u3[r]; }
    }
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    // U W = [u_2, -u_1, u_3],  U W^T = [-u_2, u_1, u_3]
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double w = u2[r] * v1[c] - u1[r] * v2[c], z = u3[r] * v3[c];
            Ra[3 * r + c] = w + z;
            Rb[3 * r + c] = z - w;
        }
    t[0] = u3[0]; t[1] = u3[1]; t[2] = u3[2];
    return true;
}

// Midpoint intersection of  t + lambda (R x_1)  and  mu x_2:  true when both depths are positive.  cosang: cosine of the parallax.
PS_DEV bool tv_in_front(const double* __restrict__ R, const double* __restrict__ t, double sgn, double x1, double y1, double x2,
                        double y2, double* __restrict__ cosang)
{
#pragma clang fp contract(off)
    const double a0 = R[0] * x1 + R[1] * y1 + R[2], a1 = R[3] * x1 + R[4] * y1 + R[5], a2 = R[6] * x1 + R[7] * y1 + R[8];
    const double t0 = sgn * t[0], t1 = sgn * t[1], t2 = sgn * t[2];
    const double aa = a0 * a0 + a1 * a1 + a2 * a2, bb = x2 * x2 + y2 * y2 + 1.0, ab = a0 * x2 + a1 * y2 + a2;
    const double at = a0 * t0 + a1 * t1 + a2 * t2, bt = x2 * t0 + y2 * t1 + t2;
    const double det = aa * bb - ab * ab;
    const double lam = (ab * bt - bb * at) / det, mu = (aa * bt - ab * at) / det;
    *cosang = ab / sqrt(aa * bb);
    return det > 0.0 && lam > 0.0 && mu > 0.0;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------

// What a scoring pass needs beside the matrix: the normalised correspondences, 1 / fu^2, 1 / fv^2 and the threshold.
struct TvScore { const double4* __restrict__ xn; double ifu2, ifv2, thresh; };

PS_DEV TvScore tv_score(const double4* __restrict__ xn, const double* __restrict__ cam, double thresh) {
    return TvScore{xn, 1.0 / (cam[2] * cam[2]), 1.0 / (cam[3] * cam[3]), thresh};
}

// is correspondence i an inlier of E
PS_DEV bool tv_point_inlier(const TvScore& s, const double* __restrict__ E, int i) {
    const double4 p = s.xn[i];
    return tv_inlier(E, p.x, p.y, p.z, p.w, s.ifu2, s.ifv2, s.thresh);
}

__global__ __launch_bounds__(256) void k_tv_normalise(int num_pts, const double* __restrict__ obs_1, const double* __restrict__ obs_2,
                                                      const double* __restrict__ cam, double4* __restrict__ xn)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= num_pts) return;
    const double cu = cam[0], cv = cam[1], fu = cam[2], fv = cam[3];
    xn[i] = make_double4((obs_1[2 * (size_t)i] - cu) / fu, (obs_1[2 * (size_t)i + 1] - cv) / fv,
                         (obs_2[2 * (size_t)i] - cu) / fu, (obs_2[2 * (size_t)i + 1] - cv) / fv);
}

// One workgroup per hypothesis.  sample_idx == NULL: the matrices are given (ps_twoview_score).  masks may be NULL.
__global__ __launch_bounds__(256) void k_tv_hypotheses(
    int num_pts, const int32_t* __restrict__ sample_idx /* [H][8] */, const double4* __restrict__ xn, const double* __restrict__ cam,
    double thresh, double* __restrict__ E_all /* [H][9], input when sample_idx == NULL */, int32_t* __restrict__ counts /* [H] */,
    uint8_t* __restrict__ flags /* [H] or NULL */, uint8_t* __restrict__ masks /* [H][num_pts] or NULL */)
{
    __shared__ double sA[72], sx[9], sf[9], sE[9];
    __shared__ int scp[9], scount[4];
    const int h = blockIdx.x, t = threadIdx.x;
    if (sample_idx) {
        if (t < 8) {
            const double4 p = xn[sample_idx[(size_t)h * 8 + t]];
            const double a[3] = {p.x, p.y, 1.0}, b[3] = {p.z, p.w, 1.0};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) sA[9 * t + 3 * r + c] = b[r] * a[c];
        }
        __syncthreads();
        if (t == 0) {
            bool ok = true;
            for (int a = 0; a < 8; ++a)
                for (int b = a + 1; b < 8; ++b)
                    if (sample_idx[(size_t)h * 8 + a] == sample_idx[(size_t)h * 8 + b]) ok = false;
            double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (ok) ok = tv_null8x9(sA, scp, sx, sf);
            if (ok) {
                double F[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) F[k] = sf[k];
                ok = tv_project(F, E);
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) { sE[k] = E[k]; E_all[(size_t)h * 9 + k] = E[k]; }
            if (flags) flags[h] = ok ? 0 : 1;
        }
    } else if (t < 9) {
        sE[t] = E_all[(size_t)h * 9 + t];
    }
    __syncthreads();
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = sE[k];
    const TvScore score = tv_score(xn, cam, thresh);
    int cnt = 0;
    for (int i = t; i < num_pts; i += 256) {
        const bool in = tv_point_inlier(score, E, i);
        if (masks) masks[(size_t)h * num_pts + i] = in ? 1 : 0;
        cnt += in ? 1 : 0;
    }
    cnt = rc_block_sum(cnt, scount);
    if (t == 0) counts[h] = cnt;
}

// np.argmax(counts): the first hypothesis with the maximal count; its matrix, and its mask by one rescoring pass
__global__ __launch_bounds__(256) void k_tv_best(
    int H, int num_pts, const int32_t* __restrict__ counts, const double* __restrict__ E_all, const double4* __restrict__ xn,
    const double* __restrict__ cam, double thresh, int32_t* __restrict__ info /* [0] index, [1] count */, double* __restrict__ E_best,
    uint8_t* __restrict__ mask)
{
    __shared__ int32_t sc[256], si[256];
    const int t = threadIdx.x;
    const RcBest w = rc_first_max(H, counts, sc, si);
    const int hb = w.index;
    if (t == 0) { info[0] = hb; info[1] = w.count; }
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = E_all[(size_t)hb * 9 + k];
    if (t < 9) E_best[t] = E_all[(size_t)hb * 9 + t];
    const TvScore score = tv_score(xn, cam, thresh);
    for (int i = t; i < num_pts; i += 256) mask[i] = tv_point_inlier(score, E, i) ? 1 : 0;
}

// Hartley statistics of the inliers from the per-workgroup partials, every thread for itself, in slot order:
// hn = cx_1 cy_1 s_1 cx_2 cy_2 s_2 (s from partB only when with_scale); returns the inlier count
PS_DEV double tv_hartley(int G, const double* __restrict__ partA, const double* __restrict__ partB, bool with_scale,
                         double* __restrict__ hn)
{
#pragma clang fp contract(off)
    double s[5] = {0, 0, 0, 0, 0}, d[2] = {0, 0};
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] += partA[8 * (size_t)g + k];
        if (with_scale) { d[0] += partB[2 * (size_t)g]; d[1] += partB[2 * (size_t)g + 1]; }
    }
    const double n = s[4];
    hn[0] = s[0] / n; hn[1] = s[1] / n; hn[3] = s[2] / n; hn[4] = s[3] / n;
    hn[2] = with_scale ? 1.4142135623730951 / (d[0] / n) : 1.0;
    hn[5] = with_scale ? 1.4142135623730951 / (d[1] / n) : 1.0;
    return n;
}

// The three passes of the refit over the inliers, one point per thread, per-workgroup partials in slot order:
// stage 0: partA[g] = sum (x_1, y_1, x_2, y_2, 1);  1: partB[g] = sum of the distances to the centroids;
// stage 2: partC[g] = the 45 entries (p <= q, row-major) of sum a a^T, a = kron(x~_2, x~_1)
__global__ __launch_bounds__(256) void k_tv_refit_pass(
    int stage, int num_pts, const double4* __restrict__ xn, const uint8_t* __restrict__ mask, double* __restrict__ partA /* [G][8] */,
    double* __restrict__ partB /* [G][2] */, double* __restrict__ partC /* [G][45] */)
{
#pragma clang fp contract(off)
    __shared__ double s4[4];
    const int g = blockIdx.x, t = threadIdx.x, i = g * 256 + t, G = gridDim.x;
    const bool in = i < num_pts && mask[i] != 0;
    const double4 p = in ? xn[i] : make_double4(0.0, 0.0, 0.0, 0.0);
    if (stage == 0) {
        const double v[5] = {p.x, p.y, p.z, p.w, in ? 1.0 : 0.0};
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double s = rc_block_sum(v[k], s4);
            if (t == 0) partA[8 * (size_t)g + k] = s;
        }
        return;
    }
    double hn[6];
    tv_hartley(G, partA, partB, stage == 2, hn);
    const double dx1 = p.x - hn[0], dy1 = p.y - hn[1], dx2 = p.z - hn[3], dy2 = p.w - hn[4];
    if (stage == 1) {
        const double d1 = rc_block_sum(in ? sqrt(dx1 * dx1 + dy1 * dy1) : 0.0, s4);
        const double d2 = rc_block_sum(in ? sqrt(dx2 * dx2 + dy2 * dy2) : 0.0, s4);
        if (t == 0) { partB[2 * (size_t)g] = d1; partB[2 * (size_t)g + 1] = d2; }
        return;
    }
    const double x1[3] = {hn[2] * dx1, hn[2] * dy1, 1.0}, x2[3] = {hn[5] * dx2, hn[5] * dy2, 1.0};
    double a[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) a[3 * r + c] = in ? x2[r] * x1[c] : 0.0;
    int k = 0;
#pragma unroll
    for (int pp = 0; pp < 9; ++pp)
#pragma unroll
        for (int q = pp; q < 9; ++q) {
            const double s = rc_block_sum(a[pp] * a[q], s4);
            if (t == 0) partC[45 * (size_t)g + k] = s;
            ++k;
        }
}

// One workgroup: the refit's eigenvector, projection, rescoring and the keep-or-not decision; then the decomposition of the
// winner with the cheirality vote.  info: [0] best index [1] raw count (both from k_tv_best) [2] final count [3] refit kept
// [4..7] cheirality counts.  result: T_21 (16) | E (9) | pad | parallax (num_pts, 0 outside the inliers)
__global__ __launch_bounds__(256) void k_tv_finish(
    int num_pts, int G, int refit, const double4* __restrict__ xn, const double* __restrict__ cam, double thresh,
    const double* __restrict__ partA, const double* __restrict__ partB, const double* __restrict__ partC,
    const double* __restrict__ E_best, uint8_t* __restrict__ mask /* in: raw, out: final */, uint8_t* __restrict__ mask_refit,
    int32_t* __restrict__ info, double* __restrict__ result)
{
    __shared__ double sM[81], sQ[81], sf[9], sE[9], sRa[9], sRb[9], st[3];
    __shared__ int sok, s4[4];
    const int t = threadIdx.x;
    const TvScore score = tv_score(xn, cam, thresh);
    const int raw_count = info[1];
    int final_count = raw_count, kept = 0;
    if (t < 9) sE[t] = E_best[t];
    if (refit && raw_count >= 8) {                             // (uniform over the workgroup)
        if (t < 45) {
            double s = 0.0;
            for (int g = 0; g < G; ++g) s += partC[45 * (size_t)g + t];
            int p = 0, k = t;
            while (k >= 9 - p) { k -= 9 - p; ++p; }
            sM[9 * p + p + k] = s; sM[9 * (p + k) + p] = s;
        }
        __syncthreads();
        if (t == 0) {
            double hn[6], Fn[9], F[9], E[9];
            tv_hartley(G, partA, partB, true, hn);
            tv_eig9_smallest(sM, sQ, sf);
#pragma unroll
            for (int k = 0; k < 9; ++k) Fn[k] = sf[k];
            tv_denormalise(Fn, hn, F);
            bool ok = hn[2] > 0.0 && hn[2] < 1e300 && hn[5] > 0.0 && hn[5] < 1e300;
            if (ok) ok = tv_project(F, E);
            if (ok)
#pragma unroll
                for (int k = 0; k < 9; ++k) sf[k] = E[k];
            sok = ok ? 1 : 0;
        }
        __syncthreads();
        if (sok) {
            double E[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) E[k] = sf[k];
            int cnt = 0;
            for (int i = t; i < num_pts; i += 256) {
                const bool in = tv_point_inlier(score, E, i);
                mask_refit[i] = in ? 1 : 0;
                cnt += in ? 1 : 0;
            }
            cnt = rc_block_sum(cnt, s4);
            if (cnt >= raw_count) {
                kept = 1; final_count = cnt;
                for (int i = t; i < num_pts; i += 256) mask[i] = mask_refit[i];      // (this thread's own entries)
                __syncthreads();
                if (t < 9) sE[t] = sf[t];
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        double E[9], Ra[9], Rb[9], tt[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = sE[k];
        const bool ok = tv_decompose(E, Ra, Rb, tt);
#pragma unroll
        for (int k = 0; k < 9; ++k) { sRa[k] = ok ? Ra[k] : (k % 4 == 0 ? 1.0 : 0.0); sRb[k] = ok ? Rb[k] : (k % 4 == 0 ? 1.0 : 0.0); }
#pragma unroll
        for (int k = 0; k < 3; ++k) st[k] = ok ? tt[k] : 0.0;
        sok = ok ? 1 : 0;
    }
    __syncthreads();
    double Ra[9], Rb[9], tt[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) { Ra[k] = sRa[k]; Rb[k] = sRb[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) tt[k] = st[k];
    int c[4] = {0, 0, 0, 0};
    if (sok)
        for (int i = t; i < num_pts; i += 256) {
            if (!mask[i]) continue;
            const double4 p = xn[i];
            double cs;
            c[0] += tv_in_front(Ra, tt, 1.0, p.x, p.y, p.z, p.w, &cs) ? 1 : 0;
            c[1] += tv_in_front(Ra, tt, -1.0, p.x, p.y, p.z, p.w, &cs) ? 1 : 0;
            c[2] += tv_in_front(Rb, tt, 1.0, p.x, p.y, p.z, p.w, &cs) ? 1 : 0;
            c[3] += tv_in_front(Rb, tt, -1.0, p.x, p.y, p.z, p.w, &cs) ? 1 : 0;
        }
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = rc_block_sum(c[k], s4);
    int win = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) if (c[k] > c[win]) win = k;
    const bool useb = win >= 2;
    const double sgn = (win & 1) ? -1.0 : 1.0;
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = useb ? Rb[k] : Ra[k];
    for (int i = t; i < num_pts; i += 256) {
        double deg = 0.0;
        if (sok && mask[i]) {
            const double4 p = xn[i];
            double cs;
            tv_in_front(R, tt, sgn, p.x, p.y, p.z, p.w, &cs);
            deg = acos(fmin(1.0, fmax(-1.0, cs))) * (180.0 / 3.14159265358979323846);
        }
        result[26 + i] = deg;
    }
    if (t == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) result[4 * r + cc] = R[3 * r + cc];
            result[4 * r + 3] = sgn * tt[r];
        }
        result[12] = 0.0; result[13] = 0.0; result[14] = 0.0; result[15] = 1.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) result[16 + k] = sE[k];
        result[25] = 0.0;
        info[2] = final_count; info[3] = kept;
#pragma unroll
        for (int k = 0; k < 4; ++k) info[4 + k] = c[k];
    }
}
