// ps_k_pnp.h -- absolute-pose (PnP) RANSAC on the device: registration of a monocular frame against the map (gfx950, fp64).
// Part of ps_core.hip (one translation unit; included after ps_k_twoview.h).  pyslam_amd/pipelines/absolute.py is the same
// definition in numpy / plain floats; this project has no reference counterpart for it (as for MonoCamera and the two-view front end).
//
// Input: N landmarks pts_w (map frame), their pixels obs, a pinhole camera (cu, cv, fu, fv), H minimal sets of 3 point indices.
//   bearings: x = (u - cu) / fu, y = (v - cv) / fv, n = sqrt(x x + y y + 1), f = (x, y, 1) / n   (k_pnp_normalise, once per call)
//   sample (P_1 P_2 P_3, f_1 f_2 f_3): P3P after Grunert, in the notation of Haralick et al. 1994:
//     a^2 = |P_2 - P_3|^2, b^2 = |P_1 - P_3|^2, c^2 = |P_1 - P_2|^2, cos alpha = f_2.f_3, cos beta = f_1.f_3, cos gamma = f_1.f_2,
//     depths s_1, s_2 = u s_1, s_3 = v s_1; v is a root of the quartic A_4 v^4 + ... + A_0 (pnp_quartic).
//     Roots by Ferrari: monic, depressed with x = y - B / 4 (y^4 + p y^2 + q y + r); the LARGEST real root m of the resolvent cubic
//     m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8 by Cardano (one real root) or the trigonometric form (three), two Newton steps on that
//     cubic; s = sqrt(2 m); the quadratics y^2 + s y + (p / 2 + m - q / (2 s)) and y^2 - s y + (p / 2 + m + q / (2 s)).
//     SLOT ORDER: 0: (-s + sqrt D_1) / 2   1: (-s - sqrt D_1) / 2   2: (s + sqrt D_2) / 2   3: (s - sqrt D_2) / 2, each minus B / 4 and
//     polished by three Newton steps on the ORIGINAL quartic.
//     u = ((r_1 - 1) v^2 - 2 r_1 cos beta v + 1 + r_1) / (2 (cos gamma - v cos alpha)), r_1 = (a^2 - c^2) / b^2;
//     s_1^2 = b^2 / (1 + v^2 - 2 v cos beta);  Q_i = s_i f_i;  pose = rigid alignment of (P_i) onto (Q_i) by ransac_align's scheme
//     (ps_ransac.h), for exactly three points and strictly evaluated (pnp_align3).
//   A slot is EMPTY (T = 0, count 0, flag bit 0) when its root is not real (D < 0 or m not positive), not positive or not finite,
//     when u <= 0, when s_1^2 is not positive, or when a denominator is zero (A_4, s, a Newton derivative, the denominators of u and
//     s_1^2, a vanishing second singular value).  Nothing is NaN.
//   A sample is DEGENERATE (all four slots empty, flag bits 0 and 1) with a repeated index, a squared side not above 1e-24 of the
//     longest squared side, a triangle area not above 1e-12 of the longest side squared, or a non-finite input row.
//   score of a slot: p = R X + t, d = (fu p_1 / p_3 + cu - u)^2 + (fv p_2 / p_3 + cv - v)^2, left to right, no contraction;
//     inlier: p_3 > 0 and d < thresh (NaN compares false).  A hypothesis' count is its largest slot count, the first such slot wins.
//   best: the FIRST hypothesis with the maximal count (np.argmax over the H x 4 counts in row-major order); mask by one rescoring pass.
//   refinement: Gauss-Newton on xi = (rho, phi), T <- exp(xi) T, over the RAW winner's inliers throughout, unit weights, L2:
//     cost = 1/2 sum |r|^2, H = sum J^T J (21), g = sum J^T r (6), H xi = -g by Cholesky; a pivot not above 1e-12 of its diagonal entry
//     FAILS and ends the iterations.  Kept when no pivot failed, the refined count is not lower than the raw count and the pose is finite.
//
// No atomics; every sum is reduced in a fixed order (thread-private in stride order, xor tree inside a wave, then waves 0..3), so two
// calls on the same input are bit-identical.  The four roots and poses live in LDS; the small solves use fully unrolled private
// arrays (static indices only) or LDS.
#pragma once
#include "ps_ransac_core.h"

// ---- scalar building blocks ----------------------------------------------------------------------------------------------------

PS_DEV double pnp_dot(const double* __restrict__ a, const double* __restrict__ b) {
#pragma clang fp contract(off)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

PS_DEV double pnp_dist2(const double* __restrict__ a, const double* __restrict__ b) {
#pragma clang fp contract(off)
    const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    return d0 * d0 + d1 * d1 + d2 * d2;
}

// the side and area rules of the world triangle P (3 x 3, finite)
PS_DEV bool pnp_triangle_ok(const double* __restrict__ P) {
#pragma clang fp contract(off)
    const double a2 = pnp_dist2(P + 3, P + 6), b2 = pnp_dist2(P, P + 6), c2 = pnp_dist2(P, P + 3);
    const double longest = fmax(a2, fmax(b2, c2)), shortest = fmin(a2, fmin(b2, c2));
    const double e[3] = {P[3] - P[0], P[4] - P[1], P[5] - P[2]}, g[3] = {P[6] - P[0], P[7] - P[1], P[8] - P[2]};
    const double cr[3] = {e[1] * g[2] - e[2] * g[1], e[2] * g[0] - e[0] * g[2], e[0] * g[1] - e[1] * g[0]};
    const double area = 0.5 * sqrt(pnp_dot(cr, cr));
    return longest > 0.0 && shortest > (1e-12 * 1e-12) * longest && area > 1e-12 * longest;
}

// Grunert's quartic: A (5: A_4 .. A_0), cs (3: cos alpha, beta, gamma), r_1, b^2
PS_DEV void pnp_quartic(const double* __restrict__ P, const double* __restrict__ f, double* __restrict__ A, double* __restrict__ cs,
                        double* __restrict__ r1_out, double* __restrict__ b2_out)
{
#pragma clang fp contract(off)
    const double a2 = pnp_dist2(P + 3, P + 6), b2 = pnp_dist2(P, P + 6), c2 = pnp_dist2(P, P + 3);
    const double ca = pnp_dot(f + 3, f + 6), cb = pnp_dot(f, f + 6), cg = pnp_dot(f, f + 3);
    const double r1 = (a2 - c2) / b2, r2 = (a2 + c2) / b2, r3 = (b2 - c2) / b2, r4 = (b2 - a2) / b2, ra = a2 / b2, rc = c2 / b2;
    A[0] = (r1 - 1.0) * (r1 - 1.0) - 4.0 * rc * ca * ca;
    A[1] = 4.0 * (r1 * (1.0 - r1) * cb - (1.0 - r2) * ca * cg + 2.0 * rc * ca * ca * cb);
    A[2] = 2.0 * (r1 * r1 - 1.0 + 2.0 * r1 * r1 * cb * cb + 2.0 * r3 * ca * ca - 4.0 * r2 * ca * cb * cg + 2.0 * r4 * cg * cg);
    A[3] = 4.0 * (-r1 * (1.0 + r1) * cb + 2.0 * ra * cg * cg * cb - (1.0 - r2) * ca * cg);
    A[4] = (1.0 + r1) * (1.0 + r1) - 4.0 * ra * cg * cg;
    cs[0] = ca; cs[1] = cb; cs[2] = cg;
    *r1_out = r1; *b2_out = b2;
}

PS_DEV bool pnp_finite(double x) { return fabs(x) < 1.7976931348623157e308; }       // false for NaN and inf

// The four slots' roots of A_4 x^4 + ... + A_0 in slot order (root, ok may address LDS).
PS_DEV void pnp_quartic_roots(const double* __restrict__ A, double* __restrict__ root /* 4 */, int* __restrict__ ok /* 4 */) {
#pragma clang fp contract(off)
    const double A4 = A[0], A3 = A[1], A2 = A[2], A1 = A[3], A0 = A[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { root[k] = 0.0; ok[k] = 0; }
    if (!(A4 != 0.0) || !pnp_finite(A4) || !pnp_finite(A3) || !pnp_finite(A2) || !pnp_finite(A1) || !pnp_finite(A0)) return;
    const double B = A3 / A4, C = A2 / A4, D = A1 / A4, E = A0 / A4;
    if (!pnp_finite(B) || !pnp_finite(C) || !pnp_finite(D) || !pnp_finite(E)) return;
    const double B2 = B * B;
    const double p = C - 0.375 * B2;
    const double q = D - 0.5 * B * C + 0.125 * B2 * B;
    const double r = E - 0.25 * B * D + 0.0625 * B2 * C - 0.01171875 * B2 * B2;
    const double c1 = 0.25 * p * p - r, c0 = -0.125 * q * q;
    const double Pc = c1 - p * p / 3.0;
    const double Qc = 2.0 * p * p * p / 27.0 - p * c1 / 3.0 + c0;
    const double hq = 0.5 * Qc, tp = Pc / 3.0;
    const double disc = hq * hq + tp * tp * tp;
    double z;
    if (disc > 0.0) {
        const double sd = sqrt(disc);
        z = cbrt(-hq + sd) + cbrt(-hq - sd);
    } else if (tp < 0.0) {
        const double amp = sqrt(-tp);
        const double arg = -hq / (amp * amp * amp);
        z = 2.0 * amp * cos(acos(fmin(1.0, fmax(-1.0, arg))) / 3.0);
    } else {
        z = 0.0;
    }
    double m = z - p / 3.0;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double fm = ((m + p) * m + c1) * m + c0;
        const double dm = (3.0 * m + 2.0 * p) * m + c1;
        if (dm != 0.0) m = m - fm / dm;
    }
    if (!(m > 0.0) || !pnp_finite(m)) return;
    const double s = sqrt(2.0 * m);
    const double hs = q / (2.0 * s);
    const double g1 = 0.5 * p + m - hs, g2 = 0.5 * p + m + hs;
    const double shift = 0.25 * B;
#pragma unroll
    for (int quad = 0; quad < 2; ++quad) {
        const double sgn = quad == 0 ? -1.0 : 1.0, g = quad == 0 ? g1 : g2;
        const double Dq = s * s - 4.0 * g;
        if (!(Dq >= 0.0)) continue;
        const double sq = sqrt(Dq);
#pragma unroll
        for (int pm = 0; pm < 2; ++pm) {
            const double y = pm == 0 ? 0.5 * (sgn * s + sq) : 0.5 * (sgn * s - sq);
            double x = y - shift;
            bool good = true;
#pragma unroll
            for (int it = 0; it < 3; ++it) {
                if (good) {
                    const double fx = (((A4 * x + A3) * x + A2) * x + A1) * x + A0;
                    const double dx = ((4.0 * A4 * x + 3.0 * A3) * x + 2.0 * A2) * x + A1;
                    if (!(dx != 0.0)) good = false;
                    else x = x - fx / dx;
                }
            }
            good = good && pnp_finite(x) && x > 0.0;
            root[2 * quad + pm] = good ? x : 0.0;
            ok[2 * quad + pm] = good ? 1 : 0;
        }
    }
}

// [R | t] (12, row-major 3 x 4) of the alignment Q_i ~ R P_i + t of three points.  false: the second singular value vanishes.
// The scheme is ransac_align's, but the Jacobi sweeps are written out here and not taken from rc_jacobi3 (ps_ransac_core.h):
// this function is evaluated strictly (`fp contract(off)`, which is lexical), rc_jacobi3 under the default contraction, and the
// contraction mode is part of the poses' bits.  Only the sort, which moves data and computes nothing, is shared.
PS_DEV bool pnp_align3(const double* __restrict__ P /* 9 */, const double* __restrict__ Q /* 9 */, double* __restrict__ T) {
#pragma clang fp contract(off)
    const double third = 1.0 / 3.0;
    double c1[3], c2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { c1[a] = (P[a] + P[3 + a] + P[6 + a]) * third; c2[a] = (Q[a] + Q[3 + a] + Q[6 + a]) * third; }
    double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};       // A[col][row], V[col][row]
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int col = 0; col < 3; ++col) {
            const double qd = P[3 * k + col] - c1[col];
#pragma unroll
            for (int row = 0; row < 3; ++row) A[col][row] += (Q[3 * k + row] - c2[row]) * qd;
        }
#pragma unroll
    for (int col = 0; col < 3; ++col)
#pragma unroll
        for (int row = 0; row < 3; ++row) A[col][row] *= third;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double al = A[p][0] * A[p][0] + A[p][1] * A[p][1] + A[p][2] * A[p][2];
            const double be = A[q][0] * A[q][0] + A[q][1] * A[q][1] + A[q][2] * A[q][2];
            const double ga = A[p][0] * A[q][0] + A[p][1] * A[q][1] + A[p][2] * A[q][2];
            if (ga == 0.0 || !(fabs(ga) > 1.2e-16 * sqrt(al * be))) continue;
            rotated = true;
            const double zeta = (be - al) / (2.0 * ga);
            const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double ap = A[p][r], aq = A[q][r], vp = V[p][r], vq = V[q][r];
                A[p][r] = c * ap - s * aq; A[q][r] = s * ap + c * aq;
                V[p][r] = c * vp - s * vq; V[q][r] = s * vp + c * vq;
            }
        }
        if (!rotated) break;
    }
    double sg[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) sg[k] = sqrt(A[k][0] * A[k][0] + A[k][1] * A[k][1] + A[k][2] * A[k][2]);
    rc_sort3(sg, A, V);
    if (!(sg[0] > 0.0) || !(sg[1] > 1e-15 * sg[0]) || !(sg[0] < 1e300)) return false;
    double u1[3], u2[3], v1[3], v2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { u1[r] = A[0][r] / sg[0]; u2[r] = A[1][r] / sg[1]; v1[r] = V[0][r]; v2[r] = V[1][r]; }
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double tr = c2[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double cv = u1[r] * v1[c] + u2[r] * v2[c] + u3[r] * v3[c];
            T[4 * r + c] = cv;
            tr -= cv * c1[c];
        }
        T[4 * r + 3] = tr;
    }
    return true;
}

// One root v -> one pose.  false: the slot is empty.
PS_DEV bool pnp_pose_of_root(double v, const double* __restrict__ P, const double* __restrict__ f, const double* __restrict__ cs,
                             double r1, double b2, double* __restrict__ T /* 12 */)
{
#pragma clang fp contract(off)
    const double ca = cs[0], cb = cs[1], cg = cs[2];
    const double den = 2.0 * (cg - v * ca);
    if (!(den != 0.0)) return false;
    const double t0 = (r1 - 1.0) * v * v, t1 = 2.0 * r1 * cb * v;
    const double num = t0 - t1 + 1.0 + r1;
    const double u = num / den;
    const double den1 = 1.0 + v * v - 2.0 * v * cb;
    if (!(u > 0.0) || !pnp_finite(u) || !(den1 > 0.0)) return false;
    const double s1sq = b2 / den1;
    if (!(s1sq > 0.0) || !pnp_finite(s1sq)) return false;
    const double s1 = sqrt(s1sq);
    const double s2 = u * s1, s3 = v * s1;
    double Q[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) { Q[k] = s1 * f[k]; Q[3 + k] = s2 * f[3 + k]; Q[6 + k] = s3 * f[6 + k]; }
    if (!pnp_align3(P, Q, T)) return false;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) fin = fin && pnp_finite(T[k]);
    return fin;
}

// squared reprojection error of one point (absolute.reprojection's operations in the same order); *front: p_3 > 0
PS_DEV double pnp_sq_err(const double* __restrict__ T /* 12 */, double X, double Y, double Z, double ou, double ov, double cu, double cv,
                         double fu, double fv, bool* __restrict__ front)
{
#pragma clang fp contract(off)
    const double p1 = T[0] * X + T[1] * Y + T[2] * Z + T[3];
    const double p2 = T[4] * X + T[5] * Y + T[6] * Z + T[7];
    const double p3 = T[8] * X + T[9] * Y + T[10] * Z + T[11];
    const double du = fu * p1 / p3 + cu - ou, dv = fv * p2 / p3 + cv - ov;
    *front = p3 > 0.0;
    return du * du + dv * dv;
}

// What a scoring pass needs beside the pose: the landmarks, their pixels, the camera and the threshold.
struct PnpScore { const double* __restrict__ pts_w; const double* __restrict__ obs; double cu, cv, fu, fv, thresh; };

PS_DEV PnpScore pnp_score(const double* __restrict__ pts_w, const double* __restrict__ obs, const double* __restrict__ cam, double thresh) {
    return PnpScore{pts_w, obs, cam[0], cam[1], cam[2], cam[3], thresh};
}

// is point i an inlier of the pose T; *d: its squared reprojection error
PS_DEV bool pnp_point_inlier(const PnpScore& s, const double* __restrict__ T /* 12 */, int i, double* __restrict__ d) {
    bool front;
    *d = pnp_sq_err(T, s.pts_w[3 * (size_t)i], s.pts_w[3 * (size_t)i + 1], s.pts_w[3 * (size_t)i + 2], s.obs[2 * (size_t)i],
                    s.obs[2 * (size_t)i + 1], s.cu, s.cv, s.fu, s.fv, &front);
    return front && *d < s.thresh;
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_pnp_normalise(int num_pts, const double* __restrict__ obs, const double* __restrict__ cam,
                                                       double* __restrict__ bear /* [N][3] */)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= num_pts) return;
    const double x = (obs[2 * (size_t)i] - cam[0]) / cam[2], y = (obs[2 * (size_t)i + 1] - cam[1]) / cam[3];
    const double n = sqrt(x * x + y * y + 1.0);
    bear[3 * (size_t)i] = x / n; bear[3 * (size_t)i + 1] = y / n; bear[3 * (size_t)i + 2] = 1.0 / n;
}

// One workgroup per sample: T_all [H][4][16], counts [H][4], flags [H][4] (bit 0: empty slot, bit 1: degenerate sample).
// sample_idx == NULL: one workgroup per GIVEN pose (ps_pnp_score): T_all [H][16] is input, counts [H], masks [H][num_pts].
__global__ __launch_bounds__(256) void k_pnp_hypotheses(
    int num_pts, const int32_t* __restrict__ sample_idx /* [H][3] or NULL */, const double* __restrict__ pts_w,
    const double* __restrict__ obs, const double* __restrict__ bear, const double* __restrict__ cam, double thresh,
    double* __restrict__ T_all, int32_t* __restrict__ counts, uint8_t* __restrict__ flags, uint8_t* __restrict__ masks)
{
    __shared__ double sT[4][12], sroot[4], scs[3], sr1b2[2];
    __shared__ int sok[4], sdeg, scount[4 * 4];
    const int h = blockIdx.x, t = threadIdx.x;
    const bool solve = sample_idx != nullptr;
    if (solve) {
        int id[3] = {0, 0, 0};
        double P[9], f[9];
        if (t < 4) {                                             // (lanes 0..3 of wave 0: each needs the sample for its own slot)
#pragma unroll
            for (int k = 0; k < 3; ++k) id[k] = sample_idx[(size_t)h * 3 + k];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int a = 0; a < 3; ++a) { P[3 * k + a] = pts_w[3 * (size_t)id[k] + a]; f[3 * k + a] = bear[3 * (size_t)id[k] + a]; }
        }
        if (t == 0) {
            bool ok = id[0] != id[1] && id[0] != id[2] && id[1] != id[2];
#pragma unroll
            for (int k = 0; k < 9; ++k) ok = ok && pnp_finite(P[k]) && pnp_finite(f[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) ok = ok && pnp_finite(obs[2 * (size_t)id[k]]) && pnp_finite(obs[2 * (size_t)id[k] + 1]);
            if (ok) ok = pnp_triangle_ok(P);
            sdeg = ok ? 0 : 1;
            if (ok) {
                double A[5], cs[3], r1, b2;
                pnp_quartic(P, f, A, cs, &r1, &b2);
                pnp_quartic_roots(A, sroot, sok);
                scs[0] = cs[0]; scs[1] = cs[1]; scs[2] = cs[2]; sr1b2[0] = r1; sr1b2[1] = b2;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) { sroot[k] = 0.0; sok[k] = 0; }
            }
        }
        __syncthreads();
        if (t < 4) {
            double T[12];
            bool ok = sok[t] != 0;
            if (ok) {
                const double cs[3] = {scs[0], scs[1], scs[2]};
                ok = pnp_pose_of_root(sroot[t], P, f, cs, sr1b2[0], sr1b2[1], T);
            }
            double* out = T_all + ((size_t)h * 4 + t) * 16;
#pragma unroll
            for (int k = 0; k < 12; ++k) { const double v = ok ? T[k] : 0.0; sT[t][k] = v; out[k] = v; }
            out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = ok ? 1.0 : 0.0;
            sok[t] = ok ? 1 : 0;
            if (flags) flags[(size_t)h * 4 + t] = (uint8_t)((ok ? 0 : 1) | (sdeg ? 2 : 0));
        }
    } else {
        if (t < 12) sT[0][t] = T_all[(size_t)h * 16 + t];
        if (t < 4) sok[t] = t == 0 ? 1 : 0;
    }
    __syncthreads();
    const PnpScore score = pnp_score(pts_w, obs, cam, thresh);
    int cnt[4] = {0, 0, 0, 0};
    for (int i = t; i < num_pts; i += 256) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double d;
            const bool in = sok[k] /* (uniform over the workgroup) */ && pnp_point_inlier(score, sT[k], i, &d);
            cnt[k] += in ? 1 : 0;
            if (masks && k == 0) masks[(size_t)h * num_pts + i] = in ? 1 : 0;
        }
    }
    rc_block_partials(cnt, scount);
    if (solve) {
        if (t < 4) counts[(size_t)h * 4 + t] = rc_block_total(scount, 4, t);
    } else if (t == 0) {
        counts[h] = rc_block_total(scount, 4, 0);
    }
}

// np.argmax over the row-major H x 4 counts: the first hypothesis with the maximal count and its first such slot; the pose, and
// its mask by one rescoring pass.  info: [0] hypothesis [1] slot [2] raw count
__global__ __launch_bounds__(256) void k_pnp_best(
    int num_slots /* 4 H */, int num_pts, const int32_t* __restrict__ counts, const double* __restrict__ T_all,
    const double* __restrict__ pts_w, const double* __restrict__ obs, const double* __restrict__ cam, double thresh,
    int32_t* __restrict__ info, double* __restrict__ T_best /* 16 */, uint8_t* __restrict__ mask)
{
    __shared__ int32_t sc[256], si[256];
    __shared__ double sT[12];
    const int t = threadIdx.x;
    const RcBest w = rc_first_max(num_slots, counts, sc, si);
    const int hb = w.index;                                      // the flat slot: 4 * hypothesis + slot
    if (t < 16) {
        const double v = T_all[(size_t)hb * 16 + t];
        T_best[t] = v;
        if (t < 12) sT[t] = v;
    }
    __syncthreads();
    const PnpScore score = pnp_score(pts_w, obs, cam, thresh);
    double d;
    for (int i = t; i < num_pts; i += 256) mask[i] = pnp_point_inlier(score, sT, i, &d) ? 1 : 0;
    if (t == 0) { info[0] = hb >> 2; info[1] = hb & 3; info[2] = w.count; }
}

#define PNP_SUMS 28        // 21 entries of H (upper triangle, row-major) | 6 of g | sum |r|^2

// One workgroup: every Gauss-Newton iteration, the keep rule, the final mask, counts and squared errors.
// info: [0..2] from k_pnp_best; out [3] final count [4] refinement kept [5] a pivot failed [6] iterations run [7] 0.
// result: T_cw (16) | cost_history (iters + 1) | sq_err (num_pts)
__global__ __launch_bounds__(256) void k_pnp_refine(
    int num_pts, int iters, const double* __restrict__ pts_w, const double* __restrict__ obs, const double* __restrict__ cam, double thresh,
    const double* __restrict__ T_best, uint8_t* __restrict__ mask /* in: raw, out: final */, int32_t* __restrict__ info,
    double* __restrict__ result)
{
    __shared__ double sT[12], sred[4 * PNP_SUMS], sH[36], sL[36], sg[6];
    __shared__ int sfail, s4[4];
    const int t = threadIdx.x;
    const PnpScore score = pnp_score(pts_w, obs, cam, thresh);
    const double cu = score.cu, cv = score.cv, fu = score.fu, fv = score.fv;
    const int raw_count = info[2];
    double* hist = result + 16;
    double* sq_err = result + 16 + iters + 1;
    if (t < 12) sT[t] = T_best[t];
    if (t == 0) sfail = 0;
    __syncthreads();
    int ran = 0;
    for (int it = 0; it < iters; ++it) {
        double acc[PNP_SUMS];
#pragma unroll
        for (int k = 0; k < PNP_SUMS; ++k) acc[k] = 0.0;
        for (int i = t; i < num_pts; i += 256) {
            if (!mask[i]) continue;
            const double X = pts_w[3 * (size_t)i], Y = pts_w[3 * (size_t)i + 1], Z = pts_w[3 * (size_t)i + 2];
            const double x = sT[0] * X + sT[1] * Y + sT[2] * Z + sT[3];
            const double y = sT[4] * X + sT[5] * Y + sT[6] * Z + sT[7];
            const double z = sT[8] * X + sT[9] * Y + sT[10] * Z + sT[11];
            const double iz = 1.0 / z;
            const double ru = fu * x / z + cu - obs[2 * (size_t)i], rv = fv * y / z + cv - obs[2 * (size_t)i + 1];
            const double a = fu * iz, b = -fu * x * iz * iz, c = fv * iz, e = -fv * y * iz * iz;
            const double Ju[6] = {a, 0.0, b, b * y, a * z - b * x, -a * y};
            const double Jv[6] = {0.0, c, e, -c * z + e * y, -e * x, c * x};
            int k = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int q = r; q < 6; ++q) { acc[k] += Ju[r] * Ju[q] + Jv[r] * Jv[q]; ++k; }
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[21 + r] += Ju[r] * ru + Jv[r] * rv;
            acc[27] += ru * ru + rv * rv;
        }
        rc_block_partials(acc, sred);
        if (t < PNP_SUMS) {
            const double s = rc_block_total(sred, PNP_SUMS, t);
            if (t < 21) {
                int r = 0, k = t;
                while (k >= 6 - r) { k -= 6 - r; ++r; }
                sH[6 * r + r + k] = s; sH[6 * (r + k) + r] = s;
            } else if (t < 27) {
                sg[t - 21] = s;
            } else {
                hist[it] = 0.5 * s;
            }
        }
        __syncthreads();
        if (t == 0) {
            bool ok = true;
            for (int j = 0; j < 6 && ok; ++j) {
                double d = sH[7 * j];
                for (int k = 0; k < j; ++k) d -= sL[6 * j + k] * sL[6 * j + k];
                if (!(d > 1e-12 * sH[7 * j]) || !pnp_finite(d)) { ok = false; break; }
                const double l = sqrt(d);
                sL[7 * j] = l;
                for (int i = j + 1; i < 6; ++i) {
                    double v = sH[6 * i + j];
                    for (int k = 0; k < j; ++k) v -= sL[6 * i + k] * sL[6 * j + k];
                    sL[6 * i + j] = v / l;
                }
            }
            if (ok) {
                for (int i = 0; i < 6; ++i) {                    // L y = -g (y over g), then L^T xi = y
                    double v = -sg[i];
                    for (int k = 0; k < i; ++k) v -= sL[6 * i + k] * sg[k];
                    sg[i] = v / sL[7 * i];
                }
                for (int i = 5; i >= 0; --i) {
                    double v = sg[i];
                    for (int k = i + 1; k < 6; ++k) v -= sL[6 * k + i] * sg[k];
                    sg[i] = v / sL[7 * i];
                }
                double xi[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) xi[k] = sg[k];
                Se3 Tc;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) Tc.R[3 * r + c] = sT[4 * r + c];
                    Tc.t[r] = sT[4 * r + 3];
                }
                const Se3 Tn = se3_mul(se3_exp(xi), Tc);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) sT[4 * r + c] = Tn.R[3 * r + c];
                    sT[4 * r + 3] = Tn.t[r];
                }
            } else {
                sfail = 1;
                for (int k = it + 1; k <= iters; ++k) hist[k] = hist[it];
            }
        }
        __syncthreads();
        if (sfail) break;                                        // (uniform)
        ++ran;
    }
    // the refined pose over all points: its count, and its cost over the raw inliers
    const bool failed = sfail != 0;
    int cnt = 0;
    double cost = 0.0;
    for (int i = t; i < num_pts; i += 256) {
        double d;
        cnt += pnp_point_inlier(score, sT, i, &d) ? 1 : 0;
        if (mask[i]) cost += d;
    }
    cnt = rc_block_sum(cnt, s4);
    cost = rc_block_sum(cost, sred);
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) fin = fin && pnp_finite(sT[k]);
    const bool kept = iters > 0 && !failed && fin && cnt >= raw_count;
    __syncthreads();
    if (t == 0 && !failed) hist[iters] = 0.5 * cost;
    if (!kept && t < 12) sT[t] = T_best[t];
    __syncthreads();
    int fcnt = 0;
    for (int i = t; i < num_pts; i += 256) {
        double d;
        const bool in = pnp_point_inlier(score, sT, i, &d);
        sq_err[i] = d;
        mask[i] = in ? 1 : 0;
        fcnt += in ? 1 : 0;
    }
    fcnt = rc_block_sum(fcnt, s4);
    if (t < 12) result[t] = sT[t];
    if (t == 0) {
        result[12] = 0.0; result[13] = 0.0; result[14] = 0.0; result[15] = T_best[15];
        info[3] = fcnt; info[4] = kept ? 1 : 0; info[5] = failed ? 1 : 0; info[6] = ran; info[7] = 0;
    }
}
