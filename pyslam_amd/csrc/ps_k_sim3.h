// ps_k_sim3.h -- similarity (Sim(3)) alignment RANSAC on the device: two matched 3-D point sets of monocular maps, whose scales
// are unrelated (gfx950, fp64).  Part of ps_core.hip (one translation unit; included after ps_k_pnp.h).
// pyslam_amd/pipelines/similarity.py is the same definition in numpy; the reference has no counterpart (it has no monocular map).
//
// Model: p_2 = s R p_1 + t, s > 0, stored as the row-major 4 x 4 S = [s R | t; 0 0 0 1] and the scalar s.
//   fit of n >= 3 pairs (Umeyama 1991): centroids c_1, c_2, q = p - c, W = sum q_2 q_1^T, v = sum |q_1|^2 (two passes: the centroids,
//     then the ten sums about them); SVD of W by rc_jacobi3 (a non-finite column pair is skipped), sigma_a >= sigma_b >= sigma_c;
//     R = u_a v_a^T + u_b v_b^T + (u_a x u_b)(v_a x v_b)^T (ransac_align's completion: a proper rotation whatever the third pair is);
//     d = sign((u_a x u_b) . u_c) sign((v_a x v_b) . v_c), 0 when sigma_c = 0;  s = (sigma_a + sigma_b + d sigma_c) / v, or 1 with
//     fixed_scale;  t = c_2 - s R c_1.
//   A fit is DEGENERATE (flag 1, S = 0 with S[15] = 0, s = 0, count 0) with fewer than 3 pairs, when v is not positive or not finite,
//     when sigma_b is not above 1e-6 sigma_a (collinear or repeated points; a NaN anywhere in W lands here), when s is not positive
//     or not finite, or when an entry of S is not finite.
//   score, from the stored S alone (M = s R its 3 x 3 block): a = M p_1 + t;  s^2 = |M|_F^2 / 3, B = M^T / s^2, b = B p_2 - B t
//     (= R^T (p_2 - t) / s).  Pixel mode (a camera, obs_1, obs_2): e = max(|pi(a) - obs_2|^2, |pi(b) - obs_1|^2), NaN if either is;
//     inlier: e < thresh, a_3 > 0 and b_3 > 0.  Metric mode: e = |a - p_2|^2; inlier: e < thresh.  A NaN compares false.
//   best: the FIRST hypothesis with the maximal count (rc_first_max); its mask by one rescoring pass, at the head of the refit kernel
//     (the same function on the same model: the same bits, without H x N bytes of masks in the call's block).
//   refit: from the winner's model and mask up to `iters` rounds, each a fit of all current inliers and a rescoring of every point
//     (the rescoring pass also takes the centroid sums of its own mask, which the next round's fit starts from: two passes a round).
//     A degenerate round (reason 3) or a round with fewer inliers than the current count (1) ends the loop and is discarded;
//     otherwise the round is adopted, and the loop ends after it when its mask equals the previous one (2).  0: all rounds ran.
//
// No atomics; every sum is thread-private in stride order, then the xor tree inside a wave, then waves 0..3 (rc_block_partials), so two
// calls on the same input are bit-identical.  The mode is a template parameter of the two kernels that score.
#pragma once
#include "ps_ransac_core.h"

#define SIM3_RATIO 1e-6

PS_DEV bool sim3_finite(double x) { return fabs(x) < 1.7976931348623157e308; }       // false for NaN and inf

PS_DEV double sim3_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

// The fit over accumulated sums, shared by the minimal and the refit case.  n pairs, their centroids c_1, c_2, W (9, row-major:
// sum q_2 q_1^T) and v -> S (12: the rows of [s R | t]) and *scale.  false: degenerate (S and *scale are not written).
PS_DEV bool sim3_fit(int n, const double (&c1)[3], const double (&c2)[3], const double (&W)[9], double v, bool fixed_scale,
                     double* __restrict__ S, double* __restrict__ scale)
{
    if (n < 3 || !(v > 0.0) || !sim3_finite(v)) return false;
    double A[3][3], V[3][3], sg[3];                              // A[col][row]: the columns of W
#pragma unroll
    for (int col = 0; col < 3; ++col)
#pragma unroll
        for (int row = 0; row < 3; ++row) A[col][row] = W[3 * row + col];
    rc_jacobi3<false>(A, V, sg);
    rc_sort3(sg, A, V);
    if (!(sg[1] > SIM3_RATIO * sg[0])) return false;
    double u1[3], u2[3], v1[3], v2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { u1[r] = A[0][r] / sg[0]; u2[r] = A[1][r] / sg[1]; v1[r] = V[0][r]; v2[r] = V[1][r]; }
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    double s = 1.0;
    if (!fixed_scale) {
        double d = 0.0;
        if (sg[2] > 0.0)                                         // (A[2] = sigma_c u_c: the same sign)
            d = sim3_sign(u3[0] * A[2][0] + u3[1] * A[2][1] + u3[2] * A[2][2]) * sim3_sign(v3[0] * V[2][0] + v3[1] * V[2][1] + v3[2] * V[2][2]);
        s = (sg[0] + sg[1] + d * sg[2]) / v;
        if (!(s > 0.0) || !sim3_finite(s)) return false;
    }
    double out[12];
    bool fin = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double tr = c2[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double m = s * (u1[r] * v1[c] + u2[r] * v2[c] + u3[r] * v3[c]);
            out[4 * r + c] = m;
            tr -= m * c1[c];
            fin = fin && sim3_finite(m);
        }
        out[4 * r + 3] = tr;
        fin = fin && sim3_finite(tr);
    }
    if (!fin) return false;
#pragma unroll
    for (int k = 0; k < 12; ++k) S[k] = out[k];
    *scale = s;
    return true;
}

// the minimal case: the three pairs of one sample (one lane)
PS_DEV bool sim3_fit_sample(const int32_t* __restrict__ id3, const double* __restrict__ pts_1, const double* __restrict__ pts_2,
                            bool fixed_scale, double* __restrict__ S, double* __restrict__ scale)
{
    double P1[9], P2[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t i = (size_t)id3[k];
#pragma unroll
        for (int a = 0; a < 3; ++a) { P1[3 * k + a] = pts_1[3 * i + a]; P2[3 * k + a] = pts_2[3 * i + a]; }
    }
    double c1[3], c2[3], W[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, v = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { c1[a] = ((P1[a] + P1[3 + a]) + P1[6 + a]) / 3.0; c2[a] = ((P2[a] + P2[3 + a]) + P2[6 + a]) / 3.0; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double q1[3] = {P1[3 * k] - c1[0], P1[3 * k + 1] - c1[1], P1[3 * k + 2] - c1[2]};
        const double q2[3] = {P2[3 * k] - c2[0], P2[3 * k + 1] - c2[1], P2[3 * k + 2] - c2[2]};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) W[3 * r + c] += q2[r] * q1[c];
        v += q1[0] * q1[0] + q1[1] * q1[1] + q1[2] * q1[2];
    }
    return sim3_fit(3, c1, c2, W, v, fixed_scale, S, scale);
}

// what the scoring pass reads beside S (12): B = M^T / s^2 and -B t, as the rows of [B | -B t] (12).  One lane; m: 24 doubles.
PS_DEV void sim3_inverse(double* __restrict__ m) {
    double s2 = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) s2 += m[4 * r + c] * m[4 * r + c];
    s2 = s2 / 3.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double tb = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double b = m[4 * c + r] / s2;
            m[12 + 4 * r + c] = b;
            tb -= b * m[4 * c + 3];
        }
        m[12 + 4 * r + 3] = tb;
    }
}

// What a scoring pass needs beside the model: the points, their pixels, the camera and the threshold.
struct Sim3Score {
    const double* __restrict__ pts_1; const double* __restrict__ pts_2; const double* __restrict__ obs_1; const double* __restrict__ obs_2;
    double cu, cv, fu, fv, thresh;
};

template <bool PIXEL> PS_DEV Sim3Score sim3_score(const double* __restrict__ pts_1, const double* __restrict__ pts_2,
                                                  const double* __restrict__ obs_1, const double* __restrict__ obs_2,
                                                  const double* __restrict__ cam, double thresh) {
    if (PIXEL) return Sim3Score{pts_1, pts_2, obs_1, obs_2, cam[0], cam[1], cam[2], cam[3], thresh};
    return Sim3Score{pts_1, pts_2, nullptr, nullptr, 0.0, 0.0, 1.0, 1.0, thresh};
}

// is pair i an inlier of the model m (24, in registers); *e: its error
template <bool PIXEL> PS_DEV bool sim3_point_inlier(const Sim3Score& s, const double (&m)[24], int i, double* __restrict__ e) {
    const size_t j = (size_t)i;
    const double x1 = s.pts_1[3 * j], y1 = s.pts_1[3 * j + 1], z1 = s.pts_1[3 * j + 2];
    const double x2 = s.pts_2[3 * j], y2 = s.pts_2[3 * j + 1], z2 = s.pts_2[3 * j + 2];
    const double a0 = m[0] * x1 + m[1] * y1 + m[2] * z1 + m[3];
    const double a1 = m[4] * x1 + m[5] * y1 + m[6] * z1 + m[7];
    const double a2 = m[8] * x1 + m[9] * y1 + m[10] * z1 + m[11];
    if (!PIXEL) {
        const double d0 = a0 - x2, d1 = a1 - y2, d2 = a2 - z2;
        *e = d0 * d0 + d1 * d1 + d2 * d2;
        return *e < s.thresh;
    }
    const double b0 = m[12] * x2 + m[13] * y2 + m[14] * z2 + m[15];
    const double b1 = m[16] * x2 + m[17] * y2 + m[18] * z2 + m[19];
    const double b2 = m[20] * x2 + m[21] * y2 + m[22] * z2 + m[23];
    const double du2 = s.fu * a0 / a2 + s.cu - s.obs_2[2 * j], dv2 = s.fv * a1 / a2 + s.cv - s.obs_2[2 * j + 1];
    const double du1 = s.fu * b0 / b2 + s.cu - s.obs_1[2 * j], dv1 = s.fv * b1 / b2 + s.cv - s.obs_1[2 * j + 1];
    const double e2 = du2 * du2 + dv2 * dv2, e1 = du1 * du1 + dv1 * dv1;
    *e = (e2 > e1 || e2 != e2) ? e2 : e1;                        // the larger; NaN if either is
    return *e < s.thresh && a2 > 0.0 && b2 > 0.0;
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------

// One workgroup per sample: S_all [H][16], scales [H], counts [H], flags [H] (1: degenerate).
// sample_idx == NULL: one workgroup per GIVEN model (ps_sim3_score): S_all [H][16] is input, counts [H], masks [H][num_pts].
template <bool PIXEL> __global__ __launch_bounds__(256) void k_sim3_hypotheses(
    int num_pts, const int32_t* __restrict__ sample_idx /* [H][3] or NULL */, const double* __restrict__ pts_1,
    const double* __restrict__ pts_2, const double* __restrict__ obs_1, const double* __restrict__ obs_2, const double* __restrict__ cam,
    double thresh, int fixed_scale, double* __restrict__ S_all, double* __restrict__ scales, int32_t* __restrict__ counts,
    uint8_t* __restrict__ flags, uint8_t* __restrict__ masks)
{
    __shared__ double sm[24];
    __shared__ int sok, scount[4];
    const int h = blockIdx.x, t = threadIdx.x;
    if (t == 0) {
        double* out = S_all + (size_t)h * 16;
        bool ok = true;
        if (sample_idx) {
            double S[12], s = 0.0;
            ok = sim3_fit_sample(sample_idx + (size_t)h * 3, pts_1, pts_2, fixed_scale != 0, S, &s);
#pragma unroll
            for (int k = 0; k < 12; ++k) { const double v = ok ? S[k] : 0.0; sm[k] = v; out[k] = v; }
            out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = ok ? 1.0 : 0.0;
            scales[h] = ok ? s : 0.0;
            flags[h] = ok ? 0 : 1;
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) sm[k] = out[k];
        }
        if (ok) sim3_inverse(sm);
        sok = ok ? 1 : 0;
    }
    __syncthreads();
    int cnt = 0;
    if (sok) {                                                   // (uniform over the workgroup)
        double m[24];
#pragma unroll
        for (int k = 0; k < 24; ++k) m[k] = sm[k];
        const Sim3Score score = sim3_score<PIXEL>(pts_1, pts_2, obs_1, obs_2, cam, thresh);
        for (int i = t; i < num_pts; i += 256) {
            double e;
            const bool in = sim3_point_inlier<PIXEL>(score, m, i, &e);
            cnt += in ? 1 : 0;
            if (masks) masks[(size_t)h * num_pts + i] = in ? 1 : 0;
        }
    }
    cnt = rc_block_sum(cnt, scount);
    if (t == 0) counts[h] = cnt;
}

// The first hypothesis with the maximal count: its model (16) and scale to S_best (17).  info: [0] hypothesis [1] raw count
__global__ __launch_bounds__(256) void k_sim3_best(
    int H, const int32_t* __restrict__ counts, const double* __restrict__ S_all, const double* __restrict__ scales,
    int32_t* __restrict__ info, double* __restrict__ S_best /* 17 */)
{
    __shared__ int32_t sc[256], si[256];
    const int t = threadIdx.x;
    const RcBest w = rc_first_max(H, counts, sc, si);
    const int hb = w.index;
    if (t < 16) S_best[t] = S_all[(size_t)hb * 16 + t];
    if (t == 16) S_best[16] = scales[hb];
    if (t == 0) { info[0] = hb; info[1] = w.count; }
}

// One workgroup: the winner's mask, every refit round, the final mask, count and errors.  A thread reads and writes only the mask
// bytes and errors of its own stride, so neither needs a barrier.  Passes over the points: the winner's mask with its centroid sums;
// per round the ten sums about the centroids, then the rescoring, which overwrites mask and sq_err and takes the centroid sums of its
// own mask for the next round.  When the last scored round was adopted, mask and sq_err are final as they stand; otherwise (no round,
// a discarded round) one more pass rescores the kept model, which gives the bits it gave before.
// info: [0..1] from k_sim3_best; out [2] final count [3] rounds adopted [4] how the loop ended [5] the result is degenerate [6..7] 0.
// result: S_21 (16) | scale | sq_err (num_pts; +inf for a degenerate result)
template <bool PIXEL> __global__ __launch_bounds__(256) void k_sim3_refit(
    int num_pts, int iters, int fixed_scale, const double* __restrict__ pts_1, const double* __restrict__ pts_2,
    const double* __restrict__ obs_1, const double* __restrict__ obs_2, const double* __restrict__ cam, double thresh,
    const double* __restrict__ S_best /* 17 */, uint8_t* __restrict__ mask, int32_t* __restrict__ info, double* __restrict__ result)
{
    __shared__ double sm[24], scur[13], snew[13], sred[4 * 10];
    __shared__ int sok, s8[4 * 2];
    const int t = threadIdx.x;
    const Sim3Score score = sim3_score<PIXEL>(pts_1, pts_2, obs_1, obs_2, cam, thresh);
    const bool valid = S_best[15] != 0.0;                        // (uniform; a degenerate winner has no inlier, so no round is adopted)
    double* sq_err = result + 17;
    int count = info[1], rounds = 0, reason = 0;
    bool scored = false;                                         // mask and sq_err are those of the kept model
    if (t < 12) scur[t] = S_best[t];
    if (t == 12) scur[12] = S_best[16];
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) sm[k] = S_best[k];
        if (valid) sim3_inverse(sm);
    }
    __syncthreads();
    double m[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) m[k] = sm[k];
    double a6[6] = {0, 0, 0, 0, 0, 0};                           // the centroid sums of the current mask
    if (iters > 0) {
#pragma unroll 2
        for (int i = t; i < num_pts; i += 256) {
            double e;
            const bool in = sim3_point_inlier<PIXEL>(score, m, i, &e) && valid;
            mask[i] = in ? 1 : 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) { a6[a] += in ? pts_1[3 * (size_t)i + a] : 0.0; a6[3 + a] += in ? pts_2[3 * (size_t)i + a] : 0.0; }
        }
    }
    for (int it = 0; it < iters; ++it) {
        rc_block_partials(a6, sred);
        double c1[3], c2[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { c1[a] = rc_block_total(sred, 6, a) / (double)count; c2[a] = rc_block_total(sred, 6, 3 + a) / (double)count; }
        double a10[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
        for (int i = t; i < num_pts; i += 256) {
            if (!mask[i]) continue;
            const double q1[3] = {pts_1[3 * (size_t)i] - c1[0], pts_1[3 * (size_t)i + 1] - c1[1], pts_1[3 * (size_t)i + 2] - c1[2]};
            const double q2[3] = {pts_2[3 * (size_t)i] - c2[0], pts_2[3 * (size_t)i + 1] - c2[1], pts_2[3 * (size_t)i + 2] - c2[2]};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) a10[3 * r + c] += q2[r] * q1[c];
            a10[9] += q1[0] * q1[0] + q1[1] * q1[1] + q1[2] * q1[2];
        }
        rc_block_partials(a10, sred);                            // (its leading barrier: every thread has read the centroid sums)
        if (t == 0) {
            double W[9], S[12], s = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) W[k] = rc_block_total(sred, 10, k);
            const bool ok = sim3_fit(count, c1, c2, W, rc_block_total(sred, 10, 9), fixed_scale != 0, S, &s);
            if (ok) {
#pragma unroll
                for (int k = 0; k < 12; ++k) { sm[k] = S[k]; snew[k] = S[k]; }
                snew[12] = s;
                sim3_inverse(sm);
            }
            sok = ok ? 1 : 0;
        }
        __syncthreads();
        if (!sok) { reason = 3; break; }                         // (uniform; mask and sq_err are untouched by this round)
#pragma unroll
        for (int k = 0; k < 24; ++k) m[k] = sm[k];
        int two[2] = {0, 0};                                     // the round's count | points whose membership changes
#pragma unroll
        for (int k = 0; k < 6; ++k) a6[k] = 0.0;
#pragma unroll 2
        for (int i = t; i < num_pts; i += 256) {
            double e;
            const bool inl = sim3_point_inlier<PIXEL>(score, m, i, &e);
            const int in = inl ? 1 : 0, cur = mask[i];
            mask[i] = (uint8_t)in;
            sq_err[i] = e;
            two[0] += in; two[1] += in != cur ? 1 : 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) { a6[a] += inl ? pts_1[3 * (size_t)i + a] : 0.0; a6[3 + a] += inl ? pts_2[3 * (size_t)i + a] : 0.0; }
        }
        rc_block_partials(two, s8);
        const int cnt = rc_block_total(s8, 2, 0), changed = rc_block_total(s8, 2, 1);
        if (cnt < count) { reason = 1; scored = false; break; }  // (mask and sq_err are the discarded round's)
        if (t < 13) scur[t] = snew[t];
        count = cnt;
        ++rounds;
        scored = true;
        if (changed == 0) { reason = 2; break; }
    }
    __syncthreads();
    if (!scored) {                                               // (uniform)
        if (t == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) sm[k] = scur[k];
            if (valid) sim3_inverse(sm);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 24; ++k) m[k] = sm[k];
        int fcnt = 0;
#pragma unroll 2
        for (int i = t; i < num_pts; i += 256) {
            double e;
            const bool in = sim3_point_inlier<PIXEL>(score, m, i, &e) && valid;
            sq_err[i] = valid ? e : __builtin_inf();
            mask[i] = in ? 1 : 0;
            fcnt += in ? 1 : 0;
        }
        count = rc_block_sum(fcnt, s8);
    }
    if (t < 12) result[t] = scur[t];
    if (t == 12) result[16] = scur[12];
    if (t == 0) {
        result[12] = 0.0; result[13] = 0.0; result[14] = 0.0; result[15] = valid ? 1.0 : 0.0;
        info[2] = count; info[3] = rounds; info[4] = reason; info[5] = valid ? 0 : 1; info[6] = 0; info[7] = 0;
    }
}
