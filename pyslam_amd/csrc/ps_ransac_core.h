// ps_ransac_core.h -- what the RANSAC front ends on the device share (gfx950): frame-to-frame rigid alignment (ps_ransac.h),
// two-view essential matrix (ps_k_twoview.h), absolute pose (ps_k_pnp.h), similarity alignment (ps_k_sim3.h).  Part of ps_core.hip,
// included before the four.
//
//   rc_first_max        np.argmax over int32 counts: the FIRST index with the maximal count.  Every front end's contract.
//   rc_block_sum        sum over the workgroup of 256 in a fixed order; rc_block_partials / rc_block_total for several sums at once
//   rc_jacobi3          the sweeps of the one-sided (Hestenes) Jacobi SVD of a 3 x 3 and its singular values
//   rc_sort3            columns by descending singular value
//
// All kernels here run workgroups of exactly 256 threads (four waves of 64).  No atomics: the order of every addition is fixed,
// so two calls on the same input are bit-identical, and that order is part of the results.
#pragma once
#include "ps_math.h"

struct RcBest { int index, count; };

// The first maximum of counts[0..n) (n >= 1), to every thread.  sc, si: LDS, 256 each.  A thread keeps the first maximum of
// its own ascending stride; the tree prefers the lower index on equal counts.
PS_DEV RcBest rc_first_max(int n, const int32_t* __restrict__ counts, int32_t* __restrict__ sc, int32_t* __restrict__ si) {
    const int t = threadIdx.x;
    int bc = -1, bi = 0x7fffffff;
    for (int h = t; h < n; h += 256) {
        const int c = counts[h];
        if (c > bc) { bc = c; bi = h; }
    }
    sc[t] = bc; si[t] = bi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
            const int c2 = sc[t + off], i2 = si[t + off];
            if (c2 > sc[t] || (c2 == sc[t] && i2 < si[t])) { sc[t] = c2; si[t] = i2; }
        }
        __syncthreads();
    }
    return RcBest{si[0], sc[0]};
}

// K sums at once: the xor tree inside each wave, then the four waves' partials to s (LDS, [4][K]).  After it
// rc_block_total(s, K, k) is sum k, for every thread.  (The leading barrier: s may still be read from the previous call.)
template <typename T, int K> PS_DEV void rc_block_partials(const T (&v)[K], T* __restrict__ s) {
    T w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        w[k] = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) w[k] += __shfl_xor(w[k], off, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s[(threadIdx.x >> 6) * K + k] = w[k];
    }
    __syncthreads();
}

template <typename T> PS_DEV T rc_block_total(const T* __restrict__ s, int K, int k) {
    return ((s[k] + s[K + k]) + s[2 * K + k]) + s[3 * K + k];       // waves 0..3 in this order
}

// sum of `v` over the workgroup, to every thread.  s4: LDS, 4.
template <typename T> PS_DEV T rc_block_sum(T v, T* __restrict__ s4) {
    const T one[1] = {v};
    rc_block_partials(one, s4);
    return rc_block_total(s4, 1, 0);
}

// One-sided Jacobi on the columns of a 3 x 3: A[col][row] in, A V out with orthogonal columns (up to 30 sweeps), V[col][row]
// the accumulated rotations, sg the column norms (singular values, unsorted).  Relative accuracy ~eps sigma_1 / sigma_2: no
// squaring of the condition number as with A^T A.  NAN_ROTATES is the caller's treatment of a non-finite column pair: true
// rotates it (ransac_align), false skips it (tv_svd2); the outputs differ, so each caller keeps its own.
// Compiled under the default contraction: a caller under `fp contract(off)` (pnp_align3) cannot share it without changing bits.
template <bool NAN_ROTATES> PS_DEV void rc_jacobi3(double (&A)[3][3], double (&V)[3][3], double (&sg)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) V[c][r] = c == r ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double al = A[p][0] * A[p][0] + A[p][1] * A[p][1] + A[p][2] * A[p][2];
            const double be = A[q][0] * A[q][0] + A[q][1] * A[q][1] + A[q][2] * A[q][2];
            const double ga = A[p][0] * A[q][0] + A[p][1] * A[q][1] + A[p][2] * A[q][2];
            if (ga == 0.0 || (NAN_ROTATES ? fabs(ga) <= 1.2e-16 * sqrt(al * be) : !(fabs(ga) > 1.2e-16 * sqrt(al * be)))) continue;
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
#pragma unroll
    for (int k = 0; k < 3; ++k) sg[k] = sqrt(A[k][0] * A[k][0] + A[k][1] * A[k][1] + A[k][2] * A[k][2]);
}

// Columns of A and V by descending sg: three compare-exchanges on static indices (no runtime-indexed private array).
// Data movement only, so it serves callers of either contraction mode.
PS_DEV void rc_sort3(double (&sg)[3], double (&A)[3][3], double (&V)[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = k == 2 ? 1 : 0, j = k == 0 ? 1 : 2;           // (0, 1) (0, 2) (1, 2)
        if (sg[j] > sg[i]) {
            double w = sg[i]; sg[i] = sg[j]; sg[j] = w;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                w = A[i][r]; A[i][r] = A[j][r]; A[j][r] = w;
                w = V[i][r]; V[i][r] = V[j][r]; V[j][r] = w;
            }
        }
    }
}
