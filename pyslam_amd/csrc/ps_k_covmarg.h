// ps_k_covmarg.h -- batched marginal covariances of every reduced pose and every variable landmark (ps_covariance_marginals).
// Part of ps_core.hip (one translation unit; included after ps_kernels.h).
//
// The reduced system S of ps_covariance_begin (lambda = 0) is densified and factored by the lagged inverse's direct-seed
// kernels (k_ldi_dense64, k_bchol_panel / k_bchol_update, k_btri_inverse / k_btri_merge: L L^T = S, X = L^-1), then
//     Sigma_pp = S^-1 = X^T X                                            (k_cov_sigma: fp64 MFMA, lower triangle, mirrored)
// and for a landmark with observations i, j on variable poses r_i, r_j, M = C^-1 (its packed lower factor) and Z_i the
// observation's 6 x 3 row of the Schur elimination (zrow_expand):
//     Sigma_ll = M^T (I + sum_{i,j} Z_i^T Sigma_pp[r_i, r_j] Z_j) M    (k_cov_landmarks)
// -- the closed form of k_cov_rhs -> reduced solve -> k_backsub, which compute one column of the same matrix -- and the cross
// blocks between any two of them (k_cov_cross): Sigma_al = -sum_i Sigma_pp[a, r_i] Z_i M, Sigma_l1l2 = M1^T (sum_ij Z_i^T
// Sigma_pp[r_i, r_j] Z_j) M2.
#pragma once

typedef double ps_f64x4 __attribute__((ext_vector_type(4)));

// S = L L^T is numerically singular where a pivot falls below this fraction of its diagonal entry of S (a free gauge leaves
// pivots of rounding size, which k_bchol_panel's "> 0" test alone may let through)
#define PS_COV_PIVOT_RTOL 1e-10

// diag[i] = A[i][i] of the dense S, before the factorisation overwrites it
__global__ __launch_bounds__(256) void k_cov_diag_save(int n, const double* __restrict__ A, double* __restrict__ diag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) diag[i] = A[(size_t)i * n + i];
}

// pivot j of the factorisation = L_jj^2 = 1 / Tinv_jj^2 (Tinv: the inverse of every PS_BC_W step's diagonal factor, written by
// k_bchol_panel); a pivot that is not above PS_COV_PIVOT_RTOL * S_jj (NaN included) marks the factorisation as failed
__global__ __launch_bounds__(256) void k_cov_pivot_check(int n, const double* __restrict__ diag, const double* __restrict__ Tinv,
                                                         int32_t* __restrict__ stat)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = i / PS_BC_W, j = i % PS_BC_W;
    const double ti = Tinv[(size_t)s * PS_BC_W * PS_BC_W + j * PS_BC_W + j];
    const double pivot = 1.0 / (ti * ti);
    if (!(pivot > PS_COV_PIVOT_RTOL * diag[i]) || !(diag[i] > 0.0)) stat[ST_DIAG_FAIL] = 1;
}

// ---------------------------------------------------------------------------
// C = X^T X for X = L^-1 (n x n, row-major, lower triangular: only entries k >= i of column i are read, whatever the buffer
// holds above the diagonal).  Lower tiles only: one 64 x 64 tile (I >= J) per 256-thread workgroup, 2 x 2 waves of 32 x 32,
// each wave 2 x 2 v_mfma_f64_16x16x4_f64 accumulators.  C[i][j] = sum_{k >= i} X[k][i] X[k][j] (i >= j), so the K range of
// tile row I starts at its first row.  Operand layouts (MI355X microarchitecture guide): A: lane l holds A[l & 15][l >> 4],
// B: B[l >> 4][l & 15], D: register r of lane l is D[(l >> 4) + 4 r][l & 15].  Both operands are rows of X: A[i][k] =
// X[k][i0 + i], B[k][j] = X[k][j0 + j], staged through LDS as [k][64] (coalesced row pieces).  Entries above the diagonal of
// a diagonal tile are not written; k_cov_mirror copies the lower triangle there.
// ---------------------------------------------------------------------------
#define PS_CS_T 64
#define PS_CS_K 16
__global__ __launch_bounds__(256) void k_cov_sigma(int n, const double* __restrict__ X, double* __restrict__ C)
{
    __shared__ double As[PS_CS_K][PS_CS_T + 2];
    __shared__ double Bs[PS_CS_K][PS_CS_T + 2];
    // tile (ti >= tj) from the linear index
    int ti = (int)((sqrt(8.0 * blockIdx.x + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
    while (ti * (ti + 1) / 2 > (int)blockIdx.x) --ti;
    const int tj = blockIdx.x - ti * (ti + 1) / 2;
    const int i0 = ti * PS_CS_T, j0 = tj * PS_CS_T;
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const int wi = w >> 1, wj = w & 1;
    ps_f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = ps_f64x4{0.0, 0.0, 0.0, 0.0};
    // staging: element e = t + 256 q of a 16 x 64 chunk is (row e >> 6, column e & 63)
    double ra[4], rb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + 256 * q, k = k0 + (e >> 6), c = e & 63;
            const int ia = i0 + c, jb = j0 + c;
            ra[q] = (k < n && ia < n && k >= ia) ? X[(size_t)k * n + ia] : 0.0;
            rb[q] = (k < n && jb < n && k >= jb) ? X[(size_t)k * n + jb] : 0.0;
        }
    };
    load(i0);
    for (int k0 = i0; k0 < n; k0 += PS_CS_K) {
        __syncthreads();                                   // (the previous chunk's fragment reads are done)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + 256 * q;
            As[e >> 6][e & 63] = ra[q];
            Bs[e >> 6][e & 63] = rb[q];
        }
        __syncthreads();
        if (k0 + PS_CS_K < n) load(k0 + PS_CS_K);          // the next chunk's loads fly during this chunk's MFMAs
#pragma unroll
        for (int kq = 0; kq < PS_CS_K; kq += 4) {
            const int kk = kq + (l >> 4);
            double fa[2], fb[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                fa[a] = As[kk][wi * 32 + a * 16 + (l & 15)];
                fb[a] = Bs[kk][wj * 32 + a * 16 + (l & 15)];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wi * 32 + a * 16 + (l >> 4) + 4 * r, j = j0 + wj * 32 + b * 16 + (l & 15);
                if (i < n && j < n && (ti > tj || i >= j)) C[(size_t)i * n + j] = acc[a][b][r];
            }
}

// C's strictly upper triangle <- its lower triangle, 32 x 32 tiles through LDS: the result is exactly symmetric
__global__ __launch_bounds__(256) void k_cov_mirror(int n, double* __restrict__ C)
{
    __shared__ double tile[32][33];
    if (blockIdx.x > blockIdx.y) return;                   // tile (I = y, J = x), I >= J: read below, write above
    const int I = blockIdx.y * 32, J = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int r = ty; r < 32; r += 8) {
        const int i = I + r, j = J + tx;
        tile[r][tx] = (i < n && j < n) ? C[(size_t)i * n + j] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int r = ty; r < 32; r += 8) {                     // C[J + r][I + tx] = C[I + tx][J + r] where I + tx > J + r
        const int i = J + r, j = I + tx;
        if (i < n && j < n && j > i) C[(size_t)i * n + j] = tile[tx][r];
    }
}

// out[k] (D x D) = C[a_k, b_k] block (a, b null: the diagonal block k of every reduced pose)
__global__ __launch_bounds__(256) void k_cov_gather(int nblk, int D, int n, const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                    const double* __restrict__ C, double* __restrict__ out)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const int DD = D * D;
    if (e >= (long)nblk * DD) return;
    const int k = (int)(e / DD), rc = (int)(e % DD), r = rc / D, c = rc % D;
    const int ra = a ? a[k] : k, rb = b ? b[k] : k;
    out[e] = C[(size_t)(ra * D + r) * n + rb * D + c];
}

// ---------------------------------------------------------------------------
// Landmark marginals, 16 lanes per landmark slot v (k_backsub's mapping): lane `sub` takes observations sub, sub + 16, ... of
// the landmark (tracks longer than 16 loop) and sums Z_i^T Sigma[r_i, r_j] Z_j over ALL observations j of the same landmark,
// in index order; the 16 partial sums are reduced in a fixed order (group16_sum), so repeated calls are bit-identical.
// Observations on constant poses (reduced index -1 in their Z row) contribute nothing.  With T the (symmetrised) sum:
// out[v] = M^T (I + T) M, lower triangle computed, mirrored (exactly symmetric).  Slot order: the host maps it to vid.
// ---------------------------------------------------------------------------

// acc (3 x 3, this lane's part) += sum over observations i = beg1 + sub, beg1 + sub + 16, ... < end1 and ALL j in [beg2, end2),
// in index order, of Z_i^T Sigma[r_i, r_j] Z_j (both on variable poses).  beg1 == beg2: the landmark marginals' sum
PS_DEV void cov_zsz_accumulate(int sub, int n, int beg1, int end1, int beg2, int end2, const double* __restrict__ Z,
                               const double* __restrict__ Sigma, double* __restrict__ acc)
{
    for (int i = beg1 + sub; i < end1; i += PS_LM_GROUP) {
        const double* zr = Z + PS_ZROW * (size_t)i;
        const int ri = (int)zr[12];
        if (ri < 0) continue;
        double zi[18];
        zrow_expand(zr, zr + 9, zi);
        for (int j = beg2; j < end2; ++j) {
            const double* zs = Z + PS_ZROW * (size_t)j;
            const int rj = (int)zs[12];
            if (rj < 0) continue;
            double zj[18];
            zrow_expand(zs, zs + 9, zj);
            const double* sg = Sigma + (size_t)ri * 6 * n + (size_t)rj * 6;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                // row a of Sigma[r_i, r_j] Z_j, then acc += Z_i[a]^T (that row)
                double s[6];
#pragma unroll
                for (int c = 0; c < 6; ++c) s[c] = sg[(size_t)a * n + c];
                double w[3];
#pragma unroll
                for (int bb = 0; bb < 3; ++bb) {
                    double x = 0.0;
#pragma unroll
                    for (int c = 0; c < 6; ++c) x += s[c] * zj[3 * c + bb];
                    w[bb] = x;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int bb = 0; bb < 3; ++bb) acc[3 * k + bb] += zi[3 * a + k] * w[bb];
            }
        }
    }
}

// o (3 x 3, row-major) = M^T (I + sym(T)) M for the reduced sum T (acc) and the landmark's packed factor m
PS_DEV void cov_landmark_finish(const double* __restrict__ acc, const double* __restrict__ m, double* __restrict__ o)
{
    double N[9];                                           // I + sym(T)
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int bb = 0; bb < 3; ++bb) N[3 * k + bb] = 0.5 * (acc[3 * k + bb] + acc[3 * bb + k]) + (k == bb ? 1.0 : 0.0);
    const double M[9] = {m[0], 0.0, 0.0, m[1], m[2], 0.0, m[3], m[4], m[5]};       // M00 M10 M11 M20 M21 M22 (lower)
    double Q[9];                                           // Q = N M
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Q[3 * r + c] = N[3 * r] * M[c] + N[3 * r + 1] * M[3 + c] + N[3 * r + 2] * M[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {                     // (M^T Q)[r][c] = sum_a M[a][r] Q[a][c]
            const double x = M[r] * Q[c] + M[3 + r] * Q[3 + c] + M[6 + r] * Q[6 + c];
            o[3 * r + c] = x;
            o[3 * c + r] = x;
        }
}

__global__ __launch_bounds__(256) void k_cov_landmarks(
    int nv, int n, const int32_t* __restrict__ lm_ptr, const double* __restrict__ Z, const double* __restrict__ Cinv,
    const double* __restrict__ Sigma, double* __restrict__ out)
{
    const int v = blockIdx.x * (blockDim.x / PS_LM_GROUP) + threadIdx.x / PS_LM_GROUP;
    const int sub = threadIdx.x & (PS_LM_GROUP - 1);
    const bool live = v < nv;                              // whole 16-lane groups are live or not
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    if (live) cov_zsz_accumulate(sub, n, lm_ptr[v], lm_ptr[v + 1], lm_ptr[v], lm_ptr[v + 1], Z, Sigma, acc);
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = group16_sum(acc[k]);
    if (!live || sub != 0) return;
    cov_landmark_finish(acc, Cinv + 6 * (size_t)v, out + 9 * (size_t)v);
}

// ---------------------------------------------------------------------------
// Any block of the full covariance (ps_covariance_cross_blocks), one 16-lane group per pair k.  rec[4 k ..] = (kind_a, a,
// kind_b, b): kind 0 a reduced pose index, kind 1 a landmark SLOT (the host maps vid -> slot).  out[36 k ..]: the block
// row-major, dof_a x dof_b, in the leading entries, the rest zero.  With M the landmark's packed factor (C^-1 = M^T M):
//   (pose a, pose b)    Sigma[a, b], copied (k_cov_gather's values)
//   (pose a, lm l)      -sum_{i in l, r_i >= 0} Sigma[a, r_i] Z_i M  (6 x 3; lanes stride over l's observations) -- the pose
//                       part of k_cov_rhs -> reduced solve for l's columns
//   (lm l, pose a)      the transpose of (a, l): the same arithmetic, stored transposed
//   (lm l, lm l)        k_cov_landmarks' marginal, the same code (bit-identical)
//   (lm l1, lm l2)      M1^T (sum_{i in l1, j in l2} Z_i^T Sigma[r_i, r_j] Z_j) M2 for slot l1 < l2; l1 > l2 is computed as
//                       (l2, l1) and stored transposed
// Every group runs the same 18 fixed-order reductions, so a pair's result does not depend on its neighbours or its chunk.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cov_cross(
    int m, int n, int D, const int32_t* __restrict__ rec, const int32_t* __restrict__ lm_ptr, const double* __restrict__ Z,
    const double* __restrict__ Cinv, const double* __restrict__ Sigma, double* __restrict__ out)
{
    const int k = blockIdx.x * (blockDim.x / PS_LM_GROUP) + threadIdx.x / PS_LM_GROUP;
    const int sub = threadIdx.x & (PS_LM_GROUP - 1);
    const bool live = k < m;                               // whole 16-lane groups are live or not
    int ka = 0, a = 0, kb = 0, b = 0;
    if (live) { ka = rec[4 * k]; a = rec[4 * k + 1]; kb = rec[4 * k + 2]; b = rec[4 * k + 3]; }
    const bool pl = ka != kb;                              // pose-landmark, either order
    const int p = ka == 0 ? a : b, l = ka == 0 ? b : a;    // (pose-landmark pairs)
    const bool swap_ll = ka == 1 && kb == 1 && a > b;
    const int l1 = swap_ll ? b : a, l2 = swap_ll ? a : b;  // (landmark pairs: canonical slot order)
    double acc[18];
#pragma unroll
    for (int q = 0; q < 18; ++q) acc[q] = 0.0;
    if (live && pl) {
        // acc (6 x 3) = sum_i Sigma[p, r_i] Z_i
        for (int i = lm_ptr[l] + sub; i < lm_ptr[l + 1]; i += PS_LM_GROUP) {
            const double* zr = Z + PS_ZROW * (size_t)i;
            const int ri = (int)zr[12];
            if (ri < 0) continue;
            double zi[18];
            zrow_expand(zr, zr + 9, zi);
            const double* sg = Sigma + (size_t)p * 6 * n + (size_t)ri * 6;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                double s[6];
#pragma unroll
                for (int c = 0; c < 6; ++c) s[c] = sg[(size_t)r * n + c];
#pragma unroll
                for (int bb = 0; bb < 3; ++bb) {
                    double x = 0.0;
#pragma unroll
                    for (int c = 0; c < 6; ++c) x += s[c] * zi[3 * c + bb];
                    acc[3 * r + bb] += x;
                }
            }
        }
    } else if (live && ka == 1)
        cov_zsz_accumulate(sub, n, lm_ptr[l1], lm_ptr[l1 + 1], lm_ptr[l2], lm_ptr[l2 + 1], Z, Sigma, acc);
#pragma unroll
    for (int q = 0; q < 18; ++q) acc[q] = group16_sum(acc[q]);
    if (!live) return;
    double* o = out + 36 * (size_t)k;
    if (ka == 0 && kb == 0) {                              // pose-pose: a copy of Sigma[a, b]
        for (int e = sub; e < 36; e += PS_LM_GROUP) {
            const int r = e / D, c = e % D;
            o[e] = e < D * D ? Sigma[(size_t)(a * D + r) * n + b * D + c] : 0.0;
        }
        return;
    }
    // every lane forms the whole block from the broadcast sums; lane sub stores entries sub, sub + 16, sub + 32
    double res[36];
#pragma unroll
    for (int e = 0; e < 36; ++e) res[e] = 0.0;
    if (pl) {
        const double* mm = Cinv + 6 * (size_t)l;
        const double M[9] = {mm[0], 0.0, 0.0, mm[1], mm[2], 0.0, mm[3], mm[4], mm[5]};
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double x = -(acc[3 * r] * M[c] + acc[3 * r + 1] * M[3 + c] + acc[3 * r + 2] * M[6 + c]);
                if (ka == 0) res[3 * r + c] = x;           // (pose, landmark): 6 x 3
                else res[6 * c + r] = x;                   // (landmark, pose): 3 x 6
            }
    } else if (l1 == l2) {
        cov_landmark_finish(acc, Cinv + 6 * (size_t)l1, res);
    } else {
        const double* m1 = Cinv + 6 * (size_t)l1;
        const double* m2 = Cinv + 6 * (size_t)l2;
        const double M1[9] = {m1[0], 0.0, 0.0, m1[1], m1[2], 0.0, m1[3], m1[4], m1[5]};
        const double M2[9] = {m2[0], 0.0, 0.0, m2[1], m2[2], 0.0, m2[3], m2[4], m2[5]};
        double Q[9];                                       // Q = T M2
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Q[3 * r + c] = acc[3 * r] * M2[c] + acc[3 * r + 1] * M2[3 + c] + acc[3 * r + 2] * M2[6 + c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {                  // (M1^T Q)[r][c]
                const double x = M1[r] * Q[c] + M1[3 + r] * Q[3 + c] + M1[6 + r] * Q[6 + c];
                if (swap_ll) res[3 * c + r] = x;           // (static indices: the array stays in registers)
                else res[3 * r + c] = x;
            }
    }
#pragma unroll
    for (int e = 0; e < 36; ++e)
        if ((e & (PS_LM_GROUP - 1)) == sub) o[e] = res[e];
}
