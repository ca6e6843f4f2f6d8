// ps_k_dense.h -- the dense RGB-D VO pipeline on the device (reference pyslam/pipelines/dense.py, keyframes.py):
// image pyramid, keyframe pixel tables and the coarse-to-fine solve of one tracked frame.
//
//   k_dense_level0      thread / pixel          : level-0 image as float64 (u8 / 255.)
//   k_dense_pyrdown<T>  16 x 16 tile / block    : cv2.pyrDown restated (pipelines/imgproc.py: pyr_down), LDS tile with a
//                                                 2-pixel halo; the raw (u8 or f64) level feeds the next, as the reference
//                                                 chains cv2.pyrDown, and the level's float64 image is raw / 255.
//   k_dense_grad        thread / pixel          : 0.5 * Sobel (imgproc.sobel) and the depth level depth[::2^l, ::2^l]
//   k_dense_flags       256 pixels / block      : RGBDCamera.is_valid_measurement && |grad| >= min_grad, block counts
//   k_dense_scan        one block               : exclusive scan of the block counts, pixel count of the level
//   k_dense_compact     256 pixels / block      : the surviving pixels in raster order -> PhotometricResidualSE3's tables
//   k_dense_pass        as k_photo_pass         : k_photo_pass with the pixel count read from the device
//   k_dense_finish      one block               : k_photo_finish + Problem.solve's stopping rule (the device state machine)
//
// Bit-exactness: the pyramid, the gradient, the selection predicate and the triangulation must reproduce the host
// arithmetic exactly (a gradient at the threshold must not flip), so those functions turn FMA contraction off.
#pragma once
#include "ps_photo.h"
#include "ps_stop_rule.h"

#define PS_DENSE_TILE 16
#define PS_DENSE_MAX_LEVELS 8

PS_DEV int dense_reflect101(int p, int n) {           // OpenCV borderInterpolate, BORDER_REFLECT_101
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

__global__ __launch_bounds__(256) void k_dense_level0(const void* __restrict__ raw, int is_u8, int n, double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = is_u8 ? (double)((const uint8_t*)raw)[i] : ((const double*)raw)[i];
    out[i] = v / 255.0;
}

template <typename T> struct DensePyrAcc;
template <> struct DensePyrAcc<uint8_t> {
    typedef int H;
    PS_DEV static int row(int a, int b, int c, int d, int e) { return a + 4 * b + 6 * c + 4 * d + e; }
    PS_DEV static uint8_t out(int a, int b, int c, int d, int e) { return (uint8_t)((row(a, b, c, d, e) + 128) >> 8); }
};
template <> struct DensePyrAcc<double> {
    typedef double H;
    PS_DEV static double row(double a, double b, double c, double d, double e) {
#pragma clang fp contract(off)
        return c * 6.0 + (b + d) * 4.0 + a + e;
    }
    PS_DEV static double out(double a, double b, double c, double d, double e) {
#pragma clang fp contract(off)
        return row(a, b, c, d, e) * (1.0 / 256.0);
    }
};

// src (sh x sw) -> dst (dh x dw) = ((sh+1)/2, (sw+1)/2); dstf = dst / 255.
template <typename T>
__global__ __launch_bounds__(256) void k_dense_pyrdown(const T* __restrict__ src, int sh, int sw, T* __restrict__ dst,
                                                        double* __restrict__ dstf, int dh, int dw)
{
#pragma clang fp contract(off)
    typedef typename DensePyrAcc<T>::H H;
    constexpr int S = 2 * PS_DENSE_TILE + 3;                      // 35 source rows / columns: 2 * 16 + the 2-pixel halo each side
    __shared__ T tile[S][S + 1];
    __shared__ H hrow[S][PS_DENSE_TILE + 1];
    const int oy0 = blockIdx.y * PS_DENSE_TILE, ox0 = blockIdx.x * PS_DENSE_TILE;
    const int sy0 = 2 * oy0 - 2, sx0 = 2 * ox0 - 2;
    for (int k = threadIdx.x; k < S * S; k += 256) {
        const int r = k / S, c = k % S;
        tile[r][c] = src[(size_t)dense_reflect101(sy0 + r, sh) * sw + dense_reflect101(sx0 + c, sw)];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < S * PS_DENSE_TILE; k += 256) {  // horizontal pass first
        const int r = k / PS_DENSE_TILE, c = 2 * (k % PS_DENSE_TILE);
        hrow[r][k % PS_DENSE_TILE] = DensePyrAcc<T>::row(tile[r][c], tile[r][c + 1], tile[r][c + 2], tile[r][c + 3], tile[r][c + 4]);
    }
    __syncthreads();
    const int ty = threadIdx.x / PS_DENSE_TILE, tx = threadIdx.x % PS_DENSE_TILE;
    const int oy = oy0 + ty, ox = ox0 + tx;
    if (oy >= dh || ox >= dw) return;
    const int r = 2 * ty;
    const T v = (T)DensePyrAcc<T>::out(hrow[r][tx], hrow[r + 1][tx], hrow[r + 2][tx], hrow[r + 3][tx], hrow[r + 4][tx]);
    dst[(size_t)oy * dw + ox] = v;
    dstf[(size_t)oy * dw + ox] = (double)v / 255.0;
}

// gx = 0.5 * Sobel_x, gy = 0.5 * Sobel_y of the level image; dl = depth[(v << l), (u << l)] (NaN when there is no depth)
__global__ __launch_bounds__(256) void k_dense_grad(const double* __restrict__ im, int h, int w, const double* __restrict__ depth0,
                                                     int w0, int shift, double* __restrict__ gx, double* __restrict__ gy,
                                                     double* __restrict__ dl)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= h * w) return;
    const int v = i / w, u = i % w;
    const int um = dense_reflect101(u - 1, w), up = dense_reflect101(u + 1, w);
    const int vm = dense_reflect101(v - 1, h), vp = dense_reflect101(v + 1, h);
    const double* rm = im + (size_t)vm * w;
    const double* r0 = im + (size_t)v * w;
    const double* rp = im + (size_t)vp * w;
    const double tm = rm[up] - rm[um], t0 = r0[up] - r0[um], tp = rp[up] - rp[um];
    gx[i] = 0.5 * (tm + 2.0 * t0 + tp);
    const double sm = rm[um] + 2.0 * rm[u] + rm[up];
    const double sp = rp[um] + 2.0 * rp[u] + rp[up];
    gy[i] = 0.5 * (sp - sm);
    dl[i] = depth0 ? depth0[(size_t)(v << shift) * w0 + (u << shift)] : __builtin_nan("");
}

struct DenseCam { double cu, cv, fu, fv, w, h; };

// the pixel predicate of PhotometricResidualSE3.__init__: RGBDCamera.is_valid_measurement(u, v, depth) && |grad| >= min_grad
PS_DEV bool dense_keep(const DenseCam& c, int u, int v, double d, double gx, double gy, double min_grad) {
#pragma clang fp contract(off)
    const double uu = (double)u, vv = (double)v;
    const bool valid = (d > 0.0) && (vv > 0.0) && (vv < c.h) && (uu > 0.0) && (uu < c.w);
    return valid && sqrt(gx * gx + gy * gy) >= min_grad;
}

__global__ __launch_bounds__(256) void k_dense_flags(int n, int w, DenseCam cam, double min_grad, const double* __restrict__ gx,
                                                      const double* __restrict__ gy, const double* __restrict__ dl,
                                                      uint8_t* __restrict__ flags, int* __restrict__ block_counts)
{
    __shared__ int wc[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < n && dense_keep(cam, i % w, i / w, dl[i], gx[i], gy[i], min_grad);
    if (i < n) flags[i] = keep ? 1 : 0;
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// exclusive scan of nb block counts in place; *total = their sum (the level's pixel count)
__global__ __launch_bounds__(1024) void k_dense_scan(int nb, int* __restrict__ counts, int* __restrict__ total) {
    __shared__ int part[1024];
    const int per = (nb + 1023) / 1024, b0 = threadIdx.x * per;
    int s = 0;
    for (int k = b0; k < min(b0 + per, nb); ++k) s += counts[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {                   // inclusive Hillis-Steele scan
        const int add = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    int run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (int k = b0; k < min(b0 + per, nb); ++k) { const int c = counts[k]; counts[k] = run; run += c; }
    if (threadIdx.x == 1023) *total = part[1023];
}

struct DenseTables { double *pt_ref, *im_ref, *im_jac, *tri_jac_d; };

// the kept pixels in raster order: triangulation as RGBDCamera.triangulate, ((u - cu) * z) / fu etc.
__global__ __launch_bounds__(256) void k_dense_compact(int n, int w, DenseCam cam, const double* __restrict__ im,
                                                        const double* __restrict__ gx, const double* __restrict__ gy,
                                                        const double* __restrict__ dl, const uint8_t* __restrict__ flags,
                                                        const int* __restrict__ block_offsets, DenseTables t)
{
#pragma clang fp contract(off)
    __shared__ int wc[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < n && flags[i];
    const unsigned long long m = __ballot(keep);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wc[wv] = __popcll(m);
    __syncthreads();
    if (!keep) return;
    int k = block_offsets[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int q = 0; q < wv; ++q) k += wc[q];
    const double u = (double)(i % w), v = (double)(i / w), z = dl[i];
    const double inv_fu = 1.0 / cam.fu, inv_fv = 1.0 / cam.fv;
    t.pt_ref[3 * (size_t)k] = (u - cam.cu) * z / cam.fu;
    t.pt_ref[3 * (size_t)k + 1] = (v - cam.cv) * z / cam.fv;
    t.pt_ref[3 * (size_t)k + 2] = z;
    t.im_ref[k] = im[i];
    t.im_jac[2 * (size_t)k] = gx[i];
    t.im_jac[2 * (size_t)k + 1] = gy[i];
    t.tri_jac_d[3 * (size_t)k] = (u - cam.cu) * inv_fu;
    t.tri_jac_d[3 * (size_t)k + 1] = (v - cam.cv) * inv_fv;
    t.tri_jac_d[3 * (size_t)k + 2] = 1.0;
}

// ---- the coarse-to-fine solve ------------------------------------------------------------------------------------------
// Device state of one tracked frame.  Each level enqueues a start-cost pass and max_iters + 1 iteration slots; once the
// stopping rule fires (or a level fails) `done` is set and every later launch of the level returns at once.
struct DenseSolveState {
    int done, failed;                   // failed: 0, 1 fewer than 6 valid pixels, 2 H not positive definite (sticky)
    ps_stop_state stop;                 // the level's iteration count, non-decreasing steps and last cost (ps_stop_rule.h)
    double dx_norm;
    double best[12];
};

__global__ __launch_bounds__(256) void k_dense_pass(PhotoArgs a, const int* __restrict__ n_dev, const double* __restrict__ pose,
                                                     int with_normal, int start, double* __restrict__ partials,
                                                     const DenseSolveState* __restrict__ st)
{
    if (start ? st->failed : st->done) return;          // (a level's start pass follows the previous level's `done`)
    a.n = *n_dev;
    __shared__ double lds[4][PS_PHOTO_NACC];
    const Se3 T = se3_load(pose);
    double acc[PS_PHOTO_NACC];
#pragma unroll
    for (int k = 0; k < PS_PHOTO_NACC; ++k) acc[k] = 0.0;
    const int base = blockIdx.x * (256 * PS_PHOTO_PPT) + threadIdx.x;
#pragma unroll
    for (int q = 0; q < PS_PHOTO_PPT; ++q) {
        const int i = base + q * 256;
        if (i >= a.n) continue;
        double r, J[6];
        bool ok;
        if (with_normal) ok = photo_eval<true>(a, T, i, r, J); else ok = photo_eval<false>(a, T, i, r, J);
        if (!ok) continue;
        acc[27] += ps_loss_rho(a.loss_id, a.loss_k, r);
        acc[28] += 1.0;
        if (with_normal) {
            const double wgt = ps_loss_weight(a.loss_id, a.loss_k, r);
            int k = 0;
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const double wj = wgt * J[c];
#pragma unroll
                for (int c2 = c; c2 < 6; ++c2) acc[k++] += wj * J[c2];
                acc[21 + c] -= wj * r;
            }
        }
    }
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 29; ++k) {
        if (!with_normal && k < 27) continue;
        const double v = wave_sum(acc[k]);
        if (lane == 0) lds[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < PS_PHOTO_NACC) {
        const int k = threadIdx.x;
        const bool used = k < 29 && (with_normal || k >= 27);
        partials[(size_t)blockIdx.x * PS_PHOTO_NACC + k] = used ? ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k] : 0.0;
    }
}

// in-place Cholesky solve of the leading n x n system (n = 6 or 3); false when H is not positive definite
PS_DEV bool dense_chol_solve(double (*H)[6], const double* b, int n, double* dx) {
    double L[6][6];
    for (int j = 0; j < n; ++j) {
        double d = H[j][j];
        for (int q = 0; q < j; ++q) d -= L[j][q] * L[j][q];
        if (!(d > 0.0)) return false;
        L[j][j] = sqrt(d);
        for (int i = j + 1; i < n; ++i) {
            double s = H[i][j];
            for (int q = 0; q < j; ++q) s -= L[i][q] * L[j][q];
            L[i][j] = s / L[j][j];
        }
    }
    for (int i = 0; i < n; ++i) {
        double s = b[i];
        for (int q = 0; q < i; ++q) s -= L[i][q] * dx[q];
        dx[i] = s / L[i][i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = dx[i];
        for (int q = i + 1; q < n; ++q) s -= L[q][i] * dx[q];
        dx[i] = s / L[i][i];
    }
    return true;
}

// R <- exp(phi) R (SO3 perturbation of the reference's R_1_0 parameter); t is left to the caller
PS_DEV void dense_rotate(Se3& T, const double* phi) {
    const double rot[6] = {0.0, 0.0, 0.0, phi[0], phi[1], phi[2]};
    const Se3 E = se3_exp(rot);
    double Rn[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            Rn[3 * i + j] = E.R[3 * i] * T.R[j] + E.R[3 * i + 1] * T.R[3 + j] + E.R[3 * i + 2] * T.R[6 + j];
    for (int k = 0; k < 9; ++k) T.R[k] = Rn[k];
}

// phase 0: start cost of a level (cost-only partials) -> hist[0]; resets the level's state.
// phase 1: one Gauss-Newton iteration from normal-equation partials: solve, update the pose (rot_only: H[3:6,3:6] dphi =
//          b[3:6], R <- exp(dphi) R, t unchanged; else R <- exp(dx[3:6]) R, t += dx[0:3]); without a line search the
//          cost of the linearisation point is the iteration's cost and the stopping rule runs here.
// phase 2: cost after the step (linesearch) -> the stopping rule.
// The stopping rule is Problem.solve's (ps_stop_rule.h: ps_stop_step).  level_out: [iterations, failed, hist...]
__global__ __launch_bounds__(256) void k_dense_finish(int nparts, const double* __restrict__ partials, int phase, int rot_only,
                                                       ps_solve_options o, double* __restrict__ pose, DenseSolveState* __restrict__ st,
                                                       double* __restrict__ level_out)
{
    if (phase != 0 && st->done) return;
    if (phase == 0 && st->failed) { if (threadIdx.x == 0) st->done = 1; return; }
    __shared__ double sp[8][PS_PHOTO_NACC];
    __shared__ double tot[PS_PHOTO_NACC];
    const int k = threadIdx.x & 31, g = threadIdx.x >> 5;
    double v = 0.0;
    for (int p = g; p < nparts; p += 8) v += partials[(size_t)p * PS_PHOTO_NACC + k];
    sp[g][k] = v;
    __syncthreads();
    if (threadIdx.x < PS_PHOTO_NACC) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += sp[q][k];
        tot[k] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double* hist = level_out + 2;
    if (phase == 0) {
        st->done = 0;
        ps_stop_begin(&st->stop, tot[27]);
        hist[0] = tot[27];
        level_out[0] = 0.0; level_out[1] = 0.0;
        return;
    }
    double c;
    if (phase == 1) {
        if (tot[28] < 6.0) { st->failed = 1; st->done = 1; level_out[1] = 1.0; return; }
        double H[6][6], b[6], dx[6];
        const int off = rot_only ? 3 : 0, n = rot_only ? 3 : 6;
        int idx = 0;
        for (int r = 0; r < 6; ++r)
            for (int c2 = r; c2 < 6; ++c2) {
                if (r >= off && c2 >= off) { H[r - off][c2 - off] = tot[idx]; H[c2 - off][r - off] = tot[idx]; }
                ++idx;
            }
        for (int r = 0; r < n; ++r) b[r] = tot[21 + off + r];
        if (!dense_chol_solve(H, b, n, dx)) { st->failed = 2; st->done = 1; level_out[1] = 2.0; return; }
        Se3 T = se3_load(pose);
        double nrm = 0.0;
        for (int r = 0; r < n; ++r) nrm += dx[r] * dx[r];
        st->dx_norm = sqrt(nrm);
        if (rot_only) {
            dense_rotate(T, dx);
        } else {
            dense_rotate(T, dx + 3);
            for (int r = 0; r < 3; ++r) T.t[r] = T.t[r] + dx[r];
        }
        se3_store(pose, T);
        if (o.linesearch) return;
        c = tot[27];
    } else {
        c = tot[27];
    }
    const int f = ps_stop_step(&o, &st->stop, c, st->dx_norm);
    hist[st->stop.iters] = c;
    level_out[0] = (double)st->stop.iters;
    if (f & PS_STOP_KEEP_BEST)
        for (int q = 0; q < 12; ++q) st->best[q] = pose[q];
    if (f & PS_STOP_RESTORE_BEST)
        for (int q = 0; q < 12; ++q) pose[q] = st->best[q];
    st->done = f & PS_STOP_DONE;
}
