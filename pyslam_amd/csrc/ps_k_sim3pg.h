// ps_k_sim3pg.h -- kernels of the Sim(3) pose graph (host driver: ps_host_sim3pg.h, C ABI: ps_abi_sim3pg.h; definition: DESIGN.md
// section 7, restated by pyslam_amd/liegroups/sim3.py and pyslam_amd/pipelines/simgraph.py).  A stand-alone handle: nothing of
// the core's D = 3 / 6 machinery is touched.  fp64 throughout, no atomics: every sum runs in a fixed order.
//
// Element: 13 doubles [R row-major (9) | t (3) | s], p -> s R p + t.  Tangent [rho | phi | sigma].  Edge (i, j, S_ji, W):
// r = W log(S_j S_i^-1 S_ji^-1), J_i = -W Ad(S_j S_i^-1), J_j = W (first order), IRLS per component through s3g_loss_weight
// (ps_loss_weight with L1's weight capped at 1 / PS_SMALL_ANGLE).
#pragma once

#define PS_S3G_EDGES 64                // edges per workgroup of k_s3g_edges
#define PS_S3G_ROW 161                 // scratch row [H11 | H12 | H22 | g1 | g2]
#define PS_S3G_DBG 105                 // debug tap row [r~ | J~1 | J~2]
#define PS_S3G_SERIES_TERMS 22
#define PS_S3G_TINY 1e-8

struct Sim3g { double R[9]; double t[3]; double s; };

PS_DEV Sim3g s3g_load(const double* __restrict__ p) {
    Sim3g S;
#pragma unroll
    for (int i = 0; i < 9; ++i) S.R[i] = p[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) S.t[i] = p[9 + i];
    S.s = p[12];
    return S;
}

PS_DEV void s3g_store(double* __restrict__ p, const Sim3g& S) {
#pragma unroll
    for (int i = 0; i < 9; ++i) p[i] = S.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[9 + i] = S.t[i];
    p[12] = S.s;
}

PS_DEV Sim3g s3g_inv(const Sim3g& S) {             // (1 / s, R^T, -R^T t / s)
    Sim3g o;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o.R[3 * i + j] = S.R[3 * j + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = -(o.R[3 * i] * S.t[0] + o.R[3 * i + 1] * S.t[1] + o.R[3 * i + 2] * S.t[2]) / S.s;
    o.s = 1.0 / S.s;
    return o;
}

PS_DEV Sim3g s3g_mul(const Sim3g& A, const Sim3g& B) {   // (s_a s_b, R_a R_b, s_a R_a t_b + t_a)
    Sim3g o;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) o.R[3 * i + j] = A.R[3 * i] * B.R[j] + A.R[3 * i + 1] * B.R[3 + j] + A.R[3 * i + 2] * B.R[6 + j];
        o.t[i] = A.s * (A.R[3 * i] * B.t[0] + A.R[3 * i + 1] * B.t[1] + A.R[3 * i + 2] * B.t[2]) + A.t[i];
    }
    o.s = A.s * B.s;
    return o;
}

// sin(theta) / theta and (1 - cos(theta)) / theta^2
PS_DEV void s3g_h12(double theta, double& h1, double& h2) {
    if (theta <= PS_S3G_TINY) { h1 = 1.0; h2 = 0.5; return; }
    const double half = 0.5 * theta, sh = sin(half) / half;
    h1 = sin(theta) / theta;
    h2 = 0.5 * sh * sh;
}

// (A, B, C) of W(phi, sigma) = A I + B phi^ + C phi^^2 = int_0^1 e^(tau sigma) Exp(tau phi) dtau: the power series of (e^z - 1) / z,
// z = sigma + i theta, inside |z|^2 <= 1 (real recurrences, no division: exact at theta = 0, sigma = 0 and both), closed forms
// outside, arranged so that a small theta beside a large sigma (or the reverse) cancels nothing.
PS_DEV void sim3_w_coef(double theta, double sigma, double& A, double& B, double& C) {
    const double th2 = theta * theta, z2 = sigma * sigma + th2;
    if (z2 <= 1.0) {
        double a = 1.0, p = 0.0, q = 0.0, sn = 1.0, inv_fact = 1.0;
        A = 1.0; B = 0.0; C = 0.0;
        for (int n = 1; n <= PS_S3G_SERIES_TERMS; ++n) {
            const double pn = sigma * p + a, qn = sigma * q + p;
            p = pn; q = qn;
            sn *= sigma;
            a = sn - th2 * q;
            inv_fact /= (double)(n + 1);
            A += sn * inv_fact;
            B += p * inv_fact;
            C += q * inv_fact;
        }
        return;
    }
    const double E = exp(sigma);
    A = sigma != 0.0 ? expm1(sigma) / sigma : 1.0;
    double h1, h2;
    s3g_h12(theta, h1, h2);
    B = (sigma * (E * h1 - A) + E * th2 * h2) / z2;
    C = (sigma * E * h2 + A - E * h1) / z2;
}

// W as a 3 x 3 matrix (row-major)
PS_DEV void s3g_w_matrix(const double* __restrict__ phi, double sigma, double* __restrict__ Wm) {
    const double x = phi[0], y = phi[1], z = phi[2];
    double A, B, C;
    sim3_w_coef(sqrt(x * x + y * y + z * z), sigma, A, B, C);
    // phi^^2 = phi phi^T - theta^2 I
    const double xx = x * x, yy = y * y, zz = z * z;
    Wm[0] = A - C * (yy + zz); Wm[1] = -B * z + C * x * y;  Wm[2] = B * y + C * x * z;
    Wm[3] = B * z + C * x * y;  Wm[4] = A - C * (xx + zz); Wm[5] = -B * x + C * y * z;
    Wm[6] = -B * y + C * x * z; Wm[7] = B * x + C * y * z;  Wm[8] = A - C * (xx + yy);
}

PS_DEV Sim3g sim3_exp(const double* __restrict__ xi) {
    Sim3g S;
    const double x = xi[3], y = xi[4], z = xi[5];
    double h1, h2;
    s3g_h12(sqrt(x * x + y * y + z * z), h1, h2);
    const double xx = x * x, yy = y * y, zz = z * z;
    S.R[0] = 1.0 - h2 * (yy + zz); S.R[1] = -h1 * z + h2 * x * y;  S.R[2] = h1 * y + h2 * x * z;
    S.R[3] = h1 * z + h2 * x * y;  S.R[4] = 1.0 - h2 * (xx + zz); S.R[5] = -h1 * x + h2 * y * z;
    S.R[6] = -h1 * y + h2 * x * z; S.R[7] = h1 * x + h2 * y * z;  S.R[8] = 1.0 - h2 * (xx + yy);
    double Wm[9];
    s3g_w_matrix(xi + 3, xi[6], Wm);
#pragma unroll
    for (int i = 0; i < 3; ++i) S.t[i] = Wm[3 * i] * xi[0] + Wm[3 * i + 1] * xi[1] + Wm[3 * i + 2] * xi[2];
    S.s = exp(xi[6]);
    return S;
}

// xi = [W^-1 t | phi | log s]; rotation angles below pi (the angle from atan2: accurate at both ends)
PS_DEV void sim3_log(const Sim3g& S, double* __restrict__ xi) {
    const double* R = S.R;
    const double v0 = R[7] - R[5], v1 = R[2] - R[6], v2 = R[3] - R[1];
    const double sn = 0.5 * sqrt(v0 * v0 + v1 * v1 + v2 * v2);
    const double cs = 0.5 * (R[0] + R[4] + R[8]) - 0.5;
    const double f = sn <= PS_S3G_TINY ? 0.5 : 0.5 * atan2(sn, cs) / sn;
    xi[3] = f * v0; xi[4] = f * v1; xi[5] = f * v2;
    xi[6] = log(S.s);
    double m[9];
    s3g_w_matrix(xi + 3, xi[6], m);
    // rho = W^-1 t by cofactors (W is regular for angles below 2 pi)
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02, id = 1.0 / det;
    const double* t = S.t;
    xi[0] = id * (c00 * t[0] + (m[2] * m[7] - m[1] * m[8]) * t[1] + (m[1] * m[5] - m[2] * m[4]) * t[2]);
    xi[1] = id * (c01 * t[0] + (m[0] * m[8] - m[2] * m[6]) * t[1] + (m[2] * m[3] - m[0] * m[5]) * t[2]);
    xi[2] = id * (c02 * t[0] + (m[1] * m[6] - m[0] * m[7]) * t[1] + (m[0] * m[4] - m[1] * m[3]) * t[2]);
}

// entry (m, c) of Ad(S) = [[s R, t^ R, -t], [0, R, 0], [0, 0, 1]] from an element in memory
PS_DEV double sim3_adj(const double* __restrict__ S, int m, int c) {
    if (m < 3) {
        if (c < 3) return S[12] * S[3 * m + c];
        if (c == 6) return -S[9 + m];
        const int q = c - 3, m1 = m == 2 ? 0 : m + 1, m2 = m == 0 ? 2 : m - 1;
        return S[9 + m1] * S[3 * m2 + q] - S[9 + m2] * S[3 * m1 + q];
    }
    if (m < 6) return (c >= 3 && c < 6) ? S[3 * (m - 3) + (c - 3)] : 0.0;
    return c == 6 ? 1.0 : 0.0;
}

// The IRLS weight of a residual component in this graph: ps_loss_weight, except that L1's 1 / |r| is capped at
// 1 / PS_SMALL_ANGLE (ps_loss_weight says NaN there; its other users keep that).  Zero components are structural here: every
// odometry and covisibility edge of a loop correction is measured from the current estimates, and zero is where an L1 solve
// converges to -- the capped weight is the usual IRLS regularisation.  Above PS_SMALL_ANGLE the bits are ps_loss_weight's;
// the cost stays |r|.
PS_DEV double s3g_loss_weight(int id, double k, double x) {
    if (id == PS_LOSS_L1) return 1.0 / fmax(fabs(x), PS_SMALL_ANGLE);
    return ps_loss_weight(id, k, x);
}

// Two phases per workgroup of 64 edges, as k_factor_pass has them (one logarithm per edge, not 64 copies of it):
//   1. one THREAD per edge: S_j S_i^-1, E = that times S_ji^-1, xi = log(E), r = W xi, the IRLS scales, the edge's cost;
//   2. one WAVE per edge, lane (r, c) of 49: J~1 = -diag(s) W Ad(S_j S_i^-1), J~2 = diag(s) W in LDS, then the three 7 x 7 products
//      and the two gradient pieces into the edge's scratch row.
// cost_part[workgroup]: the sum of its edges' costs, in edge order.  cost_only: phase 1 alone.
__global__ __launch_bounds__(256) void k_s3g_edges(
    int ne, const int32_t* __restrict__ e_i, const int32_t* __restrict__ e_j, const double* __restrict__ e_obsinv,
    const double* __restrict__ e_W /* 49 per edge, or nullptr: identity */, int loss_id, double loss_k,
    const double* __restrict__ verts, double* __restrict__ scratch, double* __restrict__ cost_part,
    double* __restrict__ dbg /* parity tap or nullptr: [r~ | J~1 | J~2] per edge */, int cost_only)
{
    constexpr int D = 7, DD = 49, EPB = PS_S3G_EDGES;
    __shared__ double sS[EPB][D], sSr[EPB][D], sT21[EPB][13];
    __shared__ double sJ1[4][DD], sJ2[4][DD];
    const int e0 = blockIdx.x * EPB;
    if (threadIdx.x < EPB) {                                  // (the whole first wave)
        const int el = threadIdx.x, e = e0 + el;
        double cst = 0.0;
        if (e < ne) {
            const Sim3g Sj = s3g_load(verts + 13 * (size_t)e_j[e]);
            const Sim3g Sii = s3g_inv(s3g_load(verts + 13 * (size_t)e_i[e]));
            const Sim3g T21 = s3g_mul(Sj, Sii);
            const Sim3g E = s3g_mul(T21, s3g_load(e_obsinv + 13 * (size_t)e));
            double xi[D];
            sim3_log(E, xi);
            const double* Wm = e_W ? e_W + (size_t)e * DD : nullptr;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                double rk = xi[k];
                bool present = true;                          // an all-zero stiffness row is an absent residual row
                if (Wm) {
                    rk = 0.0; present = false;
#pragma unroll
                    for (int m = 0; m < D; ++m) { rk += Wm[k * D + m] * xi[m]; present = present || Wm[k * D + m] != 0.0; }
                }
                const double sk = present ? sqrt(s3g_loss_weight(loss_id, loss_k, rk)) : 0.0;
                if (present) cst += ps_loss_rho(loss_id, loss_k, rk);
                sS[el][k] = sk;
                sSr[el][k] = sk * rk;
            }
            s3g_store(sT21[el], T21);
        }
        cst = wave_sum(cst);
        if (threadIdx.x == 0) cost_part[blockIdx.x] = cst;
    }
    if (cost_only) return;
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool act = lane < DD;
    const int r = act ? lane / D : 0, c = act ? lane - (lane / D) * D : 0;
    for (int q = 0; q < EPB / 4; ++q) {
        const int el = w * (EPB / 4) + q, e = e0 + el;
        if (e >= ne) break;                                   // (uniform per wave)
        const double* Wm = e_W ? e_W + (size_t)e * DD : nullptr;
        if (act) {
            const double sk = sS[el][r];
            double j1 = 0.0;
            if (Wm) {
#pragma unroll
                for (int m = 0; m < D; ++m) j1 -= Wm[r * D + m] * sim3_adj(sT21[el], m, c);
            } else {
                j1 = -sim3_adj(sT21[el], r, c);
            }
            sJ1[w][lane] = sk * j1;
            sJ2[w][lane] = sk * (Wm ? Wm[lane] : (r == c ? 1.0 : 0.0));
        }
        __builtin_amdgcn_wave_barrier();
        if (dbg != nullptr && act) {                          // (uniform: production launches pass nullptr)
            double* o = dbg + (size_t)e * PS_S3G_DBG;
            if (lane < D) o[lane] = sSr[el][lane];
            o[D + lane] = sJ1[w][lane];
            o[D + DD + lane] = sJ2[w][lane];
        }
        if (act) {
            double h11 = 0.0, h12 = 0.0, h22 = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                h11 += sJ1[w][k * D + r] * sJ1[w][k * D + c];
                h12 += sJ1[w][k * D + r] * sJ2[w][k * D + c];
                h22 += sJ2[w][k * D + r] * sJ2[w][k * D + c];
            }
            double* out = scratch + (size_t)e * PS_S3G_ROW;
            out[lane] = h11; out[DD + lane] = h12; out[2 * DD + lane] = h22;
            if (c == 0) {
                double g1 = 0.0, g2 = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) { g1 -= sJ1[w][k * D + r] * sSr[el][k]; g2 -= sJ2[w][k * D + r] * sSr[el][k]; }
                out[3 * DD + r] = g1; out[3 * DD + D + r] = g2;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// The dense system from the scratch rows, one thread per entry of the n x n matrix (n = 7 free vertices): a touched 7 x 7 block
// sums its slot list (built once on the host: edge order, an edge whose vertices run against the block's order transposed), the
// upper triangle from the mirrored block in the same order -- H is symmetric to the bit; every other entry is written as zero in
// the same launch (no memset, no read-modify-write).  H: undamped; A: diagonal times (1 + lambda), what the factorisation
// consumes.  The first n threads also sum g.
__global__ __launch_bounds__(256) void k_s3g_assemble(
    int n, int nfree, const int32_t* __restrict__ blockmap /* nfree x nfree, lower triangle: slot or -1 */,
    const int32_t* __restrict__ eptr, const int2* __restrict__ eitems /* (scratch offset, transpose) */,
    const int32_t* __restrict__ gptr, const int32_t* __restrict__ gitems, const double* __restrict__ scratch, double lambda,
    double* __restrict__ H, double* __restrict__ A, double* __restrict__ g)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)n * n) return;
    const int i = (int)(t / n), j = (int)(t - (long)i * n);
    int bi = i / 7, r = i - bi * 7, bj = j / 7, c = j - bj * 7;
    if (bi < bj) { int tmp = bi; bi = bj; bj = tmp; tmp = r; r = c; c = tmp; }
    const int slot = blockmap[(size_t)bi * nfree + bj];
    double v = 0.0;
    if (slot >= 0) {
        for (int k = eptr[slot]; k < eptr[slot + 1]; ++k) {
            const int2 it = eitems[k];
            v += scratch[(size_t)it.x + (it.y ? c * 7 + r : r * 7 + c)];
        }
    }
    H[t] = v;
    A[t] = i == j ? v * (1.0 + lambda) : v;
    if (t < n) {
        const int rid = (int)t / 7, rr = (int)t - rid * 7;
        double s = 0.0;
        for (int k = gptr[rid]; k < gptr[rid + 1]; ++k) s += scratch[(size_t)gitems[k] + rr];
        g[t] = s;
    }
}

// out[0] = sum of part[0 .. np) in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void k_s3g_sum(int np, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double lds[16];
    double s = 0.0;
    for (int k = threadIdx.x; k < np; k += 256) s += part[k];
    s = block_sum(s, lds);
    if (threadIdx.x == 0) out[0] = s;
}

// the residual k_spd_residual left of the UNDAMPED system made the damped system's: r_i -= lambda H_ii x_i; out = {r.r, b.b}
// (one workgroup, fixed order)
__global__ __launch_bounds__(256) void k_s3g_resid_fin(int n, const double* __restrict__ H, double lambda, const double* __restrict__ x,
                                                       const double* __restrict__ b, double* __restrict__ r, double* __restrict__ out) {
    __shared__ double lds[32];
    double rr = 0.0, bb = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double ri = r[i] - lambda * H[(size_t)i * n + i] * x[i], bi = b[i];
        r[i] = ri;
        rr += ri * ri; bb += bi * bi;
    }
    block_sum2(rr, bb, lds);
    if (threadIdx.x == 0) { out[0] = rr; out[1] = bb; }
}

// S_v <- exp(dx_rid) S_v for the free vertices; part[workgroup] = its share of ||dx||^2.  Nothing moves behind a failed factor.
__global__ __launch_bounds__(256) void k_s3g_retract(int nfree, const int32_t* __restrict__ free_vid, const double* __restrict__ x,
                                                     const int32_t* __restrict__ stat, double* __restrict__ verts,
                                                     double* __restrict__ part) {
    __shared__ double lds[16];
    if (stat[ST_DIAG_FAIL]) return;                           // (uniform)
    const int rid = blockIdx.x * blockDim.x + threadIdx.x;
    double sq = 0.0;
    if (rid < nfree) {
        double xi[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) { xi[k] = x[(size_t)rid * 7 + k]; sq += xi[k] * xi[k]; }
        double* p = verts + 13 * (size_t)free_vid[rid];
        s3g_store(p, s3g_mul(sim3_exp(xi), s3g_load(p)));
    }
    sq = block_sum(sq, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = sq;
}

// test entry: the device functions on a table of tangent vectors
__global__ __launch_bounds__(256) void k_s3g_explog(int n, const double* __restrict__ xi_in, double* __restrict__ S13,
                                                    double* __restrict__ xi_back, double* __restrict__ adj49) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    double xi[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) xi[k] = xi_in[(size_t)t * 7 + k];
    const Sim3g S = sim3_exp(xi);
    s3g_store(S13 + 13 * (size_t)t, S);
    sim3_log(S, xi);
#pragma unroll
    for (int k = 0; k < 7; ++k) xi_back[(size_t)t * 7 + k] = xi[k];
    for (int m = 0; m < 7; ++m)
        for (int c = 0; c < 7; ++c) adj49[(size_t)t * 49 + m * 7 + c] = sim3_adj(S13 + 13 * (size_t)t, m, c);
}
