// ps_k_triang.h -- multi-view triangulation of landmarks from their observations and the current poses (ps_triangulate).
// Part of ps_core.hip (one translation unit; included after ps_kernels.h).
//
// 16 lanes per landmark over the observation slots of the landmark-sorted tables (k_cov_landmarks' mapping): lane `sub` takes
// observations sub, sub + 16, ... of the landmark in slot order, every sum is reduced in a fixed order (group16_sum), so repeated
// calls are bit-identical.  No atomics.  Per landmark (pyslam_amd/triangulation.py is the same definition in numpy):
//
//   1. Linear start.  With x_n = (u - cu) / fu, y_n = (v - cv) / fv and the observing pose (R | t), rows r1 r2 r3, every
//      observation gives the two rows   (x_n r3 - r1) p = -(x_n t3 - t1),   (y_n r3 - r2) p = -(y_n t3 - t2);   an observation
//      that bears depth (stereo: z = fu b / d, RGB-D: z = d) a third,   r3 p = z - t3.   The 3 x 3 normal equations
//      A p = g (A = sum a^T a, g = sum a^T rhs) are solved by Cholesky.
//   2. `refine_iters` Gauss-Newton steps on the landmark's own robust reprojection cost, every pose held, through the solver's
//      evaluator (reproj_eval_obs<false, true>: camera types, stiffness and IRLS weights are the solver's):
//      H = sum J~l^T J~l, g = sum J~l^T r~, H dx = -g by Cholesky.  A step that does not lower the cost is not taken and ends
//      that landmark's iteration; so does a step whose system cannot be solved (a pivot that is not positive, NaN: under L1
//      the IRLS weight of a residual component within PS_SMALL_ANGLE of zero is NaN, which is where a converging landmark
//      ends up).  Either way the landmark keeps its last accepted point and its status.
//   3. Status: 0 ok | 1 fewer than two observations, none bearing depth | 2 no depth and the largest angle between two
//      viewing rays below the minimum parallax, or normal equations of the linear start that are not positive definite |
//      3 the result lies behind one of its cameras (z <= 0).  A landmark with a non-zero status keeps its old value.
#pragma once

enum { PS_TRI_OK = 0, PS_TRI_FEW_OBS = 1, PS_TRI_DEGENERATE = 2, PS_TRI_BEHIND = 3 };

// x = A^-1 rhs for the symmetric A = (a00, a10, a11, a20, a21, a22) by Cholesky, IEEE roots and quotients; false (x untouched
// beyond rounding noise) when a pivot is not positive (NaN included)
PS_DEV bool tri_chol_solve(const double* __restrict__ A, const double* __restrict__ rhs, double* __restrict__ x) {
#pragma clang fp contract(off)
    if (!(A[0] > 0.0)) return false;
    const double l00 = sqrt(A[0]);
    const double l10 = A[1] / l00, l20 = A[3] / l00;
    const double d1 = A[2] - l10 * l10;
    if (!(d1 > 0.0)) return false;
    const double l11 = sqrt(d1);
    const double l21 = (A[4] - l20 * l10) / l11;
    const double d2 = A[5] - l20 * l20 - l21 * l21;
    if (!(d2 > 0.0)) return false;
    const double l22 = sqrt(d2);
    const double y0 = rhs[0] / l00;
    const double y1 = (rhs[1] - l10 * y0) / l11;
    const double y2 = (rhs[2] - l20 * y0 - l21 * y1) / l22;
    x[2] = y2 / l22;
    x[1] = (y1 - l21 * x[2]) / l11;
    x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
    return true;
}

PS_DEV double group16_min(double v) {           // every lane of the 16-lane group gets the minimum (order does not matter)
#pragma unroll
    for (int off = 8; off; off >>= 1) v = fmin(v, __shfl_xor(v, off, 16));
    return v;
}

// unit viewing ray of observation `o` in the world frame: R^T (x_n, y_n, 1) / |.|
PS_DEV void tri_ray(const LObs& o, const double* __restrict__ poses, const ObsGroup* __restrict__ groups, double* __restrict__ ray) {
#pragma clang fp contract(off)
    const ObsGroup& g = groups[PS_GRP_OF(o)];
    const double* R = poses + 12 * (size_t)PS_POSE_OF(o);
    const double xn = (o.u - g.cu) / g.fu, yn = (o.v - g.cv) / g.fv;
    const double nrm = sqrt(xn * xn + yn * yn + 1.0);
#pragma unroll
    for (int j = 0; j < 3; ++j) ray[j] = (R[j] * xn + R[3 + j] * yn + R[6 + j]) / nrm;
}

template <bool WIDE>
__global__ __launch_bounds__(256) void k_triangulate(
    int n, const int32_t* __restrict__ slots /* NULL: group k takes slot k */, const int32_t* __restrict__ lm_ptr,
    const int32_t* __restrict__ lm_point, const LObs* __restrict__ lobs, const double* __restrict__ poses,
    double* __restrict__ points, const ObsGroup* __restrict__ groups, ObsWide wide, int refine_iters, double cos_min_parallax,
    int write_back, double* __restrict__ out_points, int32_t* __restrict__ out_status)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x * (blockDim.x / PS_LM_GROUP) + threadIdx.x / PS_LM_GROUP;
    const int sub = threadIdx.x & (PS_LM_GROUP - 1);
    const bool live = k < n;                               // whole 16-lane groups are live or not
    const int v = live ? (slots ? slots[k] : k) : 0;
    const int b = live ? lm_ptr[v] : 0, e = live ? lm_ptr[v + 1] : 0;

    // ---- 1. linear start
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g3[3] = {0.0, 0.0, 0.0}, ndepth = 0.0;
    for (int i = b + sub; i < e; i += PS_LM_GROUP) {
        const LObs o = lobs[i];
        const ObsGroup& g = groups[PS_GRP_OF(o)];
        const double* T = poses + 12 * (size_t)PS_POSE_OF(o);
        const double xn = (o.u - g.cu) / g.fu, yn = (o.v - g.cv) / g.fv;
        double a[3], rhs = 0.0;
        const bool depth = g.cam_type != 2;
        for (int row = 0; row < 3; ++row) {
            if (row == 2 && !depth) break;
            if (row == 0) { a[0] = xn * T[6] - T[0]; a[1] = xn * T[7] - T[1]; a[2] = xn * T[8] - T[2]; rhs = -(xn * T[11] - T[9]); }
            else if (row == 1) { a[0] = yn * T[6] - T[3]; a[1] = yn * T[7] - T[4]; a[2] = yn * T[8] - T[5]; rhs = -(yn * T[11] - T[10]); }
            else {
                const double z = g.cam_type == 1 ? o.d : g.fu * g.b / o.d;
                a[0] = T[6]; a[1] = T[7]; a[2] = T[8]; rhs = z - T[11];
            }
            A[0] += a[0] * a[0]; A[1] += a[1] * a[0]; A[2] += a[1] * a[1];
            A[3] += a[2] * a[0]; A[4] += a[2] * a[1]; A[5] += a[2] * a[2];
            g3[0] += a[0] * rhs; g3[1] += a[1] * rhs; g3[2] += a[2] * rhs;
        }
        if (depth) ndepth += 1.0;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) A[q] = group16_sum(A[q]);
#pragma unroll
    for (int q = 0; q < 3; ++q) g3[q] = group16_sum(g3[q]);
    ndepth = group16_sum(ndepth);

    int status = PS_TRI_OK;
    if (e - b < 2 && ndepth == 0.0) status = PS_TRI_FEW_OBS;
    // the largest angle between two viewing rays = the smallest cosine over all pairs: lane `sub` holds its observations
    // against every observation of the landmark (only landmarks without depth; a handful of rays from cache)
    double min_cos = 1.0;
    if (live && ndepth == 0.0 && status == PS_TRI_OK) {
        for (int i = b + sub; i < e; i += PS_LM_GROUP) {
            double ri[3];
            tri_ray(lobs[i], poses, groups, ri);
            for (int j = b; j < e; ++j) {
                double rj[3];
                tri_ray(lobs[j], poses, groups, rj);
                min_cos = fmin(min_cos, ri[0] * rj[0] + ri[1] * rj[1] + ri[2] * rj[2]);
            }
        }
    }
    min_cos = group16_min(min_cos);
    if (status == PS_TRI_OK && ndepth == 0.0 && min_cos > cos_min_parallax) status = PS_TRI_DEGENERATE;
    double p[3] = {0.0, 0.0, 0.0};
    if (status == PS_TRI_OK && !tri_chol_solve(A, g3, p)) status = PS_TRI_DEGENERATE;

    // ---- 2. Gauss-Newton on the landmark's own cost, poses held: evaluation 0 is at the linear start, evaluation it > 0 at the
    // candidate p + dx, which is accepted only if it lowers the cost.  Every lane of the wave runs every round (the sums are
    // row operations); a landmark that is done stops evaluating.
    bool active = live && status == PS_TRI_OK;
    double cost = 0.0, H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gr[3] = {0.0, 0.0, 0.0}, behind = 0.0;
    double cand[3] = {p[0], p[1], p[2]};
    for (int it = 0; it <= refine_iters; ++it) {
        double c = 0.0, Hn[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gn[3] = {0.0, 0.0, 0.0}, bh = 0.0;
        if (active) {
            for (int i = b + sub; i < e; i += PS_LM_GROUP) {
                const LObs o = lobs[i];
                const Se3 T = se3_load(poses + 12 * (size_t)PS_POSE_OF(o));
                ReprojEval ev;
                reproj_eval_obs<false, true, WIDE>(T, cand, &o.u, groups, PS_GRP_OF(o), wide, i, ev);
                c += ev.cost;
                if (!(ev.pc[2] > 0.0)) bh += 1.0;
                const double* J = ev.Jl;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    Hn[0] += J[3 * r] * J[3 * r];
                    Hn[1] += J[3 * r + 1] * J[3 * r];
                    Hn[2] += J[3 * r + 1] * J[3 * r + 1];
                    Hn[3] += J[3 * r + 2] * J[3 * r];
                    Hn[4] += J[3 * r + 2] * J[3 * r + 1];
                    Hn[5] += J[3 * r + 2] * J[3 * r + 2];
                    gn[0] += J[3 * r] * ev.r[r];
                    gn[1] += J[3 * r + 1] * ev.r[r];
                    gn[2] += J[3 * r + 2] * ev.r[r];
                }
            }
        }
        c = group16_sum(c);
        bh = group16_sum(bh);
#pragma unroll
        for (int q = 0; q < 6; ++q) Hn[q] = group16_sum(Hn[q]);
#pragma unroll
        for (int q = 0; q < 3; ++q) gn[q] = group16_sum(gn[q]);
        if (active) {
            if (it == 0 || c < cost) {
                cost = c; behind = bh;
#pragma unroll
                for (int q = 0; q < 3; ++q) { p[q] = cand[q]; gr[q] = gn[q]; }
#pragma unroll
                for (int q = 0; q < 6; ++q) H[q] = Hn[q];
            } else active = false;                          // the step did not lower the cost: not taken, this landmark is done
        }
        if (active && it < refine_iters) {
            double dx[3];
            const double mg[3] = {-gr[0], -gr[1], -gr[2]};
            if (tri_chol_solve(H, mg, dx)) { cand[0] = p[0] + dx[0]; cand[1] = p[1] + dx[1]; cand[2] = p[2] + dx[2]; }
            else active = false;                            // no step to try (pivot not positive, NaN): done, like a step not taken
        }
    }
    if (status == PS_TRI_OK && behind > 0.0) status = PS_TRI_BEHIND;
    if (!live || sub != 0) return;
    double* pt = points + 3 * (size_t)lm_point[v];
    if (status != PS_TRI_OK) { p[0] = pt[0]; p[1] = pt[1]; p[2] = pt[2]; }
    else if (write_back) { pt[0] = p[0]; pt[1] = p[1]; pt[2] = p[2]; }
    out_points[3 * (size_t)k] = p[0]; out_points[3 * (size_t)k + 1] = p[1]; out_points[3 * (size_t)k + 2] = p[2];
    out_status[k] = status;
}
