// ps_k_bjfactor.h -- the block-Jacobi factor of ONE reduced pose by ONE wave: what k_block_jacobi_factor (ps_k_cg_fused.h) runs per
// wave, and what the finalising waves of k_schur_pairs_db (ps_k_schur2.h) go on with for the diagonal block they have just
// written (option "setup_ride": the factor kernel leaves the reduced solve's dependent chain).  Both routes call this one
// function, so they run the same instruction sequence on the same values.
// Part of ps_kernels.h (included from there, in this order; not a stand-alone header).
#pragma once

// where the factors of a pose go (Linv == NULL in the pair launch: nothing rides)
struct BjFactorOut {
    double* Linv;
    int32_t* status;
    // fused CG only (r0 != NULL): also the start vectors of the scaled system, r = Linv g, w = s = p = x = 0
    double *r0, *w0, *s0, *p0, *x0;
    // two-level CG (Bmat != NULL): the coarse basis block of this pose, B_i = L_i^T Ad(T_i) (basis 1: a
    // coarse unknown is a BODY-frame twist eta, the fine correction is x_i = Ad(T_i) eta, x^_i = L_i^T x_i)
    // or the identity (basis 0: hats directly in the scaled coordinates), and bg_i = B_i^T r_i
    const double* poses;
    const int32_t* pose_of_rid;
    int basis;
    double* Bmat;
    double* bg;
};

#define PS_BJF_SCRATCH(D) (3 * (D) * (D) + 2 * (D))       // doubles of LDS scratch per wave: A | Li | B | r | g

// Lane (r, c) of the D x D block: the factorisation is a right-looking Cholesky with one column scaled and one rank-1 update
// applied per step by all lanes at once, the inverse six independent forward substitutions -- a few hundred instructions per
// wave instead of the ~3 000 of one thread working through the whole block.
// a_in: this lane's entry of the diagonal block (lanes < D*D).  sc: PS_BJF_SCRATCH(D) doubles of LDS owned by this wave; with
// start vectors (o.r0) the caller has stored g_i to sc[3 D D + D ..) -- the wave barrier behind the store of A covers it.
template <int D>
PS_DEV void block_jacobi_factor_wave(int i, int lane, double a_in, double* sc, const BjFactorOut& o)
{
    constexpr int DD = D * D;
    double* A = sc;
    double* Li = sc + DD;
    double* sB = sc + 2 * DD;
    double* sR = sc + 3 * DD;
    const double* gl = sc + 3 * DD + D;
    const bool with_g = o.r0 != nullptr;
    if (with_g && i == 0 && lane == 0) { o.status[ST_PCG_DONE] = 0; o.status[ST_PCG_ITERS] = 0; }
    const bool act = lane < DD;
    const int r = act ? lane / D : 0, c = act ? lane % D : 0;
    if (act) { A[lane] = a_in; Li[lane] = 0.0; }
    __builtin_amdgcn_wave_barrier();
    bool ok = true;
    // A = L L^T in place: after step j column j of A (rows >= j) holds L[:, j]
#pragma unroll
    for (int j = 0; j < D; ++j) {
        const double d = A[j * D + j];
        ok = ok && (d > 0.0);
        const double l = sqrt(d);
        __builtin_amdgcn_wave_barrier();
        if (act && c == j && r >= j) A[lane] = (r == j) ? l : A[lane] / l;
        __builtin_amdgcn_wave_barrier();
        if (act && r > j && c > j) A[lane] -= A[r * D + j] * A[c * D + j];
        __builtin_amdgcn_wave_barrier();
    }
    // L^-1: lane c < D runs the forward substitution of column c
    if (lane < D) {
        const int cc = lane;
        double col[D];
#pragma unroll
        for (int rr = 0; rr < D; ++rr) {
            double v = (rr == cc) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < rr; ++k) v -= (k >= cc) ? A[rr * D + k] * col[k] : 0.0;
            col[rr] = (rr >= cc) ? v / A[rr * D + rr] : 0.0;
            Li[rr * D + cc] = col[rr];
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (!ok && lane == 0) atomicAdd(&o.status[ST_DIAG_FAIL], 1);
    if (act) o.Linv[(size_t)i * DD + lane] = Li[lane];
    if (with_g && lane < D) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) v += Li[lane * D + k] * gl[k];
        const size_t oo = (size_t)i * D + lane;
        o.r0[oo] = v; o.w0[oo] = 0.0; o.s0[oo] = 0.0; o.p0[oo] = 0.0; o.x0[oo] = 0.0;
        sR[lane] = v;
    }
    if (!o.Bmat) return;
    if (act) {
        typedef PoseOps<D> G;
        double v = (r == c) ? 1.0 : 0.0;
        if (o.basis == 1) {
            const double* Tp = o.poses + G::W * (size_t)o.pose_of_rid[i];      // (c differs per lane: entries straight from memory)
            v = 0.0;
#pragma unroll
            for (int m2 = 0; m2 < D; ++m2) v += (m2 >= r) ? A[m2 * D + r] * G::adj_mem(Tp, m2, c) : 0.0;     // (L^T Ad)[r][c]
        }
        o.Bmat[(size_t)i * DD + lane] = v;
        sB[lane] = v;
    }
    __builtin_amdgcn_wave_barrier();
    if (with_g && lane < D) {
        double v = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) v += sB[a * D + lane] * sR[a];
        o.bg[(size_t)i * D + lane] = v;
    }
}
