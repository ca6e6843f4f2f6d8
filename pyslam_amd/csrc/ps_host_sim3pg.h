// ps_host_sim3pg.h -- host driver of the Sim(3) pose graph (kernels: ps_k_sim3pg.h; C ABI: ps_abi_sim3pg.h).  Part of ps_core.hip
// (inside its extern "C" block, after ps_abi_sim3.h).  A stand-alone handle, as ps_photo, ps_dense and ps_feat are: its own
// tables, its own kernels, one stream.  The linear solve is SpdSolve (ps_host_bchol.h), as in ps_sparse_normal_direct:
// factor() is bchol_chain(BCHOL_FACTOR), solve_into() two k_spd_subst, residual() k_spd_residual on the unfactored copy, add()
// k_spd_axpy; one refinement step.
//
// One iteration, all on the handle's stream, one synchronisation at its end:
//   k_s3g_edges -> k_s3g_assemble (H undamped, A = H with its diagonal times 1 + lambda, g) -> factor A -> x = A^-1 g ->
//   r = g - (H + lambda diag H) x -> x += A^-1 r -> the residual once more (what relres reports) -> k_s3g_retract ->
//   k_s3g_edges, cost only, at the new point.

extern "C++" {
struct ps_sim3pg {
    hipStream_t stream = nullptr;
    int nv = 0, ne = 0, nfree = 0, n = 0, nwg = 0, nrt = 0, nslots = 0;
    int loss_id = 0;
    double loss_k = 0.0;
    DevMem mem{0, "ps_sim3pg: "};
    double *verts = nullptr, *verts_snap = nullptr, *e_obsinv = nullptr, *e_W = nullptr, *scratch = nullptr, *cost_part = nullptr;
    int32_t *e_i = nullptr, *e_j = nullptr, *free_vid = nullptr, *blockmap = nullptr, *eptr = nullptr, *gptr = nullptr, *gitems = nullptr;
    int2* eitems = nullptr;
    double *H = nullptr, *A = nullptr, *g = nullptr, *x = nullptr, *res = nullptr, *Tinv = nullptr, *res_part = nullptr, *dx_part = nullptr;
    double* out = nullptr;           // device: {cost at the linearisation point, cost after the step, ||dx||^2, r.r, b.b}
    int32_t* stat = nullptr;
    double* dbg = nullptr;           // the parity tap's rows, allocated by the first ps_sim3pg_debug_edges
    bool snap_valid = false;
    bool profiling = false;
    hipEvent_t ev[6] = {};
    double stage_ms[5] = {};         // edges, assemble, factor, substitute + refine, retract (+ the cost after): the last iteration's
    ~ps_sim3pg() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
};

namespace {
// the inverse of a similarity on the host, as s3g_inv has it
inline void s3g_host_inv(const double* S, double* o) {
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) o[3 * i + j] = S[3 * j + i];
    for (int i = 0; i < 3; ++i) o[9 + i] = -(o[3 * i] * S[9] + o[3 * i + 1] * S[10] + o[3 * i + 2] * S[11]) / S[12];
    o[12] = 1.0 / S[12];
}

inline bool s3g_finite(const double* p, size_t count) {
    for (size_t k = 0; k < count; ++k) if (!std::isfinite(p[k])) return false;
    return true;
}

inline int s3g_check_vertices(const double* v13, int nv, const char* who) {
    if (!s3g_finite(v13, (size_t)nv * 13)) return fail(std::string(who) + ": a vertex is not finite");
    for (int v = 0; v < nv; ++v) if (!(v13[13 * (size_t)v + 12] > 0.0)) return fail(std::string(who) + ": a vertex scale is not positive");
    return 0;
}

// the iteration-invariant lists of k_s3g_assemble: one slot per touched 7 x 7 block of the lower triangle (sorted by block
// row, then column), its items in edge order, an edge whose reduced indices run (row < column) transposed
int s3g_build_structure(ps_sim3pg* h, const std::vector<int32_t>& rid, const int32_t* ei, const int32_t* ej) {
    const int nf = h->nfree;
    std::map<std::pair<int, int>, std::vector<int2>> blocks;
    std::vector<std::vector<int32_t>> gl((size_t)nf);
    for (int e = 0; e < h->ne; ++e) {
        const int a = rid[ei[e]], b = rid[ej[e]];
        const int base = e * PS_S3G_ROW;
        if (a >= 0) { blocks[{a, a}].push_back(make_int2(base, 0)); gl[a].push_back(base + 147); }
        if (b >= 0) { blocks[{b, b}].push_back(make_int2(base + 98, 0)); gl[b].push_back(base + 154); }
        if (a >= 0 && b >= 0) {
            if (a > b) blocks[{a, b}].push_back(make_int2(base + 49, 0));      // H12 = J_i^T J_j is block (a, b)
            else blocks[{b, a}].push_back(make_int2(base + 49, 1));
        }
    }
    std::vector<int32_t> bm((size_t)nf * nf, -1), eptr(1, 0), gptr(1, 0), gitems;
    std::vector<int2> items;
    for (const auto& kv : blocks) {
        bm[(size_t)kv.first.first * nf + kv.first.second] = (int32_t)eptr.size() - 1;
        items.insert(items.end(), kv.second.begin(), kv.second.end());
        eptr.push_back((int32_t)items.size());
    }
    for (int r = 0; r < nf; ++r) { gitems.insert(gitems.end(), gl[r].begin(), gl[r].end()); gptr.push_back((int32_t)gitems.size()); }
    h->nslots = (int)eptr.size() - 1;
    DevMem& M = h->mem;
    if (M.upload(&h->blockmap, bm.data(), bm.size()) || M.upload(&h->eptr, eptr.data(), eptr.size()) ||
        M.upload(&h->eitems, items.data(), items.size()) || M.upload(&h->gptr, gptr.data(), gptr.size()) ||
        M.upload(&h->gitems, gitems.data(), gitems.size())) return -1;
    return 0;
}

inline void s3g_edges(ps_sim3pg* h, int cost_only, double* dbg) {
    if (h->ne > 0)
        hipLaunchKernelGGL(k_s3g_edges, dim3(h->nwg), dim3(256), 0, h->stream, h->ne, (const int32_t*)h->e_i, (const int32_t*)h->e_j,
                           (const double*)h->e_obsinv, (const double*)h->e_W, h->loss_id, h->loss_k, (const double*)h->verts, h->scratch,
                           h->cost_part, dbg, cost_only);
}

// cost at the current vertices into out[slot]
inline void s3g_cost(ps_sim3pg* h, int slot, bool edges_done) {
    if (!edges_done) s3g_edges(h, 1, nullptr);
    hipLaunchKernelGGL(k_s3g_sum, dim3(1), dim3(256), 0, h->stream, h->ne > 0 ? h->nwg : 0, (const double*)h->cost_part, h->out + slot);
}

inline int s3g_mark(ps_sim3pg* h, int k) {
    if (!h->profiling) return 0;
    if (!h->ev[k]) HIP_OK(hipEventCreate(&h->ev[k]));
    HIP_OK(hipEventRecord(h->ev[k], h->stream));
    return 0;
}

// edges, assemble, the cost of the linearisation point into out[0]
int s3g_linearize(ps_sim3pg* h, double lambda, double* dbg) {
    if (h->n <= 0) return fail("ps_sim3pg: every vertex is held, there is nothing to linearise");
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) return fail("ps_sim3pg: lambda must be finite and >= 0");
    if (s3g_mark(h, 0)) return -1;
    s3g_edges(h, 0, dbg);
    if (s3g_mark(h, 1)) return -1;
    const int n = h->n;
    hipLaunchKernelGGL(k_s3g_assemble, dim3(cdiv((long)n * n, 256)), dim3(256), 0, h->stream, n, h->nfree, (const int32_t*)h->blockmap,
                       (const int32_t*)h->eptr, (const int2*)h->eitems, (const int32_t*)h->gptr, (const int32_t*)h->gitems,
                       (const double*)h->scratch, lambda, h->H, h->A, h->g);
    s3g_cost(h, 0, true);
    return s3g_mark(h, 2);
}

int s3g_fetch(ps_sim3pg* h, double* out5, int32_t* stw) {
    HIP_OK(hipMemcpyAsync(out5, h->out, 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (stw) HIP_OK(hipMemcpyAsync(stw, h->stat, ST_NWORDS * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    HIP_OK(hipGetLastError());
    return 0;
}

int s3g_iteration(ps_sim3pg* h, double lambda, double* cost_after, double* dx_norm, double* relres, double* cost_lin) {
    if (s3g_linearize(h, lambda, nullptr)) return -1;
    const int n = h->n;
    hipStream_t st = h->stream;
    HIP_OK(hipMemsetAsync(h->stat, 0, ST_NWORDS * sizeof(int32_t), st));
    const SpdSolve S{n, h->A, h->Tinv, h->stat};
    if (S.factor(st)) return -1;
    if (s3g_mark(h, 3)) return -1;
    auto residual = [&]() {                                    // res = g - (H + lambda diag H) x; out[3], out[4] = res.res, g.g
        S.residual(st, h->H, h->g, h->x, h->res, h->res_part);
        hipLaunchKernelGGL(k_s3g_resid_fin, dim3(1), dim3(256), 0, st, n, (const double*)h->H, lambda, (const double*)h->x,
                           (const double*)h->g, h->res, h->out + 3);
    };
    HIP_OK(hipMemcpyAsync(h->x, h->g, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    S.solve_into(st, h->x);
    residual();
    S.solve_into(st, h->res);                                  // one refinement step through the same factor
    S.add(st, h->res, h->x);
    residual();
    if (s3g_mark(h, 4)) return -1;
    hipLaunchKernelGGL(k_s3g_retract, dim3(h->nrt), dim3(256), 0, st, h->nfree, (const int32_t*)h->free_vid, (const double*)h->x,
                       (const int32_t*)h->stat, h->verts, h->dx_part);
    hipLaunchKernelGGL(k_s3g_sum, dim3(1), dim3(256), 0, st, h->nrt, (const double*)h->dx_part, h->out + 2);
    s3g_cost(h, 1, false);
    if (s3g_mark(h, 5)) return -1;
    double o[5];
    int32_t stw[ST_NWORDS];
    if (s3g_fetch(h, o, stw)) return -1;
    if (h->profiling)
        for (int k = 0; k < 5; ++k) {
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
            h->stage_ms[k] = ms;
        }
    if (stw[ST_DIAG_FAIL])
        return fail("ps_sim3pg: the system matrix is not positive definite to rounding (dense blocked Cholesky); the vertices were not moved");
    if (cost_lin) *cost_lin = o[0];
    if (cost_after) *cost_after = o[1];
    if (dx_norm) *dx_norm = std::sqrt(o[2]);
    if (relres) *relres = o[4] > 0.0 ? std::sqrt(o[3] / o[4]) : 0.0;
    return 0;
}
}  // namespace
}  // extern "C++"
