// ps_abi_sim3pg.h -- C ABI of the Sim(3) pose graph (host driver: ps_host_sim3pg.h; kernels: ps_k_sim3pg.h).  Part of ps_core.hip
// (inside its extern "C" block, after ps_host_sim3pg.h).  Host pointers in, host pointers out; errors through fail().

int ps_sim3pg_create(int32_t num_vertices, const double* vertices13, const uint8_t* held, int32_t num_edges, const int32_t* edge_i,
                     const int32_t* edge_j, const double* edge_obs13, const double* edge_stiffness49, int32_t loss_id, double loss_k,
                     void* stream, ps_sim3pg** out) {
    if (!out) return fail("ps_sim3pg_create: null argument");
    *out = nullptr;
    if (num_vertices <= 0 || num_edges < 0 || !vertices13 || !held || (num_edges > 0 && (!edge_i || !edge_j || !edge_obs13)))
        return fail("ps_sim3pg_create: bad argument");
    if (num_edges > 10000000) return fail("ps_sim3pg_create: more than 10 000 000 edges");
    if (loss_id < 0 || loss_id > 5) return fail("ps_sim3pg_create: unknown loss id");
    if (!std::isfinite(loss_k)) return fail("ps_sim3pg_create: loss_k is not finite");
    const int nv = num_vertices, ne = num_edges;
    std::vector<int32_t> rid((size_t)nv, -1), free_vid;
    for (int v = 0; v < nv; ++v) if (!held[v]) { rid[v] = (int32_t)free_vid.size(); free_vid.push_back(v); }
    if ((int)free_vid.size() == nv) return fail("ps_sim3pg_create: no held vertex (the gauge of the graph is free: hold at least one)");
    if (7 * (long)free_vid.size() > PS_SPD_MAXN)
        return fail("ps_sim3pg_create: more unknowns than the dense direct solve takes (7 per free vertex, at most 8192)");
    if (s3g_check_vertices(vertices13, nv, "ps_sim3pg_create")) return -1;
    for (int e = 0; e < ne; ++e) {
        if (edge_i[e] < 0 || edge_i[e] >= nv || edge_j[e] < 0 || edge_j[e] >= nv) return fail("ps_sim3pg_create: edge vertex index out of range");
        if (edge_i[e] == edge_j[e]) return fail("ps_sim3pg_create: an edge joins a vertex with itself (i == j)");
    }
    if (!s3g_finite(edge_obs13, (size_t)ne * 13)) return fail("ps_sim3pg_create: an edge measurement is not finite");
    for (int e = 0; e < ne; ++e) if (!(edge_obs13[13 * (size_t)e + 12] > 0.0)) return fail("ps_sim3pg_create: an edge measurement's scale is not positive");
    if (edge_stiffness49 && !s3g_finite(edge_stiffness49, (size_t)ne * 49)) return fail("ps_sim3pg_create: an edge stiffness is not finite");
    if (need_device()) return -1;
    std::unique_ptr<ps_sim3pg> h(new ps_sim3pg);
    h->stream = (hipStream_t)stream;
    h->nv = nv; h->ne = ne; h->nfree = (int)free_vid.size(); h->n = 7 * h->nfree;
    h->nwg = std::max(1, cdiv(ne, PS_S3G_EDGES)); h->nrt = std::max(1, cdiv(h->nfree, 256));
    h->loss_id = loss_id; h->loss_k = loss_k;
    std::vector<double> obsinv((size_t)ne * 13);
    for (int e = 0; e < ne; ++e) s3g_host_inv(edge_obs13 + 13 * (size_t)e, obsinv.data() + 13 * (size_t)e);
    const size_t n = (size_t)h->n;
    const double zero5[5] = {};
    DevMem& M = h->mem;
    if (M.upload(&h->verts, vertices13, (size_t)nv * 13) || M.upload(&h->verts_snap, vertices13, (size_t)nv * 13) ||
        M.upload(&h->e_i, edge_i, (size_t)ne) || M.upload(&h->e_j, edge_j, (size_t)ne) ||
        M.upload(&h->e_obsinv, obsinv.data(), obsinv.size()) ||
        (edge_stiffness49 && M.upload(&h->e_W, edge_stiffness49, (size_t)ne * 49)) ||
        M.upload(&h->free_vid, free_vid.data(), free_vid.size()) ||
        M.alloc(&h->scratch, (size_t)ne * PS_S3G_ROW) || M.alloc(&h->cost_part, (size_t)h->nwg) ||
        M.alloc(&h->H, n * n) || M.alloc(&h->A, n * n) || M.alloc(&h->g, n) || M.alloc(&h->x, n) || M.alloc(&h->res, n) ||
        M.alloc(&h->Tinv, bchol_tinv_count((long)n)) || M.alloc(&h->res_part, spd_part_count((long)n)) ||
        M.alloc(&h->dx_part, (size_t)h->nrt) || M.upload(&h->out, zero5, (size_t)5) || M.alloc(&h->stat, (size_t)ST_NWORDS) ||
        s3g_build_structure(h.get(), rid, edge_i, edge_j)) return -1;
    HIP_OK(hipMemset(h->stat, 0, ST_NWORDS * sizeof(int32_t)));
    *out = h.release();
    return 0;
}

int ps_sim3pg_destroy(ps_sim3pg* h) {
    if (!h) return 0;
    if (h->stream) hipStreamSynchronize(h->stream); else hipDeviceSynchronize();
    delete h;
    return 0;
}

int ps_sim3pg_set_vertices(ps_sim3pg* h, const double* vertices13) {
    if (!h || !vertices13) return fail("ps_sim3pg_set_vertices: null argument");
    if (s3g_check_vertices(vertices13, h->nv, "ps_sim3pg_set_vertices")) return -1;
    HIP_OK(hipMemcpyAsync(h->verts, vertices13, (size_t)h->nv * 13 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    h->snap_valid = false;
    return 0;
}

int ps_sim3pg_get_vertices(ps_sim3pg* h, double* vertices13) {
    if (!h || !vertices13) return fail("ps_sim3pg_get_vertices: null argument");
    HIP_OK(hipMemcpyAsync(vertices13, h->verts, (size_t)h->nv * 13 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    return 0;
}

int ps_sim3pg_eval_cost(ps_sim3pg* h, double* cost) {
    if (!h || !cost) return fail("ps_sim3pg_eval_cost: null argument");
    s3g_cost(h, 0, false);
    double o[5];
    if (s3g_fetch(h, o, nullptr)) return -1;
    *cost = o[0];
    return 0;
}

int ps_sim3pg_linearize(ps_sim3pg* h, double lambda, double* H_out, double* g_out, double* cost) {
    if (!h) return fail("ps_sim3pg_linearize: null argument");
    if (s3g_linearize(h, lambda, nullptr)) return -1;
    const size_t n = (size_t)h->n;
    if (H_out) HIP_OK(hipMemcpyAsync(H_out, h->A, n * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (g_out) HIP_OK(hipMemcpyAsync(g_out, h->g, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    double o[5];
    if (s3g_fetch(h, o, nullptr)) return -1;
    if (cost) *cost = o[0];
    return 0;
}

int ps_sim3pg_iteration(ps_sim3pg* h, double lambda, double* cost_after, double* dx_norm, double* relres) {
    if (!h) return fail("ps_sim3pg_iteration: null argument");
    return s3g_iteration(h, lambda, cost_after, dx_norm, relres, nullptr);
}

// The loop of Problem.solve under the linesearch != 0 meaning (an iteration's cost is the cost after its step), the stopping
// rule ps_stop_rule.h's; best parameters kept by a copy and restored by exchanging the two tables, as ps_solve does.
int ps_sim3pg_solve(ps_sim3pg* h, const ps_solve_options* options, double* cost_history, int32_t cap, int32_t* n_history,
                    int32_t* iterations, double* last_dx_norm) {
    if (!h || !options || !cost_history || !n_history) return fail("ps_sim3pg_solve: null argument");
    const ps_solve_options* o = options;
    if (o->max_iters < 0 || (long)o->max_iters + 2 > cap) return fail("ps_sim3pg_solve: cost_history holds fewer than max_iters + 2 entries");
    double c0 = 0.0;
    if (ps_sim3pg_eval_cost(h, &c0)) return -1;
    ps_stop_state stop;
    ps_stop_begin(&stop, c0);
    int n = 0;
    cost_history[n++] = c0;
    double dxn = 0.0;
    bool done = false;
    h->snap_valid = false;
    while (!done) {
        double c = 0.0;
        if (s3g_iteration(h, o->lm_lambda, &c, &dxn, nullptr, nullptr)) { *n_history = n; return -1; }
        cost_history[n++] = c;
        const int f = ps_stop_step(o, &stop, c, dxn);
        if (f & PS_STOP_KEEP_BEST) {
            HIP_OK(hipMemcpyAsync(h->verts_snap, h->verts, (size_t)h->nv * 13 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            h->snap_valid = true;
        }
        if ((f & PS_STOP_RESTORE_BEST) && h->snap_valid) std::swap(h->verts, h->verts_snap);
        done = f & PS_STOP_DONE;
    }
    HIP_OK(hipStreamSynchronize(h->stream));
    *n_history = n;
    if (iterations) *iterations = stop.iters;
    if (last_dx_norm) *last_dx_norm = dxn;
    return 0;
}

// test entry: the parity tap of k_s3g_edges at the current vertices, 105 doubles per edge
int ps_sim3pg_debug_edges(ps_sim3pg* h, double* tap105) {
    if (!h || !tap105) return fail("ps_sim3pg_debug_edges: null argument");
    if (h->ne == 0) return 0;
    if (!h->dbg && h->mem.alloc(&h->dbg, (size_t)h->ne * PS_S3G_DBG)) return -1;
    s3g_edges(h, 0, h->dbg);
    HIP_OK(hipMemcpyAsync(tap105, h->dbg, (size_t)h->ne * PS_S3G_DBG * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    HIP_OK(hipGetLastError());
    return 0;
}

// test entry: the device functions on a host table of n tangent vectors -> exp (13 each), log of that (7), the adjoint of that (49)
int ps_sim3pg_debug_explog(int32_t n, const double* xi_in, double* S13_out, double* xi_back, double* adj49_out) {
    if (n <= 0 || !xi_in || !S13_out || !xi_back || !adj49_out) return fail("ps_sim3pg_debug_explog: bad argument");
    if (need_device()) return -1;
    DevBuf bi, bs, bx, ba;
    if (bi.put(xi_in, (size_t)n * 7) || bs.get((size_t)n * 13 * 8) || bx.get((size_t)n * 7 * 8) || ba.get((size_t)n * 49 * 8)) return -1;
    hipLaunchKernelGGL(k_s3g_explog, dim3(cdiv(n, 256)), dim3(256), 0, 0, n, (const double*)bi.as<double>(), bs.as<double>(), bx.as<double>(),
                       ba.as<double>());
    HIP_OK(hipGetLastError());
    return bs.fetch(S13_out, (size_t)n * 13) || bx.fetch(xi_back, (size_t)n * 7) || ba.fetch(adj49_out, (size_t)n * 49) ? -1 : 0;
}

// measurement entry: enable != 0 times the stages of every later iteration with events; stage_ms5 (or NULL) receives the last
// iteration's {edges, assemble, factor, substitute + refine, retract + cost} in ms
int ps_sim3pg_profile(ps_sim3pg* h, int32_t enable, double* stage_ms5) {
    if (!h) return fail("ps_sim3pg_profile: null argument");
    if (stage_ms5) std::copy(h->stage_ms, h->stage_ms + 5, stage_ms5);
    h->profiling = enable != 0;
    return 0;
}
