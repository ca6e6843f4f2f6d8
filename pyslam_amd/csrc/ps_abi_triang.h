// ps_abi_triang.h -- C ABI: multi-view triangulation of variable landmarks (kernel: ps_k_triang.h).
// Part of ps_core.hip (inside its extern "C" block, after ps_abi_cov.h).
//
// One launch (linear start and every refinement step), one synchronisation.  The results pass through a device block kept on
// the handle ([points (3 n) | status (n) | slots (n)], grown when a call asks for more, freed by ps_problem_destroy).

int ps_triangulate(ps_problem* h, int64_t n, const int32_t* vids, int refine_iters, double min_parallax_deg, int write_back,
                   double* points_out, int32_t* status_out) {
    if (!h) return fail("null argument");
    if (h->nv > 0 && h->D != 6) return fail("ps_triangulate: landmarks on a problem whose poses are not SE(3)");
    if (refine_iters < 0 || refine_iters > 1000) return fail("ps_triangulate: refine_iters must lie in [0, 1000]");
    if (!(min_parallax_deg >= 0.0 && min_parallax_deg <= 180.0)) return fail("ps_triangulate: min_parallax_deg must lie in [0, 180]");
    if (!vids) n = h->nv;
    if (n < 0) return fail("ps_triangulate: negative count");
    if (n == 0) return 0;
    if (n >= (1L << 31) / 16) return fail("ps_triangulate: too many landmarks for one call");
    if (h->h_slot_of_vid.size() != h->h_vid_of_slot.size()) {
        h->h_slot_of_vid.assign(h->h_vid_of_slot.size(), 0);
        for (size_t s2 = 0; s2 < h->h_vid_of_slot.size(); ++s2) h->h_slot_of_vid[h->h_vid_of_slot[s2]] = (int32_t)s2;
    }
    std::vector<int32_t> slots;
    if (vids) {
        slots.resize((size_t)n);
        for (int64_t k = 0; k < n; ++k) {
            if (vids[k] < 0 || vids[k] >= h->nv)
                return fail("ps_triangulate: landmark index " + std::to_string(vids[k]) + " out of range (variable landmarks: " +
                            std::to_string(h->nv) + ")");
            slots[k] = h->h_slot_of_vid[vids[k]];
        }
    }
    const size_t words = (size_t)n * 3 + (size_t)n;            // doubles: points, then status | slots as int32 pairs
    if (h->tri_cap < words) {
        if (h->tri_buf) { hipStreamSynchronize(h->stream); hipFree(h->tri_buf); h->tri_buf = nullptr; h->tri_cap = 0; }
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, words * sizeof(double));
        if (e != hipSuccess) return fail(std::string("ps_triangulate: hipMalloc: ") + hipGetErrorString(e));
        h->tri_buf = (double*)p; h->tri_cap = words;
    }
    double* d_pts = h->tri_buf;
    int32_t* d_status = reinterpret_cast<int32_t*>(h->tri_buf + (size_t)n * 3);
    int32_t* d_slots = d_status + n;
    hipStream_t st = h->stream;
    if (vids) HIP_OK(hipMemcpyAsync(d_slots, slots.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const double cos_min = std::cos(min_parallax_deg * (3.14159265358979323846 / 180.0));
    const ObsWide wl{h->sidx_l, h->stiff_tab};
    const dim3 grid(cdiv(n, 256 / PS_LM_GROUP)), block(256);
    if (h->wide_obs)
        hipLaunchKernelGGL(k_triangulate<true>, grid, block, 0, st, (int)n, vids ? d_slots : (const int32_t*)nullptr, h->lm_ptr, h->lm_point,
                           h->lobs, h->poses, h->points, h->ogroups, wl, refine_iters, cos_min, write_back ? 1 : 0, d_pts, d_status);
    else
        hipLaunchKernelGGL(k_triangulate<false>, grid, block, 0, st, (int)n, vids ? d_slots : (const int32_t*)nullptr, h->lm_ptr, h->lm_point,
                           h->lobs, h->poses, h->points, h->ogroups, wl, refine_iters, cos_min, write_back ? 1 : 0, d_pts, d_status);
    if (write_back) {                                           // the parameters moved: as ps_set_params
        h->params_moved_since_lin = true;
        h->prelin_valid = h->prelm_valid = h->ride_valid = false;
        h->last_cost = h->prev_cost = -1.0;
    }
    // without a list the kernel ran in slot order: back to the caller's vid order on the host
    std::vector<double> pts(points_out && !vids ? (size_t)n * 3 : 0);
    std::vector<int32_t> stat(status_out && !vids ? (size_t)n : 0);
    if (points_out) HIP_OK(hipMemcpyAsync(vids ? points_out : pts.data(), d_pts, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (status_out) HIP_OK(hipMemcpyAsync(vids ? status_out : stat.data(), d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (sync(h)) return -1;
    if (!vids)
        for (int64_t s2 = 0; s2 < n; ++s2) {
            const int32_t vid = h->h_vid_of_slot[s2];
            if (points_out) std::memcpy(points_out + 3 * (size_t)vid, &pts[3 * (size_t)s2], 3 * sizeof(double));
            if (status_out) status_out[vid] = stat[s2];
        }
    return 0;
}
