// ps_abi_dense.h -- C ABI: the dense RGB-D VO pipeline (reference pyslam/pipelines/dense.py, keyframes.py; kernels in
// csrc/ps_k_dense.h).  Part of ps_core.hip (one translation unit; included from there, in this order).
//
// A handle owns a fixed number of frame slots, each sized for the largest frame at create time: the raw and float64
// image pyramid, the gradient and depth levels, and the pixel tables of every level.  Nothing is allocated after
// create except the history buffer of ps_dense_track when a caller asks for more iterations than before, so the
// resident bytes do not grow with the length of a sequence.

extern "C++" {      // (the handle has a member template; this file sits inside ps_core.hip's extern "C")
struct PsDenseLevel {
    int h = 0, w = 0;
    size_t off = 0;                     // pixel offset of the level inside the slot's per-pixel buffers
    size_t toff = 0;                    // offset of the level's blocks in the block-count buffer
};

struct PsDenseSlot {
    int dtype = -1;                     // -1 empty, 0 uint8, 1 float64
    int has_depth = 0;
    int grad_ok[PS_DENSE_MAX_LEVELS] = {};
    int tables_ok[PS_DENSE_MAX_LEVELS] = {};
    DenseCam cam[PS_DENSE_MAX_LEVELS] = {};
    double var_i[PS_DENSE_MAX_LEVELS] = {}, var_d[PS_DENSE_MAX_LEVELS] = {};
    void* raw = nullptr;                // pyramid in the input type (8 bytes per pixel of capacity)
    double *imf = nullptr, *gx = nullptr, *gy = nullptr, *dl = nullptr, *depth0 = nullptr;
    double *pt = nullptr, *imr = nullptr, *jac = nullptr, *tri = nullptr;
    uint8_t* flags = nullptr;
    int* counts = nullptr;              // block counts -> block offsets
    int* npix = nullptr;                // per level: pixel count of the tables (device)
};

struct ps_dense {
    hipStream_t stream = nullptr;
    int levels = 0, max_h = 0, max_w = 0, h = 0, w = 0;
    PsDenseLevel lv[PS_DENSE_MAX_LEVELS];
    size_t pix_total = 0, blocks_total = 0;
    std::vector<PsDenseSlot> slots;
    DevMem mem{8};
    double* partials = nullptr;       // k_dense_pass partials (largest level)
    int max_parts = 0;
    double* pose = nullptr;
    DenseSolveState* state = nullptr;
    double* results = nullptr;          // levels x (2 + hist_cap)
    int hist_cap = 0;
    std::vector<double> h_results;
    double h_pose[12];
};
}  // extern "C++"

namespace {
// level geometry of an h x w frame: the cv2.pyrDown chain, ((h+1)/2, (w+1)/2) per level
void dense_geometry(ps_dense* d, int h, int w) {
    size_t off = 0, boff = 0;
    for (int l = 0; l < d->levels; ++l) {
        d->lv[l].h = h; d->lv[l].w = w; d->lv[l].off = off; d->lv[l].toff = boff;
        off += (size_t)h * w;
        boff += (size_t)cdiv((long)h * w, 256);
        h = (h + 1) / 2; w = (w + 1) / 2;
    }
    d->pix_total = off; d->blocks_total = boff;
}

int dense_slot_ok(ps_dense* d, int slot) {
    if (!d) return fail("null handle");
    if (slot < 0 || slot >= (int)d->slots.size()) return fail("slot index out of range");
    return 0;
}

int dense_level_ok(ps_dense* d, int level) {
    if (level < 0 || level >= d->levels) return fail("pyramid level out of range");
    return 0;
}

// gradient and depth level l of a slot (k_dense_grad), once per upload
int dense_grad(ps_dense* d, PsDenseSlot& s, int l) {
    if (s.grad_ok[l]) return 0;
    const PsDenseLevel& L = d->lv[l];
    const int n = L.h * L.w;
    hipLaunchKernelGGL(k_dense_grad, dim3(cdiv(n, 256)), dim3(256), 0, d->stream, (const double*)(s.imf + L.off), L.h, L.w,
                       (const double*)(s.has_depth ? s.depth0 : nullptr), d->w, l, s.gx + L.off, s.gy + L.off, s.dl + L.off);
    HIP_OK(hipGetLastError());
    s.grad_ok[l] = 1;
    return 0;
}
}  // namespace

int ps_dense_create(int32_t levels, int32_t max_height, int32_t max_width, int32_t num_slots, void* stream, ps_dense** out) {
    if (!out) return fail("null argument");
    *out = nullptr;
    if (levels < 1 || levels > PS_DENSE_MAX_LEVELS) return fail("levels must be 1..8");
    if (max_height < 2 || max_width < 2) return fail("frames must be at least 2 x 2 pixels");
    if ((int64_t)max_height * max_width > (1 << 28)) return fail("frame too large");
    if (num_slots < 1 || num_slots > 16) return fail("num_slots must be 1..16");
    if (need_device()) return -1;
    std::unique_ptr<ps_dense> d(new ps_dense);
    d->stream = (hipStream_t)stream;
    d->levels = levels; d->max_h = max_height; d->max_w = max_width;
    dense_geometry(d.get(), max_height, max_width);
    const size_t P = d->pix_total, B = d->blocks_total;
    d->slots.resize(num_slots);
    DevMem& M = d->mem;
    for (PsDenseSlot& s : d->slots) {
        if (M.alloc_bytes(&s.raw, P * 8) || M.alloc(&s.imf, P) || M.alloc(&s.gx, P) || M.alloc(&s.gy, P) ||
            M.alloc(&s.dl, P) || M.alloc(&s.depth0, (size_t)max_height * max_width) || M.alloc(&s.pt, 3 * P) ||
            M.alloc(&s.imr, P) || M.alloc(&s.jac, 2 * P) || M.alloc(&s.tri, 3 * P) || M.alloc(&s.flags, P) ||
            M.alloc(&s.counts, B) || M.alloc(&s.npix, PS_DENSE_MAX_LEVELS)) return -1;
        HIP_OK(hipMemsetAsync(s.npix, 0, PS_DENSE_MAX_LEVELS * sizeof(int), d->stream));
    }
    d->max_parts = std::max(1, cdiv((long)max_height * max_width, 256 * PS_PHOTO_PPT));
    if (M.alloc(&d->partials, (size_t)d->max_parts * PS_PHOTO_NACC) || M.alloc(&d->pose, 12) || M.alloc(&d->state, 1))
        return -1;
    HIP_OK(hipStreamSynchronize(d->stream));
    *out = d.release();
    return 0;
}

int ps_dense_destroy(ps_dense* d) {
    if (!d) return 0;
    if (d->stream) hipStreamSynchronize(d->stream); else hipDeviceSynchronize();
    delete d;
    return 0;
}

int ps_dense_upload(ps_dense* d, int32_t slot, int32_t dtype, int32_t height, int32_t width, const void* image, const double* depth) {
    if (dense_slot_ok(d, slot)) return -1;
    if (!image && !depth) return fail("nothing to upload");
    PsDenseSlot& s = d->slots[slot];
    if (image) {
        if (dtype != 0 && dtype != 1) return fail("dtype must be 0 (uint8) or 1 (float64)");
        if (height < 2 || width < 2 || height > d->max_h || width > d->max_w) return fail("frame size outside the handle's capacity");
        // the level geometry follows the frame; every slot of a handle holds frames of one size
        bool others = false;
        for (int k = 0; k < (int)d->slots.size(); ++k) others = others || (k != slot && d->slots[k].dtype >= 0);
        if (others && (height != d->h || width != d->w)) return fail("all frames of a handle must have the same size");
        d->h = height; d->w = width;
        dense_geometry(d, height, width);
        const size_t n0 = (size_t)height * width;
        HIP_OK(hipMemcpyAsync(s.raw, image, n0 * (dtype ? 8 : 1), hipMemcpyHostToDevice, d->stream));
        hipLaunchKernelGGL(k_dense_level0, dim3(cdiv(n0, 256)), dim3(256), 0, d->stream, (const void*)s.raw, dtype == 0, (int)n0, s.imf);
        for (int l = 1; l < d->levels; ++l) {
            const PsDenseLevel &S = d->lv[l - 1], &D = d->lv[l];
            const dim3 grid(cdiv(D.w, PS_DENSE_TILE), cdiv(D.h, PS_DENSE_TILE));
            if (dtype == 0)
                hipLaunchKernelGGL(k_dense_pyrdown<uint8_t>, grid, dim3(256), 0, d->stream, (const uint8_t*)s.raw + S.off, S.h, S.w,
                                   (uint8_t*)s.raw + D.off, s.imf + D.off, D.h, D.w);
            else
                hipLaunchKernelGGL(k_dense_pyrdown<double>, grid, dim3(256), 0, d->stream, (const double*)s.raw + S.off, S.h, S.w,
                                   (double*)s.raw + D.off, s.imf + D.off, D.h, D.w);
        }
        HIP_OK(hipGetLastError());
        s.dtype = dtype;
        s.has_depth = 0;
        for (int l = 0; l < PS_DENSE_MAX_LEVELS; ++l) { s.grad_ok[l] = 0; s.tables_ok[l] = 0; }
    }
    if (depth) {
        if (s.dtype < 0) return fail("upload the slot's image before its depth");
        if (image == nullptr && (height != d->h || width != d->w)) return fail("depth size differs from the slot's image");
        HIP_OK(hipMemcpyAsync(s.depth0, depth, (size_t)d->h * d->w * sizeof(double), hipMemcpyHostToDevice, d->stream));
        s.has_depth = 1;
        for (int l = 0; l < PS_DENSE_MAX_LEVELS; ++l) { s.grad_ok[l] = 0; s.tables_ok[l] = 0; }
    }
    // no wait here: the caller keeps `image` and `depth` alive until its next call that synchronises (ps_dense_track)
    return 0;
}

int ps_dense_make_tables(ps_dense* d, int32_t slot, int32_t num_levels, const int32_t* levels, const double* cams6,
                         double intensity_covar, double depth_covar, double min_grad) {
    if (dense_slot_ok(d, slot)) return -1;
    if (num_levels < 0 || (num_levels && (!levels || !cams6))) return fail("bad level list");
    PsDenseSlot& s = d->slots[slot];
    if (s.dtype < 0) return fail("empty slot");
    if (!s.has_depth) return fail("the slot has no depth: upload it before making tables");
    for (int k = 0; k < num_levels; ++k) {
        const int l = levels[k];
        if (dense_level_ok(d, l)) return -1;
        const PsDenseLevel& L = d->lv[l];
        const double* c = cams6 + 6 * k;
        if ((int)c[4] != L.w || (int)c[5] != L.h) return fail("level camera size differs from the pyramid level's image");
        DenseCam cam{c[0], c[1], c[2], c[3], c[4], c[5]};
        if (dense_grad(d, s, l)) return -1;
        const int n = L.h * L.w, nb = cdiv(n, 256);
        hipLaunchKernelGGL(k_dense_flags, dim3(nb), dim3(256), 0, d->stream, n, L.w, cam, min_grad, (const double*)(s.gx + L.off),
                           (const double*)(s.gy + L.off), (const double*)(s.dl + L.off), s.flags + L.off, s.counts + L.toff);
        hipLaunchKernelGGL(k_dense_scan, dim3(1), dim3(1024), 0, d->stream, nb, s.counts + L.toff, s.npix + l);
        DenseTables t{s.pt + 3 * L.off, s.imr + L.off, s.jac + 2 * L.off, s.tri + 3 * L.off};
        hipLaunchKernelGGL(k_dense_compact, dim3(nb), dim3(256), 0, d->stream, n, L.w, cam, (const double*)(s.imf + L.off),
                           (const double*)(s.gx + L.off), (const double*)(s.gy + L.off), (const double*)(s.dl + L.off),
                           (const uint8_t*)(s.flags + L.off), (const int*)(s.counts + L.toff), t);
        HIP_OK(hipGetLastError());
        s.cam[l] = cam; s.var_i[l] = intensity_covar; s.var_d[l] = depth_covar;
        s.tables_ok[l] = 1;
    }
    return 0;
}

int ps_dense_track(ps_dense* d, int32_t ref_slot, int32_t track_slot, int32_t num_levels, const int32_t* levels,
                   const int32_t* rot_only, const ps_solve_options* opt, int32_t loss_id, double loss_k, const double* pose12_in,
                   double* pose12_out, int32_t* iterations, double* cost_history, int32_t history_cap) {
    if (dense_slot_ok(d, ref_slot) || dense_slot_ok(d, track_slot)) return -1;
    if (ref_slot == track_slot) return fail("reference and tracking frame must be in different slots");
    if (!opt || !pose12_in || !pose12_out || num_levels < 0 || num_levels > PS_DENSE_MAX_LEVELS || (num_levels && (!levels || !rot_only)))
        return fail("bad argument");
    if (loss_id < 0 || loss_id > 5) return fail("unknown loss id");
    if (opt->max_iters < 0 || opt->max_iters > 100000) return fail("max_iters out of range");
    if (opt->lm_lambda != 0.0) return fail("the dense pipeline has no damping (Options.lm_lambda must be 0)");
    const int hist = opt->max_iters + 2;
    if (num_levels && (!iterations || !cost_history || history_cap < hist)) return fail("history buffer too small: need max_iters + 2 per level");
    PsDenseSlot &R = d->slots[ref_slot], &Tr = d->slots[track_slot];
    if (Tr.dtype < 0) return fail("empty tracking slot");
    for (int k = 0; k < num_levels; ++k) {
        if (dense_level_ok(d, levels[k])) return -1;
        if (!R.tables_ok[levels[k]]) return fail("the reference slot has no tables for a level of the sequence");
    }
    const size_t per = 2 + (size_t)hist;
    if (hist > d->hist_cap) {                    // (the only allocation after create; freed with the handle)
        if (d->results) {
            HIP_OK(hipStreamSynchronize(d->stream));
            d->mem.release(d->results);
        }
        if (d->mem.alloc(&d->results, PS_DENSE_MAX_LEVELS * per)) return -1;
        d->hist_cap = hist;
    }
    std::copy(pose12_in, pose12_in + 12, d->h_pose);
    HIP_OK(hipMemcpyAsync(d->pose, d->h_pose, 12 * sizeof(double), hipMemcpyHostToDevice, d->stream));
    HIP_OK(hipMemsetAsync(d->results, 0, (size_t)num_levels * per * sizeof(double), d->stream));
    HIP_OK(hipMemsetAsync(d->state, 0, sizeof(DenseSolveState), d->stream));
    for (int k = 0; k < num_levels; ++k) {
        const int l = levels[k];
        const PsDenseLevel& L = d->lv[l];
        PhotoArgs a{};
        a.n = 0;
        a.pt_ref = R.pt + 3 * L.off; a.im_ref = R.imr + L.off; a.im_jac = R.jac + 2 * L.off; a.tri_jac_d = R.tri + 3 * L.off;
        a.image = Tr.imf + L.off; a.h = L.h; a.w = L.w;
        a.cu = R.cam[l].cu; a.cv = R.cam[l].cv; a.fu = R.cam[l].fu; a.fv = R.cam[l].fv; a.b = 0.0;
        a.cam_type = 1; a.cam_w = R.cam[l].w; a.cam_h = R.cam[l].h;
        a.var_i = R.var_i[l]; a.var_d = R.var_d[l];
        a.loss_id = loss_id; a.loss_k = loss_k;
        const int nparts = std::max(1, cdiv((long)L.h * L.w, 256 * PS_PHOTO_PPT));
        const int* n_dev = R.npix + l;
        double* out = d->results + (size_t)k * per;
        const int rot = rot_only[k] != 0;
        hipLaunchKernelGGL(k_dense_pass, dim3(nparts), dim3(256), 0, d->stream, a, n_dev, (const double*)d->pose, 0, 1, d->partials,
                           (const DenseSolveState*)d->state);
        hipLaunchKernelGGL(k_dense_finish, dim3(1), dim3(256), 0, d->stream, nparts, (const double*)d->partials, 0, rot, *opt, d->pose,
                           d->state, out);
        for (int it = 0; it <= opt->max_iters; ++it) {       // the loop stops once the iteration count exceeds max_iters
            hipLaunchKernelGGL(k_dense_pass, dim3(nparts), dim3(256), 0, d->stream, a, n_dev, (const double*)d->pose, 1, 0,
                               d->partials, (const DenseSolveState*)d->state);
            hipLaunchKernelGGL(k_dense_finish, dim3(1), dim3(256), 0, d->stream, nparts, (const double*)d->partials, 1, rot, *opt,
                               d->pose, d->state, out);
            if (opt->linesearch) {
                hipLaunchKernelGGL(k_dense_pass, dim3(nparts), dim3(256), 0, d->stream, a, n_dev, (const double*)d->pose, 0, 0,
                                   d->partials, (const DenseSolveState*)d->state);
                hipLaunchKernelGGL(k_dense_finish, dim3(1), dim3(256), 0, d->stream, nparts, (const double*)d->partials, 2, rot, *opt,
                                   d->pose, d->state, out);
            }
        }
    }
    HIP_OK(hipGetLastError());
    d->h_results.resize((size_t)num_levels * per + 12);
    HIP_OK(hipMemcpyAsync(d->h_results.data() + 12, d->results, (size_t)num_levels * per * sizeof(double), hipMemcpyDeviceToHost,
                          d->stream));
    HIP_OK(hipMemcpyAsync(d->h_results.data(), d->pose, 12 * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    HIP_OK(hipStreamSynchronize(d->stream));         // the one synchronisation of a tracked frame
    for (int k = 0; k < num_levels; ++k) {
        const double* r = d->h_results.data() + 12 + (size_t)k * per;
        if (r[1] == 1.0) return fail("photometric alignment: fewer than 6 valid pixels");
        if (r[1] == 2.0) return fail("photometric alignment: normal equations are not positive definite");
        const int its = (int)r[0];
        iterations[k] = its;
        double* hk = cost_history + (size_t)k * history_cap;
        std::fill(hk, hk + history_cap, 0.0);
        std::copy(r + 2, r + 2 + its + 1, hk);
    }
    std::copy(d->h_results.data(), d->h_results.data() + 12, pose12_out);
    return 0;
}

int ps_dense_num_pixels(ps_dense* d, int32_t slot, int32_t level, int32_t* num_pixels) {
    if (dense_slot_ok(d, slot) || dense_level_ok(d, level)) return -1;
    if (!num_pixels) return fail("null argument");
    if (!d->slots[slot].tables_ok[level]) return fail("no tables for this level");
    HIP_OK(hipMemcpyAsync(num_pixels, d->slots[slot].npix + level, sizeof(int32_t), hipMemcpyDeviceToHost, d->stream));
    HIP_OK(hipStreamSynchronize(d->stream));
    return 0;
}

int ps_dense_level_shape(ps_dense* d, int32_t level, int32_t* height, int32_t* width) {
    if (!d) return fail("null handle");
    if (dense_level_ok(d, level)) return -1;
    if (!height || !width) return fail("null argument");
    *height = d->lv[level].h; *width = d->lv[level].w;
    return 0;
}

int ps_dense_read_level(ps_dense* d, int32_t slot, int32_t level, int32_t what, double* out) {
    if (dense_slot_ok(d, slot) || dense_level_ok(d, level)) return -1;
    if (!out) return fail("null argument");
    PsDenseSlot& s = d->slots[slot];
    if (s.dtype < 0) return fail("empty slot");
    const PsDenseLevel& L = d->lv[level];
    const size_t n = (size_t)L.h * L.w;
    if (what == 0) {
        HIP_OK(hipMemcpyAsync(out, s.imf + L.off, n * 8, hipMemcpyDeviceToHost, d->stream));
    } else if (what == 1 || what == 2) {
        if (what == 2 && !s.has_depth) return fail("the slot has no depth");
        if (dense_grad(d, s, level)) return -1;
        if (what == 1) {
            HIP_OK(hipMemcpyAsync(out, s.gx + L.off, n * 8, hipMemcpyDeviceToHost, d->stream));
            HIP_OK(hipMemcpyAsync(out + n, s.gy + L.off, n * 8, hipMemcpyDeviceToHost, d->stream));
        } else {
            HIP_OK(hipMemcpyAsync(out, s.dl + L.off, n * 8, hipMemcpyDeviceToHost, d->stream));
        }
    } else {
        return fail("what must be 0 (image), 1 (gradient) or 2 (depth)");
    }
    HIP_OK(hipStreamSynchronize(d->stream));
    return 0;
}

int ps_dense_read_tables(ps_dense* d, int32_t slot, int32_t level, int32_t num_pixels, double* pt_ref, double* im_ref, double* im_jac,
                         double* tri_jac_d) {
    int32_t n = 0;
    if (ps_dense_num_pixels(d, slot, level, &n)) return -1;
    if (num_pixels != n) return fail("num_pixels differs from the level's pixel count");
    if (!pt_ref || !im_ref || !im_jac || !tri_jac_d) return fail("null argument");
    PsDenseSlot& s = d->slots[slot];
    const size_t off = d->lv[level].off;
    HIP_OK(hipMemcpyAsync(pt_ref, s.pt + 3 * off, (size_t)n * 24, hipMemcpyDeviceToHost, d->stream));
    HIP_OK(hipMemcpyAsync(im_ref, s.imr + off, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
    HIP_OK(hipMemcpyAsync(im_jac, s.jac + 2 * off, (size_t)n * 16, hipMemcpyDeviceToHost, d->stream));
    HIP_OK(hipMemcpyAsync(tri_jac_d, s.tri + 3 * off, (size_t)n * 24, hipMemcpyDeviceToHost, d->stream));
    HIP_OK(hipStreamSynchronize(d->stream));
    return 0;
}

int ps_dense_device_bytes(ps_dense* d, int64_t* bytes) {
    if (!d || !bytes) return fail("null argument");
    *bytes = d->mem.bytes();
    return 0;
}
