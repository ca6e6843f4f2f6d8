// ps_abi_feat.h -- C ABI: the feature matcher of the sparse VO pipelines (kernels in csrc/ps_k_feat.h; definition:
// DESIGN.md section 7).  Part of ps_core.hip (one translation unit; included from there, in this order).
//
// A handle keeps three frames (one or two images each): the previous and the current one, as a matcher with a
// two-frame window does, and one more as a cache.  A pushed frame whose bytes equal a frame the handle holds is not
// uploaded and its features are not computed again: the sparse pipelines push the active keyframe in front of every
// tracking frame.  Everything is allocated at create time; a match is a fixed sequence of launches on the handle's
// stream with one synchronisation at its end.  The one exception is the map of matching by projection (ps_feat_set_map,
// step 8 of the definition): its buffers are allocated at the first ps_feat_set_map and grow with the map, so a handle
// that never sets one holds exactly what it was created with.  Likewise the second-best costs of matching without a prior
// (ps_feat_match_map_global, step 9): the map's result block has room for them from the first such match on.  And the keyframe
// database (ps_feat_db_*, step 10; kernel in csrc/ps_k_feat_db.h): nothing of it exists before the first ps_feat_db_add, and its
// buffers grow by doubling.

#define PS_FEAT_DB_MAX_ENTRIES 65536
#define PS_FEAT_DB_MAX_DESC (1 << 22)

extern "C++" {
struct PsFeatImage {
    uint8_t* img = nullptr;
    short *du = nullptr, *dv = nullptr;
    int2* uv = nullptr;
    long long* R = nullptr;
    uint32_t* desc = nullptr;
    int *row_start = nullptr, *n = nullptr;
    FeatList list() const { return FeatList{n, uv, desc, row_start, du, dv}; }
};

struct PsFeatFrame {
    int h = 0, w = 0, stereo = 0;
    bool held = false, features_ok = false;
    long long det_threshold = 0;
    int det_nms = 0, det_max = 0;
    uint64_t used = 0;
    std::vector<uint8_t> host[2];           // the bytes as pushed: a frame is recognised by content
    PsFeatImage im[2];
};

struct ps_feat {
    hipStream_t stream = nullptr;
    int max_h = 0, max_w = 0, max_features = 0, raw_cap = 0;
    PsFeatFrame frame[3];
    int prev = -1, cur = -1;
    uint64_t clock = 0;
    int64_t feature_passes = 0;
    DevMem mem{16}, map_mem{16}, db_mem{16};    // what create allocates (and the map's claim words) | what grows with the map | the database
    // scratch of a feature pass and of a match
    long long *R = nullptr, *raw_R = nullptr;
    uint8_t *flags = nullptr, *keep = nullptr, *mflags = nullptr;
    int *counts = nullptr, *n_raw = nullptr, *leg[4] = {}, *visited = nullptr, *idx4 = nullptr, *n_match = nullptr;
    int2* raw_uv = nullptr;
    double* m8 = nullptr;
    int h_n_match = 0;
    // the map of matching by projection: nothing of it exists before the first ps_feat_set_map
    bool map_set = false;
    int map_n = 0, map_cap = 0, h_n_map_matched = 0, map_matched_n = -1;
    bool map_global_used = false, map_matched_global = false;      // a global match has run; the last map match was one
    // the second-best costs of a global match lie behind the block of map_out, which is that much larger (map_cap ints, at least
    // 16 bytes) from the first global match on
    double* map_pts = nullptr;
    uint32_t* map_desc = nullptr;
    uint8_t* map_out = nullptr;             // [count, 16 bytes | uv 2N doubles | feature N | status N | cost N] of the N matched last
    std::vector<uint8_t> h_map_out;         // its copy on the host: one download per match, read from there (a global match:
                                            // with the N second-best costs behind the cost array)
    unsigned long long* map_claim = nullptr;
    // the keyframe database (step 10): entries are appended, never edited; nothing of it exists before the first ps_feat_db_add
    std::vector<int> db_start, db_len, db_block;   // per entry: first descriptor, length, first workgroup (db_block has K + 1 values)
    int64_t db_n = 0, db_desc_cap = 0;                     // descriptors held, room for
    int db_block_cap = 0, db_entry_cap = 0;
    uint32_t* db_desc = nullptr;
    FeatDbBlock* db_blocks = nullptr;
    int *db_estart = nullptr, *db_elen = nullptr, *db_score = nullptr;
    // room for n values where there was room for `cap` (doubling), the first `used` kept: the stream is idle when this is called
    template <typename T> int grow_db(T** p, int64_t used, int64_t cap, int64_t n, int64_t first_cap, int64_t* new_cap) {
        int64_t c = cap ? cap : first_cap;
        while (c < n) c *= 2;
        *new_cap = c;
        if (c == cap) return 0;
        T* q = nullptr;
        if (db_mem.alloc(&q, (size_t)c)) return -1;
        if (used && hipMemcpy(q, *p, (size_t)used * sizeof(T), hipMemcpyDeviceToDevice) != hipSuccess) { db_mem.release(q); return fail("hipMemcpy failed"); }
        db_mem.release(*p);
        *p = q;
        return 0;
    }
    void free_map() { map_mem.clear(); map_cap = 0; }
    static size_t map_out_bytes(size_t n, bool with_second) { return 16 + 28 * n + (with_second ? std::max<size_t>(4 * n, 16) : 0); }
    // the first global match: map_out makes room for the second-best costs (its contents are on the host already)
    int grow_map_out_for_second() {
        uint8_t* old = map_cap ? map_out : nullptr;        // a map that never held a point has no block yet: room for the costs alone
        if (map_mem.alloc(&map_out, old ? map_out_bytes(map_cap, true) : 16)) { map_out = old; return -1; }
        map_mem.release(old);
        return 0;
    }
};
}  // extern "C++"

namespace {
// features of one image (steps 1-4 of the definition): nine launches, no synchronisation
int feat_pass(ps_feat* f, PsFeatImage& im, int h, int w, const ps_feat_params& p) {
    const dim3 grid(cdiv(w, PS_FEAT_TX), cdiv(h, PS_FEAT_TY));
    const int n = h * w, nb = cdiv(n, 256), rb = cdiv(f->raw_cap, 256);
    hipStream_t s = f->stream;
    hipLaunchKernelGGL(k_feat_sobel, grid, dim3(256), 0, s, (const uint8_t*)im.img, h, w, im.du, im.dv);
    hipLaunchKernelGGL(k_feat_response, grid, dim3(256), 0, s, (const short*)im.du, (const short*)im.dv, h, w, f->R);
    hipLaunchKernelGGL(k_feat_nms, grid, dim3(256), 0, s, (const long long*)f->R, h, w, (int)p.nms_n, (long long)p.response_threshold, f->flags);
    hipLaunchKernelGGL(k_feat_count, dim3(nb), dim3(256), 0, s, n, (const uint8_t*)f->flags, f->counts);
    hipLaunchKernelGGL(k_dense_scan, dim3(1), dim3(1024), 0, s, nb, f->counts, f->n_raw);
    hipLaunchKernelGGL(k_feat_compact_pix, dim3(nb), dim3(256), 0, s, n, w, (const uint8_t*)f->flags, (const int*)f->counts,
                       (const long long*)f->R, f->raw_cap, f->raw_uv, f->raw_R);
    hipLaunchKernelGGL(k_feat_rank, dim3(rb), dim3(256), 0, s, (const int*)f->n_raw, f->raw_cap, (const long long*)f->raw_R,
                       (int)p.max_features, f->keep);
    hipLaunchKernelGGL(k_feat_count, dim3(rb), dim3(256), 0, s, f->raw_cap, (const uint8_t*)f->keep, f->counts);
    hipLaunchKernelGGL(k_dense_scan, dim3(1), dim3(1024), 0, s, rb, f->counts, im.n);
    hipLaunchKernelGGL(k_feat_compact_feat, dim3(rb), dim3(256), 0, s, f->raw_cap, (const uint8_t*)f->keep, (const int*)f->counts,
                       (const int2*)f->raw_uv, (const long long*)f->raw_R, (const short*)im.du, (const short*)im.dv, h, w,
                       (int)p.max_features, im.uv, im.R, im.desc);
    hipLaunchKernelGGL(k_feat_rowstart, dim3(cdiv(h + 1, 256)), dim3(256), 0, s, h, (const int*)im.n, (int)p.max_features,
                       (const int2*)im.uv, im.row_start);
    HIP_OK(hipGetLastError());
    f->feature_passes += 1;
    return 0;
}

int feat_frame_features(ps_feat* f, PsFeatFrame& fr, const ps_feat_params& p) {
    if (fr.features_ok && fr.det_threshold == p.response_threshold && fr.det_nms == p.nms_n && fr.det_max == p.max_features) return 0;
    for (int k = 0; k <= fr.stereo; ++k)
        if (feat_pass(f, fr.im[k], fr.h, fr.w, p)) return -1;
    fr.features_ok = true;
    fr.det_threshold = p.response_threshold; fr.det_nms = p.nms_n; fr.det_max = p.max_features;
    return 0;
}

void feat_leg(ps_feat* f, const PsFeatImage& A, const PsFeatImage& B, int h, const ps_feat_params& p, int kind, int* out) {
    // kind 0 temporal, 1 left -> right (u_left - u_right in 0 .. disp_max), 2 right -> left
    const int du_lo = kind == 0 ? -p.match_radius_u : (kind == 1 ? -p.disp_max : 0);
    const int du_hi = kind == 0 ? p.match_radius_u : (kind == 1 ? 0 : p.disp_max);
    const int dv = kind == 0 ? p.match_radius_v : 1;
    hipLaunchKernelGGL(k_feat_match, dim3(cdiv((long)p.max_features * 64, 256)), dim3(256), 0, f->stream, A.list(), B.list(), h,
                       (int)p.max_features, du_lo, du_hi, -dv, dv, (int)p.match_cost_max, out);
}
}  // namespace

int ps_feat_create(int32_t max_height, int32_t max_width, int32_t max_features, void* stream, ps_feat** out) {
    if (!out) return fail("null argument");
    *out = nullptr;
    if (max_height < 1 || max_width < 1 || (int64_t)max_height * max_width > (1 << 28)) return fail("frame size out of range");
    if (max_features < 1 || max_features > (1 << 20)) return fail("max_features must be 1 .. 2^20");
    if (need_device()) return -1;
    std::unique_ptr<ps_feat> f(new ps_feat);
    f->stream = (hipStream_t)stream;
    f->max_h = max_height; f->max_w = max_width; f->max_features = max_features;
    // non-maximum suppression with nms_n >= 1 leaves at most one feature in every aligned 2 x 2 block
    f->raw_cap = cdiv(max_height, 2) * cdiv(max_width, 2);
    const size_t P = (size_t)max_height * max_width, M = max_features, Rc = f->raw_cap;
    DevMem& D = f->mem;
    for (PsFeatFrame& fr : f->frame)
        for (PsFeatImage& im : fr.im)
            if (D.alloc(&im.img, P) || D.alloc(&im.du, P) || D.alloc(&im.dv, P) || D.alloc(&im.uv, M) || D.alloc(&im.R, M) ||
                D.alloc(&im.desc, 8 * M) || D.alloc(&im.row_start, (size_t)max_height + 1) || D.alloc(&im.n, 1)) return -1;
    if (D.alloc(&f->R, P) || D.alloc(&f->raw_R, Rc) || D.alloc(&f->flags, P) || D.alloc(&f->keep, Rc) || D.alloc(&f->mflags, M) ||
        D.alloc(&f->counts, (size_t)cdiv((long)std::max(P, std::max(Rc, M)), 256) + 1) || D.alloc(&f->n_raw, 1) ||
        D.alloc(&f->visited, 4 * M) || D.alloc(&f->idx4, 4 * M) || D.alloc(&f->n_match, 1) || D.alloc(&f->raw_uv, Rc) ||
        D.alloc(&f->m8, 8 * M)) return -1;
    for (int k = 0; k < 4; ++k)
        if (D.alloc(&f->leg[k], M)) return -1;
    *out = f.release();
    return 0;
}

int ps_feat_destroy(ps_feat* f) {
    if (!f) return 0;
    if (f->stream) hipStreamSynchronize(f->stream); else hipDeviceSynchronize();
    delete f;
    return 0;
}

int ps_feat_push(ps_feat* f, int32_t height, int32_t width, const uint8_t* left, const uint8_t* right) {
    if (!f || !left) return fail("null argument");
    if (height < 1 || width < 1 || height > f->max_h || width > f->max_w) return fail("frame size outside the handle's capacity");
    const size_t n = (size_t)height * width;
    const int stereo = right ? 1 : 0;
    int s = -1;
    for (int k = 0; k < 3 && s < 0; ++k) {
        const PsFeatFrame& fr = f->frame[k];
        if (fr.held && fr.h == height && fr.w == width && fr.stereo == stereo && !memcmp(fr.host[0].data(), left, n) &&
            (!stereo || !memcmp(fr.host[1].data(), right, n))) s = k;
    }
    if (s < 0) {                                           // least recently used slot that is not the current frame
        for (int k = 0; k < 3; ++k)
            if (k != f->cur && (s < 0 || f->frame[k].used < f->frame[s].used)) s = k;
        PsFeatFrame& fr = f->frame[s];
        fr.h = height; fr.w = width; fr.stereo = stereo; fr.held = true; fr.features_ok = false;
        const uint8_t* src[2] = {left, right};
        for (int k = 0; k <= stereo; ++k) {
            fr.host[k].assign(src[k], src[k] + n);        // the upload reads this copy: the caller's buffer is free on return
            HIP_OK(hipMemcpyAsync(fr.im[k].img, fr.host[k].data(), n, hipMemcpyHostToDevice, f->stream));
        }
    }
    f->frame[s].used = ++f->clock;
    f->prev = f->cur;
    f->cur = s;
    return 0;
}

int ps_feat_match(ps_feat* f, int32_t mode, const ps_feat_params* params, int32_t* num_matches) {
    if (!f || !params || !num_matches) return fail("null argument");
    *num_matches = 0;
    const ps_feat_params& p = *params;
    if (mode < 0 || mode > 2) return fail("matching mode must be 0 (flow), 1 (stereo) or 2 (quad)");
    if (p.nms_n < 1 || p.nms_n > 3) return fail("nms_n must be 1..3");
    if (p.max_features < 1 || p.max_features > f->max_features) return fail("max_features outside the handle's capacity");
    if (p.match_radius_u < 0 || p.match_radius_v < 0 || p.disp_max < 0) return fail("negative matching window");
    if (f->cur < 0 || (mode != 1 && f->prev < 0)) return fail("push the frames before matching");
    PsFeatFrame& C = f->frame[f->cur];
    PsFeatFrame& P = f->frame[mode == 1 ? f->cur : f->prev];
    if (mode != 0 && (!C.stereo || !P.stereo)) return fail("stereo and quad matching need right images");
    if (P.h != C.h || P.w != C.w) return fail("the two frames differ in size");
    if (feat_frame_features(f, P, p) || feat_frame_features(f, C, p)) return -1;
    const int h = C.h, w = C.w, M = p.max_features, mb = cdiv(M, 256);
    // the images a chain visits: flow 1p 1c, stereo 1c 2c, quad 1p 2p 2c 1c
    const PsFeatImage* node[4];
    FeatChain ch{};
    if (mode == 0) {
        ch.legs = 2; node[0] = &P.im[0]; node[1] = &C.im[0]; ch.col[0] = 0; ch.col[1] = 2; ch.temporal[1] = 1;
        feat_leg(f, *node[0], *node[1], h, p, 0, f->leg[0]);
        feat_leg(f, *node[1], *node[0], h, p, 0, f->leg[1]);
    } else if (mode == 1) {
        ch.legs = 2; node[0] = &C.im[0]; node[1] = &C.im[1]; ch.col[0] = 2; ch.col[1] = 3; ch.temporal[1] = 0;
        feat_leg(f, *node[0], *node[1], h, p, 1, f->leg[0]);
        feat_leg(f, *node[1], *node[0], h, p, 2, f->leg[1]);
    } else {
        ch.legs = 4; node[0] = &P.im[0]; node[1] = &P.im[1]; node[2] = &C.im[1]; node[3] = &C.im[0];
        ch.col[0] = 0; ch.col[1] = 1; ch.col[2] = 3; ch.col[3] = 2; ch.temporal[1] = 0; ch.temporal[2] = 1; ch.temporal[3] = 0;
        feat_leg(f, *node[0], *node[1], h, p, 1, f->leg[0]);
        feat_leg(f, *node[1], *node[2], h, p, 0, f->leg[1]);
        feat_leg(f, *node[2], *node[3], h, p, 2, f->leg[2]);
        feat_leg(f, *node[3], *node[0], h, p, 0, f->leg[3]);
    }
    if (ch.legs == 2) { node[2] = node[0]; node[3] = node[1]; }
    hipStream_t s = f->stream;
    hipLaunchKernelGGL(k_feat_chain, dim3(mb), dim3(256), 0, s, (const int*)node[0]->n, M, ch.legs, (const int*)f->leg[0],
                       (const int*)f->leg[1], (const int*)f->leg[2], (const int*)f->leg[3], f->mflags, f->visited);
    hipLaunchKernelGGL(k_feat_count, dim3(mb), dim3(256), 0, s, M, (const uint8_t*)f->mflags, f->counts);
    hipLaunchKernelGGL(k_dense_scan, dim3(1), dim3(1024), 0, s, mb, f->counts, f->n_match);
    hipLaunchKernelGGL(k_feat_compact_match, dim3(mb), dim3(256), 0, s, M, (const uint8_t*)f->mflags, (const int*)f->counts,
                       (const int*)f->visited, ch, f->idx4);
    hipLaunchKernelGGL(k_feat_subpix, dim3(mb), dim3(256), 0, s, (const int*)f->n_match, M, (const int*)f->idx4, ch, node[0]->list(),
                       node[1]->list(), node[2]->list(), node[3]->list(), h, w, (int)p.refinement, f->m8);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&f->h_n_match, f->n_match, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    *num_matches = f->h_n_match;
    return 0;
}

int ps_feat_read_matches(ps_feat* f, int32_t num_matches, double* matches8, int32_t* indices4) {
    if (!f) return fail("null handle");
    if (num_matches < 0 || num_matches > f->h_n_match) return fail("more matches asked for than the last ps_feat_match found");
    if (matches8) HIP_OK(hipMemcpyAsync(matches8, f->m8, (size_t)num_matches * 8 * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    if (indices4) HIP_OK(hipMemcpyAsync(indices4, f->idx4, (size_t)num_matches * 4 * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    HIP_OK(hipStreamSynchronize(f->stream));
    return 0;
}

int ps_feat_set_map(ps_feat* f, int32_t num_points, const double* points_w, const uint8_t* descriptors) {
    if (!f) return fail("null handle");
    if (num_points < 0 || num_points > (1 << 20)) return fail("num_points must be 0 .. 2^20");
    if (num_points > 0 && (!points_w || !descriptors)) return fail("null argument");
    hipStream_t s = f->stream;
    if (!f->map_claim && f->mem.alloc(&f->map_claim, (size_t)f->max_features)) return -1;
    if (num_points > f->map_cap) {
        HIP_OK(hipStreamSynchronize(s));                   // a match of the old map may still read its buffers
        f->free_map();
        f->map_set = false;
        const size_t n = num_points;
        if (f->map_mem.alloc(&f->map_pts, 3 * n) || f->map_mem.alloc(&f->map_desc, 8 * n) ||
            f->map_mem.alloc(&f->map_out, ps_feat::map_out_bytes(n, f->map_global_used))) {
            f->free_map();
            return -1;
        }
        f->map_cap = num_points;
    }
    if (num_points > 0) {
        HIP_OK(hipMemcpyAsync(f->map_pts, points_w, (size_t)num_points * 3 * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(f->map_desc, descriptors, (size_t)num_points * 32, hipMemcpyHostToDevice, s));
        HIP_OK(hipStreamSynchronize(s));                   // the caller's arrays are free on return
    }
    f->map_n = num_points;
    f->map_set = true;
    f->map_matched_n = -1;
    return 0;
}

int ps_feat_match_map(ps_feat* f, const double* T_cw, const double* cam5, int32_t radius, const ps_feat_params* params,
                      int32_t* num_matched) {
    if (!f || !T_cw || !cam5 || !params || !num_matched) return fail("null argument");
    *num_matched = 0;
    const ps_feat_params& p = *params;
    if (p.nms_n < 1 || p.nms_n > 3) return fail("nms_n must be 1..3");
    if (p.max_features < 1 || p.max_features > f->max_features) return fail("max_features outside the handle's capacity");
    if (radius < 0) return fail("negative matching radius");
    if (f->cur < 0) return fail("push a frame before matching the map");
    if (!f->map_set) return fail("set a map before matching it");
    PsFeatFrame& Cf = f->frame[f->cur];
    if (feat_frame_features(f, Cf, p)) return -1;
    f->map_matched_n = f->map_n;
    f->map_matched_global = false;
    f->h_n_map_matched = 0;
    const int N = f->map_n, h = Cf.h, w = Cf.w;
    if (N == 0) return 0;
    FeatMapView V;
    for (int k = 0; k < 12; ++k) V.T[k] = T_cw[k];
    V.cu = cam5[0]; V.cv = cam5[1]; V.fu = cam5[2]; V.fv = cam5[3];
    // one block for everything that goes back: the count, then the four arrays (doubles first: aligned)
    uint8_t* o = f->map_out;
    const size_t n = N, total = 16 + 28 * n;
    int* count = (int*)o;
    const FeatMapOut out{(int*)(o + 16 + 16 * n), (int*)(o + 16 + 20 * n), (int*)(o + 16 + 24 * n), (double*)(o + 16)};
    const int r = std::min((int)radius, std::max(h, w));   // a window over the whole image is as large as it gets
    hipStream_t s = f->stream;
    HIP_OK(hipMemsetAsync(f->map_claim, 0xff, (size_t)f->max_features * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_feat_map_search, dim3(cdiv((long)N * 64, 256)), dim3(256), 0, s, N, (const double*)f->map_pts,
                       (const uint32_t*)f->map_desc, V, Cf.im[0].list(), h, w, (int)p.max_features, r, (int)p.match_cost_max, out,
                       f->map_claim, count);
    hipLaunchKernelGGL(k_feat_map_resolve, dim3(cdiv(N, 256)), dim3(256), 0, s, N, (const uint32_t*)f->map_desc, Cf.im[0].list(), h, w,
                       (int)p.max_features, (int)p.refinement, out, (const unsigned long long*)f->map_claim, count);
    HIP_OK(hipGetLastError());
    f->h_map_out.resize(total);
    HIP_OK(hipMemcpyAsync(f->h_map_out.data(), o, total, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    memcpy(&f->h_n_map_matched, f->h_map_out.data(), sizeof(int));
    *num_matched = f->h_n_map_matched;
    return 0;
}

int ps_feat_read_map_matches(ps_feat* f, int32_t num_points, int32_t* feature, int32_t* status, int32_t* cost, double* uv) {
    if (!f) return fail("null handle");
    if (f->map_matched_n < 0) return fail("match the map before reading its matches");
    if (num_points < 0 || num_points > f->map_matched_n) return fail("more points asked for than the map that was matched holds");
    const size_t n = num_points, N = f->map_matched_n;
    if (n == 0) return 0;
    const uint8_t* o = f->h_map_out.data();                // the match brought everything to the host already
    if (uv) memcpy(uv, o + 16, n * 2 * sizeof(double));
    if (feature) memcpy(feature, o + 16 + 16 * N, n * sizeof(int));
    if (status) memcpy(status, o + 16 + 20 * N, n * sizeof(int));
    if (cost) memcpy(cost, o + 16 + 24 * N, n * sizeof(int));
    return 0;
}

int ps_feat_match_map_global(ps_feat* f, int32_t ratio_num, int32_t ratio_den, const ps_feat_params* params, int32_t* num_matched) {
    if (!f || !params || !num_matched) return fail("null argument");
    *num_matched = 0;
    const ps_feat_params& p = *params;
    if (p.nms_n < 1 || p.nms_n > 3) return fail("nms_n must be 1..3");
    if (p.max_features < 1 || p.max_features > f->max_features) return fail("max_features outside the handle's capacity");
    if (ratio_num < 1 || ratio_num > ratio_den || ratio_den > 32768) return fail("the ratio must satisfy 0 < num <= den <= 32768");
    if (f->cur < 0) return fail("push a frame before matching the map");
    if (!f->map_set) return fail("set a map before matching it");
    PsFeatFrame& Cf = f->frame[f->cur];
    if (feat_frame_features(f, Cf, p)) return -1;
    if (!f->map_global_used) {
        HIP_OK(hipStreamSynchronize(f->stream));           // nothing in flight reads the block that is replaced
        if (f->grow_map_out_for_second()) return -1;
        f->map_global_used = true;
    }
    f->map_matched_n = f->map_n;
    f->map_matched_global = true;
    f->h_n_map_matched = 0;
    const int N = f->map_n, h = Cf.h, w = Cf.w;
    if (N == 0) return 0;
    // the block of ps_feat_match_map with the second-best costs behind it
    uint8_t* o = f->map_out;
    const size_t n = N, total = 16 + 32 * n;
    int* count = (int*)o;
    const FeatMapOut out{(int*)(o + 16 + 16 * n), (int*)(o + 16 + 20 * n), (int*)(o + 16 + 24 * n), (double*)(o + 16)};
    hipStream_t s = f->stream;
    HIP_OK(hipMemsetAsync(f->map_claim, 0xff, (size_t)f->max_features * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_feat_map_search_all, dim3(cdiv(N, 64)), dim3(256), 0, s, N, (const uint32_t*)f->map_desc, Cf.im[0].list(),
                       (int)p.max_features, (int)p.match_cost_max, (int)ratio_num, (int)ratio_den, out, (int*)(o + 16 + 28 * n),
                       f->map_claim, count);
    hipLaunchKernelGGL(k_feat_map_resolve, dim3(cdiv(N, 256)), dim3(256), 0, s, N, (const uint32_t*)f->map_desc, Cf.im[0].list(), h, w,
                       (int)p.max_features, (int)p.refinement, out, (const unsigned long long*)f->map_claim, count);
    HIP_OK(hipGetLastError());
    f->h_map_out.resize(total);
    HIP_OK(hipMemcpyAsync(f->h_map_out.data(), o, total, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    memcpy(&f->h_n_map_matched, f->h_map_out.data(), sizeof(int));
    *num_matched = f->h_n_map_matched;
    return 0;
}

int ps_feat_read_map_second(ps_feat* f, int32_t num_points, int32_t* second) {
    if (!f) return fail("null handle");
    if (f->map_matched_n < 0 || !f->map_matched_global) return fail("the last map match was not a global one: no second-best costs");
    if (num_points < 0 || num_points > f->map_matched_n) return fail("more points asked for than the map that was matched holds");
    const size_t n = num_points, N = f->map_matched_n;
    if (n && second) memcpy(second, f->h_map_out.data() + 16 + 28 * N, n * sizeof(int));
    return 0;
}

int ps_feat_db_add(ps_feat* f, int32_t num, const uint8_t* descriptors, int32_t* entry) {
    if (!f || !entry) return fail("null argument");
    *entry = -1;
    if (num < 0) return fail("num must not be negative");
    if (num > 0 && !descriptors) return fail("null argument");
    const int K = (int)f->db_start.size();
    if (K >= PS_FEAT_DB_MAX_ENTRIES) return fail("the database holds at most 65536 entries");
    if (f->db_n + num > PS_FEAT_DB_MAX_DESC) return fail("the database holds at most 2^22 descriptors");
    hipStream_t s = f->stream;
    const int nb0 = K ? f->db_block.back() : 0, nb = cdiv(num, PS_FEAT_DB_BLOCK);
    int64_t dc = f->db_desc_cap, bc = f->db_block_cap, ec = f->db_entry_cap;
    if (f->db_n + num > dc || nb0 + nb > bc || K + 1 > ec) {
        HIP_OK(hipStreamSynchronize(s));                   // a query may still read the buffers that are replaced
        int64_t ec2 = ec;
        if (f->grow_db(&f->db_desc, 8 * f->db_n, 8 * dc, 8 * (f->db_n + num), 8 * 1024, &dc) ||
            f->grow_db(&f->db_blocks, nb0, bc, nb0 + nb, 64, &bc) || f->grow_db(&f->db_estart, K, ec, K + 1, 64, &ec2) ||
            f->grow_db(&f->db_elen, K, ec, K + 1, 64, &ec2) || f->grow_db(&f->db_score, 0, ec, K + 1, 64, &ec2)) return -1;
        f->db_desc_cap = dc / 8; f->db_block_cap = (int)bc; f->db_entry_cap = (int)ec2;
    }
    const int start = (int)f->db_n;
    std::vector<FeatDbBlock> blocks(nb);
    for (int b = 0; b < nb; ++b) blocks[b] = FeatDbBlock{K, start + PS_FEAT_DB_BLOCK * b};
    const int se[2] = {start, (int)num};
    if (num > 0) {
        HIP_OK(hipMemcpyAsync(f->db_desc + 8 * (size_t)start, descriptors, (size_t)num * 32, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(f->db_blocks + nb0, blocks.data(), (size_t)nb * sizeof(FeatDbBlock), hipMemcpyHostToDevice, s));
    }
    HIP_OK(hipMemcpyAsync(f->db_estart + K, &se[0], sizeof(int), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(f->db_elen + K, &se[1], sizeof(int), hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));                       // the caller's array is free on return
    if (!K) f->db_block.assign(1, 0);
    f->db_start.push_back(start); f->db_len.push_back(num); f->db_block.push_back(nb0 + nb);
    f->db_n += num;
    *entry = K;
    return 0;
}

int ps_feat_db_clear(ps_feat* f) {
    if (!f) return fail("null handle");
    f->db_start.clear(); f->db_len.clear(); f->db_block.clear();
    f->db_n = 0;
    return 0;
}

int ps_feat_db_size(ps_feat* f, int32_t* entries, int64_t* descriptors) {
    if (!f || !entries || !descriptors) return fail("null argument");
    *entries = (int32_t)f->db_start.size();
    *descriptors = f->db_n;
    return 0;
}

int ps_feat_db_query(ps_feat* f, int32_t first, int32_t last, int32_t ratio_num, int32_t ratio_den, const ps_feat_params* params,
                     int32_t* scores) {
    if (!f || !params || !scores) return fail("null argument");
    const ps_feat_params& p = *params;
    const int K = (int)f->db_start.size();
    if (first < 0 || first > last || last > K) return fail("the entry range must satisfy 0 <= first <= last <= entries");
    if (ratio_num < 1 || ratio_num > ratio_den || ratio_den > 32768) return fail("the ratio must satisfy 0 < num <= den <= 32768");
    if (p.nms_n < 1 || p.nms_n > 3) return fail("nms_n must be 1..3");
    if (p.max_features < 1 || p.max_features > f->max_features) return fail("max_features outside the handle's capacity");
    if (f->cur < 0) return fail("push a frame before querying the database");
    PsFeatFrame& Cf = f->frame[f->cur];
    if (feat_frame_features(f, Cf, p)) return -1;
    if (first == last) return 0;                           // a query of nothing (the feature pass waits for whoever needs it)
    hipStream_t s = f->stream;
    const int n = last - first, b0 = f->db_block[first], nb = f->db_block[last] - b0;
    HIP_OK(hipMemsetAsync(f->db_score, 0, (size_t)n * sizeof(int), s));
    if (nb > 0)
        hipLaunchKernelGGL(k_feat_db_search, dim3(nb), dim3(256), 0, s, (const FeatDbBlock*)(f->db_blocks + b0), (const int*)f->db_estart,
                           (const int*)f->db_elen, (int)first, (const uint32_t*)f->db_desc, Cf.im[0].list(), (int)p.max_features,
                           (int)p.match_cost_max, (int)ratio_num, (int)ratio_den, f->db_score);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(scores, f->db_score, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return 0;
}

int ps_feat_read_features(ps_feat* f, int32_t which, int32_t capacity, int32_t* num_features, int32_t* uv, int64_t* response,
                          uint8_t* descriptors) {
    if (!f || !num_features) return fail("null argument");
    if (which < 0 || which > 3) return fail("which must be 0 (previous left), 1 (previous right), 2 (current left) or 3 (current right)");
    const int slot = which < 2 ? f->prev : f->cur;
    if (slot < 0) return fail("no such frame");
    const PsFeatFrame& fr = f->frame[slot];
    if (!fr.features_ok || ((which & 1) && !fr.stereo)) return fail("the image has no features: match first");
    const PsFeatImage& im = fr.im[which & 1];
    int n = 0;
    HIP_OK(hipMemcpyAsync(&n, im.n, sizeof(int), hipMemcpyDeviceToHost, f->stream));
    HIP_OK(hipStreamSynchronize(f->stream));
    *num_features = n;
    const size_t m = (size_t)std::min(n, capacity < 0 ? 0 : capacity);
    if (uv) HIP_OK(hipMemcpyAsync(uv, im.uv, m * 2 * sizeof(int), hipMemcpyDeviceToHost, f->stream));
    if (response) HIP_OK(hipMemcpyAsync(response, im.R, m * sizeof(long long), hipMemcpyDeviceToHost, f->stream));
    if (descriptors) HIP_OK(hipMemcpyAsync(descriptors, im.desc, m * 32, hipMemcpyDeviceToHost, f->stream));
    HIP_OK(hipStreamSynchronize(f->stream));
    return 0;
}

int ps_feat_feature_passes(ps_feat* f, int64_t* passes) {
    if (!f || !passes) return fail("null argument");
    *passes = f->feature_passes;
    return 0;
}

int ps_feat_device_bytes(ps_feat* f, int64_t* bytes) {
    if (!f || !bytes) return fail("null argument");
    *bytes = f->mem.bytes() + f->map_mem.bytes() + f->db_mem.bytes();
    return 0;
}
