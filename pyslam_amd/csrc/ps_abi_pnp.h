// ps_abi_pnp.h -- C ABI: absolute-pose (PnP) RANSAC, registration of a monocular frame against the map (kernels: ps_k_pnp.h).
// Part of ps_core.hip (inside its extern "C" block, after ps_host_ransac.h, which holds the host side the front ends share).
// Stateless; host pointers in, host pointers out.

extern "C++" {
namespace {
struct PnpLayout {                   // the parts of a call's device block (RcBlock)
    size_t pts, obs, cam, idx;                                      // in: pts_w (3 N) | obs (2 N) | cam (8) doubles | samples (3 H int32)
    size_t bear, T_best;                                            // work space
    size_t model, counts, flags;                                    // hyp: T_all (64 H doubles) | counts (4 H int32) | flags (4 H bytes)
    size_t result, info, mask;                                      // out: result (16 + iters + 1 + N doubles, padded to even) | info (8 int32) | mask (N bytes)
    RcSpan in, hyp, out;                                            // the upload, ps_pnp_hypotheses' download, ps_pnp_ransac's
    size_t total;
    PnpLayout(size_t N, size_t H, size_t iters) {
        RcBlock B;
        pts = B.part(3 * N * F64); obs = B.pack(2 * N * F64); cam = B.pack(8 * F64); idx = B.pack(3 * H * I32);
        in = B.span(pts);
        bear = B.part(3 * N * F64); T_best = B.part(16 * F64);
        model = B.part(64 * H * F64); counts = B.pack(4 * H * I32); flags = B.pack(4 * H);      // (scoring: room for the 16 H given doubles)
        hyp = B.span(model);
        const size_t nres = 16 + iters + 1 + N;
        result = B.part((nres + (nres & 1)) * F64); info = B.pack(8 * I32); mask = B.pack(N);
        out = B.span(result);
        total = B.part(0);
    }
};

int pnp_check(const double* pts_w, const double* obs, int32_t num_pts, const double* cam5, const char* who) {
    if (!pts_w || !obs || !cam5) return rc_fail(who, "bad argument");
    if (num_pts < 3) return rc_fail(who, "an absolute pose needs at least 3 points");
    return rc_check_camera(cam5, who);
}

// uploads pts_w | obs | cam | idx (idx may be NULL) and runs k_pnp_normalise
int pnp_begin(const PnpLayout& L, char* d, const double* pts_w, const double* obs, int32_t num_pts, const double* cam5,
              const int32_t* idx, int32_t num_hyp) {
    const RcCam cam(cam5);
    if (rc_upload(d, L.in, {{L.pts, pts_w, 3 * F64 * num_pts}, {L.obs, obs, 2 * F64 * num_pts}, {L.cam, cam.v, sizeof(cam.v)},
                            {L.idx, idx, 3 * I32 * num_hyp}})) return -1;
    hipLaunchKernelGGL(k_pnp_normalise, dim3(cdiv(num_pts, 256)), dim3(256), 0, 0, num_pts, (const double*)(d + L.obs),
                       (const double*)(d + L.cam), (double*)(d + L.bear));
    return 0;
}

// k_pnp_hypotheses on the uploaded samples (masks == NULL) or, scoring, on the poses at L.model
void pnp_hypotheses(const PnpLayout& L, char* d, int32_t num_pts, int32_t num_hyp, double thresh, uint8_t* masks) {
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3(num_hyp), dim3(256), 0, 0, num_pts, masks ? (const int32_t*)nullptr : (const int32_t*)(d + L.idx),
                       (const double*)(d + L.pts), (const double*)(d + L.obs), (const double*)(d + L.bear), (const double*)(d + L.cam), thresh,
                       (double*)(d + L.model), (int32_t*)(d + L.counts), masks ? (uint8_t*)nullptr : (uint8_t*)(d + L.flags), masks);
}
}  // namespace
}  // extern "C++"

int ps_pnp_hypotheses(const double* pts_w, const double* obs, int32_t num_pts, const int32_t* sample_idx, int32_t num_hyp,
                      const double* cam5, double thresh, double* T_all, int32_t* counts, uint8_t* empty) {
    if (pnp_check(pts_w, obs, num_pts, cam5, "ps_pnp_hypotheses") ||
        rc_check_samples(sample_idx, num_hyp, 3, num_pts, "ps_pnp_hypotheses")) return -1;
    const PnpLayout L((size_t)num_pts, (size_t)num_hyp, 0);
    return rc_hypotheses_call(
        L, [&](char* d) { return pnp_begin(L, d, pts_w, obs, num_pts, cam5, sample_idx, num_hyp); },
        [&](char* d) { pnp_hypotheses(L, d, num_pts, num_hyp, thresh, nullptr); },
        {{L.model, T_all, 64 * F64 * num_hyp}, {L.counts, counts, 4 * I32 * num_hyp}, {L.flags, empty, 4 * (size_t)num_hyp}});
}

int ps_pnp_score(const double* T, int32_t num_T, const double* pts_w, const double* obs, int32_t num_pts, const double* cam5,
                 double thresh, uint8_t* masks, int32_t* counts) {
    if (!T || num_T < 0) return fail("ps_pnp_score: bad argument");
    if (pnp_check(pts_w, obs, num_pts, cam5, "ps_pnp_score")) return -1;
    if (num_T == 0) return 0;
    const PnpLayout L((size_t)num_pts, (size_t)num_T, 0);
    return rc_score_call(
        L, T, 16 * F64 * num_T, num_T, num_pts, masks, counts,
        [&](char* d) { return pnp_begin(L, d, pts_w, obs, num_pts, cam5, nullptr, num_T); },
        [&](char* d, uint8_t* dmasks) { pnp_hypotheses(L, d, num_pts, num_T, thresh, dmasks); });
}

int ps_pnp_ransac(const double* pts_w, const double* obs, int32_t num_pts, const int32_t* sample_idx, int32_t num_hyp,
                  const double* cam5, double thresh, int32_t refine_iters, double* T_cw, uint8_t* mask, int32_t* info,
                  double* sq_err, double* cost_history) {
    if (pnp_check(pts_w, obs, num_pts, cam5, "ps_pnp_ransac") ||
        rc_check_samples(sample_idx, num_hyp, 3, num_pts, "ps_pnp_ransac")) return -1;
    if (refine_iters < 0 || refine_iters > 1000) return fail("ps_pnp_ransac: refine_iters must lie in 0..1000");
    const PnpLayout L((size_t)num_pts, (size_t)num_hyp, (size_t)refine_iters);
    DevBuf buf;
    if (need_device() || buf.get(L.total)) return -1;
    char* d = buf.as<char>();
    if (pnp_begin(L, d, pts_w, obs, num_pts, cam5, sample_idx, num_hyp)) return -1;
    const double* pts = (const double*)(d + L.pts);
    const double* ob = (const double*)(d + L.obs);
    const double* cam = (const double*)(d + L.cam);
    pnp_hypotheses(L, d, num_pts, num_hyp, thresh, nullptr);
    hipLaunchKernelGGL(k_pnp_best, dim3(1), dim3(256), 0, 0, 4 * num_hyp, num_pts, (const int32_t*)(d + L.counts),
                       (const double*)(d + L.model), pts, ob, cam, thresh, (int32_t*)(d + L.info), (double*)(d + L.T_best),
                       (uint8_t*)(d + L.mask));
    hipLaunchKernelGGL(k_pnp_refine, dim3(1), dim3(256), 0, 0, num_pts, refine_iters, pts, ob, cam, thresh, (const double*)(d + L.T_best),
                       (uint8_t*)(d + L.mask), (int32_t*)(d + L.info), (double*)(d + L.result));
    const size_t nh = (size_t)refine_iters + 1;
    return rc_download(d, L.out, {{L.result, T_cw, 16 * F64}, {L.result + 16 * F64, cost_history, nh * F64},
                                  {L.result + (16 + nh) * F64, sq_err, num_pts * F64}, {L.info, info, 8 * I32}, {L.mask, mask, (size_t)num_pts}});
}
