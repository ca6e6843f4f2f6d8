// ps_abi_twoview.h -- C ABI: monocular two-view initialisation, essential-matrix RANSAC (kernels: ps_k_twoview.h).
// Part of ps_core.hip (inside its extern "C" block, after ps_host_ransac.h, which holds the host side the front ends share).
// Stateless; host pointers in, host pointers out.

extern "C++" {
namespace {
struct TvLayout {                    // the parts of a call's device block (RcBlock)
    size_t obs1, obs2, cam, idx;                                    // in: obs_1 (2 N) | obs_2 (2 N) | cam (8) doubles | samples (8 H int32)
    size_t xn, E_best, partA, partB, partC, mask_refit;             // work space
    size_t model, counts, flags;                                    // hyp: E_all (9 H doubles) | counts (H int32) | flags (H bytes)
    size_t result, info, mask;                                      // out: result (26 + N doubles, padded to even) | info (8 int32) | mask (N bytes)
    RcSpan in, hyp, out;                                            // the upload, ps_twoview_hypotheses' download, ps_twoview_ransac's
    size_t total;
    int G;
    TvLayout(size_t N, size_t H) : G((int)((N + 255) / 256)) {
        RcBlock B;
        obs1 = B.part(2 * N * F64); obs2 = B.pack(2 * N * F64); cam = B.pack(8 * F64); idx = B.pack(8 * H * I32);
        in = B.span(obs1);
        xn = B.part(4 * N * F64); E_best = B.part(16 * F64); mask_refit = B.part(N);
        partA = B.part(8 * G * F64); partB = B.part(2 * G * F64); partC = B.part(45 * G * F64);
        model = B.part(9 * H * F64); counts = B.pack(H * I32); flags = B.pack(H);
        hyp = B.span(model);
        result = B.part((26 + N + (N & 1)) * F64); info = B.pack(8 * I32); mask = B.pack(N);
        out = B.span(result);
        total = B.part(0);
    }
};

int tv_check(const double* obs_1, const double* obs_2, int32_t num_pts, const double* cam5, const char* who) {
    if (!obs_1 || !obs_2 || !cam5 || num_pts <= 0) return rc_fail(who, "bad argument");
    return rc_check_camera(cam5, who);
}

// uploads obs_1 | obs_2 | cam | idx (idx may be NULL) and runs k_tv_normalise
int tv_begin(const TvLayout& L, char* d, const double* obs_1, const double* obs_2, int32_t num_pts, const double* cam5,
             const int32_t* idx, int32_t num_hyp) {
    const RcCam cam(cam5);
    const size_t ob = 2 * F64 * num_pts;
    if (rc_upload(d, L.in, {{L.obs1, obs_1, ob}, {L.obs2, obs_2, ob}, {L.cam, cam.v, sizeof(cam.v)}, {L.idx, idx, 8 * I32 * num_hyp}})) return -1;
    hipLaunchKernelGGL(k_tv_normalise, dim3(cdiv(num_pts, 256)), dim3(256), 0, 0, num_pts, (const double*)(d + L.obs1),
                       (const double*)(d + L.obs2), (const double*)(d + L.cam), (double4*)(d + L.xn));
    return 0;
}

// k_tv_hypotheses on the uploaded samples (masks == NULL) or, scoring, on the matrices at L.model
void tv_hypotheses(const TvLayout& L, char* d, int32_t num_pts, int32_t num_hyp, double thresh, uint8_t* masks) {
    hipLaunchKernelGGL(k_tv_hypotheses, dim3(num_hyp), dim3(256), 0, 0, num_pts, masks ? (const int32_t*)nullptr : (const int32_t*)(d + L.idx),
                       (const double4*)(d + L.xn), (const double*)(d + L.cam), thresh, (double*)(d + L.model), (int32_t*)(d + L.counts),
                       masks ? (uint8_t*)nullptr : (uint8_t*)(d + L.flags), masks);
}
}  // namespace
}  // extern "C++"

int ps_twoview_hypotheses(const double* obs_1, const double* obs_2, int32_t num_pts, const int32_t* sample_idx, int32_t num_hyp,
                          const double* cam5, double thresh, double* E_all, int32_t* counts, uint8_t* degenerate) {
    if (tv_check(obs_1, obs_2, num_pts, cam5, "ps_twoview_hypotheses") ||
        rc_check_samples(sample_idx, num_hyp, 8, num_pts, "ps_twoview_hypotheses")) return -1;
    const TvLayout L((size_t)num_pts, (size_t)num_hyp);
    return rc_hypotheses_call(
        L, [&](char* d) { return tv_begin(L, d, obs_1, obs_2, num_pts, cam5, sample_idx, num_hyp); },
        [&](char* d) { tv_hypotheses(L, d, num_pts, num_hyp, thresh, nullptr); },
        {{L.model, E_all, 9 * F64 * num_hyp}, {L.counts, counts, num_hyp * I32}, {L.flags, degenerate, (size_t)num_hyp}});
}

int ps_twoview_score(const double* E, int32_t num_hyp, const double* obs_1, const double* obs_2, int32_t num_pts, const double* cam5,
                     double thresh, uint8_t* masks, int32_t* counts) {
    if (!E || num_hyp < 0) return fail("ps_twoview_score: bad argument");
    if (tv_check(obs_1, obs_2, num_pts, cam5, "ps_twoview_score")) return -1;
    if (num_hyp == 0) return 0;
    const TvLayout L((size_t)num_pts, (size_t)num_hyp);
    return rc_score_call(
        L, E, 9 * F64 * num_hyp, num_hyp, num_pts, masks, counts,
        [&](char* d) { return tv_begin(L, d, obs_1, obs_2, num_pts, cam5, nullptr, num_hyp); },
        [&](char* d, uint8_t* dmasks) { tv_hypotheses(L, d, num_pts, num_hyp, thresh, dmasks); });
}

int ps_twoview_ransac(const double* obs_1, const double* obs_2, int32_t num_pts, const int32_t* sample_idx, int32_t num_hyp,
                      const double* cam5, double thresh, int32_t refit, double* T_21, double* E_out, uint8_t* mask, int32_t* info,
                      double* parallax_deg) {
    if (tv_check(obs_1, obs_2, num_pts, cam5, "ps_twoview_ransac") ||
        rc_check_samples(sample_idx, num_hyp, 8, num_pts, "ps_twoview_ransac")) return -1;
    const TvLayout L((size_t)num_pts, (size_t)num_hyp);
    DevBuf buf;
    if (need_device() || buf.get(L.total)) return -1;
    char* d = buf.as<char>();
    if (tv_begin(L, d, obs_1, obs_2, num_pts, cam5, sample_idx, num_hyp)) return -1;
    const double4* xn = (const double4*)(d + L.xn);
    const double* cam = (const double*)(d + L.cam);
    tv_hypotheses(L, d, num_pts, num_hyp, thresh, nullptr);
    hipLaunchKernelGGL(k_tv_best, dim3(1), dim3(256), 0, 0, num_hyp, num_pts, (const int32_t*)(d + L.counts), (const double*)(d + L.model),
                       xn, cam, thresh, (int32_t*)(d + L.info), (double*)(d + L.E_best), (uint8_t*)(d + L.mask));
    if (refit)
        for (int stage = 0; stage < 3; ++stage)
            hipLaunchKernelGGL(k_tv_refit_pass, dim3(L.G), dim3(256), 0, 0, stage, num_pts, xn, (const uint8_t*)(d + L.mask),
                               (double*)(d + L.partA), (double*)(d + L.partB), (double*)(d + L.partC));
    hipLaunchKernelGGL(k_tv_finish, dim3(1), dim3(256), 0, 0, num_pts, L.G, refit ? 1 : 0, xn, cam, thresh, (const double*)(d + L.partA),
                       (const double*)(d + L.partB), (const double*)(d + L.partC), (const double*)(d + L.E_best), (uint8_t*)(d + L.mask),
                       (uint8_t*)(d + L.mask_refit), (int32_t*)(d + L.info), (double*)(d + L.result));
    return rc_download(d, L.out, {{L.result, T_21, 16 * F64}, {L.result + 16 * F64, E_out, 9 * F64}, {L.result + 26 * F64, parallax_deg, num_pts * F64},
                                  {L.info, info, 8 * I32}, {L.mask, mask, (size_t)num_pts}});
}
