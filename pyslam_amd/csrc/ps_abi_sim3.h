// ps_abi_sim3.h -- C ABI: similarity (Sim(3)) alignment RANSAC of two matched 3-D point sets (kernels: ps_k_sim3.h).
// Part of ps_core.hip (inside its extern "C" block, after ps_abi_pnp.h; the host side the front ends share: ps_host_ransac.h).
// Stateless; host pointers in, host pointers out.  cam5 == NULL selects the metric mode (no obs_1, obs_2), a camera the pixel mode.

extern "C++" {
namespace {
struct Sim3Layout {                  // the parts of a call's device block (RcBlock)
    size_t pts1, pts2, obs1, obs2, cam, idx;                        // in: pts_1 | pts_2 (3 N each) | obs_1 | obs_2 (2 N each, pixel mode) | cam (8) doubles | samples (3 H int32)
    size_t S_best;                                                  // work space: the winner's model and scale (17 doubles)
    size_t model, scales, counts, flags;                            // hyp: S_all (16 H) | scales (H) doubles | counts (H int32) | flags (H bytes)
    size_t result, info, mask;                                      // out: result (16 + 1 + N doubles, padded to even) | info (8 int32) | mask (N bytes)
    RcSpan in, hyp, out;                                            // the upload, ps_sim3_hypotheses' download, ps_sim3_ransac's
    size_t total;
    Sim3Layout(size_t N, size_t H, bool pixel) {
        RcBlock B;
        const size_t no = pixel ? 2 * N * F64 : 0;
        pts1 = B.part(3 * N * F64); pts2 = B.pack(3 * N * F64); obs1 = B.pack(no); obs2 = B.pack(no); cam = B.pack(8 * F64); idx = B.pack(3 * H * I32);
        in = B.span(pts1);
        S_best = B.part(18 * F64);
        model = B.part(16 * H * F64); scales = B.pack(H * F64); counts = B.pack(H * I32); flags = B.pack(H);
        hyp = B.span(model);
        const size_t nres = 17 + N;
        result = B.part((nres + (nres & 1)) * F64); info = B.pack(8 * I32); mask = B.pack(N);
        out = B.span(result);
        total = B.part(0);
    }
};

int sim3_check(const double* pts_1, const double* pts_2, const double* obs_1, const double* obs_2, int32_t num_pts, const double* cam5,
               double thresh, const char* who) {
    if (!pts_1 || !pts_2) return rc_fail(who, "bad argument");
    if (num_pts < 3) return rc_fail(who, "a similarity needs at least 3 points");
    if (cam5 && (!obs_1 || !obs_2)) return rc_fail(who, "a camera needs obs_1 and obs_2");
    if (!cam5 && (obs_1 || obs_2)) return rc_fail(who, "obs_1 and obs_2 need a camera");
    if (cam5 && rc_check_camera(cam5, who)) return -1;
    if (!(thresh > 0.0)) return rc_fail(who, "thresh must be positive");
    return 0;
}

// uploads pts_1 | pts_2 | obs_1 | obs_2 | cam | idx (idx may be NULL: scoring)
int sim3_begin(const Sim3Layout& L, char* d, const double* pts_1, const double* pts_2, const double* obs_1, const double* obs_2,
               int32_t num_pts, const double* cam5, const int32_t* idx, int32_t num_hyp) {
    const double none[5] = {0.0, 0.0, 1.0, 1.0, 0.0};
    const RcCam cam(cam5 ? cam5 : none);
    const size_t pb = 3 * F64 * num_pts, ob = cam5 ? 2 * F64 * num_pts : 0;
    return rc_upload(d, L.in, {{L.pts1, pts_1, pb}, {L.pts2, pts_2, pb}, {L.obs1, obs_1, ob}, {L.obs2, obs_2, ob}, {L.cam, cam.v, sizeof(cam.v)},
                               {L.idx, idx, 3 * I32 * num_hyp}});
}

// the inputs of a scoring pass as the kernels take them
struct Sim3In {
    const double *pts1, *pts2, *obs1, *obs2, *cam;
    Sim3In(const Sim3Layout& L, char* d) : pts1((const double*)(d + L.pts1)), pts2((const double*)(d + L.pts2)), obs1((const double*)(d + L.obs1)),
                                           obs2((const double*)(d + L.obs2)), cam((const double*)(d + L.cam)) {}
};

// k_sim3_hypotheses on the uploaded samples (masks == NULL) or, scoring, on the models at L.model
template <bool PIXEL>
void sim3_hypotheses(const Sim3Layout& L, char* d, int32_t num_pts, int32_t num_hyp, double thresh, int32_t fixed_scale, uint8_t* masks) {
    const Sim3In in(L, d);
    hipLaunchKernelGGL(k_sim3_hypotheses<PIXEL>, dim3(num_hyp), dim3(256), 0, 0, num_pts,
                       masks ? (const int32_t*)nullptr : (const int32_t*)(d + L.idx), in.pts1, in.pts2, in.obs1, in.obs2, in.cam, thresh,
                       (int)fixed_scale, (double*)(d + L.model), (double*)(d + L.scales), (int32_t*)(d + L.counts), (uint8_t*)(d + L.flags), masks);
}

// k_sim3_best and k_sim3_refit behind the hypotheses
template <bool PIXEL>
void sim3_select_refit(const Sim3Layout& L, char* d, int32_t num_pts, int32_t num_hyp, double thresh, int32_t fixed_scale, int32_t refit_iters) {
    const Sim3In in(L, d);
    hipLaunchKernelGGL(k_sim3_best, dim3(1), dim3(256), 0, 0, num_hyp, (const int32_t*)(d + L.counts), (const double*)(d + L.model),
                       (const double*)(d + L.scales), (int32_t*)(d + L.info), (double*)(d + L.S_best));
    hipLaunchKernelGGL(k_sim3_refit<PIXEL>, dim3(1), dim3(256), 0, 0, num_pts, (int)refit_iters, (int)fixed_scale, in.pts1, in.pts2, in.obs1, in.obs2,
                       in.cam, thresh, (const double*)(d + L.S_best), (uint8_t*)(d + L.mask), (int32_t*)(d + L.info), (double*)(d + L.result));
}
}  // namespace
}  // extern "C++"

int ps_sim3_hypotheses(const double* pts_1, const double* pts_2, const double* obs_1, const double* obs_2, int32_t num_pts,
                       const int32_t* sample_idx, int32_t num_hyp, const double* cam5, double thresh, int32_t fixed_scale,
                       double* S_all, double* scales, int32_t* counts, uint8_t* flags) {
    if (sim3_check(pts_1, pts_2, obs_1, obs_2, num_pts, cam5, thresh, "ps_sim3_hypotheses") ||
        rc_check_samples(sample_idx, num_hyp, 3, num_pts, "ps_sim3_hypotheses")) return -1;
    if (fixed_scale != 0 && fixed_scale != 1) return fail("ps_sim3_hypotheses: fixed_scale must be 0 or 1");
    const Sim3Layout L((size_t)num_pts, (size_t)num_hyp, cam5 != nullptr);
    return rc_hypotheses_call(
        L, [&](char* d) { return sim3_begin(L, d, pts_1, pts_2, obs_1, obs_2, num_pts, cam5, sample_idx, num_hyp); },
        [&](char* d) {
            if (cam5) sim3_hypotheses<true>(L, d, num_pts, num_hyp, thresh, fixed_scale, nullptr);
            else sim3_hypotheses<false>(L, d, num_pts, num_hyp, thresh, fixed_scale, nullptr);
        },
        {{L.model, S_all, 16 * F64 * num_hyp}, {L.scales, scales, F64 * num_hyp}, {L.counts, counts, I32 * num_hyp}, {L.flags, flags, (size_t)num_hyp}});
}

int ps_sim3_score(const double* S, int32_t num_S, const double* pts_1, const double* pts_2, const double* obs_1, const double* obs_2,
                  int32_t num_pts, const double* cam5, double thresh, uint8_t* masks, int32_t* counts) {
    if (!S || num_S < 0) return fail("ps_sim3_score: bad argument");
    if (sim3_check(pts_1, pts_2, obs_1, obs_2, num_pts, cam5, thresh, "ps_sim3_score")) return -1;
    if (num_S == 0) return 0;
    const Sim3Layout L((size_t)num_pts, (size_t)num_S, cam5 != nullptr);
    return rc_score_call(
        L, S, 16 * F64 * num_S, num_S, num_pts, masks, counts,
        [&](char* d) { return sim3_begin(L, d, pts_1, pts_2, obs_1, obs_2, num_pts, cam5, nullptr, num_S); },
        [&](char* d, uint8_t* dmasks) {
            if (cam5) sim3_hypotheses<true>(L, d, num_pts, num_S, thresh, 0, dmasks);
            else sim3_hypotheses<false>(L, d, num_pts, num_S, thresh, 0, dmasks);
        });
}

int ps_sim3_ransac(const double* pts_1, const double* pts_2, const double* obs_1, const double* obs_2, int32_t num_pts,
                   const int32_t* sample_idx, int32_t num_hyp, const double* cam5, double thresh, int32_t fixed_scale,
                   int32_t refit_iters, double* S_21, double* scale, uint8_t* mask, int32_t* info, double* sq_err) {
    if (sim3_check(pts_1, pts_2, obs_1, obs_2, num_pts, cam5, thresh, "ps_sim3_ransac") ||
        rc_check_samples(sample_idx, num_hyp, 3, num_pts, "ps_sim3_ransac")) return -1;
    if (fixed_scale != 0 && fixed_scale != 1) return fail("ps_sim3_ransac: fixed_scale must be 0 or 1");
    if (refit_iters < 0 || refit_iters > 1000) return fail("ps_sim3_ransac: refit_iters must lie in 0..1000");
    const Sim3Layout L((size_t)num_pts, (size_t)num_hyp, cam5 != nullptr);
    DevBuf buf;
    if (need_device() || buf.get(L.total)) return -1;
    char* d = buf.as<char>();
    if (sim3_begin(L, d, pts_1, pts_2, obs_1, obs_2, num_pts, cam5, sample_idx, num_hyp)) return -1;
    if (cam5) {
        sim3_hypotheses<true>(L, d, num_pts, num_hyp, thresh, fixed_scale, nullptr);
        sim3_select_refit<true>(L, d, num_pts, num_hyp, thresh, fixed_scale, refit_iters);
    } else {
        sim3_hypotheses<false>(L, d, num_pts, num_hyp, thresh, fixed_scale, nullptr);
        sim3_select_refit<false>(L, d, num_pts, num_hyp, thresh, fixed_scale, refit_iters);
    }
    return rc_download(d, L.out, {{L.result, S_21, 16 * F64}, {L.result + 16 * F64, scale, F64}, {L.result + 17 * F64, sq_err, num_pts * F64},
                                  {L.info, info, 8 * I32}, {L.mask, mask, (size_t)num_pts}});
}
