// ps_abi_twoview.h -- C ABI: monocular two-view initialisation, essential-matrix RANSAC (kernels: ps_k_twoview.h).
// Part of ps_core.hip (inside its extern "C" block, after ps_abi_small.h).  Stateless; host pointers in, host pointers out.
//
// Every call takes ONE device block (inputs | work space | results), one upload of the packed inputs and one download of the
// packed results, which is its only synchronisation.

extern "C++" {
namespace {
struct TvLayout {                    // byte offsets into the call's device block, every part 64-byte aligned
    size_t in = 0, in_bytes = 0;     // obs_1 (2 N) | obs_2 (2 N) | cam (8) as doubles, then the int32 sample table (8 H)
    size_t obs1 = 0, obs2 = 0, cam = 0, idx = 0;
    size_t xn = 0, E_all = 0, counts = 0, flags = 0, E_best = 0, partA = 0, partB = 0, partC = 0, mask_refit = 0;
    size_t out = 0, out_bytes = 0;   // result doubles (26 + N) | info (8 int32) | mask (N bytes)
    size_t result = 0, info = 0, mask = 0;
    size_t total = 0;
    int G = 0;
    static size_t up(size_t b) { return (b + 63) & ~(size_t)63; }
    TvLayout(size_t N, size_t H) {
        G = (int)((N + 255) / 256);
        size_t o = 0;
        in = o;
        obs1 = o; o += 2 * N * sizeof(double);
        obs2 = o; o += 2 * N * sizeof(double);
        cam = o; o += 8 * sizeof(double);
        idx = o; o += 8 * H * sizeof(int32_t);
        in_bytes = o - in;
        o = up(o);
        xn = o; o = up(o + 4 * N * sizeof(double));
        E_all = o; o = up(o + 9 * H * sizeof(double));
        E_best = o; o = up(o + 16 * sizeof(double));
        partA = o; o = up(o + 8 * (size_t)G * sizeof(double));
        partB = o; o = up(o + 2 * (size_t)G * sizeof(double));
        partC = o; o = up(o + 45 * (size_t)G * sizeof(double));
        counts = o; o = up(o + H * sizeof(int32_t));
        flags = o; o = up(o + H);
        mask_refit = o; o = up(o + N);
        out = o;
        result = o; o += (26 + N + (N & 1)) * sizeof(double);
        info = o; o += 8 * sizeof(int32_t);
        mask = o; o += N;
        out_bytes = o - out;
        total = up(o);
    }
};

int tv_check(const double* obs_1, const double* obs_2, int32_t num_pts, const double* cam5, const char* who) {
    if (!obs_1 || !obs_2 || !cam5 || num_pts <= 0) return fail(std::string(who) + ": bad argument");
    if (!(cam5[2] != 0.0) || !(cam5[3] != 0.0) || !std::isfinite(cam5[0] + cam5[1] + cam5[2] + cam5[3]))
        return fail(std::string(who) + ": the focal lengths must be finite and non-zero");
    return 0;
}

// packs obs_1 | obs_2 | cam | idx, uploads them and runs k_tv_normalise
int tv_upload(const TvLayout& L, char* d, const double* obs_1, const double* obs_2, int32_t num_pts, const double* cam5,
              const int32_t* idx, int32_t num_hyp) {
    std::vector<char> stage(L.in_bytes);
    std::memcpy(stage.data() + L.obs1, obs_1, 2 * (size_t)num_pts * sizeof(double));
    std::memcpy(stage.data() + L.obs2, obs_2, 2 * (size_t)num_pts * sizeof(double));
    double cam8[8] = {cam5[0], cam5[1], cam5[2], cam5[3], cam5[4], 0.0, 0.0, 0.0};
    std::memcpy(stage.data() + L.cam, cam8, sizeof(cam8));
    if (idx) std::memcpy(stage.data() + L.idx, idx, 8 * (size_t)num_hyp * sizeof(int32_t));
    HIP_OK(hipMemcpy(d + L.in, stage.data(), L.in_bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_tv_normalise, dim3(cdiv(num_pts, 256)), dim3(256), 0, 0, num_pts, (const double*)(d + L.obs1),
                       (const double*)(d + L.obs2), (const double*)(d + L.cam), (double4*)(d + L.xn));
    return 0;
}

int tv_check_samples(const int32_t* idx, int32_t num_hyp, int32_t num_pts, const char* who) {
    if (!idx || num_hyp <= 0) return fail(std::string(who) + ": bad argument");
    for (size_t k = 0; k < (size_t)num_hyp * 8; ++k)
        if (idx[k] < 0 || idx[k] >= num_pts) return fail(std::string(who) + ": sample index out of range");
    return 0;
}
}  // namespace
}  // extern "C++"

int ps_twoview_hypotheses(const double* obs_1, const double* obs_2, int32_t num_pts, const int32_t* sample_idx, int32_t num_hyp,
                          const double* cam5, double thresh, double* E_all, int32_t* counts, uint8_t* degenerate) {
    if (tv_check(obs_1, obs_2, num_pts, cam5, "ps_twoview_hypotheses") ||
        tv_check_samples(sample_idx, num_hyp, num_pts, "ps_twoview_hypotheses")) return -1;
    if (need_device()) return -1;
    const TvLayout L((size_t)num_pts, (size_t)num_hyp);
    DevBuf buf;
    if (buf.get(L.total)) return -1;
    char* d = buf.as<char>();
    if (tv_upload(L, d, obs_1, obs_2, num_pts, cam5, sample_idx, num_hyp)) return -1;
    hipLaunchKernelGGL(k_tv_hypotheses, dim3(num_hyp), dim3(256), 0, 0, num_pts, (const int32_t*)(d + L.idx), (const double4*)(d + L.xn),
                       (const double*)(d + L.cam), thresh, (double*)(d + L.E_all), (int32_t*)(d + L.counts), (uint8_t*)(d + L.flags),
                       (uint8_t*)nullptr);
    if (E_all) HIP_OK(hipMemcpy(E_all, d + L.E_all, 9 * (size_t)num_hyp * sizeof(double), hipMemcpyDeviceToHost));
    if (counts) HIP_OK(hipMemcpy(counts, d + L.counts, (size_t)num_hyp * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (degenerate) HIP_OK(hipMemcpy(degenerate, d + L.flags, (size_t)num_hyp, hipMemcpyDeviceToHost));
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

int ps_twoview_score(const double* E, int32_t num_hyp, const double* obs_1, const double* obs_2, int32_t num_pts, const double* cam5,
                     double thresh, uint8_t* masks, int32_t* counts) {
    if (!E || num_hyp < 0) return fail("ps_twoview_score: bad argument");
    if (tv_check(obs_1, obs_2, num_pts, cam5, "ps_twoview_score")) return -1;
    if (num_hyp == 0) return 0;
    if (need_device()) return -1;
    const TvLayout L((size_t)num_pts, (size_t)num_hyp);
    DevBuf buf, dmask;
    if (buf.get(L.total) || dmask.get((size_t)num_hyp * num_pts)) return -1;
    char* d = buf.as<char>();
    if (tv_upload(L, d, obs_1, obs_2, num_pts, cam5, nullptr, num_hyp)) return -1;
    HIP_OK(hipMemcpy(d + L.E_all, E, 9 * (size_t)num_hyp * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_tv_hypotheses, dim3(num_hyp), dim3(256), 0, 0, num_pts, (const int32_t*)nullptr, (const double4*)(d + L.xn),
                       (const double*)(d + L.cam), thresh, (double*)(d + L.E_all), (int32_t*)(d + L.counts), (uint8_t*)nullptr,
                       dmask.as<uint8_t>());
    if (masks) HIP_OK(hipMemcpy(masks, dmask.p, (size_t)num_hyp * num_pts, hipMemcpyDeviceToHost));
    if (counts) HIP_OK(hipMemcpy(counts, d + L.counts, (size_t)num_hyp * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

int ps_twoview_ransac(const double* obs_1, const double* obs_2, int32_t num_pts, const int32_t* sample_idx, int32_t num_hyp,
                      const double* cam5, double thresh, int32_t refit, double* T_21, double* E_out, uint8_t* mask, int32_t* info,
                      double* parallax_deg) {
    if (tv_check(obs_1, obs_2, num_pts, cam5, "ps_twoview_ransac") ||
        tv_check_samples(sample_idx, num_hyp, num_pts, "ps_twoview_ransac")) return -1;
    if (need_device()) return -1;
    const TvLayout L((size_t)num_pts, (size_t)num_hyp);
    DevBuf buf;
    if (buf.get(L.total)) return -1;
    char* d = buf.as<char>();
    if (tv_upload(L, d, obs_1, obs_2, num_pts, cam5, sample_idx, num_hyp)) return -1;
    const double4* xn = (const double4*)(d + L.xn);
    const double* cam = (const double*)(d + L.cam);
    hipLaunchKernelGGL(k_tv_hypotheses, dim3(num_hyp), dim3(256), 0, 0, num_pts, (const int32_t*)(d + L.idx), xn, cam, thresh,
                       (double*)(d + L.E_all), (int32_t*)(d + L.counts), (uint8_t*)(d + L.flags), (uint8_t*)nullptr);
    hipLaunchKernelGGL(k_tv_best, dim3(1), dim3(256), 0, 0, num_hyp, num_pts, (const int32_t*)(d + L.counts), (const double*)(d + L.E_all),
                       xn, cam, thresh, (int32_t*)(d + L.info), (double*)(d + L.E_best), (uint8_t*)(d + L.mask));
    if (refit)
        for (int stage = 0; stage < 3; ++stage)
            hipLaunchKernelGGL(k_tv_refit_pass, dim3(L.G), dim3(256), 0, 0, stage, num_pts, xn, (const uint8_t*)(d + L.mask),
                               (double*)(d + L.partA), (double*)(d + L.partB), (double*)(d + L.partC));
    hipLaunchKernelGGL(k_tv_finish, dim3(1), dim3(256), 0, 0, num_pts, L.G, refit ? 1 : 0, xn, cam, thresh, (const double*)(d + L.partA),
                       (const double*)(d + L.partB), (const double*)(d + L.partC), (const double*)(d + L.E_best), (uint8_t*)(d + L.mask),
                       (uint8_t*)(d + L.mask_refit), (int32_t*)(d + L.info), (double*)(d + L.result));
    std::vector<char> out(L.out_bytes);
    HIP_OK(hipMemcpy(out.data(), d + L.out, L.out_bytes, hipMemcpyDeviceToHost));       // the call's one synchronisation
    const double* res = (const double*)(out.data() + (L.result - L.out));
    if (T_21) std::memcpy(T_21, res, 16 * sizeof(double));
    if (E_out) std::memcpy(E_out, res + 16, 9 * sizeof(double));
    if (parallax_deg) std::memcpy(parallax_deg, res + 26, (size_t)num_pts * sizeof(double));
    if (info) std::memcpy(info, out.data() + (L.info - L.out), 8 * sizeof(int32_t));
    if (mask) std::memcpy(mask, out.data() + (L.mask - L.out), (size_t)num_pts);
    return 0;
}
