// ps_abi_pnp.h -- C ABI: absolute-pose (PnP) RANSAC, registration of a monocular frame against the map (kernels: ps_k_pnp.h).
// Part of ps_core.hip (inside its extern "C" block, after ps_abi_twoview.h).  Stateless; host pointers in, host pointers out.
//
// Every call takes ONE device block (inputs | work space | results), one upload of the packed inputs and one download of the
// packed results, which is its only synchronisation.

extern "C++" {
namespace {
struct PnpLayout {                   // byte offsets into the call's device block, every part 64-byte aligned
    size_t in = 0, in_bytes = 0;     // pts_w (3 N) | obs (2 N) | cam (8) as doubles, then the int32 sample table (3 H)
    size_t pts = 0, obs = 0, cam = 0, idx = 0;
    size_t bear = 0, T_best = 0;
    size_t hyp = 0, hyp_bytes = 0;   // T_all (64 H doubles) | counts (4 H int32) | flags (4 H bytes): ps_pnp_hypotheses' download
    size_t T_all = 0, counts = 0, flags = 0;
    size_t out = 0, out_bytes = 0;   // result doubles (16 + iters + 1 + N, padded to even) | info (8 int32) | mask (N bytes)
    size_t result = 0, info = 0, mask = 0;
    size_t total = 0;
    static size_t up(size_t b) { return (b + 63) & ~(size_t)63; }
    PnpLayout(size_t N, size_t H, size_t iters) {
        size_t o = 0;
        in = o;
        pts = o; o += 3 * N * sizeof(double);
        obs = o; o += 2 * N * sizeof(double);
        cam = o; o += 8 * sizeof(double);
        idx = o; o += 3 * H * sizeof(int32_t);
        in_bytes = o - in;
        o = up(o);
        bear = o; o = up(o + 3 * N * sizeof(double));
        T_best = o; o = up(o + 16 * sizeof(double));
        hyp = o;
        T_all = o; o += 64 * H * sizeof(double);
        counts = o; o += 4 * H * sizeof(int32_t);
        flags = o; o += 4 * H;
        hyp_bytes = o - hyp;
        o = up(o);
        out = o;
        const size_t nres = 16 + iters + 1 + N;
        result = o; o += (nres + (nres & 1)) * sizeof(double);
        info = o; o += 8 * sizeof(int32_t);
        mask = o; o += N;
        out_bytes = o - out;
        total = up(o);
    }
};

int pnp_check(const double* pts_w, const double* obs, int32_t num_pts, const double* cam5, const char* who) {
    if (!pts_w || !obs || !cam5) return fail(std::string(who) + ": bad argument");
    if (num_pts < 3) return fail(std::string(who) + ": an absolute pose needs at least 3 points");
    if (!(cam5[2] != 0.0) || !(cam5[3] != 0.0) || !std::isfinite(cam5[0] + cam5[1] + cam5[2] + cam5[3]))
        return fail(std::string(who) + ": the focal lengths must be finite and non-zero");
    return 0;
}

int pnp_check_samples(const int32_t* idx, int32_t num_hyp, int32_t num_pts, const char* who) {
    if (!idx || num_hyp <= 0) return fail(std::string(who) + ": bad argument");
    for (size_t k = 0; k < (size_t)num_hyp * 3; ++k)
        if (idx[k] < 0 || idx[k] >= num_pts) return fail(std::string(who) + ": sample index out of range");
    return 0;
}

// packs pts_w | obs | cam | idx, uploads them and runs k_pnp_normalise
int pnp_upload(const PnpLayout& L, char* d, const double* pts_w, const double* obs, int32_t num_pts, const double* cam5,
               const int32_t* idx, int32_t num_hyp) {
    std::vector<char> stage(L.in_bytes);
    std::memcpy(stage.data() + L.pts, pts_w, 3 * (size_t)num_pts * sizeof(double));
    std::memcpy(stage.data() + L.obs, obs, 2 * (size_t)num_pts * sizeof(double));
    double cam8[8] = {cam5[0], cam5[1], cam5[2], cam5[3], cam5[4], 0.0, 0.0, 0.0};
    std::memcpy(stage.data() + L.cam, cam8, sizeof(cam8));
    if (idx) std::memcpy(stage.data() + L.idx, idx, 3 * (size_t)num_hyp * sizeof(int32_t));
    HIP_OK(hipMemcpy(d + L.in, stage.data(), L.in_bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_pnp_normalise, dim3(cdiv(num_pts, 256)), dim3(256), 0, 0, num_pts, (const double*)(d + L.obs),
                       (const double*)(d + L.cam), (double*)(d + L.bear));
    return 0;
}
}  // namespace
}  // extern "C++"

int ps_pnp_hypotheses(const double* pts_w, const double* obs, int32_t num_pts, const int32_t* sample_idx, int32_t num_hyp,
                      const double* cam5, double thresh, double* T_all, int32_t* counts, uint8_t* empty) {
    if (pnp_check(pts_w, obs, num_pts, cam5, "ps_pnp_hypotheses") ||
        pnp_check_samples(sample_idx, num_hyp, num_pts, "ps_pnp_hypotheses")) return -1;
    if (need_device()) return -1;
    const PnpLayout L((size_t)num_pts, (size_t)num_hyp, 0);
    DevBuf buf;
    if (buf.get(L.total)) return -1;
    char* d = buf.as<char>();
    if (pnp_upload(L, d, pts_w, obs, num_pts, cam5, sample_idx, num_hyp)) return -1;
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3(num_hyp), dim3(256), 0, 0, num_pts, (const int32_t*)(d + L.idx), (const double*)(d + L.pts),
                       (const double*)(d + L.obs), (const double*)(d + L.bear), (const double*)(d + L.cam), thresh, (double*)(d + L.T_all),
                       (int32_t*)(d + L.counts), (uint8_t*)(d + L.flags), (uint8_t*)nullptr);
    std::vector<char> out(L.hyp_bytes);
    HIP_OK(hipMemcpy(out.data(), d + L.hyp, L.hyp_bytes, hipMemcpyDeviceToHost));       // the call's one synchronisation
    if (T_all) std::memcpy(T_all, out.data() + (L.T_all - L.hyp), 64 * (size_t)num_hyp * sizeof(double));
    if (counts) std::memcpy(counts, out.data() + (L.counts - L.hyp), 4 * (size_t)num_hyp * sizeof(int32_t));
    if (empty) std::memcpy(empty, out.data() + (L.flags - L.hyp), 4 * (size_t)num_hyp);
    return 0;
}

int ps_pnp_score(const double* T, int32_t num_T, const double* pts_w, const double* obs, int32_t num_pts, const double* cam5,
                 double thresh, uint8_t* masks, int32_t* counts) {
    if (!T || num_T < 0) return fail("ps_pnp_score: bad argument");
    if (pnp_check(pts_w, obs, num_pts, cam5, "ps_pnp_score")) return -1;
    if (num_T == 0) return 0;
    if (need_device()) return -1;
    const PnpLayout L((size_t)num_pts, (size_t)num_T, 0);     // (T_all holds 64 H doubles: room for the 16 num_T given ones)
    DevBuf buf, dmask;
    if (buf.get(L.total) || dmask.get((size_t)num_T * num_pts)) return -1;
    char* d = buf.as<char>();
    if (pnp_upload(L, d, pts_w, obs, num_pts, cam5, nullptr, num_T)) return -1;
    HIP_OK(hipMemcpy(d + L.T_all, T, 16 * (size_t)num_T * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3(num_T), dim3(256), 0, 0, num_pts, (const int32_t*)nullptr, (const double*)(d + L.pts),
                       (const double*)(d + L.obs), (const double*)(d + L.bear), (const double*)(d + L.cam), thresh, (double*)(d + L.T_all),
                       (int32_t*)(d + L.counts), (uint8_t*)nullptr, dmask.as<uint8_t>());
    if (masks) HIP_OK(hipMemcpy(masks, dmask.p, (size_t)num_T * num_pts, hipMemcpyDeviceToHost));
    if (counts) HIP_OK(hipMemcpy(counts, d + L.counts, (size_t)num_T * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipDeviceSynchronize());
    return 0;
}

int ps_pnp_ransac(const double* pts_w, const double* obs, int32_t num_pts, const int32_t* sample_idx, int32_t num_hyp,
                  const double* cam5, double thresh, int32_t refine_iters, double* T_cw, uint8_t* mask, int32_t* info,
                  double* sq_err, double* cost_history) {
    if (pnp_check(pts_w, obs, num_pts, cam5, "ps_pnp_ransac") ||
        pnp_check_samples(sample_idx, num_hyp, num_pts, "ps_pnp_ransac")) return -1;
    if (refine_iters < 0 || refine_iters > 1000) return fail("ps_pnp_ransac: refine_iters must lie in 0..1000");
    if (need_device()) return -1;
    const PnpLayout L((size_t)num_pts, (size_t)num_hyp, (size_t)refine_iters);
    DevBuf buf;
    if (buf.get(L.total)) return -1;
    char* d = buf.as<char>();
    if (pnp_upload(L, d, pts_w, obs, num_pts, cam5, sample_idx, num_hyp)) return -1;
    const double* pts = (const double*)(d + L.pts);
    const double* ob = (const double*)(d + L.obs);
    const double* cam = (const double*)(d + L.cam);
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3(num_hyp), dim3(256), 0, 0, num_pts, (const int32_t*)(d + L.idx), pts, ob,
                       (const double*)(d + L.bear), cam, thresh, (double*)(d + L.T_all), (int32_t*)(d + L.counts), (uint8_t*)(d + L.flags),
                       (uint8_t*)nullptr);
    hipLaunchKernelGGL(k_pnp_best, dim3(1), dim3(256), 0, 0, 4 * num_hyp, num_pts, (const int32_t*)(d + L.counts),
                       (const double*)(d + L.T_all), pts, ob, cam, thresh, (int32_t*)(d + L.info), (double*)(d + L.T_best),
                       (uint8_t*)(d + L.mask));
    hipLaunchKernelGGL(k_pnp_refine, dim3(1), dim3(256), 0, 0, num_pts, refine_iters, pts, ob, cam, thresh, (const double*)(d + L.T_best),
                       (uint8_t*)(d + L.mask), (int32_t*)(d + L.info), (double*)(d + L.result));
    std::vector<char> out(L.out_bytes);
    HIP_OK(hipMemcpy(out.data(), d + L.out, L.out_bytes, hipMemcpyDeviceToHost));       // the call's one synchronisation
    const double* res = (const double*)(out.data() + (L.result - L.out));
    if (T_cw) std::memcpy(T_cw, res, 16 * sizeof(double));
    if (cost_history) std::memcpy(cost_history, res + 16, ((size_t)refine_iters + 1) * sizeof(double));
    if (sq_err) std::memcpy(sq_err, res + 16 + refine_iters + 1, (size_t)num_pts * sizeof(double));
    if (info) std::memcpy(info, out.data() + (L.info - L.out), 8 * sizeof(int32_t));
    if (mask) std::memcpy(mask, out.data() + (L.mask - L.out), (size_t)num_pts);
    return 0;
}
