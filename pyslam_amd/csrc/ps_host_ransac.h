// ps_host_ransac.h -- the host side of one RANSAC call, shared by the four front ends' C ABI (ps_abi_small.h: frame-to-frame,
// ps_abi_twoview.h, ps_abi_pnp.h, ps_abi_sim3.h).  Part of ps_core.hip (inside its extern "C" block, before the four).
//
// Every call takes ONE device block (inputs | work space | results), one upload of the packed inputs and one download of the
// packed results, which is its only synchronisation.  (The scoring exports keep their H x N masks in a block of their own and
// copy them straight into the caller's array.)

extern "C++" {
namespace {
constexpr size_t F64 = sizeof(double), I32 = sizeof(int32_t);

// Byte offsets into a call's device block.  part() starts 64-byte aligned; pack() follows its predecessor directly, so a part
// and the packs behind it are one contiguous transfer: span(first).  Within a span: doubles, then int32, then bytes.
struct RcSpan { size_t at = 0, bytes = 0; };
struct RcBlock {
    size_t o = 0;
    size_t pack(size_t bytes) { const size_t at = o; o += bytes; return at; }
    size_t part(size_t bytes) { o = (o + 63) & ~(size_t)63; return pack(bytes); }
    RcSpan span(size_t first) const { return RcSpan{first, o - first}; }
};
struct RcPart { size_t at; const void* host; size_t bytes; };       // a part of a span and the caller's array for it (or NULL)

// stages the parts of a span and uploads it in one copy
int rc_upload(char* d, RcSpan s, std::initializer_list<RcPart> parts) {
    std::vector<char> stage(s.bytes);
    for (const RcPart& p : parts)
        if (p.host) std::memcpy(stage.data() + (p.at - s.at), p.host, p.bytes);
    HIP_OK(hipMemcpy(d + s.at, stage.data(), s.bytes, hipMemcpyHostToDevice));
    return 0;
}

// downloads a span in one copy (the call's one synchronisation) and hands out its parts
int rc_download(const char* d, RcSpan s, std::initializer_list<RcPart> parts) {
    std::vector<char> out(s.bytes);
    HIP_OK(hipMemcpy(out.data(), d + s.at, s.bytes, hipMemcpyDeviceToHost));
    for (const RcPart& p : parts)
        if (p.host) std::memcpy(const_cast<void*>(p.host), out.data() + (p.at - s.at), p.bytes);
    return 0;
}

int rc_fail(const char* who, const char* msg) { return fail(who ? std::string(who) + ": " + msg : std::string(msg)); }

int rc_check_camera(const double* cam5, const char* who) {
    if (!(cam5[2] != 0.0) || !(cam5[3] != 0.0) || !std::isfinite(cam5[0] + cam5[1] + cam5[2] + cam5[3]))
        return rc_fail(who, "the focal lengths must be finite and non-zero");
    return 0;
}

int rc_check_samples(const int32_t* idx, int32_t num_hyp, int32_t set_size, int32_t num_pts, const char* who) {
    if (!idx || num_hyp <= 0 || set_size <= 0) return rc_fail(who, "bad argument");
    for (size_t k = 0; k < (size_t)num_hyp * set_size; ++k)
        if (idx[k] < 0 || idx[k] >= num_pts) return rc_fail(who, "sample index out of range");
    return 0;
}

// cam8, the camera as the kernels read it: cu cv fu fv b, padded to 64 bytes
struct RcCam {
    double v[8];
    explicit RcCam(const double* cam5) : v{cam5[0], cam5[1], cam5[2], cam5[3], cam5[4], 0.0, 0.0, 0.0} {}
};

// The body of ps_twoview_hypotheses / ps_pnp_hypotheses.  L: the call's layout (total; the download span hyp); begin(d):
// uploads the inputs and normalises; launch(d): the hypotheses kernel; parts: the caller's arrays.
template <class Layout, class Begin, class Launch>
int rc_hypotheses_call(const Layout& L, Begin begin, Launch launch, std::initializer_list<RcPart> parts) {
    DevBuf buf;
    if (need_device() || buf.get(L.total)) return -1;
    char* d = buf.as<char>();
    if (begin(d)) return -1;
    launch(d);
    return rc_download(d, L.hyp, parts);
}

// The body of ps_ransac_cost / ps_twoview_score / ps_pnp_score: `num` given models (model_bytes in all, to L.model), their
// counts (L.counts) and their masks [num][num_pts].  launch(d, dmasks): the hypotheses kernel in its scoring form.
template <class Layout, class Begin, class Launch>
int rc_score_call(const Layout& L, const double* model, size_t model_bytes, int32_t num, int32_t num_pts, uint8_t* masks,
                  int32_t* counts, Begin begin, Launch launch) {
    DevBuf buf, dmask;
    if (need_device() || buf.get(L.total) || dmask.get((size_t)num * num_pts)) return -1;
    char* d = buf.as<char>();
    if (begin(d)) return -1;
    HIP_OK(hipMemcpy(d + L.model, model, model_bytes, hipMemcpyHostToDevice));
    launch(d, dmask.as<uint8_t>());
    HIP_OK(hipGetLastError());
    if (masks) HIP_OK(hipMemcpy(masks, dmask.p, (size_t)num * num_pts, hipMemcpyDeviceToHost));
    if (counts) HIP_OK(hipMemcpy(counts, d + L.counts, num * I32, hipMemcpyDeviceToHost));
    HIP_OK(hipDeviceSynchronize());
    return 0;
}
}  // namespace
}  // extern "C++"
