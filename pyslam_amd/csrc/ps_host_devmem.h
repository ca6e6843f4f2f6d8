// ps_host_devmem.h -- device memory of everything that is not a ps_problem: the scoped buffer of the stateless entry points
// (DevBuf) and the owner of a stand-alone handle's blocks (DevMem: ps_photo, ps_dense, ps_feat, ps_sim3pg).  Part of
// ps_core.hip, in front of the ps_host_* and ps_abi_* files.  ps_problem keeps its own allocator (arena, guards, blocks the
// device writes: ps_core.hip); a RANSAC call keeps its one block per call (RcBlock, ps_host_ransac.h).
#pragma once

namespace {
int need_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device visible");
    return 0;
}

struct DevBuf {                      // scoped device allocation for the stateless entry points
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    int get(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8) == hipSuccess ? 0 : fail("hipMalloc failed"); }
    template <class T> int put(const T* src, size_t n) {       // room for n elements, filled from the host
        if (get(n * sizeof(T))) return -1;
        if (n) HIP_OK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
    template <class T> int fetch(T* dst, size_t n) const {     // the first n elements back to the host
        HIP_OK(hipMemcpy(dst, p, n * sizeof(T), hipMemcpyDeviceToHost));
        return 0;
    }
    template <class T> T* as() { return static_cast<T*>(p); }
};

// The blocks of a handle, each with the byte count hipMalloc was asked for: bytes() is their sum, so release() takes off what
// alloc() put on; the destructor frees what is left.  min_bytes: the smallest block (0: one element of the type asked for);
// who: in front of the two error texts.
struct DevMem {
    const size_t min_bytes;
    const char* const who;
    std::vector<std::pair<void*, size_t>> blocks;
    explicit DevMem(size_t min_bytes_, const char* who_ = "") : min_bytes(min_bytes_), who(who_) {}
    DevMem(const DevMem&) = delete;
    ~DevMem() { clear(); }
    int alloc_bytes(void** p, size_t b, size_t elem = 1) {
        b = std::max(b, min_bytes ? min_bytes : elem);
        if (hipMalloc(p, b) != hipSuccess) return fail(std::string(who) + "hipMalloc failed");
        blocks.emplace_back(*p, b);
        return 0;
    }
    template <typename T> int alloc(T** p, size_t n) {
        void* q = nullptr;
        if (alloc_bytes(&q, n * sizeof(T), sizeof(T))) return -1;
        *p = (T*)q;
        return 0;
    }
    template <typename T> int upload(T** p, const typename std::remove_const<T>::type* src, size_t n) {
        if (alloc(p, n)) return -1;
        if (n && hipMemcpy((void*)*p, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return fail(std::string(who) + "hipMemcpy failed");
        return 0;
    }
    void release(const void* p) {                              // (a pointer that is not a block of this owner: nothing happens)
        for (size_t k = 0; k < blocks.size(); ++k)
            if (blocks[k].first == p) {
                hipFree(blocks[k].first);
                blocks.erase(blocks.begin() + k);
                return;
            }
    }
    void clear() {
        for (auto& b : blocks) hipFree(b.first);
        blocks.clear();
    }
    int64_t bytes() const {
        int64_t s = 0;
        for (auto& b : blocks) s += (int64_t)b.second;
        return s;
    }
};
}  // namespace
