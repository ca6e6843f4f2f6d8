// ps_k_feat.h -- the sparse VO front end on the device: corner features, 32-byte gradient descriptors and circular
// matching (definition: DESIGN.md section 7; host restatement: pyslam_amd/pipelines/featproc.py, which every kernel
// here must reproduce exactly -- everything is integer up to the one division of the sub-pixel step).
//
//   k_feat_sobel        32 x 8 tile / block, 1-pixel halo in LDS  : du, dv (int16) of the uint8 image, borders replicated
//   k_feat_response     32 x 8 tile / block, 2-pixel halo in LDS  : R = 16 (a c - b^2) - (a + c)^2 over the 5 x 5 window
//   k_feat_nms          32 x 8 tile / block, nms_n halo in LDS    : feature flag per pixel
//   k_feat_count        256 flags / block                         : block counts (ballot / popcount)
//   (k_dense_scan)                                                : exclusive scan of the block counts
//   k_feat_compact_pix  256 pixels / block                        : the flagged pixels in raster order -> raw list
//   k_feat_rank         thread / raw feature                      : over capacity: keep the max_features strongest
//   k_feat_compact_feat 256 raw features / block                  : kept features in raster order + their descriptors
//   k_feat_rowstart     thread / image row                        : index of the first feature of every row
//   k_feat_match        wave / feature of A                       : best candidate in B (window, SAD of 32 bytes)
//   k_feat_chain        thread / start feature                    : follow the legs, flag the chains that close
//   k_feat_compact_match 256 start features / block               : the closed chains in order -> feature indices
//   k_feat_subpix       thread / match                            : positions with the sub-pixel refinement (fp64)
//   k_feat_map_search   wave / map point                          : projection, best feature in the window, claim (step 8)
//   k_feat_map_resolve  thread / map point                        : one point per feature, positions of the owners
//
// Every compaction is the stable ballot / popcount one (raster order is part of the definition); plain vector stores only, and in
// step 8 two integer vector atomics whose results do not depend on their order (a minimum and a count).
#pragma once
#include "ps_k_dense.h"

#define PS_FEAT_BORDER 5
#define PS_FEAT_TX 32
#define PS_FEAT_TY 8
#define PS_FEAT_R_NONE LLONG_MIN

// (du, dv) offsets of the 16 descriptor samples inside the 11 x 11 patch (featproc.OFFSETS)
__constant__ signed char c_feat_off[16][2] = {{-1, -1}, {1, -1}, {-1, 1}, {1, 1}, {-3, -1}, {3, -1}, {-3, 1}, {3, 1},
                                              {-1, -3}, {1, -3}, {-1, 3}, {1, 3}, {-5, 0}, {5, 0}, {0, -5}, {0, 5}};

PS_DEV int feat_clamp(int p, int n) { return p < 0 ? 0 : (p >= n ? n - 1 : p); }
PS_DEV int feat_byte(int g) { const int b = (g >> 2) + 128; return b < 0 ? 0 : (b > 255 ? 255 : b); }

__global__ __launch_bounds__(256) void k_feat_sobel(const uint8_t* __restrict__ img, int h, int w, short* __restrict__ du,
                                                     short* __restrict__ dv)
{
    __shared__ uint8_t t[PS_FEAT_TY + 2][PS_FEAT_TX + 4];
    const int x0 = blockIdx.x * PS_FEAT_TX, y0 = blockIdx.y * PS_FEAT_TY;
    for (int k = threadIdx.x; k < (PS_FEAT_TY + 2) * (PS_FEAT_TX + 2); k += 256) {
        const int ty = k / (PS_FEAT_TX + 2), tx = k % (PS_FEAT_TX + 2);
        t[ty][tx] = img[(size_t)feat_clamp(y0 + ty - 1, h) * w + feat_clamp(x0 + tx - 1, w)];
    }
    __syncthreads();
    const int tx = threadIdx.x % PS_FEAT_TX, ty = threadIdx.x / PS_FEAT_TX, x = x0 + tx, y = y0 + ty;
    if (x >= w || y >= h) return;
    const int a = t[ty][tx], b = t[ty][tx + 1], c = t[ty][tx + 2], d = t[ty + 1][tx], f = t[ty + 1][tx + 2],
              g = t[ty + 2][tx], hh = t[ty + 2][tx + 1], i = t[ty + 2][tx + 2];
    du[(size_t)y * w + x] = (short)((c - a) + 2 * (f - d) + (i - g));
    dv[(size_t)y * w + x] = (short)((g + 2 * hh + i) - (a + 2 * b + c));
}

__global__ __launch_bounds__(256) void k_feat_response(const short* __restrict__ du, const short* __restrict__ dv, int h, int w,
                                                        long long* __restrict__ R)
{
    __shared__ short su[PS_FEAT_TY + 4][PS_FEAT_TX + 4], sv[PS_FEAT_TY + 4][PS_FEAT_TX + 4];
    const int x0 = blockIdx.x * PS_FEAT_TX, y0 = blockIdx.y * PS_FEAT_TY;
    for (int k = threadIdx.x; k < (PS_FEAT_TY + 4) * (PS_FEAT_TX + 4); k += 256) {
        const int ty = k / (PS_FEAT_TX + 4), tx = k % (PS_FEAT_TX + 4), x = x0 + tx - 2, y = y0 + ty - 2;
        const bool in = x >= 0 && x < w && y >= 0 && y < h;          // outside: never part of a window that counts
        su[ty][tx] = in ? du[(size_t)y * w + x] : (short)0;
        sv[ty][tx] = in ? dv[(size_t)y * w + x] : (short)0;
    }
    __syncthreads();
    const int tx = threadIdx.x % PS_FEAT_TX, ty = threadIdx.x / PS_FEAT_TX, x = x0 + tx, y = y0 + ty;
    if (x >= w || y >= h) return;
    long long r = PS_FEAT_R_NONE;
    if (x >= 2 && x < w - 2 && y >= 2 && y < h - 2) {
        int a = 0, b = 0, c = 0;                                     // 25 * 1020^2 < 2^31
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int gu = su[ty + j][tx + i], gv = sv[ty + j][tx + i];
                a += gu * gu; b += gu * gv; c += gv * gv;
            }
        const long long A = a, B = b, C = c;
        r = 16 * (A * C - B * B) - (A + C) * (A + C);
    }
    R[(size_t)y * w + x] = r;
}

__global__ __launch_bounds__(256) void k_feat_nms(const long long* __restrict__ R, int h, int w, int nms_n, long long threshold,
                                                   uint8_t* __restrict__ flags)
{
    __shared__ long long s[PS_FEAT_TY + 6][PS_FEAT_TX + 6];
    const int x0 = blockIdx.x * PS_FEAT_TX, y0 = blockIdx.y * PS_FEAT_TY;
    for (int k = threadIdx.x; k < (PS_FEAT_TY + 6) * (PS_FEAT_TX + 6); k += 256) {
        const int ty = k / (PS_FEAT_TX + 6), tx = k % (PS_FEAT_TX + 6), x = x0 + tx - 3, y = y0 + ty - 3;
        s[ty][tx] = (x >= 0 && x < w && y >= 0 && y < h) ? R[(size_t)y * w + x] : PS_FEAT_R_NONE;
    }
    __syncthreads();
    const int tx = threadIdx.x % PS_FEAT_TX, ty = threadIdx.x / PS_FEAT_TX, x = x0 + tx, y = y0 + ty;
    if (x >= w || y >= h) return;
    const long long c = s[ty + 3][tx + 3];
    bool keep = x >= PS_FEAT_BORDER && x < w - PS_FEAT_BORDER && y >= PS_FEAT_BORDER && y < h - PS_FEAT_BORDER && c > threshold;
    if (keep)
        for (int dy = -nms_n; dy <= nms_n; ++dy)
            for (int dx = -nms_n; dx <= nms_n; ++dx) {
                if (dx == 0 && dy == 0) continue;
                const long long q = s[ty + 3 + dy][tx + 3 + dx];
                const bool earlier = dy < 0 || (dy == 0 && dx < 0);      // an equal value earlier in raster order wins
                keep = keep && (earlier ? q < c : q <= c);
            }
    flags[(size_t)y * w + x] = keep ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_feat_count(int n, const uint8_t* __restrict__ flags, int* __restrict__ block_counts) {
    __shared__ int wc[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long m = __ballot(i < n && flags[i]);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// position of a kept element in the compacted list (-1: not kept); every thread of the block calls it
PS_DEV int feat_slot(bool keep, const int* __restrict__ block_offsets, int* wc) {
    const unsigned long long m = __ballot(keep);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wc[wv] = __popcll(m);
    __syncthreads();
    if (!keep) return -1;
    int k = block_offsets[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int q = 0; q < wv; ++q) k += wc[q];
    return k;
}

__global__ __launch_bounds__(256) void k_feat_compact_pix(int n, int w, const uint8_t* __restrict__ flags,
                                                           const int* __restrict__ block_offsets, const long long* __restrict__ R,
                                                           int cap, int2* __restrict__ raw_uv, long long* __restrict__ raw_R)
{
    __shared__ int wc[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int k = feat_slot(i < n && flags[i], block_offsets, wc);
    if (k < 0 || k >= cap) return;
    raw_uv[k] = make_int2(i % w, i / w);
    raw_R[k] = R[i];
}

// over capacity: a raw feature is kept when fewer than max_features others are stronger (ties: the earlier one is stronger)
__global__ __launch_bounds__(256) void k_feat_rank(const int* __restrict__ n_raw, int cap, const long long* __restrict__ raw_R,
                                                    int max_features, uint8_t* __restrict__ keep)
{
    __shared__ long long sR[256];
    const int i = blockIdx.x * 256 + threadIdx.x, n = min(*n_raw, cap);
    if (n <= max_features) { if (i < cap) keep[i] = i < n; return; }
    const long long mine = i < n ? raw_R[i] : 0;
    int rank = 0;
    for (int base = 0; base < n; base += 256) {
        sR[threadIdx.x] = base + threadIdx.x < n ? raw_R[base + threadIdx.x] : PS_FEAT_R_NONE;
        __syncthreads();
        const int m = min(256, n - base);
        for (int j = 0; j < m; ++j) {
            const long long r = sR[j];
            rank += (r > mine || (r == mine && base + j < i)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (i < cap) keep[i] = i < n && rank < max_features;
}

__global__ __launch_bounds__(256) void k_feat_compact_feat(int cap, const uint8_t* __restrict__ keep, const int* __restrict__ block_offsets,
                                                            const int2* __restrict__ raw_uv, const long long* __restrict__ raw_R,
                                                            const short* __restrict__ du, const short* __restrict__ dv, int h, int w,
                                                            int max_features, int2* __restrict__ uv, long long* __restrict__ R,
                                                            uint32_t* __restrict__ desc)
{
    __shared__ int wc[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int k = feat_slot(i < cap && keep[i], block_offsets, wc);
    if (k < 0 || k >= max_features) return;
    const int2 p = raw_uv[i];
    uv[k] = p;
    R[k] = raw_R[i];
    uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const size_t at = (size_t)feat_clamp(p.y + c_feat_off[q][1], h) * w + feat_clamp(p.x + c_feat_off[q][0], w);
        d[q >> 2] |= (uint32_t)feat_byte(du[at]) << (8 * (q & 3));
        d[4 + (q >> 2)] |= (uint32_t)feat_byte(dv[at]) << (8 * (q & 3));
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) desc[8 * (size_t)k + q] = d[q];
}

// row_start[v] = number of features above row v (v = 0 .. h): the list is in raster order
__global__ __launch_bounds__(256) void k_feat_rowstart(int h, const int* __restrict__ n_feat, int max_features,
                                                        const int2* __restrict__ uv, int* __restrict__ row_start)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v > h) return;
    int lo = 0, hi = min(*n_feat, max_features);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (uv[mid].y < v) lo = mid + 1; else hi = mid;
    }
    row_start[v] = lo;
}

struct FeatList {               // the features of one image
    const int* n;
    const int2* uv;
    const uint32_t* desc;
    const int* row_start;
    const short *du, *dv;
};

// the best candidate of a descriptor among features k0 .. k1 - 1 of B (a contiguous range of its raster-ordered list: whole
// rows) whose u lies in u_lo .. u_hi: lanes stride over the range, test the u window, and the wave takes the minimum of
// (cost << 32 | index) -- lowest cost, ties to the lower index; ~0 without a candidate.  Every lane of the wave calls it.
PS_DEV unsigned long long feat_best_candidate(const uint32_t* da, const FeatList& B, int k0, int k1, int u_lo, int u_hi, int lane) {
    unsigned long long best = ~0ull;
    for (int k = k0 + lane; k < k1; k += 64) {
        const int u = B.uv[k].x;
        if (u < u_lo || u > u_hi) continue;
        const uint4 b0 = *(const uint4*)(B.desc + 8 * (size_t)k), b1 = *(const uint4*)(B.desc + 8 * (size_t)k + 4);
        unsigned c = __builtin_amdgcn_sad_u8(da[0], b0.x, 0u);
        c = __builtin_amdgcn_sad_u8(da[1], b0.y, c);
        c = __builtin_amdgcn_sad_u8(da[2], b0.z, c);
        c = __builtin_amdgcn_sad_u8(da[3], b0.w, c);
        c = __builtin_amdgcn_sad_u8(da[4], b1.x, c);
        c = __builtin_amdgcn_sad_u8(da[5], b1.y, c);
        c = __builtin_amdgcn_sad_u8(da[6], b1.z, c);
        c = __builtin_amdgcn_sad_u8(da[7], b1.w, c);
        const unsigned long long key = ((unsigned long long)c << 32) | (unsigned)k;
        best = key < best ? key : best;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o < best ? o : best;
    }
    return best;
}

// one wave per feature of A: the candidates of B are the rows v + dv_lo .. v + dv_hi of its list
__global__ __launch_bounds__(256) void k_feat_match(FeatList A, FeatList B, int h, int max_features, int du_lo, int du_hi, int dv_lo,
                                                     int dv_hi, int cost_max, int* __restrict__ out)
{
    const int a = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (a >= min(*A.n, max_features)) return;
    const int2 pa = A.uv[a];
    uint32_t da[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) da[q] = A.desc[8 * (size_t)a + q];
    const int k0 = B.row_start[min(max(pa.y + dv_lo, 0), h)], k1 = B.row_start[min(max(pa.y + dv_hi + 1, 0), h)];
    const unsigned long long best = feat_best_candidate(da, B, k0, k1, pa.x + du_lo, pa.x + du_hi, lane);
    if (lane == 0) out[a] = (best != ~0ull && (int)(best >> 32) <= cost_max) ? (int)(unsigned)best : -1;
}

struct FeatChain {              // a matching mode: the images a chain visits and where each lands in a match row
    int legs;                   // 2 (flow, stereo) or 4 (quad); the last leg closes the circle
    int col[4];                 // column group (1p, 2p, 1c, 2c) of node k
    int temporal[4];            // leg into node k refines u and v (1) or u only (0); [0] unused
};

__global__ __launch_bounds__(256) void k_feat_chain(const int* __restrict__ n_start, int max_features, int legs, const int* __restrict__ l0,
                                                     const int* __restrict__ l1, const int* __restrict__ l2, const int* __restrict__ l3,
                                                     uint8_t* __restrict__ flags, int* __restrict__ visited)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= max_features) return;
    bool ok = i < min(*n_start, max_features);
    const int* leg[4] = {l0, l1, l2, l3};
    int cur = i;
    for (int k = 0; k < legs && ok; ++k) {
        visited[4 * (size_t)i + k] = cur;
        cur = leg[k][cur];
        ok = cur >= 0;
    }
    flags[i] = ok && cur == i;
}

__global__ __launch_bounds__(256) void k_feat_compact_match(int max_features, const uint8_t* __restrict__ flags,
                                                             const int* __restrict__ block_offsets, const int* __restrict__ visited,
                                                             FeatChain ch, int* __restrict__ idx4)
{
    __shared__ int wc[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int k = feat_slot(i < max_features && flags[i], block_offsets, wc);
    if (k < 0) return;
    int row[4] = {-1, -1, -1, -1};
    for (int q = 0; q < ch.legs; ++q) row[ch.col[q]] = visited[4 * (size_t)i + q];
    *(int4*)(idx4 + 4 * (size_t)k) = make_int4(row[0], row[1], row[2], row[3]);
}

// SAD of a source descriptor against the descriptor of pixel (x, y) of the target's gradient images, taken on the fly
PS_DEV int feat_cost_at(const FeatList& T, int h, int w, int x, int y, const uint32_t* d) {
    int c = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const size_t at = (size_t)feat_clamp(y + c_feat_off[q][1], h) * w + feat_clamp(x + c_feat_off[q][0], w);
        c += abs(feat_byte(T.du[at]) - (int)((d[q >> 2] >> (8 * (q & 3))) & 255u));
        c += abs(feat_byte(T.dv[at]) - (int)((d[4 + (q >> 2)] >> (8 * (q & 3))) & 255u));
    }
    return c;
}

// sub-pixel offset from the costs at -1, 0, +1: the equiangular (two-line) fit -- a SAD cost is a V around its minimum
PS_DEV double feat_subpixel(int cm, int c0, int cp) {
#pragma clang fp contract(off)
    const int den = 2 * (max(cm, cp) - c0);
    if (den <= 0 || c0 == 0) return 0.0;            // an exact match has no sub-pixel offset
    const double d = (double)(cm - cp) / (double)den;
    return fabs(d) < 1.0 ? d : 0.0;
}

// sub-pixel offsets (step 7) of pixel p of image T against a source descriptor: in u, and in v for a temporal leg
PS_DEV void feat_refine(const FeatList& T, int h, int w, int2 p, const uint32_t* d, bool temporal, double& ou, double& ov) {
    const int c0 = feat_cost_at(T, h, w, p.x, p.y, d);
    ou = feat_subpixel(feat_cost_at(T, h, w, p.x - 1, p.y, d), c0, feat_cost_at(T, h, w, p.x + 1, p.y, d));
    ov = temporal ? feat_subpixel(feat_cost_at(T, h, w, p.x, p.y - 1, d), c0, feat_cost_at(T, h, w, p.x, p.y + 1, d)) : 0.0;
}

__global__ __launch_bounds__(256) void k_feat_subpix(const int* __restrict__ n_match, int max_features, const int* __restrict__ idx4,
                                                      FeatChain ch, FeatList n0, FeatList n1, FeatList n2, FeatList n3, int h, int w,
                                                      int refinement, double* __restrict__ m8)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(*n_match, max_features)) return;
    const FeatList node[4] = {n0, n1, n2, n3};
    double row[8] = {-1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0};
    double offu = 0.0, offv = 0.0;
    int prev = -1;
    for (int k = 0; k < ch.legs; ++k) {
        const int f = idx4[4 * (size_t)i + ch.col[k]];
        const int2 p = node[k].uv[f];
        if (k > 0 && refinement) {
            uint32_t d[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) d[q] = node[k - 1].desc[8 * (size_t)prev + q];
            double ou, ov;
            feat_refine(node[k], h, w, p, d, ch.temporal[k] != 0, ou, ov);
            offu = offu + ou;
            if (ch.temporal[k]) offv = offv + ov;
        }
        row[2 * ch.col[k]] = (double)p.x + offu;
        row[2 * ch.col[k] + 1] = (double)p.y + offv;
        prev = f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) m8[8 * (size_t)i + q] = row[q];
}

// ---- matching by projection (step 8): the map's points against the features of one image ----
struct FeatMapView {            // pose and calibration of a projection, by value
    double T[12];               // rows 0..2 of T_cw
    double cu, cv, fu, fv;
};

struct FeatMapOut {             // one entry per map point
    int *feature, *status, *cost;
    double* uv;
};

// one wave per map point: project, search the window around the rounded projection, claim the best feature with an integer
// atomicMin of (cost << 32 | point) -- order-independent, so the owner of every feature is the same in every run
__global__ __launch_bounds__(256) void k_feat_map_search(int num_points, const double* __restrict__ pts, const uint32_t* __restrict__ desc,
                                                          FeatMapView V, FeatList B, int h, int w, int max_features, int radius,
                                                          int cost_max, FeatMapOut out, unsigned long long* __restrict__ claim,
                                                          int* __restrict__ n_matched)
{
#pragma clang fp contract(off)
    const int i = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_matched = 0;       // counted by k_feat_map_resolve, the next launch
    if (i >= num_points) return;
    const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    const double xc = ((V.T[0] * x + V.T[1] * y) + V.T[2] * z) + V.T[3];
    const double yc = ((V.T[4] * x + V.T[5] * y) + V.T[6] * z) + V.T[7];
    const double zc = ((V.T[8] * x + V.T[9] * y) + V.T[10] * z) + V.T[11];
    const double u = (V.fu * xc) / zc + V.cu, v = (V.fv * yc) / zc + V.cv;
    const double cen_u = floor(u + 0.5), cen_v = floor(v + 0.5);
    const bool visible = zc > 0.0 && isfinite(xc) && isfinite(yc) && isfinite(zc) && isfinite(u) && isfinite(v) && cen_u >= 0.0 &&
                         cen_u < (double)w && cen_v >= 0.0 && cen_v < (double)h;
    int status = 1, feature = -1, cost = -1;
    if (visible) {                                                  // uniform over the wave
        const int ui = (int)cen_u, vi = (int)cen_v;
        uint32_t da[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) da[q] = desc[8 * (size_t)i + q];
        const int k0 = B.row_start[min(max(vi - radius, 0), h)], k1 = B.row_start[min(max(vi + radius + 1, 0), h)];
        const unsigned long long best = feat_best_candidate(da, B, k0, k1, ui - radius, ui + radius, lane);
        status = 2;
        if (best != ~0ull && (int)(best >> 32) <= cost_max) {
            status = 0; feature = (int)(unsigned)best; cost = (int)(best >> 32);
        }
    }
    if (lane != 0) return;
    if (status == 0 && feature < max_features) atomicMin(claim + feature, ((unsigned long long)(unsigned)cost << 32) | (unsigned)i);
    out.feature[i] = feature; out.status[i] = status; out.cost[i] = cost;
}

// thread per map point: a point that does not own its feature loses it (status 3); the owners get their position
__global__ __launch_bounds__(256) void k_feat_map_resolve(int num_points, const uint32_t* __restrict__ desc, FeatList B, int h, int w,
                                                           int max_features, int refinement, FeatMapOut out,
                                                           const unsigned long long* __restrict__ claim, int* __restrict__ n_matched)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool matched = false;
    if (i < num_points) {
        double pu = -1.0, pv = -1.0;
        const int f = out.feature[i];
        if (out.status[i] == 0 && f >= 0 && f < max_features) {
            if ((int)(unsigned)claim[f] != i) {
                out.status[i] = 3; out.feature[i] = -1;
            } else {
                matched = true;
                const int2 p = B.uv[f];
                double ou = 0.0, ov = 0.0;
                if (refinement) {
                    uint32_t d[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) d[q] = desc[8 * (size_t)i + q];
                    feat_refine(B, h, w, p, d, true, ou, ov);
                }
                pu = (double)p.x + ou; pv = (double)p.y + ov;
            }
        }
        out.uv[2 * (size_t)i] = pu; out.uv[2 * (size_t)i + 1] = pv;
    }
    const unsigned long long m = __ballot(matched);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_matched, __popcll(m));
}
