// ps_k_feat_global.h -- matching without a prior (step 9 of the matcher's definition; host restatement:
// featproc.match_map_global): every map point against every feature of the frame, best and second-best cost, ratio test.
//
//   k_feat_map_search_all  lane / map point, 4 waves / 64 points  : all-pairs SAD from an LDS tile, status, claim (step 9)
//   (k_feat_map_resolve)                                          : step 8's, unchanged: it touches status-0 entries only
//
// A workgroup of 256 threads serves 64 map points: lane l of each of its four waves holds the descriptor of point 64 b + l in 8
// VGPRs.  The frame's descriptors pass through LDS in tiles of PS_FEAT_ALL_TILE (512: 16 KiB, eight workgroups per compute unit);
// wave w compares its points with quarter w of every tile, all 64 lanes reading the same LDS address (a broadcast: no bank
// conflict), so a pair costs eight v_sad_u8 and five integer operations and no global load.  Within a wave the feature index only
// grows, so "lowest cost, ties to the lower index" is a strict comparison of the costs; the four partial results merge as the keys
// cost << 32 | feature with an order-independent rule: best = min(key_a, key_b), second = min(cost of max(key_a, key_b),
// second_a, second_b).  No floating point; plain vector stores and step 8's integer atomicMin for the claim.
#pragma once
#include "ps_k_feat.h"

#define PS_FEAT_ALL_TILE 512
#define PS_FEAT_ALL_NONE 0xffffffffu        // cost of a best or second-best candidate that does not exist

__global__ __launch_bounds__(256) void k_feat_map_search_all(int num_points, const uint32_t* __restrict__ desc, FeatList B,
                                                              int max_features, int cost_max, int ratio_num, int ratio_den,
                                                              FeatMapOut out, int* __restrict__ second,
                                                              unsigned long long* __restrict__ claim, int* __restrict__ n_matched)
{
    __shared__ uint4 tile[2 * PS_FEAT_ALL_TILE];
    __shared__ unsigned long long s_best[4][64];
    __shared__ unsigned s_second[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_matched = 0;       // counted by k_feat_map_resolve, the next launch
    const int F = min(*B.n, max_features);
    uint4 a0 = make_uint4(0u, 0u, 0u, 0u), a1 = a0;
    if (i < num_points) {
        a0 = *(const uint4*)(desc + 8 * (size_t)i);
        a1 = *(const uint4*)(desc + 8 * (size_t)i + 4);
    }
    unsigned bc = PS_FEAT_ALL_NONE, sc = PS_FEAT_ALL_NONE;
    int bk = -1;
    for (int t0 = 0; t0 < F; t0 += PS_FEAT_ALL_TILE) {              // uniform over the workgroup
        const int n = min(PS_FEAT_ALL_TILE, F - t0);
        const uint4* src = (const uint4*)(B.desc + 8 * (size_t)t0);
        for (int q = threadIdx.x; q < 2 * n; q += 256) tile[q] = src[q];
        __syncthreads();
        const int j1 = min((wv + 1) * (PS_FEAT_ALL_TILE / 4), n);
#pragma unroll 4
        for (int j = wv * (PS_FEAT_ALL_TILE / 4); j < j1; ++j) {    // uniform over the wave
            const uint4 b0 = tile[2 * j], b1 = tile[2 * j + 1];
            unsigned c = __builtin_amdgcn_sad_u8(a0.x, b0.x, 0u);
            c = __builtin_amdgcn_sad_u8(a0.y, b0.y, c);
            c = __builtin_amdgcn_sad_u8(a0.z, b0.z, c);
            c = __builtin_amdgcn_sad_u8(a0.w, b0.w, c);
            c = __builtin_amdgcn_sad_u8(a1.x, b1.x, c);
            c = __builtin_amdgcn_sad_u8(a1.y, b1.y, c);
            c = __builtin_amdgcn_sad_u8(a1.z, b1.z, c);
            c = __builtin_amdgcn_sad_u8(a1.w, b1.w, c);
            sc = min(sc, max(c, bc));                               // the larger of the new cost and the best so far
            bk = c < bc ? t0 + j : bk;                              // strict: an equal cost later in the list does not win
            bc = min(bc, c);
        }
        __syncthreads();
    }
    s_best[wv][lane] = ((unsigned long long)bc << 32) | (unsigned)bk;
    s_second[wv][lane] = sc;
    __syncthreads();
    if (wv != 0 || i >= num_points) return;
    unsigned long long best = s_best[0][lane];
    unsigned sec = s_second[0][lane];
#pragma unroll
    for (int q = 1; q < 4; ++q) {
        const unsigned long long o = s_best[q][lane], lo = o < best ? o : best, hi = o < best ? best : o;
        sec = min(min(sec, s_second[q][lane]), (unsigned)(hi >> 32));
        best = lo;
    }
    const unsigned c1 = (unsigned)(best >> 32);
    int status = 2, feature = -1, cost = -1, c2 = -1;
    if (c1 != PS_FEAT_ALL_NONE && (int)c1 <= cost_max) {
        cost = (int)c1;
        c2 = sec != PS_FEAT_ALL_NONE ? (int)sec : -1;
        if (c2 >= 0 && (long long)ratio_den * cost >= (long long)ratio_num * c2) status = 4;
        else { status = 0; feature = (int)(unsigned)best; }
    }
    if (status == 0 && feature < max_features) atomicMin(claim + feature, ((unsigned long long)(unsigned)cost << 32) | (unsigned)i);
    out.feature[i] = feature; out.status[i] = status; out.cost[i] = cost;
    second[i] = c2;
}
