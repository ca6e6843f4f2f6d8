// ps_k_feat_db.h -- the keyframe database query (step 10 of the matcher's definition; host restatement:
// featproc.db_query): every stored descriptor of a range of entries against every feature of the frame, best and second-best cost,
// ratio test, and per entry the number of descriptors that pass.
//
//   k_feat_db_search  lane / descriptor, 4 waves / 64 descriptors of ONE entry  : all-pairs SAD from an LDS tile, one count per workgroup
//
// The arrangement is k_feat_map_search_all's (ps_k_feat_global.h): lane l of each of the four waves of a workgroup holds one stored
// descriptor in 8 VGPRs, the frame's descriptors pass through LDS in tiles of PS_FEAT_ALL_TILE, wave w scans quarter w of every tile
// with broadcast reads and keeps a strict-< triple (c1, best, c2), and the four triples merge through LDS by the order-independent key
// rule.  What differs is what becomes of the result: a workgroup's 64 descriptors belong to one entry (the host's block table names it
// and the first descriptor), wave 0 counts its accepted lanes with a ballot and adds the count to the entry's score with one integer
// atomicAdd.  Integer addition does not depend on the order, so two queries give the same bits.  Lanes past the entry's end hold a zero
// descriptor, are not counted, and reach every barrier.  No floating point; no store but that atomic.
//
// PS_FEAT_DB_PER_LANE = 2 (two stored descriptors per lane, 128 per workgroup: every LDS read serves two pairs) was measured 5-8 %
// faster in the kernel at 128 and 1 024 entries of 1 000 descriptors and a tenth slower at 16, where it halves a grid that is small
// already; it is not the default.
#pragma once
#include "ps_k_feat_global.h"

#ifndef PS_FEAT_DB_PER_LANE
#define PS_FEAT_DB_PER_LANE 1                   // stored descriptors per lane: a workgroup serves 64 of them times this
#endif
#define PS_FEAT_DB_BLOCK (64 * PS_FEAT_DB_PER_LANE)

struct FeatDbBlock { int entry, start; };       // a workgroup's entry and the index of its first descriptor in the pool

__global__ __launch_bounds__(256) void k_feat_db_search(const FeatDbBlock* __restrict__ blocks, const int* __restrict__ entry_start,
                                                         const int* __restrict__ entry_len, int first_entry,
                                                         const uint32_t* __restrict__ desc, FeatList B, int max_features, int cost_max,
                                                         int ratio_num, int ratio_den, int* __restrict__ score)
{
    constexpr int P = PS_FEAT_DB_PER_LANE;
    __shared__ uint4 tile[2 * PS_FEAT_ALL_TILE];
    __shared__ unsigned long long s_best[4][64 * P];
    __shared__ unsigned s_second[4][64 * P];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const FeatDbBlock blk = blocks[blockIdx.x];
    const int end = entry_start[blk.entry] + entry_len[blk.entry];
    const int F = min(*B.n, max_features);
    uint4 a0[P], a1[P];
    unsigned bc[P], sc[P];
    int bk[P];
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const int i = blk.start + 64 * r + lane;
        a0[r] = a1[r] = make_uint4(0u, 0u, 0u, 0u);
        if (i < end) {
            a0[r] = *(const uint4*)(desc + 8 * (size_t)i);
            a1[r] = *(const uint4*)(desc + 8 * (size_t)i + 4);
        }
        bc[r] = sc[r] = PS_FEAT_ALL_NONE;
        bk[r] = -1;
    }
    for (int t0 = 0; t0 < F; t0 += PS_FEAT_ALL_TILE) {              // uniform over the workgroup
        const int n = min(PS_FEAT_ALL_TILE, F - t0);
        const uint4* src = (const uint4*)(B.desc + 8 * (size_t)t0);
        for (int q = threadIdx.x; q < 2 * n; q += 256) tile[q] = src[q];
        __syncthreads();
        const int j1 = min((wv + 1) * (PS_FEAT_ALL_TILE / 4), n);
#pragma unroll 4
        for (int j = wv * (PS_FEAT_ALL_TILE / 4); j < j1; ++j) {    // uniform over the wave
            const uint4 b0 = tile[2 * j], b1 = tile[2 * j + 1];
#pragma unroll
            for (int r = 0; r < P; ++r) {
                unsigned c = __builtin_amdgcn_sad_u8(a0[r].x, b0.x, 0u);
                c = __builtin_amdgcn_sad_u8(a0[r].y, b0.y, c);
                c = __builtin_amdgcn_sad_u8(a0[r].z, b0.z, c);
                c = __builtin_amdgcn_sad_u8(a0[r].w, b0.w, c);
                c = __builtin_amdgcn_sad_u8(a1[r].x, b1.x, c);
                c = __builtin_amdgcn_sad_u8(a1[r].y, b1.y, c);
                c = __builtin_amdgcn_sad_u8(a1[r].z, b1.z, c);
                c = __builtin_amdgcn_sad_u8(a1[r].w, b1.w, c);
                sc[r] = min(sc[r], max(c, bc[r]));                  // the larger of the new cost and the best so far
                bk[r] = c < bc[r] ? t0 + j : bk[r];                 // strict: an equal cost later in the list does not win
                bc[r] = min(bc[r], c);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < P; ++r) {
        s_best[wv][64 * r + lane] = ((unsigned long long)bc[r] << 32) | (unsigned)bk[r];
        s_second[wv][64 * r + lane] = sc[r];
    }
    __syncthreads();
    if (wv != 0) return;                                            // the last barrier is behind: wave 0 goes on whole
    int count = 0;
#pragma unroll
    for (int r = 0; r < P; ++r) {
        unsigned long long best = s_best[0][64 * r + lane];
        unsigned sec = s_second[0][64 * r + lane];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            const unsigned long long o = s_best[q][64 * r + lane], lo = o < best ? o : best, hi = o < best ? best : o;
            sec = min(min(sec, s_second[q][64 * r + lane]), (unsigned)(hi >> 32));
            best = lo;
        }
        const unsigned c1 = (unsigned)(best >> 32);
        bool ok = blk.start + 64 * r + lane < end && c1 != PS_FEAT_ALL_NONE && (int)c1 <= cost_max;
        if (ok && sec != PS_FEAT_ALL_NONE && (long long)ratio_den * (int)c1 >= (long long)ratio_num * (int)sec) ok = false;
        count += __popcll(__ballot(ok));
    }
    if (lane == 0 && count) atomicAdd(score + (blk.entry - first_entry), count);
}
