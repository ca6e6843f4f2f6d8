// ps_structure.h -- the parts of ps_problem_create that decide a structure from numbers alone: the stage timer, the landmark
// tile count and the tiled / untiled policy of the Schur pair list (ONE driver over whichever builder makes the list), and the
// block pattern of the reduced system.  No HIP, nothing of the handle: tests/test_structure_host.py compiles it with a plain
// C++ compiler (tests/structure_shim.cpp).  What can be refused is refused through a returned message; the caller fail()s.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

// "<who>: <stage>   <ms>" on stderr after every stage when PS_CREATE_TIMING is set (tools/create_time.py reads the lines)
struct StageLap {
    const char* who;
    bool on;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    StageLap(const char* who_, bool on_) : who(who_), on(on_) {}
    void operator()(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "%s: %-28s %8.1f ms\n", who, what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }
};

// ---- Schur pair list: landmark tiles or not ---------------------------------------------------------------------------------
// Landmark tiles: when Z (144 B per row) is much larger than the eight 4 MB L2s, the pair list is
// cut into tiles of consecutive landmarks (consecutive Z rows) and ONE XCD works through a whole
// tile: a Z row is then only ever requested by one L2 instead of by up to eight.  A block that
// receives pairs from several tiles gets one partial per (tile, block) task, summed in tile order
// by k_schur_combine (fixed order => deterministic).  Measured at C3 (72 MB of Z): 8 tiles of 9 MB
// beat both no tiling (71 -> 65 us) and L2-sized 2-4 MB tiles (71-82 us: five times more tasks,
// and the per-task prologue/epilogue costs more than the extra L2 hits save).
inline int ps_pair_tiles(double zbytes, double tile_kb = 9216.0, double min_mb = 16.0) {
    if (tile_kb > 0 && zbytes > min_mb * 1048576.0) return 8 * (int)std::ceil(zbytes / (8.0 * tile_kb * 1024.0));
    return 1;
}

struct PairListPolicy {
    double zbytes = 0.0;            // all of Z
    bool tiles_forced = false;      // PS_SCHUR_TILE_KB set: the tile count stands, whatever the list looks like
    bool keep_tiles = false;        // PS_SCHUR_KEEP_TILES: blocks that fill the chip are no reason to drop the tiles
    bool by_landmark = false;       // PS_PAIRS_BY_LANDMARK: no cheap untiled build to try first
};
struct PairListCounts { size_t pairs = 0, tasks = 0, blocks = 0; };     // task = run of equal (tile, block); blocks: distinct

constexpr size_t PS_PAIRS_CHIP_BLOCKS = 2 * 256 * 12;        // 2 x 256 CUs x 12 waves of the pipelined pair kernel
constexpr size_t PS_PAIRS_MIN_PER_TASK = 64;
constexpr double PS_PAIRS_CACHE_BYTES = 128.0 * 1048576.0;   // a Z of this size stays in the 256 MiB Infinity Cache

// Builder: int build(int ntiles) makes the list (0, or -1 with the error set); PairListCounts counts() describes the last build.
// -> the tile count of the list the builder is left with.
//
// Tiles multiply the tasks (one per (tile, block) with pairs): when a task is left with a handful of pairs -- a landmark
// shard of a multi-GPU run: 36 pairs per block at C4 / 8 -- the per-task skeleton dominates and the
// untiled list wins (C4 / 8 shard: Schur stage 0.159 -> 0.119 ms).  Decided on the generated list: fewer than 64 pairs
// per task on average -> generated again without tiles.
// Tiles also buy parallelism (tasks) and L2 locality, and cost a combine launch, a partial per task and short tasks.
// When the blocks alone fill the chip twice over and all of Z stays in the Infinity Cache, the untiled list wins (C3: stage
// 56 -> 48 us); at C4 (Z = 640 MB) the tiles' locality is worth 0.53 against 0.77 ms.
template <class Builder>
int ps_pair_list_build(Builder& b, const PairListPolicy& p, int ntiles, int* ntiles_out) {
    const bool z_in_cache = p.zbytes <= PS_PAIRS_CACHE_BYTES && !p.keep_tiles;
    // When all of Z stays in the Infinity Cache the untiled list is the likely winner: build IT first and keep it if the
    // blocks alone fill the chip -- no tiled list is generated only to be thrown away (C3: 23 -> 7 ms)
    if (ntiles > 1 && !p.tiles_forced && !p.by_landmark && z_in_cache) {
        if (b.build(1)) return -1;
        if (b.counts().blocks >= PS_PAIRS_CHIP_BLOCKS) { *ntiles_out = 1; return 0; }
    }
    *ntiles_out = ntiles;
    if (b.build(ntiles)) return -1;
    if (ntiles == 1 || p.tiles_forced) return 0;
    const PairListCounts c = b.counts();
    if (c.pairs == 0) return 0;
    const bool blocks_fill_chip = c.blocks >= PS_PAIRS_CHIP_BLOCKS && z_in_cache;
    if (c.pairs >= PS_PAIRS_MIN_PER_TASK * c.tasks && !blocks_fill_chip) return 0;
    *ntiles_out = 1;
    return b.build(1);
}

// ---- block pattern of the reduced system ------------------------------------------------------------------------------------
// Upper keys (ri << 32 | rj, ri <= rj) of every block: the diagonal, the pair tasks, pose-pose edges and host rows between two
// variable poses, the caller's extra pairs (reduced indices) -> BSR rows with ascending columns, both triangles.
struct BlockPattern {
    std::vector<int32_t> row_ptr, col_idx, diag_slot;
    int slot_of(int a, int b) const {
        const int32_t* lo = col_idx.data() + row_ptr[a];
        const int32_t* hi = col_idx.data() + row_ptr[a + 1];
        const int32_t* it = std::lower_bound(lo, hi, b);
        return (it != hi && *it == b) ? (int)(it - col_idx.data()) : -1;
    }
};
struct BlockPatternIn {
    int nr = 0, dof = 6;
    const int32_t* pose_rid = nullptr;
    const uint64_t* task_key = nullptr; size_t ntask = 0;
    const int32_t *edge_i = nullptr, *edge_j = nullptr; long nedge = 0;             // pose indices, both >= 0
    const int32_t *hrow_i = nullptr, *hrow_j = nullptr; long nhrow = 0;             // pose indices, i may be -1
    const int32_t *extra_i = nullptr, *extra_j = nullptr; long nextra = 0;          // reduced indices
};
// -> nullptr, or the refusal
inline const char* ps_block_pattern(const BlockPatternIn& in, BlockPattern& out) {
    const int nr = in.nr;
    auto upper = [](int ra, int rb) { return ((uint64_t)std::min(ra, rb) << 32) | (uint32_t)std::max(ra, rb); };
    std::vector<uint64_t> keys;
    keys.reserve(in.ntask + nr + in.nedge + in.nhrow + in.nextra);
    for (int r = 0; r < nr; ++r) keys.push_back(upper(r, r));
    keys.insert(keys.end(), in.task_key, in.task_key + in.ntask);
    for (long f = 0; f < in.nedge; ++f) {
        const int ra = in.pose_rid[in.edge_i[f]], rb = in.pose_rid[in.edge_j[f]];
        if (ra >= 0 && rb >= 0 && ra != rb) keys.push_back(upper(ra, rb));
    }
    for (long k = 0; k < in.nhrow; ++k) {
        const int ra = in.hrow_i[k] >= 0 ? in.pose_rid[in.hrow_i[k]] : -1, rb = in.pose_rid[in.hrow_j[k]];
        if (ra >= 0 && rb >= 0) keys.push_back(upper(ra, rb));
    }
    for (long k = 0; k < in.nextra; ++k) {
        const int ra = in.extra_i[k], rb = in.extra_j[k];
        if (ra < 0 || rb < 0 || ra >= nr || rb >= nr) return "extra pair index out of range";
        keys.push_back(upper(ra, rb));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    std::vector<int32_t>& row_ptr = out.row_ptr;
    std::vector<int32_t>& col_idx = out.col_idx;
    row_ptr.assign(nr + 1, 0);
    for (uint64_t k : keys) {
        const int a = (int)(k >> 32), b = (int)(uint32_t)k;
        row_ptr[a + 1]++;
        if (a != b) row_ptr[b + 1]++;
    }
    for (int r = 0; r < nr; ++r) row_ptr[r + 1] += row_ptr[r];
    if ((long)row_ptr[nr] * in.dof * in.dof >= (1L << 31)) return "reduced system too large for 32-bit block offsets";
    col_idx.assign(row_ptr[nr], 0);
    {
        std::vector<int32_t> f2(row_ptr.begin(), row_ptr.end() - 1);
        // lower part first needs sorted columns per row: insert (b,a) pairs in key order gives
        // ascending a for row b; then (a,b) gives ascending b >= a.  Do two passes.
        for (uint64_t k : keys) { const int a = (int)(k >> 32), b = (int)(uint32_t)k; if (a != b) col_idx[f2[b]++] = a; }
        for (uint64_t k : keys) { const int a = (int)(k >> 32), b = (int)(uint32_t)k; col_idx[f2[a]++] = b; }
    }
    out.diag_slot.resize(nr);
    for (int r = 0; r < nr; ++r) out.diag_slot[r] = out.slot_of(r, r);
    return nullptr;
}
