// The pair-list policy and the block pattern of pyslam_amd/csrc/ps_structure.h behind a C interface, for
// tests/test_structure_host.py (ctypes).
#include "ps_structure.h"

namespace {
// a pair builder that answers from a script: counts[3 * k ..] = (pairs, tasks, blocks) of a build with ntiles_of[k] tiles
struct ScriptedBuilder {
    const int* ntiles_of; const long* script; int nscript;
    int* calls; int ncalls = 0, max_calls;
    PairListCounts last;
    int build(int ntiles) {
        if (ncalls < max_calls) calls[ncalls] = ntiles;
        ++ncalls;
        for (int k = 0; k < nscript; ++k)
            if (ntiles_of[k] == ntiles) { last = {(size_t)script[3 * k], (size_t)script[3 * k + 1], (size_t)script[3 * k + 2]}; return 0; }
        return -1;                              // a tile count the script does not know: the build fails
    }
    PairListCounts counts() { return last; }
};
}  // namespace

extern "C" {
int st_tiles(double zbytes, double tile_kb, double min_mb) { return ps_pair_tiles(zbytes, tile_kb, min_mb); }
int st_default_tiles(double zbytes) { return ps_pair_tiles(zbytes); }

// -> the driver's return value; calls[0 .. *ncalls) = the tile counts of the builds in order, *ntiles_out = the list that stands
int st_drive(double zbytes, int tiles_forced, int keep_tiles, int by_landmark, int ntiles, int nscript, const int* ntiles_of,
             const long* script, int max_calls, int* calls, int* ncalls, int* ntiles_out) {
    ScriptedBuilder b{ntiles_of, script, nscript, calls, 0, max_calls, {}};
    PairListPolicy p;
    p.zbytes = zbytes; p.tiles_forced = tiles_forced != 0; p.keep_tiles = keep_tiles != 0; p.by_landmark = by_landmark != 0;
    const int rc = ps_pair_list_build(b, p, ntiles, ntiles_out);
    *ncalls = b.ncalls;
    return rc;
}

// -> 0, or 1 with *refusal set; row_ptr: nr + 1, diag_slot: nr, col_idx: up to cap entries, *nnzb = entries of the pattern
int st_pattern(int nr, int dof, const int32_t* pose_rid, const uint64_t* task_key, long ntask, const int32_t* edge_i, const int32_t* edge_j,
               long nedge, const int32_t* hrow_i, const int32_t* hrow_j, long nhrow, const int32_t* extra_i, const int32_t* extra_j,
               long nextra, int32_t* row_ptr, int32_t* col_idx, long cap, int32_t* diag_slot, long* nnzb, const char** refusal) {
    BlockPatternIn in;
    in.nr = nr; in.dof = dof; in.pose_rid = pose_rid;
    in.task_key = task_key; in.ntask = (size_t)ntask;
    in.edge_i = edge_i; in.edge_j = edge_j; in.nedge = nedge;
    in.hrow_i = hrow_i; in.hrow_j = hrow_j; in.nhrow = nhrow;
    in.extra_i = extra_i; in.extra_j = extra_j; in.nextra = nextra;
    BlockPattern pat;
    *refusal = ps_block_pattern(in, pat);
    if (*refusal) return 1;
    *nnzb = (long)pat.col_idx.size();
    std::copy(pat.row_ptr.begin(), pat.row_ptr.end(), row_ptr);
    std::copy(pat.diag_slot.begin(), pat.diag_slot.end(), diag_slot);
    std::copy(pat.col_idx.begin(), pat.col_idx.begin() + std::min<long>(cap, *nnzb), col_idx);
    for (int r = 0; r < nr; ++r)                 // slot_of agrees with diag_slot (the stages look blocks up through it)
        if (pat.slot_of(r, r) != pat.diag_slot[r]) return 2;
    return 0;
}
}
