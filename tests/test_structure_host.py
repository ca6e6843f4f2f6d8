"""The structure decisions of ps_problem_create that need no GPU (pyslam_amd/csrc/ps_structure.h, compiled here with a plain C++
compiler): the tiled / untiled policy of the Schur pair list, driven by a scripted builder that answers (pairs, tasks, blocks)
per tile count and records the builds it was asked for -- one case per branch of the policy -- and the block pattern of the
reduced system against a dense numpy construction of the same sparse pattern."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1048576.
CHIP = 2 * 256 * 12             # blocks that fill the chip twice over: 6144
ZROW = 144                      # bytes of a Z row


@pytest.fixture(scope='module')
def so(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp('structure') / 'shim.so')
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-O1', '-shared', '-fPIC',
                    '-I' + os.path.join(REPO, 'pyslam_amd', 'csrc'), os.path.join(REPO, 'tests', 'structure_shim.cpp'), '-o', lib], check=True)
    so = C.CDLL(lib)
    so.st_tiles.argtypes = [C.c_double] * 3
    so.st_default_tiles.argtypes = [C.c_double]
    so.st_drive.argtypes = [C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                            C.c_void_p, C.c_void_p]
    so.st_pattern.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p,
                              C.c_long, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]
    return so


def drive(so, zbytes, ntiles, script, forced=False, keep=False, by_landmark=False):
    """script: {tile count: (pairs, tasks, blocks)} -> (return value, [tile counts built, in order], tile count that stands)"""
    tiles = np.array(sorted(script), np.int32)
    counts = np.array([script[t] for t in sorted(script)], np.int64).reshape(-1)
    calls = np.full(8, -1, np.int32)
    ncalls, out = C.c_int(-1), C.c_int(-1)
    rc = so.st_drive(zbytes, int(forced), int(keep), int(by_landmark), ntiles, len(tiles), tiles.ctypes.data, counts.ctypes.data, 8,
                     calls.ctypes.data, C.byref(ncalls), C.byref(out))
    assert 0 <= ncalls.value <= 8
    return rc, list(calls[:ncalls.value]), out.value


def test_the_tile_count(so):
    # 8 tiles per 8 x 9 MiB of Z, none up to 16 MiB: C3 (72 MB of Z) has 8, C4 (640 MB) 72
    assert so.st_default_tiles(16 * MIB) == 1 and so.st_default_tiles(16 * MIB + ZROW) == 8
    assert so.st_default_tiles(72e6) == 8 and so.st_default_tiles(640e6) == 72
    assert so.st_default_tiles(8 * 9216 * 1024.) == 8 and so.st_default_tiles(8 * 9216 * 1024. + 1) == 16
    assert so.st_tiles(30 * MIB, 256., 16.) == 8 * 15 and so.st_tiles(30 * MIB, 0., 16.) == 1       # PS_SCHUR_TILE_KB
    assert so.st_tiles(2 * MIB, 9216., 1.) == 8 and so.st_tiles(MIB, 9216., 1.) == 1               # PS_SCHUR_TILE_MIN_MB


def test_a_small_z_is_one_tile_from_the_start(so):
    assert drive(so, 10 * MIB, 1, {1: (10 ** 6, 500, 500)}) == (0, [1], 1)
    assert drive(so, 10 * MIB, 1, {1: (10, 10, 10)}) == (0, [1], 1)                 # short tasks are no reason to build it twice


def test_z_in_the_cache_and_blocks_that_fill_the_chip_keep_the_untiled_list(so):
    assert drive(so, 72e6, 8, {1: (2 * 10 ** 6, CHIP, CHIP)}) == (0, [1], 1)         # no tiled list is ever built
    assert drive(so, 128 * MIB, 8, {1: (2 * 10 ** 6, CHIP + 9, CHIP + 9)}) == (0, [1], 1)


@pytest.mark.parametrize('tasks', [1, 7000, 40000])
def test_z_in_the_cache_with_fewer_blocks_tries_the_tiles_and_the_64_pairs_rule_decides(so, tasks):
    untiled = (64 * tasks, CHIP - 1, CHIP - 1)
    assert drive(so, 72e6, 8, {1: untiled, 8: (64 * tasks, tasks, CHIP - 1)}) == (0, [1, 8], 8)          # pairs == 64 * ntask keeps
    assert drive(so, 72e6, 8, {1: untiled, 8: (64 * tasks + 1, tasks, CHIP - 1)}) == (0, [1, 8], 8)
    assert drive(so, 72e6, 8, {1: untiled, 8: (64 * tasks - 1, tasks, CHIP - 1)}) == (0, [1, 8, 1], 1)   # rebuilt untiled


def test_z_above_128_mib_is_never_tried_untiled_first(so):
    z = 128 * MIB + ZROW
    assert drive(so, z, 16, {16: (64 * 9000, 9000, CHIP + 100)}) == (0, [16], 16)      # blocks that fill the chip: not in the cache
    assert drive(so, z, 16, {16: (64 * 9000 - 1, 9000, 100), 1: (64 * 9000 - 1, 100, 100)}) == (0, [16, 1], 1)
    assert drive(so, 640e6, 72, {72: (22500000, 150000, 80000)}) == (0, [72], 72)      # C4


def test_without_an_untiled_build_to_try_first_the_blocks_are_judged_on_the_tiled_list(so):
    tiled = {8: (64 * 9000, 9000, CHIP), 1: (64 * 9000, CHIP, CHIP)}
    assert drive(so, 72e6, 8, tiled, by_landmark=True) == (0, [8, 1], 1)               # PS_PAIRS_BY_LANDMARK
    tiled[8] = (64 * 9000, 9000, CHIP - 1)
    assert drive(so, 72e6, 8, tiled, by_landmark=True) == (0, [8], 8)
    tiled[8] = (64 * 9000, 9000, CHIP)
    assert drive(so, 72e6, 8, tiled, keep=True) == (0, [8], 8)                         # PS_SCHUR_KEEP_TILES: no first try either
    tiled[8] = (64 * 9000 - 1, 9000, CHIP)
    assert drive(so, 72e6, 8, tiled, keep=True) == (0, [8, 1], 1)                      # ... but the 64-pairs rule still holds


def test_forced_tiles_are_never_rebuilt(so):
    short = {120: (1000, 900, 900), 1: (1000, 900, 900)}
    assert drive(so, 30 * MIB, 120, short, forced=True) == (0, [120], 120)
    assert drive(so, 30 * MIB, 120, {120: (10 ** 7, CHIP * 3, CHIP), 1: (10 ** 7, CHIP, CHIP)}, forced=True) == (0, [120], 120)
    assert drive(so, 300 * MIB, 120, short, forced=True) == (0, [120], 120)


def test_zero_pairs(so):
    assert drive(so, 10 * MIB, 1, {1: (0, 0, 0)}) == (0, [1], 1)
    assert drive(so, 72e6, 8, {1: (0, 0, 0), 8: (0, 0, 0)}) == (0, [1, 8], 8)          # nothing to judge: the tile count stands
    assert drive(so, 300 * MIB, 24, {24: (0, 0, 0)}) == (0, [24], 24)


def test_a_failing_build_ends_the_driver(so):
    assert drive(so, 72e6, 8, {8: (1, 1, 1)})[:2] == (-1, [1])
    assert drive(so, 72e6, 8, {1: (5, 5, 5)})[:2] == (-1, [1, 8])
    assert drive(so, 300 * MIB, 24, {24: (5, 5, 5)})[:2] == (-1, [24, 1])


# ---- block pattern
def i32(x):
    return np.ascontiguousarray(x, np.int32).reshape(-1)


def pattern(so, nr, pose_rid, keys=(), edges=(), hrows=(), extras=(), dof=6):
    """keys: (a, b) reduced, a <= b; edges / hrows: (pose i, pose j); extras: (reduced a, reduced b) -> row_ptr, col_idx, diag_slot"""
    rid = i32(pose_rid)
    tk = np.ascontiguousarray([(a << 32) | b for a, b in keys], np.uint64)
    cols = [(i32([p[0] for p in t]), i32([p[1] for p in t])) for t in (edges, hrows, extras)]
    cap = nr * nr + 1
    row_ptr, col_idx, diag = np.full(nr + 1, -7, np.int32), np.full(cap, -7, np.int32), np.full(max(nr, 1), -7, np.int32)
    nnzb, refusal = C.c_long(-1), C.c_char_p()
    rc = so.st_pattern(nr, dof, rid.ctypes.data, tk.ctypes.data, len(tk), cols[0][0].ctypes.data, cols[0][1].ctypes.data, len(edges),
                       cols[1][0].ctypes.data, cols[1][1].ctypes.data, len(hrows), cols[2][0].ctypes.data, cols[2][1].ctypes.data,
                       len(extras), row_ptr.ctypes.data, col_idx.ctypes.data, cap, diag.ctypes.data, C.byref(nnzb), C.byref(refusal))
    if rc == 1:
        return refusal.value.decode()
    assert rc == 0 and 0 <= nnzb.value < cap
    return row_ptr, col_idx[:nnzb.value], diag[:nr]


def numpy_pattern(nr, pose_rid, keys=(), edges=(), hrows=(), extras=(), dof=6):      # (dof: the 32-bit limit only)
    rid = np.asarray(pose_rid)
    M = np.eye(nr, dtype=bool)
    for a, b in list(keys) + list(extras):
        M[a, b] = M[b, a] = True
    for i, j in list(edges) + list(hrows):
        ra, rb = (rid[i] if i >= 0 else -1), rid[j]
        if ra >= 0 and rb >= 0:
            M[ra, rb] = M[rb, ra] = True
    row_ptr = np.concatenate([[0], np.cumsum(M.sum(1))]).astype(np.int32)
    col_idx = np.nonzero(M)[1].astype(np.int32)          # row-major: ascending columns per row
    diag = np.array([row_ptr[r] + np.count_nonzero(M[r, :r]) for r in range(nr)], np.int32)
    return row_ptr, col_idx, diag


def same_pattern(so, nr, pose_rid, **kw):
    got, want = pattern(so, nr, pose_rid, **kw), numpy_pattern(nr, pose_rid, **kw)
    assert not isinstance(got, str), got
    assert np.array_equal(got[0], want[0])
    for r in range(nr):
        assert np.array_equal(np.sort(got[1][got[0][r]:got[0][r + 1]]), want[1][want[0][r]:want[0][r + 1]]), r
    assert np.array_equal(got[1], want[1])               # (and they ARE sorted: slot look-ups are binary searches)
    assert np.array_equal(got[2], want[2])
    return got


def test_the_pattern_of_one_variable_pose(so):
    row_ptr, col_idx, diag = same_pattern(so, 1, [-1, 0, -1])
    assert list(row_ptr) == [0, 1] and list(col_idx) == [0] and list(diag) == [0]
    same_pattern(so, 1, [-1, 0, -1], keys=[(0, 0)], edges=[(0, 1), (1, 2)], hrows=[(-1, 1), (2, 1)], extras=[(0, 0)])


def test_the_pattern_without_keys_is_the_diagonal_plus_the_factors(so):
    rid = [0, 1, 2, 3, 4]
    assert list(same_pattern(so, 5, rid)[1]) == [0, 1, 2, 3, 4]
    same_pattern(so, 5, rid, edges=[(0, 1), (1, 2), (4, 0)])
    same_pattern(so, 5, rid, hrows=[(-1, 3), (2, 4)], extras=[(4, 1), (1, 4), (3, 3)])
    assert pattern(so, 0, [-1, -1])[0].tolist() == [0]            # no variable pose at all: an empty pattern


def test_duplicate_keys_and_an_edge_to_a_constant_pose(so):
    rid = [-1, 0, 1, -1, 2, 3]                              # poses 0 and 3 are constant
    keys = [(0, 1), (0, 1), (0, 3), (1, 1), (0, 1), (2, 3), (0, 3)]     # tiles repeat a block's key; a diagonal task
    got = same_pattern(so, 4, rid, keys=keys, edges=[(0, 1), (2, 3), (1, 2), (2, 1), (4, 5)], hrows=[(3, 5), (-1, 4), (1, 5)])
    assert got[0][-1] == 4 + 2 * 3                          # (0,1) (0,3) (2,3) once each: no block through a constant pose
    same_pattern(so, 4, rid, keys=keys, edges=[(0, 3)])     # an edge between two constant poses


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_a_random_pattern(so, seed):
    rng = np.random.default_rng(seed)
    P, nr = 40, 29
    rid = np.full(P, -1)
    rid[rng.permutation(P)[:nr]] = rng.permutation(nr)
    keys = [tuple(sorted(rng.integers(0, nr, 2))) for _ in range(150)]
    edges = [tuple(p) for p in rng.integers(0, P, (60, 2)) if p[0] != p[1]]
    hrows = [(-1 if rng.random() < 0.3 else int(p[0]), int(p[1])) for p in rng.integers(0, P, (30, 2)) if p[0] != p[1]]
    extras = [tuple(p) for p in rng.integers(0, nr, (20, 2))]
    same_pattern(so, nr, rid, keys=keys, edges=edges, hrows=hrows, extras=extras)
    same_pattern(so, nr, rid, keys=keys, edges=edges, hrows=hrows, extras=extras, dof=3)


def test_an_extra_pair_out_of_range_is_refused_in_the_same_words(so):
    for bad in [(0, 3), (3, 0), (-1, 1), (1, -1), (7, 7)]:
        assert pattern(so, 3, [0, 1, 2], extras=[(0, 1), bad]) == 'extra pair index out of range'
    assert not isinstance(pattern(so, 3, [0, 1, 2], extras=[(2, 2), (0, 2)]), str)
