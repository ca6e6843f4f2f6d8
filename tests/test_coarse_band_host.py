"""The block half-bandwidth of the folded path's coarse matrix (pyslam_amd/csrc/ps_coarse_band.h, compiled here with a plain C++
compiler: no HIP, no GPU) on hand-made run tables, against a brute-force numpy restatement: block (q, q') of A_c = P^T S^ P is
structural iff some row of supp(q) has a non-empty run for q'.  And where the option that uses it ("coarse_chol_band") is set,
read back, documented and launched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bchol_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'coarse_chol_band'


@pytest.fixture(scope='module')
def band(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp('coarse_band') / 'shim.so')
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-O1', '-shared', '-fPIC',
                    '-I' + os.path.join(REPO, 'pyslam_amd', 'csrc'), os.path.join(REPO, 'tests', 'coarse_band_shim.cpp'), '-o', lib], check=True)
    so = C.CDLL(lib)
    p = C.POINTER(C.c_int32)
    so.coarse_band.argtypes = [C.c_int, p, p, p, p]

    def call(slo, shi, run_lo, run_hi):
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (slo, shi, run_lo, run_hi)]
        return so.coarse_band(len(arrs[0]), *[a.ctypes.data_as(p) for a in arrs])
    return call


def brute(slo, shi, run_lo, run_hi):
    """The pattern of A_c written out as a boolean matrix, then its half-bandwidth."""
    ncb = len(slo)
    nonempty = np.asarray(run_hi).reshape(-1, ncb) > np.asarray(run_lo).reshape(-1, ncb)
    pattern = np.zeros((ncb, ncb), dtype=bool)
    for q in range(ncb):
        pattern[q] = nonempty[slo[q]:shi[q]].any(axis=0) if shi[q] > slo[q] else False
    q, q2 = np.nonzero(pattern)
    return int(np.abs(q - q2).max()) if q.size else 0


def tables(nr, ncb, cols_of_row):
    """slo / shi of hat nodes over nr rows and the run tables of rows whose (sorted) columns are cols_of_row[i], as build_coarse
    makes them: the run of row i for node q is the contiguous range of its blocks whose column lies in supp(q)."""
    G = ncb - 1
    slo, shi = np.full(ncb, nr), np.zeros(ncb, dtype=int)
    for i in range(nr):
        u = i * G / (nr - 1) if G and nr > 1 else 0.0
        k = min(max(G - 1, 0), int(u))
        for q in ((k, k + 1) if G and u - k > 0 else (k,)):
            slo[q], shi[q] = min(slo[q], i), max(shi[q], i + 1)
    lo, hi, at = np.zeros((nr, ncb), dtype=int), np.zeros((nr, ncb), dtype=int), 0
    for i in range(nr):
        c = np.asarray(cols_of_row[i])
        for q in range(ncb):
            lo[i, q] = at + np.searchsorted(c, slo[q])
            hi[i, q] = at + np.searchsorted(c, shi[q])
        at += c.size
    return slo, shi, lo.ravel(), hi.ravel()


def test_hand_made_tables(band):
    # a single node: one block, bandwidth 0
    t = tables(5, 1, [[i] for i in range(5)])
    assert band(*t) == brute(*t) == 0
    # every run empty (rows without blocks): nothing structural
    t = tables(12, 4, [[] for _ in range(12)])
    assert band(*t) == brute(*t) == 0
    # a diagonal matrix: a row reaches the nodes of its own support only -> neighbours
    t = tables(40, 5, [[i] for i in range(40)])
    assert band(*t) == brute(*t) == 1
    # a window of +-6 rows over nodes 13 rows apart
    t = tables(40, 4, [list(range(max(0, i - 6), min(40, i + 7))) for i in range(40)])
    assert band(*t) == brute(*t) == 2
    # one long run: row 0 reaches the last row (a loop closure over the whole trajectory) -> dense
    cols = [[i] for i in range(40)]
    cols[0] = [0, 39]
    cols[39] = [0, 39]
    t = tables(40, 6, cols)
    assert band(*t) == brute(*t) == 5
    # the same long run seen from one side only (the tables need not be symmetric for the function to see it)
    cols[39] = [39]
    t = tables(40, 6, cols)
    assert band(*t) == brute(*t) == 5
    # an empty support (a node no row hangs on) between two others
    slo, shi = [0, 3, 3], [3, 3, 6]
    lo = np.zeros((6, 3), dtype=int)
    hi = np.zeros((6, 3), dtype=int)
    hi[0, 2] = 1                                             # row 0 (node 0) has a run for node 2
    hi[4, 1] = 1                                             # row 4 (node 2) has a run for the empty node 1
    assert band(slo, shi, lo.ravel(), hi.ravel()) == brute(slo, shi, lo.ravel(), hi.ravel()) == 2


@pytest.mark.parametrize('seed', range(8))
def test_random_windows_against_the_restatement(band, seed):
    rng = np.random.default_rng(seed)
    nr, ncb = int(rng.integers(2, 200)), int(rng.integers(1, 16))
    w = int(rng.integers(0, 25))
    cols = []
    for i in range(nr):
        c = set(range(max(0, i - w), min(nr, i + w + 1)))
        if rng.random() < 0.02:
            c.add(int(rng.integers(0, nr)))                  # a stray long edge now and then
        if rng.random() < 0.1:
            c = set()                                        # rows without blocks
        cols.append(sorted(c))
    t = tables(nr, ncb, cols)
    assert band(*t) == brute(*t)
    assert 0 <= band(*t) <= ncb - 1


def test_the_chain_family_is_the_ill_conditioned_one():
    """tests/test_gpu_coarse_chol_band.py runs the kernels on it: block tridiagonal in 6 x 6 blocks, condition ~ nodes^2 (2.6e2 at
    C3's 78 unknowns, 3e4 at the 800 of tests/test_gpu_bchol_kernels.py) against ~5 of the Gram family."""
    A = R.chain(78, 78)
    assert 1e2 < np.linalg.cond(A) < 1e3 and np.linalg.cond(R.gram(78, 78)) < 10
    q = np.arange(78) // 6
    assert np.all(A[np.abs(q[:, None] - q[None, :]) > 1] == 0.0) and not np.signbit(A[np.abs(q[:, None] - q[None, :]) > 1]).any()


def read(*parts):
    with open(os.path.join(REPO, *parts)) as f:
        return f.read()


def test_the_option_is_set_read_back_documented_and_launched():
    solver = read('pyslam_amd', 'csrc', 'ps_abi_solver.h')
    setter = re.search(r'int ps_set_option\(.*?\n}\n', solver, re.S).group(0)
    getter = re.search(r'int ps_get_option\(.*?\n}\n', solver, re.S).group(0)
    assert 0 < setter.index('"%s"' % NAME) < setter.index('ps_option_apply(')          # ahead of the table, whose rows stay
    assert '"%s"' % NAME not in read('pyslam_amd', 'csrc', 'ps_options.h')
    for n in (NAME, 'coarse_chol_bw', 'coarse_nodes'):
        assert 'n == "%s"' % n in getter
    header = read('include', 'pyslam_hip.h')
    assert '"%s"' % NAME in re.search(r'/\* Tuning knobs.*?\*/\s*int ps_set_option', header, re.S).group(0)
    assert '"coarse_chol_bw"' in re.search(r'int ps_set_option.*?int ps_get_option', header, re.S).group(0)
    assert 'int coarse_chol_band = 1;' in read('pyslam_amd', 'csrc', 'ps_core.hip')     # default on
    host = read('pyslam_amd', 'csrc', 'ps_host_cg.h')
    factor = re.search(r'int coarse_factor\(.*?\n}\n', host, re.S).group(0)
    assert 'if (h->coarse_chol_band)' in factor and 'k_coarse_chol_band<D>' in factor and 'k_coarse_chol<D, true>' in factor
    touch = read('pyslam_amd', 'csrc', 'ps_abi_problem.h')
    assert 'PS_TOUCH(k_coarse_chol_band<6>)' in touch and 'PS_TOUCH(k_coarse_chol_band<3>)' in touch
    for doc in ('DESIGN.md', 'HISTORY.md'):
        assert '`%s`' % NAME in read(doc), doc


def test_the_test_entry_is_declared_and_bound():
    from pyslam_amd import _native
    header = read('include', 'pyslam_hip.h')
    decl = re.search(r'int ps_debug_coarse_chol\((.*?)\);', header, re.S).group(1)
    assert len(decl.split(',')) == len(_native.SIGNATURES['ps_debug_coarse_chol'][1]) == 9
    assert 'int ps_debug_coarse_chol(' in read('pyslam_amd', 'csrc', 'ps_abi_small.h')
