"""The coarse factorisation that leaves out the structural zeros of a block-banded A_c (csrc/ps_k_coarse.h: k_coarse_chol_band,
option "coarse_chol_band", default) against k_coarse_chol (option 0): every entry that is computed goes through the same
operations in the same order and the terms left out are +-0 added to a sum that started at +0.0, so L^-1, its transpose and the
status words are compared bit for bit -- kernel against kernel through ps_debug_coarse_chol, and whole solves with the option on
against off.  No reference counterpart (the reference factors the reduced system on the host: pyslam/problem.py:186)."""
import functools

import numpy as np
import pytest

from pyslam_amd import synthetic
from pyslam_amd.problem import Options
import bchol_restatement as R

pytestmark = pytest.mark.gpu

ST_DIAG_FAIL = 1
NCB = {6: (1, 2, 3, 4, 5, 8, 9, 13, 15),       # the edges of the doubling levels; 13: the C3 workload; 15: the LDS limit (90 unknowns)
       3: (1, 7, 16, 17, 30)}
BWS = (0, 1, 2, 3, None)                       # None: ncb - 1, the dense matrix


def block_band(A, D):
    """Block half-bandwidth of A's non-zero pattern (a -0.0 counts as non-zero: the kernel's argument needs +0.0)."""
    ncb = A.shape[0] // D
    nz = (A != 0.0) | np.signbit(A)
    blk = nz.reshape(ncb, D, ncb, D).any(axis=(1, 3))
    q, q2 = np.nonzero(blk)
    return int(np.abs(q - q2).max()) if q.size else 0


def banded_spd(ncb, D, bw, seed):
    """B B^T + n I from a block-banded B of half-bandwidth bw // 2: half-bandwidth 2 (bw // 2) <= bw, exact +0.0 outside."""
    n, hb = ncb * D, bw // 2
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    q = np.arange(n) // D
    B[np.abs(q[:, None] - q[None, :]) > hb] = 0.0
    # (summed block by block over the band only: a product with a structural zero never enters, so nothing outside is -0.0)
    A = np.zeros((n, n))
    for i in range(ncb):
        for j in range(max(0, i - 2 * hb), min(ncb, i + 2 * hb + 1)):
            lo, hi = max(0, i - hb, j - hb), min(ncb, i + hb + 1, j + hb + 1)
            if lo < hi:
                A[i * D:(i + 1) * D, j * D:(j + 1) * D] = B[i * D:(i + 1) * D, lo * D:hi * D] @ B[j * D:(j + 1) * D, lo * D:hi * D].T
    A = 0.5 * (A + A.T) + n * np.eye(n)
    return A


def matrices(ncb, D, bw):
    """[(name, A)] for one (ncb, D, bw): every matrix's band is at most bw."""
    n = ncb * D
    out = [('banded', banded_spd(ncb, D, bw, seed=100 * ncb + 10 * D + bw))]
    chain = R.chain(n, n)                                   # 6 x 6 block tridiagonal
    if block_band(chain, D) <= bw:
        out.append(('chain', chain))
    if bw == ncb - 1:
        out.append(('gram', R.gram(n, n)))
    return out


def run(A, ncb, D, bw, variant):
    from pyslam_amd.device import coarse_chol
    Li, LiT, status, _ = coarse_chol(A, ncb, D, bw, variant)
    return Li, LiT, status


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize('D,ncb', [(D, ncb) for D in (6, 3) for ncb in NCB[D]])
def test_band_kernel_equals_the_dense_kernel_bit_for_bit(D, ncb):
    n = ncb * D
    seen = set()
    for b in BWS:
        bw = min(ncb - 1, ncb - 1 if b is None else b)
        if bw in seen:
            continue
        seen.add(bw)
        for name, A in matrices(ncb, D, bw):
            # the zeros outside the band are exact +0.0
            q = np.arange(n) // D
            outside = np.abs(q[:, None] - q[None, :]) > bw
            assert np.all(A[outside] == 0.0) and not np.signbit(A[outside]).any(), (name, bw)
            assert block_band(A, D) <= bw and np.array_equal(A, A.T)
            ref = run(A, ncb, D, bw, 0)
            new = run(A, ncb, D, bw, 1)
            assert ref[2][ST_DIAG_FAIL] == 0 and np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1])), (name, bw)
            assert np.array_equal(ref[0], ref[1].T) and np.all(np.triu(ref[0], 1) == 0.0)
            assert same_bits(new, ref), (name, ncb, D, bw, np.abs(new[0] - ref[0]).max())
            assert same_bits(run(A, ncb, D, bw, 1), new), (name, bw)          # two launches are identical
            # (and it is the inverse factor: Li A Li^T = I to rounding, so two wrong kernels cannot agree)
            assert R.residual(new[0], A) <= 1e-9, (name, bw)


@pytest.mark.parametrize('D,ncb,bw', [(6, 13, 3), (3, 17, 2), (6, 5, 4)])
def test_failure_exits(D, ncb, bw):
    """A negated diagonal entry in block 0, in a middle block and in the last block, and a NaN inside the band: both kernels
    report the pivot; what they leave in the outputs is not compared."""
    n = ncb * D
    A0 = banded_spd(ncb, D, bw, seed=3)
    bad = []
    for blk in (0, ncb // 2, ncb - 1):
        A = A0.copy()
        k = blk * D + (1 if blk else 0)
        A[k, k] = -A[k, k]
        bad.append(A)
    A = A0.copy()
    i, j = (ncb // 2) * D + 2, (ncb // 2 - min(bw, 1)) * D + 1            # inside the band, lower triangle
    A[i, j] = A[j, i] = np.nan
    bad.append(A)
    for A in bad:
        for variant in (0, 1):
            assert run(A, ncb, D, bw, variant)[2][ST_DIAG_FAIL] > 0
    assert run(A0, ncb, D, bw, 1)[2][ST_DIAG_FAIL] == 0


# ---- handle level: the option on against off ------------------------------------------------------------------------------------
def with_edge(lp, truth, i, j):
    """The pose graph plus one edge i -> j measured without noise."""
    from pyslam_amd.lowering import pack_pose_matrices
    T = truth['poses']
    meas = T[j].dot(np.linalg.inv(T[i]))
    out = lp.copy()
    out.e_i = np.append(lp.e_i, i).astype(lp.e_i.dtype)
    out.e_j = np.append(lp.e_j, j).astype(lp.e_j.dtype)
    out.e_Tobs_inv = np.vstack([lp.e_Tobs_inv, pack_pose_matrices(np.linalg.inv(meas)[None])])
    out.e_grp = np.append(lp.e_grp, 0).astype(lp.e_grp.dtype)
    return out.finalize()


@functools.lru_cache(maxsize=None)
def handle_case(name):
    if name == 'ba30':
        return synthetic.stereo_ba(num_kf=30, num_lm=1500, obs_per_lm=6, half_window=4, seed=2)[0]
    if name == 'ba60':
        return synthetic.stereo_ba(num_kf=60, num_lm=3000, obs_per_lm=6, half_window=4, seed=3)[0]
    if name == 'pg_se3':
        return synthetic.pose_graph(num_poses=100, num_loops=60, dof=6, seed=4)[0]
    if name == 'pg_se3_long_loop':
        return with_edge(*synthetic.pose_graph(num_poses=100, num_loops=60, dof=6, seed=4), 0, 90)
    if name == 'pg_se2':
        return synthetic.pose_graph(num_poses=100, num_loops=60, dof=3, seed=5)[0]
    raise KeyError(name)


def solve(lp, on):
    from pyslam_amd.device import DeviceProblem
    dev = DeviceProblem(lp)
    assert dev.get_option('coarse_chol_band') == 1          # default on
    dev.set_option('coarse_chol_band', on)
    assert dev.get_option('coarse_chol_band') == on
    opt = Options()
    opt.max_iters, opt.allow_nondecreasing_steps = 2, True
    hist, its, _ = dev.solve_loop(opt)
    out = [np.array(hist), np.array(its)] + list(dev.get_params())
    ncb, bw = int(dev.get_option('coarse_nodes')), int(dev.get_option('coarse_chol_bw'))
    dev.close()
    return out, ncb, bw


@pytest.mark.parametrize('name,banded', [('ba30', True), ('ba60', True), ('pg_se3', True), ('pg_se3_long_loop', False), ('pg_se2', True)])
def test_option_on_equals_option_off_bit_for_bit(name, banded):
    lp = handle_case(name)
    on, ncb, bw = solve(lp, 1)
    off, ncb0, bw0 = solve(lp, 0)
    print('%s: coarse nodes %d, block half-bandwidth %d' % (name, ncb, bw))
    assert (ncb, bw) == (ncb0, bw0) and ncb >= 2 and ncb * lp.dof <= 90      # the LDS branch of coarse_factor
    if banded:
        assert 0 < bw < ncb - 1                             # (so that this cannot pass by running dense)
    else:
        assert bw == ncb - 1
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(a, b, equal_nan=True), (name, k)
    assert np.all(np.isfinite(on[0])) and on[0][-1] < on[0][0] and on[1].shape[0] >= 2 and np.all(on[1][:, 0] > 0)
