"""Both RANSAC front ends on the device at their selection, shape and input edges: frame-to-frame RANSAC (csrc/ps_ransac.h) against
oracle/ransac_oracle.py, two-view essential-matrix RANSAC (csrc/ps_k_twoview.h) against pyslam_amd/pipelines/epipolar.py.
Run with `-m gpu` on an MI355X.  Every comparison prints its figure before it asserts.

The scenes, sample tables and seeds are tests/ransac_scenes.py's.  tests/test_ransac.py and tests/test_twoview_host.py assert
without a device that the oracle has no (hypothesis, point) pair within 1e-6 relative of the threshold in any of them, that the
winners used here are unique and the samples determined -- so masks, counts and winners are compared EXACTLY."""
import numpy as np
import pytest

import ransac_scenes as rs
from oracle import ransac_oracle as orc

pytestmark = pytest.mark.gpu

TOL_T = 1e-9            # T_all of the samples with sigma_2 / sigma_1 > 1e-3 (tests/test_ransac.py)
TIE_CASES = rs.TIE_POSITIONS + [(257, tuple(range(257)))]
TIE_IDS = ['H{}-at-{}'.format(h, '-'.join(map(str, p)) if len(p) < 8 else 'every-row') for h, p in TIE_CASES]


def f2f_solver(sc, thresh=rs.THRESH, k=3):
    """FrameToFrameRANSAC on the scene's observations (set_obs triangulates them as the scene did)."""
    from pyslam_amd.pipelines.ransac import FrameToFrameRANSAC
    r = FrameToFrameRANSAC(sc['cam'])
    with np.errstate(all='ignore'):
        r.set_obs(sc['obs_1'], sc['obs_2'])
    r.pts_1, r.pts_2, r.obs_2 = sc['pts_1'], sc['pts_2'], sc['obs_2']          # (the offset scene moves the points themselves)
    r.ransac_thresh, r.num_min_set_pts = thresh, k
    return r


def compare_f2f(sc, idx, thresh=rs.THRESH, tol_r=TOL_T, tol_t=TOL_T, what=''):
    """_device_ransac and compute_ransac_cost against the oracle on the same samples -> (device result, oracle dict)."""
    from pyslam_amd import _native as nat
    r = f2f_solver(sc, thresh, idx.shape[1])
    ref = rs.f2f_oracle(sc, idx, thresh)
    T_best, mask, best, count, T_all, counts = r._device_ransac(idx, want_all=True)
    well = ref['cond'] > rs.WELL
    e_r = np.abs(T_all[well, :3, :3] - ref['T_all'][well, :3, :3]).max() if well.any() else 0.
    e_t = np.abs(T_all[well, :3, 3] - ref['T_all'][well, :3, 3]).max() if well.any() else 0.
    print('{}N = {}, H = {}, sets of {}: |C - C_oracle| {:.2e}, |r - r_oracle| {:.2e} over {} rows; best {} / {} count {} / {}'.format(
        what, len(sc['pts_1']), len(idx), idx.shape[1], e_r, e_t, well.sum(), best, ref['best'], count, ref['counts'][ref['best']]))
    assert e_r <= tol_r and e_t <= tol_t
    assert np.array_equal(T_all[:, 3], np.tile([0., 0., 0., 1.], (len(idx), 1)))
    assert np.array_equal(counts, ref['counts'])
    assert best == ref['best'] and count == ref['counts'][ref['best']]
    assert np.array_equal(mask, ref['masks'][best])
    assert np.array_equal(T_best, T_all[best], equal_nan=True)                # bit for bit
    # scoring the device's own transforms again: the same masks bit for bit, the same counts
    masks = r.compute_ransac_cost(T_all, sc['pts_1'], sc['obs_2'], sc['cam'], thresh)
    assert masks.shape == ref['masks'].shape and np.array_equal(masks, ref['masks']) and np.array_equal(masks[best], mask)
    again = np.zeros(len(idx), dtype=np.int32)
    m8 = np.zeros(masks.shape, dtype=np.uint8)
    nat.check(nat.load().ps_ransac_cost(nat.f64p(np.ascontiguousarray(T_all)), len(idx), nat.f64p(np.ascontiguousarray(sc['pts_1'])),
                                        nat.f64p(np.ascontiguousarray(sc['obs_2'])), len(sc['pts_1']), nat.f64p(sc['cam5']), float(thresh),
                                        m8.ctypes.data_as(nat.c_u8p), nat.i32p(again)))
    assert np.array_equal(again, counts) and np.array_equal(m8.astype(bool), masks)
    return (T_best, mask, best, count, T_all, counts), ref


# ---- A. frame-to-frame ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,h,seed,sseed', rs.F2F_SWEEP)
def test_f2f_shape_sweep(n, h, seed, sseed):
    compare_f2f(rs.f2f_scene(n, seed), rs.f2f_samples(n, h, 3, sseed))


@pytest.fixture(scope='module')
def base257():
    """The N = 257 scene, its H = 257 table, the oracle on it and its winner / loser rows (computed once, never changed)."""
    sc = rs.f2f_scene(257, rs.F2F_SEED_257)
    idx = rs.f2f_samples(257, 257, 3, rs.F2F_SEED_257)
    ref = rs.f2f_oracle(sc, idx)
    w, l = rs.winner_and_loser(ref)
    return sc, idx, ref, w, l


@pytest.mark.parametrize('h,positions', TIE_CASES, ids=TIE_IDS)
def test_f2f_ties_go_to_the_first_maximum(base257, h, positions):
    sc, idx, ref, w, l = base257
    table = rs.tie_table(idx, w, l, h, positions)
    T_best, mask, best, count, T_all, counts = f2f_solver(sc)._device_ransac(table, want_all=True)
    print('H = {}, winner row at {}: best {}, count {} (oracle {}), loser count {}'.format(
        h, positions if len(positions) < 8 else 'every row', best, count, ref['counts'][w], ref['counts'][l]))
    assert best == min(positions) and count == ref['counts'][w]
    want = np.full(h, ref['counts'][l])
    want[list(positions)] = ref['counts'][w]
    assert np.array_equal(counts, want)
    assert np.array_equal(T_best, T_all[best]) and (T_all[list(positions)] == T_all[best]).all()
    assert np.abs(T_best - ref['T_all'][w]).max() <= TOL_T
    assert np.array_equal(mask, ref['masks'][w])


def test_f2f_all_zero_counts(base257):
    sc, idx, ref, w, l = base257
    r = f2f_solver(sc, rs.ZERO_THRESH)
    T_best, mask, best, count, T_all, counts = r._device_ransac(idx, want_all=True)
    print('threshold {:.0e}: best {}, count {}, largest count {}'.format(rs.ZERO_THRESH, best, count, counts.max()))
    assert not counts.any() and best == 0 and count == 0 and not mask.any()
    assert np.array_equal(T_best, T_all[0]) and np.abs(T_all[0] - ref['T_all'][0]).max() <= TOL_T
    np.random.seed(3)
    with pytest.raises(ValueError, match='failed to find more than 5 inliers'):
        r.perform_ransac()


def test_f2f_rgbd_camera():
    sc = rs.f2f_scene(257, rs.F2F_SEED_RGBD, rgbd=True)
    assert type(sc['cam']).__name__ == 'RGBDCamera' and sc['cam5'][4] == -1.
    compare_f2f(sc, rs.f2f_samples(257, 257, 3, rs.F2F_SEED_RGBD), what='RGB-D, ')


def test_f2f_non_finite_and_behind_camera_points():
    sc, where = rs.f2f_nonfinite_scene()
    idx, rows = rs.f2f_nonfinite_samples(where)
    (T_best, mask, best, count, T_all, counts), ref = compare_f2f(sc, idx, what='non-finite points, ')
    print('rows with a non-finite sample point {}: counts {}; the point behind the camera is an inlier of {} hypotheses'.format(
        rows, counts[rows].tolist(), int(ref['masks'][:, where['behind']].sum())))
    assert not counts[rows].any() and best not in rows and np.isfinite(T_best).all()
    assert np.isfinite(T_all[np.setdiff1d(np.arange(len(idx)), rows)]).all()
    for k in ('inf_1', 'inf_2', 'nan_2', 'nan_1'):
        assert not mask[where[k]]
    assert mask[where['behind']]
    # only such rows: nothing wins, the first row is returned, and the call returns normally
    r = f2f_solver(sc)
    T_best, mask, best, count, T_all, counts = r._device_ransac(idx[rows], want_all=True)
    assert best == 0 and count == 0 and not counts.any() and not mask.any()
    # z exactly 0 under the identity: 1 / z = inf, never an inlier (as numpy), the other points as the oracle says
    T, pts = rs.f2f_zero_depth_case(sc, ref)
    got = r.compute_ransac_cost(T, pts, sc['obs_2'], sc['cam'], rs.THRESH)
    with np.errstate(all='ignore'):
        err = orc.reprojection_errors(T, pts, sc['obs_2'], sc['cam5'])
    print('z = 0 under the identity: oracle errors {} / {}, device masks {}'.format(err[0, 7], err[0, 8], got[0, 7:9].tolist()))
    assert np.array_equal(got, err < rs.THRESH) and not got[0, 7] and not got[0, 8]


@pytest.mark.parametrize('k', [4, 6])
def test_f2f_larger_minimal_sets(base257, k):
    sc = base257[0]
    compare_f2f(sc, rs.f2f_samples(257, 257, k, rs.F2F_SEED_SETS[k]))


@pytest.mark.parametrize('n', [3, 50])
def test_compute_transform_fast_batches(n):
    from pyslam_amd.liegroups import SE3
    from pyslam_amd.pipelines.ransac import compute_transform_fast
    rng = np.random.default_rng([21, n])
    a = rng.standard_normal((65, n, 3)) * 3.
    b = np.stack([SE3.exp(0.3 * rng.standard_normal(6)).dot(a[k]) + 0.01 * rng.standard_normal((n, 3)) for k in range(65)])
    want = orc.compute_transform(a, b)
    cond = orc.sample_conditioning(a.reshape(-1, 3), b.reshape(-1, 3), np.arange(65 * n).reshape(65, n))
    tol = 1e-12 if n == 50 else 1e-9                              # tests/test_ransac.py: many points / minimal sets
    assert cond.min() > rs.WELL
    for batch in (1, 63, 64, 65):
        T = compute_transform_fast(a[:batch], b[:batch])
        err = np.abs(T - want[:batch]).max()
        print('compute_transform_fast n = {}, batch {}: |T - T_oracle| {:.2e} (worst sigma_2 / sigma_1 {:.2e})'.format(n, batch, err, cond.min()))
        assert T.shape == (batch, 4, 4) and err <= tol
        assert np.array_equal(T, compute_transform_fast(a[:65], b[:65])[:batch])     # a set's answer does not depend on its neighbours


def test_compute_transform_fast_one_and_two_points():
    """LAPACK's completion of a rank-0 / rank-1 cross-covariance is arbitrary: properties instead of values."""
    from pyslam_amd.pipelines.ransac import compute_transform_fast
    rng = np.random.default_rng(22)
    for n in (1, 2):
        a = rng.standard_normal((65, n, 3)) * 3.
        b = rng.standard_normal((65, n, 3)) * 3.
        if n == 2:                                                # equal segment lengths: set 2's segment is set 1's, turned
            d1 = a[:, 1] - a[:, 0]
            d2 = rng.standard_normal((65, 3))
            d2 *= (np.linalg.norm(d1, axis=1) / np.linalg.norm(d2, axis=1))[:, None]
            b[:, 1] = b[:, 0] + d2
        T = compute_transform_fast(a, b)
        C, r = T[:, :3, :3], T[:, :3, 3]
        e_orth = np.abs(np.einsum('bij,bkj->bik', C, C) - np.identity(3)).max()
        e_det = np.abs(np.linalg.det(C) - 1.).max()
        e_r = np.abs(r - (b.mean(axis=1) - np.einsum('bij,bj->bi', C, a.mean(axis=1)))).max()
        print('n = {}: |C C^T - I| {:.2e}, |det C - 1| {:.2e}, |r - (c_2 - C c_1)| {:.2e}'.format(n, e_orth, e_det, e_r))
        assert np.isfinite(T).all() and np.array_equal(T[:, 3], np.tile([0., 0., 0., 1.], (65, 1)))
        assert e_orth <= 1e-12 and e_det <= 1e-12 and e_r <= 1e-12
        if n == 2:
            u1 = (a[:, 1] - a[:, 0]) / np.linalg.norm(a[:, 1] - a[:, 0], axis=1)[:, None]
            u2 = (b[:, 1] - b[:, 0]) / np.linalg.norm(b[:, 1] - b[:, 0], axis=1)[:, None]
            e_dir = np.abs(np.einsum('bij,bj->bi', C, u1) - u2).max()
            print('n = 2: |C d_1 - d_2| {:.2e}'.format(e_dir))
            assert e_dir <= 1e-12


@pytest.mark.parametrize('n', [3, 6])
def test_jacobi_svd_conditioning_ladder(n):
    """Device and LAPACK oracle against the exactly known transform of tests/ransac_scenes.py's dyadic sets, rung by rung.
    Bound: the device's error is at most 10 x the oracle's on the same input, with a floor of 16 ulps of the largest entry of T."""
    from pyslam_amd.pipelines.ransac import compute_transform_fast
    sets = [rs.ladder_set(n, rung) for rung in rs.LADDER_RUNGS]
    T_dev = compute_transform_fast(np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]))
    figures = []
    for rung, (p1, p2, ratio, _), T in zip(rs.LADDER_RUNGS, sets, T_dev):
        e_dev, floor = rs.ladder_error(T)
        e_orc, _ = rs.ladder_error(orc.compute_transform(p1, p2))
        figures.append((e_dev, e_orc, floor))
        print('n = {}, rung {:.0e} (sigma_2 / sigma_1 = {:.2e}): error to the truth, device {:.2e}, oracle {:.2e} (floor {:.2e})'.format(
            n, rung, ratio, e_dev, e_orc, floor))
    # measured on an MI355X, error to the truth device / oracle per rung (floor 2.84e-14):
    #   n = 3:  1: 8.9e-16 / 8.9e-16   1e-2: 9.1e-15 / 1.5e-14   1e-4: 8.8e-13 / 2.1e-12   1e-6: 7.1e-11 / 5.9e-11
    #           1e-8: 1.5e-09 / 2.8e-08   1e-10: 1.6e-06 / 1.3e-06
    #   n = 6:  1: 1.8e-15 / 2.2e-14   1e-2: 1.8e-15 / 1.5e-14   1e-4: 3.0e-13 / 8.0e-13   1e-6: 5.8e-12 / 6.3e-12
    #           1e-8: 1.5e-09 / 1.1e-08   1e-10: 1.0e-07 / 1.7e-06
    # both follow eps sigma_1 / sigma_2; the device is never more than 1.3 x the oracle's error
    for e_dev, e_orc, floor in figures:
        assert np.isfinite(e_dev) and e_dev <= max(10. * e_orc, floor)


def test_f2f_units_and_offsets():
    idx = rs.f2f_samples(65, 64, 3, rs.F2F_SEED_UNITS)
    masks = {}
    for scale in rs.UNIT_SCALES:
        sc = rs.f2f_scene(65, rs.F2F_SEED_UNITS, scale=scale)
        size = np.abs(sc['pts_1']).max()
        (T_best, mask, best, count, T_all, counts), ref = compare_f2f(sc, idx, tol_t=TOL_T * size, what='scale {:.0e}, '.format(scale))
        masks[scale] = ref['masks']
        print('scale {:.0e}: worst |T - T_oracle| {:.2e} (coordinates up to {:.2e})'.format(scale, np.abs(T_all - ref['T_all']).max(), size))
    for scale in rs.UNIT_SCALES:
        assert np.array_equal(masks[scale], masks[1.])              # the device's masks are the oracle's at every scale (compare_f2f)
    sc = rs.f2f_offset_scene(rs.f2f_scene(65, rs.F2F_SEED_UNITS))
    size = np.abs(sc['pts_1']).max()
    (T_best, mask, best, count, T_all, counts), ref = compare_f2f(sc, idx, tol_t=TOL_T * size, what='offset {:.0e}, '.format(rs.UNIT_OFFSET))
    print('offset {:.0e}: worst |T - T_oracle| {:.2e} (coordinates up to {:.2e})'.format(rs.UNIT_OFFSET, np.abs(T_all - ref['T_all']).max(), size))


# ---- B. two-view ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,h,seed,sseed', rs.TV_SWEEP)
def test_twoview_sizes_off_the_stride(n, h, seed, sseed):
    from test_gpu_twoview import compare_hypotheses, compare_ransac
    obs_1, obs_2 = rs.tv_scene(n, seed)
    samples = rs.tv_samples(n, h, sseed)
    compare_hypotheses(obs_1, obs_2, samples, max_left_out=0)
    compare_ransac(obs_1, obs_2, samples, max_left_out=0)


@pytest.fixture(scope='module')
def tv_base():
    """The tie scene, its table, the winner / loser rows of the restatement and the device's H = 1 runs on the winner alone."""
    from test_gpu_twoview import solver
    n, h, seed, sseed = rs.TV_TIES
    obs_1, obs_2 = rs.tv_scene(n, seed)
    samples = rs.tv_samples(n, h, sseed)
    ref = rs.tv_oracle(obs_1, obs_2, samples)[0]
    w, l = rs.winner_and_loser(ref)
    alone = {refit: solver(obs_1, obs_2, refit=refit)._device_ransac(samples[w:w + 1]) for refit in (True, False)}
    return obs_1, obs_2, samples, ref, w, l, alone


@pytest.mark.parametrize('h,positions', TIE_CASES, ids=TIE_IDS)
def test_twoview_ties_go_to_the_first_maximum(tv_base, h, positions):
    from test_gpu_twoview import solver
    obs_1, obs_2, samples, ref, w, l, alone = tv_base
    table = rs.tie_table(samples, w, l, h, positions)
    for refit in (True, False):
        res = solver(obs_1, obs_2, refit=refit)._device_ransac(table)
        print('H = {}, winner row at {}, refit {}: best {}, raw count {} (restatement {}), final {}'.format(
            h, positions if len(positions) < 8 else 'every row', refit, res['best'], res['raw_count'], ref['counts'][w], res['count']))
        assert res['best'] == min(positions) and res['raw_count'] == ref['counts'][w] == alone[refit]['raw_count']
        assert res['count'] == alone[refit]['count'] and res['refit_kept'] == alone[refit]['refit_kept']
        for key in ('mask', 'E', 'T_21', 'cheirality_counts', 'parallax_deg'):
            assert np.array_equal(res[key], alone[refit][key]), key             # bit for bit


def test_twoview_non_finite_observations():
    from test_gpu_twoview import THRESH, TOL_E, rel_fro, solver
    obs_1, obs_2, planted = rs.tv_nonfinite_scene()
    idx, rows = rs.tv_nonfinite_samples(planted)
    ref = rs.tv_oracle(obs_1, obs_2, idx)[0]
    s = solver(obs_1, obs_2)
    E, counts, flags = s._device_hypotheses(idx)
    live = ~ref['degenerate']
    worst = max(rel_fro(E[h], ref['E_all'][h]) for h in np.where(live)[0])
    print('non-finite observations: flagged rows {}, E device vs restatement {:.2e}, best count {} (restatement {})'.format(
        np.where(flags)[0].tolist(), worst, counts.max(), ref['counts'].max()))
    assert np.where(flags)[0].tolist() == rows and np.array_equal(flags, ref['degenerate'])
    assert np.isfinite(E).all() and not E[rows].any() and not counts[rows].any() and worst <= TOL_E
    assert np.array_equal(counts, ref['counts'])
    masks = s.compute_ransac_cost(E, obs_1, obs_2, s.camera, THRESH)
    with np.errstate(invalid='ignore'):
        assert np.array_equal(masks, ref['dist'] < THRESH)
    assert not masks[:, planted].any()
    for refit in (True, False):
        res = solver(obs_1, obs_2, refit=refit)._device_ransac(idx)
        assert res['best'] == ref['best'] and res['best'] not in rows and res['raw_count'] == ref['raw_count']
        assert not res['mask'][planted].any()
        if refit:
            assert np.array_equal(res['mask'], ref['mask']) and res['count'] == ref['count'] and res['refit_kept'] == ref['refit_kept']
            assert np.array_equal(res['cheirality_counts'], ref['cheirality_counts'])
        for key in ('T_21', 'E', 'parallax_deg'):
            assert np.isfinite(res[key]).all(), key
    only = s._device_ransac(idx[rows])
    assert only['best'] == 0 and only['count'] == 0 and not only['mask'].any()
    for key in ('T_21', 'E', 'parallax_deg'):
        assert np.isfinite(only[key]).all(), key
