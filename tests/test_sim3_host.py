"""Similarity (Sim(3)) alignment, host side: the restatement (pyslam_amd/pipelines/similarity.py) against known answers, its
degeneracy, tie and refit rules, the scene generator, the draws of Sim3RANSAC.draw_samples, the C ABI of the new exports, the error
paths of pyslam_amd/pipelines/sim3.py, and the conditions tests/test_gpu_sim3.py relies on for every committed seed and shape
(tests/sim3_scenes.py).  No device."""
import os
import re

import numpy as np
import pytest

import sim3_scenes as sc
from pyslam_amd import synthetic
from pyslam_amd.liegroups import SE3, SO3
from pyslam_amd.pipelines import similarity as sm
from pyslam_amd.pipelines import sim3

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def known_model(seed=3, scale=1.7):
    rng = np.random.default_rng(seed)
    R = SO3.exp(np.array([0.3, -0.7, 0.4])).as_matrix()
    t = np.array([0.5, -1.5, 2.0])
    p1 = rng.uniform(-2., 2., (40, 3)) + np.array([0., 0., 6.])
    return p1, scale * p1 @ R.T + t, scale, R, t


def test_the_scene_generator():
    p1, p2, o1, o2, s, T, outlier = synthetic.sim3_scene()
    assert p1.shape == p2.shape == (192, 3) and o1.shape == o2.shape == (192, 2) and s == 2.5 and outlier.sum() == 57 and outlier[:57].all()
    again = synthetic.sim3_scene()
    assert all(np.array_equal(a, b) for a, b in zip(again[:4], (p1, p2, o1, o2)))
    clean = synthetic.sim3_scene(outlier_fraction=0., point_noise=0., pixel_noise=0.)
    assert not clean[6].any() and np.array_equal(clean[0], synthetic.two_view_points(rotvec=(0.04, -0.3, 0.06), t=(1.5, -0.2, 0.8)))
    assert np.abs(clean[1] - (s * clean[0] @ T[:3, :3].T + T[:3, 3])).max() < 1e-12           # p_2 = s R p_1 + t with T_21 = [R | t]
    assert np.abs(clean[2] - sc.project(clean[0])).max() < 1e-10 and np.abs(clean[3] - sc.project(clean[1])).max() < 1e-10
    assert (clean[1][:, 2] > 0.).all()
    # the outliers are real points matched to the wrong partner: the rows rotated by one place among themselves
    noisy = synthetic.sim3_scene(outlier_fraction=0.)
    assert np.array_equal(p2[57:], noisy[1][57:]) and np.array_equal(p2[1:57], noisy[1][:56]) and np.array_equal(p2[0], noisy[1][56])
    assert np.array_equal(o2[1:57], noisy[3][:56]) and np.array_equal(p1, noisy[0]) and np.array_equal(o1, noisy[2])
    # the depth noise is along the ray: the projections do not move
    assert np.abs(sc.project(noisy[0]) - sc.project(clean[0])).max() < 1e-10


def test_exact_points_are_recovered():
    p1, p2, s, R, t = known_model()
    S, s_fit, ok, ratio = sm.fit(p1, p2)
    err = max(np.abs(S[:3, :3] - s * R).max(), np.abs(S[:3, 3] - t).max(), abs(s_fit - s))
    print('40 exact pairs: max error {:.2e}, sigma_b / sigma_a {:.3f}'.format(err, ratio))
    assert ok and err <= 1e-12 and np.array_equal(S[3], [0., 0., 0., 1.])
    for smp in sc.samples_of(40, 16):                         # every minimal set as well
        S3, s3, ok3, _ = sm.fit(p1[smp], p2[smp])
        assert ok3 and max(np.abs(S3[:3, :3] - s * R).max(), np.abs(S3[:3, 3] - t).max(), abs(s3 - s)) <= 1e-12 * 100
    res = sm.ransac(p1, p2, None, None, None, sc.samples_of(40, 8), 1e-12)
    assert res['count'] == 40 and res['best'] == 0 and res['reason'] == sm.FIXED_POINT and res['rounds'] == 1
    cam = sc.CAM
    res = sm.ransac(p1, p2, sc.project(p1), sc.project(p2), cam, sc.samples_of(40, 8), 1e-12)
    assert res['count'] == 40 and np.abs(res['d']).max() < 1e-18


def test_a_reflection_is_not_fitted():
    p1, p2, s, R, t = known_model()
    S, s_fit, ok, _ = sm.fit(p1, p2 * np.array([1., 1., -1.]))
    assert ok and abs(np.linalg.det(S[:3, :3] / s_fit) - 1.) < 1e-12 and s_fit < s           # a proper rotation, d = -1 in the scale


def test_fixed_scale_returns_one_exactly():
    p1, p2, s, R, t = known_model()
    S, s_fit, ok, _ = sm.fit(p1, p2, fixed_scale=True)
    assert ok and s_fit == 1.0 and np.abs(S[:3, :3] - R).max() <= 1e-12                      # the rotation does not depend on the scale
    assert np.abs(S[:3, :3] @ S[:3, :3].T - np.identity(3)).max() <= 1e-12
    p1, p2 = sc.scene(192)[:2]
    res = sm.ransac(p1, p2, None, None, None, sc.samples_of(192, 64), sc.THRESH_METRIC, fixed_scale=True)
    assert (res['scales'][~res['flags']] == 1.0).all() and res['scale'] == 1.0


def test_degenerate_fits_are_flagged():
    line = np.outer([0., 1., 2.5], [0.3, -0.2, 0.5]) + np.array([1., 2., 6.])
    other = np.array([[0., 0., 5.], [1., 0., 6.], [0., 1., 7.]])
    for a, b in ((line, other), (other, line), (other[[0, 0, 1]], other[[0, 0, 1]]), (other[[1, 1, 1]], other[[1, 1, 1]]),
                 (other[:2], other[:2])):
        S, s, ok, _ = sm.fit(a, b)
        assert not ok and s == 0. and not S.any()
    bad = other.copy()
    bad[1, 2] = np.nan
    assert not sm.fit(bad, other)[2] and not sm.fit(other, bad)[2]
    assert not sm.fit(np.full((3, 3), np.inf), other)[2] and not sm.fit(other, np.full((3, 3), np.inf))[2]
    assert sm.fit(other, other)[2]
    # through ransac(): flagged hypotheses lose, and a table of nothing else gives a degenerate result
    p1, p2, o1, o2 = (x.copy() for x in sc.scene(192)[:4])
    p1[10:13] = line
    p2[20, 1] = np.nan
    samples = np.array([[4, 4, 5], [10, 11, 12], [20, 6, 7], [7, 7, 7], [100, 134, 170]], dtype=np.int32)
    ref = sm.ransac(p1, p2, o1, o2, sc.CAM, samples, sc.THRESH_PIXEL)
    assert ref['flags'].tolist() == [True, True, True, True, False] and ref['best'] == 4 and not ref['mask'][20]
    assert not ref['counts'][:4].any() and not ref['S_all'][:4].any() and np.isinf(ref['d_all'][:4]).all()
    only = sm.ransac(p1, p2, o1, o2, sc.CAM, samples[:4], sc.THRESH_PIXEL)
    assert only['degenerate'] and only['best'] == 0 and only['count'] == 0 and only['reason'] == sm.DEGENERATE and only['rounds'] == 0
    assert not only['S_21'].any() and only['scale'] == 0. and not only['mask'].any() and np.isinf(only['d']).all()


def test_the_scoring_rules():
    p1, p2, s, R, t = known_model()
    S = sm.fit(p1, p2)[0]
    o1, o2 = sc.project(p1), sc.project(p2)
    e, front = sm.errors(S, p1, p2, o1, o2, sc.CAM)
    assert front.all() and e.max() < 1e-18
    # the error is the larger of the two images'
    o2b = o2.copy()
    o2b[3] += [3., 4.]
    o1b = o1.copy()
    o1b[5] += [0., 2.]
    e, _ = sm.errors(S, p1, p2, o1b, o2b, sc.CAM)
    assert abs(e[3] - 25.) < 1e-9 and abs(e[5] - 4.) < 1e-9
    # b is R^T (p_2 - t) / s
    B = S[:3, :3].T / ((S[:3, :3] ** 2).sum() / 3.)
    assert np.abs((p2 @ B.T - B @ S[:3, 3]) - p1).max() < 1e-12
    # behind either camera, or not a number: never an inlier, the others unaffected
    q1, q2 = p1.copy(), p2.copy()
    q1[7] = -q1[7]
    q2[9, 0] = np.nan
    mask, e = sm.score(S, q1, q2, o1, o2, sc.CAM, np.inf)
    assert not mask[7] and not mask[9] and np.isnan(e[9]) and mask.sum() == 38
    mask, e = sm.score(S, q1, q2, None, None, None, np.inf)
    assert mask[7] and not mask[9] and mask.sum() == 39                                     # the metric mode has no depth rule


def test_the_refit_rules():
    for (n, h), row in sc.TABLE.items():
        samples, ref = sc.oracle(n, h)
        assert (ref['raw_count'], ref['count'], ref['rounds'], ref['reason']) == row['refit']
        _, raw = sc.oracle(n, h, 'pixel', 0)
        assert raw['rounds'] == 0 and raw['reason'] == sm.EXHAUSTED and raw['count'] == raw['raw_count'] == ref['raw_count']
        assert np.array_equal(raw['S_21'], raw['S_all'][raw['best']]) and not raw['d_rounds']
    # a lower count is discarded: the raw model comes back bit for bit
    samples, ref = sc.oracle(67, 64, 'metric')
    assert ref['reason'] == sm.LOWER_COUNT and ref['rounds'] == 0 and np.array_equal(ref['S_21'], ref['S_raw']) and len(ref['d_rounds']) == 1
    # one round only: adopted, not yet a fixed point
    _, one = sc.oracle(257, 64, 'pixel', 1)
    assert (one['raw_count'], one['count'], one['rounds'], one['reason']) == (177, 180, 1, sm.EXHAUSTED)
    # an infinite threshold and one hypothesis: plain Umeyama alignment of everything
    p1, p2 = sc.scene(67, 'metric', outlier_fraction=0.)[:2]
    res = sm.ransac(p1, p2, None, None, None, np.array([[0, 33, 66]]), np.inf, refit_iters=1)
    S_all, s_all, ok, _ = sm.fit(p1, p2)
    assert res['count'] == 67 and res['rounds'] == 1 and res['reason'] == sm.FIXED_POINT and np.array_equal(res['S_21'], S_all)


def test_transform_map_and_its_inverse():
    p1, p2, s, R, t = known_model()
    T = SE3.from_matrix(np.block([[R, t[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]), normalize=True)
    poses = [SE3.exp(0.1 * np.random.default_rng(k).standard_normal(6)) for k in range(5)]
    pts, moved = sim3.transform_map(s, T, p1, poses)
    assert np.abs(pts - p2).max() <= 1e-12 and len(moved) == 5 and isinstance(moved[0], SE3)
    # every projection stays what it was: the camera frames scale with the map
    for P, Q in zip(poses, moved):
        a, b = p1 @ P.as_matrix()[:3, :3].T + P.as_matrix()[:3, 3], pts @ Q.as_matrix()[:3, :3].T + Q.as_matrix()[:3, 3]
        assert np.abs(b - s * a).max() <= 1e-12
    s_inv, T_inv = sim3.invert(s, T)
    back_pts, back = sim3.transform_map(s_inv, T_inv, pts, moved)
    err = max(np.abs(back_pts - p1).max(), max(np.abs(a.as_matrix() - b.as_matrix()).max() for a, b in zip(back, poses)))
    print('transform_map and its inverse: max error {:.2e}'.format(err))
    assert err <= 1e-12
    arr = np.stack([P.as_matrix() for P in poses])
    only_pts, none = sim3.transform_map(s, T, points=p1)
    none2, as_arr = sim3.transform_map(s, T.as_matrix(), poses_cw=arr)
    assert none is None and none2 is None and np.array_equal(only_pts, pts) and as_arr.shape == (5, 4, 4)
    assert max(np.abs(a - b.as_matrix()).max() for a, b in zip(as_arr, moved)) <= 1e-12


def test_align_trajectories_of_a_scaled_moved_copy():
    """The device call is stood in for by the restatement here (the device path itself: tests/test_gpu_sim3.py)."""
    from pyslam_amd import _native as nat
    rng = np.random.default_rng(2)
    s, T = 3.2, SE3.exp(np.array([1., -2., 0.5, 0.4, -0.2, 0.9]))
    est = [SE3.exp(np.array([0.3 * k, 0.1 * np.sin(k), 0.05 * k * k, 0.02 * k, -0.01 * k, 0.03 * k]) + 0.01 * rng.standard_normal(6)) for k in range(9)]
    _, gt = sim3.transform_map(s, T, poses_cw=est)

    def stand_in(self, idx):
        r = sm.ransac(self.pts_1, self.pts_2, None, None, None, idx, self.ransac_thresh, refit_iters=self.refit_iters)
        n = self.num_pts
        assert idx.tolist() == [[0, n // 2, n - 1]] and self.ransac_thresh == np.inf and self.refit_iters == 1 and self.camera is None
        return r
    real, real_run = nat.require_gpu, sim3.Sim3RANSAC._device_ransac
    nat.require_gpu, sim3.Sim3RANSAC._device_ransac = (lambda: None), stand_in
    try:
        s_fit, T_fit = sim3.align_trajectories(est, gt, convention='Tvw')
        err = max(abs(s_fit - s), np.abs(T_fit.as_matrix() - T.as_matrix()).max())
        print('align_trajectories of a scaled, moved copy: max error {:.2e}'.format(err))
        assert err <= 1e-12
        # 'Twv': the poses' own translations are the centres
        inv_est, inv_gt = [P.inv() for P in est], [P.inv() for P in gt]
        s_fit, T_fit = sim3.align_trajectories(inv_est, inv_gt)
        assert max(abs(s_fit - s), np.abs(T_fit.as_matrix() - T.as_matrix()).max()) <= 1e-12
        with pytest.raises(ValueError, match='at least 3 poses'):
            sim3.align_trajectories(est[:2], gt[:2])
        with pytest.raises(ValueError, match='convention'):
            sim3.align_trajectories(est, gt, convention='Tcw')
        line = [SE3.exp(np.array([0.1 * k, 0., 0., 0., 0., 0.])) for k in range(5)]
        with pytest.raises(ValueError, match='do not determine a similarity'):
            sim3.align_trajectories(line, line)
    finally:
        nat.require_gpu, sim3.Sim3RANSAC._device_ransac = real, real_run


def test_the_draws_of_draw_samples():
    rs = sim3.Sim3RANSAC()
    p1, p2 = sc.scene(192)[:2]
    rs.set_obs(p1, p2)
    calls = []
    real = np.random.randint

    def counted(*a, **k):
        calls.append(a)
        return real(*a, **k)
    np.random.randint = counted
    try:
        rs.ransac_iters = 16
        seed = next(s for s in range(50) if not _repeats(np.random.RandomState(s).randint(0, 192, (16, 3))).any())
        np.random.seed(seed)
        s = rs.draw_samples()
        assert len(calls) == 1 and calls[0] == (0, 192, (16, 3))                  # no row repeats: the one table
        assert s.shape == (16, 3) and s.dtype == np.int32 and not _repeats(s).any()
        assert np.array_equal(s, np.random.RandomState(seed).randint(0, 192, (16, 3)))
        del calls[:]
        rs.ransac_iters = 400
        rs.set_obs(p1[:4], p2[:4])                                                # four points: most rows repeat
        np.random.seed(1)
        s = rs.draw_samples()
        assert len(calls) > 1 and s.shape == (400, 3) and not _repeats(s).any() and s.min() >= 0 and s.max() <= 3
        assert np.array_equal(s, sc.draw_samples(4, 400, 1))
    finally:
        np.random.randint = real
    rs.set_obs(p1, p2)
    np.random.seed(sc.RANSAC_SEED)
    assert np.array_equal(rs.draw_samples(), sc.draw_samples())
    rs.set_obs(p1[:2], p2[:2])
    with pytest.raises(ValueError, match='at least 3 points'):
        rs.draw_samples()


def _repeats(s):
    return (s[:, 0] == s[:, 1]) | (s[:, 0] == s[:, 2]) | (s[:, 1] == s[:, 2])


def test_the_c_abi_of_the_new_exports():
    from pyslam_amd import _native as nat
    names = ('ps_sim3_hypotheses', 'ps_sim3_ransac', 'ps_sim3_score')
    header = open(os.path.join(REPO, 'include', 'pyslam_hip.h')).read()
    src = open(os.path.join(REPO, 'pyslam_amd', 'csrc', 'ps_abi_sim3.h')).read()
    for name in names:
        decl = re.search(r'\bint ' + name + r'\((.*?)\);', header, re.S).group(1)
        defn = re.search(r'\nint ' + name + r'\((.*?)\) \{', src, re.S).group(1)
        assert name in nat.SIGNATURES, name
        assert len(decl.split(',')) == len(defn.split(',')) == len(nat.SIGNATURES[name][1]), name
        assert re.sub(r'\s+', ' ', decl) == re.sub(r'\s+', ' ', defn), name
    assert (len(nat.SIGNATURES['ps_sim3_hypotheses'][1]), len(nat.SIGNATURES['ps_sim3_score'][1]), len(nat.SIGNATURES['ps_sim3_ransac'][1])) == (14, 11, 16)
    core = open(os.path.join(REPO, 'pyslam_amd', 'csrc', 'ps_core.hip')).read()
    assert core.index('#include "ps_k_pnp.h"') < core.index('#include "ps_k_sim3.h"')
    assert core.index('#include "ps_abi_pnp.h"') < core.index('#include "ps_abi_sim3.h"')
    import __graft_entry__ as g
    assert {'ps_k_sim3.h', 'ps_abi_sim3.h'} <= set(os.listdir(os.path.dirname(g.SRC)))      # the build hash covers every file of csrc/
    kern = open(os.path.join(REPO, 'pyslam_amd', 'csrc', 'ps_k_sim3.h')).read()
    assert re.search(r'atomic\w*\s*\(', kern, re.I) is None     # no atomic call: every sum in a fixed order
    for k in ('k_sim3_hypotheses', 'k_sim3_refit'):           # the mode is a template parameter of the kernels that score
        assert re.search(r'template <bool PIXEL> __global__ __launch_bounds__\(256\) void ' + k + r'\(', kern), k
    assert re.search(r'\n__global__ __launch_bounds__\(256\) void k_sim3_best\(', kern)
    for call in ('rc_first_max(', 'rc_block_sum(', 'rc_block_partials(', 'rc_jacobi3<false>(', 'rc_sort3('):
        assert call in kern, call
    for call in ('rc_hypotheses_call(', 'rc_score_call(', 'rc_upload(', 'rc_download(', 'rc_check_samples(', 'rc_check_camera('):
        assert call in src, call
    assert 'ps_sim3_ransac' in open(os.path.join(REPO, 'INTEGRATION.md')).read()


def test_errors_and_imports():
    import pyslam.pipelines.sim3 as shim
    from pyslam_amd import _native as nat
    from pyslam_amd.sensors import MonoCamera
    assert shim.Sim3RANSAC is sim3.Sim3RANSAC and shim.align_maps is sim3.align_maps and shim.align_trajectories is sim3.align_trajectories
    assert shim.transform_map is sim3.transform_map
    cam = MonoCamera(*synthetic.TWO_VIEW_CAMERA)
    rs = sim3.Sim3RANSAC(cam)
    assert (rs.ransac_iters, rs.ransac_thresh, rs.num_min_set_pts, rs.min_inliers, rs.refit_iters, rs.fixed_scale) == (400, 9.0, 3, 12, 3, False)
    metric = sim3.Sim3RANSAC()
    assert metric.camera is None and metric.ransac_thresh is None
    p1, p2, o1, o2 = sc.scene(192)[:4]
    with pytest.raises(ValueError, match='same number of points'):
        rs.set_obs(p1, p2[:100])
    with pytest.raises(ValueError, match=r'pts_1 must have shape \(N, 3\)'):
        rs.set_obs(p1[:, :2], p2)
    with pytest.raises(ValueError, match=r'shape \(N, 2\) or \(N, 3\)'):
        rs.set_obs(p1, p2, o1.T, o2)
    with pytest.raises(ValueError, match='one row per point'):
        rs.set_obs(p1, p2, o1[:5], o2)
    with pytest.raises(ValueError, match='need a camera'):
        metric.set_obs(p1, p2, o1, o2)
    rs.set_obs(p1, p2)                                         # no observations: the points' own projections
    assert np.array_equal(rs.obs_1, sc.project(p1)) and np.array_equal(rs.obs_2, sc.project(p2)) and rs.num_pts == 192
    rs.set_obs(p1, p2, np.concatenate([o1, np.ones((192, 1))], axis=1), o2)      # a third column is ignored
    assert np.array_equal(rs.obs_1, o1) and np.array_equal(rs.obs_2, o2)
    with pytest.raises(ValueError, match=r'shape \(H, 3\)'):
        rs._samples(np.zeros((4, 8), dtype=np.int32))
    metric.set_obs(p1, p2)
    with pytest.raises(ValueError, match='ransac_thresh'):
        metric.perform_ransac()
    rs.set_obs(p1[:2], p2[:2])
    with pytest.raises(ValueError, match='at least 3 correspondences'):
        rs.perform_ransac()
    rs.set_obs(p1, p2, o1, o2)
    rs.num_min_set_pts = 4
    with pytest.raises(ValueError, match='three pairs'):
        rs.perform_ransac()
    rs.num_min_set_pts = 3
    # too few inliers: the device's answer stands in here (the device path itself: tests/test_gpu_sim3.py)
    S = np.identity(4)
    S[:3, :3] *= 2.
    few = dict(S_21=S, scale=2., mask=np.arange(192) < 9, best=0, raw_count=9, count=9, rounds=0, reason=0, degenerate=False, d=np.zeros(192))
    rs._device_ransac = lambda idx: few
    real = nat.require_gpu
    nat.require_gpu = lambda: None
    try:
        with pytest.raises(ValueError, match='failed to find 12 inliers'):
            rs.perform_ransac()
        with pytest.raises(ValueError, match='failed to find 12 inliers'):
            sim3.align_maps(cam, p1, p2, o1, o2, seed=1, ransac=rs)
        rs.min_inliers = 9
        scale, T_21, inliers = sim3.align_maps(cam, p1, p2, o1, o2, seed=1, ransac=rs)
        assert scale == 2. and inliers.tolist() == list(range(9)) and np.array_equal(T_21.as_matrix(), np.identity(4))
    finally:
        nat.require_gpu = real


# ---- the conditions tests/test_gpu_sim3.py relies on, for every committed seed and shape (tests/sim3_scenes.py) -------------------

def check_conditions(name, ref, thresh):
    c = sc.conditions(ref, thresh)
    print('{}: pairs in the margin {} of {} (winner, refit rounds, final model: {}), hypotheses below the ratio limit {:.2%} (smallest '
          'sigma_b / sigma_a {:.2e}), tied at the maximum {}, degenerate {}'.format(name, c['near'], c['pairs'], c['near_final'], c['loose'],
                                                                                   c['min_ratio'], c['ties'], int(ref['flags'].sum())))
    assert c['near'] == 0 and c['near_final'] == 0            # margin condition: every pair, every refit round
    assert c['loose'] <= sc.RATIO_CAP                         # ratio cap
    assert ref['best'] == int(np.argmax(ref['counts']))       # the first maximum
    return c


def test_committed_shapes_meet_the_conditions():
    assert sc.SHAPES == [(192, 256), (67, 64), (257, 64)] and (sc.THRESH_PIXEL, sc.THRESH_METRIC) == (9.0, 0.25)
    for n, h in sc.SHAPES:
        row = sc.TABLE[(n, h)]
        for mode in sc.MODES:
            thresh = sc.call_args(mode)[1]
            for iters in (3, 0):
                samples, ref = sc.oracle(n, h, mode, iters)
                assert samples.shape == (h, 3) and not ref['flags'].any() and ref['raw_count'] >= 12
                c = check_conditions('N = {}, H = {}, {} mode, refit_iters {}'.format(n, h, mode, iters), ref, thresh)
                assert c['loose'] == 0.                        # on the committed shapes nothing is left out
                assert c['ties'] == {'pixel': row['ties'], 'metric': row['metric_ties'], 'fixed': row['fixed_ties']}[mode]
        # the issue's table
        _, ref = sc.oracle(n, h)
        outlier = sc.scene(n)[6]
        assert ref['counts'].max() == row['best'] and (ref['raw_count'], ref['count'], ref['rounds'], ref['reason']) == row['refit']
        if n != 257:
            assert row['best'] == (~outlier).sum() and np.array_equal(ref['mask'], ~outlier)
    mins = [float(sc.oracle(n, h)[1]['ratio'].min()) for n, h in sc.SHAPES]
    assert [float('{:.1e}'.format(m)) for m in mins] == [4.4e-3, 3.6e-4, 4.0e-3]
    for mode in sc.MODES:
        samples, ref = sc.seeded_oracle(mode)
        assert samples.shape == (400, 3) and not ref['flags'].any()
        check_conditions('perform_ransac with seed {}, {} mode'.format(sc.RANSAC_SEED, mode), ref, sc.call_args(mode)[1])


def test_more_depth_noise_is_why_the_default_is_small():
    p1, p2, o1, o2, s, T, outlier = sc.scene(192, point_noise=0.02)
    ref = sm.ransac(p1, p2, o1, o2, sc.CAM, sc.samples_of(192, 256), sc.THRESH_PIXEL, refit_iters=0)
    print('point_noise 0.02: the winner finds {} of {}'.format(ref['raw_count'], (~outlier).sum()))
    assert (ref['raw_count'], int((~outlier).sum())) == (81, 135)


def test_the_edge_scenes_meet_the_conditions():
    for n in sc.EDGE_SIZES:
        scn, samples = sc.edge_scene(n)
        for mode in ('pixel', 'metric'):
            ref = sc.run(scn, mode, samples)
            c = check_conditions('edge N = {}, {} mode'.format(n, mode), ref, sc.call_args(mode)[1])
            assert ref['count'] >= 3 or n < 4


def test_end_to_end_host_figures():
    """The figures tests/test_gpu_sim3.py holds the device chains against (twice these), recorded in sim3_scenes."""
    ref = sc.host_boot()
    fig = sc.boot_figures(ref['scale'], ref['S_21'])
    print('bootstrap -> alignment with the true points: scale {:.6f}, {} of {} inliers, refit rounds {} ({}); against the truth: '
          'scale {:.3e}, rotation {:.3e} rad, translation {:.3e}'.format(ref['scale'], ref['count'], ref['mask'].size, ref['rounds'],
                                                                          sim3.REASONS[ref['reason']], fig['scale'], fig['rot'], fig['t']))
    check_conditions('bootstrap alignment', ref, sc.THRESH_PIXEL)
    for k, v in fig.items():
        assert 0.98 * sc.BOOT_HOST[k] <= v <= sc.BOOT_HOST[k], k
    est, gt, ref = sc.host_traj()
    centre = sc.traj_figures(ref['S_21'], est, gt)
    print('{} keyframes aligned with the truth: scale {:.6f}, sigma_b / sigma_a {:.2e}, largest centre error {:.3e} m'.format(
        est.shape[0], ref['scale'], float(ref['ratio'][0]), centre))
    assert ref['count'] == est.shape[0] >= 3 and ref['rounds'] == 1 and ref['reason'] == sm.FIXED_POINT
    assert 0.98 * sc.TRAJ_HOST['centre'] <= centre <= sc.TRAJ_HOST['centre']
