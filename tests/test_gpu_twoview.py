"""Monocular two-view initialisation on the device (csrc/ps_k_twoview.h, pyslam_amd/pipelines/twoview.py) against the numpy
restatement (pyslam_amd/pipelines/epipolar.py), the truth of the synthetic scene, and through bootstrap into monocular bundle
adjustment.  Run with `-m gpu` on an MI355X.  Every comparison prints its figure before it asserts.

The margin rule: a (hypothesis, point) pair whose restated squared Sampson distance lies within 1e-6 relative of the threshold may
fall on either side of it (the matrices agree to 1e-9, not to the bit); such pairs are left out of the comparison of masks and
counts, and the tests bound how many there may be."""
import numpy as np
import pytest

from pyslam_amd import synthetic, triangulation
from pyslam_amd.liegroups import SO3
from pyslam_amd.pipelines import epipolar as ep
from pyslam_amd.pipelines import twoview
from pyslam_amd.sensors import MonoCamera

pytestmark = pytest.mark.gpu

THRESH = 4.0
TOL_E = 1e-9           # relative Frobenius, device E against the restatement's (the issue's bound)
TOL_POSE = 1e-9        # rotation (rad) and translation direction, device against restatement (the issue's bound)
MARGIN = 1e-6


def camera():
    return MonoCamera(*synthetic.TWO_VIEW_CAMERA)


def samples_of(n, h, seed=5):
    rs = np.random.RandomState(seed)
    return np.stack([rs.choice(n, 8, replace=False) for _ in range(h)]).astype(np.int32)


def rel_fro(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def rot_angle(Ra, Rb):
    return np.linalg.norm(SO3.from_matrix(Ra @ Rb.T, normalize=True).log())


def dir_angle(a, b):
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)


def in_margin(d):
    return np.abs(d - THRESH) <= MARGIN * THRESH


def solver(obs_1, obs_2, **attrs):
    rs = twoview.EssentialRANSAC(camera())
    for k, v in attrs.items():
        setattr(rs, k, v)
    rs.set_obs(obs_1, obs_2)
    return rs


def compare_hypotheses(obs_1, obs_2, samples, max_left_out):
    """Device E, counts and flags of every sample against the restatement; -> (device E, counts, restatement tuple)."""
    cam = camera().intrinsics()
    rs = solver(obs_1, obs_2)
    E, counts, flags = rs._device_hypotheses(samples)
    E_ref, counts_ref, deg_ref, dist = ep.hypotheses(obs_1, obs_2, cam, samples, THRESH)
    assert np.array_equal(flags, deg_ref)
    assert np.isfinite(E).all()
    worst = max([rel_fro(E[h], E_ref[h]) for h in range(len(samples)) if not deg_ref[h]] + [0.])
    near = in_margin(dist)
    print('N = {}, H = {}: E device vs restatement max {:.2e}; pairs in the margin {} of {}'.format(
        obs_1.shape[0], len(samples), worst, near.sum(), near.size))
    assert worst <= TOL_E
    assert near.sum() <= max_left_out
    masks = rs.compute_ransac_cost(E, obs_1, obs_2, rs.camera, THRESH)
    want = dist < THRESH
    assert np.array_equal(masks[~near], want[~near])                      # compute_ransac_cost against the restatement's masks
    lo, hi = (want & ~near).sum(axis=1), (want | near).sum(axis=1)
    assert ((counts >= lo) & (counts <= hi)).all()                        # equal counts once the margin pairs are left out
    assert np.array_equal(counts, masks.sum(axis=1))
    assert (counts[deg_ref] == 0).all() and not E[deg_ref].any()
    return E, counts, (E_ref, counts_ref, deg_ref, dist)


@pytest.fixture(scope='module')
def scene():
    obs_1, obs_2, T, outlier = synthetic.two_view()
    return obs_1, obs_2, T, outlier


@pytest.fixture(scope='module')
def seeded(scene):
    """perform_ransac with np.random.seed(5) on the device, and the restatement on the same samples (computed once)."""
    obs_1, obs_2, T, outlier = scene
    rs = solver(obs_1, obs_2)
    np.random.seed(5)
    samples = rs.draw_samples()
    np.random.seed(5)
    out = rs.perform_ransac()
    ref = ep.ransac(obs_1, obs_2, camera().intrinsics(), samples, THRESH)
    return rs, out, ref, samples


def test_hypotheses_equal_the_restatement(scene):
    obs_1, obs_2, T, outlier = scene
    samples = samples_of(192, 256)
    sig = [ep.eight_point(ep.normalise(obs_1, camera().intrinsics()), ep.normalise(obs_2, camera().intrinsics()), s)[2] for s in samples]
    print('worst sample: sigma_8 / sigma_1 = {:.2e}'.format(min(s[7] / s[0] for s in sig)))       # this generator's scene: 3.2e-5
    E, counts, ref = compare_hypotheses(obs_1, obs_2, samples, max_left_out=int(0.001 * 256 * 192))
    assert not ref[2].any()                                                # no hypothesis excluded
    assert counts.max() >= 0.8 * (~outlier).sum()


def test_perform_ransac_equals_the_restatement(scene, seeded):
    obs_1, obs_2, T, outlier = scene
    rs, (T_21, in_1, in_2, inliers), ref, samples = seeded
    info = rs.info_
    print('device: best {} raw {} final {} refit kept {} cheirality {}; restatement: best {} raw {} final {} kept {} cheirality {}'.format(
        info['best'], info['raw_count'], info['count'], info['refit_kept'], info['cheirality_counts'].tolist(),
        ref['best'], ref['raw_count'], ref['count'], ref['refit_kept'], ref['cheirality_counts'].tolist()))
    assert info['best'] == ref['best'] and info['refit_kept'] == ref['refit_kept']
    near = in_margin(ref['d'])
    got = np.zeros(192, dtype=bool)
    got[inliers] = True
    assert near.sum() <= 1 and np.array_equal(got[~near], ref['mask'][~near])
    assert np.array_equal(in_1, obs_1[inliers]) and np.array_equal(in_2, obs_2[inliers])
    Tm = T_21.as_matrix()
    e_rot, e_dir = rot_angle(Tm[:3, :3], ref['T_21'][:3, :3]), dir_angle(Tm[:3, 3], ref['T_21'][:3, 3])
    print('T_21 device vs restatement: rotation {:.2e} rad, translation direction {:.2e}; E {:.2e}'.format(
        e_rot, e_dir, rel_fro(rs.E_, ref['E'])))
    assert e_rot <= TOL_POSE and e_dir <= TOL_POSE
    assert abs(np.linalg.norm(Tm[:3, 3]) - 1.) <= 1e-12
    # against the truth: no worse than 1.5 x the restatement's own errors on this scene
    r_dev, d_dev = rot_angle(Tm[:3, :3], T[:3, :3]), dir_angle(Tm[:3, 3], T[:3, 3])
    r_ref, d_ref = rot_angle(ref['T_21'][:3, :3], T[:3, :3]), dir_angle(ref['T_21'][:3, 3], T[:3, 3])
    print('against the truth: device rotation {:.3e} direction {:.3e}; restatement {:.3e} / {:.3e}'.format(r_dev, d_dev, r_ref, d_ref))
    assert r_dev <= 1.5 * r_ref and d_dev <= 1.5 * d_ref
    kept = (got & ~outlier).sum()
    print('true inliers in the winner: {} of {}'.format(kept, (~outlier).sum()))
    assert kept >= 0.8 * (~outlier).sum()
    assert np.array_equal(info['cheirality_counts'], ref['cheirality_counts'])
    assert np.abs(rs.parallax_deg_ - ref['parallax_deg']).max() <= 1e-6 if not near.any() else True


def test_eight_exact_points_give_the_exact_pose():
    obs_1, obs_2, T, _ = synthetic.two_view(num_pts=8, pixel_noise=0., outlier_fraction=0.)
    cam = camera().intrinsics()
    x1, x2 = ep.normalise(obs_1, cam), ep.normalise(obs_2, cam)
    sigma = ep.eight_point(x1, x2, np.arange(8))[2]
    cond = sigma[0] / sigma[7]
    # the elimination works on A itself: error ~ eps cond(A); the refit over these same 8 points goes through the moment
    # matrix, which squares it (the refit is meant for many noisy inliers, where it averages; here it only must not break)
    for refit, tol in ((False, 100 * 2.2e-16 * cond), (True, 100 * 2.2e-16 * cond * cond)):
        rs = solver(obs_1, obs_2, ransac_iters=1, min_inliers=8, refit=refit)
        np.random.seed(0)
        T_21, in_1, in_2, inliers = rs.perform_ransac()
        Tm = T_21.as_matrix()
        e_rot, e_dir = rot_angle(Tm[:3, :3], T[:3, :3]), dir_angle(Tm[:3, 3], T[:3, 3])
        print('8 exact points, refit {}: cond {:.2e}, rotation {:.2e} rad, direction {:.2e} (bound {:.2e})'.format(refit, cond, e_rot, e_dir, tol))
        assert inliers.tolist() == list(range(8))
        assert e_rot <= tol and e_dir <= tol


def compare_ransac(obs_1, obs_2, samples, max_left_out):
    """_device_ransac with and without the refit against the restatement on the same samples; at most `max_left_out` points of the
    winner may lie in the margin, and everything is compared when none does."""
    n = obs_1.shape[0]
    for refit in (True, False):
        rs = solver(obs_1, obs_2, refit=refit)
        res = rs._device_ransac(samples)
        ref = ep.ransac(obs_1, obs_2, camera().intrinsics(), samples, THRESH, refit_winner=refit)
        near = in_margin(ref['d']) | in_margin(ref['d_raw']) | (in_margin(ref['d_refit']) if ref['d_refit'] is not None else False)
        print('N = {}, H = {}, refit {}: device count {} kept {}, restatement {} kept {}, margin {}'.format(
            n, len(samples), refit, res['count'], res['refit_kept'], ref['count'], ref['refit_kept'], np.sum(near)))
        assert np.sum(near) <= max_left_out
        if not np.any(near):
            assert res['best'] == ref['best'] and res['refit_kept'] == ref['refit_kept'] and np.array_equal(res['mask'], ref['mask'])
            assert rel_fro(res['E'], ref['E']) <= TOL_E
            assert rot_angle(res['T_21'][:3, :3], ref['T_21'][:3, :3]) <= TOL_POSE
            assert dir_angle(res['T_21'][:3, 3], ref['T_21'][:3, 3]) <= TOL_POSE
            assert np.array_equal(res['cheirality_counts'], ref['cheirality_counts'])


@pytest.mark.parametrize('n', [67, 257])
def test_sizes_off_the_workgroup(n):
    obs_1, obs_2, T, outlier = synthetic.two_view(num_pts=n)
    samples = samples_of(n, 64)
    compare_hypotheses(obs_1, obs_2, samples, max_left_out=int(0.001 * 64 * n))
    compare_ransac(obs_1, obs_2, samples, max_left_out=1)


def test_a_single_hypothesis(scene):
    obs_1, obs_2, T, outlier = scene
    samples = samples_of(192, 256)[143:144]
    compare_hypotheses(obs_1, obs_2, samples, max_left_out=0)
    res = solver(obs_1, obs_2)._device_ransac(samples)
    ref = ep.ransac(obs_1, obs_2, camera().intrinsics(), samples, THRESH)
    assert res['best'] == 0 and res['raw_count'] == ref['raw_count'] and res['count'] == ref['count']
    assert np.array_equal(res['mask'], ref['mask']) and rel_fro(res['E'], ref['E']) <= TOL_E


def test_a_repeated_index_is_flagged_and_loses(scene):
    obs_1, obs_2, T, outlier = scene
    samples = samples_of(192, 2)
    samples[0, 6] = samples[0, 2]
    rs = solver(obs_1, obs_2)
    E, counts, flags = rs._device_hypotheses(samples)
    assert flags.tolist() == [True, False] and counts[0] == 0 and not E[0].any() and counts[1] > 0
    res = rs._device_ransac(samples)
    assert res['best'] == 1 and res['raw_count'] == counts[1]
    for key in ('T_21', 'E', 'parallax_deg'):
        assert np.isfinite(res[key]).all(), key
    # only degenerate rows: nothing wins, nothing is NaN, and the host refuses
    both = np.stack([samples[0], samples[0]])
    res = rs._device_ransac(both)
    assert res['count'] == 0 and not res['mask'].any() and np.isfinite(res['T_21']).all() and np.isfinite(res['E']).all()


def test_all_outliers_raise():
    obs_1, obs_2, T, outlier = synthetic.two_view(outlier_fraction=1.0)
    assert outlier.all()
    rs = solver(obs_1, obs_2)
    np.random.seed(5)
    with pytest.raises(ValueError, match='failed to find 16 inliers'):
        rs.perform_ransac()
    assert rs.info_['count'] < 16


def test_without_the_refit_the_raw_hypothesis_comes_back_bit_for_bit(scene, seeded):
    obs_1, obs_2, T, outlier = scene
    _, _, _, samples = seeded
    rs = solver(obs_1, obs_2, refit=False)
    res = rs._device_ransac(samples)
    E, counts, flags = rs._device_hypotheses(samples)
    best = int(np.argmax(counts))
    assert res['best'] == best and res['raw_count'] == res['count'] == counts[best] and not res['refit_kept']
    assert np.array_equal(res['E'], E[best])
    assert np.array_equal(res['mask'], rs.compute_ransac_cost(E[best], obs_1, obs_2, rs.camera, THRESH)[0])


def test_two_calls_are_bit_identical(scene, seeded):
    obs_1, obs_2, T, outlier = scene
    _, _, _, samples = seeded
    rs = solver(obs_1, obs_2)
    a, b = rs._device_ransac(samples), rs._device_ransac(samples)
    for key in ('T_21', 'E', 'mask', 'cheirality_counts', 'parallax_deg'):
        assert np.array_equal(a[key], b[key]), key
    assert (a['best'], a['raw_count'], a['count'], a['refit_kept']) == (b['best'], b['raw_count'], b['count'], b['refit_kept'])
    ha, hb = rs._device_hypotheses(samples), rs._device_hypotheses(samples)
    assert all(np.array_equal(x, y) for x, y in zip(ha, hb))


@pytest.fixture(scope='module')
def booted(scene):
    obs_1, obs_2, T, outlier = scene
    return twoview.bootstrap(camera(), obs_1, obs_2, min_parallax_deg=1.0, seed=5)


def test_bootstrap_triangulates_the_inliers(scene, booted, seeded):
    obs_1, obs_2, T, outlier = scene
    T_21, points, status, inliers = booted
    _, _, ref, _ = seeded
    assert points.shape == (inliers.size, 3) and status.shape == (inliers.size,)
    ok = status == 0
    print('bootstrap: {} inliers, status counts {}'.format(inliers.size, np.bincount(status, minlength=4).tolist()))
    assert ok.sum() >= 16
    Tm = T_21.as_matrix()
    z1, z2 = points[ok, 2], (points[ok] @ Tm[:3, :3].T + Tm[:3, 3])[:, 2]
    assert (z1 > 0.).all() and (z2 > 0.).all()
    scale = np.linalg.norm(T[:3, 3])
    truth = synthetic.two_view_points()
    err = np.median(np.linalg.norm(scale * points[ok] - truth[inliers[ok]], axis=1))
    # the restatement chain on the same input: epipolar.py, then triangulation.triangulate
    m = ref['mask']
    lp = twoview.two_view_tables(camera(), ref['T_21'], obs_1[m], obs_2[m])
    pts_ref, st_ref = triangulation.triangulate_tables(lp, 5, 1.0)
    err_ref = np.median(np.linalg.norm(scale * pts_ref[st_ref == 0] - truth[np.where(m)[0][st_ref == 0]], axis=1))
    print('median distance to the true points: device {:.4f} m, restatement chain {:.4f} m'.format(err, err_ref))
    assert err <= 1.5 * err_ref


def test_bootstrap_refuses_a_pure_rotation():
    obs_1, obs_2, T, outlier = synthetic.two_view(t=(0., 0., 0.))
    with pytest.raises(ValueError, match='too little parallax'):
        twoview.bootstrap(camera(), obs_1, obs_2, min_parallax_deg=1.0, seed=5)


def test_bootstrap_feeds_monocular_bundle_adjustment(scene, booted):
    obs_1, obs_2, T, outlier = scene
    T_21, points, status, inliers = booted
    from test_host_api import build_namespace
    ns = build_namespace()
    ns.MonoCamera = MonoCamera
    ok = status == 0
    lp = twoview.two_view_tables(camera(), T_21.as_matrix(), obs_1[inliers[ok]], obs_2[inliers[ok]])
    lp.points = points[ok].copy()
    problem = synthetic.to_objects(lp, ns, ns.Options())
    final = problem.solve()
    assert problem._device is not None
    pts = np.stack([final[k] for k in lp.point_keys])
    Tm = T_21.as_matrix()
    cam = camera()
    e1 = np.atleast_2d(cam.project(pts)) - obs_1[inliers[ok]]
    e2 = np.atleast_2d(cam.project(pts @ Tm[:3, :3].T + Tm[:3, 3])) - obs_2[inliers[ok]]
    rms = np.sqrt(np.concatenate([(e1 ** 2).sum(axis=1), (e2 ** 2).sum(axis=1)]).mean())
    hist = problem._cost_history
    print('monocular BA from bootstrap: {} landmarks, cost history {}, reprojection RMS {:.3f} px'.format(ok.sum(), hist, rms))
    # bootstrap's landmarks are already the minimisers for the held poses (five refinement steps of the triangulation), so the
    # solve starts at its optimum and a step moves the cost by rounding only, up as easily as down: a residual is a difference of
    # pixel coordinates up to 640 evaluated to a few ulps (~8 * 2.2e-16 * 640 = 1.1e-12 px) against residuals of ~0.5 px, which
    # is 2 * 1.1e-12 / 0.5 = 4.5e-12 of the cost.  The cost may not rise by more than that.
    assert np.isfinite(hist).all() and hist[-1] <= hist[0] * (1. + 4.5e-12)
    assert rms < 2 * 0.5                                                # 2 x pixel_noise of synthetic.two_view()
