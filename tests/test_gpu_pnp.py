"""Absolute-pose (PnP) registration on the device (csrc/ps_k_pnp.h, pyslam_amd/pipelines/pnp.py) against the restatement
(pyslam_amd/pipelines/absolute.py), the truth of the synthetic scene, and end to end: bootstrap -> register_frame -> monocular
bundle adjustment over three keyframes.  Run with `-m gpu` on an MI355X.  Every comparison prints its figure before it asserts.

What the comparisons rely on is asserted on the host for every seed and shape used here (tests/test_pnp_host.py over
tests/pnp_scenes.py): no (slot, point) pair within 1e-6 relative of the threshold, no branch decision of the minimal solver within
1e-9 relative of its boundary, ties resolved by the first-maximum rule, and at most 5 % of the non-empty slots with a sensitivity
above 1e-10.  So counts and flags are compared without exception; only T_all leaves the sensitive slots out."""
import numpy as np
import pytest

import pnp_scenes as sc
from pyslam_amd import synthetic, triangulation
from pyslam_amd.liegroups import SO3
from pyslam_amd.pipelines import absolute as ab
from pyslam_amd.pipelines import pnp, twoview
from pyslam_amd.sensors import MonoCamera

pytestmark = pytest.mark.gpu

THRESH = sc.THRESH
TOL_T = 1e-9             # max-abs, device T_all against the restatement's, slots with sensitivity <= 1e-10 (the issue's bound)
TOL_POSE = 1e-9          # rotation angle (rad) and translation, device T_cw against the restatement's (the issue's bound)
TOL_COST = 1e-9          # relative, cost history (the issue's bound)


def camera():
    return MonoCamera(*synthetic.TWO_VIEW_CAMERA)


def rot_angle(Ra, Rb):
    return np.linalg.norm(SO3.from_matrix(Ra @ Rb.T, normalize=True).log())


def solver(pts, obs, **attrs):
    rs = pnp.PnPRANSAC(camera())
    for k, v in attrs.items():
        setattr(rs, k, v)
    rs.set_obs(pts, obs)
    return rs


def compare_hypotheses(pts, obs, samples, ref):
    """Device T_all, counts and flags of every sample against the restatement `ref`."""
    rs = solver(pts, obs)
    T, counts, empty, degenerate = rs._device_hypotheses(samples)
    assert np.array_equal(empty, ref['empty']) and np.array_equal(degenerate, ref['degenerate'])
    assert np.isfinite(T).all() and not T[empty].any() and not counts[empty].any()
    diff = np.abs(T - ref['T_all']).reshape(len(samples), 4, 16).max(axis=2)
    tight = ~empty & (ref['sensitivity'] <= sc.SENS_LIMIT)
    loose = ~empty & ~tight
    share = loose.sum() / max(1, (~empty).sum())
    print('N = {}, H = {}: T_all device vs restatement max {:.2e} over {} slots; {} left out ({:.2%}, their max {:.2e}); '
          'counts differing {}'.format(pts.shape[0], len(samples), diff[tight].max() if tight.any() else 0., tight.sum(), loose.sum(),
                                       share, diff[loose].max() if loose.any() else 0., (counts != ref['counts']).sum()))
    assert diff[tight].max() <= TOL_T if tight.any() else True
    assert share <= sc.SENS_CAP
    assert np.array_equal(counts, ref['counts'])                              # nothing is left out of the count comparison
    return rs, T, counts


def compare_ransac(res, ref):
    assert (res['best'], res['best_slot'], res['refine_kept']) == (ref['best'], ref['best_slot'], ref['refine_kept'])
    assert res['raw_count'] == ref['raw_count'] and res['count'] == ref['count'] and np.array_equal(res['mask'], ref['mask'])
    e_rot = rot_angle(res['T_cw'][:3, :3], ref['T_cw'][:3, :3])
    e_t = np.abs(res['T_cw'][:3, 3] - ref['T_cw'][:3, 3]).max()
    # 1e-9 relative, above the floor of a cost that is zero in exact arithmetic (a minimal set explains its own three points): a
    # residual is a difference of pixel coordinates up to 640 evaluated to a few ulps (~8 * 2.2e-16 * 640 = 1.1e-12 px), and the
    # cost is half the sum of 2 n such squares
    assert res['cost_history'].shape == ref['cost_history'].shape
    floor = ref['raw_count'] * 1.1e-12 ** 2
    excess = np.abs(res['cost_history'] - ref['cost_history']) - floor
    e_cost = (excess / ref['cost_history']).max() if (ref['cost_history'] > 0.).all() else (0. if (excess <= 0.).all() else np.inf)
    print('T_cw device vs restatement: rotation {:.2e} rad, translation {:.2e}; cost history {} vs {} (relative, above the floor '
          '{:.1e}: {:.2e})'.format(e_rot, e_t, res['cost_history'].tolist(), ref['cost_history'].tolist(), floor, e_cost))
    assert e_rot <= TOL_POSE and e_t <= TOL_POSE and e_cost <= TOL_COST


@pytest.fixture(scope='module')
def seeded():
    """perform_ransac with np.random.seed(5) on the device; the restatement on the same samples comes from pnp_scenes."""
    pts, obs, T, outlier = sc.scene(192)
    rs = solver(pts, obs)
    np.random.seed(sc.RANSAC_SEED)
    out = rs.perform_ransac()
    samples, ref = sc.seeded_oracle()
    return rs, out, ref, samples


@pytest.mark.parametrize('n,h', sc.SHAPES)
def test_hypotheses_equal_the_restatement(n, h):
    pts, obs, T, outlier = sc.scene(n)
    samples, ref = sc.oracle(n, h)
    rs, T_all, counts = compare_hypotheses(pts, obs, samples, ref)
    # compute_ransac_cost: the masks of the device's own poses against the restatement's masks
    ne = ~ref['empty']
    masks = rs.compute_ransac_cost(T_all[ne], pts, obs, rs.camera, THRESH)
    with np.errstate(invalid='ignore'):
        want = ref['d_all'][ne] < THRESH
    assert masks.shape == want.shape and np.array_equal(masks, want) and np.array_equal(masks.sum(axis=1), counts[ne])
    # the whole chain on the same table, with the refinement and without
    for refine in (True, False):
        res = solver(pts, obs, refine=refine)._device_ransac(samples)
        compare_ransac(res, sc.oracle(n, h, refine)[1])


def test_a_single_hypothesis():
    n, h, row = sc.SINGLE
    pts, obs, _, _ = sc.scene(n)
    samples = sc.samples_of(n, h)[row:row + 1]
    ref = ab.ransac(pts, obs, sc.CAM, samples, THRESH, sensitivity=True)
    rs, T_all, counts = compare_hypotheses(pts, obs, samples, ref)
    res = rs._device_ransac(samples)
    assert res['best'] == 0
    compare_ransac(res, ref)


def test_perform_ransac_equals_the_restatement(seeded):
    pts, obs, T, outlier = sc.scene(192)
    rs, (T_cw, in_pts, in_obs, inliers), ref, samples = seeded
    info = rs.info_
    print('device: best {} slot {} raw {} final {} kept {}; restatement: best {} slot {} raw {} final {} kept {}'.format(
        info['best'], info['best_slot'], info['raw_count'], info['count'], info['refine_kept'],
        ref['best'], ref['best_slot'], ref['raw_count'], ref['count'], ref['refine_kept']))
    compare_ransac(info, ref)
    assert np.array_equal(inliers, np.where(ref['mask'])[0])
    assert np.array_equal(in_pts, pts[inliers]) and np.array_equal(in_obs, obs[inliers])
    assert np.abs(info['d'] - ref['d']).max() <= 1e-6 * THRESH               # every point's squared error (the margin's width)
    # against the truth: no worse than 1.5 x the restatement's own errors on this scene
    Tm = T_cw.as_matrix()
    r_dev, t_dev = rot_angle(Tm[:3, :3], T[:3, :3]), np.linalg.norm(Tm[:3, 3] - T[:3, 3])
    r_ref, t_ref = rot_angle(ref['T_cw'][:3, :3], T[:3, :3]), np.linalg.norm(ref['T_cw'][:3, 3] - T[:3, 3])
    print('against the truth: device rotation {:.3e} translation {:.3e}; restatement {:.3e} / {:.3e}'.format(r_dev, t_dev, r_ref, t_ref))
    assert r_dev <= 1.5 * r_ref and t_dev <= 1.5 * t_ref
    kept = (ref['mask'] & ~outlier).sum()
    got = np.zeros(192, dtype=bool)
    got[inliers] = True
    print('true inliers in the winner: {} of {}'.format((got & ~outlier).sum(), (~outlier).sum()))
    assert (got & ~outlier).sum() >= 0.8 * (~outlier).sum() and kept == (got & ~outlier).sum()


def test_without_the_refinement_the_raw_slot_comes_back_bit_for_bit(seeded):
    pts, obs, _, _ = sc.scene(192)
    _, _, _, samples = seeded
    rs = solver(pts, obs, refine=False)
    res = rs._device_ransac(samples)
    T_all, counts, empty, degenerate = rs._device_hypotheses(samples)
    flat = int(np.argmax(counts.reshape(-1)))
    assert (res['best'], res['best_slot']) == (flat // 4, flat % 4) and not res['refine_kept'] and res['iterations'] == 0
    assert res['raw_count'] == res['count'] == counts.reshape(-1)[flat]
    assert np.array_equal(res['T_cw'], T_all[flat // 4, flat % 4])
    assert np.array_equal(res['mask'], rs.compute_ransac_cost(res['T_cw'], pts, obs, rs.camera, THRESH)[0])
    assert res['cost_history'].shape == (1,) and np.isfinite(res['cost_history']).all()


@pytest.fixture(scope='module')
def tie_base():
    """The N = 67 scene, its H = 64 table, and the restatement's winning row and the row with the lowest count."""
    pts, obs, _, _ = sc.scene(67)
    samples, ref = sc.oracle(67, 64)
    per_row = ref['counts'].max(axis=1)
    return pts, obs, samples, ref, ref['best'], int(np.argmin(per_row)), per_row


# 4 H slots against the selection's stride of 256: exactly one stride; the only winner beyond it; a tie across it (the lower row
# wins); two strides with the later row planted first
@pytest.mark.parametrize('h,rows', [(64, (5, 63)), (65, (64,)), (65, (20, 64)), (129, (128, 3))])
def test_pnp_ties_go_to_the_first_maximum(tie_base, h, rows):
    import ransac_scenes
    pts, obs, samples, base, w, l, per_row = tie_base
    assert per_row[w] > per_row[l] and (per_row == per_row[w]).sum() == 1            # the base winner is unique
    table = ransac_scenes.tie_table(samples, w, l, h, rows)
    ref = ab.ransac(pts, obs, sc.CAM, table, THRESH, refine_winner=False, sensitivity=True)
    cond = sc.conditions(ref)
    assert cond['near'] == 0 and cond['near_final'] == 0                             # no squared error in the margin: nothing left out
    rs = solver(pts, obs, refine=False)
    res = rs._device_ransac(table)
    T_all, counts, empty, degenerate = rs._device_hypotheses(table)
    print('H = {} ({} slots), winner row {} (count {}) at {}, elsewhere row {} (count {}): device best {} slot {} count {}; '
          'restatement {} / {} / {}'.format(h, 4 * h, w, per_row[w], rows, l, per_row[l], res['best'], res['best_slot'], res['raw_count'],
                                            ref['best'], ref['best_slot'], ref['raw_count']))
    assert (res['best'], res['best_slot']) == (ref['best'], ref['best_slot']) == (min(rows), base['best_slot'])
    assert np.array_equal(counts, ref['counts']) and np.array_equal(empty, ref['empty'])
    assert res['raw_count'] == res['count'] == ref['raw_count'] == per_row[w]
    assert np.array_equal(res['mask'], ref['mask'])
    assert np.array_equal(res['T_cw'], T_all[res['best'], res['best_slot']])        # bit for bit: the refinement is off
    assert (T_all[list(rows)] == T_all[res['best']]).all()                          # every planted row is the same hypothesis


def test_two_calls_are_bit_identical(seeded):
    pts, obs, _, _ = sc.scene(192)
    _, _, _, samples = seeded
    rs = solver(pts, obs)
    a, b = rs._device_ransac(samples), rs._device_ransac(samples)
    for key in ('T_cw', 'mask', 'd', 'cost_history'):
        assert np.array_equal(a[key], b[key]), key
    keys = ('best', 'best_slot', 'raw_count', 'count', 'refine_kept', 'pivot_failed', 'iterations')
    assert [a[k] for k in keys] == [b[k] for k in keys]
    ha, hb = rs._device_hypotheses(samples), rs._device_hypotheses(samples)
    assert all(np.array_equal(x, y) for x, y in zip(ha, hb))


def test_minimal_inputs():
    pts, obs, T, samples = sc.minimal_four()
    # N = 3: three points, one sample, min_inliers = 3: every non-empty slot explains all three, the first of them wins
    ref3 = ab.ransac(pts[:3], obs[:3], sc.CAM, samples, THRESH, sensitivity=True)
    rs = solver(pts[:3], obs[:3], ransac_iters=1, min_inliers=3)
    compare_hypotheses(pts[:3], obs[:3], samples, ref3)
    res = rs._device_ransac(samples)
    compare_ransac(res, ref3)
    assert res['count'] == 3 and res['best_slot'] == int(np.argmax(~ref3['empty'][0]))
    np.random.seed(0)
    T_cw, in_pts, in_obs, inliers = rs.perform_ransac()                        # (one row: a permutation of 0 1 2)
    assert inliers.tolist() == [0, 1, 2] and np.isfinite(T_cw.as_matrix()).all()
    # N = 4 exact: the fourth point picks the right slot
    ref4 = ab.ransac(pts, obs, sc.CAM, samples, THRESH, sensitivity=True)
    rs4, T_all, counts = compare_hypotheses(pts, obs, samples, ref4)
    res = rs4._device_ransac(samples)
    compare_ransac(res, ref4)
    err = np.abs(T_all[0, res['best_slot']] - T).max()
    bound = 100. * ref4['sensitivity'][0, res['best_slot']] + 1e-12 + TOL_T
    print('four exact points: slot {} of counts {}, max|T - T_true| {:.2e} (bound {:.2e})'.format(res['best_slot'], counts[0].tolist(), err, bound))
    assert res['count'] == 4 and counts[0, res['best_slot']] == 4 and err <= bound


def test_flagged_samples_lose_and_only_flagged_samples_raise():
    pts, obs, _, _ = sc.scene(192)
    pts, obs = pts.copy(), obs.copy()
    pts[10:13] = pts[10] + np.outer([0., 1., 2.], [0.3, -0.2, 0.5])          # three collinear world points
    pts[20, 1] = np.nan
    obs[21] = np.inf
    samples = np.array([[4, 4, 5], [10, 11, 12], [20, 6, 7], [8, 21, 9], [33, 34, 35]], dtype=np.int32)
    ref = ab.ransac(pts, obs, sc.CAM, samples, THRESH, sensitivity=True)
    assert ref['degenerate'].tolist() == [True, True, True, True, False] and sc.conditions(ref)['near'] == 0
    rs = solver(pts, obs)
    T_all, counts, empty, degenerate = rs._device_hypotheses(samples)
    assert np.array_equal(degenerate, ref['degenerate']) and np.array_equal(empty, ref['empty']) and np.array_equal(counts, ref['counts'])
    assert np.isfinite(T_all).all() and not T_all[:4].any()
    res = rs._device_ransac(samples)
    assert res['best'] == 4 == ref['best'] and res['best_slot'] == ref['best_slot'] and not res['mask'][[20, 21]].any()
    # a table of only degenerate rows: count 0, everything finite, and the host refuses
    res = rs._device_ransac(samples[:4])
    assert res['count'] == 0 and res['raw_count'] == 0 and not res['mask'].any() and not res['refine_kept']
    assert not res['T_cw'].any() and np.isfinite(res['cost_history']).all()
    rs.draw_samples = lambda: samples[:4]
    with pytest.raises(ValueError, match='failed to find 12 inliers'):
        rs.perform_ransac()


def test_all_outliers_raise():
    pts, obs, T, outlier = synthetic.pnp_scene(outlier_fraction=1.0)
    assert outlier.all()
    rs = solver(pts, obs)
    np.random.seed(5)
    with pytest.raises(ValueError, match='failed to find 12 inliers'):
        rs.perform_ransac()
    assert rs.info_['count'] < 12


def test_the_exports_refuse_bad_arguments():
    from pyslam_amd import _native as nat
    pts, obs, _, _ = sc.scene(192)
    rs = solver(pts, obs)
    bad = sc.samples_of(192, 4)
    bad[2, 1] = 192
    with pytest.raises(nat.NativeError, match='sample index out of range'):
        rs._device_ransac(bad)
    with pytest.raises(nat.NativeError, match='sample index out of range'):
        rs._device_hypotheses(-bad - 1)
    two = solver(pts[:2], obs[:2])
    with pytest.raises(nat.NativeError, match='at least 3 points'):
        two._device_ransac(np.zeros((1, 3), dtype=np.int32))
    with pytest.raises(nat.NativeError, match='at least 3 points'):
        two.compute_ransac_cost(np.identity(4), pts[:2], obs[:2], two.camera, THRESH)
    for fu in (0., np.nan, np.inf):
        flat = solver(pts, obs)
        flat.camera = MonoCamera(320., 240., fu, 500., 640, 480)
        with pytest.raises(nat.NativeError, match='focal lengths must be finite and non-zero'):
            flat._device_hypotheses(sc.samples_of(192, 4))
    lib = nat.load()
    assert lib.ps_pnp_ransac(None, nat.f64p(obs), 192, nat.i32p(sc.samples_of(192, 4)), 4, nat.f64p(sc.CAM), THRESH, 5, None, None, None,
                             None, None) == -1 and b'bad argument' in lib.ps_last_error()


# ---- end to end: bootstrap -> register_frame -> three-keyframe monocular bundle adjustment ----------------------------------------

@pytest.fixture(scope='module')
def booted():
    obs_1, obs_2, T_21_true, _ = synthetic.two_view()
    T_21, points, status, inliers = twoview.bootstrap(camera(), obs_1, obs_2, min_parallax_deg=1.0, seed=5)
    ok = status == 0
    return obs_1, obs_2, T_21_true, T_21, points[ok], inliers[ok]


@pytest.fixture(scope='module')
def registered(booted):
    obs_1, obs_2, T_21_true, T_21, points, idx = booted
    _, obs_3, T_31_true, _ = sc.scene(192)
    T_31, inl = pnp.register_frame(camera(), points, obs_3[idx], seed=5)
    return obs_3[idx], T_31_true, T_31, inl


def test_register_frame_places_the_third_view_in_map_scale(booted, registered):
    obs_1, obs_2, T_21_true, T_21, points, idx = booted
    obs_3, T_31_true, T_31, inl = registered
    scale = 1. / np.linalg.norm(T_21_true[:3, 3])             # bootstrap's map has |t_21| = 1
    t_true = scale * T_31_true[:3, 3]
    Tm = T_31.as_matrix()
    e_rot, e_t = rot_angle(Tm[:3, :3], T_31_true[:3, :3]), np.linalg.norm(Tm[:3, 3] - t_true)
    # the restatement chain on the same input: absolute.py on the samples that seed 5 draws
    ref = ab.ransac(points, obs_3, sc.CAM, sc.ransac_samples(points.shape[0], 400, 5), THRESH)
    r_rot, r_t = rot_angle(ref['T_cw'][:3, :3], T_31_true[:3, :3]), np.linalg.norm(ref['T_cw'][:3, 3] - t_true)
    print('register_frame on {} bootstrapped landmarks: {} inliers (restatement {}); against the truth in map scale: rotation {:.3e} '
          'rad translation {:.3e}; restatement chain {:.3e} / {:.3e}'.format(points.shape[0], inl.size, ref['count'], e_rot, e_t, r_rot, r_t))
    assert inl.size >= 12 and e_rot <= 1.5 * r_rot and e_t <= 1.5 * r_t


def test_three_keyframe_monocular_bundle_adjustment(booted, registered):
    obs_1, obs_2, T_21_true, T_21, points, idx = booted
    obs_3, T_31_true, T_31, inl = registered
    from test_host_api import build_namespace
    ns = build_namespace()
    ns.MonoCamera = MonoCamera
    cam = camera()
    lp = pnp.three_view_tables(cam, T_21.as_matrix(), T_31.as_matrix(), obs_1[idx], obs_2[idx], points, inl, obs_3[inl])
    problem = synthetic.to_objects(lp, ns, ns.Options())
    final = problem.solve()
    assert problem._device is not None
    pts = np.stack([final[k] for k in lp.point_keys])
    T2, T3 = T_21.as_matrix(), final['T_3_w'].as_matrix()
    assert np.array_equal(final['T_2_w'].as_matrix(), T2)     # held
    e = [np.atleast_2d(cam.project(pts)) - obs_1[idx], np.atleast_2d(cam.project(pts @ T2[:3, :3].T + T2[:3, 3])) - obs_2[idx],
         np.atleast_2d(cam.project(pts[inl] @ T3[:3, :3].T + T3[:3, 3])) - obs_3[inl]]
    rms = np.sqrt(np.concatenate([(x ** 2).sum(axis=1) for x in e]).mean())
    hist = np.asarray(problem._cost_history)
    print('three-keyframe monocular BA: {} landmarks, {} seen by the third keyframe, cost history {}, reprojection RMS {:.3f} px'.format(
        pts.shape[0], inl.size, hist.tolist(), rms))
    # non-increasing to rounding: a residual is a difference of pixel coordinates up to 640 evaluated to a few ulps
    # (~8 * 2.2e-16 * 640 = 1.1e-12 px) against residuals of ~0.5 px, which is 2 * 1.1e-12 / 0.5 = 4.5e-12 of the cost
    assert np.isfinite(hist).all() and (np.diff(hist) <= 4.5e-12 * hist[0]).all()
    assert rms < 2 * 0.5                                      # 2 x pixel_noise of the synthetic scenes
