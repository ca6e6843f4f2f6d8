"""Absolute-pose (PnP) registration, host side: the restatement (pyslam_amd/pipelines/absolute.py) against the exact scene, its slot,
tie, degeneracy and refinement rules, the C ABI of the new exports, the error paths of pyslam_amd/pipelines/pnp.py, and the
conditions tests/test_gpu_pnp.py relies on for every committed seed and shape (tests/pnp_scenes.py).  No device."""
import os
import re

import numpy as np
import pytest

import pnp_scenes as sc
from pyslam_amd import synthetic
from pyslam_amd.liegroups import SE3, SO3
from pyslam_amd.pipelines import absolute as ab

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM, THRESH = sc.CAM, sc.THRESH


def rot_angle(Ra, Rb):
    return np.linalg.norm(SO3.from_matrix(Ra @ Rb.T, normalize=True).log())


def pose_error(T, T_true):
    return rot_angle(T[:3, :3], T_true[:3, :3]), np.linalg.norm(T[:3, 3] - T_true[:3, 3])


def test_the_scene_generator():
    pts, obs, T, outlier = synthetic.pnp_scene()
    assert pts.shape == (192, 3) and obs.shape == (192, 2) and T.shape == (4, 4) and outlier.sum() == 57 and outlier[-57:].all()
    assert np.array_equal(pts, synthetic.two_view_points())                     # the cloud of two_view ...
    assert not np.allclose(T, synthetic.two_view()[2])                          # ... from another pose than its second
    again = synthetic.pnp_scene()
    assert np.array_equal(obs, again[1]) and np.allclose(T[:3, :3] @ T[:3, :3].T, np.identity(3))
    p = pts @ T[:3, :3].T + T[:3, 3]
    assert (p[:, 2] > 0.).all()
    clean = synthetic.pnp_scene(pixel_noise=0., outlier_fraction=0.)
    assert not clean[3].any()
    proj = np.stack([500. * p[:, 0] / p[:, 2] + 320., 500. * p[:, 1] / p[:, 2] + 240.], axis=1)
    assert np.abs(clean[1] - proj).max() < 1e-10
    assert np.abs(obs[~outlier] - proj[~outlier]).max() < 5 * 0.5


def test_every_sample_reproduces_the_true_pose_on_the_exact_scene():
    pts, obs, T, _ = sc.scene(192, pixel_noise=0., outlier_fraction=0.)
    samples = sc.samples_of(192, 256)
    hyp = ab.hypotheses(pts, obs, CAM, samples, THRESH)
    assert not hyp['degenerate'].any() and np.isfinite(hyp['T_all']).all()
    err = np.abs(hyp['T_all'] - T).reshape(256, 4, 16).max(axis=2)
    err[hyp['empty']] = np.inf
    k = err.argmin(axis=1)
    rows = np.arange(256)
    e, s = err[rows, k], hyp['sensitivity'][rows, k]
    bound = 100. * s + 1e-12                                  # the issue's bound: 100 x that slot's sensitivity figure, plus 1e-12
    w = int(np.argmax(e / bound))
    print('noise-free scene: worst max|T - T_true| {:.2e} (sample {}); worst against its bound: {:.2e} of {:.2e} (sample {}, '
          'sensitivity {:.2e})'.format(e.max(), int(np.argmax(e)), e[w], bound[w], w, s[w]))
    assert (e <= bound).all()
    assert (hyp['counts'][rows, k] == 192).all()              # every point is an inlier of that slot
    assert (hyp['counts'][hyp['empty']] == 0).all() and not hyp['T_all'][hyp['empty']].any()


def test_the_slot_order_is_the_root_formula_s():
    pts, obs, _, _ = sc.scene(192)
    f = ab.bearings(obs, CAM)
    seen = set()
    for smp in sc.samples_of(192, 64):
        A, _, _, _ = ab.quartic(pts[smp].tolist(), f[smp].tolist())
        roots = ab.quartic_roots(A)
        real = sorted(r.real for r in np.roots(A) if abs(r.imag) < 1e-9 * (1. + abs(r)) and r.real > 0.)
        got = [r for r in roots if r is not None]
        assert len(got) == len(real) and np.allclose(sorted(got), real, rtol=1e-7, atol=0.)
        for a, b in ((0, 1), (2, 3)):                         # either quadratic emits + sqrt D first: its larger root
            assert (roots[a] is None) == (roots[b] is None) or roots[a] is not None
            if roots[a] is not None and roots[b] is not None:
                assert roots[a] >= roots[b]
        seen.add(tuple(r is not None for r in roots))
    assert len(seen) > 1                                      # more than one emptiness pattern among the samples
    assert ab.quartic_roots((0., 1., 1., 1., 1.)) == [None] * 4              # A_4 = 0: a zero denominator
    assert ab.quartic_roots((1., 0., 2., 0., 1.)) == [None] * 4              # (x^2 + 1)^2: no real root


def test_planted_ties_the_first_maximum_wins():
    pts, obs, _, _ = sc.scene(192)
    samples = sc.samples_of(192, 8)
    samples[6] = samples[1]                                   # the same sample twice: equal slots, equal counts
    ref = ab.ransac(pts, obs, CAM, samples[[3, 6, 1, 6]], THRESH, refine_winner=False)
    assert np.array_equal(ref['counts'][1], ref['counts'][2]) and np.array_equal(ref['T_all'][1], ref['T_all'][2])
    alone = ab.ransac(pts, obs, CAM, samples[[6, 3]], THRESH, refine_winner=False)
    if alone['best'] == 0:                                    # the doubled sample beats sample 3: its first copy wins
        assert ref['best'] == 1 and np.array_equal(ref['T_cw'], ref['T_all'][1, ref['best_slot']])
    else:
        assert ref['best'] == 0
    twice = ab.ransac(pts, obs, CAM, samples[[6, 1]], THRESH, refine_winner=False)
    assert twice['best'] == 0 and twice['counts'][0].max() == twice['counts'][1].max()
    # exactly three points: every non-empty slot explains all three, so all non-empty slots tie and the first of them wins
    tied = 0
    for smp in sc.samples_of(192, 32):
        p3, o3 = pts[smp], obs[smp]
        ref = ab.ransac(p3, o3, CAM, np.array([[0, 1, 2]]), THRESH, refine_winner=False)
        ne = ~ref['empty'][0]
        assert (ref['counts'][0][ne] == 3).all() and (ref['counts'][0][~ne] == 0).all()
        assert ref['best'] == 0 and ref['best_slot'] == int(np.argmax(ne)) and ref['count'] == (3 if ne.any() else 0)
        assert np.array_equal(ref['T_cw'], ref['T_all'][0, ref['best_slot']])
        tied += ne.sum() >= 2
    assert tied >= 16                                          # (most samples have two poses)


def test_degenerate_samples_are_flagged_and_stay_finite():
    pts, obs, _, _ = sc.scene(192)
    pts, obs = pts.copy(), obs.copy()
    pts[10:13] = pts[10] + np.outer([0., 1., 2.], [0.3, -0.2, 0.5])          # three collinear world points
    pts[20, 1] = np.nan
    obs[21] = np.inf
    pts[30] = pts[31]                                                         # a side of length zero
    samples = np.array([[1, 2, 3], [4, 4, 5], [10, 11, 12], [20, 6, 7], [8, 21, 9], [30, 31, 32], [33, 34, 35]], dtype=np.int32)
    ref = ab.ransac(pts, obs, CAM, samples, THRESH)
    assert ref['degenerate'].tolist() == [False, True, True, True, True, True, False]
    deg = ref['degenerate']
    assert ref['empty'][deg].all() and not ref['counts'][deg].any() and not ref['T_all'][deg].any()
    assert np.isfinite(ref['T_all']).all() and np.isfinite(ref['T_cw']).all() and ref['best'] in (0, 6)
    assert not ref['mask'][[20, 21]].any()                    # a non-finite row is never an inlier
    only = ab.ransac(pts, obs, CAM, samples[1:6], THRESH)
    assert only['degenerate'].all() and only['best'] == 0 and only['best_slot'] == 0 and only['count'] == 0
    assert not only['T_cw'].any() and not only['refine_kept'] and np.isfinite(only['cost_history']).all()


def test_the_refinement():
    pts, obs, T, outlier = sc.scene(192)
    samples, ref = sc.seeded_oracle()
    _, raw = sc.seeded_oracle(refine=False)
    hist = ref['cost_history']
    print('refinement: cost history {}, raw count {} -> {}, kept {}'.format(hist.tolist(), ref['raw_count'], ref['count'], ref['refine_kept']))
    assert hist.shape == (6,) and np.isfinite(hist).all()
    # non-increasing to rounding: a residual is a difference of pixel coordinates up to 640 evaluated to a few ulps
    # (~8 * 2.2e-16 * 640 = 1.1e-12 px) against residuals of ~0.5 px, which is 2 * 1.1e-12 / 0.5 = 4.5e-12 of the cost
    assert (np.diff(hist) <= 4.5e-12 * hist[0]).all() and hist[-1] < hist[0]
    assert ref['best'] == raw['best'] and ref['raw_count'] == raw['count'] and ref['count'] >= ref['raw_count'] and ref['refine_kept']
    assert np.array_equal(raw['T_cw'], ref['T_raw']) and not raw['refine_kept'] and raw['cost_history'].shape == (1,)
    (r0, t0), (r1, t1) = pose_error(ref['T_raw'], T), pose_error(ref['T_cw'], T)
    print('against the truth: raw rotation {:.3e} translation {:.3e}; refined {:.3e} / {:.3e}'.format(r0, t0, r1, t1))
    assert r1 <= r0 and t1 <= t0
    assert (ref['mask'] & ~outlier).sum() >= 0.8 * (~outlier).sum()
    # the Jacobian is the derivative of the residual under T <- exp(xi) T
    Tm = ref['T_cw']
    J = ab.jacobians(Tm, pts[:5], CAM)
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = 1e-6
        num = (ab.residuals(SE3.exp(xi).as_matrix() @ Tm, pts[:5], obs[:5], CAM) -
               ab.residuals(SE3.exp(-xi).as_matrix() @ Tm, pts[:5], obs[:5], CAM)) / 2e-6
        assert np.allclose(J[:, :, k], num, rtol=1e-6, atol=1e-6)


def test_a_failing_pivot_returns_the_raw_pose_bit_for_bit():
    pts, obs, T, _ = sc.scene(192)
    samples, ref = sc.seeded_oracle()
    two = np.zeros(192, dtype=bool)
    two[np.where(ref['mask'])[0][:2]] = True                  # two inliers: four equations for six unknowns
    T2, ok, hist = ab.refine(ref['T_raw'], pts, obs, CAM, two, 5)
    assert not ok and np.array_equal(T2, ref['T_raw']) and (hist == hist[0]).all()
    # through ransac(): a threshold that at most a sample's own points meet (their error is rounding, possibly 0) leaves fewer than
    # three inliers, H has rank <= 4 and a pivot fails
    none = ab.ransac(pts, obs, CAM, samples[:8], 1e-300)
    assert none['raw_count'] < 3 and not none['pivot_ok'] and not none['refine_kept']
    assert np.array_equal(none['T_cw'], none['T_all'][none['best'], none['best_slot']])
    Hm = np.identity(6)
    Hm[0, 1] = Hm[1, 0] = 1. - 1e-13                          # the second pivot is 2e-13 of its diagonal entry
    xi, ok = ab.cholesky_solve(Hm, np.ones(6))
    assert not ok and not xi.any()
    xi, ok = ab.cholesky_solve(np.diag([1., 2., 4., 1., 2., 4.]), np.ones(6))
    assert ok and np.allclose(xi, [-1., -.5, -.25, -1., -.5, -.25])


def test_the_c_abi_of_the_new_exports():
    from pyslam_amd import _native as nat
    names = ('ps_pnp_hypotheses', 'ps_pnp_ransac', 'ps_pnp_score')
    header = open(os.path.join(REPO, 'include', 'pyslam_hip.h')).read()
    src = open(os.path.join(REPO, 'pyslam_amd', 'csrc', 'ps_abi_pnp.h')).read()
    for name in names:
        decl = re.search(r'\bint ' + name + r'\((.*?)\);', header, re.S).group(1)
        defn = re.search(r'\nint ' + name + r'\((.*?)\) \{', src, re.S).group(1)
        assert name in nat.SIGNATURES, name
        assert len(decl.split(',')) == len(defn.split(',')) == len(nat.SIGNATURES[name][1]), name
    assert (len(nat.SIGNATURES['ps_pnp_hypotheses'][1]), len(nat.SIGNATURES['ps_pnp_score'][1]), len(nat.SIGNATURES['ps_pnp_ransac'][1])) == (10, 9, 13)
    core = open(os.path.join(REPO, 'pyslam_amd', 'csrc', 'ps_core.hip')).read()
    assert '#include "ps_k_pnp.h"' in core and '#include "ps_abi_pnp.h"' in core
    assert core.index('#include "ps_k_twoview.h"') < core.index('#include "ps_k_pnp.h"')
    assert core.index('#include "ps_abi_twoview.h"') < core.index('#include "ps_abi_pnp.h"')
    import __graft_entry__ as g
    assert {'ps_k_pnp.h', 'ps_abi_pnp.h'} <= set(os.listdir(os.path.dirname(g.SRC)))       # the build hash covers every file of csrc/
    kern = open(os.path.join(REPO, 'pyslam_amd', 'csrc', 'ps_k_pnp.h')).read()
    assert re.search(r'atomic\w*\s*\(', kern, re.I) is None     # no atomic call: every sum in a fixed order
    for k in ('k_pnp_normalise', 'k_pnp_hypotheses', 'k_pnp_best', 'k_pnp_refine'):
        assert re.search(r'__global__ __launch_bounds__\(256\) void ' + k + r'\(', kern), k


def test_errors_and_imports():
    import pyslam.pipelines.pnp as shim
    from pyslam_amd.pipelines import pnp
    from pyslam_amd.sensors import MonoCamera
    assert shim.PnPRANSAC is pnp.PnPRANSAC and shim.register_frame is pnp.register_frame and shim.three_view_tables is pnp.three_view_tables
    cam = MonoCamera(*synthetic.TWO_VIEW_CAMERA)
    rs = pnp.PnPRANSAC(cam)
    assert (rs.ransac_iters, rs.ransac_thresh, rs.num_min_set_pts, rs.min_inliers, rs.refine, rs.refine_iters) == (400, 4.0, 3, 12, True, 5)
    pts, obs, _, _ = sc.scene(192)
    rs.set_obs(pts[:2], obs[:2])
    with pytest.raises(ValueError, match='at least 3 correspondences'):
        rs.perform_ransac()
    with pytest.raises(ValueError, match='same number of points'):
        rs.set_obs(pts, obs[:100])
    with pytest.raises(ValueError, match=r'pts_w must have shape \(N, 3\)'):
        rs.set_obs(pts[:, :2], obs)
    with pytest.raises(ValueError, match=r'shape \(N, 2\) or \(N, 3\)'):
        rs.set_obs(pts, obs.T)
    rs.set_obs(pts, np.concatenate([obs, np.ones((192, 1))], axis=1))          # a third column is ignored
    assert rs.obs.shape == (192, 2) and np.array_equal(rs.obs, obs) and rs.num_pts == 192
    with pytest.raises(ValueError, match=r'shape \(H, 3\)'):
        rs._samples(np.zeros((4, 8), dtype=np.int32))
    np.random.seed(sc.RANSAC_SEED)
    s = rs.draw_samples()
    assert s.shape == (400, 3) and s.dtype == np.int32 and all(np.unique(r).size == 3 for r in s)
    assert np.array_equal(s, sc.ransac_samples())
    rs.num_min_set_pts = 4
    with pytest.raises(ValueError, match='P3P'):
        rs.perform_ransac()
    rs.num_min_set_pts = 3
    # too few inliers: the device's answer stands in here (the device path itself: tests/test_gpu_pnp.py)
    from pyslam_amd import _native as nat
    few = dict(T_cw=np.identity(4), mask=np.arange(192) < 9, best=0, best_slot=0, raw_count=9, count=9, refine_kept=False,
               d=np.zeros(192), cost_history=np.zeros(6))
    rs._device_ransac = lambda idx: few
    real = nat.require_gpu
    nat.require_gpu = lambda: None
    try:
        with pytest.raises(ValueError, match='failed to find 12 inliers'):
            rs.perform_ransac()
        with pytest.raises(ValueError, match='failed to find 12 inliers'):
            pnp.register_frame(cam, pts, obs, seed=1, ransac=rs)
        rs.min_inliers = 9
        T_cw, inliers = pnp.register_frame(cam, pts, obs, seed=1, ransac=rs)
        assert inliers.tolist() == list(range(9)) and np.array_equal(T_cw.as_matrix(), np.identity(4))
    finally:
        nat.require_gpu = real
    lp = pnp.three_view_tables(cam, np.identity(4), np.identity(4), obs[:5], obs[:5], pts[:5], [1, 3], obs[[1, 3]])
    assert lp.num_poses == 3 and lp.pose_rid.tolist() == [-1, -1, 0] and lp.num_var_points == 5 and lp.num_obs == 12
    assert lp.cams[0, 4] == -2. and lp.obs_pose.tolist() == [0] * 5 + [1] * 5 + [2] * 2 and lp.obs_point[-2:].tolist() == [1, 3]


# ---- the conditions tests/test_gpu_pnp.py relies on, for every committed seed and shape (tests/pnp_scenes.py) -----------------------

def check_conditions(name, ref, unique_or_rule=True):
    c = sc.conditions(ref)
    print('{}: pairs in the margin {} of {} (final poses: {}), smallest branch margin {:.2e}, slots above the sensitivity limit '
          '{:.2%} (worst {:.2e}), unique winner {}'.format(name, c['near'], c['pairs'], c['near_final'], c['branch'], c['loose'],
                                                           c['worst_sens'], c['unique']))
    assert c['near'] == 0 and c['near_final'] == 0            # margin condition
    assert c['branch'] > sc.BRANCH                            # branch condition
    assert c['loose'] <= sc.SENS_CAP                          # sensitivity cap
    flat = ref['counts'].reshape(-1)
    assert 4 * ref['best'] + ref['best_slot'] == int(np.argmax(flat))         # unique winner, or the tie resolved by the stated rule
    assert np.isfinite(ref['sensitivity'][~ref['empty']]).all()               # no slot changes its emptiness under the perturbation
    return c


def test_committed_shapes_meet_the_conditions():
    assert sc.SHAPES == [(192, 256), (67, 64), (257, 64)]
    for n, h in sc.SHAPES:
        for refine in (True, False):
            samples, ref = sc.oracle(n, h, refine)
            assert samples.shape == (h, 3) and not ref['degenerate'].any() and ref['raw_count'] >= 12
            check_conditions('N = {}, H = {}, refine {}'.format(n, h, refine), ref)
    n, h, row = sc.SINGLE
    pts, obs, _, _ = sc.scene(n)
    one = ab.ransac(pts, obs, CAM, sc.samples_of(n, h)[row:row + 1], THRESH, sensitivity=True)
    assert not one['empty'].all()
    check_conditions('a single hypothesis', one)
    for refine in (True, False):
        samples, ref = sc.seeded_oracle(refine)
        assert samples.shape == (400, 3)
        check_conditions('perform_ransac with seed {}, refine {}'.format(sc.RANSAC_SEED, refine), ref)


def test_the_minimal_inputs_meet_the_conditions():
    pts, obs, T, samples = sc.minimal_four()
    ref = ab.ransac(pts, obs, CAM, samples, THRESH, sensitivity=True)
    c = check_conditions('four exact points', ref)
    ne = ~ref['empty'][0]
    assert ne.sum() >= 2 and sorted(ref['counts'][0][ne].tolist())[-2:] == [3, 4]          # the fourth point picks the slot
    assert ref['count'] == 4 and np.abs(ref['T_all'][0, ref['best_slot']] - T).max() <= 100. * ref['sensitivity'][0, ref['best_slot']] + 1e-12
    three = ab.ransac(pts[:3], obs[:3], CAM, samples, THRESH, sensitivity=True)
    check_conditions('three points', three)
    assert three['count'] == 3 and three['best_slot'] == int(np.argmax(~three['empty'][0]))
