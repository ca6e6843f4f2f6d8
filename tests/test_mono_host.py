"""Monocular camera, its lowering and the host restatement of the multi-view triangulation (no GPU)."""
import numpy as np
import pytest

from conftest import load_golden, golden_lp

from pyslam_amd import losses, lowering, synthetic, triangulation
from pyslam_amd.liegroups import SE3
from pyslam_amd.lowering import LoweredProblem, NotLowerable
from pyslam_amd.residuals.reprojection import ReprojectionMotionOnlyResidual, ReprojectionResidual
from pyslam_amd.sensors import MonoCamera, StereoCamera


def cam_pair():
    return MonoCamera(640., 480., 1000., 990., 1280, 960), StereoCamera(640., 480., 1000., 990., 0.25, 1280, 960)


def test_mono_camera_surface_and_project():
    import pyslam.sensors
    assert pyslam.sensors.MonoCamera is MonoCamera
    mono, stereo = cam_pair()
    assert mono.CAMERA_ID == 2 and not hasattr(mono, 'triangulate')
    assert np.array_equal(mono.intrinsics(), [640., 480., 1000., 990., -2.])
    assert mono.clone().intrinsics().tolist() == mono.intrinsics().tolist() and 'MonoCamera' in repr(mono)
    mono.compute_pixel_grid()
    assert mono.u_grid.shape == (960, 1280)
    assert mono.is_valid_measurement([[10., 10.], [-1., 5.], [5., 961.]]).tolist() == [True, False, False]
    pts = np.random.default_rng(0).uniform([-3, -2, 4], [3, 2, 20], (7, 3))
    uv, jac = mono.project(pts, True)
    uvd, jac3 = stereo.project(pts, True)
    assert uv.shape == (7, 2) and jac.shape == (7, 2, 3)
    assert np.array_equal(uv, uvd[:, :2]) and np.array_equal(jac, jac3[:, :2, :])
    assert mono.project(pts[0]).shape == (2,) and mono.project(pts[0], True)[1].shape == (2, 3)
    h = 1e-6
    for k in range(3):
        d = np.zeros(3); d[k] = h
        fd = (mono.project(pts + d) - mono.project(pts - d)) / (2 * h)
        assert np.allclose(fd, jac[:, :, k], rtol=1e-7, atol=1e-7)


def small_problem(cams, n_obs=(2, 2), loss=None, const=()):
    """Two poses, len(n_obs) landmarks; landmark j has n_obs[j] observations by cams[(j + q) % len(cams)]."""
    poses = {'T0': SE3.exp(np.zeros(6)), 'T1': SE3.exp(np.array([0.5, 0., 0., 0., 0.02, 0.]))}
    params = dict(poses)
    blocks, keys, lossf = [], [], []
    S2, S3 = np.diag([1., 2.]), np.diag([1., 2., 3.])
    for j, n in enumerate(n_obs):
        p = np.array([0.3 * j, -0.2, 8. + j])
        params['p{}'.format(j)] = p
        for q in range(n):
            cam = cams[(j + q) % len(cams)]
            obs = cam.project(poses['T{}'.format(q % 2)].dot(p))
            blocks.append(ReprojectionResidual(cam, obs, S2 if cam.CAMERA_ID == 2 else S3))
            keys.append(['T{}'.format(q % 2), 'p{}'.format(j)])
            lossf.append(loss or losses.L2Loss())
    return params, blocks, keys, lossf, list(const)


def test_lowering_mono_and_mixed():
    mono, stereo = cam_pair()
    lp = lowering.lower(*small_problem([mono], const=['T0', 'T1']))
    assert lp.cams.shape == (1, 5) and lp.cams[0, 4] == -2.
    assert np.all(lp.obs_uvd[:, 2] == 0.)
    assert np.array_equal(lp.stiff3[0].reshape(3, 3), np.diag([1., 2., 0.]))
    lp = lowering.lower(*small_problem([mono, stereo], n_obs=(2, 2, 2)))
    assert sorted(lp.cams[:, 4].tolist()) == [-2., 0.25]
    is_mono = lp.cams[lp.obs_groups[lp.obs_grp, 0].astype(int), 4] == -2.
    assert is_mono.sum() == 3 and np.all(lp.obs_uvd[is_mono, 2] == 0.) and np.all(lp.obs_uvd[~is_mono, 2] > 0.)
    for g in lp.obs_groups:
        S = lp.stiff3[int(g[1])].reshape(3, 3)
        assert np.array_equal(S, np.diag([1., 2., 0.]) if lp.cams[int(g[0]), 4] == -2. else np.diag([1., 2., 3.]))
    # the same tables with and without the C walk
    import os
    os.environ['PYSLAM_AMD_LOWER_FAST'] = '0'
    try:
        saved, lowering._FAST[:] = list(lowering._FAST), [False, None]
        lp2 = lowering.lower(*small_problem([mono, stereo], n_obs=(2, 2, 2)))
    finally:
        del os.environ['PYSLAM_AMD_LOWER_FAST']
        lowering._FAST[:] = saved
    assert lp.same_tables(lp2)


def test_lowering_errors():
    mono, stereo = cam_pair()
    args = list(small_problem([mono]))
    args[1][0].obs = np.array([1., 2., 3.])
    with pytest.raises(NotLowerable, match='2-vector'):
        lowering.lower(*args)
    args = list(small_problem([mono]))
    args[1][0].stiffness = np.identity(3)
    with pytest.raises(NotLowerable, match='2x2'):
        lowering.lower(*args)
    args = list(small_problem([stereo]))
    args[1][0].stiffness = np.identity(2)
    with pytest.raises(NotLowerable, match='3x3'):
        lowering.lower(*args)

    class FakeMono(MonoCamera):
        def triangulate(self, uv):
            return np.array([0., 0., 5.])
    block = ReprojectionMotionOnlyResidual(FakeMono(*mono.intrinsics()[:4], 1280, 960), np.zeros(2), np.zeros(2), np.identity(2))
    with pytest.raises(NotLowerable, match='monocular'):
        lowering.lower({'T0': SE3.exp(np.zeros(6))}, [block], [['T0']], [losses.L2Loss()], [])

    class OtherCamera(MonoCamera):
        CAMERA_ID = 7
    with pytest.raises(NotLowerable, match='no device restatement'):
        lowering.lower(*small_problem([OtherCamera(*mono.intrinsics()[:4], 1280, 960)]))
    # one monocular observation of a variable landmark: rank-deficient, named at lowering
    with pytest.raises(ValueError, match="'p1'"):
        lowering.lower(*small_problem([mono], n_obs=(2, 1)))
    lowering.lower(*small_problem([mono], n_obs=(2, 1), const=['p1', 'T0']))       # held constant: fine
    lowering.lower(*small_problem([stereo], n_obs=(2, 1)))                         # one stereo observation fixes a point


@pytest.mark.parametrize('loss', [losses.L2Loss(), losses.L1Loss(), losses.CauchyLoss(2.5), losses.HuberLoss(1.2),
                                  losses.TukeyLoss(6.0), losses.TDistributionLoss(4.0)], ids=lambda l: type(l).__name__)
def test_dead_row_adds_nothing(loss):
    """The third row of a monocular observation is r = 0: rho(0) = 0 for every loss.  sqrt(weight(0)) is finite for every loss
    but L1, whose weight at 0 is NaN by definition (reference losses.py:30-33) -- which is why the device pins that row's
    IRLS scale to 1 (csrc/ps_math.h) instead of evaluating it."""
    z = np.zeros(1)
    assert float(np.sum(loss.loss(z))) == 0.
    with np.errstate(all='ignore'):
        w = np.sqrt(np.asarray(loss.weight(z), dtype=float))
    assert np.all(np.isfinite(w)) or isinstance(loss, losses.L1Loss)


def test_mono_ba_tables_and_objects():
    lp, truth = synthetic.mono_ba(8, 40, obs_per_lm=4, half_window=3, seed=3)
    assert lp.pose_rid.tolist() == [-1, -1, 0, 1, 2, 3, 4, 5] and lp.cams[0, 4] == -2.
    assert np.array_equal(lp.poses[:2], lowering.pack_pose_matrices(truth['poses'][:2]))
    st, _ = synthetic.stereo_ba(8, 40, obs_per_lm=4, half_window=3, seed=3)
    assert np.array_equal(lp.obs_uvd[:, :2], st.obs_uvd[:, :2]) and np.array_equal(lp.obs_pose, st.obs_pose)
    from test_host_api import build_namespace
    ns = build_namespace()
    ns.MonoCamera = MonoCamera
    problem = synthetic.to_objects(lp, ns)
    assert lp.same_tables(problem._lower()) and np.array_equal(problem._lower().points, lp.points)
    mixed, _ = synthetic.mono_ba(8, 40, obs_per_lm=4, half_window=3, seed=3, stereo_fraction=0.4)
    low = synthetic.to_objects(mixed, ns)._lower()
    assert low.cams.shape == (2, 5) and low.num_obs == mixed.num_obs
    is_mono = low.cams[low.obs_groups[low.obs_grp, 0].astype(int), 4] == -2.
    assert np.array_equal(is_mono, mixed.obs_grp == 0) and np.array_equal(low.obs_uvd, mixed.obs_uvd)


def tri_scene():
    g = load_golden('mono_ba')
    lp = golden_lp({k[3:]: v for k, v in g.items() if k.startswith('l2_lp_')})
    lp.poses = g['tri_poses'].copy()
    return g, lp


def test_triangulation_restatement_against_golden():
    g, lp = tri_scene()
    mp = float(g['tri_min_parallax_deg'])
    lin, status = triangulation.triangulate(lp, None, refine_iters=0, min_parallax_deg=mp)
    assert not status.any()                      # (a condition on the scene: tools/gen_mono_golden.py asserts it too)
    assert np.array_equal(lin, g['tri_linear'])
    pts, status = triangulation.triangulate(lp, None, refine_iters=20, min_parallax_deg=mp)
    assert not status.any()
    # Both sides stop where a step no longer lowers the landmark's cost (the rule of the definition), i.e. somewhere inside the
    # region where the cost is flat to the rounding of its own evaluation: 0.5 lmin |dp|^2 <= noise, with lmin the smallest
    # eigenvalue of the landmark's H (the depth direction: down to 0.02 here, four rays over 15 cm at 28 m) and noise the
    # rounding of the cost c_j ~ 4, a sum of 12 squares each behind ~20 operations: ~50 eps c_j.  Hence, per landmark,
    # |dp| <= sqrt(2 * 50 eps c_j / lmin_j) (2e-6 m for the weakest landmark), times 10 for the margin.  H and c are
    # evaluated at the reference's points.
    tr = triangulation._Tracks(lp, np.arange(lp.num_var_points))
    c, H6, _, _ = triangulation._evaluate(lp, tr, g['tri_refined'])
    H = H6[:, [0, 1, 3, 1, 2, 4, 3, 4, 5]].reshape(-1, 3, 3)
    bound = 10. * np.sqrt(2. * 50. * np.finfo(float).eps * c / np.linalg.eigvalsh(H)[:, 0])
    err = np.linalg.norm(pts - g['tri_refined'], axis=1)
    print('restatement vs reference-refined points: largest |dp| {:.3e} m, largest |dp| / bound {:.3f}'.format(err.max(), (err / bound).max()))
    assert np.all(err <= bound)
    full, st = triangulation.triangulate_tables(lp, 20, mp)
    assert np.array_equal(full, pts) and not st.any()
    sel, st = triangulation.triangulate(lp, [5, 17], 20, mp)
    assert np.array_equal(sel, pts[[5, 17]])


def test_triangulation_status_codes():
    """Three constructed landmarks on top of the golden scene: one observation; two views from identical poses; a point whose
    rays meet behind the cameras.  Everything else stays ok."""
    g, lp = tri_scene()
    mp = float(g['tri_min_parallax_deg'])
    L = lp.num_points
    cu, cv, fu, fv = lp.cams[0, :4]
    out = lp.copy()
    out.poses = np.concatenate([lp.poses, lp.poses[3:4]])                  # pose 6 = a copy of pose 3
    out.pose_rid = np.full(7, -1, dtype=np.int32)
    old = np.array([[1., 2., 3.], [4., 5., 6.], [7., 8., 9.]])
    out.points = np.concatenate([lp.points, old])
    out.point_vid = np.arange(L + 3, dtype=np.int32)
    R = lp.poses[:, :9].reshape(-1, 3, 3)
    t = lp.poses[:, 9:]

    def uv_of(pose, pw):
        pc = R[pose] @ pw + t[pose]
        return [fu * pc[0] / pc[2] + cu, fv * pc[1] / pc[2] + cv, 0.]
    pw = np.array([0.5, 0.2, 12.])
    # rays that diverge in front of the cameras (they meet behind them): swap the two views' image positions of a near point
    a, b = uv_of(0, np.array([0., 0., 2.])), uv_of(5, np.array([0., 0., 2.]))
    new_obs = [(0, L, uv_of(0, pw)), (3, L + 1, uv_of(3, pw)), (6, L + 1, uv_of(3, pw)), (0, L + 2, b), (5, L + 2, a)]
    out.obs_pose = np.concatenate([lp.obs_pose, [o[0] for o in new_obs]]).astype(np.int32)
    out.obs_point = np.concatenate([lp.obs_point, [o[1] for o in new_obs]]).astype(np.int32)
    out.obs_uvd = np.concatenate([lp.obs_uvd, [o[2] for o in new_obs]])
    out.obs_grp = np.concatenate([lp.obs_grp, np.zeros(len(new_obs), dtype=np.int32)])
    out.finalize()
    pts, status = triangulation.triangulate(out, None, refine_iters=5, min_parallax_deg=mp)
    assert status[L:].tolist() == [triangulation.FEW_OBS, triangulation.DEGENERATE, triangulation.BEHIND]
    assert not status[:L].any()
    assert np.array_equal(pts[L:], old)                                    # a non-zero status keeps the old value
    assert lowering.underdetermined_mono_points(out.cams, out.obs_groups, out.obs_grp, out.obs_point, out.point_vid).tolist() == [L]
    # a stereo observation bears depth: one is enough
    st, _ = synthetic.stereo_ba(6, 10, obs_per_lm=1, half_window=3, seed=2, pose_noise=0., point_noise=0.)
    pts, status = triangulation.triangulate(st, None, refine_iters=5)
    # ... and the point is the one the camera's own triangulate gives for it, in the world frame
    pc = synthetic._triangulate(st.cams[0], st.obs_uvd)
    R, t = st.poses[st.obs_pose, :9].reshape(-1, 3, 3), st.poses[st.obs_pose, 9:]
    want = np.einsum('nji,nj->ni', R, pc - t)
    assert not status.any() and np.allclose(pts[st.obs_point], want, rtol=1e-9, atol=1e-9)
