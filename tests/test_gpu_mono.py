"""Monocular bundle adjustment (camera type 2) and multi-view triangulation on the device, against the golden recorded from the
verbatim reference with this project's MonoCamera (tools/gen_mono_golden.py) and the numpy restatement
(pyslam_amd/triangulation.py).  Run with `-m gpu` on an MI355X.  Every comparison prints its figure before it asserts."""
import os

import numpy as np
import pytest

from conftest import load_golden, golden_lp, golden_options

from pyslam_amd import synthetic, triangulation
from pyslam_amd.lowering import pack_pose
from pyslam_amd.sensors import MonoCamera

pytestmark = pytest.mark.gpu

TOL_COST = 1e-9        # cost and cost history, relative (tests/test_gpu_parity.py holds the stereo goldens to 1e-10; measured here: <= 1.2e-10, the cost after the first L2 step; the issue sets 1e-9)
TOL_DX = 1e-8          # tests/test_gpu_parity.py (first step against the reference's spsolve)
COV_POSES, COV_POINTS = (2, 4), (3, 41)


def namespace():
    from test_host_api import build_namespace
    ns = build_namespace()
    ns.MonoCamera = MonoCamera
    return ns


def case(prefix, g=None):
    g = g or load_golden('mono_ba')
    sub = {k[len(prefix) + 1:]: v for k, v in g.items() if k.startswith(prefix + '_')}
    lp = golden_lp(sub)
    lp.pose_keys = ['T_cam{}_w'.format(i) for i in range(lp.num_poses)]
    lp.point_keys = ['pt{}_w'.format(j) for j in range(lp.num_points)]
    return sub, lp


def problem_of(prefix, **opts):
    sub, lp = case(prefix)
    ns = namespace()
    opt = ns.Options()
    for k, v in golden_options(sub).items():
        setattr(opt, k, v)
    for k, v in opts.items():
        setattr(opt, k, v)
    return sub, lp, synthetic.to_objects(lp, ns, opt)


@pytest.mark.parametrize('prefix', ['l2', 'huber', 'mixed'])
def test_parity_with_the_reference(prefix):
    sub, lp, problem = problem_of(prefix)
    ref = sub['cost_history']
    c0 = problem.eval_cost()
    print('{}: start cost rel diff {:.2e}'.format(prefix, abs(c0 - ref[0]) / ref[0]))
    assert abs(c0 - ref[0]) <= TOL_COST * ref[0]
    dx, cost = problem.solve_one_iter()
    e_dx = np.linalg.norm(dx - sub['iter_dx'][0]) / np.linalg.norm(sub['iter_dx'][0])
    print('{}: first step rel diff {:.2e}, cost after it {:.2e}'.format(prefix, e_dx, abs(cost - sub['iter_cost'][0]) / cost))
    assert e_dx < TOL_DX
    assert abs(cost - sub['iter_cost'][0]) <= TOL_COST * cost
    final = problem.solve()
    assert problem._device is not None and problem._device_sig == 'tables'         # the typed route, not the generic host path
    hist = np.array(problem._cost_history)
    assert len(hist) == len(ref), (hist, ref)
    print('{}: cost history rel diff {}'.format(prefix, np.abs(hist - ref) / ref))
    assert np.all(np.abs(hist - ref) <= TOL_COST * ref)
    if 'final_poses' not in sub:
        return
    e_pose = np.abs(np.stack([pack_pose(final[k]) for k in lp.pose_keys]) - sub['final_poses']).max()
    e_pt = np.abs(np.stack([final[k] for k in lp.point_keys]) - sub['final_points']).max()
    print('{}: final poses max abs diff {:.2e}, final points {:.2e}'.format(prefix, e_pose, e_pt))
    # monocular BA is worse conditioned than stereo: 10 x the deviation measured on the MI355X, never looser than 1e-6
    assert e_pose < 5.6e-12        # measured: l2 5.5e-13, huber 2.6e-13
    assert e_pt < 3.2e-9           # measured: l2 3.1e-10, huber 3.0e-10
    problem.compute_covariance()
    pk, lk = [lp.pose_keys[i] for i in COV_POSES], [lp.point_keys[j] for j in COV_POINTS]
    for name, (a, b) in {'cov_pose0': (pk[0], pk[0]), 'cov_pose1': (pk[1], pk[1]), 'cov_point0': (lk[0], lk[0]),
                         'cov_point1': (lk[1], lk[1]), 'cov_pose0_point0': (pk[0], lk[0])}.items():
        got = problem.get_covariance_block(a, b)
        print('{}: {} max rel diff {:.2e}'.format(prefix, name, np.abs(got - sub[name]).max() / np.abs(sub[name]).max()))
        assert np.allclose(got, sub[name], rtol=1e-9, atol=1e-15), name


def test_every_loss_with_a_monocular_camera_stays_finite():
    """The dead third row under every loss (L1's weight at 0 is NaN): cost, step and cost after the step are finite, and the
    L2 cost is the sum over the two live rows."""
    import types
    from pyslam_amd.device import DeviceProblem
    for loss_id, k in [(0, 0.), (1, 0.), (2, 2.5), (3, 1.2), (4, 6.0), (5, 4.0)]:
        # (a start close enough that Tukey's cut-off leaves every landmark live observations)
        lp, _ = synthetic.mono_ba(8, 80, obs_per_lm=4, half_window=3, seed=21, loss=types.SimpleNamespace(LOSS_ID=loss_id, k=k),
                                  pose_noise=1e-4, point_noise=1e-3)
        dev = DeviceProblem(lp)
        c0 = dev.eval_cost(True)
        cost, nrm, its, rel = dev.gn_iteration(0., 1e-12, 500, True)
        dev.close()
        assert np.isfinite([c0, cost, nrm]).all() and nrm > 0., (loss_id, c0, cost, nrm)
        if loss_id == 0:
            tr = triangulation._Tracks(lp, np.arange(lp.num_var_points))
            want = triangulation._evaluate(lp, tr, lp.points)[0].sum()
            assert abs(c0 - want) <= 1e-12 * want


def test_lm_adaptive_reaches_the_reference_cost():
    sub, lp, problem = problem_of('l2', lm_adaptive=True, max_iters=50, min_cost_decrease=1.0)
    problem.solve()
    hist = problem._cost_history
    # the golden's Gauss-Newton loop stopped at the reference's 10 % rule; both loops here run on (min_cost_decrease = 1) to the optimum below it
    ref, _, gn = problem_of('l2', max_iters=50, min_cost_decrease=1.0)
    gn.solve()
    print('lm final {:.12e}, gn run to convergence {:.12e}, golden final {:.12e}'.format(hist[-1], gn._cost_history[-1], sub['cost_history'][-1]))
    assert all(b <= a for a, b in zip(hist[:-1], hist[1:]))
    assert hist[-1] <= sub['cost_history'][-1] * (1 + 1e-6)
    assert abs(hist[-1] - gn._cost_history[-1]) <= 1e-6 * gn._cost_history[-1]        # tests/test_gpu_lm.py: 1e-6 relative


def test_marginals_equal_the_column_route():
    sub, lp, problem = problem_of('l2')
    pk, lk = [lp.pose_keys[i] for i in COV_POSES], [lp.point_keys[j] for j in COV_POINTS]
    pairs = [(pk[0], lk[0]), (lk[1], pk[1]), (lk[0], lk[1]), (pk[0], pk[1])]
    out = problem.compute_marginal_covariances(keys=pk + lk, cross_pairs=pairs)
    problem.compute_covariance()
    for key in list(pk + lk) + pairs:
        a, b = key if isinstance(key, tuple) else (key, key)
        ref = problem.get_covariance_block(a, b)
        print('marginal {}: max rel diff {:.2e}'.format(key, np.abs(out[key] - ref).max() / np.abs(ref).max()))
        assert np.abs(out[key] - ref).max() <= 1e-9 * np.abs(ref).max()                # tests/test_gpu_cov_marginals.py


def test_one_held_pose_is_a_clean_error():
    from pyslam_amd._native import NativeError
    sub, lp, _ = problem_of('l2')
    lp.pose_rid = np.arange(lp.num_poses, dtype=np.int32) - 1            # only pose 0 held: the scale is free
    lp.finalize()
    problem = synthetic.to_objects(lp, namespace())
    with pytest.raises(NativeError, match='singular|not positive definite'):
        problem.compute_marginal_covariances()


@pytest.fixture(scope='module')
def c3_mono():
    return synthetic.mono_ba(200, 50000, 10, 20, seed=0)


def test_c3_mono_solve_tables(c3_mono):
    from pyslam_amd import Options, solve_tables
    from pyslam_amd.device import DeviceProblem
    lp, truth = c3_mono
    st, _ = synthetic.stereo_ba(40, 2000, 6, 8, seed=4)
    rg = st.copy()
    rg.obs_uvd = rg.obs_uvd.copy(); rg.obs_uvd[:, 2] = rg.cams[0, 2] * rg.cams[0, 4] / rg.obs_uvd[:, 2]      # disparity -> depth
    rg.cams = rg.cams.copy(); rg.cams[0, 4] = -1.
    before = [solve_tables(x, Options()) for x in (st, rg)]
    opt = Options()
    opt.max_iters = 20
    hist, poses, points, stats = solve_tables(lp, opt)
    at_truth = lp.copy()
    at_truth.poses, at_truth.points = synthetic.pack_pose_matrices(truth['poses']), truth['points'].copy()
    dev = DeviceProblem(at_truth)
    c_truth = dev.eval_cost(True)
    dev.close()
    print('mono C3: history {}, cost at the truth {:.6e}, pcg iterations {}'.format(hist, c_truth, [s[0] for s in stats]))
    assert all(b < a for a, b in zip(hist[:-1], hist[1:]))
    assert np.isfinite(poses).all() and np.isfinite(points).all()
    assert hist[-1] <= c_truth          # the optimum fits the noise at least as well as the truth does
    after = [solve_tables(x, Options()) for x in (st, rg)]
    for a, b in zip(before, after):     # the stereo and RGB-D routes of the same session: bit for bit
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def tri_scene():
    g = load_golden('mono_ba')
    sub, lp = case('l2', g)
    lp.poses = g['tri_poses'].copy()
    return g, lp


def rel_diff(a, b):
    return (np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)).max()


def test_triangulation_equals_the_restatement_on_the_golden_scene():
    from pyslam_amd import triangulate_tables
    g, lp = tri_scene()
    mp = float(g['tri_min_parallax_deg'])
    for iters in (0, 5):
        pts, st = triangulate_tables(lp, iters, mp)
        want, wst = triangulation.triangulate_tables(lp, iters, mp)
        assert np.array_equal(st, wst) and not st.any()
        print('golden scene, refine_iters {}: device vs restatement max rel diff {:.2e}'.format(iters, rel_diff(pts, want)))
        # measured: 0 for the linear start (same operations in the same order, IEEE roots and quotients on both sides); 7.6e-8 after
        # five steps (the evaluator contracts multiply-adds, numpy does not, and the last accepted step of a landmark with little
        # parallax sits in the region where its cost is flat to rounding)
        assert rel_diff(pts, want) <= (0. if iters == 0 else 7.6e-7)
    again, st2 = triangulate_tables(lp, 5, mp)
    assert np.array_equal(again, pts) and np.array_equal(st, st2)         # two calls: bit-identical
    pts, st = triangulate_tables(lp, 20, mp)
    err = np.linalg.norm(pts - g['tri_refined'], axis=1).max()
    print('golden scene, 20 steps: device vs reference-refined points max |dp| {:.2e} m'.format(err))
    assert not st.any() and err < 4.2e-6                                # measured: 4.2e-7 m


def test_triangulation_status_codes_on_the_device():
    """The three constructed landmarks of tests/test_mono_host.py: the device's status array equals the restatement's."""
    from pyslam_amd import triangulate_tables
    g, lp = tri_scene()
    L = lp.num_points
    out = lp.copy()
    out.poses = np.concatenate([lp.poses, lp.poses[3:4]])
    out.pose_rid = np.full(7, -1, dtype=np.int32)
    out.points = np.concatenate([lp.points, [[1., 2., 3.], [4., 5., 6.], [7., 8., 9.]]])
    out.point_vid = np.arange(L + 3, dtype=np.int32)
    cu, cv, fu, fv = lp.cams[0, :4]
    R, t = lp.poses[:, :9].reshape(-1, 3, 3), lp.poses[:, 9:]

    def uv_of(pose, pw):
        pc = R[pose] @ pw + t[pose]
        return [fu * pc[0] / pc[2] + cu, fv * pc[1] / pc[2] + cv, 0.]
    pw = np.array([0.5, 0.2, 12.])
    a, b = uv_of(0, np.array([0., 0., 2.])), uv_of(5, np.array([0., 0., 2.]))
    new_obs = [(0, L, uv_of(0, pw)), (3, L + 1, uv_of(3, pw)), (6, L + 1, uv_of(3, pw)), (0, L + 2, b), (5, L + 2, a)]
    out.obs_pose = np.concatenate([lp.obs_pose, [o[0] for o in new_obs]]).astype(np.int32)
    out.obs_point = np.concatenate([lp.obs_point, [o[1] for o in new_obs]]).astype(np.int32)
    out.obs_uvd = np.concatenate([lp.obs_uvd, [o[2] for o in new_obs]])
    out.obs_grp = np.concatenate([lp.obs_grp, np.zeros(len(new_obs), dtype=np.int32)])
    out.finalize()
    mp = float(g['tri_min_parallax_deg'])
    pts, st = triangulate_tables(out, 5, mp)
    want, wst = triangulation.triangulate_tables(out, 5, mp)
    assert np.array_equal(st, wst) and st[L:].tolist() == [1, 2, 3]
    assert np.array_equal(pts[L:], out.points[L:])


def test_triangulation_equals_the_restatement_at_c3(c3_mono):
    from pyslam_amd import triangulate_tables
    lp, truth = c3_mono
    lp = lp.copy()
    lp.poses = synthetic.pack_pose_matrices(truth['poses'])
    pts, st = triangulate_tables(lp, 5, 0.05)
    want, wst = triangulation.triangulate_tables(lp, 5, 0.05)
    print('mono C3: status counts device {} restatement {}'.format(np.bincount(st, minlength=4), np.bincount(wst, minlength=4)))
    assert np.array_equal(st, wst)
    ok = st == 0
    d = np.linalg.norm(pts[ok] - want[ok], axis=1) / np.linalg.norm(want[ok], axis=1)
    print('mono C3: device vs restatement rel diff max {:.2e}, 99.9 % quantile {:.2e}'.format(d.max(), np.quantile(d, 0.999)))
    assert d.max() <= 2.1e-7            # measured: 2.1e-8 (99.9 % of the landmarks below 1.2e-8)


def test_triangulate_then_solve_end_to_end():
    """True poses + triangulated landmarks, then the golden's perturbed poses: solve() converges to the golden's final cost."""
    g = load_golden('mono_ba')
    sub, lp, _ = problem_of('l2')
    start = lp.copy()
    start.poses = g['tri_poses'].copy()
    start.points = np.zeros_like(lp.points) + [0., 0., 1.]            # nothing known about the landmarks
    ns = namespace()
    problem = synthetic.to_objects(start, ns, ns.Options())
    status = problem.triangulate_landmarks(min_parallax_deg=float(g['tri_min_parallax_deg']))
    assert set(status) == set(lp.point_keys) and not any(status.values())
    got = np.stack([problem.param_dict[k] for k in lp.point_keys])
    assert rel_diff(got, triangulation.triangulate(start, None, 5, float(g['tri_min_parallax_deg']))[0]) <= 7.6e-7                          # (the golden scene's five-step figure above)
    for key, row in zip(lp.pose_keys, lp.poses):                      # the golden's perturbed poses
        R, t = row[:9].reshape(3, 3), row[9:]
        problem.param_dict[key].rot.mat, problem.param_dict[key].trans = R.copy(), t.copy()
    problem.options.max_iters, problem.options.min_cost_decrease = 50, 1.0
    problem.solve()
    _, _, ref = problem_of('l2', max_iters=50, min_cost_decrease=1.0)
    ref.solve()
    print('end to end: final cost {:.12e}, from the golden start {:.12e}, golden (10 % rule) {:.12e}'.format(
        problem._cost_history[-1], ref._cost_history[-1], sub['cost_history'][-1]))
    assert abs(problem._cost_history[-1] - ref._cost_history[-1]) <= 1e-9 * ref._cost_history[-1]
    assert problem._cost_history[-1] <= sub['cost_history'][-1] * (1 + 1e-9)
    with pytest.raises(KeyError):
        problem.triangulate_landmarks(keys=['no_such_landmark'])


def test_one_rank_devices_route_on_the_golden_scene():
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29541', RANK='0', WORLD_SIZE='1')
    own = not dist.is_initialized()
    if own:
        dist.init_process_group('nccl', device_id=torch.device('cuda', 0))
    try:
        hist = {}
        for devices in (None, 'all'):
            _, _, problem = problem_of('l2', devices=devices)
            problem.solve()
            hist[devices] = list(problem._cost_history)
        print('devices None {} / all {}'.format(hist[None], hist['all']))
        assert len(hist[None]) == len(hist['all']) and np.allclose(hist[None], hist['all'], rtol=1e-9)   # tests/test_gpu_sharded.py
    finally:
        if own:
            dist.destroy_process_group()
