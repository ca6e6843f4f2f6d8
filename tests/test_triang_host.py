"""The scenes and references of the triangulation tests, checked on the host (no GPU): every scene of tests/triang_scenes.py has the
track lengths, camera mixes and lane loads it claims; the conditions tests/test_gpu_triang.py puts on its cases (share of landmarks
left out of the one-step comparison, share of unclear statuses) hold on the reference alone; the long-double reference
(tests/longdouble_triangulation.py) and the restatement (pyslam_amd/triangulation.py), written apart, agree; and the restatement keeps
a landmark whose refinement runs into L1's NaN weight."""
import numpy as np
import pytest

import longdouble_schur as ld
import longdouble_triangulation as lt
import offbox_scenes as sc
import test_gpu_triang as tg
import triang_scenes as ts
from pyslam_amd import triangulation
from pyslam_amd.lowering import pack_pose_matrices

needs_longdouble = pytest.mark.skipif(not ld.LONGDOUBLE_OK, reason=ld.LONGDOUBLE_SKIP)


def test_ldl_solve_against_numpy():
    rng = np.random.default_rng(3)
    B = rng.standard_normal((50, 3, 3))
    A = np.einsum('nij,nkj->nik', B, B) + 0.1 * np.identity(3)
    b = rng.standard_normal((50, 3))
    x, piv, ok = lt.ldl_solve(A, b)
    assert ok.all() and np.all(piv > 0) and np.all(piv <= 1 + 1e-12)
    assert np.allclose(x, np.linalg.solve(A, b[:, :, None])[:, :, 0], rtol=1e-9, atol=1e-12)
    A[0] = -A[0]
    A[1, 2, 2] = A[1, 2, 0] ** 2 / A[1, 0, 0] - 1.            # the third pivot is below -1
    A[2, 1, 1] = np.nan
    piv, ok = lt.ldl_solve(A, b)[1:]
    assert not ok[:3].any() and ok[3:].all() and np.all(piv[0] < 0)


@pytest.mark.parametrize('name', ts.OFFBOX + ts.STATUS_ONLY)
def test_offbox_scenes_stand_at_the_poses_they_were_projected_from(name):
    lp = ts.scene(name)
    src, truth = sc.scene(name)
    assert np.array_equal(lp.poses, pack_pose_matrices(truth['poses']))
    var = lp.point_vid >= 0
    assert np.all(lp.points[var] == ts.SENTINELS[0]) and np.array_equal(lp.points[~var], src.points[~var])
    other = ts.with_sentinel(lp, 1)
    assert np.all(other.points[var] == ts.SENTINELS[1]) and ts.SENTINELS[0] != ts.SENTINELS[1]
    assert np.array_equal(lp.obs_uvd, src.obs_uvd) and lp.num_var_points > 16 * 16      # more than one workgroup
    # the observations are their noise (PIXEL_NOISE px; mm: stereo_ba's 1 px) from the projection of the true points through these
    # poses (rms 0.30 to 0.32 px, mm 1.0); through mm's perturbed start poses the same figure is 11 px
    q = lp.copy()
    q.points = truth['points']
    r = tg.orc.eval_reproj(q, jac=False)
    assert np.sqrt(np.mean(r[:, :2] ** 2)) < 1.1 * (1. if name == 'mm' else ts.PIXEL_NOISE)


def test_offbox_scenes_cover_what_they_claim():
    for name in sc.MIXED_SCENES:
        lp = ts.scene(name)
        assert sc.landmarks_with_all_cameras(lp).size >= 50             # a landmark seen by all three camera types
        assert sc.min_classes_per_wave(lp) >= 2
        assert ts.has_loss(lp, 1).sum() > 200 and (~ts.has_loss(lp, 1)).sum() > 100     # L1 (test 5) and smooth (test 3) landmarks
        assert set(np.unique(lp.obs_groups[lp.obs_grp, 2])) == {0., 1., 2., 3.}         # L2, L1, Cauchy, Huber
    assert ts.scene('high_group_ids').obs_grp.max() >= 128
    assert ts.scene('wide_mixed').obs_groups.shape[0] > 255                              # the WIDE instantiation
    for name in ('near', 'base', 'far10', 'mm', 'mixed_depth'):
        assert ts.has_stereo(ts.scene(name)).all()
    d = ts.scene('far10').obs_uvd[:, 2]
    assert (d <= 0).any() and (d > 0).any()                                             # non-positive disparities occur


def test_tracks_scene():
    lp, truth, info = ts.tracks()
    assert lp.num_poses == ts.NUM_ARC_POSES and np.all(lp.pose_rid < 0) and np.all(lp.point_vid >= 0)
    n = ts.track_lengths(lp)
    assert n.tolist() == [i[0] for i in info]
    assert sorted(set(n.tolist())) == [1] + list(ts.TRACK_LENGTHS)
    assert sorted(-(-np.array(ts.TRACK_LENGTHS) // 16)) == [1, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5]   # observations of the fullest lane
    cam = ts.obs_camera(lp)
    order = np.argsort(lp.obs_point, kind='stable')
    start = np.concatenate([[0], np.cumsum(n)])
    seen_all_mono, seen_with_depth = set(), set()
    for j, (length, depth_group, mono_groups) in enumerate(info):
        rows = order[start[j]:start[j + 1]]
        c = cam[rows]
        if depth_group is None:
            assert np.all(c == -2.)
            seen_all_mono.add(length)
        else:
            assert np.all(c[:-1] == -2.) and c[-1] != -2. and lp.obs_grp[rows[-1]] == depth_group      # depth in the LAST slot
            seen_with_depth.add(length)
        assert len(set(lp.obs_pose[rows].tolist())) == length
    assert seen_all_mono == set(ts.TRACK_LENGTHS) and seen_with_depth == set(ts.TRACK_LENGTHS) | {1}
    assert {i[1] for i in info if i[0] == 1} == {ts.STEREO_L2, ts.RGBD_CAUCHY}
    assert ts.has_loss(lp, 1).any() and (~ts.has_loss(lp, 1)).sum() >= 10
    # the parallax gate: per all-mono track, the largest angle between two rays and the largest with a member in slots 0..15
    for j, (length, depth_group, _) in enumerate(info):
        if depth_group is not None:
            continue
        angle = ts.ray_angles_deg(lp, j)
        assert angle.max() > ts.TRACKS_PARALLAX_GATE + 0.5, (length, angle.max())
        if length >= 31:
            late = np.arange(length) >= 16
            early = angle[~(late[:, None] & late[None, :])].max()
            assert early < ts.TRACKS_PARALLAX_GATE - 0.5, (length, early)


def test_counts_scenes():
    base = ts.scene('base')
    for n in ts.COUNTS:
        lp = ts.counts(n)
        assert lp.num_var_points == n
        const = np.flatnonzero(lp.point_vid < 0)
        assert const.size == (ts.COUNTS_CONSTANT if n == max(ts.COUNTS) else 0)
        if const.size:
            assert const[0] > 0 and const[-1] < lp.num_points - 1 and np.all(np.diff(const) > 1)      # interleaved
            assert np.any(lp.point_vid[lp.point_vid >= 0] != np.flatnonzero(lp.point_vid >= 0))       # vid order is not point order
        # the same landmarks as base's first n, observation for observation
        want = triangulation.triangulate(base, np.arange(n), 5, 1.0)
        got = triangulation.triangulate(lp, None, 5, 1.0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        pts, st = triangulation.triangulate_tables(lp, 5, 1.0)
        assert np.all(st[const] == -1) and np.all(st[lp.point_vid >= 0] >= 0)
    assert sorted(set(-(-np.array(ts.COUNTS) // 16))) == [1, 2, 3]                                    # workgroups of 16 landmarks


@needs_longdouble
def test_decisions_scene():
    lp, named, _ = ts.decisions()
    assert lp.num_var_points > 16 and max(named.values()) >= 16 and min(named.values()) < 16          # across a workgroup's edge
    lin = lt.linear_start(lp)
    theta = float(np.degrees(np.arccos(lin.min_cos[named['two_rays']])))
    assert abs(theta - ts.DECISION_ANGLE_DEG) < 1e-9
    assert ts.track_lengths(lp)[named['late_pair']] == 18
    expected = dict(two_rays_and_stereo=0, one_mono=1, one_stereo=0, one_rgbd=0, behind=3, late_pair=0)
    for mp, two_rays in ((theta * (1 - 1e-6), 0), (theta * (1 + 1e-6), 2)):
        for iters in (0, 5):
            for pts, st in (lt.triangulate(lp, iters, mp)[:2], triangulation.triangulate(lp, None, iters, mp)):
                assert st[named['two_rays']] == two_rays
                assert all(st[named[k]] == v for k, v in expected.items())
                for k in ('zero_disparity', 'negative_disparity'):
                    assert st[named[k]] != 0
    d = lp.obs_uvd[:, 2][ts.obs_camera(lp) >= 0]
    assert (d == 0.).sum() == 1 and (d == -0.4).sum() == 1


@needs_longdouble
@pytest.mark.parametrize('name', ts.SCENES + ts.STATUS_ONLY)
def test_conditions_hold_on_the_reference_alone(name):
    lp = ts.scene(name)
    mp = 0.9 if name == 'decisions' else tg.MIN_PARALLAX_DEG
    for iters in (0, 5):
        pts, st, clear, _ = lt.triangulate(lp, iters, mp)
        unclear = 1. - clear.mean()
        print('{:15s} refine_iters {}: status {} unclear {:.1%}'.format(name, iters, np.bincount(st, minlength=4).tolist(), unclear))
        assert unclear <= (tg.UNCLEAR_FAR100 if name == 'far100' else tg.UNCLEAR)
        if name != 'far100':
            want = triangulation.triangulate(lp, None, iters, mp)[1]
            assert np.array_equal(st[clear], want[clear])
    if name in ts.STATUS_ONLY:
        return
    p1, inc, left_out, e64 = tg.one_step(name)
    print('{:15s} one step: {:.1%} left out, e64 {:.2e}; linear start e64 {:.2e}'.format(name, left_out, e64, tg.linear_e64(name)))
    assert (left_out <= tg.ONE_STEP_LEFT_OUT) == (name in tg.ONE_STEP_SCENES)
    twin_step, run_away = tg.converged_twin(name)
    print('{:15s} twin after 20 steps: step left {:.2e}, run away {:.1%}'.format(name, twin_step, run_away))
    assert run_away <= tg.RUNAWAY_SHARE
    # the restatement standing in for the device in test 3
    p20, s20 = triangulation.triangulate(lp, None, 20, tg.MIN_PARALLAX_DEG)
    left, gone = tg.step_size(lp, p20, (s20 == 0) & tg.smooth(name))
    print('{:15s} restatement after 20 steps: step left {:.2e}, run away {:.1%}'.format(name, left, gone))
    assert gone <= tg.RUNAWAY_SHARE and left <= tg.bound(twin_step, tg.FLOOR_CONVERGED)
    # the restatement, written apart from the reference, under the device's bound for the linear start
    r0, rst = triangulation.triangulate(lp, None, 0, tg.MIN_PARALLAX_DEG)
    ref, st, clear, lin = tg.reference(name, 0)
    rows = (rst == 0) & (st == 0)
    err = lt.point_err(r0, lin.point, rows)
    print('{:15s} restatement against the reference, linear start: {:.2e}'.format(name, err))
    assert rows.any() and err <= tg.bound(tg.linear_e64(name))


@needs_longdouble
@pytest.mark.parametrize('name', tg.MONOTONE_SCENES)
def test_restatement_keeps_l1_converged_landmarks(name):
    """With refine_iters the restatement must not lose a landmark it had (status 0 -> 2): under L1 the refinement converges onto a
    residual component of zero, where the weight is NaN and the 3 x 3 system has no solution -- the landmark is done, not degenerate.
    On mixed_wave 181 landmarks had gone that way after 20 steps."""
    lp = ts.scene(name)
    results = [triangulation.triangulate(lp, None, it, tg.MIN_PARALLAX_DEG) for it in tg.ITERS]
    counts = [np.bincount(st, minlength=4).tolist() for _, st in results]
    print(name, dict(zip(tg.ITERS, counts)))
    for a in range(len(results)):
        for b in range(a + 1, len(results)):
            sa, sb = results[a][1], results[b][1]
            assert not np.any((sa == 0) & (sb == triangulation.DEGENERATE))
    assert all(c[2] == counts[0][2] for c in counts)
    # and every landmark with an L1 observation that stopped on a NaN system sits where its cost is no higher than before
    p20, s20 = results[-1]
    p0, s0 = results[0]
    both = (s20 == 0) & (s0 == 0)
    c20, _, _, _, r1 = lt.evaluate(lp, np.where(both[:, None], p20, 1.))
    c0 = lt.evaluate(lp, np.where(both[:, None], p0, 1.))[0]
    assert np.all((c20 - c0)[both] <= lt.cost_slack(lp, r1)[both])
