"""Host side of Problem.compute_marginal_covariances(cross_pairs=...): the key -> (kind, rid / vid) mapping of the cross blocks,
cross_pairs validation, and where the device's (n, 36) rows land.  No GPU: the rows are placed by hand."""
import numpy as np
import pytest

from pyslam_amd import synthetic
from pyslam_amd.problem import cross_blocks_by_key, cross_pair_indices

from test_host_api import build_namespace


def _lowered(lp):
    problem = synthetic.to_objects(lp, build_namespace())
    return problem, problem._lower()


@pytest.fixture(scope='module')
def lowered():
    lp0, _ = synthetic.stereo_ba(num_kf=6, num_lm=40, obs_per_lm=3, half_window=2, seed=4, const_point_fraction=0.25)
    lp0.pose_rid[3] = -1                  # a second constant pose in the middle of the trajectory
    lp0.pose_rid[lp0.pose_rid >= 0] = np.arange(int((lp0.pose_rid >= 0).sum()))
    problem, lp = _lowered(lp0)
    assert (lp.pose_rid < 0).sum() == 2 and (lp.point_vid < 0).sum() > 0 and (lp.point_vid >= 0).sum() > 0
    return problem, lp


def _variables(lp):
    poses = [(k, int(r)) for k, r in zip(lp.pose_keys, lp.pose_rid) if r >= 0]
    points = [(k, int(v)) for k, v in zip(lp.point_keys, lp.point_vid) if v >= 0]
    return poses, points


def test_cross_pair_indices_with_constant_poses_and_fixed_landmarks(lowered):
    _, lp = lowered
    poses, points = _variables(lp)
    pairs, want = [], []
    for (kp, r), (kl, v) in zip(poses, points):
        pairs += [(kp, kl), (kl, kp)]
        want += [(0, r, 1, v), (1, v, 0, r)]
    pairs += [(points[0][0], points[-1][0]), (points[2][0], points[2][0]), (poses[1][0], poses[-1][0])]
    want += [(1, points[0][1], 1, points[-1][1]), (1, points[2][1], 1, points[2][1]), (0, poses[1][1], 0, poses[-1][1])]
    ka, a, kb, b = cross_pair_indices(lp, pairs)
    for arr in (ka, a, kb, b):
        assert arr.dtype == np.int32 and arr.shape == (len(pairs),) and arr.flags['C_CONTIGUOUS']
    assert [tuple(int(x) for x in t) for t in zip(ka, a, kb, b)] == want
    # the rid / vid of a key does not depend on the order the keys were inserted in
    problem2 = synthetic.to_objects(lp, build_namespace(), points_first=False)
    lp2 = problem2._lower()
    assert all(np.array_equal(x, y) for x, y in zip(cross_pair_indices(lp2, pairs), (ka, a, kb, b)))


def test_constant_and_unknown_keys_raise_keyerror(lowered):
    problem, lp = lowered
    poses, points = _variables(lp)
    const_pose = [k for k, r in zip(lp.pose_keys, lp.pose_rid) if r < 0][1]
    const_point = [k for k, v in zip(lp.point_keys, lp.point_vid) if v < 0][0]
    for k in (const_pose, const_point):
        with pytest.raises(KeyError, match='constant') as e:
            cross_pair_indices(lp, [(poses[0][0], points[0][0]), (points[0][0], k)])
        assert repr(k) in str(e.value)
        with pytest.raises(KeyError, match='constant'):
            problem.compute_marginal_covariances(keys=[], cross_pairs=[(k, points[0][0])])
    with pytest.raises(KeyError, match='no_such_key'):
        cross_pair_indices(lp, [(poses[0][0], 'no_such_key')])
    with pytest.raises(KeyError, match='no_such_key'):
        problem.compute_marginal_covariances(keys=[], cross_pairs=[('no_such_key', poses[0][0])])


def test_cross_pairs_validation(lowered):
    problem, lp = lowered
    for bad in (['T1'], [('T1',)], [('T1', 'T2', 'T3')], ['ab'], [5]):
        with pytest.raises(ValueError, match='cross_pairs'):
            problem.compute_marginal_covariances(keys=[], cross_pairs=bad)
    # pose_pairs keeps its own name in its errors
    with pytest.raises(ValueError, match='pose_pairs'):
        problem.compute_marginal_covariances(keys=[], pose_pairs=['ab'], cross_pairs=[])


def test_rows_land_under_their_keys_in_the_requested_orientation(lowered):
    _, lp = lowered
    poses, points = _variables(lp)
    (p0, _), (p1, _) = poses[0], poses[2]
    (l0, _), (l1, _) = points[0], points[3]
    pairs = [(p0, l0), (l0, p0), (l0, l1), (l1, l1), (p0, p1)]
    ka, a, kb, b = cross_pair_indices(lp, pairs)
    # row k holds 100 k + (the row-major position) in its leading dof_a * dof_b entries, NaN beyond
    shapes = [(6, 3), (3, 6), (3, 3), (3, 3), (6, 6)]
    rows = np.full((len(pairs), 36), np.nan)
    for k, (da, db) in enumerate(shapes):
        rows[k, :da * db] = 100. * k + np.arange(da * db)
    out = cross_blocks_by_key(pairs, ka, kb, lp.dof, rows)
    assert list(out) == pairs
    for k, pr in enumerate(pairs):
        da, db = shapes[k]
        assert out[pr].shape == (da, db)
        assert np.array_equal(out[pr], (100. * k + np.arange(da * db)).reshape(da, db))
    rows[0, 0] = -1.                       # a copy, not a view of the device's array
    assert out[(p0, l0)][0, 0] == 0.


def test_se2_pose_graph_pairs_are_3_by_3():
    lp0, _ = synthetic.pose_graph(num_poses=12, num_loops=5, dof=3, seed=1, prior_first=False, const_first=True)
    _, lp = _lowered(lp0)
    pairs = [(lp.pose_keys[2], lp.pose_keys[7]), (lp.pose_keys[5], lp.pose_keys[5])]
    ka, a, kb, b = cross_pair_indices(lp, pairs)
    assert list(ka) == [0, 0] and list(kb) == [0, 0]
    assert list(a) == [lp.pose_rid[2], lp.pose_rid[5]] and list(b) == [lp.pose_rid[7], lp.pose_rid[5]]
    rows = np.arange(72, dtype=float).reshape(2, 36)
    out = cross_blocks_by_key(pairs, ka, kb, lp.dof, rows)
    assert out[pairs[0]].shape == (3, 3) and np.array_equal(out[pairs[1]], np.arange(36, 45.).reshape(3, 3))
