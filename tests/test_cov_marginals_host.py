"""Host side of Problem.compute_marginal_covariances: the device-order -> key mapping of the batched marginals, key and
pose_pairs validation.  No GPU: the blocks are placed by hand where the device would put them."""
import numpy as np
import pytest

from pyslam_amd import synthetic
from pyslam_amd.problem import marginal_blocks_by_key, pose_pair_indices

from test_host_api import build_namespace


def _lowered(lp):
    problem = synthetic.to_objects(lp, build_namespace())
    return problem, problem._lower()


def _hand_placed(lp):
    """pose[rid] = (rid + 1) * I + 0.01 J, point[vid] = -(vid + 1) * I: every block says where it came from."""
    nr, nv = int((lp.pose_rid >= 0).sum()), int((lp.point_vid >= 0).sum())
    pose = np.array([(r + 1.) * np.eye(lp.dof) + 0.01 for r in range(nr)]).reshape(nr, lp.dof, lp.dof)
    point = np.array([-(v + 1.) * np.eye(3) for v in range(nv)]).reshape(nv, 3, 3)
    return pose, point


def test_mapping_with_constant_poses_and_fixed_landmarks():
    lp0, _ = synthetic.stereo_ba(num_kf=6, num_lm=40, obs_per_lm=3, half_window=2, seed=4, const_point_fraction=0.25)
    lp0.pose_rid[3] = -1                  # a second constant pose in the middle of the trajectory
    lp0.pose_rid[lp0.pose_rid >= 0] = np.arange(int((lp0.pose_rid >= 0).sum()))
    problem, lp = _lowered(lp0)
    assert (lp.pose_rid < 0).sum() == 2 and (lp.point_vid < 0).sum() > 0 and (lp.point_vid >= 0).sum() > 0
    pose, point = _hand_placed(lp)
    part = problem._get_update_partition_dict()
    out = marginal_blocks_by_key(lp, pose, point, list(part))
    assert set(out) == set(part)
    for k, rid in zip(lp.pose_keys, lp.pose_rid):
        if rid >= 0:
            assert np.array_equal(out[k], (rid + 1.) * np.eye(6) + 0.01) and out[k].shape == (6, 6)
        else:
            assert k not in out
    for k, vid in zip(lp.point_keys, lp.point_vid):
        if vid >= 0:
            assert np.array_equal(out[k], -(vid + 1.) * np.eye(3))
        else:
            assert k not in out
    # the mapping does not depend on the order the keys were inserted in (reference order != device order)
    problem2 = synthetic.to_objects(lp0, build_namespace(), points_first=False)
    lp2 = problem2._lower()
    out2 = marginal_blocks_by_key(lp2, *_hand_placed(lp2), list(part))
    for k, rid in zip(lp.pose_keys, lp.pose_rid):
        if rid >= 0:
            assert np.array_equal(out2[k], out[k])


def test_mapping_se2_pose_graph():
    lp0, _ = synthetic.pose_graph(num_poses=12, num_loops=5, dof=3, seed=1, prior_first=False, const_first=True)
    problem, lp = _lowered(lp0)
    assert lp.dof == 3 and lp.pose_rid[0] < 0
    pose, point = _hand_placed(lp)
    out = marginal_blocks_by_key(lp, pose, point, list(problem._get_update_partition_dict()))
    assert len(out) == 11
    for k, rid in zip(lp.pose_keys[1:], lp.pose_rid[1:]):
        assert out[k].shape == (3, 3) and np.array_equal(out[k], (rid + 1.) * np.eye(3) + 0.01)
    a, b = pose_pair_indices(lp, [(lp.pose_keys[2], lp.pose_keys[7]), (lp.pose_keys[5], lp.pose_keys[5])])
    assert a.dtype == np.int32 and list(a) == [lp.pose_rid[2], lp.pose_rid[5]] and list(b) == [lp.pose_rid[7], lp.pose_rid[5]]


def test_constant_and_unknown_keys_raise_keyerror():
    lp0, _ = synthetic.stereo_ba(num_kf=4, num_lm=10, obs_per_lm=2, half_window=1, seed=2, const_point_fraction=0.3)
    problem, lp = _lowered(lp0)
    const_pose = lp.pose_keys[0]
    const_point = [k for k, v in zip(lp.point_keys, lp.point_vid) if v < 0][0]
    pose, point = _hand_placed(lp)
    for k in (const_pose, const_point):
        with pytest.raises(KeyError, match='constant'):
            marginal_blocks_by_key(lp, pose, point, [k])
        with pytest.raises(KeyError, match='constant') as e:
            problem.compute_marginal_covariances(keys=[k])
        assert repr(k) in str(e.value)
    with pytest.raises(KeyError, match='no_such_key'):
        problem.compute_marginal_covariances(keys=['no_such_key'])
    with pytest.raises(KeyError, match='no_such_key'):
        marginal_blocks_by_key(lp, pose, point, ['no_such_key'])
    # a pair naming a constant or unknown key: KeyError as well (before anything runs on a device)
    with pytest.raises(KeyError, match='constant'):
        problem.compute_marginal_covariances(keys=[], pose_pairs=[(lp.pose_keys[1], const_pose)])
    with pytest.raises(KeyError, match='nope'):
        problem.compute_marginal_covariances(keys=[], pose_pairs=[('nope', lp.pose_keys[1])])


def test_pose_pairs_validation():
    lp0, _ = synthetic.stereo_ba(num_kf=4, num_lm=10, obs_per_lm=2, half_window=1, seed=2)
    problem, lp = _lowered(lp0)
    for bad in (['T1'], [('T1',)], [('T1', 'T2', 'T3')], ['ab'], [5]):
        with pytest.raises(ValueError, match='pose_pairs'):
            problem.compute_marginal_covariances(keys=[], pose_pairs=bad)
    var_point = [k for k, v in zip(lp.point_keys, lp.point_vid) if v >= 0][0]
    with pytest.raises(ValueError, match='not a variable pose'):
        pose_pair_indices(lp, [(lp.pose_keys[1], var_point)])
    with pytest.raises(ValueError, match='not a variable pose'):
        pose_pair_indices(lp, [(lp.pose_keys[0], lp.pose_keys[1])])       # (the constant first pose)
    a, b = pose_pair_indices(lp, [(lp.pose_keys[1], lp.pose_keys[3])])
    assert list(a) == [lp.pose_rid[1]] and list(b) == [lp.pose_rid[3]]
