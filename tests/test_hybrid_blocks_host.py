"""CPU tests of Options.hybrid_blocks: which problems qualify, the host rows (pyslam_amd/hybrid.py) against the dense normal
equations of the generic path, and the C-ABI entry points of the host rows."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO


def _ns():
    from test_host_api import build_namespace
    return build_namespace()


def _pose_graph_problem(dof=6, hybrid=True, const_first=True):
    from pyslam_amd import synthetic
    lp, _ = synthetic.pose_graph(num_poses=12, num_loops=4, dof=dof, seed=3, const_first=const_first)
    ns = _ns()
    opt = ns.Options()
    opt.hybrid_blocks = hybrid
    return synthetic.to_objects(lp, ns, opt), lp, ns


def _only_user_blocks(dof=6):
    """Poses of a small graph with nothing but user blocks: a prior, a prior on the constant pose, smoothness blocks on
    (constant, variable, variable) poses and one that lists a pose twice."""
    from pyslam_amd import synthetic
    lp, _ = synthetic.pose_graph(num_poses=8, num_loops=0, dof=dof, seed=4, const_first=True)
    ns = _ns()
    opt = ns.Options()
    opt.hybrid_blocks = True
    problem = ns.Problem(opt)
    keys = lp.pose_keys
    problem.initialize_params(dict(zip(keys, synthetic.pose_objects(lp.poses, dof, ns))))
    problem.set_parameters_constant(keys[0])
    n = 3 if dof == 6 else 2
    S = np.linalg.cholesky(np.linalg.inv(0.1 * np.identity(n) + 0.01 * np.ones((n, n)))).T
    rng = np.random.default_rng(0)
    problem.add_residual_block(synthetic.TranslationPrior(rng.standard_normal(n), S), [keys[3]], ns.HuberLoss(0.5))
    problem.add_residual_block(synthetic.TranslationPrior(rng.standard_normal(n), S), [keys[0]], ns.L2Loss())
    problem.add_residual_block(synthetic.TranslationSmoothness(S), [keys[0], keys[1], keys[2]], ns.CauchyLoss(1.0))
    problem.add_residual_block(synthetic.TranslationSmoothness(S), [keys[4], keys[4], keys[6]], ns.L2Loss())
    problem.add_residual_block(synthetic.TranslationSmoothness(S), [keys[5], keys[6], keys[7]], ns.L2Loss())
    problem.add_residual_block(ns.PoseToPoseResidual(ns.SE3.identity() if dof == 6 else ns.SE2.identity(),
                                                     np.identity(dof)), [keys[2], keys[3]])
    problem.add_residual_block(synthetic.Untyped(ns.PoseToPoseResidual(ns.SE3.identity() if dof == 6 else ns.SE2.identity(),
                                                                       np.identity(dof))), [keys[1], keys[5]])
    return problem


class _Many:
    def evaluate(self, params, compute_jacobians=None):
        r = np.zeros(3)
        return (r, [np.zeros((3, 6)) for _ in params]) if compute_jacobians else r


def test_pose_only_user_blocks_qualify_and_the_option_off_keeps_the_generic_path():
    from pyslam_amd import synthetic
    from pyslam_amd.lowering import NotLowerable
    problem, lp, ns = _pose_graph_problem(hybrid=False)
    n = 3
    synthetic.add_user_blocks(problem, lp, ns, [0, 1], [[2, -1, -1], [0, 1, 2]], np.zeros((2, 3)),
                              np.tile(np.identity(n).ravel(), (2, 1)), [[0., 0.], [3., 1.]])
    with pytest.raises(NotLowerable):
        problem._lower()
    problem.options.hybrid_blocks = True
    lp2 = problem._lower()
    assert lp2.hybrid and list(lp2.h_blocks) == [len(problem.residual_blocks) - 2, len(problem.residual_blocks) - 1]
    # typed blocks stay in the tables as they are
    assert lp2.num_edges == lp.num_edges and lp2.num_priors == lp.num_priors
    # prior on pose 2 -> (-1, 2); smoothness on (constant 0, 1, 2) -> the one pair (1, 2)
    assert list(lp2.h_i) == [-1, 1] and list(lp2.h_j) == [2, 2] and list(lp2.h_ptr) == [0, 1, 2]
    assert list(lp2.h_pose) == [2, 0, 1, 2] and list(lp2.h_pose_ptr) == [0, 1, 4]
    assert lp2.same_tables(problem._lower())


def test_blocks_on_a_landmark_a_scalar_or_nine_poses_do_not_qualify():
    from pyslam_amd import synthetic
    from pyslam_amd.lowering import NotLowerable
    lp, _ = synthetic.stereo_ba(num_kf=4, num_lm=12, obs_per_lm=3, half_window=2, seed=2)
    ns = _ns()
    opt = ns.Options()
    opt.hybrid_blocks = True
    problem = synthetic.to_objects(lp, ns, opt)
    problem.add_residual_block(synthetic.Untyped(problem.residual_blocks[0]), problem.block_param_keys[0])
    with pytest.raises(NotLowerable, match='not a pose'):
        problem._lower()

    problem, lp, ns = _pose_graph_problem()
    problem.param_dict['scale'] = np.array([1.0])
    problem.add_residual_block(_Many(), ['scale'])
    with pytest.raises(NotLowerable):
        problem._lower()

    problem, lp, ns = _pose_graph_problem()
    problem.add_residual_block(_Many(), lp.pose_keys[:8])
    assert problem._lower().hybrid
    problem.add_residual_block(_Many(), lp.pose_keys[:9])
    with pytest.raises(NotLowerable, match='more than 8 poses'):
        problem._lower()


def test_mixed_groups_and_photometric_blocks_stay_on_the_generic_path():
    from pyslam_amd.lowering import NotLowerable
    problem, lp, ns = _pose_graph_problem()
    problem.param_dict['T2d'] = ns.SE2.identity()
    problem.add_residual_block(_Many(), ['T2d'])
    with pytest.raises(NotLowerable, match='mixed'):
        problem._lower()

    class Tagged(_Many):
        KIND = 'photometric'
    problem, lp, ns = _pose_graph_problem()
    problem.add_residual_block(Tagged(), [lp.pose_keys[1]])
    with pytest.raises(NotLowerable, match='no typed device kernel'):
        problem._lower()


@pytest.mark.parametrize('dof', [6, 3])
def test_pair_rows_reassemble_to_the_generic_normal_equations(dof):
    """sum over rows of [H11 | H12 | H22 | g1 | g2] placed at their poses == J~^T J~ and -J~^T e~ of _host_jacobian restricted
    to the user blocks (the typed pose-pose block is in the tables, so it is left out of both sides)."""
    from pyslam_amd.hybrid import HostBlocks
    problem = _only_user_blocks(dof)
    lp = problem._lower()
    assert lp.hybrid and lp.num_edges == 1
    host = HostBlocks(lp, problem.residual_blocks, problem.block_param_keys, problem.block_loss_functions, problem.param_dict)
    rows, cost = host.evaluate(lp.poses)
    cost_all, cost_var = host.cost(lp.poses, True), host.cost(lp.poses, False)
    user = [k for k, blk in enumerate(problem.residual_blocks) if getattr(blk, 'KIND', 'generic') == 'generic']
    # the cost of every user block, the one on the constant pose included (ps_eval_cost's include_all_constant)
    everything = sum(np.sum(problem.block_loss_functions[k].loss(problem.residual_blocks[k].evaluate(
        [problem.param_dict[key] for key in problem.block_param_keys[k]]))) for k in user)
    D, DD = dof, dof * dof
    nr = lp.num_reduced
    H, g = np.zeros((nr * D, nr * D)), np.zeros(nr * D)
    for k, (i, j) in enumerate(zip(lp.h_i, lp.h_j)):
        ra = lp.pose_rid[i] if i >= 0 else -1
        rb = lp.pose_rid[j]
        a, b = slice(ra * D, ra * D + D), slice(rb * D, rb * D + D)
        if ra >= 0:
            H[a, a] += rows[k, :DD].reshape(D, D)
            H[a, b] += rows[k, DD:2 * DD].reshape(D, D)
            H[b, a] += rows[k, DD:2 * DD].reshape(D, D).T
            g[a] += rows[k, 3 * DD:3 * DD + D]
        else:
            assert not rows[k, :2 * DD].any() and not rows[k, 3 * DD:3 * DD + D].any()
        H[b, b] += rows[k, 2 * DD:3 * DD].reshape(D, D)
        g[b] += rows[k, 3 * DD + D:]
    # the generic path's J~ over the same blocks (typed pose-pose block removed)
    typed = [k for k, blk in enumerate(problem.residual_blocks) if getattr(blk, 'KIND', 'generic') != 'generic']
    for k in reversed(typed):
        del problem.residual_blocks[k], problem.block_param_keys[k], problem.block_loss_functions[k]
    problem._update_partition_dict = problem._get_update_partition_dict()
    J, e, cost_ref = problem._host_jacobian()
    J = J.toarray()
    # partition order is the param_dict order of the variable poses = the device's reduced order here
    assert [problem._update_partition_dict[k].start for k in lp.pose_keys[1:]] == list(range(0, nr * D, D))
    scale = np.abs(J.T @ J).max()
    assert np.abs(H - J.T @ J).max() <= 1e-13 * scale
    assert np.abs(g + J.T @ e).max() <= 1e-13 * max(np.abs(J.T @ e).max(), 1.)
    assert abs(cost - cost_ref) <= 1e-14 * abs(cost_ref)
    assert abs(cost_all - everything) <= 1e-14 * everything and cost_all > cost_var
    assert abs(cost_var - cost_ref) <= 1e-14 * cost_ref


def test_host_row_entry_points_match_the_header():
    from pyslam_amd import _native
    header = open(os.path.join(REPO, 'include', 'pyslam_hip.h')).read()
    m = re.search(r'typedef struct ps_host_rows_desc \{(.*?)\} ps_host_rows_desc;', header, re.S)
    assert m and re.findall(r'(int64_t|const int32_t\*) (\w+);', m.group(1)) == [('int64_t', 'num'), ('const int32_t*', 'i'),
                                                                              ('const int32_t*', 'j')]
    assert [f for f, _ in _native.HostRowsDesc._fields_] == ['num', 'i', 'j'] and ctypes.sizeof(_native.HostRowsDesc) == 24
    for name, nargs in (('ps_problem_create_hybrid', 4), ('ps_set_host_rows', 4)):
        proto = re.search(r'int ' + name + r'\(([^)]*)\);', header)
        assert proto, name
        assert len(proto.group(1).split(',')) == nargs == len(_native.SIGNATURES[name][1])
    assert _native.SIGNATURES['ps_set_host_rows'][1][2] is ctypes.c_int64
    assert _native.SIGNATURES['ps_set_host_rows'][1][3] is ctypes.c_double
    assert _native.SIGNATURES['ps_problem_create_hybrid'][1][1]._type_ is _native.HostRowsDesc
