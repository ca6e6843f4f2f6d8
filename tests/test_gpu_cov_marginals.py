"""Batched marginal covariances (Problem.compute_marginal_covariances, ps_covariance_marginals) against the reference's
covariance goldens, the numpy oracle's dense inverse and the per-column route (ps_covariance_column)."""
import numpy as np
import pytest

from conftest import load_golden, golden_lp, golden_options
from oracle import gn_oracle as orc
from pyslam_amd import synthetic
from pyslam_amd._native import NativeError

pytestmark = pytest.mark.gpu


def device(lp):
    from pyslam_amd.device import DeviceProblem
    return DeviceProblem(lp)


def close(blk, ref, rel):
    return np.abs(blk - ref).max() <= rel * np.abs(ref).max()


@pytest.mark.parametrize('name', ['ba_tiny_huber', 'stereo_ba_example', 'pg_orientation_huber', 'posegraph_2d_example',
                                  'posegraph_3d_example'])
def test_marginals_match_the_reference_covariance(name):
    from test_host_api import build_namespace
    g = load_golden(name)
    lp = golden_lp(g)
    ns = build_namespace()
    opt = ns.Options()
    for k, v in golden_options(g).items():
        setattr(opt, k, v)
    problem = synthetic.to_objects(lp, ns, opt, points_first=bool(g.get('points_first', True)))
    problem.solve()
    ref = g['covariance']
    part = problem._get_update_partition_dict()
    pkeys = lp.pose_keys or ['T{}'.format(i) for i in range(lp.num_poses)]
    var = [pkeys[i] for i in range(lp.num_poses) if lp.pose_rid[i] >= 0]
    if lp.num_edges:
        pairs = [(pkeys[i], pkeys[j]) for i, j in zip(lp.e_i, lp.e_j) if lp.pose_rid[i] >= 0 and lp.pose_rid[j] >= 0][:4]
    else:
        pairs = list(zip(var[:-1], var[1:]))[:4]
    pairs.append((var[-1], var[0]))
    out = problem.compute_marginal_covariances(pose_pairs=pairs)
    assert set(out) == set(part) | set(pairs)
    tol = 1e-9 * np.abs(ref).max()
    for k, r in part.items():
        assert out[k].shape == (len(r), len(r))
        assert np.abs(out[k] - ref[r.start:r.stop, r.start:r.stop]).max() <= tol, k
    for ka, kb in pairs:
        ra, rb = part[ka], part[kb]
        assert np.abs(out[(ka, kb)] - ref[ra.start:ra.stop, rb.start:rb.stop]).max() <= tol, (ka, kb)
    # the column route's state is untouched: compute_covariance still works as before afterwards
    problem.compute_covariance()
    assert np.linalg.norm(problem._covariance_matrix - ref) <= 1e-9 * np.linalg.norm(ref)


def test_marginals_generic_route_cubic():
    from pyslam.problem import Problem
    g = load_golden('cubic')

    class CubicResidual:
        def __init__(self, x, y):
            self.x, self.y = np.atleast_1d(x), np.atleast_1d(y)

        def evaluate(self, params, compute_jacobians=None):
            a, b, c, d = params
            r = a * self.x ** 3 + b * self.x ** 2 + c * self.x + d - self.y
            if compute_jacobians:
                return r, np.squeeze([self.x ** 3, self.x ** 2, self.x, np.atleast_1d(1.)])
            return r

    problem = Problem()
    for xi, yi in zip(g['x'], g['y']):
        problem.add_residual_block(CubicResidual(xi, yi), ['a', 'b', 'c', 'd'])
    problem.initialize_params(dict(zip('abcd', g['init'])))
    problem.solve()
    ref = g['covariance']
    out = problem.compute_marginal_covariances(pose_pairs=[('a', 'd'), ('c', 'b')])
    tol = 1e-9 * np.abs(ref).max()
    for q, k in enumerate('abcd'):
        assert out[k].shape == (1, 1) and abs(out[k][0, 0] - ref[q, q]) <= tol
    assert abs(out[('a', 'd')][0, 0] - ref[0, 3]) <= tol and abs(out[('c', 'b')][0, 0] - ref[2, 1]) <= tol


@pytest.fixture(scope='module')
def medium():
    """30 keyframes, 2 000 landmarks with tracks of 20 observations (longer than one 16-lane group), three constant poses,
    a tenth of the landmarks fixed."""
    lp, _ = synthetic.stereo_ba(num_kf=30, num_lm=2000, obs_per_lm=20, half_window=12, seed=7, const_point_fraction=0.1)
    lp.pose_rid[[11, 23]] = -1
    lp.pose_rid[lp.pose_rid >= 0] = np.arange(int((lp.pose_rid >= 0).sum()))
    lp.finalize()
    return lp


def test_marginals_match_the_oracle_inverse(medium):
    lp = medium
    P, _, _ = orc.normal_equations(lp, points_first=False)
    cov = np.linalg.inv(P.toarray())
    dev = device(lp)
    try:
        dev.covariance_begin()
        pose, point = dev.covariance_marginals()
        nr, nv = dev.nr, dev.nv
        assert pose.shape == (nr, 6, 6) and point.shape == (nv, 3, 3) and nr == 27
        for r in range(nr):
            assert close(pose[r], cov[6 * r:6 * r + 6, 6 * r:6 * r + 6], 1e-9), r
        o = 6 * nr
        for v in range(nv):
            assert close(point[v], cov[o + 3 * v:o + 3 * v + 3, o + 3 * v:o + 3 * v + 3], 1e-9), v
        a = np.array([0, 3, 26, 10], dtype=np.int32)
        b = np.array([1, 20, 0, 10], dtype=np.int32)
        for k, blk in enumerate(dev.covariance_pose_blocks(a, b)):
            assert close(blk, cov[6 * a[k]:6 * a[k] + 6, 6 * b[k]:6 * b[k] + 6], 1e-9), k
    finally:
        dev.close()
    # through the Problem API: every variable parameter, and none of the constant ones
    from test_host_api import build_namespace
    problem = synthetic.to_objects(lp, build_namespace())
    out = problem.compute_marginal_covariances()
    low = problem._lower()
    var = {k for k, r in zip(low.pose_keys, low.pose_rid) if r >= 0} | {k for k, v in zip(low.point_keys, low.point_vid) if v >= 0}
    assert set(out) == var and len(var) == 27 + int((lp.point_vid >= 0).sum())
    for k, r in zip(low.pose_keys, low.pose_rid):
        if r >= 0:
            assert close(out[k], pose[r], 1e-9)


@pytest.fixture(scope='module')
def c3():
    lp, _ = synthetic.stereo_ba(200, 50000, 10, 20, seed=0)
    return lp


def test_c3_marginals_match_the_column_route(c3):
    dev = device(c3)
    try:
        dev.covariance_begin()
        pose, point = dev.covariance_marginals()
        pose2, point2 = dev.covariance_marginals()
        assert np.array_equal(pose, pose2) and np.array_equal(point, point2)         # bit-identical
        assert np.array_equal(pose, np.transpose(pose, (0, 2, 1))) and np.array_equal(point, np.transpose(point, (0, 2, 1)))
        assert np.linalg.eigvalsh(pose).min() > 0 and np.linalg.eigvalsh(point).min() > 0
        assert np.isfinite(pose).all() and np.isfinite(point).all()
        nr, nv = dev.nr, dev.nv
        rids = np.linspace(0, nr - 1, 16).astype(int)
        for r in rids:
            col = np.stack([dev.covariance_column(0, int(r), c, tol=1e-13)[0][r] for c in range(6)], axis=1)
            assert close(pose[r], col, 1e-8), r
        # landmarks spread over the trajectory and the track lengths
        lm_len = np.bincount(c3.obs_point, minlength=c3.num_points)
        vid_len = np.zeros(nv, dtype=int)
        vid_len[c3.point_vid[c3.point_vid >= 0]] = lm_len[c3.point_vid >= 0]
        order = np.argsort(vid_len, kind='stable')
        vids = order[np.linspace(0, nv - 1, 64).astype(int)]
        for v in vids:
            col = np.stack([dev.covariance_column(1, int(v), c, tol=1e-13)[1][v] for c in range(3)], axis=1)
            assert close(point[v], col, 1e-8), v
    finally:
        dev.close()


def test_large_dense_pose_graph_matches_the_column_route():
    lp, _ = synthetic.pose_graph(num_poses=2000, num_loops=4000, dof=6, seed=3, prior_first=True)
    dev = device(lp)
    try:
        dev.covariance_begin()
        assert dev.nr * 6 == 12000
        pose, point = dev.covariance_marginals()
        assert point.shape == (0, 3, 3) and np.isfinite(pose).all()
        a = np.array([0, 999, 1999, 500, 1999], dtype=np.int32)
        b = np.array([0, 999, 1999, 1500, 0], dtype=np.int32)
        cross = dev.covariance_pose_blocks(a, b)
        cols = {}
        for r in sorted(set(b.tolist())):
            cols[r] = [dev.covariance_column(0, r, c, tol=1e-13)[0] for c in range(6)]
        for k in range(len(a)):
            ref = np.stack([cols[int(b[k])][c][a[k]] for c in range(6)], axis=1)
            assert close(cross[k], ref, 1e-8), k
            if a[k] == b[k]:
                assert np.array_equal(cross[k], pose[a[k]])
    finally:
        dev.close()


def test_gauge_freedom_raises_without_nans():
    from test_host_api import build_namespace
    lp, _ = synthetic.pose_graph(num_poses=40, num_loops=60, dof=6, seed=5, prior_first=False, const_first=False)
    problem = synthetic.to_objects(lp, build_namespace())
    with pytest.raises(NativeError, match='gauge freedom'):
        problem.compute_marginal_covariances()
    dev = device(lp)
    try:
        try:
            dev.covariance_begin()
        except NativeError as e:          # (the block-diagonal check may already see it)
            assert 'gauge freedom' in str(e)
            return
        with pytest.raises(NativeError, match='gauge freedom'):
            dev.covariance_marginals()
        with pytest.raises(NativeError, match='no dense inverse'):
            dev.covariance_pose_blocks([0], [0])
    finally:
        dev.close()


def test_above_the_dense_limit_raises():
    from pyslam_amd.device import COVARIANCE_MARGINALS_LIMIT
    assert COVARIANCE_MARGINALS_LIMIT == 12288
    lp, _ = synthetic.pose_graph(num_poses=4097, num_loops=100, dof=3, seed=6, prior_first=True)
    dev = device(lp)
    try:
        dev.covariance_begin()
        assert dev.nr * 3 == 12291
        with pytest.raises(NativeError, match='PS_COV_DENSE_MAX_UNKNOWNS = 12288') as e:
            dev.covariance_marginals()
        assert 'get_covariance_block' in str(e.value)
    finally:
        dev.close()


def test_marginals_need_covariance_begin():
    lp, _ = synthetic.stereo_ba(num_kf=6, num_lm=64, obs_per_lm=4, half_window=3, seed=1)
    dev = device(lp)
    try:
        with pytest.raises(NativeError, match='ps_covariance_begin first'):
            dev.covariance_marginals()
        with pytest.raises(NativeError, match='no dense inverse'):
            dev.covariance_pose_blocks([0], [1])
        dev.covariance_begin()
        pose, point = dev.covariance_marginals()
        assert np.isfinite(pose).all() and np.isfinite(point).all()
        dev.linearize(0.)                  # a linearisation ends the inverse's life
        with pytest.raises(NativeError, match='no dense inverse'):
            dev.covariance_pose_blocks([0], [1])
        with pytest.raises(NativeError, match='ps_covariance_begin first'):
            dev.covariance_marginals()
    finally:
        dev.close()
