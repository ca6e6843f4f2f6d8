"""Pose-landmark and landmark-landmark covariance blocks (ps_covariance_cross_blocks, Problem.compute_marginal_covariances
(cross_pairs=...)) against the reference's covariance goldens, the numpy oracle's dense inverse and the per-column route
(ps_covariance_column), and their exactness: transposes, the marginals, repeated and chunked calls."""
import numpy as np
import pytest

from conftest import load_golden, golden_lp, golden_options
from oracle import gn_oracle as orc
from pyslam_amd import synthetic
from pyslam_amd._native import NativeError

pytestmark = pytest.mark.gpu

CHUNK = 32768                              # pairs per pass through the device buffer (ps_abi_cov.h: PS_COV_CROSS_CHUNK)


def device(lp):
    from pyslam_amd.device import DeviceProblem
    return DeviceProblem(lp)


def close(blk, ref, rel):
    return np.abs(blk - ref).max() <= rel * np.abs(ref).max()


def block(row, ka, kb, dof=6):
    da, db = (dof if ka == 0 else 3), (dof if kb == 0 else 3)
    assert not row[da * db:].any()
    return row[:da * db].reshape(da, db)


@pytest.mark.parametrize('name', ['ba_tiny_huber', 'stereo_ba_example'])
def test_cross_blocks_match_the_reference_covariance(name):
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
    low = problem._lower()
    poses = [k for k, r in zip(low.pose_keys, low.pose_rid) if r >= 0]
    points = [k for k, v in zip(low.point_keys, low.point_vid) if v >= 0]
    pairs = [(p, l) for p in poses for l in points] + [(l, p) for p in poses for l in points]
    ll = [(l1, l2) for l1 in points for l2 in points]
    if len(ll) > 400:
        rng = np.random.default_rng(0)
        ll = [ll[q] for q in rng.choice(len(ll), 400, replace=False)] + [(points[0], points[0]), (points[1], points[0])]
    pairs += ll
    out = problem.compute_marginal_covariances(keys=[], cross_pairs=pairs)
    assert set(out) == set(pairs)
    tol = 1e-9 * np.abs(ref).max()
    for ka, kb in pairs:
        ra, rb = part[ka], part[kb]
        assert out[(ka, kb)].shape == (len(ra), len(rb))
        assert np.abs(out[(ka, kb)] - ref[ra.start:ra.stop, rb.start:rb.stop]).max() <= tol, (ka, kb)


@pytest.fixture(scope='module')
def medium():
    """30 keyframes, 2 000 landmarks with tracks of 20 observations (longer than one 16-lane group), three constant poses,
    a tenth of the landmarks fixed (the problem of test_gpu_cov_marginals.py)."""
    lp, _ = synthetic.stereo_ba(num_kf=30, num_lm=2000, obs_per_lm=20, half_window=12, seed=7, const_point_fraction=0.1)
    lp.pose_rid[[11, 23]] = -1
    lp.pose_rid[lp.pose_rid >= 0] = np.arange(int((lp.pose_rid >= 0).sum()))
    lp.finalize()
    return lp


def _obs_pairs(lp):
    """(rid, vid) of every observation of a variable landmark on a variable pose."""
    rid = lp.pose_rid[lp.obs_pose]
    vid = lp.point_vid[lp.obs_point]
    keep = (rid >= 0) & (vid >= 0)
    return rid[keep].astype(np.int32), vid[keep].astype(np.int32)


def _spread(nr, nv, seed=0):
    """Pairs of all four kinds: (kind_a, a, kind_b, b) arrays."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(60):
        rows.append((0, rng.integers(nr), 1, rng.integers(nv)))
        rows.append((1, rng.integers(nv), 0, rng.integers(nr)))
        rows.append((1, rng.integers(nv), 1, rng.integers(nv)))
        rows.append((0, rng.integers(nr), 0, rng.integers(nr)))
    rows += [(1, 5, 1, 5), (1, nv - 1, 1, 0), (0, nr - 1, 1, nv - 1), (0, 0, 0, 0)]
    return tuple(np.array(c, dtype=np.int32) for c in zip(*rows))


def test_cross_blocks_match_the_oracle_inverse(medium):
    lp = medium
    P, _, _ = orc.normal_equations(lp, points_first=False)
    cov = np.linalg.inv(P.toarray())
    dev = device(lp)
    try:
        dev.covariance_begin()
        dev.covariance_marginals()
        nr, nv = dev.nr, dev.nv
        ka, a, kb, b = _spread(nr, nv)
        out = dev.covariance_cross_blocks(ka, a, kb, b)
        assert out.shape == (len(a), 36)

        def rng_of(kind, i):
            return slice(6 * i, 6 * i + 6) if kind == 0 else slice(6 * nr + 3 * i, 6 * nr + 3 * i + 3)
        for k in range(len(a)):
            ref = cov[rng_of(ka[k], a[k]), rng_of(kb[k], b[k])]
            assert close(block(out[k], ka[k], kb[k]), ref, 1e-9), (k, ka[k], a[k], kb[k], b[k])
    finally:
        dev.close()


def test_cross_blocks_are_exact(medium):
    lp = medium
    dev = device(lp)
    try:
        dev.covariance_begin()
        pose, point = dev.covariance_marginals()
        nr, nv = dev.nr, dev.nv
        ka, a, kb, b = _spread(nr, nv, seed=1)
        out = dev.covariance_cross_blocks(ka, a, kb, b)
        assert np.array_equal(out, dev.covariance_cross_blocks(ka, a, kb, b))              # two calls
        # (b, a) is the exact transpose of (a, b)
        back = dev.covariance_cross_blocks(kb, b, ka, a)
        for k in range(len(a)):
            assert np.array_equal(block(back[k], kb[k], ka[k]), block(out[k], ka[k], kb[k]).T), k
        # (l, l): the marginal, bit for bit
        v = np.arange(nv, dtype=np.int32)
        ones = np.ones(nv, dtype=np.int32)
        diag = dev.covariance_cross_blocks(ones, v, ones, v)
        assert np.array_equal(diag[:, :9].reshape(nv, 3, 3), point) and not diag[:, 9:].any()
        # pose-pose: covariance_pose_blocks, bit for bit
        pp = ka == 0
        pp &= kb == 0
        assert np.array_equal(out[pp, :36].reshape(-1, 6, 6), dev.covariance_pose_blocks(a[pp], b[pp]))
        # every observation's (pose, landmark) block twice over, more pairs than one chunk holds: one call = calls of any size
        rid, vid = _obs_pairs(lp)
        nobs = len(rid)
        rid, vid = np.tile(rid, 2), np.tile(vid, 2)
        assert len(rid) > CHUNK
        z, o = np.zeros_like(rid), np.ones_like(rid)
        whole = dev.covariance_cross_blocks(z, rid, o, vid)
        assert np.isfinite(whole).all() and not whole[:, 18:].any()
        assert np.array_equal(whole[:nobs], whole[nobs:])                  # (the second copy straddles a chunk boundary)
        cuts = [0, 1, 1000, CHUNK - 1, CHUNK + 5, len(rid)]
        parts = [dev.covariance_cross_blocks(z[s:e], rid[s:e], o[s:e], vid[s:e]) for s, e in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts), whole)
        rev = dev.covariance_cross_blocks(o[::-1], vid[::-1], z[::-1], rid[::-1])[::-1]
        assert np.array_equal(rev[:, :18].reshape(-1, 3, 6), np.transpose(whole[:, :18].reshape(-1, 6, 3), (0, 2, 1)))
        assert dev.covariance_cross_blocks([], [], [], []).shape == (0, 36)
    finally:
        dev.close()


def test_landmark_seen_only_by_constant_poses_has_zero_cross_blocks():
    lp, _ = synthetic.stereo_ba(num_kf=8, num_lm=120, obs_per_lm=2, half_window=1, seed=3)
    lp.pose_rid[[0, 1]] = -1
    lp.pose_rid[lp.pose_rid >= 0] = np.arange(int((lp.pose_rid >= 0).sum()))
    lp.finalize()
    on_var = np.zeros(lp.num_points, dtype=bool)
    on_var[lp.obs_point[lp.pose_rid[lp.obs_pose] >= 0]] = True
    lone = [int(lp.point_vid[p]) for p in range(lp.num_points) if not on_var[p] and lp.point_vid[p] >= 0]
    seen = [int(lp.point_vid[p]) for p in range(lp.num_points) if on_var[p] and lp.point_vid[p] >= 0]
    assert lone and seen
    dev = device(lp)
    try:
        dev.covariance_begin()
        pose, point = dev.covariance_marginals()
        v = lone[0]
        rows = [(0, r, 1, v) for r in range(dev.nr)] + [(1, v, 0, 0), (1, v, 1, seen[0]), (1, seen[0], 1, v), (1, v, 1, v)]
        ka, a, kb, b = (np.array(c, dtype=np.int32) for c in zip(*rows))
        out = dev.covariance_cross_blocks(ka, a, kb, b)
        assert not out[:-1].any()
        assert np.array_equal(out[-1, :9].reshape(3, 3), point[v]) and point[v].any()
    finally:
        dev.close()


def test_cross_blocks_errors():
    lp, _ = synthetic.stereo_ba(num_kf=6, num_lm=64, obs_per_lm=4, half_window=3, seed=1)
    dev = device(lp)
    try:
        with pytest.raises(NativeError, match='no dense inverse'):
            dev.covariance_cross_blocks([0], [0], [1], [0])
        dev.covariance_begin()
        with pytest.raises(NativeError, match='no dense inverse'):
            dev.covariance_cross_blocks([0], [0], [1], [0])
        dev.covariance_marginals()
        nr, nv = dev.nr, dev.nv
        assert np.isfinite(dev.covariance_cross_blocks([0, 1], [0, 3], [1, 1], [0, 7])).all()
        for bad, msg in [(([0], [nr], [1], [0]), 'reduced pose index'), (([0], [-1], [1], [0]), 'reduced pose index'),
                         (([0], [0], [1], [nv]), 'landmark index'), (([1], [-2], [1], [0]), 'landmark index'),
                         (([2], [0], [1], [0]), 'kind 2'), (([0], [0], [-1], [0]), 'kind -1')]:
            with pytest.raises(NativeError, match=msg):
                dev.covariance_cross_blocks(*bad)
        with pytest.raises(ValueError, match='differ in length'):
            dev.covariance_cross_blocks([0, 0], [0], [1], [0])
        dev.linearize(0.)                  # a linearisation ends the inverse's life
        with pytest.raises(NativeError, match='no dense inverse'):
            dev.covariance_cross_blocks([0], [0], [1], [0])
    finally:
        dev.close()
    # a pose graph (SE(2)): pose-pose pairs only, 3 x 3 in the leading entries
    lp, _ = synthetic.pose_graph(num_poses=20, num_loops=10, dof=3, seed=2, prior_first=True)
    dev = device(lp)
    try:
        dev.covariance_begin()
        pose, _ = dev.covariance_marginals()
        out = dev.covariance_cross_blocks([0, 0], [3, 7], [0, 0], [3, 1])
        assert np.array_equal(out[0, :9].reshape(3, 3), pose[3]) and not out[:, 9:].any()
        assert np.array_equal(out[1, :9].reshape(3, 3), dev.covariance_pose_blocks([7], [1])[0])
        with pytest.raises(NativeError, match='not SE\\(3\\)'):
            dev.covariance_cross_blocks([0], [0], [1], [0])
    finally:
        dev.close()


@pytest.fixture(scope='module')
def c3():
    lp, _ = synthetic.stereo_ba(200, 50000, 10, 20, seed=0)
    return lp


def test_c3_cross_blocks_match_the_column_route(c3):
    dev = device(c3)
    try:
        dev.covariance_begin()
        dev.covariance_marginals()
        nr, nv = dev.nr, dev.nv
        rid, vid = _obs_pairs(c3)
        z, o = np.zeros_like(rid), np.ones_like(rid)
        whole = dev.covariance_cross_blocks(z, rid, o, vid)
        assert whole.shape == (len(rid), 36) and np.isfinite(whole).all()
        # 16 landmarks spread over the track lengths: every pose that observes them and two that do not
        lm_len = np.bincount(c3.obs_point, minlength=c3.num_points)
        vid_len = np.zeros(nv, dtype=int)
        vid_len[c3.point_vid[c3.point_vid >= 0]] = lm_len[c3.point_vid >= 0]
        order = np.argsort(vid_len, kind='stable')
        for v in order[np.linspace(0, nv - 1, 16).astype(int)]:
            seen = sorted(set(rid[vid == v].tolist()))
            unseen = [r for r in (0, nr // 2, nr - 1) if r not in seen][:2]
            rs = np.array(seen + unseen, dtype=np.int32)
            out = dev.covariance_cross_blocks(np.zeros_like(rs), rs, np.ones_like(rs), np.full_like(rs, v))
            cols = np.stack([dev.covariance_column(1, int(v), c, tol=1e-13)[0] for c in range(3)], axis=2)   # (nr, 6, 3)
            for k, r in enumerate(rs):
                assert close(block(out[k], 0, 1), cols[r], 1e-8), (v, r)
            for k, r in enumerate(seen):         # the same blocks inside the all-observation call
                q = np.flatnonzero((vid == v) & (rid == r))[0]
                assert np.array_equal(whole[q], out[k])
    finally:
        dev.close()


def test_problem_api_cross_pairs(medium):
    from test_host_api import build_namespace
    lp = medium
    problem = synthetic.to_objects(lp, build_namespace())
    low = problem._lower()
    pkey = {int(r): k for k, r in zip(low.pose_keys, low.pose_rid) if r >= 0}
    lkey = {int(v): k for k, v in zip(low.point_keys, low.point_vid) if v >= 0}
    nr, nv = len(pkey), len(lkey)
    ka, a, kb, b = _spread(nr, nv, seed=2)
    name = lambda kind, i: pkey[int(i)] if kind == 0 else lkey[int(i)]          # noqa: E731
    pairs = list(dict.fromkeys((name(ka[k], a[k]), name(kb[k], b[k])) for k in range(len(a))))
    pairs += [(lkey[0], lkey[0]), (lkey[7], lkey[7])]
    pose_pairs = [(pkey[0], pkey[5]), (pkey[nr - 1], pkey[2])]
    alone = problem.compute_marginal_covariances(keys=[], pose_pairs=pose_pairs)
    out = problem.compute_marginal_covariances(pose_pairs=pose_pairs, cross_pairs=pairs)
    for pr in pose_pairs:
        assert np.array_equal(out[pr], alone[pr])
    dev = device(lp)
    try:
        dev.covariance_begin()
        dev.covariance_marginals()
        rows = dev.covariance_cross_blocks(ka, a, kb, b)
    finally:
        dev.close()
    for k in range(len(a)):
        pr = (name(ka[k], a[k]), name(kb[k], b[k]))
        assert np.array_equal(out[pr], block(rows[k], ka[k], kb[k])), pr
    for v in (0, 7):
        assert np.array_equal(out[(lkey[v], lkey[v])], out[lkey[v]])


def test_generic_route_cross_pairs_cubic():
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
    pairs = [('a', 'd'), ('c', 'b'), ('b', 'b')]
    out = problem.compute_marginal_covariances(keys=['a'], pose_pairs=[('a', 'd')], cross_pairs=pairs)
    tol = 1e-9 * np.abs(ref).max()
    for ka, kb in pairs:
        assert out[(ka, kb)].shape == (1, 1) and abs(out[(ka, kb)][0, 0] - ref['abcd'.index(ka), 'abcd'.index(kb)]) <= tol
    assert abs(out['a'][0, 0] - ref[0, 0]) <= tol
