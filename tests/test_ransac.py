"""Frame-to-frame RANSAC (reference pyslam/pipelines/ransac.py).

CPU: the numpy oracle against the golden vectors the verbatim reference produced.
GPU: the HIP path (through the C ABI and the reference-named Python classes) against both."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import ransac_oracle as orc

WELL = 1e-3          # sigma_2 / sigma_1 above which a 3-point hypothesis is well determined


def well_conditioned(g):
    return orc.sample_conditioning(g['pts_1'], g['pts_2'], g['rand_idx']) > WELL


def test_oracle_matches_reference_golden():
    g = load_golden('ransac')
    T_all, counts, best, mask = orc.perform_ransac(g['pts_1'], g['pts_2'], g['obs_2'], g['rand_idx'], g['cam'][:5],
                                                   float(g['thresh']))
    ok = well_conditioned(g)
    assert ok.sum() > 350
    assert np.abs(T_all[ok] - g['T_stacked'][ok]).max() < 1e-9
    assert np.array_equal(counts[ok], g['inlier_counts'][ok])
    assert np.allclose(T_all[best], g['T_best'], atol=1e-12)
    assert np.array_equal(np.where(mask)[0], g['inlier_indices'])
    # the winner is a real solution: close to the generating motion, and it rejects the planted outliers
    assert np.abs(g['T_best'] - g['T_true']).max() < 0.05
    assert not np.intersect1d(g['inlier_indices'], g['outliers']).size


def test_oracle_degenerate_samples_do_not_crash():
    g = load_golden('ransac')
    idx = np.array([[5, 5, 5], [1, 1, 7], [0, 1, 2]])
    T = orc.compute_transform(g['pts_1'][idx], g['pts_2'][idx])
    assert np.isfinite(T).all()
    assert np.allclose(T[0, :3, :3], np.identity(3))           # W = 0: LAPACK returns U = V = I


@pytest.mark.gpu
def test_device_hypotheses_match_reference_golden():
    from pyslam_amd.pipelines.ransac import FrameToFrameRANSAC, compute_transform_fast
    from pyslam.sensors import StereoCamera
    g = load_golden('ransac')
    cam = StereoCamera(*g['cam'][:5], int(g['cam'][5]), int(g['cam'][6]))
    r = FrameToFrameRANSAC(cam)
    r.set_obs(g['obs_1'], g['obs_2'])
    assert np.allclose(r.pts_1, g['pts_1'], rtol=1e-14) and np.allclose(r.pts_2, g['pts_2'], rtol=1e-14)
    T_best, mask, best, count, T_all, counts = r._device_ransac(g['rand_idx'], want_all=True)
    ok = well_conditioned(g)
    assert np.abs(T_all[ok] - g['T_stacked'][ok]).max() < 1e-9       # fp64 tolerance: different SVD algorithm
    assert np.array_equal(counts[ok], g['inlier_counts'][ok])
    assert best == int(np.argmax(g['inlier_counts'])) and count == len(g['inlier_indices'])
    assert np.abs(T_best - g['T_best']).max() < 1e-10
    assert np.array_equal(np.where(mask)[0], g['inlier_indices'])
    # the batch alignment entry point, broadcasting over leading dimensions like the guvectorize original
    T2 = compute_transform_fast(g['pts_1'][g['rand_idx']].reshape(20, 20, 3, 3), g['pts_2'][g['rand_idx']].reshape(20, 20, 3, 3))
    assert T2.shape == (20, 20, 4, 4) and np.array_equal(T2.reshape(-1, 4, 4), T_all)
    # scoring of caller-provided transforms
    masks = r.compute_ransac_cost(g['T_stacked'], r.pts_1, r.obs_2, cam, r.ransac_thresh)
    assert masks.shape == (400, 300) and np.array_equal(masks.sum(axis=1), g['inlier_counts'])


@pytest.mark.gpu
def test_perform_ransac_is_a_drop_in_under_the_same_seed():
    from pyslam.pipelines.ransac import FrameToFrameRANSAC
    from pyslam.sensors import StereoCamera
    g = load_golden('ransac')
    cam = StereoCamera(*g['cam'][:5], int(g['cam'][5]), int(g['cam'][6]))
    r = FrameToFrameRANSAC(cam)
    r.set_obs(g['obs_1'], g['obs_2'])
    np.random.seed(int(g['seed']))
    T_21, o1, o2, inl = r.perform_ransac()
    assert np.abs(T_21.as_matrix() - g['T_best']).max() < 1e-10
    assert np.array_equal(inl, g['inlier_indices'])
    assert np.array_equal(o1, g['obs_1_inliers']) and np.array_equal(o2, g['obs_2_inliers'])
    r.ransac_thresh = 1e-9
    with pytest.raises(ValueError):
        r.perform_ransac()


@pytest.mark.gpu
def test_device_many_points_alignment_and_degenerate_sets():
    """n-point alignment (n = 50) against the oracle; repeated / collinear minimal sets stay finite."""
    from pyslam_amd.pipelines.ransac import compute_transform_fast
    rng = np.random.default_rng(5)
    a = rng.standard_normal((7, 50, 3)) * 3.
    from liegroups import SE3
    b = np.stack([SE3.exp(0.3 * rng.standard_normal(6)).dot(a[k]) + 0.01 * rng.standard_normal((50, 3)) for k in range(7)])
    T = compute_transform_fast(a, b)
    assert np.abs(T - orc.compute_transform(a, b)).max() < 1e-12
    g = load_golden('ransac')
    idx = np.array([[5, 5, 5], [1, 1, 7], [0, 1, 2]])
    Td = compute_transform_fast(g['pts_1'][idx], g['pts_2'][idx])
    assert np.isfinite(Td).all()
    assert np.allclose(Td[0, :3, :3], np.identity(3))
    for k in range(3):                                           # always a proper rotation
        C = Td[k, :3, :3]
        assert np.allclose(C.dot(C.T), np.identity(3), atol=1e-12) and abs(np.linalg.det(C) - 1.) < 1e-12
    # a reflection-prone case (noisy, nearly planar sets): the det(U) det(V) correction
    flat = rng.standard_normal((4, 6, 3)) * np.array([1., 1., 1e-3])
    other = rng.standard_normal((4, 6, 3)) * np.array([1., 1., 1e-3])
    assert np.abs(compute_transform_fast(flat, other) - orc.compute_transform(flat, other)).max() < 1e-9


# ---- the conditions tests/test_gpu_ransac_edges.py relies on, for every committed seed and shape (tests/ransac_scenes.py) ----------

def edge_conditions(sc, idx, thresh=None):
    """Nothing in the margin and every sample determined -> the oracle's result."""
    import ransac_scenes as rs
    thresh = rs.THRESH if thresh is None else thresh
    ref = rs.f2f_oracle(sc, idx, thresh)
    assert not rs.in_margin(ref['err'], thresh).any()
    assert np.array_equal(ref['masks'][ref['finite']], orc.ransac_cost(ref['T_all'][ref['finite']], sc['pts_1'], sc['obs_2'], sc['cam5'], thresh))
    assert ref['cond'][ref['finite']].min() > rs.DETERMINED
    return ref


def test_edge_scenes_shape_sweep_has_nothing_in_the_margin():
    import ransac_scenes as rs
    assert sorted({n for n, h, _, _ in rs.F2F_SWEEP if h == 257}) == [3, 63, 64, 65, 255, 256, 257, 513]
    assert sorted({h for n, h, _, _ in rs.F2F_SWEEP if n == 257}) == [1, 2, 255, 256, 257, 513]
    for n, h, seed, sseed in rs.F2F_SWEEP:
        sc = rs.f2f_scene(n, seed)
        idx = rs.f2f_samples(n, h, 3, sseed)
        assert idx.shape == (h, 3) and all(np.unique(r).size == 3 for r in idx) and sc['bad'].size == int(0.2 * n)
        ref = edge_conditions(sc, idx)
        assert ref['counts'].max() > 0                           # (not the all-zero case: that one has its own test)
        assert (ref['cond'] > rs.WELL).sum() >= 0.9 * h          # the 1e-9 comparison of T_all covers nearly every row


def test_edge_scenes_ties_zero_counts_and_larger_sets():
    import ransac_scenes as rs
    sc = rs.f2f_scene(257, rs.F2F_SEED_257)
    idx = rs.f2f_samples(257, 257, 3, rs.F2F_SEED_257)
    ref = edge_conditions(sc, idx)
    w, l = rs.winner_and_loser(ref)
    assert rs.unique_winner(ref['counts']) and ref['cond'][w] > rs.WELL and ref['cond'][l] > rs.WELL
    assert ref['counts'][l] < ref['counts'][w] // 2              # clearly worse
    for h, positions in rs.TIE_POSITIONS:
        table = rs.tie_table(idx, w, l, h, positions)
        assert table.shape == (h, 3) and (table[list(positions)] == idx[w]).all() and (np.delete(table, positions, axis=0) == idx[l]).all()
    zero = edge_conditions(sc, idx, rs.ZERO_THRESH)
    assert not zero['counts'].any()
    for k, seed in rs.F2F_SEED_SETS.items():
        more = edge_conditions(sc, rs.f2f_samples(257, 257, k, seed))
        assert more['counts'].max() > 100


def test_edge_scenes_rgbd_and_non_finite_points():
    import ransac_scenes as rs
    sc = rs.f2f_scene(257, rs.F2F_SEED_RGBD, rgbd=True)
    assert sc['cam5'][4] == -1. and np.array_equal(sc['pts_1'][:, 2], sc['obs_1'][:, 2])
    ref = edge_conditions(sc, rs.f2f_samples(257, 257, 3, rs.F2F_SEED_RGBD))
    assert ref['counts'].max() > 100
    # the stereo formula on the same input counts differently: dropping the b < 0 branch cannot go unseen
    stereo = orc.ransac_cost(ref['T_all'], sc['pts_1'], sc['obs_2'], np.append(sc['cam5'][:4], 0.25), rs.THRESH)
    assert not np.array_equal(stereo.sum(axis=1), ref['counts'])
    sc, where = rs.f2f_nonfinite_scene()
    idx, rows = rs.f2f_nonfinite_samples(where)
    ref = edge_conditions(sc, idx)
    assert np.where(~ref['finite'])[0].tolist() == rows and not ref['counts'][rows].any()
    assert np.isinf(sc['pts_1'][where['inf_1']]).any() and np.isinf(sc['pts_2'][where['inf_2']]).any()
    assert np.isnan(sc['pts_2'][where['nan_2']]).any() and np.isnan(sc['pts_1'][where['nan_1']]).any()
    for k in ('inf_1', 'nan_2', 'nan_1', 'inf_2'):
        assert not ref['masks'][:, where[k]].any()
    assert rs.unique_winner(ref['counts']) and ref['finite'][ref['best']]
    # behind the camera after the motion, and an inlier all the same (no cheirality test in the reference)
    T = sc['T_true']
    assert (sc['pts_1'][where['behind']] @ T[:3, :3].T + T[:3, 3])[2] < 0.
    assert ref['masks'][ref['best'], where['behind']] and ref['masks'][:, where['behind']].sum() > 1
    T0, pts0 = rs.f2f_zero_depth_case(sc, ref)
    err = orc.reprojection_errors(T0, pts0, sc['obs_2'], sc['cam5'])
    assert not rs.in_margin(err).any() and not np.isfinite(err[0, 7:9]).any() and (err[1] < rs.THRESH).sum() > 100
    only = idx[rows]
    assert not rs.f2f_oracle(sc, only)['counts'].any()


def test_edge_scenes_units_and_offsets():
    import ransac_scenes as rs
    idx = rs.f2f_samples(65, 64, 3, rs.F2F_SEED_UNITS)
    unit = edge_conditions(rs.f2f_scene(65, rs.F2F_SEED_UNITS), idx)
    assert (unit['cond'] > rs.WELL).all() and unit['counts'].max() > 20
    for scale in rs.UNIT_SCALES:
        sc = rs.f2f_scene(65, rs.F2F_SEED_UNITS, scale=scale)
        ref = edge_conditions(sc, idx)
        assert np.array_equal(ref['masks'], unit['masks'])         # the pixel observations do not change with the unit
        assert np.abs(sc['pts_1']).max() > 10. * scale and (ref['cond'] > rs.WELL).all()
    moved = rs.f2f_offset_scene(rs.f2f_scene(65, rs.F2F_SEED_UNITS))
    ref = edge_conditions(moved, idx)
    assert moved['pts_1'].min() > 0.9 * rs.UNIT_OFFSET and (ref['cond'] > rs.WELL).all() and ref['counts'].max() > 20


def test_edge_scenes_conditioning_ladder_is_exact_in_binary():
    import ransac_scenes as rs
    assert abs(np.linalg.det(rs.LADDER_C) - 1.) < 1e-15 and np.array_equal(np.abs(rs.LADDER_C).sum(axis=0), np.ones(3))
    for n in (3, 6):
        for rung in rs.LADDER_RUNGS:
            p1, p2, ratio, s = rs.ladder_set(n, rung)
            assert p1.shape == (n, 3) and rs.ladder_is_exact(p1, p2)
            got = orc.sample_conditioning(p1, p2, np.arange(n)[None, :])[0]
            print('n = {}, rung {:.0e}: squeeze 2^{:d}, sigma_2 / sigma_1 = {:.2e}'.format(n, rung, int(np.log2(s)), got))
            assert rung / 3. <= got <= 3. * rung and abs(got - ratio) <= 1e-3 * ratio
            # the oracle itself finds the truth to eps / ratio
            err, floor = rs.ladder_error(orc.compute_transform(p1, p2))
            assert err <= max(floor, 100 * 2.2e-16 / ratio * 8.)
