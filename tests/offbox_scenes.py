"""Scenes of the off-box linearisation tests (tests/test_offbox_host.py, tests/test_gpu_offbox.py): synthetic.stereo_ba moved out of
the box it draws from (x +-8 m, y +-3 m, z 6-30 m, one camera, one observation group) -- landmarks nearer and farther, lengths in
millimetres, landmark blocks of every magnitude in one wave, three camera types and several losses in one wave, group ids with
the sign bit of the observation record's group byte set, one stiffness per observation -- and the checks that the scenes are what
they say.  Every scene keeps stereo_ba's constants: the held first pose and a fraction of constant landmarks."""
import functools

import numpy as np

from pyslam_amd import lowering, synthetic
from pyslam_amd.lowering import pose_rows_to_matrices
from pyslam_amd.utils import invsqrt

PIXEL_NOISE = 0.3
# the shape whose fp64-against-long-double figures are tabulated (EXPECTED_E64 below), and the shape the device tests use: nine
# keyframes (eight variable: two 256-row pose items each), 600 landmarks of six observations (61 packed waves, 16 workgroups)
TABLE_SHAPE = dict(num_kf=6, num_lm=120, obs_per_lm=4, half_window=3, seed=3)
GPU_SHAPE = dict(num_kf=9, num_lm=600, obs_per_lm=6, half_window=4, seed=3)
CONST_POINT_FRACTION = 0.05

DEPTH_FACTOR = dict(near=0.08, base=1., far10=10., far100=100.)
DEPTH_SCENES = ('near', 'base', 'far10', 'far100')
MIXED_SCENES = ('mixed_wave', 'high_group_ids', 'wide_mixed')
SCENES = DEPTH_SCENES + ('mm', 'mixed_depth') + MIXED_SCENES
# camera-frame z (m) and observed disparity (px) per depth scene: 6-30 m times the factor (the cameras sit within half a metre of
# the origin), 250 / z px and 3.5 sigma of the disparity noise (0.3 sqrt(2) px) to either side
Z_RANGE = dict(near=(0.4, 2.5), base=(5.5, 30.5), far10=(59., 301.), far100=(599., 3010.))
DISPARITY_RANGE = dict(near=(98., 630.), base=(6.5, 47.), far10=(-0.7, 5.8), far100=(-1.5, 1.9))
# the distance of an fp64 landmark elimination from the same elimination in long double on TABLE_SHAPE, largest difference over the
# largest entry of (S, g): measured on the host when these scenes were written; tests/test_offbox_host.py reproduces them within
# a factor 3
EXPECTED_E64 = dict(near=(4.7e-16, 1.4e-15), base=(7.1e-15, 1.5e-13), far10=(6.0e-13, 6.2e-12), far100=(8.7e-11, 1.7e-9),
                    mm=(1.2e-14, 6.0e-15))

HIGH_IDS = (5, 127, 128, 200, 253, 254)          # where high_group_ids puts mixed_wave's six groups in a table of 255 rows


def _base(shape):
    return synthetic.stereo_ba(const_point_fraction=CONST_POINT_FRACTION, **dict(shape))


def _camera_points(lp, truth_poses, pts_true):
    T = truth_poses[lp.obs_pose]
    return np.einsum('nij,nj->ni', T[:, :3, :3], pts_true[lp.obs_point]) + T[:, :3, 3]


def _reproject(lp, truth_poses, pts_true, seed):
    """Observations of the true points from the true poses through the scene's (stereo) camera, PIXEL_NOISE px of seeded noise
    (the disparity's sigma sqrt(2) times that, as stereo_ba has it)."""
    rng = np.random.default_rng([seed, 11])
    noise = PIXEL_NOISE * rng.standard_normal((lp.num_obs, 3)) * np.sqrt([1., 1., 2.])
    return synthetic._project(lp.cams[0], _camera_points(lp, truth_poses, pts_true)) + noise


def _moved(shape, factor):
    """stereo_ba with the start of landmark j multiplied by factor[j], the poses kept, and the observations re-projected from that
    start itself: the scene is linearised PIXEL_NOISE px from a point that explains its observations exactly (residuals of the noise's
    size: what the last iterations of a solve see), at any depth.  truth: that start."""
    lp, _ = _base(shape)
    factor = np.broadcast_to(np.asarray(factor, dtype=float), (lp.num_points,))
    out = lp.copy()
    out.points = lp.points * factor[:, None]
    truth = dict(poses=pose_rows_to_matrices(lp.poses, 6), points=out.points.copy())
    out.obs_uvd = _reproject(lp, truth['poses'], truth['points'], shape['seed'])
    return out.finalize(), truth


def _mixed_depth_factors(shape):
    return np.random.default_rng([shape['seed'], 12]).choice([0.08, 1., 10., 100.], size=shape['num_lm'])


# ---------------------------------------------------------------------------
# three cameras x two stiffnesses, four losses: the six groups of mixed_wave
# ---------------------------------------------------------------------------
def _mixed_tables(cam5):
    """(cams (3, 5), stiff3 (6, 9), obs_groups (6, 4)): stereo, RGB-D (b = -1: the third coordinate is z in metres) and monocular
    (b = -2: third stiffness row and column zero); per camera one diagonal and one non-diagonal stiffness; L2, Huber, Cauchy and
    L1 -- the last on a monocular group, whose dead third row has the weight NaN on the host."""
    rgbd, mono = cam5.copy(), cam5.copy()
    rgbd[4], mono[4] = -1., -2.
    Sd = invsqrt(np.diagflat([1., 1., 2.]))
    Sn = invsqrt(np.array([[1.2, 0.3, 0.1], [0.3, 0.9, -0.2], [0.1, -0.2, 2.5]]))
    Zd = np.diag([1., 1., 40.])                                   # depth noise 25 mm
    Zn = invsqrt(np.array([[1.1, -0.2, 0.004], [-0.2, 1.3, 0.003], [0.004, 0.003, 6e-4]]))
    Md, Mn = np.zeros((3, 3)), np.zeros((3, 3))
    Md[:2, :2] = np.identity(2)
    Mn[:2, :2] = invsqrt(np.array([[1.4, 0.5], [0.5, 0.8]]))
    stiff = np.stack([Sd, Sn, Zd, Zn, Md, Mn]).reshape(6, 9)
    # (Huber's and Cauchy's k inside the residuals' spread, PIXEL_NOISE px: both branches of the weight occur)
    groups = np.array([[0., 0., 0., 0.],            # stereo, diagonal,     L2
                       [0., 1., 3., 0.3],           # stereo, non-diagonal, Huber
                       [1., 2., 2., 0.5],           # RGB-D,  diagonal,     Cauchy
                       [1., 3., 3., 0.3],           # RGB-D,  non-diagonal, Huber
                       [2., 4., 1., 0.],            # mono,   diagonal,     L1
                       [2., 5., 3., 0.3]])          # mono,   non-diagonal, Huber
    return np.stack([cam5, rgbd, mono]), stiff, groups


def _mixed_wave(shape):
    lp, truth = _moved(shape, 1.)
    out = lp.copy()
    out.cams, out.stiff3, out.obs_groups = _mixed_tables(lp.cams[0])
    rng = np.random.default_rng([shape['seed'], 13])
    grp = rng.integers(0, 6, size=lp.num_obs).astype(np.int32)
    cam = out.obs_groups[grp, 0].astype(int)
    pc = _camera_points(lp, truth['poses'], truth['points'])
    uvd = out.obs_uvd.copy()
    uvd[cam == 1, 2] = pc[cam == 1, 2] + 0.025 * rng.standard_normal(np.count_nonzero(cam == 1))
    uvd[cam == 2, 2] = 0.
    out.obs_uvd, out.obs_grp = uvd, grp
    return out.finalize(), truth


def _high_group_ids(shape):
    """mixed_wave's rows, the group table padded to 255 rows (copies of its first row: valid, unused) and the six groups moved
    to HIGH_IDS -- from 128 on the group byte of the observation record has its top bit set."""
    lp, truth = _mixed_wave(shape)
    out = lp.copy()
    table = np.tile(lp.obs_groups[0], (lowering.MAX_OBS_GROUPS, 1))
    ids = np.array(HIGH_IDS)
    table[ids] = lp.obs_groups
    out.obs_groups, out.obs_grp = table, ids[lp.obs_grp].astype(np.int32)
    return out.finalize(), truth


def _wide_mixed(shape):
    """mixed_wave's rows with one group row and one stiffness per observation (more than 255 rows: the device groups become the
    six (camera, loss) classes, the stiffness a per-observation index): the class's stiffness times a seeded factor in 0.5-1.5."""
    lp, truth = _mixed_wave(shape)
    out = lp.copy()
    n = lp.num_obs
    g = lp.obs_groups[lp.obs_grp]
    scale = 0.5 + np.random.default_rng([shape['seed'], 14]).random(n)
    out.stiff3 = lp.stiff3[g[:, 1].astype(int)] * scale[:, None]
    out.obs_groups = np.column_stack([g[:, 0], np.arange(n, dtype=float), g[:, 2], g[:, 3]])
    out.obs_grp = np.arange(n, dtype=np.int32)
    return out.finalize(), truth


def _mm(shape):
    """stereo_ba itself with every length times 1000 (pose translations, landmarks, the baseline); the pixels -- its own
    observations, a pixel of noise around its true scene -- unchanged.  truth: stereo_ba's, in millimetres."""
    lp, truth = _base(shape)
    out = lp.copy()
    out.poses = lp.poses.copy()
    out.poses[:, 9:] *= 1000.
    out.points = lp.points * 1000.
    out.cams = lp.cams.copy()
    out.cams[:, 4] *= 1000.
    poses = truth['poses'].copy()
    poses[:, :3, 3] *= 1000.
    return out.finalize(), dict(poses=poses, points=truth['points'] * 1000.)


@functools.lru_cache(maxsize=None)
def _scene(name, shape_items):
    shape = dict(shape_items)
    if name in DEPTH_FACTOR:
        return _moved(shape, DEPTH_FACTOR[name])
    if name == 'mixed_depth':
        return _moved(shape, _mixed_depth_factors(shape))
    return dict(mm=_mm, mixed_wave=_mixed_wave, high_group_ids=_high_group_ids, wide_mixed=_wide_mixed)[name](shape)


def scene(name, shape=None):
    """-> (LoweredProblem, truth dict).  Built once per (name, shape): callers must leave the tables unchanged."""
    return _scene(name, tuple(sorted((shape or GPU_SHAPE).items())))


# ---------------------------------------------------------------------------
# scene checks (asserted on the host: tests/test_offbox_host.py)
# ---------------------------------------------------------------------------
def device_class(lp):
    """What the lanes of a wave agree or disagree about: the group row -- with more than 255 rows (wide) the (camera, loss) class."""
    if lp.obs_groups.shape[0] <= lowering.MAX_OBS_GROUPS:
        return lp.obs_grp.astype(np.int64)
    key = lp.obs_groups[lp.obs_grp][:, [0, 2, 3]]
    return np.unique(key, axis=0, return_inverse=True)[1].reshape(-1).astype(np.int64)


def observation_orders(lp):
    """The observation lists the two passes walk: by landmark (variable landmarks by vid, then the constant ones; stable) and, for the
    rows on variable poses, by reduced pose."""
    vid = lp.point_vid[lp.obs_point].astype(np.int64)
    by_landmark = np.argsort(np.where(vid >= 0, vid, lp.num_var_points + lp.obs_point.astype(np.int64)), kind='stable')
    rid = lp.pose_rid[lp.obs_pose]
    on_var = np.flatnonzero(rid >= 0)
    by_pose = on_var[np.argsort(rid[on_var], kind='stable')]
    return by_landmark, by_pose


def min_distinct_per_run(values, run=64):
    """The smallest number of distinct values in any `run` consecutive entries."""
    values = np.asarray(values)
    if values.size < run:
        return int(np.unique(values).size)
    win = np.lib.stride_tricks.sliding_window_view(values, run)
    s = np.sort(win, axis=1)
    return int((1 + np.count_nonzero(np.diff(s, axis=1), axis=1)).min())


def min_classes_per_wave(lp):
    cls = device_class(lp)
    return min(min_distinct_per_run(cls[order]) for order in observation_orders(lp))


def landmarks_with_all_cameras(lp):
    cam = lp.obs_groups[lp.obs_grp, 0].astype(int)
    seen = np.zeros((lp.num_points, 3), dtype=bool)
    seen[lp.obs_point, np.minimum(cam, 2)] = True
    return np.flatnonzero(seen.all(axis=1) & (lp.point_vid >= 0))


def depth_and_disparity(lp, truth):
    """((z min, z max) of the true points in their cameras, (min, max) of the observed third coordinate)."""
    z = _camera_points(lp, truth['poses'], truth['points'])[:, 2]
    return (float(z.min()), float(z.max())), (float(lp.obs_uvd[:, 2].min()), float(lp.obs_uvd[:, 2].max()))


def underdetermined(lp):
    return lowering.underdetermined_mono_points(lp.cams, lp.obs_groups, lp.obs_grp, lp.obs_point, lp.point_vid)
