"""Scenes, sample tables and oracle runs of the RANSAC edge tests (tests/test_gpu_ransac_edges.py on the device; the conditions
the device tests rely on -- nothing in the margin, a unique winner, determined samples -- are asserted without a device in
tests/test_ransac.py and tests/test_twoview_host.py, for every seed and shape listed here).  Plain functions, numpy only.

The margin rule (tests/test_gpu_twoview.py): a (hypothesis, point) pair whose oracle squared error lies within MARGIN relative of
the threshold may fall on either side on the device.  Every scene here is chosen so that the oracle has NO such pair, so masks
and counts are compared exactly."""
from fractions import Fraction

import numpy as np

from oracle import ransac_oracle as orc
from pyslam_amd import synthetic
from pyslam_amd.liegroups import SE3
from pyslam_amd.pipelines import epipolar as ep
from pyslam_amd.sensors import RGBDCamera, StereoCamera

THRESH = 5.0            # FrameToFrameRANSAC's default
MARGIN = 1e-6
WELL = 1e-3             # sigma_2 / sigma_1 above which T_all is held to 1e-9 (tests/test_ransac.py)
DETERMINED = 1e-6       # every committed sample is at least this well determined: T agrees to ~eps / DETERMINED = 2e-10, which
#                         moves a squared pixel error of ~5 by ~2 * sqrt(5) * 1000 px/m/m * 2e-10 / 5 m = 2e-7 relative at most
TIE_POSITIONS = [(513, (5, 261)), (257, (70, 5)), (257, (200, 64, 65)), (257, (255, 256)), (513, (512,)), (1000, (0, 999))]

# frame-to-frame: (N, H, scene seed, sample seed) of the shape sweep: every N at H = 257, every H at N = 257
F2F_SWEEP = [(3, 257, 1, 1)] + [(n, 257, 0, 0) for n in (63, 64, 65, 255, 256, 257, 513)] + \
            [(257, 1, 0, 5), (257, 2, 0, 1), (257, 255, 0, 0), (257, 256, 0, 0), (257, 513, 0, 0)]
F2F_SEED_257 = 0        # the N = 257 scene of the tie, zero-count, RGB-D, non-finite and larger-set tests
F2F_SEED_RGBD = 0
F2F_SEED_NONFINITE = 0
F2F_SEED_SETS = {4: 0, 6: 0}
F2F_SEED_UNITS = 0      # N = 65, H = 64
UNIT_SCALES = (1e-3, 1., 1e3, 1e6)
UNIT_OFFSET = 1e5
ZERO_THRESH = 1e-12

# two-view: (N, H, scene seed, sample seed)
TV_SWEEP = [(67, 255, 11, 5), (67, 257, 11, 5), (67, 513, 11, 5), (9, 64, 11, 5), (256, 64, 11, 5)]
TV_TIES = (67, 513, 11, 5)
TV_NONFINITE = (67, 64, 11, 5)


def in_margin(err, thresh=THRESH):
    with np.errstate(invalid='ignore'):
        return np.abs(err - thresh) <= MARGIN * thresh


# ---- frame-to-frame ------------------------------------------------------------------------------------------------------------

def f2f_camera(rgbd=False, scale=1.):
    cu, cv, fu, fv, b, w, h = synthetic.STEREO_BA_CAMERA
    return RGBDCamera(cu, cv, fu, fv, w, h) if rgbd else StereoCamera(cu, cv, fu, fv, b * scale, w, h)


def f2f_scene(n, seed, rgbd=False, scale=1.):
    """A tests/fuzz_small.py-style two-frame scene: n points in a 12 x 6 x 25 m box, a random motion, 0.2 px noise (RGB-D: 0.02 m
    on the depth), int(0.2 n) observations of frame 2 displaced by 20-60 px.  `scale` multiplies the points, the baseline and
    the translation; the pixel observations do not depend on it.  -> dict: cam, cam5, obs_1, obs_2, pts_1, pts_2 (triangulated
    as FrameToFrameRANSAC.set_obs does), T_true (4 x 4), bad (indices of the displaced observations)."""
    rng = np.random.default_rng([seed, n, int(rgbd)])
    unit = f2f_camera(rgbd)
    T = SE3.exp(0.1 * rng.standard_normal(6) * np.array([3, 1, 3, 0.3, 0.3, 0.3])).as_matrix()
    pts = np.stack([rng.uniform(-6, 6, n), rng.uniform(-3, 3, n), rng.uniform(5, 30, n)], axis=1)
    sigma = np.array([0.2, 0.2, 0.02 if rgbd else 0.2])
    obs_1 = np.atleast_2d(unit.project(pts)) + sigma * rng.standard_normal((n, 3))
    obs_2 = np.atleast_2d(unit.project(pts @ T[:3, :3].T + T[:3, 3])) + sigma * rng.standard_normal((n, 3))
    bad = rng.choice(n, int(0.2 * n), replace=False)
    obs_2[bad, :2] += rng.uniform(20, 60, (bad.size, 2)) * rng.choice([-1., 1.], (bad.size, 2))
    cam = f2f_camera(rgbd, scale)
    T = T.copy()
    T[:3, 3] *= scale
    return dict(cam=cam, cam5=cam.intrinsics(), obs_1=obs_1, obs_2=obs_2, pts_1=np.atleast_2d(cam.triangulate(obs_1)),
                pts_2=np.atleast_2d(cam.triangulate(obs_2)), T_true=T, bad=bad)


def f2f_offset_scene(sc, offset=UNIT_OFFSET):
    """`offset` added to every coordinate of both point sets of `sc`; frame 2 is observed again at the moved points (exactly,
    so that a transform which aligns the sets is scored by more than its rounding)."""
    out = dict(sc)
    out['pts_1'], out['pts_2'] = sc['pts_1'] + offset, sc['pts_2'] + offset
    out['obs_2'] = orc.project(out['pts_2'], sc['cam5'])
    return out


def f2f_samples(n, h, k, seed):
    """(h, k) int32 minimal sets, every row without repetition."""
    rng = np.random.default_rng([seed, n, h, k])
    return np.stack([rng.permutation(n)[:k] for _ in range(h)]).astype(np.int32)


def f2f_oracle(sc, idx, thresh=THRESH):
    """The oracle on the scene `sc` and the sample table `idx` -> dict: T_all, err (H, N squared errors), masks, counts, best,
    cond (sigma_2 / sigma_1 of every sample), finite (rows whose sample points are all finite; the others: T = NaN, count 0 --
    LAPACK refuses them)."""
    with np.errstate(all='ignore'):
        finite = np.isfinite(sc['pts_1'][idx]).all(axis=(1, 2)) & np.isfinite(sc['pts_2'][idx]).all(axis=(1, 2))
        T_all = np.full((len(idx), 4, 4), np.nan)
        cond = np.zeros(len(idx))
        if finite.any():
            T_all[finite] = orc.compute_transform(sc['pts_1'][idx[finite]], sc['pts_2'][idx[finite]])
            cond[finite] = orc.sample_conditioning(sc['pts_1'], sc['pts_2'], idx[finite])
        err = orc.reprojection_errors(T_all, sc['pts_1'], sc['obs_2'], sc['cam5'])
        masks = err < thresh
    counts = masks.sum(axis=1)
    return dict(T_all=T_all, err=err, masks=masks, counts=counts, best=int(np.argmax(counts)), cond=cond, finite=finite)


def unique_winner(counts):
    return int((counts == counts.max()).sum()) == 1


def winner_and_loser(ref):
    """(w, l): the oracle's best row and the determined row with the fewest inliers."""
    ok = np.where(ref['cond'] > WELL)[0] if 'cond' in ref else np.where(~ref['degenerate'])[0]
    return ref['best'], int(ok[np.argmin(ref['counts'][ok])])


def tie_table(rows, w, l, h, positions):
    """(h, k) table: row `l` of `rows` everywhere, row `w` at `positions`."""
    out = np.tile(rows[l], (h, 1))
    out[list(positions)] = rows[w]
    return np.ascontiguousarray(out, dtype=np.int32)


def f2f_nonfinite_scene(seed=F2F_SEED_NONFINITE):
    """The N = 257 scene with six planted points -> (scene, dict of their indices):
    inf_1: disparity 0 in obs_1 (pts_1 = inf);  inf_2: disparity 0 in obs_2 (pts_2 = inf, obs_2 finite);  nan_2: NaN in obs_2;
    nan_1: NaN in obs_1;  behind: negative disparity in obs_1, observed in frame 2 exactly where the true motion projects it
    (z < 0 after the transform: the reference has no cheirality test, such a point IS an inlier)."""
    sc = f2f_scene(257, seed)
    good = np.setdiff1d(np.arange(257), sc['bad'])
    where = dict(inf_1=int(good[3]), inf_2=int(good[40]), nan_2=int(good[77]), nan_1=int(good[120]), behind=int(good[200]))
    obs_1, obs_2 = sc['obs_1'].copy(), sc['obs_2'].copy()
    obs_1[where['inf_1'], 2] = 0.
    obs_2[where['inf_2'], 2] = 0.
    obs_2[where['nan_2'], 0] = np.nan
    obs_1[where['nan_1'], 1] = np.nan
    obs_1[where['behind'], 2] = -8.
    cam = sc['cam']
    with np.errstate(all='ignore'):
        p = np.atleast_2d(cam.triangulate(obs_1[where['behind']]))
        obs_2[where['behind']] = orc.project(p @ sc['T_true'][:3, :3].T + sc['T_true'][:3, 3], sc['cam5'])[0]
        sc.update(obs_1=obs_1, obs_2=obs_2, pts_1=np.atleast_2d(cam.triangulate(obs_1)), pts_2=np.atleast_2d(cam.triangulate(obs_2)))
    return sc, where


def f2f_nonfinite_samples(where, seed=F2F_SEED_NONFINITE):
    """H = 257 rows of 3: rows 0, 9, 130, 256 hold inf_1, inf_2, nan_2, nan_1; no other row holds a planted non-finite point
    (`behind` is finite and may be drawn).  -> (table, the four row numbers)."""
    idx = f2f_samples(257, 257, 3, seed)
    banned = [where[k] for k in ('inf_1', 'inf_2', 'nan_2', 'nan_1')]
    rng = np.random.default_rng([seed, 99])
    allowed = np.setdiff1d(np.arange(257), banned)
    for r in range(len(idx)):
        while np.isin(idx[r], banned).any():
            idx[r] = rng.choice(allowed, 3, replace=False)
    rows = [0, 9, 130, 256]
    for r, b in zip(rows, banned):
        idx[r, r % 3] = b
    return idx, rows


def f2f_zero_depth_case(sc, ref):
    """(T (2, 4, 4), pts_1) for compute_ransac_cost: the identity and the oracle's winner, over the scene's points with two of them
    moved to z = 0 exactly (one of them the origin): 1 / z = inf, 0 * inf = NaN."""
    pts = sc['pts_1'].copy()
    pts[7] = [1.0, -0.5, 0.0]
    pts[8] = [0.0, 0.0, 0.0]
    return np.stack([np.identity(4), ref['T_all'][ref['best']]]), pts


# ---- the conditioning ladder: an exactly known transform --------------------------------------------------------------------------

LADDER_RUNGS = (1., 1e-2, 1e-4, 1e-6, 1e-8, 1e-10)
LADDER_C = np.array([[0., -1., 0.], [0., 0., 1.], [-1., 0., 0.]])         # a signed permutation, det +1
LADDER_R = np.array([0.5, -2.25, 8.0])
_ORIGIN = np.array([1.5, -0.75, 6.0])
_AXES = np.array([[2., 1., 2.], [1., 2., -2.], [2., -2., -1.]])            # rows: three orthogonal directions of length 3
_LOCAL = {3: np.array([[-1., 0., 0.], [1., 0., 0.], [0., 1.75, 0.]]),      # (along the line, across, across) before the squeeze
          6: np.array([[-1., 0.5, -0.25], [1., -0.25, 0.5], [0.25, 1., -0.5], [-0.5, -1., -0.75], [0.75, -0.5, 1.], [-0.5, 0.25, 0.75]])}


def ladder_set(n, rung):
    """(pts_1, pts_2, sigma_2 / sigma_1, squeeze) of the n-point set (n = 3, 6) of one rung: dyadic coordinates
    origin + x a_1 + s (y a_2 + z a_3) with s the power of two whose sigma_2 / sigma_1 comes closest to `rung`, and
    pts_2 = LADDER_C pts_1 + LADDER_R, exact in binary (ladder_is_exact)."""
    best = None
    for m in range(0, 20):
        s = 2. ** -m
        p1 = _ORIGIN + (_LOCAL[n] * np.array([1., s, s])) @ _AXES
        q = p1 - p1.mean(axis=0)
        sv = np.linalg.svd(q.T @ q, compute_uv=False)
        ratio = sv[1] / sv[0]
        if best is None or abs(np.log(ratio / rung)) < abs(np.log(best[2] / rung)):
            best = (p1, p1 @ LADDER_C.T + LADDER_R, ratio, s)
    return best


def ladder_truth():
    T = np.identity(4)
    T[:3, :3], T[:3, 3] = LADDER_C, LADDER_R
    return T


def ladder_is_exact(p1, p2):
    """pts_2 == C pts_1 + r in rational arithmetic (no rounding went into the inputs)."""
    F = np.vectorize(Fraction, otypes=[object])
    want = F(p1) @ F(LADDER_C).T + F(LADDER_R)
    return bool((F(p2) == want).all())


def ladder_error(T):
    """(error to the truth, floor): max |T - T_true| over the entries; 16 ulps of the largest entry of T_true."""
    Tt = ladder_truth()
    return float(np.abs(T - Tt).max()), 16. * float(np.spacing(np.abs(Tt).max()))


# ---- two-view -------------------------------------------------------------------------------------------------------------------

TV_THRESH = 4.0
TV_CAM = np.array(synthetic.TWO_VIEW_CAMERA[:4] + (-2.,))


def tv_samples(n, h, seed):
    """The sample tables of tests/test_gpu_twoview.py (its samples_of, imported when called: that module needs no device to load)."""
    from test_gpu_twoview import samples_of
    return samples_of(n, h, seed)


def tv_scene(n, seed):
    obs_1, obs_2, T, outlier = synthetic.two_view(num_pts=n, seed=seed)
    return obs_1, obs_2


def tv_nonfinite_scene():
    """The N = 67 scene with a NaN row in obs_1, an inf row in obs_2 and a NaN coordinate in obs_2 (inliers of the motion before)
    -> (obs_1, obs_2, their indices)."""
    n, h, seed, sseed = TV_NONFINITE
    obs_1, obs_2, T, outlier = synthetic.two_view(num_pts=n, seed=seed)
    good = np.where(~outlier)[0]
    planted = [int(good[2]), int(good[20]), int(good[41])]
    obs_1, obs_2 = obs_1.copy(), obs_2.copy()
    obs_1[planted[0]] = np.nan
    obs_2[planted[1]] = np.inf
    obs_2[planted[2], 1] = np.nan
    return obs_1, obs_2, planted


def tv_nonfinite_samples(planted):
    """H = 64 rows of 8: rows 0, 31, 63 hold one planted point each, no other row does -> (table, those rows)."""
    n, h, seed, sseed = TV_NONFINITE
    idx = tv_samples(n, h, sseed)
    rs = np.random.RandomState(sseed + 1)
    allowed = np.setdiff1d(np.arange(n), planted)
    for r in range(h):
        if np.isin(idx[r], planted).any():
            idx[r] = rs.choice(allowed, 8, replace=False)
    rows = [0, 31, 63]
    for r, p in zip(rows, planted):
        idx[r, r % 8] = p
    return idx, rows


def tv_oracle(obs_1, obs_2, samples, refit=True):
    """epipolar.ransac with the pairs in the margin counted: -> (result dict, number of (hypothesis, point) pairs in the margin
    over all hypotheses, the raw winner and the refit, worst sigma_8 / sigma_1 over the samples that are not degenerate)."""
    with np.errstate(all='ignore'):
        ref = ep.ransac(obs_1, obs_2, TV_CAM, samples, TV_THRESH, refit_winner=refit)
        x1, x2 = ep.normalise(obs_1, TV_CAM), ep.normalise(obs_2, TV_CAM)
        near = int(in_margin(ref['dist'], TV_THRESH).sum() + in_margin(ref['d'], TV_THRESH).sum() + in_margin(ref['d_raw'], TV_THRESH).sum())
        if ref['d_refit'] is not None:
            near += int(in_margin(ref['d_refit'], TV_THRESH).sum())
        sig = [ep.eight_point(x1, x2, s)[2] for s in samples]
    ratios = [s[7] / s[0] for s, d in zip(sig, ref['degenerate']) if s is not None and not d]
    return ref, near, (min(ratios) if ratios else np.inf)
