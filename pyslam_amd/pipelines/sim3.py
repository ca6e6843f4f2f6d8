"""Similarity (Sim(3)) alignment of two matched 3-D point sets on the device: what relates a monocular map, whose scale is fixed
only by |t_21| = 1 at its bootstrap, to anything else -- a ground-truth trajectory (``align_trajectories``), a second map of the same
place (``align_maps``), another keyframe that sees the same landmarks (the geometric half of a loop closure).

The reference has no counterpart (it has no monocular map); the definition is this project's own, stated in csrc/ps_k_sim3.h and
restated by pipelines/similarity.py.  ``Sim3RANSAC`` is shaped like PnPRANSAC: the random minimal sets (three pairs) are drawn on the
host with ``np.random`` (so a seeded run picks the same hypotheses), everything else -- the Umeyama fit of every sample, the scoring of
every hypothesis over every pair, the arg-max, the refit rounds over the inliers -- is one call into the HIP core (ps_sim3_ransac).
There is no CPU path.

With a camera the pairs are scored in pixels, in both images (pts_1 in the frame of camera 1, pts_2 in the frame of camera 2);
without one, in the units of pts_2, and the threshold has to come from the caller."""
import numpy as np

from pyslam_amd import _native as nat
from pyslam_amd.pipelines.pnp import _pts3
from pyslam_amd.pipelines.ransac import _cam5
from pyslam_amd.pipelines.twoview import _obs2

REASONS = ('exhausted', 'lower count', 'fixed point', 'degenerate')         # info[4] of ps_sim3_ransac


def _se3(R, t):
    from pyslam_amd.liegroups import SE3
    T = np.identity(4)
    T[:3, :3], T[:3, 3] = R, t
    return SE3.from_matrix(T, normalize=True)


def _u8p(a):
    return None if a is None else a.ctypes.data_as(nat.c_u8p)


class Sim3RANSAC:
    def __init__(self, camera=None):
        self.camera = camera
        self.ransac_iters = 400
        self.ransac_thresh = 9.0 if camera is not None else None  # (3 px)**2 on the larger of the two squared reprojection errors
        self.num_min_set_pts = 3
        self.min_inliers = 12
        self.refit_iters = 3
        self.fixed_scale = False

    def set_obs(self, pts_1, pts_2, obs_1=None, obs_2=None):
        """Matched points (N, 3) each and, with a camera, their pixels in their own images (default: their own projections)."""
        p1, p2 = _pts3(pts_1, 'pts_1'), _pts3(pts_2, 'pts_2')
        if p1.shape[0] != p2.shape[0]:
            raise ValueError("pts_1 and pts_2 must hold the same number of points, got {} and {}".format(p1.shape[0], p2.shape[0]))
        if self.camera is None:
            if obs_1 is not None or obs_2 is not None:
                raise ValueError("Sim3RANSAC: observations need a camera (without one the pairs are scored in the units of pts_2)")
            o1 = o2 = None
        else:
            cam = _cam5(self.camera)
            o1, o2 = (self._project(cam, p) if o is None else _obs2(o, name)
                      for p, o, name in ((p1, obs_1, 'obs_1'), (p2, obs_2, 'obs_2')))
            if o1.shape[0] != p1.shape[0] or o2.shape[0] != p1.shape[0]:
                raise ValueError("obs_1 and obs_2 must hold one row per point")
        self.pts_1, self.pts_2, self.obs_1, self.obs_2 = p1, p2, o1, o2
        self.num_pts = p1.shape[0]

    @staticmethod
    def _project(cam, p):
        with np.errstate(all='ignore'):
            return np.ascontiguousarray(np.stack([cam[2] * p[:, 0] / p[:, 2] + cam[0], cam[3] * p[:, 1] / p[:, 2] + cam[1]], axis=1))

    def draw_samples(self):
        """(ransac_iters, 3) indices, every row without repetition, from ``np.random``: one ``randint`` table, and the rows that
        repeat an index drawn again until none is left."""
        H, N = int(self.ransac_iters), self.num_pts
        if N < 3:
            raise ValueError("Sim3RANSAC: a row of three different indices needs at least 3 points, got {}".format(N))
        idx = np.random.randint(0, N, (H, 3))
        while True:
            bad = (idx[:, 0] == idx[:, 1]) | (idx[:, 0] == idx[:, 2]) | (idx[:, 1] == idx[:, 2])
            if not bad.any():
                return idx.astype(np.int32)
            idx[bad] = np.random.randint(0, N, (int(bad.sum()), 3))

    def _thresh(self):
        if self.ransac_thresh is None:
            raise ValueError("Sim3RANSAC: without a camera ransac_thresh (squared distance in the units of pts_2) has to be set")
        return float(self.ransac_thresh)

    def perform_ransac(self):
        """(scale, T_21: SE3 of (R, t), inlier_indices) with p_2 = scale R p_1 + t; ValueError below ``min_inliers`` inliers or 3
        points.  The counts, the refit's course and every pair's error stay on the object (info_)."""
        if self.num_min_set_pts != 3:
            raise ValueError("Sim3RANSAC: the minimal solver takes three pairs (num_min_set_pts = 3)")
        if self.num_pts < 3:
            raise ValueError("Sim3RANSAC: a similarity needs at least 3 correspondences, got {}".format(self.num_pts))
        self._thresh()
        nat.require_gpu()
        res = self._device_ransac(self.draw_samples())
        self.info_ = res
        if res['count'] < self.min_inliers or res['degenerate']:
            raise ValueError("Sim3RANSAC failed to find {} inliers (found {}). Try adjusting the thresholds.".format(
                self.min_inliers, res['count']))
        s = res['scale']
        return s, _se3(res['S_21'][:3, :3] / s, res['S_21'][:3, 3]), np.where(res['mask'])[0]

    def _samples(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.ndim != 2 or idx.shape[1] != 3:
            raise ValueError("the sample table must have shape (H, 3)")
        return idx

    def _cam(self):
        return None if self.camera is None else _cam5(self.camera)

    def _device_ransac(self, idx):
        idx = self._samples(idx)
        N = self.num_pts
        S, scale = np.zeros((4, 4)), np.zeros(1)
        mask, info, sq_err = np.zeros(N, dtype=np.uint8), np.zeros(8, dtype=np.int32), np.zeros(N)
        nat.check(nat.load().ps_sim3_ransac(
            nat.f64p(self.pts_1), nat.f64p(self.pts_2), nat.f64p(self.obs_1), nat.f64p(self.obs_2), N, nat.i32p(idx), idx.shape[0],
            nat.f64p(self._cam()), self._thresh(), int(self.fixed_scale), int(self.refit_iters), nat.f64p(S), nat.f64p(scale), _u8p(mask),
            nat.i32p(info), nat.f64p(sq_err)))
        return dict(S_21=S, scale=float(scale[0]), mask=mask.astype(bool), best=int(info[0]), raw_count=int(info[1]), count=int(info[2]),
                    rounds=int(info[3]), reason=int(info[4]), degenerate=bool(info[5]), d=sq_err)

    def _device_hypotheses(self, idx):
        """Every sample's (S_all (H, 4, 4), scales (H,), counts (H,), flags (H,) bool): what the tests hold against the restatement."""
        idx = self._samples(idx)
        H = idx.shape[0]
        S, scales, counts, flags = np.zeros((H, 4, 4)), np.zeros(H), np.zeros(H, dtype=np.int32), np.zeros(H, dtype=np.uint8)
        nat.check(nat.load().ps_sim3_hypotheses(
            nat.f64p(self.pts_1), nat.f64p(self.pts_2), nat.f64p(self.obs_1), nat.f64p(self.obs_2), self.num_pts, nat.i32p(idx), H,
            nat.f64p(self._cam()), self._thresh(), int(self.fixed_scale), nat.f64p(S), nat.f64p(scales), nat.i32p(counts), _u8p(flags)))
        return S, scales, counts, flags.astype(bool)

    def compute_ransac_cost(self, S_stacked, pts_1, pts_2, obs_1, obs_2, camera, thresh):
        """Boolean inlier mask (num_models, num_pts) of given models S (4 x 4 each); camera None: the metric mode (no observations)."""
        nat.require_gpu()
        S = np.ascontiguousarray(S_stacked, dtype=np.float64).reshape(-1, 4, 4)
        p1, p2 = _pts3(pts_1, 'pts_1'), _pts3(pts_2, 'pts_2')
        if p1.shape[0] != p2.shape[0]:
            raise ValueError("pts_1 and pts_2 must hold the same number of points")
        o1 = o2 = cam = None
        if camera is not None:
            o1, o2, cam = _obs2(obs_1, 'obs_1'), _obs2(obs_2, 'obs_2'), _cam5(camera)
        masks = np.zeros((S.shape[0], p1.shape[0]), dtype=np.uint8)
        nat.check(nat.load().ps_sim3_score(nat.f64p(S), S.shape[0], nat.f64p(p1), nat.f64p(p2), nat.f64p(o1), nat.f64p(o2), p1.shape[0],
                                           nat.f64p(cam), float(thresh), _u8p(masks), None))
        return masks.astype(bool)


def align_maps(camera, pts_1, pts_2, obs_1=None, obs_2=None, seed=None, ransac=None):
    """Matched landmarks of two maps (pts_1 in the frame of keyframe 1 of the first, pts_2 in the frame of keyframe 2 of the second)
    -> (scale, T_21: SE3, inlier_indices) with p_2 = scale R p_1 + t.  Runs Sim3RANSAC (``seed``: seeds ``np.random`` first;
    ``ransac``: a configured Sim3RANSAC to use instead of a default one; ``camera`` None: the metric mode, whose threshold only a
    configured Sim3RANSAC carries).  ValueError below ``min_inliers`` inliers."""
    rs = ransac if ransac is not None else Sim3RANSAC(camera)
    rs.set_obs(pts_1, pts_2, obs_1, obs_2)
    if seed is not None:
        np.random.seed(seed)
    return rs.perform_ransac()


def _centres(poses, convention):
    if convention not in ('Twv', 'Tvw'):
        raise ValueError('convention must be \'Tvw\' or \'Twv\'')
    M = np.stack([T.as_matrix() if hasattr(T, 'as_matrix') else np.asarray(T, dtype=np.float64) for T in poses]).reshape(-1, 4, 4)
    if convention == 'Twv':
        return np.ascontiguousarray(M[:, :3, 3])
    return np.ascontiguousarray(-np.einsum('nji,nj->ni', M[:, :3, :3], M[:, :3, 3]))


def align_trajectories(poses_est, poses_gt, convention='Twv'):
    """The similarity that carries the estimated trajectory onto the ground truth: plain Umeyama alignment of all camera centres
    (c_gt = scale R c_est + t), on the device -- ps_sim3_ransac in the metric mode with an infinite threshold and the one hypothesis
    of the first, the middle and the last pose, whose refit round fits every centre.  ``convention`` as TrajectoryMetrics: 'Twv'
    poses are vehicle-to-world, 'Tvw' world-to-vehicle.  -> (scale, T: SE3).  ValueError for fewer than 3 poses or centres on a line."""
    c_est, c_gt = _centres(poses_est, convention), _centres(poses_gt, convention)
    n = min(c_est.shape[0], c_gt.shape[0])
    if n < 3:
        raise ValueError("align_trajectories: a similarity needs at least 3 poses, got {}".format(n))
    rs = Sim3RANSAC()
    rs.ransac_thresh, rs.refit_iters = np.inf, 1
    rs.set_obs(c_est[:n], c_gt[:n])
    nat.require_gpu()
    res = rs._device_ransac(np.array([[0, n // 2, n - 1]], dtype=np.int32))
    if res['degenerate'] or res['rounds'] != 1:
        raise ValueError("align_trajectories: the camera centres do not determine a similarity (on a line, or not finite)")
    s = res['scale']
    return s, _se3(res['S_21'][:3, :3] / s, res['S_21'][:3, 3])


def invert(scale, T):
    """The inverse similarity of (scale, T): p_1 = (1 / scale) R^T p_2 - R^T t / scale."""
    M = T.as_matrix() if hasattr(T, 'as_matrix') else np.asarray(T, dtype=np.float64)
    Rt = M[:3, :3].T
    return 1. / scale, _se3(Rt, -(Rt @ M[:3, 3]) / scale)


def transform_map(scale, T, points=None, poses_cw=None):
    """A map under the similarity (scale, T): points (N, 3) -> scale R p + t; world-to-camera poses [R_cw | t_cw] ->
    [R_cw R^T | scale t_cw - R_cw R^T t] -- the camera frames scale with the map, so every projection stays what it was.
    -> (points or None, poses or None); poses come back as they were given: a list of SE3, or an array (K, 4, 4)."""
    M = T.as_matrix() if hasattr(T, 'as_matrix') else np.asarray(T, dtype=np.float64)
    R, t = M[:3, :3], M[:3, 3]
    out_pts = out_poses = None
    if points is not None:
        out_pts = scale * (_pts3(points, 'points') @ R.T) + t
    if poses_cw is not None:
        objects = len(poses_cw) > 0 and hasattr(poses_cw[0], 'as_matrix')
        P = np.stack([p.as_matrix() for p in poses_cw]) if objects else np.array(poses_cw, dtype=np.float64).reshape(-1, 4, 4)
        Q = np.tile(np.identity(4), (P.shape[0], 1, 1))
        Q[:, :3, :3] = P[:, :3, :3] @ R.T
        Q[:, :3, 3] = scale * P[:, :3, 3] - Q[:, :3, :3] @ t
        out_poses = [_se3(q[:3, :3], q[:3, 3]) for q in Q] if objects else Q
    return out_pts, out_poses
