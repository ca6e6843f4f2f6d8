"""Registration of a further monocular frame against the map on the device: absolute-pose (PnP) RANSAC over 2-D - 3-D
correspondences, and ``register_frame``, the one-line counterpart of ``twoview.bootstrap``: bootstrap -> register -> triangulate ->
bundle adjustment.

The reference has no counterpart (it has no monocular camera); the definition is this project's own, stated in csrc/ps_k_pnp.h and
restated by pipelines/absolute.py.  ``PnPRANSAC`` is shaped like EssentialRANSAC: the random minimal sets (three points) are drawn
on the host with ``np.random`` (so a seeded run picks the same hypotheses), everything else -- the P3P solves with their four slots
per sample, the scoring of every slot over every point, the arg-max, the Gauss-Newton refinement over the inliers -- is one call
into the HIP core (ps_pnp_ransac).  There is no CPU path.

The landmarks carry the scale of the map they come from (after ``bootstrap``: |t_21| = 1), and so does the translation of T_cw."""
import numpy as np

from pyslam_amd import _native as nat
from pyslam_amd.pipelines.ransac import _cam5
from pyslam_amd.pipelines.twoview import _obs2


def _pts3(pts, name):
    a = np.asarray(pts, dtype=np.float64)
    if a.ndim == 1 and a.size == 3:
        a = a.reshape(1, 3)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("{} must have shape (N, 3), got {}".format(name, a.shape))
    return np.ascontiguousarray(a)


class PnPRANSAC:
    def __init__(self, camera):
        self.camera = camera
        self.ransac_iters = 400
        self.ransac_thresh = 4.0  # (2 px)**2, squared reprojection error
        self.num_min_set_pts = 3
        self.min_inliers = 12
        self.refine = True
        self.refine_iters = 5

    def set_obs(self, pts_w, obs):
        p, o = _pts3(pts_w, 'pts_w'), _obs2(obs, 'obs')
        if p.shape[0] != o.shape[0]:
            raise ValueError("pts_w and obs must hold the same number of points, got {} and {}".format(p.shape[0], o.shape[0]))
        self.pts_w, self.obs = p, o
        self.num_pts = p.shape[0]

    def draw_samples(self):
        """(ransac_iters, 3) indices, every row without repetition, from ``np.random``."""
        return np.stack([np.random.choice(self.num_pts, self.num_min_set_pts, replace=False)
                         for _ in range(self.ransac_iters)]).astype(np.int32)

    def perform_ransac(self):
        """(T_cw: SE3, pts_inliers, obs_inliers, inlier_indices); ValueError below ``min_inliers`` inliers or 3 points.  The
        counts, the cost history and every point's squared error stay on the object (info_)."""
        from liegroups import SE3
        if self.num_min_set_pts != 3:
            raise ValueError("PnPRANSAC: the minimal solver is P3P (num_min_set_pts = 3)")
        if self.num_pts < 3:
            raise ValueError("PnPRANSAC: P3P needs at least 3 correspondences, got {}".format(self.num_pts))
        nat.require_gpu()
        res = self._device_ransac(self.draw_samples())
        self.info_ = res
        inliers = np.where(res['mask'])[0]
        if res['count'] < self.min_inliers:
            raise ValueError("PnPRANSAC failed to find {} inliers (found {}). Try adjusting the thresholds.".format(
                self.min_inliers, res['count']))
        return SE3.from_matrix(res['T_cw'], normalize=True), self.pts_w[inliers], self.obs[inliers], inliers

    def _samples(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.ndim != 2 or idx.shape[1] != 3:
            raise ValueError("the sample table must have shape (H, 3)")
        return idx

    def _device_ransac(self, idx):
        idx = self._samples(idx)
        N = self.num_pts
        iters = int(self.refine_iters) if self.refine else 0
        T = np.zeros((4, 4))
        mask, info, sq_err, hist = np.zeros(N, dtype=np.uint8), np.zeros(8, dtype=np.int32), np.zeros(N), np.zeros(iters + 1)
        nat.check(nat.load().ps_pnp_ransac(
            nat.f64p(self.pts_w), nat.f64p(self.obs), N, nat.i32p(idx), idx.shape[0], nat.f64p(_cam5(self.camera)),
            float(self.ransac_thresh), iters, nat.f64p(T), mask.ctypes.data_as(nat.c_u8p), nat.i32p(info), nat.f64p(sq_err),
            nat.f64p(hist)))
        return dict(T_cw=T, mask=mask.astype(bool), best=int(info[0]), best_slot=int(info[1]), raw_count=int(info[2]),
                    count=int(info[3]), refine_kept=bool(info[4]), pivot_failed=bool(info[5]), iterations=int(info[6]),
                    d=sq_err, cost_history=hist)

    def _device_hypotheses(self, idx):
        """Every sample's (T_all (H, 4, 4, 4), counts (H, 4), empty (H, 4) bool, degenerate (H,) bool): what the tests hold
        against the restatement."""
        idx = self._samples(idx)
        H = idx.shape[0]
        T, counts, flags = np.zeros((H, 4, 4, 4)), np.zeros((H, 4), dtype=np.int32), np.zeros((H, 4), dtype=np.uint8)
        nat.check(nat.load().ps_pnp_hypotheses(
            nat.f64p(self.pts_w), nat.f64p(self.obs), self.num_pts, nat.i32p(idx), H, nat.f64p(_cam5(self.camera)),
            float(self.ransac_thresh), nat.f64p(T), nat.i32p(counts), flags.ctypes.data_as(nat.c_u8p)))
        return T, counts, (flags & 1).astype(bool), (flags[:, 0] & 2).astype(bool)

    def compute_ransac_cost(self, T_stacked, pts_w, obs, camera, thresh):
        """Boolean inlier mask (num_poses, num_pts) of given poses T_cw (4 x 4 each)."""
        nat.require_gpu()
        T = np.ascontiguousarray(T_stacked, dtype=np.float64).reshape(-1, 4, 4)
        p, o = _pts3(pts_w, 'pts_w'), _obs2(obs, 'obs')
        if p.shape[0] != o.shape[0]:
            raise ValueError("pts_w and obs must hold the same number of points")
        masks = np.zeros((T.shape[0], p.shape[0]), dtype=np.uint8)
        nat.check(nat.load().ps_pnp_score(nat.f64p(T), T.shape[0], nat.f64p(p), nat.f64p(o), p.shape[0], nat.f64p(_cam5(camera)),
                                          float(thresh), masks.ctypes.data_as(nat.c_u8p), None))
        return masks.astype(bool)


def register_frame(camera, points, obs, seed=None, ransac=None):
    """Landmarks of the map and their pixels in a further monocular frame -> (T_cw: SE3, inlier_indices).  Runs PnPRANSAC
    (``seed``: seeds ``np.random`` first; ``ransac``: a configured PnPRANSAC to use instead of a default one).  ValueError below
    ``min_inliers`` inliers."""
    rs = ransac if ransac is not None else PnPRANSAC(camera)
    rs.set_obs(points, obs)
    if seed is not None:
        np.random.seed(seed)
    T_cw, _, _, inliers = rs.perform_ransac()
    return T_cw, inliers


def three_view_tables(camera, T_21, T_31, obs_1, obs_2, points, seen_3, obs_3):
    """two_view_tables with a third keyframe: poses 1 (the identity) and 2 (``T_21``) held, pose 3 (start value ``T_31``, 4 x 4)
    free; one variable landmark per row of ``points`` (start values), seen by keyframes 1 and 2 (``obs_1``, ``obs_2``) and, for
    the landmark indices ``seen_3``, by keyframe 3 (``obs_3``, one row per entry of ``seen_3``).  Unit pixel stiffness, L2 loss."""
    from pyslam_amd.lowering import LoweredProblem, pack_pose_matrices
    n = obs_1.shape[0]
    seen_3 = np.asarray(seen_3, dtype=np.int32)
    m = seen_3.size
    cam = np.array([camera.cu, camera.cv, camera.fu, camera.fv, -2.0])
    S2 = np.zeros((3, 3))
    S2[0, 0] = S2[1, 1] = 1.0
    uvd = np.zeros((2 * n + m, 3))
    uvd[:n, :2], uvd[n:2 * n, :2], uvd[2 * n:, :2] = obs_1, obs_2, obs_3
    arange = np.arange(n, dtype=np.int32)
    return LoweredProblem(
        dof=6, poses=pack_pose_matrices(np.stack([np.identity(4), np.asarray(T_21, dtype=np.float64), np.asarray(T_31, dtype=np.float64)])),
        pose_rid=np.array([-1, -1, 0], dtype=np.int32), points=np.array(points, dtype=np.float64).reshape(n, 3), point_vid=arange.copy(),
        obs_pose=np.concatenate([np.repeat(np.arange(2, dtype=np.int32), n), np.full(m, 2, dtype=np.int32)]),
        obs_point=np.concatenate([arange, arange, seen_3]), obs_uvd=uvd,
        cams=cam[None, :], stiff3=S2.reshape(1, 9), obs_groups=np.array([[0., 0., 0., 0.]]),
        pose_keys=['T_1_w', 'T_2_w', 'T_3_w'], point_keys=['pt{}_w'.format(j) for j in range(n)]).finalize()
