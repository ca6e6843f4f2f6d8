"""Monocular two-view initialisation on the device: essential-matrix RANSAC over 2-D - 2-D correspondences, and ``bootstrap``,
which turns its result into the two held keyframes and triangulated landmarks that monocular bundle adjustment starts from.

The reference has no counterpart (it has no monocular camera); the definition is this project's own, stated in
csrc/ps_k_twoview.h and restated in numpy by pipelines/epipolar.py.  ``EssentialRANSAC`` is shaped like FrameToFrameRANSAC:
the random minimal sets are drawn on the host with ``np.random`` (so a seeded run picks the same hypotheses), everything else
-- the eight-point solves, the scoring of every hypothesis over every point, the arg-max, the refit over the inliers, the
decomposition and the cheirality vote -- is one call into the HIP core (ps_twoview_ransac).  There is no CPU path.

The eight-point solver is degenerate for planar scenes and needs a baseline: under pure rotation the essential matrix is
undetermined and ``bootstrap`` refuses the result by its parallax."""
import ctypes as C

import numpy as np

from pyslam_amd import _native as nat
from pyslam_amd.pipelines.ransac import _cam5


def _obs2(obs, name):
    a = np.asarray(obs, dtype=np.float64)
    if a.ndim == 1 and a.size in (2, 3):
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] not in (2, 3):
        raise ValueError("{} must have shape (N, 2) or (N, 3), got {}".format(name, a.shape))
    return np.ascontiguousarray(a[:, :2])


class EssentialRANSAC:
    def __init__(self, camera):
        self.camera = camera
        self.ransac_iters = 400
        self.ransac_thresh = 4.0  # (2 px)**2, squared Sampson distance
        self.num_min_set_pts = 8
        self.min_inliers = 16
        self.refit = True

    def set_obs(self, obs_1, obs_2):
        o1, o2 = _obs2(obs_1, 'obs_1'), _obs2(obs_2, 'obs_2')
        if o1.shape[0] != o2.shape[0]:
            raise ValueError("obs_1 and obs_2 must hold the same number of points, got {} and {}".format(o1.shape[0], o2.shape[0]))
        self.obs_1, self.obs_2 = o1, o2
        self.num_pts = o1.shape[0]

    def draw_samples(self):
        """(ransac_iters, 8) indices, every row without repetition, from ``np.random``."""
        return np.stack([np.random.choice(self.num_pts, self.num_min_set_pts, replace=False)
                         for _ in range(self.ransac_iters)]).astype(np.int32)

    def perform_ransac(self):
        """(T_21: SE3 with |t| = 1, obs_1_inliers, obs_2_inliers, inlier_indices); ValueError below ``min_inliers`` inliers or
        8 points.  The essential matrix, the counts and the inliers' parallax stay on the object (E_, info_, parallax_deg_)."""
        from liegroups import SE3
        if self.num_min_set_pts != 8:
            raise ValueError("EssentialRANSAC: the minimal solver is the eight-point algorithm (num_min_set_pts = 8)")
        if self.num_pts < 8:
            raise ValueError("EssentialRANSAC: the eight-point algorithm needs at least 8 correspondences, got {}".format(self.num_pts))
        nat.require_gpu()
        res = self._device_ransac(self.draw_samples())
        self.E_, self.info_ = res['E'], res
        inliers = np.where(res['mask'])[0]
        self.parallax_deg_ = res['parallax_deg'][inliers]
        if res['count'] < self.min_inliers:
            raise ValueError("EssentialRANSAC failed to find {} inliers (found {}). Try adjusting the thresholds.".format(
                self.min_inliers, res['count']))
        return SE3.from_matrix(res['T_21'], normalize=True), self.obs_1[inliers], self.obs_2[inliers], inliers

    def _samples(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.ndim != 2 or idx.shape[1] != 8:
            raise ValueError("the sample table must have shape (H, 8)")
        return idx

    def _device_ransac(self, idx):
        idx = self._samples(idx)
        N = self.num_pts
        T, E = np.zeros((4, 4)), np.zeros((3, 3))
        mask, info, par = np.zeros(N, dtype=np.uint8), np.zeros(8, dtype=np.int32), np.zeros(N)
        nat.check(nat.load().ps_twoview_ransac(
            nat.f64p(self.obs_1), nat.f64p(self.obs_2), N, nat.i32p(idx), idx.shape[0], nat.f64p(_cam5(self.camera)),
            float(self.ransac_thresh), 1 if self.refit else 0, nat.f64p(T), nat.f64p(E), mask.ctypes.data_as(nat.c_u8p),
            nat.i32p(info), nat.f64p(par)))
        return dict(T_21=T, E=E, mask=mask.astype(bool), best=int(info[0]), raw_count=int(info[1]), count=int(info[2]),
                    refit_kept=bool(info[3]), cheirality_counts=info[4:8].copy(), parallax_deg=par)

    def _device_hypotheses(self, idx):
        """Every sample's (E (H, 3, 3), counts (H,), degenerate (H,) bool): what the tests hold against the restatement."""
        idx = self._samples(idx)
        H = idx.shape[0]
        E, counts, flags = np.zeros((H, 3, 3)), np.zeros(H, dtype=np.int32), np.zeros(H, dtype=np.uint8)
        nat.check(nat.load().ps_twoview_hypotheses(
            nat.f64p(self.obs_1), nat.f64p(self.obs_2), self.num_pts, nat.i32p(idx), H, nat.f64p(_cam5(self.camera)),
            float(self.ransac_thresh), nat.f64p(E), nat.i32p(counts), flags.ctypes.data_as(nat.c_u8p)))
        return E, counts, flags.astype(bool)

    def compute_ransac_cost(self, E_stacked, obs_1, obs_2, camera, thresh):
        """Boolean inlier mask (num_matrices, num_pts) of given essential matrices."""
        nat.require_gpu()
        E = np.ascontiguousarray(E_stacked, dtype=np.float64).reshape(-1, 3, 3)
        o1, o2 = _obs2(obs_1, 'obs_1'), _obs2(obs_2, 'obs_2')
        if o1.shape[0] != o2.shape[0]:
            raise ValueError("obs_1 and obs_2 must hold the same number of points")
        masks = np.zeros((E.shape[0], o1.shape[0]), dtype=np.uint8)
        nat.check(nat.load().ps_twoview_score(nat.f64p(E), E.shape[0], nat.f64p(o1), nat.f64p(o2), o1.shape[0],
                                              nat.f64p(_cam5(camera)), float(thresh), masks.ctypes.data_as(nat.c_u8p), None))
        return masks.astype(bool)


def two_view_tables(camera, T_21, obs_1, obs_2):
    """The two-keyframe monocular tables of the correspondences: pose 1 the identity, pose 2 ``T_21`` (4 x 4), both held, one
    variable landmark per correspondence (start value: 1 m in front of camera 1), unit pixel stiffness, L2 loss."""
    from pyslam_amd.lowering import LoweredProblem, pack_pose_matrices
    n = obs_1.shape[0]
    cam = np.array([camera.cu, camera.cv, camera.fu, camera.fv, -2.0])
    S2 = np.zeros((3, 3))
    S2[0, 0] = S2[1, 1] = 1.0
    uvd = np.zeros((2 * n, 3))
    uvd[:n, :2], uvd[n:, :2] = obs_1, obs_2
    return LoweredProblem(
        dof=6, poses=pack_pose_matrices(np.stack([np.identity(4), np.asarray(T_21, dtype=np.float64)])),
        pose_rid=np.array([-1, -1], dtype=np.int32), points=np.tile([0., 0., 1.], (n, 1)), point_vid=np.arange(n, dtype=np.int32),
        obs_pose=np.repeat(np.arange(2, dtype=np.int32), n), obs_point=np.tile(np.arange(n, dtype=np.int32), 2), obs_uvd=uvd,
        cams=cam[None, :], stiff3=S2.reshape(1, 9), obs_groups=np.array([[0., 0., 0., 0.]]),
        pose_keys=['T_1_w', 'T_2_w'], point_keys=['pt{}_w'.format(j) for j in range(n)]).finalize()


def bootstrap(camera, obs_1, obs_2, min_parallax_deg=1.0, seed=None, ransac=None):
    """Two monocular frames and their matches -> the start of monocular bundle adjustment.  Runs EssentialRANSAC (``seed``: seeds
    ``np.random`` first; ``ransac``: a configured EssentialRANSAC to use instead of a default one), takes frame 1 as the world
    frame and T_21 (|t| = 1: the scale of the map) as the second pose, and triangulates one landmark per inlier on the device
    (pyslam_amd.triangulate_tables).  -> (T_21: SE3, points (M, 3), landmark_status (M,), inlier_indices (M,)).
    ValueError when fewer than ``min_inliers`` landmarks come back with status 0 -- pure rotation or no baseline shows up as
    status 2 (parallax below ``min_parallax_deg``)."""
    from pyslam_amd.problem import triangulate_tables
    rs = ransac if ransac is not None else EssentialRANSAC(camera)
    rs.set_obs(obs_1, obs_2)
    if seed is not None:
        np.random.seed(seed)
    T_21, o1, o2, inliers = rs.perform_ransac()
    points, status = triangulate_tables(two_view_tables(camera, T_21.as_matrix(), o1, o2), 5, min_parallax_deg)
    good = int((status == 0).sum())
    if good < rs.min_inliers:
        raise ValueError("bootstrap: only {} of {} inliers triangulate (status counts {}): too little parallax for a two-view "
                         "initialisation (pure rotation or no baseline?)".format(good, inliers.size, np.bincount(status, minlength=4).tolist()))
    return T_21, points, status, inliers
