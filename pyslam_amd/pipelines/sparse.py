"""Sparse visual odometry pipelines: ``SparseVOPipeline``, ``SparseStereoPipeline`` and ``SparseRGBDPipeline``.

Constructor arguments, attribute names, defaults and the control flow of ``track`` / ``set_mode`` follow reference
pyslam/pipelines/sparse.py: the frame-to-frame motion is feature matches -> observations (``uvd`` for stereo, ``uvz``
with the depth read at ``depth[int(v), int(u)]`` for RGB-D) -> pruning of non-positive depth / disparity ->
``self.ransac`` -> a ``ReprojectionMotionOnlyBatchResidual`` in a ``Problem`` under ``self.motion_options`` with
``self.loss``; then ``normalize()``, the pose chained on the active keyframe, and keyframe drops on the ``SE3.log``
thresholds in the 'map' / 'track' modes.  ``self.ransac``, ``self.loss``, ``self.matcher`` and ``self.motion_options``
are read when ``track`` is called, so a caller may swap or edit them as with the reference.

What differs is where the work runs: the matcher is the device matcher of pipelines/matcher.py (the reference's is
libviso2, which this project does not reproduce: DESIGN.md section 7), RANSAC and the motion-only solve are the
device paths ``FrameToFrameRANSAC`` and ``Problem`` already have.  ``self.matcher`` may be any object with
``pushBack(left[, right])``, ``matchFeatures(mode)`` and ``getMatches()`` (items with ``u1p v1p u2p v2p u1c v1c u2c
v2c``); one that also has ``matches_array()`` is read through it.

Two defects of the reference are repaired: its stereo ``_compute_frame_to_frame_motion`` indexes a
Python list with ``[:, 2]`` and cannot run past the first frame (the observations are arrays here, as in its RGB-D
sibling), and ``self.mode is 'map'`` compares identity (``==`` here).
"""
import numpy as np

from pyslam_amd.liegroups import SE3
from pyslam_amd.losses import L2Loss
from pyslam_amd.problem import Options, Problem
from pyslam_amd.residuals import ReprojectionMotionOnlyBatchResidual
from pyslam_amd.pipelines.keyframes import SparseStereoKeyframe, SparseRGBDKeyframe
from pyslam_amd.pipelines.ransac import FrameToFrameRANSAC
from pyslam_amd.pipelines.matcher import Matcher, Matcher_parameters

__all__ = ['SparseVOPipeline', 'SparseStereoPipeline', 'SparseRGBDPipeline']


class SparseVOPipeline:
    """Base class for sparse VO pipelines"""

    def __init__(self, camera, first_pose=SE3.identity()):
        self.camera = camera
        """Camera model"""
        self.first_pose = first_pose
        """First pose"""
        self.keyframes = []
        """List of keyframes"""
        self.T_c_w = [first_pose]
        """List of camera poses"""
        self.motion_options = Options()
        """Optimizer parameters for motion estimation"""
        self.motion_options.allow_nondecreasing_steps = True
        self.motion_options.max_nondecreasing_steps = 5
        self.motion_options.min_cost_decrease = 0.99
        self.motion_options.max_iters = 30
        self.motion_options.num_threads = 1
        self.motion_options.linesearch_max_iters = 0

        self.keyframe_trans_thresh = 3.0  # meters
        """Translational distance threshold to drop new keyframes"""
        self.keyframe_rot_thresh = 0.3  # rad
        """Rotational distance threshold to drop new keyframes"""

        self.matcher_params = Matcher_parameters()
        """Parameters of the feature matcher"""
        self.matcher = Matcher(self.matcher_params)
        """Feature matcher (device)"""
        self.matcher_mode = 0
        """Matching mode 0=flow 1=stereo 2=quad"""

        self.ransac = FrameToFrameRANSAC(self.camera)
        """RANSAC outlier rejection"""

        self.reprojection_stiffness = np.diag([1., 1., 1.])
        """Reprojection error stiffness matrix"""
        self.mode = 'map'
        """Create new keyframes or localize against existing ones? ['map'|'track']"""

        self.loss = L2Loss()
        """Loss function"""

    def set_mode(self, mode):
        """Set the localization mode to ['map'|'track']"""
        self.mode = mode
        if self.mode == 'track':
            self.active_keyframe_idx = 0
            self.T_c_w = []

    def track(self, trackframe):
        """Track a frame (a keyframe object of the pipeline's kind)."""
        if len(self.keyframes) == 0:
            # the first frame becomes the first keyframe; nothing to track yet
            self.keyframes.append(trackframe)
            self.active_keyframe_idx = 0
            return
        active_keyframe = self.keyframes[self.active_keyframe_idx]

        T_track_ref = self._compute_frame_to_frame_motion(active_keyframe, trackframe)
        T_track_ref.normalize()
        self.T_c_w.append(T_track_ref.dot(active_keyframe.T_c_w))

        se3_vec = SE3.log(T_track_ref)
        trans_dist = np.linalg.norm(se3_vec[0:3])
        rot_dist = np.linalg.norm(se3_vec[3:6])

        if trans_dist > self.keyframe_trans_thresh or rot_dist > self.keyframe_rot_thresh:
            if self.mode == 'map':
                trackframe.T_c_w = self.T_c_w[-1]
                self.keyframes.append(trackframe)
                print('Dropped new keyframe. '
                      'Trans dist was {:.3f}. Rot dist was {:.3f}.'.format(trans_dist, rot_dist))
            self.active_keyframe_idx += 1
            print('Active keyframe idx: {}'.format(self.active_keyframe_idx))

    def _matches(self):
        """(n, 8) array u1p v1p u2p v2p u1c v1c u2c v2c of the matcher's current matches."""
        self.matcher.matchFeatures(self.matcher_mode)
        if hasattr(self.matcher, 'matches_array'):
            return self.matcher.matches_array()[0]
        return np.array([[m.u1p, m.v1p, m.u2p, m.v2p, m.u1c, m.v1c, m.u2c, m.v2c] for m in self.matcher.getMatches()],
                        dtype=float).reshape(-1, 8)

    def _solve_motion(self):
        """RANSAC on self.obs_0 / self.obs_1, then the motion-only solve on its inliers."""
        keep_mask = (self.obs_0[:, 2] > 0) & (self.obs_1[:, 2] > 0)
        self.obs_0 = self.obs_0[keep_mask, :]
        self.obs_1 = self.obs_1[keep_mask, :]

        self.ransac.set_obs(self.obs_0, self.obs_1)
        T_1_0_guess, obs_0_inliers, obs_1_inliers, _ = self.ransac.perform_ransac()

        residual = ReprojectionMotionOnlyBatchResidual(
            self.camera, obs_0_inliers, obs_1_inliers, self.reprojection_stiffness)
        problem = Problem(self.motion_options)
        problem.add_residual_block(residual, ['T_1_0'], loss=self.loss)
        problem.initialize_params({'T_1_0': T_1_0_guess})
        params = problem.solve()
        return params['T_1_0']


class SparseStereoPipeline(SparseVOPipeline):
    """Sparse stereo VO pipeline"""

    def __init__(self, camera, first_pose=SE3.identity()):
        super().__init__(camera, first_pose)
        self.matcher_mode = 2  # stereo quad matching
        self.matcher.setIntrinsics(camera.fu, camera.cu, camera.cv, camera.b)

    def track(self, im_left, im_right):
        if len(self.keyframes) == 0:
            trackframe = SparseStereoKeyframe(im_left, im_right, self.T_c_w[0])
        else:
            trackframe = SparseStereoKeyframe(im_left, im_right)
        super().track(trackframe)

    def _compute_frame_to_frame_motion(self, ref_frame, track_frame):
        self.matcher.pushBack(ref_frame.im_left, ref_frame.im_right)
        self.matcher.pushBack(track_frame.im_left, track_frame.im_right)
        m = self._matches()
        # stereo observations (u, v, disparity)
        self.obs_0 = np.stack([m[:, 0], m[:, 1], m[:, 0] - m[:, 2]], axis=1)
        self.obs_1 = np.stack([m[:, 4], m[:, 5], m[:, 4] - m[:, 6]], axis=1)
        return self._solve_motion()


class SparseRGBDPipeline(SparseVOPipeline):
    """Sparse RGB-D VO pipeline"""

    def __init__(self, camera, first_pose=SE3.identity()):
        super().__init__(camera, first_pose)
        self.matcher_mode = 0  # mono-to-mono

    def track(self, image, depth):
        if len(self.keyframes) == 0:
            trackframe = SparseRGBDKeyframe(image, depth, self.T_c_w[0])
        else:
            trackframe = SparseRGBDKeyframe(image, depth)
        super().track(trackframe)

    def _compute_frame_to_frame_motion(self, ref_frame, track_frame):
        self.matcher.pushBack(ref_frame.image)
        self.matcher.pushBack(track_frame.image)
        m = self._matches()
        # RGB-D observations (u, v, z) with the depth of the pixel the match falls in
        z0 = np.asarray(ref_frame.depth)[m[:, 1].astype(int), m[:, 0].astype(int)]
        z1 = np.asarray(track_frame.depth)[m[:, 5].astype(int), m[:, 4].astype(int)]
        self.obs_0 = np.stack([m[:, 0], m[:, 1], z0], axis=1).astype(float)
        self.obs_1 = np.stack([m[:, 4], m[:, 5], z1], axis=1).astype(float)
        return self._solve_motion()
