"""Dense visual odometry pipelines: ``DenseVOPipeline`` and ``DenseRGBDPipeline``.

Attribute names, defaults and the control flow of ``track`` follow reference pyslam/pipelines/dense.py: the initial
guess from the keyframe, the previous pose or a constant-motion model, ``normalize()`` of the estimate, keyframe drops
on the ``SE3.log`` thresholds, the 'map' / 'track' modes, the (R_1_0, t_1_0_1) parameter split with the translation
held constant at pyramid levels above 2, and one Problem.solve per level, coarse to fine.  Attributes are read when
``track`` is called, so a caller may change them after construction (the reference's KITTI example pops the finest
level out of ``pyrlevel_sequence`` and ``pyr_cameras``).

Where the work runs differs: the image pyramids, the keyframe pixel tables and the whole coarse-to-fine solve of a frame
run on the device (pyslam_amd.device.DenseTracker; include/pyslam_hip.h: ps_dense_*), with one host synchronisation
per tracked frame.  The device keeps the frames of at most three slots -- the active keyframe, one more keyframe as a
cache and the tracking frame -- so its memory does not grow with the sequence; a keyframe that left the device is
uploaded again if 'track' mode returns to it.

Extras beyond the reference: ``last_iterations`` and ``last_cost_histories`` (the per-level iteration counts and
Problem._cost_history of the last tracked frame).

``DenseStereoPipeline`` is out of scope: its disparity comes from ``cv2.StereoBM``, which nothing here can pin
(DESIGN.md).
"""
import numpy as np

from pyslam_amd.liegroups import SE3, SO3
from pyslam_amd.losses import HuberLoss
from pyslam_amd.problem import Options
from pyslam_amd.pipelines.keyframes import DenseRGBDKeyframe

__all__ = ['DenseVOPipeline', 'DenseRGBDPipeline']


class _DeviceFrames:
    """The slots of one DenseTracker and which frame each holds, least recently used first out."""
    NUM_SLOTS = 3

    def __init__(self, levels, height, width):
        from pyslam_amd.device import DenseTracker
        self.shape = (int(levels), int(height), int(width))
        self.tracker = DenseTracker(levels, height, width, num_slots=self.NUM_SLOTS)
        self.owner = [None] * self.NUM_SLOTS
        self.has_depth = [False] * self.NUM_SLOTS
        self.tables_key = [None] * self.NUM_SLOTS
        self._used = [0] * self.NUM_SLOTS
        self._clock = 0

    def close(self):
        self.owner = [None] * self.NUM_SLOTS
        self.tracker.close()

    def slot_of(self, frame):
        for k, f in enumerate(self.owner):
            if f is frame:
                return k
        return None

    def place(self, frame, exclude=(), depth=False):
        """Slot holding `frame` (its image pyramid, and its depth when `depth`), uploading it if it is not resident."""
        k = self.slot_of(frame)
        if k is None:
            free = [j for j in range(self.NUM_SLOTS) if j not in exclude and self.owner[j] is None]
            k = free[0] if free else min((j for j in range(self.NUM_SLOTS) if j not in exclude), key=lambda j: self._used[j])
            self.tracker.upload(k, frame._pyrimage, frame._depth_image() if depth else None)
            self.owner[k], self.has_depth[k], self.tables_key[k] = frame, bool(depth), None
            frame._home = self
        elif depth and not self.has_depth[k]:
            self.tracker.upload(k, None, frame._depth_image())
            self.has_depth[k], self.tables_key[k] = True, None
        self._clock += 1
        self._used[k] = self._clock
        return k


class DenseVOPipeline:
    """Base class for dense VO pipelines"""

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

        self.pyrlevels = 4
        """Number of image pyramid levels for coarse-to-fine optimization"""
        self.pyrlevel_sequence = list(range(self.pyrlevels))[::-1]
        """Pyramid levels in the order they are solved (coarse to fine)"""

        self.keyframe_trans_thresh = 3.0  # meters
        """Translational distance threshold to drop new keyframes"""
        self.keyframe_rot_thresh = 0.3  # rad
        """Rotational distance threshold to drop new keyframes"""

        self.intensity_stiffness = 1. / 0.01
        """Photometric measurement stiffness"""
        self.depth_stiffness = 1. / 0.01
        """Depth or disparity measurement stiffness"""
        self.min_grad = 0.1
        """Minimum image gradient magnitude to use a given pixel"""
        self.depth_map_type = 'depth'
        """Is the depth map depth, inverse depth, disparity? ['depth','disparity'] supported"""
        self.mode = 'map'
        """Create new keyframes or localize against existing ones? ['map'|'track']"""
        self.use_motion_model_guess = True
        """Use constant motion model for initial guess."""
        self.loss = HuberLoss(10.0)
        """Loss function"""

        self.last_iterations = []
        """(extra) Gauss-Newton iterations per level of the last tracked frame, in pyrlevel_sequence order"""
        self.last_cost_histories = []
        """(extra) cost history per level of the last tracked frame (Problem._cost_history of each level)"""
        self._frames = None

        self._make_pyramid_cameras()

    def _make_pyramid_cameras(self):
        self.pyr_cameras = []
        for pyrlevel in self.pyrlevel_sequence:
            scale = 2 ** -pyrlevel
            cam = self.camera.clone()
            cam.fu *= scale
            cam.fv *= scale
            cam.cu *= scale
            cam.cv *= scale
            cam.h = int(np.ceil(cam.h * scale))
            cam.w = int(np.ceil(cam.w * scale))
            cam.compute_pixel_grid()
            self.pyr_cameras.append(cam)

    def set_mode(self, mode):
        """Set the localization mode to ['map'|'track']"""
        self.mode = mode
        if mode == 'track':
            self.active_keyframe_idx = 0
            self.T_c_w = []

    def track(self, trackframe, guess=None):
        """Track a frame (a DenseRGBDKeyframe).  guess: optional initial guess of the camera pose (world-to-camera)."""
        if not self.keyframes:
            # the first frame becomes the first keyframe; nothing to track against yet
            trackframe.compute_pyramids()
            self.keyframes.append(trackframe)
            self.active_keyframe_idx = 0
            return

        keyframe = self.keyframes[self.active_keyframe_idx]
        if guess is not None:
            guess = guess.dot(keyframe.T_c_w.inv())
        else:
            # the previous pose relative to the keyframe (identity when relocalisation just started) ...
            guess = SE3.identity() if not self.T_c_w else self.T_c_w[-1].dot(keyframe.T_c_w.inv())
            # ... advanced by the previous motion
            if self.use_motion_model_guess and len(self.T_c_w) > 1:
                guess = self.T_c_w[-1].dot(self.T_c_w[-2].inv().dot(guess))

        T_track_ref = self._compute_frame_to_frame_motion(keyframe, trackframe, guess)
        T_track_ref.normalize()
        self.T_c_w.append(T_track_ref.dot(keyframe.T_c_w))

        xi = SE3.log(T_track_ref)
        trans_dist = np.linalg.norm(xi[0:3])
        rot_dist = np.linalg.norm(xi[3:6])
        if trans_dist > self.keyframe_trans_thresh or rot_dist > self.keyframe_rot_thresh:
            if self.mode == 'map':
                trackframe.T_c_w = self.T_c_w[-1]
                trackframe.compute_pyramids()
                self.keyframes.append(trackframe)
                print('Dropped new keyframe. '
                      'Trans dist was {:.3f}. Rot dist was {:.3f}.'.format(trans_dist, rot_dist))
            self.active_keyframe_idx += 1
            print('Active keyframe idx: {}'.format(self.active_keyframe_idx))

    def _device_frames(self, frame):
        shape = (int(self.pyrlevels),) + tuple(np.asarray(frame._pyrimage).shape)
        if self._frames is None or self._frames.shape != shape:
            if self._frames is not None:
                self._frames.close()
            self._frames = _DeviceFrames(*shape)
        return self._frames

    def _compute_frame_to_frame_motion(self, ref_frame, track_frame, guess=SE3.identity()):
        """T_track_ref: one Problem.solve per level of pyrlevel_sequence (paired with pyr_cameras), parameters
        R_1_0 and t_1_0_1, t_1_0_1 constant above level 2 -- the whole sequence in one device call."""
        levels = [int(l) for l in self.pyrlevel_sequence]
        cams = list(self.pyr_cameras)[:len(levels)]
        levels = levels[:len(cams)]
        if self.depth_map_type != 'depth':
            raise ValueError("depth_map_type {!r}: only 'depth' is supported (the stereo pipeline's disparity maps are out "
                             "of scope)".format(self.depth_map_type))
        if ref_frame.pyrlevels != track_frame.pyrlevels or ref_frame._pyrimage.shape != track_frame._pyrimage.shape:
            raise ValueError('the keyframe and the tracked frame must have the same size and pyramid levels')
        frames = self._device_frames(ref_frame)
        tracker = frames.tracker
        ref_slot = frames.place(ref_frame, depth=True)
        var_i, var_d = self.intensity_stiffness ** -2, self.depth_stiffness ** -2
        key = (tuple(levels), tuple((c.cu, c.cv, c.fu, c.fv, int(c.w), int(c.h)) for c in cams), var_i, var_d,
               float(self.min_grad), self.depth_map_type)
        if frames.tables_key[ref_slot] != key:
            tracker.make_tables(ref_slot, levels, cams, var_i, var_d, self.min_grad)
            frames.tables_key[ref_slot] = key
        track_slot = frames.place(track_frame, exclude=(ref_slot,))
        pose = np.concatenate([guess.rot.as_matrix().reshape(9), np.asarray(guess.trans, dtype=float).reshape(3)])
        pose, its, hists = tracker.track(ref_slot, track_slot, levels, [l > 2 for l in levels], self.motion_options,
                                         self.loss, pose)
        self.last_iterations, self.last_cost_histories = its, hists
        return SE3(SO3(pose[:9].reshape(3, 3).copy()), pose[9:].copy())


class DenseRGBDPipeline(DenseVOPipeline):
    """Dense RGBD VO pipeline"""

    def __init__(self, camera, first_pose=SE3.identity()):
        super().__init__(camera, first_pose)
        self.depth_map_type = 'depth'
        self.depth_stiffness = 1 / 0.01

    def track(self, image, depth, guess=None):
        if not self.keyframes:
            trackframe = DenseRGBDKeyframe(image, depth, self.pyrlevels, self.T_c_w[0])
        else:
            trackframe = DenseRGBDKeyframe(image, depth, self.pyrlevels)
        super().track(trackframe, guess)
