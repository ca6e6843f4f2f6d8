"""Monocular tracking against a map: ``track_frame``, ``relocalise_frame`` and ``SparseMonoPipeline``.

The reference has no counterpart (it has no monocular camera).  Both are compositions of pieces that run on the device and are
pinned one by one: the matcher's matching by projection (``Matcher.setMap`` / ``matchMap``), the
flow match, ``twoview.bootstrap``, ``pnp.register_frame``, ``triangulate_tables`` and the tables route of the bundle adjustment
(``solve_tables``).  There is no CPU path.

``track_frame`` registers one image against given landmarks: every landmark is projected with the pose prior, matched to the
image's features inside a small window around its projection -- every feature goes to one landmark only -- and P3P RANSAC over
the matched pairs gives the pose.

``relocalise_frame`` registers one image against given landmarks without a pose prior: every landmark is compared with every feature
of the image (``Matcher.matchMapGlobal``, step 9: best against second-best cost), P3P RANSAC over the unambiguous pairs gives a pose,
and one guided pass -- ``track_frame``'s match and RANSAC with that pose as prior -- widens the inlier set.

``SparseMonoPipeline.track(image)`` is the whole chain.  The first frame is the reference keyframe; every further frame is
flow-matched to it until ``bootstrap`` succeeds (a frame on which it does not has the pose ``None``), which makes that frame the
second keyframe and its status-0 landmarks the map, scaled so that the two keyframes are ``init_baseline`` apart.  From then on a
frame is tracked with the last pose as prior against the landmarks the last ``local_window`` keyframes see.  A frame becomes a
keyframe when its translation to the active keyframe, divided by the median depth of the landmarks it tracks, exceeds
``keyframe_parallax_thresh`` or its rotation exceeds ``keyframe_rot_thresh``: its observations join their landmarks' tracks, the
flow matches to the previous keyframe whose features are bound to no landmark are checked against the epipolar geometry of the two
poses and triangulated, and (``local_ba``) a monocular bundle adjustment runs over the window with its two oldest keyframes held,
after which landmarks behind one of their cameras are dropped.

The map lives on the host as arrays -- ``points_w`` (L, 3), ``descriptors`` (L, 32), ``alive`` (L,) and the observation table
``obs_kf`` / ``obs_lm`` / ``obs_uv`` -- and is uploaded to the matcher when the landmarks tracked against change.  Its scale is
that of the initialisation; its drift is corrected only by ``loop_correction`` below (no scale prior: DESIGN.md section 7, limits).

Loop detection (``loop_detection``, off by default): every keyframe's descriptors join the matcher's keyframe database, and after a
new keyframe k and its bundle adjustment ``loop.detect_loop`` runs over the entries ``[0, k - loop_gap)``.  A hit is recorded in
``loop_closures``; on its own it corrects nothing, and poses and map are those of the same run with the switch off.

Loop correction (``loop_correction``, off by default; needs ``loop_detection``): a recorded closure runs ``posegraph.correct_loop`` over
all keyframes -- a Sim(3) pose graph of the odometry edges, the covisibility edges between keyframes that share at least
``loop_min_shared`` landmarks and the closure, solved on the device -- and keyframe poses, landmarks (each with its first observing
keyframe) and the poses of the frames in between (each with its preceding keyframe) move; ``loop_corrections`` records the run.
Without a closure the switch changes nothing.

Tracking loss (``relocalise``): a frame on which ``register_frame`` raises ValueError is relocalised against all live landmarks.
Where that fails too the frame's pose is ``None`` and the pipeline is ``lost``: every further frame is relocalised until one
succeeds (its index joins ``relocalised``), after which tracking goes on as before."""
import numpy as np

from pyslam_amd.liegroups import SE3
from pyslam_amd.losses import L2Loss
from pyslam_amd.problem import Options
from pyslam_amd.pipelines.matcher import Matcher, Matcher_parameters
from pyslam_amd.pipelines.pnp import PnPRANSAC, register_frame, _pts3
from pyslam_amd.pipelines.twoview import EssentialRANSAC, bootstrap

__all__ = ['track_frame', 'relocalise_frame', 'SparseMonoPipeline', 'SparseMonoKeyframe', 'window_tables']


def _set_map_if_changed(matcher, pts, desc):
    held = getattr(matcher, '_map', None)
    if held is None or held[0].shape != pts.shape or not np.array_equal(held[0], pts) or not np.array_equal(held[1], desc):
        matcher.setMap(pts, desc)


def _track(camera, matcher, image, points_w, descriptors, T_prior, radius, seed, ransac):
    if np.asarray(points_w).size == 0:
        raise ValueError('track_frame: the map is empty')
    pts = _pts3(points_w, 'points_w')
    desc = np.ascontiguousarray(np.asarray(descriptors, dtype=np.uint8).reshape(-1, 32))
    if desc.shape[0] != pts.shape[0]:
        raise ValueError('track_frame: {} landmarks and {} descriptors'.format(pts.shape[0], desc.shape[0]))
    rs = ransac if ransac is not None else PnPRANSAC(camera)
    matcher.pushBack(image)
    _set_map_if_changed(matcher, pts, desc)
    feature, status, _, uv = matcher.matchMap(T_prior, camera, int(radius))
    if int((status == 0).sum()) < rs.min_inliers:              # the prior was poor: once more with twice the window
        feature, status, _, uv = matcher.matchMap(T_prior, camera, 2 * int(radius))
    idx = np.nonzero(status == 0)[0]
    T_cw, inl = register_frame(camera, pts[idx], uv[idx], seed=seed, ransac=rs)
    keep = idx[inl]
    return T_cw, keep, uv[keep], feature[keep]


def track_frame(camera, matcher, image, points_w, descriptors, T_prior, radius=12, seed=None, ransac=None):
    """One monocular image registered against landmarks -> ``(T_cw: SE3, landmark_indices, obs)``: the pose, the indices of
    the landmarks that are inliers of it and their sub-pixel positions in the image.  ``points_w`` (N, 3) and ``descriptors``
    (N, 32) are the landmarks, ``T_prior`` (SE3 or 4 x 4) the pose they are projected with, ``radius`` the half-width of the
    search window in pixels (doubled once when fewer than ``ransac.min_inliers`` landmarks match), ``seed`` / ``ransac`` as in
    ``register_frame``.  ValueError on an empty map and where ``register_frame`` raises it."""
    return _track(camera, matcher, image, points_w, descriptors, T_prior, radius, seed, ransac)[:3]


def _relocalise(camera, matcher, image, points_w, descriptors, ratio, radius, seed, ransac):
    if np.asarray(points_w).size == 0:
        raise ValueError('relocalise_frame: the map is empty')
    pts = _pts3(points_w, 'points_w')
    desc = np.ascontiguousarray(np.asarray(descriptors, dtype=np.uint8).reshape(-1, 32))
    if desc.shape[0] != pts.shape[0]:
        raise ValueError('relocalise_frame: {} landmarks and {} descriptors'.format(pts.shape[0], desc.shape[0]))
    rs = ransac if ransac is not None else PnPRANSAC(camera)
    matcher.pushBack(image)
    _set_map_if_changed(matcher, pts, desc)
    feature, status, _, _, uv = matcher.matchMapGlobal(ratio)
    idx = np.nonzero(status == 0)[0]
    T_cw, inl = register_frame(camera, pts[idx], uv[idx], seed=seed, ransac=rs)
    keep = idx[inl]
    first = T_cw, keep, uv[keep], feature[keep]
    # the guided pass: matching by projection with the pose just found
    feature, status, _, uv = matcher.matchMap(T_cw, camera, int(radius))
    idx = np.nonzero(status == 0)[0]
    try:
        T_cw, inl = register_frame(camera, pts[idx], uv[idx], seed=None if seed is None else seed + 1, ransac=rs)
    except ValueError:
        return first
    if len(inl) < first[1].shape[0]:
        return first
    keep = idx[inl]
    return T_cw, keep, uv[keep], feature[keep]


def relocalise_frame(camera, matcher, image, points_w, descriptors, ratio=(4, 5), radius=12, seed=None, ransac=None):
    """One monocular image registered against landmarks without a pose prior -> ``(T_cw: SE3, landmark_indices, obs)`` as
    ``track_frame`` returns them.  Two passes: every landmark against every feature of the image (``Matcher.matchMapGlobal`` with
    ``ratio``) and ``register_frame`` over the status-0 pairs with ``seed``; then ``matchMap`` with the pose just found and
    ``radius``, and ``register_frame`` over its status-0 pairs (with ``seed + 1`` when a seed was given).  The second pass's result
    is returned unless it raises ValueError or has fewer inliers than the first, whose result is returned then.  ValueError on an
    empty map and where the first ``register_frame`` raises it."""
    return _relocalise(camera, matcher, image, points_w, descriptors, ratio, radius, seed, ransac)[:3]


def window_tables(camera, poses, held, points, obs_kf, obs_lm, obs_uv, loss=None):
    """Monocular tables of K keyframes (``poses`` (K, 4, 4) world-to-camera, ``held`` (K,) bool: constant) and L variable
    landmarks (``points`` (L, 3) start values) with the observations ``obs_uv`` (M, 2) of landmark ``obs_lm`` in keyframe
    ``obs_kf``.  Unit pixel stiffness; ``loss``: a loss of pyslam_amd.losses (L2 by default)."""
    from pyslam_amd.lowering import LoweredProblem, pack_pose_matrices
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    held = np.asarray(held, dtype=bool)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n, m = points.shape[0], len(obs_kf)
    S2 = np.zeros((3, 3))
    S2[0, 0] = S2[1, 1] = 1.0
    uvd = np.zeros((m, 3))
    uvd[:, :2] = obs_uv
    loss = loss if loss is not None else L2Loss()
    return LoweredProblem(
        dof=6, poses=pack_pose_matrices(poses), pose_rid=np.where(held, -1, np.cumsum(~held) - 1).astype(np.int32),
        points=points, point_vid=np.arange(n, dtype=np.int32), obs_pose=np.asarray(obs_kf, dtype=np.int32),
        obs_point=np.asarray(obs_lm, dtype=np.int32), obs_uvd=uvd,
        cams=np.array([[camera.cu, camera.cv, camera.fu, camera.fv, -2.0]]), stiff3=S2.reshape(1, 9),
        obs_groups=np.array([[0., 0., float(loss.LOSS_ID), float(getattr(loss, 'k', 0.))]]),
        pose_keys=['T_{}_w'.format(k) for k in range(poses.shape[0])], point_keys=['pt{}_w'.format(j) for j in range(n)]).finalize()


def _reprojection_cost(camera, poses, lp, points=None):
    """Half the sum of the squared pixel residuals of the tables ``lp`` at the given poses (K, 4, 4) and points (lp's own by
    default)."""
    P = (lp.points if points is None else points)[lp.obs_point]
    T = np.asarray(poses)[lp.obs_pose]
    pc = np.einsum('nij,nj->ni', T[:, :3, :3], P) + T[:, :3, 3]
    r = np.stack([camera.fu * pc[:, 0] / pc[:, 2] + camera.cu, camera.fv * pc[:, 1] / pc[:, 2] + camera.cv], axis=1) - lp.obs_uvd[:, :2]
    return 0.5 * float((r * r).sum())


class SparseMonoKeyframe:
    """A keyframe of the monocular pipeline: the image, its pose, its features (``uv`` (n, 2) int32, ``desc`` (n, 32) uint8, as
    ``Matcher.features`` returns them) and ``landmark`` (n,): the landmark every feature is bound to, or -1."""

    def __init__(self, image, T_c_w=None):
        self.image = image
        self.T_c_w = T_c_w
        self.uv = self.desc = self.landmark = None

    def set_features(self, uv, desc):
        self.uv, self.desc = uv, desc
        self.landmark = np.full(uv.shape[0], -1, dtype=np.int64)


class SparseMonoPipeline:
    """Sparse monocular VO pipeline (module docstring)."""

    def __init__(self, camera, first_pose=SE3.identity()):
        self.camera = camera
        """Camera model (MonoCamera)"""
        self.first_pose = first_pose
        """First pose"""
        self.keyframes = []
        """List of keyframes"""
        self.T_c_w = []
        """List of camera poses, one per tracked frame (None: not initialised at that frame)"""
        self.matcher_params = Matcher_parameters()
        """Parameters of the feature matcher"""
        self.matcher = Matcher(self.matcher_params)
        """Feature matcher (device)"""
        self.loss = L2Loss()
        """Loss function of the bundle adjustment"""
        self.mode = 'map'
        """Create new keyframes or localize against existing ones? ['map'|'track']"""
        self.keyframe_rot_thresh = 0.3  # rad
        """Rotational distance threshold to drop new keyframes"""
        self.keyframe_parallax_thresh = 0.05
        """Translation to the active keyframe over the median depth of the tracked landmarks, to drop new keyframes"""
        self.init_baseline = 1.0
        """Distance between the two initial keyframes: the scale of the map"""
        self.init_min_parallax_deg = 1.0
        """Parallax below which a triangulated landmark is refused (initialisation and new landmarks)"""
        self.search_radius = 12
        """Half-width in pixels of the window around a landmark's projection"""
        self.local_window = 5
        """Number of latest keyframes whose landmarks are tracked against and which the bundle adjustment covers"""
        self.local_ba = True
        """Bundle adjustment over the window at every new keyframe"""
        self.ba_options = Options()
        """Optimizer parameters of the bundle adjustment"""
        self.ba_options.allow_nondecreasing_steps = True
        self.ba_options.max_nondecreasing_steps = 3
        self.ba_options.max_iters = 10
        self.init_ransac = EssentialRANSAC(camera)
        """RANSAC of the initialisation (and the epipolar check of new landmarks: its threshold)"""
        self.ransac = PnPRANSAC(camera)
        """RANSAC of the tracking"""
        self.points_w = np.zeros((0, 3))
        self.descriptors = np.zeros((0, 32), dtype=np.uint8)
        self.alive = np.zeros(0, dtype=bool)
        self.obs_kf, self.obs_lm, self.obs_uv = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 2))
        self.ba_history = []
        """Cost history of every bundle adjustment"""
        self.ba_costs = []
        """(start, final) sum of squared pixel residuals / 2 of every bundle adjustment, evaluated on the host from the parameters
        that went in and the ones that came back"""
        self.landmark_counts = []
        """Number of live landmarks after every keyframe"""
        self.relocalise = True
        """Relocalise a frame that cannot be tracked against all live landmarks (False: its ValueError propagates)"""
        self.reloc_ratio = (4, 5)
        """(num, den) of the second-best ratio test of the relocalisation's matching without a prior"""
        self.lost = False
        """The last frame could be neither tracked nor relocalised"""
        self.relocalised = []
        """Indices into ``T_c_w`` of the frames whose pose comes from a relocalisation"""
        self.loop_detection = False
        """Keep every keyframe in the matcher's database and look for a loop at every new keyframe"""
        self.loop_gap = 10
        """Number of newest keyframes that are never queried"""
        self.loop_ratio = (4, 5)
        """(num, den) of the ratio test of the database query and of the verification's matching without a prior"""
        self.loop_closures = []
        """One dict per detected loop: keyframe, entry, scale, T_21 (p_keyframe = scale R p_entry + t), pairs, connected"""
        self.loop_queries = []
        """One dict per query: keyframe, scores, candidates, verified ((entry, counts) per verification)"""
        self.loop_correction = False
        """Correct poses and map with a Sim(3) pose graph over all keyframes whenever a loop closure is recorded"""
        self.loop_min_shared = 15
        """Number of shared landmarks from which two keyframes are joined by a covisibility edge of that graph"""
        self.loop_corrections = []
        """One dict per correction: keyframe, entry, edges, iterations, cost_history, scales (the vertices' scales afterwards)"""
        self.keyframe_frames = []
        """Index into ``T_c_w`` of every keyframe's frame"""

    def set_mode(self, mode):
        """Set the localization mode to ['map'|'track']"""
        self.mode = mode

    # ---- the map ----
    def _add_landmarks(self, points_w, descriptors):
        first = self.points_w.shape[0]
        self.points_w = np.concatenate([self.points_w, points_w])
        self.descriptors = np.concatenate([self.descriptors, descriptors])
        self.alive = np.concatenate([self.alive, np.ones(points_w.shape[0], dtype=bool)])
        return np.arange(first, first + points_w.shape[0])

    def _add_observations(self, kf, lm, uv):
        self.obs_kf = np.concatenate([self.obs_kf, np.full(len(lm), kf, dtype=np.int64)])
        self.obs_lm = np.concatenate([self.obs_lm, np.asarray(lm, dtype=np.int64)])
        self.obs_uv = np.concatenate([self.obs_uv, np.asarray(uv, dtype=np.float64).reshape(-1, 2)])

    def local_landmarks(self):
        """Indices of the live landmarks the last ``local_window`` keyframes see, ascending."""
        first = max(0, len(self.keyframes) - int(self.local_window))
        seen = np.unique(self.obs_lm[self.obs_kf >= first])
        return seen[self.alive[seen]]

    def _flow(self, ref, image):
        self.matcher.pushBack(ref.image)
        self.matcher.pushBack(image)
        self.matcher.matchFeatures(0)
        return self.matcher.matches_array()

    # ---- track ----
    def track(self, image):
        """Track one uint8 image; its pose (SE3, or None before the map exists) is appended to ``T_c_w`` and returned."""
        if not self.keyframes:
            self.keyframes.append(SparseMonoKeyframe(image, self.first_pose))
            self.keyframe_frames.append(len(self.T_c_w))
            self.T_c_w.append(self.first_pose)
            return self.first_pose
        if len(self.keyframes) == 1:
            T = self._initialise(image)
        else:
            T = self._track(image)
        self.T_c_w.append(T)
        return T

    def _initialise(self, image):
        ref = self.keyframes[0]
        m, idx = self._flow(ref, image)
        try:
            T_21, points, status, inliers = bootstrap(self.camera, m[:, 0:2], m[:, 4:6], min_parallax_deg=self.init_min_parallax_deg,
                                                      ransac=self.init_ransac)
        except ValueError:
            return None
        s = float(self.init_baseline)
        T21 = T_21.as_matrix()
        T21[:3, 3] *= s
        T_1w = ref.T_c_w.as_matrix()
        T_w1 = np.linalg.inv(T_1w)
        T_2w = SE3.from_matrix(T21 @ T_1w, normalize=True)
        ok = inliers[status == 0]
        pts_w = (s * points[status == 0]) @ T_w1[:3, :3].T + T_w1[:3, 3]
        ref.set_features(*self._features(0))
        kf = SparseMonoKeyframe(image, T_2w)
        kf.set_features(*self._features(2))
        lm = self._add_landmarks(pts_w, ref.desc[idx[ok, 0]])
        ref.landmark[idx[ok, 0]] = lm
        kf.landmark[idx[ok, 2]] = lm
        self._add_observations(0, lm, m[ok, 0:2])
        self._add_observations(1, lm, m[ok, 4:6])
        self.keyframes.append(kf)
        self.keyframe_frames.append(len(self.T_c_w))
        self.landmark_counts.append(int(self.alive.sum()))
        if self.loop_detection:
            self._db_sync()
        return T_2w

    def _features(self, which):
        uv, _, desc = self.matcher.features(which)
        return uv, desc

    def _track(self, image):
        tracked = None
        if not self.lost:
            T_prior = next(T for T in reversed(self.T_c_w) if T is not None)
            local = self.local_landmarks()
            try:
                tracked = _track(self.camera, self.matcher, image, self.points_w[local], self.descriptors[local], T_prior,
                                 self.search_radius, None, self.ransac)
            except ValueError:
                if not self.relocalise:
                    raise
        if tracked is None:                                    # lost, now or before: against every live landmark, no prior
            local = np.nonzero(self.alive)[0]
            try:
                tracked = _relocalise(self.camera, self.matcher, image, self.points_w[local], self.descriptors[local],
                                      self.reloc_ratio, self.search_radius, None, self.ransac)
            except ValueError:
                self.lost = True
                return None
            self.lost = False
            self.relocalised.append(len(self.T_c_w))
        T_cw, keep, obs, feature = tracked
        lm = local[keep]
        active = self.keyframes[-1]
        T_rel = T_cw.as_matrix() @ np.linalg.inv(active.T_c_w.as_matrix())
        Tm = T_cw.as_matrix()
        depth = np.median((self.points_w[lm] @ Tm[:3, :3].T + Tm[:3, 3])[:, 2])
        parallax = np.linalg.norm(T_rel[:3, 3]) / depth
        rot = np.linalg.norm(SE3.from_matrix(T_rel, normalize=True).log()[3:6])
        if self.mode == 'map' and (parallax > self.keyframe_parallax_thresh or rot > self.keyframe_rot_thresh):
            T_cw = self._new_keyframe(image, T_cw, lm, obs, feature)
        return T_cw

    def _new_keyframe(self, image, T_cw, lm, obs, feature):
        prev = self.keyframes[-1]
        k = len(self.keyframes)
        kf = SparseMonoKeyframe(image, T_cw)
        kf.set_features(*self._features(2))
        kf.landmark[feature] = lm
        self._add_observations(k, lm, obs)
        self.keyframes.append(kf)
        self.keyframe_frames.append(len(self.T_c_w))
        self._new_landmarks(prev, kf, k)
        if self.local_ba and k + 1 >= 3:
            self._bundle_adjust()
        self._drop_behind()
        self.landmark_counts.append(int(self.alive.sum()))
        if self.loop_detection:
            self._detect_loop(k)
        return kf.T_c_w

    # ---- loop detection ----
    def loop_entry(self, k):
        """Keyframe k as an entry of ``loop.verify_loop``: its features, their landmarks in its camera frame (NaN: none, or not
        alive) and the landmarks' indices."""
        kf = self.keyframes[k]
        T = kf.T_c_w.as_matrix()
        bound = kf.landmark >= 0
        bound[bound] = self.alive[kf.landmark[bound]]
        pts = np.full((kf.uv.shape[0], 3), np.nan)
        pts[bound] = self.points_w[kf.landmark[bound]] @ T[:3, :3].T + T[:3, 3]
        return dict(desc=kf.desc, points_c=pts, uv=kf.uv, ids=np.where(bound, kf.landmark, -1))

    def _detect_loop(self, k):
        self._db_sync()
        last = k - int(self.loop_gap)
        if last <= 0:
            return
        state = np.random.get_state()                          # the verification's samples leave the tracking's draws where they were
        try:
            self._query_loop(k, last)
        finally:
            np.random.set_state(state)

    def _db_sync(self):
        while self.matcher.dbSize()[0] < len(self.keyframes):  # entry index = keyframe index
            self.matcher.dbAdd(self.keyframes[self.matcher.dbSize()[0]].desc)

    def _query_loop(self, k, last):
        from pyslam_amd.pipelines.loop import detect_loop
        pipe = self

        class Entries:
            def __getitem__(self, e):
                return pipe.loop_entry(e)
        q = self.loop_entry(k)
        hit = detect_loop(self.camera, self.matcher, self.keyframes[k].image, q['points_c'], Entries(), 0, last, ids_q=q['ids'],
                          ratio=self.loop_ratio)
        query = dict(self.matcher.loop_query_, keyframe=k)
        self.loop_queries.append(query)
        if hit is not None:
            e, scale, T_21, pairs = hit
            self.loop_closures.append(dict(keyframe=k, entry=e, scale=scale, T_21=T_21, pairs=pairs,
                                           connected=query['verified'][-1][1]['connected']))
            if self.loop_correction:
                self.correct_loop_closure(self.loop_closures[-1])

    # ---- loop correction ----
    def covisibility_edges(self):
        """Keyframe pairs (i < j) that share at least ``loop_min_shared`` landmarks, ascending."""
        K = len(self.keyframes)
        order = np.lexsort((self.obs_kf, self.obs_lm))
        lm, kf = self.obs_lm[order], self.obs_kf[order]
        keys = []
        for d in range(1, K):
            same = lm[d:] == lm[:-d]
            if not same.any():
                break
            a, b = kf[:-d][same], kf[d:][same]
            keys.append(a[a != b] * K + b[a != b])
        if not keys:
            return []
        key, count = np.unique(np.concatenate(keys), return_counts=True)
        key = key[count >= int(self.loop_min_shared)]
        return [(int(k // K), int(k % K)) for k in key]

    def landmark_owners(self):
        """The first observing keyframe of every landmark (0 for one without an observation)."""
        owner = np.full(self.points_w.shape[0], len(self.keyframes), dtype=np.int64)
        np.minimum.at(owner, self.obs_lm, self.obs_kf)
        owner[owner == len(self.keyframes)] = 0
        return owner

    def correct_loop_closure(self, closure):
        """The correction step for one closure dict (keyframe, entry, scale, T_21): ``posegraph.correct_loop`` over all keyframes,
        then keyframe poses, landmarks and the frames in between moved; the run is appended to ``loop_corrections``."""
        from pyslam_amd.liegroups import Sim3
        from pyslam_amd.pipelines import posegraph
        old = [Sim3.from_se3(kf.T_c_w) for kf in self.keyframes]
        extra = self.covisibility_edges()
        poses, scales, points = posegraph.correct_loop(
            [kf.T_c_w for kf in self.keyframes], [(closure['entry'], closure['keyframe'], closure['scale'], closure['T_21'])],
            extra_edges=extra, held=(0,), landmark_owner=self.landmark_owners(), points_w=self.points_w)
        graph = posegraph.correct_loop.last_graph
        new = graph.vertices
        frames = np.asarray(self.keyframe_frames)
        for f, T in enumerate(self.T_c_w):
            k = int(np.searchsorted(frames, f, side='right')) - 1
            if T is None or k < 0:
                continue
            if frames[k] == f:
                self.T_c_w[f] = poses[k]
            else:                                              # with its preceding keyframe: the relative similarity is kept
                self.T_c_w[f] = Sim3.from_se3(T).dot(old[k].inv()).dot(new[k]).to_se3()
        for kf, T in zip(self.keyframes, poses):
            kf.T_c_w = T
        self.points_w = points
        self.loop_corrections.append(dict(keyframe=closure['keyframe'], entry=closure['entry'], edges=len(graph.edges),
                                          covisibility=len(extra), iterations=graph.iterations,
                                          cost_history=list(graph.cost_history), scales=scales))

    def _new_landmarks(self, prev, kf, k):
        """Flow matches between the previous keyframe and the new one whose features are bound to no landmark: those that agree
        with the epipolar geometry of the two poses are triangulated and join the map where the status is 0."""
        from pyslam_amd.pipelines.epipolar import essential_from_pose
        from pyslam_amd.problem import triangulate_tables
        m, idx = self._flow(prev, kf.image)
        free = (prev.landmark[idx[:, 0]] < 0) & (kf.landmark[idx[:, 2]] < 0)
        m, idx = m[free], idx[free]
        if m.shape[0] == 0:
            return
        T1, T2 = prev.T_c_w.as_matrix(), kf.T_c_w.as_matrix()
        T_21 = T2 @ np.linalg.inv(T1)
        E = essential_from_pose(T_21[:3, :3], T_21[:3, 3])
        ok = self.init_ransac.compute_ransac_cost(E[None], m[:, 0:2], m[:, 4:6], self.camera, self.init_ransac.ransac_thresh)[0]
        m, idx = m[ok], idx[ok]
        n = m.shape[0]
        if n == 0:
            return
        T_w1 = np.linalg.inv(T1)
        start = np.tile(T_w1[:3, :3] @ np.array([0., 0., 1.]) + T_w1[:3, 3], (n, 1))      # 1 m in front of the previous keyframe
        arange = np.arange(n)
        lp = window_tables(self.camera, np.stack([T1, T2]), [True, True], start, np.repeat([0, 1], n), np.tile(arange, 2),
                           np.concatenate([m[:, 0:2], m[:, 4:6]]))
        points, status = triangulate_tables(lp, 5, self.init_min_parallax_deg)
        good = status == 0
        if not good.any():
            return
        lm = self._add_landmarks(points[good], prev.desc[idx[good, 0]])
        prev.landmark[idx[good, 0]] = lm
        kf.landmark[idx[good, 2]] = lm
        self._add_observations(k - 1, lm, m[good, 0:2])
        self._add_observations(k, lm, m[good, 4:6])

    def _window(self):
        """(first keyframe of the window, landmark indices, observation rows) of the bundle adjustment: the live landmarks with
        at least two observations inside the window, and those observations ordered by keyframe."""
        first = max(0, len(self.keyframes) - int(self.local_window))
        rows = np.nonzero((self.obs_kf >= first) & self.alive[self.obs_lm])[0]
        count = np.bincount(self.obs_lm[rows], minlength=self.points_w.shape[0])
        rows = rows[count[self.obs_lm[rows]] >= 2]
        rows = rows[np.lexsort((self.obs_lm[rows], self.obs_kf[rows]))]
        return first, np.unique(self.obs_lm[rows]), rows

    def _bundle_adjust(self):
        from pyslam_amd.lowering import pose_rows_to_matrices
        from pyslam_amd.problem import solve_tables
        first, lms, rows = self._window()
        K = len(self.keyframes) - first
        if K < 3 or lms.size == 0:
            return
        poses = np.stack([kf.T_c_w.as_matrix() for kf in self.keyframes[first:]])
        held = np.arange(K) < 2                                # the two oldest: gauge and scale
        lp = window_tables(self.camera, poses, held, self.points_w[lms], self.obs_kf[rows] - first,
                           np.searchsorted(lms, self.obs_lm[rows]), self.obs_uv[rows], self.loss)
        history, new_poses, new_points, _ = solve_tables(lp, self.ba_options)
        self.ba_history.append(np.asarray(history, dtype=np.float64))
        Ms = pose_rows_to_matrices(new_poses, 6)
        new_points = np.asarray(new_points, dtype=np.float64).reshape(-1, 3)
        self.ba_costs.append((_reprojection_cost(self.camera, poses, lp), _reprojection_cost(self.camera, Ms, lp, new_points)))
        for j in range(2, K):
            self.keyframes[first + j].T_c_w = SE3.from_matrix(Ms[j], normalize=True)
        self.points_w[lms] = new_points

    def _drop_behind(self):
        """Landmarks that are not in front of every keyframe that observes them leave the map."""
        R = np.stack([kf.T_c_w.as_matrix() for kf in self.keyframes])
        p = self.points_w[self.obs_lm]
        z = np.einsum('nj,nj->n', R[self.obs_kf, 2, :3], p) + R[self.obs_kf, 2, 3]
        bad = np.unique(self.obs_lm[~(z > 0.)])
        self.alive[bad] = False
