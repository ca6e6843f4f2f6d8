"""Scenes of the triangulation tests (tests/test_triang_host.py, tests/test_gpu_triang.py): the off-box scenes of
tests/offbox_scenes.py at the poses their observations were projected from, and small hand-built tables -- `tracks` (every track
length at which a lane of the kernel's 16-lane group takes another observation), `counts` (landmark counts around the 16-landmark
workgroup, constant landmarks interleaved) and `decisions` (landmarks whose status is known by construction).  Every variable point
of every scene is a sentinel: a triangulation result never comes from the input."""
import functools

import numpy as np

import offbox_scenes as sc
from pyslam_amd import synthetic
from pyslam_amd.lowering import LoweredProblem, pack_pose_matrices

OFFBOX = ('near', 'base', 'far10', 'mm', 'mixed_depth', 'mixed_wave', 'high_group_ids', 'wide_mixed')
STATUS_ONLY = ('far100',)
COUNTS = (1, 15, 16, 17, 33)
COUNTS_CONSTANT = 5                          # constant landmarks interleaved into the largest
HAND_BUILT = ('tracks', 'decisions') + tuple('counts{}'.format(n) for n in COUNTS)
SCENES = OFFBOX + HAND_BUILT                 # everything whose points are compared; far100: statuses only
SENTINELS = ((1e6, -2e6, 3e6), (-7e5, 4e5, -9e6))
PIXEL_NOISE = sc.PIXEL_NOISE

TRACK_LENGTHS = (2, 3, 15, 16, 17, 31, 32, 33, 48, 49, 80)
NUM_ARC_POSES = 80
# the parallax (degrees) between the two ends of the arc as the all-mono tracks' landmarks see it is 40.7 to 50; the largest between
# two observations of which one is among a track's first 16 slots is below 38 for the all-mono tracks of 31 and more (asserted in
# tests/test_triang_host.py): with this minimum those tracks are accepted only through a pair in slots 16 and up
TRACKS_PARALLAX_GATE = 39.4
DECISION_ANGLE_DEG = 1.


def with_sentinel(lp, which=0):
    """A copy whose variable points are all SENTINELS[which]."""
    out = lp.copy()
    out.points = lp.points.copy()
    out.points[lp.point_vid >= 0] = SENTINELS[which]
    return out


def offbox(name):
    lp, truth = sc.scene(name)
    out = lp.copy()
    out.poses = pack_pose_matrices(truth['poses'])
    return with_sentinel(out.finalize())


# ---------------------------------------------------------------------------
# hand-built tables: poses on an arc, all held
# ---------------------------------------------------------------------------
TARGET = np.array([0., 0., 10.])


def look_at(centre, target=TARGET):
    """World-to-camera (4, 4) of a camera at `centre` whose optical axis passes through `target`."""
    z = (target - centre) / np.linalg.norm(target - centre)
    x = np.cross([0., 1., 0.], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    T = np.identity(4)
    T[:3, :3], T[:3, 3] = R, -R @ centre
    return T


def arc_centre(a):
    return TARGET + 10. * np.array([np.sin(a), 0.05 * np.sin(5. * a), -np.cos(a)])


def arc_poses():
    return np.stack([look_at(arc_centre(a)) for a in np.linspace(-0.4, 0.4, NUM_ARC_POSES)])


def middle_out(poses_of_track):
    """The track's poses ordered from the middle of the arc outwards: the two ends of the arc come last."""
    p = np.asarray(poses_of_track)
    return p[np.argsort(np.abs(p - (NUM_ARC_POSES - 1) / 2.), kind='stable')]


class _Builder:
    def __init__(self, poses, seed):
        self.cams, self.stiff3, self.groups = sc._mixed_tables(np.array(synthetic.STEREO_BA_CAMERA[:5]))
        self.poses = list(poses)
        self.rng = np.random.default_rng([seed, 21])
        self.points, self.vid, self.obs = [], [], []          # obs: (pose, point, uvd, group)
        self.nvar = 0

    def pose(self, T):
        self.poses.append(T)
        return len(self.poses) - 1

    def landmark(self, pw, constant=False):
        self.points.append(np.asarray(pw, dtype=float))
        self.vid.append(-1 if constant else self.nvar)
        self.nvar += 0 if constant else 1
        return len(self.points) - 1

    def project(self, pose, pw, group, noise=PIXEL_NOISE):
        T = self.poses[pose]
        pc = T[:3, :3] @ np.asarray(pw, dtype=float) + T[:3, 3]
        cu, cv, fu, fv, b = self.cams[int(self.groups[group, 0])]
        third = 0. if b == -2. else (pc[2] if b == -1. else fu * b / pc[2])
        sigma = np.array([1., 1., 0. if b == -2. else (0.025 / max(noise, 1e-300) if b == -1. else np.sqrt(2.))]) * noise
        return np.array([fu * pc[0] / pc[2] + cu, fv * pc[1] / pc[2] + cv, third]) + sigma * self.rng.standard_normal(3)

    def observe(self, pose, point, group, uvd=None, noise=PIXEL_NOISE, of=None):
        """`point` seen from `pose` through `group`: the projection of `of` (default: the landmark's true point) plus noise,
        or `uvd` as given."""
        if uvd is None:
            uvd = self.project(pose, self.points[point] if of is None else of, group, noise)
        self.obs.append((pose, point, np.asarray(uvd, dtype=float), group))

    def tables(self):
        lp = LoweredProblem(
            dof=6, poses=pack_pose_matrices(np.stack(self.poses)), pose_rid=np.full(len(self.poses), -1, dtype=np.int32),
            points=np.stack(self.points), point_vid=np.array(self.vid, dtype=np.int32),
            obs_pose=np.array([o[0] for o in self.obs], dtype=np.int32), obs_point=np.array([o[1] for o in self.obs], dtype=np.int32),
            obs_uvd=np.stack([o[2] for o in self.obs]), obs_grp=np.array([o[3] for o in self.obs], dtype=np.int32),
            cams=self.cams, stiff3=self.stiff3, obs_groups=self.groups).finalize()
        return lp, np.stack(self.points)


# the groups of offbox_scenes._mixed_tables
STEREO_L2, STEREO_HUBER, RGBD_CAUCHY, RGBD_HUBER, MONO_L1, MONO_HUBER = range(6)


def _random_point(rng):
    return TARGET + rng.uniform(-1., 1., 3) * [1.5, 0.8, 1.5]


@functools.lru_cache(maxsize=None)
def _tracks():
    b = _Builder(arc_poses(), 5)
    rng = np.random.default_rng([5, 22])
    info = []                                                   # (length, depth group or None, mono groups used)
    for grp in (STEREO_L2, RGBD_CAUCHY):                        # one observation that bears depth
        lm = b.landmark(_random_point(rng))
        b.observe(int(rng.integers(0, NUM_ARC_POSES)), lm, grp)
        info.append((1, grp, ()))
    depth_groups = [STEREO_L2, RGBD_HUBER, STEREO_HUBER, RGBD_CAUCHY]
    for k, n in enumerate(TRACK_LENGTHS):
        seen = middle_out(np.round(np.linspace(0, NUM_ARC_POSES - 1, n)).astype(int))
        assert len(set(seen.tolist())) == n
        for with_depth in (False, True):
            # every other length under the smooth loss alone, the others with L1 and Huber observations mixed
            mono = np.full(n, MONO_HUBER) if k % 2 == 0 else rng.choice([MONO_L1, MONO_HUBER], size=n)
            lm = b.landmark(_random_point(rng))
            for q in range(n):
                last_depth = with_depth and q == n - 1
                b.observe(int(seen[q]), lm, depth_groups[k % 4] if last_depth else int(mono[q]))
            info.append((n, depth_groups[k % 4] if with_depth else None, tuple(sorted(set(mono[:n - 1 if with_depth else n].tolist())))))
    lp, truth = b.tables()
    return with_sentinel(lp), truth, tuple(info)


def tracks():
    """-> (tables, true points, info): 80 held poses on an arc; landmark j has info[j] = (track length, the group of the
    depth-bearing observation in its last slot or None, the mono groups of the others).  Observations in table order run from the
    middle of the arc outwards."""
    return _tracks()


@functools.lru_cache(maxsize=None)
def _counts(n):
    """The first n variable landmarks of `base` (and, for the largest n, COUNTS_CONSTANT of its constant ones put between them) with
    their observations, renumbered."""
    lp = offbox('base')
    var, const = np.flatnonzero(lp.point_vid >= 0)[:n], np.flatnonzero(lp.point_vid < 0)[:COUNTS_CONSTANT if n == max(COUNTS) else 0]
    keep = list(var)
    for k, c in enumerate(const):                               # after every sixth variable landmark, from the third on
        keep.insert(3 + 7 * k, c)
    keep = np.array(keep)
    new_of_old = np.full(lp.num_points, -1)
    new_of_old[keep] = np.arange(keep.size)
    rows = np.flatnonzero(new_of_old[lp.obs_point] >= 0)
    out = lp.copy()
    out.points = lp.points[keep]
    is_var = lp.point_vid[keep] >= 0
    out.point_vid = np.where(is_var, np.cumsum(is_var) - 1, -1).astype(np.int32)
    out.obs_pose, out.obs_uvd, out.obs_grp = lp.obs_pose[rows], lp.obs_uvd[rows], lp.obs_grp[rows]
    out.obs_point = new_of_old[lp.obs_point[rows]].astype(np.int32)
    out.point_keys = [lp.point_keys[k] for k in keep] if lp.point_keys else []
    return out.finalize()


def counts(n):
    return _counts(n)


@functools.lru_cache(maxsize=None)
def _decisions():
    """12 ordinary landmarks (tracks of 3 to 6 over the arc, every camera type) and, between them, the constructed ones.  -> (tables,
    dict name -> vid of the constructed landmarks, true points)."""
    b = _Builder(arc_poses(), 6)
    rng = np.random.default_rng([6, 22])
    named = {}

    def ordinary(count):
        for _ in range(count):
            lm = b.landmark(_random_point(rng))
            n = int(rng.integers(3, 7))
            for q, pose in enumerate(rng.choice(NUM_ARC_POSES, size=n, replace=False)):
                b.observe(int(pose), lm, [MONO_HUBER, MONO_HUBER, STEREO_L2, RGBD_HUBER, MONO_HUBER, STEREO_HUBER][q])

    def two_rays(half_angle_deg):
        """Two cameras half_angle_deg to either side of the line from P to a point 10 m in front of it; exact observations."""
        P = _random_point(rng)
        a = np.deg2rad(half_angle_deg)
        c = [P + 10. * np.array([s * np.sin(a), 0., -np.cos(a)]) for s in (-1., 1.)]
        return P, [b.pose(look_at(ck, P + [0.3, -0.2, 0.])) for ck in c]

    ordinary(2)
    # two mono rays at DECISION_ANGLE_DEG
    P, (pa, pb) = two_rays(DECISION_ANGLE_DEG / 2.)
    named['two_rays'] = b.nvar
    lm = b.landmark(P)
    b.observe(pa, lm, MONO_HUBER, noise=0.)
    b.observe(pb, lm, MONO_HUBER, noise=0.)
    # the same with a stereo observation from the first camera (zero parallax with its mono observation)
    named['two_rays_and_stereo'] = b.nvar
    lm = b.landmark(P)
    b.observe(pa, lm, MONO_HUBER, noise=0.)
    b.observe(pb, lm, MONO_HUBER, noise=0.)
    b.observe(pa, lm, STEREO_L2, noise=0.)
    ordinary(2)
    named['one_mono'] = b.nvar
    b.observe(7, b.landmark(_random_point(rng)), MONO_HUBER)
    named['one_stereo'] = b.nvar
    b.observe(11, b.landmark(_random_point(rng)), STEREO_HUBER)
    named['one_rgbd'] = b.nvar
    b.observe(60, b.landmark(_random_point(rng)), RGBD_CAUCHY)
    ordinary(2)
    # rays that diverge in front of the cameras and meet behind them: two cameras side by side, the image positions of a near point
    # swapped (tests/test_mono_host.py: test_triangulation_status_codes)
    left, right = np.identity(4), np.identity(4)
    left[0, 3], right[0, 3] = 0.5, -0.5
    pl, pr = b.pose(left), b.pose(right)
    named['behind'] = b.nvar
    lm = b.landmark([0., 0., 2.])
    b.observe(pl, lm, MONO_HUBER, uvd=b.project(pr, [0., 0., 2.], MONO_HUBER, 0.))
    b.observe(pr, lm, MONO_HUBER, uvd=b.project(pl, [0., 0., 2.], MONO_HUBER, 0.))
    # a disparity of exactly zero, alone; a negative one beside a mono pair
    named['zero_disparity'] = b.nvar
    lm = b.landmark(_random_point(rng))
    uvd = b.project(20, b.points[lm], STEREO_L2, 0.)
    b.observe(20, lm, STEREO_L2, uvd=[uvd[0], uvd[1], 0.])
    ordinary(2)
    named['negative_disparity'] = b.nvar
    lm = b.landmark(_random_point(rng))
    b.observe(10, lm, MONO_HUBER)
    b.observe(70, lm, MONO_HUBER)
    uvd = b.project(40, b.points[lm], STEREO_HUBER, 0.)
    b.observe(40, lm, STEREO_HUBER, uvd=[uvd[0], uvd[1], -0.4])
    # 18 mono observations: 16 from one camera, then one from 0.6 degrees to either side of it -- only the pair in slots 16 and 17
    # has the parallax (1.2 degrees) that a minimum of DECISION_ANGLE_DEG asks for
    P, (pa, pb) = two_rays(0.6 * DECISION_ANGLE_DEG)
    mid = b.pose(look_at(P + [0., 0., -10.], P + [0.3, -0.2, 0.]))
    named['late_pair'] = b.nvar
    lm = b.landmark(P)
    for _ in range(16):
        b.observe(mid, lm, MONO_HUBER, noise=0.)
    b.observe(pa, lm, MONO_HUBER, noise=0.)
    b.observe(pb, lm, MONO_HUBER, noise=0.)
    ordinary(4)
    lp, truth = b.tables()
    return with_sentinel(lp), named, truth


def decisions():
    return _decisions()


def scene(name):
    """The tables of any scene by name (points: SENTINELS[0])."""
    if name in OFFBOX + STATUS_ONLY:
        return _offbox_cached(name)
    if name == 'tracks':
        return tracks()[0]
    if name == 'decisions':
        return decisions()[0]
    return counts(int(name[len('counts'):]))


@functools.lru_cache(maxsize=None)
def _offbox_cached(name):
    return offbox(name)


def obs_camera(lp):
    return lp.cams[lp.obs_groups[lp.obs_grp, 0].astype(int), 4]


def track_lengths(lp):
    """Observations per variable landmark, by vid."""
    vid = lp.point_vid[lp.obs_point]
    return np.bincount(vid[vid >= 0], minlength=lp.num_var_points)


def ray_angles_deg(lp, vid):
    """(n, n) angles between the viewing rays of the n observations of variable landmark `vid`, in slot (table) order."""
    point = np.flatnonzero(lp.point_vid == vid)[0]
    rows = np.flatnonzero(lp.obs_point == point)
    cu, cv, fu, fv, _ = lp.cams[lp.obs_groups[lp.obs_grp[rows], 0].astype(int)].T
    d = np.stack([(lp.obs_uvd[rows, 0] - cu) / fu, (lp.obs_uvd[rows, 1] - cv) / fv, np.ones(rows.size)], axis=1)
    d = np.einsum('nji,nj->ni', lp.poses[lp.obs_pose[rows], :9].reshape(-1, 3, 3), d)
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.degrees(np.arccos(np.clip(d @ d.T, -1., 1.)))


def has_loss(lp, loss_id):
    """Per variable landmark (by vid): does one of its observations have this loss?"""
    vid = lp.point_vid[lp.obs_point]
    m = (vid >= 0) & (lp.obs_groups[lp.obs_grp, 2] == loss_id)
    return np.bincount(vid[m], minlength=lp.num_var_points) > 0


def has_stereo(lp):
    vid = lp.point_vid[lp.obs_point]
    m = (vid >= 0) & (obs_camera(lp) >= 0)
    return np.bincount(vid[m], minlength=lp.num_var_points) > 0
