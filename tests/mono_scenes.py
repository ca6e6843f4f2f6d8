"""The committed scenes, seeds and host chains of the monocular tracking tests (tests/test_mono_track_host.py checks the conditions
that tests/test_gpu_mono_track.py relies on; both import this module).  Every restatement result is computed once and shared;
callers do not modify what they get.

Three things are written out here with the restatements only (featproc, epipolar, absolute, triangulation), no device call:
``host_chain`` (frames 1-9 of the 240 x 320 scene tracked against frame 0's features at their true depth), ``HostMatcher`` (the
Matcher's interface over featproc) and ``host_pipeline`` (SparseMonoPipeline's control flow with ``local_ba`` off)."""
import functools

import numpy as np

import pnp_scenes as sc
from pyslam_amd import synthetic, triangulation
from pyslam_amd.liegroups import SE3, SO3
from pyslam_amd.pipelines import absolute as ab
from pyslam_amd.pipelines import epipolar as ep
from pyslam_amd.pipelines import featproc as fp

BIG = dict(h=240, w=320, n_frames=10, seed=0, step=(0.08, -0.01, 0.02, 0.004, -0.012, 0.003), edge=0.35)
SMALL_SHAPES = [(96, 128), (101, 139)]
SMALL_FRAMES = (1, 7)
SMALL_RADII = (0, 1, 8, 40)
CHAIN_RADII = (12, 6)
CHAIN_SEED = 5                      # frame f of the chain is registered with np.random.seed(CHAIN_SEED + f)
# np.random.seed once, in front of the first track().  Seed 7 was refused by the margin test: at its frames 6 and 9 the refinement is not
# kept, the raw P3P pose reprojects its three sample points onto their observations exactly, one of them has the sub-pixel offset 0.5
# exactly (c_0 = c_+), and as the next frame's prior that pose puts the point 9e-13 pixel from a rounding boundary.
PIPELINE_SEED = 8
THRESH = 4.0
ROUND_MARGIN = 1e-6                 # pixels between a projected coordinate + 0.5 and the integer at which its window centre flips
MIN_TRACKED = 0.80                  # share of the map with status 0 in every frame of the chain (the issue's bound)
# truth bounds of the chain: twice the maxima measured with the final restatement over frames 1-9, rounded up in the last digit
# (radius 12: 0.0307 m / 0.331 deg, radius 6: 0.0202 m / 0.237 deg)
TRUTH_BOUND = {12: (2 * 0.0308, 2 * 0.332), 6: (2 * 0.0202, 2 * 0.238)}


def rot_angle(Ra, Rb):
    return float(np.linalg.norm(SO3.from_matrix(Ra @ Rb.T, normalize=True).log()))


def cam5(cam):
    return np.array([cam[0], cam[1], cam[2], cam[3], 0.])


def camera(cam):
    from pyslam_amd.sensors import MonoCamera
    return MonoCamera(cam[0], cam[1], cam[2], cam[3], int(cam[4]), int(cam[5]))


@functools.lru_cache(maxsize=None)
def sequence(h=None, w=None):
    """The 240 x 320 scene, or a small one of the default trajectory (8 frames)."""
    if h is None:
        return synthetic.mono_sequence(**BIG)
    return synthetic.mono_sequence(h, w, 8, seed=0)


@functools.lru_cache(maxsize=None)
def frames(h=None, w=None):
    return [fp.features(im, fp.Params()) for im in sequence(h, w)['images']]


@functools.lru_cache(maxsize=None)
def true_map(h=None, w=None):
    """(points_w (N, 3), descriptors (N, 32)): frame 0's features at their true depth."""
    seq, f0 = sequence(h, w), frames(h, w)[0]
    cu, cv, fu, fv = seq['cam'][:4]
    u, v = f0.uv[:, 0], f0.uv[:, 1]
    z = seq['depth'][0][v, u]
    p = np.stack([(u - cu) * z / fu, (v - cv) * z / fv, z], axis=1)
    Ti = np.linalg.inv(seq['T_c_w'][0])
    return p @ Ti[:3, :3].T + Ti[:3, 3], f0.desc


def projection(points_w, T, cam):
    """(u, v, z_c) of step 8's projection, in its order of operations."""
    X, Y, Z = points_w[:, 0], points_w[:, 1], points_w[:, 2]
    with np.errstate(all='ignore'):
        xc = ((T[0, 0] * X + T[0, 1] * Y) + T[0, 2] * Z) + T[0, 3]
        yc = ((T[1, 0] * X + T[1, 1] * Y) + T[1, 2] * Z) + T[1, 3]
        zc = ((T[2, 0] * X + T[2, 1] * Y) + T[2, 2] * Z) + T[2, 3]
        return (cam[2] * xc) / zc + cam[0], (cam[3] * yc) / zc + cam[1], zc


def rounding_margin(points_w, T, cam):
    """Smallest distance of u + 0.5 or v + 0.5 from an integer over the points in front of the camera whose projection lies in the
    image or within a pixel and a half of it (further out both neighbouring centres are outside the image: status 1 either way)."""
    u, v, zc = projection(points_w, T, cam)
    w, h = cam[4], cam[5]
    with np.errstate(invalid='ignore'):
        ok = (zc > 0.) & (u >= -1.5) & (u <= w + 0.5) & (v >= -1.5) & (v <= h + 0.5)
    if not ok.any():
        return np.inf
    x = np.concatenate([u[ok], v[ok]]) + 0.5
    return float(np.abs(x - np.round(x)).min())


def brute_force(frame, points_w, descriptors, T, cam, radius, cost_max):
    """Step 8's search without row_start, over every feature: (best feature or -1, its cost or -1, number of points whose minimum
    cost is reached by more than one candidate) -- before the one-landmark-per-feature step."""
    h, w = frame.du.shape
    u, v, zc = projection(points_w, T, cam)
    N = points_w.shape[0]
    best, cost, tied = np.full(N, -1, dtype=np.int64), np.full(N, -1, dtype=np.int64), 0
    fd = frame.desc.astype(np.int64)
    for i in range(N):
        if not (zc[i] > 0. and np.isfinite([u[i], v[i], zc[i]]).all()):
            continue
        ui, vi = np.floor(u[i] + 0.5), np.floor(v[i] + 0.5)
        if not (0 <= ui < w and 0 <= vi < h):
            continue
        cand = np.nonzero((np.abs(frame.uv[:, 0] - ui) <= radius) & (np.abs(frame.uv[:, 1] - vi) <= radius))[0]
        if cand.size == 0:
            continue
        c = np.abs(fd[cand] - descriptors[i].astype(np.int64)).sum(axis=1)
        tied += int((c == c.min()).sum() > 1)
        if c.min() <= cost_max:
            best[i], cost[i] = cand[np.flatnonzero(c == c.min())[0]], c.min()      # ties: the lower index
    return best, cost, tied


def register(points, obs, cam, seed, min_inliers=12):
    """pnp.register_frame with the restatement: (T_cw normalised as SE3.from_matrix does, inlier indices, absolute.ransac's result)."""
    if points.shape[0] < 3:
        raise ValueError('fewer than 3 correspondences')
    samples = sc.ransac_samples(points.shape[0], 400, seed) if seed is not None else \
        np.stack([np.random.choice(points.shape[0], 3, replace=False) for _ in range(400)]).astype(np.int32)
    res = ab.ransac(points, obs, cam5(cam), samples, THRESH)
    if res['count'] < min_inliers:
        raise ValueError('too few inliers')
    return SE3.from_matrix(res['T_cw'], normalize=True).as_matrix(), np.nonzero(res['mask'])[0], res


def host_track(frame, points_w, descriptors, T_prior, cam, radius, seed, min_inliers=12):
    """mono.track_frame with the restatements -> dict: T, keep (landmark indices), obs, feature, status, match (the full match_map
    result that was used), res (absolute.ransac's), radius (the one that was used)."""
    out = fp.match_map(frame, points_w, descriptors, T_prior, cam, radius)
    used = radius
    if int((out[1] == 0).sum()) < min_inliers:
        used = 2 * radius
        out = fp.match_map(frame, points_w, descriptors, T_prior, cam, used)
    feature, status, _, uv = out
    idx = np.nonzero(status == 0)[0]
    T, inl, res = register(points_w[idx], uv[idx], cam, seed, min_inliers)
    keep = idx[inl]
    return dict(T=T, keep=keep, obs=uv[keep], feature=feature[keep], status=status, match=out, res=res, radius=used, matched=idx)


@functools.lru_cache(maxsize=None)
def host_chain(radius):
    """Frames 1-9 of the 240 x 320 scene against the true map, each with the previous frame's pose as prior (frame 1: the truth of
    frame 0).  -> list of host_track results with the prior and the errors against the truth (metres, degrees)."""
    seq, fr = sequence(), frames()
    pts, desc = true_map()
    T = seq['T_c_w'][0].copy()
    out = []
    for f in range(1, len(fr)):
        r = host_track(fr[f], pts, desc, T, seq['cam'], radius, CHAIN_SEED + f)
        Tt = seq['T_c_w'][f]
        r.update(prior=T, frame=f, e_t=float(np.linalg.norm(r['T'][:3, 3] - Tt[:3, 3])),
                 e_rot_deg=float(np.degrees(rot_angle(r['T'][:3, :3], Tt[:3, :3]))))
        out.append(r)
        T = r['T']
    return out


class HostMatcher:
    """pushBack / matchFeatures / matches_array of a Matcher over featproc: a two-frame window of single images (host_pipeline reads the
    two Frames themselves where the pipeline calls Matcher.features)."""

    def __init__(self):
        self.params = fp.Params()
        self._cache, self._prev, self._cur, self._map = {}, None, None, None

    def pushBack(self, image):
        key = image.tobytes()
        if key not in self._cache:
            self._cache[key] = fp.features(image, self.params)
        self._prev, self._cur = self._cur, self._cache[key]

    def matchFeatures(self, mode):
        self._m = fp.match((self._prev, None), (self._cur, None), mode, self.params)

    def matches_array(self):
        return self._m


def host_bootstrap(cam, obs_1, obs_2, min_parallax_deg, min_inliers=16):
    """twoview.bootstrap with the restatements (samples from np.random as EssentialRANSAC.draw_samples draws them)."""
    from pyslam_amd.pipelines.twoview import two_view_tables
    n = obs_1.shape[0]
    if n < 8:
        raise ValueError('fewer than 8 correspondences')
    samples = np.stack([np.random.choice(n, 8, replace=False) for _ in range(400)]).astype(np.int32)
    res = ep.ransac(obs_1, obs_2, cam5(cam), samples, THRESH)
    if res['count'] < min_inliers:
        raise ValueError('too few inliers')
    inliers = np.nonzero(res['mask'])[0]
    T_21 = SE3.from_matrix(res['T_21'], normalize=True).as_matrix()
    points, status = triangulation.triangulate_tables(two_view_tables(camera(cam), T_21, obs_1[inliers], obs_2[inliers]), 5, min_parallax_deg)
    if int((status == 0).sum()) < min_inliers:
        raise ValueError('too few landmarks')
    return T_21, points, status, inliers, res


@functools.lru_cache(maxsize=None)
def widened_case():
    """track_frame's second attempt: frame 1 of the 240 x 320 scene with a prior rotated by 0.0174 rad (5 pixels and more), radius 3
    and min_inliers = 500 -- 238 points match at radius 3, 677 at radius 6.  -> (T_prior, host_track's result)."""
    seq, fr = sequence(), frames()
    pts, desc = true_map()
    T_prior = SE3.exp(np.array([0., 0., 0., 0., 0.0174, 0.])).as_matrix() @ seq['T_c_w'][1]
    return T_prior, host_track(fr[1], pts, desc, T_prior, seq['cam'], 3, 11, min_inliers=500)


@functools.lru_cache(maxsize=None)
def host_pipeline_big():
    seq = sequence()
    return host_pipeline(seq['images'], seq['cam'])


def host_pipeline(images, cam, seed=PIPELINE_SEED, radius=12, window=5, parallax_thresh=0.05, rot_thresh=0.3, min_parallax_deg=1.0,
                  baseline=1.0):
    """SparseMonoPipeline.track over `images` with ``local_ba`` off, written out with the restatements.  -> dict: poses (list of
    4 x 4 or None, one per image), keyframes (image index of every keyframe), counts (live landmarks after every keyframe),
    init_frame, checks (per decision that a rounding could flip: the frame, what, and its margin figures)."""
    from pyslam_amd.pipelines.mono import window_tables
    np.random.seed(seed)
    m = HostMatcher()
    poses, kf_frame, counts = [np.identity(4)], [0], []
    kf_pose, kf_feat, kf_lm = [np.identity(4)], [None], [None]              # per keyframe: pose, Frame, landmark of every feature
    P, D = np.zeros((0, 3)), np.zeros((0, 32), dtype=np.uint8)
    okf, olm, ouv = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 2))
    alive = np.zeros(0, dtype=bool)
    init_frame = None
    checks = []

    def add_obs(k, lm, uv):
        nonlocal okf, olm, ouv
        okf, olm, ouv = np.concatenate([okf, np.full(len(lm), k)]), np.concatenate([olm, lm]), np.concatenate([ouv, uv])

    def add_lm(p, d):
        nonlocal P, D, alive
        first = P.shape[0]
        P, D, alive = np.concatenate([P, p]), np.concatenate([D, d]), np.concatenate([alive, np.ones(p.shape[0], dtype=bool)])
        return np.arange(first, first + p.shape[0])

    for f in range(1, len(images)):
        if len(kf_frame) == 1:                                               # initialising
            m.pushBack(images[0]); m.pushBack(images[f]); m.matchFeatures(0)
            mm, idx = m.matches_array()
            try:
                T_21, points, status, inl, res = host_bootstrap(cam, mm[:, 0:2], mm[:, 4:6], min_parallax_deg)
                checks.append(dict(frame=f, what='bootstrap', near=int(sc.in_margin(res['dist']).sum() + sc.in_margin(res['d']).sum())))
            except ValueError:
                poses.append(None)
                continue
            T_21[:3, 3] *= baseline
            T2 = SE3.from_matrix(T_21, normalize=True).as_matrix()
            ok = inl[status == 0]
            kf_feat[0], kf_feat_new = m._prev, m._cur
            kf_lm[0] = np.full(len(m._prev), -1, dtype=np.int64)
            lm_new = np.full(len(m._cur), -1, dtype=np.int64)
            lm = add_lm(baseline * points[status == 0], m._prev.desc[idx[ok, 0]])
            kf_lm[0][idx[ok, 0]] = lm
            lm_new[idx[ok, 2]] = lm
            add_obs(0, lm, mm[ok, 0:2]); add_obs(1, lm, mm[ok, 4:6])
            kf_pose.append(T2); kf_feat.append(kf_feat_new); kf_lm.append(lm_new); kf_frame.append(f)
            counts.append(int(alive.sum()))
            poses.append(T2)
            init_frame = f
            continue
        # tracking
        prior = next(T for T in reversed(poses) if T is not None)
        first = max(0, len(kf_frame) - window)
        local = np.unique(olm[okf >= first])
        local = local[alive[local]]
        m.pushBack(images[f])
        r = host_track(m._cur, P[local], D[local], prior, cam, radius, None)
        T, lm = r['T'], local[r['keep']]
        cond = sc.conditions(r['res'])
        checks.append(dict(frame=f, what='track', margin=rounding_margin(P[local], prior, cam), near=cond['near'] + cond['near_final']))
        T_rel = T @ np.linalg.inv(kf_pose[-1])
        depth = np.median((P[lm] @ T[:3, :3].T + T[:3, 3])[:, 2])
        parallax = np.linalg.norm(T_rel[:3, 3]) / depth
        rot = np.linalg.norm(SE3.from_matrix(T_rel, normalize=True).log()[3:6])
        poses.append(T)
        if not (parallax > parallax_thresh or rot > rot_thresh):
            continue
        # new keyframe
        k = len(kf_frame)
        cur = m._cur
        lm_new = np.full(len(cur), -1, dtype=np.int64)
        lm_new[r['feature']] = lm
        add_obs(k, lm, r['obs'])
        m.pushBack(images[kf_frame[-1]]); m.pushBack(images[f]); m.matchFeatures(0)
        mm, idx = m.matches_array()
        free = (kf_lm[-1][idx[:, 0]] < 0) & (lm_new[idx[:, 2]] < 0)
        mm, idx = mm[free], idx[free]
        if mm.shape[0]:
            T1 = kf_pose[-1]
            E = ep.essential_from_pose(T_rel[:3, :3], T_rel[:3, 3])
            c5 = cam5(cam)
            ok, d = ep.score(E, ep.normalise(mm[:, 0:2], c5), ep.normalise(mm[:, 4:6], c5), c5, THRESH)
            checks.append(dict(frame=f, what='epipolar check', near=int(sc.in_margin(d).sum())))
            mm, idx = mm[ok], idx[ok]
            n = mm.shape[0]
            if n:
                Ti = np.linalg.inv(T1)
                start = np.tile(Ti[:3, :3] @ np.array([0., 0., 1.]) + Ti[:3, 3], (n, 1))
                lp = window_tables(camera(cam), np.stack([T1, T]), [True, True], start, np.repeat([0, 1], n), np.tile(np.arange(n), 2),
                                   np.concatenate([mm[:, 0:2], mm[:, 4:6]]))
                pts, st = triangulation.triangulate_tables(lp, 5, min_parallax_deg)
                good = st == 0
                if good.any():
                    new = add_lm(pts[good], kf_feat[-1].desc[idx[good, 0]])
                    kf_lm[-1][idx[good, 0]] = new
                    lm_new[idx[good, 2]] = new
                    add_obs(k - 1, new, mm[good, 0:2]); add_obs(k, new, mm[good, 4:6])
        kf_pose.append(T); kf_feat.append(cur); kf_lm.append(lm_new); kf_frame.append(f)
        Rz = np.stack(kf_pose)[okf]
        z = np.einsum('nj,nj->n', Rz[:, 2, :3], P[olm]) + Rz[:, 2, 3]
        alive[np.unique(olm[~(z > 0.)])] = False
        counts.append(int(alive.sum()))
    return dict(poses=poses, keyframes=kf_frame, counts=counts, init_frame=init_frame, points=P, alive=alive, checks=checks)
