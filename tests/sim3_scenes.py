"""The committed scenes, seeds and shapes of the similarity-alignment tests (tests/test_sim3_host.py checks the conditions that
tests/test_gpu_sim3.py relies on; both import this module).  Every restatement result is computed once and shared; callers do not
modify what they get.

No seed was refused: synthetic.sim3_scene with SCENE_SEED and the sample tables of SAMPLE_SEED meet every condition on the three
shapes in the three modes (test_sim3_host.test_committed_shapes_meet_the_conditions prints the figures)."""
import functools

import numpy as np

from pyslam_amd import synthetic
from pyslam_amd.pipelines import similarity as sm

CAM = np.array([320., 240., 500., 500., 0.])
THRESH_PIXEL = 9.0
THRESH_METRIC = 0.25
MARGIN = 1e-6            # relative distance of an error from the threshold below which a count could hinge on rounding
RATIO_LIMIT = 1e-4       # hypotheses with sigma_b / sigma_a below it are left out of the comparison of S_all and scales ...
RATIO_CAP = 0.05         # ... and may be at most this share of the non-degenerate hypotheses
SCENE_SEED = 11
SAMPLE_SEED = 5
SHAPES = [(192, 256), (67, 64), (257, 64)]          # (N, H): the test shape, and off / on the 256 stride
MODES = ('pixel', 'metric', 'fixed')                # fixed: metric mode on the scene with scale 1 and fixed_scale on
RANSAC_SEED = 5                                     # np.random.seed of perform_ransac (400 x 192)
EDGE_SIZES = (3, 4, 63, 64, 65, 256, 257)
# the issue's table: best count, hypotheses tied at it, (raw count, final count, rounds adopted, how the loop ended) in pixel mode;
# ties in the metric and the fixed-scale mode
TABLE = {(192, 256): dict(best=135, ties=2, refit=(135, 135, 1, sm.FIXED_POINT), metric_ties=31, fixed_ties=76),
         (67, 64): dict(best=47, ties=2, refit=(47, 47, 1, sm.FIXED_POINT), metric_ties=5, fixed_ties=23),
         (257, 64): dict(best=177, ties=1, refit=(177, 180, 2, sm.FIXED_POINT), metric_ties=7, fixed_ties=20)}

# End to end, the host compositions' errors against the truth (test_sim3_host.test_end_to_end_host_figures prints them and holds
# them against these records; tests/test_gpu_sim3.py holds the device chains to twice these).
# bootstrap (seed 5) -> alignment of its landmarks (seed 5) with the true points: |scale - |t_true||, rotation (rad), |t|
# (measured 8.913e-5, 5.714e-3, 1.568e-2 with 135 of 136 landmarks as inliers; rounded up in the last digit)
BOOT_SEED = 5
BOOT_HOST = dict(scale=8.92e-5, rot=5.72e-3, t=1.57e-2)
# the four keyframes of host_pipeline (240 x 320, local_ba off, seed 8; frames 0 1 5 9) aligned with the scene's T_c_w: the largest
# distance of an aligned camera centre from its true one (measured 7.524e-3 m over a path of 0.75 m, scale 0.10152; the centres lie
# almost on a line, sigma_b / sigma_a = 2.8e-4, so the rotation about that line is the weakly determined part)
TRAJ_HOST = dict(centre=7.53e-3)


def samples_of(n, h, seed=SAMPLE_SEED):
    rs = np.random.RandomState(seed)
    return np.stack([rs.choice(n, 3, replace=False) for _ in range(h)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def scene(n=192, mode='pixel', **kw):
    """(pts_1, pts_2, obs_1, obs_2, scale, T_21 truth, outlier mask) of synthetic.sim3_scene(num_pts=n, seed=SCENE_SEED, **kw); the
    fixed mode's scene has scale 1."""
    if mode == 'fixed':
        kw = dict(kw, scale=1.0)
    return synthetic.sim3_scene(num_pts=n, seed=SCENE_SEED, **kw)


def call_args(mode):
    """(cam or None, thresh, fixed_scale) of a mode."""
    return (CAM, THRESH_PIXEL, False) if mode == 'pixel' else (None, THRESH_METRIC, mode == 'fixed')


def run(sc, mode, samples, refit_iters=3):
    """similarity.ransac on a scene tuple in a mode."""
    cam, thresh, fixed = call_args(mode)
    p1, p2, o1, o2 = sc[:4]
    return sm.ransac(p1, p2, o1 if cam is not None else None, o2 if cam is not None else None, cam, samples, thresh,
                     refit_iters=refit_iters, fixed_scale=fixed)


@functools.lru_cache(maxsize=None)
def oracle(n, h, mode='pixel', refit_iters=3):
    """(samples, similarity.ransac(...)) of a committed shape."""
    samples = samples_of(n, h)
    return samples, run(scene(n, mode), mode, samples, refit_iters)


def draw_samples(n=192, h=400, seed=RANSAC_SEED):
    """What Sim3RANSAC.draw_samples() returns after np.random.seed(seed), written out again."""
    state = np.random.get_state()
    np.random.seed(seed)
    idx = np.random.randint(0, n, (h, 3))
    while True:
        bad = (idx[:, 0] == idx[:, 1]) | (idx[:, 0] == idx[:, 2]) | (idx[:, 1] == idx[:, 2])
        if not bad.any():
            break
        idx[bad] = np.random.randint(0, n, (int(bad.sum()), 3))
    np.random.set_state(state)
    return idx.astype(np.int32)


@functools.lru_cache(maxsize=None)
def seeded_oracle(mode='pixel'):
    samples = draw_samples()
    return samples, run(scene(192, mode), mode, samples)


def in_margin(d, thresh):
    if not np.isfinite(thresh):
        return np.zeros(np.shape(d), dtype=bool)              # an infinite threshold has no neighbourhood
    with np.errstate(invalid='ignore'):
        return np.abs(d - thresh) <= MARGIN * thresh


def conditions(ref, thresh):
    """The figures of one restatement result: pairs in the margin (hypotheses; raw winner, refit rounds and final model), the share
    of non-degenerate hypotheses below the ratio limit, the smallest ratio, the hypotheses tied at the maximum."""
    ok = ~ref['flags']
    near = int(in_margin(ref['d_all'][ok], thresh).sum())
    final = int(in_margin(ref['d'], thresh).sum() + in_margin(ref['d_raw'], thresh).sum() + sum(in_margin(d, thresh).sum() for d in ref['d_rounds']))
    ratio = ref['ratio'][ok]
    return dict(pairs=int(ok.sum()) * ref['d_all'].shape[1], near=near, near_final=final,
                loose=float((ratio < RATIO_LIMIT).mean()) if ratio.size else 0., min_ratio=float(ratio.min()) if ratio.size else np.inf,
                ties=int((ref['counts'] == ref['counts'].max()).sum()))


def kept(ref):
    """The hypotheses whose S_all and scales are compared: not degenerate, and sigma_b / sigma_a not below the limit."""
    with np.errstate(invalid='ignore'):
        return ~ref['flags'] & ~(ref['ratio'] < RATIO_LIMIT)


def rot_angle(Ra, Rb):
    from pyslam_amd.liegroups import SO3
    return float(np.linalg.norm(SO3.from_matrix(Ra @ Rb.T, normalize=True).log()))


def model_error(S, scale, S_ref, scale_ref):
    """(rotation angle, translation, scale) differences of two models."""
    return rot_angle(S[:3, :3] / scale, S_ref[:3, :3] / scale_ref), float(np.abs(S[:3, 3] - S_ref[:3, 3]).max()), abs(scale - scale_ref)


def edge_scene(n):
    """The scene of n points without wrong matches, and a table of 8 samples (N = 3: eight orders of the one set)."""
    return scene(n, 'pixel', outlier_fraction=0.), samples_of(n, 8)


def project(p):
    """The points' own pixels in CAM, as Sim3RANSAC.set_obs computes them."""
    return np.stack([CAM[2] * p[:, 0] / p[:, 2] + CAM[0], CAM[3] * p[:, 1] / p[:, 2] + CAM[1]], axis=1)


def boot_alignment(points, rows, seed=BOOT_SEED):
    """sim3.align_maps(camera, points, two_view_points()[rows], seed=seed) with the restatement: bootstrapped landmarks (frame of
    camera 1, |t_21| = 1) against the true points of the same rows (frame of camera 1, metres)."""
    true = synthetic.two_view_points()[rows]
    return sm.ransac(points, true, project(points), project(true), CAM, draw_samples(points.shape[0], 400, seed), THRESH_PIXEL)


def boot_figures(scale, S):
    """Errors against the truth: the scale is |t_true| of two_view, the rotation and translation are none."""
    s_true = float(np.linalg.norm(synthetic.two_view()[2][:3, 3]))
    return dict(scale=abs(scale - s_true), rot=rot_angle(S[:3, :3] / scale, np.identity(3)), t=float(np.linalg.norm(S[:3, 3])))


@functools.lru_cache(maxsize=None)
def host_boot():
    """mono_scenes.host_bootstrap on synthetic.two_view (np.random.seed(BOOT_SEED)), then boot_alignment."""
    import mono_scenes as ms
    obs_1, obs_2, _, _ = synthetic.two_view()
    state = np.random.get_state()
    np.random.seed(BOOT_SEED)
    T_21, points, status, inl, _ = ms.host_bootstrap(synthetic.TWO_VIEW_CAMERA, obs_1, obs_2, 1.0)
    np.random.set_state(state)
    ok = status == 0
    return boot_alignment(points[ok], inl[ok])


def traj_alignment(poses_est, poses_gt):
    """sim3.align_trajectories(..., convention='Tvw') with the restatement, on world-to-camera 4 x 4 matrices."""
    ce, cg = centres_cw(poses_est), centres_cw(poses_gt)
    n = ce.shape[0]
    return sm.ransac(ce, cg, None, None, None, np.array([[0, n // 2, n - 1]], dtype=np.int32), np.inf, refit_iters=1)


@functools.lru_cache(maxsize=None)
def host_traj():
    """(keyframe poses of mono_scenes.host_pipeline_big, the scene's T_c_w of the same frames, traj_alignment of the two)."""
    import mono_scenes as ms
    hp, seq = ms.host_pipeline_big(), ms.sequence()
    est = np.stack([hp['poses'][f] for f in hp['keyframes']])
    gt = np.stack([seq['T_c_w'][f] for f in hp['keyframes']])
    return est, gt, traj_alignment(est, gt)


def centres_cw(poses):
    """Camera centres -R^T t of world-to-camera 4 x 4 matrices."""
    M = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    return -np.einsum('nji,nj->ni', M[:, :3, :3], M[:, :3, 3])


def traj_figures(S, poses_est, poses_gt):
    """The largest distance of an aligned camera centre (S = [s R | t]: s R c + t) from its true one."""
    c = centres_cw(poses_est) @ S[:3, :3].T + S[:3, 3]
    return float(np.linalg.norm(c - centres_cw(poses_gt), axis=1).max())
