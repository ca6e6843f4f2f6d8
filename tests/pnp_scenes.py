"""The committed scenes, seeds and shapes of the absolute-pose tests (tests/test_pnp_host.py checks the conditions that
tests/test_gpu_pnp.py relies on; both import this module).  Every restatement result is computed once and shared; callers do not
modify what they get."""
import functools

import numpy as np

from pyslam_amd import synthetic
from pyslam_amd.pipelines import absolute as ab

CAM = np.array([320., 240., 500., 500., -2.])
THRESH = 4.0
MARGIN = 1e-6            # relative distance of a squared error from the threshold below which a count could hinge on rounding
BRANCH = 1e-9            # the same for a branch decision of the minimal solver
SENS_LIMIT = 1e-10       # slots above it are left out of the comparison of T_all ...
SENS_CAP = 0.05          # ... and may be at most this share of the non-empty slots
SCENE_SEED = 11
SAMPLE_SEED = 5
SHAPES = [(192, 256), (67, 64), (257, 64)]          # (N, H): the test shape, and off / on the 256 stride
SINGLE = (192, 256, 143)                            # a single hypothesis: row 143 of the (192, 256) table
RANSAC_SEED = 5                                     # np.random.seed of perform_ransac (400 x 192)


def samples_of(n, h, seed=SAMPLE_SEED):
    rs = np.random.RandomState(seed)
    return np.stack([rs.choice(n, 3, replace=False) for _ in range(h)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def scene(n=192, **kw):
    """(pts_w, obs, T truth, outlier mask) of synthetic.pnp_scene(num_pts=n, seed=SCENE_SEED, **kw)."""
    return synthetic.pnp_scene(num_pts=n, seed=SCENE_SEED, **dict(kw))


@functools.lru_cache(maxsize=None)
def oracle(n, h, refine=True):
    """(samples, absolute.ransac(...) with sensitivities) of a committed shape."""
    pts, obs, _, _ = scene(n)
    samples = samples_of(n, h)
    return samples, ab.ransac(pts, obs, CAM, samples, THRESH, refine_winner=refine, sensitivity=True)


def ransac_samples(n=192, h=400, seed=RANSAC_SEED):
    """What PnPRANSAC.draw_samples() returns after np.random.seed(seed)."""
    state = np.random.get_state()
    np.random.seed(seed)
    out = np.stack([np.random.choice(n, 3, replace=False) for _ in range(h)]).astype(np.int32)
    np.random.set_state(state)
    return out


@functools.lru_cache(maxsize=None)
def seeded_oracle(refine=True):
    pts, obs, _, _ = scene(192)
    samples = ransac_samples()
    return samples, ab.ransac(pts, obs, CAM, samples, THRESH, refine_winner=refine, sensitivity=True)


def in_margin(d, thresh=THRESH):
    with np.errstate(invalid='ignore'):
        return np.abs(d - thresh) <= MARGIN * thresh


def conditions(ref):
    """The figures of one restatement result: pairs in the margin, the smallest branch margin, the share of non-empty slots
    above the sensitivity limit, and whether the winner is unique."""
    ne = ~ref['empty']
    near = int(in_margin(ref['d_all'][ne]).sum())
    final = int((in_margin(ref['d']) | in_margin(ref['d_raw']) | (in_margin(ref['d_refined']) if ref['d_refined'] is not None else False)).sum())
    sens = ref['sensitivity'][ne]
    best = ref['counts'].max(axis=1)
    return dict(pairs=int(ne.sum()) * ref['d_all'].shape[2], near=near, near_final=final, branch=float(ref['margins'].min()),
                loose=float((sens > SENS_LIMIT).mean()) if sens.size else 0., worst_sens=float(sens.max()) if sens.size else 0.,
                unique=int((best == best.max()).sum()) == 1)


def minimal_four():
    """Four exact points and the sample of the first three: the fourth point picks the slot.  -> (pts, obs, T truth, samples)."""
    pts, obs, T, _ = scene(4, pixel_noise=0., outlier_fraction=0.)
    return pts, obs, T, np.array([[0, 1, 2]], dtype=np.int32)
