"""The sparse VO pipelines on the MI355X: the RGB-D pipeline with its device matcher against the verbatim reference
run (tests/golden/sparse_vo.npz), the stereo pipeline (which the reference cannot run) against a hand composition of
its parts and against the true trajectory, a swapped-in matcher, and RANSAC's failure passed on unchanged."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

from pyslam_amd import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sparse_pipeline_host import GOLDEN, golden_scene, golden_matches  # noqa: E402

pytestmark = pytest.mark.gpu

HALF_STEP = (0.01, -0.005, 0.02, 0.006, 0.0075, -0.003)


class ReplayMatch:
    def __init__(self, row):
        self.u1p, self.v1p, self.u2p, self.v2p, self.u1c, self.v1c, self.u2c, self.v2c = (float(x) for x in row)


class ReplayMatcher:
    """A matcher with the three calls of the reference's, handing out recorded match lists pair by pair."""

    def __init__(self, lists):
        self.lists, self.at, self.pushed, self.modes = list(lists), 0, 0, []

    def pushBack(self, left, right=None):
        self.pushed += 1

    def matchFeatures(self, mode):
        self.modes.append(mode)
        self.current = self.lists[self.at]
        self.at += 1

    def getMatches(self):
        return [ReplayMatch(r) for r in self.current]


def _run_golden_route(g, matcher=None):
    from pyslam.pipelines import SparseRGBDPipeline
    from pyslam.problem import Problem
    from pyslam.sensors import RGBDCamera
    from liegroups import SE3
    images, depth = golden_scene(g)
    cu, cv, fu, fv, w, h = g['cam']
    p = SparseRGBDPipeline(RGBDCamera(cu, cv, fu, fv, int(w), int(h)), SE3.from_matrix(g['T_true'][0]))
    if matcher is not None:
        p.matcher = matcher
    p.keyframe_trans_thresh, p.keyframe_rot_thresh = float(g['trans_thresh']), float(g['rot_thresh'])
    inliers, histories, device_matches = [], [], []
    orig_ransac = p.ransac.perform_ransac

    def perform_ransac():
        out = orig_ransac()
        inliers.append(np.array(out[3]))
        return out
    p.ransac.perform_ransac = perform_ransac
    orig_solve = Problem.solve

    def solve(self):
        out = orig_solve(self)
        histories.append(np.array(self._cost_history, dtype=float))
        return out
    imgs = [images[f] for f in range(images.shape[0])]
    rec = dict(T=[], active=[], n_kf=[], printed=[])
    Problem.solve = solve
    try:
        for k, f in enumerate(g['frame_idx']):
            if k and g['mode'][k] == 'track' and g['mode'][k - 1] == 'map':
                rec['kf_frames'] = [next(j for j in range(len(imgs)) if kf.image is imgs[j]) for kf in p.keyframes]
                p.set_mode('track')
            np.random.seed(int(g['seeds'][k]))
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                p.track(imgs[f], depth[f])
            rec['T'].append(p.T_c_w[-1].as_matrix() if p.T_c_w else np.full((4, 4), np.nan))
            rec['active'].append(p.active_keyframe_idx); rec['n_kf'].append(len(p.keyframes)); rec['printed'].append(buf.getvalue())
            if k and matcher is None:
                device_matches.append(p.matcher.matches_array()[0])
    finally:
        Problem.solve = orig_solve
    rec.update(inliers=inliers, histories=histories, device_matches=device_matches, pipeline=p)
    return rec


def _compare_with_golden(g, rec):
    assert rec['kf_frames'] == list(g['keyframe_frames'])
    assert rec['active'] == list(g['active_idx']) and rec['n_kf'] == list(g['num_keyframes'])
    assert rec['printed'] == [str(s) for s in g['printed']]
    at_i = at_h = 0
    tracked = [k for k in range(len(g['frame_idx'])) if g['match_len'][k] >= 0]
    assert len(rec['inliers']) == len(rec['histories']) == len(tracked)
    for j, k in enumerate(tracked):
        ni, nh = int(g['inlier_len'][k]), int(g['hist_len'][k])
        assert np.array_equal(rec['inliers'][j], g['inlier_flat'][at_i:at_i + ni]), k
        want = g['hist_flat'][at_h:at_h + nh]
        assert rec['histories'][j].shape == want.shape, (k, rec['histories'][j], want)
        print('frame', k, 'inliers', ni, 'cost history rel', np.abs(rec['histories'][j] / want - 1).max())
        np.testing.assert_allclose(rec['histories'][j], want, rtol=1e-9, atol=0)
        at_i += ni; at_h += nh
    T = np.array(rec['T'])
    assert np.array_equal(np.isnan(T), np.isnan(g['T_c_w']))
    ok = ~np.isnan(g['T_c_w'])
    print('max |T - T_ref|', np.abs(T[ok] - g['T_c_w'][ok]).max())
    np.testing.assert_allclose(T[ok], g['T_c_w'][ok], rtol=0, atol=1e-8)


def test_rgbd_pipeline_against_the_verbatim_reference():
    g = np.load(GOLDEN)
    rec = _run_golden_route(g)
    replayed = [m for m in golden_matches(g) if m is not None]
    assert len(rec['device_matches']) == len(replayed)
    for d, h in zip(rec['device_matches'], replayed):
        assert d.shape == h.shape and np.abs(d - h).max() <= 1e-12
    _compare_with_golden(g, rec)
    # one feature pass per new frame: the active keyframe in front of every tracking frame is recognised
    p = rec['pipeline']
    assert p.matcher.feature_passes <= len(g['frame_idx']) + len(g['keyframe_frames']), p.matcher.feature_passes


def test_a_swapped_in_matcher_is_honoured():
    g = np.load(GOLDEN)
    replay = ReplayMatcher([m for m in golden_matches(g) if m is not None])
    rec = _run_golden_route(g, matcher=replay)
    assert replay.at == len(replay.lists) and replay.pushed == 2 * replay.at and set(replay.modes) == {0}
    _compare_with_golden(g, rec)


def test_too_few_inliers_raise_ransacs_error_out_of_track():
    from pyslam.pipelines import SparseRGBDPipeline
    from pyslam.sensors import RGBDCamera
    from liegroups import SE3
    g = np.load(GOLDEN)
    images, depth = golden_scene(g)
    cu, cv, fu, fv, w, h = g['cam']
    rng = np.random.default_rng(0)
    junk = np.full((8, 8), -1.0)
    junk[:, [0, 4]] = rng.uniform(10, 110, (8, 2))
    junk[:, [1, 5]] = rng.uniform(10, 80, (8, 2))
    p = SparseRGBDPipeline(RGBDCamera(cu, cv, fu, fv, int(w), int(h)), SE3.identity())
    p.matcher = ReplayMatcher([junk])
    p.track(images[0], np.full_like(depth[0], 3.0))
    np.random.seed(0)
    with pytest.raises(ValueError, match='RANSAC failed to find more than 5 inliers'):
        p.track(images[1], np.full_like(depth[1], 3.0))
    assert len(p.T_c_w) == 1 and len(p.keyframes) == 1


def test_stereo_pipeline_is_the_composition_of_its_parts_and_follows_the_truth():
    """Every frame's pose is, bit for bit, what FrameToFrameRANSAC and Problem return when composed by hand on the
    pipeline's own obs_0 / obs_1 under the same seed.

    The end point of the 8-frame sequence (96 x 128, baseline 0.12 m, path 0.154 m) is held to 3 x the end-point error
    of the verbatim reference RGB-D route on the same frames with the TRUE depth (measured on the host with the
    featproc matches: 0.0275 m, 0.00558 rad), the factor 3 being the allowance for disparity noise at this baseline:
    0.0825 m and 0.0167 rad.  The scene has ramped cell edges (edge=0.35): its median disparity is 2.7 pixels, so the
    depth rests on the sub-pixel step, and the step-edge texture (edge=0), point-sampled, holds no sub-pixel edge
    position at all (disparity error 0.26 pixel, the median of a uniform +-0.5, whatever the estimator; with ramped
    edges 0.04 pixel).  The same composition on the host (featproc matches, reference RANSAC and Problem) ends at
    0.054 m, 0.0094 rad, and so does the pipeline on the MI355X."""
    from pyslam.pipelines import SparseStereoPipeline, FrameToFrameRANSAC
    from pyslam.problem import Problem
    from pyslam.residuals import ReprojectionMotionOnlyBatchResidual
    from pyslam.sensors import StereoCamera
    from liegroups import SE3
    seq = synthetic.stereo_sequence(96, 128, 8, seed=1, cell=0.3, step=HALF_STEP, edge=0.35)
    cu, cv, fu, fv, b, w, h = seq['cam']
    cam = StereoCamera(cu, cv, fu, fv, b, w, h)
    p = SparseStereoPipeline(cam, SE3.from_matrix(seq['T_c_w'][0]))
    p.keyframe_trans_thresh, p.keyframe_rot_thresh = 0.05, 0.015
    assert p.matcher_mode == 2
    for f in range(8):
        kf = p.keyframes[p.active_keyframe_idx] if p.keyframes else None
        np.random.seed(100 + f)
        with contextlib.redirect_stdout(io.StringIO()):
            p.track(seq['left'][f], seq['right'][f])
        if f == 0:
            continue
        assert p.obs_0.shape == p.obs_1.shape and p.obs_0.shape[0] >= 50 and np.all(p.obs_0[:, 2] > 0) and np.all(p.obs_1[:, 2] > 0)
        np.random.seed(100 + f)
        ransac = FrameToFrameRANSAC(cam)
        ransac.set_obs(p.obs_0, p.obs_1)
        guess, in0, in1, _ = ransac.perform_ransac()
        problem = Problem(p.motion_options)
        problem.add_residual_block(ReprojectionMotionOnlyBatchResidual(cam, in0, in1, p.reprojection_stiffness), ['T_1_0'], loss=p.loss)
        problem.initialize_params({'T_1_0': guess})
        T = problem.solve()['T_1_0']
        T.normalize()
        assert np.array_equal(T.dot(kf.T_c_w).as_matrix(), p.T_c_w[-1].as_matrix()), f
    assert len(p.T_c_w) == 8 and len(p.keyframes) >= 2
    E = p.T_c_w[-1].as_matrix() @ np.linalg.inv(seq['T_c_w'][7])
    trans, rot = np.linalg.norm(E[:3, 3]), np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1))
    print('stereo end point: {:.4f} m, {:.5f} rad (bounds 0.0825 m, 0.0167 rad)'.format(trans, rot))
    assert trans <= 3 * 0.0275 and rot <= 3 * 0.00558
