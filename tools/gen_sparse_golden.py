#!/usr/bin/env python
"""Generate tests/golden/sparse_vo.npz by running the VERBATIM reference sparse RGB-D pipeline.

TEST INFRASTRUCTURE -- authoring machine only, like tools/gen_dense_golden.py, whose path set-up (oracle/gen_golden.py:
the reference first on sys.path, the numba stand-in) it shares.  Run from the repository root:

    python tools/gen_sparse_golden.py

The reference's pipelines/sparse.py, keyframes.py and ransac.py are loaded by path with two stand-in modules: ``cv2``
(imported by the reference, never called on this route) and ``viso2``, whose ``Matcher`` hands the pipeline the match
lists the numpy restatement of this project's matcher (pyslam_amd/pipelines/featproc.py) produces for each pushed
frame pair -- libviso2 itself is on no machine of ours and is not what this project reproduces.
Everything downstream of the match list is the reference: observations, pruning, FrameToFrameRANSAC, the motion-only
Problem, the keyframe logic.

The pipeline runs over the left images and depth of synthetic.stereo_sequence (with seeded holes in the depth) in
'map' mode with lowered keyframe thresholds, then re-localises a few frames in 'track' mode, with
``np.random.seed(k)`` before the k-th ``track``.  Recorded: the generator arguments and a checksum of the inputs (not
the images), the match list of every frame, every T_c_w, the keyframe frame indices, the active keyframe index after
each frame, the RANSAC inlier indices and the Problem._cost_history of each frame, the printed lines and the class
surface (attributes and defaults).  The tests read only the .npz.
"""
import contextlib
import hashlib
import importlib.util
import io
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as gg  # noqa: E402  (puts the reference first on sys.path)

import numpy as np  # noqa: E402

from pyslam_amd import synthetic  # noqa: E402
from pyslam_amd.pipelines import featproc  # noqa: E402

H, W, N_MAP, SEED, CELL = 96, 128, 8, 1, 0.3
STEP = (0.01, -0.005, 0.02, 0.006, 0.0075, -0.003)
HOLE_FRACTION = 0.01
TRACK_FRAMES = [1, 2, 3, 4, 5]
TRANS_THRESH, ROT_THRESH = 0.05, 0.015


def scene():
    """The golden's inputs: left images and depth of the textured scene, the depth with seeded NaN / 0 holes."""
    seq = synthetic.stereo_sequence(H, W, N_MAP, seed=SEED, cell=CELL, step=STEP)
    holes = np.random.default_rng(SEED + 1000).random(seq['depth'].shape)
    depth = seq['depth'].copy()
    depth[holes < HOLE_FRACTION] = np.nan
    depth[(holes >= HOLE_FRACTION) & (holes < 2 * HOLE_FRACTION)] = 0.
    cu, cv, fu, fv, b, w, h = seq['cam']
    return dict(images=seq['left'], depth=depth, cam=(cu, cv, fu, fv, w, h), T_c_w=seq['T_c_w'])


def checksum(sc):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(sc['images']).tobytes())
    h.update(np.ascontiguousarray(sc['depth']).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


class HostMatch:
    def __init__(self, row):
        self.u1p, self.v1p, self.u2p, self.v2p, self.u1c, self.v1c, self.u2c, self.v2c = (float(x) for x in row)


class HostMatcher:
    """The ``viso2.Matcher`` stand-in: featproc on the last two pushed frames; keeps every match list it handed out."""

    def __init__(self, params=None):
        self.params = featproc.Params()
        self.frames = []
        self.log = []

    def setIntrinsics(self, *args):
        pass

    def pushBack(self, left, right=None):
        self.frames = (self.frames + [(left, right)])[-2:]

    def matchFeatures(self, mode):
        fr = [(featproc.features(l, self.params), featproc.features(r, self.params) if r is not None else None)
              for l, r in self.frames]
        self.matches = featproc.match(fr[0], fr[1], mode, self.params)[0]
        self.log.append(self.matches)

    def getMatches(self):
        return [HostMatch(r) for r in self.matches]


def install_stand_ins():
    sys.modules['cv2'] = types.ModuleType('cv2')
    viso2 = types.ModuleType('viso2')
    viso2.Matcher_parameters = featproc.Params
    viso2.Matcher = HostMatcher
    sys.modules['viso2'] = viso2


def load_reference_pipeline():
    import pyslam
    assert pyslam.__file__.startswith(gg.REF), pyslam.__file__
    pkg = types.ModuleType('pyslam.pipelines')                # without the package __init__ (it imports every pipeline)
    pkg.__path__ = [os.path.join(gg.REF, 'pyslam', 'pipelines')]
    sys.modules['pyslam.pipelines'] = pkg
    mods = {}
    for name in ('keyframes', 'ransac', 'sparse'):
        spec = importlib.util.spec_from_file_location('pyslam.pipelines.' + name,
                                                      os.path.join(gg.REF, 'pyslam', 'pipelines', name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        sys.modules['pyslam.pipelines.' + name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def surface(p):
    """The class surface a test compares: attribute names and the defaults that are plain values."""
    o = p.motion_options
    return dict(
        attributes=np.array(sorted(k for k in vars(p))),
        keyframe_trans_thresh=np.array(p.keyframe_trans_thresh), keyframe_rot_thresh=np.array(p.keyframe_rot_thresh),
        matcher_mode=np.array(p.matcher_mode), reprojection_stiffness=np.array(p.reprojection_stiffness),
        mode=np.array(p.mode), loss_name=np.array(type(p.loss).__name__),
        ransac=np.array([p.ransac.ransac_iters, p.ransac.ransac_thresh, p.ransac.num_min_set_pts], dtype=float),
        num_T_c_w=np.array(len(p.T_c_w)), num_keyframes=np.array(len(p.keyframes)),
        options=np.array([o.allow_nondecreasing_steps, o.max_nondecreasing_steps, o.min_cost_decrease, o.max_iters,
                          o.num_threads, o.linesearch_max_iters, o.min_update_norm, o.min_cost], dtype=float))


def main():
    install_stand_ins()
    mods = load_reference_pipeline()
    sparse, ransac = mods['sparse'], mods['ransac']
    ref_problem = gg.ref_problem

    histories, inliers = [], []
    orig_solve = ref_problem.Problem.solve

    def solve(self):
        out = orig_solve(self)
        histories.append(np.array(self._cost_history, dtype=float))
        return out
    ref_problem.Problem.solve = solve
    orig_ransac = ransac.FrameToFrameRANSAC.perform_ransac

    def perform_ransac(self):
        out = orig_ransac(self)
        inliers.append(np.array(out[3], dtype=np.int64))
        return out
    ransac.FrameToFrameRANSAC.perform_ransac = perform_ransac

    sc = scene()
    cu, cv, fu, fv, w, h = sc['cam']
    cam = gg.ref_sensors.RGBDCamera(cu, cv, fu, fv, w, h)
    first = gg.liegroups.SE3.from_matrix(sc['T_c_w'][0])
    p = sparse.SparseRGBDPipeline(cam, first)
    stereo_surface = surface(sparse.SparseStereoPipeline(gg.ref_sensors.StereoCamera(cu, cv, fu, fv, 0.12, w, h), first))
    defaults = surface(p)
    p.keyframe_trans_thresh, p.keyframe_rot_thresh = TRANS_THRESH, ROT_THRESH

    imgs = [sc['images'][f] for f in range(N_MAP)]        # one array object per frame: keyframes are found by identity
    frame_idx, mode, T_out, active, n_kf, printed = [], [], [], [], [], []
    match_flat, match_len, inl_flat, inl_len, hist_flat, hist_len, seeds = [], [], [], [], [], [], []

    def step(f, m):
        k = len(frame_idx)
        n_log, n_h, n_i = len(p.matcher.log), len(histories), len(inliers)
        np.random.seed(k)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            p.track(imgs[f], sc['depth'][f])
        sys.stdout.write(buf.getvalue())
        frame_idx.append(f); mode.append(m); seeds.append(k)
        T_out.append(p.T_c_w[-1].as_matrix() if p.T_c_w else np.full((4, 4), np.nan))
        active.append(p.active_keyframe_idx); n_kf.append(len(p.keyframes))
        printed.append(buf.getvalue())
        new = p.matcher.log[n_log:]
        assert len(new) == len(histories) - n_h == len(inliers) - n_i and len(new) in (0, 1)
        match_len.append(new[0].shape[0] if new else -1)
        inl_len.append(inliers[-1].shape[0] if new else -1)
        hist_len.append(histories[-1].shape[0] if new else -1)
        if new:
            match_flat.extend(new[0].ravel()); inl_flat.extend(inliers[-1]); hist_flat.extend(histories[-1])

    for f in range(N_MAP):
        step(f, 'map')
    kf_frames = [next(f for f in range(N_MAP) if kf.image is imgs[f]) for kf in p.keyframes]
    p.set_mode('track')
    for f in TRACK_FRAMES:
        step(f, 'track')
    assert len(kf_frames) >= 3, kf_frames

    out = dict(height=np.array(H), width=np.array(W), n_frames=np.array(N_MAP), seed=np.array(SEED), cell=np.array(CELL),
               step=np.array(STEP), hole_fraction=np.array(HOLE_FRACTION), checksum=checksum(sc),
               cam=np.array(sc['cam'], dtype=float), T_true=sc['T_c_w'],
               trans_thresh=np.array(TRANS_THRESH), rot_thresh=np.array(ROT_THRESH),
               frame_idx=np.array(frame_idx), mode=np.array(mode), seeds=np.array(seeds), T_c_w=np.array(T_out),
               active_idx=np.array(active), num_keyframes=np.array(n_kf), keyframe_frames=np.array(kf_frames),
               printed=np.array(printed), match_flat=np.array(match_flat), match_len=np.array(match_len),
               inlier_flat=np.array(inl_flat, dtype=np.int64), inlier_len=np.array(inl_len),
               hist_flat=np.array(hist_flat), hist_len=np.array(hist_len),
               **{'default_' + k: v for k, v in defaults.items()},
               **{'stereo_default_' + k: v for k, v in stereo_surface.items()})
    path = os.path.join(REPO, 'tests', 'golden', 'sparse_vo.npz')
    np.savez_compressed(path, **out)
    print('sparse_vo: {} frames, keyframes at frames {}, matches per frame {}, {:.1f} KB'.format(
        len(frame_idx), kf_frames, match_len, os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
