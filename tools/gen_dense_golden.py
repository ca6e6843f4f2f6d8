#!/usr/bin/env python
"""Generate tests/golden/dense_rgbd.npz by running the VERBATIM reference dense RGB-D pipeline.

TEST INFRASTRUCTURE -- authoring machine only, like oracle/gen_golden.py, whose path set-up, numba stand-in and
repaired image lookup (reference_bilinear_body) it imports.  Run from the repository root:

    python tools/gen_dense_golden.py

The reference's pipelines/dense.py and keyframes.py are loaded by path (their package __init__ imports every pipeline,
sparse.py -> viso2, which is not installed), with ``cv2`` pointed at pyslam_amd/pipelines/imgproc.py (pyrDown, Sobel:
the two OpenCV calls the RGB-D pipeline makes; the StereoBM matcher its depth pyramid creates and never uses is a
placeholder).  The pipeline runs over synthetic.rgbd_sequence in 'map' mode with
lowered keyframe thresholds (so keyframes are dropped), then re-localises a few frames in 'track' mode.  Recorded:
the inputs, the pipeline's defaults and pyramid cameras, every T_c_w, the keyframe frame indices, the active keyframe
index after each frame, each level's Problem._cost_history (captured by wrapping the reference's Problem.solve) and
the printed lines.  The GPU tests read only the .npz.
"""
import contextlib
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
from pyslam_amd.pipelines import imgproc  # noqa: E402

H, W, N_MAP, SEED = 96, 128, 8, 3
TRACK_FRAMES = [1, 2, 3, 4, 5]
TRANS_THRESH, ROT_THRESH = 0.1, 0.03


def install_cv2():
    cv2 = types.ModuleType('cv2')
    cv2.pyrDown = lambda img: imgproc.pyr_down(img)

    def Sobel(img, ddepth, dx, dy):
        assert ddepth == -1
        return imgproc.sobel(img, dx, dy)
    cv2.Sobel = Sobel
    # DenseRGBDKeyframe.compute_depth_pyramid creates a StereoBM matcher and never uses it (keyframes.py): a placeholder
    cv2.StereoBM_create = lambda *args, **kwargs: object()
    sys.modules['cv2'] = cv2


def load_reference_pipeline():
    import pyslam                                              # the reference package (gg put it first on the path)
    assert pyslam.__file__.startswith(gg.REF), pyslam.__file__
    pkg = types.ModuleType('pyslam.pipelines')                # without the package __init__ (it imports sparse -> viso2)
    pkg.__path__ = [os.path.join(gg.REF, 'pyslam', 'pipelines')]
    sys.modules['pyslam.pipelines'] = pkg
    mods = {}
    for name in ('keyframes', 'dense'):
        spec = importlib.util.spec_from_file_location('pyslam.pipelines.' + name,
                                                      os.path.join(gg.REF, 'pyslam', 'pipelines', name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        sys.modules['pyslam.pipelines.' + name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods['dense']


def main():
    install_cv2()
    # the residual class the pipeline imports (pyslam.residuals loads its modules under their bare names)
    ref_photo = sys.modules[gg.ref_residuals.PhotometricResidualSE3.__module__]
    ref_photo.bilinear_interpolate = gg.reference_bilinear_body()
    dense = load_reference_pipeline()
    ref_problem = gg.ref_problem

    histories = []
    orig_solve = ref_problem.Problem.solve

    def solve(self):
        out = orig_solve(self)
        histories.append(np.array(self._cost_history, dtype=float))
        return out
    ref_problem.Problem.solve = solve

    seq = synthetic.rgbd_sequence(H, W, N_MAP, seed=SEED)
    cu, cv, fu, fv, w, h = seq['cam']
    cam = gg.ref_sensors.RGBDCamera(cu, cv, fu, fv, w, h)
    cam.compute_pixel_grid()
    first = gg.liegroups.SE3.from_matrix(seq['T_c_w'][0])
    p = dense.DenseRGBDPipeline(cam, first)

    o = p.motion_options
    defaults = dict(
        pyrlevels=np.array(p.pyrlevels), pyrlevel_sequence=np.array(p.pyrlevel_sequence),
        keyframe_trans_thresh=np.array(p.keyframe_trans_thresh), keyframe_rot_thresh=np.array(p.keyframe_rot_thresh),
        intensity_stiffness=np.array(p.intensity_stiffness), depth_stiffness=np.array(p.depth_stiffness),
        min_grad=np.array(p.min_grad), depth_map_type=np.array(p.depth_map_type), mode=np.array(p.mode),
        use_motion_model_guess=np.array(p.use_motion_model_guess), loss_k=np.array(p.loss.k),
        loss_name=np.array(type(p.loss).__name__),
        pyr_cameras=np.array([[c.cu, c.cv, c.fu, c.fv, c.w, c.h] for c in p.pyr_cameras]),
        options=np.array([o.allow_nondecreasing_steps, o.max_nondecreasing_steps, o.min_cost_decrease, o.max_iters,
                          o.num_threads, o.linesearch_max_iters, o.min_update_norm, o.min_cost], dtype=float))
    p.keyframe_trans_thresh, p.keyframe_rot_thresh = TRANS_THRESH, ROT_THRESH

    imgs = [seq['images'][f] for f in range(N_MAP)]       # one array object per frame: keyframes are found by identity
    frame_idx, mode, T_out, active, n_kf, printed, iters, hist_flat, hist_len = [], [], [], [], [], [], [], [], []

    def step(f, m):
        start = len(histories)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            p.track(imgs[f], seq['depth'][f])
        sys.stdout.write(buf.getvalue())
        frame_idx.append(f); mode.append(m)
        T_out.append(p.T_c_w[-1].as_matrix() if p.T_c_w else np.full((4, 4), np.nan))
        active.append(p.active_keyframe_idx); n_kf.append(len(p.keyframes))
        printed.append(buf.getvalue())
        new = histories[start:]
        assert len(new) in (0, len(p.pyrlevel_sequence)), len(new)
        iters.append([len(x) - 1 for x in new] if new else [-1] * len(p.pyrlevel_sequence))
        for x in new:
            hist_flat.extend(x); hist_len.append(len(x))

    for f in range(N_MAP):
        step(f, 'map')
    kf_frames = []
    for kf in p.keyframes:
        kf_frames.append(next(f for f in range(N_MAP) if kf.data[0] is imgs[f]))
    p.set_mode('track')
    for f in TRACK_FRAMES:
        step(f, 'track')
    assert len(kf_frames) >= 3, kf_frames

    out = dict(images=seq['images'], depth=seq['depth'], cam=np.array(seq['cam'], dtype=float), T_true=seq['T_c_w'],
               seed=np.array(SEED), trans_thresh=np.array(TRANS_THRESH), rot_thresh=np.array(ROT_THRESH),
               frame_idx=np.array(frame_idx), mode=np.array(mode), T_c_w=np.array(T_out), active_idx=np.array(active),
               num_keyframes=np.array(n_kf), keyframe_frames=np.array(kf_frames), printed=np.array(printed),
               iterations=np.array(iters), hist_flat=np.array(hist_flat), hist_len=np.array(hist_len),
               **{'default_' + k: v for k, v in defaults.items()})
    path = os.path.join(REPO, 'tests', 'golden', 'dense_rgbd.npz')
    np.savez_compressed(path, **out)
    print('dense_rgbd: {} tracked frames, keyframes at frames {}, {:.1f} KB'.format(
        len(frame_idx), kf_frames, os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
