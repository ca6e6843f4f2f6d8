#!/usr/bin/env python
"""ms per tracked frame of the dense RGB-D VO pipeline at 640 x 480 with 4 pyramid levels, on a synthetic.rgbd_sequence,
for two routes:

  device     pyslam.pipelines.DenseRGBDPipeline: pyramids, keyframe tables and the coarse-to-fine solve on the device
             (one synchronisation per frame)
  reference  the reference's structure on the public API that existed before it: host imgproc pyramid and gradient,
             then a new PhotometricResidualSE3 and Problem per level and frame (pipelines/dense.py:157-194)

plus a per-stage split of the device route (frame upload + pyramid, keyframe tables, the solve of each level alone and
its iteration count).  Prints one JSON object per line; --out also writes them to a file.

    python tools/dense_vo_bench.py [--frames 8] [--ref-frames 3] [--out profiles/dense_vo_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402


def sync():
    import torch
    torch.cuda.synchronize()


def camera(seq, scale=0):
    from pyslam.sensors import RGBDCamera
    cu, cv, fu, fv, w, h = seq['cam']
    cam = RGBDCamera(cu, cv, fu, fv, w, h)
    cam.compute_pixel_grid()
    return cam


def device_route(seq, frames):
    from pyslam.pipelines import DenseRGBDPipeline
    from pyslam_amd.liegroups import SE3
    p = DenseRGBDPipeline(camera(seq), SE3.from_matrix(seq['T_c_w'][0]))
    ms, its = [], []
    p.track(seq['images'][0], seq['depth'][0])
    for f in range(1, frames):
        t0 = time.perf_counter()
        p.track(seq['images'][f], seq['depth'][f])
        ms.append((time.perf_counter() - t0) * 1e3)
        its.append(list(p.last_iterations))
    return p, ms, its


def stages(p, seq, reps):
    """Per-stage split on the pipeline's own tracker (slots 0 = keyframe, 1 = tracking frame)."""
    from pyslam_amd.device import DenseTracker
    h, w = seq['images'].shape[1:]
    t = DenseTracker(4, h, w, num_slots=2)
    levels, cams = list(p.pyrlevel_sequence), list(p.pyr_cameras)
    var_i, var_d = p.intensity_stiffness ** -2, p.depth_stiffness ** -2
    out = {'upload_pyramid_ms': [], 'keyframe_tables_ms': [], 'solve_level_ms': {l: [] for l in levels},
           'iterations': {l: None for l in levels}, 'pixels': {}}
    pose0 = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    for r in range(reps + 1):
        sync()
        t0 = time.perf_counter()
        t.upload(1, seq['images'][1])
        sync()
        t1 = time.perf_counter()
        t.upload(0, seq['images'][0], seq['depth'][0])
        t.make_tables(0, levels, cams, var_i, var_d, p.min_grad)
        sync()
        t2 = time.perf_counter()
        pose = pose0
        for l in levels:
            s0 = time.perf_counter()
            pose, it, _ = t.track(0, 1, [l], [l > 2], p.motion_options, p.loss, pose)
            if r:
                out['solve_level_ms'][l].append((time.perf_counter() - s0) * 1e3)
            out['iterations'][l] = it[0]
        if r:                       # (r = 0 warms every shape)
            out['upload_pyramid_ms'].append((t1 - t0) * 1e3)
            out['keyframe_tables_ms'].append((t2 - t1) * 1e3)
    for l in levels:
        out['pixels'][l] = t.num_pixels(0, l)
    t.close()
    med = {'upload_pyramid_ms': float(np.median(out['upload_pyramid_ms'])),
           'keyframe_tables_ms': float(np.median(out['keyframe_tables_ms'])),
           'solve_level_ms': {str(l): float(np.median(v)) for l, v in out['solve_level_ms'].items()},
           'iterations': {str(l): v for l, v in out['iterations'].items()},
           'table_pixels': {str(l): v for l, v in out['pixels'].items()}}
    return med


def reference_route(seq, frames, p):
    """Host pyramids / gradients (imgproc), a new PhotometricResidualSE3 + Problem per level and frame."""
    from pyslam_amd.pipelines import imgproc
    from pyslam_amd.liegroups import SE3
    from pyslam_amd.problem import Problem
    from pyslam_amd.residuals import PhotometricResidualSE3

    def pyramid(img):
        raw = [img]
        for _ in range(1, 4):
            raw.append(imgproc.pyr_down(raw[-1]))
        return [r.astype(float) / 255. for r in raw]

    ref_im = pyramid(seq['images'][0])
    jac = [np.array([0.5 * imgproc.sobel(im, 1, 0), 0.5 * imgproc.sobel(im, 0, 1)]) for im in ref_im]
    depth = [seq['depth'][0]]
    for _ in range(1, 4):
        depth.append(depth[-1][0::2, 0::2])
    ms, its = [], []
    for f in range(1, frames):
        t0 = time.perf_counter()
        trk = pyramid(seq['images'][f])
        guess = SE3.identity()
        params = {'R_1_0': guess.rot, 't_1_0_1': guess.trans}
        it = []
        for lvl, cam in zip(p.pyrlevel_sequence, p.pyr_cameras):
            res = PhotometricResidualSE3(cam, ref_im[lvl], depth[lvl], trk[lvl], jac[lvl], p.intensity_stiffness,
                                         p.depth_stiffness, p.min_grad)
            prob = Problem(p.motion_options)
            prob.add_residual_block(res, ['R_1_0', 't_1_0_1'], loss=p.loss)
            prob.initialize_params(params)
            if lvl > 2:
                prob.set_parameters_constant('t_1_0_1')
            params = prob.solve()
            it.append(len(prob._cost_history) - 1)
        ms.append((time.perf_counter() - t0) * 1e3)
        its.append(it)
    return ms, its


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--ref-frames', type=int, default=3, help='frames of the reference-structured route (0: skip it)')
    ap.add_argument('--stage-reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pyslam_amd import synthetic
    seq = synthetic.rgbd_sequence(480, 640, max(a.frames, a.ref_frames + 1), seed=1, hole_fraction=0.005)
    lines = []
    p, ms, its = device_route(seq, a.frames)
    lines.append({'route': 'device', 'h': 480, 'w': 640, 'levels': 4, 'frames_timed': len(ms), 'ms_per_frame': ms,
                  'median_ms_per_frame': float(np.median(ms)), 'iterations_per_level': its})
    lines.append(dict({'route': 'device_stages'}, **stages(p, seq, a.stage_reps)))
    if a.ref_frames:
        rms, rits = reference_route(seq, a.ref_frames + 1, p)
        lines.append({'route': 'reference_structured', 'frames_timed': len(rms), 'ms_per_frame': rms,
                      'median_ms_per_frame': float(np.median(rms)), 'iterations_per_level': rits,
                      'speedup_of_device': float(np.median(rms) / np.median(ms))})
    text = '\n'.join(json.dumps(l) for l in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
