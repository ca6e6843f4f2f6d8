#!/usr/bin/env python
"""ms per tracked frame of monocular tracking against a map (pipelines/mono.py: track_frame) on synthetic.mono_sequence at
640 x 480 and 1 242 x 375: the map is frame 0's features at their true depth, every further frame is tracked with the previous
frame's pose as prior, split into

  upload       Matcher.pushBack of the new frame
  match_first  matchMap with the new frame's feature pass
  match_map    matchMap again on the same frame (features held): projection, search, claim, sub-pixel, read-back
  features     match_first - match_map
  pnp          register_frame on the matched pairs (P3P RANSAC, 400 samples)
  pnp_draw     of that, drawing the 400 minimal sets on the host (np.random.choice without replacement permutes all N indices
               for every sample)
  track        the whole track_frame of the frame, timed on its own
  flow_match   matchFeatures(0) between frame 0 and the same frame with the features of both held: the flow match that
               matching by projection stands beside

(median over the frames after a warm-up frame).  matchMap is, by construction (csrc/ps_abi_feat.h: ps_feat_match_map), one
memset, two kernel launches, one copy (the count and the four result arrays in one block) and one synchronisation; reading the
results is host memory only.  Then a self-initialised run of SparseMonoPipeline on the 240 x 320 scene of the tests with local_ba on
and off: keyframes, landmarks and the end pose against the truth, both trajectories scaled to a unit translation at the frame
that initialised -- a figure, not a gate (the accuracy of a self-initialised map is limited by the
two-view translation).  Prints one JSON object per line; --out also writes them to a file.

    python tools/mono_track_bench.py [--frames 6] [--out profiles/mono_track_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

STEP = (0.004, -0.002, 0.008, 0.0024, 0.003, -0.0012)
MATCH_MAP_CALLS = dict(memsets=1, kernel_launches=2, copies=1, synchronisations=1, read_back_copies=0, read_back_synchronisations=0)


def ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def rot_deg(Ra, Rb):
    from pyslam_amd.liegroups import SO3
    return float(np.degrees(np.linalg.norm(SO3.from_matrix(Ra @ Rb.T, normalize=True).log())))


def run(h, w, frames, radius):
    from pyslam_amd import synthetic
    from pyslam_amd.pipelines.matcher import Matcher
    from pyslam_amd.pipelines.mono import track_frame
    from pyslam_amd.pipelines.pnp import PnPRANSAC, register_frame
    from pyslam_amd.sensors import MonoCamera
    seq = synthetic.mono_sequence(h, w, frames + 1, seed=1, cell=0.12, step=STEP)
    cu, cv, fu, fv = seq['cam'][:4]
    cam = MonoCamera(cu, cv, fu, fv, w, h)
    m = Matcher()
    m.pushBack(seq['images'][0]); m.pushBack(seq['images'][1]); m.matchFeatures(0)
    uv, _, desc = m.features(0)
    z = seq['depth'][0][uv[:, 1], uv[:, 0]]
    p = np.stack([(uv[:, 0] - cu) * z / fu, (uv[:, 1] - cv) * z / fv, z], axis=1)
    Ti = np.linalg.inv(seq['T_c_w'][0])
    pts = p @ Ti[:3, :3].T + Ti[:3, 3]
    T = seq['T_c_w'][0]
    rows = []
    for f in range(1, frames + 1):
        r = {}
        r['track'], (T_cw, keep, _) = ms(lambda: track_frame(cam, m, seq['images'][f], pts, desc, T, radius=radius, seed=f))
        r['num_inliers'] = int(keep.size)
        Tt = seq['T_c_w'][f]
        Tm = T_cw.as_matrix()
        r['err_t'], r['err_rot_deg'] = float(np.linalg.norm(Tm[:3, 3] - Tt[:3, 3])), rot_deg(Tm[:3, :3], Tt[:3, :3])
        # the same frame again, stage by stage, as a fresh frame of the matcher's (the bytes differ by one pixel)
        img = seq['images'][f].copy(); img[0, 0] ^= 1
        r['upload'], _ = ms(lambda: m.pushBack(img))
        r['match_first'], _ = ms(lambda: m.matchMap(T, cam, radius))
        r['match_map'], (feature, status, _, obs) = ms(lambda: m.matchMap(T, cam, radius))
        r['features'] = r['match_first'] - r['match_map']
        ok = status == 0
        r['num_matched'] = int(ok.sum())
        r['pnp'], _ = ms(lambda: register_frame(cam, pts[ok], obs[ok], seed=f))
        rs = PnPRANSAC(cam)
        rs.set_obs(pts[ok], obs[ok])
        r['pnp_draw'], _ = ms(rs.draw_samples)
        m.pushBack(seq['images'][0]); m.pushBack(img); m.matchFeatures(0)
        r['flow_match'], _ = ms(lambda: m.matchFeatures(0))
        r['num_flow_matches'] = int(m.matches_array()[0].shape[0])
        rows.append(r)
        T = Tm
    warm = rows[1:] if len(rows) > 1 else rows
    out = dict(kind='track_frame', height=h, width=w, radius=radius, map_points=int(pts.shape[0]), frames_timed=len(warm),
               device_bytes=int(m.device_bytes), match_map_calls=MATCH_MAP_CALLS)
    for k in rows[0]:
        vals = [x[k] for x in warm]
        key = k if k.startswith('num_') or k.startswith('err_') else k + '_ms'
        out[key] = float(np.max(vals)) if k.startswith('err_') else float(np.median(vals))
    m.close()
    return out


def self_initialised(local_ba):
    from pyslam_amd import synthetic
    from pyslam_amd.pipelines.mono import SparseMonoPipeline
    from pyslam_amd.sensors import MonoCamera
    seq = synthetic.mono_sequence(240, 320, 10, seed=0, step=(0.08, -0.01, 0.02, 0.004, -0.012, 0.003), edge=0.35)
    cu, cv, fu, fv, w, h = seq['cam']
    p = SparseMonoPipeline(MonoCamera(cu, cv, fu, fv, w, h))
    p.local_ba = local_ba
    np.random.seed(8)
    t, _ = ms(lambda: [p.track(im) for im in seq['images']])
    p.matcher.close()
    init = next(f for f, T in enumerate(p.T_c_w) if f > 0 and T is not None)
    rel = [seq['T_c_w'][f] @ np.linalg.inv(seq['T_c_w'][0]) for f in range(len(p.T_c_w))]
    scale = np.linalg.norm(rel[init][:3, 3]) / np.linalg.norm(p.T_c_w[init].as_matrix()[:3, 3])
    end, truth = p.T_c_w[-1].as_matrix(), rel[-1]
    return dict(kind='self_initialised', local_ba=bool(local_ba), height=240, width=320, frames=len(p.T_c_w), init_frame=init,
                keyframes=len(p.keyframes), landmarks=p.landmark_counts, bundle_adjustments=[[float(a), float(b)] for a, b in p.ba_costs],
                end_err_rot_deg=rot_deg(end[:3, :3], truth[:3, :3]),
                end_err_t_relative=float(np.linalg.norm(scale * end[:3, 3] - truth[:3, 3]) / np.linalg.norm(truth[:3, 3])),
                total_ms=t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=6)
    ap.add_argument('--radius', type=int, default=12)
    ap.add_argument('--out')
    a = ap.parse_args()
    lines = []
    for h, w in ((480, 640), (375, 1242)):
        lines.append(run(h, w, a.frames, a.radius))
        print(json.dumps(lines[-1]), flush=True)
    for ba in (True, False):
        lines.append(self_initialised(ba))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as fh:
            for l in lines:
                fh.write(json.dumps(l) + '\n')


if __name__ == '__main__':
    main()
