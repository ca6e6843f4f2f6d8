#!/usr/bin/env python
"""ms per call of matching without a prior (Matcher.matchMapGlobal: k_feat_map_search_all + k_feat_map_resolve, DESIGN.md section 7
step 9) at (map points N, frame features F) = (1 000, 1 000), (20 000, 4 096) and (262 144, 4 096), against the only way the library
had before to compare a point with every feature: matchMap(identity, cam, 1 << 30) on the same map, its points placed so that every
one projects inside the image (k_feat_map_search, one wave per point over the whole list).  That call is the baseline, not the
code under test.  The frame is a 400 x 400 noise image (nms_n = 1, response_threshold = 0, max_features = F), the map descriptors
are the frame's own with +-12 grey levels of noise per byte, cycled up to N, so a share of the points passes the ratio test;
match_cost_max = 4 000.  A call is timed on the host clock from its start to its return -- it ends with the stream synchronised
and the results on the host -- features held, median of --repeat calls after two warm-up calls.

Then one relocalisation of frame 5 of the 240 x 320 scene of the tests against frame 0's features at their true depth, stage by
stage (global match with and without the frame's feature pass, first P3P, guided match, second P3P) and as one relocalise_frame.
Prints one JSON object per line; --out also writes them to a file.

    python tools/reloc_bench.py [--repeat 9] [--out profiles/reloc_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

SHAPES = ((1000, 1000), (20000, 4096), (262144, 4096))
GLOBAL_CALLS = dict(memsets=1, kernel_launches=2, copies=1, synchronisations=1)


def ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def median_ms(fn, repeat):
    for _ in range(2):
        fn()
    return float(np.median([ms(fn)[0] for _ in range(repeat)]))


def run(N, F, repeat, image):
    from pyslam_amd.pipelines.matcher import Matcher, Matcher_parameters
    h, w = image.shape
    cam = (w / 2., h / 2., 300., 300.)
    m = Matcher(Matcher_parameters(nms_n=1, response_threshold=0, max_features=F, match_cost_max=4000))
    m.pushBack(image)
    m.setMap(np.zeros((1, 3)) + [0., 0., 1.], np.zeros((1, 32), dtype=np.uint8))
    m.matchMapGlobal()                                         # the frame's feature pass
    uv, _, desc = m.features(2)
    assert uv.shape[0] == F, (uv.shape[0], F)
    rng = np.random.default_rng(N)
    pick = np.arange(N) % F
    d = np.clip(desc[pick].astype(np.int64) + rng.integers(-12, 13, size=(N, 32)), 0, 255).astype(np.uint8)
    # every point projects inside the image under the identity: on its feature's pixel, at depth 1
    pts = np.stack([(uv[pick, 0] - cam[0]) / cam[2], (uv[pick, 1] - cam[1]) / cam[3], np.ones(N)], axis=1)
    m.setMap(pts, d)
    out = dict(kind='match_map_global', map_points=N, features=F, height=h, width=w, repeat=repeat, calls=GLOBAL_CALLS)
    for name, ratio in (('', (4, 5)), ('_ratio_1_1', (1, 1))):
        out['global{}_ms'.format(name)] = median_ms(lambda: m.matchMapGlobal(ratio), repeat)
        status = m.matchMapGlobal(ratio)[1]
        out['global{}_status_counts'.format(name)] = np.bincount(status, minlength=5).tolist()
    T = np.identity(4)
    out['baseline_ms'] = median_ms(lambda: m.matchMap(T, cam, 1 << 30), repeat)
    status = m.matchMap(T, cam, 1 << 30)[1]
    out['baseline_status_counts'] = np.bincount(status, minlength=4).tolist()
    assert status.min() != 1 and not (status == 1).any()
    out['baseline_over_global'] = out['baseline_ms'] / out['global_ms']
    out['device_bytes'] = int(m.device_bytes)
    m.close()
    return out


def relocalisation(f=5):
    from pyslam_amd import synthetic
    from pyslam_amd.liegroups import SO3
    from pyslam_amd.pipelines.matcher import Matcher
    from pyslam_amd.pipelines.mono import relocalise_frame
    from pyslam_amd.pipelines.pnp import register_frame
    from pyslam_amd.sensors import MonoCamera
    seq = synthetic.mono_sequence(240, 320, 10, seed=0, step=(0.08, -0.01, 0.02, 0.004, -0.012, 0.003), edge=0.35)
    cu, cv, fu, fv, w, h = seq['cam']
    cam = MonoCamera(cu, cv, fu, fv, w, h)
    m = Matcher()
    m.pushBack(seq['images'][0]); m.pushBack(seq['images'][1]); m.matchFeatures(0)
    uv, _, desc = m.features(0)
    z = seq['depth'][0][uv[:, 1], uv[:, 0]]
    p = np.stack([(uv[:, 0] - cu) * z / fu, (uv[:, 1] - cv) * z / fv, z], axis=1)
    Ti = np.linalg.inv(seq['T_c_w'][0])
    pts = p @ Ti[:3, :3].T + Ti[:3, 3]
    m.setMap(pts, desc)
    relocalise_frame(cam, m, seq['images'][1], pts, desc, seed=1)            # warm-up: every kernel has run once
    r = dict(kind='relocalisation', height=240, width=320, frame=f, map_points=int(pts.shape[0]))
    img = seq['images'][f]
    r['upload_ms'], _ = ms(lambda: m.pushBack(img))
    r['global_first_ms'], _ = ms(m.matchMapGlobal)
    r['global_match_ms'], (feature, status, _, _, obs) = ms(m.matchMapGlobal)
    r['features_ms'] = r['global_first_ms'] - r['global_match_ms']
    ok = status == 0
    r['num_accepted'] = int(ok.sum())
    r['first_pnp_ms'], (T1, inl) = ms(lambda: register_frame(cam, pts[ok], obs[ok], seed=f))
    r['first_inliers'] = int(len(inl))
    r['guided_match_ms'], (feature, status, _, obs) = ms(lambda: m.matchMap(T1, cam, 12))
    ok = status == 0
    r['num_guided'] = int(ok.sum())
    r['second_pnp_ms'], (T2, inl) = ms(lambda: register_frame(cam, pts[ok], obs[ok], seed=f + 1))
    r['guided_inliers'] = int(len(inl))
    img2 = img.copy(); img2[0, 0] ^= 1                                       # a fresh frame of the matcher's: the bytes differ by one pixel
    r['relocalise_frame_ms'], (T_cw, keep, _) = ms(lambda: relocalise_frame(cam, m, img2, pts, desc, seed=f))
    Tm, Tt = T_cw.as_matrix(), seq['T_c_w'][f]
    r['err_t'] = float(np.linalg.norm(Tm[:3, 3] - Tt[:3, 3]))
    r['err_rot_deg'] = float(np.degrees(np.linalg.norm(SO3.from_matrix(Tm[:3, :3] @ Tt[:3, :3].T, normalize=True).log())))
    m.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=9)
    ap.add_argument('--out')
    a = ap.parse_args()
    if a.repeat < 7:
        ap.error('--repeat must be at least 7')
    image = np.random.default_rng(7).integers(0, 256, size=(400, 400)).astype(np.uint8)
    lines = []
    for N, F in SHAPES:
        lines.append(run(N, F, a.repeat, image))
        print(json.dumps(lines[-1]), flush=True)
    lines.append(relocalisation())
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            for l in lines:
                fh.write(json.dumps(l) + '\n')


if __name__ == '__main__':
    main()
