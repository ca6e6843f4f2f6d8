"""Matching by projection and the monocular tracking chain on the host: featproc.match_map alone, the true-map chain of the
240 x 320 scene against the truth, the margins tests/test_gpu_mono_track.py relies on for the scenes it reuses
(tests/mono_scenes.py), and the class surface of pyslam_amd.pipelines.mono.  No GPU."""
import numpy as np
import pytest

import mono_scenes as ms
import pnp_scenes as sc
from pyslam_amd import synthetic
from pyslam_amd.pipelines import featproc as fp

CAM = (63.5, 47.5, 115.2, 115.2, 128, 96)          # of synthetic.mono_sequence(96, 128)


@pytest.fixture(scope='module')
def small():
    seq = ms.sequence(96, 128)
    assert tuple(seq['cam']) == CAM
    return seq, ms.frames(96, 128)[0]


def back_project(frame, cam, depth):
    u, v = frame.uv[:, 0].astype(float), frame.uv[:, 1].astype(float)
    return np.stack([(u - cam[0]) * depth / cam[2], (v - cam[1]) * depth / cam[3], np.broadcast_to(depth, u.shape)], axis=1)


# ---- featproc.match_map alone ----

@pytest.mark.parametrize('depth', [0.5, 3.0, 'varying'])
def test_a_frames_own_features_find_themselves(small, depth):
    seq, f0 = small
    z = np.linspace(0.7, 9.0, len(f0)) if depth == 'varying' else depth
    pts = back_project(f0, CAM, z)
    feature, status, cost, uv = fp.match_map(f0, pts, f0.desc, np.identity(4), CAM, 8)
    assert len(f0) > 100
    assert np.array_equal(feature, np.arange(len(f0))) and not status.any() and not cost.any()
    assert np.array_equal(uv, f0.uv.astype(float))             # cost 0: no sub-pixel offset


def test_a_point_listed_twice_loses_its_second_copy(small):
    seq, f0 = small
    pts = back_project(f0, CAM, 2.0)
    k = 17
    pts2, desc2 = np.concatenate([pts, pts[k:k + 1]]), np.concatenate([f0.desc, f0.desc[k:k + 1]])
    feature, status, cost, uv = fp.match_map(f0, pts2, desc2, np.identity(4), CAM, 8)
    assert status[k] == 0 and feature[k] == k
    assert status[-1] == 3 and feature[-1] == -1 and cost[-1] == 0 and np.array_equal(uv[-1], [-1., -1.])
    assert not status[:-1].any()


def test_status_1(small):
    seq, f0 = small
    w, h = CAM[4], CAM[5]

    def at(u, v, z=2.0):
        return [(u - CAM[0]) * z / CAM[2], (v - CAM[1]) * z / CAM[3], z]
    pts = np.array([at(20, 20, 0.0), at(20, 20, -1.0), [np.nan, 0., 2.], [0., 0., np.nan], [np.inf, 0., 2.],
                    at(-0.75, 20), at(w - 0.25, 20), at(20, -0.75), at(20, h - 0.25),               # centres at -1 and at w / h
                    at(-0.25, 20), at(w - 0.75, 20), at(20, -0.25), at(20, h - 0.75)])              # centres at 0 and at w - 1 / h - 1
    desc = np.zeros((len(pts), 32), dtype=np.uint8)
    feature, status, cost, uv = fp.match_map(f0, pts, desc, np.identity(4), CAM, 3, fp.Params(match_cost_max=0))
    assert status[:9].tolist() == [1] * 9 and status[9:].tolist() == [2] * 4
    assert (feature == -1).all() and (cost == -1).all() and (uv == -1.).all()


def test_radius_0_matches_only_a_feature_on_the_centre(small):
    seq, f0 = small
    pts = back_project(f0, CAM, 2.0)
    shifted = pts.copy()
    shifted[::2, 0] += 1.0 * 2.0 / CAM[2]                      # every other point one pixel to the right
    feature, status, cost, uv = fp.match_map(f0, shifted, f0.desc, np.identity(4), CAM, 0)
    on = np.arange(len(f0)) % 2 == 1
    occupied = {(int(u), int(v)) for u, v in f0.uv}
    off_hits = np.array([(int(u) + 1, int(v)) in occupied for u, v in f0.uv[~on]])
    assert not off_hits.any()                                  # non-maximum suppression: no feature beside a feature
    assert (status[on] == 0).all() and np.array_equal(feature[on], np.nonzero(on)[0])
    assert (status[~on] == 2).all() and (feature[~on] == -1).all()
    assert (fp.match_map(f0, shifted, f0.desc, np.identity(4), CAM, 1)[1] == 0).all()


def test_the_window_is_clipped_at_the_first_and_the_last_row(small):
    seq, f0 = small
    h, w = f0.du.shape
    top, bottom = f0.uv[0], f0.uv[-1]                          # raster order: the highest and the lowest feature
    r = max(int(top[1]), h - 1 - int(bottom[1]))
    z = 2.0
    pts = np.array([[(top[0] - CAM[0]) * z / CAM[2], (0 - CAM[1]) * z / CAM[3], z],
                    [(bottom[0] - CAM[0]) * z / CAM[2], (h - 1 - CAM[1]) * z / CAM[3], z]])
    desc = np.stack([f0.desc[0], f0.desc[-1]])
    feature, status, cost, uv = fp.match_map(f0, pts, desc, np.identity(4), CAM, r)
    assert status.tolist() == [0, 0] and feature.tolist() == [0, len(f0) - 1] and cost.tolist() == [0, 0]
    best, bcost, _ = ms.brute_force(f0, pts, desc, np.identity(4), CAM, r, 1200)
    assert best.tolist() == feature.tolist()
    # a window far larger than the image is the whole image
    big = fp.match_map(f0, pts, desc, np.identity(4), CAM, 10 ** 9)
    assert big[0].tolist() == [0, len(f0) - 1]
    with pytest.raises(ValueError):
        fp.match_map(f0, pts, desc, np.identity(4), CAM, -1)


# ---- the true-map chain ----

@pytest.mark.parametrize('radius', ms.CHAIN_RADII)
def test_true_map_chain_against_the_truth(radius):
    chain = ms.host_chain(radius)
    n = ms.true_map()[0].shape[0]
    assert n == 744 and len(chain) == 9
    share = [float((r['status'] == 0).mean()) for r in chain]
    e_t, e_rot = max(r['e_t'] for r in chain), max(r['e_rot_deg'] for r in chain)
    print('radius {}: status 0 in {:.1%} .. {:.1%} of {} points, inliers {} .. {}, worst pose error {:.4f} m / {:.3f} deg'.format(
        radius, min(share), max(share), n, min(r['res']['count'] for r in chain), max(r['res']['count'] for r in chain), e_t, e_rot))
    assert all(r['radius'] == radius for r in chain)
    assert min(share) >= ms.MIN_TRACKED
    assert e_t <= ms.TRUTH_BOUND[radius][0] and e_rot <= ms.TRUTH_BOUND[radius][1]


# ---- the margins the GPU tests rely on ----

def test_chain_margins():
    seq, fr = ms.sequence(), ms.frames()
    pts, desc = ms.true_map()
    for radius in ms.CHAIN_RADII:
        for r in ms.host_chain(radius):
            margin = ms.rounding_margin(pts, r['prior'], seq['cam'])
            cond = sc.conditions(r['res'])
            best, cost, tied = ms.brute_force(fr[r['frame']], pts, desc, r['prior'], seq['cam'], radius, 1200)
            print('radius {} frame {}: rounding margin {:.2e} px, squared errors near the threshold {} + {}, P3P branch margin {:.2e}, '
                  'points with a tie at the minimum {}'.format(radius, r['frame'], margin, cond['near'], cond['near_final'], cond['branch'], tied))
            assert margin >= ms.ROUND_MARGIN
            assert cond['near'] == 0 and cond['near_final'] == 0
            # ties: the lower feature index decides, in brute_force as in match_map -- before features are shared out
            feature, status = r['match'][0], r['match'][1]
            assert np.array_equal(best[status == 0], feature[status == 0])
            assert (best[status == 2] == -1).all() and (best[status == 1] == -1).all() and (best[status == 3] >= 0).all()


@pytest.mark.parametrize('shape', ms.SMALL_SHAPES)
def test_small_scene_margins(shape):
    seq, fr = ms.sequence(*shape), ms.frames(*shape)
    pts, desc = ms.true_map(*shape)
    for f in ms.SMALL_FRAMES:
        margin = ms.rounding_margin(pts, seq['T_c_w'][f], seq['cam'])
        assert margin >= ms.ROUND_MARGIN, (shape, f, margin)
        for radius in ms.SMALL_RADII:
            best, cost, tied = ms.brute_force(fr[f], pts, desc, seq['T_c_w'][f], seq['cam'], radius, 1200)
            feature, status, c, uv = fp.match_map(fr[f], pts, desc, seq['T_c_w'][f], seq['cam'], radius)
            print(shape, 'frame', f, 'radius', radius, 'margin {:.2e}'.format(margin), 'status counts', np.bincount(status, minlength=4).tolist(),
                  'ties', tied)
            assert np.array_equal(best[status == 0], feature[status == 0]) and np.array_equal(cost[status == 0], c[status == 0])
            assert np.array_equal(cost[status == 3], c[status == 3])
            assert (best[(status == 1) | (status == 2)] == -1).all()
            # every feature has one landmark
            won = feature[status == 0]
            assert np.unique(won).size == won.size


def test_widened_case_and_pipeline_margins():
    seq = ms.sequence()
    pts, _ = ms.true_map()
    T_prior, ref = ms.widened_case()
    cond = sc.conditions(ref['res'])
    margin = ms.rounding_margin(pts, T_prior, seq['cam'])
    print('widened case: radius used {}, {} matched, {} inliers, rounding margin {:.2e}, near the threshold {} + {}'.format(
        ref['radius'], ref['matched'].size, ref['keep'].size, margin, cond['near'], cond['near_final']))
    assert ref['radius'] == 6 and ref['keep'].size >= 500
    assert margin >= ms.ROUND_MARGIN and cond['near'] == 0 and cond['near_final'] == 0
    run = ms.host_pipeline_big()
    print('host pipeline: initialised on frame {}, keyframes {}, landmarks {}'.format(run['init_frame'], run['keyframes'], run['counts']))
    assert run['init_frame'] is not None and len(run['keyframes']) >= 3
    for c in run['checks']:
        print(c)
        assert c['near'] == 0 and c.get('margin', 1.) >= ms.ROUND_MARGIN


# ---- the class surface ----

def test_pipeline_attributes_and_defaults():
    from pyslam_amd.liegroups import SE3
    from pyslam_amd.losses import L2Loss
    from pyslam_amd.pipelines.matcher import Matcher, Matcher_parameters
    from pyslam_amd.pipelines.mono import SparseMonoPipeline
    from pyslam_amd.problem import Options
    p = SparseMonoPipeline(ms.camera(CAM))
    assert p.keyframes == [] and p.T_c_w == [] and p.mode == 'map'
    assert isinstance(p.matcher, Matcher) and isinstance(p.matcher_params, Matcher_parameters) and p.matcher.params is p.matcher_params
    assert isinstance(p.loss, L2Loss) and isinstance(p.ba_options, Options)
    assert np.array_equal(p.first_pose.as_matrix(), SE3.identity().as_matrix())
    assert (p.init_baseline, p.search_radius, p.local_window, p.local_ba, p.keyframe_rot_thresh) == (1.0, 12, 5, True, 0.3)
    assert p.init_min_parallax_deg == 1.0 and p.keyframe_parallax_thresh == 0.05
    assert p.ransac.min_inliers == 12 and p.init_ransac.min_inliers == 16
    p.set_mode('track')
    assert p.mode == 'track'


def test_the_shim_and_the_exports():
    import pyslam.pipelines
    import pyslam.pipelines.mono as shim
    import pyslam_amd.pipelines
    from pyslam_amd.pipelines import mono
    assert shim.SparseMonoPipeline is mono.SparseMonoPipeline and shim.track_frame is mono.track_frame
    assert pyslam.pipelines.SparseMonoPipeline is mono.SparseMonoPipeline and pyslam.pipelines.track_frame is mono.track_frame
    assert pyslam_amd.pipelines.SparseMonoPipeline is mono.SparseMonoPipeline


def test_track_frame_refuses_an_empty_map():
    from pyslam_amd.pipelines.mono import track_frame
    with pytest.raises(ValueError, match='the map is empty'):
        track_frame(ms.camera(CAM), None, np.zeros((96, 128), dtype=np.uint8), np.zeros((0, 3)), np.zeros((0, 32), dtype=np.uint8),
                    np.identity(4))


def test_mono_sequence_is_the_left_camera_of_stereo_sequence():
    a = synthetic.mono_sequence(40, 56, 2, seed=3, cell=0.3)
    b = synthetic.stereo_sequence(40, 56, 2, seed=3, cell=0.3)
    assert np.array_equal(a['images'], b['left']) and np.array_equal(a['depth'], b['depth']) and np.array_equal(a['T_c_w'], b['T_c_w'])
    assert a['cam'] == b['cam'][:4] + (56, 40)


def test_the_header_and_the_signature_table_hold_the_map_calls():
    import os
    import re
    from pyslam_amd import _native as nat
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, '..', 'include', 'pyslam_hip.h')).read()
    for name, nargs in (('ps_feat_set_map', 4), ('ps_feat_match_map', 6), ('ps_feat_read_map_matches', 6)):
        decl = re.search(r'int {}\(([^)]*)\);'.format(name), header)
        assert decl and len(decl.group(1).split(',')) == nargs == len(nat.SIGNATURES[name][1]), name
