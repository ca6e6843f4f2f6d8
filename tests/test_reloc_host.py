"""Matching without a prior and relocalisation on the host: featproc.match_map_global against an independent dense brute force, the
rules of step 9 one by one, the conditions tests/test_gpu_reloc.py relies on for the scenes it reuses (tests/reloc_scenes.py), the
truth bounds of the relocalisation, and the surface that needs no device.  No GPU."""
import os
import re

import numpy as np
import pytest

import mono_scenes as ms
import reloc_scenes as rs
from pyslam_amd.pipelines import featproc as fp

CASES = [(shape, f) for shape in ms.SMALL_SHAPES for f in ms.SMALL_FRAMES] + [((None, None), f) for f in rs.RELOC_FRAMES]


def check_against_dense(frame, desc, ratio, params=None):
    """match_map_global against reloc_scenes.dense_global; -> (result, number of points with a tie at the minimum)."""
    p = params or fp.Params()
    feature, status, cost, second, uv = fp.match_map_global(frame, desc, ratio, p)
    best, c1, c2, st, tied = rs.dense_global(frame, desc, ratio, p.match_cost_max)
    assert all(a.dtype == np.int32 for a in (feature, status, cost, second)) and uv.dtype == np.float64
    assert np.array_equal(cost, c1) and np.array_equal(second, c2)
    assert not (status == 1).any()
    # before the features are shared out: 0 and 3 are the dense 0, the rest is equal
    assert np.array_equal(np.where(status == 3, 0, status), st)
    assert np.array_equal(feature[status == 0], best[status == 0]) and (feature[status != 0] == -1).all()
    # one landmark per feature: the lowest (cost, point) of the points whose best feature it is
    for k in np.unique(best[st == 0]):
        owners = np.nonzero((st == 0) & (best == k))[0]
        winner = owners[np.lexsort((owners, c1[owners]))[0]]
        assert status[winner] == 0 and (status[owners[owners != winner]] == 3).all()
    assert (uv[status != 0] == -1.).all() and (uv[status == 0] >= 0.).all()
    return (feature, status, cost, second, uv), tied


@pytest.mark.parametrize('shape,f', CASES)
def test_match_map_global_equals_the_dense_brute_force(shape, f):
    fr = ms.frames(*shape)[f]
    _, desc = ms.true_map(*shape)
    for ratio in rs.RATIOS:
        out, tied = check_against_dense(fr, desc, ratio)
        print(shape, 'frame', f, 'ratio', ratio, 'N', desc.shape[0], 'F', len(fr), 'status counts',
              np.bincount(out[1], minlength=5).tolist(), 'points with a tie at the minimum', tied)
    assert (fp.match_map_global(fr, desc, (4, 5))[1] == 0).sum() >= 50


def test_a_minimum_reached_by_two_features_occurs_in_the_compared_cases():
    tied = {}
    for shape, f in CASES:
        tied[(shape, f)] = rs.dense_global(ms.frames(*shape)[f], ms.true_map(*shape)[1], (4, 5))[4]
    print(tied)
    assert tied[((101, 139), 1)] >= 1 and all(tied[((None, None), f)] >= 1 for f in rs.RELOC_FRAMES)


def test_the_tie_rule_and_the_strict_ratio():
    fr = ms.frames(96, 128)[1]
    k = 23
    # one feature of the frame twice in the list: the minimum 0 is reached twice, the lower index is the best, and it is ambiguous
    twin = fp.Frame(fr.du, fr.dv, np.concatenate([fr.uv, fr.uv[k:k + 1]]), np.concatenate([fr.R, fr.R[k:k + 1]]),
                    np.concatenate([fr.desc, fr.desc[k:k + 1]]))
    for ratio in rs.RATIOS:
        feature, status, cost, second, uv = fp.match_map_global(twin, fr.desc[k:k + 1], ratio)
        assert (feature[0], status[0], cost[0], second[0]) == (-1, 4, 0, 0)
    best = rs.dense_global(twin, fr.desc[k:k + 1], (1, 1))[0]
    assert best[0] == k
    # a descriptor one grey level from feature k: c1 = 1, unambiguous at (1, 1) unless another feature is as close
    d = fr.desc[k:k + 1].copy()
    d[0, 0] ^= 1
    feature, status, cost, second, uv = fp.match_map_global(fr, d, (1, 1))
    assert (feature[0], status[0], cost[0]) == (k, 0, 1) and second[0] > 1


def test_ratio_1_1_accepts_every_strict_minimum():
    fr = ms.frames(101, 139)[1]                                # one of its points has its minimum at two features
    _, desc = ms.true_map(101, 139)
    feature, status, cost, second, uv = fp.match_map_global(fr, desc, (1, 1))
    ok = cost >= 0
    assert np.array_equal(status[ok] == 4, cost[ok] == second[ok]) and (status == 4).any()
    looser = fp.match_map_global(fr, desc, (4, 5))[1]
    assert ((looser == 4) | (status != 4)).all() and (looser == 4).sum() > (status == 4).sum()


def test_an_exact_tie_of_the_products_is_ambiguous():
    fr = ms.frames(96, 128)[1]
    _, desc = ms.true_map(96, 128)
    i, tie, looser = rs.exact_tie_point(fr, desc)
    a = fp.match_map_global(fr, desc, tie)
    b = fp.match_map_global(fr, desc, looser)
    print('point', i, 'c1', a[2][i], 'c2', a[3][i], 'tie ratio', tie, '-> status', a[1][i], '; ratio', looser, '-> status', b[1][i])
    assert tie[1] * a[2][i] == tie[0] * a[3][i] and a[1][i] == 4 and a[0][i] == -1
    assert b[1][i] in (0, 3)


def test_a_frame_without_features_and_a_frame_with_one():
    _, desc = ms.true_map(96, 128)
    flat = fp.features(np.full((96, 128), 117, dtype=np.uint8))
    feature, status, cost, second, uv = fp.match_map_global(flat, desc)
    assert len(flat) == 0 and (status == 2).all() and (feature == -1).all() and (cost == -1).all() and (second == -1).all() and (uv == -1.).all()
    p = fp.Params(max_features=1, **rs.NOISE_KW)
    fa, fb = rs.noise_features(False, 1)
    assert len(fb) == 1
    wide = fp.Params(max_features=4096, **rs.NOISE_KW)
    all_a = rs.noise_features(False)[0]
    out, _ = check_against_dense(fb, all_a.desc, (4, 5), p)
    feature, status, cost, second, uv = out
    assert (second == -1).all() and set(np.unique(status)) <= {0, 2, 3} and (status == 0).sum() == 1     # accepted; one keeps the feature
    assert (cost[status != 2] >= 0).all() and wide.max_features == 4096
    empty = fp.match_map_global(fb, np.zeros((0, 32), dtype=np.uint8))
    assert all(a.shape[0] == 0 for a in empty) and empty[4].shape == (0, 2)


@pytest.mark.parametrize('ratio', [(0, 5), (6, 5), (4, 32769), (-1, -1)])
def test_a_bad_ratio_is_refused(ratio):
    with pytest.raises(ValueError, match='ratio'):
        fp.match_map_global(ms.frames(96, 128)[1], ms.true_map(96, 128)[1], ratio)


# ---- the conditions the GPU tests rely on ----

def test_noise_cases():
    tile = rs.kernel_tile()
    fa, fb = rs.noise_features(True)
    print('tile', tile, 'big noise features', len(fa), len(fb))
    assert len(fb) > 2 * tile and len(fb) % tile != 0 and len(fb) <= 4096
    p = fp.Params(**rs.NOISE_KW)
    out, tied = check_against_dense(fb, fa.desc, (4, 5), p)
    print('big noise: status counts', np.bincount(out[1], minlength=5).tolist(), 'ties', tied)
    assert (out[1] == 0).sum() > 100 and (out[1] == 4).sum() > 0
    # the best feature of some point lies in every quarter of the first two tiles and in the last, partial tile
    part = np.unique(out[0][out[1] == 0] // (tile // 4))
    assert set(range(8)) <= set(part.tolist()) and (out[0] >= 2 * tile).any()
    for mf in rs.NOISE_MAX_FEATURES:
        fa, fb = rs.noise_features(False, mf)
        assert len(fa) == mf and len(fb) == mf
        check_against_dense(fb, fa.desc, (4, 5), fp.Params(max_features=mf, **rs.NOISE_KW))


def test_a_frames_own_descriptors_find_themselves_unless_two_are_equal():
    fr = ms.frames(96, 128)[1]
    out, tied = check_against_dense(fr, fr.desc, (4, 5))
    feature, status, cost, second, uv = out
    assert (cost == 0).all()
    own = second > 0
    print('own descriptors:', int(own.sum()), 'of', len(fr), 'are unique in the frame')
    assert own.sum() > 50 and np.array_equal(feature[own], np.nonzero(own)[0]) and (status[own] == 0).all() and (status[~own] == 4).all()
    assert np.array_equal(uv[own], fr.uv[own].astype(float))


@pytest.mark.parametrize('f', rs.RELOC_FRAMES)
def test_relocalisation_against_the_truth_and_its_margins(f):
    seq = ms.sequence()
    pts, _ = ms.true_map()
    r = rs.reloc_case(f)
    c = rs.reloc_checks(r, pts, seq['cam'])
    print('frame {}: {} accepted, first pass {} inliers, guided pass {} inliers ({} returned), error {:.5f} m / {:.4f} deg, '
          'near the threshold {}, rounding margin {:.2e}'.format(f, r['first']['matched'].size, r['first']['keep'].size,
                                                                 r['guided']['keep'].size, r['used'], r['e_t'], r['e_rot_deg'], c['near'], c['margin']))
    assert c['first_inliers'] >= 3 * 12 and c['near'] == 0 and c['margin'] >= ms.ROUND_MARGIN
    assert r['used'] == 'guided' and r['guided']['keep'].size > 2 * r['first']['keep'].size
    assert r['e_t'] <= rs.TRUTH_BOUND[f][0] and r['e_rot_deg'] <= rs.TRUTH_BOUND[f][1]
    # the bounds are twice what was measured: the figures have not moved
    assert r['e_t'] > 0.49 * rs.TRUTH_BOUND[f][0] and r['e_rot_deg'] > 0.49 * rs.TRUTH_BOUND[f][1]
    # the useless prior of the GPU test: tracking with it fails on the host as well, and by no rounding
    assert ms.rounding_margin(pts, rs.useless_prior(), seq['cam']) >= ms.ROUND_MARGIN
    with pytest.raises(ValueError):
        ms.host_track(ms.frames()[f], pts, ms.true_map()[1], rs.useless_prior(), seq['cam'], 12, rs.RELOC_SEED + f)


def test_the_pipeline_with_a_flat_frame_recovers():
    images, at = rs.lost_images()
    ref, run = ms.host_pipeline_big(), rs.host_pipeline_lost_big()
    print('flat frame at {}: keyframes {} (uninterrupted {}), landmarks {}, relocalised {}'.format(at, run['keyframes'], ref['keyframes'],
                                                                                                   run['counts'], run['relocalised']))
    assert at == ref['keyframes'][2] + 1 and len(images) == len(ref['poses']) + 1
    for a, b in zip(run['poses'][:at], ref['poses'][:at]):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
    assert run['poses'][at] is None and run['lost'][at] and not any(run['lost'][at + 1:])
    assert run['relocalised'] == [at + 1] and all(T is not None for T in run['poses'][at + 1:])
    assert len(run['keyframes']) > 3                           # a keyframe after the recovery: the map goes on growing
    for c in run['checks']:
        print(c)
        assert c['near'] == 0 and c.get('margin', 1.) >= ms.ROUND_MARGIN
        assert c['what'] != 'relocalise' or c['first_inliers'] >= 3 * 12
    seq = ms.sequence()
    for f in range(at + 1, len(images)):
        e_t, e_rot = rs.pose_errors(run['poses'][f], seq['T_c_w'][f - 1])
        print('image {}: {:.4f} m / {:.3f} deg from the truth (map scale: that of the initialisation)'.format(f, e_t, e_rot))


# ---- the surface ----

def test_the_header_and_the_signature_table_hold_the_global_calls():
    from pyslam_amd import _native as nat
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, '..', 'include', 'pyslam_hip.h')).read()
    for name, nargs in (('ps_feat_match_map_global', 5), ('ps_feat_read_map_second', 3)):
        decl = re.search(r'int {}\(([^)]*)\);'.format(name), header)
        assert decl and len(decl.group(1).split(',')) == nargs == len(nat.SIGNATURES[name][1]), name


def test_the_exports_and_the_pipeline_attributes():
    import pyslam.pipelines
    import pyslam.pipelines.mono as shim
    import pyslam_amd.pipelines
    from pyslam_amd.pipelines import mono
    assert shim.relocalise_frame is mono.relocalise_frame and pyslam.pipelines.relocalise_frame is mono.relocalise_frame
    assert pyslam_amd.pipelines.relocalise_frame is mono.relocalise_frame and 'relocalise_frame' in mono.__all__
    p = mono.SparseMonoPipeline(ms.camera(ms.sequence(96, 128)['cam']))
    assert p.relocalise is True and p.reloc_ratio == (4, 5) and p.lost is False and p.relocalised == []
    assert 'match_map_global' in fp.__all__


def test_errors_that_need_no_device():
    from pyslam_amd import _native as nat
    from pyslam_amd.pipelines.matcher import Matcher
    from pyslam_amd.pipelines.mono import relocalise_frame
    cam = ms.camera(ms.sequence(96, 128)['cam'])
    image = np.zeros((96, 128), dtype=np.uint8)
    with pytest.raises(ValueError, match='the map is empty'):
        relocalise_frame(cam, None, image, np.zeros((0, 3)), np.zeros((0, 32), dtype=np.uint8))
    with pytest.raises(ValueError, match='3 landmarks and 2 descriptors'):
        relocalise_frame(cam, None, image, np.zeros((3, 3)), np.zeros((2, 32), dtype=np.uint8))
    with pytest.raises(nat.NativeError, match='push a frame'):
        Matcher().matchMapGlobal()
