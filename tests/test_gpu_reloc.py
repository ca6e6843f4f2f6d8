"""Matching without a prior on the device (csrc/ps_k_feat_global.h: k_feat_map_search_all, then k_feat_map_resolve;
Matcher.matchMapGlobal) against its restatement (featproc.match_map_global), the handle's behaviour around it, mono.relocalise_frame
on frames 5 and 9 of the 240 x 320 scene and SparseMonoPipeline through a flat frame.  Run with `-m gpu` on an MI355X.  Every
comparison prints its figure before it asserts.

Held on every case: feature, status, cost and second equal (int32), uv within 1e-12 pixel (the matcher's bound), the matched count
equal to the number of status-0 points, two device calls bit-identical.  What the comparisons rely on is asserted on the host for
every scene used here (tests/test_reloc_host.py over tests/reloc_scenes.py)."""
import ctypes as C

import numpy as np
import pytest

import mono_scenes as ms
import reloc_scenes as rs
from pyslam_amd import _native as nat
from pyslam_amd.pipelines import featproc as fp

pytestmark = pytest.mark.gpu

TOL_UV = 1e-12           # pixels (the matcher's existing bound)
TOL_POSE = 1e-7          # the bound of tests/test_gpu_mono_track.py


def matcher(**kw):
    from pyslam_amd.pipelines.matcher import Matcher, Matcher_parameters
    return Matcher(Matcher_parameters(**kw)), fp.Params(**kw)


def compare(m, hp, frame, desc, ratio=(4, 5), what=''):
    """One matchMapGlobal against the restatement; -> the host result."""
    dev = m.matchMapGlobal(ratio)
    matched = m.num_map_matched
    ref = fp.match_map_global(frame, desc, ratio, hp)
    again = m.matchMapGlobal(ratio)
    counts = np.bincount(ref[1], minlength=5).tolist() if len(ref[1]) else [0] * 5
    err = np.abs(dev[4] - ref[4]).max() if ref[4].size else 0.
    print('{} N = {}, F = {}, ratio {}: status counts {}, device matched {}, max |uv device - restatement| {:.2e}'.format(
        what, len(ref[0]), len(frame), ratio, counts, matched, err))
    for k in range(4):
        assert dev[k].dtype == np.int32 and np.array_equal(dev[k], ref[k]), ('feature', 'status', 'cost', 'second')[k]
    assert dev[4].shape == ref[4].shape and err <= TOL_UV
    assert matched == counts[0] and m.num_map_matched == counts[0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(dev, again))
    return ref


def points_for(desc):
    """Matching without a prior never reads the points."""
    return np.zeros((desc.shape[0], 3))


# ---- device = restatement ----

@pytest.mark.parametrize('frame', ms.SMALL_FRAMES)
@pytest.mark.parametrize('shape', ms.SMALL_SHAPES)
def test_true_map_without_a_prior(shape, frame):
    seq, fr = ms.sequence(*shape), ms.frames(*shape)
    pts, desc = ms.true_map(*shape)
    m, hp = matcher()
    try:
        m.pushBack(seq['images'][frame])
        m.setMap(pts, desc)
        for ratio in rs.RATIOS:
            ref = compare(m, hp, fr[frame], desc, ratio, '{} frame {}'.format(shape, frame))
            assert not (ref[1] == 1).any()
        assert (fp.match_map_global(fr[frame], desc, (4, 5))[1] == 0).sum() >= 50
    finally:
        m.close()


@pytest.mark.parametrize('n', rs.MAP_SIZES)
def test_map_sizes(n):
    seq, fr = ms.sequence(96, 128), ms.frames(96, 128)
    pts, desc = ms.true_map(96, 128)
    reps = -(-n // pts.shape[0]) if n else 1
    pts, desc = np.tile(pts, (reps, 1))[:n], np.tile(desc, (reps, 1))[:n]      # 257 points: the map once and most of it again
    m, hp = matcher()
    try:
        m.pushBack(seq['images'][1])
        m.setMap(pts, desc)
        ref = compare(m, hp, fr[1], desc, (4, 5), 'N = {}'.format(n))
        assert ref[0].shape == (n,) and ref[4].shape == (n, 2)
        assert n < 257 or (ref[1] == 3).any()
    finally:
        m.close()


def test_a_flat_frame_has_no_features():
    pts, desc = ms.true_map(96, 128)
    flat = np.full((96, 128), 117, dtype=np.uint8)
    m, hp = matcher()
    try:
        m.pushBack(flat)
        m.setMap(pts, desc)
        ref = compare(m, hp, fp.features(flat, hp), desc, (4, 5), 'flat')
        assert (ref[1] == 2).all() and (ref[3] == -1).all() and m.features(2)[0].shape == (0, 2)
    finally:
        m.close()


@pytest.mark.parametrize('max_features', rs.NOISE_MAX_FEATURES)
def test_feature_counts_at_the_lane_and_wave_edges(max_features):
    a, b = rs.noise_pair()
    kw = dict(max_features=max_features, **rs.NOISE_KW)
    m, hp = matcher(**kw)
    fa, fb = rs.noise_features(False, max_features)
    assert len(fb) == max_features
    desc = rs.noise_features(False)[0].desc if max_features == 1 else fa.desc
    try:
        m.pushBack(b)
        m.setMap(points_for(desc), desc)
        ref = compare(m, hp, fb, desc, (4, 5), 'noise, max_features {}'.format(max_features))
        if max_features == 1:
            assert (ref[3] == -1).all() and (ref[1] == 0).sum() == 1 and not (ref[1] == 4).any()
    finally:
        m.close()


def test_more_features_than_two_tiles():
    a, b = rs.big_noise_pair()
    m, hp = matcher(**rs.NOISE_KW)
    fa, fb = rs.noise_features(True)
    assert len(fb) > 2 * rs.kernel_tile() and len(fb) % rs.kernel_tile()
    try:
        m.pushBack(b)
        m.setMap(points_for(fa.desc), fa.desc)
        for ratio in rs.RATIOS:
            ref = compare(m, hp, fb, fa.desc, ratio, 'big noise')
        assert (ref[0] >= 2 * rs.kernel_tile()).any()
    finally:
        m.close()


# ---- claim and tie ----

def test_a_frames_own_descriptors():
    seq, fr = ms.sequence(96, 128), ms.frames(96, 128)
    f1 = fr[1]
    m, hp = matcher()
    try:
        m.pushBack(seq['images'][1])
        m.setMap(points_for(f1.desc), f1.desc)
        ref = compare(m, hp, f1, f1.desc, (4, 5), 'own descriptors')
        own = ref[3] > 0
        assert (ref[2] == 0).all() and own.sum() > 50 and np.array_equal(ref[0][own], np.nonzero(own)[0]) and (ref[1][own] == 0).all()
        # one point three times: the first keeps the feature
        k = int(np.nonzero(own)[0][17])
        d3 = np.concatenate([f1.desc[k:k + 1], f1.desc, f1.desc[k:k + 1]])
        m.setMap(points_for(d3), d3)
        ref = compare(m, hp, f1, d3, (4, 5), 'one point three times')
        assert ref[1][0] == 0 and ref[0][0] == k and ref[1][k + 1] == 3 and ref[1][-1] == 3 and ref[2][-1] == 0 and ref[0][-1] == -1
        # one descriptor repeated: whichever the restatement says
        same = np.repeat(f1.desc[k:k + 1], 70, axis=0)
        m.setMap(points_for(same), same)
        ref = compare(m, hp, f1, same, (4, 5), 'one descriptor 70 times')
        assert ref[1][0] == 0 and (ref[1][1:] == 3).all()
        twin = int(np.nonzero(~own)[0][0]) if (~own).any() else None
        if twin is not None:
            same = np.repeat(f1.desc[twin:twin + 1], 70, axis=0)
            m.setMap(points_for(same), same)
            ref = compare(m, hp, f1, same, (4, 5), 'one tied descriptor 70 times')
            assert (ref[1] == 4).all()
    finally:
        m.close()


def test_an_exact_tie_of_the_products():
    seq, fr = ms.sequence(96, 128), ms.frames(96, 128)
    pts, desc = ms.true_map(96, 128)
    i, tie, looser = rs.exact_tie_point(fr[1], desc)
    m, hp = matcher()
    try:
        m.pushBack(seq['images'][1])
        m.setMap(pts, desc)
        a = compare(m, hp, fr[1], desc, tie, 'exact tie')
        b = compare(m, hp, fr[1], desc, looser, 'next looser ratio')
        assert a[1][i] == 4 and b[1][i] in (0, 3)
        compare(m, hp, fr[1], desc, (32768, 32768), 'largest ratio integers')
    finally:
        m.close()


def test_without_refinement_positions_are_integers():
    seq, fr = ms.sequence(101, 139), ms.frames(101, 139)
    pts, desc = ms.true_map(101, 139)
    m, hp = matcher(refinement=0)
    try:
        m.pushBack(seq['images'][7])
        m.setMap(pts, desc)
        ref = compare(m, hp, fr[7], desc, (4, 5), 'refinement 0')
        ok = ref[1] == 0
        assert ok.sum() > 50 and np.array_equal(ref[4][ok], fr[7].uv[ref[0][ok]].astype(float))
    finally:
        m.close()
    assert (fp.match_map_global(fr[7], desc)[4][ok] != ref[4][ok]).any()


# ---- the handle ----

def test_errors():
    seq = ms.sequence(96, 128)
    pts, desc = ms.true_map(96, 128)
    m, _ = matcher()
    try:
        m.setMap(pts, desc)                                       # kept until there is a handle
        with pytest.raises(nat.NativeError, match='push a frame'):
            m.matchMapGlobal()
    finally:
        m.close()
    lib = nat.require_gpu()
    from pyslam_amd.pipelines.matcher import Matcher_parameters
    p = Matcher_parameters(max_features=256)._native()
    n = C.c_int32()
    h = nat.H()
    nat.check(lib.ps_feat_create(96, 128, 256, None, C.byref(h)))
    try:
        assert lib.ps_feat_match_map_global(h, 4, 5, C.byref(p), C.byref(n)) == -1 and b'push a frame' in lib.ps_last_error()
        im = np.ascontiguousarray(seq['images'][0])
        nat.check(lib.ps_feat_push(h, 96, 128, im.ctypes.data_as(nat.c_u8p), None))
        assert lib.ps_feat_match_map_global(h, 4, 5, C.byref(p), C.byref(n)) == -1 and b'set a map' in lib.ps_last_error()
        nat.check(lib.ps_feat_set_map(h, pts.shape[0], nat.f64p(pts), desc.ctypes.data_as(nat.c_u8p)))
        for num, den in ((0, 5), (6, 5), (4, 32769)):
            assert lib.ps_feat_match_map_global(h, num, den, C.byref(p), C.byref(n)) == -1 and b'ratio' in lib.ps_last_error()
        out = np.zeros(pts.shape[0] + 1, dtype=np.int32)
        assert lib.ps_feat_read_map_second(h, 1, nat.i32p(out)) == -1                       # nothing matched yet
        T, c = np.identity(4), np.array(tuple(seq['cam'][:4]) + (0.,))
        nat.check(lib.ps_feat_match_map(h, nat.f64p(T), nat.f64p(c), 8, C.byref(p), C.byref(n)))
        assert lib.ps_feat_read_map_second(h, 1, nat.i32p(out)) == -1 and b'not a global one' in lib.ps_last_error()
        nat.check(lib.ps_feat_match_map_global(h, 4, 5, C.byref(p), C.byref(n)))
        assert lib.ps_feat_read_map_second(h, pts.shape[0] + 1, nat.i32p(out)) == -1 and b'more points asked for' in lib.ps_last_error()
        assert lib.ps_feat_read_map_second(h, pts.shape[0], nat.i32p(out)) == 0 and lib.ps_feat_read_map_second(h, 3, None) == 0
        nat.check(lib.ps_feat_match_map(h, nat.f64p(T), nat.f64p(c), 8, C.byref(p), C.byref(n)))
        assert lib.ps_feat_read_map_second(h, 1, nat.i32p(out)) == -1
    finally:
        lib.ps_feat_destroy(h)


def test_device_bytes_and_the_other_matches_around_a_global_match():
    seq, fr = ms.sequence(96, 128), ms.frames(96, 128)
    pts, desc = ms.true_map(96, 128)
    m, hp = matcher(max_features=300)
    try:
        m.pushBack(seq['images'][0])
        m.pushBack(seq['images'][1])
        m.matchFeatures(0)
        flow = m.matches_array()
        m.setMap(pts[:5], desc[:5])
        guided = m.matchMap(seq['T_c_w'][1], seq['cam'], 8)
        with_map = m.device_bytes
        compare(m, hp, fr[1], desc[:5], (4, 5), 'small map')
        print('device bytes', with_map, '->', m.device_bytes)
        assert m.device_bytes == with_map + max(4 * 5, 16)
        again = m.matchMap(seq['T_c_w'][1], seq['cam'], 8)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(guided, again))
        m.setMap(pts, desc)                                         # the map grows: the second-best costs grow with it
        n = pts.shape[0]
        base = with_map - (5 * 24 + 5 * 32 + (16 + 5 * 28))
        assert m.device_bytes == base + n * (24 + 32) + (16 + n * 28) + 4 * n
        compare(m, hp, fr[1], desc, (4, 5), 'grown map')
        m.setMap(pts[:7], desc[:7])                                 # shrinking keeps the buffers
        assert m.device_bytes == base + n * (24 + 32) + (16 + n * 28) + 4 * n
        compare(m, hp, fr[1], desc[:7], (4, 5), 'shrunk map')
        m.setMap(pts[:5], desc[:5])
        again = m.matchMap(seq['T_c_w'][1], seq['cam'], 8)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(guided, again)) and (guided[1] == 0).any()
        m.matchFeatures(0)
        after = m.matches_array()
        assert after[0].tobytes() == flow[0].tobytes() and after[1].tobytes() == flow[1].tobytes() and flow[0].shape[0] > 50
    finally:
        m.close()
    # a handle whose first global match comes before any other map match, on an empty map
    m, hp = matcher(max_features=300)
    try:
        m.pushBack(seq['images'][1])
        m.setMap(pts[:0], desc[:0])
        before = m.device_bytes
        compare(m, hp, fr[1], desc[:0], (4, 5), 'empty map')
        assert m.device_bytes == before + 16
    finally:
        m.close()


# ---- relocalise_frame ----

@pytest.mark.parametrize('f', rs.RELOC_FRAMES)
def test_relocalise_frame_equals_the_host_composition(f):
    from pyslam_amd.pipelines.matcher import Matcher
    from pyslam_amd.pipelines.mono import relocalise_frame, track_frame
    seq = ms.sequence()
    pts, desc = ms.true_map()
    cam = ms.camera(seq['cam'])
    ref = rs.reloc_case(f)
    m = Matcher()
    try:
        with pytest.raises(ValueError):                             # the map matched under a useless prior first
            track_frame(cam, m, seq['images'][f], pts, desc, rs.useless_prior(), radius=12, seed=rs.RELOC_SEED + f)
        T_cw, keep, obs = relocalise_frame(cam, m, seq['images'][f], pts, desc, seed=rs.RELOC_SEED + f)
        assert m.feature_passes == 1
    finally:
        m.close()
    T = T_cw.as_matrix()
    e_rot, e_t = ms.rot_angle(T[:3, :3], ref['T'][:3, :3]), float(np.abs(T[:3, 3] - ref['T'][:3, 3]).max())
    t_t, t_rot = rs.pose_errors(T, seq['T_c_w'][f])
    print('frame {}: {} inliers (host {}, its {} pass), device vs host {:.2e} rad / {:.2e}, vs truth {:.5f} m / {:.4f} deg'.format(
        f, keep.size, ref['keep'].size, ref['used'], e_rot, e_t, t_t, t_rot))
    assert np.array_equal(keep, ref['keep'])
    assert np.abs(obs - ref['obs']).max() <= TOL_UV
    assert e_rot <= TOL_POSE and e_t <= TOL_POSE
    assert t_t <= rs.TRUTH_BOUND[f][0] and t_rot <= rs.TRUTH_BOUND[f][1]


# ---- the pipeline ----

def run_pipeline(local_ba, relocalise=True):
    from pyslam_amd.pipelines.mono import SparseMonoPipeline
    images, at = rs.lost_images()
    p = SparseMonoPipeline(ms.camera(ms.sequence()['cam']))
    p.local_ba = local_ba
    p.relocalise = relocalise
    p.lost_after = []
    np.random.seed(ms.PIPELINE_SEED)
    try:
        for im in images:
            p.track(im)
            p.lost_after.append(p.lost)
    finally:
        p.matcher.close()
    return p


def pose_gap(p, poses):
    worst = [0., 0.]
    for T, Th in zip(p.T_c_w, poses):
        assert (T is None) == (Th is None)
        if T is not None:
            Tm = T.as_matrix()
            worst = [max(worst[0], ms.rot_angle(Tm[:3, :3], Th[:3, :3])), max(worst[1], float(np.abs(Tm[:3, 3] - Th[:3, 3]).max()))]
    return worst


def test_pipeline_recovers_from_a_flat_frame():
    images, at = rs.lost_images()
    ref, plain = rs.host_pipeline_lost_big(), ms.host_pipeline_big()
    p = run_pipeline(False)
    kf_frames = [next(f for f, im in enumerate(images) if np.array_equal(im, kf.image)) for kf in p.keyframes]
    print('flat frame {}: lost after each frame {}, relocalised {} (host {}), keyframes {} (host {}), landmarks {} (host {})'.format(
        at, p.lost_after, p.relocalised, ref['relocalised'], kf_frames, ref['keyframes'], p.landmark_counts, ref['counts']))
    before = pose_gap(p, plain['poses'][:at])
    print('poses before the flat frame, device vs the uninterrupted host composition: {:.2e} rad / {:.2e}'.format(*before))
    assert before[0] <= TOL_POSE and before[1] <= TOL_POSE
    assert p.T_c_w[at] is None and p.lost_after[at] is True and p.lost_after[:at] == [False] * at
    assert p.relocalised == [at + 1] and p.lost_after[at + 1] is False and p.lost is False
    assert kf_frames == ref['keyframes'] and p.landmark_counts == ref['counts'] and p.ba_history == []
    assert len(p.T_c_w) == len(ref['poses'])
    worst = pose_gap(p, ref['poses'])
    print('all poses, device vs host composition with the lost state: {:.2e} rad / {:.2e}'.format(*worst))
    assert worst[0] <= TOL_POSE and worst[1] <= TOL_POSE


def test_pipeline_without_relocalisation_raises_on_the_flat_frame():
    images, at = rs.lost_images()
    from pyslam_amd.pipelines.mono import SparseMonoPipeline
    p = SparseMonoPipeline(ms.camera(ms.sequence()['cam']))
    p.local_ba = False
    p.relocalise = False
    np.random.seed(ms.PIPELINE_SEED)
    try:
        for im in images[:at]:
            p.track(im)
        with pytest.raises(ValueError):
            p.track(images[at])
        assert len(p.T_c_w) == at and p.lost is False and p.relocalised == []
    finally:
        p.matcher.close()


def test_pipeline_with_bundle_adjustment_recovers():
    images, at = rs.lost_images()
    p = run_pipeline(True)
    print('relocalised {}, keyframes {}, landmarks {}, bundle adjustments (start, final) {}'.format(p.relocalised, len(p.keyframes),
                                                                                                    p.landmark_counts, p.ba_costs))
    assert p.T_c_w[at] is None and p.relocalised == [at + 1]
    assert all(T is not None for T in p.T_c_w[at + 1:])
    assert len(p.ba_costs) >= 1 and len(p.ba_costs) == len(p.ba_history)
    for (start, final), hist in zip(p.ba_costs, p.ba_history):
        assert abs(start - hist[0]) <= 1e-9 * hist[0]
        assert final <= start * (1 + 1e-9) and np.isfinite(hist).all()
    R = np.stack([kf.T_c_w.as_matrix() for kf in p.keyframes])[p.obs_kf]
    z = np.einsum('nj,nj->n', R[:, 2, :3], p.points_w[p.obs_lm]) + R[:, 2, 3]
    assert p.alive.sum() > 100 and (z[p.alive[p.obs_lm]] > 0.).all()
