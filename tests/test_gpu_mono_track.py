"""Matching by projection on the device (csrc/ps_k_feat.h: k_feat_map_search, k_feat_map_resolve; Matcher.setMap / matchMap)
against its restatement (featproc.match_map), the handle's behaviour around a map, mono.track_frame on the true-map chain and
SparseMonoPipeline on the 240 x 320 scene.  Run with `-m gpu` on an MI355X.  Every comparison prints its figure before it asserts.

Held on every case: feature, status and cost equal, uv within 1e-12 pixel (the matcher's bound: the same expression on the same
integers; the margin is for its one division), two device calls bit-identical.  What the comparisons rely on -- no projected
coordinate within 1e-6 pixel of a rounding boundary, no PnP squared error within 1e-6 relative of the threshold, ties decided by
the lower index -- is asserted on the host for every scene used here (tests/test_mono_track_host.py over tests/mono_scenes.py)."""
import numpy as np
import pytest

import mono_scenes as ms
from pyslam_amd import _native as nat
from pyslam_amd.pipelines import featproc as fp

pytestmark = pytest.mark.gpu

TOL_UV = 1e-12           # pixels (the matcher's existing bound)
TOL_POSE = 1e-7          # rotation angle (rad) and translation: 100 x TOL_POSE of tests/test_gpu_pnp.py (the issue's bound)


def matcher(**kw):
    from pyslam_amd.pipelines.matcher import Matcher, Matcher_parameters
    return Matcher(Matcher_parameters(**kw)), fp.Params(**kw)


def compare(m, hp, frame, pts, desc, T, cam, radius, what=''):
    """One matchMap against the restatement; -> the host result."""
    dev = m.matchMap(T, cam, radius)
    ref = fp.match_map(frame, pts, desc, T, cam, radius, hp)
    again = m.matchMap(T, cam, radius)
    counts = np.bincount(ref[1], minlength=4).tolist() if len(ref[1]) else [0, 0, 0, 0]
    err = np.abs(dev[3] - ref[3]).max() if ref[3].size else 0.
    print('{} N = {}, radius {}: status counts {}, device matched {}, max |uv device - restatement| {:.2e}'.format(
        what, len(ref[0]), radius, counts, m.num_map_matched, err))
    for k in range(3):
        assert dev[k].dtype == np.int32 and np.array_equal(dev[k], ref[k]), ('feature', 'status', 'cost')[k]
    assert dev[3].shape == ref[3].shape and err <= TOL_UV
    assert m.num_map_matched == counts[0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(dev, again))
    return ref


# ---- device = restatement ----

@pytest.mark.parametrize('frame', ms.SMALL_FRAMES)
@pytest.mark.parametrize('shape', ms.SMALL_SHAPES)
def test_true_map_at_the_true_pose(shape, frame):
    seq, fr = ms.sequence(*shape), ms.frames(*shape)
    pts, desc = ms.true_map(*shape)
    m, hp = matcher()
    try:
        m.pushBack(seq['images'][frame])
        m.setMap(pts, desc)
        matched = {}
        for radius in ms.SMALL_RADII:
            ref = compare(m, hp, fr[frame], pts, desc, seq['T_c_w'][frame], seq['cam'], radius, '{} frame {}'.format(shape, frame))
            matched[radius] = int((ref[1] == 0).sum())
        assert matched[8] >= 50 and matched[0] < matched[1]
        assert (fp.match_map(fr[frame], pts, desc, seq['T_c_w'][frame], seq['cam'], 40, hp)[1] == 3).any()
    finally:
        m.close()


@pytest.fixture(scope='module')
def noise():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(67, 93)).astype(np.uint8)
    return a, np.roll(a, (1, 2), axis=(0, 1))


def noise_map(frame, cam, z=2.0):
    u, v = frame.uv[:, 0].astype(float), frame.uv[:, 1].astype(float)
    return np.stack([(u - cam[0]) * z / cam[2], (v - cam[1]) * z / cam[3], np.full(len(frame), z)], axis=1), frame.desc


NOISE_CAM = (46., 33., 80., 80., 93, 67)


def test_noise_images_fill_a_window_with_more_than_64_candidates(noise):
    a, b = noise
    kw = dict(nms_n=1, response_threshold=0, match_cost_max=4000)
    m, hp = matcher(**kw)
    fa, fb = fp.features(a, hp), fp.features(b, hp)
    pts, desc = noise_map(fa, NOISE_CAM)
    inside = (np.abs(fb.uv[:, None, 0] - fa.uv[None, :, 0] - 2) <= 40) & (np.abs(fb.uv[:, None, 1] - fa.uv[None, :, 1] - 1) <= 40)
    print('features', len(fa), len(fb), 'candidates per window', inside.sum(axis=0).min(), '..', inside.sum(axis=0).max())
    assert inside.sum(axis=0).min() > 64
    T = np.identity(4)
    T[0, 3], T[1, 3] = 2 * 2.0 / NOISE_CAM[2], 1 * 2.0 / NOISE_CAM[3]        # the roll, as a translation at depth 2
    try:
        m.pushBack(b)
        m.setMap(pts, desc)
        ref = compare(m, hp, fb, pts, desc, T, NOISE_CAM, 40, 'noise')
        assert (ref[1] == 0).sum() > 64
        # the tie rule: every descriptor the same, so every candidate of a window ties and the lowest index wins
        same = np.repeat(desc[:1], len(desc), axis=0)
        m.setMap(pts, same)
        ref = compare(m, hp, fb, pts, same, T, NOISE_CAM, 40, 'noise, one descriptor')
        assert (ref[1] == 3).sum() > 0
    finally:
        m.close()


@pytest.mark.parametrize('n', [0, 1, 5, 65])
def test_map_sizes(n):
    seq, fr = ms.sequence(96, 128), ms.frames(96, 128)
    pts, desc = ms.true_map(96, 128)
    assert pts.shape[0] >= 65
    m, hp = matcher()
    try:
        m.pushBack(seq['images'][1])
        m.setMap(pts[:n], desc[:n])
        ref = compare(m, hp, fr[1], pts[:n], desc[:n], seq['T_c_w'][1], seq['cam'], 8, 'N = {}'.format(n))
        assert ref[0].shape == (n,) and ref[3].shape == (n, 2)
    finally:
        m.close()


def test_a_map_of_max_features_points_on_a_frame_over_capacity(noise):
    a, b = noise
    kw = dict(nms_n=1, response_threshold=0, match_cost_max=4000, max_features=64)
    m, hp = matcher(**kw)
    fa, fb = fp.features(a, hp), fp.features(b, hp)
    assert len(fa) == 64 and len(fb) == 64
    pts, desc = noise_map(fa, NOISE_CAM)
    try:
        m.pushBack(b)
        m.setMap(pts, desc)
        compare(m, hp, fb, pts, desc, np.identity(4), NOISE_CAM, 12, 'N = max_features = 64')
    finally:
        m.close()


def test_points_behind_the_camera_nan_points_and_border_centres():
    seq, fr = ms.sequence(96, 128), ms.frames(96, 128)
    cam = seq['cam']
    w, h = cam[4], cam[5]

    def at(u, v, z=2.0):
        return [(u - cam[0]) * z / cam[2], (v - cam[1]) * z / cam[3], z]
    odd = np.array([at(20, 20, 0.0), at(20, 20, -1.0), [np.nan, 0., 2.], [0., 0., np.nan], [np.inf, 0., 2.], [1e308, 1e308, 1e-308],
                    at(-0.75, 20), at(w - 0.25, 20), at(20, -0.75), at(20, h - 0.25),
                    at(-0.25, 20), at(w - 0.75, 20), at(20, -0.25), at(20, h - 0.75)])
    pts, desc = ms.true_map(96, 128)
    allp = np.concatenate([odd, pts, odd])
    alld = np.concatenate([np.zeros((len(odd), 32), dtype=np.uint8), desc, np.full((len(odd), 32), 255, dtype=np.uint8)])
    m, hp = matcher()
    try:
        m.pushBack(seq['images'][0])
        m.setMap(allp, alld)
        for radius in (3, 40, 1 << 30):
            ref = compare(m, hp, fr[0], allp, alld, seq['T_c_w'][0], cam, radius, 'odd points')
            assert ref[1][:10].tolist() == [1] * 10 and ref[1][-len(odd):][:10].tolist() == [1] * 10
            assert (ref[1][10:len(odd)] != 1).all()
    finally:
        m.close()


def test_a_point_listed_twice():
    seq, fr = ms.sequence(96, 128), ms.frames(96, 128)
    pts, desc = ms.true_map(96, 128)
    k = 17
    p2, d2 = np.concatenate([pts[k:k + 1], pts, pts[k:k + 1]]), np.concatenate([desc[k:k + 1], desc, desc[k:k + 1]])
    m, hp = matcher()
    try:
        m.pushBack(seq['images'][0])
        m.setMap(p2, d2)
        ref = compare(m, hp, fr[0], p2, d2, seq['T_c_w'][0], seq['cam'], 8, 'one point three times')
        assert ref[1][0] == 0 and ref[0][0] == k and ref[1][k + 1] == 3 and ref[1][-1] == 3 and ref[2][-1] == 0
    finally:
        m.close()


def test_without_refinement_positions_are_integers():
    seq, fr = ms.sequence(101, 139), ms.frames(101, 139)
    pts, desc = ms.true_map(101, 139)
    m, hp = matcher(refinement=0)
    try:
        m.pushBack(seq['images'][7])
        m.setMap(pts, desc)
        ref = compare(m, hp, fr[7], pts, desc, seq['T_c_w'][7], seq['cam'], 8, 'refinement 0')
        ok = ref[1] == 0
        assert ok.sum() > 50 and np.array_equal(ref[3][ok], fr[7].uv[ref[0][ok]].astype(float))
    finally:
        m.close()
    with_ref = fp.match_map(fr[7], pts, desc, seq['T_c_w'][7], seq['cam'], 8)
    assert (with_ref[3][ok] != ref[3][ok]).any()


def test_a_textureless_frame_has_no_candidates():
    seq = ms.sequence(96, 128)
    pts, desc = ms.true_map(96, 128)
    flat = np.full((96, 128), 117, dtype=np.uint8)
    m, hp = matcher()
    try:
        m.pushBack(flat)
        m.setMap(pts, desc)
        ref = compare(m, hp, fp.features(flat, hp), pts, desc, seq['T_c_w'][0], seq['cam'], 40, 'flat')
        assert (ref[1] == 2).all() and m.features(2)[0].shape == (0, 2)
    finally:
        m.close()


# ---- the handle ----

def test_matching_a_map_without_a_frame_or_without_a_map_is_an_error():
    seq = ms.sequence(96, 128)
    pts, desc = ms.true_map(96, 128)
    m, _ = matcher()
    try:
        with pytest.raises(nat.NativeError, match='push a frame'):
            m.matchMap(np.identity(4), seq['cam'], 8)
        m.setMap(pts, desc)                                       # kept until there is a handle
        with pytest.raises(nat.NativeError, match='push a frame'):
            m.matchMap(np.identity(4), seq['cam'], 8)
    finally:
        m.close()
    m, _ = matcher()
    try:
        m.pushBack(seq['images'][0])
        with pytest.raises(nat.NativeError, match='set a map'):
            m.matchMap(np.identity(4), seq['cam'], 8)
        m.setMap(pts, desc)
        with pytest.raises(nat.NativeError, match='negative matching radius'):
            m.matchMap(np.identity(4), seq['cam'], -1)
        assert (m.matchMap(seq['T_c_w'][0], seq['cam'], 8)[1] == 0).sum() > 50
        lib = nat.load()
        n = np.zeros(pts.shape[0] + 1, dtype=np.int32)
        assert lib.ps_feat_read_map_matches(m._h, pts.shape[0] + 1, nat.i32p(n), None, None, None) == -1
        assert b'more points asked for' in lib.ps_last_error()
        assert lib.ps_feat_read_map_matches(m._h, 3, None, None, None, None) == 0
        assert lib.ps_feat_set_map(m._h, (1 << 20) + 1, nat.f64p(pts), desc.ctypes.data_as(nat.c_u8p)) == -1
        assert lib.ps_feat_set_map(m._h, 4, None, None) == -1
    finally:
        m.close()
    # the handle itself, before any frame
    lib = nat.require_gpu()
    h = nat.H()
    nat.check(lib.ps_feat_create(96, 128, 256, None, np.ctypeslib.ctypes.byref(h)))
    try:
        from pyslam_amd.pipelines.matcher import Matcher_parameters
        p = Matcher_parameters(max_features=256)._native()
        n = np.zeros(1, dtype=np.int32)
        T, c = np.identity(4), np.array(seq['cam'][:4] + (0.,))
        assert lib.ps_feat_match_map(h, nat.f64p(T), nat.f64p(c), 8, np.ctypeslib.ctypes.byref(p), nat.i32p(n)) == -1
        assert b'push a frame' in lib.ps_last_error()
        assert lib.ps_feat_read_map_matches(h, 0, None, None, None, None) == -1
    finally:
        lib.ps_feat_destroy(h)


def parent_device_bytes(h, w, M):
    """What ps_feat_create allocates (csrc/ps_abi_feat.h), every buffer at least 16 bytes."""
    def b(n, size):
        return max(n * size, 16)
    P, Rc = h * w, ((h + 1) // 2) * ((w + 1) // 2)
    image = b(P, 1) + 2 * b(P, 2) + b(M, 8) + b(M, 8) + b(8 * M, 4) + b(h + 1, 4) + b(1, 4)
    scratch = (b(P, 8) + b(Rc, 8) + b(P, 1) + b(Rc, 1) + b(M, 1) + b((max(P, Rc, M) + 255) // 256 + 1, 4) + b(1, 4) + b(4 * M, 4) +
               b(4 * M, 4) + b(1, 4) + b(Rc, 8) + b(8 * M, 8) + 4 * b(M, 4))
    return 6 * image + scratch


def test_a_handle_without_a_map_holds_what_it_was_created_with_and_a_map_grows():
    seq, fr = ms.sequence(96, 128), ms.frames(96, 128)
    pts, desc = ms.true_map(96, 128)
    m, hp = matcher(max_features=300)
    try:
        m.pushBack(seq['images'][0])
        m.pushBack(seq['images'][1])
        m.matchFeatures(0)
        before = m.matches_array()
        base = m.device_bytes
        print('device bytes', base, 'formula', parent_device_bytes(96, 128, 300))
        assert base == parent_device_bytes(96, 128, 300)
        m.setMap(pts[:5], desc[:5])                                 # a small map first, then a larger one
        small = m.device_bytes
        assert small == base + 300 * 8 + 5 * 24 + 5 * 32 + (16 + 5 * 28)        # claims, points, descriptors, results
        compare(m, hp, fr[1], pts[:5], desc[:5], seq['T_c_w'][1], seq['cam'], 8, 'small map')
        m.setMap(pts, desc)
        n = pts.shape[0]
        assert m.device_bytes == base + 300 * 8 + n * (24 + 32) + (16 + n * 28)
        compare(m, hp, fr[1], pts, desc, seq['T_c_w'][1], seq['cam'], 8, 'grown map')
        m.setMap(pts[:7], desc[:7])                                 # shrinking keeps the buffers
        assert m.device_bytes == base + 300 * 8 + n * (24 + 32) + (16 + n * 28)
        compare(m, hp, fr[1], pts[:7], desc[:7], seq['T_c_w'][1], seq['cam'], 8, 'shrunk map')
        m.matchFeatures(0)                                          # the flow match of the pair is what it was
        after = m.matches_array()
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes() and before[0].shape[0] > 50
    finally:
        m.close()


# ---- track_frame on the true-map chain ----

@pytest.mark.parametrize('radius', ms.CHAIN_RADII)
def test_track_frame_on_the_true_map_chain(radius):
    from pyslam_amd.pipelines.matcher import Matcher
    from pyslam_amd.pipelines.mono import track_frame
    seq = ms.sequence()
    pts, desc = ms.true_map()
    cam = ms.camera(seq['cam'])
    chain = ms.host_chain(radius)
    m = Matcher()
    T = seq['T_c_w'][0].copy()
    worst = [0., 0., 0., 0.]
    try:
        for r in chain:
            f = r['frame']
            T_cw, keep, obs = track_frame(cam, m, seq['images'][f], pts, desc, T, radius=radius, seed=ms.CHAIN_SEED + f)
            T = T_cw.as_matrix()
            e_rot, e_t = ms.rot_angle(T[:3, :3], r['T'][:3, :3]), float(np.abs(T[:3, 3] - r['T'][:3, 3]).max())
            Tt = seq['T_c_w'][f]
            t_t, t_rot = float(np.linalg.norm(T[:3, 3] - Tt[:3, 3])), float(np.degrees(ms.rot_angle(T[:3, :3], Tt[:3, :3])))
            worst = [max(a, b) for a, b in zip(worst, (e_rot, e_t, t_t, t_rot))]
            print('radius {} frame {}: {} inliers (host {}), device vs host chain {:.2e} rad / {:.2e}, vs truth {:.4f} m / {:.3f} deg'.format(
                radius, f, keep.size, r['keep'].size, e_rot, e_t, t_t, t_rot))
            assert np.array_equal(keep, r['keep'])
            assert np.abs(obs - r['obs']).max() <= TOL_UV
            assert e_rot <= TOL_POSE and e_t <= TOL_POSE
        assert m.feature_passes == len(chain)
    finally:
        m.close()
    assert worst[2] <= ms.TRUTH_BOUND[radius][0] and worst[3] <= ms.TRUTH_BOUND[radius][1]


def test_track_frame_widens_the_window_once():
    """mono_scenes.widened_case: radius 3 matches fewer points than min_inliers = 500, radius 6 enough."""
    from pyslam_amd.pipelines.matcher import Matcher
    from pyslam_amd.pipelines.mono import track_frame
    from pyslam_amd.pipelines.pnp import PnPRANSAC
    seq = ms.sequence()
    pts, desc = ms.true_map()
    T_prior, ref = ms.widened_case()
    assert ref['radius'] == 6 and ref['keep'].size >= 500
    rs = PnPRANSAC(ms.camera(seq['cam']))
    rs.min_inliers = 500
    m = Matcher()
    try:
        T_cw, keep, obs = track_frame(rs.camera, m, seq['images'][1], pts, desc, T_prior, radius=3, seed=11, ransac=rs)
    finally:
        m.close()
    print('widened: {} inliers (host {})'.format(keep.size, ref['keep'].size))
    assert np.array_equal(keep, ref['keep']) and np.abs(T_cw.as_matrix() - ref['T']).max() <= TOL_POSE


# ---- the pipeline ----

def run_pipeline(local_ba):
    from pyslam_amd.pipelines.mono import SparseMonoPipeline
    seq = ms.sequence()
    p = SparseMonoPipeline(ms.camera(seq['cam']))
    p.local_ba = local_ba
    np.random.seed(ms.PIPELINE_SEED)
    try:
        for im in seq['images']:
            p.track(im)
    finally:
        p.matcher.close()
    return p


def test_pipeline_without_bundle_adjustment_equals_the_host_composition():
    seq = ms.sequence()
    ref = ms.host_pipeline_big()
    p = run_pipeline(False)
    init = next(f for f, T in enumerate(p.T_c_w) if f > 0 and T is not None)
    kf_frames = [next(f for f, im in enumerate(seq['images']) if np.array_equal(im, kf.image)) for kf in p.keyframes]
    print('initialised on frame {} (host {}), keyframes {} (host {}), landmarks {} (host {})'.format(
        init, ref['init_frame'], kf_frames, ref['keyframes'], p.landmark_counts, ref['counts']))
    assert init == ref['init_frame'] and kf_frames == ref['keyframes'] and p.landmark_counts == ref['counts']
    assert len(kf_frames) >= 3 and p.ba_history == []
    worst = [0., 0.]
    for f, (T, Th) in enumerate(zip(p.T_c_w, ref['poses'])):
        assert (T is None) == (Th is None)
        if T is not None:
            Tm = T.as_matrix()
            worst = [max(worst[0], ms.rot_angle(Tm[:3, :3], Th[:3, :3])), max(worst[1], float(np.abs(Tm[:3, 3] - Th[:3, 3]).max()))]
    print('poses device vs host composition: {:.2e} rad / {:.2e}'.format(*worst))
    assert worst[0] <= TOL_POSE and worst[1] <= TOL_POSE


def test_pipeline_with_bundle_adjustment():
    p = run_pipeline(True)
    init = next(f for f, T in enumerate(p.T_c_w) if f > 0 and T is not None)
    assert all(T is not None for T in p.T_c_w[init:])
    print('keyframes {}, landmarks {}, bundle adjustments (start, final) {}'.format(len(p.keyframes), p.landmark_counts, p.ba_costs))
    assert len(p.ba_costs) >= 1 and len(p.ba_costs) == len(p.ba_history)
    for (start, final), hist in zip(p.ba_costs, p.ba_history):
        # the start cost on the host against the device's: a residual is a difference of pixel coordinates up to 320 evaluated to
        # a few ulps against residuals of ~0.1 px
        assert abs(start - hist[0]) <= 1e-9 * hist[0]
        assert final <= start * (1 + 1e-9) and np.isfinite(hist).all()
    R = np.stack([kf.T_c_w.as_matrix() for kf in p.keyframes])[p.obs_kf]
    z = np.einsum('nj,nj->n', R[:, 2, :3], p.points_w[p.obs_lm]) + R[:, 2, 3]
    assert p.alive.sum() > 100 and (z[p.alive[p.obs_lm]] > 0.).all()
