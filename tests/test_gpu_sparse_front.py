"""The device feature matcher (pipelines/matcher.py, csrc/ps_k_feat.h) against its numpy restatement
(pipelines/featproc.py): feature lists, integer matches and their order equal, sub-pixel positions within 1e-12 pixel
(the same expression on the same integers; the margin is for its one division), for the three modes, at KITTI and VGA
size, on sizes that are no multiple of a tile or of 4, on an image without texture and on one over capacity."""
import numpy as np
import pytest

from pyslam_amd import synthetic
from pyslam_amd.pipelines import featproc as fp

pytestmark = pytest.mark.gpu


def _params(**kw):
    from pyslam_amd.pipelines.matcher import Matcher_parameters
    return Matcher_parameters(**kw), fp.Params(**kw)


def _host_frame(left, right, hp):
    return fp.features(left, hp), (fp.features(right, hp) if right is not None else None)


def _check_features(m, which, host):
    uv, R, d = m.features(which)
    assert np.array_equal(uv, host.uv), (which, uv.shape, host.uv.shape)
    assert np.array_equal(R, host.R)
    assert np.array_equal(d, host.desc)


def _check_pair(prev, cur, modes, **kw):
    from pyslam_amd.pipelines.matcher import Matcher
    dp, hp = _params(**kw)
    m = Matcher(dp)
    stereo = prev[1] is not None
    hprev, hcur = _host_frame(prev[0], prev[1], hp), _host_frame(cur[0], cur[1], hp)
    counts = {}
    try:
        m.pushBack(*[x for x in prev if x is not None])
        m.pushBack(*[x for x in cur if x is not None])
        for mode in modes:
            m.matchFeatures(mode)
            dm, di = m.matches_array()
            hm, hi = fp.match(hprev, hcur, mode, hp)
            print('mode', mode, 'features', len(hprev[0]), len(hcur[0]), 'matches host', hm.shape[0], 'device', dm.shape[0],
                  'max |dpos|', np.abs(dm - hm).max() if dm.shape == hm.shape and hm.size else None)
            assert np.array_equal(di, hi), (mode, di.shape, hi.shape)
            assert dm.shape == hm.shape
            assert np.array_equal(np.round(dm), np.round(hm)) or hm.size == 0 or np.abs(dm - hm).max() <= 1e-12
            assert hm.size == 0 or np.abs(dm - hm).max() <= 1e-12, (mode, np.abs(dm - hm).max())
            dm2, di2 = (m.matchFeatures(mode), m.matches_array())[1]
            assert dm2.tobytes() == dm.tobytes() and di2.tobytes() == di.tobytes()
            counts[mode] = hm.shape[0]
        _check_features(m, 0, hprev[0])
        _check_features(m, 2, hcur[0])
        if stereo:
            _check_features(m, 1, hprev[1])
            _check_features(m, 3, hcur[1])
    finally:
        m.close()
    return counts


@pytest.mark.parametrize('shape', [(375, 1242), (480, 640), (96, 128), (101, 139)])
def test_stereo_scene_all_modes(shape):
    seq = synthetic.stereo_sequence(shape[0], shape[1], 2, seed=2, cell=0.3, step=(0.01, -0.005, 0.02, 0.006, 0.0075, -0.003))
    counts = _check_pair((seq['left'][0], seq['right'][0]), (seq['left'][1], seq['right'][1]), (0, 1, 2))
    assert min(counts.values()) >= 50, counts


def test_flow_on_single_images_and_odd_width():
    seq = synthetic.stereo_sequence(77, 131, 2, seed=5, cell=0.3)
    counts = _check_pair((seq['left'][0], None), (seq['left'][1], None), (0,))
    assert counts[0] > 20


def test_without_refinement_positions_are_integers():
    seq = synthetic.stereo_sequence(96, 128, 2, seed=2, cell=0.3)
    _check_pair((seq['left'][0], seq['right'][0]), (seq['left'][1], seq['right'][1]), (0, 1, 2), refinement=0)


def test_random_noise_images_and_small_windows():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(67, 93)).astype(np.uint8)
    b = np.roll(a, (1, 2), axis=(0, 1))
    _check_pair((a, b), (b, a), (0, 1, 2), match_radius_u=7, match_radius_v=3, disp_max=5, nms_n=1, match_cost_max=4000)
    _check_pair((a, b), (b, a), (0, 2), nms_n=3, response_threshold=0)


def test_no_texture_gives_no_features_and_no_matches():
    from pyslam_amd.pipelines.matcher import Matcher
    flat = np.full((60, 80), 117, dtype=np.uint8)
    counts = _check_pair((flat, flat), (flat.copy(), flat.copy()), (0, 1, 2))
    assert counts == {0: 0, 1: 0, 2: 0}
    m = Matcher()
    try:
        m.pushBack(flat)
        m.pushBack(flat + 1)
        m.matchFeatures(0)
        assert m.getMatches() == [] and m.features(0)[0].shape == (0, 2)
    finally:
        m.close()


def test_over_capacity_keeps_the_strongest_in_raster_order():
    rng = np.random.default_rng(11)
    img = (rng.integers(0, 2, size=(120, 160)) * rng.integers(60, 256, size=(120, 160))).astype(np.uint8)
    full = fp.features(img, fp.Params(max_features=1 << 20))
    assert len(full) > 3 * 64
    img2 = np.roll(img, 1, axis=1)
    counts = _check_pair((img, img2), (img2, img), (0, 2), max_features=64)
    assert counts[0] > 0
    capped = fp.features(img, fp.Params(max_features=64))
    assert len(capped) == 64 and capped.R.min() >= np.sort(full.R)[-64]


def test_pushing_the_active_keyframe_again_adds_no_feature_pass():
    from pyslam_amd.pipelines.matcher import Matcher
    seq = synthetic.stereo_sequence(96, 128, 4, seed=2, cell=0.3)
    m = Matcher()
    try:
        first = None
        for f in (1, 2, 3):
            m.pushBack(seq['left'][0].copy(), seq['right'][0].copy())     # the keyframe, as a new array object every time
            m.pushBack(seq['left'][f], seq['right'][f])
            m.matchFeatures(2)
            if first is None:
                first = m.matches_array()
                assert m.feature_passes == 4
        assert m.feature_passes == 8, m.feature_passes           # two images per new frame, none for the keyframe
        m.pushBack(seq['left'][0], seq['right'][0])
        m.pushBack(seq['left'][1], seq['right'][1])               # left the three-frame window: computed again
        m.matchFeatures(2)
        again = m.matches_array()
        assert m.feature_passes == 10
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    finally:
        m.close()
