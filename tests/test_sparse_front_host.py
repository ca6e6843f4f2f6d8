"""The numpy restatement of the sparse front end (pyslam_amd/pipelines/featproc.py): known answers, and its matches
against the true correspondences of synthetic.stereo_sequence."""
import numpy as np
import pytest

from pyslam_amd import synthetic
from pyslam_amd.pipelines import featproc as fp

HALF_STEP = (0.01, -0.005, 0.02, 0.006, 0.0075, -0.003)


def _blocks(seed=0, rows=12, cols=16, size=8):
    rng = np.random.default_rng(seed)
    return rng.integers(20, 236, (rows, cols)).astype(np.uint8).repeat(size, 0).repeat(size, 1)


def test_a_bright_square_gives_its_four_corners():
    img = np.zeros((64, 64), dtype=np.uint8)
    img[20:40, 24:44] = 255
    f = fp.features(img)
    assert f.uv.tolist() == [[25, 21], [42, 21], [25, 38], [42, 38]]      # raster order, one pixel inside each corner
    assert len(set(f.R.tolist())) == 1 and f.R[0] > 0
    assert f.desc.shape == (4, 32) and f.desc.dtype == np.uint8
    assert f.row_start[21] == 0 and f.row_start[22] == 2 and f.row_start[39] == 4 and f.row_start.shape == (65,)


def test_gradients_are_the_integer_sobel_with_replicated_borders():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (9, 11)).astype(np.uint8)
    du, dv = fp.gradients(img)
    assert du.dtype == np.int16 and dv.dtype == np.int16
    p = np.pad(img.astype(int), 1, mode='edge')
    for (y, x) in [(0, 0), (4, 5), (8, 10), (0, 10)]:
        win = p[y:y + 3, x:x + 3]
        assert du[y, x] == (win[:, 2] - win[:, 0]) @ [1, 2, 1]
        assert dv[y, x] == (win[2] - win[0]) @ [1, 2, 1]
    ramp = np.tile(np.arange(0, 220, 20, dtype=np.uint8), (9, 1))
    assert np.all(fp.gradients(ramp)[0][:, 1:-1] == 160) and np.all(fp.gradients(ramp)[1] == 0)


@pytest.mark.parametrize('refinement', [0, 1])
def test_identical_frames_give_zero_flow(refinement):
    fa = fp.features(_blocks())
    m, idx = fp.match((fa, None), (fa, None), 0, fp.Params(refinement=refinement))
    assert m.shape[0] > 5
    assert np.array_equal(m[:, 0:2], m[:, 4:6]) and np.array_equal(idx[:, 0], idx[:, 2])
    assert np.all(m[:, 2:4] == -1) and np.all(m[:, 6:8] == -1) and np.all(idx[:, [1, 3]] == -1)
    assert np.all(np.diff(idx[:, 0]) > 0)                          # in the order of the previous-left feature


@pytest.mark.parametrize('refinement', [0, 1])
def test_an_integer_shift_gives_that_shift(refinement):
    """Two crops of one texture, 5 pixels apart in u and 3 in v.  Away from the borders the two descriptors of a match
    are equal (cost 0), so the shift is exact with and without refinement; a descriptor that reaches the border row
    sees a replicated gradient there and may move by a fraction of a pixel."""
    big = _blocks(rows=14, cols=18)
    a, b = big[8:104, 8:136], big[5:101, 3:131]
    m, _ = fp.match((fp.features(a), None), (fp.features(b), None), 0, fp.Params(refinement=refinement))
    assert m.shape[0] > 5
    inner = (m[:, 0] >= 8) & (m[:, 0] < 128 - 13) & (m[:, 1] >= 8) & (m[:, 1] < 96 - 11)
    assert inner.sum() > 5
    assert np.all(m[inner, 4] - m[inner, 0] == 5) and np.all(m[inner, 5] - m[inner, 1] == 3)
    assert np.all(np.abs(m[:, 4] - m[:, 0] - 5) <= 0.5) and np.all(np.abs(m[:, 5] - m[:, 1] - 3) <= 0.5)


def test_stereo_and_quad_of_a_shifted_pair():
    left = _blocks(seed=4)
    right = np.roll(left, -4, axis=1)                              # disparity 4 everywhere
    fl, fr = fp.features(left), fp.features(right)
    m, idx = fp.match(None, (fl, fr), 1)
    assert m.shape[0] > 5 and np.all(m[:, 4] - m[:, 6] == 4) and np.all(m[:, 5] == m[:, 7]) and np.all(m[:, 0:4] == -1)
    q, qi = fp.match((fl, fr), (fl, fr), 2)
    assert q.shape[0] > 5 and np.array_equal(q[:, 0:4], q[:, 4:8]) and np.all(q[:, 0] - q[:, 2] == 4)
    # the stereo window: 0 <= u_left - u_right <= disp_max, rows at most 1 apart
    w, _ = fp.match(None, (fr, fl), 1, fp.Params(refinement=0, disp_max=9))
    assert np.all((w[:, 4] - w[:, 6] >= 0) & (w[:, 4] - w[:, 6] <= 9) & (np.abs(w[:, 5] - w[:, 7]) <= 1))


def test_no_texture_gives_no_features_and_no_matches():
    flat = np.full((40, 50), 90, dtype=np.uint8)
    f = fp.features(flat)
    assert len(f) == 0 and f.uv.shape == (0, 2) and f.desc.shape == (0, 32)
    for mode in (0, 1, 2):
        m, idx = fp.match((f, f), (f, f), mode)
        assert m.shape == (0, 8) and idx.shape == (0, 4)
    tiny = fp.features(np.zeros((4, 7), dtype=np.uint8))
    assert len(tiny) == 0


def test_over_capacity_keeps_the_strongest_in_raster_order():
    img = _blocks(seed=2, rows=20, cols=24)
    full = fp.features(img, fp.Params(max_features=1 << 20))
    cap = len(full) // 3
    assert cap > 10
    f = fp.features(img, fp.Params(max_features=cap))
    assert len(f) == cap
    order = np.lexsort((np.arange(len(full)), -full.R))[:cap]
    keep = np.sort(order)
    assert np.array_equal(f.uv, full.uv[keep]) and np.array_equal(f.R, full.R[keep]) and np.array_equal(f.desc, full.desc[keep])
    lin = f.uv[:, 1].astype(int) * img.shape[1] + f.uv[:, 0]
    assert np.all(np.diff(lin) > 0)


def test_bad_input_is_refused():
    with pytest.raises(TypeError):
        fp.features(np.zeros((20, 20)))
    with pytest.raises(ValueError):
        fp.features(np.zeros((20, 20), dtype=np.uint8), fp.Params(nms_n=0))
    with pytest.raises(TypeError):
        fp.Params(no_such=1)


@pytest.mark.parametrize('shape', [(96, 128), (101, 139)])
def test_quad_matches_against_the_true_correspondences(shape):
    """At least 100 quad matches per frame pair, and at most 20 % of them further than 1.5 pixels from the truth in any
    of the four images (the outlier share synthetic.motion_only(outlier_fraction=0.2) already feeds RANSAC).  Scene:
    0.3 m texture cells, half of rgbd_sequence's step between frames, seed 1, 8 frames.  Measured here (default
    parameters): 96 x 128: 108 .. 128 matches, worst pair 4.6 % outliers; 101 x 139: 132 .. 138 matches, worst pair
    6.8 %."""
    seq = synthetic.stereo_sequence(shape[0], shape[1], 8, seed=1, cell=0.3, step=HALF_STEP)
    fr = [(fp.features(seq['left'][f]), fp.features(seq['right'][f])) for f in range(8)]
    for f in range(7):
        m, idx = fp.match(fr[f], fr[f + 1], 2)
        truth = synthetic.stereo_correspondence(seq, f, f + 1, fr[f][0].uv[idx[:, 0]])
        dist = np.sqrt(((m - truth).reshape(-1, 4, 2) ** 2).sum(axis=-1)).max(axis=1)
        share = float((dist > 1.5).mean())
        print('{} x {} pair {}: {} matches, {:.1f} % beyond 1.5 px, median {:.2f} px'.format(
            shape[0], shape[1], f, m.shape[0], 100 * share, np.median(dist)))
        assert m.shape[0] >= 100
        assert share <= 0.2


def test_stereo_sequence_is_consistent_with_its_own_truth():
    """The right image of a frame is the left image's scene seen from `baseline` to the right: a left pixel and its true
    right position show the same texture cell (away from depth edges)."""
    seq = synthetic.stereo_sequence(60, 80, 2, seed=3, cell=0.3)
    assert seq['left'].dtype == np.uint8 and seq['left'].shape == (2, 60, 80) and seq['depth'].min() > 0
    uv = np.stack(np.meshgrid(np.arange(10, 70, 3), np.arange(10, 50, 3)), axis=-1).reshape(-1, 2)
    t = synthetic.stereo_correspondence(seq, 0, 1, uv)
    same = 0
    for row in t:
        u2, v2 = int(round(row[2])), int(round(row[3]))
        same += seq['left'][0][int(row[1]), int(row[0])] == seq['right'][0][v2, u2]
    assert same > 0.8 * len(t)
    assert np.all(t[:, 0] - t[:, 2] > 0)
