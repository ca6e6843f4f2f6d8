"""The dense RGB-D VO kernels (csrc/ps_k_dense.h through csrc/ps_abi_dense.h and DenseTracker) against the host oracle
at 640 x 480 and above and at their edges: pyramids and gradients bit for bit against pipelines/imgproc.py, keyframe
tables against photo_oracle.tables() including the chunked scan (more than 1024 blocks), one Gauss-Newton step of
every loss against longdouble normal equations, the whole coarse-to-fine solve and its stopping rule against the host
restatement photo_oracle.dense_solve(), the failure exits, frames below the handle's capacity and determinism.

Every comparison is with the oracle, never with another device path."""
import collections

import numpy as np
import pytest

from oracle import gn_oracle as orc
from oracle import photo_oracle as po
from pyslam_amd.pipelines import imgproc

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
VAR = 100. ** -2                      # the pipeline's intensity and depth variances (stiffness 1 / 0.01)
Cam = collections.namedtuple('Cam', 'cu cv fu fv w h')
LOSSES = [(0, 0.), (1, 0.), (2, 5.), (3, 10.), (4, 20.), (5, 3.)]      # (device loss id, k): L2 L1 Cauchy Huber Tukey t
C_COST, C_STEP = 64, 4096             # the constants c of the c eps (magnitude sum) bounds (test_one_step_of_every_loss)


def _tracker(levels, h, w, slots=2):
    from pyslam_amd.device import DenseTracker
    return DenseTracker(levels, h, w, num_slots=slots)


def _loss(lid, k):
    from pyslam_amd import losses
    cls = {0: losses.L2Loss, 1: losses.L1Loss, 2: losses.CauchyLoss, 3: losses.HuberLoss, 4: losses.TukeyLoss,
           5: losses.TDistributionLoss}[lid]
    return cls() if lid in (0, 1) else cls(k)


def _options(**kw):
    from pyslam_amd.problem import Options
    o = Options()                                   # pipelines/dense.py: motion_options
    o.allow_nondecreasing_steps, o.max_nondecreasing_steps, o.min_cost_decrease = True, 5, 0.99
    o.max_iters, o.linesearch_max_iters = 30, 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _cams(cam, levels):
    return [Cam(cam[0] * 2. ** -l, cam[1] * 2. ** -l, cam[2] * 2. ** -l, cam[3] * 2. ** -l, int(np.ceil(cam[4] * 2. ** -l)),
                int(np.ceil(cam[5] * 2. ** -l))) for l in levels]


def _pose12(R, t):
    return np.concatenate([np.asarray(R, dtype=float).ravel(), np.asarray(t, dtype=float).ravel()])


def _xi_pose(xi):
    R, t = orc.se_exp(np.asarray(xi, dtype=float), 6)
    return R[0], t[0]


def _host_levels(ref, depth, trk, cam, levels, rot_only, min_grad=0.1):
    return po.dense_levels(ref, depth, trk, cam, levels, rot_only, VAR, VAR, min_grad)


def _host_pyramid(img, levels):
    raw = [img]
    for _ in range(1, levels):
        raw.append(imgproc.pyr_down(raw[-1]))
    return [r.astype(float) / 255. for r in raw]


def _assert_tables(dt, tb, what):
    """Same pixel count, same pixels in the same raster order (pt_ref carries u, v and z), the tables that use the host's
    arithmetic bit for bit, tri_jac_d within 2 ulps (the device multiplies by 1 / fu where the host divides by fu)."""
    n = tb['im_ref'].size
    assert dt['im_ref'].shape == (n,) and dt['pt_ref'].shape == (n, 3), (what, dt['im_ref'].shape, n)
    for k in ('pt_ref', 'im_ref', 'im_jac'):
        assert np.array_equal(dt[k], tb[k]), (what, k)
    assert np.all(np.abs(dt['tri_jac_d'] - tb['tri_jac_d']) <= 2 * EPS * np.abs(tb['tri_jac_d'])), what


@pytest.fixture(scope='module')
def vga():
    """640 x 480 keyframe (uint8 + depth with NaN and 0 holes), the next frame (uint8) and a float64 copy of it with
    sub-quantum dither (no residual is exactly 0 there, so the L1 weight 1 / |r| is finite), on one handle with tables for
    levels 0-3 at the pipeline's min_grad."""
    from pyslam_amd import synthetic
    seq = synthetic.rgbd_sequence(480, 640, 2, seed=1, hole_fraction=0.005)
    dither = seq['images'][1] + np.random.default_rng(5).uniform(-0.5, 0.5, seq['images'][1].shape)
    t = _tracker(4, 480, 640, slots=3)
    t.upload(0, seq['images'][0], seq['depth'][0])
    t.upload(1, seq['images'][1])
    t.upload(2, dither)
    t.make_tables(0, [0, 1, 2, 3], _cams(seq['cam'], range(4)), VAR, VAR, 0.1)
    host = {'u8': _host_levels(seq['images'][0], seq['depth'][0], seq['images'][1], seq['cam'], [0, 1, 2, 3], [False] * 4),
            'f64': _host_levels(seq['images'][0], seq['depth'][0], dither, seq['cam'], [0, 1, 2, 3], [False] * 4)}
    yield dict(t=t, seq=seq, dither=dither, host=host)
    t.close()


# ---------------------------------------------------------------- 1. pyramid, gradient and depth levels
def _edge_image(shape, dtype, seed):
    """Random content with horizontal and vertical runs of 0 and 255 (the clamp ends of the uint8 path)."""
    rng = np.random.default_rng(seed)
    h, w = shape
    img = rng.integers(0, 256, size=shape).astype(float) if dtype == np.uint8 else rng.random(shape) * 255.
    for _ in range(max(2, h * w // 400)):
        y, x, n = rng.integers(0, h), rng.integers(0, w), rng.integers(2, 12)
        v = rng.choice([0., 255.])
        if rng.random() < 0.5:
            img[y, x:x + n] = v
        else:
            img[y:y + n, x] = v
    return img.astype(dtype)


EDGE_SHAPES = [(63, 129), (64, 127), (65, 97), (31, 33), (94, 62)]     # level sizes 16k - 1, 16k, 16k + 1 (asserted)


def test_edge_shapes_cover_the_tile_edges():
    mods = {'h': set(), 'w': set()}
    for h, w in EDGE_SHAPES:
        for _ in range(1, 4):
            h, w = (h + 1) // 2, (w + 1) // 2
            mods['h'].add(h % 16 if h >= 15 else None)
            mods['w'].add(w % 16 if w >= 15 else None)
    assert {15, 0, 1} <= mods['h'] and {15, 0, 1} <= mods['w'], mods


@pytest.mark.parametrize('dtype', [np.uint8, np.float64], ids=['u8', 'f64'])
@pytest.mark.parametrize('shape,levels', [((480, 640), 4), ((481, 641), 4), ((2, 300), 8), ((300, 2), 8)] +
                         [(s, 4) for s in EDGE_SHAPES], ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_pyramid_gradient_and_depth_bit_identical(dtype, shape, levels):
    img = _edge_image(shape, dtype, seed=shape[0] * 7 + shape[1])
    rng = np.random.default_rng(shape[1])
    depth = rng.uniform(0.5, 8.0, shape)
    depth[rng.random(shape) < 0.05] = np.nan
    depth[rng.random(shape) < 0.05] = 0.
    depth[rng.random(shape) < 0.05] *= -1.
    t = _tracker(levels, *shape, slots=1)
    try:
        t.upload(0, img, depth)
        host = _host_pyramid(img, levels)
        if dtype == np.uint8 and shape[0] >= 480:        # sums that land exactly on the + 128 rounding of (sum + 128) >> 8
            assert np.sum(imgproc.pyr_down(img.astype(float)) % 1. == 0.5) > 100
        for l in range(levels):
            assert t.level_shape(l) == host[l].shape
            assert np.array_equal(t.read_level(0, l, 'image'), host[l]), l
            g = t.read_level(0, l, 'gradient')
            assert np.array_equal(g[0], 0.5 * imgproc.sobel(host[l], 1, 0)), l
            assert np.array_equal(g[1], 0.5 * imgproc.sobel(host[l], 0, 1)), l
            assert np.array_equal(t.read_level(0, l, 'depth'), depth[::2 ** l, ::2 ** l], equal_nan=True), l
        if levels == 8:
            assert min(host[7].shape) == 1 and min(host[1].shape) == 1        # deep levels one pixel high or wide
    finally:
        t.close()


# ---------------------------------------------------------------- 2. tables at VGA and above
def test_tables_every_level_of_vga(vga):
    assert -(-480 * 640 // 256) > 1024                   # level 0: 1200 blocks, two per thread of k_dense_scan
    for l, lv in enumerate(vga['host']['u8']):
        assert vga['t'].num_pixels(0, l) == lv['tb']['im_ref'].size > 1000
        _assert_tables(vga['t'].read_tables(0, l), lv['tb'], l)


def test_tables_720p_scan_four_blocks_per_thread():
    from pyslam_amd import synthetic
    seq = synthetic.rgbd_sequence(720, 1280, 1, seed=3, hole_fraction=0.005)
    nb = -(-720 * 1280 // 256)
    assert (nb + 1023) // 1024 == 4
    t = _tracker(1, 720, 1280, slots=1)
    try:
        t.upload(0, seq['images'][0], seq['depth'][0])
        t.make_tables(0, [0], _cams(seq['cam'], [0]), VAR, VAR, 0.1)
        tb = _host_levels(seq['images'][0], seq['depth'][0], seq['images'][0], seq['cam'], [0], [False])[0]['tb']
        assert t.num_pixels(0, 0) == tb['im_ref'].size > 50000
        _assert_tables(t.read_tables(0, 0), tb, '720p')
    finally:
        t.close()


def test_tables_empty_blocks_all_and_none(vga):
    """Whole 256-pixel blocks without survivors (a band without depth, a flat band), a level where every valid pixel
    survives (min_grad 0, depth everywhere: (h - 1)(w - 1) pixels, row 0 and column 0 are never valid) and one where none
    does (num_pixels 0, empty tables)."""
    seq = vga['seq']
    img, depth = seq['images'][0].copy(), seq['depth'][0].copy()
    depth[100:140] = np.nan                                # rows 100-139: blocks 250-349 lose every pixel
    img[300:340] = 77                                      # flat: no gradient inside the band
    t = _tracker(2, 480, 640, slots=1)
    try:
        t.upload(0, img, depth)
        t.make_tables(0, [0, 1], _cams(seq['cam'], [0, 1]), VAR, VAR, 0.1)
        for l, lv in enumerate(_host_levels(img, depth, img, seq['cam'], [0, 1], [False, False])):
            pt, (cu, cv, fu, fv, _, w, h) = lv['tb']['pt_ref'], lv['cam']
            rows = np.round(pt[:, 1] * fv / pt[:, 2] + cv).astype(int)
            cols = np.round(pt[:, 0] * fu / pt[:, 2] + cu).astype(int)
            flat = (301, 338) if l == 0 else (152, 167)      # rows whose 3 x 3 Sobel sees only the flat band
            assert not np.any((rows >= 100 >> l) & (rows < 140 >> l)) and not np.any((rows >= flat[0]) & (rows <= flat[1]))
            per_block = np.bincount((rows * w + cols) // 256, minlength=-(-w * h // 256))
            assert np.count_nonzero(per_block[np.argmax(per_block > 0):] == 0) >= (150 if l == 0 else 30)
            _assert_tables(t.read_tables(0, l), lv['tb'], ('bands', l))
        full = depth.copy()
        full[~(full > 0)] = 1.5
        t.upload(0, img, full)
        t.make_tables(0, [1], _cams(seq['cam'], [1]), VAR, VAR, 0.)
        lv = _host_levels(img, full, img, seq['cam'], [1], [False], min_grad=0.)[0]
        assert t.num_pixels(0, 1) == lv['tb']['im_ref'].size == 239 * 319
        _assert_tables(t.read_tables(0, 1), lv['tb'], 'all')
        t.make_tables(0, [0, 1], _cams(seq['cam'], [0, 1]), VAR, VAR, 1e9)
        for l in (0, 1):
            assert t.num_pixels(0, l) == 0
            dt = t.read_tables(0, l)
            assert dt['pt_ref'].shape == (0, 3) and dt['im_ref'].shape == (0,) and dt['im_jac'].shape == (0, 2)
    finally:
        t.close()


def test_tables_gradient_exactly_at_min_grad(vga):
    """min_grad equal to a gradient magnitude of the image, computed with the host's expression: the pixels exactly at
    the threshold are kept (|g| >= min_grad), as the host keeps them."""
    lv = vga['host']['u8'][0]
    gx, gy = lv['jac'][0], lv['jac'][1]
    mag = np.sqrt(gx ** 2 + gy ** 2)
    d = vga['seq']['depth'][0]
    valid = np.zeros(d.shape, bool)
    with np.errstate(invalid='ignore'):
        valid[1:, 1:] = d[1:, 1:] > 0
    m = np.sort(mag[valid])[np.count_nonzero(valid) // 2]
    at = np.count_nonzero(valid & (mag == m))
    assert at >= 1
    t = _tracker(1, 480, 640, slots=1)
    try:
        t.upload(0, vga['seq']['images'][0], d)
        t.make_tables(0, [0], _cams(vga['seq']['cam'], [0]), VAR, VAR, float(m))
        tb = _host_levels(vga['seq']['images'][0], d, vga['seq']['images'][0], vga['seq']['cam'], [0], [False], float(m))[0]['tb']
        assert tb['im_ref'].size == np.count_nonzero(valid & (mag >= m))
        assert t.num_pixels(0, 0) == tb['im_ref'].size
        _assert_tables(t.read_tables(0, 0), tb, 'threshold')
    finally:
        t.close()


# ---------------------------------------------------------------- 3. one step of every loss
XI0 = (0.01, -0.005, 0.02, 0.003, -0.002, 0.004)          # the perturbed start pose (translation, rotation)


@pytest.mark.parametrize('rot_only', [0, 1], ids=['6dof', 'rot'])
@pytest.mark.parametrize('level', [0, 2])
@pytest.mark.parametrize('loss', LOSSES, ids=lambda l: 'loss%d' % l[0])
def test_one_step_of_every_loss(vga, loss, level, rot_only, record_property):
    """track() with max_iters = 0 from a perturbed pose is one Gauss-Newton step: hist[0] is the cost-only pass, hist[1]
    the cost summed by the normal-equation pass, the pose change is the step.

    Bounds.  The longdouble oracle sums the float64 per-pixel rows with no rounding of its own; the device differs from it
    by (i) its float64 sums -- at most depth * eps * (magnitude sum) for a fixed summation tree of depth < 64 here (4
    pixels per thread, 6 wave levels, 4 waves, <= 38 partials per group, 8 groups) -- and (ii) the rounding of its own
    per-pixel rows (another operation order and FMA contraction in the projection and the Jacobian, which the weight and
    the image gradient amplify where |r| is small).  The cost rows are the same function of the same inputs on both sides
    (ps_loss_rho has contraction off), so only (i) bounds the cost:
        |cost_dev - cost| <= C_COST eps sum|rho|                                    C_COST = 64
    H and b carry (ii) as well; elementwise |dH| <= c eps sum|w J_i J_j|, |db| <= c eps sum|w J_i r| with c = C_STEP = 4096
    (about 1e-12 relative).  The step solves H dx = b; to first order dx_dev - dx = H^-1 (db - dH dx), so
        |dx_dev - dx| <= c eps (|sum|w J r|| + |sum|w J J||_F |dx|) / sigma_min(H)        (sigma_min = |H| / kappa(H))
    and recovering dx from the pose (so3_log(R1 R0^T), t1 - t0) adds a few eps (1 + |t|), covered by c eps (1 + |t|).
    Observed on an MI355X: cost at most 0.03 of its bound (1.9 eps sum|rho|), step at most 0.13 (L1, where the 1 / |r|
    weight amplifies (ii)), kappa(H) up to 4.7e3.  A dropped partial or a swapped rho / weight moves these by 1e-3 or more.

    The two cost passes sum in the same order and their cost rows are the same function of the same inputs (the two
    photo_eval instantiations compile r to the same instructions; ps_loss_rho has contraction off): hist[0] and hist[1] are equal
    bit for bit -- observed for every loss and level here, and asserted."""
    lid, k = loss
    t, seq = vga['t'], vga['seq']
    lv = vga['host']['f64'][level]
    R0, t0 = _xi_pose(XI0)
    opt = _options(max_iters=0)
    pose, its, hist = t.track(0, 2, [level], [rot_only], opt, _loss(lid, k), _pose12(R0, t0))
    q = po.normal_equations_ld(lv['tb'], lv['im_track'], VAR, VAR, R0, t0, lid, k)
    assert q['min_abs_r'] > 1e-8                         # no zero residual: the L1 weight is finite everywhere
    assert its == [1] and len(hist[0]) == 2
    allowed_c = C_COST * EPS * float(q['abs_cost'])
    err_c = max(abs(hist[0][0] - float(q['cost'])), abs(hist[0][1] - float(q['cost'])))
    assert err_c <= allowed_c, (err_c, allowed_c)
    record_property('cost_ratio', err_c / allowed_c)
    assert hist[0][0] == hist[0][1]
    o = 3 if rot_only else 0
    H, b = q['H'][o:, o:], q['b'][o:]
    dx = po.chol_solve_ld(H, b).astype(float)
    R1, t1 = pose[:9].reshape(3, 3), pose[9:]
    phi = orc.so3_log((R1 @ R0.T)[None])[0]
    dx_dev = phi if rot_only else np.concatenate([t1 - t0, phi])
    if rot_only:
        assert np.array_equal(t1, t0)
    sig_min = np.linalg.svd(H.astype(float), compute_uv=False)[-1]
    aH, ab = q['abs_H'][o:, o:].astype(float), q['abs_b'][o:].astype(float)
    allowed = C_STEP * EPS * ((np.linalg.norm(ab) + np.linalg.norm(aH) * np.linalg.norm(dx)) / sig_min + 1. + np.linalg.norm(t0))
    err = np.linalg.norm(dx_dev - dx)
    assert err <= allowed, (err, allowed, np.linalg.norm(dx))
    record_property('step_ratio', err / allowed)
    record_property('kappa', float(np.linalg.cond(H.astype(float))))


def test_l1_at_the_identity_pose(vga):
    """uint8 frames at the identity pose: some residuals are 0 (to within an ulp of the projection), so the L1 weight
    1 / |r| is NaN (losses.py: |r| <= 1e-8) and so is H.  The device reports 'not positive definite'; the host
    restatement fails at the same pivot test (what the reference would do -- spsolve on a NaN matrix -- returns NaN
    poses; the device's documented behaviour is an error, and that is what this pins)."""
    lv = vga['host']['u8'][2]
    q = po.normal_equations_ld(lv['tb'], lv['im_track'], VAR, VAR, np.eye(3), np.zeros(3), 1, 0.)
    assert q['min_abs_r'] <= 1e-8 and np.isnan(q['H'].astype(float)).any()
    with pytest.raises(po.DenseSolveError, match='not positive definite'):
        po.dense_solve([dict(lv, rot_only=False)], _options(max_iters=0), 1, 0., np.eye(3), np.zeros(3))
    with pytest.raises(RuntimeError, match='not positive definite'):
        vga['t'].track(0, 1, [2], [0], _options(max_iters=0), _loss(1, 0.), _pose12(np.eye(3), np.zeros(3)))


# ---------------------------------------------------------------- 4. the coarse-to-fine solve
def _compare_solve(t, host_levels, seq_levels, rot, opt, lid, k, R0, t0, ref=0, trk=1, margin=1e-6):
    lv = [dict(host_levels[l], rot_only=r) for l, r in zip(seq_levels, rot)]
    want = po.dense_solve(lv, opt, lid, k, R0, t0)
    pose, its, hist = t.track(ref, trk, seq_levels, rot, opt, _loss(lid, k), _pose12(R0, t0))
    assert min(want['margins'] or [np.inf]) > margin, min(want['margins'])       # no stopping decision is a tie
    assert its == want['iters'], (its, want['iters'])
    worst = 0.
    for h, w in zip(hist, want['hists']):
        worst = max(worst, float(np.max(np.abs(h - w) / np.abs(w))))
        assert np.allclose(h, w, rtol=1e-9, atol=0)
    perr = max(np.abs(pose[:9].reshape(3, 3) - want['R']).max(), np.abs(pose[9:] - want['t']).max())
    assert perr <= 1e-8, perr
    return want, pose, its, hist, worst, perr


@pytest.mark.parametrize('linesearch', [0, 10], ids=['nols', 'ls'])
@pytest.mark.parametrize('loss', [(3, 10.), (2, 5.)], ids=['huber', 'cauchy'])
def test_coarse_to_fine_solve_matches_the_host_restatement(vga, loss, linesearch, record_property):
    """The pipeline's default sequence [3, 2, 1, 0] (level 3 rotation-only) from the identity: iteration counts equal,
    cost histories to 1e-9 relative, pose to 1e-8, every stopping decision at least 1e-6 (relative) from its threshold."""
    want, pose, its, hist, worst, perr = _compare_solve(vga['t'], vga['host']['u8'], [3, 2, 1, 0], [1, 0, 0, 0],
                                                        _options(linesearch_max_iters=linesearch), *loss, np.eye(3), np.zeros(3))
    assert sum(its) >= 12
    record_property('hist_ratio', worst / 1e-9)
    record_property('pose_ratio', perr / 1e-8)
    record_property('min_margin', min(want['margins']))


# ---------------------------------------------------------------- 5. stopping-rule edges
@pytest.mark.parametrize('case', ['max_iters0', 'max_iters1', 'max_iters2', 'min_cost', 'min_update_norm', 'nd1', 'nd2',
                                  'pipeline_nd1', 'pipeline_max_iters0'])
def test_stopping_rule_edges(vga, case, record_property):
    host = vga['host']['u8']
    R0, t0 = _xi_pose(XI0)
    kw = {}
    if case == 'pipeline_nd1':    # the pipeline's options: best parameters kept and restored in the same (first) iteration
        kw = dict(max_nondecreasing_steps=1)
    elif case == 'pipeline_max_iters0':       # ... and the iteration limit ends it while the count of bad steps is running
        kw = dict(max_iters=0)
    elif case.startswith('max_iters'):
        kw = dict(max_iters=int(case[-1]), allow_nondecreasing_steps=False, min_cost_decrease=1.5)
    elif case == 'min_cost':
        c0 = float(po.normal_equations_ld(host[1]['tb'], host[1]['im_track'], VAR, VAR, R0, t0, 3, 10.)['cost'])
        kw = dict(min_cost=2. * c0)
    elif case == 'min_update_norm':
        first = po.dense_level_solve(host[1]['tb'], host[1]['im_track'], VAR, VAR, _options(max_iters=0), 3, 10., False, R0, t0)
        kw = dict(min_update_norm=2. * np.linalg.norm(first['steps'][0]))
    elif case == 'nd1':           # without a line search the first cost equals the start cost: nondecreasing at once
        kw = dict(max_nondecreasing_steps=1, min_cost_decrease=0.999)
    else:                         # two nondecreasing steps in a row late in the solve: back to the pose before them
        kw = dict(max_nondecreasing_steps=2, min_cost_decrease=0.95, linesearch_max_iters=10)
    opt = _options(**kw)
    want, pose, its, hist, worst, perr = _compare_solve(vga['t'], host, [1], [0], opt, 3, 10., R0, t0)
    if case.startswith('max_iters') or case == 'pipeline_max_iters0':
        assert its == [opt.max_iters + 1]
    elif case in ('min_cost', 'min_update_norm'):
        assert its == [1]
    else:
        assert want['restores'] == 1
    record_property('min_margin', min(want['margins']))


def test_growing_max_iters_reallocates_once(vga):
    """A longer history than any earlier call reallocates the history buffer once; the results are those of a fresh
    handle, bit for bit."""
    seq = vga['seq']
    R0, t0 = _xi_pose(XI0)

    def fresh(max_iters):
        f = _tracker(4, 480, 640)
        try:
            f.upload(0, seq['images'][0], seq['depth'][0])
            f.upload(1, seq['images'][1])
            f.make_tables(0, [2, 1], _cams(seq['cam'], [2, 1]), VAR, VAR, 0.1)
            return f.track(0, 1, [2, 1], [0, 0], _options(max_iters=max_iters), _loss(3, 10.), _pose12(R0, t0))
        finally:
            f.close()

    t = _tracker(4, 480, 640)
    try:
        t.upload(0, seq['images'][0], seq['depth'][0])
        t.upload(1, seq['images'][1])
        t.make_tables(0, [2, 1], _cams(seq['cam'], [2, 1]), VAR, VAR, 0.1)
        sizes = []
        for m in (2, 6, 6, 3):
            out = t.track(0, 1, [2, 1], [0, 0], _options(max_iters=m), _loss(3, 10.), _pose12(R0, t0))
            sizes.append(t.device_bytes())
            ref = fresh(m)
            assert np.array_equal(out[0], ref[0]) and out[1] == ref[1], m
            assert all(np.array_equal(a, b) for a, b in zip(out[2], ref[2])), m
        assert sizes[1] > sizes[0] and sizes[1] == sizes[2] == sizes[3], sizes
    finally:
        t.close()


# ---------------------------------------------------------------- 6. failure exits
def _good_pair():
    from pyslam_amd import synthetic
    seq = synthetic.rgbd_sequence(96, 128, 2, seed=8)
    return seq


def _track_good(t, seq):
    t.upload(0, seq['images'][0], seq['depth'][0])
    t.upload(1, seq['images'][1])
    t.make_tables(0, [2, 1, 0], _cams(seq['cam'], [2, 1, 0]), VAR, VAR, 0.1)
    return t.track(0, 1, [2, 1, 0], [1, 0, 0], _options(), _loss(3, 10.), _pose12(np.eye(3), np.zeros(3)))


def test_device_bytes_follow_the_history_buffer_exactly():
    """The history buffer is the handle's only allocation after create: 8 levels x (2 + max_iters + 2) doubles.  max_iters 2,
    then 6, then 3: the count grows by 8 x (6 - 2) x 8 = 256 bytes at the second call -- the old block's bytes come off as they
    went on -- and stays at the third."""
    seq = _good_pair()
    t = _tracker(2, 96, 128)
    try:
        t.upload(0, seq['images'][0], seq['depth'][0])
        t.upload(1, seq['images'][1])
        t.make_tables(0, [1, 0], _cams(seq['cam'], [1, 0]), VAR, VAR, 0.1)
        sizes = []
        for m in (2, 6, 3):
            t.track(0, 1, [1, 0], [0, 0], _options(max_iters=m), _loss(3, 10.), _pose12(np.eye(3), np.zeros(3)))
            sizes.append(t.device_bytes())
        print('device bytes after max_iters 2, 6, 3:', sizes)
        assert sizes[1] - sizes[0] == 8 * (6 - 2) * 8 and sizes[2] == sizes[1], sizes
    finally:
        t.close()


def _assert_same(a, b):
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))


def test_failure_exits_and_reuse():
    """Fewer than 6 valid pixels (0 and exactly 5 table pixels) and H not positive definite (an image that varies along u
    only: gy = 0, J[1] = 0, H[1][1] = 0 exactly, on a 6-DOF level).  The reference would carry on with NaN poses (spsolve
    on a singular matrix); the device's documented behaviour is an error, which the host restatement shares.  After each
    error the same handle tracks a good pair exactly as a fresh handle does."""
    seq = _good_pair()
    f = _tracker(3, 96, 128)
    try:
        want = _track_good(f, seq)
    finally:
        f.close()
    t = _tracker(3, 96, 128)
    try:
        # 0 pixels
        t.upload(0, seq['images'][0], seq['depth'][0])
        t.upload(1, seq['images'][1])
        t.make_tables(0, [0], _cams(seq['cam'], [0]), VAR, VAR, 1e9)
        assert t.num_pixels(0, 0) == 0
        with pytest.raises(RuntimeError, match='fewer than 6 valid pixels'):
            t.track(0, 1, [0], [0], _options(), _loss(3, 10.), _pose12(np.eye(3), np.zeros(3)))
        _assert_same(_track_good(t, seq), want)
        # exactly 5 pixels: min_grad at the 5th largest magnitude of the valid pixels
        lv = _host_levels(seq['images'][0], seq['depth'][0], seq['images'][1], seq['cam'], [0], [False], 0.)[0]
        mags = np.sort(np.sqrt(lv['tb']['im_jac'][:, 0] ** 2 + lv['tb']['im_jac'][:, 1] ** 2))[::-1]
        assert mags[4] > mags[5]
        t.make_tables(0, [0], _cams(seq['cam'], [0]), VAR, VAR, float(mags[4]))
        assert t.num_pixels(0, 0) == 5
        with pytest.raises(RuntimeError, match='fewer than 6 valid pixels'):
            t.track(0, 1, [0], [0], _options(), _loss(3, 10.), _pose12(np.eye(3), np.zeros(3)))
        with pytest.raises(po.DenseSolveError, match='fewer than 6'):
            po.dense_solve([_host_levels(seq['images'][0], seq['depth'][0], seq['images'][1], seq['cam'], [0], [False],
                                         float(mags[4]))[0]], _options(), 3, 10., np.eye(3), np.zeros(3))
        _assert_same(_track_good(t, seq), want)
        # H not positive definite
        u = np.arange(128, dtype=float)
        img = np.tile(np.round(128 + 100 * np.sin(u / 5.)), (96, 1)).astype(np.uint8)
        trk = np.tile(np.round(128 + 100 * np.sin((u + 0.7) / 5.)), (96, 1)).astype(np.uint8)
        depth = np.full((96, 128), 2.0)
        t.upload(0, img, depth)
        t.upload(1, trk)
        t.make_tables(0, [0], _cams(seq['cam'], [0]), VAR, VAR, 0.1)
        hl = _host_levels(img, depth, trk, seq['cam'], [0], [False])
        assert t.num_pixels(0, 0) == hl[0]['tb']['im_ref'].size > 1000 and np.all(hl[0]['tb']['im_jac'][:, 1] == 0)
        with pytest.raises(po.DenseSolveError, match='not positive definite'):
            po.dense_solve(hl, _options(), 3, 10., np.eye(3), np.zeros(3))
        with pytest.raises(RuntimeError, match='not positive definite'):
            t.track(0, 1, [0], [0], _options(), _loss(3, 10.), _pose12(np.eye(3), np.zeros(3)))
        _assert_same(_track_good(t, seq), want)
    finally:
        t.close()


# ---------------------------------------------------------------- 7. capacity and determinism
def test_frames_below_capacity_match_a_handle_of_their_size():
    from pyslam_amd import synthetic
    seq = synthetic.rgbd_sequence(97, 131, 2, seed=4)
    outs = []
    for cap in ((97, 131), (480, 640)):
        t = _tracker(4, *cap)
        try:
            t.upload(0, seq['images'][0], seq['depth'][0])
            t.upload(1, seq['images'][1])
            t.make_tables(0, [3, 2, 1, 0], _cams(seq['cam'], [3, 2, 1, 0]), VAR, VAR, 0.1)
            lv = [(t.level_shape(l), t.read_level(0, l, 'image'), t.read_level(0, l, 'gradient'), t.read_level(1, l, 'image'),
                   t.read_tables(0, l)) for l in range(4)]
            out = t.track(0, 1, [3, 2, 1, 0], [1, 0, 0, 0], _options(), _loss(3, 10.), _pose12(np.eye(3), np.zeros(3)))
            outs.append((lv, out))
            if cap == (480, 640):       # every slot of a handle holds frames of one size
                with pytest.raises(RuntimeError, match='same size'):
                    t.upload(1, np.zeros((96, 131), np.uint8))
        finally:
            t.close()
    (a, oa), (b, ob) = outs
    for l in range(4):
        assert a[l][0] == b[l][0]
        for k in (1, 2, 3):
            assert np.array_equal(a[l][k], b[l][k]), (l, k)
        for key in a[l][4]:
            assert np.array_equal(a[l][4][key], b[l][4][key]), (l, key)
    _assert_same(oa, ob)


def test_two_live_handles_bitwise_equal(vga):
    seq = vga['seq']
    u = _tracker(4, 480, 640)
    try:
        u.upload(0, seq['images'][0], seq['depth'][0])
        u.upload(1, seq['images'][1])
        u.make_tables(0, [0, 1, 2, 3], _cams(seq['cam'], range(4)), VAR, VAR, 0.1)
        args = ([3, 2, 1, 0], [1, 0, 0, 0], _options(), _loss(3, 10.), _pose12(np.eye(3), np.zeros(3)))
        _assert_same(vga['t'].track(0, 1, *args), u.track(0, 1, *args))
    finally:
        u.close()
