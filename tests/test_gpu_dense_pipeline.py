"""Dense RGB-D VO pipeline on the MI355X: device pyramids and gradients bit-identical to imgproc, device keyframe tables
identical to PhotometricResidualSE3's, the rotation-only solve against the host block protocol, the whole pipeline
against the verbatim reference (tests/golden/dense_rgbd.npz), determinism, bounded device memory and tracking accuracy
at 640 x 480."""
import os

import numpy as np
import pytest

from pyslam_amd.pipelines import imgproc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'dense_rgbd.npz')


def _tracker(levels, h, w, slots=2):
    from pyslam_amd.device import DenseTracker
    return DenseTracker(levels, h, w, num_slots=slots)


def _host_pyramid(img, levels):
    raw = [img]
    for _ in range(1, levels):
        raw.append(imgproc.pyr_down(raw[-1]))
    return [r.astype(float) / 255. for r in raw]


@pytest.mark.parametrize('dtype', [np.uint8, np.float64])
@pytest.mark.parametrize('shape', [(97, 131), (64, 80), (35, 18)])
def test_pyramid_and_gradient_bit_identical(dtype, shape):
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, size=shape).astype(np.uint8) if dtype == np.uint8 else rng.random(shape) * 255.
    levels = 4
    t = _tracker(levels, *shape, slots=1)
    try:
        t.upload(0, img)
        host = _host_pyramid(img, levels)
        for l in range(levels):
            dev = t.read_level(0, l, 'image')
            assert dev.shape == host[l].shape
            assert np.array_equal(dev, host[l]), (l, np.abs(dev - host[l]).max())
            g = t.read_level(0, l, 'gradient')
            assert np.array_equal(g[0], 0.5 * imgproc.sobel(host[l], 1, 0)), l
            assert np.array_equal(g[1], 0.5 * imgproc.sobel(host[l], 0, 1)), l
    finally:
        t.close()


def _level_camera(cam, l):
    from pyslam.sensors import RGBDCamera
    s = 2. ** -l
    c = RGBDCamera(cam[0] * s, cam[1] * s, cam[2] * s, cam[3] * s, int(np.ceil(cam[4] * s)), int(np.ceil(cam[5] * s)))
    c.compute_pixel_grid()
    return c


def test_tables_match_host_residual():
    from pyslam_amd import synthetic
    from pyslam_amd.residuals import PhotometricResidualSE3
    seq = synthetic.rgbd_sequence(97, 131, 2, seed=4)
    img, depth = seq['images'][0], seq['depth'][0]
    levels = 4
    t = _tracker(levels, *img.shape, slots=1)
    try:
        t.upload(0, img, depth)
        cams = [_level_camera(seq['cam'], l) for l in range(levels)]
        t.make_tables(0, list(range(levels)), cams, 100. ** -2, 100. ** -2, 0.1)
        host_im = _host_pyramid(img, levels)
        d = depth
        for l in range(levels):
            if l:
                d = d[0::2, 0::2]
            assert np.array_equal(t.read_level(0, l, 'depth'), d, equal_nan=True)
            jac = np.array([0.5 * imgproc.sobel(host_im[l], 1, 0), 0.5 * imgproc.sobel(host_im[l], 0, 1)])
            res = PhotometricResidualSE3(cams[l], host_im[l], d, host_im[l], jac, 100., 100., 0.1)
            ht = res.device_tables()
            dt = t.read_tables(0, l)
            assert dt['im_ref'].shape[0] == ht['im_ref'].shape[0] > 0, l
            assert np.array_equal(dt['im_ref'], ht['im_ref']), l           # same pixels in the same (raster) order
            for k in ('pt_ref', 'im_jac', 'tri_jac_d'):
                assert np.allclose(dt[k], ht[k], rtol=1e-14, atol=0), (l, k)
    finally:
        t.close()


def _options():
    from pyslam_amd.problem import Options
    o = Options()
    o.allow_nondecreasing_steps = True
    o.max_nondecreasing_steps = 5
    o.min_cost_decrease = 0.99
    o.max_iters = 30
    o.linesearch_max_iters = 0
    return o


@pytest.mark.parametrize('linesearch', [False, True])
def test_rotation_only_level_matches_host_block_protocol(linesearch):
    from pyslam_amd import synthetic
    from pyslam_amd.liegroups import SE3, SO3
    from pyslam_amd.losses import HuberLoss
    from pyslam_amd.problem import Problem
    from pyslam_amd.residuals import PhotometricResidualSE3
    seq = synthetic.rgbd_sequence(96, 128, 3, seed=2)
    levels, lvl = 4, 2
    t = _tracker(levels, 96, 128)
    try:
        t.upload(0, seq['images'][0], seq['depth'][0])
        t.upload(1, seq['images'][2])
        cam = _level_camera(seq['cam'], lvl)
        t.make_tables(0, [lvl], [cam], 100. ** -2, 100. ** -2, 0.1)
        opt = _options()
        opt.linesearch_max_iters = 10 if linesearch else 0
        guess = SE3.identity()
        pose0 = np.concatenate([guess.rot.as_matrix().ravel(), guess.trans])
        pose, its, hists = t.track(0, 1, [lvl], [True], opt, HuberLoss(10.0), pose0)

        ref_im = _host_pyramid(seq['images'][0], levels)[lvl]
        trk_im = _host_pyramid(seq['images'][2], levels)[lvl]
        depth = seq['depth'][0][0::4, 0::4]
        jac = np.array([0.5 * imgproc.sobel(ref_im, 1, 0), 0.5 * imgproc.sobel(ref_im, 0, 1)])
        res = PhotometricResidualSE3(cam, ref_im, depth, trk_im, jac, 100., 100., 0.1)
        prob = Problem(opt)
        prob.add_residual_block(res, ['R_1_0', 't_1_0_1'], loss=HuberLoss(10.0))
        prob.initialize_params({'R_1_0': SO3.identity(), 't_1_0_1': np.zeros(3)})
        prob.set_parameters_constant('t_1_0_1')
        params = prob.solve()
        hist = np.array(prob._cost_history)
        assert its[0] == len(hist) - 1 and its[0] >= 2
        assert np.allclose(hists[0], hist, rtol=1e-9, atol=0)
        assert np.allclose(pose[:9].reshape(3, 3), params['R_1_0'].as_matrix(), rtol=0, atol=1e-9)
        assert np.array_equal(pose[9:], np.zeros(3))
    finally:
        t.close()


def _run_golden_pipeline(g, capsys=None):
    from pyslam.pipelines import DenseRGBDPipeline
    from pyslam.sensors import RGBDCamera
    from pyslam_amd.liegroups import SE3
    cu, cv, fu, fv, w, h = g['cam']
    cam = RGBDCamera(cu, cv, fu, fv, w, h)
    cam.compute_pixel_grid()
    p = DenseRGBDPipeline(cam, SE3.from_matrix(g['T_true'][0]))
    p.keyframe_trans_thresh, p.keyframe_rot_thresh = float(g['trans_thresh']), float(g['rot_thresh'])
    imgs = [g['images'][f] for f in range(g['images'].shape[0])]
    out = []
    for f, m in zip(g['frame_idx'], g['mode']):
        if m == 'track' and p.mode != 'track':
            p.set_mode('track')
        p.track(imgs[f], g['depth'][f])
        printed = capsys.readouterr().out if capsys is not None else None
        out.append(dict(T=p.T_c_w[-1].as_matrix() if p.T_c_w else None, active=p.active_keyframe_idx,
                        nkf=len(p.keyframes), its=list(p.last_iterations) if len(p.keyframes) and (len(out) > 0) else [],
                        hists=[h.copy() for h in p.last_cost_histories] if len(out) > 0 else [], printed=printed))
    kf_frames = [next(f for f in range(len(imgs)) if kf.data[0] is imgs[f]) for kf in p.keyframes]
    return p, out, kf_frames


def test_pipeline_matches_reference(capsys):
    g = np.load(GOLDEN)
    p, out, kf_frames = _run_golden_pipeline(g, capsys)
    assert kf_frames == list(g['keyframe_frames'])
    offs = np.concatenate([[0], np.cumsum(g['hist_len'])])
    h = 0
    nlev = len(g['default_pyrlevel_sequence'])
    for k, o in enumerate(out):
        assert o['printed'] == str(g['printed'][k]), k
        assert o['active'] == int(g['active_idx'][k]) and o['nkf'] == int(g['num_keyframes'][k]), k
        if g['iterations'][k][0] < 0:                 # the first frame: nothing tracked
            continue
        assert np.allclose(o['T'], g['T_c_w'][k], rtol=0, atol=1e-8), (k, np.abs(o['T'] - g['T_c_w'][k]).max())
        assert o['its'] == list(g['iterations'][k]), k
        for l in range(nlev):
            ref = g['hist_flat'][offs[h]:offs[h + 1]]
            h += 1
            assert np.allclose(o['hists'][l], ref, rtol=1e-9, atol=0), (k, l)
    assert h == len(g['hist_len'])


def test_pipeline_deterministic_and_two_live():
    g = np.load(GOLDEN)
    p1, out1, _ = _run_golden_pipeline(g)
    p2, out2, _ = _run_golden_pipeline(g)                 # p1 is still alive: two pipelines on one device
    for a, b in zip(out1, out2):
        if a['T'] is not None:
            assert np.array_equal(a['T'], b['T'])
    # keyframe attributes read back from the device with the reference's shapes
    kf = p1.keyframes[-1]
    assert [im.shape for im in kf.im_pyr] == [(96, 128), (48, 64), (24, 32), (12, 16)]
    assert [j.shape for j in kf.jacobian] == [(2, 96, 128), (2, 48, 64), (2, 24, 32), (2, 12, 16)]
    assert np.array_equal(kf.depth[1], kf.data[1][0::2, 0::2], equal_nan=True)
    assert np.array_equal(kf.im_pyr[2], _host_pyramid(kf.data[0], 4)[2])


def test_device_memory_bounded():
    from pyslam.pipelines import DenseRGBDPipeline
    from pyslam.sensors import RGBDCamera
    from pyslam_amd import synthetic
    seq = synthetic.rgbd_sequence(48, 64, 12, seed=5)
    cu, cv, fu, fv, w, h = seq['cam']
    cam = RGBDCamera(cu, cv, fu, fv, w, h)
    cam.compute_pixel_grid()
    p = DenseRGBDPipeline(cam)
    p.pyrlevels = 3
    p.pyrlevel_sequence = [2, 1, 0]
    p._make_pyramid_cameras()
    p.keyframe_trans_thresh, p.keyframe_rot_thresh = 0., 0.        # every frame becomes a keyframe
    sizes = []
    for f in range(12):
        p.track(seq['images'][f], seq['depth'][f])
        if len(p.keyframes) >= 2:
            sizes.append(p._frames.tracker.device_bytes())
    assert len(p.keyframes) >= 11
    assert len(set(sizes)) == 1, sizes


def test_tracking_accuracy_vga():
    from pyslam.pipelines import DenseRGBDPipeline
    from pyslam.sensors import RGBDCamera
    from pyslam_amd import synthetic
    from pyslam_amd.liegroups import SE3
    seq = synthetic.rgbd_sequence(480, 640, 4, seed=1, hole_fraction=0.005)
    cu, cv, fu, fv, w, h = seq['cam']
    cam = RGBDCamera(cu, cv, fu, fv, w, h)
    cam.compute_pixel_grid()
    p = DenseRGBDPipeline(cam, SE3.from_matrix(seq['T_c_w'][0]))
    for f in range(4):
        p.track(seq['images'][f], seq['depth'][f])
    assert len(p.keyframes) == 1
    for f in range(1, 4):
        T_true = SE3.from_matrix(seq['T_c_w'][f]).dot(SE3.from_matrix(seq['T_c_w'][0]).inv())
        T_est = p.T_c_w[f].dot(SE3.from_matrix(seq['T_c_w'][0]).inv())
        err = T_true.dot(T_est.inv()).log()
        # interpolation-limited, as test_photometric.py accepts for the exactly rendered plane (uint8 quantisation here)
        assert np.linalg.norm(err[:3]) < 5e-3 and np.linalg.norm(err[3:]) < 2e-3, (f, err)
