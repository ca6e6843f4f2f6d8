"""Randomised sweeps of the two small device paths behind SURVEY 8f ranks 3 and 4 against their oracles:
  * frame-to-frame RANSAC: random two-frame scenes, outlier fractions, point counts and sample draws (counts and winner exactly the
    oracle's outside the 1e-6 margin of the threshold; the shapes and edges one by one: tests/test_gpu_ransac_edges.py);
  * dense photometric alignment: random image sizes, cameras (stereo / RGB-D), poses, stiffnesses, gradient thresholds
    and losses -- normal equations and one Gauss-Newton step (both parameter forms).
usage: python tests/fuzz_small.py [cases] [seed0]"""
import os, sys, time
sys.path.insert(0, os.environ.get('GRAFT_REPO_ROOT', os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from oracle import photo_oracle as po
from oracle import ransac_oracle as ro
from pyslam_amd import synthetic, losses
from pyslam_amd.liegroups import SE3
from pyslam_amd.sensors import RGBDCamera, StereoCamera

LOSSES = [lambda: losses.L2Loss(), lambda: losses.HuberLoss(8.0), lambda: losses.CauchyLoss(5.0), lambda: losses.TukeyLoss(30.0),
          lambda: losses.TDistributionLoss(5.0)]


def ransac_case(rng, case):
    from pyslam_amd.pipelines.ransac import FrameToFrameRANSAC
    cam = StereoCamera(*synthetic.STEREO_BA_CAMERA)
    N = int(rng.integers(8, 900))
    T = SE3.exp(0.1 * rng.standard_normal(6) * np.array([3, 1, 3, 0.3, 0.3, 0.3]))
    pts = np.stack([rng.uniform(-6, 6, N), rng.uniform(-3, 3, N), rng.uniform(5, 30, N)], axis=1)
    obs_1 = cam.project(pts) + 0.2 * rng.standard_normal((N, 3))
    obs_2 = cam.project(T.dot(pts)) + 0.2 * rng.standard_normal((N, 3))
    bad = rng.choice(N, int(N * rng.uniform(0, 0.4)), replace=False)
    obs_2[bad, :2] += rng.uniform(20, 60, (bad.size, 2)) * rng.choice([-1., 1.], (bad.size, 2))
    r = FrameToFrameRANSAC(cam)
    r.set_obs(obs_1, obs_2)
    H = int(rng.choice([1, 17, 100, 400]))
    idx = rng.integers(0, N, size=(H, 3)).astype(np.int32)
    T_best, mask, best, count, T_all, counts = r._device_ransac(idx, want_all=True)
    cam5 = np.array(synthetic.STEREO_BA_CAMERA[:5], dtype=float)
    T_o, counts_o, best_o, mask_o = ro.perform_ransac(r.pts_1, r.pts_2, r.obs_2, idx, cam5, float(r.ransac_thresh))
    well = ro.sample_conditioning(r.pts_1, r.pts_2, idx) > 1e-3          # 3-point sets that determine the rotation
    e_T = np.abs(T_all[well] - T_o[well]).max() if well.any() else 0.
    # the margin rule (tests/test_gpu_twoview.py): a pair whose oracle squared error lies within 1e-6 relative of the threshold may
    # fall on either side; outside it the counts are the oracle's, and so is the winner whenever the oracle's maximum is unique
    thresh = float(r.ransac_thresh)
    err = ro.reprojection_errors(T_o, r.pts_1, r.obs_2, cam5)
    near, inl = np.abs(err - thresh) <= 1e-6 * thresh, err < thresh
    lo, hi = (inl & ~near).sum(axis=1), (inl | near).sum(axis=1)
    dc = int(((counts < lo) | (counts > hi))[well].sum())
    ok = e_T < 1e-8 and dc == 0
    top = int(np.argmax(lo))
    if ok and well.all() and (lo[top] > np.delete(hi, top).max() if H > 1 else True):
        ok = best == top and lo[top] <= count <= hi[top]
    return ok, 'ransac N %d H %d: |T - T_oracle| %.1e, counts off the oracle\'s %d, pairs in the margin %d' % (N, H, e_T, dc, near.sum())


def photo_case(rng, case):
    from pyslam_amd.device import PhotometricDevice
    from pyslam_amd.residuals import PhotometricResidualSE3
    rgbd = bool(rng.integers(2))
    h, w = int(rng.integers(12, 70)), int(rng.integers(16, 90))
    sc = synthetic.photometric_scene(h=h, w=w, seed=case, rgbd=rgbd, noise=float(rng.choice([0., 0.5, 3.0])),
                                     xi_true=tuple(0.02 * rng.standard_normal(6)))
    cu, cv, fu, fv, b, _, _ = sc['cam']
    cam = RGBDCamera(cu, cv, fu, fv, w, h) if rgbd else StereoCamera(cu, cv, fu, fv, b, w, h)
    cam.compute_pixel_grid()
    depth = sc['depth_ref'].copy()
    depth[rng.integers(h), rng.integers(w)] = np.nan
    si, sd, mg = float(rng.uniform(0.2, 3)), float(rng.uniform(0.2, 5)), float(rng.choice([0., 0.5, 3.]))
    blk = PhotometricResidualSE3(cam, sc['im_ref'], depth, sc['im_track'], sc['im_jac'], si, sd, min_grad=mg)
    tb = po.tables(sc['cam'], sc['im_ref'], depth, sc['im_jac'], mg, rgbd)
    if tb['pt_ref'].shape[0] < 30:
        return True, 'photo: too few pixels, skipped'
    loss = LOSSES[rng.integers(len(LOSSES))]()
    split = bool(rng.integers(2))
    dev = PhotometricDevice(blk, loss, split)
    T = SE3.exp(0.03 * rng.standard_normal(6))
    R, t = T.rot.as_matrix(), np.asarray(T.trans, dtype=float)
    dev.set_pose(R, t)
    Hd, bd, cd, nd = dev.normal_equations()
    Ho, bo, co, no = po.normal_equations(tb, sc['im_track'], si ** -2, sd ** -2, R, t, loss.LOSS_ID, getattr(loss, 'k', 1.0))
    e_H = np.linalg.norm(Hd - Ho) / np.linalg.norm(Ho)
    e_b = np.linalg.norm(bd - bo) / max(np.linalg.norm(bo), 1e-300)
    ok = dev.num_pixels == tb['pt_ref'].shape[0] and nd == no and e_H < 1e-11 and e_b < 1e-9 and abs(cd - co) <= 1e-11 * abs(co)
    msg = 'photo %dx%d %s %s split %d: pixels %d valid %d, H %.1e b %.1e' % (h, w, 'rgbd' if rgbd else 'stereo', type(loss).__name__, split,
                                                                            dev.num_pixels, nd, e_H, e_b)
    if ok and np.linalg.cond(Ho) < 1e10:
        dxo, Ro, to, _ = po.gn_step(tb, sc['im_track'], si ** -2, sd ** -2, R, t, loss.LOSS_ID, getattr(loss, 'k', 1.0), split=split)
        dx, _ = dev.step(False)
        Rn, tn = dev.get_pose()
        e_s = max(np.abs(Rn - Ro).max(), np.abs(tn - to).max())
        ok = e_s < 1e-8 * max(1., np.linalg.cond(Ho) * 1e-6)
        msg += ' step %.1e' % e_s
    dev.close()
    return ok, msg


def run(n_cases, seed0=0, verbose=True):
    bad = 0
    t0 = time.time()
    for case in range(seed0, seed0 + n_cases):
        rng = np.random.default_rng(77000 + case)
        try:
            ok, msg = (ransac_case if case % 2 else photo_case)(rng, case)
        except Exception as e:      # noqa: BLE001
            ok, msg = False, 'EXCEPTION %r' % (e,)
        bad += not ok
        if verbose and (not ok or case % 25 == 0):
            print('%s case %d %s' % ('ok  ' if ok else 'FAIL', case, msg), flush=True)
    if verbose:
        print('%d cases, %d failures, %.0f s' % (n_cases, bad, time.time() - t0))
    return bad


if __name__ == '__main__':
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else 60, int(sys.argv[2]) if len(sys.argv) > 2 else 0) else 0)
