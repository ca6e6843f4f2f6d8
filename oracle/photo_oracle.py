"""CPU restatement of the reference's dense photometric alignment step
(pyslam/residuals/photometric_residual.py:38-161 inside pyslam/problem.py:182-194, 279-360).

TEST INFRASTRUCTURE ONLY: imported by tests/ as the checker,
never by the product path.  Works on plain tables (the constructor's outputs), one pixel per row, written
with explicit per-pixel formulas rather than the product class's stacked einsum expressions.
Pinned against tests/golden/photometric.npz, which oracle/gen_golden.py produced by running the reference
class and the reference Problem, and -- the image lookup on its own -- against tests/golden/bilinear.npz: outputs of the
reference's own kernel body with the four spellings that keep it from running repaired (x[1], y[1], out[1] -> [0],
np.int -> int; gen_golden.py: reference_bilinear_body, which the photometric case uses too).
"""
import numpy as np

from oracle import gn_oracle as orc


def tables(camera_params, im_ref, depth_ref, im_jac, min_grad, rgbd):
    """Constructor (:44-81): valid + strong-gradient pixels, triangulated points and d point / d depth."""
    cu, cv, fu, fv, b, w, h = camera_params
    w, h = int(w), int(h)
    u, v = np.meshgrid(np.arange(w, dtype=float), np.arange(h, dtype=float), indexing='xy')
    u, v, d = u.ravel(), v.ravel(), np.asarray(depth_ref, dtype=float).ravel()
    I = np.asarray(im_ref, dtype=float).ravel()
    g = np.stack([np.asarray(im_jac[0], dtype=float).ravel(), np.asarray(im_jac[1], dtype=float).ravel()], axis=1)
    with np.errstate(invalid='ignore'):
        keep = (d > 0) & (v > 0) & (v < h) & (u > 0) & (u < w)             # stereo_camera.py:93-97 / rgbd_camera.py:91-95
        if not rgbd:
            keep &= d < w
    keep &= np.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2) >= min_grad             # :72-76 (NaN depth fails `keep` already)
    u, v, d, I, g = u[keep], v[keep], d[keep], I[keep], g[keep]
    pt = np.empty((u.size, 3)); tj = np.empty((u.size, 3))
    if rgbd:                                                               # rgbd_camera.py:123-168
        pt[:, 0], pt[:, 1], pt[:, 2] = (u - cu) * d / fu, (v - cv) * d / fv, d
        tj[:, 0], tj[:, 1], tj[:, 2] = (u - cu) / fu, (v - cv) / fv, 1.
    else:                                                                  # stereo_camera.py:123-148
        bd = b / d
        pt[:, 0], pt[:, 1], pt[:, 2] = (u - cu) * bd, (v - cv) * bd * fu / fv, fu * bd
        tj[:, 0], tj[:, 1], tj[:, 2] = (cu - u) * bd / d, (cv - v) * bd / d * fu / fv, -fu * bd / d
    return dict(pt_ref=pt, im_ref=I, im_jac=g, tri_jac_d=tj, cam=(cu, cv, fu, fv, b), w=w, h=h, rgbd=bool(rgbd))


def bilinear(im, x, y):
    """utils.py:27-75 with [0] indices: weights from the unclipped corners, corners clamped afterwards."""
    h, w = im.shape
    out = np.empty(len(x))
    for i in range(len(x)):
        x0, y0 = int(x[i]), int(y[i])
        x1, y1 = x0 + 1, y0 + 1
        wa, wb = (x1 - x[i]) * (y1 - y[i]), (x1 - x[i]) * (y[i] - y0)
        wc, wd = (x[i] - x0) * (y1 - y[i]), (x[i] - x0) * (y[i] - y0)
        x0, x1 = min(max(x0, 0), w - 1), min(max(x1, 0), w - 1)
        y0, y1 = min(max(y0, 0), h - 1), min(max(y1, 0), h - 1)
        out[i] = wa * im[y0, x0] + wb * im[y1, x0] + wc * im[y0, x1] + wd * im[y1, x1]
    return out


def bilinear_vec(im, x, y):
    """bilinear() over whole arrays, with the same operations in the same order: truncated corners, weights from the
    unclipped corners, corners clamped afterwards, the four products summed left to right.  Equal to the loop bit for bit
    (tests/test_photo_oracle_host.py); fast enough for several 640 x 480 solves in one test run."""
    h, w = im.shape
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    x0, y0 = np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64)      # int(): truncation toward zero
    x1, y1 = x0 + 1, y0 + 1
    wa, wb = (x1 - x) * (y1 - y), (x1 - x) * (y - y0)
    wc, wd = (x - x0) * (y1 - y), (x - x0) * (y - y0)
    x0, x1 = np.clip(x0, 0, w - 1), np.clip(x1, 0, w - 1)
    y0, y1 = np.clip(y0, 0, h - 1), np.clip(y1, 0, h - 1)
    return wa * im[y0, x0] + wb * im[y1, x0] + wc * im[y0, x1] + wd * im[y1, x1]


def evaluate(tb, im_track, var_i, var_d, R, t):
    """evaluate() (:83-143): residual (valid pixels only), its N x 6 Jacobian ([translation | rotation]), valid mask."""
    cu, cv, fu, fv, b = tb['cam']
    p = tb['pt_ref'] @ R.T + t
    with np.errstate(divide='ignore', invalid='ignore'):
        iz = 1. / p[:, 2]
        u, v = fu * p[:, 0] * iz + cu, fv * p[:, 1] * iz + cv
        d = p[:, 2] if tb['rgbd'] else fu * b * iz
        valid = (d > 0) & (v > 0) & (v < tb['h']) & (u > 0) & (u < tb['w'])
        if not tb['rgbd']:
            valid &= d < tb['w']
    p, iz, u, v = p[valid], iz[valid], u[valid], v[valid]
    gu, gv = tb['im_jac'][valid, 0], tb['im_jac'][valid, 1]
    g = np.stack([gu * fu * iz, gv * fv * iz, -(gu * fu * p[:, 0] + gv * fv * p[:, 1]) * iz * iz], axis=1)   # :110-111
    jd = np.sum((g @ R) * tb['tri_jac_d'][valid], axis=1)                                                  # :112-116
    s = 1. / np.sqrt(var_i + var_d * jd ** 2)                                                              # :120-121
    r = s * (bilinear_vec(np.asarray(im_track, dtype=float), u, v) - tb['im_ref'][valid])
    J = np.empty((r.size, 6))
    J[:, :3] = g
    J[:, 3:] = np.cross(p, g)                                   # g (-p^) = p x g                          # :133-137
    return r, s[:, None] * J, valid


def normal_equations(tb, im_track, var_i, var_d, R, t, loss_id=0, loss_k=1.):
    """H = J~^T J~, b = -J~^T r~, cost = sum rho(r) with element-wise IRLS (problem.py:351-360, 329-335)."""
    r, J, valid = evaluate(tb, im_track, var_i, var_d, R, t)
    w = orc.loss_weight(loss_id, loss_k, r)
    H = (J * w[:, None]).T @ J
    return H, -(J * w[:, None]).T @ r, float(np.sum(orc.loss_rho(loss_id, loss_k, r))), int(valid.sum())


def gn_step(tb, im_track, var_i, var_d, R, t, loss_id=0, loss_k=1., split=False):
    """solve_one_iter + update: dx in [translation; rotation] order, the new (R, t), the linearisation cost."""
    H, b, cost, _ = normal_equations(tb, im_track, var_i, var_d, R, t, loss_id, loss_k)
    dx = np.linalg.solve(H, b)
    if split:                                                   # (SO3, translation) parameters: problem.py:405-409
        return dx, orc.so3_exp(dx[None, 3:])[0] @ R, t + dx[:3], cost
    Re, te = orc.se_exp(dx, 6)                                  # T <- exp(dx) T (liegroups perturb)
    return dx, Re[0] @ R, Re[0] @ t + te[0], cost


def normal_equations_ld(tb, im_track, var_i, var_d, R, t, loss_id=0, loss_k=1.):
    """normal_equations() accumulated in np.longdouble from the float64 per-pixel rows (r, J, w, rho of evaluate()), so the
    sums carry no float64 rounding of their own.  Also returns the element-wise magnitude sums that a tolerance is set from:
    abs_H = sum |w J_i J_j|, abs_b = sum |w J_i r|, abs_cost = sum |rho|, and min |r| (the L1 weight 1 / |r| is NaN at
    |r| <= 1e-8)."""
    r, J, valid = evaluate(tb, im_track, var_i, var_d, R, t)
    w = orc.loss_weight(loss_id, loss_k, r)
    rho = orc.loss_rho(loss_id, loss_k, r)
    L = np.longdouble
    Jl, rl = J.astype(L), r.astype(L)
    WJ = Jl * w.astype(L)[:, None]
    return dict(H=WJ.T @ Jl, b=-(WJ.T @ rl), cost=np.sum(rho.astype(L)), n=int(valid.sum()),
                abs_H=np.abs(WJ).T @ np.abs(Jl), abs_b=np.abs(WJ).T @ np.abs(rl), abs_cost=np.sum(np.abs(rho.astype(L))),
                min_abs_r=float(np.abs(r).min()) if r.size else np.inf)


def chol_solve_ld(H, b):
    """H x = b by a Cholesky factorisation in np.longdouble; None when H is not positive definite (a pivot that is not > 0,
    NaN included)."""
    n = len(b)
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        d = H[j, j] - np.sum(L[j, :j] * L[j, :j])
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (H[i, j] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
    y = np.zeros(n, dtype=np.longdouble)
    for i in range(n):
        y[i] = (b[i] - np.sum(L[i, :i] * y[:i])) / L[i, i]
    x = np.zeros(n, dtype=np.longdouble)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - np.sum(L[i + 1:, i] * x[i + 1:])) / L[i, i]
    return x


class DenseSolveError(RuntimeError):
    """The two failure exits of a level solve: fewer than 6 valid pixels, or H not positive definite."""


def dense_level_solve(tb, im_track, var_i, var_d, opt, loss_id, loss_k, rot_only, R, t):
    """One level of the dense pipeline's coarse-to-fine solve on the host: Problem.solve's loop (pyslam_amd/problem.py:
    _reference_loop) over the (R_1_0, t_1_0_1) parameters with longdouble normal equations.  rot_only: H[3:, 3:] dphi =
    b[3:], R <- exp(dphi) R, t unchanged; else dx = H^-1 b, R <- exp(dx[3:]) R, t += dx[:3].  Without a line search
    (opt.linesearch_max_iters == 0) an iteration reports the cost of its linearisation point, with one the cost after
    the step.  Raises DenseSolveError where the device reports a failure.

    -> dict(R, t, iters, hist (float64 costs), steps (dx per iteration), margins, restores (best-pose restores)): margins lists, for every stopping
    decision that compares a float with a threshold, its relative distance from the threshold -- cost / prev_cost against
    min_cost_decrease, |dx| against min_update_norm, cost against min_cost -- so a caller can show that no decision is a
    tie that a rounding difference could flip."""
    R, t = np.array(R, dtype=float), np.array(t, dtype=float)
    linesearch = opt.linesearch_max_iters > 0

    def ne(R, t):
        return normal_equations_ld(tb, im_track, var_i, var_d, R, t, loss_id, loss_k)

    cost = float(ne(R, t)['cost'])
    hist, steps, margins = [cost], [], []
    iters, nd, done, best, restores = 0, 0, False, None, 0
    while not done:
        iters += 1
        prev = cost
        q = ne(R, t)
        if q['n'] < 6:
            raise DenseSolveError('fewer than 6 valid pixels')
        o = 3 if rot_only else 0
        x = chol_solve_ld(q['H'][o:, o:], q['b'][o:])
        if x is None:
            raise DenseSolveError('not positive definite')
        dx = x.astype(float)
        steps.append(dx)
        dx_norm = float(np.sqrt(np.sum(x * x)))
        if rot_only:
            R = orc.so3_exp(dx[None])[0] @ R
        else:
            R, t = orc.so3_exp(dx[None, 3:])[0] @ R, t + dx[:3]
        cost = float(ne(R, t)['cost']) if linesearch else float(q['cost'])
        hist.append(cost)
        margins.append(abs(cost / prev - opt.min_cost_decrease) / opt.min_cost_decrease)
        if opt.min_update_norm > 0:
            margins.append(abs(dx_norm - opt.min_update_norm) / opt.min_update_norm)
        if opt.min_cost > 0:
            margins.append(abs(cost - opt.min_cost) / opt.min_cost)
        done = iters > opt.max_iters or dx_norm < opt.min_update_norm or cost < opt.min_cost
        if opt.allow_nondecreasing_steps:
            if nd == 0:
                best = (R.copy(), t.copy())
            nd = nd + 1 if cost >= opt.min_cost_decrease * prev else 0
            if nd >= opt.max_nondecreasing_steps:
                done = True
                R, t = best[0].copy(), best[1].copy()
                restores += 1
        else:
            done = done or cost >= opt.min_cost_decrease * prev
    return dict(R=R, t=t, iters=iters, hist=np.array(hist), steps=steps, margins=margins, restores=restores)


def dense_solve(levels, opt, loss_id, loss_k, R, t):
    """The coarse-to-fine sequence: `levels` is a list of dict(tb, im_track, var_i, var_d, rot_only), solved in order, each
    from the pose the previous one left.  -> dict(R, t, iters [per level], hists [per level], margins and restores [all levels])."""
    its, hists, margins, restores = [], [], [], 0
    for lv in levels:
        out = dense_level_solve(lv['tb'], lv['im_track'], lv['var_i'], lv['var_d'], opt, loss_id, loss_k, lv['rot_only'], R, t)
        R, t = out['R'], out['t']
        its.append(out['iters']); hists.append(out['hist']); margins += out['margins']; restores += out['restores']
    return dict(R=R, t=t, iters=its, hists=hists, margins=margins, restores=restores)


def dense_levels(im_ref, depth_ref, im_track, cam, levels, rot_only, var_i, var_d, min_grad):
    """Host inputs of dense_solve() for a frame pair, as the pipeline builds them: image pyramids by pyr_down on the raw
    (uint8 or float64) image, level images raw / 255, gradients 0.5 * Sobel, depth depth[::2^l, ::2^l], level cameras
    scaled by 2^-l with ceil'd sizes (pipelines/dense.py: _make_pyramid_cameras), tables(..., rgbd=True).
    cam = (cu, cv, fu, fv, w, h).  The two OpenCV operations come from pyslam_amd/pipelines/imgproc.py, the restatement
    the device pyramid is checked against bit for bit."""
    from pyslam_amd.pipelines import imgproc
    top = max(levels) + 1
    pyr_r, pyr_t = [np.asarray(im_ref)], [np.asarray(im_track)]
    for _ in range(1, top):
        pyr_r.append(imgproc.pyr_down(pyr_r[-1]))
        pyr_t.append(imgproc.pyr_down(pyr_t[-1]))
    out = []
    for l, ro in zip(levels, rot_only):
        s = 2. ** -l
        cu, cv, fu, fv, w, h = cam
        cl = (cu * s, cv * s, fu * s, fv * s, 0., int(np.ceil(w * s)), int(np.ceil(h * s)))
        ref = pyr_r[l].astype(float) / 255.
        jac = np.array([0.5 * imgproc.sobel(ref, 1, 0), 0.5 * imgproc.sobel(ref, 0, 1)])
        tb = tables(cl, ref, np.asarray(depth_ref, dtype=float)[::2 ** l, ::2 ** l], jac, min_grad, True)
        out.append(dict(tb=tb, im_track=pyr_t[l].astype(float) / 255., var_i=var_i, var_d=var_d, rot_only=bool(ro), level=l,
                        cam=cl, im_ref=ref, jac=jac))
    return out
