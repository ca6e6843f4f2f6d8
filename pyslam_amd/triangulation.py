"""Host restatement (numpy) of the device's multi-view triangulation (csrc/ps_k_triang.h, ps_triangulate): the same
definition, the same observation order and the same order of every sum, so the two agree to rounding.

Per variable landmark, from its observations and the poses of the tables (constant poses included):

1. Linear start.  With x_n = (u - cu) / fu, y_n = (v - cv) / fv and the observing pose (R | t), rows r1 r2 r3, every
   observation gives the rows (x_n r3 - r1) p = -(x_n t3 - t1) and (y_n r3 - r2) p = -(y_n t3 - t2); an observation that
   bears depth (stereo: z = fu b / d, RGB-D: z = d) a third, r3 p = z - t3.  The 3 x 3 normal equations are solved by
   Cholesky.
2. ``refine_iters`` Gauss-Newton steps on the landmark's own robust reprojection cost with every pose held: r = S (project
   (R p + t) - obs), IRLS-scaled as the solver scales it, H = sum J~^T J~, g = sum J~^T r~, H dx = -g by Cholesky.  A step that
   does not lower the cost is not taken and ends that landmark's iteration.  So does a step whose 3 x 3 system cannot be
   solved (a pivot that is not positive, NaN): under L1 the IRLS weight of a residual component within 1e-8 of zero is NaN
   (the reference's losses.py), and that is where a landmark with an L1 observation converges to.  The landmark keeps its
   last accepted point and its status.
3. Status: 0 ok; 1 fewer than two observations and none bearing depth; 2 no depth and the largest angle between two viewing
   rays below ``min_parallax_deg``, or a linear start whose normal equations are not positive definite; 3 the result lies
   behind one of its cameras.  A landmark with a non-zero status keeps its old value.

Order: a landmark's observations in the order of the observation table (the device's landmark sort is stable); observation
q of a landmark goes to lane q mod 16, a lane adds its observations in order, and the 16 lane sums are added in the
order of the device's row reduction (group16_sum: shifts by 1, 2, 4, 8).
"""
import numpy as np

from pyslam_amd import losses as _losses

OK, FEW_OBS, DEGENERATE, BEHIND = 0, 1, 2, 3
_LOSSES = [_losses.L2Loss, _losses.L1Loss, _losses.CauchyLoss, _losses.HuberLoss, _losses.TukeyLoss, _losses.TDistributionLoss]


def _group16_sum(lanes):
    """(..., 16) lane values -> the total in the device's association order (csrc/ps_k_linearize.h: group16_sum)."""
    v = np.array(lanes, dtype=np.float64)
    for sh, first in ((1, 1), (2, 2), (4, 4), (8, 8)):
        w = v.copy()
        w[..., first:] = v[..., first:] + v[..., :16 - sh][..., first - sh:]
        v = w
    return v[..., 15]


def _chol_solve(A, rhs):
    """x = A^-1 rhs for stacks of symmetric 3 x 3 (a00, a10, a11, a20, a21, a22); ok False where a pivot is not positive."""
    with np.errstate(all='ignore'):
        ok = A[:, 0] > 0.
        l00 = np.sqrt(np.where(ok, A[:, 0], 1.))
        l10, l20 = A[:, 1] / l00, A[:, 3] / l00
        d1 = A[:, 2] - l10 * l10
        ok &= d1 > 0.
        l11 = np.sqrt(np.where(ok, d1, 1.))
        l21 = (A[:, 4] - l20 * l10) / l11
        d2 = A[:, 5] - l20 * l20 - l21 * l21
        ok &= d2 > 0.
        l22 = np.sqrt(np.where(ok, d2, 1.))
        y0 = rhs[:, 0] / l00
        y1 = (rhs[:, 1] - l10 * y0) / l11
        y2 = (rhs[:, 2] - l20 * y0 - l21 * y1) / l22
        x2 = y2 / l22
        x1 = (y1 - l21 * x2) / l11
        x0 = (y0 - l10 * x1 - l20 * x2) / l00
    return np.stack([x0, x1, x2], axis=1), ok


def _outer6(a):
    return np.stack([a[:, 0] * a[:, 0], a[:, 1] * a[:, 0], a[:, 1] * a[:, 1],
                     a[:, 2] * a[:, 0], a[:, 2] * a[:, 1], a[:, 2] * a[:, 2]], axis=1)


class _Tracks:
    """The observations of the selected variable landmarks as padded (n, maxlen) index tables, in table order."""

    def __init__(self, lp, vids):
        var_pts = np.nonzero(lp.point_vid >= 0)[0]
        point_of_vid = np.empty(var_pts.size, dtype=np.int64)
        point_of_vid[lp.point_vid[var_pts]] = var_pts
        self.points = point_of_vid[vids]
        order = np.argsort(lp.obs_point, kind='stable')
        cnt = np.bincount(lp.obs_point, minlength=lp.num_points)
        start = np.concatenate([[0], np.cumsum(cnt)])
        self.len = cnt[self.points]
        self.maxlen = int(self.len.max()) if self.len.size else 0
        q = np.arange(self.maxlen)[None, :]
        self.valid = q < self.len[:, None]
        idx = np.minimum(start[self.points][:, None] + q, max(order.size - 1, 0))
        self.obs = order[idx] if order.size else np.zeros_like(idx)


def _weights(lp, grp, r):
    """sqrt of the IRLS weight of every residual component, by the group's loss (csrc/ps_math.h: ps_loss_sqrt_weight)."""
    s = np.ones_like(r)
    rho = np.zeros_like(r)
    for g in np.unique(grp):
        loss = _LOSSES[int(lp.obs_groups[g, 2])]
        loss = loss() if int(lp.obs_groups[g, 2]) < 2 else loss(lp.obs_groups[g, 3])
        m = grp == g
        with np.errstate(all='ignore'):
            s[m] = np.sqrt(np.asarray(loss.weight(r[m].ravel()), dtype=float)).reshape(r[m].shape)
        rho[m] = np.asarray(loss.loss(r[m].ravel()), dtype=float).reshape(r[m].shape)
    return s, rho


def _evaluate(lp, tr, p):
    """Cost, H (6), g (3) and the count of observations with z <= 0 of every selected landmark at the points p (n, 3)."""
    n = p.shape[0]
    lanes = np.zeros((11, n, 16))
    for q in range(tr.maxlen):
        m = tr.valid[:, q]
        o = tr.obs[m, q]
        grp = lp.obs_grp[o]
        G = lp.obs_groups[grp]
        cam = lp.cams[G[:, 0].astype(int)]
        S = lp.stiff3[G[:, 1].astype(int)].reshape(-1, 3, 3)
        T = lp.poses[lp.obs_pose[o]]
        R, t = T[:, :9].reshape(-1, 3, 3), T[:, 9:]
        pc = np.einsum('nij,nj->ni', R, p[m]) + t
        with np.errstate(all='ignore'):
            iz = 1. / pc[:, 2]
            mono, rgbd = cam[:, 4] == -2., cam[:, 4] == -1.
            uvd = lp.obs_uvd[o]
            e = np.stack([cam[:, 2] * pc[:, 0] * iz + cam[:, 0] - uvd[:, 0], cam[:, 3] * pc[:, 1] * iz + cam[:, 1] - uvd[:, 1],
                          np.where(mono, 0., np.where(rgbd, pc[:, 2] - uvd[:, 2], cam[:, 2] * np.where(mono | rgbd, 0., cam[:, 4]) * iz - uvd[:, 2]))],
                         axis=1)
            Jc = np.zeros((o.size, 3, 3))
            Jc[:, 0, 0] = cam[:, 2] * iz
            Jc[:, 0, 2] = -cam[:, 2] * pc[:, 0] * iz * iz
            Jc[:, 1, 1] = cam[:, 3] * iz
            Jc[:, 1, 2] = -cam[:, 3] * pc[:, 1] * iz * iz
            Jc[:, 2, 2] = np.where(mono, 0., np.where(rgbd, 1., -cam[:, 2] * np.where(mono | rgbd, 0., cam[:, 4]) * iz * iz))
            r = np.einsum('nij,nj->ni', S, e)
            s, rho = _weights(lp, grp, r)
            s[mono, 2] = 1.                                   # the dead third row of a monocular observation (L1: weight(0) is NaN)
            J = s[:, :, None] * np.einsum('nij,njk,nkl->nil', S, Jc, R)
            rs = s * r
        lane = q % 16
        lanes[0, m, lane] += rho.sum(axis=1)
        lanes[1, m, lane] += ~(pc[:, 2] > 0.)
        for row in range(3):                                  # (row by row, as the kernel adds them)
            lanes[2:8, m, lane] += _outer6(J[:, row, :]).T
            lanes[8:11, m, lane] += (J[:, row, :] * rs[:, row:row + 1]).T
    tot = _group16_sum(lanes)
    return tot[0], tot[2:8].T, tot[8:11].T, tot[1]


def triangulate(lp, vids=None, refine_iters=5, min_parallax_deg=1.0):
    """The variable landmarks `vids` (None: all, in vid order) of the tables `lp`.  -> (points (n, 3), status (n,) int32): the
    new point, or the old one where the status is not 0."""
    nv = lp.num_var_points
    vids = np.arange(nv) if vids is None else np.asarray(vids, dtype=np.int64).reshape(-1)
    n = vids.size
    tr = _Tracks(lp, vids)
    old = lp.points[tr.points].copy()
    status = np.zeros(n, dtype=np.int32)
    if n == 0:
        return old, status
    # ---- linear start
    lanes = np.zeros((10, n, 16))
    rays = np.zeros((n, max(tr.maxlen, 1), 3))
    for q in range(tr.maxlen):
        m = tr.valid[:, q]
        o = tr.obs[m, q]
        cam = lp.cams[lp.obs_groups[lp.obs_grp[o], 0].astype(int)]
        T = lp.poses[lp.obs_pose[o]]
        uvd = lp.obs_uvd[o]
        xn, yn = (uvd[:, 0] - cam[:, 0]) / cam[:, 2], (uvd[:, 1] - cam[:, 1]) / cam[:, 3]
        r1, r2, r3, t = T[:, 0:3], T[:, 3:6], T[:, 6:9], T[:, 9:12]
        depth = cam[:, 4] != -2.
        with np.errstate(all='ignore'):
            z = np.where(cam[:, 4] == -1., uvd[:, 2], cam[:, 2] * cam[:, 4] / uvd[:, 2])
        rows = [(xn[:, None] * r3 - r1, -(xn * t[:, 2] - t[:, 0]), np.ones(o.size, dtype=bool)),
                (yn[:, None] * r3 - r2, -(yn * t[:, 2] - t[:, 1]), np.ones(o.size, dtype=bool)),
                (r3, z - t[:, 2], depth)]
        lane = q % 16
        for a, rhs, use in rows:
            with np.errstate(all='ignore'):
                A6, g3 = _outer6(a), a * rhs[:, None]
            lanes[0:6, m, lane] += np.where(use[None, :], A6.T, 0.)
            lanes[6:9, m, lane] += np.where(use[None, :], g3.T, 0.)
        lanes[9, m, lane] += depth
        nrm = np.sqrt(xn * xn + yn * yn + 1.0)
        R = T[:, :9].reshape(-1, 3, 3)
        rays[m, q] = (R[:, 0, :] * xn[:, None] + R[:, 1, :] * yn[:, None] + R[:, 2, :]) / nrm[:, None]
    tot = _group16_sum(lanes)
    A, g3, ndepth = tot[0:6].T, tot[6:9].T, tot[9]
    status[(tr.len < 2) & (ndepth == 0.)] = FEW_OBS
    cosines = np.einsum('nqi,npi->nqp', rays, rays)
    pair_ok = tr.valid[:, :, None] & tr.valid[:, None, :] if tr.maxlen else np.zeros((n, 1, 1), dtype=bool)
    min_cos = np.minimum(1.0, np.where(pair_ok, cosines, np.inf).min(axis=(1, 2)))
    status[(status == OK) & (ndepth == 0.) & (min_cos > np.cos(np.deg2rad(min_parallax_deg)))] = DEGENERATE
    p, ok = _chol_solve(A, g3)
    status[(status == OK) & ~ok] = DEGENERATE
    # ---- Gauss-Newton on each landmark's own cost
    active = status == OK
    p = np.where(active[:, None], p, 0.)
    cand = p.copy()
    cost, H, g, behind = np.zeros(n), np.zeros((n, 6)), np.zeros((n, 3)), np.zeros(n)
    for it in range(refine_iters + 1):
        c, Hn, gn, bh = _evaluate(lp, tr, cand)
        with np.errstate(all='ignore'):
            take = active & ((it == 0) | (c < cost))
        active &= take
        cost, behind = np.where(take, c, cost), np.where(take, bh, behind)
        p, H, g = np.where(take[:, None], cand, p), np.where(take[:, None], Hn, H), np.where(take[:, None], gn, g)
        if it < refine_iters:
            dx, ok = _chol_solve(H, -g)
            active &= ok                                      # no step to try: done, at the last accepted point (status kept)
            cand = np.where(active[:, None], p + dx, p)
    status[(status == OK) & (behind > 0.)] = BEHIND
    return np.where((status == OK)[:, None], p, old), status


def triangulate_tables(lp, refine_iters=5, min_parallax_deg=1.0):
    """pyslam_amd.triangulate_tables on the host: (points (L, 3), status (L,) int32, -1 for a constant point)."""
    pts, st = triangulate(lp, None, refine_iters, min_parallax_deg)
    points = np.array(lp.points, dtype=np.float64).reshape(-1, 3)
    status = np.full(points.shape[0], -1, dtype=np.int32)
    var = np.nonzero(lp.point_vid >= 0)[0]
    points[var] = pts[lp.point_vid[var]]
    status[var] = st[lp.point_vid[var]]
    return points, status
