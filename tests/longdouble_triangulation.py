"""Multi-view triangulation (device: csrc/ps_k_triang.h) restated in numpy long double, as the reference
tests/test_gpu_triang.py measures the device against.  Written from the definition, not from pyslam_amd/triangulation.py: sums are
plain scatter-adds over a landmark's observations (no lane order), the 3 x 3 systems are solved by a root-free L D L^T, and the
robust cost and its IRLS-scaled blocks are the oracle's (oracle/gn_oracle.py: eval_reproj, loss_rho, loss_weight) evaluated on tables
of `dtype`, as tests/longdouble_schur.py: scaled_blocks takes them.  Every function takes `dtype`: run with np.float64 the same code
is the twin whose distance from the long-double result on the same input is the rounding error of an fp64 evaluation (e64).

Landmarks are numbered by vid throughout; points handed in and out are (num_var_points, 3)."""
import types

import numpy as np

import longdouble_schur as ld
from oracle import gn_oracle as orc

OK, FEW_OBS, DEGENERATE, BEHIND = 0, 1, 2, 3


def _vid_of_obs(lp):
    vid = lp.point_vid[lp.obs_point].astype(np.int64)
    return vid, np.flatnonzero(vid >= 0)


def ldl_solve(A, b):
    """x = A^-1 b for symmetric (n, 3, 3) by L D L^T in A's dtype -> (x, pivots (n, 3) relative to their diagonal entries, ok).
    From the first pivot that is not positive (NaN included) on, the later pivots repeat it; ok is False there."""
    with np.errstate(all='ignore'):
        d0 = A[:, 0, 0]
        l10, l20 = A[:, 1, 0] / d0, A[:, 2, 0] / d0
        d1 = A[:, 1, 1] - l10 * l10 * d0
        l21 = (A[:, 2, 1] - l20 * l10 * d0) / d1
        d2 = A[:, 2, 2] - l20 * l20 * d0 - l21 * l21 * d1
        z0 = b[:, 0]
        z1 = b[:, 1] - l10 * z0
        z2 = b[:, 2] - l20 * z0 - l21 * z1
        x2 = z2 / d2
        x1 = z1 / d1 - l21 * x2
        x0 = z0 / d0 - l10 * x1 - l20 * x2
        piv = np.stack([d0 / np.abs(A[:, 0, 0]), d1 / np.abs(A[:, 1, 1]), d2 / np.abs(A[:, 2, 2])], axis=1)
        piv[:, 0] = np.where(d0 == 0, 0., piv[:, 0])                                   # (else 1, -1 or NaN)
        good = piv > 0
        piv[:, 1] = np.where(good[:, 0], piv[:, 1], piv[:, 0])
        good = piv > 0
        piv[:, 2] = np.where(good[:, 1], piv[:, 2], piv[:, 1])
    return np.stack([x0, x1, x2], axis=1), piv, np.all(piv > 0, axis=1)


def linear_start(lp, dtype=np.longdouble):
    """Per variable landmark: point (nv, 3), nobs, ndepth, min_cos (the smallest cosine between two of its viewing rays, 1 for a
    single one), pivots (nv, 3) of the normal equations relative to their diagonal, ok (all pivots positive), min_z (the smallest
    camera-frame z of the point over its observations; NaN where the point is not finite)."""
    q = ld.in_dtype(lp, dtype)
    nv = lp.num_var_points
    vid, rows = _vid_of_obs(lp)
    v = vid[rows]
    G = lp.obs_groups[lp.obs_grp[rows]]
    cu, cv, fu, fv, bl = q.cams[G[:, 0].astype(int)].T
    mono, rgbd = bl == -2, bl == -1
    T = q.poses[lp.obs_pose[rows]]
    r1, r2, r3, t = T[:, 0:3], T[:, 3:6], T[:, 6:9], T[:, 9:12]
    u = q.obs_uvd[rows]
    xn, yn = (u[:, 0] - cu) / fu, (u[:, 1] - cv) / fv
    with np.errstate(all='ignore'):
        z = np.where(rgbd, u[:, 2], fu * bl / u[:, 2])
        a = np.stack([xn[:, None] * r3 - r1, yn[:, None] * r3 - r2, np.where(mono[:, None], dtype(0), r3)], axis=1)     # (n, 3 rows, 3)
        rhs = np.stack([t[:, 0] - xn * t[:, 2], t[:, 1] - yn * t[:, 2], np.where(mono, dtype(0), z - t[:, 2])], axis=1)
        A = np.zeros((nv, 3, 3), dtype=dtype)
        g = np.zeros((nv, 3), dtype=dtype)
        np.add.at(A, v, np.einsum('nki,nkj->nij', a, a))
        np.add.at(g, v, np.einsum('nki,nk->ni', a, rhs))
    nobs = np.bincount(v, minlength=nv)
    ndepth = np.bincount(v, weights=~mono, minlength=nv).astype(np.int64)
    ray = np.einsum('nji,nj->ni', T[:, :9].reshape(-1, 3, 3), np.stack([xn, yn, np.ones_like(xn)], axis=1))
    ray = ray / np.sqrt(np.einsum('ni,ni->n', ray, ray))[:, None]
    min_cos = np.ones(nv, dtype=dtype)
    order = np.argsort(v, kind='stable')
    start = np.concatenate([[0], np.cumsum(nobs)])
    for k in range(nv):
        rk = ray[order[start[k]:start[k + 1]]]
        if len(rk) > 1:
            min_cos[k] = min(dtype(1), (rk @ rk.T).min())
    p, piv, ok = ldl_solve(A, g)
    with np.errstate(all='ignore'):
        zc = np.einsum('ni,ni->n', r3, p[v]) + t[:, 2]
    min_z = np.full(nv, np.inf, dtype=dtype)
    np.fmin.at(min_z, v, zc)
    nanz = np.zeros(nv, dtype=bool)
    np.logical_or.at(nanz, v, ~np.isfinite(zc))
    min_z[nanz] = np.nan
    return types.SimpleNamespace(point=p, nobs=nobs, ndepth=ndepth, min_cos=min_cos, pivots=piv, ok=ok, min_z=min_z)


def evaluate(lp, p, dtype=np.longdouble):
    """At the points p (nv, 3) of the variable landmarks, poses held: -> (cost (nv,), H (nv, 3, 3), g (nv, 3), min_z (nv,), r1 (nv,)).
    cost = sum of rho over the landmark's residual components, H = sum J~l^T J~l, g = sum J~l^T r~, min_z the smallest camera-frame z
    (NaN if one is not finite), r1 = sum of |r| (the scale an evaluation error of the cost is measured in)."""
    q = ld.in_dtype(lp, dtype).copy()
    var = np.flatnonzero(lp.point_vid >= 0)
    q.points[var] = np.asarray(p).astype(dtype)[lp.point_vid[var]]
    nv = lp.num_var_points
    vid, rows = _vid_of_obs(lp)
    v = vid[rows]
    with np.errstate(all='ignore'):
        r, _, Jl = orc.eval_reproj(q)
        assert r.dtype == dtype
        s = np.sqrt(ld._per_loss(lp, orc.loss_weight, r))
        s[ld.mono_rows(lp), 2] = 1.
        rho = ld._per_loss(lp, orc.loss_rho, r).sum(axis=1)
        Jt, rt = (s[:, :, None] * Jl)[rows], (s * r)[rows]
        cost, H, g = np.zeros(nv, dtype=dtype), np.zeros((nv, 3, 3), dtype=dtype), np.zeros((nv, 3), dtype=dtype)
        r1 = np.zeros(nv, dtype=dtype)
        np.add.at(cost, v, rho[rows])
        np.add.at(r1, v, np.abs(r[rows]).sum(axis=1))
        np.add.at(H, v, np.einsum('nki,nkj->nij', Jt, Jt))
        np.add.at(g, v, np.einsum('nki,nk->ni', Jt, rt))
        T = q.poses[lp.obs_pose[rows]]
        zc = np.einsum('ni,ni->n', T[:, 6:9], q.points[lp.obs_point[rows]]) + T[:, 11]
    min_z = np.full(nv, np.inf, dtype=dtype)
    np.fmin.at(min_z, v, zc)
    bad = np.zeros(nv, dtype=bool)
    np.logical_or.at(bad, v, ~np.isfinite(zc))
    min_z[bad] = np.nan
    return cost, H, g, min_z, r1


def gn_step(lp, p, dtype=np.longdouble, ev=None):
    """(-H^-1 g (nv, 3), ok (nv,)): the Gauss-Newton step of every landmark at p; ok False where H is not positive definite or holds
    a NaN (L1's weight at a zero residual)."""
    _, H, g, _, _ = ev if ev is not None else evaluate(lp, p, dtype)
    dx, _, ok = ldl_solve(H, -g)
    ok &= np.all(np.isfinite(dx), axis=1)
    return np.where(ok[:, None], dx, 0), ok


def refine(lp, p0, iters, dtype=np.longdouble, active=None):
    """The accept-if-lower loop from p0: a candidate p + gn_step(p) replaces p only if it lowers the landmark's cost; a landmark whose
    candidate does not, or whose system cannot be solved, is done.  -> (p, cost at p, min_z at p)."""
    p = np.array(p0, dtype=dtype)
    active = np.ones(len(p), dtype=bool) if active is None else active.copy()
    p[~active] = 1.
    ev = evaluate(lp, p, dtype)
    cost, min_z = ev[0].copy(), ev[3].copy()
    for _ in range(iters):
        dx, ok = gn_step(lp, p, dtype, ev)
        active &= ok
        if not active.any():
            break
        cand = np.where(active[:, None], p + dx, p)
        evc = evaluate(lp, cand, dtype)
        with np.errstate(all='ignore'):
            active &= evc[0] < cost
        p = np.where(active[:, None], cand, p)
        cost, min_z = np.where(active, evc[0], cost), np.where(active, evc[3], min_z)
        # H and g of the next step: the candidate's where it was taken (the others are done and never used again)
        ev = evc
    return p, cost, min_z


def triangulate(lp, refine_iters, min_parallax_deg, dtype=np.longdouble):
    """The whole definition -> (points (nv, 3): NaN where the status is not 0, status (nv,), clear (nv,) bool, lin): `clear` where no
    decision behind the status is within rounding's reach -- pivots of the linear start above 1e-6 of their diagonal entries (or
    the status settled before the solve), |min_cos - cos(min parallax)| above 1e-9 where parallax is asked about, and the smallest
    camera-frame z of the result beyond 1e-6 |p| on either side."""
    lin = linear_start(lp, dtype)
    cos_min = np.cos(dtype(min_parallax_deg) * np.arccos(dtype(-1)) / dtype(180))
    nv = lp.num_var_points
    status = np.zeros(nv, dtype=np.int32)
    clear = np.ones(nv, dtype=bool)
    few = (lin.nobs < 2) & (lin.ndepth == 0)
    status[few] = FEW_OBS
    asked = ~few & (lin.ndepth == 0)
    flat = asked & (lin.min_cos > cos_min)
    status[flat] = DEGENERATE
    clear &= ~asked | (np.abs(lin.min_cos - cos_min) > 1e-9)
    solved = status == OK
    status[solved & ~lin.ok] = DEGENERATE
    with np.errstate(all='ignore'):
        clear &= ~solved | (np.abs(lin.pivots).min(axis=1) > 1e-6)
    active = status == OK
    p, cost, min_z = refine(lp, lin.point, refine_iters, dtype, active)
    with np.errstate(all='ignore'):
        behind = active & ~(min_z > 0)
        scale = np.sqrt(np.einsum('ni,ni->n', p, p))
        clear &= ~active | ~np.isfinite(min_z) | (np.abs(min_z) > 1e-6 * scale)      # (no finite z: behind by definition)
    status[behind] = BEHIND
    return np.where((status == OK)[:, None], p, np.nan), status, clear, lin


def point_err(got, ref, rows=None):
    """Per landmark |got - ref| / |ref| in the reference's dtype; the largest over `rows` (all if None); 0 for no rows."""
    ref = np.asarray(ref)
    got = np.asarray(got).astype(ref.dtype)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    if len(ref) == 0:
        return 0.
    e = np.sqrt(((got - ref) ** 2).sum(axis=1)) / np.sqrt((ref ** 2).sum(axis=1))
    return float(e.max()) if np.all(np.isfinite(e)) else float('inf')


def cost_slack(lp, r1, dtype=np.longdouble):
    """What an fp64 evaluation of a landmark's cost may be off by, per landmark: a residual component is r = S (project - obs) with
    project and obs of the size of the largest pixel coordinate / depth M, each operand rounded and a dozen operations behind it:
    |dr| <= 32 eps64 |S| M =: delta, and d(rho) <= |rho'(r)| delta with |rho'(r)| <= |r| for L2, Huber and Cauchy and = 1 for L1,
    so <= (|r| + 1) delta per component; summed over a landmark: delta (r1 + 3 nobs) with r1 = sum |r|.  Two costs compared in fp64
    (one accepted as lower than the other) may stand the other way round in long double by at most twice that."""
    M = max(1., float(np.abs(lp.obs_uvd).max()))
    S = float(np.abs(lp.stiff3).max())
    delta = 32 * np.finfo(np.float64).eps * S * M
    vid, rows = _vid_of_obs(lp)
    nobs = np.bincount(vid[rows], minlength=lp.num_var_points)
    return 2 * delta * (np.asarray(r1, dtype=np.longdouble) + 3 * nobs)
