"""Host restatement (numpy) of the device's two-view initialisation (csrc/ps_k_twoview.h, ps_twoview_*): the same definition,
the same sign rule, candidate order and tie rules.  Test infrastructure and documentation of the definition, as featproc.py and
triangulation.py are; nothing on the solving path calls it.

With x = ((u - cu) / fu, (v - cv) / fv, 1) the normalised coordinates of a correspondence in either image:

1. Eight-point hypothesis.  Each of the 8 sampled correspondences gives the row kron(x_2, x_1) of the 8 x 9 matrix A; the
   hypothesis is its null vector (here: the last right singular vector of ``np.linalg.svd(A)``; the device eliminates with
   complete pivoting -- neither forms A^T A), reshaped row-major to F with x_2^T F x_1 = 0.  A sample with a repeated index or a
   rank-deficient A (here sigma_8 <= 1e-12 sigma_1; on the device a pivot not above 1e-12 of the first) is degenerate: E = 0,
   count 0, flag set.
2. Projection.  F = U S V^T,  E = U diag(1, 1, 0) V^T  (Frobenius norm sqrt 2).  Sign rule: the entry of E with the largest
   absolute value is positive; of equal magnitudes the lowest row-major index decides.
3. Score.  r = x_2^T E x_1, l = E x_1, l' = E^T x_2;  d = r^2 / ((l_1^2 + l'_1^2) / fu^2 + (l_2^2 + l'_2^2) / fv^2), the squared
   Sampson distance in pixel units.  Inlier: denominator > 0 and d < thresh.
4. Best: the first hypothesis with the maximal count (``np.argmax``).
5. Refit over its inliers: Hartley normalisation per image (centroid c, s = sqrt 2 / mean distance to c, x~ = s (x - c)),
   M = sum a a^T with a = kron(x~_2, x~_1), eigenvector of the smallest eigenvalue, F = T_2^T F~ T_1, steps 2 and 3 again.  Kept
   when it is not degenerate and its count is not lower.
6. Decomposition of the winner: u_3 the unit left null vector of E with its largest component positive (lowest index decides),
   (u_1, v_1), (u_2, v_2) singular pairs with u_1 x u_2 = u_3, v_3 = v_1 x v_2, W = [0 -1 0; 1 0 0; 0 0 1]; candidates in the order
   (U W V^T, +u_3), (U W V^T, -u_3), (U W^T V^T, +u_3), (U W^T V^T, -u_3), det R = +1.  For each, every inlier's rays
   t + lambda R x_1 and mu x_2 are intersected by the midpoint formula; the count is the number of inliers with positive lambda
   and mu.  The highest count wins, the lowest index first.  T_21 = [R | t] with |t| = 1.
"""
import numpy as np

DEGENERATE_RATIO = 1e-12
W = np.array([[0., -1., 0.], [1., 0., 0.], [0., 0., 1.]])


def normalise(obs, cam):
    """(N, 2+) pixels -> (N, 2) normalised coordinates."""
    obs = np.asarray(obs, dtype=np.float64)
    return np.stack([(obs[:, 0] - cam[0]) / cam[2], (obs[:, 1] - cam[1]) / cam[3]], axis=1)


def fix_sign(E):
    """The sign rule: the largest |entry| (first of equals, row-major) is positive."""
    flat = E.reshape(-1)
    return -E if flat[np.argmax(np.abs(flat))] < 0. else E


def project_essential(F):
    """(E, ok): U diag(1, 1, 0) V^T with the sign rule; ok False (E = 0) when F has rank < 2 or is not finite."""
    if not np.isfinite(F).all():
        return np.zeros((3, 3)), False
    U, S, Vt = np.linalg.svd(F)
    if not (S[0] > 0. and S[1] > DEGENERATE_RATIO * S[0]):
        return np.zeros((3, 3)), False
    return fix_sign(np.outer(U[:, 0], Vt[0]) + np.outer(U[:, 1], Vt[1])), True


def design_rows(x1, x2):
    """Rows kron(x_2, x_1) of the normalised (n, 2) coordinates -> (n, 9)."""
    h1 = np.concatenate([x1, np.ones((x1.shape[0], 1))], axis=1)
    h2 = np.concatenate([x2, np.ones((x2.shape[0], 1))], axis=1)
    return (h2[:, :, None] * h1[:, None, :]).reshape(-1, 9)


def eight_point(x1, x2, sample):
    """(E, ok, sigma) of one sample of 8 indices; sigma: the singular values of A (None for a repeated index)."""
    sample = np.asarray(sample)
    if np.unique(sample).size != sample.size:
        return np.zeros((3, 3)), False, None
    A = design_rows(x1[sample], x2[sample])
    if not np.isfinite(A).all():
        return np.zeros((3, 3)), False, None
    _, S, Vt = np.linalg.svd(A)
    if not (S[0] > 0. and S[7] > DEGENERATE_RATIO * S[0]):
        return np.zeros((3, 3)), False, S
    E, ok = project_essential(Vt[8].reshape(3, 3))
    return E, ok, S


def sampson(E, x1, x2, cam):
    """Squared Sampson distance (N,) in pixel units, in the device's order of operations; inf where the denominator is not > 0."""
    ifu2, ifv2 = 1.0 / (cam[2] * cam[2]), 1.0 / (cam[3] * cam[3])
    a, b, c, d = x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]
    l0 = E[0, 0] * a + E[0, 1] * b + E[0, 2]
    l1 = E[1, 0] * a + E[1, 1] * b + E[1, 2]
    l2 = E[2, 0] * a + E[2, 1] * b + E[2, 2]
    r = c * l0 + d * l1 + l2
    m0 = E[0, 0] * c + E[1, 0] * d + E[2, 0]
    m1 = E[0, 1] * c + E[1, 1] * d + E[2, 1]
    den = (l0 * l0 + m0 * m0) * ifu2 + (l1 * l1 + m1 * m1) * ifv2
    with np.errstate(all='ignore'):
        dist = (r * r) / den
    return np.where(den > 0., dist, np.inf)


def score(E, x1, x2, cam, thresh):
    """(mask (N,) bool, d (N,))."""
    d = sampson(E, x1, x2, cam)
    with np.errstate(invalid='ignore'):
        return d < thresh, d


def hypotheses(obs_1, obs_2, cam, samples, thresh):
    """Every sample's (E (H, 3, 3), counts (H,), degenerate (H,) bool, d (H, N))."""
    x1, x2 = normalise(obs_1, cam), normalise(obs_2, cam)
    H = len(samples)
    E = np.zeros((H, 3, 3))
    counts = np.zeros(H, dtype=np.int32)
    degenerate = np.zeros(H, dtype=bool)
    dist = np.full((H, x1.shape[0]), np.inf)
    for h, s in enumerate(samples):
        E[h], ok, _ = eight_point(x1, x2, s)
        degenerate[h] = not ok
        if ok:
            mask, dist[h] = score(E[h], x1, x2, cam, thresh)
            counts[h] = mask.sum()
    return E, counts, degenerate, dist


def hartley(x):
    """(centroid (2,), scale) of the (n, 2) coordinates."""
    c = x.mean(axis=0)
    with np.errstate(all='ignore'):
        s = np.sqrt(2.) / np.sqrt(((x - c) ** 2).sum(axis=1)).mean()
    return c, s


def refit(x1, x2, mask):
    """(E, ok) of the normalised eight-point fit over the correspondences in `mask`."""
    if mask.sum() < 8:
        return np.zeros((3, 3)), False
    c1, s1 = hartley(x1[mask])
    c2, s2 = hartley(x2[mask])
    if not (np.isfinite([s1, s2]).all() and s1 > 0. and s2 > 0.):
        return np.zeros((3, 3)), False
    A = design_rows(s1 * (x1[mask] - c1), s2 * (x2[mask] - c2))
    w, V = np.linalg.eigh(A.T @ A)
    Fn = V[:, np.argmin(w)].reshape(3, 3)
    T1 = np.array([[s1, 0., -s1 * c1[0]], [0., s1, -s1 * c1[1]], [0., 0., 1.]])
    T2 = np.array([[s2, 0., -s2 * c2[0]], [0., s2, -s2 * c2[1]], [0., 0., 1.]])
    return project_essential(T2.T @ Fn @ T1)


def candidates(E):
    """The four (R, t) of the essential matrix E in the fixed order, or None when E has rank < 2."""
    U, S, Vt = np.linalg.svd(E)
    if not (S[0] > 0. and S[1] > DEGENERATE_RATIO * S[0]):
        return None
    u1, u2, v1, v2 = U[:, 0], U[:, 1], Vt[0], Vt[1]
    u3 = np.cross(u1, u2)
    if u3[np.argmax(np.abs(u3))] < 0.:
        u1, v1, u3 = -u1, -v1, -u3
    v3 = np.cross(v1, v2)
    Um, Vm = np.stack([u1, u2, u3], axis=1), np.stack([v1, v2, v3], axis=1)
    Ra, Rb = Um @ W @ Vm.T, Um @ W.T @ Vm.T
    Ra, Rb = (R if np.linalg.det(R) > 0. else -R for R in (Ra, Rb))
    return [(Ra, u3), (Ra, -u3), (Rb, u3), (Rb, -u3)]


def midpoint_depths(R, t, x1, x2):
    """(lambda, mu, det, cos parallax) of the rays t + lambda R x_1 and mu x_2 for the (n, 2) normalised coordinates."""
    h1 = np.concatenate([x1, np.ones((x1.shape[0], 1))], axis=1)
    b = np.concatenate([x2, np.ones((x2.shape[0], 1))], axis=1)
    a = h1 @ R.T
    aa, bb, ab = (a * a).sum(axis=1), (b * b).sum(axis=1), (a * b).sum(axis=1)
    at, bt = a @ t, b @ t
    det = aa * bb - ab * ab
    with np.errstate(all='ignore'):
        lam, mu = (ab * bt - bb * at) / det, (aa * bt - ab * at) / det
        cs = ab / np.sqrt(aa * bb)
    return lam, mu, det, cs


def cheirality(E, x1, x2, mask):
    """(T_21 (4, 4), counts (4,), winner index, parallax_deg of the inliers) of the vote over the correspondences in `mask`."""
    cands = candidates(E)
    T = np.identity(4)
    if cands is None:
        T[:3, 3] = 0.
        return T, np.zeros(4, dtype=np.int32), 0, np.zeros(int(mask.sum()))
    counts = np.zeros(4, dtype=np.int32)
    for k, (R, t) in enumerate(cands):
        lam, mu, det, _ = midpoint_depths(R, t, x1[mask], x2[mask])
        with np.errstate(invalid='ignore'):
            counts[k] = ((det > 0.) & (lam > 0.) & (mu > 0.)).sum()
    win = int(np.argmax(counts))
    R, t = cands[win]
    T[:3, :3], T[:3, 3] = R, t
    cs = midpoint_depths(R, t, x1[mask], x2[mask])[3]
    return T, counts, win, np.degrees(np.arccos(np.clip(cs, -1., 1.)))


def ransac(obs_1, obs_2, cam, samples, thresh, refit_winner=True):
    """The whole chain.  -> dict: T_21, E, mask, d (the final matrix' distances), best, raw_count, count, refit_kept,
    cheirality_counts, parallax_deg (of the inliers), E_all, counts, degenerate, dist (all hypotheses')."""
    x1, x2 = normalise(obs_1, cam), normalise(obs_2, cam)
    E_all, counts, degenerate, dist = hypotheses(obs_1, obs_2, cam, samples, thresh)
    best = int(np.argmax(counts))
    E = E_all[best]
    mask, d = score(E, x1, x2, cam, thresh)
    raw_count, kept = int(mask.sum()), False
    d_refit = None
    if refit_winner and raw_count >= 8:
        E2, ok = refit(x1, x2, mask)
        if ok:
            mask2, d_refit = score(E2, x1, x2, cam, thresh)
            if mask2.sum() >= raw_count:
                E, mask, d, kept = E2, mask2, d_refit, True
    T, ccounts, win, par = cheirality(E, x1, x2, mask)
    return dict(T_21=T, E=E, mask=mask, d=d, best=best, raw_count=raw_count, count=int(mask.sum()), refit_kept=kept,
                cheirality_counts=ccounts, winner=win, parallax_deg=par, E_all=E_all, counts=counts, degenerate=degenerate,
                dist=dist, d_raw=dist[best], d_refit=d_refit)


def essential_from_pose(R, t):
    """[t]x R / |t|, with the sign rule (E of the pose p_2 = R p_1 + t)."""
    t = np.asarray(t, dtype=np.float64) / np.linalg.norm(t)
    tx = np.array([[0., -t[2], t[1]], [t[2], 0., -t[0]], [-t[1], t[0], 0.]])
    return fix_sign(tx @ np.asarray(R, dtype=np.float64))
