"""Host restatement (numpy) of the device's similarity (Sim(3)) alignment RANSAC (csrc/ps_k_sim3.h, ps_sim3_*): the same definition,
the same degeneracy, tie and refit rules.  Test infrastructure and documentation of the definition, as absolute.py is for the
absolute-pose front end; nothing on the solving path calls it.  The singular value decomposition is ``np.linalg.svd`` (the device
runs a one-sided Jacobi SVD), so the two agree to rounding and not bit for bit.

Input: N matched points pts_1, pts_2 (N, 3), H minimal sets of 3 point indices, a threshold.  Output: the model p_2 = s R p_1 + t
with s > 0, as the 4 x 4 matrix S = [s R | t; 0 0 0 1] and the scalar s.

1. Fit of n >= 3 pairs (Umeyama 1991).  Centroids c_1, c_2, q = p - c, W = sum q_2 q_1^T, v = sum |q_1|^2; W = U diag(sigma) V^T with
   sigma_a >= sigma_b >= sigma_c; R = u_a v_a^T + u_b v_b^T + (u_a x u_b)(v_a x v_b)^T (a proper rotation whatever the third pair is);
   d = sign((u_a x u_b) . u_c) sign((v_a x v_b) . v_c), 0 when sigma_c = 0; s = (sigma_a + sigma_b + d sigma_c) / v, or 1 with
   ``fixed_scale``; t = c_2 - s R c_1.
   A fit is DEGENERATE (flag set, S = 0, s = 0, count 0, every error +inf) with fewer than 3 pairs, when v is not positive or not
   finite, when W is not finite or sigma_b is not above 1e-6 sigma_a (collinear or repeated points), when s is not positive or not
   finite, or when an entry of S is not finite.
2. Score, from the stored S alone (M = s R its 3 x 3 block): a = M p_1 + t; s^2 = |M|_F^2 / 3, B = M^T / s^2, b = B p_2 - B t, which
   is R^T (p_2 - t) / s.  Pixel mode (a camera cam = (cu, cv, fu, fv, ...), pixels obs_1 of pts_1 in camera 1 and obs_2 of pts_2 in
   camera 2): e = max(|pi(a) - obs_2|^2, |pi(b) - obs_1|^2), NaN if either is; inlier: e < thresh, a_3 > 0 and b_3 > 0.  Metric mode
   (cam is None): e = |a - p_2|^2; inlier: e < thresh.  A NaN compares false.
3. Winner: the first hypothesis with the maximal count (np.argmax); its mask by one rescoring pass.
4. Refit: from the winner's model and mask up to ``refit_iters`` rounds, each a fit of all current inliers and a rescoring of every
   point.  A degenerate round, or a round with fewer inliers than the current count, ends the loop and is discarded; otherwise the round
   is adopted, and the loop ends after it when its mask equals the previous mask.
"""
import numpy as np

RATIO = 1e-6
EXHAUSTED, LOWER_COUNT, FIXED_POINT, DEGENERATE = 0, 1, 2, 3          # info[4] of ps_sim3_ransac: how the refit loop ended


def fit(p1, p2, fixed_scale=False):
    """(S (4, 4), s, ok, sigma_b / sigma_a) of the pairs p1, p2 (n, 3); S = 0, s = 0, ok False when the fit is degenerate (the
    ratio is nan where it was not reached)."""
    bad = (np.zeros((4, 4)), 0., False, np.nan)
    n = p1.shape[0]
    if n < 3:
        return bad
    with np.errstate(all='ignore'):
        c1, c2 = p1.sum(axis=0) / n, p2.sum(axis=0) / n
        q1, q2 = p1 - c1, p2 - c2
        W = q2.T @ q1
        v = (q1 * q1).sum()
        if not (v > 0.) or not np.isfinite(v) or not np.isfinite(W).all():
            return bad
        U, sg, Vt = np.linalg.svd(W)
        ratio = sg[1] / sg[0] if sg[0] > 0. else 0.
        if not (sg[1] > RATIO * sg[0]):
            return (bad[0], 0., False, ratio)
        ua, ub, va, vb = U[:, 0], U[:, 1], Vt[0], Vt[1]
        uc, vc = np.cross(ua, ub), np.cross(va, vb)
        R = np.outer(ua, va) + np.outer(ub, vb) + np.outer(uc, vc)
        s = 1.
        if not fixed_scale:
            d = np.sign(uc @ U[:, 2]) * np.sign(vc @ Vt[2]) if sg[2] > 0. else 0.
            s = (sg[0] + sg[1] + d * sg[2]) / v
            if not (s > 0.) or not np.isfinite(s):
                return (bad[0], 0., False, ratio)
        S = np.identity(4)
        S[:3, :3] = s * R
        S[:3, 3] = c2 - S[:3, :3] @ c1
        if not np.isfinite(S).all():
            return (bad[0], 0., False, ratio)
    return S, float(s), True, ratio


def errors(S, pts_1, pts_2, obs_1=None, obs_2=None, cam=None):
    """(e (N,), front (N,) bool) of the model S over every pair: step 2."""
    with np.errstate(all='ignore'):
        M, t = S[:3, :3], S[:3, 3]
        a = pts_1 @ M.T + t
        if cam is None:
            d = a - pts_2
            return (d * d).sum(axis=1), np.ones(pts_1.shape[0], dtype=bool)
        B = M.T / ((M * M).sum() / 3.)
        b = pts_2 @ B.T - B @ t
        du2, dv2 = cam[2] * a[:, 0] / a[:, 2] + cam[0] - obs_2[:, 0], cam[3] * a[:, 1] / a[:, 2] + cam[1] - obs_2[:, 1]
        du1, dv1 = cam[2] * b[:, 0] / b[:, 2] + cam[0] - obs_1[:, 0], cam[3] * b[:, 1] / b[:, 2] + cam[1] - obs_1[:, 1]
        return np.maximum(du2 * du2 + dv2 * dv2, du1 * du1 + dv1 * dv1), (a[:, 2] > 0.) & (b[:, 2] > 0.)


def score(S, pts_1, pts_2, obs_1, obs_2, cam, thresh):
    """(mask (N,) bool, e (N,))."""
    e, front = errors(S, pts_1, pts_2, obs_1, obs_2, cam)
    with np.errstate(invalid='ignore'):
        return front & (e < thresh), e


def _inputs(pts_1, pts_2, obs_1, obs_2, cam):
    p1, p2 = np.ascontiguousarray(pts_1, dtype=np.float64), np.ascontiguousarray(pts_2, dtype=np.float64)
    if cam is None:
        return p1, p2, None, None
    return (p1, p2, np.ascontiguousarray(np.asarray(obs_1, dtype=np.float64)[:, :2]),
            np.ascontiguousarray(np.asarray(obs_2, dtype=np.float64)[:, :2]))


def hypotheses(pts_1, pts_2, obs_1, obs_2, cam, samples, thresh, fixed_scale=False):
    """Every sample's model -> dict: S_all (H, 4, 4), scales (H,), counts (H,), flags (H,) bool (degenerate), d_all (H, N) (every
    error; +inf for a degenerate sample), ratio (H,) (sigma_b / sigma_a)."""
    p1, p2, o1, o2 = _inputs(pts_1, pts_2, obs_1, obs_2, cam)
    H, N = len(samples), p1.shape[0]
    S_all, scales, counts = np.zeros((H, 4, 4)), np.zeros(H), np.zeros(H, dtype=np.int32)
    flags, d_all, ratio = np.zeros(H, dtype=bool), np.full((H, N), np.inf), np.full(H, np.nan)
    for h, smp in enumerate(samples):
        s = [int(k) for k in smp]
        S, sc, ok, ratio[h] = fit(p1[s], p2[s], fixed_scale)
        if not ok:
            flags[h] = True
            continue
        S_all[h], scales[h] = S, sc
        mask, d_all[h] = score(S, p1, p2, o1, o2, cam, thresh)
        counts[h] = mask.sum()
    return dict(S_all=S_all, scales=scales, counts=counts, flags=flags, d_all=d_all, ratio=ratio)


def refit(S, scale, mask, pts_1, pts_2, obs_1, obs_2, cam, thresh, iters, fixed_scale=False):
    """Step 4 -> (S, scale, mask, rounds adopted, reason, d_rounds: the errors of every round that was scored, the discarded one
    included)."""
    count, rounds, reason, d_rounds = int(mask.sum()), 0, EXHAUSTED, []
    for _ in range(iters):
        S2, s2, ok, _ = fit(pts_1[mask], pts_2[mask], fixed_scale)
        if not ok:
            reason = DEGENERATE
            break
        mask2, d2 = score(S2, pts_1, pts_2, obs_1, obs_2, cam, thresh)
        d_rounds.append(d2)
        if mask2.sum() < count:
            reason = LOWER_COUNT
            break
        same = np.array_equal(mask2, mask)
        S, scale, mask, count, rounds = S2, s2, mask2, int(mask2.sum()), rounds + 1
        if same:
            reason = FIXED_POINT
            break
    return S, scale, mask, rounds, reason, d_rounds


def ransac(pts_1, pts_2, obs_1, obs_2, cam, samples, thresh, refit_iters=3, fixed_scale=False):
    """The whole chain.  -> dict: S_21, scale, mask, best, raw_count, count, rounds, reason, degenerate (the result is), d (the final
    model's errors; +inf when it is degenerate), d_raw, d_rounds, and what ``hypotheses`` returns."""
    p1, p2, o1, o2 = _inputs(pts_1, pts_2, obs_1, obs_2, cam)
    hyp = hypotheses(p1, p2, o1, o2, cam, samples, thresh, fixed_scale)
    best = int(np.argmax(hyp['counts']))                       # the first hypothesis with the maximal count
    valid = not hyp['flags'][best]
    S_raw, s_raw = hyp['S_all'][best].copy(), float(hyp['scales'][best])
    N = p1.shape[0]
    if valid:
        mask, d_raw = score(S_raw, p1, p2, o1, o2, cam, thresh)
    else:
        mask, d_raw = np.zeros(N, dtype=bool), np.full(N, np.inf)
    raw_count = int(mask.sum())
    S, s, mask, rounds, reason, d_rounds = refit(S_raw, s_raw, mask, p1, p2, o1, o2, cam, thresh, refit_iters, fixed_scale)
    d = errors(S, p1, p2, o1, o2, cam)[0] if valid else np.full(N, np.inf)
    out = dict(hyp)
    out.update(S_21=S, scale=s, mask=mask, best=best, raw_count=raw_count, count=int(mask.sum()), rounds=rounds, reason=reason,
               degenerate=not valid, d=d, d_raw=d_raw, d_rounds=d_rounds, S_raw=S_raw)
    return out
