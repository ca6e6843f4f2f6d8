"""The landmark elimination of a bundle adjustment restated in numpy long double (x87 extended: 64-bit mantissa), as the reference
the off-box tests measure the device and the fp64 oracle against (tests/test_offbox_host.py, tests/test_gpu_offbox.py).

The IRLS-scaled blocks r~, J~p, J~l come from the oracle (oracle/gn_oracle.py: eval_reproj, run on tables of `dtype`; or handed in);
everything behind them -- C = sum J~l^T J~l, its inverse and inverse Cholesky factor, c, the reduced S and g in device order (poses
by rid, landmarks by vid), the landmark part of a step -- is formed in `dtype`.  dtype=np.float64 runs the same code in fp64: the
twin whose distance from the long double result is the fp64 oracle's own rounding error (e64) on a scene.  Vectorised (batched
3 x 3, np.add.at): 180 000 rows take seconds.  Counterpart of reference pyslam/problem.py:332-333 (J~^T J~, -J~^T e~) + :186 (the solve), eliminated by landmark."""
import numpy as np

from oracle import gn_oracle as orc

LONGDOUBLE_OK = np.finfo(np.longdouble).eps < 1e-18
LONGDOUBLE_SKIP = 'np.longdouble is no wider than 1e-18 here (eps {:.1e}): no reference better than fp64'.format(
    float(np.finfo(np.longdouble).eps))


def _per_loss(lp, fn, x):
    """fn(loss id, k, rows) of the oracle, by distinct (loss id, k) instead of by group row (a table with one row per observation
    has few losses): the same function on the same numbers as orc._by_group."""
    key = lp.obs_groups[lp.obs_grp][:, 2:4]
    out = np.empty_like(x)
    for lid, k in np.unique(key, axis=0):
        m = (key[:, 0] == lid) & (key[:, 1] == k)
        out[m] = fn(lid, k, x[m])
    return out


def mono_rows(lp):
    return lp.cams[lp.obs_groups[lp.obs_grp, 0].astype(int), 4] == -2.


def in_dtype(lp, dtype):
    """The problem with its real-valued observation tables in `dtype`: the oracle's block evaluation (numpy throughout) then runs
    in that precision."""
    if dtype == np.float64:
        return lp
    out = lp.copy()
    for name in ('poses', 'points', 'obs_uvd', 'cams', 'stiff3'):
        setattr(out, name, getattr(lp, name).astype(dtype))
    return out


def one_ulp_away(lp, draw):
    """The problem with every pose entry, landmark coordinate and observation moved by -1, 0 or +1 ulp (seeded by `draw`): another
    input of the same conditioning on which to SAMPLE the fp64 evaluation error -- its fp64 result against its OWN long-double
    result, never against the unmoved problem's (that difference would be the scene's sensitivity to its input, not rounding).
    What an evaluation order does to a residual -- a few ulps of the pixel coordinate, in rows it picks by accident -- falls on other
    rows in every copy; under a loss whose weight is 1 / |r| (L1, Huber's tail) the consequence is heavy-tailed, and one
    evaluation's largest error says little about another's."""
    rng = np.random.default_rng([draw, 15])
    out = lp.copy()
    for name in ('poses', 'points', 'obs_uvd'):
        a = getattr(lp, name)
        setattr(out, name, np.nextafter(a, a + rng.integers(-1, 2, size=a.shape) * np.abs(a)))
    return out


def scaled_blocks(lp, dtype=np.float64):
    """(r~ (N, 3), J~p (N, 3, 6), J~l (N, 3, 3)): the oracle's blocks (orc.eval_reproj, evaluated in `dtype`) times the square
    root of the IRLS weight, as tests/test_gpu_parity.py::test_reproj_blocks forms them.  The dead third row of a monocular
    observation (r = 0, J = 0) has the scale 1: L1's weight at 0 is NaN on the host, the device pins that row's scale
    (csrc/ps_math.h: reproj_eval_s).

    Why not the fp64 blocks, cast: r = S (project(T p) - obs) cancels pixel coordinates of ~1e3 down to the residual, so an fp64
    evaluation carries an absolute error of ~4e-13 px -- 4e-12 of a residual that is all noise (0.03 px in its largest component
    happens among 3000 rows of 0.3 px noise).  The oracle in fp64 misses TOL_BLOCK per row against itself in long double there."""
    r, Jp, Jl = orc.eval_reproj(in_dtype(lp, dtype))
    assert r.dtype == dtype and Jp.dtype == dtype and Jl.dtype == dtype
    s = np.sqrt(_per_loss(lp, orc.loss_weight, r))
    s[mono_rows(lp), 2] = 1.
    return s * r, s[:, :, None] * Jp, s[:, :, None] * Jl


def costs(lp, dtype=np.float64):
    """(sum of rho over every observation, over those with a variable pose or landmark): orc.eval_cost(lp, True / False) for a
    problem of observations only, with the losses taken by class."""
    rho = _per_loss(lp, orc.loss_rho, orc.eval_reproj(in_dtype(lp, dtype), jac=False)).sum(axis=1)
    act = (lp.pose_rid[lp.obs_pose] >= 0) | (lp.point_vid[lp.obs_point] >= 0)
    return float(rho.sum()), float(rho[act].sum())


def _inverse_cholesky(C):
    """M = L^-1 (lower, (n, 3, 3)) with C = L L^T, entry by entry in C's dtype (numpy's linalg has no long double)."""
    l00 = np.sqrt(C[:, 0, 0])
    l10, l20 = C[:, 1, 0] / l00, C[:, 2, 0] / l00
    l11 = np.sqrt(C[:, 1, 1] - l10 * l10)
    l21 = (C[:, 2, 1] - l20 * l10) / l11
    l22 = np.sqrt(C[:, 2, 2] - l20 * l20 - l21 * l21)
    M = np.zeros_like(C)
    M[:, 0, 0], M[:, 1, 1], M[:, 2, 2] = 1 / l00, 1 / l11, 1 / l22
    M[:, 1, 0] = -l10 * M[:, 0, 0] * M[:, 1, 1]
    M[:, 2, 1] = -l21 * M[:, 1, 1] * M[:, 2, 2]
    M[:, 2, 0] = -(l20 * M[:, 0, 0] + l21 * M[:, 1, 0]) * M[:, 2, 2]
    return M


def _inverse(C):
    """C^-1 of symmetric 3 x 3 blocks (n, 3, 3): adjugate over determinant, in C's dtype."""
    a, b, c, d, e, f = C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]
    A = np.zeros_like(C)
    A[:, 0, 0] = d * f - e * e
    A[:, 0, 1] = A[:, 1, 0] = c * e - b * f
    A[:, 0, 2] = A[:, 2, 0] = b * e - c * d
    A[:, 1, 1] = a * f - c * c
    A[:, 1, 2] = A[:, 2, 1] = b * c - a * e
    A[:, 2, 2] = a * d - b * b
    det = a * A[:, 0, 0] + b * A[:, 0, 1] + c * A[:, 0, 2]
    return A / det[:, None, None]


class Elimination:
    """Fields, all in `dtype`: C (nv, 3, 3) damped, M (nv, 3, 3) its inverse Cholesky factor (C^-1 = M^T M: what the device keeps
    as "Cinv", ps_get_landmark_factors), cvec (nv, 3) = M b_l, Cinv, S (6 nr, 6 nr), g (6 nr) -- or, with diagonal_only, Sdiag
    (nr, 6, 6) in place of S."""

    def __init__(self, lp, lam=0., dtype=np.longdouble, blocks=None, diagonal_only=False):
        r, Jp, Jl = [np.asarray(a).astype(dtype) for a in (blocks if blocks is not None else scaled_blocks(lp, dtype))]
        self.dtype, self.lp = dtype, lp
        nr, nv = lp.num_reduced, lp.num_var_points
        rid, vid = lp.pose_rid[lp.obs_pose].astype(np.int64), lp.point_vid[lp.obs_point].astype(np.int64)
        pv, lv = rid >= 0, vid >= 0
        damp = dtype(1) + dtype(lam)
        eye6, eye3 = np.identity(6, dtype=bool), np.identity(3, dtype=bool)
        # pose side: H_pp (block diagonal before the elimination) and b_p
        Hpp = np.zeros((nr, 6, 6), dtype=dtype)
        bp = np.zeros((nr, 6), dtype=dtype)
        np.add.at(Hpp, rid[pv], np.einsum('nki,nkj->nij', Jp[pv], Jp[pv]))
        np.add.at(bp, rid[pv], -np.einsum('nki,nk->ni', Jp[pv], r[pv]))
        Hpp[:, eye6] *= damp
        # landmark side
        C = np.zeros((nv, 3, 3), dtype=dtype)
        bl = np.zeros((nv, 3), dtype=dtype)
        np.add.at(C, vid[lv], np.einsum('nki,nkj->nij', Jl[lv], Jl[lv]))
        np.add.at(bl, vid[lv], -np.einsum('nki,nk->ni', Jl[lv], r[lv]))
        C[:, eye3] *= damp
        M = _inverse_cholesky(C)
        self.C, self.M, self.bl, self.Hpp, self.bp = C, M, bl, Hpp, bp
        self.cvec = np.einsum('vij,vj->vi', M, bl)
        self.Cinv = _inverse(C)
        # rows that couple a variable pose with a variable landmark: W_n = J~p_n^T J~l_n (6 x 3), E_n = W_n C^-1 -- the explicit
        # inverse between the two factors, as the oracle's dense Schur complement forms it (tests/test_gpu_parity.py:
        # oracle_reduced), so that the fp64 twin's error is the oracle's
        both = np.flatnonzero(pv & lv)
        both = both[np.argsort(vid[both], kind='stable')]
        self.rows, self.rows_rid, self.rows_vid = both, rid[both], vid[both]
        W = np.einsum('nki,nkj->nij', Jp[both], Jl[both])
        E = np.einsum('nij,njk->nik', W, self.Cinv[vid[both]])
        self.W, self.E = W, E
        g = bp.copy()
        np.add.at(g, rid[both], -np.einsum('nij,nj->ni', E, bl[vid[both]]))
        self.g = g.reshape(-1)
        # every ordered pair of rows of one landmark
        count = np.bincount(vid[both], minlength=nv)
        start = np.concatenate([[0], np.cumsum(count)[:-1]])
        per_row = count[vid[both]]
        a = np.repeat(np.arange(both.size), per_row)
        b = np.repeat(start[vid[both]], per_row) + (np.arange(a.size) - np.repeat(np.cumsum(per_row) - per_row, per_row))
        if diagonal_only:
            keep = rid[both][a] == rid[both][b]
            a, b = a[keep], b[keep]
            Sd = Hpp.copy()
            np.add.at(Sd, rid[both][a], -np.einsum('nik,njk->nij', E[a], W[b]))
            self.Sdiag = Sd
            return
        Sb = np.zeros((nr, nr, 6, 6), dtype=dtype)
        Sb[np.arange(nr), np.arange(nr)] = Hpp
        np.add.at(Sb, (rid[both][a], rid[both][b]), -np.einsum('nik,njk->nij', E[a], W[b]))
        self.S = Sb.transpose(0, 2, 1, 3).reshape(6 * nr, 6 * nr)

    def backsub(self, dx_pose):
        """dx_l (nv, 3) = C^-1 (b_l - W^T dx_p) for the pose step dx_pose (nr, 6)."""
        t = self.bl.copy()
        xp = np.asarray(dx_pose).astype(self.dtype)
        np.add.at(t, self.rows_vid, -np.einsum('nji,nj->ni', self.W, xp[self.rows_rid]))
        return np.einsum('vij,vj->vi', self.Cinv, t)

    def normal_equations(self):
        """Dense (J~^T J~ (+ damping), -J~^T r~) in device order [poses by rid | landmarks by vid]: orc.normal_equations(lp,
        points_first=False) from these blocks -- finite where the oracle's are not (its L1 weight of a dead monocular row)."""
        nr, nv = self.Hpp.shape[0], self.C.shape[0]
        n = 6 * nr
        P = np.zeros((n + 3 * nv, n + 3 * nv), dtype=self.dtype)
        for k in range(nr):
            P[6 * k:6 * k + 6, 6 * k:6 * k + 6] = self.Hpp[k]
        Wb = np.zeros((nr, nv, 6, 3), dtype=self.dtype)
        np.add.at(Wb, (self.rows_rid, self.rows_vid), self.W)
        P[:n, n:] = Wb.transpose(0, 2, 1, 3).reshape(n, 3 * nv)
        P[n:, :n] = P[:n, n:].T
        i = n + 3 * np.arange(nv)
        for a in range(3):
            for b in range(3):
                P[i + a, i + b] = self.C[:, a, b]
        return P, np.concatenate([self.bp.reshape(-1), self.bl.reshape(-1)])

    def device_factors(self):
        """(Cinv (nv, 6), c (nv, 3)) laid out as ps_get_landmark_factors returns them: the lower triangle of M by rows."""
        M = self.M
        return np.stack([M[:, 0, 0], M[:, 1, 0], M[:, 1, 1], M[:, 2, 0], M[:, 2, 1], M[:, 2, 2]], axis=1), self.cvec


# ---------------------------------------------------------------------------
# error measures: per row / per block, relative to that row's or block's own largest reference entry
# ---------------------------------------------------------------------------
def row_err(got, ref):
    """max over rows of (largest |got - ref| in the row) / (largest |ref| in the row); a row whose reference is all zero must be
    zero (else inf).  The first axis numbers the rows.  Differences are formed in the reference's dtype."""
    ref = np.asarray(ref)
    ref = ref.reshape(ref.shape[0], -1)
    got = np.asarray(got).reshape(ref.shape).astype(ref.dtype)
    if ref.shape[0] == 0:
        return 0.
    diff, scale = np.abs(got - ref).max(axis=1), np.abs(ref).max(axis=1)
    if not np.all(np.isfinite(diff)):
        return float('inf')
    err = np.where(scale > 0, diff / np.where(scale > 0, scale, 1), np.where(diff > 0, np.inf, 0))
    return float(err.max())


def block_err(S, Sref, d=6):
    """row_err over the d x d blocks of a square matrix."""
    n = np.asarray(Sref).shape[0] // d
    cut = lambda A: np.asarray(A).reshape(n, d, n, d).transpose(0, 2, 1, 3).reshape(n * n, d * d)
    return row_err(cut(S), cut(Sref))


def vec_err(g, gref, d=6):
    return row_err(np.asarray(g).reshape(-1, d), np.asarray(gref).reshape(-1, d))


def max_err(got, ref):
    """Largest difference over the largest entry of the whole array (the measure of EXPECTED_E64 in tests/offbox_scenes.py)."""
    ref = np.asarray(ref)
    return float(np.abs(np.asarray(got).astype(ref.dtype) - ref).max() / np.abs(ref).max())
