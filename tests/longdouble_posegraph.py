"""The pose-factor definition restated in numpy long double (x87 extended: 64-bit mantissa): the reference the pose-graph tests measure
the device and the fp64 oracle against (tests/test_posegraph_host.py, tests/test_gpu_posegraph.py).  Written apart from
oracle/gn_oracle.py -- none of its Lie-group helpers is called: its `unpack` casts to float and its `wedge3` allocates fp64, so on
long-double tables it returns a float128 array computed in fp64.  Every intermediate here asserts its dtype for that reason.

SE(3) and SE(2): inv, mul, log, exp, Ad, the six losses' rho and weight, and per factor (edges, then priors: the device's order)
  r = S log(T_2 T_1^-1 T_obs^-1)   (a prior: S log(T_2 T_obs^-1)),   s_k = sqrt(w(r_k)),
  r~ = s r,   J~_1 = -diag(s) S Ad(T_2 T_1^-1),   J~_2 = diag(s) S,
an all-zero stiffness row being an ABSENT row (scale 0, no weight evaluated: the kernel's rule for rotation-only edges,
csrc/ps_k_linearize.h: k_factor_pass); then H_11, H_12, H_22, g_1, g_2 per factor, the assembled S and g in device order (poses by
pose_rid) with (1 + lambda) on the factor part of diagonal entries, the cost under both include_all conventions, and the retraction
exp(step dx_i) T_i.  Counterpart of reference pyslam/residuals/pose_to_pose_residual.py:12-32, pose_residual.py:12-27,
problem.py:332-360 and :110-128.

dtype=np.float64 runs the same code in fp64: the twin whose distance from the long-double result is fp64's own rounding error (e64).

BRANCHES belong to the definition that is checked: `ang <= 1e-8` (log), `|phi| <= 1e-8` (inverse left Jacobian, exp), the losses'
`|x| <= k` and L1's `|x| <= 1e-8`.  Both twins take the branch the FP64 value of the quantity selects (class Predicates: the fp64
evaluation runs first and records every predicate, the long-double one replays them).  Between 1e-8 and about 1.5e-8 an fp64 acos
returns 0 where a long-double acos resolves the angle: a reference that decided for itself would compute another formula there."""
import numpy as np

LONGDOUBLE_OK = np.finfo(np.longdouble).eps < 1e-18
LONGDOUBLE_SKIP = 'np.longdouble is no wider than 1e-18 here (eps {:.1e}): no reference better than fp64'.format(
    float(np.finfo(np.longdouble).eps))

SMALL = 1e-8                       # np.isclose(x, 0.) of the reference; PS_SMALL_ANGLE of the device
L2, L1, CAUCHY, HUBER, TUKEY, TDIST = range(6)
LOSS_NAMES = ('L2', 'L1', 'Cauchy', 'Huber', 'Tukey', 'TDist')


def _is(dtype, *arrays):
    for a in arrays:
        assert a.dtype == dtype, (a.dtype, dtype)
    return arrays[0] if len(arrays) == 1 else arrays


class Predicates:
    """Branch decisions by name.  Recording (the fp64 pass): `abs(value) <= limit` on an fp64 value, unless `force` names the
    predicate (True / False: every element into that branch -- how a test asks what the other branch would have given).
    Replaying (the long-double pass): the recorded decision."""

    def __init__(self, force=None):
        self.table, self.recording, self.force = {}, True, dict(force or {})

    def __call__(self, name, value, limit):
        if self.recording:
            assert value.dtype == np.float64, (name, value.dtype)
            forced = [v for k, v in self.force.items() if name.endswith(k)]
            assert name not in self.table, name
            self.table[name] = np.full(value.shape, forced[0], dtype=bool) if forced else np.abs(value) <= limit
        assert self.table[name].shape == value.shape, name
        return self.table[name]


# ---------------------------------------------------------------------------
# SE(3) / SE(2): a transform is (R (n, m, m), t (n, m)), m = 3 or 2; a tangent vector (n, D) = [rho | phi]
# ---------------------------------------------------------------------------
def unpack(rows, dof, dtype):
    m = 3 if dof == 6 else 2
    rows = np.asarray(rows).astype(dtype).reshape(-1, m * m + m)
    return _is(dtype, rows[:, :m * m].reshape(-1, m, m).copy(), rows[:, m * m:].copy())


def pack(T):
    R, t = T
    return np.concatenate([R.reshape(R.shape[0], -1), t], axis=1)


def mul(A, B):
    dtype = A[0].dtype
    _is(dtype, A[1], B[0], B[1])
    return _is(dtype, np.einsum('nij,njk->nik', A[0], B[0]), np.einsum('nij,nj->ni', A[0], B[1]) + A[1])


def inv(A):
    Rt = np.transpose(A[0], (0, 2, 1))
    return _is(A[0].dtype, Rt, -np.einsum('nij,nj->ni', Rt, A[1]))


def wedge(v):
    out = np.zeros((v.shape[0], 3, 3), dtype=v.dtype)
    out[:, 0, 1], out[:, 0, 2] = -v[:, 2], v[:, 1]
    out[:, 1, 0], out[:, 1, 2] = v[:, 2], -v[:, 0]
    out[:, 2, 0], out[:, 2, 1] = -v[:, 1], v[:, 0]
    return out


def _eye(m, dtype):
    return np.identity(m, dtype=dtype)


def _one_minus_cos(a, c):
    """1 - cos(a) as the definition writes it (fp64: the twin carries fp64's own cancellation, 2^-53 / a^2 relative, as numpy and
    the device do); in long double the same number from 2 sin^2(a / 2): the reference is there to approximate the formula's exact value,
    and 1 - c would leave it 2^-64 / a^2 -- 5e-4 of the term at 1e-8."""
    if a.dtype == np.float64:
        return 1 - c
    h = np.sin(0.5 * a)
    return 2 * h * h


def log(T, pred, name):
    """(n, D) = [J_l^-1(phi) t | phi]."""
    R, t = T
    dtype = R.dtype
    _is(dtype, t)
    with np.errstate(divide='ignore', invalid='ignore'):
        if R.shape[1] == 3:
            ca = np.clip(0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]) - 0.5, -1, 1)
            ang = _is(dtype, np.arccos(ca))
            small = pred(name + '/log_angle', ang, SMALL)
            # (ang == 0 in the large branch: the band where fp64 resolves an angle and the long-double trace clips to 1 -- the
            # pose's entries are rounded, its trace can exceed 3; ang / sin(ang) takes its limit there)
            f = np.where(small, 0, np.where(ang == 0, 0.5, 0.5 * ang / np.sin(ang)))
            big = f[:, None] * np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
            tiny = np.stack([R[:, 2, 1], R[:, 0, 2], R[:, 1, 0]], axis=1)                   # vee(R - I)
            phi = _is(dtype, np.where(small[:, None], tiny, big))
            a = _is(dtype, np.sqrt(phi[:, 0] * phi[:, 0] + phi[:, 1] * phi[:, 1] + phi[:, 2] * phi[:, 2]))
            small = pred(name + '/log_phi', a, SMALL)
            safe = np.where(small, 1, a)
            ax = phi / safe[:, None]
            half = 0.5 * safe
            hc = half / np.tan(half)
            at = ax[:, 0] * t[:, 0] + ax[:, 1] * t[:, 1] + ax[:, 2] * t[:, 2]
            big = hc[:, None] * t + ((1 - hc) * at)[:, None] * ax - half[:, None] * np.cross(ax, t)
            tiny = t - 0.5 * np.cross(phi, t)
            rho = np.where(small[:, None], tiny, big)
            return _is(dtype, np.concatenate([rho, phi], axis=1))
        phi = _is(dtype, np.arctan2(R[:, 1, 0], R[:, 0, 0]))
        small = pred(name + '/log_phi', phi, SMALL)
        half = 0.5 * np.where(small, 1, phi)
        a = np.where(small, 1, half / np.tan(half))
        b = np.where(small, 0.5 * phi, half)
        rho = np.stack([a * t[:, 0] + b * t[:, 1], -b * t[:, 0] + a * t[:, 1]], axis=1)
        return _is(dtype, np.concatenate([rho, phi[:, None]], axis=1))


def exp(xi, pred, name):
    """T = (exp(phi^), J_l(phi) rho)."""
    dtype = xi.dtype
    with np.errstate(divide='ignore', invalid='ignore'):
        if xi.shape[1] == 6:
            rho, phi = xi[:, :3], xi[:, 3:]
            a = np.sqrt(phi[:, 0] * phi[:, 0] + phi[:, 1] * phi[:, 1] + phi[:, 2] * phi[:, 2])
            small = pred(name + '/exp_phi', a, SMALL)
            safe = np.where(small, 1, a)
            ax = phi / safe[:, None]
            s, c = np.sin(safe), np.cos(safe)
            outer = ax[:, :, None] * ax[:, None, :]
            omc = _one_minus_cos(safe, c)
            Rb = c[:, None, None] * _eye(3, dtype) + omc[:, None, None] * outer + s[:, None, None] * wedge(ax)
            sa, ca = s / safe, omc / safe
            ar = ax[:, 0] * rho[:, 0] + ax[:, 1] * rho[:, 1] + ax[:, 2] * rho[:, 2]
            tb = sa[:, None] * rho + ((1 - sa) * ar)[:, None] * ax + ca[:, None] * np.cross(ax, rho)
            R = np.where(small[:, None, None], _eye(3, dtype) + wedge(phi), Rb)
            t = np.where(small[:, None], rho + 0.5 * np.cross(phi, rho), tb)
            return _is(dtype, R, t)
        rho, phi = xi[:, :2], xi[:, 2]
        c, s = np.cos(phi), np.sin(phi)
        R = np.stack([np.stack([c, -s], 1), np.stack([s, c], 1)], 1)
        small = pred(name + '/exp_phi', phi, SMALL)
        safe = np.where(small, 1, phi)
        a = np.where(small, 1, s / safe)
        b = np.where(small, 0.5 * phi, _one_minus_cos(safe, np.cos(safe)) / safe)
        t = np.stack([a * rho[:, 0] - b * rho[:, 1], b * rho[:, 0] + a * rho[:, 1]], axis=1)
        return _is(dtype, R, t)


def Ad(T):
    R, t = T
    dtype, n = R.dtype, R.shape[0]
    if R.shape[1] == 3:
        out = np.zeros((n, 6, 6), dtype=dtype)
        out[:, :3, :3] = R
        out[:, :3, 3:] = np.einsum('nij,njk->nik', wedge(t), R)
        out[:, 3:, 3:] = R
        return out
    out = np.tile(_eye(3, dtype), (n, 1, 1))
    out[:, :2, :2] = R
    out[:, 0, 2], out[:, 1, 2] = t[:, 1], -t[:, 0]
    return _is(dtype, out)


# ---------------------------------------------------------------------------
# losses (reference pyslam/losses.py), by id; k and x in one dtype
# ---------------------------------------------------------------------------
def loss_rho(lid, k, x, pred, name):
    dtype = x.dtype
    k, a = dtype.type(k), np.abs(x)
    if lid == L2:
        out = 0.5 * x * x
    elif lid == L1:
        out = a
    elif lid == CAUCHY:
        out = (0.5 * k * k) * np.log(1 + (x / k) * (x / k))
    elif lid == HUBER:
        out = np.where(pred(name + '/inside_k', x, float(k)), 0.5 * x * x, k * (a - 0.5 * k))
    elif lid == TUKEY:
        c, q = k * k / 6, x / k
        out = np.where(pred(name + '/inside_k', x, float(k)), c * (1 - (1 - q * q) ** 3), c)
    elif lid == TDIST:
        out = 0.5 * (k + 1) * np.log(1 + x * x / k)
    else:
        raise ValueError(lid)
    return _is(dtype, out)


def loss_weight(lid, k, x, pred, name):
    dtype = x.dtype
    k, a = dtype.type(k), np.abs(x)
    with np.errstate(divide='ignore', invalid='ignore'):
        if lid == L2:
            out = np.ones_like(x)
        elif lid == L1:
            out = np.where(pred(name + '/l1_zero', x, SMALL), np.nan, 1 / a)
        elif lid == CAUCHY:
            out = 1 / (1 + (x / k) * (x / k))
        elif lid == HUBER:
            out = np.where(pred(name + '/inside_k', x, float(k)), 1, k / a)
        elif lid == TUKEY:
            out = np.where(pred(name + '/inside_k', x, float(k)), 1 - (x / k) * (x / k), 0)
        elif lid == TDIST:
            out = (k + 1) / (k + x * x)
        else:
            raise ValueError(lid)
    return _is(dtype, out.astype(dtype))


# ---------------------------------------------------------------------------
# the factors of a problem
# ---------------------------------------------------------------------------
def factor_tables(lp):
    """(i (F,) with -1 for a prior, j, group, T_obs^-1 rows): edges, then priors -- the device's numbering."""
    E, Q = lp.num_edges, lp.num_priors
    i = np.concatenate([lp.e_i, np.full(Q, -1)]).astype(np.int64)
    j = np.concatenate([lp.e_j, lp.u_i]).astype(np.int64)
    grp = np.concatenate([lp.e_grp, lp.u_grp]).astype(np.int64)
    w = lp.pose_width
    Tinv = np.concatenate([lp.e_Tobs_inv.reshape(E, w), lp.u_Tobs_inv.reshape(Q, w)])
    return i, j, grp, Tinv


def factor_scale(lp):
    """u (F,): the rounding scale of a factor's rows -- the infinity norm of its stiffness times max(1, the largest |t| among
    T_1, T_2, T_obs): the size of the numbers whose rounded products the row was formed from."""
    d = lp.dof
    i, j, grp, Tinv = factor_tables(lp)
    m = 3 if d == 6 else 2
    tt = lambda rows: np.abs(np.asarray(rows, dtype=float)[:, m * m:]).max(axis=1)             # noqa: E731
    Ro, to = unpack(Tinv, d, np.float64)
    tobs = np.abs(inv((Ro, to))[1]).max(axis=1) if len(i) else np.zeros(0)
    t2 = tt(lp.poses[j])
    t1 = np.where(i >= 0, tt(lp.poses[np.maximum(i, 0)]), 0.)
    S = lp.stiffd[lp.edge_groups[grp, 0].astype(int)].reshape(-1, d, d)
    return np.abs(S).sum(axis=2).max(axis=1) * np.maximum(1., np.maximum(np.maximum(t1, t2), tobs))


class Factors:
    """Every factor of `lp` evaluated in `dtype` (fields (F, ...) in the device's order, all of `dtype`): xi = log(E), r, s, rt = r~,
    J1 = J~_1, J2 = J~_2; and, fp64 decisions: small_angle / small_phi (the branches of log), present (F, D) stiffness rows.
    `force`: Predicates' -- e.g. {'log_angle': True} puts every factor into vee(R - I)."""

    def __init__(self, lp, dtype=np.longdouble, force=None):
        dtype = np.dtype(dtype)
        self.lp, self.dtype, self.pred = lp, dtype, Predicates(force)
        self._evaluate(np.dtype(np.float64))
        if dtype != np.float64:
            self.pred.recording = False
            self._evaluate(dtype)

    def _evaluate(self, dtype):
        lp, d, pred = self.lp, self.lp.dof, self.pred
        i, j, grp, Tinv = factor_tables(lp)
        self.i, self.j, self.grp, self.F = i, j, grp, len(i)
        binary = i >= 0
        poses = unpack(lp.poses, d, dtype)
        take = lambda T, idx: (T[0][idx], T[1][idx])                                   # noqa: E731
        T2, To = take(poses, j), unpack(Tinv, d, dtype)
        T1i = inv(take(poses, np.maximum(i, 0)))
        Eb = mul(T2, mul(T1i, To))                         # T_2 (T_1^-1 T_obs^-1)
        Eu = mul(T2, To)
        sel = lambda a, b: np.where(binary.reshape((-1,) + (1,) * (a.ndim - 1)), a, b)      # noqa: E731
        E = (sel(Eb[0], Eu[0]), sel(Eb[1], Eu[1]))
        T21 = mul(T2, T1i)
        xi = log(E, pred, 'factor')
        self.small_angle = pred.table.get('factor/log_angle', np.zeros(self.F, dtype=bool))
        self.small_phi = pred.table['factor/log_phi'] if self.F else np.zeros(0, dtype=bool)
        gid = lp.edge_groups[grp, 0].astype(int)
        S = _is(dtype, lp.stiffd.astype(dtype)[gid].reshape(-1, d, d))
        r = _is(dtype, np.einsum('nij,nj->ni', S, xi))
        self.present = np.any(lp.stiffd[gid].reshape(-1, d, d) != 0., axis=2)
        s = np.zeros_like(r)
        for g in np.unique(grp):
            m = grp == g
            lid, k = int(lp.edge_groups[g, 1]), lp.edge_groups[g, 2]
            w = loss_weight(lid, k, r[m], pred, 'group{}'.format(g))
            s[m] = np.where(self.present[m], np.sqrt(np.where(self.present[m], w, 0)), 0)
        rho = np.zeros_like(r)
        for g in np.unique(grp):
            m = grp == g
            rho[m] = loss_rho(int(lp.edge_groups[g, 1]), lp.edge_groups[g, 2], r[m], pred, 'cost/group{}'.format(g))
        self.rho = _is(dtype, rho)
        _is(dtype, s)
        self.loss = lp.edge_groups[grp, 1].astype(int)
        J2 = s[:, :, None] * S
        J1 = -s[:, :, None] * np.einsum('nij,njk->nik', S, Ad(T21))
        J1[~binary] = 0
        self.xi, self.r, self.s, self.rt, self.J1, self.J2, self.S = _is(dtype, xi, r, s, s * r, J1, J2, S)

    # ---- per factor ------------------------------------------------------
    def blocks(self):
        """(H11, H12, H22 (F, D, D), g1, g2 (F, D)): J~^T J~ and -J~^T r~ of every factor."""
        J1, J2, rt = self.J1, self.J2, self.rt
        out = (np.einsum('nki,nkj->nij', J1, J1), np.einsum('nki,nkj->nij', J1, J2), np.einsum('nki,nkj->nij', J2, J2),
               -np.einsum('nki,nk->ni', J1, rt), -np.einsum('nki,nk->ni', J2, rt))
        return _is(self.dtype, *out)

    def assemble(self, lam=0.):
        """(S (D nr, D nr), g (D nr,), touched (nr, nr) bool) in device order: the factor part alone, (1 + lambda) on its diagonal
        entries.  A constant end contributes nothing; a factor with no variable end is in no block."""
        lp, d, dtype = self.lp, self.lp.dof, self.dtype
        nr = lp.num_reduced
        H11, H12, H22, g1, g2 = self.blocks()
        rid = lp.pose_rid.astype(np.int64)
        ri, rj = np.where(self.i >= 0, rid[np.maximum(self.i, 0)], -1), rid[self.j]
        Sb = np.zeros((nr, nr, d, d), dtype=dtype)
        g = np.zeros((nr, d), dtype=dtype)
        vi, vj = ri >= 0, rj >= 0
        np.add.at(Sb, (ri[vi], ri[vi]), H11[vi])
        np.add.at(Sb, (rj[vj], rj[vj]), H22[vj])
        both = vi & vj
        np.add.at(Sb, (ri[both], rj[both]), H12[both])
        np.add.at(Sb, (rj[both], ri[both]), np.transpose(H12[both], (0, 2, 1)))
        np.add.at(g, ri[vi], g1[vi])
        np.add.at(g, rj[vj], g2[vj])
        k = np.arange(nr)
        Sb[k[:, None], k[:, None], np.arange(d)[None, :], np.arange(d)[None, :]] *= dtype.type(1) + dtype.type(lam)
        touched = np.zeros((nr, nr), dtype=bool)
        touched[ri[vi], ri[vi]] = True
        touched[rj[vj], rj[vj]] = True
        touched[ri[both], rj[both]] = True
        touched[rj[both], ri[both]] = True
        return _is(dtype, Sb.transpose(0, 2, 1, 3).reshape(d * nr, d * nr), g.reshape(-1)) + (touched,)

    def active(self):
        """Factors with a variable end: those of eval_cost(False) and of the blocks."""
        rid = self.lp.pose_rid
        return (rid[self.j] >= 0) | ((self.i >= 0) & (rid[np.maximum(self.i, 0)] >= 0))

    def costs(self):
        """(sum of rho(r_k) over every factor, over those with a variable end), as floats."""
        per = self.rho.sum(axis=1)
        return float(per.sum()), float(per[self.active()].sum())


def retract(lp, dx_pose, step=1., dtype=np.longdouble, force=None):
    """poses (P, W) in `dtype` after T_i <- exp(step dx_i) T_i for the variable poses (dx_pose (nr, D), by rid); constant poses
    unchanged.  The product step dx_i is formed in `dtype`."""
    dtype = np.dtype(dtype)
    d = lp.dof
    pred = Predicates(force)
    var = np.flatnonzero(lp.pose_rid >= 0)
    out = None
    for dt in ([np.dtype(np.float64)] if dtype == np.float64 else [np.dtype(np.float64), dtype]):
        pred.recording = dt == np.float64
        xi = _is(dt, dt.type(step) * np.asarray(dx_pose).astype(dt)[lp.pose_rid[var]].reshape(-1, d))
        T = unpack(lp.poses[var], d, dt)
        out = lp.poses.astype(dt)
        out[var] = pack(mul(exp(xi, pred, 'retract'), T))
    return _is(dtype, out), pred.table.get('retract/exp_phi', np.zeros(0, dtype=bool))


def in_branch(lp):
    """(small_angle, small_phi) per factor from the fp64 predicate alone."""
    f = Factors(lp, np.float64)
    return f.small_angle, f.small_phi


def one_ulp_away(lp, draw):
    """The problem with every entry of poses, e_Tobs_inv and u_Tobs_inv moved by -1, 0 or +1 ulp (seeded by `draw`): another input
    of the same conditioning on which to SAMPLE the fp64 evaluation error -- its fp64 result against its OWN long-double result,
    never against the unmoved problem's (the meaning of longdouble_schur.one_ulp_away)."""
    rng = np.random.default_rng([draw, 21])
    out = lp.copy()
    for name in ('poses', 'e_Tobs_inv', 'u_Tobs_inv'):
        a = getattr(lp, name)
        setattr(out, name, np.nextafter(a, a + rng.integers(-1, 2, size=a.shape) * np.abs(a)))
    return out


# ---------------------------------------------------------------------------
# the measure: per row, over max(the row's own largest reference entry, the row's rounding scale)
# ---------------------------------------------------------------------------
def row_err(got, ref, floor):
    """max over rows of (largest |got - ref| in the row) / max(largest |ref| in the row, floor of the row).  The first axis numbers
    the rows; differences are formed in the reference's dtype.  inf on a non-finite entry."""
    ref = np.asarray(ref)
    if ref.shape[0] == 0:
        return 0.
    ref = ref.reshape(ref.shape[0], -1)
    got = np.asarray(got).reshape(ref.shape).astype(ref.dtype)
    floor = np.broadcast_to(np.asarray(floor, dtype=float), (ref.shape[0],))
    assert np.all(floor > 0)
    diff = np.abs(got - ref).max(axis=1)
    if not np.all(np.isfinite(diff)):
        return float('inf')
    return float((diff / np.maximum(np.abs(ref).max(axis=1), floor.astype(ref.dtype))).max())


def cut_blocks(S, d):
    n = np.asarray(S).shape[0] // d
    return np.asarray(S).reshape(n, d, n, d).transpose(0, 2, 1, 3).reshape(n * n, d * d)


def system_floors(fac, extra_S=None, extra_g=None):
    """(floor per D x D block of S (nr nr,), floor per D-vector of g (nr,)) from a REFERENCE evaluation `fac`: a block's entries are
    sums of products of two J~ entries, each exact to about 2^-53 of its factor's rounding scale u, so the block's scale is the largest
    u_f max|J~_f| among the factors that touch it (never below the square of the smallest u: a block nothing touches keeps a
    positive floor and must be exactly zero anyway); g's is the largest u_f max|J~_f| as well -- what an absolute error of 2^-53 u_f
    in r~ (a row that is all cancellation) becomes in J~^T r~."""
    lp = fac.lp
    nr = lp.num_reduced
    u = factor_scale(lp)
    jmax = np.maximum(np.abs(fac.J1).reshape(fac.F, -1).max(axis=1), np.abs(fac.J2).reshape(fac.F, -1).max(axis=1)).astype(float)
    w = u * np.maximum(jmax, u)
    rid = lp.pose_rid.astype(np.int64)
    ri, rj = np.where(fac.i >= 0, rid[np.maximum(fac.i, 0)], -1), rid[fac.j]
    fS = np.full((nr, nr), float(u.min()) ** 2 if fac.F else 1.)
    fg = np.full(nr, float(u.min()) ** 2 if fac.F else 1.)
    for a, b in ((ri, ri), (rj, rj), (ri, rj), (rj, ri)):
        ok = (a >= 0) & (b >= 0)
        np.maximum.at(fS, (a[ok], b[ok]), w[ok])
    for a in (ri, rj):
        np.maximum.at(fg, a[a >= 0], w[a >= 0])
    if extra_S is not None:
        fS = np.maximum(fS, extra_S)
    if extra_g is not None:
        fg = np.maximum(fg, extra_g)
    return fS.reshape(-1), fg
