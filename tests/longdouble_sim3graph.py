"""The Sim(3) pose-graph definition restated in numpy long double (x87 extended: 64-bit mantissa): the reference
tests/test_sim3graph_rows_host.py and tests/test_gpu_sim3graph_rows.py measure the device and the fp64 restatement against.  Written
apart from pyslam_amd/liegroups/sim3.py and pyslam_amd/pipelines/simgraph.py -- nothing of either is called -- and vectorised over
edges (16 448 edges cost about a second).  Every intermediate asserts its dtype.

A similarity is (R (n, 3, 3), t (n, 3), s (n,)), p -> s R p + t, a row of 13 numbers [R | t | s]; a tangent vector (n, 7) =
[rho | phi | sigma].  exp(xi) = (Exp(phi), W(phi, sigma) rho, e^sigma), W = A I + B phi^ + C phi^^2 with, for z = sigma + i theta
and f(z) = (e^z - 1) / z: A = f(sigma), B = Im f / theta, C = (A - Re f) / theta^2.  An edge (i, j, S_ji, K), K the 7 x 7
stiffness:

    r = K log(S_j S_i^-1 S_ji^-1),   J_i = -K Ad(S_j S_i^-1),   J_j = K,   s_k = sqrt(w(r_k)),   r~ = s r,   J~ = diag(s) J

an all-zero stiffness row being an ABSENT row (scale 0, no cost).  H = sum J~^T J~, g = -sum J~^T r~ over the free vertices,
cost = sum rho(r_k), by plain sums; retraction S <- exp(dx) S.  L1's weight in this graph is 1 / max(|r_k|, 1e-8).

dtype=np.float64 runs the same code in fp64: the twin whose distance from the long-double result on the same input is fp64's
own rounding error (e64).

BRANCHES belong to the definition that is checked: `sn <= 1e-8` (the logarithm's small branch), `theta <= 1e-8` (h1, h2),
`|z|^2 <= 1` (series or closed forms of A, B, C: both are accurate, the twin follows the device), the losses' `|x| <= k` and L1's
`|x| <= 1e-8`.  Both passes take the branch the FP64 value selects (class Predicates: the fp64 evaluation runs first and records,
the long-double one replays).

Long-double pitfalls: 1 - cos(theta) is 2 sin^2(theta / 2) everywhere.  A, B, C of the REFERENCE come from the power series alone,
carried in pairs of long doubles (w_series_pairs: about 128 bits, rounded once) -- in plain long double the alternating series loses
two to three bits for sigma < 0 and the closed form's A - E h1 three more near theta = 1, and 4 x 2^-64 is asked
(tests/test_sim3graph_rows_host.py, against mpmath at 50 digits).  The fp64 twin keeps the device's two branches."""
import numpy as np

LONGDOUBLE_OK = np.finfo(np.longdouble).eps < 1e-18
LONGDOUBLE_SKIP = 'np.longdouble is no wider than 1e-18 here (eps {:.1e}): no reference better than fp64'.format(
    float(np.finfo(np.longdouble).eps))
LD = np.dtype(np.longdouble)
F64 = np.dtype(np.float64)

SMALL = 1e-8                       # TINY_ANGLE of sim3.py, PS_S3G_TINY / PS_SMALL_ANGLE of the device
L2, L1, CAUCHY, HUBER, TUKEY, TDIST = range(6)
LOSS_NAMES = ('L2', 'L1', 'Cauchy', 'Huber', 'Tukey', 'TDist')
SERIES_TERMS = {F64: 22}
EPS = 2. ** -53


def _is(dtype, *arrays):
    for a in arrays:
        assert a.dtype == dtype, (a.dtype, dtype)
    return arrays[0] if len(arrays) == 1 else arrays


class Predicates:
    """Branch decisions by name.  Recording (the fp64 pass): `abs(value) <= limit` on an fp64 value, unless `force` names the
    predicate (True / False: every element into that branch).  Replaying (the long-double pass): the recorded decision."""

    def __init__(self, force=None):
        self.table, self.recording, self.force = {}, True, dict(force or {})

    def __call__(self, name, value, limit):
        if self.recording:
            assert value.dtype == F64, (name, value.dtype)
            forced = [v for k, v in self.force.items() if name.endswith(k)]
            assert name not in self.table, name
            self.table[name] = np.full(value.shape, forced[0], dtype=bool) if forced else np.abs(value) <= limit
        assert self.table[name].shape == value.shape, name
        return self.table[name]


def two_pass(fn, dtype, force=None):
    """fn(dtype, pred) evaluated in fp64 (recording the predicates) and then, unless fp64 was asked for, in `dtype` (replaying
    them) -> (result, predicate table)."""
    dtype, pred = np.dtype(dtype), Predicates(force)
    out = fn(F64, pred)
    if dtype != F64:
        pred.recording = False
        out = fn(dtype, pred)
    return out, pred.table


# ---------------------------------------------------------------------------
# the group
# ---------------------------------------------------------------------------
def unpack(rows, dtype):
    rows = np.asarray(rows).astype(dtype).reshape(-1, 13)
    return _is(np.dtype(dtype), rows[:, :9].reshape(-1, 3, 3).copy(), rows[:, 9:12].copy(), rows[:, 12].copy())


def pack(S):
    return np.concatenate([S[0].reshape(-1, 9), S[1], S[2][:, None]], axis=1)


def take(S, idx):
    return S[0][idx], S[1][idx], S[2][idx]


def mul(A, B):
    dtype = A[0].dtype
    _is(dtype, A[1], A[2], B[0], B[1], B[2])
    return _is(dtype, np.einsum('nij,njk->nik', A[0], B[0]), A[2][:, None] * np.einsum('nij,nj->ni', A[0], B[1]) + A[1], A[2] * B[2])


def inv(A):
    Rt = np.transpose(A[0], (0, 2, 1))
    return _is(A[0].dtype, Rt, -np.einsum('nij,nj->ni', Rt, A[1]) / A[2][:, None], 1 / A[2])


def wedge(v):
    out = np.zeros((v.shape[0], 3, 3), dtype=v.dtype)
    out[:, 0, 1], out[:, 0, 2] = -v[:, 2], v[:, 1]
    out[:, 1, 0], out[:, 1, 2] = v[:, 2], -v[:, 0]
    out[:, 2, 0], out[:, 2, 1] = -v[:, 1], v[:, 0]
    return out


def _norm3(v):
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def h12(theta, pred, name):
    """sin(theta) / theta and (1 - cos(theta)) / theta^2 = (sin(theta / 2) / (theta / 2))^2 / 2; 1 and 1 / 2 up to 1e-8."""
    dtype = theta.dtype
    small = pred(name + '/h12', theta, SMALL)
    safe = np.where(small, 1, theta)
    half = safe / 2
    sh = np.sin(half) / half
    return _is(dtype, np.where(small, 1, np.sin(safe) / safe).astype(dtype), np.where(small, 0.5, sh * sh / 2).astype(dtype))


def w_series(theta, sigma):
    """(A, B, C) from sum_n z^n / (n + 1)!: a_n = Re z^n, p_n = Im z^n / theta, q_n = (sigma^n - Re z^n) / theta^2."""
    dtype = theta.dtype
    th2 = theta * theta
    one, zero = np.ones_like(theta), np.zeros_like(theta)
    a, p, q, sn, inv_fact = one, zero, zero, one, dtype.type(1)
    A, B, C = one, zero, zero
    for n in range(1, SERIES_TERMS[dtype] + 1):
        p, q = sigma * p + a, sigma * q + p
        sn = sn * sigma
        a = sn - th2 * q
        inv_fact = inv_fact / dtype.type(n + 1)
        A, B, C = A + sn * inv_fact, B + p * inv_fact, C + q * inv_fact
    return _is(dtype, A, B, C)


def w_closed(theta, sigma, pred, name):
    """The closed forms: B = (sigma (E h1 - A) + E theta^2 h2) / |z|^2, C = (sigma E h2 + A - E h1) / |z|^2, E = e^sigma,
    A = expm1(sigma) / sigma."""
    dtype = theta.dtype
    th2 = theta * theta
    E = np.exp(sigma)
    zero = sigma == 0
    A = np.where(zero, 1, np.expm1(sigma) / np.where(zero, 1, sigma)).astype(dtype)
    h1, h2 = h12(theta, pred, name + '/closed')
    z2 = sigma * sigma + th2
    z2 = np.where(z2 == 0, 1, z2)
    return _is(dtype, A, (sigma * (E * h1 - A) + E * th2 * h2) / z2, (sigma * E * h2 + A - E * h1) / z2)


# ---- pairs of long doubles (hi, lo), hi + lo carrying about 128 bits: the reference's series cancels nothing that matters ----
_SPLIT = np.longdouble(2) ** 32 + 1


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca, cb = _SPLIT * a, _SPLIT * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_add(x, y):
    s, e = _two_sum(x[0], y[0])
    t, f = _two_sum(x[1], y[1])
    s, e = _two_sum(s, e + t)
    return _two_sum(s, e + f)


def _dd_mul(x, y):
    p, e = _two_prod(x[0], y[0])
    return _two_sum(p, e + (x[0] * y[1] + x[1] * y[0]))


def w_series_pairs(theta, sigma):
    """(A, B, C) in long double from the series of w_series carried in pairs of long doubles: a sum that alternates (sigma < 0, or
    theta beyond 1) loses its leading bits from a 128-bit number and is rounded to long double once, at the end.  As many terms as
    |z|^n / (n + 1)! needs to fall below 1e-45 of e^|z| at the largest |z| of the table (|z| <= 21 asked: 150 terms at most)."""
    _is(LD, theta, sigma)
    zmax = float(np.sqrt((sigma * sigma + theta * theta).max())) if theta.size else 0.
    assert zmax <= 21., zmax
    terms, t = 0, 1.
    while terms < 24 or t > 1e-45:
        terms += 1
        t *= max(zmax, 1e-3) / (terms + 1)
    zero, one = np.zeros_like(theta), np.ones_like(theta)
    dd = lambda v: (v, zero)                                                                    # noqa: E731
    sg, mth2 = dd(sigma), tuple(-v for v in _two_prod(theta, theta))
    a, p, q, sn, inv_fact = dd(one), dd(zero), dd(zero), dd(one), dd(one)
    A, B, C = dd(one), dd(zero), dd(zero)
    for n in range(1, terms + 1):
        p, q = _dd_add(_dd_mul(sg, p), a), _dd_add(_dd_mul(sg, q), p)
        sn = _dd_mul(sn, sg)
        a = _dd_add(sn, _dd_mul(mth2, q))
        # 1 / (n + 1)! as a pair: the quotient and one Newton correction of it
        d = LD.type(n + 1)
        hi = inv_fact[0] / d
        ph, pl = _two_prod(hi, d * one)
        inv_fact = _two_sum(hi, ((inv_fact[0] - ph) - pl + inv_fact[1]) / d)
        A, B, C = _dd_add(A, _dd_mul(sn, inv_fact)), _dd_add(B, _dd_mul(p, inv_fact)), _dd_add(C, _dd_mul(q, inv_fact))
    return _is(LD, A[0] + A[1], B[0] + B[1], C[0] + C[1])


def w_coefficients(theta, sigma, pred, name):
    """(A, B, C).  fp64, the twin: the series inside |z|^2 <= 1, the closed forms outside, as the device has them.  Long double, the
    reference: the series in pairs of long doubles everywhere (w_series_pairs: in plain long double the alternating series loses
    two to three bits for sigma < 0, and the closed form's A - E h1 three more near theta = 1), except where theta <= 1e-8 outside the
    circle: there the closed form with h1 = 1, h2 = 1 / 2 IS the definition, and is kept."""
    dtype = theta.dtype
    _is(dtype, sigma)
    z2 = sigma * sigma + theta * theta
    inside = pred(name + '/w_series', z2.astype(F64), 1.0)
    if dtype == F64:
        clo = w_closed(np.where(inside, 2, theta).astype(dtype), np.where(inside, 0, sigma).astype(dtype), pred, name)
        ser = w_series(np.where(inside, theta, 0), np.where(inside, sigma, 0))
        return _is(dtype, *[np.where(inside, s, c) for s, c in zip(ser, clo)])
    closed = ~inside & pred.table[name + '/closed/h12']
    A, B, C = w_series_pairs(np.where(closed, 0, theta).astype(dtype), sigma)
    # closed: (A, B0, C0) at theta = 0.  With h1 = 1, h2 = 1 / 2 the closed forms are B = (sigma (E - A) + E theta^2 / 2) / |z|^2 and
    # C = (sigma E / 2 + A - E) / |z|^2; by sigma B0 = E - A and 2 B0 + 2 sigma C0 = E (the derivatives of sigma f = e^sigma - 1)
    # the same numbers without a difference:
    z2 = np.where(closed, z2, 1)
    Bc, Cc = (sigma * sigma * B + np.exp(sigma) * theta * theta / 2) / z2, sigma * sigma * C / z2
    return _is(dtype, A, np.where(closed, Bc, B), np.where(closed, Cc, C))


def w_matrix(phi, sigma, pred, name):
    dtype = phi.dtype
    A, B, C = w_coefficients(_norm3(phi), sigma, pred, name)
    K = wedge(phi)
    return _is(dtype, A[:, None, None] * np.identity(3, dtype=dtype) + B[:, None, None] * K
               + C[:, None, None] * np.einsum('nij,njk->nik', K, K))


def exp(xi, pred, name):
    dtype = xi.dtype
    rho, phi, sigma = xi[:, 0:3], xi[:, 3:6], xi[:, 6]
    h1, h2 = h12(_norm3(phi), pred, name + '/exp')
    K = wedge(phi)
    R = np.identity(3, dtype=dtype) + h1[:, None, None] * K + h2[:, None, None] * np.einsum('nij,njk->nik', K, K)
    t = np.einsum('nij,nj->ni', w_matrix(phi, sigma, pred, name + '/exp'), rho)
    return _is(dtype, R, t, np.exp(sigma))


def inv3(M):
    """The inverse of (n, 3, 3) by cross products of its columns."""
    c0, c1, c2 = M[:, :, 0], M[:, :, 1], M[:, :, 2]
    r0, r1, r2 = np.cross(c1, c2), np.cross(c2, c0), np.cross(c0, c1)
    det = (c0 * r0).sum(axis=1)
    return _is(M.dtype, np.stack([r0, r1, r2], axis=1) / det[:, None, None])


def log(S, pred, name):
    """(n, 7) = [W^-1 t | phi | log s], rotation angles below pi."""
    R, t, s = S
    dtype = R.dtype
    v = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    sn = _norm3(v) / 2
    cs = (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]) / 2 - dtype.type(0.5)
    small = pred(name + '/log_small', sn, SMALL)
    f = np.where(small, 0.5, np.arctan2(sn, cs) / np.where(small, 1, sn) / 2).astype(dtype)
    phi = f[:, None] * v
    sigma = np.log(s)
    rho = np.einsum('nij,nj->ni', inv3(w_matrix(phi, sigma, pred, name + '/log')), t)
    return _is(dtype, np.concatenate([rho, phi, sigma[:, None]], axis=1))


def Ad(S):
    R, t, s = S
    out = np.zeros((R.shape[0], 7, 7), dtype=R.dtype)
    out[:, 0:3, 0:3] = s[:, None, None] * R
    out[:, 0:3, 3:6] = np.einsum('nij,njk->nik', wedge(t), R)
    out[:, 0:3, 6] = -t
    out[:, 3:6, 3:6] = R
    out[:, 6, 6] = 1
    return _is(R.dtype, out)


# ---------------------------------------------------------------------------
# losses, by id; per component
# ---------------------------------------------------------------------------
def loss_rho(lid, k, x, pred, name):
    dtype = x.dtype
    a = np.abs(x)
    k = dtype.type(k)
    if lid == L2:
        out = x * x / 2
    elif lid == L1:
        out = a
    elif lid == CAUCHY:
        out = (k * k / 2) * np.log(1 + (x / k) * (x / k))
    elif lid == HUBER:
        out = np.where(pred(name + '/inside_k', x, float(k)), x * x / 2, k * (a - k / 2))
    elif lid == TUKEY:
        c, q = k * k / 6, x / k
        out = np.where(pred(name + '/inside_k', x, float(k)), c * (1 - (1 - q * q) ** 3), c)
    elif lid == TDIST:
        out = ((k + 1) / 2) * np.log(1 + x * x / k)
    else:
        raise ValueError(lid)
    return _is(dtype, out.astype(dtype))


def loss_weight(lid, k, x, pred, name):
    """The IRLS weight; L1: 1 / max(|x|, 1e-8), this graph's rule."""
    dtype = x.dtype
    a = np.abs(x)
    k = dtype.type(k)
    if lid == L2:
        out = np.ones_like(x)
    elif lid == L1:
        capped = pred(name + '/l1_zero', x, SMALL)
        out = 1 / np.where(capped, dtype.type(SMALL), a)
    elif lid == CAUCHY:
        out = 1 / (1 + (x / k) * (x / k))
    elif lid == HUBER:
        out = np.where(pred(name + '/inside_k', x, float(k)), 1, k / np.where(a == 0, 1, a))
    elif lid == TUKEY:
        out = np.where(pred(name + '/inside_k', x, float(k)), 1 - (x / k) * (x / k), 0)
    elif lid == TDIST:
        out = (k + 1) / (k + x * x)
    else:
        raise ValueError(lid)
    return _is(dtype, out.astype(dtype))


# ---------------------------------------------------------------------------
# a graph given as the device's tables, and its edges
# ---------------------------------------------------------------------------
class Graph:
    """vertices (N, 13), held (N,), edge_i, edge_j (E,), measurements (E, 13), stiffness (E, 7, 7) or None, loss id and k."""

    def __init__(self, V13, held, ei, ej, obs13, stiffness=None, loss_id=L2, loss_k=0.):
        self.V13 = np.ascontiguousarray(V13, dtype=np.float64).reshape(-1, 13)
        self.held = np.asarray(held, dtype=bool).reshape(self.V13.shape[0])
        self.ei, self.ej = np.asarray(ei, dtype=np.int64).ravel(), np.asarray(ej, dtype=np.int64).ravel()
        self.obs13 = np.ascontiguousarray(obs13, dtype=np.float64).reshape(-1, 13)
        self.E = self.ei.size
        self.stiffness = None if stiffness is None else np.ascontiguousarray(stiffness, dtype=np.float64).reshape(self.E, 7, 7)
        self.loss_id, self.loss_k = int(loss_id), float(loss_k)
        self.rid = np.full(self.V13.shape[0], -1, dtype=np.int64)
        self.rid[~self.held] = np.arange(int((~self.held).sum()))
        self.nfree = int((~self.held).sum())

    def K(self):
        return np.tile(np.identity(7), (self.E, 1, 1)) if self.stiffness is None else self.stiffness

    def with_vertices(self, V13):
        return Graph(V13, self.held, self.ei, self.ej, self.obs13, self.stiffness, self.loss_id, self.loss_k)

    def device_args(self):
        return self.V13, self.held, self.ei.astype(np.int32), self.ej.astype(np.int32), self.obs13, self.stiffness


def edge_scale(g):
    """u (E,): the rounding scale of an edge's rows -- the infinity norm of its stiffness times the largest magnitude among the
    summands that form the error transform's translation through S_j S_i^-1 S_ji^-1 (t_j; (s_j / s_i) t_i; (s_j / (s_i s_ji)) t_ji),
    floored at 1.  One rounding of a row is 2^-53 u."""
    V, O = g.V13, g.obs13
    tmax = lambda rows: np.abs(rows[:, 9:12]).max(axis=1)                                     # noqa: E731
    ratio = V[g.ej, 12] / V[g.ei, 12]
    m = np.maximum(np.maximum(tmax(V[g.ej]), ratio * tmax(V[g.ei])), ratio / O[:, 12] * tmax(O))
    return np.abs(g.K()).sum(axis=2).max(axis=1) * np.maximum(1., m)


class Edges:
    """Every edge of `g` evaluated in `dtype` (fields (E, ...), all of `dtype`): xi = log(E), r, s, rho (per component, 0 on an absent
    row), rt = r~, J1 = J~_i, J2 = J~_j; fp64 decisions: small (the logarithm's branch), series (|z|^2 <= 1 inside the logarithm),
    inside_k, present.  `force`: Predicates' -- {'log_small': True} puts every edge into the small branch."""

    def __init__(self, g, dtype=LD, force=None):
        self.g, self.dtype = g, np.dtype(dtype)
        _, self.table = two_pass(self._evaluate, dtype, force)

    def _evaluate(self, dtype, pred):
        g = self.g
        V = unpack(g.V13, dtype)
        T21 = mul(take(V, g.ej), inv(take(V, g.ei)))
        Err = mul(T21, inv(unpack(g.obs13, dtype)))
        xi = log(Err, pred, 'edge')
        K = _is(dtype, g.K().astype(dtype))
        self.present = np.any(g.K() != 0., axis=2)
        r = _is(dtype, np.einsum('nij,nj->ni', K, xi))
        w = loss_weight(g.loss_id, g.loss_k, r, pred, 'weight')
        s = np.where(self.present, np.sqrt(np.where(self.present, w, 0)), 0).astype(dtype)
        rho = np.where(self.present, loss_rho(g.loss_id, g.loss_k, r, pred, 'rho'), 0).astype(dtype)
        J2 = s[:, :, None] * K
        J1 = -s[:, :, None] * np.einsum('nij,njk->nik', K, Ad(T21))
        self.xi, self.r, self.s, self.rho, self.rt, self.J1, self.J2 = _is(dtype, xi, r, s, rho, s * r, J1, J2)
        self.small = pred.table['edge/log_small']
        self.series = pred.table['edge/log/w_series']
        self.inside_k = pred.table.get('weight/inside_k')
        self.l1_capped = pred.table.get('weight/l1_zero')
        return self

    def blocks(self):
        J1, J2, rt = self.J1, self.J2, self.rt
        return _is(self.dtype, np.einsum('nki,nkj->nij', J1, J1), np.einsum('nki,nkj->nij', J1, J2), np.einsum('nki,nkj->nij', J2, J2),
                   -np.einsum('nki,nk->ni', J1, rt), -np.einsum('nki,nk->ni', J2, rt))

    def assemble(self, lam=0.):
        """(H (7 nf, 7 nf) with (1 + lambda) on its diagonal, g (7 nf,), touched (nf, nf) bool) over the free vertices."""
        g, dtype, nf = self.g, self.dtype, self.g.nfree
        H11, H12, H22, g1, g2 = self.blocks()
        ri, rj = g.rid[g.ei], g.rid[g.ej]
        Hb, gv = np.zeros((nf, nf, 7, 7), dtype=dtype), np.zeros((nf, 7), dtype=dtype)
        vi, vj = ri >= 0, rj >= 0
        both = vi & vj
        np.add.at(Hb, (ri[vi], ri[vi]), H11[vi])
        np.add.at(Hb, (rj[vj], rj[vj]), H22[vj])
        np.add.at(Hb, (ri[both], rj[both]), H12[both])
        np.add.at(Hb, (rj[both], ri[both]), np.transpose(H12[both], (0, 2, 1)))
        np.add.at(gv, ri[vi], g1[vi])
        np.add.at(gv, rj[vj], g2[vj])
        k, d = np.arange(nf), np.arange(7)
        Hb[k[:, None], k[:, None], d[None, :], d[None, :]] *= dtype.type(1) + dtype.type(lam)
        touched = np.zeros((nf, nf), dtype=bool)
        touched[ri[vi], ri[vi]] = True
        touched[rj[vj], rj[vj]] = True
        touched[ri[both], rj[both]] = True
        touched[rj[both], ri[both]] = True
        return _is(dtype, Hb.transpose(0, 2, 1, 3).reshape(7 * nf, 7 * nf), gv.reshape(-1)) + (touched,)

    def cost(self):
        return float(self.rho.sum())


def retract(g, dx, dtype=LD, force=None):
    """vertices (N, 13) in `dtype` after S_v <- exp(dx_rid) S_v for the free vertices (dx (nf, 7) fp64); held ones unchanged."""
    free = np.flatnonzero(~g.held)

    def run(dt, pred):
        xi = _is(dt, np.asarray(dx, dtype=np.float64).reshape(-1, 7).astype(dt))
        out = g.V13.astype(dt)
        out[free] = pack(mul(exp(xi, pred, 'retract'), unpack(g.V13[free], dt)))
        return _is(dt, out)
    return two_pass(run, dtype, force)


def explog(xi, dtype=LD):
    """(exp(xi) rows (n, 13), log(exp(xi)) (n, 7), Ad(exp(xi)) (n, 7, 7)) in `dtype`; the logarithm is taken of the `dtype` value."""
    def run(dt, pred):
        S = exp(np.asarray(xi, dtype=np.float64).reshape(-1, 7).astype(dt), pred, 'x')
        return pack(S), log(S, pred, 'l'), Ad(S)
    return two_pass(run, dtype)[0]


def one_ulp_away(g, draw):
    """The graph with every entry of the vertices and measurements moved by -1, 0 or +1 ulp (seeded by `draw`): another input of the
    same conditioning on which to SAMPLE the fp64 evaluation error -- its fp64 result against its OWN long-double result."""
    rng = np.random.default_rng([draw, 23])
    move = lambda a: np.nextafter(a, a + rng.integers(-1, 2, size=a.shape) * np.abs(a))       # noqa: E731
    return Graph(move(g.V13), g.held, g.ei, g.ej, move(g.obs13), g.stiffness, g.loss_id, g.loss_k)


def accurate_solve(H, g):
    """H^-1 g of a long-double system: a Jacobi-scaled fp64 factorisation refined with long-double residuals (the arbiter of
    tests/test_gpu_parity.py, on the unrounded system)."""
    H, g = np.asarray(H, dtype=LD), np.asarray(g, dtype=LD)
    d = 1 / np.sqrt(np.diag(H))
    Hs, gs = H * d[:, None] * d[None, :], g * d
    import scipy.linalg as sla
    fac = sla.cho_factor(Hs.astype(np.float64))
    x = np.zeros_like(gs)
    for _ in range(4):
        x = x + sla.cho_solve(fac, (gs - Hs @ x).astype(np.float64)).astype(LD)
    return _is(LD, x * d)


# ---------------------------------------------------------------------------
# the measure: per row, over max(the row's own largest reference entry, the row's rounding scale)
# ---------------------------------------------------------------------------
def row_errs(got, ref, floor):
    """Per row: (largest |got - ref| in the row) / max(largest |ref| in the row, floor of the row); inf on a non-finite entry."""
    ref = np.asarray(ref)
    ref = ref.reshape(ref.shape[0], -1)
    got = np.asarray(got).reshape(ref.shape).astype(ref.dtype)
    floor = np.broadcast_to(np.asarray(floor, dtype=float), (ref.shape[0],))
    assert np.all(floor > 0)
    diff = np.abs(got - ref).max(axis=1) if ref.shape[0] else np.zeros(0)
    out = (diff / np.maximum(np.abs(ref).max(axis=1), floor.astype(ref.dtype))).astype(float)
    out[~np.isfinite(diff.astype(float))] = np.inf
    return out


def row_err(got, ref, floor):
    e = row_errs(got, ref, floor)
    return float(e.max()) if e.size else 0.


def cut_blocks(H):
    n = np.asarray(H).shape[0] // 7
    return np.asarray(H).reshape(n, 7, n, 7).transpose(0, 2, 1, 3).reshape(n * n, 49)


def system_floors(ed):
    """(floor per 7 x 7 block of H (nf nf,), per 7-vector of g (nf,)) from a REFERENCE evaluation: the largest u_e max(|J~_e|, u_e)
    among the edges that touch it (a block nothing touches keeps a positive floor and must be exactly zero anyway)."""
    g = ed.g
    nf, u = g.nfree, edge_scale(g)
    jmax = np.maximum(np.abs(ed.J1).reshape(g.E, -1).max(axis=1), np.abs(ed.J2).reshape(g.E, -1).max(axis=1)).astype(float) \
        if g.E else np.zeros(0)
    w = u * np.maximum(jmax, u)
    ri, rj = g.rid[g.ei], g.rid[g.ej]
    base = float(u.min()) ** 2 if g.E else 1.
    fH, fg = np.full((nf, nf), base), np.full(nf, base)
    for a, b in ((ri, ri), (rj, rj), (ri, rj), (rj, ri)):
        ok = (a >= 0) & (b >= 0)
        np.maximum.at(fH, (a[ok], b[ok]), w[ok])
    for a in (ri, rj):
        np.maximum.at(fg, a[a >= 0], w[a >= 0])
    return fH.reshape(-1), fg


def err_system(got, ref, ed):
    fH, fg = system_floors(ed)
    return (row_err(cut_blocks(got[0]), cut_blocks(ref[0]), fH), row_err(np.asarray(got[1]).reshape(-1, 7), np.asarray(ref[1]).reshape(-1, 7), fg))


def vertex_floor(V13):
    return np.ones(np.asarray(V13).shape[0])
