"""Scenes of the pose-factor tests (tests/test_posegraph_host.py, tests/test_gpu_posegraph.py), each built from a WANTED error
transform: T_2 = exp(xi_E) T_obs T_1 with T_1 and T_obs random (formed in long double, rounded to fp64), so that the error rotation,
the size of the translations and the side of every loss's k are what the scene says -- outside synthetic.pose_graph's helix (0.02 of
start noise, 0.01 of measurement noise, one loss, edges i < j, one prior).  Every scene is generated from a seed; none has more than
about 260 factors.  scene(name, dof) -> (LoweredProblem, info dict); built once, callers leave the tables unchanged.

  angles      one factor per |phi_E| of ANGLES (0 exactly, 1e-10 .. 3.1), as an edge and as a prior; SE(2): both signs, +-3.1, +-(pi - 1e-3)
  near_pi     3.13, 3.14, 3.1415 (SE(3)): fp64 itself loses digits as 2^-53 / (pi - theta)^2 there
  km, mm      `angles` with the translations of T_1, T_obs and rho_E times 1e3 and 1e-3
  rot_only    edges whose stiffness has zero translation rows (lowering.py's orientation loops in SE(3); the tables and the kernel
              template admit them in SE(2) as well; T_obs translation zero) and priors with |t_E| <= 1e-6, so that phi is the row
  mixed_wg    129 factors (the handle numbers edges before priors: 40 edges + 89 priors, so workgroup 0 and its third wave hold
              both kinds); seven groups rotating factor by factor -- the six losses at ids 0 .. 5 and one at the last row of a
              300-row group table (ps_abi_problem.h: create_pose_factors admits any id below num_edge_groups, an int32: no byte
              limit as for observation groups) -- full random stiffnesses, residuals on both sides of every k
  tails<nf>   nf = 1, 15, 16, 17, 48, 63, 64, 65, 129, 257 edges: the wave's 16-factor share and the 64-factor workgroup, each with
              its tail; a chain first, then random pairs, every third reversed (sim3graph_scenes.chain_pairs); two groups alternate
  dup, const_middle, const_pair, star70, prior_every, priors_only      the `structure` scenes
  exact       every measurement consistent, under L2, Huber, Cauchy and Tukey
  mixed_ba    (SE(3)) offbox_scenes' `base` plus odometry edges -- one between keyframes that share no landmark, one reversed, one
              from the held keyframe -- and a prior on a variable pose
  cg_size     20 variable SE(3) poses: 120 unknowns, past k_direct_solve's 90"""
import functools

import numpy as np

import longdouble_posegraph as ldp
from pyslam_amd.lowering import LoweredProblem

LD = np.dtype(np.longdouble)
# (3e-7 is an addition to the list the scenes were specified with: a factor between the band and 1e-6, so that a small branch taken too
# far is seen whatever acos makes of the factor at 1e-6 itself)
# The seeds of angles / km / mm are chosen so that, of the four factors between 1e-8 and 3e-8, the fp64 predicate puts some into
# vee(R - I) and some into the logarithm (which side a factor at 1.2e-8 falls is decided by the rounding of its poses' entries):
# tests/test_posegraph_host.py asserts it.
ANGLES = (0., 1e-10, 5e-9, 0.9e-8, 1.2e-8, 1.6e-8, 3e-8, 3e-7, 1e-6, 1e-3, 0.3, 1., 2., 3.0, 3.1)
NEAR_PI = (3.13, 3.14, 3.1415)
SE2_EXTRA = (3.1, -3.1, np.pi - 1e-3, -(np.pi - 1e-3))
TAILS = (1, 15, 16, 17, 48, 63, 64, 65, 129, 257)
TAIL_SCENES = tuple('tails{}'.format(n) for n in TAILS)
STRUCTURE_SCENES = ('dup', 'const_middle', 'const_pair', 'star70', 'prior_every', 'priors_only')
SCENES_BOTH = ('angles', 'km', 'mm', 'rot_only', 'mixed_wg') + TAIL_SCENES + STRUCTURE_SCENES + ('exact',)
SCENES_SE3_ONLY = ('near_pi', 'mixed_ba', 'cg_size')
HIGH_GROUP_ROWS = 300
DUP = [(0, 1), (1, 2), (2, 1), (1, 2), (0, 3), (3, 2), (1, 2)]          # sim3graph_scenes' `dup`, for these tables


def cases():
    """Every (scene, dof)."""
    return [(n, d) for n in SCENES_BOTH for d in (6, 3)] + [(n, 6) for n in SCENES_SE3_ONLY]


# ---------------------------------------------------------------------------
# long-double group arithmetic for the builders
# ---------------------------------------------------------------------------
def _exp(xi):
    """exp of fp64 tangent rows in long double (the branch by the fp64 value, as the definition has it)."""
    xi = np.atleast_2d(np.asarray(xi, dtype=float))
    pred = ldp.Predicates()
    ldp.exp(xi, pred, 'build')
    pred.recording = False
    return ldp.exp(xi.astype(LD), pred, 'build')


def _rows(T):
    return ldp.pack(T).astype(np.float64)


def _tangent(rng, dof, angle, tscale, rho=1.):
    """[rho | phi] with |phi| = |angle| (SE(2): phi = angle, signed), rho ~ N(0, (rho tscale)^2)."""
    if dof == 6:
        d = rng.standard_normal(3)
        return np.hstack([rho * tscale * rng.standard_normal(3), angle * d / np.linalg.norm(d)])
    return np.hstack([rho * tscale * rng.standard_normal(2), angle])


def _random_pose(rng, dof, tscale):
    ang = 0.8 * rng.standard_normal(3) if dof == 6 else rng.uniform(-3., 3., 1)
    return _exp(np.hstack([2. * tscale * rng.standard_normal(dof // 3 + 1), ang]))


def _ld(rows, dof):
    return ldp.unpack(np.atleast_2d(rows), dof, LD)


class Builder:
    def __init__(self, dof, seed):
        self.dof, self.rng = dof, np.random.default_rng([seed, dof, 33])
        self.poses, self.held, self.edges, self.priors = [], [], [], []
        self.stiff, self.groups = [], []

    def group(self, S, loss_id, k):
        self.stiff.append(np.asarray(S, dtype=float).reshape(-1))
        self.groups.append([len(self.stiff) - 1, loss_id, k])
        return len(self.groups) - 1

    def pose(self, T, held=False):
        self.poses.append(_rows(T)[0])
        self.held.append(held)
        return len(self.poses) - 1

    def random_pose(self, tscale=1., held=False):
        return self.pose(_random_pose(self.rng, self.dof, tscale), held)

    def T(self, i):
        return _ld(self.poses[i], self.dof)

    def edge_with_error(self, i, j, xi_E, grp):
        """An edge (i, j) between EXISTING poses whose error transform is exp(xi_E): T_obs^-1 = T_i T_j^-1 exp(xi_E)."""
        Tinv = ldp.mul(self.T(i), ldp.mul(ldp.inv(self.T(j)), _exp(xi_E)))
        self.edges.append((i, j, _rows(Tinv)[0], grp))

    def prior_with_error(self, j, xi_E, grp):
        Tinv = ldp.mul(ldp.inv(self.T(j)), _exp(xi_E))
        self.priors.append((j, _rows(Tinv)[0], grp))

    def measured_pose(self, i, xi_E, grp, tscale=1., zero_tobs=False, exact=False):
        """A NEW pose T_2 = exp(xi_E) T_obs T_1 behind pose i (None: a prior, T_2 = exp(xi_E) T_obs) with T_obs random; `exact`:
        the product T_obs T_1 itself, not exponentiated."""
        To = _random_pose(self.rng, self.dof, tscale)
        if zero_tobs:
            To = (To[0], np.zeros_like(To[1]))
        To = _ld(_rows(To), self.dof)                                          # (the fp64 T_obs is the measurement)
        base = To if i is None else ldp.mul(To, self.T(i))
        j = self.pose(base if exact else ldp.mul(_exp(xi_E), base))
        if i is None:
            self.priors.append((j, _rows(ldp.inv(To))[0], grp))
        else:
            self.edges.append((i, j, _rows(ldp.inv(To))[0], grp))
        return j

    def lp(self, group_rows=None):
        d = self.dof
        groups, stiff = np.array(self.groups, dtype=float), np.stack(self.stiff)
        if group_rows is not None:                                  # the last group at the last row of a longer table
            table = np.tile(groups[0], (group_rows, 1))
            table[:len(groups) - 1] = groups[:-1]
            table[-1] = groups[-1]
            remap = np.arange(len(groups))
            remap[-1] = group_rows - 1
            groups = table
        else:
            remap = np.arange(len(groups))
        held = np.array(self.held, dtype=bool)
        rid = np.where(held, -1, np.cumsum(~held) - 1).astype(np.int32)
        w = 12 if d == 6 else 6
        out = LoweredProblem(dof=d, poses=np.stack(self.poses), pose_rid=rid, stiffd=stiff, edge_groups=groups)
        if self.edges:
            out.e_i, out.e_j = [e[0] for e in self.edges], [e[1] for e in self.edges]
            out.e_Tobs_inv = np.stack([e[2] for e in self.edges]).reshape(-1, w)
            out.e_grp = remap[[e[3] for e in self.edges]]
        if self.priors:
            out.u_i = [u[0] for u in self.priors]
            out.u_Tobs_inv = np.stack([u[1] for u in self.priors]).reshape(-1, w)
            out.u_grp = remap[[u[2] for u in self.priors]]
        return out.finalize()


def _near_identity(rng, d, scale=1.):
    return scale * (np.identity(d) * rng.uniform(0.5, 2., d) + 0.1 * rng.standard_normal((d, d)))


# ---------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------
def _angles(dof, angles, tscale, seed):
    b = Builder(dof, seed)
    g = b.group(np.identity(dof), ldp.L2, 0.)
    if dof == 3:
        angles = [s * a for a in angles for s in ((1.,) if a == 0. else (1., -1.))] + list(SE2_EXTRA)
    wanted = []
    for a in angles:
        # a prior with the angle on a new pose, then an edge with the angle from that pose to another new one
        i = b.measured_pose(None, _tangent(b.rng, dof, a, tscale, 0.1), g, tscale, exact=a == 0.)
        b.measured_pose(i, _tangent(b.rng, dof, -a if dof == 6 else a, tscale, 0.1), g, tscale, exact=a == 0.)
        wanted.append(a)
    wanted = np.array(wanted + wanted)                                  # edges first, then priors
    return b.lp(), dict(angle=wanted)


def _rot_only(dof, seed):
    """Per angle: a tight prior on a new pose, a rotation-only edge to another new pose, a tight prior on that one."""
    m = dof // 3 + 1                                           # translation rows: 3 or 2
    b = Builder(dof, seed)
    Sd = np.zeros((dof, dof))
    Sd[m:, m:] = 31.6 * np.identity(dof - m)
    edge_groups = [b.group(Sd, ldp.L2, 0.), b.group(Sd, ldp.HUBER, 0.5), b.group(Sd, ldp.CAUCHY, 0.5), b.group(Sd, ldp.L1, 0.)]
    tight = b.group(np.identity(dof), ldp.L2, 0.)
    angles = list(ANGLES)
    if dof == 3:
        angles = [sg * a for a in ANGLES for sg in ((1.,) if a == 0. else (1., -1.))] + list(SE2_EXTRA)
    wanted = []
    for k, a in enumerate(angles):
        tiny = np.hstack([1e-6 * b.rng.uniform(-1., 1., m), np.zeros(dof - m)])
        i = b.measured_pose(None, _tangent(b.rng, dof, a, 1., 0.) + tiny, tight, zero_tobs=True, exact=a == 0.)
        # L1 only where no component of the row comes near zero (its weight there is NaN by definition): 0.3 and 1 rad
        grp = edge_groups[3] if abs(a) in (0.3, 1.) else edge_groups[k % 3]
        j = b.measured_pose(i, _tangent(b.rng, dof, a, 1.), grp, zero_tobs=True, exact=a == 0.)
        b.prior_with_error(j, _tangent(b.rng, dof, a, 1., 0.) + tiny, tight)
        wanted.append(a)
    return b.lp(), dict(angle=np.array(wanted + [a for a in wanted for _ in (0, 1)]))


MIXED_WG_EDGES, MIXED_WG_PRIORS, MIXED_WG_POSES = 40, 89, 30
MIXED_WG_LOSSES = ((ldp.L2, 0.), (ldp.L1, 0.), (ldp.CAUCHY, 0.3), (ldp.HUBER, 0.3), (ldp.TUKEY, 0.45), (ldp.TDIST, 3.), (ldp.HUBER, 0.2))
MIXED_WG_NOISE = 0.3


def _mixed_wg(dof, seed):
    """`noise = k`: the residual components are N(0, 0.3^2) pushed through a stiffness near the identity, k = 0.2 .. 0.45."""
    b = Builder(dof, seed)
    grp = [b.group(_near_identity(b.rng, dof), lid, k) for lid, k in MIXED_WG_LOSSES]
    for _ in range(MIXED_WG_POSES):
        b.random_pose()
    n = 0
    for e in range(MIXED_WG_EDGES):
        i, j = b.rng.choice(MIXED_WG_POSES, 2, replace=False)
        b.edge_with_error(int(i), int(j), MIXED_WG_NOISE * b.rng.standard_normal(dof), grp[n % 7])
        n += 1
    for u in range(MIXED_WG_PRIORS):
        b.prior_with_error(u % MIXED_WG_POSES, MIXED_WG_NOISE * b.rng.standard_normal(dof), grp[n % 7])
        n += 1
    lp = b.lp(HIGH_GROUP_ROWS)
    ref = ldp.Factors(lp, LD)
    l1 = ref.loss == ldp.L1
    assert np.abs(ref.r[l1]).min() > 1e-6, 'an L1 residual component within 1e-6 of zero: its weight is NaN by definition'
    return lp, {}


def _graph(dof, seed, num_poses, pairs, held, groups, noise=0.3, priors=(), prior_group=None):
    """Random poses, edges `pairs` with error exp(N(0, noise^2)), their groups rotating; priors on `priors`."""
    b = Builder(dof, seed)
    grp = [b.group(*g) if g[0] is not None else b.group(_near_identity(b.rng, dof), g[1], g[2]) for g in groups]
    for p in range(num_poses):
        b.random_pose(held=p in held)
    for k, (i, j) in enumerate(pairs):
        b.edge_with_error(i, j, noise * b.rng.standard_normal(dof), grp[k % len(grp)])
    pg = grp[0] if prior_group is None else b.group(*prior_group)
    for p in priors:
        b.prior_with_error(p, noise * b.rng.standard_normal(dof), pg)
    return b.lp(), {}


def _tails(dof, nf):
    from sim3graph_scenes import chain_pairs
    N = min(nf + 1, 20)                                     # (every pose on the chain: the reduced system is definite)
    return _graph(dof, 100 + nf, N, chain_pairs(nf, N), (0,), [(None, ldp.HUBER, 0.3), (np.identity(dof), ldp.L2, 0.)])


def _structure(name, dof):
    I = np.identity(dof)
    two = [(None, ldp.HUBER, 0.3), (I, ldp.L2, 0.)]
    if name == 'dup':
        return _graph(dof, 41, 4, DUP, (0,), two)
    if name == 'const_middle':
        return _graph(dof, 42, 5, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)], (2,), two, priors=(0,))
    if name == 'const_pair':       # two constant poses joined by an edge, in both directions
        return _graph(dof, 43, 6, [(0, 3), (3, 0), (0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 1)], (0, 3), two)
    if name == 'star70':
        star = [(0, k) if k % 2 else (k, 0) for k in range(1, 71)] + [(70, 71)]
        return _graph(dof, 44, 72, star, (71,), two)
    if name == 'prior_every':
        return _graph(dof, 45, 6, [(k, k + 1) for k in range(5)], (), two, priors=range(6), prior_group=(2. * I, ldp.CAUCHY, 0.3))
    if name == 'priors_only':
        return _graph(dof, 46, 5, [], (), two, priors=(0, 1, 2, 3, 4, 2))
    raise KeyError(name)


EXACT_LOSSES = ((ldp.L2, 0.), (ldp.HUBER, 0.3), (ldp.CAUCHY, 0.3), (ldp.TUKEY, 0.3))


def _exact(dof):
    pairs = [(k, k + 1) for k in range(7)] + [(0, 4), (6, 2), (7, 1), (3, 7), (5, 0)]
    return _graph(dof, 47, 8, pairs, (), [(None, lid, k) for lid, k in EXACT_LOSSES], noise=0., priors=(0, 5))


def _cg_size():
    rng = np.random.default_rng(48)
    pairs = [(k, k + 1) for k in range(19)] + [(int(i), int(j)) for i, j in
                                                (rng.choice(20, 2, replace=False) for _ in range(15))]
    return _graph(6, 48, 20, pairs, (), [(None, ldp.HUBER, 0.1), (np.identity(6), ldp.L2, 0.)], noise=0.05, priors=(0,),
                  prior_group=(10. * np.identity(6), ldp.L2, 0.))


# offbox_scenes.GPU_SHAPE with a window of three keyframes instead of nine: keyframes four apart share no landmark
MIXED_BA_SHAPE = dict(num_kf=9, num_lm=300, obs_per_lm=3, half_window=1, seed=3)


def _mixed_ba():
    import offbox_scenes as osc
    base, _ = osc.scene('base', MIXED_BA_SHAPE)
    P = base.num_poses
    shares = np.zeros((P, P), dtype=bool)
    for lm in range(base.num_points):
        kf = base.obs_pose[base.obs_point == lm]
        shares[np.ix_(kf, kf)] = True
    var = np.flatnonzero(base.pose_rid >= 0)
    apart = [(int(a), int(c)) for a in var for c in var if a < c and not shares[a, c]]
    assert apart, 'every pair of keyframes shares a landmark'
    factor_only = apart[-1]
    chain = [(k, k + 1) for k in range(P - 1)]                     # (0, 1) starts at the held keyframe
    assert all(shares[a, c] for a, c in chain)
    reversed_edge = (3, 2)
    b = Builder(6, 49)
    b.poses, b.held = [row for row in base.poses], list(base.pose_rid < 0)
    odo = b.group(31.6 * np.identity(6), ldp.HUBER, 1.)
    loop = b.group(_near_identity(b.rng, 6, 10.), ldp.L2, 0.)
    for i, j in chain + [reversed_edge]:
        b.edge_with_error(i, j, 0.02 * b.rng.standard_normal(6), odo)
    b.edge_with_error(factor_only[0], factor_only[1], 0.02 * b.rng.standard_normal(6), loop)
    prior_pose = int(var[2])
    b.prior_with_error(prior_pose, 0.02 * b.rng.standard_normal(6), loop)
    fac = b.lp()
    out = base.copy()
    for name in ('e_i', 'e_j', 'e_Tobs_inv', 'e_grp', 'u_i', 'u_Tobs_inv', 'u_grp', 'stiffd', 'edge_groups'):
        setattr(out, name, getattr(fac, name))
    return out.finalize(), dict(factor_only=factor_only, shared=chain[1], reversed=reversed_edge, prior=prior_pose)


@functools.lru_cache(maxsize=None)
def scene(name, dof=6):
    if name == 'angles':
        return _angles(dof, ANGLES, 1., 1)
    if name == 'near_pi':
        return _angles(6, NEAR_PI, 1., 2)
    if name == 'km':
        return _angles(dof, ANGLES, 1e3, 7)
    if name == 'mm':
        return _angles(dof, ANGLES, 1e-3, 4)
    if name == 'rot_only':
        return _rot_only(dof, 5)
    if name == 'mixed_wg':
        return _mixed_wg(dof, 6)
    if name in TAIL_SCENES:
        return _tails(dof, int(name[5:]))
    if name in STRUCTURE_SCENES:
        return _structure(name, dof)
    if name == 'exact':
        return _exact(dof)
    if name == 'mixed_ba':
        return _mixed_ba()
    if name == 'cg_size':
        return _cg_size()
    raise KeyError(name)


def error_rotation(lp):
    """|phi| of every factor's error transform (edges, then priors), from the long-double evaluation."""
    f = ldp.Factors(lp, LD)
    return np.sqrt((f.xi[:, lp.dof // 3 + 1:] ** 2).sum(axis=1)).astype(float)


# ---------------------------------------------------------------------------
# references and e64: once per scene, shared by the host and the device tests, never written to
# ---------------------------------------------------------------------------
DRAWS = 8           # copies of a scene one ulp away on which the fp64 error is sampled as well (tests/test_gpu_offbox.py)
LAMBDAS = (0., 1e-3)
FACTOR = 8          # bound = max(floor, FACTOR e64): tests/test_gpu_offbox.py, tests/test_gpu_bchol_kernels.py


def one_ulp(lp, draw):
    out = ldp.one_ulp_away(lp, draw)
    if lp.num_obs:
        import longdouble_schur as lds
        q = lds.one_ulp_away(lp, draw)
        out.points, out.obs_uvd = q.points, q.obs_uvd
    return out


@functools.lru_cache(maxsize=None)
def problems(name, dof=6):
    """The scene and DRAWS copies of it with every input one ulp away."""
    lp = scene(name, dof)[0]
    return [lp] + [one_ulp(lp, k) for k in range(DRAWS)]


@functools.lru_cache(maxsize=None)
def factor_pairs(name, dof=6):
    """Per problem of problems(): (its factors in long double, in fp64) -- like for like, the same input on both sides."""
    return [(ldp.Factors(q, LD), ldp.Factors(q, np.float64)) for q in problems(name, dof)]


def _system(fac, lam):
    """(S, g, touched) of the whole problem in fac's dtype: the factor part plus, with observations, the landmark elimination's."""
    S, g, touched = fac.assemble(lam)
    lp = fac.lp
    if lp.num_obs:
        import longdouble_schur as lds
        el = lds.Elimination(lp, lam, fac.dtype.type)
        nr = lp.num_reduced
        touched = touched | (np.abs(ldp.cut_blocks(el.S, 6)).max(axis=1) > 0).reshape(nr, nr)
        S, g = S + el.S, g + el.g
    return ldp._is(fac.dtype, S, g) + (touched,)


@functools.lru_cache(maxsize=None)
def system_pairs(name, dof, lam):
    return [(_system(r, lam), _system(t, lam)) for r, t in factor_pairs(name, dof)]


def err_rows(got, ref, lp):
    return ldp.row_err(got, ref, ldp.factor_scale(lp))


def err_system(got, ref, fac):
    """(per D x D block of S, per D-vector of g) against `ref` = (S, g, ...), floors from the reference factors `fac`."""
    d = fac.lp.dof
    fS, fg = ldp.system_floors(fac)
    return (ldp.row_err(ldp.cut_blocks(got[0], d), ldp.cut_blocks(ref[0], d), fS),
            ldp.row_err(np.asarray(got[1]).reshape(-1, d), np.asarray(ref[1]).reshape(-1, d), fg))


def err_cost(got, ref):
    return max(abs(a - b) / max(abs(b), 1e-300) if b else abs(a) for a, b in zip(got, ref))


@functools.lru_cache(maxsize=None)
def e64(name, dof=6):
    """The largest distance of the fp64 twin from the long-double twin ON THE SAME INPUT over the scene and its DRAWS copies, per
    quantity, in the tests' measure: 'rt', 'J1', 'J2', ('S', lam), ('g', lam), 'cost'."""
    out = {}
    pairs = factor_pairs(name, dof)
    for what in ('rt', 'J1', 'J2'):
        out[what] = max(err_rows(getattr(t, what), getattr(r, what), r.lp) for r, t in pairs)
    out['cost'] = max(err_cost(t.costs(), r.costs()) for r, t in pairs)
    for lam in LAMBDAS:
        errs = [err_system(st, sr, r) for (r, _), (sr, st) in zip(pairs, system_pairs(name, dof, lam))]
        out['S', lam], out['g', lam] = max(e[0] for e in errs), max(e[1] for e in errs)
    return out


def e64_retract(name, dof, dx, step=1.):
    """e64 of the retraction exp(step dx_i) T_i at the given step table, over the same nine problems."""
    worst = 0.
    for q in problems(name, dof):
        ref, _ = ldp.retract(q, dx, step, LD)
        twin, _ = ldp.retract(q, dx, step, np.float64)
        worst = max(worst, ldp.row_err(twin, ref, pose_floor(q)))
    return worst


def pose_floor(lp):
    m = 3 if lp.dof == 6 else 2
    return np.maximum(1., np.abs(lp.poses[:, m * m:]).max(axis=1))


def bound(e, floor=1e-12):
    return max(floor, FACTOR * e)
