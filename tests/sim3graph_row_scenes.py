"""Scenes of the per-row Sim(3) pose-graph tests (tests/test_sim3graph_rows_host.py, tests/test_gpu_sim3graph_rows.py), built from a
WANTED error transform: a scene picks S_i, S_ji and a tangent vector xi and sets S_j = exp(xi) S_ji S_i, so that the residual -- and
with it the branch of the logarithm, the branch of W's coefficients and the side of a loss's k -- is chosen and not drawn.  Where both
ends of an edge are already given (chords, duplicates, reversed and held-ended edges, vertices of a prescribed scale) the
measurement is set instead, S_ji = exp(-xi) S_j S_i^-1: the same error transform.  The products are formed in long double
(tests/longdouble_sim3graph.py) and rounded once, so the achieved error is xi to a rounding of the scene's numbers.

Rotation angles within 1e-8 of pi are outside the documented domain of the logarithm (liegroups/sim3.py: "rotation angles below
pi"; at pi - theta < 1e-8 the logarithm's small branch, made for angles near ZERO, answers) and are not asked for: 3.1415 is the
largest angle here.

Every scene is (Graph, info); `scene(name)` caches.  e64(name): the fp64 twin against the long-double pass on the same input, over
the scene and DRAWS one-ulp copies, in the tests' measure, per quantity and per (loss, branch) class for the rows."""
import functools

import numpy as np

import longdouble_sim3graph as ld
import sim3graph_scenes as gs

LD = ld.LD
DRAWS = 8
FACTOR = 8
TOL_ROW, TOL_COST, TOL_DX = 1e-12, 1e-10, 1e-8
LAMBDAS = (0., 1e-3)
K_LOSS = 0.3
ANGLES = (0., 1e-10, 0.9e-8, 1.1e-8, 3e-7, 1e-5, 1e-3, 0.3, 1., 2.5, 3.1, 3.1415)
SIGMAS = (0., 1e-9, -1e-9, 1e-3, -1e-3, 0.3, -0.3, 0.999, -0.999, 1.001, -1.001, 1.2, -1.2, 3., -3.)
SCALE_ANGLES = (0., 1e-9, 0.5, 1.2)
STIFFNESS_KINDS = ('identity', 'rotation_only', 'scale_only', 'translation_only', 'diagonal')
WG64_ABSENT = (0, 15, 16, 47, 63)

BARE_ANGLES = (1e-10, 0.9e-8, 1.1e-8, 3e-7, 9e-7, 1e-5, 1e-3, 0.3)

ROW_SCENES = ('angles', 'bare', 'scales', 'km', 'mm', 'map_scales', 'exact', 'wg64', 'E65', 'many_edges', 'hang257', 'noisy_loop') + \
    tuple('rows-{}-{}'.format(ld.LOSS_NAMES[l], 'identity') for l in range(6)) + \
    tuple('rows-{}-{}'.format(ld.LOSS_NAMES[l], k) for l in (ld.L2, ld.HUBER, ld.TUKEY, ld.L1) for k in STIFFNESS_KINDS[1:]) + ('l1_zero',)
STEP_SCENES = ('angles', 'bare', 'scales', 'km', 'mm', 'map_scales', 'exact', 'wg64', 'E65', 'many_edges', 'hang257', 'noisy_loop', 'l1_zero') + \
    tuple('rows-{}-identity'.format(ld.LOSS_NAMES[l]) for l in range(6)) + \
    tuple('rows-{}-diagonal'.format(ld.LOSS_NAMES[l]) for l in (ld.L2, ld.HUBER, ld.TUKEY, ld.L1)) + ('rows-L2-translation_only',)


# ---------------------------------------------------------------------------
# building blocks (long double, rounded once)
# ---------------------------------------------------------------------------
def _ld(fn):
    return ld.two_pass(fn, LD)[0]


def exp13(xi):
    return ld.pack(_ld(lambda dt, p: ld.exp(np.atleast_2d(xi).astype(dt), p, 'x'))).astype(np.float64)


def end_vertex(Si, Sji, xi):
    """S_j = exp(xi) S_ji S_i, rows (n, 13)."""
    return ld.pack(_ld(lambda dt, p: ld.mul(ld.exp(np.atleast_2d(xi).astype(dt), p, 'x'),
                                            ld.mul(ld.unpack(Sji, dt), ld.unpack(Si, dt))))).astype(np.float64)


def measurement(Si, Sj, xi):
    """S_ji = exp(-xi) S_j S_i^-1."""
    return ld.pack(_ld(lambda dt, p: ld.mul(ld.exp(-np.atleast_2d(xi).astype(dt), p, 'x'),
                                            ld.mul(ld.unpack(Sj, dt), ld.inv(ld.unpack(Si, dt)))))).astype(np.float64)


def random_elements(rng, n, trans=2., rot=0.5, sig=0.3):
    return exp13(np.hstack([trans * rng.standard_normal((n, 3)), rot * rng.standard_normal((n, 3)), sig * rng.standard_normal((n, 1))]))


def direction(rng, n=1):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


def _pairs_scene(xis, seed, trans=2., sig=0.3, loss=(ld.L2, 0.)):
    """One case per wanted error: held vertex 0, per case k the vertices i = 1 + 2k (tied to 0 by an edge with an error of 0.05) and
    j = 2 + 2k = exp(xi_k) S_ji S_i.  Edge 2k is the tie, edge 2k + 1 the case."""
    rng = np.random.default_rng([seed, 31])
    n = len(xis)
    V = np.zeros((1 + 2 * n, 13))
    V[0] = random_elements(rng, 1, trans, 0.5, sig)
    Si = random_elements(rng, n, trans, 0.5, sig)
    Sji = random_elements(rng, n, trans, 0.5, sig)
    V[1::2], V[2::2] = Si, end_vertex(Si, Sji, np.asarray(xis))
    tie_err = 0.05 * rng.standard_normal((n, 7))
    tie_err[:, :3] *= 0.5 * trans                                       # (a translation error in the scene's unit)
    ties = measurement(np.tile(V[0], (n, 1)), Si, tie_err)
    ei, ej, obs = np.zeros(2 * n, int), np.zeros(2 * n, int), np.zeros((2 * n, 13))
    ei[0::2], ej[0::2], obs[0::2] = 0, 1 + 2 * np.arange(n), ties
    ei[1::2], ej[1::2], obs[1::2] = 1 + 2 * np.arange(n), 2 + 2 * np.arange(n), Sji
    held = np.arange(V.shape[0]) == 0
    return ld.Graph(V, held, ei, ej, obs, None, *loss), dict(case_edges=1 + 2 * np.arange(n), xi=np.asarray(xis))


def _graph_scene(num_vertices, pairs, held, seed, err=0.05, loss=(ld.L2, 0.), stiffness=None, xis=None, trans=2., V=None):
    """Random vertices, every edge's measurement set from its wanted error (N(0, err^2) per component unless `xis` gives it)."""
    rng = np.random.default_rng([seed, 37])
    V = random_elements(rng, num_vertices, trans) if V is None else V
    ei, ej = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    xis = err * rng.standard_normal((len(pairs), 7)) if xis is None else np.asarray(xis)
    obs = measurement(V[ei], V[ej], xis)
    mask = np.zeros(num_vertices, dtype=bool)
    mask[list(held)] = True
    return ld.Graph(V, mask, ei, ej, obs, stiffness, *loss), dict(xi=xis)


def stiffness_kind(kind, E):
    if kind == 'identity':
        return None
    d = dict(rotation_only=[0, 0, 0, 1, 1, 1, 0], scale_only=[0, 0, 0, 0, 0, 0, 1], translation_only=[1, 1, 1, 0, 0, 0, 0],
             diagonal=[1e-3, 1e-2, 1e-1, 1., 1e1, 1e2, 1e3])[kind]
    return np.tile(np.diag(np.array(d, dtype=float)), (E, 1, 1))


def mixed_pairs(E, N, held=()):
    """gs.chain_pairs (a chain, then pseudo-random pairs, every third reversed) with three duplicates of edge 1 (one of them reversed)
    and, with two held vertices, an edge between them."""
    pairs = gs.chain_pairs(E, N)
    pairs[-1], pairs[-2], pairs[-3] = pairs[1], pairs[1][::-1], pairs[1]
    if len(held) >= 2:
        pairs[-4] = (held[0], held[1])
    return pairs


# ---------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------
def _angles():
    rng = np.random.default_rng(41)
    xis = np.array([np.hstack([direction(rng)[0], a * direction(rng)[0], 0.05]) for a in ANGLES])
    g, info = _pairs_scene(xis, 1)
    info['angle'] = np.array(ANGLES)
    return g, info


def _bare():
    """Edges whose products are EXACT: the held vertex 0 and every measurement are the identity, S_v = exp(xi_v), so that the error
    transform is S_v to the bit and the logarithm's input carries no rounding of a product.  Only here can the branch of sim3_log be
    judged below 3e-5 rad, where its two branches lie nearer than one rounding of a rotation entry (theta^3 / 6) but 64 x 2^-53 |phi|
    apart from 2e-7 rad on."""
    rng = np.random.default_rng(52)
    n = len(BARE_ANGLES)
    xis = np.array([np.hstack([direction(rng)[0], a * direction(rng)[0], 0.05 * rng.standard_normal()]) for a in BARE_ANGLES])
    eye = np.hstack([np.identity(3).ravel(), np.zeros(3), 1.])
    V = np.vstack([eye, exp13(xis)])
    g = ld.Graph(V, np.arange(n + 1) == 0, np.zeros(n, int), 1 + np.arange(n), np.tile(eye, (n, 1)))
    return g, dict(xi=xis, angle=np.array(BARE_ANGLES), bare=np.ones(n, dtype=bool))


def _scales():
    rng = np.random.default_rng(42)
    cases = [(s, a) for s in SIGMAS for a in SCALE_ANGLES]
    xis = np.array([np.hstack([direction(rng)[0], a * direction(rng)[0], s]) for s, a in cases])
    g, info = _pairs_scene(xis, 2)
    info['sigma'], info['angle'] = np.array([c[0] for c in cases]), np.array([c[1] for c in cases])
    return g, info


def _units(unit, seed):
    """Vertex and measurement translations of `unit`; the wanted errors run through both branches of the logarithm and carry a
    translation of `unit` as well."""
    rng = np.random.default_rng([seed, 43])
    angles = (0., 1e-10, 0.9e-8, 1.1e-8, 3e-7, 1e-3, 0.3, 2.5)
    xis = np.array([np.hstack([unit * direction(rng)[0], a * direction(rng)[0], 0.05 * rng.standard_normal()]) for a in angles])
    g, info = _pairs_scene(xis, seed, trans=unit)
    info['angle'] = np.array(angles)
    return g, info


def _map_scales():
    rng = np.random.default_rng(44)
    scales = [(1e-3, 1e3), (1e3, 1e-3), (1e-3, 1e-3), (1e3, 1e3), (1., 1e3), (1e-3, 1.), (1., 1.)]
    n = len(scales)
    V = random_elements(rng, 1 + 2 * n, 2., 0.5, 0.)
    V[1::2, 12], V[2::2, 12] = [s[0] for s in scales], [s[1] for s in scales]
    # NARROWED: with translations of a few units at both ends of the pair whose s_j / s_i is 1e6, the error transform's translation is a
    # difference of summands of 2e6, its fp64 evaluation carries 2^-53 x 2e6 = 2e-10 absolutely beside |rho| = 1, and the cost of the
    # scene cannot meet 1e-10 by the reference alone (fp64 twin against long double: 6.5e-11, x 8 = 5e-10).  That pair's S_i sits 2e-3
    # from the origin instead; its summands reach 2e3 (the rows' rounding scale u says so), the twin's cost is then within 1e-13.
    V[1, 9:12] *= 1e-3
    pairs = [p for k in range(n) for p in ((0, 1 + 2 * k), (1 + 2 * k, 2 + 2 * k))]
    angles = (0., 1e-10, 1.1e-8, 3e-7, 1e-3, 0.3, 2.5)
    xis = np.zeros((2 * n, 7))
    xis[0::2] = 0.05 * rng.standard_normal((n, 7))
    xis[1::2] = [np.hstack([direction(rng)[0], a * direction(rng)[0], 0.05 * rng.standard_normal()]) for a in angles]
    g, info = _graph_scene(1 + 2 * n, pairs, (0,), 44, xis=xis, V=V)
    info.update(case_edges=1 + 2 * np.arange(n), angle=np.array(angles), scales=scales)
    return g, info


def _exact():
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3), (4, 1), (2, 5)]
    return _graph_scene(6, pairs, (0,), 45, xis=np.zeros((len(pairs), 7)))


ROWS_PAIRS = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 0), (0, 2), (3, 1), (2, 4), (5, 3), (4, 6), (7, 5),
              (1, 7), (6, 0), (0, 4), (5, 1), (2, 6), (7, 3)]


def rows_errors():
    """(E, 7) wanted errors of `rows`: components of size 0.02 .. 0.25 (inside k = 0.3), every fifth component 0.35 .. 0.9 (outside),
    signs alternating at random -- 20 % of the components beyond k, and at most two of a row's seven."""
    rng = np.random.default_rng(46)
    E = len(ROWS_PAIRS)
    mag = rng.uniform(0.02, 0.25, (E, 7))
    flat = mag.reshape(-1)
    flat[2::5] = rng.uniform(0.35, 0.9, flat[2::5].size)
    return mag * rng.choice([-1., 1.], (E, 7))


def _rows(loss_id, kind):
    g, info = _graph_scene(8, ROWS_PAIRS, (0,), 46, loss=(loss_id, K_LOSS), stiffness=stiffness_kind(kind, len(ROWS_PAIRS)),
                           xis=rows_errors())
    info['kind'] = kind
    return g, info


def _l1_zero():
    from pyslam_amd import synthetic
    from pyslam_amd.losses import L1Loss
    from pyslam_amd.pipelines import posegraph as pg
    d = synthetic.sim3_drift_loop(num_keyframes=12, seed=3)
    V, held, ei, ej, obs, W = pg.loop_graph(d['poses_est'], [d['closure']], loss=L1Loss()).tables()
    return ld.Graph(V, held, ei, ej, obs, W, ld.L1, 0.), dict(scene=d)


def _wg(E, seed, loss, absent=()):
    N, held = 10, (0, 5)
    pairs = mixed_pairs(E, N, held)
    rng = np.random.default_rng([seed, 47])
    xis = rng.choice([0.03, 0.1, 0.5, 0.8], (E, 7)) * rng.standard_normal((E, 7))     # both sides of k = 0.3
    K = np.tile(np.identity(7), (E, 1, 1)) * rng.uniform(0.5, 2., (E, 1, 7)) + 0.1 * rng.standard_normal((E, 7, 7))
    for n, e in enumerate(absent):
        K[e, n % 7] = 0.
    return _graph_scene(N, pairs, held, seed, loss=loss, stiffness=K, xis=xis)


def _many_edges():
    E, N = 16448, 8
    rng = np.random.default_rng(48)
    i = rng.integers(0, N, E)
    j = (i + rng.integers(1, N, E)) % N
    return _graph_scene(N, list(zip(i.tolist(), j.tolist())), (0,), 48, err=0.1, loss=(ld.HUBER, 0.1))


def _hang257():
    """257 free vertices, each joined by one identity-stiffness L2 edge to the held vertex 0; the wanted errors cycle through
    gs.tangents().  H = I and dx_v = -r_v exactly."""
    rng = np.random.default_rng(49)
    n = 257
    T = gs.tangents()
    xis = T[np.arange(n) % T.shape[0]]
    V = np.zeros((n + 1, 13))
    V[0] = random_elements(rng, 1)
    Sji = random_elements(rng, n)
    V[1:] = end_vertex(np.tile(V[0], (n, 1)), Sji, xis)
    held = np.arange(n + 1) == 0
    return ld.Graph(V, held, np.zeros(n, int), 1 + np.arange(n), Sji), dict(xi=xis)


def _noisy_loop():
    """12 vertices on a ring with chords, every measurement disturbed by exp(N(0, 0.05^2)); the start is exp(N(0, 0.1^2)) away from the
    vertices the measurements were made from.  The minimum cost is about E * 7 * 0.05^2 / 2 > 0.05."""
    N = 12
    pairs = [(k, (k + 1) % N) for k in range(N)] + [(0, 4), (9, 3), (5, 10), (2, 7)]
    g, info = _graph_scene(N, pairs, (0,), 50, err=0.05)
    rng = np.random.default_rng(51)
    start = g.V13.copy()
    moved = ld.pack(_ld(lambda dt, p: ld.mul(ld.exp((0.1 * rng.standard_normal((N - 1, 7))).astype(dt), p, 'x'), ld.unpack(g.V13[1:], dt))))
    start[1:] = moved.astype(np.float64)
    return g.with_vertices(start), info


@functools.lru_cache(maxsize=None)
def scene(name):
    if name.startswith('rows-'):
        _, loss, kind = name.split('-')
        return _rows(ld.LOSS_NAMES.index(loss), kind)
    return dict(angles=_angles, bare=_bare, scales=_scales, km=lambda: _units(1e3, 3), mm=lambda: _units(1e-3, 4), map_scales=_map_scales,
                exact=_exact, l1_zero=_l1_zero, wg64=lambda: _wg(64, 5, (ld.HUBER, K_LOSS), WG64_ABSENT),
                E65=lambda: _wg(65, 6, (ld.CAUCHY, K_LOSS)), many_edges=_many_edges, hang257=_hang257, noisy_loop=_noisy_loop)[name]()


def draws(name):
    """(many_edges: seconds per evaluation, and its 115 136 components sample enough; hang257: 50 MB per long-double H)"""
    return dict(many_edges=1, hang257=2).get(name, DRAWS)


@functools.lru_cache(maxsize=None)
def graphs(name):
    g = scene(name)[0]
    return [g] + [ld.one_ulp_away(g, d) for d in range(draws(name))]


@functools.lru_cache(maxsize=None)
def edge_pairs(name):
    """Per graph of graphs(): (its edges in long double, in fp64) -- the same input on both sides."""
    return [(ld.Edges(q, LD), ld.Edges(q, np.float64)) for q in graphs(name)]


@functools.lru_cache(maxsize=None)
def system_pairs(name, lam):
    """[(long-double (H, g, touched), fp64 twin's)] of the scene itself (the one-ulp copies' are formed in e64 and dropped)."""
    r, t = edge_pairs(name)[0]
    return [(r.assemble(lam), t.assemble(lam))]


def classes(ed):
    """{(loss, branch): edges}: branch 'small' (sn <= 1e-8) / 'log'; under L1 an edge with a capped component is 'small+cap' /
    'log+cap' (its rows carry the weight 1e8)."""
    out = {}
    cap = ed.l1_capped.any(axis=1) if ed.l1_capped is not None else np.zeros(ed.g.E, dtype=bool)
    for e in range(ed.g.E):
        key = (ld.LOSS_NAMES[ed.g.loss_id], ('small' if ed.small[e] else 'log') + ('+cap' if cap[e] else ''))
        out.setdefault(key, []).append(e)
    return {k: np.array(v) for k, v in out.items()}


def cost_err(got, ref):
    return abs(got - ref) / abs(ref) if ref else abs(got)


@functools.lru_cache(maxsize=None)
def e64(name):
    """The largest distance of the fp64 twin from the long-double pass ON THE SAME INPUT over graphs(name), in the tests' measure:
    ('rt' | 'J1' | 'J2', class) per (loss, branch) class, ('H', lam), ('g', lam), 'cost'."""
    out = {}
    pairs = edge_pairs(name)
    for r, t in pairs:
        u = ld.edge_scale(r.g)
        for key, rows in classes(r).items():
            for what in ('rt', 'J1', 'J2'):
                e = ld.row_err(getattr(t, what)[rows], getattr(r, what)[rows], u[rows])
                out[what, key] = max(out.get((what, key), 0.), e)
        out['cost'] = max(out.get('cost', 0.), cost_err(t.cost(), r.cost()))
    for lam in LAMBDAS:
        errs = []
        for n, (r, t) in enumerate(pairs):
            sr, st = system_pairs(name, lam)[0] if n == 0 else (r.assemble(lam), t.assemble(lam))
            errs.append(ld.err_system(st, sr, r))
        out['H', lam], out['g', lam] = max(e[0] for e in errs), max(e[1] for e in errs)
    return out


def e64_retract(name, dx):
    worst = 0.
    for q in graphs(name):
        ref, _ = ld.retract(q, dx, LD)
        twin, _ = ld.retract(q, dx, np.float64)
        worst = max(worst, ld.row_err(twin, ref, ld.vertex_floor(ref)))
    return worst


def definite(name, lam=0.):
    """Whether the long-double H of the scene is positive definite (its Jacobi-scaled fp64 copy has a Cholesky factor)."""
    H = system_pairs(name, lam)[0][0][0]
    d = np.diag(H).astype(float)
    if not np.all(d > 0):
        return False
    Hs = (H / np.sqrt(d)[:, None] / np.sqrt(d)[None, :]).astype(float)
    try:
        np.linalg.cholesky(Hs)
    except np.linalg.LinAlgError:
        return False
    return True


def smallest_eigenvalue(name, lam=0.):
    """Of the Jacobi-scaled H (fp64 of the long-double system): 1 / its condition number to a factor n."""
    H = system_pairs(name, lam)[0][0][0]
    d = np.sqrt(np.diag(H).astype(float))
    return float(np.linalg.eigvalsh((H / d[:, None] / d[None, :]).astype(float))[0])


@functools.lru_cache(maxsize=None)
def step_reference(name, lam):
    """(dx_ref (long double, by ld.accurate_solve on the long-double system), e_ref: the distance of a dense fp64 solve of the fp64
    twin's system from it, over the step's largest entry)."""
    (Hr, gr, _), (Ht, gt, _) = system_pairs(name, lam)[0]
    dx = ld.accurate_solve(Hr, gr)
    twin = np.linalg.solve(Ht, gt)
    scale = max(float(np.abs(dx).max()), 1e-300)
    return dx, float(np.abs(twin - dx).max()) / scale


def bound(e, floor=TOL_ROW):
    return max(floor, FACTOR * e)
