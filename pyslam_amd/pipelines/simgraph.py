"""Sim(3) pose graph, restated in dense numpy: the definition the device path (csrc/ps_k_sim3pg.h, ps_host_sim3pg.h) is held
against.  Like similarity.py it is test infrastructure and documentation; nothing on the solving path calls it.

Vertices are ``Sim3`` (pyslam_amd/liegroups/sim3.py), an edge is ``(i, j, S_ji, W)`` with W a 7 x 7 stiffness or None (identity):

    r = W log(S_j S_i^-1 S_ji^-1),   J_i = -W Ad(S_j S_i^-1),   J_j = W          (first order, exact at r = 0)

The robust loss acts per residual component: s_k = sqrt(w(r_k)), J~ = diag(s) J, r~ = s r, H = sum J~^T J~, g = -sum J~^T r~,
cost = sum rho(r_k); an all-zero stiffness row is an absent row (no weight, no cost).  Held vertices contribute no unknowns; an
edge between two of them adds cost only.  One iteration: H's diagonal times (1 + lambda), dx = H^-1 g, S <- exp(dx) S for the
free vertices, the cost after the step.  The loop is Problem.solve's under the meaning "an iteration's cost is the cost after its
step" (pyslam_amd/problem.py: StopRule), the best vertices kept and restored."""
import numpy as np

from pyslam_amd.liegroups.sim3 import Sim3


def _edge(edge):
    i, j, S_ji = edge[0], edge[1], edge[2]
    W = edge[3] if len(edge) > 3 and edge[3] is not None else None
    return int(i), int(j), S_ji, (None if W is None else np.asarray(W, dtype=np.float64).reshape(7, 7))


def _edge_terms(V, edge):
    """(xi, r, present, W, S_j S_i^-1) of one edge."""
    i, j, S_ji, W = _edge(edge)
    T21 = V[j].dot(V[i].inv())
    xi = T21.dot(S_ji.inv()).log()
    if W is None:
        return xi, xi, np.ones(7, dtype=bool), np.identity(7), T21
    return xi, W @ xi, (W != 0.).any(axis=1), W, T21


def residuals(V, edges):
    """(E, 7): r of every edge."""
    return np.array([_edge_terms(V, e)[1] for e in edges]).reshape(-1, 7)


def _free_index(num, held):
    held = np.asarray(held, dtype=bool).reshape(num)
    if not held.any():
        raise ValueError("simgraph: at least one vertex must be held")
    rid = np.full(num, -1, dtype=np.int64)
    rid[~held] = np.arange(int((~held).sum()))
    return held, rid


L1_WEIGHT_CAP = 1e-8     # PS_SMALL_ANGLE of the device


def _rho_weight(loss, r):
    """(rho, IRLS weight) per component.  L1's weight is 1 / max(|r_k|, 1e-8) in this graph (``L1Loss.weight`` is NaN within 1e-8 of
    zero): the odometry and covisibility edges of a loop correction are measured from the current estimates, so their components
    START at zero, and zero is where an L1 solve converges to; the capped weight is the usual IRLS regularisation.  The cost stays
    |r_k| (csrc/ps_k_sim3pg.h: s3g_loss_weight)."""
    if loss is None:
        return 0.5 * r * r, np.ones(r.size)
    if getattr(loss, 'LOSS_ID', None) == 1:
        return np.abs(r), 1. / np.maximum(np.abs(r), L1_WEIGHT_CAP)
    return np.asarray(loss.loss(r), dtype=np.float64).reshape(r.size), np.asarray(loss.weight(r), dtype=np.float64).reshape(r.size)


def cost(V, edges, loss=None):
    total = 0.
    for e in edges:
        _, r, present, _, _ = _edge_terms(V, e)
        rho, _ = _rho_weight(loss, r)
        total += float(rho[present].sum())
    return total


def scaled_edge(V, edge, loss=None):
    """(r~, J~_i, J~_j, cost) of one edge: what the device's tap returns."""
    _, r, present, W, T21 = _edge_terms(V, edge)
    rho, w = _rho_weight(loss, r)
    s = np.where(present, np.sqrt(np.where(present, w, 0.)), 0.)
    return s * r, -(s[:, None] * W) @ T21.adjoint(), s[:, None] * W, float(rho[present].sum())


def linearise(V, edges, held, loss=None):
    """(H, g, cost): the undamped dense system over the free vertices, H dx = g."""
    held, rid = _free_index(len(V), held)
    n = 7 * int((~held).sum())
    H, g, total = np.zeros((n, n)), np.zeros(n), 0.
    for e in edges:
        i, j = int(e[0]), int(e[1])
        rs, J1, J2, c = scaled_edge(V, e, loss)
        total += c
        a, b = rid[i], rid[j]
        if a >= 0:
            H[7 * a:7 * a + 7, 7 * a:7 * a + 7] += J1.T @ J1
            g[7 * a:7 * a + 7] -= J1.T @ rs
        if b >= 0:
            H[7 * b:7 * b + 7, 7 * b:7 * b + 7] += J2.T @ J2
            g[7 * b:7 * b + 7] -= J2.T @ rs
        if a >= 0 and b >= 0:
            H[7 * a:7 * a + 7, 7 * b:7 * b + 7] += J1.T @ J2
            H[7 * b:7 * b + 7, 7 * a:7 * a + 7] += J2.T @ J1
    return H, g, total


def damped(H, lam):
    A = H.copy()
    A[np.diag_indices_from(A)] *= 1. + lam
    return A


def retract(V, held, dx):
    held, rid = _free_index(len(V), held)
    return [S if held[v] else Sim3.exp(dx[7 * rid[v]:7 * rid[v] + 7]).dot(S) for v, S in enumerate(V)]


def iterate(V, edges, held, loss=None, lam=0.):
    """One iteration -> (new vertices, dx, cost after the step)."""
    H, g, _ = linearise(V, edges, held, loss)
    dx = np.linalg.solve(damped(H, lam), g)
    new = retract(V, held, dx)
    return new, dx, cost(new, edges, loss)


def solve(V, edges, held, loss=None, options=None):
    """-> (vertices, cost history, iterations)."""
    from pyslam_amd.problem import Options, StopRule
    opt = options if options is not None else Options()
    V = list(V)
    history = [cost(V, edges, loss)]
    rule = StopRule(opt, history[0])
    best = V
    while True:
        V, dx, c = iterate(V, edges, held, loss, float(getattr(opt, 'lm_lambda', 0.)))
        history.append(c)
        f = rule.step(c, float(np.linalg.norm(dx)))
        if f & StopRule.KEEP_BEST:
            best = V
        if f & StopRule.RESTORE_BEST:
            V = best
        if f & StopRule.DONE:
            return V, history, rule.iters
