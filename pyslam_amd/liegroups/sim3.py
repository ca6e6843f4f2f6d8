"""Sim(3): similarities of space, stored as (rot, trans, scale) with scale > 0: p -> scale * R p + t, as a matrix
[[scale R, t], [0, 1]].

Tangent xi = [rho (3); phi (3); sigma (1)]: translation first, as SE(3) has it, scale last.  exp(xi) is the matrix exponential of
[[phi^ + sigma I, rho], [0, 0]]:

    scale = e^sigma,   R = Exp(phi),   t = W(phi, sigma) rho,   W = int_0^1 e^(tau sigma) Exp(tau phi) dtau = A I + B phi^ + C phi^^2

with, for z = sigma + i theta, theta = |phi| and f(z) = (e^z - 1) / z:  A = f(sigma),  B = Im f(z) / theta,
C = (A - Re f(z)) / theta^2.  ``w_coefficients`` evaluates them in two branches (the device's ``sim3_w_coef``, csrc/ps_k_sim3pg.h,
is the same arithmetic):

* |z|^2 <= 1: the power series sum_n z^n / (n + 1)!, carried as the real recurrences p_n = Im z^n / theta, q_n = (sigma^n -
  Re z^n) / theta^2 -- no division, exact at theta = 0, sigma = 0 and both;
* otherwise the closed forms, rearranged so that a small theta beside a large sigma (or the reverse) cancels nothing:
  B = (sigma (E h1 - A) + E theta^2 h2) / |z|^2,  C = (sigma E h2 + A - E h1) / |z|^2,  with E = e^sigma, A = expm1(sigma) / sigma,
  h1 = sin(theta) / theta, h2 = (1 - cos(theta)) / theta^2 = (sin(theta / 2) / (theta / 2))^2 / 2.

log is the inverse for rotation angles below pi; perturb is a LEFT perturbation, S <- exp(xi) S, as the other groups' is.
Adjoint in this ordering: [[scale R, t^ R, -t], [0, R, 0], [0, 0, 1]]."""
import numpy as np

from ._base import MatrixGroup
from .so3 import SO3
from .se import SE3

SERIES_RADIUS2 = 1.0     # |z|^2 up to which the power series runs
SERIES_TERMS = 22        # 1 / 23! = 3.9e-23: below an ulp of the sums at |z| = 1
TINY_ANGLE = 1e-8        # below it sin(theta) / theta = 1 and (1 - cos(theta)) / theta^2 = 1 / 2 to rounding


def w_series(theta, sigma):
    th2 = theta * theta
    a, p, q, sn = 1.0, 0.0, 0.0, 1.0                         # Re z^n, Im z^n / theta, (sigma^n - Re z^n) / theta^2, sigma^n
    inv_fact = 1.0
    A, B, C = 1.0, 0.0, 0.0
    for n in range(1, SERIES_TERMS + 1):
        p, q = sigma * p + a, sigma * q + p
        sn *= sigma
        a = sn - th2 * q
        inv_fact /= (n + 1)
        A += sn * inv_fact
        B += p * inv_fact
        C += q * inv_fact
    return A, B, C


def w_closed(theta, sigma):
    th2 = theta * theta
    E = np.exp(sigma)
    A = np.expm1(sigma) / sigma if sigma != 0. else 1.0
    h1, h2 = _h12(theta)
    z2 = sigma * sigma + th2
    return A, (sigma * (E * h1 - A) + E * th2 * h2) / z2, (sigma * E * h2 + A - E * h1) / z2


def w_coefficients(theta, sigma):
    """(A, B, C) of W = A I + B phi^ + C phi^^2 (module docstring)."""
    if sigma * sigma + theta * theta <= SERIES_RADIUS2:
        return w_series(theta, sigma)
    return w_closed(theta, sigma)


def _h12(theta):
    """sin(theta) / theta and (1 - cos(theta)) / theta^2."""
    if theta <= TINY_ANGLE:
        return 1.0, 0.5
    half = 0.5 * theta
    sh = np.sin(half) / half
    return np.sin(theta) / theta, 0.5 * sh * sh


def _w_matrix(phi, sigma):
    K = SO3.wedge(phi)
    A, B, C = w_coefficients(float(np.linalg.norm(phi)), float(sigma))
    return A * np.identity(3) + B * K + C * (K @ K)


def _rot_exp(phi):
    """Exp(phi) = I + h1 phi^ + h2 phi^^2 with the h1, h2 of the module docstring."""
    K = SO3.wedge(phi)
    h1, h2 = _h12(float(np.linalg.norm(phi)))
    return np.identity(3) + h1 * K + h2 * (K @ K)


def _rot_log(R):
    """phi of a rotation with angle below pi: the angle from atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2), accurate at both ends."""
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * float(np.linalg.norm(v))
    c = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2]) - 0.5
    theta = float(np.arctan2(s, c))
    if s <= TINY_ANGLE:
        return 0.5 * v                                        # theta / sin(theta) = 1 to rounding
    return (0.5 * theta / s) * v


class Sim3(MatrixGroup):
    dof = 7
    dim = 4

    def __init__(self, rot, trans, scale=1.0):
        self.rot = rot if isinstance(rot, SO3) else SO3(np.asarray(rot, dtype=float).reshape(3, 3))
        self.trans = np.asarray(trans, dtype=float).reshape(3)
        self.scale = float(scale)
        if not self.scale > 0.:
            raise ValueError("Sim3: the scale must be positive, got {}".format(scale))

    @classmethod
    def identity(cls):
        return cls(SO3.identity(), np.zeros(3), 1.0)

    @classmethod
    def from_se3(cls, T, scale=1.0):
        M = T.as_matrix() if hasattr(T, 'as_matrix') else np.asarray(T, dtype=float)
        return cls(SO3(M[:3, :3].copy()), M[:3, 3].copy(), scale)

    @classmethod
    def from_matrix(cls, mat, normalize=False):
        mat = np.asarray(mat, dtype=float)
        if mat.shape != (4, 4) or not np.allclose(mat[3], [0., 0., 0., 1.]):
            if not normalize:
                raise ValueError("Invalid similarity matrix. Use normalize=True to handle rounding errors.")
        M = mat[:3, :3]
        det = np.linalg.det(M)
        if not det > 0.:
            raise ValueError("Invalid similarity matrix: the determinant of its upper left block must be positive")
        s = float(np.cbrt(det))
        return cls(SO3.from_matrix(M / s, normalize=normalize), mat[:3, 3].copy(), s)

    @classmethod
    def exp(cls, xi):
        xi = np.asarray(xi, dtype=float).reshape(7)
        rho, phi, sigma = xi[0:3], xi[3:6], xi[6]
        return cls(SO3(_rot_exp(phi)), _w_matrix(phi, sigma) @ rho, np.exp(sigma))

    def log(self):
        phi = _rot_log(self.rot.mat)
        sigma = np.log(self.scale)
        rho = np.linalg.solve(_w_matrix(phi, sigma), self.trans)
        return np.hstack([rho, phi, sigma])

    def inv(self):
        Rt = self.rot.mat.T.copy()
        return Sim3(SO3(Rt), -(Rt @ self.trans) / self.scale, 1. / self.scale)

    def as_matrix(self):
        out = np.identity(4)
        out[:3, :3] = self.scale * self.rot.mat
        out[:3, 3] = self.trans
        return out

    def normalize(self):
        self.rot.normalize()

    def perturb(self, xi):
        moved = Sim3.exp(xi).dot(self)
        self.rot, self.trans, self.scale = moved.rot, moved.trans, moved.scale

    def dot(self, other):
        if isinstance(other, Sim3):
            return Sim3(SO3(self.rot.mat @ other.rot.mat), self.scale * (self.rot.mat @ other.trans) + self.trans,
                        self.scale * other.scale)
        other = np.atleast_2d(other)
        if other.shape[1] == 3:
            return np.squeeze(self.scale * other.dot(self.rot.mat.T) + self.trans)
        if other.shape[1] == 4:
            return np.squeeze(other.dot(self.as_matrix().T))
        raise ValueError("Vector must have shape (3,), (4,), (N,3) or (N,4)")

    def adjoint(self):
        R = self.rot.mat
        out = np.zeros((7, 7))
        out[0:3, 0:3] = self.scale * R
        out[0:3, 3:6] = SO3.wedge(self.trans) @ R
        out[0:3, 6] = -self.trans
        out[3:6, 3:6] = R
        out[6, 6] = 1.
        return out

    def to_se3(self):
        """(R, t / scale): the rigid pose the same camera has in the map rescaled by this similarity."""
        return SE3(SO3(self.rot.mat.copy()), self.trans / self.scale)

    @staticmethod
    def wedge(xi):
        xi = np.atleast_2d(np.asarray(xi, dtype=float))
        out = np.zeros((xi.shape[0], 4, 4))
        out[:, 0:3, 0:3] = SO3.wedge(xi[:, 3:6]).reshape(-1, 3, 3) + xi[:, 6][:, None, None] * np.identity(3)
        out[:, 0:3, 3] = xi[:, 0:3]
        return np.squeeze(out)

    @staticmethod
    def vee(Xi):
        Xi = np.asarray(Xi, dtype=float)
        if Xi.ndim < 3:
            return np.hstack([Xi[0:3, 3], SO3.vee(0.5 * (Xi[0:3, 0:3] - Xi[0:3, 0:3].T)), np.trace(Xi[0:3, 0:3]) / 3.])
        skew = 0.5 * (Xi[:, 0:3, 0:3] - np.transpose(Xi[:, 0:3, 0:3], (0, 2, 1)))
        return np.hstack([Xi[:, 0:3, 3], SO3.vee(skew), (np.trace(Xi[:, 0:3, 0:3], axis1=1, axis2=2) / 3.)[:, None]])
