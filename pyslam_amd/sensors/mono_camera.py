"""Monocular pinhole camera: (x,y,z) -> (u,v).

No counterpart in the reference package, whose ReprojectionResidual is written "for any kind of camera"
(pyslam/residuals/reprojection_residual.py): any object whose ``project(pt_c, compute_jacobians)`` has this
signature.  The device restatement shares the stereo reprojection kernels (csrc/ps_math.h, cam_type = 2: the third
row of the residual is carried as zeros).  One observation of such a camera does not fix a point, so there is no
``triangulate``: landmarks are initialised from several views (Problem.triangulate_landmarks).
"""
import numpy as np

from .stereo_camera import _rows3


def _rows2(a, name):
    a = np.atleast_2d(np.asarray(a, dtype=float))
    if a.shape[1] != 2:
        raise ValueError("{} must have shape (2,) or (N,2)".format(name))
    return a


class MonoCamera:
    CAMERA_ID = 2

    def __init__(self, cu, cv, fu, fv, w, h):
        self.cu = float(cu)
        self.cv = float(cv)
        self.fu = float(fu)
        self.fv = float(fv)
        self.w = int(w)
        self.h = int(h)

    def intrinsics(self):
        """(cu, cv, fu, fv, -2): the device camera table marks monocular rows with b = -2 (b >= 0 stereo, -1 RGB-D)."""
        return np.array([self.cu, self.cv, self.fu, self.fv, -2.0])

    def clone(self):
        return self.__class__(self.cu, self.cv, self.fu, self.fv, self.w, self.h)

    def compute_pixel_grid(self):
        u, v = np.meshgrid(np.arange(self.w), np.arange(self.h), indexing='xy')
        self.u_grid = u.astype(float)
        self.v_grid = v.astype(float)

    def is_valid_measurement(self, uv):
        uv = _rows2(uv, "uv")
        return ((uv[:, 1] > 0.) & (uv[:, 1] < self.h)
                & (uv[:, 0] > 0.) & (uv[:, 0] < self.w))

    def project(self, pt_c, compute_jacobians=None):
        pt_c = _rows3(pt_c, "pt_c")
        inv_z = 1. / pt_c[:, 2]
        uv = np.empty((pt_c.shape[0], 2))
        uv[:, 0] = self.fu * pt_c[:, 0] * inv_z + self.cu
        uv[:, 1] = self.fv * pt_c[:, 1] * inv_z + self.cv
        if not compute_jacobians:
            return np.squeeze(uv)
        inv_z2 = inv_z * inv_z
        jac = np.zeros((pt_c.shape[0], 2, 3))
        jac[:, 0, 0] = self.fu * inv_z
        jac[:, 0, 2] = -self.fu * pt_c[:, 0] * inv_z2
        jac[:, 1, 1] = self.fv * inv_z
        jac[:, 1, 2] = -self.fv * pt_c[:, 1] * inv_z2
        return np.squeeze(uv), np.squeeze(jac)

    def __repr__(self):
        return ("{}:\n cu: {:f}\n cv: {:f}\n fu: {:f}\n fv: {:f}\n"
                "  w: {:d}\n  h: {:d}\n").format(
                    self.__class__.__name__, self.cu, self.cv, self.fu, self.fv,
                    self.w, self.h)
