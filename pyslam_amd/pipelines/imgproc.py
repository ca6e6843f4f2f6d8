"""Host restatements of the two OpenCV image operations the dense RGB-D pipeline uses.

The reference front end (pyslam/pipelines/keyframes.py) calls ``cv2.pyrDown`` to build the image pyramid and a
3 x 3 ``cv2.Sobel`` for the image gradient.  ``cv2`` is not a dependency of this project, so both are restated here
from OpenCV's documented definitions (Gaussian pyramid: 5-tap [1 4 6 4 1] / 16 in each direction, output size
((h+1)//2, (w+1)//2), output pixel (y, x) centred on source pixel (2y, 2x); Sobel with ksize 3; both with the
default border, BORDER_REFLECT_101).  No ``cv2`` was available to check them against: they are the specification
the device kernels (csrc/ps_k_dense.h) are tested against bit for bit, and the ``cv2`` stand-in the dense golden
generator (tools/gen_dense_golden.py) installs.

The order of every floating-point operation is part of the specification:

* ``pyr_down`` on float64: horizontal pass ``s[c]*6 + (s[c-1] + s[c+1])*4 + s[c-2] + s[c+2]`` (left to right),
  the same vertical pass over its rows, then ``* (1/256)`` (exact: a power of two).  On uint8 the sums are integers
  and the result is ``(sum + 128) >> 8``.
* ``sobel`` (float64 only): d/dx is ``[-1 0 1]`` along the row (``s[c+1] - s[c-1]``) followed by ``[1 2 1]`` along
  the column (``(t[r-1] + 2*t[r]) + t[r+1]``); d/dy is ``[1 2 1]`` along the row followed by ``[-1 0 1]`` along the
  column.
"""
import numpy as np

__all__ = ['reflect101', 'pyr_down', 'sobel']


def reflect101(idx, n):
    """BORDER_REFLECT_101 index map (OpenCV borderInterpolate): ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...; folds until the
    index is inside [0, n).  A length of 1 maps everything to 0."""
    idx = np.array(idx, dtype=np.int64)
    if n == 1:
        return np.zeros_like(idx)
    while True:
        out = (idx < 0) | (idx >= n)
        if not out.any():
            return idx
        idx = np.where(idx < 0, -idx, np.where(idx >= n, 2 * n - 2 - idx, idx))


def _check(img, what):
    img = np.asarray(img)
    if img.ndim != 2:
        raise ValueError('{}: a single-channel 2-D image is required, got shape {}'.format(what, img.shape))
    if img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError('{}: empty image'.format(what))
    return img


def pyr_down(img):
    """cv2.pyrDown(img) with default arguments, for uint8 or float64 single-channel images."""
    img = _check(img, 'pyr_down')
    if img.dtype not in (np.uint8, np.float64):
        raise TypeError('pyr_down: uint8 or float64 images only, got {}'.format(img.dtype))
    h, w = img.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    cols = [reflect101(2 * np.arange(ow) + k, w) for k in (-2, -1, 0, 1, 2)]
    rows = [reflect101(2 * np.arange(oh) + k, h) for k in (-2, -1, 0, 1, 2)]
    if img.dtype == np.uint8:
        s = img.astype(np.int64)
        hp = s[:, cols[0]] + 4 * s[:, cols[1]] + 6 * s[:, cols[2]] + 4 * s[:, cols[3]] + s[:, cols[4]]
        vp = hp[rows[0]] + 4 * hp[rows[1]] + 6 * hp[rows[2]] + 4 * hp[rows[3]] + hp[rows[4]]
        return ((vp + 128) >> 8).astype(np.uint8)
    s = img
    hp = s[:, cols[2]] * 6. + (s[:, cols[1]] + s[:, cols[3]]) * 4. + s[:, cols[0]] + s[:, cols[4]]
    vp = hp[rows[2]] * 6. + (hp[rows[1]] + hp[rows[3]]) * 4. + hp[rows[0]] + hp[rows[4]]
    return vp * (1. / 256.)


def sobel(img, dx, dy):
    """cv2.Sobel(img, -1, dx, dy) with ksize 3 on a float64 image; (dx, dy) is (1, 0) or (0, 1)."""
    img = _check(img, 'sobel')
    if img.dtype != np.float64:
        raise TypeError('sobel: float64 images only, got {}'.format(img.dtype))
    if (dx, dy) not in ((1, 0), (0, 1)):
        raise ValueError('sobel: only first derivatives (dx, dy) = (1, 0) or (0, 1) are restated')
    h, w = img.shape
    cm, cp = reflect101(np.arange(w) - 1, w), reflect101(np.arange(w) + 1, w)
    rm, rp = reflect101(np.arange(h) - 1, h), reflect101(np.arange(h) + 1, h)
    if dx == 1:
        t = img[:, cp] - img[:, cm]
        return t[rm] + 2. * t + t[rp]
    t = img[:, cm] + 2. * img + img[:, cp]
    return t[rp] - t[rm]
