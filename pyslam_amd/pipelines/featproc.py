"""Host restatement of the sparse front end: corner features, 32-byte gradient descriptors and circular matching.

TEST INFRASTRUCTURE like ``imgproc``: pure numpy, the specification the device matcher (csrc/ps_k_feat.h, face:
pipelines/matcher.py) is tested against bit for bit.  The product's matcher never calls it.  The definition is all
integer up to the one division of the sub-pixel step:

1. ``gradients``: 3 x 3 Sobel ``du`` (``[-1 0 1]`` along the row, ``[1 2 1]`` along the column) and ``dv`` of the uint8
   image as int16, borders replicated.
2. ``response``: over the 5 x 5 window ``a = sum du^2``, ``b = sum du dv``, ``c = sum dv^2`` in int64 and
   ``R = 16 (a c - b^2) - (a + c)^2``; pixels closer than 2 to a border (window not inside the image) hold ``R_NONE``.
3. ``features``: ``R > response_threshold``, ``R`` the maximum of its ``(2 nms_n + 1)^2`` neighbourhood with an equal
   value earlier in raster order winning, at least ``BORDER`` = 5 pixels from every border; raster order; above
   ``max_features`` the strongest are kept (ties to the earlier raster index) and raster order is restored.
4. descriptor: ``clamp((g >> 2) + 128, 0, 255)`` of ``du`` at the 16 ``OFFSETS`` (bytes 0..15) and of ``dv`` at the
   same offsets (bytes 16..31); pixel coordinates clamped to the image (only the +-1 neighbours of the sub-pixel
   step can reach outside).
5. ``match_leg``: candidates of a feature of A are the features of B with ``dv_lo <= v_B - v_A <= dv_hi`` and
   ``du_lo <= u_B - u_A <= du_hi``; cost = sum of absolute byte differences; lowest cost wins, ties to the lower index
   in B; -1 when there is no candidate or the cost exceeds ``match_cost_max``.
6. ``match``: mode 0 flow (previous-left -> current-left and back), 1 stereo (left -> right and back), 2 quad
   (previous-left -> previous-right -> current-right -> current-left -> previous-left); a match is a chain that
   returns to its start; matches in the order of their first feature.
7. sub-pixel (``refinement``): the first feature of a chain stays at its integer pixel.  Each further leg adds
   ``delta = (c_minus - c_plus) / (2 (max(c_minus, c_plus) - c_0))`` (float64; 0 unless the denominator is positive,
   ``c_0 > 0`` -- an exact match stays where it is -- and ``|delta| < 1``) to a running offset, from the costs of the
   source descriptor against the target pixel and its two neighbours at +-1: in ``u`` for stereo legs, in ``u`` and
   ``v`` for temporal legs.  A position is its integer pixel plus the offset accumulated up to its leg, so the chain
   follows one scene point; the closing leg refines nothing.
8. ``match_map`` (matching by projection): a map point ``(x, y, z)`` with its descriptor is projected with ``T_cw`` and
   ``cam = (cu, cv, fu, fv, ...)`` in float64, one rounding per operation: ``x_c = ((r00 x + r01 y) + r02 z) + t0`` (``y_c``,
   ``z_c`` likewise), ``u = (fu x_c) / z_c + cu``, ``v = (fv y_c) / z_c + cv``; the window centre is ``ui = floor(u + 0.5)``,
   ``vi`` likewise.  Status 1 (not visible): ``z_c <= 0``, a non-finite value, or a centre outside the image.  Candidates are
   the frame's features with ``|u_k - ui| <= radius`` and ``|v_k - vi| <= radius``; cost, winner and tie rule as in step 5;
   status 2 without a candidate or with the best cost above ``match_cost_max``.  A feature goes to one point only: among the
   points whose best feature it is, the lowest ``(cost, point index)`` keeps it, the others get status 3 and feature -1 (no
   second choice).  The position of a matched point (status 0) is the feature's pixel plus the offsets of step 7's temporal
   leg (map descriptor against the frame's gradient images); with ``refinement`` = 0 the pixel itself.
9. ``match_map_global`` (matching without a prior): every map descriptor against every one of the frame's ``F`` features, no
   projection.  ``c(i, k)`` is step 5's cost; ``best`` is the feature with the lowest ``(c, k)``, ``c1`` its cost, ``c2`` the lowest
   cost over the features ``k != best`` (none when ``F < 2``).  Status 2 (no candidate): ``F == 0`` or ``c1 > match_cost_max``;
   else status 4 (ambiguous) when ``c2`` exists and ``ratio_den c1 >= ratio_num c2`` (``0 < ratio_num <= ratio_den <= 32768``,
   64-bit products: a minimum reached by two features is always ambiguous, and so is ``c1 = c2 = 0``); else status 0, after which
   step 8's one-landmark-per-feature rule (status 3) and sub-pixel position apply unchanged.  Status 1 does not occur.  ``cost``
   is ``c1`` and ``second`` is ``c2`` (-1 where it does not exist) for the statuses 0, 3 and 4, both -1 for status 2.
"""
import numpy as np

__all__ = ['Params', 'OFFSETS', 'BORDER', 'R_NONE', 'gradients', 'response', 'features', 'match_leg', 'match', 'match_map', 'match_map_global', 'db_query', 'Frame']

BORDER = 5
R_NONE = np.iinfo(np.int64).min
# (du, dv) pixel offsets of the 16 descriptor samples inside the 11 x 11 patch
OFFSETS = ((-1, -1), (1, -1), (-1, 1), (1, 1),
           (-3, -1), (3, -1), (-3, 1), (3, 1),
           (-1, -3), (1, -3), (-1, 3), (1, 3),
           (-5, 0), (5, 0), (0, -5), (0, 5))


class Params:
    """The constants of the definition (pipelines/matcher.py: Matcher_parameters has the same fields and defaults)."""
    FIELDS = (('response_threshold', 1 << 36), ('nms_n', 2), ('max_features', 4096), ('match_radius_u', 200),
              ('match_radius_v', 50), ('disp_max', 160), ('match_cost_max', 1200), ('refinement', 1))

    def __init__(self, **kw):
        for k, v in self.FIELDS:
            setattr(self, k, kw.pop(k, v))
        if kw:
            raise TypeError('unknown matcher parameters: {}'.format(sorted(kw)))


def _image(img):
    img = np.asarray(img)
    if img.ndim != 2 or img.dtype != np.uint8:
        raise TypeError('a single-channel uint8 image is required, got {} {}'.format(img.dtype, img.shape))
    if img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError('empty image')
    return img


def gradients(img):
    """(du, dv): the 3 x 3 Sobel derivatives of a uint8 image as int16, borders replicated."""
    p = np.pad(_image(img).astype(np.int32), 1, mode='edge')
    tx = p[:, 2:] - p[:, :-2]                              # [-1 0 1] along the row
    du = tx[:-2] + 2 * tx[1:-1] + tx[2:]                   # [1 2 1] along the column
    ty = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    dv = ty[2:] - ty[:-2]
    return du.astype(np.int16), dv.astype(np.int16)


def _box5(x):
    h, w = x.shape
    out = np.zeros((h - 4, w - 4), dtype=np.int64)
    for dy in range(5):
        for dx in range(5):
            out += x[dy:dy + h - 4, dx:dx + w - 4]
    return out


def response(du, dv):
    """R (int64) of every pixel whose 5 x 5 window lies inside the image, R_NONE elsewhere."""
    h, w = du.shape
    R = np.full((h, w), R_NONE, dtype=np.int64)
    if h < 5 or w < 5:
        return R
    x, y = du.astype(np.int64), dv.astype(np.int64)
    a, b, c = _box5(x * x), _box5(x * y), _box5(y * y)
    R[2:h - 2, 2:w - 2] = 16 * (a * c - b * b) - (a + c) * (a + c)
    return R


def _describe(du, dv, u, v):
    """Descriptors (n, 32) uint8 of the pixels (u, v) (coordinates clamped to the image)."""
    h, w = du.shape
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    out = np.zeros((u.shape[0], 32), dtype=np.uint8)
    for k, (ox, oy) in enumerate(OFFSETS):
        x, y = np.clip(u + ox, 0, w - 1), np.clip(v + oy, 0, h - 1)
        out[:, k] = np.clip((du[y, x].astype(np.int32) >> 2) + 128, 0, 255)
        out[:, 16 + k] = np.clip((dv[y, x].astype(np.int32) >> 2) + 128, 0, 255)
    return out


class Frame:
    """The features of one image: ``uv`` (n, 2) int32 in raster order, ``R`` (n,) int64, ``desc`` (n, 32) uint8, the
    gradient images and ``row_start`` (h + 1,), the index of the first feature of every row."""

    def __init__(self, du, dv, uv, R, desc):
        self.du, self.dv, self.uv, self.R, self.desc = du, dv, uv, R, desc
        self.row_start = np.searchsorted(uv[:, 1], np.arange(du.shape[0] + 1), side='left').astype(np.int32)

    def __len__(self):
        return self.uv.shape[0]


def features(img, params=None):
    """The feature list of a uint8 image (steps 1-4)."""
    p = params or Params()
    du, dv = gradients(img)
    R = response(du, dv)
    h, w = R.shape
    n = int(p.nms_n)
    if not 1 <= n <= 3:
        raise ValueError('nms_n must be 1..3')
    ok = np.zeros((h, w), dtype=bool)
    if h > 2 * BORDER and w > 2 * BORDER:
        ys, xs = slice(BORDER, h - BORDER), slice(BORDER, w - BORDER)
        c = R[ys, xs]
        keep = c > int(p.response_threshold)
        for dy in range(-n, n + 1):
            for dx in range(-n, n + 1):
                if dx == 0 and dy == 0:
                    continue
                q = R[BORDER + dy:h - BORDER + dy, BORDER + dx:w - BORDER + dx]
                keep &= (q < c) if (dy, dx) < (0, 0) else (q <= c)     # an equal value earlier in raster order wins
        ok[ys, xs] = keep
    v, u = np.nonzero(ok)                                      # raster order
    r = R[v, u]
    if u.shape[0] > int(p.max_features):
        order = np.lexsort((np.arange(u.shape[0]), -r))[:int(p.max_features)]
        order.sort()
        u, v, r = u[order], v[order], r[order]
    uv = np.stack([u, v], axis=1).astype(np.int32).reshape(-1, 2)
    return Frame(du, dv, uv, r, _describe(du, dv, u, v))


def match_leg(A, B, du_lo, du_hi, dv_lo, dv_hi, cost_max):
    """Index in B of the best candidate of every feature of A, -1 where there is none (step 5)."""
    out = np.full(len(A), -1, dtype=np.int32)
    if len(A) == 0 or len(B) == 0:
        return out
    h = A.du.shape[0]
    bd = B.desc.astype(np.int16)
    for i in range(len(A)):
        ua, va = int(A.uv[i, 0]), int(A.uv[i, 1])
        k0, k1 = B.row_start[min(max(va + dv_lo, 0), h)], B.row_start[min(max(va + dv_hi + 1, 0), h)]
        if k1 <= k0:
            continue
        d = B.uv[k0:k1, 0] - ua
        cand = np.nonzero((d >= du_lo) & (d <= du_hi))[0]
        if cand.shape[0] == 0:
            continue
        cost = np.abs(bd[k0 + cand] - A.desc[i].astype(np.int16)).sum(axis=1)
        j = int(np.argmin(cost))                               # first minimum: the lower index in B
        if cost[j] <= cost_max:
            out[i] = k0 + cand[j]
    return out


def _subpixel(cm, c0, cp):
    """Sub-pixel offset from the costs at -1, 0, +1: the equiangular (two-line) fit, the model of a SAD cost, which is a
    V around its minimum and not a parabola."""
    den = 2 * (np.maximum(cm, cp) - c0)
    d = np.zeros(cm.shape[0])
    ok = (den > 0) & (c0 > 0)                              # an exact match (cost 0) has no sub-pixel offset
    d[ok] = (cm[ok] - cp[ok]).astype(np.float64) / den[ok].astype(np.float64)
    d[~(np.abs(d) < 1.0)] = 0.0
    return d


def _refine(src, ia, dst, ib, temporal):
    """Sub-pixel offsets (du, dv) of features ib of `dst` against the descriptors of features ia of `src` (step 7)."""
    d = src.desc[ia].astype(np.int64)
    u, v = dst.uv[ib, 0], dst.uv[ib, 1]

    def cost(ox, oy):
        return np.abs(_describe(dst.du, dst.dv, u + ox, v + oy).astype(np.int64) - d).sum(axis=1)
    c0 = cost(0, 0)
    ou = _subpixel(cost(-1, 0), c0, cost(1, 0))
    ov = _subpixel(cost(0, -1), c0, cost(0, 1)) if temporal else np.zeros(ou.shape[0])
    return ou, ov


def match(prev, cur, mode, params=None):
    """Matches between two frames, each a (left Frame, right Frame or None) pair; `prev` may be None in mode 1.

    Returns ``(m, idx)``: ``m`` (n, 8) float64 with the columns u1p v1p u2p v2p u1c v1c u2c v2c (1 left, 2 right;
    -1 in the columns a mode does not fill) and ``idx`` (n, 4) int32 feature indices (1p, 2p, 1c, 2c; -1 likewise)."""
    p = params or Params()
    ru, rv, dm, cmax = int(p.match_radius_u), int(p.match_radius_v), int(p.disp_max), int(p.match_cost_max)

    def temporal(A, B):
        return match_leg(A, B, -ru, ru, -rv, rv, cmax)

    def left_right(A, B):
        return match_leg(A, B, -dm, 0, -1, 1, cmax)

    def right_left(A, B):
        return match_leg(A, B, 0, dm, -1, 1, cmax)

    def follow(cur_idx, leg):
        return np.where(cur_idx >= 0, leg[np.maximum(cur_idx, 0)], -1) if leg.shape[0] else np.full_like(cur_idx, -1)

    if mode == 0:
        chain = [(prev[0], None), (cur[0], 'T'), (prev[0], 'T')]
        cols = [0, 2]
        legs = [temporal(prev[0], cur[0]), temporal(cur[0], prev[0])]
    elif mode == 1:
        chain = [(cur[0], None), (cur[1], 'S'), (cur[0], 'S')]
        cols = [2, 3]
        legs = [left_right(cur[0], cur[1]), right_left(cur[1], cur[0])]
    elif mode == 2:
        chain = [(prev[0], None), (prev[1], 'S'), (cur[1], 'T'), (cur[0], 'S'), (prev[0], 'T')]
        cols = [0, 1, 3, 2]
        legs = [left_right(prev[0], prev[1]), temporal(prev[1], cur[1]), right_left(cur[1], cur[0]),
                temporal(cur[0], prev[0])]
    else:
        raise ValueError('matching mode must be 0 (flow), 1 (stereo) or 2 (quad)')
    start = np.arange(len(chain[0][0]), dtype=np.int32)
    visited = [start]
    for leg in legs:
        visited.append(follow(visited[-1], leg).astype(np.int32))
    good = np.nonzero(visited[-1] == start)[0]
    n = good.shape[0]
    m = np.full((n, 8), -1.0)
    idx = np.full((n, 4), -1, dtype=np.int32)
    offu, offv = np.zeros(n), np.zeros(n)
    for k, col in enumerate(cols):
        fr, kind = chain[k]
        ids = visited[k][good]
        if k > 0 and p.refinement and n:
            ou, ov = _refine(chain[k - 1][0], visited[k - 1][good], fr, ids, kind == 'T')
            offu, offv = offu + ou, offv + ov
        idx[:, col] = ids
        m[:, 2 * col] = fr.uv[ids, 0] + offu
        m[:, 2 * col + 1] = fr.uv[ids, 1] + offv
    return m, idx


def match_map(frame, points_w, descriptors, T_cw, cam, radius, params=None):
    """Map points matched into a frame by projection (step 8) -> ``(feature, status, cost, uv)``, one entry per point:
    feature index or -1 (int32), status 0 matched / 1 not visible / 2 no candidate / 3 lost its feature to a better point
    (int32), cost or -1 unless the status is 0 or 3 (int32), position (N, 2) float64 or -1 unless the status is 0."""
    p = params or Params()
    pts = np.asarray(points_w, dtype=np.float64).reshape(-1, 3)
    desc = np.asarray(descriptors, dtype=np.uint8).reshape(-1, 32)
    N = pts.shape[0]
    if desc.shape[0] != N:
        raise ValueError('match_map: {} points and {} descriptors'.format(N, desc.shape[0]))
    radius = int(radius)
    if radius < 0:
        raise ValueError('match_map: negative radius')
    T = np.asarray(T_cw, dtype=np.float64).reshape(4, 4)
    cu, cv, fu, fv = (float(c) for c in tuple(cam)[:4])
    h, w = frame.du.shape
    feature = np.full(N, -1, dtype=np.int32)
    status = np.full(N, 1, dtype=np.int32)
    cost = np.full(N, -1, dtype=np.int32)
    uv = np.full((N, 2), -1.0)
    X, Y, Z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all='ignore'):
        xc = ((T[0, 0] * X + T[0, 1] * Y) + T[0, 2] * Z) + T[0, 3]
        yc = ((T[1, 0] * X + T[1, 1] * Y) + T[1, 2] * Z) + T[1, 3]
        zc = ((T[2, 0] * X + T[2, 1] * Y) + T[2, 2] * Z) + T[2, 3]
        u, v = (fu * xc) / zc + cu, (fv * yc) / zc + cv
        cen_u, cen_v = np.floor(u + 0.5), np.floor(v + 0.5)
        visible = (zc > 0.) & np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & np.isfinite(u) & np.isfinite(v) & \
            (cen_u >= 0.) & (cen_u < w) & (cen_v >= 0.) & (cen_v < h)
    r = min(radius, max(h, w))                                 # a window over the whole image is as large as it gets
    bd = frame.desc.astype(np.int16)
    for i in np.nonzero(visible)[0]:
        ui, vi = int(cen_u[i]), int(cen_v[i])
        status[i] = 2
        k0, k1 = frame.row_start[min(max(vi - r, 0), h)], frame.row_start[min(max(vi + r + 1, 0), h)]
        if k1 <= k0:
            continue
        d = frame.uv[k0:k1, 0] - ui
        cand = np.nonzero((d >= -r) & (d <= r))[0]
        if cand.shape[0] == 0:
            continue
        c = np.abs(bd[k0 + cand] - desc[i].astype(np.int16)).sum(axis=1)
        j = int(np.argmin(c))                                  # first minimum: the lower feature index
        if c[j] <= int(p.match_cost_max):
            feature[i], cost[i], status[i] = k0 + cand[j], c[j], 0
    _claim_and_refine(frame, desc, feature, status, cost, uv, p)
    return feature, status, cost, uv


def _claim_and_refine(frame, desc, feature, status, cost, uv, p):
    """The end of steps 8 and 9, in place: one landmark per feature -- the lowest (cost, point index) keeps it, the others get
    status 3 and feature -1 -- and the positions of the owners."""
    cand = np.nonzero(status == 0)[0]
    order = cand[np.lexsort((cand, cost[cand], feature[cand]))]
    lost = order[1:][feature[order[1:]] == feature[order[:-1]]]
    status[lost], feature[lost] = 3, -1
    won = np.nonzero(status == 0)[0]
    if won.shape[0]:
        f = feature[won]
        uv[won] = frame.uv[f]
        if p.refinement:
            ou, ov = _refine(_Descriptors(desc), won, frame, f, True)
            uv[won, 0] += ou
            uv[won, 1] += ov


def match_map_global(frame, descriptors, ratio=(4, 5), params=None):
    """Map descriptors matched into a frame without a prior (step 9) -> ``(feature, status, cost, second, uv)``, one entry per map
    point: feature index or -1 (int32), status 0 matched / 2 no candidate / 3 lost its feature to a better point / 4 ambiguous
    (int32), best cost and second-best cost (int32; -1 for status 2, ``second`` also where the frame has a single feature),
    position (N, 2) float64 or -1 unless the status is 0.  ``ratio`` = (num, den): accepted when ``den * cost < num * second``."""
    p = params or Params()
    num, den = int(ratio[0]), int(ratio[1])
    if not 0 < num <= den <= 32768:
        raise ValueError('match_map_global: the ratio must satisfy 0 < num <= den <= 32768, got {}'.format(tuple(ratio)))
    desc = np.asarray(descriptors, dtype=np.uint8).reshape(-1, 32)
    N, F = desc.shape[0], len(frame)
    feature = np.full(N, -1, dtype=np.int32)
    status = np.full(N, 2, dtype=np.int32)
    cost = np.full(N, -1, dtype=np.int32)
    second = np.full(N, -1, dtype=np.int32)
    uv = np.full((N, 2), -1.0)
    bd = frame.desc.astype(np.int16)
    for i in range(N if F else 0):
        c = np.abs(bd - desc[i].astype(np.int16)).sum(axis=1).astype(np.int64)
        j = int(np.argmin(c))                                  # first minimum: the lower feature index
        c1 = int(c[j])
        if c1 > int(p.match_cost_max):
            continue
        cost[i] = c1
        if F >= 2:
            c[j] = np.iinfo(np.int64).max
            second[i] = c2 = int(c.min())
            if den * c1 >= num * c2:
                status[i] = 4
                continue
        feature[i], status[i] = j, 0
    _claim_and_refine(frame, desc, feature, status, cost, uv, p)
    return feature, status, cost, second, uv


def db_query(entries, frame, ratio=(4, 5), params=None, first=0, last=None):
    """The keyframe database query (step 10) -> scores (last - first,) int32: for every entry e of ``entries[first:last]`` -- a list
    of (n_e, 32) uint8 descriptor arrays -- the number of its descriptors whose best cost over all features of ``frame`` is at most
    ``match_cost_max`` and, where the frame has a second feature, satisfies ``den * best < num * second-best``.  A count of the
    entry's descriptors, not of distinct features.  Written on its own, without match_map_global."""
    p = params or Params()
    num, den = int(ratio[0]), int(ratio[1])
    if not 0 < num <= den <= 32768:
        raise ValueError('db_query: the ratio must satisfy 0 < num <= den <= 32768, got {}'.format(tuple(ratio)))
    K = len(entries)
    last = K if last is None else int(last)
    first = int(first)
    if not 0 <= first <= last <= K:
        raise ValueError('db_query: the entry range must satisfy 0 <= first <= last <= {}, got [{}, {})'.format(K, first, last))
    F, cmax = len(frame), int(p.match_cost_max)
    scores = np.zeros(last - first, dtype=np.int32)
    if F == 0:
        return scores
    fd = frame.desc.astype(np.int32)
    for e in range(first, last):
        d = np.asarray(entries[e], dtype=np.uint8).reshape(-1, 32).astype(np.int32)
        for row in d:
            c = np.abs(fd - row).sum(axis=1)
            order = np.argsort(c, kind='stable')               # ties: the lower feature index first
            c1 = int(c[order[0]])
            if c1 > cmax:
                continue
            if F >= 2 and den * c1 >= num * int(c[order[1]]):
                continue
            scores[e - first] += 1
    return scores


class _Descriptors:
    """The one attribute _refine reads of its source frame."""

    def __init__(self, desc):
        self.desc = desc
