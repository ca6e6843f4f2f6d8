"""The feature matcher of the sparse VO pipelines, on the device.

``Matcher_parameters`` and ``Matcher`` are the two names reference pyslam/pipelines/sparse.py takes from ``viso2``;
the three calls it makes -- ``pushBack(left[, right])``, ``matchFeatures(mode)``, ``getMatches()`` -- behave as a
pipeline written for the reference expects, and a match has the attributes ``u1p v1p u2p v2p u1c v1c u2c v2c``.
The matcher is NOT libviso2: it is a front end of this project with an exact integer definition (DESIGN.md section 7;
numpy restatement: pipelines/featproc.py) that runs in the HIP core (include/pyslam_hip.h: ps_feat_*).  There is no
CPU path.

A pushed frame whose bytes equal a frame the matcher holds -- the previous one, the current one or one cached beside
them -- is not processed again: the pipelines push the active keyframe in front of every tracking frame.
``feature_passes`` counts the images whose features were computed.  ``matches_array()`` returns the matches as arrays
(the pipelines use it instead of building one Python object per match).

``setMap`` / ``matchMap`` are matching by projection (step 8 of the definition): the map's points, each with the
descriptor it was created with, against the features of the current frame around their projections under a pose prior.
``matchMapGlobal`` is matching without a prior (step 9): every map point against every feature, with a second-best ratio test.
``dbAdd`` / ``dbQuery`` are the keyframe database (step 10): per stored entry, the number of its descriptors that pass step 9's test
against the current frame, all entries in one launch.
"""
import ctypes as C

import numpy as np

from pyslam_amd import _native as nat

__all__ = ['Matcher_parameters', 'Matcher', 'Match']

_FIELDS = (('response_threshold', 1 << 36), ('nms_n', 2), ('max_features', 4096), ('match_radius_u', 200),
           ('match_radius_v', 50), ('disp_max', 160), ('match_cost_max', 1200), ('refinement', 1))


class Matcher_parameters:
    """Constants of the matcher's definition (the same fields and defaults as featproc.Params)."""

    def __init__(self, **kw):
        for k, v in _FIELDS:
            setattr(self, k, kw.pop(k, v))
        if kw:
            raise TypeError('unknown matcher parameters: {}'.format(sorted(kw)))

    def _native(self):
        return nat.FeatParams(*[int(getattr(self, k)) for k, _ in _FIELDS], 0)


class Match:
    """One match: pixel positions in the previous (p) and current (c) left (1) and right (2) images."""
    __slots__ = ('u1p', 'v1p', 'u2p', 'v2p', 'u1c', 'v1c', 'u2c', 'v2c', 'i1p', 'i2p', 'i1c', 'i2c')

    def __init__(self, row, idx):
        self.u1p, self.v1p, self.u2p, self.v2p, self.u1c, self.v1c, self.u2c, self.v2c = (float(x) for x in row)
        self.i1p, self.i2p, self.i1c, self.i2c = (int(x) for x in idx)


def _image(img, what):
    img = np.asarray(img)
    if img.ndim != 2 or img.dtype != np.uint8:
        raise TypeError('Matcher: {} must be a single-channel uint8 image, got {} {}'.format(what, img.dtype, img.shape))
    return np.ascontiguousarray(img)


class Matcher:
    def __init__(self, params=None, stream=None):
        self.params = params if params is not None else Matcher_parameters()
        self._stream = stream
        self._h = None
        self._shape = None
        self._lib = None
        self._n = 0
        self._passes_before = 0
        self._map = None            # (points_w, descriptors) of setMap, kept so that a rebuilt handle gets the map again
        self._map_on = None         # the handle the map was uploaded to
        self._db = []               # the entries of dbAdd, kept so that a rebuilt handle gets the database again
        self._db_on = None          # the handle the database was uploaded to

    def setIntrinsics(self, *args):
        """Accepted and ignored (libviso2 uses the calibration for its 3-D outlier checks; RANSAC follows here)."""

    def close(self):
        if self._h is not None:
            self._passes_before = self.feature_passes
            self._lib.ps_feat_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass

    def _handle(self, h, w):
        cap = int(self.params.max_features)
        if self._h is None or h > self._shape[0] or w > self._shape[1] or cap > self._shape[2]:
            self.close()
            self._lib = nat.require_gpu()
            hh = nat.H()
            shape = (max(h, self._shape[0]) if self._shape else h, max(w, self._shape[1]) if self._shape else w, cap)
            nat.check(self._lib.ps_feat_create(shape[0], shape[1], shape[2], C.c_void_p(self._stream or 0), C.byref(hh)))
            self._h, self._shape, self._n = hh, shape, 0
            self._db_on = self._h if not self._db else None     # an empty database is on every handle
        return self._h

    def pushBack(self, left, right=None):
        left = _image(left, 'the left image')
        if right is not None:
            right = _image(right, 'the right image')
            if right.shape != left.shape:
                raise ValueError('Matcher: left and right images differ in size')
        h, w = left.shape
        hd = self._handle(h, w)
        nat.check(self._lib.ps_feat_push(hd, h, w, left.ctypes.data_as(nat.c_u8p),
                                         right.ctypes.data_as(nat.c_u8p) if right is not None else None))
        self._n = 0

    def matchFeatures(self, mode):
        if self._h is None:
            raise nat.NativeError('Matcher: push the frames before matching')
        n = C.c_int32()
        p = self.params._native()
        nat.check(self._lib.ps_feat_match(self._h, int(mode), C.byref(p), C.byref(n)))
        self._n = n.value

    def matches_array(self):
        """(m, idx): (n, 8) float64 u1p v1p u2p v2p u1c v1c u2c v2c and (n, 4) int32 feature indices (1p 2p 1c 2c)."""
        m = np.zeros((self._n, 8))
        idx = np.zeros((self._n, 4), dtype=np.int32)
        if self._n:
            nat.check(self._lib.ps_feat_read_matches(self._h, self._n, nat.f64p(m), nat.i32p(idx)))
        return m, idx

    def getMatches(self):
        m, idx = self.matches_array()
        return [Match(m[k], idx[k]) for k in range(m.shape[0])]

    def features(self, which):
        """(uv (n, 2) int32, R (n,) int64, descriptors (n, 32) uint8) of image `which` after a match: 0 previous left,
        1 previous right, 2 current left, 3 current right."""
        cap = self._shape[2]
        uv = np.zeros((cap, 2), dtype=np.int32)
        R = np.zeros(cap, dtype=np.int64)
        d = np.zeros((cap, 32), dtype=np.uint8)
        n = C.c_int32()
        nat.check(self._lib.ps_feat_read_features(self._h, int(which), cap, C.byref(n), nat.i32p(uv),
                                                  R.ctypes.data_as(C.POINTER(C.c_int64)), d.ctypes.data_as(nat.c_u8p)))
        return uv[:n.value].copy(), R[:n.value].copy(), d[:n.value].copy()

    def setMap(self, points_w, descriptors):
        """The map of matching by projection: ``points_w`` (N, 3) float64 in the world frame and their descriptors (N, 32)
        uint8, as ``features`` returns them.  It stays on the device until the next ``setMap``."""
        pts = np.ascontiguousarray(np.asarray(points_w, dtype=np.float64).reshape(-1, 3))
        desc = np.asarray(descriptors)
        if desc.dtype != np.uint8:
            raise TypeError('Matcher: descriptors must be uint8, got {}'.format(desc.dtype))
        desc = np.ascontiguousarray(desc.reshape(-1, 32))
        if desc.shape[0] != pts.shape[0]:
            raise ValueError('Matcher: {} points and {} descriptors'.format(pts.shape[0], desc.shape[0]))
        self._map, self._map_on = (pts, desc), None
        if self._h is not None:
            self._upload_map()

    def _upload_map(self):
        pts, desc = self._map
        nat.check(self._lib.ps_feat_set_map(self._h, pts.shape[0], nat.f64p(pts), desc.ctypes.data_as(nat.c_u8p)))
        self._map_on = self._h

    def matchMap(self, T_cw, camera, radius):
        """The map's points matched into the current frame's (left) image by projection with the pose prior ``T_cw`` (4 x 4
        or an SE3) and ``camera`` (an object with cu cv fu fv, or a tuple beginning with them), inside a window of ``radius``
        pixels around every projection -> ``(feature, status, cost, uv)``, one entry per map point: feature index or -1,
        status 0 matched / 1 not visible / 2 no candidate / 3 lost its feature to a better point, cost (-1 unless the status
        is 0 or 3), position (N, 2) with the sub-pixel refinement (-1 unless the status is 0)."""
        if self._h is None:
            raise nat.NativeError('Matcher: push a frame before matching the map')
        if self._map is not None and self._map_on is not self._h:
            self._upload_map()
        T = np.ascontiguousarray(T_cw.as_matrix() if hasattr(T_cw, 'as_matrix') else T_cw, dtype=np.float64).reshape(4, 4)
        cam = np.zeros(5)
        cam[:4] = [camera.cu, camera.cv, camera.fu, camera.fv] if hasattr(camera, 'cu') else [float(c) for c in tuple(camera)[:4]]
        n = C.c_int32()
        p = self.params._native()
        nat.check(self._lib.ps_feat_match_map(self._h, nat.f64p(T), nat.f64p(cam), int(radius), C.byref(p), C.byref(n)))
        self.num_map_matched = n.value
        N = self._map[0].shape[0]
        feature, status, cost = (np.zeros(N, dtype=np.int32) for _ in range(3))
        uv = np.zeros((N, 2))
        if N:
            nat.check(self._lib.ps_feat_read_map_matches(self._h, N, nat.i32p(feature), nat.i32p(status), nat.i32p(cost), nat.f64p(uv)))
        return feature, status, cost, uv

    def matchMapGlobal(self, ratio=(4, 5)):
        """The map's points matched into the current frame's (left) image without a pose: every point against every feature,
        accepted when ``ratio[1] * cost < ratio[0] * second-best cost`` (integers, ``0 < num <= den <= 32768``) ->
        ``(feature, status, cost, second, uv)``, one entry per map point: feature index or -1, status 0 matched / 2 no feature
        within ``match_cost_max`` / 3 lost its feature to a better point / 4 ambiguous, best and second-best cost (-1 for status
        2, ``second`` also where the frame has one feature), position (N, 2) with the sub-pixel refinement (-1 unless the status
        is 0)."""
        if self._h is None:
            raise nat.NativeError('Matcher: push a frame before matching the map')
        if self._map is not None and self._map_on is not self._h:
            self._upload_map()
        n = C.c_int32()
        p = self.params._native()
        nat.check(self._lib.ps_feat_match_map_global(self._h, int(ratio[0]), int(ratio[1]), C.byref(p), C.byref(n)))
        self.num_map_matched = n.value
        N = self._map[0].shape[0]
        feature, status, cost, second = (np.zeros(N, dtype=np.int32) for _ in range(4))
        uv = np.zeros((N, 2))
        if N:
            nat.check(self._lib.ps_feat_read_map_matches(self._h, N, nat.i32p(feature), nat.i32p(status), nat.i32p(cost), nat.f64p(uv)))
            nat.check(self._lib.ps_feat_read_map_second(self._h, N, nat.i32p(second)))
        return feature, status, cost, second, uv

    def _desc(self, descriptors):
        desc = np.asarray(descriptors)
        if desc.dtype != np.uint8:
            raise TypeError('Matcher: descriptors must be uint8, got {}'.format(desc.dtype))
        return np.ascontiguousarray(desc.reshape(-1, 32))

    def _upload_db(self):
        if self._db_on is not None:
            return
        for desc in self._db:
            e = C.c_int32()
            nat.check(self._lib.ps_feat_db_add(self._h, desc.shape[0], desc.ctypes.data_as(nat.c_u8p) if desc.shape[0] else None,
                                               C.byref(e)))
        self._db_on = self._h

    def dbAdd(self, descriptors):
        """Appends one entry -- (n, 32) uint8 descriptors as ``features`` returns them, n >= 0 -- to the keyframe database and
        returns its index.  Entries are never edited; ``dbClear`` empties the database."""
        desc = self._desc(descriptors)
        if self._h is not None and self._db_on is self._h:
            e = C.c_int32()
            nat.check(self._lib.ps_feat_db_add(self._h, desc.shape[0], desc.ctypes.data_as(nat.c_u8p) if desc.shape[0] else None,
                                               C.byref(e)))
            assert e.value == len(self._db)
        elif len(self._db) >= 65536 or sum(d.shape[0] for d in self._db) + desc.shape[0] > 1 << 22:
            raise nat.NativeError('Matcher: the database holds at most 65536 entries and 2^22 descriptors')
        self._db.append(desc)
        return len(self._db) - 1

    def dbClear(self):
        self._db = []
        if self._h is not None and self._db_on is self._h:
            nat.check(self._lib.ps_feat_db_clear(self._h))

    def dbSize(self):
        """(entries, descriptors) of the keyframe database."""
        if self._h is not None and self._db_on is self._h:
            k, n = C.c_int32(), C.c_int64()
            nat.check(self._lib.ps_feat_db_size(self._h, C.byref(k), C.byref(n)))
            return k.value, n.value
        return len(self._db), sum(d.shape[0] for d in self._db)

    def dbQuery(self, ratio=(4, 5), first=0, last=None):
        """Scores (last - first,) int32 of the database's entries ``first .. last - 1`` (default: all) against the current frame's
        (left) image: per entry, the number of its descriptors whose best cost over all features is at most ``match_cost_max`` and
        satisfies ``ratio[1] * cost < ratio[0] * second-best cost`` -- what ``matchMapGlobal`` gives status 0 or 3 with the entry
        as the map.  One launch for the whole range."""
        if self._h is None:
            raise nat.NativeError('Matcher: push a frame before querying the database')
        self._upload_db()
        last = len(self._db) if last is None else int(last)
        scores = np.zeros(max(last - int(first), 1), dtype=np.int32)
        p = self.params._native()
        nat.check(self._lib.ps_feat_db_query(self._h, int(first), last, int(ratio[0]), int(ratio[1]), C.byref(p), nat.i32p(scores)))
        return scores[:max(last - int(first), 0)]

    @property
    def feature_passes(self):
        """Number of images whose features were computed (a frame the matcher already holds adds none)."""
        if self._h is None:
            return self._passes_before
        n = C.c_int64()
        nat.check(self._lib.ps_feat_feature_passes(self._h, C.byref(n)))
        return self._passes_before + n.value

    @property
    def device_bytes(self):
        n = C.c_int64()
        nat.check(self._lib.ps_feat_device_bytes(self._h, C.byref(n)))
        return n.value
