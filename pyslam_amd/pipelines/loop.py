"""Loop detection for the monocular pipeline: which old keyframe does this frame look like, and by what similarity do the two views
of the place differ?  ``loop_candidates``, ``verify_loop`` and ``detect_loop``.

The reference has no counterpart.  Everything is a composition of pieces that run on the device and are pinned one by one: the
matcher's keyframe database (``Matcher.dbAdd`` / ``dbQuery``, DESIGN.md section 7 step 10: per stored keyframe the number of its
descriptors that pass step 9's test against the frame, all keyframes in one launch), matching without a prior (``setMap`` /
``matchMapGlobal``, step 9) and ``Sim3RANSAC``.  There is no CPU path.  Nothing here corrects a map: a hit is the constraint
``p_query = scale R p_entry + t`` between two camera frames that the Sim(3) pose graph (pipelines/posegraph.py) consumes.

An *entry* is what a caller keeps of a keyframe, as a mapping or an object with ``desc`` (n, 32) uint8, ``points_c`` (n, 3) -- the
features' landmarks in the keyframe's camera frame, non-finite rows for features without one -- ``uv`` (n, 2) and optionally ``ids``
(n,): the landmark index of every feature, negative for none."""
import numpy as np

from pyslam_amd.pipelines.sim3 import Sim3RANSAC

__all__ = ['loop_candidates', 'verify_loop', 'detect_loop', 'MIN_SCORE']

MIN_SCORE = 12           # Sim3RANSAC.min_inliers: fewer accepted descriptors cannot yield that many inliers (a floor, not a tuned value)


def loop_candidates(scores, first=0, min_score=MIN_SCORE, max_candidates=3):
    """Entry indices (``first`` + position in ``scores``) of the entries with ``score >= min_score``, by descending score with ties
    to the lower index, at most ``max_candidates``.  Empty scores give no candidates."""
    s = np.asarray(scores)
    if s.ndim != 1:
        raise ValueError('loop_candidates: scores must be one-dimensional, got shape {}'.format(s.shape))
    if int(max_candidates) < 0:
        raise ValueError('loop_candidates: max_candidates must not be negative')
    order = np.argsort(-s.astype(np.int64), kind='stable')
    order = order[s[order] >= min_score][:int(max_candidates)]
    return order.astype(np.int64) + int(first)


def _field(entry, name, default=None):
    if isinstance(entry, dict):
        return entry.get(name, default)
    return getattr(entry, name, default)


def _entry_arrays(entry):
    desc = np.asarray(_field(entry, 'desc'))
    if desc.dtype != np.uint8:
        raise TypeError('verify_loop: the entry\'s descriptors must be uint8, got {}'.format(desc.dtype))
    desc = desc.reshape(-1, 32)
    pts = np.asarray(_field(entry, 'points_c'), dtype=np.float64).reshape(-1, 3)
    uv = np.asarray(_field(entry, 'uv'), dtype=np.float64).reshape(-1, 2)
    ids = _field(entry, 'ids')
    ids = None if ids is None else np.asarray(ids, dtype=np.int64).reshape(-1)
    n = desc.shape[0]
    if pts.shape[0] != n or uv.shape[0] != n or (ids is not None and ids.shape[0] != n):
        raise ValueError('verify_loop: the entry holds {} descriptors, {} points, {} positions{}'.format(
            n, pts.shape[0], uv.shape[0], '' if ids is None else ' and {} ids'.format(ids.shape[0])))
    return desc, pts, uv, ids


def verify_loop(camera, matcher, entry, points_q, ids_q=None, ratio=(4, 5), seed=None, ransac=None):
    """The similarity between an entry and the frame the matcher currently holds -> ``(scale, T_21: SE3, pairs)`` with
    ``p_query = scale R p_entry + t`` and ``pairs`` (n, 2) the (entry row, frame feature) of the inliers.

    ``points_q`` (F, 3) are the frame's features' landmarks in its camera frame (non-finite: none), ``ids_q`` (F,) their indices.  The
    entry's landmark rows become the matcher's map; of the status-0 rows of ``matchMapGlobal(ratio)`` the pairs whose frame feature has
    a landmark are kept; the pairs whose two ids are equal and >= 0 are dropped and counted as ``connected`` (the map joins these
    points already: they say nothing about drift); ``Sim3RANSAC(camera)`` (or ``ransac``) runs over the rest, scored in both images.
    ``seed`` seeds ``np.random`` first.  ValueError where Sim3RANSAC raises it or fewer than 3 pairs remain.  The counts stay on
    ``matcher.loop_info_``: matched, bound, connected, pairs, inliers (None when it raised)."""
    desc, pts_e, uv_e, ids_e = _entry_arrays(entry)
    pts_q = np.asarray(points_q, dtype=np.float64).reshape(-1, 3)
    if ids_q is not None:
        ids_q = np.asarray(ids_q, dtype=np.int64).reshape(-1)
        if ids_q.shape[0] != pts_q.shape[0]:
            raise ValueError('verify_loop: {} points and {} ids of the frame'.format(pts_q.shape[0], ids_q.shape[0]))
    rows = np.nonzero(np.isfinite(pts_e).all(axis=1))[0]
    info = dict(matched=0, bound=0, connected=0, pairs=0, inliers=None)
    matcher.loop_info_ = info
    matcher.setMap(pts_e[rows], desc[rows])
    feature, status, _, _, uv = matcher.matchMapGlobal(ratio)
    m = np.nonzero(status == 0)[0]
    info['matched'] = int(m.size)
    if m.size and int(feature[m].max()) >= pts_q.shape[0]:
        raise ValueError('verify_loop: the frame has more features than points_q has rows ({})'.format(pts_q.shape[0]))
    m = m[np.isfinite(pts_q[feature[m]]).all(axis=1)]
    info['bound'] = int(m.size)
    if ids_e is not None and ids_q is not None and m.size:
        a, b = ids_e[rows[m]], ids_q[feature[m]]
        same = (a == b) & (a >= 0)
        info['connected'] = int(same.sum())
        m = m[~same]
    info['pairs'] = int(m.size)
    if m.size < 3:
        raise ValueError('verify_loop: a similarity needs at least 3 pairs, {} remain'.format(m.size))
    rs = ransac if ransac is not None else Sim3RANSAC(camera)
    rs.set_obs(pts_e[rows[m]], pts_q[feature[m]], uv_e[rows[m]], uv[m])
    if seed is not None:
        np.random.seed(seed)
    scale, T_21, inl = rs.perform_ransac()
    info['inliers'] = int(len(inl))
    return scale, T_21, np.stack([rows[m[inl]], feature[m[inl]].astype(np.int64)], axis=1)


def detect_loop(camera, matcher, image, points_q, entries, first=0, last=None, ids_q=None, ratio=(4, 5), min_score=MIN_SCORE,
                max_candidates=3, seed=None, ransac=None):
    """One image against the matcher's keyframe database -> ``(entry index, scale, T_21, pairs)`` of the first candidate that
    verifies, or None.  ``pushBack(image)``, ``dbQuery(ratio, first, last)``, ``loop_candidates`` and ``verify_loop`` per candidate in
    order.  ``entries`` is indexed by entry index (``entries[e]``: see the module docstring); ``points_q`` may be a callable
    ``uv (F, 2) int -> (F, 3)``, called once after the feature pass when there is a candidate.  The scores, the candidates and every
    verification's counts stay on ``matcher.loop_query_``."""
    matcher.pushBack(image)
    scores = matcher.dbQuery(ratio, first, last)
    cand = loop_candidates(scores, first, min_score, max_candidates)
    query = dict(scores=scores, candidates=cand, verified=[])
    matcher.loop_query_ = query
    if cand.size and callable(points_q):
        points_q = points_q(matcher.features(2)[0])
    for e in cand:
        try:
            scale, T_21, pairs = verify_loop(camera, matcher, entries[int(e)], points_q, ids_q, ratio, seed, ransac)
        except ValueError:
            query['verified'].append((int(e), matcher.loop_info_))
            continue
        query['verified'].append((int(e), matcher.loop_info_))
        return int(e), scale, T_21, pairs
    return None
