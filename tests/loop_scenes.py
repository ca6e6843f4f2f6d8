"""The committed scenes, seeds and host compositions of the loop-detection tests (tests/test_loop_host.py checks the conditions that
tests/test_gpu_feat_db.py and tests/test_gpu_loop.py rely on; all three import this module).  Every restatement result is computed once
and shared; callers do not modify what they get.

Written out here with the restatements only (featproc, similarity), no device call: ``brute_force`` (step 10 as a dense cost matrix,
independent of featproc.db_query's loop), ``places_scores`` (the places scene) and ``host_visit`` (loop.verify_loop on the two-visits
scene: featproc.match_map_global, then similarity.ransac with the samples Sim3RANSAC draws from the committed seed)."""
import functools

import numpy as np

import mono_scenes as ms
import sim3_scenes as s3
from pyslam_amd import synthetic
from pyslam_amd.pipelines import featproc as fp
from pyslam_amd.pipelines import similarity as sm

# ---- places: six different scenes, frame 0 of each in the database, three later frames of each as queries
PLACE_SEEDS = tuple(range(6))
PLACE_QUERIES = (1, 4, 7)
PLACE_MARGIN = 1.5                                  # the right seed's score over the best wrong seed's (the issue's bound)

# ---- the kernel's shapes (k_feat_db_search: 64 descriptors per workgroup, a workgroup within one entry, tiles of 512 features in quarters)
ENTRY_SIZES = (0, 1, 63, 64, 65, 129, 0, 200)
FRAME_SIZES = (0, 1, 2, 127, 128, 129, 511, 512, 513)
RANGES = ((0, 8), (2, 5), (3, 3), (7, 8))           # [0, K), [2, 5), [3, 3), [K - 1, K)
RATIOS = ((4, 5), (1, 1), (1, 32768))
COST_MAX = (0, 1200, 8160)
KERNEL_KW = dict(nms_n=1, response_threshold=0)     # about 275 features per 96 x 128 image: the 2 x 2 mosaic holds two tiles and more
N_PLANTED = 3                                       # per entry: exact copies of frame descriptors, and of each other

# ---- two visits: the same place seen from frame 0 and from frame f, the second time in a map 1.3 times as large
VISIT_FRAMES = (3, 7, 9)
VISIT_SCALE = 1.3
VISIT_SEED = 1                                      # np.random.seed of verify_loop (Sim3RANSAC.draw_samples: 400 x 3)
VISIT_THRESH = 9.0                                  # Sim3RANSAC(camera).ransac_thresh
# truth bounds of host_visit: twice the largest error measured with the restatement chain and VISIT_SEED over the three frames, rounded
# up in the last digit -- (|scale - 1.3|, rotation in degrees, |t - 1.3 t_rel|); test_loop_host.test_two_visits_host_chain prints the
# figures.  Measured at 96 x 128: 0.0029414, 0.22117 deg, 0.030189 (67 - 85 pairs, 61 - 80 inliers); at 240 x 320: 0.00047729,
# 0.046846 deg, 0.0051819 (254 - 332 pairs, 184 - 265 inliers).  No pair's error lies within sim3_scenes.MARGIN of the threshold.
TRUTH_BOUND = {'small': (2 * 0.00295, 2 * 0.222, 2 * 0.0302), 'big': (2 * 0.000478, 2 * 0.0469, 2 * 0.00519)}
NOT_MOVED = 0.49                                    # the measured maximum is not below this share of its bound

# ---- the negative: the 240 x 320 images out and back
LOOP_GAP = 3
OUT_AND_BACK_KEYFRAMES = [0, 1, 5, 9, 12, 16]       # images at which the host pipeline makes its keyframes


@functools.lru_cache(maxsize=None)
def place_sequence(seed):
    return synthetic.mono_sequence(96, 128, 8, seed=seed, edge=0.35)


@functools.lru_cache(maxsize=None)
def place_frame(seed, f, **kw):
    return fp.features(place_sequence(seed)['images'][f], fp.Params(**kw))


@functools.lru_cache(maxsize=None)
def places_db():
    """Frame 0 of every seed: a list of (n, 32) descriptor arrays."""
    return [place_frame(s, 0).desc for s in PLACE_SEEDS]


@functools.lru_cache(maxsize=None)
def places_scores():
    """{(seed, frame): featproc.db_query of the places database against that frame}."""
    return {(s, f): fp.db_query(places_db(), place_frame(s, f)) for s in PLACE_SEEDS for f in PLACE_QUERIES}


# ---- the kernel test
def kernel_image(F):
    """The query image of the kernel test: frame 1 of the places 0 .. 3 as a 2 x 2 mosaic (192 x 256); a flat image for F = 0."""
    if F == 0:
        return np.full((192, 256), 117, dtype=np.uint8)
    im = [place_sequence(s)['images'][1] for s in range(4)]
    return np.ascontiguousarray(np.block([[im[0], im[1]], [im[2], im[3]]]))


@functools.lru_cache(maxsize=None)
def kernel_params(F, cost_max=1200):
    return fp.Params(max_features=max(F, 1), match_cost_max=cost_max, **KERNEL_KW)


@functools.lru_cache(maxsize=None)
def kernel_frame(F):
    fr = fp.features(kernel_image(F), kernel_params(F))
    assert len(fr) == F, (len(fr), F)
    return fr


@functools.lru_cache(maxsize=None)
def kernel_entries():
    """Entries of ENTRY_SIZES descriptors: frame 0 of the places 0, 1, ... under KERNEL_KW, each strongest first (the points the query
    mosaic shows a frame later, so a share passes the ratio test), each entry's last N_PLANTED rows replaced by exact copies of
    query-frame descriptors:
    two copies of its strongest feature (cost 0 under every F >= 1, and an accepted descriptor twice over: the score counts
    descriptors) and one of a feature that only the larger F hold."""
    parts = [place_frame(p, 0, max_features=4096, **KERNEL_KW) for p in range(4)]
    desc = np.concatenate([fr.desc[np.argsort(-fr.R, kind='stable')] for fr in parts])
    q = kernel_frame(FRAME_SIZES[-1])
    top, late = q.desc[int(np.argmax(q.R))], q.desc[int(np.argmin(q.R))]
    out, at = [], 0
    for n in ENTRY_SIZES:
        d = desc[at:at + n].copy()
        at += n
        if n >= 63:
            d[-N_PLANTED:] = [top, top, late]
        elif n == 1:
            d[0] = top
        out.append(d)
    assert at <= desc.shape[0]
    return out


def brute_force(entries, frame, ratio, cost_max):
    """Step 10 per entry from the full cost matrix: argmin, the second minimum by masking -> (scores, descriptors whose minimum is
    reached by more than one feature, descriptors with c1 = c2, descriptors with den c1 = num c2 exactly)."""
    F = len(frame)
    scores, tied, equal, edge = np.zeros(len(entries), dtype=np.int32), 0, 0, 0
    for e, d in enumerate(entries):
        n = d.shape[0]
        if n == 0 or F == 0:
            continue
        C = np.abs(d.astype(np.int64)[:, None, :] - frame.desc.astype(np.int64)[None, :, :]).sum(axis=2)
        best = C.argmin(axis=1)
        c1 = C[np.arange(n), best]
        ok = c1 <= cost_max
        if F >= 2:
            masked = C.copy()
            masked[np.arange(n), best] = np.iinfo(np.int64).max
            c2 = masked.min(axis=1)
            tied += int(((C == c1[:, None]).sum(axis=1) > 1).sum())
            equal += int((c1 == c2).sum())
            edge += int((ratio[1] * c1 == ratio[0] * c2).sum())
            ok &= ratio[1] * c1 < ratio[0] * c2
        scores[e] = ok.sum()
    return scores, tied, equal, edge


@functools.lru_cache(maxsize=None)
def kernel_reference(F, ratio, cost_max):
    """featproc.db_query over all entries of the kernel test."""
    return fp.db_query(kernel_entries(), kernel_frame(F), ratio, kernel_params(F, cost_max))


# ---- two visits
@functools.lru_cache(maxsize=None)
def visit_sequence(size):
    return ms.sequence() if size == 'big' else synthetic.mono_sequence(96, 128, 10, seed=0, edge=0.35)


@functools.lru_cache(maxsize=None)
def visit_frame(size, f):
    return fp.features(visit_sequence(size)['images'][f], fp.Params())


def true_points(seq, f, uv, scale=1.0):
    """The pixels uv of frame f at their true depth, in that frame's camera frame, times ``scale``."""
    cu, cv, fu, fv = seq['cam'][:4]
    u, v = uv[:, 0], uv[:, 1]
    z = seq['depth'][f][v, u]
    return scale * np.stack([(u - cu) * z / fu, (v - cv) * z / fv, z], axis=1)


@functools.lru_cache(maxsize=None)
def visit_entry(size):
    """Visit 1 as an entry of loop.verify_loop: frame 0's features at their true depth in its camera frame."""
    seq, f0 = visit_sequence(size), visit_frame(size, 0)
    return dict(desc=f0.desc, points_c=true_points(seq, 0, f0.uv), uv=f0.uv)


def visit_points(size, f, uv=None):
    """Visit 2's features (or the pixels uv) at their true depth in frame f's camera frame, in a map VISIT_SCALE times as large."""
    return true_points(visit_sequence(size), f, visit_frame(size, f).uv if uv is None else uv, VISIT_SCALE)


def visit_truth(size, f):
    """(scale, R, t) with p_visit2 = scale R p_visit1 + t."""
    seq = visit_sequence(size)
    T = seq['T_c_w'][f] @ np.linalg.inv(seq['T_c_w'][0])
    return VISIT_SCALE, T[:3, :3], VISIT_SCALE * T[:3, 3]


@functools.lru_cache(maxsize=None)
def visit_db(size):
    """Descriptor arrays of the database: visit 1, and in the small case frame 0 of the places 1 .. 5 behind it."""
    db = [visit_entry(size)['desc']]
    return db + places_db()[1:] if size == 'small' else db


@functools.lru_cache(maxsize=None)
def host_visit(size, f, seed=VISIT_SEED):
    """loop.verify_loop of visit 1 against frame f with the restatements -> dict: pairs (entry row, frame feature) of the status-0
    rows, uv (their matched positions), res (similarity.ransac's result), inlier_pairs, and the errors against the truth."""
    seq, entry, fr = visit_sequence(size), visit_entry(size), visit_frame(size, f)
    feature, status, _, _, uv = fp.match_map_global(fr, entry['desc'], (4, 5))
    m = np.nonzero(status == 0)[0]
    pairs = np.stack([m, feature[m].astype(np.int64)], axis=1)
    p1, p2 = entry['points_c'][m], visit_points(size, f)[feature[m]]
    o1, o2 = entry['uv'][m].astype(np.float64), uv[m]
    res = sm.ransac(p1, p2, o1, o2, ms.cam5(seq['cam']), s3.draw_samples(m.size, 400, seed), VISIT_THRESH)
    out = dict(pairs=pairs, uv=uv[m], res=res, inlier_pairs=pairs[res['mask']])
    out.update(visit_errors(res['scale'], res['S_21'][:3, :3] / res['scale'], res['S_21'][:3, 3], size, f))
    return out


def visit_errors(scale, R, t, size, f):
    s_t, R_t, t_t = visit_truth(size, f)
    return dict(e_scale=abs(scale - s_t), e_rot_deg=float(np.degrees(s3.rot_angle(R, R_t))), e_t=float(np.linalg.norm(t - t_t)))


# ---- the negative
@functools.lru_cache(maxsize=None)
def out_and_back():
    """The 240 x 320 images 0 .. 9 and back 8 .. 0: the camera returns to where it started, through a map that joins the two ends
    already (the landmarks of the first keyframes are tracked again on the way back)."""
    images = list(ms.sequence()['images'])
    return images + images[-2::-1]


@functools.lru_cache(maxsize=None)
def host_out_and_back():
    """mono_scenes.host_pipeline (``local_ba`` off, PIPELINE_SEED) over out_and_back()."""
    return ms.host_pipeline(out_and_back(), ms.sequence()['cam'])
