"""Loop detection on the host: the restatement of the keyframe database query (featproc.db_query)
against a brute force and against step 9, the places and two-visits scenes of tests/loop_scenes.py with the figures the GPU tests rely
on, and the surface (header, signature table, INTEGRATION.md, exports, pipeline attributes, errors that need no device)."""
import os
import re

import numpy as np
import pytest

import loop_scenes as ls
import mono_scenes as ms
import sim3_scenes as s3
from pyslam_amd.pipelines import featproc as fp

HERE = os.path.dirname(os.path.abspath(__file__))
CALLS = (('ps_feat_db_add', 4), ('ps_feat_db_clear', 1), ('ps_feat_db_size', 3), ('ps_feat_db_query', 7))


# ---- the restatement ----

@pytest.mark.parametrize('F', ls.FRAME_SIZES)
def test_db_query_equals_the_brute_force(F):
    seen = np.zeros(3, dtype=np.int64)
    for ratio in ls.RATIOS:
        for cost_max in ls.COST_MAX:
            scores, tied, equal, edge = ls.brute_force(ls.kernel_entries(), ls.kernel_frame(F), ratio, cost_max)
            ref = ls.kernel_reference(F, ratio, cost_max)
            assert ref.dtype == np.int32 and ref.shape == (len(ls.ENTRY_SIZES),)
            assert np.array_equal(ref, scores), (F, ratio, cost_max, ref, scores)
            assert ref[0] == 0 and ref[6] == 0                                 # the entries without a descriptor
            seen += (tied, equal, edge)
    print('F = {}: descriptors whose minimum two features reach / with c1 = c2 / with den c1 = num c2, over the 9 settings: {}'.format(
        F, seen.tolist()))


def test_ties_equal_costs_and_every_outcome_occur_in_the_compared_cases():
    tied = equal = 0
    for F in ls.FRAME_SIZES:
        _, t, e, _ = ls.brute_force(ls.kernel_entries(), ls.kernel_frame(F), (4, 5), 1200)
        tied, equal = tied + t, equal + e
    assert tied > 0 and equal > 0
    ref = ls.kernel_reference(513, (4, 5), 1200)
    sizes = np.array(ls.ENTRY_SIZES)
    assert (ref[sizes >= 63] > 0).all() and (ref[sizes >= 63] < sizes[sizes >= 63]).all()      # accepted and refused, in every entry
    # the planted copies: cost 0 is within every match_cost_max, and two copies of one descriptor count twice
    assert ls.kernel_reference(1, (4, 5), 0).tolist() == [0, 1, 2, 2, 2, 2, 0, 2]
    # one feature: no second best, the cost bound alone decides; at 8 160 = 32 x 255 it refuses nothing
    assert ls.kernel_reference(1, (1, 32768), 8160).tolist() == list(ls.ENTRY_SIZES)


@pytest.mark.parametrize('F', ls.FRAME_SIZES)
def test_db_query_equals_the_count_of_step_9s_statuses_0_and_3(F):
    for ratio in ls.RATIOS:
        for cost_max in ls.COST_MAX:
            p = ls.kernel_params(F, cost_max)
            for e, d in enumerate(ls.kernel_entries()):
                status = fp.match_map_global(ls.kernel_frame(F), d, ratio, p)[1]
                assert int(((status == 0) | (status == 3)).sum()) == ls.kernel_reference(F, ratio, cost_max)[e], (F, ratio, cost_max, e)


def test_a_range_is_a_slice_and_an_empty_range_is_valid():
    fr, ents = ls.kernel_frame(129), ls.kernel_entries()
    full = ls.kernel_reference(129, (4, 5), 1200)
    for first, last in ls.RANGES:
        out = fp.db_query(ents, fr, (4, 5), ls.kernel_params(129), first, last)
        assert out.shape == (last - first,) and np.array_equal(out, full[first:last])
    assert fp.db_query([], fr).shape == (0,)


# ---- the places ----

def test_every_query_finds_its_own_place():
    lo, hi_wrong, worst = 10 ** 9, 0, np.inf
    for (s, f), scores in ls.places_scores().items():
        wrong = int(np.delete(scores, s).max())
        assert int(np.argmax(scores)) == s, (s, f, scores)
        assert scores[s] >= ls.PLACE_MARGIN * wrong, (s, f, scores)
        lo, hi_wrong, worst = min(lo, int(scores[s])), max(hi_wrong, wrong), min(worst, scores[s] / wrong)
    print('right place {} and more, best wrong place {} at most, smallest ratio within a query {:.2f}'.format(lo, hi_wrong, worst))
    assert lo >= 12                                          # loop_candidates' floor keeps every right place


# ---- two visits ----

@pytest.mark.parametrize('size', ['small', 'big'])
def test_two_visits_host_chain(size):
    worst = np.zeros(3)
    for f in ls.VISIT_FRAMES:
        h = ls.host_visit(size, f)
        res = h['res']
        c = s3.conditions(res, ls.VISIT_THRESH)
        err = np.array([h['e_scale'], h['e_rot_deg'], h['e_t']])
        print('{} frame {}: {} pairs, {} inliers, scale {:.6f}, errors {:.5g} / {:.5g} deg / {:.5g}; pairs in the margin {} + {}'.format(
            size, f, len(h['pairs']), res['count'], res['scale'], err[0], err[1], err[2], c['near'], c['near_final']))
        assert res['count'] >= 12 and not res['degenerate']
        assert c['near'] == 0 and c['near_final'] == 0       # no count hinges on a rounding
        assert (err <= ls.TRUTH_BOUND[size]).all(), (f, err)
        worst = np.maximum(worst, err)
    assert (worst >= ls.NOT_MOVED * np.array(ls.TRUTH_BOUND[size])).all(), worst           # the bounds are twice what is measured


def test_the_database_query_ranks_visit_1_first():
    db = ls.visit_db('small')
    for f in ls.VISIT_FRAMES:
        scores = fp.db_query(db, ls.visit_frame('small', f))
        assert int(np.argmax(scores)) == 0 and scores[0] >= 12 and scores[0] >= ls.PLACE_MARGIN * scores[1:].max(), (f, scores)


# ---- the negative ----

def test_the_host_pipeline_out_and_back():
    run = ls.host_out_and_back()
    print('host pipeline out and back: keyframes {}, landmarks {}'.format(run['keyframes'], run['counts']))
    assert run['keyframes'] == ls.OUT_AND_BACK_KEYFRAMES and all(T is not None for T in run['poses'])
    assert len(run['keyframes']) - 1 - ls.LOOP_GAP > 0       # the last keyframe queries the first two
    # at image 15 one pair's error lies within the rounding margin of the RANSAC threshold, so the device run need not equal this
    # one decision for decision: tests/test_gpu_loop.py holds the device run against itself (switch on / off), not against this
    close = [c for c in run['checks'] if c['near'] or c.get('margin', 1.) < ms.ROUND_MARGIN]
    print('decisions within a rounding of flipping: {}'.format(close))


# ---- the surface ----

def test_the_header_the_signature_table_and_the_integration_guide_hold_the_four_calls():
    from pyslam_amd import _native as nat
    header = open(os.path.join(HERE, '..', 'include', 'pyslam_hip.h')).read()
    guide = open(os.path.join(HERE, '..', 'INTEGRATION.md')).read()
    for name, nargs in CALLS:
        decl = re.search(r'int {}\(([^)]*)\);'.format(name), header)
        assert decl and len(decl.group(1).split(',')) == nargs == len(nat.SIGNATURES[name][1]), name
        call = re.search(r'`{}\(([^)]*)\)`'.format(name), guide)
        assert call and len(call.group(1).split(',')) == nargs, name


def test_the_exports_and_the_pipeline_attributes():
    import pyslam.pipelines
    import pyslam.pipelines.loop as shim
    import pyslam_amd.pipelines
    from pyslam_amd.pipelines import loop, mono
    from pyslam_amd.pipelines.matcher import Matcher
    for name in ('loop_candidates', 'verify_loop', 'detect_loop'):
        assert name in loop.__all__
        assert getattr(shim, name) is getattr(loop, name) is getattr(pyslam.pipelines, name) is getattr(pyslam_amd.pipelines, name)
    assert 'db_query' in fp.__all__
    for name in ('dbAdd', 'dbClear', 'dbSize', 'dbQuery'):
        assert callable(getattr(Matcher, name))
    p = mono.SparseMonoPipeline(ms.camera(ms.sequence(96, 128)['cam']))
    assert p.loop_detection is False and p.loop_gap == 10 and p.loop_ratio == (4, 5) and p.loop_closures == []
    assert loop.MIN_SCORE == 12


def test_loop_candidates():
    from pyslam_amd.pipelines.loop import loop_candidates
    assert loop_candidates(np.zeros(0, dtype=np.int32)).shape == (0,)
    s = np.array([30, 11, 40, 12, 40, 13], dtype=np.int32)
    assert loop_candidates(s).tolist() == [2, 4, 0]                            # descending, ties to the lower index
    assert loop_candidates(s, first=5, max_candidates=10).tolist() == [7, 9, 5, 10, 8]
    assert loop_candidates(s, min_score=41).tolist() == [] and loop_candidates(s, max_candidates=0).tolist() == []
    with pytest.raises(ValueError, match='one-dimensional'):
        loop_candidates(np.zeros((2, 2)))


def test_errors_that_need_no_device():
    from pyslam_amd import _native as nat
    from pyslam_amd.pipelines.loop import verify_loop
    from pyslam_amd.pipelines.matcher import Matcher
    fr, ents = ls.kernel_frame(2), ls.kernel_entries()
    for ratio in ((0, 5), (6, 5), (4, 32769), (-1, 1)):
        with pytest.raises(ValueError, match='ratio'):
            fp.db_query(ents, fr, ratio)
    for first, last in ((-1, 2), (3, 2), (0, 9)):
        with pytest.raises(ValueError, match='range'):
            fp.db_query(ents, fr, first=first, last=last)
    cam = ms.camera(ms.sequence(96, 128)['cam'])
    entry = dict(desc=np.zeros((4, 32), dtype=np.uint8), points_c=np.zeros((3, 3)), uv=np.zeros((4, 2)))
    with pytest.raises(ValueError, match='4 descriptors, 3 points'):
        verify_loop(cam, None, entry, np.zeros((5, 3)))
    entry['points_c'] = np.zeros((4, 3))
    with pytest.raises(ValueError, match='5 points and 4 ids'):
        verify_loop(cam, None, entry, np.zeros((5, 3)), ids_q=np.zeros(4))
    m = Matcher()
    assert m.dbSize() == (0, 0) and m.dbAdd(np.zeros((3, 32), dtype=np.uint8)) == 0 and m.dbSize() == (1, 3)
    m.dbClear()
    assert m.dbSize() == (0, 0)
    with pytest.raises(TypeError, match='uint8'):
        m.dbAdd(np.zeros((3, 32)))
    with pytest.raises(nat.NativeError, match='push a frame'):
        m.dbQuery()
