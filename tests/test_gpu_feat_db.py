"""The keyframe database query on the device (csrc/ps_k_feat_db.h: k_feat_db_search; Matcher.dbAdd / dbQuery, ps_feat_db_*) against
its restatement (featproc.db_query) and against the device's own matching without a prior, and the handle's behaviour around it:
growth, clearing, memory accounting, errors.  Run with `-m gpu` on an MI355X.  Scores are integers: every comparison is exact.

What the comparisons rely on -- restatement = brute force = step 9's count, ties and c1 = c2 among the cases -- is asserted on the
host (tests/test_loop_host.py over tests/loop_scenes.py)."""
import ctypes as C

import numpy as np
import pytest

import loop_scenes as ls
from pyslam_amd import _native as nat

pytestmark = pytest.mark.gpu


def matcher(F, **kw):
    from pyslam_amd.pipelines.matcher import Matcher, Matcher_parameters
    return Matcher(Matcher_parameters(max_features=max(F, 1), **dict(ls.KERNEL_KW, **kw)))


def filled(F, entries=None):
    m = matcher(F)
    m.pushBack(ls.kernel_image(F))
    for k, d in enumerate(ls.kernel_entries() if entries is None else entries):
        assert m.dbAdd(d) == k
    return m


@pytest.mark.parametrize('F', ls.FRAME_SIZES)
def test_the_query_equals_the_restatement_and_the_devices_own_global_match(F):
    ents = ls.kernel_entries()
    K = len(ents)
    m = filled(F)
    try:
        assert m.dbSize() == (K, sum(ls.ENTRY_SIZES))
        for cost_max in ls.COST_MAX:
            m.params.match_cost_max = cost_max
            for ratio in ls.RATIOS:
                ref = ls.kernel_reference(F, ratio, cost_max)
                full = m.dbQuery(ratio)
                print('F = {}, ratio {}, match_cost_max {}: device {} restatement {}'.format(F, ratio, cost_max, full.tolist(), ref.tolist()))
                assert full.dtype == np.int32 and np.array_equal(full, ref)
                assert m.dbQuery(ratio).tobytes() == full.tobytes()                # two identical queries
                for first, last in ls.RANGES:
                    out = m.dbQuery(ratio, first, last)
                    assert out.shape == (last - first,) and np.array_equal(out, ref[first:last]), (first, last)
                own = []
                for d in ents:                                                     # the only route there was: one map per entry
                    m.setMap(np.zeros((d.shape[0], 3)), d)
                    status = m.matchMapGlobal(ratio)[1]
                    own.append(int(((status == 0) | (status == 3)).sum()))
                assert own == full.tolist(), (own, full)
        assert len(m.features(2)[0]) == F
    finally:
        m.close()


def test_growth_past_the_first_allocation_and_clearing():
    F = 129
    ents = ls.kernel_entries()
    m = filled(F, [])
    try:
        assert m.dbSize() == (0, 0)
        bytes0 = m.device_bytes                                # a handle that never added an entry: what it was created with
        fresh = matcher(F)
        fresh.pushBack(ls.kernel_image(F))
        fresh.dbQuery()                                        # the feature pass; a query of nothing
        assert fresh.device_bytes == bytes0
        fresh.close()
        sizes, grown, added = [bytes0], 0, []
        while grown < 3 or len(added) <= 70:                   # the first allocation, then the descriptor pool doubled twice; and
                                                               # past the first 64 entries and 64 workgroups of the tables
            d = ents[2 + len(added) % 6]
            m.dbAdd(d)
            added.append(d)
            if m.device_bytes - sizes[-1] >= 32 * 1024:        # tables of ints grow by less; the pool by 32 KiB and more
                grown += 1
            sizes.append(m.device_bytes)
            assert len(added) < 400
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
        print('{} entries, {} descriptors, device bytes {} -> {}'.format(len(added), m.dbSize()[1], bytes0, sizes[-1]))
        scores = m.dbQuery()
        other = filled(F, added)
        try:
            assert np.array_equal(other.dbQuery(), scores)
        finally:
            other.close()
        ref = ls.kernel_reference(F, (4, 5), 1200)
        assert np.array_equal(scores, [ref[2 + k % 6] for k in range(len(added))])
        top = m.device_bytes
        m.dbClear()
        assert m.dbSize() == (0, 0) and m.device_bytes == top  # the buffers are kept
        assert m.dbQuery().shape == (0,)
        for d in ents:
            m.dbAdd(d)
        assert np.array_equal(m.dbQuery(), ref) and m.device_bytes == top
    finally:
        m.close()


def test_errors_through_the_c_abi():
    from pyslam_amd.pipelines.matcher import Matcher_parameters
    lib = nat.require_gpu()
    p = Matcher_parameters(max_features=256, **ls.KERNEL_KW)._native()
    e, k, n = C.c_int32(), C.c_int32(), C.c_int64()
    scores = np.zeros(8, dtype=np.int32)
    d = np.ascontiguousarray(ls.kernel_entries()[3])
    dp = d.ctypes.data_as(nat.c_u8p)
    h = nat.H()
    nat.check(lib.ps_feat_create(192, 256, 256, None, C.byref(h)))

    def fails(rc, text):
        assert rc == -1 and text in lib.ps_last_error(), (rc, lib.ps_last_error())
    try:
        fails(lib.ps_feat_db_add(None, 1, dp, C.byref(e)), b'null argument')
        fails(lib.ps_feat_db_add(h, 1, dp, None), b'null argument')
        fails(lib.ps_feat_db_add(h, 1, None, C.byref(e)), b'null argument')
        fails(lib.ps_feat_db_add(h, -1, dp, C.byref(e)), b'num must not be negative')
        fails(lib.ps_feat_db_clear(None), b'null')
        fails(lib.ps_feat_db_size(h, None, C.byref(n)), b'null argument')
        fails(lib.ps_feat_db_size(h, C.byref(k), None), b'null argument')
        fails(lib.ps_feat_db_query(h, 0, 0, 4, 5, None, nat.i32p(scores)), b'null argument')
        fails(lib.ps_feat_db_query(h, 0, 0, 4, 5, C.byref(p), None), b'null argument')
        nat.check(lib.ps_feat_db_add(h, 64, dp, C.byref(e)))
        nat.check(lib.ps_feat_db_add(h, 0, None, C.byref(e)))                      # an empty entry needs no array
        assert e.value == 1
        fails(lib.ps_feat_db_query(h, 0, 2, 4, 5, C.byref(p), nat.i32p(scores)), b'push a frame')
        im = ls.kernel_image(1)
        nat.check(lib.ps_feat_push(h, 192, 256, im.ctypes.data_as(nat.c_u8p), None))
        for first, last in ((-1, 1), (2, 1), (0, 3), (3, 3)):
            fails(lib.ps_feat_db_query(h, first, last, 4, 5, C.byref(p), nat.i32p(scores)), b'entry range')
        for num, den in ((0, 5), (6, 5), (4, 32769)):
            fails(lib.ps_feat_db_query(h, 0, 2, num, den, C.byref(p), nat.i32p(scores)), b'ratio')
        bad = Matcher_parameters(max_features=256, nms_n=4)._native()
        fails(lib.ps_feat_db_query(h, 0, 2, 4, 5, C.byref(bad), nat.i32p(scores)), b'nms_n')
        bad = Matcher_parameters(max_features=257)._native()
        fails(lib.ps_feat_db_query(h, 0, 2, 4, 5, C.byref(bad), nat.i32p(scores)), b'max_features')
        nat.check(lib.ps_feat_db_query(h, 0, 2, 4, 5, C.byref(p), nat.i32p(scores)))
        nat.check(lib.ps_feat_db_query(h, 2, 2, 4, 5, C.byref(p), nat.i32p(scores)))
        assert scores[1] == 0 and 0 < scores[0] <= 64
    finally:
        lib.ps_feat_destroy(h)


def test_the_two_limits():
    lib = nat.require_gpu()
    e, k, n = C.c_int32(), C.c_int32(), C.c_int64()
    h = nat.H()
    nat.check(lib.ps_feat_create(16, 16, 16, None, C.byref(h)))
    try:
        big = np.zeros((1 << 20, 32), dtype=np.uint8)
        for _ in range(4):
            nat.check(lib.ps_feat_db_add(h, 1 << 20, big.ctypes.data_as(nat.c_u8p), C.byref(e)))
        assert lib.ps_feat_db_add(h, 1, big.ctypes.data_as(nat.c_u8p), C.byref(e)) == -1 and b'2^22 descriptors' in lib.ps_last_error()
        nat.check(lib.ps_feat_db_size(h, C.byref(k), C.byref(n)))
        assert (k.value, n.value) == (4, 1 << 22)
        nat.check(lib.ps_feat_db_clear(h))
        for _ in range(65536):
            assert lib.ps_feat_db_add(h, 0, None, C.byref(e)) == 0
        assert e.value == 65535
        assert lib.ps_feat_db_add(h, 0, None, C.byref(e)) == -1 and b'65536 entries' in lib.ps_last_error()
        nat.check(lib.ps_feat_db_size(h, C.byref(k), C.byref(n)))
        assert (k.value, n.value) == (65536, 0)
    finally:
        lib.ps_feat_destroy(h)
