#!/usr/bin/env python
"""ms per keyframe database query (ps_feat_db_query: one memset, k_feat_db_search, one copy, one wait) at
K = 16, 128 and 1 024 entries of 1 000 descriptors against a frame of 1 000 features, against the only way the library had before to
get the same scores: per entry one Matcher.setMap + matchMapGlobal (an upload, a memset, two launches, a download and a wait each),
the score counted from the statuses 0 and 3.  That loop is the baseline, not the code under test; both give the same integers, which
is asserted.  The frame is a 400 x 400 noise image (nms_n = 1, response_threshold = 0, max_features = 1 000), entry e holds the
frame's own descriptors with +-12 grey levels of noise per byte (every one passes the ratio test; the work does not depend on the
outcome); match_cost_max = 4 000.  A call is timed on the host clock from its start to its return -- it ends with the stream
synchronised and the scores on the host -- features held, median of --repeat calls after two warm-up calls.

The kernel's share of a query comes from a profiler run of its own (the profiler stretches the host side, so only its kernel times
are used):

    python tools/loop_bench.py [--repeat 9] [--out profiles/loop_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o loop -- python tools/loop_bench.py --one 128
    python tools/loop_bench.py --kernel-stats DIR/.../loop_kernel_stats.csv --out profiles/loop_bench.json
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

SIZES = (16, 128, 1024)
N_DESC = F = 1000
QUERY_CALLS = dict(memsets=1, kernel_launches=1, copies=1, synchronisations=1)
BASELINE_CALLS_PER_ENTRY = dict(uploads=2, memsets=1, kernel_launches=2, copies=1, synchronisations=2)


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def median_ms(fn, repeat):
    for _ in range(2):
        fn()
    return float(np.median([ms(fn) for _ in range(repeat)]))


def make(K):
    """(matcher with the frame pushed, its features computed and K entries added; the entries)."""
    from pyslam_amd.pipelines.matcher import Matcher, Matcher_parameters
    image = np.random.default_rng(7).integers(0, 256, size=(400, 400)).astype(np.uint8)
    m = Matcher(Matcher_parameters(nms_n=1, response_threshold=0, max_features=F, match_cost_max=4000))
    m.pushBack(image)
    m.dbQuery()                                                # the frame's feature pass
    desc = m.features(2)[2]
    assert desc.shape[0] == F, desc.shape
    rng = np.random.default_rng(K)
    entries = [np.clip(desc[np.arange(N_DESC) % F].astype(np.int64) + rng.integers(-12, 13, size=(N_DESC, 32)), 0, 255).astype(np.uint8)
               for _ in range(K)]
    for d in entries:
        m.dbAdd(d)
    return m, entries


def query_fn(m, K):
    """The C call itself, as Matcher.dbQuery makes it."""
    from pyslam_amd import _native as nat
    scores = np.zeros(K, dtype=np.int32)
    p = m.params._native()
    sp, pp = nat.i32p(scores), C.byref(p)

    def call():
        nat.check(m._lib.ps_feat_db_query(m._h, 0, K, 4, 5, pp, sp))
    return call, scores


def baseline(m, entries):
    zeros = np.zeros((N_DESC, 3))
    out = np.zeros(len(entries), dtype=np.int32)
    for e, d in enumerate(entries):
        m.setMap(zeros, d)
        status = m.matchMapGlobal((4, 5))[1]
        out[e] = int(((status == 0) | (status == 3)).sum())
    return out


def run(K, repeat):
    m, entries = make(K)
    call, scores = query_fn(m, K)
    out = dict(kind='db_query', entries=K, descriptors_per_entry=N_DESC, features=F, pairs=K * N_DESC * F, repeat=repeat,
               calls=QUERY_CALLS, baseline_calls_per_entry=BASELINE_CALLS_PER_ENTRY)
    out['query_ms'] = median_ms(call, repeat)
    out['query_python_ms'] = median_ms(m.dbQuery, repeat)
    ref = baseline(m, entries)
    call()
    assert np.array_equal(scores, ref), (scores, ref)
    out['baseline_ms'] = median_ms(lambda: baseline(m, entries), max(3, repeat // 3) if K > 128 else repeat)
    out['baseline_over_query'] = out['baseline_ms'] / out['query_ms']
    out['score_min_max'] = [int(scores.min()), int(scores.max())]
    out['device_bytes'] = int(m.device_bytes)
    m.close()
    return out


def one(K, calls=20):
    m, _ = make(K)
    call, _ = query_fn(m, K)
    for _ in range(calls):
        call()
    m.close()


def kernel_stats(path):
    out = []
    for r in csv.DictReader(open(path)):
        calls = int(r.get('Calls', 0))
        total = float(r.get('TotalDurationNs', 0))
        out.append({'kernel': r.get('Name', r.get('KernelName', '')).split('(')[0], 'calls': calls, 'total_ms': total * 1e-6,
                    'average_us': total / max(calls, 1) * 1e-3, 'percent': float(r.get('Percentage', 0))})
    out.sort(key=lambda d: -d['total_ms'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=9)
    ap.add_argument('--out')
    ap.add_argument('--one', type=int, default=None, help='20 queries at this many entries and nothing else (for a profiler)')
    ap.add_argument('--kernel-stats', default=None, help='rocprofv3 kernel_stats.csv of a --one run: merged into --out')
    ap.add_argument('--stats-entries', type=int, default=128)
    a = ap.parse_args()
    if a.one:
        one(a.one)
        return
    if a.kernel_stats:
        res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        stats = kernel_stats(a.kernel_stats)
        res['kernel_stats'] = dict(entries=a.stats_entries, kernels=stats)
        k = next((s for s in stats if 'k_feat_db_search' in s['kernel']), None)
        q = next((s for s in res.get('shapes', []) if s['entries'] == a.stats_entries), None)
        if k and q:
            res['kernel_stats']['k_feat_db_search_us'] = k['average_us']
            res['kernel_stats']['share_of_query'] = k['average_us'] * 1e-3 / q['query_ms']
        print(json.dumps(res['kernel_stats']))
    else:
        if a.repeat < 7:
            ap.error('--repeat must be at least 7')
        from __graft_entry__ import source_sha
        res = {'tool': 'tools/loop_bench.py', 'source_sha16': source_sha(), 'shapes': []}
        for K in SIZES:
            res['shapes'].append(run(K, a.repeat))
            print(json.dumps(res['shapes'][-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
