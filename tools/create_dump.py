#!/usr/bin/env python
"""What ps_problem_create builds, bit for bit, in one JSON file -- and the comparison of two such files.  tests/test_gpu_create.py
holds the device builder against the host builder of ONE build; it cannot see both change together.  This can: dump on the build
before a change to handle set-up and on the build after it, then compare.

    python tools/create_dump.py --out before.json                   (on an MI355X, one process per build)
    python tools/create_dump.py --compare before.json after.json [--json profiles/NAME.json]

Per problem and per builder (PS_CREATE_DEVICE = 0 and = 2; C3 and C4 once, in the default mode): the 16 table checksums
(ps_debug_table_checksums), ps_get_info, and the whole result of one gn_iteration() -- the iteration goes through the tables the
checksums do not reach (pose items, factor lists, zero-slot list, packed landmark runs).  Floats are written as hex: equal means
equal in every bit.  --compare exits 1 when any entry differs."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def tile_cases(synthetic):
    """the three problems of test_device_build_with_landmark_tiles_and_the_untiled_fallback"""
    return [('tiled', synthetic.stereo_ba(num_kf=60, num_lm=30000, obs_per_lm=10, half_window=10, seed=5)[0]),
            ('blocks_fill_chip', synthetic.stereo_ba(num_kf=200, num_lm=9000, obs_per_lm=10, half_window=20, seed=6)[0]),
            ('short_tasks', synthetic.stereo_ba(num_kf=100, num_lm=3000, obs_per_lm=10, half_window=20, seed=8)[0])]


def constant_and_repeated(synthetic):
    """test_device_build_with_constant_poses_constant_points_and_repeated_observations"""
    lp, _ = synthetic.stereo_ba(num_kf=30, num_lm=2000, obs_per_lm=8, half_window=6, seed=7)
    const = np.zeros(lp.pose_rid.size, bool)
    const[[0, 5, 11]] = True
    rid = np.full(const.size, -1)
    rid[~const] = np.arange((~const).sum())
    lp.pose_rid = rid.astype(np.int32)
    cpt = np.zeros(lp.point_vid.size, bool)
    cpt[::7] = True
    vid = np.full(cpt.size, -1)
    vid[~cpt] = np.arange((~cpt).sum())
    lp.point_vid = vid.astype(np.int32)
    dup = np.arange(50)
    for name in ('obs_pose', 'obs_point', 'obs_grp'):
        setattr(lp, name, np.concatenate([getattr(lp, name), getattr(lp, name)[dup]]))
    lp.obs_uvd = np.concatenate([lp.obs_uvd, lp.obs_uvd[dup] + 0.25])
    return lp


def wide_groups(synthetic):
    """one stiffness per observation: more than 255 observation groups"""
    lp, _ = synthetic.stereo_ba(num_kf=8, num_lm=150, obs_per_lm=4, half_window=3, seed=12)
    rng = np.random.default_rng(1)
    n = lp.num_obs
    lp.stiff3 = np.stack([(np.eye(3) * (0.5 + rng.random(3))).ravel() for _ in range(n)])
    lp.obs_groups = np.stack([np.array([0., i, lp.obs_groups[0, 2], lp.obs_groups[0, 3]]) for i in range(n)])
    lp.obs_grp = np.arange(n, dtype=np.int32)
    assert n > 255
    return lp.finalize()


def hybrid_rows(synthetic):
    """stereo BA with pose-pair rows of caller's blocks (ps_problem_create_hybrid): one row on one pose, rows on pose pairs the
    landmarks do not couple; -> (lp, row values)"""
    lp, _ = synthetic.stereo_ba(num_kf=20, num_lm=600, obs_per_lm=5, half_window=3, seed=13)
    lp.h_i = np.array([-1, 0, 2, 5, 1], np.int32)
    lp.h_j = np.array([3, 19, 17, 6, 12], np.int32)
    lp.h_blocks = np.arange(5, dtype=np.int32)
    lp.h_ptr = np.arange(6, dtype=np.int32)
    rows = np.zeros((5, 3 * 36 + 12))
    rows[:, 0:36] = rows[:, 72:108] = (0.01 * np.eye(6)).ravel()
    rows[:, 36:72] = (1e-4 * np.arange(36).reshape(6, 6)).ravel()
    rows[:, 108:] = 1e-4 * np.arange(1, 13)
    return lp, rows


def cases():
    """[(name, lowered problem, create-time environment, builders, keyword arguments of DeviceProblem, host rows or None)]"""
    from pyslam_amd import synthetic
    from pyslam_amd.device import resident_tables
    both, host_only = (0, 2), (0,)
    out = []
    for kf, lm, obs, hw, seed in [(6, 64, 4, 3, 1), (33, 777, 12, 16, 4), (40, 3000, 6, 8, 2)]:
        out.append(('stereo_{}_{}'.format(kf, lm), synthetic.stereo_ba(num_kf=kf, num_lm=lm, obs_per_lm=obs, half_window=hw, seed=seed)[0],
                    {}, both, {}, None))
    for name, lp in tile_cases(synthetic):
        out.append(('tiles_' + name, lp, {'PS_SCHUR_TILE_MIN_MB': 1}, both, {}, None))
        out.append(('tiles_keys64_' + name, lp, {'PS_SCHUR_TILE_MIN_MB': 1, 'PS_CREATE_KEYS64': 1}, both, {}, None))
    out.append(('constant_and_repeated', constant_and_repeated(synthetic), {}, both, {}, None))
    lp33 = out[1][1]
    out.append(('stereo_33_777_by_landmark', lp33, {'PS_PAIRS_BY_LANDMARK': 1}, host_only, {}, None))
    out.append(('stereo_33_777_tile_kb_256', lp33, {'PS_SCHUR_TILE_KB': 256}, host_only, {}, None))
    out.append(('wide_groups', wide_groups(synthetic), {}, both, {}, None))
    out.append(('mono_ba', synthetic.mono_ba(num_kf=30, num_lm=2000, obs_per_lm=6, half_window=6, seed=3)[0], {}, both, {}, None))
    for dof in (3, 6):
        lp, _ = synthetic.pose_graph(num_poses=300, num_loops=500, dof=dof, seed=4)
        lp.u_i = np.array([0, 150], np.int32)                  # a second prior
        lp.u_Tobs_inv = np.concatenate([lp.u_Tobs_inv, lp.poses[150:151]])
        lp.u_grp = np.array([1, 1], np.int32)
        extra = (np.array([0, 7, 299, 12], np.int32), np.array([299, 7, 0, 200], np.int32))
        out.append(('pose_graph_se{}'.format(dof // 3 + 1), lp.finalize(), {}, both, {'extra_pairs': extra}, None))
    lp, rows = hybrid_rows(synthetic)
    out.append(('hybrid_rows', lp, {}, both, {}, rows))
    lp, truth = synthetic.stereo_ba(num_kf=25, num_lm=4000, obs_per_lm=7, half_window=6, seed=9)
    lp = synthetic.with_pose_edges(lp, 5, seed=3, truth_poses=truth['poses'])
    out.append(('pose_edges_resident', resident_tables(lp, params=True, tables=True), {}, both, {}, None))
    out.append(('C3', synthetic.stereo_ba(num_kf=200, num_lm=50000, obs_per_lm=10, half_window=20, seed=0)[0], {}, (None,), {}, None))
    out.append(('C4', synthetic.stereo_ba(num_kf=2000, num_lm=500000, obs_per_lm=10, half_window=20, seed=1)[0], {}, (None,), {}, None))
    return out


def one(lib, lp, env, mode, kw, rows):
    from pyslam_amd.device import DeviceProblem
    env = dict(env)
    if mode is not None:
        env['PS_CREATE_DEVICE'] = mode
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        dev = DeviceProblem(lp, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        sums, n = (ctypes.c_uint64 * 16)(), ctypes.c_int(0)
        assert lib.ps_debug_table_checksums(dev._h, sums, 16, ctypes.byref(n)) == 0 and n.value == 16
        if rows is not None:
            dev.set_host_rows(rows, 0.125)
        res = dev.gn_iteration()
        return {'checksums': ['{:016x}'.format(s) for s in sums], 'info': {k: repr(v) for k, v in sorted(dev.info.items())},
                'iteration': [float(x).hex() if isinstance(x, float) else repr(x) for x in res]}
    finally:
        dev.close()


def flatten(dump):
    return {'{}/{}/{}'.format(c, m, k): v for c, modes in dump['cases'].items() for m, e in modes.items() for k, v in e.items()}


def compare(a_path, b_path, json_path):
    with open(a_path) as fa, open(b_path) as fb:
        a, b = json.load(fa), json.load(fb)
    fa, fb = flatten(a), flatten(b)
    entries = {k: {'equal': k in fa and k in fb and fa[k] == fb[k]} for k in sorted(set(fa) | set(fb))}
    differing = [k for k, e in entries.items() if not e['equal']]
    res = {'build_sha_a': a['build_sha'], 'build_sha_b': b['build_sha'], 'entries': len(entries), 'differing': differing,
           'all_equal': not differing, 'per_entry': entries}
    print(json.dumps({k: res[k] for k in ('build_sha_a', 'build_sha_b', 'entries', 'differing', 'all_equal')}))
    if json_path:
        with open(json_path, 'w') as fh:
            json.dump(res, fh, indent=1)
            fh.write('\n')
    return 0 if not differing else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    ap.add_argument('--json')
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.json))
    if not a.out:
        ap.error('--out or --compare')
    from pyslam_amd import _native as nat
    lib = nat.require_gpu()
    dump = {'build_sha': nat.load().ps_build_sha().decode(), 'cases': {}}
    for name, lp, env, modes, kw, rows in cases():
        dump['cases'][name] = {'default' if m is None else 'create_device_{}'.format(m): one(lib, lp, env, m, kw, rows) for m in modes}
        print(name, 'done', flush=True)
    with open(a.out, 'w') as fh:
        json.dump(dump, fh, indent=1)
        fh.write('\n')
    print('{} problems from build {} -> {}'.format(len(dump['cases']), dump['build_sha'], a.out))


if __name__ == '__main__':
    main()
