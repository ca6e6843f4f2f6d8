#!/usr/bin/env python
"""Every output of the stand-alone handles and stateless calls that share the host plumbing of csrc/ps_host_devmem.h and the dense
direct solve of csrc/ps_host_bchol.h, bit for bit, in one .npz -- and the comparison of two such files.  The GPU tests compare
with tolerances; they cannot see a change of the last bit, nor a byte count that drifts on both sides of an assertion.  This can:
dump on the build before a change and on the build after it, then compare.  Only Python API that both builds have is used, so
the same file runs in a checkout of either.

    python tools/standalone_dump.py --out before.npz                (on an MI355X, one run per build)
    python tools/standalone_dump.py --compare before.npz after.npz [--json profiles/NAME.json]

Sections, each in a child process of its own under its own time limit (a section that fails or runs out of time ends the dump):
  sparse_direct  ps_sparse_normal_direct, n in 1 23 24 25 67 193 500, from r and from rhs, 0 and 3 refinement steps: dx, relres
  sparse_cg      ps_sparse_normal_solve, n in 1 256 257 1025, both forms: dx, iterations, relres
  dense_normal   ps_dense_normal_solve, n in 1 5 257, with and without the covariance
  sim3           the Sim(3) pose graph on tests/sim3graph_scenes.py graphs with 1, 4 (the held vertex in the middle) and 12 free
                 vertices, L2 and Huber: linearize, one iteration at lambda 0 and 1e-3, solve
  photo          the photometric handle on tests/golden/photometric.npz: normal equations, one iteration
  dense_track    DenseTracker on a 96 x 128 pair, two levels, max_iters 2, 6, 6, 3: the track outputs and device_bytes after each
  feat           the feature matcher: a temporal match, a map match, a global match, two database entries and a query, with
                 device_bytes after each
  cov            covariance_marginals on the ba_small golden
  factor         ps_debug_dense_factor at n = 67: L, Tinv, Li, LiT, Ainv
The scenes come from the tests' own helpers (tests/sim3graph_scenes.py, mono_scenes.py, conftest.py, test_photometric.py and the
underscore helpers of test_gpu_dense_kernels.py) and the sparse systems need scipy: a rename there has to be followed here.
`build_sha` is ps_build_sha() of the library that ran.  --compare exits 1 when any array differs (np.array_equal with
equal_nan=True: a NaN equals a NaN in the same place)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def sparse_system(n, seed):
    """J = [2 I; 0.3 R] with R sparse random (2 n + 1 rows, about 4 entries each), r and rhs: well conditioned, full rank."""
    import scipy.sparse as sp
    rng = np.random.default_rng([seed, n])
    m2 = 2 * n + 1
    rows = np.repeat(np.arange(m2), 4)
    R = sp.csr_matrix((0.3 * rng.standard_normal(rows.size), (rows, rng.integers(0, n, rows.size))), shape=(m2, n))
    J = sp.vstack([2. * sp.identity(n), R]).tocsr()
    return J, rng.standard_normal(J.shape[0]), rng.standard_normal(n)


def dump_sparse_direct(out):
    from pyslam_amd.device import sparse_normal_direct
    for n in (1, 23, 24, 25, 67, 193, 500):
        J, r, rhs = sparse_system(n, 1)
        for form, kw in (('r', dict(r=r)), ('rhs', dict(rhs=rhs))):
            for steps in (0, 3):
                dx, _, rel = sparse_normal_direct(J, refine_steps=steps, accept=1., **kw)
                out['sparse_direct/n{}_{}_refine{}/dx'.format(n, form, steps)] = dx
                out['sparse_direct/n{}_{}_refine{}/relres'.format(n, form, steps)] = np.array(rel)


def dump_sparse_cg(out):
    from pyslam_amd.device import sparse_normal_solve
    for n in (1, 256, 257, 1025):
        J, r, rhs = sparse_system(n, 2)
        for form, kw in (('r', dict(r=r)), ('rhs', dict(rhs=rhs))):
            dx, its, rel = sparse_normal_solve(J, accept=1., **kw)
            pre = 'sparse_cg/n{}_{}/'.format(n, form)
            out[pre + 'dx'], out[pre + 'iterations'], out[pre + 'relres'] = dx, np.array(its), np.array(rel)


def dump_dense_normal(out):
    from pyslam_amd.device import dense_normal_solve
    for n in (1, 5, 257):
        rng = np.random.default_rng([3, n])
        J, r = rng.standard_normal((2 * n + 3, n)), rng.standard_normal(2 * n + 3)
        out['dense_normal/n{}/dx'.format(n)] = dense_normal_solve(J, r)
        out['dense_normal/n{}/cov_dx'.format(n)], out['dense_normal/n{}/cov'.format(n)] = dense_normal_solve(J, r, True)


def dump_sim3(out):
    import sim3graph_scenes as gs
    from pyslam_amd.losses import HuberLoss
    from pyslam_amd.pipelines import posegraph as pg
    ring5 = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)]
    graphs = {'free1': gs.random_graph(2, [(0, 1)], (0,), 31), 'free4_held_middle': gs.random_graph(5, ring5, (2,), 32),
              'free12': gs.random_graph(13, gs.chain_pairs(16, 13), (0,), 33)}
    for gname, (V, held, edges) in graphs.items():
        tabs = gs.tables(V, held, edges)
        for lname, loss in (('l2', None), ('huber', HuberLoss(0.05))):
            pre = 'sim3/{}_{}/'.format(gname, lname)
            dev = pg.DeviceSim3Graph(*tabs, loss=loss)
            try:
                H, g, c = dev.linearize(0.)
                out[pre + 'linearize/H'], out[pre + 'linearize/g'], out[pre + 'linearize/cost'] = H, g, np.array(c)
                for lam in (0., 1e-3):
                    dev.set_vertices(tabs[0])
                    out[pre + 'iteration_lam{:g}/cost_dx_relres'.format(lam)] = np.array(dev.iteration(lam))
                    out[pre + 'iteration_lam{:g}/vertices'.format(lam)] = dev.get_vertices()
                dev.set_vertices(tabs[0])
                hist, its, dxn = dev.solve(gs.solve_options())
                out[pre + 'solve/history'], out[pre + 'solve/iterations_dx'] = hist, np.array([its, dxn])
                out[pre + 'solve/vertices'] = dev.get_vertices()
            finally:
                dev.close()


def dump_photo(out):
    from pyslam_amd.device import PhotometricDevice
    from pyslam_amd.losses import HuberLoss
    from test_photometric import GOLD, TAGS, block_of
    g = np.load(GOLD)
    for tag in TAGS:
        dev = PhotometricDevice(block_of(g, tag), HuberLoss(10.0), False)
        try:
            T = g[tag + '_T0']
            dev.set_pose(T[:3, :3], T[:3, 3])
            H, b, cost, nvalid = dev.normal_equations()
            pre = 'photo/{}/'.format(tag)
            out[pre + 'H'], out[pre + 'b'], out[pre + 'cost_nvalid'] = H, b, np.array([cost, nvalid])
            dx, cost = dev.step(linesearch=False)
            out[pre + 'iteration/dx6'], out[pre + 'iteration/cost'] = dx, np.array(cost)
            out[pre + 'iteration/pose'] = np.concatenate([a.ravel() for a in dev.get_pose()])
        finally:
            dev.close()


def dump_dense_track(out):
    import test_gpu_dense_kernels as dk
    from pyslam_amd import synthetic
    seq = synthetic.rgbd_sequence(96, 128, 2, seed=8)
    t = dk._tracker(2, 96, 128)
    try:
        t.upload(0, seq['images'][0], seq['depth'][0])
        t.upload(1, seq['images'][1])
        t.make_tables(0, [1, 0], dk._cams(seq['cam'], [1, 0]), dk.VAR, dk.VAR, 0.1)
        out['dense_track/device_bytes_created'] = np.array(t.device_bytes())
        for k, m in enumerate((2, 6, 6, 3)):
            pose, its, hist = t.track(0, 1, [1, 0], [0, 0], dk._options(max_iters=m), dk._loss(3, 10.), dk._pose12(np.eye(3), np.zeros(3)))
            pre = 'dense_track/call{}_max_iters{}/'.format(k, m)
            out[pre + 'pose'], out[pre + 'iterations'], out[pre + 'history'] = pose, np.array(its), np.concatenate(hist)
            out[pre + 'device_bytes'] = np.array(t.device_bytes())
    finally:
        t.close()


def dump_feat(out):
    import mono_scenes as ms
    from pyslam_amd.pipelines.matcher import Matcher, Matcher_parameters
    seq = ms.sequence(96, 128)
    pts, desc = ms.true_map(96, 128)
    m = Matcher(Matcher_parameters(max_features=300))
    try:
        m.pushBack(seq['images'][0])
        m.pushBack(seq['images'][1])
        m.matchFeatures(0)
        out['feat/temporal/matches'], out['feat/temporal/indices'] = m.matches_array()
        out['feat/temporal/device_bytes'] = np.array(m.device_bytes)
        m.setMap(pts, desc)
        for k, a in enumerate(m.matchMap(seq['T_c_w'][1], seq['cam'], 8)):
            out['feat/map/{}'.format(('feature', 'status', 'cost', 'uv')[k])] = a
        out['feat/map/device_bytes'] = np.array(m.device_bytes)
        for k, a in enumerate(m.matchMapGlobal((4, 5))):
            out['feat/global/{}'.format(('feature', 'status', 'cost', 'second', 'uv')[k])] = a
        out['feat/global/device_bytes'] = np.array(m.device_bytes)
        m.dbAdd(desc[:40])
        m.dbAdd(desc)
        out['feat/db/scores'] = m.dbQuery((4, 5))
        out['feat/db/device_bytes'] = np.array(m.device_bytes)
    finally:
        m.close()


def dump_cov(out):
    from conftest import golden_lp, load_golden
    from pyslam_amd.device import DeviceProblem
    dev = DeviceProblem(golden_lp(load_golden('ba_small')))
    try:
        dev.covariance_begin()
        out['cov/ba_small/pose'], out['cov/ba_small/point'] = dev.covariance_marginals()
    finally:
        dev.close()


def dump_factor(out):
    from pyslam_amd.device import dense_factor
    B = np.random.default_rng(67).standard_normal((67, 67))
    f = dense_factor(B @ B.T + 67. * np.eye(67))
    for k in ('L', 'Tinv', 'Li', 'LiT', 'ainv'):
        out['factor/n67/' + k] = f[k]
    out['factor/n67/diag_fail'] = np.array(f['diag_fail'])


# section -> (function, seconds)
SECTIONS = {'sparse_direct': (dump_sparse_direct, 120), 'sparse_cg': (dump_sparse_cg, 120), 'dense_normal': (dump_dense_normal, 60),
            'sim3': (dump_sim3, 120), 'photo': (dump_photo, 60), 'dense_track': (dump_dense_track, 60), 'feat': (dump_feat, 120),
            'cov': (dump_cov, 60), 'factor': (dump_factor, 60)}


def compare(a_path, b_path, json_path):
    a, b = np.load(a_path), np.load(b_path)
    keys = sorted((set(a.files) | set(b.files)) - {'build_sha'})
    arrays = {}
    for k in keys:
        if k not in a.files or k not in b.files:
            arrays[k] = {'shape': None, 'equal': False}
            continue
        same = a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and bool(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f'))
        arrays[k] = {'shape': list(a[k].shape), 'equal': same}
    differing = [k for k in keys if not arrays[k]['equal']]
    res = {'build_sha_a': str(a['build_sha']), 'build_sha_b': str(b['build_sha']), 'arrays': len(keys), 'differing': differing,
           'all_equal': not differing, 'per_array': arrays}
    print(json.dumps({k: res[k] for k in ('build_sha_a', 'build_sha_b', 'arrays', 'differing', 'all_equal')}))
    if json_path:
        with open(json_path, 'w') as fh:
            json.dump(res, fh, indent=1)
            fh.write('\n')
    return 0 if not differing else 1


def run_section(name, path):
    from pyslam_amd import _native as nat
    nat.require_gpu()
    out = {'build_sha': np.array(nat.load().ps_build_sha().decode())}
    with np.errstate(all='ignore'):
        SECTIONS[name][0](out)
    np.savez(path, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    ap.add_argument('--json')
    ap.add_argument('--section', choices=sorted(SECTIONS), help='(what the children of a dump run: this section alone into --out)')
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.json))
    if not a.out:
        ap.error('--out or --compare')
    if a.section:
        run_section(a.section, a.out)
        return
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (_, seconds) in SECTIONS.items():
            part = os.path.join(tmp, name + '.npz')
            # a section that faults, aborts or runs out of time ends the dump: nothing more is started on the device
            subprocess.run([sys.executable, os.path.abspath(__file__), '--section', name, '--out', part], check=True, timeout=seconds)
            with np.load(part) as z:
                if out.setdefault('build_sha', z['build_sha']) != z['build_sha']:
                    sys.exit('the library changed between two sections')
                out.update({k: z[k] for k in z.files})
            print('{}: done'.format(name), flush=True)
    np.savez(a.out, **out)
    print('{} arrays from build {} -> {}'.format(len(out) - 1, out['build_sha'], a.out))


if __name__ == '__main__':
    main()
