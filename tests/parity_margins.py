#!/usr/bin/env python
"""Measured parity margins per golden (GPU): what tests/test_gpu_parity.py asserts, as numbers.
Writes gpurun_out/parity_margins.json; the maxima are committed as tests/golden/parity_margins.json and the tests
assert the SURVEY 8d tolerances (or, where a golden cannot meet one for a stated reason, 10x the measured value)."""
import json, os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
from conftest import load_golden, golden_lp, golden_options, SOLVE_CASES, rel_err   # noqa: E402
from test_gpu_parity import oracle_reduced                                           # noqa: E402
import pyslam_amd.synthetic as synthetic                                             # noqa: E402
from test_host_api import build_namespace                                            # noqa: E402
from pyslam_amd.device import DeviceProblem                                          # noqa: E402
from pyslam_amd.lowering import pack_pose                                            # noqa: E402

out = {}
for name in SOLVE_CASES:
    g = load_golden(name)
    lp = golden_lp(g)
    dev = DeviceProblem(lp)
    dev.linearize(0.)
    S, gg = dev.reduced_dense()
    So, go, _ = oracle_reduced(lp)
    rec = {'S': rel_err(S, So), 'g': rel_err(gg, go)}
    ns = build_namespace()
    opt = ns.Options()
    for k, v in golden_options(g).items():
        setattr(opt, k, v)
    problem = synthetic.to_objects(lp, ns, opt, points_first=bool(g.get('points_first', True)))
    final = problem.solve()
    ref = g['cost_history']
    hist = np.array(problem._cost_history)
    rec['len_ok'] = len(hist) == len(ref)
    if rec['len_ok']:
        big = ref > 1e-9 * ref[0]
        rec['cost_rel'] = float(np.max(np.abs(hist[big] - ref[big]) / np.abs(ref[big])))
        rec['cost_rel_each'] = [float(abs(a - b) / abs(b)) if b != 0 else float(abs(a)) for a, b in zip(hist, ref)]
        rec['cost_ref'] = [float(x) for x in ref]
    if 'final_poses' in g:
        got = np.stack([pack_pose(final[k]) for k in problem._device.lp.pose_keys])
        rec['poses_abs'] = float(np.abs(got - g['final_poses']).max())
    if 'final_points' in g:
        got = np.stack([final[k] for k in problem._device.lp.point_keys])
        rec['points_abs'] = float(np.abs(got - g['final_points']).max())
    out[name] = rec
    print(name, json.dumps({k: v for k, v in rec.items() if k not in ('cost_rel_each', 'cost_ref')}), flush=True)
os.makedirs(os.path.join(REPO, 'gpurun_out'), exist_ok=True)
with open(os.path.join(REPO, 'gpurun_out', 'parity_margins.json'), 'w') as f:
    json.dump(out, f, indent=1)

# the off-box scenes (tests/test_gpu_offbox.py): per scene and quantity the device's distance from the long-double reference, e64 and
# the bound that follows from e64
import offbox_scenes                                                                 # noqa: E402
import test_gpu_offbox                                                               # noqa: E402
for name in offbox_scenes.SCENES:
    test_gpu_offbox.margins(name)

# the pose-factor scenes (tests/test_gpu_posegraph.py): per scene, group and quantity the device's distance from the long-double
# reference, e64 and the bound
import posegraph_scenes                                                              # noqa: E402
import test_gpu_posegraph                                                            # noqa: E402
for case in posegraph_scenes.cases():
    test_gpu_posegraph.margins(case)

# multi-view triangulation (tests/test_gpu_triang.py): per scene and stage the device's distance from the long-double restatement, e64,
# the bound, the share of landmarks each condition leaves out and the status counts
import triang_scenes                                                                 # noqa: E402
import test_gpu_triang                                                               # noqa: E402
for name in triang_scenes.SCENES:
    test_gpu_triang.margins(name)
test_gpu_triang.status('far100')
for dev in test_gpu_triang._HANDLES.values():
    dev.close()

# the Sim(3) pose-graph scenes (tests/test_gpu_sim3graph_rows.py): per scene and quantity the device's distance from the long-double
# definition, e64 and the bound
import sim3graph_row_scenes                                                          # noqa: E402
import test_gpu_sim3graph_rows                                                       # noqa: E402
for name in sim3graph_row_scenes.ROW_SCENES:
    test_gpu_sim3graph_rows.margins(name)
