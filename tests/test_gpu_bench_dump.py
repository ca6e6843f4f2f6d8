"""bench.py --dump-outputs on the device: the line counts exactly the timed steps asked for, and the arrays written are what the
last timed solve returned -- the same timed path (bench.cold_solves) run again in this process on a fresh handle of the same seeded
problem gives them back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, rel_err

pytestmark = pytest.mark.gpu


def test_dumped_outputs_are_those_of_the_last_timed_solve(tmp_path):
    import torch
    import bench
    from pyslam_amd import synthetic
    from pyslam_amd.device import DeviceProblem
    kf, lm, steps = 12, 600, 6
    cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1', '--kf', str(kf),
           '--lm', str(lm), '--no-cpu-baseline', '--dump-outputs', str(tmp_path)]
    run = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line['steps'] == steps and line['cold_solve']['iterations'] == steps and line['ms_per_step'] > 0
    assert sorted(line['dumped_outputs']) == ['cost_history', 'pcg_iterations', 'pcg_relative_residual', 'points', 'poses']
    got = {}
    for name, shape in line['dumped_outputs'].items():
        got[name] = np.load(os.path.join(str(tmp_path), name + '.npy'))
        assert got[name].dtype == np.float64 and list(got[name].shape) == shape

    lp, _ = synthetic.stereo_ba(num_kf=kf, num_lm=lm, obs_per_lm=bench.OBS_PER_LM, half_window=bench.HALF_WINDOW, seed=bench.C3['seed'])
    dev = DeviceProblem(lp, stream=torch.cuda.current_stream().cuda_stream)
    try:
        cold = bench.cold_solves(dev, (lp.poses.copy(), lp.points.copy()), steps, torch.cuda.synchronize, warm_solves=1)
        poses, points = dev.get_params()
    finally:
        dev.close()
    last = cold['last_solve']
    assert cold['iterations'] == steps and len(last['stats']) == got['pcg_iterations'].size
    assert got['poses'].shape == (kf, 12) and got['points'].shape == (lm, 3)
    assert np.array_equal(got['pcg_iterations'], [st[0] for st in last['stats']])
    assert rel_err(got['cost_history'], last['cost_history']) < 1e-12
    assert rel_err(got['poses'], poses) < 1e-12 and rel_err(got['points'], points) < 1e-12
    assert not np.array_equal(got['points'], lp.points)          # (the solve moved them: not the start)


def test_plain_run_is_the_headline_and_full_adds_the_other_legs():
    """A plain run does only what its headline figure needs; --full adds the legs that take runs of their own after the timed region
    (stage breakdown, roofline objects, launch counts, same-point figures, CPU baseline) around the same timed solves."""
    kf, lm, steps = 12, 600, 4
    base = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1', '--kf', str(kf),
            '--lm', str(lm)]
    lines = {}
    for mode, extra in (('plain', []), ('full', ['--full'])):
        run = subprocess.run(base + extra, cwd=REPO, capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, (mode, run.stderr[-3000:])
        lines[mode] = json.loads(run.stdout.strip().splitlines()[-1])
    plain, full = lines['plain'], lines['full']
    for line in (plain, full):
        assert line['steps'] == steps and line['cold_solve']['iterations'] == steps and line['ms_per_step'] > 0
        assert line['value'] == line['ms_per_step'] and line['unit'] == 'ms/LM-iter'
        assert line['higher_is_better'] is False and line['dtype'] == 'f64'
    assert plain['metric'] == full['metric']
    legs = ('stage_ms', 'roofline', 'roofline_schur', 'roofline_cg', 'reduced_solve_stage', 'lagged_inverse', 'steady_same_point_ms',
            'moving_same_point_ms', 'cpu_baseline')
    assert plain['full'] is False and [k for k in legs if k in plain] == []
    assert full['full'] is True and [k for k in legs if k not in full] == []
    assert rel_err(plain['config']['cost_history'], full['config']['cost_history']) < 1e-12
