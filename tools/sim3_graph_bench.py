#!/usr/bin/env python
"""ms per Sim(3) pose-graph solve on the device (ps_sim3pg_solve: the whole loop in one call) and per iteration
(ps_sim3pg_iteration), the iteration split by events into its stages -- edges, assemble, factor, substitute + refine,
retract + cost --, on the ring graphs of synthetic.sim3_graph with 64, 256 and 1 024 vertices and a chord from every 5th vertex
(perturbation 0.1; n = 7 (N - 1) unknowns, dense).  A call is timed on the host clock from its start to its return (it ends with
the stream synchronised and the scalars on the host); median of --repeat calls after two warm-up calls, the vertices set back to
the start in front of every call (outside the clock).  The stage times are the events' of the same calls (ps_sim3pg_profile).

Beside it, for orientation only: the numpy restatement's solve of the same graph (pipelines/simgraph.py, one run), and
Problem.solve()'s loop on an SE(3) pose graph of the same size (synthetic.pose_graph: a chain of N poses with N // 5 loop edges,
solve_tables) -- another group, another solver (Schur-free reduced system, preconditioned CG), not a baseline of this code.

    python tools/sim3_graph_bench.py [--repeat 9] [--sizes 64 256 1024] [--out profiles/sim3_graph_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import numpy as np  # noqa: E402

STAGES = ('edges', 'assemble', 'factor', 'substitute_refine', 'retract_cost')


def ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def shape(N, repeat, with_restatement):
    import sim3graph_scenes as gs
    from pyslam_amd import synthetic
    from pyslam_amd.pipelines import posegraph as pg
    from pyslam_amd.pipelines import simgraph as sg
    from pyslam_amd.problem import Options, solve_tables
    truth, start, held, edges = synthetic.sim3_graph(N, N // 5, 0, 0.1)
    tabs = gs.tables(start, held, edges)
    opt = gs.solve_options()
    dev = pg.DeviceSim3Graph(*tabs)
    rec = dict(kind='sim3_ring', vertices=N, edges=len(edges), unknowns=dev.n, repeat=repeat)
    try:
        solves, its = [], None
        for k in range(repeat + 2):
            dev.set_vertices(tabs[0])
            t, (hist, its, _) = ms(lambda: dev.solve(opt))
            if k >= 2:
                solves.append(t)
        rec.update(solve_ms=float(np.median(solves)), solve_iterations=its, solve_final_cost=float(hist[-1]),
                   truth_gap=gs.vertex_gap(gs.unpack(dev.get_vertices()), truth))
        dev.profile(True)
        calls, stages = [], []
        for k in range(repeat + 2):
            dev.set_vertices(tabs[0])
            t, _ = ms(lambda: dev.iteration(0.))
            if k >= 2:
                calls.append(t)
                stages.append([dev.profile(True)[s] for s in STAGES])
        med = np.median(np.array(stages), axis=0)
        rec.update(iteration_ms=float(np.median(calls)), stage_ms=dict(zip(STAGES, med.tolist())), stage_sum_ms=float(med.sum()))
    finally:
        dev.close()
    if with_restatement:
        t, (V, hist_ref, its_ref) = ms(lambda: sg.solve(start, edges, held, None, opt))
        rec.update(restatement_solve_ms=t, restatement_iterations=its_ref)
    lp, _ = synthetic.pose_graph(num_poses=N, num_loops=N // 5, dof=6, seed=2)
    se3 = []
    for k in range(repeat + 2):
        t, out = ms(lambda: solve_tables(lp, Options()))
        if k >= 2:
            se3.append(t)
    rec.update(se3_problem_solve_ms=float(np.median(se3)), se3_iterations=len(out[0]) - 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=9)
    ap.add_argument('--sizes', type=int, nargs='+', default=[64, 256, 1024])
    ap.add_argument('--no-restatement-above', type=int, default=1024)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from pyslam_amd import _native as nat
    lib = nat.require_gpu()
    out = dict(tool='tools/sim3_graph_bench.py', source_sha16=lib.ps_build_sha().decode(), shapes=[])
    for N in a.sizes:
        rec = shape(N, a.repeat, N <= a.no_restatement_above)
        out['shapes'].append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
