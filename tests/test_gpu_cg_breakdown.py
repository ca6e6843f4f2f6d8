"""GPU: the host's answers to a CG breakdown (status word ST_PCG_DONE == 2 behind a whole-iteration call), driven by the test hook
"cg_force_breakdown" (include/pyslam_hip.h): CG iteration n - 1 of the first pass of the next reduced solve reads a negative delta,
finds denom <= 0 through the kernel's own branch and flags the breakdown.  Every tail kernel is gated on ST_PCG_DONE == 1, so the
broken pass must have applied NOTHING, and the repeat must start from a clean set-up:

  A  gn_solve_and_finish_async, folded CG: cg_fused_run(rhs_only) and an ungated tail          (ps_host_iteration.h)
  B  gn_solve_and_finish_async, explicit two-level PCG in its one- / two-launch form: xf_skip, xcg_setup(false), three launches
  C  xcg_run, the synchronous driver behind ps_solve_reduced: the same
  E  ps_solve / ps_solve_lm: the device loops over A and B
  (D, the core's own sharded loop: tests/test_gpu_sharded.py)

A forced handle F runs beside a clean handle C made from the same tables with the same options.  The bounds are those the suite
already holds two FORMS of the same solve to (tests/test_gpu_ldi.py: test_one_launch_explicit_pcg_matches_the_three_launch_form):
the step against the fp64 oracle's direct solve 1e-8 relative, costs 1e-10 relative, parameters 1e-9 -- F's repeat is another
form of C's solve (A: the right-hand-side-only set-up of the synchronous solver; B: three launches per iteration where C runs
one).  The step of the forced iteration is asserted to be larger than 1e-4, so a step applied twice, applied to the points and
not the poses, or taken from a stale x shows at the size of the step and not of the tolerance.

The hook keeps its one pass off the one-launch-per-SOLVE forms (cg_persist, xcg_persist: no host step between iterations), so
the options stay at their defaults here.  The time-out branches (ST_PERSIST_FAIL) and the "stalled" half of B's condition are
not driven: they would need a kernel spun to its one-second limit."""
import numpy as np
import pytest

from oracle import gn_oracle as orc

pytestmark = pytest.mark.gpu

REL_BOUND = 1e-12          # relative residual every solve here is held to, clean or repeated (pcg_tol 1e-13)
PCG_TOL = 1e-13


def _lp(shape):
    from pyslam_amd import synthetic, losses
    if shape == 'ba60':        # tests/test_gpu_edges.py: test_forced_restart_of_the_pipelined_cg_reaches_the_same_solution
        return synthetic.stereo_ba(num_kf=60, num_lm=5000, obs_per_lm=6, half_window=9, seed=21)[0]
    if shape == 'ba40':        # tests/test_gpu_sharded.py
        return synthetic.stereo_ba(num_kf=40, num_lm=4000, obs_per_lm=6, half_window=8, seed=3)[0]
    if shape == 'pg600':       # tests/test_gpu_ldi.py
        return synthetic.pose_graph(num_poses=600, num_loops=2401, dof=6, seed=2, loss=losses.HuberLoss(1.0))[0]
    assert shape == 'lm'       # tests/test_gpu_lm.py: _long_tracks (240 unknowns: beyond the direct solve)
    return synthetic.stereo_ba(num_kf=40, num_lm=90, obs_per_lm=24, half_window=20, seed=3, pose_noise=0.05, point_noise=0.1)[0]


# name -> (shape, options, branch).  lagged_inverse 0: otherwise the lagged dense inverse takes iterations 2 and later of the folded CG
CONFIGS = {
    'folded-auto': ('ba60', dict(coarse_groups=-1, lagged_inverse=0), 'A'),
    'folded-fine': ('ba60', dict(coarse_groups=0, lagged_inverse=0), 'A'),
    # (coarse_groups 8: the one-launch form needs at most three coarse nodes under eight consecutive rows -- build_coarse: xf_ok --
    #  and the level these options get by themselves on 39 reduced poses, 19 intervals, is too fine for it: xcg_fused_solves stayed 0.
    #  By itself the level admits the form from about 170 keyframes on; the 40-keyframe problem with 8 intervals reaches the same
    #  kernels at a quarter of the size)
    'ba-explicit': ('ba40', dict(cg_explicit_min_rows=0, cg_split_min_rows=0, coarse_groups=8, lagged_inverse=0), 'B'),
    'pg-one-launch': ('pg600', dict(xcg_fused=1, lagged_inverse=0), 'B'),
    'pg-two-launch': ('pg600', dict(xcg_fused=2, lagged_inverse=0), 'B'),
}
_LPS = {}


def lp_of(name):
    shape = CONFIGS[name][0] if name in CONFIGS else name
    if shape not in _LPS:
        _LPS[shape] = _lp(shape)
    return _LPS[shape]


def make(name, **more):
    from pyslam_amd.device import DeviceProblem
    dev = DeviceProblem(lp_of(name))
    for k, v in dict(CONFIGS[name][1], **more).items():
        dev.set_option(k, v)
    return dev


def device_dx(dev):
    xp, xl = dev.get_dx()
    return np.concatenate([xp.ravel(), xl.ravel()])


def counters(dev):
    i = dev.get_info()
    return i['cg_restarts'], i['xcg_fused_solves'], i['xcg_fused_fallbacks']


def at_params(lp, dev):
    cur = lp.copy()
    cur.poses, cur.points = dev.get_params()
    return cur


def mid_n(its_clean):
    """A breakdown in mid-solve: beyond the 12 head launches after which the explicit PCG's side stream is kicked (xcg_side_enqueue)
    where the clean solve is long enough, and at least three iterations before it converges."""
    return max(2, min(14, its_clean - 3))


def params_close(a, b, tol=1e-9):
    pa, pb = a.get_params(), b.get_params()
    assert np.abs(pa[0] - pb[0]).max() < tol
    if pa[1].size:
        assert np.abs(pa[1] - pb[1]).max() < tol


@pytest.mark.parametrize('where', ['first', 'mid'])
@pytest.mark.parametrize('arm_it', [1, 2])
@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_a_forced_breakdown_in_a_whole_iteration_call(name, arm_it, where):
    """Branches A and B.  Armed in front of iteration 1 (a fresh handle) or 2 (the previous tail's successor landmark pass and the
    lagged coarse operators exist); n = 1 (the very first CG iteration) or mid-solve, from the clean handle's own count.

    Bit for bit where the code says so: armed in front of iteration 1, B's repeat enqueues what a handle with xcg_fused 0 enqueues
    for its first iteration -- no lagged coarse inverse exists yet (lci_next == -1), so both set-ups are xcg_setup's exact branch
    on the same S and g, followed by three launches per iteration; the broken pass wrote only CG vectors that the set-up
    initialises again.  There the step, the cost and the iteration count must EQUAL the three-launch handle's.  Armed in front of
    iteration 2 the two linearise at points that differ in the last bits (one launch per iteration against three in iteration 1),
    so the tolerance stays.  A's repeat starts from k_cg_prepare's right-hand-side-only set-up: another form, the tolerance stays.

    The three-launch handle T runs with coarse_lag 0: the repeat factors the CURRENT coarse matrix (xcg_setup(h, max_iters, false)),
    so T's set-up must do so too if its iteration count is to say anything about the repeat's -- on the pose graph a lagging handle
    takes 92 iterations in its second call (its coarse inverse is from the other side of the first, big step), the repeat 66."""
    lp, branch = lp_of(name), CONFIGS[name][2]
    F, Cn = make(name), make(name)
    T = make(name, xcg_fused=0, coarse_lag=0) if branch == 'B' else None      # the form and the set-up B falls back to
    before = counters(F)
    fused_before_next = None
    for it in (1, 2, 3):
        rc = Cn.gn_iteration(0., PCG_TOL, 3000, True)
        rt = T.gn_iteration(0., PCG_TOL, 3000, True) if T is not None else None
        forced = it == arm_it
        if forced:
            n = 1 if where == 'first' else mid_n(rc[2])
            if where == 'mid' and name.startswith('pg'):
                assert n == 14                                        # (the pose graph carries "beyond the head launches")
            cur = at_params(lp, F)
            dx_ref, _ = orc.gauss_newton_step(cur, points_first=False)
            F.set_option('cg_force_breakdown', n)
            assert F.get_option('cg_force_breakdown') == n
        if it == arm_it + 1:
            fused_before_next = counters(F)[1]
        rf = F.gn_iteration(0., PCG_TOL, 3000, True)
        print('{} it {} n {}: clean {} forced {} three-launch {}'.format(name, it, n if forced else '-', rc, rf, rt))
        if forced:
            # 1. counters; the option has cleared itself
            assert F.get_option('cg_force_breakdown') == 0
            restarts, _, fell = counters(F)
            if branch == 'A':
                assert restarts >= before[0] + 1 and fell == 0
            else:
                assert fell == 1 and restarts == before[0]
            # 2. the forced step against the fp64 direct solve at F's own linearisation point
            dx = device_dx(F)
            err = np.linalg.norm(dx - dx_ref) / np.linalg.norm(dx_ref)
            print('   |dx - dx_ref| / |dx_ref| = {:.3e}, max |dx| = {:.3e}'.format(err, np.abs(dx).max()))
            assert err <= 1e-8
            assert np.abs(dx).max() > 1e-4
        # 3. applied once, and whole
        assert abs(rf[0] - rc[0]) <= 1e-10 * abs(rc[0])
        params_close(F, Cn)
        if forced:
            # 4. the statistics reported are the repeat's
            assert rf[3] <= REL_BOUND and rc[3] <= REL_BOUND
            if T is not None:
                assert abs(rf[2] - rt[2]) <= 2
                if arm_it == 1:
                    assert rf[2] == rt[2] and rf[0] == rt[0]
                    assert np.array_equal(dx, device_dx(T))
        else:
            # 5. the un-forced iterations around it: the clean handle's count
            assert abs(rf[2] - rc[2]) <= 2 and rf[3] <= REL_BOUND
        if forced:
            assert abs(F.eval_cost(True) - rf[0]) <= 1e-12 * abs(rf[0])
            Cn.eval_cost(True)                                        # (the same calls on both handles)
            if T is not None:
                T.eval_cost(True)
        if branch == 'B' and it == arm_it + 1:
            # 5. xf_skip is consumed by the repeat's own set-up (xcg_setup): the fallback is for one solve, not for ever
            assert counters(F)[1] == fused_before_next + 1 and counters(F)[2] == 1
    assert counters(Cn)[0] == 0 and counters(Cn)[2] == 0
    if branch == 'B':
        assert counters(Cn)[1] >= 3                                  # the one- / two-launch form is what the clean handle runs
        assert counters(T)[1:] == (0, 0)
    for d in (F, Cn, T):
        if d is not None:
            d.close()


@pytest.mark.parametrize('where', ['first', 'mid'])
@pytest.mark.parametrize('name', ['ba-explicit', 'pg-one-launch'])
def test_a_forced_breakdown_through_the_staged_api(name, where):
    """Branch C: ps_linearize, the forced ps_solve_reduced (xcg_run repeats the solve in the three-launch form), ps_backsub."""
    F, Cn, T = make(name), make(name), make(name, xcg_fused=0)
    for d in (F, Cn, T):
        d.linearize(0.)
    its_c, rel_c = Cn.solve_reduced(PCG_TOL, 3000)
    its_t, _ = T.solve_reduced(PCG_TOL, 3000)
    n = 1 if where == 'first' else mid_n(its_c)
    F.set_option('cg_force_breakdown', n)
    its_f, rel_f = F.solve_reduced(PCG_TOL, 3000)
    print('{} n {}: clean {} {:.2e} forced {} {:.2e}'.format(name, n, its_c, rel_c, its_f, rel_f))
    assert F.get_option('cg_force_breakdown') == 0
    assert counters(F)[2] == 1 and counters(Cn)[2] == 0 and counters(Cn)[1] >= 1
    assert rel_f <= REL_BOUND and rel_c <= REL_BOUND and abs(its_f - its_t) <= 2        # the repeat's statistics: the three-launch form's
    F.backsub(); Cn.backsub()
    a, b = device_dx(Cn), device_dx(F)
    assert np.linalg.norm(a - b) <= 1e-9 * np.linalg.norm(a)
    assert np.abs(b).max() > 1e-4
    assert np.array_equal(Cn.reduced_system()[3], F.reduced_system()[3])        # the right-hand side is as the linearisation left it
    F.close(); Cn.close(); T.close()


def _solve_options(**kw):
    from pyslam_amd.problem import Options
    opt = Options()
    opt.pcg_tol, opt.pcg_max_iters = PCG_TOL, 3000
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


@pytest.mark.parametrize('name', ['folded-auto', 'ba-explicit'])
def test_a_forced_breakdown_inside_the_device_loop(name):
    """Branch E: ps_solve over A and over B, the hook armed in front of the loop (its first iteration breaks down at n = 1)."""
    from pyslam_amd.problem import device_solve
    opt = _solve_options(allow_nondecreasing_steps=True, max_nondecreasing_steps=3)
    out = []
    for n in (0, 1):
        dev = make(name)
        dev.set_option('cg_force_breakdown', n)
        hist, stats = device_solve(dev, opt)
        assert dev.get_option('cg_force_breakdown') == 0
        out.append((hist, stats, dev.get_params(), counters(dev)))
        dev.close()
    (hc, sc, pc, cc), (hf, sf, pf, cf) = out
    print(name, hc, hf, sc, sf, cc, cf)
    assert len(hf) == len(hc)
    assert np.abs(np.array(hf) - np.array(hc)).max() <= 1e-10 * abs(hc[0]) and all(abs(a - b) <= 1e-10 * abs(b) for a, b in zip(hf, hc))
    assert np.abs(pf[0] - pc[0]).max() < 1e-9 and np.abs(pf[1] - pc[1]).max() < 1e-9
    assert all(r <= REL_BOUND for _, r in sf)
    if CONFIGS[name][2] == 'A':
        assert cf[0] >= 1 and cc[0] == 0
    else:
        assert cf[2] == 1 and cc[2] == 0 and cf[1] >= 2 and cc[1] >= 2


def test_a_forced_breakdown_inside_the_adaptive_lm_loop():
    """Branch E under Options.lm_adaptive (ps_solve_lm; the long-track problem of tests/test_gpu_lm.py, whose 240 unknowns take the
    folded CG): the same decisions, accepted and rejected, as the clean solve."""
    from pyslam_amd.device import DeviceProblem
    from pyslam_amd.problem import device_solve
    lp = lp_of('lm')
    opt = _solve_options(lm_adaptive=True, max_iters=12, min_cost_decrease=0.999999)
    out = []
    for n in (0, 1):
        dev = DeviceProblem(lp)
        dev.set_option('cg_force_breakdown', n)
        hist, _ = device_solve(dev, opt)
        assert dev.get_option('cg_force_breakdown') == 0
        out.append((hist, dev.lm_history.copy(), dev.get_params(), dev.cg_restarts()))
        dev.close()
    (hc, rows_c, pc, rc), (hf, rows_f, pf, rf) = out
    print(hc, hf, rows_c[:, 2], rows_f[:, 2], rc, rf)
    assert rf >= 1 and rc == 0
    assert len(hf) == len(hc) and all(abs(a - b) <= 1e-10 * abs(b) for a, b in zip(hf, hc))
    assert np.array_equal(rows_f[:, 2], rows_c[:, 2])                          # accepted / rejected
    assert np.abs(pf[0] - pc[0]).max() < 1e-9 and np.abs(pf[1] - pc[1]).max() < 1e-9


@pytest.mark.parametrize('name', ['folded-auto', 'ba-explicit'])
def test_two_forced_runs_are_bit_identical(name):
    """The fallback itself is deterministic: two fresh handles, the hook armed in front of iteration 2 at n = 5."""
    runs = []
    for _ in range(2):
        dev = make(name)
        trace = []
        for it in (1, 2, 3):
            if it == 2:
                dev.set_option('cg_force_breakdown', 5)
            trace.append(dev.gn_iteration(0., PCG_TOL, 3000, True))
        runs.append((trace, dev.get_params(), counters(dev)))
        dev.close()
    (ta, pa, ca), (tb, pb, cb) = runs
    assert ta == tb and ca == cb and (ca[0] >= 1 or ca[2] == 1)
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
