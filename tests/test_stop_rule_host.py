"""The stopping rule of every solve loop, once in C (pyslam_amd/csrc/ps_stop_rule.h, compiled here with a plain C compiler: no
HIP, no GPU) and once in Python (pyslam_amd/problem.py: StopRule), against each other and against the independent restatement
of the reference's loop (tests/test_solve_loop_cpu.py: reference_loop) on one table of scripted solves: where each stops,
where best was last kept, whether it was restored, and the horizon announced before every iteration."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from pyslam_amd import _native as nat
from pyslam_amd.device import _solve_options
from pyslam_amd.problem import Options, StopRule, solve_horizon
from test_solve_loop_cpu import CASES, reference_loop

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DONE, KEEP, RESTORE = StopRule.DONE, StopRule.KEEP_BEST, StopRule.RESTORE_BEST

SHIM = r'''
#include "ps_stop_rule.h"
/* a whole scripted solve: costs[0] is the start cost, costs[k] / dx[k - 1] belong to iteration k.  -> history length, or -1
   when the n entries ran out before the rule stopped the loop */
int replay(const ps_solve_options* o, const double* costs, const double* dx, int n, int* flags, int* horizon) {
    ps_stop_state s;
    int k = 0, f = 0;
    ps_stop_begin(&s, costs[0]);
    while (!(f & PS_STOP_DONE) && k + 1 < n) {
        horizon[k] = ps_stop_horizon(o, &s);
        f = ps_stop_step(o, &s, costs[k + 1], dx[k]);
        flags[k++] = f;
    }
    return (f & PS_STOP_DONE) && s.iters == k && s.cost == costs[k] ? k + 1 : -1;
}
int base(const ps_solve_options* o, int iters, double cost, double dx) { return ps_stop_base(o, iters, cost, dx); }
int flag_values(void) { return PS_STOP_DONE | PS_STOP_KEEP_BEST << 4 | PS_STOP_RESTORE_BEST << 8; }
'''


@pytest.fixture(scope='module')
def crule(tmp_path_factory):
    """The header as C99 in a shared library (the project needs gcc to build at all: a missing compiler is a failure)."""
    d = tmp_path_factory.mktemp('stop_rule')
    src, lib = str(d / 'shim.c'), str(d / 'shim.so')
    with open(src, 'w') as f:
        f.write(SHIM)
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-O1', '-shared', '-fPIC', '-I' + os.path.join(REPO, 'include'),
                    '-I' + os.path.join(REPO, 'pyslam_amd', 'csrc'), src, '-o', lib], check=True)
    so = C.CDLL(lib)
    assert so.flag_values() == DONE | KEEP << 4 | RESTORE << 8
    return so


def make_opt(**kw):
    opt = Options()
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def c_options(opt):
    return _solve_options(nat.SolveOptions(), opt)          # (the one fill of ps_solve_options from an Options)


def run_c(so, opt, costs, dx):
    n = len(costs)
    flags, hor = (C.c_int * n)(), (C.c_int * n)()
    nh = so.replay(C.byref(c_options(opt)), (C.c_double * n)(*costs), (C.c_double * n)(*dx), n, flags, hor)
    assert nh >= 2, 'the C rule did not stop within the scripted costs'
    return list(flags[:nh - 1]), list(hor[:nh - 1])


def run_python(opt, costs, dx):
    rule, flags, hor = StopRule(opt, costs[0]), [], []
    while not (flags and flags[-1] & DONE):
        hor.append(rule.horizon())
        flags.append(rule.step(costs[rule.iters + 1], dx[rule.iters]))
        assert rule.iters == len(flags) and rule.cost == costs[rule.iters]
    return flags, hor


def summary(flags):
    """(iterations, iteration at which best was last kept or None, restored); the flags keep their contract."""
    assert all(not f & DONE for f in flags[:-1]) and flags[-1] & DONE
    assert all(not f & RESTORE for f in flags[:-1])               # RESTORE_BEST implies DONE
    kept = [k + 1 for k, f in enumerate(flags) if f & KEEP]
    return len(flags), (kept[-1] if kept else None), bool(flags[-1] & RESTORE)


def reference(opt, costs, dx):
    """reference_loop takes one ||dx|| for the whole solve.  A sequence that stays >= min_update_norm up to iteration K - 1
    and is below it at K stops the loop at K (unless something stops it earlier) with every other statement of iteration K
    run as usual -- exactly what `it > max_iters` does with max_iters = K - 1.  So: the reference on a constant large ||dx||
    with max_iters cut to K - 1."""
    below = [k + 1 for k, d in enumerate(dx) if d < opt.min_update_norm]
    ref_opt = make_opt(**vars(opt))
    if below:
        assert all(d < opt.min_update_norm for d in dx[below[0] - 1:])          # (crosses once)
        ref_opt.max_iters = min(opt.max_iters, below[0] - 1)
    ref_opt.min_update_norm = 0.
    return reference_loop(costs, ref_opt, dx_norm=1.0)


def check(so, opt, costs, dx=None):
    costs = [float(c) for c in costs]
    dx = [1.0] * len(costs) if dx is None else dx
    fc, hc = run_c(so, opt, costs, dx)
    fp, hp = run_python(opt, costs, dx)
    assert fc == fp and hc == hp                                   # C == Python: every flag, every horizon
    iters, kept, restored = summary(fp)
    hist, best_at = reference(opt, costs, dx)
    assert iters == len(hist) - 1                                  # == the reference: where it stops,
    assert restored == (best_at is not None)                       # whether best is restored,
    if restored:
        assert kept == best_at                                     # and which parameters those are
    assert (kept is not None) == bool(opt.allow_nondecreasing_steps)
    nd = 0                                                         # the horizon, from the history alone
    for it in range(1, iters + 1):
        assert hp[it - 1] == solve_horizon(opt, it, nd)
        nd = nd + 1 if hist[it] >= opt.min_cost_decrease * hist[it - 1] else 0
    return iters, kept, restored


def pad(costs, opt):
    """The scripted costs, continued (decreasing by 1 % a step) so that max_iters stops the loop if nothing else does."""
    out = list(costs)
    while len(out) < opt.max_iters + 3:
        out.append(out[-1] * 0.99)
    return out


@pytest.mark.parametrize('kw,costs', CASES)
def test_the_cases_of_the_python_loop(crule, kw, costs):
    check(crule, make_opt(**kw), costs)


# costs that fall fast, stall (non-decreasing under min_cost_decrease), fall again below min_cost = 50 and stall for good
GRID_COSTS = [1000., 400., 399.9, 399.8, 120., 60., 59.99, 40., 39.99, 39.98, 39.97, 39.96]
GRID_DX = [1., 0.5, 0.2, 0.1, 5e-2, 1e-2, 5e-3, 2e-3, 5e-4, 1e-4]          # crosses min_update_norm = 1e-3 at iteration 9


def test_the_option_grid(crule):
    n = 0
    for allow, max_nd, max_iters, min_cost, min_dx in itertools.product((0, 1), (1, 2, 3), (0, 1, 3, 30), (0., 50.), (0., 1e-3)):
        opt = make_opt(allow_nondecreasing_steps=bool(allow), max_nondecreasing_steps=max_nd, max_iters=max_iters,
                       min_cost=min_cost, min_update_norm=min_dx)
        costs = pad(GRID_COSTS, opt)
        dx = GRID_DX + [GRID_DX[-1]] * (len(costs) - len(GRID_DX))
        iters, _, _ = check(crule, opt, costs, dx)
        assert iters <= max_iters + 1
        n += 1
    assert n == 96


def test_seeded_random_cost_sequences(crule):
    rng = np.random.default_rng(20240607)
    for _ in range(48):
        opt = make_opt(allow_nondecreasing_steps=bool(rng.integers(2)), max_nondecreasing_steps=int(rng.integers(1, 5)),
                       max_iters=int(rng.integers(0, 25)), min_cost=float(rng.choice([0., 1., 30.])),
                       min_cost_decrease=float(rng.choice([0.5, 0.9, 0.99, 1.0])))
        factors = rng.choice([0.3, 0.6, 0.95, 0.995, 1.0, 1.2], size=opt.max_iters + 2)
        check(crule, opt, np.concatenate([[100.], 100. * np.cumprod(factors)]))


def test_a_tie_is_a_non_decreasing_step(crule):
    # prev = 100, min_cost_decrease = 0.5, cost = 50: cost >= 0.5 * 100 holds with equality (all three exact in binary)
    assert check(crule, make_opt(min_cost_decrease=0.5), [100., 50., 1.]) == (1, None, False)
    assert check(crule, make_opt(min_cost_decrease=0.5), [100., 49.999, 0.5 * 49.999, 1.]) == (2, None, False)
    allow = dict(allow_nondecreasing_steps=True, min_cost_decrease=0.5)
    assert check(crule, make_opt(max_nondecreasing_steps=1, **allow), [100., 50., 1.]) == (1, 1, True)      # keep and restore at once
    assert check(crule, make_opt(max_nondecreasing_steps=2, **allow), [100., 50., 25., 1.]) == (2, 1, True)
    assert check(crule, make_opt(max_nondecreasing_steps=2, **allow), [100., 50., 24., 12., 6., 1.]) == (4, 3, True)


def test_the_first_iteration_without_a_line_search_repeats_the_start_cost(crule):
    # such a loop records the cost of each iteration's linearisation point: iteration 1 compares the start cost with itself
    costs = [100., 100., 10., 1., 0.1, 0.01]
    assert check(crule, make_opt(), costs) == (1, None, False)                                               # the defaults stop at once
    assert check(crule, make_opt(allow_nondecreasing_steps=True, max_nondecreasing_steps=1), costs) == (1, 1, True)
    assert check(crule, make_opt(allow_nondecreasing_steps=True, max_nondecreasing_steps=2, max_iters=3), costs) == (4, 4, False)


def test_the_threshold_tests(crule):
    opt = make_opt(max_iters=3, min_update_norm=1e-3, min_cost=50.)
    for iters, cost, dx in itertools.product((3, 4), (50., 49.), (1e-3, 9e-4)):
        want = iters > 3 or dx < 1e-3 or cost < 50.                 # (>, <, <: the values AT the thresholds do not stop)
        assert bool(crule.base(C.byref(c_options(opt)), iters, C.c_double(cost), C.c_double(dx))) == want
        assert StopRule.base(opt, iters, cost, dx) == want
