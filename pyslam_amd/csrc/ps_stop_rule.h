/* ps_stop_rule.h -- THE stopping rule of Problem.solve (reference pyslam/problem.py:159-178), once, for every solve loop of
 * the core: ps_solve and ps_solve_lm on the host, k_motion_only_solve and k_dense_finish on the device.  The Python loops
 * drive the same contract (pyslam_amd/problem.py: StopRule); tests/test_stop_rule_host.py compiles this header with a C
 * compiler and holds the two, and an independent restatement of the reference loop, against each other.
 *
 * Written in the common subset of C99 and C++, with no HIP types: PS_HD is `__host__ __device__` under hipcc and nothing
 * for any other compiler.
 *
 * The rule, after every iteration (its cost, and the norm of its step):
 *   - stop when iterations > max_iters, ||dx|| < min_update_norm or cost < min_cost                          (ps_stop_base);
 *   - a step is NON-DECREASING when cost >= min_cost_decrease * previous cost (the tie counts as non-decreasing), the
 *     previous cost being the history entry in front of it.  A loop without a line search records the cost of each
 *     iteration's linearisation point, so its first iteration repeats the start cost and is a non-decreasing step;
 *   - without allow_nondecreasing_steps the first non-decreasing step stops the loop;
 *   - with it, the parameters are kept as `best` while the count of consecutive non-decreasing steps is 0 ON ENTRY (i.e.
 *     before this step moves the count), and once the count reaches max_nondecreasing_steps the loop stops and `best` is
 *     restored.  With max_nondecreasing_steps == 1 both happen in the same iteration: the caller stores, then restores.
 */
#ifndef PS_STOP_RULE_H
#define PS_STOP_RULE_H

#include <stdint.h>
#include "pyslam_hip.h"

#if defined(__HIPCC__)
#define PS_HD __host__ __device__
#else
#define PS_HD
#endif

typedef struct ps_stop_state {
    int32_t iters, nd;      /* iterations judged so far; consecutive non-decreasing steps */
    double cost;            /* the last entry of the cost history */
} ps_stop_state;

/* flags of ps_stop_step.  KEEP_BEST: store the CURRENT (post-step) parameters as best, now.  RESTORE_BEST (implies DONE): make
   best the current parameters.  Both set: store first, then restore. */
enum { PS_STOP_DONE = 1, PS_STOP_KEEP_BEST = 2, PS_STOP_RESTORE_BEST = 4 };

PS_HD static inline void ps_stop_begin(ps_stop_state* s, double start_cost) {
    s->iters = 0; s->nd = 0; s->cost = start_cost;
}

/* the three threshold tests (all the adaptive LM loop shares with the default one) */
PS_HD static inline int ps_stop_base(const ps_solve_options* o, int32_t iters, double cost, double dx_norm) {
    return iters > o->max_iters || dx_norm < o->min_update_norm || cost < o->min_cost;
}

/* one finished iteration: `cost` joins the history, the counters move; -> flag set */
PS_HD static inline int ps_stop_step(const ps_solve_options* o, ps_stop_state* s, double cost, double dx_norm) {
    const int nondecreasing = cost >= o->min_cost_decrease * s->cost;
    int flags;
    s->iters += 1;
    s->cost = cost;
    flags = ps_stop_base(o, s->iters, cost, dx_norm) ? PS_STOP_DONE : 0;
    if (o->allow_nondecreasing_steps) {
        if (s->nd == 0) flags |= PS_STOP_KEEP_BEST;
        s->nd = nondecreasing ? s->nd + 1 : 0;
        if (s->nd >= o->max_nondecreasing_steps) flags |= PS_STOP_DONE | PS_STOP_RESTORE_BEST;
    } else if (nondecreasing) {
        flags |= PS_STOP_DONE;
    }
    return flags;
}

/* iterations the rule still allows AFTER the one about to start if its step turns out non-decreasing (ps_set_option
   "solve_horizon"): none without allow_nondecreasing_steps, else what max_nondecreasing_steps and max_iters leave */
PS_HD static inline int ps_stop_horizon(const ps_solve_options* o, const ps_stop_state* s) {
    const int left_nd = o->max_nondecreasing_steps - (s->nd + 1);
    const int left_it = o->max_iters - s->iters;      /* the loop stops once its counter exceeds max_iters */
    const int left = left_nd < left_it ? left_nd : left_it;
    return !o->allow_nondecreasing_steps || left < 0 ? 0 : left;
}

#endif
