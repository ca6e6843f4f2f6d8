// ps_k_cg_persist.h -- the folded two-level CG of small and medium reduced systems in ONE launch (round 5).
// Part of ps_kernels.h (included from there, after ps_k_cg_fused.h; not a stand-alone header).
#pragma once

// ---------------------------------------------------------------------------
// k_cg_fused_lds runs one CG iteration per launch: 5.0-5.4 us each at C3 (a kernel boundary, one memory round trip for the
// 5.7 MB matrix out of the Infinity Cache, one block reduction), 18-21 of them per Gauss-Newton iteration = 40 % of it.
// Nothing in an iteration needs a kernel boundary except that every workgroup needs all of w = S^ r of the others.  Here
//   * the augmented matrix stays IN REGISTERS for the whole solve: a wave owns one "task" = at most 48 blocks of one block row
//     (half a fine row at C3, a fifth of a dense coarse row; the zero padding of an ELL row is left out), lane (slot, r) holds
//     row r of 6 of them (36 doubles);
//   * the vectors r, s, p, x are REPLICATED: every workgroup keeps all n entries (four per thread) and applies the same
//     recurrences with the same alpha / beta -- bitwise the same everywhere, so nobody has to agree on anything;
//   * per iteration ONE exchange: a wave publishes the six sums of its task as self-tagged 8-byte granules {tag | half of the
//     double} with write-through stores, every workgroup gathers all of them with relaxed agent-scope loads (no flags, no
//     fences, no grid barrier: the data is the flag -- /opt/skills/guides/cdna_hip_programming.md guideline 16, form R2),
//     double-buffered by the parity of the iteration (a workgroup can only be one exchange ahead of the slowest).  A thread
//     loads the granules of ITS four entries' tasks itself and adds them in task order: no staging in LDS, and TWO workgroup
//     barriers per iteration (r_new in LDS before the products; the partial sums of delta), not three;
//   * gamma = r.r and delta = w.r are summed by every workgroup itself, in the same order;
//   * gamma_new = r_new . r_new is known BEFORE the exchange, with the same bits everywhere: a solve that has converged leaves
//     there, without the exchange whose w_new and delta nothing would read -- K exchanges for K iterations, not K + 1.
// Measured on the chip before it was built (tools/probes/allgather_probe.hip): 2.0-2.7 us per exchange for 32 workgroups of 512
// threads, whatever their number -- against 5.4 us per launch.  In the kernel: ~4.5 us per CG iteration at C3 (58 workgroups),
// 3.6 on a 100-pose graph (the flat gather through LDS of round 5, two instantiations by the number of exchanged sums per
// thread; with the gather per entry there is one per D, up to 1 024 tasks, and an iteration at C3 is ~0.45 us shorter).
// Every spin is bounded: a workgroup that does not see its granules within `spin_limit` passes or one second reports a breakdown
// (ST_PCG_DONE = 2, ST_PERSIST_FAIL) and leaves; the host then solves with the launch-per-iteration kernels and stops using
// this one on the handle.
// Semantics = the launches k = -1, 0, 1, ... of k_cg_fused_lds: same recurrences (Chronopoulos-Gear), same convergence test,
// same status words, history (gamma, alpha per iteration) and scalars; sums in another (fixed) order.
// ---------------------------------------------------------------------------
#define PS_CP_NT 512                    // threads per workgroup (8 waves = 8 tasks)
#define PS_CP_NQ 6                      // blocks per lane slot: a task has at most 8 * PS_CP_NQ blocks
#define PS_CP_TASKB (8 * PS_CP_NQ)
#define PS_CP_NV 4                      // vector entries per thread: n <= PS_CP_NV * PS_CP_NT
#define PS_CP_MAXEX (12 * PS_CP_NT)     // exchanged sums per iteration: tasks * D <= PS_CP_MAXEX (1 024 tasks of SE(3) rows)
#define PS_CP_MAXN (PS_CP_NV * PS_CP_NT)
#define PS_CP_LONG 4                    // tasks of a long row (more than two tasks) gathered at a time
#define PS_CP_NCLK 16                   // words of the measurement build's phase clocks (PS_CP_CLOCKS): 0-7 the loop, 4 the recovery, 8 the prologue
// Wall-clock bound of a spin (wall_clock64: 100 MHz), beside the bound in passes: ONE SECOND.  Round 6 first took the 20 ms
// k_xcg_persist had: with two PROCESSES on one device (tests/test_gpu_sharded.py: two ranks on one GPU) the scheduler suspends a
// process's queues for whole time slices, a spin that straddles a slice sees the clock jump by more than that, and one solve in
// ~5 reported a time-out although every workgroup was resident.  The bound exists so that a grid that can never be resident
// does not hang the stream, not to police latency: residency is decided up front from the device (ps_core.hip: PersistLedger).
#define PS_PERSIST_TIMEOUT_TICKS 100000000LL
#ifndef PS_CP_SLEEP
#define PS_CP_SLEEP 1                   // s_sleep argument between two unsuccessful passes over the exchange (0: none)
#endif

struct CpTask { int32_t row, b0, b1, pad; };
// what k_coarse_recover needs: x = L^-T (x^_f + P y), y = L_c^-T x^_c -- done inside the launch once the solve has converged
// (x == NULL: not done here).  Workgroup b recovers poses [b pp, (b + 1) pp), pp = ceil(nr / workgroups) (C3: 58 workgroups, 4
// poses each), from operands it copied into LDS at kernel entry: every operand is final before the launch, every workgroup holds
// all of x^ with the same bits -- so nothing of the recovery is a dependent trip to memory behind the solve, and no workgroup
// waits for another.  (Rounds 5-6: the first workgroup alone, out of memory, while the others had left: ~20 serialised round trips.)
// maxcols: the most columns of L_c^-1 a slice's nodes select (the host's plan: build_coarse), which fixes the LDS layout.
struct CpRecover { int nr, ncb; const int32_t* pnode; const double *pw0, *pw1, *Linv, *Lci, *Bmat; double* x; int pp, maxcols; };
// The most dynamic LDS a slice's operands may take.  At 256 VGPRs the kernel's 8 waves fill a compute unit's registers (2 waves per
// SIMD): one workgroup per unit, which has the unit's 160 KB of LDS to itself -- less the static 16.3 KB (rn with the time-out flag, red), rounded to
// 17 KB: 143 KB.  (C3 needs 13.4 KB.)  A larger need: rec.x == NULL and k_coarse_recover behind the launch.
#define PS_CP_RECOVER_LDS_CAP ((160 - 17) * 1024)
// dynamic LDS of a launch whose slices are `pp` poses and select at most `maxcols` columns of L_c^-1 (nc rows each):
// columns | B, Linv, pw0, pw1 of the slice | y of the columns | pnode of the slice, its first node and number of columns
inline size_t cp_recover_lds(int D, int nc, int pp, int maxcols) {
    return ((size_t)maxcols * nc + (size_t)pp * (2 * D * D + 2) + maxcols) * sizeof(double) + (size_t)(pp + 2) * sizeof(int32_t);
}

typedef unsigned long long ps_u64;
typedef __attribute__((address_space(1))) ps_u64 ps_gu64;

// Round 6: both granules of a double PUBLISHED by one 16-byte store -- `global_store_dwordx4 ... sc1`, the same bits and cache policy
// as the two relaxed agent-scope 8-byte stores (`global_store_dwordx2 ... sc1`) it replaces, half the write requests.  A granule still
// carries its own tag and lands by an aligned 8-byte half of the access, so a reader that sees one new half and one old one retries
// as before.  (k_xcg_persist at C4: first pass over the exchange 4.7 -> 4.0 us; k_cg_persist at C3: gather 50.4 -> 48.7 us per
// launch.  Readers keep two 8-byte loads per double: 16-byte loads through inline assembly need 128-bit landing tuples --
// k_xcg_persist: scratch 32 -> 190-260 B per lane -- and where there is room for them, k_cg_persist at C3, they measured nothing.)
typedef unsigned ps_u32x4 __attribute__((ext_vector_type(4)));
PS_DEV void cp_put(ps_u64* g, unsigned tag, double v) {
    const ps_u64 b = (ps_u64)__double_as_longlong(v);
    const ps_u32x4 q = {(unsigned)(b & 0xffffffffull), tag, (unsigned)(b >> 32), tag};
    // (`s_nop 1`: on gfx940+ a VALU write to the data registers of a store wider than 64 bits needs two wait states behind it; the
    //  compiler inserts them for its own stores and cannot see into this one -- the next cp_put reuses these very registers)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(g), "v"(q) : "memory");
}

// one granule, `off` bytes into the exchange buffer (32-bit offset arithmetic: with a 64-bit index per load the 24 loads of a
// gather pass took the D = 6 kernel to 60 bytes of scratch per lane; so it has none, at 256 VGPRs)
PS_DEV ps_u64 cp_get(const ps_u64* buf, unsigned off) {
    return __hip_atomic_load((const ps_gu64*)((const char*)buf + off), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int D>
__global__ __launch_bounds__(PS_CP_NT) void k_cg_persist(
    int n /* augmented unknowns */, int ntasks, const CpTask* __restrict__ tasks,
    const int32_t* __restrict__ row_task0 /* first task of every block row; [rows] = ntasks */,
    const int32_t* __restrict__ acol_idx, const double* __restrict__ Saug,
    const double* __restrict__ r0, const double* __restrict__ w0, const double* __restrict__ s0,
    double* __restrict__ p_io, double* __restrict__ x_io,
    double* __restrict__ hist, int cap, int nlaunch /* iterations k = -1 .. nlaunch - 2 at most */, double tol2,
    int32_t* __restrict__ status, double* __restrict__ scalars,
    ps_u64* __restrict__ exch /* 2 x (ntasks * D) doubles as two granules each */, unsigned salt, unsigned spin_limit,
    long long* __restrict__ dbg /* measurement build: phase clocks of workgroup 0 (PS_CP_NCLK words), else NULL */, CpRecover rec)
{
    constexpr int DD = D * D;
    // (static LDS a multiple of 16 bytes, 16 656: the dynamic region behind it starts aligned.  rn[PS_CP_MAXN] is the time-out flag)
    __shared__ double rn[PS_CP_MAXN + 2];
    __shared__ double red[2][2][PS_CP_NT / 64];
    extern __shared__ __attribute__((aligned(16))) double cp_rec[];   // the recovery's operands of this workgroup's slice (rec.x != NULL)
    int& bad = *reinterpret_cast<int*>(&rn[PS_CP_MAXN]);
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63, kk = lane >> 3, r = lane & 7;
    const int task = blockIdx.x * (PS_CP_NT / 64) + wv;
    const bool chief = blockIdx.x == 0 && t == 0;
    const size_t nex = (size_t)ntasks * D;                   // exchanged doubles per iteration
    const long long t_entry = dbg ? wall_clock64() : 0;      // (measurement build: the prologue's clock, dbg[8])
    if (t == 0) bad = 0;
    // ---- the recovery's operands of this workgroup's slice of poses [p0, p0 + np): loaded HERE, stored to LDS behind the loads below
    // (everything is final before the launch and independent of the solve: one round trip beside the prologue's own).  A flat
    // list: entries [0, ncols * nc) are the columns qa D .. of L_c^-1 that the slice's nodes select, rows m >= k of column k only
    // (sLc[j * nc + m]); behind them B, Linv, pw0, pw1 of the slice, in this order.  Nothing of this is carried over the solve loop
    // in a register (the kernel has none to spare): the recovery works its layout out again, and reads the slice's first node
    // and number of columns back from LDS.
    constexpr int PF = 4;                                    // list entries per thread in flight (C3: 1 404 + 296 entries, one trip)
    const int nc = rec.ncb * D, p0 = blockIdx.x * rec.pp;
    const int np = rec.x ? max(0, min(rec.nr, p0 + rec.pp) - p0) : 0;
    int qa = 0, ncols = 0, nlist = 0;
    if (np > 0) {
        int32_t* const spn = reinterpret_cast<int32_t*>(cp_rec + rec.maxcols * nc + rec.pp * (2 * DD + 2) + rec.maxcols);
        qa = rec.pnode[p0];
        ncols = min((min(rec.ncb - 1, rec.pnode[p0 + np - 1] + 1) - qa + 1) * D, rec.maxcols);
        nlist = ncols * nc + np * (2 * DD + 2);
        if (t < np) spn[t] = rec.pnode[p0 + t];
        if (t == 0) { spn[rec.pp] = qa; spn[rec.pp + 1] = ncols; }
    }
    auto rec_src = [&](int idx, int& dst) -> const double* { // list entry idx: where it comes from (NULL: nothing) and goes to
        const int nl = ncols * nc;
        if (idx < nl) {
            const int m = idx / ncols, j = idx - m * ncols, k = qa * D + j;
            dst = j * nc + m;
            return m >= k ? rec.Lci + (size_t)m * nc + k : nullptr;
        }
        const int e = idx - nl, nb = np * DD;
        dst = rec.maxcols * nc + e;
        if (e < nb) return rec.Bmat + (size_t)p0 * DD + e;
        if (e < 2 * nb) return rec.Linv + (size_t)p0 * DD + (e - nb);
        if (e < 2 * nb + np) return rec.pw0 + p0 + (e - 2 * nb);
        return rec.pw1 + p0 + (e - 2 * nb - np);
    };
    double pfv[PF];
    int pfd[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int idx = t + u * PS_CP_NT;
        pfd[u] = -1; pfv[u] = 0.0;
        if (idx < nlist) { int d = 0; const double* src = rec_src(idx, d); if (src) { pfv[u] = *src; pfd[u] = d; } }
    }
    // ---- the task's blocks into registers (once), the vectors' entries of this thread
    int b0 = 0, b1 = 0;
    if (task < ntasks) { const CpTask tk = tasks[task]; b0 = tk.b0; b1 = tk.b1; }
    int cj[PS_CP_NQ];
    double sv[PS_CP_NQ][D];
#pragma unroll
    for (int q = 0; q < PS_CP_NQ; ++q) {
        const int b = b0 + kk + 8 * q;
        cj[q] = 0;
#pragma unroll
        for (int c = 0; c < D; ++c) sv[q][c] = 0.0;
        if (b < b1 && r < D) {
            cj[q] = acol_idx[b] * D;
            const double* sb = Saug + (size_t)b * DD + r * D;
#pragma unroll
            for (int c = 0; c < D; ++c) sv[q][c] = sb[c];
        }
    }
    double vr[PS_CP_NV], vw[PS_CP_NV], vs[PS_CP_NV], vp[PS_CP_NV], vx[PS_CP_NV];
    int e0[PS_CP_NV], en[PS_CP_NV];                          // first exchanged entry and number of tasks of this entry's row
#pragma unroll
    for (int v = 0; v < PS_CP_NV; ++v) {
        const int i = t + v * PS_CP_NT;
        vr[v] = vw[v] = vs[v] = vp[v] = vx[v] = 0.0; e0[v] = 0; en[v] = 0;
        if (i < n) {
            vr[v] = r0[i]; vw[v] = w0[i]; vs[v] = s0[i]; vp[v] = p_io[i]; vx[v] = x_io[i];
            const int row = i / D, ta = row_task0[row];
            e0[v] = ta * D + (i - row * D); en[v] = row_task0[row + 1] - ta;
        }
    }
    int lv = -1, le0 = 0, len = 0;                           // the thread's first entry of a row of more than two tasks
#pragma unroll
    for (int v = PS_CP_NV - 1; v >= 0; --v) if (en[v] > 2) { lv = v; le0 = e0[v]; len = en[v]; }
#pragma unroll
    for (int u = 0; u < PF; ++u) if (pfd[u] >= 0) cp_rec[pfd[u]] = pfv[u];
    for (int base = PF * PS_CP_NT; base < nlist; base += PS_CP_NT) {     // (a longer list: what is left, one entry at a time)
        const int idx = base + t;
        int d = 0;
        const double* src = idx < nlist ? rec_src(idx, d) : nullptr;
        if (src) cp_rec[d] = *src;
    }
    if (status[ST_PCG_DONE]) return;                         // (as every launch of the per-iteration form)
    // (1 / gamma_prev and 1 / alpha_prev are formed while the exchange is in flight: ONE division between an iteration's dot
    //  products and its recurrences -- the per-launch kernels do three, which changes the last bits of alpha and beta, not more)
    double gamma = 0.0, delta = 0.0, inv_gprev = 0.0, inv_aprev = 0.0, thresh = 0.0;
    bool converged = false;
    long long ck[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define PS_CP_CLK(i) do { if (dbg) { const long long now_ = wall_clock64(); ck[i] += now_ - last_; last_ = now_; } } while (0)
    long long last_ = dbg ? wall_clock64() : 0;
    if (dbg && chief) dbg[8] += last_ - t_entry;             // (the prologue: kernel entry to the first pass)
    for (int k = -1; k < nlaunch - 1; ++k) {
        double alpha = 0.0, beta = 0.0;
        if (k >= 0) {
            if (k == 0) thresh = tol2 * gamma;
            if (!(gamma > thresh)) {                         // converged (gamma == 0 too); NaN = breakdown
                if (chief) { atomicMax(&status[ST_PCG_DONE], (gamma != gamma) ? 2 : 1); scalars[SC_RRFINAL] = gamma; if (k == 0) scalars[SC_RR0] = gamma; }
                converged = !(gamma != gamma);
                break;
            }
            beta = (k == 0) ? 0.0 : gamma * inv_gprev;
            const double denom = (k == 0) ? delta : delta - beta * gamma * inv_aprev;
            alpha = gamma / denom;
            if (!(denom > 0.0)) {                            // breakdown: stop, the host reports it
                if (chief) { atomicMax(&status[ST_PCG_DONE], 2); scalars[SC_RRFINAL] = gamma; }
                break;
            }
            if (chief) {
                hist[k] = gamma; hist[cap + k] = alpha; status[ST_PCG_ITERS] = k + 1; scalars[SC_RRFINAL] = gamma;
                if (k == 0) { scalars[SC_THRESH] = thresh; scalars[SC_RR0] = gamma; }
            }
        }
        const double gamma_now = gamma, alpha_now = alpha;
        // ---- the recurrences on every entry (replicated), r_new into LDS for the products
        double gs = 0.0;
#pragma unroll
        for (int v = 0; v < PS_CP_NV; ++v) {
            const int i = t + v * PS_CP_NT;
            const double sn = vw[v] + beta * vs[v];
            const double pn = vr[v] + beta * vp[v];
            const double rnv = cg_rnew(vr[v], vw[v], vs[v], alpha, beta);
            vs[v] = sn; vp[v] = pn; vx[v] += alpha * pn; vr[v] = rnv;
            if (i < n) { rn[i] = rnv; gs += rnv * rnv; }
        }
        double (*rd)[PS_CP_NT / 64] = red[k & 1];
        gs = wave_sum(gs);
        if (lane == 0) rd[0][wv] = gs;
        PS_CP_CLK(0);
        __syncthreads();
        PS_CP_CLK(1);
        double gamma_next = 0.0;                             // r_new . r_new, known before the exchange
#pragma unroll
        for (int w2 = 0; w2 < PS_CP_NT / 64; ++w2) gamma_next += rd[0][w2];
        // ---- converged already?  Then pass k + 1 would only find that out and leave: nothing reads the w_new and delta of this
        // pass (x and p are final above, w and s are never written back), so leave HERE, before the exchange, exactly as the top
        // of pass k + 1 does.  Only where that pass would have run (k + 1 < nlaunch - 1: at the launch cap nothing changes).
        // The decision may depend ONLY on what every workgroup holds with the same bits -- gamma_next, thresh, k, nlaunch -- and
        // never on what one workgroup knows alone (`bad`): a workgroup that stays would wait for granules nobody publishes.
        if (k >= 0 && k + 1 < nlaunch - 1 && !(gamma_next > thresh)) {
            if (chief) { atomicMax(&status[ST_PCG_DONE], (gamma_next != gamma_next) ? 2 : 1); scalars[SC_RRFINAL] = gamma_next; }
            converged = !(gamma_next != gamma_next);
            break;
        }
        // ---- this wave's task: six sums of S^(row, its blocks) r_new, published as tagged granules
        const unsigned tag = salt * 4096u + (unsigned)(k + 2);
        ps_u64* buf = exch + (size_t)(k & 1) * nex * 2;
        {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < PS_CP_NQ; ++q) {
                const double* v = rn + cj[q];
#pragma unroll
                for (int c = 0; c < D; ++c) acc += sv[q][c] * v[c];
            }
            acc += __shfl_xor(acc, 8, 64);
            acc += __shfl_xor(acc, 16, 64);
            acc += __shfl_xor(acc, 32, 64);
            if (task < ntasks && lane < D) cp_put(buf + 2 * ((size_t)task * D + lane), tag, acc);
        }
        if (dbg) ck[6] += 1;                                 // (measurement build: exchanges of this launch)
        if (k >= 0) { inv_gprev = 1.0 / gamma_now; inv_aprev = 1.0 / alpha_now; }     // (while the exchange is in flight)
        PS_CP_CLK(2);
        // ---- gather: every thread loads the granules of ITS entries' tasks itself and sums them in task order from 0.0 (what the
        // flat gather + LDS redistribution summed, bit for bit) -- no staging array, no barrier between gather and dots.  The loads
        // of a pass are issued before any is waited on (one round trip): two tasks per entry unrolled (every fine row), tasks
        // 2 .. 2 + PS_CP_LONG - 1 of the thread's first long entry beside them (a coarse row at C3 has five tasks); what is left
        // (longer rows, a thread's further long entries) follows PS_CP_LONG tasks at a time, in the same pass.
        {
            bool ok = false;
            const long long t_enter = (long long)wall_clock64();        // (bounded in wall-clock time too: PS_PERSIST_TIMEOUT_TICKS)
            for (unsigned spins = 0; !ok; ++spins) {
                ok = true;
                ps_u64 ga[PS_CP_NV][2], gb[PS_CP_NV][2], xa[PS_CP_LONG], xb[PS_CP_LONG];
#pragma unroll
                for (int v = 0; v < PS_CP_NV; ++v)
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
                        ga[v][m] = gb[v][m] = 0;
                        if (m < en[v]) {
                            ga[v][m] = cp_get(buf, 16u * (unsigned)e0[v] + 16u * (m * D));
                            gb[v][m] = cp_get(buf, 16u * (unsigned)e0[v] + 16u * (m * D) + 8u);
                        }
                    }
#pragma unroll
                for (int j = 0; j < PS_CP_LONG; ++j) {
                    xa[j] = xb[j] = 0;
                    if (2 + j < len) {
                        xa[j] = cp_get(buf, 16u * (unsigned)le0 + 16u * ((2 + j) * D));
                        xb[j] = cp_get(buf, 16u * (unsigned)le0 + 16u * ((2 + j) * D) + 8u);
                    }
                }
#define PS_CP_TAKE(a_, b_) do { ok = ok && (unsigned)((a_) >> 32) == tag && (unsigned)((b_) >> 32) == tag;                   \
                                wsum += __longlong_as_double((long long)(((a_) & 0xffffffffull) | ((b_) << 32))); } while (0)
#pragma unroll
                for (int v = 0; v < PS_CP_NV; ++v) {
                    double wsum = 0.0;
#pragma unroll
                    for (int m = 0; m < 2; ++m) if (m < en[v]) PS_CP_TAKE(ga[v][m], gb[v][m]);
                    if (en[v] > 2) {                                 // a long row
                        int m0 = 2;
                        if (v == lv) {
#pragma unroll
                            for (int j = 0; j < PS_CP_LONG; ++j) if (2 + j < len) PS_CP_TAKE(xa[j], xb[j]);
                            m0 = 2 + PS_CP_LONG;
                        }
                        for (; m0 < en[v]; m0 += PS_CP_LONG) {
                            ps_u64 ya[PS_CP_LONG], yb[PS_CP_LONG];
#pragma unroll
                            for (int j = 0; j < PS_CP_LONG; ++j) {
                                ya[j] = yb[j] = 0;
                                if (m0 + j < en[v]) {
                                    ya[j] = cp_get(buf, 16u * (unsigned)(e0[v] + m0 * D) + 16u * (j * D));
                                    yb[j] = cp_get(buf, 16u * (unsigned)(e0[v] + m0 * D) + 16u * (j * D) + 8u);
                                }
                            }
#pragma unroll
                            for (int j = 0; j < PS_CP_LONG; ++j) if (m0 + j < en[v]) PS_CP_TAKE(ya[j], yb[j]);
                        }
                    }
                    vw[v] = wsum;
                }
#undef PS_CP_TAKE
                ok = __all(ok);
                if (!ok) {
                    if (spins > spin_limit || (long long)wall_clock64() - t_enter > PS_PERSIST_TIMEOUT_TICKS) { bad = 1; break; }
                    if (PS_CP_SLEEP) __builtin_amdgcn_s_sleep(PS_CP_SLEEP);
                    ck[7] += 1;
                }
            }
        }
        PS_CP_CLK(3);
        // ---- gamma = r.r, delta = w.r over all entries, by every workgroup in the same order
        double ds = 0.0;
#pragma unroll
        for (int v = 0; v < PS_CP_NV; ++v) ds += vw[v] * vr[v];
        ds = wave_sum(ds);
        if (lane == 0) rd[1][wv] = ds;
        __syncthreads();
        PS_CP_CLK(5);
        if (bad) {                                           // an exchange timed out: a breakdown the host answers with the other kernels
            if (t == 0) { atomicMax(&status[ST_PCG_DONE], 2); status[ST_PERSIST_FAIL] = 1; }
            break;
        }
        gamma = gamma_next; delta = 0.0;
#pragma unroll
        for (int w2 = 0; w2 < PS_CP_NT / 64; ++w2) delta += rd[1][w2];
    }
#undef PS_CP_CLK
    const long long t_left = dbg ? wall_clock64() : 0;       // (ck[4]: from here to the last store of rec.x)
    // ---- the recovery of k_coarse_recover, on x^ as this workgroup holds it (every workgroup holds the same bits): y for the
    // columns of the slice's nodes, then the slice's entries, all operands from LDS; the arithmetic is k_coarse_recover's own
    // (coarse_recover_ylane / coarse_recover_entry, ps_k_cg_fused.h), sum for sum.  A workgroup whose exchange timed out is not
    // here (converged is false): ST_PCG_DONE is then 2 whoever wrote last (atomicMax), and nothing downstream applies x.
    if (converged && rec.x) {
        __syncthreads();                                     // (every wave has left the loop: rn is free)
#pragma unroll
        for (int v = 0; v < PS_CP_NV; ++v) { const int i = t + v * PS_CP_NT; if (i < n) rn[i] = vx[v]; }
        __syncthreads();
        const int nc = rec.ncb * D, p0 = blockIdx.x * rec.pp, np = max(0, min(rec.nr, p0 + rec.pp) - p0);
        if (np > 0) {                                        // (np, ncols, qa are the same in every thread of the workgroup)
            const double* sLc = cp_rec;                      // maxcols x nc
            const double* sOp = sLc + rec.maxcols * nc;      // B | Linv | pw0 | pw1 of np poses
            double* sy = cp_rec + rec.maxcols * nc + rec.pp * (2 * DD + 2);    // maxcols: y of the slice's columns
            const int32_t* spn = reinterpret_cast<const int32_t*>(sy + rec.maxcols);   // pp: pnode of the slice; then qa, ncols
            const int qa = spn[rec.pp], ncols = spn[rec.pp + 1];
            const double* xc = rn + rec.nr * D;
            for (int base = 0; base < ncols; base += PS_CP_NT / 8) {
                const int j = base + t / 8, sub = t & 7;
                double v = 0.0;
                if (j < ncols) v = coarse_recover_ylane(sLc + j * nc, 1, xc, qa * D + j, sub, nc);
                v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
                if (j < ncols && sub == 0) sy[j] = v;
            }
            __syncthreads();
            const double *sB = sOp, *sLi = sOp + np * DD, *sw0 = sOp + 2 * np * DD, *sw1 = sw0 + np;
            for (int e = t; e < np * D; e += PS_CP_NT) {
                const int il = e / D, c = e - il * D, q = spn[il];
                // (a node beyond the slice's columns cannot be: the columns span pnode[first] .. pnode[last] + 1, pnode ascending)
                rec.x[(size_t)p0 * D + e] = coarse_recover_entry<D>(sy + (q - qa) * D, (q + 1 < rec.ncb) ? sy + (q + 1 - qa) * D : nullptr,
                                                                    sw0[il], sw1[il], rn + (p0 + il) * D, sB + il * DD, sLi + il * DD, c);
            }
        }
    }
    // ---- what a caller that looks at the state finds: written by the first workgroup
    if (blockIdx.x == 0) {
        if (dbg) {                                           // (measurement build; dbg is the same in every thread)
            __syncthreads();
            if (t == 0) {
                ck[4] = wall_clock64() - t_left;
                for (int i = 0; i < 8; ++i) dbg[i] += ck[i];
            }
        }
#pragma unroll
        for (int v = 0; v < PS_CP_NV; ++v) {
            const int i = t + v * PS_CP_NT;
            if (i < n) { x_io[i] = vx[v]; p_io[i] = vp[v]; }
        }
    }
}
