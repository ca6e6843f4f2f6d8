// ps_host_structure.h -- ps_problem_create's host work on std::vectors: the HOST builders of the observation tables and of the
// Schur pair list (the test oracle of the device build in ps_host_build.h, and what small problems, wide observation groups and
// the PS_SCHUR_TILE_KB / PS_PAIRS_BY_LANDMARK variants use), and the stages that turn tasks and the block pattern
// (ps_structure.h) into the kernels' work lists: pair items, per-XCD lists, combine lists, factor contribution lists, the
// zero-slot list.  Part of ps_core.hip (one translation unit; included from there, in this order).
#pragma once

namespace {

struct PairRec { uint64_t key; int32_t a, b, tile; };

// ---- observation tables, host builder.  Every table of the handle is staged in the arena in the order the stages ask for it.
struct HostPairBuild;
struct HostObsBuild : ObsBuilder {
    ps_problem* h;
    const ps_problem_desc* d;                   // with HOST observation columns (DescStage::pull_obs)
    // what the host pair builder and the packed-run stage read afterwards
    std::vector<LObs> lobs;                     // observations in landmark order: variable points (by slot) first, then constant
    std::vector<int32_t> lm_ptr, pidx, point_slot;
    // staged for their upload only
    std::vector<int32_t> lm_point, sidx_l, sidx_p;
    std::vector<LObs> pobs;
    HostObsBuild(ps_problem* h_, const ps_problem_desc* d_) : h(h_), d(d_) {}

    // Internal landmark order ("slots"): by the lowest pose index that observes the landmark, so the
    // Z rows a pose (and a reduced-system block row) touches come from a compact address range and
    // stay in the 4 MB per-XCD L2, whatever order the caller numbered the landmarks in.
    int slots(const std::vector<int32_t>& point_of_vid) override {
        const int P = h->P, L = h->L, nv = h->nv;
        const long N = h->N;
        std::vector<int32_t> first_pose(L, INT32_MAX);
        {
            const int T = ps_host_threads(N, 8);
            std::vector<std::vector<int32_t>> fp(T > 1 ? T : 0);
            ps_parallel(T, [&](int t, int TT) {
                std::vector<int32_t>& mine = TT > 1 ? fp[t] : first_pose;
                if (TT > 1) mine.assign(L, INT32_MAX);
                for (long i = N * t / TT, e = N * (t + 1) / TT; i < e; ++i) {
                    const int pt = d->obs_point[i];
                    if (pt >= 0 && pt < L) mine[pt] = std::min(mine[pt], d->obs_pose[i]);
                }
            });
            for (auto& v2 : fp) for (int i = 0; i < L; ++i) first_pose[i] = std::min(first_pose[i], v2[i]);
        }
        std::vector<int32_t>& vid_of_slot = h->h_vid_of_slot;
        vid_of_slot.resize(nv);
        {   // vids in ascending first pose, ties in vid order (what the stable sort over 500 000 landmarks gave: 40 ms at C4)
            std::vector<int32_t> fkey(nv), cnts;
            for (int v = 0; v < nv; ++v) { const int32_t f = first_pose[point_of_vid[v]]; fkey[v] = (f < 0 || f >= P) ? P : f; }
            parallel_index_sort(nv, (size_t)P + 1, fkey.data(), vid_of_slot.data(), cnts);
        }
        lm_point.resize(nv); point_slot.assign(L, -1);
        for (int s2 = 0; s2 < nv; ++s2) { lm_point[s2] = point_of_vid[vid_of_slot[s2]]; point_slot[lm_point[s2]] = s2; }
        return h->upload(&h->point_vid, point_slot);     // device-side 'vid' = internal slot
    }

    int landmark_order(const std::vector<int32_t>&, const std::vector<int32_t>& class_of_row) override {
        const int P = h->P, L = h->L, nv = h->nv;
        const long N = h->N;
        const bool wide = h->wide_obs;
        std::vector<int32_t> order((size_t)N), lkey((size_t)N), lcounts;
        {   // keys (and the range checks the fill below relies on) on several threads
            std::atomic<int> bad{0};
            ps_parallel(ps_host_threads(N), [&](int t, int TT) {
                for (long i = N * t / TT, e = N * (t + 1) / TT; i < e; ++i) {
                    const int pose = d->obs_pose[i], pt = d->obs_point[i], grp = d->obs_grp[i];
                    if (pose < 0 || pose >= P || pt < 0 || pt >= L || grp < 0 || grp >= d->num_obs_groups) { bad = 1; lkey[i] = 0; continue; }
                    const int v = point_slot[pt];
                    lkey[i] = v >= 0 ? v : nv + pt;
                }
            });
            if (bad) return fail("observation index out of range");
        }
        parallel_index_sort(N, (size_t)nv + (size_t)L + 1, lkey.data(), order.data(), lcounts);
        lobs.resize((size_t)N);
        std::vector<int32_t> lorig((size_t)N);
        lm_ptr.assign(nv + 1, 0); sidx_l.resize(wide ? N : 0);
        for (int v = 0; v < nv; ++v) { lm_ptr[v + 1] = lcounts[v]; Nl += lcounts[v]; }
        ps_parallel(ps_host_threads(N), [&](int t, int TT) {
            for (long k = N * t / TT, e = N * (t + 1) / TT; k < e; ++k) {
                const long i = order[k];
                const int pose = d->obs_pose[i], pt = d->obs_point[i], grp = d->obs_grp[i];
                LObs& o = lobs[k];
                o.u = d->obs_uvd[3 * i]; o.v = d->obs_uvd[3 * i + 1]; o.d = d->obs_uvd[3 * i + 2];
                o.pose_grp = (int32_t)((uint32_t)pose | ((uint32_t)class_of_row[grp] << 24));
                o.point = pt;
                lorig[k] = (int32_t)i;
                if (wide) sidx_l[k] = (int32_t)d->obs_groups[4 * (size_t)grp + 1];
            }
        });
        for (int v = 0; v < nv; ++v) lm_ptr[v + 1] += lm_ptr[v];
        if (h->upload(&h->lobs, lobs) || h->upload(&h->lorig, lorig) || h->upload(&h->lm_ptr, lm_ptr) ||
            h->upload(&h->lm_point, lm_point) || (wide && h->upload(&h->sidx_l, sidx_l))) return -1;
        return 0;
    }

    // observations by reduced pose (constant poses: key nr, cut off afterwards), stable in landmark order; the pose-sorted copy
    // of the observation records, whose pose bits (uniform per chunk) carry the landmark slot + 1
    int pose_order() override {
        const int nr = h->nr;
        const long N = h->N;
        pcount.assign(nr + 1, 0);
        {
            std::vector<int32_t> pkey((size_t)N), pord((size_t)N), pcnt;
            ps_parallel(ps_host_threads(N), [&](int t, int TT) {
                for (long k = N * t / TT, e = N * (t + 1) / TT; k < e; ++k) { const int r = d->pose_rid[PS_POSE_OF(lobs[k])]; pkey[k] = r >= 0 ? r : nr; }
            });
            parallel_index_sort(N, (size_t)nr + 1, pkey.data(), pord.data(), pcnt);
            for (int r = 0; r < nr; ++r) pcount[r + 1] = pcount[r] + pcnt[r];
            pord.resize((size_t)pcount[nr]);
            pidx.swap(pord);
        }
        Np = pcount[nr];
        pobs.resize((size_t)Np);
        const long np = Np;
        ps_parallel(ps_host_threads(np), [&](int t, int TT) {
            for (long k = np * t / TT, e = np * (t + 1) / TT; k < e; ++k) {
                pobs[k] = lobs[pidx[k]];
                const int slot = point_slot[pobs[k].point];          // -1: constant point
                pobs[k].pose_grp = (int32_t)(((uint32_t)PS_GRP_OF(pobs[k]) << 24) | (uint32_t)(slot + 1));
            }
        });
        return 0;
    }
    int place_sidx_p() override {
        if (!h->wide_obs) return 0;
        sidx_p.resize((size_t)Np);
        for (long k = 0; k < Np; ++k) sidx_p[k] = sidx_l[pidx[k]];
        return h->upload(&h->sidx_p, sidx_p);
    }
    int place_pobs() override { return h->upload(&h->pobs, pobs); }
    std::unique_ptr<PairBuilder> pair_builder() override;
    int landmark_extent(int* most, int* fewest) override {
        int mx = 0, mn = INT_MAX;
        for (int v = 0; v < h->nv; ++v) { const int n = lm_ptr[v + 1] - lm_ptr[v]; mx = std::max(mx, n); mn = std::min(mn, n); }
        *most = mx; *fewest = mn;
        return 0;
    }
    int place_run_starts(int W, int nw) override {
        const int nv = h->nv;
        std::vector<int32_t> first((size_t)nw + 1, nv);
        for (int w = 0, v = 0; w < nw; ++w) { while (v < nv && lm_ptr[v] < W * w) ++v; first[w] = v; }
        std::vector<LmwRun> run((size_t)nw);
        for (int w = 0; w < nw; ++w) run[w] = LmwRun{first[w], first[w + 1], lm_ptr[first[w]], lm_ptr[first[w + 1]] - lm_ptr[first[w]]};
        return (h->upload(&h->lmw_first, first) || h->upload(&h->lmw_run, run)) ? -1 : 0;
    }
};

// ---- Schur pairs per landmark (upper-triangle block keys), host builder
struct HostPairBuild : PairBuilder {
    ps_problem* h;
    const int32_t* pose_rid;
    const HostObsBuild& o;
    const int nv, nr;
    const bool by_pose;
    std::vector<long> lm_pairs_before;
    std::vector<PairRec> prs;                   // the last build
    std::vector<int2> pairs;                    // the kernels' form of it (tasks())
    HostPairBuild(ps_problem* h_, const int32_t* pose_rid_, const HostObsBuild& o_)
        : h(h_), pose_rid(pose_rid_), o(o_), nv(h_->nv), nr(h_->nr), by_pose(h_->nr > 0 && !ps_create_env("PS_PAIRS_BY_LANDMARK")) {}
    int max_tiles() const override { return INT_MAX; }
    int prepare() override {
        lm_pairs_before.assign(nv + 1, 0);
        for (int v = 0; v < nv; ++v) {
            long nvar = 0;
            for (int a = o.lm_ptr[v]; a < o.lm_ptr[v + 1]; ++a) nvar += pose_rid[PS_POSE_OF(o.lobs[a])] >= 0;
            lm_pairs_before[v + 1] = lm_pairs_before[v] + nvar * (nvar - 1) / 2;
        }
        total = lm_pairs_before[nv];
        return 0;
    }
    // One tile (the untiled list: C3): pose by pose on several host threads.  The pairs of pose r -- its rows a in landmark
    // order against the rows b of the same landmark whose pose comes later (or the same pose again, b > a: a diagonal block)
    // -- sorted by partner (stable) ARE the (block row, block column, landmark) order the two counting passes over the whole
    // list produce, so the threads' outputs are simply concatenated (C3: 70 ms -> 7 ms of ps_problem_create).
    void build_untiled_by_pose() {
        const std::vector<int32_t>& lm_ptr = o.lm_ptr;
        std::vector<int32_t> rid_row((size_t)lm_ptr[nv]), lm_row((size_t)lm_ptr[nv]);
        for (int v = 0; v < nv; ++v)
            for (int a = lm_ptr[v]; a < lm_ptr[v + 1]; ++a) { lm_row[a] = v; rid_row[a] = pose_rid[PS_POSE_OF(o.lobs[a])]; }
        const long nrows = lm_ptr[nv];
        const int nth = std::max(1, std::min({(int)std::thread::hardware_concurrency(), 16, nr}));
        std::vector<std::vector<PairRec>> outs(nth);
        auto work = [&](int th) {
            std::vector<PairRec>& out = outs[th];
            const int r0 = (int)((long)nr * th / nth), r1 = (int)((long)nr * (th + 1) / nth);
            std::vector<PairRec> tri;
            std::vector<int32_t> cnt((size_t)nr + 1, 0), touched;
            for (int r = r0; r < r1; ++r) {
                tri.clear();
                for (int s0 = o.pcount[r]; s0 < o.pcount[r + 1]; ++s0) {
                    const int k = o.pidx[s0];
                    if (k >= nrows) continue;                // an observation of a constant point: no Z row
                    const int v = lm_row[k];
                    for (int b = lm_ptr[v]; b < lm_ptr[v + 1]; ++b) {
                        const int rb = rid_row[b];
                        if (rb > r || (rb == r && b > k)) tri.push_back({((uint64_t)r << 32) | (uint32_t)rb, k, b, 0});
                    }
                }
                touched.clear();
                for (const PairRec& t : tri) { if (cnt[(uint32_t)t.key]++ == 0) touched.push_back((int32_t)(uint32_t)t.key); }
                std::sort(touched.begin(), touched.end());
                int32_t run = 0;
                for (int32_t rb : touched) { const int32_t c = cnt[rb]; cnt[rb] = run; run += c; }
                const size_t base = out.size();
                out.resize(base + tri.size());
                for (const PairRec& t : tri) out[base + cnt[(uint32_t)t.key]++] = t;
                for (int32_t rb : touched) cnt[rb] = 0;
            }
        };
        if (nth == 1) work(0);
        else {
            std::vector<std::thread> pool;
            for (int th = 0; th < nth; ++th) pool.emplace_back(work, th);
            for (auto& t : pool) t.join();
        }
        size_t at = 0;
        for (auto& out : outs) { std::copy(out.begin(), out.end(), prs.begin() + at); at += out.size(); }
        prs.resize(at);
    }
    // one unit of work per tile: the tile's pairs in (block row, block column, landmark) order, written to its
    // slice of prs; tiles are independent, so they are built by a few host threads
    void build_tiles(int ntiles) {
        const std::vector<int32_t>& lm_ptr = o.lm_ptr;
        auto tile_of = [&](int v) {
            return (ntiles > 1 && total > 0)
                ? (int)std::min<long>(ntiles - 1, (long)((double)ntiles * (double)lm_pairs_before[v] / (double)total)) : 0;
        };
        std::vector<int> tile_begin(ntiles + 1, nv);
        {
            int t_prev = -1;
            for (int v = 0; v < nv; ++v) {
                const int t = tile_of(v);
                for (int q = t_prev + 1; q <= t; ++q) tile_begin[q] = v;
                t_prev = std::max(t_prev, t);
            }
            tile_begin[ntiles] = nv;
            for (int q = ntiles - 1; q >= 0; --q) tile_begin[q] = std::min(tile_begin[q], tile_begin[q + 1]);
        }
        auto build_tile = [&](int tile) {
            const int v0 = tile_begin[tile], v1 = tile_begin[tile + 1];
            std::vector<PairRec> loc;
            loc.reserve((size_t)(lm_pairs_before[v1] - lm_pairs_before[v0]));
            for (int v = v0; v < v1; ++v)
                for (int a = lm_ptr[v]; a < lm_ptr[v + 1]; ++a) {
                    const int ra = pose_rid[PS_POSE_OF(o.lobs[a])];
                    if (ra < 0) continue;
                    for (int b = a + 1; b < lm_ptr[v + 1]; ++b) {
                        const int rb = pose_rid[PS_POSE_OF(o.lobs[b])];
                        if (rb < 0) continue;
                        if (ra <= rb) loc.push_back({((uint64_t)ra << 32) | (uint32_t)rb, a, b, tile});
                        else loc.push_back({((uint64_t)rb << 32) | (uint32_t)ra, b, a, tile});
                    }
                }
            // (block row, block column): two stable counting passes, least significant first
            counting_sort(loc, (size_t)std::max(nr, 1), [](const PairRec& x) { return (uint32_t)x.key; });
            counting_sort(loc, (size_t)std::max(nr, 1), [](const PairRec& x) { return (uint32_t)(x.key >> 32); });
            std::copy(loc.begin(), loc.end(), prs.begin() + lm_pairs_before[v0]);
        };
        const int nthreads = std::max(1, std::min({ntiles, 16, (int)std::thread::hardware_concurrency()}));
        if (nthreads <= 1) {
            for (int t = 0; t < ntiles; ++t) build_tile(t);
        } else {
            std::atomic<int> next{0};
            std::vector<std::thread> pool;
            for (int k = 0; k < nthreads; ++k)
                pool.emplace_back([&] { for (int t = next++; t < ntiles; t = next++) build_tile(t); });
            for (auto& th : pool) th.join();
        }
    }
    int build(int ntiles) override {
        prs.resize((size_t)total);
        if (ntiles == 1 && by_pose) build_untiled_by_pose();
        else build_tiles(ntiles);
        return 0;
    }
    PairListCounts counts() override {
        if (prs.empty() || prs.back().tile == 0) {          // one tile: a task per block, no key twice
            size_t nblocks = 0;
            for (size_t k = 0; k < prs.size(); ++k) nblocks += (k == 0 || prs[k].key != prs[k - 1].key);
            return {prs.size(), nblocks, nblocks};
        }
        std::vector<uint64_t> task_keys;
        for (size_t k = 0; k < prs.size(); ++k)
            if (k == 0 || prs[k].key != prs[k - 1].key || prs[k].tile != prs[k - 1].tile) task_keys.push_back(prs[k].key);
        const size_t ntask = task_keys.size();
        std::sort(task_keys.begin(), task_keys.end());
        return {prs.size(), ntask, (size_t)(std::unique(task_keys.begin(), task_keys.end()) - task_keys.begin())};
    }
    // the runs of equal (tile, block) are found (and the records copied into the kernels' int2 form) on several threads
    int tasks(PairTasks& out) override {
        pairs.resize(prs.size());
        const long np = (long)prs.size();
        const int T = ps_host_threads(np);
        std::vector<std::vector<int32_t>> starts(T);
        ps_parallel(T, [&](int t, int TT) {
            for (long k = np * t / TT, e = np * (t + 1) / TT; k < e; ++k) {
                pairs[k] = make_int2(prs[k].a, prs[k].b);
                if (k == 0 || prs[k].key != prs[k - 1].key || prs[k].tile != prs[k - 1].tile) starts[t].push_back((int32_t)k);
            }
        });
        size_t ntask = 0;
        for (auto& v2 : starts) ntask += v2.size();
        out.start.reserve(ntask); out.tile.reserve(ntask); out.key.reserve(ntask);
        for (auto& v2 : starts)
            for (int32_t k : v2) { out.start.push_back(k); out.tile.push_back(prs[k].tile); out.key.push_back(prs[k].key); }
        prs.clear(); prs.shrink_to_fit();
        return 0;
    }
    int place_pairs() override { return h->upload(&h->pairs, pairs); }
};
std::unique_ptr<PairBuilder> HostObsBuild::pair_builder() { return std::unique_ptr<PairBuilder>(new HostPairBuild(h, d->pose_rid, *this)); }

// ---- pair items: one work item (task) per (tile, block) that has pairs; per-XCD work lists; combine lists of a tiled list
int build_pair_items(ps_problem* h, const PairTasks& tk, const BlockPattern& pat, std::vector<PairItem>& pitm) {
    const long npairs_l = h->npairs;
    pitm.resize(tk.start.size());
    {
        const long nt = (long)pitm.size();
        std::atomic<int> diag{0};
        ps_parallel(ps_host_threads(nt * 16), [&](int t, int TT) {
            for (long q = nt * t / TT, e = nt * (t + 1) / TT; q < e; ++q) {
                const uint64_t key = tk.key[q];
                const int a = (int)(key >> 32), b = (int)(uint32_t)key;
                pitm[q] = {pat.slot_of(a, b), pat.slot_of(b, a), tk.start[q], q + 1 < nt ? tk.start[q + 1] : (int32_t)npairs_l};
                if (a == b) diag = 1;
            }
        });
        if (diag) h->has_diag_tasks = true;
    }
    h->npair_items = (int)pitm.size();
    return 0;
}

int build_xcd_lists(ps_problem* h, const PairTasks& tk, const std::vector<PairItem>& pitm) {
    const std::vector<int32_t>& task_tile = tk.tile;
    const int ntiles = h->schur_tiles;
    // per-XCD work lists.  Untiled: items are sorted by block row, so equal contiguous shares of
    // the PAIRS (not of the items) give each XCD a contiguous range of block rows with balanced
    // work.  Tiled: XCD x takes tiles x, x + 8, ... (tiles hold equal pair counts).
    std::vector<std::vector<int32_t>> lists(8);
    const double total = (double)h->npairs;
    for (size_t k = 0; k < pitm.size(); ++k) {
        const int x = ntiles > 1 ? (task_tile[k] & 7)
                                 : (total > 0 ? std::min(7, (int)(8.0 * pitm[k].start / total)) : 0);
        lists[x].push_back((int32_t)k);
    }
    // longest tasks first (within each tile): the short ones fill the tail of the XCD's schedule
    if (!ps_env("PS_SCHUR_NO_LPT"))
        for (auto& l : lists)
            std::stable_sort(l.begin(), l.end(), [&](int32_t x, int32_t y) {
                if (task_tile[x] != task_tile[y]) return task_tile[x] < task_tile[y];
                return pitm[x].end - pitm[x].start > pitm[y].end - pitm[y].start; });
    size_t mx = 0;
    for (auto& l : lists) mx = std::max(mx, l.size());
    mx = std::max<size_t>((mx + 3) / 4 * 4, 4);
    std::vector<PairItem> xit(8 * mx, PairItem{-1, -1, 0, 0});
    std::vector<int32_t> pos_of_task(pitm.size(), -1);
    for (int x = 0; x < 8; ++x)
        for (size_t q = 0; q < lists[x].size(); ++q) {
            xit[x * mx + q] = pitm[lists[x][q]];
            pos_of_task[lists[x][q]] = (int32_t)(x * mx + q);
        }
    h->pair_per_xcd = (int)mx;
    if (h->upload(&h->pair_xitems, xit)) return -1;
    if (ntiles > 1 && !pitm.empty()) {
        // per-block task lists in tile order (tasks are numbered tile-major); partials are
        // addressed by dispatch position
        std::vector<std::pair<int32_t, int32_t>> bt(pitm.size());      // (slot, task)
        for (size_t k = 0; k < pitm.size(); ++k) bt[k] = {pitm[k].slot, (int32_t)k};
        std::stable_sort(bt.begin(), bt.end(), [](const std::pair<int32_t, int32_t>& x, const std::pair<int32_t, int32_t>& y) {
            return x.first < y.first; });
        std::vector<PairItem> citm;
        std::vector<int32_t> ctasks(bt.size());
        for (size_t k = 0; k < bt.size(); ++k) {
            ctasks[k] = pos_of_task[bt[k].second];
            if (k == 0 || bt[k].first != bt[k - 1].first) {
                if (!citm.empty()) citm.back().end = (int32_t)k;
                citm.push_back({pitm[bt[k].second].slot, pitm[bt[k].second].slotT, (int32_t)k, 0});
            }
        }
        citm.back().end = (int32_t)bt.size();
        h->ncomb = (int)citm.size();
        if (h->upload(&h->comb_items, citm) || h->upload(&h->comb_tasks, ctasks)) return -1;
        if (h->alloc(&h->Spart, xit.size() * 36)) return -1;
    }
    return 0;
}

// ---- pose factors (edges, then priors, then the caller's host rows): where each contributes in S and g
struct FactorTables {
    std::vector<int32_t> f_i, f_j;              // first pose (-1: a prior) and second pose of factor f < F
    long E = 0, F = 0, FH = 0;
    const ps_host_rows_desc* hrows = nullptr;   // pose pairs of the caller's blocks, numbered F, F + 1, ...
    int i(long f) const { return f < F ? f_i[f] : hrows->i[f - F]; }
    int j(long f) const { return f < F ? f_j[f] : hrows->j[f - F]; }
};

int build_factor_lists(ps_problem* h, const int32_t* pose_rid, const FactorTables& fac, const BlockPattern& pat, std::vector<int32_t>& eslots) {
    const int nr = h->nr, D = h->D, DD = D * D, FROW = 3 * DD + 2 * D;
    struct C { int32_t slot, off, tr; };
    std::vector<C> cs;
    std::vector<std::vector<int32_t>> gl(nr);
    for (long f = 0; f < fac.F + fac.FH; ++f) {
        const int ra = fac.i(f) >= 0 ? pose_rid[fac.i(f)] : -1, rb = pose_rid[fac.j(f)];
        const int32_t base = (int32_t)(f * FROW);
        if ((size_t)f * FROW >= (1UL << 31)) return fail("too many pose factors for 32-bit scratch offsets");
        if (ra >= 0) { cs.push_back({pat.diag_slot[ra], base, 0}); gl[ra].push_back(base + 3 * DD); }
        if (rb >= 0) { cs.push_back({pat.diag_slot[rb], base + 2 * DD, 0}); gl[rb].push_back(base + 3 * DD + D); }
        if (ra >= 0 && rb >= 0) {
            if (ra == rb) return fail("pose-pose edge connects a pose with itself");
            cs.push_back({pat.slot_of(ra, rb), base + DD, 0});
            cs.push_back({pat.slot_of(rb, ra), base + DD, 1});
        }
    }
    std::stable_sort(cs.begin(), cs.end(), [](const C& x, const C& y) { return x.slot < y.slot; });
    std::vector<int32_t> eptr, ediag, gptr(nr + 1, 0), gitems;
    std::vector<int2> eitems(cs.size());
    for (size_t k = 0; k < cs.size(); ++k) {
        eitems[k] = make_int2(cs[k].off, cs[k].tr);
        if (k == 0 || cs[k].slot != cs[k - 1].slot) { eslots.push_back(cs[k].slot); eptr.push_back((int32_t)k); }
    }
    eptr.push_back((int32_t)cs.size());
    for (int32_t s : eslots) {
        // diagonal iff the slot is some row's diag slot: find its row by binary search on row_ptr
        const int row = (int)(std::upper_bound(pat.row_ptr.begin(), pat.row_ptr.end(), s) - pat.row_ptr.begin()) - 1;
        ediag.push_back(pat.col_idx[s] == row ? 1 : 0);
    }
    for (int r = 0; r < nr; ++r) { gptr[r + 1] = gptr[r] + (int32_t)gl[r].size(); gitems.insert(gitems.end(), gl[r].begin(), gl[r].end()); }
    h->nes = (int)eslots.size();
    if (h->upload(&h->eslots, eslots) || h->upload(&h->eptr, eptr) || h->upload(&h->eslot_diag, ediag) ||
        h->upload(&h->eitems, eitems) || h->upload(&h->gptr, gptr) || h->upload(&h->gitems, gitems)) return -1;
    return 0;
}

// ---- the slots of S a linearisation accumulates into (option "lin_zero_list"), from the structure alone: an
// off-diagonal slot that exactly ONE pair item of the untiled list writes is stored with `=` (k_schur_pairs_db); a
// diagonal slot, a slot a factor or a host row adds into, a slot no pair item writes (an extra pattern block, a block
// that exists through a factor only) and a slot with more than one writer are accumulated and must start at zero
int build_zero_slots(ps_problem* h, const BlockPattern& pat, const std::vector<PairItem>& pitm, const std::vector<int32_t>& eslots) {
    const int nnzb = h->nnzb;
    if (!(h->D == 6 && h->schur_tiles == 1 && nnzb > 0)) return 0;
    std::vector<uint8_t> writers((size_t)nnzb, 0);     // pair items that write the slot, saturating at 2
    for (const PairItem& it : pitm) {
        if (it.slot >= 0 && writers[it.slot] < 2) ++writers[it.slot];
        if (it.slotT >= 0 && it.slotT != it.slot && writers[it.slotT] < 2) ++writers[it.slotT];
    }
    for (int32_t s : eslots) if (s >= 0) writers[s] = 2;
    for (int r = 0; r < h->nr; ++r) writers[pat.diag_slot[r]] = 2;
    std::vector<int32_t> zl;
    for (int b = 0; b < nnzb; ++b) if (writers[b] != 1) zl.push_back(b);
    h->nzero_slots = (int)zl.size();
    if (!zl.empty() && h->upload(&h->zero_slots, zl)) return -1;
    return 0;
}

}  // namespace
