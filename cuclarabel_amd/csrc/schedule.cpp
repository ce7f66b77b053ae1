// The numeric engine's decisions (schedule.hpp): plain host code, compiled without HIP -- the host sanitizer driver
// (tests/sanitize/host_driver.cpp) builds it with g++ and checks what it decides on a machine without a GPU.
#include "schedule.hpp"

#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <unordered_map>

namespace hipkkt {

// too tall for the LDS of the block sweep kernels / of k_top_solve (solve_kernels.hip, k_fwd_tall)
// (HIPKKT_SOLVE_TALL_ROWS=n: fronts of n rows or more count as tall as well -- the tests' way to those paths)
static bool front_is_tall(const Symbolic& S, int s)
{
    const int tall_rows = knobs().solve_tall_rows;
    const int f = front_size(S, s), nc = S.sn_start[s + 1] - S.sn_start[s];
    return solve_lds_bytes(f, nc) > kLdsCap || (tall_rows > 0 && f >= tall_rows);
}

// the launches: every tree level's fronts by size class, with the shapes their kernels are launched with
static void form_launches(const Symbolic& S, const DeviceLimits& dev, int64_t panel_cap, int panel_max_slices, Schedule& sch)
{
    sch.tile_base.assign(S.nsuper, -1);
    auto ncols = [&](int s) { return S.sn_start[s + 1] - S.sn_start[s]; };
    auto is_small = [&](int s) {
        int f = front_size(S, s), nc = ncols(s), nb = f - nc;
        return f <= kSmallFrontMax && f * nc + nb * nb <= kSmallSliceMax;
    };
    int level_no = -1;
    for (const Level& lv : S.levels) {
        ++level_no;
        std::vector<int> small, big;
        for (int t = lv.begin; t < lv.end; ++t) {
            int s = S.level_sn[t];
            (is_small(s) ? small : big).push_back(s);
        }
        // a handful of one-wave fronts beside a block-class launch is not worth launches of its own (one in the
        // factorisation, two per solve, each ~5-45 us of pure latency): they ride with the block-class fronts
        const int merge_small = knobs().merge_small;
        if (!big.empty() && (int)small.size() <= merge_small) {
            big.insert(big.end(), small.begin(), small.end());
            small.clear();
        }
        const int slice_rows = knobs().slice_rows;
        const bool slice_fit = knobs().slice_fit;
        int level_slice_rows = slice_rows;
        auto slices_of = [&](int s) {        // row slices the panel kernel needs for this front (1: fits one CU)
            if (panel_cap <= 0) return 1;
            const int nc = ncols(s), nb = front_size(S, s) - nc;
            int r = panel_slices_needed(nc, nb, panel_cap, std::min(panel_max_slices, std::max(1, nb)));
            if (r == 0) throw std::runtime_error("panel does not fit LDS even in row slices (panel_cap too large?)");
            // More, shorter slices than LDS needs: a slice's block step is bound by its WORKER waves when it holds many
            // rows (250 rows x 90 columns: 75 trailing tiles per block on 12 waves = 4-5 us against the diagonal
            // chain's 3.7), and its assembly by what one CU can load; the price is one more redundant copy of the
            // diagonal block's factorisation per slice.  128 rows (0 = as few slices as LDS allows): cfg5's
            // factorisation 5.30 -> 5.06 ms, cfg3's 1.21 -> 1.23 (slices have K and item lists of their own, so the
            // per-slice overhead no longer grows with their number).
            // (the preference stops at 16 slices: beyond that only what LDS needs -- a 6289-row front in 49 slices of 128
            //  rows measured 44.9 ms per factorisation against 40.3 in 16)
            if (r > 1 && level_slice_rows > 0) r = std::max(r, std::min(std::min(panel_max_slices, 16), (nb + level_slice_rows - 1) / level_slice_rows));
            return r;
        };
        // One round of panel workgroups where possible: every slice needs a CU to itself, so a level with more slices
        // than CUs runs its panel kernel in two rounds (cfg3's second level: 99 fronts x 3 slices of 114 rows = 297
        // workgroups, 112 us; x 2 slices of 171 rows = 198 workgroups, one round).  Such a level takes the shortest
        // slices (>= the default 128 rows) that bring it down to the CU count, if LDS allows any.
        level_slice_rows = slice_rows;
        if (slice_fit && slice_rows > 0) {
            auto total = [&]() {
                int t = 0;
                bool any = false;
                for (int s : big) { const int r = slices_of(s); t += r; any = any || r > 1; }
                return any ? t : 0;
            };
            if (total() > dev.n_cus) {
                static const int cand[] = {144, 160, 176, 192, 224, 256, 320, 384, 512, 1 << 20};
                for (int c : cand) {
                    level_slice_rows = c;
                    if (total() <= dev.n_cus) break;
                }
                if (total() > dev.n_cus) level_slice_rows = slice_rows;
            }
        }
        auto work = [&](int s) { return (double)front_size(S, s) * front_size(S, s) * ncols(s); };
        auto by_work = [&](int a, int b) { double wa = work(a), wb = work(b); return wa != wb ? wa > wb : a < b; };
        std::sort(small.begin(), small.end(), by_work);
        std::sort(big.begin(), big.end(), by_work);
        // fronts factorised in row slices go to the end of the block-class launch (own panel kernel launch)
        std::stable_partition(big.begin(), big.end(), [&](int s) { return slices_of(s) == 1; });
        auto is_tall = [&](int s) { return front_is_tall(S, s); };
        std::stable_partition(big.begin(), big.end(), [&](int s) { return !is_tall(s); });
        // the tiny fronts (f <= 8) go to the end of the one-wave launch: the solves give them their own kernel
        std::stable_partition(small.begin(), small.end(), [&](int s) { return front_size(S, s) > 8; });
        const int ntiny_level = (int)std::count_if(small.begin(), small.end(), [&](int s) { return front_size(S, s) <= 8; });
        for (int cls = 0; cls < 2; ++cls) {
            const std::vector<int>& v = cls == 0 ? big : small;
            if (v.empty()) continue;
            Launch L{};
            L.begin = (int)sch.sched.size();
            L.count = (int)v.size();
            L.small = cls == 1;
            L.level = level_no;
            // (a level is a front's height above its leaves -- symbolic.cpp, step 9 -- so level 0 holds every childless front
            //  and nothing else: the many-column backward sweep starts the pulled leaves' kernel for level-0 launches only,
            //  launch_bwd_multi, and the engine flags childless fronts only)
            for (int s : v)
                if ((level_no == 0) != (S.child_ptr[s + 1] == S.child_ptr[s])) throw std::logic_error("level 0 must hold the childless fronts and only them");
            L.ntiny = cls == 1 ? ntiny_level : 0;
            int fmax = 0, slice = 0;
            for (int s : v) {
                int f = front_size(S, s), nc = ncols(s), nb = f - nc;
                fmax = std::max(fmax, f);
                if (!(cls == 1 && f <= 8)) slice = std::max(slice, f * nc + nb * nb);     // (tiny fronts: own kernel)
            }
            L.slice = (slice + 1) & ~1;
            int pmax = 0;                       // LDS doubles of the largest panel: a trapezoid (panel kernel)
            int64_t smax = 0;
            L.nsliced = 0;
            L.slice_begin = (int)sch.slice_list.size();
            // A launch that holds row-sliced fronts runs ALL its fronts through the sliced panel kernel, a whole front
            // as a front of one slice: two panel kernels one after the other (whole, then sliced) cost a level of
            // cfg5 30-57 us for the one to four whole fronts that sit beside its hundreds of slices.
            bool all_sliced = false;
            if (cls == 0) for (int s : v) all_sliced = all_sliced || slices_of(s) > 1;
            for (int s : v) {
                const int r = cls == 0 ? slices_of(s) : 1;
                const int nc = ncols(s), nb = front_size(S, s) - nc;
                if (r == 1 && !all_sliced) {
                    pmax = std::max(pmax, front_size(S, s) * nc - nc * (nc - 1) / 2);
                } else {
                    ++L.nsliced;
                    smax = std::max(smax, panel_slice_doubles(nc, nb, r));
                    for (int q = 0; q < r; ++q) sch.slice_list.push_back({s, q, r});
                }
            }
            L.slice_count = (int)sch.slice_list.size() - L.slice_begin;
            L.lds_sliced = L.nsliced ? panel_lds_bytes(0, (int)smax) : 0;
            L.nbk = kMaxNbk;
            // (swept on cfg2 after the tree got shorter and wider: 128 / 192 beat the earlier 96 / 128 by 2 %)
            L.bs_panel = fmax > 192 ? 1024 : (fmax > 128 ? 512 : 256);
            L.lds_panel = panel_lds_bytes(fmax, pmax);
            if (!L.small && L.lds_panel > kLdsCap)
                throw std::runtime_error("panel does not fit LDS (panel_cap too large?)");
            if (L.lds_sliced > kLdsCap) throw std::runtime_error("panel slice does not fit LDS (panel_cap too large?)");
            int ncmax = 0;
            for (int s : v) ncmax = std::max(ncmax, ncols(s));
            // (per front, then the maximum: the tallest front of a launch is a narrow panel and its widest a short one --
            //  sized from (fmax, ncmax) jointly, a level with a 7000-row panel beside a 96-column one asked for LDS
            //  nobody needs and the structure was refused as "too large")
            L.lds_solve = 0;
            L.ntall = 0;
            if (!L.small) for (int s : v) {
                if (is_tall(s)) { ++L.ntall; continue; }
                L.lds_solve = std::max(L.lds_solve, solve_lds_bytes(front_size(S, s), ncols(s)));
            }
            L.fmax = fmax;
            L.ncmax = ncmax;
            const int small_bs_count = knobs().bs128_count;
            const int small_bs_f = knobs().bs128_f;
            L.solve_bs = (L.count >= small_bs_count && fmax <= small_bs_f) ? 128 : 256;
            L.tinv_begin = (int)sch.tinv_list.size();
            L.tinv_ncmax = 1;
            if (!L.small) for (int s : v) {
                sch.tinv_list.push_back(s);
                L.tinv_ncmax = std::max(L.tinv_ncmax, ncols(s));
                sch.tinv_ncmax = std::max(sch.tinv_ncmax, ncols(s));
            }
            L.tinv_count = (int)sch.tinv_list.size() - L.tinv_begin;
            if (L.lds_solve > kLdsCap) throw std::runtime_error("front too large for the solve kernels");
            L.tile_begin = (int)sch.tiles.size();
            int64_t tile_cols = 0;
            if (!L.small) {
                for (int s : v) {
                    int nb = front_size(S, s) - ncols(s);
                    int nt = (nb + 63) / 64;
                    sch.tile_base[s] = (int64_t)sch.tiles.size();
                    tile_cols += (int64_t)ncols(s) * (nt * (nt + 1) / 2);
                    for (int ti = 0; ti < nt; ++ti)
                        for (int tj = 0; tj <= ti; ++tj) {
                            // int2 {x = s, y = ti<<16 | tj}, little endian in one int64
                            uint64_t lo = (uint32_t)s, hi = (uint32_t)((ti << 16) | tj);
                            sch.tiles.push_back((int64_t)(lo | (hi << 32)));
                        }
                }
            }
            L.ntiles = (int)sch.tiles.size() - L.tile_begin;
            L.tile_nc = L.ntiles > 0 ? (int)(tile_cols / L.ntiles) : 0;
            sch.launches.push_back(L);
            sch.sched.insert(sch.sched.end(), v.begin(), v.end());
        }
    }
    sch.spos.assign(S.nsuper, -1);
    for (size_t q = 0; q < sch.sched.size(); ++q) sch.spos[sch.sched[q]] = (int)q;
    sch.tinv_small_prefix.assign(sch.tinv_list.size() + 1, 0);      // (how many narrow supernodes a stretch of the list holds: launch_tinv)
    for (size_t k = 0; k < sch.tinv_list.size(); ++k) {
        const int s = sch.tinv_list[k];
        sch.tinv_small_prefix[k + 1] = sch.tinv_small_prefix[k] + (S.sn_start[s + 1] - S.sn_start[s] <= winv_small_nc() ? 1 : 0);
    }
}

// Overlap admission.  In overlap mode a level's PANEL workgroups (each needs a CU to itself: ~150 KB of LDS) run
// beside the level's TILE workgroups on the overlap stream (53 KB: they fit beside each other, but one of them
// on a CU is enough to keep a panel out) and the side stream's W formation.  Tiles wait for their panel's
// blocks and panels wait for their children's tiles, so forward progress needs every panel workgroup of a
// launch to be RESIDENT before a tile of that launch may wait for it.  That is enforced, not hoped for: the
// launch's tile kernel sits behind a gate (k_ov_gate) that opens when all its panel workgroups have started.
// Everything else on the device is work that ends by itself (the previous launch's tiles, whose panels are
// resident or done; the W formation, which waits for nothing), so the panel workgroups do get their CUs,
// provided there are enough CUs for all of them plus the gate's wave at once:
//     panel workgroups of the launch + 1 + margin <= CUs.
// Below that bound the width is a matter of speed only: wide launches were measured slower in the mode
// (panels that wait hold whole CUs the tiles could use), so the default admits launches of up to 120 panel
// workgroups; HIPKKT_OV_MAX_FRONTS moves that, never beyond the bound.  (The bounded waits remain for what
// this argument cannot see: another process, or another handle's kernels, on the same device.)
static void admit_overlap(const DeviceLimits& dev, Schedule& sch)
{
    sch.side_winv_blocks = knobs().winv_blocks > 0 ? knobs().winv_blocks : std::max(8, dev.n_cus * 3 / 8);
    constexpr int kOvMargin = 8;
    // (the environment override is per process, the default per handle: n_cus is this handle's device's)
    const int ov_max_env = knobs().ov_max_fronts;
    const int ov_max = std::min(ov_max_env > 0 ? ov_max_env : 120 * dev.n_cus / 256, dev.n_cus - 1 - kOvMargin);
    auto panel_wgs = [&](const Launch& L) { return L.count - L.nsliced + L.slice_count; };   // whole panels + row slices
    size_t first = sch.launches.size();
    while (first > 0) {
        const Launch& L = sch.launches[first - 1];
        if (L.small || panel_wgs(L) > ov_max) break;
        --first;
    }
    // Launches with thousands of tiles stay out of the mode, and with them the whole handle (the overlapped launches
    // are the schedule's tail): there the tiles ARE the level -- nothing to hide them behind -- and a tile of the mode
    // is the slower one (54 KB of LDS instead of 33: two workgroups per CU instead of four; operands and results
    // past the L2's write-back path).  Measured with the mode on / off, by the largest launch of the region:
    // 1080 tiles 6.25 / 6.45 ms, 1279 tiles 3.17 / 3.65, 1145 tiles 3.74 / 3.72 | 2310 tiles 18.6 / 17.6,
    // 2428 tiles 9.5 / 8.2, 4253 tiles 10.0 / 7.8, 13 041 tiles 54 / 27, cfg2 with 1 % long-range couplings
    // (24 000 tiles) 143 / 61 ms.  (cfg2's overlapped launches have at most 418 tiles, cfg5's 630.)
    const int ov_max_tiles = knobs().ov_max_tiles;
    bool heavy_tiles = false;
    for (size_t q = first; q < sch.launches.size(); ++q) heavy_tiles = heavy_tiles || sch.launches[q].ntiles > ov_max_tiles;
    sch.ov_first = (!heavy_tiles && sch.launches.size() - first >= 3) ? first : sch.launches.size();
    {
        // Runs of narrow launches whose panels share one kernel, found from the root downwards: all launches of a run
        // are of one kind (whole panels, or row slices -- a launch with sliced fronts runs all its fronts as slices),
        // a run has at most ov_merge_max workgroups in all (HIPKKT_OV_MERGE, 0 = off) and at least two launches, a
        // launch in a run has at most ov_merge_wide workgroups (HIPKKT_OV_MERGE_WIDE: the workgroups of a run hold
        // their CUs from the start of the run, which the tiles of a WIDE level below them would miss), and the first
        // overlapped launch is in none (its tiles are released by an event).
        const int ov_merge_max = knobs().ov_merge;
        const int ov_merge_wide = knobs().ov_merge_wide;
        const int ov_merge_groups = knobs().ov_merge_groups;
        sch.ov_groups.clear();
        sch.ov_group_of.assign(sch.launches.size(), -1);
        size_t m = sch.launches.size();
        const int cap = std::min(ov_merge_max, ov_max);
        while (m > sch.ov_first + 1 && (int)sch.ov_groups.size() < ov_merge_groups) {
            MergeGroup g{m, m, 0, 0, sch.launches[m - 1].nsliced > 0};
            // (the root's run takes launches of any width, as it always did; the runs below it narrow ones only)
            const int wide = sch.ov_groups.empty() ? cap : ov_merge_wide;
            while (g.first > sch.ov_first + 1 && !sch.launches[g.first - 1].small &&
                   (g.sliced ? sch.launches[g.first - 1].nsliced == sch.launches[g.first - 1].count : sch.launches[g.first - 1].nsliced == 0) &&
                   panel_wgs(sch.launches[g.first - 1]) <= wide && g.count + panel_wgs(sch.launches[g.first - 1]) <= cap) {
                const Launch& L = sch.launches[g.first - 1];
                g.count += panel_wgs(L);
                g.lds = std::max(g.lds, g.sliced ? L.lds_sliced : L.lds_panel);
                --g.first;
            }
            if (g.end - g.first < 2) break;
            sch.ov_groups.insert(sch.ov_groups.begin(), g);
            m = g.first;
        }
        for (size_t k = 0; k < sch.ov_groups.size(); ++k)
            for (size_t q = sch.ov_groups[k].first; q < sch.ov_groups[k].end; ++q) sch.ov_group_of[q] = (int)k;
    }
}

// late_launches: the longest suffix of block-class launches with <= kTopMaxFronts fronts in total -- the
// narrow top of the tree, whose W is formed behind the factorisation (enqueue_factor / wait_w)
static void pick_late(Schedule& sch)
{
    sch.late_launches = 0;
    int cnt = 0;
    for (size_t q = sch.launches.size(); q-- > 0;) {
        const Launch& L = sch.launches[q];
        if (L.small || cnt + L.count > kTopMaxFronts) break;
        cnt += L.count;
        ++sch.late_launches;
    }
    sch.late_count = cnt;
    if (sch.late_launches < 3) { sch.late_launches = 0; sch.late_count = 0; }
}

// persistent top: the longest suffix of block-class launches none of which holds more than 1.5 x as many
// fronts as the device keeps resident workgroups of the persistent kernel (a workgroup then has at most two
// fronts per level; k_top_solve walks its fronts in level order)
static void pick_top(const Symbolic& S, const DeviceLimits& dev, Schedule& sch)
{
    sch.top_launches = 0; sch.top_count = 0; sch.top_lds = 0; sch.top_grid = 0;
    {
        size_t lds = 0;
        for (size_t q = sch.launches.size(); q-- > 0 && !sch.launches[q].small;) lds = std::max(lds, sch.launches[q].lds_solve);
        const int tall_env = knobs().top_tall;
        sch.top_tall = tall_env != 0;           // the 1024-thread build unless HIPKKT_TOP_TALL=0 (solve_kernels.hip)
        const int cap_env = knobs().top_cap;
        const int cap = std::min(std::min(kTopMaxFronts, cap_env), dev.top_solve_capacity(lds, sch.top_tall));
        for (size_t q = sch.launches.size(); q-- > 0;) {
            const Launch& L = sch.launches[q];
            // (measured on cfg2 with 240 workgroups: x1 0.313, x1.25-1.7 0.307, x2.5 0.319, x6 0.346 ms per solve)
            const double mult = knobs().top_mult;
            if (L.small || L.count > mult * cap) break;
            sch.top_count += L.count;
            sch.top_lds = std::max(sch.top_lds, L.lds_solve);
            ++sch.top_launches;
        }
        sch.top_grid = std::min(cap, sch.top_count);
    }
    if (sch.top_launches < 3) { sch.top_launches = 0; sch.top_count = 0; sch.top_grid = 0; }     // not worth a special kernel
    sch.top_ntask = 0;
    sch.top_nflag = std::max(sch.top_count, 1);
    // Sets with very tall fronts (solve matrix > 3 x slice_kb: far more than a CU should stream per hop) run the
    // (front, slice) kernel: such a front is cut into slices of ~slice_kb (at most slice_max), the others are one task
    // (r03, cfg5: slices of ~80 KB, at most 16, instead of ~120 KB / 8: sweep pair 0.765 -> 0.729 ms; 60 KB / 16 and
    //  40 KB / 32: 0.74 -- a hop is mostly its fixed latencies by then.  A front is sliced when its W exceeds
    //  HIPKKT_SOLVE_SLICE_FROM KB, by default 4.5 slices' worth: cfg3's 395 KB fronts are faster whole)
    // (r04: at most 64 slices instead of 16 -- cfg5's 1.2 MB fronts take 15 either way, the long-range cfg2
    //  variant's 14 154-row panels (11 MB each, 148 of them in a chain) were streamed in 680 KB pieces: sweep pair
    //  4.98 -> 3.85 ms, unit 89.5 -> 81.7 ms; 96 and 128 slices: the same)
    const int slice_kb = knobs().solve_slice_kb;
    const int slice_max = std::max(1, std::min(64, knobs().solve_slice_max));
    const int64_t slice_from = knobs().solve_slice_from >= 0 ? knobs().solve_slice_from * 1024 : (int64_t)slice_kb * 1024 * 9 / 2;
    std::vector<int> tp, ts;
    sch.h_tbase.assign((size_t)sch.top_count + 1, 0);
    const int b0 = sch.top_launches ? sch.launches[sch.launches.size() - sch.top_launches].begin : 0;
    bool any_sliced = false, set_has_tall = false, tall_unsliceable = false;
    size_t slds = 0;
    for (int p = 0; p < sch.top_count; ++p) {
        const int sn = sch.sched[(size_t)b0 + p];
        const int f = front_size(S, sn), nc = S.sn_start[sn + 1] - S.sn_start[sn], nb = f - nc;
        const int64_t wbytes = (int64_t)f * nc * 8;
        int R = 1;
        if (slice_kb > 0 && wbytes > slice_from)
            R = (int)std::min<int64_t>(slice_max, (wbytes + (int64_t)slice_kb * 1024 - 1) / ((int64_t)slice_kb * 1024));
        const bool tallf = front_is_tall(S, sn);                        // (too tall for k_top_solve's LDS: slices only)
        if (tallf) R = std::max(R, 2);
        set_has_tall = set_has_tall || tallf;
        R = std::max(1, std::min(R, std::max(1, nb)));
        if (tallf && R < 2) tall_unsliceable = true;
        any_sliced = any_sliced || R > 1;
        sch.h_tbase[(size_t)p] = (int)tp.size();
        for (int q = 0; q < R; ++q) { tp.push_back(p); ts.push_back(q | (R << 8)); }
        const size_t nloc = (size_t)nc + (size_t)((nb + R - 1) / R) + 8;
        const size_t fwd = (size_t)((nc + 3) & ~3) + nloc * (1 + (size_t)((nc + 7) >> 3));
        const size_t bwd = (size_t)((f + 3) & ~3) + 16 * 16;
        slds = std::max(slds, std::max(fwd, bwd) * sizeof(double));
    }
    sch.h_tbase[(size_t)sch.top_count] = (int)tp.size();
    if (any_sliced && sch.top_count > 0) {
        sch.top_ntask = (int)tp.size();
        sch.top_nflag = sch.top_ntask;
        sch.top_slds = slds;
        sch.top_sgrid = std::min(dev.top_solve_sliced_capacity(slds, 1), sch.top_ntask);
        // (two right-hand sides per sweep: twice the LDS, the same grid or none)
        sch.top_sgrid2 = slds * 2 <= 150 * 1024 ? std::min(dev.top_solve_sliced_capacity(slds * 2, 2), sch.top_ntask) : 0;
        if (sch.top_sgrid2 < sch.top_sgrid) sch.top_sgrid2 = 0;
        sch.tp = tp; sch.ts = ts;
        if (sch.top_sgrid <= 0) sch.top_ntask = 0;
    }
    if (set_has_tall && (sch.top_ntask == 0 || tall_unsliceable)) {
        // fronts too tall for the one-front-per-workgroup kernel, and the (front, slice) kernel cannot take the set
        // either (a slice's vectors beyond a CU's LDS: fronts of ~18 000 rows and more): no persistent set at all,
        // the sweeps go level by level (k_fwd_tall / k_bwd_tall for those fronts).  (h_tbase, tp and ts keep the dropped
        // set's tasks; with top_ntask == 0 no sweep reads them)
        sch.top_launches = 0; sch.top_count = 0; sch.top_grid = 0; sch.top_ntask = 0; sch.top_nflag = 1;
    }
}

// chained launches: every launch must fit the chained kernels (no front beyond the block kernels' LDS)
// chain_from: the longest suffix of launches with at most chain_max workgroups each (HIPKKT_CHAIN_MAX; the wide
// levels below are throughput-bound: a launch each costs them little, while their thousands of waiting
// workgroups would crowd a chained grid), every front of which fits the chained kernels' LDS
static void pick_chain(const Symbolic& S, Schedule& sch)
{
    const int chain_max = knobs().chain_max;
    size_t q = sch.launches.size();
    while (q > 0) {
        const Launch& L = sch.launches[q - 1];
        const int wgs = chain_seg_wgs(L.small ? 0 : L.count, L.small ? L.count - L.ntiny : 0, L.small ? L.ntiny : 0);
        if (L.ntall > 0 || (!L.small && L.lds_solve > 150 * 1024) || wgs > chain_max) break;
        if (!L.small) sch.chain_lds = std::max(sch.chain_lds, L.lds_solve);
        --q;
    }
    sch.chain_from = sch.launches.size() - q >= 2 ? q : sch.launches.size();
    sch.nch.assign((size_t)std::max(S.nsuper, 1), 0);
    if (sch.chain_from < sch.launches.size()) {
        const int p0 = sch.launches[sch.chain_from].begin;
        for (int c = 0; c < S.nsuper; ++c)
            if (S.sn_parent[c] >= 0 && sch.spos[(size_t)c] >= p0) sch.nch[(size_t)S.sn_parent[c]]++;
    }
}


Schedule build_schedule(const Symbolic& S, const DeviceLimits& dev, int64_t panel_cap, int panel_max_slices)
{
    Schedule sch;
    form_launches(S, dev, panel_cap, panel_max_slices, sch);
    admit_overlap(dev, sch);
    pick_late(sch);
    pick_top(S, dev, sch);
    pick_chain(S, sch);
    sch.rec_bytes = layout_records(sch.launches, &sch.rec_refused_bytes);
    return sch;
}

int rec_classes(const Launch& L, RecClass out[2])
{
    int n = 0;
    if (L.small) {
        if (L.count - L.ntiny > 0) out[n++] = {L.begin, L.count - L.ntiny, 1};
        if (L.ntiny > 0) out[n++] = {L.begin + L.count - L.ntiny, L.ntiny, 2};
    } else if (L.count > 0) {
        out[n++] = {L.begin, L.count, 0};
    }
    return n;
}

int64_t layout_records(std::vector<Launch>& launches, int64_t* refused)
{
    const bool packed_on = knobs().packed;
    const int64_t max_mb = knobs().packed_max_mb;
    // (the legacy layout is all launches or none: a refusal half way leaves no launch with a packed segment)
    auto legacy = [&]() { for (Launch& L : launches) L.rec = RecSeg{}; return (int64_t)0; };
    if (refused) *refused = 0;
    legacy();
    if (!packed_on) return 0;
    int64_t total = 0;
    for (size_t q = 0; q < launches.size(); ++q) {
        Launch& L = launches[q];
        const bool leaf = rec_no_slots(launches, q);
        RecClass cls[2];
        const int ncls = rec_classes(L, cls);
        for (int k = 0; k < ncls; ++k) {
            const RecClass& c = cls[k];
            const int fmax = c.cls == 0 ? ((L.fmax + 3) & ~3) : (c.cls == 1 ? 64 : 8);
            const int64_t stride = ((int64_t)kSolveHdrBytes + 4 * (int64_t)fmax + (leaf ? 0 : 32 * (int64_t)fmax) + 63) & ~(int64_t)63;
            if (stride > (1 << 30)) return legacy();
            L.rec.off[c.cls] = total;
            L.rec.stride[c.cls] = (int)stride;
            L.rec.fmax[c.cls] = fmax;
            total += stride * c.count;
        }
    }
    if (total > max_mb * (1 << 20)) {
        if (refused) *refused = total;
        return legacy();
    }
    return total;
}

bool supports_nr(const Schedule& sch, int nr)
{
    if (nr == 1) return true;
    if (nr != 2 && nr != 4) return false;
    // A set with very tall fronts ((front, slice) kernel): two columns at most, and only the launches BELOW the set
    // have to fit -- the set's own fronts (1531 x 96: one column's vectors fill a CU's LDS in the per-level kernels)
    // go through the persistent kernel, or, where that is not available (no claim, given up), column by column
    // (plan_sweep: split_columns).
    if (sch.top_ntask > 0 && (nr != 2 || sch.top_sgrid2 <= 0)) return false;
    const size_t below = sch.top_ntask > 0 ? sch.launches.size() - sch.top_launches : sch.launches.size();
    for (size_t q = 0; q < below; ++q)
        if (!sch.launches[q].small && (sch.launches[q].ntall > 0 || sch.launches[q].lds_solve * (size_t)nr > kLdsCap)) return false;
    // (fronts too tall for the block kernels take one column in the per-level path; inside the (front, slice) set they
    //  are slices like any other)
    return true;
}

int top_grid_for(const Schedule& sch, const DeviceLimits& dev, NrGrids& grids, int nr)
{
    if (nr == 1) return sch.top_grid;
    if (sch.top_ntask > 0) return nr == 2 ? sch.top_sgrid2 : 0;
    int& g = grids.g[nr == 2 ? 0 : 1];
    if (g < 0) g = std::min(sch.top_grid, dev.top_solve_capacity_nr(sch.top_lds * (size_t)nr, nr));
    return g;
}

SweepPlan plan_sweep(const Schedule& sch, const SweepState& st, int nr, const DeviceLimits& dev, NrGrids& grids)
{
    SweepPlan p{};
    p.merge_levels = !knobs().no_level_merge;
    const bool no_top = knobs().no_top;
    if (nr > 1 && sch.top_ntask > 0 && (no_top || !st.use_top || st.top_disabled || sch.top_sgrid2 <= 0)) {
        // two columns through a set with very tall fronts need its persistent kernel (supports_nr): without it, one
        // column after the other
        p.split_columns = true;
        return p;
    }
    const size_t nl = sch.launches.size();
    // the persistent kernel covers the last ntl launches.  Right after a factorisation the W of the narrow top is
    // still being formed on the side stream: that sweep keeps the per-level launches for the levels below the
    // narrow top, so that the formation hides behind them
    // Chained launches (chain_kernels.hip): the launches from chain_from on -- the levels with few enough fronts that
    // a launch per level is one front's latency chain, not throughput -- as segments of ONE grid per direction, ordered
    // by counters in memory instead of kernel boundaries; the wide levels below keep their launches.  The persistent
    // kernel keeps its set -- its 1024-thread workgroups park a whole front's matrix items before the wait, a hop
    // costs ~4 us against ~4.2 forward / ~6.3 backward in the 512-thread chained kernel -- and the launches between
    // chain_from and the set are chained (cfg2: levels 3 and 4, 32 -> 26 us forward).  Both need the device's token
    // (allow_chain / use_top: the caller holds it).  HIPKKT_CHAIN=0: off; HIPKKT_CHAIN_TOP=0: chain to the root
    // instead of the persistent kernel (measured: cfg2's sweep pair 0.2675 against 0.260 ms).
    const bool chain_env = knobs().chain;
    const bool chain_top = knobs().chain_top;
    // (a set with very tall fronts keeps its (front, slice) kernel: such fronts do not fit one workgroup's LDS)
    const bool chain_want = chain_env && st.allow_chain && !st.chain_disabled && sch.chain_from < nl && sch.chain_lds * (size_t)nr <= 150 * 1024;
    p.keep_top = chain_want && (chain_top || sch.top_ntask > 0);
    p.tgrid = (no_top || !st.use_top || st.top_disabled || (chain_want && !p.keep_top)) ? 0 : top_grid_for(sch, dev, grids, nr);
    p.ntl = p.tgrid > 0 ? sch.top_launches : 0;
    p.ncount = sch.top_count;
    // (two columns through a set with very tall fronts: the whole set or nothing -- its lower levels do not fit the
    //  per-level kernels with two columns; the sweep then waits for W at the set's first level)
    if (p.ntl > 0 && st.w_pending && sch.late_launches > 0 && sch.late_launches < p.ntl && !(nr > 1 && sch.top_ntask > 0)) {
        p.ntl = sch.late_launches;
        p.ncount = sch.late_count;
    }
    p.first_w = nl - std::min(nl, sch.late_launches);    // fronts from here on get their W late (w_pending)
    p.chain_on = chain_want && sch.chain_from + 2 <= nl - p.ntl;
    p.nper = p.chain_on ? sch.chain_from : nl - p.ntl;        // launches [0, nper) go level by level, [nper, nl - ntl) chained
    const bool sliced = p.ntl > 0 && sch.top_ntask > 0;
    p.kernel = p.ntl == 0 ? TopKernel::none : (sliced ? TopKernel::sliced : TopKernel::top);
    p.pgrid = p.ntl == 0 ? 0 : (sliced ? (nr == 2 ? sch.top_sgrid2 : sch.top_sgrid) : std::min(p.tgrid, p.ncount));
    p.threads = p.ntl == 0 ? 0 : (sliced || sch.top_tall ? 1024 : 512);
    return p;
}

std::string describe(const SweepPlan& p, const Schedule& sch, int nr, bool w_pending, bool packed)
{
    const size_t nl = sch.launches.size();
    char buf[256];
    std::snprintf(buf, sizeof buf, "nr %d per-level [0,%zu) chained [%zu,%zu) persistent [%zu,%zu) grid %d kernel %s threads %d w_pending %d packed %d",
                  nr, p.nper, p.nper, nl - p.ntl, nl - p.ntl, nl, p.pgrid,
                  p.kernel == TopKernel::none ? "none" : (p.kernel == TopKernel::sliced ? "sliced" : "top"), p.threads, w_pending ? 1 : 0, packed ? 1 : 0);
    return buf;
}

std::string describe_launches(const SweepPlan& p, const Schedule& sch)
{
    std::string out;
    char buf[256];
    for (size_t q = 0; q < p.nper; ++q) {
        const Launch& L = sch.launches[q];
        if (pair_at(sch, q, p)) {
            const Launch& Ls = sch.launches[q + 1];
            std::snprintf(buf, sizeof buf, "[hipkkt] sweep launch %zu+%zu level %d: family level solve_bs %d fmax %d block %d wave %d tiny %d\n", q, q + 1,
                          L.level, L.solve_bs, std::max(L.fmax, Ls.fmax), L.count, Ls.count - Ls.ntiny, Ls.ntiny);
            ++q;
        } else if (L.small) {
            std::snprintf(buf, sizeof buf, "[hipkkt] sweep launch %zu level %d: family small solve_bs 256 fmax %d block 0 wave %d tiny %d\n", q, L.level,
                          L.fmax, L.count - L.ntiny, L.ntiny);
        } else {
            std::snprintf(buf, sizeof buf, "[hipkkt] sweep launch %zu level %d: family %s solve_bs %d fmax %d block %d wave 0 tiny 0\n", q, L.level,
                          L.ntall == 0 ? "block" : (L.ntall == L.count ? "tall" : "block+tall"), L.solve_bs, L.fmax, L.count);
        }
        out += buf;
    }
    return out;
}

// ---- the factorisation's extend-add work lists (schedule.hpp: FactorLists)
namespace {
// parts + 1 cut positions (column indices) of n columns whose pieces start at cp[0 .. n] and which hold tp[j] pulled
// terms each: equal shares of 64 x pieces + terms.  Without terms: the cut on pieces alone, as it has always been.
void cut_columns(const int64_t* cp, const int64_t* tp, int n, int parts, int* col_out)
{
    int64_t nterms = 0;
    for (int j = 0; tp && j < n; ++j) nterms += tp[j];
    const int64_t I0 = cp[0], I1 = cp[n];
    int j = 0;
    if (nterms == 0) {
        for (int w = 0; w < parts; ++w) {
            const int64_t target = I0 + ((I1 - I0) * w) / parts;
            while (j < n && cp[j] < target) ++j;
            col_out[w] = j;
        }
    } else {
        const int64_t total = 64 * (I1 - I0) + nterms;
        int64_t before = 0;                                  // weight of columns [0, j)
        for (int w = 0; w < parts; ++w) {
            const int64_t target = (total * w) / parts;
            while (j < n && before < target) { before += 64 * (cp[j + 1] - cp[j]) + tp[j]; ++j; }
            col_out[w] = j;
        }
    }
    col_out[parts] = n;
}
struct RawTerm { uint32_t leaf_off, tgt_ab; };
// the terms of one owner (the wave slices of a panel that one wave walks, a wave of a tile), in child order -> chunks of
// 64 behind `out`: sorted by target (a target's terms stay in child order), packed densely
void emit_runs(const RawTerm* t, int n, std::vector<PullTerm>& out, int64_t& n_stacked, int& max_depth)
{
    if (n == 0) return;
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return (t[a].tgt_ab & 0x7fff) < (t[b].tgt_ab & 0x7fff); });
    const size_t first = out.size();
    int depth = 0;
    for (int q = 0; q < n; ++q) {
        const RawTerm& r = t[order[(size_t)q]];
        const bool same = q > 0 && (t[order[(size_t)q - 1]].tgt_ab & 0x7fff) == (r.tgt_ab & 0x7fff);
        depth = same ? depth + 1 : 1;
        n_stacked += same;
        max_depth = std::max(max_depth, depth);
        out.push_back(PullTerm{r.leaf_off, r.tgt_ab});
    }
    while (out.size() % 64) out.push_back(PullTerm{0u, kPullNone});
    for (size_t c = first; c < out.size(); c += 64) {        // the doubling steps of the chunk's longest run, into lane 0
        int longest = 1, run = 1;
        for (size_t l = 1; l < 64 && out[c + l].tgt_ab != kPullNone; ++l) {
            run = (out[c + l].tgt_ab & 0x7fff) == (out[c + l - 1].tgt_ab & 0x7fff) ? run + 1 : 1;
            longest = std::max(longest, run);
        }
        uint32_t steps = 0;
        while ((1 << steps) < longest) ++steps;
        out[c].tgt_ab |= steps << 27;
    }
}
}  // namespace

FactorLists build_factor_lists(const Symbolic& S, const Schedule& sch)
{
    FactorLists fl;
    const size_t ns = (size_t)S.nsuper;
    auto fsize = [&](int s) { return front_size(S, s); };
    // DENSE CHILD: a child whose update block IS its parent's whole front (same rows in the same order: the
    // previous panel of a supernode that was cut into panels, the lower front of a chain) needs no work lists at
    // all -- parent entry (r, j) receives child entry (r, j).  The panel kernel and the Schur tiles add it as a
    // dense block (coalesced loads, no descriptors, no row lookups); its pieces stay out of both lists.
    std::vector<int>& dense_child = fl.dense_child;
    dense_child.assign(ns, -1);
    fl.dense_off.assign(ns, -1);
    const bool dense_on = knobs().dense_child;
    for (int p = 0; dense_on && p < S.nsuper; ++p) {
        if (sch.tile_base[p] < 0) continue;                              // block-class parents only
        const int fp = fsize(p);
        for (int e = S.child_ptr[p]; e < S.child_ptr[p + 1]; ++e) {
            const int c = S.child_idx[e];
            const int nbc = (int)(S.rowptr[c + 1] - S.rowptr[c]);
            if (nbc != fp) continue;
            bool ident = true;
            for (int q = 0; ident && q < nbc; ++q) ident = S.rel[S.rowptr[c] + q] == q;
            if (!ident) continue;
            dense_child[(size_t)p] = c;
            fl.dense_off[(size_t)p] = S.upd_off[c];
            break;
        }
    }
    // PULLED LEAVES (the rule: schedule.hpp)
    std::vector<char>& pulled = fl.pulled;
    pulled.assign(ns, 0);
    if (knobs().pull_factor_leaves && S.front_store < ((int64_t)1 << 32)) {      // (a term keeps the leaf's offset in 32 bits)
        std::vector<char> in_small(ns, 0), sliced(ns, 0);
        for (const Launch& L : sch.launches)
            if (L.small) for (int t = L.begin; t < L.begin + L.count; ++t) in_small[(size_t)sch.sched[(size_t)t]] = 1;
        for (const auto& sl : sch.slice_list) sliced[(size_t)sl[0]] = 1;
        for (int c = 0; c < S.nsuper; ++c) {
            const int p = S.sn_parent[c];
            const int nb = (int)(S.rowptr[c + 1] - S.rowptr[c]);
            if (p < 0 || S.sn_start[c + 1] - S.sn_start[c] != 1 || S.child_ptr[c + 1] != S.child_ptr[c] || !in_small[(size_t)c]) continue;
            if (nb < 1 || nb > 63 || sch.tile_base[p] < 0 || sliced[(size_t)p] || dense_child[(size_t)p] == c) continue;
            pulled[(size_t)c] = 1;
            ++fl.n_pulled;
        }
    }
    auto listed = [&](int p, int c) { return dense_child[(size_t)p] != c && !pulled[(size_t)c]; };
    // ---- panel items: one record per child update column and 64-row piece of it, grouped by the (global, permuted) panel
    // column it lands in, children in fixed order -- a wave handles sixteen pieces at a time, all of them a single load
    // round, however long the child's column is
    std::vector<int64_t>& pptr = fl.pptr;
    pptr.assign((size_t)S.N + 1, 0);
    std::vector<int64_t> pterm_col((size_t)S.N, 0);          // pulled terms per panel column
    for (int c = 0; c < S.nsuper; ++c) {
        const int p = S.sn_parent[c];
        if (p < 0 || dense_child[(size_t)p] == c) continue;
        const int pnc = S.sn_start[p + 1] - S.sn_start[p];
        const int nbc = (int)(S.rowptr[c + 1] - S.rowptr[c]);
        for (int b = 0; b < nbc; ++b) {
            const int r = S.rel[S.rowptr[c] + b];
            if (r >= pnc) break;                                   // rel ascends: the rest lands in U
            if (pulled[(size_t)c]) pterm_col[(size_t)S.sn_start[p] + r] += nbc - b;
            else pptr[(size_t)S.sn_start[p] + r + 1] += (nbc - b + 63) / 64;
        }
    }
    for (int i = 0; i < S.N; ++i) pptr[(size_t)i + 1] += pptr[(size_t)i];
    std::vector<ExtItem>& items = fl.items;
    items.resize((size_t)pptr[(size_t)S.N]);
    {
        std::vector<int64_t> nxt(pptr.begin(), pptr.end() - 1);
        for (int p = 0; p < S.nsuper; ++p) {
            const int pnc = S.sn_start[p + 1] - S.sn_start[p];
            for (int e = S.child_ptr[p]; e < S.child_ptr[p + 1]; ++e) {
                const int c = S.child_idx[e];
                if (!listed(p, c)) continue;
                const int nbc = (int)(S.rowptr[c + 1] - S.rowptr[c]);
                for (int b = 0; b < nbc; ++b) {
                    const int64_t q = S.rowptr[c] + b;
                    const int r = S.rel[q];
                    if (r >= pnc) break;
                    for (int a = b; a < nbc; a += 64) {
                        ExtItem it;
                        it.uoff = S.upd_off[c] + (int64_t)b * nbc + a;
                        it.relstart = (int)(S.rowptr[c] + a);
                        it.cnt = std::min(64, nbc - a);
                        it.rfirst = S.rel[S.rowptr[c] + a];
                        it.rlast = S.rel[S.rowptr[c] + a + it.cnt - 1];
                        it.tcol = r;
                        it.pad = 0;
                        items[(size_t)nxt[(size_t)S.sn_start[p] + r]++] = it;
                    }
                }
            }
        }
    }
    // 16 slices of each supernode's panel work, cut on column boundaries
    fl.wcut.assign((ns + sch.slice_list.size()) * 17, 0);
    std::vector<int>& wcol = fl.wcol;                        // ... and the columns they are cut at
    wcol.assign(ns * 17, 0);
    for (int s = 0; s < S.nsuper; ++s) {
        const int nc = S.sn_start[s + 1] - S.sn_start[s];
        const int64_t* cp = pptr.data() + S.sn_start[s];      // nc + 1 column pointers
        int* col = wcol.data() + (size_t)s * 17;
        cut_columns(cp, pterm_col.data() + S.sn_start[s], nc, 16, col);
        for (int w = 0; w <= 16; ++w) fl.wcut[(size_t)s * 17 + w] = cp[col[w]];
    }
    // A row slice of a sliced front gets an item list of its own: the pieces that reach its rows or the top block,
    // in the same order, cut into 16 wave slices of whole columns again -- instead of every slice walking the whole
    // front's list in rounds that are mostly skipped pieces.  (No pulled terms here: a sliced parent pulls nothing.)
    for (size_t q = 0; q < sch.slice_list.size(); ++q) {
        const int s = sch.slice_list[q][0], sl = sch.slice_list[q][1], nsl = sch.slice_list[q][2];
        const int ff = fsize(s), nc = S.sn_start[s + 1] - S.sn_start[s], nb = ff - nc;
        const int rsmax = (nb + nsl - 1) / nsl, r_lo = nc + sl * rsmax;
        const int rs = std::max(0, std::min(rsmax, ff - r_lo));
        const int64_t* cp = pptr.data() + S.sn_start[s];
        std::vector<int64_t> scp((size_t)nc + 1);
        for (int j = 0; j < nc; ++j) {
            scp[(size_t)j] = (int64_t)items.size();
            for (int64_t it = cp[j]; it < cp[j + 1]; ++it) {
                const ExtItem e = items[(size_t)it];
                if (e.rfirst >= nc && (e.rlast < r_lo || e.rfirst >= r_lo + rs)) continue;
                items.push_back(e);
            }
        }
        scp[(size_t)nc] = (int64_t)items.size();
        int col[17];
        cut_columns(scp.data(), nullptr, nc, 16, col);
        for (int k = 0; k <= 16; ++k) fl.wcut[(ns + q) * 17 + (size_t)k] = scp[(size_t)col[k]];
    }
    // ---- Schur sub-items: every child update column that lands in a U column, cut at the parent's
    // 64-row tile boundaries, grouped by (tile, tile column), children in fixed order
    const int64_t ntile = (int64_t)sch.tiles.size();
    std::vector<int64_t>& cnt = fl.tptr;
    cnt.assign((size_t)ntile * 64 + 1, 0);
    std::vector<int64_t> pterm_tcol((size_t)ntile * 64, 0);   // pulled terms per tile column
    auto for_each_sub = [&](bool of_pulled, auto&& fn) {
        for (int p = 0; p < S.nsuper; ++p) {
            if (sch.tile_base[p] < 0) continue;
            const int pnc = S.sn_start[p + 1] - S.sn_start[p];
            for (int e = S.child_ptr[p]; e < S.child_ptr[p + 1]; ++e) {
                const int c = S.child_idx[e];
                if (dense_child[(size_t)p] == c || (pulled[(size_t)c] != 0) != of_pulled) continue;
                const int nbc = (int)(S.rowptr[c + 1] - S.rowptr[c]);
                const int* rl = S.rel.data() + S.rowptr[c];
                for (int b = 0; b < nbc; ++b) {
                    if (rl[b] < pnc) continue;
                    const int j = rl[b] - pnc, tj = j >> 6;
                    int a = b;
                    while (a < nbc) {
                        const int ti = (rl[a] - pnc) >> 6;
                        int a2 = a;
                        while (a2 < nbc && ((rl[a2] - pnc) >> 6) == ti) ++a2;
                        const int64_t tile = sch.tile_base[p] + (int64_t)ti * (ti + 1) / 2 + tj;
                        fn(tile, j & 63, c, b, a, a2 - a, nbc);
                        a = a2;
                    }
                }
            }
        }
    };
    for_each_sub(false, [&](int64_t tile, int q, int, int, int, int, int) { cnt[(size_t)(tile * 64 + q + 1)]++; });
    if (fl.n_pulled) for_each_sub(true, [&](int64_t tile, int q, int, int, int, int n, int) { pterm_tcol[(size_t)(tile * 64 + q)] += n; });
    for (size_t i = 0; i + 1 < cnt.size(); ++i) cnt[i + 1] += cnt[i];
    fl.sit.resize((size_t)cnt.back());
    {
        std::vector<int64_t> nx(cnt.begin(), cnt.end() - 1);
        for_each_sub(false, [&](int64_t tile, int q, int c, int b, int a, int n, int nbc) {
            SubItem si;
            si.uoff = S.upd_off[c] + (int64_t)b * nbc + a;
            si.relstart = (int)(S.rowptr[c] + a);
            si.cnt = (unsigned char)n;
            si.qcol = (unsigned char)q;
            si.pad = 0;
            fl.sit[(size_t)nx[(size_t)(tile * 64 + q)]++] = si;
        });
    }
    fl.tcut.assign((size_t)ntile * 5 + 5, 0);
    std::vector<int>& tcol = fl.tcol;
    tcol.assign((size_t)ntile * 5 + 5, 0);
    for (int64_t t = 0; t < ntile; ++t) {
        const int64_t* cp = cnt.data() + t * 64;       // 65 column pointers of this tile
        int* col = tcol.data() + t * 5;
        cut_columns(cp, pterm_tcol.data() + t * 64, 64, 4, col);
        for (int w = 0; w <= 4; ++w) fl.tcut[(size_t)(t * 5 + w)] = cp[col[w]];
    }
    // ---- the pulled leaves' terms, by owner: wave slice w of front s is owner 16 s + w, wave w of tile t owner 16 nsuper + 4 t + w
    fl.pwcut.assign(ns * 17, 0);
    fl.ptcut.assign((size_t)ntile * 5 + 5, 0);
    // A panel kernel of NW < 16 waves gives every wave 16 / NW consecutive slices: their terms form ONE list (at the first
    // of the slices; the others' ranges are empty).  Launches of the overlap region count as 16 waves -- their panels may go
    // out in a merged 1024-thread kernel, and a kernel of fewer waves walks consecutive lists, which is as good.
    fl.spw.assign(ns, 1);
    for (size_t q = 0; q < sch.launches.size() && q < sch.ov_first; ++q) {
        const Launch& L = sch.launches[q];
        if (L.small) continue;
        for (int t = L.begin; t < L.begin + L.count; ++t) fl.spw[(size_t)sch.sched[(size_t)t]] = std::max(1, 16 / std::max(1, L.bs_panel / 64));
    }
    if (fl.n_pulled == 0) return fl;
    const size_t nown = ns * 16 + (size_t)ntile * 4;
    std::vector<int64_t> optr(nown + 1, 0);
    auto slice_of = [](const int* col, int parts, int j) { int w = 0; while (w + 1 < parts && col[w + 1] <= j) ++w; return w; };
    auto for_each_term = [&](auto&& fn) {
        for (int p = 0; p < S.nsuper; ++p) {
            if (sch.tile_base[p] < 0) continue;
            const int pnc = S.sn_start[p + 1] - S.sn_start[p], fp = fsize(p);
            for (int e = S.child_ptr[p]; e < S.child_ptr[p + 1]; ++e) {
                const int c = S.child_idx[e];
                if (!pulled[(size_t)c]) continue;
                const int nbc = (int)(S.rowptr[c + 1] - S.rowptr[c]);
                const int* rl = S.rel.data() + S.rowptr[c];
                for (int b = 0; b < nbc; ++b)
                    for (int a = b; a < nbc; ++a) {
                        const int ra = rl[a], rb = rl[b];
                        size_t owner;
                        int target;
                        if (rb < pnc) {
                            const int w = slice_of(wcol.data() + (size_t)p * 17, 16, rb);
                            owner = (size_t)p * 16 + (size_t)(w - w % fl.spw[(size_t)p]);     // the first slice of the wave that owns w
                            target = ra + (int)(((int64_t)rb * (2 * fp - 1 - rb)) >> 1);        // the panel's trapezoid (pcol)
                        } else {
                            const int j = rb - pnc, i = ra - pnc;
                            const int64_t tile = sch.tile_base[p] + (int64_t)(i >> 6) * ((i >> 6) + 1) / 2 + (j >> 6);
                            owner = ns * 16 + (size_t)tile * 4 + (size_t)slice_of(tcol.data() + tile * 5, 4, j & 63);
                            target = (j & 63) * 65 + (i & 63);                                   // Ct[qcol][row], ld TS + 1
                        }
                        if (target > 0x7fff) throw std::runtime_error("pulled leaf: target beyond 15 bits");
                        fn(owner, RawTerm{(uint32_t)S.front_off[c], (uint32_t)target | ((uint32_t)a << 15) | ((uint32_t)b << 21)});
                    }
            }
        }
    };
    for_each_term([&](size_t owner, const RawTerm&) { ++optr[owner + 1]; });
    for (size_t o = 0; o < nown; ++o) optr[o + 1] += optr[o];
    fl.n_terms = optr[nown];
    std::vector<RawTerm> raw((size_t)fl.n_terms);
    {
        std::vector<int64_t> nx(optr.begin(), optr.end() - 1);
        for_each_term([&](size_t owner, const RawTerm& t) { raw[(size_t)nx[owner]++] = t; });
    }
    for (size_t o = 0; o < nown; ++o) {
        const int chunk = (int)(fl.pterms.size() / 64);
        if (o < ns * 16) fl.pwcut[(o / 16) * 17 + o % 16] = chunk;
        else fl.ptcut[((o - ns * 16) / 4) * 5 + (o - ns * 16) % 4] = chunk;
        emit_runs(raw.data() + optr[o], (int)(optr[o + 1] - optr[o]), fl.pterms, fl.n_stacked, fl.max_depth);
        const int end = (int)(fl.pterms.size() / 64);
        if (o < ns * 16) { if (o % 16 == 15) fl.pwcut[(o / 16) * 17 + 16] = end; }
        else if ((o - ns * 16) % 4 == 3) fl.ptcut[((o - ns * 16) / 4) * 5 + 4] = end;
        if (fl.pterms.size() / 64 > (size_t)0x7fffff00) throw std::runtime_error("pulled leaves: too many term chunks");
    }
    return fl;
}

std::string describe_pieces(const Symbolic& S, const Schedule& sch, const FactorLists& fl)
{
    struct Row {
        int64_t tile_pieces = 0, tile_entries = 0, tile_len[3] = {0, 0, 0};      // pieces of <= 4, 5..16, 17..64 entries
        int64_t panel_pieces = 0, panel_entries = 0;
        int64_t pulled_tile_pieces = 0, pulled_panel_pieces = 0, terms = 0, stacked = 0;
        int depth = 0;
    };
    std::vector<Row> rows(S.levels.size());
    std::unordered_map<uint64_t, int> hit;                   // per entry (ra >= rb) of the parent's front
    for (int p = 0; p < S.nsuper; ++p) {
        if (sch.tile_base[p] < 0) continue;
        Row& R = rows[(size_t)S.sn_level[p]];
        const int pnc = S.sn_start[p + 1] - S.sn_start[p];
        hit.clear();
        for (int e = S.child_ptr[p]; e < S.child_ptr[p + 1]; ++e) {
            const int c = S.child_idx[e];
            if (fl.dense_child[(size_t)p] == c) continue;
            const bool pl = fl.pulled[(size_t)c] != 0;
            const int nbc = (int)(S.rowptr[c + 1] - S.rowptr[c]);
            const int* rl = S.rel.data() + S.rowptr[c];
            for (int b = 0; b < nbc; ++b) {
                if (rl[b] < pnc) {
                    const int64_t np = (nbc - b + 63) / 64;
                    if (pl) R.pulled_panel_pieces += np; else { R.panel_pieces += np; R.panel_entries += nbc - b; }
                } else {
                    int a = b;
                    while (a < nbc) {
                        const int ti = (rl[a] - pnc) >> 6;
                        int a2 = a;
                        while (a2 < nbc && ((rl[a2] - pnc) >> 6) == ti) ++a2;
                        const int n = a2 - a;
                        if (pl) ++R.pulled_tile_pieces;
                        else { ++R.tile_pieces; R.tile_entries += n; ++R.tile_len[n <= 4 ? 0 : n <= 16 ? 1 : 2]; }
                        a = a2;
                    }
                }
                if (pl) for (int a = b; a < nbc; ++a) {
                    const uint64_t key = (uint64_t)rl[a] << 32 | (uint32_t)rl[b];
                    ++R.terms;
                    if (hit[key]++ > 0) ++R.stacked;
                    R.depth = std::max(R.depth, hit[key]);
                }
            }
        }
    }
    std::string out;
    char buf[512];
    for (size_t l = 0; l < rows.size(); ++l) {
        const Row& R = rows[l];
        if (R.tile_pieces + R.panel_pieces + R.terms == 0) continue;
        std::snprintf(buf, sizeof buf, "[pieces] parent level %2zu: tile pieces %lld (%lld entries; <=4: %lld, 5-16: %lld, 17-64: %lld), panel pieces %lld "
                      "(%lld entries) | pulled leaves took out %lld tile and %lld panel pieces: %lld terms, %lld stacked, deepest %d\n", l,
                      (long long)R.tile_pieces, (long long)R.tile_entries, (long long)R.tile_len[0], (long long)R.tile_len[1], (long long)R.tile_len[2],
                      (long long)R.panel_pieces, (long long)R.panel_entries, (long long)R.pulled_tile_pieces, (long long)R.pulled_panel_pieces,
                      (long long)R.terms, (long long)R.stacked, R.depth);
        out += buf;
    }
    std::snprintf(buf, sizeof buf, "[pieces] pulled leaves %lld, terms %lld in %zu chunks of 64 (%lld onto an earlier term's target, deepest stack %d)\n",
                  (long long)fl.n_pulled, (long long)fl.n_terms, fl.pterms.size() / 64, (long long)fl.n_stacked, fl.max_depth);
    out += buf;
    return out;
}

}  // namespace hipkkt
