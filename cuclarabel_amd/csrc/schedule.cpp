// The numeric engine's decisions (schedule.hpp): plain host code, compiled without HIP -- the host sanitizer driver
// (tests/sanitize/host_driver.cpp) builds it with g++ and checks what it decides on a machine without a GPU.
#include "schedule.hpp"

#include <algorithm>
#include <cstdio>
#include <stdexcept>

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

}  // namespace hipkkt
