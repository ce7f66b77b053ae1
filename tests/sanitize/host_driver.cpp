// Sanitizer driver for the HOST side of the product (set-up only code: csrc/kkt_assembly.cpp, csrc/ordering.cpp,
// csrc/symbolic.cpp, csrc/schedule.cpp, csrc/engine_tables.cpp), built by tests/test_host_sanitizers.py with g++ -fsanitize=address,undefined (the
// GPU box offers no AddressSanitizer; the kernels are covered by the parity suite, the host code by this).  No HIP, no device.
//
// Input file (little-endian): int64 n, m, ncones, nnzP, nnzA, nd_leaf_size; int64 Pp[n+1], Pi[nnzP]; double Px[nnzP];
// int64 Ap[n+1], Ai[nnzA]; double Ax[nnzA]; int32 kinds[ncones]; int64 dims[ncones].
// For each file and ordering: assemble the KKT pattern and its maps, check the maps against the pattern, run the
// symbolic analysis, check the permutation and the level lists, build the launch schedule and the sweep plans
// (schedule.cpp) and check them, build the device tables of the engine (engine_tables.cpp) and of the KKT handle
// (kkt_assembly.cpp: build_kkt_image, build_cone_tables) and check their invariants, print one line.  The tables are built
// under the HIPKKT_* knobs of this process: with HIPKKT_TILE_XCD=0 the tile order must be the identity, with
// HIPKKT_PULL_LEAVES=0 nothing may be pulled.
//
// host_driver --plans FILE...: FILE holds one triu CSC pattern (int64 N, nnz; int64 colptr[N+1], rowval[nnz]); it is
// analysed in its natural order, as the tests' forests are, and the sweep-plan lines of HIPKKT_VERBOSE=2 are printed
// for it as the engine prints them -- under the HIPKKT_* knobs of this process (tests/test_schedule_host.py; built
// without sanitizers there).
//
// host_driver --multi-shape KP...: one line per padded column count with the kernel instances the many-column sweeps take
// (launch_shapes.hpp: multi_shape) under HIPKKT_MULTI_VEC / HIPKKT_MULTI_CT of this process (tests/test_multi_sweeps_host.py).
// host_driver --launches FILE...: per pattern (as for --plans) one line per launch and one per supernode, for the tests
// that reason about which fronts the many-column sweeps pull (tests/test_multi_sweeps_host.py); then, from the product's
// own tables, "P sn flag" per supernode (pulled by the many-column sweeps) and "M a b c": the three numbers of the engine's
// "contribution rows pulled" line, and "D launches tiles": the launches whose tiles were dealt to XCD residue classes and
// their tiles (tests/test_engine_tables_host.py).  Every mode that builds a schedule checks the engine's tables for it.
#include "hipkkt.h"

#include "engine_tables.hpp"
#include "kkt_assembly.hpp"
#include "knobs.hpp"
#include "launch_shapes.hpp"
#include "schedule.hpp"
#include "symbolic.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

using namespace hipkkt;

template <class T>
static std::vector<T> rd(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) throw std::runtime_error("short read");
    return v;
}

static void require(bool ok, const char* what)
{
    if (!ok) throw std::runtime_error(std::string("check failed: ") + what);
}

// The device's part of a schedule, fixed: 256 CUs and one resident workgroup per CU at 6 % spare (240) for all three
// occupancy questions -- what the comments in solve_kernels.hip describe for MI355X; nobody has confirmed the figure on a
// device from here, and the checks below hold for any positive value.
static DeviceLimits fixed_limits()
{
    DeviceLimits d;
    d.n_cus = 256;
    d.top_solve_capacity = [](size_t, bool) { return 240; };
    d.top_solve_capacity_nr = [](size_t, int) { return 240; };
    d.top_solve_sliced_capacity = [](size_t, int) { return 240; };
    return d;
}

static void check_schedule(const Symbolic& S, const Schedule& sch, const DeviceLimits& dev)
{
    const std::vector<Launch>& Ls = sch.launches;
    const size_t nl = Ls.size();
    // sched is a permutation of the supernodes, and the launches partition it in order
    require((int)sch.sched.size() == S.nsuper && (int)sch.spos.size() == S.nsuper, "sched size");
    std::vector<int> launch_of((size_t)S.nsuper, -1);
    int pos = 0;
    for (size_t q = 0; q < nl; ++q) {
        require(Ls[q].begin == pos && Ls[q].count > 0, "launches partition sched in order");
        for (int t = pos; t < pos + Ls[q].count; ++t) {
            require(t < S.nsuper, "launch inside sched");
            const int sn = sch.sched[(size_t)t];
            require(sn >= 0 && sn < S.nsuper && launch_of[(size_t)sn] == -1 && sch.spos[(size_t)sn] == t, "sched is a permutation");
            launch_of[(size_t)sn] = (int)q;
        }
        pos += Ls[q].count;
        require(Ls[q].ntiny >= 0 && Ls[q].ntiny <= Ls[q].count && Ls[q].ntall >= 0 && Ls[q].ntall <= Ls[q].count &&
                Ls[q].nsliced >= 0 && Ls[q].nsliced <= Ls[q].count, "class counts inside the launch");
    }
    require(pos == S.nsuper, "every supernode in a launch");
    // every front's children sit in an earlier launch
    for (int sn = 0; sn < S.nsuper; ++sn)
        require(S.sn_parent[sn] < 0 || launch_of[(size_t)sn] < launch_of[(size_t)S.sn_parent[sn]], "children in earlier launches");
    // a childless front sits in a level-0 launch (the many-column backward sweep runs the pulled leaves' kernel there only)
    for (int sn = 0; sn < S.nsuper; ++sn)
        require(S.child_ptr[sn + 1] != S.child_ptr[sn] || Ls[(size_t)launch_of[(size_t)sn]].level == 0, "childless fronts in level-0 launches");
    // tiles, row slices and W lists: each launch's range follows the previous one's and holds its own fronts'
    require((int)sch.tile_base.size() == S.nsuper, "tile_base size");
    size_t tile = 0, slice = 0, tinv = 0;
    for (size_t q = 0; q < nl; ++q) {
        const Launch& L = Ls[q];
        require((size_t)L.tile_begin == tile && L.ntiles >= 0, "tile ranges in order");
        require((size_t)L.slice_begin == slice && L.slice_count >= 0, "slice ranges in order");
        require((size_t)L.tinv_begin == tinv && L.tinv_count == (L.small ? 0 : L.count), "W list ranges in order");
        size_t tl = tile;
        for (int t = L.begin; t < L.begin + L.count; ++t) {
            const int sn = sch.sched[(size_t)t];
            if (L.small) { require(sch.tile_base[(size_t)sn] == -1, "one-wave fronts have no tiles"); continue; }
            require(sch.tinv_list[tinv + (size_t)(t - L.begin)] == sn, "W list holds the launch's fronts");
            const int nb = (int)(S.rowptr[sn + 1] - S.rowptr[sn]), nt = (nb + 63) / 64;
            require(sch.tile_base[(size_t)sn] == (int64_t)tl, "tile_base follows the launch order");
            for (int k = 0; k < nt * (nt + 1) / 2; ++k, ++tl) {
                require(tl < sch.tiles.size(), "tile inside the list");
                const uint64_t v = (uint64_t)sch.tiles[tl];
                const int ti = (int)((v >> 48) & 0xffff), tj = (int)((v >> 32) & 0xffff);
                require((int)(uint32_t)v == sn && tj <= ti && ti < nt, "tile of its front");
            }
        }
        require(tl == tile + (size_t)L.ntiles, "ntiles");
        for (int k = 0; k < L.slice_count; ++k) {
            require(slice + (size_t)k < sch.slice_list.size(), "slice inside the list");
            const auto& e = sch.slice_list[slice + (size_t)k];
            require(e[0] >= 0 && e[0] < S.nsuper && launch_of[(size_t)e[0]] == (int)q && e[1] >= 0 && e[1] < e[2], "slice of a front of its launch");
        }
        tile += (size_t)L.ntiles; slice += (size_t)L.slice_count; tinv += (size_t)L.tinv_count;
    }
    require(tile == sch.tiles.size() && slice == sch.slice_list.size() && tinv == sch.tinv_list.size(), "lists end with the last launch");
    require(sch.tinv_small_prefix.size() == sch.tinv_list.size() + 1, "W prefix size");
    // the persistent set, the late set and the overlap range: suffixes of block-class launches; the chained range a suffix
    auto block_suffix = [&](size_t n, const char* what) {
        require(n <= nl, what);
        for (size_t q = nl - n; q < nl; ++q) require(!Ls[q].small, what);
    };
    block_suffix(sch.top_launches, "persistent set");
    block_suffix(sch.late_launches, "late set");
    require(sch.ov_first <= nl, "overlap range");
    block_suffix(nl - sch.ov_first, "overlap range");
    require(sch.chain_from >= nl || sch.chain_from + 2 <= nl, "chained range");
    int cnt = 0;
    for (size_t q = nl - sch.top_launches; q < nl; ++q) cnt += Ls[q].count;
    require(cnt == sch.top_count && sch.top_grid <= std::max(sch.top_count, 0), "persistent set's fronts");
    // (front, slice) tasks
    for (size_t k = 0; k + 1 < sch.h_tbase.size(); ++k) require(sch.h_tbase[k] <= sch.h_tbase[k + 1], "h_tbase non-decreasing");
    // (a set dropped after its tasks were listed keeps them: consistent among themselves, and top_ntask == 0)
    require(sch.ts.size() == sch.tp.size() && (sch.top_ntask == 0 || sch.top_ntask == (int)sch.tp.size()) &&
            (sch.tp.empty() || (!sch.h_tbase.empty() && sch.h_tbase.back() == (int)sch.tp.size())), "task list consistent with h_tbase");
    for (size_t k = 0; k < sch.tp.size(); ++k)
        require(sch.tp[k] >= 0 && (size_t)sch.tp[k] + 1 < sch.h_tbase.size() && sch.h_tbase[(size_t)sch.tp[k]] <= (int)k &&
                (int)k < sch.h_tbase[(size_t)sch.tp[k] + 1], "task inside its front's range");
    if (sch.top_ntask > 0)
        require((int)sch.h_tbase.size() == sch.top_count + 1 && sch.h_tbase.back() == sch.top_ntask && (int)sch.tp.size() == sch.top_ntask &&
                sch.ts.size() == sch.tp.size(), "h_tbase ends at the task count");
    // merged panel kernels
    require(sch.ov_group_of.size() == nl, "ov_group_of size");
    for (const MergeGroup& g : sch.ov_groups)
        require(g.first >= sch.ov_first + 1 && g.end <= nl && g.end >= g.first + 2, "merged run inside the overlap range");
    // sweep plans
    NrGrids grids;
    for (int nr : {1, 2, 4}) {
        if (!supports_nr(sch, nr)) continue;
        for (int bits = 0; bits < 16; ++bits) {
            const SweepState st{(bits & 1) != 0, (bits & 2) != 0, (bits & 8) != 0, false, (bits & 4) != 0};
            const SweepPlan p = plan_sweep(sch, st, nr, dev, grids);
            if (p.split_columns) { require(nr > 1 && sch.top_ntask > 0, "column split only through a sliced set"); continue; }
            require(p.ntl <= nl && p.nper <= nl - p.ntl, "0 <= nper <= nl - ntl <= nl");
            require(p.ntl == 0 || p.ntl == sch.late_launches || p.ntl == sch.top_launches, "ntl is none, the late set or the whole set");
            require(!p.chain_on || (p.nper == sch.chain_from && nl - p.ntl >= p.nper + 2), "chained range");
            require(p.chain_on || p.nper == nl - p.ntl, "no gap without chaining");
            require((p.ntl == 0) == (p.kernel == TopKernel::none) && (p.ntl == 0 || (p.pgrid > 0 && st.use_top && !st.top_disabled)), "persistent kernel");
            (void)describe(p, sch, nr, st.w_pending, sch.rec_bytes > 0);
            (void)describe_launches(p, sch);
        }
    }
}

// The engine's device tables (engine_tables.cpp) for one schedule, under this process's knobs: built and checked.
static EngineTables check_tables(const Symbolic& S, const Schedule& sch)
{
    FactorLists fl = build_factor_lists(S, sch);
    const std::vector<int64_t> tcut0(fl.tcut);           // (in sch.tiles order: the builder permutes them with the tiles)
    const std::vector<int> ptcut0(fl.ptcut);
    const std::vector<int> dsigns((size_t)S.N, 1);
    const EngineTables T = build_engine_tables(S, sch, fl, dsigns);
    const int64_t nloc = (int64_t)S.N + (int64_t)S.rows.size();
    const size_t nrows = S.rows.size();
    auto nc_of = [&](int s) { return S.sn_start[s + 1] - S.sn_start[s]; };
    auto nb_of = [&](int s) { return (int)(S.rowptr[s + 1] - S.rowptr[s]); };
    std::vector<int> row_sn(nrows, -1);
    int64_t nparented = 0;
    for (int c = 0; c < S.nsuper; ++c) {
        for (int64_t q = S.rowptr[c]; q < S.rowptr[c + 1]; ++q) row_sn[(size_t)q] = c;
        if (S.sn_parent[c] >= 0) nparented += nb_of(c);
    }

    // ---- gather lists
    require((int64_t)T.item_ptr.size() == nloc + 1 && T.item_ptr[0] == 0, "item_ptr size");
    for (int64_t i = 0; i < nloc; ++i) require(T.item_ptr[(size_t)i] <= T.item_ptr[(size_t)i + 1], "item_ptr monotone");
    require(T.item_ptr[(size_t)nloc] == nparented && (int64_t)T.gsrc.size() == nparented, "item_ptr ends at the rows that have a parent");
    require(T.udst.size() == std::max<size_t>(nrows, 1), "udst size");
    {
        std::vector<char> hit(nrows, 0);
        for (size_t g = 0; g < T.gsrc.size(); ++g) {
            const int q = T.gsrc[g];
            require(q >= 0 && (size_t)q < nrows && !hit[(size_t)q] && S.sn_parent[row_sn[(size_t)q]] >= 0, "gsrc hits each parented row once");
            hit[(size_t)q] = 1;
            require(T.udst[(size_t)q] == (int)g, "udst[gsrc[g]] == g");
        }
        // an entry sits in the list of the row it lands in
        for (int s = 0; s < S.nsuper; ++s)
            for (int i = 0; i < front_size(S, s); ++i) {
                const int64_t lc = (int64_t)S.sn_start[s] + S.rowptr[s] + i;
                for (int64_t g = T.item_ptr[(size_t)lc]; g < T.item_ptr[(size_t)lc + 1]; ++g) {
                    const int q = T.gsrc[(size_t)g];
                    require(S.sn_parent[row_sn[(size_t)q]] == s && S.rel[(size_t)q] == i, "gather entry keyed by its receiving row");
                }
            }
    }

    // ---- packed K positions
    require(T.ksrc.size() == T.kdst.size() && T.ksrc.size() >= S.ksrc.size(), "K list sizes");
    require(T.slice_kptr.size() == sch.slice_list.size() && T.slice_nk.size() == sch.slice_list.size(), "slice K list sizes");
    for (size_t e = 0; e < S.ksrc.size(); ++e) require(T.ksrc[e] == S.ksrc[e], "whole fronts' K sources unchanged");
    for (const Launch& L : sch.launches) {
        for (int t = L.begin; t < L.begin + L.count; ++t) {
            const int s = sch.sched[(size_t)t], f = front_size(S, s), nc = nc_of(s);
            const bool packed = !L.small && t < L.begin + L.count - L.nsliced;
            std::vector<int> seen;
            for (int64_t e = S.kptr[s]; e < S.kptr[s + 1]; ++e) {
                if (!packed) { require(T.kdst[(size_t)e] == S.kdst[(size_t)e], "one-wave and sliced fronts keep lrow + lcol * f"); continue; }
                const int lcol = S.kdst[(size_t)e] / f, lrow = S.kdst[(size_t)e] - lcol * f;
                require(lcol < nc && lrow >= lcol, "K entry in the panel's lower part");
                const int64_t pos = T.kdst[(size_t)e], c0 = ((int64_t)lcol * (2 * f - 1 - lcol)) >> 1;
                require(pos == c0 + lrow && pos >= 0 && pos < (int64_t)nc * f - (int64_t)nc * (nc - 1) / 2, "packed position inside the trapezoid");
                seen.push_back((int)pos);
            }
            std::sort(seen.begin(), seen.end());
            require(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "packed positions distinct");
        }
    }
    {
        int64_t tail = (int64_t)S.ksrc.size();
        size_t q = 0;
        while (q < sch.slice_list.size()) {
            const int s = sch.slice_list[q][0], nsl = sch.slice_list[q][2];
            const int ff = front_size(S, s), nc = nc_of(s);
            std::map<int, int> times;                    // K entry of the front -> slices that list it
            for (int sl = 0; sl < nsl; ++sl, ++q) {
                require(q < sch.slice_list.size() && sch.slice_list[q][0] == s && sch.slice_list[q][1] == sl && sch.slice_list[q][2] == nsl, "a front's slices are consecutive");
                require(T.slice_kptr[q] == tail && T.slice_nk[q] >= 0, "slice K lists tile the tail");
                // a slice's entries come in the front's own order, so one merge pass matches them to the front's entries
                int64_t e = S.kptr[s];
                for (int64_t k = tail; k < tail + T.slice_nk[q]; ++k) {
                    while (e < S.kptr[s + 1] && S.ksrc[(size_t)e] != T.ksrc[(size_t)k]) ++e;
                    require(e < S.kptr[s + 1], "slice K entry belongs to its front");
                    ++times[(int)(e - S.kptr[s])];
                    ++e;
                }
                tail += T.slice_nk[q];
            }
            for (int64_t e = S.kptr[s]; e < S.kptr[s + 1]; ++e) {
                const int lcol = S.kdst[(size_t)e] / ff, r = S.kdst[(size_t)e] - lcol * ff;
                const auto it = times.find((int)(e - S.kptr[s]));
                require(it != times.end() && it->second == (r < nc ? nsl : 1), "top-block entries in every slice, the others in exactly one");
            }
        }
        require(tail == (int64_t)T.ksrc.size(), "slice K lists end the list");
    }

    // ---- tile order
    require(T.tiles.size() == sch.tiles.size() && fl.tcut.size() == tcut0.size() && fl.ptcut.size() == ptcut0.size(), "tile list sizes");
    {
        std::vector<char> covered(sch.tiles.size(), 0);
        for (const Launch& L : sch.launches) {
            std::map<int64_t, int64_t> from;             // tile word -> its index in sch.tiles (a launch's tiles are distinct)
            for (int64_t t = L.tile_begin; t < (int64_t)L.tile_begin + L.ntiles; ++t) {
                require(from.emplace(sch.tiles[(size_t)t], t).second, "tiles of a launch distinct");
                covered[(size_t)t] = 1;
            }
            for (int64_t t = L.tile_begin; t < (int64_t)L.tile_begin + L.ntiles; ++t) {
                const auto it = from.find(T.tiles[(size_t)t]);
                require(it != from.end() && it->second >= 0, "uploaded tiles are a permutation of the launch's tiles");
                const int64_t f0 = it->second;
                it->second = -1;
                for (int w = 0; w < 5; ++w)
                    require(fl.tcut[(size_t)t * 5 + w] == tcut0[(size_t)f0 * 5 + w] && fl.ptcut[(size_t)t * 5 + w] == ptcut0[(size_t)f0 * 5 + w],
                            "tcut / ptcut rows travel with their tiles");
                if (knobs().tile_xcd <= 0) require(f0 == t, "HIPKKT_TILE_XCD=0: identity");
            }
        }
        for (char c : covered) require(c != 0, "every tile in a launch");
        if (knobs().tile_xcd <= 0) require(T.dealt_launches == 0 && T.tiles == sch.tiles, "HIPKKT_TILE_XCD=0: no launch dealt");
    }

    // ---- pulled-leaf split
    require((int)T.solve_pulled.size() == S.nsuper && (int64_t)T.glm_ptr.size() == nloc + 1 && T.udst_m.size() == std::max<size_t>(nrows, 1), "pull list sizes");
    require((int)T.pr_ptr.size() == T.n_pull_rows + 1 && (int)T.pr_slot.size() == std::max(T.n_pull_rows, 1) && T.pr_ptr[0] == 0 &&
            T.pr_ptr.back() == T.n_pull_terms, "pr_ptr / pr_slot sizes agree with n_pull_rows");
    require(T.hp_col.size() == (size_t)std::max<int64_t>(T.n_pull_terms, 1) && T.hp_row.size() == T.hp_col.size() && T.hp_lidx.size() == T.hp_col.size(), "pulled term list sizes");
    {
        int64_t slot = 0, term = 0;
        int prow = 0;
        for (int64_t lc = 0; lc < nloc; ++lc) {
            require(T.glm_ptr[(size_t)lc] == slot, "a row's slots are consecutive");
            int64_t npulled = 0, nstored = 0;
            for (int64_t g = T.item_ptr[(size_t)lc]; g < T.item_ptr[(size_t)lc + 1]; ++g) npulled += T.solve_pulled[(size_t)row_sn[(size_t)T.gsrc[(size_t)g]]] != 0;
            if (npulled) {
                require(prow < T.n_pull_rows && T.pr_slot[(size_t)prow] == (int)slot && T.pr_ptr[(size_t)prow] == term &&
                        T.pr_ptr[(size_t)prow + 1] == term + npulled, "the sum slot first, its terms in pr_ptr");
                ++slot; ++prow;
            }
            for (int64_t g = T.item_ptr[(size_t)lc]; g < T.item_ptr[(size_t)lc + 1]; ++g) {
                const int q = T.gsrc[(size_t)g], c = row_sn[(size_t)q];
                if (T.solve_pulled[(size_t)c]) {
                    require(T.udst_m[(size_t)q] == -1 && T.hp_col[(size_t)term] == S.sn_start[c] && T.hp_row[(size_t)term] == S.perm[(size_t)S.sn_start[c]], "pulled term names its leaf");
                    require(T.hp_lidx[(size_t)term] > S.front_off[c] && T.hp_lidx[(size_t)term] < S.front_off[c] + front_size(S, c) &&
                            T.hp_lidx[(size_t)term] == S.front_off[c] + 1 + (q - S.rowptr[c]), "hp_lidx inside the leaf's panel");
                    ++term;
                } else {
                    require(T.udst_m[(size_t)q] == (int)slot, "stored slots consecutive");
                    ++slot; ++nstored;
                }
            }
            require(nstored + npulled == T.item_ptr[(size_t)lc + 1] - T.item_ptr[(size_t)lc], "stored slots plus pulled terms = gather count");
        }
        require(T.glm_ptr[(size_t)nloc] == slot && prow == T.n_pull_rows && term == T.n_pull_terms, "pull lists end");
        if (!knobs().pull_leaves) {
            require(T.n_pull_rows == 0 && T.n_pull_terms == 0, "HIPKKT_PULL_LEAVES=0: nothing pulled");
            for (char c : T.solve_pulled) require(c == 0, "HIPKKT_PULL_LEAVES=0: nothing pulled");
        }
    }

    // ---- packed records
    require(T.recs.empty() == (sch.rec_bytes <= 0), "records built iff laid out");
    if (!T.recs.empty()) {
        const char* base = reinterpret_cast<const char*>(T.recs.data());
        const int64_t cap = (int64_t)T.recs.size() * 8;
        require(sch.rec_bytes <= cap, "record image holds rec_bytes");
        for (size_t q = 0; q < sch.launches.size(); ++q) {
            const Launch& L = sch.launches[q];
            const bool leaf = rec_no_slots(sch.launches, q);
            RecClass classes[2];
            const int ncl = rec_classes(L, classes);
            for (int ci = 0; ci < ncl; ++ci) {
                const RecClass& c = classes[ci];
                const int fmax = L.rec.fmax[c.cls];
                const int64_t need = kSolveHdrBytes + (int64_t)fmax * 4 + (leaf ? 0 : (int64_t)fmax * 32);
                require(L.rec.stride[c.cls] >= need, "record stride holds header, idx and slots");
                for (int k = 0; k < c.count; ++k) {
                    const int64_t off = L.rec.off[c.cls] + (int64_t)k * L.rec.stride[c.cls];
                    require(off >= 0 && off + need <= sch.rec_bytes, "record inside rec_bytes");
                    const int sn = sch.sched[(size_t)(c.first + k)], nc = nc_of(sn), nb = nb_of(sn), f = nc + nb;
                    SolveHdr h;
                    std::memcpy(&h, base + off, sizeof h);
                    require(h.s == sn && h.c0 == S.sn_start[sn] && h.nc == nc && h.nb == nb && h.rp == S.rowptr[sn] && h.par == S.sn_parent[sn] &&
                            h.mat_off == (c.cls == 0 ? T.toff[(size_t)sn] : S.front_off[sn]), "record header");
                    std::vector<int> idx((size_t)fmax);
                    std::memcpy(idx.data(), base + off + kSolveHdrBytes, (size_t)fmax * 4);
                    for (int i = 0; i < f; ++i)
                        require(idx[(size_t)i] == (i < nc ? S.perm[(size_t)(h.c0 + i)] : S.rows[(size_t)(h.rp + i - nc)]), "idx = perm / rows");
                    if (leaf) {
                        // (no slots written: the bytes behind idx, up to the stride, are still zero)
                        for (int64_t b = off + kSolveHdrBytes + (int64_t)fmax * 4; b < off + L.rec.stride[c.cls]; ++b)
                            require(base[b] == 0, "no slots written where rec_no_slots holds");
                        continue;
                    }
                    const int64_t lc0 = (int64_t)h.c0 + h.rp;
                    for (int i = 0; i < fmax; ++i) {
                        int g[8];
                        std::memcpy(g, base + off + kSolveHdrBytes + (int64_t)fmax * 4 + (int64_t)i * 32, 32);
                        const int64_t g0 = i < f ? T.item_ptr[(size_t)(lc0 + i)] : 0, g1 = i < f ? T.item_ptr[(size_t)(lc0 + i + 1)] : 0;
                        require(g[0] == (int)(g1 - g0), "slot count = gather count");
                        for (int j = 0; j < 6; ++j) require(g[1 + j] == (g0 + j < g1 ? T.gsrc[(size_t)(g0 + j)] : -1), "first six sources = gsrc");
                        require(g[7] == (i < f ? (int)(g0 + 6) : 0), "seventh source's index");
                    }
                }
            }
        }
    }

    // ---- launch records and slice descriptors
    require(T.desc.size() == sch.sched.size() && T.sdesc.size() == std::max<size_t>(sch.slice_list.size(), 1), "descriptor sizes");
    require((int64_t)T.toff.size() == (int64_t)S.nsuper + 1, "toff size");
    for (size_t q = 0; q < sch.sched.size(); ++q) {
        const int s = sch.sched[q];
        const FrontDesc& d = T.desc[q];
        require(d.s == s && d.c0 == S.sn_start[s] && d.nc == nc_of(s) && d.nb == nb_of(s) && d.front_off == S.front_off[s] && d.upd_off == S.upd_off[s] &&
                d.rp == S.rowptr[s] && d.kptr == S.kptr[s] && d.nk == (int)(S.kptr[s + 1] - S.kptr[s]) && d.w_off == T.toff[(size_t)s], "launch record");
        require(d.pad == ((T.solve_pulled[(size_t)s] ? 1 : 0) | (fl.pulled[(size_t)s] ? 2 : 0)), "FrontDesc.pad bits = the two pulled flags");
    }
    for (size_t q = 0; q < sch.slice_list.size(); ++q) {
        const FrontDesc& d = T.sdesc[q];
        require(d.s == sch.slice_list[q][0] && d.pad == ((sch.slice_list[q][1] << 16) | sch.slice_list[q][2]) && d.kptr == T.slice_kptr[q] &&
                d.nk == T.slice_nk[q] && d.nc == nc_of(d.s) && d.nb == nb_of(d.s), "slice descriptor");
    }

    // ---- child cuts, ncolpar
    require((int64_t)T.cut_ptr.size() == (int64_t)S.nsuper + 1 && T.cut_ptr.back() == (int64_t)T.cuts.size() && (int)T.ncolpar.size() == S.nsuper, "cut list sizes");
    for (int c = 0; c < S.nsuper; ++c) {
        const int p = S.sn_parent[c];
        const int64_t a = T.cut_ptr[(size_t)c], b = T.cut_ptr[(size_t)c + 1];
        if (p < 0) { require(a == b && T.ncolpar[(size_t)c] == 0, "a root has no cuts"); continue; }
        require(b - a == (nb_of(p) + 63) / 64 + 1, "one cut per 64-row boundary of the parent's U");
        for (int64_t k = a; k + 1 < b; ++k) require(T.cuts[(size_t)k] <= T.cuts[(size_t)k + 1], "cuts non-decreasing");
        require(T.cuts[(size_t)a] == T.ncolpar[(size_t)c] && T.cuts[(size_t)b - 1] == nb_of(c), "first cut == ncolpar, last == nb of the child");
    }

    // ---- the rest: sizes and the diagnostics
    require((int)T.ov_ntiles.size() == S.nsuper && (int)T.ov_sbase.size() == std::max(S.nsuper, 1) && (int)T.psign.size() == S.N, "overlap table sizes");
    (void)describe_gather_sources(S, sch, T);
    (void)describe_update_blocks(S, fl);
    (void)describe_pulled_terms(fl);
    (void)describe_panel_items(S, sch, fl);
    (void)describe_tile_order(T);
    (void)describe_records(sch);
    (void)describe_solve_pulled(T);
    return T;
}

// The device tables of a KKT handle (kkt_assembly.cpp): the CSR image and the cone tables.
static void check_kkt_tables(const KKTAssembly& K)
{
    const KKTImage I = build_kkt_image(K);
    const int N = K.N;
    require((int)I.ptr.size() == N + 1 && I.ptr[0] == 0 && I.col.size() == (size_t)I.ptr[(size_t)N] && I.vmap.size() == I.col.size() &&
            (int64_t)I.col.size() == 2 * K.nnzK - N, "image sizes");
    for (int i = 0; i < N; ++i)
        for (int64_t d = I.ptr[(size_t)i]; d < I.ptr[(size_t)i + 1]; ++d) {
            require(d == I.ptr[(size_t)i] || I.col[(size_t)d - 1] < I.col[(size_t)d], "columns ascend within a row");
            const int q = I.vmap[(size_t)d], j = I.col[(size_t)d];
            require(q >= 0 && q < K.nnzK && K.rowval[(size_t)q] == std::min(i, j) && q >= K.colptr[(size_t)std::max(i, j)] && q < K.colptr[(size_t)std::max(i, j) + 1],
                    "image position maps to its K entry");
        }
    // every off-diagonal K entry has two positions, mirror images of each other; a diagonal entry one
    require((int64_t)I.kpos.size() == 2 * K.nnzK, "kpos size");
    {
        std::vector<int> row_of(I.col.size());
        for (int i = 0; i < N; ++i) for (int64_t d = I.ptr[(size_t)i]; d < I.ptr[(size_t)i + 1]; ++d) row_of[(size_t)d] = i;
        for (int j = 0; j < N; ++j)
            for (int64_t q = K.colptr[(size_t)j]; q < K.colptr[(size_t)j + 1]; ++q) {
                const int i = K.rowval[(size_t)q], a = I.kpos[2 * (size_t)q], b = I.kpos[2 * (size_t)q + 1];
                require(a >= 0 && (size_t)a < I.col.size() && I.vmap[(size_t)a] == (int)q, "kpos first slot");
                if (i == j) { require(b == -1 && row_of[(size_t)a] == j && I.col[(size_t)a] == j, "a diagonal entry has one position"); continue; }
                require(b >= 0 && (size_t)b < I.col.size() && b != a && I.vmap[(size_t)b] == (int)q, "an off-diagonal entry has two positions");
                require(row_of[(size_t)a] == I.col[(size_t)b] && row_of[(size_t)b] == I.col[(size_t)a] &&
                        std::min(row_of[(size_t)a], row_of[(size_t)b]) == i && std::max(row_of[(size_t)a], row_of[(size_t)b]) == j, "the two positions mirror each other");
            }
    }
    require(I.pend.size() == (size_t)std::max(K.n, 1), "pend size");
    for (int i = 0; i < K.n; ++i) {
        const int64_t e = I.pend[(size_t)i];
        require(e >= I.ptr[(size_t)i] && e <= I.ptr[(size_t)i + 1] && (e == I.ptr[(size_t)i] || I.col[(size_t)e - 1] < K.n) &&
                (e == I.ptr[(size_t)i + 1] || I.col[(size_t)e] >= K.n), "pend is the first column >= n");
    }
    require(I.long_chunk_ptr.size() == I.long_rows.size() + 1 && I.long_chunk_ptr[0] == 0 && I.chunk_q.size() % 2 == 0 &&
            I.long_chunk_ptr.back() == (int64_t)I.chunk_q.size() / 2, "long-row list sizes");
    {
        size_t r = 0;
        for (int i = 0; i < N; ++i) {
            if (I.ptr[(size_t)i + 1] - I.ptr[(size_t)i] <= kLongRow) continue;
            require(r < I.long_rows.size() && I.long_rows[r] == i, "every long row listed, in order");
            int64_t at = I.ptr[(size_t)i];
            for (int64_t k = I.long_chunk_ptr[r]; k < I.long_chunk_ptr[r + 1]; ++k) {
                require(I.chunk_q[2 * (size_t)k] == at && I.chunk_q[2 * (size_t)k + 1] > at && I.chunk_q[2 * (size_t)k + 1] - at <= kLongChunk, "chunks follow each other");
                at = I.chunk_q[2 * (size_t)k + 1];
            }
            require(at == I.ptr[(size_t)i + 1], "the chunks cover a long row exactly once");
            ++r;
        }
        require(r == I.long_rows.size(), "only long rows listed");
    }
    require(I.lanes_per_row == 8 || I.lanes_per_row == 64, "lanes_per_row");

    const ConeTables C = build_cone_tables(K);
    const size_t nc = K.cones.size();
    require(C.kind.size() == nc && C.off.size() == nc && C.numel.size() == nc && C.boff.size() == nc && C.sidx.size() == nc && C.soff.size() == nc &&
            C.ns_index.size() == nc && C.param.size() == nc && C.psd_dim.size() == nc && C.psd_aoff.size() == nc && (int)C.elem_cone.size() == K.m, "cone table sizes");
    {
        int at = 0;
        for (size_t c = 0; c < nc; ++c) {
            require(C.off[c] == at && C.numel[c] >= 0, "cones tile [0, m)");
            for (int t = 0; t < C.numel[c]; ++t) require(C.elem_cone[(size_t)(at + t)] == (int)c, "elem_cone consistent with off / numel");
            at += C.numel[c];
        }
        require(at == K.m, "elem_cone covers [0, m)");
    }
    // every list holds exactly the cones of its kind and class, in cone order
    auto holds = [&](const std::vector<int>& list, const char* what, auto&& member) {
        size_t k = 0;
        for (size_t c = 0; c < nc; ++c)
            if (member(K.cones[c])) { require(k < list.size() && list[k] == (int)c, what); ++k; }
        require(k == list.size(), what);
    };
    holds(C.soc_list, "soc_list", [](const ConeInfo& ci) { return ci.kind == HIPKKT_CONE_SOC; });
    holds(C.exp_list, "exp_list", [](const ConeInfo& ci) { return ci.kind == HIPKKT_CONE_EXP; });
    holds(C.pow_list, "pow_list", [](const ConeInfo& ci) { return ci.kind == HIPKKT_CONE_POW; });
    holds(C.psd_list, "psd_list", [](const ConeInfo& ci) { return ci.kind == HIPKKT_CONE_PSD && ci.dim <= kPsdMaxDim; });
    holds(C.psdb_list, "psdb_list", [](const ConeInfo& ci) { return ci.kind == HIPKKT_CONE_PSD && ci.dim > kPsdMaxDim; });
    holds(C.gp_cone, "gp_cone", [](const ConeInfo& ci) { return ci.kind == HIPKKT_CONE_GENPOW; });
    {
        std::vector<int> small, big;             // (these two list a cone's index among the generalized power cones)
        for (size_t k = 0; k < C.gp_cone.size(); ++k) {
            const ConeInfo& ci = K.cones[(size_t)C.gp_cone[k]];
            require(ci.gpidx == (int)k && C.gp_dim1[k] == ci.dim1 && C.gp_off[k] == ci.gpoff, "generalized power cone tables");
            (ci.numel <= kGenPowWaveMax ? small : big).push_back((int)k);
        }
        require(C.gp_small == small && C.gp_big == big && (int)C.gp_cone.size() == K.ngenpow, "gp_small / gp_big by size class");
        require(C.gp_cone.empty() || ((int)C.gp_mapQR.size() == K.genpow_len && (int)C.gp_alpha.size() == K.genpow_len), "generalized power map sizes");
    }
    bool has = false, big = false;
    int kmax = 1, bkmax = 1;
    int64_t ao = 0;
    for (size_t c = 0; c < nc; ++c) {
        const ConeInfo& ci = K.cones[c];
        if (ci.kind != HIPKKT_CONE_PSD) { require(C.psd_dim[c] == 0, "psd_dim of another kind"); continue; }
        has = true;
        require(C.psd_dim[c] == ci.dim && C.psd_aoff[c] == ao, "PSD matrix offsets");
        ao += (int64_t)ci.dim * ci.dim;
        if (ci.dim > kPsdMaxDim) { big = true; bkmax = std::max(bkmax, ci.dim); } else kmax = std::max(kmax, ci.dim);
    }
    require(C.has_psd == has && C.psd_too_big == big && C.psd_kmax == kmax && C.psdb_kmax == bkmax && C.psd_store == ao, "PSD flags and maxima");
}

// --plans: what the engine prints for its sweeps under HIPKKT_VERBOSE=2, for one pattern in its natural order
static void print_plans(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    const auto h = rd<int64_t>(f, 2);
    const auto colptr = rd<int64_t>(f, (size_t)h[0] + 1), rowval = rd<int64_t>(f, (size_t)h[1]);
    std::fclose(f);
    SymbolicOptions opt;
    opt.ordering = ORDER_NATURAL;
    apply_knobs(opt);
    Symbolic S;
    analyse((int)h[0], colptr.data(), rowval.data(), 0, opt, S);
    const DeviceLimits dev = fixed_limits();
    const Schedule sch = build_schedule(S, dev, opt.panel_cap, std::max(1, opt.panel_max_slices));
    check_schedule(S, sch, dev);
    (void)check_tables(S, sch);
    std::printf("@@case %s launches %zu\n", path, sch.launches.size());
    NrGrids grids;
    // a claimed sweep with W still pending and in the steady state, then the unclaimed sweeps of 1, 2 and 4 columns
    for (int k = 0; k < 5; ++k) {
        const int nr = k < 3 ? 1 : (k == 3 ? 2 : 4);
        if (!supports_nr(sch, nr)) continue;
        const SweepState st{k < 2, k < 2, false, false, k == 0};
        const SweepPlan p = plan_sweep(sch, st, nr, dev, grids);
        if (p.split_columns) continue;
        if (k == 0 || k == 2) std::printf("@@%s\n", k == 0 ? "claimed" : "unclaimed");
        std::printf("[hipkkt] sweep plan: %s\n%s", describe(p, sch, nr, st.w_pending, sch.rec_bytes > 0).c_str(), describe_launches(p, sch).c_str());
    }
}

// --launches: the launch schedule of one pattern in its natural order -- "L q level small count" per launch and
// "S sn c0 nc nb parent nchildren launch rel..." per supernode (rel: its rows' positions in the parent's front)
static void print_launches(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    const auto h = rd<int64_t>(f, 2);
    const auto colptr = rd<int64_t>(f, (size_t)h[0] + 1), rowval = rd<int64_t>(f, (size_t)h[1]);
    std::fclose(f);
    SymbolicOptions opt;
    opt.ordering = ORDER_NATURAL;
    apply_knobs(opt);
    Symbolic S;
    analyse((int)h[0], colptr.data(), rowval.data(), 0, opt, S);
    const DeviceLimits dev = fixed_limits();
    const Schedule sch = build_schedule(S, dev, opt.panel_cap, std::max(1, opt.panel_max_slices));
    check_schedule(S, sch, dev);
    const EngineTables T = check_tables(S, sch);
    std::printf("@@case %s launches %zu\n", path, sch.launches.size());
    std::vector<int> launch_of((size_t)S.nsuper, -1);
    for (size_t q = 0; q < sch.launches.size(); ++q) {
        const Launch& L = sch.launches[q];
        std::printf("L %zu %d %d %d\n", q, L.level, L.small ? 1 : 0, L.count);
        for (int t = L.begin; t < L.begin + L.count; ++t) launch_of[(size_t)sch.sched[(size_t)t]] = (int)q;
    }
    for (int sn = 0; sn < S.nsuper; ++sn) {
        // (c0 in the caller's numbering: the postorder may move siblings)
        std::printf("S %d %d %d %d %d %d %d", sn, S.perm[(size_t)S.sn_start[sn]], S.sn_start[sn + 1] - S.sn_start[sn], (int)(S.rowptr[sn + 1] - S.rowptr[sn]),
                    S.sn_parent[sn], (int)(S.child_ptr[sn + 1] - S.child_ptr[sn]), launch_of[(size_t)sn]);
        for (int64_t q = S.rowptr[sn]; q < S.rowptr[sn + 1]; ++q) std::printf(" %d", S.rel[q]);
        std::printf("\n");
    }
    for (int sn = 0; sn < S.nsuper; ++sn) std::printf("P %d %d\n", sn, T.solve_pulled[(size_t)sn] ? 1 : 0);
    std::printf("M %lld %lld %d\n", (long long)T.n_pull_terms, (long long)T.item_ptr.back(), T.n_pull_rows);
    std::printf("D %d %lld\n", T.dealt_launches, (long long)T.dealt_tiles);
}

int main(int argc, char** argv)
{
    try {
        if (argc > 1 && !std::strcmp(argv[1], "--launches")) {
            for (int a = 2; a < argc; ++a) print_launches(argv[a]);
            return 0;
        }
        if (argc > 1 && !std::strcmp(argv[1], "--multi-shape")) {
            // the many-column sweeps' instances (launch_shapes.hpp: multi_shape) under the knobs of this process
            for (int a = 2; a < argc; ++a) {
                const int KP = std::atoi(argv[a]);
                const MultiShape ms = multi_shape(KP, knobs().multi_vec, knobs().multi_ct);
                std::printf("KP %d wave_v %d leaf_v %d block_bs %d block_ct %d\n", KP, ms.wave_v, ms.leaf_v, ms.block_bs, ms.block_ct);
            }
            return 0;
        }
        if (argc > 1 && !std::strcmp(argv[1], "--plans")) {
            for (int a = 2; a < argc; ++a) print_plans(argv[a]);
            return 0;
        }
        for (int a = 1; a < argc; ++a) {
            FILE* f = std::fopen(argv[a], "rb");
            if (!f) { std::perror(argv[a]); return 2; }
            const auto h = rd<int64_t>(f, 6);
            const int64_t n = h[0], m = h[1], nc = h[2], nnzP = h[3], nnzA = h[4];
            const auto Pp = rd<int64_t>(f, n + 1), Pi = rd<int64_t>(f, nnzP);
            const auto Px = rd<double>(f, nnzP);
            const auto Ap = rd<int64_t>(f, n + 1), Ai = rd<int64_t>(f, nnzA);
            const auto Ax = rd<double>(f, nnzA);
            const auto kinds = rd<int32_t>(f, nc);
            const auto dims = rd<int64_t>(f, nc);
            std::fclose(f);

            KKTAssembly K;
            assemble_kkt(n, m, Pp.data(), Pi.data(), Px.data(), Ap.data(), Ai.data(), Ax.data(), nc, kinds.data(), dims.data(), 0, K);
            require(K.N == K.n + K.m + K.p && (int64_t)K.colptr.size() == (int64_t)K.N + 1 && K.colptr[K.N] == K.nnzK, "KKT shape");
            require((int64_t)K.mapP.size() == nnzP && (int64_t)K.mapA.size() == nnzA && (int)K.map_diag.size() == K.N, "map sizes");
            for (int64_t j = 0; j < K.N; ++j)
                for (int64_t q = K.colptr[j]; q < K.colptr[j + 1]; ++q)
                    require(K.rowval[q] >= 0 && K.rowval[q] <= j && (q == K.colptr[j] || K.rowval[q - 1] < K.rowval[q]), "triu, sorted columns");
            for (int v : K.mapP) require(v >= 0 && v < K.nnzK, "mapP range");
            for (int v : K.mapA) require(v >= 0 && v < K.nnzK, "mapA range");
            for (int v : K.mapHs) require(v >= 0 && v < K.nnzK, "mapHs range");
            for (int j = 0; j < K.N; ++j) require(K.rowval[K.map_diag[j]] == j && K.map_diag[j] == K.colptr[j + 1] - 1, "map_diag");
            for (int v : K.mapU) require(v >= 0 && v < K.nnzK, "mapU range");
            for (int v : K.mapV) require(v >= 0 && v < K.nnzK, "mapV range");
            for (int v : K.mapD) require(v >= 0 && v < K.nnzK, "mapD range");
            for (int s : K.dsigns) require(s == 1 || s == -1, "dsigns");
            check_kkt_tables(K);

            std::vector<int64_t> rowval(K.rowval.begin(), K.rowval.end());
            for (int ordering : {ORDER_ND, ORDER_AMD, ORDER_NATURAL}) {
                if (ordering == ORDER_NATURAL && K.N > 30000) continue;
                SymbolicOptions opt;
                opt.ordering = ordering;
                if (h[5] > 0) opt.nd_leaf_size = (int)h[5];
                Symbolic S;
                analyse(K.N, K.colptr.data(), rowval.data(), 0, opt, S);
                require(S.N == K.N && (int)S.perm.size() == K.N && (int)S.iperm.size() == K.N, "perm size");
                for (int j = 0; j < K.N; ++j) require(S.perm[j] >= 0 && S.perm[j] < K.N && S.iperm[S.perm[j]] == j, "perm is a permutation");
                require((int)S.sn_start.size() == S.nsuper + 1 && S.sn_start[0] == 0 && S.sn_start[S.nsuper] == K.N, "supernode partition");
                int seen = 0;
                for (size_t l = 0; l < S.levels.size(); ++l)
                    for (int t = S.levels[l].begin; t < S.levels[l].end; ++t, ++seen) {
                        const int sn = S.level_sn[t];
                        require(sn >= 0 && sn < S.nsuper && S.sn_level[sn] == (int)l, "level lists");
                        const int par = S.sn_parent[sn];
                        require(par == -1 || (par > sn && S.sn_level[par] > (int)l), "parents later and higher");
                        const int fp = par < 0 ? 0 : (S.sn_start[par + 1] - S.sn_start[par]) + (int)(S.rowptr[par + 1] - S.rowptr[par]);
                        for (int64_t q = S.rowptr[sn]; q < S.rowptr[sn + 1]; ++q) {
                            require(S.rows[q] >= S.sn_start[sn + 1] && S.rows[q] < K.N && (q == S.rowptr[sn] || S.rows[q - 1] < S.rows[q]), "row structure");
                            require(par >= 0 && S.rel[q] >= 0 && S.rel[q] < fp, "relative indices inside the parent's front");
                        }
                    }
                require(seen == S.nsuper, "every supernode scheduled once");
                const DeviceLimits dev = fixed_limits();
                const Schedule sch = build_schedule(S, dev, opt.panel_cap, std::max(1, opt.panel_max_slices));
                check_schedule(S, sch, dev);
                (void)check_tables(S, sch);
                std::printf("%s ordering %d: N %d nnzK %lld supernodes %d levels %zu nnzL_stored %lld max_front %d launches %zu overlap %zu "
                            "late %zu persistent %zu chained %zu tasks %d\n", argv[a], ordering, K.N,
                            (long long)K.nnzK, S.nsuper, S.levels.size(), (long long)S.nnzL, S.max_front, sch.launches.size(),
                            sch.launches.size() - sch.ov_first, sch.late_launches, sch.top_launches,
                            sch.launches.size() - std::min(sch.launches.size(), sch.chain_from), sch.top_ntask);
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "host_driver: %s\n", e.what());
        return 1;
    }
    std::printf("HOST SANITIZER DRIVER OK\n");
    return 0;
}
