// Sanitizer driver for the HOST side of the product (set-up only code: csrc/kkt_assembly.cpp, csrc/ordering.cpp,
// csrc/symbolic.cpp, csrc/schedule.cpp), built by tests/test_host_sanitizers.py with g++ -fsanitize=address,undefined (the
// GPU box offers no AddressSanitizer; the kernels are covered by the parity suite, the host code by this).  No HIP, no device.
//
// Input file (little-endian): int64 n, m, ncones, nnzP, nnzA, nd_leaf_size; int64 Pp[n+1], Pi[nnzP]; double Px[nnzP];
// int64 Ap[n+1], Ai[nnzA]; double Ax[nnzA]; int32 kinds[ncones]; int64 dims[ncones].
// For each file and ordering: assemble the KKT pattern and its maps, check the maps against the pattern, run the
// symbolic analysis, check the permutation and the level lists, build the launch schedule and the sweep plans
// (schedule.cpp) and check them, print one line.
//
// host_driver --plans FILE...: FILE holds one triu CSC pattern (int64 N, nnz; int64 colptr[N+1], rowval[nnz]); it is
// analysed in its natural order, as the tests' forests are, and the sweep-plan lines of HIPKKT_VERBOSE=2 are printed
// for it as the engine prints them -- under the HIPKKT_* knobs of this process (tests/test_schedule_host.py; built
// without sanitizers there).
//
// host_driver --multi-shape KP...: one line per padded column count with the kernel instances the many-column sweeps take
// (launch_shapes.hpp: multi_shape) under HIPKKT_MULTI_VEC / HIPKKT_MULTI_CT of this process (tests/test_multi_sweeps_host.py).
// host_driver --launches FILE...: per pattern (as for --plans) one line per launch and one per supernode, for the tests
// that reason about which fronts the many-column sweeps pull (tests/test_multi_sweeps_host.py).
#include "kkt_assembly.hpp"
#include "knobs.hpp"
#include "launch_shapes.hpp"
#include "schedule.hpp"
#include "symbolic.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
