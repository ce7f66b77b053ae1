// Dumps the factorisation's extend-add work lists (csrc/schedule.cpp: build_factor_lists) of triu CSC patterns as text,
// for tests/test_pulled_leaf_lists_host.py.  Host code only: no HIP, no device; the schedule is that of a fixed device
// (256 CUs, 240 resident workgroups), under the HIPKKT_* knobs of this process.
//
// pulled_lists_driver ORDERING FILE...: FILE holds int64 N, nnz; int64 colptr[N+1], rowval[nnz]; ORDERING is 1 (nested
// dissection) or 2 (natural).  Per file:
//   @@case FILE nsuper ntiles nchunks
//   S s c0 nc nb parent pulled tile_base in_small_launch sliced front_off first_child_entry..   one per supernode
//   REL s rel...            parent-local rows of s's rows below
//   CH p children...        in the order the lists walk them
//   W s spw wcol[17] pwcut[17]  block-class fronts: slice w owns columns [wcol[w], wcol[w+1]); the spw slices of one wave walk
//                               chunks [pwcut[g], pwcut[g+spw]), g their first
//   T t s ti tj tcol[5] ptcut[5]
//   I s tcol relstart cnt   a panel item of front s
//   U t qcol relstart cnt   a sub-item of tile t
//   P chunk lane leaf_off target a b steps     a pulled term (steps: lane 0's count of doubling steps for the chunk)
//   WC s base wcut[17]      the panel items' 16 wave slices as item indices; front s's I lines count from `base`
//   TC t base tcut[5]       a tile's four wave shares as sub-item indices; tile t's U lines count from `base`
//   SL q s sl nsl wcut[17]  row slice sl of nsl of the sliced front s: the 16 wave slices of its own item list ...
//   J q tcol relstart cnt rfirst rlast         ... and that list's items, in order from wcut[0]
#include "schedule.hpp"
#include "symbolic.hpp"

#include <cstdio>
#include <cstdlib>
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

static void dump(const char* path, int ordering)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    const auto h = rd<int64_t>(f, 2);
    const auto colptr = rd<int64_t>(f, (size_t)h[0] + 1), rowval = rd<int64_t>(f, (size_t)h[1]);
    std::fclose(f);
    SymbolicOptions opt;
    opt.ordering = ordering;
    apply_knobs(opt);
    Symbolic S;
    analyse((int)h[0], colptr.data(), rowval.data(), 0, opt, S);
    DeviceLimits dev;
    dev.n_cus = 256;
    dev.top_solve_capacity = [](size_t, bool) { return 240; };
    dev.top_solve_capacity_nr = [](size_t, int) { return 240; };
    dev.top_solve_sliced_capacity = [](size_t, int) { return 240; };
    const Schedule sch = build_schedule(S, dev, opt.panel_cap, std::max(1, opt.panel_max_slices));
    const FactorLists fl = build_factor_lists(S, sch);
    const int64_t ntile = (int64_t)sch.tiles.size();
    std::printf("@@case %s %d %lld %zu\n", path, S.nsuper, (long long)ntile, fl.pterms.size() / 64);
    std::vector<char> in_small((size_t)S.nsuper, 0), sliced((size_t)S.nsuper, 0);
    for (const Launch& L : sch.launches)
        if (L.small) for (int t = L.begin; t < L.begin + L.count; ++t) in_small[(size_t)sch.sched[(size_t)t]] = 1;
    for (const auto& sl : sch.slice_list) sliced[(size_t)sl[0]] = 1;
    for (int s = 0; s < S.nsuper; ++s) {
        std::printf("S %d %d %d %d %d %d %lld %d %d %lld\n", s, S.sn_start[s], S.sn_start[s + 1] - S.sn_start[s], (int)(S.rowptr[s + 1] - S.rowptr[s]),
                    S.sn_parent[s], (int)fl.pulled[(size_t)s], (long long)sch.tile_base[s], (int)in_small[(size_t)s], (int)sliced[(size_t)s],
                    (long long)S.front_off[s]);
        std::printf("REL %d %lld", s, (long long)S.rowptr[s]);
        for (int64_t q = S.rowptr[s]; q < S.rowptr[s + 1]; ++q) std::printf(" %d", S.rel[(size_t)q]);
        std::printf("\nCH %d", s);
        for (int e = S.child_ptr[s]; e < S.child_ptr[s + 1]; ++e) std::printf(" %d", S.child_idx[e]);
        std::printf("\n");
        if (sch.tile_base[s] >= 0) {
            std::printf("W %d %d", s, fl.spw[(size_t)s]);
            for (int w = 0; w <= 16; ++w) std::printf(" %d", fl.wcol[(size_t)s * 17 + w]);
            for (int w = 0; w <= 16; ++w) std::printf(" %d", fl.pwcut[(size_t)s * 17 + w]);
            std::printf("\n");
        }
        if (sch.tile_base[s] >= 0) {
            std::printf("WC %d %lld", s, (long long)fl.pptr[(size_t)S.sn_start[s]]);
            for (int w = 0; w <= 16; ++w) std::printf(" %lld", (long long)fl.wcut[(size_t)s * 17 + w]);
            std::printf("\n");
        }
        for (int64_t it = fl.pptr[(size_t)S.sn_start[s]]; it < fl.pptr[(size_t)S.sn_start[s + 1]]; ++it)
            std::printf("I %d %d %d %d\n", s, fl.items[(size_t)it].tcol, fl.items[(size_t)it].relstart, fl.items[(size_t)it].cnt);
    }
    for (int64_t t = 0; t < ntile; ++t) {
        const uint64_t v = (uint64_t)sch.tiles[(size_t)t];
        const int s = (int)(uint32_t)v, y = (int)(v >> 32);
        std::printf("T %lld %d %d %d", (long long)t, s, y >> 16, y & 0xffff);
        for (int w = 0; w <= 4; ++w) std::printf(" %d", fl.tcol[(size_t)(t * 5 + w)]);
        for (int w = 0; w <= 4; ++w) std::printf(" %d", fl.ptcut[(size_t)(t * 5 + w)]);
        std::printf("\n");
        std::printf("TC %lld %lld", (long long)t, (long long)fl.tptr[(size_t)(t * 64)]);
        for (int w = 0; w <= 4; ++w) std::printf(" %lld", (long long)fl.tcut[(size_t)(t * 5 + w)]);
        std::printf("\n");
        for (int64_t it = fl.tptr[(size_t)(t * 64)]; it < fl.tptr[(size_t)(t * 64 + 64)]; ++it)
            std::printf("U %lld %d %d %d\n", (long long)t, (int)fl.sit[(size_t)it].qcol, fl.sit[(size_t)it].relstart, (int)fl.sit[(size_t)it].cnt);
    }
    for (size_t q = 0; q < sch.slice_list.size(); ++q) {
        const int64_t* w = fl.wcut.data() + ((size_t)S.nsuper + q) * 17;
        std::printf("SL %zu %d %d %d", q, sch.slice_list[q][0], sch.slice_list[q][1], sch.slice_list[q][2]);
        for (int k = 0; k <= 16; ++k) std::printf(" %lld", (long long)w[k]);
        std::printf("\n");
        for (int64_t it = w[0]; it < w[16]; ++it) {
            const ExtItem& e = fl.items[(size_t)it];
            std::printf("J %zu %d %d %d %d %d\n", q, e.tcol, e.relstart, e.cnt, e.rfirst, e.rlast);
        }
    }
    for (size_t k = 0; k < fl.pterms.size(); ++k) {
        const PullTerm& t = fl.pterms[k];
        if (t.tgt_ab == kPullNone) continue;
        std::printf("P %zu %zu %u %u %u %u %u\n", k / 64, k % 64, t.leaf_off, t.tgt_ab & 0x7fff, (t.tgt_ab >> 15) & 63, (t.tgt_ab >> 21) & 63,
                    (t.tgt_ab >> 27) & 7);
    }
}

int main(int argc, char** argv)
{
    try {
        if (argc < 3) throw std::runtime_error("usage: pulled_lists_driver ORDERING FILE...");
        for (int a = 2; a < argc; ++a) dump(argv[a], std::atoi(argv[1]));
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "pulled_lists_driver: %s\n", e.what());
        return 1;
    }
}
