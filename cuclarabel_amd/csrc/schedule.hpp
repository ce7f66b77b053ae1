// Everything the numeric engine DECIDES, as host-only code (no HIP header, no device): which fronts form a launch, which
// launches are overlapped, chained or persistent (build_schedule), where a launch's packed sweep records lie
// (layout_records) and how one sweep is split (plan_sweep).  The device contributes one integer and three occupancy
// answers (DeviceLimits); the engine (hipkkt.hip) executes what is decided here: it allocates, uploads and launches.
// (The device tables that follow from these decisions: engine_tables.hpp.)
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "knobs.hpp"
#include "launch_shapes.hpp"
#include "symbolic.hpp"

namespace hipkkt {

// the panel-shape settings of knobs.hpp over SymbolicOptions' defaults
inline void apply_knobs(SymbolicOptions& opt)
{
    if (knobs().panel_cap >= 0) opt.panel_cap = knobs().panel_cap;
    if (knobs().panel_max_cols >= 0) opt.panel_max_cols = knobs().panel_max_cols;
    if (knobs().panel_slice_below >= 0) opt.panel_slice_below = knobs().panel_slice_below;
}

inline int front_size(const Symbolic& S, int s)
{
    return (S.sn_start[s + 1] - S.sn_start[s]) + (int)(S.rowptr[s + 1] - S.rowptr[s]);
}

// What the device contributes to the schedule.  The three callables answer how many workgroups of a persistent kernel the
// device keeps resident (solve_kernels.hip: top_solve_capacity, top_solve_capacity_nr, top_solve_sliced_capacity); each is
// asked only where a schedule needs it (the NR-column one at most once per nr: top_grid_for).
struct DeviceLimits {
    int n_cus = 256;
    std::function<int(size_t lds, bool tall)> top_solve_capacity;
    std::function<int(size_t lds_total, int nr)> top_solve_capacity_nr;
    std::function<int(size_t lds, int nr)> top_solve_sliced_capacity;
};

struct Launch {
    int begin, count;
    bool small;                 // one wave per front
    int bs_panel, nbk, slice;   // panel kernel block size / block-column width; small-front LDS slice
    size_t lds_panel, lds_solve;
    int fmax, ncmax;            // largest front / column count in the launch
    int solve_bs;               // workgroup size of the block solve kernels for this launch (128 or 256 = the default 512-thread one)
    int ntiny;                  // one-wave launches: the last ntiny fronts have f <= 8 (eight to a wave in the solves)
    int tile_begin, ntiles;     // Schur tiles of this launch's fronts
    int tile_nc = 0;            // panel columns per tile, averaged over the launch's tiles (the depth of a tile's product)
    int tinv_begin, tinv_count, tinv_ncmax;   // this launch's supernodes that need T = L11^{-1}
    int nsliced;                // the last nsliced fronts of a block-class launch are factorised in row slices ...
    int slice_begin, slice_count;   // ... their slice records in d_sdesc
    size_t lds_sliced;
    int ntall;                  // the last ntall fronts of a block-class launch are too tall for the block sweep kernels' LDS
                                //   (beyond ~10 000 rows): k_fwd_tall / k_bwd_tall; such a launch stays out of the persistent kernels
    int level;                  // tree level: a level has at most one block-class launch, followed by its one-wave launch
    RecSeg rec;                 // packed sweep records of the launch's fronts (kernels.hpp): class 0 for a block-class launch, 1 and 2 for a one-wave one
};

// overlap mode: runs of consecutive launches whose panels go out as ONE kernel each (build_schedule: overlap admission)
struct MergeGroup {
    size_t first, end;           // launches [first, end)
    int count;                   // panel workgroups of the kernel (whole fronts, or row slices: sliced)
    size_t lds;
    bool sliced;
};

struct Schedule {
    std::vector<Launch> launches;
    std::vector<int> sched;           // supernodes in launch order
    std::vector<int> spos;            // per supernode: its position in sched
    std::vector<int64_t> tiles;       // int2 {supernode, ti<<16|tj}
    std::vector<int64_t> tile_base;   // per supernode: index of its first tile in `tiles` (-1: none)
    std::vector<int> tinv_list, tinv_small_prefix;
    int tinv_ncmax = 1;
    std::vector<std::array<int, 3>> slice_list;   // (supernode, slice, slices) in launch order
    // overlap mode of the factorisation (factor_kernels.hip): the launches from ov_first on (the narrow top of the tree)
    size_t ov_first = 0;         // == launches.size(): none
    std::vector<MergeGroup> ov_groups;        // in launch order
    std::vector<int> ov_group_of;             // per launch: index into ov_groups, -1 = a kernel of its own
    // grid of the side-stream W formation while the tree is still being factorised: 3/8 of the CUs (96 of 256) unless set
    int side_winv_blocks = 96;
    // the narrow top of the tree, whose W is formed behind the factorisation
    size_t late_launches = 0;
    int late_count = 0;
    // persistent solve set
    size_t top_launches = 0, top_lds = 0;
    int top_count = 0, top_grid = 0;
    bool top_tall = true;        // the persistent kernel's 1024-thread build (default) or its 512-thread one
    int top_ntask = 0, top_nflag = 0, top_sgrid = 0, top_sgrid2 = 0;
    size_t top_slds = 0;
    std::vector<int> h_tbase;    // per position of the set: its first (front, slice) task
    std::vector<int> tp, ts;     // tasks of k_top_solve_sliced (SolveArgs::tk_*); empty unless the set has sliced fronts
    // chained launches (chain_kernels.hip)
    size_t chain_from = ~(size_t)0;  // first chained launch (>= launches.size(): none)
    size_t chain_lds = 0;            // LDS of the largest block-class front in the chained launches, per right-hand side
    std::vector<int> nch;            // per supernode: its children in chained launches (the ones that count themselves in)
    // packed sweep records (layout_records): their bytes (0: the legacy layout) and, where HIPKKT_PACKED_MAX_MB refused
    // them, what they would have taken
    int64_t rec_bytes = 0, rec_refused_bytes = 0;
};

// Today's whole schedule of one structure.  Throws std::runtime_error where a front fits no kernel.
Schedule build_schedule(const Symbolic& S, const DeviceLimits& dev, int64_t panel_cap, int panel_max_slices);

// ---- the factorisation's extend-add work lists (walked by k_panel and k_schur; the records: launch_shapes.hpp)
// Panel items: the pieces of child update columns that land in a panel column, grouped by column, children in fixed
// order, cut into 16 wave slices of whole columns per front (wcut).  Schur sub-items: the same for the columns of U, per
// (tile, tile column), cut into four wave slices per tile (tcut).  A dense child (HIPKKT_DENSE_CHILD) is in neither list.
//
// PULLED LEAVES (HIPKKT_PULL_FACTOR_LEAVES, default on).  A front is a pulled leaf iff it has one column, no children
// and a parent, sits in a one-wave launch (k_front_wave / k_front_tiny factorise it), and its parent is a block-class
// front that is not cut into row slices.  Such a leaf stores no update block and has no items or sub-items: the parent
// forms U(a, b) = -(l_a d) l_b itself, one PullTerm per entry a >= b.  The terms one wave walks -- those of its wave
// slices of the panel, or of its share of a tile's columns -- are sorted by target, a target's terms in child order,
// and packed into chunks of 64 lanes.  Many leaves hit one entry (cfg2: stacks of up to 53), so the kernel sums a run of
// equal targets in registers first (a segmented scan over the lanes) and the run's last lane adds the sum to LDS:
// no two lanes of one LDS add instruction address the same target, and the order of additions into every target is a
// fixed function of the list -- within a chunk the scan's tree over the run, chunk after chunk in list order.
// (Neither of the two plainer layouts: "round k holds every target's k-th term" was built first and measured -- 1.62 M
// terms took 224 k chunks, seven terms per wave-wide load, and a panel wave behind a stack of 49 walked 49 of them;
// "one lane sums its target's terms in a loop" has the same number of load rounds.  Runs fill the lanes.)
// wcut / tcut balance 64 x pieces + terms per column; a front or tile without pulled terms is cut exactly as before.
struct FactorLists {
    std::vector<char> pulled;            // per supernode: a pulled leaf
    std::vector<int> dense_child;        // per supernode: its dense child, -1: none
    std::vector<int64_t> dense_off;      // ... and that child's update-block offset
    std::vector<int64_t> pptr;           // N + 1: first item of every (permuted) panel column
    std::vector<ExtItem> items;          // whole fronts first, then the row slices' own lists (sch.slice_list order)
    std::vector<int64_t> wcut;           // (nsuper + row slices) x 17
    std::vector<int> wcol;               // nsuper x 17: the panel columns the whole fronts' slices are cut at (slice w: columns [wcol[w], wcol[w + 1]))
    std::vector<int64_t> tptr;           // tiles x 64 + 1: first sub-item of every tile column (sch.tiles order)
    std::vector<SubItem> sit;
    std::vector<int64_t> tcut;           // tiles x 5 (+ 5)
    std::vector<int> tcol;               // tiles x 5 (+ 5): the tile columns the waves are cut at
    std::vector<PullTerm> pterms;        // chunks of 64: the fronts' wave slices in (supernode, slice) order, then the tiles' waves
    std::vector<int> spw;                // per supernode: wave slices per wave of the panel kernel its launch uses (1, 2 or 4): their terms are one list
    std::vector<int> pwcut;              // nsuper x 17: chunk range of wave slice w of front s is [pwcut[17 s + w], pwcut[17 s + w + 1])
    std::vector<int> ptcut;              // tiles x 5 (+ 5): the same per tile wave
    int64_t n_pulled = 0, n_terms = 0, n_stacked = 0;     // leaves, terms, terms onto a target another term already hit
    int max_depth = 0;                                     // deepest stack of terms on one target
};
FactorLists build_factor_lists(const Symbolic& S, const Schedule& sch);
// diagnostic (HIPKKT_DUMP_LEVELS): the "[pieces]" lines -- per parent level the tile and panel pieces, their entries and
// lengths, what the pulled leaves took out of them and how deep their terms stack
std::string describe_pieces(const Symbolic& S, const Schedule& sch, const FactorLists& fl);

// Packed sweep records (kernels.hpp: SolveHdr / RecSeg): per launch and size class one record size, so that a
// kernel finds a front's record from its place in the launch and fetches header and row slots in one round of loads.
// HIPKKT_PACKED=0, or more than HIPKKT_PACKED_MAX_MB (4096) of records -- a wide level with one very tall front pays
// that front's height for every front --: the legacy layout.  Fills Launch::rec; -> the records' bytes (0: legacy
// layout; *refused: the bytes the limit refused).
int64_t layout_records(std::vector<Launch>& launches, int64_t* refused = nullptr);
struct RecClass { int first, count, cls; };      // schedule positions [first, first + count) of size class cls
int rec_classes(const Launch& L, RecClass out[2]);
// no gather slots for the one-wave launch of tree level 0 (its fronts have no children, and its kernels are told
// so: `leaf`) -- unless a block-class launch of that level sits in front of it: the two may then go out as one
// level kernel, whose one-wave bodies read the slots
inline bool rec_no_slots(const std::vector<Launch>& launches, size_t q)
{
    const Launch& L = launches[q];
    return L.small && L.level == 0 && !(q > 0 && !launches[q - 1].small && launches[q - 1].level == 0);
}

// The single-column kernels' NR-column instances keep NR times the vectors in LDS: possible when every level's
// share still fits a CU (the (front, slice) kernel of sets with very tall fronts: two columns at most).
bool supports_nr(const Schedule& sch, int nr);

// ---- one sweep
// use_top: the persistent kernel may be used (claimed); allow_chain: the caller reads the abort word afterwards and
// repeats the solve if a bounded wait expired (the same promise use_top implies), so the chained launches may be used
struct SweepState {
    bool use_top, allow_chain, top_disabled, chain_disabled, w_pending;
};
enum class TopKernel { none, top, sliced };
struct SweepPlan {
    bool split_columns;          // nr > 1 through a set that needs its persistent kernel and cannot have it: one column after
                                 //   the other (plans of nr = 1); nothing else of this plan is set
    size_t nper;                 // launches [0, nper) go level by level, [nper, nl - ntl) chained, the last ntl persistent
    bool chain_on;
    size_t ntl;
    int ncount;                  // fronts of the persistent part
    int tgrid, pgrid;            // the persistent kernel's grid for nr columns (0: no kernel) / the grid it is launched with
    size_t first_w;              // fronts from here on get their W late (w_pending)
    TopKernel kernel;
    int threads;
    bool keep_top;
    bool merge_levels;           // a level's block-class and one-wave launches go out as one (unless HIPKKT_NO_LEVEL_MERGE)
};
struct NrGrids { int g[2] = {-1, -1}; };     // the persistent kernel's grid for 2 / 4 right-hand sides (asked on first use)
int top_grid_for(const Schedule& sch, const DeviceLimits& dev, NrGrids& grids, int nr);
SweepPlan plan_sweep(const Schedule& sch, const SweepState& st, int nr, const DeviceLimits& dev, NrGrids& grids);

// a level's block-class launch and the one-wave launch behind it (sched order) go out as one launch:
// launches q (block-class) and q + 1 (one-wave) belong to one level
inline bool pair_at(const Schedule& sch, size_t q, const SweepPlan& p)
{
    const std::vector<Launch>& launches = sch.launches;
    return p.merge_levels && q + 1 < p.nper && !launches[q].small && launches[q].ntall == 0 && launches[q + 1].small &&
           launches[q].level == launches[q + 1].level;
}
// (a level's block-class launch and the one-wave launch behind it as one kernel launch: the records of both)
inline RecSeg pair_rec(const Launch& Lb, const Launch& Ls)
{
    RecSeg r = Ls.rec;
    r.off[0] = Lb.rec.off[0]; r.stride[0] = Lb.rec.stride[0]; r.fmax[0] = Lb.rec.fmax[0];
    return r;
}

// diagnostic (HIPKKT_VERBOSE): which path a sweep takes -- the three launch ranges, the persistent kernel and its grid,
// whether W was still pending and the record layout (the text behind "[hipkkt] sweep plan: "); at level 2 the kernel
// family and workgroup size of every per-level launch as well, one "[hipkkt] sweep launch" line each (the tests' way to
// assert a path)
std::string describe(const SweepPlan& p, const Schedule& sch, int nr, bool w_pending, bool packed);
std::string describe_launches(const SweepPlan& p, const Schedule& sch);

}  // namespace hipkkt
