// The device tables of the numeric engine, built as host-only code (no HIP header, no device): everything
// LDLEngine::upload() (hipkkt.hip) copies to the device that is not already a member of Symbolic, Schedule or FactorLists.
// This is index arithmetic whose mistakes would show as a GPU fault or a silent wrong scatter, so it lives where a
// sanitizer and the CPU tests reach it (tests/sanitize/host_driver.cpp checks every table's invariants).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "launch_shapes.hpp"
#include "schedule.hpp"
#include "symbolic.hpp"

namespace hipkkt {

struct EngineTables {
    // leaves with one column and a short row list, pulled by their parents in the many-column sweeps (per supernode;
    // HIPKKT_PULL_LEAVES=0: none): a childless one-column front of a one-wave launch with a parent and 1..47 rows
    std::vector<char> solve_pulled;
    std::vector<int> ncolpar;            // per supernode: its rows that land in its parent's columns
    // K scatter lists: S.ksrc / S.kdst with the block-class fronts' targets as positions in the panel kernel's trapezoid
    // (factor_kernels.hip: pcol; one-wave and sliced fronts keep lrow + lcol * f), then per row slice (sch.slice_list
    // order) a list of its own, [slice_kptr, slice_kptr + slice_nk), with the positions in ITS LDS image (top block + its
    // rows, as a trapezoid): the panel kernel neither scans the other slices' entries nor divides per entry
    std::vector<int> ksrc, kdst;
    std::vector<int64_t> slice_kptr;
    std::vector<int> slice_nk;
    // overlap mode: per supernode the Schur tiles of a front in an overlapped launch (0 elsewhere) and the first slice
    // record of a sliced front (-1: none; fronts factorised in row slices publish their progress per slice)
    std::vector<int> ov_ntiles, ov_sbase;
    std::vector<int64_t> toff;           // nsuper + 1: solve-matrix offsets, level by level like the panel and update stores
    std::vector<FrontDesc> desc;         // launch records in sch.sched order; pad bit 0 = solve_pulled, bit 1 = FactorLists::pulled
    std::vector<FrontDesc> sdesc;        // per row slice: its front's record with pad = slice << 16 | slices and its own K range
    // per supernode (as a child) [cut_ptr[c], cut_ptr[c + 1]): the first child-row index reaching each 64-row tile
    // boundary of the parent's U
    std::vector<int64_t> cut_ptr;
    std::vector<int> cuts;
    // forward-solve gather lists keyed by the receiving local row lc = sn_start[s] + rowptr[s] + j (= the extend-add
    // items' key): the contribution rows gsrc[item_ptr[lc] .. item_ptr[lc + 1]), children in fixed order; udst[gsrc[g]] = g
    std::vector<int64_t> item_ptr;
    std::vector<int> gsrc, udst;
    // Schur tiles in the order they are launched in: sch.tiles, with a wide launch's tiles dealt to XCD residue classes
    // (HIPKKT_TILE_XCD; FactorLists::tcut / ptcut are permuted with them)
    std::vector<int64_t> tiles;
    int dealt_launches = 0;
    int64_t dealt_tiles = 0;
    std::string dealt_list;              // " q" per dealt launch
    // PULLED LEAVES (many-column sweeps only).  Half of a sparse KKT system's contribution rows come from leaves with
    // ONE column (cfg2: 113 k of them, the slack rows of the linear cone): forward, such a leaf only forwards
    // u_r = -L(r,0) b_c to its parent's rows -- 4 KB per row and 512 columns, written and read once.  In the
    // many-column sweeps the PARENT computes those terms itself from the leaf's row of B (one row instead of nb, and
    // shared by the parent's rows through L2), the leaf does nothing forward, and its backward step is a gather
    // kernel of its own (k_bwd_leaf_m).  The parent's gather list is split: the stored contributions of its other
    // children (glm_ptr / udst_m: item_ptr / udst without the pulled ones, udst_m = -1 for them, with one extra slot at
    // the head of a row's run for the sum of its pulled terms) and the pulled terms of the n_pull_rows receiving rows
    // (row k: terms [pr_ptr[k], pr_ptr[k + 1]), sum slot pr_slot[k]; a term: leaf column hp_col in tree order, hp_row in
    // the caller's order, position hp_lidx of L(r,0) in the fronts).  Empty lists hold one zero entry.
    std::vector<int64_t> glm_ptr, hp_lidx, pr_ptr;
    std::vector<int> udst_m, hp_col, hp_row, pr_slot;
    int n_pull_rows = 0;
    int64_t n_pull_terms = 0;
    std::vector<signed char> psign;      // N: expected pivot sign, permuted order
    // byte image of the packed sweep records (launch_shapes.hpp: SolveHdr) in the layout schedule.cpp decided
    // (layout_records: Launch::rec, sch.rec_bytes); empty: the legacy layout
    std::vector<int64_t> recs;
    size_t tall_ws = 0;                  // doubles of the tall-front sweep kernels' work space (0: no such front)
};

// Throws std::runtime_error where a list exceeds int32 indexing, the tile permutation loses a tile or a front is larger
// than its record class.  fl is completed on the way: tcut / ptcut follow the launch order of `tiles`, and an empty
// items / pterms / pwcut gets the one zero entry the device buffers hold.  Reads knobs() (pull_leaves, tile_xcd).
EngineTables build_engine_tables(const Symbolic& S, const Schedule& sch, FactorLists& fl, const std::vector<int>& dsigns);

// diagnostics (HIPKKT_VERBOSE), one or more whole "[hipkkt] ..." lines each; the engine prints them in this order
std::string describe_gather_sources(const Symbolic& S, const Schedule& sch, const EngineTables& T);    // the persistent solve set's rows
std::string describe_update_blocks(const Symbolic& S, const FactorLists& fl);     // "dense children", "update blocks"
std::string describe_pulled_terms(const FactorLists& fl);                         // "pulled leaves' terms"
std::string describe_panel_items(const Symbolic& S, const Schedule& sch, const FactorLists& fl);       // the schedule's last fronts
std::string describe_tile_order(const EngineTables& T);
std::string describe_records(const Schedule& sch);                                // refused and / or built
std::string describe_solve_pulled(const EngineTables& T);                         // "many-column sweeps: ... pulled"

}  // namespace hipkkt
