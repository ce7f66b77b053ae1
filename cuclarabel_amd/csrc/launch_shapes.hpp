// What the host's schedule (schedule.cpp) and the kernels must agree on, as plain C++ without a HIP header: the size-class
// bounds, the LDS a kernel asks for as a function of its fronts, the chained kernels' workgroup count and the place of a
// launch's packed sweep records.  One definition each; kernels.hpp includes this file.
#pragma once
#include <cstddef>
#include <cstdint>

namespace hipkkt {

// LDS a workgroup may ask for: a CU's 160 KB less what the runtime keeps
constexpr size_t kLdsCap = 160 * 1024 - 512;

// rows of the full-CSR image longer than kLongRow entries are cut into chunks of kLongChunk entries, one workgroup each
// (kernels.hpp: SpmvDev; iterate_rows.hpp for the prefixes the iterate-residual kernel walks)
constexpr int kLongRow = 4096;
constexpr int kLongChunk = 2048;

// the data updates of level C (kernels.hip, "data updates"): most workgroups of 256 lanes an update kernel is launched
// with (grid-stride beyond kDataUpdateGridCap * 256 items), and of the one-launch maximum behind hipkkt_kkt_system_data_norms
constexpr int kDataUpdateGridCap = 4096;
constexpr int kDataNormsGridCap = 256;

// one-wave fronts (a wave per front in the factorisation and the sweeps)
constexpr int kSmallFrontMax = 64;         // f <= 64 ...
constexpr int kSmallSliceMax = 1536;       // ... and f*nc + nb*nb <= this many doubles of LDS per wave

// the panel kernel (factor_kernels.hip): block-column width, widest block column, trailing columns per block whose d*L
// copy is kept (nc - 16 <= 128 enforced by host)
constexpr int kPanelNB = 16;
constexpr int kMaxNbk = 16;
constexpr int kBdCols = 128;
inline size_t panel_lds_bytes(int fmax, int panel_max)
{
    (void)fmax;
    return ((size_t)8 * kPanelNB + 2 * kPanelNB * kPanelNB + (kBdCols + kPanelNB) + 2 + (size_t)panel_max + 256) * sizeof(double);
}

// the block sweep kernels (solve_kernels.hip): a front's vector and its partial sums, forward and backward
inline size_t solve_lds_bytes(int fmax, int ncmax)
{
    const size_t fpad = (size_t)((fmax + 3) & ~3), ncpad = (size_t)((ncmax + 3) & ~3);
    const size_t nks = (size_t)((ncmax + 7) >> 3), nrs = (size_t)((fmax + 7) >> 3);
    const size_t fwd = fpad + nks * fpad, bwd = fpad + nrs * ncpad;
    return (fwd > bwd ? fwd : bwd) * sizeof(double);
}

// ---- the factorisation's extend-add work lists (built on the host: schedule.cpp, build_factor_lists; walked by
// factor_kernels.hip)
struct ExtItem {                 // a piece (<= 64 rows) of one child update column that lands in a panel column; 32 bytes
    int64_t uoff;                // offset in the update store of the piece's first entry U_c(a, b)
    int relstart;                // index into rel[] of the child's row a
    int cnt;                     // rows in the piece
    int rfirst, rlast;           // parent-local target rows of the piece's first and last entry (row slices skip
                                 // pieces that miss their row range without touching rel[])
    int tcol;                    // parent-local column this item lands in
    int pad;
};

struct SubItem {                 // a child update column restricted to one 64-row tile of the parent's U; 16 bytes
    int64_t uoff;                // offset in the update store of the first entry
    int relstart;                // index into rel[] of the first row
    unsigned char cnt;           // rows (1..64)
    unsigned char qcol;          // column inside the tile (0..63)
    unsigned short pad;
};

// A PULLED LEAF (schedule.cpp: build_factor_lists) stores no update block: its parent forms the entries it needs,
// U(a, b) = -(l_a d) l_b, from the leaf's panel in the front store ([d, l_0 .. l_nb-1], one column).  One term per entry,
// eight bytes: the leaf's offset in the front store and target | a << 15 | b << 21, the target being the entry's place
// in the parent's LDS image (the panel's trapezoid index, or qcol * 65 + row of a Schur tile; below 2^15: a CU's LDS
// holds 20 480 doubles).  Terms come in chunks of 64, lane = term; the terms of one target are neighbours (a run).  Lane 0
// of a chunk carries in bits 27..29 the doubling steps that sum the chunk's longest run (0: no two terms share a
// target).  tgt_ab = kPullNone: the lane has no term.
struct PullTerm {
    uint32_t leaf_off;
    uint32_t tgt_ab;
};
constexpr uint32_t kPullNone = 0xffffffffu;
static_assert(sizeof(ExtItem) == 32, "ExtItem layout");
static_assert(sizeof(SubItem) == 16, "SubItem layout");
static_assert(sizeof(PullTerm) == 8, "PullTerm layout");

// most fronts the persistent top-of-tree kernel takes (every workgroup resident: solve_kernels.hip, k_top_solve)
constexpr int kTopMaxFronts = 480;

// narrow supernodes of the W formation: k_winv's 128-thread build (solve_kernels.hip)
constexpr int kWinvSmallNc = 32;
inline int winv_small_nc() { return kWinvSmallNc; }

// chained kernels (chain_kernels.hip): workgroup size -- one block-class front, 8 one-wave or 64 tiny fronts -- and the
// workgroups of one segment
constexpr int kChainBS = 512;
inline int chain_seg_wgs(int nblock, int nwave, int ntiny)
{
    return nblock + (nwave + kChainBS / 64 - 1) / (kChainBS / 64) + (ntiny + kChainBS / 8 - 1) / (kChainBS / 8);
}

// many-column sweeps (solve_kernels.hip, "several right-hand sides"): the kernel instances one call takes, from the padded
// column count KP (a multiple of 16) and the knobs HIPKKT_MULTI_VEC / HIPKKT_MULTI_CT.  One-wave fronts: wave_v columns
// per lane (2 where a wave's 128 columns divide KP).  Pulled leaves, forward and backward: leaf_v columns per lane (4 where
// 64 | KP unless the knob caps it, else 2 where 32 | KP, else 1).  Block-class fronts: block_bs threads and block_ct column
// tiles of 16 per workgroup (two tiles from 256 columns on where 32 | KP, unless the knob says 1; 512 threads below 128
// columns: few column blocks, so more waves per front).
struct MultiShape { int wave_v; int leaf_v; int block_bs; int block_ct; };
inline MultiShape multi_shape(int KP, int multi_vec, int multi_ct)
{
    MultiShape m;
    m.wave_v = KP % 128 == 0 ? 2 : 1;
    m.leaf_v = (KP % 64 == 0 && multi_vec >= 4) ? 4 : (KP % 32 == 0 ? 2 : 1);
    const bool wide = multi_ct != 1 && KP % 32 == 0 && KP >= 256;
    m.block_ct = wide ? 2 : 1;
    m.block_bs = (wide || KP >= 128) ? 256 : 512;
    return m;
}

// fronts too tall for the block sweep kernels' LDS (solve_kernels.hip: k_fwd_tall / k_bwd_tall): columns of a front the
// kernels keep in LDS (panels have at most 144), rows of a front per workgroup (HIPKKT_TALL_BLOCK_ROWS, a multiple of 64
// in 64..4096), and the doubles SolveArgs::tall_ws needs for a launch with ntall such fronts, the tallest of fmax rows
constexpr int kBdColsSolveMax = 160;
inline int tall_block_rows(int knob) { return knob < 64 ? 64 : (knob > 4096 ? 4096 : (knob & ~63)); }
inline size_t tall_ws_doubles(int N, int ntall, int fmax, int block_rows)
{
    return (size_t)N + (size_t)ntall * (size_t)((fmax + block_rows - 1) / block_rows) * kBdColsSolveMax;
}

// the cone kernels' size classes (kernels.hip, psd_cone.hpp; the lists: kkt_assembly.cpp, build_cone_tables): the largest
// PSD side handled by the in-LDS scaling kernel, and the rows of a generalized power cone that one wave scales (and
// multiplies), four cones to a workgroup: 8 rows per lane, all loads of a pass in flight at once.  A larger one takes a
// workgroup of 256 with an LDS stage.
constexpr int kPsdMaxDim = 48;
constexpr int kGenPowWaveMax = 512;

struct FrontDesc {               // everything a kernel needs to know about one front, in launch order; 64 bytes
    int64_t front_off;           // panel store offset
    int64_t upd_off;             // update store offset
    int64_t w_off;               // solve-matrix store offset
    int64_t rp;                  // rowptr[s]
    int64_t kptr;                // first K entry
    int s;                       // supernode id
    int c0;                      // first column
    int nc;                      // columns
    int nb;                      // rows below
    int nk;                      // K entries
    int pad;                     // row-sliced panels (TreeDev::sdesc): slice << 16 | number of slices
};
static_assert(sizeof(FrontDesc) == 64, "FrontDesc layout");

// packed sweep records: bytes of a record's header
constexpr int kSolveHdrBytes = 64;
// Packed sweep records (layout: schedule.cpp, layout_records; byte image: engine_tables.cpp, build_engine_tables): what a
// sweep kernel needs to know about a front, laid out so that it
// arrives in ONE round of loads.  The fronts of a launch and size class (block-class / one-wave / tiny) have records of one
// size, so a record's address follows from the front's place in the launch alone: [SolveHdr (64 B)] [idx: fmax ints]
// [gather slots: fmax x 32 B, absent on tree level 0] -- a thread fetches the header and its row's slots side by side,
// and the values (b, the children's contributions, the matrix) in the second round.  The legacy layout (FrontDesc ->
// gl_ptr / perm / rows -> gl_src -> values) took four.
//   idx[i]   i < nc: the row of column c0 + i in the caller's order (perm); i >= nc: the permuted index of below-row i (rows)
//   slot i   {count, six sources (indices into uvec, -1 beyond the count), index into gl_src of the seventh source}
struct SolveHdr {
    int64_t mat_off;             // block class: W = [T; M] in the solve-matrix store (W' behind it); one-wave / tiny: the panel in the front store
    int64_t rp;                  // rowptr[s]: first of the nb rows below in rows[] / uvec
    int s, c0, nc, nb;
    int par;                     // parent supernode, -1 for a root
    int nchild;                  // children swept by chained launches (ChainArgs::nchild)
    int64_t pad[3];
};
static_assert(sizeof(SolveHdr) == kSolveHdrBytes, "SolveHdr layout");
struct RecSeg {                  // the records of one kernel launch's fronts, by size class: 0 block-class, 1 one-wave, 2 tiny
    int64_t off[3];              // byte offset in SolveArgs::recs of the class's first record
    int stride[3];               // bytes per record
    int fmax[3];                 // row slots per record (a multiple of 4)
};
static_assert(sizeof(RecSeg) == 48, "RecSeg layout (a kernel argument)");

}  // namespace hipkkt
