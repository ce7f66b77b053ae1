// Device kernels of the supernodal multifrontal LDL^T, the tree solves, the KKT value updates,
// the residual SpMV and the cone scalings.  gfx950 (wave64) only.
//
// Data layout in HBM (all fronts of the tree are resident at once -- 288 GB makes the classic
// multifrontal stack unnecessary, and a static layout lets every per-iteration step be a pure
// function of precomputed index maps):
//   panel store   per supernode s: f_s x nc_s column-major (ld = f_s), f_s = nc_s + nb_s.
//                 after factorisation: strictly-lower part = L, diagonal = D.
//   update store  per supernode s: nb_s x nb_s column-major (ld = nb_s), lower triangle =
//                 the Schur complement s hands to its parent.
//   uvec          per supernode s: nb_s doubles, forward-solve contributions to the ancestors.
#pragma once
#include <hip/hip_runtime.h>
#include "launch_shapes.hpp"
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <string>

namespace hipkkt {

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };   // -> HIPKKT_ERR_HIP at the C ABI

// Function attributes (hipFuncSetAttribute) are per DEVICE, and a process may hold handles on several devices and
// drive them from several threads: run `fn` once per device ordinal, under a lock; `fn` returns a hipError_t and a
// failure throws (the C ABI turns that into a negative return code) instead of leaving a kernel that cannot launch.
class PerDeviceOnce {
    std::mutex mu_;
    uint64_t done_[4] = {0, 0, 0, 0};       // 256 device ordinals
public:
    template <class F>
    void run(F&& fn)
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 256) throw HipError("hipGetDevice failed");
        std::lock_guard<std::mutex> lk(mu_);
        if (done_[dev >> 6] >> (dev & 63) & 1) return;
        const hipError_t e = fn();
        if (e != hipSuccess) {
            (void)hipGetLastError();
            throw HipError(std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e));
        }
        done_[dev >> 6] |= (uint64_t)1 << (dev & 63);
    }
};
template <class K>
inline hipError_t set_max_lds(K kernel, int bytes)
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// (ExtItem, SubItem -- the extend-add work lists' records, built by schedule.cpp -- and PullTerm: launch_shapes.hpp)

// (FrontDesc, the launch records, and SolveHdr, the header of the packed sweep records: launch_shapes.hpp)
// (RecSeg, the records of one kernel launch's fronts by size class: launch_shapes.hpp)

struct TreeDev {                 // device copies of the symbolic structure
    int nsuper;
    const int* sn_start;         // nsuper+1
    const int64_t* rowptr;       // nsuper+1
    const int* rows;             // sum nb
    const int* rel;              // sum nb: local row in the parent's front
    const int* ncolpar;          // nsuper: how many of s's rows fall in its parent's columns
    const int64_t* front_off;    // nsuper+1
    const int64_t* upd_off;      // nsuper+1
    const int* child_ptr;        // nsuper+1
    const int* child_idx;
    const int64_t* kptr;         // nsuper+1
    const int* ksrc;
    const int* kdst;
    const int* sched;            // supernodes in launch order (level by level, size class inside)
    const int* spos;             // supernode -> position in sched
    const int* sn_parent;        // assembly tree
    const FrontDesc* sdesc;      // row slices of the panels too tall for one CU's LDS, one record per slice (k_panel SLICED)
    const FrontDesc* desc;       // same order: one 64-byte record per launch slot (one scalar load instead of a
                                 // chain of dependent index loads at the head of every kernel)
    const signed char* psign;    // N: expected pivot sign, permuted order
    const int* perm;             // N: perm[new] = old
    // Extend-add work lists of the panel columns: the pieces of child update columns that land in a panel column,
    // grouped by column, children in fixed order; a wave owns whole columns (wave_cut) and applies their pieces
    // one after the other (deterministic).  Local row / column j of front s has index lc = sn_start[s] + rowptr[s] + j
    // (used by the gather lists below).
    const int64_t* item_ptr;     // = gl_ptr
    const ExtItem* items;
    // dense child (schedule.cpp, build_factor_lists): offset in upd of the child whose update block is this front's whole front
    // (entry (r, j) -> entry (r, j), leading dimension = this front's size), or -1; block-class fronts only
    const int64_t* dense_off;
    // forward-solve gather lists: local row r of front s (same indexing) receives
    // uvec[gl_src[q]] for q in gl_ptr[lc] .. gl_ptr[lc+1]
    const int64_t* gl_ptr;
    const int* gl_src;
    // inverse of gl_src: contribution entry e of the tree (index into uvec) is gather-list entry udst[e] of its
    // receiver.  The multi-column solve stores contributions in THAT order, so a receiver reads a contiguous run.
    const int* udst;
    // many-column sweeps (solve_kernels.hip, k_*_m): one-column leaves are PULLED -- the parent computes -L(r,0) b_c from
    // the leaf's row of B instead of reading a stored contribution row.  glm_ptr / udst_m are gl_ptr / udst without the
    // pulled leaves' entries (udst_m = -1 for them), with one extra slot at the head of a row's run for the SUM of its pulled
    // terms (k_pull_leaves_m); a term is the leaf's column hp_col (tree order) and the position hp_lidx of L(r,0) in
    // `fronts`.  A pulled leaf's launch record has FrontDesc::pad bit 0 set.
    const int64_t* glm_ptr;
    const int* udst_m;
    const int* hp_col;
    const int* hp_row;           // = perm[hp_col]: the leaf's row in the caller's order
    const int64_t* hp_lidx;
    const int64_t* pr_ptr;       // receiving rows with pulled terms: row k's terms are pr_ptr[k] .. pr_ptr[k+1] of hp_*, their sum
    const int* pr_slot;          // goes to slot pr_slot[k] of the receiver-ordered store (the first of the row's run)
    // per child c: cuts[cut_ptr[c] + t] = first child row index whose parent-local row >= nc_p + 64 t
    const int64_t* cut_ptr;
    const int* cuts;
    // per supernode: 17 item indices splitting its panel items (local columns < nc) into 16 slices
    // that end on column boundaries: a wave takes whole columns, so no two waves share a target column
    const int64_t* wave_cut;     // (nsuper + row slices) * 17: supernode s at s, row slice q of sdesc at nsuper + q (its own item list)
    const int64_t* tinv_off;     // nsuper+1: offset of the solve matrix W = [L11^{-1}; L21 L11^{-1}] (f x nc)
    // Schur tiles: sub-items of tile t are sitems[tile_cut[5t] .. tile_cut[5t+4]), sorted by tile column;
    // wave w of the tile's workgroup takes [tile_cut[5t+w], tile_cut[5t+w+1]) -- whole columns
    const SubItem* sitems;
    const int64_t* tile_cut;     // 5 per tile
    // the factorisation's pulled leaves (schedule.hpp: FactorLists; FrontDesc::pad bit 1 marks such a leaf): chunks of 64
    // terms; wave slice w of front s walks chunks [pwave_cut[17 s + w], pwave_cut[17 s + w + 1]), wave w of the tile at
    // launch position t chunks [ptile_cut[5 t + w], ptile_cut[5 t + w + 1])
    const PullTerm* pterms;
    const int* pwave_cut;
    const int* ptile_cut;
};

struct FactorArgs {
    TreeDev T;
    const double* Kval;          // caller's K.nzval (original order, un-regularised)
    const double* eps;           // device scalar: static regulariser to add as eps*sign, or null
    const double* eps_col;       // N, permuted order: the regulariser of each column's member instead of *eps, or null
    double* fronts;
    double* upd;
    double* Dinv;                // N, permuted order
    int* flags;                  // [0] #dynamic regularisations, [1] non-finite pivot seen, [2] an overlap-mode wait gave up
    // Overlap mode (the narrow top of the tree, factor_kernels.hip "overlap"): a level's Schur tiles run on a second
    // stream BESIDE its panels and the next level's panels, ordered by counters in memory instead of kernel boundaries.
    //   ov_prog[s]    panel columns of supernode s whose L / D entries are published (written through) this factorisation
    //   ov_done[s]    Schur tiles of s completed this factorisation
    //   ov_ntiles[s]  tiles a parent's panel must wait for (0: s is not factorised in overlap mode)
    int* ov_prog;
    int* ov_done;
    const int* ov_ntiles;
    //   ov_sprog[q]   the same progress per ROW SLICE q (position in TreeDev::sdesc) of a front factorised in slices
    //   ov_sbase[s]   first slice of supernode s in sdesc (-1: s is factorised whole)
    int* ov_sprog;
    const int* ov_sbase;
    //   ov_started[q] panel workgroups (whole panels and row slices) of launch q that have begun to run this
    //                 factorisation: the launch's tile kernel is released by a gate (k_ov_gate) once ALL of them are
    //                 resident -- a tile workgroup that waits for its panel then never keeps that panel off a CU
    int* ov_started;
    int ov_slot;                 // this launch's index q
    int ov;                      // this launch runs in overlap mode
    long long ov_limit;          // bound of every overlap-mode wait in 100 MHz ticks (50 ms; the tests set it to 0 to
                                 // force the give-up-and-repeat path: HIPKKT_OV_TEST_LIMIT)
    double dyn_eps, dyn_delta;
    int nbk;                     // block-column width (<= 16), chosen so the LDS buffer fits
    long long* stamps;           // diagnostic only (HIPKKT_STAMPS=1): phase time stamps of block 0, else null
    int stamp_row;
};
#define HIPKKT_STAMP(A, k) do { if ((A).stamps && blockIdx.x == 0 && threadIdx.x == 0) \
        (A).stamps[(A).stamp_row * 16 + (k)] = wall_clock64(); } while (0)

struct SolveArgs {
    TreeDev T;
    const double* fronts;
    const double* tinv;          // per supernode: W = [T; M], f x nc col-major
    const double* Dinv;
    const double* b;             // original order
    double* out;                 // original order
    double* xp;                  // N, permuted work vector
    double* uvec;                // sum nb
    // NR right-hand sides in one launch (the single-column kernels' NR template parameter): column c of b, out, xp,
    // uvec lives at these strides
    long long* top_stamps;       // diagnostic only (HIPKKT_TOP_STAMPS=1): per front of the persistent set and direction eight
                                 // wall-clock stamps of its hop (k_top_solve), else null
    long long top_limit;         // bound of every wait of the persistent kernels in 100 MHz ticks (50 ms; the tests set
                                 // it to 0 to force the give-up-and-repeat path: HIPKKT_TOP_TEST_LIMIT)
    int64_t ld_b, ld_out, ld_xp, ld_uvec;   // (b, out: columns ld apart.  The sweeps' internal vectors xp and uvec keep their
                                            //  NR columns INTERLEAVED -- entry i of column c at i * NR + c -- so that a gather
                                            //  touches one cache line for all columns; ld_xp / ld_uvec are unused)
    // k_top_solve_sliced (sets with very tall fronts): its tasks are (front, slice) pairs -- a front whose W is too
    // large for one CU to stream per hop is cut into R slices (rows of W forward, columns of x backward) that never
    // exchange anything.  Task t works on the front at set position tk_pos[t], slice tk_sl[t] & 0xff of tk_sl[t] >> 8;
    // the tasks of position p are tbase[p] .. tbase[p+1]; xf keeps a front's forward solution while its backward
    // slices overwrite xp.
    const int* tk_pos;
    const int* tk_sl;
    const int* tbase;
    double* xf;
    const double* add;           // many-column sweeps (row-major N x KP): out = solution + add where non-null
    double* tall_ws;             // work space of the tall-front sweep kernels (k_*_tall_*): N doubles + the blocks' partial sums; or null
    const char* recs;            // packed sweep records (SolveHdr ...), or null: the legacy layout (TreeDev::desc, gl_ptr, ...)
    int* chain_cnt;              // nullable; the chained launches' forward counters (ChainArgs::cnt): a sweep that chains the
                                 // levels below the persistent set leaves the set's fronts' counters at their bottom
                                 // children's count, and the persistent kernels put them back to zero
};

constexpr int kSolveChunk = 128;  // diagonal chunk of the triangular solves: one wave, two unknowns per lane
// (kMaxNbk, solve_lds_bytes, kTopMaxFronts, winv_small_nc, kSmallFrontMax / kSmallSliceMax, panel_lds_bytes: launch_shapes.hpp)
// persistent kernel over the top `count` fronts (schedule positions begin ..): forward then backward sweep
int top_solve_capacity(size_t lds, bool tall);   // resident workgroups the device guarantees for the persistent kernel
                                                // (tall: its 1024-thread build for sets with very tall fronts)
int top_solve_capacity_nr(size_t lds_total, int nr);     // the same for the 1024-thread build's NR-column instance
// nr right-hand sides (1, 2 or 4); lds = bytes per right-hand side
void launch_top_solve(const SolveArgs& a, int begin, int count, int grid, size_t lds, int* flags, int nflag, int epoch,
                      hipStream_t st, bool tall, int nr = 1);
int top_solve_sliced_capacity(size_t lds, int nr = 1);
void launch_top_solve_sliced(const SolveArgs& a, int begin, int pos0, int task0, int task1, int grid, size_t lds, int* flags, int nflag,
                             int epoch, hipStream_t st, int nr = 1);
// max_blocks > 0: at most that many workgroups (each walks several supernodes); nsmall: how many of the list's supernodes
// have at most winv_small_nc() columns -- enough of them and they go to a launch of their own, four times as many 128-thread
// workgroups (solve_kernels.hip: k_winv)
void launch_tinv(const TreeDev& T, const double* fronts, double* tinv, const int* list, int count, int ncmax,
                 hipStream_t st, int max_blocks = 0, int nsmall = 0);

// factorisation of one level: small fronts (one wave each), panels (one workgroup each), then the
// update blocks tiled over many workgroups
void launch_front_wave(const FactorArgs& a, int begin, int count, int slice_doubles, hipStream_t st);
void launch_front_tiny(const FactorArgs& a, int begin, int count, hipStream_t st);     // fronts with f <= 8, eight to a wave
void launch_panel(const FactorArgs& a, int begin, int count, int bs, size_t lds, hipStream_t st);
// row slices of the panels too tall for one CU (TreeDev::sdesc[begin ..]), one 1024-thread workgroup each
void launch_panel_sliced(const FactorArgs& a, int begin, int count, size_t lds, hipStream_t st);
// ov_grid: overlap mode only -- the number of tile workgroups that may exist at a time (they walk the launch's tiles)
void launch_schur(const FactorArgs& a, const int2* tiles, int tile_begin, int ntiles, hipStream_t st, int ov_grid = 0, int tile_nc = 0);
// which build of the tile kernel launch_schur takes for a launch of ntiles tiles, tile_nc columns deep on average (ov: the
// launch runs in overlap mode) -- launch_schur's own decision, also named on the per-launch line of HIPKKT_VERBOSE=2
enum class SchurBuild { none, plain, pipelined, overlap };
SchurBuild schur_build(bool ov, int ntiles, int tile_nc);
inline const char* schur_build_name(SchurBuild b)
{
    return b == SchurBuild::none ? "none" : b == SchurBuild::plain ? "plain" : b == SchurBuild::pipelined ? "pipelined" : "overlap";
}
// overlap mode: returns (the stream goes on) once *started >= target, i.e. every panel workgroup of the launch is resident
void launch_ov_gate(const int* started, int target, int* abort_word, long long limit, hipStream_t st);
// word2[0] must be 0; afterwards word2[1] = 1 iff a kernel on `second`, submitted behind a waiting kernel on `first`, ran
// while that one waited -- i.e. the two streams do not share a hardware queue
void launch_concurrency_probe(int* word2, hipStream_t first, hipStream_t second);
// litmus test of the hand-over contract (factor_kernels.hip): 2 * pairs workgroups, producer / consumer pairs
void launch_handover_litmus(int variant, double* payload, int* sig, int* ack, int pairs, int words, int rounds,
                            unsigned long long* mismatches, unsigned long long* timeouts, hipStream_t st);
// nr = 1, 2 or 4 right-hand sides per launch (column strides in SolveArgs::ld_*); lds = bytes per right-hand side
// (rs: the launch's packed records; ignored when SolveArgs::recs is null)
void launch_fwd(const SolveArgs& a, const RecSeg& rs, int begin, int count, int bs, size_t lds, hipStream_t st, int nr = 1);
void launch_bwd(const SolveArgs& a, const RecSeg& rs, int begin, int count, int bs, size_t lds, hipStream_t st, int nr = 1);
// one launch for a level's one-wave fronts [begin, begin + nwave) and the tiny fronts behind them
void launch_fwd_small(const SolveArgs& a, const RecSeg& rs, int begin, int nwave, int ntiny, hipStream_t st, bool leaf = false, int nr = 1);
void launch_bwd_small(const SolveArgs& a, const RecSeg& rs, int begin, int nwave, int ntiny, hipStream_t st, int nr = 1);
// one launch for a whole level: nblock block-class fronts at [begin, ..), then nwave one-wave, then ntiny tiny fronts
void launch_fwd_level(const SolveArgs& a, const RecSeg& rs, int begin, int nblock, int nwave, int ntiny, int bs, size_t lds, hipStream_t st, int nr = 1);
void launch_bwd_level(const SolveArgs& a, const RecSeg& rs, int begin, int nblock, int nwave, int ntiny, int bs, size_t lds, hipStream_t st, int nr = 1);

// several right-hand sides: work vectors row-major N x KP / sum(nb) x KP (KP = columns rounded up to 16)
// iperm[caller's index] = permuted index
void launch_permute_in(const double* B, int64_t ldb, double* Xp, int KP, const int* iperm, int N, int nrhs, hipStream_t st);
// row-major source / destination (N x KP): rows move, columns stay; dir 0: Xp[iperm[o]] = B[o], 1: X[o] = Xp[iperm[o]]
void launch_permute_rows(double* dst, const double* src, int KP, const int* iperm, int N, int dir, hipStream_t st, const double* add = nullptr);
void launch_permute_out(double* X, int64_t ldx, const double* Xp, int KP, const int* iperm, int N, int nrhs, hipStream_t st);
void launch_fwd_multi(const SolveArgs& a, int begin, int count, bool small, int ncmax, int KP, hipStream_t st);
// fronts too tall for the block kernels' LDS: their rows spread over workgroups (fmax: tallest of them; SolveArgs::tall_ws)
void launch_fwd_tall(const SolveArgs& a, int begin, int count, int fmax, hipStream_t st);
void launch_bwd_tall(const SolveArgs& a, int begin, int count, int fmax, int N, hipStream_t st);
// (the doubles SolveArgs::tall_ws needs for a launch with such fronts: launch_shapes.hpp, tall_ws_doubles)
void launch_pull_leaves_multi(const SolveArgs& a, int nrows, int KP, hipStream_t st);
void launch_bwd_multi(const SolveArgs& a, int begin, int count, bool small, int ncmax, int KP, hipStream_t st, bool leaves = false);

// ---- chained levels (chain_kernels.hip): several tree levels of a sweep in ONE launch, ordered by counters in memory
// instead of kernel boundaries.  A segment is one launch of the per-level path (same three size classes); workgroups are
// numbered segment by segment, so that every workgroup depends only on workgroups with a LOWER index.
struct ChainSeg {
    int begin;                   // schedule position of the segment's first front
    int nblock, nwave, ntiny;    // block-class fronts, then one-wave fronts, then tiny fronts (f <= 8)
    int wg0;                     // the segment's first workgroup
    int leaf;                    // forward: the fronts have no children (tree level 0)
    RecSeg rec;                  // the fronts' packed records
};
constexpr int kChainMaxSeg = 20;
struct ChainArgs {
    int nseg;
    int lo, hi;                  // schedule positions covered by this launch (backward: a parent at a position >= hi is complete)
    int* cnt;                    // nsuper: forward, children of supernode s that have handed over their contribution this sweep
    const int* nchild;           // nsuper: how many of s's children are swept by chained launches (the ones that add to cnt[s])
    int* done;                   // nsuper: backward, epoch of supernode s's last finished backward step
    int* abort_word;             // set when a bounded wait expires: everyone leaves, the host repeats the sweep level by level
    int epoch;
    int lo0, nstamp;             // diagnostic (SolveArgs::top_stamps): first position and number of fronts of the sweep's chained part
    ChainSeg seg[kChainMaxSeg];
};
// lds = bytes per right-hand side of the largest block-class front in the segments (0: none)
void launch_fwd_chain(const SolveArgs& a, const ChainArgs& c, int nwg, size_t lds, hipStream_t st, int nr);
void launch_bwd_chain(const SolveArgs& a, const ChainArgs& c, int nwg, size_t lds, hipStream_t st, int nr);
inline int chain_seg_wgs(const ChainSeg& s) { return chain_seg_wgs(s.nblock, s.nwave, s.ntiny); }     // (kChainBS: launch_shapes.hpp)

// ---- KKT value updates (kktsolver_directldl.jl:130-188, 211-245, 374-386)
void launch_scatter(double* Kval, const int* idx, const double* vals, int64_t n, double scale, hipStream_t st);
// ---- data updates with the handle's frozen equilibration (data_updating.jl:56-247): one matrix of the handle as the
// update kernel sees it.  val: the handle's scaled copy of the matrix's values; map: its entries' places in K; row / col:
// every entry's row and column in the matrix's own numbering (data_update.hpp); L, R, c: the scalings (P: d, d, c;
// A: e, d, 1).  fval = nullptr: the residual's copy is dirty and is left alone (it will be gathered whole).
struct DataMatDev {
    double* val; double* K; double* fval;
    const int* kpos; const int* map; const int* row; const int* col;
    const double* L; const double* R;
    double c;
};
// v: k unscaled values; idx: their positions (device, int64) or nullptr for positions 0 .. k - 1
void launch_data_update_matrix(const DataMatDev& M, const double* v, const int64_t* idx, int64_t k, hipStream_t st);
// y[j] = fl(fl(v * scale[j]) * c), yneg[j] = -y[j] (yneg nullable)
void launch_data_update_vector(double* y, double* yneg, const double* scale, double c, const double* v, const int64_t* idx,
                               int64_t k, hipStream_t st);
void launch_reciprocals(double* dinv, const double* d, int64_t n, double* einv, const double* e, int64_t m, hipStream_t st);
// out2[0] = max |q dinv|, out2[1] = max |b einv|; out2 (two doubles) must hold zeros when the kernel starts
void launch_data_norms(const double* q, const double* dinv, int64_t n, const double* b, const double* einv, int64_t m,
                       double* out2, hipStream_t st);
// the two updates that carry c, and the norms, on a stack whose members have their own cost scaling: c = cmem[xmem[row]]
// (xmem: the partition's x row -> member table; cmem: nb doubles), same order of operations.  slot: n + m words' indices
// (data_update.hpp: build_norm_slots); out: 2 nb doubles that hold zeros when the kernel starts -> out[2 b] = member b's
// max |q dinv| (NOT yet divided by its c), out[2 b + 1] = its max |b einv|
void launch_data_update_matrix_member(const DataMatDev& M, const int* xmem, const double* cmem, const double* v, const int64_t* idx,
                                      int64_t k, hipStream_t st);
void launch_data_update_vector_member(double* y, double* yneg, const double* scale, const int* xmem, const double* cmem,
                                      const double* v, const int64_t* idx, int64_t k, hipStream_t st);
void launch_data_norms_member(const double* q, const double* dinv, int64_t n, const double* b, const double* einv, int64_t m,
                              const int* slot, double* out, hipStream_t st);
void launch_scale(double* Kval, const int* idx, double scale, int64_t n, hipStream_t st);
// eps = c0 + c1 * max_i |Kval[diag[i]]|  (kktsolver_directldl.jl:297-310) -> *eps_out
void launch_regularizer(const double* Kval, const int* diag, int N, double c0, double c1,
                        double* partial, double* eps_out, hipStream_t st);

// ---- residual: e = b - K_sym x on the un-regularised K, and infinity norms
struct SpmvDev {
    const int64_t* ptr;          // N+1, full symmetric CSR
    const int* col;
    const int* vmap;             // entry -> index into Kval
    const double* val;           // the values in CSR order (a refreshed copy of Kval[vmap[.]]), or null
    const int64_t* pend;         // nullable; rows of the x block (row < n): end of the row's entries with column < n (P)
    int N;
    int lanes_per_row;           // 8 or 64
    // rows longer than kLongRow entries (a dense constraint row, say) are cut into chunks of kLongChunk entries,
    // one workgroup each, and their partial sums combined in chunk order: no single wave walks 50 000 entries
    int nlong, nchunks;
    const int* long_rows;        // nlong
    const int64_t* long_chunk_ptr;   // nlong + 1: chunk range of each long row
    const int64_t* chunk_q;      // nchunks + 1 would not do (rows are not adjacent): 2 per chunk, [begin, end)
    double* long_partial;        // nchunks per right-hand side
};
// (kLongRow, kLongChunk: launch_shapes.hpp)
// norm_out[j] = ||e_j||_inf (not finite if any entry is non-finite).  nrhs > 1: column j of b, x, e
// at stride ld; `partial` then needs nrhs * (kNormParts + 1) doubles
constexpr int kNormParts = 2048;   // partial needs nrhs * (kNormParts + 1) doubles
constexpr int kMaxNormbCols = 4;   // ||b|| rides along in the residual pass for up to this many columns: partial then needs
                                   // nrhs * (2 kNormParts + 1) doubles
void launch_update_values(double* K, const int* mapHs, const double* Hs, int nHs, const int* mapU, const int* mapV,
                          const int* mapD, const double* u, const double* v, const double* eta2, const int* soc_of_entry,
                          int sparse_len, int nsparse, double* fval, const int* kpos, hipStream_t st);
// flag_in/flag_out (nullable): *flag_out = (*flag_in != 0) as a double, so that a device status word rides along
// with the norm read-back
void launch_residual(const SpmvDev& A, const double* Kval, const double* b, const double* x, double* e,
                     double* partial, double* norm_out, hipStream_t st, int nrhs = 1, int64_t ld = 0,
                     const int* flag_in = nullptr, double* flag_out = nullptr, double* normb_out = nullptr);
// normb_out (nullable): ||b_j||_inf as well -- in the same pass when there is one column and no long row
// (partial then needs 2 * (kNormParts + 1) doubles), by a separate reduction otherwise
void launch_norm_inf(const double* v, int n, double* partial, double* out, hipStream_t st, int nrhs = 1,
                     int64_t ld = 0);
void launch_axpby_sum(double* y, const double* a, const double* b, int64_t n, hipStream_t st);   // y = a + b
// val[q] = Kval[vmap[q]]: the CSR-ordered copy the residual streams (one gather per value update instead of one
// per residual)
void launch_gather_values(double* val, const double* Kval, const int* vmap, int64_t nnz, hipStream_t st);
// b_j = [rx_j; rz_j; 0]: rx is n x nrhs (ld n), rz is m x nrhs (ld m), b is N x nrhs (ld N)
void launch_pack_rhs(double* b, const double* rx, const double* rz, int n, int m, int p, hipStream_t st,
                     int nrhs = 1);
// ---- row-major (N x KP, KP = columns rounded up to 16, padding columns zero) variants for the multi-column path:
// a row of 16 columns is one 128-byte line, so the SpMV's gather of x moves whole lines
void launch_pack_rhs_rm(double* B, const double* rx, const double* rz, int n, int m, int p, int nrhs, int KP, hipStream_t st);
void launch_unpack_lhs_rm(double* lhsx, double* lhsz, const double* X, int n, int m, int nrhs, int KP, hipStream_t st);
// norm_out[c] = ||e_c||_inf, normb_out[c] = ||b_c||_inf (nullable); partial: 2 * 512 * KP doubles; no long rows (A.nlong == 0)
void launch_residual_rm(const SpmvDev& A, const double* B, const double* X, double* E, double* partial, double* norm_out,
                        double* normb_out, int KP, hipStream_t st);
void launch_accept_columns_rm(double* X, const double* cand, double* E, const double* E2, const int* mask, int N, int KP,
                              hipStream_t st);
// columns j with mask[j] != 0: x_j = cand_j, e_j = e2_j  (N x nrhs, ld N)
void launch_accept_columns(double* x, const double* cand, double* e, const double* e2, const int* mask, int N,
                           int nrhs, hipStream_t st);
void launch_check_finite(const double* v, int n, int* flag, hipStream_t st);
// kktsolver_getlhs! (kktsolver_directldl.jl:329-343) on the device: lhsx = x[0:n], lhsz = x[n:n+m]; either may be null.
// One kernel instead of two device-to-device copies (the copy engine's latency is several kernel launches' worth).
void launch_unpack_lhs(double* lhsx, double* lhsz, const double* x, int n, int m, hipStream_t st);
// The refinement loop's accept / stop rule (kktsolver_directldl.jl:389-449) evaluated on the device after round r
// (kernels.hip, k_ir_round), for nr right-hand side columns at once (column c: state + c state_stride, norme0[c],
// normb[c], cand[c], x + c n, dx + c n, readback + 5 c).  state holds 4 doubles per round {active, rounds, bad, norme};
// readback (nullable): 5 doubles {state of round r, abort} per column for ONE copy to the host; sticky (nullable): the
// deferred-status record {bad, more, abort, rounds, #dyn. regularisations, eps, solves} (several columns: each adds its own).
// IrPartials: the residual kernels' partial maxima left un-finished (launch_residual with norm_out = nullptr, allowed when
// residual_partials_ok): column c's np = residual_grid + 1 partials of ||e0|| at e0 + c np, its np - 1 of ||b|| at
// b0 + c (np - 1), of the candidate's ||e|| at cand + c np -- the kernel takes the maxima itself and stores ||e0||, ||b||
// to norme0 / normb for later rounds.  flag_in: the sweeps' abort word (instead of abort_word, its copy as a double).
// Null pointers: the norms come finished in norme0 / normb / cand.
struct IrPartials { const double* e0 = nullptr; const double* b0 = nullptr; const double* cand = nullptr; int np = 0; const int* flag_in = nullptr; };
void launch_ir_round(double* state, int state_stride, int r, bool first, double* norme0, double* normb,
                     const double* cand, const double* abort_word, double* x, const double* dx, int n, int nr, double abstol,
                     double reltol, double stop_ratio, int max_iter, double* readback, double* sticky, hipStream_t st,
                     const IrPartials& Q = IrPartials{});
int residual_grid(const SpmvDev& A);     // workgroups (= partials per column, less the long rows' one) of the residual kernel
inline bool residual_partials_ok(const SpmvDev& A, int nrhs) { return A.nlong == 0 && nrhs <= kMaxNormbCols; }
void launch_ir_fold(const double* state, int state_stride, int r, int nr, const double* abort_word, double* sticky, hipStream_t st);
void launch_fold_update_status(double* sticky, const double* st4, hipStream_t st);
void launch_fold_flag(double* sticky, const int* flag, hipStream_t st);
// p[0..n) = 0 with a kernel: a small hipMemsetAsync stalls the stream for ~40 us on this stack
void launch_zero_ints(int* p, int n, hipStream_t st);
struct ZeroList {
    int* p[8];
    int n[8];
    int count = 0;
    void add(int* ptr, int len) { if (ptr && len > 0 && count < 8) { p[count] = ptr; n[count] = len; ++count; } }
};
void launch_zero_ints_multi(const ZeroList& Z, hipStream_t st);      // up to eight arrays in one launch
// dst[0..4] = {eps[0], conefail[0], flags[0], flags[1], flags[2]} (null pointers read as 0)
// sticky (nullable): also fold the words into the deferred-status record (what launch_fold_update_status does)
void launch_collect_status(double* dst, const double* eps, const int* conefail, const int* flags, hipStream_t st, double* sticky = nullptr);

// ---- cone scalings on the device (update_scaling! + get_Hs!, src/cones/coneops_*.jl)
struct ConeDev {
    int ncones;
    const int* kind;             // per cone
    const int* off;              // rng_cones start
    const int* numel;
    const int64_t* boff;         // rng_blocks start
    const int* sidx;             // sparse SOC index or -1
    const int* soff;             // offset in concatenated u/v or -1
    // per-element cone id for the elementwise (zero / nonnegative) kernels
    const int* elem_cone;        // m
    // list of second-order cones
    const int* soc_list;
    int nsoc;
    // list of PSD cones; psd_dim = matrix side k, psd_aoff = offset of the cone's k x k matrix R R' in psdA
    const int* psd_list;
    const int* psd_dim;          // per cone (0 for non-PSD)
    const int64_t* psd_aoff;     // per cone
    int npsd;
    int psd_kmax;
    // lists of exponential and of power cones (kinds 4, 5; three rows each), so that neighbouring lanes of the scaling
    // kernel run the same branch; ns_index = position among both (in cone order) or -1; param = alpha of a power cone
    const int* exp_list = nullptr;
    const int* pow_list = nullptr;
    const int* ns_index = nullptr;   // per cone
    const double* param = nullptr;   // per cone
    int nexp = 0, npow = 0;
    int ns_strategy = 0;             // 0 primal-dual, 1 dual (hipkkt_kkt_set_nonsymmetric_scaling)
    double ns_mu = 0.0;              // read by the dual strategy only, and by the generalized power cones always
    // generalized power cones (kind 6), k = index among them in cone order: gp_cone[k] = cone, gp_dim1[k] = number of
    // alphas, gp_off[k] = start of the cone's rows in the concatenated per-row arrays (gp_alpha holds the alphas in the
    // first dim1 slots of a cone; gp_mapP the K entries of column p; gp_mapQR those of q, then of r).  gp_small lists the
    // k that one wave takes (numel <= kGenPowWaveMax), gp_big those that take a workgroup.  gp_mu: the mu of the scaling
    // that the stored p, q, r, d belong to (mul_Hs).
    const int* gp_cone = nullptr;
    const int* gp_dim1 = nullptr;
    const int* gp_off = nullptr;
    const double* gp_alpha = nullptr;
    const int* gp_small = nullptr;
    const int* gp_big = nullptr;
    const int* gp_mapP = nullptr;
    const int* gp_mapQR = nullptr;
    const int* gp_mapD = nullptr;    // three per cone
    int ngp_small = 0, ngp_big = 0;
    double gp_mu = 0.0;
    // PSD cones of side kPsdMaxDim < k <= kPsdBigMaxDim, listed only on a handle that has opted in
    // (hipkkt_kkt_enable_large_psd); psd_list holds the sides <= kPsdMaxDim.  psd_work: 3 psdb_kmax^2 doubles per listed
    // cone, in list order -- the matrices the big-class kernels stream instead of keeping them in LDS.
    const int* psdb_list = nullptr;
    int npsdb = 0, psdb_kmax = 1;
    double* psd_work = nullptr;
};
// (kGenPowWaveMax, the rows of a generalized power cone that one wave takes: launch_shapes.hpp)
struct ConeState {
    double* w;                   // m: NN: sqrt(s/z); SOC: normalised w
    double* lam;                 // m: scaled point lambda = W z (NN: sqrt(s z); SOC: coneops_socone.jl:113-123); may be null
    double* eta;                 // per cone (SOC)
    double* u;                   // sparse_len
    double* v;                   // sparse_len
    double* eta2;                // nsparse
    double* Hs;                  // |Hs| positive blocks
    double* psdA;                // per PSD cone: A = R R' (k x k col-major), Hs = A (x)_s A
    double* psdR;                // per PSD cone: R = L1 V Lam^{-1/2} and Rinv = Lam^{-1/2} U' L2' (k x k col-major, same
    double* psdRinv;             //   offsets as psdA); the singular values Lam go to lam[off .. off + k), descending
    int* fail;                   // set to 1 when a point is not interior
    // hipkkt_kkt_system_set_member_status: fail_mem[cone_mem[c]] is set beside *fail (nb words; cone_mem: BatchDev's)
    int* fail_mem = nullptr;
    const int* cone_mem = nullptr;
    double* ns_grad = nullptr;  // per exponential / power cone: grad f*(z), 3 doubles
    double* ns_H = nullptr;      // ... and H*(z), 3 x 3
    // generalized power cones, per row at gp_off: grad f*(z), d = (d1, d2 ...), p, and q followed by r -- all unscaled
    double* gp_grad = nullptr;
    double* gp_d = nullptr;
    double* gp_p = nullptr;
    double* gp_qr = nullptr;
    // where their expansion columns go in the same launch: K.nzval and the residual's CSR-ordered copy (put_k)
    double* Kval = nullptr;
    double* fval = nullptr;
    const int* kpos = nullptr;
};
// (kPsdMaxDim, the largest PSD side handled by the in-LDS scaling kernel: launch_shapes.hpp)
// Largest side of the big class.  Its scaling kernel keeps in LDS only the pair (M, V) that the one-sided Jacobi rotates,
// 2 k^2 doubles: 147 456 B at k = 96, which leaves 16 KB of the CU's 160 KiB for the reduction arrays; at k = 100 the pair
// takes 160 000 B and leaves 3 840 B.  96 is the last multiple of 16 that fits.  (= HIPKKT_PSD_MAX_SIDE_LARGE)
constexpr int kPsdBigMaxDim = 96;
// Workgroup of the big class: the Jacobi sweeps give a column pair eight lanes, and side 96 has 48 pairs, which 256
// threads (32 groups of eight) cannot hold; 512 threads are 64 groups.
constexpr int kPsdBigThreads = 512;
void launch_cone_scaling(const ConeDev& C, const ConeState& S, const double* s, const double* z, int m,
                         hipStream_t st);
// addend != null: y = -(W'W x + addend) (the Delta_s recovery of kkt_solve!, kktsystem.jl:206-212)
// Publish: a call's status record handed to the host by the call's LAST kernel instead of a copy and a zeroing launch
// behind it (~5 us each): n doubles from rec to dst -- page-locked host memory the device can write -- then the first
// nzero doubles of rec set to zero for the next call.  The host reads dst after synchronising with the stream.
// seq: written behind the record (dst[n]); the host checks it against the number it passed -- a device store to host memory
// that did not arrive (a mapping this code has not been run on) is then seen, not read as an all-zero "no error" record.
struct Publish { double* dst = nullptr; double* rec = nullptr; int n = 0, nzero = 0; double seq = 0.0; };
void launch_publish(const Publish& p, hipStream_t st);            // ... as a kernel of its own
void launch_mul_Hs(const ConeDev& C, const ConeState& S, double* y, const double* x, int m, hipStream_t st, const double* addend = nullptr,
                   const Publish& pub = Publish{});
void launch_psd_A_from_R(const ConeDev& C, const ConeState& S, hipStream_t st);    // psdA = psdR psdR' per PSD cone
// Hs blocks, sparse second-order-cone u / v / eta^2 (and psdA) from the scaling already in S (w, eta, psdR): get_Hs! on the device
void launch_cone_from_scaling(const ConeDev& C, const ConeState& S, int m, hipStream_t st);

// ---- the reduced-system algebra around the three solves of an IPM iteration (kktsystem.jl:135-215), device-resident
// konst = Delta_s_from_Delta_z_offset!(cones, ds, z) (coneops_compositecone.jl:185-202; zero :137-150, nonnegative
// coneops_nncone.jl:140-148, second-order coneops_socone.jl:241-268, PSD coneops_psdtrianglecone.jl:218-228), or a
// copy of s for the affine step; workz = konst - rhs_z.  Returns false if the cone list holds a kind it does not cover.
bool launch_sys_offset(const ConeDev& C, const ConeState& S, double* konst, double* workz, const double* ds,
                       const double* z, const double* rhs_z, int m, bool affine, hipStream_t st);
// y = Symmetric(P) x for the leading n x n block of K (rows / columns < n of the full-CSR image)
void launch_P_spmv(const SpmvDev& A, const double* Kval, const double* x, double* y, int n, hipStream_t st);
// out = a / (*alpha_div) + beta * b  (alpha_div null: a as is; beta from the device scalar if given, else beta_host):
// xi - x2 with xi = x / tau, and x1 + dtau x2
void launch_sys_axpby(double* out, const double* a, const double* alpha_div, const double* b, const double* beta,
                      double beta_host, int n, hipStream_t st);
struct DotPairs { const double* a[8]; const double* b[8]; int len[8]; int npairs; };
// out[p] = sum_i a_p[i] b_p[i], p < npairs (two-stage, fixed order); partial needs 8 * 64 doubles
void launch_dots(const DotPairs& P, double* partial, double* out, hipStream_t st);
// the scalars of kkt_solve! (kktsystem.jl:176-206): dots = {q.x1, b.z1, x.(P x1), xm.(P xm)}, cached = {q.x2, b.z2, x2.(P x2)}
// scal_in = {rhs_tau, rhs_kappa, var_tau, var_kappa}; out = {dtau, dkappa, tau_num, tau_den}
void launch_sys_scalars(const double* dots, const double* cached, const double* scal_in, double* out, hipStream_t st);
void launch_neg_sum(double* y, const double* a, const double* b, int n, hipStream_t st);      // y = -(a + b)
// fused forms of the above for kkt_solve!'s step recovery (fewer dependent launches, scalars by value)
// (pc nullable: P x2 too; P.npairs = 4, or 7 with the x2-only pairs {q.x2, b.z2, x2.(P x2)} behind them, which are then stored to `cached`)
void launch_P_spmv2(const SpmvDev& A, const double* Kval, const double* x1, const double* x, const double* x2, double tau,
                    double* pa, double* pb, double* xm_out, double* pc, int n, hipStream_t st);
void launch_pack_rhs_affine(double* b, const double* negq, const double* bb, const double* rhs_x, const double* s,
                            const double* rhs_z, int n, int m, int p, int ncol, hipStream_t st);
void launch_sys_step(double* dx, double* dz, const double* x1, const double* z1, const double* x2, const double* z2,
                     const double* scal, int n, int m, hipStream_t st);
// the dot products of P, the scalars of kkt_solve! (P.npairs = 4, or 7 with the x2-only pairs {q.x2, b.z2, x2.(P x2)} behind
// them, which are then stored to `cached`) and the step, the scalars formed inside the step kernel (every workgroup adds
// the partial sums up itself): two launches
void launch_dots_sys_step(const DotPairs& P, double* partial, double* cached, double rhs_tau, double rhs_kappa, double tau,
                          double kappa, double* out, double* dx, double* dz, const double* x1, const double* z1, const double* x2,
                          const double* z2, int n, int m, hipStream_t st, double* keep_x2 = nullptr, double* keep_z2 = nullptr);
// (keep_x2 / keep_z2: (x2, z2) copied there on the way -- it came out of this call's own solve and outlives the call)
void launch_neg_copy(double* y, const double* a, int n, hipStream_t st);                    // y = -a

// ---- the cone operations of the loop BETWEEN the solves, on device vectors (step_kernels.hip); symmetric cones only
// (zero, nonnegative, second-order, PSD side <= kPsdMaxDim) -- the caller refuses other handles.
constexpr int kStepGridCap = 2048;          // workgroups of the elementwise part (grid-stride beyond 2048 * 256 rows)
// slots of the step-length partials (one per elementwise workgroup, second-order cone and PSD cone); margins needs twice as many.
// The big PSD class keeps its slots at the END of every partials array, so that the others' positions and the fold order
// do not depend on it.
inline int step_partials(const ConeDev& C) { return kStepGridCap + C.nsoc + C.npsd + C.npsdb; }
// out = lambda o lambda (affine_ds!, coneops_compositecone.jl:153-165), and with `combined`
//       + (W^{-T} step_s) o (W (m_corr step_z)) - sigma_mu e (_combined_ds_shift_symmetric!, coneops_symmetric_common.jl:1-35)
void launch_step_ds(const ConeDev& C, const ConeState& S, double* out, const double* step_z, const double* step_s,
                    double sigma_mu, double m_corr, int m, bool combined, hipStream_t st);
// rec[0] = min(1, tau limit, kappa limit, every cone's alpha_z, alpha_s) (variables.jl:14-43 without max_step_fraction),
// handed to the host through `pub` by the finishing kernel
void launch_step_length(const ConeDev& C, const ConeState& S, const double* dz, const double* ds, const double* z,
                        const double* s, double step_tau, double step_kappa, double tau, double kappa, double* partial,
                        double* rec, const Publish& pub, int m, hipStream_t st);
// rec[0..1] = (min_margin, pos_margin) of v over all cones (coneops_compositecone.jl:49-63)
void launch_margins(const ConeDev& C, const double* v, double* partial, double* rec, const Publish& pub, int m, hipStream_t st);
// scaled_unit_shift! over all cones: v += a1 e, then (two) += a2 e; a primal zero cone's rows are set to 0
void launch_unit_shift(const ConeDev& C, double* v, double a1, double a2, bool two, bool primal, int m, hipStream_t st);

// ---- the same for handles that also hold exponential / power cones (three rows each; one lane per cone through
// exp_list / pow_list) and generalized power cones (coneops_genpowcone.jl): the symmetric rows by the
// kernels above, unchanged; then the lane-per-cone kernel where C.nexp + C.npow > 0; then, where C.ngp_small + C.ngp_big > 0,
// one wave per cone of gp_small / one workgroup per cone of gp_big, as the scaling kernel splits them
// slots of the barrier partials: elementwise workgroups, second-order cones, PSD cones, workgroups of the lane-per-cone part
// and a slot per generalized power cone (the step length's per-cone minima fit in the same array)
inline int barrier_partials(const ConeDev& C) { return 2 * kStepGridCap + C.nsoc + C.npsd + C.ngp_small + C.ngp_big + C.npsdb; }
// unit_initialization! of every cone (solver.jl:383-404, the asymmetric start) into s and z; a generalized power cone
// (coneops_genpowcone.jl:34-53): s_i = z_i = sqrt(1 + alpha_i) on its first dim1 rows, 0 behind
void launch_unit_initialization(const ConeDev& C, const ConeState& S, double* s, double* z, int m, hipStream_t st);
// launch_step_ds, then the exponential / power rows: a copy of s, and with `combined`
//       s + sigma_mu grad f*(z) - eta(step_s, m_corr step_z); z: the point the scaling was computed from
// the generalized power rows: a copy of s (coneops_genpowcone.jl:137-147), with `combined` s + sigma_mu grad f*(z), the
// stored gradient (:149-168)
void launch_step_ds_ns(const ConeDev& C, const ConeState& S, double* out, const double* step_z, const double* step_s,
                       const double* s, const double* z, double sigma_mu, double m_corr, int m, bool combined, hipStream_t st);
// launch_step_length (its record stays on the device), min(., 1 - sqrt(eps)), then every exponential / power / generalized
// power cone's backtrack_search (coneops_genpowcone.jl:186-207) from that common start; ns_partial: 2 * barrier_partials(C) doubles
void launch_step_length_ns(const ConeDev& C, const ConeState& S, const double* dz, const double* ds, const double* z,
                           const double* s, double step_tau, double step_kappa, double tau, double kappa, double backtrack_step,
                           double alpha_min, int trip_cap, double* partial, double* ns_partial, double* rec, const Publish& pub,
                           int m, hipStream_t st);
// rec[0..1] = (sum of compute_barrier over the cones -- a generalized power cone's barrier_dual + barrier_primal,
// coneops_genpowcone.jl:209-234 --, <z + alpha dz, s + alpha ds>); partial: 2 * barrier_partials(C) doubles
void launch_barrier(const ConeDev& C, const double* z, const double* s, const double* dz, const double* ds, double alpha,
                    double* partial, double* rec, const Publish& pub, int m, hipStream_t st);

// ---- residuals and termination scalars of a device-resident iterate (iterate_kernels.hip)
// What the pass walks of the image besides SpmvDev: the end of each row's walked prefix and the long ones among those
// prefixes (iterate_rows.hpp, computed on the host); long_partial: two doubles per chunk.
struct IterDev {
    const int64_t* rend;             // n + m
    int nlong, nchunks;
    const int* long_rows;
    const int64_t* long_chunk_ptr;
    const int64_t* chunk_q;
    double* long_partial;
};
// d == null: the four equilibration vectors read as ones
struct IterVecs {
    const double *x, *s, *z, *q, *b;
    double tau;
    double *rx, *rz, *rx_inf, *rz_inf, *Px;
    const double *d, *dinv, *e, *einv;
};
constexpr int kIterValues = 28;                      // four dot products, and three sums of squares for each of eight norms
constexpr int kIterGridCap = 2048;                   // workgroups of 32 rows (grid-stride beyond)
constexpr int kIterStride = kIterGridCap + 1;        // slots per value: one per workgroup and the long rows' one
inline size_t iterate_partials() { return (size_t)kIterValues * kIterStride; }
int iterate_grid(int n, int m);
// rec[0..11] = {q.x, b.z, s.z, x.Px, |d x|, |e z|, |einv s|, |dinv rx_inf|, |dinv Px|, |einv rz_inf|, |einv rz|, |dinv rx|}
// (2-norms), handed to the host through `pub` by the finishing kernel; A.val must be current (kkt_spmv)
void launch_iterate_residuals(const SpmvDev& A, const IterDev& I, const IterVecs& V, int n, int m, double* partial, double* rec,
                              const Publish& pub, hipStream_t st);
// ox = f rx (n), oz = f rz (m) in one launch; outputs may alias inputs
void launch_iterate_scale(double* ox, double* oz, const double* rx, const double* rz, double f, int n, int m, hipStream_t st);
// x += alpha dx (n); s += alpha ds, z += alpha dz (m) in one launch
void launch_iterate_add_step(double* x, double* s, double* z, const double* dx, const double* ds, const double* dz, double alpha,
                             int n, int m, hipStream_t st);

// ---- the same operations on a stack of independent member problems (hipkkt_kkt_system_set_problems): every
// scalar is an array over the members on the device, every reduction is segmented by member.  The tables are those of
// batch_plan.hpp on the device.  A workgroup of a reducing kernel belongs to ONE member (wg_mem) and leaves its partial
// values in its own slot; member b's slots are wg_ptr[b] .. wg_ptr[b + 1] - 1 (and the slots of its second-order cones,
// PSD cones and long rows, ranges as well), folded in slot order by the member's own finishing wave / workgroup: fixed
// layout, no floating-point atomic, and the number of launches does not depend on the number of members.
struct BatchChunksDev { const int* wg_mem; const int* wg_first; const int* wg_ptr; int nwg; };
struct BatchDev {
    int nb;
    const int *x_off, *z_off;        // nb + 1
    const int *xmem, *zmem;          // row -> member
    const int* cone_mem;             // cone -> member
    const int *soc_ptr, *psd_ptr;    // nb + 1: a member's range in ConeDev::soc_list / psd_list
    const double* degree;            // nb
    BatchChunksDev rows32, rows256, z256;
    const int *long_order, *long_ptr;    // the residual pass's long rows by member (positions in IterDev::long_rows)
};
// slots of the batched residual pass: one per 32-row workgroup and one per long row, kIterValues values each
inline size_t batch_residual_slots(const BatchDev& B, const IterDev& I) { return (size_t)B.rows32.nwg + (size_t)I.nlong; }
// rec[12 b .. 12 b + 11]: the record of launch_iterate_residuals over member b's rows, rx and rz formed with tau[b]
void launch_batch_residuals(const SpmvDev& A, const IterDev& I, const IterVecs& V, const BatchDev& B, const double* tau, int n,
                            int m, double* partial, double* rec, hipStream_t st);
// ox = (1 - sigma[b]) rx, oz = (1 - sigma[b]) rz on member b's rows
void launch_batch_scale(const BatchDev& B, double* ox, double* oz, const double* rx, const double* rz, const double* sigma, int n,
                        int m, hipStream_t st);
// x += alpha[b] dx, s += alpha[b] ds, z += alpha[b] dz on member b's rows; alpha[b] == 0: the rows are not written
void launch_batch_add_step(const BatchDev& B, double* x, double* s, double* z, const double* dx, const double* ds, const double* dz,
                           const double* alpha, int n, int m, hipStream_t st);
// launch_step_ds(combined) with member b's sigma_mu[b], m_corr[b] on its cones
void launch_batch_step_ds(const ConeDev& C, const ConeState& S, const BatchDev& B, double* out, const double* step_z,
                          const double* step_s, const double* sigma_mu, const double* m_corr, int m, hipStream_t st);
// slots of the batched step length / margins: elementwise workgroups, second-order cones, PSD cones (margins: twice)
inline size_t batch_step_slots(const ConeDev& C, const BatchDev& B) { return (size_t)B.z256.nwg + (size_t)C.nsoc + (size_t)C.npsd; }
// rec[b] = min(1, member b's tau / kappa limits, its cones' limits); scal = {step_tau, step_kappa, tau, kappa}, nb each
void launch_batch_step_length(const ConeDev& C, const ConeState& S, const BatchDev& B, const double* dz, const double* ds,
                              const double* z, const double* s, const double* scal, double* partial, double* rec, int m,
                              hipStream_t st);
// rec[2 b .. 2 b + 1] = member b's (min_margin, pos_margin) of v, then its branch of _shift_to_cone_interior! applied to its
// rows (shift: 3 nb doubles of work space)
void launch_batch_shift_to_interior(const ConeDev& C, const BatchDev& B, double* v, bool primal, double* partial, double* shift,
                                    double* rec, int m, hipStream_t st);
// the step recovery of kkt_solve! per member (kktsystem.jl:185-206): scal = {rhs_tau, rhs_kappa, var_tau, var_kappa}, nb
// each; out[2 b .. 2 b + 1] = (dtau_b, dkappa_b); (dx, dz) = (x1, z1) + dtau_b (x2, z2).  pa, pb, pc, xm: n doubles of work
// space each; partial: 7 slots per 256-row workgroup; dtau: nb doubles
void launch_batch_sys_step(const SpmvDev& A, const double* Kval, const BatchDev& B, const double* q, const double* bvec,
                           const double* x, const double* x1, const double* z1, const double* x2, const double* z2,
                           const double* scal, double* pa, double* pb, double* pc, double* xm, double* partial, double* dtau,
                           double* out, double* dx, double* dz, int n, int m, hipStream_t st);

// ---- the refinement rule per member (hipkkt_kkt_system_set_member_refinement; kktsolver_directldl.jl:389-449 applied to
// each member's rows of K's image).  The tables are those of batch_plan.hpp's BatchImagePlan on the device.
//   slots   3 arrays of nwg + nb partial maxima: ||e0||, ||b|| (first residual of a solve) and the candidate's ||e||;
//           workgroup w writes slot w + wg_mem[w], member b's long rows slot wg_ptr[b + 1] + b, so that member b folds
//           the adjacent slots wg_ptr[b] + b .. wg_ptr[b + 1] + b
//   state   slot r (4 nb doubles) after round r: member b's {active, rounds, bad, norme} at 4 b; normb: nb
//   info    4 nb: {rounds, norme, normb, bad} of the last round kernel, for ONE copy to the host
//   agg     two 64-bit words, zero between kernels: the members' leading workgroups count themselves in with agent-scope
//           integer atomics, the last one writes the aggregate (batch_kernels.hip: k_member_ir_round)
struct MemberIrDev {
    int nb, N, chunk, nwg;
    const int *wg_mem, *wg_first, *wg_ptr;
    const int *img_rows, *img_ptr;
    const int *long_order, *long_ptr;
    double *slots, *state, *normb, *info;
    unsigned long long* agg;
};
// e = b - K x, every row by residual_row_dot as in launch_residual (one column), and the members' partial maxima: into the
// ||e0|| and ||b|| slots (first) or the candidate's.  Two launches more when the image has long rows.
void launch_member_residual(const SpmvDev& A, const double* Kval, const MemberIrDev& M, const double* b, const double* x, double* e,
                            bool first, hipStream_t st);
// Round r per member: r == 0 the initial state from the first residual's slots; r >= 1 the accept / stop rule on the
// candidate dx (x <- dx on the rows of accepting members).  Then e = 0 on the rows of members that are not active, the
// members' state and info, and the aggregate {any active, most rounds, any bad, largest norme, abort} in readback.
// ONE launch whatever nb.  flag_in (nullable): the sweeps' abort word.
void launch_member_ir_round(const MemberIrDev& M, int r, const int* flag_in, double* x, const double* dx, double* e, double abstol,
                            double reltol, double stop_ratio, int max_iter, double* readback, hipStream_t st);
// the long rows' chunk sums of launch_residual alone (one column), for the member pass's own finish
void launch_residual_long_chunks(const SpmvDev& A, const double* Kval, const double* x, hipStream_t st);

// ---- the static regulariser and the failure words per member (hipkkt_kkt_system_set_member_status)
//   rowmem[i]   member of row i of K's image (batch_plan.hpp: BatchImagePlan::rowmem)
//   colmem[k]   member of column k of the factor's numbering (plan_column_members)
//   maxbits     nb + 1 words, zeroed by the caller before every update: the bit patterns of max |K_ii| per member, [nb] the stack's
//   eps_mem     nb: c0 + c1 max_b;  eps_col: N, eps_mem through colmem (FactorArgs::eps_col)
//   cone_fail   nb words, set by the cone scaling (ConeState::fail_mem);  piv_bad: nb words, set by the pivot scan
struct MemberStatusDev {
    int nb, N;
    const int *rowmem, *colmem;
    unsigned long long* maxbits;
    double *eps_mem, *eps_col;
    int *cone_fail, *piv_bad;
};
// two launches whatever nb: the segmented maximum of |K_ii| (diag: position of K_ii in Kval per image row), then eps_mem,
// eps_col and eps_top[0] = the largest eps_b
void launch_member_regularizer(const MemberStatusDev& M, const double* Kval, const int* diag, double c0, double c1, double* eps_top,
                               hipStream_t st);
// one launch behind the factorisation: piv_bad[colmem[k]] = 1 where Dinv[k] is not finite
void launch_member_pivot_scan(const MemberStatusDev& M, const double* Dinv, hipStream_t st);


// ---- Ruiz equilibration of (P, A, q, b) (problemdata.jl:133-221, mathutils.jl:129-269), all vectors on the device
struct EquilDev {
    int n, m;
    int64_t nnzP, nnzA;
    const int* Prow; const int* Pcol;   // per entry of triu(P)
    const int* Arow; const int* Acol;   // per entry of A
    double* Pval; double* Aval; double* q; double* b;
    double* d; double* e;               // cumulative scalings
    double* dwork; double* ework;       // this round's scalings
    double* scal;                       // [0] c, [1] ctmp, [2..] scratch
    double* partial;                    // 2 * 256 doubles
};
// one round of the loop at problemdata.jl:163-205
void launch_equil_round(const EquilDev& E, double scale_min, double scale_max, hipStream_t st);
// rectify_equilibration! (coneops_compositecone.jl:28-47; default coneops_defaults.jl:32-44, elementwise cones
// coneops_nncone.jl:8-17 / coneops_zerocone.jl:16-25) followed by the row re-scaling at problemdata.jl:212-216
void launch_equil_rectify(const EquilDev& E, const int* cone_kind, const int* cone_off, const int* cone_numel,
                          const int* elem_cone, int ncones, hipStream_t st);
// values[j] *= cscale * L[row[j]] * R[col[j]]   (lrscale!, mathutils.jl:231-244; data_updating.jl:181-194)
void launch_lrscale(double* values, const int* row, const int* col, int64_t nnz, const double* L, const double* R,
                    double cscale, hipStream_t st);

}  // namespace hipkkt
