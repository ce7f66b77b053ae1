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

// packed sweep records (kernels.hpp: SolveHdr): bytes of a record's header
constexpr int kSolveHdrBytes = 64;
struct RecSeg {                  // the records of one kernel launch's fronts, by size class: 0 block-class, 1 one-wave, 2 tiny
    int64_t off[3];              // byte offset in SolveArgs::recs of the class's first record
    int stride[3];               // bytes per record
    int fmax[3];                 // row slots per record (a multiple of 4)
};
static_assert(sizeof(RecSeg) == 48, "RecSeg layout (a kernel argument)");

}  // namespace hipkkt
