// The partition of a block-diagonal stack into its independent member problems (hipkkt_kkt_system_set_problems), checked
// and tabulated once on the host as host-only code (no HIP header, no device), like iterate_rows.cpp for the row plan:
//   the check      offsets start at 0, do not decrease and end at n and m; every member owns an x row; every cone lies in one
//                  member's z range; every stored entry of P and of A has its row and its column in the same member
//   row -> member  xmem (n), zmem (m); cone -> member (cone_mem); a member's second-order and PSD cones as a range of the
//                  handle's soc_list / psd_list (both ascending in cone order, as the cones of a member are contiguous)
//   workgroups     the segmented reductions give every workgroup ONE member: a member's rows are cut into chunks, a chunk
//                  is a workgroup, and the workgroups of member b are wg_ptr[b] .. wg_ptr[b + 1] - 1 -- so a member's
//                  partial sums sit side by side and are folded in workgroup order by that member's finishing wave
//   long rows      the rows of K's image that the residual pass hands to chunk workgroups, grouped by member
// A member's "combined" rows are its x rows followed by its z rows (local index r: x row x_off[b] + r for r < nx, else z
// row z_off[b] + r - nx).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace hipkkt {

constexpr int kBatchRowsResidual = 32;     // combined rows per workgroup of the residual pass (eight lanes per row)
constexpr int kBatchRowsDots = 256;        // combined rows per workgroup of the step recovery's dot products
constexpr int kBatchRowsCone = 256;        // z rows per workgroup of the elementwise step-length / margins part

struct BatchChunks {
    std::vector<int> wg_mem;               // per workgroup: its member
    std::vector<int> wg_first;             // per workgroup: local index of its first row
    std::vector<int> wg_ptr;               // nb + 1
};

struct BatchCone { int kind, off, numel, dim; };       // HIPKKT_CONE_* kind; dim: matrix side of a PSD cone

struct BatchPlan {
    int nb = 0;
    std::vector<int> x_off, z_off;         // nb + 1
    std::vector<int> xmem, zmem;           // n, m
    std::vector<int> cone_mem;             // per cone
    std::vector<int> soc_ptr, psd_ptr;     // nb + 1: ranges in the lists of second-order / PSD cones
    std::vector<double> degree;            // nb: sum of the member's cone degrees (nonnegative: numel, second-order: 1, PSD: side)
    BatchChunks rows32, rows256, z256;     // combined rows by 32 and by 256, z rows by 256
    std::vector<int> long_order;           // positions in long_rows, grouped by member (ascending inside a member)
    std::vector<int> long_ptr;             // nb + 1
};

// chunks of `chunk` rows over members of nx[b] + nz[b] rows (either offset array may be null: no rows of that kind)
BatchChunks plan_batch_chunks(int nb, const int* x_off, const int* z_off, int chunk);

// colptr / rowval: K as upper-triangular CSC (columns j < n hold P, column n + i holds row i of A in its rows < n; rows
// >= n and columns >= n + m are not looked at).  long_rows: nlong rows of the image in [0, n + m), ascending.
// Returns "" and fills `out`, or the text of the refusal (which names the offending member or entry); `out` is then unspecified.
std::string plan_batch(int n, int m, int64_t nb, const int64_t* x_off, const int64_t* z_off, const BatchCone* cones, int ncones,
                       const int64_t* colptr, const int* rowval, const int* long_rows, int nlong, BatchPlan& out);

// ---- the member refinement rule (hipkkt_kkt_system_set_member_refinement): the partition carried over to ALL N = n + m + p
// rows of K's image, where the refinement's residual e = b - K x lives.  Member b's image rows are its x rows, its z rows
// and the expansion rows n + m + pcol .. n + m + pcol + pwidth - 1 of its sparse second-order cones, which lie far from
// its other rows; so the rows are listed by member (img_rows, ascending inside a member) and a workgroup walks a chunk of
// that list:
//   workgroups     workgroup w belongs to member wg.wg_mem[w] and takes the positions wg.wg_first[w] .. wg.wg_first[w] +
//                  chunk - 1 of img_rows (cut at img_ptr[b + 1]; wg_first is a position in img_rows here, not a local
//                  index); member b's workgroups are wg.wg_ptr[b] .. wg.wg_ptr[b + 1] - 1
//   slots          member b folds the slots wg.wg_ptr[b] + b .. wg.wg_ptr[b + 1] + b: one per workgroup (workgroup w
//                  writes slot w + wg_mem[w]) and, last, one for its long rows -- side by side, nwg + nb in all
//   long rows      positions in the residual pass's list of long rows (all of the image this time), grouped by member
struct BatchImageCone { int pcol, pwidth; };           // per cone, as in ConeInfo (pwidth 0: no expansion rows)

struct BatchImagePlan {
    int nb = 0, N = 0, chunk = 0;
    std::vector<int> rowmem;               // N: row of the image -> member
    std::vector<int> img_rows;             // N: the rows by member
    std::vector<int> img_ptr;              // nb + 1
    BatchChunks wg;
    std::vector<int> long_order;           // positions in long_rows, grouped by member (ascending inside a member)
    std::vector<int> long_ptr;             // nb + 1
};

// B: a plan of plan_batch for the same n, m.  cones: one entry per cone of B.cone_mem.  long_rows: nlong rows of the image
// in [0, n + m + p), ascending.  chunk >= 1: rows per workgroup.  Returns "" and fills `out`, or the text of the refusal.
std::string plan_batch_image(int n, int m, int p, const BatchPlan& B, const BatchImageCone* cones, int ncones, const int* long_rows,
                             int nlong, int chunk, BatchImagePlan& out);

// ---- per-member regulariser and pivot status (hipkkt_kkt_system_set_member_status): column k of the factor's numbering
// holds row perm[k] of the image, so colmem[k] = rowmem[perm[k]].  perm must be a permutation of 0 .. N - 1 (nperm = N
// entries) and rowmem must have N entries in [0, nb).  Returns "" and fills colmem, or the text of the refusal.
std::string plan_column_members(int N, int nb, const int* perm, size_t nperm, const int* rowmem, size_t nrowmem, std::vector<int>& colmem);

}  // namespace hipkkt
