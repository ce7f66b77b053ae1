// What the iterate-residual kernel (iterate_kernels.hip) walks of the full-CSR image of K, decided once on the host at
// handle creation (hipkkt_kkt_create*, next to SpmvDev::pend: the pattern is fixed there) as host-only code (no HIP header,
// no device), like schedule.cpp for the launch plan:
//   rows i < n        the whole row: its P entries (columns < n, a prefix ending at SpmvDev::pend) and its A' entries
//                     (columns in [n, n + m)); an x row has no other column
//   rows n + i        the entries with column < n only -- row i of A.  They are a prefix of the row (kkt_assembly.cpp
//                     puts A' first into column n + i, and the image takes a row's own column first); the -Hs diagonal
//                     and blocks and the expansion columns of sparse second-order and generalized power cones lie behind
//                     it and are never walked
// and which of those walked prefixes are long (more than long_row entries: cut into chunks of long_chunk, combined in
// chunk order, as launch_residual does for whole rows).
#pragma once
#include <cstdint>
#include <vector>

namespace hipkkt {

struct IterateRows {
    std::vector<int64_t> rend;             // n + m: end of the walked prefix of each row (rend[r] - ptr[r] entries)
    std::vector<int> long_rows;            // rows whose walked prefix is longer than long_row, ascending
    std::vector<int64_t> long_chunk_ptr;   // long_rows.size() + 1: chunk range of each long row
    std::vector<int64_t> chunk_q;          // two per chunk: [begin, end) in the image
    bool prefix_ok = true;                 // false: a walked range holds a column it must not (the layout changed)
};

// ptr (n + m + 1 entries at least), col: the image.  Columns of a z row behind its prefix are not looked at for
// prefix_ok beyond "no column < n follows the first column >= n".
IterateRows plan_iterate_rows(int n, int m, const int64_t* ptr, const int* col, int long_row, int long_chunk);

}  // namespace hipkkt
