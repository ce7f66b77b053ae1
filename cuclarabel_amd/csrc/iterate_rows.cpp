// See iterate_rows.hpp.  Host-only: compiled with -x c++, and by the sanitizer driver of tests/sanitize.
#include "iterate_rows.hpp"

#include <algorithm>

namespace hipkkt {

IterateRows plan_iterate_rows(int n, int m, const int64_t* ptr, const int* col, int long_row, int long_chunk)
{
    IterateRows R;
    const int rows = n + m;
    R.rend.assign((size_t)std::max(rows, 1), 0);
    R.long_chunk_ptr.push_back(0);
    for (int r = 0; r < rows; ++r) {
        const int64_t q0 = ptr[r], q1 = ptr[r + 1];
        int64_t end = q1;
        if (r < n) {
            // P entries first, then A': columns never fall back below n, and none reaches the expansion block
            bool behind = false;
            for (int64_t q = q0; q < q1; ++q) {
                const int c = col[q];
                if (c < 0 || c >= rows) R.prefix_ok = false;
                if (c >= n) behind = true;
                else if (behind) R.prefix_ok = false;
            }
        } else {
            end = q0;
            while (end < q1 && col[end] >= 0 && col[end] < n) ++end;
            for (int64_t q = end; q < q1; ++q)
                if (col[q] < n) R.prefix_ok = false;
        }
        R.rend[(size_t)r] = end;
        if (end - q0 <= long_row) continue;
        R.long_rows.push_back(r);
        for (int64_t q = q0; q < end; q += long_chunk) {
            R.chunk_q.push_back(q);
            R.chunk_q.push_back(std::min<int64_t>(q + long_chunk, end));
        }
        R.long_chunk_ptr.push_back((int64_t)R.chunk_q.size() / 2);
    }
    return R;
}

}  // namespace hipkkt
