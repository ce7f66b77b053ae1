// See data_update.hpp.
#include "data_update.hpp"

#include <algorithm>
#include <cmath>

namespace hipkkt {

IndexCheck check_update_index(const int64_t* index, int64_t k, int64_t len)
{
    IndexCheck out;
    if (k <= 0 || !index) return out;
    for (int64_t t = 0; t < k; ++t)
        if (index[t] < 0 || index[t] >= len) {
            out.fault = IndexFault::OutOfRange;
            out.pos = t;
            out.value = index[t];
            return out;
        }
    // a repeat: the place in index[] that was seen first marks every position.  Dense marks where the update covers a
    // fair part of the vector, a sorted copy otherwise (a two-entry update of a million-entry matrix allocates two words).
    int64_t first_repeat = -1;
    if (k >= len / 16) {
        std::vector<unsigned char> seen((size_t)len, 0);
        for (int64_t t = 0; t < k; ++t) {
            if (seen[(size_t)index[t]]) { first_repeat = t; break; }
            seen[(size_t)index[t]] = 1;
        }
    } else {
        std::vector<std::pair<int64_t, int64_t>> byval((size_t)k);
        for (int64_t t = 0; t < k; ++t) byval[(size_t)t] = {index[t], t};
        std::sort(byval.begin(), byval.end());
        for (int64_t t = 1; t < k; ++t)
            if (byval[(size_t)t].first == byval[(size_t)t - 1].first &&
                (first_repeat < 0 || byval[(size_t)t].second < first_repeat))
                first_repeat = byval[(size_t)t].second;    // (sorted by (value, place): the later place of each pair)
    }
    if (first_repeat >= 0) {
        out.fault = IndexFault::Repeated;
        out.pos = first_repeat;
        out.value = index[first_repeat];
    }
    return out;
}

EntryTables build_entry_tables(int n, int m, int N, const int64_t* colptr, const int* rowval, const int* mapP, int64_t nP,
                               const int* mapA, int64_t nA)
{
    EntryTables T;
    T.Prow.resize((size_t)nP); T.Pcol.resize((size_t)nP);
    T.Arow.resize((size_t)nA); T.Acol.resize((size_t)nA);
    const int64_t nnzK = N > 0 ? colptr[N] : 0;
    // the column of a K entry: the last column that starts at or before it
    auto col_of = [&](int64_t q) { return (int)(std::upper_bound(colptr, colptr + N + 1, q) - colptr) - 1; };
    for (int64_t t = 0; t < nP; ++t) {
        const int64_t q = mapP[t];
        if (q < 0 || q >= nnzK) { T.ok = false; T.bad = t; return T; }
        const int c = col_of(q), r = rowval[q];
        if (r < 0 || r > c || c >= n) { T.ok = false; T.bad = t; return T; }
        T.Prow[(size_t)t] = r;
        T.Pcol[(size_t)t] = c;
    }
    for (int64_t t = 0; t < nA; ++t) {
        const int64_t q = mapA[t];
        if (q < 0 || q >= nnzK) { T.ok = false; T.bad = t; return T; }
        const int c = col_of(q), r = rowval[q];
        if (r < 0 || r >= n || c < n || c >= n + m) { T.ok = false; T.bad = t; return T; }
        T.Arow[(size_t)t] = c - n;
        T.Acol[(size_t)t] = r;
    }
    return T;
}

int64_t check_member_costs(const double* c, int64_t nb)
{
    for (int64_t b = 0; b < nb; ++b)
        if (!(c[b] > 0.0) || !std::isfinite(c[b])) return b;
    return -1;
}

EntryMembers build_entry_members(const int* Prow, const int* Pcol, int64_t nP, const int* xmem, int n, int nb)
{
    EntryMembers E;
    E.Pmem.resize((size_t)nP);
    for (int64_t t = 0; t < nP; ++t) {
        const int r = Prow[t], c = Pcol[t];
        if (r < 0 || r >= n || c < 0 || c >= n) { E.ok = false; E.bad = t; return E; }
        const int b = xmem[r];
        if (b < 0 || b >= nb || xmem[c] != b) { E.ok = false; E.bad = t; return E; }
        E.Pmem[(size_t)t] = b;
    }
    return E;
}

std::vector<int> build_norm_slots(const int* xmem, int n, const int* zmem, int m, int nb)
{
    std::vector<int> slot((size_t)n + (size_t)m);
    for (int i = 0; i < n; ++i) {
        if (xmem[i] < 0 || xmem[i] >= nb) return {};
        slot[(size_t)i] = 2 * xmem[i];
    }
    for (int i = 0; i < m; ++i) {
        if (zmem[i] < 0 || zmem[i] >= nb) return {};
        slot[(size_t)n + (size_t)i] = 2 * zmem[i] + 1;
    }
    return slot;
}

}  // namespace hipkkt
