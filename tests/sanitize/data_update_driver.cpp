// check_update_index and build_entry_tables (csrc/data_update.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer
// against brute force: the position check of an (index, value) update -- empty, k = 1, first and last position, -1, len,
// a repeat at the ends and in the middle, unsorted input, on both of its paths (dense marks / sorted copy) -- and the
// row and column of every stored entry of P and A from K's pattern, for a P with an empty column, an A with an empty
// row, n = 0 and m = 0.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "data_update.hpp"

using namespace hipkkt;

static int g_fail = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "data_update_driver: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
    } while (0)

// brute force: the first place out of range, else the first place whose value occurred at an earlier place
static IndexCheck brute(const std::vector<int64_t>& idx, int64_t len)
{
    IndexCheck out;
    for (size_t t = 0; t < idx.size(); ++t)
        if (idx[t] < 0 || idx[t] >= len) { out.fault = IndexFault::OutOfRange; out.pos = (int64_t)t; out.value = idx[t]; return out; }
    for (size_t t = 0; t < idx.size(); ++t)
        for (size_t s = 0; s < t; ++s)
            if (idx[s] == idx[t]) { out.fault = IndexFault::Repeated; out.pos = (int64_t)t; out.value = idx[t]; return out; }
    return out;
}

static void check_index(const std::vector<int64_t>& idx, int64_t len, IndexFault want, int64_t want_pos)
{
    // an exact-size heap copy, so that a read past the end is the sanitizer's to see
    int64_t* p = idx.empty() ? nullptr : (int64_t*)std::malloc(idx.size() * sizeof(int64_t));
    for (size_t t = 0; t < idx.size(); ++t) p[t] = idx[t];
    const IndexCheck got = check_update_index(p, (int64_t)idx.size(), len), ref = brute(idx, len);
    std::free(p);
    CHECK(got.fault == want && got.pos == want_pos);
    CHECK(got.fault == ref.fault && got.pos == ref.pos);
    if (got.fault != IndexFault::None) CHECK(got.value == idx[(size_t)got.pos] && got.value == ref.value);
}

// K = [P A'; A -I] (triu CSC) from dense 0/1 patterns, with mapP / mapA in the matrices' own CSC order
struct Built {
    int n, m, N;
    std::vector<int64_t> colptr;
    std::vector<int> rowval, mapP, mapA, Prow, Pcol, Arow, Acol;
};
static Built build(int n, int m, const std::vector<std::vector<int>>& P, const std::vector<std::vector<int>>& A)
{
    Built B;
    B.n = n; B.m = m; B.N = n + m;
    B.colptr.push_back(0);
    std::vector<std::vector<int>> placeP((size_t)n, std::vector<int>((size_t)n, -1)), placeA((size_t)m, std::vector<int>((size_t)n, -1));
    for (int c = 0; c < n; ++c) {                                          // columns of P (upper triangle)
        for (int r = 0; r <= c; ++r)
            if (P[(size_t)r][(size_t)c]) { placeP[(size_t)r][(size_t)c] = (int)B.rowval.size(); B.rowval.push_back(r); }
        B.colptr.push_back((int64_t)B.rowval.size());
    }
    for (int i = 0; i < m; ++i) {                                          // column n + i: row i of A, then the -Hs diagonal
        for (int j = 0; j < n; ++j)
            if (A[(size_t)i][(size_t)j]) { placeA[(size_t)i][(size_t)j] = (int)B.rowval.size(); B.rowval.push_back(j); }
        B.rowval.push_back(n + i);
        B.colptr.push_back((int64_t)B.rowval.size());
    }
    for (int c = 0; c < n; ++c)                                            // P's CSC order
        for (int r = 0; r <= c; ++r)
            if (P[(size_t)r][(size_t)c]) { B.mapP.push_back(placeP[(size_t)r][(size_t)c]); B.Prow.push_back(r); B.Pcol.push_back(c); }
    for (int j = 0; j < n; ++j)                                            // A's CSC order
        for (int i = 0; i < m; ++i)
            if (A[(size_t)i][(size_t)j]) { B.mapA.push_back(placeA[(size_t)i][(size_t)j]); B.Arow.push_back(i); B.Acol.push_back(j); }
    return B;
}
static void check_tables(const Built& B)
{
    // exact-size heap copies again
    auto dup = [](const std::vector<int>& v) {
        int* p = v.empty() ? nullptr : (int*)std::malloc(v.size() * sizeof(int));
        for (size_t t = 0; t < v.size(); ++t) p[t] = v[t];
        return p;
    };
    int *rv = dup(B.rowval), *mp = dup(B.mapP), *ma = dup(B.mapA);
    const EntryTables T = build_entry_tables(B.n, B.m, B.N, B.colptr.data(), rv, mp, (int64_t)B.mapP.size(), ma, (int64_t)B.mapA.size());
    std::free(rv); std::free(mp); std::free(ma);
    CHECK(T.ok && T.bad == -1);
    CHECK(T.Prow == B.Prow && T.Pcol == B.Pcol && T.Arow == B.Arow && T.Acol == B.Acol);
}

int main()
{
    // ---- the position check: dense marks (k >= len / 16) and the sorted copy (k < len / 16) take the same cases
    for (int64_t len : {(int64_t)8, (int64_t)1000}) {
        check_index({}, len, IndexFault::None, -1);
        check_index({0}, len, IndexFault::None, -1);
        check_index({len - 1}, len, IndexFault::None, -1);
        check_index({len - 1, 0}, len, IndexFault::None, -1);
        check_index({5, 2, 7, 0}, len, IndexFault::None, -1);                // unsorted: accepted
        check_index({-1}, len, IndexFault::OutOfRange, 0);
        check_index({len}, len, IndexFault::OutOfRange, 0);
        check_index({0, len - 1, len}, len, IndexFault::OutOfRange, 2);
        check_index({3, -1, 3}, len, IndexFault::OutOfRange, 1);             // out of range is named before a repeat
        check_index({4, 4}, len, IndexFault::Repeated, 1);
        check_index({0, 1, 2, 0}, len, IndexFault::Repeated, 3);             // a repeat at the ends
        check_index({1, 3, 3, 5}, len, IndexFault::Repeated, 2);             // ... in the middle
        check_index({6, 1, 2, 1, 6}, len, IndexFault::Repeated, 3);          // two repeats: the earlier second occurrence
        check_index({7, 7, 7}, len, IndexFault::Repeated, 1);
    }
    {
        std::vector<int64_t> all;                                            // every position once, descending; then one too many
        for (int64_t j = 99; j >= 0; --j) all.push_back(j);
        check_index(all, 100, IndexFault::None, -1);
        all.push_back(50);
        check_index(all, 100, IndexFault::Repeated, 100);
    }
    check_index({}, 0, IndexFault::None, -1);
    check_index({0}, 0, IndexFault::OutOfRange, 0);
    // (index = NULL is the vector form: nothing to check)
    CHECK(check_update_index(nullptr, 5, 5).fault == IndexFault::None);

    // ---- the entry tables
    {
        // P with an empty column (column 1) and off-diagonal entries; A with an empty row (row 2)
        const std::vector<std::vector<int>> P = {{1, 0, 1, 0}, {0, 0, 0, 1}, {0, 0, 1, 1}, {0, 0, 0, 1}};
        const std::vector<std::vector<int>> A = {{1, 0, 0, 1}, {0, 1, 0, 0}, {0, 0, 0, 0}, {1, 1, 1, 1}, {0, 0, 1, 0}};
        check_tables(build(4, 5, P, A));
    }
    check_tables(build(3, 0, {{1, 1, 0}, {0, 1, 1}, {0, 0, 1}}, {}));       // m = 0
    check_tables(build(0, 3, {}, {{}, {}, {}}));                            // n = 0: K is the -Hs diagonal alone
    check_tables(build(0, 0, {}, {}));
    check_tables(build(2, 2, {{0, 0}, {0, 0}}, {{1, 0}, {0, 1}}));          // no P at all
    {
        // a map that points outside its block is reported, not followed
        Built B = build(2, 2, {{1, 1}, {0, 1}}, {{1, 0}, {0, 1}});
        std::vector<int> badP = B.mapP, badA = B.mapA;
        badP[1] = B.mapA[0];                                                 // an A entry among P's
        EntryTables T = build_entry_tables(B.n, B.m, B.N, B.colptr.data(), B.rowval.data(), badP.data(), (int64_t)badP.size(),
                                           B.mapA.data(), (int64_t)B.mapA.size());
        CHECK(!T.ok && T.bad == 1);
        badA[1] = (int)B.rowval.size();                                      // past the end of K
        T = build_entry_tables(B.n, B.m, B.N, B.colptr.data(), B.rowval.data(), B.mapP.data(), (int64_t)B.mapP.size(), badA.data(),
                               (int64_t)badA.size());
        CHECK(!T.ok && T.bad == 1);
        badA[1] = -1;
        T = build_entry_tables(B.n, B.m, B.N, B.colptr.data(), B.rowval.data(), B.mapP.data(), (int64_t)B.mapP.size(), badA.data(),
                               (int64_t)badA.size());
        CHECK(!T.ok && T.bad == 1);
    }
    if (g_fail) return 1;
    std::printf("DATA UPDATE DRIVER OK\n");
    return 0;
}
