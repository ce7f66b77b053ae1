// plan_iterate_rows (csrc/iterate_rows.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer against a brute-force
// count: the end of every row's walked prefix and the long-row chunk lists, for prefix lengths 0, 1, kLongRow - 1,
// kLongRow, kLongRow + 1 and 3 kLongChunk + 1 in x rows and in z rows, and for rows whose whole-K length is long while
// the walked prefix is short (a PSD row: a handful of A entries in front of a dense Hs block).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "iterate_rows.hpp"
#include "launch_shapes.hpp"

using namespace hipkkt;

static int g_fail = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "iterate_rows_driver: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
    } while (0)

struct Image {
    int n = 0, m = 0;
    std::vector<int64_t> ptr{0};
    std::vector<int> col;
    void row(const std::vector<int>& c) { col.insert(col.end(), c.begin(), c.end()); ptr.push_back((int64_t)col.size()); }
};

// x row: np columns < n, then na columns in [n, n + m); z row: na columns < n, then `tail` columns >= n
static std::vector<int> x_row(int n, int m, int np, int na)
{
    std::vector<int> c;
    for (int j = 0; j < np; ++j) c.push_back(j % n);
    for (int j = 0; j < na; ++j) c.push_back(n + j % m);
    return c;
}
static std::vector<int> z_row(int n, int m, int na, int tail)
{
    std::vector<int> c;
    for (int j = 0; j < na; ++j) c.push_back(j % n);
    for (int j = 0; j < tail; ++j) c.push_back(n + j % (m + 7));          // (Hs block and expansion columns beyond n + m)
    return c;
}

static void check_against_brute_force(const Image& I, bool want_ok)
{
    const IterateRows R = plan_iterate_rows(I.n, I.m, I.ptr.data(), I.col.data(), kLongRow, kLongChunk);
    CHECK(R.prefix_ok == want_ok);
    if (!want_ok) return;
    const int rows = I.n + I.m;
    CHECK((int)R.rend.size() == (rows > 0 ? rows : 1));
    std::vector<int> want_long;
    for (int r = 0; r < rows; ++r) {
        int64_t walked = 0;                                                // brute force: count, do not search
        for (int64_t q = I.ptr[r]; q < I.ptr[r + 1]; ++q)
            if (r < I.n || I.col[q] < I.n) ++walked;
        CHECK(R.rend[r] == I.ptr[r] + walked);
        if (walked > kLongRow) want_long.push_back(r);
    }
    CHECK(R.long_rows == want_long);
    CHECK(R.long_chunk_ptr.size() == want_long.size() + 1 && R.long_chunk_ptr[0] == 0);
    CHECK(R.chunk_q.size() % 2 == 0 && R.long_chunk_ptr.back() == (int64_t)R.chunk_q.size() / 2);
    for (size_t t = 0; t < want_long.size(); ++t) {
        const int r = want_long[t];
        int64_t at = I.ptr[r];
        const int64_t c0 = R.long_chunk_ptr[t], c1 = R.long_chunk_ptr[t + 1];
        CHECK(c1 - c0 == (R.rend[r] - I.ptr[r] + kLongChunk - 1) / kLongChunk);
        for (int64_t c = c0; c < c1; ++c) {
            CHECK(R.chunk_q[2 * c] == at);
            const int64_t len = R.chunk_q[2 * c + 1] - R.chunk_q[2 * c];
            CHECK(len > 0 && len <= kLongChunk && (c + 1 == c1 || len == kLongChunk));
            at = R.chunk_q[2 * c + 1];
        }
        CHECK(at == R.rend[r]);
    }
}

int main()
{
    const int edges[6] = {0, 1, kLongRow - 1, kLongRow, kLongRow + 1, 3 * kLongChunk + 1};
    {
        // every edge as the walked prefix of a z row (short and long tails behind it) and of an x row (all P, all A', mixed)
        Image I;
        I.n = 7000; I.m = 6200;
        std::vector<std::vector<int>> xr, zr;
        for (int L : edges) {
            xr.push_back(x_row(I.n, I.m, L, 0));
            xr.push_back(x_row(I.n, I.m, 0, L < I.m ? L : 0));
            xr.push_back(x_row(I.n, I.m, L / 2, L - L / 2));
            zr.push_back(z_row(I.n, I.m, L, 1));
            zr.push_back(z_row(I.n, I.m, L, 1176 + 3));
            zr.push_back(z_row(I.n, I.m, L, 0));
        }
        // whole-K length long, walked prefix short: PSD(48)-like rows, and a sparse cone's expansion columns behind them
        zr.push_back(z_row(I.n, I.m, 3, kLongRow + 100));
        zr.push_back(z_row(I.n, I.m, 0, 3 * kLongChunk + 1));
        zr.push_back(z_row(I.n, I.m, kLongRow, kLongRow + 1));
        for (int r = 0; r < I.n; ++r) I.row(r < (int)xr.size() ? xr[r] : std::vector<int>{r});
        for (int r = 0; r < I.m; ++r) I.row(r < (int)zr.size() ? zr[r] : std::vector<int>{r % I.n, I.n + r});
        I.row({0});                                                       // an expansion row behind n + m: never looked at
        check_against_brute_force(I, true);
    }
    {
        Image I;                                                          // m = 0
        I.n = 3; I.m = 0;
        I.row({0}); I.row({0, 1, 2}); I.row({});
        check_against_brute_force(I, true);
    }
    {
        Image I;                                                          // n = 1, m = 1
        I.n = 1; I.m = 1;
        I.row({0, 1}); I.row({0, 1});
        check_against_brute_force(I, true);
    }
    {
        Image I;                                                          // nothing at all
        check_against_brute_force(I, true);
    }
    {
        Image I;                                                          // a column of A behind the Hs entry: not a prefix
        I.n = 2; I.m = 2;
        I.row({0, 2}); I.row({1, 3}); I.row({0, 2, 1}); I.row({1, 3});
        check_against_brute_force(I, false);
    }
    {
        Image I;                                                          // an x row reaching into the expansion block
        I.n = 2; I.m = 1;
        I.row({0, 2, 3}); I.row({1}); I.row({0, 2});
        check_against_brute_force(I, false);
    }
    if (g_fail) return 1;
    std::printf("ITERATE ROWS DRIVER OK\n");
    return 0;
}
