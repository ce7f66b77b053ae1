// check_member_costs, build_entry_members and build_norm_slots (csrc/data_update.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer against brute force, on the partitions the member-cost kernels can go wrong at: nb = 1;
// members of 1, 63, 64, 65, 255, 256, 257 x rows in one stack; a member without z rows; a member without a stored entry
// of P; nb = 300 with two x rows each.  Every table goes in as an exact-size heap copy, so that a read past its end is the
// sanitizer's to see.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "data_update.hpp"

using namespace hipkkt;

static int g_fail = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "batch_equilibration_driver: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
    } while (0)

template <class T>
static T* dup(const std::vector<T>& v)
{
    T* p = v.empty() ? nullptr : (T*)std::malloc(v.size() * sizeof(T));
    for (size_t t = 0; t < v.size(); ++t) p[t] = v[t];
    return p;
}

// brute force: the member of a row is the last member whose offset is at or before it
static int member_of(const std::vector<int>& off, int row)
{
    int b = -1;
    for (size_t k = 0; k + 1 < off.size(); ++k)
        if (off[k] <= row && row < off[k + 1]) b = (int)k;
    return b;
}

struct Stack {
    int nb = 0, n = 0, m = 0;
    std::vector<int> x_off, z_off, xmem, zmem, Prow, Pcol;
};
// members of nx[b] x rows and nz[b] z rows; P of member b is tridiagonal (upper triangle, CSC order) unless noP[b]
static Stack make_stack(const std::vector<int>& nx, const std::vector<int>& nz, const std::vector<int>& noP)
{
    Stack S;
    S.nb = (int)nx.size();
    S.x_off.push_back(0); S.z_off.push_back(0);
    for (int b = 0; b < S.nb; ++b) {
        S.x_off.push_back(S.x_off.back() + nx[(size_t)b]);
        S.z_off.push_back(S.z_off.back() + nz[(size_t)b]);
    }
    S.n = S.x_off.back(); S.m = S.z_off.back();
    for (int b = 0; b < S.nb; ++b) {
        for (int i = 0; i < nx[(size_t)b]; ++i) S.xmem.push_back(b);
        for (int i = 0; i < nz[(size_t)b]; ++i) S.zmem.push_back(b);
        if (noP[(size_t)b]) continue;
        for (int c = S.x_off[(size_t)b]; c < S.x_off[(size_t)b + 1]; ++c) {
            if (c > S.x_off[(size_t)b]) { S.Prow.push_back(c - 1); S.Pcol.push_back(c); }
            S.Prow.push_back(c); S.Pcol.push_back(c);
        }
    }
    return S;
}

static void check_stack(const Stack& S)
{
    int *pr = dup(S.Prow), *pc = dup(S.Pcol), *xm = dup(S.xmem), *zm = dup(S.zmem);
    const int64_t nP = (int64_t)S.Prow.size();
    // ---- the member of every stored entry of P
    const EntryMembers E = build_entry_members(pr, pc, nP, xm, S.n, S.nb);
    CHECK(E.ok && E.bad == -1 && (int64_t)E.Pmem.size() == nP);
    for (int64_t t = 0; t < nP && E.ok; ++t) {
        const int want = member_of(S.x_off, S.Prow[(size_t)t]);
        CHECK(E.Pmem[(size_t)t] == want && want == member_of(S.x_off, S.Pcol[(size_t)t]));
    }
    // ---- the norms' words: x row i -> 2 b, z row i -> 2 b + 1
    const std::vector<int> slot = build_norm_slots(xm, S.n, zm, S.m, S.nb);
    CHECK(slot.size() == (size_t)S.n + (size_t)S.m);
    if (slot.size() == (size_t)S.n + (size_t)S.m) {
        for (int i = 0; i < S.n; ++i) CHECK(slot[(size_t)i] == 2 * member_of(S.x_off, i));
        for (int i = 0; i < S.m; ++i) CHECK(slot[(size_t)S.n + (size_t)i] == 2 * member_of(S.z_off, i) + 1);
        // a word is one run of the combined rows: a wave of 64 rows that holds one word may fold before its atomic
        std::vector<int> runs((size_t)2 * (size_t)S.nb, 0);
        for (size_t i = 0; i < slot.size(); ++i)
            if (i == 0 || slot[i] != slot[i - 1]) ++runs[(size_t)slot[i]];
        for (int b = 0; b < S.nb; ++b) {
            CHECK(runs[(size_t)2 * (size_t)b] == 1);
            CHECK(runs[(size_t)2 * (size_t)b + 1] == (S.z_off[(size_t)b + 1] > S.z_off[(size_t)b] ? 1 : 0));
        }
    }
    // ---- an entry that couples two members is reported, not passed on (nb >= 2, a member behind the first with a P)
    if (S.nb >= 2 && nP >= 1) {
        std::vector<int> badcol = S.Pcol;
        int64_t t = -1;
        for (int64_t u = 0; u < nP; ++u)
            if (member_of(S.x_off, S.Prow[(size_t)u]) != member_of(S.x_off, S.n - 1)) { t = u; break; }
        if (t >= 0) {
            badcol[(size_t)t] = S.n - 1;                                        // a column of the last member
            int* bc = dup(badcol);
            const EntryMembers B = build_entry_members(pr, bc, nP, xm, S.n, S.nb);
            std::free(bc);
            CHECK(!B.ok && B.bad == t);
        }
    }
    if (nP >= 1) {
        std::vector<int> badrow = S.Prow;
        badrow[(size_t)nP - 1] = S.n;                                           // past the last x row
        int* br = dup(badrow);
        EntryMembers B = build_entry_members(br, pc, nP, xm, S.n, S.nb);
        CHECK(!B.ok && B.bad == nP - 1);
        br[nP - 1] = -1;
        B = build_entry_members(br, pc, nP, xm, S.n, S.nb);
        CHECK(!B.ok && B.bad == nP - 1);
        std::free(br);
    }
    {
        // a member outside [0, nb) in a table: refused (an empty result), not used as an index
        std::vector<int> badmem = S.xmem;
        badmem[(size_t)S.n - 1] = S.nb;
        int* bm = dup(badmem);
        CHECK(build_norm_slots(bm, S.n, zm, S.m, S.nb).empty());
        if (nP >= 1 && S.Prow[(size_t)nP - 1] == S.n - 1) {
            const EntryMembers B = build_entry_members(pr, pc, nP, bm, S.n, S.nb);
            CHECK(!B.ok);
        }
        std::free(bm);
    }
    std::free(pr); std::free(pc); std::free(xm); std::free(zm);
}

static void check_costs(const std::vector<double>& c, int64_t want)
{
    double* p = dup(c);
    CHECK(check_member_costs(p, (int64_t)c.size()) == want);
    std::free(p);
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- the check of c[]
    check_costs({}, -1);
    check_costs({1.0}, -1);
    check_costs({1e-300, 1e300, 0.37}, -1);
    check_costs({5e-324}, -1);                                                  // (a subnormal is positive and finite)
    check_costs({0.0}, 0);
    check_costs({1.0, -0.0, 1.0}, 1);
    check_costs({1.0, 2.0, -1.0}, 2);
    check_costs({inf, 1.0}, 0);
    check_costs({1.0, -inf}, 1);
    check_costs({1.0, nan, 0.0}, 1);                                            // the first offender is named
    {
        std::vector<double> many(300, 2.0);
        check_costs(many, -1);
        many[299] = 0.0;
        check_costs(many, 299);
    }
    // ---- the partitions
    check_stack(make_stack({5}, {3}, {0}));                                     // nb = 1
    check_stack(make_stack({1}, {0}, {0}));                                     // ... of one x row and no z row
    check_stack(make_stack({1, 63, 64, 65, 255, 256, 257}, {2, 64, 63, 1, 257, 255, 256}, {0, 0, 0, 0, 0, 0, 0}));
    check_stack(make_stack({257, 256, 255, 65, 64, 63, 1}, {1, 1, 1, 1, 1, 1, 1}, {0, 0, 0, 0, 0, 0, 0}));
    check_stack(make_stack({64, 3, 64}, {5, 0, 7}, {0, 0, 0}));                 // a member without z rows, in the middle
    check_stack(make_stack({3, 4}, {0, 0}, {0, 0}));                            // no z rows at all
    check_stack(make_stack({4, 70, 5}, {2, 3, 0}, {0, 1, 0}));                  // a member without a stored entry of P
    check_stack(make_stack({2, 2}, {1, 1}, {1, 1}));                            // no P at all
    check_stack(make_stack(std::vector<int>(300, 2), std::vector<int>(300, 1), std::vector<int>(300, 0)));      // nb = 300
    if (g_fail) return 1;
    std::printf("BATCH EQUILIBRATION DRIVER OK\n");
    return 0;
}
