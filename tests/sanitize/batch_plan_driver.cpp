// plan_batch (csrc/batch_plan.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: the tables of
// hipkkt_kkt_system_set_problems -- row -> member, cone -> member, the members' ranges in the cone lists, the degrees, the
// assignment of workgroups to (member, chunk) for all three chunkings, the long rows by member -- against brute force on
// random partitions, and every refusal with the member or entry it must name.
// With arguments: each names a text file that holds a stack (tests/test_batch_plan_host.py writes those of
// problems.block_diagonal); every one must be accepted and its tables must pass the same brute-force check.
//   file: n m nb / x_off (nb + 1) / z_off (nb + 1) / ncones / kind off numel dim per cone / colptr (n + m + 1) / rowval
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "batch_plan.hpp"

using namespace hipkkt;

static int g_fail = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "batch_plan_driver: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
    } while (0)

struct Stack {
    int n = 0, m = 0;
    std::vector<int64_t> x_off{0}, z_off{0};
    std::vector<BatchCone> cones;
    std::vector<int64_t> colptr;           // n + m + 1: upper-triangular CSC of K's first n + m columns
    std::vector<int> rowval;
    std::vector<int> long_rows;
    int64_t nb() const { return (int64_t)x_off.size() - 1; }
    std::string plan(BatchPlan& P) const
    {
        return plan_batch(n, m, nb(), x_off.data(), z_off.data(), cones.data(), (int)cones.size(), colptr.data(), rowval.data(),
                          long_rows.data(), (int)long_rows.size(), P);
    }
};

// member sizes (nx, nz) -> a stack with random P and A entries inside the members, random cones that tile every member's
// z range (second-order cones of 2 and 3 rows, PSD cones of side 1, 2 and 3 among them) and a few long rows
static Stack make_stack(const std::vector<std::pair<int, int>>& sizes, std::mt19937& rng)
{
    Stack S;
    for (auto& s : sizes) { S.x_off.push_back(S.x_off.back() + s.first); S.z_off.push_back(S.z_off.back() + s.second); }
    S.n = (int)S.x_off.back();
    S.m = (int)S.z_off.back();
    std::vector<std::vector<int>> cols((size_t)S.n + S.m);
    for (size_t b = 0; b < sizes.size(); ++b) {
        const int x0 = (int)S.x_off[b], nx = sizes[b].first, z0 = (int)S.z_off[b], nz = sizes[b].second;
        for (int j = 0; j < nx; ++j) {
            if (j > 0 && rng() % 2) cols[(size_t)x0 + j].push_back(x0 + (int)(rng() % (unsigned)j));     // P(i, j), i < j
            if (j > 1 && rng() % 4 == 0) cols[(size_t)x0 + j].push_back(x0);                            // the member's first row
            cols[(size_t)x0 + j].push_back(x0 + j);
        }
        for (int r = 0; r < nz; ++r) {
            const int k = 1 + (int)(rng() % 3);
            for (int t = 0; t < k; ++t) cols[(size_t)S.n + z0 + r].push_back(x0 + (int)(rng() % (unsigned)nx));
            if (rng() % 8 == 0) cols[(size_t)S.n + z0 + r].push_back(x0 + nx - 1);                       // ... and its last column
            cols[(size_t)S.n + z0 + r].push_back(S.n + z0 + r);                                          // -Hs diagonal
        }
        int at = z0;
        while (at < z0 + nz) {
            const int left = z0 + nz - at;
            const int pick = (int)(rng() % 8);
            BatchCone c{1, at, left, left};
            if (pick == 0) { c.kind = 0; c.numel = 1 + (int)(rng() % 4); }
            else if (pick == 1) { c.kind = 2; c.numel = 2; }
            else if (pick == 2) { c.kind = 2; c.numel = 3; }
            else if (pick == 3) { c.kind = 3; c.dim = 1 + (int)(rng() % 3); c.numel = c.dim * (c.dim + 1) / 2; }
            else if (pick == 4) { c.kind = 1; c.numel = 1 + (int)(rng() % 40); }
            if (c.numel > left) { c.kind = 1; c.numel = left; }
            if (c.kind != 3) c.dim = c.numel;
            S.cones.push_back(c);
            at += c.numel;
        }
    }
    S.colptr.push_back(0);
    for (auto& c : cols) {
        S.rowval.insert(S.rowval.end(), c.begin(), c.end());
        S.colptr.push_back((int64_t)S.rowval.size());
    }
    for (int r = 0; r < S.n + S.m; ++r)
        if (rng() % 97 == 0 || r == S.n - 1 || r == S.n) S.long_rows.push_back(r);
    return S;
}

static void check_chunks(const BatchChunks& C, const Stack& S, bool with_x, bool with_z, int chunk)
{
    const int nb = (int)S.nb();
    CHECK((int)C.wg_ptr.size() == nb + 1 && C.wg_ptr[0] == 0);
    CHECK(C.wg_mem.size() == C.wg_first.size());
    if ((int)C.wg_ptr.size() != nb + 1) return;
    CHECK(C.wg_ptr[(size_t)nb] == (int)C.wg_mem.size());
    for (int b = 0; b < nb; ++b) {
        const int64_t rows = (with_x ? S.x_off[b + 1] - S.x_off[b] : 0) + (with_z ? S.z_off[b + 1] - S.z_off[b] : 0);
        std::vector<int> covered((size_t)rows, 0);                       // brute force: every local row in exactly one workgroup
        CHECK(C.wg_ptr[b] <= C.wg_ptr[b + 1]);
        for (int w = C.wg_ptr[b]; w < C.wg_ptr[b + 1]; ++w) {
            CHECK(C.wg_mem[w] == b);
            CHECK(C.wg_first[w] >= 0 && C.wg_first[w] < rows && C.wg_first[w] % chunk == 0);
            for (int64_t r = C.wg_first[w]; r < C.wg_first[w] + chunk && r < rows; ++r) ++covered[(size_t)r];
            if (w > C.wg_ptr[b]) CHECK(C.wg_first[w] == C.wg_first[w - 1] + chunk);
        }
        for (int64_t r = 0; r < rows; ++r) CHECK(covered[(size_t)r] == 1);
    }
}

static void check_against_brute_force(const Stack& S)
{
    BatchPlan P;
    const std::string err = S.plan(P);
    if (!err.empty()) std::fprintf(stderr, "batch_plan_driver: refused: %s\n", err.c_str());
    CHECK(err.empty());
    if (!err.empty()) return;
    const int nb = (int)S.nb();
    CHECK(P.nb == nb && (int)P.xmem.size() == S.n && (int)P.zmem.size() == S.m);
    auto brute = [&](const std::vector<int64_t>& off, int i) { int b = 0; while (!(off[b] <= i && i < off[b + 1])) ++b; return b; };
    for (int i = 0; i < S.n; ++i) CHECK(P.xmem[i] == brute(S.x_off, i));
    for (int i = 0; i < S.m; ++i) CHECK(P.zmem[i] == brute(S.z_off, i));
    for (int b = 0; b <= nb; ++b) { CHECK(P.x_off[b] == S.x_off[b]); CHECK(P.z_off[b] == S.z_off[b]); }
    // cones
    CHECK(P.cone_mem.size() == S.cones.size() && (int)P.soc_ptr.size() == nb + 1 && (int)P.psd_ptr.size() == nb + 1);
    std::vector<double> degree((size_t)nb, 0.0);
    std::vector<int> nsoc((size_t)nb, 0), npsd((size_t)nb, 0);
    int soc_seen = 0, psd_seen = 0;
    for (size_t c = 0; c < S.cones.size(); ++c) {
        const BatchCone& ci = S.cones[c];
        if (ci.numel == 0) continue;
        const int b = brute(S.z_off, ci.off);
        CHECK(P.cone_mem[c] == b);
        degree[(size_t)b] += ci.kind == 1 ? ci.numel : ci.kind == 2 ? 1 : ci.kind == 3 ? ci.dim : 0;
        if (ci.kind == 2) { CHECK(P.soc_ptr[b] <= soc_seen && soc_seen < P.soc_ptr[b + 1]); ++soc_seen; ++nsoc[(size_t)b]; }
        if (ci.kind == 3) { CHECK(P.psd_ptr[b] <= psd_seen && psd_seen < P.psd_ptr[b + 1]); ++psd_seen; ++npsd[(size_t)b]; }
    }
    for (int b = 0; b < nb; ++b) {
        CHECK(P.degree[b] == degree[(size_t)b]);
        CHECK(P.soc_ptr[b + 1] - P.soc_ptr[b] == nsoc[(size_t)b]);
        CHECK(P.psd_ptr[b + 1] - P.psd_ptr[b] == npsd[(size_t)b]);
    }
    CHECK(P.soc_ptr[0] == 0 && P.psd_ptr[0] == 0 && P.soc_ptr[nb] == soc_seen && P.psd_ptr[nb] == psd_seen);
    // workgroups
    check_chunks(P.rows32, S, true, true, kBatchRowsResidual);
    check_chunks(P.rows256, S, true, true, kBatchRowsDots);
    check_chunks(P.z256, S, false, true, kBatchRowsCone);
    // long rows: a permutation, grouped by member, ascending inside a member
    const int nl = (int)S.long_rows.size();
    CHECK((int)P.long_order.size() == nl && (int)P.long_ptr.size() == nb + 1 && P.long_ptr[0] == 0 && P.long_ptr[nb] == nl);
    std::vector<int> seen((size_t)nl, 0);
    for (int b = 0; b < nb; ++b)
        for (int k = P.long_ptr[b]; k < P.long_ptr[b + 1]; ++k) {
            const int t = P.long_order[k];
            CHECK(t >= 0 && t < nl);
            if (t < 0 || t >= nl) continue;
            ++seen[(size_t)t];
            const int row = S.long_rows[t];
            CHECK((row < S.n ? brute(S.x_off, row) : brute(S.z_off, row - S.n)) == b);
            if (k > P.long_ptr[b]) CHECK(P.long_order[k - 1] < t);
        }
    for (int t = 0; t < nl; ++t) CHECK(seen[(size_t)t] == 1);
}

static void expect_refusal(const Stack& S, const char* must_name)
{
    BatchPlan P;
    const std::string err = S.plan(P);
    CHECK(!err.empty());
    if (err.find(must_name) == std::string::npos) {
        std::fprintf(stderr, "batch_plan_driver: refusal \"%s\" does not name \"%s\"\n", err.c_str(), must_name);
        ++g_fail;
    }
}

static void add_entry(Stack& S, int col, int row)      // one more stored entry (row, col) of K's upper triangle
{
    S.rowval.insert(S.rowval.begin() + S.colptr[(size_t)col], row);
    for (size_t j = (size_t)col + 1; j < S.colptr.size(); ++j) ++S.colptr[j];
}

static int read_stack(const char* path, Stack& S)
{
    std::ifstream f(path);
    int64_t nb = 0, ncones = 0;
    if (!(f >> S.n >> S.m >> nb)) return 1;
    S.x_off.assign((size_t)nb + 1, 0);
    S.z_off.assign((size_t)nb + 1, 0);
    for (auto& v : S.x_off) f >> v;
    for (auto& v : S.z_off) f >> v;
    f >> ncones;
    S.cones.resize((size_t)ncones);
    for (auto& c : S.cones) f >> c.kind >> c.off >> c.numel >> c.dim;
    S.colptr.assign((size_t)S.n + S.m + 1, 0);
    for (auto& v : S.colptr) f >> v;
    S.rowval.assign((size_t)S.colptr.back(), 0);
    for (auto& v : S.rowval) f >> v;
    return f ? 0 : 1;
}

int main(int argc, char** argv)
{
    if (argc > 1) {
        for (int a = 1; a < argc; ++a) {
            Stack S;
            if (read_stack(argv[a], S)) { std::fprintf(stderr, "batch_plan_driver: cannot read %s\n", argv[a]); return 2; }
            check_against_brute_force(S);
        }
        if (g_fail) return 1;
        std::printf("BATCH PLAN DRIVER OK (%d stacks)\n", argc - 1);
        return 0;
    }
    std::mt19937 rng(20240607u);
    // ---- the member sizes at which a chunking changes: around 8 lanes, a wave's half, 32 owner rows, a workgroup of 256;
    // a member of 5000 rows; a member without z rows; in several orders
    {
        const int edge[10] = {1, 7, 8, 9, 31, 32, 33, 255, 256, 257};
        std::vector<std::pair<int, int>> sizes;
        for (int e : edge) sizes.push_back({e, e});
        for (int e : edge) sizes.push_back({1, e});                      // (combined rows e + 1: just past every edge)
        for (int e : edge) sizes.push_back({e, 0});                      // no z rows
        sizes.push_back({2000, 3000});                                   // 5000 combined rows
        sizes.push_back({5000, 5000});
        check_against_brute_force(make_stack(sizes, rng));
        std::vector<std::pair<int, int>> rev(sizes.rbegin(), sizes.rend());
        check_against_brute_force(make_stack(rev, rng));
    }
    // ---- member counts
    for (int nb : {1, 2, 3, 64, 65, 256, 257}) {
        for (int rep = 0; rep < 3; ++rep) {
            std::vector<std::pair<int, int>> sizes;
            for (int b = 0; b < nb; ++b) sizes.push_back({1 + (int)(rng() % 40), rng() % 5 == 0 ? 0 : (int)(rng() % 70)});
            check_against_brute_force(make_stack(sizes, rng));
        }
    }
    {
        std::vector<std::pair<int, int>> sizes(257, {1, 1});               // the smallest members there are
        check_against_brute_force(make_stack(sizes, rng));
        std::vector<std::pair<int, int>> nz(3, {2, 0});                    // m = 0 altogether
        check_against_brute_force(make_stack(nz, rng));
    }
    // ---- refusals
    const std::vector<std::pair<int, int>> three{{5, 6}, {4, 9}, {7, 3}};
    {
        Stack S = make_stack(three, rng);                                // offsets not monotone
        S.x_off[1] = 9; S.x_off[2] = 5;
        expect_refusal(S, "x_off decreases at member 1");
        S = make_stack(three, rng);
        S.z_off[2] = 2;
        expect_refusal(S, "z_off decreases at member 1");
    }
    {
        Stack S = make_stack(three, rng);                                // wrong end
        S.x_off[3] -= 1;
        expect_refusal(S, "x_off ends at 15, not at n = 16");
        S = make_stack(three, rng);
        S.z_off[3] += 1;
        expect_refusal(S, "z_off of member 2 ends past m");
        S = make_stack(three, rng);
        S.x_off[0] = 1;
        expect_refusal(S, "x_off[0]");
    }
    {
        Stack S = make_stack(three, rng);                                // empty x range
        S.x_off[2] = S.x_off[1];
        expect_refusal(S, "member 1 has no x row");
    }
    {
        Stack S = make_stack(three, rng);                                // a cone across a boundary
        S.cones.clear();
        S.cones.push_back(BatchCone{1, 0, 4, 4});
        S.cones.push_back(BatchCone{2, 4, 3, 3});                        // rows 4 .. 6: member 0 ends at row 5
        S.cones.push_back(BatchCone{1, 7, 11, 11});
        expect_refusal(S, "cone 1 (rows 4 .. 6) crosses the boundary behind member 0");
    }
    {
        Stack S = make_stack(three, rng);                                // one coupling entry in P: (2, 6), members 0 and 1
        add_entry(S, 6, 2);
        expect_refusal(S, "entry (2, 6) of P couples member 0 with member 1");
    }
    {
        Stack S = make_stack(three, rng);                                // one coupling entry in A: row 7 (member 1), column 1 (member 0)
        add_entry(S, S.n + 7, 1);
        expect_refusal(S, "entry (7, 1) of A couples member 1 (its row) with member 0 (its column)");
    }
    {
        Stack S = make_stack(three, rng);                                // the last member coupled with the first, in P and in A
        add_entry(S, S.n - 1, 0);
        expect_refusal(S, "of P couples member 0 with member 2");
        S = make_stack(three, rng);
        add_entry(S, S.n + S.m - 1, 0);
        expect_refusal(S, "of A couples member 2 (its row) with member 0 (its column)");
    }
    {
        Stack S = make_stack(three, rng);                                // more members than rows, none at all
        BatchPlan P;
        CHECK(!plan_batch(S.n, S.m, 0, S.x_off.data(), S.z_off.data(), S.cones.data(), (int)S.cones.size(), S.colptr.data(),
                          S.rowval.data(), nullptr, 0, P).empty());
        CHECK(!plan_batch(S.n, S.m, 3, nullptr, S.z_off.data(), S.cones.data(), (int)S.cones.size(), S.colptr.data(),
                          S.rowval.data(), nullptr, 0, P).empty());
        CHECK(!plan_batch(2, S.m, 3, S.x_off.data(), S.z_off.data(), S.cones.data(), (int)S.cones.size(), S.colptr.data(),
                          S.rowval.data(), nullptr, 0, P).empty());
    }
    if (g_fail) return 1;
    std::printf("BATCH PLAN DRIVER OK\n");
    return 0;
}
