// plan_column_members (csrc/batch_plan.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: the column -> member
// table of hipkkt_kkt_system_set_member_status, colmem[k] = rowmem[perm[k]], against brute force -- the member of column k
// found by searching the members' own row lists for row perm[k] -- on random partitions through plan_batch and
// plan_batch_image and random permutations, and on the edges: nb = 1; members of one row; members whose expansion rows lie
// far from their other rows; nb close to N (every member one x row, some with a z row).  And every refusal: a permutation
// or a row table of the wrong length, an entry outside 0 .. N - 1, a row that appears twice, a row without a member, a
// member index >= nb, nb < 1.
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "batch_plan.hpp"

using namespace hipkkt;

static int g_fail = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "member_status_driver: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
    } while (0)

// a member: nx x rows, then its cones in order (numel, sparse second-order or not)
struct Member { int nx; std::vector<std::pair<int, bool>> cones; };

struct Image {
    int n = 0, m = 0, p = 0, N = 0;
    BatchImagePlan I;
    std::vector<std::vector<int>> rows;    // brute force: every member's rows of the image, listed by walking the member
};

static Image make_image(const std::vector<Member>& members)
{
    Image G;
    std::vector<int64_t> x_off{0}, z_off{0};
    std::vector<BatchCone> bc;
    std::vector<BatchImageCone> ic;
    std::vector<std::vector<int>> exp(members.size());
    for (size_t b = 0; b < members.size(); ++b) {
        int nz = 0;
        for (auto& c : members[b].cones) {
            bc.push_back(BatchCone{c.second ? 2 : 1, (int)z_off.back() + nz, c.first, c.first});
            ic.push_back(BatchImageCone{c.second ? G.p : 0, c.second ? 2 : 0});
            if (c.second) { exp[b].push_back(G.p); exp[b].push_back(G.p + 1); G.p += 2; }
            nz += c.first;
        }
        x_off.push_back(x_off.back() + members[b].nx);
        z_off.push_back(z_off.back() + nz);
    }
    G.n = (int)x_off.back();
    G.m = (int)z_off.back();
    G.N = G.n + G.m + G.p;
    std::vector<int64_t> colptr((size_t)G.n + G.m + 1);
    std::vector<int> rowval((size_t)G.n + G.m);
    for (int j = 0; j < G.n + G.m; ++j) { colptr[(size_t)j] = j; rowval[(size_t)j] = j; }
    colptr[(size_t)G.n + G.m] = G.n + G.m;
    BatchPlan B;
    std::string err = plan_batch(G.n, G.m, (int64_t)members.size(), x_off.data(), z_off.data(), bc.data(), (int)bc.size(),
                                 colptr.data(), rowval.data(), nullptr, 0, B);
    CHECK(err.empty());
    err = plan_batch_image(G.n, G.m, G.p, B, ic.data(), (int)ic.size(), nullptr, 0, 32, G.I);
    CHECK(err.empty());
    G.rows.resize(members.size());
    for (size_t b = 0; b < members.size(); ++b) {
        for (int64_t i = x_off[b]; i < x_off[b + 1]; ++i) G.rows[b].push_back((int)i);
        for (int64_t i = z_off[b]; i < z_off[b + 1]; ++i) G.rows[b].push_back(G.n + (int)i);
        for (int e : exp[b]) G.rows[b].push_back(G.n + G.m + e);
    }
    return G;
}

static void check_columns(const std::vector<Member>& members, std::mt19937& rng, bool identity = false)
{
    const Image G = make_image(members);
    const int nb = (int)members.size(), N = G.N;
    std::vector<int> perm((size_t)N);
    std::iota(perm.begin(), perm.end(), 0);
    if (!identity) std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<int> colmem{7, 7, 7};                                       // (whatever it held is replaced)
    const std::string err = plan_column_members(N, nb, perm.data(), perm.size(), G.I.rowmem.data(), G.I.rowmem.size(), colmem);
    if (!err.empty()) std::fprintf(stderr, "member_status_driver: refused: %s\n", err.c_str());
    CHECK(err.empty());
    CHECK((int)colmem.size() == N);
    if (!err.empty() || (int)colmem.size() != N) return;
    std::vector<int> count((size_t)nb, 0);
    for (int k = 0; k < N; ++k) {
        int owner = -1;
        for (int b = 0; b < nb && owner < 0; ++b)
            if (std::find(G.rows[(size_t)b].begin(), G.rows[(size_t)b].end(), perm[(size_t)k]) != G.rows[(size_t)b].end()) owner = b;
        CHECK(owner >= 0 && colmem[(size_t)k] == owner);
        if (owner >= 0) ++count[(size_t)owner];
    }
    for (int b = 0; b < nb; ++b) CHECK(count[(size_t)b] == (int)G.rows[(size_t)b].size());     // every member keeps all its columns
}

static std::vector<Member> random_members(std::mt19937& rng, int nb)
{
    std::vector<Member> M;
    for (int b = 0; b < nb; ++b) {
        Member mb;
        mb.nx = 1 + (int)(rng() % 12);
        const int nc = (int)(rng() % 4);
        for (int c = 0; c < nc; ++c) {
            const bool soc = rng() % 3 == 0;
            mb.cones.push_back({soc ? 5 + (int)(rng() % 4) : 1 + (int)(rng() % 9), soc});
        }
        M.push_back(mb);
    }
    return M;
}

static bool refused(const std::string& err, const char* text) { return err.find(text) != std::string::npos; }

int main()
{
    std::mt19937 rng(20241103);
    for (int trial = 0; trial < 200; ++trial) check_columns(random_members(rng, 1 + (int)(rng() % 12)), rng);
    // ---- the edges
    check_columns({Member{7, {{9, false}, {5, true}}}}, rng);                                         // nb = 1
    check_columns({Member{7, {{9, false}, {5, true}}}}, rng, true);                                   // ... the identity
    check_columns({Member{1, {}}}, rng);                                                              // N = 1
    check_columns({Member{1, {}}, Member{1, {}}, Member{3, {{4, false}}}, Member{1, {}}}, rng);       // members of one row
    check_columns({Member{3, {{40, false}}}, Member{2, {{5, true}}}, Member{4, {{30, false}, {6, true}}}, Member{2, {{7, true}}}}, rng);   // far expansion rows
    {
        std::vector<Member> M;                                                                        // nb close to N
        for (int b = 0; b < 500; ++b) M.push_back(b % 3 == 0 ? Member{1, {{1, false}}} : Member{1, {}});
        check_columns(M, rng);
        std::vector<Member> M1;                                                                       // nb = N
        for (int b = 0; b < 64; ++b) M1.push_back(Member{1, {}});
        check_columns(M1, rng);
    }
    // ---- refusals
    {
        const Image G = make_image({Member{2, {{5, true}}}, Member{2, {{3, false}}}});
        const int N = G.N, nb = 2;
        std::vector<int> perm((size_t)N), out;
        std::iota(perm.begin(), perm.end(), 0);
        const std::vector<int>& rm = G.I.rowmem;
        CHECK(plan_column_members(N, nb, perm.data(), perm.size(), rm.data(), rm.size(), out).empty());
        CHECK(refused(plan_column_members(N, nb, perm.data(), perm.size() - 1, rm.data(), rm.size(), out), "the permutation has"));
        CHECK(refused(plan_column_members(N, nb, perm.data(), perm.size(), rm.data(), rm.size() - 1, out), "the row table has"));
        CHECK(refused(plan_column_members(N, 0, perm.data(), perm.size(), rm.data(), rm.size(), out), "at least one member"));
        CHECK(refused(plan_column_members(-1, nb, perm.data(), perm.size(), rm.data(), rm.size(), out), "N >= 0"));
        std::vector<int> bad = perm;
        bad[3] = N;
        CHECK(refused(plan_column_members(N, nb, bad.data(), bad.size(), rm.data(), rm.size(), out), "outside the image"));
        bad[3] = -1;
        CHECK(refused(plan_column_members(N, nb, bad.data(), bad.size(), rm.data(), rm.size(), out), "outside the image"));
        bad[3] = 4;
        CHECK(refused(plan_column_members(N, nb, bad.data(), bad.size(), rm.data(), rm.size(), out), "appears twice"));
        std::vector<int> brm = rm;
        brm[5] = nb;
        CHECK(refused(plan_column_members(N, nb, perm.data(), perm.size(), brm.data(), brm.size(), out), "belongs to no member"));
        brm[5] = -1;
        CHECK(refused(plan_column_members(N, nb, perm.data(), perm.size(), brm.data(), brm.size(), out), "belongs to no member"));
        CHECK(refused(plan_column_members(N, 1, perm.data(), perm.size(), rm.data(), rm.size(), out), "belongs to no member"));   // nb too small
    }
    if (g_fail) { std::fprintf(stderr, "member_status_driver: %d checks failed\n", g_fail); return 1; }
    std::printf("MEMBER STATUS DRIVER OK\n");
    return 0;
}
