// plan_batch_image (csrc/batch_plan.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: the tables of
// hipkkt_kkt_system_set_member_refinement -- row of K's image -> member for all n + m + p rows, the rows listed by member,
// the assignment of workgroups to (member, chunk of that member's image rows) with its slot layout, the long rows by
// member -- against brute force, on random partitions and on the edges that the kernels meet: one member; a member of one x
// row and no z row; a member whose rows fill a chunk exactly, and one row more; a member whose only z rows belong to a
// sparse second-order cone (its expansion rows lie far from its other rows); long rows in two different members; as many
// members as x rows.  And the refusals: an expansion row without a cone, one with two, a long row outside the image.
#include <algorithm>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "batch_plan.hpp"

using namespace hipkkt;

static int g_fail = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "batch_image_driver: line %d: %s\n", __LINE__, #cond); ++g_fail; } \
    } while (0)

// a member: nx x rows, then its cones in order (numel, sparse second-order or not)
struct Member { int nx; std::vector<std::pair<int, bool>> cones; };

struct Image {
    int n = 0, m = 0, p = 0;
    BatchPlan B;
    std::vector<BatchImageCone> cones;
    std::vector<int> cone_member;          // brute force: the member that listed the cone
};

// the partition through plan_batch itself (a diagonal K: no coupling), the expansion columns in cone order
static Image make_image(const std::vector<Member>& members)
{
    Image I;
    std::vector<int64_t> x_off{0}, z_off{0};
    std::vector<BatchCone> bc;
    for (size_t b = 0; b < members.size(); ++b) {
        int nz = 0;
        for (auto& c : members[b].cones) {
            bc.push_back(BatchCone{c.second ? 2 : 1, (int)z_off.back() + nz, c.first, c.first});
            I.cones.push_back(BatchImageCone{c.second ? I.p : 0, c.second ? 2 : 0});
            I.cone_member.push_back((int)b);
            if (c.second) I.p += 2;
            nz += c.first;
        }
        x_off.push_back(x_off.back() + members[b].nx);
        z_off.push_back(z_off.back() + nz);
    }
    I.n = (int)x_off.back();
    I.m = (int)z_off.back();
    std::vector<int64_t> colptr((size_t)I.n + I.m + 1);
    std::vector<int> rowval((size_t)I.n + I.m);
    for (int j = 0; j < I.n + I.m; ++j) { colptr[(size_t)j] = j; rowval[(size_t)j] = j; }
    colptr[(size_t)I.n + I.m] = I.n + I.m;
    const std::string err = plan_batch(I.n, I.m, (int64_t)members.size(), x_off.data(), z_off.data(), bc.data(), (int)bc.size(),
                                       colptr.data(), rowval.data(), nullptr, 0, I.B);
    if (!err.empty()) std::fprintf(stderr, "batch_image_driver: plan_batch refused: %s\n", err.c_str());
    CHECK(err.empty());
    return I;
}

static void check_image(const std::vector<Member>& members, const std::vector<int>& long_rows, int chunk)
{
    const Image I = make_image(members);
    const int nb = (int)members.size(), N = I.n + I.m + I.p;
    BatchImagePlan P;
    const std::string err = plan_batch_image(I.n, I.m, I.p, I.B, I.cones.data(), (int)I.cones.size(), long_rows.data(),
                                             (int)long_rows.size(), chunk, P);
    if (!err.empty()) std::fprintf(stderr, "batch_image_driver: refused: %s\n", err.c_str());
    CHECK(err.empty());
    if (!err.empty()) return;
    // ---- brute force: the member of every row, by walking the members' own lists
    std::vector<int> want((size_t)N, -1);
    {
        int x = 0, z = 0, c = 0;
        for (int b = 0; b < nb; ++b) {
            for (int i = 0; i < members[(size_t)b].nx; ++i) want[(size_t)x++] = b;
            for (auto& cn : members[(size_t)b].cones) {
                for (int i = 0; i < cn.first; ++i) want[(size_t)I.n + z++] = b;
                if (cn.second) { want[(size_t)I.n + I.m + I.cones[(size_t)c].pcol] = b; want[(size_t)I.n + I.m + I.cones[(size_t)c].pcol + 1] = b; }
                ++c;
            }
        }
    }
    CHECK(P.nb == nb && P.N == N && P.chunk == chunk);
    CHECK((int)P.rowmem.size() == N && (int)P.img_rows.size() == N && (int)P.img_ptr.size() == nb + 1);
    if ((int)P.rowmem.size() != N || (int)P.img_rows.size() != N || (int)P.img_ptr.size() != nb + 1) return;
    for (int i = 0; i < N; ++i) CHECK(P.rowmem[(size_t)i] == want[(size_t)i]);
    // ---- the rows by member: member b's range holds exactly its rows, ascending
    CHECK(P.img_ptr[0] == 0 && P.img_ptr[(size_t)nb] == N);
    for (int b = 0; b < nb; ++b) {
        std::vector<int> rows;
        for (int i = 0; i < N; ++i) if (want[(size_t)i] == b) rows.push_back(i);
        CHECK(P.img_ptr[(size_t)b + 1] - P.img_ptr[(size_t)b] == (int)rows.size());
        if (P.img_ptr[(size_t)b + 1] - P.img_ptr[(size_t)b] != (int)rows.size()) return;
        for (size_t k = 0; k < rows.size(); ++k) CHECK(P.img_rows[(size_t)P.img_ptr[(size_t)b] + k] == rows[k]);
    }
    // ---- workgroups: every position of img_rows in exactly one workgroup, of its member; slots side by side
    const BatchChunks& W = P.wg;
    CHECK((int)W.wg_ptr.size() == nb + 1 && W.wg_mem.size() == W.wg_first.size());
    if ((int)W.wg_ptr.size() != nb + 1 || W.wg_mem.size() != W.wg_first.size()) return;
    CHECK(W.wg_ptr[0] == 0 && W.wg_ptr[(size_t)nb] == (int)W.wg_mem.size());
    std::vector<int> covered((size_t)N, 0), slot_owner(W.wg_mem.size() + (size_t)nb, -1);
    for (int b = 0; b < nb; ++b) {
        const int rows = P.img_ptr[(size_t)b + 1] - P.img_ptr[(size_t)b];
        CHECK(W.wg_ptr[(size_t)b + 1] - W.wg_ptr[(size_t)b] == (rows + chunk - 1) / chunk);
        for (int w = W.wg_ptr[(size_t)b]; w < W.wg_ptr[(size_t)b + 1]; ++w) {
            CHECK(W.wg_mem[(size_t)w] == b);
            CHECK(W.wg_first[(size_t)w] == P.img_ptr[(size_t)b] + (w - W.wg_ptr[(size_t)b]) * chunk);
            for (int pos = W.wg_first[(size_t)w]; pos < W.wg_first[(size_t)w] + chunk && pos < P.img_ptr[(size_t)b + 1]; ++pos)
                if (pos >= 0 && pos < N) ++covered[(size_t)pos];
            const size_t slot = (size_t)w + (size_t)W.wg_mem[(size_t)w];               // what the residual kernel writes
            CHECK(slot < slot_owner.size() && slot_owner[slot] == -1);
            if (slot < slot_owner.size()) slot_owner[slot] = b;
        }
        const size_t lslot = (size_t)W.wg_ptr[(size_t)b + 1] + (size_t)b;              // ... and the long rows' finish
        CHECK(lslot < slot_owner.size() && slot_owner[lslot] == -1);
        if (lslot < slot_owner.size()) slot_owner[lslot] = b;
        // what the round kernel folds: wg_ptr[b] + b .. wg_ptr[b + 1] + b, all member b's, nothing else
        for (size_t s = (size_t)W.wg_ptr[(size_t)b] + (size_t)b; s <= lslot && s < slot_owner.size(); ++s) CHECK(slot_owner[s] == b);
    }
    for (int i = 0; i < N; ++i) CHECK(covered[(size_t)i] == 1);
    for (size_t s = 0; s < slot_owner.size(); ++s) CHECK(slot_owner[s] >= 0);
    // ---- long rows by member
    CHECK((int)P.long_ptr.size() == nb + 1 && P.long_order.size() == long_rows.size());
    if ((int)P.long_ptr.size() != nb + 1 || P.long_order.size() != long_rows.size()) return;
    CHECK(P.long_ptr[0] == 0 && P.long_ptr[(size_t)nb] == (int)long_rows.size());
    for (int b = 0; b < nb; ++b) {
        std::vector<int> mine;
        for (size_t t = 0; t < long_rows.size(); ++t) if (want[(size_t)long_rows[t]] == b) mine.push_back((int)t);
        CHECK(P.long_ptr[(size_t)b + 1] - P.long_ptr[(size_t)b] == (int)mine.size());
        if (P.long_ptr[(size_t)b + 1] - P.long_ptr[(size_t)b] != (int)mine.size()) return;
        for (size_t k = 0; k < mine.size(); ++k) CHECK(P.long_order[(size_t)P.long_ptr[(size_t)b] + k] == mine[k]);
    }
}

static std::vector<Member> random_members(std::mt19937& rng, int nb)
{
    std::vector<Member> M;
    for (int b = 0; b < nb; ++b) {
        Member mb;
        mb.nx = 1 + (int)(rng() % 40);
        const int nc = (int)(rng() % 4);
        for (int c = 0; c < nc; ++c) {
            const bool soc = rng() % 3 == 0;
            mb.cones.push_back({soc ? 5 + (int)(rng() % 4) : 1 + (int)(rng() % 50), soc});
        }
        M.push_back(mb);
    }
    return M;
}

int main()
{
    std::mt19937 rng(20240607);
    for (int trial = 0; trial < 200; ++trial) {
        const int nb = 1 + (int)(rng() % 12);
        const std::vector<Member> M = random_members(rng, nb);
        const Image I = make_image(M);
        std::vector<int> lr;
        for (int r = 0; r < I.n + I.m + I.p; ++r) if (rng() % 23 == 0) lr.push_back(r);
        const int chunks[5] = {1, 4, 32, 64, 1000};
        check_image(M, lr, chunks[trial % 5]);
    }
    // ---- the edges
    check_image({Member{7, {{9, false}, {5, true}}}}, {0, 20}, 32);                                   // nb = 1
    check_image({Member{3, {{4, false}}}, Member{1, {}}, Member{2, {{3, false}}}}, {}, 32);           // one x row, no z row
    check_image({Member{1, {}}}, {}, 4);
    check_image({Member{20, {{12, false}}}, Member{20, {{13, false}}}, Member{2, {}}}, {}, 32);       // a chunk exactly, and one row more
    check_image({Member{2, {{2, false}}}, Member{2, {{3, false}}}}, {}, 4);                           // (the same with the 64-lane kernel's 4 rows)
    check_image({Member{3, {{40, false}}}, Member{2, {{5, true}}}, Member{4, {{30, false}, {6, true}}}}, {}, 32);   // only z rows: one sparse cone
    {
        // long rows in two different members (one of them an expansion row), none in the middle member
        const std::vector<Member> M{Member{5, {{6, false}}}, Member{4, {{3, false}}}, Member{3, {{7, true}}}};
        const Image I = make_image(M);
        check_image(M, {1, 4, I.n + 2, I.n + I.m + 1}, 32);
    }
    {
        std::vector<Member> M;                                                                        // nb = the row count of x
        for (int b = 0; b < 700; ++b) M.push_back(Member{1, {{2, false}}});
        check_image(M, {5, 1400}, 32);
        std::vector<Member> M1;
        for (int b = 0; b < 9; ++b) M1.push_back(Member{1, {}});
        check_image(M1, {}, 32);
    }
    // ---- refusals
    {
        const std::vector<Member> M{Member{2, {{5, true}}}, Member{2, {{6, true}}}};
        Image I = make_image(M);
        BatchImagePlan P;
        std::vector<BatchImageCone> c = I.cones;
        c[1].pwidth = 0;                                                                              // rows 2, 3 of the expansion: no cone
        CHECK(plan_batch_image(I.n, I.m, I.p, I.B, c.data(), (int)c.size(), nullptr, 0, 32, P).find("belongs to no cone") != std::string::npos);
        c = I.cones;
        c[1].pcol = 1;                                                                                // overlaps cone 0's
        CHECK(plan_batch_image(I.n, I.m, I.p, I.B, c.data(), (int)c.size(), nullptr, 0, 32, P).find("two cones") != std::string::npos);
        c = I.cones;
        c[1].pcol = 3;
        CHECK(plan_batch_image(I.n, I.m, I.p, I.B, c.data(), (int)c.size(), nullptr, 0, 32, P).find("outside the image") != std::string::npos);
        const int bad_long[1] = {I.n + I.m + I.p};
        CHECK(plan_batch_image(I.n, I.m, I.p, I.B, I.cones.data(), (int)I.cones.size(), bad_long, 1, 32, P).find("long row 0") != std::string::npos);
        CHECK(plan_batch_image(I.n, I.m, I.p, I.B, I.cones.data(), (int)I.cones.size(), nullptr, 0, 0, P).find("chunk") != std::string::npos);
        CHECK(plan_batch_image(I.n + 1, I.m, I.p, I.B, I.cones.data(), (int)I.cones.size(), nullptr, 0, 32, P).find("does not belong") != std::string::npos);
    }
    if (g_fail) { std::fprintf(stderr, "batch_image_driver: %d checks failed\n", g_fail); return 1; }
    std::printf("BATCH IMAGE DRIVER OK\n");
    return 0;
}
