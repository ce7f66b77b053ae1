// The numeric engine's device tables (engine_tables.hpp), host-only.
#include "engine_tables.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <utility>

#include "knobs.hpp"

namespace hipkkt {

namespace {

void mark_solve_pulled(const Symbolic& S, const Schedule& sch, EngineTables& T)
{
    T.solve_pulled.assign((size_t)S.nsuper, 0);
    if (!knobs().pull_leaves) return;
    std::vector<char> in_small((size_t)S.nsuper, 0);       // (one-wave launches only: the block kernels do not know the flag)
    for (const Launch& L : sch.launches)
        if (L.small) for (int t = L.begin; t < L.begin + L.count; ++t) in_small[(size_t)sch.sched[(size_t)t]] = 1;
    for (int s = 0; s < S.nsuper; ++s) {
        const int nb = (int)(S.rowptr[s + 1] - S.rowptr[s]);
        T.solve_pulled[(size_t)s] = in_small[(size_t)s] && S.child_ptr[s + 1] == S.child_ptr[s] && S.sn_start[s + 1] - S.sn_start[s] == 1 &&
                                    S.sn_parent[s] >= 0 && nb >= 1 && nb <= 47;
    }
}

void build_ncolpar(const Symbolic& S, EngineTables& T)
{
    T.ncolpar.assign((size_t)S.nsuper, 0);
    for (int s = 0; s < S.nsuper; ++s) {
        int p = S.sn_parent[s];
        if (p < 0) continue;
        int pnc = S.sn_start[p + 1] - S.sn_start[p], k = 0;
        for (int64_t q = S.rowptr[s]; q < S.rowptr[s + 1] && S.rel[q] < pnc; ++q) ++k;
        T.ncolpar[s] = k;
    }
}

void build_k_lists(const Symbolic& S, const Schedule& sch, EngineTables& T)
{
    std::vector<int>& ks_all = T.ksrc;
    std::vector<int>& kd = T.kdst;
    ks_all = S.ksrc;
    kd = S.kdst;
    T.slice_kptr.assign(sch.slice_list.size(), 0);
    T.slice_nk.assign(sch.slice_list.size(), 0);
    // the panel kernel keeps a block-class front as a trapezoid in LDS (factor_kernels.hip: pcol): its K
    // entries get their packed position; one-wave fronts keep lrow + lcol*f
    for (const Launch& L : sch.launches) {
        if (L.small) continue;
        for (int q = L.begin; q < L.begin + L.count - L.nsliced; ++q) {      // (sliced fronts keep lrow + lcol*f)
            const int s = sch.sched[q];
            const int f = front_size(S, s);
            for (int64_t e = S.kptr[s]; e < S.kptr[s + 1]; ++e) {
                const int lcol = kd[e] / f, lrow = kd[e] - lcol * f;
                kd[e] = lrow + (int)(((int64_t)lcol * (2 * f - 1 - lcol)) >> 1);
            }
        }
    }
    for (size_t q = 0; q < sch.slice_list.size(); ++q) {
        const int s = sch.slice_list[q][0], sl = sch.slice_list[q][1], nsl = sch.slice_list[q][2];
        const int ff = front_size(S, s), nc = S.sn_start[s + 1] - S.sn_start[s], nb = ff - nc;
        const int rsmax = (nb + nsl - 1) / nsl, r_lo = nc + sl * rsmax;
        const int rs = std::max(0, std::min(rsmax, ff - r_lo)), f = nc + rs;
        T.slice_kptr[q] = (int64_t)ks_all.size();
        for (int64_t e = S.kptr[s]; e < S.kptr[s + 1]; ++e) {
            const int lcol = S.kdst[e] / ff;
            int r = S.kdst[e] - lcol * ff;
            if (r >= nc) { if (r < r_lo || r >= r_lo + rs) continue; r = nc + (r - r_lo); }
            ks_all.push_back(S.ksrc[e]);
            kd.push_back(r + (int)(((int64_t)lcol * (2 * f - 1 - lcol)) >> 1));
        }
        T.slice_nk[q] = (int)((int64_t)ks_all.size() - T.slice_kptr[q]);
    }
    if (ks_all.size() >= ((size_t)1 << 31)) throw std::runtime_error("K scatter lists exceed int32 indexing");
}

void build_overlap_tables(const Symbolic& S, const Schedule& sch, EngineTables& T)
{
    T.ov_ntiles.assign((size_t)S.nsuper, 0);
    for (size_t q = sch.ov_first; q < sch.launches.size(); ++q) {
        const Launch& L = sch.launches[q];
        for (int t = L.begin; t < L.begin + L.count; ++t) {
            const int sn = sch.sched[(size_t)t];
            const int nb = front_size(S, sn) - (S.sn_start[sn + 1] - S.sn_start[sn]);
            const int k = (nb + 63) / 64;
            T.ov_ntiles[(size_t)sn] = k * (k + 1) / 2;
        }
    }
    T.ov_sbase.assign((size_t)std::max(S.nsuper, 1), -1);
    for (size_t q = sch.slice_list.size(); q-- > 0;) T.ov_sbase[(size_t)sch.slice_list[q][0]] = (int)q;      // (slices of a front are consecutive)
}

void build_descs(const Symbolic& S, const Schedule& sch, const FactorLists& fl, EngineTables& T)
{
    std::vector<int64_t>& toff = T.toff;
    toff.assign((size_t)S.nsuper + 1, 0);
    std::vector<char> in_list(S.nsuper, 0);
    for (int s : sch.tinv_list) in_list[s] = 1;
    // (level by level like the panel and update stores: symbolic.cpp, step 10)
    int64_t wo = 0;
    for (int t = 0; t < S.nsuper; ++t) {
        const int s = S.level_sn[t];
        int64_t nc = S.sn_start[s + 1] - S.sn_start[s];
        int64_t fs = nc + (S.rowptr[s + 1] - S.rowptr[s]);
        toff[s] = wo;
        wo += in_list[s] ? 2 * fs * nc : 0;
    }
    toff[S.nsuper] = wo;
    T.desc.resize(sch.sched.size());
    for (size_t q = 0; q < sch.sched.size(); ++q) {
        const int s = sch.sched[q];
        FrontDesc d;
        d.front_off = S.front_off[s]; d.upd_off = S.upd_off[s]; d.w_off = toff[s]; d.rp = S.rowptr[s];
        d.kptr = S.kptr[s]; d.s = s; d.c0 = S.sn_start[s]; d.nc = S.sn_start[s + 1] - S.sn_start[s];
        d.nb = (int)(S.rowptr[s + 1] - S.rowptr[s]); d.nk = (int)(S.kptr[s + 1] - S.kptr[s]);
        d.pad = (T.solve_pulled[(size_t)s] ? 1 : 0) | (fl.pulled[(size_t)s] ? 2 : 0);     // (bit 0 = a pulled leaf of the many-column sweeps; bit 1 = of the factorisation)
        T.desc[q] = d;
    }
    T.sdesc.assign(std::max<size_t>(sch.slice_list.size(), 1), FrontDesc{});
    for (size_t q = 0; q < sch.slice_list.size(); ++q) {
        FrontDesc d = T.desc[(size_t)sch.spos[(size_t)sch.slice_list[q][0]]];
        d.pad = (sch.slice_list[q][1] << 16) | sch.slice_list[q][2];
        d.kptr = T.slice_kptr[q]; d.nk = T.slice_nk[q];             // (its own K list, positions in the slice's image)
        T.sdesc[q] = d;
    }
}

void build_cuts(const Symbolic& S, EngineTables& T)
{
    T.cut_ptr.assign((size_t)S.nsuper + 1, 0);
    std::vector<int>& cuts = T.cuts;
    for (int c = 0; c < S.nsuper; ++c) {
        T.cut_ptr[c] = (int64_t)cuts.size();
        int p = S.sn_parent[c];
        if (p < 0) continue;
        int pnc = S.sn_start[p + 1] - S.sn_start[p];
        int pnb = (int)(S.rowptr[p + 1] - S.rowptr[p]);
        int nt = (pnb + 63) / 64;
        const int* rb = S.rel.data() + S.rowptr[c];
        int nbc = (int)(S.rowptr[c + 1] - S.rowptr[c]);
        for (int t = 0; t <= nt; ++t)
            cuts.push_back((int)(std::lower_bound(rb, rb + nbc, pnc + 64 * t) - rb));
    }
    T.cut_ptr[S.nsuper] = (int64_t)cuts.size();
}

int64_t lbase(const Symbolic& S, int s) { return (int64_t)S.sn_start[s] + S.rowptr[s]; }

void build_gather_lists(const Symbolic& S, EngineTables& T)
{
    const int64_t nloc = (int64_t)S.N + (int64_t)S.rows.size();
    std::vector<int64_t>& ptr = T.item_ptr;
    ptr.assign((size_t)nloc + 1, 0);
    for (int c = 0; c < S.nsuper; ++c) {
        int p = S.sn_parent[c];
        if (p < 0) continue;
        for (int64_t q = S.rowptr[c]; q < S.rowptr[c + 1]; ++q) ptr[lbase(S, p) + S.rel[q] + 1]++;
    }
    for (int64_t i = 0; i < nloc; ++i) ptr[i + 1] += ptr[i];
    // one entry per child row, keyed by the receiving local row
    T.gsrc.assign((size_t)ptr[nloc], 0);
    {
        std::vector<int64_t> nxt(ptr.begin(), ptr.end() - 1);
        for (int p = 0; p < S.nsuper; ++p)
            for (int e = S.child_ptr[p]; e < S.child_ptr[p + 1]; ++e) {     // children in fixed order
                int c = S.child_idx[e];
                for (int64_t q = S.rowptr[c]; q < S.rowptr[c + 1]; ++q) T.gsrc[nxt[lbase(S, p) + S.rel[q]]++] = (int)q;
            }
    }
    if (S.rows.size() >= ((size_t)1 << 31)) throw std::runtime_error("row structure exceeds int32 indexing");
    // where each contribution entry sits in its receiver's gather list (solve_multi's layout)
    T.udst.assign(std::max<size_t>(S.rows.size(), 1), 0);
    for (size_t g = 0; g < T.gsrc.size(); ++g) T.udst[(size_t)T.gsrc[g]] = (int)g;
}

// XCD-aware launch order of a wide level's tiles (HIPKKT_TILE_XCD=n: launches with at least n fronts;
// 0 = off): workgroup i of a launch runs on XCD i mod 8, each XCD has its own L2, and every tile of a front
// reads that front's L21 strips -- a front's tiles are dealt to ONE residue class (eight fronts interleaved,
// fronts in work order so that a group's fronts have similar tile counts), so its strips come from HBM
// once instead of once per XCD that happens to hold one of its tiles.
// Measured on cfg2 (rocprofv3 --pmc FETCH_SIZE, r03): k_schur's reads 838 -> 525 MB per factorisation with the
// wide levels (>= 150 fronts) permuted, factorisation 1.754 / 1.760 -> 1.743 / 1.751 ms; permuting the narrow
// levels as well costs time (>= 32: 1.766 / 1.770 -- a handful of fronts' tiles then crowd one XCD).
void build_tile_order(const Symbolic& S, const Schedule& sch, FactorLists& fl, EngineTables& T)
{
    std::vector<int64_t>& tcut = fl.tcut;
    std::vector<int>& ptcut = fl.ptcut;
    T.tiles = sch.tiles;
    const int tile_xcd = knobs().tile_xcd;
    if (tile_xcd <= 0) return;
    std::vector<int64_t> nc2(tcut);
    std::vector<int> pc2(ptcut);
    for (const Launch& L : sch.launches) {
        if (L.small || L.count < tile_xcd || L.ntiles <= 0) continue;
        ++T.dealt_launches;
        T.dealt_tiles += L.ntiles;
        T.dealt_list += " " + std::to_string(&L - sch.launches.data());
        // the launch's fronts and their (contiguous) logical tile ranges
        std::vector<std::pair<int64_t, int64_t>> rng;       // [first, last) per front, launch order
        for (int t = L.begin; t < L.begin + L.count; ++t) {
            const int sn = sch.sched[(size_t)t];
            if (sch.tile_base[sn] < 0) continue;
            const int nb = front_size(S, sn) - (S.sn_start[sn + 1] - S.sn_start[sn]);
            const int k = (nb + 63) / 64;
            if (k > 0) rng.push_back({sch.tile_base[sn], sch.tile_base[sn] + (int64_t)k * (k + 1) / 2});
        }
        int64_t pos = L.tile_begin;
        for (size_t g0 = 0; g0 < rng.size(); g0 += 8) {
            const size_t g1 = std::min(rng.size(), g0 + 8);
            int64_t longest = 0;
            for (size_t x = g0; x < g1; ++x) longest = std::max(longest, rng[x].second - rng[x].first);
            for (int64_t j = 0; j < longest; ++j)
                for (size_t x = g0; x < g1; ++x)
                    if (rng[x].first + j < rng[x].second) {
                        const int64_t from = rng[x].first + j;
                        T.tiles[(size_t)pos] = sch.tiles[(size_t)from];
                        for (int w = 0; w < 5; ++w) nc2[(size_t)pos * 5 + w] = tcut[(size_t)from * 5 + w];
                        for (int w = 0; w < 5; ++w) pc2[(size_t)pos * 5 + w] = ptcut[(size_t)from * 5 + w];
                        ++pos;
                    }
        }
        if (pos != (int64_t)L.tile_begin + L.ntiles) throw std::runtime_error("tile permutation lost a tile");
    }
    tcut.swap(nc2);
    ptcut.swap(pc2);
}

// the split gather lists of the many-column sweeps (EngineTables: PULLED LEAVES)
void build_pull_lists(const Symbolic& S, EngineTables& T)
{
    const int64_t nloc = (int64_t)S.N + (int64_t)S.rows.size();
    const std::vector<int64_t>& ptr = T.item_ptr;
    const std::vector<int>& gsrc = T.gsrc;
    const std::vector<char>& pulled = T.solve_pulled;
    std::vector<int> row_sn(std::max<size_t>(S.rows.size(), 1), -1);
    for (int c = 0; c < S.nsuper; ++c)
        for (int64_t q = S.rowptr[c]; q < S.rowptr[c + 1]; ++q) row_sn[(size_t)q] = c;
    std::vector<int64_t>&mptr = T.glm_ptr, &prp = T.pr_ptr, &hl = T.hp_lidx;
    std::vector<int>&udm = T.udst_m, &hcol = T.hp_col, &prs = T.pr_slot;
    mptr.assign((size_t)nloc + 1, 0);
    prp.assign(1, 0);
    udm.assign(std::max<size_t>(S.rows.size(), 1), -1);
    int64_t slot = 0;
    for (int64_t lc = 0; lc < nloc; ++lc) {
        mptr[(size_t)lc] = slot;
        bool any = false;
        for (int64_t g = ptr[(size_t)lc]; g < ptr[(size_t)lc + 1] && !any; ++g) any = pulled[(size_t)row_sn[(size_t)gsrc[(size_t)g]]] != 0;
        if (any) prs.push_back((int)slot++);                  // the sum of this row's pulled terms: first of its run
        for (int64_t g = ptr[(size_t)lc]; g < ptr[(size_t)lc + 1]; ++g) {
            const int q = gsrc[(size_t)g], c = row_sn[(size_t)q];
            if (pulled[(size_t)c]) {
                hcol.push_back(S.sn_start[c]);
                hl.push_back(S.front_off[c] + 1 + ((int64_t)q - S.rowptr[c]));     // L(r, 0): column-major, ld f, nc = 1
            } else {
                udm[(size_t)q] = (int)slot++;
            }
        }
        if (any) prp.push_back((int64_t)hcol.size());
    }
    mptr[(size_t)nloc] = slot;
    T.n_pull_rows = (int)prs.size();
    T.n_pull_terms = (int64_t)hcol.size();      // (before the padding entry of an empty list)
    if (hcol.empty()) { hcol.push_back(0); hl.push_back(0); }
    if (prs.empty()) prs.push_back(0);
    T.hp_row.resize(hcol.size());
    for (size_t k = 0; k < hcol.size(); ++k) T.hp_row[k] = S.perm[(size_t)hcol[k]];
}

void build_records(const Symbolic& S, const Schedule& sch, EngineTables& T)
{
    const int64_t total = sch.rec_bytes;
    if (total <= 0) return;
    const std::vector<int64_t>& glptr = T.item_ptr;
    const std::vector<int>& gsrc = T.gsrc;
    T.recs.assign((size_t)(total / 8) + 8, 0);
    char* base = reinterpret_cast<char*>(T.recs.data());
    for (size_t q = 0; q < sch.launches.size(); ++q) {
        const Launch& L = sch.launches[q];
        const bool leaf = rec_no_slots(sch.launches, q);
        RecClass classes[2];
        const int nclasses = rec_classes(L, classes);
        for (int ci = 0; ci < nclasses; ++ci) {
            const RecClass& c = classes[ci];
            const int fmax = L.rec.fmax[c.cls];
            for (int k = 0; k < c.count; ++k) {
                const int sn = sch.sched[(size_t)(c.first + k)];
                char* rec = base + L.rec.off[c.cls] + (int64_t)k * L.rec.stride[c.cls];
                const int nc = S.sn_start[sn + 1] - S.sn_start[sn], nb = (int)(S.rowptr[sn + 1] - S.rowptr[sn]), f = nc + nb;
                if (f > fmax) throw std::runtime_error("packed record: front larger than its class");
                SolveHdr h{};
                h.mat_off = c.cls == 0 ? T.toff[(size_t)sn] : S.front_off[sn];
                h.rp = S.rowptr[sn];
                h.s = sn; h.c0 = S.sn_start[sn]; h.nc = nc; h.nb = nb;
                h.par = S.sn_parent[sn];
                h.nchild = sch.nch.empty() ? 0 : sch.nch[(size_t)sn];
                std::memcpy(rec, &h, sizeof(h));
                int* idx = reinterpret_cast<int*>(rec + sizeof(SolveHdr));
                for (int i = 0; i < nc; ++i) idx[i] = S.perm[(size_t)(h.c0 + i)];
                for (int i = nc; i < f; ++i) idx[i] = S.rows[(size_t)(h.rp + i - nc)];
                if (leaf) continue;
                int* slot = idx + fmax;
                const int64_t lc0 = (int64_t)h.c0 + h.rp;
                for (int i = 0; i < fmax; ++i) {
                    int* g = slot + 8 * (int64_t)i;
                    g[0] = 0;
                    for (int j = 1; j <= 6; ++j) g[j] = -1;
                    g[7] = 0;
                    if (i >= f) continue;
                    const int64_t g0 = glptr[(size_t)(lc0 + i)], g1 = glptr[(size_t)(lc0 + i + 1)];
                    g[0] = (int)(g1 - g0);
                    for (int j = 0; j < 6 && g0 + j < g1; ++j) g[1 + j] = gsrc[(size_t)(g0 + j)];
                    g[7] = (int)(g0 + 6);
                }
            }
        }
    }
}

}  // namespace

EngineTables build_engine_tables(const Symbolic& S, const Schedule& sch, FactorLists& fl, const std::vector<int>& dsigns)
{
    EngineTables T;
    mark_solve_pulled(S, sch, T);
    build_ncolpar(S, T);
    build_k_lists(S, sch, T);
    build_overlap_tables(S, sch, T);
    build_descs(S, sch, fl, T);
    build_cuts(S, T);
    build_gather_lists(S, T);
    build_tile_order(S, sch, fl, T);
    // what the device buffers of empty lists hold: one zero record
    if (fl.items.empty()) fl.items.push_back(ExtItem{});
    if (fl.pterms.empty()) fl.pterms.push_back(PullTerm{});
    if (fl.pwcut.empty()) fl.pwcut.push_back(0);
    build_records(S, sch, T);
    build_pull_lists(S, T);
    T.psign.resize((size_t)S.N);
    for (int k = 0; k < S.N; ++k) T.psign[k] = (signed char)(dsigns[S.perm[k]] >= 0 ? 1 : -1);
    const int block_rows = tall_block_rows(knobs().tall_block_rows);
    for (const Launch& L : sch.launches)
        if (L.ntall > 0) T.tall_ws = std::max(T.tall_ws, tall_ws_doubles(S.N, L.ntall, L.fmax, block_rows));
    return T;
}

// gather-list lengths of the rows of the persistent solve set (what k_top_solve's parked indices must cover)
std::string describe_gather_sources(const Symbolic& S, const Schedule& sch, const EngineTables& T)
{
    const std::vector<int64_t>& ptr = T.item_ptr;
    long hist[6] = {0, 0, 0, 0, 0, 0};
    long fronts_over8 = 0, fronts_over12 = 0, nf = 0;
    int64_t gmax = 0;
    for (size_t q = sch.launches.size() - sch.top_launches; q < sch.launches.size(); ++q)
        for (int t = sch.launches[q].begin; t < sch.launches[q].begin + sch.launches[q].count; ++t) {
            const int sn = sch.sched[(size_t)t];
            const int f = front_size(S, sn);
            int64_t fm = 0;
            for (int i = 0; i < f; ++i) {
                const int64_t n = ptr[lbase(S, sn) + i + 1] - ptr[lbase(S, sn) + i];
                hist[n == 0 ? 0 : n <= 4 ? 1 : n <= 8 ? 2 : n <= 12 ? 3 : n <= 16 ? 4 : 5]++;
                fm = std::max(fm, n);
            }
            gmax = std::max(gmax, fm);
            fronts_over8 += fm > 8; fronts_over12 += fm > 12; ++nf;
        }
    char buf[512];
    std::snprintf(buf, sizeof buf, "[hipkkt] persistent solve set: gather sources per row: 0: %ld, 1-4: %ld, 5-8: %ld, 9-12: %ld, "
                  "13-16: %ld, more: %ld (max %lld); fronts with a row over 8: %ld, over 12: %ld of %ld\n",
                  hist[0], hist[1], hist[2], hist[3], hist[4], hist[5], (long long)gmax, fronts_over8, fronts_over12, nf);
    return buf;
}

std::string describe_update_blocks(const Symbolic& S, const FactorLists& fl)
{
    int64_t n_dense = 0;
    for (int c : fl.dense_child) n_dense += c >= 0;
    char buf[512];
    std::snprintf(buf, sizeof buf, "[hipkkt] dense children: %lld\n", (long long)n_dense);
    std::string out = buf;
    std::snprintf(buf, sizeof buf, "[hipkkt] update blocks: %d chains of panels (%d links) share two buffers each; %lld bytes kept, %lld without sharing\n",
                  S.shared_chains, S.shared_links, (long long)(S.update_store * 8), (long long)(S.update_store_unshared * 8));
    return out + buf;
}

std::string describe_pulled_terms(const FactorLists& fl)
{
    char buf[256];
    std::snprintf(buf, sizeof buf, "[hipkkt] pulled leaves' terms: %zu chunks of 64, deepest stack %d\n", fl.pterms.size() / 64, fl.max_depth);
    return buf;
}

// the extend-add work of the last fronts of the schedule
std::string describe_panel_items(const Symbolic& S, const Schedule& sch, const FactorLists& fl)
{
    std::string out;
    char buf[512];
    for (size_t q = sch.sched.size() > 12 ? sch.sched.size() - 12 : 0; q < sch.sched.size(); ++q) {
        const int sn = sch.sched[q];
        const int64_t* w = fl.wcut.data() + (size_t)sn * 17;
        int64_t mx = 0, rows = 0;
        for (int k = 0; k < 16; ++k) mx = std::max(mx, w[k + 1] - w[k]);
        for (int64_t it = w[0]; it < w[16]; ++it) rows += fl.items[(size_t)it].cnt;
        std::snprintf(buf, sizeof buf, "[hipkkt] front %d f %d nc %d kids %d: %lld panel items (%lld entries), largest wave slice %lld\n",
                      sn, front_size(S, sn), S.sn_start[sn + 1] - S.sn_start[sn], S.child_ptr[sn + 1] - S.child_ptr[sn],
                      (long long)(w[16] - w[0]), (long long)rows, (long long)mx);
        out += buf;
    }
    return out;
}

std::string describe_tile_order(const EngineTables& T)
{
    char buf[128];
    std::snprintf(buf, sizeof buf, "[hipkkt] tile order: %d launches dealt to XCD residue classes (%lld tiles):", T.dealt_launches,
                  (long long)T.dealt_tiles);
    return buf + (T.dealt_launches ? T.dealt_list : std::string(" none")) + "\n";
}

std::string describe_records(const Schedule& sch)
{
    std::string out;
    char buf[128];
    if (sch.rec_refused_bytes) {
        std::snprintf(buf, sizeof buf, "[hipkkt] packed sweep records would take %.0f MB: legacy layout\n", sch.rec_refused_bytes / 1048576.0);
        out += buf;
    }
    if (sch.rec_bytes > 0) {
        std::snprintf(buf, sizeof buf, "[hipkkt] packed sweep records: %.1f MB\n", sch.rec_bytes / 1048576.0);
        out += buf;
    }
    return out;
}

std::string describe_solve_pulled(const EngineTables& T)
{
    char buf[256];
    std::snprintf(buf, sizeof buf, "[hipkkt] many-column sweeps: %lld of %lld contribution rows pulled from one-column leaves into %d sums\n",
                  (long long)T.n_pull_terms, (long long)T.item_ptr.back(), T.n_pull_rows);
    return buf;
}

}  // namespace hipkkt
