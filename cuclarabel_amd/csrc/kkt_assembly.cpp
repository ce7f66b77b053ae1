// See kkt_assembly.hpp.  Built column by column with explicit per-column writers instead of the
// reference's count / fill / back-shift passes over colptr; the resulting layout is the same:
// within each column rows ascend and the diagonal is the last entry
// (directldl_kkt_assembly.jl:161-165).
#include "kkt_assembly.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>

#include "../../include/hipkkt.h"
#include "launch_shapes.hpp"

namespace hipkkt {

static inline int64_t tri(int64_t k) { return k * (k + 1) / 2; }

void assemble_kkt(int64_t n64, int64_t m64, const int64_t* Pp, const int64_t* Pi, const double* Px,
                  const int64_t* Ap, const int64_t* Ai, const double* Ax, int64_t ncones,
                  const int32_t* kinds, const int64_t* dims, int base, KKTAssembly& K, const int64_t* param_ptr,
                  const double* param_vals)
{
    K = KKTAssembly();
    if (n64 < 0 || m64 < 0 || n64 + m64 > 1900000000) throw std::runtime_error("kkt: bad dimensions");
    const int n = (int)n64, m = (int)m64;
    K.n = n;
    K.m = m;
    // ---- cone layout (compositecone_type.jl:114-141)
    int64_t off = 0, boff = 0;
    for (int64_t c = 0; c < ncones; ++c) {
        ConeInfo ci{};
        ci.kind = kinds[c];
        if (ci.kind < HIPKKT_CONE_ZERO || ci.kind > HIPKKT_CONE_GENPOW) throw std::runtime_error("kkt: unknown cone kind");
        ci.nsidx = -1;
        ci.gpidx = -1;
        const int64_t npar = param_ptr ? param_ptr[c + 1] - param_ptr[c] : 0;
        const double* par = param_ptr ? param_vals + (param_ptr[c] - base) : nullptr;
        if (npar < 0 || (npar > 0 && !param_vals)) throw std::runtime_error("kkt: malformed cone_param_ptr / cone_param_vals");
        if (ci.kind == HIPKKT_CONE_EXP || ci.kind == HIPKKT_CONE_POW) {
            if (dims[c] != 3) throw std::runtime_error("kkt: exponential and power cones have dimension 3");
            if (ci.kind == HIPKKT_CONE_POW) {
                if (npar != 1)
                    throw std::runtime_error("kkt: a power cone needs its alpha: use hipkkt_kkt_create_ex with cone_params");
                ci.param = par[0];
                if (!(ci.param > 0.0 && ci.param < 1.0)) throw std::runtime_error("kkt: power cone alpha must lie in (0, 1)");
            }
            ci.nsidx = K.nnonsym++;
        }
        if (dims[c] < 0) throw std::runtime_error("kkt: negative cone dimension");
        if (ci.kind == HIPKKT_CONE_GENPOW) {
            // GenPowerConeT's constructor (cone_api.jl:37-47); dims[c] = dim1 + dim2
            if (npar < 1) throw std::runtime_error("kkt: a generalized power cone needs dim1 >= 1 alphas: use hipkkt_kkt_create_ex2");
            if (dims[c] - npar < 1) throw std::runtime_error("kkt: a generalized power cone needs dim2 = dim - dim1 >= 1");
            double sum = 0.0;
            for (int64_t i = 0; i < npar; ++i) {
                if (!(par[i] > 0.0) || !std::isfinite(par[i]))
                    throw std::runtime_error("kkt: generalized power cone alphas must be positive and finite");
                sum += par[i];
            }
            if (!(std::fabs(sum - 1.0) <= std::numeric_limits<double>::epsilon() * (double)npar / 2.0))
                throw std::runtime_error("kkt: generalized power cone alphas must sum to 1");
            ci.gpidx = K.ngenpow++;
            ci.dim1 = (int)npar;
            ci.gpoff = K.genpow_len;
            ci.gqoff = K.genpow_len1;
            ci.groff = K.genpow_len - K.genpow_len1;
            K.genpow_len += (int)dims[c];
            K.genpow_len1 += (int)npar;
            K.gp_alpha.insert(K.gp_alpha.end(), par, par + npar);
        }
        ci.dim = (int)dims[c];
        ci.numel = ci.kind == HIPKKT_CONE_PSD ? (int)tri(dims[c]) : (int)dims[c];
        if (ci.kind == HIPKKT_CONE_SOC && ci.dim < 2) throw std::runtime_error("kkt: second-order cone needs dim >= 2");
        ci.off = (int)off;
        off += ci.numel;
        ci.sparse = (ci.kind == HIPKKT_CONE_SOC && ci.dim > 4) ? 1 : 0;     // cone_types.jl:101-112
        ci.boff = boff;
        bool dense = cone_is_dense(ci);
        ci.blen = dense ? tri(ci.numel) : ci.numel;
        boff += ci.blen;
        if (ci.sparse) {
            ci.sidx = K.nsparse++;
            ci.soff = K.sparse_len;
            K.sparse_len += ci.numel;
        }
        // sparse maps are taken in cone order and pcol += pdim(map) (directldl_kkt_assembly.jl:77-98)
        ci.pcol = K.p;
        ci.pwidth = ci.sparse ? 2 : ci.kind == HIPKKT_CONE_GENPOW ? 3 : 0;
        K.p += ci.pwidth;
        K.cones.push_back(ci);
    }
    if (off != m) throw std::runtime_error("kkt: cone dimensions do not sum to m");
    K.nHs = boff;
    const int N = K.N = n + m + K.p;

    // ---- the caller's CSC arrays: a wrong index_base or a malformed colptr must end as an argument error, not as
    // host writes out of bounds further down
    auto check_csc = [&](const char* what, const int64_t* cp, const int64_t* ri, const double* vx, int64_t nrows) {
        if (!cp) throw std::runtime_error(std::string("kkt: ") + what + " colptr is null");
        if (cp[0] != base) throw std::runtime_error(std::string("kkt: ") + what + " colptr[0] does not equal index_base");
        for (int j = 0; j < n; ++j)
            if (cp[j + 1] < cp[j]) throw std::runtime_error(std::string("kkt: ") + what + " colptr is not non-decreasing");
        const int64_t nnz = cp[n] - base;
        if (nnz >= ((int64_t)1 << 31)) throw std::runtime_error(std::string("kkt: ") + what + " has too many entries");
        if (nnz > 0 && (!ri || !vx)) throw std::runtime_error(std::string("kkt: ") + what + " rowval / nzval is null");
        for (int64_t q = 0; q < nnz; ++q) {
            const int64_t r = ri[q] - base;
            if (r < 0 || r >= nrows) throw std::runtime_error(std::string("kkt: ") + what + " row index out of range");
        }
    };
    check_csc("P", Pp, Pi, Px, n);
    check_csc("A", Ap, Ai, Ax, m);

    // ---- column lengths
    std::vector<int64_t> len((size_t)N, 0);
    const int64_t nnzP = Pp[n] - base, nnzA = Ap[n] - base;
    std::vector<char> has_diag((size_t)n, 0);
    for (int j = 0; j < n; ++j) {
        int64_t b = Pp[j] - base, e = Pp[j + 1] - base;
        for (int64_t q = b; q < e; ++q) {
            int64_t i = Pi[q] - base;
            if (i > j) throw std::runtime_error("kkt: P must be upper triangular");
            if (q > b && Pi[q] <= Pi[q - 1]) throw std::runtime_error("kkt: P rows must ascend within a column");
        }
        has_diag[j] = (e > b && Pi[e - 1] - base == j) ? 1 : 0;     // csc_assembly.jl:36-48
        len[j] = (e - b) + (has_diag[j] ? 0 : 1);
    }
    for (int64_t q = 0; q < nnzA; ++q) {
        int64_t r = Ai[q] - base;
        if (r < 0 || r >= m) throw std::runtime_error("kkt: A row index out of range");
        len[n + r] += 1;
    }
    for (const ConeInfo& ci : K.cones) {
        const int pcol = n + m + ci.pcol;
        bool dense = cone_is_dense(ci);
        for (int t = 0; t < ci.numel; ++t) len[n + ci.off + t] += dense ? t + 1 : 1;
        if (ci.sparse) {
            len[pcol] += ci.numel + 1;
            len[pcol + 1] += ci.numel + 1;
        } else if (ci.kind == HIPKKT_CONE_GENPOW) {          // q, r, p (directldl_datamaps.jl:101-122)
            len[pcol] += ci.dim1 + 1;
            len[pcol + 1] += ci.numel - ci.dim1 + 1;
            len[pcol + 2] += ci.numel + 1;
        }
    }
    K.colptr.assign((size_t)N + 1, 0);
    for (int j = 0; j < N; ++j) K.colptr[j + 1] = K.colptr[j] + len[j];
    K.nnzK = K.colptr[N];
    if (K.nnzK >= ((int64_t)1 << 31)) throw std::runtime_error("kkt: nnz(K) exceeds int32 indexing");
    K.rowval.assign((size_t)K.nnzK, 0);
    K.nzval.assign((size_t)K.nnzK, 0.0);
    K.mapP.assign((size_t)nnzP, 0);
    K.mapA.assign((size_t)nnzA, 0);
    K.mapHs.assign((size_t)K.nHs, 0);
    K.map_diag.assign((size_t)N, 0);
    K.mapU.assign((size_t)K.sparse_len, 0);
    K.mapV.assign((size_t)K.sparse_len, 0);
    K.mapD.assign((size_t)2 * K.nsparse, 0);
    K.mapGP_p.assign((size_t)K.genpow_len, 0);
    K.mapGP_q.assign((size_t)K.genpow_len1, 0);
    K.mapGP_r.assign((size_t)(K.genpow_len - K.genpow_len1), 0);
    K.mapGP_D.assign((size_t)3 * K.ngenpow, 0);

    std::vector<int64_t> nxt(K.colptr.begin(), K.colptr.end() - 1);
    auto put = [&](int col, int row, double v) -> int {
        int64_t d = nxt[col]++;
        K.rowval[d] = row;
        K.nzval[d] = v;
        return (int)d;
    };
    // upper-left block: triu(P) plus structural zeros on a missing diagonal (csc_assembly.jl:207-220)
    for (int j = 0; j < n; ++j) {
        for (int64_t q = Pp[j] - base; q < Pp[j + 1] - base; ++q) K.mapP[q] = put(j, (int)(Pi[q] - base), Px[q]);
        if (!has_diag[j]) put(j, j, 0.0);
    }
    // upper-right block: A transposed (csc_assembly.jl:125-143 with shape :T)
    for (int j = 0; j < n; ++j)
        for (int64_t q = Ap[j] - base; q < Ap[j + 1] - base; ++q) K.mapA[q] = put(n + (int)(Ai[q] - base), j, Ax[q]);
    // lower-right blocks per cone, then the sparse-expansion columns (v first, then u)
    for (const ConeInfo& ci : K.cones) {
        const int pcol = n + m + ci.pcol;
        int row0 = n + ci.off;
        int* block = K.mapHs.data() + ci.boff;
        bool dense = cone_is_dense(ci);
        if (dense) {
            int64_t kidx = 0;
            for (int t = 0; t < ci.numel; ++t)
                for (int r = 0; r <= t; ++r) block[kidx++] = put(row0 + t, row0 + r, 0.0);
        } else {
            for (int t = 0; t < ci.numel; ++t) block[t] = put(row0 + t, row0 + t, 0.0);
        }
        if (ci.sparse) {
            for (int t = 0; t < ci.numel; ++t) K.mapV[ci.soff + t] = put(pcol, row0 + t, 0.0);
            for (int t = 0; t < ci.numel; ++t) K.mapU[ci.soff + t] = put(pcol + 1, row0 + t, 0.0);
            K.mapD[2 * ci.sidx] = put(pcol, pcol, 0.0);
            K.mapD[2 * ci.sidx + 1] = put(pcol + 1, pcol + 1, 0.0);
        } else if (ci.kind == HIPKKT_CONE_GENPOW) {          // directldl_datamaps.jl:124-144, triu
            const int d1 = ci.dim1, d2 = ci.numel - ci.dim1;
            for (int t = 0; t < d1; ++t) K.mapGP_q[ci.gqoff + t] = put(pcol, row0 + t, 0.0);
            for (int t = 0; t < d2; ++t) K.mapGP_r[ci.groff + t] = put(pcol + 1, row0 + d1 + t, 0.0);
            for (int t = 0; t < ci.numel; ++t) K.mapGP_p[ci.gpoff + t] = put(pcol + 2, row0 + t, 0.0);
            for (int t = 0; t < 3; ++t) K.mapGP_D[3 * ci.gpidx + t] = put(pcol + t, pcol + t, 0.0);
        }
    }
    for (int j = 0; j < N; ++j) {
        if (nxt[j] != K.colptr[j + 1]) throw std::runtime_error("kkt: internal column fill mismatch");
        K.map_diag[j] = (int)(K.colptr[j + 1] - 1);
        if (K.rowval[K.map_diag[j]] != j) throw std::runtime_error("kkt: diagonal is not last in column");
    }
    // expected pivot signs
    K.dsigns.assign((size_t)N, 1);
    for (int i = n; i < n + m; ++i) K.dsigns[i] = -1;
    for (const ConeInfo& ci : K.cones) {
        const int pcol = n + m + ci.pcol;
        if (ci.sparse) {
            K.dsigns[pcol] = -1;               // Dsigns(::SOCExpansionMap) = (-1, 1)
            K.dsigns[pcol + 1] = 1;
        } else if (ci.kind == HIPKKT_CONE_GENPOW) {
            K.dsigns[pcol] = -1;               // Dsigns(::GenPowExpansionMap) = (-1, -1, 1)
            K.dsigns[pcol + 1] = -1;
            K.dsigns[pcol + 2] = 1;
        }
    }
}

KKTImage build_kkt_image(const KKTAssembly& K)
{
    KKTImage I;
    const int N = K.N;
    std::vector<int64_t>& ptr = I.ptr;
    ptr.assign((size_t)N + 1, 0);
    for (int j = 0; j < N; ++j)
        for (int64_t q = K.colptr[j]; q < K.colptr[j + 1]; ++q) {
            int i = K.rowval[q];
            ptr[i + 1]++;
            if (i != j) ptr[j + 1]++;
        }
    for (int i = 0; i < N; ++i) ptr[i + 1] += ptr[i];
    std::vector<int>&col = I.col, &vmap = I.vmap;
    col.assign((size_t)ptr[N], 0);
    vmap.assign((size_t)ptr[N], 0);
    std::vector<int64_t> nx(ptr.begin(), ptr.end() - 1);
    // row i gets its upper-triangle partners (i, j>i) from column scans in ascending j and its
    // lower partners from its own column; fill lower part first so columns ascend within a row
    for (int j = 0; j < N; ++j) {            // entries (i<j) stored in column j: row j, col i
        for (int64_t q = K.colptr[j]; q < K.colptr[j + 1]; ++q) {
            int i = K.rowval[q];
            int64_t d = nx[j]++;
            col[d] = i;
            vmap[d] = (int)q;
        }
    }
    for (int j = 0; j < N; ++j)              // mirrored entries: row i, col j (j > i), ascending j
        for (int64_t q = K.colptr[j]; q < K.colptr[j + 1]; ++q) {
            int i = K.rowval[q];
            if (i == j) continue;
            int64_t d = nx[i]++;
            col[d] = j;
            vmap[d] = (int)q;
        }
    I.pend.assign((size_t)std::max<int64_t>(K.n, 1), 0);
    for (int64_t i = 0; i < K.n; ++i)
        I.pend[(size_t)i] = std::lower_bound(col.begin() + ptr[(size_t)i], col.begin() + ptr[(size_t)i + 1], (int)K.n) - col.begin();
    I.kpos.assign((size_t)2 * K.nnzK, -1);
    for (size_t q = 0; q < vmap.size(); ++q) {
        const size_t e = (size_t)vmap[q];
        if (I.kpos[2 * e] < 0) I.kpos[2 * e] = (int)q; else I.kpos[2 * e + 1] = (int)q;
    }
    I.long_chunk_ptr.assign(1, 0);
    for (int i = 0; i < N; ++i) {
        const int64_t len = ptr[i + 1] - ptr[i];
        if (len <= kLongRow) continue;
        I.long_rows.push_back(i);
        for (int64_t q = ptr[i]; q < ptr[i + 1]; q += kLongChunk) {
            I.chunk_q.push_back(q);
            I.chunk_q.push_back(std::min<int64_t>(q + kLongChunk, ptr[i + 1]));
        }
        I.long_chunk_ptr.push_back((int64_t)I.chunk_q.size() / 2);
    }
    double avg = (double)ptr[N] / std::max(N, 1);
    I.lanes_per_row = avg > 24.0 ? 64 : 8;
    return I;
}

ConeTables build_cone_tables(const KKTAssembly& K)
{
    ConeTables C;
    const size_t nc = K.cones.size();
    C.kind.resize(nc); C.off.resize(nc); C.numel.resize(nc); C.sidx.resize(nc); C.soff.resize(nc); C.boff.resize(nc);
    C.elem_cone.assign((size_t)K.m, 0);
    C.ns_index.assign(nc, -1);
    C.param.assign(nc, 0.0);
    C.soc_of_entry.assign((size_t)K.sparse_len, 0);
    for (size_t c = 0; c < nc; ++c) {
        const ConeInfo& ci = K.cones[c];
        C.kind[c] = ci.kind; C.off[c] = ci.off; C.numel[c] = ci.numel; C.boff[c] = ci.boff;
        C.sidx[c] = ci.sparse ? ci.sidx : -1;
        C.soff[c] = ci.sparse ? ci.soff : -1;
        for (int t = 0; t < ci.numel; ++t) C.elem_cone[ci.off + t] = (int)c;
        if (ci.kind == HIPKKT_CONE_SOC) C.soc_list.push_back((int)c);
        if (ci.kind == HIPKKT_CONE_EXP) C.exp_list.push_back((int)c);
        if (ci.kind == HIPKKT_CONE_POW) C.pow_list.push_back((int)c);
        C.ns_index[c] = ci.nsidx; C.param[c] = ci.param;
        if (ci.kind == HIPKKT_CONE_PSD) {
            C.has_psd = true;
            if (ci.dim > kPsdMaxDim) C.psd_too_big = true;
        }
        if (ci.sparse) for (int t = 0; t < ci.numel; ++t) C.soc_of_entry[ci.soff + t] = ci.sidx;
    }
    if (K.ngenpow > 0) {
        C.gp_mapQR.assign((size_t)K.genpow_len, 0);
        C.gp_alpha.assign((size_t)K.genpow_len, 0.0);
        for (size_t c = 0; c < nc; ++c) {
            const ConeInfo& ci = K.cones[c];
            if (ci.kind != HIPKKT_CONE_GENPOW) continue;
            C.gp_cone.push_back((int)c); C.gp_dim1.push_back(ci.dim1); C.gp_off.push_back(ci.gpoff);
            (ci.numel <= kGenPowWaveMax ? C.gp_small : C.gp_big).push_back(ci.gpidx);
            for (int t = 0; t < ci.dim1; ++t) {
                C.gp_alpha[ci.gpoff + t] = K.gp_alpha[ci.gqoff + t];
                C.gp_mapQR[ci.gpoff + t] = K.mapGP_q[ci.gqoff + t];
            }
            for (int t = ci.dim1; t < ci.numel; ++t) C.gp_mapQR[ci.gpoff + t] = K.mapGP_r[ci.groff + t - ci.dim1];
        }
    }
    C.psd_dim.assign(nc, 0);
    C.psd_aoff.assign(nc, 0);
    for (size_t c = 0; c < nc; ++c) {
        const ConeInfo& ci = K.cones[c];
        if (ci.kind != HIPKKT_CONE_PSD) continue;
        C.psd_dim[c] = ci.dim;
        C.psd_aoff[c] = C.psd_store;
        C.psd_store += (int64_t)ci.dim * ci.dim;
        // two size classes, as gp_small / gp_big: the all-in-LDS kernels see sides <= kPsdMaxDim only
        if (ci.dim <= kPsdMaxDim) { C.psd_list.push_back((int)c); C.psd_kmax = std::max(C.psd_kmax, ci.dim); }
        else { C.psdb_list.push_back((int)c); C.psdb_kmax = std::max(C.psdb_kmax, ci.dim); }
    }
    return C;
}

}  // namespace hipkkt
