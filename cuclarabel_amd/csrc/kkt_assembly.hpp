// Host-side assembly of the triu CSC KKT matrix and its data maps (setup only).
// Follows /root/reference/src/kktsolvers/direct-ldl/directldl_kkt_assembly.jl:15-175,
// src/utils/csc_assembly.jl, directldl_datamaps.jl:8-79,170-214 and the cone layout of
// src/cones/compositecone_type.jl:114-141.  All indices 0-based, int32 on the way to the device.
#pragma once
#include <cstdint>
#include <vector>

namespace hipkkt {

struct ConeInfo {
    int kind;          // HIPKKT_CONE_*
    int dim;           // numel, or matrix side for PSD
    int numel;
    int off;           // rng_cones start (0-based) in (s, z)
    int64_t boff;      // rng_blocks start in Hsblocks
    int64_t blen;
    int sparse;        // SOC with dim > 4: sparse expansion
    int sidx;          // index among sparse SOCs
    int soff;          // offset into the concatenated u / v
    int nsidx;         // index among the exponential / power cones, -1 otherwise
    double param;      // alpha of a power cone
    // sparse expansion (directldl_datamaps.jl): columns [pcol, pcol + pwidth) behind n + m; a sparse second-order cone
    // has two, a generalized power cone three, every other cone none
    int pcol, pwidth;
    // generalized power cone (kind 6): index among them (-1 otherwise), dim1 = number of alphas, offsets into the
    // concatenated p (numel per cone), q (dim1 per cone) and r (dim2 per cone)
    int gpidx, dim1, gpoff, gqoff, groff;
};
// cones whose Hs block is a packed dense upper triangle
inline bool cone_is_dense(const ConeInfo& ci) { return ci.kind == 3 || (ci.kind == 2 && !ci.sparse) || ci.kind == 4 || ci.kind == 5; }

struct KKTAssembly {
    int n = 0, m = 0, p = 0, N = 0;
    int64_t nnzK = 0, nHs = 0;
    int nsparse = 0, sparse_len = 0;
    int nnonsym = 0;               // exponential + power cones
    int ngenpow = 0, genpow_len = 0, genpow_len1 = 0;   // generalized power cones, their rows, their alphas
    std::vector<double> gp_alpha;  // genpow_len1: the alphas, cone after cone
    std::vector<ConeInfo> cones;
    // triu CSC
    std::vector<int64_t> colptr;
    std::vector<int> rowval;
    std::vector<double> nzval;
    // LDLDataMap (directldl_datamaps.jl:170-214)
    std::vector<int> mapP, mapA, mapHs, map_diag, mapU, mapV, mapD;
    // GenPowExpansionMap (directldl_datamaps.jl:81-99), concatenated in cone order; mapGP_D has three entries per cone
    std::vector<int> mapGP_p, mapGP_q, mapGP_r, mapGP_D;
    std::vector<int> dsigns;       // kktsolver_directldl.jl:112-126
};

// P: triu CSC n x n; A: CSC m x n (any index base).  Throws std::runtime_error on bad input.
// param_ptr (ncones + 1 offsets in the same base) / param_vals: the ragged cone parameters -- one alpha for a power cone,
// dim1 alphas for a generalized power cone, none for every other kind.
void assemble_kkt(int64_t n, int64_t m, const int64_t* Pp, const int64_t* Pi, const double* Px,
                  const int64_t* Ap, const int64_t* Ai, const double* Ax, int64_t ncones,
                  const int32_t* kinds, const int64_t* dims, int base, KKTAssembly& K,
                  const int64_t* param_ptr = nullptr, const double* param_vals = nullptr);

// ---- the device tables of a KKT handle (hipkkt_kkt_create uploads them as they are)

// K's full-symmetric CSR image for the residual products: row i holds its lower partners (from its own column) and then
// the mirrored upper ones, so columns ascend within a row; vmap[d] = the K entry behind position d.  pend (rows < n): where
// the row's P entries end (columns ascend, so those are a prefix of the row) -- the reduced-system layer's P x products
// stop there instead of walking the row's A' entries as well (cfg3: ~250 of them per row behind a handful of P entries).
// kpos: the one (diagonal) or two positions of every K entry in the image, -1 for the second slot of a diagonal entry.
// Rows longer than kLongRow entries (launch_shapes.hpp) are listed in long_rows and cut into chunks of kLongChunk:
// chunk k of long row r is [chunk_q[2 k], chunk_q[2 k + 1]), k in [long_chunk_ptr[r], long_chunk_ptr[r + 1]).
struct KKTImage {
    std::vector<int64_t> ptr, pend;
    std::vector<int> col, vmap, kpos;
    std::vector<int> long_rows;
    std::vector<int64_t> long_chunk_ptr, chunk_q;
    int lanes_per_row = 8;         // lanes the residual kernel gives a row: 64 where rows average more than 24 entries
};
KKTImage build_kkt_image(const KKTAssembly& K);

// The cone tables (kernels.hpp: ConeDev): per cone its kind, rows, Hs block and sparse expansion; per row its cone; the
// lists by kind -- second-order, exponential, power, PSD by size class (side <= kPsdMaxDim: psd_list, the others:
// psdb_list), generalized power by size class (numel <= kGenPowWaveMax: gp_small) -- and the generalized power cones'
// per-row alphas and K positions (q, then r, concatenated per cone).
struct ConeTables {
    std::vector<int> kind, off, numel, sidx, soff, elem_cone, soc_list, soc_of_entry;
    std::vector<int64_t> boff;
    std::vector<int> exp_list, pow_list, ns_index;
    std::vector<double> param;
    std::vector<int> gp_cone, gp_dim1, gp_off, gp_small, gp_big, gp_mapQR;
    std::vector<double> gp_alpha;
    std::vector<int> psd_list, psdb_list, psd_dim;
    std::vector<int64_t> psd_aoff;
    int64_t psd_store = 0;         // doubles of all PSD cones' matrices (sum of side^2)
    bool has_psd = false, psd_too_big = false;
    int psd_kmax = 1, psdb_kmax = 1;
};
ConeTables build_cone_tables(const KKTAssembly& K);

}  // namespace hipkkt
