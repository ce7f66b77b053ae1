/*
 * hipkkt.h -- C ABI of libhipkkt.so: an MI355X-native (HIP, gfx950) KKT linear-system solver
 * that drops in behind Clarabel.jl's KKT-solver interfaces.  fp64 throughout.
 *
 * Two boundaries are exported, plus the two layers either side of them
 * (section 8f); citations are into /root/reference:
 *
 *   Level A  hipkkt_ldl_*   replaces an AbstractDirectLDLSolver backend
 *            contract  src/kktsolvers/direct-ldl/directldl_defaults.jl:1-72
 *            example   src/kktsolvers/direct-ldl/directldl_qdldl.jl:1-96   (the CPU path)
 *   Level B  hipkkt_kkt_*   replaces the whole DirectLDLKKTSolver <: AbstractKKTSolver
 *            contract  src/kktsolvers/kktsolver_defaults.jl:2-48
 *            example   src/kktsolvers/kktsolver_directldl.jl:5-466
 *   Level C  hipkkt_kkt_system_*   the caller of level B, DefaultKKTSystem, with its vectors in HBM
 *            src/kktsystem.jl:21-215  (kkt_update!, kkt_solve_initial_point!, kkt_solve!)
 *   Data     hipkkt_equilibrate / hipkkt_scale_matrix_values   Ruiz equilibration before level B is built
 *            src/problemdata.jl:133-242, src/data_updating.jl:169-194
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every array it passes and may free or
 *     move it as soon as the call returns (the library copies during the call).
 *   - index arrays are int64 with the caller's `index_base` (1 for Julia, 0 for C/Python).
 *   - return value: 0 = success; > 0 = numeric failure (non-finite pivot or residual), which the
 *     reference reports as `false` (directldl_qdldl.jl:79, kktsolver_directldl.jl:411,429);
 *     < 0 = usage or HIP error (hipkkt_last_error() has the text).
 *   - one handle = one HIP stream; calls on one handle must be sequential (the reference calls
 *     its backend from one thread: update_values!* -> refactor! -> solve!*).
 *   - functions ending in _dev take DEVICE pointers (resident in HBM on the handle's device) and
 *     are asynchronous on the handle's stream unless they return a status that needs a read-back.
 */
#ifndef HIPKKT_H
#define HIPKKT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPKKT_OK 0
#define HIPKKT_NUMERIC_FAILURE 1
#define HIPKKT_REFINEMENT_INCOMPLETE 2   /* hipkkt_kkt_deferred_status only */
#define HIPKKT_ERR_ARG (-1)
#define HIPKKT_ERR_HIP (-2)
#define HIPKKT_ERR_INTERNAL (-3)

/* cone kinds (src/cones/cone_api.jl:18-55); dims[] = numel, except PSD: matrix side */
#define HIPKKT_CONE_ZERO 0
#define HIPKKT_CONE_NN 1
#define HIPKKT_CONE_SOC 2
#define HIPKKT_CONE_PSD 3
/* the non-symmetric cones (coneops_expcone.jl, coneops_powcone.jl): dims[] must be 3.  A power cone's alpha comes
 * through hipkkt_kkt_create_ex. */
#define HIPKKT_CONE_EXP 4
#define HIPKKT_CONE_POW 5
/* the generalized power cone (coneops_genpowcone.jl): prod_i s_i^alpha_i >= ||s[dim1:]||, s[:dim1] >= 0.  dims[] is
 * dim1 + dim2; dim1 is the number of alphas the cone gets through hipkkt_kkt_create_ex2.  It has no unexpanded form:
 * its rows carry a DIAGONAL Hs block and K gets three expansion columns behind n + m -- q (rows 0 .. dim1 of the cone),
 * r (rows dim1 .. dim), p (all rows) -- with Dsigns (-1, -1, +1), in cone order among the sparse second-order cones'
 * pairs of columns (directldl_datamaps.jl:81-167). */
#define HIPKKT_CONE_GENPOW 6

/* scaling strategy of the non-symmetric cones (types.jl:74) */
#define HIPKKT_SCALING_PRIMAL_DUAL 0
#define HIPKKT_SCALING_DUAL 1

/* fill-reducing ordering */
#define HIPKKT_ORDER_AMD 0      /* approximate minimum degree (what the reference asks QDLDL for) */
#define HIPKKT_ORDER_ND 1       /* nested dissection over AMD leaves: short, bushy trees (default) */
#define HIPKKT_ORDER_NATURAL 2
#define HIPKKT_ORDER_USER 3     /* settings.user_perm */

typedef struct hipkkt_ldl_s *hipkkt_ldl_t;
typedef struct hipkkt_kkt_s *hipkkt_kkt_t;

/* mirrors the path-relevant fields of Clarabel.Settings (src/settings.jl:110-132) */
typedef struct {
    double static_regularization_constant;      /* 1e-8   :118 */
    double static_regularization_proportional;  /* eps^2  :119 */
    double dynamic_regularization_eps;          /* 1e-13  :123 */
    double dynamic_regularization_delta;        /* 2e-7   :124 */
    double iterative_refinement_reltol;         /* 1e-13  :128 */
    double iterative_refinement_abstol;         /* 1e-12  :129 */
    double iterative_refinement_stop_ratio;     /* 5      :131 */
    int32_t iterative_refinement_max_iter;      /* 10     :130 */
    int32_t static_regularization_enable;       /* true   :117 */
    int32_t iterative_refinement_enable;        /* true   :127 */
    int32_t ordering;                           /* HIPKKT_ORDER_*, default ND */
    int32_t nd_leaf_size;                       /* sub-domain size below which ND hands over to AMD */
    int32_t device;                             /* HIP device ordinal, -1 = current */
    const int64_t *user_perm;                   /* length N, caller's index base; ORDER_USER only */
    double amd_dense_scale;                     /* 1.5 (directldl_qdldl.jl:24) */
} hipkkt_settings;

typedef struct {
    int64_t n, m, p, N;        /* N = n + m + p, p = 2 per sparse second-order cone */
    int64_t nnzK;              /* entries of the triu KKT matrix */
    int64_t nnzL;              /* structural nnz(L) (QDLDL's count; what linear_solver_info reports) */
    int64_t nnzL_stored;       /* incl. explicit zeros of amalgamated supernodes */
    int64_t nsuper, nlevels, max_front, etree_height;
    int64_t nHs;               /* length of Hsblocks */
    int64_t nsparse_soc, sparse_soc_len;
    double factor_flops;
    double front_bytes, update_bytes;
} hipkkt_info;

/* accumulated device time per phase (hipEvents on the handle's stream), for bench.py */
typedef struct {
    double update_ms, factor_ms, trisolve_ms, residual_ms, other_ms;
    int64_t n_update, n_factor, n_trisolve, n_residual;
    int64_t ir_iterations;     /* refinement rounds beyond the first residual check */
    int64_t dynamic_regularizations;
    /* Fallbacks taken over the handle's LIFETIME (not cleared by hipkkt_kkt_profile_reset): a bounded wait of the
     * factorisation's overlap mode / of the persistent top-of-tree sweep kernel expired, the mechanism was switched off
     * for the handle and the operation repeated level by level.  The reference has nothing like it (its only report is the
     * Bool of refactor! / solve!, directldl_qdldl.jl:79): results stay correct, but a non-zero count means a 50 ms stall
     * happened and the handle runs on its slower path from then on.  Expected value: 0. */
    int64_t overlap_fallbacks, top_fallbacks;
    /* Factorisations of this handle (lifetime) that ran level by level because ANOTHER handle's overlapped factorisation
     * was in flight on the device: one overlapped factorisation per device at a time (the mode's forward-progress
     * argument needs every other kernel on the device to end by itself).  Not a fallback: no stall, nothing is
     * switched off, the next factorisation asks again. */
    int64_t overlap_deferrals;
    /* ... and sweeps that took the chained kernels instead of the persistent one for the same reason (one kernel with a
     * residency requirement per device at a time, whichever handle's). */
    int64_t top_deferrals;
} hipkkt_profile;

/* -------------------------------------------------------------------- general */
int hipkkt_available(void);                 /* 1 if a gfx950 device is usable; never throws
                                               (ldlsolver_is_available, directldl_defaults.jl:22-27) */
const char *hipkkt_last_error(void);
void hipkkt_default_settings(hipkkt_settings *s);
const char *hipkkt_version(void);

/* host-only symbolic analysis of a triu CSC pattern (no GPU needed): fill-reducing permutation
 * (perm[k] = 0-based original index eliminated k-th) and the structure statistics.  This is the
 * setup step QDLDL.qdldl(...; logical=true) performs for the reference (directldl_qdldl.jl:18-25). */
int hipkkt_symbolic_analyse(int64_t N, const int64_t *colptr, const int64_t *rowval, int index_base,
                            int ordering, int nd_leaf_size, int64_t *perm_out, hipkkt_info *info_out);

/* ------------------------------------------- Level A: AbstractDirectLDLSolver */
/* constructor (directldl_qdldl.jl:6-28): symbolic analysis of the triu CSC matrix K, keeps a
 * device copy of nzval.  dsigns: +1/-1 expected pivot signs (kktsolver_directldl.jl:112-126). */
int hipkkt_ldl_create(hipkkt_ldl_t *out, int64_t N, const int64_t *colptr, const int64_t *rowval,
                      const double *nzval, const int64_t *dsigns, const hipkkt_settings *settings,
                      int index_base);
void hipkkt_ldl_destroy(hipkkt_ldl_t h);
/* update_values! / scale_values! (directldl_qdldl.jl:46-68): index = positions in K.nzval */
int hipkkt_ldl_update_values(hipkkt_ldl_t h, const int64_t *index, const double *values, int64_t k);
int hipkkt_ldl_scale_values(hipkkt_ldl_t h, const int64_t *index, double scale, int64_t k);
/* refactor! (directldl_qdldl.jl:72-81): numeric LDL^T; 1 if some pivot is not finite */
int hipkkt_ldl_refactor(hipkkt_ldl_t h);
/* solve! (directldl_qdldl.jl:85-96): x = K^{-1} b, host vectors of length N, x != b allowed */
int hipkkt_ldl_solve(hipkkt_ldl_t h, double *x, const double *b);
int hipkkt_ldl_solve_dev(hipkkt_ldl_t h, double *d_x, const double *d_b);
/* solve! for nrhs right-hand sides against the same factors (SURVEY.md 8b "batched", 8e(ii):
 * the reference has no such call -- its solve! at directldl_qdldl.jl:85-96 takes one vector --
 * a caller with several vectors loops over it).  X, B: N x nrhs column-major, host (ld = N) or
 * device (ldx, ldb >= N); X may alias B.  Column j's result equals hipkkt_ldl_solve on column j. */
int hipkkt_ldl_solve_multi(hipkkt_ldl_t h, int64_t nrhs, double *X, const double *B);
int hipkkt_ldl_solve_multi_dev(hipkkt_ldl_t h, int64_t nrhs, double *d_X, int64_t ldx,
                               const double *d_B, int64_t ldb);
/* linear_solver_info (directldl_qdldl.jl:35-42) */
int hipkkt_ldl_info(hipkkt_ldl_t h, hipkkt_info *info);
int hipkkt_ldl_get_perm(hipkkt_ldl_t h, int64_t *perm /* N, 0-based */);
/* out[0] = overlap-mode fallbacks, out[1] = persistent-sweep-kernel fallbacks of this handle so far (see hipkkt_profile) */
int hipkkt_ldl_fallbacks(hipkkt_ldl_t h, int64_t out[2]);

/* ---------------------------------------------- Level B: AbstractKKTSolver */
/* constructor (kktsolver_directldl.jl:46-92): P n x n triu CSC, A m x n CSC, cone list.
 * Does the KKT assembly + data maps (directldl_kkt_assembly.jl:15-175), Dsigns, symbolic LDL. */
int hipkkt_kkt_create(hipkkt_kkt_t *out, int64_t n, int64_t m,
                      const int64_t *Pcolptr, const int64_t *Prowval, const double *Pnzval,
                      const int64_t *Acolptr, const int64_t *Arowval, const double *Anzval,
                      int64_t ncones, const int32_t *cone_kinds, const int64_t *cone_dims,
                      const hipkkt_settings *settings, int index_base);
/* hipkkt_kkt_create plus one double per cone: alpha of a power cone, in (0, 1); ignored for every other kind.
 * cone_params may be NULL when the list holds no power cone.  hipkkt_kkt_create forwards here with NULL: it takes
 * exponential cones and refuses power cones.
 * An exponential or power cone is a dense 3 x 3 block of K with 6 packed-triu Hs entries -- the layout of a
 * second-order cone of dimension 3 -- with no expansion columns and Dsigns -1 on its rows. */
int hipkkt_kkt_create_ex(hipkkt_kkt_t *out, int64_t n, int64_t m,
                         const int64_t *Pcolptr, const int64_t *Prowval, const double *Pnzval,
                         const int64_t *Acolptr, const int64_t *Arowval, const double *Anzval,
                         int64_t ncones, const int32_t *cone_kinds, const int64_t *cone_dims,
                         const double *cone_params, const hipkkt_settings *settings, int index_base);
/* hipkkt_kkt_create_ex with RAGGED cone parameters: cone c has the values cone_param_vals[cone_param_ptr[c] ..
 * cone_param_ptr[c + 1]) (ncones + 1 offsets in index_base).  A power cone has one value (alpha), a generalized power
 * cone its dim1 >= 1 values of alpha, every other kind none.  Both may be NULL when no cone has a parameter.  A
 * generalized power cone is validated as GenPowerConeT is (cone_api.jl:37-47): every alpha positive and finite,
 * |sum(alpha) - 1| <= eps dim1 / 2, and dim2 = cone_dims[c] - dim1 >= 1.
 * hipkkt_kkt_create and hipkkt_kkt_create_ex forward here; given HIPKKT_CONE_GENPOW they return HIPKKT_ERR_ARG.
 * A handle that holds a generalized power cone is scaled on the device only (hipkkt_kkt_update_from_sz[_dev],
 * hipkkt_kkt_system_update*): hipkkt_kkt_update_cones, hipkkt_kkt_system_update_cones and
 * hipkkt_kkt_system_update_scaling have no way to receive its p, q, r and return HIPKKT_ERR_ARG on it. */
int hipkkt_kkt_create_ex2(hipkkt_kkt_t *out, int64_t n, int64_t m,
                          const int64_t *Pcolptr, const int64_t *Prowval, const double *Pnzval,
                          const int64_t *Acolptr, const int64_t *Arowval, const double *Anzval,
                          int64_t ncones, const int32_t *cone_kinds, const int64_t *cone_dims,
                          const int64_t *cone_param_ptr, const double *cone_param_vals,
                          const hipkkt_settings *settings, int index_base);
void hipkkt_kkt_destroy(hipkkt_kkt_t h);
int hipkkt_kkt_info(hipkkt_kkt_t h, hipkkt_info *info);

/* kktsolver_update! (kktsolver_directldl.jl:197-294) with the cone data the reference reads from
 * its cones: Hsblocks = get_Hs! output (positive W'W blocks, |Hs| values), and for each sparse
 * second-order cone its u, v (concatenated) and eta^2.  Scatter, regularise, refactor. */
int hipkkt_kkt_update_cones(hipkkt_kkt_t h, const double *Hsblocks, const double *soc_u,
                            const double *soc_v, const double *soc_eta2);
/* device-native variant: NT scaling + Hs blocks computed on the device from (s, z)
 * (update_scaling! + get_Hs!, src/cones/coneops_*.jl), then as above.  Returns 1 also when a
 * point is not interior (update_scaling! returning false). */
int hipkkt_kkt_update_from_sz(hipkkt_kkt_t h, const double *s, const double *z);
int hipkkt_kkt_update_from_sz_dev(hipkkt_kkt_t h, const double *d_s, const double *d_z);
/* PSD cones of side 49 ... HIPKKT_PSD_MAX_SIDE_LARGE on the device, opt-in per handle.  update_scaling! of a PSD cone
 * (coneops_psdtrianglecone.jl:78-161: two Cholesky factors, the SVD of L2'L1, R, Rinv, Hs = RR' (x)_s RR') runs for
 * sides <= 48 in one workgroup with all six k x k work matrices in LDS; that is the default, and without this call a
 * handle with a larger PSD cone is refused by hipkkt_kkt_update_from_sz[_dev], by level C and by the cone operations
 * between the solves ("side > 48") exactly as before.  With
 * enable = 1 the cones of side 49 ... 96 are scaled by a second kernel class that keeps in LDS only the matrix pair
 * (M, V) the one-sided Jacobi SVD rotates and streams the rest through a per-handle work area in HBM, which this call
 * allocates; Hs is then formed by many workgroups per cone.  Why 96: 2 k^2 doubles are 147 456 B at k = 96, leaving
 * 16 KB of a CU's 160 KiB of LDS for the reduction arrays; at k = 100 they are 160 000 B and leave 3 840 B; 96 is the
 * last multiple of 16 that fits.  An enabled handle is taken by every entry point that takes side <= 48 without the
 * call: hipkkt_kkt_update_from_sz[_dev], hipkkt_kkt_mul_Hs, hipkkt_kkt_get_Hs / _get_scaling / _get_scaling_w, all of
 * level C (hipkkt_kkt_system_*) and the fourteen cone operations between the solves.  A cone of side > 96 stays
 * refused by the same guards, with a message that says "side > 96".  Cones of side <= 48 and all other cones launch what they
 * launch without the call and give the same bits.  May be called at any time between operations; it synchronises the
 * handle's stream, and a device-side scaling made under the other setting stops being valid (hipkkt_kkt_mul_Hs and
 * hipkkt_kkt_get_scaling then ask for a new hipkkt_kkt_update_from_sz).  hipkkt_kkt_update_cones, which takes any
 * side, is unaffected.  After an update that reports a cone point outside its cone, the Hs block of that cone is
 * unspecified (the small class leaves it as it was, the big class overwrites it).  Returns HIPKKT_OK, HIPKKT_ERR_ARG for a null handle, or a HIP error. */
#define HIPKKT_PSD_MAX_SIDE_LARGE 96
int hipkkt_kkt_enable_large_psd(hipkkt_kkt_t h, int enable);
/* kktsolver_update_P! / kktsolver_update_A! (kktsolver_directldl.jl:374-386) */
int hipkkt_kkt_update_P(hipkkt_kkt_t h, const double *Pnzval);
int hipkkt_kkt_update_A(hipkkt_kkt_t h, const double *Anzval);
/* kktsolver_setrhs! (:313-327) and kktsolver_solve! (:346-371, with iterative refinement
 * :389-449).  lhsx / lhsz may be NULL (Union{Nothing,...}). */
int hipkkt_kkt_setrhs(hipkkt_kkt_t h, const double *rhsx, const double *rhsz);
int hipkkt_kkt_solve(hipkkt_kkt_t h, double *lhsx, double *lhsz);
int hipkkt_kkt_setrhs_dev(hipkkt_kkt_t h, const double *d_rhsx, const double *d_rhsz);
int hipkkt_kkt_solve_dev(hipkkt_kkt_t h, double *d_lhsx, double *d_lhsz);
/* Deferred status (no counterpart in the reference, whose calls are synchronous): with defer = 1 the device-pointer
 * entry points hipkkt_kkt_update_from_sz_dev, hipkkt_kkt_solve_dev and hipkkt_kkt_solve_multi_dev with nrhs <= 8 (the
 * columns that share the single-column sweeps; ir_iterations then receives -1 per column) only ENQUEUE their work and
 * return 0 at once (hipkkt_kkt_solve_multi_dev with more than 8 columns always synchronises and returns its own status);
 * what they would have returned is accumulated on the device.  The refinement loop's accept / stop decisions
 * (kktsolver_directldl.jl:389-449) are taken on the device either way; in this mode a solve runs as many refinement
 * rounds ahead as the previous solves on the handle needed (at least one).  hipkkt_kkt_deferred_status synchronises,
 * returns the worst status since the previous query and clears it: 0, HIPKKT_NUMERIC_FAILURE (some pivot, cone point
 * or residual was not finite), or HIPKKT_REFINEMENT_INCOMPLETE (some solve stopped while the reference's loop would
 * have gone on: its result is the last accepted iterate; later solves run one more round ahead -- repeat the step,
 * or call hipkkt_kkt_solve_dev with defer = 0, for the reference's exact loop).  A caller issues a whole iteration's
 * update + solves and asks once. */
int hipkkt_kkt_set_deferred_status(hipkkt_kkt_t h, int defer);
int hipkkt_kkt_deferred_status(hipkkt_kkt_t h);
/* kktsolver_setrhs! + kktsolver_solve! for nrhs right-hand sides at once (SURVEY.md 8b
 * "hipkkt_kkt_solve_multi"): rhsx n x nrhs, rhsz m x nrhs, column-major, contiguous; lhsx / lhsz
 * likewise, either may be NULL.  Every column goes through the reference's refinement rule on its
 * own (kktsolver_directldl.jl:389-449) and ends where its single solve would; ir_iterations
 * (host, nrhs entries, may be NULL) receives the rounds each column took.  Returns 1 if any
 * column's residual is not finite.  Does not disturb the right-hand side set by hipkkt_kkt_setrhs. */
int hipkkt_kkt_solve_multi(hipkkt_kkt_t h, int64_t nrhs, const double *rhsx, const double *rhsz,
                           double *lhsx, double *lhsz, int64_t *ir_iterations);
int hipkkt_kkt_solve_multi_dev(hipkkt_kkt_t h, int64_t nrhs, const double *d_rhsx,
                               const double *d_rhsz, double *d_lhsx, double *d_lhsz,
                               int64_t *ir_iterations);
/* ------------------------------------------- Level C: DefaultKKTSystem, device-resident
 * The layer that calls the KKT solver three times per interior-point iteration
 * (/root/reference/src/kktsystem.jl:21-215) with all its vectors in HBM: right-hand-side
 * construction (Delta_s_from_Delta_z_offset!, coneops_compositecone.jl:185-202) and the recovery of
 * (dtau, dx, dz, ds, dkappa) (dots, quad_form mathutils.jl:299-337, mul_Hs!) run on the device, so
 * per solve only the scalars cross PCIe.  Vectors named d_* are
 * device pointers: x-like length n, s/z-like length m.  Covers zero, nonnegative, second-order and PSD
 * cones (PSD side <= 48, the limit of hipkkt_kkt_update_from_sz; <= 96 on a handle that has called
 * hipkkt_kkt_enable_large_psd). */
/* DefaultKKTSystem constructor (kktsystem.jl:21-52): q (n), b (m) host vectors, copied */
int hipkkt_kkt_system_init(hipkkt_kkt_t h, const double *q, const double *b);
/* kkt_update! (kktsystem.jl:62-78): cone scaling from (s, z), refactor, constant-RHS solve */
int hipkkt_kkt_system_update(hipkkt_kkt_t h, const double *d_s, const double *d_z);
/* _kkt_solve_constant_rhs! (kktsystem.jl:80-92) alone, after hipkkt_kkt_update_cones */
int hipkkt_kkt_system_solve_constant_rhs(hipkkt_kkt_t h);
/* kkt_solve_initial_point! (kktsystem.jl:95-143): LP / QP branch on nnz(P) */
int hipkkt_kkt_system_solve_initial_point(hipkkt_kkt_t h, double *d_x, double *d_s, double *d_z);
/* kkt_solve! (kktsystem.jl:145-215): lhs <- step for right-hand side rhs at the iterate
 * `variables`; steptype 0 = :affine, 1 = :combined.  lhs_tau_kappa (host, 2) receives (dtau, dkappa). */
int hipkkt_kkt_system_solve(hipkkt_kkt_t h, double *d_lhs_x, double *d_lhs_s, double *d_lhs_z,
                            double *lhs_tau_kappa,
                            const double *d_rhs_x, const double *d_rhs_s, const double *d_rhs_z,
                            double rhs_tau, double rhs_kappa,
                            const double *d_var_x, const double *d_var_s, const double *d_var_z,
                            double var_tau, double var_kappa, int steptype);

/* kkt_update! followed by the affine kkt_solve! in ONE call (kktsystem.jl:62-92 and :145-215 with steptype :affine).
 * The constant right-hand side (-q, b) of kkt_update! and the affine right-hand side (rhs.x, s - rhs.z) do not depend on
 * each other, so their two solves share every triangular sweep (one 2-column solve with per-column refinement).  Same
 * results as hipkkt_kkt_system_update(h, d_var_s, d_var_z) followed by hipkkt_kkt_system_solve(..., steptype 0); the
 * affine step does not read rhs.s (:157-158). */
int hipkkt_kkt_system_update_and_solve_affine(hipkkt_kkt_t h, double *d_lhs_x, double *d_lhs_s, double *d_lhs_z,
                                              double *lhs_tau_kappa, const double *d_rhs_x, const double *d_rhs_z,
                                              double rhs_tau, double rhs_kappa,
                                              const double *d_var_x, const double *d_var_s, const double *d_var_z,
                                              double var_tau, double var_kappa);

/* The cone operations an interior-point loop performs BETWEEN its kkt_solve! calls (solver.jl:258-351), on the caller's
 * DEVICE vectors, so that an iterate kept in HBM never leaves it: per call only scalars cross the bus.  All vectors are
 * device pointers of length m on the handle's device; all work goes on the handle's stream (in lazy mode simply behind
 * the pending update).  They need hipkkt_kkt_system_init and -- except hipkkt_kkt_system_shift_to_interior -- the cone
 * scaling of a hipkkt_kkt_system_update* call.  Inputs are never modified (the reference uses step.z / step.s as work
 * space; these do not); d_out must not alias an input.  Symmetric cones only (zero, nonnegative, second-order, PSD side
 * <= 48, or <= 96 after hipkkt_kkt_enable_large_psd): on a handle that holds an exponential, power or generalized
 * power cone, or a larger PSD cone, and on a
 * deferred-status handle, every one of them returns HIPKKT_ERR_ARG (see hipkkt_last_error) and enqueues nothing.
 * Results are reproducible bit for bit: every reduction has a fixed layout and there are no floating-point atomics. */
/* affine_ds! over all cones (coneops_compositecone.jl:153-165; nncone :117-126, socone :219-228 via circ_op! :376-392,
 * psdtrianglecone :189-205, zero cone: 0): out = lambda o lambda */
int hipkkt_kkt_system_affine_ds(hipkkt_kkt_t h, double *d_out);

/* d.s of variables_combined_step_rhs! (variables.jl:124-162) in one pass:
 *   out = lambda o lambda + m_corr * (W^{-T} step_s) o (W step_z) - sigma_mu * e
 * (_combined_ds_shift_symmetric!, coneops_symmetric_common.jl:1-35; mul_W!/mul_Winv!: nncone :196-227, socone :313-359,
 * psdtrianglecone :298-333, :409-437; e = the cone's unit; zero cone rows: 0).  m_corr is the reference's `m`, which
 * scales step.z before the product -- the product is bilinear, so it multiplies the circ term. */
int hipkkt_kkt_system_combined_ds(hipkkt_kkt_t h, double *d_out, const double *d_step_z, const double *d_step_s,
                                  double sigma_mu, double m_corr);

/* variables_calc_step_length (variables.jl:14-43) WITHOUT the max_step_fraction factor (the caller multiplies):
 *   alpha = min(1, -tau/step_tau if step_tau < 0, -kappa/step_kappa if step_kappa < 0, every cone's alpha_z, alpha_s)
 * (composite :205-243; nncone :151-170; socone :271-285 + _step_length_soc_component :443-512, every branch;
 * psdtrianglecone :230-254 + step_length_psd_component :439-466).  Every cone's limit has the form min(alpha_max, f(cone)),
 * so the reference's sequential tightening of alpha_max is an order-free minimum and the result does not depend on the
 * order of the reduction; where nothing binds it is alpha_max itself.  Synchronises; *alpha_out is a host double. */
int hipkkt_kkt_system_step_length(hipkkt_kkt_t h, const double *d_step_z, const double *d_step_s,
                                  const double *d_z, const double *d_s, double step_tau, double step_kappa,
                                  double tau, double kappa, double *alpha_out);

/* _shift_to_cone_interior! (variables.jl:180-208): margins (composite :49-63; zero :27-39, nncone :19-39,
 * socone :13-23, psdtrianglecone :8-27), then the one or two scaled_unit_shift! calls of its three branches, in place.
 * primal = 1: a zero cone's rows are set to 0; primal = 0: they are left alone.  degree = sum of cone degrees.
 * margins_out (host, 2, may be NULL) receives (min_margin, pos_margin) as found BEFORE the shift.  Synchronises. */
int hipkkt_kkt_system_shift_to_interior(hipkkt_kkt_t h, double *d_v, int primal, double *margins_out);

/* The same operations for cone lists that hold an exponential or a power cone, and the two that only such lists need
 * (the unit start and the barrier of the dual-scaling line search), so that their iterate stays in HBM too.  They are
 * entry points of their own: the four above keep refusing such handles.  Covered: zero, nonnegative, second-order, PSD
 * (side <= 48, or <= 96 after hipkkt_kkt_enable_large_psd), exponential and power cones in any order.  Same rules as above: they need hipkkt_kkt_system_init and --
 * except hipkkt_kkt_system_unit_initialization -- the cone scaling of a hipkkt_kkt_system_update* call; on a handle that
 * holds a generalized power cone or a PSD cone of side > 48 (> 96 once enabled), and on a deferred-status handle, each returns
 * HIPKKT_ERR_ARG and enqueues nothing.  Inputs are never modified, outputs must not alias inputs, all work goes on the
 * handle's stream, results are reproducible bit for bit (fixed reduction layout, no floating-point atomics).  On the
 * rows of the symmetric cones each gives, bit for bit, what its counterpart above gives on a handle with those cones
 * alone (the same kernels run); the exponential / power rows take one lane per cone. */
/* variables_unit_initialization! (variables.jl:213-226; the asymmetric start of solver.jl:383-404): every cone's
 * unit_initialization! into s and z -- zero: 0; nonnegative: 1; second-order: e_1; PSD: svec(I); exponential
 * (coneops_expcone.jl:36-52): (-1.051383945322714, 0.556409619469370, 1.258967884768947); power
 * (coneops_powcone.jl:36-54): (sqrt(1 + alpha), sqrt(1 + (1 - alpha)), 0).  One launch, no synchronisation; d_s != d_z. */
int hipkkt_kkt_system_unit_initialization(hipkkt_kkt_t h, double *d_s, double *d_z);

/* affine_ds! over all cones (coneops_compositecone.jl:153-165): lambda o lambda on the symmetric rows as
 * hipkkt_kkt_system_affine_ds, a copy of s on the exponential / power rows (coneops_expcone.jl:117-127,
 * coneops_powcone.jl:120-130). */
int hipkkt_kkt_system_affine_ds_ns(hipkkt_kkt_t h, double *d_out, const double *d_s);

/* The whole d.s of variables_combined_step_rhs! (variables.jl:124-162).  Symmetric rows: as
 * hipkkt_kkt_system_combined_ds.  Exponential / power rows (combined_ds_shift!: coneops_expcone.jl:130-147,
 * coneops_powcone.jl:132-149):
 *   out = s + sigma_mu * grad f*(z) - eta(step_s, m_corr * step_z)
 * with grad f*(z) as the scaling stored it and eta what higher_correction! returns, +1/2 D^3 f*(z)[H*^{-1} step_s, m_corr
 * step_z] (the negative of the method's third-order correction, which this subtraction restores; coneops_expcone.jl:319-366, coneops_powcone.jl:329-404; the 3 x 3 Cholesky factor and
 * solve of H*(z) as mathutils.jl:427-466; eta = 0 where that factorisation fails).  d_z MUST be the z the current
 * scaling was computed from (the z of the last hipkkt_kkt_system_update*): the stored gradient and Hessian belong to
 * it, and the correction's closed form reads z itself. */
int hipkkt_kkt_system_combined_ds_ns(hipkkt_kkt_t h, double *d_out, const double *d_step_z, const double *d_step_s,
                                     const double *d_s, const double *d_z, double sigma_mu, double m_corr);

/* step_length of the composite cone for lists that hold an exponential or power cone (coneops_compositecone.jl:205-243),
 * WITHOUT the max_step_fraction factor:
 *   1. a = min(1, tau limit, kappa limit, every symmetric cone's limit), as hipkkt_kkt_system_step_length;
 *   2. a0 = min(a, 1 - sqrt(eps));
 *   3. every exponential / power cone's backtrack_search (coneops_nonsymmetric_common.jl:5-34) on z with
 *      is_dual_feasible and on s with is_primal_feasible: alpha <- alpha * backtrack_step until the point is in the
 *      cone, 0 once alpha < alpha_min.
 * The reference tightens alpha cone after cone; here every cone backtracks independently from the common start a0 and
 * the results are folded by a minimum.  The values any search visits are a0 * backtrack_step^j formed by repeated
 * multiplication -- the same doubles whichever cone's search a value is reached in -- and the feasible set along a ray
 * out of an interior point of a convex cone is an interval [0, t), so a cone accepts a visited value exactly if it
 * accepts every smaller one: the sequential result is the largest visited value every cone accepts, which is the
 * minimum of the independent results (0 included: a search that gives up makes both 0).
 * Stage 2 is applied whether or not the list holds such a cone -- which is the composite's rule only for lists that do:
 * this entry point is FOR those lists; use hipkkt_kkt_system_step_length for symmetric ones.
 * The start a0 is read by the lane-per-cone kernel from the device record the symmetric stage left: one synchronisation
 * per call.  The call ends on any input: backtrack_step outside (0, 1) or alpha_min <= 0 (or NaN) is HIPKKT_ERR_ARG; the
 * search has a hard trip cap of floor(log(alpha_min) / log(backtrack_step)) + 2 after which it gives 0; a NaN point is
 * not in the cone.  *alpha_out is a host double. */
int hipkkt_kkt_system_step_length_ns(hipkkt_kkt_t h, const double *d_step_z, const double *d_step_s,
                                     const double *d_z, const double *d_s, double step_tau, double step_kappa,
                                     double tau, double kappa, double backtrack_step, double alpha_min,
                                     double *alpha_out);

/* The cone part of variables_barrier (variables.jl:46-72) at (z + alpha step_z, s + alpha step_s):
 *   out[0] = sum over the cones of compute_barrier -- zero: 0; nonnegative: coneops_nncone.jl:172-189; second-order:
 *            coneops_socone.jl:287-305; PSD: coneops_psdtrianglecone.jl:256-295 (log-determinants by Cholesky in LDS, one
 *            workgroup per cone); exponential / power: barrier_dual + barrier_primal
 *            (coneops_expcone.jl:189-251, coneops_powcone.jl:193-254);
 *   out[1] = <z + alpha step_z, s + alpha step_s> over all rows.
 * The caller forms mu_a and the tau / kappa terms from out[1].  A point outside a cone gives +inf or NaN in out[0]: a
 * result, not an error (HIPKKT_OK).  Synchronises: one read-back per call.  out: host, 2 doubles. */
int hipkkt_kkt_system_barrier(hipkkt_kkt_t h, const double *d_z, const double *d_s, const double *d_step_z,
                              const double *d_step_s, double alpha, double out[2]);

/* The same five operations for cone lists that hold a generalized power cone as well (coneops_genpowcone.jl), so that
 * the iterate of such a problem stays in HBM too.  Entry points of their own: the nine above keep refusing what they
 * refuse.  Covered: zero, nonnegative, second-order, PSD (side <= 48, or <= 96 after hipkkt_kkt_enable_large_psd),
 * exponential, power and generalized power cones in
 * any order.  Same rules as the _ns block: they need hipkkt_kkt_system_init and -- except the unit start -- the cone
 * scaling of a hipkkt_kkt_system_update* call; on a deferred-status handle or one with a PSD cone of side > 48 (> 96
 * once enabled) each
 * returns HIPKKT_ERR_ARG with nothing enqueued and nothing written.  Inputs are never modified, outputs must not alias
 * inputs, all work goes on the handle's stream.  On every row that is not a generalized power cone's each call gives,
 * bit for bit, what its _ns counterpart gives on a handle with those cones alone: the same kernels are launched first,
 * and on a handle without a generalized power cone the five calls ARE the _ns calls.  A generalized power cone of up to
 * 512 rows is taken by one wave (four cones to a workgroup), a larger one by a workgroup of 256; every reduction has a
 * fixed order (a lane its strided rows ascending, a butterfly over the lanes, the waves left to right) and there is no
 * floating-point atomic, so two runs give the same bits. */
/* unit_initialization! with the generalized power cones' start (coneops_genpowcone.jl:34-53): s_i = z_i =
 * sqrt(1 + alpha_i) on the first dim1 rows of such a cone and 0 on the dim2 rows behind them; every other cone as
 * hipkkt_kkt_system_unit_initialization.  Needs no cone scaling.  Two launches on the handle's stream, no
 * synchronisation; d_s and d_z are outputs and must not alias each other. */
int hipkkt_kkt_system_unit_initialization_gp(hipkkt_kkt_t h, double *d_s, double *d_z);

/* affine_ds! over all cones: as hipkkt_kkt_system_affine_ds_ns, and a copy of s on the rows of a generalized power cone
 * (coneops_genpowcone.jl:137-147).  d_out must not alias d_s; d_s is not modified; no synchronisation -- the result is
 * ordered on the handle's stream like every other launch of the call's kernels. */
int hipkkt_kkt_system_affine_ds_gp(hipkkt_kkt_t h, double *d_out, const double *d_s);

/* The whole d.s of the combined step: as hipkkt_kkt_system_combined_ds_ns, and on the rows of a generalized power cone
 * (combined_ds_shift!, coneops_genpowcone.jl:149-168)
 *   out_i = s_i + sigma_mu * grad_i
 * with grad = grad f*(z) as the scaling kernel stored it (what hipkkt_kkt_get_genpow returns).  There is no higher-order
 * correction for this cone (the reference has it commented out): d_step_z, d_step_s and m_corr are read on the other
 * cones' rows only.  d_z must be the z of the last hipkkt_kkt_system_update*.  d_out must not alias an input; no
 * synchronisation. */
int hipkkt_kkt_system_combined_ds_gp(hipkkt_kkt_t h, double *d_out, const double *d_step_z, const double *d_step_s,
                                     const double *d_s, const double *d_z, double sigma_mu, double m_corr);

/* step_length of the composite cone, WITHOUT max_step_fraction: stages 1 and 2 as hipkkt_kkt_system_step_length_ns
 * (a = min(1, tau limit, kappa limit, symmetric limits); a0 = min(a, 1 - sqrt(eps))); stage 3 folds the minimum over every
 * exponential, power AND generalized power cone's independent backtrack_search from a0 (coneops_genpowcone.jl:186-207):
 * on z with is_dual_feasible (:272-292), on s with is_primal_feasible (:249-269) -- the first dim1 entries all > 0 and
 *   exp(sum_i 2 alpha_i logsafe(v_i [/ alpha_i])) - ||v[dim1:]||^2 > 0.
 * The order-free argument of the _ns call carries over: every search visits the same doubles a0 * backtrack_step^j, and
 * the feasible set along a ray is an interval.  A trip of a search is one three-value reduction over the cone's rows (sum
 * of logs, sum of squares, count of non-positive entries) that every thread of the cone's wave / workgroup receives, so
 * the loop is uniform.  backtrack_step outside (0, 1) or alpha_min <= 0 (or NaN) is HIPKKT_ERR_ARG; the trip cap is
 * floor(log(alpha_min) / log(backtrack_step)) + 2, after which the search gives 0; a NaN point is not in the cone.
 * Inputs are not modified (nothing to alias: the result is the host double *alpha_out).  Synchronises once. */
int hipkkt_kkt_system_step_length_gp(hipkkt_kkt_t h, const double *d_step_z, const double *d_step_s,
                                     const double *d_z, const double *d_s, double step_tau, double step_kappa,
                                     double tau, double kappa, double backtrack_step, double alpha_min,
                                     double *alpha_out);

/* The cone part of variables_barrier at (z', s') = (z + alpha step_z, s + alpha step_s): as hipkkt_kkt_system_barrier,
 * with every generalized power cone's compute_barrier (coneops_genpowcone.jl:209-234) added to out[0]:
 *   barrier_dual(z') (:313-333) = -logsafe(exp(sum 2 alpha_i logsafe(z'_i / alpha_i)) - ||z'[dim1:]||^2)
 *                                 - sum (1 - alpha_i) logsafe(z'_i)
 *   barrier_primal(s') = -barrier_dual(-g(s')) - (dim1 + 1), g = gradient_primal! (:393-426): for ||s'[dim1:]|| > eps
 *   the root of the one-dimensional equation by _newton_raphson_genpowcone (:437-472, psi = 1 / (alpha . alpha)) --
 *   the start is halved at most 64 times while f0 > 0 fails (the guard ipm._newton_raphson_genpowcone has; the reference
 *   has it for the 3-row power cone only), then at most 100 one-sided Newton steps with the three stop tests of
 *   coneops_nonsymmetric_common.jl:170-193; otherwise the closed form g_i = -(1 + alpha_i) / s'_i, g[dim1:] = 0.
 * A Newton trip reduces f0 and f1 in one pass; a NaN leaves every loop.  out[1] = <z', s'> over all rows.  A point
 * outside a cone gives +inf or NaN in out[0] and HIPKKT_OK.  Inputs are not modified (nothing to alias: out is a host
 * array of 2 doubles).  Synchronises once. */
int hipkkt_kkt_system_barrier_gp(hipkkt_kkt_t h, const double *d_z, const double *d_s, const double *d_step_z,
                                 const double *d_step_s, double alpha, double out[2]);

/* The first step of every iteration on an iterate kept in HBM: residuals_update! (residuals.jl:1-37) and the scalars
 * info_update! reads (the four dot products and the eight norm_scaled calls of info.jl:33-51), from the P, A the handle
 * holds inside K and the q, b of hipkkt_kkt_system_init -- the caller needs no copy of the matrices and no sparse mat-vec
 * of its own, and after hipkkt_kkt_update_P / _update_A the residuals are those of the new values (also in lazy mode
 * with an update pending: the call simply queues on the handle's stream).  One pass over rows 0 .. n+m-1 of K:
 *   Px = Symmetric(P) x     rx_inf = -A'z              rz_inf = A x + s
 *   rx = rx_inf - Px - q tau                           rz = rz_inf - b tau
 * d_x, d_rx, d_rx_inf, d_Px, d_d, d_dinv: device, length n; d_s, d_z, d_rz, d_rz_inf, d_e, d_einv: device, length m (a
 * pointer of length 0 may be NULL).  out (host, 12):
 *   q.x, b.z, s.z, x.Px, |d o x|, |e o z|, |einv o s|, |dinv o rx_inf|, |dinv o Px|, |einv o rz_inf|, |einv o rz|, |dinv o rx|
 * (2-norms; x.Px and |.. rx| use the Px and rx that were stored).  The four equilibration vectors are ALL NULL (read as
 * ones) or all given, anything else is HIPKKT_ERR_ARG; the scalar c and 1/tau are the caller's to apply, and
 * r_tau = q.x + b.z + kappa + x.Px / tau its to form.  The norms survive the range norm_scaled survives
 * (mathutils.jl:57-80): entries of 1e200 do not give inf, entries of 1e-200 do not give 0, a zero vector gives exactly 0;
 * a non-finite entry gives a non-finite scalar.  Needs hipkkt_kkt_system_init and nothing else -- no cone scaling, no
 * factorisation -- and works with every cone kind (the residuals do not depend on the cones; nothing behind a row's A
 * entries is read).  The five outputs must not alias an input or each other (HIPKKT_ERR_ARG where the pointers are equal).
 * A deferred-status handle is refused with HIPKKT_ERR_ARG, nothing enqueued, nothing written.  Synchronises: one
 * read-back per call.  Reproducible bit for bit (fixed reduction layout, no floating-point atomics). */
int hipkkt_kkt_system_residuals(hipkkt_kkt_t h, const double *d_x, const double *d_s, const double *d_z, double tau,
                                double *d_rx, double *d_rz, double *d_rx_inf, double *d_rz_inf, double *d_Px,
                                const double *d_d, const double *d_dinv, const double *d_e, const double *d_einv,
                                double out[12]);

/* The x and z parts of variables_combined_step_rhs! (variables.jl:124-162): rhs_x = (1 - sigma) rx (n),
 * rhs_z = (1 - sigma) rz (m); the s part is hipkkt_kkt_system_combined_ds.  One launch on the handle's stream, no
 * synchronisation.  Outputs may alias inputs.  A pointer to a vector of length 0 (n = 0 or m = 0) may be NULL, any other
 * NULL is HIPKKT_ERR_ARG.  Needs hipkkt_kkt_system_init; refused on a deferred-status handle (HIPKKT_ERR_ARG, nothing
 * enqueued). */
int hipkkt_kkt_system_combined_rhs(hipkkt_kkt_t h, double *d_rhs_x, double *d_rhs_z, const double *d_rx,
                                   const double *d_rz, double sigma);

/* variables_add_step! (variables.jl:107-122) for the vector part: x += alpha dx (n), s += alpha ds, z += alpha dz (m),
 * each element fl(v + fl(alpha d)), as one launch on the handle's stream, no synchronisation (tau and kappa are the
 * caller's scalars).  A step must not alias the vector it is added to, and d_s must not be d_z (HIPKKT_ERR_ARG where the
 * pointers are equal).  A pointer to a vector of length 0 may be NULL, any other NULL is HIPKKT_ERR_ARG.  Needs
 * hipkkt_kkt_system_init; refused on a deferred-status handle (HIPKKT_ERR_ARG, nothing enqueued). */
int hipkkt_kkt_system_add_step(hipkkt_kkt_t h, double *d_x, double *d_s, double *d_z, const double *d_dx,
                               const double *d_ds, const double *d_dz, double alpha);

/* ------------------------------------------- Level C: data updating (parametric re-solves)
 * update_data! / update_P! / update_A! / update_q! / update_b! (/root/reference/src/data_updating.jl:26-247): new problem
 * data on a handle that keeps its ordering, schedule, sweep plans and allocations.  The reference scales new data by the
 * equilibration it computed once (data_updating.jl:63-65, 93-95, 116-118, 140-141); so does the handle, which holds
 * that equilibration on the device. */

/* The frozen equilibration of data_equilibrate! (problemdata.jl:133-221) on the handle: d (n) and e (m) are HOST vectors,
 * copied to the device once together with dinv = 1 / d and einv = 1 / e (IEEE quotients), c is the cost scaling.
 * d = e = NULL clears the scalings to all ones with c = 1 -- the state of a handle that never called this.  c <= 0, a
 * non-finite c, or exactly one of the two pointers NULL where its length is > 0: HIPKKT_ERR_ARG.  The first call (or the
 * first data update, whichever comes first) also builds, once, the row and column of every stored entry of P and A from
 * K's pattern and the assembly's maps, and the staging of an indexed update's positions.  P, A, q and b on the handle are
 * NOT touched: the caller created the handle from data that is already scaled.  Synchronises (the host arrays may be
 * reused when it returns). */
int hipkkt_kkt_system_set_equilibration(hipkkt_kkt_t h, const double *d, const double *e, double c);

/* The handle's device copies of d, dinv (n) and e, einv (m) -- data.equilibration of the reference, which update_P! and
 * its siblings read (data_updating.jl:63-64, 93-94, 116, 140) -- for hipkkt_kkt_system_residuals (info_update! with
 * equilibration, info.jl:19-51); valid until the next hipkkt_kkt_system_set_equilibration or destroy.  All ones on a
 * handle whose scalings were never set or were cleared.  Enqueues nothing. */
int hipkkt_kkt_system_equilibration_dev(hipkkt_kkt_t h, const double **d_d, const double **d_dinv,
                                        const double **d_e, const double **d_einv);

/* update_P! / update_A! / update_q! / update_b! (data_updating.jl:56-147).  d_values: k UNSCALED user values on the
 * DEVICE; index: a HOST array of k zero-based positions -- into the stored upper-triangular nzval of P, the nzval of A,
 * or the vector q / b -- or NULL for the vector form (_update_matrix :181-194, _update_vector :216-231), where k must
 * equal nnz(triu P), nnz(A), n or m.  k = 0 is a no-op that returns HIPKKT_OK (:61, :189, :223).  An index out of range
 * or a REPEATED index is HIPKKT_ERR_ARG with the offending place in index[] named by hipkkt_last_error, the handle
 * untouched (the reference's tuple form, :196-213 and :234-247, applies repeats in order; a parallel scatter cannot).
 * The checks are host-only code (csrc/data_update.cpp).
 *   P: fl(fl(v * fl(d[row] * d[col])) * c)      A: fl(v * fl(e[row] * d[col]))
 *   q: fl(fl(v * d[i]) * c)                     b: fl(v * e[i])
 * without contraction -- what lrscale! followed by the product by c computes (:191-193), and the SAME order in the
 * (index, value) form, so that an indexed update of every entry equals the vector update bit for bit.  The reference's
 * tuple form multiplies in another order, (lscale * rscale * cscale) * value (:208-210), and can differ from its own
 * vector form, and from this, in the last bit.
 * P and A: the scaled value goes to the handle's copy of the matrix, to K, and -- when the residual's image of K is
 * current -- through to its one or two slots there, as a cone update's values do; a dirty image is left alone (it is
 * gathered whole before its next use) and the call never makes a current image dirty: a two-entry update costs two
 * entries.  q writes q and -q, b writes b.
 * Afterwards the factorisation is stale (P, A) and so are (x2, z2) and the cached constant terms of kkt_solve! (all four):
 * the next hipkkt_kkt_system_update / _update_cones / _update_scaling refactors, the next constant-RHS solve (eager, or
 * the lazy mode's paired one) renews (x2, z2).  Until then hipkkt_kkt_system_solve, _solve_batch and _solve_host
 * (stale (x2, z2)), and _solve_constant_rhs and _solve_initial_point (stale factorisation) return HIPKKT_ERR_ARG and
 * enqueue nothing.  hipkkt_kkt_update_P / _A of level B keep their behaviour and set no such mark.
 * One launch per call on the handle's stream, behind the upload of index where there is one; no synchronisation beyond
 * what that upload needs, and the number of launches does not depend on k.  The q and b calls need
 * hipkkt_kkt_system_init; all four are refused on a deferred-status handle (HIPKKT_ERR_ARG).  On a handle partitioned
 * by hipkkt_kkt_system_set_problems they work unchanged with the handle's one c, until
 * hipkkt_kkt_system_set_equilibration_batch has given every member its own cost scaling: from then on the c of the P and
 * q formulas is c[b] of the member b that owns the entry's row (P: row and column lie in one member; q: row i) -- same
 * rounding order, still one launch whatever k and nb, the indexed and the vector form still bit for bit equal, the
 * write-through, the staleness marks and the refusals unchanged; _A and _b carry no c and do not change. */
int hipkkt_kkt_system_update_data_P(hipkkt_kkt_t h, const double *d_values, const int64_t *index, int64_t k);
int hipkkt_kkt_system_update_data_A(hipkkt_kkt_t h, const double *d_values, const int64_t *index, int64_t k);
int hipkkt_kkt_system_update_data_q(hipkkt_kkt_t h, const double *d_values, const int64_t *index, int64_t k);
int hipkkt_kkt_system_update_data_b(hipkkt_kkt_t h, const double *d_values, const int64_t *index, int64_t k);

/* data_get_normq! / data_get_normb! (problemdata.jl:91-109): out[0] = max |q_i dinv_i| / c and out[1] = max |b_i einv_i|
 * from the handle's scaled q and b -- the norms of the user's unscaled vectors that info_update! compares the residuals
 * with.  One launch and one read-back (synchronises).  A maximum does not depend on the order it is taken in, so the
 * result is exact; a non-finite entry gives a non-finite result, empty vectors give 0.  Needs hipkkt_kkt_system_init;
 * refused on a deferred-status handle. */
int hipkkt_kkt_system_data_norms(hipkkt_kkt_t h, double out[2]);

/* ------------------------------------------- Level C on a stack of INDEPENDENT problems
 * A batch of independent conic problems is put on ONE handle as a block-diagonal stack (P = blkdiag(P_b), A = blkdiag(A_b),
 * the cone lists one behind the other), so that the elimination forest shares every per-level launch.  The calls below
 * make such a stack solvable as the problems it consists of: every scalar the loop keeps between its solves -- tau,
 * kappa, mu, sigma, alpha, the residual norms, the margins, (dtau, dkappa) -- exists once per member.  Each _batch entry
 * point is its scalar twin with every scalar argument a HOST array of nb doubles and every scalar result a host array
 * with member b's values contiguous; vector arguments stay whole-stack device pointers.  Per call the scalar arrays go
 * up in one copy and the results come back in one copy, and the number of kernel launches does not depend on nb: the
 * reductions are segmented by member on the device (a workgroup belongs to one member; member b's wave folds b's slots
 * in slot order -- fixed layout, no floating-point atomic, two calls give the same bits).
 * What stays JOINT on a partitioned handle unless the handle opts out: the static regulariser's epsilon, scaled by the
 * largest diagonal entry of the whole K (kktsolver_directldl.jl:297-310), and the attribution of a failed
 * hipkkt_kkt_system_update (a failed kkt_update!, kktsystem.jl:62-78, names no member) -- both per member once
 * hipkkt_kkt_system_set_member_status (below) has been enabled; and the iterative refinement's stopping rule, whose
 * infinity-norms run over the stack (kktsolver_directldl.jl:389-470) -- per member once
 * hipkkt_kkt_system_set_member_refinement (below) has been enabled.  JOINT whatever is enabled: the RETURN VALUE of
 * hipkkt_kkt_system_update and of the solves, the status of the call (HIPKKT_NUMERIC_FAILURE if any member failed: which
 * member is read from hipkkt_kkt_system_member_status and hipkkt_kkt_system_member_refinement_info); the LP / QP branch of
 * the symmetric start, decided by nnz(P) of the stack; and the count of dynamic regularisations.
 * hipkkt_kkt_system_update,
 * _solve_constant_rhs, _solve_initial_point and _affine_ds have no scalar argument and serve a partitioned handle as
 * they are: the block-diagonal K does their work per member.  No scalar entry point changes its behaviour on a
 * partitioned handle. */
/* The partition: member b owns rows x_off[b] .. x_off[b+1]-1 of every x-like vector and z_off[b] .. z_off[b+1]-1 of every
 * s/z-like vector (DefaultProblemData's P, q, A, b of problemdata.jl:3-88 cut member by member; the cones of
 * compositecone_type.jl:114-141 likewise).  x_off, z_off: HOST arrays of nb + 1 entries, copied.  Callable after
 * hipkkt_kkt_system_init, again to replace the partition, and with nb = 0 (offsets ignored) to clear it.  HIPKKT_ERR_ARG,
 * with a text in hipkkt_last_error that names the offending member or entry and the handle's partition left as it was,
 * unless: the offsets start at 0, do not decrease and end at n and m; every member has at least one x row (a member
 * without z rows is allowed); every cone lies inside one member's z range; every stored entry of P has its row and its
 * column in the same member; every entry of A has its row's member equal to its column's.  Symmetric cones with PSD side
 * <= 48 only: a handle that holds an exponential, power or generalized power cone or a PSD cone of side > 48, or that
 * has called hipkkt_kkt_enable_large_psd, is refused with HIPKKT_ERR_ARG, and so is a deferred-status handle.  The
 * tables (row -> member, cone -> member, workgroup -> (member, chunk)) and all work space are sized by nb; nb is bounded
 * by n only.  Synchronises with the handle's stream once (tables in use are replaced); enqueues no kernel.  A handle that
 * holds member cost scalings (hipkkt_kkt_system_set_equilibration_batch, below) refuses to replace or clear its partition
 * (HIPKKT_ERR_ARG, nothing changed): the caller clears them first with hipkkt_kkt_system_set_equilibration. */
int hipkkt_kkt_system_set_problems(hipkkt_kkt_t h, int64_t nb, const int64_t *x_off, const int64_t *z_off);

/* hipkkt_kkt_system_set_equilibration with the cost scaling given per member: data_equilibrate! (problemdata.jl:133-221)
 * computes c for ONE problem, from that problem's q and P; a stack of independent problems equilibrated as the problems
 * it consists of has one c per member, where a joint c would be the cost scaling of the member with the largest q.
 * d (n) and e (m): HOST vectors, handled exactly as in the scalar call (copied once, dinv = 1 / d and einv = 1 / e as
 * IEEE quotients, both NULL: all ones; the same tables built on first use); c: a HOST array of nb cost scalings.  Needs a
 * partition (HIPKKT_ERR_ARG without one).  c[b] must be finite and > 0, else HIPKKT_ERR_ARG with member b named by
 * hipkkt_last_error and the handle untouched.  The handle keeps the c[b] and nothing derived from them; the scalar c that
 * hipkkt_kkt_system_set_equilibration stored is left alone, so no scalar call except the two data updates that carry c
 * (hipkkt_kkt_system_update_data_P / _q, above) and hipkkt_kkt_system_data_norms_batch can observe this mode.  The scalar
 * hipkkt_kkt_system_set_equilibration (also with NULLs) afterwards returns the handle to one joint c.  While the handle
 * holds member cost scalings hipkkt_kkt_system_set_problems is refused, so that a partition that no longer matches them
 * cannot be reached.  P, A, q and b on the handle are NOT touched.  Refused on a deferred-status handle.  Synchronises
 * (the host arrays may be reused when it returns).  The check of c[] and the tables are host-only code
 * (csrc/data_update.cpp). */
int hipkkt_kkt_system_set_equilibration_batch(hipkkt_kkt_t h, const double *d, const double *e, const double *c);

/* hipkkt_kkt_system_data_norms per member -- data_get_normq! / data_get_normb! (problemdata.jl:91-109) on each member's
 * rows: out (HOST, 2 nb doubles) gets out[2 b] = the maximum over member b's x rows of |q_i dinv_i|, divided by c[b] (by
 * the handle's c on a handle without member cost scalings), and out[2 b + 1] = the maximum over its z rows of
 * |b_i einv_i|, 0 for a member without z rows.  Products and quotient are formed as the scalar call forms them; the
 * maxima are taken with an integer atomicMax on the bit patterns of the non-negative products (no floating-point
 * atomic): exact, and the same whatever the order.  A NaN in member b's q makes out[2 b] non-finite and leaves every
 * other member's values as they are.  One launch and one read-back whatever nb (synchronises).  Needs
 * hipkkt_kkt_system_init and a partition; refused on a deferred-status handle.  With nb = 1 and c[0] equal to the
 * handle's c the two values equal the scalar call's. */
int hipkkt_kkt_system_data_norms_batch(hipkkt_kkt_t h, double *out);

/* The iterative refinement's accept / stop rule (kktsolver_directldl.jl:389-449) per member instead of over the stack.
 * enable != 0: from now on every single-column solve of this handle -- hipkkt_kkt_solve, hipkkt_kkt_solve_dev,
 * hipkkt_kkt_system_solve_constant_rhs, _solve_initial_point, _solve_batch and a scalar hipkkt_kkt_system_solve --
 * applies the reference's loop to each member separately: member b's norms are ||e_b||_inf and ||b_b||_inf over ITS rows
 * of K's image (its x rows, its z rows and the expansion rows behind n + m of its sparse second-order cones), its
 * tolerance is abstol + reltol ||b_b||_inf, and it has its own ratio test, accept decision, round count and bad flag.
 * Sweeps and residual passes still run once per round over the whole stack, as long as any member is active; a member
 * that has left its loop is not written again (x keeps its accepted solution, and its rows of the residual are zero for
 * the following sweeps, so that its rows of every later candidate equal x).  A non-finite norm marks that member alone
 * as bad; the other members finish their loops, then the solve returns HIPKKT_NUMERIC_FAILURE: the status stays joint.
 * The protocol with the host is the joint rule's on the aggregate over the members (active: any member; rounds, as
 * hipkkt_kkt_last_ir_iterations and hipkkt_info report them and hipkkt_kkt_speculative_rounds enqueues them ahead: the
 * most any member took; bad: any member).  With nb = 1 a solve is bit for bit the joint rule's.  While enabled the lazy
 * 2-column pairing of hipkkt_kkt_system_solve is not taken -- a pending constant-RHS solve runs by itself first, as
 * hipkkt_kkt_system_solve_batch does it --, and hipkkt_kkt_solve_multi(_dev) with two or more columns keeps its joint
 * rule per column.  The deferred-status mode never meets this path: hipkkt_kkt_system_set_problems refuses a
 * deferred-status handle.  enable == 0 switches back to the joint rule; so does replacing or clearing the partition.
 * HIPKKT_ERR_ARG on a handle without a partition, and for 2^20 members or more (the aggregate counts the members in
 * 21-bit fields of one word).  Two launches per round (residual, rule) whatever nb, no
 * floating-point atomic; tables, slots and state are sized by nb and iterative_refinement_max_iter and allocated HERE,
 * not in a solve.  Synchronises with the handle's stream (tables in use are replaced). */
int hipkkt_kkt_system_set_member_refinement(hipkkt_kkt_t h, int enable);

/* What the last solve under the member rule did (kktsolver_directldl.jl:389-449, per member): out (host, 4 nb) receives
 * for member b at out[4 b ..] {its refinement rounds, ||e_b||_inf of its accepted solution, ||b_b||_inf, 1 if a norm of
 * its was not finite else 0}.  HIPKKT_ERR_ARG if member refinement is not enabled or no solve has run under it since it
 * was enabled.  Synchronises: one read-back of 4 nb doubles, no kernel. */
int hipkkt_kkt_system_member_refinement_info(hipkkt_kkt_t h, double *out);

/* The static regulariser and the failure words of a refactorisation per member instead of over the stack
 * (kktsolver_directldl.jl:259-310, kktsystem.jl:62-78, directldl_qdldl.jl:72-81 on each member's rows and columns).
 * enable != 0: from now on every refactorisation of this handle -- hipkkt_kkt_system_update, _update_cones,
 * _update_scaling, _update_host, _update_and_solve_affine and the level-B updates -- takes
 * eps_b = static_regularization_constant + static_regularization_proportional * max |K_ii| with i over member b's rows
 * of K's image (its x rows, its z rows and the expansion rows behind n + m of its sparse second-order cones), and member
 * b's pivots receive eps_b * sign; K itself stays un-regularised.  With static_regularization_enable = 0 nothing is
 * added and eps_b = 0.  hipkkt_kkt_last_regularizer reports the largest eps_b.  Beside the handle's words, the scaling
 * of a cone that fails marks its member, and one pass behind the factorisation marks the member of every column whose
 * pivot's reciprocal is not finite (K is block diagonal: a member's columns form their own subtrees, a non-finite value
 * never leaves its block).  The return value of the update stays the joint one, HIPKKT_NUMERIC_FAILURE if any member
 * failed.  Three launches more per update whatever nb (the segmented maximum, eps per member and per column, the pivot
 * pass; the members' words are zeroed by the launch that zeroes the handle's), the maxima by integer atomicMax on bit
 * patterns: no floating-point atomic, exact.  While enabled the lazy mode's enqueue-only update is not taken: an update
 * is read back at once, so that a failure can be answered member by member before the next solve.  While this mode AND
 * member refinement are enabled, a hipkkt_kkt_system_solve_batch whose solve fails because members were marked bad still
 * recovers the step of every member (the member rule has finished the others' rows) before it returns
 * HIPKKT_NUMERIC_FAILURE; otherwise a failed solve returns at once, as before.  With nb = 1 an
 * update and every solve behind it are bit for bit those of the same handle with the mode off.  enable == 0 switches
 * back; so does replacing or clearing the partition.  HIPKKT_ERR_ARG on a handle without a partition.  Tables (row ->
 * member, column of the factor -> member) and work space are sized by nb and N and allocated HERE, not in an update.
 * Synchronises with the handle's stream (tables in use are replaced); enqueues no kernel. */
int hipkkt_kkt_system_set_member_status(hipkkt_kkt_t h, int enable);

/* What the last refactorisation under hipkkt_kkt_system_set_member_status found (kktsolver_directldl.jl:259-310,
 * directldl_qdldl.jl:72-81, per member): out (host, 3 nb) receives for member b at out[3 b ..] {1 if the scaling of one
 * of its cones failed else 0, 1 if a pivot in its columns was not finite else 0, eps_b}.  The OR over the members of
 * either word is the handle's joint word.  HIPKKT_ERR_ARG if the mode is not enabled or no update has run since it was
 * enabled.  Synchronises: one read-back of 2 nb doubles, no kernel. */
int hipkkt_kkt_system_member_status(hipkkt_kkt_t h, double *out);

/* Rules for the seven _batch calls: on a handle without a partition, on a deferred-status handle and with a NULL scalar
 * array each returns HIPKKT_ERR_ARG and enqueues nothing; the aliasing rules are the twin's. */
/* hipkkt_kkt_system_residuals per member (residuals.jl:1-37, info.jl:33-51): rx and rz are formed with the row's own
 * tau[b]; out (host, 12 nb) receives for member b at out[12 b ..] the twelve scalars of the twin over THAT member's rows
 * only.  The five vectors are, bit for bit, what the twin writes on member b's rows when called with tau[b].  The
 * equilibration vectors are all NULL or all given; the outputs alias neither an input nor each other.  Synchronises: one
 * upload (tau), one read-back. */
int hipkkt_kkt_system_residuals_batch(hipkkt_kkt_t h, const double *d_x, const double *d_s, const double *d_z,
                                      const double *tau, double *d_rx, double *d_rz, double *d_rx_inf, double *d_rz_inf,
                                      double *d_Px, const double *d_d, const double *d_dinv, const double *d_e,
                                      const double *d_einv, double *out);

/* kkt_solve! per member (kktsystem.jl:145-215), steptype 0 = :affine, 1 = :combined: ONE solve of the stacked system
 * for (x1, z1) (:150-173, as hipkkt_kkt_system_solve), then per member, from that member's rows of q, b, x, x1, x2, z1,
 * z2: every dot product of :185-196, P x1 and P (x / tau_b - x2), dtau_b, (dx, dz) = (x1, z1) + dtau_b (x2, z2)
 * (:200-203) and dkappa_b (:206); ds = -(Hs dz + const) (:206-212) is per cone anyway.  rhs_tau, rhs_kappa, var_tau,
 * var_kappa: host arrays of nb; lhs_tau_kappa (host, 2 nb) receives (dtau_b, dkappa_b) at [2 b], [2 b + 1].  The x2-only
 * terms of tau_den are formed per member by this call itself.  On a lazy handle (hipkkt_kkt_system_set_lazy) with the
 * constant-RHS solve pending, that solve runs by itself first, as for a :combined hipkkt_kkt_system_solve arriving
 * first; there is no 2-column pairing for batches.  The return value is the joint status of the solve.  Inputs are not
 * modified; the lhs vectors must not alias an input.  Synchronises: one upload, one read-back (besides the solve's own
 * refinement read-backs, as in the twin). */
int hipkkt_kkt_system_solve_batch(hipkkt_kkt_t h, double *d_lhs_x, double *d_lhs_s, double *d_lhs_z, double *lhs_tau_kappa,
                                  const double *d_rhs_x, const double *d_rhs_s, const double *d_rhs_z,
                                  const double *rhs_tau, const double *rhs_kappa,
                                  const double *d_var_x, const double *d_var_s, const double *d_var_z,
                                  const double *var_tau, const double *var_kappa, int steptype);

/* hipkkt_kkt_system_combined_ds per member (variables.jl:124-162; coneops_symmetric_common.jl:1-35): on member b's
 * cones out = lambda o lambda + m_corr[b] (W^{-T} step_s) o (W step_z) - sigma_mu[b] e -- bit for bit what the twin
 * writes there with member b's scalars (the same per-cone code runs).  d_out must not alias an input.  One upload, no
 * synchronisation. */
int hipkkt_kkt_system_combined_ds_batch(hipkkt_kkt_t h, double *d_out, const double *d_step_z, const double *d_step_s,
                                        const double *sigma_mu, const double *m_corr);

/* hipkkt_kkt_system_step_length per member (variables.jl:14-43; coneops_compositecone.jl:205-243), WITHOUT the
 * max_step_fraction factor as in the twin: alpha_out[b] = min(1, -tau[b]/step_tau[b] if step_tau[b] < 0, the same for
 * kappa, the limits of member b's cones) -- an order-free minimum, so it equals the twin's result on a handle that holds
 * member b alone.  step_tau, step_kappa, tau, kappa, alpha_out: host arrays of nb.  Inputs are not modified.
 * Synchronises: one upload, one read-back. */
int hipkkt_kkt_system_step_length_batch(hipkkt_kkt_t h, const double *d_step_z, const double *d_step_s, const double *d_z,
                                        const double *d_s, const double *step_tau, const double *step_kappa,
                                        const double *tau, const double *kappa, double *alpha_out);

/* _shift_to_cone_interior! per member (variables.jl:180-208): the margins of member b's cones, then the branch they
 * select, applied to member b's rows in place; the degree is that of the member's own cones.  margins_out (host, 2 nb,
 * may be NULL) receives (min_margin_b, pos_margin_b) as found BEFORE the shift.  The branch is chosen on the device: no
 * upload, one read-back.  Synchronises. */
int hipkkt_kkt_system_shift_to_interior_batch(hipkkt_kkt_t h, double *d_v, int primal, double *margins_out);

/* hipkkt_kkt_system_combined_rhs per member (variables.jl:124-162): rhs_x = (1 - sigma[b]) rx, rhs_z = (1 - sigma[b]) rz
 * on member b's rows, bit for bit the twin's values with sigma[b]; the s part is hipkkt_kkt_system_combined_ds_batch.
 * Outputs may alias inputs.  A pointer to a vector of length 0 may be NULL, any other NULL is HIPKKT_ERR_ARG.  One launch
 * on the handle's stream behind one upload (sigma), no synchronisation. */
int hipkkt_kkt_system_combined_rhs_batch(hipkkt_kkt_t h, double *d_rhs_x, double *d_rhs_z, const double *d_rx,
                                         const double *d_rz, const double *sigma);

/* variables_add_step! per member (variables.jl:107-122): x += alpha[b] dx, s += alpha[b] ds, z += alpha[b] dz on member
 * b's rows, each element fl(v + fl(alpha[b] d)) as in the twin; alpha[b] == 0 leaves member b's rows bit for bit as they
 * were (they are not written).  A step must not alias the vector it is added to, and d_s must not be d_z.  One upload,
 * no synchronisation. */
int hipkkt_kkt_system_add_step_batch(hipkkt_kkt_t h, double *d_x, double *d_s, double *d_z, const double *d_dx,
                                     const double *d_ds, const double *d_dz, const double *alpha);

/* Lazy constant-RHS solve: the same pairing reached through the reference's own TWO calls, so that solver.jl:278-295
 * stays as it is.  With lazy = 1, kkt_update! (hipkkt_kkt_system_update / _update_cones) scales, scatters and
 * refactors, returns the factorisation's status and only NOTES that (x2, z2) = K \ (-q, b) is due
 * (kktsystem.jl:71-77 would solve it at once); the next hipkkt_kkt_system_solve with steptype :affine sends both
 * right-hand sides through the sweeps as one 2-column solve and returns the AND of the two solves' status -- which is
 * what solver.jl:279-295 computes from the two calls (`is_kkt_solve_success = kkt_update!(...)`, then
 * `is_kkt_solve_success && kkt_solve!(..., :affine)`), so the loop's control flow is unchanged.  Any other consumer of
 * (x2, z2) -- a :combined solve arriving first, a structure that takes one right-hand side per sweep -- makes the
 * pending solve run by itself first; hipkkt_kkt_system_solve_initial_point does not read (x2, z2) and leaves it
 * pending (the next kkt_update! supersedes it: solver.jl:389-393). */
int hipkkt_kkt_system_set_lazy(hipkkt_kkt_t h, int lazy);
/* kkt_update!(kktsystem, data, cones) for a caller that keeps the reference's cone objects (the Julia glue: kkt_update!
 * gets `cones`, not the iterate): the reference's data for kktsolver_update! (as hipkkt_kkt_update_cones) plus the NT
 * scaling the step recovery of kkt_solve! reads from the same cones -- w (m: nonnegative cones sqrt(s/z), second-order
 * cones the normalised w, coneops_nncone.jl:75-86, coneops_socone.jl:75-123), eta (one per cone; second-order cones),
 * lambda (m; a PSD cone of side k keeps its k values in the first k of its slots), and R, Rinv of the PSD cones
 * (k x k column-major, concatenated in cone order; coneops_psdtrianglecone.jl:127-132).  Then the constant-RHS solve,
 * or its note in lazy mode. */
int hipkkt_kkt_system_update_cones(hipkkt_kkt_t h, const double *Hsblocks, const double *soc_u, const double *soc_v,
                                   const double *soc_eta2, const double *w, const double *eta, const double *lambda,
                                   const double *psd_R, const double *psd_Rinv);
/* The same kkt_update! from the NT scaling ALONE: the Hs blocks and the sparse second-order-cone vectors u, v, eta^2 are
 * functions of (w, eta) and of R (get_Hs!: coneops_nncone.jl:91-101, coneops_socone.jl:125-192,
 * coneops_psdtrianglecone.jl:135-161) and are formed on the device -- for the headline workload 3.2 MB cross PCIe per
 * iteration instead of 6.4, for PSD cones of side k the k x k factor R instead of the t(t+1)/2-entry block, t = k(k+1)/2.
 * The values equal get_Hs!'s to round-off (bit for bit when the scaling came from the device: the tests pin that).  In
 * lazy mode the call only enqueues, like hipkkt_kkt_system_update; the arrays may be reused when it returns. */
int hipkkt_kkt_system_update_scaling(hipkkt_kkt_t h, const double *w, const double *eta, const double *lambda,
                                     const double *psd_R, const double *psd_Rinv);
/* (w, eta, lambda, R, Rinv cannot carry the 3 x 3 block of an exponential or power cone: on a handle that holds one
 * the call above returns HIPKKT_ERR_ARG; hipkkt_kkt_system_update_cones, whose Hs blocks are the whole scaling of
 * such a cone, is the route from the caller's cone objects.) */
/* The same entry points for a caller whose iterate lives in HOST memory (DefaultVariables are Vector{T},
 * variables.jl:1-30): vectors are staged through buffers the handle owns (n + 2m doubles each way per call).
 * hipkkt_kkt_system_solve_host: var_x = var_s = var_z = NULL means "the variables of the previous call" -- they do not
 * change between the affine and the combined kkt_solve! of an iteration (solver.jl:289-323), so the glue sends them once. */
int hipkkt_kkt_system_update_host(hipkkt_kkt_t h, const double *s, const double *z);
int hipkkt_kkt_system_solve_initial_point_host(hipkkt_kkt_t h, double *x, double *s, double *z);
int hipkkt_kkt_system_solve_host(hipkkt_kkt_t h, double *lhs_x, double *lhs_s, double *lhs_z, double *lhs_tau_kappa,
                                 const double *rhs_x, const double *rhs_s, const double *rhs_z,
                                 double rhs_tau, double rhs_kappa,
                                 const double *var_x, const double *var_s, const double *var_z,
                                 double var_tau, double var_kappa, int steptype);

/* Self-test of the hand-over protocol by which kernels that run side by side pass data (persistent / chained sweep
 * kernels, the factorisation's overlap mode; contract stated in csrc/factor_kernels.hip): `pairs` producer / consumer
 * workgroup pairs on different XCDs hand `words` doubles over `rounds` times.  variant 0 = the contract; 1 = without the
 * producer's s_waitcnt before its signal; 2 = with plain instead of agent-scope payload accesses.  out[0] = payload words
 * read stale, out[1] = expired waits.  Test infrastructure (tests/test_gpu_parity.py::test_handover_litmus): variant 0
 * must give (0, 0). */
int hipkkt_selftest_handover(int variant, int pairs, int words, int rounds, int device, int64_t out[2]);

/* Page-lock a host array the caller keeps for the solver's lifetime (an interior-point method's work vectors:
 * DefaultVariables, the right-hand sides, the cones' w / lambda) so that the copies of the *_host entry points run at
 * the link's rate and without the runtime's per-call pinning (cfg2: the host-vector iteration 4.4 -> 3.9 ms).  Optional;
 * unregister before the array is freed.  Returns HIPKKT_OK, or HIPKKT_ERR_HIP if the range cannot be registered (the
 * entry points work with unregistered memory all the same). */
int hipkkt_host_register(void *ptr, int64_t bytes);
int hipkkt_host_unregister(void *ptr);

/* ------------------------------------------- problem-data scaling (before the KKT solver is built)
 * data_equilibrate! (/root/reference/src/problemdata.jl:133-221): Ruiz equilibration of
 * [P A'; A 0], q, b on the device.  P: n x n upper-triangular CSC,
 * A: m x n CSC.  Pnzval, Anzval, q, b are overwritten with c D P D, E A D, c D q, E b; d (n),
 * e (m) and c (1) receive the scalings (all ones / one when max_iter = 0).  Defaults of the
 * reference: max_iter 10, min_scaling 1e-4, max_scaling 1e4 (settings.jl:98-101).  Cones that do
 * not admit elementwise scaling (second-order, PSD) get one common factor per cone
 * (rectify_equilibration!, coneops_defaults.jl:32-44). */
int hipkkt_equilibrate(int64_t n, int64_t m,
                       const int64_t *Pcolptr, const int64_t *Prowval, double *Pnzval,
                       const int64_t *Acolptr, const int64_t *Arowval, double *Anzval,
                       double *q, double *b,
                       int64_t ncones, const int32_t *cone_kinds, const int64_t *cone_dims,
                       int32_t max_iter, double min_scaling, double max_scaling,
                       double *d, double *e, double *c, int index_base, int device);
/* _update_matrix (data_updating.jl:169-194), the re-scaling update_P! / update_A! apply to new
 * values before kktsolver_update_P!/A!: nzval <- cscale * lscale[row] * rscale[col] * nzval
 * (P: lscale = rscale = d, cscale = c; A: lscale = e, rscale = d, cscale = 1). */
int hipkkt_scale_matrix_values(int64_t nrows, int64_t ncols, const int64_t *colptr,
                               const int64_t *rowval, double *nzval, const double *lscale,
                               const double *rscale, double cscale, int index_base, int device);

/* y = W'W x over all cones with the current scaling (mul_Hs!, coneops_compositecone.jl:138-150);
 * valid after hipkkt_kkt_update_from_sz*.  Host vectors of length m. */
int hipkkt_kkt_mul_Hs(hipkkt_kkt_t h, double *y, const double *x);

/* introspection used by the parity tests: the assembled K (triu CSC, 0-based) and data maps */
int hipkkt_kkt_get_pattern(hipkkt_kkt_t h, int64_t *colptr /* N+1 */, int64_t *rowval /* nnzK */);
int hipkkt_kkt_get_values(hipkkt_kkt_t h, double *nzval /* nnzK, un-regularised */);
/* e = b - K_sym x on the current un-regularised values (the residual of _iterative_refinement,
 * kktsolver_directldl.jl:455-466), by the residual, norm and refinement-round kernels of the solves themselves, launched
 * as a solve of nrhs columns would launch them.  Test infrastructure (tests/test_gpu_residual.py): it lets the kernels be
 * compared with a high-precision residual directly, not through a refined solution.  x, b: host, N x nrhs column-major
 * (all N = n + m + p rows, in K's order -- the order of hipkkt_kkt_get_pattern); e: host, the same shape, may be NULL;
 * norm_e, norm_b: host, nrhs infinity norms each, norm_b may be NULL.  A column holding a non-finite entry has a
 * non-finite norm; that is a result, and the call still returns HIPKKT_OK.
 *   route 0 "columns"    column-major kernels with a finishing kernel behind them, any nrhs >= 1 (two columns per matrix
 *                        walk when nrhs is even); ||b|| by a separate reduction: hipkkt_kkt_solve_multi on K with long rows
 *   route 1 "partials"   the partial maxima left to the refinement-round kernel, ||b|| riding along with the residual:
 *                        hipkkt_kkt_solve and the 2..8-column solves.  Needs nrhs in {1, 2, 4} and no row of K longer
 *                        than 4096 entries, HIPKKT_ERR_ARG otherwise
 *   route 2 "row-major"  N x KP work vectors, KP = nrhs rounded up to 16: hipkkt_kkt_solve_multi with 9 or more columns.
 *                        Needs no row of K longer than 4096 entries, HIPKKT_ERR_ARG otherwise
 * Synchronises.  Writes only the many-column work buffers: the right-hand side of hipkkt_kkt_setrhs and the last solution
 * are kept. */
int hipkkt_kkt_get_residual(hipkkt_kkt_t h, int route, int64_t nrhs, const double *x, const double *b, double *e,
                            double *norm_e, double *norm_b);
int hipkkt_kkt_get_maps(hipkkt_kkt_t h, int64_t *mapP, int64_t *mapA, int64_t *mapHs,
                        int64_t *map_diag_full, int64_t *map_soc_u, int64_t *map_soc_v,
                        int64_t *map_soc_D, int64_t *dsigns);   /* any may be NULL */
/* the GenPowExpansionMaps, concatenated in cone order: p (dim per cone), q (dim1), r (dim2), D (3); any may be NULL */
int hipkkt_kkt_get_genpow_maps(hipkkt_kkt_t h, int64_t *map_p, int64_t *map_q, int64_t *map_r, int64_t *map_D);
int hipkkt_kkt_get_perm(hipkkt_kkt_t h, int64_t *perm /* N, 0-based */);
int hipkkt_kkt_get_Hs(hipkkt_kkt_t h, double *Hsblocks /* |Hs|, positive */);
/* the NT scaling held on the device after hipkkt_kkt_update_from_sz*: the scaled point lambda (length m; a PSD cone
 * of side k keeps its k singular values, descending, in the first k of its slots), and for the PSD cones R and Rinv
 * (coneops_psdtrianglecone.jl:127-132), k x k column-major each, concatenated in cone order.  Any may be NULL. */
int hipkkt_kkt_get_scaling(hipkkt_kkt_t h, double *lambda, double *psd_R, double *psd_Rinv);
/* the rest of the device's NT scaling: w (m) and eta (one per cone), as hipkkt_kkt_system_update_cones takes them */
int hipkkt_kkt_get_scaling_w(hipkkt_kkt_t h, double *w, double *eta);
/* How the next device-side scaling treats the exponential and power cones (update_Hs, coneops_nonsymmetric_common.jl:
 * 50-67): strategy HIPKKT_SCALING_PRIMAL_DUAL (the default; mu is not read, the cone's own <s,z>/3 is used, :97-98) or
 * HIPKKT_SCALING_DUAL (Hs = mu H*(z)).  Host-only, no device work: call it once per iteration before
 * hipkkt_kkt_update_from_sz[_dev], hipkkt_kkt_system_update[_host] or hipkkt_kkt_system_update_and_solve_affine, in
 * lazy mode too.  On a handle without such cones it does nothing and returns 0.
 * A generalized power cone always takes Hs = mu H*(z) (allows_primal_dual_scaling is false, coneops_genpowcone.jl:21):
 * mu is read for it under BOTH strategies. */
int hipkkt_kkt_set_nonsymmetric_scaling(hipkkt_kkt_t h, int strategy, double mu);
/* After a device-side scaling: grad f*(z) (3 doubles) and the Hessian H*(z) (9 doubles, symmetric) of every exponential
 * and power cone, in cone order -- K.grad and K.H_dual, which combined_ds_shift! reads.  Either may be NULL.  The caller sizes
 * the arrays from its own cone list. */
int hipkkt_kkt_get_nonsymmetric(hipkkt_kkt_t h, double *grad, double *H_dual);
/* After a device-side scaling, for the generalized power cones, concatenated in cone order: grad f*(z) (dim per cone --
 * K.data.grad, which combined_ds_shift! reads), d (dim per cone: d1, then d2 repeated dim2 times), p (dim), q (dim1),
 * r (dim2), all unscaled: Hs = mu (diag(d) + p p' - q q' - r r') (update_dual_grad_H, coneops_genpowcone.jl:336-389).
 * Any may be NULL.  hipkkt_kkt_get_nonsymmetric covers the exponential and power cones only. */
int hipkkt_kkt_get_genpow(hipkkt_kkt_t h, double *grad, double *d, double *p, double *q, double *r);
double hipkkt_kkt_last_regularizer(hipkkt_kkt_t h);
int64_t hipkkt_kkt_last_ir_iterations(hipkkt_kkt_t h);
/* (tests) the refinement rounds a solve enqueues ahead of its first status read-back -- what the previous solves took
 * (kktsolver_directldl.jl:397-449 decides round by round; here the rounds are enqueued speculatively and the reference's
 * accept / stop rule runs on the device).  set >= 0 replaces it first; returns the value in force, < 0 on a null handle. */
int hipkkt_kkt_speculative_rounds(hipkkt_kkt_t h, int set);

/* run on the caller's stream (e.g. torch's current stream) instead of the handle's own */
int hipkkt_kkt_set_stream(hipkkt_kkt_t h, void *hip_stream);
int hipkkt_kkt_synchronize(hipkkt_kkt_t h);
/* per-phase device timing */
int hipkkt_kkt_profile_enable(hipkkt_kkt_t h, int enable);
int hipkkt_kkt_profile_reset(hipkkt_kkt_t h);
int hipkkt_kkt_profile_get(hipkkt_kkt_t h, hipkkt_profile *out);

#ifdef __cplusplus
}
#endif
#endif
