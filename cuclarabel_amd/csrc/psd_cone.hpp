// The building blocks of the PSD cone kernels (kernels.hip: scaling, mul_Hs, sys_offset; step_kernels.hip: step_ds,
// step_length, margins, barrier), each written once, and the two size classes as a compile-time policy.  Device-only.
//
// A PSD cone is handled by one workgroup of NT threads.  What differs between the classes is in the policy structs
// at the end of this file -- PsdSmall (side <= kPsdMaxDim: 256 threads, C.psd_list, every work matrix in LDS) and PsdBig
// (side <= kPsdBigMaxDim on an opted-in handle: kPsdBigThreads threads, C.psdb_list, at most two matrices in LDS and the
// others in the workgroup's slice of C.psd_work) -- and a kernel body `template <class P>` picks between them with
// `if constexpr`: the arithmetic, and the order of every fma chain and reduction, is the one text below for both.
// Matrices are k x k, column-major, in LDS or (big class) in HBM behind a workgroup barrier.
#pragma once
#include "kernels.hpp"
#include <cfloat>
#include <cmath>

namespace hipkkt {

constexpr double kIs2 = 0.70710678118654752440;        // 1/sqrt(2)
constexpr double kS2 = 1.41421356237309504880;         // sqrt(2)

__device__ inline void svec_index(int idx, int& row, int& col)     // idx = col(col+1)/2 + row, row <= col
{
    int c = (int)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
    while (c * (c + 1) / 2 > idx) --c;
    while ((c + 1) * (c + 2) / 2 <= idx) ++c;
    col = c;
    row = idx - c * (c + 1) / 2;
}

struct OpMin { __device__ double operator()(double a, double b) const { return fmin(a, b); } };
struct OpMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };
struct OpSum { __device__ double operator()(double a, double b) const { return a + b; } };

// fixed tree over the NT threads of a workgroup; every thread gets the result
template <int NT, class Op>
__device__ inline double block_reduce_n(double v, double* sh, Op op)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (tid < o) sh[tid] = op(sh[tid], sh[tid + o]);
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------
//  Eigenvalues of a symmetric k x k matrix in LDS (both triangles stored, column-major): cyclic two-sided Jacobi with the
//  round-robin pairing of psd_onesided_jacobi -- m/2 disjoint pairs (p, q) per step, eight lanes per pair.  A step is
//      1. every pair reads (a_pp, a_qq, a_pq) and forms its rotation (c, s)         [barrier]
//      2. A <- A J: the pair rotates its two columns                                [barrier]
//      3. A <- J'A: the pair rotates its two rows; the 2 x 2 block gets its exact values (a_pq = 0)   [barrier]
//  The pairs of a step touch disjoint columns in 2 and disjoint rows in 3.  Unlike the one-sided sweep (an SVD) this
//  keeps the signs, and its error in every eigenvalue is ABSOLUTE, a modest multiple of k u ||A|| -- what the step
//  length needs of the smallest one (the reference calls LAPACK's syevr).  Rotations stop when a whole sweep saw no
//  off-diagonal entry above 2^-60 ||A||_F.  On return the eigenvalues are the diagonal.  All NT threads call; NT / 8
//  groups of eight lanes must cover the pairs: 256 threads up to side 64, kPsdBigThreads up to kPsdBigMaxDim.
//  sh: NT doubles of LDS.
// ---------------------------------------------------------------------------------------------------------------------
template <int NT>
__device__ inline void sym_jacobi_eig(double* A, int k, double* sh)
{
    const int tid = threadIdx.x;
    double f = 0.0;
    for (int idx = tid; idx < k * k; idx += NT) f += A[idx] * A[idx];
    f = sqrt(block_reduce_n<NT>(f, sh, OpSum{}));
    if (!(f > 0.0) || !(f <= DBL_MAX)) return;          // the zero matrix (or a non-finite one: unspecified input)
    const double thr_conv = ldexp(f, -60), thr_skip = ldexp(f, -80);
    const int mm = (k + 1) & ~1, npair = mm / 2;         // at most NT / 8 pairs
    const int grp = tid >> 3, sub = tid & 7;
    for (int sweep = 0; sweep < 40; ++sweep) {
        double myoff = 0.0;
        for (int step = 0; step < mm - 1; ++step) {
            bool act = false;
            int p = 0, q = 0;
            double c = 1.0, s = 0.0, app2 = 0.0, aqq2 = 0.0;
            if (grp < npair) {
                if (grp == 0) { p = mm - 1; q = step; }
                else { p = (step + grp) % (mm - 1); q = (step - grp + (mm - 1)) % (mm - 1); }
                if (p > q) { const int tmp = p; p = q; q = tmp; }
                if (q < k) {                                           // (q == k: the dummy index of an odd k)
                    const double apq = A[p + q * k], app = A[p + p * k], aqq = A[q + q * k];
                    myoff = fmax(myoff, fabs(apq));
                    if (fabs(apq) > thr_skip) {
                        act = true;
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = c * t;
                        app2 = app - t * apq;
                        aqq2 = aqq + t * apq;
                    }
                }
            }
            __syncthreads();
            if (act) {
                for (int i = sub; i < k; i += 8) {
                    const double ap = A[i + p * k], aq = A[i + q * k];
                    A[i + p * k] = c * ap - s * aq;
                    A[i + q * k] = s * ap + c * aq;
                }
            }
            __syncthreads();
            if (act) {
                for (int j = sub; j < k; j += 8) {
                    if (j == p) { A[p + p * k] = app2; A[q + p * k] = 0.0; }
                    else if (j == q) { A[p + q * k] = 0.0; A[q + q * k] = aqq2; }
                    else {
                        const double ap = A[p + j * k], aq = A[q + j * k];
                        A[p + j * k] = c * ap - s * aq;
                        A[q + j * k] = s * ap + c * aq;
                    }
                }
            }
            __syncthreads();
        }
        const double offn = block_reduce_n<NT>(myoff, sh, OpMax{});
        if (offn <= thr_conv) break;
    }
}

// X = mat(scale * x) of an svec vector (coneops_psdtrianglecone.jl:469-483), both triangles
template <int NT>
__device__ inline void psd_load_mat(double* X, const double* __restrict__ x, double scale, int k)
{
    const int t = k * (k + 1) / 2;
    for (int idx = threadIdx.x; idx < t; idx += NT) {
        int r, cl;
        svec_index(idx, r, cl);
        const double v = scale * x[idx] * (r == cl ? 1.0 : kIs2);
        X[r + cl * k] = v;
        X[cl + r * k] = v;
    }
}

// Sm = mat(s), Zm = mat(z) of the cone's two svec vectors, both triangles
template <int NT>
__device__ inline void psd_load_pair(double* Sm, double* Zm, const double* __restrict__ s, const double* __restrict__ z, int k)
{
    const int t = k * (k + 1) / 2;
    for (int idx = threadIdx.x; idx < t; idx += NT) {
        int r, cl;
        svec_index(idx, r, cl);
        const double sv = s[idx], zv = z[idx];
        if (r == cl) { Sm[r + cl * k] = sv; Zm[r + cl * k] = zv; }
        else {
            Sm[r + cl * k] = Sm[cl + r * k] = sv * kIs2;
            Zm[r + cl * k] = Zm[cl + r * k] = zv * kIs2;
        }
    }
}

// M = G' X G for symmetric X, exactly symmetric (each pair (r, c) from both orders, averaged).  mul_W!(:N) is G = R
// (R' X R, :409-437 with :N), mul_Winv!(:T) is G = Rinv' (Rinv X Rinv').  T: work matrix.  Ends with a barrier.
// (The big class passes T, and where it can M, in its work area in HBM: the workgroup's own stores, read behind a barrier.)
template <int NT>
__device__ inline void psd_congruence(double* M, double* T, const double* G, const double* X, int k)
{
    const int tid = threadIdx.x, kk = k * k, t = k * (k + 1) / 2;
    for (int idx = tid; idx < kk; idx += NT) {           // T = X G
        const int r = idx % k, cl = idx / k;
        double acc = 0.0;
        for (int q = 0; q < k; ++q) acc = fma(X[r + q * k], G[q + cl * k], acc);
        T[idx] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < t; idx += NT) {            // M = G' T
        int r, cl;
        svec_index(idx, r, cl);
        double a1 = 0.0, a2 = 0.0;
        for (int q = 0; q < k; ++q) { a1 = fma(G[q + r * k], T[q + cl * k], a1); a2 = fma(G[q + cl * k], T[q + r * k], a2); }
        const double v = r == cl ? a1 : 0.5 * (a1 + a2);
        M[r + cl * k] = v;
        M[cl + r * k] = v;
    }
    __syncthreads();
}

// G = R (transpose = 0) or Rinv' (transpose = 1) into LDS
template <int NT>
__device__ inline void psd_load_G(double* G, const double* __restrict__ src, int k, int transpose)
{
    for (int idx = threadIdx.x; idx < k * k; idx += NT) {
        const int r = idx % k, cl = idx / k;
        G[idx] = transpose ? src[cl + r * k] : src[idx];
    }
}

// Cholesky factor of the symmetric X in place (lower triangle; the upper one keeps what it held), right-looking
// (coneops_psdtrianglecone.jl:97-104).  A pivot that is not positive sets *sh_fail (LDS, zeroed by the caller before a
// barrier) and ends the factorisation for the whole workgroup.  per_pivot(sqrt(pivot)) runs on thread 0 only: how the
// barrier function collects its logarithms.  Ends with a barrier.
template <int NT, class F>
__device__ inline void psd_cholesky(double* Mx, int k, int* sh_fail, F per_pivot)
{
    const int tid = threadIdx.x;
    for (int j = 0; j < k; ++j) {
        const double d = Mx[j + j * k];
        if (!(d > 0.0)) { if (tid == 0) *sh_fail = 1; }
        __syncthreads();
        if (*sh_fail) break;
        const double sd = sqrt(d);
        for (int i = j + 1 + tid; i < k; i += NT) Mx[i + j * k] /= sd;
        if (tid == 0) { Mx[j + j * k] = sd; per_pivot(sd); }
        __syncthreads();
        const int w = k - j - 1;
        for (int idx = tid; idx < w * w; idx += NT) {
            const int a = j + 1 + idx / w, b = j + 1 + idx % w;
            if (a >= b) Mx[a + b * k] -= Mx[a + j * k] * Mx[b + j * k];
        }
        __syncthreads();
    }
}

// SVD of M by a one-sided (Hestenes) Jacobi: column pairs (p, q) of M, and of V with them, are rotated until all
// columns of M are mutually orthogonal; then M = U diag(sv) and V holds the right singular vectors.  Every singular
// value comes out to high RELATIVE accuracy.  Rotations in the round-robin order: a sweep is m - 1 steps of m/2
// rotations on disjoint column pairs, eight lanes per pair, one barrier per step; at most 60 sweeps, a pair whose inner
// product is below 1e-300 or 1e-17 of the norms' product is left alone, and a sweep that saw no cosine above 1e-15 is
// the last.  NT / 8 groups must cover the pairs; sh_off: NT / 8 doubles of LDS.
template <int NT>
__device__ inline void psd_onesided_jacobi(double* M, double* V, int k, double* sh_off)
{
    const int tid = threadIdx.x;
    const int m = (k + 1) & ~1, npair = m / 2;
    const int grp = tid >> 3, sub = tid & 7;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double myoff = 0.0;
        for (int step = 0; step < m - 1; ++step) {
            if (grp < npair) {
                int p, q;
                if (grp == 0) { p = m - 1; q = step; }
                else { p = (step + grp) % (m - 1); q = (step - grp + (m - 1)) % (m - 1); }
                if (p > q) { const int tmp = p; p = q; q = tmp; }
                if (q < k) {                                           // (q == k: the dummy index of an odd k)
                    double a = 0.0, b = 0.0, cc = 0.0;
                    for (int i = sub; i < k; i += 8) {
                        const double mp = M[i + p * k], mq = M[i + q * k];
                        a = fma(mp, mp, a); b = fma(mq, mq, b); cc = fma(mp, mq, cc);
                    }
#pragma unroll
                    for (int o = 4; o > 0; o >>= 1) {
                        a += __shfl_xor(a, o, 8); b += __shfl_xor(b, o, 8); cc += __shfl_xor(cc, o, 8);
                    }
                    const double ab = sqrt(a) * sqrt(b);       // (sqrt(a * b) overflows / flushes for entries beyond ~2^+-256)
                    if (!(fabs(cc) <= 1e-300 || fabs(cc) <= 1e-17 * ab)) {
                        myoff = fmax(myoff, fabs(cc) / ab);
                        const double zeta = (b - a) / (2.0 * cc);
                        const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
                        for (int i = sub; i < k; i += 8) {
                            const double mp = M[i + p * k], mq = M[i + q * k];
                            M[i + p * k] = cs * mp - sn * mq;
                            M[i + q * k] = sn * mp + cs * mq;
                            const double vp = V[i + p * k], vq = V[i + q * k];
                            V[i + p * k] = cs * vp - sn * vq;
                            V[i + q * k] = sn * vp + cs * vq;
                        }
                    }
                }
            }
            __syncthreads();               // the next step pairs the columns differently
        }
        if (sub == 0) sh_off[grp] = grp < npair ? myoff : 0.0;
        __syncthreads();
        double offn = 0.0;
        for (int i = 0; i < npair; ++i) offn = fmax(offn, sh_off[i]);   // uniform: every thread reads the same words
        __syncthreads();
        if (offn < 1e-15) break;
    }
}

// singular values = the column norms of M = U diag(sv), into sh_sv; sh_rank[i] = the place of sv_i in descending order
// (LAPACK's, dense_algebra.jl:219; equal values keep their index order); lam (where the handle keeps one) = the sorted
// values in the first k of the cone's t slots, zeros behind them.  Ends with a barrier.
template <int NT>
__device__ inline void psd_singular_values(const double* M, int k, double* sh_sv, int* sh_rank, double* lam)
{
    const int tid = threadIdx.x, t = k * (k + 1) / 2;
    if (tid < k) {
        double nrm = 0.0;
        for (int i = 0; i < k; ++i) nrm = fma(M[i + tid * k], M[i + tid * k], nrm);
        sh_sv[tid] = sqrt(nrm);
    }
    __syncthreads();
    if (tid < k) {
        const double mine = sh_sv[tid];
        int rank = 0;
        for (int i = 0; i < k; ++i) rank += (sh_sv[i] > mine || (sh_sv[i] == mine && i < tid)) ? 1 : 0;
        sh_rank[tid] = rank;
        if (lam) lam[rank] = mine;
    }
    if (lam) for (int i = k + tid; i < t; i += NT) lam[i] = 0.0;
    __syncthreads();
}

// R = L1 V Lam^{-1/2} (columns in sorted order), Rinv = Lam^{-1/2} U' L2' (rows in sorted order), :127-132, from the
// lower-triangular L1, L2 (zero above the diagonal) and the Jacobi's M = U diag(sv), V.  Rinv goes to Riout;
// store_R(index, value) stores an entry of R.
template <int NT, class Store>
__device__ inline void psd_R_Rinv(const double* L1, const double* L2, const double* M, const double* V, int k,
                                  const double* sh_sv, const int* sh_rank, double* __restrict__ Riout, Store store_R)
{
    for (int idx = threadIdx.x; idx < k * k; idx += NT) {
        const int r = idx % k, cl = idx / k;
        double acc = 0.0;
        for (int q = 0; q <= r; ++q) acc = fma(L1[r + q * k], V[q + cl * k], acc);
        const double sc = 1.0 / sqrt(sh_sv[cl]);
        store_R(r + sh_rank[cl] * k, acc * sc);
        // Rinv(row cl of the unsorted order, column r): (1/sqrt(s_cl)) (1/s_cl) sum_q M(q, cl) L2(r, q)
        double acc2 = 0.0;
        for (int q = 0; q <= r; ++q) acc2 = fma(M[q + cl * k], L2[r + q * k], acc2);
        Riout[sh_rank[cl] + r * k] = acc2 * sc / sh_sv[cl];
    }
}

// A = R R' (:135-141): the upper triangle (syrk 'U'), mirrored, so exactly symmetric; store_A(r, c, value), r <= c
template <int NT, class Store>
__device__ inline void psd_A_from_R_sym(const double* R, int k, Store store_A)
{
    for (int idx = threadIdx.x; idx < k * k; idx += NT) {
        const int r = idx % k, cl = idx / k;
        double acc = 0.0;
        if (r <= cl) {
            for (int q = 0; q < k; ++q) acc = fma(R[r + q * k], R[cl + q * k], acc);
            store_A(r, cl, acc);
        }
    }
}

// svec(G X G') for symmetric X (kGt = false: G symmetric, so T = X G) or svec(G X G') through T = X G' (kGt = true):
// T = the first product, then entry (r, c) of G T from both orders, off-diagonal ones as (a1 + a2)/sqrt(2);
// store(svec index, value).  T: where the first product is written; Tl: the LDS it is read from.  kCopyBack: T lies
// in HBM and Tl is X's place -- T cannot be written over X while other threads still read X's rows, so it makes the
// round trip and every thread copies back the entries it wrote itself.  Without it T == Tl.
template <int NT, bool kGt, bool kCopyBack, class Store>
__device__ inline void psd_sandwich_svec(const double* X, const double* G, double* T, double* Tl, int k, Store store)
{
    const int tid = threadIdx.x, kk = k * k, t = k * (k + 1) / 2;
    for (int idx = tid; idx < kk; idx += NT) {
        const int r = idx % k, cl = idx / k;
        double acc = 0.0;
        for (int q = 0; q < k; ++q) acc = fma(X[r + q * k], G[kGt ? cl + q * k : q + cl * k], acc);
        T[idx] = acc;
    }
    __syncthreads();
    if constexpr (kCopyBack) {
        for (int idx = tid; idx < kk; idx += NT) Tl[idx] = T[idx];
        __syncthreads();
    }
    for (int idx = tid; idx < t; idx += NT) {
        int r, cl;
        svec_index(idx, r, cl);
        double a1 = 0.0, a2 = 0.0;
        for (int q = 0; q < k; ++q) { a1 = fma(G[r + q * k], Tl[q + cl * k], a1); a2 = fma(G[cl + q * k], Tl[q + r * k], a2); }
        store(idx, (r == cl) ? a1 : (a1 + a2) * kIs2);
    }
}

// entry ((i, j), (kq, l)), i <= j, kq <= l, of A (x)_s A (skron!, coneops_psdtrianglecone.jl:502-540)
__device__ inline double psd_hs_entry(const double* Am, int k, int i, int j, int kq, int l)
{
    const double s2 = kS2;
    const bool ij = (i == j), kl = (kq == l);
    if (!ij && !kl) return Am[i + kq * k] * Am[j + l * k] + Am[i + l * k] * Am[j + kq * k];
    if (ij && !kl) return s2 * Am[j + l * k] * Am[j + kq * k];
    if (!ij && kl) return s2 * Am[i + l * k] * Am[j + kq * k];
    return Am[j + l * k] * Am[j + l * k];
}

// ---- the two size classes.  cone(): the workgroup's cone; work(): the workgroup's 3 psdb_kmax^2 doubles of C.psd_work
struct PsdSmall {
    static constexpr int NT = 256, kMaxDim = kPsdMaxDim;
    static constexpr bool kBig = false;
    __device__ static int cone(const ConeDev& C) { return C.psd_list[blockIdx.x]; }
};
struct PsdBig {
    static constexpr int NT = kPsdBigThreads, kMaxDim = kPsdBigMaxDim;
    static constexpr bool kBig = true;
    __device__ static int cone(const ConeDev& C) { return C.psdb_list[blockIdx.x]; }
    __device__ static double* work(const ConeDev& C) { return C.psd_work + (size_t)blockIdx.x * 3 * C.psdb_kmax * C.psdb_kmax; }
};
static_assert((PsdSmall::kMaxDim + 1) / 2 <= PsdSmall::NT / 8 && (PsdBig::kMaxDim + 1) / 2 <= PsdBig::NT / 8,
              "one group of eight lanes per column pair");

}  // namespace hipkkt
