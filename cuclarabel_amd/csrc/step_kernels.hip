// The cone operations an interior-point loop performs BETWEEN its KKT solves, on device vectors (see kernels.hpp):
//   affine_ds!, combined_ds_shift!      coneops_compositecone.jl:153-182
//   step_length                         coneops_compositecone.jl:205-243
//   margins, scaled_unit_shift!         coneops_compositecone.jl:49-76
// for the symmetric cones (zero, nonnegative, second-order, PSD side <= kPsdMaxDim; on an opted-in handle the big PSD
// class up to kPsdBigMaxDim: one body per operation, instantiated for either class, see psd_cone.hpp).  Launch shapes as
// k_sys_offset / k_sys_offset_psd: an elementwise grid-stride part with one wave per second-order cone riding behind it,
// one workgroup per PSD cone (256 threads and its matrices in LDS; the big class 512 threads, at most two matrices in
// LDS and the others in its work area).  Compiled without FMA contraction: the exact-zero branches of the
// second-order step length are tested on products and differences formed as the reference forms them.
//
// The exponential and the power cone (three rows each) ride behind them for handles that hold one: one lane per cone
// through the handle's lists of such cones, see "exponential and power cones between the solves" below.  Generalized
// power cones ride behind those: one wave or one workgroup per cone, as the scaling kernel splits them, see "generalized
// power cones between the solves".
//
// Every reduction has a fixed layout (a slot per workgroup / wave / cone in a partials array, folded by one workgroup in
// a fixed order) and there is no floating-point atomic: the same call on the same data gives the same bits.
#include "kernels.hpp"
#include "nonsym_cone.hpp"
#include "psd_cone.hpp"
#include <cfloat>
#include <cmath>

namespace hipkkt {

namespace {

__device__ inline double st_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <class Op>
__device__ inline double block_reduce_256(double v, double* sh, Op op) { return block_reduce_n<256>(v, sh, op); }

__device__ inline void st_publish(const Publish& P)
{
    for (int i = 0; i < P.n; ++i) P.dst[i] = P.rec[i];
    P.dst[P.n] = P.seq;
    for (int i = 0; i < P.nzero; ++i) P.rec[i] = 0.0;
}

// =====================================================================================================================
//  affine_ds! / combined ds: out = lambda o lambda [+ (W^{-T} step_s) o (W (m step_z)) - sigma_mu e]
// =====================================================================================================================
__device__ inline void step_ds_elementwise_body(const ConeDev& C, const ConeState& S, double* __restrict__ out,
                                                const double* __restrict__ dz, const double* __restrict__ ds,
                                                double sigma_mu, double m_corr, int m, int combined, int bx, int nb)
{
    for (int i = bx * 256 + threadIdx.x; i < m; i += nb * 256) {
        const int kind = C.kind[C.elem_cone[i]];
        if (kind == 0) out[i] = 0.0;                                    // coneops_zerocone.jl
        else if (kind == 1) {                                           // coneops_nncone.jl:117-126, :196-227
            const double l = S.lam[i];
            double o = l * l;
            if (combined) {
                const double w = S.w[i];
                o += (ds[i] / w) * (w * (m_corr * dz[i])) - sigma_mu;
            }
            out[i] = o;
        }
    }
}

// one wave per second-order cone: circ_op! (coneops_socone.jl:376-392), mul_W! / mul_Winv! (:313-357)
__device__ inline void step_ds_soc_body(const ConeDev& C, const ConeState& S, double* __restrict__ out,
                                        const double* __restrict__ dz, const double* __restrict__ ds, double sigma_mu,
                                        double m_corr, int combined, int ci, int lane)
{
    const int c = C.soc_list[ci];
    const int off = C.off[c], n = C.numel[c];
    const double* lam = S.lam + off;
    const double* w = S.w + off;
    double ll = 0.0, zz = 0.0, zs = 0.0;
    for (int i = lane; i < n; i += 64) ll += lam[i] * lam[i];
    if (combined)
        for (int i = 1 + lane; i < n; i += 64) {
            zz += w[i] * (m_corr * dz[off + i]);
            zs += w[i] * ds[off + i];
        }
    ll = st_wave_sum(ll);
    const double l0 = lam[0];
    if (!combined) {
        for (int i = lane; i < n; i += 64) out[off + i] = i == 0 ? ll : l0 * lam[i] + l0 * lam[i];
        return;
    }
    zz = st_wave_sum(zz);
    zs = st_wave_sum(zs);
    const double eta = S.eta[c], etainv = 1.0 / eta, w0 = w[0];
    const double dz0 = m_corr * dz[off], ds0 = ds[off];
    const double cz = dz0 + zz / (1.0 + w0), cs = -ds0 + zs / (1.0 + w0);
    const double Z0 = eta * (w0 * dz0 + zz), Y0 = etainv * (w0 * ds0 - zs);
    double yz = 0.0;
    for (int i = 1 + lane; i < n; i += 64) {
        const double Zi = eta * (m_corr * dz[off + i] + cz * w[i]);
        const double Yi = etainv * (ds[off + i] + cs * w[i]);
        yz += Yi * Zi;
        out[off + i] = (l0 * lam[i] + l0 * lam[i]) + (Y0 * Zi + Z0 * Yi);
    }
    yz = st_wave_sum(yz);
    if (lane == 0) out[off] = ll + ((Y0 * Z0 + yz) - sigma_mu);
}

__global__ __launch_bounds__(256) void k_step_ds(ConeDev C, ConeState S, double* __restrict__ out, const double* __restrict__ dz,
                                                 const double* __restrict__ ds, double sigma_mu, double m_corr, int m,
                                                 int combined, int ge)
{
    if ((int)blockIdx.x < ge) { step_ds_elementwise_body(C, S, out, dz, ds, sigma_mu, m_corr, m, combined, blockIdx.x, ge); return; }
    const int ci = ((int)blockIdx.x - ge) * 4 + (int)(threadIdx.x >> 6);
    if (ci < C.nsoc) step_ds_soc_body(C, S, out, dz, ds, sigma_mu, m_corr, combined, ci, threadIdx.x & 63);
}

// PSD cones (coneops_psdtrianglecone.jl:189-205, circ_op! :361-382): Z = R'mat(m dz)R, Y = Rinv mat(ds) Rinv',
// out = svec((YZ + ZY)/2) with lambda_i^2 - sigma_mu added on the diagonal.  One workgroup per cone, of either class
// (psd_cone.hpp: PsdSmall, PsdBig).  LDS: the operands G and X of a product, and for the small class T and Z behind
// them; the big class has T and Z in its work area.  c: the cone, P::cone(C); smem: the workgroup's dynamic LDS.
template <class P>
__device__ inline void step_ds_psd_body(const ConeDev& C, const ConeState& S, double* __restrict__ out,
                                        const double* __restrict__ dz, const double* __restrict__ ds, double sigma_mu,
                                        double m_corr, int combined, int c, double* smem)
{
    constexpr int NT = P::NT;
    const int tid = threadIdx.x;
    const int k = C.psd_dim[c], off = C.off[c], kk = k * k, t = k * (k + 1) / 2;
    if constexpr (!P::kBig) if (k == 0) return;
    const double* lam = S.lam + off;
    if (!combined) {
        for (int idx = tid; idx < t; idx += NT) {
            int r, cl;
            svec_index(idx, r, cl);
            out[off + idx] = r == cl ? lam[r] * lam[r] : 0.0;
        }
        return;
    }
    double* G = smem;
    double* X = smem + kk;          // mat(ds), then Y
    double* T = smem + 2 * kk;
    double* Z = smem + 3 * kk;
    if constexpr (P::kBig) { T = P::work(C); Z = T + kk; }
    psd_load_G<NT>(G, S.psdR + C.psd_aoff[c], k, 0);
    psd_load_mat<NT>(X, dz + off, m_corr, k);
    __syncthreads();
    psd_congruence<NT>(Z, T, G, X, k);
    psd_load_G<NT>(G, S.psdRinv + C.psd_aoff[c], k, 1);
    psd_load_mat<NT>(X, ds + off, 1.0, k);
    __syncthreads();
    psd_congruence<NT>(X, T, G, X, k);                   // (the product X G is complete before X is overwritten)
    const double* Y = X;
    for (int idx = tid; idx < t; idx += NT) {
        int r, cl;
        svec_index(idx, r, cl);
        double a1 = 0.0, a2 = 0.0;
        for (int q = 0; q < k; ++q) { a1 = fma(Y[r + q * k], Z[q + cl * k], a1); a2 = fma(Z[r + q * k], Y[q + cl * k], a2); }
        const double v = 0.5 * (a1 + a2);
        out[off + idx] = r == cl ? lam[r] * lam[r] + (v - sigma_mu) : v * kS2;
    }
}
__global__ __launch_bounds__(PsdSmall::NT) void k_step_ds_psd(ConeDev C, ConeState S, double* __restrict__ out,
                                                              const double* __restrict__ dz, const double* __restrict__ ds,
                                                              double sigma_mu, double m_corr, int combined)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    step_ds_psd_body<PsdSmall>(C, S, out, dz, ds, sigma_mu, m_corr, combined, PsdSmall::cone(C), smem);
}
__global__ __launch_bounds__(PsdBig::NT) void k_step_ds_psd_big(ConeDev C, ConeState S, double* __restrict__ out,
                                                                const double* __restrict__ dz, const double* __restrict__ ds,
                                                                double sigma_mu, double m_corr, int combined)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    step_ds_psd_body<PsdBig>(C, S, out, dz, ds, sigma_mu, m_corr, combined, PsdBig::cone(C), smem);
}

// =====================================================================================================================
//  step_length: every cone's limit is min(alpha_max, f(cone)), so the composite's sequential tightening of alpha_max
//  (coneops_compositecone.jl:205-243) is an order-free minimum: each workgroup / wave / PSD cone leaves its f in a slot
//  of `partial` (DBL_MAX where nothing binds), and the finishing kernel takes the minimum with the tau / kappa limits.
// =====================================================================================================================
__device__ inline void step_length_elementwise_body(const ConeDev& C, const double* __restrict__ dz, const double* __restrict__ ds,
                                                    const double* __restrict__ z, const double* __restrict__ s, int m,
                                                    double* __restrict__ partial, int bx, int nb, double* sh)
{
    double a = DBL_MAX;
    for (int i = bx * 256 + threadIdx.x; i < m; i += nb * 256) {
        if (C.kind[C.elem_cone[i]] != 1) continue;                     // coneops_nncone.jl:151-170
        const double dzi = dz[i], dsi = ds[i];
        if (dzi < 0.0) a = fmin(a, -z[i] / dzi);
        if (dsi < 0.0) a = fmin(a, -s[i] / dsi);
    }
    a = block_reduce_256(a, sh, OpMin{});
    if (threadIdx.x == 0) partial[bx] = a;
}

// _step_length_soc_component (coneops_socone.jl:443-512) with alpha_max = DBL_MAX; ny = ||y[2:end]||, nx = ||x[2:end]||,
// xy = <x[2:end], y[2:end]>
__device__ inline double soc_step_component(double x0, double y0, double nx, double ny, double xy)
{
    double amax = DBL_MAX;
    if (x0 >= 0.0 && y0 < 0.0) amax = fmin(amax, -x0 / y0);
    const double a = (y0 - ny) * (y0 + ny);                            // _soc_residual, :415-419
    const double b = 2.0 * (x0 * y0 - xy);
    const double c = fmax(0.0, (x0 - nx) * (x0 + nx));
    const double d = b * b - 4.0 * a * c;
    if ((a > 0.0 && b > 0.0) || d < 0.0) return amax;
    if (a == 0.0) return amax;
    if (c == 0.0) return a >= 0.0 ? amax : 0.0;
    const double t = b >= 0.0 ? (-b - sqrt(d)) : (-b + sqrt(d));
    double r1 = (2.0 * c) / t, r2 = t / (2.0 * a);
    if (r1 < 0.0) r1 = DBL_MAX;
    if (r2 < 0.0) r2 = DBL_MAX;
    return fmin(amax, fmin(r1, r2));
}

__device__ inline void step_length_soc_body(const ConeDev& C, const double* __restrict__ dz, const double* __restrict__ ds,
                                            const double* __restrict__ z, const double* __restrict__ s,
                                            double* __restrict__ slot, int ci, int lane)
{
    const int c = C.soc_list[ci];
    const int off = C.off[c], n = C.numel[c];
    double zz = 0.0, dd = 0.0, zd = 0.0, ss = 0.0, ee = 0.0, se = 0.0;
    for (int i = 1 + lane; i < n; i += 64) {
        const double zi = z[off + i], di = dz[off + i], si = s[off + i], ei = ds[off + i];
        zz += zi * zi; dd += di * di; zd += zi * di;
        ss += si * si; ee += ei * ei; se += si * ei;
    }
    zz = sqrt(st_wave_sum(zz)); dd = sqrt(st_wave_sum(dd)); zd = st_wave_sum(zd);
    ss = sqrt(st_wave_sum(ss)); ee = sqrt(st_wave_sum(ee)); se = st_wave_sum(se);
    if (lane == 0) {
        const double az = soc_step_component(z[off], dz[off], zz, dd, zd);
        const double as = soc_step_component(s[off], ds[off], ss, ee, se);
        *slot = fmin(az, as);
    }
}

__global__ __launch_bounds__(256) void k_step_length(ConeDev C, const double* __restrict__ dz, const double* __restrict__ ds,
                                                     const double* __restrict__ z, const double* __restrict__ s, int m,
                                                     double* __restrict__ partial, int ge)
{
    __shared__ double sh[256];
    if ((int)blockIdx.x < ge) { step_length_elementwise_body(C, dz, ds, z, s, m, partial, blockIdx.x, ge, sh); return; }
    const int ci = ((int)blockIdx.x - ge) * 4 + (int)(threadIdx.x >> 6);
    if (ci < C.nsoc) step_length_soc_body(C, dz, ds, z, s, partial + ge + ci, ci, threadIdx.x & 63);
}

// PSD cones (coneops_psdtrianglecone.jl:230-254, :439-466): both components by the cone's workgroup, its limit into
// slots[blockIdx.x].  gamma = lambda_min(Lam^{-1/2} mat(d) Lam^{-1/2}), d = W dz or W^{-T} ds; the limit is 1/(-gamma)
// where gamma < 0.  LDS: G and X, and for the small class T and M behind them; the big class has T in its work area and
// M in X's place, where the two-sided Jacobi then runs.
template <class P>
__device__ inline void step_length_psd_body(const ConeDev& C, const ConeState& S, const double* __restrict__ dz,
                                            const double* __restrict__ ds, double* __restrict__ slots, double* smem)
{
    __shared__ double sh[P::NT];
    constexpr int NT = P::NT;
    const int tid = threadIdx.x;
    const int c = P::cone(C);
    const int k = C.psd_dim[c], off = C.off[c], kk = k * k;
    if constexpr (!P::kBig) if (k == 0) { if (tid == 0) slots[blockIdx.x] = DBL_MAX; return; }
    double* G = smem;
    double* X = smem + kk;
    double* T = smem + 2 * kk;
    double* M = smem + 3 * kk;
    if constexpr (P::kBig) { T = P::work(C); M = X; }
    const double* lam = S.lam + off;
    double alpha = DBL_MAX;
    for (int comp = 0; comp < 2; ++comp) {
        psd_load_G<NT>(G, (comp == 0 ? S.psdR : S.psdRinv) + C.psd_aoff[c], k, comp);
        psd_load_mat<NT>(X, (comp == 0 ? dz : ds) + off, 1.0, k);
        __syncthreads();
        psd_congruence<NT>(M, T, G, X, k);               // (the product X G is complete before X is overwritten)
        for (int idx = tid; idx < kk; idx += NT) {       // lrscale! with Lam^{-1/2} (symmetric entries get the same factors)
            const int r = idx % k, cl = idx / k;
            M[idx] = M[idx] * ((1.0 / sqrt(lam[r])) * (1.0 / sqrt(lam[cl])));
        }
        __syncthreads();
        sym_jacobi_eig<NT>(M, k, sh);
        double g = DBL_MAX;
        for (int i = 0; i < k; ++i) g = fmin(g, M[i + i * k]);          // uniform: every thread reads the same words
        if (g < 0.0) alpha = fmin(alpha, 1.0 / (-g));
        __syncthreads();
    }
    if (tid == 0) slots[blockIdx.x] = alpha;
}
__global__ __launch_bounds__(PsdSmall::NT) void k_step_length_psd(ConeDev C, ConeState S, const double* __restrict__ dz,
                                                                  const double* __restrict__ ds, double* __restrict__ slots)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    step_length_psd_body<PsdSmall>(C, S, dz, ds, slots, smem);
}
__global__ __launch_bounds__(PsdBig::NT) void k_step_length_psd_big(ConeDev C, ConeState S, const double* __restrict__ dz,
                                                                    const double* __restrict__ ds, double* __restrict__ slots)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    step_length_psd_body<PsdBig>(C, S, dz, ds, slots, smem);
}

// variables_calc_step_length (variables.jl:14-43) without max_step_fraction: min(1, tau limit, kappa limit, cones)
__global__ __launch_bounds__(256) void k_step_length_finish(const double* __restrict__ partial, int np, double step_tau,
                                                            double step_kappa, double tau, double kappa,
                                                            double* __restrict__ rec, Publish P)
{
    __shared__ double sh[256];
    double v = DBL_MAX;
    for (int i = threadIdx.x; i < np; i += 256) v = fmin(v, partial[i]);
    v = block_reduce_256(v, sh, OpMin{});
    if (threadIdx.x == 0) {
        const double at = step_tau < 0.0 ? -tau / step_tau : DBL_MAX;
        const double ak = step_kappa < 0.0 ? -kappa / step_kappa : DBL_MAX;
        rec[0] = fmin(fmin(fmin(at, ak), 1.0), v);
        if (P.dst) st_publish(P);
    }
}

// =====================================================================================================================
//  margins (composite :49-63) and scaled_unit_shift!
// =====================================================================================================================
// one wave per second-order cone (coneops_socone.jl:13-23); pmin / psum: where the cone's two values go
__device__ inline void margins_soc_body(const ConeDev& C, const double* __restrict__ v, double* __restrict__ pmin,
                                        double* __restrict__ psum, int ci, int lane)
{
    const int c = C.soc_list[ci];
    const int off = C.off[c], n = C.numel[c];
    double sq = 0.0;
    for (int i = 1 + lane; i < n; i += 64) sq += v[off + i] * v[off + i];
    sq = st_wave_sum(sq);
    if (lane == 0) {
        const double a = v[off] - sqrt(sq);
        *pmin = a;
        *psum = fmax(0.0, a);
    }
}

__global__ __launch_bounds__(256) void k_margins(ConeDev C, const double* __restrict__ v, int m, double* __restrict__ pmin,
                                                 double* __restrict__ psum, int ge)
{
    __shared__ double sh[256];
    const int bx = blockIdx.x;
    if (bx < ge) {                                                     // coneops_nncone.jl:19-39; zero cone: (floatmax, 0)
        double mn = DBL_MAX, sum = 0.0;
        for (int i = bx * 256 + threadIdx.x; i < m; i += ge * 256) {
            if (C.kind[C.elem_cone[i]] != 1) continue;
            const double x = v[i];
            mn = fmin(mn, x);
            if (x > 0.0) sum += x;
        }
        mn = block_reduce_256(mn, sh, OpMin{});
        sum = block_reduce_256(sum, sh, OpSum{});
        if (threadIdx.x == 0) { pmin[bx] = mn; psum[bx] = sum; }
        return;
    }
    const int ci = (bx - ge) * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ci >= C.nsoc) return;
    margins_soc_body(C, v, pmin + ge + ci, psum + ge + ci, ci, lane);
}

// PSD cones (coneops_psdtrianglecone.jl:8-27): the eigenvalues of mat(v), one matrix in LDS for either class.  The
// cone's workgroup leaves its two values in pmin[blockIdx.x], psum[blockIdx.x].
template <class P>
__device__ inline void margins_psd_body(const ConeDev& C, const double* __restrict__ v, double* __restrict__ pmin,
                                        double* __restrict__ psum, double* smem)
{
    __shared__ double sh[P::NT];
    const int c = P::cone(C);
    const int k = C.psd_dim[c], off = C.off[c];
    if constexpr (!P::kBig) if (k == 0) { if (threadIdx.x == 0) { pmin[blockIdx.x] = DBL_MAX; psum[blockIdx.x] = 0.0; } return; }
    psd_load_mat<P::NT>(smem, v + off, 1.0, k);
    __syncthreads();
    sym_jacobi_eig<P::NT>(smem, k, sh);
    if (threadIdx.x == 0) {
        double mn = DBL_MAX, sum = 0.0;
        for (int i = 0; i < k; ++i) {
            const double e = smem[i + i * k];
            mn = fmin(mn, e);
            if (e > 0.0) sum += e;
        }
        pmin[blockIdx.x] = mn;
        psum[blockIdx.x] = sum;
    }
}
__global__ __launch_bounds__(PsdSmall::NT) void k_margins_psd(ConeDev C, const double* __restrict__ v, double* __restrict__ pmin,
                                                              double* __restrict__ psum)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    margins_psd_body<PsdSmall>(C, v, pmin, psum, smem);
}
__global__ __launch_bounds__(PsdBig::NT) void k_margins_psd_big(ConeDev C, const double* __restrict__ v,
                                                                double* __restrict__ pmin, double* __restrict__ psum)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    margins_psd_body<PsdBig>(C, v, pmin, psum, smem);
}

__global__ __launch_bounds__(256) void k_margins_finish(const double* __restrict__ pmin, const double* __restrict__ psum,
                                                        int np, double* __restrict__ rec, Publish P)
{
    __shared__ double sh[256];
    double mn = DBL_MAX, sum = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) { mn = fmin(mn, pmin[i]); sum += psum[i]; }
    mn = block_reduce_256(mn, sh, OpMin{});
    sum = block_reduce_256(sum, sh, OpSum{});
    if (threadIdx.x == 0) {
        rec[0] = mn;
        rec[1] = sum;
        if (P.dst) st_publish(P);
    }
}

// scaled_unit_shift! of every cone: v += a e (nonnegative: every element, coneops_nncone.jl:42-52; second-order: element 0,
// coneops_socone.jl:26-37; PSD: the diagonal entries, coneops_psdtrianglecone.jl:30-44), a zero cone's rows set to 0 for the
// primal cone.  two: a second shift a2 applied AFTER the first, not their sum (variables.jl:190-191).
__device__ inline void unit_shift_row(const ConeDev& C, double* __restrict__ v, double a1, double a2, int two, int primal, int i)
{
    const int c = C.elem_cone[i];
    const int kind = C.kind[c];
    bool hit;
    if (kind == 0) { if (primal) v[i] = 0.0; return; }
    else if (kind == 1) hit = true;
    else if (kind == 2) hit = i == C.off[c];
    else {
        int r, cl;
        svec_index(i - C.off[c], r, cl);
        hit = r == cl;
    }
    if (!hit) return;
    double x = v[i] + a1;
    if (two) x = x + a2;
    v[i] = x;
}
__global__ __launch_bounds__(256) void k_unit_shift(ConeDev C, double* __restrict__ v, double a1, double a2, int two, int primal,
                                                    int m)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) unit_shift_row(C, v, a1, a2, two, primal, i);
}

// =====================================================================================================================
//  The same operations on a stack of member problems (kernels.hpp: BatchDev): a cone lies in one member, so every
//  per-cone body above runs as it is with the scalars of the cone's member; the elementwise part is cut by member
//  (B.z256: 256 z rows of one member per workgroup), and the finishing kernels fold member b's slots -- its elementwise
//  workgroups', its second-order cones', its PSD cones' -- with wave b.  The minima are order-free; the margins' sums
//  are taken lane-strided in slot order and met in a fixed butterfly.
// =====================================================================================================================
__global__ __launch_bounds__(256) void k_batch_step_ds(ConeDev C, ConeState S, BatchDev B, double* __restrict__ out,
                                                       const double* __restrict__ dz, const double* __restrict__ ds,
                                                       const double* __restrict__ sigma_mu, const double* __restrict__ m_corr,
                                                       int m, int ge)
{
    if ((int)blockIdx.x < ge) {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += ge * 256) {
            const int kind = C.kind[C.elem_cone[i]];
            if (kind == 0) out[i] = 0.0;
            else if (kind == 1) {                                       // (as step_ds_elementwise_body, the member's scalars)
                const int b = B.zmem[i];
                const double l = S.lam[i], w = S.w[i];
                double o = l * l;
                o += (ds[i] / w) * (w * (m_corr[b] * dz[i])) - sigma_mu[b];
                out[i] = o;
            }
        }
        return;
    }
    const int ci = ((int)blockIdx.x - ge) * 4 + (int)(threadIdx.x >> 6);
    if (ci >= C.nsoc) return;
    const int b = B.cone_mem[C.soc_list[ci]];
    step_ds_soc_body(C, S, out, dz, ds, sigma_mu[b], m_corr[b], 1, ci, threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void k_batch_step_ds_psd(ConeDev C, ConeState S, BatchDev B, double* __restrict__ out,
                                                           const double* __restrict__ dz, const double* __restrict__ ds,
                                                           const double* __restrict__ sigma_mu, const double* __restrict__ m_corr)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int c = C.psd_list[blockIdx.x];
    const int b = B.cone_mem[c];
    step_ds_psd_body<PsdSmall>(C, S, out, dz, ds, sigma_mu[b], m_corr[b], 1, c, smem);
}

// slots: [0, nwg) the elementwise workgroups, then a slot per second-order cone
__global__ __launch_bounds__(256) void k_batch_step_length(ConeDev C, BatchDev B, const double* __restrict__ dz,
                                                           const double* __restrict__ ds, const double* __restrict__ z,
                                                           const double* __restrict__ s, double* __restrict__ partial)
{
    __shared__ double sh[256];
    const int ge = B.z256.nwg;
    if ((int)blockIdx.x < ge) {
        const int b = B.z256.wg_mem[blockIdx.x];
        const int i = B.z_off[b] + B.z256.wg_first[blockIdx.x] + (int)threadIdx.x;
        double a = DBL_MAX;
        if (i < B.z_off[b + 1] && C.kind[C.elem_cone[i]] == 1) {        // coneops_nncone.jl:151-170
            const double dzi = dz[i], dsi = ds[i];
            if (dzi < 0.0) a = fmin(a, -z[i] / dzi);
            if (dsi < 0.0) a = fmin(a, -s[i] / dsi);
        }
        a = block_reduce_256(a, sh, OpMin{});
        if (threadIdx.x == 0) partial[blockIdx.x] = a;
        return;
    }
    const int ci = ((int)blockIdx.x - ge) * 4 + (int)(threadIdx.x >> 6);
    if (ci < C.nsoc) step_length_soc_body(C, dz, ds, z, s, partial + ge + ci, ci, threadIdx.x & 63);
}

// lane-strided over member b's three slot ranges, in slot order
template <class F>
__device__ inline void batch_member_slots(const ConeDev& C, const BatchDev& B, int b, int lane, F f)
{
    const int ge = B.z256.nwg;
    for (int i = B.z256.wg_ptr[b] + lane; i < B.z256.wg_ptr[b + 1]; i += 64) f(i);
    for (int i = B.soc_ptr[b] + lane; i < B.soc_ptr[b + 1]; i += 64) f(ge + i);
    for (int i = B.psd_ptr[b] + lane; i < B.psd_ptr[b + 1]; i += 64) f(ge + C.nsoc + i);
}

// wave = member: variables_calc_step_length (variables.jl:14-43) without max_step_fraction, the member's tau and kappa
__global__ __launch_bounds__(256) void k_batch_step_length_finish(ConeDev C, BatchDev B, const double* __restrict__ partial,
                                                                  const double* __restrict__ scal, double* __restrict__ rec)
{
    const int b = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B.nb) return;
    double v = DBL_MAX;
    batch_member_slots(C, B, b, lane, [&](int i) { v = fmin(v, partial[i]); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    if (lane == 0) {
        const double step_tau = scal[b], step_kappa = scal[B.nb + b], tau = scal[2 * B.nb + b], kappa = scal[3 * B.nb + b];
        const double at = step_tau < 0.0 ? -tau / step_tau : DBL_MAX;
        const double ak = step_kappa < 0.0 ? -kappa / step_kappa : DBL_MAX;
        rec[b] = fmin(fmin(fmin(at, ak), 1.0), v);
    }
}

__global__ __launch_bounds__(256) void k_batch_margins(ConeDev C, BatchDev B, const double* __restrict__ v, double* __restrict__ pmin,
                                                       double* __restrict__ psum)
{
    __shared__ double sh[256];
    const int ge = B.z256.nwg;
    if ((int)blockIdx.x < ge) {                                         // coneops_nncone.jl:19-39; zero cone: (floatmax, 0)
        const int b = B.z256.wg_mem[blockIdx.x];
        const int i = B.z_off[b] + B.z256.wg_first[blockIdx.x] + (int)threadIdx.x;
        double mn = DBL_MAX, sum = 0.0;
        if (i < B.z_off[b + 1] && C.kind[C.elem_cone[i]] == 1) {
            const double x = v[i];
            mn = fmin(mn, x);
            if (x > 0.0) sum += x;
        }
        mn = block_reduce_256(mn, sh, OpMin{});
        sum = block_reduce_256(sum, sh, OpSum{});
        if (threadIdx.x == 0) { pmin[blockIdx.x] = mn; psum[blockIdx.x] = sum; }
        return;
    }
    const int ci = ((int)blockIdx.x - ge) * 4 + (int)(threadIdx.x >> 6);
    if (ci < C.nsoc) margins_soc_body(C, v, pmin + ge + ci, psum + ge + ci, ci, threadIdx.x & 63);
}

// wave = member: (min_margin, pos_margin) into rec, and the member's branch of _shift_to_cone_interior!
// (variables.jl:186-204) as (a1, a2, two) into shift
__global__ __launch_bounds__(256) void k_batch_margins_finish(ConeDev C, BatchDev B, const double* __restrict__ pmin,
                                                              const double* __restrict__ psum, double* __restrict__ rec,
                                                              double* __restrict__ shift)
{
    const int b = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B.nb) return;
    double mn = DBL_MAX, sum = 0.0;
    batch_member_slots(C, B, b, lane, [&](int i) { mn = fmin(mn, pmin[i]); sum += psum[i]; });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mn = fmin(mn, __shfl_xor(mn, o, 64)); sum += __shfl_xor(sum, o, 64); }
    if (lane == 0) {
        rec[2 * b] = mn;
        rec[2 * b + 1] = sum;
        const double degree = B.degree[b];
        const double target = degree > 0.0 ? fmax(1.0, 0.1 * sum / degree) : 1.0;
        double a1 = 0.0, a2 = 0.0, two = 0.0;
        if (mn <= 0.0) { a1 = -mn; a2 = target; two = 1.0; }
        else if (mn < target) a1 = target - mn;
        shift[3 * b] = a1;
        shift[3 * b + 1] = a2;
        shift[3 * b + 2] = two;
    }
}

__global__ __launch_bounds__(256) void k_batch_unit_shift(ConeDev C, BatchDev B, double* __restrict__ v,
                                                          const double* __restrict__ shift, int primal, int m)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) {
        const double* sp = shift + 3 * B.zmem[i];
        unit_shift_row(C, v, sp[0], sp[1], sp[2] != 0.0, primal, i);
    }
}

// =====================================================================================================================
//  Exponential and power cones between the solves (coneops_nonsymmetric_common.jl, coneops_expcone.jl,
//  coneops_powcone.jl).  One LANE per cone: lane j takes the handle's j-th exponential cone, lanes from nexp on its
//  power cones, so that neighbouring lanes run the same branch; a cone is three rows and a few dozen to a few hundred
//  scalar fp64 operations (log / exp / pow cost ~100 instructions each and dominate; there is nothing to share between
//  lanes).  Lanes that backtrack or iterate different numbers of times diverge.  Per-workgroup minima and sums go to
//  slots that one workgroup folds in a fixed order.
// =====================================================================================================================
constexpr double kSqrtEps = 1.4901161193847656e-08;                    // sqrt(eps(Float64)) = 2^-26

__device__ inline int ns_lane_cone(const ConeDev& C, int j, bool& is_pow)
{
    is_pow = j >= C.nexp;
    return is_pow ? C.pow_list[j - C.nexp] : C.exp_list[j];
}

// cholesky_3x3_explicit_factor! (mathutils.jl:427-451) of a row-major symmetric A; L = (l00, l10, l11, l20, l21, l22)
__device__ inline bool ns_chol3_factor(const double* A, double* L)
{
    double t = A[0];
    if (!(t > 0.0)) return false;
    L[0] = sqrt(t);
    L[1] = A[3] / L[0];
    t = A[4] - L[1] * L[1];
    if (!(t > 0.0)) return false;
    L[2] = sqrt(t);
    L[3] = A[6] / L[0];
    L[4] = (A[7] - L[1] * L[3]) / L[2];
    t = A[8] - L[3] * L[3] - L[4] * L[4];
    if (!(t > 0.0)) return false;
    L[5] = sqrt(t);
    return true;
}

// cholesky_3x3_explicit_solve! (mathutils.jl:455-466)
__device__ inline void ns_chol3_solve(const double* L, const double* b, double* x)
{
    const double l00 = L[0], l10 = L[1], l11 = L[2], l20 = L[3], l21 = L[4], l22 = L[5];
    const double c1 = b[0] / l00;
    const double c2 = (b[1] * l00 - b[0] * l10) / (l00 * l11);
    const double c3 = (b[2] * l00 * l11 - b[1] * l00 * l21 + b[0] * l10 * l21 - b[0] * l11 * l20) / (l00 * l11 * l22);
    x[0] = (c1 * l11 * l22 - c2 * l10 * l22 + c3 * l10 * l21 - c3 * l11 * l20) / (l00 * l11 * l22);
    x[1] = (c2 * l22 - c3 * l21) / (l11 * l22);
    x[2] = c3 / l22;
}

// higher_correction! of the exponential cone (coneops_expcone.jl:319-366): eta = +1/2 D^3 f*(z)[u, v], u = H*^{-1} ds, which
// combined_ds_shift! subtracts
__device__ inline void ns_exp_higher_correction(const double* z, const double* u, const double* v, double* eta)
{
    eta[1] = 1.0;
    eta[2] = -z[0] / z[2];
    eta[0] = ns_logsafe(eta[2]);
    const double psi = z[0] * eta[0] - z[0] + z[1];
    const double dpu = eta[0] * u[0] + eta[1] * u[1] + eta[2] * u[2];
    const double dpv = eta[0] * v[0] + eta[1] * v[1] + eta[2] * v[2];
    const double coef = ((u[0] * (v[0] / z[0] - v[2] / z[2]) + u[2] * (z[0] * v[2] / z[2] - v[0]) / z[2]) * psi - 2.0 * dpu * dpv)
                        / (psi * psi * psi);
    for (int i = 0; i < 3; ++i) eta[i] *= coef;
    const double ip2 = 1.0 / psi / psi;
    eta[0] += (1.0 / psi - 2.0 / z[0]) * u[0] * v[0] / (z[0] * z[0]) - u[2] * v[2] / (z[2] * z[2]) / psi
              + dpu * ip2 * (v[0] / z[0] - v[2] / z[2]) + dpv * ip2 * (u[0] / z[0] - u[2] / z[2]);
    eta[2] += 2.0 * (z[0] / psi - 1.0) * u[2] * v[2] / (z[2] * z[2] * z[2]) - (u[2] * v[0] + u[0] * v[2]) / (z[2] * z[2]) / psi
              + dpu * ip2 * (z[0] * v[2] / (z[2] * z[2]) - v[0] / z[2]) + dpv * ip2 * (z[0] * u[2] / (z[2] * z[2]) - u[0] / z[2]);
    for (int i = 0; i < 3; ++i) eta[i] /= 2.0;
}

// ... of the power cone (coneops_powcone.jl:329-404)
__device__ inline void ns_pow_higher_correction(const double* z, double a, const double* u, const double* v, double* out)
{
    const double phi = pow(z[0] / a, 2.0 * a) * pow(z[1] / (1.0 - a), 2.0 - 2.0 * a);
    const double psi = phi - z[2] * z[2];
    const double eta[3] = {2.0 * a * phi / z[0], 2.0 * (1.0 - a) * phi / z[1], -2.0 * z[2]};
    const double H11 = 2.0 * a * (2.0 * a - 1.0) * phi / (z[0] * z[0]);
    const double H12 = 4.0 * a * (1.0 - a) * phi / (z[0] * z[1]);
    const double H22 = 2.0 * (1.0 - a) * (1.0 - 2.0 * a) * phi / (z[1] * z[1]);
    const double dpu = eta[0] * u[0] + eta[1] * u[1] + eta[2] * u[2];
    const double dpv = eta[0] * v[0] + eta[1] * v[1] + eta[2] * v[2];
    const double Hv[3] = {H11 * v[0] + H12 * v[1], H12 * v[0] + H22 * v[1], -2.0 * v[2]};
    const double coef = ((u[0] * Hv[0] + u[1] * Hv[1] + u[2] * Hv[2]) * psi - 2.0 * dpu * dpv) / (psi * psi * psi);
    const double coef2 = 4.0 * a * (2.0 * a - 1.0) * (1.0 - a) * phi * (u[0] / z[0] - u[1] / z[1]) * (v[0] / z[0] - v[1] / z[1]) / psi;
    const double ip2 = 1.0 / psi / psi;
    const double e0 = coef * eta[0] - 2.0 * (1.0 - a) * u[0] * v[0] / (z[0] * z[0] * z[0]) + coef2 / z[0] + Hv[0] * dpu * ip2;
    const double e1 = coef * eta[1] - 2.0 * a * u[1] * v[1] / (z[1] * z[1] * z[1]) - coef2 / z[1] + Hv[1] * dpu * ip2;
    const double e2 = coef * eta[2] + Hv[2] * dpu * ip2;
    const double Hu[3] = {H11 * u[0] + H12 * u[1], H12 * u[0] + H22 * u[1], -2.0 * u[2]};
    out[0] = (e0 + Hu[0] * dpv * ip2) / 2.0;
    out[1] = (e1 + Hu[1] * dpv * ip2) / 2.0;
    out[2] = (e2 + Hu[2] * dpv * ip2) / 2.0;
}

// affine_ds! (coneops_expcone.jl:117-127, coneops_powcone.jl:120-130: a copy of s) and, with `combined`, the cone's d.s of the combined step:
// s + sigma_mu grad f*(z) - eta(step_s, m_corr step_z), grad and H*(z) as the scaling kernel stored them; eta = 0 where
// the 3 x 3 factorisation fails
__global__ __launch_bounds__(256) void k_ns_ds(ConeDev C, ConeState S, double* __restrict__ out, const double* __restrict__ dz,
                                               const double* __restrict__ ds, const double* __restrict__ s,
                                               const double* __restrict__ z, double sigma_mu, double m_corr, int combined)
{
    const int nns = C.nexp + C.npow;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < nns; j += gridDim.x * 256) {
        bool is_pow;
        const int c = ns_lane_cone(C, j, is_pow);
        const int off = C.off[c];
        const double sv[3] = {s[off], s[off + 1], s[off + 2]};
        if (!combined) {
            for (int i = 0; i < 3; ++i) out[off + i] = sv[i];
            continue;
        }
        const int k = C.ns_index[c];
        const double* grad = S.ns_grad + 3 * k;
        double H[9], L[6], eta[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < 9; ++i) H[i] = S.ns_H[9 * k + i];
        if (ns_chol3_factor(H, L)) {
            const double zv[3] = {z[off], z[off + 1], z[off + 2]};
            const double dsv[3] = {ds[off], ds[off + 1], ds[off + 2]};
            const double v[3] = {m_corr * dz[off], m_corr * dz[off + 1], m_corr * dz[off + 2]};
            double u[3];
            ns_chol3_solve(L, dsv, u);
            if (is_pow) ns_pow_higher_correction(zv, C.param[c], u, v, eta);
            else ns_exp_higher_correction(zv, u, v, eta);
        }
        for (int i = 0; i < 3; ++i) out[off + i] = sv[i] + (grad[i] * sigma_mu - eta[i]);
    }
}

// is_primal_feasible / is_dual_feasible (coneops_expcone.jl:253-281, coneops_powcone.jl:256-286); a NaN point fails
// every comparison: it is not in the cone
__device__ inline bool ns_exp_primal_feasible(const double* s)
{
    return s[2] > 0.0 && s[1] > 0.0 && s[1] * ns_logsafe(s[2] / s[1]) - s[0] > 0.0;
}
__device__ inline bool ns_exp_dual_feasible(const double* z)
{
    return z[2] > 0.0 && z[0] < 0.0 && z[1] - z[0] - z[0] * ns_logsafe(-z[2] / z[0]) > 0.0;
}
__device__ inline bool ns_pow_primal_feasible(const double* s, double a)
{
    return s[0] > 0.0 && s[1] > 0.0 && exp(2.0 * a * ns_logsafe(s[0]) + 2.0 * (1.0 - a) * ns_logsafe(s[1])) - s[2] * s[2] > 0.0;
}
__device__ inline bool ns_pow_dual_feasible(const double* z, double a)
{
    return z[0] > 0.0 && z[1] > 0.0
           && exp(2.0 * a * ns_logsafe(z[0] / a) + 2.0 * (1.0 - a) * ns_logsafe(z[1] / (1.0 - a))) - z[2] * z[2] > 0.0;
}

// backtrack_search (coneops_nonsymmetric_common.jl:5-34) from alpha = a: the values visited are a step^j by repeated
// multiplication.  `cap` bounds the trips whatever the input (a NaN alpha never drops below alpha_min): the result is then 0.
template <class F>
__device__ inline double ns_backtrack(const double* q, const double* dq, double a, double amin, double step, int cap, F in_cone)
{
    for (int trip = 0; trip < cap; ++trip) {
        const double p[3] = {q[0] + a * dq[0], q[1] + a * dq[1], q[2] + a * dq[2]};
        if (in_cone(p)) return a;
        a *= step;
        if (a < amin) return 0.0;
    }
    return 0.0;
}

// Stage 2 and 3 of the composite step length (coneops_compositecone.jl:205-243): every cone backtracks on z and on s
// from the common start a0 = min(rec[0], 1 - sqrt(eps)), rec[0] being what k_step_length_finish left on the device.
__global__ __launch_bounds__(256) void k_ns_step_length(ConeDev C, const double* __restrict__ dz, const double* __restrict__ ds,
                                                        const double* __restrict__ z, const double* __restrict__ s,
                                                        const double* __restrict__ rec, double step, double amin, int cap,
                                                        double* __restrict__ partial)
{
    __shared__ double sh[256];
    const double a0 = fmin(rec[0], 1.0 - kSqrtEps);
    const int nns = C.nexp + C.npow;
    double amine = a0;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < nns; j += gridDim.x * 256) {
        bool is_pow;
        const int c = ns_lane_cone(C, j, is_pow);
        const int off = C.off[c];
        const double zv[3] = {z[off], z[off + 1], z[off + 2]}, dzv[3] = {dz[off], dz[off + 1], dz[off + 2]};
        const double sv[3] = {s[off], s[off + 1], s[off + 2]}, dsv[3] = {ds[off], ds[off + 1], ds[off + 2]};
        double az, as;
        if (is_pow) {
            const double a = C.param[c];
            az = ns_backtrack(zv, dzv, a0, amin, step, cap, [a](const double* p) { return ns_pow_dual_feasible(p, a); });
            as = ns_backtrack(sv, dsv, a0, amin, step, cap, [a](const double* p) { return ns_pow_primal_feasible(p, a); });
        } else {
            az = ns_backtrack(zv, dzv, a0, amin, step, cap, [](const double* p) { return ns_exp_dual_feasible(p); });
            as = ns_backtrack(sv, dsv, a0, amin, step, cap, [](const double* p) { return ns_exp_primal_feasible(p); });
        }
        amine = fmin(amine, fmin(az, as));
    }
    amine = block_reduce_256(amine, sh, OpMin{});
    if (threadIdx.x == 0) partial[blockIdx.x] = amine;
}

__global__ __launch_bounds__(256) void k_ns_step_length_finish(const double* __restrict__ partial, int np, double* __restrict__ rec,
                                                               Publish P)
{
    __shared__ double sh[256];
    double v = DBL_MAX;
    for (int i = threadIdx.x; i < np; i += 256) v = fmin(v, partial[i]);
    v = block_reduce_256(v, sh, OpMin{});
    if (threadIdx.x == 0) {
        rec[0] = fmin(fmin(rec[0], 1.0 - kSqrtEps), v);
        if (P.dst) st_publish(P);
    }
}

// ---- compute_barrier at (z + alpha dz, s + alpha ds)
// barrier_dual + barrier_primal (coneops_expcone.jl:189-251, coneops_powcone.jl:193-254)
__device__ inline double ns_exp_barrier(const double* z, const double* s)
{
    const double l = ns_logsafe(-z[2] / z[0]);
    const double dual = -ns_logsafe(-z[2] * z[0]) - ns_logsafe(z[1] - z[0] - z[0] * l);
    double w = ns_wright_omega(1.0 - s[0] / s[1] - ns_logsafe(s[1] / s[2]));
    w = (w - 1.0) * (w - 1.0) / w;
    const double primal = -ns_logsafe(w) - 2.0 * ns_logsafe(s[1]) - ns_logsafe(s[2]) - 3.0;
    return dual + primal;
}
__device__ inline double ns_pow_barrier(const double* z, const double* s, double a)
{
    const double dual = -ns_logsafe(pow(z[0] / a, 2.0 * a) * pow(z[1] / (1.0 - a), 2.0 - 2.0 * a) - z[2] * z[2])
                        - (1.0 - a) * ns_logsafe(z[0]) - a * ns_logsafe(z[1]);
    double g[3];
    ns_pow_gradient_primal(s, a, g);
    const double primal = ns_logsafe(pow(-g[0] / a, 2.0 * a) * pow(-g[1] / (1.0 - a), 2.0 - 2.0 * a) - g[2] * g[2])
                          + (1.0 - a) * ns_logsafe(-g[0]) + a * ns_logsafe(-g[1]) - 3.0;
    return dual + primal;
}

// Workgroups below ge: <z + alpha dz, s + alpha ds> over ALL rows and the nonnegative cones' barrier
// (coneops_nncone.jl:172-189); behind them one wave per second-order cone (coneops_socone.jl:287-305).
__global__ __launch_bounds__(256) void k_barrier(ConeDev C, const double* __restrict__ z, const double* __restrict__ s,
                                                 const double* __restrict__ dz, const double* __restrict__ ds, double alpha, int m,
                                                 double* __restrict__ pbar, double* __restrict__ pdot, int ge)
{
    __shared__ double sh[256];
    const int bx = blockIdx.x;
    if (bx < ge) {
        double bar = 0.0, dot = 0.0;
        for (int i = bx * 256 + threadIdx.x; i < m; i += ge * 256) {
            const double zi = z[i] + alpha * dz[i], si = s[i] + alpha * ds[i];
            dot += zi * si;
            if (C.kind[C.elem_cone[i]] == 1) bar -= ns_logsafe(si * zi);
        }
        bar = block_reduce_256(bar, sh, OpSum{});
        dot = block_reduce_256(dot, sh, OpSum{});
        if (threadIdx.x == 0) { pbar[bx] = bar; pdot[bx] = dot; }
        return;
    }
    const int ci = (bx - ge) * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ci >= C.nsoc) return;
    const int c = C.soc_list[ci];
    const int off = C.off[c], n = C.numel[c];
    double sq_s = 0.0, sq_z = 0.0;
    for (int i = 1 + lane; i < n; i += 64) {
        const double zi = z[off + i] + alpha * dz[off + i], si = s[off + i] + alpha * ds[off + i];
        sq_z += zi * zi;
        sq_s += si * si;
    }
    sq_z = sqrt(st_wave_sum(sq_z));
    sq_s = sqrt(st_wave_sum(sq_s));
    if (lane == 0) {
        const double z0 = z[off] + alpha * dz[off], s0 = s[off] + alpha * ds[off];
        const double rz = (z0 - sq_z) * (z0 + sq_z), rs = (s0 - sq_s) * (s0 + sq_s);        // _soc_residual, :415-419
        pbar[ge + ci] = (rs > 0.0 && rz > 0.0) ? -ns_logsafe(rs * rz) / 2.0 : HUGE_VAL;
    }
}

// PSD cones (coneops_psdtrianglecone.jl:256-295): -logdet of mat(z + alpha dz) and of mat(s + alpha ds) by psd_cholesky
// in LDS (k x k doubles, either class), +inf where one fails
template <class P>
__device__ inline void barrier_psd_body(const ConeDev& C, const double* __restrict__ z, const double* __restrict__ s,
                                        const double* __restrict__ dz, const double* __restrict__ ds, double alpha,
                                        double* __restrict__ slots, double* X)
{
    __shared__ int sh_fail;
    const int tid = threadIdx.x;
    const int c = P::cone(C);
    const int k = C.psd_dim[c], off = C.off[c], t = k * (k + 1) / 2;
    if constexpr (!P::kBig) if (k == 0) { if (tid == 0) slots[blockIdx.x] = 0.0; return; }
    if (tid == 0) sh_fail = 0;
    double bar = 0.0;                                                  // (thread 0's)
    for (int comp = 0; comp < 2; ++comp) {
        const double* x = (comp == 0 ? z : s) + off;
        const double* dx = (comp == 0 ? dz : ds) + off;
        for (int idx = tid; idx < t; idx += P::NT) {
            int r, cl;
            svec_index(idx, r, cl);
            const double v = (x[idx] + alpha * dx[idx]) * (r == cl ? 1.0 : kIs2);
            X[r + cl * k] = v;
            X[cl + r * k] = v;
        }
        __syncthreads();
        psd_cholesky<P::NT>(X, k, &sh_fail, [&](double sd) { bar -= 2.0 * log(sd); });
        if (sh_fail) break;
    }
    if (tid == 0) slots[blockIdx.x] = sh_fail ? HUGE_VAL : bar;
}
__global__ __launch_bounds__(PsdSmall::NT) void k_barrier_psd(ConeDev C, const double* __restrict__ z, const double* __restrict__ s,
                                                              const double* __restrict__ dz, const double* __restrict__ ds,
                                                              double alpha, double* __restrict__ slots)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    barrier_psd_body<PsdSmall>(C, z, s, dz, ds, alpha, slots, smem);
}
__global__ __launch_bounds__(PsdBig::NT) void k_barrier_psd_big(ConeDev C, const double* __restrict__ z,
                                                                const double* __restrict__ s, const double* __restrict__ dz,
                                                                const double* __restrict__ ds, double alpha,
                                                                double* __restrict__ slots)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    barrier_psd_body<PsdBig>(C, z, s, dz, ds, alpha, slots, smem);
}

__global__ __launch_bounds__(256) void k_barrier_ns(ConeDev C, const double* __restrict__ z, const double* __restrict__ s,
                                                    const double* __restrict__ dz, const double* __restrict__ ds, double alpha,
                                                    double* __restrict__ slots)
{
    __shared__ double sh[256];
    const int nns = C.nexp + C.npow;
    double bar = 0.0;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < nns; j += gridDim.x * 256) {
        bool is_pow;
        const int c = ns_lane_cone(C, j, is_pow);
        const int off = C.off[c];
        const double zv[3] = {z[off] + alpha * dz[off], z[off + 1] + alpha * dz[off + 1], z[off + 2] + alpha * dz[off + 2]};
        const double sv[3] = {s[off] + alpha * ds[off], s[off + 1] + alpha * ds[off + 1], s[off + 2] + alpha * ds[off + 2]};
        bar += is_pow ? ns_pow_barrier(zv, sv, C.param[c]) : ns_exp_barrier(zv, sv);
    }
    bar = block_reduce_256(bar, sh, OpSum{});
    if (threadIdx.x == 0) slots[blockIdx.x] = bar;
}

// rec = (sum of the nbar barrier slots, sum of the first ndot dot-product slots), each lane its strided slots in ascending
// order, then the fixed tree
__global__ __launch_bounds__(256) void k_barrier_finish(const double* __restrict__ pbar, int nbar, const double* __restrict__ pdot,
                                                        int ndot, double* __restrict__ rec, Publish P)
{
    __shared__ double sh[256];
    double bar = 0.0, dot = 0.0;
    for (int i = threadIdx.x; i < nbar; i += 256) bar += pbar[i];
    for (int i = threadIdx.x; i < ndot; i += 256) dot += pdot[i];
    bar = block_reduce_256(bar, sh, OpSum{});
    dot = block_reduce_256(dot, sh, OpSum{});
    if (threadIdx.x == 0) {
        rec[0] = bar;
        rec[1] = dot;
        if (P.dst) st_publish(P);
    }
}

// unit_initialization! of every cone into s and z (zero: 0; nonnegative: 1; second-order: e_1; PSD: svec(I);
// exponential: coneops_expcone.jl:36-52; power: coneops_powcone.jl:36-54)
__global__ __launch_bounds__(256) void k_unit_initialization(ConeDev C, double* __restrict__ s, double* __restrict__ z, int m)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) {
        const int c = C.elem_cone[i];
        const int kind = C.kind[c], j = i - C.off[c];
        double v = 0.0;
        if (kind == 1) v = 1.0;
        else if (kind == 2) v = j == 0 ? 1.0 : 0.0;
        else if (kind == 3) {
            int r, cl;
            svec_index(j, r, cl);
            v = r == cl ? 1.0 : 0.0;
        } else if (kind == 4) v = j == 0 ? -1.051383945322714 : j == 1 ? 0.556409619469370 : 1.258967884768947;
        else if (kind == 5) {
            const double a = C.param[c];
            v = j == 0 ? sqrt(1.0 + a) : j == 1 ? sqrt(1.0 + (1.0 - a)) : 0.0;
        }
        s[i] = v;
        z[i] = v;
    }
}

// =====================================================================================================================
//  Generalized power cones between the solves (coneops_genpowcone.jl), with the scaling kernel's work split
//  (kernels.hip, cone_genpow_body): NT = 64, one wave per cone of gp_small, four to a workgroup; NT = 256, one workgroup
//  per cone of gp_big.  Every sum is reduced in a fixed order -- a lane its strided rows in ascending order, a butterfly
//  over the lanes, the waves left to right through LDS -- and every thread of the cone's wave / workgroup receives the
//  same bits, so the data-dependent loops below (backtracking, Newton) take the same turn in every thread: no barrier
//  sits under a branch that can differ between the threads of a workgroup.  DESIGN.md 4.4b.
// =====================================================================================================================
constexpr double kEps = 2.220446049250313e-16;
constexpr int kGpRedMax = 6;                                           // values per reduction; LDS: 4 waves x kGpRedMax

// v[0..N) summed over the cone's threads (v[0] multiplied where PROD0).  NT = 256: two barriers, so that a caller's loop
// may come back before a slow wave has read the slots.
template <int NT, int N, bool PROD0>
__device__ inline void gpst_reduce(double (&v)[N], double* sh)
{
    static_assert(N <= kGpRedMax, "LDS slots");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double t = __shfl_xor(v[j], o, 64);
            v[j] = (PROD0 && j == 0) ? v[j] * t : v[j] + t;
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = __shfl(v[j], 0, 64);              // (the butterfly's sums commute: the same bits already)
    if (NT > 64) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0)
            for (int j = 0; j < N; ++j) sh[N * wave + j] = v[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < N; ++j)
            v[j] = (PROD0 && j == 0) ? (sh[j] * sh[N + j]) * (sh[2 * N + j] * sh[3 * N + j])
                                     : (sh[j] + sh[N + j]) + (sh[2 * N + j] + sh[3 * N + j]);
        __syncthreads();
    }
}

struct GpCone { int off, n, d1; const double* al; int g; };
__device__ inline GpCone gp_cone_of(const ConeDev& C, int k)
{
    const int c = C.gp_cone[k];
    return GpCone{C.off[c], C.numel[c], C.gp_dim1[k], C.gp_alpha + C.gp_off[k], C.gp_off[k]};
}

// mode 0: unit_initialization! (:34-53) into out and out2; 1: affine_ds! (:137-147), a copy of s; 2: the combined step's
// d.s (:149-168), s + sigma_mu grad f*(z) with the gradient the scaling kernel stored (no higher-order correction)
template <int NT>
__device__ inline void gp_rows_body(const ConeDev& C, const ConeState& S, int k, int tid, int mode, double* __restrict__ out,
                                    double* __restrict__ out2, const double* __restrict__ s, double sigma_mu)
{
    const GpCone G = gp_cone_of(C, k);
    for (int i = tid; i < G.n; i += NT) {
        if (mode == 0) {
            const double v = i < G.d1 ? sqrt(1.0 + G.al[i]) : 0.0;
            out[G.off + i] = v;
            out2[G.off + i] = v;
        } else if (mode == 1) out[G.off + i] = s[G.off + i];
        else out[G.off + i] = s[G.off + i] + sigma_mu * S.gp_grad[G.g + i];
    }
}

__global__ __launch_bounds__(256) void k_gp_rows(ConeDev C, ConeState S, int mode, double* __restrict__ out, double* __restrict__ out2,
                                                 const double* __restrict__ s, double sigma_mu)
{
    const int gq = (C.ngp_small + 3) / 4, bx = (int)blockIdx.x;
    if (bx < gq) {
        const int i = bx * 4 + (int)(threadIdx.x >> 6);
        if (i < C.ngp_small) gp_rows_body<64>(C, S, C.gp_small[i], threadIdx.x & 63, mode, out, out2, s, sigma_mu);
        return;
    }
    gp_rows_body<256>(C, S, C.gp_big[bx - gq], threadIdx.x, mode, out, out2, s, sigma_mu);
}

// backtrack_search (coneops_nonsymmetric_common.jl:5-34) of one cone from a with is_dual_feasible (scaled, :272-292) or
// is_primal_feasible (:249-269): the first dim1 entries > 0 and exp(sum 2 alpha_i logsafe(v_i [/ alpha_i])) - ||v[dim1:]||^2 > 0.
// A NaN entry fails its comparison: the point is not in the cone.  At most `cap` trips.
template <int NT>
__device__ inline double gp_backtrack(const GpCone& G, const double* __restrict__ q, const double* __restrict__ dq, double a,
                                      double amin, double step, int cap, bool scaled, int tid, double* sh)
{
    for (int trip = 0; trip < cap; ++trip) {
        double v[3] = {0.0, 0.0, 0.0};                                 // sum of logs, sum of squares, entries not > 0
        for (int i = tid; i < G.n; i += NT) {
            const double x = q[G.off + i] + a * dq[G.off + i];
            if (i < G.d1) {
                const double al = G.al[i];
                if (!(x > 0.0)) v[2] += 1.0;
                v[0] += 2.0 * al * ns_logsafe(scaled ? x / al : x);
            } else v[1] += x * x;
        }
        gpst_reduce<NT, 3, false>(v, sh);
        if (v[2] == 0.0 && exp(v[0]) - v[1] > 0.0) return a;
        a *= step;
        if (a < amin) return 0.0;
    }
    return 0.0;
}

template <int NT>
__device__ inline void gp_step_length_body(const ConeDev& C, int k, int tid, const double* __restrict__ dz,
                                           const double* __restrict__ ds, const double* __restrict__ z, const double* __restrict__ s,
                                           double a0, double step, double amin, int cap, double* __restrict__ slot, double* sh)
{
    const GpCone G = gp_cone_of(C, k);
    const double az = gp_backtrack<NT>(G, z, dz, a0, amin, step, cap, true, tid, sh);
    const double as = gp_backtrack<NT>(G, s, ds, a0, amin, step, cap, false, tid, sh);
    if (tid == 0) *slot = fmin(az, as);
}

// slot k (the cone's index among the generalized power cones) = the cone's limit, from the common start a0 (k_ns_step_length)
__global__ __launch_bounds__(256) void k_gp_step_length(ConeDev C, const double* __restrict__ dz, const double* __restrict__ ds,
                                                        const double* __restrict__ z, const double* __restrict__ s,
                                                        const double* __restrict__ rec, double step, double amin, int cap,
                                                        double* __restrict__ slots)
{
    __shared__ double sh[4 * kGpRedMax];
    const double a0 = fmin(rec[0], 1.0 - kSqrtEps);
    const int gq = (C.ngp_small + 3) / 4, bx = (int)blockIdx.x;
    if (bx < gq) {
        const int i = bx * 4 + (int)(threadIdx.x >> 6);
        if (i < C.ngp_small) {
            const int k = C.gp_small[i];
            gp_step_length_body<64>(C, k, threadIdx.x & 63, dz, ds, z, s, a0, step, amin, cap, slots + k, nullptr);
        }
        return;
    }
    const int k = C.gp_big[bx - gq];
    gp_step_length_body<256>(C, k, threadIdx.x, dz, ds, z, s, a0, step, amin, cap, slots + k, sh);
}

// compute_barrier (:209-234) of one cone at (z + alpha dz, s + alpha ds): barrier_dual(z') (:313-333) +
// barrier_primal(s') = -barrier_dual(-g(s')) - (dim1 + 1), g = gradient_primal! (:393-426) with the one-dimensional Newton
// iteration of ipm._newton_raphson_genpowcone (:437-472; the start halved at most 64 times until f0 > 0, then at most 100
// one-sided steps with the three stop tests of coneops_nonsymmetric_common.jl:170-193).  Every comparison that keeps a
// loop running is false for NaN.
template <int NT>
__device__ inline void gp_barrier_body(const ConeDev& C, int k, int tid, const double* __restrict__ z, const double* __restrict__ s,
                                       const double* __restrict__ dz, const double* __restrict__ ds, double alpha,
                                       double* __restrict__ slot, double* sh)
{
    const GpCone G = gp_cone_of(C, k);
    // one pass: the dual barrier's three sums, and of s': phi = prod s_i^(2 alpha_i), ||r||^2, sum alpha_i^2
    double v[6] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < G.n; i += NT) {
        const double zi = z[G.off + i] + alpha * dz[G.off + i], si = s[G.off + i] + alpha * ds[G.off + i];
        if (i < G.d1) {
            const double al = G.al[i];
            v[0] *= pow(si, 2.0 * al);
            v[1] += 2.0 * al * ns_logsafe(zi / al);
            v[2] += (1.0 - al) * ns_logsafe(zi);
            v[5] += al * al;
        } else {
            v[3] += zi * zi;
            v[4] += si * si;
        }
    }
    gpst_reduce<NT, 6, true>(v, sh);
    const double dual = -ns_logsafe(exp(v[1]) - v[3]) - v[2];
    const double phi = v[0], nr = sqrt(v[4]), psi = 1.0 / v[5];
    double g1 = 0.0;
    const bool newton = nr > kEps;
    if (newton) {
        double x = -1.0 / nr + (psi * nr + sqrt((phi / nr / nr + psi * psi - 1.0) * phi)) / (phi - nr * nr);
        double f[2];
        // f0(x) and f1(x) in one pass
        auto eval = [&](double y) {
            f[0] = 0.0; f[1] = 0.0;
            for (int i = tid; i < G.d1; i += NT) {
                const double al = G.al[i], pi = s[G.off + i] + alpha * ds[G.off + i];
                const double t = (1.0 + al) / al;
                f[0] += 2.0 * al * (ns_logsafe(y * nr + t) - ns_logsafe(pi));
                f[1] += 2.0 * al * nr / (nr * y + t);
            }
            gpst_reduce<NT, 2, false>(f, sh);
            f[0] = -ns_logsafe(2.0 * y / nr + y * y) + f[0];
            f[1] = -(2.0 * y + 2.0 / nr) / (y * y + 2.0 * y / nr) + f[1];
        };
        eval(x);
        for (int h = 0; h < 64 && f[0] <= 0.0; ++h) {
            x *= 0.5;
            eval(x);
        }
        for (int iter = 0; iter < 100; ++iter) {
            const double dfdx = f[1];
            const double dx = -f[0] / dfdx;
            if (!(dx >= kEps) || !(fabs(dx / x) >= kSqrtEps) || !(fabs(dfdx) >= kEps)) break;
            x += dx;
            if (iter + 1 < 100) eval(x);
        }
        g1 = x;
    }
    // barrier_dual(-g): -g_i = (1 + alpha_i + alpha_i g1 ||r||) / p_i, -g_w = -g1 r / ||r||
    double w[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < G.n; i += NT) {
        const double si = s[G.off + i] + alpha * ds[G.off + i];
        if (i < G.d1) {
            const double al = G.al[i];
            const double g = newton ? -(1.0 + al + al * g1 * nr) / si : -(1.0 + al) / si;
            w[0] += 2.0 * al * ns_logsafe(-g / al);
            w[2] += (1.0 - al) * ns_logsafe(-g);
        } else {
            const double g = newton ? g1 * si / nr : 0.0;
            w[1] += g * g;
        }
    }
    gpst_reduce<NT, 3, false>(w, sh);
    const double primal = -(-ns_logsafe(exp(w[0]) - w[1]) - w[2]) - (double)(G.d1 + 1);
    if (tid == 0) *slot = dual + primal;
}

__global__ __launch_bounds__(256) void k_gp_barrier(ConeDev C, const double* __restrict__ z, const double* __restrict__ s,
                                                    const double* __restrict__ dz, const double* __restrict__ ds, double alpha,
                                                    double* __restrict__ slots)
{
    __shared__ double sh[4 * kGpRedMax];
    const int gq = (C.ngp_small + 3) / 4, bx = (int)blockIdx.x;
    if (bx < gq) {
        const int i = bx * 4 + (int)(threadIdx.x >> 6);
        if (i < C.ngp_small) {
            const int k = C.gp_small[i];
            gp_barrier_body<64>(C, k, threadIdx.x & 63, z, s, dz, ds, alpha, slots + k, nullptr);
        }
        return;
    }
    const int k = C.gp_big[bx - gq];
    gp_barrier_body<256>(C, k, threadIdx.x, z, s, dz, ds, alpha, slots + k, sh);
}

inline int step_grid(int m)
{
    int64_t g = ((int64_t)m + 255) / 256;
    if (g < 1) g = 1;
    if (g > kStepGridCap) g = kStepGridCap;
    return (int)g;
}

inline size_t step_psd_lds(const ConeDev& C) { return (size_t)4 * C.psd_kmax * C.psd_kmax * sizeof(double); }
// the big PSD class: n matrices of its largest side
inline size_t step_psdb_lds(const ConeDev& C, int n) { return (size_t)n * C.psdb_kmax * C.psdb_kmax * sizeof(double); }
// the dynamic LDS of this file's PSD kernels beyond the 64 KiB default, once per device and class
inline void step_psd_set_lds(bool big)
{
    static PerDeviceOnce once_small, once_big;
    if (!big) {
        once_small.run([]() {
            hipError_t e = set_max_lds(k_step_ds_psd, 150 * 1024);
            if (e == hipSuccess) e = set_max_lds(k_batch_step_ds_psd, 150 * 1024);
            if (e == hipSuccess) e = set_max_lds(k_step_length_psd, 150 * 1024);
            if (e == hipSuccess) e = set_max_lds(k_margins_psd, 150 * 1024);
            return e;
        });
        return;
    }
    once_big.run([]() {
        const int one = kPsdBigMaxDim * kPsdBigMaxDim * (int)sizeof(double);
        hipError_t e = set_max_lds(k_step_ds_psd_big, 2 * one);
        if (e == hipSuccess) e = set_max_lds(k_step_length_psd_big, 2 * one);
        if (e == hipSuccess) e = set_max_lds(k_margins_psd_big, one);
        if (e == hipSuccess) e = set_max_lds(k_barrier_psd_big, one);
        return e;
    });
}

}  // namespace

void launch_step_ds(const ConeDev& C, const ConeState& S, double* out, const double* step_z, const double* step_s,
                    double sigma_mu, double m_corr, int m, bool combined, hipStream_t st)
{
    if (m <= 0) return;
    if (C.npsd > 0) {
        step_psd_set_lds(false);
        hipLaunchKernelGGL(k_step_ds_psd, dim3(C.npsd), dim3(256), combined ? step_psd_lds(C) : 0, st, C, S, out, step_z, step_s,
                           sigma_mu, m_corr, combined ? 1 : 0);
    }
    if (C.npsdb > 0) {
        step_psd_set_lds(true);
        hipLaunchKernelGGL(k_step_ds_psd_big, dim3(C.npsdb), dim3(kPsdBigThreads), combined ? step_psdb_lds(C, 2) : 0, st, C, S,
                           out, step_z, step_s, sigma_mu, m_corr, combined ? 1 : 0);
    }
    const int ge = step_grid(m), gs = (C.nsoc + 3) / 4;
    hipLaunchKernelGGL(k_step_ds, dim3(ge + gs), dim3(256), 0, st, C, S, out, step_z, step_s, sigma_mu, m_corr, m,
                       combined ? 1 : 0, ge);
}

void launch_step_length(const ConeDev& C, const ConeState& S, const double* dz, const double* ds, const double* z,
                        const double* s, double step_tau, double step_kappa, double tau, double kappa, double* partial,
                        double* rec, const Publish& pub, int m, hipStream_t st)
{
    const int ge = step_grid(m), gs = (C.nsoc + 3) / 4;
    if (C.npsd > 0) {
        step_psd_set_lds(false);
        hipLaunchKernelGGL(k_step_length_psd, dim3(C.npsd), dim3(256), step_psd_lds(C), st, C, S, dz, ds, partial + ge + C.nsoc);
    }
    if (C.npsdb > 0) {
        step_psd_set_lds(true);
        hipLaunchKernelGGL(k_step_length_psd_big, dim3(C.npsdb), dim3(kPsdBigThreads), step_psdb_lds(C, 2), st, C, S, dz, ds,
                           partial + ge + C.nsoc + C.npsd);
    }
    hipLaunchKernelGGL(k_step_length, dim3(ge + gs), dim3(256), 0, st, C, dz, ds, z, s, m, partial, ge);
    hipLaunchKernelGGL(k_step_length_finish, dim3(1), dim3(256), 0, st, partial, ge + C.nsoc + C.npsd + C.npsdb, step_tau,
                       step_kappa, tau, kappa, rec, pub);
}

void launch_margins(const ConeDev& C, const double* v, double* partial, double* rec, const Publish& pub, int m, hipStream_t st)
{
    const int ge = step_grid(m), gs = (C.nsoc + 3) / 4, np = step_partials(C);
    double* pmin = partial;
    double* psum = partial + np;
    if (C.npsd > 0) {
        step_psd_set_lds(false);
        hipLaunchKernelGGL(k_margins_psd, dim3(C.npsd), dim3(256), (size_t)C.psd_kmax * C.psd_kmax * sizeof(double), st, C, v,
                           pmin + ge + C.nsoc, psum + ge + C.nsoc);
    }
    if (C.npsdb > 0) {
        step_psd_set_lds(true);
        hipLaunchKernelGGL(k_margins_psd_big, dim3(C.npsdb), dim3(kPsdBigThreads), step_psdb_lds(C, 1), st, C, v,
                           pmin + ge + C.nsoc + C.npsd, psum + ge + C.nsoc + C.npsd);
    }
    hipLaunchKernelGGL(k_margins, dim3(ge + gs), dim3(256), 0, st, C, v, m, pmin, psum, ge);
    hipLaunchKernelGGL(k_margins_finish, dim3(1), dim3(256), 0, st, pmin, psum, ge + C.nsoc + C.npsd + C.npsdb, rec, pub);
}

void launch_unit_shift(const ConeDev& C, double* v, double a1, double a2, bool two, bool primal, int m, hipStream_t st)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(k_unit_shift, dim3(step_grid(m)), dim3(256), 0, st, C, v, a1, a2, two ? 1 : 0, primal ? 1 : 0, m);
}

void launch_batch_step_ds(const ConeDev& C, const ConeState& S, const BatchDev& B, double* out, const double* step_z,
                          const double* step_s, const double* sigma_mu, const double* m_corr, int m, hipStream_t st)
{
    if (m <= 0) return;
    if (C.npsd > 0) {
        step_psd_set_lds(false);
        hipLaunchKernelGGL(k_batch_step_ds_psd, dim3(C.npsd), dim3(256), step_psd_lds(C), st, C, S, B, out, step_z, step_s, sigma_mu,
                           m_corr);
    }
    const int ge = step_grid(m), gs = (C.nsoc + 3) / 4;
    hipLaunchKernelGGL(k_batch_step_ds, dim3(ge + gs), dim3(256), 0, st, C, S, B, out, step_z, step_s, sigma_mu, m_corr, m, ge);
}

void launch_batch_step_length(const ConeDev& C, const ConeState& S, const BatchDev& B, const double* dz, const double* ds,
                              const double* z, const double* s, const double* scal, double* partial, double* rec, int m,
                              hipStream_t st)
{
    (void)m;
    const int ge = B.z256.nwg, gs = (C.nsoc + 3) / 4;
    if (C.npsd > 0) {
        step_psd_set_lds(false);
        hipLaunchKernelGGL(k_step_length_psd, dim3(C.npsd), dim3(256), step_psd_lds(C), st, C, S, dz, ds, partial + ge + C.nsoc);
    }
    if (ge + gs > 0) hipLaunchKernelGGL(k_batch_step_length, dim3(ge + gs), dim3(256), 0, st, C, B, dz, ds, z, s, partial);
    hipLaunchKernelGGL(k_batch_step_length_finish, dim3((B.nb + 3) / 4), dim3(256), 0, st, C, B, (const double*)partial, scal, rec);
}

void launch_batch_shift_to_interior(const ConeDev& C, const BatchDev& B, double* v, bool primal, double* partial, double* shift,
                                    double* rec, int m, hipStream_t st)
{
    const int ge = B.z256.nwg, gs = (C.nsoc + 3) / 4;
    double* pmin = partial;
    double* psum = partial + batch_step_slots(C, B);
    if (C.npsd > 0) {
        step_psd_set_lds(false);
        hipLaunchKernelGGL(k_margins_psd, dim3(C.npsd), dim3(256), (size_t)C.psd_kmax * C.psd_kmax * sizeof(double), st, C,
                           (const double*)v, pmin + ge + C.nsoc, psum + ge + C.nsoc);
    }
    if (ge + gs > 0) hipLaunchKernelGGL(k_batch_margins, dim3(ge + gs), dim3(256), 0, st, C, B, (const double*)v, pmin, psum);
    hipLaunchKernelGGL(k_batch_margins_finish, dim3((B.nb + 3) / 4), dim3(256), 0, st, C, B, (const double*)pmin, (const double*)psum,
                       rec, shift);
    if (m > 0)
        hipLaunchKernelGGL(k_batch_unit_shift, dim3(step_grid(m)), dim3(256), 0, st, C, B, v, (const double*)shift, primal ? 1 : 0, m);
}

// the generalized power cones' rows (mode 0: the unit start into out and out2; 1: a copy of s; 2: s + sigma_mu grad f*(z))
static void launch_gp_rows(const ConeDev& C, const ConeState& S, int mode, double* out, double* out2, const double* s, double sigma_mu,
                           hipStream_t st)
{
    const int g = (C.ngp_small + 3) / 4 + C.ngp_big;
    if (g > 0) hipLaunchKernelGGL(k_gp_rows, dim3(g), dim3(256), 0, st, C, S, mode, out, out2, s, sigma_mu);
}

void launch_unit_initialization(const ConeDev& C, const ConeState& S, double* s, double* z, int m, hipStream_t st)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(k_unit_initialization, dim3(step_grid(m)), dim3(256), 0, st, C, s, z, m);   // (a generalized power cone's rows: 0)
    launch_gp_rows(C, S, 0, s, z, nullptr, 0.0, st);
}

void launch_step_ds_ns(const ConeDev& C, const ConeState& S, double* out, const double* step_z, const double* step_s,
                       const double* s, const double* z, double sigma_mu, double m_corr, int m, bool combined, hipStream_t st)
{
    launch_step_ds(C, S, out, step_z, step_s, sigma_mu, m_corr, m, combined, st);
    const int nns = C.nexp + C.npow;
    if (nns > 0)
        hipLaunchKernelGGL(k_ns_ds, dim3(step_grid(nns)), dim3(256), 0, st, C, S, out, step_z, step_s, s, z, sigma_mu, m_corr,
                           combined ? 1 : 0);
    launch_gp_rows(C, S, combined ? 2 : 1, out, nullptr, s, sigma_mu, st);
}

// stages 1 to 3 of the composite step length; the generalized power cones' searches keep their slots behind the
// lane-per-cone workgroups'
void launch_step_length_ns(const ConeDev& C, const ConeState& S, const double* dz, const double* ds, const double* z,
                           const double* s, double step_tau, double step_kappa, double tau, double kappa, double backtrack_step,
                           double alpha_min, int trip_cap, double* partial, double* ns_partial, double* rec, const Publish& pub,
                           int m, hipStream_t st)
{
    launch_step_length(C, S, dz, ds, z, s, step_tau, step_kappa, tau, kappa, partial, rec, Publish{}, m, st);
    const int nns = C.nexp + C.npow, gn = nns > 0 ? step_grid(nns) : 0;
    const int ngp = C.ngp_small + C.ngp_big;
    if (gn > 0)
        hipLaunchKernelGGL(k_ns_step_length, dim3(gn), dim3(256), 0, st, C, dz, ds, z, s, rec, backtrack_step, alpha_min, trip_cap,
                           ns_partial);
    if (ngp > 0)
        hipLaunchKernelGGL(k_gp_step_length, dim3((C.ngp_small + 3) / 4 + C.ngp_big), dim3(256), 0, st, C, dz, ds, z, s, rec,
                           backtrack_step, alpha_min, trip_cap, ns_partial + gn);
    hipLaunchKernelGGL(k_ns_step_length_finish, dim3(1), dim3(256), 0, st, ns_partial, gn + ngp, rec, pub);
}

// the generalized power cones' terms: in slots behind the lane-per-cone workgroups'
void launch_barrier(const ConeDev& C, const double* z, const double* s, const double* dz, const double* ds, double alpha,
                    double* partial, double* rec, const Publish& pub, int m, hipStream_t st)
{
    const int ge = step_grid(m), gs = (C.nsoc + 3) / 4, nns = C.nexp + C.npow, gn = nns > 0 ? step_grid(nns) : 0;
    const int ngp = C.ngp_small + C.ngp_big;
    double* pbar = partial;
    double* pdot = partial + barrier_partials(C);
    if (C.npsd > 0)
        hipLaunchKernelGGL(k_barrier_psd, dim3(C.npsd), dim3(256), (size_t)C.psd_kmax * C.psd_kmax * sizeof(double), st, C, z, s, dz,
                           ds, alpha, pbar + ge + C.nsoc);
    hipLaunchKernelGGL(k_barrier, dim3(ge + gs), dim3(256), 0, st, C, z, s, dz, ds, alpha, m, pbar, pdot, ge);
    if (gn > 0) hipLaunchKernelGGL(k_barrier_ns, dim3(gn), dim3(256), 0, st, C, z, s, dz, ds, alpha, pbar + ge + C.nsoc + C.npsd);
    if (ngp > 0)
        hipLaunchKernelGGL(k_gp_barrier, dim3((C.ngp_small + 3) / 4 + C.ngp_big), dim3(256), 0, st, C, z, s, dz, ds, alpha,
                           pbar + ge + C.nsoc + C.npsd + gn);
    if (C.npsdb > 0) {
        step_psd_set_lds(true);
        hipLaunchKernelGGL(k_barrier_psd_big, dim3(C.npsdb), dim3(kPsdBigThreads), step_psdb_lds(C, 1), st, C, z, s, dz, ds, alpha,
                           pbar + ge + C.nsoc + C.npsd + gn + ngp);
    }
    hipLaunchKernelGGL(k_barrier_finish, dim3(1), dim3(256), 0, st, pbar, ge + C.nsoc + C.npsd + gn + ngp + C.npsdb, pdot, ge, rec,
                       pub);
}

}  // namespace hipkkt
