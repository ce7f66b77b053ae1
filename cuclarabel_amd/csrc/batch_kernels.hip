// The elementwise steps and the step recovery of kkt_solve! on a stack of independent member problems (kernels.hpp:
// BatchDev).  Every scalar of the whole-handle kernels is an array over the members here, read through the
// row's member; every dot product is segmented by member:
//   variables_combined_step_rhs! x, z  variables.jl:124-162   (1 - sigma_b) rx, (1 - sigma_b) rz
//   variables_add_step!                variables.jl:107-122   x += a_b dx, s += a_b ds, z += a_b dz
//   kkt_solve!, behind its solve       kktsystem.jl:185-206   the seven dot products, dtau_b, dkappa_b, (dx, dz)
// The segmented residual pass stands beside its twin in iterate_kernels.hip, the cone operations beside theirs in
// step_kernels.hip (they call the same per-row and per-cone device functions).
// Reductions: a workgroup takes 256 combined rows of ONE member (BatchDev::rows256), folds its values in a fixed tree and
// leaves them in its slot; member b's wave adds b's slots lane-strided in slot order and meets in a fixed butterfly.  No
// floating-point atomic.  Compiled without FMA contraction, as the twins are.
#include "kernels.hpp"
#include <cmath>

namespace hipkkt {

namespace {

constexpr int kBatchDots = 7;        // q.x1, b.z1, x.(P x1), xm.(P xm), q.x2, b.z2, x2.(P x2)

inline int batch_elem_grid(int64_t len)
{
    int64_t g = (len + 255) / 256;
    if (g > 2048) g = 2048;
    return (int)(g < 1 ? 1 : g);
}

// (outputs may alias inputs -- an element is read and written by the same thread --, so no __restrict__ here)
__global__ __launch_bounds__(256) void k_batch_scale(BatchDev B, double* ox, double* oz, const double* rx, const double* rz,
                                                     const double* __restrict__ sigma, int n, int64_t len)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
        if (i < n) ox[i] = (1.0 - sigma[B.xmem[i]]) * rx[i];
        else oz[i - n] = (1.0 - sigma[B.zmem[i - n]]) * rz[i - n];
    }
}

__global__ __launch_bounds__(256) void k_batch_add_step(BatchDev B, double* x, double* s, double* z, const double* __restrict__ dx,
                                                        const double* __restrict__ ds, const double* __restrict__ dz,
                                                        const double* __restrict__ alpha, int n, int m, int64_t len)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
        if (i < n) {
            const double a = alpha[B.xmem[i]];
            if (a != 0.0) x[i] = x[i] + a * dx[i];                       // (a frozen member's rows are not written at all)
        } else if (i < (int64_t)n + m) {
            const double a = alpha[B.zmem[i - n]];
            if (a != 0.0) s[i - n] = s[i - n] + a * ds[i - n];
        } else {
            const double a = alpha[B.zmem[i - n - m]];
            if (a != 0.0) z[i - n - m] = z[i - n - m] + a * dz[i - n - m];
        }
    }
}

// pa = P x1, pb = P xm, pc = P x2 with xm = x / tau_b - x2 formed on the fly and stored by the row that owns it: k_P_spmv2
// with the row's member's tau (P couples no two members, so a row's columns are its own member's)
__global__ __launch_bounds__(256) void k_batch_P_spmv3(SpmvDev A, const double* __restrict__ K, BatchDev B,
                                                       const double* __restrict__ x1, const double* __restrict__ x,
                                                       const double* __restrict__ x2, const double* __restrict__ tau_of,
                                                       double* __restrict__ pa, double* __restrict__ pb, double* __restrict__ pc,
                                                       double* __restrict__ xm_out, int n)
{
    const int sub = threadIdx.x & 7;
    for (int row = blockIdx.x * 32 + (threadIdx.x >> 3); row < n; row += gridDim.x * 32) {
        const double tau = tau_of[B.xmem[row]];
        double a1 = 0.0, a2 = 0.0, a3 = 0.0;
        const int64_t qend = A.pend ? A.pend[row] : A.ptr[row + 1];
        for (int64_t q = A.ptr[row] + sub; q < qend; q += 8) {
            const int c = A.col[q];
            if (c < n) {
                const double v = A.val ? A.val[q] : K[A.vmap[q]];
                const double x2c = x2[c];
                a1 = fma(v, x1[c], a1);
                a2 = fma(v, x[c] / tau - x2c, a2);
                a3 = fma(v, x2c, a3);
            }
        }
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) { a1 += __shfl_down(a1, o, 8); a2 += __shfl_down(a2, o, 8); a3 += __shfl_down(a3, o, 8); }
        if (sub == 0) {
            pa[row] = a1;
            pb[row] = a2;
            pc[row] = a3;
            xm_out[row] = x[row] / tau - x2[row];
        }
    }
}

// workgroup w: 256 combined rows of member wg_mem[w], a thread per row; partial[v * nwg + w]
__global__ __launch_bounds__(256) void k_batch_sys_dots(BatchDev B, const double* __restrict__ q, const double* __restrict__ bvec,
                                                        const double* __restrict__ x, const double* __restrict__ x1,
                                                        const double* __restrict__ z1, const double* __restrict__ x2,
                                                        const double* __restrict__ z2, const double* __restrict__ pa,
                                                        const double* __restrict__ pb, const double* __restrict__ pc,
                                                        const double* __restrict__ xm, double* __restrict__ partial)
{
    __shared__ double sh[kBatchDots][256];
    const int b = B.rows256.wg_mem[blockIdx.x];
    const int x0 = B.x_off[b], nx = B.x_off[b + 1] - x0, z0 = B.z_off[b], nrows = nx + (B.z_off[b + 1] - z0);
    const int local = B.rows256.wg_first[blockIdx.x] + (int)threadIdx.x;
    double v[kBatchDots];
#pragma unroll
    for (int k = 0; k < kBatchDots; ++k) v[k] = 0.0;
    if (local < nx) {
        const int i = x0 + local;
        v[0] = q[i] * x1[i];
        v[2] = x[i] * pa[i];
        v[3] = xm[i] * pb[i];
        v[4] = q[i] * x2[i];
        v[6] = x2[i] * pc[i];
    } else if (local < nrows) {
        const int i = z0 + (local - nx);
        v[1] = bvec[i] * z1[i];
        v[5] = bvec[i] * z2[i];
    }
#pragma unroll
    for (int k = 0; k < kBatchDots; ++k) sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < kBatchDots; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x < kBatchDots) partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = sh[threadIdx.x][0];
}

// wave = member: the scalars of kkt_solve! (kktsystem.jl:185-196, :206) from the member's own dot products;
// scal = {rhs_tau, rhs_kappa, tau, kappa}, nb each; out[2 b] = dtau, out[2 b + 1] = dkappa
__global__ __launch_bounds__(256) void k_batch_sys_scalars(BatchDev B, const double* __restrict__ partial, const double* __restrict__ scal,
                                                           double* __restrict__ dtau_out, double* __restrict__ out)
{
    const int b = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B.nb) return;
    const int nwg = B.rows256.nwg;
    double d[kBatchDots];
#pragma unroll
    for (int k = 0; k < kBatchDots; ++k) {
        double s = 0.0;
        for (int i = B.rows256.wg_ptr[b] + lane; i < B.rows256.wg_ptr[b + 1]; i += 64) s += partial[(size_t)k * nwg + i];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        d[k] = s;
    }
    if (lane == 0) {
        const double rhs_tau = scal[b], rhs_kappa = scal[B.nb + b], tau = scal[2 * B.nb + b], kappa = scal[3 * B.nb + b];
        // xi = x / tau, so xi.(P x1) = d[2] / tau
        const double tau_num = rhs_tau - rhs_kappa / tau + d[0] + d[1] + 2.0 * (d[2] / tau);
        double tau_den = kappa / tau - d[4] - d[5];
        tau_den += d[3] - d[6];
        const double dtau = tau_num / tau_den;
        dtau_out[b] = dtau;
        out[2 * b] = dtau;
        out[2 * b + 1] = -(rhs_kappa + kappa * dtau) / tau;              // :206
    }
}

// (dx, dz) = (x1, z1) + dtau_b (x2, z2)   (kktsystem.jl:200-203)
__global__ __launch_bounds__(256) void k_batch_sys_step(BatchDev B, double* __restrict__ dx, double* __restrict__ dz,
                                                        const double* __restrict__ x1, const double* __restrict__ z1,
                                                        const double* __restrict__ x2, const double* __restrict__ z2,
                                                        const double* __restrict__ dtau, int n, int64_t len)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
        if (i < n) dx[i] = x1[i] + dtau[B.xmem[i]] * x2[i];
        else dz[i - n] = z1[i - n] + dtau[B.zmem[i - n]] * z2[i - n];
    }
}

}  // namespace

void launch_batch_scale(const BatchDev& B, double* ox, double* oz, const double* rx, const double* rz, const double* sigma, int n,
                        int m, hipStream_t st)
{
    const int64_t len = (int64_t)n + m;
    if (len <= 0) return;
    hipLaunchKernelGGL(k_batch_scale, dim3(batch_elem_grid(len)), dim3(256), 0, st, B, ox, oz, rx, rz, sigma, n, len);
}

void launch_batch_add_step(const BatchDev& B, double* x, double* s, double* z, const double* dx, const double* ds, const double* dz,
                           const double* alpha, int n, int m, hipStream_t st)
{
    const int64_t len = (int64_t)n + 2 * (int64_t)m;
    if (len <= 0) return;
    hipLaunchKernelGGL(k_batch_add_step, dim3(batch_elem_grid(len)), dim3(256), 0, st, B, x, s, z, dx, ds, dz, alpha, n, m, len);
}

void launch_batch_sys_step(const SpmvDev& A, const double* Kval, const BatchDev& B, const double* q, const double* bvec,
                           const double* x, const double* x1, const double* z1, const double* x2, const double* z2,
                           const double* scal, double* pa, double* pb, double* pc, double* xm, double* partial, double* dtau,
                           double* out, double* dx, double* dz, int n, int m, hipStream_t st)
{
    int g = (n + 31) / 32;
    if (g > 2048) g = 2048;
    if (n > 0)
        hipLaunchKernelGGL(k_batch_P_spmv3, dim3(g), dim3(256), 0, st, A, Kval, B, x1, x, x2, scal + 2 * (size_t)B.nb, pa, pb, pc, xm, n);
    hipLaunchKernelGGL(k_batch_sys_dots, dim3(B.rows256.nwg), dim3(256), 0, st, B, q, bvec, x, x1, z1, x2, z2, (const double*)pa,
                       (const double*)pb, (const double*)pc, (const double*)xm, partial);
    hipLaunchKernelGGL(k_batch_sys_scalars, dim3((B.nb + 3) / 4), dim3(256), 0, st, B, (const double*)partial, scal, dtau, out);
    const int64_t len = (int64_t)n + m;
    hipLaunchKernelGGL(k_batch_sys_step, dim3(batch_elem_grid(len)), dim3(256), 0, st, B, dx, dz, x1, z1, x2, z2, (const double*)dtau,
                       n, len);
}

}  // namespace hipkkt
