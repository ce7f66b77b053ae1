// The first step of every interior-point iteration on a device-resident iterate (see kernels.hpp):
//   residuals_update!                  residuals.jl:1-37      Px, rx_inf = -A'z, rz_inf = A x + s, rx, rz
//   the dots and norm_scaled calls     info.jl:33-51          q.x, b.z, s.z, x.Px and eight scaled 2-norms
//   variables_combined_step_rhs! x, z  variables.jl:124-162   (1 - sigma) rx, (1 - sigma) rz
//   variables_add_step!                variables.jl:107-122   x += a dx, s += a ds, z += a dz
// The residuals are ONE pass over rows 0 .. n + m - 1 of the full-CSR image of K (SpmvDev): eight lanes per row, the row's
// owner lane writes the five vectors and keeps 28 running values (four dot products, and per norm three sums of squares
// -- see iter_nrm_add), which the workgroup folds in a fixed order into its slot of `partial`; a finishing workgroup folds
// the slots in slot order and publishes twelve scalars.  No floating-point atomic anywhere: the same call on the same
// data gives the same bits.  Compiled without FMA contraction (the elementwise kernels promise fl(v + fl(a d))); the
// row sums use explicit fma as the other SpMV kernels do.
#include "kernels.hpp"
#include <cmath>

namespace hipkkt {

namespace {

// value slots: 0 q.x, 1 b.z, 2 s.z, 3 x.Px, then {big, mid, small} for each norm in the order of the record
constexpr int kIterNorm0 = 4;
constexpr int kIterOwners = 32;                       // rows (owner lanes) per workgroup of 256 at eight lanes per row

// Sums of squares that neither overflow nor underflow (Blue's three accumulators, the thresholds and scalings of LAPACK's
// dnrm2): |a| > 2^486 is squared as a 2^-538, |a| < 2^-511 as a 2^537, everything else as it is.  The scalings are powers
// of two, so every term carries the one rounding of its square.  A NaN fails both comparisons and lands in the middle
// sum, +-Inf in the big one: a non-finite entry cannot be hidden by a maximum, because there is none.
constexpr double kTbig = 0x1p486, kTsml = 0x1p-511, kSbig = 0x1p-538, kSsml = 0x1p537, kSsmlInv = 0x1p-537, kSbigInv = 0x1p538;

__device__ inline void iter_nrm_add(double v, double* acc3)
{
    const double a = fabs(v);
    if (a > kTbig) { const double t = a * kSbig; acc3[0] += t * t; }
    else if (a < kTsml) { const double t = a * kSsml; acc3[2] += t * t; }
    else acc3[1] += a * a;
}

__device__ inline double iter_nrm_finish(double big, double mid, double sml)
{
    if (mid != mid) return mid;
    if (big > 0.0) return sqrt(big + (mid * kSbig) * kSbig) * kSbigInv;
    if (sml > 0.0) return mid > 0.0 ? sqrt(mid + (sml * kSsmlInv) * kSsmlInv) : sqrt(sml) * kSsmlInv;
    return sqrt(mid);
}

// what the owner lane of row `row` does with the row's two sums: ap over the columns < n, aa over the columns >= n
__device__ inline void iter_row_owner(const IterVecs& V, int n, int row, double ap, double aa, double* acc)
{
    if (row < n) {
        const double xi = V.x[row], qi = V.q[row];
        const double Px = ap, rxi = -aa;
        const double rx = (rxi - Px) - qi * V.tau;
        V.Px[row] = Px;
        V.rx_inf[row] = rxi;
        V.rx[row] = rx;
        acc[0] += qi * xi;
        acc[3] += xi * Px;
        const double d = V.d ? V.d[row] : 1.0, dinv = V.d ? V.dinv[row] : 1.0;
        iter_nrm_add(d * xi, acc + kIterNorm0 + 0);
        iter_nrm_add(dinv * rxi, acc + kIterNorm0 + 9);
        iter_nrm_add(dinv * Px, acc + kIterNorm0 + 12);
        iter_nrm_add(dinv * rx, acc + kIterNorm0 + 21);
    } else {
        const int i = row - n;
        const double si = V.s[i], zi = V.z[i], bi = V.b[i];
        const double rzi = ap + si;
        const double rz = rzi - bi * V.tau;
        V.rz_inf[i] = rzi;
        V.rz[i] = rz;
        acc[1] += bi * zi;
        acc[2] += si * zi;
        const double e = V.d ? V.e[i] : 1.0, einv = V.d ? V.einv[i] : 1.0;
        iter_nrm_add(e * zi, acc + kIterNorm0 + 3);
        iter_nrm_add(einv * si, acc + kIterNorm0 + 6);
        iter_nrm_add(einv * rzi, acc + kIterNorm0 + 15);
        iter_nrm_add(einv * rz, acc + kIterNorm0 + 18);
    }
}

// the workgroup's 32 owner lanes (threadIdx.x % 8 == 0) -> partial[v * kIterStride + slot] for each of the 28 values:
// eight lanes per value add four owners each (in owner order) and meet in a fixed tree
// (dst: the slot's first value; stride: doubles between a slot's values)
__device__ inline void iter_fold_at(const double* acc, double* sh, double* __restrict__ dst, size_t stride)
{
    const int tid = threadIdx.x;
    if ((tid & 7) == 0) {
#pragma unroll
        for (int v = 0; v < kIterValues; ++v) sh[v * kIterOwners + (tid >> 3)] = acc[v];
    }
    __syncthreads();
    if (tid < kIterValues * 8) {
        const int v = tid >> 3, l = tid & 7;
        const double* p = sh + v * kIterOwners + l;
        double s = ((p[0] + p[8]) + p[16]) + p[24];
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) s += __shfl_down(s, o, 8);
        if (l == 0) dst[(size_t)v * stride] = s;
    }
}
__device__ inline void iter_fold(const double* acc, double* sh, double* __restrict__ partial, int slot)
{
    iter_fold_at(acc, sh, partial + slot, kIterStride);
}

__global__ __launch_bounds__(256) void k_iterate_residuals(SpmvDev A, IterDev I, IterVecs V, int n, int m,
                                                           double* __restrict__ partial)
{
    __shared__ double sh[kIterValues * kIterOwners];
    const int sub = threadIdx.x & 7;
    const int rows = n + m;
    double acc[kIterValues];
#pragma unroll
    for (int v = 0; v < kIterValues; ++v) acc[v] = 0.0;
    for (int64_t row = (int64_t)blockIdx.x * kIterOwners + (threadIdx.x >> 3); row < rows; row += (int64_t)gridDim.x * kIterOwners) {
        const int64_t q0 = A.ptr[row], q1 = I.rend[row];                 // (the walked prefix: iterate_rows.hpp)
        if (q1 - q0 > kLongRow) continue;                                // k_iterate_long_*
        double ap = 0.0, aa = 0.0;
        for (int64_t q = q0 + sub; q < q1; q += 8) {
            const int c = A.col[q];
            const double v = A.val[q];
            if (c < n) ap = fma(v, V.x[c], ap);
            else aa = fma(v, V.z[c - n], aa);
        }
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) { ap += __shfl_down(ap, o, 8); aa += __shfl_down(aa, o, 8); }
        if (sub == 0) iter_row_owner(V, n, (int)row, ap, aa, acc);
    }
    iter_fold(acc, sh, partial, blockIdx.x);
}

// one workgroup per chunk of a long walked prefix: fixed assignment of entries to threads, fixed reduction tree
__global__ __launch_bounds__(256) void k_iterate_long_chunks(SpmvDev A, IterDev I, IterVecs V, int n)
{
    __shared__ double shp[256], sha[256];
    const int64_t q0 = I.chunk_q[2 * blockIdx.x], q1 = I.chunk_q[2 * blockIdx.x + 1];
    double ap = 0.0, aa = 0.0;
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
        const int c = A.col[q];
        const double v = A.val[q];
        if (c < n) ap = fma(v, V.x[c], ap);
        else aa = fma(v, V.z[c - n], aa);
    }
    shp[threadIdx.x] = ap;
    sha[threadIdx.x] = aa;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { shp[threadIdx.x] += shp[threadIdx.x + o]; sha[threadIdx.x] += sha[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { I.long_partial[2 * (size_t)blockIdx.x] = shp[0]; I.long_partial[2 * (size_t)blockIdx.x + 1] = sha[0]; }
}

// the long rows' owners: chunk sums in chunk order, then what every other row's owner does; their slot is `slot`
__global__ __launch_bounds__(256) void k_iterate_long_finish(IterDev I, IterVecs V, int n, double* __restrict__ partial, int slot)
{
    __shared__ double sh[kIterValues * kIterOwners];
    double acc[kIterValues];
#pragma unroll
    for (int v = 0; v < kIterValues; ++v) acc[v] = 0.0;
    if ((threadIdx.x & 7) == 0)
        for (int t = threadIdx.x >> 3; t < I.nlong; t += kIterOwners) {
            double ap = 0.0, aa = 0.0;
            for (int64_t c = I.long_chunk_ptr[t]; c < I.long_chunk_ptr[t + 1]; ++c) { ap += I.long_partial[2 * c]; aa += I.long_partial[2 * c + 1]; }
            iter_row_owner(V, n, I.long_rows[t], ap, aa, acc);
        }
    iter_fold(acc, sh, partial, slot);
}

// 16 waves, a value each (then a second one): a lane adds every 64th slot, the wave meets in a fixed butterfly
__global__ __launch_bounds__(1024) void k_iterate_finish(const double* __restrict__ partial, int np, double* __restrict__ rec,
                                                          Publish P)
{
    __shared__ double sh[kIterValues];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int v = wave; v < kIterValues; v += 16) {
        double s = 0.0;
        for (int i = lane; i < np; i += 64) s += partial[(size_t)v * kIterStride + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) sh[v] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 0; i < 4; ++i) rec[i] = sh[i];
        for (int j = 0; j < 8; ++j) rec[4 + j] = iter_nrm_finish(sh[kIterNorm0 + 3 * j], sh[kIterNorm0 + 3 * j + 1], sh[kIterNorm0 + 3 * j + 2]);
        if (P.dst) {
            for (int i = 0; i < P.n; ++i) P.dst[i] = P.rec[i];
            P.dst[P.n] = P.seq;
            for (int i = 0; i < P.nzero; ++i) P.rec[i] = 0.0;
        }
    }
}

// (outputs may alias inputs -- an element is read and written by the same thread --, so no __restrict__ here)
__global__ __launch_bounds__(256) void k_iterate_scale(double* ox, double* oz, const double* rx, const double* rz, double f, int n,
                                                       int64_t len)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
        if (i < n) ox[i] = f * rx[i];
        else oz[i - n] = f * rz[i - n];
    }
}

__global__ __launch_bounds__(256) void k_iterate_add_step(double* x, double* s, double* z, const double* __restrict__ dx,
                                                          const double* __restrict__ ds, const double* __restrict__ dz,
                                                          double alpha, int n, int m, int64_t len)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
        if (i < n) x[i] = x[i] + alpha * dx[i];
        else if (i < (int64_t)n + m) s[i - n] = s[i - n] + alpha * ds[i - n];
        else z[i - n - m] = z[i - n - m] + alpha * dz[i - n - m];
    }
}

// ---- the same pass over a stack of member problems (kernels.hpp: BatchDev): workgroup w takes 32 combined rows of ONE
// member -- the row sums are formed exactly as above, the owner lane applies the member's own tau -- and leaves its 28
// values in slot w; a long row is a slot of its own behind them; member b's workgroup folds b's slots in slot order.
// partial[v * nslots + slot].
__global__ __launch_bounds__(256) void k_batch_residuals(SpmvDev A, IterDev I, IterVecs V, BatchDev B, const double* __restrict__ tau,
                                                         int n, double* __restrict__ partial, size_t nslots)
{
    __shared__ double sh[kIterValues * kIterOwners];
    const int sub = threadIdx.x & 7;
    const int b = B.rows32.wg_mem[blockIdx.x];
    const int x0 = B.x_off[b], nx = B.x_off[b + 1] - x0, z0 = B.z_off[b], nrows = nx + (B.z_off[b + 1] - z0);
    const int local = B.rows32.wg_first[blockIdx.x] + (int)(threadIdx.x >> 3);
    V.tau = tau[b];
    double acc[kIterValues];
#pragma unroll
    for (int v = 0; v < kIterValues; ++v) acc[v] = 0.0;
    if (local < nrows) {
        const int row = local < nx ? x0 + local : n + z0 + (local - nx);
        const int64_t q0 = A.ptr[row], q1 = I.rend[row];
        if (q1 - q0 <= kLongRow) {                                       // (a long one: k_iterate_long_chunks, k_batch_long_finish)
            double ap = 0.0, aa = 0.0;
            for (int64_t q = q0 + sub; q < q1; q += 8) {
                const int c = A.col[q];
                const double v = A.val[q];
                if (c < n) ap = fma(v, V.x[c], ap);
                else aa = fma(v, V.z[c - n], aa);
            }
#pragma unroll
            for (int o = 4; o > 0; o >>= 1) { ap += __shfl_down(ap, o, 8); aa += __shfl_down(aa, o, 8); }
            if (sub == 0) iter_row_owner(V, n, row, ap, aa, acc);
        }
    }
    iter_fold_at(acc, sh, partial + blockIdx.x, nslots);
}

// one long row per workgroup (B.long_order): chunk sums in chunk order, the owner's work with the member's tau
__global__ __launch_bounds__(64) void k_batch_long_finish(IterDev I, IterVecs V, BatchDev B, const double* __restrict__ tau, int n,
                                                          double* __restrict__ partial, size_t nslots)
{
    if (threadIdx.x != 0) return;
    const int t = B.long_order[blockIdx.x];
    const int row = I.long_rows[t];
    V.tau = tau[row < n ? B.xmem[row] : B.zmem[row - n]];
    double acc[kIterValues];
#pragma unroll
    for (int v = 0; v < kIterValues; ++v) acc[v] = 0.0;
    double ap = 0.0, aa = 0.0;
    for (int64_t c = I.long_chunk_ptr[t]; c < I.long_chunk_ptr[t + 1]; ++c) { ap += I.long_partial[2 * c]; aa += I.long_partial[2 * c + 1]; }
    iter_row_owner(V, n, row, ap, aa, acc);
    double* dst = partial + (size_t)B.rows32.nwg + blockIdx.x;
#pragma unroll
    for (int v = 0; v < kIterValues; ++v) dst[(size_t)v * nslots] = acc[v];
}

// member b = blockIdx.x: four waves, a value each (then the next four): a lane adds every 64th of b's slots -- its
// workgroups', then its long rows' --, the wave meets in a fixed butterfly
__global__ __launch_bounds__(256) void k_batch_residuals_finish(BatchDev B, const double* __restrict__ partial, size_t nslots,
                                                                double* __restrict__ rec)
{
    __shared__ double sh[kIterValues];
    const int b = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w0 = B.rows32.wg_ptr[b], nw = B.rows32.wg_ptr[b + 1] - w0;
    const int l0 = B.rows32.nwg + B.long_ptr[b], nl = B.long_ptr[b + 1] - B.long_ptr[b];
    for (int v = wave; v < kIterValues; v += 4) {
        const double* p = partial + (size_t)v * nslots;
        double s = 0.0;
        for (int i = lane; i < nw + nl; i += 64) s += p[i < nw ? w0 + i : l0 + (i - nw)];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) sh[v] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* r = rec + (size_t)12 * b;
        for (int i = 0; i < 4; ++i) r[i] = sh[i];
        for (int j = 0; j < 8; ++j) r[4 + j] = iter_nrm_finish(sh[kIterNorm0 + 3 * j], sh[kIterNorm0 + 3 * j + 1], sh[kIterNorm0 + 3 * j + 2]);
    }
}

inline int iter_elem_grid(int64_t len)
{
    int64_t g = (len + 255) / 256;
    if (g > kIterGridCap) g = kIterGridCap;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace

int iterate_grid(int n, int m)
{
    int64_t g = ((int64_t)n + m + kIterOwners - 1) / kIterOwners;
    if (g > kIterGridCap) g = kIterGridCap;
    return (int)g;
}

void launch_iterate_residuals(const SpmvDev& A, const IterDev& I, const IterVecs& V, int n, int m, double* partial, double* rec,
                              const Publish& pub, hipStream_t st)
{
    const int g = iterate_grid(n, m);
    if (g > 0) hipLaunchKernelGGL(k_iterate_residuals, dim3(g), dim3(256), 0, st, A, I, V, n, m, partial);
    if (I.nlong > 0) {
        hipLaunchKernelGGL(k_iterate_long_chunks, dim3(I.nchunks), dim3(256), 0, st, A, I, V, n);
        hipLaunchKernelGGL(k_iterate_long_finish, dim3(1), dim3(256), 0, st, I, V, n, partial, g);
    }
    hipLaunchKernelGGL(k_iterate_finish, dim3(1), dim3(1024), 0, st, (const double*)partial, g + (I.nlong > 0 ? 1 : 0), rec, pub);
}

void launch_batch_residuals(const SpmvDev& A, const IterDev& I, const IterVecs& V, const BatchDev& B, const double* tau, int n,
                            int m, double* partial, double* rec, hipStream_t st)
{
    (void)m;
    const size_t nslots = batch_residual_slots(B, I);
    if (B.rows32.nwg > 0)
        hipLaunchKernelGGL(k_batch_residuals, dim3(B.rows32.nwg), dim3(256), 0, st, A, I, V, B, tau, n, partial, nslots);
    if (I.nlong > 0) {
        hipLaunchKernelGGL(k_iterate_long_chunks, dim3(I.nchunks), dim3(256), 0, st, A, I, V, n);
        hipLaunchKernelGGL(k_batch_long_finish, dim3(I.nlong), dim3(64), 0, st, I, V, B, tau, n, partial, nslots);
    }
    hipLaunchKernelGGL(k_batch_residuals_finish, dim3(B.nb), dim3(256), 0, st, B, (const double*)partial, nslots, rec);
}

void launch_iterate_scale(double* ox, double* oz, const double* rx, const double* rz, double f, int n, int m, hipStream_t st)
{
    const int64_t len = (int64_t)n + m;
    if (len <= 0) return;
    hipLaunchKernelGGL(k_iterate_scale, dim3(iter_elem_grid(len)), dim3(256), 0, st, ox, oz, rx, rz, f, n, len);
}

void launch_iterate_add_step(double* x, double* s, double* z, const double* dx, const double* ds, const double* dz, double alpha,
                             int n, int m, hipStream_t st)
{
    const int64_t len = (int64_t)n + 2 * (int64_t)m;
    if (len <= 0) return;
    hipLaunchKernelGGL(k_iterate_add_step, dim3(iter_elem_grid(len)), dim3(256), 0, st, x, s, z, dx, ds, dz, alpha, n, m, len);
}

}  // namespace hipkkt
