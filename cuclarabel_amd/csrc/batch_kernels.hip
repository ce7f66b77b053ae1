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
#include "launch_shapes.hpp"
#include "refine_device.hpp"
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

// ---- the refinement rule per member (kernels.hpp: MemberIrDev; kktsolver_directldl.jl:389-449 on each member's rows).
// maxima of up to two slot ranges [s0, s1), known to every thread afterwards (a maximum does not depend on the order, so
// every workgroup of a member gets the same bits)
__device__ inline void block_max2_all(const double* __restrict__ p0, const double* __restrict__ p1, int s0, int s1, double& o0,
                                      double& o1, double (*sh)[4])
{
    double v0 = 0.0, v1 = 0.0;
    for (int i = s0 + (int)threadIdx.x; i < s1; i += 256) {
        v0 = fmax(v0, p0[i]);
        if (p1) v1 = fmax(v1, p1[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { v0 = fmax(v0, __shfl_xor(v0, o, 64)); v1 = fmax(v1, __shfl_xor(v1, o, 64)); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = v0; sh[1][threadIdx.x >> 6] = v1; }
    __syncthreads();
    o0 = fmax(fmax(sh[0][0], sh[0][1]), fmax(sh[0][2], sh[0][3]));
    o1 = fmax(fmax(sh[1][0], sh[1][1]), fmax(sh[1][2], sh[1][3]));
}

// workgroup w: the positions wg_first[w] .. + chunk - 1 of member wg_mem[w]'s list of image rows, G lanes per row; a
// row's sum is k_residual<G, 1>'s (residual_row_dot), so e holds the same bits.  pe / pb: the slot arrays (pb null: not
// the first residual of a solve).  Long rows are left to the chunk kernel and k_member_long_finish.
template <int G>
__global__ __launch_bounds__(256) void k_member_residual(SpmvDev A, const double* __restrict__ K, MemberIrDev M,
                                                         const double* __restrict__ b, const double* __restrict__ x,
                                                         double* __restrict__ e, double* __restrict__ pe, double* __restrict__ pb)
{
    __shared__ double sh[2][4];
    const int mem = M.wg_mem[blockIdx.x];
    const int first = M.wg_first[blockIdx.x];
    const int end = min(first + M.chunk, M.img_ptr[mem + 1]);
    const int sub = threadIdx.x % G;
    double vmax = 0.0, bmax = 0.0;
    bool bad = false;
    // (the row comes from a table here, one dependent load more than k_residual's: the next pass's row and entry range are
    //  fetched while this pass's row is summed)
    int pos = first + (int)threadIdx.x / G;
    int row = -1;
    int64_t q0 = 0, q1 = 0;
    if (pos < end) { row = M.img_rows[pos]; q0 = A.ptr[row]; q1 = A.ptr[row + 1]; }
    while (pos < end) {
        const int row_now = row;
        const int64_t q0_now = q0, q1_now = q1;
        pos += 256 / G;
        if (pos < end) { row = M.img_rows[pos]; q0 = A.ptr[row]; q1 = A.ptr[row + 1]; }
        if (q1_now - q0_now > kLongRow) continue;
        double acc[1];
        residual_row_dot<G, 1>(A, K, x, 0, q0_now, q1_now, sub, acc);
        if (sub == 0) {
            const double bv = b[row_now];
            const double r = bv - acc[0];
            e[row_now] = r;
            if (!isfinite(r)) bad = true;
            vmax = fmax(vmax, fabs(r));
            bmax = isfinite(bv) ? fmax(bmax, fabs(bv)) : INFINITY;
        }
    }
    if (bad) vmax = INFINITY;                        // (marks non-finite, as k_residual does)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { vmax = fmax(vmax, __shfl_xor(vmax, o, 64)); bmax = fmax(bmax, __shfl_xor(bmax, o, 64)); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = vmax; sh[1][threadIdx.x >> 6] = bmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int slot = (int)blockIdx.x + mem;
        pe[slot] = fmax(fmax(sh[0][0], sh[0][1]), fmax(sh[0][2], sh[0][3]));
        if (pb) pb[slot] = fmax(fmax(sh[1][0], sh[1][1]), fmax(sh[1][2], sh[1][3]));
    }
}

// wave = member: its long rows' residuals from the chunk sums (summed in chunk order, as k_residual_long_finish does) and
// their maxima into the member's last slot
__global__ __launch_bounds__(256) void k_member_long_finish(SpmvDev A, MemberIrDev M, const double* __restrict__ b,
                                                            double* __restrict__ e, double* __restrict__ pe, double* __restrict__ pb)
{
    const int mem = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (mem >= M.nb) return;
    double vmax = 0.0, bmax = 0.0;
    bool bad = false;
    for (int i = M.long_ptr[mem] + lane; i < M.long_ptr[mem + 1]; i += 64) {
        const int t = M.long_order[i];
        const int row = A.long_rows[t];
        double acc = 0.0;
        for (int64_t c = A.long_chunk_ptr[t]; c < A.long_chunk_ptr[t + 1]; ++c) acc += A.long_partial[c];
        const double bv = b[row];
        const double r = bv - acc;
        e[row] = r;
        if (!isfinite(r)) bad = true;
        vmax = fmax(vmax, fabs(r));
        bmax = isfinite(bv) ? fmax(bmax, fabs(bv)) : INFINITY;
    }
    if (bad) vmax = INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { vmax = fmax(vmax, __shfl_xor(vmax, o, 64)); bmax = fmax(bmax, __shfl_xor(bmax, o, 64)); }
    if (lane == 0) {
        const int slot = M.wg_ptr[mem + 1] + mem;
        pe[slot] = vmax;
        if (pb) pb[slot] = bmax;
    }
}

// The aggregate over the members without a second launch: every member's leading workgroup adds {1, active, bad} to ONE
// packed 64-bit counter (whole numbers, kMemberCountBits bits each) after folding its norme into a 64-bit maximum (the bit
// pattern of a non-negative double orders as the double does); both are agent-scope atomics on both sides.  The leader
// whose add completes the count writes the record and clears the two words for the next kernel.
constexpr int kMemberCountBits = 21;

__global__ __launch_bounds__(256) void k_member_ir_round(MemberIrDev M, int r, const int* __restrict__ flag_in, double* __restrict__ x,
                                                         const double* __restrict__ dx, double* __restrict__ e, double abstol,
                                                         double reltol, double stop_ratio, int max_iter, double* __restrict__ readback)
{
    __shared__ double sh[2][4];
    const int mem = M.wg_mem[blockIdx.x];
    const int s0 = M.wg_ptr[mem] + mem, s1 = M.wg_ptr[mem + 1] + mem + 1;
    const int S = M.nwg + M.nb;
    double active, rounds, bad, norme, normb;
    bool accept = false;
    if (r == 0) {
        double ne0;
        block_max2_all(M.slots, M.slots + S, s0, s1, ne0, normb, sh);
        ir_initial(ne0, normb, abstol, reltol, max_iter, active, rounds, bad, norme);
    } else {
        const double* prev = M.state + ((size_t)(r - 1) * M.nb + mem) * 4;
        active = prev[0]; rounds = prev[1]; bad = prev[2]; norme = prev[3];
        normb = M.normb[mem];
        if (active != 0.0) {                         // (uniform over the workgroup: the barrier inside is safe)
            double cand, unused;
            block_max2_all(M.slots + 2 * (size_t)S, nullptr, s0, s1, cand, unused, sh);
            accept = ir_apply_rule(cand, r, max_iter, abstol, reltol, stop_ratio, normb, active, rounds, bad, norme);
        }
    }
    // a member that has left its loop is not written again: its x stays, its rows of e are zero for the next sweeps
    const int first = M.wg_first[blockIdx.x];
    const int end = min(first + M.chunk, M.img_ptr[mem + 1]);
    if (accept || active == 0.0) {
        for (int pos = first + (int)threadIdx.x; pos < end; pos += 4 * 256) {          // (four rows in flight)
            int rows[4];
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) rows[u] = (pos + u * 256 < end) ? M.img_rows[pos + u * 256] : -1;
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = (accept && rows[u] >= 0) ? dx[rows[u]] : 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (rows[u] < 0) continue;
                if (accept) x[rows[u]] = v[u];
                if (active == 0.0) e[rows[u]] = 0.0;
            }
        }
    }
    if ((int)blockIdx.x != M.wg_ptr[mem] || threadIdx.x != 0) return;
    double* st = M.state + ((size_t)r * M.nb + mem) * 4;
    st[0] = active; st[1] = rounds; st[2] = bad; st[3] = norme;
    if (r == 0) M.normb[mem] = normb;
    double* info = M.info + 4 * (size_t)mem;
    info[0] = rounds; info[1] = norme; info[2] = normb; info[3] = bad;
    unsigned long long* agg = M.agg;                                   // [0] the packed counts, [1] the largest norme's bits
    // (norme is never NaN: the residual kernels mark non-finite rows as +Inf)
    unsigned long long seen = __hip_atomic_fetch_max(agg + 1, (unsigned long long)__double_as_longlong(norme), __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(seen) : : "memory");      // the maximum has been performed before the count moves
    const unsigned long long add = 1ull + ((active != 0.0 ? 1ull : 0ull) << kMemberCountBits) +
                                   ((bad != 0.0 ? 1ull : 0ull) << (2 * kMemberCountBits));
    const unsigned long long before = __hip_atomic_fetch_add(agg, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long now = before + add, mask = (1ull << kMemberCountBits) - 1;
    if ((now & mask) != (unsigned long long)M.nb) return;
    const unsigned long long top = __hip_atomic_load(agg + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(agg, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(agg + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the most rounds any member took: a member's rounds are the rounds it entered active, so the count grows by one in
    // every round that some member entered active (the previous kernel's record says whether one did)
    const double most = r == 0 ? 0.0 : (readback[0] != 0.0 ? (double)r : readback[1]);
    readback[0] = ((now >> kMemberCountBits) & mask) ? 1.0 : 0.0;
    readback[1] = most;
    readback[2] = ((now >> (2 * kMemberCountBits)) & mask) ? 1.0 : 0.0;
    readback[3] = __longlong_as_double((long long)top);
    readback[4] = (flag_in && flag_in[0]) ? 1.0 : 0.0;
}

// ---- the static regulariser and the failure words per member (kernels.hpp: MemberStatusDev;
// kktsolver_directldl.jl:259-310 on each member's rows of K's image).
// max |K_ii| over every member's image rows, and over all rows, on the bit patterns of the non-negative values (their
// order is the doubles' order) with an integer atomicMax into words the caller zeroed: exact whatever the order.  A NaN
// diagonal counts as 0, as k_diag_absmax's fmax drops it.  A member's rows are runs of the image (its x rows, its z rows,
// its cones' expansion rows), so nearly every wave holds ONE member and folds its 64 values before its single atomic;
// a wave that straddles members sends its lanes' values one by one.
__global__ __launch_bounds__(256) void k_member_diag_max(MemberStatusDev M, const double* __restrict__ K, const int* __restrict__ diag)
{
    __shared__ unsigned long long sh[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long all = 0ull;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < M.N; base += (int64_t)gridDim.x * 256) {      // (uniform over the workgroup)
        const int64_t i = base + (int64_t)threadIdx.x;
        const bool valid = i < M.N;
        const int mem = valid ? M.rowmem[i] : -1;
        const double v = valid ? fmax(0.0, fabs(K[diag[i]])) : 0.0;
        unsigned long long p = (unsigned long long)__double_as_longlong(v);
        all = p > all ? p : all;
        if (base + wave * 64 >= M.N) continue;                                       // (the wave has no row: uniform over the wave)
        const int lead = __builtin_amdgcn_readfirstlane(mem);                        // (lane 0's row is valid: the rows are a prefix)
        if (__all(!valid || mem == lead)) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long q = (unsigned long long)__double_as_longlong(__shfl_xor(__longlong_as_double((long long)p), o, 64));
                p = q > p ? q : p;
            }
            if (lane == 0 && p) atomicMax(M.maxbits + lead, p);
        } else if (valid && p) {
            atomicMax(M.maxbits + mem, p);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long q = (unsigned long long)__double_as_longlong(__shfl_xor(__longlong_as_double((long long)all), o, 64));
        all = q > all ? q : all;
    }
    if (lane == 0) sh[wave] = all;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) all = sh[w] > all ? sh[w] : all;
        if (all) atomicMax(M.maxbits + M.nb, all);
    }
}

// eps_b = c0 + c1 max_b (k_finish_regularizer's expression) per member, per column of the factor through the column's
// member, and the largest of them -- c0 + c1 (the stack's maximum), as the expression does not decrease in the maximum
__global__ __launch_bounds__(256) void k_member_eps(MemberStatusDev M, double c0, double c1, double* __restrict__ eps_top)
{
    const int len = M.N > M.nb ? M.N : M.nb;
    for (int k = blockIdx.x * 256 + (int)threadIdx.x; k < len; k += gridDim.x * 256) {
        if (k < M.N) M.eps_col[k] = c0 + c1 * __longlong_as_double((long long)M.maxbits[M.colmem[k]]);
        if (k < M.nb) M.eps_mem[k] = c0 + c1 * __longlong_as_double((long long)M.maxbits[k]);
        if (k == 0) eps_top[0] = c0 + c1 * __longlong_as_double((long long)M.maxbits[M.nb]);
    }
}

// behind the factorisation: column k of the factor marks its member if its pivot's reciprocal is not finite (the
// predicate of FactorArgs::flags[1], on the value the factor kernels stored)
__global__ __launch_bounds__(256) void k_member_pivot_scan(MemberStatusDev M, const double* __restrict__ Dinv)
{
    for (int k = blockIdx.x * 256 + (int)threadIdx.x; k < M.N; k += gridDim.x * 256)
        if (!isfinite(Dinv[k])) M.piv_bad[M.colmem[k]] = 1;
}

}  // namespace

void launch_member_regularizer(const MemberStatusDev& M, const double* Kval, const int* diag, double c0, double c1, double* eps_top,
                               hipStream_t st)
{
    hipLaunchKernelGGL(k_member_diag_max, dim3(batch_elem_grid(M.N)), dim3(256), 0, st, M, Kval, diag);
    hipLaunchKernelGGL(k_member_eps, dim3(batch_elem_grid(M.N > M.nb ? M.N : M.nb)), dim3(256), 0, st, M, c0, c1, eps_top);
}

void launch_member_pivot_scan(const MemberStatusDev& M, const double* Dinv, hipStream_t st)
{
    hipLaunchKernelGGL(k_member_pivot_scan, dim3(batch_elem_grid(M.N)), dim3(256), 0, st, M, Dinv);
}

void launch_member_residual(const SpmvDev& A, const double* Kval, const MemberIrDev& M, const double* b, const double* x, double* e,
                            bool first, hipStream_t st)
{
    const size_t S = (size_t)M.nwg + (size_t)M.nb;
    double* pe = first ? M.slots : M.slots + 2 * S;
    double* pb = first ? M.slots + S : nullptr;
    if (A.lanes_per_row == 8) hipLaunchKernelGGL(k_member_residual<8>, dim3(M.nwg), dim3(256), 0, st, A, Kval, M, b, x, e, pe, pb);
    else hipLaunchKernelGGL(k_member_residual<64>, dim3(M.nwg), dim3(256), 0, st, A, Kval, M, b, x, e, pe, pb);
    if (A.nlong > 0) {
        launch_residual_long_chunks(A, Kval, x, st);
        hipLaunchKernelGGL(k_member_long_finish, dim3((M.nb + 3) / 4), dim3(256), 0, st, A, M, b, e, pe, pb);
    }
}

void launch_member_ir_round(const MemberIrDev& M, int r, const int* flag_in, double* x, const double* dx, double* e, double abstol,
                            double reltol, double stop_ratio, int max_iter, double* readback, hipStream_t st)
{
    hipLaunchKernelGGL(k_member_ir_round, dim3(M.nwg), dim3(256), 0, st, M, r, flag_in, x, dx, e, abstol, reltol, stop_ratio, max_iter,
                       readback);
}

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
