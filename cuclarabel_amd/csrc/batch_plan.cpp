// See batch_plan.hpp.  Host-only: compiled with -x c++, and by the sanitizer driver of tests/sanitize.
#include "batch_plan.hpp"

#include <algorithm>
#include <climits>

namespace hipkkt {

BatchChunks plan_batch_chunks(int nb, const int* x_off, const int* z_off, int chunk)
{
    BatchChunks C;
    C.wg_ptr.assign((size_t)nb + 1, 0);
    for (int b = 0; b < nb; ++b) {
        const int64_t rows = (x_off ? (int64_t)x_off[b + 1] - x_off[b] : 0) + (z_off ? (int64_t)z_off[b + 1] - z_off[b] : 0);
        for (int64_t first = 0; first < rows; first += chunk) {
            C.wg_mem.push_back(b);
            C.wg_first.push_back((int)first);
        }
        C.wg_ptr[(size_t)b + 1] = (int)C.wg_mem.size();
    }
    return C;
}

static std::string num(int64_t v) { return std::to_string(v); }

std::string plan_batch(int n, int m, int64_t nb64, const int64_t* x_off, const int64_t* z_off, const BatchCone* cones, int ncones,
                       const int64_t* colptr, const int* rowval, const int* long_rows, int nlong, BatchPlan& out)
{
    if (nb64 < 1) return "the number of members must be positive";
    if (nb64 > n) return "more members (" + num(nb64) + ") than x rows (" + num(n) + "): every member owns at least one";
    if (!x_off || !z_off) return "the offset arrays are NULL";
    const int nb = (int)nb64;
    // ---- the offsets
    if (x_off[0] != 0) return "x_off[0] is " + num(x_off[0]) + ", not 0";
    if (z_off[0] != 0) return "z_off[0] is " + num(z_off[0]) + ", not 0";
    for (int b = 0; b < nb; ++b) {
        if (x_off[b + 1] < x_off[b]) return "x_off decreases at member " + num(b);
        if (z_off[b + 1] < z_off[b]) return "z_off decreases at member " + num(b);
        if (x_off[b + 1] == x_off[b]) return "member " + num(b) + " has no x row";
        if (x_off[b + 1] > n) return "x_off of member " + num(b) + " ends past n = " + num(n);
        if (z_off[b + 1] > m) return "z_off of member " + num(b) + " ends past m = " + num(m);
    }
    if (x_off[nb] != n) return "x_off ends at " + num(x_off[nb]) + ", not at n = " + num(n);
    if (z_off[nb] != m) return "z_off ends at " + num(z_off[nb]) + ", not at m = " + num(m);
    // (with the rows of a member counted as a 32-bit sum below)
    if ((int64_t)n + m + nb > INT_MAX) return "n + m + nb does not fit the tables' 32-bit indices";
    BatchPlan& B = out;
    B = BatchPlan{};
    B.nb = nb;
    B.x_off.assign(x_off, x_off + nb + 1);
    B.z_off.assign(z_off, z_off + nb + 1);
    B.xmem.assign((size_t)n, 0);
    B.zmem.assign((size_t)m, 0);
    for (int b = 0; b < nb; ++b) {
        std::fill(B.xmem.begin() + B.x_off[b], B.xmem.begin() + B.x_off[b + 1], b);
        std::fill(B.zmem.begin() + B.z_off[b], B.zmem.begin() + B.z_off[b + 1], b);
    }
    // ---- the cones: each inside one member's z range; an empty cone goes with the member whose range it starts in
    B.cone_mem.assign((size_t)ncones, 0);
    B.soc_ptr.assign((size_t)nb + 1, 0);
    B.psd_ptr.assign((size_t)nb + 1, 0);
    B.degree.assign((size_t)nb, 0.0);
    {
        int b = 0;
        for (int c = 0; c < ncones; ++c) {
            const BatchCone& ci = cones[c];
            if (ci.off < 0 || ci.numel < 0 || (int64_t)ci.off + ci.numel > m) return "cone " + num(c) + " lies outside the z rows";
            if (ci.numel > 0) {
                b = B.zmem[(size_t)ci.off];
                if (B.zmem[(size_t)ci.off + ci.numel - 1] != b)
                    return "cone " + num(c) + " (rows " + num(ci.off) + " .. " + num((int64_t)ci.off + ci.numel - 1) +
                           ") crosses the boundary behind member " + num(b);
            }
            B.cone_mem[(size_t)c] = b;
            if (ci.kind == 2) ++B.soc_ptr[(size_t)b + 1];
            if (ci.kind == 3) ++B.psd_ptr[(size_t)b + 1];
            B.degree[(size_t)b] += ci.kind == 1 ? ci.numel : ci.kind == 2 ? 1 : ci.kind == 3 ? ci.dim : 0;
        }
        for (int k = 0; k < nb; ++k) { B.soc_ptr[(size_t)k + 1] += B.soc_ptr[(size_t)k]; B.psd_ptr[(size_t)k + 1] += B.psd_ptr[(size_t)k]; }
    }
    // ---- no entry of P or A couples two members
    for (int j = 0; j < n; ++j)
        for (int64_t q = colptr[j]; q < colptr[j + 1]; ++q) {
            const int i = rowval[q];
            if (i < 0 || i >= n) continue;
            if (B.xmem[(size_t)i] != B.xmem[(size_t)j])
                return "entry (" + num(i) + ", " + num(j) + ") of P couples member " + num(B.xmem[(size_t)i]) + " with member " +
                       num(B.xmem[(size_t)j]);
        }
    for (int r = 0; r < m; ++r)
        for (int64_t q = colptr[n + r]; q < colptr[n + r + 1]; ++q) {
            const int c = rowval[q];
            if (c < 0 || c >= n) continue;
            if (B.xmem[(size_t)c] != B.zmem[(size_t)r])
                return "entry (" + num(r) + ", " + num(c) + ") of A couples member " + num(B.zmem[(size_t)r]) + " (its row) with member " +
                       num(B.xmem[(size_t)c]) + " (its column)";
        }
    // ---- workgroups
    B.rows32 = plan_batch_chunks(nb, B.x_off.data(), B.z_off.data(), kBatchRowsResidual);
    B.rows256 = plan_batch_chunks(nb, B.x_off.data(), B.z_off.data(), kBatchRowsDots);
    B.z256 = plan_batch_chunks(nb, nullptr, B.z_off.data(), kBatchRowsCone);
    // ---- long rows by member (a counting sort: stable, so ascending inside a member)
    B.long_ptr.assign((size_t)nb + 1, 0);
    B.long_order.assign((size_t)nlong, 0);
    auto member_of = [&](int row) { return row < n ? B.xmem[(size_t)row] : B.zmem[(size_t)row - n]; };
    for (int t = 0; t < nlong; ++t) {
        if (long_rows[t] < 0 || (int64_t)long_rows[t] >= (int64_t)n + m) return "long row " + num(t) + " lies outside the image";
        ++B.long_ptr[(size_t)member_of(long_rows[t]) + 1];
    }
    for (int k = 0; k < nb; ++k) B.long_ptr[(size_t)k + 1] += B.long_ptr[(size_t)k];
    {
        std::vector<int> at(B.long_ptr.begin(), B.long_ptr.end() - 1);
        for (int t = 0; t < nlong; ++t) B.long_order[(size_t)at[(size_t)member_of(long_rows[t])]++] = t;
    }
    return "";
}

std::string plan_batch_image(int n, int m, int p, const BatchPlan& B, const BatchImageCone* cones, int ncones, const int* long_rows,
                             int nlong, int chunk, BatchImagePlan& out)
{
    if (n < 0 || m < 0 || p < 0 || (int64_t)n + m + p > INT_MAX) return "the image's row count does not fit 32 bits";
    if (chunk < 1) return "the chunk must be positive";
    const int nb = B.nb, N = n + m + p;
    if (nb < 1 || (int)B.xmem.size() != n || (int)B.zmem.size() != m || (int)B.cone_mem.size() != ncones)
        return "the partition does not belong to this image";
    if ((int64_t)N + nb > INT_MAX) return "N + nb does not fit the tables' 32-bit indices";
    BatchImagePlan& I = out;
    I = BatchImagePlan{};
    I.nb = nb; I.N = N; I.chunk = chunk;
    I.rowmem.assign((size_t)N, -1);
    for (int i = 0; i < n; ++i) I.rowmem[(size_t)i] = B.xmem[(size_t)i];
    for (int i = 0; i < m; ++i) I.rowmem[(size_t)n + i] = B.zmem[(size_t)i];
    for (int c = 0; c < ncones; ++c) {
        const BatchImageCone& ci = cones[c];
        if (ci.pwidth == 0) continue;
        if (ci.pwidth < 0 || ci.pcol < 0 || (int64_t)ci.pcol + ci.pwidth > p) return "cone " + num(c) + " has expansion rows outside the image";
        for (int t = 0; t < ci.pwidth; ++t) {
            int& r = I.rowmem[(size_t)n + m + ci.pcol + t];
            if (r >= 0) return "expansion row " + num(ci.pcol + t) + " belongs to two cones";
            r = B.cone_mem[(size_t)c];
        }
    }
    for (int i = n + m; i < N; ++i)
        if (I.rowmem[(size_t)i] < 0) return "expansion row " + num(i - n - m) + " belongs to no cone";
    // ---- the rows by member (a counting sort: stable, so ascending inside a member)
    I.img_ptr.assign((size_t)nb + 1, 0);
    for (int i = 0; i < N; ++i) ++I.img_ptr[(size_t)I.rowmem[(size_t)i] + 1];
    for (int k = 0; k < nb; ++k) I.img_ptr[(size_t)k + 1] += I.img_ptr[(size_t)k];
    I.img_rows.assign((size_t)N, 0);
    {
        std::vector<int> at(I.img_ptr.begin(), I.img_ptr.end() - 1);
        for (int i = 0; i < N; ++i) I.img_rows[(size_t)at[(size_t)I.rowmem[(size_t)i]]++] = i;
    }
    // ---- workgroups
    I.wg.wg_ptr.assign((size_t)nb + 1, 0);
    for (int b = 0; b < nb; ++b) {
        for (int64_t first = I.img_ptr[(size_t)b]; first < I.img_ptr[(size_t)b + 1]; first += chunk) {
            I.wg.wg_mem.push_back(b);
            I.wg.wg_first.push_back((int)first);
        }
        I.wg.wg_ptr[(size_t)b + 1] = (int)I.wg.wg_mem.size();
    }
    // ---- long rows by member
    I.long_ptr.assign((size_t)nb + 1, 0);
    I.long_order.assign((size_t)nlong, 0);
    for (int t = 0; t < nlong; ++t) {
        if (long_rows[t] < 0 || long_rows[t] >= N) return "long row " + num(t) + " lies outside the image";
        ++I.long_ptr[(size_t)I.rowmem[(size_t)long_rows[t]] + 1];
    }
    for (int k = 0; k < nb; ++k) I.long_ptr[(size_t)k + 1] += I.long_ptr[(size_t)k];
    {
        std::vector<int> at(I.long_ptr.begin(), I.long_ptr.end() - 1);
        for (int t = 0; t < nlong; ++t) I.long_order[(size_t)at[(size_t)I.rowmem[(size_t)long_rows[t]]]++] = t;
    }
    return "";
}

std::string plan_column_members(int N, int nb, const int* perm, size_t nperm, const int* rowmem, size_t nrowmem, std::vector<int>& colmem)
{
    if (N < 0 || nb < 1) return "the column table needs N >= 0 and at least one member";
    if (nperm != (size_t)N) return "the permutation has " + num((int64_t)nperm) + " entries, the image has " + num(N) + " rows";
    if (nrowmem != (size_t)N) return "the row table has " + num((int64_t)nrowmem) + " entries, the image has " + num(N) + " rows";
    for (int i = 0; i < N; ++i)
        if (rowmem[i] < 0 || rowmem[i] >= nb) return "row " + num(i) + " of the image belongs to no member below " + num(nb);
    std::vector<char> seen((size_t)N, 0);
    colmem.assign((size_t)N, 0);
    for (int k = 0; k < N; ++k) {
        const int r = perm[k];
        if (r < 0 || r >= N) return "column " + num(k) + " of the factor maps to row " + num(r) + " outside the image";
        if (seen[(size_t)r]) return "row " + num(r) + " of the image appears twice in the permutation";
        seen[(size_t)r] = 1;
        colmem[(size_t)k] = rowmem[r];
    }
    return "";
}

}  // namespace hipkkt
