// Host-only part of the data updates of level C (hipkkt_kkt_system_update_data_P / _A / _q / _b, include/hipkkt.h): the
// check of an (index, value) update's positions and the per-entry tables the update kernels read.  Plain C++ without a
// HIP header, so that both are tested without a GPU (tests/sanitize/data_update_driver.cpp).
#pragma once
#include <cstdint>
#include <vector>

namespace hipkkt {

// What is wrong with the k positions of an indexed update into a vector of `len` entries: nothing, a position outside
// [0, len), or a position named twice.  `pos` is the place IN index[] of the first offender (for a repeat: of its second
// occurrence in array order); `value` is index[pos].  Unsorted input is fine.  The reference applies repeats in order
// (data_updating.jl:196-211); a parallel scatter cannot, so they are refused.
enum class IndexFault { None, OutOfRange, Repeated };
struct IndexCheck {
    IndexFault fault = IndexFault::None;
    int64_t pos = -1, value = 0;
};
IndexCheck check_update_index(const int64_t* index, int64_t k, int64_t len);

// Row and column, in the matrix's own numbering, of every stored entry of P (triu, n x n) and of A (m x n), from K's
// triu CSC pattern and the entries' places in it (mapP / mapA of the assembly): K = [P A'; A -Hs], so a P entry sits at
// K(row, col) with row <= col < n and an A entry (i, j) at K(j, n + i).  ok = false (and `bad` = the first entry that
// lies outside its block) where a map does not point into the block it should.
struct EntryTables {
    std::vector<int> Prow, Pcol, Arow, Acol;
    bool ok = true;
    int64_t bad = -1;
};
EntryTables build_entry_tables(int n, int m, int N, const int64_t* colptr, const int* rowval, const int* mapP, int64_t nP,
                               const int* mapA, int64_t nA);

// ---- member cost scalings (hipkkt_kkt_system_set_equilibration_batch, hipkkt_kkt_system_data_norms_batch): on a stack
// of independent problems every member b has its own cost scaling c[b] (the reference computes c per problem:
// problemdata.jl:133-221).

// The first member whose c is not positive and finite (0, negative, inf, NaN), or -1 where all nb are fine.
int64_t check_member_costs(const double* c, int64_t nb);

// The member of every stored entry of P in the matrix's own numbering: Pmem[t] = xmem[Prow[t]], which the partition
// guarantees to equal xmem[Pcol[t]].  ok = false (and `bad` = the first offender) where a row or column lies outside
// [0, n), a member outside [0, nb), or an entry's row and column belong to different members -- the update kernel reads
// c through the ROW, and this is the check that the row's member is the entry's.
struct EntryMembers {
    std::vector<int> Pmem;
    bool ok = true;
    int64_t bad = -1;
};
EntryMembers build_entry_members(const int* Prow, const int* Pcol, int64_t nP, const int* xmem, int n, int nb);

// The word of the segmented norms a row's product is folded into, for the n x rows followed by the m z rows: x row i of
// member b -> 2 b (max |q dinv|), z row i of member b -> 2 b + 1 (max |b einv|).  A member's x rows and z rows are
// contiguous runs, so nearly every wave of 64 rows holds one word.  Empty where a member lies outside [0, nb).
std::vector<int> build_norm_slots(const int* xmem, int n, const int* zmem, int m, int nb);

}  // namespace hipkkt
