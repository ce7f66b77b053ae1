// libhipkkt.so: the C ABI of include/hipkkt.h over the symbolic analysis (symbolic.cpp), the KKT
// assembly (kkt_assembly.cpp) and the device kernels (kernels.hip).
#include "../../include/hipkkt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "kkt_assembly.hpp"
#include "symbolic.hpp"
#include "knobs.hpp"
#include "schedule.hpp"
#include "engine_tables.hpp"
#include "data_update.hpp"
#include "iterate_rows.hpp"
#include "batch_plan.hpp"

namespace hipkkt {

static thread_local std::string g_last_error;

struct ArgError : std::runtime_error { using std::runtime_error::runtime_error; };

#define HIP_CHECK(expr)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            throw HipError(std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    } while (0)

template <class T>
struct DBuf {
    T* p = nullptr;
    size_t n = 0;
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { if (p) (void)hipFree(p); }
    void alloc(size_t count)
    {
        if (p) { (void)hipFree(p); p = nullptr; }
        n = count;
        HIP_CHECK(hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T)));
    }
    void zero(hipStream_t st) { HIP_CHECK(hipMemsetAsync(p, 0, std::max<size_t>(n, 1) * sizeof(T), st)); }
    template <class V>
    void upload(const std::vector<V>& v)
    {
        static_assert(sizeof(V) == sizeof(T), "element size mismatch");
        alloc(v.size());
        if (!v.empty()) HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    }
};

static constexpr int kMaxNR = 4;          // right-hand sides the single-column solve path takes in one sweep (1, 2 or 4)
// (environment settings: knobs.hpp -- one table, read once per process)

// WHAT MAY RUN BESIDE WHAT ON ONE DEVICE, ACROSS HANDLES.  Three mechanisms of this library put kernels on the device
// whose workgroups WAIT for other workgroups: the factorisation's overlap mode (panel workgroups that hold a CU each
// while they wait for their children's tiles on ANOTHER stream; tiles behind a gate: enqueue_factor), the persistent
// top-of-tree sweep kernel (all its workgroups resident: k_top_solve) and the chained sweep launches (a workgroup waits
// for lower-index workgroups of its own grid: chain_kernels.hip).  Each is safe beside kernels that end by themselves;
// none is safe beside another handle's waiting kernel, and the overlap mode -- whose waits cross streams -- is not even
// safe beside another handle's plain cross-stream dependencies.  All three were seen in round 4 as 50 ms give-ups with
// two and three handles on their own streams:
//   * handle 0's persistent kernel had part of its workgroups resident, the rest waiting for CUs held by handle 1's
//     resident panels, which waited for tiles behind their gate, which waited for handle 1's remaining panels, which needed
//     the CUs handle 0's workgroups sat on;
//   * a chained grid's workgroups are dealt to the eight XCDs round-robin and each XCD starts its share in order, so the
//     grid's lowest unfinished workgroup may be the one NOT yet resident on an XCD whose CUs another handle's waiting
//     workgroups hold, while its own resident workgroups hold the CUs those are waiting for;
//   * HIP maps a process's streams onto a few hardware queues, and a queue runs its packets in order: handle B's main
//     stream waiting (an event) for B's W-formation kernel, parked in the queue behind handle A's tile kernel, which waits
//     for A's panel kernel, which sits in the queue behind B's wait.
// So per device the operations that are not plain single-stream work are classed and admitted under a mutex:
//   X  overlapped factorisation (in-kernel waits across streams)    admitted iff every OTHER handle is idle (no M, S, X in flight)
//                                                                     and has been for 20 ms (it is not in a loop beside this one:
//                                                                     an X in flight takes the others' M away, which costs a busy
//                                                                     handle more than the mode gives -- 64 SOCPs on three handles:
//                                                                     3.7 k problems/s with X admitted on idleness alone, 4.4 k so)
//   S  sweep through the persistent / chained kernels                admitted iff no other handle has an S or X in flight
//   M  factorisation with side-stream W formation (no in-kernel wait) admitted iff no other handle has an X in flight
// "in flight" = enqueued and not yet past the handle's three events (main, tile and W-formation stream); handles that
// share one stream never conflict (the stream serialises them).  An operation that is not admitted is not switched off:
// THAT factorisation runs level by level on the main stream alone, THAT sweep level by level -- kernels and packets that
// depend on earlier work of their own stream only, safe beside anything.  Under contention (bench.py --mode problems:
// three busy handles) X is rarely admitted and the handles settle on M + one S at a time, which is what round 3 reached
// with HIPKKT_FACTOR_OVERLAP=0 set by hand.  A handle alone on its device (the common case) pays a mutex and no event;
// the first time a second handle appears on a device the device is synchronised once, so that no operation without
// events is in flight.
enum DevOp { kOpNone = 0, kOpM = 1, kOpS = 2, kOpX = 3 };
struct DevRec {
    const void* eng = nullptr;
    hipStream_t stream = nullptr;
    int kind = kOpNone;                          // strongest class among the handle's operations still in flight
    bool enqueuing = false;                      // between admission and the recording of its events
    hipEvent_t done_main = nullptr, done_tiles = nullptr, done_side = nullptr;
    std::chrono::steady_clock::time_point last_seen{};   // the handle's last factorisation / sweep call (admitted or not)
};
struct DevState { std::vector<DevRec> recs; };
static std::mutex g_dev_mu;
static std::map<int, DevState> g_dev;

// ------------------------------------------------------------------------------------
//  The numeric engine shared by both API levels
// ------------------------------------------------------------------------------------
class LDLEngine {
public:
    Symbolic S;
    hipStream_t stream = nullptr;
    int device_id = 0;
    double dyn_eps, dyn_delta;

    LDLEngine(int N, const int64_t* colptr, const int64_t* rowval, int base, const std::vector<int>& dsigns,
              const hipkkt_settings& st)
    {
        SymbolicOptions opt;
        opt.ordering = st.ordering;
        opt.amd_dense_scale = st.amd_dense_scale > 0 ? st.amd_dense_scale : 1.5;
        if (st.nd_leaf_size > 0) opt.nd_leaf_size = st.nd_leaf_size;
        opt.user_perm = st.user_perm;
        apply_knobs(opt);
        // user_perm arrives in the caller's index base; analyse() applies `base` to it
        analyse(N, colptr, rowval, base, opt, S);
        dyn_eps = st.dynamic_regularization_eps;
        dyn_delta = st.dynamic_regularization_delta;
        // what the device contributes to the schedule: its CU count (256 where the query fails) and the persistent
        // kernels' occupancy answers, asked where schedule.cpp needs them
        {
            int d = 0;
            hipDeviceProp_t prop;
            if (hipGetDevice(&d) == hipSuccess && hipGetDeviceProperties(&prop, d) == hipSuccess) dev.n_cus = prop.multiProcessorCount;
            else (void)hipGetLastError();
        }
        dev.top_solve_capacity = [](size_t lds, bool tall) { return top_solve_capacity(lds, tall); };
        dev.top_solve_capacity_nr = [](size_t lds_total, int nr) { return top_solve_capacity_nr(lds_total, nr); };
        dev.top_solve_sliced_capacity = [](size_t lds, int nr) { return top_solve_sliced_capacity(lds, nr); };
        sch = build_schedule(S, dev, opt.panel_cap, std::max(1, opt.panel_max_slices));
        upload(dsigns);
        if (knobs().verbose) {
            int nblock = 0, nsl_fronts = 0, ov_slices = 0;
            for (const Launch& L : sch.launches) if (!L.small) { nblock += L.count; nsl_fronts += L.nsliced; }
            if (overlap_wanted()) for (size_t q = sch.ov_first; q < sch.launches.size(); ++q) ov_slices += sch.launches[q].slice_count;
            std::fprintf(stderr, "[hipkkt] N %d, %d supernodes in %zu levels (%zu launches), %d block-class fronts, %d of them in "
                         "%zu row slices; persistent solve set: last %zu launches, %d fronts on %d workgroups, %d (front, slice) tasks; "
                         "factorisation overlap: last %zu launches (%d row slices in them); pulled leaves: %lld (%lld terms)\n",
                         S.N, S.nsuper, S.levels.size(), sch.launches.size(), nblock, nsl_fronts, sch.slice_list.size(), sch.top_launches,
                         sch.top_count, sch.top_ntask > 0 ? sch.top_sgrid : sch.top_grid, sch.top_ntask, overlap_wanted() ? sch.launches.size() - sch.ov_first : (size_t)0,
                         ov_slices, (long long)n_factor_pulled, (long long)n_factor_terms);
            {
                int ntall_all = 0;
                for (const Launch& L : sch.launches) ntall_all += L.ntall;
                if (ntall_all) std::fprintf(stderr, "[hipkkt] %d fronts too tall for the block sweep kernels (k_fwd_tall / k_bwd_tall)\n", ntall_all);
            }
            if (knobs().verbose >= 2)
                for (size_t q = 0; q < sch.launches.size(); ++q) {
                    const Launch& L = sch.launches[q];
                    int fmin = 1 << 30, ncmin = 1 << 30;
                    double flops = 0;
                    for (int t = L.begin; t < L.begin + L.count; ++t) {
                        const int sn = sch.sched[(size_t)t], nc = S.sn_start[sn + 1] - S.sn_start[sn], f = front_size(sn);
                        fmin = std::min(fmin, f); ncmin = std::min(ncmin, nc);
                        flops += (double)nc * (f - nc) * (f - nc) + (double)nc * nc * (f - nc) + (double)nc * nc * nc / 3;
                    }
                    // (the tile kernel's build: launch_schur's own decision, for an admitted overlapped factorisation)
                    const bool ov = overlap_wanted() && q >= sch.ov_first;
                    std::fprintf(stderr, "[hipkkt] launch %zu level %d: %d fronts (%s), f %d..%d, nc %d..%d, %d sliced into %d, %d tiles (%d columns deep on average), %.3f GF, tile kernel: %s\n",
                                 q, L.level, L.count, L.small ? "one wave" : "block", fmin, L.fmax, ncmin, L.ncmax, L.nsliced, L.slice_count,
                                 L.ntiles, L.tile_nc, flops * 1e-9, schur_build_name(schur_build(ov, L.ntiles, L.tile_nc)));
                }
            if (overlap_wanted())
                for (size_t q = sch.ov_first; q < sch.launches.size(); ++q)
                    std::fprintf(stderr, "[hipkkt] overlap admission: launch %zu: %d panel workgroups, %d tiles behind a gate, %d CUs\n", q,
                                 sch.ov_group_of[q] >= 0 ? sch.ov_groups[(size_t)sch.ov_group_of[q]].count : sch.launches[q].count - sch.launches[q].nsliced + sch.launches[q].slice_count,
                                 sch.launches[q].ntiles, dev.n_cus);
        }
    }

    // Both sequences are static (no pivoting, fixed structure), so they can be captured once into
    // hipGraphs and replayed (HIPKKT_GRAPH=1), with the T = L11^{-1} kernels on a parallel branch.
    void factor(const double* d_Kval, const double* d_eps)
    {
        const bool want_stamps = knobs().stamps;
        // measured on MI355X/ROCm 7.2: replay is ~25 % slower than eager launches for these ~100-node
        // chains (the work is GPU-latency-bound, not host-bound), so graphs are opt-in
        const bool no_graph = !knobs().graph;
        // (a per-column regulariser is not part of a captured graph's key: such a factorisation is enqueued)
        if (want_stamps || no_graph || eps_col || n_factor_calls++ == 0) {
            enqueue_factor(d_Kval, d_eps, stream, nullptr, want_stamps);
            return;
        }
        auto key = std::make_pair((const void*)d_Kval, (const void*)d_eps);
        auto it = factor_graphs.find(key);
        if (it == factor_graphs.end()) {
            ensure_capture_streams();
            HIP_CHECK(hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal));
            enqueue_factor(d_Kval, d_eps, cap_stream, cap_side, false);
            hipGraph_t g;
            HIP_CHECK(hipStreamEndCapture(cap_stream, &g));
            hipGraphExec_t ex;
            HIP_CHECK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
            HIP_CHECK(hipGraphDestroy(g));
            it = factor_graphs.emplace(key, ex).first;
        }
        HIP_CHECK(hipGraphLaunch(it->second, stream));
    }

    // d_b, d_x in the caller's (original) ordering; may alias.  allow_top: the caller will synchronise and ask
    // top_gave_up() afterwards (and repeat the solve if so); otherwise the launch-per-level path is used.
    // nr = 1, 2 or 4 right-hand sides in ONE sweep (column c at d_b + c ldb / d_x + c ldx): see supports_nr().
    void solve(const double* d_b, double* d_x, bool allow_top = false, int nr = 1, int64_t ldb = 0, int64_t ldx = 0)
    {
        const bool no_graph = !knobs().graph;
        if (nr > 1) {
            if (!supports_nr(nr)) throw ArgError("solve: this structure takes one right-hand side per sweep");
            reserve_nr(nr);
        }
        if (no_graph || nr > 1 || n_solve_calls++ == 0) {
            // the persistent kernel AND the chained launches hold workgroups that wait for other workgroups: class S
            // (DevOp); not admitted, this sweep goes level by level
            const bool waits = allow_top && ((!top_disabled && sch.top_launches > 0) || (!chain_disabled && sch.chain_from < sch.launches.size()));
            const bool tok = waits && claim_dev(kOpS);
            TokenRelease rel{this, tok};
            enqueue_solve(d_b, d_x, stream, tok, nr, ldb, ldx, tok);
            if (tok) { rel.on = false; dev_enqueued(true); }
            return;
        }
        auto key = std::make_pair((const void*)d_b, (const void*)d_x);
        auto it = solve_graphs.find(key);
        if (it == solve_graphs.end()) {
            ensure_capture_streams();
            HIP_CHECK(hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal));
            enqueue_solve(d_b, d_x, cap_stream, false, 1, 0, 0);
            hipGraph_t g;
            HIP_CHECK(hipStreamEndCapture(cap_stream, &g));
            hipGraphExec_t ex;
            HIP_CHECK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
            HIP_CHECK(hipGraphDestroy(g));
            it = solve_graphs.emplace(key, ex).first;
        }
        HIP_CHECK(hipGraphLaunch(it->second, stream));
    }
    bool supports_nr(int nr) const { return hipkkt::supports_nr(sch, nr); }

    // nrhs right-hand sides at once: column j of d_B at stride ldb, of d_X at stride ldx (may alias d_B).
    // Every level is one launch (grid.y = block of 16 columns, 8 for the one-wave fronts): the per-level latency
    // that bounds a single solve is paid once for all columns, and every entry of the solve matrices a workgroup
    // fetches is used for all of its columns (solve_kernels.hip, "several right-hand sides").
    void solve_multi(const double* d_B, int64_t ldb, double* d_X, int64_t ldx, int nrhs)
    {
        if (nrhs <= 0) return;
        if (nrhs == 1) { solve(d_B, d_X); return; }
        const int KP = multi_prepare(nrhs);
        launch_permute_in(d_B, ldb, xp_m.p, KP, d_iperm.p, S.N, nrhs, stream);
        multi_sweeps(KP);
        launch_permute_out(d_X, ldx, xp_m.p, KP, d_iperm.p, S.N, nrhs, stream);
        HIP_CHECK(hipGetLastError());
    }
    // the same with ROW-major vectors, N x KP (KP a multiple of 16, padding columns zero); d_X may alias d_B;
    // d_add (nullable, same layout): X = K^{-1} B + add, formed while the solution is permuted back
    void solve_multi_rm(const double* d_B, double* d_X, int KP, const double* d_add = nullptr)
    {
        if (KP <= 0 || (KP & 15)) throw ArgError("solve_multi_rm: KP must be a positive multiple of 16");
        multi_prepare(KP);
        // (r03: the two row permutations -- 2 x (read + write) of N x KP per sweep pair, 5 GB at 512 columns -- are gone: the
        //  forward kernels read a front's own rows of B through the permutation, the backward kernels store the solution
        //  (+ add) to the caller's rows beside the tree-ordered copy the descendants read)
        multi_sweeps(KP, d_B, d_X, d_add);
        HIP_CHECK(hipGetLastError());
    }

private:
    int multi_prepare(int nrhs)
    {
        const int KP = (nrhs + 15) & ~15;
        if (KP / 8 > 65535) throw ArgError("solve_multi: too many right-hand sides per call");
        {   // the block kernels' grid.y is (fronts of a launch / 8) x (column blocks of 16)
            int64_t widest = 0;
            for (const Launch& L : sch.launches) if (!L.small) widest = std::max<int64_t>(widest, (L.count + 7) / 8);
            if (widest * (KP / 16) > 65535) throw ArgError("solve_multi: too many right-hand sides per call for this structure (split the call)");
        }
        wait_w(stream);
        if ((size_t)KP > multi_cap) {
            xp_m.alloc((size_t)S.N * KP);
            uvec_m.alloc(std::max<size_t>(S.rows.size(), 1) * KP);
            multi_cap = (size_t)KP;
        }
        if (!d_iperm.p) d_iperm.upload(S.iperm);
        return KP;
    }
    void multi_sweeps(int KP, const double* b_rm = nullptr, double* out_rm = nullptr, const double* add_rm = nullptr)
    {
        SolveArgs a;
        a.T = tree();
        a.fronts = fronts.p;
        a.tinv = tinv.p;
        a.Dinv = Dinv.p;
        a.b = b_rm;                  // (row-major N x KP in the caller's row order, or null: xp_m holds the permuted right-hand sides)
        a.out = out_rm;
        a.add = add_rm;
        a.xp = xp_m.p;
        a.uvec = uvec_m.p;
        a.ld_b = a.ld_out = a.ld_xp = a.ld_uvec = 0;
        a.top_limit = 5000000;       // (the multi-column path has no persistent kernel)
        a.tk_pos = nullptr; a.tk_sl = nullptr; a.tbase = nullptr; a.xf = nullptr; a.chain_cnt = nullptr; a.recs = nullptr; a.tall_ws = nullptr;
        if (knobs().verbose) {       // the instances this call takes (launch_shapes.hpp: multi_shape)
            const MultiShape ms = multi_shape(KP, knobs().multi_vec, knobs().multi_ct);
            std::fprintf(stderr, "[hipkkt] many-column sweep: KP %d entry %s add %d wave_v %d leaf_v %d block_bs %d block_ct %d pull_rows %d\n",
                         KP, b_rm ? "rm" : "cm", add_rm ? 1 : 0, ms.wave_v, ms.leaf_v, ms.block_bs, ms.block_ct, n_pull_rows);
        }
        launch_pull_leaves_multi(a, n_pull_rows, KP, stream);        // (the pulled leaves' terms, summed per receiving row)
        for (const Launch& L : sch.launches) launch_fwd_multi(a, L.begin, L.count, L.small, L.ncmax, KP, stream);
        for (size_t q = sch.launches.size(); q-- > 0;) {
            const Launch& L = sch.launches[q];
            launch_bwd_multi(a, L.begin, L.count, L.small, L.ncmax, KP, stream, L.level == 0);
        }
    }

public:
    ~LDLEngine()
    {
        engine_gone();
        for (auto& kv : factor_graphs) (void)hipGraphExecDestroy(kv.second);
        for (auto& kv : solve_graphs) (void)hipGraphExecDestroy(kv.second);
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
        if (cap_side) (void)hipStreamDestroy(cap_side);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (ev_join2) (void)hipEventDestroy(ev_join2);
        if (ev_side) (void)hipEventDestroy(ev_side);
        if (ov_stream) (void)hipStreamDestroy(ov_stream);
        if (ev_ov_fork) (void)hipEventDestroy(ev_ov_fork);
        if (ev_ov_join) (void)hipEventDestroy(ev_ov_join);
        if (ev_dev_done) (void)hipEventDestroy(ev_dev_done);
    }

private:
    std::map<std::pair<const void*, const void*>, hipGraphExec_t> factor_graphs, solve_graphs;
    hipStream_t cap_stream = nullptr, cap_side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr, ev_side = nullptr;
    long n_factor_calls = 0, n_solve_calls = 0;

    void ensure_capture_streams()
    {
        if (cap_stream) return;
        HIP_CHECK(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
        HIP_CHECK(hipStreamCreateWithFlags(&cap_side, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&ev_join2, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&ev_side, hipEventDisableTiming));
    }

    // Do two streams really run side by side?  HIP deals a process's streams to a few hardware queues, and two streams on
    // one queue execute in submission order: the side stream's W formation would then sit in the middle of the
    // factorisation (seen: cfg2's 1.75 ms became 2.69 in a process that had created a few streams before), the tile
    // stream's kernels would not overlap their panels.  A kernel on `a` waits up to 2 ms for a kernel submitted AFTER it
    // on `b` (factor_kernels.hip, launch_concurrency_probe).
    bool streams_concurrent(hipStream_t a, hipStream_t b)
    {
        int* w = flags.p + 8;
        launch_zero_ints(w, 2, a);
        HIP_CHECK(hipStreamSynchronize(a));
        HIP_CHECK(hipStreamSynchronize(b));
        launch_concurrency_probe(w, a, b);
        int seen[2] = {0, 0};
        HIP_CHECK(hipMemcpyAsync(seen, w, sizeof(seen), hipMemcpyDeviceToHost, a));
        HIP_CHECK(hipStreamSynchronize(a));
        HIP_CHECK(hipStreamSynchronize(b));
        return seen[1] != 0;
    }
    // A stream that runs beside every stream of `beside`: `have` if it does (or nullptr: create one), else new streams are
    // tried -- up to six, the rejected ones held until the search ends so that the next creation lands on another queue.
    // *ok says whether the search succeeded; without success the last candidate is returned (everything still works
    // on a shared queue, in submission order).
    template <typename Create>
    hipStream_t stream_beside(hipStream_t have, const std::vector<hipStream_t>& beside, Create&& create, bool* ok)
    {
        std::vector<hipStream_t> rejected;
        hipStream_t cand = have;
        *ok = false;
        for (int attempt = 0; attempt < 6; ++attempt) {
            if (!cand && create(&cand) != hipSuccess) { (void)hipGetLastError(); cand = nullptr; break; }
            bool good = true;
            for (hipStream_t o : beside) good = good && streams_concurrent(o, cand);
            if (good) { *ok = true; break; }
            if (attempt == 5) break;
            rejected.push_back(cand);
            cand = nullptr;
        }
        if (!cand && !rejected.empty()) { cand = rejected.back(); rejected.pop_back(); }
        for (hipStream_t r : rejected) { (void)hipStreamSynchronize(r); (void)hipStreamDestroy(r); }
        return cand;
    }
    hipStream_t sides_for = (hipStream_t)(-1);     // the main stream the side / tile streams were chosen for
    bool side_concurrent = false;
    // (eager path only) the W-formation stream and the tile stream, each beside the main stream and beside each other
    void choose_side_streams(hipStream_t st, bool want_tiles)
    {
        if (sides_for == st && (!want_tiles || ov_stream || ov_disabled)) return;
        wait_w(st);
        auto plain = [](hipStream_t* out) { return hipStreamCreateWithFlags(out, hipStreamNonBlocking); };
        const bool new_main = sides_for != st;
        // The tile stream first: created before the capture / W-formation streams, as it always was (with the W-formation
        // stream created first the factorisation of cfg2 measured 13 us longer: which hardware queue a stream lands on
        // follows the order of creation, and the queues are not served alike)
        if (want_tiles && !ov_disabled && (new_main || !ov_stream)) {
            // (HIPKKT_OV_CU_MASK=1 confines the tile stream to every other CU.  Measured: on this stack a CU-masked
            // stream slows EVERY stream of the process down as if all of them were masked -- residual 0.032 -> 0.054 ms,
            // sweep 0.29 -> 0.37 ms -- so the default is a plain stream.)
            const bool cu_mask = knobs().ov_cu_mask;
            hipDeviceProp_t prop;
            HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
            std::vector<uint32_t> mask((size_t)std::max((prop.multiProcessorCount + 31) / 32, 1), 0x55555555u);
            auto masked = [&](hipStream_t* out) { return hipExtStreamCreateWithCUMask(out, (uint32_t)mask.size(), mask.data()); };
            const bool had = ov_stream != nullptr;
            std::vector<hipStream_t> beside{st};
            if (cap_side && !new_main) beside.push_back(cap_side);           // (a W-formation stream already chosen for st)
            if (cu_mask) ov_stream = stream_beside(ov_stream, beside, masked, &ov_concurrent);
            else ov_stream = stream_beside(ov_stream, beside, plain, &ov_concurrent);
            if (!ov_stream) {
                ov_disabled = true;
                std::fprintf(stderr, "[hipkkt] no stream for the Schur tiles: factorisation overlap off\n");
            } else if (!had) {
                HIP_CHECK(hipEventCreateWithFlags(&ev_ov_fork, hipEventDisableTiming));
                HIP_CHECK(hipEventCreateWithFlags(&ev_ov_join, hipEventDisableTiming));
            }
            if (ov_stream && !ov_concurrent && knobs().verbose)
                std::fprintf(stderr, "[hipkkt] the main and the tile stream share a hardware queue: no merged panel kernel for this handle\n");
        }
        ensure_capture_streams();
        if (new_main) {
            std::vector<hipStream_t> beside{st};
            if (ov_stream) beside.push_back(ov_stream);
            cap_side = stream_beside(cap_side, beside, plain, &side_concurrent);
            if (!side_concurrent && knobs().verbose)
                std::fprintf(stderr, "[hipkkt] no stream beside the main stream for the W formation: it will run in submission order\n");
        }
        sides_for = st;
    }

    // side != nullptr: put the T = L11^{-1} kernels on that stream, forked after each level's panels
    void enqueue_factor(const double* d_Kval, const double* d_eps, hipStream_t st, hipStream_t side, bool want_stamps)
    {
        wait_w(st);                  // (a refactorisation without a solve in between: the side stream still reads the fronts)
        if (ov_join_pending) {
            // the previous factorisation's tile stream (see the end of the overlapped launches below) before its counters
            // and update blocks are touched again
            if (side) HIP_CHECK(hipEventSynchronize(ev_ov_join));        // (a stream being captured cannot wait for it)
            else HIP_CHECK(hipStreamWaitEvent(st, ev_ov_join, 0));
            ov_join_pending = false;
        }
        ZeroList zl;
        zl.add(flags.p, 3);
        // overlap mode (eager launches only): the top launches' Schur tiles on their own stream, ordered by counters
        // in memory instead of kernel boundaries.  On by default (HIPKKT_FACTOR_OVERLAP=0 turns it off).  Measured on cfg2:
        // the tiles hide completely behind the panels (a top level costs its panel kernel instead of panel + tiles:
        // factorisation 1.85 -> 1.79 ms); it pays since the solve matrices W are formed early enough on the side stream
        // (3.43 -> 3.365 ms per step; with the round's earlier, slower W formation the first sweep waited for W by as
        // much as the factorisation ended earlier).
        const bool want_ov = overlap_wanted();
        const bool use_ov = want_ov && !side && !want_stamps && !ov_disabled && sch.ov_first < sch.launches.size();
        // Whatever this factorisation does on more than ONE stream needs admission (DevOp): the overlap mode (class X:
        // its kernels wait across streams) or, failing that, the side stream's W formation with its fork / join events
        // (class M).  Not admitted, it keeps to its main stream, where every packet depends on earlier packets of the same
        // stream only.
        const bool no_overlap = knobs().no_overlap;
        const bool side_w = !side && !no_overlap && !want_stamps && sch.late_launches > 0 && sch.late_launches < sch.launches.size();
        const bool tok_x = use_ov && claim_dev(kOpX);
        const bool tok = tok_x || (side_w && claim_dev(kOpM));
        TokenRelease ov_release{this, tok};      // (the "enqueuing" mark ends with this call, however it ends)
        // the side streams (W formation, Schur tiles) are chosen once per main stream, each probed to run BESIDE it.  The
        // tile stream only once an overlapped factorisation has been admitted: a stream that exists changes which
        // hardware queues the process's other streams share (three busy handles, each with an idle tile stream: 3.7 k
        // problems/s instead of 4.2 k)
        if (!side && !want_stamps) choose_side_streams(st, tok_x);
        const bool ov_on = tok_x && !ov_disabled && ov_stream != nullptr;
        // The merged panel kernels of the narrow top (below) wait for tile kernels that are submitted BEHIND them: that
        // needs the two streams on different hardware queues (ov_concurrent: choose_side_streams' probe; seen without it,
        // eight handles in one process: two of them waited for their 50 ms bound).  Without concurrency every level keeps
        // its own panel kernel, whose waits only ever look at work submitted earlier (panel L, tiles L, panel L + 1, ...:
        // correct on one queue as well).
        // (the merged kernels only where the two streams run side by side)
        auto group_of = [&](size_t q) -> const MergeGroup* {
            return (ov_concurrent && q < sch.ov_group_of.size() && sch.ov_group_of[q] >= 0) ? &sch.ov_groups[(size_t)sch.ov_group_of[q]] : nullptr;
        };
        const size_t merge_from = (ov_concurrent && !sch.ov_groups.empty()) ? sch.ov_groups.back().first : ~(size_t)0;
        if (ov_on) {
            zl.add(d_ov_prog.p, S.nsuper);
            zl.add(d_ov_done.p, S.nsuper);
            if (!sch.slice_list.empty()) zl.add(d_ov_sprog.p, (int)sch.slice_list.size());
            zl.add(d_ov_started.p, (int)sch.launches.size());
        }
        launch_zero_ints_multi(zl, st);
        FactorArgs a;
        a.T = tree();
        a.Kval = d_Kval;
        a.eps = d_eps;
        a.eps_col = d_eps ? eps_col : nullptr;
        a.fronts = fronts.p;
        a.upd = upd.p;
        a.Dinv = Dinv.p;
        a.flags = flags.p;
        a.dyn_eps = dyn_eps;
        a.dyn_delta = dyn_delta;
        a.ov_prog = d_ov_prog.p; a.ov_done = d_ov_done.p; a.ov_ntiles = d_ov_ntiles.p; a.ov = 0;
        a.ov_sprog = d_ov_sprog.p; a.ov_sbase = d_ov_sbase.p;
        a.ov_started = d_ov_started.p; a.ov_slot = 0;
        const long long ov_limit = knobs().ov_test_limit;
        a.ov_limit = ov_limit;
        a.stamps = nullptr;
        a.stamp_row = 0;
        if (want_stamps) {
            if (!stamps.p) { stamps.alloc(sch.launches.size() * 16); }
            stamps.zero(st);
            a.stamps = (long long*)stamps.p;
        }
        int li = 0;
        bool forked = false;
#ifdef HIPKKT_EXPERIMENTS
        // EXPERIMENT (timing only; without the gate the overlap mode's forward progress rests on submission order again)
        static const bool no_gate = std::getenv("HIPKKT_EXPERIMENT_NO_GATE") != nullptr;
#else
        constexpr bool no_gate = false;
#endif
#ifdef HIPKKT_EXPERIMENTS
        // EXPERIMENT (timing only, wrong results unless K stays the same between factorisations; compiled in only with
        // -DHIPKKT_EXPERIMENTS, never in the default build): skip W formation after n factorisations
        static const int skip_w_after = std::getenv("HIPKKT_EXPERIMENT_SKIP_WINV") ? std::atoi(std::getenv("HIPKKT_EXPERIMENT_SKIP_WINV")) : -1;
        const bool skip_w = skip_w_after >= 0 && n_skipw_calls++ >= skip_w_after;
#else
        const bool skip_w = false;
#endif
        // (every W formation of this factorisation goes through form_w)
        auto form_w = [&](const int* list, int count, int ncmax, hipStream_t on, int max_blocks) {
            const size_t i0 = (size_t)(list - d_tinv_list.p);
            const int nsmall = i0 + (size_t)count < sch.tinv_small_prefix.size() ? sch.tinv_small_prefix[i0 + (size_t)count] - sch.tinv_small_prefix[i0] : 0;
            if (!skip_w) launch_tinv(a.T, fronts.p, tinv.p, list, count, ncmax, on, max_blocks, nsmall);
        };
        // eager mode: once the tree narrows to its top levels most CUs idle, so the solve matrices
        // W = [T; M] of everything below are formed on a side stream meanwhile (HIPKKT_NO_OVERLAP=1 disables)
        const size_t nl = sch.launches.size();
        const size_t first_top = (tok && side_w) ? nl - sch.late_launches : nl;
        bool eager_fork = false;
        int w_done = 0;
        for (size_t q = 0; q < nl; ++q) {
            const Launch& L = sch.launches[q];
            a.stamp_row = li++;
            // fork points of the side stream: a few levels before the narrow top (the bulk of the fronts), at the narrow
            // top, and a few levels before the root -- behind the tree only the last levels' handful of fronts is left,
            // which the next sweep's bottom levels hide
            // (with the top launches' panels merged into one kernel, the last fork sits in front of that kernel: an event
            //  behind it would wait for the whole top of the tree)
            // (with merged panel kernels every run's first launch is a fork point: the W of everything factorised so far is
            //  formed beside the run.  With the last run's start as the only late fork, cfg3 and cfg5 formed the W of their
            //  widest levels behind the tree and the first sweep waited for it: 0.1 and 0.37 ms per step)
            const bool runs = ov_on && merge_from < nl;
            const size_t tail_fork = runs ? nl : (nl >= (size_t)std::max(0, knobs().winv_tail) ? nl - (size_t)std::max(0, knobs().winv_tail) : 0);
            const MergeGroup* gq = runs ? group_of(q) : nullptr;
            const bool run_forks = knobs().winv_run_forks;
            const bool run_first = gq && gq->first == q && (run_forks || q == merge_from);
            // (a fork point inside a merged run moves to the run's first launch: an event recorded behind the run's kernel
            //  would wait for the whole run)
            auto fork_at = [&](size_t want) {
                if (want >= nl) return want;
                const MergeGroup* g = ov_on ? group_of(want) : nullptr;
                return g ? g->first : want;
            };
            const bool fork_here = first_top < nl && (q == fork_at(first_top >= (size_t)std::max(0, knobs().winv_early) ? first_top - (size_t)std::max(0, knobs().winv_early) : nl) ||
                                                      q == fork_at(first_top) || (q > first_top && (run_first || q == tail_fork)));
            if (fork_here && sch.launches[q].tinv_begin > w_done) {
                ensure_capture_streams();
                HIP_CHECK(hipEventRecord(ev_fork, st));
                HIP_CHECK(hipStreamWaitEvent(cap_side, ev_fork, 0));
                // a bounded grid: the top panels need whole CUs (their LDS), which a full-width launch would hold
                form_w(d_tinv_list.p + w_done, sch.launches[q].tinv_begin - w_done, sch.tinv_ncmax, cap_side, sch.side_winv_blocks);
                eager_fork = true;
                w_done = sch.launches[q].tinv_begin;
                // the fronts below the narrow top are used by the next sweep's first launches: the factorisation ends
                // with a wait for this event (normally long past by then)
                if (q <= first_top) HIP_CHECK(hipEventRecord(ev_side, cap_side));
            }
            if (ov_on && q >= sch.ov_first) {
                // Panels on the main stream, the level's Schur tiles on the overlap stream,
                // submitted in this order -- panel L, tiles L, panel L+1, ... -- which is correct even if the two streams
                // share a hardware queue.  Tiles of level L become ready only when the tiles of level L-1 have finished,
                // i.e. after panel L-1 ended and panel L got ready: the panels reach the CUs first.  (A tile workgroup
                // that waits for its panel holds LDS a panel workgroup needs; the first overlapped level therefore
                // starts its tiles only after its panels have finished.)
                a.ov = 1;
                a.nbk = L.nbk;
                // The panels of a run of narrow launches go out as ONE kernel (ov_groups: a few dozen workgroups): every one of
                // them is resident from the start, zeroes its panel, scatters K and fetches its item lists while its
                // children are still being factorised, and then waits for its children's tiles -- a level of the narrow
                // top costs its critical path (children's assembly, block loop, tiles) without a kernel boundary and
                // launch ramp in between.  Workgroups are dispatched in schedule order, i.e. lower levels first.
                const MergeGroup* g = group_of(q);
                const bool merged = g != nullptr;
                a.ov_slot = merged ? (int)g->first : (int)q;
                if (!merged) {
                    launch_panel(a, L.begin, L.count - L.nsliced, L.bs_panel, L.lds_panel, st);
                    launch_panel_sliced(a, L.slice_begin, L.slice_count, L.lds_sliced, st);
                } else if (q == g->first) {
                    if (g->sliced) launch_panel_sliced(a, L.slice_begin, g->count, g->lds, st);
                    else launch_panel(a, L.begin, g->count, 1024, g->lds, st);
                }
                if (q == sch.ov_first) {
                    HIP_CHECK(hipEventRecord(ev_ov_fork, st));
                    HIP_CHECK(hipStreamWaitEvent(ov_stream, ev_ov_fork, 0));
                } else if (L.ntiles > 0 && !no_gate) {
                    // the gate: this launch's tiles are released once all its panel workgroups are resident (k_ov_gate)
                    if (merged) launch_ov_gate(d_ov_started.p + g->first, g->count, flags.p + 2, ov_limit, ov_stream);
                    else launch_ov_gate(d_ov_started.p + q, L.count - L.nsliced + L.slice_count, flags.p + 2, ov_limit, ov_stream);
                }
                launch_schur(a, (const int2*)d_tiles.p, L.tile_begin, L.ntiles, ov_stream, L.ntiles);
                a.ov = 0;
                // (the tile stream's join event: behind the loop -- the last W formation may ride on that stream)
                continue;
            }
            if (L.small) {
                launch_front_wave(a, L.begin, L.count - L.ntiny, L.slice, st);
                launch_front_tiny(a, L.begin + L.count - L.ntiny, L.ntiny, st);
            } else {
                a.nbk = L.nbk;
                launch_panel(a, L.begin, L.count - L.nsliced, L.bs_panel, L.lds_panel, st);
                launch_panel_sliced(a, L.slice_begin, L.slice_count, L.lds_sliced, st);
                if (L.tinv_count > 0 && side) {
                    HIP_CHECK(hipEventRecord(ev_fork, st));
                    HIP_CHECK(hipStreamWaitEvent(side, ev_fork, 0));
                    form_w(d_tinv_list.p + L.tinv_begin, L.tinv_count, L.tinv_ncmax, side, 0);
                    forked = true;
                }
                launch_schur(a, (const int2*)d_tiles.p, L.tile_begin, L.ntiles, st, 0, L.tile_nc);
            }
        }
        if (forked) {
            HIP_CHECK(hipEventRecord(ev_join, side));
            HIP_CHECK(hipStreamWaitEvent(st, ev_join, 0));
        } else if (eager_fork) {
            // the solve matrices of the top fronts are formed on a side stream as well, behind the tree: the next
            // sweep only needs them when it reaches the top of the tree (enqueue_solve waits for ev_join there), so
            // their formation hides behind the sweep's bottom levels instead of ending the factorisation.
            // In the overlap mode it rides on the TILE stream, which has nothing left to do by now (a root has no tiles):
            // on the W stream it queued behind the previous fork's formation -- 170 us on a bounded grid, started when the
            // last run of panels started -- and the first sweep's persistent kernel waited ~50 us for it every step.
            const int done = w_done;
            hipStream_t last_on = ov_on ? ov_stream : cap_side;
            HIP_CHECK(hipStreamWaitEvent(st, ev_side, 0));
            HIP_CHECK(hipEventRecord(ev_fork, st));
            HIP_CHECK(hipStreamWaitEvent(last_on, ev_fork, 0));
            form_w(d_tinv_list.p + done, (int)sch.tinv_list.size() - done, sch.tinv_ncmax, last_on, 0);
            HIP_CHECK(hipEventRecord(ev_join, cap_side));
            if (ov_on) { HIP_CHECK(hipEventRecord(ev_join2, ov_stream)); w2_pending = true; }
            w_pending = true;
        } else {
            // one launch over every supernode, after the tree (all of them independent)
            form_w(d_tinv_list.p, (int)sch.tinv_list.size(), sch.tinv_ncmax, st, 0);
        }
        if (ov_on) {
            // The tile stream is joined by the NEXT factorisation, not by this one's tail: every tile has been counted
            // by its parent's panel (a root has no tiles), so when the main stream's last panel kernel ends all
            // tile data has long been stored; what is left on the tile stream are workgroups on their way out (and the
            // last W formation, which the sweeps wait for by ev_join2).  A cross-stream wait here cost ~17 us between the
            // last panel and the status kernel, every step.
            HIP_CHECK(hipEventRecord(ev_ov_join, ov_stream));
            ov_join_pending = true;
        }
        if (tok) {
            ov_release.on = false;
            dev_enqueued(true);                  // (records the event that, with ev_ov_join / ev_join, says this factorisation has left its streams)
        }
        HIP_CHECK(hipGetLastError());
        if (want_stamps) {
            std::vector<long long> h(sch.launches.size() * 16);
            HIP_CHECK(hipMemcpyAsync(h.data(), stamps.p, h.size() * 8, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            static int printed = 0;
            if (printed++ == 2) {
                for (size_t r = 0; r < sch.launches.size(); ++r) {
                    const long long* q = &h[r * 16];
                    if (sch.launches[r].small) continue;
                    std::fprintf(stderr, "[stamps2] launch %zu: wave 0's items %.1f us (first batch's loads %.1f us), then all waves %.1f us\n", r, (q[7] - q[6]) * 0.01, (q[15] - q[6]) * 0.01, (q[3] - q[7]) * 0.01);
                    std::fprintf(stderr, "[stamps] launch %zu fronts %d f=%lld nc=%lld kids=%lld | zero %.1f K %.1f kids %.1f factor %.1f "
                                 "(diag %.1f trsm %.1f trail %.1f) store %.1f us  clk %.0f MHz\n", r, sch.launches[r].count, q[11], q[12], q[13],
                                 (q[1] - q[0]) * 0.01, (q[2] - q[1]) * 0.01, (q[3] - q[2]) * 0.01, (q[4] - q[3]) * 0.01,
                                 q[8] * 0.01, q[9] * 0.01, q[10] * 0.01, (q[5] - q[4]) * 0.01,
                                 (double)q[14] / ((q[5] - q[0]) * 0.01));
                }
            }
        }
    }

    void reserve_nr(int nr)
    {
        if ((size_t)nr <= nr_cap) return;
        wait_w(stream);
        HIP_CHECK(hipStreamSynchronize(stream));
        // (solve graphs captured so far have the old xp / uvec baked in)
        for (auto& kv : solve_graphs) (void)hipGraphExecDestroy(kv.second);
        solve_graphs.clear();
        xp.alloc((size_t)S.N * nr);
        uvec.alloc(std::max<size_t>(S.rows.size(), 1) * nr);
        nr_cap = (size_t)nr;
    }
    // use_top: the persistent kernel may be used (claimed); allow_chain: the caller reads the abort word afterwards and
    // repeats the solve if a bounded wait expired (the same promise use_top implies), so the chained launches may be used.
    // How the sweep is split is decided by plan_sweep (schedule.cpp); this function launches the plan.
    void enqueue_solve(const double* d_b, double* d_x, hipStream_t st, bool use_top, int nr, int64_t ldb, int64_t ldx, bool allow_chain = false)
    {
        const SweepPlan plan = plan_sweep(sch, SweepState{use_top, allow_chain, top_disabled, chain_disabled, w_pending}, nr, dev, top_grid_nr);
        if (plan.split_columns) {
            for (int c = 0; c < nr; ++c) enqueue_solve(d_b + (int64_t)c * ldb, d_x + (int64_t)c * ldx, st, use_top, 1, 0, 0, allow_chain);
            return;
        }
        SolveArgs a;
        a.T = tree();
        a.fronts = fronts.p;
        a.tinv = tinv.p;
        a.Dinv = Dinv.p;
        a.b = d_b;
        a.out = d_x;
        a.xp = xp.p;
        a.uvec = uvec.p;
        a.top_limit = knobs().top_test_limit;
        // diagnostic (HIPKKT_TOP_STAMPS=n): the n-th single-column sweep over the full persistent set records eight time
        // stamps per front and direction, printed per level afterwards (this call then synchronises)
        const int stamp_call = knobs().top_stamps;
        a.top_stamps = nullptr;
        a.ld_b = ldb; a.ld_out = ldx; a.ld_xp = S.N; a.ld_uvec = (int64_t)std::max<size_t>(S.rows.size(), 1);
        a.tk_pos = d_tk_pos.p; a.tk_sl = d_tk_sl.p; a.tbase = d_tbase.p; a.xf = xf.p; a.add = nullptr;
        a.chain_cnt = nullptr;       // (set below when this sweep chains its lower levels)
        a.recs = d_recs.p ? reinterpret_cast<const char*>(d_recs.p) : nullptr;
        a.tall_ws = tall_ws.p;
        const std::vector<Launch>& launches = sch.launches;
        const size_t nl = launches.size(), nper = plan.nper, ntl = plan.ntl, first_w = plan.first_w;
        const bool chain_on = plan.chain_on;
        const int ncount = plan.ncount;
        // diagnostic (HIPKKT_VERBOSE): the plan, once per distinct plan of this engine (describe: schedule.cpp)
        if (knobs().verbose >= 1) {
            const std::string text = describe(plan, sch, nr, w_pending, a.recs != nullptr);
            if (std::find(sweep_plans_seen.begin(), sweep_plans_seen.end(), text) == sweep_plans_seen.end()) {
                sweep_plans_seen.push_back(text);
                std::fprintf(stderr, "[hipkkt] sweep plan: %s\n", text.c_str());
                if (knobs().verbose >= 2) std::fputs(describe_launches(plan, sch).c_str(), stderr);
            }
        }
        bool chain_stamp = false;
        ChainArgs ca;
        int ca_wgs = 0;
        size_t ca_lds = 0;
        auto chain_reset = [&]() {
            ca.nseg = 0; ca.lo = 1 << 30; ca.hi = 0; ca.cnt = d_chain.p; ca.done = d_chain.p + S.nsuper; ca.nchild = d_chain_nchild.p;
            ca.abort_word = top_flags.p + 2 * sch.top_nflag; ca.epoch = chain_epoch;
            ca.lo0 = chain_on ? launches[nper].begin : 0;
            ca.nstamp = chain_on ? launches[nl - ntl - 1].begin + launches[nl - ntl - 1].count - ca.lo0 : 0;
            ca_wgs = 0; ca_lds = 0;
        };
        auto chain_flush = [&](bool fwd) {
            if (ca.nseg > 0) {
                a.top_stamps = chain_stamp ? (long long*)top_stamps.p : nullptr;
                if (fwd) launch_fwd_chain(a, ca, ca_wgs, ca_lds, st, nr);
                else launch_bwd_chain(a, ca, ca_wgs, ca_lds, st, nr);
                a.top_stamps = nullptr;
            }
            chain_reset();
        };
        auto chain_add = [&](const Launch& L, bool fwd) {
            const bool blocks = !L.small;
            if (ca.nseg == kChainMaxSeg) chain_flush(fwd);
            ChainSeg& sg = ca.seg[ca.nseg++];
            sg.begin = L.begin;
            sg.nblock = blocks ? L.count : 0;
            sg.nwave = blocks ? 0 : L.count - L.ntiny;
            sg.ntiny = blocks ? 0 : L.ntiny;
            sg.wg0 = ca_wgs;
            sg.leaf = (L.small && L.level == 0) ? 1 : 0;
            sg.rec = L.rec;
            ca_wgs += chain_seg_wgs(sg);
            ca.lo = std::min(ca.lo, L.begin);
            ca.hi = std::max(ca.hi, L.begin + L.count);
            if (blocks) ca_lds = std::max(ca_lds, L.lds_solve);
        };
        if (chain_on) {
            ++chain_epoch;
            a.chain_cnt = d_chain.p;
            // diagnostic (HIPKKT_TOP_STAMPS=n): the n-th single-column chained sweep records six time stamps per
            // block-class front and direction, printed per launch afterwards
            if (stamp_call > 0 && nr == 1 && !w_pending && ++n_stamp_sweeps == stamp_call) {
                start_stamps((size_t)(launches[nl - ntl - 1].begin + launches[nl - ntl - 1].count - launches[nper].begin), st);
                chain_stamp = true;
            }
        }
        for (size_t q = 0; q < nper; ++q) {
            const Launch& L = launches[q];
            if (q == first_w) wait_w(st);
            if (pair_at(sch, q, plan)) {
                const Launch& Ls = launches[q + 1];
                if (q + 1 == first_w) wait_w(st);
                launch_fwd_level(a, pair_rec(L, Ls), L.begin, L.count, Ls.count - Ls.ntiny, Ls.ntiny, L.solve_bs, L.lds_solve, st, nr);
                ++q;
            } else if (L.small) {
                launch_fwd_small(a, L.rec, L.begin, L.count - L.ntiny, L.ntiny, st, L.level == 0, nr);
            } else {
                launch_fwd(a, L.rec, L.begin, L.count - L.ntall, L.solve_bs, L.lds_solve, st, nr);
                launch_fwd_tall(a, L.begin + L.count - L.ntall, L.ntall, L.fmax, st);       // (fronts beyond the block kernels' LDS)
            }
        }
        if (chain_on) {
            chain_reset();
            for (size_t q = nper; q + ntl < nl; ++q) {
                if (q == first_w) { chain_flush(true); wait_w(st); }
                chain_add(launches[q], true);
            }
            chain_flush(true);
        }
        wait_w(st);
        if (plan.kernel == TopKernel::sliced) {
            // the set holds very tall fronts: the (front, slice) kernel; positions count from the full set's first front
            const Launch& Lfull = launches[nl - sch.top_launches];
            const int pos0 = sch.top_count - ncount;
            const int task0 = sch.h_tbase[(size_t)pos0];
            const bool sl_stamp = stamp_call > 0 && !chain_on && nr == 1 && ntl == sch.top_launches && ++n_stamp_sweeps == stamp_call;
            if (sl_stamp) {
                start_stamps((size_t)(sch.top_ntask - task0), st);
                a.top_stamps = (long long*)top_stamps.p;
            }
            launch_top_solve_sliced(a, Lfull.begin, pos0, task0, sch.top_ntask, plan.pgrid, sch.top_slds, top_flags.p,
                                    sch.top_nflag, ++top_epoch, st, nr);
            a.top_stamps = nullptr;
            if (sl_stamp) print_sliced_stamps((size_t)(sch.top_ntask - task0), st);
        } else if (plan.kernel == TopKernel::top) {
            const bool stamp_now = stamp_call > 0 && !chain_on && nr == knobs().top_stamps_nr && ntl == sch.top_launches && ++n_stamp_sweeps == stamp_call;
            if (stamp_now) {
                start_stamps((size_t)ncount, st);
                a.top_stamps = (long long*)top_stamps.p;
            }
            launch_top_solve(a, launches[nl - ntl].begin, ncount, plan.pgrid, sch.top_lds, top_flags.p, sch.top_count, ++top_epoch, st, sch.top_tall, nr);
            a.top_stamps = nullptr;
            if (stamp_now) print_top_stamps(plan, st);
        }
        if (chain_on) {
            chain_reset();
            for (size_t q = nl - ntl; q-- > nper;) chain_add(launches[q], false);
            chain_flush(false);
            if (chain_stamp) print_chain_stamps(plan, st);
        }
        for (size_t q = nper; q-- > 0;) {
            const Launch& L = launches[q];
            if (q > 0 && pair_at(sch, q - 1, plan)) {
                const Launch& Lb = launches[q - 1];
                launch_bwd_level(a, pair_rec(Lb, L), Lb.begin, Lb.count, L.count - L.ntiny, L.ntiny, Lb.solve_bs, Lb.lds_solve, st, nr);
                --q;
            } else if (L.small) {
                launch_bwd_small(a, L.rec, L.begin, L.count - L.ntiny, L.ntiny, st, nr);
            } else {
                launch_bwd(a, L.rec, L.begin, L.count - L.ntall, L.solve_bs, L.lds_solve, st, nr);
                launch_bwd_tall(a, L.begin + L.count - L.ntall, L.ntall, L.fmax, S.N, st);
            }
        }
        HIP_CHECK(hipGetLastError());
    }

    // ---- diagnostic time stamps (HIPKKT_TOP_STAMPS): eight stamps per record and direction in top_stamps, n records per
    // direction; read back behind the sweep (synchronises) and printed by the kernel that wrote them
    void start_stamps(size_t n, hipStream_t st)
    {
        top_stamps.alloc(2 * n * 8);
        top_stamps.zero(st);
    }
    std::vector<long long> read_stamps(size_t n, hipStream_t st)
    {
        std::vector<long long> h(2 * n * 8);
        HIP_CHECK(hipMemcpyAsync(h.data(), top_stamps.p, h.size() * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return h;
    }
    // one front's five phases (preload, wait, gather, products, reduce + store) in us, added to d
    static void add_phases(const long long* e, double d[5])
    {
        for (int k = 0; k < 5; ++k) d[k] += (e[k + 1] - e[k]) * 0.01;
    }
    // (front, slice) tasks: per direction the mean time from a task's start to its flags seen, from there
    // to its publication, and the sweep's span
    void print_sliced_stamps(size_t nt, hipStream_t st)
    {
        const std::vector<long long> h = read_stamps(nt, st);
        for (int dir = 0; dir < 2; ++dir) {
            double wait = 0, work = 0;
            long long lo = h[(size_t)dir * nt * 8], hi = 0;
            std::vector<double> works;
            for (size_t t = 0; t < nt; ++t) {
                const long long* e = &h[((size_t)dir * nt + t) * 8];
                wait += (e[2] - e[0]) * 0.01;
                work += (e[5] - e[2]) * 0.01;
                works.push_back((e[5] - e[2]) * 0.01);
                lo = std::min(lo, e[0]); hi = std::max(hi, e[5]);
            }
            std::sort(works.begin(), works.end());
            std::fprintf(stderr, "[top stamps] sliced %s: %zu tasks, span %.1f us; per task: start->flags seen %.2f us (mean), flags seen->publish "
                         "%.2f us (mean), %.2f (median), %.2f (max)\n", dir == 0 ? "fwd" : "bwd", nt, (hi - lo) * 0.01, wait / nt, work / nt,
                         works[nt / 2], works.back());
        }
    }
    // the persistent kernel, per level of its part of the set
    void print_top_stamps(const SweepPlan& plan, hipStream_t st)
    {
        const std::vector<Launch>& launches = sch.launches;
        const size_t nl = launches.size(), ntl = plan.ntl;
        const int ncount = plan.ncount;
        const std::vector<long long> h = read_stamps((size_t)ncount, st);
        long long t0 = h[0];
        for (int p = 0; p < ncount; ++p) t0 = std::min(t0, h[(size_t)p * 8]);
        const int pbase = launches[nl - ntl].begin;
        for (int dir = 0; dir < 2; ++dir) {
            double prev_done = 0.0;
            for (size_t qq = 0; qq < ntl; ++qq) {
                const size_t q = dir == 0 ? nl - ntl + qq : nl - 1 - qq;
                const Launch& L = launches[q];
                double d[5] = {0, 0, 0, 0, 0}, first_start = 1e30, last_seen = 0, last_done = 0, crit[5] = {0, 0, 0, 0, 0};
                for (int t = L.begin; t < L.begin + L.count; ++t) {
                    const long long* e = &h[((size_t)dir * ncount + (size_t)(t - pbase)) * 8];
                    add_phases(e, d);
                    first_start = std::min(first_start, (e[0] - t0) * 0.01);
                    last_seen = std::max(last_seen, (e[2] - t0) * 0.01);
                    if ((e[5] - t0) * 0.01 > last_done) {
                        last_done = (e[5] - t0) * 0.01;
                        for (int k = 0; k < 5; ++k) crit[k] = (e[k + 1] - e[k]) * 0.01;
                    }
                }
                std::fprintf(stderr, "[top stamps] %s level %2d: %4d fronts, first starts %7.2f, last sees its flags %7.2f, last publishes %7.2f "
                             "(hop %5.2f) us | mean: preload %5.2f wait %6.2f gather %5.2f products %5.2f reduce+store %5.2f | "
                             "last front: %5.2f %6.2f %5.2f %5.2f %5.2f\n", dir == 0 ? "fwd" : "bwd", L.level, L.count, first_start, last_seen,
                             last_done, last_done - prev_done, d[0] / L.count, d[1] / L.count, d[2] / L.count, d[3] / L.count,
                             d[4] / L.count, crit[0], crit[1], crit[2], crit[3], crit[4]);
                prev_done = last_done;
            }
        }
    }
    // the chained kernels, per block-class launch of the chained range
    void print_chain_stamps(const SweepPlan& plan, hipStream_t st)
    {
        const std::vector<Launch>& launches = sch.launches;
        const size_t nl = launches.size(), nper = plan.nper, ntl = plan.ntl;
        const int lo0 = launches[nper].begin;
        const size_t nst = (size_t)(launches[nl - ntl - 1].begin + launches[nl - ntl - 1].count - lo0);
        const std::vector<long long> h = read_stamps(nst, st);
        for (int dir = 0; dir < 2; ++dir) {
            long long t00 = 0;
            for (size_t k = 0; k < nst; ++k) { const long long v = h[((size_t)dir * nst + k) * 8]; if (v && (!t00 || v < t00)) t00 = v; }
            for (size_t qq = nper; qq + ntl < nl; ++qq) {
                const size_t q = dir == 0 ? qq : nl - ntl - 1 - (qq - nper);
                const Launch& L = launches[q];
                if (L.small) continue;
                double d[5] = {0, 0, 0, 0, 0}, first_start = 1e30, last_start = 0, last_seen = 0, first_done = 1e30, last_done = 0;
                for (int t = L.begin; t < L.begin + L.count; ++t) {
                    const long long* e = &h[((size_t)dir * nst + (size_t)(t - lo0)) * 8];
                    add_phases(e, d);
                    first_start = std::min(first_start, (e[0] - t00) * 0.01);
                    last_start = std::max(last_start, (e[0] - t00) * 0.01);
                    last_seen = std::max(last_seen, (e[2] - t00) * 0.01);
                    first_done = std::min(first_done, (e[5] - t00) * 0.01);
                    last_done = std::max(last_done, (e[5] - t00) * 0.01);
                }
                std::fprintf(stderr, "[chain stamps] %s launch %2zu level %2d: %4d fronts, starts %6.2f .. %6.2f, last sees its flag %6.2f, done %6.2f .. %6.2f us | "
                             "mean: preload %5.2f wait %6.2f gather %5.2f products %5.2f reduce+store %5.2f\n", dir == 0 ? "fwd" : "bwd", q, L.level, L.count,
                             first_start, last_start, last_seen, first_done, last_done, d[0] / L.count, d[1] / L.count, d[2] / L.count, d[3] / L.count, d[4] / L.count);
            }
        }
    }

    std::vector<std::string> sweep_plans_seen;      // (HIPKKT_VERBOSE: the plans enqueue_solve has printed)
    // the side stream may still be forming the top fronts' solve matrices (enqueue_factor)
    bool w_pending = false, w2_pending = false;    // (w2: the last formation rode on the tile stream: ev_join2)
    void wait_w(hipStream_t st)
    {
        if (!w_pending) return;
        HIP_CHECK(hipStreamWaitEvent(st, ev_join, 0));
        if (w2_pending) HIP_CHECK(hipStreamWaitEvent(st, ev_join2, 0));
        w_pending = false;
        w2_pending = false;
    }

    // ---- chained launches (chain_kernels.hip)
    DBuf<int> d_chain;           // [0, nsuper): forward counters (zero between sweeps); [nsuper, 2 nsuper): backward epoch words
    int chain_epoch = 0;
    bool chain_disabled = false;
    DBuf<int> d_chain_nchild;    // per supernode: its children in chained launches (the ones that count themselves in)
    DBuf<int64_t> d_recs;        // packed sweep records (kernels.hpp: SolveHdr); empty: the legacy layout
    DBuf<double> tall_ws;        // work space of the tall-front sweep kernels (allocated when the schedule holds such fronts)

    // ---- admission of this handle's multi-stream / waiting operations on its device (DevOp)
    struct TokenRelease {
        LDLEngine* e; bool on;
        ~TokenRelease() { if (on) e->dev_enqueued(false); }
    };
public:
    void set_device(int d)       // (once, right after construction: the engine joins its device's bookkeeping)
    {
        device_id = d;
        if (born) return;
        born = true;
        std::lock_guard<std::mutex> lk(g_dev_mu);
        DevState& D = g_dev[device_id];
        DevRec r;
        r.eng = this;
        D.recs.push_back(r);
        if (D.recs.size() == 2) (void)hipDeviceSynchronize();     // from now on operations carry events (see DevOp)
    }
private:
    bool born = false;
    void engine_gone()
    {
        if (!born) return;
        std::lock_guard<std::mutex> lk(g_dev_mu);
        auto it = g_dev.find(device_id);
        if (it == g_dev.end()) return;
        auto& v = it->second.recs;
        for (size_t k = 0; k < v.size(); ++k) if (v[k].eng == this) { v.erase(v.begin() + (long)k); break; }
    }
    static bool rec_idle(DevRec& r)
    {
        if (r.kind == kOpNone) return true;
        if (r.enqueuing) return false;
        const bool done = (!r.done_main || hipEventQuery(r.done_main) == hipSuccess) &&
                          (!r.done_tiles || hipEventQuery(r.done_tiles) == hipSuccess) &&
                          (!r.done_side || hipEventQuery(r.done_side) == hipSuccess);
        (void)hipGetLastError();
        if (done) r.kind = kOpNone;
        return done;
    }
    bool claim_dev(int kind)
    {
        if (!born) return true;
        std::lock_guard<std::mutex> lk(g_dev_mu);
        DevState& D = g_dev[device_id];
        DevRec* me = nullptr;
        int busy = kOpNone;
        bool others_quiet = true;                // no other handle has called in during the last 20 ms
        const auto now = std::chrono::steady_clock::now();
        for (DevRec& r : D.recs) {
            if (r.eng == this) { me = &r; continue; }
            if (D.recs.size() > 1 && r.stream != stream) {
                if (!rec_idle(r)) busy = std::max(busy, r.kind);
                if (now - r.last_seen < std::chrono::milliseconds(20)) others_quiet = false;
            }
        }
        if (!me) return true;
        me->last_seen = now;
        const bool ok = kind == kOpX ? (busy == kOpNone && others_quiet) : (kind == kOpS ? busy < kOpS : busy < kOpX);
        if (!ok) { ++(kind == kOpS ? n_top_busy : n_ov_busy); return false; }
        if (D.recs.size() > 1) {
            if (!ev_dev_done) HIP_CHECK(hipEventCreateWithFlags(&ev_dev_done, hipEventDisableTiming));
            const bool mine_idle = rec_idle(*me);
            me->kind = std::max(mine_idle ? (int)kOpNone : me->kind, kind);
            me->done_main = ev_dev_done; me->done_tiles = ev_ov_join; me->done_side = ev_join;
        }
        me->stream = stream;
        me->enqueuing = true;
        claimed_kind = kind;
        return true;
    }
    int claimed_kind = kOpNone;
    // the operation is enqueued (recorded = true: mark its end on the main stream) or the call was abandoned
    void dev_enqueued(bool recorded)
    {
        if (!born) return;
        std::lock_guard<std::mutex> lk(g_dev_mu);
        DevState& D = g_dev[device_id];
        for (DevRec& r : D.recs) {
            if (r.eng != this) continue;
            if (recorded && D.recs.size() > 1) {
                if (!ev_dev_done && hipEventCreateWithFlags(&ev_dev_done, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); r.enqueuing = false; continue; }
                (void)hipEventRecord(ev_dev_done, stream);
                r.kind = std::max(r.kind, claimed_kind);       // (a second handle may have appeared since the admission)
                r.done_main = ev_dev_done; r.done_tiles = ev_ov_join; r.done_side = ev_join;     // (the streams' events may have been created meanwhile)
            }
            r.enqueuing = false;
        }
    }

    // ---- persistent-kernel bookkeeping
    bool top_disabled = false;

public:
    // device word set by the persistent kernel when one of its bounded waits expired (nullptr: no such kernel)
    const int* top_abort_word() const { return (top_flags.p && (sch.top_launches > 0 || sch.chain_from < sch.launches.size())) ? top_flags.p + 2 * sch.top_nflag : nullptr; }
    // The caller has synchronised and found the abort word set: clear it and never use the kernel again.
    int64_t n_ov_fallbacks = 0, n_top_fallbacks = 0;      // lifetime counts (hipkkt_profile, hipkkt_ldl_fallbacks)
    int64_t n_ov_busy = 0;       // factorisations that were not admitted as class X / M (DevOp) and ran on fewer streams
    int64_t n_top_busy = 0;      // sweeps that were not admitted as class S and went level by level
    void top_gave_up()
    {
        top_disabled = true;
        chain_disabled = true;       // (the chained launches share the abort word: whichever wait expired, both go)
        ++n_top_fallbacks;
        launch_zero_ints(top_flags.p + 2 * sch.top_nflag, 1, stream);
        if (d_chain.p) launch_zero_ints(d_chain.p, 2 * S.nsuper, stream);       // (an abandoned sweep leaves counters behind)
        std::fprintf(stderr, "[hipkkt] persistent top-of-tree kernel gave up waiting (GPU shared with another "
                             "resident kernel?); falling back to one launch per level\n");
    }
    // synchronises; for callers without a read-back of their own
    bool top_aborted_sync()
    {
        const int* w = top_abort_word();
        if (!w) return false;
        int v = 0;
        HIP_CHECK(hipMemcpyAsync(&v, w, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return v != 0;
    }

    // synchronises: {#dynamic regularisations, non-finite flag, an overlap-mode wait gave up}
    void read_flags(int out[3])
    {
        HIP_CHECK(hipMemcpyAsync(out, flags.p, 3 * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    // The caller found flags[2] set: a bounded wait of the overlap mode expired (never expected; another process on
    // the GPU, or two streams that could not run side by side).  From now on the factorisation runs level by level;
    // the caller repeats it.
    void ov_gave_up()
    {
        ov_disabled = true;
        ++n_ov_fallbacks;
        if (knobs().verbose) {            // which wait expired first (factor_kernels.hip, ov_wait_ge)
            // (the diagnostic words are plain stores behind the abort's CAS: let the tile stream drain first)
            if (ov_stream) (void)hipStreamSynchronize(ov_stream);
            int w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            (void)hipMemcpy(w, flags.p, sizeof(w), hipMemcpyDeviceToHost);
            const int sn = w[4];
            std::fprintf(stderr, "[hipkkt] expired wait: kind %d (1 panel for a child's tiles, 2 tile for its panel, 3 gate), waited for %d "
                         "(saw %d of %d)", w[3], sn, w[5], w[6]);
            if ((w[3] == 1 || w[3] == 2) && sn >= 0 && sn < S.nsuper) {
                int q = -1;
                for (size_t k = 0; k < sch.sched.size(); ++k) if (sch.sched[k] == sn) q = (int)k;
                size_t lq = 0;
                while (lq < sch.launches.size() && !(q >= sch.launches[lq].begin && q < sch.launches[lq].begin + sch.launches[lq].count)) ++lq;
                std::fprintf(stderr, "; supernode %d is in launch %zu of %zu (overlap from %zu, %zu merged runs, the first from %zu), level %d, parent %d", sn, lq,
                             sch.launches.size(), sch.ov_first, sch.ov_groups.size(), sch.ov_groups.empty() ? sch.launches.size() : sch.ov_groups.front().first, lq < sch.launches.size() ? sch.launches[lq].level : -1, S.sn_parent[sn]);
            }
            std::fprintf(stderr, "\n");
            // the lowest overlapped launch with unfinished fronts: progress of its panels and tiles as the abort left them
            std::vector<int> prog((size_t)S.nsuper), done((size_t)S.nsuper), nt((size_t)S.nsuper), started(sch.launches.size());
            (void)hipMemcpy(prog.data(), d_ov_prog.p, prog.size() * sizeof(int), hipMemcpyDeviceToHost);
            (void)hipMemcpy(done.data(), d_ov_done.p, done.size() * sizeof(int), hipMemcpyDeviceToHost);
            (void)hipMemcpy(nt.data(), d_ov_ntiles.p, nt.size() * sizeof(int), hipMemcpyDeviceToHost);
            (void)hipMemcpy(started.data(), d_ov_started.p, started.size() * sizeof(int), hipMemcpyDeviceToHost);
            int shown = 0;
            for (size_t q = sch.ov_first; q < sch.launches.size() && shown < 12; ++q) {
                const Launch& L = sch.launches[q];
                int unfinished = 0;
                for (int t = L.begin; t < L.begin + L.count; ++t) {
                    const int s2 = sch.sched[(size_t)t];
                    const int ncs = S.sn_start[s2 + 1] - S.sn_start[s2];
                    if (prog[(size_t)s2] < ncs || done[(size_t)s2] < nt[(size_t)s2]) {
                        if (shown < 12) {
                            std::fprintf(stderr, "[hipkkt]   launch %zu (started %d) position %d supernode %d: %d of %d columns published, %d of %d tiles done, "
                                         "%d children:", q, started[q], t - L.begin, s2, prog[(size_t)s2], ncs, done[(size_t)s2], nt[(size_t)s2],
                                         S.child_ptr[s2 + 1] - S.child_ptr[s2]);
                            for (int e = S.child_ptr[s2]; e < S.child_ptr[s2 + 1]; ++e) {
                                const int c = S.child_idx[e];
                                if (nt[(size_t)c] > 0) std::fprintf(stderr, " %d(%d/%d)", c, done[(size_t)c], nt[(size_t)c]);
                            }
                            if (sch.ov_group_of[q] >= 0) {
                                const MergeGroup& g = sch.ov_groups[(size_t)sch.ov_group_of[q]];
                                std::fprintf(stderr, " | merged kernel of launches %zu..%zu: %d of %d workgroups started", g.first, g.end - 1, started[g.first], g.count);
                            }
                            std::fprintf(stderr, "\n");
                            ++shown;
                        }
                        ++unfinished;
                    }
                }
                if (unfinished) std::fprintf(stderr, "[hipkkt]   launch %zu: %d of %d fronts unfinished, %d tiles\n", q, unfinished, L.count, L.ntiles);
            }
        }
        std::fprintf(stderr, "[hipkkt] factorisation overlap gave up waiting; falling back to one level after the other\n");
    }
    static bool overlap_wanted()
    {
        return knobs().factor_overlap;
    }
    bool ov_active() const { return overlap_wanted() && !ov_disabled && sch.ov_first < sch.launches.size(); }

    int* flags_ptr() { return flags.p; }
    const double* dinv_ptr() const { return Dinv.p; }
    // hipkkt_kkt_system_set_member_status: N regularisers in the factor's column order that replace *d_eps (FactorArgs::eps_col)
    const double* eps_col = nullptr;

private:
    DBuf<int> d_sn_start, d_rows, d_rel, d_ncolpar, d_child_ptr, d_child_idx, d_ksrc, d_kdst, d_sched, d_perm;
    DBuf<int64_t> d_rowptr, d_front_off, d_upd_off, d_kptr;
    DBuf<signed char> d_psign;
    DBuf<double> fronts, upd, Dinv, xp, uvec, tinv;
    DBuf<double> xp_m, uvec_m;   // work vectors of solve_multi, row-major N x cap and sum(nb) x cap
    DBuf<int> d_iperm;
    size_t multi_cap = 0;
    DBuf<int64_t> d_tinv_off;
    DBuf<double> top_stamps;
    int n_stamp_sweeps = 0;
#ifdef HIPKKT_EXPERIMENTS
    int n_skipw_calls = 0;
#endif
    DBuf<int> d_tinv_list;
    DBuf<int> flags;
    DBuf<int64_t> stamps;
    DBuf<int64_t> d_tiles;       // int2 {supernode, ti<<16|tj}
    DBuf<int64_t> d_cut_ptr;     // per supernode (as a child): offset into d_cuts
    DBuf<int> d_cuts;            // first child-row index reaching each 64-row tile boundary of the parent's U
    DBuf<int64_t> d_item_ptr;
    DBuf<ExtItem> d_items;
    DBuf<int64_t> d_dense_off;   // per supernode: offset of its dense child's update block (-1: none)
    DBuf<int64_t> d_wave_cut;
    DBuf<SubItem> d_sitems;
    DBuf<int64_t> d_tile_cut;
    DBuf<PullTerm> d_pterms;
    DBuf<int> d_pwave_cut, d_ptile_cut;
    int64_t n_factor_pulled = 0, n_factor_terms = 0;
    DBuf<FrontDesc> d_desc;
    DBuf<FrontDesc> d_sdesc;     // per row slice of the sliced panels
    DBuf<int> d_spos, d_sn_parent, top_flags;
    DBuf<int> d_tk_pos, d_tk_sl, d_tbase;      // tasks of k_top_solve_sliced (SolveArgs::tk_*); empty unless the set has tall fronts
    DBuf<double> xf;
    bool ov_disabled = false;
    bool ov_concurrent = false;          // the main and the tile stream run side by side (choose_side_streams)
    DBuf<int> d_ov_prog, d_ov_done, d_ov_ntiles, d_ov_sprog, d_ov_sbase, d_ov_started;
    hipStream_t ov_stream = nullptr;
    hipEvent_t ev_ov_fork = nullptr, ev_ov_join = nullptr, ev_dev_done = nullptr;
    bool ov_join_pending = false;    // ev_ov_join recorded, not yet waited for (enqueue_factor)
    size_t nr_cap = 1;           // right-hand sides xp / uvec are sized for
    int top_epoch = 0;
    DBuf<int> d_gl_src, d_udst;
    DBuf<int64_t> d_glm_ptr, d_hp_lidx, d_pr_ptr;     // many-column sweeps: gather lists without the pulled leaves, and the pulled terms
    DBuf<int> d_udst_m, d_hp_col, d_hp_row, d_pr_slot;
    int n_pull_rows = 0;
    // ---- what was decided (schedule.cpp) and what the device contributed to it
    Schedule sch;
    DeviceLimits dev;
    NrGrids top_grid_nr;         // the persistent kernel's grid for 2 / 4 right-hand sides (asked on first use)

    TreeDev tree() const
    {
        TreeDev t;
        t.nsuper = S.nsuper;
        t.sn_start = d_sn_start.p; t.rowptr = d_rowptr.p; t.rows = d_rows.p; t.rel = d_rel.p;
        t.ncolpar = d_ncolpar.p; t.front_off = d_front_off.p; t.upd_off = d_upd_off.p;
        t.child_ptr = d_child_ptr.p; t.child_idx = d_child_idx.p; t.kptr = d_kptr.p;
        t.ksrc = d_ksrc.p; t.kdst = d_kdst.p; t.sched = d_sched.p; t.psign = d_psign.p; t.perm = d_perm.p;
        t.dense_off = d_dense_off.p; t.item_ptr = d_item_ptr.p; t.items = d_items.p; t.gl_ptr = d_item_ptr.p; t.gl_src = d_gl_src.p; t.udst = d_udst.p;
        t.glm_ptr = d_glm_ptr.p; t.udst_m = d_udst_m.p; t.hp_col = d_hp_col.p; t.hp_row = d_hp_row.p; t.hp_lidx = d_hp_lidx.p; t.pr_ptr = d_pr_ptr.p; t.pr_slot = d_pr_slot.p;
        t.cut_ptr = d_cut_ptr.p; t.cuts = d_cuts.p; t.wave_cut = d_wave_cut.p; t.tinv_off = d_tinv_off.p;
        t.sitems = d_sitems.p; t.tile_cut = d_tile_cut.p;
        t.pterms = d_pterms.p; t.pwave_cut = d_pwave_cut.p; t.ptile_cut = d_ptile_cut.p; t.desc = d_desc.p; t.sdesc = d_sdesc.p;
        t.spos = d_spos.p; t.sn_parent = d_sn_parent.p;
        return t;
    }

    int front_size(int s) const { return hipkkt::front_size(S, s); }

    // The device tables are built on the host (engine_tables.cpp, schedule.cpp); here they are uploaded, group by
    // group, and the work buffers allocated and zeroed.
    void upload(const std::vector<int>& dsigns)
    {
        const int verbose = knobs().verbose;
        // the factorisation's extend-add work lists and which leaves their parents pull (schedule.cpp)
        FactorLists fl = build_factor_lists(S, sch);
        n_factor_pulled = fl.n_pulled; n_factor_terms = fl.n_terms;
        EngineTables T = build_engine_tables(S, sch, fl, dsigns);
        n_pull_rows = T.n_pull_rows;
        d_sn_start.upload(S.sn_start);
        d_rowptr.upload(S.rowptr);
        d_rows.upload(S.rows);
        d_rel.upload(S.rel);
        d_ncolpar.upload(T.ncolpar);
        d_front_off.upload(S.front_off);
        d_upd_off.upload(S.upd_off);
        d_child_ptr.upload(S.child_ptr);
        d_child_idx.upload(S.child_idx);
        d_kptr.upload(S.kptr);
        d_kdst.upload(T.kdst);
        d_ksrc.upload(T.ksrc);
        d_sched.upload(sch.sched);
        d_ov_started.alloc(std::max<size_t>(sch.launches.size(), 1));
        HIP_CHECK(hipMemset(d_ov_started.p, 0, std::max<size_t>(sch.launches.size(), 1) * sizeof(int)));
        d_ov_ntiles.upload(T.ov_ntiles);
        d_ov_sbase.upload(T.ov_sbase);
        d_ov_sprog.alloc(std::max<size_t>(sch.slice_list.size(), 1));
        HIP_CHECK(hipMemset(d_ov_sprog.p, 0, std::max<size_t>(sch.slice_list.size(), 1) * sizeof(int)));
        d_ov_prog.alloc((size_t)S.nsuper);
        d_ov_done.alloc((size_t)S.nsuper);
        HIP_CHECK(hipMemset(d_ov_prog.p, 0, (size_t)std::max(S.nsuper, 1) * sizeof(int)));
        HIP_CHECK(hipMemset(d_ov_done.p, 0, (size_t)std::max(S.nsuper, 1) * sizeof(int)));
        d_tinv_off.upload(T.toff);
        d_desc.upload(T.desc);
        d_sdesc.upload(T.sdesc);
        d_spos.upload(sch.spos);
        d_sn_parent.upload(S.sn_parent);
        if (!sch.tp.empty()) {       // the set has sliced fronts: the tasks of k_top_solve_sliced
            d_tk_pos.upload(sch.tp); d_tk_sl.upload(sch.ts); d_tbase.upload(sch.h_tbase);
            xf.alloc((size_t)S.N * 2);
        }
        top_flags.alloc((size_t)2 * std::max(sch.top_nflag, 1) + 4);
        HIP_CHECK(hipMemset(top_flags.p, 0, top_flags.n * sizeof(int)));
        d_chain_nchild.upload(sch.nch);
        d_chain.alloc((size_t)2 * std::max(S.nsuper, 1));
        HIP_CHECK(hipMemset(d_chain.p, 0, d_chain.n * sizeof(int)));
        tinv.alloc((size_t)T.toff[S.nsuper]);
        HIP_CHECK(hipMemset(tinv.p, 0, std::max<size_t>(tinv.n, 1) * sizeof(double)));
        d_tinv_list.upload(sch.tinv_list);
        d_cut_ptr.upload(T.cut_ptr);
        d_cuts.upload(T.cuts);
        if (verbose >= 2 && sch.top_launches > 0) std::fputs(describe_gather_sources(S, sch, T).c_str(), stderr);
        d_item_ptr.upload(T.item_ptr);
        // extend-add items of the PANEL columns and Schur sub-items of the update-block columns: schedule.cpp
        d_dense_off.upload(fl.dense_off);
        if (verbose) {
            std::fputs(describe_update_blocks(S, fl).c_str(), stderr);
            if (verbose >= 2) std::fputs(describe_pieces(S, sch, fl).c_str(), stderr);      // the "[pieces]" lines of this handle's lists
            std::fputs(describe_pulled_terms(fl).c_str(), stderr);
        }
        d_items.upload(fl.items);
        d_wave_cut.upload(fl.wcut);
        if (verbose >= 2) std::fputs(describe_panel_items(S, sch, fl).c_str(), stderr);
        if (verbose) std::fputs(describe_tile_order(T).c_str(), stderr);
        d_tiles.upload(T.tiles);       // (the tiles in the order they are launched in; tcut / ptcut follow it)
        d_sitems.upload(fl.sit);
        d_tile_cut.upload(fl.tcut);
#ifdef HIPKKT_EXPERIMENTS
        // EXPERIMENT (timing only, WRONG RESULTS; never in the default build): the pulled leaves' items and sub-items are
        // gone and their update blocks are not stored, but nobody forms their terms either -- what the factorisation
        // would take if the leaves' extend-add cost nothing: the ceiling of HIPKKT_PULL_FACTOR_LEAVES
        if (std::getenv("HIPKKT_EXPERIMENT_DROP_LEAF_UPDATES")) {
            fl.pterms.assign(1, PullTerm{});
            std::fill(fl.pwcut.begin(), fl.pwcut.end(), 0);
            std::fill(fl.ptcut.begin(), fl.ptcut.end(), 0);
        }
#endif
        // the pulled leaves' terms and their chunk ranges per wave slice / tile wave
        d_pterms.upload(fl.pterms);
        d_pwave_cut.upload(fl.pwcut);
        d_ptile_cut.upload(fl.ptcut);
        d_gl_src.upload(T.gsrc);
        if (!T.recs.empty()) d_recs.upload(T.recs);
        if (verbose) std::fputs(describe_records(sch).c_str(), stderr);
        d_udst.upload(T.udst);
        // the many-column sweeps' split gather lists (engine_tables.hpp: PULLED LEAVES)
        d_glm_ptr.upload(T.glm_ptr); d_udst_m.upload(T.udst_m); d_hp_col.upload(T.hp_col); d_hp_row.upload(T.hp_row); d_hp_lidx.upload(T.hp_lidx);
        d_pr_ptr.upload(T.pr_ptr); d_pr_slot.upload(T.pr_slot);
        if (verbose) std::fputs(describe_solve_pulled(T).c_str(), stderr);
        d_perm.upload(S.perm);
        d_psign.upload(T.psign);
        if (T.tall_ws) { tall_ws.alloc(T.tall_ws); tall_ws.zero(nullptr); HIP_CHECK(hipStreamSynchronize(nullptr)); }     // (its first N doubles: ticket words, zero between sweeps)
        fronts.alloc((size_t)S.front_store);
        upd.alloc((size_t)S.update_store);
        Dinv.alloc((size_t)S.N);
        xp.alloc((size_t)S.N);
        uvec.alloc(S.rows.size());
        flags.alloc(12);      // [0..2] status words, [3..6] which wait expired (diagnostic), [8..9] concurrency probe
        HIP_CHECK(hipMemset(fronts.p, 0, std::max<size_t>(fronts.n, 1) * sizeof(double)));
        HIP_CHECK(hipMemset(Dinv.p, 0, std::max<size_t>(Dinv.n, 1) * sizeof(double)));
        HIP_CHECK(hipMemset(flags.p, 0, 12 * sizeof(int)));
    }
};

static void fill_info(const Symbolic& S, hipkkt_info* info)
{
    info->N = S.N;
    info->nnzK = S.nnzK;
    info->nnzL = S.nnzL_struct;
    info->nnzL_stored = S.nnzL;
    info->nsuper = S.nsuper;
    info->nlevels = (int64_t)S.levels.size();
    info->max_front = S.max_front;
    info->etree_height = S.etree_height;
    info->factor_flops = S.flops;
    info->front_bytes = (double)S.front_store * 8.0;
    info->update_bytes = (double)S.update_store * 8.0;
}

struct PinnedScalars {
    double* h = nullptr;
    PinnedScalars() { HIP_CHECK(hipHostMalloc((void**)&h, 72 * sizeof(double))); }   // [8..11] update status, [16..35] refinement read-back, [40..47] sticky, [52..64] step / residual record
    ~PinnedScalars() { if (h) (void)hipHostFree(h); }
};

// phase timing with hipEvents on the handle's stream
struct Profiler {
    bool enabled = false;
    struct Span { hipEvent_t a, b; int phase; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> pool;
    hipkkt_profile acc{};
    hipEvent_t get()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        return e;
    }
    int begin(int phase, hipStream_t st)
    {
        if (!enabled) return -1;
        Span s{get(), get(), phase};
        HIP_CHECK(hipEventRecord(s.a, st));
        spans.push_back(s);
        return (int)spans.size() - 1;
    }
    void end(int id, hipStream_t st)
    {
        if (id < 0) return;
        HIP_CHECK(hipEventRecord(spans[id].b, st));
    }
    void resolve()
    {
        for (Span& s : spans) {
            HIP_CHECK(hipEventSynchronize(s.b));
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, s.a, s.b));
            switch (s.phase) {
            case 0: acc.update_ms += ms; acc.n_update++; break;
            case 1: acc.factor_ms += ms; acc.n_factor++; break;
            case 2: acc.trisolve_ms += ms; acc.n_trisolve++; break;
            case 3: acc.residual_ms += ms; acc.n_residual++; break;
            default: acc.other_ms += ms;
            }
            pool.push_back(s.a);
            pool.push_back(s.b);
        }
        spans.clear();
    }
    ~Profiler()
    {
        for (Span& s : spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    }
};

}  // namespace hipkkt

using namespace hipkkt;

// ====================================================================================
//  handles
// ====================================================================================
struct hipkkt_ldl_s {
    int device = 0;
    hipkkt_settings st;
    hipStream_t stream = nullptr;
    int64_t N = 0, nnzK = 0;
    int base = 0;
    std::unique_ptr<LDLEngine> eng;
    DBuf<double> Kval, vals, b, x;
    DBuf<double> mB;             // host-pointer solve_multi staging, N x mcap
    size_t mcap = 0;
    DBuf<int> idx;
    ~hipkkt_ldl_s() { if (stream) (void)hipStreamDestroy(stream); }
};

struct hipkkt_kkt_s {
    int device = 0;
    hipkkt_settings st;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    KKTAssembly K;
    std::unique_ptr<LDLEngine> eng;
    // values and maps
    DBuf<double> Kval, Pval, Aval;
    DBuf<int> mapP, mapA, mapHs, mapDiag, mapU, mapV, mapD, soc_of_entry;
    // residual SpMV
    DBuf<int64_t> fptr;
    DBuf<int> fcol, fmap;
    DBuf<int64_t> fpend;         // rows < n: end of the row's P entries in the image (SpmvDev::pend)
    DBuf<double> fval;               // K values in the CSR image's order: gathered whole after P / A changed (fval_dirty), kept
    bool fval_dirty = true;          //   current by write-through from the cone update otherwise (kpos: two slots per K entry)
    DBuf<int> kpos;
    // long rows of the image (kernels.hpp, SpmvDev)
    DBuf<int> long_rows;
    DBuf<int64_t> long_chunk_ptr, chunk_q;
    DBuf<double> long_partial;
    int nlong = 0, nchunks = 0;
    size_t long_partial_cols = 0;
    int lanes_per_row = 8;
    // the prefixes the iterate-residual pass walks (iterate_rows.hpp; kernels.hpp: IterDev), its slots and long-row sums
    DBuf<int64_t> it_rend, it_long_chunk_ptr, it_chunk_q;
    DBuf<int> it_long_rows;
    std::vector<int> it_long_rows_h;                             // ... on the host, for hipkkt_kkt_system_set_problems
    DBuf<double> it_long_partial, it_partial;
    int it_nlong = 0, it_nchunks = 0;
    bool it_prefix_ok = true;
    // vectors
    DBuf<double> b, x, e, dx, rx, rz, sbuf, zbuf, ybuf;
    double *cur_x = nullptr, *cur_dx = nullptr;
    DBuf<double> partial, scal;      // scal: [0] eps, [1] norme, [2] normb
    std::unique_ptr<PinnedScalars> pin;
    // cones
    DBuf<int> c_kind, c_off, c_numel, c_sidx, c_soff, c_elem, c_soclist;
    DBuf<int64_t> c_boff;
    DBuf<double> w, eta, soc_u, soc_v, soc_eta2, Hs;
    DBuf<int> fail;
    int nsoc = 0, npsd = 0, psd_kmax = 1;
    // exponential and power cones: lists, per-cone index among them and alpha, grad f*(z) (3 each) and H*(z) (9 each);
    // the strategy and mu of hipkkt_kkt_set_nonsymmetric_scaling travel to the scaling kernel as arguments
    DBuf<int> c_explist, c_powlist, c_nsidx;
    DBuf<double> c_param, ns_grad, ns_H;
    int nexp = 0, npow = 0, ns_strategy = HIPKKT_SCALING_PRIMAL_DUAL;
    double ns_mu = 0.0;
    // generalized power cones (kernels.hpp, ConeDev / ConeState); gp_mu: the mu of the scaling now on the device
    DBuf<int> gp_cone, gp_dim1, gp_off, gp_small, gp_big, gp_mapP, gp_mapQR, gp_mapD;
    DBuf<double> gp_alpha, gp_grad, gp_d, gp_p, gp_qr;
    int ngp_small = 0, ngp_big = 0;
    double gp_mu = 0.0;
    DBuf<int> c_psdlist, c_psddim;
    DBuf<int64_t> c_psdaoff;
    DBuf<double> psdA, psdR, psdRinv;
    bool has_psd = false, psd_too_big = false, scaling_valid = false;
    // the big class (side > kPsdMaxDim; kernels.hpp, ConeDev): listed at creation, handed to the kernels only after
    // hipkkt_kkt_enable_large_psd, which also allocates psd_work
    DBuf<int> c_psdblist;
    DBuf<double> psd_work;
    int npsdb = 0, psdb_kmax = 1;
    bool large_psd = false;
    double last_eps = 0;
    int64_t last_ir = 0;
    // refinement on the device (k_ir_round): state slots (4 doubles per round), a 5-double read-back record, the
    // sticky deferred-status record (8 doubles)
    DBuf<double> irbuf;
    double *ir_state = nullptr, *ir_readback = nullptr, *ir_sticky = nullptr, *ir_norms = nullptr, *sys_out_dev = nullptr;
    int ir_stride = 0;
    int r_spec = 1;                  // refinement rounds enqueued ahead of the first read-back (= what the previous solve took)
    bool publish_ok = true;          // the status record reaches the host by the call's last kernel (kernels.hpp: Publish); false: by a copy
    long long publish_seq = 0;
    int spec_low_calls = 0;          // status records in a row whose solves took fewer rounds than were enqueued (kkt_eval_sticky)
    bool deferred = false;           // hipkkt_kkt_set_deferred_status
    // level C (DefaultKKTSystem on the device, kktsystem.jl:21-215)
    DBuf<double> lam;                                        // scaled point, m
    DBuf<double> sq, snegq, sb, sx2, sz2, sworkx, sworkz, sconic, spa, spb, spc;
    DBuf<double> sys_partial, sys_dots, sys_cached, sys_in;
    DBuf<double> ns_partial;                                 // ... of the *_ns entry points and the barrier (2 * barrier_partials)
    DBuf<double> step_partial, step_rec;                     // step length / margins: partial slots and the result record (12 doubles)
    bool sys_ready = false;
    bool sys_lazy = false;           // hipkkt_kkt_system_set_lazy: kkt_update! leaves (x2, z2) = K \ (-q, b) to the affine kkt_solve!
    bool sys_const_pending = false;  // ... and that solve is still due
    bool sys_update_unread = false;  // lazy mode: the last kkt_update!'s status sits in the sticky record, read with the next solve's
    // hipkkt_kkt_system_set_problems: the partition's tables on the device (batch_plan.hpp; kernels.hpp: BatchDev) and the
    // work space of the _batch entry points, all sized by the number of members.  bat_nb = 0: no partition.
    int bat_nb = 0, bat_nwg32 = 0, bat_nwg256 = 0, bat_nwgz = 0;
    DBuf<int> bat_xoff, bat_zoff, bat_xmem, bat_zmem, bat_cmem, bat_socptr, bat_psdptr, bat_lorder, bat_lptr;
    DBuf<int> bat_r32mem, bat_r32first, bat_r32ptr, bat_r256mem, bat_r256first, bat_r256ptr, bat_z256mem, bat_z256first, bat_z256ptr;
    DBuf<double> bat_degree;
    DBuf<double> bat_scal, bat_rec, bat_shift, bat_dtau;     // 4 nb scalars in, 12 nb results out, 3 nb shifts, nb dtau
    DBuf<double> bat_it_partial, bat_step_partial, bat_dot_partial;
    double* bat_pin = nullptr;       // page-locked: [0, 4 nb) the scalars on their way up, [4 nb, 16 nb) the results on their way down
    hipEvent_t bat_ev = nullptr;     // behind the last upload from bat_pin: waited for before bat_pin is written again
    BatchDev batch_dev() const
    {
        BatchDev B;
        B.nb = bat_nb;
        B.x_off = bat_xoff.p; B.z_off = bat_zoff.p; B.xmem = bat_xmem.p; B.zmem = bat_zmem.p; B.cone_mem = bat_cmem.p;
        B.soc_ptr = bat_socptr.p; B.psd_ptr = bat_psdptr.p; B.degree = bat_degree.p;
        B.rows32 = BatchChunksDev{bat_r32mem.p, bat_r32first.p, bat_r32ptr.p, bat_nwg32};
        B.rows256 = BatchChunksDev{bat_r256mem.p, bat_r256first.p, bat_r256ptr.p, bat_nwg256};
        B.z256 = BatchChunksDev{bat_z256mem.p, bat_z256first.p, bat_z256ptr.p, bat_nwgz};
        B.long_order = bat_lorder.p; B.long_ptr = bat_lptr.p;
        return B;
    }
    // hipkkt_kkt_system_set_member_refinement: the tables of plan_batch_image on the device, the slots and the members'
    // state (kernels.hpp: MemberIrDev), all allocated when the rule is enabled.  mr_valid: a solve has run under it.
    bool mr_on = false, mr_valid = false;
    BatchPlan bat_plan;              // the partition on the host
    std::vector<int> long_rows_h;    // the image's long rows on the host
    int mr_nwg = 0, mr_chunk = 0;
    DBuf<int> mr_wgmem, mr_wgfirst, mr_wgptr, mr_rows, mr_ptr, mr_lorder, mr_lptr;
    DBuf<double> mr_slots, mr_state, mr_normb, mr_info;
    DBuf<unsigned long long> mr_agg;
    MemberIrDev member_dev() const
    {
        MemberIrDev M;
        M.nb = bat_nb; M.N = K.N; M.chunk = mr_chunk; M.nwg = mr_nwg;
        M.wg_mem = mr_wgmem.p; M.wg_first = mr_wgfirst.p; M.wg_ptr = mr_wgptr.p;
        M.img_rows = mr_rows.p; M.img_ptr = mr_ptr.p; M.long_order = mr_lorder.p; M.long_ptr = mr_lptr.p;
        M.slots = mr_slots.p; M.state = mr_state.p; M.normb = mr_normb.p; M.info = mr_info.p; M.agg = mr_agg.p;
        return M;
    }
    // hipkkt_kkt_system_set_member_status: row -> member and column -> member on the device, the maxima's words, the column
    // table of regularisers and the record {eps_b (nb doubles), cone words, pivot words (nb ints each)} that
    // hipkkt_kkt_system_member_status reads back in one copy -- all allocated when the mode is enabled.  ms_valid: an update
    // has run under it.
    bool ms_on = false, ms_valid = false;
    DBuf<int> ms_rowmem, ms_colmem;
    DBuf<unsigned long long> ms_maxbits;
    DBuf<double> ms_epscol, ms_rec;
    bool member_status_on() const { return ms_on && bat_nb > 0; }
    MemberStatusDev member_status_dev() const
    {
        MemberStatusDev M;
        M.nb = bat_nb; M.N = K.N;
        M.rowmem = ms_rowmem.p; M.colmem = ms_colmem.p; M.maxbits = ms_maxbits.p;
        M.eps_mem = ms_rec.p; M.eps_col = ms_epscol.p;
        M.cone_fail = (int*)(ms_rec.p + bat_nb); M.piv_bad = M.cone_fail + bat_nb;
        return M;
    }
    // data updating (hipkkt_kkt_system_set_equilibration and the four hipkkt_kkt_system_update_data_* calls): the frozen
    // scalings d, 1/d (n), e, 1/e (m) and c, every stored P / A entry's row and column (data_update.hpp) and the staging of
    // an indexed update's positions -- all built once (data_ensure), sized for the longest update there can be
    DBuf<double> eq_d, eq_dinv, eq_e, eq_einv, du_norms;
    double eq_c = 1.0;
    bool eq_ready = false;
    DBuf<int> du_Prow, du_Pcol, du_Arow, du_Acol;
    DBuf<int64_t> du_idx;
    // hipkkt_kkt_system_set_equilibration_batch: one cost scaling per member of the partition (eqb_on), on the host and the
    // device, and nothing derived from them; eq_c is left as it was.  hipkkt_kkt_system_data_norms_batch: every combined
    // row's word (data_update.hpp: build_norm_slots), built for the current partition on first use, and the 2 nb words.
    bool eqb_on = false;
    std::vector<double> eqb_c_h;
    DBuf<double> eqb_c, eqb_norms;
    DBuf<int> eqb_slot;
    bool eqb_slot_ready = false;
    bool data_factor_stale = false;  // P or A changed since the last factorisation
    bool data_const_stale = false;   // P, A, q or b changed since (x2, z2) and the cached constant terms were formed
    DBuf<double> hst;                // staging of the *_host entry points of level C: 3 x (n + 2 m) doubles (rhs, variables, lhs)
    bool host_vars_valid = false;    // hst holds the variables of the previous hipkkt_kkt_system_solve_host call
    // "the caller's host arrays may be reused": an event behind the uploads, waited for at the end of the call -- the
    // kernels enqueued in between keep the device busy meanwhile (a stream synchronise would wait for them as well)
    hipEvent_t ev_upload = nullptr;
    void host_upload_mark(hipStream_t st)
    {
        if (!ev_upload) HIP_CHECK(hipEventCreateWithFlags(&ev_upload, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(ev_upload, st));
    }
    void host_upload_wait() { if (ev_upload) HIP_CHECK(hipEventSynchronize(ev_upload)); }
    // solve_multi work space, N x mcap each (grown on demand)
    DBuf<double> mB, mX, mC, mE, mE2, mpartial, mnorms;
    DBuf<int> mmask;
    size_t mcap = 0;
    Profiler prof;
    ~hipkkt_kkt_s()
    {
        if (ev_upload) (void)hipEventDestroy(ev_upload);
        if (bat_ev) (void)hipEventDestroy(bat_ev);
        if (bat_pin) (void)hipHostFree(bat_pin);
        if (stream && own_stream) (void)hipStreamDestroy(stream);
    }

    ConeDev cone_dev() const
    {
        ConeDev C;
        C.ncones = (int)K.cones.size();
        C.kind = c_kind.p; C.off = c_off.p; C.numel = c_numel.p; C.boff = c_boff.p; C.sidx = c_sidx.p;
        C.soff = c_soff.p; C.elem_cone = c_elem.p; C.soc_list = c_soclist.p; C.nsoc = nsoc;
        C.psd_list = c_psdlist.p; C.psd_dim = c_psddim.p; C.psd_aoff = c_psdaoff.p; C.npsd = npsd; C.psd_kmax = psd_kmax;
        C.exp_list = c_explist.p; C.nexp = nexp; C.pow_list = c_powlist.p; C.npow = npow; C.ns_index = c_nsidx.p;
        C.param = c_param.p; C.ns_strategy = ns_strategy; C.ns_mu = ns_mu;
        C.gp_cone = gp_cone.p; C.gp_dim1 = gp_dim1.p; C.gp_off = gp_off.p; C.gp_alpha = gp_alpha.p;
        C.gp_small = gp_small.p; C.gp_big = gp_big.p; C.ngp_small = ngp_small; C.ngp_big = ngp_big;
        C.gp_mapP = gp_mapP.p; C.gp_mapQR = gp_mapQR.p; C.gp_mapD = gp_mapD.p; C.gp_mu = gp_mu;
        C.psdb_list = c_psdblist.p; C.npsdb = large_psd ? npsdb : 0; C.psdb_kmax = psdb_kmax; C.psd_work = psd_work.p;
        return C;
    }
    ConeState cone_state()
    {
        ConeState S;
        S.w = w.p; S.eta = eta.p; S.u = soc_u.p; S.v = soc_v.p; S.eta2 = soc_eta2.p; S.Hs = Hs.p; S.fail = fail.p;
        S.psdA = psdA.p; S.psdR = psdR.p; S.psdRinv = psdRinv.p;
        S.lam = lam.p;
        S.ns_grad = ns_grad.p; S.ns_H = ns_H.p;
        S.gp_grad = gp_grad.p; S.gp_d = gp_d.p; S.gp_p = gp_p.p; S.gp_qr = gp_qr.p;
        S.Kval = Kval.p; S.fval = fval_dirty ? nullptr : fval.p; S.kpos = kpos.p;
        if (member_status_on()) { S.fail_mem = (int*)(ms_rec.p + bat_nb); S.cone_mem = bat_cmem.p; }
        return S;
    }
};

template <class F>
static int guarded(F&& f)
{
    try {
        return f();
    } catch (const ArgError& e) {
        g_last_error = e.what();
        return HIPKKT_ERR_ARG;
    } catch (const HipError& e) {
        g_last_error = e.what();
        return HIPKKT_ERR_HIP;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return HIPKKT_ERR_INTERNAL;
    }
}

static int select_device(const hipkkt_settings& st)
{
    int dev = st.device;
    if (dev < 0) HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipSetDevice(dev));
    return dev;
}

extern "C" {

int hipkkt_available(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return 0; }
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return std::strncmp(p.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

const char* hipkkt_last_error(void) { return g_last_error.c_str(); }
const char* hipkkt_version(void) { return "hipkkt 0.1.0 (gfx950)"; }

void hipkkt_default_settings(hipkkt_settings* s)
{
    s->static_regularization_constant = 1e-8;
    s->static_regularization_proportional = DBL_EPSILON * DBL_EPSILON;
    s->dynamic_regularization_eps = 1e-13;
    s->dynamic_regularization_delta = 2e-7;
    s->iterative_refinement_reltol = 1e-13;
    s->iterative_refinement_abstol = 1e-12;
    s->iterative_refinement_stop_ratio = 5.0;
    s->iterative_refinement_max_iter = 10;
    s->static_regularization_enable = 1;
    s->iterative_refinement_enable = 1;
    s->ordering = HIPKKT_ORDER_ND;
    s->nd_leaf_size = 1000;
    s->device = -1;
    s->user_perm = nullptr;
    s->amd_dense_scale = 1.5;
}

int hipkkt_symbolic_analyse(int64_t N, const int64_t* colptr, const int64_t* rowval, int base, int ordering,
                            int nd_leaf_size, int64_t* perm_out, hipkkt_info* info_out)
{
    return guarded([&]() {
        if (!colptr || !rowval || N <= 0 || N > 2000000000 || (base != 0 && base != 1))
            throw ArgError("hipkkt_symbolic_analyse: bad argument");
        if (ordering != HIPKKT_ORDER_AMD && ordering != HIPKKT_ORDER_ND && ordering != HIPKKT_ORDER_NATURAL)
            throw ArgError("hipkkt_symbolic_analyse: ordering must be AMD, ND or NATURAL");
        SymbolicOptions opt;
        opt.ordering = ordering;
        if (nd_leaf_size > 0) opt.nd_leaf_size = nd_leaf_size;
        apply_knobs(opt);
        Symbolic S;
        analyse((int)N, colptr, rowval, base, opt, S);
        if (knobs().dump_levels) {          // diagnostic: the shape of every tree level (host only)
            for (size_t l = 0; l < S.levels.size(); ++l) {
                int cnt = 0, fmax = 0, ncmax = 0, n8 = 0, n64 = 0;
                int lds3 = 0, lds2 = 0, lds1 = 0;        // panels (f > 64) that would fit 3 / 2 / 1 to a CU's LDS
                double flops = 0, panel = 0, upd = 0, cols = 0;
                for (int t = S.levels[l].begin; t < S.levels[l].end; ++t) {
                    const int sn = S.level_sn[t];
                    const int nc = S.sn_start[sn + 1] - S.sn_start[sn], nb = (int)(S.rowptr[sn + 1] - S.rowptr[sn]), f = nc + nb;
                    ++cnt; fmax = std::max(fmax, f); ncmax = std::max(ncmax, nc);
                    n8 += f <= 8; n64 += f <= 64;
                    if (f > 64) {
                        const size_t b = panel_lds_bytes(f, f * nc - nc * (nc - 1) / 2);
                        (b <= 52 * 1024 ? lds3 : b <= 79 * 1024 ? lds2 : lds1)++;
                    }
                    cols += nc; panel += (double)f * nc; upd += (double)nb * nb;
                    for (int j = 0; j < nc; ++j) { const double c = f - 1 - j; flops += c * c + 3 * c; }
                }
                std::fprintf(stderr, "[levels] %2zu: %6d fronts (%6d f<=8, %6d f<=64) fmax %4d ncmax %3d cols %7.0f panel %.2f MB "
                             "upd %.2f MB flops %.1f M | panels by LDS <=52K %d, <=79K %d, more %d\n", l, cnt, n8, n64, fmax, ncmax, cols, panel * 8e-6,
                             upd * 8e-6, flops * 1e-6, lds3, lds2, lds1);
            }
        }
        if (knobs().dump_levels) {          // ... and the extend-add pieces per parent level, for the schedule of a 256-CU device
            DeviceLimits dev;
            dev.top_solve_capacity = [](size_t, bool) { return 240; };
            dev.top_solve_capacity_nr = [](size_t, int) { return 240; };
            dev.top_solve_sliced_capacity = [](size_t, int) { return 240; };
            const Schedule sch = build_schedule(S, dev, opt.panel_cap, std::max(1, opt.panel_max_slices));
            std::fputs(describe_pieces(S, sch, build_factor_lists(S, sch)).c_str(), stderr);
        }
        if (knobs().dump_subtrees) {        // diagnostic: what the subtrees below a cut level look like (host only)
            {
                std::vector<int> hist(8, 0);
                int mx = 0;
                for (int sn = 0; sn < S.nsuper; ++sn) {
                    const int k = S.child_ptr[sn + 1] - S.child_ptr[sn];
                    mx = std::max(mx, k);
                    hist[k == 0 ? 0 : k <= 4 ? 1 : k <= 16 ? 2 : k <= 64 ? 3 : k <= 256 ? 4 : k <= 1024 ? 5 : 6]++;
                }
                std::fprintf(stderr, "[subtrees] children per front: 0: %d, 1-4: %d, 5-16: %d, 17-64: %d, 65-256: %d, 257-1024: %d, more: %d (max %d)\n",
                             hist[0], hist[1], hist[2], hist[3], hist[4], hist[5], hist[6], mx);
            }
            for (int cut = 0; cut < (int)S.levels.size() && cut < 10; ++cut) {
                std::vector<int> root_of((size_t)S.nsuper, -1);
                // level_sn is leaves first: walk from the top so that a parent's root is known before its children's
                for (int t = S.nsuper - 1; t >= 0; --t) {
                    const int sn = S.level_sn[(size_t)t];
                    if (S.sn_level[(size_t)sn] > cut) continue;
                    const int p = S.sn_parent[(size_t)sn];
                    root_of[(size_t)sn] = (p >= 0 && S.sn_level[(size_t)p] <= cut) ? root_of[(size_t)p] : sn;
                }
                struct St { double fronts = 0, cols = 0, snb = 0, bytes = 0, border = 0; int fmax = 0; };
                std::map<int, St> st;
                for (int sn = 0; sn < S.nsuper; ++sn) {
                    if (root_of[(size_t)sn] < 0) continue;
                    St& x = st[root_of[(size_t)sn]];
                    const int nc = S.sn_start[sn + 1] - S.sn_start[sn], nb = (int)(S.rowptr[sn + 1] - S.rowptr[sn]);
                    x.fronts += 1; x.cols += nc; x.snb += nb; x.bytes += 8.0 * (nc + nb) * nc * (nc + nb > 64 ? 2 : 1);
                    x.fmax = std::max(x.fmax, nc + nb);
                    if (root_of[(size_t)sn] == sn) x.border = nb;
                }
                St mx, sum;
                for (auto& kv : st) {
                    const St& x = kv.second;
                    mx.fronts = std::max(mx.fronts, x.fronts); mx.cols = std::max(mx.cols, x.cols); mx.snb = std::max(mx.snb, x.snb);
                    mx.bytes = std::max(mx.bytes, x.bytes); mx.border = std::max(mx.border, x.border); mx.fmax = std::max(mx.fmax, x.fmax);
                    sum.fronts += x.fronts; sum.cols += x.cols; sum.snb += x.snb; sum.bytes += x.bytes;
                }
                const double k = st.empty() ? 1.0 : (double)st.size();
                std::fprintf(stderr, "[subtrees] cut %d: %zu subtrees; fronts %.0f total, %.0f mean, %.0f max; cols %.0f mean %.0f max; "
                             "sum nb %.0f mean %.0f max; matrix %.1f MB total, %.0f KB mean, %.0f KB max; border max %.0f, fmax %d\n",
                             cut, st.size(), sum.fronts, sum.fronts / k, mx.fronts, sum.cols / k, mx.cols, sum.snb / k, mx.snb,
                             sum.bytes * 1e-6, sum.bytes / k * 1e-3, mx.bytes * 1e-3, mx.border, mx.fmax);
            }
        }
        if (perm_out) for (int64_t i = 0; i < N; ++i) perm_out[i] = S.perm[i];
        if (info_out) { std::memset(info_out, 0, sizeof(*info_out)); fill_info(S, info_out); }
        return HIPKKT_OK;
    });
}

// ------------------------------------------------------------------------ level A
int hipkkt_ldl_create(hipkkt_ldl_t* out, int64_t N, const int64_t* colptr, const int64_t* rowval,
                      const double* nzval, const int64_t* dsigns, const hipkkt_settings* settings, int base)
{
    return guarded([&]() {
        if (!out || !colptr || !rowval || !nzval || !dsigns || N <= 0 || N > 2000000000)
            throw ArgError("hipkkt_ldl_create: bad argument");
        if (base != 0 && base != 1) throw ArgError("index_base must be 0 or 1");
        std::unique_ptr<hipkkt_ldl_s> h(new hipkkt_ldl_s);
        if (settings) h->st = *settings; else hipkkt_default_settings(&h->st);
        h->device = select_device(h->st);
        HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->N = N;
        h->nnzK = colptr[N] - base;
        h->base = base;
        std::vector<int> ds((size_t)N);
        for (int64_t i = 0; i < N; ++i) ds[i] = dsigns[i] >= 0 ? 1 : -1;
        h->eng.reset(new LDLEngine((int)N, colptr, rowval, base, ds, h->st));
        h->eng->stream = h->stream;
        h->eng->set_device(h->device);
        h->Kval.alloc((size_t)h->nnzK);
        HIP_CHECK(hipMemcpy(h->Kval.p, nzval, (size_t)h->nnzK * sizeof(double), hipMemcpyHostToDevice));
        h->b.alloc((size_t)N);
        h->x.alloc((size_t)N);
        *out = h.release();
        return HIPKKT_OK;
    });
}

void hipkkt_ldl_destroy(hipkkt_ldl_t h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

static void ldl_stage_index(hipkkt_ldl_t h, const int64_t* index, int64_t k)
{
    std::vector<int> idx((size_t)k);
    for (int64_t i = 0; i < k; ++i) {
        int64_t v = index[i] - h->base;
        if (v < 0 || v >= h->nnzK) throw ArgError("value index out of range");
        idx[i] = (int)v;
    }
    if (h->idx.n < (size_t)k) h->idx.alloc((size_t)k);
    HIP_CHECK(hipMemcpyAsync(h->idx.p, idx.data(), (size_t)k * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
}

int hipkkt_ldl_update_values(hipkkt_ldl_t h, const int64_t* index, const double* values, int64_t k)
{
    return guarded([&]() {
        if (!h || k < 0 || (k > 0 && (!index || !values))) throw ArgError("hipkkt_ldl_update_values: bad argument");
        if (k == 0) return HIPKKT_OK;
        HIP_CHECK(hipSetDevice(h->device));
        ldl_stage_index(h, index, k);
        if (h->vals.n < (size_t)k) h->vals.alloc((size_t)k);
        HIP_CHECK(hipMemcpyAsync(h->vals.p, values, (size_t)k * sizeof(double), hipMemcpyHostToDevice, h->stream));
        launch_scatter(h->Kval.p, h->idx.p, h->vals.p, k, 1.0, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_ldl_scale_values(hipkkt_ldl_t h, const int64_t* index, double scale, int64_t k)
{
    return guarded([&]() {
        if (!h || k < 0 || (k > 0 && !index)) throw ArgError("hipkkt_ldl_scale_values: bad argument");
        if (k == 0) return HIPKKT_OK;
        HIP_CHECK(hipSetDevice(h->device));
        ldl_stage_index(h, index, k);
        launch_scale(h->Kval.p, h->idx.p, scale, k, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_ldl_refactor(hipkkt_ldl_t h)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        HIP_CHECK(hipSetDevice(h->device));
        h->eng->factor(h->Kval.p, nullptr);
        int fl[3];
        h->eng->read_flags(fl);
        if (fl[2]) {                                            // never expected; see LDLEngine::ov_gave_up
            h->eng->ov_gave_up();
            h->eng->factor(h->Kval.p, nullptr);
            h->eng->read_flags(fl);
        }
        return fl[1] ? HIPKKT_NUMERIC_FAILURE : HIPKKT_OK;      // directldl_qdldl.jl:79
    });
}

int hipkkt_ldl_solve_dev(hipkkt_ldl_t h, double* d_x, const double* d_b)
{
    return guarded([&]() {
        if (!h || !d_x || !d_b) throw ArgError("hipkkt_ldl_solve_dev: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        h->eng->solve(d_b, d_x);
        return HIPKKT_OK;
    });
}

int hipkkt_ldl_solve(hipkkt_ldl_t h, double* x, const double* b)
{
    return guarded([&]() {
        if (!h || !x || !b) throw ArgError("hipkkt_ldl_solve: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        HIP_CHECK(hipMemcpyAsync(h->b.p, b, (size_t)h->N * sizeof(double), hipMemcpyHostToDevice, h->stream));
        h->eng->solve(h->b.p, h->x.p, true);
        if (h->eng->top_aborted_sync()) {                  // never expected; see TopOwner
            h->eng->top_gave_up();
            h->eng->solve(h->b.p, h->x.p, false);
        }
        HIP_CHECK(hipMemcpyAsync(x, h->x.p, (size_t)h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_ldl_solve_multi_dev(hipkkt_ldl_t h, int64_t nrhs, double* d_X, int64_t ldx, const double* d_B, int64_t ldb)
{
    return guarded([&]() {
        if (!h || nrhs < 0 || (nrhs > 0 && (!d_X || !d_B || ldx < h->N || ldb < h->N)))
            throw ArgError("hipkkt_ldl_solve_multi_dev: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        h->eng->solve_multi(d_B, ldb, d_X, ldx, (int)nrhs);
        return HIPKKT_OK;
    });
}

int hipkkt_ldl_solve_multi(hipkkt_ldl_t h, int64_t nrhs, double* X, const double* B)
{
    return guarded([&]() {
        if (!h || nrhs < 0 || (nrhs > 0 && (!X || !B))) throw ArgError("hipkkt_ldl_solve_multi: bad argument");
        if (nrhs == 0) return HIPKKT_OK;
        HIP_CHECK(hipSetDevice(h->device));
        if ((size_t)nrhs > h->mcap) { h->mB.alloc((size_t)h->N * nrhs); h->mcap = (size_t)nrhs; }
        const size_t bytes = (size_t)h->N * nrhs * sizeof(double);
        HIP_CHECK(hipMemcpyAsync(h->mB.p, B, bytes, hipMemcpyHostToDevice, h->stream));
        h->eng->solve_multi(h->mB.p, h->N, h->mB.p, h->N, (int)nrhs);     // in place: every entry is read before its slot is written
        HIP_CHECK(hipMemcpyAsync(X, h->mB.p, bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_ldl_info(hipkkt_ldl_t h, hipkkt_info* info)
{
    return guarded([&]() {
        if (!h || !info) throw ArgError("hipkkt_ldl_info: bad argument");
        std::memset(info, 0, sizeof(*info));
        fill_info(h->eng->S, info);
        return HIPKKT_OK;
    });
}

int hipkkt_ldl_get_perm(hipkkt_ldl_t h, int64_t* perm)
{
    return guarded([&]() {
        if (!h || !perm) throw ArgError("hipkkt_ldl_get_perm: bad argument");
        for (int64_t i = 0; i < h->N; ++i) perm[i] = h->eng->S.perm[i];
        return HIPKKT_OK;
    });
}

int hipkkt_ldl_fallbacks(hipkkt_ldl_t h, int64_t out[2])
{
    return guarded([&]() {
        if (!h || !out) throw ArgError("hipkkt_ldl_fallbacks: bad argument");
        out[0] = h->eng->n_ov_fallbacks;
        out[1] = h->eng->n_top_fallbacks;
        return HIPKKT_OK;
    });
}

// ------------------------------------------------------------------------ level B
int hipkkt_kkt_create(hipkkt_kkt_t* out, int64_t n, int64_t m, const int64_t* Pcolptr, const int64_t* Prowval,
                      const double* Pnzval, const int64_t* Acolptr, const int64_t* Arowval, const double* Anzval,
                      int64_t ncones, const int32_t* kinds, const int64_t* dims, const hipkkt_settings* settings,
                      int base)
{
    return hipkkt_kkt_create_ex(out, n, m, Pcolptr, Prowval, Pnzval, Acolptr, Arowval, Anzval, ncones, kinds, dims, nullptr,
                                settings, base);
}

int hipkkt_kkt_create_ex(hipkkt_kkt_t* out, int64_t n, int64_t m, const int64_t* Pcolptr, const int64_t* Prowval,
                         const double* Pnzval, const int64_t* Acolptr, const int64_t* Arowval, const double* Anzval,
                         int64_t ncones, const int32_t* kinds, const int64_t* dims, const double* cone_params,
                         const hipkkt_settings* settings, int base)
{
    // one double per cone -> the ragged form: a power cone's alpha is the only value that travels
    std::vector<int64_t> pptr;
    std::vector<double> pvals;
    if (ncones > 0 && kinds) {
        for (int64_t c = 0; c < ncones; ++c)
            if (kinds[c] == HIPKKT_CONE_GENPOW) {
                g_last_error = "a generalized power cone has one alpha per row of its first block: use hipkkt_kkt_create_ex2";
                return HIPKKT_ERR_ARG;
            }
        if (cone_params) {
            pptr.assign((size_t)ncones + 1, base);
            for (int64_t c = 0; c < ncones; ++c) {
                pptr[(size_t)c + 1] = pptr[(size_t)c];
                if (kinds[c] == HIPKKT_CONE_POW) { pvals.push_back(cone_params[c]); pptr[(size_t)c + 1] += 1; }
            }
        }
    }
    return hipkkt_kkt_create_ex2(out, n, m, Pcolptr, Prowval, Pnzval, Acolptr, Arowval, Anzval, ncones, kinds, dims,
                                 pptr.empty() ? nullptr : pptr.data(), pvals.data(), settings, base);
}

int hipkkt_kkt_create_ex2(hipkkt_kkt_t* out, int64_t n, int64_t m, const int64_t* Pcolptr, const int64_t* Prowval,
                          const double* Pnzval, const int64_t* Acolptr, const int64_t* Arowval, const double* Anzval,
                          int64_t ncones, const int32_t* kinds, const int64_t* dims, const int64_t* cone_param_ptr,
                          const double* cone_param_vals, const hipkkt_settings* settings, int base)
{
    return guarded([&]() {
        if (!out || !Pcolptr || !Acolptr || n < 0 || m < 0 || ncones < 0 || (ncones > 0 && (!kinds || !dims)))
            throw ArgError("hipkkt_kkt_create: bad argument");
        if (base != 0 && base != 1) throw ArgError("index_base must be 0 or 1");
        if (n + m == 0) throw ArgError("empty problem");
        std::unique_ptr<hipkkt_kkt_s> h(new hipkkt_kkt_s);
        if (settings) h->st = *settings; else hipkkt_default_settings(&h->st);
        // host-side assembly first: a malformed (P, A, cones) is an argument error whether or not a device is there
        try {
            assemble_kkt(n, m, Pcolptr, Prowval, Pnzval, Acolptr, Arowval, Anzval, ncones, kinds, dims, base, h->K, cone_param_ptr,
                         cone_param_vals);
        } catch (const std::runtime_error& e) {
            throw ArgError(e.what());
        }
        h->device = select_device(h->st);
        HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        KKTAssembly& K = h->K;
        hipkkt_settings st = h->st;
        if (st.ordering == HIPKKT_ORDER_USER && !st.user_perm) throw ArgError("ORDER_USER needs user_perm");
        std::vector<int64_t> rv(K.rowval.begin(), K.rowval.end());
        // K is 0-based here; a user permutation stays in the caller's base
        std::vector<int64_t> uperm;
        if (st.ordering == HIPKKT_ORDER_USER) {
            uperm.resize(K.N);
            for (int i = 0; i < K.N; ++i) uperm[i] = st.user_perm[i] - base;
            st.user_perm = uperm.data();
        }
        h->eng.reset(new LDLEngine(K.N, K.colptr.data(), rv.data(), 0, K.dsigns, st));
        h->eng->stream = h->stream;
        h->eng->set_device(h->device);
        h->st.user_perm = nullptr;

        h->Kval.upload(K.nzval);
        h->mapP.upload(K.mapP);
        h->mapA.upload(K.mapA);
        h->mapHs.upload(K.mapHs);
        h->mapDiag.upload(K.map_diag);
        h->mapU.upload(K.mapU);
        h->mapV.upload(K.mapV);
        h->mapD.upload(K.mapD);
        h->Pval.alloc(K.mapP.size());
        h->Aval.alloc(K.mapA.size());
        // full symmetric CSR image of K for the residual (kkt_assembly.cpp)
        {
            const KKTImage I = build_kkt_image(K);
            h->fptr.upload(I.ptr);
            h->fcol.upload(I.col);
            h->fmap.upload(I.vmap);
            h->fpend.upload(I.pend);
            {
                // ... and what hipkkt_kkt_system_residuals walks: whole x rows, the A prefix of the z rows
                const IterateRows R = plan_iterate_rows(K.n, K.m, I.ptr.data(), I.col.data(), kLongRow, kLongChunk);
                h->it_prefix_ok = R.prefix_ok;
                h->it_rend.upload(R.rend);
                h->it_nlong = (int)R.long_rows.size();
                h->it_nchunks = (int)(R.chunk_q.size() / 2);
                h->it_long_rows_h = R.long_rows;
                if (h->it_nlong) {
                    h->it_long_rows.upload(R.long_rows);
                    h->it_long_chunk_ptr.upload(R.long_chunk_ptr);
                    h->it_chunk_q.upload(R.chunk_q);
                    h->it_long_partial.alloc((size_t)2 * h->it_nchunks);
                }
            }
            h->fval.alloc(I.vmap.size());
            h->kpos.upload(I.kpos);
            h->nlong = (int)I.long_rows.size();
            h->long_rows_h = I.long_rows;
            h->nchunks = (int)(I.chunk_q.size() / 2);
            if (h->nlong) {
                h->long_rows.upload(I.long_rows);
                h->long_chunk_ptr.upload(I.long_chunk_ptr);
                h->chunk_q.upload(I.chunk_q);
                h->long_partial.alloc((size_t)h->nchunks * kMaxNR);
                h->long_partial_cols = kMaxNR;
            }
            h->lanes_per_row = I.lanes_per_row;
        }
        const size_t N = (size_t)K.N;
        // right-hand side, solution, residual and candidate: up to kMaxNR columns share a sweep (kkt_solve_core)
        h->b.alloc(N * kMaxNR); h->x.alloc(N * kMaxNR); h->e.alloc(N * kMaxNR); h->dx.alloc(N * kMaxNR);
        HIP_CHECK(hipMemset(h->b.p, 0, N * kMaxNR * sizeof(double)));
        HIP_CHECK(hipMemset(h->x.p, 0, N * kMaxNR * sizeof(double)));
        h->cur_x = h->x.p;
        h->cur_dx = h->dx.p;
        h->rx.alloc((size_t)K.n); h->rz.alloc((size_t)K.m);
        h->sbuf.alloc((size_t)K.m); h->zbuf.alloc((size_t)K.m); h->ybuf.alloc((size_t)K.m);
        h->partial.alloc(2 * ((size_t)std::max(2, kMaxNR) * (2 * kNormParts + 1) + 8));      // (two halves: kkt_partials)
        h->scal.alloc(16);               // [0] eps, [1] norme, [2] normb, [3] abort, [4] speculative norme, [8..11] update status
        HIP_CHECK(hipMemset(h->scal.p, 0, 16 * sizeof(double)));
        h->pin.reset(new PinnedScalars);
        {
            h->ir_stride = 4 * (std::max(h->st.iterative_refinement_max_iter, 0) + 2);
            const size_t nstate = (size_t)h->ir_stride * kMaxNR;
            const size_t total = nstate + 5 * kMaxNR + 4 + 8 + 4 + 3 * kMaxNR;
            h->irbuf.alloc(total);
            HIP_CHECK(hipMemset(h->irbuf.p, 0, total * sizeof(double)));
            h->ir_state = h->irbuf.p;
            h->ir_readback = h->irbuf.p + nstate;
            h->ir_sticky = h->ir_readback + 5 * kMaxNR + 4;
            h->sys_out_dev = h->ir_sticky + 8;          // {dtau, dkappa, tau_num, tau_den} of kkt_solve!: read back with the record in ONE copy
            h->ir_norms = h->sys_out_dev + 4;           // several columns: norme0[kMaxNR], normb[kMaxNR], cand[kMaxNR]
        }
        // cones (kkt_assembly.cpp)
        {
            const ConeTables C = build_cone_tables(K);
            const size_t nc = K.cones.size();
            h->has_psd = C.has_psd; h->psd_too_big = C.psd_too_big;
            h->nsoc = (int)C.soc_list.size();
            h->nexp = (int)C.exp_list.size(); h->npow = (int)C.pow_list.size();
            if (K.nnonsym > 0) {
                h->c_explist.upload(C.exp_list); h->c_powlist.upload(C.pow_list); h->c_nsidx.upload(C.ns_index); h->c_param.upload(C.param);
                h->ns_grad.alloc((size_t)3 * K.nnonsym); h->ns_H.alloc((size_t)9 * K.nnonsym);
                HIP_CHECK(hipMemset(h->ns_grad.p, 0, (size_t)3 * K.nnonsym * sizeof(double)));
                HIP_CHECK(hipMemset(h->ns_H.p, 0, (size_t)9 * K.nnonsym * sizeof(double)));
            }
            if (K.ngenpow > 0) {
                h->ngp_small = (int)C.gp_small.size(); h->ngp_big = (int)C.gp_big.size();
                h->gp_cone.upload(C.gp_cone); h->gp_dim1.upload(C.gp_dim1); h->gp_off.upload(C.gp_off); h->gp_alpha.upload(C.gp_alpha);
                h->gp_small.upload(C.gp_small); h->gp_big.upload(C.gp_big);
                h->gp_mapP.upload(K.mapGP_p); h->gp_mapQR.upload(C.gp_mapQR); h->gp_mapD.upload(K.mapGP_D);
                const size_t gl = (size_t)K.genpow_len;
                h->gp_grad.alloc(gl); h->gp_d.alloc(gl); h->gp_p.alloc(gl); h->gp_qr.alloc(gl);
                for (double* q : {h->gp_grad.p, h->gp_d.p, h->gp_p.p, h->gp_qr.p}) HIP_CHECK(hipMemset(q, 0, gl * sizeof(double)));
            }
            h->psd_kmax = C.psd_kmax; h->psdb_kmax = C.psdb_kmax;
            h->npsd = (int)C.psd_list.size(); h->npsdb = (int)C.psdb_list.size();
            h->c_psdlist.upload(C.psd_list); h->c_psddim.upload(C.psd_dim); h->c_psdaoff.upload(C.psd_aoff);
            h->c_psdblist.upload(C.psdb_list);
            h->psdA.alloc((size_t)C.psd_store); h->psdR.alloc((size_t)C.psd_store); h->psdRinv.alloc((size_t)C.psd_store);
            h->c_kind.upload(C.kind); h->c_off.upload(C.off); h->c_numel.upload(C.numel); h->c_boff.upload(C.boff);
            h->c_sidx.upload(C.sidx); h->c_soff.upload(C.soff); h->c_elem.upload(C.elem_cone); h->c_soclist.upload(C.soc_list);
            h->soc_of_entry.upload(C.soc_of_entry);
            h->w.alloc((size_t)K.m); h->eta.alloc(nc); h->lam.alloc((size_t)K.m);
            h->soc_u.alloc((size_t)K.sparse_len); h->soc_v.alloc((size_t)K.sparse_len);
            h->soc_eta2.alloc((size_t)K.nsparse); h->Hs.alloc((size_t)K.nHs);
            h->fail.alloc(1);
            HIP_CHECK(hipMemset(h->fail.p, 0, sizeof(int)));
        }
        *out = h.release();
        return HIPKKT_OK;
    });
}

void hipkkt_kkt_destroy(hipkkt_kkt_t h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

int hipkkt_kkt_info(hipkkt_kkt_t h, hipkkt_info* info)
{
    return guarded([&]() {
        if (!h || !info) throw ArgError("hipkkt_kkt_info: bad argument");
        std::memset(info, 0, sizeof(*info));
        fill_info(h->eng->S, info);
        info->n = h->K.n; info->m = h->K.m; info->p = h->K.p;
        info->nHs = h->K.nHs; info->nsparse_soc = h->K.nsparse; info->sparse_soc_len = h->K.sparse_len;
        return HIPKKT_OK;
    });
}

// the cone-failure word in front of a value update and, under hipkkt_kkt_system_set_member_status, the members' words
// and the maxima in the same launch
static void kkt_zero_update_words(hipkkt_kkt_t h)
{
    if (!h->member_status_on()) { launch_zero_ints(h->fail.p, 1, h->stream); return; }
    ZeroList zl;
    zl.add(h->fail.p, 1);
    zl.add((int*)(h->ms_rec.p + h->bat_nb), 2 * h->bat_nb);
    zl.add((int*)h->ms_maxbits.p, 2 * (h->bat_nb + 1));
    launch_zero_ints_multi(zl, h->stream);
}

// scatter of -Hs and the sparse-cone columns, static regulariser, numeric factorisation
// (kktsolver_directldl.jl:211-294).  Hs/u/v/eta2 already on the device.
static int kkt_update_device(hipkkt_kkt_t h, bool deferred = false)
{
    KKTAssembly& K = h->K;
    const bool members = h->member_status_on();
    h->data_factor_stale = false;                    // (every value of Kval, updated P and A included, is factorised below)
    int pu = h->prof.begin(0, h->stream);
    // -Hs (:225-228) and the sparse cones' columns (:235-241) in one launch, written through to the residual's copy of K
    // when that copy is current (otherwise it is gathered whole before the next residual: kkt_spmv)
    launch_update_values(h->Kval.p, h->mapHs.p, h->Hs.p, (int)K.nHs, h->mapU.p, h->mapV.p, h->mapD.p, h->soc_u.p, h->soc_v.p,
                         h->soc_eta2.p, h->soc_of_entry.p, K.sparse_len, K.nsparse, h->fval_dirty ? nullptr : h->fval.p,
                         h->kpos.p, h->stream);
    const double* eps_ptr = nullptr;
    h->eng->eps_col = nullptr;
    if (h->st.static_regularization_enable) {                                      // :259-279
        if (members) {
            // eps_b from member b's own rows of the image, handed to the factor kernels column by column; scal[0]: the largest
            launch_member_regularizer(h->member_status_dev(), h->Kval.p, h->mapDiag.p, h->st.static_regularization_constant,
                                      h->st.static_regularization_proportional, h->scal.p, h->stream);
            h->eng->eps_col = h->ms_epscol.p;
        } else {
            launch_regularizer(h->Kval.p, h->mapDiag.p, K.N, h->st.static_regularization_constant,
                               h->st.static_regularization_proportional, h->partial.p, h->scal.p, h->stream);
        }
        eps_ptr = h->scal.p;
    }
    h->prof.end(pu, h->stream);
    int pf = h->prof.begin(1, h->stream);
    h->eng->factor(h->Kval.p, eps_ptr);          // K itself stays un-regularised (:283-291)
    if (members) {
        launch_member_pivot_scan(h->member_status_dev(), h->eng->dinv_ptr(), h->stream);
        h->ms_valid = true;
    }
    h->prof.end(pf, h->stream);
    // read back: flags, eps, cone failure
    // (one small kernel gathers the four words, one copy into pinned memory brings them over: three separate
    // copies, two of them into pageable memory, cost ~60 us of idle GPU per update)
    // (deferred: no read-back, the status joins the sticky record in the same launch -- hipkkt_kkt_deferred_status)
    launch_collect_status(h->scal.p + 8, h->scal.p, h->fail.p, h->eng->flags_ptr(), h->stream, deferred ? h->ir_sticky : nullptr);
    if (deferred) return HIPKKT_OK;
    HIP_CHECK(hipMemcpyAsync(h->pin->h + 8, h->scal.p + 8, 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (h->pin->h[12] != 0.0) {                      // never expected; see LDLEngine::ov_gave_up: repeat level by level
        h->eng->ov_gave_up();
        h->eng->factor(h->Kval.p, eps_ptr);
        if (members) launch_member_pivot_scan(h->member_status_dev(), h->eng->dinv_ptr(), h->stream);
        launch_collect_status(h->scal.p + 8, h->scal.p, h->fail.p, h->eng->flags_ptr(), h->stream);
        HIP_CHECK(hipMemcpyAsync(h->pin->h + 8, h->scal.p + 8, 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    h->last_eps = h->st.static_regularization_enable ? h->pin->h[8] : 0.0;
    h->prof.acc.dynamic_regularizations += (int64_t)h->pin->h[10];
    if (h->pin->h[9] != 0.0) return HIPKKT_NUMERIC_FAILURE;
    return h->pin->h[11] != 0.0 ? HIPKKT_NUMERIC_FAILURE : HIPKKT_OK;
}

int hipkkt_kkt_update_cones(hipkkt_kkt_t h, const double* Hs, const double* soc_u, const double* soc_v,
                            const double* soc_eta2)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        KKTAssembly& K = h->K;
        if ((K.nHs > 0 && !Hs) || (K.nsparse > 0 && (!soc_u || !soc_v || !soc_eta2)))
            throw ArgError("hipkkt_kkt_update_cones: missing cone data");
        if (K.ngenpow > 0)
            throw ArgError("hipkkt_kkt_update_cones: (Hs, u, v, eta^2) cannot carry p, q, r of a generalized power cone; such a "
                           "handle is scaled on the device (hipkkt_kkt_update_from_sz, hipkkt_kkt_system_update)");
        HIP_CHECK(hipSetDevice(h->device));
        if (K.nHs) HIP_CHECK(hipMemcpyAsync(h->Hs.p, Hs, (size_t)K.nHs * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (K.nsparse) {
            HIP_CHECK(hipMemcpyAsync(h->soc_u.p, soc_u, (size_t)K.sparse_len * sizeof(double), hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(h->soc_v.p, soc_v, (size_t)K.sparse_len * sizeof(double), hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(h->soc_eta2.p, soc_eta2, (size_t)K.nsparse * sizeof(double), hipMemcpyHostToDevice, h->stream));
        }
        kkt_zero_update_words(h);
        h->scaling_valid = false;
        return kkt_update_device(h);
    });
}

static int kkt_update_from_sz_dev_impl(hipkkt_kkt_t h, const double* d_s, const double* d_z, bool deferred)
{
    return guarded([&]() {
        if (!h || (h->K.m > 0 && (!d_s || !d_z))) throw ArgError("hipkkt_kkt_update_from_sz: bad argument");
        if (h->psd_too_big && !h->large_psd)
            throw ArgError("update_from_sz: PSD cones with side > 48 are scaled by the caller; use hipkkt_kkt_update_cones");
        if (h->psdb_kmax > kPsdBigMaxDim)
            throw ArgError("update_from_sz: PSD cones with side > 96 are scaled by the caller; use hipkkt_kkt_update_cones");
        HIP_CHECK(hipSetDevice(h->device));
        kkt_zero_update_words(h);
        int pu = h->prof.begin(0, h->stream);
        h->gp_mu = h->ns_mu;
        launch_cone_scaling(h->cone_dev(), h->cone_state(), d_s, d_z, h->K.m, h->stream);
        h->prof.end(pu, h->stream);
        h->scaling_valid = true;
        return kkt_update_device(h, deferred);
    });
}
// Opt-in to the big PSD class (hipkkt.h).  The flag decides what cone_dev() hands to the launchers; a scaling made under
// the other setting does not cover the same cones, so it stops being valid.
int hipkkt_kkt_enable_large_psd(hipkkt_kkt_t h, int enable)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        HIP_CHECK(hipSetDevice(h->device));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        const bool on = enable != 0;
        if (on && h->npsdb > 0 && h->psdb_kmax <= kPsdBigMaxDim && !h->psd_work.p) {
            const size_t n = (size_t)3 * h->psdb_kmax * h->psdb_kmax * h->npsdb;
            h->psd_work.alloc(n);
            HIP_CHECK(hipMemset(h->psd_work.p, 0, n * sizeof(double)));
        }
        if (on != h->large_psd && h->npsdb > 0) h->scaling_valid = false;
        h->large_psd = on;
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_update_from_sz_dev(hipkkt_kkt_t h, const double* d_s, const double* d_z)
{
    return kkt_update_from_sz_dev_impl(h, d_s, d_z, h && h->deferred);
}

int hipkkt_kkt_update_from_sz(hipkkt_kkt_t h, const double* s, const double* z)
{
    return guarded([&]() {
        if (!h || (h->K.m > 0 && (!s || !z))) throw ArgError("hipkkt_kkt_update_from_sz: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        size_t bytes = (size_t)h->K.m * sizeof(double);
        if (bytes) {
            HIP_CHECK(hipMemcpyAsync(h->sbuf.p, s, bytes, hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(h->zbuf.p, z, bytes, hipMemcpyHostToDevice, h->stream));
        }
        return hipkkt_kkt_update_from_sz_dev(h, h->sbuf.p, h->zbuf.p);
    });
}

int hipkkt_kkt_update_P(hipkkt_kkt_t h, const double* Pnzval)
{
    return guarded([&]() {
        if (!h || (h->K.mapP.size() && !Pnzval)) throw ArgError("hipkkt_kkt_update_P: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        size_t k = h->K.mapP.size();
        if (!k) return HIPKKT_OK;
        HIP_CHECK(hipMemcpyAsync(h->Pval.p, Pnzval, k * sizeof(double), hipMemcpyHostToDevice, h->stream));
        launch_scatter(h->Kval.p, h->mapP.p, h->Pval.p, (int64_t)k, 1.0, h->stream);
        h->fval_dirty = true;
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_update_A(hipkkt_kkt_t h, const double* Anzval)
{
    return guarded([&]() {
        if (!h || (h->K.mapA.size() && !Anzval)) throw ArgError("hipkkt_kkt_update_A: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        size_t k = h->K.mapA.size();
        if (!k) return HIPKKT_OK;
        HIP_CHECK(hipMemcpyAsync(h->Aval.p, Anzval, k * sizeof(double), hipMemcpyHostToDevice, h->stream));
        launch_scatter(h->Kval.p, h->mapA.p, h->Aval.p, (int64_t)k, 1.0, h->stream);
        h->fval_dirty = true;
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_setrhs_dev(hipkkt_kkt_t h, const double* d_rx, const double* d_rz)
{
    return guarded([&]() {
        if (!h || (h->K.n && !d_rx) || (h->K.m && !d_rz)) throw ArgError("hipkkt_kkt_setrhs: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        launch_pack_rhs(h->b.p, d_rx, d_rz, h->K.n, h->K.m, h->K.p, h->stream);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_setrhs(hipkkt_kkt_t h, const double* rx, const double* rz)
{
    return guarded([&]() {
        if (!h || (h->K.n && !rx) || (h->K.m && !rz)) throw ArgError("hipkkt_kkt_setrhs: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        if (h->K.n) HIP_CHECK(hipMemcpyAsync(h->rx.p, rx, (size_t)h->K.n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (h->K.m) HIP_CHECK(hipMemcpyAsync(h->rz.p, rz, (size_t)h->K.m * sizeof(double), hipMemcpyHostToDevice, h->stream));
        launch_pack_rhs(h->b.p, h->rx.p, h->rz.p, h->K.n, h->K.m, h->K.p, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));     // rx/rz staging may be overwritten by the next call
        return HIPKKT_OK;
    });
}

// the full-symmetric CSR image of K with its values streamed in CSR order
static SpmvDev kkt_spmv(hipkkt_kkt_t h)
{
    if (h->fval_dirty) {
        launch_gather_values(h->fval.p, h->Kval.p, h->fmap.p, (int64_t)h->fmap.n, h->stream);
        h->fval_dirty = false;
    }
    SpmvDev A;
    A.ptr = h->fptr.p; A.col = h->fcol.p; A.vmap = h->fmap.p; A.val = h->fval.p; A.N = h->K.N;
    A.pend = h->fpend.p;
    A.lanes_per_row = h->lanes_per_row;
    A.nlong = h->nlong; A.nchunks = h->nchunks; A.long_rows = h->long_rows.p; A.long_chunk_ptr = h->long_chunk_ptr.p;
    A.chunk_q = h->chunk_q.p; A.long_partial = h->long_partial.p;
    return A;
}

// e = b - K xi for nr columns (ld N); ||e_c||_inf -> norm_out[c], optionally ||b_c||_inf -> normb_out[c]; scal[3] carries
// the persistent solve kernel's abort word along.  Nothing is read back here.
// The norms' second stage: a finishing kernel behind the residual, or -- kkt_partials_mode -- left to k_ir_round, which
// reduces the partial maxima itself (kernels.hpp: IrPartials).  The first residual of a solve leaves its partials in the
// first half of h->partial, the candidates' residuals in the second half (both are read by the same k_ir_round).
static bool kkt_partials_mode(hipkkt_kkt_t h, int nr) { return residual_partials_ok(kkt_spmv(h), nr); }
static double* kkt_partials(hipkkt_kkt_t h, bool candidate) { return h->partial.p + (candidate ? h->partial.n / 2 : 0); }
static void kkt_enqueue_refine_error(hipkkt_kkt_t h, const double* xi, double* norm_out, double* normb_out, int nr, bool candidate)
{
    const SpmvDev A = kkt_spmv(h);
    const bool unfinished = kkt_partials_mode(h, nr);
    int pr = h->prof.begin(3, h->stream);
    // (||b|| rides along with the FIRST residual only; its slot is still named so that the b partials are written)
    launch_residual(A, h->Kval.p, h->b.p, xi, h->e.p, kkt_partials(h, candidate), unfinished ? nullptr : norm_out, h->stream, nr,
                    nr > 1 ? (int64_t)h->K.N : 0, h->eng->top_abort_word(), h->scal.p + 3, normb_out);
    h->prof.end(pr, h->stream);
}
static void kkt_trisolve(hipkkt_kkt_t h, const double* rhs, double* out, bool allow_top = true, int nr = 1)
{
    int ps = h->prof.begin(2, h->stream);
    h->eng->solve(rhs, out, allow_top, nr, h->K.N, h->K.N);
    h->prof.end(ps, h->stream);
}

// kktsolver_solve! with _iterative_refinement (kktsolver_directldl.jl:346-449); leaves the solution in h->x.
// The accept / stop rule of the loop runs on the device (k_ir_round): the host enqueues the first solve, its
// residual and r_spec refinement rounds (what the previous solve on this handle took) without waiting, then reads ONE
// 5-double record back -- or nothing at all in deferred-status mode.  Only when the device reports that the
// reference's loop would go on does the host add rounds, one read-back each.  A candidate is computed into h->dx and
// copied over h->x when accepted, so the solution always sits in the same buffer.
// Returns HIPKKT_OK or HIPKKT_NUMERIC_FAILURE.
struct IrNorms { double *norme0, *normb, *cand; };
static IrNorms kkt_ir_norms(hipkkt_kkt_t h, int nr)
{
    // one column: the residual kernel's single-column slots in scal; several: the per-column arrays
    if (nr == 1) return IrNorms{h->scal.p + 1, h->scal.p + 2, h->scal.p + 4};
    return IrNorms{h->ir_norms, h->ir_norms + kMaxNR, h->ir_norms + 2 * kMaxNR};
}
static void kkt_launch_ir(hipkkt_kkt_t h, int r, bool first, bool readback, bool fold, int nr)
{
    const hipkkt_settings& st = h->st;
    const IrNorms nm = kkt_ir_norms(h, nr);
    const double* abortw = h->eng->top_abort_word() ? h->scal.p + 3 : nullptr;
    IrPartials Q;
    const bool unfinished = kkt_partials_mode(h, nr);
    if (unfinished) {
        Q.np = residual_grid(kkt_spmv(h)) + 1;
        Q.e0 = kkt_partials(h, false);
        Q.b0 = Q.e0 + (size_t)nr * Q.np;
        Q.cand = r > 0 ? kkt_partials(h, true) : nullptr;
        Q.flag_in = h->eng->top_abort_word();
    }
    launch_ir_round(h->ir_state, h->ir_stride, r, first, nm.norme0, nm.normb, nm.cand, abortw, h->x.p, h->dx.p, h->K.N, nr,
                    st.iterative_refinement_abstol, st.iterative_refinement_reltol, st.iterative_refinement_stop_ratio,
                    std::max(st.iterative_refinement_max_iter, 0), readback ? h->ir_readback : nullptr,
                    (fold && (nr == 1 || unfinished)) ? h->ir_sticky : nullptr, h->stream, Q);
    if (fold && nr > 1 && !unfinished) launch_ir_fold(h->ir_state, h->ir_stride, r, nr, abortw, h->ir_sticky, h->stream);
}
static void kkt_enqueue_round(hipkkt_kkt_t h, int r, bool first, bool readback, bool fold, int nr)
{
    kkt_trisolve(h, h->e.p, h->dx.p, true, nr);                                   // dx = K^{-1} e
    launch_axpby_sum(h->dx.p, h->dx.p, h->x.p, (int64_t)h->K.N * nr, h->stream);  // prospective solution x + dx
    kkt_enqueue_refine_error(h, h->dx.p, kkt_ir_norms(h, nr).cand, nullptr, nr, true);  // e <- b - K (x + dx), its norm -> cand
    kkt_launch_ir(h, r, first, readback, fold, nr);
}
// The same loop with the rule applied per member of the partition (hipkkt_kkt_system_set_member_refinement; kernels.hpp:
// MemberIrDev): sweeps and residual passes run once per round over the whole stack, as long as any member is active; the
// protocol with the host -- r_spec rounds ahead, one 5-double record, the abort word and its repeat -- is the joint
// path's, on the aggregate over the members.  The initial state has a launch of its own here (round 0), so that e is zero
// on the rows of members that need no refinement before the first refinement sweep reads it.
static int kkt_solve_core(hipkkt_kkt_t h, bool may_defer, int nr, int64_t* ir_out, bool force_defer);
static void kkt_member_residual(hipkkt_kkt_t h, const MemberIrDev& M, const double* xi, bool first)
{
    const SpmvDev A = kkt_spmv(h);
    int pr = h->prof.begin(3, h->stream);
    launch_member_residual(A, h->Kval.p, M, h->b.p, xi, h->e.p, first, h->stream);
    h->prof.end(pr, h->stream);
}
static void kkt_member_ir(hipkkt_kkt_t h, const MemberIrDev& M, int r)
{
    const hipkkt_settings& st = h->st;
    launch_member_ir_round(M, r, h->eng->top_abort_word(), h->x.p, h->dx.p, h->e.p, st.iterative_refinement_abstol,
                           st.iterative_refinement_reltol, st.iterative_refinement_stop_ratio,
                           std::max(st.iterative_refinement_max_iter, 0), h->ir_readback, h->stream);
}
static void kkt_member_round(hipkkt_kkt_t h, const MemberIrDev& M, int r)
{
    kkt_trisolve(h, h->e.p, h->dx.p, true, 1);                                    // dx = K^{-1} e (zero on inactive members' rows)
    launch_axpby_sum(h->dx.p, h->dx.p, h->x.p, (int64_t)h->K.N, h->stream);       // prospective solution x + dx
    kkt_member_residual(h, M, h->dx.p, false);                                    // e <- b - K (x + dx), the members' norms
    kkt_member_ir(h, M, r);
}
static int kkt_solve_core_members(hipkkt_kkt_t h, int64_t* ir_out)
{
    const MemberIrDev M = h->member_dev();
    const int max_iter = std::max(h->st.iterative_refinement_max_iter, 0);
    int R = std::min(max_iter, std::max(h->r_spec, 0));
    h->mr_valid = false;
    kkt_trisolve(h, h->b.p, h->x.p, true, 1);
    kkt_member_residual(h, M, h->x.p, true);
    kkt_member_ir(h, M, 0);
    for (int r = 1; r <= R; ++r) kkt_member_round(h, M, r);
    for (;;) {
        HIP_CHECK(hipMemcpyAsync(h->pin->h + 16, h->ir_readback, 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        const double* rb = h->pin->h + 16;
        if (rb[4] != 0.0 && h->eng->top_abort_word() != nullptr) {      // never expected; see TopOwner
            h->eng->top_gave_up();                                      // the per-level path from now on: repeat the solve
            return kkt_solve_core(h, false, 1, ir_out, false);
        }
        const int64_t most = (int64_t)rb[1];
        h->last_ir = most;
        if (ir_out) ir_out[0] = most;
        h->mr_valid = true;
        if (rb[0] == 0.0 || R >= max_iter) break;
        ++R;                                                            // some member's loop goes on: one more round
        kkt_member_round(h, M, R);
    }
    h->prof.acc.ir_iterations += h->last_ir;
    // (a bad member does not end the others' loops: they finish first, then the solve as a whole fails)
    if (h->pin->h[16 + 2] != 0.0) return HIPKKT_NUMERIC_FAILURE;
    h->r_spec = (int)std::min<int64_t>(h->last_ir, max_iter);
    return HIPKKT_OK;
}
// nr = 1, 2 or 4 right-hand sides (columns of h->b, N apart) share every sweep; each column goes through the
// reference's loop on its own.  ir_out (nullable, nr entries): rounds per column (-1 in deferred mode).
static int kkt_solve_core(hipkkt_kkt_t h, bool may_defer = false, int nr = 1, int64_t* ir_out = nullptr, bool force_defer = false)
{
    const hipkkt_settings& st = h->st;
    const bool deferred = force_defer || (may_defer && h->deferred);
    h->cur_x = h->x.p;
    h->cur_dx = h->dx.p;
    h->last_ir = 0;
    if (ir_out) for (int c = 0; c < nr; ++c) ir_out[c] = deferred ? -1 : 0;
    if (h->mr_on && h->bat_nb > 0 && nr == 1 && !deferred && st.iterative_refinement_enable) return kkt_solve_core_members(h, ir_out);
    if (!st.iterative_refinement_enable) {
        kkt_trisolve(h, h->b.p, h->x.p, false, nr);   // nothing reads the abort word back on this path
        int bad = 0;
        launch_zero_ints(h->fail.p, 1, h->stream);
        launch_check_finite(h->x.p, h->K.N * nr, h->fail.p, h->stream);
        if (deferred) { launch_fold_flag(h->ir_sticky, h->fail.p, h->stream); return HIPKKT_OK; }
        HIP_CHECK(hipMemcpyAsync(&bad, h->fail.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return bad ? HIPKKT_NUMERIC_FAILURE : HIPKKT_OK;
    }
    const int max_iter = std::max(st.iterative_refinement_max_iter, 0);
    int R = std::min(max_iter, std::max(h->r_spec, deferred ? 1 : 0));
    const IrNorms nm = kkt_ir_norms(h, nr);
    kkt_trisolve(h, h->b.p, h->x.p, true, nr);        // (deferred mode reads the persistent kernel's abort word at the status query)
    kkt_enqueue_refine_error(h, h->x.p, nm.norme0, nm.normb, nr, false);     // e = b - K x, ||e||, ||b||
    if (R == 0) kkt_launch_ir(h, 0, true, !deferred, deferred, nr);
    for (int r = 1; r <= R; ++r) kkt_enqueue_round(h, r, r == 1, r == R && !deferred, r == R && deferred, nr);
    if (deferred) { h->last_ir = -1; return HIPKKT_OK; }
    int64_t total = 0;
    for (;;) {
        HIP_CHECK(hipMemcpyAsync(h->pin->h + 16, h->ir_readback, 5 * (size_t)nr * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        bool any_active = false, any_bad = false, aborted = false;
        total = 0;
        for (int c = 0; c < nr; ++c) {
            const double* rb = h->pin->h + 16 + 5 * c;
            any_active = any_active || rb[0] != 0.0;
            any_bad = any_bad || rb[2] != 0.0;
            aborted = aborted || rb[4] != 0.0;
            total += (int64_t)rb[1];
            if (ir_out) ir_out[c] = (int64_t)rb[1];
        }
        if (aborted && h->eng->top_abort_word() != nullptr) {           // never expected; see TopOwner
            h->eng->top_gave_up();                                      // the per-level path from now on: repeat the solve
            return kkt_solve_core(h, false, nr, ir_out);
        }
        h->last_ir = total;
        if (any_bad) { h->prof.acc.ir_iterations += total; return HIPKKT_NUMERIC_FAILURE; }
        if (!any_active || R >= max_iter) break;
        ++R;                                                            // the reference's loop goes on: one more round
        kkt_enqueue_round(h, R, false, true, false, nr);
    }
    h->prof.acc.ir_iterations += total;
    int64_t most = 0;
    for (int c = 0; c < nr; ++c) most = std::max<int64_t>(most, (int64_t)h->pin->h[16 + 5 * c + 1]);
    h->r_spec = (int)std::min<int64_t>(most, max_iter);
    return HIPKKT_OK;
}

int hipkkt_kkt_solve_dev(hipkkt_kkt_t h, double* d_lhsx, double* d_lhsz)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        HIP_CHECK(hipSetDevice(h->device));
        int rc = kkt_solve_core(h, true);
        if (rc != HIPKKT_OK) return rc;
        launch_unpack_lhs(d_lhsx, d_lhsz, h->cur_x, h->K.n, h->K.m, h->stream);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_speculative_rounds(hipkkt_kkt_t h, int set)
{
    if (!h) return -1;
    if (set >= 0) { h->r_spec = std::min(set, std::max(h->st.iterative_refinement_max_iter, 0)); h->spec_low_calls = 0; }
    return h->r_spec;
}

int hipkkt_kkt_set_deferred_status(hipkkt_kkt_t h, int defer)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        HIP_CHECK(hipSetDevice(h->device));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        launch_zero_ints((int*)h->ir_sticky, 16, h->stream);
        h->deferred = defer != 0;
        return HIPKKT_OK;
    });
}

// what the sticky record {bad, more, abort, rounds, #dyn. regularisations, eps, solves, overlap gave up} read back into
// pinned memory says about everything enqueued since the last query: OK / NUMERIC_FAILURE / REFINEMENT_INCOMPLETE
// gave_up_out (nullable): a bounded wait expired -- the factor (or the solution) is void, as opposed to "a solve would
// have refined further".  will_repeat: the caller repeats the whole attempt synchronously whenever this returns
// HIPKKT_REFINEMENT_INCOMPLETE, so that attempt's counts stay out of the profile (the repeat adds its own).
static int kkt_eval_sticky(hipkkt_kkt_t h, const double* s, bool* gave_up_out = nullptr, bool will_repeat = false)
{
        const int max_iter = std::max(h->st.iterative_refinement_max_iter, 0);
        const bool void_step = s[7] != 0.0 || (s[2] != 0.0 && h->eng->top_abort_word() != nullptr);
        const bool repeat = will_repeat && (void_step || (s[0] == 0.0 && s[1] != 0.0));
        if (gave_up_out) *gave_up_out = false;
        if (!repeat) h->prof.acc.ir_iterations += (int64_t)s[3];
        if (!(will_repeat && void_step)) h->prof.acc.dynamic_regularizations += (int64_t)s[4];   // (a void factorisation is repeated too)
        if (s[5] != 0.0 || !h->st.static_regularization_enable) h->last_eps = h->st.static_regularization_enable ? s[5] : 0.0;
        if (s[6] > 0.0) h->last_ir = (int64_t)(s[3] / s[6] + 0.5);      // mean rounds per solve since the last query
        // The give-up words come first (as on the synchronous paths: kkt_update_device, kkt_solve_core): after a bounded
        // wait expired the factor or the solution is void and may well be non-finite -- that is not a numeric failure of
        // the problem but a step to repeat, with the mechanism switched off.
        bool gave_up = false;
        if (s[7] != 0.0) { h->eng->ov_gave_up(); gave_up = true; }      // never expected; see LDLEngine::ov_gave_up
        if (s[2] != 0.0 && h->eng->top_abort_word() != nullptr) { h->eng->top_gave_up(); gave_up = true; }   // see TopOwner
        if (gave_up_out) *gave_up_out = gave_up;
        if (gave_up) return HIPKKT_REFINEMENT_INCOMPLETE;               // (the step's results are void: repeat it)
        if (s[0] != 0.0) return HIPKKT_NUMERIC_FAILURE;
        if (s[1] != 0.0) {                                              // some solve would have gone on refining
            h->r_spec = std::min(max_iter, h->r_spec + 1);
            h->spec_low_calls = 0;
            return HIPKKT_REFINEMENT_INCOMPLETE;
        }
        // The speculation depth comes down again: one solve that took two rounds (a borderline accept / stop decision)
        // would otherwise cost every later solve of the run a wasted sweep pair (seen once as 3.77 instead of 3.36 ms per
        // step).  Eight records in a row whose solves could all have done with one round fewer: one round fewer.
        if (s[6] > 0.0 && h->r_spec > 1 && s[3] <= s[6] * (double)(h->r_spec - 1)) {
            if (++h->spec_low_calls >= 8) { --h->r_spec; h->spec_low_calls = 0; }
        } else if (s[6] > 0.0) {
            h->spec_low_calls = 0;
        }
        return HIPKKT_OK;
}

int hipkkt_kkt_deferred_status(hipkkt_kkt_t h)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        HIP_CHECK(hipSetDevice(h->device));
        HIP_CHECK(hipMemcpyAsync(h->pin->h + 40, h->ir_sticky, 8 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        launch_zero_ints((int*)h->ir_sticky, 16, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->sys_update_unread = false;
        return kkt_eval_sticky(h, h->pin->h + 40);
    });
}

int hipkkt_kkt_solve(hipkkt_kkt_t h, double* lhsx, double* lhsz)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        HIP_CHECK(hipSetDevice(h->device));
        int rc = kkt_solve_core(h);
        if (rc != HIPKKT_OK) return rc;
        if (lhsx && h->K.n)
            HIP_CHECK(hipMemcpyAsync(lhsx, h->cur_x, (size_t)h->K.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (lhsz && h->K.m)
            HIP_CHECK(hipMemcpyAsync(lhsz, h->cur_x + h->K.n, (size_t)h->K.m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

// ---- several right-hand sides against one factorisation (SURVEY.md 8b "solve_multi", 8e(ii)).
// Per column exactly the sequence of kkt_solve_core: the refinement rounds run in lockstep over the
// columns that still need them; a column that has met its stopping rule is frozen (its candidate is
// not accepted any more), so every column ends where its own single solve would.
static void kkt_multi_reserve(hipkkt_kkt_t h, size_t k)
{
    k = (k + 15) & ~(size_t)15;                      // the row-major path pads the columns to a multiple of 16
    if (k <= h->mcap) return;
    const size_t N = (size_t)h->K.N;
    h->mB.alloc(N * k); h->mX.alloc(N * k); h->mC.alloc(N * k); h->mE.alloc(N * k); h->mE2.alloc(N * k);
    h->mpartial.alloc(std::max((size_t)(kNormParts + 1) * k, (size_t)2 * 512 * k));
    if (h->nlong && k > h->long_partial_cols) { h->long_partial.alloc((size_t)h->nchunks * k); h->long_partial_cols = k; }
    h->mnorms.alloc(2 * k);
    h->mmask.alloc(k);                               // (k is padded: enough for the row-major path's KP entries)
    h->mcap = k;
}

static int kkt_solve_multi_core(hipkkt_kkt_t h, int k, int64_t* ir_out)
{
    const hipkkt_settings& st = h->st;
    const int N = (int)h->K.N;
    const int64_t ld = N;
    std::vector<int64_t> ir((size_t)k, 0);
    auto trisolve = [&](const double* rhs, double* out) {
        int ps = h->prof.begin(2, h->stream);
        h->eng->solve_multi(rhs, ld, out, ld, k);
        h->prof.end(ps, h->stream);
    };
    trisolve(h->mB.p, h->mX.p);
    if (!st.iterative_refinement_enable) {
        int bad = 0;
        launch_zero_ints(h->fail.p, 1, h->stream);
        for (int j = 0; j < k; ++j) launch_check_finite(h->mX.p + (size_t)j * N, N, h->fail.p, h->stream);
        HIP_CHECK(hipMemcpyAsync(&bad, h->fail.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (ir_out) std::copy(ir.begin(), ir.end(), ir_out);
        return bad ? HIPKKT_NUMERIC_FAILURE : HIPKKT_OK;
    }
    const SpmvDev A = kkt_spmv(h);
    std::vector<double> hn(2 * (size_t)k), norme((size_t)k), normb((size_t)k);
    std::vector<int> active((size_t)k, 1), mask((size_t)k, 0);
    {
        int pr = h->prof.begin(3, h->stream);
        launch_residual(A, h->Kval.p, h->mB.p, h->mX.p, h->mE.p, h->mpartial.p, h->mnorms.p, h->stream, k, ld);
        launch_norm_inf(h->mB.p, N, h->mpartial.p, h->mnorms.p + k, h->stream, k, ld);
        h->prof.end(pr, h->stream);
        HIP_CHECK(hipMemcpyAsync(hn.data(), h->mnorms.p, 2 * (size_t)k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    for (int j = 0; j < k; ++j) {
        norme[j] = hn[j];
        normb[j] = hn[k + j];
        if (!std::isfinite(norme[j])) return HIPKKT_NUMERIC_FAILURE;
    }
    for (int i = 0; i < st.iterative_refinement_max_iter; ++i) {
        bool any = false;
        for (int j = 0; j < k; ++j) {
            if (active[j] && norme[j] <= st.iterative_refinement_abstol + st.iterative_refinement_reltol * normb[j]) active[j] = 0;
            any = any || active[j];
        }
        if (!any) break;
        trisolve(h->mE.p, h->mC.p);                                            // dx_j = K^{-1} e_j
        launch_axpby_sum(h->mC.p, h->mC.p, h->mX.p, (int64_t)N * k, h->stream); // prospective x_j + dx_j
        int pr = h->prof.begin(3, h->stream);
        launch_residual(A, h->Kval.p, h->mB.p, h->mC.p, h->mE2.p, h->mpartial.p, h->mnorms.p, h->stream, k, ld);
        h->prof.end(pr, h->stream);
        HIP_CHECK(hipMemcpyAsync(hn.data(), h->mnorms.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        for (int j = 0; j < k; ++j) {
            mask[j] = 0;
            if (!active[j]) continue;
            ir[j]++;
            h->prof.acc.ir_iterations++;
            if (!std::isfinite(hn[j])) return HIPKKT_NUMERIC_FAILURE;
            const double ratio = norme[j] / hn[j];
            if (ratio < st.iterative_refinement_stop_ratio) {
                if (ratio > 1.0) mask[j] = 1;
                active[j] = 0;
            } else {
                mask[j] = 1;
            }
            if (mask[j]) norme[j] = hn[j];
        }
        HIP_CHECK(hipMemcpyAsync(h->mmask.p, mask.data(), (size_t)k * sizeof(int), hipMemcpyHostToDevice, h->stream));
        launch_accept_columns(h->mX.p, h->mC.p, h->mE.p, h->mE2.p, h->mmask.p, N, k, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));      // `mask` (pageable) must outlive the copy
    }
    h->last_ir = 0;
    for (int j = 0; j < k; ++j) h->last_ir += ir[j];
    if (ir_out) std::copy(ir.begin(), ir.end(), ir_out);
    return HIPKKT_OK;
}

// The same on ROW-major work vectors (N x KP): used when the CSR image has no long rows.  A row of 16 columns is one
// cache line, so the residual's gather of x, the permutations and the accept step all move whole lines.
static int kkt_solve_multi_core_rm(hipkkt_kkt_t h, int k, int KP, int64_t* ir_out)
{
    const hipkkt_settings& st = h->st;
    const int N = (int)h->K.N;
    std::vector<int64_t> ir((size_t)k, 0);
    auto trisolve = [&](const double* rhs, double* out, const double* add = nullptr) {
        int ps = h->prof.begin(2, h->stream);
        h->eng->solve_multi_rm(rhs, out, KP, add);
        h->prof.end(ps, h->stream);
    };
    trisolve(h->mB.p, h->mX.p);
    if (!st.iterative_refinement_enable) {
        int bad = 0;
        launch_zero_ints(h->fail.p, 1, h->stream);
        launch_check_finite(h->mX.p, N * KP, h->fail.p, h->stream);
        HIP_CHECK(hipMemcpyAsync(&bad, h->fail.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (ir_out) std::copy(ir.begin(), ir.end(), ir_out);
        return bad ? HIPKKT_NUMERIC_FAILURE : HIPKKT_OK;
    }
    const SpmvDev A = kkt_spmv(h);
    std::vector<double> hn(2 * (size_t)KP), norme((size_t)k), normb((size_t)k);
    std::vector<int> active((size_t)k, 1), mask((size_t)KP, 0);
    {
        int pr = h->prof.begin(3, h->stream);
        launch_residual_rm(A, h->mB.p, h->mX.p, h->mE.p, h->mpartial.p, h->mnorms.p, h->mnorms.p + KP, KP, h->stream);
        h->prof.end(pr, h->stream);
        HIP_CHECK(hipMemcpyAsync(hn.data(), h->mnorms.p, 2 * (size_t)KP * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    for (int j = 0; j < k; ++j) {
        norme[j] = hn[j];
        normb[j] = hn[KP + j];
        if (!std::isfinite(norme[j])) return HIPKKT_NUMERIC_FAILURE;
    }
    for (int i = 0; i < st.iterative_refinement_max_iter; ++i) {
        bool any = false;
        for (int j = 0; j < k; ++j) {
            if (active[j] && norme[j] <= st.iterative_refinement_abstol + st.iterative_refinement_reltol * normb[j]) active[j] = 0;
            any = any || active[j];
        }
        if (!any) break;
        trisolve(h->mE.p, h->mC.p, h->mX.p);                                      // prospective x_j + dx_j, dx_j = K^{-1} e_j
        int pr = h->prof.begin(3, h->stream);
        launch_residual_rm(A, h->mB.p, h->mC.p, h->mE2.p, h->mpartial.p, h->mnorms.p, nullptr, KP, h->stream);
        h->prof.end(pr, h->stream);
        HIP_CHECK(hipMemcpyAsync(hn.data(), h->mnorms.p, (size_t)KP * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        for (int j = 0; j < k; ++j) {
            mask[j] = 0;
            if (!active[j]) continue;
            ir[j]++;
            h->prof.acc.ir_iterations++;
            if (!std::isfinite(hn[j])) return HIPKKT_NUMERIC_FAILURE;
            const double ratio = norme[j] / hn[j];
            if (ratio < st.iterative_refinement_stop_ratio) {
                if (ratio > 1.0) mask[j] = 1;
                active[j] = 0;
            } else {
                mask[j] = 1;
            }
            if (mask[j]) norme[j] = hn[j];
        }
        bool all_accept = true;
        for (int j = 0; j < k; ++j) all_accept = all_accept && mask[j] != 0;
        if (all_accept) {
            // every column takes its candidate (the usual first round): the buffers change roles, nothing is copied
            // (the padding columns are zero in both)
            std::swap(h->mX.p, h->mC.p);
            std::swap(h->mE.p, h->mE2.p);
            continue;
        }
        HIP_CHECK(hipMemcpyAsync(h->mmask.p, mask.data(), (size_t)KP * sizeof(int), hipMemcpyHostToDevice, h->stream));
        launch_accept_columns_rm(h->mX.p, h->mC.p, h->mE.p, h->mE2.p, h->mmask.p, N, KP, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));      // `mask` (pageable) must outlive the copy
    }
    h->last_ir = 0;
    for (int j = 0; j < k; ++j) h->last_ir += ir[j];
    if (ir_out) std::copy(ir.begin(), ir.end(), ir_out);
    return HIPKKT_OK;
}

static void kkt_multi_unpack(hipkkt_kkt_t h, int k, double* lhsx, double* lhsz, hipMemcpyKind kind)
{
    const size_t n = (size_t)h->K.n, m = (size_t)h->K.m, N = (size_t)h->K.N;
    if (lhsx && n)
        HIP_CHECK(hipMemcpy2DAsync(lhsx, n * sizeof(double), h->mX.p, N * sizeof(double), n * sizeof(double), (size_t)k, kind, h->stream));
    if (lhsz && m)
        HIP_CHECK(hipMemcpy2DAsync(lhsz, m * sizeof(double), h->mX.p + n, N * sizeof(double), m * sizeof(double), (size_t)k, kind, h->stream));
}

// A handful of right-hand sides (2 .. kSmallBatch): the single-column kernels' 2- and 4-column instances, every
// sweep shared by up to four columns -- the tree's dependency chain is paid once per sweep, not once per column (the
// 16-column MFMA path below only pays off from ~a dozen columns on).  Device pointers, column-major, contiguous.
static constexpr int kSmallBatch = 8;
static int kkt_solve_small_batch(hipkkt_kkt_t h, int nrhs, const double* d_rhsx, const double* d_rhsz, double* d_lhsx,
                                 double* d_lhsz, int64_t* ir_iterations, bool may_defer)
{
    const int n = h->K.n, m = h->K.m;
    const size_t N = (size_t)h->K.N;
    const int chunk = h->eng->supports_nr(4) ? 4 : 2;
    kkt_multi_reserve(h, kMaxNR);
    std::swap(h->b.p, h->mB.p);                   // a borrowed right-hand-side buffer: the one set by setrhs! stays as it is
    int rc = HIPKKT_OK;
    int64_t total = 0;
    try {
        for (int j0 = 0; j0 < nrhs && rc == HIPKKT_OK; j0 += chunk) {
            const int k = std::min(chunk, nrhs - j0);
            const int nr = k == 1 ? 1 : (k == 2 ? 2 : 4);
            launch_pack_rhs(h->b.p, d_rhsx + (size_t)j0 * n, d_rhsz + (size_t)j0 * m, n, m, h->K.p, h->stream, k);
            if (k < nr) HIP_CHECK(hipMemsetAsync(h->b.p + (size_t)k * N, 0, (size_t)(nr - k) * N * sizeof(double), h->stream));
            int64_t ir[kMaxNR] = {0, 0, 0, 0};
            rc = kkt_solve_core(h, may_defer, nr, ir);
            if (rc != HIPKKT_OK) break;
            for (int c = 0; c < k; ++c) {
                launch_unpack_lhs(d_lhsx ? d_lhsx + (size_t)(j0 + c) * n : nullptr, d_lhsz ? d_lhsz + (size_t)(j0 + c) * m : nullptr,
                                  h->x.p + (size_t)c * N, n, m, h->stream);
                if (ir_iterations) ir_iterations[j0 + c] = ir[c];
                total += std::max<int64_t>(ir[c], 0);
            }
        }
    } catch (...) { std::swap(h->b.p, h->mB.p); throw; }
    std::swap(h->b.p, h->mB.p);
    h->last_ir = total;
    return rc;
}

int hipkkt_kkt_solve_multi_dev(hipkkt_kkt_t h, int64_t nrhs, const double* d_rhsx, const double* d_rhsz, double* d_lhsx,
                               double* d_lhsz, int64_t* ir_iterations)
{
    return guarded([&]() {
        if (!h || nrhs < 0 || nrhs > 65535 || (nrhs > 0 && ((h->K.n && !d_rhsx) || (h->K.m && !d_rhsz))))
            throw ArgError("hipkkt_kkt_solve_multi_dev: bad argument");
        if (nrhs == 0) return HIPKKT_OK;
        HIP_CHECK(hipSetDevice(h->device));
        if (nrhs == 1) {
            // one column: the single-column path (persistent top kernel, no padding to 16 columns), on a borrowed
            // right-hand-side buffer so that the one set by hipkkt_kkt_setrhs stays as it is
            kkt_multi_reserve(h, 1);
            std::swap(h->b.p, h->mB.p);
            launch_pack_rhs(h->b.p, d_rhsx, d_rhsz, h->K.n, h->K.m, h->K.p, h->stream);
            int rc;
            try { rc = kkt_solve_core(h, true); } catch (...) { std::swap(h->b.p, h->mB.p); throw; }
            std::swap(h->b.p, h->mB.p);
            if (ir_iterations) ir_iterations[0] = h->last_ir;      // (-1 in deferred-status mode, as for 2..8 columns)
            if (rc != HIPKKT_OK) return rc;
            launch_unpack_lhs(d_lhsx, d_lhsz, h->cur_x, h->K.n, h->K.m, h->stream);
            return HIPKKT_OK;
        }
        if (nrhs <= kSmallBatch && h->eng->supports_nr(2))
            return kkt_solve_small_batch(h, (int)nrhs, d_rhsx, d_rhsz, d_lhsx, d_lhsz, ir_iterations, true);
        kkt_multi_reserve(h, (size_t)nrhs);
        if (h->nlong == 0) {
            const int KP = ((int)nrhs + 15) & ~15;
            launch_pack_rhs_rm(h->mB.p, d_rhsx, d_rhsz, h->K.n, h->K.m, h->K.p, (int)nrhs, KP, h->stream);
            int rc = kkt_solve_multi_core_rm(h, (int)nrhs, KP, ir_iterations);
            if (rc != HIPKKT_OK) return rc;
            launch_unpack_lhs_rm(d_lhsx, d_lhsz, h->mX.p, h->K.n, h->K.m, (int)nrhs, KP, h->stream);
            return HIPKKT_OK;
        }
        launch_pack_rhs(h->mB.p, d_rhsx, d_rhsz, h->K.n, h->K.m, h->K.p, h->stream, (int)nrhs);
        int rc = kkt_solve_multi_core(h, (int)nrhs, ir_iterations);
        if (rc != HIPKKT_OK) return rc;
        kkt_multi_unpack(h, (int)nrhs, d_lhsx, d_lhsz, hipMemcpyDeviceToDevice);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_solve_multi(hipkkt_kkt_t h, int64_t nrhs, const double* rhsx, const double* rhsz, double* lhsx,
                           double* lhsz, int64_t* ir_iterations)
{
    return guarded([&]() {
        if (!h || nrhs < 0 || nrhs > 65535 || (nrhs > 0 && ((h->K.n && !rhsx) || (h->K.m && !rhsz))))
            throw ArgError("hipkkt_kkt_solve_multi: bad argument");
        if (nrhs == 0) return HIPKKT_OK;
        HIP_CHECK(hipSetDevice(h->device));
        kkt_multi_reserve(h, (size_t)nrhs);
        const size_t n = (size_t)h->K.n, m = (size_t)h->K.m, k = (size_t)nrhs;
        // stage [rhsx | rhsz] in the candidate buffer (N k >= (n + m) k doubles, not needed before the first round)
        double* sx = h->mC.p;
        double* sz = h->mC.p + n * k;
        if (n) HIP_CHECK(hipMemcpyAsync(sx, rhsx, n * k * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (m) HIP_CHECK(hipMemcpyAsync(sz, rhsz, m * k * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (nrhs >= 2 && nrhs <= kSmallBatch && h->eng->supports_nr(2)) {
            // staged in the candidate buffer of the many-column path (unused by this one); solutions come back through it too
            double* ox = h->mE.p;
            double* oz = h->mE.p + n * k;
            int rc = kkt_solve_small_batch(h, (int)nrhs, sx, sz, lhsx ? ox : nullptr, lhsz ? oz : nullptr, ir_iterations, false);
            if (rc != HIPKKT_OK) return rc;
            if (lhsx && n) HIP_CHECK(hipMemcpyAsync(lhsx, ox, n * k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            if (lhsz && m) HIP_CHECK(hipMemcpyAsync(lhsz, oz, m * k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipStreamSynchronize(h->stream));
            return HIPKKT_OK;
        }
        if (h->nlong == 0) {
            const int KP = ((int)nrhs + 15) & ~15;
            launch_pack_rhs_rm(h->mB.p, sx, sz, h->K.n, h->K.m, h->K.p, (int)nrhs, KP, h->stream);
            int rc = kkt_solve_multi_core_rm(h, (int)nrhs, KP, ir_iterations);
            if (rc != HIPKKT_OK) return rc;
            // column-major staging in the candidate buffer again, then to the host
            double* ox = h->mC.p;
            double* oz = h->mC.p + n * k;
            launch_unpack_lhs_rm(lhsx ? ox : nullptr, lhsz ? oz : nullptr, h->mX.p, h->K.n, h->K.m, (int)nrhs, KP, h->stream);
            if (lhsx && n) HIP_CHECK(hipMemcpyAsync(lhsx, ox, n * k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            if (lhsz && m) HIP_CHECK(hipMemcpyAsync(lhsz, oz, m * k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipStreamSynchronize(h->stream));
            return HIPKKT_OK;
        }
        launch_pack_rhs(h->mB.p, sx, sz, h->K.n, h->K.m, h->K.p, h->stream, (int)nrhs);
        int rc = kkt_solve_multi_core(h, (int)nrhs, ir_iterations);
        if (rc != HIPKKT_OK) return rc;
        kkt_multi_unpack(h, (int)nrhs, lhsx, lhsz, hipMemcpyDeviceToHost);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

// ------------------------------------------------------------------------------------------------
//  Level C: the reduced-system layer (DefaultKKTSystem, /root/reference/src/kktsystem.jl:21-215) with every
//  vector resident in HBM -- right-hand-side construction and the recovery of (dtau, dx, dz, ds, dkappa)
//  around the solves run on the device, so nothing but two scalars per solve crosses PCIe.
// ------------------------------------------------------------------------------------------------
static SpmvDev sys_spmv(hipkkt_kkt_t h) { return kkt_spmv(h); }

int hipkkt_kkt_system_init(hipkkt_kkt_t h, const double* q, const double* b)
{
    return guarded([&]() {
        if (!h || (h->K.n && !q) || (h->K.m && !b)) throw ArgError("hipkkt_kkt_system_init: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        const size_t n = (size_t)h->K.n, m = (size_t)h->K.m;
        h->sq.alloc(n); h->snegq.alloc(n); h->sb.alloc(m);
        h->sx2.alloc(n); h->sworkx.alloc(n); h->spa.alloc(n); h->spb.alloc(n); h->spc.alloc(n);
        h->sz2.alloc(m); h->sworkz.alloc(m); h->sconic.alloc(m);
        h->sys_partial.alloc(8 * 64); h->sys_dots.alloc(8); h->sys_cached.alloc(4); h->sys_in.alloc(4); 
        if (n) HIP_CHECK(hipMemcpyAsync(h->sq.p, q, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (m) HIP_CHECK(hipMemcpyAsync(h->sb.p, b, m * sizeof(double), hipMemcpyHostToDevice, h->stream));
        launch_neg_copy(h->snegq.p, h->sq.p, (int)n, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->sys_ready = true;
        return HIPKKT_OK;
    });
}

// setrhs! + solve! with device vectors; either output may be null
static int sys_solve_into(hipkkt_kkt_t h, const double* rx, const double* rz, double* outx, double* outz)
{
    launch_pack_rhs(h->b.p, rx, rz, h->K.n, h->K.m, h->K.p, h->stream);
    int rc = kkt_solve_core(h);
    if (rc != HIPKKT_OK) return rc;
    launch_unpack_lhs(outx, outz, h->cur_x, h->K.n, h->K.m, h->stream);
    return HIPKKT_OK;
}

static void sys_cache_constant_terms(hipkkt_kkt_t h);
// data updates (hipkkt_kkt_system_update_data_*) leave the factorisation (P, A) and (x2, z2) with its cached terms (all
// four) stale until the next kkt_update! / constant-RHS solve; a call that would read either is refused before it
// enqueues anything
static void data_refuse_stale_factor(hipkkt_kkt_t h, const char* what)
{
    if (h->data_factor_stale)
        throw ArgError(std::string("hipkkt_kkt_system_*: ") + what + " would read a factorisation that is stale since "
                       "hipkkt_kkt_system_update_data_P / _A: call hipkkt_kkt_system_update first");
}
static void data_refuse_stale_solve(hipkkt_kkt_t h)
{
    data_refuse_stale_factor(h, "the solve");
    if (h->data_const_stale && !h->sys_const_pending)
        throw ArgError("hipkkt_kkt_system_*: the solve would read (x2, z2) that is stale since a hipkkt_kkt_system_update_data_* "
                       "call: call hipkkt_kkt_system_update (or _solve_constant_rhs) first");
}
static int sys_flush_update_status(hipkkt_kkt_t h);
static int sys_flush_startup(hipkkt_kkt_t h);
static int sys_constant_rhs(hipkkt_kkt_t h)
{
    // _kkt_solve_constant_rhs! (kktsystem.jl:80-92): (x2, z2) = K \ (-q, b)
    data_refuse_stale_factor(h, "the constant-RHS solve");
    int rc = sys_solve_into(h, h->snegq.p, h->sb.p, h->sx2.p, h->sz2.p);
    if (rc != HIPKKT_OK) return rc;
    sys_cache_constant_terms(h);
    h->data_const_stale = false;
    return HIPKKT_OK;
}

int hipkkt_kkt_system_solve_constant_rhs(hipkkt_kkt_t h)
{
    return guarded([&]() {
        if (!h || !h->sys_ready) throw ArgError("hipkkt_kkt_system_*: call hipkkt_kkt_system_init first");
        data_refuse_stale_factor(h, "the constant-RHS solve");
        HIP_CHECK(hipSetDevice(h->device));
        h->sys_const_pending = false;
        const int rc = sys_flush_update_status(h);      // (an enqueued-only kkt_update! before it: its status is due here)
        if (rc != HIPKKT_OK) return rc;
        return sys_constant_rhs(h);
    });
}

int hipkkt_kkt_system_set_lazy(hipkkt_kkt_t h, int lazy)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        if (!lazy && h->sys_const_pending) {           // leaving the mode with a solve still due: run it now
            if (!h->sys_ready) throw ArgError("hipkkt_kkt_system_*: call hipkkt_kkt_system_init first");
            HIP_CHECK(hipSetDevice(h->device));
            h->sys_const_pending = false;
            h->sys_lazy = false;
            const int rc = sys_flush_update_status(h);
            if (rc != HIPKKT_OK) return rc;
            return sys_constant_rhs(h);
        }
        if (!lazy && h->sys_ready) {                   // (an enqueued-only update's record does not outlive the mode)
            HIP_CHECK(hipSetDevice(h->device));
            const int rc = sys_flush_update_status(h);
            if (rc != HIPKKT_OK) { h->sys_lazy = false; return rc; }
        }
        h->sys_lazy = lazy != 0;
        return HIPKKT_OK;
    });
}

// the constant-RHS part of kkt_update! (kktsystem.jl:74-77): at once, or noted for the affine kkt_solve! (lazy mode)
static int sys_after_update(hipkkt_kkt_t h)
{
    if (!h->sys_ready) throw ArgError("hipkkt_kkt_system_*: call hipkkt_kkt_system_init first");
    if (h->deferred) throw ArgError("hipkkt_kkt_system_*: level C reads its scalars back (deferred status is for level B)");
    if (h->sys_lazy) { h->sys_const_pending = true; return HIPKKT_OK; }
    h->sys_const_pending = false;
    return sys_constant_rhs(h);
}

int hipkkt_kkt_system_update(hipkkt_kkt_t h, const double* d_s, const double* d_z)
{
    // kkt_update! (kktsystem.jl:62-78)
    if (h && h->deferred) {
        g_last_error = "hipkkt_kkt_system_*: level C reads its scalars back (deferred status is for level B)";
        return HIPKKT_ERR_ARG;         // (before anything is enqueued: a deferred factorisation's status would be left unread)
    }
    // Lazy mode: the update is only ENQUEUED (its status -- cone points, pivots, the overlap mode's waits -- joins the
    // sticky record on the device) and is read back together with the affine kkt_solve!'s own result: one host round
    // trip for kkt_update! + kkt_solve!(:affine) instead of three.  A failed factorisation therefore surfaces at the
    // affine kkt_solve! -- `is_kkt_solve_success = kkt_update!(...)` and `is_kkt_solve_success && kkt_solve!(...)`
    // (solver.jl:279-295) reach the same branch either way.
    // (not under hipkkt_kkt_system_set_member_status: a failed update is answered member by member before the solve, so it
    //  is read back at once, as member refinement keeps the lazy pairing's solves apart)
    const bool enqueue_only = h && h->sys_lazy && h->sys_ready && !h->member_status_on();
    int rc = kkt_update_from_sz_dev_impl(h, d_s, d_z, enqueue_only);
    if (rc != HIPKKT_OK) return rc;                    // "bail if the factorization has failed" (:71)
    if (enqueue_only) h->sys_update_unread = true;
    return guarded([&]() { return sys_after_update(h); });
}

int hipkkt_kkt_system_solve_initial_point(hipkkt_kkt_t h, double* d_x, double* d_s, double* d_z)
{
    return guarded([&]() {
        if (!h || !h->sys_ready) throw ArgError("hipkkt_kkt_system_*: call hipkkt_kkt_system_init first");
        if ((h->K.n && !d_x) || (h->K.m && (!d_s || !d_z))) throw ArgError("hipkkt_kkt_system_solve_initial_point: bad argument");
        data_refuse_stale_factor(h, "the initial-point solve");
        HIP_CHECK(hipSetDevice(h->device));
        const int n = h->K.n, m = h->K.m;
        int rc = sys_flush_startup(h);
        if (rc != HIPKKT_OK) return rc;
        if (h->mapP.n == 0) {
            // LP initialisation (kktsystem.jl:107-128): [0; b] -> (x, -s), then [-q; 0] -> z
            if (n) HIP_CHECK(hipMemsetAsync(h->sworkx.p, 0, (size_t)n * sizeof(double), h->stream));
            rc = sys_solve_into(h, h->sworkx.p, h->sb.p, d_x, h->sworkz.p);
            if (rc != HIPKKT_OK) return rc;
            launch_neg_copy(d_s, h->sworkz.p, m, h->stream);
            if (m) HIP_CHECK(hipMemsetAsync(h->sworkz.p, 0, (size_t)m * sizeof(double), h->stream));
            rc = sys_solve_into(h, h->snegq.p, h->sworkz.p, nullptr, d_z);
            if (rc != HIPKKT_OK) return rc;
        } else {
            // QP initialisation (:129-137): [-q; b] -> (x, z), s = -z
            rc = sys_solve_into(h, h->snegq.p, h->sb.p, d_x, d_z);
            if (rc != HIPKKT_OK) return rc;
            launch_neg_copy(d_s, d_z, m, h->stream);
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

// the part of kkt_solve! behind the solve for (x1, z1) (kktsystem.jl:175-212): dtau, (dx, dz), ds, dkappa
// with_const: (x2, z2) is new as well (it came out of the same 2-column solve): its terms of tau_den are formed here too
// addend: Delta_s constant term (sconic, or variables.s itself for the affine step)
// (x1, z1): the solve's solution where the sweeps left it (h->x: no copy); it is consumed before the next solve
static void sys_finish_step(hipkkt_kkt_t h, const double* x1, const double* z1, double* d_lhs_x, double* d_lhs_s, double* d_lhs_z,
                            double* lhs_tau_kappa, double rhs_tau, double rhs_kappa, const double* d_var_x, double var_tau,
                            double var_kappa, bool with_const = false, const double* addend = nullptr, const Publish& pub = Publish{})
{
    const int n = h->K.n, m = h->K.m;
    hipStream_t st = h->stream;
    // (x2, z2): the handle's copy -- or, fresh out of this call's 2-column solve, column 0 where the sweeps left it; the copy
    // that the iteration's later solves read is then written by the step kernel on its way
    const double* x2 = with_const ? h->x.p : h->sx2.p;
    const double* z2 = with_const ? h->x.p + n : h->sz2.p;
    // P x1 and P (xi - x2), xi = x / tau, in one pass (xi - x2 kept in workx for its dot product)
    launch_P_spmv2(sys_spmv(h), h->Kval.p, x1, d_var_x, x2, var_tau, h->spa.p, h->spb.p, h->sworkx.p,
                   with_const ? h->spc.p : nullptr, n, st);
    DotPairs P{};
    P.npairs = with_const ? 7 : 4;
    if (with_const) {
        P.a[4] = h->sq.p; P.b[4] = x2; P.len[4] = n;
        P.a[5] = h->sb.p; P.b[5] = z2; P.len[5] = m;
        P.a[6] = x2; P.b[6] = h->spc.p; P.len[6] = n;
    }
    P.a[0] = h->sq.p; P.b[0] = x1; P.len[0] = n;
    P.a[1] = h->sb.p; P.b[1] = z1; P.len[1] = m;
    P.a[2] = d_var_x; P.b[2] = h->spa.p; P.len[2] = n;
    P.a[3] = h->sworkx.p; P.b[3] = h->spb.p; P.len[3] = n;
    // ... the scalars (:185-196, :206) and (dx, dz) = (x1, z1) + dtau (x2, z2)   (:200-203)
    launch_dots_sys_step(P, h->sys_partial.p, h->sys_cached.p, rhs_tau, rhs_kappa, var_tau, var_kappa, h->sys_out_dev, d_lhs_x, d_lhs_z,
                         x1, z1, x2, z2, n, m, st, with_const ? h->sx2.p : nullptr, with_const ? h->sz2.p : nullptr);
    // ds = -(Hs dz + const)                                               (:206-212)
    launch_mul_Hs(h->cone_dev(), h->cone_state(), d_lhs_s, d_lhs_z, m, st, addend ? addend : h->sconic.p, pub);
    if (!lhs_tau_kappa) return;                      // (the caller reads sys_out back with its own status record)
    // (dtau, dkappa) through the handle's pinned block: a copy into pageable memory would be staged
    HIP_CHECK(hipMemcpyAsync(h->pin->h + 48, h->sys_out_dev, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    lhs_tau_kappa[0] = h->pin->h[48];
    lhs_tau_kappa[1] = h->pin->h[49];
}
// an enqueued-only kkt_update! whose status nobody has read yet (lazy mode), before a call that reads back on its own
static int sys_flush_update_status(hipkkt_kkt_t h)
{
    if (!h->sys_update_unread) return HIPKKT_OK;
    h->sys_update_unread = false;
    HIP_CHECK(hipMemcpyAsync(h->pin->h + 40, h->ir_sticky, 8 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    launch_zero_ints((int*)h->ir_sticky, 16, h->stream);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    bool gave_up = false;
    int rc = kkt_eval_sticky(h, h->pin->h + 40, &gave_up);
    if (rc == HIPKKT_REFINEMENT_INCOMPLETE) rc = gave_up ? kkt_update_device(h) : HIPKKT_OK;   // a bounded wait gave up: level by level, synchronously
    return rc;
}
// ... before the calls of the start-up sequence (solver.jl:389-393: kkt_update!, then kkt_solve_initial_point!, the
// update's Bool ignored): the record is read so that a give-up is repaired and no stale word reaches the first
// iteration; a numeric failure of that update is the reference's to ignore -- the solve that follows reports its own
static int sys_flush_startup(hipkkt_kkt_t h)
{
    const int rc = sys_flush_update_status(h);
    return rc == HIPKKT_NUMERIC_FAILURE ? HIPKKT_OK : rc;
}
// the x2-only terms of tau_den (kktsystem.jl:194-196) are the same for both solves of the iteration
static void sys_cache_constant_terms(hipkkt_kkt_t h)
{
    launch_P_spmv(sys_spmv(h), h->Kval.p, h->sx2.p, h->spa.p, h->K.n, h->stream);
    DotPairs P{};
    P.npairs = 3;
    P.a[0] = h->sq.p; P.b[0] = h->sx2.p; P.len[0] = h->K.n;
    P.a[1] = h->sb.p; P.b[1] = h->sz2.p; P.len[1] = h->K.m;
    P.a[2] = h->sx2.p; P.b[2] = h->spa.p; P.len[2] = h->K.n;
    launch_dots(P, h->sys_partial.p, h->sys_cached.p, h->stream);
}

// kkt_solve! (kktsystem.jl:145-215).  With the constant-RHS solve of the preceding kkt_update! still due (lazy mode)
// an affine step sends both right-hand sides through the sweeps together.
static int sys_solve_step(hipkkt_kkt_t h, double* d_lhs_x, double* d_lhs_s, double* d_lhs_z, double* lhs_tau_kappa,
                          const double* d_rhs_x, const double* d_rhs_s, const double* d_rhs_z, double rhs_tau,
                          double rhs_kappa, const double* d_var_x, const double* d_var_s, const double* d_var_z,
                          double var_tau, double var_kappa, int steptype)
{
    if (!h->sys_ready) throw ArgError("hipkkt_kkt_system_*: call hipkkt_kkt_system_init first");
    const int n = h->K.n, m = h->K.m;
    const bool affine = steptype == 0;
    // (the affine step does not read rhs.s: kktsystem.jl:157-158)
    if ((n && (!d_lhs_x || !d_rhs_x || !d_var_x)) || (m && (!d_lhs_s || !d_lhs_z || !d_rhs_z || !d_var_s || !d_var_z)) ||
        (m && !affine && !d_rhs_s) || !lhs_tau_kappa || (steptype != 0 && steptype != 1))
        throw ArgError("hipkkt_kkt_system_solve: bad argument");
    if (!h->scaling_valid) throw ArgError("hipkkt_kkt_system_solve: needs the cone scaling of hipkkt_kkt_system_update");
    if (h->deferred) throw ArgError("hipkkt_kkt_system_*: level C reads its scalars back (deferred status is for level B)");
    data_refuse_stale_solve(h);
    HIP_CHECK(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    // (under the member refinement rule the pairing is not taken: the rule covers single-column solves)
    const bool pair = h->sys_const_pending && affine && h->eng->supports_nr(2) && !h->mr_on;
    if (h->sys_const_pending && !pair) {
        // (x2, z2) is due and cannot ride with this solve: by itself first, as kkt_update! would have done it
        h->sys_const_pending = false;
        int rc = sys_flush_update_status(h);
        if (rc == HIPKKT_OK) rc = sys_constant_rhs(h);
        if (rc != HIPKKT_OK) return rc;
    }
    h->sys_const_pending = false;
    const size_t N = (size_t)h->K.N;
    // everything of this call, enqueued; `defer`: the solve's refinement decisions stay on the device, nothing is read back here
    auto run = [&](bool defer) -> int {
        // Delta_s constant term and the z part of the right-hand side (kktsystem.jl:150-166).  Affine step: the constant
        // term is variables.s itself (:157-158), so the right-hand side is packed straight from (rhs.x, s - rhs.z)
        if (!affine && !launch_sys_offset(h->cone_dev(), h->cone_state(), h->sconic.p, h->sworkz.p, d_rhs_s, d_var_z, d_rhs_z,
                                          m, false, st))
            throw ArgError("hipkkt_kkt_system_solve: unsupported cone kind");
        if (pair) {
            // _kkt_solve_constant_rhs! (:80-92) and this solve (:170-173) as ONE 2-column solve: column 0 = (-q, b),
            // column 1 = (rhs.x, s - rhs.z); each column is refined by the reference's rule on its own
            launch_pack_rhs_affine(h->b.p, h->snegq.p, h->sb.p, d_rhs_x, d_var_s, d_rhs_z, n, m, h->K.p, 2, st);
            int rc = kkt_solve_core(h, false, 2, nullptr, defer);
            if (rc != HIPKKT_OK) return rc;
            h->data_const_stale = false;
            // ((x2, z2) = column 0 outlives this solve: sys_finish_step copies it on its way)
        } else {
            // (x1, z1) = K \ (rhs.x, const - rhs.z)                              (:170-173)
            if (affine) launch_pack_rhs_affine(h->b.p, nullptr, nullptr, d_rhs_x, d_var_s, d_rhs_z, n, m, h->K.p, 1, st);
            else launch_pack_rhs(h->b.p, d_rhs_x, h->sworkz.p, n, m, h->K.p, st);
            int rc = kkt_solve_core(h, false, 1, nullptr, defer);
            if (rc != HIPKKT_OK) return rc;
        }
        const double* x1 = h->x.p + (pair ? N : 0);
        // (deferred: the status record and (dtau, dkappa) behind it reach the host with the call's last kernel)
        sys_finish_step(h, x1, x1 + n, d_lhs_x, d_lhs_s, d_lhs_z, defer ? nullptr : lhs_tau_kappa, rhs_tau, rhs_kappa, d_var_x, var_tau, var_kappa,
                        pair, affine ? d_var_s : nullptr,
                        (defer && h->publish_ok) ? Publish{h->pin->h + 40, h->ir_sticky, 10, 8, (double)++h->publish_seq} : Publish{});
        return HIPKKT_OK;
    };
    if (h->sys_lazy && h->st.iterative_refinement_enable && !h->mr_on) {
        // Lazy mode: ONE read-back per call -- the sticky status record (this call's solve, and the kkt_update! before it
        // if that was enqueued only) together with (dtau, dkappa).  If the record says that the reference's refinement loop
        // would have gone on, or that a bounded wait gave up, the call is repeated with the synchronous sequence.
        const bool update_unread = h->sys_update_unread;
        h->sys_update_unread = false;
        int rc = run(true);
        if (rc != HIPKKT_OK) return rc;
        if (h->publish_ok) {
            HIP_CHECK(hipStreamSynchronize(st));       // (pin->h[40..49]: the record, then dtau, dkappa -- published by run's last kernel)
            if (h->pin->h[50] != (double)h->publish_seq || knobs().test_publish_fail) {
                // The device's stores to the page-locked block did not arrive (never seen; a mapping this code has not been
                // run on): the record -- zeroed on the device by the kernel that published it -- is lost for this call, so
                // the call is repeated with the synchronous sequence, its update included; copies from now on.
                h->publish_ok = false;
                if (knobs().verbose) std::fprintf(stderr, "[hipkkt] status record not published to host memory: copying it from now on\n");
                if (update_unread) {
                    rc = kkt_update_device(h);
                    if (rc != HIPKKT_OK) return rc;
                }
                return run(false);
            }
        } else {
            HIP_CHECK(hipMemcpyAsync(h->pin->h + 40, h->ir_sticky, 10 * sizeof(double), hipMemcpyDeviceToHost, st));   // (the record, then dtau, dkappa)
            launch_zero_ints((int*)h->ir_sticky, 16, st);
            HIP_CHECK(hipStreamSynchronize(st));
        }
        bool gave_up = false;
        rc = kkt_eval_sticky(h, h->pin->h + 40, &gave_up, true);
        h->last_ir = (int64_t)h->pin->h[43];           // this call's refinement rounds, summed over its columns (as the synchronous path reports)
        if (rc == HIPKKT_OK) {
            lhs_tau_kappa[0] = h->pin->h[48];
            lhs_tau_kappa[1] = h->pin->h[49];
            return HIPKKT_OK;
        }
        if (rc != HIPKKT_REFINEMENT_INCOMPLETE) return rc;
        if (update_unread && gave_up) {                // (the factorisation itself may be void: a wait of the overlap mode gave up;
            rc = kkt_update_device(h);                 //  a solve that merely wanted another refinement round keeps its factor)
            if (rc != HIPKKT_OK) return rc;
        }
    } else {
        int rc = sys_flush_update_status(h);
        if (rc != HIPKKT_OK) return rc;
    }
    return run(false);
}

int hipkkt_kkt_system_solve(hipkkt_kkt_t h, double* d_lhs_x, double* d_lhs_s, double* d_lhs_z, double* lhs_tau_kappa,
                            const double* d_rhs_x, const double* d_rhs_s, const double* d_rhs_z, double rhs_tau,
                            double rhs_kappa, const double* d_var_x, const double* d_var_s, const double* d_var_z,
                            double var_tau, double var_kappa, int steptype)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        return sys_solve_step(h, d_lhs_x, d_lhs_s, d_lhs_z, lhs_tau_kappa, d_rhs_x, d_rhs_s, d_rhs_z, rhs_tau, rhs_kappa,
                              d_var_x, d_var_s, d_var_z, var_tau, var_kappa, steptype);
    });
}

// ---- the cone operations between the solves (step_kernels.hip): affine_ds!, the combined step's d.s, step_length,
// _shift_to_cone_interior! on the caller's device vectors
// the family of an entry point: what its name promises to cover (the symmetric four, the _ns five, the _gp five)
enum class StepFamily { Symmetric, Nonsym, Genpow };

static void step_guard(hipkkt_kkt_t h, const char* who, StepFamily fam, bool need_scaling)
{
    if (!h) throw ArgError("null handle");
    if (!h->sys_ready) throw ArgError("hipkkt_kkt_system_*: call hipkkt_kkt_system_init first");
    if (h->deferred) throw ArgError("hipkkt_kkt_system_*: level C reads its scalars back (deferred status is for level B)");
    if (fam == StepFamily::Nonsym && h->K.ngenpow > 0)
        throw ArgError(std::string(who) + ": generalized power cones are not covered (the _gp entry points are)");
    if (fam == StepFamily::Symmetric && (h->K.nnonsym > 0 || h->K.ngenpow > 0))
        throw ArgError(std::string(who) + ": symmetric cones only (the handle holds an exponential, power or generalized power cone)");
    if (h->psd_too_big && !h->large_psd) throw ArgError(std::string(who) + ": PSD cones with side > 48 are not covered");
    if (h->psdb_kmax > kPsdBigMaxDim) throw ArgError(std::string(who) + ": PSD cones with side > 96 are not covered");
    if (need_scaling && !h->scaling_valid)
        throw ArgError(std::string(who) + ": needs the cone scaling of hipkkt_kkt_system_update");
    HIP_CHECK(hipSetDevice(h->device));
    ConeDev Call = h->cone_dev();
    Call.npsdb = h->npsdb;                            // (sized for the big PSD class whether or not it is enabled now)
    if (!h->step_partial.p) h->step_partial.alloc((size_t)2 * step_partials(Call));
    if (!h->step_rec.p) h->step_rec.alloc(12);        // (shared with hipkkt_kkt_system_residuals' twelve scalars)
    if (fam != StepFamily::Symmetric && !h->ns_partial.p) h->ns_partial.alloc((size_t)2 * barrier_partials(Call));
}

// the record of a finishing kernel (nrec doubles) on the host: published by that kernel into the pinned block and
// sequence-checked, or -- where such stores do not arrive -- copied
static const double* step_read_record(hipkkt_kkt_t h, int nrec, const std::function<void(const Publish&)>& enqueue)
{
    double* dst = h->pin->h + 52;                     // [52 .. 52 + nrec) the record, then the sequence number
    if (h->publish_ok) {
        enqueue(Publish{dst, h->step_rec.p, nrec, 0, (double)++h->publish_seq});
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (dst[nrec] == (double)h->publish_seq && !knobs().test_publish_fail) return dst;
        h->publish_ok = false;                        // (the record itself is still on the device: nothing is repeated)
        if (knobs().verbose) std::fprintf(stderr, "[hipkkt] status record not published to host memory: copying it from now on\n");
    } else {
        enqueue(Publish{});
    }
    HIP_CHECK(hipMemcpyAsync(dst, h->step_rec.p, (size_t)nrec * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    return dst;
}

int hipkkt_kkt_system_affine_ds(hipkkt_kkt_t h, double* d_out)
{
    return guarded([&]() {
        step_guard(h, "hipkkt_kkt_system_affine_ds", StepFamily::Symmetric, true);
        if (h->K.m && !d_out) throw ArgError("hipkkt_kkt_system_affine_ds: bad argument");
        launch_step_ds(h->cone_dev(), h->cone_state(), d_out, nullptr, nullptr, 0.0, 0.0, h->K.m, false, h->stream);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_combined_ds(hipkkt_kkt_t h, double* d_out, const double* d_step_z, const double* d_step_s,
                                  double sigma_mu, double m_corr)
{
    return guarded([&]() {
        step_guard(h, "hipkkt_kkt_system_combined_ds", StepFamily::Symmetric, true);
        if (h->K.m && (!d_out || !d_step_z || !d_step_s || d_out == d_step_z || d_out == d_step_s))
            throw ArgError("hipkkt_kkt_system_combined_ds: bad argument (d_out must not alias an input)");
        launch_step_ds(h->cone_dev(), h->cone_state(), d_out, d_step_z, d_step_s, sigma_mu, m_corr, h->K.m, true, h->stream);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_step_length(hipkkt_kkt_t h, const double* d_step_z, const double* d_step_s, const double* d_z,
                                  const double* d_s, double step_tau, double step_kappa, double tau, double kappa,
                                  double* alpha_out)
{
    return guarded([&]() {
        step_guard(h, "hipkkt_kkt_system_step_length", StepFamily::Symmetric, true);
        if ((h->K.m && (!d_step_z || !d_step_s || !d_z || !d_s)) || !alpha_out)
            throw ArgError("hipkkt_kkt_system_step_length: bad argument");
        const double* rec = step_read_record(h, 1, [&](const Publish& pub) {
            launch_step_length(h->cone_dev(), h->cone_state(), d_step_z, d_step_s, d_z, d_s, step_tau, step_kappa, tau, kappa,
                               h->step_partial.p, h->step_rec.p, pub, h->K.m, h->stream);
        });
        *alpha_out = rec[0];
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_shift_to_interior(hipkkt_kkt_t h, double* d_v, int primal, double* margins_out)
{
    return guarded([&]() {
        step_guard(h, "hipkkt_kkt_system_shift_to_interior", StepFamily::Symmetric, false);
        if ((h->K.m && !d_v) || (primal != 0 && primal != 1)) throw ArgError("hipkkt_kkt_system_shift_to_interior: bad argument");
        const ConeDev C = h->cone_dev();
        const double* rec = step_read_record(h, 2, [&](const Publish& pub) {
            launch_margins(C, d_v, h->step_partial.p, h->step_rec.p, pub, h->K.m, h->stream);
        });
        const double min_margin = rec[0], pos_margin = rec[1];
        if (margins_out) { margins_out[0] = min_margin; margins_out[1] = pos_margin; }
        double degree = 0.0;                          // degree(cones): nonnegative n, second-order 1, PSD its side
        for (const ConeInfo& ci : h->K.cones)
            degree += ci.kind == HIPKKT_CONE_NN ? ci.numel : ci.kind == HIPKKT_CONE_SOC ? 1 : ci.kind == HIPKKT_CONE_PSD ? ci.dim : 0;
        const double target = degree > 0.0 ? std::max(1.0, 0.1 * pos_margin / degree) : 1.0;
        // variables.jl:186-204
        if (min_margin <= 0.0) launch_unit_shift(C, d_v, -min_margin, target, true, primal == 1, h->K.m, h->stream);
        else if (min_margin < target) launch_unit_shift(C, d_v, target - min_margin, 0.0, false, primal == 1, h->K.m, h->stream);
        else launch_unit_shift(C, d_v, 0.0, 0.0, false, primal == 1, h->K.m, h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

// ---- the same for cone lists that hold exponential / power cones (the _ns entry points) and generalized power cones as
// well (the _gp ones, coneops_genpowcone.jl), and the two operations only such lists need (the unit start and the barrier
// of the dual-scaling line search).  Entry points of their own: each family keeps refusing what its name does not cover.
// One body per operation: the family decides what step_guard refuses, the handle's cone list which kernels run.
static int step_unit_initialization(hipkkt_kkt_t h, StepFamily fam, const char* who, double* d_s, double* d_z)
{
    return guarded([&]() {
        step_guard(h, who, fam, false);
        if (h->K.m && (!d_s || !d_z || d_s == d_z)) throw ArgError(std::string(who) + ": bad argument");
        launch_unit_initialization(h->cone_dev(), h->cone_state(), d_s, d_z, h->K.m, h->stream);
        return HIPKKT_OK;
    });
}

static int step_affine_ds(hipkkt_kkt_t h, StepFamily fam, const char* who, double* d_out, const double* d_s)
{
    return guarded([&]() {
        step_guard(h, who, fam, true);
        if (h->K.m && (!d_out || !d_s || d_out == d_s))
            throw ArgError(std::string(who) + ": bad argument (d_out must not alias an input)");
        launch_step_ds_ns(h->cone_dev(), h->cone_state(), d_out, nullptr, nullptr, d_s, nullptr, 0.0, 0.0, h->K.m, false, h->stream);
        return HIPKKT_OK;
    });
}

static int step_combined_ds(hipkkt_kkt_t h, StepFamily fam, const char* who, double* d_out, const double* d_step_z,
                            const double* d_step_s, const double* d_s, const double* d_z, double sigma_mu, double m_corr)
{
    return guarded([&]() {
        step_guard(h, who, fam, true);
        if (h->K.m && (!d_out || !d_step_z || !d_step_s || !d_s || !d_z || d_out == d_step_z || d_out == d_step_s || d_out == d_s ||
                       d_out == d_z))
            throw ArgError(std::string(who) + ": bad argument (d_out must not alias an input)");
        launch_step_ds_ns(h->cone_dev(), h->cone_state(), d_out, d_step_z, d_step_s, d_s, d_z, sigma_mu, m_corr, h->K.m, true,
                          h->stream);
        return HIPKKT_OK;
    });
}

static int step_length_backtrack(hipkkt_kkt_t h, StepFamily fam, const char* who, const double* d_step_z, const double* d_step_s,
                                 const double* d_z, const double* d_s, double step_tau, double step_kappa, double tau, double kappa,
                                 double backtrack_step, double alpha_min, double* alpha_out)
{
    return guarded([&]() {
        step_guard(h, who, fam, true);
        if ((h->K.m && (!d_step_z || !d_step_s || !d_z || !d_s)) || !alpha_out) throw ArgError(std::string(who) + ": bad argument");
        if (!(backtrack_step > 0.0 && backtrack_step < 1.0) || !(alpha_min > 0.0))
            throw ArgError(std::string(who) + ": backtrack_step must lie in (0, 1) and alpha_min be positive");
        // the search starts at a0 <= 1 - sqrt(eps) and visits a0 step^j while that is >= alpha_min: at most
        // floor(log(alpha_min) / log(step)) + 1 points; one more trip absorbs the rounding of the two logarithms
        const double trips = std::log(alpha_min) / std::log(backtrack_step);
        const int cap = !(trips > 0.0) ? 2 : trips >= 2.0e9 ? INT_MAX : (int)trips + 2;
        const double* rec = step_read_record(h, 1, [&](const Publish& pub) {
            launch_step_length_ns(h->cone_dev(), h->cone_state(), d_step_z, d_step_s, d_z, d_s, step_tau, step_kappa, tau, kappa,
                                  backtrack_step, alpha_min, cap, h->step_partial.p, h->ns_partial.p, h->step_rec.p, pub, h->K.m,
                                  h->stream);
        });
        *alpha_out = rec[0];
        return HIPKKT_OK;
    });
}

static int step_barrier(hipkkt_kkt_t h, StepFamily fam, const char* who, const double* d_z, const double* d_s,
                        const double* d_step_z, const double* d_step_s, double alpha, double out[2])
{
    return guarded([&]() {
        step_guard(h, who, fam, true);
        if ((h->K.m && (!d_z || !d_s || !d_step_z || !d_step_s)) || !out) throw ArgError(std::string(who) + ": bad argument");
        const double* rec = step_read_record(h, 2, [&](const Publish& pub) {
            launch_barrier(h->cone_dev(), d_z, d_s, d_step_z, d_step_s, alpha, h->ns_partial.p, h->step_rec.p, pub, h->K.m, h->stream);
        });
        out[0] = rec[0];
        out[1] = rec[1];
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_unit_initialization(hipkkt_kkt_t h, double* d_s, double* d_z)
{
    return step_unit_initialization(h, StepFamily::Nonsym, "hipkkt_kkt_system_unit_initialization", d_s, d_z);
}

int hipkkt_kkt_system_affine_ds_ns(hipkkt_kkt_t h, double* d_out, const double* d_s)
{
    return step_affine_ds(h, StepFamily::Nonsym, "hipkkt_kkt_system_affine_ds_ns", d_out, d_s);
}

int hipkkt_kkt_system_combined_ds_ns(hipkkt_kkt_t h, double* d_out, const double* d_step_z, const double* d_step_s,
                                     const double* d_s, const double* d_z, double sigma_mu, double m_corr)
{
    return step_combined_ds(h, StepFamily::Nonsym, "hipkkt_kkt_system_combined_ds_ns", d_out, d_step_z, d_step_s, d_s, d_z, sigma_mu,
                            m_corr);
}

int hipkkt_kkt_system_step_length_ns(hipkkt_kkt_t h, const double* d_step_z, const double* d_step_s, const double* d_z,
                                     const double* d_s, double step_tau, double step_kappa, double tau, double kappa,
                                     double backtrack_step, double alpha_min, double* alpha_out)
{
    return step_length_backtrack(h, StepFamily::Nonsym, "hipkkt_kkt_system_step_length_ns", d_step_z, d_step_s, d_z, d_s, step_tau,
                                 step_kappa, tau, kappa, backtrack_step, alpha_min, alpha_out);
}

int hipkkt_kkt_system_barrier(hipkkt_kkt_t h, const double* d_z, const double* d_s, const double* d_step_z,
                              const double* d_step_s, double alpha, double out[2])
{
    return step_barrier(h, StepFamily::Nonsym, "hipkkt_kkt_system_barrier", d_z, d_s, d_step_z, d_step_s, alpha, out);
}

int hipkkt_kkt_system_unit_initialization_gp(hipkkt_kkt_t h, double* d_s, double* d_z)
{
    return step_unit_initialization(h, StepFamily::Genpow, "hipkkt_kkt_system_unit_initialization_gp", d_s, d_z);
}

int hipkkt_kkt_system_affine_ds_gp(hipkkt_kkt_t h, double* d_out, const double* d_s)
{
    return step_affine_ds(h, StepFamily::Genpow, "hipkkt_kkt_system_affine_ds_gp", d_out, d_s);
}

int hipkkt_kkt_system_combined_ds_gp(hipkkt_kkt_t h, double* d_out, const double* d_step_z, const double* d_step_s,
                                     const double* d_s, const double* d_z, double sigma_mu, double m_corr)
{
    return step_combined_ds(h, StepFamily::Genpow, "hipkkt_kkt_system_combined_ds_gp", d_out, d_step_z, d_step_s, d_s, d_z, sigma_mu,
                            m_corr);
}

int hipkkt_kkt_system_step_length_gp(hipkkt_kkt_t h, const double* d_step_z, const double* d_step_s, const double* d_z,
                                     const double* d_s, double step_tau, double step_kappa, double tau, double kappa,
                                     double backtrack_step, double alpha_min, double* alpha_out)
{
    return step_length_backtrack(h, StepFamily::Genpow, "hipkkt_kkt_system_step_length_gp", d_step_z, d_step_s, d_z, d_s, step_tau,
                                 step_kappa, tau, kappa, backtrack_step, alpha_min, alpha_out);
}

int hipkkt_kkt_system_barrier_gp(hipkkt_kkt_t h, const double* d_z, const double* d_s, const double* d_step_z,
                                 const double* d_step_s, double alpha, double out[2])
{
    return step_barrier(h, StepFamily::Genpow, "hipkkt_kkt_system_barrier_gp", d_z, d_s, d_step_z, d_step_s, alpha, out);
}

// ---- residuals and termination scalars of a device-resident iterate (iterate_kernels.hip), and the two elementwise
// steps around them.  They read K's image, q and b: no cone scaling, no factorisation, any cone kind.
static void iterate_guard(hipkkt_kkt_t h)
{
    if (!h) throw ArgError("null handle");
    if (!h->sys_ready) throw ArgError("hipkkt_kkt_system_*: call hipkkt_kkt_system_init first");
    if (h->deferred) throw ArgError("hipkkt_kkt_system_*: level C reads its scalars back (deferred status is for level B)");
    HIP_CHECK(hipSetDevice(h->device));
}

int hipkkt_kkt_system_residuals(hipkkt_kkt_t h, const double* d_x, const double* d_s, const double* d_z, double tau,
                                double* d_rx, double* d_rz, double* d_rx_inf, double* d_rz_inf, double* d_Px,
                                const double* d_d, const double* d_dinv, const double* d_e, const double* d_einv, double out[12])
{
    return guarded([&]() {
        iterate_guard(h);
        const int n = h->K.n, m = h->K.m;
        if (!out || (n && (!d_x || !d_rx || !d_rx_inf || !d_Px)) || (m && (!d_s || !d_z || !d_rz || !d_rz_inf)))
            throw ArgError("hipkkt_kkt_system_residuals: bad argument");
        const int given = (d_d ? 1 : 0) + (d_dinv ? 1 : 0) + (d_e ? 1 : 0) + (d_einv ? 1 : 0);
        if (given != 0 && given != 4)
            throw ArgError("hipkkt_kkt_system_residuals: the equilibration vectors d, dinv, e, einv are all NULL or all given");
        {
            const void* outs[5] = {d_rx, d_rz, d_rx_inf, d_rz_inf, d_Px};
            const void* ins[7] = {d_x, d_s, d_z, d_d, d_dinv, d_e, d_einv};
            for (int i = 0; i < 5; ++i) {
                if (!outs[i]) continue;
                for (int j = 0; j < 7; ++j)
                    if (outs[i] == ins[j]) throw ArgError("hipkkt_kkt_system_residuals: an output aliases an input");
                for (int j = i + 1; j < 5; ++j)
                    if (outs[i] == outs[j]) throw ArgError("hipkkt_kkt_system_residuals: two outputs alias");
            }
        }
        if (!h->it_prefix_ok) throw std::runtime_error("hipkkt_kkt_system_residuals: the rows of A are not a prefix of K's z rows");
        if (!h->it_partial.p) h->it_partial.alloc(iterate_partials());
        if (!h->step_rec.p) h->step_rec.alloc(12);
        const SpmvDev A = kkt_spmv(h);                   // (gathers the image's values first where P or A changed: fval_dirty)
        IterDev I;
        I.rend = h->it_rend.p;
        I.nlong = h->it_nlong; I.nchunks = h->it_nchunks; I.long_rows = h->it_long_rows.p;
        I.long_chunk_ptr = h->it_long_chunk_ptr.p; I.chunk_q = h->it_chunk_q.p; I.long_partial = h->it_long_partial.p;
        IterVecs V;
        V.x = d_x; V.s = d_s; V.z = d_z; V.q = h->sq.p; V.b = h->sb.p; V.tau = tau;
        V.rx = d_rx; V.rz = d_rz; V.rx_inf = d_rx_inf; V.rz_inf = d_rz_inf; V.Px = d_Px;
        V.d = d_d; V.dinv = d_dinv; V.e = d_e; V.einv = d_einv;
        const double* rec = step_read_record(h, 12, [&](const Publish& pub) {
            launch_iterate_residuals(A, I, V, n, m, h->it_partial.p, h->step_rec.p, pub, h->stream);
        });
        for (int i = 0; i < 12; ++i) out[i] = rec[i];
        return HIPKKT_OK;
    });
}

// ---- data updating (update_data!, data_updating.jl:26-247): the equilibration frozen on the handle, and new P, A, q, b
// values scaled by it on the device.  The host-only parts (index check, entry tables) are data_update.cpp's.
static void data_ensure(hipkkt_kkt_t h)
{
    // the tables and the staging, once; scalings of ones until hipkkt_kkt_system_set_equilibration says otherwise
    if (h->eq_ready) return;
    const KKTAssembly& K = h->K;
    const EntryTables T = build_entry_tables(K.n, K.m, K.N, K.colptr.data(), K.rowval.data(), K.mapP.data(), (int64_t)K.mapP.size(),
                                             K.mapA.data(), (int64_t)K.mapA.size());
    if (!T.ok) throw std::runtime_error("data updating: an entry of P or A lies outside its block of K");
    h->du_Prow.upload(T.Prow); h->du_Pcol.upload(T.Pcol);
    h->du_Arow.upload(T.Arow); h->du_Acol.upload(T.Acol);
    const std::vector<double> ones((size_t)std::max(K.n, K.m), 1.0);
    auto fill = [&](DBuf<double>& v, int len) {
        v.alloc((size_t)len);
        if (len) HIP_CHECK(hipMemcpy(v.p, ones.data(), (size_t)len * sizeof(double), hipMemcpyHostToDevice));
    };
    fill(h->eq_d, K.n); fill(h->eq_dinv, K.n); fill(h->eq_e, K.m); fill(h->eq_einv, K.m);
    h->eq_c = 1.0;
    h->du_idx.alloc(std::max(std::max(K.mapP.size(), K.mapA.size()), (size_t)std::max(K.n, K.m)));
    h->du_norms.alloc(2);
    h->eq_ready = true;
}

int hipkkt_kkt_system_set_equilibration(hipkkt_kkt_t h, const double* d, const double* e, double c)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        const int n = h->K.n, m = h->K.m;
        const bool clear = !d && !e;
        if (!clear && ((n > 0 && !d) || (m > 0 && !e)))
            throw ArgError("hipkkt_kkt_system_set_equilibration: d and e are both given or both NULL");
        if (clear) c = 1.0;
        if (!(c > 0.0) || !std::isfinite(c)) throw ArgError("hipkkt_kkt_system_set_equilibration: c must be positive and finite");
        HIP_CHECK(hipSetDevice(h->device));
        data_ensure(h);
        hipStream_t st = h->stream;
        if (clear) {
            const std::vector<double> ones((size_t)std::max(n, m), 1.0);
            for (DBuf<double>* v : {&h->eq_d, &h->eq_dinv, &h->eq_e, &h->eq_einv})
                if (v->n) HIP_CHECK(hipMemcpyAsync(v->p, ones.data(), v->n * sizeof(double), hipMemcpyHostToDevice, st));
        } else {
            if (n) HIP_CHECK(hipMemcpyAsync(h->eq_d.p, d, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
            if (m) HIP_CHECK(hipMemcpyAsync(h->eq_e.p, e, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
            launch_reciprocals(h->eq_dinv.p, h->eq_d.p, n, h->eq_einv.p, h->eq_e.p, m, st);
        }
        HIP_CHECK(hipStreamSynchronize(st));             // the caller's (and this call's) host arrays may go away
        h->eq_c = c;
        h->eqb_on = false;                               // (one joint c again: the members' cost scalings are dropped)
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_set_equilibration_batch(hipkkt_kkt_t h, const double* d, const double* e, const double* c)
{
    return guarded([&]() {
        const char* who = "hipkkt_kkt_system_set_equilibration_batch";
        if (!h) throw ArgError("null handle");
        if (h->deferred) throw ArgError("hipkkt_kkt_system_*: level C reads its scalars back (deferred status is for level B)");
        if (h->bat_nb <= 0) throw ArgError(std::string(who) + ": the handle has no partition (hipkkt_kkt_system_set_problems)");
        const int n = h->K.n, m = h->K.m, nb = h->bat_nb;
        const bool ones = !d && !e;
        if (!ones && ((n > 0 && !d) || (m > 0 && !e))) throw ArgError(std::string(who) + ": d and e are both given or both NULL");
        if (!c) throw ArgError(std::string(who) + ": c is NULL");
        const int64_t badc = check_member_costs(c, nb);
        if (badc >= 0)
            throw ArgError(std::string(who) + ": c[" + std::to_string(badc) + "] must be positive and finite (member " +
                           std::to_string(badc) + ")");
        HIP_CHECK(hipSetDevice(h->device));
        data_ensure(h);
        {
            // the update kernels read c through an entry's ROW: every stored entry of P has its column in the row's member
            const KKTAssembly& K = h->K;
            const EntryTables T = build_entry_tables(K.n, K.m, K.N, K.colptr.data(), K.rowval.data(), K.mapP.data(),
                                                     (int64_t)K.mapP.size(), K.mapA.data(), (int64_t)K.mapA.size());
            const EntryMembers E = build_entry_members(T.Prow.data(), T.Pcol.data(), (int64_t)T.Prow.size(), h->bat_plan.xmem.data(), n, nb);
            if (!T.ok || !E.ok) throw std::runtime_error(std::string(who) + ": a stored entry of P couples two members of the partition");
        }
        hipStream_t st = h->stream;
        if (h->eqb_c.n != (size_t)nb) h->eqb_c.alloc((size_t)nb);
        if (ones) {
            const std::vector<double> one((size_t)std::max(n, m), 1.0);
            for (DBuf<double>* v : {&h->eq_d, &h->eq_dinv, &h->eq_e, &h->eq_einv})
                if (v->n) HIP_CHECK(hipMemcpyAsync(v->p, one.data(), v->n * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(h->eqb_c.p, c, (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));
        } else {
            if (n) HIP_CHECK(hipMemcpyAsync(h->eq_d.p, d, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
            if (m) HIP_CHECK(hipMemcpyAsync(h->eq_e.p, e, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
            launch_reciprocals(h->eq_dinv.p, h->eq_d.p, n, h->eq_einv.p, h->eq_e.p, m, st);
            HIP_CHECK(hipMemcpyAsync(h->eqb_c.p, c, (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));         // the caller's host arrays may go away
        }
        h->eqb_c_h.assign(c, c + nb);
        h->eqb_on = true;
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_equilibration_dev(hipkkt_kkt_t h, const double** d_d, const double** d_dinv, const double** d_e,
                                        const double** d_einv)
{
    return guarded([&]() {
        if (!h || !d_d || !d_dinv || !d_e || !d_einv) throw ArgError("hipkkt_kkt_system_equilibration_dev: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        data_ensure(h);
        *d_d = h->eq_d.p; *d_dinv = h->eq_dinv.p; *d_e = h->eq_e.p; *d_einv = h->eq_einv.p;
        return HIPKKT_OK;
    });
}

// the checks the four calls share -> the device copy of the positions (nullptr: the vector form), staged behind nothing
// but its own upload; returns false for the no-op k = 0.  Nothing of the handle is touched before every check has passed.
static bool data_update_begin(hipkkt_kkt_t h, const char* who, const double* d_values, const int64_t* index, int64_t k,
                              int64_t len, bool need_init, const int64_t** d_index)
{
    if (!h) throw ArgError("null handle");
    if (h->deferred) throw ArgError("hipkkt_kkt_system_*: level C reads its scalars back (deferred status is for level B)");
    if (need_init && !h->sys_ready) throw ArgError("hipkkt_kkt_system_*: call hipkkt_kkt_system_init first");
    if (k < 0) throw ArgError(std::string(who) + ": k is negative");
    if (k == 0) return false;                            // (data_updating.jl:61, 189, 223)
    if (!d_values) throw ArgError(std::string(who) + ": d_values is NULL");
    if (!index && k != len)
        throw ArgError(std::string(who) + ": the vector form takes " + std::to_string(len) + " values, got k = " + std::to_string(k));
    if (index) {
        const IndexCheck ic = check_update_index(index, k, len);
        if (ic.fault == IndexFault::OutOfRange)
            throw ArgError(std::string(who) + ": index[" + std::to_string(ic.pos) + "] = " + std::to_string(ic.value) +
                           " is out of range [0, " + std::to_string(len) + ")");
        if (ic.fault == IndexFault::Repeated)
            throw ArgError(std::string(who) + ": index[" + std::to_string(ic.pos) + "] = " + std::to_string(ic.value) +
                           " repeats an earlier position (a parallel scatter cannot apply repeats in order)");
    }
    HIP_CHECK(hipSetDevice(h->device));
    data_ensure(h);
    *d_index = nullptr;
    if (index) {
        HIP_CHECK(hipMemcpyAsync(h->du_idx.p, index, (size_t)k * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
        h->host_upload_mark(h->stream);
        *d_index = h->du_idx.p;
    }
    return true;
}

static int data_update_matrix(hipkkt_kkt_t h, const char* who, bool isP, const double* d_values, const int64_t* index, int64_t k)
{
    return guarded([&]() {
        const int64_t len = h ? (int64_t)(isP ? h->K.mapP.size() : h->K.mapA.size()) : 0;
        const int64_t* d_index = nullptr;
        if (!data_update_begin(h, who, d_values, index, k, len, false, &d_index)) return HIPKKT_OK;
        DataMatDev M;
        M.val = isP ? h->Pval.p : h->Aval.p;
        M.K = h->Kval.p;
        M.fval = h->fval_dirty ? nullptr : h->fval.p;    // (through to a current image, never into a dirty one)
        M.kpos = h->kpos.p;
        M.map = isP ? h->mapP.p : h->mapA.p;
        M.row = isP ? h->du_Prow.p : h->du_Arow.p;
        M.col = isP ? h->du_Pcol.p : h->du_Acol.p;
        M.L = isP ? h->eq_d.p : h->eq_e.p;
        M.R = h->eq_d.p;
        M.c = isP ? h->eq_c : 1.0;                       // (a product by 1.0 is exact: A's fl(v * fl(e d)))
        // (member cost scalings: P's c is that of the entry's row's member; uniform over the launch, decided here)
        if (isP && h->eqb_on) launch_data_update_matrix_member(M, h->bat_xmem.p, h->eqb_c.p, d_values, d_index, k, h->stream);
        else launch_data_update_matrix(M, d_values, d_index, k, h->stream);
        HIP_CHECK(hipGetLastError());
        h->data_factor_stale = true;
        h->data_const_stale = true;
        if (index) h->host_upload_wait();
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_update_data_P(hipkkt_kkt_t h, const double* d_values, const int64_t* index, int64_t k)
{
    return data_update_matrix(h, "hipkkt_kkt_system_update_data_P", true, d_values, index, k);
}

int hipkkt_kkt_system_update_data_A(hipkkt_kkt_t h, const double* d_values, const int64_t* index, int64_t k)
{
    return data_update_matrix(h, "hipkkt_kkt_system_update_data_A", false, d_values, index, k);
}

static int data_update_vector(hipkkt_kkt_t h, const char* who, bool isq, const double* d_values, const int64_t* index, int64_t k)
{
    return guarded([&]() {
        const int64_t len = h ? (isq ? h->K.n : h->K.m) : 0;
        const int64_t* d_index = nullptr;
        if (!data_update_begin(h, who, d_values, index, k, len, true, &d_index)) return HIPKKT_OK;
        if (isq && h->eqb_on)
            launch_data_update_vector_member(h->sq.p, h->snegq.p, h->eq_d.p, h->bat_xmem.p, h->eqb_c.p, d_values, d_index, k, h->stream);
        else if (isq) launch_data_update_vector(h->sq.p, h->snegq.p, h->eq_d.p, h->eq_c, d_values, d_index, k, h->stream);
        else launch_data_update_vector(h->sb.p, nullptr, h->eq_e.p, 1.0, d_values, d_index, k, h->stream);
        HIP_CHECK(hipGetLastError());
        h->data_const_stale = true;
        if (index) h->host_upload_wait();
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_update_data_q(hipkkt_kkt_t h, const double* d_values, const int64_t* index, int64_t k)
{
    return data_update_vector(h, "hipkkt_kkt_system_update_data_q", true, d_values, index, k);
}

int hipkkt_kkt_system_update_data_b(hipkkt_kkt_t h, const double* d_values, const int64_t* index, int64_t k)
{
    return data_update_vector(h, "hipkkt_kkt_system_update_data_b", false, d_values, index, k);
}

int hipkkt_kkt_system_data_norms(hipkkt_kkt_t h, double out[2])
{
    return guarded([&]() {
        iterate_guard(h);
        if (!out) throw ArgError("hipkkt_kkt_system_data_norms: bad argument");
        data_ensure(h);
        hipStream_t st = h->stream;
        HIP_CHECK(hipMemsetAsync(h->du_norms.p, 0, 2 * sizeof(double), st));
        launch_data_norms(h->sq.p, h->eq_dinv.p, h->K.n, h->sb.p, h->eq_einv.p, h->K.m, h->du_norms.p, st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(h->pin->h + 52, h->du_norms.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        out[0] = h->pin->h[52] / h->eq_c;                // data_get_normq!: the unscaled norm, cinv applied (problemdata.jl:91-100)
        out[1] = h->pin->h[53];
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_data_norms_batch(hipkkt_kkt_t h, double* out)
{
    return guarded([&]() {
        iterate_guard(h);
        if (!out) throw ArgError("hipkkt_kkt_system_data_norms_batch: bad argument");
        if (h->bat_nb <= 0)
            throw ArgError("hipkkt_kkt_system_data_norms_batch: the handle has no partition (hipkkt_kkt_system_set_problems)");
        data_ensure(h);
        const int n = h->K.n, m = h->K.m;
        const size_t nb = (size_t)h->bat_nb;
        if (!h->eqb_slot_ready) {                        // every combined row's word, once per partition
            const std::vector<int> slot = build_norm_slots(h->bat_plan.xmem.data(), n, h->bat_plan.zmem.data(), m, h->bat_nb);
            if (slot.size() != (size_t)n + (size_t)m) throw std::runtime_error("hipkkt_kkt_system_data_norms_batch: a row's member is out of range");
            h->eqb_slot.upload(slot);
            h->eqb_norms.alloc(2 * nb);
            h->eqb_slot_ready = true;
        }
        hipStream_t st = h->stream;
        h->eqb_norms.zero(st);
        launch_data_norms_member(h->sq.p, h->eq_dinv.p, n, h->sb.p, h->eq_einv.p, m, h->eqb_slot.p, h->eqb_norms.p, st);
        HIP_CHECK(hipGetLastError());
        double* stage = h->bat_pin + 4 * nb;             // (the results' part of the page-locked staging: 2 nb of its 12 nb)
        HIP_CHECK(hipMemcpyAsync(stage, h->eqb_norms.p, 2 * nb * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (size_t b = 0; b < nb; ++b) {
            // data_get_normq! per member: the unscaled norm, the member's cinv applied (problemdata.jl:91-100)
            out[2 * b] = stage[2 * b] / (h->eqb_on ? h->eqb_c_h[b] : h->eq_c);
            out[2 * b + 1] = stage[2 * b + 1];
        }
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_combined_rhs(hipkkt_kkt_t h, double* d_rhs_x, double* d_rhs_z, const double* d_rx, const double* d_rz,
                                   double sigma)
{
    return guarded([&]() {
        iterate_guard(h);
        if ((h->K.n && (!d_rhs_x || !d_rx)) || (h->K.m && (!d_rhs_z || !d_rz)))
            throw ArgError("hipkkt_kkt_system_combined_rhs: bad argument");
        launch_iterate_scale(d_rhs_x, d_rhs_z, d_rx, d_rz, 1.0 - sigma, h->K.n, h->K.m, h->stream);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_add_step(hipkkt_kkt_t h, double* d_x, double* d_s, double* d_z, const double* d_dx, const double* d_ds,
                               const double* d_dz, double alpha)
{
    return guarded([&]() {
        iterate_guard(h);
        if ((h->K.n && (!d_x || !d_dx)) || (h->K.m && (!d_s || !d_z || !d_ds || !d_dz)))
            throw ArgError("hipkkt_kkt_system_add_step: bad argument");
        if ((d_x && d_x == d_dx) || (d_s && (d_s == d_ds || d_s == d_dz)) || (d_z && (d_z == d_dz || d_z == d_ds)) || (d_s && d_s == d_z))
            throw ArgError("hipkkt_kkt_system_add_step: bad argument (a step must not alias the vector it is added to)");
        launch_iterate_add_step(d_x, d_s, d_z, d_dx, d_ds, d_dz, alpha, h->K.n, h->K.m, h->stream);
        return HIPKKT_OK;
    });
}

// ---- a stack of independent member problems on one handle (batch_plan.hpp; kernels.hpp: BatchDev): the partition, and the
// seven operations between the solves with every scalar an array over the members.  Each call uploads its scalar arrays
// in ONE copy and reads its results back in ONE copy, whatever the number of members.
int hipkkt_kkt_system_set_problems(hipkkt_kkt_t h, int64_t nb, const int64_t* x_off, const int64_t* z_off)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        if (!h->sys_ready) throw ArgError("hipkkt_kkt_system_*: call hipkkt_kkt_system_init first");
        if (h->deferred) throw ArgError("hipkkt_kkt_system_*: level C reads its scalars back (deferred status is for level B)");
        if (h->eqb_on)
            throw ArgError("hipkkt_kkt_system_set_problems: the handle holds member cost scalings "
                           "(hipkkt_kkt_system_set_equilibration_batch) that belong to its partition; clear them first with "
                           "hipkkt_kkt_system_set_equilibration");
        HIP_CHECK(hipSetDevice(h->device));
        if (nb == 0) {                                   // (the tables stay allocated until the next partition or the handle's end)
            h->eqb_slot_ready = false;
            h->bat_nb = 0;
            h->mr_on = h->mr_valid = false;             // (the member refinement rule goes with its partition)
            h->ms_on = h->ms_valid = false;             // (... and so does the member status)
            return HIPKKT_OK;
        }
        if (nb < 0) throw ArgError("hipkkt_kkt_system_set_problems: the number of members is negative");
        if (h->K.nnonsym > 0 || h->K.ngenpow > 0)
            throw ArgError("hipkkt_kkt_system_set_problems: symmetric cones only (the handle holds an exponential, power or "
                           "generalized power cone)");
        if (h->large_psd || h->psd_too_big)
            throw ArgError("hipkkt_kkt_system_set_problems: PSD cones up to side 48 only (the handle has enabled large PSD cones "
                           "or holds one)");
        std::vector<BatchCone> cones;
        for (const ConeInfo& ci : h->K.cones) cones.push_back(BatchCone{ci.kind, ci.off, ci.numel, ci.dim});
        BatchPlan P;
        const std::string err = plan_batch(h->K.n, h->K.m, nb, x_off, z_off, cones.data(), (int)cones.size(), h->K.colptr.data(),
                                           h->K.rowval.data(), h->it_long_rows_h.data(), (int)h->it_long_rows_h.size(), P);
        if (!err.empty()) throw ArgError("hipkkt_kkt_system_set_problems: " + err);
        HIP_CHECK(hipStreamSynchronize(h->stream));      // (nothing in flight reads the tables that are replaced now)
        h->bat_nb = 0;
        h->mr_on = h->mr_valid = false;
        h->ms_on = h->ms_valid = false;
        h->eqb_slot_ready = false;                       // (the norms' words go with their partition)
        h->bat_xoff.upload(P.x_off); h->bat_zoff.upload(P.z_off); h->bat_xmem.upload(P.xmem); h->bat_zmem.upload(P.zmem);
        h->bat_cmem.upload(P.cone_mem); h->bat_socptr.upload(P.soc_ptr); h->bat_psdptr.upload(P.psd_ptr);
        h->bat_degree.upload(P.degree);
        h->bat_r32mem.upload(P.rows32.wg_mem); h->bat_r32first.upload(P.rows32.wg_first); h->bat_r32ptr.upload(P.rows32.wg_ptr);
        h->bat_r256mem.upload(P.rows256.wg_mem); h->bat_r256first.upload(P.rows256.wg_first); h->bat_r256ptr.upload(P.rows256.wg_ptr);
        h->bat_z256mem.upload(P.z256.wg_mem); h->bat_z256first.upload(P.z256.wg_first); h->bat_z256ptr.upload(P.z256.wg_ptr);
        h->bat_lorder.upload(P.long_order); h->bat_lptr.upload(P.long_ptr);
        h->bat_nwg32 = (int)P.rows32.wg_mem.size();
        h->bat_nwg256 = (int)P.rows256.wg_mem.size();
        h->bat_nwgz = (int)P.z256.wg_mem.size();
        const size_t k = (size_t)P.nb;
        h->bat_scal.alloc(4 * k); h->bat_rec.alloc(12 * k); h->bat_shift.alloc(3 * k); h->bat_dtau.alloc(k);
        h->bat_it_partial.alloc((size_t)kIterValues * ((size_t)h->bat_nwg32 + (size_t)h->it_nlong));
        h->bat_step_partial.alloc(2 * ((size_t)h->bat_nwgz + (size_t)h->nsoc + (size_t)h->npsd));
        h->bat_dot_partial.alloc((size_t)7 * h->bat_nwg256);
        if (h->bat_pin) { (void)hipHostFree(h->bat_pin); h->bat_pin = nullptr; }
        HIP_CHECK(hipHostMalloc((void**)&h->bat_pin, 16 * k * sizeof(double)));
        if (!h->bat_ev) HIP_CHECK(hipEventCreateWithFlags(&h->bat_ev, hipEventDisableTiming));
        h->bat_nb = P.nb;
        h->bat_plan = std::move(P);              // (kept for hipkkt_kkt_system_set_member_refinement)
        return HIPKKT_OK;
    });
}

// the partition carried over to K's image (batch_plan.hpp: plan_batch_image), for either member mode; returns the chunk
static int member_image_plan(hipkkt_kkt_t h, const char* who, BatchImagePlan& I)
{
    std::vector<BatchImageCone> cones;
    for (const ConeInfo& ci : h->K.cones) cones.push_back(BatchImageCone{ci.pcol, ci.pwidth});
    // rows per workgroup: whole passes of the residual kernel's rows per block, few enough workgroups that a member's
    // slots are folded cheaply (at most kNormParts + nb in all, as the whole-handle pass has kNormParts)
    const int rpb = 256 / h->lanes_per_row;
    const int passes = (int)(((int64_t)h->K.N + (int64_t)rpb * kNormParts - 1) / ((int64_t)rpb * kNormParts));
    const int chunk = rpb * std::max(passes, 1);
    const std::string err = plan_batch_image(h->K.n, h->K.m, h->K.p, h->bat_plan, cones.data(), (int)cones.size(),
                                             h->long_rows_h.data(), (int)h->long_rows_h.size(), chunk, I);
    if (!err.empty()) throw ArgError(std::string(who) + ": " + err);
    return chunk;
}

// The refinement rule per member (kktsolver_directldl.jl:389-449 on each member's rows of K's image): plans the image's
// rows by member on the host (batch_plan.hpp: plan_batch_image), uploads the tables and allocates slots and state.
int hipkkt_kkt_system_set_member_refinement(hipkkt_kkt_t h, int enable)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        if (!h->sys_ready) throw ArgError("hipkkt_kkt_system_*: call hipkkt_kkt_system_init first");
        if (h->bat_nb <= 0)
            throw ArgError("hipkkt_kkt_system_set_member_refinement: the handle has no partition (hipkkt_kkt_system_set_problems)");
        HIP_CHECK(hipSetDevice(h->device));
        HIP_CHECK(hipStreamSynchronize(h->stream));      // (nothing in flight reads the tables that are replaced now)
        h->mr_on = h->mr_valid = false;
        if (!enable) return HIPKKT_OK;
        if (h->bat_nb >= (1 << 20)) throw ArgError("hipkkt_kkt_system_set_member_refinement: at most 2^20 - 1 members");
        BatchImagePlan I;
        const int chunk = member_image_plan(h, "hipkkt_kkt_system_set_member_refinement", I);
        h->mr_wgmem.upload(I.wg.wg_mem); h->mr_wgfirst.upload(I.wg.wg_first); h->mr_wgptr.upload(I.wg.wg_ptr);
        h->mr_rows.upload(I.img_rows); h->mr_ptr.upload(I.img_ptr);
        h->mr_lorder.upload(I.long_order); h->mr_lptr.upload(I.long_ptr);
        h->mr_nwg = (int)I.wg.wg_mem.size();
        h->mr_chunk = chunk;
        const size_t nb = (size_t)h->bat_nb, S = (size_t)h->mr_nwg + nb;
        const size_t rounds = (size_t)std::max(h->st.iterative_refinement_max_iter, 0) + 1;
        h->mr_slots.alloc(3 * S); h->mr_state.alloc(4 * nb * rounds); h->mr_normb.alloc(nb); h->mr_info.alloc(4 * nb);
        h->mr_agg.alloc(2);
        // (the long rows' slots stay zero when the image has none; the counters are zero between kernels)
        h->mr_slots.zero(h->stream); h->mr_state.zero(h->stream); h->mr_normb.zero(h->stream); h->mr_info.zero(h->stream);
        h->mr_agg.zero(h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->mr_on = true;
        return HIPKKT_OK;
    });
}

// The static regulariser and the failure words per member (kktsolver_directldl.jl:259-310, directldl_qdldl.jl:72-81 on
// each member's rows and columns): row -> member from the image plan, column -> member through the factor's permutation
// (batch_plan.hpp: plan_column_members), and the work space of the three kernels.
int hipkkt_kkt_system_set_member_status(hipkkt_kkt_t h, int enable)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        if (!h->sys_ready) throw ArgError("hipkkt_kkt_system_*: call hipkkt_kkt_system_init first");
        if (h->bat_nb <= 0)
            throw ArgError("hipkkt_kkt_system_set_member_status: the handle has no partition (hipkkt_kkt_system_set_problems)");
        HIP_CHECK(hipSetDevice(h->device));
        HIP_CHECK(hipStreamSynchronize(h->stream));      // (nothing in flight reads the tables that are replaced now)
        h->ms_on = h->ms_valid = false;
        h->eng->eps_col = nullptr;
        if (!enable) return HIPKKT_OK;
        BatchImagePlan I;
        (void)member_image_plan(h, "hipkkt_kkt_system_set_member_status", I);
        std::vector<int> colmem;
        const std::vector<int>& perm = h->eng->S.perm;
        const std::string err = plan_column_members(h->K.N, h->bat_nb, perm.data(), perm.size(), I.rowmem.data(), I.rowmem.size(), colmem);
        if (!err.empty()) throw ArgError("hipkkt_kkt_system_set_member_status: " + err);
        h->ms_rowmem.upload(I.rowmem); h->ms_colmem.upload(colmem);
        const size_t nb = (size_t)h->bat_nb;
        h->ms_maxbits.alloc(nb + 1); h->ms_epscol.alloc((size_t)h->K.N); h->ms_rec.alloc(2 * nb);
        // (eps_b stays 0 when the static regulariser is disabled: nothing writes it then)
        h->ms_maxbits.zero(h->stream); h->ms_epscol.zero(h->stream); h->ms_rec.zero(h->stream);
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->ms_on = true;
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_member_status(hipkkt_kkt_t h, double* out)
{
    return guarded([&]() {
        if (!h || !out) throw ArgError("hipkkt_kkt_system_member_status: bad argument");
        if (!h->member_status_on()) throw ArgError("hipkkt_kkt_system_member_status: member status is not enabled");
        if (!h->ms_valid) throw ArgError("hipkkt_kkt_system_member_status: no update has run since member status was enabled");
        HIP_CHECK(hipSetDevice(h->device));
        const size_t nb = (size_t)h->bat_nb;
        double* stage = h->bat_pin + 4 * nb;             // {eps_b, the cone words, the pivot words}: 2 nb doubles
        HIP_CHECK(hipMemcpyAsync(stage, h->ms_rec.p, 2 * nb * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        const int* words = (const int*)(stage + nb);
        for (size_t b = 0; b < nb; ++b) {
            out[3 * b] = words[b] ? 1.0 : 0.0;
            out[3 * b + 1] = words[nb + b] ? 1.0 : 0.0;
            out[3 * b + 2] = h->st.static_regularization_enable ? stage[b] : 0.0;
        }
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_member_refinement_info(hipkkt_kkt_t h, double* out)
{
    return guarded([&]() {
        if (!h || !out) throw ArgError("hipkkt_kkt_system_member_refinement_info: bad argument");
        if (!h->mr_on || h->bat_nb <= 0) throw ArgError("hipkkt_kkt_system_member_refinement_info: member refinement is not enabled");
        if (!h->mr_valid) throw ArgError("hipkkt_kkt_system_member_refinement_info: no solve has run under the member rule yet");
        HIP_CHECK(hipSetDevice(h->device));
        const size_t count = 4 * (size_t)h->bat_nb;
        double* stage = h->bat_pin + 4 * (size_t)h->bat_nb;
        HIP_CHECK(hipMemcpyAsync(stage, h->mr_info.p, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        std::memcpy(out, stage, count * sizeof(double));
        return HIPKKT_OK;
    });
}

static void batch_guard(hipkkt_kkt_t h, const char* who, bool cones, bool need_scaling)
{
    if (!h) throw ArgError("null handle");
    if (!h->sys_ready) throw ArgError("hipkkt_kkt_system_*: call hipkkt_kkt_system_init first");
    if (h->deferred) throw ArgError("hipkkt_kkt_system_*: level C reads its scalars back (deferred status is for level B)");
    if (h->bat_nb <= 0) throw ArgError(std::string(who) + ": the handle has no partition (hipkkt_kkt_system_set_problems)");
    if (cones && h->large_psd) throw ArgError(std::string(who) + ": PSD cones up to side 48 only (large PSD cones were enabled)");
    if (need_scaling && !h->scaling_valid) throw ArgError(std::string(who) + ": needs the cone scaling of hipkkt_kkt_system_update");
    HIP_CHECK(hipSetDevice(h->device));
}

// k host arrays of nb doubles -> the device, array after array, in one copy; returns the device address of the first
static const double* batch_upload(hipkkt_kkt_t h, const char* who, std::initializer_list<const double*> arrays)
{
    const size_t nb = (size_t)h->bat_nb;
    for (const double* a : arrays)
        if (!a) throw ArgError(std::string(who) + ": a scalar array is NULL");
    HIP_CHECK(hipEventSynchronize(h->bat_ev));        // (the previous call's upload has left bat_pin)
    size_t at = 0;
    for (const double* a : arrays) { std::memcpy(h->bat_pin + at, a, nb * sizeof(double)); at += nb; }
    HIP_CHECK(hipMemcpyAsync(h->bat_scal.p, h->bat_pin, at * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipEventRecord(h->bat_ev, h->stream));
    return h->bat_scal.p;
}

// per doubles per member from bat_rec to the caller's host array, in one copy; synchronises
static void batch_download(hipkkt_kkt_t h, double* out, int per)
{
    const size_t count = (size_t)per * (size_t)h->bat_nb;
    double* stage = h->bat_pin + 4 * (size_t)h->bat_nb;
    HIP_CHECK(hipMemcpyAsync(stage, h->bat_rec.p, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (out) std::memcpy(out, stage, count * sizeof(double));
}

int hipkkt_kkt_system_residuals_batch(hipkkt_kkt_t h, const double* d_x, const double* d_s, const double* d_z, const double* tau,
                                      double* d_rx, double* d_rz, double* d_rx_inf, double* d_rz_inf, double* d_Px,
                                      const double* d_d, const double* d_dinv, const double* d_e, const double* d_einv, double* out)
{
    return guarded([&]() {
        batch_guard(h, "hipkkt_kkt_system_residuals_batch", false, false);
        const int n = h->K.n, m = h->K.m;
        if (!out || !tau || (n && (!d_x || !d_rx || !d_rx_inf || !d_Px)) || (m && (!d_s || !d_z || !d_rz || !d_rz_inf)))
            throw ArgError("hipkkt_kkt_system_residuals_batch: bad argument");
        const int given = (d_d ? 1 : 0) + (d_dinv ? 1 : 0) + (d_e ? 1 : 0) + (d_einv ? 1 : 0);
        if (given != 0 && given != 4)
            throw ArgError("hipkkt_kkt_system_residuals_batch: the equilibration vectors d, dinv, e, einv are all NULL or all given");
        {
            const void* outs[5] = {d_rx, d_rz, d_rx_inf, d_rz_inf, d_Px};
            const void* ins[7] = {d_x, d_s, d_z, d_d, d_dinv, d_e, d_einv};
            for (int i = 0; i < 5; ++i) {
                if (!outs[i]) continue;
                for (int j = 0; j < 7; ++j)
                    if (outs[i] == ins[j]) throw ArgError("hipkkt_kkt_system_residuals_batch: an output aliases an input");
                for (int j = i + 1; j < 5; ++j)
                    if (outs[i] == outs[j]) throw ArgError("hipkkt_kkt_system_residuals_batch: two outputs alias");
            }
        }
        if (!h->it_prefix_ok) throw std::runtime_error("hipkkt_kkt_system_residuals_batch: the rows of A are not a prefix of K's z rows");
        const SpmvDev A = kkt_spmv(h);
        IterDev I;
        I.rend = h->it_rend.p;
        I.nlong = h->it_nlong; I.nchunks = h->it_nchunks; I.long_rows = h->it_long_rows.p;
        I.long_chunk_ptr = h->it_long_chunk_ptr.p; I.chunk_q = h->it_chunk_q.p; I.long_partial = h->it_long_partial.p;
        IterVecs V;
        V.x = d_x; V.s = d_s; V.z = d_z; V.q = h->sq.p; V.b = h->sb.p; V.tau = 0.0;
        V.rx = d_rx; V.rz = d_rz; V.rx_inf = d_rx_inf; V.rz_inf = d_rz_inf; V.Px = d_Px;
        V.d = d_d; V.dinv = d_dinv; V.e = d_e; V.einv = d_einv;
        const double* d_tau = batch_upload(h, "hipkkt_kkt_system_residuals_batch", {tau});
        launch_batch_residuals(A, I, V, h->batch_dev(), d_tau, n, m, h->bat_it_partial.p, h->bat_rec.p, h->stream);
        batch_download(h, out, 12);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_combined_rhs_batch(hipkkt_kkt_t h, double* d_rhs_x, double* d_rhs_z, const double* d_rx, const double* d_rz,
                                         const double* sigma)
{
    return guarded([&]() {
        batch_guard(h, "hipkkt_kkt_system_combined_rhs_batch", false, false);
        if ((h->K.n && (!d_rhs_x || !d_rx)) || (h->K.m && (!d_rhs_z || !d_rz)))
            throw ArgError("hipkkt_kkt_system_combined_rhs_batch: bad argument");
        const double* d_sigma = batch_upload(h, "hipkkt_kkt_system_combined_rhs_batch", {sigma});
        launch_batch_scale(h->batch_dev(), d_rhs_x, d_rhs_z, d_rx, d_rz, d_sigma, h->K.n, h->K.m, h->stream);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_add_step_batch(hipkkt_kkt_t h, double* d_x, double* d_s, double* d_z, const double* d_dx, const double* d_ds,
                                     const double* d_dz, const double* alpha)
{
    return guarded([&]() {
        batch_guard(h, "hipkkt_kkt_system_add_step_batch", false, false);
        if ((h->K.n && (!d_x || !d_dx)) || (h->K.m && (!d_s || !d_z || !d_ds || !d_dz)))
            throw ArgError("hipkkt_kkt_system_add_step_batch: bad argument");
        if ((d_x && d_x == d_dx) || (d_s && (d_s == d_ds || d_s == d_dz)) || (d_z && (d_z == d_dz || d_z == d_ds)) || (d_s && d_s == d_z))
            throw ArgError("hipkkt_kkt_system_add_step_batch: bad argument (a step must not alias the vector it is added to)");
        const double* d_alpha = batch_upload(h, "hipkkt_kkt_system_add_step_batch", {alpha});
        launch_batch_add_step(h->batch_dev(), d_x, d_s, d_z, d_dx, d_ds, d_dz, d_alpha, h->K.n, h->K.m, h->stream);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_combined_ds_batch(hipkkt_kkt_t h, double* d_out, const double* d_step_z, const double* d_step_s,
                                        const double* sigma_mu, const double* m_corr)
{
    return guarded([&]() {
        batch_guard(h, "hipkkt_kkt_system_combined_ds_batch", true, true);
        if (h->K.m && (!d_out || !d_step_z || !d_step_s || d_out == d_step_z || d_out == d_step_s))
            throw ArgError("hipkkt_kkt_system_combined_ds_batch: bad argument (d_out must not alias an input)");
        const double* d_scal = batch_upload(h, "hipkkt_kkt_system_combined_ds_batch", {sigma_mu, m_corr});
        launch_batch_step_ds(h->cone_dev(), h->cone_state(), h->batch_dev(), d_out, d_step_z, d_step_s, d_scal, d_scal + h->bat_nb,
                             h->K.m, h->stream);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_step_length_batch(hipkkt_kkt_t h, const double* d_step_z, const double* d_step_s, const double* d_z,
                                        const double* d_s, const double* step_tau, const double* step_kappa, const double* tau,
                                        const double* kappa, double* alpha_out)
{
    return guarded([&]() {
        batch_guard(h, "hipkkt_kkt_system_step_length_batch", true, true);
        if ((h->K.m && (!d_step_z || !d_step_s || !d_z || !d_s)) || !alpha_out)
            throw ArgError("hipkkt_kkt_system_step_length_batch: bad argument");
        const double* d_scal = batch_upload(h, "hipkkt_kkt_system_step_length_batch", {step_tau, step_kappa, tau, kappa});
        launch_batch_step_length(h->cone_dev(), h->cone_state(), h->batch_dev(), d_step_z, d_step_s, d_z, d_s, d_scal,
                                 h->bat_step_partial.p, h->bat_rec.p, h->K.m, h->stream);
        batch_download(h, alpha_out, 1);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_shift_to_interior_batch(hipkkt_kkt_t h, double* d_v, int primal, double* margins_out)
{
    return guarded([&]() {
        batch_guard(h, "hipkkt_kkt_system_shift_to_interior_batch", true, false);
        if ((h->K.m && !d_v) || (primal != 0 && primal != 1)) throw ArgError("hipkkt_kkt_system_shift_to_interior_batch: bad argument");
        launch_batch_shift_to_interior(h->cone_dev(), h->batch_dev(), d_v, primal == 1, h->bat_step_partial.p, h->bat_shift.p,
                                       h->bat_rec.p, h->K.m, h->stream);
        batch_download(h, margins_out, 2);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_solve_batch(hipkkt_kkt_t h, double* d_lhs_x, double* d_lhs_s, double* d_lhs_z, double* lhs_tau_kappa,
                                  const double* d_rhs_x, const double* d_rhs_s, const double* d_rhs_z, const double* rhs_tau,
                                  const double* rhs_kappa, const double* d_var_x, const double* d_var_s, const double* d_var_z,
                                  const double* var_tau, const double* var_kappa, int steptype)
{
    return guarded([&]() {
        batch_guard(h, "hipkkt_kkt_system_solve_batch", true, true);
        const int n = h->K.n, m = h->K.m;
        const bool affine = steptype == 0;
        if ((n && (!d_lhs_x || !d_rhs_x || !d_var_x)) || (m && (!d_lhs_s || !d_lhs_z || !d_rhs_z || !d_var_s || !d_var_z)) ||
            (m && !affine && !d_rhs_s) || !lhs_tau_kappa || (steptype != 0 && steptype != 1))
            throw ArgError("hipkkt_kkt_system_solve_batch: bad argument");
        if (!rhs_tau || !rhs_kappa || !var_tau || !var_kappa) throw ArgError("hipkkt_kkt_system_solve_batch: a scalar array is NULL");
        data_refuse_stale_solve(h);
        hipStream_t st = h->stream;
        // (x2, z2) still due (lazy mode): by itself first, as kkt_update! would have done it -- the 2-column pairing is the
        // whole-handle call's; and the status of an enqueued-only update is read before this call's own
        int rc = sys_flush_update_status(h);
        if (rc == HIPKKT_OK && h->sys_const_pending) {
            h->sys_const_pending = false;
            rc = sys_constant_rhs(h);
        }
        if (rc != HIPKKT_OK) return rc;
        const double* d_scal = batch_upload(h, "hipkkt_kkt_system_solve_batch", {rhs_tau, rhs_kappa, var_tau, var_kappa});
        // Delta_s constant term and the right-hand side (kktsystem.jl:150-173), as hipkkt_kkt_system_solve
        if (!affine && !launch_sys_offset(h->cone_dev(), h->cone_state(), h->sconic.p, h->sworkz.p, d_rhs_s, d_var_z, d_rhs_z, m, false, st))
            throw ArgError("hipkkt_kkt_system_solve_batch: unsupported cone kind");
        if (affine) launch_pack_rhs_affine(h->b.p, nullptr, nullptr, d_rhs_x, d_var_s, d_rhs_z, n, m, h->K.p, 1, st);
        else launch_pack_rhs(h->b.p, d_rhs_x, h->sworkz.p, n, m, h->K.p, st);
        rc = kkt_solve_core(h, false, 1, nullptr, false);
        // Under member status AND member refinement a failed solve names its members (hipkkt_kkt_system_member_refinement_info)
        // and the others' rows are finished: the step is recovered for every member, the return value stays the joint one
        const bool attributed = rc == HIPKKT_NUMERIC_FAILURE && h->member_status_on() && h->mr_on && h->mr_valid;
        if (rc != HIPKKT_OK && !attributed) return rc;
        const double* x1 = h->x.p;
        // the dot products, dtau, dkappa and (dx, dz) per member (:185-206); the x2-only terms are formed here as well
        launch_batch_sys_step(sys_spmv(h), h->Kval.p, h->batch_dev(), h->sq.p, h->sb.p, d_var_x, x1, x1 + n, h->sx2.p, h->sz2.p, d_scal,
                              h->spa.p, h->spb.p, h->spc.p, h->sworkx.p, h->bat_dot_partial.p, h->bat_dtau.p, h->bat_rec.p, d_lhs_x,
                              d_lhs_z, n, m, st);
        // ds = -(Hs dz + const)                                               (:206-212)
        launch_mul_Hs(h->cone_dev(), h->cone_state(), d_lhs_s, d_lhs_z, m, st, affine ? d_var_s : h->sconic.p);
        batch_download(h, lhs_tau_kappa, 2);
        return rc;
    });
}

int hipkkt_kkt_system_update_and_solve_affine(hipkkt_kkt_t h, double* d_lhs_x, double* d_lhs_s, double* d_lhs_z,
                                              double* lhs_tau_kappa, const double* d_rhs_x, const double* d_rhs_z,
                                              double rhs_tau, double rhs_kappa, const double* d_var_x, const double* d_var_s,
                                              const double* d_var_z, double var_tau, double var_kappa)
{
    // kkt_update! in lazy mode followed by the affine kkt_solve!: exactly what the two separate calls do
    if (!h) { g_last_error = "null handle"; return HIPKKT_ERR_ARG; }
    const bool was_lazy = h->sys_lazy;
    h->sys_lazy = true;
    int rc = hipkkt_kkt_system_update(h, d_var_s, d_var_z);
    h->sys_lazy = was_lazy;
    if (rc != HIPKKT_OK) return rc;
    return guarded([&]() {
        return sys_solve_step(h, d_lhs_x, d_lhs_s, d_lhs_z, lhs_tau_kappa, d_rhs_x, nullptr, d_rhs_z, rhs_tau, rhs_kappa,
                              d_var_x, d_var_s, d_var_z, var_tau, var_kappa, 0);
    });
}

// kkt_update! from the caller's cone objects (the Julia glue): kktsolver_update!'s data plus the NT scaling that
// kkt_solve!'s right-hand-side construction and step recovery read from the same cones
int hipkkt_kkt_system_update_cones(hipkkt_kkt_t h, const double* Hs, const double* soc_u, const double* soc_v,
                                   const double* soc_eta2, const double* w, const double* eta, const double* lambda,
                                   const double* psd_R, const double* psd_Rinv)
{
    if (h && h->deferred) {
        g_last_error = "hipkkt_kkt_system_*: level C reads its scalars back (deferred status is for level B)";
        return HIPKKT_ERR_ARG;
    }
    int rc = hipkkt_kkt_update_cones(h, Hs, soc_u, soc_v, soc_eta2);
    if (rc != HIPKKT_OK) return rc;
    return guarded([&]() {
        const size_t m = (size_t)h->K.m, nc = h->K.cones.size();
        if ((m && (!w || !lambda)) || (h->nsoc > 0 && !eta) || (h->npsd + h->npsdb > 0 && (!psd_R || !psd_Rinv)))
            throw ArgError("hipkkt_kkt_system_update_cones: missing scaling data");
        if (h->psd_too_big && !h->large_psd)
            throw ArgError("hipkkt_kkt_system_*: PSD cones with side > 48 are not covered by level C");
        if (h->psdb_kmax > kPsdBigMaxDim)
            throw ArgError("hipkkt_kkt_system_*: PSD cones with side > 96 are not covered by level C");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        if (m) {
            HIP_CHECK(hipMemcpyAsync(h->w.p, w, m * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(h->lam.p, lambda, m * sizeof(double), hipMemcpyHostToDevice, st));
        }
        if (eta && nc) HIP_CHECK(hipMemcpyAsync(h->eta.p, eta, nc * sizeof(double), hipMemcpyHostToDevice, st));
        if (h->npsd + h->npsdb > 0) {
            HIP_CHECK(hipMemcpyAsync(h->psdR.p, psd_R, h->psdR.n * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(h->psdRinv.p, psd_Rinv, h->psdRinv.n * sizeof(double), hipMemcpyHostToDevice, st));
            launch_psd_A_from_R(h->cone_dev(), h->cone_state(), st);       // A = R R' (mul_Hs!, coneops_psdtrianglecone.jl:164-187)
        }
        HIP_CHECK(hipStreamSynchronize(st));           // the caller's arrays may go away
        h->scaling_valid = true;
        return sys_after_update(h);
    });
}

int hipkkt_kkt_system_update_scaling(hipkkt_kkt_t h, const double* w, const double* eta, const double* lambda,
                                     const double* psd_R, const double* psd_Rinv)
{
    if (h && h->deferred) {
        g_last_error = "hipkkt_kkt_system_*: level C reads its scalars back (deferred status is for level B)";
        return HIPKKT_ERR_ARG;
    }
    bool enqueue_only = false;
    int rc = guarded([&]() {
        if (!h) throw ArgError("null handle");
        const size_t m = (size_t)h->K.m, nc = h->K.cones.size();
        if ((m && (!w || !lambda)) || (h->nsoc > 0 && !eta) || (h->npsd + h->npsdb > 0 && (!psd_R || !psd_Rinv)))
            throw ArgError("hipkkt_kkt_system_update_scaling: missing scaling data");
        if (h->psd_too_big && !h->large_psd)
            throw ArgError("hipkkt_kkt_system_*: PSD cones with side > 48 are not covered by level C");
        if (h->psdb_kmax > kPsdBigMaxDim)
            throw ArgError("hipkkt_kkt_system_*: PSD cones with side > 96 are not covered by level C");
        if (h->K.nnonsym > 0)
            throw ArgError("hipkkt_kkt_system_update_scaling: (w, eta, lambda, R) cannot carry the 3 x 3 block of an exponential "
                           "or power cone; use hipkkt_kkt_system_update_cones");
        if (h->K.ngenpow > 0)
            throw ArgError("hipkkt_kkt_system_update_scaling: (w, eta, lambda, R) cannot carry p, q, r of a generalized power "
                           "cone; such a handle is scaled on the device (hipkkt_kkt_system_update)");
        HIP_CHECK(hipSetDevice(h->device));
        hipStream_t st = h->stream;
        if (m) {
            HIP_CHECK(hipMemcpyAsync(h->w.p, w, m * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(h->lam.p, lambda, m * sizeof(double), hipMemcpyHostToDevice, st));
        }
        if (eta && nc) HIP_CHECK(hipMemcpyAsync(h->eta.p, eta, nc * sizeof(double), hipMemcpyHostToDevice, st));
        if (h->npsd + h->npsdb > 0) {
            HIP_CHECK(hipMemcpyAsync(h->psdR.p, psd_R, h->psdR.n * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(h->psdRinv.p, psd_Rinv, h->psdRinv.n * sizeof(double), hipMemcpyHostToDevice, st));
        }
        // the caller's arrays are free again once these copies have run; the kernels behind them need not have
        h->host_upload_mark(st);
        kkt_zero_update_words(h);
        int pu = h->prof.begin(0, st);
        launch_cone_from_scaling(h->cone_dev(), h->cone_state(), h->K.m, st);      // Hs, u, v, eta^2 (and R R') on the device
        h->prof.end(pu, st);
        h->scaling_valid = true;
        enqueue_only = h->sys_lazy && h->sys_ready && !h->member_status_on();       // (as in hipkkt_kkt_system_update)
        const int r = kkt_update_device(h, enqueue_only);
        h->host_upload_wait();
        return r;
    });
    if (rc != HIPKKT_OK) return rc;
    if (enqueue_only) h->sys_update_unread = true;
    return guarded([&]() { return sys_after_update(h); });
}

int hipkkt_selftest_handover(int variant, int pairs, int words, int rounds, int device, int64_t out[2])
{
    return guarded([&]() {
        if (variant < 0 || variant > 2 || pairs <= 0 || pairs > 96 || words <= 0 || rounds <= 0 || !out)
            throw ArgError("hipkkt_selftest_handover: bad argument");     // (<= 96 pairs: every workgroup resident, whatever else runs)
        HIP_CHECK(hipSetDevice(device < 0 ? 0 : device));
        DBuf<double> payload;
        DBuf<int> words_i;
        DBuf<int64_t> counts;
        payload.alloc((size_t)pairs * words);
        words_i.alloc((size_t)2 * pairs);
        counts.alloc(2);
        HIP_CHECK(hipMemset(payload.p, 0, payload.n * sizeof(double)));
        HIP_CHECK(hipMemset(words_i.p, 0, words_i.n * sizeof(int)));
        HIP_CHECK(hipMemset(counts.p, 0, 2 * sizeof(int64_t)));
        launch_handover_litmus(variant, payload.p, words_i.p, words_i.p + pairs, pairs, words, rounds,
                               reinterpret_cast<unsigned long long*>(counts.p), reinterpret_cast<unsigned long long*>(counts.p) + 1, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, counts.p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
        return HIPKKT_OK;
    });
}

int hipkkt_host_register(void* ptr, int64_t bytes)
{
    return guarded([&]() {
        if (!ptr || bytes <= 0) throw ArgError("hipkkt_host_register: bad argument");
        HIP_CHECK(hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault));
        return HIPKKT_OK;
    });
}
int hipkkt_host_unregister(void* ptr)
{
    return guarded([&]() {
        if (!ptr) throw ArgError("hipkkt_host_unregister: bad argument");
        HIP_CHECK(hipHostUnregister(ptr));
        return HIPKKT_OK;
    });
}

// ---- host-vector variants: the iterate, right-hand side and step live in host memory (DefaultVariables)
static double* sys_host_stage(hipkkt_kkt_t h)
{
    const size_t len = (size_t)h->K.n + 2 * (size_t)h->K.m;
    if (h->hst.n < 3 * len) { h->hst.alloc(3 * len); h->host_vars_valid = false; }
    return h->hst.p;
}

int hipkkt_kkt_system_update_host(hipkkt_kkt_t h, const double* s, const double* z)
{
    int rc = guarded([&]() {
        if (!h || (h->K.m && (!s || !z))) throw ArgError("hipkkt_kkt_system_update_host: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        const size_t bytes = (size_t)h->K.m * sizeof(double);
        if (bytes) {
            HIP_CHECK(hipMemcpyAsync(h->sbuf.p, s, bytes, hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(h->zbuf.p, z, bytes, hipMemcpyHostToDevice, h->stream));
        }
        return HIPKKT_OK;
    });
    if (rc != HIPKKT_OK) return rc;
    return hipkkt_kkt_system_update(h, h->sbuf.p, h->zbuf.p);
}

int hipkkt_kkt_system_solve_initial_point_host(hipkkt_kkt_t h, double* x, double* s, double* z)
{
    if (!h) { g_last_error = "null handle"; return HIPKKT_ERR_ARG; }
    const size_t n = (size_t)h->K.n, m = (size_t)h->K.m;
    double* d = nullptr;
    int rc = guarded([&]() {
        if ((n && !x) || (m && (!s || !z))) throw ArgError("hipkkt_kkt_system_solve_initial_point_host: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        d = sys_host_stage(h);
        return HIPKKT_OK;
    });
    if (rc != HIPKKT_OK) return rc;
    rc = hipkkt_kkt_system_solve_initial_point(h, d, d + n, d + n + m);
    if (rc != HIPKKT_OK) return rc;
    return guarded([&]() {
        if (n) HIP_CHECK(hipMemcpyAsync(x, d, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (m) HIP_CHECK(hipMemcpyAsync(s, d + n, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (m) HIP_CHECK(hipMemcpyAsync(z, d + n + m, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_system_solve_host(hipkkt_kkt_t h, double* lhs_x, double* lhs_s, double* lhs_z, double* lhs_tau_kappa,
                                 const double* rhs_x, const double* rhs_s, const double* rhs_z, double rhs_tau,
                                 double rhs_kappa, const double* var_x, const double* var_s, const double* var_z,
                                 double var_tau, double var_kappa, int steptype)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        const size_t n = (size_t)h->K.n, m = (size_t)h->K.m, len = n + 2 * m;
        const bool affine = steptype == 0;
        // (var_x = var_s = var_z = NULL: the variables uploaded by the previous call -- the combined step's are the affine step's)
        const bool reuse_vars = !var_x && !var_s && !var_z && h->host_vars_valid;
        if ((n && (!lhs_x || !rhs_x || (!var_x && !reuse_vars))) || (m && (!lhs_s || !lhs_z || !rhs_z || ((!var_s || !var_z) && !reuse_vars))) ||
            (m && !affine && !rhs_s) || !lhs_tau_kappa)
            throw ArgError("hipkkt_kkt_system_solve_host: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        double* d = sys_host_stage(h);
        double *dr = d, *dv = d + len, *dl = d + 2 * len;
        hipStream_t st = h->stream;
        auto up = [&](double* dst, const double* src, size_t k) {
            if (k && src) HIP_CHECK(hipMemcpyAsync(dst, src, k * sizeof(double), hipMemcpyHostToDevice, st));
        };
        up(dr, rhs_x, n); up(dr + n, affine ? nullptr : rhs_s, m); up(dr + n + m, rhs_z, m);
        if (!reuse_vars) { up(dv, var_x, n); up(dv + n, var_s, m); up(dv + n + m, var_z, m); h->host_vars_valid = true; }
        int rc = sys_solve_step(h, dl, dl + n, dl + n + m, lhs_tau_kappa, dr, dr + n, dr + n + m, rhs_tau, rhs_kappa,
                                dv, dv + n, dv + n + m, var_tau, var_kappa, steptype);
        if (rc != HIPKKT_OK) return rc;
        if (n) HIP_CHECK(hipMemcpyAsync(lhs_x, dl, n * sizeof(double), hipMemcpyDeviceToHost, st));
        if (m) HIP_CHECK(hipMemcpyAsync(lhs_s, dl + n, m * sizeof(double), hipMemcpyDeviceToHost, st));
        if (m) HIP_CHECK(hipMemcpyAsync(lhs_z, dl + n + m, m * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return HIPKKT_OK;
    });
}

// ------------------------------------------------------------------------------------------------
//  Ruiz equilibration of the problem data (data_equilibrate!, problemdata.jl:133-221) -- SURVEY.md 8 f4.
//  Stand-alone: runs before the KKT solver is built from the scaled (P, A).
// ------------------------------------------------------------------------------------------------
static void expand_csc(int64_t ncols, const int64_t* colptr, const int64_t* rowval, int base, std::vector<int>& row,
                       std::vector<int>& col)
{
    const int64_t nnz = colptr[ncols] - base;
    row.resize((size_t)nnz);
    col.resize((size_t)nnz);
    for (int64_t j = 0; j < ncols; ++j)
        for (int64_t q = colptr[j] - base; q < colptr[j + 1] - base; ++q) {
            row[(size_t)q] = (int)(rowval[q] - base);
            col[(size_t)q] = (int)j;
        }
}

int hipkkt_equilibrate(int64_t n, int64_t m, const int64_t* Pcolptr, const int64_t* Prowval, double* Pnzval,
                       const int64_t* Acolptr, const int64_t* Arowval, double* Anzval, double* q, double* b,
                       int64_t ncones, const int32_t* cone_kinds, const int64_t* cone_dims, int32_t max_iter,
                       double min_scaling, double max_scaling, double* d, double* e, double* c, int index_base,
                       int device)
{
    return guarded([&]() {
        if (n < 0 || m < 0 || !Pcolptr || !Acolptr || (n && (!q || !d)) || (m && (!b || !e)) || !c || max_iter < 0 ||
            ncones < 0 || (ncones && (!cone_kinds || !cone_dims)))
            throw ArgError("hipkkt_equilibrate: bad argument");
        hipkkt_settings st{};
        st.device = device;
        select_device(st);
        hipStream_t stream;
        HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } sg{stream};
        std::vector<int> prow, pcol, arow, acol;
        expand_csc(n, Pcolptr, Prowval, index_base, prow, pcol);
        expand_csc(n, Acolptr, Arowval, index_base, arow, acol);
        for (size_t j = 0; j < prow.size(); ++j)
            if (prow[j] < 0 || prow[j] >= n) throw ArgError("hipkkt_equilibrate: P row index out of range");
        for (size_t j = 0; j < arow.size(); ++j)
            if (arow[j] < 0 || arow[j] >= m) throw ArgError("hipkkt_equilibrate: A row index out of range");
        // cone layout (numel per cone: k(k+1)/2 for a PSD cone of side k)
        std::vector<int> ckind((size_t)ncones), coff((size_t)ncones), cnumel((size_t)ncones);
        int64_t off = 0;
        for (int64_t k = 0; k < ncones; ++k) {
            const int64_t dim = cone_dims[k];
            // (exponential and power cones take the default rectification, one scalar per cone: coneops_defaults.jl:32-44,
            // which k_equil_rectify applies to every kind >= 2)
            if (cone_kinds[k] < HIPKKT_CONE_ZERO || cone_kinds[k] > HIPKKT_CONE_GENPOW || dim < 0)
                throw ArgError("hipkkt_equilibrate: unknown cone kind or negative dimension");
            if ((cone_kinds[k] == HIPKKT_CONE_EXP || cone_kinds[k] == HIPKKT_CONE_POW) && dim != 3)
                throw ArgError("hipkkt_equilibrate: exponential and power cones have dimension 3");
            const int64_t ne = cone_kinds[k] == HIPKKT_CONE_PSD ? dim * (dim + 1) / 2 : dim;
            ckind[(size_t)k] = cone_kinds[k];
            coff[(size_t)k] = (int)off;
            cnumel[(size_t)k] = (int)ne;
            off += ne;
        }
        if (off != m) throw ArgError("hipkkt_equilibrate: cone dimensions do not add up to m");

        DBuf<int> dprow, dpcol, darow, dacol, dkind, doff, dnumel;
        dprow.upload(prow); dpcol.upload(pcol); darow.upload(arow); dacol.upload(acol);
        dkind.upload(ckind); doff.upload(coff); dnumel.upload(cnumel);
        DBuf<double> dP, dA, dq, db, dd, de, dw, ew, scal, partial;
        const size_t nnzP = prow.size(), nnzA = arow.size();
        dP.alloc(nnzP); dA.alloc(nnzA); dq.alloc((size_t)n); db.alloc((size_t)m);
        dd.alloc((size_t)n); de.alloc((size_t)m); dw.alloc((size_t)n); ew.alloc((size_t)m);
        scal.alloc(8); partial.alloc(512);
        if (nnzP) HIP_CHECK(hipMemcpyAsync(dP.p, Pnzval, nnzP * sizeof(double), hipMemcpyHostToDevice, stream));
        if (nnzA) HIP_CHECK(hipMemcpyAsync(dA.p, Anzval, nnzA * sizeof(double), hipMemcpyHostToDevice, stream));
        if (n) HIP_CHECK(hipMemcpyAsync(dq.p, q, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream));
        if (m) HIP_CHECK(hipMemcpyAsync(db.p, b, (size_t)m * sizeof(double), hipMemcpyHostToDevice, stream));
        std::vector<double> ones((size_t)std::max<int64_t>(std::max(n, m), 8), 1.0);
        if (n) HIP_CHECK(hipMemcpyAsync(dd.p, ones.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream));
        if (m) HIP_CHECK(hipMemcpyAsync(de.p, ones.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(scal.p, ones.data(), 8 * sizeof(double), hipMemcpyHostToDevice, stream));
        EquilDev E;
        E.n = (int)n; E.m = (int)m; E.nnzP = (int64_t)nnzP; E.nnzA = (int64_t)nnzA;
        E.Prow = dprow.p; E.Pcol = dpcol.p; E.Arow = darow.p; E.Acol = dacol.p;
        E.Pval = dP.p; E.Aval = dA.p; E.q = dq.p; E.b = db.p; E.d = dd.p; E.e = de.p; E.dwork = dw.p; E.ework = ew.p;
        E.scal = scal.p; E.partial = partial.p;
        for (int it = 0; it < max_iter; ++it) launch_equil_round(E, min_scaling, max_scaling, stream);
        if (max_iter > 0) launch_equil_rectify(E, dkind.p, doff.p, dnumel.p, nullptr, (int)ncones, stream);
        HIP_CHECK(hipGetLastError());
        if (nnzP) HIP_CHECK(hipMemcpyAsync(Pnzval, dP.p, nnzP * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (nnzA) HIP_CHECK(hipMemcpyAsync(Anzval, dA.p, nnzA * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (n) HIP_CHECK(hipMemcpyAsync(q, dq.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (m) HIP_CHECK(hipMemcpyAsync(b, db.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (n) HIP_CHECK(hipMemcpyAsync(d, dd.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (m) HIP_CHECK(hipMemcpyAsync(e, de.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(c, scal.p, sizeof(double), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return HIPKKT_OK;
    });
}

// _update_matrix (data_updating.jl:169-194): values <- cscale * L[row] * R[col] * values for a CSC matrix
int hipkkt_scale_matrix_values(int64_t nrows, int64_t ncols, const int64_t* colptr, const int64_t* rowval, double* nzval,
                               const double* lscale, const double* rscale, double cscale, int index_base, int device)
{
    return guarded([&]() {
        if (nrows < 0 || ncols < 0 || !colptr || !lscale || !rscale) throw ArgError("hipkkt_scale_matrix_values: bad argument");
        hipkkt_settings st{};
        st.device = device;
        select_device(st);
        std::vector<int> row, col;
        expand_csc(ncols, colptr, rowval, index_base, row, col);
        if (row.empty()) return HIPKKT_OK;
        if (!nzval) throw ArgError("hipkkt_scale_matrix_values: bad argument");
        for (int r : row) if (r < 0 || r >= nrows) throw ArgError("hipkkt_scale_matrix_values: row index out of range");
        DBuf<int> drow, dcol;
        drow.upload(row); dcol.upload(col);
        DBuf<double> v, L, R;
        v.alloc(row.size()); L.alloc((size_t)nrows); R.alloc((size_t)ncols);
        HIP_CHECK(hipMemcpy(v.p, nzval, row.size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(L.p, lscale, (size_t)nrows * sizeof(double), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(R.p, rscale, (size_t)ncols * sizeof(double), hipMemcpyHostToDevice));
        launch_lrscale(v.p, drow.p, dcol.p, (int64_t)row.size(), L.p, R.p, cscale, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(nzval, v.p, row.size() * sizeof(double), hipMemcpyDeviceToHost));
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_mul_Hs(hipkkt_kkt_t h, double* y, const double* x)
{
    return guarded([&]() {
        if (!h || !y || !x) throw ArgError("hipkkt_kkt_mul_Hs: bad argument");
        if (!h->scaling_valid) throw ArgError("mul_Hs needs a device-side scaling (hipkkt_kkt_update_from_sz)");
        HIP_CHECK(hipSetDevice(h->device));
        size_t bytes = (size_t)h->K.m * sizeof(double);
        HIP_CHECK(hipMemcpyAsync(h->sbuf.p, x, bytes, hipMemcpyHostToDevice, h->stream));
        launch_mul_Hs(h->cone_dev(), h->cone_state(), h->ybuf.p, h->sbuf.p, h->K.m, h->stream);
        HIP_CHECK(hipMemcpyAsync(y, h->ybuf.p, bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_get_pattern(hipkkt_kkt_t h, int64_t* colptr, int64_t* rowval)
{
    return guarded([&]() {
        if (!h || !colptr || !rowval) throw ArgError("hipkkt_kkt_get_pattern: bad argument");
        std::copy(h->K.colptr.begin(), h->K.colptr.end(), colptr);
        for (int64_t q = 0; q < h->K.nnzK; ++q) rowval[q] = h->K.rowval[q];
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_get_values(hipkkt_kkt_t h, double* nzval)
{
    return guarded([&]() {
        if (!h || !nzval) throw ArgError("hipkkt_kkt_get_values: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        HIP_CHECK(hipMemcpyAsync(nzval, h->Kval.p, (size_t)h->K.nnzK * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

// e = b - K_sym x through the launch functions and the SpmvDev of the solves (test infrastructure; hipkkt.h).  The CSR
// image is K's own (unpermuted) order, as the solves' work vectors are: the fill-reducing permutation lives inside the
// sweeps.  Only the many-column work buffers are written, and for route 1 the refinement state's scratch words, which
// every solve initialises before it reads them.
int hipkkt_kkt_get_residual(hipkkt_kkt_t h, int route, int64_t nrhs, const double* x, const double* b, double* e,
                            double* norm_e, double* norm_b)
{
    return guarded([&]() {
        if (!h || !x || !b || !norm_e || nrhs < 1 || nrhs > 65535 || route < 0 || route > 2)
            throw ArgError("hipkkt_kkt_get_residual: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        const int k = (int)nrhs, N = (int)h->K.N;
        if (route == 1 && !(kkt_partials_mode(h, k) && (k == 1 || k == 2 || k == 4)))
            throw ArgError("hipkkt_kkt_get_residual: route 1 (partials) needs no long rows and 1, 2 or 4 columns");
        if (route == 2 && h->nlong != 0) throw ArgError("hipkkt_kkt_get_residual: route 2 (row-major) needs no long rows");
        kkt_multi_reserve(h, (size_t)k);
        const SpmvDev A = kkt_spmv(h);                   // (after the reserve: it may move the long rows' partial sums)
        const size_t bytes = (size_t)N * k * sizeof(double);
        std::vector<double> hn(2 * (size_t)h->mcap, 0.0);
        const double* e_dev = h->mE.p;
        if (route == 2) {
            const int KP = (k + 15) & ~15;
            // column-major staging in the candidate buffer, as hipkkt_kkt_solve_multi does; all N rows are "x rows" here
            HIP_CHECK(hipMemcpyAsync(h->mC.p, x, bytes, hipMemcpyHostToDevice, h->stream));
            launch_pack_rhs_rm(h->mX.p, h->mC.p, nullptr, N, 0, 0, k, KP, h->stream);
            HIP_CHECK(hipMemcpyAsync(h->mC.p, b, bytes, hipMemcpyHostToDevice, h->stream));
            launch_pack_rhs_rm(h->mB.p, h->mC.p, nullptr, N, 0, 0, k, KP, h->stream);
            launch_residual_rm(A, h->mB.p, h->mX.p, h->mE.p, h->mpartial.p, h->mnorms.p, h->mnorms.p + KP, KP, h->stream);
            launch_unpack_lhs_rm(h->mC.p, nullptr, h->mE.p, N, 0, k, KP, h->stream);
            e_dev = h->mC.p;
            HIP_CHECK(hipMemcpyAsync(hn.data(), h->mnorms.p, 2 * (size_t)KP * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIP_CHECK(hipStreamSynchronize(h->stream));
            for (int c = 0; c < k; ++c) { norm_e[c] = hn[c]; if (norm_b) norm_b[c] = hn[KP + c]; }
        } else {
            const int64_t ld = N;
            HIP_CHECK(hipMemcpyAsync(h->mX.p, x, bytes, hipMemcpyHostToDevice, h->stream));
            HIP_CHECK(hipMemcpyAsync(h->mB.p, b, bytes, hipMemcpyHostToDevice, h->stream));
            if (route == 0) {
                launch_residual(A, h->Kval.p, h->mB.p, h->mX.p, h->mE.p, h->mpartial.p, h->mnorms.p, h->stream, k, ld);
                launch_norm_inf(h->mB.p, N, h->mpartial.p, h->mnorms.p + k, h->stream, k, ld);
                HIP_CHECK(hipMemcpyAsync(hn.data(), h->mnorms.p, 2 * (size_t)k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            } else {
                // what kkt_solve_core enqueues ahead of a solve's first decision (kkt_enqueue_refine_error + kkt_launch_ir
                // with r = 0): the partial maxima stay un-finished, ||b|| rides along, k_ir_round reduces both
                const hipkkt_settings& st = h->st;
                const IrNorms nm = kkt_ir_norms(h, k);
                launch_residual(A, h->Kval.p, h->mB.p, h->mX.p, h->mE.p, h->mpartial.p, nullptr, h->stream, k,
                                k > 1 ? ld : 0, nullptr, nullptr, nm.normb);
                IrPartials Q;
                Q.np = residual_grid(A) + 1;
                Q.e0 = h->mpartial.p;
                Q.b0 = Q.e0 + (size_t)k * Q.np;
                launch_ir_round(h->ir_state, h->ir_stride, 0, true, nm.norme0, nm.normb, nm.cand, nullptr, h->mX.p, h->mC.p, N, k,
                                st.iterative_refinement_abstol, st.iterative_refinement_reltol, st.iterative_refinement_stop_ratio,
                                std::max(st.iterative_refinement_max_iter, 0), h->ir_readback, nullptr, h->stream, Q);
                HIP_CHECK(hipMemcpyAsync(hn.data(), nm.norme0, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
                HIP_CHECK(hipMemcpyAsync(hn.data() + k, nm.normb, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            }
            HIP_CHECK(hipStreamSynchronize(h->stream));
            for (int c = 0; c < k; ++c) { norm_e[c] = hn[c]; if (norm_b) norm_b[c] = hn[k + c]; }
        }
        if (e) HIP_CHECK(hipMemcpyAsync(e, e_dev, bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_get_maps(hipkkt_kkt_t h, int64_t* mapP, int64_t* mapA, int64_t* mapHs, int64_t* map_diag,
                        int64_t* mapU, int64_t* mapV, int64_t* mapD, int64_t* dsigns)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        auto cp = [](const std::vector<int>& v, int64_t* o) { if (o) for (size_t i = 0; i < v.size(); ++i) o[i] = v[i]; };
        cp(h->K.mapP, mapP); cp(h->K.mapA, mapA); cp(h->K.mapHs, mapHs); cp(h->K.map_diag, map_diag);
        cp(h->K.mapU, mapU); cp(h->K.mapV, mapV); cp(h->K.mapD, mapD); cp(h->K.dsigns, dsigns);
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_get_perm(hipkkt_kkt_t h, int64_t* perm)
{
    return guarded([&]() {
        if (!h || !perm) throw ArgError("hipkkt_kkt_get_perm: bad argument");
        for (int i = 0; i < h->K.N; ++i) perm[i] = h->eng->S.perm[i];
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_get_Hs(hipkkt_kkt_t h, double* Hs)
{
    return guarded([&]() {
        if (!h || (h->K.nHs && !Hs)) throw ArgError("hipkkt_kkt_get_Hs: bad argument");
        HIP_CHECK(hipSetDevice(h->device));
        if (h->K.nHs) HIP_CHECK(hipMemcpyAsync(Hs, h->Hs.p, (size_t)h->K.nHs * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_get_scaling(hipkkt_kkt_t h, double* lambda, double* psd_R, double* psd_Rinv)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        if (!h->scaling_valid) throw ArgError("hipkkt_kkt_get_scaling needs a device-side scaling (hipkkt_kkt_update_from_sz)");
        HIP_CHECK(hipSetDevice(h->device));
        if (lambda && h->K.m) HIP_CHECK(hipMemcpyAsync(lambda, h->lam.p, (size_t)h->K.m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (psd_R && h->psdR.n) HIP_CHECK(hipMemcpyAsync(psd_R, h->psdR.p, h->psdR.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (psd_Rinv && h->psdRinv.n) HIP_CHECK(hipMemcpyAsync(psd_Rinv, h->psdRinv.p, h->psdRinv.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_get_scaling_w(hipkkt_kkt_t h, double* w, double* eta)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        if (!h->scaling_valid) throw ArgError("hipkkt_kkt_get_scaling_w needs a device-side scaling (hipkkt_kkt_update_from_sz)");
        HIP_CHECK(hipSetDevice(h->device));
        if (w && h->K.m) HIP_CHECK(hipMemcpyAsync(w, h->w.p, (size_t)h->K.m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (eta && h->eta.n) HIP_CHECK(hipMemcpyAsync(eta, h->eta.p, h->eta.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_set_nonsymmetric_scaling(hipkkt_kkt_t h, int strategy, double mu)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        if (strategy != HIPKKT_SCALING_PRIMAL_DUAL && strategy != HIPKKT_SCALING_DUAL)
            throw ArgError("hipkkt_kkt_set_nonsymmetric_scaling: strategy must be PRIMAL_DUAL (0) or DUAL (1)");
        if (h->K.nnonsym == 0 && h->K.ngenpow == 0) return HIPKKT_OK;
        h->ns_strategy = strategy;
        h->ns_mu = mu;
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_get_nonsymmetric(hipkkt_kkt_t h, double* grad, double* H_dual)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        const size_t nn = (size_t)h->K.nnonsym;
        if (nn == 0) return HIPKKT_OK;
        if (!h->scaling_valid) throw ArgError("hipkkt_kkt_get_nonsymmetric needs a device-side scaling (hipkkt_kkt_update_from_sz)");
        HIP_CHECK(hipSetDevice(h->device));
        if (grad) HIP_CHECK(hipMemcpyAsync(grad, h->ns_grad.p, 3 * nn * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (H_dual) HIP_CHECK(hipMemcpyAsync(H_dual, h->ns_H.p, 9 * nn * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_get_genpow(hipkkt_kkt_t h, double* grad, double* d, double* p, double* q, double* r)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        const KKTAssembly& K = h->K;
        if (K.ngenpow == 0) return HIPKKT_OK;
        if (!h->scaling_valid) throw ArgError("hipkkt_kkt_get_genpow needs a device-side scaling (hipkkt_kkt_update_from_sz)");
        HIP_CHECK(hipSetDevice(h->device));
        const size_t gl = (size_t)K.genpow_len;
        if (grad) HIP_CHECK(hipMemcpyAsync(grad, h->gp_grad.p, gl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (d) HIP_CHECK(hipMemcpyAsync(d, h->gp_d.p, gl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (p) HIP_CHECK(hipMemcpyAsync(p, h->gp_p.p, gl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        std::vector<double> qr;
        if (q || r) {
            qr.resize(gl);
            HIP_CHECK(hipMemcpyAsync(qr.data(), h->gp_qr.p, gl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (q || r)
            for (const ConeInfo& ci : K.cones) {
                if (ci.kind != HIPKKT_CONE_GENPOW) continue;
                if (q) std::copy(qr.begin() + ci.gpoff, qr.begin() + ci.gpoff + ci.dim1, q + ci.gqoff);
                if (r) std::copy(qr.begin() + ci.gpoff + ci.dim1, qr.begin() + ci.gpoff + ci.numel, r + ci.groff);
            }
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_get_genpow_maps(hipkkt_kkt_t h, int64_t* map_p, int64_t* map_q, int64_t* map_r, int64_t* map_D)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        auto cp = [](const std::vector<int>& v, int64_t* dst) { if (dst) for (size_t i = 0; i < v.size(); ++i) dst[i] = v[i]; };
        cp(h->K.mapGP_p, map_p); cp(h->K.mapGP_q, map_q); cp(h->K.mapGP_r, map_r); cp(h->K.mapGP_D, map_D);
        return HIPKKT_OK;
    });
}

double hipkkt_kkt_last_regularizer(hipkkt_kkt_t h) { return h ? h->last_eps : 0.0; }
int64_t hipkkt_kkt_last_ir_iterations(hipkkt_kkt_t h) { return h ? h->last_ir : 0; }

int hipkkt_kkt_set_stream(hipkkt_kkt_t h, void* stream)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        HIP_CHECK(hipSetDevice(h->device));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        if (h->own_stream && h->stream) HIP_CHECK(hipStreamDestroy(h->stream));
        h->stream = (hipStream_t)stream;
        h->own_stream = false;
        h->eng->stream = h->stream;
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_synchronize(hipkkt_kkt_t h)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        HIP_CHECK(hipSetDevice(h->device));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_profile_enable(hipkkt_kkt_t h, int enable)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        h->prof.resolve();
        h->prof.enabled = enable != 0;
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_profile_reset(hipkkt_kkt_t h)
{
    return guarded([&]() {
        if (!h) throw ArgError("null handle");
        h->prof.resolve();
        h->prof.acc = hipkkt_profile{};
        return HIPKKT_OK;
    });
}

int hipkkt_kkt_profile_get(hipkkt_kkt_t h, hipkkt_profile* out)
{
    return guarded([&]() {
        if (!h || !out) throw ArgError("hipkkt_kkt_profile_get: bad argument");
        h->prof.resolve();
        *out = h->prof.acc;
        out->overlap_fallbacks = h->eng->n_ov_fallbacks;
        out->top_fallbacks = h->eng->n_top_fallbacks;
        out->overlap_deferrals = h->eng->n_ov_busy;
        out->top_deferrals = h->eng->n_top_busy;
        return HIPKKT_OK;
    });
}

}  // extern "C"
