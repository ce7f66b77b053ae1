// Device functions that the whole-handle refinement kernels (kernels.hip: k_residual, k_ir_round) and the member-segmented
// ones (batch_kernels.hip) share, so that both compute the same bits and take the same decisions.
#pragma once
#include "kernels.hpp"
#include <cmath>

namespace hipkkt {

// One row of K x in the residual e = b - K_sym x (kktsolver_directldl.jl:455-466): G lanes share the row, lane `sub` takes
// the entries q0 + sub, q0 + sub + G, ... in that order, and the lanes meet in a fixed shuffle tree; lane 0 of the group
// ends with the sum.  Every lane of a group must arrive here with the same row.
template <int G, int NC>
__device__ inline void residual_row_dot(const SpmvDev& A, const double* __restrict__ K, const double* __restrict__ x, int64_t ld,
                                        int64_t q0, int64_t q1, int sub, double (&acc)[NC])
{
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0;
    for (int64_t q = q0 + sub; q < q1; q += G) {
        const double a = A.val ? A.val[q] : K[A.vmap[q]];
        const int j = A.col[q];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = fma(a, x[c * ld + j], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) acc[c] += __shfl_down(acc[c], o, G);
    }
}

// The refinement loop's decisions (kktsolver_directldl.jl:389-449) on a state {active: the reference's loop would go on,
// rounds done, bad: a residual norm was not finite, norme: residual norm of the accepted solution}.
// The state before the first round, from the first solve's residual norm:
__device__ inline void ir_initial(double norme0, double normb, double abstol, double reltol, int max_iter,
                                  double& active, double& rounds, double& bad, double& norme)
{
    norme = norme0;
    bad = isfinite(norme) ? 0.0 : 1.0;
    rounds = 0.0;
    active = (bad == 0.0 && max_iter > 0 && !(norme <= abstol + reltol * normb)) ? 1.0 : 0.0;
}
// Round r >= 1 of an active state has produced a candidate whose residual norm is cand: the accept / stop rule.  Returns
// whether the candidate becomes the solution.
__device__ inline bool ir_apply_rule(double cand, int r, int max_iter, double abstol, double reltol, double stop_ratio, double normb,
                                     double& active, double& rounds, double& bad, double& norme)
{
    bool accept = false;
    rounds += 1.0;
    if (!isfinite(cand)) {                      // :429: return is_success = false
        bad = 1.0; active = 0.0;
    } else {
        const double ratio = norme / cand;      // :437-446
        if (ratio < stop_ratio) { accept = ratio > 1.0; active = 0.0; }
        else accept = true;
        if (accept) norme = cand;
        // the head of the next iteration (:407-417): tolerance met, or max_iter rounds done
        if (active != 0.0 && (r >= max_iter || norme <= abstol + reltol * normb)) active = 0.0;
    }
    return accept;
}

}  // namespace hipkkt
