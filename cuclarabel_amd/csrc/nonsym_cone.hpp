// The scalar pieces of the exponential and the power cone that more than one translation unit needs: the scaling kernel
// (kernels.hip) and the step kernels between the solves (step_kernels.hip).  Device-only, one thread per cone; every
// including file is compiled without FMA contraction (the reference restated term for term, see kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace hipkkt {

__device__ inline double ns_logsafe(double v) { return v > 0.0 ? log(v) : -HUGE_VAL; }

__device__ inline double ns_wright_omega(double z)
{
    if (!(z >= 0.0)) return NAN;                   // the reference throws; reached only from outside the primal cone
    double w;
    if (z < 1.0 + 3.14159265358979323846) {
        const double zm1 = z - 1.0;
        double p = zm1;
        w = 1.0 + 0.5 * p;
        p *= zm1;
        w += (1.0 / 16.0) * p;
        p *= zm1;
        w -= (1.0 / 192.0) * p;
        p *= zm1;
        w -= (1.0 / 3072.0) * p;
        p *= zm1;
        w += (13.0 / 61440.0) * p;
    } else {
        const double logz = ns_logsafe(z);
        const double zinv = 1.0 / z;
        w = z - logz;
        double q = logz * zinv;
        w += q;
        q *= zinv;
        w += q * (logz / 2.0 - 1.0);
        // (:451 of the reference forms q*zinv and drops it: the cubic term is weighted by log(z)/z^2 there, and here)
        w += q * (logz * logz / 3.0 - (3.0 / 2.0) * logz + 1.0);
    }
    double r = z - w - ns_logsafe(w);
    for (int i = 0; i < 2; ++i) {
        const double wp1 = w + 1.0;
        const double t = wp1 * (wp1 + (2.0 * r) / 3.0);
        w *= 1.0 + (r / wp1) * (t - 0.5 * r) / (t - r);
        r = (2.0 * w * w - 8.0 * w - 1.0) / (72.0 * (wp1 * wp1 * wp1 * wp1 * wp1 * wp1)) * r * r * r * r;
    }
    return w;
}

__device__ inline double ns_newton_raphson_powcone(double s3, double phi, double a)
{
    const double eps = 2.220446049250313e-16, sqrt_eps = 1.4901161193847656e-08;
    double x = -1.0 / s3 + (2.0 * s3 + sqrt(phi * phi / s3 / s3 + 3.0 * phi)) / (phi - s3 * s3);
    const double t0 = -2.0 * a * ns_logsafe(a) - 2.0 * (1.0 - a) * ns_logsafe(1.0 - a);
    auto f0 = [&](double y) {
        const double t1 = y * y, t2 = 2.0 * y / s3;
        return 2.0 * a * ns_logsafe(2.0 * a * t1 + (1.0 + a) * t2) + 2.0 * (1.0 - a) * ns_logsafe(2.0 * (1.0 - a) * t1 + (2.0 - a) * t2)
               - ns_logsafe(phi) - ns_logsafe(t1 + t2) - 2.0 * ns_logsafe(t2) + t0;
    };
    // the one-sided iteration needs f0(x0) > 0; the reference's x0 lies right of the root for alpha away from 1/2 and its
    // iteration then halts at once (ipm.py: _newton_raphson_powcone has the figures).  f0 -> +Inf as x -> 0+: halve.
    for (int k = 0; k < 64 && !(f0(x) > 0.0); ++k) x *= 0.5;
    for (int iter = 0; iter < 100; ++iter) {
        const double t1 = x * x, t2 = x * 2.0 / s3;
        const double dfdx = 2.0 * a * a / (a * x + (1.0 + a) / s3) + 2.0 * (1.0 - a) * (1.0 - a) / ((1.0 - a) * x + (2.0 - a) / s3)
                            - 2.0 * (x + 1.0 / s3) / (t1 + t2);
        const double dx = -f0(x) / dfdx;
        if ((dx < eps) || (fabs(dx / x) < sqrt_eps) || (fabs(dfdx) < eps)) break;
        x += dx;
    }
    return x;
}

// grad f*(z) -> g, H*(z) -> H (row-major 3 x 3); returns whether z is strictly inside the dual cone
__device__ inline bool ns_exp_dual_grad_H(const double* z, double* g, double* H)
{
    const double l = ns_logsafe(-z[2] / z[0]);
    const double r = -z[0] * l - z[0] + z[1];
    const double c2 = 1.0 / r;
    g[0] = c2 * l - 1.0 / z[0];
    g[1] = -c2;
    g[2] = (c2 * z[0] - 1.0) / z[2];
    H[0] = (r * r - z[0] * r + l * l * z[0] * z[0]) / (r * z[0] * z[0] * r);
    H[1] = H[3] = -l / (r * r);
    H[4] = 1.0 / (r * r);
    H[2] = H[6] = (z[1] - z[0]) / (r * r * z[2]);
    H[5] = H[7] = -z[0] / (r * r * z[2]);
    H[8] = (r * r - z[0] * r + z[0] * z[0]) / (r * r * z[2] * z[2]);
    // is_dual_feasible (:269-281): res = z2 - z1 - z1 log(-z3/z1) is r in the order the reference sums it there
    return z[2] > 0.0 && z[0] < 0.0 && (z[1] - z[0] - z[0] * l) > 0.0;
}
__device__ inline void ns_exp_gradient_primal(const double* s, double* g)
{
    const double w = ns_wright_omega(1.0 - s[0] / s[1] - ns_logsafe(s[1] / s[2]));
    g[0] = 1.0 / ((w - 1.0) * s[1]);
    g[1] = g[0] + g[0] * ns_logsafe(w * s[1] / s[2]) - 1.0 / s[1];
    g[2] = w / ((1.0 - w) * s[2]);
}
__device__ inline bool ns_pow_dual_grad_H(const double* z, double a, double* g, double* H)
{
    const double phi = pow(z[0] / a, 2.0 * a) * pow(z[1] / (1.0 - a), 2.0 - 2.0 * a);
    const double psi = phi - z[2] * z[2];
    const double g0 = 2.0 * a * phi / (z[0] * psi), g1 = 2.0 * (1.0 - a) * phi / (z[1] * psi), g2 = -2.0 * z[2] / psi;
    H[0] = g0 * g0 - 2.0 * a * (2.0 * a - 1.0) * phi / (z[0] * z[0] * psi) + (1.0 - a) / (z[0] * z[0]);
    H[1] = H[3] = g0 * g1 - 4.0 * a * (1.0 - a) * phi / (z[0] * z[1] * psi);
    H[4] = g1 * g1 - 2.0 * (1.0 - a) * (1.0 - 2.0 * a) * phi / (z[1] * z[1] * psi) + a / (z[1] * z[1]);
    H[2] = H[6] = g0 * g2;
    H[5] = H[7] = g1 * g2;
    H[8] = g2 * g2 + 2.0 / psi;
    g[0] = -2.0 * a * phi / (z[0] * psi) - (1.0 - a) / z[0];
    g[1] = -2.0 * (1.0 - a) * phi / (z[1] * psi) - a / z[1];
    g[2] = 2.0 * z[2] / psi;
    // is_dual_feasible (:272-284)
    if (!(z[0] > 0.0 && z[1] > 0.0)) return false;
    return exp(2.0 * a * ns_logsafe(z[0] / a) + 2.0 * (1.0 - a) * ns_logsafe(z[1] / (1.0 - a))) - z[2] * z[2] > 0.0;
}
__device__ inline void ns_pow_gradient_primal(const double* s, double a, double* g)
{
    const double phi = pow(s[0], 2.0 * a) * pow(s[1], 2.0 - 2.0 * a);
    const double abs_s = fabs(s[2]);
    if (abs_s > 2.220446049250313e-16) {
        g[2] = ns_newton_raphson_powcone(abs_s, phi, a);
        if (s[2] < 0.0) g[2] = -g[2];
        g[0] = -(a * g[2] * s[2] + 1.0 + a) / s[0];
        g[1] = -((1.0 - a) * g[2] * s[2] + 2.0 - a) / s[1];
    } else {
        g[2] = 0.0;
        g[0] = -(1.0 + a) / s[0];
        g[1] = -(2.0 - a) / s[1];
    }
}

}  // namespace hipkkt
