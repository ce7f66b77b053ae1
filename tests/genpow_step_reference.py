"""Extended-precision reference for the cone operations between the solves on cone lists that hold generalized power
cones (TEST INFRASTRUCTURE), built on tests/genpow_reference.py (the dual barrier AS WRITTEN, differentiated by mpmath in
60 digits) and, for the other six cone kinds of a mixed list, on tests/nonsym_step_reference.py.

    unit start        sqrt(1 + alpha_i) on the first dim1 rows, 0 behind (sqrt is correctly rounded: numpy's bits)
    affine d.s        a copy of s
    combined d.s      s + sigma_mu grad f*(z), grad by genpow_reference.mp_grad (no higher-order correction)
    barrier           f*(z') + f(s') at z' = fl(z + alpha dz), s' = fl(s + alpha ds), f(s) = -f*(-g) - (dim1 + 1).  The
                      candidate g is built from a 60-digit root of the cone's one-dimensional equation and then VERIFIED,
                      not trusted: ||grad f*(-g) + s|| <= 1e-40 ||s||, the gradient by differentiating the barrier as
                      written -- coordinate by coordinate on cones of up to SMALL_NUMEL rows, along e_i for a handful of
                      sampled coordinates and along two random directions on larger ones.
    step length       the composite rule restated sequentially over the fp64 classes of cuclarabel_amd/ipm.py
                      (nonsym_step_reference.step_length_sequential runs over ipm._GenPow unchanged)

Bound of a generalized power cone's barrier term:

    BOUND_C u (|term| + k_z + k_s) + gamma_dim * sum |summands|

k_z = (phi + ||w||^2) / (phi - ||w||^2) at z' (phi = prod (z_i / alpha_i)^(2 alpha_i)), k_s the same at s' (phi = prod
s_i^(2 alpha_i)): what the logarithm of the cancelling difference loses.  The summands are the terms of every sum the
barrier forms: 2 alpha_i log(z_i / alpha_i), (1 - alpha_i) log z_i and log zeta at z', the same three at -g, and
dim1 + 1; gamma_dim covers adding them in any order.

BOUND_C was FIXED BY MEASUREMENT on the CPU (tests/test_genpow_step_reference_host.py prints the ratio under -s): the
worst distance of ipm._GenPow.compute_barrier from the mpmath value over exactly the points the GPU test uses, in units
of the bound with C = 1 (its gamma part included), rounded up to the next power of two, at least 1:

    quantity                             measured worst (numpy class)     C
    bar_gp   barrier term                    0.245                        1
    ds_gp    combined d.s row                1.468                        2

(ds_gp: |row - (s_i + sigma_mu grad_i)| in units of u (|s_i| + |sigma_mu| k_z |grad_i|), small shapes.)  The host test
asserts the numpy class stays within C; the device gets DEVICE_FACTOR = 4 times that.

Step length.  A binding case puts the ray's exit point at a0 step^(j + 1/2), half a backtracking step away from the two
values the search visits around it (found by bisection over the fp64 class's test, then the direction is rescaled),
j in {0, 1, 5}.  A case is EXCLUDED where a feasibility residual at a visited alpha lies within
FEAS_C u (1 + dim) (phi (1 + sum |2 alpha_i log v_i|) + ||w||^2) of zero; at most 5 % may be (with the exits half a
step away: none)."""
import math

import numpy as np
import mpmath as mp

from cuclarabel_amd import ipm
from cuclarabel_amd.cones import (ZeroConeT, NonnegativeConeT, SecondOrderConeT, PSDTriangleConeT, ExponentialConeT,
                                  PowerConeT, GenPowerConeT)
from tests import genpow_reference as gr
from tests import nonsymmetric_reference as nr
from tests import nonsym_step_reference as ns

U, DEVICE_FACTOR, FEAS_C, SQRT_EPS = ns.U, ns.DEVICE_FACTOR, ns.FEAS_C, ns.SQRT_EPS
BARRIER_ALPHAS, BACKTRACK_STEP, ALPHA_MIN = ns.BARRIER_ALPHAS, ns.BACKTRACK_STEP, ns.ALPHA_MIN
SMALL_NUMEL = 8                                          # up to here the gradient is checked coordinate by coordinate
VERIFY_TOL = mp.mpf(10) ** -40

NUMPY_WORST = dict(bar_gp=0.245, ds_gp=1.468)
BOUND_C = dict(bar_gp=1.0, ds_gp=2.0)


def is_gp(spec):
    return isinstance(spec, GenPowerConeT)


# ------------------------------------------------------------------------------------------
#  the cone lists both test files share
# ------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (2, 1), (1, 63), (63, 1), (64, 1), (1, 64), (65, 2),       # wave edges
          (200, 312), (256, 257),                                           # kGenPowWaveMax = 512 on both sides
          (10, 600), (300, 800))                                            # workgroup walks of 3 and 5 strides
FIVE = ((2, 1), (1, 3), (3, 2), (2, 5), (7, 4))                             # a partly filled workgroup of four waves
LISTS = tuple(f"{a}x{b}" for a, b in SHAPES) + ("five", "mixed")


def _list(name, rng):
    if name == "five":
        return [gr.random_spec(rng, a, b) for a, b in FIVE]
    if name == "mixed":
        return [SecondOrderConeT(6), gr.random_spec(rng, 2, 2), NonnegativeConeT(3), ExponentialConeT(),
                GenPowerConeT([1.0], 1), PSDTriangleConeT(8), PowerConeT(0.4), SecondOrderConeT(3),
                gr.random_spec(rng, 3, 4), ZeroConeT(2)]
    a, b = (int(t) for t in name.split("x"))
    return [gr.random_spec(rng, a, b)]


class Case:
    """cones, an interior (s, z) and a step (dz, ds) short enough that BARRIER_ALPHAS stay interior"""

    def __init__(self, name, seed=1):
        rng = np.random.default_rng([seed, LISTS.index(name), 9])
        self.name, self.cones = name, _list(name, rng)
        self.m = sum(c.numel for c in self.cones)
        self.off = ns.offsets(self.cones)
        s, z = np.zeros(self.m), np.zeros(self.m)
        dz, ds = 0.3 * rng.normal(size=self.m), 0.3 * rng.normal(size=self.m)
        for c, o in zip(self.cones, self.off):
            r = slice(o, o + c.numel)
            if isinstance(c, ZeroConeT):
                z[r] = rng.normal(size=c.numel)
            elif isinstance(c, NonnegativeConeT):
                s[r], z[r] = np.exp(rng.normal(size=c.numel)), np.exp(rng.normal(size=c.numel))
            elif isinstance(c, SecondOrderConeT):
                for v in (s, z):
                    t = rng.normal(size=c.numel)
                    t[0] = np.linalg.norm(t[1:]) + np.exp(rng.normal())
                    v[r] = t
            elif isinstance(c, PSDTriangleConeT):
                for v in (s, z):
                    G = rng.normal(size=(c.dim, c.dim))
                    v[r] = ipm._mat_to_svec(G @ G.T + 0.5 * np.eye(c.dim))
            elif is_gp(c):
                s[r], z[r] = gr.random_interior_pair(c, rng)
                dz[r] /= math.sqrt(c.numel)                               # (||alpha dz|| stays a small fraction of the margin)
                ds[r] /= math.sqrt(c.numel)
            else:
                s[r], z[r] = nr.random_interior_pair(c, rng)
        self.s, self.z, self.dz, self.ds = s, z, dz, ds
        self.mu = float(s @ z) / max(1, sum(ipm._make_cones([c])[0].degree for c in self.cones))
        self.scal = {}

    def gp(self):
        return [(c, o) for c, o in zip(self.cones, self.off) if is_gp(c)]

    def gp_rows(self):
        rows = np.zeros(self.m, bool)
        for c, o in self.gp():
            rows[o:o + c.numel] = True
        return rows

    def twin(self):
        """the other cones alone (a list the _ns entry points take), with their rows"""
        return [c for c in self.cones if not is_gp(c)], ~self.gp_rows()

    def permuted(self, order):
        """the same cones in another order, the rows moved with them"""
        out = Case.__new__(Case)
        out.name, out.cones = self.name, [self.cones[i] for i in order]
        rows = np.concatenate([np.arange(self.off[i], self.off[i] + self.cones[i].numel) for i in order]).astype(int)
        out.m, out.off = self.m, ns.offsets(out.cones)
        out.s, out.z, out.dz, out.ds = self.s[rows], self.z[rows], self.dz[rows], self.ds[rows]
        out.mu, out.scal = self.mu, dict(self.scal)
        return out


# ------------------------------------------------------------------------------------------
#  unit start, d.s rows
# ------------------------------------------------------------------------------------------
def unit_start(spec):
    return np.concatenate([np.sqrt(1.0 + np.array(spec.alpha, dtype=np.float64)), np.zeros(spec.dim2)])


def _phi_norm(spec, v, scaled):
    """(phi, ||w||^2, sum |2 alpha_i log(v_i [/ alpha_i])|) at the fp64 point v, in mpmath; None where a v_i <= 0"""
    a = [mp.mpf(t) for t in spec.alpha]
    d1 = len(a)
    v = [mp.mpf(float(t)) for t in v]
    if not all(t > 0 for t in v[:d1]):
        return None
    logs = [2 * a[i] * mp.log(v[i] / a[i] if scaled else v[i]) for i in range(d1)]
    return mp.exp(sum(logs)), sum(t * t for t in v[d1:]), sum(abs(t) for t in logs)


def cancellation(spec, v, scaled):
    """(phi + ||w||^2) / (phi - ||w||^2), inf outside"""
    t = _phi_norm(spec, v, scaled)
    if t is None or not t[0] - t[1] > 0:
        return math.inf
    return float((t[0] + t[1]) / (t[0] - t[1]))


def ds_rows(spec, s, z, sigma_mu):
    """(value, magnitude) of the cone's combined d.s rows, s + sigma_mu mp_grad; the bound is C u magnitude"""
    g = gr.mp_grad(spec, z)
    kz = cancellation(spec, z, True)
    val = np.array([float(mp.mpf(float(s[i])) + mp.mpf(float(sigma_mu)) * g[i]) for i in range(len(s))])
    mag = np.array([abs(float(s[i])) + abs(float(sigma_mu)) * kz * abs(float(g[i])) for i in range(len(s))])
    return val, mag


def ds_numpy(spec, s, z, mu, sigma_mu):
    c = ipm._make_cones([spec])[0]
    c.update_scaling(np.array(s, float), np.array(z, float), mu, ipm.DUAL)
    return c.affine_ds(np.array(s, float)) + c.combined_ds_shift(None, None, sigma_mu)


# ------------------------------------------------------------------------------------------
#  barrier
# ------------------------------------------------------------------------------------------
def _mp_derivative(f, y, v):
    """grad f(y) . v by differentiating t -> f(y + t v), y and v mpmath"""
    n = len(y)
    return mp.diff(lambda t: f(*[y[i] + t * v[i] for i in range(n)]), 0)


def mp_primal_gradient(spec, sp_, rng=None):
    """g(s) with grad f*(-g) = -s: the candidate from a 60-digit root of the one-dimensional equation
    (coneops_genpowcone.jl:393-472), then verified against the derivative of the barrier as written"""
    a = [mp.mpf(t) for t in spec.alpha]
    d1, n = len(a), len(sp_)
    s = [mp.mpf(float(t)) for t in sp_]
    p, r = s[:d1], s[d1:]
    nrm = mp.sqrt(sum(t * t for t in r))
    if nrm == 0:
        g = [-(1 + a[i]) / p[i] for i in range(d1)] + [mp.mpf(0)] * (n - d1)
    else:
        def f0(x):
            return -mp.log(2 * x / nrm + x * x) + sum(2 * a[i] * (mp.log(x * nrm + (1 + a[i]) / a[i]) - mp.log(p[i])) for i in range(d1))
        c = ipm._make_cones([spec])[0]
        with np.errstate(all="ignore"):
            g0 = c.gradient_primal(np.asarray(sp_, float))
        x0 = float(np.linalg.norm(g0[d1:]))                               # g1 of the fp64 class: a starting point only
        x = mp.findroot(f0, mp.mpf(x0), tol=mp.mpf(10) ** -110, maxsteps=100, verify=False)
        g = [-(1 + a[i] + a[i] * x * nrm) / p[i] for i in range(d1)] + [x * t / nrm for t in r]
    # ---- verification
    f = gr.dual_barrier(spec)
    y = [-t for t in g]
    snorm = mp.sqrt(sum(t * t for t in s))
    if n <= SMALL_NUMEL:
        res = [_mp_derivative(f, y, [mp.mpf(1 if i == k else 0) for i in range(n)]) + s[k] for k in range(n)]
        assert mp.sqrt(sum(t * t for t in res)) <= VERIFY_TOL * snorm, ("g(s) is not the conjugate gradient", spec, res)
    else:
        rng = rng or np.random.default_rng(n)
        dirs = []
        for k in sorted({0, d1 - 1, d1, n - 1, int(rng.integers(n))}):
            dirs.append([mp.mpf(1 if i == k else 0) for i in range(n)])
        for _ in range(2):
            dirs.append([mp.mpf(float(t)) for t in rng.normal(size=n)])
        for v in dirs:
            vnorm = mp.sqrt(sum(t * t for t in v))
            res = _mp_derivative(f, y, v) + sum(s[i] * v[i] for i in range(n))
            assert abs(res) <= VERIFY_TOL * snorm * vnorm, ("g(s) is not the conjugate gradient", spec.dim1, spec.dim2, res)
    return g


_BAR_CACHE = {}


def gp_barrier_term(spec, zp, sp_):
    """(value, |term| + k_z + k_s, sum |summands|) of one cone's compute_barrier at the fp64 points; (inf, 0, 0) outside"""
    key = (tuple(spec.alpha), spec.dim2, np.asarray(zp, float).tobytes(), np.asarray(sp_, float).tobytes())
    if key in _BAR_CACHE:
        return _BAR_CACHE[key]
    c = ipm._make_cones([spec])[0]
    with np.errstate(all="ignore"):
        inside = c.is_dual_feasible(np.asarray(zp, float)) and c.is_primal_feasible(np.asarray(sp_, float))
    if not inside:
        out = (math.inf, 0.0, 0.0)
    else:
        with mp.workdps(60):
            a = [mp.mpf(t) for t in spec.alpha]
            d1 = len(a)
            f = gr.dual_barrier(spec)
            z = [mp.mpf(float(t)) for t in zp]
            g = mp_primal_gradient(spec, sp_)
            y = [-t for t in g]
            val = f(*z) + (-f(*y) - (d1 + 1))
            summ = mp.mpf(d1 + 1)
            for v in (z, y):
                logs = [2 * a[i] * mp.log(v[i] / a[i]) for i in range(d1)]
                zeta = mp.exp(sum(logs)) - sum(t * t for t in v[d1:])
                summ += sum(abs(t) for t in logs) + sum(abs((1 - a[i]) * mp.log(v[i])) for i in range(d1)) + abs(mp.log(zeta))
            out = (float(val), abs(float(val)) + cancellation(spec, zp, True) + cancellation(spec, sp_, False), float(summ))
    _BAR_CACHE[key] = out
    return out


def gp_term_bound(spec, term, factor=1.0):
    return factor * BOUND_C["bar_gp"] * U * term[1] + ns.gamma(spec.numel) * term[2]


def barrier_reference(cones, z, s, dz, ds, alpha, factor=1.0):
    """(sum over all cones, bound): the generalized power cones' terms from here, the other cones' from
    nonsym_step_reference on the list without them; the terms' bounds add, and gamma_n covers adding the n terms"""
    off = ns.offsets(cones)
    zp, sp_ = z + alpha * dz, s + alpha * ds
    others = [c for c in cones if not is_gp(c)]
    rows = np.ones(len(z), bool)
    vals, bound = [], 0.0
    for c, o in zip(cones, off):
        if is_gp(c):
            rows[o:o + c.numel] = False
            t = gp_barrier_term(c, zp[o:o + c.numel], sp_[o:o + c.numel])
            vals.append(t[0])
            bound += gp_term_bound(c, t, factor)
    if others:
        # (the stepped point is formed again from the same fp64 operands: the same doubles)
        terms = ns.barrier_terms(others, z[rows], s[rows], dz[rows], ds[rows], alpha)
        vals += [t[1] for t in terms]
        bound += factor * sum(ns.BOUND_C["bar_" + t[0]] * U * t[2] for t in terms if t[0] != "zero")
    if any(not math.isfinite(v) for v in vals):
        return math.inf, 0.0
    return math.fsum(vals), bound + ns.gamma(len(vals)) * math.fsum(abs(v) for v in vals)


def barrier_numpy(cones, z, s, dz, ds, alpha):
    return ns.barrier_numpy(cones, z, s, dz, ds, alpha)


# ------------------------------------------------------------------------------------------
#  step length
# ------------------------------------------------------------------------------------------
step_length_sequential = ns.step_length_sequential       # (ipm._GenPow is an ipm._NonSym: the restatement covers it)
step_length_independent = ns.step_length_independent


def step_length_ambiguous(cones, z, s, dz, ds, a0, step=BACKTRACK_STEP, amin=ALPHA_MIN):
    """whether some feasibility test at a visited a0 step^j sits within its evaluation bound of the boundary"""
    if ns.step_length_ambiguous(cones, z, s, dz, ds, a0, step, amin):     # (the exponential / power cones of the list)
        return True
    visited, a = [], a0
    while a >= amin:
        visited.append(a)
        a *= step
    with mp.workdps(40):
        for c, o in zip(cones, ns.offsets(cones)):
            if not is_gp(c):
                continue
            r = slice(o, o + c.numel)
            for q, dq, scaled in ((z[r], dz[r], True), (s[r], ds[r], False)):
                for a in visited:
                    t = _phi_norm(c, q + a * dq, scaled)
                    if t is None:
                        continue                                      # a coordinate <= 0: outside whatever the rounding
                    res, mag = t[0] - t[1], t[0] * (1 + t[2]) + t[1]
                    if abs(res) <= FEAS_C * U * (1 + c.numel) * mag:
                        return True
                    if res > 0:
                        break
    return False


STEP_KINDS = ("free", "dual0", "dual1", "dual5", "primal0", "primal1", "primal5", "coord", "giveup")


def step_case(name, kind, seed=1):
    """free: nothing binds; dualJ / primalJ: one generalized power cone's ray leaves the dual / primal cone at
    a0 step^(J + 1/2); coord: a u_i reaches 0 (at a0 step^(1 + 1/2)) with the product bound never binding before it;
    giveup: a direction that is outside for every alpha >= alpha_min.  Every other cone steps along 0.01 (z, s)."""
    case = Case(name, seed=seed)
    rng = np.random.default_rng([seed, 78, STEP_KINDS.index(kind), LISTS.index(name)])
    case.dz, case.ds = 0.01 * case.z, 0.01 * case.s
    gp = case.gp()
    c, o = gp[int(rng.integers(len(gp)))]
    r = slice(o, o + c.numel)
    a0 = 1.0 - SQRT_EPS
    if kind[:-1] in ("dual", "primal"):
        dual, j = kind.startswith("dual"), int(kind[-1])
        q = (case.z if dual else case.s)[r]
        for _ in range(20):
            d = -q + 0.5 * np.abs(q).max() * rng.normal(size=c.numel) / math.sqrt(c.numel)
            t = ns._ray_exit(c, q, d, dual)
            if t is not None and t > 1e-3:
                break
        else:
            raise AssertionError("no leaving direction found")
        (case.dz if dual else case.ds)[r] = d * (t / (a0 * BACKTRACK_STEP ** (j + 0.5)))
    elif kind == "coord":
        # u_i and w shrink together: phi ~ (1 - a/T)^(2 alpha_i) falls no faster than ||w||^2 ~ (1 - a/T)^2
        T = a0 * BACKTRACK_STEP ** 1.5
        d = np.zeros(c.numel)
        i = int(rng.integers(c.dim1))
        d[i] = -case.z[o + i] / T
        d[c.dim1:] = -case.z[o + c.dim1:o + c.numel] / T
        case.dz[r] = d
    elif kind == "giveup":
        case.dz[r] = -1e6 * case.z[r]
    return case


_CASES = None


def step_cases():
    """every (list, kind) the GPU test runs with the excluded ones marked: {(name, kind): (case, excluded)}"""
    global _CASES
    if _CASES is None:
        _CASES = {}
        for name in LISTS:
            for kind in STEP_KINDS:
                case = step_case(name, kind)
                _CASES[(name, kind)] = (case, step_length_ambiguous(case.cones, case.z, case.s, case.dz, case.ds, 1.0 - SQRT_EPS))
    return _CASES
