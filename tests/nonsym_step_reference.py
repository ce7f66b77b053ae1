"""Extended-precision reference for the cone operations between the solves on cone lists that hold exponential and
power cones (TEST INFRASTRUCTURE): the non-symmetric rows of affine_ds / the combined step's d.s, the per-cone barrier,
and the composite step length with its backtracking searches.

Written from the definitions, with mpmath (60 digits) derivatives of the dual barriers AS WRITTEN
(tests/nonsymmetric_reference.dual_barrier), not from the closed forms of cuclarabel_amd/ipm.py or the kernels:

    affine d.s        a copy of s
    combined d.s      s + sigma_mu grad f*(z) + eta,   eta = -1/2 D^3 f*(z)[u, v],  u = H*(z)^{-1} ds,  v = m dz
                      (the third directional derivative: sum_jk d^3 f* / dz_i dz_j dz_k  u_j v_k).  SIGN: this eta is the
                      correction as the method defines it (H dz + ds = -s - sigma mu grad f*(z) - eta).  The reference's
                      higher_correction! -- and ipm._Exp / _Pow.higher_correction, and the kernel -- return its NEGATIVE,
                      +1/2 D^3 f*(z)[u, v], and combined_ds_shift! subtracts that: the same d.s.
    barrier           f*(z') + f(s') at z' = fl(z + alpha dz), s' = fl(s + alpha ds); the primal barrier is the conjugate
                      f(s) = -f*(-g(s)) - 3 with g(s) the root of grad f*(-g) = -s (mp findroot)
                      nonnegative  -sum log(s_i z_i);  second-order  -1/2 log(res(s) res(z)), res(v) = v0^2 - ||v1||^2;
                      PSD  -log det mat(s) - log det mat(z);  +inf outside
    step length       the composite rule of coneops_compositecone.jl:205-243, restated SEQUENTIALLY over the fp64 classes
                      of cuclarabel_amd/ipm.py (they are the definition of "the same doubles" here): tau / kappa / symmetric
                      limits, min(., 1 - sqrt(eps)), then cone after cone backtrack_search from the running alpha

Error bounds.  Every reference value carries a bound  C * u * (magnitude from its own conditioning):
    kz   cancellation in the dual barrier's argument: exp  (|z2| + |z1| + |z1 log(-z3/z1)|) / (z2 - z1 - z1 log(-z3/z1)),
         pow  (phi + z3^2) / (phi - z3^2);  ks the same for the primal feasibility argument
    grad rows          |s_i| + |sigma_mu| kz |grad_i|
    eta rows           kz * 1/2 sum_jk |T_ijk| (|H^-1| |H| |u|)_j |v_k|: the componentwise conditioning of the 3 x 3 solve
                       carried through the third-derivative tensor with absolute values (no cancellation credit)
    barrier term       |term| + kz + ks  (log of an argument that lost kz / ks to cancellation)
    sum of n terms     sum of the terms' bounds + gamma_n sum |term|

The constants C were FIXED BY MEASUREMENT on the CPU (tests/test_nonsym_step_reference_host.py prints the ratios under
-s): the worst distance of the committed numpy classes (ipm._Exp, ipm._Pow and the symmetric ones) from the mpmath value
over every point the GPU test uses, in units of u * magnitude, rounded up to the next power of two (at least 1):

    quantity                            measured worst (numpy classes)     C
    ds_exp    combined d.s, exponential    1.452                           2
    ds_pow    combined d.s, power          0.592                           1
    bar_exp   barrier term, exponential  105.729                         128
    bar_pow   barrier term, power          0.420                           1
    bar_nn    ... nonnegative              0.187                           1
    bar_soc   ... second-order             0.115                           1
    bar_psd   ... PSD                      0.062                           1

(bar_exp is not conditioning: barrier_primal goes through the Wright omega series with two refinement rounds, whose
truncation leaves w up to a hundred ulp off (w between 4 and 5 on these points) -- the numpy class and the kernel share that formula.)
The host test asserts the numpy classes stay within C (unmultiplied).  The DEVICE gets DEVICE_FACTOR = 4 times that: it
goes through the same formulas, but its log, exp and pow may differ from numpy's by a few ulp per call.

Step length: a case is EXCLUDED where some feasibility test at a visited alpha sits within its evaluation bound of the
boundary (|residual| <= FEAS_C u * sum of the magnitudes of its terms): there a few ulp in log / exp decide the test, and
neither answer is wrong.  At most 5 % of the generated cases may be excluded (asserted by the host test).
"""
import math

import numpy as np
import mpmath as mp

from cuclarabel_amd import ipm
from cuclarabel_amd.cones import (ZeroConeT, NonnegativeConeT, SecondOrderConeT, PSDTriangleConeT, ExponentialConeT,
                                  PowerConeT)
from tests import nonsymmetric_reference as nr

U = 2.0 ** -53
DEVICE_FACTOR = 4.0
FEAS_C = 32.0
SQRT_EPS = float(np.sqrt(np.finfo(float).eps))
BARRIER_ALPHAS = (0.0, 0.01)                             # where both test files evaluate the barrier: interior at every list
BACKTRACK_STEP, ALPHA_MIN = 0.8, 1e-4                    # settings.jl defaults (linesearch_backtrack_step, min_terminate_step_length)

# measured worst |numpy - mpmath| / (u * magnitude) over the GPU test's points (test_nonsym_step_reference_host.py -s),
# and the constant it fixes (the next power of two)
NUMPY_WORST = dict(ds_exp=1.452, ds_pow=0.592, bar_exp=105.729, bar_pow=0.42, bar_nn=0.187, bar_soc=0.115, bar_psd=0.062)
BOUND_C = dict(ds_exp=2.0, ds_pow=1.0, bar_exp=128.0, bar_pow=1.0, bar_nn=1.0, bar_soc=1.0, bar_psd=1.0)


def gamma(k):
    return k * U / (1.0 - k * U)


def is_ns(spec):
    return isinstance(spec, (ExponentialConeT, PowerConeT))


def fam(spec):
    return "exp" if isinstance(spec, ExponentialConeT) else "pow"


def offsets(cones):
    return np.concatenate([[0], np.cumsum([c.numel for c in cones])]).astype(int)


# ------------------------------------------------------------------------------------------
#  conditioning
# ------------------------------------------------------------------------------------------
def _feas_terms(spec, v, dual):
    """(residual, sum of |terms|) of the feasibility argument at the fp64 point v, in mpmath"""
    v = [mp.mpf(float(t)) for t in v]
    if isinstance(spec, ExponentialConeT):
        if dual:
            if not (v[2] > 0 and v[0] < 0):
                return mp.mpf(-1), mp.mpf(0)
            t = v[0] * mp.log(-v[2] / v[0])
            return v[1] - v[0] - t, abs(v[1]) + abs(v[0]) + abs(t)
        if not (v[2] > 0 and v[1] > 0):
            return mp.mpf(-1), mp.mpf(0)
        t = v[1] * mp.log(v[2] / v[1])
        return t - v[0], abs(t) + abs(v[0]) + abs(v[1])      # (s2 itself: the Wright omega argument is 1 - s1/s2 - log(s2/s3))
    a = mp.mpf(spec.alpha)
    if not (v[0] > 0 and v[1] > 0):
        return mp.mpf(-1), mp.mpf(0)
    l0, l1 = (2 * a * mp.log(v[0] / a), 2 * (1 - a) * mp.log(v[1] / (1 - a))) if dual else \
        (2 * a * mp.log(v[0]), 2 * (1 - a) * mp.log(v[1]))
    phi = mp.exp(l0 + l1)
    return phi - v[2] * v[2], phi * (1 + abs(l0) + abs(l1)) + v[2] * v[2]


def cancellation(spec, v, dual):
    r, mag = _feas_terms(spec, v, dual)
    return float(mag / r) if r > 0 else math.inf


# ------------------------------------------------------------------------------------------
#  d.s rows
# ------------------------------------------------------------------------------------------
_T_CACHE = {}


def _derivs(spec, z):
    """(grad, H, T) of f* at the fp64 point z in mpmath; T[i][j][k] the third derivatives"""
    key = (fam(spec), getattr(spec, "alpha", None), tuple(float(t) for t in z))
    if key not in _T_CACHE:
        f = nr.dual_barrier(spec)
        zz = [mp.mpf(float(t)) for t in z]
        g, H = nr.mp_grad(f, z), nr.mp_hess(f, z)
        T = [[[None] * 3 for _ in range(3)] for _ in range(3)]
        for i in range(3):
            for j in range(i, 3):
                for k in range(j, 3):
                    order = [0, 0, 0]
                    for t in (i, j, k):
                        order[t] += 1
                    val = mp.diff(f, zz, tuple(order))
                    for (a, b, c) in {(i, j, k), (i, k, j), (j, i, k), (j, k, i), (k, i, j), (k, j, i)}:
                        T[a][b][c] = val
        _T_CACHE[key] = (g, H, T)
    return _T_CACHE[key]


def ns_ds_rows(spec, s, z, dz, ds, sigma_mu, m_corr, combined):
    """(value, magnitude) of the cone's three d.s rows; the bound is C u magnitude"""
    if not combined:
        return np.array(s, float), np.zeros(3)                       # a copy: exact
    with mp.workdps(60):
        g, H, T = _derivs(spec, z)
        dsv = mp.matrix([float(t) for t in ds])
        v = [mp.mpf(float(m_corr)) * mp.mpf(float(t)) for t in dz]
        Hinv = H ** -1
        u = Hinv * dsv
        cu = [sum(abs(Hinv[j, a]) * sum(abs(H[a, b]) * abs(u[b]) for b in range(3)) for a in range(3)) for j in range(3)]
        kz = cancellation(spec, z, True)
        val, mag = np.zeros(3), np.zeros(3)
        for i in range(3):
            eta = -sum(T[i][j][k] * u[j] * v[k] for j in range(3) for k in range(3)) / 2
            val[i] = float(mp.mpf(float(s[i])) + mp.mpf(float(sigma_mu)) * g[i] + eta)
            e_abs = sum(abs(T[i][j][k]) * cu[j] * abs(v[k]) for j in range(3) for k in range(3)) / 2
            mag[i] = abs(float(s[i])) + kz * (abs(float(sigma_mu)) * float(abs(g[i])) + float(e_abs))
    return val, mag


def ns_ds_numpy(spec, s, z, dz, ds, mu, strategy, sigma_mu, m_corr, combined):
    """the same rows through the committed numpy class, as ipm.solve forms them"""
    c = ipm._make_cones([spec])[0]
    c.update_scaling(np.array(s, float), np.array(z, float), mu, strategy)
    aff = c.affine_ds(np.array(s, float))
    return aff + c.combined_ds_shift(np.array(dz, float) * m_corr, np.array(ds, float), sigma_mu) if combined else aff


# ------------------------------------------------------------------------------------------
#  barrier
# ------------------------------------------------------------------------------------------
_BAR_CACHE = {}


def _ns_barrier_term(spec, zp, sp_):
    key = (fam(spec), getattr(spec, "alpha", None), tuple(map(float, zp)), tuple(map(float, sp_)))
    if key in _BAR_CACHE:
        return _BAR_CACHE[key]
    c = ipm._make_cones([spec])[0]
    if not (c.is_dual_feasible(zp) and c.is_primal_feasible(sp_)):
        out = (math.inf, 0.0)
    else:
        with mp.workdps(60):
            f = nr.dual_barrier(spec)
            with np.errstate(all="ignore"):
                g0 = c.gradient_primal(np.asarray(sp_, float))
            g = nr.mp_primal_gradient(spec, sp_, g0)
            val = f(*[mp.mpf(float(t)) for t in zp]) + (-f(-g[0], -g[1], -g[2]) - 3)
            out = (float(val), abs(float(val)) + cancellation(spec, zp, True) + cancellation(spec, sp_, False))
    _BAR_CACHE[key] = out
    return out


def _smat_mp(x, k):
    M = mp.zeros(k, k)
    idx = 0
    for col in range(k):
        for row in range(col + 1):
            v = mp.mpf(float(x[idx])) * (1 if row == col else 1 / mp.sqrt(2))
            M[row, col] = M[col, row] = v
            idx += 1
    return M


def barrier_terms(cones, z, s, dz, ds, alpha):
    """[(family, value, magnitude)] per cone at the fp64 stepped point (formed as the kernels form it)"""
    off = offsets(cones)
    zp, sp_ = z + alpha * dz, s + alpha * ds
    out = []
    for c, o in zip(cones, off):
        r = slice(o, o + c.numel)
        zc, sc = zp[r], sp_[r]
        if isinstance(c, ZeroConeT) or c.numel == 0:
            out.append(("zero", 0.0, 0.0))
        elif isinstance(c, NonnegativeConeT):
            if np.all(zc > 0) and np.all(sc > 0):
                with mp.workdps(60):
                    logs = [mp.log(mp.mpf(float(a)) * mp.mpf(float(b))) for a, b in zip(zc, sc)]
                    out.append(("nn", -float(sum(logs)), (len(logs) + 2) * float(sum(abs(t) + 2 for t in logs))))
            else:
                out.append(("nn", math.inf, 0.0))
        elif isinstance(c, SecondOrderConeT):
            with mp.workdps(60):
                res, mag = [], 0.0
                for v in (sc, zc):
                    v = [mp.mpf(float(t)) for t in v]
                    n2 = sum(t * t for t in v[1:])
                    res.append(v[0] * v[0] - n2 if v[0] > 0 else mp.mpf(-1))
                    mag += float((v[0] * v[0] + n2) / res[-1]) * len(v) if res[-1] > 0 else 0.0
                if res[0] > 0 and res[1] > 0:
                    val = -float(mp.log(res[0] * res[1]) / 2)
                    out.append(("soc", val, abs(val) + mag))
                else:
                    out.append(("soc", math.inf, 0.0))
        elif isinstance(c, PSDTriangleConeT):
            k = c.dim
            with mp.workdps(60):
                val, mag, ok = mp.mpf(0), 0.0, True
                for v in (zc, sc):
                    M = _smat_mp(v, k)
                    try:
                        L = mp.cholesky(M)
                    except (ValueError, ZeroDivisionError):
                        ok = False
                        break
                    val -= 2 * sum(mp.log(L[i, i]) for i in range(k))
                    Mf = np.array([[float(M[i, j]) for j in range(k)] for i in range(k)])
                    mag += k * k * float(np.linalg.cond(Mf))
                out.append(("psd", float(val), abs(float(val)) + mag) if ok else ("psd", math.inf, 0.0))
        else:
            val, mag = _ns_barrier_term(c, zc, sc)
            out.append((fam(c), val, mag))
    return out


def barrier_sum(terms, factor=1.0):
    """(sum, bound) of a list of barrier terms: sum of the per-term bounds + gamma_n sum |term|"""
    vals = [t[1] for t in terms]
    if any(not math.isfinite(v) for v in vals):
        return math.inf, 0.0
    total = math.fsum(vals)
    bound = factor * sum(BOUND_C["bar_" + t[0]] * U * t[2] for t in terms if t[0] != "zero")
    return total, bound + gamma(len(terms)) * math.fsum(abs(v) for v in vals)     # (adding the slots' exact zeros costs nothing)


def barrier_numpy(cones, z, s, dz, ds, alpha):
    """per-cone compute_barrier of the committed numpy classes"""
    cs = ipm._make_cones(cones)
    return [c.compute_barrier(z[c.rng], s[c.rng], dz[c.rng], ds[c.rng], alpha) for c in cs]


# ------------------------------------------------------------------------------------------
#  step length
# ------------------------------------------------------------------------------------------
class _St:
    linesearch_backtrack_step = BACKTRACK_STEP
    min_terminate_step_length = ALPHA_MIN


def _scaled(cones, s, z):
    cs = ipm._make_cones(cones)
    for c in cs:
        if isinstance(c, ipm._NonSym):
            continue
        assert c.update_scaling(s[c.rng].copy(), z[c.rng].copy())
    return cs


def _start(cs, z, s, dz, ds, dtau, dkappa, tau, kappa):
    at = -tau / dtau if dtau < 0 else np.finfo(float).max
    ak = -kappa / dkappa if dkappa < 0 else np.finfo(float).max
    a = min(at, ak, 1.0)
    for c in cs:
        if not isinstance(c, ipm._NonSym):
            a = min(a, c.step_length(dz[c.rng], ds[c.rng], z[c.rng], s[c.rng], a))
    return min(a, 1.0 - SQRT_EPS)


def step_length_sequential(cones, z, s, dz, ds, dtau=1.0, dkappa=1.0, tau=1.0, kappa=1.0, step=BACKTRACK_STEP, amin=ALPHA_MIN):
    """coneops_compositecone.jl:205-243 as ipm.solve restates it: alpha tightened cone after cone"""
    cs = _scaled(cones, s, z)
    st = _St()
    st.linesearch_backtrack_step, st.min_terminate_step_length = step, amin
    a = _start(cs, z, s, dz, ds, dtau, dkappa, tau, kappa)
    for c in cs:
        if isinstance(c, ipm._NonSym):
            a = min(a, c.step_length(dz[c.rng], ds[c.rng], z[c.rng], s[c.rng], a, st))
    return a


def step_length_independent(cones, z, s, dz, ds, dtau=1.0, dkappa=1.0, tau=1.0, kappa=1.0, step=BACKTRACK_STEP, amin=ALPHA_MIN):
    """the form the device uses: every cone from the common start, folded by a minimum"""
    cs = _scaled(cones, s, z)
    st = _St()
    st.linesearch_backtrack_step, st.min_terminate_step_length = step, amin
    a0 = _start(cs, z, s, dz, ds, dtau, dkappa, tau, kappa)
    return min([a0] + [c.step_length(dz[c.rng], ds[c.rng], z[c.rng], s[c.rng], a0, st) for c in cs if isinstance(c, ipm._NonSym)])


def step_length_ambiguous(cones, z, s, dz, ds, a0, step=BACKTRACK_STEP, amin=ALPHA_MIN):
    """whether some feasibility test at a visited a0 step^j sits within its evaluation bound of the boundary"""
    off = offsets(cones)
    visited, a = [], a0
    while a >= amin:
        visited.append(a)
        a *= step
    with mp.workdps(40):
        for c, o in zip(cones, off):
            if not is_ns(c):
                continue
            for q, dq, dual in ((z[o:o + 3], dz[o:o + 3], True), (s[o:o + 3], ds[o:o + 3], False)):
                for a in visited:
                    r, mag = _feas_terms(c, q + a * dq, dual)
                    if mag > 0 and abs(r) <= FEAS_C * U * mag:
                        return True
                    if r > 0:
                        break                                  # inside: the search stops here (and stays inside below)
    return False


# ------------------------------------------------------------------------------------------
#  the cases both test files share
# ------------------------------------------------------------------------------------------
def _list(name):
    E, Pw = ExponentialConeT, PowerConeT
    if name == "exp":
        return [E()]
    if name == "pow":
        return [Pw(0.3)]
    if name == "mixed":
        return [NonnegativeConeT(3), E(), SecondOrderConeT(3), Pw(0.7), ZeroConeT(1), PSDTriangleConeT(2), E()]
    return [NonnegativeConeT(1)] + [E() for _ in range(int(name))]    # "255", "256", "257"


LISTS = ("exp", "pow", "mixed", "255", "256", "257")
POOL = 8                                                              # distinct exponential points tiled over the long lists


class Case:
    """cones, an interior (s, z) -- random_interior_pair, or central_pair with central=True -- and a step (dz, ds)"""

    def __init__(self, name, seed=1, central=False, step_scale=0.3):
        rng = np.random.default_rng([seed, LISTS.index(name), int(central)])
        self.name, self.cones = name, _list(name)
        self.m = sum(c.numel for c in self.cones)
        self.off = offsets(self.cones)
        s, z = np.zeros(self.m), np.zeros(self.m)
        pool = []
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
            else:
                if name in ("255", "256", "257") and len(pool) == POOL:
                    s[r], z[r] = pool[(o // 3) % POOL]                # few distinct points: the mpmath reference is cached
                else:
                    pr = nr.central_pair(c, rng) if central else nr.random_interior_pair(c, rng)
                    pool.append(pr)
                    s[r], z[r] = pr
        self.s, self.z = s, z
        self.dz, self.ds = step_scale * rng.normal(size=self.m), step_scale * rng.normal(size=self.m)
        if name in ("255", "256", "257"):                             # tile the steps as well
            for o in self.off[1 + POOL:-1]:
                src = self.off[1 + ((o // 3) % POOL)]
                self.dz[o:o + 3], self.ds[o:o + 3] = self.dz[src:src + 3], self.ds[src:src + 3]
        self.mu = float(s @ z) / max(1, sum(ipm._make_cones([c])[0].degree for c in self.cones))

    def ns(self):
        return [(c, o) for c, o in zip(self.cones, self.off) if is_ns(c)]

    def sym_rows(self):
        rows = np.ones(self.m, bool)
        for _, o in self.ns():
            rows[o:o + 3] = False
        return rows

    def twin(self):
        """the symmetric cones alone, with their rows of s and z"""
        return [c for c in self.cones if not is_ns(c)], self.sym_rows()


def _ray_exit(c, q, d, dual):
    """the alpha at which q + alpha d leaves the cone (bisection over the fp64 class's test), or None within 4"""
    cone = ipm._make_cones([c])[0]
    inside = cone.is_dual_feasible if dual else cone.is_primal_feasible
    with np.errstate(all="ignore"):
        if inside(q + 4.0 * d):
            return None
        lo, hi = 0.0, 4.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if inside(q + mid * d) else (lo, mid)
    return lo


STEP_KINDS = ("free", "dual", "primal", "symmetric", "zero")


def step_case(name, kind, seed):
    """One of the five step-length situations -> a Case with .scal, the (dtau, dkappa, tau, kappa) keywords.  The symmetric
    cones step along (z, s) themselves (inside their cones: no limit) except where kind == "symmetric": there a
    nonnegative row limits the step to exactly 0.5 -- or, on a list without a symmetric cone, the tau limit does."""
    case = Case(name, seed=seed)
    case.scal = {}
    rng = np.random.default_rng([seed, 77, STEP_KINDS.index(kind)])
    sym = case.sym_rows()
    case.dz[sym], case.ds[sym] = 0.01 * case.z[sym], 0.01 * case.s[sym]
    ns = case.ns()
    for c, o in ns:                                                    # nothing binds: a short step towards the inside
        case.dz[o:o + 3], case.ds[o:o + 3] = 0.01 * case.z[o:o + 3], 0.01 * case.s[o:o + 3]
    c, o = ns[int(rng.integers(len(ns)))]
    if kind in ("dual", "primal"):
        q = case.z[o:o + 3] if kind == "dual" else case.s[o:o + 3]
        target = float(rng.uniform(0.05, 0.62))                        # below 0.64 (1 - sqrt(eps)): j >= 2 backtracks
        for _ in range(20):
            d = -q + 0.5 * np.abs(q).max() * rng.normal(size=3)
            t = _ray_exit(c, q, d, kind == "dual")
            if t is not None and t > 1e-3:
                break
        else:
            raise AssertionError("no leaving direction found")
        d = d * (t / target)
        (case.dz if kind == "dual" else case.ds)[o:o + 3] = d
    elif kind == "symmetric":
        nn = [oo for cc, oo in zip(case.cones, case.off) if isinstance(cc, NonnegativeConeT)]
        if nn:
            case.dz[nn[0]] = -case.z[nn[0]] / 0.5                      # the nonnegative limit: exactly 0.5 on both sides
        else:
            case.scal = dict(dtau=-2.0, tau=1.0)
    elif kind == "zero":
        case.dz[o:o + 3] = -1e6 * case.z[o:o + 3]                      # (1 - 1e6 alpha) z: outside for every alpha >= alpha_min
    return case


def step_cases(seeds=(1, 2, 3)):
    """every (list, kind, seed) the GPU test runs, with the excluded ones marked: [(name, kind, seed, case, excluded)]"""
    out = []
    for name in LISTS:
        for kind in STEP_KINDS:
            for seed in (seeds if name in ("exp", "pow", "mixed") else seeds[:1]):
                case = step_case(name, kind, seed)
                cs = _scaled(case.cones, case.s, case.z)
                a0 = _start(cs, case.z, case.s, case.dz, case.ds, case.scal.get("dtau", 1.0), 1.0, case.scal.get("tau", 1.0), 1.0)
                out.append((name, kind, seed, case, step_length_ambiguous(case.cones, case.z, case.s, case.dz, case.ds, a0)))
    return out
