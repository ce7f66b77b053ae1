r"""Host reference for the level-C Newton step (hipkkt_kkt_system_solve, _update_and_solve_affine, _solve_initial_point):
the four equations that define the step evaluated exactly, order-free bounds on them, a plain numpy restatement of
kkt_solve! / kkt_solve_initial_point!, simulated kernel faults and problems with prescribed lane and grid edges -- TEST
INFRASTRUCTURE ONLY.

The step (kktsystem.jl:145-215), xi = x / tau, (x2, z2) = K \ (-q, b), (x1, z1) = K \ (rhs_x, c - rhs_z):

    c      = s (affine step)  or  W^T (lambda \ rhs_s)                          the constant term of Delta s
    dtau   = N / D,  N = rhs_tau - rhs_kappa / tau + q.x1 + b.z1 + 2 xi.P x1,
                     D = kappa / tau - q.x2 - b.z2 + (xi - x2).P (xi - x2) - x2.P x2
    dx, dz = x1 + dtau x2, z1 + dtau z2      ds = -(Hs dz + c)      dkappa = -(rhs_kappa + kappa dtau) / tau

It satisfies, whatever the condition of K and without knowing (x1, z1) and (x2, z2) apart:

    (1) reduced rows   K [dx; dz] - [rhs_x; c - rhs_z] - dtau [-q; b]  =  r1 + dtau r2
    (2) tau row        rhs_tau - rhs_kappa / tau + q.dx + b.dz + 2 xi.P dx - dtau (kappa / tau + xi.P xi)  =  0
    (3) kappa          dkappa + (rhs_kappa + kappa dtau) / tau  =  0
    (4) s row          ds + Hs dz + c  =  0

K is the un-regularised matrix the refinement measures against (its sparse second-order-cone columns included: their
variables are eliminated exactly from their own rows, which moves a row residual r_e into the cone's z rows through
|K12| |K22^-1|); r1, r2 are the residuals refinement stopped at.  (2) is N - dtau D = 0 with (xi - x2).P (xi - x2) -
x2.P x2 expanded -- an identity of the formula, not a property of the solves.

EXACT VALUES.  Every product of two doubles is split without error (two_product) and math.fsum adds exactly, as in
tests/residual_reference.py; what is not a sum of such products (the divisions by tau, c of a nonnegative cone, the
eliminated second-order-cone variables) is carried as a Fraction and split into hi + lo doubles (2^-106); lambda \ and
R X R' of second-order and PSD cones are evaluated with mpmath at 50 digits from the scaling the handle RETURNED (w,
eta, lambda, R), the congruences as exact integer matrix products.

BOUNDS (u = 2^-53, gamma_j = j u / (1 - j u); an inner product of k terms in ANY order, with or without fma, errs by
at most gamma_k sum |a_i b_i| -- Higham, Accuracy and Stability, 2nd ed., (3.5)).  Magnitudes: X2 = |x2|, Z2 = |z2|
from a level-B solve of (-q, b) on the same handle, X1 = |dx| + |dtau| X2 >= |x1| (1 - gamma_2), XM = |x| / tau + X2 >=
|xi - x2|; kP the longest row of P the kernel walks (structural diagonal included).  They enter the bounds only.

    (3)  three roundings:  gamma_3 (|rhs_kappa| + |kappa dtau|) / tau
    (2)  the computed N^ and D^ err by
           eN = g(n) |q|.X1 + g(m) |b|.Z1 + (2 / tau) g(n + kP) |x|.|P| X1 + gamma_8 (|rhs_tau| + |rhs_kappa| / tau + |q|.X1 + ...)
           eD = g(n) |q|.X2 + g(m) |b|.Z2 + (g(n + kP) + 2 gamma_3) XM.|P| XM + g(n + kP) X2.|P| X2 + gamma_8 magD
         with g(k) = gamma_{k+2} (a dot product of length k behind a product that is itself rounded), 2 gamma_3 XM.|P| XM the
         rounding of xi - x2 carried through both sides of the quadratic form, gamma_8 the scalar tail of at most eight
         operations, magD = kappa / tau + |q|.X2 + |b|.Z2 + XM.|P| XM + X2.|P| X2.  dtau = N^ / D^ (1 + e), |e| <= u, gives
         |N - dtau D| <= eN + |dtau| (eD + u magD); forming dx, dz adds gamma_2 (|q|.X1 + |b|.Z1 + (2 / tau) |x|.|P| X1).
    (1)  per row of the full K:  tol1 + |dtau| tol2, tol_i = abstol + reltol ||b_i||_inf (the handle's settings)
         + gamma_{k+1} (|b1| + |K| M1) + |dtau| gamma_{k+1} (|b2| + |K| M2)      the residual kernel's own rounding, k the row length
         + gamma_2 |K| (M1 + |dtau| M2)                                          forming dx, dz
         + u |c - rhs_z| + |c^ - c|                                              forming the right-hand side (z rows)
         with M2 = (X2, Z2, |K22^-1| |K21| (X2, Z2)), M1 = (|dx|, |dz|, |p|) + |dtau| M2; rows of eliminated variables are then
         added to the rows they feed: bound_top += |K12| |K22^-1| bound_ext.
    (4)  zero cone: exact.  nonnegative: ds = -fl(fl(w fl(w dz)) + fl(rhs_s / z)): gamma_4 (w^2 |dz| + |c|); affine rows of
         every cone read c = s exactly.  Second-order and PSD cones have no textbook bound for k_mul_Hs and k_sys_offset*
         (the stable form through z, A = fl(R R')): as in tests/nonsym_step_reference.py the fp64 numpy classes of
         cuclarabel_amd/ipm.py -- the reference, not the kernel -- are measured over every builder, both iterate scales and
         both step types (python -m tests.system_reference measure, seeds as in ITERATE_SEED / RHS_SEED) and the device gets
         DEVICE_FACTOR = 4 times their largest ratio to the natural scale per cone,
             (4):  u max_i (|Hs| |dz| + |c|)_i            |c^ - c| in (1):  u max_i |c_i|
         (NUMPY_WORST below; |Hs| = eta^2 (2 |w| |w|' + I), |A| (.) |A| with A = |R| |R|').
"""
import math
import sys
from fractions import Fraction

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import cone_reference as cr
from tests import step_reference as sr
from tests.iterate_reference import _fsum_rows, _prod_lists, dot_exact, ratio
from tests.residual_reference import U, gamma, sym_from_triu, two_product

MP = cr.MP
DEVICE_FACTOR = 4.0
ITERATE_SEED, RHS_SEED = 7301, 7302
SCALES = ("unit", "late")
# measured: the largest error of the numpy classes / (u * natural scale), per family, over BUILDERS x SCALES x step types
# (python -m tests.system_reference measure)
NUMPY_WORST = dict(ds_soc=739.135, ds_psd=1.5, c_soc=1922.159, c_psd=4.936)
SPMV_ROWS_PER_WG, SPMV_GRID_CAP = 32, 2048
DOT_BLOCKS = 64


def _F(v):
    return Fraction(float(v))


def _split(fr):
    """Fraction or mpmath number -> (hi, lo) doubles, hi + lo = value to 2^-106"""
    if isinstance(fr, Fraction):
        hi = float(fr)
        return hi, float(fr - Fraction(hi))
    hi = float(fr)
    return hi, float(fr - MP.mpf(hi))


# ---------------------------------------------------------------------------------------------------------------------
#  problems
# ---------------------------------------------------------------------------------------------------------------------
class Problem:
    def __init__(self, name, P, A, cones, seed):
        rng = np.random.default_rng(seed)
        self.name, self.cones, self.late_decades = name, list(cones), 6
        self.P = sp.triu(sp.csc_matrix(P), format="csc")
        self.A = sp.csc_matrix(A)
        self.P.sort_indices()
        self.A.sort_indices()
        self.n, self.m = self.P.shape[0], self.A.shape[0]
        assert self.m == sum(c.numel for c in self.cones)
        self.q, self.b = rng.standard_normal(self.n), rng.standard_normal(self.m)
        self.Pfull = sp.csr_matrix(self.P + sp.triu(self.P, 1, format="csc").T)
        self.Pfull.sort_indices()
        one = sp.csc_matrix((np.ones(self.P.nnz), self.P.indices, self.P.indptr), shape=self.P.shape)
        self.user_rows = np.diff(sp.csr_matrix(one + sp.triu(one, 1, format="csc").T).indptr)   # full symmetric rows of P
        pat = sp.csr_matrix(one + sp.triu(one, 1, format="csc").T + sp.identity(self.n, format="csc"))
        self.kP = int(np.diff(pat.indptr).max()) if self.n else 0
        if self.m:
            assert np.diff(self.A.indptr).min() >= 1 and np.diff(sp.csr_matrix(self.A).indptr).min() >= 1

    def offsets(self):
        off = 0
        for i, c in enumerate(self.cones):
            yield c, i, slice(off, off + c.numel)
            off += c.numel


def _vals(rng, k, lo=0.5, hi=1.5):
    return rng.uniform(lo, hi, k) * rng.choice([-1.0, 1.0], k)


def _make_A(rng, m, n, per_row=3):
    """m x n, an entry of size 1..2 in every column (at row j mod m) and per_row entries of size <= 0.5 in every row"""
    if m == 0:
        return sp.csc_matrix((0, n))
    r = [np.arange(n) % m]
    c = [np.arange(n)]
    v = [_vals(rng, n, 1.0, 2.0)]
    k = min(per_row, n)
    for i in range(m):
        cols = rng.choice(n, size=k, replace=False)
        r.append(np.full(k, i))
        c.append(cols)
        v.append(_vals(rng, k, 0.1, 0.5))
    A = sp.csc_matrix(sp.coo_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(m, n)))
    A.sum_duplicates()
    return A


def _tridiag(rng, n):
    if n == 1:
        return sp.csc_matrix(np.array([[rng.uniform(1.0, 2.0)]]))
    return sp.diags([rng.uniform(1.0, 2.0, n), rng.uniform(-0.3, 0.3, n - 1)], [0, 1], format="csc")


def _cones(*spec):
    from cuclarabel_amd.cones import NonnegativeConeT, PSDTriangleConeT, SecondOrderConeT, ZeroConeT
    T = dict(z=ZeroConeT, nn=NonnegativeConeT, soc=SecondOrderConeT, psd=PSDTriangleConeT)
    return [T[k](d) for k, d in spec]


P_ROW_LENGTHS = (0, 1, 7, 8, 9, 17, 65)
N_EDGES = (1, 31, 32, 33, 255, 257)
SOC_COUNTS = {1: (130,), 4: (2, 3, 64, 65), 5: (2, 3, 64, 65, 130)}
PSD_SIDES = (1, 2, 16, 23, 48)


def build_mixed(seed=7101):
    """every symmetric cone kind, dense and sparse second-order cones, a random sparse P"""
    rng = np.random.default_rng(seed)
    n = 40
    B = sp.random(n, n, density=0.08, random_state=np.random.RandomState(seed), format="csc", data_rvs=lambda k: _vals(rng, k))
    P = (B.T @ B + 0.5 * sp.identity(n)).tocsc()
    cones = _cones(("z", 3), ("nn", 30), ("soc", 3), ("soc", 4), ("soc", 6), ("soc", 15), ("psd", 2), ("psd", 3), ("psd", 6))
    return Problem("mixed", P, _make_A(rng, sum(c.numel for c in cones), n, 5), cones, seed + 1)


def build_p_rows(seed=7102, explicit_zero=False):
    """Rows of P (full symmetric, structural diagonal counted) of every length in P_ROW_LENGTHS against eight lanes per
    row: hubs with their diagonal and L - 1 links to leaves of their own (a leaf: diagonal and link, length 2), variables
    with the diagonal alone (1) and variables without any entry of P (0).  Diagonally dominant, so P >= 0.
    explicit_zero: one of the links is a stored 0.0 (a structural entry the kernels walk)."""
    rng = np.random.default_rng(seed)
    lens = [L for L in P_ROW_LENGTHS if L >= 2]
    nleaf = sum(L - 1 for L in lens)
    n = len(lens) + nleaf + 4
    pr, pc, pv = [], [], []
    dg = np.zeros(n)
    leaf = len(lens)
    for h, L in enumerate(lens):
        for _ in range(L - 1):
            v = float(_vals(rng, 1, 0.05, 0.2)[0])
            pr.append(h); pc.append(leaf); pv.append(v)
            dg[h] += abs(v)
            dg[leaf] += abs(v)
            leaf += 1
    for i in range(leaf):
        dg[i] += rng.uniform(0.5, 1.0)
    dg[leaf], dg[leaf + 1] = 1.25, 0.75                      # diagonal alone; the last two variables: no entry at all
    if explicit_zero:
        pv[3] = 0.0
    keep = np.flatnonzero(dg)
    P = sp.csc_matrix(sp.coo_matrix((np.r_[pv, dg[keep]], (np.r_[pr, keep].astype(int), np.r_[pc, keep].astype(int))), shape=(n, n)))
    if explicit_zero:                                         # (coo -> csc keeps the stored zero)
        assert P.nnz == len(pv) + keep.size and (P.data == 0.0).sum() == 1
    cones = _cones(("z", 4), ("nn", n + 6))
    pb = Problem("p_zero" if explicit_zero else "p_rows", P, _make_A(rng, n + 10, n, 2), cones, seed + 1)
    assert set(P_ROW_LENGTHS) <= set(pb.user_rows.tolist()), "P row lengths"
    return pb


def build_lp(n, seed=7103):
    """P exactly empty (the LP branch of the initial point); m > n rows so that K is well conditioned"""
    rng = np.random.default_rng(seed + n)
    cones = _cones(("z", max(n // 8, 0)), ("nn", n + 5 - max(n // 8, 0)))
    pb = Problem(f"lp{n}", sp.csc_matrix((n, n)), _make_A(rng, n + 5, n, 2), cones, seed + n + 1)
    pb.late_decades = 4
    assert pb.P.nnz == 0
    return pb


def build_n(n, seed=7104):
    """n against the 32 rows per workgroup of the spmv kernels and the i < n / i >= n split of the step kernel"""
    rng = np.random.default_rng(seed + n)
    cones = _cones(("z", 1), ("nn", 9), ("soc", 3))
    return Problem(f"n{n}", _tridiag(rng, n), _make_A(rng, 13, n, 3), cones, seed + n + 1)


def build_m0(seed=7105):
    rng = np.random.default_rng(seed)
    return Problem("m0", _tridiag(rng, 33), sp.csc_matrix((0, 33)), [], seed + 1)


def build_soc(count, seed=7106):
    """second-order cones: four to a workgroup, rows strided by 64 lanes; sides on both sides of the dense / sparse switch"""
    rng = np.random.default_rng(seed + count)
    cones = _cones(*[("soc", d) for d in SOC_COUNTS[count]])
    return Problem(f"soc{count}", _tridiag(rng, 24), _make_A(rng, sum(c.numel for c in cones), 24, 3), cones, seed + count + 1)


def build_psd(seed=7107):
    """PSD sides: k (k + 1) / 2 and k^2 against 256 threads (23: 276 > 256), 48 the largest side level C accepts"""
    rng = np.random.default_rng(seed)
    cones = _cones(*[("psd", k) for k in PSD_SIDES])
    return Problem("psd", _tridiag(rng, 24), _make_A(rng, sum(c.numel for c in cones), 24, 2), cones, seed + 1)


def build_interleaved(seed=7108):
    """every symmetric kind between zero cones of size 0 and 1"""
    rng = np.random.default_rng(seed)
    cones = _cones(("z", 0), ("nn", 3), ("z", 1), ("soc", 3), ("z", 0), ("psd", 2), ("z", 1), ("soc", 6), ("nn", 1), ("z", 0),
                   ("psd", 3), ("z", 1), ("soc", 2), ("z", 0))
    return Problem("interleaved", _tridiag(rng, 20), _make_A(rng, sum(c.numel for c in cones), 20, 3), cones, seed + 1)


def build_large(seed=7109):
    """the second laps: n = 2048 * 32 + 33 rows of a tridiagonal P (the spmv grid cap), one nonnegative cone of m = 64 * 256
    + 257 rows (k_dots' 64 x 256 threads per pair), one or two entries per row of A"""
    rng = np.random.default_rng(seed)
    n, m = SPMV_GRID_CAP * SPMV_ROWS_PER_WG + 33, DOT_BLOCKS * 256 + 257
    cols0 = np.arange(n)
    home = (cols0 * m) // n                                  # column j sits in row j m / n: K stays banded, the fill small
    odd = np.arange(1, m, 2)
    r = np.concatenate([home, odd])
    c = np.concatenate([cols0, np.minimum((odd * n) // m + 5, n - 1)])
    A = sp.csc_matrix(sp.coo_matrix((_vals(rng, r.size, 0.2, 0.6), (r, c)), shape=(m, n)))
    A.sum_duplicates()
    return Problem("large", _tridiag(rng, n), A, _cones(("nn", m)), seed + 1)


BUILDERS = dict([("mixed", build_mixed), ("p_rows", build_p_rows), ("p_zero", lambda: build_p_rows(explicit_zero=True))] +
                [(f"lp{n}", (lambda n=n: build_lp(n))) for n in (1, 33, 257)] +
                [(f"n{n}", (lambda n=n: build_n(n))) for n in N_EDGES] +
                [("m0", build_m0)] + [(f"soc{k}", (lambda k=k: build_soc(k))) for k in SOC_COUNTS] +
                [("psd", build_psd), ("interleaved", build_interleaved), ("large", build_large)])
EDGE_BUILDERS = tuple(k for k in BUILDERS if k not in ("mixed", "large"))
_PROBLEMS = {}


def problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = BUILDERS[name]()
    return _PROBLEMS[name]


class Iterate:
    pass


def iterate(pb, scale, seed=ITERATE_SEED):
    """(x, s, z, tau, kappa) with (s, z) strictly interior.  unit: entries of order one, tau, kappa = 1.3, 0.7.  late: mu ~
    1e-6 with the magnitude of every cone (every entry of a nonnegative cone) drawn from six decades, s z ~ mu, second-order
    cones at relative distance 1e-3 .. 1e-1 from the boundary; tau, kappa = 1e-3, 2e-5.  (Replaced because the oracle's refined
    solves did not reach the stopping tolerance on them: PSD cones of condition 1e6 on top of the magnitudes -- they are well
    conditioned now --, and six decades on a problem without P -- pb.late_decades = 4 there.)"""
    rng = np.random.default_rng(seed + (0 if scale == "unit" else 1))
    it = Iterate()
    it.scale, it.mu = scale, (1.0 if scale == "unit" else 1e-6)
    it.x = rng.standard_normal(pb.n)
    it.tau, it.kappa = (1.3, 0.7) if scale == "unit" else (1e-3, 2e-5)
    s, z = np.zeros(pb.m), np.zeros(pb.m)
    for c, _, r in pb.offsets():
        k = c.numel
        if k == 0:
            continue
        if c.kind == 0:
            s[r], z[r] = it.mu * rng.standard_normal(k), rng.standard_normal(k)
        elif c.kind == 1:
            if scale == "unit":
                s[r], z[r] = np.exp(rng.uniform(-1, 1, k)), np.exp(rng.uniform(-1, 1, k))
            else:
                s[r] = 10.0 ** rng.uniform(-3 - pb.late_decades / 2, -3 + pb.late_decades / 2, k)
                z[r] = it.mu / s[r] * np.exp(rng.uniform(-0.5, 0.5, k))
        elif c.kind == 2:
            if scale == "unit":
                s[r], z[r] = cr.soc_pair(rng, k)
            else:
                f = 10.0 ** rng.uniform(-6, 0)
                s[r] = f * cr.soc_point(rng, k, 10.0 ** rng.uniform(-3, -1))
                z[r] = it.mu / f * cr.soc_point(rng, k, 10.0 ** rng.uniform(-3, -1))
        else:
            if scale == "unit":
                s[r], z[r] = cr.psd_pair(rng, c.dim, "interior")
            else:
                f = 10.0 ** rng.uniform(-6, 0)
                a, b = cr.psd_pair(rng, c.dim, "interior")
                s[r], z[r] = f * a, it.mu / f * b
    it.s, it.z = s, z
    return it


class Rhs:
    pass


def rhs_for(pb, it, seed=RHS_SEED):
    rng = np.random.default_rng(seed)
    r = Rhs()
    r.x, r.z = rng.standard_normal(pb.n), rng.standard_normal(pb.m)
    r.s = it.mu * rng.standard_normal(pb.m)
    r.tau, r.kappa = 0.4, -0.2
    return r


# ---------------------------------------------------------------------------------------------------------------------
#  what a handle shows: K, the scaling, its refinement settings and a level-B solve
# ---------------------------------------------------------------------------------------------------------------------
class View:
    def __init__(self, pb, Ktriu, sc, abstol, reltol, solve):
        Ktriu = sp.csc_matrix(Ktriu)
        self.pb, self.sc, self.abstol, self.reltol, self.solve = pb, sc, abstol, reltol, solve
        self.K = sym_from_triu(Ktriu.indptr, Ktriu.indices, Ktriu.data)
        nm = pb.n + pb.m
        self.N = self.K.shape[0]
        Kc = self.K.tocsc()
        self.K11 = sp.csr_matrix(self.K[:nm, :][:, :nm])
        self.K12 = sp.csr_matrix(self.K[:nm, :][:, nm:])
        self.K21 = sp.csr_matrix(self.K[nm:, :][:, :nm])
        K22 = sp.csr_matrix(self.K[nm:, :][:, nm:])
        for M in (self.K11, self.K12, self.K21):
            M.sort_indices()
        self.d22 = K22.diagonal()
        assert (K22 - sp.diags(self.d22)).count_nonzero() == 0 and (self.N == nm or np.all(self.d22 != 0)), \
            "the extra block of K is expected to be diagonal"
        del Kc
        self.rowlen = np.diff(self.K.indptr)
        self._x2z2 = None

    def x2z2_mag(self):
        if self._x2z2 is None:
            x2, z2 = self.solve(-self.pb.q, self.pb.b)
            self._x2z2 = (np.abs(x2), np.abs(z2))
        return self._x2z2


def oracle_view(pb, o, exact_solve=False):
    """the CPU oracle as a handle: its K, its scaling, its refined solve (exact_solve: sparse LU with two refinement steps
    whose residual is formed in long double)"""
    sc = sr.Scaling(pb.cones, *o.scaling_w(), o.cone_lambda(), o.psd_scaling())
    st = o._settings

    def solve(rx, rz):
        o.kktsolver_setrhs(rx, rz)
        ok, x, z = o.kktsolver_solve()
        assert ok
        return x.copy(), z.copy()
    v = View(pb, o.K(), sc, st.ir_abstol, st.ir_reltol, solve)
    if exact_solve:
        v.solve = ExactSolve(v)
    return v


def device_view(pb, ks):
    lam, psd = ks.scaling()
    w, eta = ks.scaling_w()
    sc = sr.Scaling(pb.cones, w, eta, lam, psd)

    def solve(rx, rz):
        ks.kktsolver_setrhs(rx, rz)
        x, z = np.zeros(pb.n), np.zeros(pb.m)
        assert ks.kktsolver_solve(x, z)
        return x, z
    return View(pb, ks.KKT(), sc, ks.settings.iterative_refinement_abstol, ks.settings.iterative_refinement_reltol, solve)


class ExactSolve:
    """K \\ (rx, rz) to the rounding of the stored solution: sparse LU, then two refinement steps on a long-double residual"""

    def __init__(self, view):
        self.v = view
        self.Kc = view.K.tocsc()
        self.lu = spla.splu(self.Kc) if view.N else None
        self.Kl = (view.K.data.astype(np.longdouble), view.K.indices, view.K.indptr)

    def _resid(self, b, x):
        d, idx, ptr = self.Kl
        prod = d * x.astype(np.longdouble)[idx]
        Kx = np.add.reduceat(np.r_[prod, np.longdouble(0)], ptr[:-1]) if len(prod) else np.zeros(len(b), np.longdouble)
        Kx[np.diff(ptr) == 0] = 0
        return (b.astype(np.longdouble) - Kx).astype(np.float64)

    def __call__(self, rx, rz):
        n, m, N = self.v.pb.n, self.v.pb.m, self.v.N
        b = np.concatenate([rx, rz, np.zeros(N - n - m)])
        x = self.lu.solve(b)
        for _ in range(2):
            x = x + self.lu.solve(self._resid(b, x))
        return x[:n].copy(), x[n:n + m].copy()


# ---------------------------------------------------------------------------------------------------------------------
#  cone operations at extended precision from the handle's scaling
# ---------------------------------------------------------------------------------------------------------------------
def _cong(G, X):
    """G X G' (mpmath), G fp64 taken as exact, X an mpmath matrix: X is split into hi + lo doubles and both congruences
    are exact integer matrix products"""
    k = G.shape[0]
    hi = np.array([[float(X[i, j]) for j in range(k)] for i in range(k)])
    lo = np.array([[float(X[i, j] - MP.mpf(hi[i, j])) for j in range(k)] for i in range(k)])
    Gi, eg = sr._dyadic(G)
    out = MP.matrix(k, k)
    for part in (hi, lo):
        Xi, ex = sr._dyadic(part)
        Pm = Gi.dot(Xi).dot(Gi.T)
        for i in range(k):
            for j in range(k):
                out[i, j] += MP.ldexp(MP.mpf(int(Pm[i, j])), 2 * eg + ex)
    return out


def _svec_mp(M, k):
    return sr._svec_mp(M, k)


def _soc_const(lam, w, eta, d):
    """W (lambda \\ d), W symmetric: y = lambda \\ d from lambda o y = d, then W y"""
    lm, wm, dm, e = sr._mpv(lam), sr._mpv(w), sr._mpv(d), MP.mpf(float(eta))
    l1d1 = MP.fsum(a * b for a, b in zip(lm[1:], dm[1:]))
    res = lm[0] * lm[0] - MP.fsum(a * a for a in lm[1:])
    y0 = (lm[0] * dm[0] - l1d1) / res
    y = [y0] + [(dm[i] - y0 * lm[i]) / lm[0] for i in range(1, len(lm))]
    w1y = MP.fsum(a * b for a, b in zip(wm[1:], y[1:]))
    return [e * (wm[0] * y[0] + w1y)] + [e * (y[i] + (y[0] + w1y / (1 + wm[0])) * wm[i]) for i in range(1, len(lm))]


def _soc_hs(w, eta, x):
    wm, xm, e2 = sr._mpv(w), sr._mpv(x), MP.mpf(float(eta)) ** 2
    c = 2 * MP.fsum(a * b for a, b in zip(wm, xm))
    return [e2 * ((-xm[i] if i == 0 else xm[i]) + c * wm[i]) for i in range(len(wm))]


def _psd_const(lam_k, R, d, k, fault=False):
    X = cr._smat_mp(d, k)
    if fault and k >= 2:                                     # one off-diagonal entry unpacked with 1 instead of 1 / sqrt(2)
        X[0, k - 1] = X[k - 1, 0] = MP.mpf(float(d[(k - 1) * k // 2]))
    lm = sr._mpv(lam_k)
    for i in range(k):
        for j in range(k):
            X[i, j] = 2 * X[i, j] / (lm[i] + lm[j])
    return _svec_mp(_cong(R, X), k)


def _psd_hs(R, x, k):
    return _svec_mp(_cong(R, _cong(R.T, cr._smat_mp(x, k))), k)


def _abs_hs_dz(c, sc, i, r, tri, dz):
    """|Hs| |dz| of one second-order or PSD cone"""
    a = np.abs(dz[r])
    if c.kind == 2:
        w = np.abs(sc.w[r])
        return float(sc.eta[i]) ** 2 * (2 * w * (w @ a) + a)
    A = np.abs(tri[0]) @ np.abs(tri[0]).T
    return cr.svec(A @ cr.smat(a, c.dim) @ A)


class Const:
    """c of one step: hi + lo doubles per row, |c^ - c| allowed per row, and its mpmath / Fraction values per cone"""


def const_term(pb, sc, it, rhs, affine, psd_fault=False):
    m = pb.m
    out = Const()
    out.hi, out.lo, out.err, out.val = np.zeros(m), np.zeros(m), np.zeros(m), [None] * len(pb.cones)
    for c, i, r, tri in sc.pieces():
        k = c.numel
        if k == 0:
            continue
        if affine:
            out.hi[r] = it.s[r]
            out.val[i] = [_F(v) for v in it.s[r]]
            continue
        if c.kind == 0:
            out.val[i] = [Fraction(0)] * k
        elif c.kind == 1:
            out.val[i] = [_F(a) / _F(b) for a, b in zip(rhs.s[r], it.z[r])]
        elif c.kind == 2:
            out.val[i] = _soc_const(sc.lam[r], sc.w[r], sc.eta[i], rhs.s[r])
        else:
            out.val[i] = _psd_const(tri[2], tri[0], rhs.s[r], c.dim, psd_fault)
        hl = [_split(v) for v in out.val[i]]
        out.hi[r], out.lo[r] = [h for h, _ in hl], [l for _, l in hl]
        if c.kind == 1:
            out.err[r] = U * np.abs(out.hi[r])
        elif c.kind >= 2:
            fam = "c_soc" if c.kind == 2 else "c_psd"
            out.err[r] = DEVICE_FACTOR * NUMPY_WORST[fam] * U * np.abs(out.hi[r]).max()
    return out


# ---------------------------------------------------------------------------------------------------------------------
#  the four defects: exact values and bounds
# ---------------------------------------------------------------------------------------------------------------------
def _absm(M):
    return sp.csr_matrix((np.abs(M.data), M.indices, M.indptr), shape=M.shape)


def _neg(g):
    return ([-v for v in g[0]], [-v for v in g[1]], g[2])


def defect1(view, it, rhs, const, step):
    """(|defect| per row of (x, z), bound per row)"""
    pb = view.pb
    n, m = pb.n, pb.m
    nm, N = n + m, view.N
    dx, dz, ds, dtau, dkappa = step
    sol = np.concatenate([dx, dz])
    # the eliminated variables from their own rows: K21 sol + K22 p = 0
    ne = N - nm
    if ne:
        th, tl = _fsum_rows(ne, [_prod_lists(view.K21, sol, 1.0)], [])
        pf = [-(_F(a) + _F(b)) / _F(d) for a, b, d in zip(th, tl, view.d22)]
        ph = np.array([_split(v)[0] for v in pf])
        pl = np.array([_split(v)[1] for v in pf])
    else:
        ph = pl = np.zeros(0)
    groups = [_prod_lists(view.K11, sol, 1.0)]
    if ne:
        groups += [_prod_lists(view.K12, ph, 1.0)]
        if np.any(pl != 0):
            plz = np.where(np.abs(pl) < 1e-250, 0.0, pl)
            groups += [_prod_lists(view.K12, plz, 1.0)]
    tq = two_product(np.full(n, dtau), pb.q)
    tb = two_product(np.full(m, dtau), pb.b)
    ex = [np.r_[-rhs.x, -const.hi].tolist(), np.r_[np.zeros(n), -const.lo].tolist(), np.r_[np.zeros(n), rhs.z].tolist(),
          np.r_[tq[0], -tb[0]].tolist(), np.r_[tq[1], -tb[1]].tolist()]
    hi, lo = _fsum_rows(nm, groups, ex)
    val = np.abs(hi + lo)
    # ---- bound
    X2, Z2 = view.x2z2_mag()
    Ka = _absm(view.K)
    K12a, K21a = _absm(view.K12), _absm(view.K21)
    d22i = 1.0 / np.abs(view.d22) if ne else np.zeros(0)
    top2 = np.r_[X2, Z2]
    M2 = np.r_[top2, d22i * (K21a @ top2)] if ne else top2
    M1 = np.r_[np.abs(sol), np.abs(ph)] + abs(dtau) * M2
    cz = np.abs(const.hi - rhs.z)
    b1 = np.r_[np.abs(rhs.x), cz + const.err, np.zeros(ne)]
    b2 = np.r_[np.abs(pb.q), np.abs(pb.b), np.zeros(ne)]
    tol1 = view.abstol + view.reltol * (b1.max() if N else 0.0) * (1 + 8 * U)
    tol2 = view.abstol + view.reltol * (b2.max() if N else 0.0)
    g = gamma(view.rowlen + 1)
    B = (tol1 + abs(dtau) * tol2) + g * (b1 + Ka @ M1) + abs(dtau) * g * (b2 + Ka @ M2) + gamma(2) * (Ka @ (M1 + abs(dtau) * M2))
    B[n:nm] += U * cz + const.err
    bound = B[:nm] + (K12a @ (d22i * B[nm:]) if ne else 0.0)
    return val, bound * (1 + 1e-9)


def _quad(pb, a, b):
    """a.P b exactly as (hi, lo): the rows of P b as hi + lo, then two exact dot products"""
    if pb.n == 0:
        return 0.0, 0.0
    h, l = _fsum_rows(pb.n, [_prod_lists(pb.Pfull, b, 1.0)], [])
    h1, l1 = dot_exact(a, h)
    l = np.where(np.abs(l) < 1e-250, 0.0, l)
    h2, l2 = dot_exact(a, l)
    return h1, math.fsum([l1, h2, l2])


def defect2_fraction(pb, it, rhs, step, Pfull=None):
    """the tau row as a Fraction, exact up to the u^2 tails of the dot products"""
    dx, dz, ds, dtau, dkappa = step
    if Pfull is not None:
        pb = _WithP(pb, Pfull)
    tau, kappa = _F(it.tau), _F(it.kappa)
    S = lambda hl: _F(hl[0]) + _F(hl[1])
    qd, bd = S(dot_exact(pb.q, dx)), S(dot_exact(pb.b, dz))
    xPd, xPx = S(_quad(pb, it.x, dx)), S(_quad(pb, it.x, it.x))
    return _F(rhs.tau) - _F(rhs.kappa) / tau + qd + bd + 2 * xPd / tau - _F(dtau) * (kappa / tau + xPx / (tau * tau))


class _WithP:
    def __init__(self, pb, Pfull):
        self.q, self.b, self.n, self.m, self.Pfull = pb.q, pb.b, pb.n, pb.m, Pfull


def defect2(view, it, rhs, step, Pfull=None):
    pb = view.pb
    dx, dz, ds, dtau, dkappa = step
    val = abs(float(defect2_fraction(pb, it, rhs, step, Pfull)))
    n, m, kP, tau = pb.n, pb.m, pb.kP, it.tau
    Pa = _absm(pb.Pfull if Pfull is None else Pfull)
    X2, Z2 = view.x2z2_mag()
    X1, Z1 = np.abs(dx) + abs(dtau) * X2, np.abs(dz) + abs(dtau) * Z2
    ax = np.abs(it.x)
    XM = ax / tau + X2
    aq, ab = np.abs(pb.q), np.abs(pb.b)
    g = lambda k: float(gamma(k + 2))
    g8, g3, g2 = float(gamma(8)), float(gamma(3)), float(gamma(2))
    xPX1 = float(ax @ (Pa @ X1)) if n else 0.0
    qX1, bZ1, qX2, bZ2 = float(aq @ X1), float(ab @ Z1), float(aq @ X2), float(ab @ Z2)
    mPm, x2Px2 = (float(XM @ (Pa @ XM)), float(X2 @ (Pa @ X2))) if n else (0.0, 0.0)
    magN = abs(rhs.tau) + abs(rhs.kappa) / tau + qX1 + bZ1 + 2 / tau * xPX1
    magD = it.kappa / tau + qX2 + bZ2 + mPm + x2Px2
    eN = g(n) * qX1 + g(m) * bZ1 + 2 / tau * g(n + kP) * xPX1 + g8 * magN
    eD = g(n) * qX2 + g(m) * bZ2 + (g(n + kP) + 2 * g3) * mPm + g(n + kP) * x2Px2 + g8 * magD
    bound = eN + abs(dtau) * (eD + U * magD) + g2 * (qX1 + bZ1 + 2 / tau * xPX1)
    return val, bound * (1 + 1e-6)


def defect3(it, rhs, step):
    dtau, dkappa = step[3], step[4]
    val = abs(float(_F(dkappa) + (_F(rhs.kappa) + _F(it.kappa) * _F(dtau)) / _F(it.tau)))
    return val, float(gamma(3)) * (abs(rhs.kappa) + abs(it.kappa * dtau)) / it.tau * (1 + 1e-9)


def defect4(view, it, rhs, const, step, affine, factor=DEVICE_FACTOR):
    """(|defect| per row, bound per row, {family: worst |defect| / (u natural scale)} of the second-order and PSD cones)"""
    pb, sc = view.pb, view.sc
    dx, dz, ds, dtau, dkappa = step
    val, bound, fam = np.zeros(pb.m), np.zeros(pb.m), {}
    for c, i, r, tri in sc.pieces():
        k = c.numel
        if k == 0:
            continue
        cv = const.val[i]
        if c.kind == 0:
            val[r] = [abs(float(_F(a) + b)) for a, b in zip(ds[r], cv)]
        elif c.kind == 1:
            w = sc.w[r]
            val[r] = [abs(float(_F(a) + _F(ww) * _F(ww) * _F(d) + b)) for a, ww, d, b in zip(ds[r], w, dz[r], cv)]
            bound[r] = float(gamma(4)) * (w * w * np.abs(dz[r]) + np.abs(const.hi[r]))
        else:
            hs = _soc_hs(sc.w[r], sc.eta[i], dz[r]) if c.kind == 2 else _psd_hs(tri[0], dz[r], c.dim)
            cm = [MP.mpf(v.numerator) / MP.mpf(v.denominator) if isinstance(v, Fraction) else v for v in cv]
            val[r] = [abs(float(MP.mpf(float(a)) + h + b)) for a, h, b in zip(ds[r], hs, cm)]
            scale = U * float(np.max(_abs_hs_dz(c, sc, i, r, tri, dz) + np.abs(const.hi[r])))
            name = "ds_soc" if c.kind == 2 else "ds_psd"
            bound[r] = factor * NUMPY_WORST[name] * scale
            fam[name] = max(fam.get(name, 0.0), float(val[r].max()) / scale if scale > 0 else 0.0)
    return val, bound, fam


def step_ratios(view, it, rhs, step, affine, share=1.0, Pfull=None, which=(1, 2, 3, 4), stop_above=None):
    """{defect number: worst |defect| / (share * bound)} of one step, evaluated in the order of `which` (stop_above: no
    further defect is evaluated once one exceeds it -- the fault tests, which only need one).  share < 1 (the restatement): at least the rounding of
    the stored values themselves is allowed -- u |ds| in (4), u |dkappa| in (3)."""
    cache = view.__dict__.setdefault("_const", {})
    key = (id(it), id(rhs), affine)
    if key not in cache:
        cache[key] = (const_term(view.pb, view.sc, it, rhs, affine), it, rhs)
    const = cache[key][0]
    dx, dz, ds, dtau, dkappa = step
    out = {}
    ok = all(np.isfinite(v).all() for v in (dx, dz, ds)) and math.isfinite(dtau) and math.isfinite(dkappa)
    if not ok:
        return {k: math.inf for k in which}
    for d in which:
        if d == 1:
            v, b = defect1(view, it, rhs, const, step)
            out[1] = ratio(v, share * b)
        elif d == 2:
            v, b = defect2(view, it, rhs, step, Pfull)
            out[2] = ratio(v, share * b)
        elif d == 3:
            v, b = defect3(it, rhs, step)
            out[3] = ratio(v, max(share * b, U * abs(dkappa)) if share < 1 else b)
        else:
            v, b, _ = defect4(view, it, rhs, const, step, affine)
            out[4] = ratio(v, np.maximum(share * b, U * np.abs(ds)) if share < 1 else b)
        if stop_above is not None and out[d] > stop_above:
            break
    return out


# ---------------------------------------------------------------------------------------------------------------------
#  numpy restatement of kkt_solve! and kkt_solve_initial_point!, and simulated faults
# ---------------------------------------------------------------------------------------------------------------------
STEP_FAULTS = ("drop_P_entry", "drop_xm_row", "drop_dots_block", "stale_cache", "stale_x2_tail", "no_2", "flip_rhs_z",
               "psd_offdiag", "swap_kappa_tau")
INIT_FAULTS = ("lp_plus_s", "lp_reuse_z")


def fault_applies(pb, fault, affine=False):
    """the (builder, fault) pairs that cannot occur: no P entry to drop, no 2 xi.P x1 term and no pair 3 when P is empty, no z block
    without rows, no PSD fault without a PSD cone of side >= 2 or on the affine step (c = s there), LP faults off the LP branch"""
    if fault in ("drop_P_entry", "no_2", "drop_xm_row"):      # (pair 3 is (xi - x2).P (xi - x2): zero without P)
        return pb.P.nnz > 0 and bool(np.any(pb.P.data != 0))
    if fault in ("flip_rhs_z", "stale_cache", "stale_x2_tail"):   # (without cones K does not depend on (s, z): nothing is stale)
        return pb.m > 0
    if fault == "psd_offdiag":
        return (not affine) and any(c.kind == 3 and c.dim >= 2 for c in pb.cones)
    if fault in INIT_FAULTS:
        return pb.P.nnz == 0 and pb.m > 0
    return True


def host_cones(pb, sc):
    """the fp64 numpy cone classes of cuclarabel_amd/ipm.py carrying the handle's scaling"""
    from cuclarabel_amd import ipm
    cones = ipm._make_cones(pb.cones)
    for (c, i, r, tri), h in zip(sc.pieces(), cones):
        if c.kind == 1:
            h.w, h.lam = sc.w[r].copy(), sc.lam[r].copy()
        elif c.kind == 2:
            h.w, h.lam, h.eta = sc.w[r].copy(), sc.lam[r].copy(), float(sc.eta[i])
        elif c.kind == 3:
            h.R, h.Rinv, h.lam = tri[0].copy(), tri[1].copy(), tri[2].copy()
    return cones


def _last_block(length):
    """the entries of a k_dots pair that its last working workgroup adds (64 workgroups of 256, grid-strided)"""
    i = np.arange(length)
    blk = (i // 256) % DOT_BLOCKS
    return blk == blk.max()


def restate_step(view, it, rhs, affine, fault=None, prev=None):
    """kkt_solve! in plain numpy on view.solve (an exact-enough K^-1) -> (dx, dz, ds, dtau, dkappa), all fp64.  The algebra
    around the solves and the nonnegative rows are evaluated in long double and rounded once (as in
    tests/iterate_reference.py); second-order and PSD cones go through the fp64 classes of cuclarabel_amd/ipm.py.
    prev: the view of the previous (s, z) on the same problem (the stale faults)."""
    pb = view.pb
    n, m = pb.n, pb.m
    L = np.longdouble
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    cones = host_cones(pb, view.sc)
    P = pb.Pfull.astype(L)
    q, b, x = pb.q.astype(L), pb.b.astype(L), it.x.astype(L)
    x2, z2 = view.solve(-pb.q, pb.b)
    x2c, z2c = x2, z2                                        # what the cached terms were formed from
    if fault == "stale_cache":
        x2c, z2c = prev.solve(-pb.q, pb.b)
    if fault == "stale_x2_tail":
        old = np.concatenate(prev.solve(-pb.q, pb.b))
        v = np.concatenate([x2, z2])
        t0 = 256 * ((n + m - 1) // 256)
        v[t0:] = old[t0:]
        x2, z2 = v[:n], v[n:]
    const = np.zeros(m, dtype=L)
    for h in cones:
        if h.n == 0:
            continue
        if affine:
            const[h.rng] = it.s[h.rng]
        elif h.spec.kind == 1:
            const[h.rng] = rhs.s[h.rng].astype(L) / it.z[h.rng].astype(L)
        elif fault == "psd_offdiag" and h.spec.kind == 3 and h.k >= 2:
            from cuclarabel_amd import ipm
            k = h.k
            X = ipm._svec_to_mat(rhs.s[h.rng], k)
            X[0, k - 1] = X[k - 1, 0] = rhs.s[h.rng][(k - 1) * k // 2]
            X = 2.0 * X / (h.lam[:, None] + h.lam[None, :])
            const[h.rng] = ipm._mat_to_svec(h.R @ X @ h.R.T)
        else:
            const[h.rng] = h.ds_from_dz_offset(rhs.s[h.rng].copy(), it.z[h.rng].copy())
    rz = const - rhs.z.astype(L)
    if fault == "flip_rhs_z":
        r = next(r for c, _, r in pb.offsets() if c.numel)
        rz[r] = const[r] + rhs.z[r]
    x1, z1 = (v.astype(L) for v in view.solve(rhs.x, f64(rz)))
    x2, z2, x2c, z2c = (v.astype(L) for v in (x2, z2, x2c, z2c))
    Px1 = P @ x1
    if fault == "drop_P_entry":
        Pd = P.copy()
        e = np.flatnonzero(Pd.data != 0)
        Pd.data[e[len(e) // 2]] = 0.0
        Px1 = Pd @ x1
    tau, kappa = L(it.tau), L(it.kappa)
    qx1 = q @ x1
    if fault == "drop_dots_block":
        keep = ~_last_block(n)
        qx1 = q[keep] @ x1[keep]
    tnum = L(rhs.tau) - L(rhs.kappa) / tau + qx1 + b @ z1 + (1.0 if fault == "no_2" else 2.0) * ((x @ Px1) / tau)
    xm = x / tau - x2
    Pxm = P @ xm
    xmd = xm.copy()
    if fault == "drop_xm_row":
        xmd[n // 2] = 0.0
    c0, c1, c2 = q @ x2c, b @ z2c, x2c @ (P @ x2c)
    tden = kappa / tau - c0 - c1
    tden += xmd @ Pxm - c2
    dtau = L(float(tnum / tden))
    dx, dz = f64(x1 + dtau * x2), f64(z1 + dtau * z2)
    ds = np.zeros(m)
    for h in cones:
        if h.n == 0:
            continue
        if h.spec.kind == 1:                                  # (long double: the rounding of the stored ds is all that is left)
            w = h.w.astype(L)
            ds[h.rng] = f64(-(w * w * dz[h.rng].astype(L) + const[h.rng]))
        else:
            ds[h.rng] = -(h.mul_Hs(dz[h.rng]) + f64(const[h.rng]))
    dkappa = -(L(rhs.kappa) + tau * dtau) / kappa if fault == "swap_kappa_tau" else -(L(rhs.kappa) + kappa * dtau) / tau
    return dx, dz, ds, float(dtau), float(dkappa)


def restate_initial_point(pb, solve, fault=None):
    """kkt_solve_initial_point! (kktsystem.jl:96-140) on `solve` -> (x, s, z)"""
    if pb.P.nnz == 0:
        x, ms = solve(np.zeros(pb.n), pb.b)
        s = ms.copy() if fault == "lp_plus_s" else -ms
        _, z = solve(-pb.q, pb.b.copy() if fault == "lp_reuse_z" else np.zeros(pb.m))
        return x, s, z
    x, z = solve(-pb.q, pb.b)
    return x, -z, z


def initial_point_mismatches(pb, solve, x, s, z):
    """entries of (x, s, z) that are not bit for bit the level-B solves of the exact right-hand sides on the same handle:
    (-q, b) -> (x, z), s = -z; without P (0, b) -> (x, -s), then (-q, 0) -> z.  The right-hand sides are data: no tolerance."""
    eq = lambda a, b: int(np.sum(np.asarray(a).view(np.int64) != np.asarray(b).view(np.int64)))
    f = lambda v: np.ascontiguousarray(v, dtype=np.float64) + 0.0          # (-0.0 and 0.0 compare as numbers)
    if pb.P.nnz == 0:
        xa, za = solve(np.zeros(pb.n), pb.b)
        _, zb = solve(-pb.q, np.zeros(pb.m))
        return eq(f(x), f(xa)) + eq(f(s), f(-za)) + eq(f(z), f(zb))
    xa, za = solve(-pb.q, pb.b)
    return eq(f(x), f(xa)) + eq(f(z), f(za)) + eq(f(s), f(-za))


# ---------------------------------------------------------------------------------------------------------------------
#  host cases: the oracle as the handle
# ---------------------------------------------------------------------------------------------------------------------
_HOST = {}


def host_view(name, scale, seed=ITERATE_SEED):
    """(problem, iterate, rhs, view with exact solves, oracle) of one host case; built once and shared"""
    key = (name, scale, seed)
    if key not in _HOST:
        from tests.oracle_bindings import OracleKKT
        pb = problem(name)
        it = iterate(pb, scale, seed)
        o = OracleKKT(pb.P, pb.A, pb.cones)
        assert o.update_scaling(it.s, it.z) and o.kktsolver_update(), f"{name}/{scale}: the oracle could not factor K"
        _HOST[key] = (pb, it, rhs_for(pb, it), oracle_view(pb, o, exact_solve=True), o)
    return _HOST[key]


def measure():
    """the ratios behind NUMPY_WORST: the numpy restatement's defect (4) and its c against the extended-precision values"""
    worst = dict(ds_soc=0.0, ds_psd=0.0, c_soc=0.0, c_psd=0.0)
    for name in BUILDERS:
        for scale in SCALES:
            pb, it, rhs, view, _ = host_view(name, scale)
            if not any(c.kind >= 2 for c in pb.cones):
                continue
            for affine in (True, False):
                step = restate_step(view, it, rhs, affine)
                const = const_term(pb, view.sc, it, rhs, affine)
                fam = defect4(view, it, rhs, const, step, affine)[2]
                if not affine:
                    cones = host_cones(pb, view.sc)
                    for (c, i, r, tri), h in zip(view.sc.pieces(), cones):
                        if c.kind >= 2 and c.numel:
                            got = h.ds_from_dz_offset(rhs.s[r].copy(), it.z[r].copy())
                            e = np.abs((got - const.hi[r]) - const.lo[r]).max() / (U * np.abs(const.hi[r]).max())
                            key = "c_soc" if c.kind == 2 else "c_psd"
                            fam[key] = max(fam.get(key, 0.0), float(e))
                for k, v in fam.items():
                    worst[k] = max(worst[k], v)
                print(f"{name:12s} {scale:5s} {'affine' if affine else 'combined':8s}", {k: round(v, 3) for k, v in fam.items()})
    print("NUMPY_WORST =", {k: round(v, 3) for k, v in worst.items()})
    return worst


if __name__ == "__main__":
    if sys.argv[1:] == ["measure"]:
        measure()
