"""Host reference for hipkkt_kkt_system_residuals (csrc/iterate_kernels.hip): exact residual vectors, exact dot products
and norms, order-free a-priori bounds, problems with prescribed row lengths, a plain numpy restatement and simulated kernel
faults -- TEST INFRASTRUCTURE ONLY.

    Px = Symmetric(P) x     rx_inf = -A'z     rz_inf = A x + s     rx = rx_inf - Px - q tau     rz = rz_inf - b tau

Exact values as in tests/residual_reference.py: every product is split without error into two doubles (two_product) and
math.fsum returns the correctly rounded exact sum, so each vector entry comes as hi + lo, exact to ~u^2 of the row's
magnitude.  Norms are exact integers: every double is mantissa * 2^exponent, the squares of the products are added as
Python integers and only the final square root is taken in mpmath at 60 digits -- any finite range, 1e200 and 1e-200
included.

Bounds (u = 2^-53, gamma_j = j u / (1 - j u), k = the entries the kernel walks in the row: a whole x row of the image --
P's row with its structural diagonal, then A's column --, the A prefix of a z row); each is the textbook bound of an inner
product of that length in ANY summation order, with or without fma (Higham, Accuracy and Stability, 2nd ed., (3.5)),
followed by the two or three roundings of the elementwise tail:
    |dPx_i|     <= gamma_{k+1} sum |P_ij| |x_j|
    |drx_inf_i| <= gamma_{k+1} sum |A_ji| |z_j|
    |drz_inf_i| <= gamma_{k+2} (sum |A_ij| |x_j| + |s_i|)
    |drx_i|     <= gamma_{k+4} (sum |A_ji| |z_j| + sum |P_ij| |x_j| + |q_i| tau)
    |drz_i|     <= gamma_{k+4} (sum |A_ij| |x_j| + |s_i| + |b_i| tau)
Scalars are judged against exact values formed from the vectors the device RETURNED, so that a vector error and a
reduction error are told apart:
    a dot product of length L: gamma_{L+1} sum |a_i b_i|          a norm: relative gamma_{L+4}
"""
import math

import mpmath
import numpy as np
import scipy.sparse as sp

from tests.residual_reference import U, gamma, two_product, LONG_ROW, LONG_CHUNK

VECTORS = ("Px", "rx_inf", "rz_inf", "rx", "rz")
SCALARS = ("qx", "bz", "sz", "xPx", "n_dx", "n_ez", "n_einv_s", "n_dinv_rx_inf", "n_dinv_Px", "n_einv_rz_inf", "n_einv_rz",
           "n_dinv_rx")
LANES = 8                   # lanes per row of k_iterate_residuals
ROWS_PER_WG = 32
GRID_CAP = 2048             # kIterGridCap
ELEM_GRID_CAP = 2048        # workgroups of 256 of the elementwise kernels
EDGE_LENGTHS = (0, 1, 7, 8, 9, 64, 65)
LONG_EDGES = (LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, 3 * LONG_CHUNK + 1)


class Parts:
    """What the kernel walks, from (triu P, A): Symmetric(P), A and A' as CSR, and the walked entry counts per row."""

    def __init__(self, P, A):
        P = sp.triu(sp.csc_matrix(P), format="csc")
        A = sp.csc_matrix(A)
        self.n, self.m = P.shape[0], A.shape[0]
        n = self.n
        self.P = sp.csr_matrix(P + sp.triu(P, 1, format="csc").T)
        self.A = sp.csr_matrix(A)
        self.At = sp.csr_matrix(A.T)
        for M in (self.P, self.A, self.At):
            M.sort_indices()
        # structural counts (explicit zeros count, and a missing diagonal of P is there as a structural zero)
        one = sp.csc_matrix((np.ones(P.nnz), P.indices, P.indptr), shape=P.shape)
        pat = sp.csr_matrix(one + sp.triu(one, 1, format="csc").T + sp.identity(n, format="csc"))
        self.kP = np.diff(pat.indptr).astype(np.int64) if n else np.zeros(0, np.int64)
        Apat = sp.csc_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
        self.kAcol = np.diff(Apat.indptr).astype(np.int64)
        self.kx = self.kP + self.kAcol
        self.kz = np.diff(sp.csr_matrix(Apat).indptr).astype(np.int64)


class Problem:
    def __init__(self, name, P, A, cones, seed, tau=0.7):
        rng = np.random.default_rng(seed)
        self.name, self.cones, self.tau = name, cones, tau
        self.P = sp.triu(sp.csc_matrix(P), format="csc")
        self.A = sp.csc_matrix(A)
        self.P.sort_indices()
        self.A.sort_indices()
        self.n, self.m = self.P.shape[0], self.A.shape[0]
        self.q, self.x = rng.standard_normal(self.n), rng.standard_normal(self.n)
        self.b, self.s, self.z = (rng.standard_normal(self.m) for _ in range(3))
        self.parts = Parts(self.P, self.A)

    def data(self):
        return dict(q=self.q, b=self.b, x=self.x, s=self.s, z=self.z, tau=self.tau)


# ------------------------------------------------------------------------------------------------ exact values, bounds
def _prod_lists(M, v, sign):
    p, q = two_product(M.data, v[M.indices])
    assert np.isfinite(p).all() and not np.any((p != 0) & (np.abs(p) < 1e-280)), "products out of the exact split's range"
    return (sign * p).tolist(), (sign * q).tolist(), M.indptr


def _fsum_rows(nrows, groups, extras):
    hi, lo = np.empty(nrows), np.empty(nrows)
    fsum = math.fsum
    for i in range(nrows):
        t = []
        for pl, ql, ptr in groups:
            a, z = ptr[i], ptr[i + 1]
            t += pl[a:z]
            t += ql[a:z]
        for e in extras:
            t.append(e[i])
        h = fsum(t)
        t.append(-h)
        hi[i], lo[i] = h, fsum(t)
    return hi, lo


def exact_vectors(parts, q, b, x, s, z, tau):
    """name -> (hi, lo) for the five vectors."""
    n, m = parts.n, parts.m
    Px = _prod_lists(parts.P, x, 1.0)
    Atz = _prod_lists(parts.At, z, -1.0)
    Ax = _prod_lists(parts.A, x, 1.0)
    nPx = ([-v for v in Px[0]], [-v for v in Px[1]], Px[2])
    qt, bt = two_product(q, np.full(n, tau)), two_product(b, np.full(m, tau))
    return dict(Px=_fsum_rows(n, [Px], []),
                rx_inf=_fsum_rows(n, [Atz], []),
                rz_inf=_fsum_rows(m, [Ax], [s.tolist()]),
                rx=_fsum_rows(n, [Atz, nPx], [(-qt[0]).tolist(), (-qt[1]).tolist()]),
                rz=_fsum_rows(m, [Ax], [s.tolist(), (-bt[0]).tolist(), (-bt[1]).tolist()]))


def _abs(M):
    return sp.csr_matrix((np.abs(M.data), M.indices, M.indptr), shape=M.shape)


def vector_bounds(parts, q, b, x, s, z, tau):
    """name -> bound per entry.  The magnitude sums are fp64 inner products of non-negative terms themselves: rounded UP
    by their own gamma."""
    SP, SAt, SA = _abs(parts.P) @ np.abs(x), _abs(parts.At) @ np.abs(z), _abs(parts.A) @ np.abs(x)
    kx, kz = parts.kx, parts.kz

    def up(g, S, k):
        gg = gamma(k + 4)
        return g * S / (1.0 - gg)
    return dict(Px=up(gamma(kx + 1), SP, kx),
                rx_inf=up(gamma(kx + 1), SAt, kx),
                rz_inf=up(gamma(kz + 2), SA + np.abs(s), kz),
                rx=up(gamma(kx + 4), SAt + SP + np.abs(q) * tau, kx),
                rz=up(gamma(kz + 4), SA + np.abs(s) + np.abs(b) * tau, kz))


def ratio(err, bound):
    """max err / bound; an entry with bound 0 must have error 0 (-> 0), else inf."""
    err, bound = np.atleast_1d(np.asarray(err, np.float64)), np.atleast_1d(np.asarray(bound, np.float64))
    if err.size == 0:
        return 0.0
    if not np.isfinite(err).all():
        return math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def vector_ratios(pb_or_parts, data, got, exact=None, bounds=None, share=1.0):
    """name -> worst |got - exact| / (share * bound) over the five vectors.  got: name -> array.
    share < 1: an entry is allowed max(share * bound, u |exact|) -- the rounding of the stored fp64 value itself, which no
    result can avoid and which is half of gamma_2 on a row of one entry."""
    parts = getattr(pb_or_parts, "parts", pb_or_parts)
    exact = exact or exact_vectors(parts, **data)
    bounds = bounds or vector_bounds(parts, **data)
    out = {}
    for name in VECTORS:
        hi, lo = exact[name]
        g = np.asarray(got[name], np.float64)
        allowed = bounds[name] if share == 1.0 else np.maximum(share * bounds[name], U * np.abs(hi))
        out[name] = ratio(np.abs((g - hi) - lo), allowed) if np.isfinite(g).all() else math.inf
    return out


def dot_exact(a, b):
    p, q = two_product(np.asarray(a, np.float64), np.asarray(b, np.float64))
    t = p.tolist() + q.tolist()
    h = math.fsum(t)
    t.append(-h)
    return h, math.fsum(t)


def dot_bound(a, b):
    L = len(a)
    S = float(np.abs(np.asarray(a) * np.asarray(b)).sum()) if L else 0.0
    return float(gamma(L + 1)) * S / (1.0 - float(gamma(L + 2)))


def _mant_exp(v):
    m, e = np.frexp(np.asarray(v, np.float64))
    return [int(t) for t in np.ldexp(m, 53).astype(np.int64)], [int(t) - 53 for t in e]


def norm_exact(d, v):
    """||d o v||_2 as an mpmath number at 60 digits, the sum of squares exact (d None: ones).  Finite input only."""
    v = np.asarray(v, np.float64)
    assert np.isfinite(v).all() and (d is None or np.isfinite(d).all())
    mv, ev = _mant_exp(v)
    if d is None:
        md, ed = [1] * len(mv), [0] * len(mv)
    else:
        md, ed = _mant_exp(d)
    terms = [((a * b) ** 2, 2 * (ea + eb)) for a, b, ea, eb in zip(md, mv, ed, ev) if a and b]
    if not terms:
        return mpmath.mpf(0)
    emin = min(t[1] for t in terms)
    S = sum(t[0] << (t[1] - emin) for t in terms)
    with mpmath.workdps(60):
        return mpmath.sqrt(mpmath.ldexp(mpmath.mpf(S), emin))


def norm_ratio(got, d, v, share=1.0):
    """|got - ||d o v||| / (share gamma_{L+4} ||d o v||); an exact 0 must come back as exactly 0.  share < 1: at least the
    rounding u of the returned fp64 number is allowed."""
    ref = norm_exact(d, v)
    if not math.isfinite(got):
        return math.inf
    if ref == 0:
        return 0.0 if got == 0.0 else math.inf
    with mpmath.workdps(60):
        rel = float(gamma(len(v) + 4)) if share == 1.0 else max(share * float(gamma(len(v) + 4)), U)
        return float(abs(mpmath.mpf(got) - ref) / (ref * mpmath.mpf(rel)))


def scalar_ratios(data, vec, scal, equil=None, dots=True, share=1.0):
    """name -> error / bound for the twelve scalars `scal` (in SCALARS order), against exact values formed from the
    vectors `vec` the device returned.  equil: (d, dinv, e, einv) or None.  dots=False: norms only (a range test whose
    products leave the exact split's range)."""
    q, b, x, s, z = (data[k] for k in ("q", "b", "x", "s", "z"))
    d, dinv, e, einv = equil if equil is not None else (None,) * 4
    out = {}
    if dots:
        for name, a, c, got in (("qx", q, x, scal[0]), ("bz", b, z, scal[1]), ("sz", s, z, scal[2]), ("xPx", x, vec["Px"], scal[3])):
            hi, lo = dot_exact(a, c)
            allowed = dot_bound(a, c) if share == 1.0 else max(share * dot_bound(a, c), U * abs(hi))
            out[name] = ratio(abs((got - hi) - lo), allowed)
    for name, w, v, got in (("n_dx", d, x, scal[4]), ("n_ez", e, z, scal[5]), ("n_einv_s", einv, s, scal[6]),
                            ("n_dinv_rx_inf", dinv, vec["rx_inf"], scal[7]), ("n_dinv_Px", dinv, vec["Px"], scal[8]),
                            ("n_einv_rz_inf", einv, vec["rz_inf"], scal[9]), ("n_einv_rz", einv, vec["rz"], scal[10]),
                            ("n_dinv_rx", dinv, vec["rx"], scal[11])):
        out[name] = norm_ratio(float(got), w, v, share)
    return out


# ------------------------------------------------------------------------------------------------ numpy restatement, faults
def restate(parts, q, b, x, s, z, tau, equil=None, fault=None, A_stale=None, dtype=np.float64):
    """The five vectors and twelve scalars in plain numpy -> (dict of vectors, array of 12), all fp64.  fault: None or one of
    FAULTS -- what a wrong kernel would return.  dtype: the type the expressions are evaluated in before the one rounding
    to fp64 (np.longdouble: the x87 format's 64-bit significand leaves that final rounding, half an ulp, as the only
    error of note; a row of ONE entry evaluated in fp64 may use half of its gamma_2 by itself)."""
    T = lambda v: np.asarray(v, dtype=dtype)
    M = lambda S: S.astype(dtype)
    A, At = parts.A, parts.At
    if fault == "drop_A_entry":                     # one entry of A not walked (from the middle of its row and column)
        A = A.copy()
        k = A.nnz // 2
        A.data[k] = 0.0
        At = sp.csr_matrix(A.T)
    if fault == "stale_A":                          # the values before hipkkt_kkt_update_A
        A, At = A_stale.A, A_stale.At
    P, A, At = M(parts.P), M(A), M(At)
    q, b, x, s, z = T(q), T(b), T(x), T(s), T(z)
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    Px = P @ x
    rx_inf = At @ z if fault == "plus_Atz" else -(At @ z)
    rz_inf = A @ x if fault == "no_s" else A @ x + s
    if fault == "hs_leak":                          # the -Hs diagonal behind the A prefix walked as well (Hs = I)
        rz_inf = rz_inf - z
    t = 1.0 if fault == "no_tau" else tau
    rx = rx_inf - Px - q * dtype(t)
    rz = rz_inf - b * dtype(t)
    vec = dict(Px=f64(Px), rx_inf=f64(rx_inf), rz_inf=f64(rz_inf), rx=f64(rx), rz=f64(rz))
    d, dinv, e, einv = (T(v) for v in equil) if equil is not None else (dtype(1.0),) * 4
    nrm = np.linalg.norm
    # (the scalars from the ROUNDED vectors, as the kernel forms them from what it stored)
    v = {k: T(a) for k, a in vec.items()}
    scal = f64([q @ x, b @ z, s @ z, x @ v["Px"], nrm(d * x), nrm(e * z), nrm(einv * s), nrm(dinv * v["rx_inf"]),
                nrm(dinv * v["Px"]), nrm(einv * v["rz_inf"]), nrm(einv * v["rz"]), nrm(dinv * v["rx"])])
    return vec, scal


FAULTS = ("drop_A_entry", "no_tau", "plus_Atz", "no_s", "hs_leak", "stale_A")


def stale_parts(pb):
    """The problem's parts with the values A had before an update: every entry 0.1 % off."""
    A = pb.A.copy()
    A.data = A.data * (1.0 + 1e-3)
    return Parts(pb.P, A)


# ------------------------------------------------------------------------------------------------ problems
def _vals(rng, k):
    return rng.uniform(0.5, 1.5, k) * rng.choice([-1.0, 1.0], k)


def _cones(m, nzero):
    from cuclarabel_amd.cones import NonnegativeConeT, ZeroConeT
    out = []
    if nzero:
        out.append(ZeroConeT(nzero))
    if m - nzero:
        out.append(NonnegativeConeT(m - nzero))
    return out


def build_edges(seed=5101):
    """Rows of P, rows of A and columns of A with each of EDGE_LENGTHS entries (against eight lanes per row); a variable in
    no constraint and without any P entry; an empty row of A.
    Variables: six P hubs (a hub of length L: its diagonal and L - 1 links to leaves of its own), their leaves, six A column
    hubs, a pool of plain variables for the A row hubs, and one last variable that nothing touches."""
    rng = np.random.default_rng(seed)
    lens = [L for L in EDGE_LENGTHS if L > 0]
    nleaf = sum(L - 1 for L in lens)
    hubs = list(range(len(lens)))
    leaf0 = len(lens)
    colhub0 = leaf0 + nleaf
    pool0 = colhub0 + len(lens)
    npool = 70
    n = pool0 + npool + 1
    pr, pc = [], []
    leaf = leaf0
    for h, L in zip(hubs, lens):
        pr.append(h); pc.append(h)
        for _ in range(L - 1):
            pr.append(h); pc.append(leaf)
            leaf += 1
    P = sp.csc_matrix(sp.coo_matrix((_vals(rng, len(pr)), (pr, pc)), shape=(n, n)))
    ar, ac = [], []
    row = 0
    for L in EDGE_LENGTHS:                          # row hubs (L = 0: the empty row)
        cols = pool0 + rng.choice(npool, size=L, replace=False)
        ar += [row] * L
        ac += sorted(cols.tolist())
        row += 1
    for j, L in enumerate(lens):                    # column hubs: L rows of one entry each
        ar += list(range(row, row + L))
        ac += [colhub0 + j] * L
        row += L
    m = row
    A = sp.csc_matrix(sp.coo_matrix((_vals(rng, len(ar)), (ar, ac)), shape=(m, n)))
    pb = Problem("edges", P, A, _cones(m, 5), seed + 1)
    kP, kAcol, kz = pb.parts.kP, pb.parts.kAcol, pb.parts.kz
    userP = np.diff(sp.csr_matrix(pb.parts.P).indptr)
    assert set(EDGE_LENGTHS) <= set(userP.tolist()), "P row lengths"
    assert set(EDGE_LENGTHS) <= set(kz.tolist()) and set(EDGE_LENGTHS) <= set(kAcol.tolist()), "A row / column lengths"
    assert kAcol[-1] == 0 and userP[-1] == 0 and kP[-1] == 1
    return pb


def build_lp(seed=5102):
    """P = 0: every P prefix is the structural diagonal alone."""
    rng = np.random.default_rng(seed)
    n, m = 40, 30
    A = sp.random(m, n, density=0.2, random_state=np.random.RandomState(seed), format="csc", data_rvs=lambda k: _vals(rng, k))
    return Problem("lp", sp.csc_matrix((n, n)), A, _cones(m, 4), seed + 1)


def build_unconstrained(seed=5103):
    """m = 0 (the reference's unconstrained QP)."""
    rng = np.random.default_rng(seed)
    n = 50
    P = sp.diags([rng.uniform(1.0, 2.0, n), rng.uniform(-0.3, 0.3, n - 1)], [0, 1], format="csc")
    return Problem("unconstrained", P, sp.csc_matrix((0, n)), [], seed + 1)


def build_tiny(seed=5104):
    return Problem("n1m1", sp.csc_matrix(np.array([[1.25]])), sp.csc_matrix(np.array([[-0.75]])), _cones(1, 0), seed + 1)


def build_wrap(seed=5105):
    """n and m of 65 537 + 31 rows each: with one x-or-z row per owner lane the grid-stride loop takes a second (and, over
    n + m rows, a third and fifth) trip.  P tridiagonal, one or two entries per row of A."""
    rng = np.random.default_rng(seed)
    n = m = ROWS_PER_WG * GRID_CAP + 1 + 31
    P = sp.diags([rng.uniform(1.0, 2.0, n), rng.uniform(-0.3, 0.3, n - 1)], [0, 1], format="csc")
    two = rng.random(m) < 0.5
    r = np.concatenate([np.arange(m), np.flatnonzero(two)])
    c = np.concatenate([np.arange(m), (np.flatnonzero(two) + 17) % n])
    A = sp.csc_matrix(sp.coo_matrix((_vals(rng, r.size), (r, c)), shape=(m, n)))
    pb = Problem("wrap", P, A, _cones(m, 100), seed + 1)
    assert n + m > ROWS_PER_WG * GRID_CAP and set(pb.parts.kz.tolist()) == {1, 2}
    return pb


def build_dense_row(L, seed=5106):
    """One row of A with L entries (the walked prefix of its z row): n = L + 3, three short rows around it."""
    rng = np.random.default_rng(seed + L)
    n, m = L + 3, 4
    r = [0, 0, 1] + [2] * L + [3]
    c = [0, 5, 1] + list(range(L)) + [n - 1]
    A = sp.csc_matrix(sp.coo_matrix((_vals(rng, len(r)), (r, c)), shape=(m, n)))
    P = sp.diags(rng.uniform(1.0, 2.0, n), format="csc")
    pb = Problem(f"dense_row_{L}", P, A, _cones(m, 1), seed + L + 1)
    assert pb.parts.kz.max() == L and pb.parts.kx.max() <= 3
    return pb


def build_dense_col(L, seed=5107):
    """One x row whose walked prefix (its diagonal of P, then a column of A with L - 1 entries) has L entries."""
    rng = np.random.default_rng(seed + L)
    n, m = 5, L + 2
    r = list(range(L - 1)) + [L, L + 1, 0]
    c = [2] * (L - 1) + [0, 4, 3]
    A = sp.csc_matrix(sp.coo_matrix((_vals(rng, len(r)), (r, c)), shape=(m, n)))
    P = sp.diags(rng.uniform(1.0, 2.0, n), format="csc")
    pb = Problem(f"dense_col_{L}", P, A, _cones(m, 2), seed + L + 1)
    assert pb.parts.kx.max() == L and pb.parts.kx[2] == L and pb.parts.kz.max() <= 2
    return pb


BUILDERS = dict([("edges", build_edges), ("lp", build_lp), ("unconstrained", build_unconstrained), ("n1m1", build_tiny),
                 ("wrap", build_wrap)] +
                [(f"dense_row_{L}", (lambda L=L: build_dense_row(L))) for L in LONG_EDGES] +
                [(f"dense_col_{L}", (lambda L=L: build_dense_col(L))) for L in LONG_EDGES])

_CACHE = {}


def problem(name):
    """The builder's problem with its exact vectors and bounds, computed once and shared (never modified)."""
    if name not in _CACHE:
        pb = BUILDERS[name]()
        pb.exact = exact_vectors(pb.parts, **pb.data())
        pb.bounds = vector_bounds(pb.parts, **pb.data())
        _CACHE[name] = pb
    return _CACHE[name]


def equil_vectors(pb, seed=77):
    """random positive d, e with their reciprocals (as fp64 numbers: the kernel takes the four as given)"""
    rng = np.random.default_rng(seed)
    d, e = rng.uniform(0.25, 4.0, pb.n), rng.uniform(0.25, 4.0, pb.m)
    return d, 1.0 / d, e, 1.0 / e
