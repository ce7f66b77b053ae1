"""Host reference for the refinement layer: exact residuals, a summation-order-free error bound, KKT problems with
prescribed row lengths, and the reference's refinement loop in numpy -- TEST INFRASTRUCTURE ONLY.

The residual kernels (csrc/kernels.hip: k_residual<G, NC>, k_residual_long_*, k_residual_rm<V>) compute
e = b - K_sym x with G lanes per row, chunk trees for long rows and 8-entry unrolls; which instance runs depends on the
row lengths of the full symmetric image of K and on the column count.  Everything here works on that image:

    sym_from_triu      the image, with the structural row lengths the library's own CSR has (explicit zeros kept);
    residual_exact     b - K x as an unevaluated sum hi + lo of two doubles, exact to ~2^-100 of the row's magnitude:
                       every product a x is split without error into two doubles (Dekker / Veltkamp), and math.fsum
                       returns the correctly rounded EXACT sum of doubles -- exact rational arithmetic in effect, at the
                       cost of a C loop, which the 1-2 M entries of the largest matrices need;
    residual_bound     gamma_{k+1} (|b_i| + sum_j |K_ij| |x_j|), k the row's entry count: the textbook bound of a length
                       k + 1 inner product in ANY summation order, with or without fma (Higham, Accuracy and Stability of
                       Numerical Algorithms, 2nd ed., (3.5)); it holds for every lane split, chunk tree and unroll.

The reference's own error: |lo's rounding| <= u |lo| <= u^2 |e_i| <= u^2 S_i against a bound of at least 2 u S_i / (1 - 2u), a
factor of 2 / u = 2^54 below it (tests/test_residual_reference_host.py checks the pair against mpmath at 60 digits).
"""
import math

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
LONG_ROW = 4096          # kLongRow, kLongChunk, kNormParts of csrc/kernels.hpp; the lane-width rule of hipkkt_kkt_create
LONG_CHUNK = 2048
NORM_PARTS = 2048
LANE_AVG = 24.0
RM_BLOCKS = 512          # kRmBlocks (k_residual_rm), 16 rows per workgroup
IR_BLOCKS = 304          # kIrBlocks (k_ir_round in partials mode), 256 threads x 4 entries per pass


# ------------------------------------------------------------------------------------------------ the symmetric image
def sym_from_triu(colptr, rowval, nzval):
    """Full symmetric K (CSR, columns ascending in every row, explicit zeros kept) from the triu CSC arrays of
    get_pattern / get_values."""
    colptr, rowval, nzval = np.asarray(colptr, np.int64), np.asarray(rowval, np.int64), np.asarray(nzval, np.float64)
    N = colptr.size - 1
    col = np.repeat(np.arange(N, dtype=np.int64), np.diff(colptr))
    assert (rowval <= col).all(), "not upper triangular"
    off = rowval != col
    r = np.concatenate([rowval, col[off]])
    c = np.concatenate([col, rowval[off]])
    v = np.concatenate([nzval, nzval[off]])
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=N), out=indptr[1:])
    K = sp.csr_matrix((v, c, indptr), shape=(N, N))
    K.has_sorted_indices = True
    return K


def sym_of(ks):
    """The image of a HipKKTSolver's current un-regularised K."""
    U_ = ks.KKT()
    return sym_from_triu(U_.indptr, U_.indices, U_.data)


def row_lengths(K):
    return np.diff(K.indptr)


def shape_facts(K):
    """What the residual dispatch reads off the image: N, nlong, chunks, lane width, workgroups of k_residual."""
    L = row_lengths(K)
    N = K.shape[0]
    lanes = 64 if K.indptr[-1] / max(N, 1) > LANE_AVG else 8
    rpb = 256 // lanes
    long_ = L[L > LONG_ROW]
    return dict(N=N, nlong=int(long_.size), nchunks=int(np.sum((long_ + LONG_CHUNK - 1) // LONG_CHUNK)), lanes=lanes,
                grid=min((N + rpb - 1) // rpb, NORM_PARTS), grid_uncapped=(N + rpb - 1) // rpb, lengths=L)


# ------------------------------------------------------------------------------------------------ exact residual, bound
_SPLIT = 134217729.0      # 2^27 + 1


def two_product(a, b):
    """a * b = p + q exactly (p = fl(a b)); no fma needed (Dekker 1971).  Valid away from over- and underflow."""
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    q = al * bl - (((p - ah * bh) - al * bh) - ah * bl)
    return p, q


def residual_exact(K, x, b):
    """(hi, lo): b - K x = hi + lo up to ~u^2 of each row's magnitude; hi is the exact residual rounded to fp64.
    x, b: (N,) or (N, k)."""
    x, b = np.asarray(x, np.float64), np.asarray(b, np.float64)
    if x.ndim == 2:
        cols = [residual_exact(K, x[:, j], b[:, j]) for j in range(x.shape[1])]
        return np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)
    N = K.shape[0]
    ptr = K.indptr
    p, q = two_product(K.data, x[K.indices])
    assert np.isfinite(p).all() and np.isfinite(q).all() and np.isfinite(b).all(), "residual_exact needs finite data"
    # (every product whose low part could underflow would be below 1e-290: not in these tests)
    assert not np.any((p != 0) & (np.abs(p) < 1e-280)), "products too small for an exact split"
    pl, ql, bl = (-p).tolist(), (-q).tolist(), b.tolist()
    hi, lo = np.empty(N), np.empty(N)
    fsum = math.fsum
    for i in range(N):
        a, z = ptr[i], ptr[i + 1]
        t = pl[a:z] + ql[a:z]
        t.append(bl[i])
        h = fsum(t)
        t.append(-h)
        hi[i], lo[i] = h, fsum(t)
    return hi, lo


def error_vs_exact(e, exact):
    """|e - (hi + lo)| per entry.  e - hi is exact whenever e is within a factor 2 of hi (Sterbenz), which is all that a
    comparison with a bound needs."""
    hi, lo = exact
    return np.abs((np.asarray(e, np.float64) - hi) - lo)


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def residual_bound(K, x, b):
    """Per row gamma_{k+1} (|b_i| + sum_j |K_ij| |x_j|), k = the row's structural entry count.  The magnitude sum is
    itself an fp64 inner product of non-negative terms (relative error <= gamma_k): it is rounded UP by that much."""
    x, b = np.asarray(x, np.float64), np.asarray(b, np.float64)
    Ka = sp.csr_matrix((np.abs(K.data), K.indices, K.indptr), shape=K.shape)
    S = np.abs(b) + Ka @ np.abs(x)
    g = gamma(row_lengths(K) + 1)
    if x.ndim == 2:
        g = g[:, None]
    return g * S / (1.0 - g)


# ------------------------------------------------------------------------------------------------ problems
def build_rows(n, zero_rows, nn_rows, seed, p_offdiag=False, free_tail=8):
    """(P, A, cones): P diagonal (or tridiagonal), A one row per entry of zero_rows + nn_rows with that many entries
    (values of magnitude in [0.5, 1.5], random signs), the first len(zero_rows) rows on a zero cone and the rest on a
    nonnegative cone.  The last free_tail variables appear in no constraint: their rows of K hold the diagonal alone."""
    from cuclarabel_amd.cones import NonnegativeConeT, ZeroConeT
    rng = np.random.default_rng(seed)
    counts = list(zero_rows) + list(nn_rows)
    avail = n - free_tail
    assert avail >= 1 and max(counts, default=0) <= avail
    rows, cols = [], []
    for r, c in enumerate(counts):
        if c == avail:
            cc = np.arange(avail)
        elif c <= 4:
            cc = (rng.integers(0, avail) + np.arange(c) * 7) % avail      # (cheap: the padding rows are many)
        else:
            cc = rng.choice(avail, size=c, replace=False)
        rows.append(np.full(c, r, dtype=np.int64))
        cols.append(np.sort(cc))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.uniform(0.5, 1.5, rows.size) * rng.choice([-1.0, 1.0], rows.size)
    A = sp.csc_matrix(sp.coo_matrix((vals, (rows, cols)), shape=(len(counts), n)))
    A.sort_indices()
    assert A.nnz == rows.size, "duplicate entries in a constraint row"
    P = sp.diags(rng.uniform(0.5, 1.5, n), format="csc")
    if p_offdiag:
        P = (P + sp.diags(rng.uniform(-0.2, 0.2, n - 1), 1, format="csc")).tocsc()
    cones = []
    if zero_rows:
        cones.append(ZeroConeT(len(zero_rows)))
    if nn_rows:
        cones.append(NonnegativeConeT(len(nn_rows)))
    return sp.triu(P, format="csc"), A, cones


def hs_values(cones, seed):
    """Hs blocks for kktsolver_update: 0 on a zero cone, w^2 in [0.5, 2] on a nonnegative cone."""
    from cuclarabel_amd.cones import NonnegativeConeT
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(0.5, 2.0, c.numel) if isinstance(c, NonnegativeConeT) else np.zeros(c.numel)
                           for c in cones] + [np.zeros(0)])


def interleave(special, filler, every):
    """special entries spread through a list of `filler` ones, `every` fillers apart: no two special rows adjacent."""
    out, f = [], list(filler)
    for s in special:
        out.extend(f[:every])
        del f[:every]
        out.append(s)
    return out + f


EDGE8_LENGTHS = (1, 2, 7, 8, 9, 63, 64, 65, 4095, 4096, 4097, 6144, 6145)


def spec_edges8():
    """Lane width 8: rows of EDGE8_LENGTHS entries in the image (a constraint row of c entries has c + 1 with its
    diagonal; length 1 is a variable no constraint touches), four of them long (4097 twice, 6144, 6145), padded with
    2-entry rows: N = 6200 + 70 = 6270."""
    n = 6200
    special = [c - 1 for c in EDGE8_LENGTHS if c >= 2]
    z = interleave(special[:6] + [4096], [1] * 30, 3)       # zero cone: short edges and one 4097
    nn = interleave(special[6:], [1] * 27, 3)               # nonnegative cone: 64 .. 6145
    return dict(name="edges8", n=n, zero_rows=z, nn_rows=nn, seed=4101,
                want=dict(lanes=8, nlong=4, lengths=EDGE8_LENGTHS, n_mod=(32, False), nonadjacent=True))


EDGE64_LENGTHS = (63, 64, 65, 127, 128, 129)


def spec_edges64():
    """Lane width 64, no long rows: eight constraint rows of each of EDGE64_LENGTHS over 131 variables; N = 179."""
    per = [c - 1 for c in EDGE64_LENGTHS]
    return dict(name="edges64", n=131, zero_rows=per * 3, nn_rows=per * 5, seed=4102, free_tail=2,
                want=dict(lanes=64, nlong=0, lengths=EDGE64_LENGTHS, n_mod=(4, False)))


def spec_long257():
    """Lane width 64 with 257 long rows: a dense 257 x 4200 block on a zero cone (rows of 4201 entries)."""
    return dict(name="long257", n=4200, zero_rows=[4200] * 257, nn_rows=[], seed=4103, free_tail=0,
                want=dict(lanes=64, nlong=257, lengths=(4201,), n_mod=(1, True)))


def spec_wrap70k():
    """Lane width 8 past the grid cap of k_residual (2048 workgroups x 32 rows), of k_residual_rm (512 x 16) and -- in
    partials mode -- with 2048 + 1 partials per column: tridiagonal P of 40 000, 30 001 two-entry rows."""
    return dict(name="wrap70k", n=40_000, zero_rows=[2] * 10_000, nn_rows=[2] * 20_001, seed=4104, p_offdiag=True,
                want=dict(lanes=8, nlong=0, lengths=(3,), n_mod=(32, False), min_N=NORM_PARTS * 32 + 1))


def spec_accept320k():
    """One short constraint per variable, 160 001 + 160 001 rows: past one pass of k_ir_round's accept copy."""
    n = 160_001
    return dict(name="accept320k", n=n, zero_rows=[], nn_rows=[1] * n, seed=4105, free_tail=0, identity_A=True,
                want=dict(lanes=8, nlong=0, lengths=(2,), n_mod=(1, True), min_N=IR_BLOCKS * 256 * 4 + 1))


def make_problem(spec):
    if spec.get("identity_A"):
        from cuclarabel_amd.cones import NonnegativeConeT
        rng = np.random.default_rng(spec["seed"])
        n = spec["n"]
        P = sp.triu(sp.diags(rng.uniform(0.5, 1.5, n), format="csc"), format="csc")
        A = sp.diags(rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n), format="csc")
        return P, A, [NonnegativeConeT(n)]
    return build_rows(spec["n"], spec["zero_rows"], spec["nn_rows"], spec["seed"], spec.get("p_offdiag", False),
                      spec.get("free_tail", 8))


def expected_image(P, A, hs):
    """The image the library must assemble for (P, A) with Hs on the constraint diagonal: [P A'; A -diag(hs)], every
    diagonal entry structurally present (directldl_kkt_assembly.jl:15-175).  For the host tests, which have no handle."""
    n, m = P.shape[0], A.shape[0]
    Pu = sp.triu(P, format="coo")
    Ac = A.tocoo()
    r = np.concatenate([Pu.row, Ac.col, n + np.arange(m)])
    c = np.concatenate([Pu.col, n + Ac.row, n + np.arange(m)])
    v = np.concatenate([Pu.data, Ac.data, -np.asarray(hs, np.float64)])
    order = np.lexsort((r, c))
    r, c, v = r[order], c[order], v[order]
    colptr = np.zeros(n + m + 1, dtype=np.int64)
    np.cumsum(np.bincount(c, minlength=n + m), out=colptr[1:])
    return sym_from_triu(colptr, r, v)


def check_shape(K, want):
    """The builder's preconditions, from the image itself.  A failure is an error of the test, never a skip."""
    f = shape_facts(K)
    L = set(f["lengths"].tolist())
    assert f["lanes"] == want["lanes"], (f["lanes"], want)
    assert f["nlong"] == want["nlong"], (f["nlong"], want)
    missing = [c for c in want["lengths"] if c not in L]
    assert not missing, ("row lengths missing from the image", missing)
    mod, divisible = want["n_mod"]
    assert (f["N"] % mod == 0) == divisible, (f["N"], want["n_mod"])
    assert f["N"] >= want.get("min_N", 0), (f["N"], want)
    if want.get("nonadjacent"):              # at least two long rows, no two of them neighbours
        idx = np.flatnonzero(f["lengths"] > LONG_ROW)
        assert idx.size >= 2 and np.diff(idx).min() > 1, idx
    return f


def probe_vectors(N, k, seed):
    """x, b (N, k), different in every column, magnitudes O(1)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, k)), rng.standard_normal((N, k))


# ------------------------------------------------------------------------------------------------ simulated faults
def _row_terms(K, x, i):
    a, z = K.indptr[i], K.indptr[i + 1]
    return K.data[a:z], K.indices[a:z]


def faulty_residual(K, x, b, i, fault, x_other=None):
    """Row i of b - K x (fp64, exact up to rounding) with one simulated kernel fault:
    drop_entry (one from the middle), drop_chunk (entries [LONG_CHUNK, 2 LONG_CHUNK), or the row's second half when it is
    shorter), drop_last, double_entry, wrong_column (x_other for one entry)."""
    v, j = _row_terms(K, x, i)
    w = np.ones(v.size)
    xx = x[j].copy()
    mid = v.size // 2
    if fault == "drop_entry":
        w[mid] = 0.0
    elif fault == "drop_chunk":
        if v.size > LONG_CHUNK:
            w[LONG_CHUNK:2 * LONG_CHUNK] = 0.0
        else:
            w[mid:] = 0.0
    elif fault == "drop_last":
        w[-1] = 0.0
    elif fault == "double_entry":
        w[mid] = 2.0
    elif fault == "wrong_column":
        xx[mid] = x_other[j[mid]]
    else:
        raise ValueError(fault)
    p, q = two_product(v * w, xx)            # (w is 0, 1 or 2: v w is exact)
    return math.fsum([b[i]] + (-p).tolist() + (-q).tolist())


FAULTS = ("drop_entry", "drop_chunk", "drop_last", "double_entry", "wrong_column")


# ------------------------------------------------------------------------------------------------ the refinement loop
class HostFactor:
    """Solves with the REGULARISED K on the host: K + eps diag(dsigns), sparse LU in fp64."""

    def __init__(self, K, dsigns, eps):
        import scipy.sparse.linalg as spla
        self.Kreg = (K + sp.diags(eps * np.asarray(dsigns, np.float64))).tocsc()
        self.lu = spla.splu(self.Kreg)

    def __call__(self, r):
        return self.lu.solve(np.asarray(r, np.float64))


def margin(a, b):
    """How clear of each other two positive numbers are: max(a / b, b / a); inf when one is 0."""
    if a == 0.0 or b == 0.0:
        return math.inf
    return max(a / b, b / a)


def refine_loop(K, solve, b, abstol, reltol, stop_ratio, max_iter):
    """_iterative_refinement (kktsolver_directldl.jl:389-449) for one column, with `solve` for the factor of the
    regularised K and fp64 residuals on the un-regularised K.  Returns dict(x, rounds, norms = [||e|| of the first solve,
    then of every candidate], stop = 'tol' | 'ratio' | 'cap', accepted_last: the last candidate became x, iterates = [x
    after the first solve, then x after every round], margin = the smallest distance of any comparison from its
    threshold, as a factor)."""
    b = np.asarray(b, np.float64)
    normb = np.abs(b).max() if b.size else 0.0
    x = solve(b)
    e = b - K @ x
    norme = np.abs(e).max()
    out = dict(norms=[float(norme)], iterates=[x.copy()], rounds=0, stop="cap", accepted_last=True, margin=math.inf,
               normb=float(normb), ok=bool(np.isfinite(norme)))
    if not out["ok"]:
        return dict(out, x=x, stop="bad")
    tol = abstol + reltol * normb
    for _ in range(max_iter):
        out["margin"] = min(out["margin"], margin(norme, tol) if tol > 0 else (math.inf if norme > 0 else 1.0))
        if norme <= tol:
            out["stop"] = "tol"
            break
        last = norme
        cand = x + solve(e)
        e2 = b - K @ cand
        n2 = np.abs(e2).max()
        out["rounds"] += 1
        out["norms"].append(float(n2))
        if not np.isfinite(n2):
            return dict(out, x=x, stop="bad", ok=False)
        ratio = last / n2 if n2 > 0 else math.inf
        out["margin"] = min(out["margin"], margin(ratio, stop_ratio), margin(ratio, 1.0))
        if ratio < stop_ratio:
            out["accepted_last"] = bool(ratio > 1.0)
            if ratio > 1.0:
                x, e, norme = cand, e2, n2
            out["iterates"].append(x.copy())
            out["stop"] = "ratio"
            break
        x, e, norme = cand, e2, n2
        out["iterates"].append(x.copy())
    else:
        # the cap: the loop ends without another look at the tolerance
        out["stop"] = "cap"
    out["x"] = x
    out["norme"] = float(norme)
    return out


# ------------------------------------------------------------------------------------------------ refinement cases
REG_EPS = 1e-4            # static_regularization_constant of the refinement tests (proportional part 0)
SCALES = (1.0, 1e-3, 0.0, 1e-9, 1e-6)        # column j of a case: 10^(-3c) x random; one zero column; 1e-9: first solve enough
SCALES_ACTIVE = (1.0, 1e-3)                  # every column needs a round (the row-major driver's buffer-swap branch):
                                             # the 1e-6 columns meet the tolerances below with their first solve


def refinement_columns(N, k, seed, scales=SCALES):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((N, k))
    for j in range(k):
        B[:, j] *= scales[j % len(scales)]
    return B


def refinement_case(name, k=5, scales=SCALES, abstol=None):
    """A builder's problem under strong static regularisation: dict(P, A, cones, hs, B (N, k), eps, abstol, settings for
    the library and for the oracle)."""
    spec = {"edges64": spec_edges64, "edges8": spec_edges8, "accept320k": spec_accept320k}[name]()
    P, A, cones = make_problem(spec)
    N = P.shape[0] + A.shape[0]
    abstol = REFINE_ABSTOL[name] if abstol is None else abstol
    return dict(name=name, spec=spec, P=P, A=A, cones=cones, hs=hs_values(cones, spec["seed"] + 1),
                B=refinement_columns(N, k, spec["seed"] + 10 + k, scales), eps=REG_EPS, abstol=abstol,
                settings=dict(static_regularization_constant=REG_EPS, static_regularization_proportional=0.0,
                              iterative_refinement_reltol=0.0, iterative_refinement_abstol=abstol,
                              iterative_refinement_max_iter=20),
                oracle_settings=dict(static_reg_constant=REG_EPS, static_reg_proportional=0.0, ir_reltol=0.0,
                                     ir_abstol=abstol, ir_max_iter=20))


# absolute tolerances: every comparison of every column of the cases is clear of them by 4 x or more (norm sequences in
# tests/test_gpu_refinement.py; each test re-asserts the margins from its own prediction)
REFINE_ABSTOL = {"edges64": 3e-9, "edges8": 5e-9, "accept320k": 1e-9}

# The many-column sweeps' `add` store (tests/test_gpu_multi_sweeps.py): three trees of tests/front_shapes.py and
# tests/pulled_leaf_shapes.py as P of a problem without constraints (every sign +1), under the same settings.  name ->
# (scale of the matrix, abstol).  The tolerance sits in the gap between the second residual of the 10^0 columns (two
# rounds) and the first residual of the 10^-6 columns (none); that gap is (eps / d) / 1e-6 wide for diagonal entries ~ d,
# less the spread of the random columns: 24 (wc_roots), 59 (counts_40_65) and, with panel_nc33's values as they are, 9 -- not
# enough for a 4 x margin on both sides, so that case's matrix is halved (19).  Predicted sequences (10^0 | 10^-3 | 10^-6):
#   wc_roots      6e-5 -> 2e-9 -> 9e-14 (2 rounds) | 1e-7 -> 4e-12 (1) | 9e-11 (0)
#   counts_40_65  2e-4 -> 1e-8 -> 1e-12 (2 rounds) | 2e-7 -> 2e-11 (1) | 2e-10 (0)
#   panel_nc33    1e-4 -> 3e-9 -> 3e-13 (2 rounds) | 1e-7 -> 1e-11 (1) | 2e-10 (0)
# tests/test_multi_sweeps_host.py re-checks the conditions (first residual >= 1e4 abstol, every decision clear by 4 x).
MULTI_REFINE = {"wc_roots": (1.0, 4.6e-10), "counts_40_65": (1.0, 1.3e-9), "panel_nc33": (0.5, 6.8e-10)}
MULTI_REFINE_COLUMNS = ((9, SCALES_ACTIVE, 59), (33, SCALES, 83))      # (k, column scales, seed)


def multi_refine_settings(abstol):
    return dict(static_regularization_constant=REG_EPS, static_regularization_proportional=0.0,
                iterative_refinement_reltol=0.0, iterative_refinement_abstol=abstol, iterative_refinement_max_iter=20)
