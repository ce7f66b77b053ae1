"""Host model of the KKT value path: the two copies of K's values and the protocol that keeps them equal -- TEST
INFRASTRUCTURE ONLY.

The library holds K twice (csrc/hipkkt.hip): `Kval`, the triu CSC values that get factorised, and `fval`, the same values
in the order of the full symmetric CSR image, streamed by the refinement residual, k_P_spmv* and k_iterate_residuals.
`fval` is kept current by hand: P and A updates scatter into Kval and set `fval_dirty`; the next user of the image
(kkt_spmv) gathers the copy whole and clears the flag; a cone update writes every value THROUGH to its one or two slots of
the copy (kpos) when the copy is current, and leaves it alone when it is dirty.  The invariant: after any call, the image
read by kkt_spmv equals the image of Kval.

KModel restates that protocol in numpy with every value the update kernels write (csrc/kernels.hip, "KKT value
updates"): copies, negations, single products and a maximum, each with one correct fp64 answer because kernels.hip is
built without contraction.  Nothing here has a tolerance.

A "device" below is either a HipKKTSolver or a KModel (possibly with a seeded fault), so that the GPU tests and the host
tests of the test design share one code path: the sequences call the same methods on both, and assert_values /
assert_image / assert_eps compare the device with a fault-free model that received the same calls.
"""
import numpy as np
import scipy.sparse as sp

from tests import residual_reference as rr

REG_C0 = 1e-8                                   # static_regularization_constant, _proportional (eps^2) of the defaults
REG_C1 = 2.220446049250313e-16 ** 2
UPDATE_BLOCK = 256                              # k_update_values, k_scatter, k_gather_values: 256 threads, <= 4096 workgroups
UPDATE_GRID_CAP = 4096
RED_BLOCKS = 256                                # k_diag_absmax: <= 256 workgroups of 256
EXACT_PROBE_MAX_N = 4096                        # above: the two-column bounded probe

FAULTS = ("second_slot", "through_while_dirty", "P_not_dirty", "cone_lookup", "D_signs", "tail_skipped", "last_partial")


class ValuePathError(AssertionError):
    """raised by the three helpers; .helper names which"""

    def __init__(self, helper, msg):
        super().__init__(f"{helper}: {msg}")
        self.helper = helper


def image_pattern(colptr, rowval):
    """(indptr, indices, vmap) of the full symmetric CSR image in residual_reference.sym_from_triu's order; vmap[q] = the
    triu CSC entry behind image position q."""
    colptr, rowval = np.asarray(colptr, np.int64), np.asarray(rowval, np.int64)
    N = colptr.size - 1
    col = np.repeat(np.arange(N, dtype=np.int64), np.diff(colptr))
    assert (rowval <= col).all(), "not upper triangular"
    src = np.arange(rowval.size, dtype=np.int64)
    off = rowval != col
    r = np.concatenate([rowval, col[off]])
    c = np.concatenate([col, rowval[off]])
    e = np.concatenate([src, src[off]])
    order = np.lexsort((c, r))
    r, c, e = r[order], c[order], e[order]
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=N), out=indptr[1:])
    return indptr, c, e


def kpos_of(vmap, nnzK):
    """Two slots per K entry, -1 = none: the first image position that names the entry, then the second -- what the loop
    `if (kp[2e] < 0) kp[2e] = q; else kp[2e+1] = q;` over q ascending leaves (hipkkt_kkt_create)."""
    kp = np.full(2 * nnzK, -1, dtype=np.int64)
    qs = np.argsort(vmap, kind="stable")                      # grouped by entry, q ascending inside a group
    es = vmap[qs]
    first = np.ones(es.size, bool)
    first[1:] = es[1:] != es[:-1]
    kp[2 * es[first]] = qs[first]
    kp[2 * es[~first] + 1] = qs[~first]
    return kp


def sparse_soc_dims(cones):
    from cuclarabel_amd.cones import SecondOrderConeT, SOC_NO_EXPANSION_MAX_SIZE
    return [c.dim for c in cones if isinstance(c, SecondOrderConeT) and c.dim > SOC_NO_EXPANSION_MAX_SIZE]


class KModel:
    """Kval, fval, dirty, kpos and the CSR image of one handle; the operations do what the library does.
    fault: None or one of FAULTS (a simulated defect of the library, for the host tests of the test design)."""

    def __init__(self, colptr, rowval, maps, cones, Pdata, Adata, c0=REG_C0, c1=REG_C1, reg_enable=True, fault=None):
        assert fault is None or fault in FAULTS, fault
        self.colptr, self.rowval = np.asarray(colptr, np.int64), np.asarray(rowval, np.int64)
        self.N, self.nnzK = self.colptr.size - 1, self.rowval.size
        self.maps = {k: np.asarray(v, np.int64) for k, v in maps.items()}
        self.indptr, self.indices, self.vmap = image_pattern(self.colptr, self.rowval)
        self.kpos = kpos_of(self.vmap, self.nnzK)
        self.soc_of_entry = np.repeat(np.arange(len(sparse_soc_dims(cones)), dtype=np.int64), sparse_soc_dims(cones))
        assert self.soc_of_entry.size == self.maps["soc_u"].size and 2 * len(sparse_soc_dims(cones)) == self.maps["soc_D"].size
        self.c0, self.c1, self.reg_enable, self.fault = float(c0), float(c1), bool(reg_enable), fault
        self.Kval = np.zeros(self.nnzK)
        self.Kval[self.maps["P"]] = np.asarray(Pdata, np.float64)
        self.Kval[self.maps["A"]] = np.asarray(Adata, np.float64)
        self.fval = np.full(self.vmap.size, np.nan)            # (never read before the first gather)
        self.dirty = True
        self.eps = 0.0

    # ---- counts of the cone update's one launch
    @property
    def nHs(self):
        return self.maps["Hsblocks"].size

    @property
    def sparse_len(self):
        return self.maps["soc_u"].size

    @property
    def nsparse(self):
        return self.maps["soc_D"].size // 2

    @property
    def total(self):
        return self.nHs + self.sparse_len + self.nsparse

    # ---- the library's operations
    def _put(self, entries, values, through):
        self.Kval[entries] = values
        if through:
            p0 = self.kpos[2 * entries]
            self.fval[p0[p0 >= 0]] = values[p0 >= 0]
            if self.fault != "second_slot":
                p1 = self.kpos[2 * entries + 1]
                self.fval[p1[p1 >= 0]] = values[p1 >= 0]

    def update_cones(self, Hs, u=(), v=(), eta2=()):
        """k_update_values (one launch, items nHs | sparse_len | nsparse), then the regulariser"""
        Hs, u, v, eta2 = (np.asarray(a, np.float64).ravel() for a in (Hs, u, v, eta2))
        assert Hs.size == self.nHs and u.size == v.size == self.sparse_len and eta2.size == self.nsparse
        through = not self.dirty
        if self.fault == "through_while_dirty" and self.dirty:
            through, self.dirty = True, False                  # writes into a stale copy, and the gather never comes
        lookup = self.soc_of_entry
        if self.fault == "cone_lookup" and lookup.size:
            lookup = np.concatenate([lookup[:1], lookup[:-1]])  # entry j reads the cone of entry j - 1
        e2 = eta2[lookup] if lookup.size else np.zeros(0)
        dneg, dpos = (1, 0) if self.fault == "D_signs" else (0, 1)
        m = self.maps
        item = np.concatenate([np.arange(self.nHs), self.nHs + np.arange(self.sparse_len), self.nHs + np.arange(self.sparse_len),
                               self.nHs + self.sparse_len + np.arange(self.nsparse),
                               self.nHs + self.sparse_len + np.arange(self.nsparse)])
        entries = np.concatenate([m["Hsblocks"], m["soc_u"], m["soc_v"], m["soc_D"][dneg::2], m["soc_D"][dpos::2]])
        values = np.concatenate([-Hs, u * (-e2), v * (-e2), -eta2, eta2])
        if self.fault == "tail_skipped":
            keep = item < self.total - self.total % UPDATE_BLOCK
            entries, values = entries[keep], values[keep]
        self._put(entries, values, through)
        self.eps = self._regularizer() if self.reg_enable else 0.0
        return True

    def _regularizer(self):
        """c0 + c1 max |K[diag]|: block maxima over a grid-stride walk, then their maximum; one product, one sum"""
        d = np.abs(self.Kval[self.maps["diag_full"]])
        g = min(max((self.N + UPDATE_BLOCK - 1) // UPDATE_BLOCK, 1), RED_BLOCKS)
        block = (np.arange(self.N) // UPDATE_BLOCK) % g
        if self.fault == "last_partial":
            d = d[block != g - 1]
        mx = float(d.max()) if d.size else 0.0
        return self.c0 + self.c1 * mx

    def update_P(self, vals):
        self.Kval[self.maps["P"]] = np.asarray(vals, np.float64)
        if self.fault != "P_not_dirty":
            self.dirty = True

    def update_A(self, vals):
        self.Kval[self.maps["A"]] = np.asarray(vals, np.float64)
        self.dirty = True

    def spmv_use(self):
        if self.dirty:
            self.fval = self.Kval[self.vmap]
            self.dirty = False

    def expected_image(self, Kval=None):
        """always the symmetric image of Kval"""
        return rr.sym_from_triu(self.colptr, self.rowval, self.Kval if Kval is None else Kval)

    def read_image(self):
        """what a residual would read now (CSR data in image order)"""
        self.spmv_use()
        return self.fval.copy()

    # ---- the same under HipKKTSolver's names, so that a model can stand in for a handle
    def kktsolver_update(self, Hs, u=None, v=None, eta2=None):
        return self.update_cones(Hs, () if u is None else u, () if v is None else v, () if eta2 is None else eta2)

    def kktsolver_update_P(self, P):
        self.update_P(P.data if sp.issparse(P) else P)

    def kktsolver_update_A(self, A):
        self.update_A(A.data if sp.issparse(A) else A)

    def solve_once(self):
        """a solve reads the image (its refinement residual) and nothing else of what is modelled here"""
        self.spmv_use()
        return True

    @property
    def diagonal_regularizer(self):
        return self.eps


def model_of_handle(ks, P, A):
    """The fault-free model of a HipKKTSolver just created from (P, A): the handle's own pattern, maps and settings."""
    K = ks.KKT()
    st = ks.settings
    return KModel(K.indptr, K.indices, ks.maps(), ks.cones, sp.triu(sp.csc_matrix(P), format="csc").data,
                  sp.csc_matrix(A).data, c0=st.static_regularization_constant, c1=st.static_regularization_proportional,
                  reg_enable=bool(st.static_regularization_enable))


def model_of_oracle(o, P, A, cones, fault=None, **kw):
    K = o.K()
    return KModel(K.indptr, K.indices, o.maps(), cones, sp.triu(sp.csc_matrix(P), format="csc").data,
                  sp.csc_matrix(A).data, fault=fault, **kw)


# ------------------------------------------------------------------------------------------------ the three helpers
def _solve(dev):
    if isinstance(dev, KModel):
        return dev.solve_once()
    rng = np.random.default_rng(77)
    dev.kktsolver_setrhs(rng.standard_normal(dev.n), rng.standard_normal(dev.m))
    return dev.kktsolver_solve(np.zeros(dev.n), np.zeros(dev.m))


def device_values(dev):
    return dev.Kval.copy() if isinstance(dev, KModel) else dev.KKT().data


def assert_values(dev, model, tag=""):
    """Kval byte for byte"""
    got, want = device_values(dev), model.Kval
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
        raise ValuePathError("assert_values", f"{tag}: {bad.size} of {want.size} K values differ, first at entry {bad[0]} "
                                              f"(row {model.rowval[bad[0]]}): {got[bad[0]]!r} != {want[bad[0]]!r}")


def assert_image(dev, model, tag="", Kval=None, seed=0):
    """The image the residual reads equals the image of the model's Kval (or of the given values).  A model and a small
    handle are read exactly; a large handle by two random columns against the exact residual and its order-free bound
    (every stale entry must then be off by a factor outside [0.5, 2]: see assert_changed)."""
    want = model.expected_image(Kval)
    if isinstance(dev, KModel):
        got = dev.read_image()
        bad = np.flatnonzero(~(got == want.data))
        if bad.size:
            raise ValuePathError("assert_image", f"{tag}: {bad.size} image entries differ, first at position {bad[0]}: "
                                                 f"{got[bad[0]]!r} != {want.data[bad[0]]!r}")
        return
    N = dev.N
    assert N == want.shape[0]
    if N <= EXACT_PROBE_MAX_N:
        dense = want.toarray()
        for j0 in range(0, N, 64):
            j1 = min(j0 + 64, N)
            X = np.zeros((N, j1 - j0), order="F")
            X[np.arange(j0, j1), np.arange(j1 - j0)] = 1.0
            e, _, _ = dev.residual(X, np.zeros_like(X), route=0)
            ok = e == -dense[:, j0:j1]                          # (==: the signs of zeros may differ)
            if not ok.all():
                i, j = np.argwhere(~ok)[0]
                raise ValuePathError("assert_image", f"{tag}: {int((~ok).sum())} entries of columns {j0}..{j1 - 1} differ, "
                                                     f"first K[{i}, {j0 + j}]: {-e[i, j]!r} != {dense[i, j0 + j]!r}")
        return
    x, b = rr.probe_vectors(N, 2, 5151 + seed)
    e, _, _ = dev.residual(x, b, route=0)
    ratio = rr.error_vs_exact(e, rr.residual_exact(want, x, b)) / rr.residual_bound(want, x, b)
    if not ratio.max() <= 1.0:
        i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise ValuePathError("assert_image", f"{tag}: residual of column {j} off its bound by {ratio.max():.3g} at row {i}")


def assert_eps(dev, model, tag=""):
    got, want = dev.diagonal_regularizer, model.eps
    if not got == want:
        raise ValuePathError("assert_eps", f"{tag}: regulariser {got!r} != {want!r}")


def assert_changed(old, new, tag=""):
    """The test's own inputs: every value a step writes differs from the one it replaces by a factor outside [0.5, 2]
    (a stale entry then misses any bound by orders of magnitude); zeros may stay zeros."""
    old, new = np.asarray(old, np.float64), np.asarray(new, np.float64)
    both0 = (old == 0) & (new == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(new / old)
    ok = both0 | ((old == 0) & (new != 0)) | (r < 0.5) | (r > 2.0)
    assert ok.all(), (tag, "a new value within a factor 2 of the old one", int((~ok).sum()))


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """(P, A, cones) with the values of every step of the sequences: hs(step) -> (Hs, u, v, eta2), P2, A2."""

    EXPONENTS = (0, 1, -1, 2, -2, 3, -3, 4)                  # step s scales its cone data by 8^EXPONENTS[s]

    def __init__(self, name, P, A, cones, seed):
        from cuclarabel_amd.cones import SOC_NO_EXPANSION_MAX_SIZE
        self.name, self.cones, self.seed = name, list(cones), seed
        self.P = sp.triu(sp.csc_matrix(P), format="csc")
        self.P.sort_indices()
        self.A = sp.csc_matrix(A)
        self.A.sort_indices()
        self.n, self.m = self.P.shape[0], self.A.shape[0]
        assert self.m == sum(c.numel for c in cones)
        rng = np.random.default_rng(seed)
        self._base = []                                       # per cone: what the steps rescale
        for c in self.cones:
            k = c.numel
            if c.kind == 0:
                self._base.append(("zero", k))
            elif c.kind == 1 or (c.kind == 2 and c.dim > SOC_NO_EXPANSION_MAX_SIZE):
                diag = rng.uniform(1.0, 1.35, k)
                if c.kind == 1:
                    self._base.append(("diag", diag))
                else:
                    sg = lambda: rng.choice([-1.0, 1.0], k)
                    self._base.append(("sparse", diag, sg() * rng.uniform(0.05, 0.1, k) / np.sqrt(k),
                                       sg() * rng.uniform(0.05, 0.1, k) / np.sqrt(k), rng.uniform(1.0, 1.35)))
            else:                                              # dense block: second-order cone of dim <= 4, PSD triangle
                G = rng.standard_normal((k, k))
                self._base.append(("dense", G @ G.T / k + np.eye(k)))
        self._P_d = rng.uniform(1.0, 1.18, self.n)
        self._A_f = rng.uniform(1.0, 1.4, self.A.nnz)

    def hs(self, step):
        """Cone data of step `step`: 8^e times a base, times factors in [1, 1.03] that differ from step to step -- so two
        steps' values differ by 8^k / 1.1 .. 8^k 1.1, k != 0, entry by entry.  Dense blocks are D (G G'/k + I) D, positive
        definite; the sparse cones' u, v are short enough that the expanded block keeps its pivot signs."""
        scale = 8.0 ** self.EXPONENTS[step]
        rng = np.random.default_rng([self.seed, 1000 + step])
        Hs, U_, V_, E2 = [], [], [], []
        for b in self._base:
            if b[0] == "zero":
                Hs.append(np.zeros(b[1]))
            elif b[0] == "diag":
                Hs.append(scale * b[1] * rng.uniform(1.0, 1.03, b[1].size))
            elif b[0] == "sparse":
                k = b[1].size
                Hs.append(scale * b[1] * rng.uniform(1.0, 1.03, k))
                U_.append(b[2] * rng.uniform(1.0, 1.03, k))
                V_.append(b[3] * rng.uniform(1.0, 1.03, k))
                E2.append(scale * b[4] * rng.uniform(1.0, 1.03))
            else:
                k = b[1].shape[0]
                d = rng.uniform(1.0, 1.015, k)
                M = scale * (d[:, None] * b[1] * d[None, :])
                Hs.append(M.T[np.tril_indices(k)])            # column t, rows 0..t: the packed upper triangle
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)
        return cat(Hs), cat(U_), cat(V_), np.array(E2)

    def P2(self):
        """c D P D, c = 8: positive definite like P"""
        col = np.repeat(np.arange(self.n), np.diff(self.P.indptr))
        return 8.0 * self.P.data * (self._P_d[self.P.indices] * self._P_d[col])

    def A2(self):
        return self.A.data * self._A_f / 8.0


def _one_or_two_per_row(m, n, rng, two_every=3):
    """A (m x n): one entry per row, a second one in every `two_every`-th row (None: in no row), every column used when
    m >= n"""
    rows = np.arange(m)
    cols = rows % n
    extra = rows[::two_every] if two_every else rows[:0]
    two_every = two_every or 1
    r = np.concatenate([rows, extra])
    c = np.concatenate([cols, (cols[extra] + 1 + extra // two_every) % n])
    keep = np.ones(r.size, bool)
    keep[m:] = c[m:] != cols[extra]
    r, c = r[keep], c[keep]
    v = rng.uniform(0.5, 1.5, r.size) * rng.choice([-1.0, 1.0], r.size)
    A = sp.csc_matrix(sp.coo_matrix((v, (r, c)), shape=(m, n)))
    A.sort_indices()
    assert A.nnz == r.size
    return A


def _tridiag_P(n, rng):
    P = sp.diags(rng.uniform(1.0, 2.0, n), format="csc")
    if n > 1:
        P = (P + sp.diags(rng.uniform(-0.2, 0.2, n - 1), 1, format="csc")).tocsc()
    return sp.triu(P, format="csc")


def case_segments():
    """All three segments of k_update_values inside one wave: nHs 2 + 3 + 10 + 5 + 7 + 6 = 33, sparse_len 12, nsparse 2"""
    from cuclarabel_amd.cones import ZeroConeT, NonnegativeConeT, SecondOrderConeT, PSDTriangleConeT
    cones = [ZeroConeT(2), NonnegativeConeT(3), SecondOrderConeT(4), SecondOrderConeT(5), SecondOrderConeT(7),
             PSDTriangleConeT(2)]
    rng = np.random.default_rng(8101)
    n, m = 6, sum(c.numel for c in cones)
    return Case("segments", _tridiag_P(n, rng), _one_or_two_per_row(m, n, rng, 2), cones, 8101)


def case_block_edge(nn, k):
    """NN(nn), SOC(k): nHs = nn + k, then k entries of u and v, then one D pair"""
    from cuclarabel_amd.cones import NonnegativeConeT, SecondOrderConeT
    cones = [NonnegativeConeT(nn), SecondOrderConeT(k)]
    rng = np.random.default_rng(8200 + 16 * nn + k)
    n = 8
    return Case(f"block_edge[{nn},{k}]", _tridiag_P(n, rng), _one_or_two_per_row(nn + k, n, rng), cones, 8200 + 16 * nn + k)


# nHs = nn + k on 255, 256, 257 (first three); the sparse / D boundary nn + 2 k moved by k (next two) and put on 255, 256,
# 257 (last three: total = 256, 257, 258, so one of them has no tail at all)
BLOCK_EDGES = ((245, 10), (246, 10), (247, 10), (246, 9), (246, 11), (235, 10), (236, 10), (237, 10))


def case_many_soc():
    """300 SOC(5): sparse_len 1500, nsparse 300; the D segment (items 3000..3299) spans a workgroup edge"""
    from cuclarabel_amd.cones import SecondOrderConeT
    cones = [SecondOrderConeT(5) for _ in range(300)]
    rng = np.random.default_rng(8301)
    n = 10
    return Case("many_soc", _tridiag_P(n, rng), _one_or_two_per_row(1500, n, rng), cones, 8301)


def case_psd_wrap():
    """Two PSD(48) and NN(8): nHs = 2 * 692 076 + 8 > 4096 * 256"""
    from cuclarabel_amd.cones import NonnegativeConeT, PSDTriangleConeT
    cones = [PSDTriangleConeT(48), PSDTriangleConeT(48), NonnegativeConeT(8)]
    rng = np.random.default_rng(8401)
    n, m = 16, 2 * 1176 + 8
    return Case("psd_wrap", sp.triu(sp.diags(rng.uniform(1.0, 2.0, n), format="csc"), format="csc"),
                _one_or_two_per_row(m, n, rng, None), cones, 8401)


def banded_big_data(n=209_716, bands=5, seed=8501):
    """(P, A): P diagonal, A (n x n) with columns i .. i + bands - 1 (wrapped) in row i: nnzA = bands n > 4096 * 256"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), bands)
    cols = (rows + np.tile(np.arange(bands), n)) % n
    vals = rng.uniform(0.5, 1.5, rows.size) * rng.choice([-1.0, 1.0], rows.size)
    A = sp.csc_matrix(sp.coo_matrix((vals, (rows, cols)), shape=(n, n)))
    A.sort_indices()
    P = sp.triu(sp.diags(rng.uniform(1.0, 2.0, n), format="csc"), format="csc")
    return P, A


def case_banded_big():
    from cuclarabel_amd.cones import NonnegativeConeT
    P, A = banded_big_data()
    return Case("banded_big", P, A, [NonnegativeConeT(A.shape[0])], 8501)


SMALL_CASES = {"segments": case_segments, "many_soc": case_many_soc,
               **{f"block_edge[{nn},{k}]": (lambda nn=nn, k=k: case_block_edge(nn, k)) for nn, k in BLOCK_EDGES}}


# ------------------------------------------------------------------------------------------------ sequences
def _check(dev, model, tag, eps=False, seed=0):
    assert_values(dev, model, tag)
    assert_image(dev, model, tag, seed=seed)
    if eps:
        assert_eps(dev, model, tag)


def _update(dev, model, case, step, tag):
    """the same cone update on both; the step's values are checked against the ones they replace"""
    Hs, u, v, e2 = case.hs(step)
    m = model.maps
    lookup = model.soc_of_entry
    new = np.concatenate([-Hs, u * -e2[lookup], v * -e2[lookup], -e2, e2])
    ent = np.concatenate([m["Hsblocks"], m["soc_u"], m["soc_v"], m["soc_D"][0::2], m["soc_D"][1::2]])
    assert_changed(model.Kval[ent], new, tag)
    ok = dev.kktsolver_update(Hs, u, v, e2)
    if not ok:
        raise ValuePathError("update", f"{tag}: the update reported a numeric failure")
    model.update_cones(Hs, u, v, e2)


def sequence_level_b(dev, model, case):
    """Sequences 1-6 on one handle, every step checked.  The step names appear in the errors:
    1 create; 2 write-through after a probe; 3 update, solve, update; 4 update_P (gather; cones still H3);
    5 update_A then a cone update while dirty; 6 write-through again."""
    _check(dev, model, "seq1 create")
    _update(dev, model, case, 0, "seq2 update(H1)")
    _check(dev, model, "seq2 update(H1) write-through", eps=True)
    _update(dev, model, case, 1, "seq3 update(H2)")
    if not _solve(dev):
        raise ValuePathError("solve", "seq3: the solve failed")
    model.spmv_use()
    _update(dev, model, case, 2, "seq3 update(H3)")
    _check(dev, model, "seq3 update(H2) solve update(H3)", eps=True, seed=1)
    P2 = case.P2()
    assert_changed(case.P.data, P2, "seq4 P2")
    dev.kktsolver_update_P(P2)
    model.update_P(P2)
    _check(dev, model, "seq4 update_P gather", seed=2)
    A2 = case.A2()
    assert_changed(case.A.data, A2, "seq5 A2")
    dev.kktsolver_update_A(A2)
    model.update_A(A2)
    _update(dev, model, case, 3, "seq5 update(H4)")
    _check(dev, model, "seq5 update_A update(H4) while dirty", eps=True, seed=3)
    _update(dev, model, case, 4, "seq6 update(H5)")
    _check(dev, model, "seq6 update(H5) write-through", eps=True, seed=4)


def sequence_fresh(dev, model, case):
    """Sequence 7: never probed before its first update: update(H1), solve, update(H2), probe"""
    _update(dev, model, case, 0, "seq7 update(H1)")
    if not _solve(dev):
        raise ValuePathError("solve", "seq7: the solve failed")
    model.spmv_use()
    _update(dev, model, case, 1, "seq7 update(H2)")
    _check(dev, model, "seq7 update(H1) solve update(H2)", eps=True, seed=5)


# ------------------------------------------------------------------------------------------------ regulariser placement
BIG = 2.0 ** 40        # with the default c1 = eps^2 the proportional part reaches the last bit of c0 = 1e-8 only above ~2e7


def placement_positions(model, big=False):
    """Diagonal positions (indices into diag_full) to carry the largest magnitude in turn: 0, 255, 256, N - 1, one past
    the reduction grid's first lap (big), a negative -Hs entry, and the +eta^2 entry of a sparse cone's extension."""
    N = model.N
    hs_diag = np.intersect1d(model.maps["Hsblocks"], model.maps["diag_full"])
    pos = {"0": 0, "N-1": N - 1, "-Hs": int(np.flatnonzero(model.maps["diag_full"] == hs_diag[hs_diag.size // 2])[0])}
    for p in (255, 256):
        if p < N:
            pos[str(p)] = p
    if big:
        assert N > RED_BLOCKS * UPDATE_BLOCK + 300
        pos["65536+300"] = RED_BLOCKS * UPDATE_BLOCK + 300
    if model.nsparse:
        pos["+eta2"] = int(np.flatnonzero(model.maps["diag_full"] == model.maps["soc_D"][1])[0])
    return pos


def placement_inputs(model, case, position, big_value=None):
    """(P values, Hs, u, v, eta2) that put |big_value| at diagonal `position` and positive values below 2 on every other
    diagonal entry; None where the position is not a diagonal this test owns (an A entry cannot be: K's diagonal is P,
    -Hs and the extensions' D)."""
    big_value = BIG if big_value is None else big_value
    m = model.maps
    entry = m["diag_full"][position]
    Pd = case.P.data.copy()
    Hs, u, v, e2 = case.hs(0)
    assert np.abs(Pd).max() < big_value / 4 and np.abs(Hs).max() < big_value / 4 and (e2.size == 0 or e2.max() < big_value / 4)
    for name, arr in (("P", Pd), ("Hsblocks", Hs)):
        hit = np.flatnonzero(m[name] == entry)
        if hit.size:
            arr[hit[0]] = big_value
            return Pd, Hs, u, v, e2
    hit = np.flatnonzero(m["soc_D"] == entry)
    if hit.size:
        e2[hit[0] // 2] = big_value
        mine = model.soc_of_entry == hit[0] // 2             # (u eta^2, v eta^2 stay of order 0.1: the pivots keep their signs)
        u[mine] /= big_value
        v[mine] /= big_value
        return Pd, Hs, u, v, e2
    return None


def run_placement(dev, model, case, name, position):
    """one placement on a device and its model: eps must be the model's, bit for bit, and must name the big entry"""
    inp = placement_inputs(model, case, position)
    if inp is None:
        raise ValuePathError("placement", f"{name}: diagonal position {position} belongs to no value the test owns")
    Pd, Hs, u, v, e2 = inp
    dev.kktsolver_update_P(Pd)
    model.update_P(Pd)
    if not dev.kktsolver_update(Hs, u, v, e2):
        raise ValuePathError("update", f"placement {name}: the update reported a numeric failure")
    model.update_cones(Hs, u, v, e2)
    d = np.abs(model.Kval[model.maps["diag_full"]])
    top = np.flatnonzero(d == d.max())                       # (an extension's -eta^2 and +eta^2 share the magnitude)
    assert position in top and d[position] == BIG and top.size <= 2, (name, position)
    second = float(np.delete(d, top).max())
    assert 0.0 < second < BIG / 4
    assert model.eps == model.c0 + model.c1 * BIG
    assert model.c1 == 0.0 or model.eps != model.c0 + model.c1 * second, "the second largest entry would give the same eps"
    assert_eps(dev, model, f"placement {name}")
    assert_values(dev, model, f"placement {name}")
