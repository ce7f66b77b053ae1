"""Independent checks for the generalized power cone, a numpy restatement of the expanded KKT matrix, and a CPU
backend built on it.

The extended-precision oracle differentiates the dual barrier AS WRITTEN (coneops_genpowcone.jl:240-246) with mpmath.
`mp_closed` restates update_dual_grad_H's closed forms in 60 digits; tests/test_genpow_host.py ties it to the
derivatives of the barrier, the device tests then measure against it."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import mpmath as mp

from cuclarabel_amd import ipm, problems
from cuclarabel_amd.cones import GenPowerConeT, SecondOrderConeT, ZeroConeT, NonnegativeConeT

mp.mp.dps = 60


# ------------------------------------------------------------------------------------------
#  mpmath oracle
# ------------------------------------------------------------------------------------------
def dual_barrier(spec):
    a = [mp.mpf(v) for v in spec.alpha]
    d1 = len(a)

    def f(*z):
        phi = mp.mpf(1)
        for i in range(d1):
            phi *= (z[i] / a[i]) ** (2 * a[i])
        out = -mp.log(phi - sum(w * w for w in z[d1:]))
        for i in range(d1):
            out -= (1 - a[i]) * mp.log(z[i])
        return out
    return f


def _mpv(z):
    return [mp.mpf(float(v)) for v in z]


def mp_grad(spec, z):
    """grad f*(z) by numerical differentiation in extended precision, one coordinate at a time"""
    f, z = dual_barrier(spec), _mpv(z)
    out = []
    for k in range(len(z)):
        out.append(mp.diff(lambda t: f(*[z[i] + (t if i == k else 0) for i in range(len(z))]), 0))
    return mp.matrix(out)


def mp_hess(spec, z):
    """the full Hessian of f* by numerical differentiation (small cones)"""
    f, z = dual_barrier(spec), _mpv(z)
    n = len(z)
    H = mp.zeros(n, n)
    for i in range(n):
        for j in range(i, n):
            def g(t, u):
                y = list(z)
                y[i] += t
                y[j] += u
                return f(*y)
            H[i, j] = H[j, i] = mp.diff(g, (0, 0), (1, 1)) if i != j else \
                mp.diff(lambda t: f(*[z[k] + (t if k == i else 0) for k in range(n)]), 0, 2)
    return H


def mp_directional(spec, z, v, w):
    """(grad f*(z) . v, v' H*(z) w) by differentiating t -> f*(z + t v) and (t, u) -> f*(z + t v + u w): the cost is a
    few evaluations of the barrier whatever the dimension, so cones of hundreds of rows can be checked"""
    f, z, v, w = dual_barrier(spec), _mpv(z), _mpv(v), _mpv(w)
    n = len(z)
    g = mp.diff(lambda t: f(*[z[i] + t * v[i] for i in range(n)]), 0)
    h = mp.diff(lambda t, u: f(*[z[i] + t * v[i] + u * w[i] for i in range(n)]), (0, 0), (1, 1))
    return g, h


def mp_closed(spec, z):
    """(grad, d, p, q, r) of update_dual_grad_H (coneops_genpowcone.jl:336-389) evaluated in 60 digits"""
    a, z = [mp.mpf(v) for v in spec.alpha], _mpv(z)
    d1 = len(a)
    phi = mp.mpf(1)
    for i in range(d1):
        phi *= (z[i] / a[i]) ** (2 * a[i])
    nw = sum(w * w for w in z[d1:])
    zeta = phi - nw
    tau = [2 * a[i] / z[i] for i in range(d1)]
    grad = [-tau[i] * phi / zeta - (1 - a[i]) / z[i] for i in range(d1)] + [2 * w / zeta for w in z[d1:]]
    p0 = mp.sqrt(phi * (phi + nw) / 2)
    p1 = -2 * phi / p0
    q0 = mp.sqrt(zeta * phi / 2)
    r1 = 2 * mp.sqrt(zeta / (phi + nw))
    d = [tau[i] * phi / (zeta * z[i]) + (1 - a[i]) / (z[i] * z[i]) for i in range(d1)] + [2 / zeta] * (len(z) - d1)
    p = [p0 * tau[i] / zeta for i in range(d1)] + [p1 * w / zeta for w in z[d1:]]
    q = [tau[i] * q0 / zeta for i in range(d1)]
    r = [r1 * w / zeta for w in z[d1:]]
    return tuple(mp.matrix(v) for v in (grad, d, p, q, r))


def mp_dense_H(d, p, q, r):
    n, d1 = len(d), len(q)
    H = mp.diag(list(d)) + p * p.T
    for i in range(d1):
        for j in range(d1):
            H[i, j] -= q[i] * q[j]
    for i in range(n - d1):
        for j in range(n - d1):
            H[d1 + i, d1 + j] -= r[i] * r[j]
    return H


def rel_err(a, M):
    """max |a - M| / max |M| of a float64 vector against an mpmath vector, the subtraction in extended precision"""
    a = np.asarray(a, float).ravel()
    num = max(abs(mp.mpf(float(a[i])) - M[i]) for i in range(len(a)))
    den = max(abs(M[i]) for i in range(len(a)))
    return float(num / den)


# ------------------------------------------------------------------------------------------
#  points
# ------------------------------------------------------------------------------------------
def random_spec(rng, d1, d2):
    a = rng.dirichlet(np.full(d1, 2.0)) if d1 > 1 else np.array([1.0])
    return GenPowerConeT(problems.normalised_alphas(a), d2)


def random_interior_pair(spec, rng, spread=0.5, frac=0.9):
    """(s, z): s strictly inside the primal cone, z strictly inside the dual one; ||w|| is a uniform fraction (up to
    frac) of the bound"""
    a = np.array(spec.alpha)
    d1, d2 = spec.dim1, spec.dim2
    su, zu = np.exp(spread * rng.normal(size=d1)), np.exp(spread * rng.normal(size=d1))
    sb = np.exp(np.sum(a * np.log(su)))
    zb = np.exp(np.sum(a * np.log(zu / a)))
    sw, zw = rng.normal(size=d2), rng.normal(size=d2)
    sw *= rng.uniform(0.0, frac) * sb / np.linalg.norm(sw)
    zw *= rng.uniform(0.0, frac) * zb / np.linalg.norm(zw)
    return np.concatenate([su, sw]), np.concatenate([zu, zw])


def central_pair(spec, rng):
    """z random interior, s = -mu grad f*(z)"""
    _, z = random_interior_pair(spec, rng)
    c = ipm._make_cones([spec])[0]
    g, _ = c.dual_grad_H(z)
    return -np.exp(rng.normal()) * g, z


SHAPES = ((1, 1), (2, 1), (1, 3), (3, 2), (2, 5), (7, 4))          # fully differentiated
BIG_SHAPES = ((63, 1), (1, 64), (65, 40), (120, 200))              # differentiated along directions


# ------------------------------------------------------------------------------------------
#  numpy restatement of the expanded KKT matrix (directldl_kkt_assembly.jl:52-160, directldl_datamaps.jl:81-167)
# ------------------------------------------------------------------------------------------
def expansion_width(c):
    if isinstance(c, SecondOrderConeT) and c.dim > 4:
        return 2
    return 3 if isinstance(c, GenPowerConeT) else 0


def expanded_structure(P, A, specs):
    """triu CSC pattern of K with its maps, for lists of zero, nonnegative, second-order, exponential, power and
    generalized power cones.
    Rows ascend within a column and the diagonal comes last; the expansion columns follow n + m in cone order,
    pcol += pdim(map)."""
    P = sp.triu(sp.csc_matrix(P), format="csc")
    P.sort_indices()
    A = sp.csc_matrix(A)
    A.sort_indices()
    m, n = A.shape
    p = sum(expansion_width(c) for c in specs)
    N = n + m + p
    cols = [[] for _ in range(N)]                                   # per column: [(row, tag)]
    for j in range(n):
        rows = P.indices[P.indptr[j]:P.indptr[j + 1]]
        for k, r in enumerate(rows):
            cols[j].append((int(r), ("P", P.indptr[j] + k)))
        if not (len(rows) and rows[-1] == j):
            cols[j].append((j, None))
    for j in range(n):
        for k in range(A.indptr[j], A.indptr[j + 1]):
            cols[n + A.indices[k]].append((j, ("A", k)))
    off, boff, pcol = 0, 0, n + m
    soff = sidx = goff = gq = gr = gidx = 0
    for c in specs:
        row0, ne = n + off, c.numel
        dense = (isinstance(c, SecondOrderConeT) and c.dim <= 4) or c.kind in (4, 5)      # packed-triu blocks
        if dense:
            k = 0
            for t in range(ne):
                for r in range(t + 1):
                    cols[row0 + t].append((row0 + r, ("Hsblocks", boff + k)))
                    k += 1
            boff += k
        else:
            for t in range(ne):
                cols[row0 + t].append((row0 + t, ("Hsblocks", boff + t)))
            boff += ne
        if isinstance(c, SecondOrderConeT) and c.dim > 4:
            for t in range(ne):
                cols[pcol].append((row0 + t, ("soc_v", soff + t)))
                cols[pcol + 1].append((row0 + t, ("soc_u", soff + t)))
            cols[pcol].append((pcol, ("soc_D", 2 * sidx)))
            cols[pcol + 1].append((pcol + 1, ("soc_D", 2 * sidx + 1)))
            soff, sidx, pcol = soff + ne, sidx + 1, pcol + 2
        elif isinstance(c, GenPowerConeT):
            for t in range(c.dim1):
                cols[pcol].append((row0 + t, ("genpow_q", gq + t)))
            for t in range(c.dim2):
                cols[pcol + 1].append((row0 + c.dim1 + t, ("genpow_r", gr + t)))
            for t in range(ne):
                cols[pcol + 2].append((row0 + t, ("genpow_p", goff + t)))
            for t in range(3):
                cols[pcol + t].append((pcol + t, ("genpow_D", 3 * gidx + t)))
            goff, gq, gr, gidx, pcol = goff + ne, gq + c.dim1, gr + c.dim2, gidx + 1, pcol + 3
        off += ne
    sizes = dict(P=P.nnz, A=A.nnz, Hsblocks=boff, soc_u=soff, soc_v=soff, soc_D=2 * sidx, genpow_p=goff, genpow_q=gq,
                 genpow_r=gr, genpow_D=3 * gidx)
    maps = {k: np.zeros(v, np.int64) for k, v in sizes.items()}
    indptr, indices = np.zeros(N + 1, np.int64), []
    for j in range(N):
        for row, tag in cols[j]:
            if tag is not None:
                maps[tag[0]][tag[1]] = len(indices)
            indices.append(row)
        indptr[j + 1] = len(indices)
    maps["diag_full"] = indptr[1:] - 1
    dsigns = np.ones(N, np.int64)
    dsigns[n:n + m] = -1
    pcol = n + m
    for c in specs:
        w = expansion_width(c)
        dsigns[pcol:pcol + w] = (-1, 1) if w == 2 else (-1, -1, 1)[:w]
        pcol += w
    maps["dsigns"] = dsigns
    return dict(n=n, m=m, p=p, N=N, indptr=indptr, indices=np.array(indices, np.int64), maps=maps, Pdata=P.data.copy(),
                Adata=A.data.copy())


def expanded_values(S, cones):
    """K.nzval for host cone objects after update_scaling (kktsolver_directldl.jl:211-241 with the GenPow map update)"""
    v = np.zeros(len(S["indices"]))
    M = S["maps"]
    v[M["P"]] = S["Pdata"]
    v[M["A"]] = S["Adata"]
    v[M["Hsblocks"]] = -np.concatenate([c.get_Hs() for c in cones]) if cones else []
    so = si = go = gq = gr = gi = 0
    for c in cones:
        if isinstance(c, ipm._SOC) and c.sparse:
            u, vv, _ = c.sparse_data()
            e2 = c.eta ** 2
            v[M["soc_u"][so:so + c.n]] = u * (-e2)
            v[M["soc_v"][so:so + c.n]] = vv * (-e2)
            v[M["soc_D"][2 * si:2 * si + 2]] = (-e2, e2)
            so, si = so + c.n, si + 1
        elif isinstance(c, ipm._GenPow):
            q, r, p, D = c.sparse_data()
            v[M["genpow_q"][gq:gq + c.d1]] = q
            v[M["genpow_r"][gr:gr + c.d2]] = r
            v[M["genpow_p"][go:go + c.n]] = p
            v[M["genpow_D"][3 * gi:3 * gi + 3]] = D
            go, gq, gr, gi = go + c.n, gq + c.d1, gr + c.d2, gi + 1
    return v


def expanded_matrix(S, values):
    U = sp.csc_matrix((values, S["indices"], S["indptr"]), shape=(S["N"], S["N"]))
    return (U + sp.triu(U, 1).T).tocsc()


def dense_Hs(c):
    """W'W of one host cone as a dense matrix, column by column through mul_Hs"""
    return np.column_stack([c.mul_Hs(e) for e in np.eye(c.n)])


def reduced_matrix(P, A, cones):
    """[[P, A'], [A, -Hs]] dense, Hs block diagonal over the cones"""
    P = sp.triu(sp.csc_matrix(P), format="csc")
    Pf = (P + sp.triu(P, 1).T).toarray()
    A = sp.csc_matrix(A).toarray()
    m, n = A.shape
    H = np.zeros((m, m))
    for c in cones:
        H[c.rng, c.rng] = dense_Hs(c)
    return np.block([[Pf, A.T], [A, -H]])


def scale_cones(specs, s, z, mu, strategy=ipm.DUAL):
    cones = ipm._make_cones(specs)
    for c in cones:
        args = (mu, strategy) if isinstance(c, ipm._NonSym) else ()
        assert c.update_scaling(s[c.rng].copy(), z[c.rng].copy(), *args)
    return cones


class ExpandedScipyBackend:
    """CPU backend for ipm.solve: the expanded K of the restatement, factorised by scipy's sparse LU.  The static
    regulariser of the reference (kktsolver_directldl.jl:259-279) keeps the zero-cone pivots away from zero; one
    round of refinement against the unregularised K removes its footprint."""

    def __init__(self, P, A, cone_specs):
        self.specs = list(cone_specs)
        self.S = expanded_structure(P, A, self.specs)
        self.cones = ipm._make_cones(self.specs)
        self.last_ir_iterations = 0

    def update_identity(self):
        raise AssertionError("a problem with a non-symmetric cone never asks for the identity scaling")

    def update(self, s, z, mu, strategy):
        for c in self.cones:
            args = (mu, strategy) if isinstance(c, ipm._NonSym) else ()
            if not c.update_scaling(s[c.rng].copy(), z[c.rng].copy(), *args):
                return False
        S = self.S
        self.K = expanded_matrix(S, expanded_values(S, self.cones))
        eps = 1e-8 + 4.8e-20 * np.abs(self.K.diagonal()).max()
        self.lu = spla.splu((self.K + sp.diags(eps * S["maps"]["dsigns"].astype(float))).tocsc())
        return True

    def kktsolver_setrhs(self, rx, rz):
        self.rhs = np.concatenate([rx, rz, np.zeros(self.S["p"])])

    def kktsolver_solve(self, x, z):
        sol = self.lu.solve(self.rhs)
        for _ in range(3):
            sol += self.lu.solve(self.rhs - self.K @ sol)
        n, m = self.S["n"], self.S["m"]
        if x is not None:
            x[:] = sol[:n]
        if z is not None:
            z[:] = sol[n:n + m]
        return bool(np.all(np.isfinite(sol)))


def mixed_problem(seed, specs):
    rng = np.random.default_rng(seed)
    m = sum(c.numel for c in specs)
    n = m // 2 + 2
    A = sp.random(m, n, density=0.4, random_state=int(rng.integers(1 << 30)), format="csc", data_rvs=rng.standard_normal)
    Pm = sp.random(n, n, density=0.3, random_state=int(rng.integers(1 << 30)), format="csc", data_rvs=rng.standard_normal)
    P = sp.triu(Pm @ Pm.T + sp.identity(n), format="csc")
    s, z = np.zeros(m), np.zeros(m)
    off = 0
    for c in specs:
        if isinstance(c, GenPowerConeT):
            s[off:off + c.numel], z[off:off + c.numel] = random_interior_pair(c, rng)
        elif isinstance(c, SecondOrderConeT):
            for v in (s, z):
                v[off + 1:off + c.numel] = rng.standard_normal(c.numel - 1)
                v[off] = np.linalg.norm(v[off + 1:off + c.numel]) + np.exp(rng.normal())
        else:
            s[off:off + c.numel], z[off:off + c.numel] = np.exp(rng.normal(size=(2, c.numel)))
        off += c.numel
    return P, A, s, z


MIXED = [SecondOrderConeT(6), GenPowerConeT([0.3, 0.7], 2), NonnegativeConeT(3), GenPowerConeT([1.0], 1),
         SecondOrderConeT(3), SecondOrderConeT(9), GenPowerConeT([0.2, 0.3, 0.5], 4), ZeroConeT(2)]


