"""Extended-precision reference for the cone operations between the solves (TEST INFRASTRUCTURE): affine_ds, the
combined step's ds, step_length, margins and the shift to the cone interior, for zero, nonnegative, second-order and PSD
cones.

Written from the definitions, not from the kernels or from cuclarabel_amd/ipm.py:

    Jordan product    nonnegative  x o y = (x_i y_i);  second-order  x o y = (x'y, x0 y1 + y0 x1);
                      PSD  X o Y = (XY + YX)/2 on mat(.), svec of it with sqrt(2) on the off-diagonal entries
    unit e            nonnegative 1;  second-order (1, 0);  PSD svec(I)
    scaling           nonnegative  W = diag(w);  second-order  W = eta [w0 w1'; w1 I + w1 w1'/(1 + w0)], W^{-1} = (1/eta)
                      [w0 -w1'; -w1 I + w1 w1'/(1 + w0)];  PSD  W x = svec(R' mat(x) R), W^{-T} x = svec(Rinv mat(x) Rinv')
    affine ds         lambda o lambda  (PSD: lambda holds the k values of the diagonal matrix Lam)
    combined ds       lambda o lambda + m (W^{-T} ds) o (W dz) - sigma_mu e;  zero cone rows 0
    step length       the largest alpha <= alpha_max with z + alpha dz and s + alpha ds in the cone:
                      nonnegative  min over dz_i < 0 of -z_i/dz_i;
                      second-order  the reference's quadratic (x0 + a y0)^2 = ||x1 + a y1||^2 with a = y'Jy, b = 2 x'Jy,
                      c = max(0, x'Jx), every branch of _step_length_soc_component, and the scalar-part clamp;
                      PSD  1/(-gamma), gamma = lambda_min(Lam^{-1/2} mat(W dz) Lam^{-1/2}) where gamma < 0
                      alpha_max = min(1, -tau/dtau if dtau < 0, -kappa/dkappa if dkappa < 0)
    margins           nonnegative (min v, sum of positive v);  second-order a = v0 - ||v1||, (a, max(0, a));
                      PSD (lambda_min, sum of positive eigenvalues) of mat(v);  zero cone and empty cones (floatmax, 0)
    shift             v += a e per cone, in the three branches of _shift_to_cone_interior!; a primal zero cone's rows -> 0

The fp64 inputs -- the vectors AND the scaling (w, eta, lambda, R, Rinv) as the device holds it -- are taken as exact;
every quantity is computed with mpmath at 50 digits and rounded once to fp64.  (Nonnegative rows, of which the tests hold
half a million, go through numpy's 64-bit-mantissa long double instead: a handful of operations per row, 2^-11 u.)

Each value comes with an error bound: BOUND_C[family] * u * (size factor) * (magnitude from the reference):
    circ products, congruences   the product of the operand norms (||W^-1|| ||ds|| ||W|| ||dz||, ||R||^2 ||X|| ...)
    gamma                        k * || |Lam^-1/2| |G'| |X| |G| |Lam^-1/2| ||_2 (= ||M||_2 where nothing cancels in the
                                 congruence that forms M, and covering that cancellation where something does)
    1/(-gamma)                   the bound on gamma carried through the reciprocal
    second-order root            the bounds on a, b, c carried through d = b^2 - 4ac and the two root formulas; the condition
                                 term is 1/sqrt(d) (a double root is ill-conditioned) and 1/|a|, 1/c
A point within its own bound of a branch switch (d ~ 0, a ~ 0, c ~ 0, b ~ 0 with a > 0; gamma ~ 0) is `ambiguous`: both
answers are admissible and the reference then returns an interval that contains both.

The constants were fixed with tests/test_step_reference_host.py: the numpy fp64 classes of cuclarabel_amd/ipm.py, which
follow the reference solver operation by operation, evaluated at every shape the GPU test uses; each constant is chosen
so that their worst error / bound is at most 0.25 (measured worst ratios beside the constants).  The device gets a
factor 4 over that for its other summation order and Jacobi instead of LAPACK.
"""
import math

import numpy as np

from tests import cone_reference as cr

U = cr.U
MP = cr.MP
FMAX = float(np.finfo(float).max)
#                      constant     worst ratio of the fp64 numpy classes with it (test_step_reference_host.py)
BOUND_C = dict(nn=16.0,       # 0.22   nonnegative rows of affine / combined ds (half a million rows: the worst of six roundings)
               circ=4.0,      # 0.14   second-order rows of affine / combined ds
               cong=3.0,      # 0.14   PSD rows of affine / combined ds
               gamma=6.0,     # 0.13 / 0.17   smallest eigenvalue of the scaled step (step length) / of mat(v) (PSD margin)
               root=2.0,      # 0.12   second-order step length
               margin=8.0,    # 0.02 / 0.19   second-order margin / the shifted entries
               pos=1.0)       # 0.18   pos_margin


def _f(x):
    return float(x)


def _mpv(x):
    return [MP.mpf(float(v)) for v in x]


def _mpm(A):
    A = np.asarray(A, dtype=float)
    M = MP.matrix(A.shape[0], A.shape[1])
    for i in range(A.shape[0]):
        for j in range(A.shape[1]):
            M[i, j] = MP.mpf(float(A[i, j]))
    return M


def _smat_mp(x, k):
    return cr._smat_mp(x, k)


def _svec_mp(M, k):
    r2 = MP.sqrt(2)
    return [M[r, c] if r == c else (M[r, c] + M[c, r]) / r2 for r, c in cr.svec_pairs(k)]


_SHL = np.frompyfunc(lambda a, k: int(a) << int(k), 2, 1)


def _dyadic(A):
    """fp64 matrix -> (matrix of Python ints, e) with A = ints * 2^e exactly"""
    A = np.asarray(A, dtype=float)
    mant, ex = np.frexp(A)
    mi = np.rint(np.ldexp(mant, 53)).astype(np.int64)
    ex = ex.astype(np.int64) - 53
    nz = mi != 0
    emin = int(ex[nz].min()) if nz.any() else 0
    return _SHL(mi.astype(object), np.where(nz, ex - emin, 0).astype(object)), emin


def _congruence_mp(G, x, k):
    """G' mat(x) G as an mpmath matrix, the fp64 inputs exact: mat(x) = D + O / sqrt(2) with D the diagonal and O the
    off-diagonal svec entries as they stand, so that both congruences are integer matrix products (exact), combined and
    rounded to the working precision once per entry."""
    D, O = np.zeros((k, k)), np.zeros((k, k))
    for e, (r, c) in enumerate(cr.svec_pairs(k)):
        if r == c:
            D[r, r] = x[e]
        else:
            O[r, c] = O[c, r] = x[e]
    Gi, eg = _dyadic(G)
    out = MP.matrix(k, k)
    r2 = MP.sqrt(2)
    parts = []
    for X in (D, O):
        Xi, ex = _dyadic(X)
        parts.append((Gi.T.dot(Xi).dot(Gi), 2 * eg + ex))
    (Pd, ed), (Po, eo) = parts
    for i in range(k):
        for j in range(k):
            out[i, j] = MP.ldexp(MP.mpf(int(Pd[i, j])), ed) + MP.ldexp(MP.mpf(int(Po[i, j])), eo) / r2
    return out


class Scaling:
    """the device's NT scaling of a cone list: w (m), eta (per cone), lam (m), psd = [(R, Rinv, lam_k) per PSD cone]"""

    def __init__(self, cones, w, eta, lam, psd):
        self.cones, self.w, self.eta, self.lam, self.psd = list(cones), np.asarray(w), np.asarray(eta), np.asarray(lam), list(psd)

    def pieces(self):
        """(cone, index, slice, psd triple or None)"""
        off, ip = 0, 0
        for i, c in enumerate(self.cones):
            tri = None
            if c.kind == 3:
                tri = self.psd[ip]
                ip += 1
            yield c, i, slice(off, off + c.numel), tri
            off += c.numel


# ---------------------------------------------------------------------------------------------------------------------
#  affine ds / combined ds
# ---------------------------------------------------------------------------------------------------------------------
def nn_ds(lam, w, dz, ds, sigma_mu, m_corr, combined):
    L = np.longdouble
    lam, w = lam.astype(L), w.astype(L)
    val = lam * lam
    mag = np.abs(lam * lam)
    if combined:
        t = (ds.astype(L) / w) * (w * (L(m_corr) * dz.astype(L)))
        val = val + t - L(sigma_mu)
        mag = mag + np.abs(t) + abs(sigma_mu)
    return val.astype(float), BOUND_C["nn"] * U * mag.astype(float)


def soc_ds(lam, w, eta, dz, ds, sigma_mu, m_corr, combined):
    n = len(lam)
    lm, wm = _mpv(lam), _mpv(w)
    ll = MP.fsum(v * v for v in lm)
    out = [ll] + [2 * lm[0] * lm[i] for i in range(1, n)]
    mag = float(np.dot(lam, lam))
    if combined:
        e = MP.mpf(float(eta))
        zm = [MP.mpf(float(m_corr)) * v for v in _mpv(dz)]
        sm = _mpv(ds)
        w1z = MP.fsum(a * b for a, b in zip(wm[1:], zm[1:]))
        w1s = MP.fsum(a * b for a, b in zip(wm[1:], sm[1:]))
        Z = [e * (wm[0] * zm[0] + w1z)] + [e * (zm[i] + wm[i] * (zm[0] + w1z / (1 + wm[0]))) for i in range(1, n)]
        Y = [(wm[0] * sm[0] - w1s) / e] + [(sm[i] + wm[i] * (-sm[0] + w1s / (1 + wm[0]))) / e for i in range(1, n)]
        yz = MP.fsum(a * b for a, b in zip(Y, Z))
        out[0] += yz - MP.mpf(float(sigma_mu))
        for i in range(1, n):
            out[i] += Y[0] * Z[i] + Z[0] * Y[i]
        nW = float(w[0] + np.linalg.norm(w[1:]))                       # ||W||_2 = eta (w0 + ||w1||), ||W^-1||_2 = (w0 + ||w1||)/eta
        mag += abs(m_corr) * (nW * float(eta) * np.linalg.norm(dz)) * (nW / float(eta) * np.linalg.norm(ds)) + abs(sigma_mu)
    return np.array([_f(v) for v in out]), np.full(n, BOUND_C["circ"] * U * max(n, 2) * mag)


def psd_ds(lam_k, R, Rinv, dz, ds, sigma_mu, m_corr, combined, k):
    t = k * (k + 1) // 2
    if k == 0:
        return np.zeros(0), np.zeros(0)
    lm = _mpv(lam_k)
    M = MP.matrix(k, k)
    for i in range(k):
        M[i, i] = lm[i] * lm[i]
    mag = float(np.max(lam_k) ** 2)
    if combined:
        Z = _congruence_mp(R, dz, k) * MP.mpf(float(m_corr))
        Y = _congruence_mp(Rinv.T, ds, k)
        YZ = Y * Z                                       # (Y, Z symmetric: ZY = (YZ)')
        M = M + (YZ + YZ.T) / 2
        for i in range(k):
            M[i, i] -= MP.mpf(float(sigma_mu))
        n2 = lambda A: float(np.linalg.norm(A, 2))
        mag += abs(m_corr) * (n2(R) ** 2 * n2(cr.smat(dz, k))) * (n2(Rinv) ** 2 * n2(cr.smat(ds, k))) + abs(sigma_mu)
    return np.array([_f(v) for v in _svec_mp(M, k)]), np.full(t, BOUND_C["cong"] * U * k * mag)


def ds_ref(sc, dz, ds, sigma_mu, m_corr, combined):
    """(value (m), bound (m), family per row) of affine_ds (combined False) or of the combined step's ds"""
    m = sum(c.numel for c in sc.cones)
    val, bnd, fam = np.zeros(m), np.zeros(m), np.empty(m, dtype=object)
    for c, i, rng, tri in sc.pieces():
        if c.numel == 0:
            continue
        if c.kind == 0:
            fam[rng] = "zero"
        elif c.kind == 1:
            val[rng], bnd[rng] = nn_ds(sc.lam[rng], sc.w[rng], dz[rng], ds[rng], sigma_mu, m_corr, combined)
            fam[rng] = "nn_ds"
        elif c.kind == 2:
            val[rng], bnd[rng] = soc_ds(sc.lam[rng], sc.w[rng], sc.eta[i], dz[rng], ds[rng], sigma_mu, m_corr, combined)
            fam[rng] = "soc_ds"
        else:
            val[rng], bnd[rng] = psd_ds(tri[2], tri[0], tri[1], dz[rng], ds[rng], sigma_mu, m_corr, combined, c.dim)
            fam[rng] = "psd_ds"
    return val, bnd, fam


# ---------------------------------------------------------------------------------------------------------------------
#  step length.  A limit is an interval [lo, hi] around the once-rounded value: where nothing is ambiguous lo / hi are
#  value -+ bound; the minimum of limits each perturbed inside its interval lies in [min lo, min hi].
# ---------------------------------------------------------------------------------------------------------------------
class Limit:
    def __init__(self, value, bound=0.0, lo=None, hi=None, ambiguous=False, family="", where=""):
        self.value = float(value)
        self.lo = self.value - bound if lo is None else float(lo)
        self.hi = self.value + bound if hi is None else float(hi)
        self.hi = min(self.hi, FMAX)
        self.ambiguous, self.family, self.where = ambiguous, family, where

    def ratio(self, got):
        """|got - value| / bound on the side got lies on (0/0 = 0): <= 1 is admissible"""
        got = float(got)
        if got == self.value:
            return 0.0
        if not np.isfinite(got):
            return np.inf
        room = (self.hi - self.value) if got > self.value else (self.value - self.lo)
        return abs(got - self.value) / room if room > 0 else np.inf


def fold_min(limits):
    """the minimum of limits (pure minimum: order-free); the family / where of the one that binds"""
    best = min(limits, key=lambda l: l.value)
    return Limit(best.value, lo=min(l.lo for l in limits), hi=min(l.hi for l in limits),
                 ambiguous=any(l.ambiguous and l.lo <= best.hi for l in limits), family=best.family, where=best.where)


def nn_step(z, dz):
    m = dz < 0
    if not m.any():
        return Limit(FMAX, family="nn_step")
    q = -z[m] / dz[m]                                    # IEEE division: correctly rounded already
    v = float(q.min())
    return Limit(v, U * abs(v), family="nn_step")


def soc_step_component(x, y, branch_out=None):
    """_step_length_soc_component with alpha_max = floatmax -> Limit.  branch_out (a list) receives the branch's name."""
    n = len(x)
    xm, ym = _mpv(x), _mpv(y)
    limits = []
    if x[0] >= 0 and y[0] < 0:
        v = _f(-xm[0] / ym[0])
        limits.append(Limit(v, U * abs(v), family="soc_step"))
    y1 = MP.fsum(v * v for v in ym[1:])
    x1 = MP.fsum(v * v for v in xm[1:])
    xy = MP.fsum(a * b for a, b in zip(xm[1:], ym[1:]))
    a = ym[0] ** 2 - y1
    b = 2 * (xm[0] * ym[0] - xy)
    c = max(MP.mpf(0), xm[0] ** 2 - x1)
    d = b * b - 4 * a * c
    # absolute error bounds of the fp64 evaluations (sums of n products), the inputs being exact
    g = BOUND_C["root"] * max(n, 2) * MP.mpf(U)
    ea = g * (ym[0] ** 2 + y1)
    eb = g * 2 * (abs(xm[0] * ym[0]) + MP.sqrt(x1 * y1))
    ec = g * (xm[0] ** 2 + x1)
    ed = 2 * abs(b) * eb + 4 * (abs(a) * ec + abs(c) * ea) + g * (b * b + 4 * abs(a * c))
    name = None
    if (a > 0 and b > 0) or d < 0:
        name, root = ("a>0,b>0" if (a > 0 and b > 0) else "d<0"), None
    elif a == 0:
        name, root = "a==0", None
    elif c == 0:
        name, root = ("c==0,a>=0" if a >= 0 else "c==0,a<0"), (None if a >= 0 else MP.mpf(0))
    else:
        sd = MP.sqrt(d)
        t = (-b - sd) if b >= 0 else (-b + sd)
        r1, r2 = (2 * c) / t, t / (2 * a)
        cands = [r for r in (r1, r2) if r >= 0]
        root = min(cands) if cands else None
        name = "two positive roots" if len(cands) == 2 else ("one negative root" if len(cands) == 1 else "no positive root")
    if branch_out is not None:
        branch_out.append(name)
    # within its own bound of a branch switch?  (the exact-zero cases are exact in fp64 too: their data are dyadic)
    amb = (a != 0 and abs(a) <= ea) or (c != 0 and c <= ec) or (abs(d) <= ed and not (a > 0 and b > 0) and a != 0 and c != 0) \
        or (a > 0 and b != 0 and abs(b) <= eb)
    if root is None:
        lim = Limit(FMAX, family="soc_step")
    elif root == 0:
        lim = Limit(0.0, family="soc_step")
    else:
        # root r = 2c/t or t/(2a): relative error (ec/c + et/|t|) or (et/|t| + ea/|a|), et = eb + ed/(2 sqrt d) + u|t|
        sd = MP.sqrt(d)
        t = (-b - sd) if b >= 0 else (-b + sd)
        esd = min(ed / (2 * sd), MP.sqrt(ed)) if sd > 0 else MP.sqrt(ed)       # |sqrt(d + e) - sqrt(d)| <= sqrt|e|
        et = eb + esd + g * abs(t)
        rel = et / abs(t) + (ec / c if root == (2 * c) / t else ea / abs(a)) + g
        bound = _f(root * rel) if rel < 1 else FMAX
        lim = Limit(_f(root), bound, family="soc_step")
    if amb:
        # both sides of the switch are admissible: anything from 0 (c ~ 0) or the root up to "no limit"
        lim = Limit(lim.value, lo=0.0 if (c != 0 and c <= ec) else lim.lo, hi=FMAX, ambiguous=True, family="soc_step")
    limits.append(lim)
    return fold_min(limits)


def psd_gamma(lam_k, G, x, k):
    """gamma = lambda_min(Lam^{-1/2} G' mat(x) G Lam^{-1/2}) and its bound; G = R (W x) or Rinv' (W^{-T} x)"""
    M = _congruence_mp(G, x, k)
    isq = [1 / MP.sqrt(MP.mpf(float(v))) for v in lam_k]
    for i in range(k):
        for j in range(k):
            M[i, j] = M[i, j] * isq[i] * isq[j]
    E = MP.eigsy((M + M.T) / 2, eigvals_only=True)
    gamma = min(E[i] for i in range(k))
    li = 1.0 / np.sqrt(lam_k)
    absM = (li[:, None] * (np.abs(G).T @ np.abs(cr.smat(x, k)) @ np.abs(G))) * li[None, :]
    return gamma, BOUND_C["gamma"] * U * k * float(np.linalg.norm(absM, 2))


def psd_step_component(lam_k, G, x, k):
    if k == 0:
        return Limit(FMAX, family="psd_step")
    gamma, bg = psd_gamma(lam_k, G, x, k)
    g = _f(gamma)
    if g >= bg:
        return Limit(FMAX, family="psd_step")
    if g > -bg:                                          # gamma ~ 0: "no limit" and any large limit are admissible
        return Limit(FMAX if g >= 0 else 1.0 / -g, lo=1.0 / (bg - g), hi=FMAX, ambiguous=True, family="psd_step")
    v = _f(1 / -gamma)
    return Limit(v, lo=1.0 / (-g + bg), hi=1.0 / (-g - bg), family="psd_step")


def cone_step_limits(sc, dz, ds, z, s):
    """one Limit per cone (the minimum of its z and its s component), in cone order; zero and empty cones: no limit"""
    out = []
    for c, i, rng, tri in sc.pieces():
        if c.kind == 0 or c.numel == 0:
            lim = Limit(FMAX, family="none")
        elif c.kind == 1:
            lim = fold_min([nn_step(z[rng], dz[rng]), nn_step(s[rng], ds[rng])])
        elif c.kind == 2:
            lim = fold_min([soc_step_component(z[rng], dz[rng]), soc_step_component(s[rng], ds[rng])])
        else:
            R, Rinv, lam_k = tri
            lim = fold_min([psd_step_component(lam_k, R, dz[rng], c.dim), psd_step_component(lam_k, Rinv.T, ds[rng], c.dim)])
        lim.where = f"cone {i} (kind {c.kind}, {c.numel} rows)"
        out.append(lim)
    return out


def alpha_max(dtau, dkappa, tau, kappa):
    lims = [Limit(1.0, family="one")]
    if dtau < 0:
        v = -tau / dtau
        lims.append(Limit(v, U * abs(v), family="tau"))
    if dkappa < 0:
        v = -kappa / dkappa
        lims.append(Limit(v, U * abs(v), family="kappa"))
    return lims


def step_length_ref(sc, dz, ds, z, s, dtau, dkappa, tau, kappa):
    """variables_calc_step_length without max_step_fraction -> Limit (the minimum of the per-cone limits and alpha_max)"""
    return fold_min(alpha_max(dtau, dkappa, tau, kappa) + cone_step_limits(sc, dz, ds, z, s))


# ---------------------------------------------------------------------------------------------------------------------
#  margins and the shift to the interior
# ---------------------------------------------------------------------------------------------------------------------
def margins_ref(cones, v):
    """(min_margin Limit, pos_margin, bound on pos_margin)"""
    mins, pos, bpos, off, nterms = [Limit(FMAX, family="none")], MP.mpf(0), 0.0, 0, 0
    for i, c in enumerate(cones):
        x = v[off:off + c.numel]
        off += c.numel
        if c.kind == 0 or c.numel == 0:
            continue
        if c.kind == 1:
            mins.append(Limit(float(x.min()), family="nn_margin", where=f"cone {i}"))
            p = x[x > 0]
            pos += MP.mpf(math.fsum(p.tolist()))           # (exact sum, rounded once)
            bpos += float(p.sum())
            nterms += len(p)
        elif c.kind == 2:
            xm = _mpv(x)
            n1 = MP.sqrt(MP.fsum(t * t for t in xm[1:]))
            a = xm[0] - n1
            mins.append(Limit(_f(a), BOUND_C["margin"] * U * max(c.numel, 2) * _f(abs(xm[0]) + n1), family="soc_margin",
                              where=f"cone {i}"))
            pos += max(a, MP.mpf(0))
            bpos += max(c.numel, 2) * _f(abs(xm[0]) + n1)
            nterms += 1
        else:
            k = c.dim
            E = MP.eigsy(_smat_mp(x, k), eigvals_only=True)
            ev = [E[j] for j in range(k)]
            nrm = _f(max(abs(t) for t in ev))
            mins.append(Limit(_f(min(ev)), BOUND_C["gamma"] * U * k * nrm, family="psd_margin", where=f"cone {i}"))
            pos += MP.fsum(t for t in ev if t > 0)
            bpos += k * k * nrm
            nterms += k
    return fold_min(mins), _f(pos), BOUND_C["pos"] * U * (max(nterms, 1).bit_length() + 1) * bpos


def degree(cones):
    return sum(c.numel if c.kind == 1 else 1 if c.kind == 2 else c.dim if c.kind == 3 else 0 for c in cones)


def unit_rows(cones):
    """mask of the rows a unit shift touches, and mask of the zero cones' rows"""
    m = sum(c.numel for c in cones)
    hit, zero, off = np.zeros(m, dtype=bool), np.zeros(m, dtype=bool), 0
    for c in cones:
        if c.kind == 0:
            zero[off:off + c.numel] = True
        elif c.kind == 1:
            hit[off:off + c.numel] = True
        elif c.kind == 2:
            hit[off] = True
        elif c.numel:
            hit[off + np.array([j * (j + 1) // 2 + j for j in range(c.dim)], dtype=int)] = True
        off += c.numel
    return hit, zero


def shift_ref(cones, v, primal):
    """_shift_to_cone_interior! -> dict(min=Limit, pos, bpos, branch, value (m), bound (m)); branch is None when the
    margins sit within their bounds of a switch (the tests avoid that)"""
    lim, pos, bpos = margins_ref(cones, v)
    deg = degree(cones)
    target = max(1.0, 0.1 * pos / deg) if deg > 0 else 1.0
    btarget = 0.1 * bpos / deg + U * target if (deg > 0 and target > 1.0) else 0.0
    mn = lim.value
    bmn = max(lim.hi - mn, mn - lim.lo)
    if mn <= 0:
        branch, shifts = "outside", [(-mn, bmn), (target, btarget)]
    elif mn < target:
        branch, shifts = "small", [(target - mn, bmn + btarget + U * abs(target - mn))]
    else:
        branch, shifts = "good", [(0.0, 0.0)]
    if abs(mn) <= bmn or abs(mn - target) <= bmn + btarget:
        branch = None
    hit, zero = unit_rows(cones)
    L = np.longdouble                                    # (one addition per shift and row: the long double sum, rounded)
    out, bnd = np.array(v, dtype=float), np.zeros(len(v))
    for a, ba in shifts:                                 # one rounding per shift, applied in order
        out[hit] = (out[hit].astype(L) + L(a)).astype(float)
        bnd[hit] += ba + BOUND_C["margin"] * U * (np.abs(out[hit]) + 2 * abs(a))
    if primal:
        out[zero] = 0.0
    return dict(min=lim, pos=pos, bpos=bpos, branch=branch, value=out, bound=bnd)


# ---------------------------------------------------------------------------------------------------------------------
#  seeded steps
# ---------------------------------------------------------------------------------------------------------------------
def soc_exact_cases():
    """(name, x, y, limit with alpha_max = 1) for every branch of _step_length_soc_component, on dyadic / Pythagorean
    data so that fp64 and extended precision take the same branch.

    `d<0` is the exception.  For a > 0 and c > 0 both x and y are timelike, and then (x'Jy)^2 >= (x'Jx)(y'Jy) (the
    reversed Cauchy-Schwarz inequality): d >= 0 in exact arithmetic, with equality for parallel vectors.  The branch
    exists for rounding alone, so its case is a step from x = (4, 2, 3) straight through the apex (y = -2x, exact double
    root 1/2, d = 0), where the fp64 evaluation with ||x1|| = fl(sqrt(13)) gives d = -1.4e-13.  Both branches give 1/2
    there: d < 0 returns the scalar-part clamp -x0/y0 = 1/2, the root branch min(clamp, root)."""
    return [
        ("a>0,b>0", [2.0, 1.0, 0.0], [2.0, 0.0, 1.0], 1.0),               # a = 3, b = 8
        ("d<0", [4.0, 2.0, 3.0], [-8.0, -4.0, -6.0], 0.5),
        ("a==0", [8.0, 1.0, 2.0], [5.0, 3.0, 4.0], 1.0),                  # y on the boundary: 25 = 9 + 16
        ("c==0,a>=0", [5.0, 3.0, 4.0], [-2.0, 0.0, 1.0], 1.0),            # x on the boundary; a = 3, b = -28: alpha_max
        ("c==0,a<0", [5.0, 3.0, 4.0], [0.0, 1.0, 0.0], 0.0),              # x on the boundary; a = -1
        ("clamp", [4.0, 1.0, 2.0], [-5.0, 3.0, 4.0], 0.8),                # a == 0 returns alpha_max, which the clamp made 4/5
        ("two positive roots", [3.0, 0.0, 0.0], [-5.0, 4.0, 0.0], 1.0 / 3.0),   # d = 576: roots 1/3 and 3
        ("one negative root", [2.0, 0.0, 0.0], [0.0, 4.0, 0.0], 0.5),     # a = -16, b = 0, d = 256: roots -1/2, 1/2
    ]


# the shapes both test modules run (the GPU test's edge sizes; the host test fixes the constants on the same ones)
NN_SIZES = (1, 255, 256, 257, 2048 * 256 + 1)
SOC_DIMS = (2, 3, 4, 5, 6, 63, 64, 65, 128, 129)
PSD_SIDES = (1, 2, 3, 7, 8, 16, 17, 32, 33, 47, 48)


class Case:
    """A cone list with a seeded interior point (s, z) and a step (dz, ds).  pieces:
         ('nn', n) | ('zero', n) | ('soc', n, delta | None) | ('psd', k, class, leave)
       leave False: the PSD step is positive definite (gamma > 0, no limit); True: symmetric indefinite (gamma < 0).
       Zero cones carry nonzero garbage in every vector."""

    def __init__(self, pieces, seed=1, step_scale=1.0):
        from cuclarabel_amd.cones import ZeroConeT, NonnegativeConeT, SecondOrderConeT, PSDTriangleConeT
        rng = np.random.default_rng(seed)
        self.cones, ss, zz, dzs, dss = [], [], [], [], []
        for p in pieces:
            if p[0] == "nn":
                n = p[1]
                self.cones.append(NonnegativeConeT(n))
                s, z = cr.nn_point(rng, n), cr.nn_point(rng, n)
                dz, ds = step_scale * rng.standard_normal(n) * z, step_scale * rng.standard_normal(n) * s
            elif p[0] == "zero":
                n = p[1]
                self.cones.append(ZeroConeT(n))
                s, z, dz, ds = (rng.standard_normal(n) + 3.0 for _ in range(4))
            elif p[0] == "soc":
                n = p[1]
                self.cones.append(SecondOrderConeT(n))
                s, z = cr.soc_pair(rng, n, p[2] if len(p) > 2 else None)
                dz, ds = (step_scale * rng.standard_normal(n) * v[0] for v in (z, s))
            else:
                k, cls, leave = p[1], p[2], p[3]
                self.cones.append(PSDTriangleConeT(k))
                s, z = cr.psd_pair(rng, k, cls) if k else (np.zeros(0), np.zeros(0))
                steps = []
                for v in (z, s):
                    G = rng.standard_normal((k, k))
                    D = G @ G.T / max(k, 1) + np.eye(k) if not leave else (G + G.T) / 2
                    scale = np.abs(v).max() if k else 1.0
                    steps.append(cr.svec(step_scale * scale * D) if k else np.zeros(0))
                dz, ds = steps
            ss.append(s); zz.append(z); dzs.append(dz); dss.append(ds)
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)
        self.s, self.z, self.dz, self.ds = cat(ss), cat(zz), cat(dzs), cat(dss)
        self.m = len(self.s)
