"""Extended-precision reference for the cone scalings (TEST INFRASTRUCTURE).

Written from the definitions (the docstring of tests/ref_kkt_numpy.py), not from the kernels or
the oracle.  The float64 inputs s, z are taken as exact and every quantity is computed with mpmath at 50 digits, then
rounded once to float64:

    nonnegative   w = sqrt(s/z), lambda = sqrt(s z), Hs = s/z
    second-order  eta = (res(s)/res(z))^(1/2), res(x) = sqrt(x'Jx);  w = (s/res(s) + J z/res(z)) / (2 gamma),
                  gamma = sqrt((1 + s'z/(res(s) res(z)))/2), so that w'Jw = 1;  W = eta [w0 w1'; w1 I + w1 w1'/(1+w0)],
                  lambda = W z;  Hs = eta^2 (2ww' - J), or for dim > 4 its sparse form eta^2 (D + uu' - vv')
    PSD           A = Z^{-1/2} (Z^{1/2} S Z^{1/2})^{1/2} Z^{-1/2}, the SPD matrix with A Z A = S, formed as A = R R' with
                  R = L1 V Lam^{-1/2} from the SVD L2'L1 = U Lam V' (L1, L2 the Cholesky factors of S, Z);
                  lambda = the singular values of L2'L1, descending;  Hs = A (x)_s A packed (upper triangle, by
                  columns, of the matrix of x -> svec(A smat(x) A));  mul_Hs(x) = svec(A smat(x) A)

Besides the values, each reference carries the error bounds the tests apply (`*_bounds`): stated formulas in the unit
roundoff u, the cone size and quantities of the reference, each times one fixed constant (BOUND_C).
"""
import numpy as np
import mpmath

U = 2.0 ** -53
DPS = 50
# the fixed constants of the bounds below (one per quantity family)
BOUND_C = dict(nn=2.0, soc=4.0, lam=4.0, A=2.0, Ainv=8.0, ident=8.0, Hs=8.0, mulHs=8.0)


MP = mpmath.MPContext()
MP.dps = DPS


def _f(x):
    return float(x)


def _tonp(Mm):
    return np.array([[float(Mm[i, j]) for j in range(Mm.cols)] for i in range(Mm.rows)])


# ---------------------------------------------------------------------------------------------------------------
#  svec / smat and the symmetric Kronecker product, from their definitions
# ---------------------------------------------------------------------------------------------------------------
def svec_pairs(k):
    """(row, col) of each svec slot: the upper triangle by columns."""
    return [(r, c) for c in range(k) for r in range(c + 1)]


def svec_basis(k):
    """Q (t x k^2): svec(X) = Q vec(X) for symmetric X (vec by columns); its rows are orthonormal."""
    t = k * (k + 1) // 2
    Q = np.zeros((t, k * k))
    for e, (r, c) in enumerate(svec_pairs(k)):
        if r == c:
            Q[e, r + c * k] = 1.0
        else:
            Q[e, r + c * k] = Q[e, c + r * k] = np.sqrt(0.5)
    return Q


def skron(X, Y, Q=None):
    """The t x t matrix of x -> svec((X smat(x) Y' + Y smat(x) X') / 2) = Q ((Y (x) X + X (x) Y) / 2) Q'."""
    k = X.shape[0]
    Q = svec_basis(k) if Q is None else Q
    return Q @ ((np.kron(Y, X) + np.kron(X, Y)) * 0.5) @ Q.T


def packed_triu(H):
    """packed upper triangle by columns: get_Hs()'s layout of one block."""
    t = H.shape[0]
    return np.concatenate([H[:c + 1, c] for c in range(t)])


def smat(x, k):
    out = np.zeros((k, k))
    for e, (r, c) in enumerate(svec_pairs(k)):
        out[r, c] = out[c, r] = x[e] if r == c else x[e] * np.sqrt(0.5)
    return out


def svec(X):
    k = X.shape[0]
    return np.array([X[r, c] if r == c else (X[r, c] + X[c, r]) * np.sqrt(0.5) for r, c in svec_pairs(k)])


# ---------------------------------------------------------------------------------------------------------------
#  nonnegative cone
# ---------------------------------------------------------------------------------------------------------------
def nn_ref(s, z):
    w = np.array([_f(MP.sqrt(MP.mpf(a) / MP.mpf(b))) for a, b in zip(s, z)])
    lam = np.array([_f(MP.sqrt(MP.mpf(a) * MP.mpf(b))) for a, b in zip(s, z)])
    Hs = np.array([_f(MP.mpf(a) / MP.mpf(b)) for a, b in zip(s, z)])
    return dict(w=w, lam=lam, Hs=Hs)


def nn_bounds(ref):
    c = BOUND_C["nn"] * U
    return dict(w=c * np.abs(ref["w"]), lam=c * np.abs(ref["lam"]), Hs=2 * c * np.abs(ref["Hs"]))


# ---------------------------------------------------------------------------------------------------------------
#  second-order cone
# ---------------------------------------------------------------------------------------------------------------
def soc_ref(s, z):
    n = len(s)
    sm = [MP.mpf(v) for v in s]
    zm = [MP.mpf(v) for v in z]
    s1 = MP.fsum(v * v for v in sm[1:])
    z1 = MP.fsum(v * v for v in zm[1:])
    sres2, zres2 = sm[0] ** 2 - s1, zm[0] ** 2 - z1
    if not (sm[0] > 0 and zm[0] > 0 and sres2 > 0 and zres2 > 0):
        return None
    sres, zres = MP.sqrt(sres2), MP.sqrt(zres2)
    eta = MP.sqrt(sres / zres)
    sb = [v / sres for v in sm]
    zb = [v / zres for v in zm]
    gamma = MP.sqrt((1 + MP.fsum(a * b for a, b in zip(sb, zb))) / 2)
    w = [(sb[0] + zb[0]) / (2 * gamma)] + [(a - b) / (2 * gamma) for a, b in zip(sb[1:], zb[1:])]
    # lambda = W z, W = eta [w0 w1'; w1 I + w1 w1'/(1 + w0)]
    w1z1 = MP.fsum(a * b for a, b in zip(w[1:], zm[1:]))
    lam = [eta * (w[0] * zm[0] + w1z1)] + \
          [eta * (zm[0] * w[i] + zm[i] + w[i] * w1z1 / (1 + w[0])) for i in range(1, n)]
    # sizes of the terms that make up w_i = (sb_i -+ zb_i) / (2 gamma) and lambda = W z (what their errors scale with)
    wt = [(abs(a) + abs(b)) / (2 * gamma) for a, b in zip(sb, zb)]
    wtz = MP.fsum(a * abs(b) for a, b in zip(wt[1:], zm[1:]))
    lamterms = [eta * (wt[0] * abs(zm[0]) + wtz)] + \
               [eta * (abs(zm[0]) * wt[i] + abs(zm[i]) + wt[i] * wtz / (1 + w[0])) for i in range(1, n)]
    out = dict(eta=_f(eta), w=np.array([_f(v) for v in w]), lam=np.array([_f(v) for v in lam]),
               wterms=np.array([_f(v) for v in wt]), lamterms=np.array([_f(v) for v in lamterms]),
               eta2=_f(eta * eta),
               delta_s=_f(sres2 / (2 * sm[0] ** 2)), delta_z=_f(zres2 / (2 * zm[0] ** 2)))
    wJw = w[0] ** 2 - MP.fsum(v * v for v in w[1:])
    out["wJw_minus_1"] = _f(wJw - 1)
    if n <= 4:
        H = np.zeros((n, n))
        for i in range(n):
            for j in range(n):
                J = (1 if i == 0 else -1) if i == j else 0
                H[i, j] = _f(eta * eta * (2 * w[i] * w[j] - J))
        out["H"] = H
        out["Hs"] = packed_triu(H)
    else:
        wsq = MP.fsum(v * v for v in w)
        d = 1 / (2 * wsq)
        u0 = MP.sqrt(wsq - d)
        u1 = 2 * w[0] / u0
        v1 = MP.sqrt(2 * (2 + 1 / wsq) / (2 * wsq - 1 / wsq))
        out["d"], out["u1"], out["v1"] = _f(d), _f(u1), _f(v1)
        out["u"] = np.array([_f(u0)] + [_f(u1 * v) for v in w[1:]])
        out["v"] = np.array([0.0] + [_f(v1 * v) for v in w[1:]])
        out["Hs"] = np.r_[_f(eta * eta * d), np.full(n - 1, _f(eta * eta))]
        # the identity that defines the sparse form, checked at working precision on a few entries
        for (i, j) in ((0, 0), (0, n - 1), (1, 1), (1, n - 1), (n - 1, n - 1)):
            D = (d if i == 0 else 1) if i == j else 0
            ui = u0 if i == 0 else u1 * w[i]
            uj = u0 if j == 0 else u1 * w[j]
            vi = 0 if i == 0 else v1 * w[i]
            vj = 0 if j == 0 else v1 * w[j]
            J = (1 if i == 0 else -1) if i == j else 0
            lhs = D + ui * uj - vi * vj
            rhs = 2 * w[i] * w[j] - J
            assert abs(lhs - rhs) <= MP.mpf(10) ** (-DPS + 8) * (1 + abs(rhs)), (i, j)
    return out


def soc_bounds(ref):
    """Relative error e of every SOC scalar: each goes through res(x) = (x0 - |x1|)(x0 + |x1|), where rounding in |x1|
    (a sum of n squares) is amplified by 1/delta, delta = res^2 / (2 x0^2) the relative gap to the boundary.  Vector
    entries are bounded componentwise by e times the size of their terms: w_i = (sb_i -+ zb_i) / (2 gamma) by
    (|sb_i| + |zb_i|) / (2 gamma), lambda = W z by the same sum taken over |W| |z|, u and v (multiples of w) likewise."""
    e = BOUND_C["soc"] * len(ref["w"]) * U * (1.0 + 1.0 / ref["delta_s"] + 1.0 / ref["delta_z"])
    wt = ref["wterms"]
    out = dict(eps=e, eta=e * ref["eta"], eta2=2 * e * ref["eta2"], w=e * wt, lam=e * ref["lamterms"])
    if "H" in ref:
        out["H"] = 2 * e * ref["eta2"] * (2 * np.outer(wt, wt) + 1)
        out["Hs"] = packed_triu(out["H"])
    else:
        out["u"] = 2 * e * np.r_[np.abs(ref["u"][0]), abs(ref["u1"]) * wt[1:]]
        out["v"] = 2 * e * np.r_[0.0, abs(ref["v1"]) * wt[1:]]
        out["Hs"] = 2 * e * np.abs(ref["Hs"])
    return out


# ---------------------------------------------------------------------------------------------------------------
#  PSD cone
# ---------------------------------------------------------------------------------------------------------------
def _smat_mp(x, k):
    Sm = MP.matrix(k, k)
    r2 = MP.sqrt(2)
    for e, (r, c) in enumerate(svec_pairs(k)):
        if r == c:
            Sm[r, c] = MP.mpf(x[e])
        else:
            Sm[r, c] = Sm[c, r] = MP.mpf(x[e]) / r2
    return Sm


def psd_ref(s, z, k):
    """None when S or Z is not positive definite."""
    Sm, Zm = _smat_mp(s, k), _smat_mp(z, k)
    try:
        L1, L2 = MP.cholesky(Sm), MP.cholesky(Zm)
    except ValueError:
        return None
    M = L2.T * L1
    # M'M = V Lam^2 V'  (at 50 digits the squared condition number costs nothing at these spectra)
    E, V = MP.eigsy(M.T * M)
    order = sorted(range(k), key=lambda i: -E[i])
    lam = [MP.sqrt(E[i]) for i in order]
    Vs = MP.matrix(k, k)
    for j, i in enumerate(order):
        for r in range(k):
            Vs[r, j] = V[r, i]
    Dm = MP.diag([1 / MP.sqrt(l) for l in lam])
    R = L1 * Vs * Dm
    Rinv = MP.diag([MP.sqrt(l) for l in lam]) * Vs.T * MP.inverse(L1)
    A = R * R.T
    Ainv = Rinv.T * Rinv
    out = dict(k=k, lam=np.array([_f(v) for v in lam]), R=_tonp(R), Rinv=_tonp(Rinv), A=_tonp(A), Ainv=_tonp(Ainv),
               S=_tonp(Sm), Z=_tonp(Zm))
    # A Z A = S, the definition, at working precision
    res = A * Zm * A - Sm
    assert max(abs(res[i, j]) for i in range(k) for j in range(k)) <= \
        MP.mpf(10) ** (-DPS + 12) * max(1, max(abs(Sm[i, j]) for i in range(k) for j in range(k)))
    return out


def psd_hs(ref):
    """packed Hs of the reference and the size of its terms |A_ik A_jl| + |A_il A_jk| (in svec scaling); kept with
    the reference (a second at side 48)"""
    if "_hs" not in ref:
        A = ref["A"]
        Q = svec_basis(ref["k"])
        ref["_hs"] = (packed_triu(skron(A, A, Q)), packed_triu(skron(np.abs(A), np.abs(A), Q)))
    return ref["_hs"]


def psd_bounds(ref):
    """the bounds of _psd_bounds, kept with the reference"""
    if "_bounds" not in ref:
        ref["_bounds"] = _psd_bounds(ref)
    return ref["_bounds"]


def _psd_bounds(ref):
    """First-order bounds.  A perturbation dS, dZ of the inputs moves A by R X R' with X_ij = (R^{-1} dS R^{-T} -
    R' dZ R)_ij / (lam_i + lam_j) (differentiate A Z A = S in the coordinates where R'ZR = R^{-1}SR^{-T} = Lam).  A
    backward-stable Cholesky / SVD perturbs S and Z componentwise by k u sqrt(S_ii S_jj), k u sqrt(Z_ii Z_jj)."""
    k, lam, R, Ri, A = ref["k"], ref["lam"], ref["R"], ref["Rinv"], ref["A"]
    S, Z = ref["S"], ref["Z"]
    ES = np.sqrt(np.outer(np.diag(S), np.diag(S)))
    EZ = np.sqrt(np.outer(np.diag(Z), np.diag(Z)))
    X = (np.abs(Ri) @ ES @ np.abs(Ri).T + np.abs(R).T @ EZ @ np.abs(R)) / (lam[:, None] + lam[None, :])
    ku = k * U
    bA = BOUND_C["A"] * ku * (np.abs(R) @ X @ np.abs(R).T + np.abs(R) @ np.abs(R).T)
    bAinv = BOUND_C["Ainv"] * ku * (np.abs(Ri).T @ X @ np.abs(Ri) + np.abs(Ri).T @ np.abs(Ri))
    Q = svec_basis(k)
    absA = np.abs(A)
    TZ, TS = np.abs(R).T @ np.abs(Z) @ np.abs(R), np.abs(Ri) @ np.abs(S) @ np.abs(Ri).T
    bHs = packed_triu(2 * skron(bA, absA, Q) + skron(bA, bA, Q)) + BOUND_C["Hs"] * U * packed_triu(skron(absA, absA, Q))
    return dict(
        # d lam_i = (R^{-1} dS R^{-T} + R' dZ R)_ii / 2 = lam_i X_ii at first order
        lam=BOUND_C["lam"] * ku * lam * (np.diag(X) + 1.0),
        A=bA, Ainv=bAinv, Hs=bHs,
        # R Rinv = I and R'ZR = Lam = Rinv S Rinv': rounding in the products plus the Jacobi stopping rule
        RRinv=BOUND_C["ident"] * ku * (np.abs(R) @ X @ np.abs(Ri) + np.abs(R) @ np.abs(Ri)),
        RZR=BOUND_C["ident"] * ku * (TZ + TZ @ X + X @ TZ + np.sqrt(np.outer(lam, lam))),
        RiSRi=BOUND_C["ident"] * ku * (TS + TS @ X + X @ TS + np.sqrt(np.outer(lam, lam))))


def psd_mul_Hs(ref, x):
    """svec(A smat(x) A) and the bound on a computed one: terms |A| |X| |A| plus the error of A itself."""
    k, A = ref["k"], ref["A"]
    X = smat(x, k)
    y = svec(A @ X @ A)
    b = psd_bounds(ref)["A"]
    absA, absX = np.abs(A), np.abs(X)
    terms = svec(absA @ absX @ absA)
    return y, BOUND_C["mulHs"] * k * U * terms + svec(b @ absX @ absA + absA @ absX @ b)


def ratio(err, bound):
    """the worst of |err| / bound (0 / 0 = 0); a NaN or infinite error or bound anywhere gives inf"""
    err, bound = np.abs(np.asarray(err, dtype=float)), np.asarray(bound, dtype=float)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(err) & np.isfinite(bound), r, np.inf)
    r[~np.isfinite(r)] = np.inf
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------
#  seeded points
# ---------------------------------------------------------------------------------------------------------------
def nn_point(rng, n):
    return np.exp(rng.uniform(-3, 3, n))


def soc_point(rng, n, delta=None):
    """x0 - |x1| = delta x0 (relative gap to the boundary); delta None: well inside (0.2 .. 0.8)."""
    if delta is None:
        delta = rng.uniform(0.2, 0.8)
    d = rng.standard_normal(n - 1)
    d /= np.linalg.norm(d)
    x0 = np.exp(rng.uniform(-1, 1))
    return np.r_[x0, x0 * (1.0 - delta) * d]


def soc_pair(rng, n, delta=None, which="both"):
    """which in ('s', 'z', 'both'): the side(s) at relative gap delta; the other well inside."""
    s = soc_point(rng, n, delta if which in ("s", "both") else None)
    z = soc_point(rng, n, delta if which in ("z", "both") else None)
    return s, z


def _orth(rng, k):
    Q, Rr = np.linalg.qr(rng.standard_normal((k, k)))
    return Q * np.sign(np.diag(Rr))


PSD_CLASSES = ("interior", "cond", "identity", "scaled", "cluster", "diagonal", "late")


def psd_pair(rng, k, cls="interior"):
    """(S, Z) as svec vectors.
    interior  S = G G'/k + I, Z likewise
    cond      S = D C1 D, Z = E C2 E, D = diag(logspace(0, -3)), E = D permuted, C1, C2 well conditioned: cond(S), cond(Z) ~ 1e6,
              lambda over ~6 decades (graded, as interior-point iterates are)
    identity  S = Z = I (every singular value tied: no rotation, rank tiebreak)
    scaled    S = 4 Z (A = 2 I exactly)
    cluster   S = R Lam R', Z = R^{-T} Lam R^{-1} with Lam in three clusters of equal values
    diagonal  diagonal S, Z whose products repeat (ties resolved by position)
    late      nearly complementary: S, Z spectra over 12 decades, S_i Z_i ~ mu = 1e-8, bases 1e-6 apart"""
    if cls == "interior":
        G1, G2 = rng.standard_normal((k, k)), rng.standard_normal((k, k))
        S, Z = G1 @ G1.T / k + np.eye(k), G2 @ G2.T / k + np.eye(k)
    elif cls == "cond":
        d = np.logspace(0, -3, k)
        C1, C2 = [G @ G.T / k + np.eye(k) for G in (rng.standard_normal((k, k)), rng.standard_normal((k, k)))]
        e = d[rng.permutation(k)]
        S, Z = (d[:, None] * C1) * d[None, :], (e[:, None] * C2) * e[None, :]
    elif cls == "identity":
        S, Z = np.eye(k), np.eye(k)
    elif cls == "scaled":
        G = rng.standard_normal((k, k))
        Z = G @ G.T / k + np.eye(k)
        S = 4.0 * Z
    elif cls == "cluster":
        vals = np.array([2.0, 1.0, 0.25])[np.arange(k) % 3]
        Rm = _orth(rng, k) * np.exp(rng.uniform(-0.5, 0.5, k))
        S = (Rm * vals) @ Rm.T
        Ri = np.linalg.inv(Rm)
        Z = (Ri.T * vals) @ Ri
    elif cls == "diagonal":
        a = np.exp(rng.uniform(-2, 2, k))
        p = np.array([1.0, 4.0, 0.25])[np.arange(k) % 3]
        S, Z = np.diag(a * p), np.diag(p / a)          # S_i Z_i in {1, 16, 1/16}: ties
    elif cls == "late":
        mu = 1e-8
        sd = np.logspace(-10, 2, k)
        zd = mu / sd * np.exp(rng.uniform(-0.5, 0.5, k))
        Q = _orth(rng, k)
        Gs = rng.standard_normal((k, k))
        Q2, _ = np.linalg.qr(Q @ (np.eye(k) + 1e-6 * (Gs - Gs.T)))
        Q2 = Q2 * np.sign(np.sum(Q2 * Q, axis=0))
        S, Z = (Q * sd) @ Q.T, (Q2 * zd) @ Q2.T
    else:
        raise ValueError(cls)
    S, Z = (S + S.T) / 2, (Z + Z.T) / 2
    return svec(S), svec(Z)


# ---------------------------------------------------------------------------------------------------------------
#  comparisons: observed error / bound per quantity (<= 1 passes)
# ---------------------------------------------------------------------------------------------------------------
def psd_ratios(ref, lam, R, Rinv, Hs=None):
    """lam (k, descending), R, Rinv (k x k) and the packed Hs block of one PSD cone against the reference.  The
    singular vectors are determined only up to sign (and rotations inside clusters), so R and Rinv are compared
    through R R' = A, Rinv'Rinv = A^{-1} and the identities R Rinv = I, R'ZR = Lam = Rinv S Rinv'."""
    b = psd_bounds(ref)
    k = ref["k"]
    L = np.diag(ref["lam"])
    out = dict(
        lam=ratio(lam - ref["lam"], b["lam"]),
        RRt=ratio(R @ R.T - ref["A"], b["A"]),
        RitRi=ratio(Rinv.T @ Rinv - ref["Ainv"], b["Ainv"]),
        RRinv=ratio(R @ Rinv - np.eye(k), b["RRinv"]),
        RZR=ratio(R.T @ ref["Z"] @ R - L, b["RZR"]),
        RiSRi=ratio(Rinv @ ref["S"] @ Rinv.T - L, b["RiSRi"]))
    if not np.all(np.diff(lam) <= 0):
        out["lam"] = np.inf
    if Hs is not None:
        H, _ = psd_hs(ref)
        out["Hs"] = ratio(Hs - H, b["Hs"])
    return out


def soc_ratios(ref, lam=None, w=None, eta=None, Hs=None, u=None, v=None, eta2=None):
    b = soc_bounds(ref)
    out = {}
    for key, val in (("lam", lam), ("w", w), ("eta", eta), ("Hs", Hs), ("u", u), ("v", v), ("eta2", eta2)):
        if val is not None:
            out["soc_" + key] = ratio(np.asarray(val) - ref[key], b[key])
    return out


class Worst:
    """worst observed error / bound per quantity over a test module (printed under -s)"""

    def __init__(self, title):
        self.title, self.r = title, {}

    def add(self, ratios, where=""):
        for key, val in ratios.items():
            if val > self.r.get(key, (-1.0, ""))[0]:
                self.r[key] = (val, where)
        return ratios

    def report(self):
        print(f"\n{self.title}: worst observed error / bound")
        for key in sorted(self.r):
            print(f"  {key:12s} {self.r[key][0]:9.3e}   {self.r[key][1]}")
