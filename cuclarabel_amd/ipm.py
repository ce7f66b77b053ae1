"""Interior-point test driver over the KKT-solver boundary.

A host-side (numpy) restatement of the reference's IPM loop for Zero / Nonnegative /
SecondOrder / PSDTriangle / Exponential / Power cones, without presolve, equilibration or chordal decomposition:

    solve!                          /root/reference/src/solver.jl:189-380
    default start                   solver.jl:383-404, kktsystem.jl:95-132, variables.jl:196-237
    residuals, mu                   residuals.jl:1-37, variables.jl:1-10
    termination                     info.jl:1-120,225-330 (full tolerances, settings.jl:76-81)
    reduced KKT solves, dtau etc.   kktsystem.jl:62-215
    rhs construction                variables.jl:107-190
    step lengths                    variables.jl:13-45, coneops_nncone.jl:151-170, coneops_socone.jl:443-512
    NT scaling, W, lambda           coneops_nncone.jl:77-114, coneops_socone.jl:75-154,302-412
    PSD cone                        coneops_psdtrianglecone.jl:8-44 (margins, shift), :78-143 (scaling), :164-254,
                                    :299-466 (mul_Hs!, ds offsets, W / W^-1, Jordan product, step length)

    generalized power cones         coneops_genpowcone.jl (dual scaling only, no higher-order correction)
    exponential / power cones       coneops_expcone.jl, coneops_powcone.jl, coneops_nonsymmetric_common.jl; the loop's
                                    branches for them: solver.jl:221 (strategy), :383-404 (unit start), :407-442 (barrier
                                    backtrack), :453-504 (checkpoints), variables.jl:46-72.  They fire only when such a cone
                                    is present; a symmetric problem takes the code path it always took.

It exists to drive a KKT backend through exactly the call sequence Clarabel uses
(`kktsolver_update!` -> constant-RHS solve -> affine solve -> combined solve, every iteration)
so that the reference's end-to-end known answers (test/OptTests/basic_*.jl) become parity
checks for the boundary.  The backend is anything with the `kktsolver_*` methods of
`cuclarabel_amd.kktsolver.HipKKTSolver`; cone scaling for the KKT update is done by the backend
(`update(s, z)`), the driver keeps its own numpy copy of the scaling for the step computations,
which stay on the host in the reference too (kktsystem.jl:135-215).
"""
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from .cones import (ZeroConeT, NonnegativeConeT, SecondOrderConeT, PSDTriangleConeT,
                    ExponentialConeT, PowerConeT, GenPowerConeT)

SOLVED, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE = "SOLVED", "PRIMAL_INFEASIBLE", "DUAL_INFEASIBLE"
MAX_ITERATIONS, NUMERICAL_ERROR, INSUFFICIENT_PROGRESS, UNSOLVED = \
    "MAX_ITERATIONS", "NUMERICAL_ERROR", "INSUFFICIENT_PROGRESS", "UNSOLVED"
ALMOST_SOLVED = "ALMOST_SOLVED"
PRIMAL_DUAL, DUAL = 0, 1      # ScalingStrategy (types.jl:74); the codes hipkkt_kkt_set_nonsymmetric_scaling takes


@dataclass
class IPMSettings:            # settings.jl:70-106 (code defaults)
    max_iter: int = 200
    max_step_fraction: float = 0.99
    tol_gap_abs: float = 1e-8
    tol_gap_rel: float = 1e-8
    tol_feas: float = 1e-8
    tol_infeas_abs: float = 1e-8
    tol_infeas_rel: float = 1e-8
    tol_ktratio: float = 1e-6
    min_terminate_step_length: float = 1e-4
    min_switch_step_length: float = 1e-1       # non-symmetric cones only (settings.jl)
    linesearch_backtrack_step: float = 0.8
    # reduced-accuracy tolerances (settings.jl:88-93), used by info_post_process! after an error exit
    reduced_tol_gap_abs: float = 5e-5
    reduced_tol_gap_rel: float = 5e-5
    reduced_tol_feas: float = 1e-4


@dataclass
class IPMResult:
    status: str
    x: np.ndarray
    z: np.ndarray
    s: np.ndarray
    obj_val: float
    obj_val_dual: float
    iterations: int
    kkt_ir_rounds: int = 0
    history: list = field(default_factory=list)


# ------------------------------------------------------------------------------------------
#  host cone operations (symmetric cones only)
# ------------------------------------------------------------------------------------------
class _Cone:
    def __init__(self, spec, off):
        self.spec, self.off, self.n = spec, off, spec.numel
        self.rng = slice(off, off + spec.numel)

    degree = 0


class _Zero(_Cone):
    degree = 0

    def margins(self, z):
        return np.finfo(float).max, 0.0

    def unit_shift(self, z, a, primal):
        if primal:
            z[:] = 0.0

    def update_scaling(self, s, z):
        return True

    def affine_ds(self, s):
        return np.zeros(self.n)

    def combined_ds_shift(self, dz, ds, sigma_mu):
        return np.zeros(self.n)

    def ds_from_dz_offset(self, ds, z):
        return np.zeros(self.n)

    def mul_Hs(self, x):
        return np.zeros(self.n)

    def get_Hs(self):                                    # coneops_zerocone.jl get_Hs!: zeros
        return np.zeros(self.n)

    def step_length(self, dz, ds, z, s, amax):
        return amax

    def unit_initialization(self):                       # coneops_zerocone.jl unit_initialization!
        return np.zeros(self.n), np.zeros(self.n)

    def compute_barrier(self, z, s, dz, ds, a):
        return 0.0


class _NN(_Cone):
    @property
    def degree(self):
        return self.n

    def margins(self, z):
        a = z.min() if self.n else np.finfo(float).max
        return a, float(np.sum(z[z > 0]))

    def unit_shift(self, z, a, primal):
        z += a

    def update_scaling(self, s, z):
        self.lam = np.sqrt(s * z)
        self.w = np.sqrt(s / z)
        return bool(np.all(np.isfinite(self.w)))

    def affine_ds(self, s):
        return self.lam ** 2

    def combined_ds_shift(self, dz, ds, sigma_mu):
        return (ds / self.w) * (self.w * dz) - sigma_mu          # W^-1 ds o W dz - sigma mu e

    def ds_from_dz_offset(self, ds, z):
        return ds / z

    def mul_Hs(self, x):
        return self.w * (self.w * x)

    def get_Hs(self):                                    # coneops_nncone.jl get_Hs!: w.^2
        return self.w ** 2

    def step_length(self, dz, ds, z, s, amax):
        a = amax
        m = dz < 0
        if m.any():
            a = min(a, float(np.min(-z[m] / dz[m])))
        m = ds < 0
        if m.any():
            a = min(a, float(np.min(-s[m] / ds[m])))
        return a

    def unit_initialization(self):
        return np.ones(self.n), np.ones(self.n)

    def compute_barrier(self, z, s, dz, ds, a):          # coneops_nncone.jl:172-189
        with np.errstate(all="ignore"):
            return -float(sum(_logsafe(v) for v in (s + a * ds) * (z + a * dz)))


def _soc_res(v):
    n1 = np.linalg.norm(v[1:])
    return (v[0] - n1) * (v[0] + n1)


class _SOC(_Cone):
    degree = 1

    def margins(self, z):
        a = z[0] - np.linalg.norm(z[1:])
        return a, max(0.0, a)

    def unit_shift(self, z, a, primal):
        z[0] += a

    def update_scaling(self, s, z):                      # coneops_socone.jl:75-123
        rs, rz = _soc_res(s), _soc_res(z)
        if not (rs > 0 and rz > 0):
            return False
        ss, zs = np.sqrt(rs), np.sqrt(rz)
        self.eta = np.sqrt(ss / zs)
        w = s / ss
        w[0] += z[0] / zs
        w[1:] -= z[1:] / zs
        rw = _soc_res(w)
        if not rw > 0:
            return False
        ws = np.sqrt(rw)
        w /= ws
        w[0] = np.sqrt(1 + w[1:] @ w[1:])
        self.w = w
        g = 0.5 * ws
        lam = np.empty(self.n)
        lam[0] = g
        lam[1:] = (((g + z[0] / zs) / ss) * s[1:] + ((g + s[0] / ss) / zs) * z[1:]) / (s[0] / ss + z[0] / zs + 2 * g)
        self.lam = lam * np.sqrt(ss * zs)
        return True

    def _W(self, x):                                     # mul_W!, :302-322
        zeta = self.w[1:] @ x[1:]
        c = x[0] + zeta / (1 + self.w[0])
        y = np.empty(self.n)
        y[0] = self.eta * (self.w[0] * x[0] + zeta)
        y[1:] = self.eta * (x[1:] + c * self.w[1:])
        return y

    def _Winv(self, x):                                  # mul_Winv!, :325-347
        zeta = self.w[1:] @ x[1:]
        c = -x[0] + zeta / (1 + self.w[0])
        y = np.empty(self.n)
        y[0] = (self.w[0] * x[0] - zeta) / self.eta
        y[1:] = (x[1:] + c * self.w[1:]) / self.eta
        return y

    @staticmethod
    def _circ(y, z):
        x = np.empty_like(y)
        x[0] = y @ z
        x[1:] = y[0] * z[1:] + z[0] * y[1:]
        return x

    def affine_ds(self, s):
        return self._circ(self.lam, self.lam)

    def combined_ds_shift(self, dz, ds, sigma_mu):
        out = self._circ(self._Winv(ds), self._W(dz))
        out[0] -= sigma_mu
        return out

    def ds_from_dz_offset(self, ds, z):                  # :243-268
        resz = _soc_res(z)
        l1 = self.lam[1:] @ ds[1:]
        w1 = self.w[1:] @ ds[1:]
        out = -z.copy()
        out[0] = z[0]
        out *= (self.lam[0] * ds[0] - l1) / resz
        out[0] += self.eta * w1
        out[1:] += self.eta * (ds[1:] + w1 / (1 + self.w[0]) * self.w[1:])
        return out / self.lam[0]

    def mul_Hs(self, x):
        c = 2 * (self.w @ x)
        y = x.copy()
        y[0] = -x[0]
        return (y + c * self.w) * self.eta ** 2

    @property
    def sparse(self):                                    # SOC_NO_EXPANSION_MAX_SIZE = 4 (cone_types.jl)
        return self.n > 4

    def sparse_data(self):                               # coneops_socone.jl:126-150: (u, v, d) of the rank-2 form of W'W
        w = self.w
        wsq = w[0] * w[0] + w[1:] @ w[1:]
        wsqinv = 1.0 / wsq
        d = wsqinv / 2
        u0 = np.sqrt(wsq - d)
        u1 = 2 * w[0] / u0
        v1 = np.sqrt(2 * (2 + wsqinv) / (2 * wsq - wsqinv))
        u, v = u1 * w, v1 * w
        u[0], v[0] = u0, 0.0
        return u, v, d

    def get_Hs(self):                                    # coneops_socone.jl:154-186
        e2 = self.eta ** 2
        if self.sparse:
            out = np.full(self.n, e2)
            out[0] *= self.sparse_data()[2]
            return out
        w = self.w
        blk = [(np.sqrt(2.0) * w[0] - 1.0) * (np.sqrt(2.0) * w[0] + 1.0)]
        for col in range(1, self.n):
            for row in range(col + 1):
                blk.append(2 * w[row] * w[col] + (1.0 if row == col else 0.0))
        return np.array(blk) * e2

    @staticmethod
    def _step(x, y, amax):                               # :443-512
        if x[0] >= 0 and y[0] < 0:
            amax = min(amax, -x[0] / y[0])
        a = _soc_res(y)
        b = 2 * (x[0] * y[0] - x[1:] @ y[1:])
        c = max(0.0, _soc_res(x))
        d = b * b - 4 * a * c
        if (a > 0 and b > 0) or d < 0:
            return amax
        if a == 0:
            return amax
        if c == 0:
            return amax if a >= 0 else 0.0
        t = (-b - np.sqrt(d)) if b >= 0 else (-b + np.sqrt(d))
        r1, r2 = (2 * c) / t, t / (2 * a)
        big = np.finfo(float).max
        r1 = big if r1 < 0 else r1
        r2 = big if r2 < 0 else r2
        return min(amax, r1, r2)

    def step_length(self, dz, ds, z, s, amax):
        return min(self._step(z, dz, amax), self._step(s, ds, amax))

    def unit_initialization(self):
        e = np.zeros(self.n)
        e[0] = 1.0
        return e.copy(), e

    def compute_barrier(self, z, s, dz, ds, a):          # coneops_socone.jl:287-305
        rs, rz = _soc_res(s + a * ds), _soc_res(z + a * dz)
        return -_logsafe(rs * rz) / 2 if rs > 0 and rz > 0 else np.inf


def _svec_to_mat(x, k):                                  # coneops_psdtrianglecone.jl:469-483
    M = np.zeros((k, k))
    iu = np.triu_indices(k)
    # svec runs down the columns of the upper triangle: (row, col) with row <= col, column-major
    order = np.lexsort((iu[0], iu[1]))
    r, c = iu[0][order], iu[1][order]
    v = np.where(r == c, x, x / np.sqrt(2.0))
    M[r, c] = v
    M[c, r] = v
    return M


def _mat_to_svec(M):                                     # :486-497
    k = M.shape[0]
    iu = np.triu_indices(k)
    order = np.lexsort((iu[0], iu[1]))
    r, c = iu[0][order], iu[1][order]
    return np.where(r == c, M[r, c], (M[r, c] + M[c, r]) / np.sqrt(2.0))


class _PSD(_Cone):
    def __init__(self, spec, off):
        super().__init__(spec, off)
        self.k = spec.dim
        self.diag = np.array([j * (j + 1) // 2 + j for j in range(self.k)], dtype=int)   # triangular_index - 1

    @property
    def degree(self):
        return self.k

    def margins(self, z):                                # :8-27
        if self.n == 0:
            return np.finfo(float).max, 0.0
        e = np.linalg.eigvalsh(_svec_to_mat(z, self.k))
        return float(e.min()), float(e[e > 0].sum())

    def unit_shift(self, z, a, primal):                  # :30-44
        z[self.diag] += a

    def update_scaling(self, s, z):                      # :78-143
        if self.n == 0:
            return True
        try:
            L1 = np.linalg.cholesky(_svec_to_mat(s, self.k))
            L2 = np.linalg.cholesky(_svec_to_mat(z, self.k))
        except np.linalg.LinAlgError:
            return False
        U, sv, Vt = np.linalg.svd(L2.T @ L1)
        self.lam = sv
        isq = 1.0 / np.sqrt(sv)
        self.R = (L1 @ Vt.T) * isq[None, :]
        self.Rinv = isq[:, None] * (U.T @ L2.T)
        return True

    def _W(self, x):                                     # mul_W!(:N): R' X R
        return _mat_to_svec(self.R.T @ _svec_to_mat(x, self.k) @ self.R)

    def _Wt(self, x):                                    # mul_W!(:T): R X R'
        return _mat_to_svec(self.R @ _svec_to_mat(x, self.k) @ self.R.T)

    def _WinvT(self, x):                                 # mul_Winv!(:T): Rinv X Rinv'
        return _mat_to_svec(self.Rinv @ _svec_to_mat(x, self.k) @ self.Rinv.T)

    def affine_ds(self, s):                              # :189-204
        out = np.zeros(self.n)
        out[self.diag] = self.lam ** 2
        return out

    def combined_ds_shift(self, dz, ds, sigma_mu):       # coneops_symmetric_common.jl:2-36, circ_op! :361-382
        Y = _svec_to_mat(self._WinvT(ds), self.k)
        Z = _svec_to_mat(self._W(dz), self.k)
        out = _mat_to_svec((Y @ Z + Z @ Y) / 2)
        out[self.diag] -= sigma_mu
        return out

    def ds_from_dz_offset(self, ds, z):                  # :218-228, lambda_inv_circ_op! :335-353
        X = _svec_to_mat(ds, self.k)
        X = 2.0 * X / (self.lam[:, None] + self.lam[None, :])
        return self._Wt(_mat_to_svec(X))

    def mul_Hs(self, x):                                 # :164-187
        return self._Wt(self._W(x))

    def get_Hs(self):                                    # :146-162: packed upper triangle of (R R') (x)_s (R R')
        t = self.n
        M = np.empty((t, t))
        for e in range(t):
            unit = np.zeros(t)
            unit[e] = 1.0
            M[:, e] = self.mul_Hs(unit)
        return np.concatenate([M[:col + 1, col] for col in range(t)]) if t else np.zeros(0)

    def _step_component(self, d, amax):                  # :439-466
        if self.n == 0:
            return amax
        isq = 1.0 / np.sqrt(self.lam)
        M = _svec_to_mat(d, self.k) * isq[:, None] * isq[None, :]
        g = float(np.linalg.eigvalsh(M).min())
        return min(1.0 / -g, amax) if g < 0 else amax

    def step_length(self, dz, ds, z, s, amax):           # :230-254
        return min(self._step_component(self._W(dz), amax), self._step_component(self._WinvT(ds), amax))

    def unit_initialization(self):
        e = np.zeros(self.n)
        e[self.diag] = 1.0
        return e.copy(), e

    def compute_barrier(self, z, s, dz, ds, a):          # coneops_psdtrianglecone.jl:256-295
        out = 0.0
        for v in (z + a * dz, s + a * ds):
            try:
                L = np.linalg.cholesky(_svec_to_mat(v, self.k))
            except np.linalg.LinAlgError:
                return np.inf
            out -= 2.0 * float(np.sum(np.log(np.diag(L))))
        return out


# ------------------------------------------------------------------------------------------
#  non-symmetric cones: exponential and power (coneops_expcone.jl, coneops_powcone.jl,
#  coneops_nonsymmetric_common.jl), restated term for term; the device kernel restates the same
# ------------------------------------------------------------------------------------------
_EPS = np.finfo(float).eps


def _logsafe(v):                                         # mathutils.jl:12-18; log(0) is -Inf as well
    return np.log(v) if v > 0 else -np.inf


def _wright_omega(z):                                    # coneops_expcone.jl:412-468
    if not z >= 0:
        return np.nan                                    # the reference throws; outside the cone only
    if z < 1 + np.pi:
        zm1 = z - 1
        p = zm1
        w = 1 + 0.5 * p
        p *= zm1
        w += (1 / 16.0) * p
        p *= zm1
        w -= (1 / 192.0) * p
        p *= zm1
        w -= (1 / 3072.0) * p
        p *= zm1
        w += (13 / 61440.0) * p
    else:
        logz = _logsafe(z)
        zinv = 1.0 / z
        w = z - logz
        q = logz * zinv
        w += q
        q *= zinv
        w += q * (logz / 2 - 1)
        # the reference's next line computes q*zinv and drops it (:451), so the cubic term is
        # weighted by log(z)/z^2; the two refinement rounds absorb the difference
        w += q * (logz * logz / 3. - (3 / 2.) * logz + 1)
    r = z - w - _logsafe(w)
    for _ in range(2):
        wp1 = w + 1
        t = wp1 * (wp1 + (2. * r) / 3.0)
        w *= 1 + (r / wp1) * (t - 0.5 * r) / (t - r)
        r = (2 * w * w - 8 * w - 1) / (72.0 * (wp1 * wp1 * wp1 * wp1 * wp1 * wp1)) * r * r * r * r
    return w


def _newton_raphson_onesided(x0, f0, f1):                # coneops_nonsymmetric_common.jl:170-193
    x, it = x0, 0
    while it < 100:
        it += 1
        dfdx = f1(x)
        dx = -f0(x) / dfdx
        if (dx < _EPS) or (abs(dx / x) < np.sqrt(_EPS)) or (abs(dfdx) < _EPS):
            break
        x += dx
    return x


def _newton_raphson_powcone(s3, phi, a):                 # coneops_powcone.jl:449-478
    x0 = -1.0 / s3 + (2 * s3 + np.sqrt(phi * phi / s3 / s3 + 3 * phi)) / (phi - s3 * s3)
    t0 = -2 * a * _logsafe(a) - 2 * (1 - a) * _logsafe(1 - a)

    def f0(x):
        t1 = x * x; t2 = 2 * x / s3
        return (2 * a * _logsafe(2 * a * t1 + (1 + a) * t2) + 2 * (1 - a) * _logsafe(2 * (1 - a) * t1 + (2 - a) * t2)
                - _logsafe(phi) - _logsafe(t1 + t2) - 2 * _logsafe(t2) + t0)

    def f1(x):
        t1 = x * x; t2 = x * 2 / s3
        return (2 * a * a / (a * x + (1 + a) / s3) + 2 * (1 - a) * (1 - a) / ((1 - a) * x + (2 - a) / s3)
                - 2 * (x + 1 / s3) / (t1 + t2))

    # The one-sided iteration needs f0(x0) > 0 (x0 left of the root), as the reference's own comment says (:455).  Its
    # x0 was derived for a differently scaled barrier and lies to the RIGHT of the root for alpha well away from 1/2
    # (alpha = 0.1, s = (1.03, 3.90, -2.28): x0 = 1.485, root 1.197), where the first Newton step is negative, the
    # iteration halts at once and g(s) comes out up to 26 % off.  f0 -> +Inf as x -> 0+, so halving reaches the left
    # side; this is the one deliberate departure from the reference, and the device kernel makes the same one.
    for _ in range(64):
        if f0(x0) > 0:
            break
        x0 *= 0.5
    return _newton_raphson_onesided(x0, f0, f1)


def _chol3_factor(A):                                    # mathutils.jl:427-451
    L = np.zeros((3, 3))
    t = A[0, 0]
    if not t > 0:
        return None
    L[0, 0] = np.sqrt(t)
    L[1, 0] = A[1, 0] / L[0, 0]
    t = A[1, 1] - L[1, 0] * L[1, 0]
    if not t > 0:
        return None
    L[1, 1] = np.sqrt(t)
    L[2, 0] = A[2, 0] / L[0, 0]
    L[2, 1] = (A[2, 1] - L[1, 0] * L[2, 0]) / L[1, 1]
    t = A[2, 2] - L[2, 0] * L[2, 0] - L[2, 1] * L[2, 1]
    if not t > 0:
        return None
    L[2, 2] = np.sqrt(t)
    return L


def _chol3_solve(L, b):                                  # mathutils.jl:455-466
    c1 = b[0] / L[0, 0]
    c2 = (b[1] * L[0, 0] - b[0] * L[1, 0]) / (L[0, 0] * L[1, 1])
    c3 = (b[2] * L[0, 0] * L[1, 1] - b[1] * L[0, 0] * L[2, 1] + b[0] * L[1, 0] * L[2, 1] - b[0] * L[1, 1] * L[2, 0]) \
        / (L[0, 0] * L[1, 1] * L[2, 2])
    x1 = (c1 * L[1, 1] * L[2, 2] - c2 * L[1, 0] * L[2, 2] + c3 * L[1, 0] * L[2, 1] - c3 * L[1, 1] * L[2, 0]) \
        / (L[0, 0] * L[1, 1] * L[2, 2])
    x2 = (c2 * L[2, 2] - c3 * L[2, 1]) / (L[1, 1] * L[2, 2])
    x3 = c3 / L[2, 2]
    return np.array([x1, x2, x3])


class _NonSym(_Cone):
    """What the exponential and the power cone share (coneops_nonsymmetric_common.jl)."""
    degree = 3
    symmetric = False

    def update_scaling(self, s, z, mu, strategy):        # update_scaling!: dual gradient and Hessian, then Hs
        with np.errstate(all="ignore"):
            s, z = np.asarray(s, dtype=np.float64), np.asarray(z, dtype=np.float64)
            self.grad, self.H_dual = self.dual_grad_H(z)
            if strategy == DUAL:
                self.Hs = mu * self.H_dual
                self.used_primal_dual = False
            else:
                self._primal_dual_scaling(s, z)
            self.z = z.copy()
        return bool(np.all(np.isfinite(self.Hs)))

    def scaling_guards(self, s, z):
        """(de1, de2, <s,z>, <ds,dz>) of use_primal_dual_scaling, for tests that must know how far a point is
        from the branch."""
        with np.errstate(all="ignore"):
            st, H = self.dual_grad_H(z)
            zt = self.gradient_primal(s)
            dot_sz = z @ s
            mu = dot_sz / 3
            mut = (zt @ st) / 3
            return mu * mut - 1, zt @ H @ zt - 3 * mut * mut, dot_sz, (s + mu * st) @ (z + mu * zt)

    def _primal_dual_scaling(self, s, z):                # use_primal_dual_scaling, :82-164
        st, H = self.grad, self.H_dual
        zt = self.gradient_primal(s)
        dot_sz = z[0] * s[0] + z[1] * s[1] + z[2] * s[2]
        mu = dot_sz / 3
        mut = (zt[0] * st[0] + zt[1] * st[1] + zt[2] * st[2]) / 3
        dls = s + mu * st
        dlz = z + mu * zt
        dot_dsz = dls[0] * dlz[0] + dls[1] * dlz[1] + dls[2] * dlz[2]
        de1 = mu * mut - 1
        Hzt = np.array([H[i, 0] * zt[0] + H[i, 1] * zt[1] + H[i, 2] * zt[2] for i in range(3)])
        de2 = (zt[0] * Hzt[0] + zt[1] * Hzt[1] + zt[2] * Hzt[2]) - 3 * mut * mut
        if abs(de1) > np.sqrt(_EPS) and abs(de2) > _EPS and dot_sz > 0 and dot_dsz > 0:
            tmp = np.array([mut * st[i] - H[i, 0] * zt[0] - H[i, 1] * zt[1] - H[i, 2] * zt[2] for i in range(3)])
            W = H.copy()
            for i in range(3):
                for j in range(3):
                    W[i, j] -= st[i] * st[j] / 3 + tmp[i] * tmp[j] / de2
            t = mu * np.sqrt(np.sum(W * W))
            ax = np.array([z[1] * zt[2] - z[2] * zt[1], z[2] * zt[0] - z[0] * zt[2], z[0] * zt[1] - z[1] * zt[0]])
            ax = ax / np.sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2])
            Hs = np.empty((3, 3))
            for i in range(3):
                for j in range(i, 3):
                    Hs[i, j] = s[i] * s[j] / dot_sz + dls[i] * dls[j] / dot_dsz + t * ax[i] * ax[j]
                    Hs[j, i] = Hs[i, j]
            self.Hs = Hs
            self.used_primal_dual = True
        else:
            self.Hs = mu * H                              # on the central path: mu H*(z) with the local mu
            self.used_primal_dual = False

    def get_Hs(self):                                    # pack_triu, mathutils.jl:402-412
        return np.array([self.Hs[r, c] for c in range(3) for r in range(c + 1)])

    def mul_Hs(self, x):
        H = self.Hs
        return np.array([H[i, 0] * x[0] + H[i, 1] * x[1] + H[i, 2] * x[2] for i in range(3)])

    def affine_ds(self, s):
        return s.copy()

    def combined_ds_shift(self, dz, ds, sigma_mu):
        with np.errstate(all="ignore"):
            return self.grad * sigma_mu - self.higher_correction(ds, dz)

    def ds_from_dz_offset(self, ds, z):
        return ds.copy()

    def _backtrack(self, dq, q, a, amin, step, in_cone):  # backtrack_search, :5-34
        while True:
            if in_cone(q + a * dq):
                break
            a *= step
            if a < amin:
                a = 0.0
                break
        return a

    def step_length(self, dz, ds, z, s, amax, st=None):
        st = st or IPMSettings()
        step, amin = st.linesearch_backtrack_step, st.min_terminate_step_length
        with np.errstate(all="ignore"):
            az = self._backtrack(dz, z, amax, amin, step, self.is_dual_feasible)
            as_ = self._backtrack(ds, s, amax, amin, step, self.is_primal_feasible)
        return min(az, as_)

    def compute_barrier(self, z, s, dz, ds, a):
        with np.errstate(all="ignore"):
            return self.barrier_dual(z + a * dz) + self.barrier_primal(s + a * ds)


class _Exp(_NonSym):
    """Primal: s3 >= s2 exp(s1/s2), s2, s3 > 0.  Dual: z3 >= -z1 exp(z2/z1 - 1), z3 > 0, z1 < 0.
    Dual barrier f*(z) = -log(z2 - z1 - z1 log(z3/-z1)) - log(-z1) - log(z3)."""

    def unit_initialization(self):                       # coneops_expcone.jl:36-52
        s = np.array([-1.051383945322714, 0.556409619469370, 1.258967884768947])
        return s.copy(), s

    def barrier_dual(self, z):
        l = _logsafe(-z[2] / z[0])
        return -_logsafe(-z[2] * z[0]) - _logsafe(z[1] - z[0] - z[0] * l)

    def barrier_primal(self, s):
        w = _wright_omega(1 - s[0] / s[1] - _logsafe(s[1] / s[2]))
        w = (w - 1) * (w - 1) / w
        return -_logsafe(w) - 2 * _logsafe(s[1]) - _logsafe(s[2]) - 3

    def is_primal_feasible(self, s):
        return bool(s[2] > 0 and s[1] > 0 and s[1] * _logsafe(s[2] / s[1]) - s[0] > 0)

    def is_dual_feasible(self, z):
        return bool(z[2] > 0 and z[0] < 0 and z[1] - z[0] - z[0] * _logsafe(-z[2] / z[0]) > 0)

    def gradient_primal(self, s):                        # :284-297
        w = _wright_omega(1 - s[0] / s[1] - _logsafe(s[1] / s[2]))
        g1 = 1.0 / ((w - 1.0) * s[1])
        g2 = g1 + g1 * _logsafe(w * s[1] / s[2]) - 1.0 / s[1]
        g3 = w / ((1.0 - w) * s[2])
        return np.array([g1, g2, g3])

    def dual_grad_H(self, z):                            # update_dual_grad_H, :370-399
        l = _logsafe(-z[2] / z[0])
        r = -z[0] * l - z[0] + z[1]
        c2 = 1.0 / r
        grad = np.array([c2 * l - 1 / z[0], -c2, (c2 * z[0] - 1) / z[2]])
        H = np.empty((3, 3))
        H[0, 0] = (r * r - z[0] * r + l * l * z[0] * z[0]) / (r * z[0] * z[0] * r)
        H[0, 1] = H[1, 0] = -l / (r * r)
        H[1, 1] = 1 / (r * r)
        H[0, 2] = H[2, 0] = (z[1] - z[0]) / (r * r * z[2])
        H[1, 2] = H[2, 1] = -z[0] / (r * r * z[2])
        H[2, 2] = (r * r - z[0] * r + z[0] * z[0]) / (r * r * z[2] * z[2])
        return grad, H

    def higher_correction(self, ds, v):                  # :319-366
        z = self.z
        L = _chol3_factor(self.H_dual)
        if L is None:
            return np.zeros(3)
        u = _chol3_solve(L, ds)
        eta = np.zeros(3)
        eta[1] = 1.0
        eta[2] = -z[0] / z[2]
        eta[0] = _logsafe(eta[2])
        psi = z[0] * eta[0] - z[0] + z[1]
        dpu = eta @ u
        dpv = eta @ v
        coef = ((u[0] * (v[0] / z[0] - v[2] / z[2]) + u[2] * (z[0] * v[2] / z[2] - v[0]) / z[2]) * psi
                - 2 * dpu * dpv) / (psi * psi * psi)
        eta *= coef
        ip2 = 1.0 / psi / psi
        eta[0] += (1 / psi - 2 / z[0]) * u[0] * v[0] / (z[0] * z[0]) - u[2] * v[2] / (z[2] * z[2]) / psi \
            + dpu * ip2 * (v[0] / z[0] - v[2] / z[2]) + dpv * ip2 * (u[0] / z[0] - u[2] / z[2])
        eta[2] += 2 * (z[0] / psi - 1) * u[2] * v[2] / (z[2] * z[2] * z[2]) \
            - (u[2] * v[0] + u[0] * v[2]) / (z[2] * z[2]) / psi \
            + dpu * ip2 * (z[0] * v[2] / (z[2] * z[2]) - v[0] / z[2]) \
            + dpv * ip2 * (z[0] * u[2] / (z[2] * z[2]) - u[0] / z[2])
        return eta / 2


class _Pow(_NonSym):
    """Primal: s1^a s2^(1-a) >= |s3|, s1, s2 >= 0.  Dual: (z1/a)^a (z2/(1-a))^(1-a) >= |z3|.
    Dual barrier f*(z) = -log((z1/a)^2a (z2/(1-a))^(2-2a) - z3^2) - (1-a) log z1 - a log z2."""

    def __init__(self, spec, off):
        super().__init__(spec, off)
        self.alpha = float(spec.alpha)

    def unit_initialization(self):                       # coneops_powcone.jl:36-54
        a = self.alpha
        s = np.array([np.sqrt(1 + a), np.sqrt(1 + (1 - a)), 0.0])
        return s.copy(), s

    def barrier_dual(self, z):
        a = self.alpha
        return -_logsafe((z[0] / a) ** (2 * a) * (z[1] / (1 - a)) ** (2 - 2 * a) - z[2] * z[2]) \
            - (1 - a) * _logsafe(z[0]) - a * _logsafe(z[1])

    def barrier_primal(self, s):
        a = self.alpha
        g = self.gradient_primal(s)
        return _logsafe((-g[0] / a) ** (2 * a) * (-g[1] / (1 - a)) ** (2 - 2 * a) - g[2] * g[2]) \
            + (1 - a) * _logsafe(-g[0]) + a * _logsafe(-g[1]) - 3

    def is_primal_feasible(self, s):
        a = self.alpha
        return bool(s[0] > 0 and s[1] > 0 and
                    np.exp(2 * a * _logsafe(s[0]) + 2 * (1 - a) * _logsafe(s[1])) - s[2] * s[2] > 0)

    def is_dual_feasible(self, z):
        a = self.alpha
        return bool(z[0] > 0 and z[1] > 0 and
                    np.exp(2 * a * _logsafe(z[0] / a) + 2 * (1 - a) * _logsafe(z[1] / (1 - a))) - z[2] * z[2] > 0)

    def gradient_primal(self, s):                        # :288-316
        a = self.alpha
        s = np.asarray(s, dtype=np.float64)
        phi = s[0] ** (2 * a) * s[1] ** (2 - 2 * a)
        g = np.zeros(3)
        abs_s = abs(s[2])
        if abs_s > _EPS:
            g[2] = _newton_raphson_powcone(abs_s, phi, a)
            if s[2] < 0:
                g[2] = -g[2]
            g[0] = -(a * g[2] * s[2] + 1 + a) / s[0]
            g[1] = -((1 - a) * g[2] * s[2] + 2 - a) / s[1]
        else:
            g[2] = 0.0
            g[0] = -(1 + a) / s[0]
            g[1] = -(2 - a) / s[1]
        return g

    def dual_grad_H(self, z):                            # update_dual_grad_H, :408-440
        a = self.alpha
        z = np.asarray(z, dtype=np.float64)
        phi = (z[0] / a) ** (2 * a) * (z[1] / (1 - a)) ** (2 - 2 * a)
        psi = phi - z[2] * z[2]
        g = np.array([2 * a * phi / (z[0] * psi), 2 * (1 - a) * phi / (z[1] * psi), -2 * z[2] / psi])
        H = np.empty((3, 3))
        H[0, 0] = g[0] * g[0] - 2 * a * (2 * a - 1) * phi / (z[0] * z[0] * psi) + (1 - a) / (z[0] * z[0])
        H[0, 1] = H[1, 0] = g[0] * g[1] - 4 * a * (1 - a) * phi / (z[0] * z[1] * psi)
        H[1, 1] = g[1] * g[1] - 2 * (1 - a) * (1 - 2 * a) * phi / (z[1] * z[1] * psi) + a / (z[1] * z[1])
        H[0, 2] = H[2, 0] = g[0] * g[2]
        H[1, 2] = H[2, 1] = g[1] * g[2]
        H[2, 2] = g[2] * g[2] + 2 / psi
        grad = np.array([-2 * a * phi / (z[0] * psi) - (1 - a) / z[0],
                         -2 * (1 - a) * phi / (z[1] * psi) - a / z[1],
                         2 * z[2] / psi])
        return grad, H

    def higher_correction(self, ds, v):                  # :329-404
        z, a = self.z, self.alpha
        L = _chol3_factor(self.H_dual)
        if L is None:
            return np.zeros(3)
        u = _chol3_solve(L, ds)
        phi = (z[0] / a) ** (2 * a) * (z[1] / (1 - a)) ** (2 - 2 * a)
        psi = phi - z[2] * z[2]
        eta = np.array([2 * a * phi / z[0], 2 * (1 - a) * phi / z[1], -2 * z[2]])
        H11 = 2 * a * (2 * a - 1) * phi / (z[0] * z[0])
        H12 = 4 * a * (1 - a) * phi / (z[0] * z[1])
        H22 = 2 * (1 - a) * (1 - 2 * a) * phi / (z[1] * z[1])
        dpu = eta @ u
        dpv = eta @ v
        Hv = np.array([H11 * v[0] + H12 * v[1], H12 * v[0] + H22 * v[1], -2 * v[2]])
        coef = ((u @ Hv) * psi - 2 * dpu * dpv) / (psi * psi * psi)
        coef2 = 4 * a * (2 * a - 1) * (1 - a) * phi * (u[0] / z[0] - u[1] / z[1]) * (v[0] / z[0] - v[1] / z[1]) / psi
        ip2 = 1 / psi / psi
        e0 = coef * eta[0] - 2 * (1 - a) * u[0] * v[0] / (z[0] * z[0] * z[0]) + coef2 / z[0] + Hv[0] * dpu * ip2
        e1 = coef * eta[1] - 2 * a * u[1] * v[1] / (z[1] * z[1] * z[1]) - coef2 / z[1] + Hv[1] * dpu * ip2
        e2 = coef * eta[2] + Hv[2] * dpu * ip2
        Hu = np.array([H11 * u[0] + H12 * u[1], H12 * u[0] + H22 * u[1], -2 * u[2]])
        return (np.array([e0, e1, e2]) + Hu * dpv * ip2) / 2


def _newton_raphson_genpowcone(norm_r, p, phi, alpha, psi):   # coneops_genpowcone.jl:437-472
    x0 = -1.0 / norm_r + (psi * norm_r + np.sqrt((phi / norm_r / norm_r + psi * psi - 1.0) * phi)) / (phi - norm_r * norm_r)

    def f0(x):
        out = -_logsafe(2 * x / norm_r + x * x)
        for i in range(len(alpha)):
            out += 2 * alpha[i] * (_logsafe(x * norm_r + (1 + alpha[i]) / alpha[i]) - _logsafe(p[i]))
        return out

    def f1(x):
        out = -(2 * x + 2 / norm_r) / (x * x + 2 * x / norm_r)
        for i in range(len(alpha)):
            out += 2 * alpha[i] * norm_r / (norm_r * x + (1 + alpha[i]) / alpha[i])
        return out

    # the one-sided iteration needs f0(x0) > 0 (it stops at the first non-positive step); f0 -> +Inf as x -> 0+, so a
    # start right of the root is halved until it is left of it -- the guard _newton_raphson_powcone has
    k = 0
    while k < 64 and not f0(x0) > 0:
        x0, k = 0.5 * x0, k + 1
    return _newton_raphson_onesided(x0, f0, f1)


class _GenPow(_NonSym):
    """Primal: prod_i s_i^a_i >= ||s[d1:]||, s[:d1] >= 0.  Dual: prod_i (z_i/a_i)^a_i >= ||z[d1:]||, z[:d1] >= 0.
    Dual barrier f*(z) = -log(prod_i (z_i/a_i)^(2 a_i) - ||z[d1:]||^2) - sum_i (1 - a_i) log z_i
    (coneops_genpowcone.jl).  Dual scaling only (allows_primal_dual_scaling is false): Hs = mu H*(z) =
    mu (diag(d) + p p' - q q' - r r'), which enters K as a diagonal block and three expansion columns."""

    def __init__(self, spec, off):
        super().__init__(spec, off)
        self.alpha = np.array(spec.alpha, dtype=np.float64)
        self.d1, self.d2 = len(spec.alpha), int(spec.dim2)
        self.degree = self.d1 + 1
        self.psi = 1.0 / float(self.alpha @ self.alpha)          # cone_types.jl:301
        self.mu = 1.0

    def unit_initialization(self):                       # :34-53
        s = np.concatenate([np.sqrt(1.0 + self.alpha), np.zeros(self.d2)])
        return s.copy(), s

    def dual_grad_H(self, z):                            # update_dual_grad_H, :336-389: (grad, (d, p, q, r))
        a, d1 = self.alpha, self.d1
        z = np.asarray(z, dtype=np.float64)
        phi = 1.0
        for i in range(d1):
            phi *= (z[i] / a[i]) ** (2 * a[i])
        norm2w = 0.0
        for i in range(d1, self.n):
            norm2w += z[i] * z[i]
        zeta = phi - norm2w
        u, w = z[:d1], z[d1:]
        tau = 2 * a / u
        grad = np.concatenate([-tau * phi / zeta - (1 - a) / u, 2 * w / zeta])
        p0 = np.sqrt(phi * (phi + norm2w) / 2)
        p1 = -2 * phi / p0
        q0 = np.sqrt(zeta * phi / 2)
        r1 = 2 * np.sqrt(zeta / (phi + norm2w))
        dd = np.concatenate([tau * phi / (zeta * u) + (1 - a) / (u * u), np.full(self.d2, 2 / zeta)])
        p = np.concatenate([p0 * tau / zeta, p1 * w / zeta])
        q = tau * (q0 / zeta)
        r = r1 * w / zeta
        self.zeta = zeta
        return grad, (dd, p, q, r)

    def update_scaling(self, s, z, mu, strategy):        # :64-82; the strategy is not read
        with np.errstate(all="ignore"):
            z = np.asarray(z, dtype=np.float64)
            self.grad, (self.d, self.p, self.q, self.r) = self.dual_grad_H(z)
            self.mu = mu
            self.z = z.copy()
            self.used_primal_dual = False
        # (the reference asserts zeta > 0 here)
        return bool(self.zeta > 0 and np.all(z[:self.d1] > 0) and np.all(np.isfinite(self.p)))

    @property
    def H_dual(self):                                    # dense H*(z), for tests
        P = np.diag(self.d) + np.outer(self.p, self.p)
        P[:self.d1, :self.d1] -= np.outer(self.q, self.q)
        P[self.d1:, self.d1:] -= np.outer(self.r, self.r)
        return P

    @property
    def Hs(self):
        return self.mu * self.H_dual

    def get_Hs(self):                                    # :91-108: the diagonal block only
        return self.mu * self.d

    def sparse_data(self):                               # _csc_update_sparsecone: (q, r, p) scaled by -sqrt(mu), D
        sm = -np.sqrt(self.mu)
        return self.q * sm, self.r * sm, self.p * sm, np.array([-1.0, -1.0, 1.0])

    def mul_Hs(self, x):                                 # :110-135
        d1 = self.d1
        cp, cq, cr = self.p @ x, self.q @ x[:d1], self.r @ x[d1:]
        y = self.d * x
        y[:d1] -= cq * self.q
        y[d1:] -= cr * self.r
        y += cp * self.p
        return y * self.mu

    def combined_ds_shift(self, dz, ds, sigma_mu):       # :149-168: no higher-order correction
        return self.grad * sigma_mu

    def _phi2(self, v, scaled):                          # exp(sum 2 a_i log(v_i [/ a_i])) - ||v[d1:]||^2
        a, d1 = self.alpha, self.d1
        res = 0.0
        for i in range(d1):
            res += 2 * a[i] * _logsafe(v[i] / a[i] if scaled else v[i])
        return np.exp(res) - float(v[d1:] @ v[d1:])

    def is_primal_feasible(self, s):                     # :249-269
        return bool(np.all(s[:self.d1] > 0) and self._phi2(s, False) > 0)

    def is_dual_feasible(self, z):                       # :272-292
        return bool(np.all(z[:self.d1] > 0) and self._phi2(z, True) > 0)

    def barrier_dual(self, z):                           # :313-333
        out = -_logsafe(self._phi2(z, True))
        for i in range(self.d1):
            out -= (1 - self.alpha[i]) * _logsafe(z[i])
        return out

    def barrier_primal(self, s):                         # :294-310
        return -self.barrier_dual(-self.gradient_primal(s)) - self.degree

    def gradient_primal(self, s):                        # :393-426
        a, d1 = self.alpha, self.d1
        s = np.asarray(s, dtype=np.float64)
        phi = 1.0
        for i in range(d1):
            phi *= s[i] ** (2 * a[i])
        pp, rr = s[:d1], s[d1:]
        norm_r = float(np.sqrt(rr @ rr))
        g = np.zeros(self.n)
        if norm_r > _EPS:
            g1 = _newton_raphson_genpowcone(norm_r, pp, phi, a, self.psi)
            g[d1:] = g1 * rr / norm_r
            g[:d1] = -(1 + a + a * g1 * norm_r) / pp
        else:
            g[:d1] = -(1 + a) / pp
        return g

    def higher_correction(self, ds, v):
        return np.zeros(self.n)


def adopt_device_scaling(cones, dev_scaling):
    """Give the host PSD cone objects the (R, Rinv, lambda) triples `HipKKTSolver.scaling()` returns."""
    it = iter(dev_scaling)
    for c in cones:
        if isinstance(c, _PSD):
            c.R, c.Rinv, c.lam = next(it)


def adopt_device_genpow(cones, dev_genpow):
    """Give the host generalized power cones the (grad, d, p, q, r) `HipKKTSolver.genpow()` returns.  In the reference
    one cone object serves K, mul_Hs! and combined_ds_shift!.  zeta = phi - ||w||^2 cancels towards the boundary, so a
    host scaling that reduces phi in another order than the device differs from the device's by eps phi / zeta, and
    ds = -(Hs dz + ...) formed with it does not belong to the dz that the device's K gave: the primal residual then
    stops falling short of the tolerance."""
    for c, (grad, d, p, q, r) in zip([c for c in cones if isinstance(c, _GenPow)], dev_genpow):
        c.grad, c.d, c.p, c.q, c.r = grad, d, p, q, r


def host_cone_data(cones):
    """What the Julia glue reads from the reference's cone objects for kkt_update! (hipkkt_kkt_system_update_cones):
    get_Hs! blocks, the sparse second-order cones' (u, v, eta^2), and the NT scaling w (m), eta (per cone), lambda (m),
    R / Rinv of the PSD cones (column-major, concatenated).  After update_scaling on every cone."""
    m = cones[-1].off + cones[-1].n if cones else 0
    Hs, u, v, e2, R, Ri = [], [], [], [], [], []
    w, lam, eta = np.ones(m), np.zeros(m), np.ones(len(cones))
    for i, c in enumerate(cones):
        Hs.append(c.get_Hs())
        if isinstance(c, (_NN, _SOC)):
            w[c.rng] = c.w
            lam[c.rng] = c.lam
        if isinstance(c, _SOC):
            eta[i] = c.eta
            if c.sparse:
                uu, vv, _ = c.sparse_data()
                u.append(uu); v.append(vv); e2.append(c.eta ** 2)
        if isinstance(c, _PSD) and c.n:
            lam[c.off:c.off + c.k] = c.lam
            R.append(np.asarray(c.R).ravel(order="F")); Ri.append(np.asarray(c.Rinv).ravel(order="F"))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)
    return cat(Hs), cat(u), cat(v), np.array(e2), w, eta, lam, cat(R), cat(Ri)


def _make_cones(specs):
    out, off = [], 0
    for c in specs:
        if isinstance(c, ZeroConeT):
            out.append(_Zero(c, off))
        elif isinstance(c, NonnegativeConeT):
            out.append(_NN(c, off))
        elif isinstance(c, SecondOrderConeT):
            out.append(_SOC(c, off))
        elif isinstance(c, PSDTriangleConeT):
            out.append(_PSD(c, off))
        elif isinstance(c, ExponentialConeT):
            out.append(_Exp(c, off))
        elif isinstance(c, PowerConeT):
            out.append(_Pow(c, off))
        elif isinstance(c, GenPowerConeT):
            out.append(_GenPow(c, off))
        else:
            raise NotImplementedError("the IPM test driver covers Zero, Nonnegative, SecondOrder, PSDTriangle, "
                                      "Exponential, Power and GenPower cones")
        off += c.numel
    return out


def identity_scaling_data(specs):
    """What get_Hs! and the sparse SOC data look like under set_identity_scaling!
    (coneops_*cone.jl set_identity_scaling!): Hsblocks, soc_u, soc_v, soc_eta2."""
    Hs, u, v, e2 = [], [], [], []
    for c in specs:
        if isinstance(c, ZeroConeT):
            Hs.append(np.zeros(c.dim))
        elif isinstance(c, NonnegativeConeT):
            Hs.append(np.ones(c.dim))
        elif isinstance(c, SecondOrderConeT):
            if c.dim > 4:
                d = np.ones(c.dim)
                d[0] = 0.5
                Hs.append(d)
                uu = np.zeros(c.dim)
                uu[0] = np.sqrt(0.5)
                u.append(uu)
                v.append(np.zeros(c.dim))
                e2.append(1.0)
            else:
                # packed triu of eta^2 (2 w w' - J) at w = e_1, eta = 1, with the reference's
                # cancellation-free first entry (coneops_socone.jl:168-186)
                blk = []
                for col in range(c.dim):
                    for row in range(col + 1):
                        blk.append(1.0 if row == col else 0.0)
                blk[0] = (np.sqrt(2.0) * 1.0 - 1.0) * (np.sqrt(2.0) * 1.0 + 1.0)
                Hs.append(np.array(blk))
        elif isinstance(c, PSDTriangleConeT):
            # Hs = I (coneops_psdtrianglecone.jl:65-75), packed upper triangle of the t x t identity
            t = c.numel
            blk = np.zeros(t * (t + 1) // 2)
            blk[[j * (j + 1) // 2 + j for j in range(t)]] = 1.0
            Hs.append(blk)
        else:
            raise NotImplementedError
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)
    return cat(Hs), cat(u), cat(v), np.array(e2)


# ------------------------------------------------------------------------------------------
#  the loop
# ------------------------------------------------------------------------------------------
def solve(P, q, A, b, cone_specs, backend, settings=None):
    """Clarabel.solve! restated.  `backend` must offer
         update_identity()            -> bool     (kkt_update! under set_identity_scaling!)
         update(s, z)                 -> bool     (kktsolver_update! after update_scaling!(s,z))
         kktsolver_setrhs(rx, rz); kktsolver_solve(x_out, z_out) -> bool
         last_ir_iterations
       and may offer
         psd_scaling()                -> [(R, Rinv, lambda) per PSD cone] of the scaling the last update(s, z) built K
                                         from; the host's PSD cone objects then adopt it (one scaling per iteration)
    """
    st = settings or IPMSettings()
    P = sp.csc_matrix(P)
    Pt = sp.triu(P, format="csc")
    Pfull = (Pt + sp.triu(Pt, 1).T).tocsr()
    A = sp.csr_matrix(A)
    At = A.T.tocsr()
    q, b = np.asarray(q, float), np.asarray(b, float)
    n, m = Pfull.shape[0], A.shape[0]
    cones = _make_cones(cone_specs)
    degree = sum(c.degree for c in cones)
    normq = np.abs(q).max() if n else 0.0
    normb = np.abs(b).max() if m else 0.0
    ir_total = 0

    def each(fn, *vecs):
        out = np.empty(m)
        for c in cones:
            out[c.rng] = fn(c, *[v[c.rng] for v in vecs])
        return out

    def ksolve(rx, rz, want_x=True, want_z=True):
        nonlocal ir_total
        backend.kktsolver_setrhs(rx, rz)
        xo, zo = np.zeros(n), np.zeros(m)
        ok = backend.kktsolver_solve(xo if want_x else None, zo if want_z else None)
        ir_total += backend.last_ir_iterations
        return ok, xo, zo

    # ---- default start: solver.jl:383-404
    x = np.zeros(n); s = np.zeros(m); z = np.zeros(m)
    system = getattr(backend, "system", None)          # device-resident DefaultKKTSystem (level C), if the backend has one
    if system is not None:
        system.init(q, b)
    # With a non-symmetric cone the start is the unit point on the central ray (variables_unit_initialization!):
    # no identity update and no initial-point solve is issued.  `strategy` is the reference's `scaling` variable
    # (solver.jl:221); it and its three checkpoints (:453-504) exist only on that path.
    nonsym = any(isinstance(c, _NonSym) for c in cones)
    strategy = PRIMAL_DUAL
    x2 = z2 = None
    if nonsym:
        for c in cones:
            z[c.rng], s[c.rng] = c.unit_initialization()
    else:
        ok = backend.update_identity()
    if nonsym:
        pass
    elif system is not None:
        ok_c = system.solve_constant_rhs()
        ok1, x, s, z = system.solve_initial_point()
        ok2 = True
        x2 = z2 = None
    else:
        ok_c, x2, z2 = ksolve(-q, b)                   # kkt_update! also solves the constant RHS
    if system is not None or nonsym:
        pass
    elif Pt.nnz == 0:                                  # kktsystem.jl:101-120 (LP initialisation)
        ok1, x, s = ksolve(np.zeros(n), b)
        s = -s
        ok2, _, z = ksolve(-q, np.zeros(m), want_x=False)
    else:                                              # :121-129 (QP initialisation)
        ok1, x, z = ksolve(-q, b)
        s = -z.copy()
        ok2 = True

    def shift_to_interior(v, primal):                  # variables.jl:213-237
        mins, pos = np.finfo(float).max, 0.0
        for c in cones:
            a, bb = c.margins(v[c.rng])
            mins, pos = min(mins, a), pos + bb
        target = max(1.0, 0.1 * pos / max(degree, 1))
        shifts = []
        if mins <= 0:
            shifts = [-mins, target]
        elif mins < target:
            shifts = [target - mins]
        else:
            shifts = [0.0]
        for a in shifts:
            for c in cones:
                c.unit_shift(v[c.rng], a, primal)

    if not nonsym:
        shift_to_interior(s, True)
        shift_to_interior(z, False)
    tau, kappa = 1.0, 1.0

    it, alpha, sigma = 0, 0.0, 1.0
    status = UNSOLVED
    prev = None
    hist = []
    prev_vars = None
    while True:
        # ---- residuals (residuals.jl:1-37)
        qx, bz, sz = q @ x, b @ z, s @ z
        Px = Pfull @ x
        xPx = x @ Px
        rx_inf = -(At @ z)
        rz_inf = A @ x + s
        rx = rx_inf - Px - q * tau
        rz = rz_inf - b * tau
        rtau = qx + bz + kappa + xPx / tau
        mu = (sz + tau * kappa) / (degree + 1)
        # ---- info_update! (info.jl:1-63), no equilibration
        tinv = 1.0 / tau
        cost_p = qx * tinv + xPx * tinv * tinv / 2
        cost_d = -bz * tinv - xPx * tinv * tinv / 2
        nx, nz, ns = np.linalg.norm(x), np.linalg.norm(z), np.linalg.norm(s)
        res_pinf = np.linalg.norm(rx_inf) / max(1.0, nz)
        res_dinf = max(np.linalg.norm(Px) / max(1.0, nx), np.linalg.norm(rz_inf) / max(1.0, nx + ns))
        nx, nz, ns = nx * tinv, nz * tinv, ns * tinv
        res_p = np.linalg.norm(rz) * tinv / max(1.0, normb + nx + ns)
        res_d = np.linalg.norm(rx) * tinv / max(1.0, normq + nx + nz)
        gap_abs = abs(cost_p - cost_d)
        gap_rel = gap_abs / max(1.0, min(abs(cost_p), abs(cost_d)))
        kt = kappa * tinv
        hist.append(dict(iter=it, pcost=cost_p, dcost=cost_d, gap=gap_abs, pres=res_p, dres=res_d, kt=kt, mu=mu,
                         step=alpha))
        # ---- termination (info.jl:65-120, 270-330)
        status = UNSOLVED
        if kt <= 1 and (gap_abs < st.tol_gap_abs or gap_rel < st.tol_gap_rel) and res_p < st.tol_feas and res_d < st.tol_feas:
            status = SOLVED
        elif kt > 1000.0 / st.tol_ktratio:
            if bz < -st.tol_infeas_abs and res_pinf < -st.tol_infeas_rel * bz:
                status = PRIMAL_INFEASIBLE
            elif qx < -st.tol_infeas_abs and res_dinf < -st.tol_infeas_rel * qx:
                status = DUAL_INFEASIBLE
        if status == UNSOLVED and it > 1 and prev is not None and (res_d > prev["res_d"] or res_p > prev["res_p"]):
            if kt < 100 * np.finfo(float).eps and (prev["gap_abs"] < st.tol_gap_abs or prev["gap_rel"] < st.tol_gap_rel):
                status = INSUFFICIENT_PROGRESS
            if kt < 1 and ((res_d > 100 * st.tol_feas and res_d > 100 * prev["res_d"]) or
                           (res_p > 100 * st.tol_feas and res_p > 100 * prev["res_p"])):
                status = INSUFFICIENT_PROGRESS
        if status == UNSOLVED and it == st.max_iter:
            status = MAX_ITERATIONS
        if status != UNSOLVED:
            if status == INSUFFICIENT_PROGRESS and prev_vars is not None:
                x, s, z, tau, kappa = prev_vars
            if status == INSUFFICIENT_PROGRESS and nonsym and strategy == PRIMAL_DUAL:
                # _strategy_checkpoint_insufficient_progress: go on from the previous iterate with dual scaling
                strategy, status = DUAL, UNSOLVED
                continue
            break
        # ---- scale cones, KKT update + constant-RHS solve (solver.jl:258-280, kktsystem.jl:62-92)
        if not all(c.update_scaling(s[c.rng].copy(), z[c.rng].copy(), mu, strategy) if isinstance(c, _NonSym)
                   else c.update_scaling(s[c.rng].copy(), z[c.rng].copy()) for c in cones):
            status = NUMERICAL_ERROR
            break
        it += 1
        aff_step = None
        if nonsym and system is not None:
            backend.ks.set_nonsymmetric_scaling(strategy, mu)      # host-only; every update route below picks it up
        if system is not None and getattr(backend, "batch_affine", False):
            # kkt_update! and the affine kkt_solve! as ONE call: the constant and the affine right-hand side do not
            # depend on each other (kktsystem.jl:87-88 vs :170-171; the affine step does not read rhs.s, :157-158),
            # so their solves share every triangular sweep
            ok, aff_step = system.update_and_solve_affine(rx, rz, rtau, tau * kappa, x, s, z, tau, kappa)
            ir_total += backend.last_ir_iterations
            if ok and any(isinstance(c, _PSD) and c.n for c in cones):
                adopt_device_scaling(cones, backend.ks.scaling()[1])
        elif system is not None and getattr(backend, "host_cones", False):
            # kkt_update!(kktsystem, data, cones) as the Julia glue issues it: everything from the caller's cone objects
            ok = system.update_cones(*host_cone_data(cones))
        elif system is not None:
            ok = system.update(s, z)                   # kkt_update!: scaling, refactor, constant-RHS solve
            # The scaled space of a PSD cone is fixed only up to the signs of the singular vectors of L2'L1.  With the
            # reduced system on the device, ITS scaling is the one the right-hand sides must be expressed in (in the
            # reference one cone object serves both sides): adopt the device's R, Rinv, lambda.
            if ok and any(isinstance(c, _PSD) and c.n for c in cones):
                adopt_device_scaling(cones, backend.ks.scaling()[1])
        else:
            ok = backend.update(s, z, mu=mu, strategy=strategy) if nonsym else backend.update(s, z)
            # A backend that can say which PSD scaling its K was built from (psd_scaling() -> [(R, Rinv, lambda)]) is
            # asked: ds = -(Hs dz + ...) formed with the host's own R does not belong to the dz that K gave, the
            # two A = R R' differ by eps cond, and on the 1225-row blocks of a nearly complementary PSD(49) the primal
            # residual then grows again from 1e-8 (as adopt_device_genpow's note says of the generalized power cone).
            if ok and hasattr(backend, "psd_scaling") and any(isinstance(c, _PSD) and c.n for c in cones):
                adopt_device_scaling(cones, backend.psd_scaling())
            if ok:
                ok, x2, z2 = ksolve(-q, b)

        if ok and hasattr(backend, "ks") and any(isinstance(c, _GenPow) for c in cones):
            adopt_device_genpow(cones, backend.ks.genpow())

        def kkt_solve(rhs_x, rhs_z, rhs_s, rhs_tau, rhs_kappa, affine, lhs_z_work=None):   # kktsystem.jl:135-215
            nonlocal ir_total
            if system is not None:
                okk, out = system.solve(rhs_x, rhs_s, rhs_z, rhs_tau, rhs_kappa, x, s, z, tau, kappa, affine)
                ir_total += backend.last_ir_iterations
                return okk, out
            if affine:
                const = s.copy()
            else:
                const = each(lambda c, ds, zz: c.ds_from_dz_offset(ds, zz), rhs_s, z)
            okk, x1, z1 = ksolve(rhs_x, const - rhs_z)
            if not okk:
                return False, None
            xi = x / tau
            tnum = rhs_tau - rhs_kappa / tau + q @ x1 + b @ z1 + 2 * (xi @ (Pfull @ x1))
            xm = xi - x2
            tden = kappa / tau - q @ x2 - b @ z2 + xm @ (Pfull @ xm) - x2 @ (Pfull @ x2)
            dtau = tnum / tden
            dx = x1 + dtau * x2
            dz = z1 + dtau * z2
            ds = -(each(lambda c, v: c.mul_Hs(v), dz) + const)
            dkappa = -(rhs_kappa + kappa * dtau) / tau
            return True, (dx, dz, ds, dtau, dkappa)

        def step_length(dz, ds, dtau, dkappa, combined):                                   # variables.jl:13-45
            at = -tau / dtau if dtau < 0 else np.finfo(float).max
            ak = -kappa / dkappa if dkappa < 0 else np.finfo(float).max
            a = min(at, ak, 1.0)
            if not nonsym:
                for c in cones:
                    a = min(a, c.step_length(dz[c.rng], ds[c.rng], z[c.rng], s[c.rng], a))
                return a * st.max_step_fraction if combined else a
            # coneops_compositecone.jl:205-243: symmetric cones first, then back off from the full step so that the
            # logarithms of the non-symmetric cones do not fail right at the boundary, then those cones
            for c in cones:
                if not isinstance(c, _NonSym):
                    a = min(a, c.step_length(dz[c.rng], ds[c.rng], z[c.rng], s[c.rng], a))
            a = min(a, 1.0 - np.sqrt(_EPS))
            for c in cones:
                if isinstance(c, _NonSym):
                    a = min(a, c.step_length(dz[c.rng], ds[c.rng], z[c.rng], s[c.rng], a, st))
            if not combined:
                return a
            a *= st.max_step_fraction
            if strategy == DUAL:                       # solver_backtrack_step_to_barrier, solver.jl:407-442
                for _ in range(50):
                    if barrier(dz, ds, dtau, dkappa, a) < 1.0:
                        break
                    a *= st.linesearch_backtrack_step
            return a

        def barrier(dz, ds, dtau, dkappa, a):                                              # variables.jl:46-72
            ct, ck = tau + a * dtau, kappa + a * dkappa
            mu_a = ((z + a * dz) @ (s + a * ds) + ct * ck) / (degree + 1)
            out = (degree + 1) * _logsafe(mu_a) - _logsafe(ct) - _logsafe(ck)
            for c in cones:
                out += c.compute_barrier(z[c.rng], s[c.rng], dz[c.rng], ds[c.rng], a)
            return out

        step = None
        if ok:
            aff_s = each(lambda c, v: c.affine_ds(v), s)
            if aff_step is not None:
                step = aff_step
            else:
                ok, step = kkt_solve(rx, rz, aff_s, rtau, tau * kappa, True)
        if ok:
            dx, dz, ds, dtau, dkappa = step
            alpha = step_length(dz, ds, dtau, dkappa, False)
            sigma = (1 - alpha) ** 3
            mcorr = 1.0 if it > 1 else alpha
            shift = each(lambda c, a_, b_: c.combined_ds_shift(a_, b_, sigma * mu), dz * mcorr, ds)
            rhs_s = aff_s + shift
            ok, step = kkt_solve((1 - sigma) * rx, (1 - sigma) * rz, rhs_s, (1 - sigma) * rtau,
                                 -sigma * mu + mcorr * dtau * dkappa + tau * kappa, False)
        if not ok:
            alpha = 0.0
            if nonsym and strategy == PRIMAL_DUAL:     # _strategy_checkpoint_numerical_error
                strategy = DUAL
                continue
            status = NUMERICAL_ERROR
            break
        dx, dz, ds, dtau, dkappa = step
        alpha = step_length(dz, ds, dtau, dkappa, True)
        if nonsym and strategy == PRIMAL_DUAL and alpha < st.min_switch_step_length:
            strategy, alpha = DUAL, 0.0                # _strategy_checkpoint_small_step
            continue
        if alpha <= max(0.0, st.min_terminate_step_length):
            status = INSUFFICIENT_PROGRESS
            alpha = 0.0
            break
        prev = dict(res_p=res_p, res_d=res_d, gap_abs=gap_abs, gap_rel=gap_rel)
        prev_vars = (x.copy(), s.copy(), z.copy(), tau, kappa)
        x = x + alpha * dx
        s = s + alpha * ds
        z = z + alpha * dz
        tau += alpha * dtau
        kappa += alpha * dkappa

    # ---- info_post_process! (info.jl:196-211): after an error / limit exit, accept an iterate that
    #      meets the reduced tolerances as ALMOST_SOLVED
    if status in (NUMERICAL_ERROR, INSUFFICIENT_PROGRESS, MAX_ITERATIONS):
        tinv = 1.0 / tau
        Px = Pfull @ x
        xPx = x @ Px
        cp = (q @ x) * tinv + xPx * tinv * tinv / 2
        cd = -(b @ z) * tinv - xPx * tinv * tinv / 2
        nx, nz, ns = np.linalg.norm(x) * tinv, np.linalg.norm(z) * tinv, np.linalg.norm(s) * tinv
        rp = np.linalg.norm(A @ x + s - b * tau) * tinv / max(1.0, normb + nx + ns)
        rd = np.linalg.norm(-(At @ z) - Px - q * tau) * tinv / max(1.0, normq + nx + nz)
        ga = abs(cp - cd)
        gr = ga / max(1.0, min(abs(cp), abs(cd)))
        if kappa * tinv <= 1 and (ga < st.reduced_tol_gap_abs or gr < st.reduced_tol_gap_rel) and \
                rp < st.reduced_tol_feas and rd < st.reduced_tol_feas:
            status = ALMOST_SOLVED
    # ---- solution_post_process!: unscale by tau (kappa for certificates)
    infeasible = status in (PRIMAL_INFEASIBLE, DUAL_INFEASIBLE)
    sc = 1.0 / (kappa if infeasible else tau)
    xo, zo, so = x * sc, z * sc, s * sc
    objp = q @ xo + 0.5 * xo @ (Pfull @ xo)
    objd = -b @ zo - 0.5 * xo @ (Pfull @ xo)
    if infeasible:
        objp = objd = float("nan")
    return IPMResult(status, xo, zo, so, objp, objd, it, ir_total, hist)


# ------------------------------------------------------------------------------------------
#  backends
# ------------------------------------------------------------------------------------------
class HipBackend:
    """The MI355X path: libhipkkt.so through HipKKTSolver (level B of the C ABI)."""

    def __init__(self, P, A, cone_specs, settings=None, large_psd=False):
        from .kktsolver import HipKKTSolver
        self.ks = HipKKTSolver(P, A, cone_specs, settings=settings, large_psd=large_psd)
        self.specs = list(cone_specs)

    def update_identity(self):
        return self.ks.kktsolver_update(*identity_scaling_data(self.specs))

    def update(self, s, z, mu=None, strategy=None):
        if strategy is not None:                       # only a problem with a non-symmetric cone passes these
            self.ks.set_nonsymmetric_scaling(strategy, mu)
        return self.ks.kktsolver_update_from_sz(s, z)

    def kktsolver_setrhs(self, rx, rz):
        self.ks.kktsolver_setrhs(rx, rz)

    def kktsolver_solve(self, x, z):
        return self.ks.kktsolver_solve(x, z)

    @property
    def last_ir_iterations(self):
        return self.ks.last_ir_iterations


class HipSystemBackend(HipBackend):
    """As HipBackend, but the reduced-system layer (kktsystem.jl) runs on the device too (level C of the
    C ABI): the driver hands over iterates and right-hand sides and gets the step back."""

    def __init__(self, P, A, cone_specs, settings=None, batch_affine=False, lazy=False, host_cones=False, staging="host",
                 large_psd=False):
        super().__init__(P, A, cone_specs, settings=settings, large_psd=large_psd)
        from .kktsolver import HipKKTSystem
        self.system = HipKKTSystem(self.ks)
        self.system.staging = staging              # "host": the *_host entry points; "torch": device tensors + *_dev
        self.batch_affine = batch_affine           # kkt_update! + affine kkt_solve! as one 2-column solve, ONE call
        self.host_cones = host_cones               # kkt_update! from the driver's own cone objects (the Julia glue's route)
        if lazy:
            # the same pairing through the reference's TWO calls (solver.jl:278-295 untouched): kkt_update! leaves the
            # constant-RHS solve to the affine kkt_solve!, which sends both right-hand sides through the sweeps together
            self.system.set_lazy(True)
