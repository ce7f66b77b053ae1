"""Independent checks for the exponential and the power cone, and a CPU backend for problems that hold them.

The extended-precision oracle differentiates the two dual barriers AS WRITTEN (coneops_expcone.jl:216-219,
coneops_powcone.jl:220-223) with mpmath; the conjugate (primal) gradient g(s) is the root of grad f*(-g) = -s.
None of the closed forms under test is used."""
import numpy as np
import scipy.sparse as sp
import mpmath as mp

from cuclarabel_amd import ipm
from cuclarabel_amd.cones import ExponentialConeT, PowerConeT, SecondOrderConeT
from tests.oracle_bindings import OracleKKT

mp.mp.dps = 60


# ------------------------------------------------------------------------------------------
#  mpmath oracle
# ------------------------------------------------------------------------------------------
def dual_barrier(spec):
    if isinstance(spec, ExponentialConeT):
        return lambda z1, z2, z3: -mp.log(z2 - z1 - z1 * mp.log(z3 / -z1)) - mp.log(-z1) - mp.log(z3)
    a = mp.mpf(spec.alpha)
    return lambda z1, z2, z3: (-mp.log((z1 / a) ** (2 * a) * (z2 / (1 - a)) ** (2 - 2 * a) - z3 * z3)
                               - (1 - a) * mp.log(z1) - a * mp.log(z2))


def mp_grad(f, z):
    z = [mp.mpf(float(v)) for v in z]
    return mp.matrix([mp.diff(f, z, tuple(1 if i == k else 0 for i in range(3))) for k in range(3)])


def mp_hess(f, z):
    z = [mp.mpf(float(v)) for v in z]
    H = mp.zeros(3, 3)
    for i in range(3):
        for j in range(3):
            order = [0, 0, 0]
            order[i] += 1
            order[j] += 1
            H[i, j] = mp.diff(f, z, tuple(order))
    return H


def mp_primal_gradient(spec, s, g0):
    """g with grad f*(-g) = -s, started from the float64 guess g0 (only a starting point: findroot converges to
    60 digits or raises)."""
    f = dual_barrier(spec)
    s = [mp.mpf(float(v)) for v in s]

    def F(g1, g2, g3):
        gr = [mp.diff(f, (-g1, -g2, -g3), tuple(1 if i == k else 0 for i in range(3))) for k in range(3)]
        return [gr[0] + s[0], gr[1] + s[1], gr[2] + s[2]]

    return mp.findroot(F, [mp.mpf(float(v)) for v in g0], tol=mp.mpf(10) ** -40, maxsteps=50)


def mp_point(spec, s, z):
    """(grad f*(z), H*(z), g(s)) in extended precision: everything the two strategies need at one point."""
    f = dual_barrier(spec)
    st, H = mp_grad(f, z), mp_hess(f, z)
    c = ipm._make_cones([spec])[0]
    with np.errstate(all="ignore"):
        g0 = c.gradient_primal(np.asarray(s, float))
    return st, H, mp_primal_gradient(spec, s, g0)


def mp_scaling(spec, s, z, mu, strategy, point=None):
    """(grad, H_dual, Hs, used_primal_dual, guards) in extended precision, following the DEFINITION of the
    primal-dual scaling (coneops_nonsymmetric_common.jl:82-164) with the oracle's gradients."""
    st, H, zt = point if point is not None else mp_point(spec, s, z)
    sm, zm = mp.matrix([float(v) for v in s]), mp.matrix([float(v) for v in z])
    if strategy == ipm.DUAL:
        return st, H, mp.mpf(float(mu)) * H, False, None
    dot_sz = (zm.T * sm)[0]
    mul = dot_sz / 3
    mut = (zt.T * st)[0] / 3
    dls, dlz = sm + mul * st, zm + mul * zt
    dot_dsz = (dls.T * dlz)[0]
    de1 = mul * mut - 1
    de2 = (zt.T * H * zt)[0] - 3 * mut * mut
    guards = (de1, de2, dot_sz, dot_dsz)
    eps = np.finfo(float).eps
    if abs(de1) > np.sqrt(eps) and abs(de2) > eps and dot_sz > 0 and dot_dsz > 0:
        tmp = mut * st - H * zt
        W = H - st * st.T / 3 - tmp * tmp.T / de2
        t = mul * mp.sqrt(sum(W[i, j] ** 2 for i in range(3) for j in range(3)))
        ax = mp.matrix([zm[1] * zt[2] - zm[2] * zt[1], zm[2] * zt[0] - zm[0] * zt[2], zm[0] * zt[1] - zm[1] * zt[0]])
        ax = ax / mp.sqrt((ax.T * ax)[0])
        Hs = sm * sm.T / dot_sz + dls * dls.T / dot_dsz + t * ax * ax.T
        return st, H, Hs, True, guards
    return st, H, mul * H, False, guards


def guard_margin(guards):
    """How far the float64 guards (de1, de2, <s,z>, <ds,dz>) of a point are from their thresholds, as a factor:
    min over the four of value / threshold (the two sign tests count as far when positive).  > 1: primal-dual branch."""
    de1, de2, dot_sz, dot_dsz = [float(g) for g in guards]
    eps = np.finfo(float).eps
    if not (dot_sz > 0 and dot_dsz > 0):
        return 0.0
    return min(abs(de1) / np.sqrt(eps), abs(de2) / eps)


def to_np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)]).squeeze()


def rel_err(a, M):
    """max |a - M| / max |M| of a float64 array against an mpmath matrix, the subtraction in extended precision"""
    a = np.atleast_2d(np.asarray(a, float))
    if M.cols == 1 and a.shape[0] == 1:
        a = a.T
    num = max(abs(mp.mpf(float(a[i, j])) - M[i, j]) for i in range(M.rows) for j in range(M.cols))
    den = max(abs(M[i, j]) for i in range(M.rows) for j in range(M.cols))
    return float(num / den)


# ------------------------------------------------------------------------------------------
#  random interior points
# ------------------------------------------------------------------------------------------
def random_interior_pair(spec, rng, spread=1.0):
    """(s, z) with s strictly inside the primal cone and z strictly inside the dual one."""
    if isinstance(spec, ExponentialConeT):
        s2, s3 = np.exp(spread * rng.normal(size=2))
        s1 = s2 * np.log(s3 / s2) - np.exp(spread * rng.normal())           # s2 log(s3/s2) - s1 > 0
        z1 = -np.exp(spread * rng.normal())
        z3 = np.exp(spread * rng.normal())
        z2 = z1 + z1 * np.log(-z3 / z1) + np.exp(spread * rng.normal())     # z2 - z1 - z1 log(-z3/z1) > 0
        return np.array([s1, s2, s3]), np.array([z1, z2, z3])
    a = spec.alpha
    s1, s2, z1, z2 = np.exp(spread * rng.normal(size=4))
    s3 = rng.uniform(-0.95, 0.95) * s1 ** a * s2 ** (1 - a)
    z3 = rng.uniform(-0.95, 0.95) * (z1 / a) ** a * (z2 / (1 - a)) ** (1 - a)
    return np.array([s1, s2, s3]), np.array([z1, z2, z3])


def central_pair(spec, rng, spread=1.0):
    """(s, z) on the central path: z random interior, s = -mu grad f*(z), where de1 of the primal-dual scaling vanishes."""
    _, z = random_interior_pair(spec, rng, spread)
    c = ipm._make_cones([spec])[0]
    g, _ = c.dual_grad_H(z)
    return -np.exp(rng.normal()) * g, z


POW_ALPHAS = (0.1, 0.5, 0.6, 0.9)


def scaling_points(kind, seed, nrandom, ncentral):
    """[(spec, s, z)] for one cone kind ("exp" or "pow"): random interior pairs, then central-path pairs; the power
    cone cycles through POW_ALPHAS."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(nrandom + ncentral):
        spec = ExponentialConeT() if kind == "exp" else PowerConeT(POW_ALPHAS[j % len(POW_ALPHAS)])
        s, z = random_interior_pair(spec, rng) if j < nrandom else central_pair(spec, rng)
        out.append((spec, s, z))
    return out


def fixture_points(fixture):
    """Every (spec, s, z, mu, strategy) at which the CPU run of a fixture scaled a non-symmetric cone."""
    P, q, A, b, cones, _ = fixture()
    be = OracleNonsymBackend(P, A, cones)
    ipm.solve(P, q, A, b, cones, be)
    out = []
    for s, z, mu, strategy in be.points:
        for c in be.cones:
            if isinstance(c, ipm._NonSym):
                out.append((c.spec, s[c.rng].copy(), z[c.rng].copy(), mu, strategy))
    return out


# ------------------------------------------------------------------------------------------
#  CPU backend: the oracle's KKT path with each EXP / POW cone declared as SOC(3) (the same dense 3x3
#  structure) and the values handed over from the driver's own cone objects
# ------------------------------------------------------------------------------------------
def soc3_twin(specs):
    return [SecondOrderConeT(3) if isinstance(c, (ExponentialConeT, PowerConeT)) else c for c in specs]


class OracleNonsymBackend:
    def __init__(self, P, A, cone_specs):
        self.specs = list(cone_specs)
        self.o = OracleKKT(P, A, soc3_twin(self.specs))
        self.cones = ipm._make_cones(self.specs)
        self.points = []                                  # every (s, z, mu, strategy) the driver scaled at

    def update_identity(self):
        raise AssertionError("a problem with a non-symmetric cone never asks for the identity scaling")

    def update(self, s, z, mu, strategy):
        self.points.append((s.copy(), z.copy(), mu, strategy))
        for c in self.cones:
            args = (mu, strategy) if isinstance(c, ipm._NonSym) else ()
            if not c.update_scaling(s[c.rng].copy(), z[c.rng].copy(), *args):
                return False
        Hs, u, v, e2 = ipm.host_cone_data(self.cones)[:4]
        return self.o.kktsolver_update_values(Hs, u, v, e2)

    def kktsolver_setrhs(self, rx, rz):
        self.o.kktsolver_setrhs(rx, rz)

    def kktsolver_solve(self, x, z):
        ok, xo, zo = self.o.kktsolver_solve(x is not None, z is not None)
        if x is not None:
            x[:] = xo
        if z is not None:
            z[:] = zo
        return ok

    @property
    def last_ir_iterations(self):
        return self.o.last_ir_iters


def mixed_six(seed=41):
    """A problem with all six cone kinds: problems.small_mixed (zero, nonnegative, dense and sparse second-order, PSD)
    plus two exponential and three power cones on random rows; (s0, z0) strictly interior."""
    from cuclarabel_amd import problems
    pb = problems.small_mixed(seed=seed, psds=(2, 3, 6), socs=(3, 4, 6, 15))
    rng = np.random.default_rng(seed + 1000)
    extra = [ExponentialConeT(), PowerConeT(0.6), ExponentialConeT(), PowerConeT(0.1), PowerConeT(0.9)]
    pairs = [random_interior_pair(c, rng) for c in extra]
    Ax = sp.random(3 * len(extra), pb.n, density=0.3, random_state=rng.integers(1 << 30), format="csc",
                   data_rvs=rng.standard_normal)
    A = sp.vstack([pb.A, Ax]).tocsc()
    A.sort_indices()
    return problems.Problem("mixed_six", pb.P, pb.q, A, np.concatenate([pb.b, rng.standard_normal(3 * len(extra))]),
                            list(pb.cones) + extra, np.concatenate([pb.s0] + [p[0] for p in pairs]),
                            np.concatenate([pb.z0] + [p[1] for p in pairs]), pb.x0)
