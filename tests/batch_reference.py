"""References for the _batch entry points of level C (tests/test_gpu_batch_ops.py): a stack of independent member problems,
and the cut that takes ONE member's view out of it, so that the references the scalar entry points are held to
(tests/iterate_reference.py, tests/step_reference.py, tests/system_reference.py) apply to that member unchanged.  Nothing
here restates a kernel: the bounds are those modules' own.

Simulated faults (`restate_member`, `faulty_step`) show that those bounds bite on a batch: member b's scalars taken over
member b + 1's rows, and the joint tau used for every member."""
import numpy as np
import scipy.sparse as sp

from tests import iterate_reference as I
from tests import step_reference as sr
from tests import system_reference as S


class Stack:
    """members: problems with P (triu), A, cones, q, b (tests/system_reference.Problem or tests/iterate_reference.Problem)"""

    def __init__(self, name, members):
        self.name, self.members, self.nb = name, list(members), len(members)
        self.blocks = [(pb.n, pb.m) for pb in self.members]
        self.x_off = np.concatenate([[0], np.cumsum([b[0] for b in self.blocks])]).astype(int)
        self.z_off = np.concatenate([[0], np.cumsum([b[1] for b in self.blocks])]).astype(int)
        self.c_off = np.concatenate([[0], np.cumsum([len(pb.cones) for pb in self.members])]).astype(int)
        self.n, self.m = int(self.x_off[-1]), int(self.z_off[-1])
        self.P = sp.triu(sp.block_diag([pb.P for pb in self.members], format="csc"), format="csc")
        self.A = sp.csc_matrix(sp.block_diag([pb.A for pb in self.members], format="csc"))
        self.P.sort_indices()
        self.A.sort_indices()
        self.q = np.concatenate([pb.q for pb in self.members])
        self.b = np.concatenate([pb.b for pb in self.members])
        self.cones = [c for pb in self.members for c in pb.cones]

    def xr(self, b):
        return slice(self.x_off[b], self.x_off[b + 1])

    def zr(self, b):
        return slice(self.z_off[b], self.z_off[b + 1])

    def cat_x(self, parts):
        return np.concatenate([np.asarray(p, float) for p in parts]) if self.nb else np.zeros(0)

    cat_z = cat_x

    def handle(self, update=None):
        """(ks, system) of the stack with the partition set; update = (s, z): scaled and factorised there"""
        from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
        ks = HipKKTSolver(self.P, self.A, self.cones)
        system = HipKKTSystem(ks)
        system.staging = "torch"
        system.init(self.q, self.b)
        system.set_problems(self.blocks)
        if update is not None:
            assert system.update(*update)
        return ks, system


def alone(pb, update=None):
    """(ks, system) of a handle that holds this member alone"""
    from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
    ks = HipKKTSolver(pb.P, pb.A, pb.cones)
    system = HipKKTSystem(ks)
    system.staging = "torch"
    system.init(pb.q, pb.b)
    if update is not None:
        assert system.update(*update)
    return ks, system


TINY_CONES = ((), (("z", 1),), (("nn", 2),), (("soc", 2),), (("soc", 3),), (("psd", 1),), (("psd", 2),),
              (("nn", 1), ("soc", 3), ("psd", 2)), (("z", 2), ("nn", 3)), (("soc", 2), ("soc", 3), ("nn", 5)))
_TINY = {}


def tiny(k):
    """member k of the many-member stacks: one to four x rows, a cone list from TINY_CONES (every tenth member has m = 0, the
    next one a zero cone only)"""
    if k not in _TINY:
        rng = np.random.default_rng(9100 + k)
        cones = S._cones(*TINY_CONES[k % len(TINY_CONES)])
        m, nzero = sum(c.numel for c in cones), sum(c.numel for c in cones if c.kind == 0)
        n = max(1 + (k * 7) % 4, nzero + 1)               # (more equality rows than variables would make K singular)
        _TINY[k] = S.Problem(f"tiny{k}", S._tridiag(rng, n), S._make_A(rng, m, n, 2), cones, 9500 + k)
    return _TINY[k]


_STACKS = {}
SYSTEM_STACKS = {            # members of tests/system_reference.py: interior iterates, every cone operation and the solves
    "one": ("mixed",),
    "two": ("psd", "n32"),
    "three": ("n33", "m0", "mixed"),
    "three_b": ("lp33", "soc5", "n255"),
}
ITERATE_STACKS = {           # members of tests/iterate_reference.py: the residual pass, long rows across member boundaries
    "it_two": ("edges", "dense_row_4097"),
    "it_three": ("n1m1", "dense_col_4097", "dense_row_4096"),
}
MANY = {"many65": 65, "many257": 257}


def stack(name):
    if name not in _STACKS:
        if name in SYSTEM_STACKS:
            members = [S.problem(k) for k in SYSTEM_STACKS[name]]
        elif name in ITERATE_STACKS:
            members = [I.problem(k) for k in ITERATE_STACKS[name]]
        else:
            members = [tiny(k) for k in range(MANY[name])]
        _STACKS[name] = Stack(name, members)
    return _STACKS[name]


def spread(nb, lo, hi, seed):
    """nb values spread over the decades lo .. hi, in shuffled order"""
    v = 10.0 ** np.linspace(lo, hi, nb) if nb > 1 else np.array([10.0 ** lo])
    return np.random.default_rng(seed).permutation(v)


# --------------------------------------------------------------------------------------------- the residual pass
def member_parts(pb):
    if not hasattr(pb, "parts"):
        pb.parts = I.Parts(pb.P, pb.A)
    return pb.parts


def residual_data(st, seed=31):
    """x, s, z of the stack (a member of iterate_reference keeps its own) and tau per member over 1e-6 .. 1e3"""
    rng = np.random.default_rng(seed)
    xs, ss, zs = [], [], []
    for pb in st.members:
        if hasattr(pb, "x"):
            xs.append(pb.x); ss.append(pb.s); zs.append(pb.z)
        else:
            xs.append(rng.standard_normal(pb.n)); ss.append(rng.standard_normal(pb.m)); zs.append(rng.standard_normal(pb.m))
    return st.cat_x(xs), st.cat_z(ss), st.cat_z(zs), spread(st.nb, -6, 3, seed + 1)


def member_data(st, b, x, s, z, tau):
    pb = st.members[b]
    return dict(q=pb.q, b=pb.b, x=x[st.xr(b)], s=s[st.zr(b)], z=z[st.zr(b)], tau=float(tau[b]))


def cut_vectors(st, b, vec):
    return {k: (v[st.xr(b)] if k in ("Px", "rx_inf", "rx") else v[st.zr(b)]) for k, v in vec.items()}


def joint_tau(taus):
    """the one tau a loop without per-member scalars would hold: of the members' order of magnitude, and none of theirs
    (three times the geometric mean)"""
    return 3.0 * float(np.exp(np.mean(np.log(np.asarray(taus, float)))))


def restate_member(st, b, x, s, z, tau, fault=None):
    """(vectors, 12 scalars) of member b in plain numpy, as iterate_reference.restate forms them.  fault "neighbour_rows":
    the scalars are taken over member b + 1's rows; "joint_tau": every member's rx, rz use one tau (`joint_tau`)."""
    t = np.array(tau, float)
    if fault == "joint_tau":
        t[:] = joint_tau(t)
    d = member_data(st, b, x, s, z, t)
    vec, scal = I.restate(member_parts(st.members[b]), **d)
    if fault == "neighbour_rows":
        nb_ = (b + 1) % st.nb
        _, scal = I.restate(member_parts(st.members[nb_]), **member_data(st, nb_, x, s, z, t))
    return vec, scal


def residual_ratios(st, b, x, s, z, tau, vec_b, scal_b):
    """iterate_reference's ratios of member b: the twelve scalars against exact values formed from the member's vectors, and
    the five vectors against the member's exact residuals"""
    d = member_data(st, b, x, s, z, tau)
    out = I.scalar_ratios(d, vec_b, scal_b)
    out.update({"v_" + k: v for k, v in I.vector_ratios(member_parts(st.members[b]), d, vec_b).items()})
    return out


# --------------------------------------------------------------------------------------------- interior iterates, steps
def interior(st, seed=41):
    """an interior iterate per member (system_reference.iterate, unit scale) -> list of Iterate, with tau and kappa that
    differ strongly between the members"""
    taus, kappas = spread(st.nb, -2, 1, seed), spread(st.nb, -2, 0, seed + 1)
    its = []
    for b, pb in enumerate(st.members):
        it = S.iterate(pb, "unit", S.ITERATE_SEED + 100 * b + seed)
        it.tau, it.kappa = float(taus[b]), float(kappas[b])
        its.append(it)
    return its


def rhs_of(st, its, seed=43):
    rng = np.random.default_rng(seed)
    out = []
    for b, (pb, it) in enumerate(zip(st.members, its)):
        r = S.rhs_for(pb, it, S.RHS_SEED + b)
        r.tau, r.kappa = float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1))
        out.append(r)
    return out


def seeded_steps(st, its, seed=47):
    """(dz, ds) of the stack: steps of the iterates' own size, a third of them pointing out of the cones"""
    rng = np.random.default_rng(seed)
    dz = st.cat_z([np.abs(it.z).max(initial=1.0) * rng.standard_normal(pb.m) for pb, it in zip(st.members, its)])
    ds = st.cat_z([np.abs(it.s).max(initial=1.0) * rng.standard_normal(pb.m) for pb, it in zip(st.members, its)])
    return dz, ds


def member_scaling(st, b, ks):
    lam, psd = ks.scaling()
    w, eta = ks.scaling_w()
    npsd_before = sum(1 for c in st.cones[:st.c_off[b]] if c.kind == 3)
    npsd = sum(1 for c in st.members[b].cones if c.kind == 3)
    return sr.Scaling(st.members[b].cones, w[st.zr(b)], eta[st.c_off[b]:st.c_off[b + 1]], lam[st.zr(b)],
                      psd[npsd_before:npsd_before + npsd])


def member_view(st, b, ks):
    """system_reference.View of member b cut out of the stack's handle: its rows and columns of K (with the expansion
    columns of its own sparse second-order cones), its part of the scaling, and a solve that embeds the member's
    right-hand side into the stack (K is block diagonal, so the other members' rows stay zero)"""
    Kt = sp.csc_matrix(ks.KKT())
    full = sp.csr_matrix(Kt + sp.triu(Kt, 1).T)
    nm = st.n + st.m
    idx = np.concatenate([np.arange(st.x_off[b], st.x_off[b + 1]), st.n + np.arange(st.z_off[b], st.z_off[b + 1])])
    ext = nm + np.flatnonzero(np.diff(sp.csc_matrix(full[idx, :][:, nm:]).indptr))
    sel = np.concatenate([idx, ext]).astype(int)
    Kb = sp.triu(full[sel, :][:, sel], format="csc")
    pb = st.members[b]

    def solve(rx, rz):
        RX, RZ = np.zeros(st.n), np.zeros(st.m)
        RX[st.xr(b)], RZ[st.zr(b)] = rx, rz
        ks.kktsolver_setrhs(RX, RZ)
        X, Z = np.zeros(st.n), np.zeros(st.m)
        assert ks.kktsolver_solve(X, Z)
        return X[st.xr(b)].copy(), Z[st.zr(b)].copy()
    return S.View(pb, Kb, member_scaling(st, b, ks), ks.settings.iterative_refinement_abstol,
                  ks.settings.iterative_refinement_reltol, solve)


def faulty_step(st, b, views, its, rhss, affine, fault):
    """kkt_solve! of member b restated in numpy (system_reference.restate_step) with a batch fault: None -- none;
    "joint_tau" -- the member's step formed with the geometric mean of all members' tau; "neighbour_rows" -- (dtau,
    dkappa) come from member b + 1's rows (its dot products), beside member b's own vectors.  views: member -> View."""
    import copy
    it = copy.copy(its[b])
    if fault == "joint_tau":
        it.tau = joint_tau([i.tau for i in its])
    dx, dz, ds, dtau, dkappa = S.restate_step(views[b], it, rhss[b], affine)
    if fault == "neighbour_rows":
        nb_ = (b + 1) % st.nb
        _, _, _, dtau, dkappa = S.restate_step(views[nb_], its[nb_], rhss[nb_], affine)
    return dx, dz, ds, dtau, dkappa
