"""Host model of the per-member static regulariser and failure words (hipkkt_kkt_system_set_member_status) -- TEST
INFRASTRUCTURE ONLY, shared by tests/test_member_status_reference_host.py (which checks the model against an independent
truth on the CPU, on the image the C oracle assembles, and shows that every seeded fault is caught) and tests/
test_gpu_member_status.py (which compares the device with the model on the image the device holds).

The model, per member b of a block-diagonal stack:
  rows_b    its rows of K's image: x rows, z rows, the two expansion rows of each of its sparse second-order cones
  eps_b     c0 + c1 * max |K_ii| over rows_b, in numpy's two roundings (kktsolver_directldl.jl:297-310 on the member)
  solve     (K_b + eps_b S_b)^-1 rhs_b dense, S_b = diag(dsigns on rows_b) (kktsolver_directldl.jl:283-291)
  words     (cone word, pivot word) per member, predicted from where a non-interior cone or a NaN was put

FAULTS are simulated defects of such an implementation; the host test shows that each is caught by at least one case:
  joint_eps           every member receives the stack's epsilon
  neighbour_max       member b's maximum is taken over member b + 1's rows
  no_expansion_rows   a member's rows stop at n + m
  next_member         a failure is attributed to the member behind the one it happened in

The truth the model is checked against does not use the partition at all: K is block diagonal, so the members are the
connected components of the image's graph (every member here is connected: A_b is dense), and a regularised solve of
the whole stack with each row's component's epsilon is what the members' own solves must add up to.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from tests import member_refinement_cases as mc

C0, C1 = 1e-8, 1e-3
FAULTS = ("joint_eps", "neighbour_max", "no_expansion_rows", "next_member")
ULP = 2.0 ** -52


def settings(refine=False):
    """Large proportional part, so that the members' epsilons differ by orders of magnitude; dynamic regularisation at
    its default 1e-13, far below every pivot of the cases."""
    return dict(static_regularization_enable=1, static_regularization_constant=C0, static_regularization_proportional=C1,
                iterative_refinement_enable=1 if refine else 0)


def oracle_settings():
    return dict(static_reg_constant=C0, static_reg_proportional=C1)


# ------------------------------------------------------------------------------------------------ the model
def member_rows(st, fault=None):
    rows, N = mc.member_rows(st)
    if fault == "no_expansion_rows":
        rows = [r[r < st.n + st.m] for r in rows]
    return rows, N


def member_eps(diag, rows, fault=None):
    """eps_b = c0 + c1 * max_b; a NaN diagonal entry does not count (fmax drops it)."""
    a = np.abs(np.asarray(diag, float))
    a = np.where(np.isnan(a), 0.0, a)
    nb = len(rows)
    if fault == "joint_eps":
        return np.full(nb, C0 + C1 * a.max())
    pick = [(b + 1) % nb if fault == "neighbour_max" else b for b in range(nb)]
    return np.array([C0 + C1 * a[rows[k]].max() for k in pick])


def member_solve(K, dsigns, rows, eps, rhs):
    """stack vector over the image: member b's rows hold (K_b + eps_b S_b)^-1 rhs_b; also the blocks' condition numbers"""
    out, cond = np.zeros(K.shape[0]), []
    Kc = sp.csr_matrix(K)
    for b, r in enumerate(rows):
        Kb = Kc[r][:, r].toarray() + np.diag(eps[b] * dsigns[r])
        out[r] = np.linalg.solve(Kb, rhs[r])
        cond.append(np.linalg.cond(Kb))
    return out, np.array(cond)


def solve_tolerance(cond):
    return 100.0 * cond * ULP


def member_words(st, poison, fault=None):
    """poison: list of (kind, z row) with kind in {"soc", "psd"} (a cone that is not interior: the cone word of the row's
    member) or "nn" (a negative z on a nonnegative row: NaN in Hs, the pivot word) -> (nb, 2) array of 0 / 1."""
    z_off = np.concatenate([[0], np.cumsum([bl[1] for bl in st.blocks])])
    W = np.zeros((st.nb, 2))
    for kind, row in poison:
        b = int(np.searchsorted(z_off, row, side="right") - 1)
        if fault == "next_member":
            b = (b + 1) % st.nb
        W[b, 0 if kind in ("soc", "psd") else 1] = 1.0
    return W


# ------------------------------------------------------------------------------------------------ the truth
def components(K):
    """row of the image -> component label, labels numbered by first row (= member order: the x rows come first)"""
    G = sp.csr_matrix(K).copy()
    G.data = np.ones_like(G.data)                            # (explicit zeros and NaN values are edges too)
    _, lab = connected_components(G, directed=False)
    first = {}
    for i, l in enumerate(lab):
        first.setdefault(l, len(first))
    return np.array([first[l] for l in lab])


def truth_eps(K):
    lab = components(K)
    a = np.abs(sp.csr_matrix(K).diagonal())
    return np.array([C0 + C1 * a[lab == c].max() for c in range(lab.max() + 1)]), lab


def truth_solve(K, dsigns, rhs):
    eps, lab = truth_eps(K)
    Kreg = sp.csr_matrix(K).toarray() + np.diag(eps[lab] * dsigns)
    return np.linalg.solve(Kreg, rhs)


# ------------------------------------------------------------------------------------------------ the cases
def _psd(k):
    from cuclarabel_amd.cones import PSDTriangleConeT
    return PSDTriangleConeT(k)


def _set_hs(st, b, local_z_row, ratio):
    """s / z = ratio on one nonnegative row of member b: its -Hs entry of K's diagonal becomes -ratio"""
    z_off = np.concatenate([[0], np.cumsum([bl[1] for bl in st.blocks])])
    i = z_off[b] + (local_z_row if local_z_row >= 0 else st.blocks[b][1] + local_z_row)
    st.s[i], st.z[i] = ratio, 1.0


def _set_p(st, b, local_x_row, value):
    x_off = np.concatenate([[0], np.cumsum([bl[0] for bl in st.blocks])])
    P = sp.lil_matrix(st.P)
    P[x_off[b] + local_x_row, x_off[b] + local_x_row] = value
    st.P = sp.triu(sp.csc_matrix(P), format="csc")


def _scale_soc(st, b, factor):
    """s of member b's second-order cone times factor: eta^2 = sscale / zscale grows by it, on the cone's rows of Hs and
    on its two expansion rows (-eta^2, +eta^2)"""
    from cuclarabel_amd.cones import SecondOrderConeT
    off, zb = 0, np.concatenate([[0], np.cumsum([bl[1] for bl in st.blocks])])
    for c in st.cones:
        if isinstance(c, SecondOrderConeT) and zb[b] <= off < zb[b + 1]:
            st.s[off:off + c.numel] *= factor
        off += c.numel


def case_sizes():
    """members of 1, 255, 256 and 257 image rows and one with a second-order cone of dimension 5 (10 rows: 3 + 5 + 2).
    Maxima: member 1 at its LAST row (a negative -Hs entry), member 2 at its FIRST row (a P entry), member 3 in the
    middle, member 4 on its cone's rows and expansion rows (eta^2); the stack's maximum lies in member 1."""
    st = mc.make_stack("ms_sizes", [("healthy", 1, []), ("healthy", 100, [mc._nn(155)]), ("healthy", 100, [mc._nn(156)]),
                                    ("healthy", 100, [mc._nn(157)]), ("healthy", 3, [mc._soc(5)])], [1.0] * 5, seed=9301)
    _set_hs(st, 1, -1, 4.0e4)
    _set_p(st, 2, 0, 300.0)
    _set_hs(st, 3, 70, 25.0)
    _scale_soc(st, 4, 50.0)
    return st


def case_one():
    """nb = 1: the member's epsilon is the joint one"""
    st = mc.make_stack("ms_one", [("healthy", 4, [mc._nn(3), mc._soc(5)])], [1.0], seed=9302)
    _set_hs(st, 0, 1, 40.0)
    return st


def case_three():
    """nb = 3, blocks with condition number below 1e3 whose epsilons lie more than an order of magnitude apart: the case of the
    regularised solve.  Member 0's maximum on an expansion row / cone row (eta^2), member 1's on a negative -Hs entry,
    member 2's on a P entry; the stack's maximum in member 1."""
    st = mc.make_stack("ms_three", [("healthy", 4, [mc._nn(3), mc._soc(5)]), ("healthy", 3, [mc._zero(1), mc._nn(4)]),
                                    ("healthy", 5, [mc._soc(6), mc._nn(2)])], [1.0] * 3, seed=9303)
    _scale_soc(st, 0, 6.0)
    _set_hs(st, 1, -1, 60.0)
    _set_p(st, 2, 4, 3.0)
    return st


def case_many(nb=300):
    """nb = 300 (past one workgroup of members, and past 256 rows many times over): three-row members, every seventh with a
    sparse second-order cone; diagonal maxima cycle over five orders of magnitude"""
    members = [("healthy", 3, [mc._soc(5)]) if k % 7 == 3 else ("healthy", 1, [mc._nn(2)]) for k in range(nb)]
    st = mc.make_stack(f"ms_many{nb}", members, [1.0] * nb, seed=9304)
    for k in range(nb):
        if k % 7 == 3:
            _scale_soc(st, k, 10.0 ** (k % 4))
        else:
            _set_hs(st, k, k % 2, 10.0 ** (k % 6 - 1))
    return st


EPS_CASES = (case_sizes, case_one, case_three, case_many)


def attribution_stack(nb):
    """every member: 3 variables, a nonnegative cone of 3, a second-order cone of 5 and a PSD cone of side 2 (11 z rows).
    Returns (stack, {kind: local z row to poison})."""
    members = [("healthy", 3, [mc._nn(3), mc._soc(5), _psd(2)]) for _ in range(nb)]
    st = mc.make_stack(f"ms_attr{nb}", members, [1.0] * nb, seed=9310 + nb)
    rng = np.random.default_rng(9320 + nb)
    z_off = np.concatenate([[0], np.cumsum([bl[1] for bl in st.blocks])])
    for b in range(nb):                                       # the PSD rows: svec of a multiple of the identity (interior)
        for v in (st.s, st.z):
            v[z_off[b] + 8:z_off[b] + 11] = rng.uniform(0.8, 1.2) * np.array([1.0, 0.0, 1.0])
    return st, dict(nn=1, soc=3, psd=8)


def poisoned(st, where, kind, b):
    """(s, z, poison list) with member b's cone of that kind made non-interior: second-order z0 < ||z1|| (z0 = -1); a
    nonnegative z = -0.5 (Hs = s / z < 0 under the square root: NaN); a PSD z = svec([[1, 3], [3, 1]]), indefinite"""
    z_off = np.concatenate([[0], np.cumsum([bl[1] for bl in st.blocks])])
    s, z = st.s.copy(), st.z.copy()
    row = int(z_off[b] + where[kind])
    if kind == "soc":
        z[row] = -1.0
    elif kind == "nn":
        z[row] = -0.5
    else:
        z[row:row + 3] = [1.0, 3.0 * np.sqrt(2.0), 1.0]
    return s, z, [(kind, row)]


def member_problem(st, b):
    """member b alone: (P_b, A_b, cones_b, s_b, z_b)"""
    x_off = np.concatenate([[0], np.cumsum([bl[0] for bl in st.blocks])])
    z_off = np.concatenate([[0], np.cumsum([bl[1] for bl in st.blocks])])
    xs, zs = slice(x_off[b], x_off[b + 1]), slice(z_off[b], z_off[b + 1])
    cones, off = [], 0
    for c in st.cones:
        if z_off[b] <= off < z_off[b + 1]:
            cones.append(c)
        off += c.numel
    P = sp.triu(sp.csc_matrix(st.P + sp.triu(st.P, 1).T)[xs][:, xs], format="csc")
    return P, sp.csc_matrix(sp.csc_matrix(st.A)[zs][:, xs]), cones, st.s[zs], st.z[zs]


def oracle_image(st):
    """(K image, dsigns) of the stack at (s, z) from the C oracle on the CPU"""
    from tests import oracle_bindings as ob
    from tests import residual_reference as rr
    o = ob.OracleKKT(st.P, st.A, st.cones, settings=ob.default_settings(**oracle_settings()))
    if st.m:
        assert o.update_scaling(st.s, st.z)
    assert o.kktsolver_update()
    U_ = sp.csc_matrix(o.K())
    U_.sort_indices()
    return rr.sym_from_triu(U_.indptr, U_.indices, U_.data), np.array(o.dsigns(), dtype=np.float64)
