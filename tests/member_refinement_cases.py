"""Stacks of small independent KKT systems for the per-member refinement rule
(hipkkt_kkt_system_set_member_refinement), with the host prediction of what each member's own loop and the joint loop do
-- TEST INFRASTRUCTURE ONLY, shared by tests/test_member_refinement_reference_host.py (which asserts the margins on the
CPU, on the image the C oracle assembles) and tests/test_gpu_member_refinement.py (which asserts them again on the image
the device holds, then asks the device).

Settings are those of residual_reference.refinement_case: static regularisation 1e-4 constant with proportional part 0,
so that the bare solve of the regularised factor is wrong at the 1e-4 level and a round gains about four digits.

A member is (n, cone list) with a diagonal P in [0.5, 1.5], a dense A with entries of magnitude in [0.5, 1.5] and an
interior point (s, z) for the scaling; `singular` members have more equality rows than variables, so that K_b is singular and a random right-hand
side inconsistent: their residual stagnates at the size of the right-hand side whatever the rounds.
"""
import math
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from tests import residual_reference as rr

STOP_RATIO = 5.0
MAX_ITER = 20
MARGIN = 4.0
# Residual norms under these settings fall by about 1e4 per round: ~1e-4, ~1e-8, ~1e-12 times the right-hand side's scale.
# The tolerance sits in the gap between the second and the third, clear of both by more than MARGIN in every stack below
# (the host test asserts it).
ABSTOL = 3e-10


@dataclass
class Stack:
    name: str
    P: sp.csc_matrix
    A: sp.csc_matrix
    cones: list
    blocks: list                 # (n_b, m_b)
    s: np.ndarray
    z: np.ndarray
    scales: list                 # right-hand side scale per member (0: a zero member)
    kinds: list                  # "healthy" | "singular" | "zero" per member
    abstol: float = ABSTOL
    reltol: float = 0.0
    seed: int = 0
    meta: dict = field(default_factory=dict)

    @property
    def nb(self):
        return len(self.blocks)

    @property
    def n(self):
        return self.P.shape[0]

    @property
    def m(self):
        return self.A.shape[0]

    def settings(self):
        return dict(static_regularization_constant=rr.REG_EPS, static_regularization_proportional=0.0,
                    iterative_refinement_reltol=self.reltol, iterative_refinement_abstol=self.abstol,
                    iterative_refinement_max_iter=MAX_ITER)

    def oracle_settings(self):
        return dict(static_reg_constant=rr.REG_EPS, static_reg_proportional=0.0, ir_reltol=self.reltol, ir_abstol=self.abstol,
                    ir_max_iter=MAX_ITER)


def _interior(cones, rng):
    """Nonnegative rows in [0.7, 1.4] (so that Hs = s / z stays within [0.5, 2]), second-order cones (|t| + 1, t) with a
    short t, zero cone rows 0."""
    from cuclarabel_amd.cones import NonnegativeConeT, SecondOrderConeT
    out = []
    for c in cones:
        if isinstance(c, NonnegativeConeT):
            out.append(rng.uniform(0.7, 1.4, c.numel))
        elif isinstance(c, SecondOrderConeT):
            t = 0.3 * rng.standard_normal(c.numel - 1)
            out.append(np.concatenate([[np.linalg.norm(t) + 1.0], t]))
        else:
            out.append(np.zeros(c.numel))
    return np.concatenate(out + [np.zeros(0)])


def _member(rng, n, cones):
    m = sum(c.numel for c in cones)
    P = sp.diags(rng.uniform(0.5, 1.5, n), format="csc")
    A = sp.csc_matrix(rng.uniform(0.5, 1.5, (m, n)) * rng.choice([-1.0, 1.0], (m, n)))
    return P, A, cones, _interior(cones, rng), _interior(cones, rng)


def make_stack(name, members, scales, seed, abstol=ABSTOL, reltol=0.0, **meta):
    """members: list of (kind, n, cone list)."""
    rng = np.random.default_rng(seed)
    parts = [_member(rng, n, cones) for _, n, cones in members]
    P = sp.triu(sp.block_diag([p[0] for p in parts], format="csc"), format="csc")
    A = sp.csc_matrix(sp.block_diag([p[1] for p in parts], format="csc"))      # (a member without cones: a 0 x n block)
    assert A.shape == (sum(p[1].shape[0] for p in parts), P.shape[0])
    A.sort_indices()
    return Stack(name, P, A, [c for p in parts for c in p[2]], [(p[0].shape[0], p[1].shape[0]) for p in parts],
                 np.concatenate([p[3] for p in parts]), np.concatenate([p[4] for p in parts]), list(scales),
                 [k for k, _, _ in members], abstol, reltol, seed, meta)


def member_rows(st):
    """Per member the rows of K's image it owns: its x rows, its z rows, and the two expansion rows behind n + m of each
    of its sparse second-order cones (dimension > 4), taken in cone order."""
    from cuclarabel_amd.cones import SecondOrderConeT
    x_off = np.concatenate([[0], np.cumsum([b[0] for b in st.blocks])])
    z_off = np.concatenate([[0], np.cumsum([b[1] for b in st.blocks])])
    rows = [list(range(x_off[k], x_off[k + 1])) + [st.n + i for i in range(z_off[k], z_off[k + 1])] for k in range(st.nb)]
    off, pc = 0, 0
    for c in st.cones:
        if isinstance(c, SecondOrderConeT) and c.numel > 4:
            k = int(np.searchsorted(z_off, off, side="right") - 1)
            rows[k] += [st.n + st.m + pc, st.n + st.m + pc + 1]
            pc += 2
        off += c.numel
    return [np.array(r, dtype=np.int64) for r in rows], st.n + st.m + pc


def rhs(st, N, rows, seed=None):
    """b over the image: entries of magnitude in [0.5, 1] and random sign times the member's scale on its x and z rows, 0
    on expansion rows (kktsolver_setrhs)."""
    rng = np.random.default_rng(st.seed + 77 if seed is None else seed)
    b = np.zeros(N)
    for k, r in enumerate(rows):
        v = rng.uniform(0.5, 1.0, r.size) * rng.choice([-1.0, 1.0], r.size) * st.scales[k]
        v[r >= st.n + st.m] = 0.0
        b[r] = v
    return b


def oracle_image(st):
    """(K as the full symmetric CSR image of the un-regularised matrix, dsigns) from the C oracle on the CPU."""
    from tests import oracle_bindings as ob
    o = ob.OracleKKT(st.P, st.A, st.cones, settings=ob.default_settings(**st.oracle_settings()))
    if st.m:
        assert o.update_scaling(st.s, st.z)
    assert o.kktsolver_update()
    U_ = sp.csc_matrix(o.K())
    U_.sort_indices()
    return rr.sym_from_triu(U_.indptr, U_.indices, U_.data), np.array(o.dsigns(), dtype=np.float64)


def stagnation_margin(pred, tol):
    """For a member whose residual stagnates only the STOP decision is asserted: its first norm is clear of the tolerance
    and its first ratio clear of stop_ratio (it is about 1: not clear of the accept threshold, so neither its accept
    decision nor its x is ever compared)."""
    assert pred["rounds"] == 1 and pred["stop"] == "ratio", pred["norms"]
    return min(rr.margin(pred["norms"][0], tol) if tol > 0 else math.inf,
               rr.margin(pred["norms"][0] / pred["norms"][1], STOP_RATIO))


def predict(st, K, dsigns, b, rows):
    """dict(members = [refine_loop on member b's block with its own rows of b], joint = refine_loop on the stack,
    joint_member_norme = per member ||e_b|| of the joint loop's final x).  Members with a non-finite right-hand side are
    predicted 'bad' with 0 rounds."""
    preds = []
    for k, r in enumerate(rows):
        bk = b[r]
        if not np.all(np.isfinite(bk)):
            preds.append(dict(rounds=0, stop="bad", ok=False, norms=[math.inf], margin=math.inf, normb=math.inf, x=None))
            continue
        Kb = sp.csr_matrix(K[r][:, r])
        fac = rr.HostFactor(Kb, dsigns[r], rr.REG_EPS)
        preds.append(rr.refine_loop(Kb, fac, bk, st.abstol, st.reltol, STOP_RATIO, MAX_ITER))
    out = dict(members=preds)
    if np.all(np.isfinite(b)):
        fac = rr.HostFactor(K, dsigns, rr.REG_EPS)
        joint = rr.refine_loop(K, fac, b, st.abstol, st.reltol, STOP_RATIO, MAX_ITER)
        e = b - K @ joint["x"]
        out["joint"] = joint
        out["joint_member_norme"] = [float(np.abs(e[r]).max()) for r in rows]
    return out


def member_tol(st, pred):
    return st.abstol + st.reltol * pred["normb"]


def assert_margins(st, P):
    """Every decision whose outcome a GPU test asserts is clear of its threshold by MARGIN: all of a healthy or zero
    member's; the stop decision alone of a singular one."""
    for k, p in enumerate(P["members"]):
        if p["stop"] == "bad":
            continue
        if st.kinds[k] == "singular":
            mg = stagnation_margin(p, member_tol(st, p))
        else:
            mg = p["margin"]
        assert p["ok"] and mg >= MARGIN, ("a decision too close to its threshold", st.name, k, mg, p["norms"])


# ------------------------------------------------------------------------------------------------ the stacks
def _nn(k):
    from cuclarabel_amd.cones import NonnegativeConeT
    return NonnegativeConeT(k)


def _zero(k):
    from cuclarabel_amd.cones import ZeroConeT
    return ZeroConeT(k)


def _soc(k):
    from cuclarabel_amd.cones import SecondOrderConeT
    return SecondOrderConeT(k)


def _healthy(n=6, zero=1, nn=4):
    return ("healthy", n, ([_zero(zero)] if zero else []) + ([_nn(nn)] if nn else []))


def stagnating():
    """One singular and inconsistent member (2 variables, 3 equality rows), then healthy members with right-hand sides
    scaled 1, 1e-3 and 1e-9, and a zero member."""
    return make_stack("stagnating", [("singular", 2, [_zero(3)]), _healthy(), _healthy(), _healthy(), ("zero", 4, [_nn(3)])],
                      [1.0, 1.0, 1e-3, 1e-9, 0.0], seed=9101)


def alike(nb=4):
    """Members scaled alike: each takes the joint rule's own decisions."""
    return make_stack("alike", [_healthy() for _ in range(nb)], [1.0] * nb, seed=9102)


def edges(nb):
    """The edge shapes of the host driver in one stack of nb in {4, 5} members: a member of one x row and nothing else; a
    member whose only z rows belong to a sparse second-order cone of dimension 5 (two expansion rows far from its other
    rows); a member of 32 rows (a chunk of the 8-lane kernel exactly) and one of 33; with nb = 5 a zero member too."""
    members = [("healthy", 1, []), ("healthy", 3, [_soc(5)]), ("healthy", 12, [_zero(2), _nn(18)]),
               ("healthy", 12, [_zero(2), _nn(19)])]
    scales = [1.0, 1.0, 1e-3, 1.0]
    if nb == 5:
        members.append(("zero", 3, [_nn(2)]))
        scales.append(0.0)
    return make_stack(f"edges{nb}", members, scales, seed=9106, chunk_rows=(32, 33))


def many(nb=700):
    """nb members of three rows each (one variable, two inequality rows), scales cycling 1, 1e-3, 0, 1e-9."""
    cyc = (1.0, 1e-3, 0.0, 1e-9)
    return make_stack(f"many{nb}", [("zero" if cyc[k % 4] == 0.0 else "healthy", 1, [_nn(2)]) for k in range(nb)],
                      [cyc[k % 4] for k in range(nb)], seed=9110)


def relative():
    """reltol > 0, abstol 0, the members' ||b_b|| 1e3 apart: with its own ||b_b|| the small member needs the rounds the
    large one needs; under the stack's ||b|| its first round would already meet the tolerance."""
    return make_stack("relative", [_healthy(), _healthy(), _healthy()], [1.0, 1e-3, 1.0], seed=9120, abstol=0.0, reltol=3e-10)
