"""Host model of the member cost scalings of a stack of independent problems (hipkkt_kkt_system_set_equilibration_batch,
the hipkkt_kkt_system_update_data_P / _q calls under it, hipkkt_kkt_system_data_norms_batch) -- TEST INFRASTRUCTURE ONLY.

BatchDataModel extends data_update_reference.DataModel by the partition (x_off, z_off -> xmem, zmem) and one cost scaling
per member.  With member costs held, the c of

    P: fl(fl(v * fl(d[row] * d[col])) * c)      q: fl(fl(v * d[i]) * c)

is that of the ROW's member (csrc/kernels.hip: k_data_update_matrix_member / k_data_update_vector_member); A and b carry
no c.  The norms are, per member b, max |q_i dinv_i| / c_b over its x rows and max |b_i einv_i| over its z rows, taken as
the kernel takes them: wave by wave of 64 combined rows (x rows, then z rows), a wave whose rows share one word folded
into that word, a wave that straddles a boundary lane by lane (k_data_norms_member).  A maximum does not depend on the
order, so the fault-free model equals numpy's maxima; the wave walk is there so that the fold's defect can be seeded.

Seeded faults (BFAULTS), each caught by tests/test_batch_equilibration_reference_host.py:
    joint_c            the handle's one c used for every member
    column_member      the member read through the entry's COLUMN (shows only with an inconsistent row -> member table)
    c_before_d         fl(fl(v * c) * fl(d d)) and fl(fl(v * c) * d): c applied before d
    norm_wrong_member  a member's max |q dinv| divided by the next member's c
    straddle_fold      a wave that straddles a boundary folds all its rows into its first lane's word
"""
import numpy as np

from tests import data_update_reference as du
from tests.data_update_reference import Refused

BFAULTS = ("joint_c", "column_member", "c_before_d", "norm_wrong_member", "straddle_fold")
WAVE = 64


def offsets(blocks):
    """(x_off, z_off) of the members' (n_b, m_b)"""
    x_off = np.concatenate([[0], np.cumsum([b[0] for b in blocks])]).astype(np.int64)
    z_off = np.concatenate([[0], np.cumsum([b[1] for b in blocks])]).astype(np.int64)
    return x_off, z_off


class BatchDataModel(du.DataModel):
    """bfault: None or one of BFAULTS (the data-update path below is DataModel's, fault-free)."""

    def __init__(self, *args, bfault=None, **kw):
        assert bfault is None or bfault in BFAULTS, bfault
        super().__init__(*args, **kw)
        self.bfault = bfault
        self.nb = 0
        self.x_off = self.z_off = self.xmem = self.zmem = None
        self.cmem = None                                  # the members' cost scalings, or None: the handle's one c

    # ---- the library's calls
    def set_problems(self, blocks):
        """hipkkt_kkt_system_set_problems; refused while member cost scalings are held"""
        if self.deferred:
            raise Refused("deferred status")
        if self.cmem is not None:
            raise Refused("member cost scalings are held")
        blocks = list(blocks or [])
        if not blocks:
            self.nb, self.x_off = 0, None
            return
        x_off, z_off = offsets(blocks)
        if x_off[-1] != self.n or z_off[-1] != self.m or min(b[0] for b in blocks) < 1:
            raise Refused("partition")
        self.nb, self.x_off, self.z_off = len(blocks), x_off, z_off
        self.xmem = np.repeat(np.arange(self.nb), np.diff(x_off))
        self.zmem = np.repeat(np.arange(self.nb), np.diff(z_off))

    def set_equilibration(self, d=None, e=None, c=1.0):
        super().set_equilibration(d, e, c)
        self.cmem = None                                  # (one joint c again)

    def set_equilibration_batch(self, d, e, c):
        """hipkkt_kkt_system_set_equilibration_batch; Refused.pos names the member whose c is refused"""
        if self.deferred:
            raise Refused("deferred status")
        if self.nb <= 0:
            raise Refused("no partition")
        c = np.array(c, np.float64).ravel()
        assert c.size == self.nb
        bad = np.flatnonzero(~((c > 0) & np.isfinite(c)))
        if bad.size:
            raise Refused("c", int(bad[0]))
        if d is None and e is None:
            self.d, self.e = np.ones(self.n), np.ones(self.m)
        elif (d is None and self.n) or (e is None and self.m):
            raise Refused("set_equilibration_batch")
        else:
            self.d, self.e = np.array(d, np.float64), np.array(e, np.float64)
        self.cmem = c                                     # (self.c, the scalar call's, is left alone)

    def _scaled(self, which, v, j):
        if self.cmem is None or which in "Ab":
            return super()._scaled(which, v, j)
        f = self.bfault
        with np.errstate(all="ignore"):
            if which == "P":
                row, col = self.Prow[j], self.Pcol[j]
                c = np.full(len(j), self.c) if f == "joint_c" else self.cmem[self.xmem[col if f == "column_member" else row]]
                if f == "c_before_d":
                    return (v * c) * (self.d[row] * self.d[col])
                return v * (self.d[row] * self.d[col]) * c
            c = np.full(len(j), self.c) if f == "joint_c" else self.cmem[self.xmem[j]]
            if f == "c_before_d":
                return (v * c) * self.d[j]
            return v * self.d[j] * c

    def data_norms_batch(self):
        """hipkkt_kkt_system_data_norms_batch -> (nb, 2)"""
        if self.deferred:
            raise Refused("deferred status")
        if not self.ready:
            raise Refused("before init")
        if self.nb <= 0:
            raise Refused("no partition")
        with np.errstate(all="ignore"):
            prod = np.concatenate([np.abs(self.q * (1.0 / self.d)), np.abs(self.b * (1.0 / self.e))])
        word = np.concatenate([2 * self.xmem, 2 * self.zmem + 1])
        bits = np.zeros(2 * self.nb, np.uint64)           # integer maxima on the bit patterns, as the kernel takes them
        pat = prod.view(np.uint64)
        for w0 in range(0, prod.size, WAVE):
            ws, ps = word[w0:w0 + WAVE], pat[w0:w0 + WAVE]
            if (ws == ws[0]).all() or self.bfault == "straddle_fold":
                bits[ws[0]] = max(bits[ws[0]], ps.max())
            else:
                np.maximum.at(bits, ws, ps)
        val = bits.view(np.float64).reshape(self.nb, 2).copy()
        c = self.cmem if self.cmem is not None else np.full(self.nb, self.c)
        if self.bfault == "norm_wrong_member":
            c = np.roll(c, -1)
        if self.bfault == "joint_c":
            c = np.full(self.nb, self.c)
        with np.errstate(all="ignore"):
            val[:, 0] = val[:, 0] / c
        return val


def model_of_case(case, K, maps, bfault=None, **kw):
    """the model of a handle just created from kvalue_reference.Case `case`"""
    return BatchDataModel(K.indptr, K.indices, maps, case.cones, case.P.data, case.A.data, case.n, case.m, bfault=bfault, **kw)


def numpy_norms(model):
    """the members' norms as numpy takes them, member by member -- what data_norms_batch must equal"""
    out = np.zeros((model.nb, 2))
    with np.errstate(all="ignore"):
        pq, pb = np.abs(model.q * (1.0 / model.d)), np.abs(model.b * (1.0 / model.e))
        c = model.cmem if model.cmem is not None else np.full(model.nb, model.c)
        for b in range(model.nb):
            xs, zs = pq[model.x_off[b]:model.x_off[b + 1]], pb[model.z_off[b]:model.z_off[b + 1]]
            out[b, 0] = (np.nan if np.isnan(xs).any() else xs.max()) / c[b]
            out[b, 1] = 0.0 if zs.size == 0 else (np.nan if np.isnan(zs).any() else zs.max())
    return out


def same(a, b):
    """== with NaN equal to NaN (a member's NaN norm)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------------------------------------ inputs
def member_costs(nb, seed, lo=1e-4, hi=1e4):
    """c_b log-uniform over eight decades with both ends present (nb >= 2), no power of two"""
    rng = np.random.default_rng(seed)
    c = np.exp(rng.uniform(np.log(lo), np.log(hi), nb)) * 1.0123
    if nb >= 2:
        c[0], c[-1] = lo * 1.0123, hi * 1.0123
    return c


# the stacks the member-cost kernels can go wrong at: (x rows, z rows, has a P) per member
STACKS = {
    "one": [(6, 4, True)],
    "edges": [(1, 2, True), (63, 3, True), (64, 0, True), (65, 5, True), (255, 1, True), (256, 4, True), (257, 2, True)],
    "no_z_no_P": [(4, 2, True), (70, 3, False), (5, 0, True)],
    "300": [(2, 1, True)] * 300,
}


def stack_case(name):
    """kvalue_reference.Case of STACKS[name]: tridiagonal P blocks (none where the member has no P), one or two entries per
    row of A, a nonnegative cone over each member's z rows; -> (case, blocks)"""
    import scipy.sparse as sp
    from cuclarabel_amd.cones import NonnegativeConeT
    from tests import kvalue_reference as kv
    rng = np.random.default_rng(9100 + len(name))
    Ps, As, cones, blocks = [], [], [], []
    for nx, nz, hasP in STACKS[name]:
        Ps.append(kv._tridiag_P(nx, rng) if hasP else sp.csc_matrix((nx, nx)))
        As.append(kv._one_or_two_per_row(nz, nx, rng) if nz else sp.csc_matrix((0, nx)))
        if nz:
            cones.append(NonnegativeConeT(nz))
        blocks.append((nx, nz))
    case = kv.Case("stack_" + name, sp.block_diag(Ps, format="csc"), sp.block_diag(As, format="csc"), cones, 9100)
    return case, blocks


# ------------------------------------------------------------------------------------------------ sequences
def alternating_index(model, which):
    """positions of `which` (P or q) that alternate between the first and the last member that has some"""
    mem = model.xmem[model.Prow] if which == "P" else model.xmem
    first, last = mem.min(), mem.max()
    a, b = np.flatnonzero(mem == first), np.flatnonzero(mem == last)
    k = min(a.size, b.size, 40)
    out = np.empty(2 * k, np.int64)
    out[0::2], out[1::2] = a[:k], b[::-1][:k]
    return np.unique(out) if first == last else out


def sequence_member_updates(dev, model, case, seed, check=du.check):
    """vector and indexed updates of P and q under member costs, `check` after every step; _A and _b beside them"""
    both = du.both
    check(dev, model, "create")
    nP, n = model.length("P"), model.n
    vP = du.values_like(case.P.data, seed)
    both(dev, model, "update_data", "P", vP)
    check(dev, model, "P vector")
    both(dev, model, "update_data", "q", du.new_values(n, seed + 1))
    check(dev, model, "q vector")
    for which, length in (("P", nP), ("q", n)):
        idx = alternating_index(model, which)                          # alternates between members
        vals = du.values_like(case.P.data, seed + 2)[idx] if which == "P" else du.new_values(idx.size, seed + 3)
        both(dev, model, "update_data", which, vals, idx)
        check(dev, model, f"{which} indexed, alternating between members")
        one = np.array([length - 1])                                   # of length 1: the last entry of the last member
        both(dev, model, "update_data", which, np.array([-3.25]), one)
        check(dev, model, f"{which} indexed, one entry")
        # an indexed update of every entry (scrambled) leaves what the vector form leaves
        v = du.values_like(case.P.data, seed + 4) if which == "P" else du.new_values(length, seed + 5)
        perm = np.random.default_rng(seed).permutation(length)
        both(dev, model, "update_data", which, v[perm], perm)
        check(dev, model, f"{which} indexed-all")
        want = (model.Kval.copy(), model.observe_qb())
        both(dev, model, "update_data", which, 2.0 * v)
        both(dev, model, "update_data", which, v)
        check(dev, model, f"{which} vector again")
        assert np.array_equal(model.Kval, want[0]) and all(np.array_equal(a, b) for a, b in zip(model.observe_qb(), want[1]))
    # _A and _b carry no c: a model that never heard of member costs agrees
    both(dev, model, "update_data", "A", du.new_values(model.length("A"), seed + 6))
    check(dev, model, "A vector")
    if model.m:
        both(dev, model, "update_data", "b", du.new_values(model.m, seed + 7))
        both(dev, model, "update_data", "b", np.array([7.5]), np.array([model.m - 1]))
        check(dev, model, "b vector and indexed")
    with np.errstate(all="ignore"):
        assert np.array_equal(model.Aval, du.new_values(model.length("A"), seed + 6) * (model.e[model.Arow] * model.d[model.Acol]))
