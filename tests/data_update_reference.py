"""Host model of the data-updating path of level C (hipkkt_kkt_system_set_equilibration, the four
hipkkt_kkt_system_update_data_* calls, hipkkt_kkt_system_data_norms) -- TEST INFRASTRUCTURE ONLY.

DataModel extends kvalue_reference.KModel -- K's two copies, kpos and the dirty flag -- by what the data updates add: the
frozen scalings d, e, c, the handle's scaled copies of P's and A's values, q, -q and b, the two staleness marks, and the
arithmetic of the update kernels (csrc/kernels.hip, "data updates"), every value of which has one correct fp64 answer
because the kernels are built without contraction:

    P: fl(fl(v * fl(d[row] * d[col])) * c)      A: fl(v * fl(e[row] * d[col]))
    q: fl(fl(v * d[i]) * c)                     b: fl(v * e[i])

The protocol: an update writes Kval and, when the image is current, its one or two kpos slots; it never
writes into a dirty image and never makes a current one dirty.  P and A updates leave the factorisation stale, all four
leave (x2, z2) stale; kkt_update! clears the first mark, the constant-RHS solve the second; a solve that would read stale
state is refused.

A "device" in the sequences below is a DataModel (possibly with a seeded fault) or the GPU adapter of
tests/test_gpu_data_update.py; both have the same methods, and `check` compares either with a fault-free model that
received the same calls.
"""
import numpy as np

from tests import kvalue_reference as kv

FAULTS = ("scaling_operand", "missing_negq", "through_while_dirty", "second_slot", "stale_accepted")
UPDATE_BLOCK = 256                              # k_data_update_*: 256 lanes, <= UPDATE_GRID_CAP workgroups (launch_shapes.hpp)
UPDATE_GRID_CAP = 4096


class Refused(Exception):
    """the call was refused (HIPKKT_ERR_ARG on the device); .pos names the offending place of an index array, if any"""

    def __init__(self, msg, pos=None):
        super().__init__(msg)
        self.pos = pos


def entry_coords(colptr, rowval, maps, n):
    """(Prow, Pcol, Arow, Acol): every stored entry's row and column in its own matrix, from K = [P A'; A -Hs] (triu CSC)."""
    colptr, rowval = np.asarray(colptr, np.int64), np.asarray(rowval, np.int64)
    col = np.repeat(np.arange(colptr.size - 1, dtype=np.int64), np.diff(colptr))
    P, A = np.asarray(maps["P"], np.int64), np.asarray(maps["A"], np.int64)
    assert (rowval[P] <= col[P]).all() and (col[P] < n).all() and (rowval[A] < n).all() and (col[A] >= n).all()
    return rowval[P], col[P], col[A] - n, rowval[A]


def check_index(index, k, length):
    """the library's index check (csrc/data_update.cpp): first out-of-range place, else the first place that repeats an
    earlier one; None if the positions are fine"""
    index = np.asarray(index, np.int64)
    bad = np.flatnonzero((index < 0) | (index >= length))
    if bad.size:
        return "range", int(bad[0])
    seen = set()
    for t, j in enumerate(index.tolist()):
        if j in seen:
            return "repeat", t
        seen.add(j)
    return None


class DataModel(kv.KModel):
    """fault: None or one of FAULTS, a simulated defect of the data-update path (the value path below it is KModel's,
    fault-free)."""

    def __init__(self, colptr, rowval, maps, cones, Pdata, Adata, n, m, fault=None, **kw):
        assert fault is None or fault in FAULTS, fault
        super().__init__(colptr, rowval, maps, cones, Pdata, Adata, **kw)
        self.dfault = fault
        self.n, self.m = int(n), int(m)
        self.Prow, self.Pcol, self.Arow, self.Acol = entry_coords(colptr, rowval, self.maps, self.n)
        self.Pval, self.Aval = np.array(Pdata, np.float64), np.array(Adata, np.float64)
        self.d, self.e, self.c = np.ones(self.n), np.ones(self.m), 1.0
        self.q = self.negq = self.b = None
        self.ready = False
        self.deferred = False
        self.factor_stale = self.const_stale = False

    # ---- the library's calls
    def set_equilibration(self, d=None, e=None, c=1.0):
        if d is None and e is None:
            self.d, self.e, self.c = np.ones(self.n), np.ones(self.m), 1.0
            return
        if (d is None and self.n) or (e is None and self.m) or not (c > 0 and np.isfinite(c)):
            raise Refused("set_equilibration")
        self.d, self.e, self.c = np.array(d, np.float64), np.array(e, np.float64), float(c)

    def init(self, q, b):
        """hipkkt_kkt_system_init: q and b as given (already scaled)"""
        self.q, self.b = np.array(q, np.float64), np.array(b, np.float64)
        self.negq = -self.q
        self.ready = True

    def _scaled(self, which, v, j):
        wrong = self.dfault == "scaling_operand"
        with np.errstate(all="ignore"):
            if which == "P":
                return v * (self.d[self.Prow[j]] * self.d[self.Prow[j] if wrong else self.Pcol[j]]) * self.c
            if which == "A":
                return v * (self.e[self.Arow[j]] * self.d[self.Acol[j]]) * (self.c if wrong else 1.0)
            if which == "q":
                return v * self.d[j] * (1.0 if wrong else self.c)
            return v * self.e[j] * (self.c if wrong else 1.0)

    def length(self, which):
        return {"P": self.Pval.size, "A": self.Aval.size, "q": self.n, "b": self.m}[which]

    def update_data(self, which, values, index=None):
        """hipkkt_kkt_system_update_data_<which>; raises Refused and changes nothing where the library refuses"""
        v = np.asarray(values, np.float64).ravel()
        k, length = v.size, self.length(which)
        if self.deferred:
            raise Refused("deferred status")
        if which in "qb" and not self.ready:
            raise Refused("before init")
        if k == 0:
            return
        if index is None:
            if k != length:
                raise Refused("wrong k")
            j = np.arange(length)
        else:
            j = np.asarray(index, np.int64).ravel()
            assert j.size == k
            bad = check_index(j, k, length)
            if bad is not None:
                raise Refused(bad[0], bad[1])
        s = self._scaled(which, v, j)
        if which in "PA":
            (self.Pval if which == "P" else self.Aval)[j] = s
            entries = self.maps[which][j]
            through = not self.dirty
            if self.dfault == "through_while_dirty" and self.dirty:
                through, self.dirty = True, False              # writes into a stale copy, and the gather never comes
            self.Kval[entries] = s
            if through:
                p0 = self.kpos[2 * entries]
                self.fval[p0[p0 >= 0]] = s[p0 >= 0]
                if self.dfault != "second_slot":
                    p1 = self.kpos[2 * entries + 1]
                    self.fval[p1[p1 >= 0]] = s[p1 >= 0]
            self.factor_stale = True
        elif which == "q":
            self.q[j] = s
            if self.dfault != "missing_negq":
                self.negq[j] = -s
        else:
            self.b[j] = s
        self.const_stale = True

    def level_b_update_P(self, vals):
        """hipkkt_kkt_update_P: already-scaled values, the image dirty, no staleness mark"""
        self.update_P(vals)
        self.Pval = np.array(vals, np.float64)

    def system_update(self, Hs, u=(), v=(), eta2=()):
        """kkt_update! (eager): the cone update, the factorisation, the constant-RHS solve (whose refinement reads the image)"""
        self.update_cones(Hs, u, v, eta2)
        self.factor_stale = False
        self.spmv_use()
        self.const_stale = False
        return True

    def solve(self):
        """hipkkt_kkt_system_solve: refused while it would read stale state"""
        if (self.factor_stale or self.const_stale) and self.dfault != "stale_accepted":
            raise Refused("stale")
        self.spmv_use()
        return True

    def observe_qb(self):
        """(q, -q, b) as the handle holds them"""
        return self.q.copy(), self.negq.copy(), self.b.copy()

    def data_norms(self):
        with np.errstate(all="ignore"):
            nq = np.abs(self.q * (1.0 / self.d)).max() / self.c if self.n else 0.0
            nb = np.abs(self.b * (1.0 / self.e)).max() if self.m else 0.0
        return float(nq), float(nb)

    @property
    def handle(self):
        return self


def model_of_case(case, K, maps, fault=None, **kw):
    """the model of a handle just created from kvalue_reference.Case `case`; K: its triu CSC pattern (scipy), maps: its maps"""
    return DataModel(K.indptr, K.indices, maps, case.cones, case.P.data, case.A.data, case.n, case.m, fault=fault, **kw)


# ------------------------------------------------------------------------------------------------ inputs
def scalings(n, m, seed, lo=1e-4, hi=1e4):
    """d, e log-uniform over [lo, hi] with both ends present, c != 1 and no power of two"""
    rng = np.random.default_rng(seed)
    d = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    e = np.exp(rng.uniform(np.log(lo), np.log(hi), m))
    for v in (d, e):
        if v.size >= 2:
            v[0], v[-1] = lo, hi
    return d, e, 0.37


def new_values(k, seed):
    """k values of either sign with magnitudes in [8, 16) or (1/16, 1/8]: at least a factor 4 off values of order one"""
    rng = np.random.default_rng(seed)
    mag = np.where(rng.random(k) < 0.5, rng.uniform(8.0, 16.0, k), 1.0 / rng.uniform(8.0, 16.0, k))
    return mag * rng.choice([-1.0, 1.0], k)


def values_like(base, seed):
    """`base` with every entry scaled by a factor of its own in [8, 16) (even seed) or (1/16, 1/8] (odd seed): for the
    P of kvalue_reference's cases (diagonal in [1, 2], off-diagonals below 0.2) the result stays diagonally dominant with a
    positive diagonal, so that a handle that factorises afterwards keeps a quasi-definite K"""
    base = np.asarray(base, np.float64)
    f = np.random.default_rng(seed).uniform(8.0, 16.0, base.size)
    return base * (f if seed % 2 == 0 else 1.0 / f)


# ------------------------------------------------------------------------------------------------ comparisons
def check(dev, model, tag, seed=0):
    """Kval byte for byte, the image the residual reads, and the handle's q, -q, b where it has them"""
    kv.assert_values(dev.handle, model, tag)
    kv.assert_image(dev.handle, model, tag, seed=seed)
    model.spmv_use()                                           # (the probe read the image: gathered if it was dirty)
    if model.ready:
        for name, got, want in zip(("q", "-q", "b"), dev.observe_qb(), model.observe_qb()):
            if not np.array_equal(got, want):
                bad = np.flatnonzero(~(got == want))
                raise kv.ValuePathError("check", f"{tag}: {name} differs at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}")


def expect_refused(dev, model, tag, call, pos=None):
    """`call(device)` must be refused by both, with the same offending place, and leave both unchanged"""
    before = model.Kval.copy()
    for who in (dev, model):
        try:
            call(who)
        except Refused as r:
            if pos is not None and r.pos != pos:
                raise kv.ValuePathError("refusal", f"{tag}: names place {r.pos}, expected {pos}")
        else:
            raise kv.ValuePathError("refusal", f"{tag}: accepted by {'the model' if who is model else 'the device'}")
    assert np.array_equal(model.Kval, before)
    check(dev, model, tag + " (after the refusal)")


def both(dev, model, name, *args, **kw):
    out = getattr(dev, name)(*args, **kw)
    getattr(model, name)(*args, **kw)
    return out


# ------------------------------------------------------------------------------------------------ sequences
def sequence_vector_P(dev, model, case, seed):
    """create, probe, update_data_P vector, probe: written through"""
    check(dev, model, "seqA create")
    assert not model.dirty
    both(dev, model, "update_data", "P", values_like(case.P.data, seed))
    assert not model.dirty, "an update must not make a current image dirty"
    check(dev, model, "seqA update_data_P vector (written through)")


def sequence_indexed_A(dev, model, case, seed):
    """cone update, update_data_A indexed, solve refused, system_update, solve, probe"""
    both(dev, model, "system_update", *case.hs(0))
    check(dev, model, "seqB system_update(H1)")
    nA = model.length("A")
    idx = np.random.default_rng(seed).permutation(nA)[:max(1, nA // 3)]
    both(dev, model, "update_data", "A", new_values(idx.size, seed + 1), idx)
    check(dev, model, "seqB update_data_A indexed")
    expect_refused(dev, model, "seqB solve on stale state", lambda w: w.solve())
    both(dev, model, "system_update", *case.hs(1))
    if not dev.solve():
        raise kv.ValuePathError("solve", "seqB: the solve failed")
    model.solve()
    check(dev, model, "seqB system_update(H2) solve")


def sequence_dirty_P(dev, model, case, seed):
    """hipkkt_kkt_update_P (dirty), update_data_P indexed: nothing written through; the gather picks it up"""
    both(dev, model, "level_b_update_P", case.P2())
    assert model.dirty
    nP = model.length("P")
    diag = np.flatnonzero(model.Prow == model.Pcol)
    off = np.flatnonzero(model.Prow != model.Pcol)
    idx = np.concatenate([diag[:1], off[:1], [nP - 1]]) if off.size else diag[:1]
    idx = np.unique(idx)[::-1].copy()                                  # (unsorted input is fine)
    both(dev, model, "update_data", "P", values_like(case.P.data, seed + 1)[idx], idx)
    assert model.dirty, "an update into a dirty image leaves the flag set"
    check(dev, model, "seqC update_P (level B) update_data_P indexed while dirty")


def sequence_diag_and_offdiag(dev, model, case, seed):
    """an indexed update of one diagonal entry of P (second kpos slot -1) and one off-diagonal entry (two slots), image current"""
    check(dev, model, "seqD probe")
    diag = np.flatnonzero(model.Prow == model.Pcol)
    off = np.flatnonzero(model.Prow != model.Pcol)
    assert diag.size and off.size
    assert model.kpos[2 * model.maps["P"][diag[0]] + 1] == -1 and model.kpos[2 * model.maps["P"][off[-1]] + 1] >= 0
    idx = np.array([off[-1], diag[0]])
    both(dev, model, "update_data", "P", values_like(case.P.data, seed)[idx], idx)
    check(dev, model, "seqD diagonal and off-diagonal entry")


def sequence_indexed_all_equals_vector(dev, model, case, seed):
    """indexed-all (in a scrambled order) leaves what the vector form leaves, bit for bit"""
    for which in ("P", "A", "q", "b"):
        k = model.length(which)
        v = values_like(case.P.data, seed) if which == "P" else new_values(k, seed + ord(which))
        perm = np.random.default_rng(seed).permutation(k)
        both(dev, model, "update_data", which, v[perm], perm)
        check(dev, model, f"seqE update_data_{which} indexed-all")
        want = (model.Kval.copy(), model.observe_qb())
        both(dev, model, "update_data", which, 2.0 * v)                # (something else in between)
        both(dev, model, "update_data", which, v)
        check(dev, model, f"seqE update_data_{which} vector")
        assert np.array_equal(model.Kval, want[0]) and all(np.array_equal(a, b) for a, b in zip(model.observe_qb(), want[1]))


def sequence_qb(dev, model, case, seed):
    """q and b, vector and indexed"""
    check(dev, model, "seqF init")
    both(dev, model, "update_data", "q", new_values(model.n, seed))
    check(dev, model, "seqF update_data_q vector")
    both(dev, model, "update_data", "b", new_values(model.m, seed + 1))
    check(dev, model, "seqF update_data_b vector")
    both(dev, model, "update_data", "q", new_values(2, seed + 2), np.array([model.n - 1, 0]))
    both(dev, model, "update_data", "b", new_values(2, seed + 3), np.array([model.m - 1, 0]))
    check(dev, model, "seqF update_data_q / _b indexed")
    got, want = dev.data_norms(), model.data_norms()
    if got != want:
        raise kv.ValuePathError("data_norms", f"seqF: {got!r} != {want!r}")


SEQUENCES = (sequence_vector_P, sequence_indexed_A, sequence_dirty_P, sequence_diag_and_offdiag,
             sequence_indexed_all_equals_vector, sequence_qb)


def run_all(dev, model, case, seed=4000, factorise=True):
    """every sequence on one handle, in order; factorise = False leaves out the one that factorises and solves (for
    scalings under which K is too badly conditioned to ask that of it)"""
    assert seed % 2 == 0
    for i, seq in enumerate(SEQUENCES):
        if factorise or seq is not sequence_indexed_A:
            seq(dev, model, case, seed + 100 * i)
