"""The device cone operations between the solves (hipkkt_kkt_system_affine_ds / _combined_ds / _step_length /
_shift_to_interior: csrc/step_kernels.hip) against the extended-precision reference of tests/step_reference.py.

The reference takes the fp64 vectors and the scaling the device itself holds (w, eta, lambda, R, Rinv read back after
system.update) as exact inputs, so these tests measure the new kernels alone, at the shapes where they could go wrong:
elementwise sizes around a workgroup and one row past the capped grid, second-order cones at wave-stride edges, one /
four / five to a handle and 1e-8 from the boundary, every PSD side class up to 48 with steps that leave the cone and
steps that do not, zero cones with garbage in between, and every exact branch of the second-order step length.  Every
operation is called twice and must repeat bit for bit.  Worst error / bound per quantity is printed under -s."""
import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd.cones import (ZeroConeT, NonnegativeConeT, SecondOrderConeT, PSDTriangleConeT, ExponentialConeT)
from tests import cone_reference as cr
from tests import step_reference as sr

pytestmark = pytest.mark.gpu

WORST = cr.Worst("device cone operations between the solves against the extended-precision reference")
SIGMA_MU, M_CORR = 0.3, 0.7


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    WORST.report()


class Dev:
    """a level-C handle over a cone list (P = I_2, A = ones(m, 2)), scaled at (s, z) unless s is None"""

    def __init__(self, cones, s=None, z=None, factor_may_fail=False):
        """factor_may_fail: K of a late iterate (Hs condition ~1e24) may be refused by the factorisation; the scaling is
        on the device either way, and the operations under test read nothing else"""
        import torch
        from cuclarabel_amd import _lib
        from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
        assert _lib.lib().hipkkt_available() == 1, "no gfx950 device visible"
        self.torch, self.cones = torch, list(cones)
        self.m = sum(c.numel for c in cones)
        self.ks = HipKKTSolver(sp.identity(2, format="csc"), sp.csc_matrix(np.ones((self.m, 2))), cones)
        self.system = HipKKTSystem(self.ks)
        self.system.init(np.zeros(2), np.zeros(self.m))
        self.sc = None
        if s is not None:
            assert self.system.update(s, z) or factor_may_fail
            lam, psd = self.ks.scaling()
            w, eta = self.ks.scaling_w()
            self.sc = sr.Scaling(cones, w, eta, lam, psd)

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")
        self.torch.cuda.synchronize()
        return t

    def down(self, t):
        self.ks.synchronize()
        return t.cpu().numpy()

    def out(self):
        t = self.torch.full((max(self.m, 1),), float("nan"), dtype=self.torch.float64, device="cuda")
        self.torch.cuda.synchronize()
        return t

    def twice(self, fn):
        """fn() -> numpy result, called twice: identical bits"""
        a, b = fn(), fn()
        a, b = np.asarray(a), np.asarray(b)
        assert a.tobytes() == b.tobytes(), "the same call on the same data gave other bits"
        return a

    def affine_ds(self):
        def run():
            o = self.out()
            assert self.system.affine_ds_dev(o.data_ptr())
            return self.down(o)[:self.m]
        return self.twice(run)

    def combined_ds(self, dz, ds, sigma_mu, m_corr):
        tz, ts = self.up(dz), self.up(ds)

        def run():
            o = self.out()
            assert self.system.combined_ds_dev(o.data_ptr(), tz.data_ptr(), ts.data_ptr(), sigma_mu, m_corr)
            return self.down(o)[:self.m]
        got = self.twice(run)
        assert self.down(tz).tobytes() == np.ascontiguousarray(dz).tobytes() and \
            self.down(ts).tobytes() == np.ascontiguousarray(ds).tobytes(), "an input was modified"
        return got

    def step_length(self, dz, ds, z, s, dtau=1.0, dkappa=1.0, tau=1.0, kappa=1.0):
        t = [self.up(v) for v in (dz, ds, z, s)]
        return float(self.twice(lambda: self.system.step_length_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                                                    t[3].data_ptr(), dtau, dkappa, tau, kappa)))

    def shift(self, v, primal):
        def run():
            t = self.up(v)
            mg = self.system.shift_to_interior_dev(t.data_ptr(), primal)
            return np.r_[mg, self.down(t)[:self.m]]
        r = self.twice(run)
        return r[0], r[1], r[2:]


def _within(ratios, where):
    WORST.add(ratios, where)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{where}: error / bound > 1 for {bad}"


def _family_ratios(err, bound, fam):
    return {f: cr.ratio(err[fam == f], bound[fam == f]) for f in set(fam[fam != None]) if f != "zero"}   # noqa: E711


def _zero_rows(cones):
    return sr.unit_rows(cones)[1]


def _check_ds(dev, case, where):
    zero = _zero_rows(case.cones)
    got = dev.affine_ds()
    val, bnd, fam = sr.ds_ref(dev.sc, case.dz, case.ds, 0.0, 0.0, False)
    assert np.all(got[zero] == 0.0), f"{where}: affine_ds left something in a zero cone's rows"
    _within({"aff_" + k: v for k, v in _family_ratios(got - val, bnd, fam).items()}, where)
    got = dev.combined_ds(case.dz, case.ds, SIGMA_MU, M_CORR)
    val, bnd, fam = sr.ds_ref(dev.sc, case.dz, case.ds, SIGMA_MU, M_CORR, True)
    assert np.all(got[zero] == 0.0), f"{where}: combined_ds left something in a zero cone's rows"
    _within(_family_ratios(got - val, bnd, fam), where)


def _check_step(dev, case, where, allow_ambiguous=False, **scal):
    lims = sr.cone_step_limits(dev.sc, case.dz, case.ds, case.z, case.s)
    ref = sr.fold_min(sr.alpha_max(scal.get("dtau", 1.0), scal.get("dkappa", 1.0), scal.get("tau", 1.0),
                                   scal.get("kappa", 1.0)) + lims)
    assert allow_ambiguous or not ref.ambiguous, f"{where}: generated point within its bound of a branch switch"
    got = dev.step_length(case.dz, case.ds, case.z, case.s, **scal)
    # the composite's result IS the minimum of the per-cone references (and alpha_max, bit for bit, when nothing binds)
    _within({(ref.family or "step"): ref.ratio(got)}, f"{where} ({ref.where})")
    if ref.family in ("one", "tau", "kappa") and not ref.ambiguous and ref.lo == ref.value:
        assert got == ref.value
    return got, ref


def _check_shift(dev, case, where, vectors=None):
    zero = _zero_rows(case.cones)
    if vectors is None:
        vectors = ((case.s - 2.0 * np.abs(case.s).max(), True, "outside"), (0.7 * case.z, False, None),
                   (1e3 * case.z, False, None))
    seen = set()
    for v, primal, want in vectors:
        ref = sr.shift_ref(case.cones, v, primal)
        assert ref["branch"] is not None and (want is None or ref["branch"] == want), (where, ref["branch"])
        seen.add(ref["branch"])
        mn, pos, got = dev.shift(v, primal)
        out = {ref["min"].family or "margin": ref["min"].ratio(mn), "pos_margin": cr.ratio(pos - ref["pos"], ref["bpos"]),
               "shift": cr.ratio(got - ref["value"], ref["bound"])}
        _within(out, f"{where} {ref['branch']}")
        if primal:
            assert np.all(got[zero] == 0.0), f"{where}: a primal shift must zero the zero cones' rows"
        else:
            assert got[zero].tobytes() == v[zero].tobytes(), f"{where}: a dual shift must leave the zero cones' rows alone"
    return seen


def _run(pieces, where, seed=1, one_shift=False, **kw):
    """one_shift: a single shifted vector (cases with a large PSD side: each costs an eigen-reference of seconds)"""
    case = sr.Case(pieces, seed=seed, **kw)
    dev = Dev(case.cones, case.s, case.z, factor_may_fail=any(p[0] == "psd" and p[2] == "late" for p in pieces))
    _check_ds(dev, case, where)
    _check_step(dev, case, where)
    _check_shift(dev, case, where, ((case.s - 2.0 * np.abs(case.s).max(), True, "outside"),) if one_shift else None)
    return case, dev


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sr.NN_SIZES)
def test_nonnegative(n):
    """sizes around one workgroup, and 2048 * 256 + 1: one row past the capped grid, so the stride loop runs"""
    _run([("nn", n)], f"nn {n}", seed=n)


@pytest.mark.parametrize("n", sr.SOC_DIMS)
def test_second_order(n):
    _run([("soc", n)], f"soc {n}", seed=n)


@pytest.mark.parametrize("n", (2, 5, 64, 129))
def test_second_order_near_boundary(n):
    _run([("soc", n, 1e-8)], f"soc {n} delta 1e-8", seed=100 + n)


@pytest.mark.parametrize("ncones", (1, 4, 5))
def test_second_order_wave_per_cone(ncones):
    """four cones to a workgroup: 1, exactly 4, and 5 (a second workgroup with one wave at work)"""
    _run([("soc", 5)] * ncones, f"{ncones} x soc 5", seed=ncones)


@pytest.mark.parametrize("k", sr.PSD_SIDES)
def test_psd(k):
    cls = cr.PSD_CLASSES[k % len(cr.PSD_CLASSES)]
    _run([("psd", k, cls, k % 2 == 0)], f"psd {k} {cls}", seed=k, one_shift=k > 17)


@pytest.mark.parametrize("cls", cr.PSD_CLASSES)
def test_psd_spectrum_classes(cls):
    _run([("psd", 7, cls, True)], f"psd 7 {cls} leaving", seed=3)
    case, dev = _run([("psd", 8, cls, False)], f"psd 8 {cls} staying", seed=4)
    # a step that stays in the cone does not limit: alpha_max itself
    assert dev.step_length(case.dz, case.ds, case.z, case.s) == 1.0


def test_psd_mixed_sides_and_an_empty_cone():
    _run([("psd", 3, "interior", True), ("psd", 48, "cond", True), ("psd", 0, "interior", True), ("psd", 1, "interior", True),
          ("psd", 17, "cluster", False)], "psd (3, 48, 0, 1, 17)", seed=6, one_shift=True)


def test_zero_cones_interleaved():
    """zero cones between the others, nonzero garbage in their rows of every input"""
    case, dev = _run([("zero", 3), ("nn", 5), ("zero", 2), ("soc", 6), ("zero", 1), ("psd", 3, "interior", True), ("zero", 4),
                      ("nn", 0), ("psd", 0, "interior", True)], "zero cones interleaved", seed=8)
    zero = _zero_rows(case.cones)
    # the step is not limited by them: a huge negative step in their rows changes nothing
    dz, ds = case.dz.copy(), case.ds.copy()
    dz[zero], ds[zero] = -1e30, -1e30
    assert dev.step_length(dz, ds, case.z, case.s) == dev.step_length(case.dz, case.ds, case.z, case.s)


def test_elementwise_grid_next_to_soc_workgroups():
    _run([("nn", 257)] + [("soc", 5)] * 5 + [("nn", 1)], "[NN(257), SOC(5) x 5, NN(1)]", seed=11)


def test_mixed_handle_step_length():
    """the result is the minimum of the per-cone references; alpha_max bitwise when nothing binds; the tau and the
    kappa limit binding"""
    pieces = [("nn", 40), ("zero", 2), ("soc", 7), ("soc", 3), ("psd", 5, "interior", True), ("nn", 3)]
    case = sr.Case(pieces, seed=21)
    dev = Dev(case.cones, case.s, case.z)
    got, ref = _check_step(dev, case, "mixed")
    assert ref.family not in ("one", "tau", "kappa") and got < 1.0            # a cone binds at the generated step
    # a tiny step: nothing binds
    small = sr.Case(pieces, seed=21, step_scale=1e-3)
    for scal, want in ((dict(), 1.0), (dict(dtau=-4.0, tau=2.0), 0.5), (dict(dkappa=-8.0, kappa=2.0, dtau=-1.0, tau=3.0), 0.25),
                       (dict(dtau=-3.0, tau=1.0), 1.0 / 3.0)):
        got, ref = _check_step(dev, small, f"mixed, tiny step {scal}", **scal)
        assert got == want and ref.value == want, (scal, got)
    # a positive-semidefinite / inside-the-cone step everywhere: exactly alpha_max
    assert dev.step_length(case.z, case.s, case.z, case.s) == 1.0


def test_soc_exact_branches_on_the_device():
    """every exact branch case of the host test, each as the z component of its own cone in ONE handle (s well inside,
    ds = 0), and each alone through a handle of its own"""
    cases = sr.soc_exact_cases()
    cones = [SecondOrderConeT(3) for _ in cases]
    inside = np.array([4.0, 1.0, 2.0])
    s = np.concatenate([inside for _ in cases])
    z_scale = np.concatenate([inside for _ in cases])                  # the scaling point; the step is taken from x below
    dev = Dev(cones, s, z_scale)
    x = np.concatenate([np.array(c[1]) for c in cases])
    y = np.concatenate([np.array(c[2]) for c in cases])
    zeros = np.zeros_like(x)
    for i, (name, xi, yi, want) in enumerate(cases):
        # only cone i steps; the others stand still at an interior point (y = 0: a == 0, no limit)
        xx, yy = s.copy(), zeros.copy()
        xx[3 * i:3 * i + 3], yy[3 * i:3 * i + 3] = xi, yi
        for got in (dev.step_length(yy, zeros, xx, s), dev.step_length(zeros, yy, s, xx)):     # as the z and as the s component
            if name == "d<0":
                # reachable by rounding alone (sr.soc_exact_cases): both branches are admissible and give 1/2 to rounding
                lim = sr.fold_min([sr.Limit(1.0), sr.soc_step_component(np.array(xi), np.array(yi))])
                assert lim.ambiguous and lim.ratio(got) <= 1.0, (name, got)
            else:
                assert got == want, (name, got, want)
    # all at once: the minimum is the c == 0, a < 0 case's 0
    assert dev.step_length(y, zeros, x, s) == 0.0


def test_shift_branches():
    """all three branches with margins and the shifted vector against the reference, and entries of -1e300 for the
    two-stage branch (applied as two shifts: their sum would return the -1e300 rows as exactly 0)"""
    pieces = [("nn", 300), ("zero", 3), ("soc", 9), ("psd", 4, "interior", True), ("soc", 2)]
    case = sr.Case(pieces, seed=31)
    dev = Dev(case.cones)                                              # shift_to_interior needs no scaling
    inside = np.abs(case.z) + 0.0
    inside[sr.unit_rows(case.cones)[0]] += 50.0                        # every margin >= ~50 with pos_margin small enough
    seen = _check_shift(dev, case, "shift", ((case.s - 2.0 * np.abs(case.s).max(), True, "outside"),
                                             (0.01 * case.z, False, "small"), (0.01 * case.z, True, "small"),
                                             (1e4 * inside, False, "good"), (1e4 * inside, True, "good")))
    assert seen == {"outside", "small", "good"}
    v = case.z.copy()
    v[[0, 7, 299]] = -1e300
    ref = sr.shift_ref(case.cones, v, False)
    assert ref["branch"] == "outside"
    mn, pos, got = dev.shift(v, False)
    assert mn == -1e300
    assert got[0] == got[7] == got[299] == ref["value"][0] > 0.0       # (x + 1e300) + target = target, not x + (1e300 + target) = 0
    _within({"shift": cr.ratio(got - ref["value"], ref["bound"])}, "shift -1e300")


def test_refusals():
    """the right code and nothing written: an exponential cone in the handle, a call before system.update, a
    deferred-status handle"""
    import torch
    from cuclarabel_amd import _lib

    def refused(dev, scaled_only=False):
        L, h = _lib.lib(), dev.ks._h
        m = dev.m
        o = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
        a = torch.ones(m, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        P = lambda t: t.data_ptr()
        alpha, mg = np.full(1, 7.0), np.full(2, 7.0)
        calls = [lambda: L.hipkkt_kkt_system_affine_ds(h, P(o)),
                 lambda: L.hipkkt_kkt_system_combined_ds(h, P(o), P(a), P(a), 0.1, 1.0),
                 lambda: L.hipkkt_kkt_system_step_length(h, P(a), P(a), P(a), P(a), 1.0, 1.0, 1.0, 1.0, _lib.ptr(alpha))]
        if not scaled_only:
            calls.append(lambda: L.hipkkt_kkt_system_shift_to_interior(h, P(o), 1, _lib.ptr(mg)))
        for call in calls:
            assert call() == -1, L.hipkkt_last_error()                 # HIPKKT_ERR_ARG
            assert L.hipkkt_last_error()
        dev.ks.synchronize()
        assert np.all(o.cpu().numpy() == 7.0) and alpha[0] == 7.0 and np.all(mg == 7.0), "a refused call wrote something"

    refused(Dev([NonnegativeConeT(3), ExponentialConeT(), SecondOrderConeT(3)]))
    refused(Dev([NonnegativeConeT(3), SecondOrderConeT(3), ZeroConeT(1), PSDTriangleConeT(2)]), scaled_only=True)   # before update
    case = sr.Case([("nn", 3), ("soc", 3)], seed=2)
    dev = Dev(case.cones, case.s, case.z)
    dev.ks.set_deferred_status(True)
    refused(dev)
    dev.ks.set_deferred_status(False)
    assert dev.ks.deferred_status() in (0, 1, 2)
    assert dev.step_length(case.dz, case.ds, case.z, case.s) > 0.0     # and works again afterwards
