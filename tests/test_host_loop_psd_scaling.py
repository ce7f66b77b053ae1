"""`ipm.solve` at level B with ONE PSD scaling per iteration: a backend that offers psd_scaling() hands the host's PSD cone
objects the (R, Rinv, lambda) its K was built from, as the level-C branch of the loop does with the device's.

On small_mixed(socs=(5,), psds=(20,)) the plain loop over the CPU oracle -- K from the oracle's R, ds = -(Hs dz + ...)
from numpy's -- ends NUMERICAL_ERROR after 16 iterations at 22.39318308 (printed here, not asserted: it is a defect of
that pairing, not a property to keep); with the hook it ends SOLVED in 12.  A backend without the method is not asked."""
import numpy as np

from cuclarabel_amd import ipm, problems
from tests.ipm_backends import OracleBackend


class _Hooked(OracleBackend):
    calls = 0

    def psd_scaling(self):
        type(self).calls += 1
        return self.o.psd_scaling()


def test_the_host_loop_adopts_the_backends_psd_scaling_and_converges():
    pb = problems.small_mixed(socs=(5,), psds=(20,))
    plain = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, OracleBackend(pb.P, pb.A, pb.cones))
    print(f"\nplain oracle loop: {plain.status} after {plain.iterations} iterations at {plain.obj_val!r}")
    _Hooked.calls = 0
    res = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, _Hooked(pb.P, pb.A, pb.cones))
    print(f"with psd_scaling(): {res.status} after {res.iterations} iterations at {res.obj_val!r}")
    assert res.status == ipm.SOLVED
    assert _Hooked.calls == res.iterations                             # once per kkt_update! from (s, z)
    st = ipm.IPMSettings()
    h = res.history[-1]
    assert h["pres"] < st.tol_feas and h["dres"] < st.tol_feas
    assert abs(res.obj_val - res.obj_val_dual) <= max(st.tol_gap_abs, st.tol_gap_rel * max(1.0, abs(res.obj_val)))
    # the two loops reach the same optimum as far as the plain one gets (its last iterates lose primal feasibility)
    assert abs(plain.obj_val - res.obj_val) <= 1e-6 * max(1.0, abs(res.obj_val))


def test_a_problem_without_psd_cones_never_asks():
    pb = problems.small_mixed(psds=())
    _Hooked.calls = 0
    res = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, _Hooked(pb.P, pb.A, pb.cones))
    assert res.status == ipm.SOLVED and _Hooked.calls == 0
    assert np.all(np.isfinite(res.x))
