"""Why a stack of independent problems needs scalars of its own per member, pinned on the CPU oracle: `ipm.solve` on a
block-diagonal stack treats it as ONE conic problem -- one step length, one mu, one homogenising tau, one termination
test, one status -- so an infeasible member takes the whole stack with it.  tests/test_gpu_batch_ipm.py contrasts
`ipm_device.solve_device_batch` with this: there every member ends with its own status."""
import numpy as np
import scipy.sparse as sp

from cuclarabel_amd import ipm
from tests.golden.reference_fixtures import ALL
from tests.ipm_backends import OracleBackend


def _alone(name):
    P, q, A, b, cones, _ = ALL[name]()
    return ipm.solve(P, q, A, b, cones, OracleBackend(P, A, cones))


def _stacked(names):
    parts = [ALL[k]() for k in names]
    P = sp.block_diag([sp.csc_matrix(p[0]) for p in parts], format="csc")
    A = sp.block_diag([sp.csc_matrix(p[2]) for p in parts], format="csc")
    q, b = np.concatenate([p[1] for p in parts]), np.concatenate([p[3] for p in parts])
    cones = [c for p in parts for c in p[4]]
    return ipm.solve(P, q, A, b, cones, OracleBackend(P, A, cones))


def test_one_infeasible_member_takes_the_joint_loop_with_it():
    names = ["basic_qp", "basic_socp", "basic_qp_priminf"]
    alone = [_alone(k) for k in names]
    assert [r.status for r in alone] == ["SOLVED", "SOLVED", "PRIMAL_INFEASIBLE"]
    assert [r.iterations for r in alone] == [8, 7, 5]
    res = _stacked(names)
    assert res.status == "PRIMAL_INFEASIBLE"
    assert res.iterations == 6


def test_a_dual_infeasible_member_does_the_same():
    assert [_alone(k).status for k in ("basic_qp", "basic_lp_dualinf")] == ["SOLVED", "DUAL_INFEASIBLE"]
    assert _stacked(["basic_qp", "basic_lp_dualinf"]).status == "DUAL_INFEASIBLE"
