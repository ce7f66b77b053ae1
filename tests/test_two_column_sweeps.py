"""Two-column sweeps against one-column sweeps.

With two right-hand sides the block-class hops of the sweeps (k_top_solve, k_top_solve_sliced's ordinary fronts, the
chained and per-level block kernels) keep their LDS vectors interleaved and walk every matrix item once for both
columns.  Per column the order of the operations is the one-column kernels', so column j of a 2-column
`kktsolver_solve_multi_dev` must end BIT FOR BIT where the single solve of the same right-hand side ends (the parent of
the commit that introduced the shared walk, d290291, agrees bit for bit on the same inputs: measured with this file).
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_SCRIPT = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
from cuclarabel_amd import _lib, problems
from cuclarabel_amd.kktsolver import HipKKTSolver
assert _lib.lib().hipkkt_available() == 1, "no gfx950 device visible"
pb = {maker}
ks = HipKKTSolver(pb.P, pb.A, pb.cones)
assert ks.kktsolver_update_from_sz(pb.s0, pb.z0)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(2024)
for rep in range(2):
    RX, RZ = rng.standard_normal((pb.n, 2)), rng.standard_normal((pb.m, 2))
    if rep == 1:
        RX[:, 1] *= 1e-6                       # columns of very different size share nothing but the matrix entries
        RZ[:, 1] *= 1e-6
    drx = torch.from_numpy(np.ascontiguousarray(RX.T)).to(dev)
    drz = torch.from_numpy(np.ascontiguousarray(RZ.T)).to(dev)
    dlx = torch.zeros(2, pb.n, dtype=torch.float64, device=dev)
    dlz = torch.zeros(2, pb.m, dtype=torch.float64, device=dev)
    ok, ir = ks.kktsolver_solve_multi_dev(2, drx.data_ptr(), drz.data_ptr(), dlx.data_ptr(), dlz.data_ptr())
    assert ok
    LX, LZ = dlx.cpu().numpy(), dlz.cpu().numpy()
    for j in range(2):
        ks.kktsolver_setrhs(RX[:, j], RZ[:, j])
        x, z = np.zeros(pb.n), np.zeros(pb.m)
        assert ks.kktsolver_solve(x, z)
        print("rep", rep, "col", j, "max |2col - 1col|", max(np.abs(LX[j] - x).max(), np.abs(LZ[j] - z).max()),
              "rounds", int(ir[j]), ks.last_ir_iterations)
        np.testing.assert_array_equal(LX[j], x)
        np.testing.assert_array_equal(LZ[j], z)
        assert int(ir[j]) == ks.last_ir_iterations
assert ks.fallbacks == (0, 0), ks.fallbacks
print("TWO COLUMN OK")
"""


def _schedule(stderr):
    from tests.test_gpu_parity import _schedule_line
    return _schedule_line(stderr)


@pytest.mark.parametrize("name,maker,env,sliced", [
    ("cfg2_reduced", "problems.config2(n=20000)", {}, False),
    ("cfg2_full", "problems.config2()", {}, False),
    ("cfg5_reduced_sliced", "problems.config5(n=120, npsd=6, psd_dim=8, nsoc=4, soc_dim=12)",
     {"HIPKKT_SOLVE_SLICE_KB": "4", "HIPKKT_SOLVE_SLICE_FROM": "12"}, True),
])
def test_two_column_solve_equals_single_column_solves(name, maker, env, sliced):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _SCRIPT.format(root=root, maker=maker)],
                       env=dict(os.environ, HIPKKT_VERBOSE="1", **env), cwd=root, capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TWO COLUMN OK" in r.stdout and "gave up" not in r.stderr, r.stderr
    sched = _schedule(r.stderr)
    assert sched["top_fronts"] > 0, sched                      # the persistent kernel took the top of the tree
    if sliced:
        assert sched["top_tasks"] > sched["top_fronts"], sched  # (front, slice) tasks: k_top_solve_sliced was selected
