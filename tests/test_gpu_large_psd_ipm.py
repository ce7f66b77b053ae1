"""`ipm_device.solve_device*` on problems with PSD cones of side 49 ... 96: the entry points opt the handle in themselves
(hipkkt_kkt_enable_large_psd), the iterate stays in HBM, and every cone operation between the solves runs in the
big-class kernels.  Known answers (the largest eigenvalue of a seeded matrix as an SDP), parity with `ipm.solve` on the
CPU oracle at sides (49, 50), and at sides (64, 65, 96), where the oracle's factorisation would take minutes, the
solution's own optimality conditions."""
import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd import ipm, problems
from cuclarabel_amd.cones import PSDTriangleConeT
from cuclarabel_amd.ipm_device import solve_device, solve_device_nonsymmetric
from tests.ipm_backends import OracleBackend
from tests.test_gpu_ipm_device_nonsym import _resident

pytestmark = pytest.mark.gpu

ST = ipm.IPMSettings()            # the loop's termination tolerances: tol_gap_abs = tol_gap_rel = tol_feas = 1e-8


def _backend_hook(seen):
    """an inspect hook that checks residency and keeps the loop's backend (its handle holds P, A, q, b)"""
    def inspect(tensors, backend):
        for name, t in tensors.items():
            assert t.is_cuda and t.dtype.is_floating_point, f"{name} is not a device tensor"
        seen["backend"] = backend
        seen["calls"] = seen.get("calls", 0) + 1
    return inspect


def _termination(pb, res, backend):
    """The quantities of the loop's own termination test (ipm_device._solve, info_update!: 2-norms of the residuals over
    max(1, |b|_inf + |x| + |s|) and max(1, |q|_inf + |x| + |z|), the absolute and the relative gap) at the RETURNED
    point, tau = 1: the twelve scalars from hipkkt_kkt_system_residuals on the loop's own handle, and the same from
    numpy beside them -> (device dict, numpy dict)."""
    import torch
    system = backend.system
    dev = system._devstr
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    new = lambda k: torch.zeros(max(k, 1), dtype=torch.float64, device=dev)
    n, m = len(res.x), len(res.s)
    x, s, z = up(res.x), up(res.s), up(res.z)
    rx, rz, rxi, rzi, Px = new(n), new(m), new(n), new(m), new(n)
    torch.cuda.synchronize()
    P_ = lambda t: t.data_ptr()
    dev12 = system.residuals_dev(P_(x), P_(s), P_(z), 1.0, P_(rx), P_(rz), P_(rxi), P_(rzi), P_(Px)).tolist()
    P = pb.P + sp.triu(pb.P, 1).T
    xh, sh, zh = res.x, res.s, res.z
    Pxh = P @ xh
    nrm = np.linalg.norm
    np12 = [pb.q @ xh, pb.b @ zh, sh @ zh, xh @ Pxh, nrm(xh), nrm(zh), nrm(sh), 0.0, 0.0, 0.0,
            nrm(pb.A @ xh + sh - pb.b), nrm(-(pb.A.T @ zh) - Pxh - pb.q)]
    normq, normb = np.abs(pb.q).max(), np.abs(pb.b).max()
    out = []
    for qx, bz, sz, xPx, nx, nz, ns, _a, _b, _c, n_rz, n_rx in (dev12, np12):
        cp, cd = qx + xPx / 2, -bz - xPx / 2
        out.append(dict(res_p=n_rz / max(1.0, normb + nx + ns), res_d=n_rx / max(1.0, normq + nx + nz), gap_abs=abs(cp - cd),
                        gap_rel=abs(cp - cd) / max(1.0, min(abs(cp), abs(cd))), sz=sz, nx=nx, nz=nz, ns=ns, n_rz=n_rz,
                        n_rx=n_rx, obj=min(abs(cp), abs(cd))))
    return out


def _assert_terminated(pb, res, backend, where):
    """the loop's termination test, at its tolerances, on both evaluations; s'z = gap - x'rd - z'rp at a point with
    residuals rd, rp, so |s'z| <= gap + |x| |rd| + |z| |rp|, each factor at its tolerance"""
    d, h = _termination(pb, res, backend)
    print(f"{where}: device {d}\n{where}: numpy {h}")
    for c in (d, h):
        assert c["res_p"] < ST.tol_feas and c["res_d"] < ST.tol_feas, (where, c)
        assert c["gap_abs"] < ST.tol_gap_abs or c["gap_rel"] < ST.tol_gap_rel, (where, c)
        gap_tol = max(ST.tol_gap_abs, ST.tol_gap_rel * max(1.0, c["obj"]))
        assert abs(c["sz"]) <= gap_tol + c["nx"] * c["n_rx"] + c["nz"] * c["n_rz"], (where, c)


class OracleWithItsScaling(OracleBackend):
    """the CPU oracle as ipm.solve's backend, offering the scaling its K was built from (ipm.solve: psd_scaling)"""

    def psd_scaling(self):
        return self.o.psd_scaling()


def _sym(seed, k):
    G = np.random.default_rng(seed).standard_normal((k, k))
    return (G + G.T) / 2


@pytest.mark.parametrize("plumbing", ["torch", "device"])
@pytest.mark.parametrize("k", [49, 65, 96])
def test_largest_eigenvalue_is_found(k, plumbing):
    C = _sym(k, k)
    pb = problems.max_eigenvalue_sdp(C)
    seen, kept = [], {}
    resident, hook = _resident(seen), _backend_hook(kept)

    def inspect(tensors, backend):
        resident(tensors, backend)
        hook(tensors, backend)

    res = solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, inspect=inspect, plumbing=plumbing)
    want = np.linalg.eigvalsh(C)[-1]
    print(f"side {k} {plumbing}: {res.status} in {res.iterations} iterations, t = {res.x[0]!r}, lambda_max = {want!r}")
    assert res.status == ipm.SOLVED
    # the objective is t: to the gap tolerance of the loop
    tol = max(ST.tol_gap_abs, ST.tol_gap_rel * max(1.0, abs(want)))
    assert abs(res.x[0] - want) <= tol
    assert abs(res.obj_val - want) <= tol and abs(res.obj_val_dual - want) <= tol
    _assert_terminated(pb, res, kept["backend"], f"side {k} {plumbing}")
    assert len(seen) >= res.iterations + 1                             # every vector of every iteration: a device tensor


def test_parity_with_the_host_loop_on_the_oracle_at_sides_49_and_50():
    """ipm.solve over the CPU oracle, with the host's PSD cone objects on the oracle's own (R, Rinv, lambda): the backend
    offers psd_scaling().  Without that the host loop runs on two scalings per iteration -- K from the oracle's R, ds from
    numpy's -- and at these sides ends NUMERICAL_ERROR after 21 iterations, its primal residual growing from 8.6e-9 at
    iteration 15 to 1.7e-3 while the gap falls to 5e-11 (the same at n = 60, 120, 200, 600 and other seeds); with it, SOLVED
    in 17 iterations at -25.775843785992, where the device loop ends in 17 at -25.775843785995, x within 4.1e-9."""
    pb = problems.sdp_large_cones(sides=(49, 50), n=30)
    res = solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones)
    ref = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, OracleWithItsScaling(pb.P, pb.A, pb.cones))
    print(f"\niterations: device loop {res.iterations}, oracle loop {ref.iterations}; status {res.status} / {ref.status}; "
          f"objective {res.obj_val!r} / {ref.obj_val!r}; |x - x_ref| / max(1, |x_ref|) = "
          f"{np.linalg.norm(res.x - ref.x) / max(1.0, np.linalg.norm(ref.x)):.3e}")
    assert res.status == ref.status == ipm.SOLVED
    assert abs(res.iterations - ref.iterations) <= 1
    # the tolerances of test_gpu_ipm_device_loop.test_same_answer_as_the_host_vector_loop
    assert np.linalg.norm(res.x - ref.x) <= 1e-7 * max(1.0, np.linalg.norm(ref.x))
    assert abs(res.obj_val - ref.obj_val) <= 1e-7 * max(1.0, abs(ref.obj_val))


def _psd_margins(pb, res):
    """the smallest eigenvalue of mat(s) and of mat(z) over the PSD cones, relative to max(1, |v|_inf)"""
    out, off = {}, 0
    for c in pb.cones:
        if isinstance(c, PSDTriangleConeT):
            for name, v in (("s", res.s), ("z", res.z)):
                M = problems.svec_to_mat(v[off:off + c.numel], c.dim)
                e = np.linalg.eigvalsh(M)[0] / max(1.0, np.abs(v).max())
                out[name] = min(out.get(name, np.inf), e)
        off += c.numel
    return out


def test_sides_64_65_96_by_their_own_optimality_conditions(monkeypatch):
    from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem
    pb = problems.sdp_large_cones(sides=(64, 65, 96), n=40)
    seen = {}
    # every route by which an Hs block would cross the bus is counted: the caller's Hs into the handle (level B and C),
    # the handle's Hs back out
    crossed = dict(kktsolver_update=0, update_cones=0, get_Hs=0)
    for cls, name in ((HipKKTSolver, "kktsolver_update"), (HipKKTSystem, "update_cones"), (HipKKTSolver, "get_Hs")):
        def counted(self, *a, _f=getattr(cls, name), _n=name, **kw):
            crossed[_n] += 1
            return _f(self, *a, **kw)
        monkeypatch.setattr(cls, name, counted)
    res = solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, inspect=_backend_hook(seen))
    # the symmetric start's identity scaling goes over once, before the first iteration; after that none
    assert res.iterations >= 2 and crossed["kktsolver_update"] <= 1 and crossed["update_cones"] == crossed["get_Hs"] == 0, crossed
    print(f"\n(64, 65, 96): {res.status} in {res.iterations} iterations")
    assert res.status == ipm.SOLVED
    _assert_terminated(pb, res, seen["backend"], "(64, 65, 96)")
    margins = _psd_margins(pb, res)
    print(f"(64, 65, 96): smallest eigenvalues / max(1, |v|) {margins}")
    assert margins["s"] >= -ST.tol_feas and margins["z"] >= -ST.tol_feas
    assert seen["backend"].ks.fallbacks == (0, 0)


def test_a_mixed_list_with_an_exponential_cone_solves():
    """[Zero, NN, SOC, PSD(20)] + [PSD(65)] + [Zero, Exp x 3] as one block-diagonal problem through the non-symmetric loop"""
    blocks = [problems.small_mixed(socs=(5,), psds=(20,)), problems.sdp_large_cones(sides=(65,), n=20),
              problems.entropy_maximization(3, nrows=1)]
    pb = problems.block_diagonal(blocks)
    seen = {}
    res = solve_device_nonsymmetric(pb.P, pb.q, pb.A, pb.b, pb.cones, inspect=_backend_hook(seen))
    print(f"\nmixed: {res.status} in {res.iterations} iterations, obj {res.obj_val!r}")
    assert res.status == ipm.SOLVED
    # independent of the code under test: the combined solution's own conditions at the loop's tolerances ...
    _assert_terminated(pb, res, seen["backend"], "mixed")
    margins = _psd_margins(pb, res)
    assert margins["s"] >= -ST.tol_feas and margins["z"] >= -ST.tol_feas
    # ... and the first block's optimum from ipm.solve on the CPU oracle (the blocks are independent, so a block's part
    # of the objective is that block's optimum; both loops stop at the gap tolerance, and the two gaps add)
    off = 0
    for i, b in enumerate(blocks):
        xb = res.x[off:off + b.n]
        off += b.n
        if i != 0:
            continue                               # (the PSD(65) block would take the oracle minutes; the exponential
        #                                            block's answer is held by the combined conditions above)
        Pb = b.P + sp.triu(b.P, 1).T
        got = 0.5 * xb @ (Pb @ xb) + b.q @ xb
        ref = ipm.solve(b.P, b.q, b.A, b.b, b.cones, OracleWithItsScaling(b.P, b.A, b.cones))
        assert ref.status == ipm.SOLVED
        print(f"mixed: block {i} objective {got!r}, oracle loop {ref.obj_val!r}")
        assert abs(got - ref.obj_val) <= 2 * max(ST.tol_gap_abs, ST.tol_gap_rel * max(1.0, abs(ref.obj_val), abs(res.obj_val)))

