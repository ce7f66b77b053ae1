"""The interior-point loop of `ipm.solve` with the iterate resident in HBM.

`solve_device` is `ipm.solve` for symmetric cone lists (zero, nonnegative, second-order, PSD side <= 48), line for line,
with x, s, z, the steps, the right-hand sides and the residual vectors held as torch device tensors for the whole
solve.  Level C of the C ABI does everything KKT-shaped (init, initial point, kkt_update!, the two kkt_solve!) and --
through hipkkt_kkt_system_affine_ds / _combined_ds / _step_length / _shift_to_interior -- everything cone-shaped; torch
does the plumbing between them (the residual mat-vecs with fp64 CSR tensors, dots, norms, axpy) -- or, with
plumbing="device", the library does that too (hipkkt_kkt_system_residuals / _combined_rhs / _add_step).  After
`system.init` nothing of length n or m crosses the bus until the final solution: per iteration only scalars do (one
batch of dot products and norms, alpha twice, (dtau, dkappa) twice, the solves' status).

    residuals, mu, termination, sigma = (1 - alpha)^3, m = alpha on the first iteration and 1 afterwards,
    post-processing                       as ipm.solve (solver.jl:189-380, info.jl, variables.jl:107-190)

One difference in bookkeeping: a cone point that is not interior is reported by kkt_update! itself (the device scales
the cones inside it), so `iterations` counts that last, failed iteration, where `ipm.solve` with host cones stops one
line earlier.  The status is NUMERICAL_ERROR either way.

`solve_device_nonsymmetric` is the same loop for cone lists that hold exponential or power cones (the non-symmetric
branch of `ipm.solve`): the unit start, `set_nonsymmetric_scaling(strategy, mu)` before every update, the three strategy
checkpoints, and the barrier line search under the dual strategy -- the cone operations through
hipkkt_kkt_system_unit_initialization / _affine_ds_ns / _combined_ds_ns / _step_length_ns / _barrier.  Per iteration
the same scalars cross the bus, plus two per barrier evaluation.  There the bookkeeping difference has one more
consequence: kkt_update! does not say WHY it failed, so a failed scaling under the primal-dual strategy passes through
the numerical-error checkpoint (one more iteration under the dual strategy, where it fails again) before the loop
ends with NUMERICAL_ERROR.

`solve_device_genpow` is that loop again for cone lists that hold generalized power cones (any of the other six kinds
beside them), through hipkkt_kkt_system_unit_initialization_gp / _affine_ds_gp / _combined_ds_gp / _step_length_gp /
_barrier_gp.  A generalized power cone has degree dim1 + 1 and dual scaling only; the loop still starts under
PRIMAL_DUAL, as `ipm.solve` does for such lists, so that the two are comparable.  The combined d.s uses the gradient the
device's own scaling kernel stored, so nothing of the scaling is read back.
"""
import warnings

import numpy as np
import scipy.sparse as sp

from .cones import (ZeroConeT, NonnegativeConeT, SecondOrderConeT, PSDTriangleConeT, ExponentialConeT, PowerConeT,
                    GenPowerConeT)
from .ipm import (IPMSettings, IPMResult, HipSystemBackend, SOLVED, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE, MAX_ITERATIONS,
                  NUMERICAL_ERROR, INSUFFICIENT_PROGRESS, UNSOLVED, ALMOST_SOLVED, PRIMAL_DUAL, DUAL, _logsafe)

PSD_MAX_SIDE = 48          # kPsdMaxDim of the device kernels: the all-in-LDS class, what a handle covers by default
PSD_MAX_SIDE_LARGE = 96    # kPsdBigMaxDim = HIPKKT_PSD_MAX_SIDE_LARGE: with hipkkt_kkt_enable_large_psd, which the entry
#                            points below call themselves for a list that holds a side above PSD_MAX_SIDE


class _Csr:
    """y = M x on the device for a scipy matrix: an fp64 CSR tensor; where the installed torch has no fp64 CSR mat-vec
    on the GPU, the COO product written with index_add_ (mode tells which)."""

    def __init__(self, M, dev):
        import torch
        M = sp.csr_matrix(M)
        M.sort_indices()
        self.shape = M.shape
        self.torch = torch
        val = torch.from_numpy(np.ascontiguousarray(M.data, dtype=np.float64)).to(dev)
        self.mode = "csr"
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")          # ("sparse CSR tensor support is in beta state")
                self.M = torch.sparse_csr_tensor(torch.from_numpy(M.indptr.astype(np.int64)).to(dev),
                                                 torch.from_numpy(M.indices.astype(np.int64)).to(dev), val, size=M.shape)
            self.M @ torch.zeros(M.shape[1], dtype=torch.float64, device=dev)
        except (RuntimeError, NotImplementedError, ValueError, IndexError):
            self.mode = "coo"
            coo = M.tocoo()
            self.row = torch.from_numpy(coo.row.astype(np.int64)).to(dev)
            self.col = torch.from_numpy(coo.col.astype(np.int64)).to(dev)
            self.val = torch.from_numpy(np.ascontiguousarray(coo.data, dtype=np.float64)).to(dev)
        self.dev = dev

    def mv(self, x):
        if self.mode == "csr":
            return self.M @ x
        y = self.torch.zeros(self.shape[0], dtype=self.torch.float64, device=self.dev)
        return y.index_add_(0, self.row, self.val * x[self.col])


_SYMMETRIC = (ZeroConeT, NonnegativeConeT, SecondOrderConeT, PSDTriangleConeT)
_NONSYMMETRIC = _SYMMETRIC + (ExponentialConeT, PowerConeT)


def _check_cones(who, cone_specs, allowed, hint):
    """The entry points' argument check -> the cone list.  hint: the refusal of a kind outside `allowed`, with {} for
    that kind's name."""
    cone_specs = list(cone_specs)
    for c in cone_specs:
        if not isinstance(c, allowed):
            raise ValueError(hint.format(type(c).__name__))
        if isinstance(c, PSDTriangleConeT) and c.dim > PSD_MAX_SIDE_LARGE:
            raise ValueError(f"{who} covers PSD cones up to side {PSD_MAX_SIDE_LARGE}")
    return cone_specs


def solve_device(P, q, A, b, cone_specs, settings=None, inspect=None, plumbing="torch"):
    """Clarabel.solve! restated with device-resident vectors -> IPMResult (numpy x, z, s).

    inspect (optional): called once per iteration with (dict of the tensors the loop holds, the HipSystemBackend) --
    for tests that check residency.
    plumbing: "torch" (the default) -- the residual mat-vecs, dots, norms and axpys between the library's calls are torch
    expressions over fp64 CSR copies of P, A and A'; "device" -- they are the library's own
    hipkkt_kkt_system_residuals / _combined_rhs / _add_step over the P, A the handle already holds: no second copy of the
    matrices, and torch only allocates (and clones the previous iterate)."""
    if plumbing not in ("torch", "device"):
        raise ValueError(f"plumbing must be 'torch' or 'device', got {plumbing!r}")
    cone_specs = _check_cones("solve_device", cone_specs, _SYMMETRIC,
                              "solve_device covers the symmetric cones only (zero, nonnegative, second-order, PSD); "
                              "got {}: use solve_device_nonsymmetric for exponential and power cones, "
                              "solve_device_genpow for generalized power cones")
    return _solve(P, q, A, b, cone_specs, settings, inspect, plumbing == "device", False)


def solve_device_nonsymmetric(P, q, A, b, cone_specs, settings=None, inspect=None, plumbing="device"):
    """`solve_device` for cone lists with exponential and power cones among the symmetric ones (any order): the
    non-symmetric branch of Clarabel.solve! with device-resident vectors -> IPMResult.  Generalized power cones are not
    covered (use solve_device_genpow).  `inspect` and `plumbing` as in solve_device; settings.min_terminate_step_length must be
    positive and linesearch_backtrack_step lie in (0, 1) (the device's backtracking search refuses anything else)."""
    if plumbing not in ("torch", "device"):
        raise ValueError(f"plumbing must be 'torch' or 'device', got {plumbing!r}")
    cone_specs = _check_cones("solve_device_nonsymmetric", cone_specs, _NONSYMMETRIC,
                              "solve_device_nonsymmetric covers zero, nonnegative, second-order, PSD, exponential and power "
                              "cones; got {}: use solve_device_genpow")
    return _solve(P, q, A, b, cone_specs, settings, inspect, plumbing == "device", True)


def solve_device_genpow(P, q, A, b, cone_specs, settings=None, inspect=None, plumbing="device"):
    """`solve_device_nonsymmetric` for cone lists that hold a generalized power cone, with any of the other six kinds
    beside it (any order) -> IPMResult.  The cone operations go through the library's _gp entry points; `inspect`,
    `plumbing` and the two settings constraints as in solve_device_nonsymmetric."""
    if plumbing not in ("torch", "device"):
        raise ValueError(f"plumbing must be 'torch' or 'device', got {plumbing!r}")
    cone_specs = _check_cones("solve_device_genpow", cone_specs, _NONSYMMETRIC + (GenPowerConeT,),
                              "solve_device_genpow: unknown cone type {}")
    return _solve(P, q, A, b, cone_specs, settings, inspect, plumbing == "device", True, True)


def solve_device_batch(problems, settings=None, inspect=None):
    """A batch of INDEPENDENT problems solved as one block-diagonal stack on one handle -> list of IPMResult, one per
    member: its own status, iteration count, history, x, z, s and objectives.

    problems: list of (P, q, A, b, cone_specs); symmetric cones with PSD side <= 48 only (anything else is refused with
    ValueError before a handle is built).

    The loop is `solve_device(plumbing="device")` on the stacked handle with every scalar -- tau, kappa, mu, sigma,
    alpha, the residual norms, (dtau, dkappa) -- a numpy array over the members, through the library's _batch entry
    points (hipkkt_kkt_system_set_problems and the seven calls behind it); every line of the termination logic
    (info.jl:65-120, :196-211, :270-330) is applied per member.  A member that has reached a final status is FROZEN: its
    alpha is 0 from then on (its rows are not written), its status, iterate and history no longer change, and its result
    is the iterate it ended on; restoring the previous iterate on INSUFFICIENT_PROGRESS copies back that member's rows
    only.  From the iteration after it ended, its block of K is scaled at the member's start point and its rows of the
    right-hand sides are zero, so that a finished member costs the members still running nothing of their solves'
    refinement (see the loop).  The loop ends when no member is UNSOLVED; max_iter counts per member (all members start together, so that is
    the loop's own count).  What stays joint, because the factorisation is one: a failed kkt_update! or solve ends every
    member still UNSOLVED with NUMERICAL_ERROR; the static regulariser and the refinement's stopping rule see the whole
    stack; `ir_iterations` of every result is the stack's total.  The symmetric start takes the handle's LP / QP branch
    (kktsystem.jl:95-143), which is decided by nnz(P) of the STACK: a batch that mixes members with and without a P starts
    its LP members from the QP start (another interior point; the answers agree to the tolerances, the iteration counts
    need not).  solve_device_batch_isolated is this loop with the regulariser and a failure's status per member.

    inspect (optional): called once per iteration with (dict of the tensors the loop holds, the HipSystemBackend)."""
    return _solve_batch("solve_device_batch", problems, settings, inspect, False)


def solve_device_batch_refined(problems, settings=None, inspect=None):
    """solve_device_batch with the refinement's accept / stop rule applied per member
    (hipkkt_kkt_system_set_member_refinement): the loop, the freeze of finished members included, is the same; inside
    every solve each member is refined by the reference's rule on its own rows, so that a member whose rows cannot be
    refined further no longer ends the refinement of the others.  What stays joint: the status of kkt_update! and of a
    solve, and the static regulariser.  `kkt_ir_rounds` of every result is that member's own total over the loop's
    solves."""
    return _solve_batch("solve_device_batch_refined", problems, settings, inspect, True)


def solve_device_batch_isolated(problems, settings=None, inspect=None, member_refinement=True):
    """solve_device_batch in which a member that fails ends ALONE (hipkkt_kkt_system_set_member_status): every member is
    regularised by eps_b = c0 + c1 max |K_ii| over its own rows of K, as it would be alone, and

      - a failed kkt_update! reads the members' words: every active member whose cone scaling failed or whose block
        produced a non-finite pivot ends with NUMERICAL_ERROR at that iteration and is frozen like a finished member (its
        block scaled at its start point, its right-hand-side rows zero, alpha 0); the update is repeated in the same
        iteration -- each repeat removes at least one member, so at most nb repeats.  If the words name no active member
        the members still running end together, as in solve_device_batch;
      - member_refinement=True (hipkkt_kkt_system_set_member_refinement as well): a failed solve reads the members' bad
        flags; the flagged members end with NUMERICAL_ERROR and are frozen, the others carry on with the step the solve
        produced for them (the member rule finishes their rows before the solve reports its failure);
      - member_refinement=False: a failed solve stays JOINT and ends every member still running -- the joint rule's one
        non-finite norm cannot be attributed to a member.

    A member with a non-finite entry in P, q, A or b is refused with ValueError naming it before a handle is built: its
    block could never be factorised.  Still joint: the LP / QP branch of the symmetric start, decided by nnz(P) of the
    stack.  Without a failure the loop is solve_device_batch's (member_refinement=False) or solve_device_batch_refined's
    (True) under the members' own regularisers."""
    return _solve_batch("solve_device_batch_isolated", problems, settings, inspect, bool(member_refinement), True)


def _solve_batch(who, problems, settings, inspect, member_refinement, isolate=False, equilibrations=None):
    """What solve_device_batch, solve_device_batch_refined and solve_device_batch_isolated share: the set-up, then the loop
    from the default start.  equilibrations: see _setup_batch."""
    return _loop_batch(_setup_batch(who, problems, settings, member_refinement, isolate, equilibrations), inspect)


class _BatchSetup:
    """Everything a batch solve needs that does not depend on the iterate: the stacked handle with its partition and
    member modes, the loop's device tensors, the members' offsets and degrees.  Built once by _setup_batch; _loop_batch runs
    on it any number of times (solver_device.DeviceBatchSolver)."""


def _check_batch(who, problems, isolate):
    """The batch entry points' argument check -> the members as (triu P, q, A, b, cone list); refusals are ValueError,
    raised before a handle is built."""
    problems = list(problems)
    if not problems:
        raise ValueError(f"{who} needs at least one problem")
    members = []
    for (P, q, A, b, cone_specs) in problems:
        cone_specs = _check_cones(who, cone_specs, _SYMMETRIC,
                                  who + " covers the symmetric cones only (zero, nonnegative, second-order, PSD); got {}")
        if any(isinstance(c, PSDTriangleConeT) and c.dim > PSD_MAX_SIDE for c in cone_specs):
            raise ValueError(f"{who} covers PSD cones up to side {PSD_MAX_SIDE}")
        Pt = sp.triu(sp.csc_matrix(P), format="csc")
        members.append((Pt, np.asarray(q, float), sp.csc_matrix(A), np.asarray(b, float), cone_specs))
        if isolate:
            for name, values in (("P", Pt.data), ("q", members[-1][1]), ("A", members[-1][2].data), ("b", members[-1][3])):
                if not np.all(np.isfinite(values)):
                    raise ValueError(f"{who}: member {len(members) - 1} has a non-finite entry in {name}")
    return members


def _setup_batch(who, problems, settings, member_refinement, isolate=False, equilibrations=None):
    """equilibrations: None -- the stack is built from the members' data as given and the loop knows no equilibration, as
    it always did; or a list of `equilibrate.Equilibration`, one per member (solver_device.DeviceBatchSolver) -- the
    handle is built from every member's data scaled by its own (d, e, c_b) in the update kernels' order
    (solver_device.scale_data), the scalings go onto the handle (hipkkt_kkt_system_set_equilibration_batch) and the loop
    takes the equilibrated path of _loop per member."""
    import torch
    members = _check_batch(who, problems, isolate)
    c = _BatchSetup()
    c.st = settings or IPMSettings()
    c.member_refinement, c.isolate = member_refinement, isolate
    c.members = members
    c.nb = nb = len(members)
    if equilibrations is not None:
        from .solver_device import scale_data
        equilibrations = list(equilibrations)
        if len(equilibrations) != nb:
            raise ValueError(f"{who}: one Equilibration per member ({nb}), got {len(equilibrations)}")
        members = [scale_data(mb[0], mb[1], mb[2], mb[3], eq) + (mb[4],) for mb, eq in zip(members, equilibrations)]
    P = sp.block_diag([mb[0] for mb in members], format="csc")
    A = sp.block_diag([mb[2] for mb in members], format="csc")
    q = np.concatenate([mb[1] for mb in members])
    b = np.concatenate([mb[3] for mb in members])
    cone_specs = [k for mb in members for k in mb[4]]
    blocks = [(mb[0].shape[0], mb[2].shape[0]) for mb in members]
    x_off = np.concatenate([[0], np.cumsum([bl[0] for bl in blocks])]).astype(int)
    z_off = np.concatenate([[0], np.cumsum([bl[1] for bl in blocks])]).astype(int)
    n, m = int(x_off[-1]), int(z_off[-1])
    c.x_off, c.z_off, c.n, c.m = x_off, z_off, n, m
    c.degree = np.array([sum(k.dim if isinstance(k, (NonnegativeConeT, PSDTriangleConeT)) else 1 if isinstance(k, SecondOrderConeT)
                             else 0 for k in mb[4]) for mb in members], float)
    # (no equilibration: the norms of q and b from the host data; equilibrated: from the handle, once per solve)
    c.normq = np.array([np.abs(mb[1]).max() if mb[1].size else 0.0 for mb in members])
    c.normb = np.array([np.abs(mb[3]).max() if mb[3].size else 0.0 for mb in members])

    c.backend = backend = HipSystemBackend(P, A, cone_specs)
    ks, system = backend.ks, backend.system
    c.dev = dev = system._devstr
    ks.set_stream(torch.cuda.current_stream(torch.device(dev)).cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    new = lambda k: torch.zeros(max(k, 1), dtype=torch.float64, device=dev)[:k]
    c.qd, c.bd = up(q), up(b)

    c.x, c.s, c.z = new(n), new(m), new(m)
    c.dx, c.ds, c.dz = new(n), new(m), new(m)
    c.aff_s, c.rhs_s = new(m), new(m)
    c.rx, c.rx_inf, c.Px, c.rhs_x = new(n), new(n), new(n), new(n)
    c.rz, c.rz_inf, c.rhs_z = new(m), new(m), new(m)
    c.aff_x, c.aff_z = new(n), new(m)                    # the affine right-hand side with the frozen members' rows zeroed
    system.init(q, b)
    system.set_problems(blocks)
    if member_refinement:
        system.set_member_refinement(True)
    if isolate:
        system.set_member_status(True)
    c.equil = None
    if equilibrations is not None:
        # the members' scalings onto the handle; what the loop reads of them (as solver_device._Equil for one problem)
        system.set_equilibration_batch(equilibrations)
        c.equil = eq = _BatchSetup()
        eq.ptrs = system.equilibration_dev()
        eq.c = np.array([float(e_.c) for e_ in equilibrations])
        eq.cinv = 1.0 / eq.c
        eq.d = np.concatenate([np.asarray(e_.d, float).ravel() for e_ in equilibrations])
        eq.e = np.concatenate([np.asarray(e_.e, float).ravel() for e_ in equilibrations])
        eq.einv = 1.0 / eq.e
        eq.fx, eq.fz, eq.fs = new(n), new(m), new(m)     # variables_unscale!'s factors per row, filled at the end of a solve
    return c


def _loop_batch(c, inspect=None):
    """The loop of solve_device_batch, solve_device_batch_refined and solve_device_batch_isolated, from the default start,
    on a _BatchSetup.  c.equil set (solver_device.DeviceBatchSolver): the handle was built from data equilibrated member by
    member -- the residual pass takes the handle's (d, dinv, e, einv), every member's cost scaling c_b is backed out of
    its own scalars (cinv, info.jl:19-51), the norms of its unscaled q and b come from the handle once per solve
    (hipkkt_kkt_system_data_norms_batch), variables_unscale! (variables.jl:247-275) is applied per member before the one
    copy to the host, and the objectives are those of the residual pass's scalars (the host keeps no current copy of the
    data).  None: the loop as it always was."""
    import torch
    st, member_refinement, isolate, members, nb = c.st, c.member_refinement, c.isolate, c.members, c.nb
    x_off, z_off, n, m, degree = c.x_off, c.z_off, c.n, c.m, c.degree
    backend = c.backend
    system, dev = backend.system, c.dev
    qd, bd = c.qd, c.bd
    equil = c.equil
    d_equil = None if equil is None else equil.ptrs
    normq, normb = (c.normq, c.normb) if equil is None else system.data_norms_batch().T.copy()
    p = lambda t: t.data_ptr()
    ir_total = 0

    # ---- default start (solver.jl:383-404), the shifts per member
    x, s, z = c.x, c.s, c.z
    dx, ds, dz = c.dx, c.ds, c.dz
    aff_s, rhs_s = c.aff_s, c.rhs_s
    rx, rx_inf, Px, rhs_x = c.rx, c.rx_inf, c.Px, c.rhs_x
    rz, rz_inf, rhs_z = c.rz, c.rz_inf, c.rhs_z
    aff_x, aff_z = c.aff_x, c.aff_z
    ir_member = np.zeros(nb, dtype=np.int64)             # (member rule: every member's own rounds)
    backend.update_identity()
    system.solve_constant_rhs()
    system.solve_initial_point_dev(p(x), p(s), p(z))
    system.shift_to_interior_batch_dev(p(s), True)
    system.shift_to_interior_batch_dev(p(z), False)
    tau, kappa = np.ones(nb), np.ones(nb)
    s0, z0 = s.clone(), z.clone()                        # the start: where a frozen member's block of K is scaled (below)

    it = 0
    nfrozen = 0
    alpha = np.zeros(nb)
    status = [UNSOLVED] * nb
    iterations = [0] * nb
    prev = [None] * nb
    hist = [[] for _ in range(nb)]
    restored = [False] * nb                              # (the member ended on the iterate before its last history row)
    prev_vars = None
    tiny = 100 * np.finfo(float).eps

    def end_members(named, act, active):
        """isolate: the active members that `named` marks end with NUMERICAL_ERROR and leave act / active"""
        for k in active:
            if named[k]:
                status[k], iterations[k] = NUMERICAL_ERROR, it
                act[k] = False
        return [k for k in active if act[k]]

    with np.errstate(all="ignore"):                      # (a frozen member's scalars may overflow; they are not used)
        while True:
            active = [k for k in range(nb) if status[k] == UNSOLVED]
            # ---- residuals (residuals.jl:1-37); every member's twelve scalars in ONE read-back
            R = system.residuals_batch_dev(p(x), p(s), p(z), tau, p(rx), p(rz), p(rx_inf), p(rz_inf), p(Px), d_equil)
            qx, bz, sz, xPx = R[:, 0], R[:, 1], R[:, 2], R[:, 3]
            rtau = qx + bz + kappa + xPx / tau
            mu = (sz + tau * kappa) / (degree + 1)
            if inspect is not None:
                inspect(dict(x=x, s=s, z=z, dx=dx, ds=ds, dz=dz, aff_s=aff_s, rhs_s=rhs_s, rx=rx, rz=rz, rx_inf=rx_inf,
                             rz_inf=rz_inf, Px=Px, q=qd, b=bd), backend)
            for k in active:
                # ---- info_update! (info.jl:1-63); equilibrated: the norms came scaled by d, e and their inverses out of
                #      the residual pass, and the member's cost scaling c_b is backed out here (cinv, info.jl:19-51)
                nx, nz, ns, n_rxi, n_Px, n_rzi, n_rz, n_rx = (float(v) for v in R[k, 4:12])
                tinv = 1.0 / tau[k]
                cost_p = qx[k] * tinv + xPx[k] * tinv * tinv / 2
                cost_d = -bz[k] * tinv - xPx[k] * tinv * tinv / 2
                if equil is not None:
                    cinv = equil.cinv[k]
                    cost_p, cost_d, nz = cost_p * cinv, cost_d * cinv, nz * cinv          # info.jl:27-28, :34
                    n_rxi = n_rxi * cinv                                                  # :38
                res_pinf = n_rxi / max(1.0, nz)
                res_dinf = max(n_Px / max(1.0, nx), n_rzi / max(1.0, nx + ns))
                nx, nz, ns = nx * tinv, nz * tinv, ns * tinv
                res_p = n_rz * tinv / max(1.0, normb[k] + nx + ns)
                res_d = (n_rx * tinv if equil is None else n_rx * tinv * cinv) / max(1.0, normq[k] + nx + nz)      # :51
                gap_abs = abs(cost_p - cost_d)
                gap_rel = gap_abs / max(1.0, min(abs(cost_p), abs(cost_d)))
                kt = kappa[k] * tinv
                hist[k].append(dict(iter=it, pcost=float(cost_p), dcost=float(cost_d), gap=float(gap_abs), pres=res_p, dres=res_d,
                                    kt=float(kt), mu=float(mu[k]), step=float(alpha[k])))
                # ---- termination (info.jl:65-120, 270-330)
                stk = UNSOLVED
                if kt <= 1 and (gap_abs < st.tol_gap_abs or gap_rel < st.tol_gap_rel) and res_p < st.tol_feas and res_d < st.tol_feas:
                    stk = SOLVED
                elif kt > 1000.0 / st.tol_ktratio:
                    if bz[k] < -st.tol_infeas_abs and res_pinf < -st.tol_infeas_rel * bz[k]:
                        stk = PRIMAL_INFEASIBLE
                    elif qx[k] < -st.tol_infeas_abs and res_dinf < -st.tol_infeas_rel * qx[k]:
                        stk = DUAL_INFEASIBLE
                pv = prev[k]
                if stk == UNSOLVED and it > 1 and pv is not None and (res_d > pv["res_d"] or res_p > pv["res_p"]):
                    if kt < tiny and (pv["gap_abs"] < st.tol_gap_abs or pv["gap_rel"] < st.tol_gap_rel):
                        stk = INSUFFICIENT_PROGRESS
                    if kt < 1 and ((res_d > 100 * st.tol_feas and res_d > 100 * pv["res_d"]) or
                                   (res_p > 100 * st.tol_feas and res_p > 100 * pv["res_p"])):
                        stk = INSUFFICIENT_PROGRESS
                if stk == UNSOLVED and it == st.max_iter:
                    stk = MAX_ITERATIONS
                prev[k] = dict(res_p=res_p, res_d=res_d, gap_abs=gap_abs, gap_rel=gap_rel)
                if stk != UNSOLVED:
                    status[k], iterations[k] = stk, it
                    if stk == INSUFFICIENT_PROGRESS and prev_vars is not None:      # this member's rows only
                        px, ps, pz, ptau, pkappa = prev_vars
                        x[x_off[k]:x_off[k + 1]] = px[x_off[k]:x_off[k + 1]]
                        s[z_off[k]:z_off[k + 1]] = ps[z_off[k]:z_off[k + 1]]
                        z[z_off[k]:z_off[k + 1]] = pz[z_off[k]:z_off[k + 1]]
                        tau[k], kappa[k] = ptau[k], pkappa[k]
                        restored[k] = True
            active = [k for k in range(nb) if status[k] == UNSOLVED]
            if not active:
                break
            act = np.zeros(nb, bool)
            act[active] = True
            # ---- kkt_update!: cone scaling from (s, z), refactor, constant-RHS solve (solver.jl:258-280); joint
            it += 1
            # What a frozen member leaves in the stack.  The iterate a member ENDS on is one that no stand-alone loop ever
            # factorises (the loop stops before the next kkt_update!); with s z ~ 1e-10 its block of K spoils the refinement
            # of the whole stack's solves, whose accept / stop rule is joint: a member SOLVED after 11 iterations alone ended
            # ALMOST_SOLVED after 15 beside one that had ended after 10.  So from the iteration after it ended
            #   - a frozen member's block of K is scaled at the member's START point (s0, z0), which is well conditioned
            #     (a row mask and torch.where: two elementwise launches), and
            #   - its rows of the affine and the combined right-hand side are made exactly ZERO, so that its rows of the
            #     solutions and of the refinement's error are exactly zero too (K is block diagonal) and its size does not enter
            #     the joint tolerance reltol ||b||_inf -- by the library's own elementwise calls with 0 / 1 as the members'
            #     scalars, three small launches.
            # Its step is discarded anyway (alpha = 0); nothing here runs before a member has ended.
            while True:
                frozen = (~act).astype(float)
                any_frozen = len(active) < nb
                if nb - len(active) != nfrozen:
                    nfrozen = nb - len(active)
                    hm = np.zeros(m, bool)
                    for k in range(nb):
                        if not act[k]:
                            hm[z_off[k]:z_off[k + 1]] = True
                    frozen_rows = torch.from_numpy(hm).to(dev)
                s_u, z_u = (torch.where(frozen_rows, s0, s), torch.where(frozen_rows, z0, z)) if any_frozen else (s, z)
                ok = system.update_dev(p(s_u), p(z_u))
                if ok or not isolate:
                    break
                # isolate: the members the failed update names end alone, and the update is repeated without them
                words = system.member_status()
                named = (words[:, 0] != 0) | (words[:, 1] != 0)
                if not any(named[k] for k in active):
                    break                                                    # (no member to blame: joint, below)
                active = end_members(named, act, active)
                if not active:
                    break
            if ok:
                # ---- affine step (solver.jl:282-295): right-hand side (rx, s - rz)
                system.affine_ds_dev(p(aff_s))
                arx, arz = rx, rz
                if any_frozen:
                    system.combined_rhs_batch_dev(p(aff_x), p(aff_z), p(rx), p(rz), frozen)      # frozen rows: 0, others: rx, rz
                    # ... and aff_z = 0 + 1 s there, so that s - aff_z = 0 (dx, ds: scratch, written by the solve below)
                    system.add_step_batch_dev(p(dx), p(ds), p(aff_z), p(rx), p(rz), p(s), frozen)
                    arx, arz = aff_x, aff_z
                ok, dtau, dkappa = system.solve_batch_dev((p(dx), p(ds), p(dz)), (p(arx), p(aff_s), p(arz)), rtau, tau * kappa,
                                                          (p(x), p(s), p(z)), tau, kappa, True)
                ir_total += backend.last_ir_iterations
                if member_refinement:
                    rinfo = system.member_refinement_info()
                    ir_member += rinfo[:, 0].astype(np.int64)
                    if not ok and isolate and rinfo[:, 3].any():
                        # the flagged members end alone; the others' rows of the step are finished
                        active = end_members(rinfo[:, 3] != 0, act, active)
                        ok = True
            if ok:
                # ---- combined step (solver.jl:297-323)
                alpha = system.step_length_batch_dev(p(dz), p(ds), p(z), p(s), dtau, dkappa, tau, kappa)
                sigma = np.where(act, (1 - alpha) ** 3, 1.0)                 # (frozen: (1 - sigma) rx = 0)
                mcorr = np.where(act, np.ones(nb) if it > 1 else alpha, 0.0)
                system.combined_ds_batch_dev(p(rhs_s), p(dz), p(ds), np.where(act, sigma * mu, 0.0), mcorr)
                if any_frozen:                                               # rhs_s = 0 on frozen rows (rhs_x: rewritten below)
                    system.combined_rhs_batch_dev(p(rhs_x), p(rhs_s), p(rx), p(rhs_s), frozen)
                system.combined_rhs_batch_dev(p(rhs_x), p(rhs_z), p(rx), p(rz), sigma)
                ok, dtau, dkappa = system.solve_batch_dev((p(dx), p(ds), p(dz)), (p(rhs_x), p(rhs_s), p(rhs_z)), (1 - sigma) * rtau,
                                                          -sigma * mu + mcorr * dtau * dkappa + tau * kappa,
                                                          (p(x), p(s), p(z)), tau, kappa, False)
                ir_total += backend.last_ir_iterations
                if member_refinement:
                    rinfo = system.member_refinement_info()
                    ir_member += rinfo[:, 0].astype(np.int64)
                    if not ok and isolate and rinfo[:, 3].any():
                        active = end_members(rinfo[:, 3] != 0, act, active)
                        ok = True
            if not ok:
                alpha = np.zeros(nb)
                for k in active:
                    status[k], iterations[k] = NUMERICAL_ERROR, it
                break
            alpha = system.step_length_batch_dev(p(dz), p(ds), p(z), p(s), dtau, dkappa, tau, kappa) * st.max_step_fraction
            alpha[~act] = 0.0
            for k in active:
                if not alpha[k] > max(0.0, st.min_terminate_step_length):
                    status[k], iterations[k] = INSUFFICIENT_PROGRESS, it
                    alpha[k] = 0.0
            prev_vars = (x.clone(), s.clone(), z.clone(), tau.copy(), kappa.copy())
            system.add_step_batch_dev(p(x), p(s), p(z), p(dx), p(ds), p(dz), alpha)
            go = alpha != 0.0
            tau = np.where(go, tau + alpha * dtau, tau)
            kappa = np.where(go, kappa + alpha * dkappa, kappa)

        # ---- info_post_process! (info.jl:196-211) per member: after an error / limit exit, an iterate that meets the reduced
        #      tolerances is ALMOST_SOLVED
        late = [k for k in range(nb) if status[k] in (NUMERICAL_ERROR, INSUFFICIENT_PROGRESS, MAX_ITERATIONS)]
        if late:
            R = system.residuals_batch_dev(p(x), p(s), p(z), tau, p(rx), p(rz), p(rx_inf), p(rz_inf), p(Px), d_equil)
            for k in late:
                qx, bz, xPx, nx, nz, ns, n_rz, n_rx = (float(R[k, i]) for i in (0, 1, 3, 4, 5, 6, 10, 11))
                tinv = 1.0 / tau[k]
                cp = qx * tinv + xPx * tinv * tinv / 2
                cd = -bz * tinv - xPx * tinv * tinv / 2
                if equil is not None:
                    cinv = equil.cinv[k]
                    cp, cd, nz, n_rx = cp * cinv, cd * cinv, nz * cinv, n_rx * cinv
                nx, nz, ns = nx * tinv, nz * tinv, ns * tinv
                rp = n_rz * tinv / max(1.0, normb[k] + nx + ns)
                rd = n_rx * tinv / max(1.0, normq[k] + nx + nz)
                ga = abs(cp - cd)
                gr = ga / max(1.0, min(abs(cp), abs(cd)))
                if kappa[k] * tinv <= 1 and (ga < st.reduced_tol_gap_abs or gr < st.reduced_tol_gap_rel) and \
                        rp < st.reduced_tol_feas and rd < st.reduced_tol_feas:
                    status[k] = ALMOST_SOLVED
    # ---- solution_post_process! per member: unscale by the member's tau (kappa for certificates); one copy to the host
    torch.cuda.synchronize()
    if equil is not None:
        # variables_unscale! (variables.jl:247-275) per member: x *= d / scale, z *= e / (scale c_b), s *= einv / scale, on
        # the device, then the one copy; the objectives are the costs of the residual pass over the iterate the member
        # ended on (its last history row; the one before where the previous iterate was restored)
        scale = np.array([1.0 / (kappa[k] if status[k] in (PRIMAL_INFEASIBLE, DUAL_INFEASIBLE) else tau[k]) for k in range(nb)])
        equil.fx.copy_(torch.from_numpy(equil.d * np.repeat(scale, np.diff(x_off))))
        equil.fz.copy_(torch.from_numpy(equil.e * np.repeat(scale * equil.cinv, np.diff(z_off))))
        equil.fs.copy_(torch.from_numpy(equil.einv * np.repeat(scale, np.diff(z_off))))
        xh, zh, sh = (x * equil.fx).cpu().numpy(), (z * equil.fz).cpu().numpy(), (s * equil.fs).cpu().numpy()
        out = []
        for k in range(nb):
            row = hist[k][-2 if restored[k] else -1]
            objp, objd = row["pcost"], row["dcost"]
            if status[k] in (PRIMAL_INFEASIBLE, DUAL_INFEASIBLE):
                objp = objd = float("nan")
            out.append(IPMResult(status[k], xh[x_off[k]:x_off[k + 1]].copy(), zh[z_off[k]:z_off[k + 1]].copy(),
                                 sh[z_off[k]:z_off[k + 1]].copy(), objp, objd, iterations[k],
                                 int(ir_member[k]) if member_refinement else ir_total, hist[k]))
        return out
    xh, zh, sh = x.cpu().numpy(), z.cpu().numpy(), s.cpu().numpy()
    out = []
    for k, (Pt, qk, _, bk, _) in enumerate(members):
        infeasible = status[k] in (PRIMAL_INFEASIBLE, DUAL_INFEASIBLE)
        sc = 1.0 / (kappa[k] if infeasible else tau[k])
        xo, zo, so = xh[x_off[k]:x_off[k + 1]] * sc, zh[z_off[k]:z_off[k + 1]] * sc, sh[z_off[k]:z_off[k + 1]] * sc
        Pfull = (Pt + sp.triu(Pt, 1).T).tocsr()
        quad = 0.5 * xo @ (Pfull @ xo)
        objp, objd = qk @ xo + quad, -bk @ zo - quad
        if infeasible:
            objp = objd = float("nan")
        out.append(IPMResult(status[k], xo, zo, so, objp, objd, iterations[k], int(ir_member[k]) if member_refinement else ir_total,
                             hist[k]))
    return out


def _solve(P, q, A, b, cone_specs, settings, inspect, native, nonsym, genpow=False):
    """What the entry points share: the set-up, then the loop from the default start."""
    return _loop(_setup(P, q, A, b, cone_specs, settings, native, nonsym, genpow), inspect)


class _Setup:
    """Everything a solve needs that does not depend on the iterate: the handle (ordering, symbolic analysis, schedule,
    allocations), the loop's device tensors, the host copies the objectives are computed from.  Built once by _setup;
    _loop runs on it any number of times (solver_device.DeviceSolver)."""


def _setup(P, q, A, b, cone_specs, settings, native, nonsym, genpow=False, kkt_data=None):
    """kkt_data: (P, q, A, b) the handle is built from where that is not the data of the objectives (equilibrated data:
    solver_device.DeviceSolver); None: the same."""
    import torch
    c = _Setup()
    c.st = settings or IPMSettings()
    c.native, c.nonsym, c.genpow, c.cone_specs = native, nonsym, genpow, cone_specs
    P = sp.csc_matrix(P)
    Pt = sp.triu(P, format="csc")
    c.Pfull_h = (Pt + sp.triu(Pt, 1).T).tocsr()              # (the objective of the final solution, on the host)
    c.q, c.b = np.asarray(q, float), np.asarray(b, float)
    n, m = c.Pfull_h.shape[0], sp.csc_matrix(A).shape[0]
    c.n, c.m = n, m
    c.degree = sum(k.dim if isinstance(k, (NonnegativeConeT, PSDTriangleConeT)) else 1 if isinstance(k, SecondOrderConeT)
                   else 3 if isinstance(k, (ExponentialConeT, PowerConeT))
                   else len(k.alpha) + 1 if isinstance(k, GenPowerConeT) else 0 for k in cone_specs)
    c.normq = np.abs(c.q).max() if n else 0.0
    c.normb = np.abs(c.b).max() if m else 0.0
    kP, kq, kA, kb = (P, c.q, A, c.b) if kkt_data is None else kkt_data
    large_psd = any(isinstance(k, PSDTriangleConeT) and k.dim > PSD_MAX_SIDE for k in cone_specs)
    c.backend = HipSystemBackend(kP, kA, cone_specs, large_psd=large_psd)
    ks, system = c.backend.ks, c.backend.system
    c.dev = dev = system._devstr
    ks.set_stream(torch.cuda.current_stream(torch.device(dev)).cuda_stream)     # torch's kernels and the library's: one queue
    if not native:
        A_h = sp.csr_matrix(kA)
        kPt = sp.triu(sp.csc_matrix(kP), format="csc")
        c.csr = (_Csr((kPt + sp.triu(kPt, 1).T).tocsr(), dev), _Csr(A_h, dev), _Csr(A_h.T, dev))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    new = lambda k: torch.zeros(max(k, 1), dtype=torch.float64, device=dev)[:k]
    c.qd, c.bd = up(kq), up(kb)
    c.x, c.s, c.z = new(n), new(m), new(m)
    c.dx, c.ds, c.dz = new(n), new(m), new(m)
    c.aff_s, c.rhs_s = new(m), new(m)
    if native:
        c.rx, c.rx_inf, c.Px, c.rhs_x = new(n), new(n), new(n), new(n)
        c.rz, c.rz_inf, c.rhs_z = new(m), new(m), new(m)
    system.init(kq, kb)
    return c


def _loop(c, inspect=None, equil=None):
    """The loop the entry points share, from the default start (as the reference's solve!, solver.jl:189-380), on a
    _Setup.  nonsym: the reference's path for a list that does not allow the symmetric start (solver.jl:383-404) -- every
    line that differs sits under `if nonsym`.  genpow (with nonsym): the cone operations are the _gp calls, which cover
    generalized power cones as well.
    equil (solver_device.DeviceSolver; needs the library's own plumbing): the handle was built from equilibrated data --
    .ptrs: the device pointers (d, dinv, e, einv) that residuals_dev takes, .cinv: 1 / c, .d, .e, .einv: device tensors
    for variables_unscale!.  None: the loop as it always was."""
    import torch
    st, native, nonsym, genpow, cone_specs = c.st, c.native, c.nonsym, c.genpow, c.cone_specs
    assert equil is None or native
    Pfull_h, q, b, n, m, degree = c.Pfull_h, c.q, c.b, c.n, c.m, c.degree
    # (equilibrated: the norms of the UNSCALED q and b from the handle's scaled ones, once per solve -- info.jl:14-16)
    normq, normb = (c.normq, c.normb) if equil is None else c.backend.system.data_norms()
    d_equil = None if equil is None else equil.ptrs
    cinv = 1.0 if equil is None else equil.cinv
    backend = c.backend
    ks, system = backend.ks, backend.system
    if genpow:                                           # the five cone operations of a non-symmetric list
        unit_initialization, affine_ds_ns, combined_ds_ns, step_length_ns_dev, barrier_dev = (
            system.unit_initialization_gp_dev, system.affine_ds_gp_dev, system.combined_ds_gp_dev, system.step_length_gp_dev,
            system.barrier_gp_dev)
    else:
        unit_initialization, affine_ds_ns, combined_ds_ns, step_length_ns_dev, barrier_dev = (
            system.unit_initialization_dev, system.affine_ds_ns_dev, system.combined_ds_ns_dev, system.step_length_ns_dev,
            system.barrier_dev)
    if not native:
        Pfull, Ad, At = c.csr
    qd, bd = c.qd, c.bd
    p = lambda t: t.data_ptr()
    ir_total = 0

    # ---- default start: solver.jl:383-404
    x, s, z = c.x, c.s, c.z
    dx, ds, dz = c.dx, c.ds, c.dz
    aff_s, rhs_s = c.aff_s, c.rhs_s
    if native:
        rx, rx_inf, Px, rhs_x = c.rx, c.rx_inf, c.Px, c.rhs_x
        rz, rz_inf, rhs_z = c.rz, c.rz_inf, c.rhs_z
    strategy = PRIMAL_DUAL                               # the reference's `scaling` (solver.jl:221); read under nonsym only
    bt_step, bt_min = st.linesearch_backtrack_step, st.min_terminate_step_length
    if nonsym:
        x.zero_()
        unit_initialization(p(s), p(z))                  # variables_unit_initialization!: x = 0, no solve
    else:
        backend.update_identity()
        system.solve_constant_rhs()
        system.solve_initial_point_dev(p(x), p(s), p(z))
        system.shift_to_interior_dev(p(s), True)         # variables.jl:213-237
        system.shift_to_interior_dev(p(z), False)
    tau, kappa = 1.0, 1.0

    def step_length_ns(combined):                        # solver_get_step_length (solver.jl:407-442) on a non-symmetric list
        a = step_length_ns_dev(p(dz), p(ds), p(z), p(s), dtau, dkappa, tau, kappa, bt_step, bt_min)
        if not combined:
            return a
        a *= st.max_step_fraction
        if strategy == DUAL:                             # solver_backtrack_step_to_barrier
            for _ in range(50):
                if barrier(a) < 1.0:
                    break
                a *= bt_step
        return a

    def barrier(a):                                      # variables_barrier (variables.jl:46-72): two scalars per call
        cone_barrier, dot = barrier_dev(p(z), p(s), p(dz), p(ds), a)
        ct, ck = tau + a * dtau, kappa + a * dkappa
        with np.errstate(all="ignore"):
            mu_a = (dot + ct * ck) / (degree + 1)
            return (degree + 1) * _logsafe(mu_a) - _logsafe(ct) - _logsafe(ck) + cone_barrier

    it, alpha, sigma = 0, 0.0, 1.0
    status = UNSOLVED
    prev = None
    hist = []
    prev_vars = None
    nrm = torch.linalg.vector_norm
    while True:
        # ---- residuals (residuals.jl:1-37); the scalars in ONE read-back
        if native:
            qx, bz, sz, xPx, nx, nz, ns, n_rxi, n_Px, n_rzi, n_rz, n_rx = system.residuals_dev(
                p(x), p(s), p(z), tau, p(rx), p(rz), p(rx_inf), p(rz_inf), p(Px), d_equil).tolist()
        else:
            Px = Pfull.mv(x)
            rx_inf = -At.mv(z)
            rz_inf = Ad.mv(x) + s
            rx = rx_inf - Px - qd * tau
            rz = rz_inf - bd * tau
            qx, bz, sz, xPx, nx, nz, ns, n_rxi, n_Px, n_rzi, n_rz, n_rx = torch.stack(
                [qd @ x, bd @ z, s @ z, x @ Px, nrm(x), nrm(z), nrm(s), nrm(rx_inf), nrm(Px), nrm(rz_inf), nrm(rz), nrm(rx)]).tolist()
        rtau = qx + bz + kappa + xPx / tau
        mu = (sz + tau * kappa) / (degree + 1)
        if inspect is not None:
            inspect(dict(x=x, s=s, z=z, dx=dx, ds=ds, dz=dz, aff_s=aff_s, rhs_s=rhs_s, rx=rx, rz=rz, rx_inf=rx_inf,
                         rz_inf=rz_inf, Px=Px, q=qd, b=bd), backend)
        # ---- info_update! (info.jl:1-63); equilibrated: the norms came scaled by d, e and their inverses out of the
        #      residual pass, and the cost scaling c is backed out here (cinv, info.jl:19-51)
        tinv = 1.0 / tau
        cost_p = qx * tinv + xPx * tinv * tinv / 2
        cost_d = -bz * tinv - xPx * tinv * tinv / 2
        if equil is not None:
            cost_p, cost_d, nz = cost_p * cinv, cost_d * cinv, nz * cinv              # info.jl:27-28, :34
            n_rxi = n_rxi * cinv                                                      # :38
        res_pinf = n_rxi / max(1.0, nz)
        res_dinf = max(n_Px / max(1.0, nx), n_rzi / max(1.0, nx + ns))
        nx, nz, ns = nx * tinv, nz * tinv, ns * tinv
        res_p = n_rz * tinv / max(1.0, normb + nx + ns)
        res_d = (n_rx * tinv if equil is None else n_rx * tinv * cinv) / max(1.0, normq + nx + nz)      # :51
        gap_abs = abs(cost_p - cost_d)
        gap_rel = gap_abs / max(1.0, min(abs(cost_p), abs(cost_d)))
        kt = kappa * tinv
        hist.append(dict(iter=it, pcost=cost_p, dcost=cost_d, gap=gap_abs, pres=res_p, dres=res_d, kt=kt, mu=mu,
                         step=alpha))
        # ---- termination (info.jl:65-120, 270-330)
        status = UNSOLVED
        if kt <= 1 and (gap_abs < st.tol_gap_abs or gap_rel < st.tol_gap_rel) and res_p < st.tol_feas and res_d < st.tol_feas:
            status = SOLVED
        elif kt > 1000.0 / st.tol_ktratio:
            if bz < -st.tol_infeas_abs and res_pinf < -st.tol_infeas_rel * bz:
                status = PRIMAL_INFEASIBLE
            elif qx < -st.tol_infeas_abs and res_dinf < -st.tol_infeas_rel * qx:
                status = DUAL_INFEASIBLE
        if status == UNSOLVED and it > 1 and prev is not None and (res_d > prev["res_d"] or res_p > prev["res_p"]):
            if kt < 100 * np.finfo(float).eps and (prev["gap_abs"] < st.tol_gap_abs or prev["gap_rel"] < st.tol_gap_rel):
                status = INSUFFICIENT_PROGRESS
            if kt < 1 and ((res_d > 100 * st.tol_feas and res_d > 100 * prev["res_d"]) or
                           (res_p > 100 * st.tol_feas and res_p > 100 * prev["res_p"])):
                status = INSUFFICIENT_PROGRESS
        if status == UNSOLVED and it == st.max_iter:
            status = MAX_ITERATIONS
        if status != UNSOLVED:
            if status == INSUFFICIENT_PROGRESS and prev_vars is not None:
                x, s, z, tau, kappa = prev_vars
            if status == INSUFFICIENT_PROGRESS and nonsym and strategy == PRIMAL_DUAL:
                # _strategy_checkpoint_insufficient_progress: go on from the previous iterate with dual scaling
                strategy, status = DUAL, UNSOLVED
                continue
            break
        # ---- kkt_update!: cone scaling from (s, z), refactor, constant-RHS solve (solver.jl:258-280)
        it += 1
        if nonsym:
            ks.set_nonsymmetric_scaling(strategy, mu)    # host-only; the update below picks it up
        ok = system.update_dev(p(s), p(z))
        if ok:
            # ---- affine step (solver.jl:282-295)
            if nonsym:
                affine_ds_ns(p(aff_s), p(s))
            else:
                system.affine_ds_dev(p(aff_s))
            ok, dtau, dkappa = system.solve_dev((p(dx), p(ds), p(dz)), (p(rx), p(aff_s), p(rz)), rtau, tau * kappa,
                                                (p(x), p(s), p(z)), tau, kappa, True)
            ir_total += backend.last_ir_iterations
        if ok:
            # ---- combined step (solver.jl:297-323)
            alpha = step_length_ns(False) if nonsym else \
                system.step_length_dev(p(dz), p(ds), p(z), p(s), dtau, dkappa, tau, kappa)
            sigma = (1 - alpha) ** 3
            mcorr = 1.0 if it > 1 else alpha
            if nonsym:
                combined_ds_ns(p(rhs_s), p(dz), p(ds), p(s), p(z), sigma * mu, mcorr)
            else:
                system.combined_ds_dev(p(rhs_s), p(dz), p(ds), sigma * mu, mcorr)
            if native:
                system.combined_rhs_dev(p(rhs_x), p(rhs_z), p(rx), p(rz), sigma)
            else:
                rhs_x, rhs_z = (1 - sigma) * rx, (1 - sigma) * rz
            ok, dtau, dkappa = system.solve_dev((p(dx), p(ds), p(dz)), (p(rhs_x), p(rhs_s), p(rhs_z)), (1 - sigma) * rtau,
                                                -sigma * mu + mcorr * dtau * dkappa + tau * kappa,
                                                (p(x), p(s), p(z)), tau, kappa, False)
            ir_total += backend.last_ir_iterations
        if not ok:
            alpha = 0.0
            if nonsym and strategy == PRIMAL_DUAL:       # _strategy_checkpoint_numerical_error
                strategy = DUAL
                continue
            status = NUMERICAL_ERROR
            break
        if nonsym:
            alpha = step_length_ns(True)
            if strategy == PRIMAL_DUAL and alpha < st.min_switch_step_length:
                strategy, alpha = DUAL, 0.0              # _strategy_checkpoint_small_step
                continue
        else:
            alpha = system.step_length_dev(p(dz), p(ds), p(z), p(s), dtau, dkappa, tau, kappa) * st.max_step_fraction
        if alpha <= max(0.0, st.min_terminate_step_length):
            status = INSUFFICIENT_PROGRESS
            alpha = 0.0
            break
        prev = dict(res_p=res_p, res_d=res_d, gap_abs=gap_abs, gap_rel=gap_rel)
        prev_vars = (x.clone(), s.clone(), z.clone(), tau, kappa)
        if native:
            system.add_step_dev(p(x), p(s), p(z), p(dx), p(ds), p(dz), alpha)
        else:
            x.add_(dx, alpha=alpha)
            s.add_(ds, alpha=alpha)
            z.add_(dz, alpha=alpha)
        tau += alpha * dtau
        kappa += alpha * dkappa

    # ---- info_post_process! (info.jl:196-211): after an error / limit exit, accept an iterate that meets the reduced
    #      tolerances as ALMOST_SOLVED
    if status in (NUMERICAL_ERROR, INSUFFICIENT_PROGRESS, MAX_ITERATIONS):
        tinv = 1.0 / tau
        if native:
            o = system.residuals_dev(p(x), p(s), p(z), tau, p(rx), p(rz), p(rx_inf), p(rz_inf), p(Px), d_equil)
            qx, bz, xPx, nx, nz, ns, n_rz, n_rx = (float(o[i]) for i in (0, 1, 3, 4, 5, 6, 10, 11))
        else:
            Px = Pfull.mv(x)
            qx, bz, xPx, nx, nz, ns, n_rz, n_rx = torch.stack(
                [qd @ x, bd @ z, x @ Px, nrm(x), nrm(z), nrm(s), nrm(Ad.mv(x) + s - bd * tau), nrm(-At.mv(z) - Px - qd * tau)]).tolist()
        cp = qx * tinv + xPx * tinv * tinv / 2
        cd = -bz * tinv - xPx * tinv * tinv / 2
        if equil is not None:
            cp, cd, nz, n_rx = cp * cinv, cd * cinv, nz * cinv, n_rx * cinv
        nx, nz, ns = nx * tinv, nz * tinv, ns * tinv
        rp = n_rz * tinv / max(1.0, normb + nx + ns)
        rd = n_rx * tinv / max(1.0, normq + nx + nz)
        ga = abs(cp - cd)
        gr = ga / max(1.0, min(abs(cp), abs(cd)))
        if kappa * tinv <= 1 and (ga < st.reduced_tol_gap_abs or gr < st.reduced_tol_gap_rel) and \
                rp < st.reduced_tol_feas and rd < st.reduced_tol_feas:
            status = ALMOST_SOLVED
    # ---- solution_post_process!: unscale by tau (kappa for certificates); the one copy of length n / m to the host
    infeasible = status in (PRIMAL_INFEASIBLE, DUAL_INFEASIBLE)
    sc = 1.0 / (kappa if infeasible else tau)
    torch.cuda.synchronize()
    if equil is None:
        xo, zo, so = (x * sc).cpu().numpy(), (z * sc).cpu().numpy(), (s * sc).cpu().numpy()
    else:
        # variables_unscale! (variables.jl:247-275): x *= d / scale, z *= e / (scale c), s *= einv / scale
        xo, zo, so = ((x * (equil.d * sc)).cpu().numpy(), (z * (equil.e * (sc * cinv))).cpu().numpy(),
                      (s * (equil.einv * sc)).cpu().numpy())
    objp = q @ xo + 0.5 * xo @ (Pfull_h @ xo)
    objd = -b @ zo - 0.5 * xo @ (Pfull_h @ xo)
    if infeasible:
        objp = objd = float("nan")
    return IPMResult(status, xo, zo, so, objp, objd, it, ir_total, hist)
