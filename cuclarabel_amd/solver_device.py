"""A resident solver: set up once, solve, change the numbers, solve again.

`DeviceSolver` is the reference's `Solver` for the workload this design suits best -- the same structure solved again and
again with new data (a model-predictive controller, a parameter sweep).  Construction pays the host ordering, the symbolic
analysis, the schedule, the sweep plans, every allocation and the equilibration once; `.solve()` is the loop of
`ipm_device.solve_device*` with `plumbing="device"` from the default start (the reference has no warm start either:
solver.jl:189-225); `.update_data` / `.update_P` / `.update_A` / `.update_q` / `.update_b` are `update_data!` and its
siblings (`/root/reference/src/data_updating.jl:26-247`): new UNSCALED values are scaled by the equilibration frozen at
construction and written where the handle keeps them, on the device (hipkkt_kkt_system_update_data_*).

`DeviceBatchSolver` is the same for a batch of independent problems on one stacked handle (ipm_device.solve_device_batch*):
every member is equilibrated by its own Ruiz scalings and its own cost scaling c_b, once, at construction
(hipkkt_kkt_system_set_equilibration_batch), and a re-solve after `.update_data` / `.update_data_stack` pays neither the
host ordering of the stack nor an allocation.

Not covered: warm starts (the reference has none), presolve and chordal decomposition (the reference
forbids updates under them: data_updating.jl:149-158).
"""
import numpy as np
import scipy.sparse as sp

from . import equilibrate as _eq
from . import ipm_device as _dev
from .cones import ExponentialConeT, PowerConeT, GenPowerConeT


class _Equil:
    """what ipm_device._loop reads of the equilibration"""


def scale_data(P, q, A, b, eq):
    """(c D P D on the upper triangle, c D q, E A D, E b) in the update kernels' order of operations -- P: (v (d_r d_c)) c,
    A: v (e_r d_c), q: (v d) c, b: v e (data_updating.jl:181-194, :216-231) -- so that a solver built from new data with a
    given Equilibration holds, bit for bit, what a resident solver holds after update_data with the same data."""
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    Pt.sort_indices()
    Ac = sp.csc_matrix(A).copy()
    Ac.sort_indices()
    n = Pt.shape[0]
    d, e, c = np.asarray(eq.d, float), np.asarray(eq.e, float), float(eq.c)
    pcol = np.repeat(np.arange(n), np.diff(Pt.indptr))
    acol = np.repeat(np.arange(n), np.diff(Ac.indptr))
    Ps = sp.csc_matrix((Pt.data * (d[Pt.indices] * d[pcol]) * c, Pt.indices, Pt.indptr), shape=Pt.shape)
    As = sp.csc_matrix((Ac.data * (e[Ac.indices] * d[acol]), Ac.indices, Ac.indptr), shape=Ac.shape)
    return Ps, np.asarray(q, float) * d * c, As, np.asarray(b, float) * e


def _prepare_update(name, arg, ref, length, dev):
    """One argument of update_data -> None (a no-op) or (name, values, index | None), argument errors raised.  ref: the
    original matrix whose pattern a sparse argument must match (P: its upper triangle), None for q and b; length: the
    number of stored values; dev: the device a tensor must live on."""
    import torch
    if arg is None:
        return None
    index = None
    if sp.issparse(arg):
        if name not in "PA":
            raise ValueError(f"{name} is a vector")
        M = sp.triu(sp.csc_matrix(arg), format="csc") if name == "P" else sp.csc_matrix(arg)
        M.sort_indices()
        if M.shape != ref.shape or not np.array_equal(M.indptr, ref.indptr) or not np.array_equal(M.indices, ref.indices):
            raise ValueError(f"the input must match the sparsity pattern of the original {name}" +
                             (" (its upper triangle)" if name == "P" else ""))
        arg = M.data
    elif isinstance(arg, tuple):
        if len(arg) != 2:
            raise ValueError("an indexed update is a pair (index, values)")
        index = np.ascontiguousarray(arg[0], dtype=np.int64).ravel()
        arg = arg[1]
    if isinstance(arg, torch.Tensor):
        if arg.dtype != torch.float64 or arg.dim() != 1 or not arg.is_contiguous() or str(arg.device) != dev:
            raise ValueError(f"a tensor must be a contiguous fp64 vector on {dev}")
        values = arg
    else:
        values = np.ascontiguousarray(arg, dtype=np.float64).ravel()
    k = int(values.numel() if isinstance(values, torch.Tensor) else values.size)
    if index is not None:
        if index.size != k:
            raise ValueError("index and values must have the same length")
        if k and (index.min() < 0 or index.max() >= length or np.unique(index).size != k):
            raise ValueError(f"the positions must be distinct and lie in [0, {length})")
    elif k not in (0, length):
        raise ValueError(f"the input must match the length of the original {name}'s values ({length}), got {k}")
    return None if k == 0 else (name, values, index)


class DeviceSolver:
    """DeviceSolver(P, q, A, b, cone_specs, settings=None, equilibrate=True, equilibration=None)

    Accepts every cone list the three `solve_device*` functions accept and runs their loop (symmetric lists: the symmetric
    start; a list with an exponential or power cone: the non-symmetric loop; with a generalized power cone: the _gp calls).
    equilibrate: Ruiz-equilibrate the data on the device (data_equilibrate!, problemdata.jl:133-221), as the reference
    does by default; False: scalings of one.  equilibration: adopt this `equilibrate.Equilibration` instead of computing
    one (the data is then scaled with it in the update kernels' order: scale_data)."""

    def __init__(self, P, q, A, b, cone_specs, settings=None, equilibrate=True, equilibration=None):
        import torch
        cone_specs = list(cone_specs)
        genpow = any(isinstance(k, GenPowerConeT) for k in cone_specs)
        nonsym = genpow or any(isinstance(k, (ExponentialConeT, PowerConeT)) for k in cone_specs)
        who, allowed = ("solve_device_genpow", _dev._NONSYMMETRIC + (GenPowerConeT,)) if genpow else \
            ("solve_device_nonsymmetric", _dev._NONSYMMETRIC) if nonsym else ("solve_device", _dev._SYMMETRIC)
        cone_specs = _dev._check_cones("DeviceSolver", cone_specs, allowed, "DeviceSolver (the loop of " + who + "): unknown cone type {}")
        # the unscaled data, on the host: the objectives are computed from it, and pattern checks compare with it
        self.P = sp.triu(sp.csc_matrix(P), format="csc").astype(np.float64)
        self.P.sort_indices()
        self.A = sp.csc_matrix(A).astype(np.float64)
        self.A.sort_indices()
        self.q, self.b = np.array(q, np.float64), np.array(b, np.float64)
        n, m = self.P.shape[0], self.A.shape[0]
        if self.A.shape[1] != n or self.q.shape != (n,) or self.b.shape != (m,):
            raise ValueError("P must be n x n, A m x n, q of length n and b of length m")
        if equilibration is not None:
            self.equilibration = equilibration
        else:
            self.equilibration = _eq.equilibrate(self.P, self.q, self.A, self.b, cone_specs, max_iter=10 if equilibrate else 0)[4]
        # The handle's data is ALWAYS scale_data(unscaled data, equilibration) -- not the Ruiz rounds' own output, which is
        # the same to a few ulps but is a product of ten roundings per entry: what the handle holds is then a function of
        # the unscaled data and (d, e, c) alone, whether a datum arrived at construction or through an update, so that a
        # re-solve after update_data equals a fresh solver with the same equilibration bit for bit.
        Ps, qs, As, bs = scale_data(self.P, self.q, self.A, self.b, self.equilibration)
        # one handle from the scaled data; the scalings onto it; init; the loop's tensors, once
        self._c = _dev._setup(self.P, self.q, self.A, self.b, cone_specs, settings, True, nonsym, genpow, kkt_data=(Ps, qs, As, bs))
        self.system = self._c.backend.system
        self.system.set_equilibration(self.equilibration)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self._c.dev)
        eq = self.equilibration
        self._equil = _Equil()
        self._equil.ptrs = self.system.equilibration_dev()
        self._equil.cinv = 1.0 / float(eq.c)
        self._equil.d, self._equil.e, self._equil.einv = up(eq.d), up(eq.e), up(1.0 / np.asarray(eq.e, float))
        self.n, self.m = n, m

    def solve(self):
        """-> IPMResult, always from the default start, as the reference's solve! (solver.jl:189-225)."""
        return _dev._loop(self._c, None, self._equil)

    # ---- update_data! and its siblings (data_updating.jl:26-147)
    def update_data(self, P=None, q=None, A=None, b=None):
        """Each of P, q, A, b: None or an empty array (a no-op), a full vector of new values (numpy, or a torch fp64 tensor
        already on the handle's device, which is passed by pointer), a pair (index, values) with zero-based positions
        into the stored values (for P: of its upper triangle), or -- P and A -- a scipy sparse matrix whose pattern equals
        the original's (for P: that of triu), else ValueError as the reference throws DimensionMismatch
        (data_updating.jl:177).  Everything is checked before anything is changed."""
        jobs = [self._prepare(name, arg) for name, arg in (("P", P), ("q", q), ("A", A), ("b", b))]
        for job in jobs:
            if job is not None:
                self._apply(*job)

    def update_P(self, P):
        self.update_data(P=P)

    def update_A(self, A):
        self.update_data(A=A)

    def update_q(self, q):
        self.update_data(q=q)

    def update_b(self, b):
        self.update_data(b=b)

    def _host(self, name):
        return {"P": self.P.data, "A": self.A.data, "q": self.q, "b": self.b}[name]

    def _prepare(self, name, arg):
        """-> None (a no-op) or (name, values, index | None), argument errors raised"""
        return _prepare_update(name, arg, self.P if name == "P" else self.A if name == "A" else None, self._host(name).size,
                               self._c.dev)

    def _apply(self, name, values, index):
        import torch
        if isinstance(values, torch.Tensor):
            dv, hv = values, values.cpu().numpy()
        else:
            dv = torch.from_numpy(values).to(self._c.dev)
            hv = values
        getattr(self.system, f"update_data_{name}_dev")(dv.data_ptr(), index, int(hv.size))
        torch.cuda.current_stream(torch.device(self._c.dev)).synchronize()      # (dv may go away)
        host = self._host(name)
        if index is None:
            host[:] = hv
        else:
            host[index] = hv
        # the host copies the objectives are computed from
        c = self._c
        if name == "P":
            c.Pfull_h = (self.P + sp.triu(self.P, 1).T).tocsr()
        elif name == "q":
            c.q = self.q
        elif name == "b":
            c.b = self.b


class DeviceBatchSolver:
    """DeviceBatchSolver(problems, settings=None, equilibrate=True, equilibrations=None, member_refinement=True, isolate=True)

    problems: list of (P, q, A, b, cone_specs) as for `ipm_device.solve_device_batch` -- symmetric cones with PSD side
    <= 48, anything else refused with ValueError before a handle is built.  Every member is equilibrated SEPARATELY with
    `equilibrate.equilibrate` (equilibrate=False: scalings of one and c_b = 1), or adopts its entry of `equilibrations` (a
    list of `equilibrate.Equilibration`, one per member); its data is scaled with `scale_data` and the scaled members are
    stacked, so that what the handle holds is a function of the unscaled data and the members' (d, e, c_b) alone, whether a
    datum arrived at construction or through an update.  member_refinement / isolate: the two member modes of
    solve_device_batch_refined and solve_device_batch_isolated (both False: the loop of solve_device_batch).

    The host keeps the members' patterns for the checks of `update_data` and no current copy of their values: the
    objectives of a result are the costs of the residual pass over the iterate the member ended on."""

    def __init__(self, problems, settings=None, equilibrate=True, equilibrations=None, member_refinement=True, isolate=True):
        who = "DeviceBatchSolver"
        members = _dev._check_batch(who, problems, bool(isolate))
        pats = []
        for (Pt, q, A, b, _) in members:
            Pt, A = Pt.copy(), A.copy()
            Pt.sort_indices()
            A.sort_indices()
            if A.shape[1] != Pt.shape[0] or q.shape != (Pt.shape[0],) or b.shape != (A.shape[0],):
                raise ValueError(f"{who}: member {len(pats)}: P must be n x n, A m x n, q of length n and b of length m")
            pats.append((Pt, A))
        if equilibrations is not None:
            self.equilibrations = list(equilibrations)
            if len(self.equilibrations) != len(members):
                raise ValueError(f"{who}: one Equilibration per member ({len(members)}), got {len(self.equilibrations)}")
        else:
            self.equilibrations = [_eq.equilibrate(Pt, q, A, b, cones, max_iter=10 if equilibrate else 0)[4]
                                   for (Pt, q, A, b, cones) in members]
        # one handle from the members scaled and stacked; partition, member modes and the members' scalings onto it; init;
        # the loop's tensors, once
        self._c = _dev._setup_batch(who, members, settings, bool(member_refinement), bool(isolate), self.equilibrations)
        self.system = self._c.backend.system
        self.nb = len(members)
        # the patterns (values unused) and where a member's rows and stored entries sit in the stack: a member's columns
        # are a run of the stack's columns, so its stored entries of P and A are a run of the stacked CSC values
        self._P = [pt for pt, _ in pats]
        self._A = [a for _, a in pats]
        off = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self._off = {"P": off([pt.nnz for pt in self._P]), "A": off([a.nnz for a in self._A]),
                     "q": off([pt.shape[0] for pt in self._P]), "b": off([a.shape[0] for a in self._A])}

    def solve(self):
        """-> list of IPMResult, one per member, always from the default start (the reference has no warm start)."""
        return _dev._loop_batch(self._c)

    # ---- update_data! and its siblings (data_updating.jl:26-147), member by member or on the whole stack
    def update_data(self, member, P=None, q=None, A=None, b=None):
        """New UNSCALED data of one member: each of P, q, A, b in one of the forms of `DeviceSolver.update_data`, with
        positions LOCAL to the member (translated here to positions in the stack).  ValueError for a member out of range, a
        pattern mismatch, a repeated or out-of-range position or a wrong length; everything is checked before anything is
        changed."""
        k = int(member)
        if k != member or not 0 <= k < self.nb:
            raise ValueError(f"member must lie in [0, {self.nb}), got {member!r}")
        jobs = []
        for name, arg in (("P", P), ("q", q), ("A", A), ("b", b)):
            ref = self._P[k] if name == "P" else self._A[k] if name == "A" else None
            lo, hi = self._off[name][k], self._off[name][k + 1]
            job = _prepare_update(name, arg, ref, int(hi - lo), self._c.dev)
            if job is not None:
                index = np.arange(lo, hi, dtype=np.int64) if job[2] is None else job[2] + lo
                jobs.append((name, job[1], index))
        for job in jobs:
            self._apply(*job)

    def update_data_stack(self, P=None, q=None, A=None, b=None):
        """New UNSCALED data of the whole stack: each of P, q, A, b None or a full vector over the stack (the members'
        values one behind the other; numpy, or a torch fp64 tensor already on the handle's device, which is passed by
        pointer and never copied to the host) -- the form a controller uses every step."""
        jobs = []
        for name, arg in (("P", P), ("q", q), ("A", A), ("b", b)):
            if arg is not None and (sp.issparse(arg) or isinstance(arg, tuple)):
                raise ValueError(f"update_data_stack takes whole vectors; {name} is not one (use update_data for a member)")
            job = _prepare_update(name, arg, None, int(self._off[name][-1]), self._c.dev)
            if job is not None:
                jobs.append(job)
        for job in jobs:
            self._apply(*job)

    def _apply(self, name, values, index):
        import torch
        own = not isinstance(values, torch.Tensor)
        dv = torch.from_numpy(values).to(self._c.dev) if own else values
        getattr(self.system, f"update_data_{name}_dev")(dv.data_ptr(), index, int(dv.numel()))
        if own:
            torch.cuda.current_stream(torch.device(self._c.dev)).synchronize()      # (dv may go away)
