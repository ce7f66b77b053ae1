"""A resident solver: set up once, solve, change the numbers, solve again.

`DeviceSolver` is the reference's `Solver` for the workload this design suits best -- the same structure solved again and
again with new data (a model-predictive controller, a parameter sweep).  Construction pays the host ordering, the symbolic
analysis, the schedule, the sweep plans, every allocation and the equilibration once; `.solve()` is the loop of
`ipm_device.solve_device*` with `plumbing="device"` from the default start (the reference has no warm start either:
solver.jl:189-225); `.update_data` / `.update_P` / `.update_A` / `.update_q` / `.update_b` are `update_data!` and its
siblings (`/root/reference/src/data_updating.jl:26-247`): new UNSCALED values are scaled by the equilibration frozen at
construction and written where the handle keeps them, on the device (hipkkt_kkt_system_update_data_*).

Not covered: a resident solver for batches (it needs per-member data norms), warm starts (the reference
has none), presolve and chordal decomposition (the reference forbids updates under them: data_updating.jl:149-158).
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
        import torch
        if arg is None:
            return None
        index = None
        if sp.issparse(arg):
            if name not in "PA":
                raise ValueError(f"{name} is a vector")
            ref = self.P if name == "P" else self.A
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
        length = self._host(name).size
        if isinstance(arg, torch.Tensor):
            if arg.dtype != torch.float64 or arg.dim() != 1 or not arg.is_contiguous() or str(arg.device) != self._c.dev:
                raise ValueError(f"a tensor must be a contiguous fp64 vector on {self._c.dev}")
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
