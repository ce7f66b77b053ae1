"""Host-side mirror of the reference's KKT solver objects over the C ABI.

`HipKKTSolver` has the methods of `DirectLDLKKTSolver <: AbstractKKTSolver`
(`/root/reference/src/kktsolvers/kktsolver_directldl.jl:46-92,197-386`, contract
`kktsolver_defaults.jl:2-48`) and `HipDirectLDLSolver` those of an
`AbstractDirectLDLSolver` backend (`direct-ldl/directldl_defaults.jl:1-72`, example
`directldl_qdldl.jl`).  Method names drop Julia's `!`; Bool returns keep the reference's
meaning (True = success, False = numeric failure; usage errors raise).
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import check, f64, i64, ptr
from .cones import cone_kinds_dims, cone_param_ptr_vals, KIND_EXP, KIND_POW, KIND_GENPOW


class LinearSolverInfo:
    """types.jl:198-206"""

    def __init__(self, name, threads, direct, nnzA, nnzL):
        self.name, self.threads, self.direct, self.nnzA, self.nnzL = name, threads, direct, nnzA, nnzL

    def __repr__(self):
        return (f"LinearSolverInfo(name={self.name!r}, threads={self.threads}, direct={self.direct}, "
                f"nnzA={self.nnzA}, nnzL={self.nnzL})")


class HipKKTSolver:
    """DirectLDLKKTSolver on the MI355X: KKT assembly maps, value scatter, regularisation,
    numeric LDL', triangular solves and iterative refinement all run on the device."""

    def __init__(self, P, A, cones, m=None, n=None, settings=None, large_psd=False):
        L = _lib.lib()
        P = sp.triu(sp.csc_matrix(P), format="csc")
        P.sort_indices()
        A = sp.csc_matrix(A)
        A.sort_indices()
        self.n = P.shape[0] if n is None else n
        self.m = A.shape[0] if m is None else m
        if P.shape != (self.n, self.n) or A.shape != (self.m, self.n):
            raise ValueError("P must be n x n and A m x n")
        self.cones = list(cones)
        kinds, dims = cone_kinds_dims(self.cones)
        self.settings = settings if settings is not None else _lib.default_settings()
        self._h = C.c_void_p()
        Pp, Pi, Px = i64(P.indptr), i64(P.indices), f64(P.data)
        Ap, Ai, Ax = i64(A.indptr), i64(A.indices), f64(A.data)
        pptr, pvals = cone_param_ptr_vals(self.cones)
        if len(pvals):                                           # cone parameters travel through _ex2 only
            rc = L.hipkkt_kkt_create_ex2(C.byref(self._h), self.n, self.m, ptr(Pp), ptr(Pi), ptr(Px),
                                         ptr(Ap), ptr(Ai), ptr(Ax), len(self.cones), ptr(kinds), ptr(dims), ptr(pptr),
                                         ptr(pvals), C.byref(self.settings), 0)
        else:
            rc = L.hipkkt_kkt_create(C.byref(self._h), self.n, self.m, ptr(Pp), ptr(Pi), ptr(Px),
                                     ptr(Ap), ptr(Ai), ptr(Ax), len(self.cones), ptr(kinds), ptr(dims),
                                     C.byref(self.settings), 0)
        if not check(rc, "hipkkt_kkt_create"):
            raise _lib.HipKKTError("hipkkt_kkt_create reported a numeric failure")
        self._nnzP, self._nnzA = P.nnz, A.nnz
        info = _lib.Info()
        check(L.hipkkt_kkt_info(self._h, C.byref(info)), "hipkkt_kkt_info")
        self.info = info.as_dict()
        self.p = info.p
        self.N = info.N
        if large_psd:
            self.enable_large_psd(True)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.lib().hipkkt_kkt_destroy(h)
            self._h = None

    # ---- AbstractKKTSolver interface (kktsolver_defaults.jl:2-48)
    def kktsolver_update(self, Hsblocks, soc_u=None, soc_v=None, soc_eta2=None):
        """kktsolver_update!(kktsolver, cones) with the cone data flattened the way the glue does:
        get_Hs! output plus each sparse second-order cone's (u, v, eta^2)."""
        Hs = f64(Hsblocks)
        u = f64(soc_u if soc_u is not None else [])
        v = f64(soc_v if soc_v is not None else [])
        e2 = f64(soc_eta2 if soc_eta2 is not None else [])
        if Hs.size != self.info["nHs"] or u.size != self.info["sparse_soc_len"] or \
                v.size != u.size or e2.size != self.info["nsparse_soc"]:
            raise ValueError("cone data has the wrong length")
        return check(_lib.lib().hipkkt_kkt_update_cones(self._h, ptr(Hs), ptr(u), ptr(v), ptr(e2)),
                     "hipkkt_kkt_update_cones")

    def kktsolver_update_from_sz(self, s, z):
        """Device-native variant: update_scaling! + get_Hs! run on the GPU from (s, z)."""
        s, z = f64(s), f64(z)
        if s.size != self.m or z.size != self.m:
            raise ValueError("s, z must have length m")
        return check(_lib.lib().hipkkt_kkt_update_from_sz(self._h, ptr(s), ptr(z)),
                     "hipkkt_kkt_update_from_sz")

    def kktsolver_update_from_sz_dev(self, d_s, d_z):
        return check(_lib.lib().hipkkt_kkt_update_from_sz_dev(self._h, C.c_void_p(d_s), C.c_void_p(d_z)),
                     "hipkkt_kkt_update_from_sz_dev")

    def enable_large_psd(self, enable=True):
        """Opt in to (or out of) the device path for PSD cones of side 49 ... 96 (hipkkt_kkt_enable_large_psd), at every
        level: without it a handle with such a cone is refused as before."""
        check(_lib.lib().hipkkt_kkt_enable_large_psd(self._h, int(bool(enable))), "hipkkt_kkt_enable_large_psd")

    def kktsolver_setrhs(self, rhsx, rhsz):
        rx, rz = f64(rhsx), f64(rhsz)
        if rx.size != self.n or rz.size != self.m:
            raise ValueError("rhs has the wrong length")
        check(_lib.lib().hipkkt_kkt_setrhs(self._h, ptr(rx), ptr(rz)), "hipkkt_kkt_setrhs")

    def kktsolver_solve(self, lhsx=None, lhsz=None):
        """kktsolver_solve!(kktsolver, lhsx, lhsz): writes into the given arrays (either may be
        None, as in the reference) and returns is_success."""
        for a, k in ((lhsx, self.n), (lhsz, self.m)):
            if a is not None and (a.dtype != np.float64 or a.size != k or not a.flags.c_contiguous):
                raise ValueError("lhs arrays must be contiguous float64 of the right length")
        return check(_lib.lib().hipkkt_kkt_solve(self._h, ptr(lhsx), ptr(lhsz)), "hipkkt_kkt_solve")

    def kktsolver_setrhs_dev(self, d_rx, d_rz):
        check(_lib.lib().hipkkt_kkt_setrhs_dev(self._h, C.c_void_p(d_rx), C.c_void_p(d_rz)), "hipkkt_kkt_setrhs_dev")

    def kktsolver_solve_dev(self, d_lhsx, d_lhsz):
        return check(_lib.lib().hipkkt_kkt_solve_dev(self._h, C.c_void_p(d_lhsx) if d_lhsx else None,
                                                     C.c_void_p(d_lhsz) if d_lhsz else None),
                     "hipkkt_kkt_solve_dev")

    def set_deferred_status(self, on=True):
        """The *_dev entry points only enqueue; `deferred_status()` reports once for everything since the last query."""
        check(_lib.lib().hipkkt_kkt_set_deferred_status(self._h, int(on)), "hipkkt_kkt_set_deferred_status")

    def deferred_status(self):
        """0 = every call since the last query succeeded, 1 = numeric failure, 2 = some solve's refinement was cut short."""
        rc = _lib.lib().hipkkt_kkt_deferred_status(self._h)
        if rc < 0:
            check(rc, "hipkkt_kkt_deferred_status")
        return rc

    def kktsolver_solve_multi(self, rhsx, rhsz, want_x=True, want_z=True):
        """setrhs! + solve! for several right-hand sides against the current factorisation.
        rhsx: (n, k), rhsz: (m, k).  Returns (is_success, lhsx (n, k) | None, lhsz (m, k) | None,
        refinement rounds per column)."""
        RX = np.asfortranarray(rhsx, dtype=np.float64)
        RZ = np.asfortranarray(rhsz, dtype=np.float64)
        if RX.ndim != 2 or RZ.ndim != 2 or RX.shape[0] != self.n or RZ.shape[0] != self.m or RX.shape[1] != RZ.shape[1]:
            raise ValueError("rhsx must be (n, k) and rhsz (m, k)")
        k = RX.shape[1]
        LX = np.zeros((self.n, k), order="F") if want_x else None
        LZ = np.zeros((self.m, k), order="F") if want_z else None
        ir = np.zeros(max(k, 1), dtype=np.int64)
        ok = check(_lib.lib().hipkkt_kkt_solve_multi(self._h, k, ptr(RX), ptr(RZ), ptr(LX), ptr(LZ), ptr(ir)),
                   "hipkkt_kkt_solve_multi")
        return ok, LX, LZ, ir[:k]

    def kktsolver_solve_multi_dev(self, k, d_rx, d_rz, d_lhsx, d_lhsz):
        """Device-pointer variant (column-major, contiguous).  Returns (is_success, rounds per column)."""
        ir = np.zeros(max(k, 1), dtype=np.int64)
        ok = check(_lib.lib().hipkkt_kkt_solve_multi_dev(self._h, k, C.c_void_p(d_rx), C.c_void_p(d_rz),
                                                         C.c_void_p(d_lhsx) if d_lhsx else None,
                                                         C.c_void_p(d_lhsz) if d_lhsz else None, ptr(ir)),
                   "hipkkt_kkt_solve_multi_dev")
        return ok, ir[:k]

    def kktsolver_update_P(self, P):
        Px = f64(P.data if sp.issparse(P) else P)
        if Px.size != self._nnzP:
            raise ValueError("P.nzval has the wrong length")
        check(_lib.lib().hipkkt_kkt_update_P(self._h, ptr(Px)), "hipkkt_kkt_update_P")

    def kktsolver_update_A(self, A):
        Ax = f64(A.data if sp.issparse(A) else A)
        if Ax.size != self._nnzA:
            raise ValueError("A.nzval has the wrong length")
        check(_lib.lib().hipkkt_kkt_update_A(self._h, ptr(Ax)), "hipkkt_kkt_update_A")

    def kktsolver_linear_solver_info(self):
        return LinearSolverInfo("hipldl", 1, True, self.info["nnzK"], self.info["nnzL"])

    # ---- extras
    def mul_Hs(self, x):
        x = f64(x)
        y = np.zeros(self.m)
        check(_lib.lib().hipkkt_kkt_mul_Hs(self._h, ptr(y), ptr(x)), "hipkkt_kkt_mul_Hs")
        return y

    def get_Hs(self):
        out = np.zeros(max(self.info["nHs"], 1))
        check(_lib.lib().hipkkt_kkt_get_Hs(self._h, ptr(out)), "hipkkt_kkt_get_Hs")
        return out[:self.info["nHs"]]

    def KKT(self):
        """The assembled triu CSC KKT matrix with its current (un-regularised) values."""
        colptr = np.zeros(self.N + 1, dtype=np.int64)
        rowval = np.zeros(self.info["nnzK"], dtype=np.int64)
        nzval = np.zeros(self.info["nnzK"])
        L = _lib.lib()
        check(L.hipkkt_kkt_get_pattern(self._h, ptr(colptr), ptr(rowval)), "hipkkt_kkt_get_pattern")
        check(L.hipkkt_kkt_get_values(self._h, ptr(nzval)), "hipkkt_kkt_get_values")
        return sp.csc_matrix((nzval, rowval, colptr), shape=(self.N, self.N))

    def residual(self, x, b, route=0):
        """(tests) e = b - K x on the current un-regularised K through the solves' own residual and norm kernels
        (hipkkt_kkt_get_residual).  x, b: (N,) or (N, k) in K's order.  route 0 = column-major with a finishing kernel,
        1 = partial maxima reduced by the refinement-round kernel (k in 1, 2, 4; no long rows), 2 = row-major (no long
        rows).  Returns (e, norm_e (k), norm_b (k)); a route the handle cannot take raises HipKKTError."""
        one = np.ndim(x) == 1
        X = np.asfortranarray(np.reshape(x, (self.N, -1), order="F"), dtype=np.float64)
        B = np.asfortranarray(np.reshape(b, (self.N, -1), order="F"), dtype=np.float64)
        if X.shape != B.shape or X.shape[1] < 1:
            raise ValueError("x and b must both be (N,) or (N, k)")
        k = X.shape[1]
        E = np.zeros((self.N, k), order="F")
        ne, nb = np.zeros(k), np.zeros(k)
        check(_lib.lib().hipkkt_kkt_get_residual(self._h, int(route), k, ptr(X), ptr(B), ptr(E), ptr(ne), ptr(nb)),
              "hipkkt_kkt_get_residual")
        return (E[:, 0] if one else E), ne, nb

    def maps(self):
        i = self.info
        out = dict(P=np.zeros(self._nnzP, np.int64), A=np.zeros(self._nnzA, np.int64),
                   Hsblocks=np.zeros(i["nHs"], np.int64), diag_full=np.zeros(self.N, np.int64),
                   soc_u=np.zeros(i["sparse_soc_len"], np.int64), soc_v=np.zeros(i["sparse_soc_len"], np.int64),
                   soc_D=np.zeros(2 * i["nsparse_soc"], np.int64), dsigns=np.zeros(self.N, np.int64))
        check(_lib.lib().hipkkt_kkt_get_maps(self._h, *[ptr(out[k]) for k in
              ("P", "A", "Hsblocks", "diag_full", "soc_u", "soc_v", "soc_D", "dsigns")]), "hipkkt_kkt_get_maps")
        gp = [c for c in self.cones if c.kind == KIND_GENPOW]
        if gp:
            out.update(genpow_p=np.zeros(sum(c.dim for c in gp), np.int64), genpow_q=np.zeros(sum(c.dim1 for c in gp), np.int64),
                       genpow_r=np.zeros(sum(c.dim2 for c in gp), np.int64), genpow_D=np.zeros(3 * len(gp), np.int64))
            check(_lib.lib().hipkkt_kkt_get_genpow_maps(self._h, *[ptr(out[k]) for k in
                  ("genpow_p", "genpow_q", "genpow_r", "genpow_D")]), "hipkkt_kkt_get_genpow_maps")
        return out

    def perm(self):
        out = np.zeros(self.N, dtype=np.int64)
        check(_lib.lib().hipkkt_kkt_get_perm(self._h, ptr(out)), "hipkkt_kkt_get_perm")
        return out

    def scaling(self):
        """The NT scaling on the device: (lambda (m), [(R, Rinv, lam) per PSD cone])."""
        ks = [c.dim for c in self.cones if c.kind == 3]
        tot = sum(k * k for k in ks)
        lam, R, Ri = np.zeros(max(self.m, 1)), np.zeros(max(tot, 1)), np.zeros(max(tot, 1))
        check(_lib.lib().hipkkt_kkt_get_scaling(self._h, ptr(lam), ptr(R), ptr(Ri)), "hipkkt_kkt_get_scaling")
        out, o, off = [], 0, 0
        for c in self.cones:
            if c.kind == 3:
                k = c.dim
                out.append((R[o:o + k * k].reshape(k, k, order="F").copy(), Ri[o:o + k * k].reshape(k, k, order="F").copy(),
                            lam[off:off + k].copy()))
                o += k * k
            off += c.numel
        return lam[:self.m], out

    def set_nonsymmetric_scaling(self, strategy, mu=0.0):
        """How the next device-side scaling treats exponential / power cones: strategy 0 primal-dual (mu unused),
        1 dual (Hs = mu H*(z)).  Host-only; a no-op on a handle without such cones."""
        return check(_lib.lib().hipkkt_kkt_set_nonsymmetric_scaling(self._h, int(strategy), float(mu)),
                     "hipkkt_kkt_set_nonsymmetric_scaling")

    def nonsymmetric(self):
        """(grad (k, 3), H_dual (k, 3, 3)) of the k exponential / power cones, in cone order, after a device-side scaling."""
        k = sum(1 for c in self.cones if c.kind in (KIND_EXP, KIND_POW))
        grad, H = np.zeros(max(3 * k, 1)), np.zeros(max(9 * k, 1))
        check(_lib.lib().hipkkt_kkt_get_nonsymmetric(self._h, ptr(grad), ptr(H)), "hipkkt_kkt_get_nonsymmetric")
        return grad[:3 * k].reshape(k, 3), H[:9 * k].reshape(k, 3, 3)

    def genpow(self):
        """[(grad, d, p, q, r) per generalized power cone], in cone order, after a device-side scaling: all unscaled,
        Hs = mu (diag(d) + p p' - q q' - r r'); d is (d1, then d2 repeated)."""
        gp = [c for c in self.cones if c.kind == KIND_GENPOW]
        n, n1 = sum(c.dim for c in gp), sum(c.dim1 for c in gp)
        grad, d, p = np.zeros(max(n, 1)), np.zeros(max(n, 1)), np.zeros(max(n, 1))
        q, r = np.zeros(max(n1, 1)), np.zeros(max(n - n1, 1))
        check(_lib.lib().hipkkt_kkt_get_genpow(self._h, ptr(grad), ptr(d), ptr(p), ptr(q), ptr(r)), "hipkkt_kkt_get_genpow")
        out, o, o1, o2 = [], 0, 0, 0
        for c in gp:
            out.append((grad[o:o + c.dim].copy(), d[o:o + c.dim].copy(), p[o:o + c.dim].copy(),
                        q[o1:o1 + c.dim1].copy(), r[o2:o2 + c.dim2].copy()))
            o, o1, o2 = o + c.dim, o1 + c.dim1, o2 + c.dim2
        return out

    def scaling_w(self):
        """(w (m), eta (per cone)) of the device's NT scaling."""
        w, eta = np.zeros(max(self.m, 1)), np.zeros(max(len(self.cones), 1))
        check(_lib.lib().hipkkt_kkt_get_scaling_w(self._h, ptr(w), ptr(eta)), "hipkkt_kkt_get_scaling_w")
        return w[:self.m], eta[:len(self.cones)]

    @property
    def fallbacks(self):
        """(overlap-mode, persistent-sweep-kernel) fallbacks taken by this handle so far; expected (0, 0)."""
        p = self.profile()
        return int(p["overlap_fallbacks"]), int(p["top_fallbacks"])

    @property
    def diagonal_regularizer(self):
        return _lib.lib().hipkkt_kkt_last_regularizer(self._h)

    @property
    def last_ir_iterations(self):
        return int(_lib.lib().hipkkt_kkt_last_ir_iterations(self._h))

    def speculative_rounds(self, set=-1):
        """(tests) refinement rounds a solve enqueues ahead of its first status read-back; `set` >= 0 replaces it first"""
        return int(_lib.lib().hipkkt_kkt_speculative_rounds(self._h, int(set)))

    def set_stream(self, stream_ptr):
        check(_lib.lib().hipkkt_kkt_set_stream(self._h, C.c_void_p(stream_ptr)), "hipkkt_kkt_set_stream")

    def synchronize(self):
        check(_lib.lib().hipkkt_kkt_synchronize(self._h), "hipkkt_kkt_synchronize")

    def profile_enable(self, on=True):
        check(_lib.lib().hipkkt_kkt_profile_enable(self._h, int(on)), "hipkkt_kkt_profile_enable")

    def profile_reset(self):
        check(_lib.lib().hipkkt_kkt_profile_reset(self._h), "hipkkt_kkt_profile_reset")

    def profile(self):
        p = _lib.Profile()
        check(_lib.lib().hipkkt_kkt_profile_get(self._h, C.byref(p)), "hipkkt_kkt_profile_get")
        return p.as_dict()


class HipKKTSystem:
    """DefaultKKTSystem (`/root/reference/src/kktsystem.jl:21-215`) with its vectors in HBM (level C of
    the C ABI): `kkt_update!`, `kkt_solve_initial_point!`, `kkt_solve!`.  The `*_dev` methods take raw
    device pointers; the numpy-facing ones stage through torch tensors (plumbing for tests and the IPM
    test driver)."""

    def __init__(self, kktsolver):
        self.ks = kktsolver
        self._ready = False
        self.nb = 0                  # members of the partition (set_problems); 0: none

    def init(self, q, b):
        q, b = f64(q), f64(b)
        if q.size != self.ks.n or b.size != self.ks.m:
            raise ValueError("q must have length n and b length m")
        check(_lib.lib().hipkkt_kkt_system_init(self.ks._h, ptr(q), ptr(b)), "hipkkt_kkt_system_init")
        self._ready = True

    # ---- device-pointer interface
    def update_dev(self, d_s, d_z):
        return check(_lib.lib().hipkkt_kkt_system_update(self.ks._h, C.c_void_p(d_s), C.c_void_p(d_z)),
                     "hipkkt_kkt_system_update")

    def solve_constant_rhs(self):
        return check(_lib.lib().hipkkt_kkt_system_solve_constant_rhs(self.ks._h), "hipkkt_kkt_system_solve_constant_rhs")

    def solve_initial_point_dev(self, d_x, d_s, d_z):
        return check(_lib.lib().hipkkt_kkt_system_solve_initial_point(self.ks._h, C.c_void_p(d_x), C.c_void_p(d_s),
                                                                       C.c_void_p(d_z)),
                     "hipkkt_kkt_system_solve_initial_point")

    def solve_dev(self, d_lhs, d_rhs, rhs_tau, rhs_kappa, d_var, var_tau, var_kappa, affine):
        """d_lhs, d_rhs, d_var: (x, s, z) triples of device pointers.  Returns (is_success, dtau, dkappa)."""
        tk = np.zeros(2)
        ok = check(_lib.lib().hipkkt_kkt_system_solve(
            self.ks._h, C.c_void_p(d_lhs[0]), C.c_void_p(d_lhs[1]), C.c_void_p(d_lhs[2]), ptr(tk),
            C.c_void_p(d_rhs[0]), C.c_void_p(d_rhs[1]), C.c_void_p(d_rhs[2]), float(rhs_tau), float(rhs_kappa),
            C.c_void_p(d_var[0]), C.c_void_p(d_var[1]), C.c_void_p(d_var[2]), float(var_tau), float(var_kappa),
            0 if affine else 1), "hipkkt_kkt_system_solve")
        return ok, tk[0], tk[1]

    # ---- the cone operations between the solves, on device vectors (raw pointers, like solve_dev)
    def affine_ds_dev(self, d_out):
        """out = lambda o lambda (affine_ds!)."""
        return check(_lib.lib().hipkkt_kkt_system_affine_ds(self.ks._h, C.c_void_p(d_out)), "hipkkt_kkt_system_affine_ds")

    def combined_ds_dev(self, d_out, d_step_z, d_step_s, sigma_mu, m_corr):
        """out = lambda o lambda + m_corr (W^-T step_s) o (W step_z) - sigma_mu e: d.s of the combined right-hand side."""
        return check(_lib.lib().hipkkt_kkt_system_combined_ds(self.ks._h, C.c_void_p(d_out), C.c_void_p(d_step_z),
                                                               C.c_void_p(d_step_s), float(sigma_mu), float(m_corr)),
                     "hipkkt_kkt_system_combined_ds")

    def step_length_dev(self, d_step_z, d_step_s, d_z, d_s, step_tau, step_kappa, tau, kappa):
        """variables_calc_step_length without the max_step_fraction factor -> alpha (a host float)."""
        out = np.zeros(1)
        check(_lib.lib().hipkkt_kkt_system_step_length(self.ks._h, C.c_void_p(d_step_z), C.c_void_p(d_step_s), C.c_void_p(d_z),
                                                       C.c_void_p(d_s), float(step_tau), float(step_kappa), float(tau),
                                                       float(kappa), ptr(out)), "hipkkt_kkt_system_step_length")
        return float(out[0])

    def shift_to_interior_dev(self, d_v, primal):
        """_shift_to_cone_interior! in place -> (min_margin, pos_margin) as found before the shift."""
        out = np.zeros(2)
        check(_lib.lib().hipkkt_kkt_system_shift_to_interior(self.ks._h, C.c_void_p(d_v), 1 if primal else 0, ptr(out)),
              "hipkkt_kkt_system_shift_to_interior")
        return float(out[0]), float(out[1])

    # ---- the same for cone lists with exponential / power cones (the _ns symbols) and with generalized power cones as
    #      well (the _gp symbols): one marshalling helper per operation, the symbol's name chosen by the public method
    def _unit_initialization(self, sym, d_s, d_z):
        return check(getattr(_lib.lib(), sym)(self.ks._h, C.c_void_p(d_s), C.c_void_p(d_z)), sym)

    def _affine_ds(self, sym, d_out, d_s):
        return check(getattr(_lib.lib(), sym)(self.ks._h, C.c_void_p(d_out), C.c_void_p(d_s)), sym)

    def _combined_ds(self, sym, d_out, d_step_z, d_step_s, d_s, d_z, sigma_mu, m_corr):
        return check(getattr(_lib.lib(), sym)(self.ks._h, C.c_void_p(d_out), C.c_void_p(d_step_z), C.c_void_p(d_step_s),
                                              C.c_void_p(d_s), C.c_void_p(d_z), float(sigma_mu), float(m_corr)), sym)

    def _step_length_bt(self, sym, d_step_z, d_step_s, d_z, d_s, step_tau, step_kappa, tau, kappa, backtrack_step, alpha_min):
        out = np.zeros(1)
        check(getattr(_lib.lib(), sym)(self.ks._h, C.c_void_p(d_step_z), C.c_void_p(d_step_s), C.c_void_p(d_z), C.c_void_p(d_s),
                                       float(step_tau), float(step_kappa), float(tau), float(kappa), float(backtrack_step),
                                       float(alpha_min), ptr(out)), sym)
        return float(out[0])

    def _barrier(self, sym, d_z, d_s, d_step_z, d_step_s, alpha):
        out = np.zeros(2)
        check(getattr(_lib.lib(), sym)(self.ks._h, C.c_void_p(d_z), C.c_void_p(d_s), C.c_void_p(d_step_z), C.c_void_p(d_step_s),
                                       float(alpha), ptr(out)), sym)
        return float(out[0]), float(out[1])

    # zero, nonnegative, second-order, PSD <= 48, exponential and power cones in any order; a generalized power cone is refused
    def unit_initialization_dev(self, d_s, d_z):
        """Every cone's unit_initialization! into s and z (the asymmetric start): one launch, no scaling needed."""
        return self._unit_initialization("hipkkt_kkt_system_unit_initialization", d_s, d_z)

    def affine_ds_ns_dev(self, d_out, d_s):
        """out = lambda o lambda on symmetric rows, a copy of s on exponential / power rows (affine_ds!)."""
        return self._affine_ds("hipkkt_kkt_system_affine_ds_ns", d_out, d_s)

    def combined_ds_ns_dev(self, d_out, d_step_z, d_step_s, d_s, d_z, sigma_mu, m_corr):
        """d.s of the combined right-hand side; exponential / power rows: s + sigma_mu grad f*(z) - eta(step_s, m_corr
        step_z).  d_z must be the z the current scaling was computed from."""
        return self._combined_ds("hipkkt_kkt_system_combined_ds_ns", d_out, d_step_z, d_step_s, d_s, d_z, sigma_mu, m_corr)

    def step_length_ns_dev(self, d_step_z, d_step_s, d_z, d_s, step_tau, step_kappa, tau, kappa, backtrack_step, alpha_min):
        """The composite step length of a list with exponential / power cones, without max_step_fraction -> alpha."""
        return self._step_length_bt("hipkkt_kkt_system_step_length_ns", d_step_z, d_step_s, d_z, d_s, step_tau, step_kappa, tau,
                                    kappa, backtrack_step, alpha_min)

    def barrier_dev(self, d_z, d_s, d_step_z, d_step_s, alpha):
        """(sum of the cones' compute_barrier, <z + alpha dz, s + alpha ds>) at the stepped point, as host floats."""
        return self._barrier("hipkkt_kkt_system_barrier", d_z, d_s, d_step_z, d_step_s, alpha)

    # any of the seven kinds, in any order
    def unit_initialization_gp_dev(self, d_s, d_z):
        """unit_initialization_dev with the generalized power cones' start: sqrt(1 + alpha_i) on the first dim1 rows, 0 behind."""
        return self._unit_initialization("hipkkt_kkt_system_unit_initialization_gp", d_s, d_z)

    def affine_ds_gp_dev(self, d_out, d_s):
        """affine_ds_ns_dev, and a copy of s on the generalized power rows."""
        return self._affine_ds("hipkkt_kkt_system_affine_ds_gp", d_out, d_s)

    def combined_ds_gp_dev(self, d_out, d_step_z, d_step_s, d_s, d_z, sigma_mu, m_corr):
        """combined_ds_ns_dev, and s + sigma_mu grad f*(z) (the stored gradient, no higher-order correction) on the
        generalized power rows.  d_z must be the z the current scaling was computed from."""
        return self._combined_ds("hipkkt_kkt_system_combined_ds_gp", d_out, d_step_z, d_step_s, d_s, d_z, sigma_mu, m_corr)

    def step_length_gp_dev(self, d_step_z, d_step_s, d_z, d_s, step_tau, step_kappa, tau, kappa, backtrack_step, alpha_min):
        """step_length_ns_dev with every generalized power cone's backtracking search in the minimum -> alpha."""
        return self._step_length_bt("hipkkt_kkt_system_step_length_gp", d_step_z, d_step_s, d_z, d_s, step_tau, step_kappa, tau,
                                    kappa, backtrack_step, alpha_min)

    def barrier_gp_dev(self, d_z, d_s, d_step_z, d_step_s, alpha):
        """barrier_dev with every generalized power cone's barrier_dual + barrier_primal in the sum."""
        return self._barrier("hipkkt_kkt_system_barrier_gp", d_z, d_s, d_step_z, d_step_s, alpha)

    # ---- residuals and termination scalars of a device-resident iterate, and the elementwise steps around them
    def residuals_dev(self, d_x, d_s, d_z, tau, d_rx, d_rz, d_rx_inf, d_rz_inf, d_Px, d_equil=None):
        """residuals_update! and the scalars info_update! reads, in one pass over K's image -> numpy array of 12:
        q.x, b.z, s.z, x.Px, |d x|, |e z|, |einv s|, |dinv rx_inf|, |dinv Px|, |einv rz_inf|, |einv rz|, |dinv rx|.
        d_equil: (d, dinv, e, einv) device pointers, or None for ones."""
        out = np.zeros(12)
        eq = (None,) * 4 if d_equil is None else tuple(d_equil)
        check(_lib.lib().hipkkt_kkt_system_residuals(
            self.ks._h, C.c_void_p(d_x), C.c_void_p(d_s), C.c_void_p(d_z), float(tau), C.c_void_p(d_rx), C.c_void_p(d_rz),
            C.c_void_p(d_rx_inf), C.c_void_p(d_rz_inf), C.c_void_p(d_Px), C.c_void_p(eq[0]), C.c_void_p(eq[1]),
            C.c_void_p(eq[2]), C.c_void_p(eq[3]), ptr(out)), "hipkkt_kkt_system_residuals")
        return out

    def combined_rhs_dev(self, d_rhs_x, d_rhs_z, d_rx, d_rz, sigma):
        """rhs_x = (1 - sigma) rx, rhs_z = (1 - sigma) rz: the x and z parts of the combined right-hand side."""
        return check(_lib.lib().hipkkt_kkt_system_combined_rhs(self.ks._h, C.c_void_p(d_rhs_x), C.c_void_p(d_rhs_z),
                                                                C.c_void_p(d_rx), C.c_void_p(d_rz), float(sigma)),
                     "hipkkt_kkt_system_combined_rhs")

    def add_step_dev(self, d_x, d_s, d_z, d_dx, d_ds, d_dz, alpha):
        """x += alpha dx, s += alpha ds, z += alpha dz (variables_add_step!) as one launch."""
        return check(_lib.lib().hipkkt_kkt_system_add_step(self.ks._h, C.c_void_p(d_x), C.c_void_p(d_s), C.c_void_p(d_z),
                                                            C.c_void_p(d_dx), C.c_void_p(d_ds), C.c_void_p(d_dz), float(alpha)),
                     "hipkkt_kkt_system_add_step")

    # ---- data updating (update_P! / update_A! / update_q! / update_b!, data_updating.jl:26-247) with the equilibration
    #      frozen on the handle: new UNSCALED values on the device, scaled and written where the handle keeps them
    def set_equilibration(self, eq):
        """The frozen scalings of `equilibrate.Equilibration` (d, e, c) onto the handle, or None to clear them to ones."""
        if eq is None:
            check(_lib.lib().hipkkt_kkt_system_set_equilibration(self.ks._h, None, None, 1.0),
                  "hipkkt_kkt_system_set_equilibration")
            return
        d, e = f64(eq.d), f64(eq.e)
        if d.size != self.ks.n or e.size != self.ks.m:
            raise ValueError("d must have length n and e length m")
        check(_lib.lib().hipkkt_kkt_system_set_equilibration(self.ks._h, ptr(d), ptr(e), float(eq.c)),
              "hipkkt_kkt_system_set_equilibration")

    def equilibration_dev(self):
        """(d, dinv, e, einv) device pointers of the handle's scalings, as `residuals_dev(d_equil=...)` takes them."""
        out = [C.c_void_p() for _ in range(4)]
        check(_lib.lib().hipkkt_kkt_system_equilibration_dev(self.ks._h, *[C.byref(o) for o in out]),
              "hipkkt_kkt_system_equilibration_dev")
        return tuple(o.value for o in out)

    def _update_data(self, name, d_values_ptr, index, k):
        idx = None if index is None else i64(index)
        if idx is not None and idx.ndim != 1:
            raise ValueError("index must be one-dimensional")
        if k is None:
            if idx is None:
                raise ValueError("the vector form needs k (the number of values behind the pointer)")
            k = idx.size
        elif idx is not None and idx.size != int(k):
            raise ValueError("index must have k entries")
        fn = getattr(_lib.lib(), "hipkkt_kkt_system_update_data_" + name)
        check(fn(self.ks._h, C.c_void_p(d_values_ptr), ptr(idx), int(k)), "hipkkt_kkt_system_update_data_" + name)

    def update_data_P_dev(self, d_values_ptr, index=None, k=None):
        """k unscaled values of triu(P) behind a device pointer; index: their zero-based positions in its nzval (host), or
        None for all of them in order (k = nnz).  Refusals raise HipKKTError and leave the handle as it was."""
        self._update_data("P", d_values_ptr, index, k)

    def update_data_A_dev(self, d_values_ptr, index=None, k=None):
        self._update_data("A", d_values_ptr, index, k)

    def update_data_q_dev(self, d_values_ptr, index=None, k=None):
        self._update_data("q", d_values_ptr, index, k)

    def update_data_b_dev(self, d_values_ptr, index=None, k=None):
        self._update_data("b", d_values_ptr, index, k)

    def data_norms(self):
        """(max |q dinv| / c, max |b einv|): the norms of the unscaled q and b (data_get_normq!, data_get_normb!)."""
        out = np.zeros(2)
        check(_lib.lib().hipkkt_kkt_system_data_norms(self.ks._h, ptr(out)), "hipkkt_kkt_system_data_norms")
        return float(out[0]), float(out[1])

    # ---- a stack of independent member problems on this handle: the partition, and the operations between the solves
    #      with every scalar a numpy array over the members (the _batch symbols).  One upload of the scalar arrays and one
    #      read-back per call; the number of launches does not depend on the number of members.
    def set_problems(self, blocks):
        """The partition of the stack: blocks = the members' (n_b, m_b) in stacking order, or None / [] to clear it.
        Raises HipKKTError where the library refuses it (a coupling entry, a cone across a boundary, a cone kind or PSD
        side outside the batched set)."""
        blocks = [] if blocks is None else [(int(nb_), int(mb_)) for nb_, mb_ in blocks]
        x_off = i64(np.concatenate([[0], np.cumsum([b_[0] for b_ in blocks])])) if blocks else i64([0])
        z_off = i64(np.concatenate([[0], np.cumsum([b_[1] for b_ in blocks])])) if blocks else i64([0])
        check(_lib.lib().hipkkt_kkt_system_set_problems(self.ks._h, len(blocks), ptr(x_off), ptr(z_off)),
              "hipkkt_kkt_system_set_problems")
        self.nb = len(blocks)

    def set_equilibration_batch(self, equilibrations):
        """set_equilibration with the cost scaling per member: a list of `equilibrate.Equilibration`, one per member in
        stacking order; their d and e are concatenated, their c form the array of nb.  Raises HipKKTError where the library
        refuses (no partition, a c that is not positive and finite -- the member is named)."""
        eqs = list(equilibrations)
        if self.nb and len(eqs) != self.nb:
            raise ValueError(f"one Equilibration per member ({self.nb}), got {len(eqs)}")
        d = f64(np.concatenate([np.asarray(q.d, float).ravel() for q in eqs])) if eqs else f64([])
        e = f64(np.concatenate([np.asarray(q.e, float).ravel() for q in eqs])) if eqs else f64([])
        c = f64([float(q.c) for q in eqs])
        if d.size != self.ks.n or e.size != self.ks.m:
            raise ValueError("the members' d must have n entries together and their e m entries")
        check(_lib.lib().hipkkt_kkt_system_set_equilibration_batch(self.ks._h, ptr(d), ptr(e), ptr(c)),
              "hipkkt_kkt_system_set_equilibration_batch")

    def data_norms_batch(self):
        """numpy array (nb, 2): row b = (max |q dinv| over member b's x rows / c_b, max |b einv| over its z rows) -- the
        norms of member b's unscaled q and b (data_get_normq!, data_get_normb! per member)."""
        out = np.zeros((max(self.nb, 1), 2))
        check(_lib.lib().hipkkt_kkt_system_data_norms_batch(self.ks._h, ptr(out)), "hipkkt_kkt_system_data_norms_batch")
        return out[:self.nb]

    def set_member_refinement(self, enable):
        """The refinement's accept / stop rule per member of the partition instead of over the stack, for every
        single-column solve of the handle.  Replacing or clearing the partition switches it off again.  Raises
        HipKKTError on a handle without a partition."""
        check(_lib.lib().hipkkt_kkt_system_set_member_refinement(self.ks._h, 1 if enable else 0),
              "hipkkt_kkt_system_set_member_refinement")

    def member_refinement_info(self):
        """numpy array (nb, 4) of the last solve under the member rule: row b = (member b's rounds, ||e_b||_inf of its
        accepted solution, ||b_b||_inf, 1.0 if one of its norms was not finite)."""
        out = np.zeros((max(self.nb, 1), 4))
        check(_lib.lib().hipkkt_kkt_system_member_refinement_info(self.ks._h, ptr(out)),
              "hipkkt_kkt_system_member_refinement_info")
        return out[:self.nb]

    def set_member_status(self, enable):
        """The static regulariser per member (eps_b from member b's own rows of K's image) and a failed update's cone and
        pivot words per member, for every refactorisation of the handle.  Replacing or clearing the partition switches it
        off again.  Raises HipKKTError on a handle without a partition."""
        check(_lib.lib().hipkkt_kkt_system_set_member_status(self.ks._h, 1 if enable else 0),
              "hipkkt_kkt_system_set_member_status")

    def member_status(self):
        """numpy array (nb, 3) of the last refactorisation under member status: row b = (1.0 if the scaling of one of
        member b's cones failed, 1.0 if a pivot in its columns was not finite, eps_b)."""
        out = np.zeros((max(self.nb, 1), 3))
        check(_lib.lib().hipkkt_kkt_system_member_status(self.ks._h, ptr(out)), "hipkkt_kkt_system_member_status")
        return out[:self.nb]

    def _scalars(self, *arrays):
        """The members' scalars as contiguous float64 arrays of length nb (a Python float is not broadcast: one value per
        member is the point of these calls)."""
        out = []
        for a in arrays:
            if a is None:                                # (NULL: the library's to refuse)
                out.append(None)
                continue
            a = f64(a)
            if self.nb and a.shape != (self.nb,):        # (no partition: the library's to refuse)
                raise ValueError(f"a scalar array must have one entry per member ({self.nb}), got shape {a.shape}")
            out.append(a)
        return out

    def residuals_batch_dev(self, d_x, d_s, d_z, tau, d_rx, d_rz, d_rx_inf, d_rz_inf, d_Px, d_equil=None):
        """residuals_dev per member: rx, rz with the row's own tau[b] -> numpy array (nb, 12), row b the twelve scalars over
        member b's rows."""
        tau, = self._scalars(tau)
        out = np.zeros((self.nb, 12))
        eq = (None,) * 4 if d_equil is None else tuple(d_equil)
        check(_lib.lib().hipkkt_kkt_system_residuals_batch(
            self.ks._h, C.c_void_p(d_x), C.c_void_p(d_s), C.c_void_p(d_z), ptr(tau), C.c_void_p(d_rx), C.c_void_p(d_rz),
            C.c_void_p(d_rx_inf), C.c_void_p(d_rz_inf), C.c_void_p(d_Px), C.c_void_p(eq[0]), C.c_void_p(eq[1]),
            C.c_void_p(eq[2]), C.c_void_p(eq[3]), ptr(out)), "hipkkt_kkt_system_residuals_batch")
        return out

    def solve_batch_dev(self, d_lhs, d_rhs, rhs_tau, rhs_kappa, d_var, var_tau, var_kappa, affine):
        """solve_dev per member: the scalars are arrays over the members.  Returns (is_success, dtau, dkappa) with dtau,
        dkappa numpy arrays of nb; is_success is the joint status of the one stacked solve."""
        rhs_tau, rhs_kappa, var_tau, var_kappa = self._scalars(rhs_tau, rhs_kappa, var_tau, var_kappa)
        tk = np.zeros((self.nb, 2))
        ok = check(_lib.lib().hipkkt_kkt_system_solve_batch(
            self.ks._h, C.c_void_p(d_lhs[0]), C.c_void_p(d_lhs[1]), C.c_void_p(d_lhs[2]), ptr(tk),
            C.c_void_p(d_rhs[0]), C.c_void_p(d_rhs[1]), C.c_void_p(d_rhs[2]), ptr(rhs_tau), ptr(rhs_kappa),
            C.c_void_p(d_var[0]), C.c_void_p(d_var[1]), C.c_void_p(d_var[2]), ptr(var_tau), ptr(var_kappa),
            0 if affine else 1), "hipkkt_kkt_system_solve_batch")
        return ok, tk[:, 0].copy(), tk[:, 1].copy()

    def combined_ds_batch_dev(self, d_out, d_step_z, d_step_s, sigma_mu, m_corr):
        """combined_ds_dev with member b's sigma_mu[b], m_corr[b] on its cones."""
        sigma_mu, m_corr = self._scalars(sigma_mu, m_corr)
        return check(_lib.lib().hipkkt_kkt_system_combined_ds_batch(self.ks._h, C.c_void_p(d_out), C.c_void_p(d_step_z),
                                                                     C.c_void_p(d_step_s), ptr(sigma_mu), ptr(m_corr)),
                     "hipkkt_kkt_system_combined_ds_batch")

    def step_length_batch_dev(self, d_step_z, d_step_s, d_z, d_s, step_tau, step_kappa, tau, kappa):
        """step_length_dev per member (without the max_step_fraction factor) -> numpy array of nb."""
        step_tau, step_kappa, tau, kappa = self._scalars(step_tau, step_kappa, tau, kappa)
        out = np.zeros(self.nb)
        check(_lib.lib().hipkkt_kkt_system_step_length_batch(self.ks._h, C.c_void_p(d_step_z), C.c_void_p(d_step_s),
                                                             C.c_void_p(d_z), C.c_void_p(d_s), ptr(step_tau), ptr(step_kappa),
                                                             ptr(tau), ptr(kappa), ptr(out)),
              "hipkkt_kkt_system_step_length_batch")
        return out

    def shift_to_interior_batch_dev(self, d_v, primal):
        """_shift_to_cone_interior! per member, in place -> numpy array (nb, 2): (min_margin, pos_margin) before the shift."""
        out = np.zeros((self.nb, 2))
        check(_lib.lib().hipkkt_kkt_system_shift_to_interior_batch(self.ks._h, C.c_void_p(d_v), 1 if primal else 0, ptr(out)),
              "hipkkt_kkt_system_shift_to_interior_batch")
        return out

    def combined_rhs_batch_dev(self, d_rhs_x, d_rhs_z, d_rx, d_rz, sigma):
        """rhs_x = (1 - sigma[b]) rx, rhs_z = (1 - sigma[b]) rz on member b's rows."""
        sigma, = self._scalars(sigma)
        return check(_lib.lib().hipkkt_kkt_system_combined_rhs_batch(self.ks._h, C.c_void_p(d_rhs_x), C.c_void_p(d_rhs_z),
                                                                      C.c_void_p(d_rx), C.c_void_p(d_rz), ptr(sigma)),
                     "hipkkt_kkt_system_combined_rhs_batch")

    def add_step_batch_dev(self, d_x, d_s, d_z, d_dx, d_ds, d_dz, alpha):
        """x += alpha[b] dx, s += alpha[b] ds, z += alpha[b] dz on member b's rows; alpha[b] == 0 leaves them untouched."""
        alpha, = self._scalars(alpha)
        return check(_lib.lib().hipkkt_kkt_system_add_step_batch(self.ks._h, C.c_void_p(d_x), C.c_void_p(d_s), C.c_void_p(d_z),
                                                                  C.c_void_p(d_dx), C.c_void_p(d_ds), C.c_void_p(d_dz),
                                                                  ptr(alpha)),
                     "hipkkt_kkt_system_add_step_batch")

    def prepared(self, d_lhs, d_rhs, rhs_tau, rhs_kappa, d_var, var_tau, var_kappa):
        """(update, solve_affine, solve_combined) closures over pre-converted ctypes arguments for a caller that issues the
        same three calls on the same resident buffers every iteration (bench.py): the per-call argument marshalling of
        `update_dev` / `solve_dev` is host time during which the GPU idles.  d_rhs = (affine (x, s, z), combined (x, s, z))."""
        L = _lib.lib()
        h = self.ks._h
        tk = np.zeros(2)
        P = lambda v: C.c_void_p(v)
        upd_args = (h, P(d_var[1]), P(d_var[2]))
        sol_args = [(h, P(d_lhs[0]), P(d_lhs[1]), P(d_lhs[2]), ptr(tk), P(r[0]), P(r[1]), P(r[2]), C.c_double(rhs_tau),
                     C.c_double(rhs_kappa), P(d_var[0]), P(d_var[1]), P(d_var[2]), C.c_double(var_tau), C.c_double(var_kappa),
                     C.c_int(st)) for r, st in ((d_rhs[0], 0), (d_rhs[1], 1))]
        fu, fs = L.hipkkt_kkt_system_update, L.hipkkt_kkt_system_solve

        def update():
            return check(fu(*upd_args), "hipkkt_kkt_system_update")

        def solve(i):
            ok = check(fs(*sol_args[i]), "hipkkt_kkt_system_solve")
            return ok, tk[0], tk[1]
        return update, (lambda: solve(0)), (lambda: solve(1))

    def prepared_host(self, lhs, rhs, rhs_tau, rhs_kappa, var, var_tau, var_kappa, scaling, reduced=True, reuse_variables=True):
        """The same three closures for HOST-resident numpy vectors -- what integration/HipKKTExt.jl does per iteration:
        kkt_update! from the caller's cone scaling (reduced: hipkkt_kkt_system_update_scaling with (w, eta, lambda, R,
        Rinv); otherwise hipkkt_kkt_system_update_cones with the full nine arrays), then the two kkt_solve! through
        hipkkt_kkt_system_solve_host, the combined one re-using the affine one's variables.  lhs, var: (x, s, z) arrays;
        rhs = (affine (x, s, z), combined (x, s, z)); the arrays must stay alive (and may be page-locked: _lib.host_register)."""
        L = _lib.lib()
        h = self.ks._h
        tk = np.zeros(2)
        keep = (lhs, rhs, var, scaling, tk)
        fs = L.hipkkt_kkt_system_solve_host
        if reduced:
            w, eta, lam, R, Ri = scaling[-5:]
            fu, upd_args = L.hipkkt_kkt_system_update_scaling, (h, ptr(w), ptr(eta), ptr(lam), ptr(R), ptr(Ri))
        else:
            fu, upd_args = L.hipkkt_kkt_system_update_cones, (h,) + tuple(ptr(v) for v in scaling)
        sol_args = []
        for r, st in ((rhs[0], 0), (rhs[1], 1)):
            vv = (None, None, None) if (st == 1 and reuse_variables) else (ptr(var[0]), ptr(var[1]), ptr(var[2]))
            sol_args.append((h, ptr(lhs[0]), ptr(lhs[1]), ptr(lhs[2]), ptr(tk), ptr(r[0]), ptr(r[1]), ptr(r[2]), C.c_double(rhs_tau),
                             C.c_double(rhs_kappa)) + vv + (C.c_double(var_tau), C.c_double(var_kappa), C.c_int(st)))

        def update():
            return check(fu(*upd_args), "kkt_update! (host scaling)")

        def solve(i):
            ok = check(fs(*sol_args[i]), "hipkkt_kkt_system_solve_host")
            return ok, tk[0], tk[1]
        update._keep = keep
        return update, (lambda: solve(0)), (lambda: solve(1))

    # ---- lazy constant-RHS solve (hipkkt_kkt_system_set_lazy): kkt_update! + kkt_solve!(:affine) as two SEPARATE calls
    #      whose two solves still share one 2-column sweep
    def set_lazy(self, on=True):
        return check(_lib.lib().hipkkt_kkt_system_set_lazy(self.ks._h, int(on)), "hipkkt_kkt_system_set_lazy")

    def update_cones(self, Hsblocks, soc_u, soc_v, soc_eta2, w, eta, lam, psd_R=None, psd_Rinv=None):
        """kkt_update!(kktsystem, data, cones) from the CALLER's cone objects (what the Julia glue has): the data of
        kktsolver_update! plus the NT scaling (w, eta per cone, lambda, and R / Rinv of the PSD cones concatenated
        column-major) that kkt_solve!'s right-hand sides and step recovery use."""
        a = [f64(v if v is not None else []) for v in (Hsblocks, soc_u, soc_v, soc_eta2, w, eta, lam, psd_R, psd_Rinv)]
        i = self.ks.info
        if a[0].size != i["nHs"] or a[1].size != i["sparse_soc_len"] or a[2].size != a[1].size or \
                a[3].size != i["nsparse_soc"] or a[4].size != self.ks.m or a[6].size != self.ks.m or \
                a[5].size != len(self.ks.cones):
            raise ValueError("cone data has the wrong length")
        tot = sum(c.dim * c.dim for c in self.ks.cones if c.kind == 3)
        if a[7].size != tot or a[8].size != tot:
            raise ValueError("psd_R / psd_Rinv have the wrong length")
        return check(_lib.lib().hipkkt_kkt_system_update_cones(self.ks._h, *[ptr(v) for v in a]),
                     "hipkkt_kkt_system_update_cones")

    def update_scaling(self, w, eta, lam, psd_R=None, psd_Rinv=None):
        """kkt_update! from the NT scaling alone (hipkkt_kkt_system_update_scaling): the Hs blocks and the sparse
        second-order-cone vectors are formed on the device from (w, eta, R) instead of crossing PCIe."""
        a = [f64(v if v is not None else []) for v in (w, eta, lam, psd_R, psd_Rinv)]
        if a[0].size != self.ks.m or a[2].size != self.ks.m or a[1].size != len(self.ks.cones):
            raise ValueError("scaling data has the wrong length")
        tot = sum(c.dim * c.dim for c in self.ks.cones if c.kind == 3)
        if a[3].size != tot or a[4].size != tot:
            raise ValueError("psd_R / psd_Rinv have the wrong length")
        self._keep = a          # (registered or not, the arrays outlive the call)
        return check(_lib.lib().hipkkt_kkt_system_update_scaling(self.ks._h, *[ptr(v) for v in a]),
                     "hipkkt_kkt_system_update_scaling")

    # ---- numpy interface.  staging = "host": the *_host entry points of the C ABI (vectors staged by the library: what
    #      a caller with host-resident DefaultVariables uses); "torch": device tensors + the device-pointer entry points
    staging = "host"

    @property
    def _devstr(self):
        import torch
        d = self.ks.settings.device
        return f"cuda:{d if d >= 0 else torch.cuda.current_device()}"       # -1 = the current device

    def _dev(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self._devstr)

    def update(self, s, z):
        if self.staging == "host":
            s, z = f64(s), f64(z)
            if s.size != self.ks.m or z.size != self.ks.m:
                raise ValueError("s, z must have length m")
            return check(_lib.lib().hipkkt_kkt_system_update_host(self.ks._h, ptr(s), ptr(z)), "hipkkt_kkt_system_update_host")
        ds, dz = self._dev(s), self._dev(z)
        return self.update_dev(ds.data_ptr(), dz.data_ptr())

    def update_and_solve_affine_dev(self, d_lhs, d_rhs, rhs_tau, rhs_kappa, d_var, tau, kappa):
        """The same on device pointers: d_lhs = (dx, ds, dz), d_rhs = (rhs.x, rhs.z), d_var = (x, s, z).
        Returns (is_success, dtau, dkappa)."""
        tk = np.zeros(2)
        ok = check(_lib.lib().hipkkt_kkt_system_update_and_solve_affine(
            self.ks._h, C.c_void_p(d_lhs[0]), C.c_void_p(d_lhs[1]), C.c_void_p(d_lhs[2]), ptr(tk),
            C.c_void_p(d_rhs[0]), C.c_void_p(d_rhs[1]), float(rhs_tau), float(rhs_kappa),
            C.c_void_p(d_var[0]), C.c_void_p(d_var[1]), C.c_void_p(d_var[2]), float(tau), float(kappa)),
            "hipkkt_kkt_system_update_and_solve_affine")
        return ok, float(tk[0]), float(tk[1])

    def update_and_solve_affine(self, rhs_x, rhs_z, rhs_tau, rhs_kappa, x, s, z, tau, kappa):
        """kkt_update! + kkt_solve!(:affine) in one call: the constant and the affine right-hand side share one
        2-column solve (hipkkt_kkt_system_update_and_solve_affine).  Returns (is_success, step | None)."""
        import torch
        dev = self._devstr
        n, m = self.ks.n, self.ks.m
        rhs = [self._dev(rhs_x), self._dev(rhs_z)]
        var = [self._dev(x), self._dev(s), self._dev(z)]
        lhs = [torch.zeros(max(k, 1), dtype=torch.float64, device=dev) for k in (n, m, m)]
        ok, dtau, dkappa = self.update_and_solve_affine_dev([t.data_ptr() for t in lhs], [t.data_ptr() for t in rhs],
                                                            rhs_tau, rhs_kappa, [t.data_ptr() for t in var], tau, kappa)
        if not ok:
            return False, None
        dx, ds, dz = lhs[0][:n].cpu().numpy(), lhs[1][:m].cpu().numpy(), lhs[2][:m].cpu().numpy()
        return True, (dx, dz, ds, dtau, dkappa)

    def solve_initial_point(self):
        n, m = self.ks.n, self.ks.m
        if self.staging == "host":
            x, s, z = np.zeros(max(n, 1)), np.zeros(max(m, 1)), np.zeros(max(m, 1))
            ok = check(_lib.lib().hipkkt_kkt_system_solve_initial_point_host(self.ks._h, ptr(x), ptr(s), ptr(z)),
                       "hipkkt_kkt_system_solve_initial_point_host")
            return ok, x[:n], s[:m], z[:m]
        import torch
        dev = self._devstr
        x = torch.zeros(max(n, 1), dtype=torch.float64, device=dev)
        s = torch.zeros(max(m, 1), dtype=torch.float64, device=dev)
        z = torch.zeros(max(m, 1), dtype=torch.float64, device=dev)
        ok = self.solve_initial_point_dev(x.data_ptr(), s.data_ptr(), z.data_ptr())
        return ok, x[:n].cpu().numpy(), s[:m].cpu().numpy(), z[:m].cpu().numpy()

    def solve(self, rhs_x, rhs_s, rhs_z, rhs_tau, rhs_kappa, x, s, z, tau, kappa, affine, reuse_variables=False):
        """reuse_variables (host staging): (x, s, z) are those of the previous call -- the combined step's are the affine
        step's (solver.jl:289-323) -- and are not sent again."""
        n, m = self.ks.n, self.ks.m
        if self.staging == "host":
            a = [f64(v) for v in (rhs_x, rhs_s, rhs_z, x, s, z)]
            for v, k in zip(a, (n, m, m, n, m, m)):
                if v.size != k:
                    raise ValueError("vector of the wrong length")
            lhs = [np.zeros(max(k, 1)) for k in (n, m, m)]
            tk = np.zeros(2)
            ok = check(_lib.lib().hipkkt_kkt_system_solve_host(
                self.ks._h, ptr(lhs[0]), ptr(lhs[1]), ptr(lhs[2]), ptr(tk), ptr(a[0]), ptr(a[1]), ptr(a[2]),
                float(rhs_tau), float(rhs_kappa), *([None, None, None] if reuse_variables else [ptr(a[3]), ptr(a[4]), ptr(a[5])]),
                float(tau), float(kappa), 0 if affine else 1), "hipkkt_kkt_system_solve_host")
            if not ok:
                return False, None
            return True, (lhs[0][:n], lhs[2][:m], lhs[1][:m], float(tk[0]), float(tk[1]))
        import torch
        dev = self._devstr
        rhs = [self._dev(rhs_x), self._dev(rhs_s), self._dev(rhs_z)]
        var = [self._dev(x), self._dev(s), self._dev(z)]
        lhs = [torch.zeros(max(k, 1), dtype=torch.float64, device=dev) for k in (n, m, m)]
        ok, dtau, dkappa = self.solve_dev([t.data_ptr() for t in lhs], [t.data_ptr() for t in rhs], rhs_tau, rhs_kappa,
                                          [t.data_ptr() for t in var], tau, kappa, affine)
        if not ok:
            return False, None
        dx, ds, dz = lhs[0][:n].cpu().numpy(), lhs[1][:m].cpu().numpy(), lhs[2][:m].cpu().numpy()
        return True, (dx, dz, ds, float(dtau), float(dkappa))


class HipDirectLDLSolver:
    """An AbstractDirectLDLSolver backend (`ldlsolver_constructor(::Val{:hipldl})`):
    constructor(KKT, Dsigns, settings), update_values!, scale_values!, refactor!, solve!."""

    matrix_shape = "triu"           # ldlsolver_matrix_shape

    @staticmethod
    def is_available():             # ldlsolver_is_available: must not throw
        try:
            return bool(_lib.lib().hipkkt_available())
        except Exception:
            return False

    def __init__(self, KKT, Dsigns, settings=None):
        L = _lib.lib()
        KKT = sp.csc_matrix(KKT)
        KKT.sort_indices()
        if sp.tril(KKT, -1).nnz:
            raise ValueError("KKT must be upper triangular (:triu)")
        self.N = KKT.shape[0]
        self.nnzK = KKT.nnz
        self.settings = settings if settings is not None else _lib.default_settings()
        self._h = C.c_void_p()
        cp, ri, nz, ds = i64(KKT.indptr), i64(KKT.indices), f64(KKT.data), i64(Dsigns)
        rc = L.hipkkt_ldl_create(C.byref(self._h), self.N, ptr(cp), ptr(ri), ptr(nz), ptr(ds),
                                 C.byref(self.settings), 0)
        if not check(rc, "hipkkt_ldl_create"):
            raise _lib.HipKKTError("hipkkt_ldl_create reported a numeric failure")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.lib().hipkkt_ldl_destroy(h)
            self._h = None

    def update_values(self, index, values):
        idx, v = i64(index), f64(values)
        check(_lib.lib().hipkkt_ldl_update_values(self._h, ptr(idx), ptr(v), idx.size), "hipkkt_ldl_update_values")

    def scale_values(self, index, scale):
        idx = i64(index)
        check(_lib.lib().hipkkt_ldl_scale_values(self._h, ptr(idx), float(scale), idx.size), "hipkkt_ldl_scale_values")

    def refactor(self, K=None):
        return check(_lib.lib().hipkkt_ldl_refactor(self._h), "hipkkt_ldl_refactor")

    def solve(self, K, x, b):
        b = f64(b)
        if x.dtype != np.float64 or x.size != self.N or b.size != self.N:
            raise ValueError("x, b must be float64 of length N")
        check(_lib.lib().hipkkt_ldl_solve(self._h, ptr(x), ptr(b)), "hipkkt_ldl_solve")

    def solve_multi(self, K, X, B):
        """solve! on the columns of B (N, k) into X (N, k), both Fortran-ordered float64."""
        B = np.asfortranarray(B, dtype=np.float64)
        if X.dtype != np.float64 or X.shape != B.shape or B.shape[0] != self.N or not X.flags.f_contiguous:
            raise ValueError("X, B must be Fortran-ordered float64 (N, k)")
        check(_lib.lib().hipkkt_ldl_solve_multi(self._h, B.shape[1], ptr(X), ptr(B)), "hipkkt_ldl_solve_multi")

    def linear_solver_info(self):
        info = _lib.Info()
        check(_lib.lib().hipkkt_ldl_info(self._h, C.byref(info)), "hipkkt_ldl_info")
        return LinearSolverInfo("hipldl", 1, True, info.nnzK, info.nnzL)

    def perm(self):
        out = np.zeros(self.N, dtype=np.int64)
        check(_lib.lib().hipkkt_ldl_get_perm(self._h, ptr(out)), "hipkkt_ldl_get_perm")
        return out

    @property
    def fallbacks(self):
        out = np.zeros(2, dtype=np.int64)
        check(_lib.lib().hipkkt_ldl_fallbacks(self._h, ptr(out)), "hipkkt_ldl_fallbacks")
        return int(out[0]), int(out[1])
