"""Level A (hipkkt_ldl_*, no refinement) at every front-class boundary of the schedule, against exact answers.

The matrices of tests/front_shapes.py put a front of a chosen (nc, nb) exactly where a kernel class or a tile / slice /
block-size rule switches; x_true is known and b = K~ x_true is exact.  Every solve must meet
    forward error  |x - x_true|_inf / |x_true|_inf <= max(100 cond u, 10 x scipy's error on the same case)
    backward error |b - K~ x|_inf / (|K~|_inf |x|_inf + |b|_inf) <= 64 u   (long double)
Each group runs in ONE child process under a timeout (the HIPKKT_* knobs are read once per process, the schedule
summary of HIPKKT_VERBOSE goes to stderr), one child at a time.

Which BUILD of k_panel / k_schur a case meets here follows from its tree, by the overlap mode's three-launch rule
(csrc/schedule.cpp: admit_overlap): a designed tree is the front, a stick and the root, the stick merges into the root, and
the overlap builds (k_panel<BS, false, true>, k_schur<true, true>) run only where that root is wide enough to be cut into
chain links, so that three or more block-class launches end the schedule -- the cases with tall sticks (large nb, narrow
nc).  Every other case runs the plain builds (k_panel<BS, false, false>, k_schur<false, false>); test_shape_sweep asserts
which, per case.  The pipelined tile kernel k_schur<false, true> never runs here.  Every build at every edge, named by the
handle's own report -- plain, pipelined and overlap, the XCD tile order on and off -- is tests/test_gpu_factor_builds.py's."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import front_shapes as fs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fs.all_cases()

EPS, DELTA = 0.25, 1.0            # level-A dynamic regularisation of the pivot-rule cases
_BELOW = float(np.nextafter(0.25, 0.0))
# (value, sign): regularised, regularised, wrong sign, kept (the rule is a strict <), regularised, kept, regularised
PIVOT_VALUES = [(0.0, 1), (0.0, -1), (-0.5, 1), (0.25, 1), (_BELOW, 1), (-0.25, -1), (-_BELOW, -1)]


def _positions(nc):
    return sorted({p for p in (0, 15, 16, 31, 49, 96, nc - 1) if p < nc})


# pivot-rule cases: name -> (shape case, extra env of the child)
PIVOT_CASES = {
    "tiny_2_6": ({}, "tiny"),
    "wave_16_28": ({}, "one-wave"),
    "panel_nc33": ({}, "whole panel"),
    "chain_nc97": ({}, "chained panels (columns 49 and 96: the second link)"),
    "schur_nb193": ({"HIPKKT_PANEL_CAP": "6000"}, "row-sliced panel"),
}


def pivot_variants(name):
    """Variants of a pivot-rule case: enough that every value of PIVOT_VALUES lands in the case's front at least once."""
    npos = len(_positions(CASES[name][0][0][0]))
    return -(-len(PIVOT_VALUES) // npos)


def pivot_case(name, variant=0):
    """The shape case `name` with pivot-rule values at positions 0, 15, 16, 31, 49, 96 and the last column of its
    designed front (those that exist), the values of PIVOT_VALUES in turn from value npos * variant on."""
    c = fs.make_case(CASES[name][0], 7 + variant)
    cols = c.cols[0]
    pos = _positions(len(cols))
    shift = len(pos) * variant
    pivots = [(cols[p], *PIVOT_VALUES[(i + shift) % len(PIVOT_VALUES)]) for i, p in enumerate(pos)]
    assert any(v * s < EPS for _, v, s in pivots)
    fs.set_pivots(c, pivots, EPS, DELTA)
    return c, pivots, EPS, DELTA


def control_error(c):
    """Forward error against x_true of K~ of the exact solve of K x = b (the rule NOT applied): must be large."""
    try:
        x = fs.reference_solve(c, K=c.K)
    except RuntimeError:          # K itself singular
        return np.inf
    if not np.all(np.isfinite(x)):
        return np.inf
    return fs.errors(c, x)[0]


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
from cuclarabel_amd import _lib
from cuclarabel_amd.kktsolver import HipDirectLDLSolver
from tests import front_shapes as fs
from tests import test_gpu_front_shapes as g
for job in {jobs!r}:
    print("@@case", job["name"], file=sys.stderr, flush=True)
    if job.get("pivots"):
        c, pivots, eps, delta = g.pivot_case(job["name"], job.get("variant", 0))
        st = _lib.default_settings(ordering=_lib.ORDER_NATURAL, dynamic_regularization_eps=eps,
                                   dynamic_regularization_delta=delta)
    else:
        c = fs.make_case(g.CASES[job["name"]][0], 1)
        st = _lib.default_settings(ordering=_lib.ORDER_NATURAL)
    _lib.symbolic_analyse(c.K, ordering=_lib.ORDER_NATURAL)     # [levels] lines of the same structure (host only)
    h = HipDirectLDLSolver(c.K, c.dsigns, st)
    out = dict(name=job["name"], N=c.K.shape[0])
    if job.get("nan"):
        # a non-finite pivot in the designed front: refactor() reports it, no exception; a finite value repairs it
        k = c.cols[0][job["nan"]]
        q = int(c.K.indptr[k + 1] - 1)              # the diagonal: last entry of column k of the upper triangle
        assert c.K.indices[q] == k
        h.update_values([q], [np.nan])
        out["nan_refactor"] = h.refactor()
        h.update_values([q], [c.K.data[q]])
    out["refactor"] = h.refactor()
    x = np.zeros(c.K.shape[0])
    h.solve(None, x, c.b)
    out["fwd"], out["bwd"] = fs.errors(c, x)
    out["scipy_fwd"] = fs.errors(c, fs.reference_solve(c))[0]
    out["bound"] = fs.forward_bound(c, out["scipy_fwd"])
    if job.get("pivots"):
        out["control"] = g.control_error(c)
    if job.get("multi"):
        out["multi"] = g.multi_checks(h, c)
    out["fallbacks"] = list(h.fallbacks)
    print(json.dumps(out), flush=True)
    del h
"""


def _run(jobs, env=None, timeout=240):
    """Run the jobs in one child process; -> [(result dict, schedule dict, stderr of the job)]."""
    from tests.test_gpu_parity import _schedule_line
    e = dict(os.environ, HIPKKT_VERBOSE="1", HIPKKT_DUMP_LEVELS="1")
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, jobs=jobs)], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = [json.loads(line) for line in r.stdout.split("\n") if line.startswith("{")]
    errs = [chunk.split("\n", 1)[1] for chunk in r.stderr.split("@@case ")[1:]]
    assert len(res) == len(errs) == len(jobs), r.stderr[-3000:]
    out = []
    for d, err in zip(res, errs):
        assert "gave up" not in err, err
        sch = _schedule_line(err)
        sch["levels"] = [(int(m[2]), int(m[5]), int(m[6])) for m in _LEVEL.finditer(err)]
        out.append((d, sch, err))
    return out


_OVERLAP = re.compile(r"factorisation overlap: last (\d+) launches")
_LEVEL = re.compile(r"\[levels\]\s+(\d+):\s+(\d+) fronts \(\s*(\d+) f<=8,\s+(\d+) f<=64\) fmax\s+(\d+) ncmax\s+(\d+)")


def _expected_block_fronts(sch):
    """Block-class fronts of a tree whose levels each hold identical fronts (the shape table's design, checked by
    test_front_shapes_host): every level's fronts are (fmax, ncmax)."""
    return sum(cnt for cnt, f, nc in sch["levels"] if fs.klass(f, nc) == "block")


def _check(d):
    assert d["refactor"] is True, d
    assert d["fallbacks"] == [0, 0], d
    assert d["fwd"] <= d["bound"], d
    assert d["bwd"] <= fs.BWD_BOUND, d


def _report(tag, rows):
    """One line per case in the test log: the numbers the PR description quotes."""
    for d, sch, _ in rows:
        print(f"\n[{tag}] {d['name']:16s} N {d['N']:6d} block {sch['block_fronts']:5d} sliced {sch['sliced_fronts']:3d} "
              f"({sch['row_slices']} slices) fwd {d['fwd']:.2e} (bound {d['bound']:.2e}) bwd {d['bwd']:.2e}")


# ------------------------------------------------------------------------------------------------ a. shape sweep
def test_shape_sweep():
    names = list(fs.all_cases())
    rows = _run([{"name": n} for n in names])
    _report("shape", rows)
    sched = {d["name"]: s for d, s, _ in rows}
    for d, s, err in rows:
        _check(d)
        assert s["sliced_fronts"] == 0, (d["name"], s)
        # which builds ran, by the three-launch rule (see the module docstring): the overlap mode takes the trailing
        # block-class levels where there are three or more -- the chain links of a wide stick's root -- and nothing otherwise
        tail = 0
        for cnt, f, nc in reversed(s["levels"]):
            if fs.klass(f, nc) != "block":
                break
            tail += 1
        ov = int(_OVERLAP.search(err)[1])
        print(f"[shape] {d['name']:16s} levels {len(s['levels'])}, block-class at the top {tail}: overlap mode on the last {ov} launches")
        assert ov == (tail if tail >= 3 else 0), (d["name"], ov, s["levels"])
    # the designed front's class, read from the schedule: roots alone are the whole count
    for n in ("f1_root", "f2_root", "f8_root", "f9_root", "wave_39_0"):
        assert sched[n]["block_fronts"] == 0, (n, sched[n])
    assert sched["block_40_0"]["block_fronts"] == 2
    # f*nc + nb^2 <= 1536 at (16, 28) and not at (16, 29): one more block-class front, with the same tree above it
    assert sched["block_16_29"]["block_fronts"] == sched["wave_16_28"]["block_fronts"] + 1
    # merge_small: 128 one-wave fronts ride with the level's block-class launch, 129 get their own
    assert sched["merge_128"]["block_fronts"] == 129
    assert sched["merge_129"]["block_fronts"] == 1
    assert sched["solve_bs_1023"]["block_fronts"] == 1023 and sched["solve_bs_1024"]["block_fronts"] == 1024
    # every other case: the exact count, front by front, from the structure's levels -- the designed front included, so a
    # designed front that fell into the one-wave class would be one short
    for n in names:
        if not n.startswith("merge_"):
            assert sched[n]["block_fronts"] == _expected_block_fronts(sched[n]), (n, sched[n])


# ------------------------------------------------------------------------------------------------ b. forced paths
def _sliced_pair():
    """(40, 256) and (40, 257) on the same stick: the trees differ only in the designed front's last row."""
    st = fs.stick(40, 257)
    return {"slice_256": (fs.designed(40, 256, st=st), None, "block"), "slice_257": (fs.designed(40, 257, st=st), None, "block")}


CASES.update(_sliced_pair())


@pytest.mark.parametrize("overlap", ["1", "0"])
def test_row_slices_at_128_row_edges(overlap):
    # HIPKKT_PANEL_CAP 6000: a 40-column panel of 256 or 257 rows needs two slices for LDS (820 + 129 * 40 <= 6000),
    # and the schedule's 128-row preference then asks ceil(nb / 128): 256 rows -> 2 slices, 257 -> 3.  The rest of
    # both trees is the same.
    env = {"HIPKKT_PANEL_CAP": "6000", "HIPKKT_FACTOR_OVERLAP": overlap}
    rows = _run([{"name": "slice_256"}, {"name": "slice_257"}], env=env)
    _report(f"slices ov={overlap}", rows)
    for d, s, _ in rows:
        _check(d)
        assert s["sliced_fronts"] >= 1, s
    assert rows[1][1]["row_slices"] == rows[0][1]["row_slices"] + 1, (rows[0][1], rows[1][1])


@pytest.mark.parametrize("rows_env,tall", [("193", True), ("194", False)])
def test_tall_front_sweeps_at_the_edge(rows_env, tall):
    rows = _run([{"name": "bs_f193"}], env={"HIPKKT_SOLVE_TALL_ROWS": rows_env})
    _report(f"tall={rows_env}", rows)
    d, s, err = rows[0]
    _check(d)
    assert ("too tall for the block sweep kernels" in err) == tall, err


@pytest.mark.parametrize("env", [{"HIPKKT_NO_TOP": "1"}, {"HIPKKT_SOLVE_SLICE_KB": "4"}],
                         ids=["no_top", "slice_kb4"])
def test_forced_sweep_paths(env):
    names = ["schur_nb193", "trap_96_151", "trap_96_152", "chain_nc97", "merge_128"]
    rows = _run([{"name": n} for n in names], env=env)
    _report(next(iter(env)), rows)
    for d, _, _ in rows:
        _check(d)


# ------------------------------------------------------------------------------------------------ c. pivot rule
@pytest.mark.parametrize("name", list(PIVOT_CASES))
def test_pivot_rule_in_every_class(name):
    env, _ = PIVOT_CASES[name]
    rows = _run([{"name": name, "pivots": True, "variant": v} for v in range(pivot_variants(name))], env=env)
    _report(f"pivot {PIVOT_CASES[name][1]}", rows)
    for d, s, _ in rows:
        _check(d)
        assert d["control"] > 1e-3, d
        if env.get("HIPKKT_PANEL_CAP"):
            assert s["sliced_fronts"] >= 1, s


# ------------------------------------------------------------------------------------------------ e. non-finite pivot
CASES["nan_64_80"] = (fs.designed(64, 80), None, "block")


def test_nan_pivot_in_a_panel_front_then_recovers():
    rows = _run([{"name": "nan_64_80", "nan": 5}])
    _report("nan", rows)
    d, s, _ = rows[0]
    assert d["nan_refactor"] is False, d
    _check(d)


# ------------------------------------------------------------------------------------------------ f. column counts
NRHS = [2, 3, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257]


def multi_checks(h, c):
    """solve_multi, solve_multi_dev with ldb = N + 5 / ldx = N + 3 (padding untouched) and with X aliasing B: every
    column against its own solve (rel. 1e-12) and the bounds.  A zero column and a x 1e6 column ride along.
    Returns the worst (vs own solve, forward error / bound, backward error / bound) over all columns."""
    import ctypes as C
    import scipy.sparse.linalg as spla
    import torch
    from cuclarabel_amd import _lib
    N = c.K.shape[0]
    L = _lib.lib()
    Kd = fs.full(c.Kt).toarray().astype(np.longdouble)
    lu = spla.splu(fs.full(c.Kt).tocsc())
    knorm = np.longdouble(fs.norm_inf_sym(c.Kt))
    rng = np.random.default_rng(5)
    dev = torch.device("cuda")
    worst = [0.0, 0.0, 0.0]
    for k in NRHS:
        Xt = rng.standard_normal((N, k))
        Xt[:, 0] = 0.0
        Xt[:, -1] *= 1e6
        B = np.asfortranarray((Kd @ Xt.astype(np.longdouble)).astype(np.float64))
        ref = lu.solve(B)
        xinf = np.abs(Xt).max(axis=0)
        bound = np.maximum(100 * c.cond_bound * fs.U, 10 * np.abs(ref - Xt).max(axis=0) / np.maximum(xinf, 1e-300))
        single = np.zeros((N, k))
        for j in range(k):
            x = np.zeros(N)
            h.solve(None, x, B[:, j])
            single[:, j] = x
        assert np.all(single[:, 0] == 0.0)
        got = []
        X = np.zeros((N, k), order="F")
        h.solve_multi(None, X, B)
        got.append(X)
        dB = torch.zeros((k, N + 5), dtype=torch.float64, device=dev)     # column-major N x k, ld N + 5
        dB[:, :N] = torch.from_numpy(np.ascontiguousarray(B.T)).to(dev)
        dX = torch.full((k, N + 3), -7.25, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        rc = L.hipkkt_ldl_solve_multi_dev(h._h, k, C.c_void_p(dX.data_ptr()), N + 3, C.c_void_p(dB.data_ptr()), N + 5)
        assert rc == 0, L.hipkkt_last_error()
        torch.cuda.synchronize()
        dXh = dX.cpu().numpy()
        assert np.all(dXh[:, N:] == -7.25), (k, "padding rows of X were written")
        got.append(dXh[:, :N].T)
        dA = torch.from_numpy(np.ascontiguousarray(B.T)).to(dev)        # X aliasing B, ld = N
        torch.cuda.synchronize()
        rc = L.hipkkt_ldl_solve_multi_dev(h._h, k, C.c_void_p(dA.data_ptr()), N, C.c_void_p(dA.data_ptr()), N)
        assert rc == 0, L.hipkkt_last_error()
        torch.cuda.synchronize()
        got.append(dA.cpu().numpy().T)
        for G in got:
            assert np.all(G[:, 0] == 0.0), (k, "zero column")
            G, S, T, Bc = G[:, 1:], single[:, 1:], Xt[:, 1:], B[:, 1:]
            worst[0] = max(worst[0], float((np.abs(G - S).max(axis=0) / np.abs(S).max(axis=0)).max()))
            fwd = np.abs(G - T).max(axis=0) / np.abs(T).max(axis=0)
            worst[1] = max(worst[1], float((fwd / bound[1:]).max()))
            Gl = G.astype(np.longdouble)
            R = np.abs(Bc.astype(np.longdouble) - Kd @ Gl).max(axis=0)
            bwd = R / (knorm * np.abs(Gl).max(axis=0) + np.abs(Bc.astype(np.longdouble)).max(axis=0))
            worst[2] = max(worst[2], float((bwd / fs.BWD_BOUND).max()))
    return worst


@pytest.mark.parametrize("name,env", [("panel_nc33", {}), ("bs_f193", {"HIPKKT_SOLVE_TALL_ROWS": "193"})],
                         ids=["panel", "tall"])
def test_many_columns_at_level_A(name, env):
    rows = _run([{"name": name, "multi": True}], env=env, timeout=300)
    d, _, _ = rows[0]
    _check(d)
    rel, fwd, bwd = d["multi"]
    print(f"\n[multi {name}] worst vs own solve {rel:.2e}, forward / bound {fwd:.2f}, backward / bound {bwd:.2f}")
    assert rel <= 1e-12, d
    assert fwd <= 1.0 and bwd <= 1.0, d


# ------------------------------------------------------------------------------------------------ d. the count at level B
_LEVEL_B_CHILD = r"""
import json, sys
import numpy as np
import scipy.sparse as sp
sys.path.insert(0, {root!r})
from cuclarabel_amd import _lib
from cuclarabel_amd.cones import NonnegativeConeT
from cuclarabel_amd.kktsolver import HipKKTSolver
from tests.oracle_bindings import OracleKKT, default_settings as orc_settings
for n in {ns!r}:
    print("@@case", n, file=sys.stderr, flush=True)
    m = n
    I, J = np.triu_indices(n)
    P = sp.csc_matrix((np.zeros(I.size), (I, J)), shape=(n, n))       # dense pattern, every value an explicit 0
    A = sp.identity(m, format="csc")
    cones = [NonnegativeConeT(m)]
    ks = HipKKTSolver(P, A, cones, settings=_lib.default_settings(static_regularization_enable=0,
                                                                  ordering=_lib.ORDER_NATURAL))
    ks.profile_enable(True)
    ks.profile_reset()
    assert ks.kktsolver_update(np.ones(m))
    o = OracleKKT(P, A, cones, perm=ks.perm(), settings=orc_settings(static_reg_enable=0))
    o.set_identity_scaling()
    assert o.kktsolver_update()
    _, host = _lib.symbolic_analyse(o.K(), ordering=_lib.ORDER_NATURAL)
    rng = np.random.default_rng(n)
    rx, rz = rng.standard_normal(n), rng.standard_normal(m)
    ks.kktsolver_setrhs(rx, rz)
    o.kktsolver_setrhs(rx, rz)
    x, z = np.zeros(n), np.zeros(m)
    ok = ks.kktsolver_solve(x, z)
    oko, xo, zo = o.kktsolver_solve()
    scale = max(np.abs(xo).max(), np.abs(zo).max())
    print(json.dumps(dict(n=n, ok=bool(ok), oko=bool(oko), count=int(ks.profile()["dynamic_regularizations"]),
                          oracle=int(o.num_dyn_regularized), err=float(max(np.abs(x - xo).max(), np.abs(z - zo).max()) / scale),
                          rounds=int(ks.last_ir_iterations), oracle_rounds=int(o.last_ir_iters), info=ks.info, host=host,
                          fallbacks=list(ks.fallbacks))), flush=True)
    del ks
"""


@pytest.mark.parametrize("ns,env", [((40, 100, 200), {}), ((200,), {"HIPKKT_PANEL_CAP": "6000"})], ids=["panels", "sliced"])
def test_dynamic_regularisation_count_in_panel_chain_and_sliced_fronts(ns, env):
    """P = 0 with a DENSE pattern of explicit zeros, ORDER_NATURAL, no static regularisation: the x columns are dense
    fronts -- one panel at n = 40, chains of panels at 100 and 200, row slices under HIPKKT_PANEL_CAP --
    every x pivot is exactly 0 and every L entry among the x columns 0, so the sign rule fires exactly n times.  A slice
    that counted a pivot the first slice already counted, or a chain link that missed one, changes the count."""
    from tests.test_gpu_parity import _schedule_line
    e = dict(os.environ, HIPKKT_VERBOSE="1")
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _LEVEL_B_CHILD.format(root=ROOT, ns=list(ns))], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = [json.loads(line) for line in r.stdout.split("\n") if line.startswith("{")]
    errs = [chunk.split("\n", 1)[1] for chunk in r.stderr.split("@@case ")[1:]]
    assert len(res) == len(errs) == len(ns), r.stderr[-3000:]
    for d, err in zip(res, errs):
        n = d["n"]
        sch = _schedule_line(err)
        print(f"\n[level B n={n} {env}] count {d['count']} oracle {d['oracle']} err {d['err']:.2e} rounds {d['rounds']} "
              f"max_front {d['info']['max_front']} nlevels {d['info']['nlevels']} sliced {sch['sliced_fronts']}")
        assert "gave up" not in err, err
        # the explicit zeros survive the assembly: all n(n+1)/2 entries of P are in K, and the structure is the one the
        # host analysis finds for the oracle's K with them (without them every x column would be a front of 2 rows)
        assert d["info"]["nnzK"] == n * (n + 1) // 2 + 2 * n, d["info"]
        for key in ("max_front", "nsuper", "nlevels", "nnzL"):
            assert d["info"][key] == d["host"][key], (key, d["info"], d["host"])
        assert d["info"]["max_front"] > n, d["info"]
        assert d["ok"] and d["oko"], d
        assert d["count"] == n == d["oracle"], d
        assert d["err"] < 1e-9, d
        assert d["rounds"] == d["oracle_rounds"], d
        assert d["fallbacks"] == [0, 0], d
        if n > 96:
            assert d["info"]["nlevels"] >= 3, d["info"]          # the x block is a chain of panels
        if env:
            assert sch["sliced_fronts"] >= 1, sch
