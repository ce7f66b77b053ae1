"""The many-column sweeps (csrc/solve_kernels.hip, "several right-hand sides") UNREFINED, at every front class and
instance, against exact answers.

solve_multi with more than eight columns runs through kernels of its own -- k_fwd_wave_m / k_bwd_wave_m (one-wave and tiny
fronts), k_pull_leaves_m / k_bwd_leaf_m (one-column leaves pulled by their parents), k_fwd_block_m / k_bwd_block_m (MFMA,
block-class fronts) and k_permute_in / k_permute_out -- chosen by the padded column count KP and two knobs
(csrc/launch_shapes.hpp: multi_shape).  Here, per environment (one child process each: the knobs are read once), every
case of GROUPS is solved with k = 9, 17, 33, 64, 65, 128, 129, 256 and 257 known columns (KP = 16 .. 272) through both entries:

    a. level A, column-major (hipkkt_ldl_solve_multi_dev: A.b == nullptr, a permute pass on each side) with ldb = N + 5 and
       ldx = N + 3 -- the padding must stay untouched -- and with X aliasing B;
    b. level B, row-major, refinement off (kktsolver_solve_multi_dev on the all-signs-+1 variant of the pattern: the forward
       kernels read B through the permutation, the three backward kernels store out[perm[c]] themselves).  No row of these
       matrices comes near kLongRow = 4096 entries, so the image has no long row and the entry is the row-major one -- asserted
       from the verbose line; ir == 0 everywhere.

The instance taken is ASSERTED from the "[hipkkt] many-column sweep:" line of every call against the table typed into
tests/test_multi_sweeps_host.py, the pulled rows of the leaf cases from the "contribution rows pulled" line against the
numbers their construction gives (tests/pulled_leaf_shapes.py: solve_cases).

Columns: known X_true, B = K X_true in long double rounded once; column 0 is zero, the last one x 1e6, column k - 2 a bit copy
of column 1.  Every column of every call meets front_shapes' bounds -- forward error <= max(100 cond u, 10 x scipy's error
on that column), long-double backward error <= 64 u; the zero column is exactly zero; column k - 2 equals column 1 BIT FOR
BIT (within one call every column block runs the same instance and no kernel's arithmetic depends on the column's place:
lanes and MFMA output columns are independent chains of the same operations); fallbacks == (0, 0).  In the default
environment columns 1, k // 2 and k - 1 are also compared with their own single-column solves at rel. 1e-12 (the figure of
test_gpu_front_shapes.multi_checks).

Across environments: pull_off against default is held to the bounds, not to bits -- with the leaves pulled a parent row's
terms are summed per receiving row first (k_pull_leaves_m) and enter its gather list as ONE stored contribution, without
them each leaf's term is a contribution of its own: another order of the same sum.

The references (scipy's LU, the long-double products, the bounds) are computed once per session in this process; the
children get the right-hand sides in a file.  After a child that faulted, aborted or ran out of time no further child is
started: the remaining items fail at once."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import front_shapes as fs
from tests import pulled_leaf_shapes as pls
from tests.test_multi_sweeps_host import ENVS, EXPECT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (9, 17, 33, 64, 65, 128, 129, 256, 257)
SAMPLE = lambda k: (1, k // 2, k - 1)          # noqa: E731  (columns compared with their own single solves)

_SPECS = fs.multi_specs()
_LEAF = pls.solve_cases()
GROUPS = {
    "small": ["tiny_n9", "tiny_n33", "wave9_n5", "wave39_n5", "wave_16_28_n5", "wave_1_38_n5", "wc_roots", "wc_designed"],
    "mixed": ["mixed_few", "mixed_129", "tall_mixed"],
    "panels": ["panel_nc15", "panel_nc17", "panel_nc33", "panel_nc95", "panel_nc96", "schur_nb1", "schur_nb65"],
    "wide": ["bs_f129", "trap_96_151", "chain_nc97"],
    "slices_a": ["slice_nt1", "slice_nt2"],
    "slices_b": ["slice_nt3", "slice_nt5", "slice_nt6"],
    "leaves_a": ["heights_16_28", "heights_16_29", "heights_40_65", "gather_17_24"],
    "leaves_b": ["counts_40_65", "counts_16_28", "slots_40_65", "slots_16_28", "ride_40_65"],
}
assert sorted(n for g in GROUPS.values() for n in g) == sorted(list(_SPECS) + list(_LEAF))


def make(name, level):
    """The case's matrix: level A with random signs (seed 1), level B with every sign +1 (seed 2: SPD and diagonally
    dominant, P of a problem without constraints).  Deterministic: the children rebuild it."""
    seed, signs = (1, None) if level == "A" else (2, "ones")
    if name in _SPECS:
        N = fs.layout(_SPECS[name])[2]
        return fs.make_case(_SPECS[name], seed, signs=None if signs is None else np.ones(N, dtype=np.int64))
    cols, rows, _ = _LEAF[name]
    N = cols[-1][-1] + 1
    return pls.make_case(cols, rows, seed, signs=None if signs is None else np.ones(N, dtype=np.int64))


# ------------------------------------------------------------------------------------------------ references
_REF = {}


def reference(name):
    """Per level and k: X_true, B (long double, rounded once) and the per-column forward bound; once per session."""
    import scipy.sparse.linalg as spla
    if name in _REF:
        return _REF[name]
    ref = {}
    for level in "AB":
        c = make(name, level)
        N = c.K.shape[0]
        assert np.diff(fs.full(c.K).tocsr().indptr).max() <= 4096, "a long row: level B would not take the row-major entry"
        lu = spla.splu(fs.full(c.Kt).tocsc(), permc_spec="COLAMD")
        per_k = {}
        for k in KS:
            X = np.random.default_rng(7000 + 10 * k + (level == "B")).standard_normal((N, k))
            X[:, 0] = 0.0
            X[:, -1] *= 1e6
            X[:, k - 2] = X[:, 1]
            B = fs.symmetric_matmat_ld(c.K, X).astype(np.float64)
            assert np.array_equal(B[:, k - 2], B[:, 1]) and not np.any(B[:, 0])
            sfwd = fs.errors_columns(c, lu.solve(B), X, B)[0]
            per_k[k] = dict(X=X, B=B, bound=np.maximum(100.0 * c.cond_bound * fs.U, 10.0 * sfwd))
        ref[level] = dict(case=c, k=per_k)
    _REF[name] = ref
    return ref


# ------------------------------------------------------------------------------------------------ the children
_CHILD = r"""
import ctypes as C, json, sys
import numpy as np
import scipy.sparse as sp
import torch
sys.path.insert(0, {root!r})
from cuclarabel_amd import _lib
from cuclarabel_amd.kktsolver import HipDirectLDLSolver, HipKKTSolver
from tests import test_gpu_multi_sweeps as g
dev = torch.device("cuda")
L = _lib.lib()
rhs = np.load({rhs!r})
singles = {singles!r}
out = {{}}
for name in {names!r}:
    print("@@case", name, file=sys.stderr, flush=True)
    c = g.make(name, "A")
    N = c.K.shape[0]
    print("@@A", file=sys.stderr, flush=True)
    h = HipDirectLDLSolver(c.K, c.dsigns, _lib.default_settings(ordering=_lib.ORDER_NATURAL))
    rec = dict(name=name, N=N, refactor=h.refactor(), pad_ok=True)
    for k in g.KS:
        print("@@k", k, file=sys.stderr, flush=True)
        B = rhs[f"{{name}}/A{{k}}"]
        dB = torch.zeros((k, N + 5), dtype=torch.float64, device=dev)          # column-major N x k, ld N + 5
        dB[:, :N] = torch.from_numpy(np.ascontiguousarray(B.T)).to(dev)
        dX = torch.full((k, N + 3), -7.25, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        rc = L.hipkkt_ldl_solve_multi_dev(h._h, k, C.c_void_p(dX.data_ptr()), N + 3, C.c_void_p(dB.data_ptr()), N + 5)
        assert rc == 0, L.hipkkt_last_error()
        torch.cuda.synchronize()
        X = dX.cpu().numpy()
        rec["pad_ok"] = rec["pad_ok"] and bool(np.all(X[:, N:] == -7.25)) and bool(np.all(dB.cpu().numpy()[:, N:] == 0.0))
        out[f"{{name}}/Acm{{k}}"] = X[:, :N].T.copy()
        dA = torch.from_numpy(np.ascontiguousarray(B.T)).to(dev)                # X aliasing B, ld = N
        torch.cuda.synchronize()
        rc = L.hipkkt_ldl_solve_multi_dev(h._h, k, C.c_void_p(dA.data_ptr()), N, C.c_void_p(dA.data_ptr()), N)
        assert rc == 0, L.hipkkt_last_error()
        torch.cuda.synchronize()
        out[f"{{name}}/Aal{{k}}"] = dA.cpu().numpy().T.copy()
        if singles:
            print("@@single", file=sys.stderr, flush=True)
            S = np.zeros((N, 3))
            for q, j in enumerate(g.SAMPLE(k)):
                x = np.zeros(N)
                h.solve(None, x, np.ascontiguousarray(B[:, j]))
                S[:, q] = x
            out[f"{{name}}/As{{k}}"] = S
    rec["fallbacksA"] = list(h.fallbacks)
    del h
    print("@@B", file=sys.stderr, flush=True)
    c = g.make(name, "B")
    st = _lib.default_settings(static_regularization_enable=0, iterative_refinement_enable=0, ordering=_lib.ORDER_NATURAL)
    ks = HipKKTSolver(c.K, sp.csc_matrix((0, N)), [], settings=st)
    assert ks.N == N
    rec["update"] = bool(ks.kktsolver_update(np.zeros(0)))
    rec["ir"], rec["ok"] = {{}}, {{}}
    for k in g.KS:
        print("@@k", k, file=sys.stderr, flush=True)
        B = rhs[f"{{name}}/B{{k}}"]
        drx = torch.from_numpy(np.ascontiguousarray(B.T)).to(dev)
        dlx = torch.full((k, N), -7.25, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ok, ir = ks.kktsolver_solve_multi_dev(k, drx.data_ptr(), 0, dlx.data_ptr(), 0)
        torch.cuda.synchronize()
        out[f"{{name}}/Brm{{k}}"] = dlx.cpu().numpy().T.copy()
        rec["ir"][k], rec["ok"][k] = [int(v) for v in ir], bool(ok)
        if singles:
            print("@@single", file=sys.stderr, flush=True)
            S = np.zeros((N, 3))
            for q, j in enumerate(g.SAMPLE(k)):
                ks.kktsolver_setrhs(np.ascontiguousarray(B[:, j]), np.zeros(0))
                x = np.zeros(N)
                assert ks.kktsolver_solve(x, None)
                S[:, q] = x
            out[f"{{name}}/Bs{{k}}"] = S
    rec["fallbacksB"] = list(ks.fallbacks)
    del ks
    print(json.dumps(rec), flush=True)
np.savez({npz!r}, **out)
"""

_SWEEP = re.compile(r"\[hipkkt\] many-column sweep: KP (\d+) entry (cm|rm) add (\d) wave_v (\d+) leaf_v (\d+) block_bs (\d+) "
                    r"block_ct (\d+) pull_rows (\d+)")
_PULLED = re.compile(r"\[hipkkt\] many-column sweeps: (\d+) of (\d+) contribution rows pulled from one-column leaves into (\d+) sums")
_DEAD = []           # set by the first child that faulted, aborted or ran out of time: nothing is started after it
_RHS = {}


def sweep_lines(text):
    return [dict(KP=int(m[1]), entry=m[2], add=int(m[3]), shape=(int(m[4]), int(m[5]), int(m[6]), int(m[7])), pull_rows=int(m[8]))
            for m in _SWEEP.finditer(text)]


def _rhs_file(group, tmp_path_factory):
    if group not in _RHS:
        path = str(tmp_path_factory.mktemp("multi_rhs") / f"{group}.npz")
        np.savez(path, **{f"{name}/{lvl}{k}": reference(name)[lvl]["k"][k]["B"] for name in GROUPS[group] for lvl in "AB" for k in KS})
        _RHS[group] = path
    return _RHS[group]


def run_child(env_id, names, tmp_path_factory, script=_CHILD, rhs=None, timeout=300):
    """One child process under ENVS[env_id] for the named cases -> (records by case, arrays, stderr by case)."""
    if _DEAD:
        pytest.fail(f"not started: an earlier child ended abnormally ({_DEAD[0]})")
    group = names[0]
    npz = str(tmp_path_factory.mktemp("multi") / f"{env_id}_{group}.npz")
    e = dict(os.environ, HIPKKT_VERBOSE="1")
    e.update(ENVS[env_id])
    code = script.format(root=ROOT, names=names, npz=npz, rhs=rhs, singles=env_id == "default")
    try:
        r = subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as ex:
        _DEAD.append(f"{env_id}/{group}: timeout")
        err = ex.stderr.decode(errors="replace") if isinstance(ex.stderr, bytes) else (ex.stderr or "")
        pytest.fail(f"child ran out of time; last markers: {[l for l in err.splitlines() if l.startswith('@@')][-4:]}")
    if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in r.stderr or "HSA_STATUS_ERROR" in r.stderr:
        _DEAD.append(f"{env_id}/{group}: exit {r.returncode}")
    assert r.returncode == 0, (r.returncode, [l for l in r.stderr.splitlines() if l.startswith("@@")][-4:], r.stdout[-1000:], r.stderr[-3000:])
    assert "gave up" not in r.stderr, r.stderr[-3000:]
    recs = {d["name"]: d for d in (json.loads(line) for line in r.stdout.split("\n") if line.startswith("{"))}
    errs = {}
    for chunk in r.stderr.split("@@case ")[1:]:
        name, rest = chunk.split("\n", 1)
        errs[name.strip()] = rest
    assert set(recs) == set(errs) == set(names)
    return recs, np.load(npz), errs


# ------------------------------------------------------------------------------------------------ checks
def _k_chunks(part):
    """{k: (text of the many-column calls, text of the single solves)} of one level's stderr."""
    out = {}
    for s in part.split("@@k ")[1:]:
        head, rest = s.split("\n", 1)
        multi, _, single = rest.partition("@@single")
        out[int(head)] = (multi, single)
    return out


def check_lines(env_id, name, err):
    """The instance lines of every call and the pulled-rows line of both handles; -> the set of instances named."""
    partA, partB = err.split("@@B", 1)
    named = set()
    exp_leaf = _LEAF[name][2] if name in _LEAF else None
    pulled = [tuple(int(x) for x in m.groups()) for m in _PULLED.finditer(err)]
    assert len(pulled) == 2, (env_id, name, pulled)               # one engine per level
    if exp_leaf is not None:
        want = (0, exp_leaf["b"], 0) if env_id == "pull_off" else (exp_leaf["a"], exp_leaf["b"], exp_leaf["c"])
        assert pulled == [want, want], (env_id, name, pulled, want)
    if env_id == "pull_off":
        assert all(p[0] == 0 and p[2] == 0 for p in pulled), (name, pulled)
    for level, part, entry, ncalls in (("A", partA, "cm", 2), ("B", partB, "rm", 1)):
        chunks = _k_chunks(part)
        assert sorted(chunks) == sorted(KS), (env_id, name, level, sorted(chunks))
        for k, (multi, single) in chunks.items():
            KP = (k + 15) & ~15
            lines = sweep_lines(multi)
            assert len(lines) == ncalls, (env_id, name, level, k, lines)
            assert not sweep_lines(single), "a single-column solve went through the many-column sweeps"
            for ln in lines:
                tag = (env_id, name, level, k, ln)
                assert ln["KP"] == KP and ln["entry"] == entry and ln["add"] == 0, tag
                assert ln["shape"] == EXPECT[env_id][KP], (tag, EXPECT[env_id][KP])
                assert ln["pull_rows"] == pulled[0][2], tag
                named.add((KP,) + ln["shape"])
    return named, pulled[0]


def check_numbers(env_id, name, rec, arr):
    """Every column of every call of one case; -> worst (forward / bound, backward / bound, vs own single solve)."""
    ref = reference(name)
    assert rec["refactor"] is True and rec["update"] is True and rec["pad_ok"] is True, rec
    assert rec["fallbacksA"] == [0, 0] and rec["fallbacksB"] == [0, 0], rec
    worst = [0.0, 0.0, 0.0]
    for k in KS:
        assert rec["ok"][str(k)] is True and rec["ir"][str(k)] == [0] * k, (env_id, name, k, rec["ir"][str(k)])
        for level, keys in (("A", ("Acm", "Aal")), ("B", ("Brm",))):
            c, R = ref[level]["case"], ref[level]["k"][k]
            seen = []
            for key in keys:
                G = arr[f"{name}/{key}{k}"]
                tag = (env_id, name, key, k)
                assert G.shape == R["X"].shape and np.all(np.isfinite(G)), tag
                assert not np.any(G[:, 0]), (tag, "the zero column")
                assert np.array_equal(G[:, k - 2], G[:, 1]), (tag, "column k - 2 is not a bit copy of column 1",
                                                              float(np.abs(G[:, k - 2] - G[:, 1]).max()))
                if env_id == "default":
                    S = arr[f"{name}/{level}s{k}"]
                    cols = list(SAMPLE(k))
                    rel = np.abs(G[:, cols] - S).max(axis=0) / np.abs(S).max(axis=0)
                    worst[2] = max(worst[2], float(rel.max()))
                    assert rel.max() <= 1e-12, (tag, "against the columns' own single solves", rel)
                if any(np.array_equal(G, H) for H in seen):
                    continue                                     # the same bits: the same errors
                seen.append(G)
                fwd, bwd = fs.errors_columns(c, G, R["X"], R["B"])
                rf, rb = fwd[1:] / R["bound"][1:], bwd[1:] / fs.BWD_BOUND
                worst[0], worst[1] = max(worst[0], float(rf.max())), max(worst[1], float(rb.max()))
                assert rf.max() <= 1.0, (tag, "forward error", int(rf.argmax()) + 1, float(rf.max()))
                assert rb.max() <= 1.0, (tag, "backward error", int(rb.argmax()) + 1, float(rb.max()))
    return worst


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("env_id", list(ENVS))
def test_many_column_sweeps_unrefined(env_id, group, tmp_path_factory):
    recs, arr, errs = run_child(env_id, GROUPS[group], tmp_path_factory, rhs=_rhs_file(group, tmp_path_factory))
    named, worst = set(), [0.0, 0.0, 0.0]
    for name in GROUPS[group]:
        nm, pulled = check_lines(env_id, name, errs[name])
        named |= nm
        w = check_numbers(env_id, name, recs[name], arr)
        print(f"\n[multi {env_id}] {name:16s} N {recs[name]['N']:5d} pulled {pulled[0]} of {pulled[1]} rows into {pulled[2]} sums; "
              f"fwd/bound {w[0]:.3f} bwd/bound {w[1]:.3f} vs single {w[2]:.1e}")
        worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"\n[multi {env_id}] {group}: worst fwd/bound {worst[0]:.3f} bwd/bound {worst[1]:.3f} vs single {worst[2]:.1e}")
    for KP, wv, lv, bs, ct in sorted(named):
        print(f"[multi {env_id}] {group}: KP {KP:3d} -> wave V={wv} leaf V={lv} block {bs}/{ct}")
    assert {n[0] for n in named} == {(k + 15) & ~15 for k in KS}


# ------------------------------------------------------------------------------------------------ the `add` store
# In refinement rounds the three backward kernels store out = x + add themselves (k_bwd_wave_m, k_bwd_leaf_m,
# k_bwd_block_m).  Refinement hides small errors, so these runs are built as tests/test_gpu_refinement.py builds its own:
# static regularisation 1e-4, reltol 0, an absolute tolerance chosen on the CPU (residual_reference.MULTI_REFINE) such that
# the round count of every column is a property of the problem; a wrong `add` row shows as a round count or a residual.
_REFINE = {}


def refine_problem(name):
    """(triu P, symmetric image, abstol) of a refinement case: the level-B matrix of the case, scaled."""
    from tests import residual_reference as rr
    scale, abstol = rr.MULTI_REFINE[name]
    c = make(name, "B")
    P = c.K.copy()
    P.data = P.data * scale
    return P, rr.sym_from_triu(P.indptr, P.indices, P.data), abstol


def refine_predictions(name):
    """Per (k, scales, seed) of MULTI_REFINE_COLUMNS: (B, predictions), with predict()'s conditions asserted."""
    from tests import residual_reference as rr
    if name not in _REFINE:
        P, K, abstol = refine_problem(name)
        N = K.shape[0]
        fac = rr.HostFactor(K, np.ones(N), rr.REG_EPS)
        out = []
        for k, scales, seed in rr.MULTI_REFINE_COLUMNS:
            B = rr.refinement_columns(N, k, seed, scales)
            preds = [rr.refine_loop(K, fac, B[:, j], abstol, 0.0, 5.0, 20) for j in range(k)]
            assert preds[0]["norms"][0] >= 1e4 * abstol, ("the first residual must need refinement by 1e4", name, preds[0]["norms"], abstol)
            for j, p in enumerate(preds):
                assert p["ok"] and p["margin"] >= 4.0, ("a decision too close to its threshold", name, k, j, p["margin"], p["norms"])
            out.append((k, B, preds))
        _REFINE[name] = (K, abstol, out)
    return _REFINE[name]


_REFINE_CHILD = r"""
import json, sys
import numpy as np
import scipy.sparse as sp
import torch
sys.path.insert(0, {root!r})
from cuclarabel_amd import _lib
from cuclarabel_amd.kktsolver import HipKKTSolver
from tests import residual_reference as rr
from tests import test_gpu_multi_sweeps as g
dev = torch.device("cuda")
out = {{}}
for name in {names!r}:
    print("@@case", name, file=sys.stderr, flush=True)
    P, K, abstol = g.refine_problem(name)
    N = P.shape[0]
    st = _lib.default_settings(ordering=_lib.ORDER_NATURAL, **rr.multi_refine_settings(abstol))
    ks = HipKKTSolver(P, sp.csc_matrix((0, N)), [], settings=st)
    rec = dict(name=name, N=N, update=bool(ks.kktsolver_update(np.zeros(0))), reg=float(ks.diagonal_regularizer), ir={{}}, ok={{}})
    Kdev = rr.sym_of(ks)
    rec["same_K"] = bool((abs(Kdev - K)).nnz == 0)
    for k, scales, seed in rr.MULTI_REFINE_COLUMNS:
        print("@@k", k, file=sys.stderr, flush=True)
        B = rr.refinement_columns(N, k, seed, scales)
        drx = torch.from_numpy(np.ascontiguousarray(B.T)).to(dev)
        dlx = torch.full((k, N), -7.25, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ok, ir = ks.kktsolver_solve_multi_dev(k, drx.data_ptr(), 0, dlx.data_ptr(), 0)
        torch.cuda.synchronize()
        out[f"{{name}}/X{{k}}"] = dlx.cpu().numpy().T.copy()
        rec["ir"][k], rec["ok"][k] = [int(v) for v in ir], bool(ok)
    rec["fallbacks"] = list(ks.fallbacks)
    del ks
    print(json.dumps(rec), flush=True)
np.savez({npz!r}, **out)
"""


def test_add_store_in_refinement_rounds(tmp_path_factory):
    """One wave-only case, one with pulled leaves under a block-class parent and panel_nc33, k = 9 with every column active
    (round 1: all accept, the buffer swap; round 2: some, launch_accept_columns_rm) and k = 33 with the mixed columns."""
    from tests import residual_reference as rr
    names = list(rr.MULTI_REFINE)
    recs, arr, errs = run_child("default", names, tmp_path_factory, script=_REFINE_CHILD)
    for name in names:
        K, abstol, runs = refine_predictions(name)
        rec = recs[name]
        assert rec["update"] is True and rec["reg"] == rr.REG_EPS and rec["same_K"] is True and rec["fallbacks"] == [0, 0], rec
        if name in _LEAF:
            e = _LEAF[name][2]
            assert [tuple(int(x) for x in m.groups()) for m in _PULLED.finditer(errs[name])] == [(e["a"], e["b"], e["c"])] and e["a"] > 0
        chunks = {int(s.split("\n", 1)[0]): s for s in errs[name].split("@@k ")[1:]}
        for k, B, preds in runs:
            KP = (k + 15) & ~15
            rounds = [p["rounds"] for p in preds]
            lines = sweep_lines(chunks[k])
            tag = (name, k, rounds, rec["ir"][str(k)], lines)
            assert rec["ok"][str(k)] is True and rec["ir"][str(k)] == rounds, tag
            # one sweep pair for the first solve, one per round while any column is active -- those with the add store
            assert [ln["add"] for ln in lines] == [0] + [1] * max(rounds), tag
            assert all(ln["entry"] == "rm" and ln["KP"] == KP and ln["shape"] == EXPECT["default"][KP] for ln in lines), tag
            if k == 9:
                assert min(rounds) >= 1 and min(rounds) < max(rounds), tag          # round 1: the swap; round 2: the kernel
            else:
                assert min(rounds) == 0 < max(rounds), tag
            X = arr[f"{name}/X{k}"]
            worst = 0.0
            for j, p in enumerate(preds):
                if not np.any(B[:, j]):
                    assert not np.any(X[:, j]), (name, k, j, "zero column")
                    continue
                assert p["stop"] == "tol", (name, k, j, p["stop"])
                true = np.abs(rr.residual_exact(K, X[:, j], B[:, j])[0]).max()
                limit = abstol + rr.residual_bound(K, X[:, j], B[:, j]).max()
                worst = max(worst, float(true / limit))
                assert true <= limit, (name, k, j, true, limit, p["norms"])
            print(f"\n[multi add] {name:14s} k {k:2d}: rounds {rounds} device {rec['ir'][str(k)]} add-1 sweeps {max(rounds)} "
                  f"worst residual / (abstol + bound) {worst:.3f}")
