"""The tree solves on EVERY sweep path, front class and column count, without refinement, against exact answers.

tests/test_gpu_front_shapes.py does this for the factorisation; its trees are two or three launches tall and its one
solve per case is the one right after refactor().  Here the forests of tests/front_shapes.py (sweep_table: tiny and
one-wave fronts at the packing edges of their kernels, all three classes in one level, trees tall enough for a chained
range below a persistent set) go through every way plan_sweep (csrc/schedule.cpp) can split a sweep, forced by the
HIPKKT_* knobs and ASSERTED from the "[hipkkt] sweep plan" line of HIPKKT_VERBOSE:

    a. level A (hipkkt_ldl_*): refactor(), then four solves with four known x_true -- the first with W still pending,
       the others in the steady state, the epoch-carrying flags and counters on their second to fourth use;
    b. level B (hipkkt_kkt_*), refinement off, 1, 2, 3, 4, 5 and 8 columns through kktsolver_solve_multi_dev: the NR = 2
       and NR = 4 instances of the sweep kernels; every column bit for bit its own single solve;
    c. chained sweeps and the legacy record layout bit for bit against the per-level sweep of the packed layout.

Every solve meets front_shapes' bounds: forward error <= max(100 cond u, 10 x scipy's error), long-double backward
error <= 64 u.  One child process per environment (the knobs are read once per process), each under a timeout; the
references (scipy's LU, the right-hand sides in long double) are computed once in this process and shared.

Unrefined level-B solves go level by level in every environment: kkt_solve_core reads no abort word back on that path,
so it may not start kernels with bounded waits.  The NR = 2 / 4 instances checked here are therefore the per-level
kernels' (level, small, block, in both record layouts and both workgroup sizes); the chained and persistent kernels'
two- and four-column instances stay with the refined tests (test_two_column_sweeps.py, test_small_batches_*)."""
import dataclasses
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import front_shapes as fs
from tests.test_gpu_front_shapes import _check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fs.sweep_cases()
TALL = ("tall_wave", "tall_mixed")
KS = (1, 2, 3, 4, 5, 8)
NSOLVES = 4

_PER_LEVEL = {"HIPKKT_NO_TOP": "1", "HIPKKT_CHAIN": "0"}
_CHAIN_ROOT = {"HIPKKT_CHAIN_TOP": "0"}
ENVS = {
    "default": {},                                  # (on the tall trees: the issue's "chain_below")
    "per_level": _PER_LEVEL,
    "unmerged": dict(_PER_LEVEL, HIPKKT_NO_LEVEL_MERGE="1"),
    "merge0": dict(_PER_LEVEL, HIPKKT_MERGE_SMALL="0"),
    "bs128": dict(_PER_LEVEL, HIPKKT_BS128_COUNT="1"),
    "chain_root": _CHAIN_ROOT,
    "legacy_per_level": dict(_PER_LEVEL, HIPKKT_PACKED="0"),
    "legacy_chain_root": dict(_CHAIN_ROOT, HIPKKT_PACKED="0"),
    "top_cap3": {"HIPKKT_TOP_CAP": "3"},
    "top_512": {"HIPKKT_TOP_TALL": "0"},
}


# ------------------------------------------------------------------------------------------------ the sweep-plan line
_PLAN = re.compile(r"\[hipkkt\] sweep plan: nr (\d+) per-level \[0,(\d+)\) chained \[(\d+),(\d+)\) persistent \[(\d+),(\d+)\) "
                   r"grid (\d+) kernel (\w+) threads (\d+) w_pending (\d) packed (\d)")
_LAUNCH = re.compile(r"\[hipkkt\] sweep launch (\d+)(?:\+(\d+))? level (\d+): family (\S+) solve_bs (\d+) fmax (\d+) "
                     r"block (\d+) wave (\d+) tiny (\d+)")


def _sweep_plans(stderr):
    """The HIPKKT_VERBOSE sweep-plan lines (describe, csrc/schedule.cpp; printed by enqueue_solve), one dict per line, each with the per-level
    launch lines (HIPKKT_VERBOSE=2) that follow it."""
    plans = []
    for line in stderr.split("\n"):
        m = _PLAN.search(line)
        if m:
            g = m.groups()
            plans.append(dict(nr=int(g[0]), per_level=(0, int(g[1])), chained=(int(g[2]), int(g[3])),
                              persistent=(int(g[4]), int(g[5])), grid=int(g[6]), kernel=g[7], threads=int(g[8]),
                              w_pending=g[9] == "1", packed=g[10] == "1", launches=[]))
            continue
        m = _LAUNCH.search(line)
        if m and plans:
            g = m.groups()
            plans[-1]["launches"].append(dict(level=int(g[2]), family=g[3], solve_bs=int(g[4]), fmax=int(g[5]),
                                              block=int(g[6]), wave=int(g[7]), tiny=int(g[8]), merged=g[1] is not None))
    return plans


def _empty(r):
    return r[0] == r[1]


# ------------------------------------------------------------------------------------------------ problems, references
def problem(name):
    """Level A: the case's matrix with NSOLVES known solutions; level B: the same pattern with every sign +1 (SPD and
    diagonally dominant: P of a problem without constraints) and k known columns for every k of KS, one of them zero and
    one x 1e6 (k >= 2).  Right-hand sides in long double, rounded once.  Deterministic: the children rebuild it."""
    spec = CASES[name][0]
    A = fs.make_case(spec, 1)
    N = A.K.shape[0]
    XA = np.empty((N, NSOLVES))
    XA[:, 0] = A.x_true
    for i in range(1, NSOLVES):
        XA[:, i] = np.random.default_rng(100 + i).standard_normal(N)
    BA = np.stack([A.b] + [fs.symmetric_matvec_ld(A.K, XA[:, i]).astype(np.float64) for i in range(1, NSOLVES)], axis=1)
    B = fs.make_case(spec, 2, signs=np.ones(N, dtype=np.int64))
    XB, BB = {}, {}
    for k in KS:
        X = np.random.default_rng(1000 + k).standard_normal((N, k))
        if k >= 2:
            X[:, 0] = 0.0
            X[:, -1] *= 1e6
        XB[k] = X
        BB[k] = np.stack([fs.symmetric_matvec_ld(B.K, X[:, j]).astype(np.float64) for j in range(k)], axis=1)
    return dict(A=A, XA=XA, BA=BA, B=B, XB=XB, BB=BB)


_REF = {}


def reference(name):
    """problem(name) plus scipy's forward error for every column: computed once, shared by every environment."""
    import scipy.sparse.linalg as spla
    if name not in _REF:
        p = problem(name)
        for lvl, cols in (("A", [("A", i, p["XA"][:, i], p["BA"][:, i]) for i in range(NSOLVES)]),
                          ("B", [(k, j, p["XB"][k][:, j], p["BB"][k][:, j]) for k in KS for j in range(k)])):
            c = p[lvl]
            lu = spla.splu(fs.full(c.Kt).tocsc(), permc_spec="COLAMD")
            p["cases" + lvl] = {}
            for key, j, x, b in cols:
                cj = dataclasses.replace(c, x_true=x, b=b)
                sfwd = fs.errors(cj, lu.solve(b))[0] if np.any(x) else 0.0
                p["cases" + lvl][(key, j)] = (cj, fs.forward_bound(cj, sfwd))
        _REF[name] = p
    return _REF[name]


# ------------------------------------------------------------------------------------------------ the children
_CHILD = r"""
import json, sys
import numpy as np
import scipy.sparse as sp
import torch
sys.path.insert(0, {root!r})
from cuclarabel_amd import _lib
from cuclarabel_amd.kktsolver import HipDirectLDLSolver, HipKKTSolver
from tests import test_gpu_sweep_paths as g
dev = torch.device("cuda")
out = {{}}
for name in {names!r}:
    p = g.problem(name)
    c = p["A"]
    N = c.K.shape[0]
    print("@@A", name, file=sys.stderr, flush=True)
    h = HipDirectLDLSolver(c.K, c.dsigns, _lib.default_settings(ordering=_lib.ORDER_NATURAL))
    rec = dict(name=name, N=N, refactor=h.refactor())
    XA = np.zeros((N, g.NSOLVES))
    for i in range(g.NSOLVES):
        x = np.zeros(N)
        h.solve(None, x, p["BA"][:, i])
        XA[:, i] = x
    out[name + "/A"] = XA
    rec["fallbacksA"] = list(h.fallbacks)
    del h
    print("@@B", name, file=sys.stderr, flush=True)
    c = p["B"]
    st = _lib.default_settings(static_regularization_enable=0, iterative_refinement_enable=0, ordering=_lib.ORDER_NATURAL)
    ks = HipKKTSolver(c.K, sp.csc_matrix((0, N)), [], settings=st)
    assert ks.N == N and (ks.perm() == np.arange(N)).all()
    rec["update"] = bool(ks.kktsolver_update(np.zeros(0)))
    rec["ir"], rec["ok"] = {{}}, {{}}
    for k in g.KS:
        print("@@k", k, file=sys.stderr, flush=True)
        Bk = p["BB"][k]
        drx = torch.from_numpy(np.ascontiguousarray(Bk.T)).to(dev)
        dlx = torch.full((k, N), -7.25, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ok, ir = ks.kktsolver_solve_multi_dev(k, drx.data_ptr(), 0, dlx.data_ptr(), 0)
        torch.cuda.synchronize()
        out[f"{{name}}/B{{k}}"] = dlx.cpu().numpy().T.copy()
        S = np.zeros((N, k))
        oks = [bool(ok)]
        for j in range(k):
            ks.kktsolver_setrhs(Bk[:, j], np.zeros(0))
            x = np.zeros(N)
            oks.append(bool(ks.kktsolver_solve(x, None)))
            S[:, j] = x
        out[f"{{name}}/S{{k}}"] = S
        rec["ir"][k], rec["ok"][k] = [int(v) for v in ir], oks
    rec["fallbacksB"] = list(ks.fallbacks)
    del ks
    print(json.dumps(rec), flush=True)
np.savez({npz!r}, **out)
"""

_RUNS = {}


def run_env(env_id, tmp_path_factory):
    """All cases in one child process under ENVS[env_id]; -> {name: dict(rec, X: arrays, plansA, plansB: {k: plans})}."""
    if env_id in _RUNS:
        return _RUNS[env_id]
    npz = str(tmp_path_factory.mktemp("sweep") / f"{env_id}.npz")
    e = dict(os.environ, HIPKKT_VERBOSE="2")
    e.update(ENVS[env_id])
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, names=list(CASES), npz=npz)], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "gave up" not in r.stderr, r.stderr[-4000:]
    recs = {d["name"]: d for d in (json.loads(line) for line in r.stdout.split("\n") if line.startswith("{"))}
    arrays = np.load(npz)
    res = {}
    for chunk in r.stderr.split("@@A ")[1:]:
        name = chunk.split("\n", 1)[0].strip()
        partA, partB = chunk.split("@@B ", 1)
        ks = partB.split("@@k ")
        res[name] = dict(rec=recs[name], plansA=_sweep_plans(partA),
                         plansB={int(s.split("\n", 1)[0]): _sweep_plans(s) for s in ks[1:]},
                         X={key.split("/", 1)[1]: arrays[key] for key in arrays.files if key.startswith(name + "/")})
    assert set(res) == set(CASES), sorted(set(CASES) - set(res))
    _RUNS[env_id] = res
    return res


# ------------------------------------------------------------------------------------------------ checks
def _check_bounds(env_id, name, run):
    """a. and b. for one (environment, case): every level-A solve through front_shapes' _check, every level-B column
    against the same bounds, its own single solve (bit for bit) and ir == 0.  -> the worst error / bound ratios."""
    ref, rec, X = reference(name), run["rec"], run["X"]
    worst = dict(fwdA=0.0, bwdA=0.0, fwdB=0.0, bwdB=0.0)
    for i in range(NSOLVES):
        cj, bound = ref["casesA"][("A", i)]
        fwd, bwd = fs.errors(cj, X["A"][:, i])
        d = dict(env=env_id, name=name, solve=i, refactor=rec["refactor"], fallbacks=rec["fallbacksA"], fwd=fwd, bwd=bwd, bound=bound)
        worst["fwdA"], worst["bwdA"] = max(worst["fwdA"], fwd / bound), max(worst["bwdA"], bwd / fs.BWD_BOUND)
        _check(d)
    assert rec["update"] is True and rec["fallbacksB"] == [0, 0], rec
    for k in KS:
        G, S = X[f"B{k}"], X[f"S{k}"]
        assert all(rec["ok"][str(k)]) and rec["ir"][str(k)] == [0] * k, (env_id, name, k, rec)
        for j in range(k):
            cj, bound = ref["casesB"][(k, j)]
            tag = (env_id, name, k, j)
            assert np.array_equal(G[:, j], S[:, j]), (tag, "differs from its own single solve", np.abs(G[:, j] - S[:, j]).max())
            if not np.any(cj.x_true):
                assert not np.any(G[:, j]), (tag, "zero column")
                continue
            fwd, bwd = fs.errors(cj, G[:, j])
            worst["fwdB"], worst["bwdB"] = max(worst["fwdB"], fwd / bound), max(worst["bwdB"], bwd / fs.BWD_BOUND)
            assert fwd <= bound, (tag, fwd, bound)
            assert bwd <= fs.BWD_BOUND, (tag, bwd)
    return worst


def _check_paths(env_id, name, run):
    """The path assertions of the environment, from the sweep-plan lines of the level-A solves (level B: see the module
    docstring) and, for the column counts, of the level-B ones."""
    plans = run["plansA"]
    steady = [p for p in plans if p["nr"] == 1 and not p["w_pending"]]
    assert steady, (env_id, name, plans)                   # solves 2..4: W is there
    tag = (env_id, name, plans)
    env = ENVS[env_id]
    nl = plans[0]["persistent"][1]
    for p in plans:
        assert p["nr"] == 1 and p["persistent"][1] == nl, tag
        assert p["packed"] == (env.get("HIPKKT_PACKED") != "0"), tag
    if "HIPKKT_NO_TOP" in env:
        for p in plans:
            assert _empty(p["chained"]) and _empty(p["persistent"]) and p["per_level"] == (0, nl) and p["kernel"] == "none", tag
            assert p["launches"], tag
        fam = [l for p in plans for l in p["launches"]]
        if env_id == "unmerged":
            assert all(l["family"] != "level" and not l["merged"] for l in fam), tag
            if name in ("mixed_129", "merge_129"):         # more small fronts than ride along: two launches in level 0
                assert {l["family"] for l in fam if l["level"] == 0} == {"block", "small"}, tag
        if env_id == "merge0" and name in ("mixed_few", "mixed_129", "merge_128", "tall_mixed"):
            l0 = [l for l in steady[0]["launches"] if l["level"] == 0]          # nothing rides along: one merged launch
            assert len(l0) == 1 and l0[0]["family"] == "level" and l0[0]["block"] > 0 and l0[0]["wave"] + l0[0]["tiny"] > 0, tag
        if env_id == "per_level" and name == "mixed_129":
            l0 = [l for l in steady[0]["launches"] if l["level"] == 0]
            assert len(l0) == 1 and (l0[0]["family"], l0[0]["block"], l0[0]["wave"], l0[0]["tiny"]) == ("level", 2, 96, 33), tag
        if env_id == "per_level" and name.startswith("tiny_n"):
            l0 = [l for l in steady[0]["launches"] if l["level"] == 0]
            assert len(l0) == 1 and (l0[0]["family"], l0[0]["tiny"]) == ("small", int(name[6:])), tag
        for l in fam:
            if l["family"] in ("block", "level"):
                assert l["solve_bs"] == (128 if env_id == "bs128" and l["fmax"] <= 128 else 256), (l, tag)
    if "HIPKKT_CHAIN_TOP" in env:
        for p in plans:
            assert _empty(p["persistent"]) and p["kernel"] == "none", tag
            if nl >= 2:
                assert p["chained"][1] == nl and p["chained"][1] - p["chained"][0] >= 2, tag
    if env_id in ("default", "top_cap3", "top_512") and name in TALL:
        for p in plans:                                    # "chain_below": two chained launches under the persistent set
            assert p["chained"] == (0, 2) and p["persistent"] == (2, 5) and p["kernel"] == "top", tag
            assert p["grid"] == (3 if env_id == "top_cap3" else 6), tag        # six fronts in the set
            assert p["threads"] == (512 if env_id == "top_512" else 1024), tag
    # the column counts: k = 2 sweeps two columns at once, k = 3 (the first of 3, 4, 5, 8) four
    pb = run["plansB"]
    assert any(p["nr"] == 2 for p in pb[2]), (env_id, name, pb[2])
    assert any(p["nr"] in (2, 4) for p in pb[3]), (env_id, name, pb[3])
    assert all(p["nr"] == 1 for p in pb[1]) and pb[1], (env_id, name, pb[1])


@pytest.mark.parametrize("env_id", list(ENVS))
def test_every_sweep_path_meets_the_bounds(env_id, tmp_path_factory):
    runs = run_env(env_id, tmp_path_factory)
    worst = {}
    for name in CASES:
        w = _check_bounds(env_id, name, runs[name])
        p = runs[name]["plansA"][-1]
        print(f"\n[sweep {env_id}] {name:16s} N {runs[name]['rec']['N']:5d} per-level {p['per_level']} chained {p['chained']} "
              f"persistent {p['persistent']} {p['kernel']}/{p['grid']} A: fwd/bound {w['fwdA']:.3f} bwd/bound {w['bwdA']:.3f} "
              f"B: fwd/bound {w['fwdB']:.3f} bwd/bound {w['bwdB']:.3f}")
        for key, v in w.items():
            worst[key] = max(worst.get(key, 0.0), v)
    print(f"\n[sweep {env_id}] worst ratios {worst}")
    for name in CASES:
        _check_paths(env_id, name, runs[name])


def test_both_sweep_states_are_seen(tmp_path_factory):
    """The first solve after refactor() finds W still pending where the factorisation forms it behind the tree: a
    narrow top (three or more block-class launches at the end) with block-class fronts below it, whose W is forked to the
    side stream (enqueue_factor) -- tall_mixed.  The plan line shows that variant and the steady state; every other case
    shows the steady state for all four solves."""
    runs = run_env("default", tmp_path_factory)
    for name in CASES:
        plans = runs[name]["plansA"]
        assert any(not p["w_pending"] for p in plans), (name, plans)
    plans = runs["tall_mixed"]["plansA"]
    assert any(p["w_pending"] for p in plans), plans


@pytest.mark.parametrize("other", ["chain_root", "default", "legacy_per_level", "legacy_chain_root"])
def test_chained_sweeps_and_record_layouts_are_bit_identical(other, tmp_path_factory):
    """a chained sweep does the per-level sweep's arithmetic in the same order, and so do both record
    layouts.  `default` is compared on the tall trees' CHAINED levels only in as far as the whole solution shows them:
    see the note in DESIGN 5 on the persistent kernel above them."""
    base = run_env("per_level", tmp_path_factory)
    runs = run_env(other, tmp_path_factory)
    names = TALL if other == "default" else list(CASES)
    bad = []
    for name in names:
        for key, ref in base[name]["X"].items():
            got = runs[name]["X"][key]
            for j in range(ref.shape[1]):
                if not np.array_equal(ref[:, j], got[:, j]):
                    bad.append((name, key, j, float(np.abs(ref[:, j] - got[:, j]).max() / np.abs(ref[:, j]).max())))
    assert not bad, (other, len(bad), bad[:12])
