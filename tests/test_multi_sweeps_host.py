"""Host side of tests/test_gpu_multi_sweeps.py: what that module asserts on the GPU is prepared and cross-checked here.

  * The dispatch table of the many-column sweeps (csrc/launch_shapes.hpp: multi_shape) under the knobs, through
    tests/sanitize/host_driver.cpp --multi-shape (the product's header and knobs.hpp, read from the environment as in the
    product), against EXPECT -- typed in from the `if` chains of launch_fwd_multi, launch_bwd_multi and
    launch_pull_leaves_multi as they stood before multi_shape replaced them.
  * The new trees (front_shapes.multi_forests, pulled_leaf_shapes.solve_cases): host_driver --launches prints every
    supernode and launch of the real schedule; the designed fronts are there with their shapes and classes, the leaves the
    solves pull are the ones the construction names, and the three numbers of the engine's "contribution rows pulled" line
    follow from the construction.  Every childless front sits in a level-0 launch (the driver's check_schedule).  The
    driver also reports what the PRODUCT's tables hold (csrc/engine_tables.cpp: the pulled flags and the three numbers);
    they equal the restatement here, by default and under HIPKKT_PULL_LEAVES=0.
  * The references of the new cases are exact, calibrated and discriminating, as in test_front_shapes_host.py.
  * A numpy restatement of the many-column sweeps with three simulated faults: each one fails the bounds or the
    duplicate-column equality, the fault-free restatement does not."""
import os
import subprocess

import numpy as np
import pytest

from tests import front_shapes as fs
from tests import pulled_leaf_shapes as pls
from tests.test_host_sanitizers import CSRC, ROOT, SOURCES

KPS = (16, 32, 48, 64, 80, 128, 144, 256, 272)
ENVS = {
    "default": {},
    "pull_off": {"HIPKKT_PULL_LEAVES": "0"},
    "vec2": {"HIPKKT_MULTI_VEC": "2"},
    "vec1": {"HIPKKT_MULTI_VEC": "1"},
    "ct1": {"HIPKKT_MULTI_CT": "1"},
}
# KP -> (wave_v, leaf_v, block_bs, block_ct).  wave: V = 2 where 128 | KP.  leaf: V = 4 where 64 | KP and the knob allows
# four, else V = 2 where 32 | KP, else 1 -- HIPKKT_MULTI_VEC=1 therefore takes V = 2 wherever 32 | KP, like =2 (the chain
# has no branch for the knob below 4).  block: 256 / 2 where 32 | KP and KP >= 256 unless HIPKKT_MULTI_CT=1, else 256 / 1
# from 128 columns on, else 512 / 1.
_DEFAULT = {16: (1, 1, 512, 1), 32: (1, 2, 512, 1), 48: (1, 1, 512, 1), 64: (1, 4, 512, 1), 80: (1, 1, 512, 1),
            128: (2, 4, 256, 1), 144: (1, 1, 256, 1), 256: (2, 4, 256, 2), 272: (1, 1, 256, 1)}
_VEC2 = {**_DEFAULT, 64: (1, 2, 512, 1), 128: (2, 2, 256, 1), 256: (2, 2, 256, 2)}
EXPECT = {"default": _DEFAULT, "pull_off": _DEFAULT, "vec2": _VEC2, "vec1": _VEC2, "ct1": {**_DEFAULT, 256: (2, 4, 256, 1)}}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("multi")
    exe = str(d / "host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "include")] + SOURCES + ["-o", exe])
    return exe, d


def _clean_env(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HIPKKT_")}
    env.update(extra)
    return env


@pytest.mark.parametrize("env_id", list(ENVS))
def test_dispatch_table(driver, env_id):
    exe, _ = driver
    r = subprocess.run([exe, "--multi-shape"] + [str(k) for k in KPS], env=_clean_env(ENVS[env_id]), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {}
    for line in r.stdout.splitlines():
        w = line.split()
        assert w[0::2] == ["KP", "wave_v", "leaf_v", "block_bs", "block_ct"], line
        got[int(w[1])] = tuple(int(x) for x in w[3::2])
    assert got == EXPECT[env_id]


def test_every_instance_is_in_the_table():
    """wave V = 1, 2; leaf V = 1, 2, 4; block 512 / 1, 256 / 1, 256 / 2 -- each at some (environment, KP) of the GPU module."""
    seen = {(e, kp): v for e in EXPECT for kp, v in EXPECT[e].items()}
    assert {v[0] for v in seen.values()} == {1, 2}
    assert {v[1] for v in seen.values()} == {1, 2, 4}
    assert {v[2:] for v in seen.values()} == {(512, 1), (256, 1), (256, 2)}
    assert any(kp >= 256 and kp % 32 and v[2:] == (256, 1) for (e, kp), v in seen.items())           # KP >= 256, 32 does not divide it
    assert any(kp >= 256 and e == "ct1" and v[2:] == (256, 1) and kp % 32 == 0 for (e, kp), v in seen.items())


# ------------------------------------------------------------------------------------------------ the new trees
def new_cases():
    """name -> (Case maker, expectation dict) of every case this pull request adds."""
    T = {}
    for name, (spec, level0, kl) in fs.multi_forests().items():
        T[name] = (lambda spec=spec: fs.make_case(spec, 1), dict(level0=level0, klass=kl))
    for name, (cols, rows, exp) in pls.solve_cases().items():
        T[name] = (lambda cols=cols, rows=rows: pls.make_case(cols, rows, 1), dict(leaf=exp))
    return T


NEW = new_cases()


def _launches(exe, d, names, extra_env=None):
    files = []
    for name in names:
        path = str(d / (name + ".bin"))
        if not os.path.exists(path):
            pls.write_pattern(NEW[name][0]().K, path)
        files.append(path)
    r = subprocess.run([exe, "--launches"] + files, env=_clean_env(extra_env or {}), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for name, chunk in zip(names, r.stdout.split("@@case ")[1:]):
        L, S, product = {}, {}, dict(pulled=[], numbers=None)
        for line in chunk.split("\n")[1:]:
            w = line.split()
            if w and w[0] == "L":
                L[int(w[1])] = dict(level=int(w[2]), small=w[3] == "1", count=int(w[4]))
            elif w and w[0] == "S":
                v = list(map(int, w[1:]))
                S[v[0]] = dict(c0=v[1], nc=v[2], nb=v[3], parent=v[4], nchild=v[5], launch=v[6], rel=v[7:])
            elif w and w[0] == "P" and w[2] == "1":        # the product's own flag (EngineTables::solve_pulled)
                product["pulled"].append(int(w[1]))
            elif w and w[0] == "M":                        # ... and the numbers of its "contribution rows pulled" line
                product["numbers"] = tuple(int(x) for x in w[1:])
        out[name] = (L, S, product)
    return out


@pytest.fixture(scope="module")
def launches(driver):
    exe, d = driver
    return _launches(exe, d, list(NEW))


def solve_pulled(L, S, pull_on=True):
    """The fronts the many-column sweeps pull, by the rule of build_engine_tables (csrc/engine_tables.cpp) restated here,
    and the three numbers of the engine's verbose line."""
    got = sorted(s for s, d in S.items() if pull_on and L[d["launch"]]["small"] and d["nchild"] == 0 and d["nc"] == 1
                 and d["parent"] >= 0 and 1 <= d["nb"] <= 47)
    a = sum(S[s]["nb"] for s in got)
    b = sum(d["nb"] for d in S.values())
    c = len({(S[s]["parent"], r) for s in got for r in S[s]["rel"]})
    return got, (a, b, c)


_PRODUCT_RUNS = {}


@pytest.mark.parametrize("env_id", ["default", "pull_off"])
@pytest.mark.parametrize("name", list(NEW))
def test_the_product_pulls_what_the_rule_says(driver, launches, name, env_id):
    """What the product's tables hold -- the pulled set and the three numbers -- equals the restatement solve_pulled, for
    every new case, by default and with the pulling switched off."""
    if env_id not in _PRODUCT_RUNS:
        _PRODUCT_RUNS[env_id] = launches if env_id == "default" else _launches(*driver, list(NEW), ENVS[env_id])
    L, S, product = _PRODUCT_RUNS[env_id][name]
    got, abc = solve_pulled(L, S, pull_on=env_id == "default")
    assert product["pulled"] == got, (product["pulled"], got)
    assert product["numbers"] == abc, (product["numbers"], abc)
    if env_id == "pull_off":
        assert got == [] and abc[0] == 0 and abc[2] == 0 and abc[1] == launches[name][2]["numbers"][1]


@pytest.mark.parametrize("name", list(NEW))
def test_the_schedule_holds_the_designed_fronts(launches, name):
    L, S, _ = launches[name]
    exp = NEW[name][1]
    for d in S.values():           # (check_schedule requires it too, for every pattern the driver sees)
        assert d["nchild"] > 0 or L[d["launch"]]["level"] == 0, "a childless front outside level 0"
    level0 = sorted((d["nc"], d["nb"]) for d in S.values() if L[d["launch"]]["level"] == 0)
    if "level0" in exp:
        assert level0 == exp["level0"], (level0, exp["level0"])
        for nc, nb in level0:
            assert fs.klass(nc + nb, nc) == exp["klass"], (nc, nb)
            cls_small = all(L[d["launch"]]["small"] for d in S.values() if (d["nc"], d["nb"]) == (nc, nb) and L[d["launch"]]["level"] == 0)
            assert cls_small == (exp["klass"] == "wave"), (nc, nb)
        return
    e = exp["leaf"]
    sh = e["shape"]
    cols, rows, _ = pls.solve_cases()[name]
    nleaves = sum(1 for c in cols[:-3] if len(c) == 1)
    # every leaf and regular child is a front of its own with the rows it was given, under P' = (rp + k, sp)
    by_c0 = {d["c0"]: d for d in S.values()}
    pprime = by_c0[cols[-3][0]]                                  # S's first column: P' starts there
    assert (pprime["nc"], pprime["nb"]) == (sh["rp"] + sh["k"], sh["sp_"]), pprime
    for cs, rs in zip(cols[:-3], rows[:-3]):
        d = by_c0[cs[0]]
        assert (d["nc"], d["nb"], d["nchild"]) == (len(cs), len(rs), 0), (cs, d)
        assert S[d["parent"]] is pprime
        assert d["rel"] == [r - cols[-3][0] for r in rs], (d["rel"], rs)       # positions in P' = pattern rows less P''s first column
    got, abc = solve_pulled(L, S)
    assert sorted(S[s]["c0"] for s in got) == e["pulled"], (got, e["pulled"])
    assert abc == (e["a"], e["b"], e["c"]), (abc, e)
    assert fs.klass(pprime["nc"] + pprime["nb"], pprime["nc"]) == ("wave" if "16_28" in name or name.startswith("gather") else "block")
    if name.startswith("ride"):
        # the short leaves are one-wave fronts, but ride in the block-class leaves' launch
        short = [by_c0[cs[0]] for cs, rs in zip(cols[:nleaves], rows[:nleaves]) if len(rs) <= 38]
        assert short and all(fs.klass(1 + d["nb"], 1) in ("wave", "tiny") and not L[d["launch"]]["small"] for d in short)
        assert all(fs.klass(1 + nb, 1) == "block" for nb in (39, 47, 48)) and fs.klass(39, 1) == "wave"


def test_the_slice_rule_takes_every_branch():
    """k_bwd_block_m's ns = min(NW / nt, ceil(f / 32)): over the designed fronts ns = 1, ns = NW / nt with idle waves, and
    the cap by f all occur, for both workgroup sizes; f sits on both sides of 32 ns."""
    seen = set()
    for name, fronts in fs.SLICE_FRONTS.items():
        for nc, nb in fronts:
            f = nc + nb
            for nw in (8, 4):
                nt, ns = fs.bwd_multi_slices(nc, f, nw)
                by_f = (f + 31) // 32
                kind = "one" if ns == 1 else "waves" if ns == nw // nt and by_f >= ns else "f"
                idle = nw - nt * ns if nt * ns < nw else 0
                print(f"[slices] {name:14s} ({nc:2d}, {nb:3d}) f {f:3d} NW {nw}: nt {nt} ns {ns} ({kind}, {idle} idle waves)")
                seen.add((nt, nw, kind, idle > 0 and ns == nw // nt))
    assert {nt for nt, *_ in seen} == {1, 2, 3, 5, 6}
    for nw in (8, 4):
        assert {k for _, w, k, _ in seen if w == nw} == {"one", "waves", "f"}, (nw, seen)
        assert any(i for _, w, k, i in seen if w == nw), "ns = NW / nt with idle waves"
    # both sides of 32 ns
    for nc, lo, nw in ((16, 64, 8), (16, 128, 8), (32, 64, 8), (16, 64, 4)):
        a, b = fs.bwd_multi_slices(nc, lo, nw)[1], fs.bwd_multi_slices(nc, lo + 1, nw)[1]
        assert 32 * a == lo and b == min(a + 1, nw // ((nc + 15) // 16)), (nc, lo, nw, a, b)


@pytest.mark.parametrize("name", list(NEW))
def test_new_references_are_exact_calibrated_and_discriminating(name):
    c = NEW[name][0]()
    r = fs.symmetric_matvec_ld(c.Kt, c.x_true)
    assert np.abs(r - np.asarray(c.b, np.longdouble)).max() <= fs.U * np.abs(r).max()
    assert np.linalg.cond(fs.full(c.Kt).toarray()) <= c.cond_bound * (1 + 1e-12)
    x = fs.reference_solve(c)
    fwd, bwd = fs.errors(c, x)
    assert fwd <= 100 * c.cond_bound * fs.U and bwd <= fs.BWD_BOUND, (fwd, bwd, c.cond_bound)
    tol = fs.forward_bound(c, fwd)
    xe = fs.reference_solve(c, K=fs.perturbed(c))
    fe, be = fs.errors(c, xe)
    assert fe >= 100 * tol, (fe, tol)
    assert be >= 100 * fs.BWD_BOUND, be


# ------------------------------------------------------------------------------------------------ the refinement cases
@pytest.mark.parametrize("name", ["wc_roots", "counts_40_65", "panel_nc33"])
def test_refinement_tolerances_meet_their_conditions(name):
    """residual_reference.MULTI_REFINE: with the chosen abstol the first residual needs refinement by 1e4 and every accept /
    stop decision of every column is clear of its threshold by 4 x (asserted inside refine_predictions); k = 9 has every
    column accept in round 1 and only some in round 2, k = 33 mixes columns of 0, 1 and 2 rounds and a zero column."""
    from tests import residual_reference as rr
    from tests import test_gpu_multi_sweeps as g
    assert set(rr.MULTI_REFINE) == {"wc_roots", "counts_40_65", "panel_nc33"}
    K, abstol, runs = g.refine_predictions(name)
    assert rr.shape_facts(K)["nlong"] == 0
    (k9, B9, p9), (k33, B33, p33) = runs
    assert (k9, k33) == (9, 33)
    r9, r33 = [p["rounds"] for p in p9], [p["rounds"] for p in p33]
    assert min(r9) >= 1 and min(r9) < max(r9) and all(p["norms"][1] < p["norms"][0] / 5 for p in p9), r9
    assert set(r33) == {0, 1, 2} and any(not np.any(B33[:, j]) for j in range(33)), r33
    assert all(p["stop"] == "tol" for p in p9 + p33)
    print(name, abstol, r9, r33)


# ------------------------------------------------------------------------------------------------ the bounds bite
def _ldl(A):
    """L, d of A = L diag(d) L' without pivoting (the matrices are strictly diagonally dominant)."""
    n = A.shape[0]
    L, d, W = np.eye(n), np.zeros(n), A.copy()
    for k in range(n):
        d[k] = W[k, k]
        L[k + 1:, k] = W[k + 1:, k] / d[k]
        W[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], W[k + 1:, k])
    return L, d


def _sweeps(L, d, B, drop=None):
    """The two sweeps for a block of columns, column by column of L as the tree does it: forward, every column c sends
    -L(r, c) y_c to the rows r below it; backward x_c = y_c / d_c - sum_r L(r, c) x_r.  drop = (c, r): that one forward term
    is left out in every column of B -- a pulled term -L(r, 0) b_c missing from its parent row's sum."""
    n = L.shape[0]
    Y = B.copy()
    for c in range(n):
        u = np.outer(L[c + 1:, c], Y[c])
        if drop is not None and drop[0] == c:
            u[drop[1] - c - 1] = 0.0
        Y[c + 1:] -= u
    X = Y / d[:, None]
    for c in range(n - 1, -1, -1):
        X[c] -= L[c + 1:, c] @ X[c + 1:]
    return X


def test_the_bounds_and_the_duplicate_column_notice_simulated_faults():
    """A numpy restatement of the many-column sweeps on slots_40_65 (pulled leaves [0, 1] and [1, 2] and a regular child
    under a block-class parent), k = 17 columns built as the GPU module builds them.  Fault-free it meets what the GPU
    must meet; with one pulled term dropped, with the last active column's values written into its neighbour on the
    parent's rows, or with a refinement round's `add` taken from row o + 1, a forward or backward ratio exceeds 1 or the
    duplicate column stops being a bit copy."""
    import scipy.sparse.linalg as spla
    name, k = "slots_40_65", 17
    cols, rows, exp = pls.solve_cases()[name]
    c = pls.make_case(cols, rows, 1)
    N = c.K.shape[0]
    X = np.random.default_rng(3).standard_normal((N, k))
    X[:, 0] = 0.0
    X[:, -1] *= 1e6
    X[:, k - 2] = X[:, 1]
    B = fs.symmetric_matmat_ld(c.K, X).astype(np.float64)
    sfwd = fs.errors_columns(c, spla.splu(fs.full(c.Kt).tocsc()).solve(B), X, B)[0]
    bound = np.maximum(100.0 * c.cond_bound * fs.U, 10.0 * sfwd)
    L, d = _ldl(fs.full(c.K).toarray())

    def verdict(G):
        fwd, bwd = fs.errors_columns(c, G, X, B)
        return dict(fwd=float((fwd[1:] / bound[1:]).max()), bwd=float((bwd[1:] / fs.BWD_BOUND).max()), zero=not np.any(G[:, 0]),
                    dup=bool(np.array_equal(G[:, k - 2], G[:, 1])))

    good = _sweeps(L, d, B)
    v = verdict(good)
    print("fault-free", v)
    assert v["fwd"] <= 1.0 and v["bwd"] <= 1.0 and v["zero"] and v["dup"], v
    # 1. one pulled term dropped: leaf 0 (column cols[0][0]) towards its second row
    leaf, row = cols[0][0], rows[0][1]
    assert row > leaf and L[row, leaf] != 0.0
    v = verdict(_sweeps(L, d, B, drop=(leaf, row)))
    print("dropped pulled term", v)
    assert v["fwd"] > 1.0 or v["bwd"] > 1.0, v
    # 2. a tail mix-up: on the parent's rows the last active column's values land in its neighbour
    bad = good.copy()
    prow = cols[-3] + cols[-2]
    bad[prow, k - 2] = good[prow, k - 1]
    v = verdict(bad)
    print("tail mix-up", v)
    assert not v["dup"] and (v["fwd"] > 1.0 or v["bwd"] > 1.0), v
    # 3. a refinement round, out = dx + add with add = x: one row o of the parent takes add from row o + 1
    dx = _sweeps(L, d, (np.asarray(B, np.longdouble) - fs.symmetric_matmat_ld(c.K, good)).astype(np.float64))
    v = verdict(good + dx)
    print("refined", v)
    assert v["fwd"] <= 1.0 and v["bwd"] <= 1.0 and v["zero"] and v["dup"], v
    o = cols[-2][0]
    out = good + dx
    out[o] = dx[o] + good[o + 1]
    v = verdict(out)
    print("add from row o + 1", v)
    assert v["fwd"] > 1.0 or v["bwd"] > 1.0, v
