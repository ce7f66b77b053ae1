"""Host side of the front-shape cases (tests/front_shapes.py): the symbolic phase gives every case the fronts its table
says, and the references the GPU tests measure against are sound -- exact right-hand sides, tolerances that scipy's
fp64 solve meets, and tolerances tight enough that a factor wrong by one perturbed extend-add term fails them."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import front_shapes as fs
from tests import test_gpu_front_shapes as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fs.all_cases()
SWEEP = fs.sweep_table()         # the forests of tests/test_gpu_sweep_paths.py

_DUMP_SCRIPT = r"""
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
from cuclarabel_amd import _lib
from tests import front_shapes as fs
T = dict(fs.all_cases(), **fs.sweep_table())
for name in {names!r}:
    spec = T[name][0]
    c = fs.make_case(spec, 1)
    print("@@case", name, file=sys.stderr, flush=True)
    perm, info = _lib.symbolic_analyse(c.K, ordering=_lib.ORDER_NATURAL)
    print(json.dumps(dict(name=name, identity=bool((perm == np.arange(len(perm))).all()), max_front=info["max_front"],
                          nsuper=info["nsuper"], nlevels=info["nlevels"])), flush=True)
"""

_LEVEL = re.compile(r"\[levels\]\s+(\d+):\s+(\d+) fronts \(\s*(\d+) f<=8,\s+(\d+) f<=64\) fmax\s+(\d+) ncmax\s+(\d+)")


def _dump(names):
    env = dict(os.environ, HIPKKT_DUMP_LEVELS="1")
    r = subprocess.run([sys.executable, "-c", _DUMP_SCRIPT.format(root=ROOT, names=list(names))], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    infos = {d["name"]: d for d in map(json.loads, r.stdout.split("\n")[:-1])}
    levels = {}
    for chunk in r.stderr.split("@@case ")[1:]:
        name, rest = chunk.split("\n", 1)
        levels[name.strip()] = [(int(m[2]), int(m[5]), int(m[6]), int(m[3]), int(m[4])) for m in _LEVEL.finditer(rest)]
    return infos, levels   # per level: (fronts, fmax, ncmax, f<=8 count, f<=64 count)


@pytest.fixture(scope="module")
def dumps():
    """[levels] lines and info of every case, from ONE child process (HIPKKT_DUMP_LEVELS is read once per process)."""
    return _dump(CASES)


@pytest.fixture(scope="module")
def sweep_dumps():
    return _dump(SWEEP)


@pytest.mark.parametrize("name", list(CASES))
def test_symbolic_gives_the_designed_fronts(dumps, name):
    infos, levels = dumps
    spec, level0, _ = CASES[name]
    info, lv = infos[name], levels[name]
    assert info["identity"], "ORDER_NATURAL must eliminate these matrices in index order"
    assert lv[0] == level0, (lv[0], level0)
    copies = level0[0] if spec[0][1] == 0 else sum(1 for s in spec if s[2] == -1)
    assert info["nlevels"] == len(lv)
    if spec[0][1] == 0 and all(s[2] == -1 for s in spec):
        # forests of roots: one level, the fronts themselves
        assert len(lv) == 1 and info["nsuper"] == len(spec)
        assert info["max_front"] == max(s[0] for s in spec)
    else:
        # the designed front, then the stick's root (and chain links) above it: one front per tree per level
        assert all(l[0] == copies for l in lv[1:]), lv
        assert info["nsuper"] == copies * len(lv)
        f0 = spec[0][0] + spec[0][1]
        if spec[1][:2] == (20, 1):
            top = 20 + 1 + spec[2][1]                # beside_sibling: P = (1, R) with S absorbed, rows = G
        else:
            top = spec[2][0] + spec[1][0]            # the stick merged into its root
        assert info["max_front"] == max(f0, top), (info["max_front"], f0, top)
    # the designed front lands in the kernel class the table names (a chain's first link is a block-class front)
    want = CASES[name][2]
    if want in ("tiny", "wave", "block", "chain"):
        assert fs.klass(level0[1], level0[2]) == ("block" if want == "chain" else want), (name, level0)


@pytest.mark.parametrize("name", list(SWEEP))
def test_symbolic_gives_the_forests_their_levels(sweep_dumps, name):
    """Every level of a forest holds the fronts its constructors reason out: count, tallest, widest, tiny and f <= 64."""
    infos, levels = sweep_dumps
    spec, want, _ = SWEEP[name]
    assert infos[name]["identity"], "ORDER_NATURAL must eliminate these matrices in index order"
    assert tuple(levels[name]) == want, (levels[name], want)
    assert infos[name]["nlevels"] == len(want)
    assert infos[name]["nsuper"] == sum(l[0] for l in want)
    assert infos[name]["max_front"] == max(l[1] for l in want)


def test_the_forests_hold_the_counts_and_classes_they_are_for():
    """Packing edges of the sweep kernels: tiny fronts go eight to a wave, one-wave fronts four to a 256-thread
    workgroup; a level with block-class fronts keeps up to merge_small (128) small ones in its launch."""
    lv0 = {n: SWEEP[n][1][0] for n in SWEEP}
    assert sorted(lv0[f"tiny_n{n}"][3] for n in (1, 7, 8, 9, 31, 32, 33)) == [1, 7, 8, 9, 31, 32, 33]
    for n in (1, 7, 8, 9, 31, 32, 33):
        fronts = {(nc + nb) for nc, nb, _ in SWEEP[f"tiny_n{n}"][0][:1]} | {nc for nc, nb, p in SWEEP[f"tiny_n{n}"][0] if p < 0 and nc <= 8}
        assert lv0[f"tiny_n{n}"][0] == n and (n < 9 or fronts == {1, 2, 8}), (n, fronts)
    for stem, f, nc in (("wave9", 9, 9), ("wave39", 39, 39), ("wave_16_28", 44, 16), ("wave_1_38", 39, 1)):
        for n in (3, 4, 5):
            assert lv0[f"{stem}_n{n}"] == (n, f, nc, 0, n) and fs.klass(f, nc) == "wave"
    # all three classes in one level, on either side of merge_small
    cnt, fmax, ncmax, n8, n64 = lv0["mixed_few"]
    assert n8 == 9 and n64 - n8 == 5 and cnt - n64 == 1 and n64 <= 128 and fs.klass(fmax, ncmax) == "block"
    cnt, fmax, ncmax, n8, n64 = lv0["mixed_129"]
    assert n8 == 33 and cnt == 33 + 96 + 2 and (fmax, ncmax) == (40, 40) and fs.klass(40, 40) == "block" and cnt - 2 == 129
    # taller trees: two levels of one-wave fronts alone (launches of their own), three block-class levels above them
    for n in ("tall_wave", "tall_mixed"):
        lv = SWEEP[n][1]
        assert len(lv) == 5 and lv[1][:3] == (2, 24, 20) and all(l[:3] == (2, 44 if l is not lv[4] else 40, 40) for l in lv[2:]), lv
    assert fs.klass(24, 20) == "wave" and fs.klass(44, 40) == "block"
    assert SWEEP["tall_wave"][1][0] == (2, 24, 20, 0, 2)
    assert SWEEP["tall_mixed"][1][0] == (7, 40, 40, 3, 7)         # 3 tiny, 2 one-wave (24, 20), 2 block-class (40, 40)
    assert not fs.UNREACHABLE.keys() & set(SWEEP)


# ------------------------------------------------------------------------------------------------ the factor-build cases
BUILD = fs.build_table()             # the new shapes
BUILD_CASES = fs.build_cases()       # ... and the shape-table cases that get a tall variant: name -> (spec, tall spec, group)
BUILD_SPECS = fs.build_specs()       # every spec of tests/test_gpu_factor_builds.py
NEW_NAMES = list(BUILD) + [n + "+tall" for n in BUILD_CASES] + ["xcd_forest", "xcd_forest+tall", "xcd_parents"]

_BUILD_DUMP = r"""
import sys
sys.path.insert(0, {root!r})
from cuclarabel_amd import _lib
from tests import test_gpu_factor_builds as fb
for name in {names!r}:
    print("@@case", name, file=sys.stderr, flush=True)
    _lib.symbolic_analyse(fb.case_of(name).K, ordering=_lib.ORDER_NATURAL)
"""


@pytest.fixture(scope="module")
def build_dumps():
    """[levels] lines of every factor-build case: name -> per level (fronts, fmax, ncmax, f<=8 count, f<=64 count)."""
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("HIPKKT_")}, HIPKKT_DUMP_LEVELS="1")
    r = subprocess.run([sys.executable, "-c", _BUILD_DUMP.format(root=ROOT, names=NEW_NAMES)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for chunk in r.stderr.split("@@case ")[1:]:
        name, rest = chunk.split("\n", 1)
        out[name.strip()] = [(int(m[2]), int(m[5]), int(m[6]), int(m[3]), int(m[4])) for m in _LEVEL.finditer(rest)]
    assert set(out) == set(NEW_NAMES)
    return out


def test_the_build_table_holds_the_edges_it_is_for():
    shapes = {n: v[0][0][:2] for n, v in BUILD.items()}
    assert {s[1] for n, s in shapes.items() if n.startswith("quad")} == {31, 32, 33, 95, 96, 97}          # 32-row quadrants
    assert all(s[0] == 40 for n, s in shapes.items() if n.startswith("quad"))
    chunk = sorted(s for n, s in shapes.items() if n.startswith("chunk"))
    assert chunk == sorted([(nc, nb) for nc in (15, 16, 17, 33, 48, 49) for nb in (65, 129)] + [(96, 129)])
    # ... every one of them has an off-diagonal tile whose tile row is short: nr = 1 of 64, nq = 64
    assert all(nb > 64 and nb % 64 == 1 for _, nb in chunk)
    assert sorted(s for n, s in shapes.items() if n.startswith("shallow")) == [(3, 39), (4, 39), (5, 39)]
    assert all(fs.klass(nc + nb, nc) == "block" for nc, nb in shapes.values())
    assert not any(n.split("_")[0] in ("quad", "chunk", "shallow") for n in fs.UNREACHABLE)
    assert set(fs.BUILD_FROM_SHAPES) <= set(CASES) and all(CASES[n][2] == "block" for n in fs.BUILD_FROM_SHAPES)


@pytest.mark.parametrize("name", list(BUILD))
def test_symbolic_gives_the_new_designed_fronts(build_dumps, name):
    spec, level0, want = BUILD[name]
    lv = build_dumps[name]
    assert lv[0] == level0 == (1, spec[0][0] + spec[0][1], spec[0][0], 0, int(spec[0][0] + spec[0][1] <= 64)), (lv[0], level0)
    assert all(l[0] == 1 for l in lv), lv
    assert fs.klass(level0[1], level0[2]) == want == "block"


@pytest.mark.parametrize("name", list(BUILD_CASES))
def test_tall_variants_have_the_levels_the_construction_predicts(build_dumps, name):
    """The designed front as in the plain case, above it the fronts tall_fronts() reasons out -- one per level, every one
    block-class (a one-wave launch would end the overlap mode's tail), at least three of them."""
    spec = BUILD_CASES[name][0]
    lv = build_dumps[name + "+tall"]
    assert lv[0][:3] == (1, spec[0][0] + spec[0][1], spec[0][0]), lv[0]
    want = fs.tall_fronts(spec)
    assert [l[:3] for l in lv[1:]] == [(1, f, nc) for f, nc in want], (lv, want)
    assert len(want) >= 3 and all(fs.klass(f, nc) == "block" for f, nc in want), want


def test_the_xcd_forests_hold_the_launches_they_are_for(build_dumps):
    from tests import extend_add_shapes as ea
    tiles = sorted((nb + 63) // 64 * ((nb + 63) // 64 + 1) // 2 for nb in fs.XCD_NB)
    assert tiles == [1, 1, 1, 1, 3, 3, 3, 6, 6, 10, 10]              # eleven fronts: a group of eight, a group of three
    for name in ("xcd_forest", "xcd_forest+tall"):
        lv = build_dumps[name]
        # all in one level, the two (40, 0) roots with them (f <= 64: those two and the two (40, 1) fronts)
        assert lv[0] == (13, 233, 40, 0, 4), lv[0]
        assert all(fs.klass(l[1], l[2]) == "block" for l in lv), lv
    spec = fs.xcd_forest()
    roots = [i for i, s in enumerate(spec) if s[:2] == (40, 0)]
    assert len(roots) == 2 and 0 < roots[0] < roots[1] < len(spec) - 3      # between the designed fronts
    assert len(build_dumps["xcd_forest+tall"]) >= 4
    # parents with stored children: ten of them in level 1, their children in level 0, two links of each root above
    lv = build_dumps["xcd_parents"]
    assert len(lv) == 4 and lv[1][0] == len(ea.XCD_PARENTS) == 10 and lv[2][0] == lv[3][0] == 10, lv
    assert all(fs.klass(l[1], l[2]) == "block" for l in lv), lv
    T = ea.cases()
    with_pieces = [n for n in ea.XCD_PARENTS if T[n]["level1"][2] > 0]
    assert len(with_pieces) >= 9 and len({T[n]["shape"]["sp_"] for n in ea.XCD_PARENTS}) >= 3


def _case(name, seed=1):
    if name in NEW_NAMES:
        from tests import test_gpu_factor_builds as fb
        return fb.case_of(name)
    return fs.make_case((CASES.get(name) or SWEEP[name])[0], seed)


@pytest.mark.parametrize("name", NEW_NAMES)
def test_a_fault_in_the_product_is_far_over_the_bound(name):
    """The seeded fault aimed at the product: the last column's term l_ik d_k l_jk left out of the last entry of the designed
    front's update block misses the forward bound by 100 x or more."""
    c = _case(name)
    tol = fs.forward_bound(c, fs.errors(c, fs.reference_solve(c))[0])
    fe, be = fs.errors(c, fs.reference_solve(c, K=fs.product_fault(c)))
    print(f"\n[product fault] {name:22s} forward {fe:.2e} (bound {tol:.2e}, x{fe / tol:.0f}) backward {be:.2e}")
    assert fe >= 100 * tol, (fe, tol)
    assert be >= 100 * fs.BWD_BOUND, be


@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("solve_bs")] + ["solve_bs_1024"] + list(SWEEP) + NEW_NAMES)
def test_references_are_exact_calibrated_and_discriminating(name):
    c = _case(name)
    # b = K~ x_true was rounded once from long double
    r = fs.symmetric_matvec_ld(c.Kt, c.x_true)
    assert np.abs(r - np.asarray(c.b, np.longdouble)).max() <= fs.U * np.abs(r).max()
    # the a-priori condition bound holds where it can be measured
    if c.K.shape[0] <= 3000:
        assert np.linalg.cond(fs.full(c.Kt).toarray()) <= c.cond_bound * (1 + 1e-12)
    # scipy's fp64 solve meets the tolerances the GPU must meet
    x = fs.reference_solve(c)
    fwd, bwd = fs.errors(c, x)
    assert fwd <= 100 * c.cond_bound * fs.U and bwd <= fs.BWD_BOUND, (fwd, bwd, c.cond_bound)
    tol = fs.forward_bound(c, fwd)
    # discrimination: one extend-add term wrong by 1e-7 misses the forward bound by 100x or more
    xe = fs.reference_solve(c, K=fs.perturbed(c))
    fe, be = fs.errors(c, xe)
    assert fe >= 100 * tol, (fe, tol)
    assert be >= 100 * fs.BWD_BOUND, be


@pytest.mark.parametrize("name,variant", [(n, v) for n in g.PIVOT_CASES for v in range(g.pivot_variants(n))])
def test_pivot_cases_are_exact(name, variant):
    """The pivot-rule cases: with row k an explicit zero in every earlier column the pivot at k is exactly K_kk, so
    K~ (the regularised diagonal) is known exactly -- an LDL^T without pivoting that applies the rule to K in fp64
    reproduces x_true of K~, and the control (the rule not applied) is far from it."""
    c, pivots, eps, delta = g.pivot_case(name, variant)
    A = fs.full(c.K).toarray()
    n = A.shape[0]
    L, d = np.eye(n), np.zeros(n)
    W = A.copy()
    nreg = 0
    for k in range(n):
        dk = W[k, k]
        if dk * c.dsigns[k] < eps:
            dk = c.dsigns[k] * delta
            nreg += 1
        d[k] = dk
        L[k + 1:, k] = W[k + 1:, k] / dk
        W[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], W[k + 1:, k])
    assert nreg == sum(1 for _, v, s in pivots if v * s < eps)
    y = np.linalg.solve(L, c.b)
    x = np.linalg.solve(L.T, y / d)
    fwd, bwd = fs.errors(c, x)
    assert fwd <= 100 * c.cond_bound * fs.U and bwd <= fs.BWD_BOUND, (fwd, bwd)
    assert g.control_error(c) > 1e-3
