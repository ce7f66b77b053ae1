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


def _case(name, seed=1):
    return fs.make_case((CASES.get(name) or SWEEP[name])[0], seed)


@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("solve_bs")] + ["solve_bs_1024"] + list(SWEEP))
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
