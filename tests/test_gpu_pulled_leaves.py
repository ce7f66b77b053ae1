"""The factorisation's pulled leaves (HIPKKT_PULL_FACTOR_LEAVES) at the smallest shapes where they can go wrong, through
level A (hipkkt_ldl_*, no refinement), against exact answers.

tests/pulled_leaf_shapes.py builds trees of one-column leaves with chosen rows under a parent of a chosen shape, with
front_shapes' value rule: x_true is known and b = K~ x_true is exact.  Every solve meets the a-priori bounds of
tests/test_gpu_front_shapes.py (its _check: forward error <= max(100 cond u, 10 x scipy's), backward error <= 64 u, no
fall-back).  Every case runs with the knob on and off, with the overlap mode on (the parent's panel and tiles are
k_panel<.., true> and k_schur<true, true>: a small tree's block-class launches are all in the overlap region) and off, and the
schedule summary must name exactly the intended leaves and terms as pulled -- or none.  One child process per
environment (the knobs are read once per process), every case in it.

Cases (pulled_leaf_shapes.cases): leaf heights 1, 7, 8, 35; leaves across the panel / update boundary and across the
64-row tile boundary (rows 63 and 64 of a parent with 120 update rows: tiles (0, 0), (1, 0), (1, 1)); a one-wave parent
(16, 28) that pulls nothing beside the block-class (16, 29); parents of f = 64 and 65 (both block-class: no front of 64
rows meets the one-wave rule f nc + nb^2 <= 1536); 70 and 130 leaves stacked on the same entries (a wave with more than
64 terms, waves and tiles with none); pulled leaves beside regular children and a dense child; a parent without leaves
(front_shapes' schur_nb65); a row-sliced parent (HIPKKT_PANEL_CAP), whose leaves stay stored; a leaf whose pivot is
regularised dynamically (the term must use the regularised d: the exact answer is that of K~, front_shapes.set_pivots);
two fresh handles give bit-identical solutions; knob on and off agree within the same bound."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import front_shapes as fs
from tests import pulled_leaf_shapes as pls
from tests.test_gpu_front_shapes import DELTA, EPS, _check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = pls.cases()
NAMES = list(SHAPES) + ["no_leaves", "regularised"]


def build(name):
    """-> (case, leaves, terms, eps, delta)"""
    if name == "no_leaves":
        return fs.make_case(fs.all_cases()["schur_nb65"][0], 1), 0, 0, None, None
    if name == "regularised":
        # two leaves of "heights" get pivots the rule replaces by sign * delta (a zero, and a value of the wrong sign)
        cols, rows, leaves, terms, _ = SHAPES["heights"]
        c = pls.make_case(cols, rows, 3)
        fs.set_pivots(c, [(cols[2][0], 0.0, 1), (cols[4][0], -0.5, 1), (cols[6][0], 0.25, 1)], EPS, DELTA)
        return c, leaves, terms, EPS, DELTA
    cols, rows, leaves, terms, _ = SHAPES[name]
    return pls.make_case(cols, rows, 1), leaves, terms, None, None


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
from cuclarabel_amd import _lib
from cuclarabel_amd.kktsolver import HipDirectLDLSolver
from tests import front_shapes as fs
from tests import test_gpu_pulled_leaves as g
for name in {names!r}:
    print("@@case", name, file=sys.stderr, flush=True)
    c, leaves, terms, eps, delta = g.build(name)
    kw = dict(dynamic_regularization_eps=eps, dynamic_regularization_delta=delta) if eps is not None else {{}}
    st = _lib.default_settings(ordering=_lib.ORDER_NATURAL, **kw)
    xs = []
    for rep in range(2 if {twice!r} else 1):
        h = HipDirectLDLSolver(c.K, c.dsigns, st)
        out = dict(name=name, N=c.K.shape[0], refactor=h.refactor())
        x = np.zeros(c.K.shape[0])
        h.solve(None, x, c.b)
        out["fallbacks"] = list(h.fallbacks)
        xs.append(x)
        del h
    out["fwd"], out["bwd"] = fs.errors(c, x)
    out["scipy_fwd"] = fs.errors(c, fs.reference_solve(c))[0]
    out["bound"] = fs.forward_bound(c, out["scipy_fwd"])
    out["identical"] = all(np.array_equal(xs[0], y) for y in xs)
    out["x"] = x.tolist()
    print(json.dumps(out), flush=True)
"""

_PULLED = re.compile(r"factorisation overlap: last (\d+) launches \(\d+ row slices in them\); pulled leaves: (\d+) \((\d+) terms\)")
_RUNS = {}


def run(knob, overlap, names=tuple(NAMES), extra=None, twice=False):
    """One child process under (knob, overlap): -> {name: (result, (overlap launches, leaves, terms) per handle)}"""
    key = (knob, overlap, names, tuple(sorted((extra or {}).items())), twice)
    if key not in _RUNS:
        from tests.test_gpu_parity import _schedule_line
        e = dict(os.environ, HIPKKT_VERBOSE="2", HIPKKT_PULL_FACTOR_LEAVES=knob, HIPKKT_FACTOR_OVERLAP=overlap)
        e.update(extra or {})
        r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, names=list(names), twice=twice)], env=e, cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        res = [json.loads(line) for line in r.stdout.split("\n") if line.startswith("{")]
        errs = [chunk.split("\n", 1)[1] for chunk in r.stderr.split("@@case ")[1:]]
        assert len(res) == len(errs) == len(names), r.stderr[-3000:]
        out = {}
        for d, err in zip(res, errs):
            assert "gave up" not in err, err
            handles = [tuple(map(int, m.groups())) for m in _PULLED.finditer(err)]
            assert handles, err
            sch = _schedule_line(err)
            # block-class launches (the launch lines of HIPKKT_VERBOSE=2), per handle
            sch["block_launches"] = len(re.findall(r"\[hipkkt\] launch \d+ level \d+: \d+ fronts \(block\)", err)) // len(handles)
            out[d["name"]] = (d, handles, sch)
        _RUNS[key] = out
    return _RUNS[key]


@pytest.mark.parametrize("overlap", ["1", "0"])
@pytest.mark.parametrize("knob", ["1", "0"])
def test_every_case_solves_exactly_and_pulls_what_it_should(knob, overlap):
    for name, (d, handles, sch) in run(knob, overlap).items():
        _, leaves, terms, _, _ = build(name)
        print(f"\n[pulled knob {knob} overlap {overlap}] {name:14s} N {d['N']:5d} leaves {handles[0][1]:4d} terms {handles[0][2]:5d} "
              f"fwd {d['fwd']:.2e} (bound {d['bound']:.2e}) bwd {d['bwd']:.2e}")
        _check(d)
        want = (leaves, terms) if knob == "1" else (0, 0)
        assert all(h[1:] == want for h in handles), (name, handles, want)
        assert sch["sliced_fronts"] == 0, (name, sch)
        if overlap == "1" and leaves > 0:                  # the parent's launch (the first block-class one) is in the overlap region
            assert handles[0][0] >= sch["block_launches"] >= 1, (name, handles, sch)
        if overlap == "0":
            assert handles[0][0] == 0, (name, handles)


@pytest.mark.parametrize("overlap", ["1", "0"])
def test_knob_on_and_off_agree_within_the_bound(overlap):
    on, off = run("1", overlap), run("0", overlap)
    for name in NAMES:
        c = build(name)[0]
        x1, x0 = np.array(on[name][0]["x"]), np.array(off[name][0]["x"])
        rel = np.abs(x1 - x0).max() / np.abs(c.x_true).max()
        assert rel <= 2 * on[name][0]["bound"], (name, rel)          # each is within the bound of x_true


def test_two_fresh_handles_give_identical_bits():
    for name, (d, handles, _) in run("1", "1", names=("heights", "stack_130", "tile_edge", "mixed"), twice=True).items():
        assert len(handles) == 2 and d["identical"], name
        _check(d)


@pytest.mark.parametrize("knob", ["1", "0"])
def test_a_row_sliced_parent_keeps_its_leaves_stored(knob):
    # HIPKKT_PANEL_CAP 3000: the parent P' = (48, 60), a trapezoid of 4056 doubles, is cut into row slices
    for name, (d, handles, sch) in run(knob, "1", names=("heights", "stack_70"), extra={"HIPKKT_PANEL_CAP": "3000"}).items():
        _check(d)
        assert sch["sliced_fronts"] > 0 and sch["row_slices"] > sch["sliced_fronts"], sch
        assert handles[0][1:] == (0, 0), handles
