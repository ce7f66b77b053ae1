"""The factorisation's extend-add at chosen row geometries, through level A (hipkkt_ldl_*, no refinement, ORDER_NATURAL),
against exact answers.

tests/extend_add_shapes.py builds trees whose stored children (two or more columns) sit on chosen rows of their parent's
front, at the edges of the work lists that k_panel, k_schur and k_front_wave walk: pieces of 63 .. 129 rows that start at a
panel column > 0 and cross the panel / update and the 64-row tile boundaries; 15 .. 129 items in one wave slice of a panel
and in one wave's share of a tile (16 in flight, 64 descriptors a round); 33 children on the same entries; chains of three
and five panels that share two update buffers, with children whose columns belong to the second and to the last link; a
row-sliced parent; one-wave parents with children of 10 and 11 rows and with 64 and 65 children; a tiny parent with children.
x_true is known and b = K~ x_true is exact.  Every solve meets front_shapes' bounds (tests/test_gpu_front_shapes.py: _check)
    forward error  <= max(100 cond u, 10 x scipy's error on the same case),   backward error <= 64 u in long double,
the handle must report the pieces, dense children, shared chains, sliced fronts and pulled leaves the construction
predicts (a case that silently takes another path fails), and
  * HIPKKT_UPD_PINGPONG=1 and =0 give bit-identical solutions on every chain case (only addresses differ);
  * HIPKKT_DENSE_CHILD=1 and =0 agree within twice the forward bound, bit for bit on the chains without other children;
  * two fresh handles give identical bits on the many-children case, in overlap mode too;
  * after hipkkt_ldl_update_values with new values on the same pattern, hipkkt_ldl_refactor + solve meet the same bounds (the
    second pass over shared buffers that hold the first factorisation's last blocks).
HIPKKT_FACTOR_OVERLAP 1 / 0 is crossed with HIPKKT_PULL_FACTOR_LEAVES 1 / 0 for every case, and the chain group's
HIPKKT_UPD_PINGPONG=0 and HIPKKT_DENSE_CHILD=0 runs with both again.  One child process per knob environment (the knobs are read once per process), one at a time, each under its own timeout; the
summary is parsed from stderr.  Worst error / bound per group is printed under -s."""
import json
import os
import re
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pytest

from tests import extend_add_shapes as ea
from tests import front_shapes as fs
from tests.test_gpu_front_shapes import _check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ea.cases()
TWICE = ("many_33",)

_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
from cuclarabel_amd import _lib
from cuclarabel_amd.kktsolver import HipDirectLDLSolver
from tests import extend_add_shapes as ea
from tests import front_shapes as fs
for name in {names!r}:
    print("@@case", name, file=sys.stderr, flush=True)
    c, c2 = ea.case(name), ea.second(name)
    st = _lib.default_settings(ordering=_lib.ORDER_NATURAL)
    xs, out = [], dict()
    for rep in range(2 if name in {twice!r} else 1):
        h = HipDirectLDLSolver(c.K, c.dsigns, st)
        out = dict(out, name=name, N=c.K.shape[0], refactor=h.refactor())
        x = np.zeros(c.K.shape[0])
        h.solve(None, x, c.b)
        xs.append(x)
        if rep == 0:
            # new values of the same pattern: update, refactor, solve -- the second pass over the handle's buffers
            assert np.array_equal(c.K.indices, c2.K.indices) and np.array_equal(c.K.indptr, c2.K.indptr)
            h.update_values(np.arange(c2.K.nnz), c2.K.data)
            out["refactor2"] = h.refactor()
            x2 = np.zeros(c.K.shape[0])
            h.solve(None, x2, c2.b)
        out["fallbacks"] = list(h.fallbacks)
        del h
    out["fwd"], out["bwd"] = fs.errors(c, xs[0])
    out["scipy_fwd"] = fs.errors(c, fs.reference_solve(c))[0]
    out["bound"] = fs.forward_bound(c, out["scipy_fwd"])
    out["fwd2"], out["bwd2"] = fs.errors(c2, x2)
    out["bound2"] = fs.forward_bound(c2, fs.errors(c2, fs.reference_solve(c2))[0])
    out["identical"] = all(np.array_equal(xs[0], y) for y in xs)
    out["handles"] = len(xs)
    out["x"] = [v.hex() for v in xs[0].tolist()]
    print(json.dumps(out), flush=True)
"""

_OVERLAP = re.compile(r"factorisation overlap: last (\d+) launches \(\d+ row slices in them\); pulled leaves: (\d+) \((\d+) terms\)")
_DENSE = re.compile(r"\[hipkkt\] dense children: (\d+)")
_SHARED = re.compile(r"\[hipkkt\] update blocks: (\d+) chains of panels \((\d+) links\) share two buffers each; (\d+) bytes kept, (\d+) without sharing")
_RUNS = {}


def run(names, env):
    """One child process for `names` under `env`: -> {name: (result, report)}; report: what the handle said on stderr."""
    key = (tuple(names), tuple(sorted(env.items())))
    if key not in _RUNS:
        from tests.test_gpu_parity import _schedule_line
        e = {k: v for k, v in os.environ.items() if not k.startswith("HIPKKT_")}
        e.update(env, HIPKKT_VERBOSE="2")
        r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, names=list(names), twice=TWICE)], env=e, cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        res = [json.loads(line) for line in r.stdout.split("\n") if line.startswith("{")]
        errs = [chunk.split("\n", 1)[1] for chunk in r.stderr.split("@@case ")[1:]]
        assert len(res) == len(errs) == len(names), r.stderr[-3000:]
        out = {}
        for d, err in zip(res, errs):
            assert "gave up" not in err, err
            levels, pulled = ea.parse_pieces(err)
            sh = _SHARED.search(err)
            rep = dict(levels=levels, pulled=pulled, dense=int(_DENSE.search(err)[1]), shared=tuple(map(int, sh.groups())),
                       overlap=[tuple(map(int, m.groups())) for m in _OVERLAP.finditer(err)], sch=_schedule_line(err))
            d["x"] = np.array([float.fromhex(v) for v in d["x"]])
            out[d["name"]] = (d, rep)
        _RUNS[key] = out
    return _RUNS[key]


def _env(overlap="1", pull="1", **extra):
    return dict({"HIPKKT_FACTOR_OVERLAP": overlap, "HIPKKT_PULL_FACTOR_LEAVES": pull}, **extra)


def _run_group(group, env):
    """The cases of a group (None: all of them) under `env`, plus a case's own environment (the row-sliced parent's
    HIPKKT_PANEL_CAP): one child process per distinct environment, cached."""
    out = {}
    by_env = defaultdict(list)
    for n in ea.names(group):
        by_env[tuple(sorted((CASES[n]["env"] if n in CASES else {}).items()))].append(n)
    for extra, names in by_env.items():
        out.update(run(names, dict(env, **dict(extra))))
    return out


def _check_both(d):
    """front_shapes' bounds for the first factorisation and for the refactorisation with new values."""
    _check(d)
    assert d["refactor2"] is True, d["name"]
    assert d["fwd2"] <= d["bound2"] and d["bwd2"] <= fs.BWD_BOUND, (d["name"], d["fwd2"], d["bound2"], d["bwd2"])


def _check_paths(name, rep, env):
    """The handle took the paths the construction predicts."""
    pull, dense_on, share_on = env["HIPKKT_PULL_FACTOR_LEAVES"] == "1", env.get("HIPKKT_DENSE_CHILD", "1") == "1", env.get("HIPKKT_UPD_PINGPONG", "1") == "1"
    if name == "tiny_parent":
        assert rep["levels"] == {} and rep["pulled"] == (0, 0) and rep["dense"] == 0 and rep["sch"]["block_fronts"] == 0, rep
        return
    d = CASES[name]
    want_pulled = d["pulled"] if pull else (0, 0)
    assert rep["pulled"] == want_pulled and all(o[1:] == want_pulled for o in rep["overlap"]), (name, rep["pulled"], rep["overlap"])
    assert rep["dense"] == (d["dense"] if dense_on else 0), (name, rep["dense"])
    assert rep["shared"][:1] == ((d["shared"],) if share_on else (0,)), (name, rep["shared"])
    if d["links"] and share_on:
        # links 0, 2, 4 .. write one buffer, links 1, 3 .. the other: the blocks of the links from the third on are saved (a
        # root's last link has no block: a three-link root shares in name only, the chain under a stick saves its third block)
        f, nbs = sum(d["links"]) + d["shape"]["sp_"], []
        for w in d["links"]:
            f -= w
            nbs.append(f)
        assert rep["shared"][1] == len(d["links"]) and rep["shared"][3] - rep["shared"][2] == 8 * sum(n * n for n in nbs[2:]), (name, rep["shared"], nbs)
    if not share_on:
        assert rep["shared"][2] == rep["shared"][3], (name, rep["shared"])
    if d["env"]:
        assert rep["sch"]["sliced_fronts"] >= d["sliced"] >= 1 and rep["sch"]["row_slices"] > rep["sch"]["sliced_fronts"], (name, rep["sch"])
    else:
        assert rep["sch"]["sliced_fronts"] == d["sliced"], (name, rep["sch"])
    # overlap mode takes the schedule's tail of at least three block-class launches: the designed parent's launch, the links
    # above it and the root's are in it (k_panel<.., true>, k_schur<true, true>) -- or, with the knob off, nothing is.  (A
    # one-wave parent is k_front_wave's either way.)
    assert rep["overlap"], name
    if env["HIPKKT_FACTOR_OVERLAP"] == "0":
        assert all(o[0] == 0 for o in rep["overlap"]), (name, rep["overlap"])
    elif d["block"]:
        above = len(d["links"] or (1,)) + (len(d["glinks"]) if d["glinks"] is not None else ea._g_links(d["shape"]["ng"]))
        assert above >= 3 and all(o[0] >= above for o in rep["overlap"]), (name, rep["overlap"], above)
    lv = rep["levels"]
    if d["block"] and any(d["level1"][:4]):
        got = lv[1]
        if want_pulled == (0, 0):
            assert got["listed"] == d["level1"] and got["out"] == (0, 0, 0), (name, got, d["level1"])
        else:
            assert got["listed"][0] + got["out"][1] == d["level1"][0] and got["listed"][2] + got["out"][0] == d["level1"][2], (name, got)
            assert got["listed"][1] + got["listed"][3] + got["out"][2] == d["level1"][1] + d["level1"][3], (name, got)
            assert got["out"][2] == want_pulled[1], (name, got)
    elif dense_on or not d["links"]:
        assert 1 not in lv, (name, lv)
    if d["links"] and not dense_on:
        # without dense children every link above the first lists the link below: its whole front, an identity map (the first
        # link is level 1 above its children, level 0 in a chain without any)
        f, base = sum(d["links"]) + d["shape"]["sp_"], int(bool(d["children"] or d["leaves"]))
        for i in range(1, len(d["links"])):
            f -= d["links"][i - 1]
            assert lv[base + i]["listed"] == ea.level_pieces(d["links"][i], [list(range(f))]), (name, i, lv[base + i])


_WORST = defaultdict(lambda: [0.0, 0.0])


def _record(tag, group, d):
    w = _WORST[tag, group]
    w[0] = max(w[0], d["fwd"] / d["bound"], d["fwd2"] / d["bound2"])
    w[1] = max(w[1], d["bwd"] / fs.BWD_BOUND, d["bwd2"] / fs.BWD_BOUND)


def _group(name):
    return CASES[name]["group"] if name in CASES else "wave"


@pytest.mark.parametrize("overlap", ["1", "0"])
@pytest.mark.parametrize("pull", ["1", "0"])
def test_every_case_meets_the_bounds_on_the_predicted_path(pull, overlap):
    env = _env(overlap, pull)
    for name, (d, rep) in _run_group(None, env).items():
        print(f"\n[extend-add pull {pull} overlap {overlap}] {name:14s} N {d['N']:4d} fwd {d['fwd']:.2e} (bound {d['bound']:.2e}) "
              f"bwd {d['bwd']:.2e} | refactored: fwd {d['fwd2']:.2e} (bound {d['bound2']:.2e}) bwd {d['bwd2']:.2e} | dense {rep['dense']} "
              f"shared {rep['shared'][0]} pulled {rep['pulled']}")
        _check_both(d)
        _check_paths(name, rep, dict(env, **(CASES[name]["env"] if name in CASES else {})))
        _record(f"pull {pull} ov {overlap}", _group(name), d)
    _print_record(f"pull {pull} ov {overlap}", ea.GROUPS)


@pytest.mark.parametrize("overlap", ["1", "0"])
def test_two_fresh_handles_give_identical_bits_on_the_many_children_case(overlap):
    for name in ea.names("many"):
        d, rep = _run_group(None, _env(overlap, "1"))[name]
        assert d["handles"] == 2 and d["identical"], name
        _check_both(d)


def _print_record(tag, groups):
    for group in groups:
        w = _WORST[tag, group]
        print(f"\n[extend-add record] {tag:22s} {group:12s} worst forward / bound {w[0]:.3f}, worst backward / bound {w[1]:.3f}")


@pytest.mark.parametrize("overlap", ["1", "0"])
@pytest.mark.parametrize("pull", ["1", "0"])
def test_shared_update_buffers_change_no_bit(pull, overlap):
    """HIPKKT_UPD_PINGPONG only moves the chain links' update blocks: the arithmetic and its order are the same.  A stale or
    overwritten buffer can show only where a block is really shared: the chain under a stick and the five-link chains (a
    three-link root's last link has no block) -- those must keep fewer bytes than they would without sharing."""
    on = _run_group(None, _env(overlap, pull))
    env = _env(overlap, pull, HIPKKT_UPD_PINGPONG="0")
    off = _run_group("chains", env)
    tag = f"pingpong 0 pull {pull} ov {overlap}"
    really_shared = 0
    for name in ea.names("chains"):
        _check_both(off[name][0])
        _check_paths(name, off[name][1], env)
        _record(tag, "chains", off[name][0])
        assert on[name][1]["shared"][0] == 1 and off[name][1]["shared"][0] == 0
        kept, without = on[name][1]["shared"][2:]
        if CASES[name]["shape"]["sp_"] or len(CASES[name]["links"]) >= 5:
            assert kept < without, (name, kept, without)
            really_shared += 1
        assert np.array_equal(on[name][0]["x"], off[name][0]["x"]), (name, np.abs(on[name][0]["x"] - off[name][0]["x"]).max())
    assert really_shared >= 4
    _print_record(tag, ("chains",))


@pytest.mark.parametrize("overlap", ["1", "0"])
@pytest.mark.parametrize("pull", ["1", "0"])
def test_dense_children_and_listed_links_agree(pull, overlap):
    """HIPKKT_DENSE_CHILD=0 sends every link's block through the item lists: within twice the forward bound (each is within
    the bound of x_true), and bit for bit where the chain has no other child -- every parent entry receives one term."""
    on = _run_group(None, _env(overlap, pull))
    env = _env(overlap, pull, HIPKKT_DENSE_CHILD="0")
    off = _run_group("chains", env)
    tag = f"dense 0 pull {pull} ov {overlap}"
    for name in ea.names("chains"):
        _check_both(off[name][0])
        _check_paths(name, off[name][1], env)
        _record(tag, "chains", off[name][0])
        c = ea.case(name)
        rel = np.abs(on[name][0]["x"] - off[name][0]["x"]).max() / np.abs(c.x_true).max()
        print(f"\n[extend-add dense child on / off, pull {pull} overlap {overlap}] {name:14s} differ by {rel:.2e} (bound {on[name][0]['bound']:.2e})")
        assert rel <= 2 * on[name][0]["bound"], (name, rel)
        if name.endswith("_bare"):
            assert rel == 0.0, (name, rel)
    _print_record(tag, ("chains",))


def test_pulled_and_stored_leaves_agree_within_the_bound():
    on, off = _run_group(None, _env("1", "1")), _run_group(None, _env("1", "0"))
    for name in ea.names("chains"):
        rel = np.abs(on[name][0]["x"] - off[name][0]["x"]).max() / np.abs(ea.case(name).x_true).max()
        assert rel <= 2 * on[name][0]["bound"], (name, rel)
