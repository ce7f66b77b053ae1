"""Every build of the panel and the tile kernel (k_panel, k_schur: csrc/factor_kernels.hip) at the shape edges, through level A
(hipkkt_ldl_*, no refinement, ORDER_NATURAL), against exact answers -- and each run must SAY which build it ran.

Which build a front meets is the schedule's decision, not the front's:
    plain      k_panel<BS, false, false>, k_schur<false, false>   outside the overlap mode (HIPKKT_FACTOR_OVERLAP=0 here)
    pipelined  k_schur<false, true>                               ... in launches of more than HIPKKT_SCHUR_PIPE_TILES tiles
                                                                  that are HIPKKT_SCHUR_PIPE_NC columns deep (both 0 here)
    overlap    k_panel<BS, false, true>, k_schur<true, true>      the schedule's tail of at least three block-class launches:
                                                                  the TALL variant of a case (front_shapes.tall)
(Row slices, k_panel<1024, true, *>, keep their tests in test_gpu_front_shapes.py.)  The cases are front_shapes.build_cases():
update blocks on the 32-row quadrant edges of a tile, chunk-edge depths (KC = 16) with off-diagonal tiles whose tile row
holds one row, depths of 3, 4 and 5 columns (an MFMA step is 4), and the panel / tile / block-size cases of the shape table.

Every run meets test_gpu_front_shapes._check's bounds
    forward error  <= max(100 cond u, 10 x scipy's error on the same case),   backward error <= 64 u in long double,
refactor() is True, no fall-back, no wait given up, and
  * the handle's own report names the mode: "factorisation overlap: last 0 launches" (plain, pipelined) or every launch from
    the designed front's on, with that launch in an "overlap admission" line (overlap); the per-launch lines of
    HIPKKT_VERBOSE=2 name the tile kernel's build of every launch with tiles;
  * a second refactor() on the same values and a second solve give the same bits (in overlap mode: the progress and done
    counters start clean);
  * plain and pipelined give bit-identical x (the pipelining moves loads, not arithmetic);
  * HIPKKT_TILE_XCD=2 and =0 give bit-identical x on two forests whose launches hold groups of eight fronts with unequal tile
    counts, a short last group, fronts without tiles and parents with stored children (pass-through lists), outside and
    inside the overlap mode; the "tile order" line must show the launch dealt in the first run and none in the second.
One child process per knob environment (the knobs are read once per process), one at a time, each under its timeout; the
worst error / bound per mode and group is printed under -s."""
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
CASES = fs.build_cases()
SPECS = fs.build_specs()
GROUPS = ("edges", "panel", "schur")
FORESTS = {"plain": ("xcd_forest", "xcd_parents"), "overlap": ("xcd_forest+tall", "xcd_parents")}

MODES = {
    "plain": {"HIPKKT_FACTOR_OVERLAP": "0"},
    "pipelined": {"HIPKKT_FACTOR_OVERLAP": "0", "HIPKKT_SCHUR_PIPE_TILES": "0", "HIPKKT_SCHUR_PIPE_NC": "0"},
    "overlap": {},
}
# the tile kernel's build on the per-launch line (csrc/kernels.hpp: schur_build_name)
BUILD_OF = {"plain": "plain", "pipelined": "pipelined", "overlap": "overlap"}

_CASE_CACHE = {}


def case_of(name):
    """The fs.Case of a name of front_shapes.build_specs(), or of "xcd_parents" (extend_add_shapes): built once, left unchanged."""
    if name not in _CASE_CACHE:
        _CASE_CACHE[name] = ea.case(name) if name == "xcd_parents" else fs.make_case(SPECS[name], 1)
    return _CASE_CACHE[name]


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
from cuclarabel_amd import _lib
from cuclarabel_amd.kktsolver import HipDirectLDLSolver
from tests import front_shapes as fs
from tests import test_gpu_factor_builds as fb
for name in {names!r}:
    print("@@case", name, file=sys.stderr, flush=True)
    c = fb.case_of(name)
    h = HipDirectLDLSolver(c.K, c.dsigns, _lib.default_settings(ordering=_lib.ORDER_NATURAL))
    out = dict(name=name, N=c.K.shape[0], refactor=h.refactor())
    x = np.zeros(c.K.shape[0])
    h.solve(None, x, c.b)
    # the same values once more: the factorisation's counters and buffers carry nothing over
    out["refactor_again"] = h.refactor()
    y = np.zeros(c.K.shape[0])
    h.solve(None, y, c.b)
    out["same_bits"] = bool(np.array_equal(x, y))
    out["fallbacks"] = list(h.fallbacks)
    del h
    out["fwd"], out["bwd"] = fs.errors(c, x)
    out["scipy_fwd"] = fs.errors(c, fs.reference_solve(c))[0]
    out["bound"] = fs.forward_bound(c, out["scipy_fwd"])
    out["x"] = [v.hex() for v in x.tolist()]
    print(json.dumps(out), flush=True)
"""

_SUMMARY = re.compile(r"supernodes in (\d+) levels \((\d+) launches\)")
_OVERLAP = re.compile(r"factorisation overlap: last (\d+) launches")
_LAUNCH = re.compile(r"\[hipkkt\] launch (\d+) level (\d+): (\d+) fronts \((one wave|block)\).*? (\d+) tiles \(\d+ columns deep on average\).*tile kernel: (\w+)")
_ADMIT = re.compile(r"overlap admission: launch (\d+):")
_ORDER = re.compile(r"\[hipkkt\] tile order: (\d+) launches dealt to XCD residue classes \((\d+) tiles\):(.*)")
_RUNS = {}


def run(names, env, timeout=240):
    """One child process for `names` under `env`: -> {name: (result, report)}; report: what the handle said on stderr."""
    key = (tuple(names), tuple(sorted(env.items())))
    if key not in _RUNS:
        from tests.test_gpu_parity import _schedule_line
        # (no knob of the caller's but the library under test itself)
        e = {k: v for k, v in os.environ.items() if not k.startswith("HIPKKT_") or k == "HIPKKT_LIB"}
        e.update(env, HIPKKT_VERBOSE="2")
        r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, names=list(names))], env=e, cwd=ROOT,
                           capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        res = [json.loads(line) for line in r.stdout.split("\n") if line.startswith("{")]
        errs = [chunk.split("\n", 1)[1] for chunk in r.stderr.split("@@case ")[1:]]
        assert len(res) == len(errs) == len(names), r.stderr[-3000:]
        out = {}
        for d, err in zip(res, errs):
            assert "gave up" not in err, err
            assert "no stream for the Schur tiles" not in err, err
            m, o = _SUMMARY.search(err), _ORDER.search(err)
            rep = dict(levels=int(m[1]), launches=int(m[2]), overlap=[int(v) for v in _OVERLAP.findall(err)],
                       admitted=sorted(int(v) for v in _ADMIT.findall(err)),
                       lines=[dict(q=int(v[0]), level=int(v[1]), fronts=int(v[2]), klass=v[3], tiles=int(v[4]), build=v[5])
                              for v in _LAUNCH.findall(err)],
                       dealt=(int(o[1]), int(o[2]), [int(v) for v in o[3].split() if v != "none"]), sch=_schedule_line(err))
            d["x"] = np.array([float.fromhex(v) for v in d["x"]])
            out[d["name"]] = (d, rep)
        _RUNS[key] = out
    return _RUNS[key]


def _names(group, mode):
    return [n + ("+tall" if mode == "overlap" else "") for n, v in CASES.items() if v[2] == group]


def _check_run(d):
    _check(d)
    assert d["refactor_again"] is True and d["same_bits"], (d["name"], "a second refactor() on the same values changed the solution")


def _check_mode(name, rep, mode):
    """The handle's report: the run took the builds its mode names."""
    assert len(rep["overlap"]) == 1 and len(rep["lines"]) == rep["launches"], (name, rep)
    with_tiles = [l for l in rep["lines"] if l["tiles"] > 0]
    assert with_tiles and with_tiles[0]["level"] == 0, (name, rep["lines"])              # the designed front has an update block
    assert all(l["build"] == BUILD_OF[mode] for l in with_tiles), (name, mode, rep["lines"])
    assert all(l["build"] == "none" for l in rep["lines"] if l["tiles"] == 0), (name, rep["lines"])
    if mode == "overlap":
        # every launch from the designed front's (the first) on: k_panel<BS, false, true> / k_schur<true, true>
        assert rep["launches"] >= 3 and all(l["klass"] == "block" for l in rep["lines"]), (name, rep["lines"])
        assert rep["overlap"][0] == rep["launches"] and rep["admitted"] == list(range(rep["launches"])), (name, rep)
    else:
        assert rep["overlap"][0] == 0 and rep["admitted"] == [], (name, rep)


_WORST = defaultdict(lambda: [0.0, 0.0, ""])


def _record(tag, d):
    w = _WORST[tag]
    if d["fwd"] / d["bound"] > w[0]:
        w[0], w[2] = d["fwd"] / d["bound"], d["name"]
    w[1] = max(w[1], d["bwd"] / fs.BWD_BOUND)


def _print_record(tag):
    w = _WORST[tag]
    print(f"\n[factor builds record] {tag:34s} worst forward / bound {w[0]:.3f} ({w[2]}), worst backward / bound {w[1]:.3f}")


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("mode", list(MODES))
def test_every_case_meets_the_bounds_in_the_build_it_names(mode, group):
    rows = run(_names(group, mode), MODES[mode])
    tag = f"{mode} {group}"
    for name, (d, rep) in rows.items():
        print(f"\n[factor builds {mode}] {name:22s} N {d['N']:5d} launches {rep['launches']} overlap {rep['overlap'][0]} tile kernels "
              f"{','.join(l['build'] for l in rep['lines'])} sliced {rep['sch']['sliced_fronts']} fwd {d['fwd']:.2e} (bound {d['bound']:.2e}) "
              f"bwd {d['bwd']:.2e}")
    for name, (d, rep) in rows.items():
        _check_run(d)
        _check_mode(name, rep, mode)
        _record(tag, d)
    _print_record(tag)


@pytest.mark.parametrize("group", GROUPS)
def test_the_pipelined_tile_kernel_changes_no_bit(group):
    """k_schur<false, true> loads chunk k + 1 while chunk k's products run: the same operands in the same order."""
    plain, pipe = run(_names(group, "plain"), MODES["plain"]), run(_names(group, "pipelined"), MODES["pipelined"])
    for name in plain:
        x, y = plain[name][0]["x"], pipe[name][0]["x"]
        assert np.array_equal(x, y), (name, float(np.abs(x - y).max()))


@pytest.mark.parametrize("mode", ["plain", "overlap"])
def test_the_xcd_tile_order_changes_no_bit(mode):
    """HIPKKT_TILE_XCD permutes a launch's tiles with their pass-through ranges (tile_cut, ptile_cut): which workgroup takes a
    tile changes, what the tile computes does not.  A tile paired with another tile's lists would miss the bounds and the
    bits."""
    names = FORESTS[mode]
    on, off = run(names, dict(MODES[mode], HIPKKT_TILE_XCD="2")), run(names, dict(MODES[mode], HIPKKT_TILE_XCD="0"))
    for name in names:
        for tag, rows in (("xcd 2", on), ("xcd 0", off)):
            d, rep = rows[name]
            print(f"\n[factor builds {mode} {tag}] {name:18s} N {d['N']:5d} launches {rep['launches']} overlap {rep['overlap'][0]} dealt "
                  f"{rep['dealt'][0]} launches ({rep['dealt'][1]} tiles) fwd {d['fwd']:.2e} (bound {d['bound']:.2e}) bwd {d['bwd']:.2e}")
            _check_run(d)
            _record(f"{mode} forests {tag}", d)
            assert all(l["build"] == BUILD_OF[mode] for l in rep["lines"] if l["tiles"] > 0), (name, rep["lines"])
            if mode == "overlap":
                assert rep["overlap"][0] == rep["launches"] >= 3 and rep["admitted"] == list(range(rep["launches"])), (name, rep)
            else:
                assert rep["overlap"][0] == 0, (name, rep)
        # the launch the forest is for: the level of the thirteen fronts / of the ten parents
        lines = on[name][1]["lines"]
        (wide,) = [l["q"] for l in lines if l["level"] == (1 if name == "xcd_parents" else 0)]
        assert lines[wide]["fronts"] >= 10 and lines[wide]["tiles"] > lines[wide]["fronts"], lines[wide]
        n_on, t_on, dealt_on = on[name][1]["dealt"]
        assert wide in dealt_on and n_on == len(dealt_on) and t_on >= lines[wide]["tiles"], (name, on[name][1]["dealt"])
        assert off[name][1]["dealt"] == (0, 0, []), (name, off[name][1]["dealt"])
        x, y = on[name][0]["x"], off[name][0]["x"]
        assert np.array_equal(x, y), (name, float(np.abs(x - y).max()))
    for tag in ("xcd 2", "xcd 0"):
        _print_record(f"{mode} forests {tag}")
