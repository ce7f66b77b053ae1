"""The device tables of the engine and of the KKT handle under the knobs that change them, on the CPU.

csrc/engine_tables.cpp builds what LDLEngine::upload() copies to the device, csrc/kkt_assembly.cpp the CSR image and the
cone tables of a KKT handle; tests/sanitize/host_driver.cpp builds them for every schedule it sees and checks their
invariants (gather lists, packed K positions, tile order, pulled-leaf split, packed records, descriptors, child cuts, the
image and the cone tables).  tests/test_host_sanitizers.py runs it under the default knobs; here the same ASan / UBSan
build runs where a knob takes another branch:

  * HIPKKT_TILE_XCD=0 and HIPKKT_PULL_LEAVES=0 over the reduced configurations and the small zoo: the tile order is the
    identity with no launch dealt, and nothing is pulled (the driver requires both when the knobs say so).
  * HIPKKT_TILE_XCD=1 on front_shapes.xcd_forest: ONE level with eleven fronts of 1, 1, 3, 3, 6 and 10 tiles, a group of
    eight with unequal tile counts and a last group of three -- the launch is dealt, and the uploaded tiles are a
    permutation of the launch's tiles whose tcut / ptcut rows travelled with them."""
import os
import subprocess

import pytest

from tests import front_shapes as fs
from tests import pulled_leaf_shapes as pls
from tests.test_host_sanitizers import CASES, CSRC, ROOT, SOURCES, _write

_SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tables") / "host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", CSRC, "-I", os.path.join(ROOT, "include")] + SOURCES + ["-o", exe])
    return exe


def _run(driver, args, knobs):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HIPKKT_")}
    env.update(_SAN_ENV)
    env.update(knobs)
    p = subprocess.run([driver] + args, capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
    return p.stdout


def test_tables_with_the_tile_deal_and_the_pulling_switched_off(driver, tmp_path):
    files = []
    for name, maker, leaf in CASES:
        if name == "cfg2_n8000_longrange":                 # (the default-knob run covers it; the branches here need no size)
            continue
        path = str(tmp_path / (name + ".bin"))
        _write(path, maker(), leaf)
        files.append(path)
    out = _run(driver, files, {"HIPKKT_TILE_XCD": "0", "HIPKKT_PULL_LEAVES": "0"})
    assert "HOST SANITIZER DRIVER OK" in out
    assert out.count(" ordering ") >= 2 * len(files)


@pytest.mark.parametrize("tall", [False, True])
def test_the_xcd_deal_permutes_a_launch(driver, tmp_path, tall):
    path = str(tmp_path / "xcd_forest.bin")
    pls.write_pattern(fs.make_case(fs.xcd_forest(tall), 1).K, path)
    tiles = lambda nb: ((nb + 63) // 64) * ((nb + 63) // 64 + 1) // 2
    assert sum(tiles(nb) for nb in fs.XCD_NB) == 45        # 1, 10, 1, 6, 3, 3, 10, 1, 6, 3 and 1 tiles
    dealt = {}
    for xcd in ("1", "0"):
        out = _run(driver, ["--launches", path], {"HIPKKT_TILE_XCD": xcd})
        line = [l for l in out.splitlines() if l.startswith("D ")]
        assert len(line) == 1, out[-2000:]
        dealt[xcd] = tuple(int(x) for x in line[0].split()[1:])
    # what must be dealt with HIPKKT_TILE_XCD=1, from the schedule the driver printed: every block-class launch that has
    # tiles, with all of its tiles; the designed level is one of them
    small = {int(w[1]): w[3] == "1" for w in (l.split() for l in out.splitlines()) if w and w[0] == "L"}
    per_launch = {}
    for w in (l.split() for l in out.splitlines()):
        if w and w[0] == "S" and not small[int(w[7])]:
            per_launch.setdefault(int(w[7]), []).append(tiles(int(w[4])))
    assert sorted(t for t in per_launch[0] if t) == sorted(tiles(nb) for nb in fs.XCD_NB), per_launch[0]
    expect = (sum(1 for v in per_launch.values() if sum(v)), sum(sum(v) for v in per_launch.values()))
    # the driver's permutation check passed in both runs (exit 0)
    assert dealt["1"] == expect and expect[0] >= 1, (dealt, expect)
    assert dealt["0"] == (0, 0), dealt
