"""The host-only partition plan of hipkkt_kkt_system_set_problems (csrc/batch_plan.cpp: the check of a partition, row ->
member, cone -> member, the assignment of workgroups to (member, chunk), the long rows by member) under AddressSanitizer +
UndefinedBehaviorSanitizer, against brute force: tests/sanitize/batch_plan_driver.cpp, a stand-alone program built from
the same source.  Run once on its own random partitions and refusals, and once on the stacks that
problems.block_diagonal makes of small_mixed members, which must all be accepted."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd import problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuclarabel_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_plan") / "batch_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "sanitize", "batch_plan_driver.cpp"),
                           os.path.join(CSRC, "batch_plan.cpp"), "-o", exe])
    return exe


def _clean(p):
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "BATCH PLAN DRIVER OK" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]


def test_tables_match_brute_force_and_every_refusal_names_its_cause(driver):
    _clean(subprocess.run([driver], capture_output=True, text=True, env=ENV, timeout=300))


def _write_stack(path, pb):
    """The stack as the library sees it: the partition of meta['blocks'], the cone list, and K's upper triangle (P with
    its diagonal in the first n columns, A' over the diagonal in the next m) as CSC."""
    n, m = pb.n, pb.m
    K = sp.bmat([[sp.triu(pb.P) + sp.identity(n), sp.csc_matrix(pb.A).T], [None, sp.identity(m)]], format="csc")
    K.sort_indices()
    x_off = np.concatenate([[0], np.cumsum([b[0] for b in pb.meta["blocks"]])])
    z_off = np.concatenate([[0], np.cumsum([b[1] for b in pb.meta["blocks"]])])
    lines = [f"{n} {m} {len(pb.meta['blocks'])}", " ".join(map(str, x_off)), " ".join(map(str, z_off)), str(len(pb.cones))]
    off = 0
    for c in pb.cones:
        lines.append(f"{c.kind} {off} {c.numel} {c.dim}")
        off += c.numel
    lines.append(" ".join(map(str, K.indptr)))
    lines.append(" ".join(map(str, K.indices)))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_every_block_diagonal_stack_of_small_mixed_members_is_accepted(driver, tmp_path):
    stacks = [
        [problems.small_mixed(seed=3)],
        [problems.small_mixed(seed=s) for s in (1, 2)],
        [problems.small_mixed(seed=s, n=5 + 3 * s, nn=s, zero=s % 2) for s in range(1, 8)],
        [problems.small_mixed(seed=s, n=3, nn=2, socs=(2, 3), psds=(1, 2), zero=0) for s in range(65)],
        [problems.small_mixed(seed=11, n=300, nn=260, socs=(3,), psds=(), zero=1), problems.small_mixed(seed=12, n=7, nn=1)],
    ]
    files = []
    for k, members in enumerate(stacks):
        files.append(str(tmp_path / f"stack{k}.txt"))
        _write_stack(files[-1], problems.block_diagonal(members))
    p = subprocess.run([driver] + files, capture_output=True, text=True, env=ENV, timeout=300)
    _clean(p)
    assert f"({len(files)} stacks)" in p.stdout
