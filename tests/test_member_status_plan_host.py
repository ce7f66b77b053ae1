"""The host-only column -> member table of hipkkt_kkt_system_set_member_status (csrc/batch_plan.cpp, plan_column_members:
colmem[k] = rowmem[perm[k]] with its checks of the permutation and the row table) under AddressSanitizer +
UndefinedBehaviorSanitizer, against brute force: tests/sanitize/member_status_driver.cpp, a stand-alone program built
from the same source.  It runs random partitions and permutations, the edges and every refusal named in its head
comment."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuclarabel_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("member_status") / "member_status_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "sanitize", "member_status_driver.cpp"),
                           os.path.join(CSRC, "batch_plan.cpp"), "-o", exe])
    return exe


def test_column_table_matches_brute_force_and_every_refusal_is_given(driver):
    p = subprocess.run([driver], capture_output=True, text=True, env=ENV, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "MEMBER STATUS DRIVER OK" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]


def test_the_plan_file_stays_host_only():
    src = open(os.path.join(CSRC, "batch_plan.cpp")).read() + open(os.path.join(CSRC, "batch_plan.hpp")).read()
    assert "hip/" not in src and "hip_runtime" not in src
