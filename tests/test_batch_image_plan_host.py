"""The host-only tables of hipkkt_kkt_system_set_member_refinement (csrc/batch_plan.cpp, plan_batch_image: row of K's
image -> member for all n + m + p rows, the rows listed by member, workgroup -> (member, chunk of its image rows) with
the slot layout the kernels use, the long rows by member) under AddressSanitizer + UndefinedBehaviorSanitizer, against
brute force: tests/sanitize/batch_image_driver.cpp, a stand-alone program built from the same source.  It runs random
partitions and the edges named in its head comment."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuclarabel_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_image") / "batch_image_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "sanitize", "batch_image_driver.cpp"),
                           os.path.join(CSRC, "batch_plan.cpp"), "-o", exe])
    return exe


def test_image_tables_match_brute_force_on_random_partitions_and_edges(driver):
    p = subprocess.run([driver], capture_output=True, text=True, env=ENV, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "BATCH IMAGE DRIVER OK" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
