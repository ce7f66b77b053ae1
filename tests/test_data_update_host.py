"""The host-only part of the data updates of level C (csrc/data_update.cpp: the position check of an (index, value)
update and the row / column tables of P's and A's stored entries) under AddressSanitizer + UndefinedBehaviorSanitizer,
against brute force: tests/sanitize/data_update_driver.cpp, a stand-alone program built from the same source."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuclarabel_amd", "csrc")


def test_index_check_and_entry_tables_match_brute_force_and_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "data_update_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "sanitize", "data_update_driver.cpp"),
                           os.path.join(CSRC, "data_update.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "DATA UPDATE DRIVER OK" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]


def test_data_update_translation_unit_has_no_hip_header():
    """it is host-only so that this file can test it: neither source includes a HIP header"""
    for f in ("data_update.cpp", "data_update.hpp"):
        text = open(os.path.join(CSRC, f)).read()
        assert "#include <hip" not in text and '#include "kernels.hpp"' not in text, f
