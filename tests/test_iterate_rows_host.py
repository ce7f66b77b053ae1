"""The host-only row plan of hipkkt_kkt_system_residuals (csrc/iterate_rows.cpp: the end of each row's walked prefix and
the long-row chunk lists) under AddressSanitizer + UndefinedBehaviorSanitizer, against a brute-force count:
tests/sanitize/iterate_rows_driver.cpp, a stand-alone program built from the same source."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuclarabel_amd", "csrc")


def test_row_plan_matches_brute_force_and_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "iterate_rows_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "sanitize", "iterate_rows_driver.cpp"),
                           os.path.join(CSRC, "iterate_rows.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "ITERATE ROWS DRIVER OK" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
