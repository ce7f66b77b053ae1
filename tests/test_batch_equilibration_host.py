"""The host-only part of the member cost scalings (csrc/data_update.cpp: the check of c[], the member of every stored entry
of P, the words of the segmented data norms) under AddressSanitizer + UndefinedBehaviorSanitizer, against brute force:
tests/sanitize/batch_equilibration_driver.cpp, a stand-alone program built from the same source."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuclarabel_amd", "csrc")


def test_member_cost_tables_match_brute_force_and_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "batch_equilibration_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", CSRC,
                           os.path.join(ROOT, "tests", "sanitize", "batch_equilibration_driver.cpp"),
                           os.path.join(CSRC, "data_update.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "BATCH EQUILIBRATION DRIVER OK" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
