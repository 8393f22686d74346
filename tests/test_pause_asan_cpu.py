"""The pause limit's host rule under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (make pause-asan:
tools/pause_plan_check.cpp linked with csrc/host/pause_plan.cpp; no sanitizer is loaded into Python): the CPU cases of
tests/test_pause_cpu.py against a sample-by-sample second implementation, with cut tables sized exactly so that one pair too many would
be an overrun."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "build_asan", "pause_plan_check")


def test_pause_plan_runs_clean_under_the_sanitizers():
    p = subprocess.run(["make", "-C", ROOT, "-s", "pause-asan"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([PROG], capture_output=True, text=True, timeout=120, env=env)
    txt = p.stdout + p.stderr
    assert "AddressSanitizer" not in txt and "runtime error:" not in txt and "LeakSanitizer" not in txt, txt[-3000:]
    assert p.returncode == 0 and "pause_plan_check OK" in p.stdout and "MISMATCH" not in p.stdout, txt[-3000:]
    assert p.stdout.count(": ok") == 9  # every case ran
