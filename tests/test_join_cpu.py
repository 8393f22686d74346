"""The plan of a joined fetch (stn_join_plan, include/stn.h "join") against tests/join_ref.py, and every argument
it refuses: host arithmetic, no GPU.  The same cases run once more against the sanitizer build of the host code (make host-asan)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import join_ref  # noqa: E402
from supertonic_amd import binding  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STN_ERR_INVALID = -1

# (name, rows, gap_samples, gap_seconds, member_len, member_dur, W_out, hz)
CASES = [
    ("one programme of one member", [1], [13230], [0.3], [30720], [0.6731], 30720, 44100),
    ("unlike programmes", [3, 1, 2], [13230, 7, 4800], [0.3, 0.25, 0.1], [30720, 61440, 3072, 9216, 12288, 52224],
     [0.66, 1.37, 0.05, 0.2, 0.27, 1.18], 61440, 44100),
    ("gap 0", [2, 2], [0, 0], [0.0, 0.0], [1001, 17, 333, 4095], [0.0227, 0.0003, 0.0075, 0.0928], 4096, 44100),
    ("members of length 0", [3, 2], [5, 3], [0.3, 0.3], [0, 100, 0, 0, 0], [0.0, 0.002, 0.0, 0.0, 0.0], 128, 48000),
    ("trim binds on the row", [2, 1], [2400, 2400], [0.3, 0.3], [4000, 8000, 6000], [9.5, 0.3333, 0.81], 8000, 8000),
    ("B programmes of one", [1, 1, 1], [1, 2, 3], [0.1, 0.2, 0.3], [10, 20, 30], [0.5, 0.25, 0.125], 32, 16000),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("mode", [join_ref.WHOLE, join_ref.TRIM], ids=["whole", "trim"])
def test_plan_equals_the_reference(case, mode):
    _, rows, gs, gt, ml, md, W, hz = case
    want = join_ref.plan(rows, gs, gt, ml, md, hz, mode)
    got = binding.join_plan(rows, gs, gt, ml, md, W, hz, mode=mode)
    assert got["W_join"] == want["W_join"]
    for k in ("prog_len", "seg_len", "seg_dst"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert got["prog_dur"].dtype == np.float32 and got["prog_dur"].tobytes() == want["prog_dur"].tobytes()  # bit-equal fp32 sums
    if mode == join_ref.TRIM and case[0] == "trim binds on the row":
        assert got["seg_len"][0] == 4000 and got["seg_len"][1] == int(np.float32(0.3333) * np.float32(8000)) < 8000  # min binds / duration binds


def test_duration_is_the_fp32_sum_in_member_order():
    durs = np.array([0.1, 0.7, 0.2, 1e-3, 3.3], np.float32)
    got = binding.join_plan([5], [13230], [0.3], [100] * 5, durs, 100, 44100)
    d = np.float32(durs[0])
    for v in durs[1:]:
        d = np.float32(d + np.float32(v + np.float32(0.3)))
    assert got["prog_dur"][0] == d
    assert got["prog_len"][0] == 500 + 4 * 13230 and list(got["seg_dst"]) == [i * (100 + 13230) for i in range(5)]


REFUSED = [
    ("rows sum below B", dict(rows=[1, 1])),
    ("rows sum above B", dict(rows=[2, 2])),
    ("a count of 0", dict(rows=[3, 0])),
    ("a negative count", dict(rows=[4, -1])),
    ("a negative gap", dict(gap_samples=[-1, 0])),
    ("an unknown mode", dict(mode=2)),
    ("an unknown scope", dict(gain_scope=7)),
    ("a member longer than the row", dict(member_len=[10, 20, 4097])),
    ("a negative member length", dict(member_len=[10, -1, 5])),
]


@pytest.mark.parametrize("why,over", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_arguments(why, over):
    a = dict(rows=[2, 1], gap_samples=[3, 3], gap_seconds=[0.3, 0.3], member_len=[10, 20, 30], member_dur=[0.1, 0.2, 0.3], W_out=4096, hz=44100)
    a.update(over)
    with pytest.raises(binding.StnError) as ei:
        binding.join_plan(**a)
    assert ei.value.code == STN_ERR_INVALID and "join" in str(ei.value)


def test_no_programme_is_refused():
    lib = binding.load()
    j = binding.StnJoin(0, None, None, None, 0, 0)
    import ctypes
    lib.stn_join_plan.argtypes = [ctypes.POINTER(binding.StnJoin), ctypes.c_int, ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 7
    assert lib.stn_join_plan(ctypes.byref(j), 1, 8, 44100, None, None, None, None, None, None, None) == STN_ERR_INVALID
    assert lib.stn_join_plan(None, 1, 8, 44100, None, None, None, None, None, None, None) == STN_ERR_INVALID


def test_join_ref_joins_with_the_zero_codeword():
    rows = np.arange(24, dtype=np.uint8).reshape(3, 8) + 1
    progs = join_ref.join(rows, [3, 0, 8], [2, 1], [2, 0], 0xFF)
    assert progs[0].tolist() == [1, 2, 3, 0xFF, 0xFF] and progs[1].tolist() == list(range(17, 25))
    y = join_ref.padded(progs, 9, 0xD5)
    assert y.shape == (2, 9) and y[0, 5:].tolist() == [0xD5] * 4 and y[1, 8] == 0xD5


def test_plan_on_the_sanitizer_build():
    """The plan function is host code: the cases above, refused arguments included, against build_asan/libstn_host_asan.so."""
    if os.environ.get("STN_HOST_ONLY") == "1":
        pytest.skip("already inside the sanitizer run")
    p = subprocess.run(["make", "-C", ROOT, "-s", "host-asan"], capture_output=True, text=True, timeout=900)
    if p.returncode != 0 and ("libasan" in p.stderr or "libubsan" in p.stderr or "sanitize" in p.stderr):
        pytest.skip("this toolchain has no sanitizer runtime: " + p.stderr[-300:])
    assert p.returncode == 0, p.stderr[-2000:]
    rt = " ".join(subprocess.run(["g++", f"-print-file-name={n}"], capture_output=True, text=True).stdout.strip() for n in ("libasan.so", "libstdc++.so"))
    env = dict(os.environ, STN_LIB=os.path.join(ROOT, "build_asan", "libstn_host_asan.so"), STN_HOST_ONLY="1", LD_PRELOAD=rt,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    q = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "tests/test_join_cpu.py"], capture_output=True, text=True,
                       cwd=ROOT, env=env, timeout=900)
    txt = q.stdout + q.stderr
    assert "AddressSanitizer" not in txt and "runtime error:" not in txt, txt[-3000:]
    assert q.returncode == 0 and " passed" in q.stdout, (q.stdout[-3000:], q.stderr[-2000:])
