"""The loudness report on an MI355X (include/stn.h "loudness range"; loudness_range_kernel, kernels_loudness.hip):
maximum momentary loudness, maximum short-term loudness and loudness range of the case rows (tests/loudness_range_ref.py: nine spans in
one launch at 8, 44.1 and 48 kHz; the issue's list has nine, so the launch has nine rows) against the host rule on the device's own
segment sums and against the float64 reference, independence of the batch, the finished batch's and the joined programmes' report
against the op on what the fetch delivers, the refusals and the CLI's line."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.arch import tiny_arch
from gpu_util import make_inputs
import loudness_range_ref as ref
from loudness_ref import hop, segments_from_shares

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
RULE_TOL = 2e-5  # dB: two fp32 units in the last place below 128 (the final rounding and the device's log10)
REF_TOL = 0.01   # LU: the bound tests/test_gpu_loudness.py holds for L_b against its float64 reference; twice that for lra
DURS = np.array([3.9, 3.3, 0.5, 4.2, 3.6], np.float32)
HP = (("highpass", 80.0, 0.7071, 0.0),)


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


_DEV = {}


def _device(eng, hz):
    """the op's four results on the case rows at hz, once per rate"""
    if hz not in _DEV:
        x, n = ref.case_rows(hz)
        _DEV[hz] = eng.op_loudness_range(x, hz, n)
    return _DEV[hz]


def _same(a, b):
    return all(u.dtype == v.dtype and u.tobytes() == v.tobytes() for u, v in zip(a, b))


# ---- 1. against the host rule on the device's own segment sums ----------------------------------------------------------------------------
@pytest.mark.parametrize("hz", ref.RATES)
def test_op_equals_the_host_rule_on_the_device_segments(eng, hz):
    x, n = ref.case_rows(hz)
    m, s, lra, n_st = _device(eng, hz)
    o = eng.op_loudness_ex(x, hz, n)
    h = hop(hz)
    worst = 0.0
    for r in range(len(n)):
        seg = segments_from_shares(o["pa"][r], o["pb"][r], n[r], h)
        wm, ws, wl, wn = binding.loudness_range_rule(seg, h)
        print(f"{hz} Hz row {r}: device m {m[r]:.6f} s {s[r]:.6f} lra {lra[r]:.6f} n_st {n_st[r]} | rule m {wm:.6f} s {ws:.6f} lra {wl:.6f} n_st {wn}")
        assert n_st[r] == wn, (hz, r)
        for got, want in ((m[r], wm), (s[r], ws), (lra[r], wl)):
            if math.isinf(want):
                assert got == want, (hz, r, got, want)  # -inf is exactly -inf
            else:
                worst = max(worst, abs(float(got) - want))
                assert abs(float(got) - want) <= RULE_TOL, (hz, r, got, want)
    assert np.all(np.isneginf(m[[0, 1]])) and np.all(np.isneginf(s[[0, 1, 2, 4]])) and np.all(np.isfinite(s[[3, 5, 6, 7, 8]]))
    assert list(n_st[:6]) == [0, 0, 0, 1, 0, 2] and lra[3] == 0.0 and lra[5] > 0.1
    print(f"{hz} Hz: worst distance from the host rule {worst:.2e} dB")


# ---- 2. against the float64 reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", ref.RATES)
def test_op_against_float64(eng, hz):
    m, s, lra, n_st = _device(eng, hz)
    worst = 0.0
    for r, want in enumerate(ref.case_refs(hz)):
        print(f"{hz} Hz row {r}: device m {m[r]:.5f} s {s[r]:.5f} lra {lra[r]:.5f} n_st {n_st[r]} | float64 m {want['m_max']:.5f} "
              f"s {want['s_max']:.5f} lra {want['lra']:.5f} n_st {want['n_st']}")
        assert n_st[r] == want["n_st"], (hz, r)
        for got, w, tol in ((m[r], want["m_max"], REF_TOL), (s[r], want["s_max"], REF_TOL), (lra[r], want["lra"], 2 * REF_TOL)):
            if math.isinf(w):
                assert got == w, (hz, r, got, w)
            else:
                worst = max(worst, abs(float(got) - w))
                assert abs(float(got) - w) <= tol, (hz, r, got, w)
    print(f"{hz} Hz: worst distance from float64 {worst:.2e} LU")


# ---- 3. independence -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", [8000, 44100])
def test_a_row_does_not_depend_on_its_batch(eng, hz):
    x, n = ref.case_rows(hz)
    full = _device(eng, hz)
    assert _same(full, eng.op_loudness_range(x, hz, n))  # two runs
    padded = eng.op_loudness_range(np.pad(x, ((0, 0), (0, 1000))), hz, n)  # W padded by 1000 samples
    assert _same(full, padded)
    for r in (5, 6, 7, 8):
        alone = eng.op_loudness_range(x[r:r + 1], hz, n[r:r + 1])  # row 0 of 1
        among = np.zeros((7, x.shape[1]), np.float32)  # row 5 of 7, among unlike neighbours
        among[[0, 1, 2, 3, 4, 6]] = x[[8, 3, 6, 2, 7, 1]]
        among[5] = x[r]
        seven = eng.op_loudness_range(among, hz, np.array([n[8], n[3], n[6], n[2], n[7], n[r], n[1]], np.int64))
        cut = eng.op_loudness_range(x[r:r + 1, : n[r]], hz)  # the span as a whole row
        for k in range(4):
            assert alone[k][0].tobytes() == full[k][r].tobytes() == seven[k][5].tobytes() == cut[k][0].tobytes(), (hz, r, k)


# ---- 4. the finished batch -----------------------------------------------------------------------------------------------------------------
def _batch_wav(a, e):
    """rows of known dynamics: tones that rise by 7.5 dB per second (rows 0, 2, 4) or fall as fast (rows 1, 3)"""
    B, _, W = e.batch_dims()
    t = np.arange(W) / a.sample_rate
    wav = np.zeros((B, W), np.float32)
    for b in range(B):
        db = -7.5 * np.abs((0.0 if b % 2 else 4.5) - t)
        wav[b] = 0.5 * 10.0 ** (db / 20.0) * np.sin(2 * np.pi * (400.0 + 130.0 * b) * t)
    return wav


@pytest.fixture(scope="module")
def batch():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 5, 14, [14, 9, 5, 12, 7], seed=2)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=DURS)
    for _ in range(3):  # (the third run replays the captured graph)
        e.batch_run(2, 1.05, 9)
    e.dbg_batch_set_wav(_batch_wav(a, e))
    yield a, e
    e.close()


def _spans(e, dur):
    Wo = e.batch_dims()[2]
    return np.array([max(0, min(Wo, int(np.float32(d) * np.float32(e.output_rate)))) for d in dur], np.int64)


@pytest.mark.parametrize("setting", ["off", "chain"])
def test_batch_report_is_the_op_on_the_fetched_rows(batch, setting):
    a, e = batch
    if setting == "chain":
        e.set_output_rate(16000)
        e.set_filters(HP)
        e.set_compressor(binding.COMPRESSOR_SPEECH)
    try:
        cached, replays = e.graphs_cached, e.graph_replays
        before, dur = e.batch_fetch()
        got = e.batch_loudness_range()
        after, _ = e.batch_fetch()
        assert before.tobytes() == after.tobytes()  # the report changes no fetch
        assert e.graphs_cached == cached and e.graph_replays == replays  # and no captured graph
        n = _spans(e, dur)
        want = e.op_loudness_range(before, e.output_rate, n)
        print(f"{setting}: m {got[0]} s {got[1]} lra {got[2]} n_st {got[3]}")
        assert _same(got, want)
        assert np.isneginf(got[1][2]) and got[3][2] == 0 and got[2][2] == 0.0 and np.all(got[3][[0, 1, 3, 4]] >= 2) and np.all(got[2][[0, 1, 3, 4]] > 0.0)
        if setting == "off":  # (0.75 dB per 100 ms between neighbouring windows)
            assert np.all(got[2][[0, 3, 4]] > 2.0)
        # the integrated measurement next to it is untouched, and normalization on or off reports the same signal
        lufs = e.batch_loudness()[0]
        e.set_loudness(-16.0)
        try:
            assert _same(e.batch_loudness_range(), got) and e.batch_loudness()[0].tobytes() == lufs.tobytes()
            assert np.any(e.batch_loudness()[2] != 1.0)
        finally:
            e.set_loudness(None)
        assert e.batch_fetch()[0].tobytes() == before.tobytes()
    finally:
        e.set_compressor(None)
        e.set_filters(None)
        e.set_output_rate(None)


# ---- 5. joined programmes ------------------------------------------------------------------------------------------------------------------
def test_join_report_is_the_op_on_the_joined_fetch(batch):
    a, e = batch
    rows, gap, gap_s = [2, 3], [int(0.3 * a.sample_rate), int(0.2 * a.sample_rate)], [0.3, 0.2]
    joined, prog_len, prog_dur = e.batch_fetch_joined(rows, gap, gap_s, cut=False)
    n = np.array([max(0, min(int(prog_len[g]), int(np.float32(prog_dur[g]) * np.float32(e.output_rate)))) for g in range(2)], np.int64)
    got = e.batch_join_loudness_range(rows, gap, gap_s)
    want = e.op_loudness_range(joined, e.output_rate, n)
    print(f"join: m {got[0]} s {got[1]} lra {got[2]} n_st {got[3]} spans {n}")
    assert _same(got, want) and np.all(got[3] >= 30) and np.all(np.isfinite(got[1]))
    assert joined.shape[1] >= n.max()
    assert e.batch_fetch_joined(rows, gap, gap_s, cut=False)[0].tobytes() == joined.tobytes()


# ---- 6. refusals: messages, not faults -----------------------------------------------------------------------------------------------------
def test_refusals(eng, batch):
    hz = 8000
    with pytest.raises(binding.StnError) as ei:  # a row of 8193 segments: one over the kernel's cap
        eng.op_loudness_range(np.zeros((1, 8193 * hop(hz)), np.float32), hz)
    assert ei.value.code == -1 and "8192" in str(ei.value) and "8193" in str(ei.value)
    m, s, lra, n_st = eng.op_loudness_range(np.zeros((1, 8193 * hop(hz)), np.float32), hz, [8192 * hop(hz)])  # at the cap: measured
    assert np.isneginf(m[0]) and np.isneginf(s[0]) and lra[0] == 0.0 and n_st[0] == 0
    with pytest.raises(binding.StnError) as ei:
        eng.op_loudness_range(np.zeros((65536, 4), np.float32), hz)
    assert ei.value.code == -1 and "65535" in str(ei.value)
    for bad in (7999, 192001):
        with pytest.raises(binding.StnError):
            eng.op_loudness_range(np.zeros((1, 100), np.float32), bad)
    with pytest.raises(binding.StnError) as ei:
        eng.op_loudness_range(np.zeros((1, 100), np.float32), hz, [101])
    assert "outside [0, W]" in str(ei.value)
    # no finished batch
    assert eng._lib.stn_batch_loudness_range(eng._h, None, None, None, None) == -3
    assert "no finished batch" in eng.last_error()
    j, keep = binding._join([1], [0], [0.0])
    import ctypes
    assert eng._lib.stn_batch_join_loudness_range(eng._h, ctypes.byref(j), None, None, None, None) == -3
    # a bad join on a finished batch
    a, e = batch
    for rows in ([2, 2], [6]):
        with pytest.raises(binding.StnError) as ei:
            e.batch_join_loudness_range(rows, 0, 0.0)
        assert ei.value.code == -1, rows
    assert e._lib.stn_batch_join_loudness_range(e._h, None, None, None, None, None) == -1
    assert _same(e.batch_loudness_range(), e.batch_loudness_range())  # and the handle works on


# ---- 7. the CLI ----------------------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^Loudness: integrated (\S+) LUFS, range (\S+) LU, max momentary (\S+) LUFS, max short-term (\S+) LUFS \((\d+) short-term windows\), "
                  r"peak (\S+), gain (\S+)$")


def _run(args, cwd):
    p = subprocess.run([CLI, "--synthetic", "--onnx-dir", "no_assets_here", "--seed", "7", "--total-step", "2"] + args, cwd=cwd, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return [re.sub(r"completed in \S+ sec", "completed", ln) for ln in p.stdout.splitlines()]


def test_cli_prints_one_line_per_file(tmp_path):
    plain = _run(["--n-test", "2", "--save-dir", "plain"], tmp_path)
    assert not any(ln.startswith("Loudness") for ln in plain)
    rep = _run(["--n-test", "2", "--save-dir", "plain", "--loudness-report"], tmp_path)
    assert [ln for ln in rep if not ln.startswith("Loudness:")] == plain  # nothing else changes
    at = [i for i, ln in enumerate(rep) if ln.startswith("Loudness:")]
    assert len(at) == 2 and all(rep[i - 1].startswith("Saved: ") for i in at)
    for i in at:
        g = LINE.match(rep[i])
        assert g, rep[i]
        vals = [float(v) for v in g.groups()]  # ("-inf" parses)
        assert all(re.fullmatch(r"-inf|-?\d+\.\d{3}", v) for v in g.groups()[:4] + g.groups()[5:]), rep[i]
        assert vals[5] > 0 and vals[6] == 1.0  # no --loudness: gain 1
    # several texts as a batch: one line per file
    two = _run(["--n-test", "1", "--save-dir", "two", "--batch", "--text", "first text here|and the second one", "--voice-style", "a,b", "--lang", "en,en",
                "--loudness-report", "--loudness", "-16"], tmp_path)
    lines = [ln for ln in two if ln.startswith("Loudness:")]
    assert len(lines) == 2 and all(LINE.match(ln) for ln in lines) and len(os.listdir(tmp_path / "two")) == 2
