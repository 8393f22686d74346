"""The loudness report without a GPU (include/stn.h "loudness range"): the host rule stn_loudness_range_rule
against the float64 reference (tests/loudness_range_ref.py) on the segment sums of the case rows and at the rule's edges, a
hand-checked three-level tone, the condition of the case list (no 3 s window of any case row within 0.05 LU of a gate), and the hosts
with stand-ins: the binding's Engine methods over a recording library, TextToSpeech.loudness_report, the CLI flag and the service's
headers."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding, service
from supertonic_amd.output import OutputSettings
from supertonic_amd.tts import Style, TextToSpeech
import loudness_range_ref as ref
from loudness_ref import hop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
SR = 44100
TOL = 1e-9  # dB: the rule and the reference are the same arithmetic in double, summed in different orders


def _agree(got, want):
    m, s, lra, n_st = got
    assert n_st == want["n_st"], (got, want)
    for g, w in ((m, want["m_max"]), (s, want["s_max"]), (lra, want["lra"])):
        assert g == w if math.isinf(w) else abs(g - w) <= TOL, (got, want)


# ---- 1. the rule against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", ref.RATES)
def test_rule_equals_the_reference_on_the_case_rows(hz):
    x, n = ref.case_rows(hz)
    for r, want in enumerate(ref.case_refs(hz)):
        seg = ref.segment_sums(x[r, : n[r]].astype(np.float64), hz)
        assert len(seg) == n[r] // hop(hz)
        _agree(binding.loudness_range_rule(seg, hop(hz)), want)
    # the list holds what it says: no block, one block, no window, one window, two windows, gated windows
    got = [(w["m_max"] > -math.inf, w["s_max"] > -math.inf, w["n_st"]) for w in ref.case_refs(hz)]
    assert got[:6] == [(False, False, 0), (False, False, 0), (True, False, 0), (True, True, 1), (True, False, 0), (True, True, 2)]
    assert got[6][2] == 80 and got[7][2] == 80 and got[8][2] == 88  # of 91, 91 and 88 windows
    assert ref.case_refs(hz)[5]["lra"] > 0.1 and ref.case_refs(hz)[7]["S"].min() < -100.0  # (only the filter's decay is left there)


@pytest.mark.parametrize("nseg", [0, 3, 4, 29, 30, 31])
def test_rule_at_the_edges_of_block_and_window(nseg):
    h = 800
    seg = np.random.default_rng(nseg).uniform(0.5, 2.0, nseg) * h * 1e-3
    want = ref.range_from_segments(seg, h)
    got = binding.loudness_range_rule(seg, h)
    _agree(got, want)
    assert (got[0] > -math.inf) == (nseg >= 4) and (got[1] > -math.inf) == (nseg >= 30)
    assert got[3] == max(0, nseg - 29) and (got[2] > 0) == (nseg >= 31)


def test_rule_gates():
    h = 800
    # every window under -70 LUFS: the maxima are reported, nothing is kept
    quiet = np.full(40, h * 10.0 ** (-7.5))
    got = binding.loudness_range_rule(quiet, h)
    _agree(got, ref.range_from_segments(quiet, h))
    assert got[3] == 0 and got[2] == 0.0 and -76.0 < got[1] < -75.0 and abs(got[0] - got[1]) < 1e-9
    # one window over the absolute gate (-69.90 LUFS; with 29 of its 30 segments the next reads -70.05): n_st = 1, range 0
    one = np.concatenate([np.full(30, h * 1.2e-7), np.full(30, h * 1e-12)])
    got = binding.loudness_range_rule(one, h)
    _agree(got, ref.range_from_segments(one, h))
    assert got[3] == 1 and got[2] == 0.0
    # the relative gate: windows more than 20 LU under the gated mean are dropped, and the range is read among the rest
    two = np.concatenate([np.full(60, h * 1e-2), np.full(60, h * 1e-5)])
    want = ref.range_from_segments(two, h)
    got = binding.loudness_range_rule(two, h)
    _agree(got, want)
    assert 31 < got[3] < 91 - 31 + 30 and want["rel"] < -20.0
    # digital silence: -inf everywhere, nothing kept
    assert binding.loudness_range_rule(np.zeros(50), h) == (-math.inf, -math.inf, 0.0, 0)
    # results are optional, arguments are checked
    L = binding.load()
    seg = np.ones(31)
    assert L.stn_loudness_range_rule(h, 31, seg.ctypes.data, None, None, None, None) == 0
    for bad in ((0, 31, seg.ctypes.data), (h, -1, seg.ctypes.data), (h, 31, None)):
        assert L.stn_loudness_range_rule(*bad, None, None, None, None) < 0, bad
    with pytest.raises(binding.StnError):
        binding.loudness_range_rule(seg, 0)


# ---- 2. a hand-checked case --------------------------------------------------------------------------------------------------------------
def test_three_level_tone_reads_fifteen():
    """A 1 kHz tone of 12 s at amplitude 0.5 x (-15 dB, 0 dB, -30 dB) in 4 s thirds, 48 kHz.  By hand: a sine of amplitude 0.5 has a
    mean square of 0.125 (-9.03 dB); K-weighting lifts 1 kHz by 0.70 dB and the formula's -0.691 takes it back: the thirds read
    -24.02, -9.02 and -39.02 LUFS.  The windows over the absolute gate average about a third of the loud third's power (-13.5), so
    the relative threshold lies near -32.5 and drops the windows dominated by the quiet third.  Of the 80 windows left, the 10th
    percentile lies in the -24.02 third and the 95th in the -9.02 third: LRA = 15.0 LU.  The loudest 3 s window and the loudest 400 ms
    block both lie wholly inside the loud third, so they read the same: s_max - m_max = 0."""
    hz = 48000
    seg = ref.segment_sums(ref.three_level(hz), hz)
    want = ref.range_from_segments(seg, hop(hz))
    assert abs(want["lra"] - 15.000) <= 0.001 and want["n_st"] == 80 and abs(want["rel"] - (-32.505)) <= 0.001  # the reference's numbers
    assert abs(want["m_max"] - (-9.024)) <= 0.001 and abs(want["s_max"] - (-9.024)) <= 0.001
    m, s, lra, n_st = binding.loudness_range_rule(seg, hop(hz))
    assert abs(lra - 15.000) <= 0.5 and abs(lra - want["lra"]) <= 0.5
    assert abs(s - m) < 0.1 and abs(m - (-9.024)) <= 0.001
    assert n_st == 80


# ---- 3. the condition of the case list ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", ref.RATES)
def test_no_window_of_a_case_row_lies_near_a_gate(hz):
    """So that a device rounding cannot flip a gate decision of the GPU test: in the float64 reference every S_j of every case row is at
    least 0.05 LU from -70 and from the row's relative threshold."""
    assert ref.MARGIN == 0.05
    for r, w in enumerate(ref.case_refs(hz)):
        S = w["S"]
        assert w["margin"] >= ref.MARGIN, (hz, r, w["margin"])
        if len(S):
            assert np.abs(S + 70.0).min() >= ref.MARGIN, (hz, r)
        if w["rel"] is not None:
            assert np.abs(S[S > -70.0] - w["rel"]).min() >= ref.MARGIN, (hz, r)
    x, n = ref.case_rows(hz)
    assert x.shape[0] == 9 and n.max() <= 12 * hz and not x.flags.writeable


# ---- 4. the hosts, with stand-ins --------------------------------------------------------------------------------------------------------
class FakeLib:
    """The three engine entries of the report: records the arguments and fills every result with known values."""

    def __init__(self, B):
        self.B, self.calls = B, []

    def _fill(self, ptr, rows):
        for k, (p, t) in enumerate(zip(ptr, (ctypes.c_float,) * 3 + (ctypes.c_int32,))):
            a = (t * rows).from_address(p)
            for r in range(rows):
                a[r] = 10 * k + r
        return 0

    def stn_batch_dims(self, h, B, L, W):
        B._obj.value, L._obj.value, W._obj.value = self.B, 4, 1000
        return 0

    def stn_batch_loudness_range(self, h, *ptr):
        self.calls.append(("batch",))
        return self._fill(ptr, self.B)

    def stn_batch_join_loudness_range(self, h, j, *ptr):
        j = j._obj
        self.calls.append(("join", j.n_prog, list((ctypes.c_int32 * j.n_prog).from_address(j.rows)),
                           list((ctypes.c_int64 * j.n_prog).from_address(j.gap_samples)), j.mode, j.gain_scope))
        return self._fill(ptr, j.n_prog)

    def stn_op_loudness_range(self, h, hz, rows, W, x, n, *ptr):
        self.calls.append(("op", hz, rows, W, None if n is None else list((ctypes.c_int64 * rows).from_address(n))))
        return self._fill(ptr, rows)


def _fake_engine(B):
    e = object.__new__(binding.Engine)
    e._lib, e._h = FakeLib(B), None
    return e


def _filled(out, rows):
    assert [a.dtype for a in out] == [np.float32] * 3 + [np.int32] and all(a.shape == (rows,) for a in out)
    return all(np.array_equal(a, 10 * k + np.arange(rows)) for k, a in enumerate(out))


def test_binding_engine_methods():
    e = _fake_engine(3)
    assert _filled(e.batch_loudness_range(), 3) and e._lib.calls == [("batch",)]
    assert _filled(e.batch_join_loudness_range([2, 3], [100, 200], [0.1, 0.2], mode="trim"), 2)
    assert e._lib.calls[-1] == ("join", 2, [2, 3], [100, 200], binding.JOIN_TRIM, binding.JOIN_GAIN_PROG)
    assert _filled(e.op_loudness_range(np.zeros((4, 50)), 16000, [1, 2, 3, 50]), 4)
    assert e._lib.calls[-1] == ("op", 16000, 4, 50, [1, 2, 3, 50])
    assert _filled(e.op_loudness_range(np.zeros(50), 8000), 1) and e._lib.calls[-1] == ("op", 8000, 1, 50, None)


class FakeEngine:
    def __init__(self, B=5):
        self.B, self.calls = B, []

    def set_output_rate(self, hz):
        self.calls.append(("rate", hz))

    def batch_loudness(self):
        self.calls.append(("rows",))
        return tuple(np.full(self.B, v, np.float32) for v in (-20.0, 0.5, 1.0))

    def batch_loudness_range(self):
        self.calls.append(("rows_range",))
        return tuple(np.full(self.B, v, np.float32) for v in (-15.0, -17.0, 4.0)) + (np.full(self.B, 12, np.int32),)

    def batch_join_loudness(self, rows, gap, gap_s, mode):
        self.calls.append(("join", list(rows), list(gap), [float(v) for v in gap_s], mode))
        return tuple(np.full(len(rows), v, np.float32) for v in (-21.0, 0.6, 1.0))

    def batch_join_loudness_range(self, rows, gap, gap_s, mode):
        self.calls.append(("join_range", list(rows), list(gap), [float(v) for v in gap_s], mode))
        return tuple(np.full(len(rows), v, np.float32) for v in (-14.0, -16.0, 6.0)) + (np.full(len(rows), 40, np.int32),)


KEYS = {"integrated", "peak", "gain", "max_momentary", "max_short_term", "range", "n_short_term"}


def test_tts_loudness_report():
    eng = FakeEngine()
    tts = TextToSpeech(eng, None, {"ae": {"sample_rate": SR, "base_chunk_size": 512}, "ttl": {"chunk_compress_factor": 6, "latent_dim": 24}})
    rep = tts.loudness_report()
    assert set(rep) == KEYS and all(v.shape == (5,) for v in rep.values())
    assert rep["integrated"][0] == -20.0 and rep["max_momentary"][0] == -15.0 and rep["max_short_term"][0] == -17.0
    assert rep["range"][0] == 4.0 and rep["n_short_term"][0] == 12 and rep["n_short_term"].dtype == np.int32
    assert eng.calls == [("rows",), ("rows_range",)]
    # programmes: joined_batch's rows and silences, at the rate of the audio
    del eng.calls[:]
    rep = tts.loudness_report(rows=[2, 3], silence_duration=0.25)
    gap = [int(0.25 * SR)] * 2
    assert eng.calls == [("join", [2, 3], gap, [0.25, 0.25], "whole"), ("join_range", [2, 3], gap, [0.25, 0.25], "whole")]
    assert set(rep) == KEYS and all(v.shape == (2,) for v in rep.values()) and rep["range"][1] == 6.0
    # a call's settings are in force for the report and the instance's afterwards
    del eng.calls[:]
    tts.loudness_report(rows=[5], silence_duration=[0.5], trim_chunks=True, output_rate=16000)
    assert eng.calls == [("rate", 16000), ("join", [5], [8000], [0.5], "trim"), ("join_range", [5], [8000], [0.5], "trim"), ("rate", 0)]
    with pytest.raises(TypeError):
        tts.loudness_report(volume=3)
    with tts.exclusive():  # re-entrant: the methods take the same lock
        assert set(tts.loudness_report()) == KEYS


def test_cli_flag_is_parsed():
    p = subprocess.run([CLI, "--synthetic", "--loudness-report", "--gpus", "2", "--n-test", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--loudness-report needs the batch on one device" in p.stderr, p.stdout + p.stderr
    p = subprocess.run([CLI, "--synthetic", "--loudness-report", "--devices", "0,0", "--n-test", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--loudness-report" in p.stderr, p.stdout + p.stderr


class FakeTTS:
    """Each utterance -> a constant wave of 0.01 s per character; joined_batch and loudness_report as TextToSpeech has them."""
    sample_rate = SR

    def __init__(self):
        self.calls = []

    def _one(self, text):
        dur = np.float32(0.01 * max(len(text), 1))
        n = (int(SR * dur) + 3071) // 3072 * 3072
        return np.full(n, 0.25, np.float32), dur

    def joined_batch(self, texts, langs, style, total_step, speed, rows=None, silence_duration=0.3, loudness_scope="chunk", trim_chunks=False, **out):
        self.calls.append(("joined", list(rows), dict(out)))
        waves, durs, o = [], [], 0
        for g, k in enumerate(rows):
            ws, ds = zip(*[self._one(t) for t in texts[o:o + k]])
            w, d = service.join_chunks(list(ws), list(ds), silence_duration[g], SR)
            waves.append(w)
            durs.append(d)
            o += k
        return waves, np.array(durs, np.float32)

    def batch(self, texts, langs, style, total_step, speed=1.05, **out):
        self.calls.append(("batch", list(texts), dict(out)))
        ws, ds = zip(*[self._one(t) for t in texts])
        wav = np.zeros((len(ws), max(len(w) for w in ws)), np.float32)
        for i, w in enumerate(ws):
            wav[i, : len(w)] = w
        return wav, np.array(ds, np.float32)

    def loudness_report(self, rows=None, silence_duration=0.3, trim_chunks=False, **out):
        self.calls.append(("report", None if rows is None else list(rows), dict(out)))
        n = 1 if rows is None else len(rows)
        vals = {"integrated": -18.25, "peak": 0.25, "gain": 1.0, "max_momentary": -17.5, "max_short_term": -math.inf, "range": 0.0, "n_short_term": 0}
        return {k: np.full(n, v, np.int32 if k == "n_short_term" else np.float32) for k, v in vals.items()}


class PlainTTS(FakeTTS):
    """A synthesizer without the report (the stand-ins of the other tests)."""
    loudness_report = None


def _styles(paths):
    return Style(np.zeros((len(paths), 2, 4), np.float32), np.zeros((len(paths), 2, 3), np.float32))


def _client(tts):
    from fastapi.testclient import TestClient
    return TestClient(service.create_app(tts, max_batch=8, max_wait_ms=5.0, style_loader=_styles))


HEADERS = ("x-loudness-integrated", "x-loudness-range", "x-loudness-max-momentary", "x-loudness-max-short-term")


def test_service_headers():
    tts = FakeTTS()
    body = {"text": "Hello there, this is a test.", "voice_style": "M1"}
    with _client(tts) as c:
        plain = c.post("/tts", json=body)
        assert plain.status_code == 200 and not any(h in plain.headers for h in HEADERS)
        assert [k[0] for k in tts.calls] == ["joined"]  # absent: today's calls and today's response
        same = c.post("/tts", json=dict(body, loudness_report=False))
        assert same.status_code == 200 and same.content == plain.content and dict(same.headers) == dict(plain.headers)
        assert [k[0] for k in tts.calls] == ["joined", "joined"]
        r = c.post("/tts", json=dict(body, loudness_report=True, loudness=-16.0, sample_rate=16000))
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
        assert [r.headers[h] for h in HEADERS] == ["-18.250", "0.000", "-17.500", "-inf"]
        assert r.headers["content-disposition"] == plain.headers["content-disposition"]
        kind, rows, out = tts.calls[-1]
        assert kind == "report" and rows == [1] and out == tts.calls[-2][2] == {"output_rate": 16000, "loudness": (-16.0, -1.0)}
        # the audio does not depend on the field
        quiet = c.post("/tts", json=dict(body, loudness=-16.0, sample_rate=16000))
        assert quiet.content == r.content and not any(h in quiet.headers for h in HEADERS)
        # batch mode: one utterance carries the headers, several (a zip) do not
        r = c.post("/tts", json={"text": ["one text"], "lang": ["en"], "voice_style": ["M1"], "batch": True, "loudness_report": True})
        assert r.status_code == 200 and r.headers["x-loudness-integrated"] == "-18.250" and tts.calls[-1] == ("report", None, {})
        n = len(tts.calls)
        r = c.post("/tts", json={"text": ["a b", "c d e"], "lang": ["en", "en"], "voice_style": ["M1", "M1"], "batch": True, "loudness_report": True})
        assert r.status_code == 200 and r.headers["content-type"] == "application/zip" and not any(h in r.headers for h in HEADERS)
        assert [k[0] for k in tts.calls[n:]] == ["batch"]


def test_service_without_a_reporting_synthesizer_sends_no_headers():
    tts = PlainTTS()
    with _client(tts) as c:
        r = c.post("/tts", json={"text": "Hello there.", "voice_style": "M1", "loudness_report": True})
        assert r.status_code == 200 and not any(h in r.headers for h in HEADERS)
        assert [k[0] for k in tts.calls] == ["joined"]


def test_report_is_no_part_of_the_batch_key():
    import threading
    tts = FakeTTS()
    b = service.DynamicBatcher(tts, max_batch=8, max_wait_ms=200.0)
    out = {}

    def go(i):
        out[i] = b.submit([f"text {i}"], "en", _styles(["x"]), 2, 1.05, silence_duration=0.3, **({"loudness_report": True} if i % 2 else {}))

    th = [threading.Thread(target=go, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    b.close()
    assert sum(b.batches) == 4 and len(b.batches) < 4  # jobs with and without the report shared a batch
    for i in range(4):
        assert len(out[i]) == (3 if i % 2 else 2)
        if i % 2:
            assert set(out[i][2]) == KEYS and out[i][2]["integrated"] == -18.25 and isinstance(out[i][2]["range"], float)
    assert service.batch_key(SR, 2, 1.05) == service.batch_key(SR, 2, 1.05) and "loudness_report" not in service.BatchKey._fields
