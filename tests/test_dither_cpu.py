"""The dithered PCM quantizer without a GPU (include/stn.h "dither"): the reference (tests/dither_ref.py) against
Random123's known answers; the host-only entry points stn_dither_noise / stn_dither_quantize against it bit for bit; the reference's
statistics (zero-mean error of variance LSB^2 / 4 whatever the signal, the two spectra, the dead zone of truncation and rounding gone);
every fault the bit-exact GPU test must catch, on its shapes; and the parsers of the binding, OutputSettings, the command line and the
service."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.output import OutputSettings
import dither_cases as dc
import dither_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
NOISY = (dr.TPDF, dr.TPDF_HP)
N = 65536


# ---- the reference and the host functions ------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for c, k, want in kat:
        assert tuple(int(v) for v in dr.philox4x32_10(np.array(c, np.uint64), k)) == want
    got = dr.philox4x32_10(np.array([c for c, _, _ in kat[:1]] * 3, np.uint64), kat[0][1])  # (and vectorized)
    assert got.shape == (3, 4) and all(tuple(int(v) for v in row) == kat[0][2] for row in got)


def test_stream_counter_and_key():
    """sample n's word is output [n & 3] of the block with counter {n >> 2, id lo, id hi, 0xD17E0000 | kind} under key {seed lo, seed hi}"""
    seed, id = 0x0123456789ABCDEF, (5 << 32) | 9
    for kind in (dr.ROW, dr.PROG):
        for n in (0, 1, 3, 4, 6, (1 << 34) - 1):
            blk = dr.philox4x32_10(np.array([n >> 2, 9, 5, 0xD17E0000 | kind], np.uint64), (0x89ABCDEF, 0x01234567))
            assert int(dr.words(seed, kind, id, np.array([n]))[0]) == int(blk[n & 3])
    w = dr.words(seed, 0, id, np.arange(8))
    a, b = (w & np.uint64(0xFFFF)).astype(np.int64), (w >> np.uint64(16)).astype(np.int64)
    assert np.array_equal(dr.noise(dr.TPDF, seed, 0, id, 0, 8) * 65536, a - b)
    assert np.array_equal(dr.noise(dr.TPDF_HP, seed, 0, id, 0, 8) * 65536, a - np.concatenate([b[:1], a[:-1]]))  # a_{-1} := b_0
    assert np.array_equal(dr.noise(dr.TPDF_HP, seed, 0, id, 4, 4), dr.noise(dr.TPDF_HP, seed, 0, id, 0, 8)[4:])  # across the block's edge


@pytest.mark.parametrize("kind", [dr.ROW, dr.PROG])
def test_host_functions_equal_the_reference_bit_for_bit(kind):
    rng = np.random.default_rng(3)
    for id in (0, 7, (1 << 32) + 5, (1 << 63) + (3 << 32) + 1):
        for seed in (0, dc.SEED):
            for n0 in (0, 1, 3, 4, 5, (1 << 34) - 9):
                for n in (0, 1, 2, 4, 5, 9):
                    for mode in (dr.OFF, dr.ROUND) + NOISY:
                        d = binding.dither_noise(mode, seed, kind, id, n0, n)
                        assert np.array_equal(d.astype(np.float64), dr.noise(mode, seed, kind, id, n0, n)), (id, seed, n0, n, mode)
                n = 23  # (several blocks, both ends inside one)
                v = np.concatenate([rng.uniform(-1.3, 1.3, 8), rng.uniform(-2, 2, 8) / 32767, [0.0, 1.0, -1.0, 0.5 / 32767, -0.5 / 32767, 1.5 / 8388607, -2.5 / 8388607]]).astype(np.float32)
                for enc in (dr.PCM16, dr.PCM24):
                    for mode in (dr.OFF, dr.ROUND) + NOISY:
                        vv = v if n0 <= 5 else v[-9:]  # (up to the last sample a stream has)
                        got = binding.dither_quantize(enc, mode, seed, kind, id, n0, vv)
                        want = dr.pack(enc, dr.quantize_stream(enc, mode, seed, kind, id, vv, n0))
                        assert got.dtype == want.dtype and np.array_equal(got, want), (id, seed, n0, enc, mode)


def test_host_functions_refuse_what_the_header_says():
    L = binding._dither_lib()
    d, v, o = np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(12, np.uint8)
    assert L.stn_dither_noise(2, 0, 0, 0, 0, 4, d.ctypes.data) == 0 and L.stn_dither_quantize(1, 2, 0, 1, 0, 0, 4, v.ctypes.data, o.ctypes.data) == 0
    for args in ((4, 0, 0, 0, 0, 4), (-1, 0, 0, 0, 0, 4), (2, 0, 2, 0, 0, 4), (2, 0, 0, 0, -1, 4), (2, 0, 0, 0, (1 << 34) - 3, 4), (2, 0, 0, 0, 0, -1)):
        assert L.stn_dither_noise(*args, d.ctypes.data) < 0, args
    for enc in (0, 3, 4, 5):
        assert L.stn_dither_quantize(enc, 2, 0, 0, 0, 0, 4, v.ctypes.data, o.ctypes.data) < 0
    with pytest.raises(binding.StnError):
        binding.dither_quantize("mulaw", "tpdf", 0, 0, 0, 0, v)
    assert L.stn_dither_noise(2, 0, 0, 0, (1 << 34) - 4, 4, d.ctypes.data) == 0  # the last four samples a stream has


# ---- statistics of the reference ---------------------------------------------------------------------------------------------------------
def _band_ratio(d):
    p = np.abs(np.fft.rfft(d)) ** 2
    h = len(p) // 2
    return p[h:].sum() / p[1:h].sum()


@pytest.mark.parametrize("enc", [dr.PCM16, dr.PCM24])
def test_error_is_zero_mean_with_variance_a_quarter_lsb_whatever_the_signal(enc):
    """Bounds from the reference's own spread (measured over 200 seeds at N = 16384: |mean| <= 0.011, variance in [0.244, 0.256]; the
    sampling error of the variance at N = 65536 is about 0.0015)."""
    S = dr.SCALE[enc]
    for f in (0, 0.1, 0.25, 0.5, 0.75, 0.9):
        v = np.full(N, (100 + f) / S, np.float32)
        x = v.astype(np.float64) * S  # (the constant as fp32 holds it)
        for mode in NOISY:
            err = dr.quantize_stream(enc, mode, dc.SEED, dr.ROW, 7, v) - x
            print(f"enc {enc} f {f} mode {mode}: mean {err.mean():+.4f} var {err.var():.4f}")
            assert abs(err.mean()) <= 0.02 and 0.24 <= err.var() <= 0.26, (enc, f, mode, err.mean(), err.var())
        plain = dr.quantize_stream(enc, dr.ROUND, dc.SEED, dr.ROW, 7, v) - x  # without dither the error is the signal's: a constant
        assert plain.var() == 0 and abs(abs(plain[0]) - min(f, 1 - f)) < 1e-3


def test_spectra_white_and_high_passed():
    """(pi + 2) / (pi - 2) = 4.50 is the upper-to-lower half-band power ratio of 2 - 2 cos w; measured 4.53 (TPDF_HP) and 1.00 (TPDF).
    The density's bounds: a triangular density has variance 1/6 and kurtosis 2.4, so the sample variance of N = 65536 values spreads by
    (1/6) sqrt(1.4 / N) = 0.0008 (0.004 is five of those), the sample mean by sqrt(1/6 / N) = 0.0016 (0.005 is three)."""
    hp, flat = _band_ratio(dr.noise(dr.TPDF_HP, dc.SEED, 0, 7, 0, N)), _band_ratio(dr.noise(dr.TPDF, dc.SEED, 0, 7, 0, N))
    print(f"band power ratio: tpdf-hp {hp:.3f}, tpdf {flat:.3f}")
    assert 4.0 <= hp <= 5.0 and 0.9 <= flat <= 1.1
    for mode in NOISY:  # the same density and power: triangular over (-1, 1), variance 1/6
        d = dr.noise(mode, dc.SEED, 0, 7, 0, N)
        assert np.abs(d).max() < 1.0 and abs(d.var() - 1 / 6) < 0.004 and abs(d.mean()) < 0.005


@pytest.mark.parametrize("enc", [dr.PCM16, dr.PCM24])
def test_dead_zone(enc):
    """a 0.4 LSB sine at 1 kHz: nothing of it survives truncation or rounding; under dither its amplitude is there (0.3972 and 0.3995
    measured with this seed; the standard error of the estimate is sqrt(2 (1/4) / N) = 0.003)"""
    S = dr.SCALE[enc]
    s = np.sin(2 * np.pi * 1000.0 * np.arange(N) / 44100.0)
    v = (0.4 / S * s).astype(np.float32)
    for mode in (dr.OFF, dr.ROUND):
        assert not dr.quantize_stream(enc, mode, dc.SEED, 0, 7, v).any()
    for mode in NOISY:
        q = dr.quantize_stream(enc, mode, dc.SEED, 0, 7, v)
        amp = 2.0 * np.dot(q, s) / N
        print(f"enc {enc} mode {mode}: recovered amplitude {amp:.4f} LSB")
        assert abs(amp - 0.4) <= 0.02, (enc, mode, amp)


# ---- the faults the bit-exact bound must catch, on the GPU test's shapes -------------------------------------------------------------------
def _op_shapes(enc, mode, fault=None):
    """the op-level test's expected bytes over all its widths, with and without the gain"""
    out = []
    for W in dc.WS:
        x = dc.inputs(enc, W)
        for g in (None, dc.GAIN):
            v = x if g is None else x * g[:, None]
            out.append(dr.quantize_rows(enc, mode, dc.SEED, dr.ROW, dc.IDS, v, fault=fault).tobytes())
    return out


@pytest.mark.parametrize("fault,mode,encs", [("same_block_predecessor", dr.TPDF_HP, (dr.PCM16, dr.PCM24)), ("first_predecessor_zero", dr.TPDF_HP, (dr.PCM16, dr.PCM24)),
                                             ("fp32_sum", dr.TPDF, (dr.PCM24,)), ("fp32_sum", dr.TPDF_HP, (dr.PCM24,)),
                                             ("id_high_dropped", dr.TPDF, (dr.PCM16, dr.PCM24)), ("id_high_dropped", dr.TPDF_HP, (dr.PCM16, dr.PCM24))])
def test_a_fault_breaks_equality_on_the_op_shapes(fault, mode, encs):
    for enc in encs:
        good, bad = _op_shapes(enc, mode), _op_shapes(enc, mode, fault)
        differ = [g != b for g, b in zip(good, bad)]
        print(f"{fault} enc {enc} mode {mode}: {sum(differ)} of {len(differ)} comparisons differ")
        assert any(differ), (fault, enc, mode)
        if fault == "same_block_predecessor":  # (first seen where a row reaches sample 4)
            assert not any(d for d, W in zip(differ[::2], dc.WS) if W <= 4) and all(d for d, W in zip(differ[::2], dc.WS) if W >= 33)


@pytest.mark.parametrize("enc", [dr.PCM16, dr.PCM24])
@pytest.mark.parametrize("mode", NOISY)
def test_undithered_gaps_break_equality_on_the_joined_shape(enc, mode):
    a, b = dc.inputs(enc, 48)[0], dc.inputs(enc, 33)[1]
    v = np.concatenate([a, np.zeros(dc.GAP, np.float32), b, np.zeros(7, np.float32)])  # programme 0: two members, the gap, padding
    members, length = [(0, 48), (48 + dc.GAP, 48 + dc.GAP + 33)], 48 + dc.GAP + 33
    good = dr.quantize_prog(enc, mode, dc.SEED, 0, v, length, members)
    bad = dr.quantize_prog(enc, mode, dc.SEED, 0, v, length, members, fault="gaps_undithered")
    assert not np.array_equal(good, bad) and np.array_equal(good[:48], bad[:48]) and not good[length:].any()
    gap = dr.quantize_stream(enc, mode, dc.SEED, dr.PROG, 0, v, length=length)[48:48 + dc.GAP]
    assert set(np.unique(gap)) <= {-1, 0, 1} and 10 <= np.count_nonzero(gap) <= 45  # silence under dither: +-1 a quarter of the time


# ---- parsers -------------------------------------------------------------------------------------------------------------------------------
def test_binding_parser():
    da = binding.dither_args
    assert da(None) is None and da(False) is None and da("off") is None and da(0) is None and da(("off", 9)) is None
    assert da(True) == ("tpdf", 0) and da("tpdf") == ("tpdf", 0) and da("TPDF-HP") == ("tpdf-hp", 0) and da("tpdf_hp", 4) == ("tpdf-hp", 4)
    assert da("round", seed=np.int64(7)) == ("round", 7) and da(3) == ("tpdf-hp", 0) and da(("tpdf", 5)) == ("tpdf", 5) and da(["round", 1]) == ("round", 1)
    assert da({"mode": "tpdf", "seed": (1 << 64) - 1}) == ("tpdf", (1 << 64) - 1) and da({"mode": "tpdf"}, 3) == ("tpdf", 3)
    assert type(da("tpdf", np.int32(3))[1]) is int and hash(da(True)) == hash(("tpdf", 0))
    for bad, word in (("noise", "mode"), (4, "mode"), (1.0, "mode"), (("tpdf",), "(mode, seed)"), (("tpdf", 1, 2), "(mode, seed)"), ({"seed": 1}, "mode"),
                      ({"mode": "tpdf", "shape": 1}, "shape"), (("tpdf", -1), "seed"), (("tpdf", 1 << 64), "seed"), (("tpdf", 1.5), "seed"),
                      (("tpdf", True), "seed")):
        with pytest.raises(ValueError) as ei:
            da(bad)
        assert word in str(ei.value), (bad, str(ei.value))
    with pytest.raises(ValueError):
        da("tpdf", "7")
    assert [binding.dither_mode_id(m) for m in ("off", "round", "tpdf", "tpdf-hp")] == [0, 1, 2, 3] == [dr.OFF, dr.ROUND, dr.TPDF, dr.TPDF_HP]
    assert binding.DITHER_MODES == dr.MODES and (binding.DITHER_ROW, binding.DITHER_PROG) == (dr.ROW, dr.PROG)


def test_command_line_flags():
    if os.path.exists(CLI):  # the command line spells its errors before any device is touched
        for args, word in ((["--dither", "noise"], "one of off, round, tpdf, tpdf-hp"), (["--dither", "tpdf", "--dither-seed", "x"], "unsigned integer"),
                           (["--dither-seed", "-3"], "unsigned integer"), (["--dither-seed", "12a"], "unsigned integer")):
            r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60)
            assert r.returncode == 1 and word in r.stderr, (args, r.stderr)


def test_service_key():
    from supertonic_amd import service
    key = lambda **kw: service.batch_key(44100, 5, 1.05, **kw)
    assert key().settings.dither is None and key(dither=False).settings.dither is False and key(dither="off").settings.dither is False
    assert key(dither=True) == key(dither="tpdf") == key(dither="tpdf", dither_seed=0) and key(dither=True).settings.dither == ("tpdf", 0)
    assert key(dither=True) != key() and key(dither=True) != key(dither=False) and key(dither="tpdf") != key(dither="tpdf-hp")
    assert key(dither="tpdf", dither_seed=1) != key(dither="tpdf") and key(dither_seed=5) == key()  # (a seed alone is dropped)
    assert key(dither="tpdf-hp", dither_seed=9).settings.kwargs() == {"dither": ("tpdf-hp", 9)} and key(dither=False).settings.kwargs() == {"dither": False}
    assert key(dither=True, loudness=-16.0) != key(loudness=-16.0) and hash(key(dither=True)) == hash(key(dither=("tpdf", 0)))
    for kw, word in ((dict(dither="noise"), "mode"), (dict(dither="tpdf", dither_seed=-1), "seed"), (dict(dither_seed=1 << 64), "seed"),
                     (dict(dither="tpdf", dither_seed=1.5), "seed")):
        with pytest.raises(ValueError) as ei:
            key(**kw)
        assert word in str(ei.value), (kw, str(ei.value))


class FakeTTS:
    """The synthesizer's surface with the fetch settings recorded: each utterance a constant wave in the encoding asked for"""
    sample_rate = 44100

    def __init__(self, settings=None):
        self.calls = []
        if settings is not None:
            self.settings = settings

    def _waves(self, texts, encoding):
        durs = np.array([0.01 * max(len(t), 1) for t in texts], np.float32)
        dt = np.int16 if encoding == "pcm16" else np.float32
        return [np.full((int(44100 * d) + 3071) // 3072 * 3072, 1 if dt is np.int16 else 0.25, dt) for d in durs], durs

    def solo_batch(self, texts, langs, style, total_step, speed, dither=None, encoding=None, **_):
        encoding = None if encoding is None else binding.ENCODING_NAMES[binding.encoding_id(encoding)]
        self.calls.append((list(texts), dither, encoding))
        return self._waves(texts, encoding)

    def batch(self, texts, langs, style, total_step, speed=1.05, dither=None, encoding=None, **_):
        self.calls.append((list(texts), dither, encoding))
        ws, ds = self._waves(texts, encoding)
        return np.stack([w[: min(len(x) for x in ws)] for w in ws]), ds


def _styles(paths):
    from supertonic_amd.tts import Style
    return Style(np.zeros((len(paths), 2, 4), np.float32), np.zeros((len(paths), 2, 3), np.float32))


def test_service_validates_the_fields_and_hands_them_to_the_synthesizer():
    from fastapi.testclient import TestClient
    from supertonic_amd import service
    tts = FakeTTS()
    app = service.create_app(tts, max_batch=8, max_wait_ms=1.0, style_loader=_styles)
    with TestClient(app) as c:
        for body in ({"dither": "noise"}, {"dither": 2}, {"dither": "tpdf", "dither_seed": -1}, {"dither_seed": 1 << 64}, {"dither_seed": "x"},
                     {"dither": {"mode": "tpdf"}}):
            r = c.post("/tts", json=dict(text="hello there", **body))
            assert r.status_code == 422, (body, r.status_code, r.text)
        assert tts.calls == []
        # with a mode in force, 16-bit PCM is the GPU's (the float waves would be truncated behind the dither); other encodings as asked
        assert c.post("/tts", json={"text": "hello there", "dither": "tpdf", "dither_seed": 5}).status_code == 200
        assert tts.calls[-1] == (["hello there"], ("tpdf", 5), "pcm16")
        assert c.post("/tts", json={"text": "hello there", "dither": True}).status_code == 200 and tts.calls[-1][1:] == (("tpdf", 0), "pcm16")
        assert c.post("/tts", json={"text": "hello there", "dither": "tpdf-hp", "encoding": "f32"}).status_code == 200
        assert tts.calls[-1][1:] == (("tpdf-hp", 0), "f32")
        for off in (False, "off"):
            assert c.post("/tts", json={"text": "hello there", "dither": off, "dither_seed": 3}).status_code == 200 and tts.calls[-1][1:] == (False, None)
        assert c.post("/tts", json={"text": "hello there"}).status_code == 200 and tts.calls[-1][1:] == (None, None)
        assert c.post("/tts", json={"text": "hello there", "dither_seed": 3}).status_code == 200 and tts.calls[-1][1:] == (None, None)
        r = c.post("/tts", json={"text": ["ab", "abcd"], "lang": ["en", "en"], "voice_style": ["x", "y"], "batch": True, "dither": "round"})
        assert r.status_code == 200 and tts.calls[-1] == (["ab", "abcd"], ("round", 0), "pcm16")
    # a server whose own setting dithers: a request that names none gets the GPU's 16-bit samples as well, one that says off the floats
    tts = FakeTTS(OutputSettings.parse(dither="tpdf").decided())
    with TestClient(service.create_app(tts, max_batch=8, max_wait_ms=1.0, style_loader=_styles)) as c:
        assert c.post("/tts", json={"text": "hello there"}).status_code == 200 and tts.calls[-1][1:] == (None, "pcm16")
        assert c.post("/tts", json={"text": "hello there", "dither": False}).status_code == 200 and tts.calls[-1][1:] == (False, None)


# ---- OutputSettings ------------------------------------------------------------------------------------------------------------------------
class _Engine:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("set_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append((name, a))


def test_output_settings_dither():
    P = OutputSettings.parse
    assert P().dither is None and P(dither=None).dither is None and P(dither=False).dither is False and P(dither="off").dither is False
    assert P(dither=True).dither == ("tpdf", 0) and P(dither=("tpdf-hp", 7)).dither == ("tpdf-hp", 7) and P(dither={"mode": "round"}).dither == ("round", 0)
    assert P(dither="tpdf") == P(dither=True) and hash(P(dither="tpdf")) == hash(P(dither=("tpdf", 0))) and {P(dither=True): 1}[P(dither="tpdf")] == 1
    assert P(dither=True) != P() and P(dither=False) != P() and P(dither=("tpdf", 1)) != P(dither=True) and P(dither=True) != P(dither=True, loudness=-16)
    assert "dither=('tpdf', 0)" in repr(P(dither=True))
    with pytest.raises(ValueError):
        P(dither="noise")
    assert P(dither=True).kwargs() == {"dither": ("tpdf", 0)} and P(**P(dither=("round", 3)).kwargs()) == P(dither=("round", 3))
    assert P(dither=False).over(P(dither=True)).dither is False and P().over(P(dither=True)).dither == ("tpdf", 0)
    on = P(dither=True, loudness=-16)
    assert on.replace(loudness=False).dither == ("tpdf", 0) and on.replace(dither=False).loudness == (-16.0, -1.0)
    # it is no dataclass field (OFF and ALL_OFF are pinned by the equalities of the compressor's and the de-esser's tests): neither names
    # it, dataclasses.replace drops it, and decided() is what leaves nothing unset
    assert "dither" not in [f.name for f in dataclasses.fields(OutputSettings)]
    assert OutputSettings.OFF.dither is None and OutputSettings.ALL_OFF.dither is None and dataclasses.replace(on, loudness=False).dither is None
    d = P().decided()
    assert d.dither is False and d == OutputSettings.ALL_OFF.replace(dither=False) and P(dither="round").decided().dither == ("round", 0)
    assert all(getattr(d, k) is not None for k in ("dither",) + tuple(f.name for f in dataclasses.fields(d)))
    with pytest.raises(TypeError):
        OutputSettings(dither=True)


def test_output_settings_apply_and_restore():
    e = _Engine()
    P = OutputSettings.parse
    P(output_rate=16000, loudness=-16, dither=("tpdf", 3), peak_mode="true").apply(e)  # the last step of the chain is set last
    assert [c[0] for c in e.calls] == ["set_output_rate", "set_loudness", "set_peak_mode", "set_dither"] and e.calls[-1] == ("set_dither", (("tpdf", 3),))
    e.calls.clear()
    P(dither=False).apply(e)
    assert e.calls == [("set_dither", (None,))]
    e.calls.clear()
    P().apply(e)
    assert e.calls == []
    base = P().decided()  # a per-call dither over an instance that has none is put back to off
    with P(dither="tpdf-hp").applied(e, base) as now:
        assert now.dither == ("tpdf-hp", 0) and e.calls == [("set_dither", (("tpdf-hp", 0),))]
    assert e.calls[-1] == ("set_dither", (None,)) and len(e.calls) == 2
    base = P(dither=("round", 2)).decided()  # and over an instance that has one, back to the instance's
    e.calls.clear()
    with P(dither=False).applied(e, base):
        pass
    assert e.calls == [("set_dither", (None,)), ("set_dither", (("round", 2),))]
    e.calls.clear()
    with P(loudness=-20).applied(e, base):  # a call that names none leaves it alone
        pass
    assert [c[0] for c in e.calls] == ["set_loudness", "set_loudness"]
