"""Fetch encodings without a GPU (include/stn.h STN_ENC_*, include/stn_host.h stn_wav_encode_as, supertonic_amd/host.py wav_bytes):
the numpy G.711 reference against CPython's audioop on every int16 value and at fixed anchors, the 24-bit PCM rule at its edges,
and the RIFF layout of every encoding read back field by field (and by the stdlib wave module for PCM)."""
import ctypes
import io
import struct
import wave

import numpy as np
import pytest

from supertonic_amd import binding, host
from g711_ref import alaw, pcm16, pcm24, pcm24_int, ulaw

ALL = np.arange(-32768, 32768, dtype=np.int32)


def test_g711_reference_matches_audioop_on_every_int16():
    try:
        import audioop
    except ImportError:
        pytest.skip("audioop is not available in this Python")
    raw = ALL.astype("<i2").tobytes()
    assert np.array_equal(ulaw(ALL), np.frombuffer(audioop.lin2ulaw(raw, 2), np.uint8))
    assert np.array_equal(alaw(ALL), np.frombuffer(audioop.lin2alaw(raw, 2), np.uint8))


def test_g711_anchors():
    s = np.array([0, 32767, -32768, -1, 1], np.int32)
    assert list(ulaw(s)[:3]) == [0xFF, 0x80, 0x00]
    assert list(alaw(s)[:3]) == [0xD5, 0xAA, 0x2A]
    # every codeword is reached but mu-law's negative zero 0x7F (-1 >> 2 = -1 already lands in 0x7E)
    assert set(range(256)) - set(np.unique(ulaw(ALL)).tolist()) == {0x7F} and len(np.unique(alaw(ALL))) == 256


def test_pcm24_rule_edges():
    v = np.array([1.0, -1.0, 1.5, -7.0, 0.0, -0.0, 0.5, -0.5, 1.0 / 8388607.0, -1.0 / 8388607.0,
                  np.nextafter(np.float32(1.0 / 8388607.0), np.float32(0.0))], np.float32)
    got = pcm24_int(v)
    assert list(got[:8]) == [8388607, -8388607, 8388607, -8388607, 0, 0, 4194303, -4194303]
    assert got[8] == 1 and got[9] == -1 and got[10] == 0  # truncation toward zero
    b = pcm24(np.array([1.0, -1.0, 0.0], np.float32))
    assert b.tolist() == [[0xFF, 0xFF, 0x7F], [0x01, 0x00, 0x80], [0, 0, 0]]
    assert pcm16(np.array([1.0, -2.0, 0.99999], np.float32)).tolist() == [32767, -32767, 32766]


def test_encoding_ids_and_bytes():
    L = binding.load()
    for name, e in binding.ENCODINGS.items():
        assert L.stn_encoding_bytes(e) == binding.ENCODING_BYTES[e] and binding.encoding_id(name) == e
    assert L.stn_encoding_bytes(5) == 0 and L.stn_encoding_bytes(-1) == 0
    with pytest.raises(ValueError):
        binding.encoding_id("opus")


def _parse(b):
    """RIFF chunks -> {id: payload}; checks the RIFF size and word alignment"""
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE"
    assert struct.unpack("<I", b[4:8])[0] == len(b) - 8
    out, off = {}, 12
    while off < len(b):
        cid, n = b[off:off + 4], struct.unpack("<I", b[off + 4:off + 8])[0]
        out[cid] = b[off + 8:off + 8 + n]
        off += 8 + n + (n & 1)
    assert off == len(b)
    return out


def _encode_as(enc, samples, n, rate):
    L = host._lib()
    a = np.ascontiguousarray(samples)
    need = L.stn_wav_encode_as(enc, a.ctypes.data, n, rate, None, 0)
    buf = ctypes.create_string_buffer(max(need, 1))
    assert L.stn_wav_encode_as(enc, a.ctypes.data, n, rate, buf, need) == need
    return buf.raw[:need]


@pytest.mark.parametrize("n", [0, 1, 7, 1000])
@pytest.mark.parametrize("enc", [0, 1, 2, 3, 4])
def test_wav_encode_as_layout(enc, n):
    rng = np.random.default_rng(enc * 100 + n)
    v = rng.uniform(-1.1, 1.1, n).astype(np.float32)
    samples = {0: v, 1: pcm16(v), 2: pcm24(v), 3: ulaw(pcm16(v)), 4: alaw(pcm16(v))}[enc]
    rate = 8000 if enc in (3, 4) else 44100
    b = _encode_as(enc, samples, n, rate)
    ch = _parse(b)
    bps = binding.ENCODING_BYTES[enc]
    tag, nch, sr, byte_rate, align, bits = struct.unpack("<HHIIHH", ch[b"fmt "][:16])
    assert (tag, nch, sr, byte_rate, align, bits) == ({0: 3, 1: 1, 2: 1, 3: 7, 4: 6}[enc], 1, rate, rate * bps, bps, 8 * bps)
    if enc in (1, 2):
        assert len(ch[b"fmt "]) == 16 and b"fact" not in ch
    else:
        assert len(ch[b"fmt "]) == 18 and ch[b"fmt "][16:] == b"\0\0"
        assert struct.unpack("<I", ch[b"fact"])[0] == n
    assert ch[b"data"] == np.ascontiguousarray(samples).tobytes() and len(ch[b"data"]) == n * bps
    if enc in (1, 2):
        with wave.open(io.BytesIO(b)) as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, bps, rate, n)
            assert w.readframes(n) == ch[b"data"]


def test_pcm16_encode_as_equals_wav_encode_of_the_representatives():
    """stn_wav_encode_as(PCM16) of int16 samples is stn_wav_encode of floats that writeWavFile quantizes to them"""
    s = np.concatenate([np.arange(-32767, 32768, 97), [32767, -32767, 0]]).astype(np.int16)
    rep = np.where(s == 0, 0.0, (s.astype(np.float64) + np.where(s > 0, 0.5, -0.5)) / 32767.0).astype(np.float32)
    assert np.array_equal(pcm16(rep), s)
    assert _encode_as(1, s, s.size, 44100) == host.wav_bytes(rep, 44100)
    assert host.wav_bytes(s, 44100, encoding="pcm16") == host.wav_bytes(rep, 44100)


def test_unknown_encoding_is_refused():
    L = host._lib()
    x = np.zeros(4, np.uint8)
    assert L.stn_wav_encode_as(9, x.ctypes.data, 4, 8000, None, 0) < 0


@pytest.mark.parametrize("enc", ["f32", "pcm16", "pcm24", "mulaw", "alaw"])
def test_python_wav_bytes_round_trip(enc):
    v = np.random.default_rng(3).uniform(-1, 1, 333).astype(np.float32)
    e = binding.encoding_id(enc)
    samples = {0: v, 1: pcm16(v), 2: pcm24(v), 3: ulaw(pcm16(v)), 4: alaw(pcm16(v))}[e]
    b = host.wav_bytes(samples, 16000, encoding=enc)
    ch = _parse(b)
    assert struct.unpack("<H", ch[b"fmt "][:2])[0] == {0: 3, 1: 1, 2: 1, 3: 7, 4: 6}[e]
    back = np.frombuffer(ch[b"data"], samples.dtype).reshape(samples.shape)
    assert np.array_equal(back, samples)
    assert host.wav_bytes(v, 16000) == host.wav_bytes(v, 16000, encoding=None)  # None: today's bytes
