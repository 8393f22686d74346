"""numpy references of the fetch encodings (include/stn.h, STN_ENC_*): G.711 mu-law and A-law written from ITU-T G.191's table search
form (the segment end tables, as CPython's audioop spells them), and the 16- and 24-bit PCM rules in float32."""
import numpy as np

SEG_UEND = np.array([0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF], np.int32)
SEG_AEND = np.array([0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF], np.int32)


def ulaw(s):
    """int16 samples -> mu-law codewords (uint8): the 14-bit p = s >> 2, |p| clipped at 8159, bias 33, segment by table search."""
    p = np.asarray(s, np.int32) >> 2
    mask = np.where(p < 0, 0x7F, 0xFF)
    m = np.minimum(np.abs(p), 8159) + 33
    seg = np.searchsorted(SEG_UEND, m, side="left")
    code = np.where(seg >= 8, 0x7F ^ mask, ((np.minimum(seg, 7) << 4) | ((m >> (np.minimum(seg, 7) + 1)) & 0xF)) ^ mask)
    return code.astype(np.uint8)


def alaw(s):
    """int16 samples -> A-law codewords (uint8): the 13-bit p = s >> 3, magnitude -p - 1 for p < 0, segment by table search."""
    p = np.asarray(s, np.int32) >> 3
    mask = np.where(p >= 0, 0xD5, 0x55)
    m = np.where(p >= 0, p, -p - 1)
    seg = np.searchsorted(SEG_AEND, m, side="left")
    sg = np.minimum(seg, 7)
    aval = (sg << 4) | np.where(sg < 2, (m >> 1) & 0xF, (m >> sg) & 0xF)
    return np.where(seg >= 8, 0x7F ^ mask, aval ^ mask).astype(np.uint8)


def pcm16(v):
    """writeWavFile's rule in float32: clamp to [-1, 1], * 32767, truncation toward zero."""
    return (np.clip(np.asarray(v, np.float32), -1.0, 1.0) * np.float32(32767.0)).astype(np.int32).astype(np.int16)


def pcm24_int(v):
    """the 24-bit rule in float32: clamp to [-1, 1], * 8388607, truncation toward zero (int32 values)."""
    return (np.clip(np.asarray(v, np.float32), -1.0, 1.0) * np.float32(8388607.0)).astype(np.int32)


def pcm24(v):
    """the 24-bit rule as the fetch delivers it: uint8 [..., 3], little-endian two's complement."""
    c = pcm24_int(v).astype(np.uint32)
    return np.stack([(c & 0xFF), (c >> 8) & 0xFF, (c >> 16) & 0xFF], axis=-1).astype(np.uint8)


def encode(enc, v):
    """fp32 samples -> what an encoded fetch of encoding enc (binding.ENC_*) delivers for them."""
    v = np.asarray(v, np.float32)
    if enc == 0:
        return v
    if enc == 1:
        return pcm16(v)
    if enc == 2:
        return pcm24(v)
    return (ulaw if enc == 3 else alaw)(pcm16(v))
