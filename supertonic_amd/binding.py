"""ctypes binding of include/stn.h (libstn.so).  The library is the product path: if it is missing or
no HIP device is present, loading / Engine() raises — there is no CPU fallback."""
import ctypes
import os

import numpy as np

from .arch import StnArch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STN_LIB") or os.path.join(_HERE, "libstn.so")  # STN_LIB: a diagnostic build (timing variants)
_LIB = None

F32, BF16, F16 = 0, 1, 2
_DTYPES = {"f32": F32, "fp32": F32, "float32": F32, "bf16": BF16, "f16": F16, "fp16": F16, "float16": F16, "half": F16,
           F32: F32, BF16: BF16, F16: F16}
ACT_NONE, ACT_GELU, ACT_SILU, ACT_GELU_TANH = 0, 1, 2, 3
EPI_STORE, EPI_RESID, EPI_STORE_T = 0, 1, 2  # GEMM epilogue modes (stn_op_gemm_ex)
FFN_VOCODER, FFN_ESTIMATOR, FFN_TEXT = 1, 2, 4  # ConvNeXt stages (ffn_form)
# kernels of stn_op_layout
LAYOUT_ROW_MAP, LAYOUT_NCL_TO_ROWS, LAYOUT_EULER_NCL, LAYOUT_UNPACK_ROWS, LAYOUT_EMBED, LAYOUT_MASKED_MEAN, LAYOUT_IM2COL, LAYOUT_VOCODER_IN = range(8)
LAYOUT_FILL_ROWS, LAYOUT_HS_PAIRS, LAYOUT_TRIM_LEN = 8, 9, 10
# sample encodings of a fetch (STN_ENC_*, include/stn.h)
ENC_F32, ENC_PCM16, ENC_PCM24, ENC_MULAW, ENC_ALAW = 0, 1, 2, 3, 4
ENCODINGS = {"f32": ENC_F32, "pcm16": ENC_PCM16, "pcm24": ENC_PCM24, "mulaw": ENC_MULAW, "alaw": ENC_ALAW}
ENCODING_NAMES = {v: k for k, v in ENCODINGS.items()}
ENCODING_BYTES = {ENC_F32: 4, ENC_PCM16: 2, ENC_PCM24: 3, ENC_MULAW: 1, ENC_ALAW: 1}
ZERO_CODEWORD = {ENC_F32: 0, ENC_PCM16: 0, ENC_PCM24: 0, ENC_MULAW: 0xFF, ENC_ALAW: 0xD5}  # silence / padding (0x00 is mu-law's -full scale)


def encoding_id(enc):
    """An encoding name ("f32", "pcm16", "pcm24", "mulaw", "alaw") or STN_ENC_* value -> the value."""
    if isinstance(enc, str) and enc.lower() in ENCODINGS:
        return ENCODINGS[enc.lower()]
    if not isinstance(enc, str) and int(enc) in ENCODING_NAMES:
        return int(enc)
    raise ValueError(f"unknown sample encoding {enc!r}: one of {', '.join(ENCODINGS)}")


def encoded_empty(enc, rows, W):
    """An uninitialised array for rows x W samples of an encoding: float32 / int16 / uint8 [rows, W], uint8 [rows, W, 3] for PCM24."""
    e = encoding_id(enc)
    if e == ENC_PCM24:
        return np.empty((rows, W, 3), np.uint8)
    return np.empty((rows, W), {ENC_F32: np.float32, ENC_PCM16: np.int16}.get(e, np.uint8))


# a joined fetch (stn_join, include/stn.h)
JOIN_WHOLE, JOIN_TRIM = 0, 1
JOIN_MODES = {"whole": JOIN_WHOLE, "trim": JOIN_TRIM, JOIN_WHOLE: JOIN_WHOLE, JOIN_TRIM: JOIN_TRIM}
JOIN_GAIN_ROW, JOIN_GAIN_PROG = 0, 1
JOIN_SCOPES = {"row": JOIN_GAIN_ROW, "programme": JOIN_GAIN_PROG, "prog": JOIN_GAIN_PROG, JOIN_GAIN_ROW: JOIN_GAIN_ROW, JOIN_GAIN_PROG: JOIN_GAIN_PROG}


class StnJoin(ctypes.Structure):
    _fields_ = [("n_prog", ctypes.c_int32), ("rows", ctypes.c_void_p), ("gap_samples", ctypes.c_void_p), ("gap_seconds", ctypes.c_void_p),
                ("mode", ctypes.c_int32), ("gain_scope", ctypes.c_int32)]


def _join(rows, gap_samples, gap_seconds, mode="whole", gain_scope="row"):
    """(stn_join, the arrays it points to).  rows: members per programme; the gaps: one value, or one per programme.  mode and
    gain_scope: a name of JOIN_MODES / JOIN_SCOPES, or any integer (passed on as given: the library refuses what it does not know)."""
    rows = np.ascontiguousarray(np.atleast_1d(rows), np.int32)
    G = rows.size
    gs = np.ascontiguousarray(np.broadcast_to(np.asarray(gap_samples, np.int64), (G,)))
    gt = np.ascontiguousarray(np.broadcast_to(np.asarray(gap_seconds, np.float32), (G,)))
    j = StnJoin(G, rows.ctypes.data, gs.ctypes.data, gt.ctypes.data, int(JOIN_MODES.get(mode, mode)), int(JOIN_SCOPES.get(gain_scope, gain_scope)))
    return j, (rows, gs, gt)


def join_plan(rows, gap_samples, gap_seconds, member_len, member_dur, W_out, hz, mode="whole", gain_scope="row"):
    """stn_join_plan (host only, no device): B members of whole lengths member_len (each within [0, W_out]) and durations member_dur at
    rate hz, joined into len(rows) programmes -> dict(W_join, prog_len [G], prog_dur [G] float32, seg_len [B], seg_dst [B]).
    A refused argument raises StnError(STN_ERR_INVALID) with the reason."""
    L = load()
    L.stn_join_plan.argtypes = [ctypes.POINTER(StnJoin), ctypes.c_int, ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 7
    L.stn_join_plan_error.restype = ctypes.c_char_p
    j, keep = _join(rows, gap_samples, gap_seconds, mode, gain_scope)
    ml = np.ascontiguousarray(np.atleast_1d(member_len), np.int64)
    md = np.ascontiguousarray(np.atleast_1d(member_dur), np.float32)
    if md.size != ml.size:
        raise ValueError("member_len and member_dur must have one entry per member")
    B, G = ml.size, keep[0].size
    wj = ctypes.c_int64()
    prog_len, prog_dur = np.zeros(G, np.int64), np.zeros(G, np.float32)
    seg_len, seg_dst = np.zeros(B, np.int64), np.zeros(B, np.int64)
    rc = L.stn_join_plan(ctypes.byref(j), B, int(W_out), int(hz), ml.ctypes.data, md.ctypes.data, ctypes.addressof(wj), prog_len.ctypes.data,
                         prog_dur.ctypes.data, seg_len.ctypes.data, seg_dst.ctypes.data)
    if rc != 0:
        raise StnError(rc, L.stn_join_plan_error().decode())
    return {"W_join": wj.value, "prog_len": prog_len, "prog_dur": prog_dur, "seg_len": seg_len, "seg_dst": seg_dst}


FILTER_TYPES = {"highpass": 0, "lowpass": 1, "notch": 2, "peak": 3, "lowshelf": 4, "highshelf": 5}
FILTER_TYPE_NAMES = {v: k for k, v in FILTER_TYPES.items()}
MAX_FILTERS = 8
FILTER_Q = 0.7071
# presets expand on the host (the C ABI takes only the list): a rumble high-pass; the telephone band as a 4th-order Butterworth
# high-pass at 300 Hz and low-pass at 3400 Hz, each two sections of Q 0.541 and 1.307
FILTER_PRESETS = {
    "rumble": (("highpass", 80.0, FILTER_Q, 0.0),),
    "telephone": (("highpass", 300.0, 0.541, 0.0), ("highpass", 300.0, 1.307, 0.0), ("lowpass", 3400.0, 0.541, 0.0), ("lowpass", 3400.0, 1.307, 0.0)),
}


class StnFilter(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int), ("freq_hz", ctypes.c_float), ("q", ctypes.c_float), ("gain_db", ctypes.c_float)]


def parse_filter_spec(spec):
    """A command-line filter "TYPE:FREQ[:Q[:GAIN_DB]]" (Q 0.7071 and 0 dB when left out) -> (type, freq_hz, q, gain_db).  ValueError
    naming what is wrong."""
    parts = str(spec).split(":")
    if not 2 <= len(parts) <= 4:
        raise ValueError(f"filter {spec!r}: expected TYPE:FREQ[:Q[:GAIN_DB]]")
    if parts[0] not in FILTER_TYPES:
        raise ValueError(f"filter {spec!r}: type must be one of {', '.join(FILTER_TYPES)}")
    try:
        nums = [float(v) for v in parts[1:]]
    except ValueError:
        raise ValueError(f"filter {spec!r}: FREQ, Q and GAIN_DB must be numbers") from None
    return (parts[0], nums[0], nums[1] if len(nums) > 1 else FILTER_Q, nums[2] if len(nums) > 2 else 0.0)


def filter_args(filters, preset=None):
    """A filters argument -> tuple of (type name, freq_hz, q, gain_db): None = no chain; a list whose entries are
    {"type", "freq", "q" (0.7071), "gain_db" (0)} dicts, (type, freq[, q[, gain_db]]) tuples or "TYPE:FREQ[:Q[:GAIN_DB]]" strings.
    preset ("rumble" / "telephone") expands here, in front of the list.  ValueError naming the field for a malformed entry, an unknown
    type or preset, or more than 8 sections; the numeric limits are the C ABI's (filter_error, Engine.set_filters)."""
    out = []
    if preset is not None:
        if preset not in FILTER_PRESETS:
            raise ValueError(f"filter_preset {preset!r}: must be one of {', '.join(FILTER_PRESETS)}")
        out.extend(FILTER_PRESETS[preset])
    if filters is not None:
        if isinstance(filters, (str, bytes, dict)) or not hasattr(filters, "__iter__"):
            raise ValueError(f"filters: a list of filters, not {filters!r}")
        for i, f in enumerate(filters):
            if isinstance(f, str):
                out.append(parse_filter_spec(f))
                continue
            if isinstance(f, dict):
                unknown = set(f) - {"type", "freq", "q", "gain_db"}
                if unknown:
                    raise ValueError(f"filters[{i}]: unknown field {sorted(unknown)[0]!r} (type, freq, q, gain_db)")
                if "type" not in f or "freq" not in f:
                    raise ValueError(f"filters[{i}]: {'type' if 'type' not in f else 'freq'} is required")
                f = (f["type"], f["freq"], f.get("q", FILTER_Q), f.get("gain_db", 0.0))
            if not isinstance(f, (tuple, list)) or not 2 <= len(f) <= 4:
                raise ValueError(f"filters[{i}]: a dict, a TYPE:FREQ[:Q[:GAIN_DB]] string or (type, freq[, q[, gain_db]]), not {f!r}")
            t = FILTER_TYPE_NAMES.get(f[0], f[0]) if isinstance(f[0], int) and not isinstance(f[0], bool) else f[0]
            if t not in FILTER_TYPES:
                raise ValueError(f"filters[{i}]: type {f[0]!r} must be one of {', '.join(FILTER_TYPES)}")
            vals = list(f[1:]) + [FILTER_Q, 0.0][len(f) - 2:]
            for name, v in zip(("freq", "q", "gain_db"), vals):
                if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
                    raise ValueError(f"filters[{i}]: {name} must be a finite number, not {v!r}")
            out.append((t, float(vals[0]), float(vals[1]), float(vals[2])))
    if len(out) > MAX_FILTERS:
        raise ValueError(f"filters: {len(out)} sections, at most {MAX_FILTERS}")
    return tuple(out)


def _filter_array(filters):
    f = filter_args(filters)
    arr = (StnFilter * max(len(f), 1))()
    for i, (t, fr, q, g) in enumerate(f):
        arr[i] = StnFilter(FILTER_TYPES[t], fr, q, g)
    return len(f), arr


def filter_error(filters, rate_hz):
    """Why Engine.set_filters would refuse the chain at an output rate of rate_hz (host only): "" when it would not; the message names
    the filter and the field."""
    n, arr = _filter_array(filters)
    return load().stn_filter_error(n, arr, int(rate_hz)).decode()


def filter_coefs(f, rate_hz):
    """One section at rate_hz (host only) -> (c float64 [5]: b0 b1 b2 a1 a2 of the double design, a0 = 1; c32 float32 [5]: what the GPU
    multiplies by).  StnError for what set_filters refuses at that rate."""
    n, arr = _filter_array([f])
    c, c32 = np.zeros(5, np.float64), np.zeros(5, np.float32)
    rc = load().stn_filter_coefs(arr, int(rate_hz), c, c32)
    if rc < 0:
        raise StnError(rc, filter_error([f], rate_hz) or "stn_filter_coefs failed")
    return c, c32


def filter_response(filters, rate_hz, freq_hz):
    """Magnitude in dB of the fp32-rounded chain (what is actually run) at the frequencies freq_hz (host only)."""
    n, arr = _filter_array(filters)
    fr = np.ascontiguousarray(np.atleast_1d(freq_hz), np.float64)
    out = np.zeros(fr.shape, np.float64)
    rc = load().stn_filter_response(n, arr, int(rate_hz), fr.size, fr, out)
    if rc < 0:
        raise StnError(rc, filter_error(filters, rate_hz) or "stn_filter_response failed")
    return out


def filter_geometry():
    """(chunk, wg_span, scan_tile_chunks, biquads_per_section) of the filter passes' decomposition."""
    v = [ctypes.c_int() for _ in range(4)]
    load().stn_dbg_filter_geometry(*(ctypes.byref(x) for x in v))
    return tuple(x.value for x in v)


COMPRESSOR_FIELDS = ("threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "makeup_db")
# the documented "speech" default: -24 dB, 3:1, a 6 dB knee, 5 ms attack, 120 ms release, no makeup
COMPRESSOR_SPEECH = (-24.0, 3.0, 6.0, 5.0, 120.0, 0.0)
COMPRESSOR_PRESETS = {"speech": COMPRESSOR_SPEECH}
# what a spelling that leaves fields out fills them with (THRESHOLD and RATIO are always given there)
_COMPRESSOR_REST = COMPRESSOR_SPEECH[2:]

EXPANDER_FIELDS = ("threshold_db", "ratio", "knee_db", "range_db", "attack_ms", "hold_ms", "release_ms")
# the documented defaults: "speech" -50 dB, 3:1, a 6 dB knee, at most 24 dB, 1 ms attack, 30 ms hold, 150 ms release; "gate" -45 dB,
# 20:1, no knee, 60 dB, 0.5 ms, 50 ms, 100 ms
EXPANDER_SPEECH = (-50.0, 3.0, 6.0, 24.0, 1.0, 30.0, 150.0)
EXPANDER_GATE = (-45.0, 20.0, 0.0, 60.0, 0.5, 50.0, 100.0)
EXPANDER_PRESETS = {"speech": EXPANDER_SPEECH, "gate": EXPANDER_GATE}

DEESSER_FIELDS = ("freq_hz", "threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "range_db", "mode")
DEESSER_MODES = ("split", "wide")  # STN_DEESS_SPLIT, STN_DEESS_WIDE
# the documented "speech" default: 5500 Hz, -30 dB, 4:1, a 6 dB knee, 1 ms attack, 40 ms release, at most 12 dB, on the band alone
DEESSER_SPEECH = (5500.0, -30.0, 4.0, 6.0, 1.0, 40.0, 12.0, "split")
DEESSER_PRESETS = {"speech": DEESSER_SPEECH}
_DEESSER_SPELLING = "FREQ:THRESHOLD[:RATIO[:KNEE[:ATTACK_MS[:RELEASE_MS[:RANGE_DB[:MODE]]]]]]"


class StnCompressor(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in COMPRESSOR_FIELDS]


class StnExpander(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in EXPANDER_FIELDS]


class StnDeesser(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in DEESSER_FIELDS[:7]] + [("mode", ctypes.c_int)]


class _Dynamics:
    """What the three dynamics stages' arguments differ by: the unit's name, its fields (floats, and behind them the de-esser's mode),
    its presets, the command line's spelling and its C struct.  Everything below that takes one is the same for all three."""

    def __init__(self, unit, fields, presets, spelling, struct, modes=()):
        self.unit, self.fields, self.presets, self.spelling, self.struct, self.modes = unit, fields, presets, spelling, struct, modes
        self.nf = len(fields) - bool(modes)  # the float fields
        self.words = spelling.replace("[", "").replace("]", "").split(":")[:self.nf]


_COMPRESSOR = _Dynamics("compressor", COMPRESSOR_FIELDS, COMPRESSOR_PRESETS, "THRESHOLD:RATIO[:KNEE[:ATTACK_MS[:RELEASE_MS[:MAKEUP_DB]]]]", StnCompressor)
_EXPANDER = _Dynamics("expander", EXPANDER_FIELDS, EXPANDER_PRESETS, "THRESHOLD:RATIO[:KNEE[:RANGE_DB[:ATTACK_MS[:HOLD_MS[:RELEASE_MS]]]]]", StnExpander)
_DEESSER = _Dynamics("deesser", DEESSER_FIELDS, DEESSER_PRESETS, _DEESSER_SPELLING, StnDeesser, DEESSER_MODES)


def _dyn_mode(d, v):
    if isinstance(v, str) and v in d.modes:
        return v
    if not isinstance(v, bool) and isinstance(v, (int, np.integer)) and 0 <= int(v) < len(d.modes):
        return d.modes[int(v)]
    raise ValueError(f"{d.unit}: mode must be one of {', '.join(d.modes)}, not {v!r}")


def _dyn_spec(d, spec, preset=None, base=None):
    """the command line's spelling -> the tuple; what is left out comes from base, or from the preset ("speech" unless given)"""
    parts = str(spec).split(":")
    if not 2 <= len(parts) <= len(d.fields):
        raise ValueError(f"{d.unit} {spec!r}: expected {d.spelling}")
    try:
        nums = [float(v) for v in parts[:d.nf]]
    except ValueError:
        raise ValueError(f"{d.unit} {spec!r}: {', '.join(d.words[:-1])} and {d.words[-1]} must be numbers") from None
    if len(parts) > d.nf and parts[d.nf] not in d.modes:
        raise ValueError(f"{d.unit} {spec!r}: MODE must be one of {', '.join(d.modes)}")
    base = base or d.presets[preset or "speech"]
    return tuple(nums) + base[len(nums):d.nf] + ((parts[d.nf] if len(parts) > d.nf else base[d.nf],) if d.modes else ())


def _dyn_args(d, value, preset):
    """a setting argument -> the tuple, or None for off (what compressor_args, expander_args and deesser_args document)"""
    if preset is not None:
        if preset not in d.presets:
            raise ValueError(f"{d.unit}_preset {preset!r}: must be one of {', '.join(d.presets)}")
        if value is None or value is False:
            value = True
    if value is None or value is False:
        return None
    base = d.presets[preset or "speech"]
    if value is True:
        return base
    if isinstance(value, str):
        return _dyn_spec(d, value, preset)
    if isinstance(value, dict):
        unknown = set(value) - set(d.fields)
        if unknown:
            raise ValueError(f"{d.unit}: unknown field {sorted(unknown)[0]!r} ({', '.join(d.fields)})")
        vals = [value.get(n, v) for n, v in zip(d.fields, base)]
    elif isinstance(value, (tuple, list)) and len(value) == len(d.fields):
        vals = list(value)
    else:
        n = len(d.fields)
        raise ValueError(f"{d.unit}: True, a dict of {', '.join(d.fields)}, or {'an' if n == 8 else 'a'} {n}-tuple of them, not {value!r}")
    for name, v in zip(d.fields[:d.nf], vals):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{d.unit}: {name} must be a finite number, not {v!r}")
    return tuple(float(v) for v in vals[:d.nf]) + ((_dyn_mode(d, vals[d.nf]),) if d.modes else ())


def _dyn_struct(d, value, off_ok=False):
    """the C struct of a setting argument (off_ok: None for off)"""
    c = _dyn_args(d, value, None)
    if c is None:
        if off_ok:
            return None
        raise ValueError(f"{d.unit}: a setting is needed here, not off")
    return d.struct(*c[:d.nf], *(d.modes.index(m) for m in c[d.nf:]))


def _dyn_tuple(d, c):
    """a C struct as the tuple the *_args give"""
    return tuple(getattr(c, n) for n in d.fields[:d.nf]) + ((d.modes[c.mode],) if d.modes else ())


def _set_dynamics(owner, fn, handle, d, value):
    """stn_set_<unit> / stn_group_set_<unit> (fn) on an Engine's or a Group's handle"""
    c = _dyn_struct(d, value, off_ok=True)
    owner._ck(fn(handle, int(c is not None), None if c is None else ctypes.byref(c)))


def _dyn_error(d, value, rate_hz):
    return getattr(load(), f"stn_{d.unit}_error")(ctypes.byref(_dyn_struct(d, value)), int(rate_hz)).decode()


def _dyn_ck(d, rc, what, value, rate_hz):
    """the return code of the host-only entry stn_<unit>_<what>: StnError with the unit's own reason"""
    if rc < 0:
        raise StnError(rc, _dyn_error(d, value, rate_hz) or f"stn_{d.unit}_{what} failed")


def _dyn_curve(d, value, in_db):
    c = _dyn_struct(d, value)
    x = np.ascontiguousarray(np.atleast_1d(in_db), np.float64)
    out = np.zeros(x.shape, np.float64)
    _dyn_ck(d, getattr(load(), f"stn_{d.unit}_curve")(ctypes.byref(c), x.size, x, out), "curve", value, 0)
    return out


def _dyn_coefs(d, value, rate_hz, n, *more):
    c = _dyn_struct(d, value)
    k, k32 = np.zeros(n, np.float64), np.zeros(n, np.float32)
    _dyn_ck(d, getattr(load(), f"stn_{d.unit}_coefs")(ctypes.byref(c), int(rate_hz), k, k32, *more), "coefs", value, rate_hz)
    return k, k32


def parse_compressor_spec(spec):
    """A command-line compressor "THRESHOLD:RATIO[:KNEE[:ATTACK_MS[:RELEASE_MS[:MAKEUP_DB]]]]" (the speech default's knee 6, attack 5,
    release 120 and makeup 0 when left out) -> the 6-tuple of floats.  ValueError naming what is wrong."""
    return _dyn_spec(_COMPRESSOR, spec, base=COMPRESSOR_SPEECH[:2] + _COMPRESSOR_REST)


def compressor_args(compressor, preset=None):
    """A compressor argument -> the 6-tuple of floats (threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db), or None for off
    (None or False).  True is the "speech" default (-24 dB, 3:1, knee 6 dB, attack 5 ms, release 120 ms, makeup 0 dB); a dict names
    fields and takes the others from that default; a 6-tuple gives all six; a "THRESHOLD:RATIO[:...]" string is the command line's
    spelling.  preset ("speech") stands for True.  ValueError naming the field for a malformed value or an unknown field or preset; the
    numeric limits are the C ABI's (compressor_error, Engine.set_compressor)."""
    return _dyn_args(_COMPRESSOR, compressor, preset)


def _compressor_struct(compressor):
    return _dyn_struct(_COMPRESSOR, compressor)


def compressor_error(compressor, rate_hz=0):
    """Why Engine.set_compressor would refuse the setting (host only): "" when it would not; the message names the field."""
    return _dyn_error(_COMPRESSOR, compressor, rate_hz)


def compressor_coefs(compressor, rate_hz):
    """(k float64 [2]: kA, kR = -expm1(-1000 / (ms rate)); k32 float32 [2]: what the GPU multiplies by) at rate_hz (host only)."""
    return _dyn_coefs(_COMPRESSOR, compressor, rate_hz, 2)


def compressor_curve(compressor, in_db):
    """The static curve, makeup included: output level in dB at the input levels in_db (host only, float64)."""
    return _dyn_curve(_COMPRESSOR, compressor, in_db)


def parse_expander_spec(spec, preset=None):
    """A command-line expander "THRESHOLD:RATIO[:KNEE[:RANGE_DB[:ATTACK_MS[:HOLD_MS[:RELEASE_MS]]]]]" (what is left out comes from the
    preset, "speech" unless given) -> the 7-tuple of floats.  ValueError naming what is wrong."""
    return _dyn_spec(_EXPANDER, spec, preset)


def expander_args(expander, preset=None):
    """An expander argument -> the 7-tuple of floats (threshold_db, ratio, knee_db, range_db, attack_ms, hold_ms, release_ms), or None
    for off (None or False).  True is the preset ("speech" unless given: -50 dB, 3:1, knee 6 dB, range 24 dB, attack 1 ms, hold 30 ms,
    release 150 ms; "gate": -45 dB, 20:1, knee 0, range 60 dB, 0.5 ms, 50 ms, 100 ms); a dict names fields and takes the others from
    the preset; a 7-tuple gives all seven; a "THRESHOLD:RATIO[:...]" string is the command line's spelling.  A preset alone stands for
    True.  ValueError naming the field for a malformed value or an unknown field or preset; the numeric limits are the C ABI's
    (expander_error, Engine.set_expander)."""
    return _dyn_args(_EXPANDER, expander, preset)


def _expander_struct(expander):
    return _dyn_struct(_EXPANDER, expander)


def expander_error(expander, rate_hz=0):
    """Why Engine.set_expander would refuse the setting (host only): "" when it would not; the message names the field."""
    return _dyn_error(_EXPANDER, expander, rate_hz)


def expander_coefs(expander, rate_hz):
    """(k float64 [3]: kA = -expm1(-1000 / (attack_ms rate)), delta = range_db 1000 / (release_ms rate), Bh = delta32 Hs; k32 float32
    [3]: what the GPU computes with; Hs: the hold in samples) at rate_hz (host only)."""
    hs = ctypes.c_int64()
    k, k32 = _dyn_coefs(_EXPANDER, expander, rate_hz, 3, ctypes.byref(hs))
    return k, k32, int(hs.value)


def expander_curve(expander, in_db):
    """The static curve: output level in dB at the input levels in_db (host only, float64)."""
    return _dyn_curve(_EXPANDER, expander, in_db)


def parse_deesser_spec(spec):
    """A command-line de-esser "FREQ:THRESHOLD[:RATIO[:KNEE[:ATTACK_MS[:RELEASE_MS[:RANGE_DB[:MODE]]]]]]" (the speech default's values for
    what is left out; MODE split or wide) -> the 8-tuple.  ValueError naming what is wrong."""
    return _dyn_spec(_DEESSER, spec)


def deesser_args(deesser, preset=None):
    """A de-esser argument -> the 8-tuple (freq_hz, threshold_db, ratio, knee_db, attack_ms, release_ms, range_db as floats, mode "split"
    or "wide"), or None for off (None or False).  True is the "speech" default (5500 Hz, -30 dB, 4:1, knee 6 dB, attack 1 ms, release
    40 ms, range 12 dB, split); a dict names fields and takes the others from that default; an 8-tuple gives all eight (mode by name, or
    0 / 1); a "FREQ:THRESHOLD[:...]" string is the command line's spelling.  preset ("speech") stands for True.  ValueError naming the
    field for a malformed value or an unknown field or preset; the numeric limits are the C ABI's (deesser_error, Engine.set_deesser)."""
    return _dyn_args(_DEESSER, deesser, preset)


def _deesser_struct(deesser):
    return _dyn_struct(_DEESSER, deesser)


def deesser_error(deesser, rate_hz=0):
    """Why Engine.set_deesser would refuse the setting at an output rate of rate_hz (host only; 0: the limits that need no rate): ""
    when it would not; the message names the field."""
    return _dyn_error(_DEESSER, deesser, rate_hz)


def deesser_band(deesser, rate_hz):
    """(c float64 [2, 5], c32 float32 [2, 5]): the band's two high-pass sections b0 b1 b2 a1 a2 at rate_hz, the double design and what
    the GPU multiplies by (host only)."""
    s = _deesser_struct(deesser)
    c, c32 = np.zeros(10, np.float64), np.zeros(10, np.float32)
    _dyn_ck(_DEESSER, load().stn_deesser_band(ctypes.byref(s), int(rate_hz), c, c32), "band", deesser, rate_hz)
    return c.reshape(2, 5), c32.reshape(2, 5)


def deesser_coefs(deesser, rate_hz):
    """(k float64 [2]: kA, kR = -expm1(-1000 / (ms rate)); k32 float32 [2]: what the GPU multiplies by) at rate_hz (host only)."""
    return _dyn_coefs(_DEESSER, deesser, rate_hz, 2)


class StnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"stn error {code}: {msg}")
        self.code = code


class StnConfig(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("dtype", ctypes.c_int32)]


_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")


def runtime_info(L=None):
    """{'hip_built': ..., 'hip_runtime': ..., 'torch_preloaded': ...}: which HIP runtime libstn.so was compiled against and which
    one this process bound it to (PyTorch-ROCm wheels bundle their own; importing torch first makes that the one in use)."""
    import sys
    L = L or load()
    b, r = ctypes.c_int(), ctypes.c_int()
    L.stn_hip_versions(ctypes.byref(b), ctypes.byref(r))
    return {"hip_built": b.value, "hip_runtime": r.value, "torch_preloaded": "torch" in sys.modules, "lib": LIB_PATH}


def device_count():
    """Visible HIP devices, through libstn.so (no PyTorch needed)."""
    n = load().stn_device_count()
    if n < 0:
        raise StnError(n, "hipGetDeviceCount failed")
    return n


def device_sync(device=0):
    """hipDeviceSynchronize on `device`, through libstn.so."""
    rc = load().stn_device_sync(int(device))
    if rc < 0:
        raise StnError(rc, "hipDeviceSynchronize failed")


def _check_runtime(L):
    """libstn.so's code objects are built and tested with the system ROCm; when the process bound it to another HIP runtime major.minor
    (torch's bundled copy), say so once: not an error — the GPU suite runs in exactly that configuration and
    records it (tests/test_gpu_runtime_record.py) — but a mismatch the user should be able to see."""
    import warnings
    info = runtime_info(L)
    b, r = info["hip_built"], info["hip_runtime"]
    if r > 0 and (b // 100000) != (r // 100000):  # HIP_VERSION = major * 10^7 + minor * 10^5 + patch
        warnings.warn(f"libstn.so was built against HIP {b // 10000000}.{b // 100000 % 100} but runs on HIP runtime {r // 10000000}.{r // 100000 % 100}"
                      + (" (PyTorch's bundled runtime was loaded first; set STN_NO_TORCH_PRELOAD=1 in processes that do not need torch)" if info["torch_preloaded"] else ""),
                      RuntimeWarning, stacklevel=3)


def load():
    """Load libstn.so (built by `make` / __graft_entry__.build()).  Raises if it is not there."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} not found: build it with `make` (hipcc --offload-arch=gfx950); "
                                "the engine has no fallback path")
    # PyTorch-ROCm wheels carry their own copy of the HIP runtime.  If libstn.so brings the system runtime in first, a later
    # `import torch` in the same process finds no GPU ("No HIP GPUs are available"); the other order works (libstn.so then
    # resolves against the runtime that is already loaded).  The multi-GPU helpers (supertonic_amd.dist) and bench.py need
    # torch in the same process, so when torch is installed it is imported before the library (STN_NO_TORCH_PRELOAD=1 skips this).
    import sys
    if "torch" not in sys.modules and os.environ.get("STN_NO_TORCH_PRELOAD") != "1" and os.environ.get("STN_HOST_ONLY") != "1":
        import importlib.util
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    if os.environ.get("STN_HOST_ONLY") == "1":
        # the sanitizer build of the host-side parsers (make host-asan, STN_LIB=build_asan/libstn_host_asan.so): include/stn_host.h
        # only, no engine entry points to declare (supertonic_amd.host sets its own signatures)
        _LIB = L
        return L
    vp, ci, cu64, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_float
    L.stn_hip_versions.argtypes = [ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.stn_ffn_fused_forms.argtypes = [ci, ci, ci]
    L.stn_device_count.argtypes = []
    L.stn_device_sync.argtypes = [ci]
    _check_runtime(L)
    L.stn_version.restype = ctypes.c_char_p
    L.stn_create.argtypes = [ctypes.POINTER(StnConfig), ctypes.POINTER(vp)]
    L.stn_destroy.argtypes = [vp]
    L.stn_last_error.restype = ctypes.c_char_p
    L.stn_last_error.argtypes = [vp]
    L.stn_load_dir.argtypes = [vp, ctypes.c_char_p]
    L.stn_tensor_names.argtypes = [vp, ctypes.POINTER(StnArch), ctypes.c_char_p, ctypes.c_size_t]
    L.stn_load_synthetic.argtypes = [vp, ctypes.POINTER(StnArch), cu64]
    L.stn_get_arch.argtypes = [vp, ctypes.POINTER(StnArch)]
    L.stn_param_count.restype = ctypes.c_int64
    L.stn_param_count.argtypes = [vp]
    L.stn_duration.argtypes = [vp, ci, ci, _i64p, _f32p, _f32p, _f32p]
    L.stn_text_enc.argtypes = [vp, ci, ci, _i64p, _f32p, _f32p, _f32p]
    L.stn_vector_est.argtypes = [vp, ci, ci, ci] + [_f32p] * 8
    L.stn_vocoder.argtypes = [vp, ci, ci, _f32p, _f32p]
    L.stn_batch_upload.argtypes = [vp, ci, ci, _i64p, _f32p, _f32p, _f32p, vp, vp]
    L.stn_batch_set_noise.argtypes = [vp, _f32p, ci]
    L.stn_batch_run.argtypes = [vp, ci, cf, cu64]
    L.stn_set_graph_mode.argtypes = [vp, ci]
    L.stn_set_vocoder_mode.argtypes = [vp, ci]
    L.stn_set_row_layout.argtypes = [vp, ci]
    L.stn_set_fused_xattn.argtypes = [vp, ci]
    L.stn_set_shape_buckets.argtypes = [vp, ci]
    L.stn_set_duration_read.argtypes = [vp, ci]
    L.stn_set_gelu_form.argtypes = [vp, ci]
    L.stn_get_gelu_form.argtypes = [vp]
    L.stn_batch_ve_rows.argtypes = [vp]
    L.stn_batch_ve_rows.restype = ctypes.c_int64
    L.stn_batch_vo_rows.argtypes = [vp]
    L.stn_batch_vo_rows.restype = ctypes.c_int64
    L.stn_graph_replays.restype = ctypes.c_int64
    L.stn_graph_replays.argtypes = [vp]
    L.stn_graphs_cached.restype = ctypes.c_int64
    L.stn_graphs_cached.argtypes = [vp]
    L.stn_batch_dims.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_int64)]
    L.stn_batch_fetch.argtypes = [vp, vp, ctypes.c_size_t, vp]
    L.stn_batch_fetch_latent.argtypes = [vp, _f32p]
    L.stn_batch_fetch_pcm16.argtypes = [vp, vp, ctypes.c_size_t, vp]
    L.stn_batch_fetch_pcm16_begin.argtypes = [vp, ci]
    L.stn_batch_fetch_slot_dims.argtypes = [vp, ci, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_int64)]
    L.stn_batch_fetch_pcm16_end.argtypes = [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), vp]
    L.stn_host_alloc_pinned.restype = vp
    L.stn_host_alloc_pinned.argtypes = [ctypes.c_size_t]
    L.stn_host_free_pinned.argtypes = [vp]
    L.stn_batch_wav_device_ptr.argtypes = [vp, ctypes.POINTER(vp)]
    L.stn_sync.argtypes = [vp]
    L.stn_set_stream.argtypes = [vp, vp]
    L.stn_batch_copy_wav_device.argtypes = [vp, vp, ctypes.c_int64]
    L.stn_batch_copy_pcm16_device.argtypes = [vp, vp, ctypes.c_int64]
    L.stn_profile_filter.argtypes = [vp, ctypes.c_char_p]
    L.stn_profile_sample.argtypes = [vp, ci]
    L.stn_launch_log_enable.argtypes = [vp, ci]
    L.stn_dbg_xattn_hs_enable.argtypes = [vp, ci]
    L.stn_dbg_xattn_hs_stamps.argtypes = [vp, vp, ctypes.c_size_t]
    L.stn_dbg_xattn_hs_stamps.restype = ctypes.c_int64
    L.stn_dbg_fold_run_frames.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.stn_dbg_fold_run_frames.restype = ctypes.c_int
    L.stn_dbg_gemm_form.argtypes = [ci, ci, ci, ci, ci, ci, ci, ci, ci, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_dbg_gemm_form.restype = ctypes.c_int
    L.stn_dbg_attn_form.argtypes = [ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_dbg_attn_form.restype = ctypes.c_int
    L.stn_dbg_ffn_form.argtypes = [ci, ci, ci, ci, ctypes.c_int64, ctypes.c_int64, ci, ci, ci, ci, ctypes.c_int64, ctypes.c_int64, ci,
                                   ctypes.c_char_p, ctypes.c_size_t]
    L.stn_dbg_ffn_form.restype = ctypes.c_int
    L.stn_launch_log.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_launch_log.restype = ctypes.c_int64
    L.stn_profile_enable.argtypes = [vp, ci]
    L.stn_profile_reset.argtypes = [vp]
    L.stn_profile_count.argtypes = [vp]
    L.stn_profile_get.argtypes = [vp, ci, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_double)]
    L.stn_op_gemm.argtypes = [vp, ci, ci, ci, ci, _f32p, _f32p, vp, ci, _f32p]
    L.stn_op_gemm_ex.argtypes = [vp, ci, ci, ci, ci, _f32p, _f32p, ci, ci, ci, ci, vp, vp, vp, ci, vp, vp, ci, ci, ci, _f32p,
                                 ctypes.c_int64, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_op_gemm_bench.argtypes = [vp, ci, ci, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_double)]
    L.stn_op_gemm_phases.argtypes = [vp, ci, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_double)]
    L.stn_op_dwconv_ln.argtypes = [vp, ci, ci, ci, ci, ci, ci, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p]
    L.stn_op_dwconv_ln_ragged.argtypes = [vp, ci, ci, ci, ci, ci, ci, _f32p, _f32p, _f32p, _f32p, _f32p, _i32p, _f32p]
    L.stn_op_attention.argtypes = [vp, ci, ci, ci, ci, ci, ci, _f32p, _f32p, _f32p, vp, vp, ci, _f32p]
    L.stn_op_gemm_rows.argtypes = [vp, ci, ci, ci, ci, _f32p, _f32p, vp, ci, _i32p, _i32p, ci, _f32p, ctypes.c_int64, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_op_dwconv_ln_ex.argtypes = [vp, ci, ci, ci, ci, ci, ci, _f32p, ctypes.c_int64, vp, vp, _f32p, _f32p, vp, ci, ci, _f32p, ctypes.c_int64,
                                      ctypes.c_char_p, ctypes.c_size_t]
    L.stn_op_dwconv_ln_tail.argtypes = [vp, ci, ci, ci, ci, ci, ci, _f32p, ctypes.c_int64, _f32p, _f32p, _f32p, _f32p, _i32p, _f32p, ci, ci, _f32p,
                                        ctypes.c_int64, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_dbg_resample_form.argtypes = [ci, ci, ctypes.c_int64, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_dbg_resample_form.restype = ctypes.c_int
    L.stn_dbg_dwconv_ln_form.argtypes = [ci, ci, ci, ci, ci, ci, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_dbg_dwconv_ln_form.restype = ctypes.c_int
    L.stn_dbg_len_tables.argtypes = [ci, _i32p, ci, ci, ci, ci, ci, ci, _i32p, ctypes.c_void_p, ctypes.c_int64]
    L.stn_dbg_len_tables.restype = ctypes.c_int64
    L.stn_op_fold_ln.argtypes = [vp, ci, ci, ci, ci, _f32p, _f32p, _f32p, vp, vp, ci, _f32p, _f32p, _f32p, _f32p]
    L.stn_op_layout.argtypes = [vp, ci, ci, _i32p, ci, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, ci,
                                vp, ctypes.c_int64, vp, ctypes.c_int64, vp, ctypes.c_int64]
    L.stn_op_attention_ex.argtypes = [vp, ci, ci, ci, ci, ci, ci, _f32p, ctypes.c_int64, ci, ci, _f32p, ctypes.c_int64, ci, ci, ci,
                                      _f32p, ctypes.c_int64, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_op_xattn_hs.argtypes = [vp, ci, ci, _f32p, _f32p, vp, _f32p, _f32p, ctypes.c_int64, ci, ci, ci, ci, ci, _i32p, vp, vp, ci, ci,
                                  ctypes.c_int64, _f32p, ctypes.c_int64, vp, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_op_randn.argtypes = [vp, cu64, ci, ci, ci, vp, vp, _f32p]
    L.stn_op_ffn.argtypes = [vp, ci, ci, ci, _f32p, _f32p, _f32p, _f32p, vp, vp, vp, vp, ci, _f32p, ci]
    L.stn_op_ffn_ex.argtypes = [vp, ci, ci, ci, ci, _f32p, ci, ctypes.c_int64, _f32p, _f32p, _f32p, vp, vp, vp, ci, vp, vp, ci, ci, ci, ci, _f32p, ci,
                                ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_op_ffn_bench.argtypes = [vp, ci, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_double)]
    L.stn_set_fused_ffn.argtypes = [vp, ci]
    L.stn_set_fused_ffn_min_rows.argtypes = [vp, ctypes.c_int64, ctypes.c_int64]
    L.stn_op_fold_dwconv_ln.argtypes = [vp, ci, ci, ci, ci, ci, _i32p, _f32p, _f32p, vp, vp, vp, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p]
    L.stn_op_fold_dwconv_ln_ex.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, ci, _i32p, _f32p, ctypes.c_int64, _f32p, ctypes.c_int64, ctypes.c_int64, vp, vp,
                                           vp, ci, _f32p, _f32p, _f32p, _f32p, _f32p, ctypes.c_int64, _f32p, ctypes.c_int64, ctypes.c_char_p,
                                           ctypes.c_size_t]
    L.stn_dbg_fold_dwconv_ln_form.argtypes = [ci, ci, ci, ci, ci, ci, ci, ci, ci, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_dbg_fold_dwconv_ln_form.restype = ctypes.c_int
    L.stn_op_block_bench.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_double)]
    # include/stn_group.h: several devices in one process
    L.stn_group_create.argtypes = [ci, vp, ci, ctypes.POINTER(vp)]
    L.stn_group_destroy.argtypes = [vp]
    L.stn_group_last_error.restype = ctypes.c_char_p
    L.stn_group_last_error.argtypes = [vp]
    L.stn_group_size.argtypes = [vp]
    L.stn_group_uses_rccl.argtypes = [vp]
    L.stn_group_handle.restype = vp
    L.stn_group_handle.argtypes = [vp, ci]
    L.stn_group_load_synthetic.argtypes = [vp, ctypes.POINTER(StnArch), cu64]
    L.stn_group_load_dir.argtypes = [vp, ctypes.c_char_p]
    L.stn_group_deal.argtypes = [ci, _i32p, ci, _i32p, _i32p]
    L.stn_group_synthesize.argtypes = [vp, ci, ci, _i64p, _f32p, _f32p, _f32p, ci, cf, vp, cu64, ctypes.POINTER(ctypes.c_int64)]
    L.stn_group_fetch_pcm16.argtypes = [vp, vp, ctypes.c_size_t, vp]
    L.stn_set_output_rate.argtypes = [vp, ci]
    L.stn_get_output_rate.argtypes = [vp]
    L.stn_resample_filter.argtypes = [ci, ci, vp, ctypes.c_size_t, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.stn_resample_error.argtypes = [ci, ci]
    L.stn_resample_error.restype = ctypes.c_char_p
    L.stn_op_resample.argtypes = [vp, ci, ci, ci, ci, _f32p, vp, vp]
    L.stn_group_set_output_rate.argtypes = [vp, ci]
    _f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    L.stn_set_loudness.argtypes = [vp, ci, cf, cf]
    L.stn_get_loudness.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(cf), ctypes.POINTER(cf)]
    L.stn_batch_loudness.argtypes = [vp, vp, vp, vp]
    L.stn_op_loudness.argtypes = [vp, ci, ci, ci, _f32p, vp, vp, vp]
    L.stn_kweighting_filter.argtypes = [ci, _f64p, _f64p, _f64p, _f64p]
    L.stn_op_loudness_ex.argtypes = [vp, ci, ci, ci, _f32p, vp, ci, cf, cf, ci, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_loudness_table.argtypes = [ci, vp, vp, ctypes.c_size_t, ctypes.POINTER(ci)]
    L.stn_group_set_loudness.argtypes = [vp, ci, cf, cf]
    L.stn_batch_loudness_range.argtypes = [vp, vp, vp, vp, vp]
    L.stn_op_loudness_range.argtypes = [vp, ci, ci, ci, _f32p, vp, vp, vp, vp, vp]
    L.stn_batch_f0_frames.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_int64)]
    L.stn_batch_f0.argtypes = [vp, vp, ctypes.c_int64, vp, vp, vp]
    L.stn_op_f0.argtypes = [vp, ci, ci, ci, _f32p, vp, vp, ctypes.c_int64, vp, vp, vp]
    L.stn_set_silence_trim.argtypes = [vp, ci, cf, cf, cf]
    L.stn_get_silence_trim.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(cf), ctypes.POINTER(cf), ctypes.POINTER(cf)]
    L.stn_batch_silence_edges.argtypes = [vp, vp, vp]
    L.stn_op_silence_edges.argtypes = [vp, ci, ci, ci, _f32p, vp, cf, cf, vp, vp]
    L.stn_op_silence_trim.argtypes = [vp, ci, ci, ci, _f32p, vp, cf, cf, cf, vp, ci, vp, vp, vp]
    L.stn_silence_fade_window.argtypes = [ci, cf, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    L.stn_set_pause_limit.argtypes = [vp, ci, cf]
    L.stn_get_pause_limit.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(cf)]
    L.stn_batch_pauses.argtypes = [vp, vp, vp, vp, ci]
    L.stn_op_pause_trim.argtypes = [vp, ci, ci, ci, _f32p, vp, cf, cf, cf, cf, vp, ci, vp, vp, vp, vp, vp, vp, ci]
    L.stn_op_silence_edges_ex.argtypes = [vp, ci, ci, ci, _f32p, vp, cf, cf, cf, cf, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ctypes.c_char_p,
                                          ctypes.c_size_t]
    L.stn_group_set_pause_limit.argtypes = [vp, ci, cf]
    L.stn_set_limiter.argtypes = [vp, ci, cf]
    L.stn_get_limiter.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(cf)]
    L.stn_batch_limiter.argtypes = [vp, vp, vp]
    L.stn_op_limiter.argtypes = [vp, ci, ci, ci, _f32p, vp, vp, cf, cf, vp, vp, vp, vp]
    L.stn_limiter_window.argtypes = [ci, cf, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    L.stn_group_set_limiter.argtypes = [vp, ci, cf]
    L.stn_set_peak_mode.argtypes = [vp, ci]
    L.stn_get_peak_mode.argtypes = [vp]
    L.stn_group_set_peak_mode.argtypes = [vp, ci]
    L.stn_true_peak_filter.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.stn_batch_true_peak.argtypes = [vp, vp, vp, vp]
    L.stn_op_true_peak.argtypes = [vp, ci, ci, ci, _f32p, vp, vp, ci, vp, vp, vp, ctypes.c_char_p, ctypes.c_size_t]
    L.stn_op_limiter_ex.argtypes = [vp, ci, ci, ci, _f32p, vp, vp, cf, cf, vp, vp, vp, vp, ci, vp, vp]
    fp = ctypes.POINTER(StnFilter)
    L.stn_set_filters.argtypes = [vp, ci, fp]
    L.stn_get_filters.argtypes = [vp, ctypes.POINTER(ci), fp]
    L.stn_group_set_filters.argtypes = [vp, ci, fp]
    L.stn_op_filter.argtypes = [vp, ci, ci, ci, _f32p, ci, fp, _f32p]
    L.stn_op_filter_ex.argtypes = [vp, ci, ci, ci, _f32p, ci, fp, ci, _f32p, vp, vp, ctypes.POINTER(ci), ctypes.c_char_p, ctypes.c_size_t]
    L.stn_filter_error.argtypes = [ci, fp, ci]
    L.stn_filter_error.restype = ctypes.c_char_p
    L.stn_filter_coefs.argtypes = [fp, ci, _f64p, _f32p]
    L.stn_filter_response.argtypes = [ci, fp, ci, ci, _f64p, _f64p]
    L.stn_dbg_filter_geometry.argtypes = [ctypes.POINTER(ci)] * 4
    cpp = ctypes.POINTER(StnCompressor)
    L.stn_set_compressor.argtypes = [vp, ci, cpp]
    L.stn_get_compressor.argtypes = [vp, ctypes.POINTER(ci), cpp]
    L.stn_group_set_compressor.argtypes = [vp, ci, cpp]
    L.stn_batch_compressor.argtypes = [vp, vp]
    L.stn_op_compressor.argtypes = [vp, ci, ci, ci, _f32p, cpp, _f32p]
    L.stn_op_compressor_ex.argtypes = [vp, ci, ci, ci, _f32p, cpp, ci, ci, _f32p, vp, vp, vp, vp, vp, ctypes.POINTER(ci), ctypes.c_char_p, ctypes.c_size_t]
    L.stn_compressor_error.argtypes = [cpp, ci]
    L.stn_compressor_error.restype = ctypes.c_char_p
    L.stn_compressor_coefs.argtypes = [cpp, ci, _f64p, _f32p]
    L.stn_compressor_curve.argtypes = [cpp, ci, _f64p, _f64p]
    xpp = ctypes.POINTER(StnExpander)
    L.stn_set_expander.argtypes = [vp, ci, xpp]
    L.stn_get_expander.argtypes = [vp, ctypes.POINTER(ci), xpp]
    L.stn_group_set_expander.argtypes = [vp, ci, xpp]
    L.stn_batch_expander.argtypes = [vp, vp, vp]
    L.stn_op_expander.argtypes = [vp, ci, ci, ci, _f32p, xpp, _f32p]
    L.stn_op_expander_ex.argtypes = [vp, ci, ci, ci, _f32p, xpp, ci, ci, _f32p, vp, vp, vp, vp, vp, ctypes.POINTER(ci), ctypes.c_char_p, ctypes.c_size_t]
    L.stn_expander_error.argtypes = [xpp, ci]
    L.stn_expander_error.restype = ctypes.c_char_p
    L.stn_expander_coefs.argtypes = [xpp, ci, _f64p, _f32p, ctypes.POINTER(ctypes.c_int64)]
    L.stn_expander_curve.argtypes = [xpp, ci, _f64p, _f64p]
    dsp = ctypes.POINTER(StnDeesser)
    L.stn_set_deesser.argtypes = [vp, ci, dsp]
    L.stn_get_deesser.argtypes = [vp, ctypes.POINTER(ci), dsp]
    L.stn_group_set_deesser.argtypes = [vp, ci, dsp]
    L.stn_batch_deesser.argtypes = [vp, vp]
    L.stn_op_deesser.argtypes = [vp, ci, ci, ci, _f32p, dsp, _f32p]
    L.stn_op_deesser_ex.argtypes = [vp, ci, ci, ci, _f32p, dsp, ci, ci, _f32p] + [vp] * 8 + [ctypes.POINTER(ci), ctypes.c_char_p, ctypes.c_size_t]
    L.stn_deesser_error.argtypes = [dsp, ci]
    L.stn_deesser_error.restype = ctypes.c_char_p
    L.stn_deesser_band.argtypes = [dsp, ci, _f64p, _f32p]
    L.stn_deesser_coefs.argtypes = [dsp, ci, _f64p, _f32p]
    L.stn_dbg_batch_set_wav.argtypes = [vp, _f32p]
    L.stn_dbg_span_uploads.argtypes = [vp]
    L.stn_dbg_span_uploads.restype = ctypes.c_int64
    L.stn_encoding_bytes.argtypes = [ci]
    L.stn_batch_fetch_encoded.argtypes = [vp, ci, vp, ctypes.c_size_t, vp]
    L.stn_batch_copy_encoded_device.argtypes = [vp, ci, vp, ctypes.c_int64]
    L.stn_batch_fetch_encoded_begin.argtypes = [vp, ci, ci]
    L.stn_batch_fetch_encoded_end.argtypes = [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), vp]
    L.stn_op_encode.argtypes = [vp, ci, ci, ci, _f32p, vp]
    L.stn_set_dither.argtypes = [vp, ci, cu64]
    L.stn_get_dither.argtypes = [vp, ctypes.POINTER(cu64)]
    L.stn_group_set_dither.argtypes = [vp, ci, cu64]
    L.stn_op_encode_ex.argtypes = [vp, ci, ci, ci, _f32p, ci, vp, vp, ci, cu64, ctypes.c_int64, vp]
    L.stn_set_pitch.argtypes = [vp, cf]
    L.stn_get_pitch.argtypes = [vp, ctypes.POINTER(cf), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.stn_group_set_pitch.argtypes = [vp, cf]
    L.stn_op_time_stretch.argtypes = [vp, ci, ci, ci, _f32p, vp, ci, ci, vp, vp, vp]
    L.stn_op_pitch.argtypes = [vp, ci, ci, ci, _f32p, vp, cf, vp]
    L.stn_set_pitch_mode.argtypes = [vp, ci]
    L.stn_get_pitch_mode.argtypes = [vp]
    L.stn_group_set_pitch_mode.argtypes = [vp, ci]
    L.stn_op_formant.argtypes = [vp, ci, ci, ci, _f32p, _f32p, vp, vp]
    L.stn_op_formant_ex.argtypes = [vp, ci, ci, ci, _f32p, _f32p, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(ci)]
    L.stn_op_pitch_ex.argtypes = [vp, ci, ci, ci, _f32p, vp, cf, ci, vp]
    jp =ctypes.POINTER(StnJoin)
    L.stn_batch_join_dims.argtypes = [vp, jp, ctypes.POINTER(ctypes.c_int64), vp, vp]
    L.stn_batch_fetch_joined.argtypes = [vp, jp, ci, vp, ctypes.c_size_t, vp, vp]
    L.stn_batch_copy_joined_device.argtypes = [vp, jp, ci, vp, ctypes.c_int64]
    L.stn_batch_fetch_joined_begin.argtypes = [vp, ci, jp, ci]
    L.stn_batch_join_loudness.argtypes = [vp, jp, vp, vp, vp]
    L.stn_batch_join_loudness_range.argtypes = [vp, jp, vp, vp, vp, vp]
    L.stn_op_join.argtypes = [vp, ci, ci, ci, _f32p, _i64p, jp, ci, ci, cf, cf, vp, vp, vp, vp]
    L.stn_group_set_encoding.argtypes = [vp, ci]
    L.stn_group_fetch_encoded.argtypes = [vp, vp, ctypes.c_size_t, vp]
    L.stn_group_last_shards.argtypes = [vp, _i32p, np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")]
    _LIB = L
    return L


def group_deal(lengths, n_ranks):
    """include/stn_group.h's deal (host only): (rank_of, row_of) for utterances of these token counts."""
    lengths = _c(lengths, np.int32)
    rank_of, row_of = np.empty(len(lengths), np.int32), np.empty(len(lengths), np.int32)
    rc = load().stn_group_deal(len(lengths), lengths, int(n_ranks), rank_of, row_of)
    if rc < 0:
        raise StnError(rc, "stn_group_deal: invalid arguments")
    return rank_of, row_of


class Group:
    """n devices in one process (include/stn_group.h): one engine per device, utterances dealt by length, 16-bit PCM (or the encoding
    set_encoding chose) gathered into the first device (RCCL when the devices are distinct; the same ordinal repeated is a rehearsal on
    one GPU)."""

    def __init__(self, devices, dtype="bf16"):
        self._lib = load()
        self._g = ctypes.c_void_p()
        devices = list(range(devices)) if isinstance(devices, int) else list(devices)
        arr = (ctypes.c_int * len(devices))(*devices)
        rc = self._lib.stn_group_create(len(devices), arr, _DTYPES[dtype], ctypes.byref(self._g))
        if rc < 0:
            self._g = None
            raise StnError(rc, self._lib.stn_group_last_error(None).decode())
        self.n = len(devices)
        self._enc = ENC_PCM16

    def close(self):
        if getattr(self, "_g", None):
            self._lib.stn_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            raise StnError(rc, self._lib.stn_group_last_error(self._g).decode())

    @property
    def uses_rccl(self):
        return bool(self._lib.stn_group_uses_rccl(self._g))

    def load_synthetic(self, arch: StnArch, seed: int = 7):
        self._ck(self._lib.stn_group_load_synthetic(self._g, ctypes.byref(arch), seed))

    def load_dir(self, onnx_dir: str):
        self._ck(self._lib.stn_group_load_dir(self._g, onnx_dir.encode()))

    def synthesize(self, text_ids, text_mask, style_ttl, style_dp, total_step=5, speed=1.05, duration_override=None, noise_seed=1234):
        """-> (samples [B, W] in caller order in the gather's encoding: int16 PCM by default (encoded_empty's dtypes), duration [B])"""
        B, Lt = text_ids.shape
        _d, dptr = _opt(duration_override, np.float32)
        W = ctypes.c_int64()
        enc = self._enc
        self._ck(self._lib.stn_group_synthesize(self._g, B, Lt, _c(text_ids, np.int64), _c(text_mask, np.float32), _c(style_ttl, np.float32),
                                                _c(style_dp, np.float32), total_step, speed, dptr, noise_seed, ctypes.byref(W)))
        out, dur = encoded_empty(enc, B, W.value), np.empty(B, np.float32)
        self._ck(self._lib.stn_group_fetch_encoded(self._g, out.ctypes.data, out.nbytes, dur.ctypes.data))
        return out, dur

    def set_encoding(self, enc):
        """Sample encoding of the next synthesize's gather (a name or ENC_*; "pcm16" is the default)."""
        e = encoding_id(enc)
        self._ck(self._lib.stn_group_set_encoding(self._g, e))
        self._enc = e

    def set_output_rate(self, hz):
        """Output rate of every rank (0 or None = the model's rate): the gathered PCM is then at that rate."""
        self._ck(self._lib.stn_group_set_output_rate(self._g, int(hz or 0)))

    def set_loudness(self, target_lufs=None, ceiling_dbfs=-1.0):
        """Loudness normalization of every rank (Engine.set_loudness): the gathered PCM is then normalized row by row."""
        on, t = _loudness_args(target_lufs)
        self._ck(self._lib.stn_group_set_loudness(self._g, on, t, float(ceiling_dbfs)))

    def set_pause_limit(self, max_pause=None):
        """The group does not trim, so it refuses the pause limit (StnError with the reason); None or False is accepted."""
        on, ms = pause_limit_args(max_pause)
        self._ck(self._lib.stn_group_set_pause_limit(self._g, on, ms))

    def set_limiter(self, lookahead_ms=None):
        """Look-ahead peak limiter of every rank (Engine.set_limiter): the gathered PCM is then limited row by row."""
        on, ms = limiter_args(lookahead_ms)
        self._ck(self._lib.stn_group_set_limiter(self._g, on, ms))

    def set_peak_mode(self, mode="sample"):
        """Peak mode of every rank (Engine.set_peak_mode): "sample" or "true"."""
        self._ck(self._lib.stn_group_set_peak_mode(self._g, peak_mode_id(mode)))

    def set_dither(self, dither=None, seed=None):
        """Dither of every rank's 16- and 24-bit PCM store (Engine.set_dither): rows are keyed by the caller's utterance index."""
        mode, seed = dither_args(dither, seed) or ("off", 0)
        self._ck(self._lib.stn_group_set_dither(self._g, DITHER_MODES[mode], seed))

    def set_pitch(self, semitones=None):
        """Pitch of every rank (Engine.set_pitch): rows are shifted on their own, so the gathered rows are the single engine's."""
        self._ck(self._lib.stn_group_set_pitch(self._g, pitch_args(semitones)))

    def set_pitch_mode(self, mode="resample"):
        """Pitch mode of every rank (Engine.set_pitch_mode): "resample" or "formant"."""
        self._ck(self._lib.stn_group_set_pitch_mode(self._g, pitch_mode_id(mode)))

    def set_filters(self, filters=None):
        """Filter chain of every rank (Engine.set_filters): the gathered rows are then the single engine's filtered rows."""
        n, arr = _filter_array(filters)
        self._ck(self._lib.stn_group_set_filters(self._g, n, arr))

    def set_compressor(self, compressor=None):
        """Compressor of every rank (Engine.set_compressor): the gathered rows are then the single engine's compressed rows."""
        _set_dynamics(self, self._lib.stn_group_set_compressor, self._g, _COMPRESSOR, compressor)

    def set_expander(self, expander=None):
        """Expander of every rank (Engine.set_expander): the gathered rows are then the single engine's expanded rows."""
        _set_dynamics(self, self._lib.stn_group_set_expander, self._g, _EXPANDER, expander)

    def set_deesser(self, deesser=None):
        """De-esser of every rank (Engine.set_deesser): the gathered rows are then the single engine's de-essed rows."""
        _set_dynamics(self, self._lib.stn_group_set_deesser, self._g, _DEESSER, deesser)

    def last_shards(self):
        rows, samples = np.zeros(self.n, np.int32), np.zeros(self.n, np.int64)
        self._ck(self._lib.stn_group_last_shards(self._g, rows, samples))
        return rows, samples


SUPPORTED_OUTPUT_RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)


def resample_filter(in_hz, out_hz):
    """The output-rate resampler's filter for in_hz -> out_hz (host only): taps [P, T] float32; tap j of phase p multiplies input
    floor(n*Q/P) - (T/2 - 1) + j of output n, whose phase is (n*Q) mod P.  Raises StnError for a refused pair."""
    L = load()
    P, T = ctypes.c_int(), ctypes.c_int()
    rc = L.stn_resample_filter(int(in_hz), int(out_hz), None, 0, ctypes.byref(P), ctypes.byref(T))
    if rc < 0:
        raise StnError(rc, L.stn_resample_error(int(in_hz), int(out_hz)).decode())
    taps = np.empty((P.value, T.value), np.float32)
    rc = L.stn_resample_filter(int(in_hz), int(out_hz), taps.ctypes.data, taps.size, ctypes.byref(P), ctypes.byref(T))
    if rc < 0:
        raise StnError(rc, "stn_resample_filter failed")
    return taps


def kweighting_filter(hz):
    """BS.1770-4 K-weighting at hz (host only): (shelf_b, shelf_a, hp_b, hp_a), float64 [3] each, a[0] = 1.  StnError outside
    [8000, 192000] Hz."""
    out = [np.zeros(3, np.float64) for _ in range(4)]
    rc = load().stn_kweighting_filter(int(hz), *out)
    if rc < 0:
        raise StnError(rc, f"stn_kweighting_filter: {hz} Hz is outside [8000, 192000] Hz")
    return tuple(out)


def loudness_table(hz):
    """What the loudness kernels are given at hz (host only): (coef float32 [10]: shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2;
    mpow float32 [1024, 4, 4]: entry i = M^(i+1), M the zero-input state transition over one 32-sample chunk, the scan's double table
    rounded to fp32; hop: samples per 100 ms).
    StnError outside [8000, 192000] Hz."""
    coef, mpow, hop = np.zeros(10, np.float32), np.zeros((1024, 4, 4), np.float32), ctypes.c_int()
    rc = load().stn_loudness_table(int(hz), coef.ctypes.data, mpow.ctypes.data, mpow.size, ctypes.byref(hop))
    if rc < 0:
        raise StnError(rc, f"stn_loudness_table: {hz} Hz is outside [8000, 192000] Hz")
    return coef, mpow, hop.value


TRIM_KEEP_MS, TRIM_FADE_MS = 20.0, 5.0


def silence_trim_args(trim_silence):
    """A trim_silence argument -> (on, top_db, keep_ms, fade_ms) for stn_set_silence_trim: None = off, a number = top_db with 20 ms kept
    and a 5 ms fade, or (top_db, keep_ms, fade_ms).  ValueError, with the ABI's ranges, for anything else."""
    if trim_silence is None:
        return 0, 40.0, TRIM_KEEP_MS, TRIM_FADE_MS
    if isinstance(trim_silence, bool):
        raise ValueError("trim_silence: None, top_db or (top_db, keep_ms, fade_ms), not a bool")
    try:
        t = tuple(float(v) for v in trim_silence) if isinstance(trim_silence, (tuple, list)) else (float(trim_silence), TRIM_KEEP_MS, TRIM_FADE_MS)
    except (TypeError, ValueError):
        raise ValueError(f"trim_silence: None, top_db or (top_db, keep_ms, fade_ms), not {trim_silence!r}") from None
    if len(t) != 3:
        raise ValueError(f"trim_silence: None, top_db or (top_db, keep_ms, fade_ms), not {trim_silence!r}")
    db, keep, fade = t
    if not 1.0 <= db <= 120.0:
        raise ValueError(f"trim_silence top_db {db} dB: must be in [1, 120]")
    if not 0.0 <= keep <= 1000.0:
        raise ValueError(f"trim_silence keep {keep} ms: must be in [0, 1000]")
    if not 0.0 <= fade <= 50.0:
        raise ValueError(f"trim_silence fade {fade} ms: must be in [0, 50]")
    return 1, db, keep, fade


def silence_fade_window(hz, fade_ms):
    """The fade of a cut edge at hz (host only): float32 [Fd], Fd = int(fade_ms * hz / 1000 + 0.5), w[j] = 0.5 - 0.5 cos(pi (j + 0.5) / Fd).
    StnError when fade_ms is outside [0, 50]."""
    L = load()
    n = ctypes.c_int64()
    if L.stn_silence_fade_window(int(hz), float(fade_ms), None, 0, ctypes.byref(n)) < 0:
        raise StnError(-1, f"stn_silence_fade_window: fade {fade_ms} ms at {hz} Hz refused (fade_ms in [0, 50], hz >= 1)")
    w = np.empty(n.value, np.float32)
    if L.stn_silence_fade_window(int(hz), float(fade_ms), w.ctypes.data, w.size, ctypes.byref(n)) < 0:
        raise StnError(-1, "stn_silence_fade_window failed")
    return w


MAX_PAUSE_MS = 300.0  # what stn_get_pause_limit reports while the limit was never set
PAUSE_MAX_CUTS = 255


def pause_limit_args(max_pause):
    """A max_pause argument -> (on, max_pause_ms) for stn_set_pause_limit: None or False = off, a number = the longest pause left inside
    an utterance in milliseconds.  ValueError, with the ABI's range, for anything else."""
    if max_pause is None or max_pause is False:
        return 0, MAX_PAUSE_MS
    if isinstance(max_pause, bool):
        raise ValueError("max_pause: None, False or milliseconds in [20, 5000], not True")
    try:
        ms = float(max_pause)
    except (TypeError, ValueError):
        raise ValueError(f"max_pause: None, False or milliseconds in [20, 5000], not {max_pause!r}") from None
    if not 20.0 <= ms <= 5000.0:
        raise ValueError(f"max_pause {ms} ms: must be in [20, 5000]")
    return 1, ms


def pause_plan(level, n, hz, top_db=40.0, keep_ms=None, max_pause_ms=MAX_PAUSE_MS, cap_pairs=PAUSE_MAX_CUTS):
    """stn_pause_plan (host only, no device): one row's frame levels (float64 [K], K = ceil(n / F)) -> (start, end, cuts [n_cuts, 2]
    int64 as (lo, hi), n_cuts); cuts holds the first min(n_cuts, cap_pairs) pairs.  A refused argument raises StnError with the reason."""
    L = load()
    L.stn_pause_plan.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.stn_pause_plan_error.restype = ctypes.c_char_p
    lv = np.ascontiguousarray(level, np.float64)
    start, end, nc = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    cuts = np.zeros((max(int(cap_pairs), 0), 2), np.int64)
    rc = L.stn_pause_plan(int(hz), int(n), lv.ctypes.data, lv.size, float(top_db), float(TRIM_KEEP_MS if keep_ms is None else keep_ms),
                          float(max_pause_ms), ctypes.addressof(start), ctypes.addressof(end), cuts.ctypes.data if cuts.size else None,
                          cuts.shape[0], ctypes.addressof(nc))
    if rc != 0:
        raise StnError(rc, L.stn_pause_plan_error().decode())
    return start.value, end.value, cuts[:min(nc.value, cuts.shape[0])], nc.value


def loudness_range_rule(seg, hop):
    """stn_loudness_range_rule (host only, no device): one row's 100 ms segment sums (float64 [nseg], sums of K-weighted y^2 over hop
    samples each) -> (m_max, s_max, lra, n_st): maximum momentary and maximum short-term loudness (LUFS, -inf without a block / a
    window), loudness range (LU, EBU Tech 3342) and the number of 3 s windows behind both gates.  include/stn.h "loudness range"."""
    L = load()
    L.stn_loudness_range_rule.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]
    sg = np.ascontiguousarray(seg, np.float64).reshape(-1)
    m, s, r, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int32()
    rc = L.stn_loudness_range_rule(int(hop), sg.size, sg.ctypes.data if sg.size else None, ctypes.addressof(m), ctypes.addressof(s),
                                   ctypes.addressof(r), ctypes.addressof(k))
    if rc != 0:
        raise StnError(rc, f"stn_loudness_range_rule: hop {hop} must be at least 1")
    return m.value, s.value, r.value, k.value


class StnF0Params(ctypes.Structure):
    _fields_ = [("fmin_hz", ctypes.c_float), ("fmax_hz", ctypes.c_float), ("threshold", ctypes.c_float), ("gate_db", ctypes.c_float)]


F0_STATS = np.dtype([("frames", np.int32), ("voiced", np.int32), ("median_hz", np.float32), ("mean_hz", np.float32), ("min_hz", np.float32),
                     ("max_hz", np.float32)])
F0_DEFAULTS = {"fmin_hz": 60.0, "fmax_hz": 500.0, "threshold": 0.15, "gate_db": -60.0}


def _f0_lib():
    L = load()
    ci, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    L.stn_f0_error.argtypes = [ci, vp]
    L.stn_f0_error.restype = ctypes.c_char_p
    L.stn_f0_plan.argtypes = [ci, i64, vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(i64)]
    L.stn_f0_rule.argtypes = [ci, i64, vp, vp, i64, vp, vp, ctypes.POINTER(i64)]
    L.stn_f0_rule_lags.argtypes = [ci, i64, vp, vp, i64, vp, ctypes.POINTER(i64)]
    L.stn_f0_stats_rule.argtypes = [vp, i64, vp]
    L.stn_f0_group.restype = ci
    L.stn_f0_max_frames.restype = i64
    return L


def f0_params(params=None):
    """A pitch-report parameter argument -> StnF0Params: None is the defaults (60 Hz, 500 Hz, 0.15, -60 dB), a dict overrides some of
    fmin_hz, fmax_hz, threshold, gate_db.  The limits are the ABI's (f0_error)."""
    if isinstance(params, StnF0Params):
        return params
    p = dict(F0_DEFAULTS)
    if params:
        unknown = set(params) - set(p)
        if unknown:
            raise ValueError(f"f0 parameters: unknown field(s) {sorted(unknown)}")
        p.update(params)
    return StnF0Params(*(float(p[k]) for k in ("fmin_hz", "fmax_hz", "threshold", "gate_db")))


def f0_error(hz, params=None):
    """Why the pitch report refuses (hz, params) (host only; stn_f0_error), or "" for what it takes."""
    p = f0_params(params)
    return _f0_lib().stn_f0_error(int(hz), ctypes.addressof(p)).decode()


def _f0_refuse(L, hz, p, what):
    why = L.stn_f0_error(int(hz), ctypes.addressof(p)).decode()
    raise StnError(-1, why or what)


def f0_plan(hz, n, params=None):
    """stn_f0_plan (host only): the pitch report's geometry of a span of n samples at hz -> dict k, hop, tau_min, tau_max, frames."""
    L, p = _f0_lib(), f0_params(params)
    k, hop, lo, hi, fr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    if L.stn_f0_plan(int(hz), int(n), ctypes.addressof(p), k, hop, lo, hi, fr) != 0:
        _f0_refuse(L, hz, p, f"stn_f0_plan: n = {n} must not be negative")
    return {"k": k.value, "hop": hop.value, "tau_min": lo.value, "tau_max": hi.value, "frames": fr.value}


def f0_rule(x, hz, params=None, lags=False):
    """stn_f0_rule (host only): the contract of include/stn.h "f0" in double on one row x (fp32) at hz -> (f0 [frames], ap [frames])
    float64; with lags=True also tau^ [frames] int32 (0 for an unvoiced frame)."""
    L, p = _f0_lib(), f0_params(params)
    xr = np.ascontiguousarray(x, np.float32).reshape(-1)
    F = f0_plan(hz, xr.size, p)["frames"]
    f0, ap, lag, fr = np.empty(F, np.float64), np.empty(F, np.float64), np.empty(F, np.int32), ctypes.c_int64()
    xp = xr.ctypes.data if xr.size else None
    if L.stn_f0_rule(int(hz), xr.size, xp, ctypes.addressof(p), F, f0.ctypes.data, ap.ctypes.data, fr) != 0 or fr.value != F:
        _f0_refuse(L, hz, p, "stn_f0_rule failed")
    if not lags:
        return f0, ap
    if L.stn_f0_rule_lags(int(hz), xr.size, xp, ctypes.addressof(p), F, lag.ctypes.data, fr) != 0:
        _f0_refuse(L, hz, p, "stn_f0_rule_lags failed")
    return f0, ap, lag


def f0_stats_rule(f0):
    """stn_f0_stats_rule (host only): the statistics of one fp32 track (0 = unvoiced) -> a numpy record of F0_STATS."""
    L = _f0_lib()
    t = np.ascontiguousarray(f0, np.float32).reshape(-1)
    out = np.zeros(1, F0_STATS)
    if L.stn_f0_stats_rule(t.ctypes.data if t.size else None, t.size, out.ctypes.data) != 0:
        raise StnError(-1, "stn_f0_stats_rule: bad argument")
    return out[0]


def f0_group():
    """frames a workgroup of the track kernel owns (stn_f0_group) and the most frames a row may hold (stn_f0_max_frames)"""
    L = _f0_lib()
    return L.stn_f0_group(), L.stn_f0_max_frames()


LIMITER_MS = 5.0


def limiter_args(lookahead_ms):
    """A limiter argument -> (on, lookahead_ms) for stn_set_limiter: None or False = off, True = 5 ms, a number = the look-ahead in
    milliseconds.  ValueError, with the ABI's range, for anything else."""
    if lookahead_ms is None or lookahead_ms is False:
        return 0, LIMITER_MS
    if lookahead_ms is True:
        return 1, LIMITER_MS
    try:
        ms = float(lookahead_ms)
    except (TypeError, ValueError):
        raise ValueError(f"limiter: None, True or a look-ahead in milliseconds, not {lookahead_ms!r}") from None
    if not 0.5 <= ms <= 10.0:
        raise ValueError(f"limiter look-ahead {ms} ms: must be in [0.5, 10]")
    return 1, ms


PEAK_SAMPLE, PEAK_TRUE = 0, 1
PEAK_MODES = {"sample": PEAK_SAMPLE, "true": PEAK_TRUE}


def peak_mode_id(mode):
    """A peak-mode argument -> STN_PEAK_SAMPLE / STN_PEAK_TRUE: "sample" or "true" (None: "sample"); anything else is a ValueError."""
    if mode is None:
        return PEAK_SAMPLE
    if isinstance(mode, str) and mode in PEAK_MODES:
        return PEAK_MODES[mode]
    raise ValueError(f"peak_mode: 'sample' or 'true', not {mode!r}")


# dither of the 16- and 24-bit PCM stores (STN_DITHER_*, include/stn.h "dither")
DITHER_OFF, DITHER_ROUND, DITHER_TPDF, DITHER_TPDF_HP = 0, 1, 2, 3
DITHER_MODES = {"off": DITHER_OFF, "round": DITHER_ROUND, "tpdf": DITHER_TPDF, "tpdf-hp": DITHER_TPDF_HP}
DITHER_NAMES = {v: k for k, v in DITHER_MODES.items()}
DITHER_ROW, DITHER_PROG = 0, 1  # stream kinds: a row keyed by its utterance id, a joined programme keyed by its index


def dither_mode_id(mode):
    """A dither mode ("off", "round", "tpdf", "tpdf-hp"; "tpdf_hp" is read as the last) or STN_DITHER_* value -> the value."""
    if isinstance(mode, str) and mode.lower().replace("_", "-") in DITHER_MODES:
        return DITHER_MODES[mode.lower().replace("_", "-")]
    if isinstance(mode, (int, np.integer)) and not isinstance(mode, bool) and int(mode) in DITHER_NAMES:
        return int(mode)
    raise ValueError(f"dither mode {mode!r}: one of {', '.join(DITHER_MODES)}")


def dither_args(dither, seed=None):
    """A dither argument -> None (off) or the normalized (mode name, seed): None, False or "off"; True ("tpdf"); a mode (name or
    STN_DITHER_* value); (mode, seed); or a dict with "mode" and optionally "seed".  seed (here or in the argument; default 0) is an
    integer in [0, 2^64).  Anything else is a ValueError."""
    if dither is None or dither is False:
        return None
    if isinstance(dither, dict):
        extra = set(dither) - {"mode", "seed"}
        if extra or "mode" not in dither:
            raise ValueError(f"dither: a dict of 'mode' and optionally 'seed', not {sorted(dither)}")
        dither, seed = dither["mode"], dither.get("seed", seed)
    elif isinstance(dither, (tuple, list)):
        if len(dither) != 2:
            raise ValueError(f"dither: a mode or (mode, seed), not {dither!r}")
        dither, seed = dither
    mode = DITHER_TPDF if dither is True else dither_mode_id(dither)
    seed = 0 if seed is None else seed
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"dither seed {seed!r}: an integer in [0, 2^64)")
    return None if mode == DITHER_OFF else (DITHER_NAMES[mode], int(seed))


def _pitch_lib():
    L = load()
    ci, cf, i64 = ctypes.c_int, ctypes.c_float, ctypes.c_int64
    L.stn_pitch_ratio.argtypes = [cf, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.stn_pitch_error.argtypes = [cf]
    L.stn_pitch_error.restype = ctypes.c_char_p
    L.stn_pitch_plan.argtypes = [ci, i64, ci, ci, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.stn_pitch_window.argtypes = [ci, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ci)]
    return L


def pitch_error(semitones):
    """Why the engine refuses a pitch of `semitones` (host only; stn_pitch_error), or "" for a value it takes."""
    return _pitch_lib().stn_pitch_error(float(semitones)).decode()


def pitch_args(pitch):
    """A pitch argument -> semitones as a float: None or False is 0.0 (off); a number must be finite and in [-12, 12] (ValueError with
    the engine's message otherwise)."""
    if pitch is None or pitch is False:
        return 0.0
    if isinstance(pitch, bool) or not isinstance(pitch, (int, float, np.integer, np.floating)):
        raise ValueError(f"pitch {pitch!r}: a number of semitones in [-12, 12]")
    why = pitch_error(pitch)
    if why:
        raise ValueError(why)
    return float(np.float32(pitch))


def pitch_ratio(semitones):
    """The fraction (a, b) closest to 2^(semitones / 12) with both terms in [1, 640] (host only; stn_pitch_ratio)."""
    a, b = ctypes.c_int(), ctypes.c_int()
    if _pitch_lib().stn_pitch_ratio(float(semitones), ctypes.byref(a), ctypes.byref(b)) < 0:
        raise StnError(-1, pitch_error(semitones))
    return a.value, b.value


def pitch_cents(semitones):
    """The realised shift of a request in cents: 1200 log2(a / b)."""
    import math
    a, b = pitch_ratio(semitones)
    return 1200.0 * math.log2(a / b)


def pitch_plan(hz, W, a, b):
    """The stretcher's geometry (host only; stn_pitch_plan) -> dict H, N, delta, M, Ws."""
    H, D, M, Ws = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    if _pitch_lib().stn_pitch_plan(int(hz), int(W), int(a), int(b), ctypes.byref(H), ctypes.byref(D), ctypes.byref(M), ctypes.byref(Ws)) < 0:
        raise StnError(-1, f"stn_pitch_plan: bad argument (hz {hz}, W {W}, {a}/{b})")
    return dict(H=H.value, N=2 * H.value, delta=D.value, M=M.value, Ws=Ws.value)


def pitch_window(hz):
    """The stretcher's window at hz (host only; stn_pitch_window) -> float32 [N]."""
    n = ctypes.c_int()
    if _pitch_lib().stn_pitch_window(int(hz), None, 0, ctypes.byref(n)) < 0:
        raise StnError(-1, f"stn_pitch_window: rate {hz} Hz outside [8000, 192000]")
    w = np.empty(n.value, np.float32)
    _pitch_lib().stn_pitch_window(int(hz), w.ctypes.data, w.size, ctypes.byref(n))
    return w


# the pitch mode (STN_PITCH_*, include/stn.h "formant")
PITCH_RESAMPLE, PITCH_FORMANT = 0, 1
PITCH_MODES = {"resample": PITCH_RESAMPLE, "formant": PITCH_FORMANT}
PITCH_MODE_NAMES = {v: k for k, v in PITCH_MODES.items()}


def pitch_mode_id(mode):
    """A pitch-mode argument -> STN_PITCH_RESAMPLE / STN_PITCH_FORMANT: "resample" or "formant" (None: "resample"); anything else is a
    ValueError."""
    if mode is None:
        return PITCH_RESAMPLE
    if isinstance(mode, str) and mode in PITCH_MODES:
        return PITCH_MODES[mode]
    raise ValueError(f"pitch_mode: 'resample' or 'formant', not {mode!r}")


def pitch_mode_name(mode):
    """The normalized name of a pitch-mode argument: None reads as "resample"."""
    return PITCH_MODE_NAMES[pitch_mode_id(mode)]


def _formant_lib():
    L = load()
    ci, i64, dp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    L.stn_formant_plan.argtypes = [ci, i64, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(i64), dp, ctypes.c_size_t]
    L.stn_formant_lpc.argtypes = [ci, dp, ci, dp, ctypes.POINTER(ctypes.c_double), dp]
    return L


def formant_plan(hz, W):
    """The formant correction's geometry (host only; stn_formant_plan) -> dict H, N, p, frames and lag (the lag window, float64 [p + 1])."""
    H, p, F = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    lag = np.zeros(49, np.float64)
    if _formant_lib().stn_formant_plan(int(hz), int(W), ctypes.byref(H), ctypes.byref(p), ctypes.byref(F), lag.ctypes.data, lag.size) < 0:
        raise StnError(-1, f"stn_formant_plan: bad argument (hz {hz}, W {W})")
    return dict(H=H.value, N=2 * H.value, p=p.value, frames=F.value, lag=lag[:p.value + 1].copy())


def formant_lpc(hz, r):
    """The conditioning and Levinson-Durbin in double on the lags r [p + 1] at hz (host only; stn_formant_lpc) -> (a float64 [p + 1],
    the final error, the reflection coefficients float64 [p])."""
    r = np.ascontiguousarray(r, np.float64)
    p = r.size - 1
    a, k, e = np.empty(p + 1, np.float64), np.empty(max(p, 0), np.float64), ctypes.c_double()
    if _formant_lib().stn_formant_lpc(int(hz), r.ctypes.data, p, a.ctypes.data, ctypes.byref(e), k.ctypes.data) < 0:
        raise StnError(-1, f"stn_formant_lpc: bad argument (hz {hz}, p {p})")
    return a, e.value, k


def _dither_lib():
    L = load()
    i64, u64 = ctypes.c_int64, ctypes.c_uint64
    L.stn_dither_noise.argtypes = [ctypes.c_int, u64, ctypes.c_int, u64, i64, i64, ctypes.c_void_p]
    L.stn_dither_quantize.argtypes = [ctypes.c_int, ctypes.c_int, u64, ctypes.c_int, u64, i64, i64, ctypes.c_void_p, ctypes.c_void_p]
    return L


def dither_noise(mode, seed, kind, id, n0, n):
    """The dither of samples n0 .. n0 + n of stream (kind, id) in LSB (host only; stn_dither_noise) -> float32 [n]."""
    d = np.empty(int(n), np.float32)
    if _dither_lib().stn_dither_noise(dither_mode_id(mode), int(seed), int(kind), int(id), int(n0), int(n), d.ctypes.data) < 0:
        raise StnError(-1, "stn_dither_noise: bad argument")
    return d


def dither_quantize(enc, mode, seed, kind, id, n0, v):
    """v (float32 [n]) as the samples n0 .. of stream (kind, id) in 16- or 24-bit PCM under a mode (host only; stn_dither_quantize) ->
    int16 [n] or uint8 [n, 3]."""
    v = np.ascontiguousarray(v, np.float32).ravel()
    e = encoding_id(enc)
    out = encoded_empty(e, 1, v.size)[0] if e in (ENC_PCM16, ENC_PCM24) else np.empty(v.size, np.uint8)
    if _dither_lib().stn_dither_quantize(e, dither_mode_id(mode), int(seed), int(kind), int(id), int(n0), v.size, v.ctypes.data, out.ctypes.data) < 0:
        raise StnError(-1, "stn_dither_quantize: bad argument")
    return out


def true_peak_filter():
    """The 4x oversampling filter of the true-peak mode (host only): float32 [4, 16], every phase's DC gain 1, phase 0 the unit tap."""
    L = load()
    P, T = ctypes.c_int(), ctypes.c_int()
    if L.stn_true_peak_filter(None, 0, ctypes.byref(P), ctypes.byref(T)) < 0:
        raise StnError(-1, "stn_true_peak_filter failed")
    taps = np.empty((P.value, T.value), np.float32)
    if L.stn_true_peak_filter(taps.ctypes.data, taps.size, ctypes.byref(P), ctypes.byref(T)) < 0:
        raise StnError(-1, "stn_true_peak_filter failed")
    return taps


def limiter_window(hz, lookahead_ms=LIMITER_MS):
    """The limiter's weights at hz (host only): float32 [A + 1], A = int(lookahead_ms * hz / 1000 + 0.5), a Hann window
    0.5 - 0.5 cos(2 pi (k + 1) / (A + 2)) normalized to sum 1.  StnError when lookahead_ms is outside [0.5, 10] or hz outside
    [8000, 192000]."""
    L = load()
    n = ctypes.c_int64()
    if L.stn_limiter_window(int(hz), float(lookahead_ms), None, 0, ctypes.byref(n)) < 0:
        raise StnError(-1, f"stn_limiter_window: {lookahead_ms} ms at {hz} Hz refused (lookahead_ms in [0.5, 10], hz in [8000, 192000])")
    w = np.empty(n.value, np.float32)
    if L.stn_limiter_window(int(hz), float(lookahead_ms), w.ctypes.data, w.size, ctypes.byref(n)) < 0:
        raise StnError(-1, "stn_limiter_window failed")
    return w


def _loudness_args(target_lufs):
    """(on, target) for stn_set_loudness: None = off (the target passed along is then the default, -23 LUFS)"""
    return (0, -23.0) if target_lufs is None else (1, float(target_lufs))


def resample_error(in_hz, out_hz):
    """Why the pair is refused, or "" when it is supported (host only)."""
    return load().stn_resample_error(int(in_hz), int(out_hz)).decode()


def resample_form(in_hz, out_hz, W):
    """The form the resampler's launcher takes for rows of W samples (stn_dbg_resample_form; host-only): "resample lds G<n>" or
    "resample cache G<n>", n the groups of 64 output periods a workgroup owns."""
    buf = ctypes.create_string_buffer(64)
    r = load().stn_dbg_resample_form(int(in_hz), int(out_hz), int(W), buf, len(buf))
    if r < 0:
        why = resample_error(in_hz, out_hz)
        raise StnError(r, f"stn_dbg_resample_form: {why}" if why else f"stn_dbg_resample_form: W = {W}, W >= 1 is required")
    return buf.value.decode()


def fold_run_frames(latent_lengths, n_cu=256):
    """frames per workgroup of the estimator's fold kernel for these latent lengths (0 = the default 32); host-only"""
    a = np.ascontiguousarray(latent_lengths, dtype=np.int32)
    r = load().stn_dbg_fold_run_frames(a.ctypes.data, len(a), int(n_cu))
    if r < 0:
        raise StnError(r, "stn_dbg_fold_run_frames: bad arguments")
    return int(r)


def gemm_form(dtype, M, N, K, mode=EPI_STORE, out_dtype="f32", ldo=None, masked=False, tr=-1):
    """The form the engine's GEMM launcher takes for this call (stn_dbg_gemm_form; host-only), e.g. "tiled<128,128,2,4,4,64,2> cfg8 tr".
    Where the form is tiled, the string names the kernel template arguments <BM,BN,WM,WN,NSTAGE,KS,ESZ>."""
    buf = ctypes.create_string_buffer(128)
    r = load().stn_dbg_gemm_form(_DTYPES[dtype], int(M), int(N), int(K), int(mode), _DTYPES[out_dtype], int(N if ldo is None else ldo),
                                 int(bool(masked)), int(tr), buf, len(buf))
    if r < 0:
        raise StnError(r, "stn_dbg_gemm_form: the launcher refuses this call")
    return buf.value.decode()


def attn_form(dtype, B, Lq, Lk, H, dh, ldq=None, ldk=None, misaligned=0, kind=0):
    """The form the engine's attention launchers take (stn_dbg_attn_form; host-only).  kind 0, launch_attention: e.g. "mfma<64,bf16> kc128
    nch3", "scalar<f32,TPR8> vec"; misaligned: bits 1 / 2 / 4 = the q / k / v pointer 4 bytes off 16-byte alignment.  kind 1, the
    head-split launch (C = H*dh, L = Lq): e.g. "xattn_hs<f16,U2> kc64".  ld defaults to H*dh."""
    buf = ctypes.create_string_buffer(64)
    C = H * dh
    r = load().stn_dbg_attn_form(int(kind), _DTYPES[dtype], int(B), int(Lq), int(Lk), int(H), int(dh), int(C if ldq is None else ldq),
                                 int(C if ldk is None else ldk), int(misaligned), buf, len(buf))
    if r < 0:
        raise StnError(r, "stn_dbg_attn_form: the launcher refuses this call")
    return buf.value.decode()


def dwconv_ln_form(dtype, B, L, C, k, packed=False):
    """The form the engine's depthwise-conv + LayerNorm launcher takes (stn_dbg_dwconv_ln_form; host-only): "v3<K,R>", "v3occ4<7,4>",
    "v2<K>" or "generic".  Raises StnError where the launcher refuses the call."""
    buf = ctypes.create_string_buffer(32)
    r = load().stn_dbg_dwconv_ln_form(_DTYPES[dtype], int(B), int(L), int(C), int(k), int(bool(packed)), buf, len(buf))
    if r < 0:
        raise StnError(r, "stn_dbg_dwconv_ln_form: the launcher refuses this call")
    return buf.value.decode()


LEN_VO_NONE, LEN_VO_2RF, LEN_VO_TAIL, LEN_VO_SCALED = range(4)


def len_tables(llen, ve_rows=0, with_pairs=False, vo_form=LEN_VO_NONE, ccf=6, T=0, rf=0):
    """The length tables a batch run uploads in front of its pipeline, built on the host (stn_dbg_len_tables; no device).  Returns a dict of
    int32 arrays: llen, and where built ve_off [B+1], ve_row_b [ve_rows], pairs [B+2], vo_n, vo_valid [B], vo_off [B+1]; 'total' (words)."""
    llen = _c(llen, np.int32)
    B = len(llen)
    lay = np.zeros(9, np.int32)
    args = (B, llen, int(ve_rows), int(bool(with_pairs)), int(vo_form), int(ccf), int(T), int(rf))
    tot = load().stn_dbg_len_tables(*args, lay, None, 0)
    if tot < 0:
        raise StnError(int(tot), "stn_dbg_len_tables: bad argument")
    out = np.full(tot, -12345, np.int32)
    out[:2] = 7
    assert load().stn_dbg_len_tables(*args, lay, out.ctypes.data, out.size) == tot
    assert out[0] == 7 and out[1] == 7  # the seed words are the caller's
    names = ("seed", "llen", "ve_off", "ve_row_b", "pairs", "vo_n", "vo_valid", "vo_off")
    sizes = {"llen": B, "ve_off": B + 1, "ve_row_b": int(ve_rows), "pairs": B + 2, "vo_n": B, "vo_valid": B, "vo_off": B + 1}
    res = {"total": int(tot)}
    for i, n in enumerate(names):
        if n != "seed" and lay[i] >= 0:
            res[n] = out[lay[i]:lay[i] + sizes[n]].copy()
    return res


def fold_dwconv_ln_form(dtype, B, L, C, k, dil, S, rowvec=True, run_frames=0):
    """The form the fold + depthwise-conv + LayerNorm launcher takes (stn_dbg_fold_dwconv_ln_form; host-only), e.g.
    "fold_dwconv_ln<bf16,K5,rv,ns3,S4,U3> run 40 cps 3": kernel instantiation, run length in frames, workgroups per sequence.  Raises
    StnError where the launcher refuses the call."""
    buf = ctypes.create_string_buffer(96)
    r = load().stn_dbg_fold_dwconv_ln_form(_DTYPES[dtype], int(B), int(L), int(C), int(k), int(dil), int(S), int(bool(rowvec)), int(run_frames),
                                           buf, len(buf))
    if r < 0:
        raise StnError(r, "stn_dbg_fold_dwconv_ln_form: the launcher refuses this call")
    return buf.value.decode()


def ffn_form(dtype, stage, C, I, M, gate_rows=0, packed=True, k=5, max_dil=1, mask=9, min_rows=18432, split_min_rows=1, nt_hints=True):
    """The form a ConvNeXt block's pointwise pair takes (stn_dbg_ffn_form; host-only): "gemms", "gemms nt", "k4" or "k4splitS".
    stage: FFN_VOCODER, FFN_ESTIMATOR or FFN_TEXT; the settings default to the engine's."""
    buf = ctypes.create_string_buffer(32)
    r = load().stn_dbg_ffn_form(_DTYPES[dtype], int(stage), int(C), int(I), int(M), int(gate_rows), int(bool(packed)), int(k), int(max_dil),
                                int(mask), int(min_rows), int(split_min_rows), int(bool(nt_hints)), buf, len(buf))
    if r < 0:
        raise StnError(r, "stn_dbg_ffn_form: invalid arguments")
    return buf.value.decode()


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _opt(a, dt):
    if a is None:
        return None, None
    arr = _c(a, dt)
    return arr, arr.ctypes.data


class Engine:
    """One GPU + one HIP stream.  Mirrors the four ONNX sessions of the reference's TextToSpeech
    (/root/reference/cpp/helper.cpp:404-422) behind the C ABI."""

    def __init__(self, device=0, dtype="bf16"):
        self._lib = load()
        self._h = ctypes.c_void_p()
        cfg = StnConfig(device, _DTYPES[dtype])
        rc = self._lib.stn_create(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc != 0:
            msg = self._lib.stn_last_error(None).decode()
            self._h = None
            raise StnError(rc, msg)
        self.dtype = _DTYPES[dtype]
        self.device = device
        self.arch = None
        self._slot_enc = {}  # encoding each fetch slot was begun with

    def close(self):
        if getattr(self, "_h", None):
            self._lib.stn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _need_model(self):
        if self.arch is None:
            raise StnError(-3, "no model loaded: call load_synthetic or load_dir first")

    def _ck(self, rc):
        if rc < 0:
            raise StnError(rc, self._lib.stn_last_error(self._h).decode())
        return rc

    # ---- model -------------------------------------------------------------------------------
    def load_synthetic(self, arch: StnArch, seed: int = 7):
        self._ck(self._lib.stn_load_synthetic(self._h, ctypes.byref(arch), seed))
        self.arch = arch

    def last_error(self) -> str:
        """stn_last_error: the last failure's text — or, after a successful manifest-less stn_load_dir, its notes."""
        return (self._lib.stn_last_error(self._h) or b"").decode()

    def load_dir(self, onnx_dir: str):
        self._ck(self._lib.stn_load_dir(self._h, onnx_dir.encode()))
        a = StnArch()
        self._ck(self._lib.stn_get_arch(self._h, ctypes.byref(a)))
        self.arch = a

    def tensor_names(self, arch: StnArch):
        n = self._ck(self._lib.stn_tensor_names(self._h, ctypes.byref(arch), None, 0))
        buf = ctypes.create_string_buffer(n + 1)
        self._ck(self._lib.stn_tensor_names(self._h, ctypes.byref(arch), buf, n + 1))
        return buf.value.decode().split("\n")[:-1]

    @property
    def param_count(self):
        return self._lib.stn_param_count(self._h)

    # ---- the four former Run sites ----------------------------------------------------------------
    def duration(self, text_ids, style_dp, text_mask):
        self._need_model()
        B, Lt = text_ids.shape
        out = np.empty(B, np.float32)
        self._ck(self._lib.stn_duration(self._h, B, Lt, _c(text_ids, np.int64), _c(style_dp, np.float32),
                                        _c(text_mask, np.float32), out))
        return out

    def text_enc(self, text_ids, style_ttl, text_mask):
        self._need_model()
        B, Lt = text_ids.shape
        out = np.empty((B, self.arch.te_out_dim, Lt), np.float32)
        self._ck(self._lib.stn_text_enc(self._h, B, Lt, _c(text_ids, np.int64), _c(style_ttl, np.float32),
                                        _c(text_mask, np.float32), out))
        return out

    def vector_est(self, noisy, text_emb, style_ttl, text_mask, latent_mask, total_step, current_step):
        self._need_model()
        B, D, L = noisy.shape
        Lt = text_emb.shape[2]
        out = np.empty((B, D, L), np.float32)
        self._ck(self._lib.stn_vector_est(self._h, B, L, Lt, _c(noisy, np.float32), _c(text_emb, np.float32),
                                          _c(style_ttl, np.float32), _c(text_mask, np.float32),
                                          _c(latent_mask, np.float32), _c(total_step, np.float32),
                                          _c(current_step, np.float32), out))
        return out

    def vocoder(self, latent):
        self._need_model()
        B, D, L = latent.shape
        out = np.empty((B, L * self.arch.chunk_size), np.float32)
        self._ck(self._lib.stn_vocoder(self._h, B, L, _c(latent, np.float32), out))
        return out

    # ---- fused, HBM-resident synthesis ----------------------------------------------------------------
    def batch_upload(self, text_ids, text_mask, style_ttl, style_dp, duration_override=None, utt_ids=None):
        B, Lt = text_ids.shape
        _d, dptr = _opt(duration_override, np.float32)
        _u, uptr = _opt(utt_ids, np.int64)
        self._ck(self._lib.stn_batch_upload(self._h, B, Lt, _c(text_ids, np.int64), _c(text_mask, np.float32),
                                            _c(style_ttl, np.float32), _c(style_dp, np.float32), dptr, uptr))

    def batch_set_noise(self, noise):
        noise = _c(noise, np.float32)
        self._ck(self._lib.stn_batch_set_noise(self._h, noise, noise.shape[2]))

    def batch_run(self, total_step=5, speed=1.05, noise_seed=1234):
        self._ck(self._lib.stn_batch_run(self._h, total_step, speed, noise_seed))

    def set_graph_mode(self, on=True):
        self._ck(self._lib.stn_set_graph_mode(self._h, int(on)))

    def set_packed_rows(self, on=True):
        """Vector-estimator row layout in batch_run: packed (default, no work on padding) or padded [b*L + t]."""
        self._ck(self._lib.stn_set_row_layout(self._h, int(bool(on))))

    def set_fused_ffn(self, mask):
        """K4 stage mask: 1 vocoder, 2 vector estimator, 4 text encoder / duration predictor (0 = two GEMM launches everywhere)."""
        self._ck(self._lib.stn_set_fused_ffn(self._h, int(mask)))

    def set_shape_buckets(self, on=True):
        """Round Lt, L and the packed row counts up to bucket boundaries so that requests of unlike lengths share captured graphs."""
        self._ck(self._lib.stn_set_shape_buckets(self._h, int(bool(on))))

    def set_duration_read(self, always):
        """Measurement aid: read the predicted durations back even when they are overridden (the critical path of a predicted-duration run)."""
        self._ck(self._lib.stn_set_duration_read(self._h, int(bool(always))))

    def set_gelu_form(self, tanh_form):
        """0 erf (default), 1 the tanh approximation (what stn_load_dir selects for graphs that spell GELU with Tanh)."""
        self._ck(self._lib.stn_set_gelu_form(self._h, int(bool(tanh_form))))

    @property
    def gelu_form(self):
        return self._lib.stn_get_gelu_form(self._h)

    def set_fused_xattn(self, on=True):
        """Cross-attention blocks of the vector estimator: True head-split (default), False four launches."""
        self._ck(self._lib.stn_set_fused_xattn(self._h, int(on)))

    @property
    def vo_rows(self):
        return self._lib.stn_batch_vo_rows(self._h)

    @property
    def ve_rows(self):
        return self._lib.stn_batch_ve_rows(self._h)

    def set_vocoder_mode(self, length_aware):
        """False: the reference's batched vocoder (padding decoded as zero latent). True: every utterance ends at its own length."""
        self._ck(self._lib.stn_set_vocoder_mode(self._h, int(bool(length_aware))))

    def set_output_rate(self, hz):
        """Rate of every fetch (0 or None = the model's rate, the default): the finished waveform is resampled on the GPU."""
        self._ck(self._lib.stn_set_output_rate(self._h, int(hz or 0)))

    @property
    def output_rate(self):
        """The effective rate of the fetches (the model's rate when no output rate is set)."""
        return self._lib.stn_get_output_rate(self._h)

    def op_resample(self, x, in_hz, out_hz, pcm=False):
        """rows x W fp32 at in_hz -> rows x ceil(W*P/Q) at out_hz on the GPU: fp32, or (pcm=True) the int16 PCM epilogue."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        P, T = resample_filter(in_hz, out_hz).shape
        import math
        g = math.gcd(int(in_hz), int(out_hz))
        Q = int(in_hz) // g
        W_out = -(-W * P // Q)
        out = np.empty((rows, W_out), np.int16 if pcm else np.float32)
        self._ck(self._lib.stn_op_resample(self._h, int(in_hz), int(out_hz), rows, W, x, None if pcm else out.ctypes.data,
                                           out.ctypes.data if pcm else None))
        return out

    def set_filters(self, filters=None):
        """Filter every row of every fetch through a chain of up to 8 biquads on the GPU, at the output rate, after the resampler and
        before everything else (trimming, loudness, limiter, encoding, join): None or [] = off (the default).  Entries as filter_args
        takes them, e.g. [("highpass", 80)] or [{"type": "peak", "freq": 3000, "q": 1, "gain_db": 4}].  StnError naming the field for a
        value outside the limits at the output rate in force (include/stn.h, "filter chain")."""
        n, arr = _filter_array(filters)
        self._ck(self._lib.stn_set_filters(self._h, n, arr))

    def get_filters(self):
        """The chain in force: a tuple of (type name, freq_hz, q, gain_db), empty when off."""
        n, arr = ctypes.c_int(), (StnFilter * MAX_FILTERS)()
        self._ck(self._lib.stn_get_filters(self._h, ctypes.byref(n), arr))
        return tuple((FILTER_TYPE_NAMES[arr[i].type], arr[i].freq_hz, arr[i].q, arr[i].gain_db) for i in range(n.value))

    def op_filter(self, x, hz, filters):
        """rows x W fp32 at hz through the chain on the GPU -> y [rows, W] float32, every row from zero state."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        n, arr = _filter_array(filters)
        y = np.empty_like(x)
        self._ck(self._lib.stn_op_filter(self._h, int(hz), x.shape[0], x.shape[1], x, n, arr, y))
        return y

    def op_filter_ex(self, x, hz, filters, x_misalign=0):
        """op_filter with its scratch laid open -> dict: y [rows, W]; st_end, st_start [P, rows, Ks, 4] (per section pass of two biquads:
        the chunks' end states from zero state, their start states after the scan; the state buffer is poisoned with the quiet NaN
        0x7FC00000 before every pass); guard_ok (the poisoned floats around x and y came back whole); form ("vec" / "scalar").
        x_misalign = 1 places x and y 4 bytes off 16-byte alignment."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        n, arr = _filter_array(filters)
        P, Ks = (n + 1) // 2, (W + 31) // 32
        o = dict(y=np.empty_like(x), st_end=np.empty((P, rows, Ks, 4), np.float32), st_start=np.empty((P, rows, Ks, 4), np.float32))
        ok, form = ctypes.c_int(), ctypes.create_string_buffer(16)
        self._ck(self._lib.stn_op_filter_ex(self._h, int(hz), rows, W, x, n, arr, int(x_misalign), o["y"], o["st_end"].ctypes.data,
                                            o["st_start"].ctypes.data, ctypes.byref(ok), form, ctypes.sizeof(form)))
        o["guard_ok"] = bool(ok.value)
        o["form"] = form.value.decode()
        return o

    # ---- what the three dynamics stages' methods share (d: _COMPRESSOR, _EXPANDER or _DEESSER)
    def _get_dynamics(self, d):
        on, c = ctypes.c_int(), d.struct()
        self._ck(getattr(self._lib, f"stn_get_{d.unit}")(self._h, ctypes.byref(on), ctypes.byref(c)))
        return _dyn_tuple(d, c) if on.value else None

    def _batch_rows(self, fn, *dtypes):
        """a report of one array [B] per dtype -> the tuple of them"""
        out = tuple(np.zeros(self.batch_dims()[0], t) for t in dtypes)
        self._ck(fn(self._h, *(a.ctypes.data for a in out)))
        return out

    def _op_dynamics(self, d, x, hz, value):
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        y = np.empty_like(x)
        self._ck(getattr(self._lib, f"stn_op_{d.unit}")(self._h, int(hz), x.shape[0], x.shape[1], x, ctypes.byref(_dyn_struct(d, value)), y))
        return y

    def _op_dynamics_ex(self, d, x, hz, value, x_misalign, in_place, per_sample, band_states=()):
        """per_sample: the outputs [rows, W] behind y; band_states: those [rows, Ks, 4]; then the four [rows, Ks], guard_ok and form"""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        Ks = (W + 31) // 32
        o = dict(y=np.empty_like(x), **{k: np.empty_like(x) for k in per_sample})
        for k in band_states:
            o[k] = np.empty((rows, Ks, 4), np.float32)
        for k in ("s1_end", "s1_start", "s2_end", "s2_start"):
            o[k] = np.empty((rows, Ks), np.float32)
        ok, form = ctypes.c_int(), ctypes.create_string_buffer(16)
        probes = [a.ctypes.data for k, a in o.items() if k != "y"]
        self._ck(getattr(self._lib, f"stn_op_{d.unit}_ex")(self._h, int(hz), rows, W, x, ctypes.byref(_dyn_struct(d, value)), int(x_misalign),
                                                            int(in_place), o["y"], *probes, ctypes.byref(ok), form, ctypes.sizeof(form)))
        o["guard_ok"] = bool(ok.value)
        o["form"] = form.value.decode()
        return o

    def set_compressor(self, compressor=None):
        """Compress the dynamic range of every row of every fetch on the GPU, at the output rate, behind the filter chain and before
        everything else (trimming, loudness, limiter, encoding, join): None or False = off (the default); True = the "speech" default;
        a dict or 6-tuple as compressor_args takes them, e.g. {"threshold_db": -20, "ratio": 4}.  StnError naming the field for a value
        outside the limits (include/stn.h, "compressor")."""
        _set_dynamics(self, self._lib.stn_set_compressor, self._h, _COMPRESSOR, compressor)

    def get_compressor(self):
        """The setting in force: the 6-tuple (threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db), or None when off."""
        return self._get_dynamics(_COMPRESSOR)

    def batch_compressor(self):
        """Per row of the finished batch, the largest reduction in dB the compressor applied over the row's valid samples (float32 [B];
        zeros while it is off)."""
        return self._batch_rows(self._lib.stn_batch_compressor, np.float32)[0]

    def op_compressor(self, x, hz, compressor):
        """rows x W fp32 at hz through the compressor on the GPU -> y [rows, W] float32, every row from zero state."""
        return self._op_dynamics(_COMPRESSOR, x, hz, compressor)

    def op_compressor_ex(self, x, hz, compressor, x_misalign=0, in_place=0):
        """op_compressor with its scratch laid open -> dict: y, gr_db (yL) [rows, W]; s1_end, s1_start, s2_end, s2_start [rows, Ks] (per
        chunk of 32 samples: y1 at its end from zero, y1 at its start after the scan, yL at its end from zero, yL at its start; the
        scratch is poisoned with the quiet NaN 0x7FC00000 first); guard_ok (the poisoned floats around x and y came back whole); form
        ("vec" / "scalar").  x_misalign = 1 places x and y 4 bytes off 16-byte alignment; in_place = 1 writes y over x on the device."""
        return self._op_dynamics_ex(_COMPRESSOR, x, hz, compressor, x_misalign, in_place, ("gr_db",))

    def set_expander(self, expander=None):
        """Turn down what lies under a threshold (the noise floor between words) in every row of every fetch on the GPU, at the output
        rate, behind the filter chain and in front of the de-esser, the compressor and everything else: None or False = off (the
        default); True = the "speech" default; a dict or 7-tuple as expander_args takes them, e.g. {"threshold_db": -45}.  StnError
        naming the field for a value outside the limits (include/stn.h, "expander")."""
        _set_dynamics(self, self._lib.stn_set_expander, self._h, _EXPANDER, expander)

    def get_expander(self):
        """The setting in force: the 7-tuple (threshold_db, ratio, knee_db, range_db, attack_ms, hold_ms, release_ms), or None when off."""
        return self._get_dynamics(_EXPANDER)

    expander = property(get_expander)

    def batch_expander(self):
        """Per row of the finished batch, over the row's valid samples: (min_attenuation_db float32 [B], the least attenuation the
        expander applied; closed_samples int64 [B], the samples at least half closed).  Zeros while it is off."""
        return self._batch_rows(self._lib.stn_batch_expander, np.float32, np.int64)

    def op_expander(self, x, hz, expander):
        """rows x W fp32 at hz through the expander on the GPU -> y [rows, W] float32, every row from zero state (closed)."""
        return self._op_dynamics(_EXPANDER, x, hz, expander)

    def op_expander_ex(self, x, hz, expander, x_misalign=0, in_place=0):
        """op_expander with its scratch laid open -> dict: y, open_db (yL) [rows, W]; s1_end, s1_start, s2_end, s2_start [rows, Ks] (per
        chunk of 32 samples: u at its end from zero, u at its start after the scan, yL at its end from zero, yL at its start; the
        scratch is poisoned with the quiet NaN 0x7FC00000 first); guard_ok (the poisoned floats around x and y came back whole); form
        ("vec" / "scalar").  x_misalign = 1 places x and y 4 bytes off 16-byte alignment; in_place = 1 writes y over x on the device."""
        return self._op_dynamics_ex(_EXPANDER, x, hz, expander, x_misalign, in_place, ("open_db",))

    def set_deesser(self, deesser=None):
        """Turn down the sibilants of every row of every fetch on the GPU, at the output rate, behind the filter chain and in front of the
        compressor and everything else: None or False = off (the default); True = the "speech" default; a dict or 8-tuple as deesser_args
        takes them, e.g. {"freq_hz": 6000, "threshold_db": -28}.  StnError naming the field for a value outside the limits, the two that
        depend on the output rate in force included (include/stn.h, "de-esser")."""
        _set_dynamics(self, self._lib.stn_set_deesser, self._h, _DEESSER, deesser)

    def get_deesser(self):
        """The setting in force: the 8-tuple (freq_hz, threshold_db, ratio, knee_db, attack_ms, release_ms, range_db, mode), or None when off."""
        return self._get_dynamics(_DEESSER)

    def batch_deesser(self):
        """Per row of the finished batch, the largest reduction in dB the de-esser applied over the row's valid samples (float32 [B];
        zeros while it is off)."""
        return self._batch_rows(self._lib.stn_batch_deesser, np.float32)[0]

    def op_deesser(self, x, hz, deesser):
        """rows x W fp32 at hz through the de-esser on the GPU -> y [rows, W] float32, every row from zero state."""
        return self._op_dynamics(_DEESSER, x, hz, deesser)

    def op_deesser_ex(self, x, hz, deesser, x_misalign=0, in_place=0):
        """op_deesser with its scratch laid open -> dict: y, band (h), gr_db (yL) [rows, W]; st_end, st_start [rows, Ks, 4] (the band's
        state per chunk of 32 samples: at its end from zero, at its start after the scan); s1_end, s1_start, s2_end, s2_start [rows, Ks]
        (y1 and yL likewise; the scratch is poisoned with the quiet NaN 0x7FC00000 first); guard_ok (the poisoned floats around x and y
        came back whole); form ("vec" / "scalar").  x_misalign = 1 places x and y 4 bytes off 16-byte alignment; in_place = 1 writes y
        over x on the device."""
        return self._op_dynamics_ex(_DEESSER, x, hz, deesser, x_misalign, in_place, ("band", "gr_db"), ("st_end", "st_start"))

    def set_loudness(self, target_lufs=None, ceiling_dbfs=-1.0):
        """Normalize every fetch to target_lufs (BS.1770-4 integrated loudness, [-60, 0]) with the gain capped so that the sample
        peak stays at or below ceiling_dbfs ([-30, 0]); None = off (the default).  Measured on the GPU at the output rate."""
        on, t = _loudness_args(target_lufs)
        self._ck(self._lib.stn_set_loudness(self._h, on, t, float(ceiling_dbfs)))

    def _loudness(self):
        on, t, c = ctypes.c_int(), ctypes.c_float(), ctypes.c_float()
        self._ck(self._lib.stn_get_loudness(self._h, ctypes.byref(on), ctypes.byref(t), ctypes.byref(c)))
        return bool(on.value), t.value, c.value

    @property
    def loudness(self):
        """The normalization target in LUFS, or None when normalization is off."""
        on, t, _ = self._loudness()
        return t if on else None

    @property
    def loudness_ceiling(self):
        """The sample-peak ceiling of the normalization gain, dBFS."""
        return self._loudness()[2]

    def batch_loudness(self):
        """The finished batch measured at the output rate -> (lufs [B], peak [B], gain [B]) float32; gain is what the current setting
        applies (1 when off); lufs is -inf where a row is shorter than one 400 ms block or every block is gated out."""
        B = self.batch_dims()[0]
        lufs, peak, gain = (np.empty(B, np.float32) for _ in range(3))
        self._ck(self._lib.stn_batch_loudness(self._h, lufs.ctypes.data, peak.ctypes.data, gain.ctypes.data))
        return lufs, peak, gain

    def op_loudness(self, x, hz, n=None):
        """rows x W fp32 at hz on the GPU -> (lufs [rows], peak [rows]) over row r's first n[r] samples (None: all W)."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        nn = None if n is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int64), (rows,)))
        lufs, peak = np.empty(rows, np.float32), np.empty(rows, np.float32)
        self._ck(self._lib.stn_op_loudness(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, lufs.ctypes.data,
                                           peak.ctypes.data))
        return lufs, peak

    @staticmethod
    def _range_out(rows):
        out = tuple(np.empty(rows, np.float32) for _ in range(3)) + (np.empty(rows, np.int32),)
        return out, [a.ctypes.data for a in out]

    def batch_loudness_range(self):
        """The finished batch measured at the output rate, over the spans of batch_loudness -> (max_momentary [B], max_short_term [B],
        range [B]) float32 and n_short_term [B] int32: the 400 ms and 3 s maxima in LUFS (-inf where the span holds no block / no
        window), the loudness range in LU (EBU Tech 3342) and the 3 s windows behind its gates.  Measured before the loudness gain."""
        out, ptr = self._range_out(self.batch_dims()[0])
        self._ck(self._lib.stn_batch_loudness_range(self._h, *ptr))
        return out

    def batch_join_loudness_range(self, rows, gap_samples, gap_seconds, mode="whole"):
        """batch_loudness_range of the joined signal measured as programmes (batch_join_loudness's spans) -> four arrays [G]."""
        j, keep = _join(rows, gap_samples, gap_seconds, mode, JOIN_GAIN_PROG)
        out, ptr = self._range_out(keep[0].size)
        self._ck(self._lib.stn_batch_join_loudness_range(self._h, ctypes.byref(j), *ptr))
        return out

    def op_loudness_range(self, x, hz, n=None):
        """rows x W fp32 at hz on the GPU -> (max_momentary, max_short_term, range, n_short_term) [rows] over row r's first n[r] samples
        (None: all W)."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        nn = None if n is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int64), (rows,)))
        out, ptr = self._range_out(rows)
        self._ck(self._lib.stn_op_loudness_range(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, *ptr))
        return out

    @staticmethod
    def _f0_out(rows, cap):
        f0, ap, st = np.empty((rows, cap), np.float32), np.empty((rows, cap), np.float32), np.zeros(rows, F0_STATS)
        return f0, ap, st

    def batch_f0(self, params=None):
        """The pitch report of the finished batch at the output rate (include/stn.h "f0": YIN on the rows batch_loudness measures, before
        the loudness gain) -> (f0 [B, Fmax], ap [B, Fmax], stats): f0 in Hz, 0 for an unvoiced frame, ap the aperiodicity d'(tau^);
        stats a dict of [B] arrays frames, voiced, median_hz, mean_hz, min_hz, max_hz.  Row b's frames are columns 0 .. frames[b] - 1."""
        p = f0_params(params)
        cap = ctypes.c_int64()
        self._ck(self._lib.stn_batch_f0_frames(self._h, ctypes.addressof(p), cap))
        f0, ap, st = self._f0_out(self.batch_dims()[0], cap.value)
        self._ck(self._lib.stn_batch_f0(self._h, ctypes.addressof(p), cap.value, f0.ctypes.data, ap.ctypes.data, st.ctypes.data))
        return f0, ap, {k: st[k].copy() for k in F0_STATS.names}

    def op_f0(self, x, hz, n=None, params=None, cap=None):
        """rows x W fp32 at hz on the GPU -> (f0, ap, stats) as batch_f0 over row r's first n[r] samples (None: all W).  cap: the
        columns of f0 / ap (None: the longest row's frame count)."""
        p = f0_params(params)
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        nn = None if n is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int64), (rows,)))
        if cap is None:
            why = f0_error(hz, p)
            if why:
                raise StnError(-1, why)
            cap = max((f0_plan(hz, max(0, int(v)), p)["frames"] for v in (nn if nn is not None else [W])), default=0)
            cap = min(cap, f0_group()[1])  # (a longer row is the engine's to refuse, before it uploads anything)
        f0, ap, st = self._f0_out(rows, int(cap))
        self._ck(self._lib.stn_op_f0(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, ctypes.addressof(p), int(cap),
                                     f0.ctypes.data, ap.ctypes.data, st.ctypes.data))
        return f0, ap, {k: st[k].copy() for k in F0_STATS.names}

    def op_loudness_ex(self, x, hz, n=None, on=False, target_lufs=-23.0, ceiling_dbfs=-1.0, x_misalign=0):
        """op_loudness with its scratch laid open (poisoned with the quiet NaN 0x7FC00000 first) -> dict: st_end, st_start [rows, Ks, 4]
        (chunk end states from zero state; true start states after the scan), pk, pa, pb [rows, Ks], lufs, peak, gain [rows], form
        ("vec" / "scalar": the staging path that ran).  x_misalign = 1 uploads x 4 bytes off 16-byte alignment."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        Ks = (W + 31) // 32
        nn = None if n is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int64), (rows,)))
        o = dict(st_end=np.empty((rows, Ks, 4), np.float32), st_start=np.empty((rows, Ks, 4), np.float32))
        o.update({k: np.empty((rows, Ks), np.float32) for k in ("pk", "pa", "pb")})
        o.update({k: np.empty(rows, np.float32) for k in ("lufs", "peak", "gain")})
        form = ctypes.create_string_buffer(16)
        self._ck(self._lib.stn_op_loudness_ex(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, int(bool(on)), float(target_lufs),
                                              float(ceiling_dbfs), int(x_misalign), *(o[k].ctypes.data for k in ("st_end", "st_start", "pk", "pa", "pb",
                                                                                                                 "lufs", "peak", "gain")),
                                              form, ctypes.sizeof(form)))
        o["form"] = form.value.decode()
        return o

    def set_silence_trim(self, trim_silence=None):
        """Trim leading and trailing silence of every fetch by level on the GPU: None = off (the default), top_db (frames more than
        top_db below the row's loudest 10 ms frame are silence; 20 ms kept, 5 ms fade) or (top_db, keep_ms, fade_ms)."""
        on, db, keep, fade = silence_trim_args(trim_silence)
        self._ck(self._lib.stn_set_silence_trim(self._h, on, db, keep, fade))

    @property
    def silence_trim(self):
        """(top_db, keep_ms, fade_ms), or None when trimming is off."""
        on, db, keep, fade = ctypes.c_int(), ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        self._ck(self._lib.stn_get_silence_trim(self._h, ctypes.byref(on), ctypes.byref(db), ctypes.byref(keep), ctypes.byref(fade)))
        return (db.value, keep.value, fade.value) if on.value else None

    def batch_silence_edges(self):
        """The finished batch's edges at the output rate under the current parameters, trimming on or off -> (start [B], end [B]) int64."""
        B = self.batch_dims()[0]
        start, end = np.empty(B, np.int64), np.empty(B, np.int64)
        self._ck(self._lib.stn_batch_silence_edges(self._h, start.ctypes.data, end.ctypes.data))
        return start, end

    def op_silence_edges(self, x, hz, n=None, top_db=40.0, keep_ms=TRIM_KEEP_MS):
        """rows x W fp32 at hz on the GPU -> (start [rows], end [rows]) over row r's first n[r] samples (None: all W)."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        nn = None if n is None else np.ascontiguousarray(n, np.int64)
        start, end = np.empty(rows, np.int64), np.empty(rows, np.int64)
        self._ck(self._lib.stn_op_silence_edges(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, float(top_db), float(keep_ms),
                                                start.ctypes.data, end.ctypes.data))
        return start, end

    def op_silence_trim(self, x, hz, n=None, top_db=40.0, keep_ms=TRIM_KEEP_MS, fade_ms=TRIM_FADE_MS, gain=None, encoding=None):
        """Detection plus the trimmed store on the GPU -> (y [rows, W] in the encoding (encoded_empty's dtypes), start, end): row r's
        segment from column 0, times gain[r], cut edges faded, zero codewords behind it."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        e = ENC_F32 if encoding is None else encoding_id(encoding)
        nn = None if n is None else np.ascontiguousarray(n, np.int64)
        g = None if gain is None else np.ascontiguousarray(gain, np.float32)
        y = encoded_empty(e, rows, W)
        start, end = np.empty(rows, np.int64), np.empty(rows, np.int64)
        self._ck(self._lib.stn_op_silence_trim(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, float(top_db), float(keep_ms),
                                               float(fade_ms), None if g is None else g.ctypes.data, e, y.ctypes.data, start.ctypes.data,
                                               end.ctypes.data))
        return y, start, end

    def set_pause_limit(self, max_pause=None):
        """Shorten every pause inside an utterance that is longer than max_pause milliseconds ([20, 5000]) to max_pause, on the GPU at
        fetch time: None or False = off (the default).  It has effect only while silence trimming is on, and uses its parameters."""
        on, ms = pause_limit_args(max_pause)
        self._ck(self._lib.stn_set_pause_limit(self._h, on, ms))

    @property
    def pause_limit(self):
        """max_pause in milliseconds, or None when the limit is off."""
        on, ms = ctypes.c_int(), ctypes.c_float()
        self._ck(self._lib.stn_get_pause_limit(self._h, ctypes.byref(on), ctypes.byref(ms)))
        return ms.value if on.value else None

    def batch_pauses(self, cap_pairs=PAUSE_MAX_CUTS):
        """The finished batch as the current trimming parameters and max_pause cut it, either setting on or off -> (len [B] int64,
        n_cuts [B] int32, cuts [B, cap_pairs, 2] int64 as (lo, hi); pairs behind a row's n_cuts are -1)."""
        B = self.batch_dims()[0]
        ln, nc = np.empty(B, np.int64), np.empty(B, np.int32)
        cuts = np.full((B, max(int(cap_pairs), 1), 2), -1, np.int64)
        self._ck(self._lib.stn_batch_pauses(self._h, ln.ctypes.data, nc.ctypes.data, cuts.ctypes.data, cuts.shape[1]))
        return ln, nc, cuts

    def op_pause_trim(self, x, hz, n=None, top_db=40.0, keep_ms=TRIM_KEEP_MS, fade_ms=TRIM_FADE_MS, max_pause_ms=MAX_PAUSE_MS, gain=None, encoding=None,
                      cap_pairs=PAUSE_MAX_CUTS):
        """Detection, the pause limit's cuts and the store on the GPU -> dict(y [rows, W] in the encoding, start, end, len [rows] int64,
        n_cuts [rows] int32, cuts [rows, cap_pairs, 2] int64 with -1 behind a row's n_cuts): row r's segments end to end from column 0,
        times gain[r], cut edges faded, zero codewords behind len[r]."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        e = ENC_F32 if encoding is None else encoding_id(encoding)
        nn = None if n is None else np.ascontiguousarray(n, np.int64)
        g = None if gain is None else np.ascontiguousarray(gain, np.float32)
        y = encoded_empty(e, rows, W)
        start, end, ln = np.empty(rows, np.int64), np.empty(rows, np.int64), np.empty(rows, np.int64)
        nc = np.empty(rows, np.int32)
        cuts = np.full((rows, max(int(cap_pairs), 1), 2), -1, np.int64)
        self._ck(self._lib.stn_op_pause_trim(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, float(top_db), float(keep_ms),
                                             float(fade_ms), float(max_pause_ms), None if g is None else g.ctypes.data, e, y.ctypes.data,
                                             start.ctypes.data, end.ctypes.data, ln.ctypes.data, nc.ctypes.data, cuts.ctypes.data, cuts.shape[1]))
        return dict(y=y, start=start, end=end, len=ln, n_cuts=nc, cuts=cuts)

    def op_silence_edges_ex(self, x, hz, n=None, top_db=40.0, keep_ms=TRIM_KEEP_MS, fade_ms=TRIM_FADE_MS, max_pause_ms=0.0, x_misalign=0,
                            cap_pairs=PAUSE_MAX_CUTS):
        """The detection (and, with max_pause_ms > 0, the pause pass) with its scratch laid open (every 32-bit word 0x7FC00000 first) ->
        dict: pa, pb [rows, Ks] float32 (the chunks' two frame shares), lev [rows, Kf] float64 (the frame levels), start, end, len [rows]
        int64, n_cuts [rows] int32, cuts [rows, cap_pairs, 2] int64 with -1 behind a row's n_cuts, form ("vec" / "scalar": the staging
        path that ran).  x_misalign = 1 uploads x 4 bytes off 16-byte alignment."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        F = max((int(hz) + 50) // 100, 1)
        nn = None if n is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int64), (rows,)))
        o = dict(pa=np.empty((rows, (W + 31) // 32), np.float32), pb=np.empty((rows, (W + 31) // 32), np.float32),
                 lev=np.empty((rows, -(-W // F)), np.float64), start=np.empty(rows, np.int64), end=np.empty(rows, np.int64),
                 len=np.empty(rows, np.int64), n_cuts=np.empty(rows, np.int32), cuts=np.full((rows, max(int(cap_pairs), 1), 2), -1, np.int64))
        form = ctypes.create_string_buffer(16)
        self._ck(self._lib.stn_op_silence_edges_ex(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, float(top_db), float(keep_ms),
                                                   float(fade_ms), float(max_pause_ms), int(x_misalign),
                                                   *(o[k].ctypes.data for k in ("pa", "pb", "lev", "start", "end", "len", "n_cuts", "cuts")),
                                                   o["cuts"].shape[1], form, ctypes.sizeof(form)))
        o["form"] = form.value.decode()
        return o

    def set_limiter(self, lookahead_ms=None):
        """Look-ahead peak limiter behind the loudness gain: None = off (the default), True = 5 ms, or the look-ahead in milliseconds
        ([0.5, 10]).  With loudness on, every row then gets the full loudness gain and only the milliseconds around a sample above the
        ceiling are turned down; with loudness off it has no effect."""
        on, ms = limiter_args(lookahead_ms)
        self._ck(self._lib.stn_set_limiter(self._h, on, ms))

    @property
    def limiter(self):
        """The look-ahead in milliseconds, or None when the limiter is off."""
        on, ms = ctypes.c_int(), ctypes.c_float()
        self._ck(self._lib.stn_get_limiter(self._h, ctypes.byref(on), ctypes.byref(ms)))
        return ms.value if on.value else None

    def batch_limiter(self):
        """The finished batch as the current setting limits it -> (reduction_db [B] float32, limited [B] int64): the deepest reduction
        of each row and the samples of its span that are turned down (zeros while the limiter or loudness is off)."""
        B = self.batch_dims()[0]
        red, lim = np.empty(B, np.float32), np.empty(B, np.int64)
        self._ck(self._lib.stn_batch_limiter(self._h, red.ctypes.data, lim.ctypes.data))
        return red, lim

    def op_limiter(self, x, hz, n=None, gain=None, ceiling_dbfs=-1.0, lookahead_ms=LIMITER_MS):
        """rows x W fp32 at hz on the GPU, row r's first n[r] samples (None: all W) times gain[r] (None: 1), limited to ceiling_dbfs ->
        (y [rows, W], s [rows, W], reduction_db [rows], limited [rows])."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        nn = None if n is None else np.ascontiguousarray(n, np.int64)
        g = None if gain is None else np.ascontiguousarray(gain, np.float32)
        y, s = np.empty((rows, W), np.float32), np.empty((rows, W), np.float32)
        red, lim = np.empty(rows, np.float32), np.empty(rows, np.int64)
        self._ck(self._lib.stn_op_limiter(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, None if g is None else g.ctypes.data,
                                          float(ceiling_dbfs), float(lookahead_ms), y.ctypes.data, s.ctypes.data, red.ctypes.data, lim.ctypes.data))
        return y, s, red, lim

    def op_limiter_ex(self, x, hz, n=None, gain=None, ceiling_dbfs=-1.0, lookahead_ms=LIMITER_MS, peak_mode="true"):
        """op_limiter under a peak mode -> dict(y, s, env [rows, W], reduction_db, limited, trim [rows]): with "true" the curve follows
        the true-peak envelope env of x * gain, y is the limited row before the trim, and trim = min(1, c / true peak of y)."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        nn = None if n is None else np.ascontiguousarray(n, np.int64)
        g = None if gain is None else np.ascontiguousarray(gain, np.float32)
        o = dict(y=np.empty((rows, W), np.float32), s=np.empty((rows, W), np.float32), env=np.full((rows, W), np.nan, np.float32),
                 reduction_db=np.empty(rows, np.float32), limited=np.empty(rows, np.int64), trim=np.empty(rows, np.float32))
        mode = peak_mode if isinstance(peak_mode, int) else peak_mode_id(peak_mode)
        self._ck(self._lib.stn_op_limiter_ex(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, None if g is None else g.ctypes.data,
                                             float(ceiling_dbfs), float(lookahead_ms), o["y"].ctypes.data, o["s"].ctypes.data,
                                             o["reduction_db"].ctypes.data, o["limited"].ctypes.data, mode, o["env"].ctypes.data, o["trim"].ctypes.data))
        return o

    def set_peak_mode(self, mode="sample"):
        """The ceiling of set_loudness as a sample-peak ("sample", the default) or a true-peak ceiling ("true": 4x oversampled, ITU-R
        BS.1770-4 Annex 2).  With loudness off it has no effect."""
        self._ck(self._lib.stn_set_peak_mode(self._h, peak_mode_id(mode)))

    @property
    def peak_mode(self):
        """"sample" or "true"."""
        return "true" if self._ck_mode(self._lib.stn_get_peak_mode(self._h)) == PEAK_TRUE else "sample"

    def _ck_mode(self, rc):
        if rc < 0:
            self._ck(rc)
        return rc

    def batch_true_peak(self):
        """The finished batch at the output rate -> (tp_in, tp_out, trim) float32 [B]: the true peak of the measured row, of the fp32
        row as a fetch delivers it under the current settings, and the limiter's trim (1 except with the limiter in true mode)."""
        B = self.batch_dims()[0]
        a, b, t = np.empty(B, np.float32), np.empty(B, np.float32), np.empty(B, np.float32)
        self._ck(self._lib.stn_batch_true_peak(self._h, a.ctypes.data, b.ctypes.data, t.ctypes.data))
        return a, b, t

    def op_true_peak(self, x, hz, n=None, gain=None, x_misalign=0, env=True):
        """rows x W fp32 on the GPU, row r's first n[r] samples (None: all W) times gain[r] (None: 1) -> dict: tp [rows], env [rows, W]
        (the envelope; None when env is False), pk [rows, Ks] (per chunk of 32), form ("vec" / "scalar").  The device buffers are
        poisoned with the quiet NaN 0x7FC00000 first; x_misalign = 1 uploads x 4 bytes off 16-byte alignment."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        nn = None if n is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int64), (rows,)))
        g = None if gain is None else np.ascontiguousarray(gain, np.float32)
        o = dict(tp=np.empty(rows, np.float32), env=np.empty((rows, W), np.float32) if env else None, pk=np.empty((rows, (W + 31) // 32), np.float32))
        form = ctypes.create_string_buffer(16)
        self._ck(self._lib.stn_op_true_peak(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, None if g is None else g.ctypes.data,
                                            int(x_misalign), o["tp"].ctypes.data, None if o["env"] is None else o["env"].ctypes.data,
                                            o["pk"].ctypes.data, form, ctypes.sizeof(form)))
        o["form"] = form.value.decode()
        return o

    def dbg_batch_set_wav(self, wav):
        """Diagnostic: overwrite the finished batch's model-rate waveform ([B, L * chunk] float32) for tests that need known silences."""
        wav = np.ascontiguousarray(wav, np.float32)
        B, L, _ = self.batch_dims()
        a = StnArch()
        self._ck(self._lib.stn_get_arch(self._h, ctypes.byref(a)))
        W = L * a.base_chunk_size * a.chunk_compress_factor
        if wav.shape != (B, W):
            raise ValueError(f"dbg_batch_set_wav: wav must be [{B}, {W}], got {wav.shape}")
        self._ck(self._lib.stn_dbg_batch_set_wav(self._h, wav))

    def span_uploads(self):
        """Diagnostic: uploads of the finished batch's row spans since the handle was created (stn_dbg_span_uploads)."""
        return int(self._lib.stn_dbg_span_uploads(self._h))

    def set_pitch(self, semitones=None):
        """Shift the pitch of every row of every fetch by `semitones` on the GPU, in front of every other fetch-time stage and without
        a change of length (stn_set_pitch): None, False or 0 = off (the default).  ValueError with the engine's message for a value
        that is not finite or outside [-12, 12]; the previous setting then stays."""
        self._ck(self._lib.stn_set_pitch(self._h, pitch_args(semitones)))

    @property
    def pitch(self):
        """(semitones, a, b): the setting and the ratio it is realised with (0.0, 1, 1 when off)."""
        s, a, b = ctypes.c_float(), ctypes.c_int(), ctypes.c_int()
        self._ck(self._lib.stn_get_pitch(self._h, ctypes.byref(s), ctypes.byref(a), ctypes.byref(b)))
        return s.value, a.value, b.value

    def op_time_stretch(self, x, hz, a, b, n=None):
        """rows x W fp32 at hz, row r's span n[r] (None: W), stretched by a / b on the GPU (stn_op_time_stretch) -> (y [rows, Ws]
        float32, delta [rows, M] int32, score [rows, M] float32)."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        p = pitch_plan(hz, W, a, b)
        nn = None if n is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int64), (rows,)))
        y, d, sc = np.empty((rows, p["Ws"]), np.float32), np.empty((rows, p["M"]), np.int32), np.empty((rows, p["M"]), np.float32)
        self._ck(self._lib.stn_op_time_stretch(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, int(a), int(b), y.ctypes.data,
                                               d.ctypes.data, sc.ctypes.data))
        return y, d, sc

    def op_pitch(self, x, hz, semitones, n=None, mode=None):
        """rows x W fp32 at hz shifted by `semitones` on the GPU (stn_op_pitch: the stretch, then the resample back; mode="formant":
        stn_op_pitch_ex, the formant correction behind them) -> [rows, W]."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        nn = None if n is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int64), (rows,)))
        y = np.empty((rows, W), np.float32)
        if pitch_mode_id(mode) == PITCH_RESAMPLE:
            self._ck(self._lib.stn_op_pitch(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, float(semitones), y.ctypes.data))
        else:
            self._ck(self._lib.stn_op_pitch_ex(self._h, int(hz), rows, W, x, None if nn is None else nn.ctypes.data, float(semitones),
                                               pitch_mode_id(mode), y.ctypes.data))
        return y

    def set_pitch_mode(self, mode="resample"):
        """What set_pitch delivers (stn_set_pitch_mode): "resample" (the default: formants move with the pitch) or "formant" (the
        spectral envelope of the rows before the shift is put back onto the shifted rows on the GPU).  With pitch off it has no effect."""
        self._ck(self._lib.stn_set_pitch_mode(self._h, pitch_mode_id(mode)))

    @property
    def pitch_mode(self):
        """"resample" or "formant"."""
        return PITCH_MODE_NAMES[self._ck_mode(self._lib.stn_get_pitch_mode(self._h))]

    def op_formant(self, x, y, hz, n=None, ex=False):
        """The formant correction on the caller's rows (stn_op_formant): x (before the shift) and y (shifted), rows x W fp32 at hz, row
        r's span n[r] (None: W) -> out [rows, W].  ex=True (stn_op_formant_ex) -> dict out, ax and cy [rows, frames, p + 1] float32,
        g, ex and ey [rows, frames] float64, and guard_ok."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        y = np.ascontiguousarray(np.atleast_2d(y), np.float32)
        if x.shape != y.shape:
            raise ValueError(f"op_formant: x {x.shape} and y {y.shape} must have one shape")
        rows, W = x.shape
        nn = None if n is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int64), (rows,)))
        np_ = None if nn is None else nn.ctypes.data
        out = np.empty((rows, W), np.float32)
        if not ex:
            self._ck(self._lib.stn_op_formant(self._h, int(hz), rows, W, x, y, np_, out.ctypes.data))
            return out
        p = formant_plan(hz, W)
        o = dict(out=out, ax=np.empty((rows, p["frames"], p["p"] + 1), np.float32), cy=np.empty((rows, p["frames"], p["p"] + 1), np.float32),
                 g=np.empty((rows, p["frames"]), np.float64), ex=np.empty((rows, p["frames"]), np.float64), ey=np.empty((rows, p["frames"]), np.float64))
        ok = ctypes.c_int()
        self._ck(self._lib.stn_op_formant_ex(self._h, int(hz), rows, W, x, y, np_, out.ctypes.data, o["ax"].ctypes.data, o["cy"].ctypes.data,
                                             o["g"].ctypes.data, o["ex"].ctypes.data, o["ey"].ctypes.data, ctypes.byref(ok)))
        o["guard_ok"] = bool(ok.value)
        return o

    def set_dither(self, dither=None, seed=None):
        """How the 16- and 24-bit PCM stores of every fetch quantize (stn_set_dither): None / False / "off" (the default: truncation),
        "round", "tpdf" (True) or "tpdf-hp", as dither_args takes them; seed keys the noise, with the utterance id (per-row fetches)
        or the programme index (joined fetches) and the sample index.  fp32, mu-law and A-law fetches are unaffected."""
        mode, seed = dither_args(dither, seed) or ("off", 0)
        self._ck(self._lib.stn_set_dither(self._h, DITHER_MODES[mode], seed))

    @property
    def dither(self):
        """None (off) or (mode name, seed)."""
        seed = ctypes.c_uint64()
        mode = self._ck_mode(self._lib.stn_get_dither(self._h, ctypes.byref(seed)))
        return None if mode == DITHER_OFF else (DITHER_NAMES[mode], seed.value)

    def op_encode_ex(self, x, enc, dither="off", seed=0, gain=None, row_id=None, dst_stride=None, x_misalign=0, fill=0x5A):
        """op_encode with the store's other arguments (stn_op_encode_ex) -> samples [rows, dst_stride] (encoded_empty's dtypes): times
        gain [rows], row r's dither stream (0, row_id[r]) (None: r), rows dst_stride (None: W) samples apart in a buffer that goes in
        as bytes `fill`, x placed x_misalign floats off 16-byte alignment on the device."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        e = encoding_id(enc)
        stride = W if dst_stride is None else int(dst_stride)
        out = encoded_empty(e, rows, stride)
        out.view(np.uint8)[...] = fill
        g = None if gain is None else np.ascontiguousarray(gain, np.float32)
        ids = None if row_id is None else np.ascontiguousarray(row_id, np.int64)
        self._ck(self._lib.stn_op_encode_ex(self._h, e, rows, W, x, int(x_misalign), None if g is None else g.ctypes.data,
                                            None if ids is None else ids.ctypes.data, dither_mode_id(dither), int(seed), stride, out.ctypes.data))
        return out

    def op_encode(self, x, enc):
        """rows x W fp32 -> rows x W samples of an encoding on the GPU (the fetch's store kernel without a gain; encoded_empty's dtypes)."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        rows, W = x.shape
        e = encoding_id(enc)
        out = encoded_empty(e, rows, W)
        self._ck(self._lib.stn_op_encode(self._h, e, rows, W, x, out.ctypes.data))
        return out

    def batch_fetch_encoded(self, enc):
        """The finished batch in an encoding -> (samples [B, W] (encoded_empty's dtypes), duration [B])."""
        e = encoding_id(enc)
        B, _, W = self.batch_dims()
        out, dur = encoded_empty(e, B, W), np.empty(B, np.float32)
        self._ck(self._lib.stn_batch_fetch_encoded(self._h, e, out.ctypes.data, out.nbytes, dur.ctypes.data))
        return out, dur

    def batch_join_dims(self, rows, gap_samples, gap_seconds, mode="whole", gain_scope="row"):
        """The finished batch's plan under a join -> (W_join, prog_len [G] int64, prog_dur [G] float32)."""
        j, keep = _join(rows, gap_samples, gap_seconds, mode, gain_scope)
        G = keep[0].size
        wj, prog_len, prog_dur = ctypes.c_int64(), np.zeros(G, np.int64), np.zeros(G, np.float32)
        self._ck(self._lib.stn_batch_join_dims(self._h, ctypes.byref(j), ctypes.byref(wj), prog_len.ctypes.data, prog_dur.ctypes.data))
        return wj.value, prog_len, prog_dur

    def batch_fetch_joined(self, rows, gap_samples, gap_seconds, mode="whole", gain_scope="row", encoding=None, cut=True):
        """Consecutive rows of the finished batch joined on the GPU into len(rows) programmes (rows[g] members each, gap_samples[g] samples
        of silence between two members, gap_seconds[g] added to the duration per gap) -> (list of G arrays cut at prog_len, prog_dur [G]);
        cut=False: (the padded [G, W_join] array, prog_len, prog_dur).  mode "whole" | "trim", gain_scope "row" | "programme" (with
        loudness normalization on: one gain per member row, or one per programme measured as a whole).  encoding: as batch_fetch_encoded
        (None: float32)."""
        e = ENC_F32 if encoding is None else encoding_id(encoding)
        j, keep = _join(rows, gap_samples, gap_seconds, mode, gain_scope)
        G = keep[0].size
        wj, prog_len, prog_dur = ctypes.c_int64(), np.zeros(G, np.int64), np.zeros(G, np.float32)
        self._ck(self._lib.stn_batch_join_dims(self._h, ctypes.byref(j), ctypes.byref(wj), None, None))
        out = encoded_empty(e, G, wj.value)
        self._ck(self._lib.stn_batch_fetch_joined(self._h, ctypes.byref(j), e, out.ctypes.data, out.nbytes, prog_len.ctypes.data, prog_dur.ctypes.data))
        if not cut:
            return out, prog_len, prog_dur
        return [out[g, : int(prog_len[g])] for g in range(G)], prog_dur

    def fetch_joined_begin(self, slot, rows, gap_samples, gap_seconds, mode="whole", gain_scope="row", encoding=None):
        """fetch_encoded_begin of the joined rows; ended by fetch_encoded_end -> (samples [G, W_join], prog_dur [G])."""
        e = ENC_F32 if encoding is None else encoding_id(encoding)
        j, _keep = _join(rows, gap_samples, gap_seconds, mode, gain_scope)
        self._ck(self._lib.stn_batch_fetch_joined_begin(self._h, int(slot), ctypes.byref(j), e))
        self._slot_enc[int(slot)] = e

    def batch_copy_joined_device(self, rows, gap_samples, gap_seconds, dst_ptr, dst_stride, mode="whole", gain_scope="row", encoding=None):
        """Device->device copy of the joined rows in an encoding; dst_stride in samples (>= W_join)."""
        e = ENC_F32 if encoding is None else encoding_id(encoding)
        j, _keep = _join(rows, gap_samples, gap_seconds, mode, gain_scope)
        self._ck(self._lib.stn_batch_copy_joined_device(self._h, ctypes.byref(j), e, dst_ptr, dst_stride))

    def batch_join_loudness(self, rows, gap_samples, gap_seconds, mode="whole"):
        """The joined signal measured as programmes -> (lufs [G], peak [G], gain [G]); gain: what gain_scope="programme" applies."""
        j, keep = _join(rows, gap_samples, gap_seconds, mode, JOIN_GAIN_PROG)
        G = keep[0].size
        lufs, peak, gain = (np.empty(G, np.float32) for _ in range(3))
        self._ck(self._lib.stn_batch_join_loudness(self._h, ctypes.byref(j), lufs.ctypes.data, peak.ctypes.data, gain.ctypes.data))
        return lufs, peak, gain

    def op_join(self, x, n, rows, gap_samples, hz, encoding=None, loudness=None, measure=False):
        """rows x W fp32 at hz, row r's first n[r] samples member r's segment, joined on the GPU -> y [G, W_join] in the encoding
        (encoded_empty's dtypes).  loudness = (target LUFS, ceiling dBFS): every programme normalized as a whole; then, or with
        measure=True, returns (y, lufs [G], peak [G], gain [G])."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        R, W = x.shape
        nn = np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int64), (R,)))
        e = ENC_F32 if encoding is None else encoding_id(encoding)
        j, keep = _join(rows, gap_samples, 0.0)
        G = keep[0].size
        plan = join_plan(rows, gap_samples, 0.0, nn, np.zeros(R, np.float32), W, hz)
        y = encoded_empty(e, G, plan["W_join"])
        lufs, peak, gain = (np.empty(G, np.float32) for _ in range(3))
        want = loudness is not None or measure
        t, c = loudness if loudness is not None else (-23.0, -1.0)
        self._ck(self._lib.stn_op_join(self._h, int(hz), R, W, x, nn, ctypes.byref(j), e, int(loudness is not None), float(t), float(c), y.ctypes.data,
                                       lufs.ctypes.data if want else None, peak.ctypes.data if want else None, gain.ctypes.data if want else None))
        return (y, lufs, peak, gain) if want else y

    def fetch_encoded_begin(self, slot, enc):
        """fetch_pcm16_begin in an encoding."""
        e = encoding_id(enc)
        self._ck(self._lib.stn_batch_fetch_encoded_begin(self._h, int(slot), e))
        self._slot_enc[int(slot)] = e

    def fetch_encoded_end(self, slot, copy=True):
        """Wait for the slot's copy -> (samples [B, W] in the slot's encoding, duration [B]); copy=False: a view of the pinned buffer."""
        B, W = ctypes.c_int(), ctypes.c_int64()
        self._ck(self._lib.stn_batch_fetch_slot_dims(self._h, int(slot), ctypes.byref(B), ctypes.byref(W)))
        ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
        dur = np.empty(B.value, np.float32)
        self._ck(self._lib.stn_batch_fetch_encoded_end(self._h, int(slot), ctypes.byref(ptr), ctypes.byref(n), dur.ctypes.data))
        like = encoded_empty(self._slot_enc.get(int(slot), ENC_PCM16), B.value, W.value)
        assert like.nbytes == n.value, (like.shape, n.value)
        raw = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(n.value,))
        arr = raw.view(like.dtype).reshape(like.shape)
        return (arr.copy() if copy else arr), dur

    def batch_copy_encoded_device(self, enc, dst_ptr, dst_stride):
        """Device->device copy of the finished batch in an encoding; dst_stride in samples."""
        self._ck(self._lib.stn_batch_copy_encoded_device(self._h, encoding_id(enc), dst_ptr, dst_stride))

    def fetch_pcm16_begin(self, slot):
        """Start the PCM conversion + device->host copy of the finished batch on `slot` (0/1); returns at once."""
        self._ck(self._lib.stn_batch_fetch_pcm16_begin(self._h, int(slot)))
        self._slot_enc[int(slot)] = ENC_PCM16

    def fetch_pcm16_end(self, slot, copy=True):
        """Wait for the slot's copy -> (pcm [B, W] int16, duration [B]).  copy=False returns a view of the handle's pinned buffer
        (valid until the slot's next fetch_pcm16_begin)."""
        B, W = ctypes.c_int(), ctypes.c_int64()
        self._ck(self._lib.stn_batch_fetch_slot_dims(self._h, int(slot), ctypes.byref(B), ctypes.byref(W)))  # the slot's batch, not the resident one
        ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
        dur = np.empty(B.value, np.float32)
        self._ck(self._lib.stn_batch_fetch_pcm16_end(self._h, int(slot), ctypes.byref(ptr), ctypes.byref(n), dur.ctypes.data))
        arr = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int16)), shape=(n.value,))
        rows = n.value // max(dur.size, 1)
        arr = arr.reshape(dur.size, rows)
        return (arr.copy() if copy else arr), dur

    @property
    def graph_replays(self):
        return self._lib.stn_graph_replays(self._h)

    @property
    def graphs_cached(self):
        return self._lib.stn_graphs_cached(self._h)

    def batch_dims(self):
        B, L, W = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        self._ck(self._lib.stn_batch_dims(self._h, ctypes.byref(B), ctypes.byref(L), ctypes.byref(W)))
        return B.value, L.value, W.value

    def batch_fetch(self, want_wav=True):
        B, L, W = self.batch_dims()
        dur = np.empty(B, np.float32)
        wav = np.empty((B, W), np.float32) if want_wav else None
        self._ck(self._lib.stn_batch_fetch(self._h, wav.ctypes.data if want_wav else None, B * W if want_wav else 0,
                                           dur.ctypes.data))
        return wav, dur

    def batch_fetch_pcm16(self):
        B, L, W = self.batch_dims()
        pcm = np.empty((B, W), np.int16)
        dur = np.empty(B, np.float32)
        self._ck(self._lib.stn_batch_fetch_pcm16(self._h, pcm.ctypes.data, B * W, dur.ctypes.data))
        return pcm, dur

    def batch_fetch_latent(self):
        B, L, _ = self.batch_dims()
        out = np.empty((B, self.arch.latent_channels, L), np.float32)
        self._ck(self._lib.stn_batch_fetch_latent(self._h, out))
        return out

    def batch_wav_device_ptr(self):
        p = ctypes.c_void_p()
        self._ck(self._lib.stn_batch_wav_device_ptr(self._h, ctypes.byref(p)))
        return p.value

    def sync(self):
        self._ck(self._lib.stn_sync(self._h))

    def set_stream(self, hip_stream_ptr):
        """Enqueue on a caller-owned HIP stream (int pointer, e.g. torch.cuda.current_stream().cuda_stream)."""
        self._ck(self._lib.stn_set_stream(self._h, hip_stream_ptr))

    def batch_copy_pcm16_device(self, dst_ptr, dst_stride):
        self._ck(self._lib.stn_batch_copy_pcm16_device(self._h, dst_ptr, dst_stride))

    def batch_copy_wav_device(self, dst_ptr, dst_stride):
        self._ck(self._lib.stn_batch_copy_wav_device(self._h, dst_ptr, dst_stride))

    def synthesize(self, text_ids, text_mask, style_ttl, style_dp, total_step=5, speed=1.05, noise=None,
                   duration_override=None, noise_seed=1234, utt_ids=None):
        """TextToSpeech::_infer (/root/reference/cpp/helper.cpp:469-683) -> (wav [B, L*cs], duration [B])."""
        self.batch_upload(text_ids, text_mask, style_ttl, style_dp, duration_override, utt_ids)
        if noise is not None:
            self.batch_set_noise(noise)
        self.batch_run(total_step, speed, noise_seed)
        return self.batch_fetch()

    # ---- measurement -----------------------------------------------------------------------------------
    def xattn_hs_stamps_enable(self, on=True):
        self._ck(self._lib.stn_dbg_xattn_hs_enable(self._h, int(bool(on))))

    def xattn_hs_stamps(self):
        """[workgroups, 8] shader-clock stamps of the last head-split cross-attention launch (diagnostics)."""
        n = int(self._lib.stn_dbg_xattn_hs_stamps(self._h, None, 0))
        out = np.zeros((max(n, 0), 8), np.uint64)
        if n > 0:
            self._lib.stn_dbg_xattn_hs_stamps(self._h, out.ctypes.data, out.size)
        return out

    def profile_enable(self, on=True):
        self._ck(self._lib.stn_profile_enable(self._h, int(on)))

    def profile_filter(self, family=None):
        self._ck(self._lib.stn_profile_filter(self._h, family.encode() if family else None))

    def launch_log_enable(self, on=True):
        self._ck(self._lib.stn_launch_log_enable(self._h, int(bool(on))))

    def launch_log(self):
        """[(family, kernel)] of every launch since the last profile_reset (profiling on, log enabled), in dispatch order."""
        n = self._lib.stn_launch_log(self._h, None, 0)
        if n < 0:
            self._ck(int(n))
        buf = ctypes.create_string_buffer(int(n) + 1)
        self._lib.stn_launch_log(self._h, buf, int(n) + 1)
        return [tuple(l.split("\t")) for l in buf.value.decode().splitlines()]

    def profile_sample(self, every=1):
        self._ck(self._lib.stn_profile_sample(self._h, int(every)))

    def profile_reset(self):
        self._ck(self._lib.stn_profile_reset(self._h))

    def profile(self):
        """{kernel family: dict(ms, launches, flops, bytes)} measured with HIP events on the engine's stream."""
        n = self._ck(self._lib.stn_profile_count(self._h))
        out = {}
        name = ctypes.create_string_buffer(64)
        ms, fl, by, la = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        for i in range(n):
            self._ck(self._lib.stn_profile_get(self._h, i, name, 64, ctypes.byref(ms), ctypes.byref(la),
                                               ctypes.byref(fl), ctypes.byref(by)))
            out[name.value.decode()] = dict(ms=ms.value, launches=la.value, flops=fl.value, bytes=by.value)
        return out

    # ---- op-level (kernel parity tests) ----------------------------------------------------------------
    def op_gemm(self, A, W, bias=None, act=ACT_NONE, dtype=None):
        M, K = A.shape
        N = W.shape[0]
        out = np.empty((M, N), np.float32)
        _b, bptr = _opt(bias, np.float32)
        self._ck(self._lib.stn_op_gemm(self._h, self.dtype if dtype is None else _DTYPES[dtype], M, N, K,
                                       _c(A, np.float32), _c(W, np.float32), bptr, act, out))
        return out

    def op_gemm_ex(self, A, W, out, mode=EPI_STORE, act=ACT_NONE, out_dtype="f32", ldo=None, bias=None, gamma=None, len=None, L=1,
                   row_b=None, rowvec=None, nt=0, tr=-1, dtype=None):
        """One GEMM through the engine's launcher with the given epilogue (stn_op_gemm_ex).  `out` is the whole destination buffer (the residual
        for EPI_RESID): a copy goes up, the result comes back as a new fp32 array of the same shape.  len / rowvec: one entry / row per sequence.
        Returns (result, form string)."""
        M, K = A.shape
        N = W.shape[0]
        res = np.array(out, dtype=np.float32, order="C", copy=True)
        nseq = 0
        for v in (len, rowvec):
            if v is not None:
                nseq = max(nseq, np.asarray(v).shape[0])
        if row_b is not None and rowvec is None:
            nseq = max(nseq, int(np.max(row_b)) + 1)
        _b, bp = _opt(bias, np.float32)
        _g, gp = _opt(gamma, np.float32)
        _l, lp = _opt(len, np.int32)
        _r, rp = _opt(row_b, np.int32)
        _v, vp_ = _opt(rowvec, np.float32)
        form = ctypes.create_string_buffer(128)
        self._ck(self._lib.stn_op_gemm_ex(self._h, self.dtype if dtype is None else _DTYPES[dtype], M, N, K, _c(A, np.float32), _c(W, np.float32),
                                          int(mode), int(act), _DTYPES[out_dtype], int(N if ldo is None else ldo), bp, gp, lp, int(L), rp, vp_, nseq,
                                          int(nt), int(tr), res.reshape(-1), res.size, form, ctypes.sizeof(form)))
        return res, form.value.decode()

    def op_gemm_bench(self, M, N, K, mode=0, iters=20, dtype=None):
        ms = ctypes.c_double()
        self._ck(self._lib.stn_op_gemm_bench(self._h, self.dtype if dtype is None else _DTYPES[dtype], M, N, K, mode,
                                             iters, ctypes.byref(ms)))
        return ms.value

    def op_ffn(self, xn, W1, b1, W2, b2, gamma, x, rowvec=None, row_b=None, fused=True):
        """Pointwise pair of a ConvNeXt block (K4): returns x + gamma * (W2 . GELU(W1 . xn + b1) + b2) [+ rowvec[row_b]]."""
        M, C = xn.shape
        I = W1.shape[0]
        out = np.array(x, dtype=np.float32, order="C", copy=True)
        _, b2p = _opt(b2, np.float32)
        b2a = _opt(b2, np.float32)[0]
        ga, gp = _opt(gamma, np.float32)
        rva, rvp = _opt(rowvec, np.float32)
        rba, rbp = _opt(row_b, np.int32)
        b2p = b2a.ctypes.data if b2a is not None else None
        self._ck(self._lib.stn_op_ffn(self._h, M, C, I, _c(xn, np.float32), _c(W1, np.float32), _c(b1, np.float32), _c(W2, np.float32),
                                      b2p, gp, rvp, rbp, 0 if rva is None else rva.shape[0], out, int(fused)))
        return out

    def op_ffn_ex(self, xn, W1, b1, W2, x, mode=1, b2=None, gamma=None, len=None, L=None, row_b=None, rowvec=None, split=0, part=None,
                  part_stride=0, M=None, dtype=None):
        """The pointwise pair through the engine's own launch on whole buffers (stn_op_ffn_ex).  xn [rows, ldx] and x [rows, ldo] are 2-D with
        the launch's C = W1.shape[1] columns first; M (default: xn's rows) rows run.  len [nseq] with L, row_b [M], rowvec [nseq, rv_ld].
        mode 0 two launches, 1 K4, 2 K4-split with `split` ways (0: the launcher's choice), which stops at the partial sums: part is the
        whole buffer (any shape), its shares part_stride elements apart.  Returns (x, part or None, form string), x and part as new arrays."""
        xn = _c(xn, np.float32)
        I, C = W1.shape
        M = xn.shape[0] if M is None else int(M)
        x_r = np.array(x, dtype=np.float32, order="C", copy=True)
        p_r = None if part is None else np.array(part, dtype=np.float32, order="C", copy=True)
        nseq = 0
        for v in (len, rowvec):
            if v is not None:
                nseq = max(nseq, np.asarray(v).shape[0])
        if row_b is not None and rowvec is None:
            nseq = max(nseq, int(np.max(row_b)) + 1)
        _b, bp = _opt(b2, np.float32)
        _g, gp = _opt(gamma, np.float32)
        _l, lp = _opt(len, np.int32)
        _r, rp = _opt(row_b, np.int32)
        _v, vp_ = _opt(rowvec, np.float32)
        form = ctypes.create_string_buffer(32)
        self._ck(self._lib.stn_op_ffn_ex(self._h, self.dtype if dtype is None else _DTYPES[dtype], M, C, I, xn.reshape(-1), xn.shape[1], xn.size,
                                         _c(W1, np.float32), _c(b1, np.float32), _c(W2, np.float32), bp, gp, lp, int(M if L is None else L), rp, vp_,
                                         C if _v is None else _v.shape[1], nseq, int(mode), int(split), x_r.reshape(-1), x_r.shape[1], x_r.size,
                                         None if p_r is None else p_r.ctypes.data, int(part_stride), 0 if p_r is None else p_r.size, form,
                                         ctypes.sizeof(form)))
        return x_r, p_r, form.value.decode()

    def op_ffn_bench(self, M, C, I, fused=True, iters=20):
        """fused: 0 / False two launches, 1 / True K4, 2 K4-split (partial sums only; the fold is part of op_block_bench)."""
        out = (ctypes.c_double * 5)()
        self._ck(self._lib.stn_op_ffn_bench(self._h, M, C, I, int(fused), iters, out))
        return dict(ms=out[0], first_stage=out[1], tile_loop=out[2], epilogue=out[3], workgroups=int(out[4]))

    def op_fold_dwconv_ln(self, seqlen, x, part, b2, gamma, rowvec, w, bias, g, b, k, dil):
        """fold + depthwise conv + LayerNorm on packed rows -> (x_out, y)."""
        seqlen = np.ascontiguousarray(seqlen, np.int32)
        S, M, C = part.shape
        xo = np.empty((M, C), np.float32)
        y = np.empty((M, C), np.float32)
        b2a, _ = _opt(b2, np.float32)
        ga, _ = _opt(gamma, np.float32)
        rva, _ = _opt(rowvec, np.float32)
        p = lambda a: None if a is None else a.ctypes.data
        self._ck(self._lib.stn_op_fold_dwconv_ln(self._h, len(seqlen), C, k, dil, S, seqlen, _c(x, np.float32), _c(part, np.float32), p(b2a), p(ga), p(rva),
                                                 _c(w, np.float32), _c(bias, np.float32), _c(g, np.float32), _c(b, np.float32), xo, y))
        return xo, y

    def op_fold_dwconv_ln_ex(self, seqlen, L, x_in, part, part_stride, S, b2, gamma, rowvec, w, bias, g, b, dil, x_out, y, run_frames=0, dtype=None):
        """launch_fold_dwconv_ln on whole buffers (stn_op_fold_dwconv_ln_ex).  x_in, x_out, y: 2-D [rows, C]; part: flat, split s at
        s * part_stride; rowvec [B, rv_ld] or None; w [C, k].  Returns (x_out, y as new fp32 arrays, whole; form string)."""
        seqlen = _c(seqlen, np.int32)
        x_in = _c(x_in, np.float32)
        part = _c(part, np.float32).reshape(-1)
        xo = np.array(x_out, dtype=np.float32, order="C", copy=True)
        yo = np.array(y, dtype=np.float32, order="C", copy=True)
        C = x_in.shape[1]
        w = _c(w, np.float32)
        _b2, b2p = _opt(b2, np.float32)
        _g, gp = _opt(gamma, np.float32)
        _v, vp_ = _opt(rowvec, np.float32)
        form = ctypes.create_string_buffer(96)
        self._ck(self._lib.stn_op_fold_dwconv_ln_ex(self._h, self.dtype if dtype is None else _DTYPES[dtype], len(seqlen), int(L), C, w.shape[1], int(dil),
                                                    int(S), int(run_frames), seqlen, x_in.reshape(-1), x_in.shape[0], part, int(part_stride), part.size,
                                                    b2p, gp, vp_, C if _v is None else _v.shape[1], w, _c(bias, np.float32), _c(g, np.float32),
                                                    _c(b, np.float32), xo.reshape(-1), xo.shape[0], yo.reshape(-1), yo.shape[0], form, ctypes.sizeof(form)))
        return xo, yo, form.value.decode()

    def op_block_bench(self, B, L, C, I, k, dil, mode, iters=20):
        out = (ctypes.c_double * 6)()
        self._ck(self._lib.stn_op_block_bench(self._h, B, L, C, I, k, dil, mode, iters, out))
        return dict(ms=out[0], conv_ms=out[1], fold_phase1=out[2], fold_barrier=out[3], fold_phase2=out[4], fold_span=out[5])

    def set_fused_ffn_min_rows(self, k4_rows=-1, split_rows=-1):
        self._ck(self._lib.stn_set_fused_ffn_min_rows(self._h, int(k4_rows), int(split_rows)))

    def op_gemm_phases(self, M, N, K, mode=0, dtype=None):
        out = (ctypes.c_double * 6)()
        self._ck(self._lib.stn_op_gemm_phases(self._h, self.dtype if dtype is None else _DTYPES[dtype], M, N, K, mode, out))
        return dict(first_stage=out[0], k_loop=out[1], epilogue=out[2], grid_span=out[3], entry_spread=out[4], workgroups=int(out[5]))

    def op_dwconv_ln(self, x, w, bias, g, b, dil, dtype=None, seqlen=None):
        B, L, C = x.shape
        k = w.shape[1]
        y = np.empty((B, L, C), np.float32)
        if seqlen is not None:
            self._ck(self._lib.stn_op_dwconv_ln_ragged(self._h, self.dtype if dtype is None else _DTYPES[dtype], B, L, C, k,
                                                       dil, _c(x, np.float32), _c(w, np.float32), _c(bias, np.float32),
                                                       _c(g, np.float32), _c(b, np.float32), _c(seqlen, np.int32), y))
            return y
        self._ck(self._lib.stn_op_dwconv_ln(self._h, self.dtype if dtype is None else _DTYPES[dtype], B, L, C, k, dil,
                                            _c(x, np.float32), _c(w, np.float32), _c(bias, np.float32),
                                            _c(g, np.float32), _c(b, np.float32), y))
        return y

    def op_gemm_rows(self, A, W, out, rows, valid, T, bias=None, dtype=None):
        """One GEMM whose packed rows are stored through the destination map (stn_op_gemm_rows).  A [M, K], W [N, K]; sequence b owns rows[b]
        consecutive rows of A; out: the whole [B, T, N] destination (plus any guard), uploaded as given.  Returns (out as a new fp32 array, form)."""
        A = _c(A, np.float32)
        W = _c(W, np.float32)
        rows = _c(rows, np.int32)
        valid = _c(valid, np.int32)
        o_r = np.array(out, dtype=np.float32, order="C", copy=True)
        _b, bp = _opt(bias, np.float32)
        form = ctypes.create_string_buffer(96)
        self._ck(self._lib.stn_op_gemm_rows(self._h, self.dtype if dtype is None else _DTYPES[dtype], A.shape[0], W.shape[0], A.shape[1],
                                            A.reshape(-1), W.reshape(-1), bp, len(rows), rows, valid, int(T), o_r.reshape(-1), o_r.size, form,
                                            ctypes.sizeof(form)))
        return o_r, form.value.decode()

    def op_dwconv_ln_ex(self, x, w, bias, g, b, dil, out, B, L, seqlen=None, packed=False, ln_only=False, dtype=None):
        """launch_dwconv_ln (ln_only: launch_layernorm over B*L rows) on whole buffers (stn_op_dwconv_ln_ex).  x, out: 2-D [rows, C], x
        uploaded as given; packed: sequence b owns seqlen[b] consecutive rows.  w [C, k] (None with ln_only).  Returns (out as a new fp32
        array, whole; form string)."""
        x = _c(x, np.float32)
        o_r = np.array(out, dtype=np.float32, order="C", copy=True)
        C = x.shape[1]
        _w, wp = _opt(w, np.float32)
        _b, bp = _opt(bias, np.float32)
        _l, lp = _opt(seqlen, np.int32)
        form = ctypes.create_string_buffer(32)
        self._ck(self._lib.stn_op_dwconv_ln_ex(self._h, self.dtype if dtype is None else _DTYPES[dtype], int(B), int(L), C,
                                               1 if _w is None else _w.shape[1], int(dil), x.reshape(-1), x.shape[0], wp, bp, _c(g, np.float32),
                                               _c(b, np.float32), lp, int(bool(packed)), int(bool(ln_only)), o_r.reshape(-1), o_r.shape[0], form,
                                               ctypes.sizeof(form)))
        return o_r, form.value.decode()

    def op_dwconv_ln_tail(self, x, w, bias, g, b, dil, out, L, seqlen, tail, T, dtype=None):
        """The tail-reading variant of the packed launch_dwconv_ln (stn_op_dwconv_ln_tail): sequence i owns seqlen[i] consecutive rows of x / out
        and is the head of a row of T >= L frames; a tap at a frame tt >= seqlen[i] reads tail[min(T - 1 - tt, rf)] (tail [rf + 1, C]) and
        zero from T on.  Returns (out as a new fp32 array, whole; form string)."""
        x = _c(x, np.float32)
        tail = _c(tail, np.float32)
        o_r = np.array(out, dtype=np.float32, order="C", copy=True)
        C = x.shape[1]
        w = _c(w, np.float32)
        seqlen = _c(seqlen, np.int32)
        assert tail.ndim == 2 and tail.shape[1] == C and tail.shape[0] >= 1
        form = ctypes.create_string_buffer(32)
        self._ck(self._lib.stn_op_dwconv_ln_tail(self._h, self.dtype if dtype is None else _DTYPES[dtype], len(seqlen), int(L), C, w.shape[1],
                                                 int(dil), x.reshape(-1), x.shape[0], w, _c(bias, np.float32), _c(g, np.float32),
                                                 _c(b, np.float32), seqlen, tail.reshape(-1), int(T), tail.shape[0] - 1, o_r.reshape(-1),
                                                 o_r.shape[0], form, ctypes.sizeof(form)))
        return o_r, form.value.decode()

    def op_fold_ln(self, x, part, b2, gamma, g, b, rowvec=None, row_b=None, dtype=None):
        """launch_fold_ln on host operands (stn_op_fold_ln).  x [M, C], part [S, M, C] (rounded to the 16-bit dtype first), rowvec [nseq, C].
        Returns (updated x, LayerNorm output as fp32)."""
        x_r = np.array(x, dtype=np.float32, order="C", copy=True)
        M, C = x_r.shape
        part = _c(part, np.float32)
        y = np.empty((M, C), np.float32)
        _v, vp_ = _opt(rowvec, np.float32)
        _r, rp = _opt(row_b, np.int32)
        self._ck(self._lib.stn_op_fold_ln(self._h, self.dtype if dtype is None else _DTYPES[dtype], M, C, part.shape[0], part.reshape(-1),
                                          _c(b2, np.float32), _c(gamma, np.float32), vp_, rp, 0 if _v is None else _v.shape[0],
                                          _c(g, np.float32), _c(b, np.float32), x_r, y))
        return x_r, y

    def op_layout(self, which, p, a=None, b=None, c=None, ids=None, length=None, packed=False, out=None, out2=None, iout=None, dtype="f32"):
        """One layout kernel of kernels_layout.hip on host operands (stn_op_layout; LAYOUT_* and the parameter lists: include/stn.h).
        out / out2 (float32) and iout (int32) are whole destination buffers; they come back as new arrays (out, out2, iout)."""
        def f32(v):
            return (None, None, 0) if v is None else (lambda arr: (arr, arr.ctypes.data, arr.size))(_c(v, np.float32))
        pa = _c(p, np.int32)
        _a, ap, an = f32(a)
        _b, bp, bn = f32(b)
        _cc, cp, cn = f32(c)
        _i, ip = _opt(ids, np.int64)
        _l, lp = _opt(length, np.int32)
        o1 = None if out is None else np.array(out, dtype=np.float32, order="C", copy=True)
        o2 = None if out2 is None else np.array(out2, dtype=np.float32, order="C", copy=True)
        io = None if iout is None else np.array(iout, dtype=np.int32, order="C", copy=True)
        ptr = lambda v: (None, 0) if v is None else (v.ctypes.data, v.size)  # noqa: E731
        self._ck(self._lib.stn_op_layout(self._h, int(which), _DTYPES[dtype], pa, len(pa), ap, an, bp, bn, cp, cn, ip, 0 if _i is None else _i.size,
                                         lp, int(bool(packed)), *ptr(o1), *ptr(o2), *ptr(io)))
        return o1, o2, io

    def op_attention(self, q, k, v, H, qlen=None, klen=None, rope_mode=-1, dtype=None):
        B, Lq, C = q.shape
        Lk = k.shape[1]
        o = np.empty((B, Lq, C), np.float32)
        _q, qp = _opt(qlen, np.int32)
        _k, kp = _opt(klen, np.int32)
        self._ck(self._lib.stn_op_attention(self._h, self.dtype if dtype is None else _DTYPES[dtype], B, Lq, Lk, H,
                                            C // H, _c(q, np.float32), _c(k, np.float32), _c(v, np.float32), qp, kp,
                                            rope_mode, o))
        return o

    def op_attention_ex(self, q, kv, out, B, Lq, Lk, H, dh, q_col=0, k_col=0, v_col=None, qlen=None, klen=None, q_off=None, k_off=None,
                        rope_mode=-1, k_rotated=False, rot_groups=1, rot_stride=0, rot_col=None, dtype=None):
        """One attention through the engine's launcher in a given layout (stn_op_attention_ex).  q, kv, out: 2-D [rows, ld] buffers (their
        row length is the stride); kv and out come back as new fp32 arrays of the same shapes, whole.  v_col defaults to k_col + H*dh,
        rot_col to k_col.  Returns (out, kv, form string)."""
        q = _c(q, np.float32)
        kv_r = np.array(kv, dtype=np.float32, order="C", copy=True)
        o_r = np.array(out, dtype=np.float32, order="C", copy=True)
        _a, qlp = _opt(qlen, np.int32)
        _b, klp = _opt(klen, np.int32)
        _d, qop = _opt(q_off, np.int32)
        _e, kop = _opt(k_off, np.int32)
        form = ctypes.create_string_buffer(64)
        self._ck(self._lib.stn_op_attention_ex(self._h, self.dtype if dtype is None else _DTYPES[dtype], int(B), int(Lq), int(Lk), int(H), int(dh),
                                               q.reshape(-1), q.size, q.shape[1], int(q_col), kv_r.reshape(-1), kv_r.size, kv_r.shape[1],
                                               int(k_col), int(k_col + H * dh if v_col is None else v_col), o_r.reshape(-1), o_r.size,
                                               o_r.shape[1], qlp, klp, qop, kop, int(rope_mode), int(bool(k_rotated)), int(rot_groups),
                                               int(rot_stride), int(k_col if rot_col is None else rot_col), form, ctypes.sizeof(form)))
        return o_r, kv_r, form.value.decode()

    def op_xattn_hs(self, xn, Wq, bq, Wo, kv, part, part_stride, B, L, Lk, qlen, k_col=0, klen=None, k_off=None, rope_mode=-1,
                    pairs=False, dtype=None):
        """One head-split cross-attention launch (stn_op_xattn_hs).  xn [M, 384]; kv: 2-D [rows, ldk]; part: the whole 1-D destination
        buffer, returned as a new fp32 array.  Returns (part, pairs table or None, form string)."""
        xn = _c(xn, np.float32)
        kv = _c(kv, np.float32)
        part_r = np.array(part, dtype=np.float32, order="C", copy=True).reshape(-1)
        _b, bqp = _opt(bq, np.float32)
        _k, klp = _opt(klen, np.int32)
        _o, kop = _opt(k_off, np.int32)
        pr = np.full(2 * ((B + 1) // 2), -7, np.int32) if pairs else None
        form = ctypes.create_string_buffer(64)
        self._ck(self._lib.stn_op_xattn_hs(self._h, self.dtype if dtype is None else _DTYPES[dtype], xn.shape[0], xn.reshape(-1),
                                           _c(Wq, np.float32), bqp, _c(Wo, np.float32), kv.reshape(-1), kv.size, kv.shape[1], int(k_col),
                                           int(B), int(L), int(Lk), _c(qlen, np.int32), klp, kop, int(rope_mode), int(bool(pairs)),
                                           int(part_stride), part_r, part_r.size, None if pr is None else pr.ctypes.data, form,
                                           ctypes.sizeof(form)))
        return part_r, pr, form.value.decode()

    def op_randn(self, seed, B, D, L, utt_ids=None, length=None):
        out = np.empty((B, D, L), np.float32)
        _u, up = _opt(utt_ids, np.int64)
        _l, lp = _opt(length, np.int32)
        self._ck(self._lib.stn_op_randn(self._h, seed, B, D, L, up, lp, out))
        return out


def pinned_array(shape, dtype):
    """A numpy array on page-locked host memory (stn_host_alloc_pinned): uploads from it are asynchronous DMA.  The memory is
    released when the array (and every view of it) is gone."""
    L = load()
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    p = L.stn_host_alloc_pinned(n)
    if not p:
        raise MemoryError("stn_host_alloc_pinned failed")
    buf = (ctypes.c_char * n).from_address(p)
    arr = np.frombuffer(buf, dtype=dt).reshape(shape)
    import weakref
    weakref.finalize(buf, L.stn_host_free_pinned, ctypes.c_void_p(p))
    return arr
