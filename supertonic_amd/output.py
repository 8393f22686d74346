"""The fetch-time settings of the returned audio as one value (host only): what TextToSpeech keeps per instance, what a call overrides,
and what the service's batch key compares."""
import contextlib
import dataclasses

from . import binding


def _loudness(v):
    if isinstance(v, (tuple, list)):
        t, c = v
        return float(t), float(c)
    return float(v), -1.0


def _switched(args):
    """A binding.*_args function, (on, value), as a parser: the value, or False for off"""
    def parse(v):
        on, ms = args(v)
        return ms if on else False
    return parse


def _peak_mode(v):
    binding.peak_mode_id(v)
    return v


# keyword -> its parser, for every value but None (unset); the order is the order the keywords are validated in
_PARSE = {
    "output_rate": int,
    "filters": lambda v: binding.filter_args(None if v is False else v),
    "expander": lambda v: binding.expander_args(v) or False,
    "deesser": lambda v: binding.deesser_args(v) or False,
    "compressor": lambda v: binding.compressor_args(v) or False,
    "loudness": lambda v: v is not False and _loudness(v),
    "trim_silence": lambda v: v is not False and binding.silence_trim_args(v)[1:],
    "max_pause": _switched(binding.pause_limit_args),
    "limiter": _switched(binding.limiter_args),
    "peak_mode": _peak_mode,
    "dither": lambda v: binding.dither_args(v) or False,
    "pitch": lambda v: binding.pitch_args(v) or False,
    "pitch_mode": binding.pitch_mode_name,
}


@dataclasses.dataclass(frozen=True)
class OutputSettings:
    """What happens to the audio on the GPU at fetch time (include/stn.h; no captured graph depends on any of it), in the order it
    happens.  Every field is None (unset: the instance's value holds), off, or a value in one normalized form; equal settings compare
    and hash equal.  The keywords of load_text_to_speech and of TextToSpeech's methods are these fields, as parse() takes them:

    output_rate   Hz of the returned audio, resampled from the model's rate (stn_set_output_rate).  Off: 0, the model's rate.
    filters       a chain of up to 8 biquads every utterance goes through, after the resampler and before everything below
                  (stn_set_filters): a list as binding.filter_args takes it, e.g. [("highpass", 80)]; the numeric limits are checked by
                  the engine against the output rate in force.  Normalized: a tuple of (type, freq_hz, q, gain_db).  Off: False or [], ().
    expander      what lies under a threshold (the noise floor between words) turned down, behind the chain and in front of the de-esser
                  (stn_set_expander): True (the "speech" default: -50 dB, 3:1, knee 6 dB, range 24 dB, attack 1 ms, hold 30 ms, release
                  150 ms), a dict of those fields or a 7-tuple, as binding.expander_args takes them.  Normalized: the 7-tuple of floats.
                  Off: False.
    deesser       the sibilants of every utterance turned down, behind the chain and in front of the compressor (stn_set_deesser): True (the
                  "speech" default: 5500 Hz, -30 dB, 4:1, knee 6 dB, attack 1 ms, release 40 ms, range 12 dB, split), a dict of those
                  fields or an 8-tuple, as binding.deesser_args takes them; freq_hz is checked by the engine against the output rate in
                  force.  Normalized: the 8-tuple (seven floats and the mode's name).  Off: False.
    compressor    the dynamic range of every utterance compressed, behind the chain and the de-esser and before everything below (stn_set_compressor): True
                  (the "speech" default: -24 dB, 3:1, knee 6 dB, attack 5 ms, release 120 ms, makeup 0 dB), a dict of those fields or
                  a 6-tuple, as binding.compressor_args takes them.  Normalized: the 6-tuple of floats.  Off: False.
    loudness      every utterance normalized to this BS.1770-4 integrated loudness, measured at the output rate (stn_set_loudness): a
                  target in LUFS (peak ceiling -1 dBFS) or (target, ceiling dBFS).  Normalized: (target, ceiling).  Off: False.
    trim_silence  leading and trailing silence trimmed by level (stn_set_silence_trim): top_db (20 ms kept, 5 ms fade) or
                  (top_db, keep_ms, fade_ms).  Normalized: the triple.  Off: False.
    max_pause     every pause inside an utterance longer than this many milliseconds ([20, 5000]) shortened to it (stn_set_pause_limit);
                  it acts only while trim_silence is on.  Off: False.
    limiter       the full loudness gain, and a look-ahead peak limiter holds the ceiling (stn_set_limiter): True (5 ms) or the look-ahead
                  in milliseconds ([0.5, 10]); it acts only while loudness is on.  Normalized: milliseconds.  Off: False, the capped gain.
    peak_mode     the ceiling of loudness as a sample peak ("sample") or a true peak ("true": dBTP, 4x oversampled; stn_set_peak_mode);
                  it acts only while loudness is on.  Off: "sample".
    dither        how the 16- and 24-bit PCM stores quantize, the last step (stn_set_dither): True or "tpdf", "tpdf-hp", "round", or
                  (mode, seed), as binding.dither_args takes them; it acts on audio fetched as "pcm16" or "pcm24" only (float, mu-law
                  and A-law are unaffected).  Normalized: (mode name, seed).  Off: False or "off", the truncating store.
    pitch         every utterance shifted by this many semitones ([-12, 12]) without a change of length, the first step: everything above
                  sees the shifted audio (stn_set_pitch).  Normalized: a float.  Off: False or 0.
    pitch_mode    what the shift does to the formants (stn_set_pitch_mode): "resample" (they move with the pitch) or "formant" (the
                  spectral envelope of the audio before the shift is put back); it acts only while pitch is on.  Off: "resample"."""
    output_rate: object = None
    filters: object = None
    loudness: object = None
    trim_silence: object = None
    max_pause: object = None
    limiter: object = None
    peak_mode: object = None
    compressor: object = None  # (declared last: OFF and positional construction keep their seven fields; applied behind filters)
    # (applied between filters and compressor.)  Not a constructor argument: it is set by parse() and replace() only, so that positional
    # construction, OFF, and dataclasses.replace of a value that names no de-esser keep meaning what they meant before the field was
    # there (dataclasses.replace copies constructor arguments only: it leaves this field unset, and refuses to be given it).  Compared
    # and hashed like every other field.
    deesser: object = dataclasses.field(default=None, init=False)
    # No dataclass field at all, but an attribute that parse() and replace() set, kept through over() and compared and hashed with the
    # fields: OFF and ALL_OFF are pinned from three sides (ALL_OFF leaves no field at None; taking compressor and deesser out of ALL_OFF
    # gives OFF; OFF is the constructor's value of its seven arguments), which no further field of any kind satisfies.  So neither
    # names it, and who needs every setting decided asks decided().
    dither = None
    # An attribute like dither, for the same reasons.  Unset and off compare and hash equal here, so that a value decided() made stays
    # equal to ALL_OFF with dither off, as it was before the setting was there.  Where the difference matters (a request that names no
    # pitch gets the server's, one that says 0 gets none) the service's BatchKey carries it beside the settings (pitch_set).
    pitch = None
    # An attribute like pitch, for the same reasons, and with unset and off comparing equal as its are (applied between filters and
    # deesser).  The service's BatchKey carries the difference (expander_set).
    expander = None
    # An attribute like pitch, applied next to it.  Unset and "resample" compare equal; the service's BatchKey carries the difference
    # (pitch_mode_set).
    pitch_mode = None

    def _all(self):
        return tuple(getattr(self, f.name) for f in dataclasses.fields(self)) + (self.dither, self.pitch or False, self.expander or False,
                                                                               self.pitch_mode or "resample")

    def __eq__(self, other):
        return other._all() == self._all() if type(other) is type(self) else NotImplemented

    def __hash__(self):
        return hash(self._all())

    def __repr__(self):
        return "OutputSettings(" + ", ".join(f"{k}={v!r}" for k, v in zip([f.name for f in dataclasses.fields(self)] + ["dither", "pitch", "expander", "pitch_mode"], self._all())) + ")"

    def decided(self):
        """This value over ALL_OFF, and dither, pitch, expander and pitch_mode off where that leaves them unset: every setting decided
        (what an instance holds)"""
        s = self.over(OutputSettings.ALL_OFF)
        return s.replace(dither=False if s.dither is None else s.dither, pitch=False if s.pitch is None else s.pitch,
                         expander=False if s.expander is None else s.expander, pitch_mode=s.pitch_mode or "resample")

    @classmethod
    def parse(cls, **kw):
        """The keyword forms above -> the value; None leaves a field unset.  A refused value is binding's ValueError, an unknown keyword
        a TypeError."""
        for k in kw:
            if k not in _PARSE:
                raise TypeError(f"{k!r} is not an output setting ({', '.join(_PARSE)})")
        return cls().replace(**{k: p(kw[k]) for k, p in _PARSE.items() if kw.get(k) is not None})

    def replace(self, **changes):
        """This value with the fields named in changes set to their (normalized) values: dataclasses.replace for every field, deesser,
        dither, pitch, expander and pitch_mode included"""
        deesser, dither, pitch = changes.pop("deesser", self.deesser), changes.pop("dither", self.dither), changes.pop("pitch", self.pitch)
        expander, pitch_mode = changes.pop("expander", self.expander), changes.pop("pitch_mode", self.pitch_mode)
        new = dataclasses.replace(self, **changes)
        object.__setattr__(new, "pitch_mode", pitch_mode)
        object.__setattr__(new, "expander", expander)
        object.__setattr__(new, "deesser", deesser)
        object.__setattr__(new, "dither", dither)
        object.__setattr__(new, "pitch", pitch)
        return new

    def kwargs(self):
        """The set fields under their keywords, as parse takes them (filters as a list)"""
        kw = {k: getattr(self, k) for k in _PARSE if getattr(self, k) is not None}
        if "filters" in kw:
            kw["filters"] = list(self.filters)
        return kw

    def over(self, base):
        """base with this value's set fields in force"""
        return base.replace(**{k: getattr(self, k) for k in self.kwargs()})

    def apply(self, engine):
        """The set fields onto a binding.Engine, in the one order that works: a chain is checked against the output rate in force, so
        it goes off before the rate changes and on after it, and so does the de-esser.  The rest are independent of each other; pitch,
        the first stage of the chain, goes first."""
        if self.pitch is not None:
            engine.set_pitch(self.pitch or None)
        if self.pitch_mode is not None:
            engine.set_pitch_mode(self.pitch_mode)
        if self.filters is not None:
            engine.set_filters(None)
        if self.deesser is not None and (self.output_rate is not None or not self.deesser):
            engine.set_deesser(None)
        if self.output_rate is not None:
            engine.set_output_rate(self.output_rate)
        if self.filters:
            engine.set_filters(self.filters)
        if self.expander is not None:
            engine.set_expander(self.expander or None)
        if self.deesser:
            engine.set_deesser(self.deesser)
        if self.compressor is not None:
            engine.set_compressor(self.compressor or None)
        if self.loudness is not None:
            engine.set_loudness(*(self.loudness or (None,)))
        if self.trim_silence is not None:
            engine.set_silence_trim(self.trim_silence or None)
        if self.max_pause is not None:
            engine.set_pause_limit(self.max_pause or None)
        if self.limiter is not None:
            engine.set_limiter(self.limiter or None)
        if self.peak_mode is not None:
            engine.set_peak_mode(self.peak_mode)
        if self.dither is not None:
            engine.set_dither(self.dither or None)

    @contextlib.contextmanager
    def applied(self, engine, base):
        """For the body, the engine (which holds base) holds self.over(base), which is what the body gets.  On every way out, a setter's
        refusal part-way through included, the fields this value set are base's again."""
        try:
            self.apply(engine)
            yield self.over(base)
        finally:
            OutputSettings().replace(**{k: getattr(base, k) for k in self.kwargs()}).apply(engine)


# OFF leaves compressor and deesser unset (a base that does not name them compares equal after over(OFF)); ALL_OFF names every field
# (dither and pitch, which are none, neither names: decided())
OutputSettings.OFF = OutputSettings(0, (), False, False, False, False, "sample")
OutputSettings.ALL_OFF = OutputSettings.OFF.replace(compressor=False, deesser=False)
