"""OutputSettings (supertonic_amd/output.py) and the service's BatchKey on the CPU: every keyword form to its normalized form and every
refusal, the order and the extent of apply(), what applied() puts back on every way out (a setter's refusal part-way included), and the
merge rule of service.batch_key against the rule written out here."""
import itertools

import pytest

from supertonic_amd import binding, service
from supertonic_amd.output import OutputSettings

FIELDS = ("output_rate", "filters", "loudness", "trim_silence", "max_pause", "limiter", "peak_mode")
SETTERS = {"output_rate": "set_output_rate", "filters": "set_filters", "loudness": "set_loudness", "trim_silence": "set_silence_trim",
           "max_pause": "set_pause_limit", "limiter": "set_limiter", "peak_mode": "set_peak_mode"}


class FakeEngine:
    """binding.Engine's seven setters: records the calls, keeps what is in force, and refuses the k-th call from now (refuse_at) once,
    before it changes anything"""

    def __init__(self):
        self.state = {"output_rate": 0, "filters": (), "loudness": False, "trim_silence": False, "max_pause": False, "limiter": False,
                      "peak_mode": "sample"}
        self.calls, self.refuse_at = [], None

    def _set(self, field, value):
        if self.refuse_at is not None:
            self.refuse_at -= 1
            if self.refuse_at < 0:
                self.refuse_at = None
                raise binding.StnError(-1, f"{SETTERS[field]} refused")
        self.calls.append((SETTERS[field], value))
        self.state[field] = value

    def set_output_rate(self, hz):
        self._set("output_rate", int(hz or 0))

    def set_filters(self, filters=None):
        self._set("filters", tuple(filters or ()))

    def set_loudness(self, target_lufs=None, ceiling_dbfs=-1.0):
        self._set("loudness", False if target_lufs is None else (target_lufs, ceiling_dbfs))

    def set_silence_trim(self, trim_silence=None):
        self._set("trim_silence", False if trim_silence is None else trim_silence)

    def set_pause_limit(self, max_pause=None):
        self._set("max_pause", False if max_pause is None else max_pause)

    def set_limiter(self, lookahead_ms=None):
        self._set("limiter", False if lookahead_ms is None else lookahead_ms)

    def set_peak_mode(self, mode="sample"):
        self._set("peak_mode", mode)


HP = ("highpass", 80.0, binding.FILTER_Q, 0.0)
# the instance's settings, and a call's that differ in every field
BASE = dict(output_rate=16000, filters=[("highpass", 80)], loudness=-16, trim_silence=40, max_pause=250, limiter=True, peak_mode="true")
CALL = dict(output_rate=8000, filters=False, loudness=(-23, -2), trim_silence=False, max_pause=100, limiter=2, peak_mode="sample")


def test_parse_takes_every_form_to_its_normalized_form():
    forms = {
        "output_rate": [(None, None), (16000, 16000), (16000.0, 16000), (0, 0)],
        "filters": [(None, None), (False, ()), ([], ()), ([("highpass", 80)], (HP,)), (["highpass:80"], (HP,)), ([{"type": "highpass", "freq": 80}], (HP,)),
                    ((HP,), (HP,))],
        "loudness": [(None, None), (False, False), (-16, (-16.0, -1.0)), ((-16, -2), (-16.0, -2.0)), ([-23, -3], (-23.0, -3.0))],
        "trim_silence": [(None, None), (False, False), (40, (40.0, 20.0, 5.0)), ((30, 0, 50), (30.0, 0.0, 50.0)), ([30, 10, 0], (30.0, 10.0, 0.0))],
        "max_pause": [(None, None), (False, False), (20, 20.0), (250.5, 250.5)],
        "limiter": [(None, None), (False, False), (True, 5.0), (2, 2.0), (0.5, 0.5)],
        "peak_mode": [(None, None), ("sample", "sample"), ("true", "true")],
    }
    assert set(forms) == set(FIELDS)
    for field, cases in forms.items():
        for given, want in cases:
            s = OutputSettings.parse(**{field: given})
            assert getattr(s, field) == want and type(getattr(s, field)) is type(want), (field, given)
            assert all(getattr(s, f) is None for f in FIELDS if f != field)
    assert OutputSettings.parse() == OutputSettings()


def test_parse_refuses_what_the_hosts_refuse_today():
    for kw, what in (({"max_pause": True}, "max_pause"), ({"max_pause": 19}, "must be in [20, 5000]"), ({"limiter": 0.4}, "must be in [0.5, 10]"),
                     ({"limiter": 10.1}, "must be in [0.5, 10]"), ({"peak_mode": "rms"}, "peak_mode"), ({"filters": [("bandpass", 300)]}, "type"),
                     ({"filters": [("highpass", 80)] * 9}, "at most 8"), ({"trim_silence": True}, "not a bool"), ({"trim_silence": 121}, "top_db"),
                     ({"trim_silence": (40, 1001, 5)}, "keep"), ({"trim_silence": (40, 20, 51)}, "fade")):
        with pytest.raises(ValueError) as ei:
            OutputSettings.parse(**kw)
        assert what in str(ei.value), (kw, str(ei.value))
    for bad in ({"trim_silence": 121}, {"limiter": 0.4}, {"max_pause": 5001}):
        with pytest.raises(ValueError) as ei:
            OutputSettings.parse(**bad)
        assert "must be in" in str(ei.value)
    with pytest.raises(TypeError):
        OutputSettings.parse(sample_rate=16000)
    # the service has no off form: a bool for trimming is refused there, False included
    for bad in (True, False):
        with pytest.raises(ValueError) as ei:
            service.batch_key(44100, 5, 1.05, trim_silence=bad)
        assert "not a bool" in str(ei.value)


def test_equality_hash_over_and_kwargs():
    a, b = OutputSettings.parse(loudness=-16, filters=["highpass:80"], limiter=True), OutputSettings.parse(loudness=(-16.0, -1), filters=[HP], limiter=5)
    assert a == b and hash(a) == hash(b) and {a: 1}[b] == 1 and a != OutputSettings.parse(loudness=-16, filters=[HP])
    base, call = OutputSettings.parse(**BASE), OutputSettings.parse(loudness=False, max_pause=100)
    both = call.over(base)
    assert (both.loudness, both.max_pause) == (False, 100.0)
    assert all(getattr(both, f) == getattr(base, f) for f in FIELDS if f not in ("loudness", "max_pause"))
    assert OutputSettings().over(base) == base and base.over(OutputSettings.OFF) == base
    assert all(getattr(OutputSettings.OFF, f) is not None for f in FIELDS)
    assert OutputSettings().kwargs() == {}
    assert a.kwargs() == {"filters": [HP], "loudness": (-16.0, -1.0), "limiter": 5.0}
    assert OutputSettings.parse(**a.kwargs()) == a and OutputSettings.parse(**base.kwargs()) == base


def test_apply_calls_the_setters_of_the_set_fields_in_the_documented_order():
    eng = FakeEngine()
    OutputSettings().apply(eng)
    assert eng.calls == []
    OutputSettings.parse(**BASE).apply(eng)
    assert eng.calls == [("set_filters", ()), ("set_output_rate", 16000), ("set_filters", (HP,)), ("set_loudness", (-16.0, -1.0)),
                         ("set_silence_trim", (40.0, 20.0, 5.0)), ("set_pause_limit", 250.0), ("set_limiter", 5.0), ("set_peak_mode", "true")]
    eng.calls = []
    OutputSettings.parse(**CALL).apply(eng)  # off goes to the engine as off; a chain that goes off is not set again behind the rate
    assert eng.calls == [("set_filters", ()), ("set_output_rate", 8000), ("set_loudness", (-23.0, -2.0)), ("set_silence_trim", False),
                         ("set_pause_limit", 100.0), ("set_limiter", 2.0), ("set_peak_mode", "sample")]
    for n in range(len(FIELDS) + 1):  # every subset: the setters of its fields and no other
        for fields in itertools.combinations(FIELDS, n):
            eng.calls = []
            OutputSettings.parse(**{f: BASE[f] for f in fields}).apply(eng)
            assert {c[0] for c in eng.calls} == {SETTERS[f] for f in fields}


def _engine_holding(base):
    eng = FakeEngine()
    base.apply(eng)
    eng.calls = []
    return eng, dict(eng.state)


@pytest.mark.parametrize("fields", [FIELDS, ("output_rate", "filters"), ("loudness", "limiter", "peak_mode"), ("trim_silence",), ()])
def test_applied_puts_back_exactly_the_overridden_fields_on_every_way_out(fields):
    base, call = OutputSettings.parse(**BASE), OutputSettings.parse(**{f: CALL[f] for f in fields})
    eng, held = _engine_holding(base)
    mine = {SETTERS[f] for f in fields}
    # a normal exit: the body sees the call's settings over the instance's, on the engine as well
    with call.applied(eng, base) as now:
        assert now == call.over(base) and eng.state == {f: getattr(now, f) for f in FIELDS}
    assert eng.state == held and {c[0] for c in eng.calls} == mine
    # an exception in the body
    with pytest.raises(KeyError):
        with call.applied(eng, base):
            raise KeyError("body")
    assert eng.state == held
    # the k-th setter of the apply refused, for every k: the body does not run, and what the setters before it changed is put back
    eng.calls = []
    call.apply(eng)
    n = len(eng.calls)
    eng, held = _engine_holding(base)
    for k in range(n):
        eng.calls, eng.refuse_at = [], k
        with pytest.raises(binding.StnError):
            with call.applied(eng, base):
                pytest.fail("the body ran although a setter was refused")
        assert eng.state == held, (k, eng.state)
        assert len(eng.calls) > k and {c[0] for c in eng.calls} == mine  # (k of the apply, then the restore: these fields only)


# ---- the merge rule ------------------------------------------------------------------------------------------------------------------------
def merge_grid():
    """Requests as batch_key's keyword arguments: {unset, two values} of every setting (loudness with its ceiling: a ceiling alone is
    unset as well), two values of encoding, scope and trim_chunks, as two products that each hold one group of settings at one value."""
    loud = [dict(), dict(peak_ceiling=-3.0), dict(loudness=-16.0), dict(loudness=-16.0, peak_ceiling=-2.0), dict(loudness=-23.0)]
    lim = [dict(), dict(limiter_ms=2.0), dict(limiter_ms=5.0)]
    peak = [dict(), dict(peak_mode="sample"), dict(peak_mode="true")]
    trim = [dict(), dict(trim_silence=40), dict(trim_silence=(40, 10, 0))]
    pause = [dict(), dict(max_pause_ms=100.0), dict(max_pause_ms=250.0)]
    rate = [dict(), dict(sample_rate=16000), dict(sample_rate=48000)]
    filt = [dict(), dict(filters=[]), dict(filters=[("highpass", 80)])]
    enc = [dict(), dict(encoding="mulaw")]
    scope = [dict(), dict(loudness_scope="text")]
    chunks = [dict(), dict(trim_chunks=True)]
    grid = list(itertools.product(loud, lim, peak, trim[:2], pause[:2], enc)) + list(itertools.product(trim, pause, rate, filt, scope, chunks))
    return [{k: v for part in parts for k, v in part.items()} for parts in grid]


def effective(r):
    """the rule, written out: two requests may merge when all their effective fields are equal; limiter, peak mode and the ceiling count
    only with loudness, the pause limit only with trimming"""
    r = dict(r)
    if "loudness" in r:
        r.setdefault("peak_ceiling", -1.0)
    else:
        for k in ("peak_ceiling", "limiter_ms", "peak_mode"):
            r.pop(k, None)
    if "trim_silence" in r:
        r["trim_silence"] = r["trim_silence"] if isinstance(r["trim_silence"], tuple) else (r["trim_silence"], 20, 5)
    else:
        r.pop("max_pause_ms", None)
    return r


def test_two_requests_share_a_batch_key_exactly_when_the_rule_says_so():
    grid = merge_grid()
    keys = [service.batch_key(44100, 5, 1.05, **r) for r in grid]
    effs = [effective(r) for r in grid]
    assert 300 <= len(grid) <= 1000
    assert all(hash(k) == hash(service.batch_key(44100, 5, 1.05, **r)) for k, r in zip(keys[::37], grid[::37]))
    n_same = 0
    for i, j in itertools.combinations(range(len(grid)), 2):
        same = effs[i] == effs[j]
        n_same += same
        assert (keys[i] == keys[j]) == same, (grid[i], grid[j])
    assert n_same > 100  # (the dropped fields do fold requests together)
    # total_step and speed are part of the key; a field the request leaves unset is unset in the key and absent from the call
    assert service.batch_key(44100, 5, 1.05) != service.batch_key(44100, 6, 1.05) != service.batch_key(44100, 6, 1.0)
    k = service.batch_key(44100, 5, 1.05, limiter_ms=2.0, peak_mode="true", max_pause_ms=100.0, peak_ceiling=-3.0)
    assert k.settings == OutputSettings() and k.settings.kwargs() == {} and k[2:5] == (None, "chunk", False)
    k = service.batch_key(44100, 5, 1.05, 16000, -16.0, -2.0, "alaw", "text", True, 40, 2.0, "true", 100.0, [("highpass", 80)])
    assert k.settings.kwargs() == {"output_rate": 16000, "filters": [HP], "loudness": (-16.0, -2.0), "trim_silence": (40.0, 20.0, 5.0),
                                   "max_pause": 100.0, "limiter": 2.0, "peak_mode": "true"}
    assert (k.encoding, k.loudness_scope, k.trim_chunks) == (binding.ENC_ALAW, "text", True)
