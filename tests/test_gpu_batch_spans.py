"""The finished batch's span table under a live handle on an MI355X (DESIGN.md sections 11 and 11a): one table per finished batch and
(rate, row length) that every stage of a fetch takes its spans from, two entries of it (the model's rate, which pitch reads, and the
output rate), and the joined programmes' spans riding in the join tables.  Tiny arch, bf16, output_walk's three rows of about a second
with busy_rows planted.  Every comparison is byte equality against a fresh handle that has only seen the state compared
(fetch_take.py); beside it the handle's count of span uploads (stn_dbg_span_uploads) is held to the rule: once per finished batch and
(rate, row length), whatever is fetched or reported in between."""
import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.arch import tiny_arch
from gpu_util import make_inputs
from fetch_take import assert_same, take
import output_walk as ow

pytestmark = pytest.mark.gpu
LENS, DURS, SEED = ow.BATCHES[1]
# two batches of one shape (the same token lengths, the same longest duration: the same B, L and row length at every rate, so no
# scratch moves between them) whose spans differ in every row by 0.43 s and more after the speed: more than one 400 ms gating block
SPANS_A = (1.40, 0.80, 0.90)
SPANS_B = (0.95, 1.40, 0.45)
JOIN = ([2, 1], [120, 60], [0.1, 0.05])
EVERY_STAGE = dict(rate=16000, filters=ow.VALUES["filters"][0], expander=binding.EXPANDER_SPEECH, deesser=binding.DEESSER_SPEECH,
                   compressor=binding.COMPRESSOR_SPEECH, loudness=(-12.0, -1.0), limiter=5.0, peak="true", trim=(40.0, 20.0, 5.0), pause=60.0,
                   pitch=2.0)
_SETTERS = dict(
    rate=lambda e, v: e.set_output_rate(v),
    filters=lambda e, v: e.set_filters(list(v)),
    expander=lambda e, v: e.set_expander(v),
    deesser=lambda e, v: e.set_deesser(v),
    compressor=lambda e, v: e.set_compressor(v),
    loudness=lambda e, v: e.set_loudness(*v),
    limiter=lambda e, v: e.set_limiter(v),
    peak=lambda e, v: e.set_peak_mode(v),
    trim=lambda e, v: e.set_silence_trim(v),
    pause=lambda e, v: e.set_pause_limit(v),
    pitch=lambda e, v: e.set_pitch(v),
)


def _handle(a, settings):
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    for name, value in settings.items():
        _SETTERS[name](e, value)
    return e


def _load(a, e, durs=DURS, wav_seed=41):
    ids, mask, sttl, sdp = make_inputs(a, len(LENS), max(LENS), LENS, seed=SEED)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=np.asarray(durs, np.float32))
    e.batch_run(2, ow.SPEED, 9)
    W = e.batch_dims()[1] * a.base_chunk_size * a.chunk_compress_factor
    e.dbg_batch_set_wav(ow.busy_rows(a.sample_rate, W, ow.spans(a.sample_rate, W, durs), wav_seed))


def _fresh(a, settings, durs, what):
    """what(e) of a handle that has done nothing but reach the state"""
    e = _handle(a, settings)
    _load(a, e, durs)
    out = what(e)
    e.close()
    return out


def _arrays(r):
    r = r if isinstance(r, tuple) else (r,)
    return {str(i): np.asarray(v) for i, v in enumerate(r)}


def test_same_shape_other_spans():
    """a second batch of the first one's shape and other spans, every stage on: whatever is kept of the spans is kept per batch"""
    a = tiny_arch()
    want = {d: _fresh(a, EVERY_STAGE, d, lambda e: (take(e, 0, more=True), e.batch_dims())) for d in (SPANS_A, SPANS_B)}
    assert want[SPANS_A][1] == want[SPANS_B][1], "the two batches are to have one shape"
    wa, wb = want[SPANS_A][0], want[SPANS_B][0]
    assert np.all(np.abs(wa["dur"] - wb["dur"]) > 0.4) and wa["f32"].tobytes() != wb["f32"].tobytes() and wa["lufs"].tobytes() != wb["lufs"].tobytes()
    e = _handle(a, EVERY_STAGE)
    for i, d in enumerate((SPANS_A, SPANS_B, SPANS_A)):
        _load(a, e, d)
        assert_same(take(e, i % 2, more=True), want[d][0], f"batch {i}")
        assert_same(take(e, i % 2, more=True), want[d][0], f"batch {i}, from what the handle kept")
    e.close()


def _visit(e):
    out = {}
    for name, r in (("f32", e.batch_fetch()), ("loudness", e.batch_loudness()), ("edges", e.batch_silence_edges()), ("compressor", e.batch_compressor())):
        out.update({name + k: v for k, v in _arrays(r).items()})
    return out


def test_rates_in_rotation_within_one_batch():
    """pitch on, three rates visited twice each: the table's two entries are the model's rate (what pitch reads, and every stage while
    no rate is set) and the output rate, so 16 kHz and 22.05 kHz evict each other and the model's rate is never uploaded again"""
    a = tiny_arch()
    settings = dict(pitch=2.0, compressor=binding.COMPRESSOR_SPEECH, loudness=(-12.0, -1.0), trim=(40.0, 20.0, 5.0))
    rates = (16000, 22050, None)
    want = {hz: _fresh(a, dict(settings, rate=hz), DURS, _visit) for hz in rates}
    assert len({w["f32" + "0"].shape for w in want.values()}) == 3
    e = _handle(a, settings)
    _load(a, e)
    # the first fetch uploads both entries; then 22.05 kHz takes 16 kHz's place, no rate needs what pitch uploaded, and the revisits
    # of the two rates find the other one in their place
    for visit, (hz, rise) in enumerate(zip(rates + rates, (2, 1, 0, 1, 1, 0))):
        before = e.span_uploads()
        e.set_output_rate(hz)
        assert_same(_visit(e), want[hz], f"visit {visit} at {hz}")
        assert e.span_uploads() - before == rise, (visit, hz)
        assert_same(_arrays(e.batch_fetch()), _arrays((want[hz]["f320"], want[hz]["f321"])), f"visit {visit} at {hz}, repeated")
        assert e.span_uploads() - before == rise, (visit, hz, "an immediate repeat fetch uploaded")
    e.close()


def test_rows_and_programmes_do_not_clobber_each_other():
    """the batch's rows and a join's programmes measured in turn on one handle: each call returns what it returns alone"""
    a = tiny_arch()
    settings = dict(loudness=(-12.0, -1.0))
    calls = (
        ("joined, programme gain", lambda e: e.batch_fetch_joined(*JOIN, gain_scope="programme", cut=False)),
        ("batch_loudness", lambda e: e.batch_loudness()),
        ("batch_join_loudness", lambda e: e.batch_join_loudness(*JOIN)),
        ("batch_join_loudness_range", lambda e: e.batch_join_loudness_range(*JOIN)),
        ("batch_loudness_range", lambda e: e.batch_loudness_range()),
        ("batch_fetch", lambda e: e.batch_fetch()),
    )
    want = [_fresh(a, settings, DURS, lambda e, c=c: _arrays(c(e))) for _, c in calls]
    e = _handle(a, settings)
    _load(a, e)
    for (name, c), w in zip(calls, want):
        assert_same(_arrays(c(e)), w, name)
    e.close()


def test_the_upload_count():
    a = tiny_arch()
    settings = dict(EVERY_STAGE)
    del settings["pitch"]
    e = _handle(a, settings)
    _load(a, e)
    u = e.span_uploads()
    e.batch_fetch()
    assert e.span_uploads() == u + 1, "the first fetch of a batch uploads its spans once, for every stage"
    take(e, 0, more=True)  # every fetch path and every report
    take(e, 1, more=True)
    assert e.span_uploads() == u + 1, "fetches and reports of the same batch uploaded spans again"
    _load(a, e, wav_seed=42)
    e.batch_fetch_encoded("pcm16")
    assert e.span_uploads() == u + 2, "the next batch uploads once"
    e.set_pitch(2.0)
    _load(a, e)
    e.fetch_pcm16_begin(0)
    e.fetch_pcm16_end(0)
    assert e.span_uploads() == u + 4, "with pitch on a first fetch uploads the spans at the model's rate and at the output rate"
    take(e, 1, more=True)
    assert e.span_uploads() == u + 4
    e.close()
