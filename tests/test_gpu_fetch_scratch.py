"""The output stage's fetch scratch under a live handle on an MI355X: every grow-only buffer of the stage (the measurement's, the
detection's, the limiter's and the true-peak mode's scratch, the resampled fp32 rows, the encoded rows, the join tables) grows when a
larger batch follows a small one, and is then reused, larger than needed and holding the large batch's values, by the small batch again.
With every option on (16 kHz, loudness, limiter, true peak, silence trim), whatever a handle delivers and reports after each of its
batches is byte for byte what a fresh handle delivers that has only ever seen that one batch."""
import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.arch import tiny_arch
from gpu_util import make_inputs
import fetch_rows
from fetch_take import assert_same as _assert_same, take as _take

pytestmark = pytest.mark.gpu
RATE, TARGET, CEIL, MS, SPEED = 16000, -12.0, -1.0, 5.0, 1.05
# (token lengths, forced durations, seed): two short utterances, each longer than the measurement's one 400 ms block, and six longer ones
SMALL = ([9, 6], np.array([0.50, 0.46], np.float32), 3)
BIG = ([14, 9, 5, 12, 7, 11], np.array([0.95, 1.10, 0.88, 1.21, 1.02, 0.91], np.float32), 2)


def _handle(a, rate=RATE):
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.set_output_rate(rate)
    e.set_loudness(TARGET, CEIL)
    e.set_limiter(MS)
    e.set_peak_mode("true")
    e.set_silence_trim((40.0, 20.0, 5.0))
    return e


def _load(a, e, batch, rate=RATE):
    lens, durs, seed = batch
    ids, mask, sttl, sdp = make_inputs(a, len(lens), max(lens), lens, seed=seed)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, SPEED, 9)
    B, L, _ = e.batch_dims()
    W = L * a.base_chunk_size * a.chunk_compress_factor
    spans = [min(W, int(np.float32(d / np.float32(SPEED)) * np.float32(a.sample_rate))) for d in durs]
    e.dbg_batch_set_wav(fetch_rows.rows(a.sample_rate, W, spans, rate, MS, 40 + seed))


@pytest.fixture(scope="module")
def fresh():
    """what a handle that has only ever seen the one batch delivers, per batch: computed once"""
    a = tiny_arch()
    want = {}
    for name, batch in (("small", SMALL), ("big", BIG)):
        e = _handle(a)
        _load(a, e, batch)
        want[name] = _take(e, 0)
        e.close()
    return want


def test_fresh_handles_have_something_to_do(fresh):
    """the rows keep every option busy: trimmed edges inside the spans, limited samples, a gain other than 1, a true peak to report"""
    for name, w in fresh.items():
        assert np.all(np.isfinite(w["lufs"])) and np.all(w["gain"] != 1.0), name
        assert np.any(w["start"] > 0) and np.all(w["end"] > w["start"]), name
        assert np.any(w["limited"] > 0) and np.any(w["red"] > 0.0), name
        assert np.all(w["tp_out"] > 0.0) and np.all(w["trim"] <= 1.0) and w["f32"].any() and w["slot"].any(), name


def test_scratch_grows_under_a_live_handle_and_is_reused_dirty(fresh):
    a = tiny_arch()
    e = _handle(a)
    _load(a, e, SMALL)
    _assert_same(_take(e, 0), fresh["small"], "first small batch")
    _load(a, e, BIG)  # every scratch grows
    _assert_same(_take(e, 1), fresh["big"], "big batch after a small one")
    _load(a, e, SMALL)  # larger than needed now, and holding the big batch's values
    # an op-level measurement of other rows in between: the spans the scratch held are gone, the next fetch uploads them again
    x = (0.1 * np.sin(np.arange(3 * 5000) / 7.0)).astype(np.float32).reshape(3, 5000)
    e.op_loudness(x, RATE, np.array([5000, 4100, 3000], np.int64))
    _assert_same(_take(e, 0), fresh["small"], "small batch in the big batch's scratch, after op_loudness")
    _assert_same(_take(e, 1), fresh["small"], "the same again, from what the handle cached")
    e.close()


def test_scratch_grows_and_is_reused_at_192_khz():
    """the same at the top of the range: W_out is 4.35 W, and every carve, span guard and join plan is computed from it"""
    a, rate = tiny_arch(), 192000
    want = {}
    for name, batch in (("small", SMALL), ("big", BIG)):
        f = _handle(a, rate)
        _load(a, f, batch, rate)
        want[name] = _take(f, 0)
        f.close()
        assert np.any(want[name]["limited"] > 0) and np.all(want[name]["end"] > want[name]["start"]) and np.all(np.isfinite(want[name]["lufs"])), name
    e = _handle(a, rate)
    _load(a, e, SMALL, rate)
    _assert_same(_take(e, 0), want["small"], "first small batch")
    _load(a, e, BIG, rate)
    _assert_same(_take(e, 1), want["big"], "big batch after a small one")
    _load(a, e, SMALL, rate)
    _assert_same(_take(e, 1), want["small"], "small batch in the big batch's scratch")
    e.close()
