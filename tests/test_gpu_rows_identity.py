"""When the output stage's chain runs again for a report.  The walk tests prove that every report and fetch returns the right values; this
one proves that a report reuses what a fetch left exactly as long as nothing in front of its stage changed.

The chain order is pitch, rate, filter chain, expander, de-esser, compressor, and behind them the silence edges.
The rule, from that order alone: after one setting of stage c changed, the report of stage r runs the whole chain once (Engine::out_source
runs every stage that is on, so every family of the three dynamics stages shows one launch) if c is at or in front of r, and launches
nothing if c is behind r.  Every change is in front of the silence edges.  The same report again launches nothing.

A tiny model, one batch of 3 rows of about a second (output_walk.BATCHES[1]), the filter chain, expander, de-esser, compressor and
silence trim on, one warm fetch, then one change and one report with the launch counts of the `out.*` families read from profile()."""
import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.arch import tiny_arch
from gpu_util import make_inputs
import output_walk as ow

pytestmark = pytest.mark.gpu

CHAIN = ("pitch", "rate", "filters", "expander", "deesser", "compressor")  # the order out_source runs the stages in
EXPANDERS = (binding.EXPANDER_SPEECH, (-40.0, 4.0, 0.0, 30.0, 1.0, 10.0, 40.0))
BASE = dict(pitch=None, rate=None, filters=ow.VALUES["filters"][0], expander=EXPANDERS[0], deesser=ow.VALUES["deesser"][0],
            compressor=ow.VALUES["compressor"][0])
CHANGED = dict(pitch=ow.VALUES["pitch"][0], rate=ow.VALUES["rate"][1], filters=ow.VALUES["filters"][1], expander=EXPANDERS[1],
               deesser=ow.VALUES["deesser"][1], compressor=ow.VALUES["compressor"][1])
SETTERS = dict(pitch=lambda e, v: e.set_pitch(v), rate=lambda e, v: e.set_output_rate(v), filters=lambda e, v: e.set_filters(list(v)),
               expander=lambda e, v: e.set_expander(v), deesser=lambda e, v: e.set_deesser(v), compressor=lambda e, v: e.set_compressor(v))
# the reports, by the stage whose results they read (the edges are found on the rows behind every stage)
REPORTS = dict(expander=lambda e: e.batch_expander(), deesser=lambda e: e.batch_deesser(), compressor=lambda e: e.batch_compressor(),
               silence_edges=lambda e: e.batch_silence_edges())
XP = ["out.expander_chunks1", "out.expander_scan1", "out.expander_chunks2", "out.expander_scan2", "out.expander_write", "out.expander_rows"]
DS = ["out.deesser_band_chunks", "out.deesser_band_scan", "out.deesser_chunks1", "out.deesser_scan1", "out.deesser_chunks2",
      "out.deesser_scan2", "out.deesser_write", "out.deesser_rowmax"]
CP = ["out.compressor_chunks1", "out.compressor_scan1", "out.compressor_chunks2", "out.compressor_scan2", "out.compressor_write",
      "out.compressor_rowmax"]
ED = ["out.edges_frames", "out.edges_rows"]


def reruns(change, report):
    """the rule: the chain runs again when the changed stage is at or in front of the report's"""
    return report == "silence_edges" or CHAIN.index(change) <= CHAIN.index(report)


@pytest.fixture(scope="module")
def engine():
    a = tiny_arch()
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    lens, durs, seed = ow.BATCHES[1]
    ids, mask, sttl, sdp = make_inputs(a, len(lens), max(lens), lens, seed=seed)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=np.asarray(durs, np.float32))
    e.batch_run(2, ow.SPEED, 9)
    _, L, _ = e.batch_dims()
    W = L * a.base_chunk_size * a.chunk_compress_factor
    e.dbg_batch_set_wav(ow.busy_rows(a.sample_rate, W, ow.spans(a.sample_rate, W, durs), 41))
    e.set_silence_trim(ow.VALUES["trim"][0])
    yield e
    e.close()


def _launches(e):
    return {k: v["launches"] for k, v in e.profile().items() if k.startswith("out.") and v["launches"]}


@pytest.mark.parametrize("report", list(REPORTS))
@pytest.mark.parametrize("change", CHAIN)
def test_a_report_runs_the_chain_again_exactly_when_a_stage_in_front_of_it_changed(engine, change, report):
    e = engine
    for name in CHAIN:
        SETTERS[name](e, BASE[name])
    e.batch_fetch()  # warm: every stage's results are those of this batch under BASE
    SETTERS[change](e, CHANGED[change])
    e.profile_enable(True)
    e.profile_reset()
    try:
        REPORTS[report](e)
        first = _launches(e)
        e.profile_reset()
        REPORTS[report](e)
        second = _launches(e)
    finally:
        e.profile_enable(False)
    print(f"\n{change} changed, batch_{report}: {first or 'nothing'}; again: {second or 'nothing'}")
    if reruns(change, report):
        assert all(first.get(k, 0) == 1 for k in XP + DS + CP), first
        assert any(k.startswith("out.filter") for k in first), first
        if report == "silence_edges":
            assert all(first.get(k, 0) == 1 for k in ED), first
        else:
            assert not any(k in first for k in ED), first
    else:
        assert first == {}, first
    assert second == {}, second
