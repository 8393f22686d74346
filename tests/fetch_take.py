"""What the fetch-scratch and span-table tests compare between a live handle and a fresh one (test_gpu_fetch_scratch.py,
test_gpu_batch_spans.py): every fetch path and report of the finished batch, taken in one fixed order, and the byte comparison."""
import numpy as np


def take(e, slot, more=False):
    """every fetch path and every report of the finished batch, as name -> array; more: also the reports of the stages in front of
    the measurement (compressor, de-esser, expander), the pauses, the loudness range and the joined programmes' measurement"""
    B = e.batch_dims()[0]
    out = {}
    out["f32"], out["dur"] = e.batch_fetch()
    out["pcm16"] = e.batch_fetch_encoded("pcm16")[0]
    join = ([B - B // 2, B // 2], [120, 60], [0.1, 0.05])
    for scope in ("programme", "row"):
        out["join_" + scope], out["plen_" + scope], out["pdur_" + scope] = e.batch_fetch_joined(*join, gain_scope=scope, cut=False)
    e.fetch_pcm16_begin(slot)
    out["slot"] = e.fetch_pcm16_end(slot)[0]
    out["lufs"], out["peak"], out["gain"] = e.batch_loudness()
    out["red"], out["limited"] = e.batch_limiter()
    out["tp_in"], out["tp_out"], out["trim"] = e.batch_true_peak()
    out["start"], out["end"] = e.batch_silence_edges()
    if more:
        out["cp_db"] = e.batch_compressor()
        out["ds_db"] = e.batch_deesser()
        out["xp_db"], out["xp_closed"] = e.batch_expander()
        out["pz_len"], out["pz_cuts"], out["pz_pairs"] = e.batch_pauses()
        out["m_max"], out["s_max"], out["lra"], out["n_st"] = e.batch_loudness_range()
        out["j_lufs"], out["j_peak"], out["j_gain"] = e.batch_join_loudness(*join)
        out["j_m_max"], out["j_s_max"], out["j_lra"], out["j_n_st"] = e.batch_join_loudness_range(*join)
    return {k: np.asarray(v) for k, v in out.items()}


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)
