"""The pitch report on an MI355X (include/stn.h "f0"; f0_track_kernel and f0_stats_kernel, kernels_f0.hip): the
YIN track and the statistics of the case rows (tests/f0_cases.py: thirteen rows in one launch at 8, 16, 44.1, 48 and 192 kHz) against
the float64 contract (tests/f0_ref.py) within the derived bound (f0_ref.device_bound) and against the host rule on the device's own
track, independence of the batch, the refusals, the finished batch's report against the op on what the fetch delivers, and the pitch
stage's interval measured on the device.  tests/test_f0_cpu.py shows that the frames excluded here are few and that the bound's
first-order premise holds on these rows."""
import os
import re
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.arch import tiny_arch
from gpu_util import make_inputs
import f0_cases as fc
import f0_ref as ref
from f0_cases import PITCH_HZ, pitch_chain, pitch_row

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
G, CAP = binding.f0_group()
DURS = np.array([0.9, 0.7, 0.2, 1.0, 0.55], np.float32)
HP = (("highpass", 80.0, 0.7071, 0.0),)


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


_DEV = {}


def _device(eng, hz):
    """the op's results on the case rows at hz, once per rate"""
    if hz not in _DEV:
        x, n = fc.case_rows(hz, G)
        _DEV[hz] = eng.op_f0(x, hz, n)
    return _DEV[hz]


def _same(a, b):
    return (a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            and all(a[2][k].dtype == b[2][k].dtype and a[2][k].tobytes() == b[2][k].tobytes() for k in a[2]))


# ---- 1. against the float64 contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", fc.RATES)
def test_op_against_float64(eng, hz):
    x, n = fc.case_rows(hz, G)
    f0, ap, st = _device(eng, hz)
    assert np.all(np.isfinite(f0)) and np.all(np.isfinite(ap))  # the NaN behind every span reaches nothing
    und = fc.undecidable(hz, G)
    worst_f, worst_a, share_f, share_a, moved = 0.0, 0.0, 0.0, 0.0, 0
    for r, w in enumerate(fc.refs(hz, G)):
        F = w["plan"]["frames"]
        assert st["frames"][r] == F, (hz, fc.NAMES[r])  # the frame count exactly
        assert np.all(f0[r, F:] == 0.0) and np.all(ap[r, F:] == 1.0)
        for t in range(F):
            lag, det, got_f, got_a = int(w["lag"][t]), w["det"][t], float(f0[r, t]), float(ap[r, t])
            if t not in und[r]:
                assert (got_f > 0) == (lag > 0), (hz, fc.NAMES[r], t)  # voicing exactly
                if lag == 0:
                    assert got_f == 0.0 and got_a == 1.0
                    continue
                bf, ba = ref.device_bound(det, lag, w["plan"])
                ef, ea = abs(got_f / w["f0"][t] - 1.0), abs(got_a - w["ap"][t])
                worst_f, worst_a = max(worst_f, ef), max(worst_a, ea)
                share_f, share_a = max(share_f, ef / bf), max(share_a, ea / ba)
                assert ef <= bf and ea <= ba, (hz, fc.NAMES[r], t, ef, bf, ea, ba)
            else:  # the reference's value, or the reference's with tau^ moved by one lag
                moved += 1
                ok = False
                for step in (0, -1, 1):
                    cand = ref.moved(det, lag, w["plan"], step)
                    if cand is None:
                        continue
                    bf, _ = ref.device_bound(det, lag + step, w["plan"])
                    ok = ok or abs(got_f / cand[0] - 1.0) <= bf
                assert ok, (hz, fc.NAMES[r], t, got_f, w["f0"][t])
    print(f"{hz} Hz: worst |f0 / ref - 1| {worst_f:.3e} ({share_f:.3f} of its bound), worst |ap - ref| {worst_a:.3e} ({share_a:.3f} of its bound), "
          f"{moved} undecidable frame(s)")


@pytest.mark.parametrize("hz", fc.RATES)
def test_stats_are_the_host_rule_on_the_device_track(eng, hz):
    f0, _, st = _device(eng, hz)
    for r in range(f0.shape[0]):
        F = int(st["frames"][r])
        want = binding.f0_stats_rule(f0[r, :F])
        for key in ("frames", "voiced", "median_hz", "min_hz", "max_hz"):
            assert st[key][r].tobytes() == want[key].tobytes(), (hz, fc.NAMES[r], key, st[key][r], want[key])
        assert abs(float(st["mean_hz"][r]) - float(want["mean_hz"])) <= 2 * float(np.spacing(want["mean_hz"])), (hz, fc.NAMES[r])
    assert list(st["voiced"][:3]) == [0, 0, 1] and st["voiced"][fc.NOISE] == 0 and st["median_hz"][fc.NOISE] == 0.0
    for r, f in fc.TONES.items():
        assert abs(ref.cents(float(st["median_hz"][r]), f)) < 2.5 and abs(ref.cents(float(st["mean_hz"][r]), f)) < 2.5


# ---- 2. independence ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", [8000, 44100, 192000])
def test_a_row_does_not_depend_on_its_batch(eng, hz):
    x, n = fc.case_rows(hz, G)
    full = _device(eng, hz)
    assert _same(full, eng.op_f0(x, hz, n))  # a second run
    assert _same(full, eng.op_f0(np.pad(x, ((0, 0), (0, 1000)), constant_values=np.nan), hz, n))  # W padded by 1000 samples
    for r in (4, 5, fc.GLIDE, 12):
        F = int(full[2]["frames"][r])
        alone = eng.op_f0(x[r:r + 1], hz, n[r:r + 1])
        among = np.full((5, x.shape[1]), np.nan, np.float32)  # row 3 of 5, among unlike neighbours
        among[[0, 1, 2, 4]] = x[[11, 3, 9, 6]]
        among[3] = x[r]
        five = eng.op_f0(among, hz, np.array([n[11], n[3], n[9], n[r], n[6]], np.int64))
        for k in range(2):
            assert alone[k][0, :F].tobytes() == full[k][r, :F].tobytes() == five[k][3, :F].tobytes(), (hz, r, k)
        for key in full[2]:
            assert alone[2][key][0] == full[2][key][r] == five[2][key][3], (hz, r, key)


# ---- 3. refusals: messages, not faults, and nothing launched ----------------------------------------------------------------------------------
def test_refusals(eng):
    hz = 8000
    g = ref.plan(hz, 0)
    at_cap = (CAP - 1) * g["hop"] + 2 * g["tau_max"]
    x = np.zeros((1, at_cap + g["hop"]), np.float32)
    eng.profile_enable(True)
    try:
        eng.profile_reset()
        with pytest.raises(binding.StnError) as ei:  # one frame over the cap
            eng.op_f0(x, hz)
        assert ei.value.code == -1 and str(CAP) in str(ei.value) and str(CAP + 1) in str(ei.value)
        with pytest.raises(binding.StnError) as ei:  # arrays shorter than a row's track
            eng.op_f0(x[:, :8000], hz, cap=3)
        assert ei.value.code == -1 and "arrays" in str(ei.value)
        assert not any(k.startswith("out.f0") for k in eng.profile()), eng.profile()  # nothing was launched
        f0, ap, st = eng.op_f0(x, hz, [at_cap])  # at the cap: measured (digital silence: every frame gated)
        assert st["frames"][0] == CAP and st["voiced"][0] == 0 and f0.shape == (1, CAP) and not f0.any() and np.all(ap == 1.0)
        assert eng.profile()["out.f0"]["launches"] == 2
        print(f"one row at the cap ({CAP} frames at {hz} Hz): out.f0 {eng.profile()['out.f0']['ms']:.3f} ms")
    finally:
        eng.profile_enable(False)
    for bad in (7999, 192001):
        with pytest.raises(binding.StnError):
            eng.op_f0(np.zeros((1, 100), np.float32), bad)
    with pytest.raises(binding.StnError) as ei:
        eng.op_f0(np.zeros((1, 100), np.float32), hz, [101])
    assert "outside [0, W]" in str(ei.value)
    with pytest.raises(binding.StnError) as ei:
        eng.op_f0(np.zeros((1, 100), np.float32), hz, params={"fmin_hz": 20.0})
    assert "30 <= fmin" in str(ei.value)
    assert eng._lib.stn_batch_f0(eng._h, None, 0, None, None, None) == -3  # no finished batch
    assert "no finished batch" in eng.last_error()


# ---- 4. the finished batch ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 5, 14, [14, 9, 5, 12, 7], seed=2)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=DURS)
    for _ in range(3):  # (the third run replays the captured graph)
        e.batch_run(2, 1.05, 9)
    B, _, W = e.batch_dims()
    wav = np.stack([fc.harmonic(a.sample_rate, W, 95.0 + 40.0 * b) for b in range(B)]).astype(np.float32)
    e.dbg_batch_set_wav(wav)
    yield a, e
    e.close()


def _spans(e, dur):
    Wo = e.batch_dims()[2]
    return np.array([max(0, min(Wo, int(np.float32(d) * np.float32(e.output_rate)))) for d in dur], np.int64)


@pytest.mark.parametrize("setting", ["off", "chain"])
def test_batch_report_is_the_op_on_the_fetched_rows(batch, setting):
    a, e = batch
    if setting == "chain":
        e.set_pitch(3.0)
        e.set_output_rate(16000)
        e.set_filters(HP)
    try:
        cached, replays = e.graphs_cached, e.graph_replays
        before, dur = e.batch_fetch()  # (loudness is off: the fetch is the signal before the gain)
        got = e.batch_f0()
        after, _ = e.batch_fetch()
        assert before.tobytes() == after.tobytes()  # the report changes no fetch
        assert e.graphs_cached == cached and e.graph_replays == replays  # and no captured graph
        n = _spans(e, dur)
        want = e.op_f0(before, e.output_rate, n)
        print(f"{setting}: frames {got[2]['frames']} voiced {got[2]['voiced']} median {got[2]['median_hz']}")
        assert got[0].shape == want[0].shape and _same(got, want)
        shift = 2.0 ** (3.0 / 12.0) if setting == "chain" else 1.0
        for b in (0, 1, 3, 4):
            assert got[2]["voiced"][b] >= got[2]["frames"][b] - 4 > 0
            assert abs(ref.cents(float(got[2]["median_hz"][b]), (95.0 + 40.0 * b) * shift)) < 10.0, (setting, b, got[2]["median_hz"][b])
        e.set_loudness(-16.0)  # normalization on or off reports the same signal
        try:
            assert _same(e.batch_f0(), got)
        finally:
            e.set_loudness(None)
        assert e.batch_fetch()[0].tobytes() == before.tobytes()
    finally:
        e.set_filters(None)
        e.set_output_rate(None)
        e.set_pitch(None)


def test_python_host_pools_a_joined_programme(batch):
    from supertonic_amd.tts import TextToSpeech
    a, e = batch
    tts = TextToSpeech(e, None, {"ae": {"sample_rate": a.sample_rate, "base_chunk_size": a.base_chunk_size},
                                 "ttl": {"chunk_compress_factor": a.chunk_compress_factor, "latent_dim": a.latent_dim}})
    rows = tts.pitch_report()
    f0, _, st = e.batch_f0()
    assert rows["f0"].tobytes() == f0.tobytes() and all(rows[k].tobytes() == st[k].tobytes() for k in st)
    prog = tts.pitch_report(rows=[2, 3])
    assert list(prog["frames"]) == [st["frames"][:2].sum(), st["frames"][2:].sum()] and list(prog["voiced"]) == [st["voiced"][:2].sum(), st["voiced"][2:].sum()]
    assert prog["min_hz"][0] == st["min_hz"][:2].min() and prog["max_hz"][1] == st["max_hz"][2:].max()


# ---- 5. the CLI ------------------------------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^Pitch: median (\d+\.\d{3}) Hz, min (\d+\.\d{3}) Hz, max (\d+\.\d{3}) Hz, voiced (\d+\.\d{3}) % \((\d+) of (\d+) frames\)$")


def _run(args, cwd):
    p = subprocess.run([CLI, "--synthetic", "--onnx-dir", "no_assets_here", "--seed", "7", "--total-step", "2"] + args, cwd=cwd, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return [re.sub(r"completed in \S+ sec", "completed", ln) for ln in p.stdout.splitlines()]


def test_cli_prints_one_line_per_file(tmp_path):
    plain = _run(["--n-test", "1", "--save-dir", "plain"], tmp_path)
    assert not any(ln.startswith("Pitch") for ln in plain)
    rep = _run(["--n-test", "1", "--save-dir", "plain", "--pitch-report"], tmp_path)
    assert [ln for ln in rep if not ln.startswith("Pitch:")] == plain  # nothing else changes
    at = [i for i, ln in enumerate(rep) if ln.startswith("Pitch:")]
    assert len(at) == 1 and rep[at[0] - 1].startswith("Saved: ")
    g = LINE.match(rep[at[0]])
    assert g, rep[at[0]]
    med, lo, hi, share, voiced, frames = (float(v) for v in g.groups())
    assert frames > 0 and voiced <= frames and abs(share - 100.0 * voiced / frames) < 1e-3 and (voiced == 0 or 60.0 <= lo <= med <= hi <= 500.0)


# ---- 6. the pitch stage, measured ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semitones", [4.0, -3.0])
def test_pitch_stage_moves_the_fundamental_by_the_interval(eng, semitones):
    """the device's shift and report against the float64 chain (tests/pitch_ref.py, then f0_ref.py): the medians within the device
    bound of the report (the largest over the reference track's frames)"""
    y_ref, (a, b) = pitch_chain(semitones)
    f_ref, _, lag, det = ref.track(y_ref, PITCH_HZ, detail=True)
    g = ref.plan(PITCH_HZ, y_ref.size)
    bound = max(ref.device_bound(det[t], int(lag[t]), g)[0] for t in range(len(lag)) if lag[t])
    want = ref.stats(f_ref)["median_hz"]
    y = eng.op_pitch(pitch_row(), PITCH_HZ, semitones)
    _, _, st = eng.op_f0(y, PITCH_HZ)
    got = float(st["median_hz"][0])
    print(f"{semitones:+} st ({a}/{b}): device median {got:.4f} Hz, float64 chain {want:.4f} Hz ({ref.cents(got, want):+.4f} cents), bound {bound:.3e} relative; "
          f"asked for {150.0 * 2.0 ** (semitones / 12.0):.4f} Hz")
    assert st["voiced"][0] >= st["frames"][0] - 2
    assert abs(got / want - 1.0) <= bound, (semitones, got, want, bound)
