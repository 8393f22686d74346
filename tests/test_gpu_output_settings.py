"""A call's OutputSettings go with the call: with all seven settings set on the instance, a call that overrides all seven, and a call
whose override the engine refuses part-way, both leave the engine with the instance's settings and the next call's bytes unchanged."""
import numpy as np
import pytest

from supertonic_amd import binding

pytestmark = pytest.mark.gpu

TEXT = "Every setting of a call leaves with the call."


def _in_force(engine):
    return (engine.output_rate, engine.get_filters(), engine.loudness, engine.loudness_ceiling, engine.silence_trim, engine.pause_limit,
            engine.limiter, engine.peak_mode)


def test_a_call_overriding_every_setting_and_a_refused_one_leave_the_instances_settings():
    from supertonic_amd import workload
    from supertonic_amd.arch import default_arch
    from supertonic_amd.tts import Style, load_text_to_speech
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, noise_seed=21, output_rate=16000, filters=[("highpass", 80, 0.5)],
                              loudness=(-16, -1.5), trim_silence=(40, 10, 0), max_pause=250, limiter=2, peak_mode="true")
    sttl, sdp = workload.synthetic_styles(default_arch(), [0])
    style = Style(sttl, sdp)
    own = _in_force(tts.engine)  # (16000, one high-pass, -16 LUFS under -1.5 dB, (40, 10, 0), 250 ms, 2 ms, true peak: all exact in fp32)
    assert own == (16000, (("highpass", 80.0, 0.5, 0.0),), -16.0, -1.5, (40.0, 10.0, 0.0), 250.0, 2.0, "true")
    before, _ = tts.batch([TEXT], ["en"], style, 2, 1.05)
    assert _in_force(tts.engine) == own
    # (a) every setting overridden at once, by another value or by off
    got, _ = tts.batch([TEXT], ["en"], style, 2, 1.05, output_rate=8000, filters=[("lowpass", 3000)], loudness=-23, trim_silence=False, max_pause=100,
                       limiter=False, peak_mode="sample")
    assert _in_force(tts.engine) == own and got.shape[1] != before.shape[1]
    # (b) the rate is accepted, then the chain is refused at it (6 kHz is above 8 kHz's Nyquist): a host-side argument check, nothing runs
    with pytest.raises(binding.StnError) as ei:
        tts.batch([TEXT], ["en"], style, 2, 1.05, output_rate=8000, filters=[("lowpass", 6000)], loudness=False, trim_silence=40, max_pause=False,
                  limiter=5, peak_mode="sample")
    assert "freq_hz" in str(ei.value) and _in_force(tts.engine) == own
    tts.noise_seed, tts._calls = 21, 0
    after, _ = tts.batch([TEXT], ["en"], style, 2, 1.05)
    tts.engine.close()
    assert after.dtype == before.dtype and after.shape == before.shape and after.tobytes() == before.tobytes()
