"""Known model-rate rows for the output-stage tests that overwrite a finished batch (stn_dbg_batch_set_wav): every option of the stage
has something to do on them."""
import numpy as np

import limiter_ref


def rows(sr, W, spans, hz_out, ms, seed):
    """float32 [len(spans), W], row b's signal inside its first spans[b] samples and quiet noise everywhere, three kinds in turn.  Quiet:
    a low tone behind 60 ms and in front of 80 ms of silence (trimming cuts both; the loudness gain leaves it under the ceiling).  Tone:
    hz_out / 4 at 45 degrees to the output rate's sample instants in 6 ms bursts every 150 ms (loudness far under its peaks, true peak
    over its sample peak).  Clicky: limiter_ref.peaky_row (peaks the limiter turns down, none of it silent)."""
    rng = np.random.default_rng(seed)
    wav = (1e-5 * rng.standard_normal((len(spans), W))).astype(np.float32)
    t = np.arange(W) / sr
    for b, nb in enumerate(int(n) for n in spans):
        if b % 3 == 0:
            lo, hi = min(nb, int(0.06 * sr)), max(0, nb - int(0.08 * sr))
            wav[b, lo:hi] += (0.02 * np.sin(2 * np.pi * (200.0 + 30.0 * b) * t[lo:hi])).astype(np.float32)
        elif b % 3 == 1:
            envl = 0.004 + 0.3 * np.exp(-0.5 * (((t % 0.15) - 0.05) / 0.003) ** 2)
            wav[b, :nb] += (envl * np.sin(2 * np.pi * (hz_out / 4.0) * t + np.pi / 4))[:nb].astype(np.float32)
        else:
            wav[b] = limiter_ref.peaky_row(W, nb, 1.0, 0.1, limiter_ref.samples(sr, ms), seed + b)
    return wav
