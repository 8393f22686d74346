"""The resampler's launch decision without a GPU (resample_form, kernels_resample.hip; stn_dbg_resample_form): the form string for
pairs that reach every G, the K-limited stop on short rows, the cache path, P = 640, and every pair of 40 common rates against the
rule restated here in Python (nothing is read back from the library but the taps per phase T, which the rule takes as given).

The rule.  out / in = P / Q reduced, W_out = ceil(W P / Q), K = ceil(W_out / P) output periods a row.  A workgroup of G groups reads
span(G) = (64 G - 1) Q + floor((P - 1) Q / P) + T samples.  G doubles from 1 while G P < 16 and 64 G < K and 4 span(2 G) <= 160 KiB;
the span is staged in LDS where 4 span(G) <= 160 KiB, else the row is read through the caches.

The 160 KiB stop.  Of the 1352 supported ordered pairs of COMMON (40 rates), none stops the doubling on the LDS condition: 1278 end
on G P >= 16 with the span in LDS and 74 are cache pairs at G = 1 (P >= 16 and Q > ~620).  The stop needs (128 G - 1) Q + T above 40960
words while G P < 16.  With Q / P at most 24 (192000 / 8000) that leaves P = 7 at G = 2 (Q >= 154) and P in 8 .. 15 at G = 1: a steep
decimation by an odd ratio, such as 192000 -> 8400 Hz (P / Q = 7 / 160, T = 1744: G stops at 2, not 4, because span(4) is 166 KiB).
That pair is asserted here and runs in tests/test_gpu_resample_forms.py although 8400 Hz is no common rate."""
import itertools
import math

import pytest

from supertonic_amd import binding

SR = 44100
LDS_MAX = 160 * 1024
COMMON = (8000, 8001, 9600, 11025, 12000, 14700, 16000, 18900, 22050, 24000, 25200, 28224, 29400, 32000, 33075, 36000, 37800, 40000,
          44056, 44100, 47250, 48000, 50000, 50400, 56000, 58800, 64000, 66150, 72000, 75600, 80000, 88200, 96000, 100000, 112000,
          128000, 132300, 144000, 176400, 192000)


def rule(in_hz, out_hz, W, T):
    """-> (form string, what ended the doubling: "P", "K" or "LDS", grid x)"""
    g = math.gcd(in_hz, out_hz)
    P, Q = out_hz // g, in_hz // g
    K = -(-(-(-W * P // Q)) // P)

    def span(G):
        return (64 * G - 1) * Q + (P - 1) * Q // P + T

    G = 1
    while True:
        if G * P >= 16:
            stop = "P"
            break
        if 64 * G >= K:
            stop = "K"
            break
        if 4 * span(2 * G) > LDS_MAX:
            stop = "LDS"
            break
        G *= 2
    return f"resample {'lds' if 4 * span(G) <= LDS_MAX else 'cache'} G{G}", stop, -(-K // (64 * G))


def _T(in_hz, out_hz):
    return binding.resample_filter(in_hz, out_hz).shape[1]


@pytest.mark.parametrize("in_hz,out_hz,W,form,stop", [
    (SR, 22050, 4097, "resample lds G16", "P"),      # P = 1
    (SR, 88200, 4097, "resample lds G8", "P"),       # P = 2
    (SR, 18900, 4097, "resample lds G8", "P"),       # P = 3: 8 * 3 >= 16 only after the third doubling
    (SR, 176400, 4097, "resample lds G4", "P"),      # P = 4
    (SR, 50400, 4097, "resample lds G2", "P"),       # P = 8
    (SR, 192000, 4097, "resample lds G1", "P"),      # P = 640 = RESAMPLE_MAX_P
    (SR, 8000, 4097, "resample lds G1", "P"),        # Q = 441: 112 KiB of span
    (SR, 8001, 20011, "resample cache G1", "P"),     # P / Q = 127 / 700: 177 KiB of span
    (192000, 8000, 98328, "resample lds G16", "P"),  # P / Q = 1 / 24, T = 1832
    (192000, 8400, 400000, "resample lds G2", "LDS"),  # P / Q = 7 / 160: span(4) = 166 KiB
    # short rows: 64 G >= K ends the doubling early (22050: K = ceil(W / 2))
    (SR, 22050, 1, "resample lds G1", "K"),
    (SR, 22050, 7, "resample lds G1", "K"),
    (SR, 22050, 128, "resample lds G1", "K"),   # K = 64
    (SR, 22050, 129, "resample lds G2", "K"),   # K = 65
    (SR, 22050, 300, "resample lds G4", "K"),   # K = 150
    (SR, 22050, 2048, "resample lds G16", "P"),  # K = 1024: 64 * 16 >= K would stop it too, P is asked first
    (SR, 22050, 2047, "resample lds G16", "P"),
    (SR, 22050, 1024, "resample lds G8", "K"),  # K = 512
    (SR, 176400, 65, "resample lds G2", "K"),   # K = 65, P = 4
])
def test_form_of_the_named_pairs(in_hz, out_hz, W, form, stop):
    assert binding.resample_form(in_hz, out_hz, W) == form
    assert rule(in_hz, out_hz, W, _T(in_hz, out_hz))[:2] == (form, stop)


def test_p_640_is_the_last_accepted():
    assert binding.resample_filter(SR, 192000).shape == (640, 80)
    assert binding.resample_form(SR, 192000, 1) == "resample lds G1"
    for bad in ((SR, 44101, 100), (SR, 192001, 100), (SR, 22050, 0), (SR, 22050, -3)):
        with pytest.raises(binding.StnError) as e:
            binding.resample_form(*bad)
        why = binding.resample_error(*bad[:2])  # the refusal names its reason: the pair's, or the width
        assert (why in str(e.value)) if why else ("W >= 1" in str(e.value)), str(e.value)


def test_every_pair_of_the_common_rates_follows_the_rule():
    assert len(COMMON) == 40 and len(set(COMMON)) == 40
    stops, forms, n = {}, set(), 0
    for in_hz, out_hz in itertools.permutations(COMMON, 2):
        if binding.resample_error(in_hz, out_hz):
            continue
        n += 1
        T = _T(in_hz, out_hz)
        for W in (1, 4099, 10 ** 6):
            form, stop, _ = rule(in_hz, out_hz, W, T)
            assert binding.resample_form(in_hz, out_hz, W) == form, (in_hz, out_hz, W)
        forms.add(form)
        key = (stop, form.split()[1])
        stops[key] = stops.get(key, 0) + 1
    assert n == 1352
    assert stops == {("P", "lds"): 1278, ("P", "cache"): 74}  # no pair of the list stops on the 160 KiB condition (module docstring)
    assert forms == {f"resample lds G{g}" for g in (1, 2, 4, 8, 16)} | {"resample cache G1"}
