"""The loudness kernel tests' own ground, without a GPU: the pass-by-pass float64 reference (tests/loudness_ref.py: cascade_states,
chunk_shares, gate_from_segments) restates BS.1770-4 and not the kernels; the scan's power table (stn_loudness_table) is the matrix
power it claims to be; and the bounds tests/test_gpu_loudness_kernels.py holds each pass to (tests/loudness_cases.py) are sharp: a
decomposition that loses the scan's carry, drops the next-segment share or drops a chunk misses them by at least 10 x on the rows used."""
import math

import numpy as np
import pytest

from supertonic_amd import binding
import loudness_cases as lc
from loudness_ref import CHUNK, cascade_states, chunk_shares, coef_of, gate_from_segments, integrated_loudness, segments_from_shares


@pytest.mark.parametrize("hz", lc.RATES)
def test_reference_equals_the_scipy_reference(hz):
    """cascade_states + chunk_shares + gate_from_segments with the float64 coefficients against integrated_loudness (scipy lfilter on the
    same coefficients, segments by reshape): 1e-9 LU, and undefined where that one is undefined."""
    x, n = lc.signals(hz)
    _, _, y = cascade_states(x, coef_of(hz), n)
    defined = 0
    for r in range(6):
        pa, pb = chunk_shares(np.nan_to_num(y[r]), n[r], lc.hop(hz))
        L, gain, _ = gate_from_segments(segments_from_shares(pa, pb, n[r], lc.hop(hz)), lc.hop(hz))
        want = integrated_loudness(x[r, : n[r]].astype(np.float64), hz)
        assert gain == 1.0
        if math.isinf(want):
            assert L == -math.inf, (hz, r)
        else:
            defined += 1
            assert abs(L - want) <= 1e-9, (hz, lc.NAMES[r], L, want)
    assert defined >= 1


def _kinds(n, h):
    seen = set()
    for v in n:
        seen.add(int(v))
        if v and v % h == 0:
            seen.add("hop")
        if v > 1 and v % h == 1:
            seen.add("hop+1")
        if v % h == h - 1:
            seen.add("hop-1")
        if v % 4:
            seen.add(f"mod4={v % 4}")  # with W % 4 == 0: the 16-byte path's last load runs past n
    return seen


def test_the_lengths_walk_every_boundary():
    kinds = {"hop", "hop+1", "hop-1", "mod4=1", "mod4=2", "mod4=3"}
    seen = set()
    for hz in lc.RATES:
        n, h, w = lc.lengths(hz), lc.hop(hz), lc.width(hz)
        assert w % 4 == 0 and w % lc.TILE == 40 and w // h >= 10  # at least 7 gating blocks in a full row
        assert np.all(n <= w) and n[lc.SHORT] == 4 * h - 1 and n[lc.EMPTY] == 0
        assert n.max() > w // lc.TILE * lc.TILE + CHUNK  # a chunk beyond the last full tile
        seen |= _kinds(n, h)
        if hz in lc.HIGH:  # each of these rates walks the hop and the 16-byte tail by itself, on rows long enough to have a loudness
            long_rows = n[[lc.TONE, lc.NOISE, lc.QUIET_LOUD, lc.ZERO]]
            assert _kinds(long_rows, h) >= kinds and long_rows.min() >= 9 * h - 1, (hz, n)
    assert [lc.width(hz) for hz in lc.RATES] == [lc.W] * 7 + [lc.W_WIDE] * 2 and lc.W == 3 * 32768 + 40 and lc.W_WIDE == 6 * 32768 + 40
    assert set(lc.STRADDLING) == {hz for hz in lc.RATES if lc.hop(hz) % CHUNK}
    assert seen >= set(lc.REQUIRED_LENGTHS) | kinds, seen


def test_gate_margins_of_the_rows():
    """no 400 ms block of any row lies within 1e-4 LU of a gate threshold (the GPU test asserts the same of the device's own segments), and
    at every rate the relative gate removes blocks of the quiet-then-loud row"""
    for hz in lc.RATES:
        c = lc.case(hz)
        for r in range(6):
            assert c.gate[r][2] >= 1e-4, (hz, lc.NAMES[r], c.gate[r])
        seg = c.ref["seg"][lc.QUIET_LOUD]
        z = ((seg[:-3] + seg[1:-2]) + (seg[2:-1] + seg[3:])) / (4.0 * c.hop)
        L = c.gate[lc.QUIET_LOUD][0]
        assert np.isfinite(L) and abs(L - (-0.691 + 10 * math.log10(z.mean()))) > 1.0, hz  # ungated, the mean reads lower


TABLE_ULPS = 2.0


@pytest.mark.parametrize("hz", [8000, 11025, 16000, 22050, 44100, 48000, 192000])
def test_power_table(hz):
    """mpow[i] = A^(32 (i + 1)) of the fp32 coefficients, A the zero-input transition of the state (s1, s2, t1, t2), for i = 0, 1, 255,
    1022, 1023.  The unit is what one final rounding to fp32 can cost: half an ulp of the entry, at most 2^-24 of the matrix's largest
    entry (plus half the smallest subnormal, 2^-150, once the power has decayed that far: at 44.1 kHz M^1024 is all zeros).  The table
    is held to TABLE_ULPS = 2 units against the exact power: one for that rounding, one for the float64 product chain in front of it.
    The chain needs an allowance of its own because the high-pass has a nearly double pole (Q = 0.5003), so A is nearly defective and
    float64 products of its powers lose up to eight digits: numpy's matrix_power by squaring is off by up to 2e-5 of the largest entry,
    the engine's sequential chain by 1.1e-7 at most where the entry is still representable.  So the reference here is not a float64 power
    but the power in 200-bit arithmetic (mpmath), which is exact to every digit float64 shows.
    Measured: the table is within 0.97 units at every rate and entry (worst 22050 Hz, i = 255); the chain alone within 0.24."""
    import mpmath
    coef, mpow, h = binding.loudness_table(hz)
    assert h == (hz + 5) // 10 and coef.dtype == np.float32 and mpow.shape == (1024, 4, 4)
    assert np.array_equal(coef, coef_of(hz).astype(np.float32))
    c = coef.astype(np.float64)
    A = np.array([[-c[3], 1, 0, 0],
                  [-c[4], 0, 0, 0],
                  [c[6] - c[8] * c[5], 0, -c[8], 1],
                  [c[7] - c[9] * c[5], 0, -c[9], 0]])
    # A is what one sample of cascade_states does to a state with u = 0
    s = np.array([0.3, -0.2, 0.7, 0.4])
    v = s[0]
    yy = c[5] * v + s[2]
    step = np.array([s[1] - c[3] * v, -c[4] * v, (c[6] * v + s[3]) - c[8] * yy, c[7] * v - c[9] * yy])
    assert np.abs(A @ s - step).max() <= 1e-15
    worst = 0.0
    with mpmath.workprec(200):
        Am = mpmath.matrix(4, 4)
        Am[0, 0], Am[0, 1], Am[1, 0] = -mpmath.mpf(c[3]), 1, -mpmath.mpf(c[4])
        Am[2, 0], Am[2, 2], Am[2, 3] = mpmath.mpf(c[6]) - mpmath.mpf(c[8]) * mpmath.mpf(c[5]), -mpmath.mpf(c[8]), 1
        Am[3, 0], Am[3, 2] = mpmath.mpf(c[7]) - mpmath.mpf(c[9]) * mpmath.mpf(c[5]), -mpmath.mpf(c[9])
        for i in (0, 1, 255, 1022, 1023):
            P = Am ** (CHUNK * (i + 1))
            unit = mpmath.mpf(2) ** -24 * max(abs(P[r, q]) for r in range(4) for q in range(4)) + mpmath.mpf(2) ** -150
            err = max(abs(mpmath.mpf(float(mpow[i, r, q])) - P[r, q]) for r in range(4) for q in range(4))
            worst = max(worst, float(err / unit))
            assert err <= TABLE_ULPS * unit, (hz, i, float(err), float(unit))
    print(f"\n{hz} Hz: power table within {worst:.2f} x (2^-24 max|entry| + 2^-150) of the exact power")


def test_table_refuses_rates_out_of_range():
    for bad in (7999, 192001, 0):
        with pytest.raises(binding.StnError):
            binding.loudness_table(bad)


# ---- sharpness: each fault of a float64 model of the decomposition against the bound of the pass it breaks ---------------------------
def _ratio(c, got, keys):
    d = lc.deviations(c, got)
    return max(d[k] / c.bound[k] for k in keys)


@pytest.mark.parametrize("hz", lc.RATES)
def test_bounds_see_every_injected_fault(hz):
    """The faults a tolerance of 0.01 LU on L lets through, each against the bound of the pass it breaks, at every rate at which the
    fault changes anything:
      the scan's carry lost at every tile (state zeroed every 32768 samples) and beyond a workgroup span (every 8192): the scan bound;
      the next-segment share dropped: the pa / pb bound and the segment bound, at the rates whose hop is no multiple of 32 (at 8 and
        48 kHz no chunk straddles, pb is all zeros and there is nothing to drop: the GPU test asserts those zeros exactly);
      the last chunk of the last whole segment dropped: the pa / pb bound.
    Every one misses its bound by at least 10 x; the change of L it causes is printed next to that.
    One pair cannot reach 10 x, by arithmetic and not by the choice of rows: the dropped share against the segment bound at 176.4 kHz.  A
    chunk hands at most 31 samples to the next segment (24 there: the boundaries fall 8, 16 and 24 samples into a chunk) out of hop =
    17640, and a tone's y^2 is at most twice its mean, so the fault moves a segment by at most about 2 * 31 / 17640 = 3.5e-3 of the
    largest one (2.7e-3 on these rows, the tone row), while the fp32 restatement itself moves the tone row's segments by 1.5e-4 and the
    bound is 4 x that: 10 x the bound is 6.2e-3, more than the fault can be.  The pass that breaks is held to the share bound, which the
    fault misses by 43 x there; against the segment bound it is asserted to fail (ratio above 1; 4.3 on the float64 model) and the
    ratio is printed, so the segment check alone is about 4 x sharp at that rate."""
    c = lc.case(hz)
    assert all(v > 0 for v in c.bound.values())
    lines = []
    faults = [("tile carry lost", lc.fault_lost_carry(c, lc.TILE), ("start",)),
              ("carry lost every span", lc.fault_lost_carry(c, lc.SPAN), ("start",)),
              ("last chunk dropped", lc.fault_last_chunk_dropped(c), ("share",))]
    if hz in lc.STRADDLING:
        pbd = lc.fault_pb_dropped(c)
        faults += [("pb dropped (shares)", pbd, ("share",)), ("pb dropped (segments)", pbd, ("seg",))]
    else:
        assert c.hop % CHUNK == 0 and not c.ref["pb"].any()
    for name, got, keys in faults:
        ratio = _ratio(c, got, keys)
        dL = max(abs(lc.loudness_of(c, got, r) - c.gate[r][0]) for r in range(6) if np.isfinite(c.gate[r][0]))
        lines.append(f"{name}: {ratio:.0f} x its bound, moves L by {dL:.4f} LU")
        need = 10.0
        if hz == 176400 and name == "pb dropped (segments)":
            assert 10.0 * c.bound["seg"] > 2 * 31 / c.hop  # out of the fault's reach (docstring); it still has to fail the bound
            need = 1.0 + 1e-9
        assert ratio >= need, (hz, name, ratio)
    print(f"\n{hz} Hz: " + "; ".join(lines))
