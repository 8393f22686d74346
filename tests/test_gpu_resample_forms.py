"""Every form of the output-rate resampler on an MI355X (kernels_resample.hip; the form is resample_form's, asserted first in every
case as stn_dbg_resample_form reports it) against float64 and against the tap table itself.

Cases (input 44100 Hz unless noted): 22050 (G16), 88200 (G8), 18900 (P = 3, G8), 176400 (G4), 50400 (G2), 192000 (P = 640, the refusal
boundary, G1), 8000 (Q = 441, G1), 8001 (the cache path), 192000 -> 8000 (P / Q = 1 / 24, T = 1832, G16) and 192000 -> 8400 (P / Q =
7 / 160: the one stop of the doubling on the 160 KiB condition, G2; tests/test_resample_form_cpu.py says why no common rate has it).

1. Float64.  Rows of scale 1, of scale 1e-3 and of scale 1 with a spike of 1e3, at W in {1, 7, 63 Q + 1, 4097, 4099} and at a width
   of three workgroups in x.  The kernel sums T products as eight FMA chains of T / 8 terms and a three-level tree, so
   |y - ref| <= (T / 8 + 3) 2^-24 sum_j |tap_j x_j| * 1.01 per output (the sum in float64; 1.01 holds the second-order terms); the former
   absolute 2e-6 stays asserted on the row of scale 1.
2. Exact impulses.  Rows that are zero but for samples of +-1 and +-0.5 more than T apart: every output then holds at most one
   non-zero product, every FMA and every add of the tree is exact, and y[n] must equal amp * taps[(n Q) mod P][p - first(n)] as a
   value, 0 where no impulse lies under the window.  Row 0 carries impulses at sample 0, at W - 1 and on a lattice whose step is
   coprime to Q, so that every residue mod Q occurs away from the row's ends; rows 1 to 5 carry one impulse per workgroup at the
   first staged sample k0 Q - off, the samples before and after it, the last staged sample and the one behind it.  The test counts
   the (phase, tap) entries the expected outputs read and asserts that all P T of them were read in every case.  The int16 PCM
   epilogue of the same rows must equal the PCM rule on the fp32 output.

Measured on an MI355X (the bound is never taken from these), worst |y - ref| / bound over all widths and rows: 22050 G16 0.150, 88200 G8
0.319, 18900 G8 0.159, 176400 G4 0.282, 50400 G2 0.261, 192000 G1 0.287, 8000 G1 0.108, 8001 cache 0.085, 192000 -> 8000 G16 0.064,
192000 -> 8400 G2 0.045; the unit row's largest |y - ref| stayed under 1.2e-7.  Every impulse case returned the table exactly, all
P T entries read (160 entries at 22050 up to 53848 at 8001).  Wall time of the file: 1.8 s for its 20 cases, none above 0.3 s."""
import math

import numpy as np
import pytest

from supertonic_amd import binding

pytestmark = pytest.mark.gpu
SR = 44100
U = 2.0 ** -24

# (in_hz, out_hz, the form at a width of three workgroups or more)
CASES = [
    (SR, 22050, "resample lds G16"),
    (SR, 88200, "resample lds G8"),
    (SR, 18900, "resample lds G8"),
    (SR, 176400, "resample lds G4"),
    (SR, 50400, "resample lds G2"),
    (SR, 192000, "resample lds G1"),
    (SR, 8000, "resample lds G1"),
    (SR, 8001, "resample cache G1"),
    (192000, 8000, "resample lds G16"),
    (192000, 8400, "resample lds G2"),
]
IDS = [f"{i}-{o}" for i, o, _ in CASES]


def _pq(in_hz, out_hz):
    g = math.gcd(in_hz, out_hz)
    return out_hz // g, in_hz // g


def _geometry(in_hz, out_hz, form):
    P, Q = _pq(in_hz, out_hz)
    taps = binding.resample_filter(in_hz, out_hz)
    assert taps.shape[0] == P
    return P, Q, taps.shape[1], int(form.rsplit("G", 1)[1]), taps


def _three_groups(Q, G):
    """the smallest W whose K = ceil(ceil(W P / Q) / P) is 128 G + 5: three workgroups of 64 G output periods, the last one short"""
    return (128 * G + 4) * Q + 1


def pcm_rule(y):
    """writeWavFile's conversion in fp32: clamp to [-1, 1], * 32767, truncation toward zero."""
    return (np.clip(np.asarray(y, np.float32), -1.0, 1.0) * np.float32(32767.0)).astype(np.int32).astype(np.int16)


def ref_and_mass(x, taps, P, Q):
    """float64: y[n] = sum_j taps[(n Q) mod P][j] x[floor(n Q / P) - (T / 2 - 1) + j] (0 outside the row) and sum_j |taps x|"""
    taps = taps.astype(np.float64)
    T = taps.shape[1]
    x = np.atleast_2d(np.asarray(x, np.float64))
    rows, W = x.shape
    Wo = -(-W * P // Q)
    off = T // 2 - 1
    pad = np.zeros((rows, W + 2 * T + Q + 8))
    pad[:, T:T + W] = x
    y, mass = np.empty((rows, Wo)), np.empty((rows, Wo))
    step = max(1, (1 << 20) // T)
    for s in range(0, Wo, step):
        n = np.arange(s, min(Wo, s + step), dtype=np.int64)
        ph, base = (n * Q) % P, (n * Q) // P - off + T
        win = pad[:, base[:, None] + np.arange(T)[None, :]]
        y[:, s:s + len(n)] = np.einsum("rnt,nt->rn", win, taps[ph])
        mass[:, s:s + len(n)] = np.einsum("rnt,nt->rn", np.abs(win), np.abs(taps[ph]))
    return y, mass


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


@pytest.mark.parametrize("in_hz,out_hz,form", CASES, ids=IDS)
def test_every_form_against_float64(eng, in_hz, out_hz, form):
    P, Q, T, G, taps = _geometry(in_hz, out_hz, form)
    W3 = _three_groups(Q, G)
    assert binding.resample_form(in_hz, out_hz, W3) == form
    K3 = -(-(-(-W3 * P // Q)) // P)
    assert -(-K3 // (64 * G)) == 3  # three workgroups in x
    rng = np.random.default_rng(out_hz + in_hz)
    worst = 0.0
    for W in (1, 7, 63 * Q + 1, 4097, 4099, W3):
        x = rng.uniform(-1, 1, (3, W))
        x[1] *= 1e-3
        x[2, (W * 5) // 8] = 1e3 if W % 2 else -1e3
        x = x.astype(np.float32)
        y = eng.op_resample(x, in_hz, out_hz)
        ref, mass = ref_and_mass(x, taps, P, Q)
        assert y.shape == ref.shape and np.all(np.isfinite(y))
        err = np.abs(y.astype(np.float64) - ref)
        bound = (T // 8 + 3) * U * mass * 1.01
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        worst = max(worst, ratio)
        print(f"{in_hz} -> {out_hz} ({binding.resample_form(in_hz, out_hz, W)}), W {W}: worst |y - ref| / bound {ratio:.3f}, "
              f"unit row max |y - ref| {err[0].max():.3g}")
        assert np.all(err <= bound), (W, ratio)
        assert err[0].max() <= 2e-6, (W, float(err[0].max()))
        assert np.array_equal(eng.op_resample(x, in_hz, out_hz, pcm=True), pcm_rule(y)), W
    print(f"{in_hz} -> {out_hz} {form}: worst |y - ref| / bound over the widths {worst:.3f}")


def _impulse_rows(P, Q, T, G, off):
    """x [6, W] float32, the impulses as (row, position, amplitude)"""
    S = T + 1
    while math.gcd(S, Q) != 1:
        S += 1
    W = max((Q + 1) * S + 1, (256 * G + 4) * Q + 1)  # five workgroups or more: the ends of the first spans lie inside the row
    K = -(-(-(-W * P // Q)) // P)
    blocks = -(-K // (64 * G))
    assert blocks >= 5
    span = (64 * G - 1) * Q + (P - 1) * Q // P + T
    amps = (1.0, -0.5, -1.0, 0.5)
    imp = []
    lattice = list(range(0, W - 1 - S + 1, S)) + [W - 1]
    assert len(lattice) >= Q + 2 and {p % Q for p in lattice[1:-1]} == set(range(Q))  # every residue, away from the row's ends
    imp += [(0, p, amps[i % 4]) for i, p in enumerate(lattice)]
    for row, delta in ((1, -1), (2, 0), (3, 1)):  # around the first sample a workgroup stages
        imp += [(row, b * 64 * G * Q - off + delta, amps[(b + row) % 4]) for b in range(blocks)]
    for row, delta in ((4, 0), (5, 1)):  # the last sample a workgroup stages, and the one behind it
        imp += [(row, b * 64 * G * Q - off + span - 1 + delta, amps[(b + row) % 4]) for b in range(blocks)]
    imp = [(r, p, a) for r, p, a in imp if 0 <= p < W]
    x = np.zeros((6, W), np.float32)
    for r in range(6):
        pos = sorted(p for rr, p, _ in imp if rr == r)
        assert len(pos) >= 2 and min(np.diff(pos)) > T, (r, pos[:4])  # more than T apart: one product per output at the most
    for r, p, a in imp:
        x[r, p] = a
    return x, imp


@pytest.mark.parametrize("in_hz,out_hz,form", CASES, ids=IDS)
def test_impulses_return_the_table_exactly(eng, in_hz, out_hz, form):
    P, Q, T, G, taps = _geometry(in_hz, out_hz, form)
    off = T // 2 - 1
    x, imp = _impulse_rows(P, Q, T, G, off)
    W = x.shape[1]
    assert binding.resample_form(in_hz, out_hz, W) == form
    Wo = -(-W * P // Q)
    assert np.array_equal((taps * np.float32(0.5)) * np.float32(2.0), taps)  # halving a tap is exact (none is subnormal)
    want = np.zeros((6, Wo), np.float32)
    read = np.zeros((P, T), bool)
    for r, p, a in imp:
        # outputs n whose window [first(n), first(n) + T) holds p: floor(n Q / P) in (p + off - T, p + off]
        lo, hi = max(0, p + off - T + 1), p + off
        n = np.arange(-(-lo * P // Q), min(Wo, -(-(hi + 1) * P // Q)), dtype=np.int64)
        ph, j = (n * Q) % P, p - ((n * Q) // P - off)
        assert np.all((j >= 0) & (j < T)) and np.all(want[r, n] == 0)
        want[r, n] = np.float32(a) * taps[ph, j]
        read[ph, j] = True
    # `read` counts the entries the expectation is made of, not loads on the device: it shows that the impulses reach the whole table, and
    # the comparison below, exact at every output, then shows that the kernel read each of them (and nothing else: zeros elsewhere)
    assert read.all(), f"{np.count_nonzero(~read)} of {P * T} table entries not reached by any impulse"
    y = eng.op_resample(x, in_hz, out_hz)
    assert y.shape == want.shape
    # as values: != takes -0.0 for +0.0, which is what the contract asks (the chains start from +0.0 and add tap * 0 products of either
    # sign under negative taps and amplitudes; whatever sign the zero ends with is no error)
    bad = np.argwhere(y != want)
    assert bad.size == 0, (form, len(bad), bad[:5].tolist())
    assert np.array_equal(eng.op_resample(x, in_hz, out_hz, pcm=True), pcm_rule(want))
    print(f"{in_hz} -> {out_hz} {form}: {len(imp)} impulses over 6 x {W} samples, all {P * T} (phase, tap) entries read and returned exactly")
