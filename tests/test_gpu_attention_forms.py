"""Every form of the engine's attention launchers (csrc/kernels_attn.hip: attn_mfma_kernel, attn_kernel<T, TPR> with its fp32 staging
variants, rope_rows_kernel; csrc/kernels_xattn_hs.hip: xattn_hs_kernel<F16, U> and hs_pairs_kernel) against float64 on operands rounded
to the engine's format, in the layouts the engine runs (fused QKV rows, packed query and key rows, K/V of block blk of an nb*2C row, keys
rotated once beforehand), through stn_op_attention_ex and stn_op_xattn_hs.  Each case first asserts the form it expects, so a heuristic
change that moves a shape to another kernel fails here instead of silently losing coverage.  The reference rounds where each kernel
rounds: the scalar kernel only its output (and rope_rows its rotated keys); the MFMA kernel also q after rotation and scaling, keys rotated
in the kernel, and the exponentials of the P V product (not those of the row sum); the head-split kernel q after the projection and
again after rotation and scaling, the exponentials, the attention output and the per-head partial sums.

Bounds (one reason each; "measured" = the largest value over every case here on an MI355X):
  * fp32 outputs: max |d| <= F32_REL rms(ref): fp32 rotation, dot products and online softmax in another order than float64.
    Measured 2.6e-5; bound 1e-4.
  * 16-bit outputs: |d| <= 1 ulp of the output format at |ref| (its one rounding) plus FLOOR_ULPS ulps at rms(ref).  The floor is
    not 0: where fp32 and float64 put an intermediate (a rotated or projected q, a pre-rotated key, an exponential, the head-split O)
    on opposite sides of a rounding midpoint, that flip moves every output it feeds by a fraction of an ulp of that intermediate,
    i.e. of the output's scale, not of each element's own magnitude.  Measured: attention 1.9 (bf16) / 2.4 (half), head-split 2.1
    (bf16) / 2.75 (half) ulps at rms; bounds 4 and 6.
  * 16-bit outputs: the share of a launch's outputs that differ from the rounded float64 value at all <= FRAC_DIFFER: the same flips
    (one flipped head-split O element changes a whole 384-wide row).  Measured per sequence at most 3.6 % (bf16) / 13 % (half) for
    attention, 8.7 % / 29 % for the head-split rows of a one-row utterance; bounds per launch 10 % / 30 %.
  * rope_rows' rotated keys: <= 1 ulp of the storage format plus the fp32 bound above (one rounding of an fp32 rotation).
  * Everything outside the rows and columns a launch owns (NaN sentinels), key/value rows past a context's end (NaN: never read into a
    result), what rope_rows must not touch, a sequence's bits across batch positions and batch contents, and two launches: exact."""
import numpy as np
import pytest

from supertonic_amd import binding

pytestmark = pytest.mark.gpu

SENTINEL_BITS = 0x7FC00000  # the canonical quiet NaN: survives the round trip through bf16 / half bit for bit
SENTINEL = np.array([SENTINEL_BITS], np.uint32).view(np.float32)[0]
BASE, GAMMA = 10000.0, 10.0  # the engine's defaults without a model (op entry points)
LOG2E = 1.4426950408889634
F32_REL = 1e-4
FLOOR_ULPS = {"attn": 4, "hs": 6}
FRAC_DIFFER = {"bf16": 0.1, "f16": 0.3}
HS_C, HS_H, HS_DH = 384, 4, 96


@pytest.fixture(scope="module")
def eng():
    return binding.Engine(0, "bf16")


# ---- float64 model ----------------------------------------------------------------------------------------------------------------
def rnd(x, fmt):
    """Round to the engine's format: bf16 round-to-nearest-even, IEEE half, or fp32 (float64 out)."""
    x = np.asarray(x)
    if fmt == "bf16":
        u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
        return u.astype(np.uint32).view(np.float32).astype(np.float64)
    if fmt == "f16":
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)
    return np.asarray(x, np.float32).astype(np.float64)


def ulp(x, fmt):
    e = np.floor(np.log2(np.maximum(np.abs(x), 1e-300)))
    if fmt == "bf16":
        return np.exp2(np.maximum(e, -126) - 7)
    return np.exp2(np.maximum(e, -14) - 10)


def rope64(x, n, mode, dh):
    """x [n_rows, H, dh] of one sequence (rows = positions 0..), rotated as the kernels do (pairs i, i + dh/2), float64"""
    if mode < 0:
        return x
    # the angle as the kernels form it, in fp32 (position, frequency, their product: at ~300 rad its rounding alone moves a 16-bit
    # rounding of the rotated value); its sine and cosine in float64
    rows = x.shape[0]
    pos = np.arange(rows, dtype=np.float32)
    if mode == 1:
        pos = np.float32(GAMMA) * pos / np.float32(max(int(n), 1))
    inv = np.exp(-np.float32(np.log(np.float32(BASE))) * np.float32(2) * np.arange(dh // 2, dtype=np.float32) / np.float32(dh))
    ang = (pos[:, None] * inv[None, :].astype(np.float32)).astype(np.float64)
    c, s = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]
    a0, a1 = x[..., :dh // 2], x[..., dh // 2:]
    return np.concatenate([a0 * c - a1 * s, a1 * c + a0 * s], axis=-1)


def attn_ref(q, k, v, nq, nk, mode, dh, fmt, mfma, k_pre):
    """One sequence: q [Lq_s, H, dh], k / v [nk, H, dh] (rounded operands, float64).  nq: the length-aware q length."""
    Lq_s, H = q.shape[0], q.shape[1]
    if nk <= 0:
        return np.zeros((Lq_s, H, dh))
    qr = rope64(q, nq, mode, dh)
    if k_pre:
        kr = rnd(rope64(k, nk, mode, dh), fmt)  # rope_rows: one rounding to the storage format
    elif mfma:
        kr = rnd(rope64(k, nk, mode, dh), fmt) if mode >= 0 else k
    else:
        kr = rope64(k, nk, mode, dh)
    if mfma:
        qs = rnd(qr * (LOG2E / np.sqrt(dh)), fmt)
        s = np.einsum("qhd,khd->hqk", qs, kr)
        p = np.exp2(s - s.max(axis=2, keepdims=True))
        o = np.einsum("hqk,khd->qhd", rnd(p, fmt), v) / p.sum(axis=2).T[:, :, None]
    else:
        s = np.einsum("qhd,khd->hqk", qr / np.sqrt(dh), kr)
        p = np.exp(s - s.max(axis=2, keepdims=True))
        o = np.einsum("hqk,khd->qhd", p, v) / p.sum(axis=2).T[:, :, None]
    return o


STATS = {}


def check_vals(got, ref, fmt, what, kind="attn"):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert np.all(np.isfinite(got)), what
    if ref.size == 0:
        return
    rms = np.sqrt(np.mean(ref ** 2)) + 1e-30
    d = np.abs(got - ref)
    st = STATS.setdefault((kind, fmt), {"rel": 0.0, "ulps": 0.0, "frac": 0.0})
    if fmt == "f32":
        st["rel"] = max(st["rel"], float(d.max() / rms))
        assert d.max() <= F32_REL * rms, (what, d.max() / rms)
        return
    u_rms = ulp(rms, fmt)
    need = float(np.max((d - ulp(ref, fmt)) / u_rms))  # the floor, in ulps at rms(ref), that 1 ulp at |ref| leaves to cover
    st["ulps"] = max(st["ulps"], need)
    assert np.all(d <= ulp(ref, fmt) + FLOOR_ULPS[kind] * u_rms), (what, need)
    return got != rnd(ref, fmt)


def check_frac(differ, fmt, what):
    """the share of a launch's 16-bit outputs that differ from the rounded reference"""
    if fmt == "f32" or not differ:
        return
    frac = float(np.mean(np.concatenate([np.ravel(x) for x in differ])))
    st = STATS.setdefault(("launch", fmt), {"frac": 0.0})
    st["frac"] = max(st["frac"], frac)
    assert frac <= FRAC_DIFFER[fmt], (what, frac)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- one attention in a given layout ------------------------------------------------------------------------------------------------
class Layout:
    """Buffers of one attention call.  kind: dense (q [B*Lq, ldq], kv [B*Lk, ldk] with K, V side by side), self (fused QKV rows, packed
    q and k, ld 3C), text (packed q; K/V of block blk of an nb*2C row, packed keys rotated beforehand by rope_rows over all nb groups),
    style (packed q; dense keys of block blk of an nb*2C row)."""

    def __init__(self, kind, B, Lq, Lk, H, dh, fmt, rng, qlen=None, klen=None, q_pad=0, kv_pad=0, o_pad=0, q_col=0, nb=4, blk=2,
                 scale=1.0, gap=3):
        C = H * dh
        self.kind, self.B, self.Lq, self.Lk, self.H, self.dh, self.C, self.fmt = kind, B, Lq, Lk, H, dh, C, fmt
        self.qlen = None if qlen is None else np.asarray(qlen, np.int32)
        self.klen = None if klen is None else np.asarray(klen, np.int32)
        self.q_off = self.k_off = None
        self.rot = dict(rot_groups=1, rot_stride=0, rot_col=None)
        nkq = lambda b: Lq if self.qlen is None else int(self.qlen[b])  # noqa: E731
        nkk = lambda b: Lk if self.klen is None else min(int(self.klen[b]), Lk)  # noqa: E731
        self.nq, self.nk = nkq, nkk
        if kind == "dense":
            self.ldq, self.ldk, self.ldo = q_col + C + q_pad, 2 * C + kv_pad, C + o_pad
            self.q_col, self.k_col, self.v_col = q_col, 0, C
            qrows, krows = B * Lq, B * Lk
            self.qrow0 = [b * Lq for b in range(B)]
            self.qn = [Lq] * B  # rows of q / o each sequence owns
            self.krow0 = [b * Lk for b in range(B)]
        else:
            offs, r = [], 2
            for b in range(B):
                offs.append(r)
                r += nkq(b) + gap
            self.q_off = np.asarray(offs, np.int32)
            qrows = r + 2
            self.qrow0, self.qn = list(offs), [nkq(b) for b in range(B)]
            if kind == "self":
                self.ldq = self.ldk = 3 * C + kv_pad
                self.ldo = C + o_pad
                self.q_col, self.k_col, self.v_col = 0, C, 2 * C
                self.k_off, self.krow0, krows = self.q_off, list(offs), qrows
            else:
                self.ldq, self.ldo = C + q_pad, C + o_pad
                self.ldk = nb * 2 * C + kv_pad
                self.q_col, self.k_col, self.v_col = 0, blk * 2 * C, blk * 2 * C + C
                if kind == "text":
                    koffs, r = [], 1
                    for b in range(B):
                        koffs.append(r)
                        r += nkk(b) + gap
                    self.k_off, self.krow0, krows = np.asarray(koffs, np.int32), koffs, r + 1
                    self.rot = dict(rot_groups=nb, rot_stride=2 * C, rot_col=0)
                else:
                    self.krow0, krows = [b * Lk for b in range(B)], B * Lk
        self.qrows, self.krows = qrows, krows
        # q: random everywhere (what lies outside the heads is never read); kv: random K/V of valid key rows, NaN elsewhere
        self.q = (scale * rng.standard_normal((qrows, self.ldq))).astype(np.float32)
        if kind == "self":
            self.q = np.full((qrows, self.ldq), SENTINEL, np.float32)
        self.kv = np.full((krows, self.ldk), SENTINEL, np.float32)
        for b in range(B):
            n = nkk(b)
            r0 = self.krow0[b]
            if kind == "text":  # every group's K and V of the valid rows (rope_rows rotates all groups' keys)
                self.kv[r0:r0 + n, :nb * 2 * C] = scale * rng.standard_normal((n, nb * 2 * C))
            else:
                self.kv[r0:r0 + n, self.k_col:self.k_col + C] = scale * rng.standard_normal((n, C))
                self.kv[r0:r0 + n, self.v_col:self.v_col + C] = rng.standard_normal((n, C))
        if kind == "self":  # fused rows: q columns of each sequence's rows, the K/V part shared with kv
            for b in range(B):
                r0, n = self.qrow0[b], self.qn[b]
                self.kv[r0:r0 + n, :C] = scale * rng.standard_normal((n, C))
            self.q = self.kv.copy()
        self.o = np.full((qrows if kind != "dense" else B * Lq, self.ldo), SENTINEL, np.float32)

    def run(self, eng, rope, k_rot):
        o, kv, form = eng.op_attention_ex(self.q, self.kv, self.o, self.B, self.Lq, self.Lk, self.H, self.dh, q_col=self.q_col,
                                          k_col=self.k_col, v_col=self.v_col, qlen=self.qlen, klen=self.klen, q_off=self.q_off,
                                          k_off=self.k_off, rope_mode=rope, k_rotated=k_rot, dtype=self.fmt, **self.rot)
        return o, kv, form

    def seq_out(self, o, b):
        r0, n = self.qrow0[b], self.qn[b]
        return o[r0:r0 + n, :self.C]

    def reference(self, b, rope, k_rot, mfma):
        H, dh, C, fmt = self.H, self.dh, self.C, self.fmt
        r0, n = self.qrow0[b], self.qn[b]
        q = rnd(self.q[r0:r0 + n, self.q_col:self.q_col + C], fmt).reshape(n, H, dh)
        nk, k0 = self.nk(b), self.krow0[b]
        k = rnd(self.kv[k0:k0 + max(nk, 0), self.k_col:self.k_col + C], fmt).reshape(-1, H, dh)
        v = rnd(self.kv[k0:k0 + max(nk, 0), self.v_col:self.v_col + C], fmt).reshape(-1, H, dh)
        nq = self.Lq if self.qlen is None else int(self.qlen[b])
        return attn_ref(q, k, v, nq, nk, rope, dh, fmt, mfma, k_rot and rope >= 0).reshape(n, C)

    def written_mask(self):
        m = np.zeros(self.o.shape, bool)
        for b in range(self.B):
            m[self.qrow0[b]:self.qrow0[b] + self.qn[b], :self.C] = True
        return m


def check_layout(eng, lay, rope, k_rot, expect_form):
    o, kv, form = lay.run(eng, rope, k_rot)
    assert form == expect_form, (form, expect_form)
    mfma = form.startswith("mfma")
    # nothing outside the written rows and columns changes
    w = lay.written_mask()
    assert np.all(bits(o)[~w] == SENTINEL_BITS), "a write outside the launch's rows / columns"
    differ = []
    for b in range(lay.B):
        differ.append(check_vals(lay.seq_out(o, b), lay.reference(b, rope, k_rot, mfma), lay.fmt,
                                 (lay.kind, lay.fmt, form, lay.Lq, lay.Lk, rope, k_rot, b)))
    check_frac([x for x in differ if x is not None], lay.fmt, (lay.kind, form, lay.Lq, lay.Lk, rope, k_rot))
    # rope_rows: the K columns of valid key rows (every group) and nothing else
    kin = np.asarray(rnd(lay.kv, lay.fmt), np.float32)
    if k_rot and rope >= 0:
        g, st, c0 = lay.rot["rot_groups"], lay.rot["rot_stride"], lay.rot["rot_col"]
        c0 = lay.k_col if c0 is None else c0
        touched = np.zeros(kv.shape, bool)
        for b in range(lay.B):
            r0, nk = lay.krow0[b], lay.nk(b)
            for gi in range(g):
                touched[r0:r0 + nk, c0 + gi * st:c0 + gi * st + lay.C] = True
                x = rnd(lay.kv[r0:r0 + nk, c0 + gi * st:c0 + gi * st + lay.C], lay.fmt).reshape(nk, lay.H, lay.dh)
                ref = rope64(x, nk, rope, lay.dh).reshape(nk, lay.C)
                d = np.abs(kv[r0:r0 + nk, c0 + gi * st:c0 + gi * st + lay.C] - ref)
                tol = (ulp(ref, lay.fmt) if lay.fmt != "f32" else 0) + F32_REL * (np.sqrt(np.mean(ref ** 2)) + 1e-30)
                assert np.all(d <= tol), ("rope_rows", b, gi)
        assert np.array_equal(bits(kv)[~touched], bits(kin)[~touched]), "rope_rows wrote outside the K columns of valid rows"
    else:
        assert np.array_equal(bits(kv), bits(kin)), "the K/V buffer changed"
    return o, form


def mform(dh, fmt, Lk):
    kc = min((Lk + 31) // 32 * 32, 128)
    return f"mfma<{dh},{fmt}> kc{kc} nch{(Lk + kc - 1) // kc}"


# ---- MFMA kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("dh", [32, 64, 96])
def test_mfma_key_lengths(eng, fmt, dh):
    """One chunk (Lk <= 128: kc = 32 .. 128) and two or three with a partial last chunk, every rope mode, keys rotated in the kernel and
    beforehand; Lq over several 128-row tiles and not a multiple of 32.  Per-sequence key lengths below Lk, and one above (clipped)."""
    rng = np.random.default_rng(dh)
    for i, Lk in enumerate([1, 31, 32, 33, 49, 63, 64, 65, 127, 128, 129, 257, 311]):
        rope = (-1, 0, 1)[i % 3]
        Lq = (40, 300, 97)[i % 3]
        lay = Layout("dense", 2, Lq, Lk, 2, dh, fmt, rng, qlen=[Lq, max(1, Lq - 5)], klen=[Lk + 3, max(1, Lk - Lk // 3)])
        check_layout(eng, lay, rope, False, mform(dh, fmt, Lk))
        if rope >= 0:
            lay = Layout("dense", 2, Lq, Lk, 2, dh, fmt, rng, qlen=[Lq, max(1, Lq - 5)], klen=[Lk, max(1, Lk // 2)])
            check_layout(eng, lay, rope, True, mform(dh, fmt, Lk))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("dh", [32, 64, 96])
def test_mfma_hazard_key_range(eng, fmt, dh):
    """Regression of the MFMA hazard on the key-loop exit (query rows 27 and 31 of a wave lost the last key tile at 49-64 keys): every
    context length of that range, 64 query rows (two waves), each key length once as the full context and once clipped by klen."""
    rng = np.random.default_rng(100 + dh)
    for Lk in range(49, 65):
        lay = Layout("dense", 2, 64, Lk, 1, dh, fmt, rng, klen=[Lk, Lk - 16])
        check_layout(eng, lay, (-1, 0, 1)[Lk % 3], False, mform(dh, fmt, Lk))


# ---- scalar kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("tpr", [32, 8])
def test_scalar_head_dims(eng, fmt, tpr):
    """attn_kernel<T, TPR> at head dims the MFMA kernel does not take (and, for fp32, at the MFMA ones too): TPR = 32 at B = 2, H = 2
    (few workgroups), TPR = 8 at B = 8, H = 4, Lq = 100 (128 workgroups of 32 rows); one and several 64-key tiles, every rope mode."""
    rng = np.random.default_rng(tpr)
    dhs = [8, 16, 40, 48, 80] + ([32, 64, 96] if fmt == "f32" else [])
    for i, dh in enumerate(dhs):
        rope = (-1, 0, 1)[i % 3]
        Lk = (50, 130, 311, 64, 1)[i % 5]
        B, H, Lq = (2, 2, 70) if tpr == 32 else (8, 4, 100)
        qlen = [Lq - (b % 3) for b in range(B)]
        klen = [Lk - (b * 7) % max(Lk, 1) for b in range(B)]
        lay = Layout("dense", B, Lq, Lk, H, dh, fmt, rng, qlen=qlen, klen=klen)
        suffix = " vec" if fmt == "f32" else ""
        check_layout(eng, lay, rope, False, f"scalar<{fmt},TPR{tpr}>{suffix}")
        if rope >= 0:
            check_layout(eng, lay, rope, True, f"scalar<{fmt},TPR{tpr}>{suffix}")


@pytest.mark.parametrize("tpr", [32, 8])
def test_scalar_staging_and_fallbacks(eng, tpr):
    """fp32 element-wise staging (ld % 4 != 0, or a pointer off 16-byte alignment) for q, for k / v and for both; the 16-bit scalar
    fallback of MFMA head dims (ld % 8 != 0, unaligned q)."""
    rng = np.random.default_rng(7 + tpr)
    B, H, Lq = (2, 2, 70) if tpr == 32 else (8, 4, 100)
    cases = [("f32", 64, dict(q_pad=1), "vec kv", None), ("f32", 64, dict(kv_pad=2), "vec q", None),
             ("f32", 96, dict(q_pad=3, kv_pad=1), "elem", None), ("f32", 32, dict(q_col=1), "vec kv", None),
             ("bf16", 64, dict(q_pad=4), None, None), ("f16", 96, dict(kv_pad=4), None, None), ("bf16", 32, dict(q_col=4), None, None),
             ("f16", 64, dict(q_col=2), None, None)]
    for i, (fmt, dh, kw, vec, _) in enumerate(cases):
        rope = (-1, 0, 1)[i % 3]
        lay = Layout("dense", B, Lq, 77, H, dh, fmt, rng, qlen=[Lq] * B, klen=[77 - b for b in range(B)], o_pad=3, **kw)
        want = f"scalar<{fmt},TPR{tpr}>" + (f" {vec}" if vec else "")
        check_layout(eng, lay, rope, False, want)
        if rope >= 0:
            check_layout(eng, lay, rope, True, want)


# ---- the engine's layouts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
def test_engine_layouts(eng, fmt):
    """self: fused QKV rows (ld 3C), packed q and k (gaps between sequences); text: K/V of block 2 of an nb*2C row, packed keys rotated
    once by rope_rows over all four blocks (as ve_text_kv_dev), length-aware rope; style: dense keys of block 3, 50 tokens, no rope.
    Padding columns of o and rows between packed sequences must keep their sentinels."""
    rng = np.random.default_rng(3)
    for dh, H in [(64, 4), (96, 4), (32, 2)]:
        mf = fmt != "f32"

        def fm(Lk, B, Lq):
            if mf:
                return mform(dh, fmt, Lk)
            tpr = 32 if ((Lq + 31) // 32) * H * B < 96 else 8
            return f"scalar<f32,TPR{tpr}> vec"

        ql = [70, 33, 1, 128]
        lay = Layout("self", 4, 128, 128, H, dh, fmt, rng, qlen=ql, klen=ql, o_pad=8)
        check_layout(eng, lay, 0, False, fm(128, 4, 128))
        lay = Layout("text", 4, 128, 140, H, dh, fmt, rng, qlen=ql, klen=[140, 33, 64, 1], o_pad=8, blk=2)
        check_layout(eng, lay, 1, True, fm(140, 4, 128))
        lay = Layout("style", 4, 128, 50, H, dh, fmt, rng, qlen=ql, o_pad=8, blk=3)
        check_layout(eng, lay, -1, False, fm(50, 4, 128))


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
def test_empty_and_clipped_lengths(eng, fmt):
    """klen = 0: zeros; klen > Lk: clipped to Lk; qlen = 0 with packed rows: nothing is written; all in one launch."""
    rng = np.random.default_rng(11)
    dh = 64
    lay = Layout("text", 4, 40, 50, 2, dh, fmt, rng, qlen=[40, 0, 17, 9], klen=[0, 50, 60, 50], blk=1)
    o, form = check_layout(eng, lay, 1, True, mform(dh, fmt, 50) if fmt != "f32" else "scalar<f32,TPR32> vec")
    assert np.all(lay.seq_out(o, 0) == 0)
    lay = Layout("dense", 3, 40, 50, 2, dh, fmt, rng, qlen=[40, 40, 40], klen=[0, 50, 99])
    o, _ = check_layout(eng, lay, 0, False, form)
    assert np.all(lay.seq_out(o, 0) == 0)


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
def test_large_scores(eng, fmt):
    """Scores of magnitude ~80 (q, k scaled by 5.5 at dh = 64): the running / two-pass maximum keeps the exponentials finite."""
    rng = np.random.default_rng(13)
    for Lk in (50, 200):
        lay = Layout("dense", 2, 70, Lk, 2, 64, fmt, rng, klen=[Lk, Lk // 2 + 1], scale=5.5)
        o, form = check_layout(eng, lay, -1, False, mform(64, fmt, Lk) if fmt != "f32" else "scalar<f32,TPR32> vec")


@pytest.mark.parametrize("fmt,dh,B,H,Lq,Lk", [("f32", 48, 2, 2, 70, 130), ("f32", 64, 8, 4, 100, 50), ("bf16", 40, 2, 2, 70, 80),
                                              ("f16", 80, 8, 4, 100, 80), ("bf16", 64, 4, 2, 150, 140), ("f16", 96, 4, 2, 150, 50)])
def test_batch_independence_and_repeat(eng, fmt, dh, B, H, Lq, Lk):
    """A sequence's output bits do not depend on its batch position or on the other sequences (batch reversed, the others' data
    replaced), at a fixed form; two launches give identical bits."""
    rng = np.random.default_rng(dh + B)
    ql = [Lq - 3 * b for b in range(B)]
    kl = [Lk - 5 * b for b in range(B)]
    lay = Layout("text", B, Lq, Lk, H, dh, fmt, rng, qlen=ql, klen=kl, blk=1)
    o1, k1, f1 = lay.run(eng, 1, True)
    o2, k2, _ = lay.run(eng, 1, True)
    assert np.array_equal(bits(o1), bits(o2)) and np.array_equal(bits(k1), bits(k2))
    # sequence 0 alone at the last batch position, the others' data redrawn
    lay2 = Layout("text", B, Lq, Lk, H, dh, fmt, np.random.default_rng(99), qlen=ql[::-1], klen=kl[::-1], blk=1)
    C = H * dh
    r0, n = lay.qrow0[0], lay.qn[0]
    s0, m = lay2.qrow0[B - 1], lay2.qn[B - 1]
    lay2.q[s0:s0 + m] = lay.q[r0:r0 + n]
    k0, nk = lay.krow0[0], lay.nk(0)
    t0 = lay2.krow0[B - 1]
    lay2.kv[t0:t0 + nk] = lay.kv[k0:k0 + nk]
    o3, _, f3 = lay2.run(eng, 1, True)
    assert f3 == f1
    assert np.array_equal(bits(o3[s0:s0 + m, :C]), bits(o1[r0:r0 + n, :C]))


# ---- head-split block ------------------------------------------------------------------------------------------------------------------
def pairs_ref(lens):
    B = len(lens)
    order = sorted(range(B), key=lambda i: (lens[i], i))
    G = (B + 1) // 2
    out = []
    for g in range(G):
        out += [order[B - 1 - g], order[g] if B - 1 - g > g else -1]
    return np.asarray(out, np.int32)


class HsCase:
    def __init__(self, fmt, qlen, Lk, rng, text, klen=None, bias=True, extra_rows=5, nb=4, blk=None):
        C = HS_C
        self.fmt, self.qlen, self.Lk, self.text = fmt, np.asarray(qlen, np.int32), Lk, text
        self.B = len(qlen)
        self.L = int(max(max(qlen), 1))
        self.M = int(self.qlen.sum()) + extra_rows
        self.xn = rng.standard_normal((self.M, C)).astype(np.float32)
        self.Wq = (rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
        self.Wo = (rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
        self.bq = (0.5 * rng.standard_normal(C)).astype(np.float32) if bias else None
        self.blk = (2 if text else 3) if blk is None else blk
        self.ldk = nb * 2 * C
        self.k_col = self.blk * 2 * C
        self.rope = 1 if text else -1
        B = self.B
        if text:
            self.klen = np.asarray(klen, np.int32)
            offs, r = [], 1
            for b in range(B):
                offs.append(r)
                r += min(int(self.klen[b]), Lk) + 2
            self.k_off, self.krow0, krows = np.asarray(offs, np.int32), offs, r
        else:
            self.klen = None if klen is None else np.asarray(klen, np.int32)
            self.k_off, self.krow0, krows = None, [b * Lk for b in range(B)], B * Lk
        self.kv = np.full((krows, self.ldk), SENTINEL, np.float32)
        for b in range(B):
            n = self.nk(b)
            self.kv[self.krow0[b]:self.krow0[b] + n, self.k_col:self.k_col + 2 * C] = rng.standard_normal((n, 2 * C))
        self.row0 = np.concatenate([[0], np.cumsum(self.qlen)])[:-1]
        self.part_stride = (self.M + 3) * C
        self.part = np.full(3 * self.part_stride + self.M * C + 2 * C, SENTINEL, np.float32)

    def nk(self, b):
        return self.Lk if self.klen is None else min(int(self.klen[b]), self.Lk)

    def run(self, eng, pairs):
        return eng.op_xattn_hs(self.xn, self.Wq, self.bq, self.Wo, self.kv, self.part, self.part_stride, self.B, self.L, self.Lk, self.qlen,
                               k_col=self.k_col, klen=self.klen, k_off=self.k_off, rope_mode=self.rope, pairs=pairs, dtype=self.fmt)

    def head_view(self, part, h):
        return part[h * self.part_stride:h * self.part_stride + self.M * HS_C].reshape(self.M, HS_C)

    def reference(self, b):
        """part[h] rows of utterance b, float64, rounded where xattn_hs_kernel rounds"""
        fmt, C, DH = self.fmt, HS_C, HS_DH
        r0, n, nk, k0 = int(self.row0[b]), int(self.qlen[b]), self.nk(b), self.krow0[b]
        x = rnd(self.xn[r0:r0 + n], fmt)
        q = x @ rnd(self.Wq, fmt).T + (0.0 if self.bq is None else self.bq.astype(np.float64))
        q = rnd(q, fmt).reshape(n, HS_H, DH)
        q = rnd(rope64(q, n, self.rope, DH) * (LOG2E / np.sqrt(DH)), fmt)
        K = rnd(self.kv[k0:k0 + nk, self.k_col:self.k_col + C], fmt).reshape(nk, HS_H, DH)
        V = rnd(self.kv[k0:k0 + nk, self.k_col + C:self.k_col + 2 * C], fmt).reshape(nk, HS_H, DH)
        out = []
        Wo = rnd(self.Wo, fmt)
        for h in range(HS_H):
            if nk == 0:
                O = np.zeros((n, DH))
            else:
                s = q[:, h] @ K[:, h].T
                p = np.exp2(s - s.max(axis=1, keepdims=True))
                O = rnd((rnd(p, fmt) @ V[:, h]) * (1.0 / p.sum(axis=1))[:, None], fmt)
            out.append(rnd(O @ Wo[:, h * DH:(h + 1) * DH].T, fmt))
        return out


def check_hs(eng, case, pairs, expect_form):
    part, pr, form = case.run(eng, pairs)
    assert form == expect_form, (form, expect_form)
    if pairs:
        assert np.array_equal(pr, pairs_ref(list(case.qlen))), pr
    written = np.zeros(part.shape, bool)
    for h in range(HS_H):
        base = h * case.part_stride
        for b in range(case.B):
            r0, n = int(case.row0[b]), int(case.qlen[b])
            written[base + r0 * HS_C:base + (r0 + n) * HS_C] = True
    assert np.all(bits(part)[~written] == SENTINEL_BITS), "a write outside the launch's rows (stride gap, tail, rows past sum qlen)"
    differ = []
    for b in range(case.B):
        ref = case.reference(b)
        r0, n = int(case.row0[b]), int(case.qlen[b])
        for h in range(HS_H):
            differ.append(check_vals(case.head_view(part, h)[r0:r0 + n], ref[h], case.fmt, ("hs", case.fmt, form, b, h), kind="hs"))
    check_frac([x for x in differ if x is not None], case.fmt, ("hs", form, case.B, case.Lk))
    return part, form


def lens_of(rng, B, lo, hi):
    return [int(x) for x in rng.integers(lo, hi + 1, B)]


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_head_split_one_per_workgroup(eng, fmt):
    """U = 1 (B <= 64, or an utterance longer than 128 rows): odd batches, utterances of 1 .. 256 rows (above 128: a wave owns two
    tiles), every key length of the text and the style form, with and without the q bias, pairs table or none (unused at U = 1)."""
    rng = np.random.default_rng(21)
    cases = [([1, 32, 33], 1, True, True), ([128, 129, 256, 40, 7], 31, True, False), ([256, 1, 200], 32, False, True),
             ([33, 64, 100, 129, 5], 33, True, True), ([60, 61, 62], 50, False, False), ([129, 30, 31, 2, 90], 64, True, True),
             ([256, 255, 3], 127, False, True), ([32, 128, 70, 1, 9], 128, True, False)]
    for i, (ql, Lk, text, bias) in enumerate(cases):
        kl = [Lk - (b * 11) % Lk for b in range(len(ql))] if text else None
        case = HsCase(fmt, ql, Lk, rng, text, klen=kl, bias=bias)
        kc = (Lk + 31) // 32 * 32
        check_hs(eng, case, i % 2 == 0, f"xattn_hs<{fmt},U1> kc{kc}")


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_head_split_pairs(eng, fmt):
    """U = 2 (B >= 65, L <= 128, Lk <= 96): odd batches (the -1 slot), pairs null (2g, 2g + 1) and the computed longest-with-shortest
    table, text and style forms; lengths from 1 to 128 so that some pairs span more than four tiles (a wave owns two)."""
    rng = np.random.default_rng(22)
    for i, (B, lo, hi, Lk, text) in enumerate([(65, 1, 128, 50, True), (67, 60, 128, 33, False), (69, 1, 40, 96, True),
                                                 (65, 100, 128, 1, False)]):
        ql = lens_of(rng, B, lo, hi)
        kl = [max(0, Lk - (b * 5) % (Lk + 1)) for b in range(B)] if text else None
        case = HsCase(fmt, ql, Lk, rng, text, klen=kl, bias=i % 2 == 0)
        kc = (Lk + 31) // 32 * 32
        for pairs in (False, True):
            check_hs(eng, case, pairs, f"xattn_hs<{fmt},U2> kc{kc}")


def test_hs_pairs_table(eng):
    """hs_pairs_kernel against its restatement: sorted ascending by length (ties by index), the k-th longest with the k-th shortest."""
    rng = np.random.default_rng(23)
    for ql in ([5], [3, 9], [7, 7, 7, 7, 7], [4, 1, 4, 2, 9, 2, 4], lens_of(rng, 1024, 1, 8), lens_of(rng, 66, 1, 3)):
        case = HsCase("bf16", ql, 32, rng, False, bias=False, extra_rows=0)
        part, pr, form = case.run(eng, True)
        assert np.array_equal(pr, pairs_ref(ql)), (len(ql), pr[:16])


@pytest.mark.parametrize("fmt,B", [("bf16", 5), ("f16", 67)])
def test_head_split_batch_independence(eng, fmt, B):
    """At a fixed U and pairing, an utterance's partial sums do not depend on its batch position or on the other utterances' data (the
    batch reversed with distinct lengths, so that the same utterances pair up); two launches give identical bits."""
    rng = np.random.default_rng(24)
    ql = list(rng.permutation(np.arange(20, 20 + B)))[:B] if B <= 64 else [int(x) for x in rng.permutation(np.arange(1, 129))[:B]]
    c1 = HsCase(fmt, ql, 50, rng, True, klen=[50 - b % 7 for b in range(B)])
    p1, _, f1 = c1.run(eng, True)
    p1b, _, _ = c1.run(eng, True)
    assert np.array_equal(bits(p1), bits(p1b))
    c2 = HsCase(fmt, ql[::-1], 50, np.random.default_rng(25), True, klen=[50 - b % 7 for b in range(B)][::-1])
    c2.Wq, c2.Wo, c2.bq = c1.Wq, c1.Wo, c1.bq
    for b in range(B):  # utterance b of c1 is utterance B-1-b of c2: copy its rows and keys
        r1, n = int(c1.row0[b]), int(c1.qlen[b])
        r2 = int(c2.row0[B - 1 - b])
        c2.xn[r2:r2 + n] = c1.xn[r1:r1 + n]
        k1, k2, nk = c1.krow0[b], c2.krow0[B - 1 - b], c1.nk(b)
        c2.kv[k2:k2 + nk] = c1.kv[k1:k1 + nk]
    p2, _, f2 = c2.run(eng, True)
    assert f2 == f1
    for b in (0, B // 2, B - 1):
        r1, n = int(c1.row0[b]), int(c1.qlen[b])
        r2 = int(c2.row0[B - 1 - b])
        for h in range(HS_H):
            assert np.array_equal(bits(c1.head_view(p1, h)[r1:r1 + n]), bits(c2.head_view(p2, h)[r2:r2 + n])), (b, h)


def test_entry_points_refuse_bad_calls(eng):
    """Bad calls come back as error codes, not aborts."""
    rng = np.random.default_rng(0)
    lay = Layout("dense", 2, 10, 10, 2, 32, "bf16", rng)
    with pytest.raises(binding.StnError):
        eng.op_attention_ex(lay.q, lay.kv, lay.o, 2, 10, 10, 2, 32, k_col=lay.ldk - 32)  # K past the row end
    with pytest.raises(binding.StnError):
        eng.op_attention_ex(lay.q, lay.kv[:5], lay.o, 2, 10, 10, 2, 32)  # fewer than B*Lk key rows
    with pytest.raises(binding.StnError):
        eng.op_attention_ex(lay.q, lay.kv, lay.o, 2, 10, 10, 2, 32, q_off=[0, 5])  # packed without qlen
    with pytest.raises(binding.StnError):
        eng.op_attention_ex(lay.q, lay.kv, lay.o, 2, 10, 10, 2, 36)  # head dim
    case = HsCase("bf16", [3, 4], 10, rng, False)
    with pytest.raises(binding.StnError):
        eng.op_xattn_hs(case.xn, case.Wq, None, case.Wo, case.kv, case.part, case.part_stride, 2, 4, 129, case.qlen)  # Lk > 128
    with pytest.raises(binding.StnError):
        eng.op_xattn_hs(case.xn[:5], case.Wq, None, case.Wo, case.kv, case.part, case.part_stride, 2, 4, 10, case.qlen)  # sum qlen > M
    with pytest.raises(binding.StnError):
        eng.op_xattn_hs(case.xn, case.Wq, None, case.Wo, case.kv, case.part, case.part_stride, 2, 4, 10, case.qlen, dtype="f32")


def test_zz_report_measured():
    """(prints the largest errors seen by the cases above: the measured values of the module docstring)"""
    for k, v in sorted(STATS.items()):
        print("measured", k, {a: round(b, 6) for a, b in v.items()})
