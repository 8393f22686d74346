// body of kernels_ffn.hip, one kernel variant per inclusion.  The includer defines only the switches that differ from the product, which is all of
// them 0; every switch it was given is undefined again at the end, except STN_V_ACCA, which the command line may set for the whole unit:
//   STN_V_F16         1: IEEE-half operands (the f16k instantiation of the product); 0: bf16
//   STN_V_NODMA, STN_V_NOGELU, STN_V_EARLYRD (1, 2), STN_V_STAGESTAMP      timing-only variants (kernels_ffn.hip: STN_FFN_VARIANTS)
//   STN_V_NOBAR       timing-only variants: 1 drops the ring hand-over's barrier, 2 its counted vmcnt wait too
#ifndef STN_V_F16
#define STN_V_F16 0
#endif
#ifndef STN_V_NODMA
#define STN_V_NODMA 0
#endif
#ifndef STN_V_NOGELU
#define STN_V_NOGELU 0
#endif
#ifndef STN_V_EARLYRD
#define STN_V_EARLYRD 0
#endif
#ifndef STN_V_NOBAR
#define STN_V_NOBAR 0
#endif
#ifndef STN_V_STAGESTAMP
#define STN_V_STAGESTAMP 0
#endif
#ifndef STN_V_ACCA
#define STN_V_ACCA 0
#endif

#if STN_V_NOBAR == 0
#define STN_HANDOVER(PER) do { wait_vm<PER>(); __builtin_amdgcn_s_barrier(); } while (0)
#elif STN_V_NOBAR == 1
#define STN_HANDOVER(PER) do { wait_vm<PER>(); } while (0)
#else
#define STN_HANDOVER(PER) do { } while (0)
#endif
// ---- asm blocks --------------------------------------------------------------------------------------------------------
// Every block: 4 MFMAs on the fragments `f` that the PREVIOUS block read, the 4 fragment reads of the NEXT block (%[n0..n3]
// at %[ad] + %[o0] + 0/1024/2048/3072: this lane's 16 bytes of KiB pieces), ONE LDS-DMA piece of the stage that is being
// filled two stages ahead (the wave's instruction stream is the only thing that hides its issue cost at one wave per SIMD, so
// the 16 pieces a wave moves per hidden tile sit one behind the first MFMA of each block instead of in a burst at the ring
// hand-over), optionally the GELU of two accumulator elements of a finished phase-1 tile, and the s_waitcnt that makes the
// outputs valid.
#if STN_V_EARLYRD == 2
#define STN_RD01 ""
#define STN_RD2 ""
#define STN_RD3 ""
#elif STN_V_EARLYRD
#define STN_RD01                                             \
    "ds_read_b128 %[n0], %[ad] offset:%[o0]\n\t"             \
    "ds_read_b128 %[n1], %[ad] offset:%[o0]+1024\n\t"        \
    "ds_read_b128 %[n2], %[ad] offset:%[o0]+2048\n\t"        \
    "ds_read_b128 %[n3], %[ad] offset:%[o0]+3072\n\t"
#define STN_RD2 ""
#define STN_RD3 ""
#else
#define STN_RD01                                             \
    "ds_read_b128 %[n0], %[ad] offset:%[o0]\n\t"             \
    "ds_read_b128 %[n1], %[ad] offset:%[o0]+1024\n\t"
#define STN_RD2 "ds_read_b128 %[n2], %[ad] offset:%[o0]+2048\n\t"
#define STN_RD3 "ds_read_b128 %[n3], %[ad] offset:%[o0]+3072\n\t"
#endif
// LDS-DMA of one KiB: M0 = LDS byte address of the piece, written IN FRONT of the block's first MFMA (which is then the wait state the
// hardware wants between an s_mov to M0 and an LDS-DMA) and declared as a clobber — nothing the compiler places in these loops uses M0,
// so the former save / s_nop / restore around every piece (three scalar instructions and a nop per block, on the issue path of the one
// wave a SIMD has) is gone; per-lane source offset %[dv] (beyond the buffer for a stage past the last one: the hardware range check then
// writes zeros, and every wave's vmcnt arithmetic stays the same to the end), descriptor %[rs], scalar offset %[so] = tile * stage bytes
#if STN_V_NODMA
#define STN_M0 ""
#define STN_DMA ""
#else
#define STN_M0 "s_mov_b32 m0, %[dm]\n\t"
#define STN_DMA "buffer_load_dwordx4 %[dv], %[rs], %[so] offen offset:%[di] lds\n\t"
#endif
// An MFMA result inside an asm statement is invisible to hipcc: whatever it places behind the statement (a live-range copy of
// the accumulator, an epilogue read) may read the destination before the 8-pass MFMA has written it (needs 11 wait states;
// found the hard way: a v_mov copy two instructions behind the last MFMA of a block lost that MFMA's contribution).  Every
// block therefore keeps >= 11 wait states between its last MFMA into an arch-VGPR accumulator and its end — the GELU tail where
// there is one, this pad where there is none; of the AGPR accumulators of phase 2 only the last block of a stage is padded
// (its other blocks' tiles are four MFMAs older by then).  tools/check_hazards.py walks the shipped code object for exactly
// this (tests/test_isa_cpu.py).
#define STN_MFMA_PAD "s_nop 7\n\ts_nop 2\n\t"
// STN_V_F16 = 1: IEEE-half operands (v_mfma_f32_32x32x16_f16, v_cvt_pk_f16_f32); everything else is the same instruction stream
#if STN_V_F16
#define STN_MFMA_OP "v_mfma_f32_32x32x16_f16"
#define STN_CVT_PK "v_cvt_pk_f16_f32"
#else
#define STN_MFMA_OP "v_mfma_f32_32x32x16_bf16"
#define STN_CVT_PK "v_cvt_pk_bf16_f32"
#endif
#define STN_MF1(f, x) STN_MFMA_OP " %[acc], %[" #f "], %[" #x "], %[acc]\n\t"
#define STN_MF2(y, f, gg) STN_MFMA_OP " %[" #y "], %[" #f "], %[" #gg "], %[" #y "]\n\t"
// GELU of the pw1 epilogue (gelu_bf16_f: x / (1 + exp2(x * fma(x*x, -0.10294324, -2.30220819)))) on two accumulator
// elements, in three groups that go behind successive MFMAs; every dependent pair has an instruction between it and its
// producer (the transcendental-result wait state of gfx950: one state between a v_exp / v_rcp and a plain VALU reading it — the
// other element's instruction is that state, no s_nop: an s_nop next to MFMAs costs 5-20 cycles, profiles/r03_mfma_chain.txt)
#if STN_V_NOGELU
#define STN_GELU_A "v_mov_b32 %[ta], %[ha]\n\tv_mov_b32 %[tb], %[hb]\n\t"
#define STN_GELU_B ""
#define STN_GELU_C STN_CVT_PK " %[gw], %[ta], %[tb]\n\ts_nop 7\n\t"
#else
#define STN_GELU_A                                        \
    "v_mul_f32 %[ta], %[ha], %[ha]\n\t"                   \
    "v_mul_f32 %[tb], %[hb], %[hb]\n\t"                   \
    "v_fmamk_f32 %[ta], %[ta], 0xbdd2d3e8, %[cb]\n\t"     \
    "v_fmamk_f32 %[tb], %[tb], 0xbdd2d3e8, %[cb]\n\t"
#define STN_GELU_B                                        \
    "v_mul_f32 %[ta], %[ha], %[ta]\n\t"                   \
    "v_mul_f32 %[tb], %[hb], %[tb]\n\t"                   \
    "v_exp_f32 %[ta], %[ta]\n\t"                          \
    "v_exp_f32 %[tb], %[tb]\n\t"
#define STN_GELU_C                                        \
    "v_add_f32 %[ta], 1.0, %[ta]\n\t"                     \
    "v_add_f32 %[tb], 1.0, %[tb]\n\t"                     \
    "v_rcp_f32 %[ta], %[ta]\n\t"                          \
    "v_rcp_f32 %[tb], %[tb]\n\t"                          \
    "v_mul_f32 %[ta], %[ha], %[ta]\n\t"                   \
    "v_mul_f32 %[tb], %[hb], %[tb]\n\t"                   \
    STN_CVT_PK " %[gw], %[ta], %[tb]\n\t"
#endif
// the same GELU on ONE element, in two groups (C = 512: every block of a stage carries one element; an even block hands its
// result `y` to the odd block behind it, which packs the pair)
#if STN_V_NOGELU
#define STN_GEL1_A "v_mov_b32 %[ta], %[ha]\n\t"
#define STN_GEL1_B ""
#else
#define STN_GEL1_A                                        \
    "v_mul_f32 %[ta], %[ha], %[ha]\n\t"                   \
    "v_fmamk_f32 %[ta], %[ta], 0xbdd2d3e8, %[cb]\n\t"     \
    "v_mul_f32 %[ta], %[ha], %[ta]\n\t"                   \
    "v_exp_f32 %[ta], %[ta]\n\t"
#define STN_GEL1_B                                        \
    "v_add_f32 %[ta], 1.0, %[ta]\n\t"                     \
    "v_rcp_f32 %[ta], %[ta]\n\t"                          \
    "s_nop 0\n\t"                                         \
    "v_mul_f32 %[ta], %[ha], %[ta]\n\t"
#endif
#define STN_GEL1_PK STN_CVT_PK " %[gw], %[yp], %[ta]\n\t"

#if STN_V_ACCA
#define STN_ACCC "+a"
#else
#define STN_ACCC "+v"
#endif
struct DmaPiece {              // one LDS-DMA wave-instruction (all wave-uniform except dv)
    unsigned dm;               // LDS byte address of the KiB, less the instruction's immediate offset
    unsigned dv;               // this lane's source byte offset
    int so;                    // scalar source offset, less the immediate offset
};
// The instruction's 12-bit immediate offset is added to the memory address AND to the LDS address: pieces j = 4g .. 4g+3 of a stage share
// M0 = (piece 4g's address) and one scalar offset, and differ in the immediate (j & 3) KiB — no scalar add per piece.
__device__ __forceinline__ constexpr int ffn_piece_imm(int j) { return (j & 3) * 1024; }
#define STN_NOUT [n0] "=&v"(n[0]), [n1] "=&v"(n[1]), [n2] "=&v"(n[2]), [n3] "=&v"(n[3])
#define STN_FIN [f0] "v"(f[0]), [f1] "v"(f[1]), [f2] "v"(f[2]), [f3] "v"(f[3]), [ad] "v"(ad), [dm] "s"(d.dm), [dv] "v"(d.dv), [rs] "s"(rsw), [so] "s"(d.so), [o0] "i"(O0), [di] "i"(DI)

// phase-1 block: 4 MFMAs into the chained accumulator `acc` (arch VGPRs)
template <int O0, int DI>
__device__ __forceinline__ void p1_block(f32x16& acc, const bf16x8 (&f)[4], bf16x8 (&n)[4], bf16x8 x0, bf16x8 x1, bf16x8 x2, bf16x8 x3,
                                         unsigned ad, const DmaPiece& d, const __amdgpu_buffer_rsrc_t rsw) {
    asm volatile(STN_RD01 STN_M0 STN_MF1(f0, x0) STN_DMA STN_RD2 STN_MF1(f1, x1) STN_RD3 STN_MF1(f2, x2) STN_MF1(f3, x3)
                 "s_waitcnt lgkmcnt(0)"
                 : STN_NOUT, [acc] STN_ACCC(acc)
                 : STN_FIN, [x0] "v"(x0), [x1] "v"(x1), [x2] "v"(x2), [x3] "v"(x3)
                 : "memory", "m0");
}
// ... with the GELU of two elements (ha, hb) of the previous tile -> one packed word
template <int O0, int DI>
__device__ __forceinline__ void p1_block_g(f32x16& acc, const bf16x8 (&f)[4], bf16x8 (&n)[4], bf16x8 x0, bf16x8 x1, bf16x8 x2, bf16x8 x3,
                                           unsigned ad, const DmaPiece& d, const __amdgpu_buffer_rsrc_t rsw, float ha, float hb, float cb, unsigned& gw) {
    float ta, tb;
    asm volatile(STN_RD01 STN_M0 STN_MF1(f0, x0) STN_DMA STN_RD2 STN_MF1(f1, x1) STN_GELU_A STN_RD3 STN_MF1(f2, x2) STN_GELU_B STN_MF1(f3, x3) STN_GELU_C
                 "s_waitcnt lgkmcnt(0)"
                 : STN_NOUT, [acc] STN_ACCC(acc), [ta] "=&v"(ta), [tb] "=&v"(tb), [gw] "=&v"(gw)
                 : STN_FIN, [x0] "v"(x0), [x1] "v"(x1), [x2] "v"(x2), [x3] "v"(x3), [ha] "v"(ha), [hb] "v"(hb), [cb] "v"(cb)
                 : "memory", "m0");
}
// phase-2 block: pieces (nt, s) = (2b, 0), (2b, 1), (2b+1, 0), (2b+1, 1) -> two accumulator tiles in the AGPR file
template <int O0, int DI>
__device__ __forceinline__ void p2_block(f32x16& ya, f32x16& yb, const bf16x8 (&f)[4], bf16x8 (&n)[4], bf16x8 g0, bf16x8 g1, unsigned ad,
                                         const DmaPiece& d, const __amdgpu_buffer_rsrc_t rsw) {
    asm volatile(STN_RD01 STN_M0 STN_MF2(ya, f0, g0) STN_DMA STN_RD2 STN_MF2(yb, f2, g0) STN_RD3 STN_MF2(ya, f1, g1) STN_MF2(yb, f3, g1)
                 "s_waitcnt lgkmcnt(0)"
                 : STN_NOUT, [ya] "+a"(ya), [yb] "+a"(yb)
                 : STN_FIN, [g0] "v"(g0), [g1] "v"(g1)
                 : "memory", "m0");
}
// ... with the GELU of two elements of the phase-1 tile that has just been finished
template <int O0, int DI>
__device__ __forceinline__ void p2_block_g(f32x16& ya, f32x16& yb, const bf16x8 (&f)[4], bf16x8 (&n)[4], bf16x8 g0, bf16x8 g1, unsigned ad,
                                           const DmaPiece& d, const __amdgpu_buffer_rsrc_t rsw, float ha, float hb, float cb, unsigned& gw) {
    float ta, tb;
    asm volatile(STN_RD01 STN_M0 STN_MF2(ya, f0, g0) STN_DMA STN_RD2 STN_MF2(yb, f2, g0) STN_GELU_A STN_RD3 STN_MF2(ya, f1, g1) STN_GELU_B
                 STN_MF2(yb, f3, g1) STN_GELU_C
                 "s_waitcnt lgkmcnt(0)"
                 : STN_NOUT, [ya] "+a"(ya), [yb] "+a"(yb), [ta] "=&v"(ta), [tb] "=&v"(tb), [gw] "=&v"(gw)
                 : STN_FIN, [g0] "v"(g0), [g1] "v"(g1), [ha] "v"(ha), [hb] "v"(hb), [cb] "v"(cb)
                 : "memory", "m0");
}
// ... the last block of a phase-2 stage also fetches b1 of the hidden tile whose phase 1 comes next (4 x 16 bytes at `bad`)
template <int O0, int DI>
__device__ __forceinline__ void p2_block_bias(f32x16& ya, f32x16& yb, const bf16x8 (&f)[4], bf16x8 (&n)[4], bf16x8 g0, bf16x8 g1, unsigned ad,
                                              const DmaPiece& d, const __amdgpu_buffer_rsrc_t rsw, unsigned bad, f32x4 (&bq)[4]) {
    asm volatile(STN_RD01 STN_M0 STN_MF2(ya, f0, g0) STN_DMA STN_RD2
                 "ds_read_b128 %[b0], %[bad]\n\t"
                 "ds_read_b128 %[b1], %[bad] offset:32\n\t" STN_MF2(yb, f2, g0) STN_RD3
                 "ds_read_b128 %[b2], %[bad] offset:64\n\t"
                 "ds_read_b128 %[b3], %[bad] offset:96\n\t" STN_MF2(ya, f1, g1) STN_MF2(yb, f3, g1)
                 "s_waitcnt lgkmcnt(0)\n\t" STN_MFMA_PAD  /* the stage's last MFMAs: whatever hipcc puts behind the stage may read them */
                 : STN_NOUT, [ya] "+a"(ya), [yb] "+a"(yb), [b0] "=&v"(bq[0]), [b1] "=&v"(bq[1]), [b2] "=&v"(bq[2]), [b3] "=&v"(bq[3])
                 : STN_FIN, [g0] "v"(g0), [g1] "v"(g1), [bad] "v"(bad)
                 : "memory", "m0");
}
// ---- one GELU element per block (C = 512) --------------------------------------------------------------------------------
// phase 1, even block: GELU(ha) -> y;  odd block: GELU(ha) and the pair (yp, that) -> packed word
template <int O0, int DI>
__device__ __forceinline__ void p1_block_e(f32x16& acc, const bf16x8 (&f)[4], bf16x8 (&n)[4], bf16x8 x0, bf16x8 x1, bf16x8 x2, bf16x8 x3,
                                           unsigned ad, const DmaPiece& d, const __amdgpu_buffer_rsrc_t rsw, float ha, float cb, float& y) {
    asm volatile(STN_RD01 STN_M0 STN_MF1(f0, x0) STN_DMA STN_RD2 STN_MF1(f1, x1) STN_GEL1_A STN_RD3 STN_MF1(f2, x2) STN_GEL1_B STN_MF1(f3, x3)
                 "s_waitcnt lgkmcnt(0)"
                 : STN_NOUT, [acc] STN_ACCC(acc), [ta] "=&v"(y)
                 : STN_FIN, [x0] "v"(x0), [x1] "v"(x1), [x2] "v"(x2), [x3] "v"(x3), [ha] "v"(ha), [cb] "v"(cb)
                 : "memory", "m0");
}
template <int O0, int DI, bool PAD>
__device__ __forceinline__ void p1_block_o(f32x16& acc, const bf16x8 (&f)[4], bf16x8 (&n)[4], bf16x8 x0, bf16x8 x1, bf16x8 x2, bf16x8 x3,
                                           unsigned ad, const DmaPiece& d, const __amdgpu_buffer_rsrc_t rsw, float ha, float cb, float yp, unsigned& gw) {
    float ta;
    if constexpr (PAD)
        asm volatile(STN_RD01 STN_M0 STN_MF1(f0, x0) STN_DMA STN_RD2 STN_MF1(f1, x1) STN_GEL1_A STN_RD3 STN_MF1(f2, x2) STN_GEL1_B STN_GEL1_PK STN_MF1(f3, x3)
                     "s_waitcnt lgkmcnt(0)\n\t" STN_MFMA_PAD
                     : STN_NOUT, [acc] STN_ACCC(acc), [ta] "=&v"(ta), [gw] "=&v"(gw)
                     : STN_FIN, [x0] "v"(x0), [x1] "v"(x1), [x2] "v"(x2), [x3] "v"(x3), [ha] "v"(ha), [cb] "v"(cb), [yp] "v"(yp)
                     : "memory", "m0");
    else
        asm volatile(STN_RD01 STN_M0 STN_MF1(f0, x0) STN_DMA STN_RD2 STN_MF1(f1, x1) STN_GEL1_A STN_RD3 STN_MF1(f2, x2) STN_GEL1_B STN_GEL1_PK STN_MF1(f3, x3)
                     "s_waitcnt lgkmcnt(0)"
                     : STN_NOUT, [acc] STN_ACCC(acc), [ta] "=&v"(ta), [gw] "=&v"(gw)
                     : STN_FIN, [x0] "v"(x0), [x1] "v"(x1), [x2] "v"(x2), [x3] "v"(x3), [ha] "v"(ha), [cb] "v"(cb), [yp] "v"(yp)
                     : "memory", "m0");
}
template <int O0, int DI>
__device__ __forceinline__ void p2_block_e(f32x16& ya, f32x16& yb, const bf16x8 (&f)[4], bf16x8 (&n)[4], bf16x8 g0, bf16x8 g1, unsigned ad,
                                           const DmaPiece& d, const __amdgpu_buffer_rsrc_t rsw, float ha, float cb, float& y) {
    asm volatile(STN_RD01 STN_M0 STN_MF2(ya, f0, g0) STN_DMA STN_RD2 STN_MF2(yb, f2, g0) STN_GEL1_A STN_RD3 STN_MF2(ya, f1, g1) STN_GEL1_B STN_MF2(yb, f3, g1)
                 "s_waitcnt lgkmcnt(0)"
                 : STN_NOUT, [ya] "+a"(ya), [yb] "+a"(yb), [ta] "=&v"(y)
                 : STN_FIN, [g0] "v"(g0), [g1] "v"(g1), [ha] "v"(ha), [cb] "v"(cb)
                 : "memory", "m0");
}
template <int O0, int DI>
__device__ __forceinline__ void p2_block_o(f32x16& ya, f32x16& yb, const bf16x8 (&f)[4], bf16x8 (&n)[4], bf16x8 g0, bf16x8 g1, unsigned ad,
                                           const DmaPiece& d, const __amdgpu_buffer_rsrc_t rsw, float ha, float cb, float yp, unsigned& gw) {
    float ta;
    asm volatile(STN_RD01 STN_M0 STN_MF2(ya, f0, g0) STN_DMA STN_RD2 STN_MF2(yb, f2, g0) STN_GEL1_A STN_RD3 STN_MF2(ya, f1, g1) STN_GEL1_B STN_GEL1_PK
                 STN_MF2(yb, f3, g1)
                 "s_waitcnt lgkmcnt(0)"
                 : STN_NOUT, [ya] "+a"(ya), [yb] "+a"(yb), [ta] "=&v"(ta), [gw] "=&v"(gw)
                 : STN_FIN, [g0] "v"(g0), [g1] "v"(g1), [ha] "v"(ha), [cb] "v"(cb), [yp] "v"(yp)
                 : "memory", "m0");
}
// ... the last block of the stage: odd, plus the bias tile of the phase 1 that comes next
template <int O0, int DI>
__device__ __forceinline__ void p2_block_o_bias(f32x16& ya, f32x16& yb, const bf16x8 (&f)[4], bf16x8 (&n)[4], bf16x8 g0, bf16x8 g1, unsigned ad,
                                                const DmaPiece& d, const __amdgpu_buffer_rsrc_t rsw, float ha, float cb, float yp, unsigned& gw, unsigned bad, f32x4 (&bq)[4]) {
    float ta;
    asm volatile(STN_RD01 STN_M0 STN_MF2(ya, f0, g0) STN_DMA STN_RD2
                 "ds_read_b128 %[b0], %[bad]\n\t"
                 "ds_read_b128 %[b1], %[bad] offset:32\n\t" STN_MF2(yb, f2, g0) STN_GEL1_A STN_RD3
                 "ds_read_b128 %[b2], %[bad] offset:64\n\t"
                 "ds_read_b128 %[b3], %[bad] offset:96\n\t" STN_MF2(ya, f1, g1) STN_GEL1_B STN_GEL1_PK STN_MF2(yb, f3, g1)
                 "s_waitcnt lgkmcnt(0)\n\t" STN_MFMA_PAD
                 : STN_NOUT, [ya] "+a"(ya), [yb] "+a"(yb), [ta] "=&v"(ta), [gw] "=&v"(gw), [b0] "=&v"(bq[0]), [b1] "=&v"(bq[1]), [b2] "=&v"(bq[2]),
                   [b3] "=&v"(bq[3])
                 : STN_FIN, [g0] "v"(g0), [g1] "v"(g1), [ha] "v"(ha), [cb] "v"(cb), [yp] "v"(yp), [bad] "v"(bad)
                 : "memory", "m0");
}
// four fragments (pieces 0..3 at `ad`): the pipeline's start
__device__ __forceinline__ void prime_frags(bf16x8 (&n)[4], unsigned ad) {
    asm volatile("ds_read_b128 %[n0], %[ad]\n\tds_read_b128 %[n1], %[ad] offset:1024\n\tds_read_b128 %[n2], %[ad] offset:2048\n\t"
                 "ds_read_b128 %[n3], %[ad] offset:3072\n\ts_waitcnt lgkmcnt(0)"
                 : [n0] "=&v"(n[0]), [n1] "=&v"(n[1]), [n2] "=&v"(n[2]), [n3] "=&v"(n[3])
                 : [ad] "v"(ad)
                 : "memory");
}
__device__ __forceinline__ void read_bias(f32x4 (&bq)[4], unsigned bad) {
    asm volatile("ds_read_b128 %[b0], %[bad]\n\tds_read_b128 %[b1], %[bad] offset:32\n\tds_read_b128 %[b2], %[bad] offset:64\n\t"
                 "ds_read_b128 %[b3], %[bad] offset:96\n\ts_waitcnt lgkmcnt(0)"
                 : [b0] "=&v"(bq[0]), [b1] "=&v"(bq[1]), [b2] "=&v"(bq[2]), [b3] "=&v"(bq[3])
                 : [bad] "v"(bad)
                 : "memory");
}
__device__ __forceinline__ void bias_to_acc(const f32x4 (&bq)[4], f32x16& h) {  // register 4q + j of lane half hf = unit 8q + 4hf + j
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) h[4 * q + j] = bq[q][j];
}

// The stage sequence: W1(0), W1(1), W2(0), W1(2), W2(1), ..., W1(T-1), W2(T-2), W2(T-1)  (2T stages; stage v lives in ring
// buffer v & 3 and — launch_ffn_pack stores the stages in this very order — at byte v * SB of the packed weights).  Where the
// pieces of stage v come from and go to, for this wave.  The ring slot of every stage of the tile loop is a compile-time constant
// (the loop body is four stages long and starts at stage 1), the stream offset is carried in one scalar, and only the loop's last
// trip can reach past the end of the stream (LIVE = false: decided at run time): the set-up of a stage is a handful of scalar
// instructions instead of the ~24 that `v & 3`, `v * SB` and `v < 2T` cost per stage when v was a run-time value — they sit between the
// stages, where no MFMA is in flight to hide them.
struct StageSrc { int so; unsigned dm0; bool live; };
template <int SB, int SLOT, bool LIVE>
__device__ __forceinline__ StageSrc ffn_src(int so, int stream_bytes, unsigned base_w) {
    StageSrc s;
    s.so = so;
    s.dm0 = base_w + (unsigned)SLOT * SB;
    s.live = LIVE ? true : so < stream_bytes;
    return s;
}
__device__ __forceinline__ DmaPiece ffn_piece(const StageSrc& s, int j, unsigned voff) {
    DmaPiece d;
    d.dm = s.dm0 + (unsigned)(j & ~3) * 1024u;
    d.dv = s.live ? voff : OOB;      // the piece index travels in the scalar + immediate offsets: one VGPR serves all pieces
    d.so = s.so + (j & ~3) * 1024;
    return d;
}
// Hand-over of stage q+1, executed in the middle of stage q (inside the stage functions): this wave's pieces of stage q+1 have
// landed (only the pieces of stage q+2, all issued by then, may still be in flight: wait_vm<PER>), and behind the barrier every
// wave is past stage q-1, whose buffer the blocks that follow fill with stage q+3.
// GELU words carried by the blocks of a stage when a block carries TWO elements (C = 384: six blocks for four words):
// word w (elements 2w, 2w+1 of the stage's half of the tile) rides in block 0, 1, 3, 4
__device__ __forceinline__ constexpr int ffn_gelu_word6(int b) { return b == 0 ? 0 : b == 1 ? 1 : b == 3 ? 2 : b == 4 ? 3 : -1; }

// One stage = NB blocks of four MFMAs.  `f` holds the fragments of block 0 on entry and of the NEXT stage's block 0 on exit.
// q = this stage's index.  Blocks 0..NB/2-1 issue the second half of stage q+2's pieces (`sa`), the hand-over of stage q+1 runs
// before block NB/2, blocks NB/2..NB-1 issue the first half of stage q+3's pieces (`sb`).
// Phase 1 of a tile into `acc`, with the GELU of elements 8..15 of the previous tile `hprev` -> g1 (GELU = false: stage 0).
// SL = this stage's ring slot (q & 3).  The fragment reads address slot s as (s < 2 ? ring_ad : ring_ad2) + (s & 1) * SB + piece: the slot part
// is in the instruction's 16-bit offset (ring_ad2 = ring_ad + 2 SB; 2 SB + the largest piece offset would not fit).
template <int C, bool GELU, int SL>
__device__ __forceinline__ void ffn_stage_p1(f32x16& acc, const f32x16& hprev, bf16x8& g1, bf16x8 (&f)[4], const bf16x8 (&xf)[C / 16],
                                             const StageSrc& sa, const StageSrc& sb, const __amdgpu_buffer_rsrc_t rsw, unsigned ring_ad, unsigned ring_ad2, unsigned voff, float cb) {
    constexpr int NB = C / 64, SB = C * 64, PER = SB / 4096, H = NB / 2;
    static_assert(NB == 6 || NB == 8, "blocks per stage");
    bf16x8 n[4];
    unsigned gw[4] = {0u, 0u, 0u, 0u};
    float y = 0.f;
    constexpr int SN = (SL + 1) & 3, OC = (SL & 1) * SB, ON = (SN & 1) * SB;
    static_assert(SB + 28672 + 3072 < 65536, "slot + piece offset must fit the ds_read offset field");
    const unsigned ad_cur = SL < 2 ? ring_ad : ring_ad2, ad_nxt = SN < 2 ? ring_ad : ring_ad2;
#define STN_XF(b) xf[4 * (b)], xf[4 * (b) + 1], xf[4 * (b) + 2], xf[4 * (b) + 3]
#define STN_P1(b, F, N, AD, OB)                                                                                                 \
    do {                                                                                                                        \
        if ((b) == H) STN_HANDOVER(PER);                                                         \
        const DmaPiece d_ = (b) < H ? ffn_piece(sa, (b) + H, voff) : ffn_piece(sb, (b) - H, voff);                              \
        constexpr int DJ = ffn_piece_imm((b) < H ? (b) + H : (b) - H);                                                          \
        if constexpr (!GELU) p1_block<OB, DJ>(acc, F, N, STN_XF(b), AD, d_, rsw);                                                        \
        else if constexpr (NB == 8 && ((b) & 1) == 0) p1_block_e<OB, DJ>(acc, F, N, STN_XF(b), AD, d_, rsw, hprev[(8 + (b)) & 15], cb, y); \
        else if constexpr (NB == 8) p1_block_o<OB, DJ, (b) == NB - 1>(acc, F, N, STN_XF(b), AD, d_, rsw, hprev[(8 + (b)) & 15], cb, y, gw[((b) >> 1) & 3]); \
        else if constexpr (ffn_gelu_word6(b) < 0) p1_block<OB, DJ>(acc, F, N, STN_XF(b), AD, d_, rsw);                                   \
        else p1_block_g<OB, DJ>(acc, F, N, STN_XF(b), AD, d_, rsw, hprev[(8 + 2 * ffn_gelu_word6(b)) & 15], hprev[(9 + 2 * ffn_gelu_word6(b)) & 15], cb, gw[ffn_gelu_word6(b) & 3]); \
    } while (0)
    // blocks alternate the two fragment sets; block b reads pieces 4(b+1).. of this stage, the last one pieces 0..3 of the next
    STN_P1(0, f, n, ad_cur, OC + 4096);
    STN_P1(1, n, f, ad_cur, OC + 8192);
    STN_P1(2, f, n, ad_cur, OC + 12288);
    STN_P1(3, n, f, ad_cur, OC + 16384);
    STN_P1(4, f, n, ad_cur, OC + 20480);
    if constexpr (NB == 6) { STN_P1(5, n, f, ad_nxt, ON); }
    else {
        STN_P1(5, n, f, ad_cur, OC + 24576);
        STN_P1(6, f, n, ad_cur, OC + 28672);
        STN_P1(7, n, f, ad_nxt, ON);
    }
#undef STN_P1
#undef STN_XF
    if constexpr (!GELU || NB == 6) asm volatile(STN_MFMA_PAD : "+v"(acc));  // (NB == 8: inside the last block)
    if constexpr (GELU) {
        const u32x4 v1 = {gw[0], gw[1], gw[2], gw[3]};
        g1 = __builtin_bit_cast(bf16x8, v1);
    }
}
// Phase 2 of a tile with its GELU'd hidden tile (g0, g1), with the GELU of elements 0..7 of the phase-1 tile `hnext` that was
// finished just before -> gn0; the last block fetches the bias tile at `bad`.
template <int C, int SL>
__device__ __forceinline__ void ffn_stage_p2(f32x16 (&yacc)[C / 32], bf16x8 g0, bf16x8 g1, const f32x16& hnext, bf16x8& gn0, bf16x8 (&f)[4],
                                             const StageSrc& sa, const StageSrc& sb, const __amdgpu_buffer_rsrc_t rsw, unsigned ring_ad, unsigned ring_ad2, unsigned voff, float cb, unsigned bad,
                                             f32x4 (&bq)[4]) {
    constexpr int NB = C / 64, SB = C * 64, PER = SB / 4096, H = NB / 2;
    bf16x8 n[4];
    unsigned gw[4] = {0u, 0u, 0u, 0u};
    float y = 0.f;
    constexpr int SN = (SL + 1) & 3, OC = (SL & 1) * SB, ON = (SN & 1) * SB;
    const unsigned ad_cur = SL < 2 ? ring_ad : ring_ad2, ad_nxt = SN < 2 ? ring_ad : ring_ad2;
#define STN_P2(b, F, N, AD, OB)                                                                                                 \
    do {                                                                                                                        \
        if ((b) == H) STN_HANDOVER(PER);                                                         \
        const DmaPiece d_ = (b) < H ? ffn_piece(sa, (b) + H, voff) : ffn_piece(sb, (b) - H, voff);                              \
        constexpr int DJ = ffn_piece_imm((b) < H ? (b) + H : (b) - H);                                                          \
        if constexpr (NB == 8 && (b) == NB - 1) p2_block_o_bias<OB, DJ>(yacc[2 * (b)], yacc[2 * (b) + 1], F, N, g0, g1, AD, d_, rsw, hnext[(b) & 15], cb, y, gw[((b) >> 1) & 3], bad, bq); \
        else if constexpr (NB == 8 && ((b) & 1) == 0) p2_block_e<OB, DJ>(yacc[2 * (b)], yacc[2 * (b) + 1], F, N, g0, g1, AD, d_, rsw, hnext[(b) & 15], cb, y); \
        else if constexpr (NB == 8) p2_block_o<OB, DJ>(yacc[2 * (b)], yacc[2 * (b) + 1], F, N, g0, g1, AD, d_, rsw, hnext[(b) & 15], cb, y, gw[((b) >> 1) & 3]); \
        else if constexpr ((b) == NB - 1) p2_block_bias<OB, DJ>(yacc[2 * (b)], yacc[2 * (b) + 1], F, N, g0, g1, AD, d_, rsw, bad, bq);   \
        else if constexpr (ffn_gelu_word6(b) < 0) p2_block<OB, DJ>(yacc[2 * (b)], yacc[2 * (b) + 1], F, N, g0, g1, AD, d_, rsw);         \
        else p2_block_g<OB, DJ>(yacc[2 * (b)], yacc[2 * (b) + 1], F, N, g0, g1, AD, d_, rsw, hnext[(2 * ffn_gelu_word6(b)) & 15], hnext[(2 * ffn_gelu_word6(b) + 1) & 15], cb, gw[ffn_gelu_word6(b) & 3]); \
    } while (0)
    STN_P2(0, f, n, ad_cur, OC + 4096);
    STN_P2(1, n, f, ad_cur, OC + 8192);
    STN_P2(2, f, n, ad_cur, OC + 12288);
    STN_P2(3, n, f, ad_cur, OC + 16384);
    STN_P2(4, f, n, ad_cur, OC + 20480);
    if constexpr (NB == 6) { STN_P2(5, n, f, ad_nxt, ON); }
    else {
        STN_P2(5, n, f, ad_cur, OC + 24576);
        STN_P2(6, f, n, ad_cur, OC + 28672);
        STN_P2(7, n, f, ad_nxt, ON);
    }
#undef STN_P2
    const u32x4 v0 = {gw[0], gw[1], gw[2], gw[3]};
    gn0 = __builtin_bit_cast(bf16x8, v0);
}

// GELU of half a tile outside the stages (the first tile's first half, the last tile's second half): same arithmetic,
// compiler-scheduled
__device__ __forceinline__ bf16x8 ffn_gelu_half(const f32x16& h, int s) {
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        w[j] = (unsigned)cvt16<(STN_V_F16 != 0)>(gelu_bf16_f(s ? h[8 + 2 * j] : h[2 * j])) | ((unsigned)cvt16<(STN_V_F16 != 0)>(gelu_bf16_f(s ? h[9 + 2 * j] : h[2 * j + 1])) << 16);
    const u32x4 v = {w[0], w[1], w[2], w[3]};
    return __builtin_bit_cast(bf16x8, v);
}

template <int C>
__global__ __launch_bounds__(256, 1) void ffn_fused_kernel(FfnArgs p) {
    constexpr int NKS = C / 16;       // phase-1 k-steps = KiB pieces of a W1 stage
    constexpr int NT2 = C / 32;       // output-channel tiles
    constexpr int SB = C * 64;        // bytes per stage (W1 tile: 32 x C x 2; W2 tile: C x 32 x 2)
    constexpr int PER = SB / 4096;    // DMA pieces per wave and stage (= blocks per stage)
    constexpr int NST = 4;
    static_assert(C == 384 || C == 512, "shape");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // ring + b2 + gamma + b1: the only LDS object
    float* const b2s = reinterpret_cast<float*>(smem + NST * SB);
    float* const gms = b2s + C;
    float* const b1s = gms + C;
    const int M = p.M, I = p.I, ldx = p.ldx, ldo = p.ldo, rv_ld = p.rv_ld, Lseq = p.L;
    const void* const xn = p.xn; const void* const wseq = p.wseq;
    const float* const b1 = p.b1; const float* const b2 = p.b2; const float* const gamma = p.gamma;
    float* const x = p.x; const int* const row_b = p.row_b; const float* const rowvec = p.rowvec; const int* const len = p.len;
    unsigned long long* const ts = p.ts;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    // Hidden split (p.split = S > 1): workgroup (slab, sp) computes the contribution of hidden tiles [sp*T, (sp+1)*T) of its 128
    // rows and stores it as a 16-bit partial sum (p.part); the fixed-order sum over sp, b2, the layer scale, the residual and the
    // time vector are applied by the next kernel that reads x (fold_dwconv_ln / fold_ln, kernels_fold.hip).  S is chosen per launch
    // from its row count (ffn_split_choose: 12 ways up to 1536 rows, 8 up to 4096, 4 beyond), so results agree across that boundary to the rounding
    // of the 16-bit partial sums, and bit for bit within one S.  The S workgroups of a slab have the same
    // blockIdx.x % 8 (one XCD under round-robin placement: they read the same xn rows; speed only).
    const int S = p.split > 1 ? p.split : 1;
    int slab = (int)blockIdx.x, sp = 0;
    if (S > 1) {
        const int g = (int)blockIdx.x >> 3;
        sp = g % S;
        slab = (g / S) * 8 + ((int)blockIdx.x & 7);
        if (slab * 128 >= M) return;  // (the grid is rounded up to whole groups of 8 slabs)
    }
    const int T = (I >> 5) / S;  // hidden tiles of this workgroup; even (the tile loop is unrolled by two)
    const int m = slab * 128 + wave * 32 + lr;  // this lane's row
    unsigned long long t_in = 0, t_first = 0, t_loop = 0;
    if (ts) t_in = __builtin_readcyclecounter();

    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const size_t wbytes = (size_t)2 * T * SB;  // this workgroup's stage stream (launch_ffn_pack stores the S streams one after another)
    const __amdgpu_buffer_rsrc_t rsw = make_rsrc(static_cast<const unsigned char*>(wseq) + (size_t)sp * wbytes, wbytes);
    const unsigned voff = (unsigned)(wave * PER * 1024 + lane * 16);
    const unsigned base_w = lds0 + (unsigned)wave * (PER * 1024);
    // This wave's rows of xn as phase-1 B fragments: lane (r, hf), k-step s holds xn[r][16s + 8hf .. +8]; rows >= M read as zeros.
    // Fragment-shaped loads straight from memory take 32 bytes of 32 different lines per instruction and fetch every line four
    // times (the slab is six times the vector L1): 9.7 k cycles for 96 KB.  The slab goes through LDS instead, in whole lines: the
    // ring is not in use yet and a wave's 32 rows are exactly one ring buffer (32 x 2C = SB bytes), so each wave LDS-DMAs its rows
    // into buffer `wave` (KiB pieces, lane-linear in LDS; the 16-byte chunk c of row r sits at chunk c ^ (r & 15) of its row, so the
    // 16 lanes of a ds_read_b128 group, whose rows differ in r & 15, hit 16 different slots of the 256-byte bank row) and reads its
    // fragments back.  Only then is the ring filled: stages 0 and 1 and the first half of stage 2 — the blocks of stage 0 carry on
    // from there.
    // C = 384 leaves room for a fifth buffer behind the biases (ffn_lds_bytes): wave 0's rows go there, ring buffer 0 is free from the
    // start and stage 0 streams in beside the slab.
    constexpr bool XSIDE = ffn_lds_has_side(C);
    static_assert(NST == 4, "ffn_lds_side_offset assumes the 4-deep ring");
    const __amdgpu_buffer_rsrc_t rsx = make_rsrc(xn, (size_t)M * ldx * 2);
    bf16x8 xf[NKS];
    if constexpr (XSIDE) {
#pragma unroll
        for (int j = 0; j < PER; ++j) dma16(rsw, smem + wave * (PER * 1024) + j * 1024, voff + j * 1024, 0);
    }
    {
        constexpr int CPR = C / 8;  // 16-byte chunks per row
        static_assert(CPR % 16 == 0 && 32 * CPR == SB / 16, "a wave's rows fill one ring buffer; the chunk swizzle stays inside its 16-chunk group");
        unsigned char* const xreg = XSIDE && wave == 0 ? smem + ffn_lds_side_offset(C, I) : smem + wave * SB;
#pragma unroll
        for (int j = 0; j < SB / 1024; ++j) {
            const int pch = j * 64 + lane, r = pch / CPR, c = (pch - r * CPR) ^ (r & 15);
            const int row = slab * 128 + wave * 32 + r;
            dma16(rsx, xreg + j * 1024, row < M ? (unsigned)row * (unsigned)ldx * 2u + (unsigned)c * 16u : OOB, 0);
        }
        // biases and layer scale into LDS behind the ring, beside the slab's pieces (the compiler's own wait for these loads is a vmcnt(0))
        for (int i = tid; i < T * 32; i += 256) b1s[i] = b1[sp * T * 32 + i];
        for (int i = tid; i < C; i += 256) { b2s[i] = b2 ? b2[i] : 0.f; gms[i] = gamma ? gamma[i] : 1.f; }
        wait_vm<0>();  // wave-private: the pieces this wave reads are its own
        const unsigned char* const xrow = xreg + lr * (2 * C);
#pragma unroll
        for (int s = 0; s < NKS; ++s) xf[s] = *reinterpret_cast<const bf16x8*>(xrow + (((2 * s + lh) ^ (lr & 15)) << 4));
    }
    __syncthreads();  // every wave holds its fragments: the buffers may be filled with weights (XSIDE: and stage 0 is in, everyone's pieces)
#pragma unroll
    for (int v = XSIDE ? 1 : 0; v < 3; ++v)
#pragma unroll
        for (int j = 0; j < (v < 2 ? PER : PER / 2); ++j)
            dma16(rsw, smem + v * SB + wave * (PER * 1024) + j * 1024, voff + j * 1024, v * SB);
    if constexpr (!XSIDE) {
        wait_vm<PER + PER / 2>();  // stage 0 is in (this wave's pieces; behind the barrier everyone's); stages 1 and 2 land under stage 0's blocks
        __builtin_amdgcn_s_barrier();
    }
    const unsigned ring_ad = lds0 + (unsigned)lane * 16u;                                   // this lane's 16 bytes of piece 0, stage buffer 0
    const unsigned bias_ad = lds0 + (unsigned)(NST * SB + 2 * C * 4) + (unsigned)lh * 16u;  // b1s + 4hf floats; tile t at + t*128 bytes
    f32x16 hA, hB;
    f32x4 bq[4];
    read_bias(bq, bias_ad);
    bias_to_acc(bq, hA);
    read_bias(bq, bias_ad + 128u);
    bias_to_acc(bq, hB);

    f32x16 yacc[NT2];
#pragma unroll
    for (int nt = 0; nt < NT2; ++nt)
#pragma unroll
        for (int i = 0; i < 16; ++i) yacc[nt][i] = 0.f;
    float cb = __builtin_bit_cast(float, 0xc0135761u);  // -2.30220819f
    asm volatile("" : "+v"(cb));

    // stage 0 is in (the barrier above drained the prologue); prime the fragment pipeline
    if (ts) t_first = __builtin_readcyclecounter();
    bf16x8 f[4], g0, g1, gn0;
    prime_frags(f, ring_ad);
    // Stage q fills stage q+2 (second half) and stage q+3 (first half); `so` = byte offset of stage q+2 in this workgroup's stream.
    const unsigned ring_ad2 = ring_ad + 2u * SB;
    const int wb = (int)wbytes;
    int so = 2 * SB;
    ffn_stage_p1<C, false, 0>(hA, hA, g1, f, xf, ffn_src<SB, 2, true>(so, wb, base_w), ffn_src<SB, 3, true>(so + SB, wb, base_w), rsw, ring_ad, ring_ad2, voff, cb);
    so += SB;
    g0 = ffn_gelu_half(hA, 0);  // first half of tile 0 (later tiles: inside the preceding phase-2 stage)
#if STN_V_STAGESTAMP
    // diagnostic build only: stamps around the four stages of the loop's second trip replace the three phase stamps
    unsigned long long sg[5] = {0, 0, 0, 0, 0};
#define STN_SG(i) do { if (t == 2) { __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(sg[i]) :: "memory"); __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define STN_SG(i) do { } while (0)
#endif
    // One trip = tiles t, t+1 = stages 2t+1 .. 2t+4 in ring slots 1, 2, 3, 0: phase 1 of tile t+1 into hB beside the second half of
    // GELU(tile t = hA); phase 2 of tile t beside the first half of GELU(tile t+1); then the same with the roles of hA and hB swapped.
    // Every trip but the last reads ahead inside the stream (LIVE); the last one (TAIL) has no third phase 1 and its read-ahead runs past the end.
#define STN_TRIP(LIVE)                                                                                                                                       \
    do {                                                                                                                                                    \
        STN_SG(0);                                                                                                                                          \
        ffn_stage_p1<C, true, 1>(hB, hA, g1, f, xf, ffn_src<SB, 3, LIVE>(so, wb, base_w), ffn_src<SB, 0, LIVE>(so + SB, wb, base_w), rsw, ring_ad, ring_ad2, voff, cb); \
        STN_SG(1);                                                                                                                                          \
        ffn_stage_p2<C, 2>(yacc, g0, g1, hB, gn0, f, ffn_src<SB, 0, LIVE>(so + SB, wb, base_w), ffn_src<SB, 1, LIVE>(so + 2 * SB, wb, base_w), rsw, ring_ad, ring_ad2, voff, cb, \
                           bias_ad + (unsigned)(LIVE || t + 2 < T ? t + 2 : 0) * 128u, bq);                                                                 \
        STN_SG(2);                                                                                                                                          \
        if (LIVE || t + 2 < T) {                                                                                                                            \
            bias_to_acc(bq, hA);                                                                                                                            \
            ffn_stage_p1<C, true, 3>(hA, hB, g1, f, xf, ffn_src<SB, 1, LIVE>(so + 2 * SB, wb, base_w), ffn_src<SB, 2, LIVE>(so + 3 * SB, wb, base_w), rsw, ring_ad, ring_ad2, voff, cb); \
            STN_SG(3);                                                                                                                                      \
            ffn_stage_p2<C, 0>(yacc, gn0, g1, hA, g0, f, ffn_src<SB, 2, LIVE>(so + 3 * SB, wb, base_w), ffn_src<SB, 3, LIVE>(so + 4 * SB, wb, base_w), rsw, ring_ad, ring_ad2, voff, cb, \
                               bias_ad + (unsigned)(LIVE || t + 3 < T ? t + 3 : 0) * 128u, bq);                                                             \
            so += 4 * SB;                                                                                                                                   \
        } else {                                                                                                                                            \
            g1 = ffn_gelu_half(hB, 1); /* (hB's MFMAs are a whole stage old) */                                                                            \
            STN_SG(3);                                                                                                                                      \
            ffn_stage_p2<C, 3>(yacc, gn0, g1, hA, g0, f, ffn_src<SB, 1, LIVE>(so + 2 * SB, wb, base_w), ffn_src<SB, 2, LIVE>(so + 3 * SB, wb, base_w), rsw, ring_ad, ring_ad2, voff, cb, \
                               bias_ad, bq);                                                                                                                \
        }                                                                                                                                                   \
        STN_SG(4);                                                                                                                                          \
        bias_to_acc(bq, hB);                                                                                                                                \
    } while (0)
    int t = 0;
    for (; t < T - 2; t += 2) STN_TRIP(true);
    STN_TRIP(false);
#undef STN_TRIP
#undef STN_SG
    wait_vm<0>();  // the zero-fill pieces of the stages past the end must have landed before this workgroup's LDS is given back
    if (ts) t_loop = __builtin_readcyclecounter();

    // ---- epilogue, hidden split: the accumulators as a 16-bit partial sum, rows whole ------------------------------------------
    // A lane holds 4 consecutive channels of its row per register quad: 8-byte pieces.  They go through a wave-private LDS image
    // [32 rows][2C + 16 bytes] (the ring is dead; the 16 bytes of padding spread the rows over the banks) and leave as whole rows:
    // every global store instruction writes one contiguous KiB of part[sp][slab*128 + wave*32 ..][:].
    if (p.part) {
        constexpr int ROWB = C * 2 + 16;
        __syncthreads();  // every wave is done with the ring's last stage
        unsigned char* const img = smem + wave * (32 * ROWB);
#pragma unroll
        for (int nt = 0; nt < NT2; ++nt)
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                uint2 w;
                w.x = (unsigned)cvt16<(STN_V_F16 != 0)>(yacc[nt][4 * qq]) | ((unsigned)cvt16<(STN_V_F16 != 0)>(yacc[nt][4 * qq + 1]) << 16);
                w.y = (unsigned)cvt16<(STN_V_F16 != 0)>(yacc[nt][4 * qq + 2]) | ((unsigned)cvt16<(STN_V_F16 != 0)>(yacc[nt][4 * qq + 3]) << 16);
                *reinterpret_cast<uint2*>(img + lr * ROWB + (32 * nt + 8 * qq + 4 * lh) * 2) = w;
            }
        unsigned char* const dst = static_cast<unsigned char*>(p.part) + ((size_t)sp * p.part_stride + (size_t)(slab * 128 + wave * 32) * C) * 2;
        if (slab * 128 + wave * 32 < M) {  // (a wavefront whose 32 rows all lie past the end has nothing anyone reads)
#pragma unroll
            for (int c = 0; c < 32 * C * 2 / 1024; ++c) {
                const int o = c * 1024 + lane * 16, row = o / (C * 2), col = o - row * (C * 2);
                *reinterpret_cast<uint4*>(dst + o) = *reinterpret_cast<const uint4*>(img + row * ROWB + col);
            }
        }
        if (ts && tid == 0) {
            __builtin_amdgcn_s_waitcnt(0);
            unsigned long long* tp = ts + (size_t)blockIdx.x * 4;
            tp[0] = t_in; tp[1] = t_first; tp[2] = t_loop; tp[3] = __builtin_readcyclecounter();
#if STN_V_STAGESTAMP
            tp[0] = sg[0]; tp[1] = sg[1]; tp[2] = sg[2]; tp[3] = sg[4];  // "first" = phase 1, "loop" = phase 2, "epilogue" = the next pair
#endif
        }
        return;
    }
    // ---- epilogue: residual update from the accumulators, 16 bytes per access ---------------------------------------------
    // yacc[nt][4q + j] is channel 32nt + 8q + 4hf + j of row r: a lane owns 4 consecutive channels per register quad
    const bool row_ok = m < M;
    int bsel = 0;
    float keep = 1.f;
    if (row_ok) {
        if (row_b) bsel = row_b[m];
        else if (len || rowvec) { bsel = m / Lseq; if (len && m - bsel * Lseq >= len[bsel]) keep = 0.f; }
    }
    float* xr = x + (size_t)(row_ok ? m : 0) * ldo;
    const float* rv = rowvec ? rowvec + (size_t)bsel * rv_ld : nullptr;
#pragma unroll
    for (int nt = 0; nt < NT2; ++nt) {
        float4 r[4], tv[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int n = 32 * nt + 8 * qq + 4 * lh;
            r[qq] = make_float4(0.f, 0.f, 0.f, 0.f); tv[qq] = r[qq];
            if (row_ok) { r[qq] = *reinterpret_cast<const float4*>(xr + n); if (rv) tv[qq] = *reinterpret_cast<const float4*>(rv + n); }
        }
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int n = 32 * nt + 8 * qq + 4 * lh;
            const float4 bb = *reinterpret_cast<const float4*>(b2s + n), gm = *reinterpret_cast<const float4*>(gms + n);
            float4 o;
            o.x = (r[qq].x + gm.x * (yacc[nt][4 * qq] + bb.x) + tv[qq].x) * keep;
            o.y = (r[qq].y + gm.y * (yacc[nt][4 * qq + 1] + bb.y) + tv[qq].y) * keep;
            o.z = (r[qq].z + gm.z * (yacc[nt][4 * qq + 2] + bb.z) + tv[qq].z) * keep;
            o.w = (r[qq].w + gm.w * (yacc[nt][4 * qq + 3] + bb.w) + tv[qq].w) * keep;
            if (row_ok) *reinterpret_cast<float4*>(xr + n) = o;
        }
    }
    if (ts && tid == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        unsigned long long* tp = ts + (size_t)blockIdx.x * 4;
        tp[0] = t_in; tp[1] = t_first; tp[2] = t_loop; tp[3] = __builtin_readcyclecounter();
    }
}


#undef STN_RD01
#undef STN_RD2
#undef STN_RD3
#undef STN_DMA
#undef STN_M0
#undef STN_MFMA_PAD
#undef STN_MFMA_OP
#undef STN_CVT_PK
#undef STN_MF1
#undef STN_MF2
#undef STN_GELU_A
#undef STN_GELU_B
#undef STN_GELU_C
#undef STN_GEL1_A
#undef STN_GEL1_B
#undef STN_GEL1_PK
#undef STN_ACCC
#undef STN_NOUT
#undef STN_FIN
#undef STN_HANDOVER
#undef STN_V_F16
#undef STN_V_NODMA
#undef STN_V_NOGELU
#undef STN_V_EARLYRD
#undef STN_V_NOBAR
#undef STN_V_STAGESTAMP
