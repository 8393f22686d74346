"""The join of a long text in plain numpy / Python: what the reference's hosts do with the chunks of `TextToSpeech::call`.

WHOLE: every chunk's untrimmed wave, zeros between (/root/reference/cpp/helper.cpp:706-715, py/helper.py:235-243).
TRIM: every chunk cut at its reported duration first, `wav_len = (sample_rate * duration) as usize` with the product in fp32
(/root/reference/rust/src/helper.rs:700-713).  The duration of the joined text is the fp32 sum in member order,
`d = dur_0; d += dur_i + silence` (cpp/helper.cpp:708,714).  No engine code is used here."""
import numpy as np

WHOLE, TRIM = 0, 1
ZERO_CODEWORD = {"f32": 0, "pcm16": 0, "pcm24": 0, "mulaw": 0xFF, "alaw": 0xD5}


def member_lengths(member_len, member_dur, hz, mode):
    """The samples each member gives: its whole length, or (TRIM) the first int(float32(dur) * float32(hz)) of them."""
    out = []
    for n, d in zip(member_len, member_dur):
        n = int(n)
        if mode == TRIM:
            n = max(0, min(n, int(np.float32(d) * np.float32(hz))))
        out.append(n)
    return out


def plan(rows, gap_samples, gap_seconds, member_len, member_dur, hz, mode=WHOLE):
    """-> dict(W_join, prog_len [G], prog_dur [G] float32, seg_len [B], seg_dst [B]); rows[g] consecutive members per programme."""
    lens = member_lengths(member_len, member_dur, hz, mode)
    prog_len, prog_dur, seg_dst = [], [], []
    i = 0
    for g, k in enumerate(rows):
        at, d = 0, np.float32(0)
        for m in range(int(k)):
            if m == 0:
                d = np.float32(member_dur[i])
            else:
                at += int(gap_samples[g])
                d = np.float32(d + np.float32(np.float32(member_dur[i]) + np.float32(gap_seconds[g])))
            seg_dst.append(at)
            at += lens[i]
            i += 1
        prog_len.append(at)
        prog_dur.append(d)
    assert i == len(lens)
    return {"W_join": max(prog_len), "prog_len": np.array(prog_len, np.int64), "prog_dur": np.array(prog_dur, np.float32),
            "seg_len": np.array(lens, np.int64), "seg_dst": np.array(seg_dst, np.int64)}


def join(rows_enc, seg_len, rows, gap_samples, zero):
    """rows_enc [B, W(, 3)]: the members' rows in some encoding; member i gives its first seg_len[i] samples.  -> list of G arrays: the
    members of each programme with gap_samples[g] samples of `zero` between two of them."""
    out, i = [], 0
    for g, k in enumerate(rows):
        parts = []
        for m in range(int(k)):
            if m > 0:
                sil = np.empty((int(gap_samples[g]),) + rows_enc.shape[2:], rows_enc.dtype)
                sil[...] = zero
                parts.append(sil)
            parts.append(rows_enc[i, : int(seg_len[i])])
            i += 1
        out.append(np.concatenate(parts))
    return out


def padded(progs, width, zero):
    """The programmes as one [G, width(, 3)] array, `zero` behind each programme's end."""
    y = np.empty((len(progs), width) + progs[0].shape[1:], progs[0].dtype)
    y[...] = zero
    for g, p in enumerate(progs):
        y[g, : len(p)] = p
    return y
