#!/usr/bin/env python3
"""What the formant correction costs, by tools/pitch_cost.py's protocol: a pcm16 fetch of a C3-sized batch (128
utterances of the default architecture on synthetic weights) and of one row, with pitch on in mode "formant" against the same fetch in
mode "resample", wall clock around the call and the output stage's spans per kernel family (out.formant_lpc and out.formant_filter
beside out.pitch_search).  The modes are interleaved round by round and the medians printed with their ranges; the rows are kept per
batch, shift and mode, so the shift is set again in front of every timed fetch (that drops them).

    python tools/formant_cost.py [--rounds 15] [--rows 128] [--semitones 4]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from supertonic_amd import binding, host, workload  # noqa: E402
from supertonic_amd.arch import default_arch  # noqa: E402

TAGS = ("out.pitch_search", "out.pitch_ola", "out.pitch_resample", "out.formant_lpc", "out.formant_filter")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--semitones", type=float, default=4.0)
    args = ap.parse_args()
    arch = default_arch()
    hz = arch.sample_rate
    out = {"semitones": args.semitones, "hz": hz, "plan": {k: v for k, v in binding.formant_plan(hz, 1).items() if k != "lag"}}
    e = binding.Engine(0, "bf16")
    e.load_synthetic(arch, 7)
    for rows in (args.rows, 1):
        texts = workload.utterances(args.rows, min_words=3, max_words=12, seed=11)[:rows]
        ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * rows)
        sttl, sdp = workload.synthetic_styles(arch, list(range(rows)))
        e.batch_upload(ids, mask, sttl, sdp, duration_override=workload.forced_durations(texts))
        e.batch_run(5, 1.05, 1)
        B, _, Wb = e.batch_dims()
        modes = ("resample", "formant")
        for m in modes:  # warm: the table, the scratch
            e.set_pitch_mode(m)
            e.set_pitch(args.semitones)
            e.batch_fetch_encoded("pcm16")
        wall = {m: [] for m in modes}
        fam = {m: {} for m in modes}
        for _ in range(args.rounds):
            for m in modes:
                e.set_pitch_mode(m)
                e.set_pitch(args.semitones)
                e.sync()
                t0 = time.perf_counter()
                e.batch_fetch_encoded("pcm16")
                wall[m].append((time.perf_counter() - t0) * 1e6)
        e.profile_enable(True)
        for _ in range(args.rounds):
            for m in modes:
                e.set_pitch_mode(m)
                e.set_pitch(args.semitones)
                e.profile_reset()
                e.batch_fetch_encoded("pcm16")
                for f, st in e.profile().items():
                    fam[m].setdefault(f, []).append(st["ms"] * 1e3)
        e.profile_enable(False)
        print(f"pcm16 fetch of {B} rows x {Wb} samples at {hz} Hz, pitch {args.semitones:+g}; median [min, max] of {args.rounds} interleaved rounds, us")
        for m in modes:
            w = statistics.median(wall[m])
            spans = {f: (statistics.median(v), min(v), max(v)) for f, v in fam[m].items() if f in TAGS}
            out[f"rows{B}_{m}"] = dict(W=Wb, wall_us=round(w, 1), wall_min_us=round(min(wall[m]), 1), wall_max_us=round(max(wall[m]), 1),
                                       spans={f: [round(x, 1) for x in v] for f, v in spans.items()})
            print(f"  {m:8s}: wall {w:9.1f} [{min(wall[m]):.1f}, {max(wall[m]):.1f}]   " + "  ".join(f"{f} {v[0]:.1f} [{v[1]:.1f}, {v[2]:.1f}]" for f, v in spans.items()))
    print(json.dumps(out))
    e.close()


if __name__ == "__main__":
    main()
