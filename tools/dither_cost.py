#!/usr/bin/env python3
"""What the dithered PCM stores cost: the output stage's own spans (stn_profile_*) of one fetch of a C3-sized
batch (128 utterances of the default architecture on synthetic weights), PCM16 and PCM24, every dither mode, for the plain store, the
trimmed store and the resample-only fetch at 16 kHz.  The configurations are interleaved round by round and the median over the rounds
is printed per kernel family, with its ratio to the same path's mode-off span.

    python tools/dither_cost.py [--rounds 15] [--rows 128]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from supertonic_amd import binding, host, workload  # noqa: E402
from supertonic_amd.arch import default_arch  # noqa: E402

MODES = ("off", "round", "tpdf", "tpdf-hp")
PATHS = {"store": dict(), "trim": dict(trim=40.0), "resample_16k": dict(rate=16000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--rows", type=int, default=128)
    args = ap.parse_args()
    arch = default_arch()
    texts = workload.utterances(args.rows, min_words=3, max_words=12, seed=11)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * args.rows)
    sttl, sdp = workload.synthetic_styles(arch, list(range(args.rows)))
    e = binding.Engine(0, "bf16")
    e.load_synthetic(arch, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=workload.forced_durations(texts))
    e.batch_run(5, 1.05, 1)
    B, _, W = e.batch_dims()
    configs = [(p, enc, m) for p in PATHS for enc in ("pcm16", "pcm24") for m in MODES]

    def setup(path, mode):
        s = PATHS[path]
        e.set_output_rate(s.get("rate", 0))
        e.set_silence_trim(s.get("trim"))
        e.set_dither(mode, 1)

    for path, enc, mode in configs:  # warm: tables, scratch, the edges of the trimmed path
        setup(path, mode)
        e.batch_fetch_encoded(enc)
    us = {c: {} for c in configs}
    e.profile_enable(True)
    for _ in range(args.rounds):
        for c in configs:
            setup(c[0], c[2])
            e.profile_reset()
            e.batch_fetch_encoded(c[1])
            for fam, st in e.profile().items():
                us[c].setdefault(fam, []).append(st["ms"] * 1e3)
    e.profile_enable(False)
    print(f"{B} rows x {W} samples at {arch.sample_rate} Hz; median of {args.rounds} interleaved rounds, microseconds per fetch")
    out = {}
    for path, enc, mode in configs:
        med = {fam: statistics.median(v) for fam, v in us[(path, enc, mode)].items()}
        total = sum(med.values())
        base = sum(statistics.median(v) for v in us[(path, enc, "off")].values())
        out[f"{path}/{enc}/{mode}"] = dict(total_us=round(total, 2), ratio_to_off=round(total / base, 3), families={k: round(v, 2) for k, v in med.items()})
        print(f"  {path:13s} {enc:6s} {mode:8s} {total:9.1f} us  x{total / base:5.2f}   " + "  ".join(f"{k} {v:.1f}" for k, v in med.items()))
    print(json.dumps(out))
    e.close()


if __name__ == "__main__":
    main()
