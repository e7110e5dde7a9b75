#!/usr/bin/env python3
"""Recording input stage timing (hifigan/input.py, csrc/mt_audio_in.hip) on the ragged lengths of
bench.py's 32-utterance batch: its y_lengths x 256 samples at 22,050 Hz (the bench's forced durations give 3 frames a
token, 18,765 frames in all). Three things are timed, alternating in rounds within one process:

  (a) the ragged featurizer: ONE mt_log_mel_ragged launch on the padded batch;
  (b) the same work the way it had to be done before: a loop of per-row mel_spectrogram calls (32 mt_log_mel launches);
  (c) the full AudioInput call from 48 kHz stereo PCM16 of the same durations (decode, resample, peak level, trim,
      ragged log-mel, and its one host read).

(a) and (b) are checked to give the same bits before anything is timed. Needs the MI355X; writes one JSON record
(default profiles/featurize_bench.json) and prints it on one line.

    python tools/featurize_bench.py [--reps 200] [--rounds 7] [--out profiles/featurize_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(HERE, "matcha-tts_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FRAMES_PER_TOKEN = 3  # bench.build_models: force_log_duration = log 2.5, ceil(2.5) frames a token


def timed(fn, reps: int) -> float:
    """milliseconds per call: a host clock around `reps` calls that end in a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--reps", type=int, default=200, help="calls per timed window (about 0.1 s each)")
    ap.add_argument("--rounds", type=int, default=7, help="windows per variant, alternating; the median is reported")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "featurize_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("featurize_bench: no ROCm GPU; nothing is measured on a CPU", file=sys.stderr)
        return 2

    from hifigan.input import AudioInput
    from hifigan.meldataset import mel_basis, mel_spectrogram
    from matcha_hip import audio_out, synthetic
    from matcha_hip import runtime as rt

    dev = torch.device("cuda", 0)
    _, xl = synthetic.synthetic_text(a.batch, seed=a.seed)
    y_lengths = [FRAMES_PER_TOKEN * int(v) for v in xl]
    n22 = [256 * f for f in y_lengths]
    B, L = a.batch, max(n22)
    g = torch.Generator().manual_seed(a.seed)
    audio = ((torch.rand(B, L, generator=g) * 2 - 1) * 0.5)
    for b, n in enumerate(n22):
        audio[b, n:] = 0.0
    audio = audio.to(dev)
    lens = torch.tensor(n22, dtype=torch.int32, device=dev)
    basis = mel_basis(22050, 1024, 80, 0, 8000, dev)
    args = (1024, 80, 22050, 256, 1024, 0, 8000)

    def ragged():
        return rt.log_mel_ragged(audio, basis, None, lens)

    def per_row():
        return [mel_spectrogram(audio[b, :n], *args) for b, n in enumerate(n22)]

    # 48 kHz stereo PCM16 of the same durations: ceil(n 320 / 147) frames come back as n samples or one more
    n48 = [-(-n * 320 // 147) for n in n22]
    L48 = max(n48)
    pcm = torch.randint(-12000, 12000, (B, L48 * 2), generator=g, dtype=torch.int16)
    for b, n in enumerate(n48):
        pcm[b, : (n // 10) * 2] = 0          # a silent lead-in and tail for the trim to find
        pcm[b, (n - n // 10) * 2:] = 0
    pcm, lens48 = pcm.to(dev), torch.tensor(n48, dtype=torch.int32, device=dev)
    stage = AudioInput(48000, "pcm16", channels=2, normalize="peak", trim_db=-40.0, trim_pad_ms=10.0)

    def full():
        return stage(pcm, lens48)

    # same bits first
    mel, frames = ragged()
    rows = per_row()
    assert frames.tolist() == y_lengths, "frame counts differ from the bench's y_lengths"
    for b, f in enumerate(y_lengths):
        assert torch.equal(mel[b, :, :f], rows[b]), f"row {b}: the ragged call and the per-row call differ"
    rec48 = full()
    assert audio_out.rates(48000, 22050) == (147, 320)

    variants = {"ragged": ragged, "per_row_loop": per_row, "audio_input_48k_stereo_pcm16": full}
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, a.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    total_frames = sum(y_lengths)
    rec = {"tool": "featurize_bench", "device": torch.cuda.get_device_name(0), "batch": B, "frames": total_frames,
           "samples_22050": int(sum(n22)), "padded_shape": [B, L], "reps": a.reps, "rounds": a.rounds,
           "ms_per_call_median": med, "ms_per_call_min": {k: min(v) for k, v in times.items()},
           "ms_per_call_max": {k: max(v) for k, v in times.items()},
           # kernels of the library per call, counted from the launchers (mt_resample: table + tile kernel,
           # mt_audio_stats and mt_audio_edges: tiles + final); AudioInput adds torch's elementwise ops on [B] vectors
           "library_launches": {"ragged": 1, "per_row_loop": B, "audio_input_48k_stereo_pcm16": 1 + 2 + 2 + 2 + 1},
           "ragged_speedup_over_loop": med["per_row_loop"] / med["ragged"],
           "ragged_frames_per_s": total_frames / (med["ragged"] * 1e-3),
           "audio_input_mel_frames": int(rec48.mel_lengths.sum()),
           "audio_input_audio_seconds_per_s": float(np.sum(n48)) / 48000.0 / (med["audio_input_48k_stereo_pcm16"] * 1e-3),
           "bits_equal_ragged_vs_loop": True}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
