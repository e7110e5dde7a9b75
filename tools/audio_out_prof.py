"""The audio output stage's three launches at the bench's batch, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/audio_out_prof.py --rate 16000

B utterances at synthetic.ljspeech_lengths (mel frames, x 256 samples) in one padded [B, L] buffer of noise; each
iteration runs the ragged denoiser (the stage this one follows, for comparison) and AudioOutput(rate, "peak", "pcm16");
with --loudness LUFS also AudioOutput(rate, loudness=LUFS) (the K-weighting scan and the true peak),
and with --limiter MS also AudioOutput(rate, loudness=LUFS or -16, limiter=MS) (the look-ahead limiter).
Prints one JSON line: the shapes, and the bytes each launch has to move with their time at the HBM rate DESIGN.md §4
uses. Kernel times come from the trace, not from this script.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "matcha-tts_amd"))

HBM = 8.0e12  # B/s, DESIGN.md §4


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rate", type=int, default=16000)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--encoding", default="pcm16")
    p.add_argument("--loudness", type=float, default=None,
                   help="also run AudioOutput(rate, loudness=LUFS) on the same batch each iteration (DESIGN.md §21)")
    p.add_argument("--limiter", type=float, default=None,
                   help="also run AudioOutput(rate, loudness=LUFS or -16, limiter=MS) each iteration (DESIGN.md §23)")
    a = p.parse_args()
    from hifigan.output import AudioOutput
    from matcha_hip import audio_out, synthetic
    from matcha_hip import runtime as rt
    dev = torch.device("cuda", 0)
    lens = synthetic.ljspeech_lengths(a.batch)
    L = 256 * int(lens.max())
    g = torch.Generator().manual_seed(0)
    audio = (torch.randn(a.batch, L, generator=g) * 0.2).clamp_(-1, 1).to(dev)
    ld = torch.from_numpy(lens.astype(np.int32)).to(dev)
    bias = torch.rand(513, generator=g).to(dev)
    stage = AudioOutput(a.rate, normalize="peak", encoding=a.encoding)
    leveled = None if a.loudness is None else AudioOutput(a.rate, loudness=a.loudness, encoding=a.encoding)
    limited = None if a.limiter is None else AudioOutput(
        a.rate, loudness=-16.0 if a.loudness is None else a.loudness, limiter=a.limiter, encoding=a.encoding)
    for _ in range(a.warmup + a.iters):
        d = rt.denoise(audio, bias, 0.00025, lengths=ld)
        out = stage(d, ld)
        if leveled is not None:
            leveled(d, ld)
        if limited is not None:
            limited(d, ld)
    torch.cuda.synchronize()
    up, down = audio_out.rates(22050, a.rate)
    n_in = int(256 * lens.sum())
    n_out = int(out.lengths.sum())
    Lout = out.audio.shape[1]
    esz = out.audio.element_size()
    moved = {"resample_kernel": 4 * n_in + 4 * a.batch * Lout,           # valid samples in, whole rows out
             "audio_stats_kernel": 4 * n_out,
             "audio_encode_kernel": (4 + esz) * a.batch * Lout}
    if limited is not None:  # per launch: samples in and envelope out; samples and envelope in, whole rows out
        moved["peak_envelope_kernel"] = 4 * n_out + 4 * a.batch * Lout
        moved["limit_kernel"] = 8 * n_out + 4 * a.batch * Lout
    print(json.dumps({"rate": a.rate, "up": up, "down": down, "batch": a.batch, "L": L, "Lout": Lout,
                      "samples_in": n_in, "samples_out": n_out, "iters": a.warmup + a.iters,
                      "bytes": moved, "hbm_us": {k: round(v / HBM * 1e6, 2) for k, v in moved.items()}}))


if __name__ == "__main__":
    main()
