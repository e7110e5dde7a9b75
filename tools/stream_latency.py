"""Time to first audio of streaming delivery against the one-shot path:

    python tools/stream_latency.py [--out profiles/stream_latency.json]

From a finished mel (the end of the CFM solve) to delivered 16 kHz PCM16, for (B, T) = (1, 728) and (32, 728), every
row T frames long, bf16 vocoder with synthetic weights, denoiser strength 0.00025:
  one-shot  Generator.forward(mel, lengths) -> Denoiser.forward -> AudioOutput (the calls as they were before
            streaming existed; they are unchanged)
  stream    WaveStreamer(chunk_frames=32, first_chunk_frames=8): time to the first non-empty chunk, and to the last
Device events on the stream (one before the first launch, one after each chunk), so the times include the host's
launch work where the GPU waits for it. Warm-up runs of both paths first, then `--repeats` (default 20) alternating
measurements; medians and the spread (min, max) are reported. The stream's result is compared with the one-shot's
bit for bit once per shape. Prints one JSON line per shape and writes them all to --out. Not part of the test suite.

Level in the stream: `--gain-db G` gives the output stage a fixed gain, `--limiter MS` with it the
look-ahead limiter at -1 dBTP (the one-shot path then runs the same stage); written to
profiles/stream_latency_limiter.json with `--out`. The chunks end `added_delay_samples` earlier than without.

Launches per step: `rocprofv3 --kernel-trace --stats ... -- python tools/stream_latency.py --trace-streams K` for two
values of K; the difference of the two call counts belongs to the streams alone (tools/stream_launches.py).
"""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "matcha-tts_amd"))


def _generator(dev):
    from hifigan.config import v1
    from hifigan.env import AttrDict
    from hifigan.models import Generator
    from matcha_hip import synthetic
    g = Generator(AttrDict(v1), precision="bf16")
    sd = synthetic.make_state_dict([(k, tuple(v.shape)) for k, v in g.state_dict().items()], 8)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    g = g.to(dev).eval()
    g.remove_weight_norm()
    return g


def _stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(HERE, "profiles", "stream_latency.json"))
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--chunk", type=int, default=32)
    p.add_argument("--first", type=int, default=8)
    p.add_argument("--rate", type=int, default=16000)
    p.add_argument("--shapes", default="1x728,32x728")
    p.add_argument("--gain-db", type=float, default=None, help="a fixed gain in dB for the output stage")
    p.add_argument("--limiter", type=float, default=None, help="with --gain-db: the limiter's window in ms")
    p.add_argument("--trace-streams", type=int, default=0,
                   help="run only this many streams of the first shape, untimed, and exit: for a kernel trace (two "
                        "runs with different counts; their difference is the launches of the streams alone)")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_latency: needs the GPU (a time taken anywhere else says nothing)")
    from hifigan.denoiser import Denoiser
    from hifigan.output import AudioOutput
    from hifigan.stream import WaveStreamer
    dev = torch.device("cuda", 0)
    g = _generator(dev)
    den = Denoiser(g, mode="zeros")
    if a.limiter is not None and a.gain_db is None:
        raise SystemExit("stream_latency: --limiter needs --gain-db")
    out = AudioOutput(a.rate, encoding="pcm16", gain_db=a.gain_db, true_peak=-1.0, limiter=a.limiter)
    s = WaveStreamer(g, den, out, chunk_frames=a.chunk, first_chunk_frames=a.first, strength=0.00025)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    results = []
    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        mel = (torch.randn(B, 80, T, generator=torch.Generator().manual_seed(9)) * 2.1 - 5.5).to(dev)
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        host_lens = [T] * B

        def one_shot():
            e0, e1 = ev(), ev()
            e0.record()
            w = g(mel, lens)
            d = den(w.squeeze(1), 0.00025, lens)
            o = out(d, lens)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1), o

        def stream(keep=False):
            e0 = ev()
            marks, chunks = [], []
            e0.record()
            for ch in s(mel, host_lens):  # lengths from the host: the solve's caller has them (synthesize's y_lengths)
                e = ev()
                e.record()
                marks.append((e, ch.audio.shape[1]))
                if keep:
                    chunks.append(ch)
            marks[-1][0].synchronize()
            first = next(e for e, n in marks if n > 0)
            return e0.elapsed_time(first), e0.elapsed_time(marks[-1][0]), chunks, len(marks)

        if a.trace_streams:
            for _ in range(a.trace_streams):
                stream()
            torch.cuda.synchronize()
            return
        for _ in range(a.warmup):
            one_shot()
            stream()
        _, ref = one_shot()
        _, _, chunks, steps = stream(keep=True)
        got = torch.cat([c.audio for c in chunks], dim=1)
        n = int(ref.lengths[0])
        same = bool(torch.equal(got[:, :n], ref.audio[:, :n])) and got.shape[1] == n
        t_one, t_first, t_last = [], [], []
        for _ in range(a.repeats):
            t_one.append(one_shot()[0])
            f, l, _, _ = stream()
            t_first.append(f)
            t_last.append(l)
        pl = s.plan(host_lens, dev)
        first_step = next(st for st in pl.steps if st.delivered[1] > st.delivered[0])
        delay = 0 if pl.window is None else pl.env_reach + pl.window - 1
        r = {"B": B, "T": T, "chunk_frames": a.chunk, "first_chunk_frames": a.first, "rate": a.rate,
             "encoding": "pcm16", "gain_db": a.gain_db, "limiter_ms": a.limiter, "added_delay_samples": delay,
             "repeats": a.repeats, "warmup": a.warmup, "steps": steps,
             "first_chunk_step": first_step.index,
             "first_chunk_samples": first_step.delivered[1] - first_step.delivered[0],
             "first_window_frames": max(first_step.voc.length), "max_window_frames": pl.max_vocoder_window,
             "vocoder_frames_streamed": sum(sum(st.voc.length) for st in pl.steps) // B,
             "bit_identical_to_one_shot": same,
             "min_reduction": None if s.reduction is None else round(float(s.reduction.min()), 6),
             "one_shot": _stats(t_one), "stream_first_chunk": _stats(t_first), "stream_last_chunk": _stats(t_last)}
        print(json.dumps(r), flush=True)
        results.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/stream_latency.py", "device": torch.cuda.get_device_name(0), "results": results}, f,
                  indent=1)
        f.write("\n")
    if not all(r["bit_identical_to_one_shot"] for r in results):
        raise SystemExit("stream_latency: the stream's result is not the one-shot result")


if __name__ == "__main__":
    main()
