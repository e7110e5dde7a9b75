#!/usr/bin/env python3
"""Long-form synthesis throughput (hifigan/longform.py): D documents of N sentences with synthetic
LJSpeech-like lengths (matcha_hip.synthetic, the weights and text recipe of bench.py), through LongForm at
max_batch 1, 8 and 32, and the time of the join chain (mt_audio_edges + mt_join_plan + mt_join) alone against the
vocoder time of the same run. Needs the MI355X; writes one JSON record (default profiles/longform_bench.json) and
prints it on one line.

    python tools/longform_bench.py [--docs 8] [--sentences 24] [--reps 3] [--out profiles/longform_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(HERE, "matcha-tts_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


class TimedVocoder:
    """the generator behind device events: LongForm calls it once per batch"""

    def __init__(self, g):
        self.g, self.events = g, []

    def __call__(self, mel, lengths=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = self.g(mel, lengths=lengths)
        b.record()
        self.events.append((a, b))
        return out

    def take_ms(self) -> float:
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for a, b in self.events)
        self.events = []
        return ms


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--docs", type=int, default=8)
    ap.add_argument("--sentences", type=int, default=24)
    ap.add_argument("--n-timesteps", type=int, default=10)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chain-reps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "longform_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("longform_bench: no ROCm GPU; nothing is measured on a CPU", file=sys.stderr)
        return 2

    import bench
    from hifigan.longform import LongForm
    from hifigan.output import AudioOutput
    from matcha_hip import runtime as rt
    from matcha_hip import synthetic

    dev = torch.device("cuda", 0)
    m, g, den, _, _ = bench.build_models(dev, a.precision, a.seed)
    S = a.docs * a.sentences
    x, xl = synthetic.synthetic_text(S, seed=a.seed)
    sents = [torch.from_numpy(x[i, :xl[i]].copy()).to(dev) for i in range(S)]
    docs = [sents[d * a.sentences:(d + 1) * a.sentences] for d in range(a.docs)]
    seeds = list(range(1, a.docs + 1))
    output = AudioOutput(16000, loudness=-16.0, encoding="pcm16")
    voc = TimedVocoder(g)

    runs = []
    for mb in (1, 8, 32):
        lf = LongForm(m, voc, den, output, n_timesteps=a.n_timesteps, max_batch=mb)
        for _ in range(a.warmup):
            lf(docs, seeds=seeds)
        voc.take_ms()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            doc = lf(docs, seeds=seeds)
        torch.cuda.synchronize()
        sec = (time.perf_counter() - t0) / a.reps
        audio_s = float(doc.lengths.sum()) / doc.sample_rate
        runs.append({"max_batch": mb, "sec_per_call": sec, "audio_seconds": audio_s,
                     "audio_seconds_per_second": audio_s / sec, "vocoder_ms_per_call": voc.take_ms() / a.reps})

    # the join chain alone, on the rows of the last configuration (its one device -> host copy included)
    seg, lens, doc_first = lf.segments(docs, seeds=seeds)
    gap = torch.tensor(lf._gaps(None, doc_first.tolist()), dtype=torch.int32, device=dev)

    def chain():
        start, end = lf.edges(seg, lens)
        dst, doc_len, bad = rt.join_plan(doc_first, start, end, gap, lf.head, lf.tail, seg.shape[1])
        return start, end, rt.join(seg, start, end, doc_first, dst, doc_len, lf.fade, bad=bad), doc_len

    for _ in range(3):
        start, end, joined, doc_len = chain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.chain_reps):
        chain()
    torch.cuda.synchronize()
    chain_ms = (time.perf_counter() - t0) / a.chain_reps * 1e3
    kept = float((end - start).sum()) / max(float(lens.sum()), 1.0)
    # bytes the three kernels move: 4 per valid sample read by edges; per document sample one fp32
    # store and 4 per covering segment sample read
    moved = 4.0 * float(lens.sum()) + 4.0 * joined.numel() + 4.0 * float((end - start).sum())
    rec = {"tool": "longform_bench", "device": torch.cuda.get_device_name(0), "dtype": a.precision,
           "docs": a.docs, "sentences_per_doc": a.sentences, "n_timesteps": a.n_timesteps, "sample_rate": 16000,
           "segment_rows": list(seg.shape), "document_rows": list(joined.shape), "kept_fraction": kept,
           "runs": runs, "join_chain_ms": chain_ms, "join_chain_bytes": moved,
           "vocoder_ms_same_run": runs[-1]["vocoder_ms_per_call"],
           "join_chain_over_vocoder": chain_ms / runs[-1]["vocoder_ms_per_call"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
