#!/usr/bin/env python3
"""In-process A/B of the output-store policy (plain against write-through sc1 stores, bit-identical) on the bench
step's vocoder and text encoder: interleaved rounds, median and min per setting, outputs compared. The vocoder runs
the step's ragged launch chain on the mel the bench's synthesize produces, once per stage mask
(mt_vocoder_set_store_policy: bit i = stage i); the encoder runs the bench's text batch with
mt_encoder_set_store_policy 0 / 1. The decoder's bits are timed by tools/deck_ab.py (masks 3,7,11,15).
Usage: python tools/store_policy_ab.py voc|enc [B] [rounds] [settings, e.g. 0,1,2,4,8,15]"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "matcha-tts_amd"))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import bench  # noqa: E402

fam = sys.argv[1] if len(sys.argv) > 1 else "voc"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
R = int(sys.argv[3]) if len(sys.argv) > 3 else 7
default = "0,1,2,4,8,15" if fam == "voc" else "0,1"
SET = [int(c) for c in (sys.argv[4] if len(sys.argv) > 4 else default).split(",")]
REPS = 4
dev = torch.device("cuda", 0)
m, g, _, _, _ = bench.build_models(dev, "bf16", 1234)
x, xl = bench.shard_inputs(0, 1, B, 1234)
x, xl = x.to(dev), xl.to(dev)
res = {s: [] for s in SET}
outs = {}
with torch.inference_mode():
    if fam == "voc":
        mel, yl, _ = m.synthesize(x, xl, n_timesteps=10, temperature=0.667, length_scale=1.0)
        eng, base = g.engine(), 0
        run = lambda: g(mel, lengths=yl)  # noqa: E731
    else:
        m.encoder(x, xl)  # checked once (OOV ids raise)
        eng, base = m.encoder.engine(), 0
        run = lambda: m.encoder.forward_unchecked(x, xl)  # noqa: E731
    for r in range(R + 1):
        for s in SET:
            eng.set_store_policy(s)
            run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                o = run()
            e1.record()
            torch.cuda.synchronize()
            if r > 0:
                res[s].append(e0.elapsed_time(e1) / REPS)
            outs[s] = [t.clone() for t in (o if isinstance(o, (tuple, list)) else (o,)) if torch.is_tensor(t)]
    eng.set_store_policy(base)
for s in SET:
    v = sorted(res[s])
    print(f"{fam} B={B} store policy {s}: median {v[len(v) // 2]:.4f} ms min {v[0]:.4f} ms max {v[-1]:.4f} ms", flush=True)
print("outputs equal:", all(all(torch.equal(a, b) for a, b in zip(outs[s], outs[SET[0]])) for s in SET))
