#!/usr/bin/env python3
"""Forced-aligner timing: mt_align (direct log-prior + textbook MAS, two launches, a bit table) against what the
repository offered for the same job before it, train.log_prior + mt_maximum_path (about ten launches, an fp32
(Tx + Ty) x Tx table), on a padded batch of full-length utterances. Default stream, device events, 20 runs after 5
warm-ups; prints one JSON line.
Usage: python tools/align_bench.py [B] [Tx] [Ty]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "matcha-tts_amd"))
sys.path.insert(0, HERE)
import torch  # noqa: E402

from matcha_hip import runtime as rt  # noqa: E402
from matcha_hip import train as tr  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
TX = int(sys.argv[2]) if len(sys.argv) > 2 else 200
TY = int(sys.argv[3]) if len(sys.argv) > 3 else 800
g = torch.Generator().manual_seed(0)
mu = torch.randn(B, 80, TX, generator=g).cuda()
y = (1.3 * torch.randn(B, 80, TY, generator=g) + 0.2).cuda()
t_xs = torch.full((B,), TX, dtype=torch.int32).cuda()
t_ys = torch.full((B,), TY, dtype=torch.int32).cuda()
mask = torch.ones(B, TX, TY).cuda()
mu_btc, y_btc = mu.transpose(1, 2).contiguous(), y.transpose(1, 2).contiguous()


def new():
    return rt.align(mu, y, t_xs, t_ys)[0]


def new_attn():
    return rt.align(mu, y, t_xs, t_ys, want_attn=True)[1]


def old():
    return rt.maximum_path(tr.log_prior(mu_btc, y_btc), mask)


def timed(fn, runs=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


res = {"shape": {"B": B, "Tx": TX, "Ty": TY}}
for rnd in (1, 2):  # alternate, to see the spread
    for name, fn in (("log_prior+mt_maximum_path", old), ("mt_align", new), ("mt_align+attn", new_attn)):
        res[f"{name}#{rnd}"] = timed(fn)
print(json.dumps(res), flush=True)
