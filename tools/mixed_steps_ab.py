#!/usr/bin/env python3
"""In-process A/B of a CFM solve with two step counts in one batch (DESIGN.md "Per-utterance step counts"): the bf16
Euler solve alone at B x T, ragged like the bench (the longest utterance T - 4 frames), seeded noise, half the rows
(the odd ones, so the sort has work to do) at 4 steps and half at 10:
  mixed    one solve(n_timesteps=[10, 4, 10, 4, ...]) (mt_cfm_solve_rows: direct launches, rows gathered and scattered)
  uniform  one 10-step solve of the whole batch (the graph path): every row pays for the largest count
  split    two solves, the 10-step rows and the 4-step rows as batches of B / 2 (graph path; the halves gathered
           beforehand, outside the timing)
Interleaved rounds of `reps` back-to-back solves each; median, min and max of the per-solve time per variant. Also
prints the rows per evaluation and checks the mixed solve against the split one (rel-RMS per half).
Usage: python tools/mixed_steps_ab.py [B] [T] [rounds] [reps]"""
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "matcha-tts_amd"))
sys.path.insert(0, os.path.join(HERE, "tests"))
import torch  # noqa: E402

from conftest import make_decoder, rel_rms  # noqa: E402
from matcha_hip import runtime as rt  # noqa: E402
from matcha_hip import synthetic  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
T = int(sys.argv[2]) if len(sys.argv) > 2 else 728
R = int(sys.argv[3]) if len(sys.argv) > 3 else 9
K = int(sys.argv[4]) if len(sys.argv) > 4 else 3
N_HI, N_LO = 10, 4
dec = make_decoder(160, "bf16")
sd = synthetic.make_state_dict([(k, tuple(v.shape)) for k, v in dec.state_dict().items()], 7)
dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
dec = dec.cuda().eval()
eng = dec.engine()
packed = dec.packed(torch.device("cuda", 0))
g = torch.Generator().manual_seed(0)
lens = torch.randint(T // 3, T - 4, (B,), generator=g)
lens[0] = T - 4
mask = (torch.arange(T)[None] < lens[:, None]).float()[:, None].cuda()
mu = torch.randn(B, 80, T, generator=g).cuda() * mask
seeds = torch.arange(B, dtype=torch.int64).cuda() * 7919 - 3
mv = int(lens.max())
counts = [N_HI if b % 2 == 0 else N_LO for b in range(B)]
hi = torch.tensor([b for b in range(B) if counts[b] == N_HI]).cuda()
lo = torch.tensor([b for b in range(B) if counts[b] == N_LO]).cuda()
halves = [(n, idx, mu[idx].contiguous(), mask[idx].contiguous(), seeds[idx].contiguous())
          for n, idx in ((N_HI, hi), (N_LO, lo))]


def mixed():
    return eng.solve(packed, None, 0.667, mu, mask, None, counts, "euler", max_valid=mv, seeds=seeds)


def uniform():
    return eng.solve(packed, None, 0.667, mu, mask, None, N_HI, "euler", max_valid=mv, seeds=seeds)


def split():
    return [eng.solve(packed, None, 0.667, m_, k_, None, n, "euler", max_valid=mv, seeds=s_)
            for n, _, m_, k_, s_ in halves]


plan = rt.rows_plan(sorted(counts, reverse=True))
print(f"B={B} T={T}: rows per evaluation {plan}: {sum(plan)} row-evaluations, uniform {B * N_HI}", flush=True)
VARIANTS = (("mixed", mixed), ("uniform", uniform), ("split", split))
res = {n: [] for n, _ in VARIANTS}
for r in range(R + 1):  # round 0 warms every variant up (code objects, the graph captures)
    for name, fn in VARIANTS:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            fn()
        torch.cuda.synchronize()
        if r > 0:
            res[name].append((time.perf_counter() - t0) * 1e3 / K)
for name, _ in VARIANTS:
    v = sorted(res[name])
    print(f"cfm solve B={B} T={T} {name}: median {v[len(v) // 2]:.3f} ms min {v[0]:.3f} ms max {v[-1]:.3f} ms "
          f"({R} rounds x {K} solves)", flush=True)
a, parts = mixed(), split()
for (n, idx, _, _, _), p in zip(halves, parts):
    print(f"mixed vs split, the {n}-step rows: rel-RMS {rel_rms(a[idx].cpu(), p.cpu()):.3e}, "
          f"equal {torch.equal(a[idx], p)}")
