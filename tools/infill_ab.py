#!/usr/bin/env python3
"""In-process A/B of mel infill's cost in the CFM solve: the bf16 Euler solve alone at the bench's
headline shape (B = 32, T = 728, ragged like the bench: the longest utterance T - 4 frames), 10 steps on a shared
explicit grid so that both variants take the rows path (mt_cfm_solve_rows / mt_cfm_solve_infill: direct launches):
  plain    solve(t_span=linspace(0, 1, 11))
  infill   the same with the first half of each utterance's valid frames kept (x1 = randn)
Interleaved rounds of `reps` back-to-back solves each, timed with device events; median, min and max of the per-solve
time per variant. infill adds 11 launches of infill_clamp_kernel (one before evaluation 0, one per evaluation), one
device-to-device copy (z0) and one transpose (x1); per evaluation the kernel moves at most B T 80 (4 + 4 + 4 + 2)
bytes (z0 and x1 read, the master and the bf16 input slot written). Writes profiles/infill_ab.json.
Usage: python tools/infill_ab.py [B] [T] [rounds] [reps]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "matcha-tts_amd"))
sys.path.insert(0, os.path.join(HERE, "tests"))
import torch  # noqa: E402

from conftest import make_decoder  # noqa: E402
from matcha_hip import synthetic  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
T = int(sys.argv[2]) if len(sys.argv) > 2 else 728
R = int(sys.argv[3]) if len(sys.argv) > 3 else 9
K = int(sys.argv[4]) if len(sys.argv) > 4 else 3
N = 10
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
x1 = torch.randn(B, 80, T, generator=g).cuda()
keep = (torch.arange(T)[None] < (lens // 2)[:, None]).cuda()
seeds = torch.arange(B, dtype=torch.int64).cuda() * 7919 - 3
mv = int(lens.max())
grid = torch.linspace(0, 1, N + 1)


def plain():
    return eng.solve(packed, None, 0.667, mu, mask, None, None, "euler", max_valid=mv, seeds=seeds, t_span=grid)


def infill():
    return eng.solve(packed, None, 0.667, mu, mask, None, None, "euler", max_valid=mv, seeds=seeds, t_span=grid,
                     x1=x1, keep=keep)


VARIANTS = (("plain", plain), ("infill", infill))
res = {n: [] for n, _ in VARIANTS}
for r in range(R + 1):  # round 0 warms both variants up (code objects, the workspace)
    for name, fn in VARIANTS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(K):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if r > 0:
            res[name].append(e0.elapsed_time(e1) / K)
out = {"shape": {"B": B, "T": T, "steps": N, "solver": "euler", "dtype": "bf16", "kept": "first half of each utterance"},
       "rounds": R, "solves_per_round": K, "timer": "device events around the back-to-back solves of a round"}
for name, _ in VARIANTS:
    v = sorted(res[name])
    out[name + "_ms"] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "all": res[name]}
    print(f"cfm solve B={B} T={T} {name}: median {v[len(v) // 2]:.3f} ms min {v[0]:.3f} ms max {v[-1]:.3f} ms "
          f"({R} rounds x {K} solves)", flush=True)
extra = out["infill_ms"]["median"] - out["plain_ms"]["median"]
bound = B * T * 80 * (4 + 4 + 4 + 2)
out["extra_ms_per_solve"] = extra
out["extra_us_per_evaluation"] = extra * 1e3 / N  # the launch before evaluation 0 and the two set-up copies included
out["bytes_per_evaluation_bound"] = bound
out["us_per_evaluation_at_8TBps"] = bound / 8.0e12 * 1e6
a, p = infill(), plain()
kv = (keep[:, None, :] & (mask != 0)).expand_as(a)
out["kept_frames_are_x1"] = bool(torch.equal(a[kv], x1[kv]))
out["padded_frames_unchanged"] = bool(torch.equal(a[(mask == 0).expand_as(a)], p[(mask == 0).expand_as(a)]))
print(f"infill extra: {extra:.3f} ms per solve, {out['extra_us_per_evaluation']:.1f} us per evaluation; the kernel moves "
      f"at most {bound / 1e6:.1f} MB per evaluation ({out['us_per_evaluation_at_8TBps']:.1f} us at 8 TB/s); kept frames "
      f"are x1: {out['kept_frames_are_x1']}", flush=True)
os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
with open(os.path.join(HERE, "profiles", "infill_ab.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
