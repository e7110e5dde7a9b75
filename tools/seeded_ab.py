#!/usr/bin/env python3
"""In-process A/B of the seeded CFM solve against the unseeded one (DESIGN.md "Seeded noise"): the bf16 solve (10-step
Euler, graph path) at B x T, ragged like the bench (the longest utterance T - 4 frames), as CFM.forward issues it:
unseeded = torch.randn_like(mu) + solve(z_noise, out=z) (two transposes of the noise tensor), seeded = solve(seeds=...)
into a fresh output (one generator kernel). Interleaved rounds of `reps` back-to-back solves each; median, min and
max of the per-solve time per variant. Also checks the seeded solve equals the solve on rt.seeded_noise.
Usage: python tools/seeded_ab.py [B] [T] [rounds] [reps]"""
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "matcha-tts_amd"))
sys.path.insert(0, os.path.join(HERE, "tests"))
import torch  # noqa: E402

from conftest import make_decoder  # noqa: E402
from matcha_hip import runtime as rt  # noqa: E402
from matcha_hip import synthetic  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
T = int(sys.argv[2]) if len(sys.argv) > 2 else 728
R = int(sys.argv[3]) if len(sys.argv) > 3 else 9
K = int(sys.argv[4]) if len(sys.argv) > 4 else 5
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


def unseeded():
    z = torch.randn_like(mu)
    return eng.solve(packed, z, 0.667, mu, mask, None, 10, "euler", out=z, max_valid=mv)


def seeded():
    return eng.solve(packed, None, 0.667, mu, mask, None, 10, "euler", max_valid=mv, seeds=seeds)


VARIANTS = (("unseeded", unseeded), ("seeded", seeded))
res = {n: [] for n, _ in VARIANTS}
for r in range(R + 1):  # round 0 warms both up (code objects, the graph capture)
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
ref = eng.solve(packed, rt.seeded_noise(seeds, T), 0.667, mu, mask, None, 10, "euler", max_valid=mv)
print("seeded solve equals the solve on seeded_noise:", torch.equal(seeded(), ref))
