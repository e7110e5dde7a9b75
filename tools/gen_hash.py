#!/usr/bin/env python3
"""Hash of the bf16 Generator's output on fixed synthetic weights and mel (B=5, T=200: every pair kernel walks
several tiles), for build-vs-build bit-identity checks (MT_LIB selects the library). PAIR sets the vocoder pair mode
(as tools/pair_probe.py) and MT_VPAIRK the pair-kernel mask (mt_vpair_set_kernels), so the hash can be taken on the
non-default pair paths too; the library's other env knobs (MT_VPAIR3, ...) apply as always.
Usage: [PAIR=0|2|4] [MT_VPAIRK=0] python tools/gen_hash.py"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "matcha-tts_amd"))
sys.path.insert(0, os.path.join(HERE, "tests"))
import torch  # noqa: E402

if os.environ.get("MT_LIB"):
    import matcha_hip._lib as _L  # noqa: E402
    _L.LIB_PATH = os.environ["MT_LIB"]
from conftest import make_generator  # noqa: E402
from matcha_hip import runtime as rt, synthetic  # noqa: E402

gen = make_generator("bf16")
sd = synthetic.make_state_dict([(k, tuple(v.shape)) for k, v in gen.state_dict().items()], 23)
gen.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
gen = gen.cuda().eval()
gen.remove_weight_norm()
if os.environ.get("PAIR"):
    gen.engine().set_pair(int(os.environ["PAIR"]))
if os.environ.get("MT_VPAIRK"):
    rt.set_vpair_kernels(int(os.environ["MT_VPAIRK"]))
mel = (torch.randn(5, 80, 200, generator=torch.Generator().manual_seed(9)) * 2 - 5).cuda()
with torch.inference_mode():
    a = gen(mel).float().cpu()
tag = " ".join(f"{k}={os.environ[k]}" for k in ("PAIR", "MT_VPAIRK", "MT_VPAIR3") if os.environ.get(k))
print("gen_hash", tag or "default", hashlib.sha256(a.numpy().tobytes()).hexdigest()[:16], float(a.abs().max()))
