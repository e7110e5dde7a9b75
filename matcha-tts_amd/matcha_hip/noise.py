"""The seeded noise stream of ``MatchaTTS.synthesize(..., seeds=...)`` on the CPU (numpy only, no GPU).

The value at (seed, channel c, frame t) is a pure function of those three numbers ("Seeded noise"):

* Philox4x32-10, key ``(seed & 0xffffffff, seed >> 32)`` of the int64 seed's two's-complement uint64, counter
  ``(t, c // 4, 0, 0)``;
* each output word x gives the uniform ``u(x) = (2 * (x >> 9) + 1) * 2**-24`` (exact in fp32, inside (0, 1));
* channels ``4q, 4q + 1`` are ``r(u(x0)) * cos(2 pi u(x1))`` and ``r(u(x0)) * sin(2 pi u(x1))``, channels
  ``4q + 2, 4q + 3`` the same from ``x2, x3``, with ``r(u) = sqrt(-2 ln u)``.

``reference_noise`` is that specification in float64; the HIP kernel (csrc/mt_noise.hip) evaluates it in fp32.
"""
from __future__ import annotations

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)
_SH32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., Random123). counter: four uint32 words (arrays broadcast against each other),
    key: two -> the four output words, uint32 arrays of the broadcast shape."""
    c = [np.asarray(v).astype(np.uint64) & _MASK32 for v in counter]
    k = [np.asarray(v).astype(np.uint64) & _MASK32 for v in key]
    if len(c) != 4 or len(k) != 2:
        raise ValueError("philox4x32_10: counter has four words, key has two")
    c = list(np.broadcast_arrays(*c, *k)[:4])
    for r in range(10):
        if r:
            k = [(k[0] + np.uint64(PHILOX_W0)) & _MASK32, (k[1] + np.uint64(PHILOX_W1)) & _MASK32]
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> _SH32) ^ c[1] ^ k[0], p1 & _MASK32, (p0 >> _SH32) ^ c[3] ^ k[1], p0 & _MASK32]
    return tuple(v.astype(np.uint32) for v in c)


def seed_key(seed: int):
    """(low, high) 32-bit key words of an int64 seed taken as its two's-complement uint64"""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32


def reference_noise(seed: int, T: int, C: int = 80, dtype=np.float64) -> np.ndarray:
    """The stream of one seed at temperature 1 -> [C, T]. dtype float64 (default) is the specification; float32
    evaluates the same formula on the same counters in fp32, as an estimate of what fp32 arithmetic can hold."""
    if C % 4 != 0 or C <= 0 or T <= 0:
        raise ValueError(f"reference_noise: C {C} must be a positive multiple of 4, T {T} positive")
    ft = np.dtype(dtype).type
    t = np.arange(T, dtype=np.uint64)[None, :]
    q = np.arange(C // 4, dtype=np.uint64)[:, None]
    x = philox4x32_10((t, q, 0, 0), seed_key(seed))
    # 2 * (x >> 9) + 1 < 2**24: exact in fp32, and so is the scaling by a power of two
    u = [((2 * (w >> np.uint32(9)).astype(np.int64) + 1).astype(ft) * ft(2.0 ** -24)) for w in x]
    out = np.empty((C // 4, 4, T), dtype=ft)
    for j in (0, 1):
        r = np.sqrt(ft(-2.0) * np.log(u[2 * j]))
        a = ft(2.0 * np.pi) * u[2 * j + 1]
        out[:, 2 * j] = r * np.cos(a)
        out[:, 2 * j + 1] = r * np.sin(a)
    return out.reshape(C, T)
