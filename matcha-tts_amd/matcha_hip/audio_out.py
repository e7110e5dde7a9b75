"""The audio output stage on the CPU (numpy only, no GPU): the specification the HIP kernels of
csrc/mt_audio.hip are tested against.

* ``rates(src, dst)``: the rational factor ``up / down`` of a rate change, ``up = dst // g``, ``down = src // g``,
  ``g = gcd(src, dst)``; either above ``MAX_FACTOR`` is refused.
* ``design_filter``: the Kaiser-windowed sinc ``scipy.signal.resample_poly`` designs by default,
  ``firwin(2 * half + 1, 1 / max(up, down), window=("kaiser", beta)) * up``, without scipy.
* ``resample_ref``: ``y[m] = sum_k h[half + m * down - k * up] * x[k]`` in fp64, ``ceil(n * up / down)`` outputs:
  zero padding at both ends, zero phase, sample 0 stays at time 0.
* ``resample_range_ref``: a range of those outputs evaluated alone, the same sum per output (mt_resample_range, the
  streaming resampler of DESIGN.md §20).
* ``pcm16_ref`` / ``mulaw_ref``: 16-bit PCM (fp32 arithmetic, round half to even) and G.711 mu-law bytes.
* ``gain_ref``: the per-utterance gain of peak / RMS normalisation.
"""
from __future__ import annotations

import math

import numpy as np

MAX_FACTOR = 1024
ENCODINGS = ("f32", "pcm16", "mulaw")
NORMALIZE = (None, "peak", "rms")
MULAW_BIAS, MULAW_CLIP = 0x84, 32635


def rates(src: int, dst: int):
    """(up, down) of the rate change src -> dst"""
    src, dst = int(src), int(dst)
    if src <= 0 or dst <= 0:
        raise ValueError(f"sample rates must be positive, got {src} -> {dst}")
    g = math.gcd(src, dst)
    up, down = dst // g, src // g
    if up > MAX_FACTOR or down > MAX_FACTOR:
        raise ValueError(f"{src} -> {dst} Hz is the factor {up}/{down}: factors above {MAX_FACTOR} are not supported")
    return up, down


def out_length(n: int, up: int, down: int) -> int:
    return -((-int(n) * int(up)) // int(down))


def design_filter(up: int, down: int, zeros: int = 10, beta: float = 5.0):
    """-> (h fp64 [2 * half + 1], half): cutoff 1 / max(up, down) of the up-sampled Nyquist, `zeros` zero crossings
    of the sinc on each side, Kaiser(beta) window, DC gain up."""
    up, down, zeros = int(up), int(down), int(zeros)
    if up < 1 or down < 1 or zeros < 1:
        raise ValueError(f"design_filter: up {up}, down {down}, zeros {zeros} must be positive")
    big = max(up, down)
    half = zeros * big
    fc = 1.0 / big
    i = np.arange(2 * half + 1, dtype=np.float64)
    h = fc * np.sinc(fc * (i - half)) * np.kaiser(2 * half + 1, float(beta))
    h *= up / h.sum()
    return h, half


def polyphase(h: np.ndarray, half: int, up: int) -> np.ndarray:
    """The taps by phase: P[p][q] = h[q * up + p], [up][ceil((2 * half + 1) / up)], zero-filled; output m then is
    sum_q P[(half + m * down) % up][q] * x[(half + m * down) // up - q]."""
    n = 2 * int(half) + 1
    if h.shape != (n,):
        raise ValueError(f"polyphase: {h.shape} taps, expected ({n},)")
    q = -(-n // int(up))
    full = np.zeros(q * up, dtype=h.dtype)
    full[:n] = h
    return np.ascontiguousarray(full.reshape(q, up).T)


def resample_ref(x: np.ndarray, up: int, down: int, h: np.ndarray, half: int) -> np.ndarray:
    """x [n] -> y fp64 [ceil(n * up / down)], the defining sum evaluated in fp64"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.shape[0]
    n_out = out_length(n, up, down)
    if n_out == 0:
        return np.zeros(0, dtype=np.float64)
    P = polyphase(np.asarray(h, dtype=np.float64), half, up)
    c = half + np.arange(n_out, dtype=np.int64) * down
    k = (c // up)[:, None] - np.arange(P.shape[1], dtype=np.int64)[None, :]
    ok = (k >= 0) & (k < n)
    xg = np.where(ok, x[np.clip(k, 0, n - 1)], 0.0)
    return (P[c % up] * xg).sum(axis=1)


def resample_range_ref(x: np.ndarray, up: int, down: int, h: np.ndarray, half: int, m_lo: int, m_hi: int) -> np.ndarray:
    """The outputs [m_lo, min(m_hi, ceil(n up / down))) of ``resample_ref(x, ...)``, x [n], evaluated alone: the same
    sum per output, with phase and input span from the output's own index m (mt_resample_range's specification).
    It reads no sample of x past (half + (m_hi - 1) down) // up, so those may still be unwritten (NaN)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.shape[0]
    m_lo, m_hi = max(int(m_lo), 0), min(int(m_hi), out_length(n, up, down))
    if m_hi <= m_lo:
        return np.zeros(0, dtype=np.float64)
    P = polyphase(np.asarray(h, dtype=np.float64), half, up)
    c = half + np.arange(m_lo, m_hi, dtype=np.int64) * down
    k = (c // up)[:, None] - np.arange(P.shape[1], dtype=np.int64)[None, :]
    ok = (k >= 0) & (k < n)
    xg = np.where(ok, x[np.clip(k, 0, n - 1)], 0.0)
    return (P[c % up] * xg).sum(axis=1)


def pcm16_ref(x: np.ndarray, gain) -> np.ndarray:
    """int16 = rint(clamp(gain * x, -1, 1) * 32767), every step in fp32, round half to even"""
    v = np.float32(gain) * np.asarray(x, dtype=np.float32)
    v = np.minimum(np.maximum(v, np.float32(-1.0)), np.float32(1.0))
    return np.rint(v * np.float32(32767.0)).astype(np.int16)


def f32_ref(x: np.ndarray, gain) -> np.ndarray:
    v = np.float32(gain) * np.asarray(x, dtype=np.float32)
    return np.minimum(np.maximum(v, np.float32(-1.0)), np.float32(1.0))


def mulaw_ref(q: np.ndarray) -> np.ndarray:
    """G.711 mu-law of int16 samples -> uint8: magnitude clipped to 32635 plus the bias 0x84, the segment = the
    position of its highest set bit among bits 14..7, the four bits below that bit as mantissa, the sign bit set for
    negative samples, all eight bits inverted (silence is 0xFF)."""
    q = np.asarray(q, dtype=np.int16).astype(np.int32)
    sign = np.where(q < 0, 0x80, 0)
    mag = np.minimum(np.abs(q), MULAW_CLIP) + MULAW_BIAS
    seg = np.zeros_like(mag)
    for s in range(1, 8):
        seg = np.where(mag >= (1 << (s + 7)), s, seg)
    mant = (mag >> (seg + 3)) & 0xF
    return (~(sign | (seg << 4) | mant) & 0xFF).astype(np.uint8)


def mulaw_decode(u: np.ndarray) -> np.ndarray:
    """the G.711 expansion of mu-law bytes -> int16 (the centre of each code's interval)"""
    u = ~np.asarray(u, dtype=np.uint8).astype(np.int32) & 0xFF
    t = (((u & 0xF) << 3) + MULAW_BIAS) << ((u >> 4) & 7)
    return np.where(u & 0x80, MULAW_BIAS - t, t - MULAW_BIAS).astype(np.int16)


def gain_ref(peak, meansq, normalize, level, limit=True) -> np.float32:
    """The gain of one utterance from its peak = max |x| and meansq = mean x^2, fp64 rounded to fp32 at the end:
    None -> 1; "peak" -> level / peak; "rms" -> level / sqrt(meansq), with limit at most 1 / peak (no clipping).
    A silent or empty utterance (peak == 0) keeps gain 1."""
    if normalize not in NORMALIZE:
        raise ValueError(f"normalize must be one of {NORMALIZE}, got {normalize!r}")
    peak = float(peak)
    if normalize is None or not peak > 0.0:
        return np.float32(1.0)
    level = float(level)
    if normalize == "peak":
        g = level / peak
    else:
        g = level / math.sqrt(float(meansq))
        if limit:
            g = min(g, 1.0 / peak)
    return np.float32(g)
