"""Programme loudness (ITU-R BS.1770) and true peak of one utterance on the CPU (numpy only, no GPU): the
specification the HIP kernels of csrc/mt_loudness.hip are tested against. Arithmetic is fp64 on the
fp32 samples unless stated otherwise; `fs` is the rate of the measured signal.

* ``k_weighting(fs)``: the two biquads of the K-weighting for any fs >= 8000, by the bilinear transform of the
  analogue prototypes behind the standard's 48 kHz table (which they reproduce to 8.9e-16).
* ``biquad_ref`` / ``k_filter_ref``: transposed direct form II from a zero state; the cascade's state is the 4 values
  the kernel's chunked scan carries.
* ``block_energies(x, fs)``: z_j, the mean square of the K-weighted signal over 400 ms blocks at 100 ms hops.
* ``gate_ref(z)``: absolute and relative gating in the energy domain, sums in block order, one IEEE operation at a
  time -> E; ``lufs(E)`` = -0.691 + 10 log10 E (reporting only).
* ``true_peak_ref(x)``: max of |x| and of the 4x oversampled signal, the resampler's own fp32 FMA chain.
* ``loudness_gain_ref``: the gain to a target loudness under a true-peak ceiling, worded through
  ``audio_out.gain_ref``.
"""
from __future__ import annotations

import math

import numpy as np

from . import audio_out

MIN_RATE = 8000
ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)  # -70 LUFS as a mean square of the K-weighted signal
REL_GATE = 0.1                               # -10 LU under the mean of the blocks past the absolute gate
SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196)  # f0 Hz, G dB, Q
SHELF_VB_EXP = 0.4996667741545416
HIGHPASS = (38.13547087602444, 0.5003270373238773)                   # f0 Hz, Q


def hop_of(fs: int) -> int:
    """samples per 100 ms hop; a block is four hops"""
    return (int(fs) + 5) // 10


def k_weighting(fs: int):
    """-> (b1, a1, b2, a2), each fp64 [3] with a[0] = 1: stage 1 (high shelf), stage 2 (high-pass)"""
    fs = int(fs)
    if fs < MIN_RATE:
        raise ValueError(f"k_weighting: sample rate {fs} below {MIN_RATE} Hz")
    f0, G, Q = SHELF
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** SHELF_VB_EXP
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = HIGHPASS
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return b1, a1, b2, a2


def coefficients(fs: int) -> np.ndarray:
    """the 10 doubles mt_loudness takes: b1[0..2], a1[1..2], b2[0..2], a2[1..2]"""
    b1, a1, b2, a2 = k_weighting(fs)
    return np.concatenate([b1, a1[1:], b2, a2[1:]])


def biquad_ref(b, a, x) -> np.ndarray:
    """one biquad, transposed direct form II from a zero state: y = s0 + b0 x; s0 = s1 + b1 x - a1 y;
    s1 = b2 x - a2 y (the order scipy.signal.lfilter evaluates them in)"""
    b0, b1, b2 = (float(v) for v in b)
    a1, a2 = float(a[1]), float(a[2])
    xs = np.asarray(x, dtype=np.float64).reshape(-1).tolist()
    y = [0.0] * len(xs)
    s0 = s1 = 0.0
    for i, v in enumerate(xs):
        o = b0 * v + s0
        s0 = s1 + b1 * v - a1 * o
        s1 = b2 * v - a2 * o
        y[i] = o
    return np.array(y, dtype=np.float64)


def k_filter_ref(x, fs: int) -> np.ndarray:
    b1, a1, b2, a2 = k_weighting(fs)
    return biquad_ref(b2, a2, biquad_ref(b1, a1, x))


def block_count(n: int, fs: int) -> int:
    n, h = int(n), hop_of(fs)
    if n <= 0:
        return 0
    return (n - 4 * h) // h + 1 if n >= 4 * h else 1


def block_energies(x, fs: int) -> np.ndarray:
    """z fp64 [J]: n >= 4h: J = (n - 4h) // h + 1 blocks of 4h samples at hops of h (what follows the last complete
    block is not measured); 0 < n < 4h: the whole utterance is one block, z_0 = sum y^2 / n; n = 0: none."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n, h = x.shape[0], hop_of(fs)
    J = block_count(n, fs)
    if J == 0:
        return np.zeros(0, dtype=np.float64)
    y2 = k_filter_ref(x, fs) ** 2
    if n < 4 * h:
        return np.array([y2.sum() / n])
    return np.array([y2[j * h:j * h + 4 * h].sum() / (4 * h) for j in range(J)])


def gate_ref(z) -> float:
    """E: the mean of the blocks past both gates (0 when none passes the absolute gate). Plain fp64 adds in block
    order, one multiplication and two divisions: what loudness_gate_kernel does, operation for operation."""
    z = [float(v) for v in np.asarray(z, dtype=np.float64).reshape(-1)]
    s, c = 0.0, 0
    for v in z:
        if v > ABS_GATE:
            s, c = s + v, c + 1
    if c == 0:
        return 0.0
    rel = REL_GATE * (s / float(c))
    s, c = 0.0, 0
    for v in z:
        if v > ABS_GATE and v > rel:
            s, c = s + v, c + 1
    return s / float(c) if c else 0.0


def gate_counts(z):
    """(blocks, past the absolute gate, past both gates)"""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    m1 = z > ABS_GATE
    if not m1.any():
        return z.shape[0], 0, 0
    m2 = m1 & (z > REL_GATE * z[m1].mean())
    return z.shape[0], int(m1.sum()), int(m2.sum())


def loudness_ref(x, fs: int):
    """-> (E, z)"""
    z = block_energies(x, fs)
    return gate_ref(z), z


def lufs(E) -> float:
    E = float(E)
    return -0.691 + 10.0 * math.log10(E) if E > 0.0 else -math.inf


def _fma32(a, b, c) -> np.ndarray:
    """fp32 fma(a, b, c) with its single rounding: the product is exact in fp64, the fp64 sum is made odd where it is
    inexact (round to odd), and rounding that to fp32 then equals rounding the exact value"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)  # TwoSum: p + c = s + e exactly
    even = (s.view(np.int64) & 1) == 0
    s = np.where((e != 0.0) & even, np.nextafter(s, np.where(e > 0.0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def oversample4_ref(x, zeros: int = 10, beta: float = 5.0) -> np.ndarray:
    """r fp32 [4n]: audio_out.resample_ref's sum at up = 4, down = 1 with the fp32-rounded taps of
    design_filter(4, 1, zeros, beta), evaluated as resample_kernel does: one fp32 FMA chain from 0 over q = 0 .. Q-1"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = x.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    h, half = audio_out.design_filter(4, 1, zeros, beta)
    P = audio_out.polyphase(h.astype(np.float32), half, 4)
    c = half + np.arange(4 * n, dtype=np.int64)
    acc = np.zeros(4 * n, dtype=np.float32)
    for q in range(P.shape[1]):
        k = c // 4 - q
        xg = np.where((k >= 0) & (k < n), x[np.clip(k, 0, n - 1)], np.float32(0.0)).astype(np.float32)
        acc = _fma32(P[c % 4, q], xg, acc)
    return acc


def true_peak_ref(x, zeros: int = 10, beta: float = 5.0) -> np.float32:
    """TP = max(max |x|, max |r|), fp32 (0 for an empty utterance)"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    if x.shape[0] == 0:
        return np.float32(0.0)
    return np.float32(max(np.abs(x).max(), np.abs(oversample4_ref(x, zeros, beta)).max()))


def target_level(target_lufs: float) -> float:
    """the RMS of the K-weighted signal at a loudness of target_lufs"""
    return math.sqrt(10.0 ** ((float(target_lufs) + 0.691) / 10.0))


def effective_peak(TP, E, ceiling_dbtp: float) -> np.float32:
    """peak_eff = float32(float64(TP) / c), c = 10^(ceiling / 20): gain_ref's 1 / peak cap then is c / TP. 0 for a
    row with E == 0 (silent, empty or below the absolute gate), which keeps gain 1."""
    if not float(E) > 0.0:
        return np.float32(0.0)
    return np.float32(float(np.float32(TP)) / 10.0 ** (float(ceiling_dbtp) / 20.0))


def loudness_gain_ref(E, TP, target_lufs: float, ceiling_dbtp: float = -1.0, limit: bool = True) -> np.float32:
    """level / sqrt(E), with limit at most c / TP; 1 when E == 0 or TP == 0. fp64, rounded to fp32 at the end."""
    return audio_out.gain_ref(effective_peak(TP, E, ceiling_dbtp), E, "rms", target_level(target_lufs), limit)
