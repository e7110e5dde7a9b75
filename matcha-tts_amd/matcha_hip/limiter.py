"""Look-ahead true-peak limiter of one utterance on the CPU (numpy only, no GPU): the specification the HIP kernels of
csrc/mt_limiter.hip are tested against, bit for bit. `x` is one row, fp32 [n]; c32 =
float32(10^(ceiling / 20)).

* ``envelope_ref(x)``: p[i], the largest magnitude the waveform reaches around sample i: |x[i]| and the 4x oversampled
  signal (loudness.oversample4_ref, the true-peak meter's own FMA chain) three outputs to each side of it.
* ``window_samples(fs, window_ms)``: the smoothing window W in samples, 1 .. MAX_WINDOW.
* ``gain_curve_ref(p, g0, c32, W)``: s[i] <= 1, the gain reduction: the quotient c32 / (g0 p) where the levelled
  envelope passes the ceiling, as an integer of 30 fractional bits; the minimum over W samples ahead; the mean of W
  such minima. Integer minimum and integer sum: exact in any order.
* ``apply_ref(x, g0, s)``: y = fl32(fl32(g0 x) s), two products rounded one after the other.
* ``limiter_ref``: the make-up passes: the gain g rises until the limited signal reads the target loudness, then one
  static trim holds what the smoothing let through of the true peak, with the headroom (trim_headroom) that the fp32
  arithmetic of delivery and meter needs, so that the meter reads the delivered signal at or under the ceiling.
* ``fixed_gain_ref`` / ``limit_fixed_ref``: the limiter at a gain fixed beforehand, in one pass, with nothing measured,
  made up or trimmed; ``envelope_reach``: how far ahead the envelope reads. What a stream delivers chunk by chunk
  (the ranges are stream_plan's).
"""
from __future__ import annotations

import math

import numpy as np

from . import audio_out
from . import loudness as ld

MAX_WINDOW = 2048           # samples (mt_limiter.hip LM_MAX_W)
MAX_PASSES = 8
ONE = 1 << 30               # gain 1 in the curve's fixed point
REACH = 3                   # 4x outputs on each side of a sample that count against it


def envelope_ref(x, zeros: int = 10, beta: float = 5.0) -> np.ndarray:
    """p fp32 [n]: p[i] = max(|x[i]|, max |r[m]|, 4i - 3 <= m <= 4i + 3 inside [0, 4n)), r = oversample4_ref(x): the
    three outputs between two samples count against both of them, because an inter-sample peak is shaped by the gains
    of both. The maximum is the kernel's: it starts at 0 and folds every value in with fmaxf, which returns the other
    operand when one is a NaN, so a NaN (a NaN sample, and the outputs whose taps reach it) counts as absent and p is
    never a NaN; an infinite sample gives inf."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = x.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.abs(ld.oversample4_ref(x, zeros, beta))
    p = np.fmax(np.float32(0.0), np.abs(x))
    m0 = 4 * np.arange(n, dtype=np.int64)
    for d in range(-REACH, REACH + 1):
        m = m0 + d
        ok = (m >= 0) & (m < 4 * n)
        p = np.where(ok, np.fmax(p, r[np.clip(m, 0, 4 * n - 1)]), p)
    return p.astype(np.float32)


def window_samples(fs: int, window_ms: float) -> int:
    """W = max(1, rint(window_ms fs / 1000)); ValueError outside 1 .. MAX_WINDOW or for a window that is not finite
    and positive"""
    window_ms = float(window_ms)
    if not (math.isfinite(window_ms) and window_ms > 0.0):
        raise ValueError(f"limiter: the window must be finite and positive, got {window_ms} ms")
    W = max(1, int(np.rint(window_ms * int(fs) / 1000.0)))
    if W > MAX_WINDOW:
        raise ValueError(f"limiter: {window_ms} ms at {fs} Hz is a window of {W} samples; at most {MAX_WINDOW}")
    return W


def _check_window(W: int) -> int:
    W = int(W)
    if not 1 <= W <= MAX_WINDOW:
        raise ValueError(f"limiter: window of {W} samples outside 1 .. {MAX_WINDOW}")
    return W


def quotient_ref(p, g0, c32) -> np.ndarray:
    """r fp32 [n]: with a = fl32(g0 p[i]), the fp32 IEEE quotient c32 / a where a > c32, else 1. A NaN is not over the
    ceiling; a = inf gives 0."""
    p = np.asarray(p, dtype=np.float32).reshape(-1)
    c32 = np.float32(c32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        a = (np.float32(g0) * p).astype(np.float32)
        over = a > c32
        r = np.where(over, c32 / np.where(over, a, np.float32(1.0)), np.float32(1.0))
    return r.astype(np.float32)


def gain_curve_ref(p, g0, c32, W: int) -> np.ndarray:
    """s fp32 [n]. q[i] = floor(r[i] 2^30) (exact: r is fp32 in [0, 1]); q = 2^30 outside [0, n);
    m[j] = min q[j .. j + W - 1]; S[i] = sum_{k < W} m[i - k] (an integer under 2^41);
    s[i] = float32(float64(S[i]) / float64(W 2^30)). Every window of the sum holds i, so S / (W 2^30) <= q[i] / 2^30
    <= r[i], and both roundings are monotone with r[i] an fp32 value: s[i] <= r[i] exactly."""
    W = _check_window(W)
    r = quotient_ref(p, g0, c32)
    n = r.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    q = np.floor(r.astype(np.float64) * float(ONE)).astype(np.int64)
    ext = np.full(n + 2 * (W - 1), ONE, dtype=np.int64)
    ext[W - 1:W - 1 + n] = q
    m = np.lib.stride_tricks.sliding_window_view(ext, W).min(axis=1)  # [n + W - 1]: m[j], j = -(W - 1) .. n - 1
    P = np.concatenate([[0], np.cumsum(m)])
    S = P[W:W + n] - P[:n]                                            # sum of m[i - W + 1 .. i]
    return (S.astype(np.float64) / float(W * ONE)).astype(np.float32)


def apply_ref(x, g0, s) -> np.ndarray:
    """y[i] = fl32(fl32(g0 x[i]) s[i]): two separately rounded fp32 products, never one fused"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = (np.float32(g0) * x).astype(np.float32)
        return (t * np.asarray(s, dtype=np.float32)).astype(np.float32)


def envelope_reach(half4: int) -> int:
    """The samples after i that p[i] reads, with a 4x filter of 2 half4 + 1 taps: the chain of the 4x output 4i + 3
    starts at the sample (half4 + 4i + 3) // 4 = i + (half4 + 3) // 4 (10 for the default filter, half4 = 40)."""
    half4 = int(half4)
    if half4 < 0:
        raise ValueError(f"envelope_reach: half-length {half4}")
    return (half4 + 3) // 4


def fixed_gain_ref(gain_db) -> np.float32:
    """float32(10^(float64(gain_db) / 20)): a gain chosen beforehand, in dB; ValueError unless finite"""
    gain_db = float(gain_db)
    if not math.isfinite(gain_db):
        raise ValueError(f"limiter: gain_db must be finite, got {gain_db}")
    with np.errstate(over="ignore"):
        return np.float32(10.0 ** (np.float64(gain_db) / 20.0))


def limit_fixed_ref(x, gain_db, ceiling_dbtp: float, W: int, zeros: int = 10, beta: float = 5.0):
    """-> (y fp32 [n], reduction): the limiter at a fixed gain g = fixed_gain_ref(gain_db), one pass: s =
    gain_curve_ref(envelope_ref(x), g, c32, W), y = apply_ref(x, g, s), reduction = min s (1 for an empty row). No
    loudness is measured, nothing is made up or trimmed, and there is no "levelled at all" test: a silent row is
    g * 0. Every part of it is local (envelope_reach samples ahead for p, W - 1 more for s), so a stream can
    deliver it chunk by chunk."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    g = fixed_gain_ref(gain_db)
    c32 = np.float32(10.0 ** (float(ceiling_dbtp) / 20.0))
    s = gain_curve_ref(envelope_ref(x, zeros, beta), g, c32, W)
    return apply_ref(x, g, s), (s.min() if s.shape[0] else np.float32(1.0))


def next_gain_ref(g, level: float, E) -> np.float32:
    """g_{k+1} = float32(float64(g_k) level / sqrt(E_k)); unchanged when E_k == 0"""
    if not float(E) > 0.0:
        return np.float32(g)
    return np.float32(float(np.float32(g)) * float(level) / math.sqrt(float(E)))


def trim_headroom(P) -> float:
    """eps: what the fp32 arithmetic between the trim and the meter can add to the delivered true peak, relative.
    P: the fp32 taps by phase of the 4x filter, [4][Q]. With u = 2^-24, A = max_p sum_q |P[p][q]| and t = trim: a
    delivered sample is fl32(t y) = t y (1 + d), |d| <= u; a 4x output of it is a chain of Q FMAs, sum h x' (1 + th),
    |th| <= Q u, and TP' was read from such a chain on y itself. Their difference is at most t A max|y| (2 Q + 1) u
    and max|y| <= TP', so the meter reads at most t TP' (1 + A (2 Q + 1) u) on the delivered signal. The trim is
    fl32(1 / fl32(TP' (1 + eps) / c)), two roundings more. eps = (2 (Q + 2) A + 4) u covers all of it with room for
    the second-order terms (6.4e-6, 5.5e-5 dB, at the default filter)."""
    P = np.asarray(P, dtype=np.float64)
    return (2.0 * (P.shape[1] + 2) * float(np.abs(P).sum(axis=1).max()) + 4.0) * 2.0 ** -24


def default_headroom(zeros: int = 10, beta: float = 5.0) -> float:
    h, half = audio_out.design_filter(4, 1, zeros, beta)
    return trim_headroom(audio_out.polyphase(h.astype(np.float32), half, 4))


def trim_peak_ref(TP, E, ceiling_dbtp: float, eps: float) -> np.float32:
    """float32(float64(TP') / c (1 + eps)), the peak over the ceiling with the headroom; 0 for a row that was not
    levelled (E == 0)"""
    if not float(E) > 0.0:
        return np.float32(0.0)
    return np.float32(float(np.float32(TP)) / 10.0 ** (float(ceiling_dbtp) / 20.0) * (1.0 + float(eps)))


def trim_ref(TP, E, ceiling_dbtp: float, eps: float) -> np.float32:
    """min(1, 1 / trim_peak_ref) of the limited signal, through gain_ref's limit: 1 for a row that was not levelled.
    TP' trim <= c (1 - eps + 2^-23) < c, and the delivered signal's true peak, as the meter reads it, is under c."""
    return audio_out.gain_ref(trim_peak_ref(TP, E, ceiling_dbtp, eps), 1.0, "rms", 1.0, True)


def limiter_ref(x, fs: int, target: float, ceiling: float, W: int, passes: int = 3, zeros: int = 10,
                beta: float = 5.0, trace=None):
    """-> (y fp32 [n], g, reduction, trim). E, TP as DESIGN §21 measures them; g_0 = the uncapped gain to the target;
    pass k: y_k = apply(x, g_k, gain_curve(p, g_k)), E_k = the gated energy of y_k, g_{k+1} = next_gain_ref; after the
    last pass trim = min(1, c / ((1 + eps) true_peak(y))), eps = trim_headroom of the filter. Returns the last pass' y and g, reduction = min s of it (1 for an empty
    row). The delivered signal is clamp(trim y). A silent, empty or fully gated row (E == 0): y = x, g = 1, s = 1,
    trim = 1. trace: a list that receives (g_k, E_k) per pass."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    W = _check_window(W)
    passes = int(passes)
    if not 1 <= passes <= MAX_PASSES:
        raise ValueError(f"limiter: {passes} passes outside 1 .. {MAX_PASSES}")
    one = np.float32(1.0)
    E, _ = ld.loudness_ref(x, fs)
    if not E > 0.0:
        return x.copy(), one, one, one
    TP = ld.true_peak_ref(x, zeros, beta)
    level = ld.target_level(target)
    c32 = np.float32(10.0 ** (float(ceiling) / 20.0))
    p = envelope_ref(x, zeros, beta)
    g = audio_out.gain_ref(ld.effective_peak(TP, E, ceiling), E, "rms", level, limit=False)
    for k in range(passes):
        s = gain_curve_ref(p, g, c32, W)
        y = apply_ref(x, g, s)
        if trace is not None or k + 1 < passes:
            Ek, _ = ld.loudness_ref(y, fs)
            if trace is not None:
                trace.append((g, Ek))
        if k + 1 < passes:
            g = next_gain_ref(g, level, Ek)
    trim = trim_ref(ld.true_peak_ref(y, zeros, beta), E, ceiling, default_headroom(zeros, beta))
    return y, g, s.min(), trim
