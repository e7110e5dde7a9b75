"""Joining a batch of sentences into documents, on the CPU in numpy: the specification the HIP kernels of
csrc/mt_join.hip are tested against. Integers are exact (64-bit inside, int32 out); a sample of a
document is one fp32 product per covering segment and one fp32 sum per product, each rounded on its own.

A segment is a row of seg (fp32 [S][L]); of it only the samples [a_s, e_s) (its trim edges) are ever read. Document d
owns the segments doc_first[d] .. doc_first[d + 1] - 1, in that order (CSR).
"""
from __future__ import annotations

import numpy as np

LCAP_MAX = 1 << 30   # the longest document: mt_loudness' bound on a row
FADE_MAX = 1 << 14   # the longest fade in samples: (2 j + 1) fade stays inside int32


def edges_ref(x, n: int, thr: float, pad: int):
    """-> (start, end) of the row x[0 .. n): from `pad` samples before its first loud sample (|x| >= thr as fp32;
    NaN is not loud) to `pad` samples past its last one, inside [0, n]; (0, 0) when no sample is loud. Nothing at or
    past n is read."""
    if not (thr >= 0 and np.isfinite(thr)) or pad < 0:
        raise ValueError(f"edges_ref: thr {thr} (finite, >= 0), pad {pad} (>= 0)")
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = min(max(int(n), 0), x.shape[0])
    with np.errstate(invalid="ignore"):
        loud = np.flatnonzero(np.abs(x[:n]) >= np.float32(thr))
    if loud.size == 0:
        return 0, 0
    return max(int(loud[0]) - int(pad), 0), min(int(loud[-1]) + 1 + int(pad), n)


def _clamped(start, end, L: int):
    a = np.clip(np.asarray(start, dtype=np.int64), 0, L)
    e = np.minimum(np.maximum(np.asarray(end, dtype=np.int64), a), L)
    return a, e


def _ranges(doc_first, S: int):
    """[(lo, hi)] per document, clamped the way the kernels clamp the table"""
    df = np.asarray(doc_first, dtype=np.int64).reshape(-1)
    out = []
    for d in range(df.shape[0] - 1):
        lo = min(max(int(df[d]), 0), S)
        out.append((lo, min(max(int(df[d + 1]), lo), S)))
    return out


def plan_ref(doc_first, start, end, gap, head: int, tail: int, L: int, Lcap: int = LCAP_MAX):
    """-> (dst int32 [S], doc_len int32 [D], bad): where each segment's first kept sample lands in its document, and
    each document's length. len_s = e_s - a_s of the clamped edges; the gap after s is g_s = max(gap[s], -min(len_s //
    2, len_{s+1} // 2)) (ignored on a document's last segment); dst[first] = head, dst[s + 1] = dst[s] + len_s + g_s,
    doc_len[d] = dst[last] + len_last + tail, head + tail for a document without segments. bad = 1 when a doc_len
    exceeds Lcap; every output is then min(., Lcap) of its 64-bit value. dst of a segment no document owns is 0."""
    if head < 0 or tail < 0 or L <= 0 or not (1 <= Lcap <= LCAP_MAX):
        raise ValueError(f"plan_ref: head {head}, tail {tail} (>= 0), L {L} (> 0), Lcap {Lcap} (1..2^30)")
    a, e = _clamped(start, end, L)
    ln = e - a
    S = ln.shape[0]
    gap = np.asarray(gap, dtype=np.int64).reshape(-1)
    rng = _ranges(doc_first, S)
    dst = np.zeros(S, dtype=np.int64)
    doc_len = np.zeros(len(rng), dtype=np.int64)
    for d, (lo, hi) in enumerate(rng):
        pos = int(head)
        for s in range(lo, hi):
            dst[s] = pos
            pos += int(ln[s])
            if s + 1 < hi:
                pos += max(int(gap[s]), -min(int(ln[s]) // 2, int(ln[s + 1]) // 2))
        doc_len[d] = pos + int(tail)
    bad = int((doc_len > Lcap).any())
    return np.minimum(dst, Lcap).astype(np.int32), np.minimum(doc_len, Lcap).astype(np.int32), bad


def ramp(fade: int) -> np.ndarray:
    """fp32 [fade]: 0.5 - 0.5 cos(pi (j + 0.5) / fade), computed in fp64 and rounded once. ramp[i] + ramp[fade - 1 -
    i] = 1 before the rounding: a fade-out over a fade-in of the same length sums to gain 1."""
    fade = int(fade)
    if not (0 <= fade <= FADE_MAX):
        raise ValueError(f"ramp: fade {fade} outside 0..{FADE_MAX}")
    j = np.arange(fade, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (j + 0.5) / max(fade, 1))).astype(np.float32)


def weights_ref(n: int, fade: int, table: np.ndarray) -> np.ndarray:
    """fp32 [n]: the fade weights of a segment of n kept samples. F = min(fade, n // 2) samples fade in and F fade
    out, through table[((2 j + 1) fade) // (2 F)] (j itself when F == fade); 1 between them."""
    w = np.ones(n, dtype=np.float32)
    F = min(int(fade), n // 2)
    if F > 0:
        idx = ((2 * np.arange(F, dtype=np.int64) + 1) * int(fade)) // (2 * F)
        w[:F] = table[idx]
        w[n - F:] = table[idx][::-1]
    return w


def join_ref(seg, start, end, doc_first, dst, doc_len, fade: int, Ld: int | None = None) -> np.ndarray:
    """-> out fp32 [D][Ld] (Ld: max(doc_len, 1) unless given). out[d][i] starts from 0.0f and adds, in segment order,
    fl32(w x) of every segment of document d that covers i, one fp32 add each (a plan of plan_ref: at most two);
    zero where nothing covers it and from doc_len[d] on."""
    seg = np.asarray(seg, dtype=np.float32)
    S, L = seg.shape
    a, e = _clamped(start, end, L)
    dst = np.asarray(dst, dtype=np.int64).reshape(-1)
    doc_len = np.asarray(doc_len, dtype=np.int64).reshape(-1)
    rng = _ranges(doc_first, S)
    if Ld is None:
        Ld = max(int(doc_len.max()) if doc_len.size else 0, 1)
    table = ramp(fade)
    out = np.zeros((len(rng), Ld), dtype=np.float32)
    for d, (lo, hi) in enumerate(rng):
        n_d = min(max(int(doc_len[d]), 0), Ld)
        for s in range(lo, hi):
            n = int(e[s] - a[s])
            j0 = max(0, -int(dst[s]))
            j1 = min(n, n_d - int(dst[s]))
            if j1 <= j0:
                continue
            w = weights_ref(n, fade, table)[j0:j1]
            x = seg[s, a[s] + j0:a[s] + j1]
            i0 = int(dst[s]) + j0
            prod = (w * x).astype(np.float32)                      # one rounding
            out[d, i0:i0 + (j1 - j0)] = out[d, i0:i0 + (j1 - j0)] + prod   # and another
    return out
