"""The window calculus of streaming delivery (numpy / pure Python, no GPU): the specification hifigan/stream.py and
csrc/mt_stream.hip run.

Everything after the mel is local: HiFi-GAN is a conv stack of finite support, the denoiser a 1024 / 256 STFT, the
resampler a FIR and the encoder pointwise. A stream therefore walks the mel in chunks of frames; each step vocodes a
WINDOW of the mel (the chunk plus a halo), keeps the part of the result no frame outside the window could have
changed (the CROP), and the later stages do the same on the stitched result of the stage before. The crops of a
stage partition the utterance, and every kept value is computed from exactly the inputs, in exactly the order, of
the one-shot call: the concatenated chunks of a row are, bit for bit, that row of the one-shot path.

* ``vocoder_reach(h)``: the mel frames on each side an output sample can depend on, by exact integer interval
  propagation from the waveform back to the mel through the config's layers (13 for hifigan.config.v1).
* ``denoise_reach()`` / ``denoise_window`` / ``denoise_final``: the STFT denoiser's window rule. The kernel
  transforms the frames (2j, 2j + 1) as one complex FFT, so a window starts on an even frame of the utterance and a
  sample is kept only when every frame covering it, and each such frame's partner, lies wholly inside the window.
* ``envelope_final`` / ``limit_final``: what of the limiter's envelope and of its output is final once so much of the
  stage before is (a fixed gain and the limiter in a stream).
* ``plan(lengths, chunk_frames, ...)``: per step and live row the vocoder window and crop, the denoise window and
  crop, and the output-sample range that becomes final.

Units: a *frame* is one mel frame = one hop of ``HOP`` = 256 samples = one STFT hop; the denoiser's STFT frame f
(n_fft 1024, center=True) covers the hop blocks f - 2 .. f + 1, and hop block j is the overlap-add of the STFT
frames j - 1 .. j + 2.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

HOP = 256
# hop blocks of context each side a kept hop block of the denoiser needs: 3 (STFT frames j - 1 .. j + 2, each two hop
# blocks to either side of its centre) plus one more where the pair alignment asks for it
DENOISE_CORE = 3


# ---------------------------------------------------------------------------------------------------------------
# vocoder
# ---------------------------------------------------------------------------------------------------------------

def _get(h, name):
    return h[name] if isinstance(h, dict) else getattr(h, name)


def _resblock_reach(kind: str, k: int, dilations: Sequence[int]) -> int:
    """samples on each side one ResBlock output depends on: ResBlock1 is, per dilation d, conv(k, d) then conv(k, 1)
    plus the identity; ResBlock2 conv(k, d) plus the identity; "same" padding d (k - 1) / 2"""
    k = int(k)
    if k % 2 != 1:
        raise ValueError(f"resblock kernel size {k}: the symmetric 'same' padding needs an odd size")
    r = (k - 1) // 2
    if str(kind) == "1":
        return sum(r * int(d) + r for d in dilations)
    return sum(r * int(d) for d in dilations)


def vocoder_interval(h, lo: int, hi: int):
    """The mel frames [lo', hi'] the output samples [lo, hi] (inclusive, any integers) depend on: the interval is
    carried from the waveform back to the mel through conv_post (k = 7), every stage's parallel ResBlocks (the widest
    of them), its transposed conv (output o = i u - p + j, j < k, p = (k - u) / 2, so i runs over
    ceil((o + p - k + 1) / u) .. floor((o + p) / u)) and conv_pre (k = 7)."""
    ur = [int(u) for u in _get(h, "upsample_rates")]
    uk = [int(k) for k in _get(h, "upsample_kernel_sizes")]
    rk = list(_get(h, "resblock_kernel_sizes"))
    rd = list(_get(h, "resblock_dilation_sizes"))
    kind = str(_get(h, "resblock"))
    if len(ur) != len(uk) or len(rk) != len(rd) or not ur or not rk:
        raise ValueError("vocoder_interval: inconsistent config")
    lo, hi = int(lo) - 3, int(hi) + 3
    rb = max(_resblock_reach(kind, k, d) for k, d in zip(rk, rd))
    for u, k in zip(reversed(ur), reversed(uk)):
        lo, hi = lo - rb, hi + rb
        p = (k - u) // 2
        lo, hi = -((-(lo + p - k + 1)) // u), (hi + p) // u
    return lo - 3, hi + 3


def vocoder_hop(h) -> int:
    return int(math.prod(int(u) for u in _get(h, "upsample_rates")))


def vocoder_reach(h) -> int:
    """The mel frames on each side that an output sample can depend on: the samples of frame 0 depend on the frames
    [-a, b] (``vocoder_interval``); every stride divides the hop, so the samples of frame t depend on [t - a, t + b]
    and the reach is max(a, b). A block of frames [s, e) vocoded from the window [s - reach, e + reach), or from a
    window that ends earlier at an end of the utterance itself, has the one-shot call's values."""
    lo, hi = vocoder_interval(h, 0, vocoder_hop(h) - 1)
    return max(-lo, hi)


def vocoder_reach_table(h):
    """The derivation, one row per layer group from the waveform back to the mel: (name, samples per mel frame at the
    layer's output, lo, hi) with [lo, hi] the positions at that layer's INPUT which the samples of mel frame 0
    depend on (DESIGN.md §20 prints it for v1)."""
    ur = [int(u) for u in _get(h, "upsample_rates")]
    uk = [int(k) for k in _get(h, "upsample_kernel_sizes")]
    kind = str(_get(h, "resblock"))
    rb = max(_resblock_reach(kind, k, d) for k, d in
             zip(_get(h, "resblock_kernel_sizes"), _get(h, "resblock_dilation_sizes")))
    rate = vocoder_hop(h)
    lo, hi = 0, rate - 1
    rows = [("waveform", rate, lo, hi)]
    lo, hi = lo - 3, hi + 3
    rows.append(("conv_post k=7", rate, lo, hi))
    for i in reversed(range(len(ur))):
        u, k = ur[i], uk[i]
        lo, hi = lo - rb, hi + rb
        rows.append((f"resblocks.{i} (+-{rb})", rate, lo, hi))
        p = (k - u) // 2
        lo, hi = -((-(lo + p - k + 1)) // u), (hi + p) // u
        rate //= u
        rows.append((f"ups.{i} u={u} k={k}", rate * u, lo, hi))
    lo, hi = lo - 3, hi + 3
    rows.append(("conv_pre k=7", 1, lo, hi))
    return rows


# ---------------------------------------------------------------------------------------------------------------
# denoiser
# ---------------------------------------------------------------------------------------------------------------

def denoise_reach() -> int:
    """Hop blocks of valid input a kept hop block of the denoiser needs on each side, at most: hop block j is the
    overlap-add of the STFT frames j - 1 .. j + 2; frame f reads the hop blocks f - 2 .. f + 1 and is transformed
    together with its partner f ^ 1. So block j reads the frames (j - 1) & ~1 .. (j + 2) | 1 and through them the hop
    blocks ((j - 1) & ~1) - 2 .. ((j + 2) | 1) + 1: j - 3 .. j + 3 for odd j and j - 4 .. j + 4 for even j. The
    answer is 4: ``DENOISE_CORE`` = 3 plus one for the pair alignment."""
    return DENOISE_CORE + 1


def denoise_final(end: int, n: int) -> int:
    """Hop blocks [0, result) of an utterance of n frames that are final once its first `end` hop blocks of input are:
    all of them when end == n; else block j needs (j + 2) | 1 <= end - 2 (its last STFT frame and that frame's
    partner read no sample at or past 256 end), which is j < (end - 3) & ~1."""
    end, n = int(end), int(n)
    if end >= n:
        return n
    return max(0, (end - 3) & ~1)


def denoise_window(done: int, end: int, n: int):
    """The window [start, end) of hop blocks to denoise so that the blocks [done, denoise_final(end, n)) come out
    with the one-shot call's bits, `done` being what earlier windows delivered: the start is the even frame at or
    below done - 3 (block `done` reads the STFT frames from (done - 1) & ~1 on, which read from two hop blocks before
    themselves; the pair (2j, 2j + 1) of the window must be a pair of the utterance), or the utterance's own start."""
    start = max(0, (int(done) - DENOISE_CORE) & ~1)
    check_denoise_window(start, end, n)
    return start, int(end)


def check_denoise_window(start: int, end: int, n: int) -> None:
    if start % 2:
        raise ValueError(f"denoise window [{start}, {end}) starts on an odd frame: the kernel transforms the frames "
                         "(2j, 2j + 1) of its input as one complex FFT, so the window's pairs must be the "
                         "utterance's pairs")
    if not (0 <= start <= end <= n):
        raise ValueError(f"denoise window [{start}, {end}) outside the utterance [0, {n})")


def denoise_keep(start: int, end: int, n: int):
    """The hop blocks [lo, hi) of the window [start, end) of an utterance of n frames whose values are the one-shot
    call's: from start + 3 on (from 0 when the window starts the utterance) up to ``denoise_final``."""
    check_denoise_window(start, end, n)
    lo = 0 if start == 0 else start + DENOISE_CORE
    hi = denoise_final(end, n)
    return (lo, hi) if hi > lo else (lo, lo)


# ---------------------------------------------------------------------------------------------------------------
# resampler
# ---------------------------------------------------------------------------------------------------------------

def out_length(n: int, up: int, down: int) -> int:
    return -((-int(n) * int(up)) // int(down))


def resample_final(avail: int, n: int, up: int, down: int, half: int) -> int:
    """Outputs [0, result) of an utterance of n samples that are final once its first `avail` samples are: all
    ceil(n up / down) when avail == n; else output m's chain reads the samples (half + m down) // up - q, q >= 0, so
    it needs half + m down < avail up."""
    if avail >= n:
        return out_length(n, up, down)
    x = int(avail) * int(up) - int(half)
    return max(0, -((-x) // int(down)))


def resample_last_read(m_hi: int, up: int, down: int, half: int) -> int:
    """the last input sample the outputs [0, m_hi) read (-1: none)"""
    return (int(half) + (int(m_hi) - 1) * int(down)) // int(up) if m_hi > 0 else -1


# ---------------------------------------------------------------------------------------------------------------
# fixed gain and limiter (matcha_hip/limiter.py is the specification of the two stages)
# ---------------------------------------------------------------------------------------------------------------

def envelope_final(avail: int, n: int, ereach: int) -> int:
    """Envelope samples [0, result) of a row of n samples that are final once its first `avail` samples are: all n
    when avail >= n; else p[i] reads the samples up to i + ereach (limiter.envelope_reach), so it needs
    i + ereach < avail."""
    avail, n = int(avail), int(n)
    if avail >= n:
        return n
    return max(0, avail - int(ereach))


def limit_final(avail_env: int, n: int, W: int) -> int:
    """Limited samples [0, result) of a row of n samples that are final once its first `avail_env` envelope samples
    are: all n when avail_env >= n; else s[i] reads the envelope up to i + W - 1 (the last of the W windows that
    hold i), so it needs i + W - 1 < avail_env."""
    avail_env, n = int(avail_env), int(n)
    if avail_env >= n:
        return n
    return max(0, avail_env - (int(W) - 1))


# ---------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------

@dataclass
class Windows:
    """One stage of one step: per live row its window [start, start + length) and the crop [crop_lo, crop_hi) that
    becomes final, in frames (hop blocks) of the utterance."""
    rows: List[int] = field(default_factory=list)
    start: List[int] = field(default_factory=list)
    length: List[int] = field(default_factory=list)
    crop_lo: List[int] = field(default_factory=list)
    crop_hi: List[int] = field(default_factory=list)

    def add(self, b, start, end, lo, hi):
        self.rows.append(b)
        self.start.append(start)
        self.length.append(end - start)
        self.crop_lo.append(lo)
        self.crop_hi.append(hi)

    def __len__(self):
        return len(self.rows)


@dataclass
class Step:
    index: int
    s: int                 # mel frames [s, e) of the shared schedule
    e: int
    voc: Windows
    den: Optional[Windows]
    m_lo: int              # outputs [m_lo, m_hi) of every row become final (clipped to the row's own count)
    m_hi: int
    raw_final: List[int]   # per row, after this step: frames of final vocoder output,
    den_final: List[int]   # frames of final denoised audio (= raw_final without a denoiser),
    out_final: List[int]   # final outputs
    # with a limiter (plan(env_reach=, window=)): [m_lo, m_hi) is the resampled range made final, not yet delivered;
    p_lo: Optional[int] = None   # the envelope samples [p_lo, p_hi) become final,
    p_hi: Optional[int] = None
    y_lo: Optional[int] = None   # and the limited samples [y_lo, y_hi) are delivered (each clipped to the row's count)
    y_hi: Optional[int] = None

    @property
    def delivered(self):
        """the range of outputs [lo, hi) this step delivers: [y_lo, y_hi) with a limiter, else [m_lo, m_hi)"""
        return (self.m_lo, self.m_hi) if self.y_hi is None else (self.y_lo, self.y_hi)

    def out_counts(self, n_out):
        """per row: (offset, valid samples, done) of the chunk this step delivers; done in the one step that
        delivers the row's last sample (the first step for an empty row)"""
        res = []
        lo, hi = self.delivered
        for n in n_out:
            off = min(lo, n)
            cnt = min(max(n - lo, 0), hi - lo)
            res.append((off, cnt, n <= hi and (cnt > 0 or (n == 0 and self.index == 0))))
        return res


@dataclass
class Plan:
    lengths: List[int]
    chunk_frames: int
    first_chunk_frames: int
    reach: int
    denoise: bool
    up: int
    down: int
    half: int
    n_out: List[int]
    steps: List[Step]
    env_reach: Optional[int] = None
    window: Optional[int] = None

    @property
    def max_vocoder_window(self) -> int:
        return max([max(st.voc.length, default=0) for st in self.steps] + [1])

    @property
    def max_denoise_window(self) -> int:
        return max([max(st.den.length, default=0) for st in self.steps if st.den is not None] + [1])

    @property
    def max_chunk(self) -> int:
        return max(st.delivered[1] - st.delivered[0] for st in self.steps)


def plan(lengths, chunk_frames: int, first_chunk_frames: Optional[int] = None, up: int = 1, down: int = 1,
         half: int = 0, *, reach: int, denoise: bool = True, hop: int = HOP, env_reach: Optional[int] = None,
         window: Optional[int] = None) -> Plan:
    """The steps of a stream over a batch of utterances of `lengths` mel frames.

    The mel-frame schedule [s_c, e_c) is shared by the batch: e_0 = first_chunk_frames (default chunk_frames),
    e_c = e_{c-1} + chunk_frames. Step c reads no mel frame at or past e_c + reach. Per row of n frames:
      vocoder   final frames V_c = n once e_c + reach >= n (the window then ends at the utterance's own end and the
                whole rest is exact), else e_c; window [max(0, V_{c-1} - reach), min(n, e_c + reach)), crop
                [V_{c-1}, V_c);
      denoiser  (optional) final hop blocks D_c = denoise_final(V_c, n); window denoise_window(D_{c-1}, V_c, n) of
                the stitched vocoder output, crop [D_{c-1}, D_c);
      output    final samples M_c = resample_final(hop D_c, hop n, up, down, half) of ceil(hop n up / down) (up =
                down = 1, half = 0: no rate change, M_c = hop D_c).
    A row is live in a stage while that stage has something left to make final for it and its crop is not empty. The
    range [m_lo, m_hi) a step delivers is shared by the batch, m_hi = the least M_c of the rows that are not complete
    (the greatest output count once all are); a row's chunk is that range clipped to its own output count, so the
    ranges of a row partition its outputs. The stream ends with the step in which every row is complete: the last
    step flushes. reach: ``vocoder_reach`` of the generator's config."""
    lens = [int(n) for n in lengths]
    chunk = int(chunk_frames)
    first = chunk if first_chunk_frames is None else int(first_chunk_frames)
    up, down, half, reach, hop = int(up), int(down), int(half), int(reach), int(hop)
    if min(lens, default=0) < 0:
        raise ValueError(f"plan: negative length in {lens}")
    if chunk < 1 or first < 1:
        raise ValueError(f"plan: chunk_frames {chunk} / first_chunk_frames {first} must be >= 1")
    if up < 1 or down < 1 or half < 0 or reach < 0 or math.gcd(up, down) != 1:
        raise ValueError(f"plan: factor {up}/{down} (coprime, positive), half {half}, reach {reach}")
    if (env_reach is None) != (window is None):
        raise ValueError("plan: env_reach and window come together (a limiter after the rate change) or not at all")
    limited = window is not None
    if limited:
        env_reach, window = int(env_reach), int(window)
        if env_reach < 0 or window < 1:
            raise ValueError(f"plan: env_reach {env_reach} (>= 0), window {window} (>= 1)")
    B = len(lens)
    n_out = [out_length(hop * n, up, down) for n in lens]
    V, D, M = [0] * B, [0] * B, [0] * B
    steps: List[Step] = []
    s, e, m_done, p_done, y_done = 0, first, 0, 0, 0
    while True:
        voc, den = Windows(), (Windows() if denoise else None)
        for b, n in enumerate(lens):
            if V[b] < n:
                v_new = n if e + reach >= n else e
                if v_new > V[b]:
                    voc.add(b, max(0, V[b] - reach), min(n, e + reach), V[b], v_new)
                    V[b] = v_new
            if denoise:
                if D[b] < n:
                    d_new = denoise_final(V[b], n)
                    if d_new > D[b]:
                        ws, we = denoise_window(D[b], V[b], n)
                        lo, hi = denoise_keep(ws, we, n)
                        assert lo <= D[b] and hi == d_new, (ws, we, n, lo, hi, D[b], d_new)
                        den.add(b, ws, we, D[b], d_new)
                        D[b] = d_new
            else:
                D[b] = V[b]
            M[b] = resample_final(hop * D[b], hop * n, up, down, half)
        open_rows = [M[b] for b in range(B) if D[b] < lens[b]]
        m_hi = max(min(open_rows) if open_rows else max(n_out, default=0), m_done)
        step = Step(len(steps), s, e, voc, den, m_done, m_hi, list(V), list(D), list(M))
        if limited:
            # an open row goes on past m_hi: envelope_final / limit_final of a row that has not ended
            p_hi = max(m_hi - env_reach, p_done) if open_rows else m_hi
            y_hi = max(p_hi - (window - 1), y_done) if open_rows else m_hi
            step.p_lo, step.p_hi, step.y_lo, step.y_hi = p_done, p_hi, y_done, y_hi
            p_done, y_done = p_hi, y_hi
        steps.append(step)
        m_done = m_hi
        if not open_rows:
            break
        s, e = e, e + chunk
    return Plan(lens, chunk, first, reach, bool(denoise), up, down, half, n_out, steps, env_reach, window)
