"""Streaming waveform delivery: the vocoder, the denoiser and the output stage chunk by chunk (DESIGN.md §20;
matcha_hip/stream_plan.py is the specification of the windows). No counterpart module in the reference.

    s = WaveStreamer(generator, denoiser, AudioOutput(8000, encoding="mulaw"), chunk_frames=32, first_chunk_frames=8)
    for ch in s(mel, lengths):            # mel [B,80,T] on the GPU, lengths int [B]
        ch.audio[b, :ch.lengths[b]]       # the next samples of row b, in the output encoding

For every row b the concatenation of ``ch.audio[b, :ch.lengths[b]]`` over the chunks is, bit for bit, the first
``out.lengths[b]`` elements of the one-shot

    AudioOutput(...)(Denoiser(...)(Generator(...)(mel, lengths).squeeze(1), strength, lengths), lengths).audio[b]

(of the shorter chains when `denoiser` and / or `output` is None): the stream runs the same ragged kernels on windows
of the utterance and keeps only the values no sample outside the window could have changed.

Where a chunk ends: the mel is walked in steps of `chunk_frames` frames (the first step `first_chunk_frames`), step c
ending at frame e_c. The step makes final, for every row that goes on past e_c + reach (reach =
``Generator.receptive_field()``, 13 frames for v1): the vocoder's samples up to frame e_c; with a denoiser, the
denoised samples up to frame D_c = (e_c - 3) & ~1 (the STFT's overlap and its frame pairs, ``denoise_final``); and the
output samples up to ceil((256 D_c up - half) / down) for a rate change by up / down with a filter of 2 half + 1 taps
(``resample_final``; 256 D_c without one). The chunk is that range of outputs, shared by the batch and clipped to
each row's own length, so early chunks of a stream with small steps can be empty. A row that ends within reach of
e_c is vocoded to its end at once; what it has beyond the shared range comes with the following chunks. The last step
flushes every row.

Causality: step c reads no mel frame at or past e_c + reach, and the mel is read in place when it is a contiguous
fp32 tensor: a caller may fill it in as the stream advances (``WaveStreamer.schedule`` gives the e_c).

The loop does not synchronise with the host: `lengths` is fetched once at the start, the tables of all steps are
uploaded once, and each step enqueues a fixed chain for the whole batch: gather -> mt_vocoder_forward_ragged ->
scatter -> gather -> mt_denoise_ragged -> scatter -> mt_resample_range -> mt_audio_encode. Not streamed: the CFM solve
(global over the utterance) and level normalisation (`normalize="peak"` / `"rms"` and `loudness=` need the whole
utterance).

Level in a stream: an output stage with a gain fixed beforehand, `AudioOutput(..., gain_db=6.0)`, and
with it the look-ahead limiter, `AudioOutput(..., gain_db=6.0, true_peak=-1.0, limiter=5.0)`, is streamed, again bit
for bit the one-shot call of the same stage; `s(mel, lengths, gain_db=[...])` sets the gain row by row. Once the gain
is known the limiter is local: the envelope of a sample reads `envelope_reach` = 10 samples ahead (the 4x filter)
and the gain curve W - 1 envelope samples ahead (W: the limiter's window in samples). The chain of a step then ends
... -> mt_resample_range (into a stitched buffer at the output rate) -> mt_peak_envelope_range (into a stitched
envelope) -> mt_limit_range -> mt_audio_encode, and a chunk ends `envelope_reach + W - 1` output samples before the
resampled range does: the added delay, 89 samples = 5.6 ms at 16 kHz with limiter=5.0 (W = 80). Without limiter= the
gain is one fp32 product on the delivered range and nothing is delayed. `WaveStreamer.reduction` holds the deepest
reduction of every row of the stream in progress.
"""
from __future__ import annotations

from typing import Iterator, List, NamedTuple, Optional

import torch

from matcha_hip import limiter as lm
from matcha_hip import runtime as rt
from matcha_hip import stream_plan as sp


class Chunk(NamedTuple):
    audio: torch.Tensor      # [B, n] in the output encoding (f32 / int16 / uint8); n may be 0
    lengths: torch.Tensor    # int32 [B]: valid samples of each row in this chunk
    offset: torch.Tensor     # int32 [B]: index of the chunk's first sample in the row's whole output
    done: torch.Tensor       # bool [B]: this chunk holds the row's last sample (set in exactly one chunk per row)


class WaveStreamer:
    """generator: a hifigan.models.Generator on the bf16 ragged path, or an fp32 one (the parity mode: the same plan
    with one vocoder call per window, slow). denoiser: a hifigan.denoiser.Denoiser or None, applied with `strength`.
    output: a hifigan.output.AudioOutput without level normalisation, or None (fp32 at the vocoder's rate, not
    clamped)."""

    def __init__(self, generator, denoiser=None, output=None, chunk_frames: int = 32,
                 first_chunk_frames: Optional[int] = None, strength: float = 0.00025, _halo: Optional[int] = None):
        if output is not None and output.normalize is not None:
            raise ValueError(f"WaveStreamer: normalize={output.normalize!r} takes its gain from the peak / RMS of the "
                             "whole utterance, which a stream has not seen when it delivers the first chunk; "
                             "normalise the level after the stream, or use normalize=None")
        if output is not None and getattr(output, "loudness", None) is not None:
            raise ValueError(f"WaveStreamer: loudness={output.loudness!r} takes its gain from the gated loudness and "
                             "the true peak of the whole utterance, which a stream has not seen when it delivers "
                             "the first chunk; level the loudness after the stream, or use loudness=None")
        eng = generator.engine()
        self.per_row = generator.precision in ("fp32", "float32", "f32")
        if not self.per_row and not eng.ragged_supported():
            raise ValueError("WaveStreamer: the vocoder engine has no ragged path in this mode "
                             "(mt_vocoder_ragged_supported); use the default bf16 path or fp32")
        if output is not None and output.hop != eng.hop:
            raise ValueError(f"WaveStreamer: output.hop {output.hop} != the vocoder's {eng.hop}")
        if eng.hop != sp.HOP and denoiser is not None:
            raise ValueError(f"WaveStreamer: the denoiser's hop is {sp.HOP}, the vocoder's {eng.hop}")
        self.generator, self.denoiser, self.output = generator, denoiser, output
        self.chunk_frames = int(chunk_frames)
        self.first_chunk_frames = self.chunk_frames if first_chunk_frames is None else int(first_chunk_frames)
        if self.chunk_frames < 1 or self.first_chunk_frames < 1:
            raise ValueError("WaveStreamer: chunk_frames and first_chunk_frames must be >= 1")
        self.strength = float(strength)
        self.hop = eng.hop
        self.reach = generator.receptive_field() if _halo is None else int(_halo)
        self.resample = output is not None and output.sample_rate != output.source_rate
        self.fixed_gain = output is not None and getattr(output, "gain_db", None) is not None
        self.limited = self.fixed_gain and output.limiter is not None
        # fp32 [B] on the device: min s of every row of the stream in progress (1: the limiter never worked); valid
        # for a row once its `done` chunk was yielded. None before the first stream and without limiter=.
        self.reduction: Optional[torch.Tensor] = None

    def _factor(self, device):
        if not self.resample:
            return None, 1, 1, 0
        o = self.output
        p = rt.resample_plan(o.source_rate, o.sample_rate, o.zeros, o.beta, device)
        return p, p.up, p.down, p.half

    def _plan4(self, device):
        """the 4x plan of the limiter's envelope at the output rate, or None"""
        if not self.limited:
            return None
        o = self.output
        return rt.resample_plan(o.sample_rate, 4 * o.sample_rate, o.zeros, o.beta, device)

    def _plan(self, lens, up, down, half, plan4) -> sp.Plan:
        lim = {} if plan4 is None else dict(env_reach=lm.envelope_reach(plan4.half),
                                            window=self.output.limiter_window)
        return sp.plan(lens, self.chunk_frames, self.first_chunk_frames, up, down, half, reach=self.reach,
                       denoise=self.denoiser is not None, hop=self.hop, **lim)

    def plan(self, lengths, device=None) -> sp.Plan:
        """the stream's steps for utterances of `lengths` mel frames (a sequence of ints)"""
        _, up, down, half = self._factor(device)
        return self._plan(lengths, up, down, half, self._plan4(device))

    def schedule(self, lengths, device=None) -> List[int]:
        """e_c of every step: the chunk of step c needs the mel frames below e_c + reach, and no others"""
        return [st.e for st in self.plan(lengths, device).steps]

    @staticmethod
    def _upload(cols, device) -> List[torch.Tensor]:
        """lists of ints -> views of ONE int32 tensor on the device (one copy), each from a 16-byte boundary"""
        flat, offs = [], []
        for c in cols:
            offs.append(len(flat))
            flat.extend(c)
            flat.extend([0] * (-len(flat) % 4))
        t = torch.tensor(flat or [0], dtype=torch.int32).pin_memory().to(device, non_blocking=True)
        return [t[o:o + len(c)] for o, c in zip(offs, cols)]

    def __call__(self, mel: torch.Tensor, lengths, gain_db=None) -> Iterator[Chunk]:
        """gain_db: per-row fixed gains in dB in place of the output stage's gain_db= (a sequence or CPU tensor of B
        finite floats; the stage must have been built with gain_db=)"""
        if gain_db is not None and not self.fixed_gain:
            raise ValueError("WaveStreamer: gain_db= overrides the output stage's fixed gain; the stage was built "
                             "without gain_db=")
        rt.require_gpu(mel, what="WaveStreamer")
        if mel.dim() != 3 or mel.shape[1] != 80:
            raise ValueError(f"WaveStreamer: mel {tuple(mel.shape)}, expected [B, 80, T]")
        B, _, T = mel.shape
        if B > rt.RAGGED_MAX_BATCH:
            raise ValueError(f"WaveStreamer: {B} utterances; one stream takes up to {rt.RAGGED_MAX_BATCH}")
        lens = torch.as_tensor(lengths).reshape(-1)
        if lens.numel() != B:
            raise ValueError(f"lengths {tuple(lens.shape)}: expected ({B},)")
        # the one host sync of the stream
        lens = [min(max(int(v), 0), T) for v in lens.tolist()]
        gain = self.output.fixed_gain(B, mel.device, gain_db) if self.fixed_gain else None  # refusals before the start
        return self._run(mel, lens, gain)

    def _run(self, mel, lens, gain=None) -> Iterator[Chunk]:
        dev = mel.device
        B, _, T = mel.shape
        hop = self.hop
        rplan, up, down, half = self._factor(dev)
        plan4 = self._plan4(dev)
        pl = self._plan(lens, up, down, half, plan4)
        x = mel if (mel.dtype == torch.float32 and mel.is_contiguous()) else rt.f32c(mel)
        g = self.generator
        eng = g.engine()
        with torch.no_grad():
            packed = g.packed(dev)
            # the tables of every step, uploaded once
            cols = []
            for st in pl.steps:
                v = st.voc
                cols += [v.rows, v.start, v.length, [(lo - s) * hop for lo, s in zip(v.crop_lo, v.start)],
                         [lo * hop for lo in v.crop_lo], [(hi - lo) * hop for lo, hi in zip(v.crop_lo, v.crop_hi)]]
                d = st.den if st.den is not None else sp.Windows()
                cols += [d.rows, [s * hop for s in d.start], [n * hop for n in d.length], d.length,
                         [(lo - s) * hop for lo, s in zip(d.crop_lo, d.start)], [lo * hop for lo in d.crop_lo],
                         [(hi - lo) * hop for lo, hi in zip(d.crop_lo, d.crop_hi)]]
                oc = st.out_counts(pl.n_out)
                cols += [[o for o, _, _ in oc], [c for _, c, _ in oc], [int(f) for _, _, f in oc]]
            tabs = self._upload(cols, dev)
            src_lens = torch.tensor(lens, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
            # full-length stitched buffers; a stage reads only what the stage before made final
            raw = torch.zeros((B, T * hop), dtype=torch.float32, device=dev)
            den = torch.zeros((B, T * hop), dtype=torch.float32, device=dev) if self.denoiser is not None else raw
            Wv = pl.max_vocoder_window
            Wd = max(pl.max_denoise_window * hop, 768)  # mt_denoise takes rows longer than n_fft / 2
            Rmax = max([len(st.voc) for st in pl.steps] + [len(st.den) for st in pl.steps if st.den is not None] + [1])
            mel_rows = None if self.per_row else torch.empty((Rmax, 80, Wv), dtype=torch.float32, device=dev)
            wav_rows = None if self.per_row else torch.empty((Rmax, 1, Wv * hop), dtype=torch.float32, device=dev)
            aud_rows = torch.empty((Rmax, Wd), dtype=torch.float32, device=dev) if self.denoiser is not None else None
            done = [tabs[16 * i + 15].bool() for i in range(len(pl.steps))]
            if plan4 is not None:
                # stitched buffers at the output rate: the resampled signal (the denoised buffer itself at equal
                # rates) and its envelope; a range kernel reads only what the stage before made final
                Lo = max(max(pl.n_out, default=0), 1)
                out_lens = torch.tensor(pl.n_out, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
                res = torch.zeros((B, Lo), dtype=torch.float32, device=dev) if rplan is not None else den
                envb = torch.zeros_like(res)
                ceiling = 10.0 ** (self.output.true_peak / 20.0)
                red = self.reduction = torch.ones((B,), dtype=torch.float32, device=dev)  # this stream's own
        enc = self.output.encoding if self.output is not None else None
        for i, st in enumerate(pl.steps):
            t = tabs[16 * i:16 * i + 16]
            with torch.no_grad():
                R = len(st.voc)
                if R and self.per_row:  # fp32: one vocoder call per window
                    v = st.voc
                    for b, s, n, lo, hi in zip(v.rows, v.start, v.length, v.crop_lo, v.crop_hi):
                        w = eng.forward(packed, x[b:b + 1, :, s:s + n].contiguous())
                        raw[b, lo * hop:hi * hop] = w[0, 0, (lo - s) * hop:(hi - s) * hop]
                elif R:
                    rt.window_gather(x, t[0], t[1], t[2], Wv, out=mel_rows[:R])
                    eng.forward(packed, mel_rows[:R], out=wav_rows[:R], lengths=t[2])
                    rt.window_scatter(wav_rows[:R], t[0], t[3], t[4], t[5], raw)
                R = len(st.den) if st.den is not None else 0
                if R:
                    rt.window_gather(raw, t[6], t[7], t[8], Wd, out=aud_rows[:R])
                    y = rt.denoise(aud_rows[:R], self.denoiser.bias_spec, self.strength, lengths=t[9], hop=hop)
                    rt.window_scatter(y, t[6], t[10], t[11], t[12], den)
                if plan4 is not None:
                    # the resampled range into its place in the stitched buffer, its envelope, then the delivered
                    # range through the limiter; rows that ended are clipped inside the kernels
                    if rplan is not None and st.m_hi > st.m_lo:
                        part, _ = rt.resample_range(den, rplan, src_lens, hop, st.m_lo, st.m_hi - st.m_lo)
                        res[:, st.m_lo:st.m_hi] = part  # m_hi <= the greatest output count = Lo
                    if st.p_hi > st.p_lo:
                        rt.peak_envelope_range(res, out_lens, plan4, st.p_lo, st.p_hi - st.p_lo, envb)
                y_lo, y_hi = st.delivered
                cnt = y_hi - y_lo
                if cnt == 0:
                    code = rt.ENCODING_CODES[enc][1] if enc is not None else torch.float32
                    audio = torch.empty((B, 0), dtype=code, device=dev)
                elif plan4 is not None:
                    audio, _ = rt.limit_range(res, envb, out_lens, gain, ceiling, self.output.limiter_window, y_lo,
                                              cnt, red)
                elif rplan is not None:
                    audio, _ = rt.resample_range(den, rplan, src_lens, hop, y_lo, cnt)
                else:
                    audio = den[:, y_lo:y_hi]
                if cnt and gain is not None and plan4 is None:
                    audio = audio * gain[:, None]  # fl32(g x): one rounded fp32 product per sample
                if cnt and self.output is not None:
                    o = self.output
                    audio, _ = rt.encode_audio(audio, t[14], None, o.level, o.limit, o.encoding)
                elif cnt and rplan is None:
                    audio = audio.clone()
            yield Chunk(audio, t[14], t[13], done[i])
