"""The output stage after the vocoder / denoiser: sample-rate conversion, per-utterance level and the delivery
encoding for a whole padded batch (the reference's main.py:198-201 does `.clamp(-1, 1)` on one utterance and hands it
to soundfile; rate, level and encoding are left to the caller there). No counterpart module in the reference.

    wav = vocoder(mel, lengths)                      # [B, 1, L], ragged
    wav = denoiser(wav.squeeze(1), 0.00025, lengths) # [B, L]
    out = AudioOutput(16000, normalize="peak", encoding="pcm16")(wav, lengths)
    out.audio[b, :out.lengths[b]]                    # int16 at 16 kHz, peak at 0.95 of full scale

Three HIP launches on the whole batch (mt_resample, mt_audio_stats, mt_audio_encode); row b of the result is, bit for
bit, what the same call returns for that utterance alone (matcha_hip/audio_out.py is the
specification on the CPU).

    out = AudioOutput(16000, loudness=-16.0, true_peak=-1.0, encoding="pcm16")(wav, lengths)

levels every utterance to -16 LUFS (ITU-R BS.1770 gated loudness) with its true peak held at or under -1 dBTP
(mt_loudness and mt_true_peak in place of mt_audio_stats; DESIGN.md §21, matcha_hip/loudness.py), and
`AudioOutput(16000).measure(wav, lengths)` reports both figures of what the stage would deliver at gain 1.

    out = AudioOutput(16000, loudness=-16.0, true_peak=-1.0, limiter=5.0, encoding="pcm16")(wav, lengths)

meets both figures where they conflict: a look-ahead limiter turns the gain down around the peaks only (over 5 ms
before and after each) and the level is made up until the limited signal reads the target (mt_peak_envelope and
mt_limit; DESIGN.md §23, matcha_hip/limiter.py). `AudioOutput.limited` returns that signal before encoding, with the
gain, the deepest reduction and the last static trim of every row.

    out = AudioOutput(16000, gain_db=6.0, true_peak=-1.0, limiter=5.0, encoding="pcm16")(wav, lengths)

applies a gain fixed beforehand (calibrated per voice, say, from `measure`) and the same limiter in one pass: nothing
of it needs the whole utterance, so hifigan.stream.WaveStreamer delivers exactly this chunk by chunk (DESIGN.md §24,
limiter.limit_fixed_ref). `gain_db=` of a call overrides the stage's figure row by row.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from matcha_hip import audio_out
from matcha_hip import limiter as lm
from matcha_hip import loudness as ld
from matcha_hip import runtime as rt


class AudioOut(NamedTuple):
    audio: torch.Tensor          # [B, L_out] fp32 ("f32"), int16 ("pcm16") or uint8 ("mulaw")
    lengths: torch.Tensor        # int32 [B], valid samples of each row at sample_rate
    sample_rate: int
    gain: torch.Tensor           # fp32 [B], the gain each row was multiplied by


class Loudness(NamedTuple):
    lufs: torch.Tensor           # fp64 [B], gated loudness; -inf for a silent, empty or fully gated row
    true_peak_db: torch.Tensor   # fp64 [B], dBTP; -inf for a silent or empty row
    lengths: torch.Tensor        # int32 [B], the measured samples of each row at sample_rate
    sample_rate: int


class Limited(NamedTuple):
    audio: torch.Tensor          # [B, L] fp32 at sample_rate: the levelled and limited signal, before trim and encoding
    lengths: torch.Tensor        # int32 [B]
    sample_rate: int
    gain: torch.Tensor           # fp32 [B], the make-up gain of the last pass
    reduction: torch.Tensor      # fp32 [B], the smallest factor the limiter applied on top of it (1: never worked)
    trim: torch.Tensor           # fp32 [B], min(1, ceiling / ((1 + eps) true peak of `audio`)): the encoder's gain


class AudioOutput:
    """sample_rate / source_rate: any pair whose reduced factor up/down has both parts <= 1024 (from 22,050 Hz: 8000,
    11025, 16000, 24000, 32000, 44100, 48000, ...), Kaiser-windowed sinc with `zeros` zero crossings per side at the
    lower rate and Kaiser `beta` (scipy.signal.resample_poly's default design). normalize: None, "peak" (the row's
    peak becomes `level`, default 0.95) or "rms" (its RMS becomes `level`, default -20 dBFS; with `limit` the gain
    stops where the peak would pass full scale). encoding: "f32", "pcm16" or "mulaw" (G.711). Level and encoding are
    measured on, and applied to, the resampled signal. loudness: a target in LUFS (-70 < target <= 0, ITU-R BS.1770
    gated loudness; needs normalize=None and sample_rate >= 8000): the row's loudness becomes the target, and with
    `limit` the gain stops where the row's true peak (4x oversampled) would pass `true_peak` dBTP (<= 0).
    limiter: a window in ms (needs loudness=; 1 .. 2048 samples at sample_rate): instead of capping the whole row's
    gain, the gain is turned down around the peaks alone, falling over one window before a peak and recovering over
    one after it, and made up in `limiter_passes` (1 .. 8) rounds so that the limited row reads the target.
    gain_db: a fixed gain in dB (finite; excludes normalize= and loudness=): every row is multiplied by
    float32(10^(gain_db / 20)), nothing is measured. With limiter= the gain is turned down around the peaks as above,
    in one pass: no make-up and no trim, and `limiter_passes` is ignored; every sample's envelope is held at the
    ceiling, the delivered true peak passes it by what the smoothing lets through."""

    def __init__(self, sample_rate: int = 22050, source_rate: int = 22050, normalize: Optional[str] = None,
                 level: Optional[float] = None, limit: bool = True, encoding: str = "f32", zeros: int = 10,
                 beta: float = 5.0, hop: int = 256, loudness: Optional[float] = None, true_peak: float = -1.0,
                 limiter: Optional[float] = None, limiter_passes: int = 3, gain_db: Optional[float] = None):
        if normalize not in rt.NORMALIZE_CODES:
            raise ValueError(f"normalize must be one of {list(rt.NORMALIZE_CODES)}, got {normalize!r}")
        if encoding not in rt.ENCODING_CODES:
            raise ValueError(f"encoding must be one of {list(rt.ENCODING_CODES)}, got {encoding!r}")
        audio_out.rates(source_rate, sample_rate)  # ValueError for a factor the kernel does not take
        level = rt.DEFAULT_LEVEL[normalize] if level is None else float(level)
        if not (level > 0 and level < float("inf")):
            raise ValueError(f"level must be finite and positive, got {level}")
        self.sample_rate, self.source_rate = int(sample_rate), int(source_rate)
        self.normalize, self.level, self.limit, self.encoding = normalize, level, bool(limit), encoding
        self.zeros, self.beta, self.hop = int(zeros), float(beta), int(hop)
        true_peak = float(true_peak)
        if not (math.isfinite(true_peak) and true_peak <= 0.0):
            raise ValueError(f"true_peak must be a finite ceiling in dBTP at or under 0, got {true_peak}")
        if loudness is not None:
            loudness = float(loudness)
            if normalize is not None:
                raise ValueError(f"loudness={loudness} and normalize={normalize!r} both set the level: use one")
            if not (math.isfinite(loudness) and -70.0 < loudness <= 0.0):
                raise ValueError(f"loudness must be a finite target in LUFS with -70 < target <= 0, got {loudness}")
            if self.sample_rate < ld.MIN_RATE:
                raise ValueError(f"loudness: sample_rate {self.sample_rate} is below {ld.MIN_RATE} Hz, the lowest "
                                 "rate the K-weighting is designed for")
        if gain_db is not None:
            if normalize is not None or loudness is not None:
                raise ValueError(f"gain_db={gain_db} fixes the gain; normalize= and loudness= measure one: use one")
            lm.fixed_gain_ref(gain_db)  # ValueError unless finite
            gain_db = float(gain_db)
        self.loudness, self.true_peak, self.gain_db = loudness, true_peak, gain_db
        self.limiter, self.limiter_window, self.limiter_passes = None, None, int(limiter_passes)
        if not 1 <= self.limiter_passes <= lm.MAX_PASSES or self.limiter_passes != limiter_passes:
            raise ValueError(f"limiter_passes must be an integer in 1 .. {lm.MAX_PASSES}, got {limiter_passes}")
        if limiter is not None:
            if loudness is None and gain_db is None:
                raise ValueError(f"limiter={limiter} limits a levelled signal: set loudness= (the level is made up "
                                 "to the target) or gain_db= (a fixed gain)")
            self.limiter = float(limiter)
            self.limiter_window = lm.window_samples(self.sample_rate, self.limiter)  # ValueError outside 1 .. 2048

    def _resampled(self, audio: torch.Tensor, lengths, what: str):
        """-> (audio [B, L_out] at sample_rate, lens int32 [B] in samples)"""
        rt.require_gpu(audio, what=what)
        if audio.dim() == 3 and audio.shape[1] == 1:
            audio = audio[:, 0]
        if audio.dim() != 2:
            raise ValueError(f"{what}: audio {tuple(audio.shape)}, expected [B, L] or [B, 1, L]")
        B, L = audio.shape
        if self.sample_rate != self.source_rate:
            plan = rt.resample_plan(self.source_rate, self.sample_rate, self.zeros, self.beta, audio.device)
            return rt.resample(audio, plan, lengths, lmul=self.hop)
        if lengths is None:
            return audio, torch.full((B,), L, dtype=torch.int32, device=audio.device)
        lens = (torch.as_tensor(lengths).to(device=audio.device, dtype=torch.int64) * self.hop).clamp_(0, L)
        return audio, lens.to(torch.int32)

    def _measure(self, audio: torch.Tensor, lens: torch.Tensor):
        """-> (E fp64 [B], TP fp32 [B]) of rows at sample_rate"""
        if self.sample_rate < ld.MIN_RATE:
            raise ValueError(f"loudness: sample_rate {self.sample_rate} is below {ld.MIN_RATE} Hz")
        energy, _ = rt.loudness(audio, lens, self.sample_rate)
        plan4 = rt.resample_plan(self.sample_rate, 4 * self.sample_rate, self.zeros, self.beta, audio.device)
        return energy, rt.true_peak(audio, lens, plan4)

    @torch.inference_mode()
    def measure(self, audio: torch.Tensor, lengths=None) -> Loudness:
        """Loudness (LUFS) and true peak (dBTP) of each row as the stage delivers it at gain 1: measured after the
        rate conversion, before any level. audio and lengths as in __call__. The two log10 are for reporting; the
        gain of `loudness=` is computed from the energies themselves."""
        audio, lens = self._resampled(audio, lengths, "AudioOutput.measure")
        energy, tp = self._measure(audio, lens)
        return Loudness(10.0 * torch.log10(energy) - 0.691, 20.0 * torch.log10(tp.double()), lens, self.sample_rate)

    def fixed_gain(self, B: int, device, gain_db=None) -> torch.Tensor:
        """-> g fp32 [B] on `device`: limiter.fixed_gain_ref of the stage's gain_db, or of the per-row override (a
        sequence or CPU tensor of B finite floats), converted on the host and uploaded: no host synchronisation. A
        device tensor is refused, since reading it would force one."""
        if self.gain_db is None:
            raise ValueError("AudioOutput: gain_db= of a call overrides the stage's fixed gain; the stage was built "
                             "without gain_db=")
        if gain_db is None:
            vals = [self.gain_db] * B
        else:
            if isinstance(gain_db, torch.Tensor):
                if gain_db.device.type != "cpu":
                    raise ValueError("AudioOutput: gain_db is a sequence or a CPU tensor (a device tensor would have "
                                     "to be read back)")
                gain_db = gain_db.reshape(-1).tolist()
            vals = [float(v) for v in gain_db]
            if len(vals) != B:
                raise ValueError(f"AudioOutput: gain_db has {len(vals)} entries for {B} rows")
        g = torch.tensor([float(lm.fixed_gain_ref(v)) for v in vals], dtype=torch.float32)
        return g.to(device, non_blocking=True)

    @torch.inference_mode()
    def __call__(self, audio: torch.Tensor, lengths=None, gain_db=None) -> AudioOut:
        """audio [B, L] or [B, 1, L] at source_rate; lengths int [B] in mel frames (x hop = 256 samples), as
        Generator.forward and Denoiser.forward take it; None: every row is L samples long. gain_db: per-row fixed
        gains in dB in place of the stage's gain_db= (a sequence or CPU tensor of B finite floats)."""
        if gain_db is not None and self.gain_db is None:
            self.fixed_gain(0, None, gain_db)  # ValueError before any launch
        audio, lens = self._resampled(audio, lengths, "AudioOutput")
        return self.finish(audio, lens, gain_db)

    @torch.inference_mode()
    def finish(self, audio: torch.Tensor, lens_samples: torch.Tensor, gain_db=None) -> AudioOut:
        """The level-and-encode half of __call__: audio fp32 [B, L] already at sample_rate, lens_samples int32 [B] in
        samples. What __call__ runs after its rate conversion, and what LongForm runs on joined documents."""
        if gain_db is not None and self.gain_db is None:
            self.fixed_gain(0, None, gain_db)
        rt.require_gpu(audio, what="AudioOutput.finish")
        if audio.dim() != 2:
            raise ValueError(f"AudioOutput.finish: audio {tuple(audio.shape)}, expected [B, L]")
        lens = lens_samples
        if self.gain_db is not None:
            g = self.fixed_gain(audio.shape[0], audio.device, gain_db)
            if self.limiter is not None:
                y = self._limited_fixed(audio, lens, g).audio
            else:
                y = rt.f32c(audio) * g[:, None]  # fl32(g x), one rounded product per sample
            out, _ = rt.encode_audio(y, lens, None, 1.0, True, self.encoding)
            return AudioOut(out, lens, self.sample_rate, g)
        if self.limiter is not None:
            # the limited signal through the unchanged encoder: "rms" at mean square 1 and level 1 is gain 1, which
            # the limit caps at 1 / peak = ceiling / ((1 + eps) TP'): the trim
            lim, peak_eff = self._limited(audio, lens)
            out, _ = rt.encode_audio(lim.audio, lens, "rms", 1.0, True, self.encoding,
                                     stats=(peak_eff, torch.ones_like(peak_eff, dtype=torch.float64)))
            return AudioOut(out, lens, self.sample_rate, lim.gain * lim.trim)
        if self.loudness is None:
            out, gain = rt.encode_audio(audio, lens, self.normalize, self.level, self.limit, self.encoding)
            return AudioOut(out, lens, self.sample_rate, gain)
        # loudness.loudness_gain_ref through gain_ref's "rms" branch: the mean square is the gated energy, the level
        # the target's RMS, and the peak is the true peak over the ceiling, so that 1 / peak caps the gain at c / TP
        energy, tp = self._measure(audio, lens)
        peak_eff = (tp.double() / 10.0 ** (self.true_peak / 20.0)).float()
        peak_eff = torch.where(energy > 0, peak_eff, torch.zeros_like(peak_eff))  # nothing to level: gain 1
        out, gain = rt.encode_audio(audio, lens, "rms", ld.target_level(self.loudness), self.limit, self.encoding,
                                    stats=(peak_eff, energy))
        return AudioOut(out, lens, self.sample_rate, gain)

    def _limited(self, audio: torch.Tensor, lens: torch.Tensor):
        """-> (Limited, peak_eff fp32 [B] = TP' (1 + eps) / ceiling of the limited rows, 0 for a row that was not
        levelled)"""
        c = 10.0 ** (self.true_peak / 20.0)
        level = ld.target_level(self.loudness)
        energy, tp = self._measure(audio, lens)
        live = energy > 0
        zero = torch.zeros_like(tp)
        peak0 = torch.where(live, (tp.double() / c).float(), zero)
        plan4 = rt.resample_plan(self.sample_rate, 4 * self.sample_rate, self.zeros, self.beta, audio.device)
        env = rt.peak_envelope(audio, lens, plan4)
        gain, e_k = None, energy
        for k in range(self.limiter_passes):
            y, gain, reduction = rt.limit(audio, env, lens, (peak0, e_k), level, c, self.limiter_window, gain_in=gain)
            if k + 1 < self.limiter_passes:
                e_k, _ = rt.loudness(y, lens, self.sample_rate)
        # limiter.trim_peak_ref: TP' over the ceiling with the headroom that fp32 delivery and the meter's chain need
        headroom = 1.0 + lm.trim_headroom(plan4.taps_host)
        peak_eff = torch.where(live, (rt.true_peak(y, lens, plan4).double() / c * headroom).float(), zero)
        # audio_out.gain_ref("rms", meansq 1, level 1, limit): min(1, 1 / peak) in fp64, rounded to fp32
        trim = torch.where(peak_eff > 0, 1.0 / peak_eff.double(), torch.ones_like(energy)).clamp_(max=1.0).float()
        return Limited(y, lens, self.sample_rate, gain, reduction, trim), peak_eff

    def _limited_fixed(self, audio: torch.Tensor, lens: torch.Tensor, g: torch.Tensor) -> Limited:
        """limiter.limit_fixed_ref per row: one mt_peak_envelope and one mt_limit at stats (1, 1) and level 1, which
        make the kernel's gain g itself"""
        plan4 = rt.resample_plan(self.sample_rate, 4 * self.sample_rate, self.zeros, self.beta, audio.device)
        env = rt.peak_envelope(audio, lens, plan4)
        ones = torch.ones_like(g)
        y, gain, reduction = rt.limit(audio, env, lens, (ones, ones.double()), 1.0, 10.0 ** (self.true_peak / 20.0),
                                      self.limiter_window, gain_in=g)
        return Limited(y, lens, self.sample_rate, gain, reduction, ones)

    @torch.inference_mode()
    def limited(self, audio: torch.Tensor, lens_samples: torch.Tensor, gain_db=None) -> Limited:
        """audio fp32 [B, L] already at sample_rate, lens_samples int32 [B] in samples (as finish takes them) -> the
        levelled and limited rows before trim and encoding, and the report (limiter.limiter_ref per row; with
        gain_db=, limiter.limit_fixed_ref: gain = g, trim = 1). Needs limiter=. No host synchronisation: the gains,
        energies and peaks stay on the device."""
        if self.limiter is None:
            raise ValueError("AudioOutput.limited: the stage was built without limiter=")
        if gain_db is not None and self.gain_db is None:
            self.fixed_gain(0, None, gain_db)
        rt.require_gpu(audio, what="AudioOutput.limited")
        if audio.dim() != 2:
            raise ValueError(f"AudioOutput.limited: audio {tuple(audio.shape)}, expected [B, L]")
        if self.gain_db is not None:
            return self._limited_fixed(audio, lens_samples, self.fixed_gain(audio.shape[0], audio.device, gain_db))
        return self._limited(audio, lens_samples)[0]
