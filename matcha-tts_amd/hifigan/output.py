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
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from matcha_hip import audio_out
from matcha_hip import runtime as rt


class AudioOut(NamedTuple):
    audio: torch.Tensor          # [B, L_out] fp32 ("f32"), int16 ("pcm16") or uint8 ("mulaw")
    lengths: torch.Tensor        # int32 [B], valid samples of each row at sample_rate
    sample_rate: int
    gain: torch.Tensor           # fp32 [B], the gain each row was multiplied by


class AudioOutput:
    """sample_rate / source_rate: any pair whose reduced factor up/down has both parts <= 1024 (from 22,050 Hz: 8000,
    11025, 16000, 24000, 32000, 44100, 48000, ...), Kaiser-windowed sinc with `zeros` zero crossings per side at the
    lower rate and Kaiser `beta` (scipy.signal.resample_poly's default design). normalize: None, "peak" (the row's
    peak becomes `level`, default 0.95) or "rms" (its RMS becomes `level`, default -20 dBFS; with `limit` the gain
    stops where the peak would pass full scale). encoding: "f32", "pcm16" or "mulaw" (G.711). Level and encoding are
    measured on, and applied to, the resampled signal."""

    def __init__(self, sample_rate: int = 22050, source_rate: int = 22050, normalize: Optional[str] = None,
                 level: Optional[float] = None, limit: bool = True, encoding: str = "f32", zeros: int = 10,
                 beta: float = 5.0, hop: int = 256):
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

    @torch.inference_mode()
    def __call__(self, audio: torch.Tensor, lengths=None) -> AudioOut:
        """audio [B, L] or [B, 1, L] at source_rate; lengths int [B] in mel frames (x hop = 256 samples), as
        Generator.forward and Denoiser.forward take it; None: every row is L samples long."""
        rt.require_gpu(audio, what="AudioOutput")
        if audio.dim() == 3 and audio.shape[1] == 1:
            audio = audio[:, 0]
        if audio.dim() != 2:
            raise ValueError(f"AudioOutput: audio {tuple(audio.shape)}, expected [B, L] or [B, 1, L]")
        B, L = audio.shape
        if self.sample_rate != self.source_rate:
            plan = rt.resample_plan(self.source_rate, self.sample_rate, self.zeros, self.beta, audio.device)
            audio, lens = rt.resample(audio, plan, lengths, lmul=self.hop)
        elif lengths is None:
            lens = torch.full((B,), L, dtype=torch.int32, device=audio.device)
        else:
            lens = (torch.as_tensor(lengths).to(device=audio.device, dtype=torch.int64) * self.hop).clamp_(0, L)
            lens = lens.to(torch.int32)
        out, gain = rt.encode_audio(audio, lens, self.normalize, self.level, self.limit, self.encoding)
        return AudioOut(out, lens, self.sample_rate, gain)
