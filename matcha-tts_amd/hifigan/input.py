"""The input stage in front of the model: from a ragged batch of recordings as they arrive (interleaved f32, PCM16 or
G.711 mu-law frames, any channel count up to 8, any rate within a factor of 1024 of 22,050 Hz) to the log-mel and mel
lengths that MatchaTTS.align, MatchaTTS.edit, synthesize(infill_mel=...) and MatchaTrainer.training_step take. The
mirror image of hifigan.output.AudioOutput; no counterpart module in the reference, whose DataLoader workers load,
normalise and featurize one file each on the CPU (train_standalone.py:164-210, hifigan/meldataset.py).

    inp = AudioInput(48000, encoding="pcm16", channels=2, normalize="peak", trim_db=-40.0, trim_pad_ms=10.0)
    rec = inp(raw, lengths)                          # raw int16 [B, Lcap * 2] on the GPU, lengths in frames
    rec.mel[b, :, :rec.mel_lengths[b]]               # log-mel of row b, what align(..., normalized=False) takes
    durations = model.align(x, x_lengths, rec.mel, rec.mel_lengths)

A handful of HIP launches on the whole batch (mt_audio_decode -> mt_resample -> mt_audio_stats -> mt_audio_edges ->
mt_log_mel_ragged) and one host read at the end, of the frame counts; row b of every result is, bit for bit, what the
same call returns for that recording alone (matcha_hip/audio_in.py is the specification on the CPU).
With the model's mel_mean / mel_std and fill=0 the mel is the trainer's batch.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from matcha_hip import audio_in, audio_out
from matcha_hip import runtime as rt


class AudioIn(NamedTuple):
    audio: torch.Tensor          # fp32 [B, L22]: every row decoded, mixed down and at 22,050 Hz (gain not applied)
    lengths: torch.Tensor        # int32 [B], valid samples of each row at 22,050 Hz
    mel: torch.Tensor            # fp32 [B, 80, max(mel_lengths)], `fill` past each row's frames
    mel_lengths: torch.Tensor    # int64 [B]
    gain: torch.Tensor           # fp32 [B], the gain each row was featurized at
    start: torch.Tensor          # int32 [B], the trim edges in samples of `audio`: the mel is that of
    end: torch.Tensor            # int32 [B],  gain * audio[b, start[b]:end[b]]


class AudioInput:
    """sample_rate: the recordings' rate; the factor to 22,050 Hz must have both parts <= 1024 (8000, 16000, 24000,
    44100, 48000, ...; 22050 itself skips the step), Kaiser-windowed sinc as in AudioOutput. encoding: "f32", "pcm16"
    or "mulaw"; channels 1..8 are mixed down to their mean. normalize: None or "peak" (the row's peak becomes `level`,
    default 0.95: hifigan/meldataset.py's normalisation). trim_db: a sample at or above this level (dB re full scale)
    is loud; what lies more than trim_pad_ms before a row's first or after its last loud sample is left out of the mel
    (None: nothing is). mel_mean / mel_std: the model's data statistics, fused (defaults: the plain log-mel). fill:
    the value of mel past a row's last frame."""

    def __init__(self, sample_rate: int, encoding: str = "f32", channels: int = 1, normalize: Optional[str] = None,
                 level: float = 0.95, trim_db: Optional[float] = None, trim_pad_ms: float = 0.0,
                 mel_mean: float = 0.0, mel_std: float = 1.0, fill: float = 0.0, fmin: float = 0, fmax: float = 8000,
                 zeros: int = 10, beta: float = 5.0):
        if encoding not in rt.ENCODING_CODES:
            raise ValueError(f"encoding must be one of {list(rt.ENCODING_CODES)}, got {encoding!r}")
        if int(channels) != channels or not 1 <= int(channels) <= audio_in.MAX_CHANNELS:
            raise ValueError(f"channels must be an integer in 1..{audio_in.MAX_CHANNELS}, got {channels}")
        if normalize not in (None, "peak"):
            raise ValueError(f"normalize must be None or 'peak', got {normalize!r}")
        audio_out.rates(sample_rate, audio_in.SAMPLE_RATE)  # ValueError for a factor the kernel does not take
        level = float(level)
        if not (level > 0 and level < float("inf")):
            raise ValueError(f"level must be finite and positive, got {level}")
        self.thr = None if trim_db is None else float(audio_in.threshold(trim_db))  # ValueError unless finite, <= 0
        self.pad = audio_in.pad_samples(trim_pad_ms)                                # ValueError unless finite, >= 0
        mel_mean, mel_std, fill = float(mel_mean), float(mel_std), float(fill)
        if not (math.isfinite(mel_mean) and math.isfinite(mel_std) and mel_std != 0.0):
            raise ValueError(f"mel_mean {mel_mean} and mel_std {mel_std} must be finite, mel_std non-zero")
        if not (0 <= float(fmin) < float(fmax) <= audio_in.SAMPLE_RATE / 2):
            raise ValueError(f"fmin {fmin} and fmax {fmax} must satisfy 0 <= fmin < fmax <= {audio_in.SAMPLE_RATE / 2}")
        self.sample_rate, self.encoding, self.channels = int(sample_rate), encoding, int(channels)
        self.normalize, self.level = normalize, level
        self.trim_db = None if trim_db is None else float(trim_db)
        self.mel_mean, self.mel_std, self.fill = mel_mean, mel_std, fill
        self.fmin, self.fmax, self.zeros, self.beta = float(fmin), float(fmax), int(zeros), float(beta)

    def _basis(self, device) -> torch.Tensor:
        from hifigan.meldataset import mel_basis
        return mel_basis(audio_in.SAMPLE_RATE, audio_in.N_FFT, audio_in.N_MELS, self.fmin, self.fmax, device)

    @torch.inference_mode()
    def __call__(self, raw: torch.Tensor, lengths=None) -> AudioIn:
        """raw [B, Lcap * channels] of the encoding's dtype (float32, int16, uint8) on the GPU, frames interleaved;
        lengths int [B] in frames at sample_rate (None: every row is Lcap frames long)."""
        rt.require_gpu(raw, what="AudioInput")
        x = rt.decode_audio(raw, lengths, self.encoding, self.channels)
        B, Lcap = x.shape
        if self.sample_rate != audio_in.SAMPLE_RATE:
            plan = rt.resample_plan(self.sample_rate, audio_in.SAMPLE_RATE, self.zeros, self.beta, x.device)
            audio, lens = rt.resample(x, plan, lengths)
        elif lengths is None:
            audio, lens = x, torch.full((B,), Lcap, dtype=torch.int32, device=x.device)
        else:
            audio = x
            lens = torch.as_tensor(lengths).to(device=x.device, dtype=torch.int64).clamp_(0, Lcap).to(torch.int32)
        gain = None
        if self.normalize is not None:
            # audio_out.gain_ref("peak"): level / peak in fp64, rounded to fp32 once; 1 for a silent or empty row
            peak, _ = rt.audio_stats(audio, lens)
            gain = torch.where(peak > 0, self.level / peak.double(), torch.ones_like(peak, dtype=torch.float64)).float()
        if self.thr is not None:
            start, end = rt.audio_edges(audio, lens, self.thr, self.pad)
        else:
            start, end = torch.zeros_like(lens), lens
        mel, frames = rt.log_mel_ragged(audio, self._basis(x.device), start, end, gain, self.mel_mean, self.mel_std,
                                        self.fill)
        mel_lengths = frames.to(torch.int64)
        fmax = int(mel_lengths.max())  # the stage's one host read
        if fmax < mel.shape[2]:
            mel = mel[:, :, :fmax].contiguous()
        if gain is None:
            gain = torch.ones((B,), dtype=torch.float32, device=x.device)
        return AudioIn(audio, lens, mel, mel_lengths, gain, start, end)
