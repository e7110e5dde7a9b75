"""The recording input stage on the CPU (numpy only, no GPU): the specification the HIP kernels of
csrc/mt_audio_in.hip and the stage hifigan/input.py builds from them are tested against. The mirror
image of audio_out.py, whose definitions it reuses wherever they already state the operation:

* ``decode_ref``: interleaved f32 / PCM16 / G.711 mu-law frames -> mono fp32 (mt_audio_decode).
* the rate change to ``SAMPLE_RATE``: ``audio_out.rates`` / ``design_filter`` / ``polyphase`` / ``resample_ref``
  (``rates_in``, ``resample_in_ref``).
* trim: ``join.edges_ref`` at ``threshold(trim_db)``, the pad given in samples at 22,050 Hz (``edges_in_ref``).
* level: ``audio_out.gain_ref(peak, None, "peak", level)`` of the whole resampled row (``gain_in_ref``). The peak of
  the trimmed range equals the whole row's whenever that range is not empty: the loudest sample is loud.
* ``frames_ref`` and ``log_mel_ref``: the reference's featurizer restated in fp64 (mt_log_mel_ragged).
"""
from __future__ import annotations

import numpy as np

from . import audio_out
from . import join as jn

SAMPLE_RATE = 22050
ENCODINGS = ("f32", "pcm16", "mulaw")
DTYPES = {"f32": np.float32, "pcm16": np.int16, "mulaw": np.uint8}
MAX_CHANNELS = 8
N_FFT, HOP, N_MELS, PAD = 1024, 256, 80, (1024 - 256) // 2


def decode_ref(raw, encoding: str, channels: int = 1) -> np.ndarray:
    """raw [n * channels] interleaved frames of the encoding's type -> mono fp32 [n]. pcm16: q / 32768 (exact, the
    reference's MAX_WAV_VALUE); mulaw: audio_out.mulaw_decode(u) / 32768; f32: the value, 0.0f in place of a NaN or
    an infinity. channels > 1: the fp32 sum in channel order ((c0 + c1) + c2) ..., then ONE fp32 product with
    float32(1 / channels)."""
    if encoding not in ENCODINGS:
        raise ValueError(f"encoding must be one of {ENCODINGS}, got {encoding!r}")
    channels = int(channels)
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"channels must be in 1..{MAX_CHANNELS}, got {channels}")
    raw = np.asarray(raw).reshape(-1)
    if raw.dtype != DTYPES[encoding]:
        raise ValueError(f"{encoding} frames are {np.dtype(DTYPES[encoding]).name}, got {raw.dtype.name}")
    if raw.shape[0] % channels:
        raise ValueError(f"{raw.shape[0]} values are no whole number of {channels}-channel frames")
    if encoding == "f32":
        v = np.where(np.isfinite(raw), raw, np.float32(0.0)).astype(np.float32)
    elif encoding == "pcm16":
        v = raw.astype(np.float32) / np.float32(32768.0)
    else:
        v = audio_out.mulaw_decode(raw).astype(np.float32) / np.float32(32768.0)
    v = v.reshape(-1, channels)
    if channels == 1:
        return np.ascontiguousarray(v[:, 0])
    acc = v[:, 0].copy()
    for c in range(1, channels):
        acc = (acc + v[:, c]).astype(np.float32)
    return (acc * np.float32(1.0 / channels)).astype(np.float32)


def rates_in(sample_rate: int):
    """(up, down) of sample_rate -> 22,050 Hz; ValueError above audio_out.MAX_FACTOR, as on the output side"""
    return audio_out.rates(sample_rate, SAMPLE_RATE)


def resample_in_ref(x, sample_rate: int, zeros: int = 10, beta: float = 5.0, fp32_taps: bool = True) -> np.ndarray:
    """x [n] at sample_rate -> fp64 [ceil(n up / down)] at 22,050 Hz: audio_out.resample_ref with the filter
    audio_out.design_filter gives, its taps rounded to fp32 as the kernel holds them (fp32_taps)."""
    up, down = rates_in(sample_rate)
    h, half = audio_out.design_filter(up, down, zeros, beta)
    if fp32_taps:
        h = h.astype(np.float32).astype(np.float64)
    return audio_out.resample_ref(x, up, down, h, half)


def threshold(trim_db: float) -> np.float32:
    """10^(trim_db / 20) as fp32: a sample is loud when |x| >= it"""
    trim_db = float(trim_db)
    if not (np.isfinite(trim_db) and trim_db <= 0.0):
        raise ValueError(f"trim_db must be a finite level at or under 0 dBFS, got {trim_db}")
    return np.float32(10.0 ** (trim_db / 20.0))


def pad_samples(trim_pad_ms: float) -> int:
    trim_pad_ms = float(trim_pad_ms)
    if not (np.isfinite(trim_pad_ms) and trim_pad_ms >= 0.0):
        raise ValueError(f"trim_pad_ms must be finite and >= 0, got {trim_pad_ms}")
    return int(round(trim_pad_ms * SAMPLE_RATE / 1000.0))


def edges_in_ref(x, n: int, trim_db, pad: int = 0):
    """-> (start, end) of the row x[0 .. n) at 22,050 Hz: join.edges_ref at threshold(trim_db); (0, n) without trim"""
    if trim_db is None:
        return 0, min(max(int(n), 0), np.asarray(x).reshape(-1).shape[0])
    return jn.edges_ref(x, n, float(threshold(trim_db)), int(pad))


def gain_in_ref(x, n: int, normalize, level: float = 0.95) -> np.float32:
    """The gain of the row x[0 .. n): audio_out.gain_ref of its peak; 1 without normalisation and for a silent row"""
    if normalize not in (None, "peak"):
        raise ValueError(f"normalize must be None or 'peak', got {normalize!r}")
    x = np.asarray(x, dtype=np.float32).reshape(-1)[:max(int(n), 0)]
    peak = float(np.abs(x).max()) if x.size else 0.0
    return audio_out.gain_ref(peak, None, normalize, level)


def frames_ref(n: int) -> int:
    """Frames of a row of n samples: the reflect padding of 384 needs n > 384 (a shorter row yields none and is not
    an error), torch's framing then gives (n - 256) // 256 + 1"""
    n = int(n)
    return 0 if n <= PAD else (n - HOP) // HOP + 1


def mel_basis(fmin: float = 0.0, fmax: float = 8000.0) -> np.ndarray:
    """The Slaney filterbank fp32 [80][513] of the reference's configuration (hifigan.meldataset.librosa_mel_fn)"""
    from hifigan.meldataset import librosa_mel_fn
    return librosa_mel_fn(SAMPLE_RATE, N_FFT, N_MELS, fmin, fmax)


def log_mel_ref(x, basis, gain=1.0, mean: float = 0.0, std: float = 1.0) -> np.ndarray:
    """fp64 [80][frames_ref(n)] of the signal fl32(gain x[i]): reflect pad 384 at the signal's own two ends, periodic
    Hann 1024, hop 256, sqrt(re^2 + im^2 + 1e-9), basis ., log(clamp(., 1e-5)), (. - mean) / std: the reference's
    featurizer (train_standalone.py:164-210) in fp64."""
    x = (np.float32(gain) * np.asarray(x, dtype=np.float32).reshape(-1)).astype(np.float32)
    nfr = frames_ref(x.shape[0])
    basis = np.asarray(basis, dtype=np.float64)
    if nfr == 0:
        return np.zeros((basis.shape[0], 0), dtype=np.float64)
    y = np.pad(x.astype(np.float64), (PAD, PAD), mode="reflect")
    win = np.sin(np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT) ** 2
    idx = np.arange(nfr)[:, None] * HOP + np.arange(N_FFT)[None, :]
    spec = np.fft.rfft(y[idx] * win[None, :], axis=1)                  # [F][513]
    mag = np.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    mel = np.log(np.maximum(basis @ mag.T, 1e-5))
    return (mel - float(mean)) / float(std)
