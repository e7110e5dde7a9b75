// Log-mel featurizer of the training data path (§8f rank 4): train_standalone.py:164-201
// `mel_spectrogram` (same as hifigan/meldataset.py:52-89) followed by `normalize` (:204-210), on gfx950.
//
//   y   = reflect_pad(audio, (n_fft - hop) / 2 = 384 each side)
//   S   = stft(y, n_fft 1024, hop 256, win 1024 Hann (periodic), center=False, onesided)
//   mag = sqrt(re^2 + im^2 + 1e-9)
//   mel = log(clamp(mel_basis[80][513] . mag, 1e-5)),   out = (mel - mean) / std
//
// One 256-thread workgroup per (utterance, frame): the windowed reflect-padded frame goes bit-reversed
// into LDS, a radix-2 1024-point complex FFT runs in place (twiddles from sincospif, the denoiser's
// fft1024), the 513 one-sided magnitudes stay in LDS and each of the 80 filters is a 513-long dot product
// split over 3 lanes. Output [B][80][F] fp32, F = (L - 256) / 256 + 1 frames (torch's framing).
#include "mt_logmel.h"  // the frame body, shared with mt_log_mel_ragged (mt_audio_in.hip)

namespace mt {

namespace {
constexpr int NFFT = LM_NFFT, HOP = LM_HOP, PAD = LM_PAD, NMEL = LM_NMEL;
}

__global__ __launch_bounds__(256) void logmel_kernel(const float* __restrict__ audio, int L, int nfr,
                                                     const float* __restrict__ basis, float mean, float stdv,
                                                     float* __restrict__ out) {
  __shared__ LogMelLds s;
  const int f = blockIdx.x, b = blockIdx.y;
  const float* x = audio + (size_t)b * L;
  logmel_twiddles(s);
  logmel_frame(s, f, L, [x](int i) { return x[i]; }, basis, mean, stdv,
               [=](int m, float v) { out[((size_t)b * NMEL + m) * nfr + f] = v; });
}

int log_mel(const float* audio, int B, int L, const float* basis, float mean, float stdv, float* mel, hipStream_t st) {
  MT_REQUIRE(B > 0 && L >= NFFT - 2 * PAD && L > PAD, "log_mel: need at least %d samples (reflect padding %d)",
             NFFT - 2 * PAD, PAD);
  MT_REQUIRE(stdv != 0.f, "log_mel: std must be non-zero");
  const int nfr = (L + 2 * PAD - NFFT) / HOP + 1;
  hipLaunchKernelGGL(logmel_kernel, dim3(nfr, B), dim3(256), 0, st, audio, L, nfr, basis, mean, stdv, mel);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace mt
