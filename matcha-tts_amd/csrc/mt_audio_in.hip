// Recording input stage on gfx950 (matcha_hip/audio_in.py is the same specification on the CPU): the
// mirror image of mt_audio.hip, from the bytes of a ragged batch of recordings to the log-mel that MatchaTTS.align,
// MatchaTTS.edit and the trainer take. Between the two kernels of this file the stage runs mt_resample (to 22,050 Hz),
// mt_audio_stats (peak level) and mt_audio_edges (trim) as they stand.
//
// audio_decode_kernel: one thread per output frame. PCM16 q / 32768 and the G.711 expansion / 32768 are exact in fp32;
//   an fp32 sample that is not finite becomes 0 (one bad sample must not poison the row's peak, gain and mel).
//   Down-mix: the fp32 sum in channel order, then one product with float(1 / channels). Frames at or past the row's
//   length are not read and come out as 0.
// logmel_ragged_kernel: mt_log_mel's frame body (mt_logmel.h) on s_b[i] = fl32(gain_b audio[b][a_b + i]), i < n_b,
//   reflected at the row's own two ends. One workgroup per (row, LMR_FPW consecutive frames): the twiddle table is
//   built once and the frames' 80 values go through LDS, so that each filter's LMR_FPW values leave as one run. A
//   workgroup past the row's last frame only writes `fill`. The bits of a frame depend on f, n_b and the samples
//   alone: not on the batch, the buffer's L or Fcap.
#include <math.h>

#include "mt_common.h"
#include "mt_logmel.h"
#include "mt_resample.h"  // AU_MAXB, utt_len

namespace mt {

enum { DEC_F32 = 0, DEC_PCM16 = 1, DEC_MULAW = 2 };  // MT_ENC_*
constexpr int DEC_MAX_CH = 8;
constexpr int LMR_FPW = 8;          // frames per workgroup (runtime.LOGMEL_FRAMES)
constexpr int LMR_MAX_L = 1 << 30;  // 2 (n - 1) - i and f * 256 stay inside int32

template <int ENC> struct DecIn;
template <> struct DecIn<DEC_F32> { typedef float T; };
template <> struct DecIn<DEC_PCM16> { typedef int16_t T; };
template <> struct DecIn<DEC_MULAW> { typedef uint8_t T; };

// audio_out.mulaw_decode
__device__ __forceinline__ int mulaw_expand(unsigned byte) {
  const unsigned u = ~byte & 0xFFu;
  const int t = (int)((((u & 0xFu) << 3) + 0x84u) << ((u >> 4) & 7u));
  return (u & 0x80u) ? 0x84 - t : t - 0x84;
}

template <int ENC> __device__ __forceinline__ float dec_sample(typename DecIn<ENC>::T v) {
  if (ENC == DEC_F32) return isfinite((float)v) ? (float)v : 0.f;
  if (ENC == DEC_PCM16) return (float)(int)v * (1.f / 32768.f);
  return (float)mulaw_expand((unsigned)v) * (1.f / 32768.f);
}

template <int ENC>
__global__ __launch_bounds__(256) void audio_decode_kernel(const typename DecIn<ENC>::T* __restrict__ raw, int Lcap,
                                                           const int* __restrict__ lens, int channels, float inv_ch,
                                                           float* __restrict__ out) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Lcap) return;
  const int len = utt_len(lens, b, 1, Lcap);
  float v = 0.f;
  if (i < len) {
    const typename DecIn<ENC>::T* fr = raw + ((size_t)b * Lcap + i) * channels;
    v = dec_sample<ENC>(fr[0]);
    if (channels > 1) {
      for (int c = 1; c < channels; ++c) v = v + dec_sample<ENC>(fr[c]);
      v = v * inv_ch;
    }
  }
  out[(size_t)b * Lcap + i] = v;
}

__global__ __launch_bounds__(256) void logmel_ragged_kernel(const float* __restrict__ audio, int L,
                                                            const int* __restrict__ start,
                                                            const int* __restrict__ end,
                                                            const float* __restrict__ gain,
                                                            const float* __restrict__ basis, float mean, float stdv,
                                                            float fill, float* __restrict__ mel, int Fcap,
                                                            int* __restrict__ frames) {
  __shared__ LogMelLds s;
  __shared__ float tile[LM_NMEL][LMR_FPW];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int f0 = blockIdx.x * LMR_FPW;
  const int a = start ? min(max(start[b], 0), L) : 0;
  const int e = end ? min(max(end[b], a), L) : L;
  const int n = e - a;
  const int nfr = min(logmel_frames(n), Fcap);  // the host checked Fcap >= logmel_frames(L) >= logmel_frames(n)
  if (blockIdx.x == 0 && tid == 0) frames[b] = nfr;
  const int nw = min(LMR_FPW, Fcap - f0);       // columns of mel this workgroup writes (0 when Fcap == 0)
  const int live = min(max(nfr - f0, 0), nw);   // ... and those that are frames of the row
  if (live > 0) {
    const float* x = audio + (size_t)b * L + a;
    const bool scaled = gain != nullptr;
    const float g = scaled ? gain[b] : 1.f;
    logmel_twiddles(s);
    for (int j = 0; j < live; ++j)
      logmel_frame(s, f0 + j, n, [=](int i) { return scaled ? g * x[i] : x[i]; }, basis, mean, stdv,
                   [&](int m, float v) { tile[m][j] = v; });
    __syncthreads();
  }
  float* o = mel + (size_t)b * LM_NMEL * Fcap + f0;
  for (int t = tid; t < LM_NMEL * nw; t += 256) {
    const int m = t / nw, j = t - m * nw;
    o[(size_t)m * Fcap + j] = j < live ? tile[m][j] : fill;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------

int audio_decode(const void* raw, int B, int Lcap, const int* lens, int encoding, int channels, float* out,
                 hipStream_t st) {
  MT_REQUIRE(encoding == DEC_F32 || encoding == DEC_PCM16 || encoding == DEC_MULAW,
             "audio_decode: unknown encoding %d (0 f32, 1 pcm16, 2 mulaw)", encoding);
  MT_REQUIRE(channels >= 1 && channels <= DEC_MAX_CH, "audio_decode: channels %d outside 1..%d", channels,
             DEC_MAX_CH);
  MT_REQUIRE(B > 0 && B <= AU_MAXB && Lcap > 0, "audio_decode: B %d (1..%d), Lcap %d", B, AU_MAXB, Lcap);
  MT_REQUIRE((long long)Lcap * channels < (1ll << 31), "audio_decode: Lcap %d x %d channels per row", Lcap, channels);
  MT_REQUIRE(raw && out, "audio_decode: null argument");
  const dim3 grid((Lcap + 255) / 256, B);
  const float inv_ch = (float)(1.0 / channels);
  if (encoding == DEC_F32)
    hipLaunchKernelGGL(audio_decode_kernel<DEC_F32>, grid, dim3(256), 0, st, (const float*)raw, Lcap, lens, channels,
                       inv_ch, out);
  else if (encoding == DEC_PCM16)
    hipLaunchKernelGGL(audio_decode_kernel<DEC_PCM16>, grid, dim3(256), 0, st, (const int16_t*)raw, Lcap, lens,
                       channels, inv_ch, out);
  else
    hipLaunchKernelGGL(audio_decode_kernel<DEC_MULAW>, grid, dim3(256), 0, st, (const uint8_t*)raw, Lcap, lens,
                       channels, inv_ch, out);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

int log_mel_ragged(const float* audio, int B, int L, const int* start, const int* end, const float* gain,
                   const float* basis, float mean, float stdv, float fill, float* mel, int Fcap, int* frames,
                   hipStream_t st) {
  MT_REQUIRE(B > 0 && B <= AU_MAXB && L > 0 && L < LMR_MAX_L, "log_mel_ragged: B %d (1..%d), L %d (1..%d)", B,
             AU_MAXB, L, LMR_MAX_L - 1);
  MT_REQUIRE(stdv != 0.f, "log_mel_ragged: std must be non-zero");
  MT_REQUIRE(Fcap >= logmel_frames(L) && Fcap <= LMR_MAX_L / LM_HOP,
             "log_mel_ragged: Fcap %d, a row of %d samples has %d frames (at most %d)", Fcap, L, logmel_frames(L),
             LMR_MAX_L / LM_HOP);
  MT_REQUIRE(audio && basis && frames && (mel || Fcap == 0), "log_mel_ragged: null argument");
  const dim3 grid(Fcap > 0 ? (Fcap + LMR_FPW - 1) / LMR_FPW : 1, B);
  hipLaunchKernelGGL(logmel_ragged_kernel, grid, dim3(256), 0, st, audio, L, start, end, gain, basis, mean, stdv,
                     fill, mel, Fcap, frames);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace mt
