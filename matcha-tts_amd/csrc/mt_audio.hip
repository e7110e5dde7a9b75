// Audio output stage on gfx950 (matcha_hip/audio_out.py is the same specification on the CPU): what
// the reference does on the host after the vocoder (main.py: `.clamp(-1, 1)`, then soundfile), for a whole ragged
// batch: rational resampling, per-utterance level, and the f32 / PCM16 / G.711 mu-law encodings.
//
// resample_kernel: y[m] = sum_k h[half + m down - k up] x[k], m < ceil(len up / down). With c = half + m down the
//   taps that meet a sample are those of phase c % up: y[m] = sum_{q < Q} P[c % up][q] x[c / up - q], one fp32 FMA
//   chain from 0 over q = 0 .. Q - 1 (zero taps of the zero-filled table and zero samples outside [0, len) included):
//   the order depends on nothing but m, which makes a row's bits independent of the batch it sits in.
//   One workgroup per (utterance, tile of RS_TN outputs); a tile at or past the utterance's n_out only writes zeros.
//   Table layout: neighbouring outputs step through the phases with stride s = down % up, so the caller's [up][Q]
//   table is first re-ordered (resample_table_kernel, into the workspace) to tab[q][r] with r the ORDER in which the
//   outputs meet the phases, p(r) = r s % up: output m reads column (r0 + m) % up, lane l + 1 the word after lane
//   l's, for every factor (32 lanes on 32 banks; only the wrap at column up breaks the run when up % 32 != 0).
//   LDS: the whole table (<= 52.5 KiB at the rates of a 22,050 Hz source) and the tile's input span, staged with
//   coalesced loads, zero outside [0, len). When table + span exceed 64 KiB (factors far from the audio rates) the
//   same chain reads both from global memory instead (STAGED = false): same bits, no LDS.
//   mt_resample_range runs the same kernel on the outputs [m_lo, m_lo + cnt) of every row (mg0 = m_lo; 0 for
//   mt_resample): phase, table column and input span come from the output's index in the utterance, so a slice has
//   the bits of the whole, and a tile reads no sample past the one its last output's chain starts at.
//   The tile's staging and chain live in mt_resample.h (resample_tile), shared with true_peak_kernel (mt_loudness.hip).
// audio_stats_kernel: peak = max |x| and the fp64 sum of x^2 over tiles of ST_TILE samples counted from the
//   utterance's start, then audio_stats_final_kernel sums the partials of one utterance in a fixed order. No atomics.
// audio_encode_kernel: gain from the stats (fp64, rounded to fp32), v = clamp(g x, -1, 1) in fp32, then f32 / PCM16
//   rint(v 32767) / mu-law of that PCM16 value; past the utterance's length 0, 0 and 0xFF (mu-law silence).
#include <math.h>

#include "mt_common.h"
#include "mt_level.h"     // NORM_*, gain_of (shared with mt_limiter.hip)
#include "mt_resample.h"  // the tile's staging and FMA chain, utt_len

namespace mt {

constexpr int RS_TN = 2048;            // outputs per resample tile (runtime.RESAMPLE_TILE)
constexpr int RS_MAX_FACTOR = 1024;
constexpr int ST_TILE = 4096;          // samples per stats partial

__global__ void resample_table_kernel(const float* __restrict__ taps, int up, int Q, int s, float* __restrict__ tab,
                                      int tabN) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= tabN) return;
  float v = 0.f;
  if (i < up * Q) {
    const int q = i / up, r = i - q * up;
    v = taps[(size_t)((r * s) % up) * Q + q];
  }
  tab[i] = v;
}

template <bool STAGED>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ audio, int L,
                                                              const int* __restrict__ lens, int lmul,
                                                              const float* __restrict__ tab, int tabN, int half,
                                                              int up, int down, int Q, int r0, int mg0,
                                                              float* __restrict__ out, int Lout,
                                                              int* __restrict__ out_lens) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.y, tid = threadIdx.x;
  // the row holds the outputs [mg0, mg0 + Lout) of the utterance (mt_resample: mg0 = 0, the whole utterance;
  // mt_resample_range: a slice of it). m0 and everything derived from it (phase, input span) count from output 0.
  const int t0 = blockIdx.x * RS_TN;
  const int m0 = mg0 + t0;
  const int len = utt_len(lens, b, lmul, L);
  const long long no = ((long long)len * up + down - 1) / down;
  const long long lend = (long long)mg0 + Lout;
  const int n_out = (int)(no < lend ? no : lend);
  if (blockIdx.x == 0 && tid == 0) out_lens[b] = max(n_out - mg0, 0);
  float* y = out + (size_t)b * Lout + t0;  // y[j]: output m0 + j
  const int nrow = min(RS_TN, Lout - t0);  // outputs of this tile inside the row
  if (m0 >= n_out) {
    for (int j = tid; j < nrow; j += RS_THREADS) y[j] = 0.f;
    return;
  }
  const int nt = min(RS_TN, n_out - m0);   // ... and inside the utterance
  resample_tile<STAGED>(audio + (size_t)b * L, len, tab, tabN, half, up, down, Q, r0, m0, nt, nrow, lds,
                        [y](int j, float v) { y[j] = v; });
}

__global__ __launch_bounds__(256) void audio_stats_kernel(const float* __restrict__ audio, int L,
                                                          const int* __restrict__ lens, int nT,
                                                          double* __restrict__ psum, float* __restrict__ pmax) {
  __shared__ double sd[256];
  __shared__ float sm[256];
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int len = utt_len(lens, b, 1, L);
  const long long i0 = (long long)t * ST_TILE;
  if (i0 >= len) return;  // the final pass reads the partials of live tiles only
  const int e = (int)(i0 + ST_TILE < len ? i0 + ST_TILE : len);
  const float* x = audio + (size_t)b * L;
  double s = 0.0;
  float mx = 0.f;
  for (int i = (int)i0 + tid; i < e; i += 256) {
    const float v = x[i];
    s += (double)v * (double)v;  // the product of two fp32 values is exact in fp64
    mx = fmaxf(mx, fabsf(v));
  }
  sd[tid] = s;
  sm[tid] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      sd[tid] += sd[tid + o];
      sm[tid] = fmaxf(sm[tid], sm[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    psum[(size_t)b * nT + t] = sd[0];
    pmax[(size_t)b * nT + t] = sm[0];
  }
}

__global__ __launch_bounds__(256) void audio_stats_final_kernel(const double* __restrict__ psum,
                                                                const float* __restrict__ pmax, int L,
                                                                const int* __restrict__ lens, int nT,
                                                                float* __restrict__ peak,
                                                                double* __restrict__ meansq) {
  __shared__ double sd[256];
  __shared__ float sm[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = utt_len(lens, b, 1, L);
  const int nt = (int)(((long long)len + ST_TILE - 1) / ST_TILE);
  double s = 0.0;
  float mx = 0.f;
  for (int t = tid; t < nt; t += 256) {
    s += psum[(size_t)b * nT + t];
    mx = fmaxf(mx, pmax[(size_t)b * nT + t]);
  }
  sd[tid] = s;
  sm[tid] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      sd[tid] += sd[tid + o];
      sm[tid] = fmaxf(sm[tid], sm[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    peak[b] = sm[0];
    meansq[b] = len > 0 ? sd[0] / (double)len : 0.0;
  }
}

enum { ENC_F32 = 0, ENC_PCM16 = 1, ENC_MULAW = 2 };

// audio_out.mulaw_ref
__device__ __forceinline__ unsigned mulaw_of(int q) {
  const unsigned sign = q < 0 ? 0x80u : 0u;
  const int mag = min(abs(q), 32635) + 0x84;  // 0x84 .. 0x7fff: the highest set bit is one of bits 7 .. 14
  const int seg = 24 - __clz(mag);
  const unsigned mant = (unsigned)(mag >> (seg + 3)) & 0xFu;
  return ~(sign | ((unsigned)seg << 4) | mant) & 0xFFu;
}

template <int ENC> struct EncOut;
template <> struct EncOut<ENC_F32> { typedef float T; };
template <> struct EncOut<ENC_PCM16> { typedef int16_t T; };
template <> struct EncOut<ENC_MULAW> { typedef uint8_t T; };

// V samples per thread (4: rows and pointers allow 16-byte loads; 1 otherwise)
template <int V, int ENC>
__global__ __launch_bounds__(256) void audio_encode_kernel(const float* __restrict__ audio, int L,
                                                           const int* __restrict__ lens,
                                                           const float* __restrict__ peak,
                                                           const double* __restrict__ meansq, int normalize,
                                                           double level, int limit, void* __restrict__ out,
                                                           float* __restrict__ gain_out) {
  typedef typename EncOut<ENC>::T OT;
  __shared__ float gs;
  const int b = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) {
    gs = normalize == NORM_NONE ? 1.f : gain_of(peak[b], meansq[b], normalize, level, limit);
    if (gain_out && blockIdx.x == 0) gain_out[b] = gs;
  }
  __syncthreads();
  const float g = gs;
  const int i = (blockIdx.x * 256 + tid) * V;
  if (i >= L) return;
  const int len = utt_len(lens, b, 1, L);
  const float* x = audio + (size_t)b * L + i;
  float xv[V];
  if (V == 4) {
    const f32x4 v4 = *(const f32x4*)x;
#pragma unroll
    for (int e = 0; e < V; ++e) xv[e] = v4[e];
  } else {
    xv[0] = x[0];
  }
  struct alignas(sizeof(OT) * V) Pack {
    OT v[V];
  } o;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const bool live = i + e < len;
    const float v = fminf(fmaxf(g * xv[e], -1.f), 1.f);
    if (ENC == ENC_F32) {
      o.v[e] = (OT)(live ? v : 0.f);
    } else {
      const int q = live ? (int)rintf(v * 32767.f) : 0;
      o.v[e] = (OT)(ENC == ENC_PCM16 ? q : (int)mulaw_of(q));
    }
  }
  *(Pack*)((OT*)out + (size_t)b * L + i) = o;
}

// ---- host side -----------------------------------------------------------------------------------------------

static int taps_per_phase(int half, int up) { return (2 * half + 1 + up - 1) / up; }
static size_t table_floats(int half, int up) { return ((size_t)up * taps_per_phase(half, up) + 3) & ~(size_t)3; }
int resample_taps_per_phase(int half, int up) { return taps_per_phase(half, up); }
size_t resample_table_floats(int half, int up) { return table_floats(half, up); }
static int igcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

static int resample_check(int half, int up, int down) {
  MT_REQUIRE(up >= 1 && down >= 1 && up <= RS_MAX_FACTOR && down <= RS_MAX_FACTOR,
             "resample: factor %d/%d outside 1..%d", up, down, RS_MAX_FACTOR);
  MT_REQUIRE(igcd(up, down) == 1, "resample: factor %d/%d is not in lowest terms", up, down);
  MT_REQUIRE(half >= 0 && half <= (1 << 24), "resample: filter half-length %d", half);
  return 0;
}

size_t resample_workspace_bytes(int half, int up, int down) {
  if (resample_check(half, up, down) != 0) return 0;
  return table_floats(half, up) * sizeof(float);
}

int resample_table_launch(const float* taps, int half, int up, int down, float* tab, int* r0_out, hipStream_t st) {
  const size_t tabN = table_floats(half, up);
  const int Q = taps_per_phase(half, up), s = down % up;
  int r0 = 0;  // the column of output 0: its phase is half % up
  while ((r0 * s) % up != half % up) ++r0;
  hipLaunchKernelGGL(resample_table_kernel, dim3((unsigned)((tabN + 255) / 256)), dim3(256), 0, st, taps, up, Q, s,
                     tab, (int)tabN);
  MT_CHECK_HIP(hipGetLastError());
  *r0_out = r0;
  return 0;
}

// the table re-order, then resample_kernel on the outputs [mg0, mg0 + Lout) of every row (the callers check the rest)
static int resample_launch(const float* audio, int B, int L, const int* lens, int lmul, const float* taps, int half,
                           int up, int down, int mg0, float* out, int Lout, int* out_lens, void* ws, size_t ws_bytes,
                           hipStream_t st) {
  const size_t tabN = table_floats(half, up);
  MT_REQUIRE(ws && ws_bytes >= tabN * sizeof(float) && ((uintptr_t)ws & 15) == 0,
             "resample: workspace too small or not 16-byte aligned");
  const int Q = taps_per_phase(half, up);
  int r0 = 0;
  float* tab = (float*)ws;
  const int rc = resample_table_launch(taps, half, up, down, tab, &r0, st);
  if (rc != 0) return rc;
  const size_t span_max = ((size_t)(up - 1) + (size_t)(RS_TN - 1) * down) / up + Q;
  const size_t lds = (tabN + span_max) * sizeof(float);
  const dim3 grid((Lout + RS_TN - 1) / RS_TN, B);
  if (lds <= (size_t)RS_LDS_MAX)
    hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(RS_THREADS), lds, st, audio, L, lens, lmul, tab, (int)tabN,
                       half, up, down, Q, r0, mg0, out, Lout, out_lens);
  else
    hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(RS_THREADS), 0, st, audio, L, lens, lmul, tab, (int)tabN,
                       half, up, down, Q, r0, mg0, out, Lout, out_lens);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

int resample(const float* audio, int B, int L, const int* lens, int lmul, const float* taps, int half, int up,
             int down, float* out, int Lout, int* out_lens, void* ws, size_t ws_bytes, hipStream_t st) {
  if (resample_check(half, up, down) != 0) return -1;
  MT_REQUIRE(B > 0 && B <= AU_MAXB && L > 0, "resample: B %d (1..%d), L %d", B, AU_MAXB, L);
  const long long need = ((long long)L * up + down - 1) / down;
  MT_REQUIRE(need < (1ll << 31) - RS_TN, "resample: %lld output samples per row", need);
  MT_REQUIRE(Lout >= need, "resample: Lout %d < ceil(L up / down) = %lld", Lout, need);
  MT_REQUIRE(Lout < (1ll << 31) - RS_TN, "resample: Lout %d", Lout);
  MT_REQUIRE(!lens || lmul > 0, "resample: length multiplier %d", lmul);
  MT_REQUIRE(audio && taps && out && out_lens, "resample: null argument");
  return resample_launch(audio, B, L, lens, lmul, taps, half, up, down, 0, out, Lout, out_lens, ws, ws_bytes, st);
}

int resample_range(const float* audio, int B, int L, const int* lens, int lmul, const float* taps, int half, int up,
                   int down, int m_lo, int cnt, float* out, int* out_cnt, void* ws, size_t ws_bytes, hipStream_t st) {
  if (resample_check(half, up, down) != 0) return -1;
  MT_REQUIRE(B > 0 && B <= AU_MAXB && L > 0, "resample_range: B %d (1..%d), L %d", B, AU_MAXB, L);
  MT_REQUIRE(m_lo >= 0 && cnt > 0, "resample_range: outputs [%d, %d + %d)", m_lo, m_lo, cnt);
  MT_REQUIRE((long long)m_lo + cnt < (1ll << 31) - RS_TN, "resample_range: outputs [%d, %d + %d)", m_lo, m_lo, cnt);
  MT_REQUIRE(!lens || lmul > 0, "resample_range: length multiplier %d", lmul);
  MT_REQUIRE(audio && taps && out && out_cnt, "resample_range: null argument");
  return resample_launch(audio, B, L, lens, lmul, taps, half, up, down, m_lo, out, cnt, out_cnt, ws, ws_bytes, st);
}

size_t audio_stats_workspace_bytes(int B, int L) {
  if (B <= 0 || L <= 0) return 0;
  const size_t nT = ((size_t)L + ST_TILE - 1) / ST_TILE;
  return (size_t)B * nT * (sizeof(double) + sizeof(float));
}

int audio_stats(const float* audio, int B, int L, const int* lens, float* peak, double* meansq, void* ws,
                size_t ws_bytes, hipStream_t st) {
  MT_REQUIRE(B > 0 && B <= AU_MAXB && L > 0, "audio_stats: B %d (1..%d), L %d", B, AU_MAXB, L);
  MT_REQUIRE(audio && peak && meansq, "audio_stats: null argument");
  MT_REQUIRE(ws && ws_bytes >= audio_stats_workspace_bytes(B, L) && ((uintptr_t)ws & 7) == 0,
             "audio_stats: workspace too small or not 8-byte aligned");
  const int nT = (int)(((size_t)L + ST_TILE - 1) / ST_TILE);
  double* psum = (double*)ws;
  float* pmax = (float*)(psum + (size_t)B * nT);
  hipLaunchKernelGGL(audio_stats_kernel, dim3(nT, B), dim3(256), 0, st, audio, L, lens, nT, psum, pmax);
  MT_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(audio_stats_final_kernel, dim3(B), dim3(256), 0, st, (const double*)psum, (const float*)pmax, L,
                     lens, nT, peak, meansq);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

template <int V>
static void launch_encode(int encoding, dim3 grid, hipStream_t st, const float* audio, int L, const int* lens,
                          const float* peak, const double* meansq, int normalize, double level, int limit, void* out,
                          float* gain_out) {
  if (encoding == ENC_F32)
    hipLaunchKernelGGL((audio_encode_kernel<V, ENC_F32>), grid, dim3(256), 0, st, audio, L, lens, peak, meansq,
                       normalize, level, limit, out, gain_out);
  else if (encoding == ENC_PCM16)
    hipLaunchKernelGGL((audio_encode_kernel<V, ENC_PCM16>), grid, dim3(256), 0, st, audio, L, lens, peak, meansq,
                       normalize, level, limit, out, gain_out);
  else
    hipLaunchKernelGGL((audio_encode_kernel<V, ENC_MULAW>), grid, dim3(256), 0, st, audio, L, lens, peak, meansq,
                       normalize, level, limit, out, gain_out);
}

int audio_encode(const float* audio, int B, int L, const int* lens, const float* peak, const double* meansq,
                 int normalize, double level, int limit, int encoding, void* out, float* gain_out, hipStream_t st) {
  MT_REQUIRE(encoding == ENC_F32 || encoding == ENC_PCM16 || encoding == ENC_MULAW,
             "audio_encode: unknown encoding %d (0 f32, 1 pcm16, 2 mulaw)", encoding);
  MT_REQUIRE(normalize == NORM_NONE || normalize == NORM_PEAK || normalize == NORM_RMS,
             "audio_encode: unknown normalisation mode %d (0 none, 1 peak, 2 rms)", normalize);
  MT_REQUIRE(isfinite(level) && level > 0.0,
             "audio_encode: level %g is not a finite positive number", level);
  MT_REQUIRE(B > 0 && B <= AU_MAXB && L > 0, "audio_encode: B %d (1..%d), L %d", B, AU_MAXB, L);
  MT_REQUIRE(audio && out && (normalize == NORM_NONE || (peak && meansq)), "audio_encode: null argument");
  const bool v4 = L % 4 == 0 && (((uintptr_t)audio | (uintptr_t)out) & 15) == 0;
  if (v4)
    launch_encode<4>(encoding, dim3((L / 4 + 255) / 256, B), st, audio, L, lens, peak, meansq, normalize, level,
                     limit, out, gain_out);
  else
    launch_encode<1>(encoding, dim3((L + 255) / 256, B), st, audio, L, lens, peak, meansq, normalize, level, limit,
                     out, gain_out);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace mt
