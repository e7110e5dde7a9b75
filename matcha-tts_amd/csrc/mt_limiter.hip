// Look-ahead true-peak limiter of every row of a ragged batch on gfx950 (matcha_hip/limiter.py is the
// same specification on the CPU, bit for bit).
//
// peak_envelope_kernel: p[i] = the largest magnitude the waveform reaches around sample i: |x[i]| and the 4x
//   oversampled signal three outputs to each side. One workgroup per (row, tile of LM_ENV_T samples counted from the
//   row's start): the resampler's tile (mt_resample.h) at 4/1 over the outputs 4 t0 - 3 .. 4 (t0 + T - 1) + 3 that lie
//   inside the row, with a sink that leaves |r| in LDS (the FMA chain of mt_true_peak, the same bits; nothing of r
//   goes to memory), then seven LDS reads per sample. fmaxf from 0: a NaN counts as absent.
// limit_kernel: one workgroup per (row, tile of LM_T samples counted from the row's start).
//   1. q[j] = floor(2^30 c32 / (g p[j])) where g p[j] > c32, else 2^30, for j in [t0 - (W - 1), t0 + T + W - 1]
//      (2^30 outside the row), staged into LDS with coalesced loads of p. g is the row's gain, formed here with the
//      encoder's gain_of (mt_level.h).
//   2. m[j] = min q[j .. j + W - 1] by van Herk / Gil-Werman: the staged span is cut into blocks of W; a prefix
//      minimum and a suffix minimum inside every block, then m[u] = min(suffix[u], prefix[u + W - 1]). Both are
//      segmented scans: a thread walks its own chunk of C consecutive words (C odd: 32 lanes on 32 banks), the 256
//      chunk results combine through a segmented Hillis-Steele scan in LDS, and the carry is folded into the words
//      before the chunk's first block edge. O(1) per sample for every W.
//   3. S[i] = sum of m over the W windows that hold i, from an exclusive 64-bit prefix sum of m in LDS (the same
//      chunks, a plain scan of the 256 totals), and s[i] = float32(double(S) / double(W 2^30)).
//   4. y[i] = fl32(fl32(g x[i]) s[i]) (contraction off), coalesced; zero from the row's length on. The tile's
//      min s goes to the workspace; limit_final_kernel takes the row's minimum over its live tiles.
//   Minimum and sum are integer operations: any order gives the same bits, so a row's result depends on its own
//   samples alone. No atomics. peak, meansq and the gains are device memory the host never reads.
// Both tile bodies are device functions of the tile's origin (envelope_tile, limit_tile). The whole-row kernels call
// them from blockIdx.x * T; peak_envelope_range_kernel and limit_range_kernel (a fixed gain and the
// limiter chunk by chunk in a stream) call them from i_lo + blockIdx.x * T, cut at the range's end, on full-length
// buffers of which only what the range needs has been written: the envelope reads (half + 3) / 4 samples past the
// range, the limiter W - 1 envelope samples to either side of it. Same code, same bits as the whole rows.
// limit_range_final_kernel folds the range's tile minima into a running minimum per row.
#include <limits.h>
#include <math.h>

#include "mt_common.h"
#include "mt_level.h"
#include "mt_resample.h"

namespace mt {

constexpr int LM_THREADS = 256;
constexpr int LM_ENV_T = 512;                 // samples per envelope tile (runtime.ENVELOPE_TILE)
constexpr int LM_ENV_N = 4 * LM_ENV_T + 3;    // 4x outputs a tile reads: 4 t0 - 3 .. 4 (t0 + T - 1) + 3
constexpr int LM_T = 2048;                    // samples per limiter tile (runtime.LIMIT_TILE)
constexpr int LM_MAX_W = 2048;                // window in samples (runtime.LIMIT_MAX_WINDOW)
constexpr int LM_ONE = 1 << 30;               // gain 1 in the curve's fixed point
constexpr int LM_MAX_HALF = 1024;             // mt_true_peak's bounds on the filter and on a row
constexpr int LM_MAX_L = (1 << 29) - 2048;
static_assert(LM_THREADS == RS_THREADS && LM_T % LM_THREADS == 0 && LM_ENV_T % LM_THREADS == 0, "tile shapes");
// q and the prefix sums of the widest window, with the scans' scratch, inside 64 KiB
static_assert(4 * (LM_T + 2 * LM_MAX_W) + 8 * (LM_T + LM_MAX_W) + 16 * LM_THREADS + 64 <= 64 * 1024, "LDS");

// One envelope tile: the samples [t0, min(t0 + LM_ENV_T, k_end)) of the row x[0 .. len), t0 < len, into e[k]; zero
// from len on. The 4x outputs, and through them the samples of x, are those of these samples alone: nothing past
// min(len - 1, min(t0 + LM_ENV_T, k_end) - 1 + (half + 3) / 4) is read. Every output's chain depends on its own
// index in the row, not on t0: the same bits from any origin.
__device__ __forceinline__ void envelope_tile(const float* __restrict__ x, int len, const float* __restrict__ tab,
                                              int tabN, int half, int Q, int r0, int t0, int k_end,
                                              float* __restrict__ e) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float ar[LM_ENV_N];
  const int tid = threadIdx.x;
  const int t1 = min(t0 + LM_ENV_T, k_end);  // > t0
  const int n_out = 4 * len;
  const int m0 = max(4 * t0 - 3, 0);
  const int m1 = min(4 * (t1 - 1) + 3, n_out - 1);  // >= 4 t0 >= m0
  const int nt = m1 - m0 + 1;                       // <= LM_ENV_N
  float* a = ar;
  resample_tile<true>(x, len, tab, tabN, half, 4, 1, Q, r0, m0, nt, nt, lds,
                      [a](int j, float v) { a[j] = fabsf(v); });
  __syncthreads();
  for (int i = tid; i < LM_ENV_T; i += LM_THREADS) {
    const int k = t0 + i;
    if (k >= t1) break;
    float p = 0.f;
    if (k < len) {
      p = fmaxf(p, fabsf(x[k]));
      const int lo = max(4 * k - 3, m0), hi = min(4 * k + 3, m1);
      for (int m = lo; m <= hi; ++m) p = fmaxf(p, ar[m - m0]);
    }
    e[k] = p;
  }
}

__global__ __launch_bounds__(LM_THREADS) void peak_envelope_kernel(const float* __restrict__ audio, int L,
                                                                   const int* __restrict__ lens,
                                                                   const float* __restrict__ tab, int tabN, int half,
                                                                   int Q, int r0, float* __restrict__ env) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int t0 = blockIdx.x * LM_ENV_T;  // < L <= LM_MAX_L
  const int len = utt_len(lens, b, 1, L);
  float* e = env + (size_t)b * L;
  if (t0 >= len) {
    for (int i = tid; i < LM_ENV_T && t0 + i < L; i += LM_THREADS) e[t0 + i] = 0.f;
    return;
  }
  envelope_tile(audio + (size_t)b * L, len, tab, tabN, half, Q, r0, t0, L, e);
}

// mt_peak_envelope_range: the tiles count from i_lo, and only [i_lo, i_lo + cnt) inside the row is written
__global__ __launch_bounds__(LM_THREADS) void peak_envelope_range_kernel(const float* __restrict__ audio, int L,
                                                                         const int* __restrict__ lens,
                                                                         const float* __restrict__ tab, int tabN,
                                                                         int half, int Q, int r0, int i_lo, int cnt,
                                                                         float* __restrict__ env) {
  const int b = blockIdx.y;
  const int len = utt_len(lens, b, 1, L);
  const long long t0 = (long long)i_lo + (long long)blockIdx.x * LM_ENV_T;  // < i_lo + cnt < 2^31
  const int k_end = (int)min((long long)len, (long long)i_lo + cnt);
  if (t0 >= k_end) return;  // t0 < len <= LM_MAX_L from here on
  envelope_tile(audio + (size_t)b * L, len, tab, tabN, half, Q, r0, (int)t0, k_end, env + (size_t)b * L);
}

// the row's gain: g_in (1 without one) through gain_of's "rms" branch at the level g_in * level, i.e.
// float32(double(g_in) level / sqrt(meansq)); unchanged when the row is not levelled (peak == 0) or meansq == 0
__device__ __forceinline__ float limit_gain(const float* __restrict__ peak, const double* __restrict__ meansq,
                                            const float* __restrict__ gain_in, int b, double level, bool& live) {
  const float pk = peak[b];
  const double ms = meansq[b];
  live = pk > 0.f;
  float g = gain_in ? gain_in[b] : 1.f;
  if (live && ms > 0.0) g = gain_of(pk, ms, NORM_RMS, (double)g * level, 0);
  return g;
}

// Exclusive segmented min-scan over the 256 chunk results in the order of idx: the minimum of the chunks before idx
// back to (and with) the last one that holds a block edge (f != 0); INT_MAX for idx 0. sv, sf: [2][LM_THREADS].
__device__ __forceinline__ int seg_min_carry(int v, int f, int idx, int* sv, int* sf) {
  int cur = 0;
  sv[idx] = v;
  sf[idx] = f;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < LM_THREADS; o <<= 1) {
    int bv = sv[cur * LM_THREADS + idx], bf = sf[cur * LM_THREADS + idx];
    if (idx >= o) {
      if (!bf) bv = min(bv, sv[cur * LM_THREADS + idx - o]);
      bf |= sf[cur * LM_THREADS + idx - o];
    }
    cur ^= 1;
    sv[cur * LM_THREADS + idx] = bv;
    sf[cur * LM_THREADS + idx] = bf;
    __syncthreads();
  }
  const int r = idx > 0 ? sv[cur * LM_THREADS + idx - 1] : INT_MAX;
  __syncthreads();  // the scratch is free again
  return r;
}

// exclusive sum of the 256 chunk totals; sp: [2][LM_THREADS]
__device__ __forceinline__ long long sum_carry(long long v, int idx, long long* sp) {
  int cur = 0;
  sp[idx] = v;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < LM_THREADS; o <<= 1) {
    const long long s = sp[cur * LM_THREADS + idx] + (idx >= o ? sp[cur * LM_THREADS + idx - o] : 0ll);
    cur ^= 1;
    sp[cur * LM_THREADS + idx] = s;
    __syncthreads();
  }
  const long long r = sp[cur * LM_THREADS + idx] - v;
  __syncthreads();
  return r;
}

// words of q a tile stages: j = t0 - (W - 1) .. t0 + T + W - 1
__host__ __device__ __forceinline__ int limit_span(int W) { return LM_T + 2 * W - 1; }
// dynamic LDS: q (an even count of words), then the prefix minima, later the T + W prefix sums in their place
__host__ __device__ __forceinline__ size_t limit_lds_bytes(int W) {
  return (size_t)((limit_span(W) + 1) & ~1) * sizeof(int) + (size_t)(LM_T + W) * sizeof(long long);
}

// One limiter tile: the samples [t0, min(t0 + LM_T, i_end)) of the row (x, e)[0 .. len), t0 < len, at the gain g
// (live: the row is levelled at all) into y[i] = the output of sample t0 + i, zero from len on, and the smallest s
// of them into *tmin. Of e only [t0 - (W - 1), t0 + LM_T + W - 1] below j_end <= len is read, 2^30 in place of the
// rest; a sample's s reads the W - 1 words of q to each side of it, so j_end >= min(len, i_end + W - 1) gives every
// written sample the whole row's bits. Minimum and sum are integer: the same bits from any origin t0.
__device__ __forceinline__ void limit_tile(const float* __restrict__ x, const float* __restrict__ e, int len, float g,
                                           bool live, float c32, int W, int t0, int i_end, int j_end,
                                           float* __restrict__ y, float* __restrict__ tmin) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) int lq[];
  __shared__ __attribute__((aligned(8))) int scratch[4 * LM_THREADS];  // sv, sf [2][256] or sp [2][256]
  __shared__ float smin[LM_THREADS / 64];
  const int tid = threadIdx.x;
  const int N = limit_span(W);   // staged words of q
  const int M = LM_T + W - 1;    // windows m[u], u < M: the window of u starts at sample t0 - (W - 1) + u
  int* q = lq;
  int* pre = lq + ((N + 1) & ~1);
  long long* Pe = (long long*)pre;  // M + 1 exclusive prefix sums of m, once the prefix minima are spent
  int* sv = scratch;
  int* sf = scratch + 2 * LM_THREADS;

  const int j0 = t0 - (W - 1);
  for (int u = tid; u < N; u += LM_THREADS) {
    const int j = j0 + u;
    int v = LM_ONE;
    if (live && j >= 0 && j < j_end) {
      const float a = g * e[j];
      if (a > c32) v = (int)((c32 / a) * 1073741824.f);  // false for a NaN; a = inf: 0
    }
    q[u] = v;
  }
  __syncthreads();

  const int C = ((N + LM_THREADS - 1) / LM_THREADS) | 1;  // words per thread, odd
  const int u0 = min(tid * C, N), u1 = min(u0 + C, N);
  {  // prefix minima inside blocks of W
    int run = INT_MAX, fb = u1;          // fb: the first block start inside the chunk
    int nb = ((u0 + W - 1) / W) * W;     // the next block start
    for (int u = u0; u < u1; ++u) {
      if (u == nb) {
        if (fb == u1) fb = u;
        run = INT_MAX;
        nb += W;
      }
      run = min(run, q[u]);
      pre[u] = run;
    }
    const int carry = seg_min_carry(run, fb < u1, tid, sv, sf);
    for (int u = u0; u < fb; ++u) pre[u] = min(pre[u], carry);
  }
  {  // suffix minima inside the same blocks, in place of q: the mirror image
    int run = INT_MAX, lb = u0 - 1;      // lb: the last block end inside the chunk
    int nb = (u1 / W) * W - 1;           // the next block end going down
    for (int u = u1 - 1; u >= u0; --u) {
      if (u == nb) {
        if (lb == u0 - 1) lb = u;
        run = INT_MAX;
        nb -= W;
      }
      run = min(run, q[u]);
      q[u] = run;
    }
    const int carry = seg_min_carry(run, lb >= u0, LM_THREADS - 1 - tid, sv, sf);
    for (int u = u1 - 1; u > lb; --u) q[u] = min(q[u], carry);
  }
  __syncthreads();

  long long tot = 0;
  const int um = min(u1, M);
  for (int u = u0; u < um; ++u) {  // u + W - 1 <= N - 2
    const int mv = min(q[u], pre[u + W - 1]);
    q[u] = mv;
    tot += mv;
  }
  long long acc = sum_carry(tot, tid, (long long*)scratch);  // every thread is past its reads of pre
  for (int u = u0; u < min(u1, M + 1); ++u) {                // M + 1 <= N
    Pe[u] = acc;
    if (u < M) acc += q[u];
  }
  __syncthreads();

  const double den = (double)((long long)W << 30);
  float mn = 1.f;
#pragma unroll 2
  for (int k = 0; k < LM_T / LM_THREADS; ++k) {
    const int i = k * LM_THREADS + tid;
    const int gi = t0 + i;
    if (gi >= i_end) break;
    float o = 0.f;
    if (gi < len) {
      const long long S = Pe[i + W] - Pe[i];  // the windows u = i .. i + W - 1 hold sample t0 + i
      const float s = (float)((double)S / den);
      const float t = g * x[gi];
      o = t * s;
      mn = fminf(mn, s);
    }
    y[i] = o;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
  if ((tid & 63) == 0) smin[tid >> 6] = mn;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < LM_THREADS / 64; ++k) mn = fminf(mn, smin[k]);
    *tmin = mn;
  }
}

__global__ __launch_bounds__(LM_THREADS) void limit_kernel(const float* __restrict__ audio,
                                                           const float* __restrict__ env, int L,
                                                           const int* __restrict__ lens,
                                                           const float* __restrict__ peak,
                                                           const double* __restrict__ meansq,
                                                           const float* __restrict__ gain_in, double level, float c32,
                                                           int W, float* __restrict__ out, int nT,
                                                           float* __restrict__ tmin) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int t0 = blockIdx.x * LM_T;  // < L <= LM_MAX_L
  const int len = utt_len(lens, b, 1, L);
  float* y = out + (size_t)b * L + t0;
  if (t0 >= len) {  // the final pass reads the minima of live tiles only
    for (int i = tid; i < LM_T && t0 + i < L; i += LM_THREADS) y[i] = 0.f;
    return;
  }
  bool live;
  const float g = limit_gain(peak, meansq, gain_in, b, level, live);
  limit_tile(audio + (size_t)b * L, env + (size_t)b * L, len, g, live, c32, W, t0, L, len, y,
             tmin + (size_t)b * nT + blockIdx.x);
}

// mt_limit_range: the tiles count from i_lo; out is [B][cnt], the row's gain is gain[b] as it stands
__global__ __launch_bounds__(LM_THREADS) void limit_range_kernel(const float* __restrict__ audio,
                                                                 const float* __restrict__ env, int L,
                                                                 const int* __restrict__ lens,
                                                                 const float* __restrict__ gain, float c32, int W,
                                                                 int i_lo, int cnt, float* __restrict__ out, int nT,
                                                                 float* __restrict__ tmin) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int len = utt_len(lens, b, 1, L);
  const int d0 = blockIdx.x * LM_T;                 // < cnt
  const long long t0 = (long long)i_lo + d0;        // < i_lo + cnt < 2^31 - 4 LM_T
  float* y = out + (size_t)b * cnt + d0;
  if (t0 >= len) {  // the final pass reads the minima of live tiles only
    for (int i = tid; i < LM_T && d0 + i < cnt; i += LM_THREADS) y[i] = 0.f;
    return;
  }
  const int i_end = i_lo + cnt;
  const int j_end = (int)min((long long)len, (long long)i_end + W - 1);
  limit_tile(audio + (size_t)b * L, env + (size_t)b * L, len, gain[b], true, c32, W, (int)t0, i_end, j_end, y,
             tmin + (size_t)b * nT + blockIdx.x);
}

__global__ __launch_bounds__(LM_THREADS) void limit_final_kernel(const float* __restrict__ tmin, int L,
                                                                 const int* __restrict__ lens,
                                                                 const float* __restrict__ peak,
                                                                 const double* __restrict__ meansq,
                                                                 const float* __restrict__ gain_in, double level,
                                                                 int nT, float* __restrict__ reduction,
                                                                 float* __restrict__ gain_out) {
  __shared__ float smin[LM_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = utt_len(lens, b, 1, L);
  const int nt = (len + LM_T - 1) / LM_T;  // <= nT
  float mn = 1.f;
  for (int t = tid; t < nt; t += LM_THREADS) mn = fminf(mn, tmin[(size_t)b * nT + t]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
  if ((tid & 63) == 0) smin[tid >> 6] = mn;
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int k = 1; k < LM_THREADS / 64; ++k) mn = fminf(mn, smin[k]);
  bool live;
  reduction[b] = mn;
  gain_out[b] = limit_gain(peak, meansq, gain_in, b, level, live);
}

// the running minimum of a stream: reduction[b] = min(reduction[b], the minima of the range's live tiles), and the
// row's count of outputs in the range
__global__ __launch_bounds__(LM_THREADS) void limit_range_final_kernel(const float* __restrict__ tmin, int L,
                                                                       const int* __restrict__ lens, int nT, int i_lo,
                                                                       int cnt, float* __restrict__ reduction,
                                                                       int* __restrict__ out_cnt) {
  __shared__ float smin[LM_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = utt_len(lens, b, 1, L);
  const int n = (int)min(max((long long)len - i_lo, 0ll), (long long)cnt);  // outputs of the range inside the row
  const int nt = (n + LM_T - 1) / LM_T;                                     // <= nT
  float mn = 1.f;
  for (int t = tid; t < nt; t += LM_THREADS) mn = fminf(mn, tmin[(size_t)b * nT + t]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
  if ((tid & 63) == 0) smin[tid >> 6] = mn;
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int k = 1; k < LM_THREADS / 64; ++k) mn = fminf(mn, smin[k]);
  reduction[b] = fminf(reduction[b], mn);
  out_cnt[b] = n;
}

// ---- host side -----------------------------------------------------------------------------------------------

static bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
  return p < q + b_bytes && q < p + a_bytes;
}
static bool overlaps(const void* a, const void* b, size_t bytes) { return overlaps(a, bytes, b, bytes); }

static int limiter_shape_check(const char* what, int B, int L) {
  MT_REQUIRE(B > 0 && B <= AU_MAXB && L > 0 && L <= LM_MAX_L, "%s: B %d (1..%d), L %d (1..%d)", what, B, AU_MAXB, L,
             LM_MAX_L);
  return 0;
}

size_t peak_envelope_workspace_bytes() { return resample_table_floats(LM_MAX_HALF, 4) * sizeof(float); }

// the checks both envelope entry points share, then the table re-order; i_lo < 0: the whole rows
static int peak_envelope_launch(const char* what, const float* audio, int B, int L, const int* lens,
                                const float* taps, int half, int i_lo, int cnt, float* env, void* ws,
                                size_t ws_bytes, hipStream_t st) {
  MT_REQUIRE(half >= 1 && half <= LM_MAX_HALF, "%s: filter half-length %d outside 1..%d", what, half, LM_MAX_HALF);
  MT_REQUIRE(audio && taps && env, "%s: null argument", what);
  MT_REQUIRE(!overlaps(audio, env, (size_t)B * L * sizeof(float)), "%s: env overlaps audio", what);
  MT_REQUIRE(ws && ws_bytes >= peak_envelope_workspace_bytes() && ((uintptr_t)ws & 15) == 0,
             "%s: workspace too small or not 16-byte aligned", what);
  const int Q = resample_taps_per_phase(half, 4);
  const size_t tabN = resample_table_floats(half, 4);
  float* tab = (float*)ws;
  int r0 = 0;
  const int rc = resample_table_launch(taps, half, 4, 1, tab, &r0, st);
  if (rc != 0) return rc;
  const size_t lds = (tabN + (size_t)(3 + LM_ENV_N - 1) / 4 + Q) * sizeof(float);  // table + the widest input span
  if (i_lo < 0)
    hipLaunchKernelGGL(peak_envelope_kernel, dim3((L + LM_ENV_T - 1) / LM_ENV_T, B), dim3(LM_THREADS), lds, st, audio,
                       L, lens, (const float*)tab, (int)tabN, half, Q, r0, env);
  else
    hipLaunchKernelGGL(peak_envelope_range_kernel, dim3((cnt + LM_ENV_T - 1) / LM_ENV_T, B), dim3(LM_THREADS), lds,
                       st, audio, L, lens, (const float*)tab, (int)tabN, half, Q, r0, i_lo, cnt, env);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

int peak_envelope(const float* audio, int B, int L, const int* lens, const float* taps, int half, float* env, void* ws,
                  size_t ws_bytes, hipStream_t st) {
  if (limiter_shape_check("peak_envelope", B, L) != 0) return -1;
  return peak_envelope_launch("peak_envelope", audio, B, L, lens, taps, half, -1, 0, env, ws, ws_bytes, st);
}

// a range [i_lo, i_lo + cnt) of samples: the tiles' origins and what they stage stay inside 32 bits
static int limiter_range_check(const char* what, int i_lo, int cnt) {
  MT_REQUIRE(i_lo >= 0 && cnt >= 1 && (long long)i_lo + cnt < (1ll << 31) - 4 * LM_T,
             "%s: samples [%d, %d + %d) (i_lo >= 0, cnt >= 1, i_lo + cnt < 2^31 - %d)", what, i_lo, i_lo, cnt,
             4 * LM_T);
  return 0;
}

int peak_envelope_range(const float* audio, int B, int L, const int* lens, const float* taps, int half, int i_lo,
                        int cnt, float* env, void* ws, size_t ws_bytes, hipStream_t st) {
  if (limiter_shape_check("peak_envelope_range", B, L) != 0) return -1;
  if (limiter_range_check("peak_envelope_range", i_lo, cnt) != 0) return -1;
  return peak_envelope_launch("peak_envelope_range", audio, B, L, lens, taps, half, i_lo, cnt, env, ws, ws_bytes, st);
}

static int limit_window_check(int W) {
  MT_REQUIRE(W >= 1 && W <= LM_MAX_W, "limit: window of %d samples outside 1..%d", W, LM_MAX_W);
  return 0;
}

size_t limit_workspace_bytes(int B, int L, int W) {
  if (limiter_shape_check("limit", B, L) != 0 || limit_window_check(W) != 0) return 0;
  return (size_t)B * (((size_t)L + LM_T - 1) / LM_T) * sizeof(float);
}

int limit(const float* audio, const float* env, int B, int L, const int* lens, const float* peak,
          const double* meansq, const float* gain_in, double level, double ceiling, int W, float* out,
          float* reduction, float* gain_out, void* ws, size_t ws_bytes, hipStream_t st) {
  if (limiter_shape_check("limit", B, L) != 0 || limit_window_check(W) != 0) return -1;
  MT_REQUIRE(isfinite(level) && level > 0.0, "limit: level %g is not a finite positive number", level);
  MT_REQUIRE(isfinite(ceiling) && ceiling > 0.0 && (float)ceiling > 0.f && isfinite((float)ceiling),
             "limit: ceiling %g is not a finite positive fp32 amplitude", ceiling);
  MT_REQUIRE(audio && env && peak && meansq && out && reduction && gain_out, "limit: null argument");
  MT_REQUIRE(!overlaps(audio, out, (size_t)B * L * sizeof(float)) && !overlaps(env, out, (size_t)B * L * sizeof(float)),
             "limit: out overlaps audio or env (never in place)");
  MT_REQUIRE(ws && ws_bytes >= limit_workspace_bytes(B, L, W) && ((uintptr_t)ws & 15) == 0,
             "limit: workspace too small or not 16-byte aligned");
  const int nT = (L + LM_T - 1) / LM_T;
  float* tmin = (float*)ws;
  hipLaunchKernelGGL(limit_kernel, dim3(nT, B), dim3(LM_THREADS), limit_lds_bytes(W), st, audio, env, L, lens, peak,
                     meansq, gain_in, level, (float)ceiling, W, out, nT, tmin);
  MT_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(limit_final_kernel, dim3(B), dim3(LM_THREADS), 0, st, (const float*)tmin, L, lens, peak, meansq,
                     gain_in, level, nT, reduction, gain_out);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

static int limit_range_count_check(int B, int cnt) {
  MT_REQUIRE(B > 0 && B <= AU_MAXB && cnt >= 1, "limit_range: B %d (1..%d), cnt %d (>= 1)", B, AU_MAXB, cnt);
  return 0;
}

size_t limit_range_workspace_bytes(int B, int cnt, int W) {
  if (limit_range_count_check(B, cnt) != 0 || limit_window_check(W) != 0) return 0;
  return (size_t)B * (((size_t)cnt + LM_T - 1) / LM_T) * sizeof(float);
}

int limit_range(const float* audio, const float* env, int B, int L, const int* lens, const float* gain,
                double ceiling, int W, int i_lo, int cnt, float* out, int* out_cnt, float* reduction, void* ws,
                size_t ws_bytes, hipStream_t st) {
  if (limiter_shape_check("limit_range", B, L) != 0 || limit_window_check(W) != 0) return -1;
  if (limiter_range_check("limit_range", i_lo, cnt) != 0) return -1;
  MT_REQUIRE(isfinite(ceiling) && ceiling > 0.0 && (float)ceiling > 0.f && isfinite((float)ceiling),
             "limit_range: ceiling %g is not a finite positive fp32 amplitude", ceiling);
  MT_REQUIRE(audio && env && gain && out && out_cnt && reduction, "limit_range: null argument");
  const size_t in_bytes = (size_t)B * L * sizeof(float), out_bytes = (size_t)B * cnt * sizeof(float);
  MT_REQUIRE(!overlaps(audio, in_bytes, out, out_bytes) && !overlaps(env, in_bytes, out, out_bytes),
             "limit_range: out overlaps audio or env (never in place)");
  MT_REQUIRE(ws && ws_bytes >= limit_range_workspace_bytes(B, cnt, W) && ((uintptr_t)ws & 15) == 0,
             "limit_range: workspace too small or not 16-byte aligned");
  const int nT = (int)(((long long)cnt + LM_T - 1) / LM_T);
  float* tmin = (float*)ws;
  hipLaunchKernelGGL(limit_range_kernel, dim3(nT, B), dim3(LM_THREADS), limit_lds_bytes(W), st, audio, env, L, lens,
                     gain, (float)ceiling, W, i_lo, cnt, out, nT, tmin);
  MT_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(limit_range_final_kernel, dim3(B), dim3(LM_THREADS), 0, st, (const float*)tmin, L, lens, nT,
                     i_lo, cnt, reduction, out_cnt);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace mt
