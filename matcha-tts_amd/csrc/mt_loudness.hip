// Programme loudness (ITU-R BS.1770 K-weighting, 400 ms blocks, two gates) and true peak of every row of a ragged
// batch on gfx950 (matcha_hip/loudness.py is the same specification on the CPU).
//
// The K-weighting is two biquads in transposed direct form II: a linear recurrence s[i+1] = A s[i] + B x[i],
// y[i] = C s[i] + D x[i] with s in R^4, run in parallel along time as a chunked scan in fp64:
//   kw_kernel<false>: one workgroup per (row, tile of KW_TILE = 8192 samples counted from the row's start), one
//     thread per chunk of KW_CH = 32 samples. The tile is staged into LDS with coalesced loads (zero from the row's
//     length on), thread c at words c * 33 ..: an odd stride, 32 lanes on 32 banks. Each thread runs its chunk from a
//     zero state; the end states e_c combine through LDS by s_in[c+1] = A^32 s_in[c] + e_c, in two levels (16 threads
//     each walk 16 chunks, one thread walks the 16 groups with A^512), to the tile's end state from a zero entry.
//   kw_kernel<true>: the same up to the e_c, while thread 255 walks the end states of the row's earlier tiles
//     (S[t+1] = A^8192 S[t] + E[t], at most L / 8192 steps) to the tile's true entry state; the scan then yields every
//     chunk's true entry state, each thread reruns its chunk from it and sums y^2 in fp64 in sample order, split where
//     a hop boundary (hop >= 32: at most one) cuts the chunk: two partials per chunk.
//   loudness_gate_kernel: one workgroup per row. A thread per hop sums that hop's partials in sample order; a thread
//     per block forms z_j from four consecutive hops; thread 0 runs both gates in block order, one IEEE operation at
//     a time (contraction off), all in the energy domain: no log or pow in a decision.
//   Chunks, tiles and every summation order count from the row's first sample and depend on nothing else: a row's bits
//   do not depend on B, L, the row's index or what the padding holds. No atomics.
// true_peak_kernel: the resampler's tile (mt_resample.h) at 4/1 with a sink that keeps max |.| instead of storing;
//   true_peak_final_kernel takes the row's maximum over its tiles and folds the sample peak in.
#include <math.h>

#include "mt_common.h"
#include "mt_resample.h"

namespace mt {

constexpr int KW_CH = 32;                      // samples per chunk (runtime.LOUDNESS_CHUNK)
constexpr int KW_THREADS = 256;                // chunks per tile
constexpr int KW_TILE = KW_CH * KW_THREADS;    // samples per tile (runtime.LOUDNESS_TILE)
constexpr int KW_GRP = 16;                     // chunks per scan group, and groups per tile
constexpr int KW_MAX_L = 1 << 30;
constexpr int KW_MAX_HOP = 1 << 24;
constexpr int TP_TN = 2048;                    // 4x outputs per true-peak tile
constexpr int TP_MAX_HALF = 1024;              // taps: at most 2 * 1024 + 1 (256 zero crossings per side)
constexpr int TP_MAX_L = (1 << 29) - TP_TN;
static_assert(KW_GRP * KW_GRP == KW_THREADS, "two scan levels");

struct KwParams {
  double c[10];   // b1[0..2], a1[1..2], b2[0..2], a2[1..2]
  double aC[16];  // A^KW_CH, row-major
  double aG[16];  // A^(KW_CH KW_GRP)
  double aT[16];  // A^KW_TILE
};

// one sample through both biquads (transposed direct form II): the state is s[0..1] of stage 1, s[2..3] of stage 2
__host__ __device__ __forceinline__ double kw_step(const double* c, double* s, double x) {
  const double y1 = c[0] * x + s[0];
  s[0] = s[1] + c[1] * x - c[3] * y1;
  s[1] = c[2] * x - c[4] * y1;
  const double y = c[5] * y1 + s[2];
  s[2] = s[3] + c[6] * y1 - c[8] * y;
  s[3] = c[7] * y1 - c[9] * y;
  return y;
}

// v = M v + e
__device__ __forceinline__ void kw_carry(const double* m, double* v, const double* e) {
  double r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = m[4 * i] * v[0] + m[4 * i + 1] * v[1] + m[4 * i + 2] * v[2] + m[4 * i + 3] * v[3] + e[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = r[i];
}

// chunk c's 4 doubles in the LDS state array: 2 doubles of padding per group, so the 16 threads that walk one group
// each (stride 66 doubles) read distinct banks
__device__ __forceinline__ int kw_slot(int c) { return c * 4 + (c / KW_GRP) * 2; }

template <bool FINAL>
__global__ __launch_bounds__(KW_THREADS) void kw_kernel(const float* __restrict__ audio, int L,
                                                        const int* __restrict__ lens, const KwParams p, int nT,
                                                        double* __restrict__ tile_state, int hop,
                                                        double* __restrict__ part) {
  __shared__ float xs[KW_TILE + KW_TILE / 32];
  __shared__ __attribute__((aligned(16))) double st[KW_THREADS * 4 + KW_GRP * 2];
  __shared__ double grp[KW_GRP][4];
  __shared__ double ent[4];
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int len = utt_len(lens, b, 1, L);
  const int i0 = t * KW_TILE;  // < L <= 2^30
  if (i0 >= len) return;       // later tiles of the row read the end states of live tiles only
  const float* x = audio + (size_t)b * L;
#pragma unroll 8
  for (int k = 0; k < KW_CH; ++k) {
    const int i = tid + k * KW_THREADS;
    xs[i + (i >> 5)] = i0 + i < len ? x[i0 + i] : 0.f;
  }
  if (FINAL && tid == KW_THREADS - 1) {
    // the tile's entry state from the row's earlier tiles, in tile order
    double S[4] = {0.0, 0.0, 0.0, 0.0};
    const double* E = tile_state + (size_t)b * nT * 4;
    for (int u = 0; u < t; ++u) kw_carry(p.aT, S, E + (size_t)u * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) ent[i] = S[i];
  }
  __syncthreads();
  const float* xc = xs + tid * (KW_CH + 1);
  {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
    for (int k = 0; k < KW_CH; ++k) kw_step(p.c, s, (double)xc[k]);
    double* o = st + kw_slot(tid);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = s[i];
  }
  __syncthreads();
  if (tid < KW_GRP) {  // the group's end state from a zero entry
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < KW_GRP; ++j) kw_carry(p.aC, v, st + kw_slot(tid * KW_GRP + j));
#pragma unroll
    for (int i = 0; i < 4; ++i) grp[tid][i] = v[i];
  }
  __syncthreads();
  if (tid == 0) {  // every group's entry state; S ends as the tile's end state
    double S[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) S[i] = FINAL ? ent[i] : 0.0;
    for (int g = 0; g < KW_GRP; ++g) {
      double e[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        e[i] = grp[g][i];
        grp[g][i] = S[i];
      }
      kw_carry(p.aG, S, e);
    }
    if (!FINAL) {
      double* E = tile_state + ((size_t)b * nT + t) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) E[i] = S[i];
    }
  }
  if (!FINAL) return;
  __syncthreads();
  if (tid < KW_GRP) {  // every chunk's entry state
    double v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = grp[tid][i];
    for (int j = 0; j < KW_GRP; ++j) {
      double* o = st + kw_slot(tid * KW_GRP + j);
      double e[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        e[i] = o[i];
        o[i] = v[i];
      }
      kw_carry(p.aC, v, e);
    }
  }
  __syncthreads();
  const int g0 = i0 + tid * KW_CH;  // the chunk's first sample in the row
  if (g0 >= len) return;
  const long long nb = ((long long)(g0 / hop) + 1) * hop;  // the next hop boundary
  const int n0 = (int)(nb - g0 < KW_CH ? nb - g0 : KW_CH);  // samples of the chunk before it
  const int nv = min(KW_CH, len - g0);                      // samples of the chunk inside the row
  double s[4];
  {
    const double* o = st + kw_slot(tid);
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = o[i];
  }
  double p0 = 0.0, p1 = 0.0;
#pragma unroll 8
  for (int k = 0; k < KW_CH; ++k) {
    const double y = kw_step(p.c, s, (double)xc[k]);
    const double yy = y * y;
    if (k < nv) {
      if (k < n0)
        p0 += yy;
      else
        p1 += yy;
    }
  }
  double* o = part + ((size_t)b * nT * KW_THREADS + (size_t)(g0 / KW_CH)) * 2;
  o[0] = p0;
  o[1] = p1;
}

// blocks of a row of len samples
__host__ __device__ __forceinline__ int kw_blocks(long long len, long long hop) {
  if (len <= 0) return 0;
  return len >= 4 * hop ? (int)((len - 4 * hop) / hop + 1) : 1;
}

__global__ __launch_bounds__(256) void loudness_gate_kernel(int L, const int* __restrict__ lens, int nT, int hop,
                                                            double gate_abs, const double* __restrict__ part,
                                                            double* __restrict__ hops, int nHcap,
                                                            double* __restrict__ zbuf, int Jcap,
                                                            int* __restrict__ nblocks, double* __restrict__ energy) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = utt_len(lens, b, 1, L);
  const int J = kw_blocks(len, hop);
  const bool whole = len >= 4ll * hop;
  const int nH = whole ? J + 3 : (len + hop - 1) / hop;  // hops that enter a block: complete ones, or all (<= 4)
  const double* pr = part + (size_t)b * nT * KW_THREADS * 2;
  double* H = hops + (size_t)b * nHcap;
  double* z = zbuf + (size_t)b * Jcap;
  for (int k = tid; k < nH; k += 256) {
    const long long lo = (long long)k * hop;
    const long long hi = lo + hop < len ? lo + hop : len;
    const int cf = (int)(lo / KW_CH), cl = (int)((hi - 1) / KW_CH);
    // the first chunk may begin in the hop before: its second partial is this hop's
    double s = (long long)cf * KW_CH < lo ? pr[(size_t)cf * 2 + 1] : pr[(size_t)cf * 2];
    for (int c = cf + 1; c <= cl; ++c) s += pr[(size_t)c * 2];
    H[k] = s;
  }
  __threadfence_block();
  __syncthreads();
  for (int j = tid; j < Jcap; j += 256) {
    double v = 0.0;
    if (j < J) {
      if (whole) {
        v = (((H[j] + H[j + 1]) + H[j + 2]) + H[j + 3]) / (double)(4ll * hop);
      } else {
        for (int k = 0; k < nH; ++k) v += H[k];
        v = v / (double)len;
      }
    }
    z[j] = v;
  }
  __threadfence_block();
  __syncthreads();
  if (tid != 0) return;
  double s = 0.0;
  int c = 0;
  for (int j = 0; j < J; ++j) {
    const double v = z[j];
    if (v > gate_abs) {
      s += v;
      ++c;
    }
  }
  double E = 0.0;
  if (c > 0) {
    const double rel = 0.1 * (s / (double)c);
    s = 0.0;
    c = 0;
    for (int j = 0; j < J; ++j) {
      const double v = z[j];
      if (v > gate_abs && v > rel) {
        s += v;
        ++c;
      }
    }
    if (c > 0) E = s / (double)c;
  }
  nblocks[b] = J;
  energy[b] = E;
}

__global__ __launch_bounds__(RS_THREADS) void true_peak_kernel(const float* __restrict__ audio, int L,
                                                               const int* __restrict__ lens,
                                                               const float* __restrict__ tab, int tabN, int half,
                                                               int Q, int r0, int nT, float* __restrict__ pmax) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float sm[RS_THREADS];
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int len = utt_len(lens, b, 1, L);
  const int n_out = 4 * len;  // L <= TP_MAX_L
  const int m0 = t * TP_TN;
  if (m0 >= n_out) return;  // the final pass reads the partials of live tiles only
  const int nt = min(TP_TN, n_out - m0);
  float mx = 0.f;
  resample_tile<true>(audio + (size_t)b * L, len, tab, tabN, half, 4, 1, Q, r0, m0, nt, nt, lds,
                      [&mx](int, float v) { mx = fmaxf(mx, fabsf(v)); });
  sm[tid] = mx;
  __syncthreads();
  for (int o = RS_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) sm[tid] = fmaxf(sm[tid], sm[tid + o]);
    __syncthreads();
  }
  if (tid == 0) pmax[(size_t)b * nT + t] = sm[0];
}

__global__ __launch_bounds__(256) void true_peak_final_kernel(const float* __restrict__ pmax, int L,
                                                              const int* __restrict__ lens, int nT,
                                                              const float* __restrict__ sample_peak,
                                                              float* __restrict__ tpeak) {
  __shared__ float sm[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = utt_len(lens, b, 1, L);
  const int nt = (int)((4ll * len + TP_TN - 1) / TP_TN);
  float mx = 0.f;
  for (int t = tid; t < nt; t += 256) mx = fmaxf(mx, pmax[(size_t)b * nT + t]);
  sm[tid] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sm[tid] = fmaxf(sm[tid], sm[tid + o]);
    __syncthreads();
  }
  if (tid == 0) tpeak[b] = sample_peak ? fmaxf(sm[0], sample_peak[b]) : sm[0];
}

// ---- host side -----------------------------------------------------------------------------------------------

static void mat4_mul(const double* a, const double* b, double* o) {
  double r[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
      r[4 * i + j] = s;
    }
  for (int i = 0; i < 16; ++i) o[i] = r[i];
}

// m^(2^n)
static void mat4_pow2(const double* m, int n, double* o) {
  for (int i = 0; i < 16; ++i) o[i] = m[i];
  for (int i = 0; i < n; ++i) mat4_mul(o, o, o);
}

static void kw_params(const double* coef, KwParams* p) {
  for (int i = 0; i < 10; ++i) p->c[i] = coef[i];
  for (int k = 0; k < 4; ++k) {  // column k of A^KW_CH: KW_CH steps of the homogeneous recurrence from e_k
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    s[k] = 1.0;
    for (int i = 0; i < KW_CH; ++i) kw_step(p->c, s, 0.0);
    for (int i = 0; i < 4; ++i) p->aC[4 * i + k] = s[i];
  }
  mat4_pow2(p->aC, 4, p->aG);  // KW_GRP = 2^4
  mat4_pow2(p->aG, 4, p->aT);
}

struct KwLayout {
  size_t nT, nH, J, state, part, hops, zbuf, total;
};
static KwLayout kw_layout(int B, int L, int hop) {
  KwLayout w;
  w.nT = ((size_t)L + KW_TILE - 1) / KW_TILE;
  w.nH = (size_t)L / hop + 4;
  w.J = (size_t)(kw_blocks(L, hop) > 0 ? kw_blocks(L, hop) : 1);
  w.state = 0;
  w.part = w.state + (size_t)B * w.nT * 4 * sizeof(double);
  w.hops = w.part + (size_t)B * w.nT * KW_THREADS * 2 * sizeof(double);
  w.zbuf = w.hops + (size_t)B * w.nH * sizeof(double);
  w.total = w.zbuf + (size_t)B * w.J * sizeof(double);
  return w;
}

static int loudness_shape_check(int B, int L, int hop) {
  MT_REQUIRE(B > 0 && B <= AU_MAXB && L > 0 && L <= KW_MAX_L, "loudness: B %d (1..%d), L %d (1..%d)", B, AU_MAXB, L,
             KW_MAX_L);
  MT_REQUIRE(hop >= KW_CH && hop <= KW_MAX_HOP, "loudness: hop %d outside %d..%d samples", hop, KW_CH, KW_MAX_HOP);
  return 0;
}

size_t loudness_workspace_bytes(int B, int L, int hop) {
  if (loudness_shape_check(B, L, hop) != 0) return 0;
  return kw_layout(B, L, hop).total;
}

int loudness(const float* audio, int B, int L, const int* lens, const double* coef, int hop, double gate_abs,
             double* z, int Jcap, int* nblocks, double* energy, void* ws, size_t ws_bytes, hipStream_t st) {
  if (loudness_shape_check(B, L, hop) != 0) return -1;
  MT_REQUIRE(audio && coef && nblocks && energy, "loudness: null argument");
  for (int i = 0; i < 10; ++i) MT_REQUIRE(isfinite(coef[i]), "loudness: coefficient %d is not finite", i);
  MT_REQUIRE(isfinite(gate_abs) && gate_abs >= 0.0, "loudness: absolute gate %g is not a finite energy", gate_abs);
  const KwLayout w = kw_layout(B, L, hop);
  MT_REQUIRE(!z || (Jcap >= 1 && (size_t)Jcap >= w.J), "loudness: Jcap %d < %zu blocks of a row of %d samples", Jcap,
             w.J, L);
  MT_REQUIRE(ws && ws_bytes >= w.total && ((uintptr_t)ws & 15) == 0,
             "loudness: workspace too small or not 16-byte aligned");
  KwParams p;
  kw_params(coef, &p);
  char* base = (char*)ws;
  double* state = (double*)(base + w.state);
  double* part = (double*)(base + w.part);
  double* hops = (double*)(base + w.hops);
  double* zb = z ? z : (double*)(base + w.zbuf);
  const int Jc = z ? Jcap : (int)w.J;
  const dim3 grid((unsigned)w.nT, B);
  hipLaunchKernelGGL(kw_kernel<false>, grid, dim3(KW_THREADS), 0, st, audio, L, lens, p, (int)w.nT, state, hop, part);
  MT_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(kw_kernel<true>, grid, dim3(KW_THREADS), 0, st, audio, L, lens, p, (int)w.nT, state, hop, part);
  MT_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(loudness_gate_kernel, dim3(B), dim3(256), 0, st, L, lens, (int)w.nT, hop, gate_abs,
                     (const double*)part, hops, (int)w.nH, zb, Jc, nblocks, energy);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

static size_t tp_table_bytes() { return resample_table_floats(TP_MAX_HALF, 4) * sizeof(float); }

static int true_peak_shape_check(int B, int L) {
  MT_REQUIRE(B > 0 && B <= AU_MAXB && L > 0 && L <= TP_MAX_L, "true_peak: B %d (1..%d), L %d (1..%d)", B, AU_MAXB, L,
             TP_MAX_L);
  return 0;
}

size_t true_peak_workspace_bytes(int B, int L) {
  if (true_peak_shape_check(B, L) != 0) return 0;
  const size_t nT = (4 * (size_t)L + TP_TN - 1) / TP_TN;
  return tp_table_bytes() + (size_t)B * nT * sizeof(float);
}

int true_peak(const float* audio, int B, int L, const int* lens, const float* taps, int half,
              const float* sample_peak, float* tpeak, void* ws, size_t ws_bytes, hipStream_t st) {
  if (true_peak_shape_check(B, L) != 0) return -1;
  MT_REQUIRE(half >= 1 && half <= TP_MAX_HALF, "true_peak: filter half-length %d outside 1..%d", half, TP_MAX_HALF);
  MT_REQUIRE(audio && taps && tpeak, "true_peak: null argument");
  MT_REQUIRE(ws && ws_bytes >= true_peak_workspace_bytes(B, L) && ((uintptr_t)ws & 15) == 0,
             "true_peak: workspace too small or not 16-byte aligned");
  const int nT = (int)((4 * (size_t)L + TP_TN - 1) / TP_TN);
  const int Q = resample_taps_per_phase(half, 4);
  const size_t tabN = resample_table_floats(half, 4);
  float* tab = (float*)ws;
  float* pmax = (float*)((char*)ws + tp_table_bytes());
  int r0 = 0;
  const int rc = resample_table_launch(taps, half, 4, 1, tab, &r0, st);
  if (rc != 0) return rc;
  const size_t lds = (tabN + (size_t)(3 + TP_TN - 1) / 4 + Q) * sizeof(float);  // table + the widest input span
  hipLaunchKernelGGL(true_peak_kernel, dim3(nT, B), dim3(RS_THREADS), lds, st, audio, L, lens, (const float*)tab,
                     (int)tabN, half, Q, r0, nT, pmax);
  MT_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(true_peak_final_kernel, dim3(B), dim3(256), 0, st, (const float*)pmax, L, lens, nT, sample_peak,
                     tpeak);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace mt
