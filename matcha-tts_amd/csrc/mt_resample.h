// The resampler's tile, shared by resample_kernel (mt_audio.hip), which stores the outputs, and
// true_peak_kernel (mt_loudness.hip, §21), which only takes their largest magnitude: one copy of the staging and of
// the per-output fp32 FMA chain, so both see the same bits.
#pragma once
#include "mt_common.h"

namespace mt {

constexpr int RS_THREADS = 256;
constexpr int RS_U = 4;                // outputs a thread carries at once
constexpr int RS_LDS_MAX = 64 * 1024;  // staged variant: table + span within this, else the global-read variant
constexpr int AU_MAXB = 65535;         // grid.y

__device__ __forceinline__ int utt_len(const int* lens, int b, int lmul, int L) {
  if (!lens) return L;
  const long long n = (long long)lens[b] * lmul;
  return (int)(n < 0 ? 0 : (n > L ? L : n));
}

// Outputs m0 .. m0 + nrow of one utterance x[0 .. len), of which the first nt lie inside it (nt >= 1): sink(j, v) is
// called once for every j < nrow with v = y[m0 + j], 0 for j >= nt. tab: the re-ordered table (resample_table_kernel),
// r0 the column of output 0. STAGED: lds holds tabN floats of table, then the tile's input span.
template <bool STAGED, class Sink>
__device__ __forceinline__ void resample_tile(const float* __restrict__ x, int len, const float* __restrict__ tab,
                                              int tabN, int half, int up, int down, int Q, int r0, int m0, int nt,
                                              int nrow, float* lds, Sink sink) {
  const int tid = threadIdx.x;
  // output m0 + j reads x[k0 + (rem0 + j down) / up - q]; kS is the first sample any output of the tile reads
  const long long c0 = half + (long long)m0 * down;
  const long long k0 = c0 / up;
  const int rem0 = (int)(c0 - k0 * up);
  const long long kS = k0 - (Q - 1);
  float* xl = lds + tabN;  // STAGED: lds = table [Q][up] (tabN floats), then the tile's input span from kS on
  if (STAGED) {
    for (int i = tid * 4; i < tabN; i += RS_THREADS * 4) *(f32x4*)(lds + i) = *(const f32x4*)(tab + i);
    const int span = (rem0 + (nt - 1) * down) / up + Q;
    for (int i = tid; i < span; i += RS_THREADS) {
      const long long k = kS + i;
      xl[i] = (k >= 0 && k < len) ? x[k] : 0.f;
    }
    __syncthreads();
  }
  const int rbase = (int)((r0 + (long long)m0) % up);
  if (STAGED) {
    // RS_U outputs per thread at a time: independent chains keep RS_U pairs of LDS reads in flight per tap; each
    // chain is still q = 0 .. Q - 1 on its own accumulator. An output past nt runs on output 0's operands, unused.
    for (int j0 = tid; j0 < nrow; j0 += RS_THREADS * RS_U) {
      float acc[RS_U];
      int ti[RS_U], xi[RS_U];
#pragma unroll
      for (int u = 0; u < RS_U; ++u) {
        const int j = j0 + u * RS_THREADS;
        const int jj = j < nt ? j : 0;
        xi[u] = (rem0 + jj * down) / up + (Q - 1);  // x[k0 + (rem0 + j down) / up] relative to kS
        ti[u] = (rbase + jj) % up;
        acc[u] = 0.f;
      }
      for (int q = 0; q < Q; ++q) {
#pragma unroll
        for (int u = 0; u < RS_U; ++u) acc[u] = __builtin_fmaf(lds[q * up + ti[u]], xl[xi[u] - q], acc[u]);
      }
#pragma unroll
      for (int u = 0; u < RS_U; ++u) {
        const int j = j0 + u * RS_THREADS;
        if (j < nrow) sink(j, j < nt ? acc[u] : 0.f);
      }
    }
  } else {
    for (int j = tid; j < nrow; j += RS_THREADS) {
      float acc = 0.f;
      if (j < nt) {
        const int i0 = (rem0 + j * down) / up + (Q - 1);
        const int r = (rbase + j) % up;
        for (int q = 0; q < Q; ++q) {
          const long long k = kS + i0 - q;
          const float xv = (k >= 0 && k < len) ? x[k] : 0.f;
          acc = __builtin_fmaf(tab[(size_t)q * up + r], xv, acc);
        }
      }
      sink(j, acc);
    }
  }
}

// host side (mt_audio.hip): the table of a factor and its re-order into `tab` on the stream
int resample_taps_per_phase(int half, int up);
size_t resample_table_floats(int half, int up);
// launches resample_table_kernel (taps [up][Q] -> tab, resample_table_floats(half, up) floats, 16-byte aligned) and
// returns the column of output 0 in *r0
int resample_table_launch(const float* taps, int half, int up, int down, float* tab, int* r0, hipStream_t st);

}  // namespace mt
