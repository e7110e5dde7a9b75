// One frame of the log-mel featurizer (train_standalone.py:164-201), the body shared by mt_log_mel (mt_featurize.hip:
// a rectangular batch) and mt_log_mel_ragged (mt_audio_in.hip: every row at its own trim edges and gain): the same
// FFT, the same magnitude, the same three-way split of each 513-bin dot product, so both give the same bits for the
// same signal.
#pragma once
#include <math.h>

#include "mt_fft.h"

namespace mt {

constexpr int LM_NFFT = 1024, LM_HOP = 256, LM_NBIN = LM_NFFT / 2 + 1, LM_PAD = (LM_NFFT - LM_HOP) / 2, LM_NMEL = 80;

// frames of a row of n samples: reflect padding needs n > LM_PAD, torch's framing gives (n - 256) / 256 + 1
__host__ __device__ __forceinline__ int logmel_frames(int n) { return n <= LM_PAD ? 0 : (n - LM_HOP) / LM_HOP + 1; }

struct LogMelLds {
  float re[LM_NFFT], im[LM_NFFT], twc[LM_NFFT / 2], tws[LM_NFFT / 2], mag[LM_NBIN], part[3][LM_NMEL];
};

// twc/tws[k] = cos/sin(2 pi k / 1024); once per workgroup, visible after the barrier fft1024 starts with
__device__ __forceinline__ void logmel_twiddles(LogMelLds& s) {
  for (int k = threadIdx.x; k < LM_NFFT / 2; k += 256) {
    float sn, c;
    sincospif(2.f * (float)k / (float)LM_NFFT, &sn, &c);
    s.twc[k] = c;
    s.tws[k] = sn;
  }
}

// Frame f of the signal x(0) .. x(n - 1), reflected at 0 and at n - 1 (n > LM_PAD): emit(m, v) is called by thread m
// < 80 with the frame's value of filter m. Every thread of the 256-thread workgroup must call it. Calls may follow
// each other without a barrier between them: what a call writes first (re, im) the one before it has not read since
// its second-last barrier, and `part` is rewritten only after the next call's barriers.
template <class Sample, class Emit>
__device__ __forceinline__ void logmel_frame(LogMelLds& s, int f, int n, Sample x, const float* __restrict__ basis,
                                             float mean, float stdv, Emit emit) {
  const int tid = threadIdx.x;
  for (int j = tid; j < LM_NFFT; j += 256) {
    int i = f * LM_HOP + j - LM_PAD;  // index into the unpadded signal, reflected at both ends
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    const int r = __brev((unsigned)j) >> (32 - 10);
    s.re[r] = x(i) * hann(j);
    s.im[r] = 0.f;
  }
  fft1024(s.re, s.im, s.twc, s.tws, -1.f);
  for (int k = tid; k < LM_NBIN; k += 256) s.mag[k] = sqrtf(s.re[k] * s.re[k] + s.im[k] * s.im[k] + 1e-9f);
  __syncthreads();
  if (tid < 3 * LM_NMEL) {  // filter m = tid % 80, bins of third tid / 80
    const int m = tid % LM_NMEL, third = tid / LM_NMEL;
    const int k0 = third * 171, k1 = min(LM_NBIN, k0 + 171);
    const float* w = basis + (size_t)m * LM_NBIN;
    float acc = 0.f;
    for (int k = k0; k < k1; ++k) acc = fmaf(w[k], s.mag[k], acc);
    s.part[third][m] = acc;
  }
  __syncthreads();
  if (tid < LM_NMEL) {
    const float acc = (s.part[0][tid] + s.part[1][tid]) + s.part[2][tid];
    emit(tid, (logf(fmaxf(acc, 1e-5f)) - mean) / stdv);
  }
}

}  // namespace mt
