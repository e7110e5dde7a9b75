// The per-utterance gain of the output stage: one copy for the encoder (mt_audio.hip) and the limiter
// (mt_limiter.hip, §23), so both form the same bits from the same statistics.
#pragma once
#include <math.h>

#include "mt_common.h"

namespace mt {

enum { NORM_NONE = 0, NORM_PEAK = 1, NORM_RMS = 2 };

// audio_out.gain_ref
__device__ __forceinline__ float gain_of(float peak, double meansq, int normalize, double level, int limit) {
  if (normalize == NORM_NONE || !(peak > 0.f)) return 1.f;
  if (normalize == NORM_PEAK) return (float)(level / (double)peak);
  double g = level / sqrt(meansq);
  if (limit) g = fmin(g, 1.0 / (double)peak);
  return (float)g;
}

}  // namespace mt
