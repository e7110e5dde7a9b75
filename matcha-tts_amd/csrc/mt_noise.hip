// Seeded, counter-based Gaussian noise (DESIGN.md "Seeded noise"; CPU specification: matcha_hip/noise.py).
// The value at (seed, channel c, frame t) depends on those three numbers only: Philox4x32-10 keyed by the seed's two
// 32-bit halves on the counter (t, c / 4, 0, 0), its four words turned into two Box-Muller pairs. One thread per
// (utterance, frame, channel quad); nothing is read but the seed and the temperature.
#include "mt_misc.h"

namespace mt {

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// u(x) = (2 * (x >> 9) + 1) * 2^-24: a 24-bit odd integer, exact in fp32, inside [2^-24, 1 - 2^-24]
__device__ __forceinline__ float unit_open(uint32_t x) { return (float)(2u * (x >> 9) + 1u) * 0x1p-24f; }

// channels 4q .. 4q + 3 of frame t: (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1) * temp, r = sqrt(-2 ln u(x_even)),
// a = 2 pi u(x_odd). sincospif takes the exact argument 2 u. Both kernels below call this one function, so a value
// has the same bits in every output layout.
__device__ __forceinline__ f32x4 noise_quad(uint32_t k0, uint32_t k1, uint32_t t, uint32_t q, float temp) {
  uint32_t c0 = t, c1 = q, c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(PHILOX_M0, c0), l0 = PHILOX_M0 * c0;
    const uint32_t h1 = __umulhi(PHILOX_M1, c2), l1 = PHILOX_M1 * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  const float r0 = sqrtf(-2.f * logf(unit_open(c0)));
  const float r1 = sqrtf(-2.f * logf(unit_open(c2)));
  float s0, cs0, s1, cs1;
  sincospif(2.f * unit_open(c1), &s0, &cs0);
  sincospif(2.f * unit_open(c3), &s1, &cs1);
  f32x4 v;
  v[0] = (r0 * cs0) * temp;
  v[1] = (r0 * s0) * temp;
  v[2] = (r1 * cs1) * temp;
  v[3] = (r1 * s1) * temp;
  return v;
}

// z [B][C][T] fp32; consecutive threads walk t, so each of the four channel rows gets coalesced stores
__global__ __launch_bounds__(256) void noise_bct_kernel(const long long* __restrict__ seeds,
                                                        const float* __restrict__ temp, int Q, int T, size_t total,
                                                        float* __restrict__ z) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int t = (int)(i % (size_t)T);
  const size_t bq = i / (size_t)T;
  const int q = (int)(bq % (size_t)Q), b = (int)(bq / (size_t)Q);
  const unsigned long long s = (unsigned long long)seeds[b];
  const f32x4 v = noise_quad((uint32_t)s, (uint32_t)(s >> 32), (uint32_t)t, (uint32_t)q, temp ? temp[b] : 1.f);
  float* o = z + ((size_t)b * (4 * Q) + 4 * q) * T + t;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[(size_t)j * T] = v[j];
}

// the decoder's two workspace layouts in one pass: zm [B][T][80] fp32 and xin [B][T][ld] (element type E) columns
// 0 .. 79, xin holding E's rounding of the fp32 value zm gets. Consecutive threads walk the quads of a frame.
template <class E>
__global__ __launch_bounds__(256) void noise_dec_kernel(const long long* __restrict__ seeds,
                                                        const float* __restrict__ temp, int T, size_t total,
                                                        float* __restrict__ zm, E* __restrict__ xin, int ld) {
  constexpr int Q = 20;  // 80 mel channels
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % Q);
  const size_t bt = i / Q;  // b * T + t
  const int t = (int)(bt % (size_t)T), b = (int)(bt / (size_t)T);
  const unsigned long long s = (unsigned long long)seeds[b];
  const f32x4 v = noise_quad((uint32_t)s, (uint32_t)(s >> 32), (uint32_t)t, (uint32_t)q, temp ? temp[b] : 1.f);
  *reinterpret_cast<f32x4*>(zm + bt * (4 * Q) + 4 * q) = v;
  E* x = xin + bt * (size_t)ld + 4 * q;
  if constexpr (sizeof(E) == 4) {
    *reinterpret_cast<f32x4*>(x) = v;
  } else {
    bf16x4 h;
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = from_f<bf16>(v[j]);
    *reinterpret_cast<bf16x4*>(x) = h;
  }
}

int grid_for(size_t total, const char* what, unsigned* blocks) {
  const size_t nb = (total + 255) / 256;
  MT_REQUIRE(nb <= 0x7fffffffu, "%s: %zu values are more than one launch covers", what, total * 4);
  *blocks = (unsigned)nb;
  return 0;
}

}  // namespace

int noise_fill(const long long* seeds, const float* temp, int B, int C, int T, float* z, hipStream_t st) {
  MT_REQUIRE(B > 0 && T > 0 && C > 0 && C % 4 == 0, "noise_fill: B %d, C %d (a multiple of 4), T %d", B, C, T);
  const size_t total = (size_t)B * (C / 4) * T;
  unsigned blocks;
  if (int rc = grid_for(total, "noise_fill", &blocks)) return rc;
  hipLaunchKernelGGL(noise_bct_kernel, dim3(blocks), dim3(256), 0, st, seeds, temp, C / 4, T, total, z);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

int noise_fill_decoder(int dtype, const long long* seeds, const float* temp, int B, int T, float* zm, void* xin,
                       int ld, hipStream_t st) {
  // 16-byte fp32 / 8-byte bf16 stores at column 4 q of a row: the row stride keeps them aligned
  MT_REQUIRE(B > 0 && T > 0 && ld >= 80 && ld % 4 == 0, "noise_fill_decoder: B %d, T %d, row stride %d", B, T, ld);
  const size_t total = (size_t)B * T * 20;
  unsigned blocks;
  if (int rc = grid_for(total, "noise_fill_decoder", &blocks)) return rc;
  if (dtype == BF16)
    hipLaunchKernelGGL(noise_dec_kernel<bf16>, dim3(blocks), dim3(256), 0, st, seeds, temp, T, total, zm, (bf16*)xin,
                       ld);
  else
    hipLaunchKernelGGL(noise_dec_kernel<float>, dim3(blocks), dim3(256), 0, st, seeds, temp, T, total, zm,
                       (float*)xin, ld);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace mt
