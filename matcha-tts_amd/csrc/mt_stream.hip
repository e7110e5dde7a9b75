// Window gather / scatter for streaming delivery (matcha_hip/stream_plan.py is the specification of
// the windows): a step of the stream cuts one window per live utterance out of a full-length buffer (the mel, the
// stitched vocoder output), runs the ragged vocoder / denoiser on the windows as a batch of their own, and writes the
// samples that became final back into a full-length buffer. Both are plain copies: no arithmetic touches a value.
//
// window_gather_kernel: rows[r][c][w] = src[row_src[r]][c][row_start[r] + w] for w < row_len[r], else 0; one thread
//   per element of rows, neighbouring threads on neighbouring w (coalesced on both sides).
// window_scatter_kernel: dst[row_dst[r]][dst_start[r] + i] = rows[r][crop_from[r] + i] for i < crop_len[r].
// The tables live on the device (a stream uploads the tables of all its steps once), so the host cannot check them:
// an entry outside its buffer is clamped away here, it never turns into an access out of range. A gather of such an
// entry reads as zero, a scatter of it writes nothing.
#include "mt_common.h"
#include "mt_ragged.h"

namespace mt {

constexpr int WG_THREADS = 256;
constexpr int WG_MAXC = 65535;  // grid.y

__global__ __launch_bounds__(WG_THREADS) void window_gather_kernel(const float* __restrict__ src, int Bs, int C,
                                                                   int Ls, const int* __restrict__ row_src,
                                                                   const int* __restrict__ row_start,
                                                                   const int* __restrict__ row_len, int W,
                                                                   float* __restrict__ rows) {
  const int r = blockIdx.z, c = blockIdx.y;
  const int w = blockIdx.x * WG_THREADS + threadIdx.x;
  if (w >= W) return;
  const int b = row_src[r], s = row_start[r];
  const int n = min(row_len[r], W);
  float v = 0.f;
  if (b >= 0 && b < Bs && s >= 0 && w < n) {
    const long long k = (long long)s + w;
    if (k < Ls) v = src[((size_t)b * C + c) * Ls + k];
  }
  rows[((size_t)r * C + c) * W + w] = v;
}

__global__ __launch_bounds__(WG_THREADS) void window_scatter_kernel(const float* __restrict__ rows, int W,
                                                                    const int* __restrict__ row_dst,
                                                                    const int* __restrict__ crop_from,
                                                                    const int* __restrict__ dst_start,
                                                                    const int* __restrict__ crop_len,
                                                                    float* __restrict__ dst, int Bd, int Ld) {
  const int r = blockIdx.y;
  const int i = blockIdx.x * WG_THREADS + threadIdx.x;
  if (i >= W) return;
  const int b = row_dst[r], f = crop_from[r], d = dst_start[r];
  if (b < 0 || b >= Bd || f < 0 || d < 0 || i >= crop_len[r]) return;
  const long long k = (long long)f + i, o = (long long)d + i;
  if (k >= W || o >= Ld) return;
  dst[(size_t)b * Ld + o] = rows[(size_t)r * W + k];
}

int window_gather(const float* src, int Bs, int C, int Ls, const int* row_src, const int* row_start,
                  const int* row_len, int R, int W, float* rows, hipStream_t st) {
  MT_REQUIRE(src && row_src && row_start && row_len && rows, "window_gather: null argument");
  MT_REQUIRE(Bs > 0 && Ls > 0 && C > 0 && C <= WG_MAXC, "window_gather: source [%d][%d][%d]", Bs, C, Ls);
  MT_REQUIRE(R > 0 && R <= RAG_MAXB, "window_gather: %d window rows (1..%d)", R, RAG_MAXB);
  MT_REQUIRE(W > 0, "window_gather: window of %d", W);
  hipLaunchKernelGGL(window_gather_kernel, dim3((W + WG_THREADS - 1) / WG_THREADS, C, R), dim3(WG_THREADS), 0, st,
                     src, Bs, C, Ls, row_src, row_start, row_len, W, rows);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

int window_scatter(const float* rows, int R, int W, const int* row_dst, const int* crop_from, const int* dst_start,
                   const int* crop_len, float* dst, int Bd, int Ld, hipStream_t st) {
  MT_REQUIRE(rows && row_dst && crop_from && dst_start && crop_len && dst, "window_scatter: null argument");
  MT_REQUIRE(Bd > 0 && Ld > 0, "window_scatter: destination [%d][%d]", Bd, Ld);
  MT_REQUIRE(R > 0 && R <= RAG_MAXB, "window_scatter: %d window rows (1..%d)", R, RAG_MAXB);
  MT_REQUIRE(W > 0, "window_scatter: window of %d", W);
  hipLaunchKernelGGL(window_scatter_kernel, dim3((W + WG_THREADS - 1) / WG_THREADS, R), dim3(WG_THREADS), 0, st,
                     rows, W, row_dst, crop_from, dst_start, crop_len, dst, Bd, Ld);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace mt
