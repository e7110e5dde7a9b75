// Forced aligner for inference: given the encoder's mu [B][C][Tx] and a mel y [B][C][Ty], the
// frames each token spans under the textbook Monotonic Alignment Search (Glow-TTS / upstream Matcha
// `maximum_path_each`), whose predecessors are (x, y-1) and (x-1, y-1). The trainer keeps the reference's recurrence
// (mt_mas.hip, predecessors (x-1, y) and (x, y-1)): that one is the parity contract, this one recovers durations.
//
// Two launches:
//  1. align_lp_kernel: the log-prior in direct form, lp[b][x][j] = -0.5 * sum_c (yh[c][j] - mu[c][x])^2 - 0.5 C log(2 pi),
//     yh = (y - mean) / std. fp32, a compensated (Kahan) sum over c ascending, every fma spelled out: a cell's bits
//     are a function of mu[b,:,x] and y[b,:,j] alone. 64 x 64 cells per workgroup, 16-channel slabs of both
//     operands in LDS, 4 x 4 cells per thread.
//  2. align_mas_kernel: one workgroup per utterance, one thread per token, walking the frame columns. Both
//     predecessors of (x, y) lie on column y-1: a thread keeps its own p[x][y-1] in a register and reads p[x-1][y-1]
//     from a double-buffered LDS column (one barrier per column). Its lp row is prefetched eight columns ahead. Per
//     cell it keeps one bit, "the backtrack leaves token x when it steps from frame y to y-1":
//       x != 0 && (x == y || p[x][y-1] < p[x-1][y-1]),
//     a wave's 64 bits stored as one word per column. The backtrack stages those words through LDS, 128 columns at
//     a time, and one lane follows them from (tx-1, ty-1) down to (0, 0).
#include "mt_common.h"
#include "mt_misc.h"

namespace mt {

constexpr int ALIGN_MAXX = 1024;  // tokens per utterance (one thread each), as mt_mas.hip
constexpr int LP_TILE = 64;       // cells per workgroup side
constexpr int LP_CC = 16;         // channels per LDS slab
constexpr float ALIGN_NEG = -1e9f;

__global__ __launch_bounds__(256) void align_lp_kernel(const float* __restrict__ mu, const float* __restrict__ y,
                                                       const float* __restrict__ mean, const float* __restrict__ stdv,
                                                       int C, int Tx, int Ty, float cst, float* __restrict__ lp) {
  __shared__ float ms[LP_CC][LP_TILE], ys[LP_CC][LP_TILE];
  const int b = blockIdx.z, x0 = blockIdx.y * LP_TILE, j0 = blockIdx.x * LP_TILE;
  const int tid = threadIdx.x, jl = tid & 15, xl = tid >> 4;
  const bool norm = mean && stdv;
  float acc[4][4] = {}, cmp[4][4] = {};  // the running sum and its compensation: sum = acc - cmp
  for (int c0 = 0; c0 < C; c0 += LP_CC) {
    const int nc = min(LP_CC, C - c0);
    __syncthreads();  // the previous slab's reads are done
#pragma unroll
    for (int r = 0; r < LP_CC * LP_TILE / 256; ++r) {
      const int i = tid + 256 * r, c = i / LP_TILE, col = i % LP_TILE;
      float m = 0.f, v = 0.f;
      if (c < nc) {
        const size_t row = (size_t)b * C + c0 + c;
        if (x0 + col < Tx) m = mu[row * Tx + x0 + col];
        if (j0 + col < Ty) {
          v = y[row * Ty + j0 + col];
          if (norm) v = (v - mean[c0 + c]) / stdv[c0 + c];
        }
      }
      ms[c][col] = m;
      ys[c][col] = v;
    }
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
      float mv[4], yv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        mv[k] = ms[c][xl + 16 * k];
        yv[k] = ys[c][jl + 16 * k];
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          // Kahan's step, the square fused into the corrected term. A plain fp32 running sum of 80 positive terms
          // loses ~8e-5 at |lp| = 180 (half an ulp of the partial sum per add), more than the reference's expanded
          // form; compensated, what is left is the final rounding.
          const float d = yv[k] - mv[m];
          const float t = __builtin_fmaf(d, d, -cmp[m][k]);
          const float s = acc[m][k] + t;
          cmp[m][k] = (s - acc[m][k]) - t;
          acc[m][k] = s;
        }
    }
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int x = x0 + xl + 16 * m;
    if (x >= Tx) continue;
    float* o = lp + ((size_t)b * Tx + x) * Ty;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + jl + 16 * k;
      if (j < Ty) o[j] = __builtin_fmaf(-0.5f, acc[m][k], __builtin_fmaf(0.5f, cmp[m][k], -cst));
    }
  }
}

constexpr int MAS_CH = 8;     // lp columns a thread prefetches at a time
constexpr int MAS_BCOLS = 128;  // backtrack: columns of bit words staged in LDS at a time (x 16 words = 16 KiB)

__global__ __launch_bounds__(ALIGN_MAXX) void align_mas_kernel(const float* __restrict__ lp,
                                                               const int* __restrict__ t_xs,
                                                               const int* __restrict__ t_ys, int Tx, int Ty,
                                                               unsigned long long* __restrict__ bits,
                                                               long long* __restrict__ durations,
                                                               float* __restrict__ paths) {
  __shared__ float D[2][ALIGN_MAXX];
  __shared__ int sdur[ALIGN_MAXX], sstart[ALIGN_MAXX];
  __shared__ unsigned long long sb[MAS_BCOLS * (ALIGN_MAXX / 64)];
  const int b = blockIdx.x, x = threadIdx.x, nthr = blockDim.x;
  const int nw = (Tx + 63) / 64;  // bit words per column = waves of this workgroup
  // lengths clamped to the table: nothing below leaves this utterance's rows
  int tx = min(max(t_xs[b], 0), Tx);
  const int ty = min(max(t_ys[b], 0), Ty);
  if (ty < tx) tx = 0;  // no monotonic path with a frame per token: all-zero durations
  unsigned long long* bg = bits + (size_t)b * Ty * nw;
  for (int i = x; i < ALIGN_MAXX; i += nthr) sdur[i] = sstart[i] = 0;
  if (tx > 0) {
    const bool act = x < tx;
    const float* row = lp + ((size_t)b * Tx + (act ? x : 0)) * Ty;
    float cur[MAS_CH], nxt[MAS_CH];
#pragma unroll
    for (int k = 0; k < MAS_CH; ++k) cur[k] = (act && k < ty) ? row[k] : 0.f;
    float p = ALIGN_NEG;  // p[x][y-1]; NEG while (x, y-1) lies outside the band
    for (int y0 = 0; y0 < ty; y0 += MAS_CH) {
#pragma unroll
      for (int k = 0; k < MAS_CH; ++k) nxt[k] = (act && y0 + MAS_CH + k < ty) ? row[y0 + MAS_CH + k] : 0.f;
#pragma unroll
      for (int k = 0; k < MAS_CH; ++k) {
        const int yy = y0 + k;
        if (yy >= ty) break;  // uniform
        const bool in = act && x >= tx + yy - ty && x <= yy;
        bool dec = false;
        float pn = ALIGN_NEG;
        if (in) {
          const float vc = x == yy ? ALIGN_NEG : p;
          const float vp = x == 0 ? (yy == 0 ? 0.f : ALIGN_NEG) : (yy > 0 ? D[(yy + 1) & 1][x - 1] : ALIGN_NEG);
          pn = cur[k] + fmaxf(vc, vp);
          dec = x != 0 && (x == yy || p < vp);
        }
        p = pn;
        D[yy & 1][x] = pn;
        const unsigned long long w = __ballot(dec);
        if ((x & 63) == 0) bg[(size_t)yy * nw + (x >> 6)] = w;
        __syncthreads();
      }
#pragma unroll
      for (int k = 0; k < MAS_CH; ++k) cur[k] = nxt[k];
    }
    // backtrack: idx = tx - 1; for y = ty-1 .. 0: durations[idx] += 1, then leave idx when its bit is set
    int idx = tx - 1, run = 0;
    for (int c1 = ty; c1 > 0; c1 -= MAS_BCOLS) {
      const int c0 = max(c1 - MAS_BCOLS, 0);
      __syncthreads();  // the bit words are this workgroup's own stores; the previous chunk's walk is done
      for (int i = x; i < (c1 - c0) * nw; i += nthr) sb[i] = bg[(size_t)c0 * nw + i];
      __syncthreads();
      if (x == 0) {
        for (int yy = c1 - 1; yy >= c0; --yy) {
          ++run;
          if ((sb[(yy - c0) * nw + (idx >> 6)] >> (idx & 63)) & 1ull) {
            sdur[idx] = run;
            sstart[idx] = yy;
            run = 0;
            --idx;
          }
        }
        if (c0 == 0) sdur[idx] = run;  // idx == 0 here (idx <= y throughout); it starts at frame 0
      }
    }
  }
  __syncthreads();
  for (int i = x; i < Tx; i += nthr) durations[(size_t)b * Tx + i] = i < tx ? sdur[i] : 0;
  if (paths) {
    float* o = paths + (size_t)b * Tx * Ty;
    for (int r = 0; r < Tx; ++r) {
      const int s = sstart[r], e = r < tx ? s + sdur[r] : s;
      for (int j = x; j < Ty; j += nthr) o[(size_t)r * Ty + j] = (j >= s && j < e) ? 1.f : 0.f;
    }
  }
}

static size_t align_bits_bytes(int B, int Tx, int Ty) {
  const size_t n = (size_t)B * Ty * ((Tx + 63) / 64) * sizeof(unsigned long long);
  return (n + 255) / 256 * 256;
}

size_t align_workspace_bytes(int B, int C, int Tx, int Ty) {
  (void)C;
  if (B <= 0 || Tx <= 0 || Ty <= 0) return 0;
  return align_bits_bytes(B, Tx, Ty) + (size_t)B * Tx * Ty * sizeof(float);  // bit table + log-prior
}

int align(const float* mu, const float* y, const float* mean, const float* stdv, const int* t_xs, const int* t_ys,
          int B, int C, int Tx, int Ty, long long* durations, float* log_prior, float* paths, void* ws,
          size_t ws_bytes, hipStream_t st) {
  MT_REQUIRE(B > 0 && C > 0 && Tx > 0 && Ty > 0, "align: B %d, C %d, Tx %d, Ty %d", B, C, Tx, Ty);
  MT_REQUIRE(Tx <= ALIGN_MAXX, "align: %d tokens > %d", Tx, ALIGN_MAXX);
  MT_REQUIRE(B <= 65535 && (Tx + LP_TILE - 1) / LP_TILE <= 65535, "align: batch %d too large", B);
  MT_REQUIRE(ws && ws_bytes >= align_workspace_bytes(B, C, Tx, Ty), "align: workspace too small");
  float* lp = log_prior ? log_prior : (float*)((char*)ws + align_bits_bytes(B, Tx, Ty));
  const float cst = (float)(0.5 * C * 1.8378770664093454835606594728112);  // 0.5 C log(2 pi)
  dim3 grid((Ty + LP_TILE - 1) / LP_TILE, (Tx + LP_TILE - 1) / LP_TILE, B);
  hipLaunchKernelGGL(align_lp_kernel, grid, dim3(256), 0, st, mu, y, mean, stdv, C, Tx, Ty, cst, lp);
  MT_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(align_mas_kernel, dim3(B), dim3((Tx + 63) / 64 * 64), 0, st, lp, t_xs, t_ys, Tx, Ty,
                     (unsigned long long*)ws, durations, paths);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace mt
