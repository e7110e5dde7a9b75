// Joining a batch of sentences into documents on gfx950 (matcha_hip/join.py is the same specification
// on the CPU): trim edges of every row, the place of every segment in its document, and the documents themselves with
// raised-cosine fades and overlaps. Three memory-bound single passes; integers are exact, and a document sample is one
// fp32 product per covering segment plus one fp32 sum per product, in segment order: no atomics anywhere, so a
// document's bits depend on its own segments alone.
//
// edges_tile_kernel: one workgroup per (row, tile of ED_TILE samples counted from the row's start); tiles at or past
//   the row's length return at once and nothing at or past it is read. Thread t reads samples t, t + 256, ...
//   (coalesced), keeps the smallest and the largest loud index, and the workgroup's pair goes to the workspace.
//   edges_final_kernel (one workgroup per row) reduces the pairs of the row's live tiles and applies the padding.
// join_plan_kernel: one workgroup per document walks its segments in chunks of JP_CHUNK with an exclusive scan of
//   len_s + g_s in 64-bit integers (an LDS scan per chunk, the carry in a register).
// join_kernel: one workgroup per (document, tile of JN_TILE output samples). The tile's first segment is the one before
//   the last segment whose dst is at or before the tile's first sample (binary search in the document's range of
//   dst, which a plan of join_plan leaves non-decreasing); from there the workgroup walks forward until a segment
//   starts past the tile. Thread t owns samples t, t + 256, ... of the tile: coalesced loads of the segment, coalesced
//   stores of the document, which is written whole (zero where nothing covers a sample and from doc_len on).
//   The product w * x and the sum are rounded separately: the kernel is compiled with `#pragma clang fp contract(off)`
//   (HIP's __fmul_rn / __fadd_rn are plain operators the compiler may fuse again after inlining).
// The tables are device memory the host cannot check: every entry is clamped where it is used (row and segment
// ranges to their buffers, edges to [0, L], doc_len to [0, Ld]), so a wrong entry gives wrong audio, never an access
// out of range, and every loop is bounded by the table sizes.
#include <limits.h>
#include <math.h>

#include "mt_common.h"
#include "mt_resample.h"

namespace mt {

constexpr int JN_THREADS = 256;
constexpr int ED_TILE = 4096;        // samples per edges tile (runtime.EDGES_TILE)
constexpr int JP_CHUNK = 256;        // segments per scan step of the plan (runtime.JOIN_PLAN_CHUNK)
constexpr int JN_TILE = 1024;        // document samples per join tile (runtime.JOIN_TILE)
constexpr int JN_MAX_ROWS = 65535;   // S and D: grid.y
constexpr int JN_MAX_L = 1 << 30;    // L, Ld and Lcap: mt_loudness' bound on a row
constexpr int JN_MAX_FADE = 1 << 14; // (2 j + 1) fade < 2^31
static_assert(ED_TILE % JN_THREADS == 0 && JN_TILE % JN_THREADS == 0 && JP_CHUNK == JN_THREADS, "tile shapes");

__device__ __forceinline__ int clampi(long long v, int lo, int hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

// the workgroup's min of lo and max of hi, valid in thread 0
__device__ __forceinline__ void block_minmax(int& lo, int& hi, int* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o, 64));
    hi = max(hi, __shfl_xor(hi, o, 64));
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sm[2 * w] = lo;
    sm[2 * w + 1] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < JN_THREADS / 64; ++k) {
      lo = min(lo, sm[2 * k]);
      hi = max(hi, sm[2 * k + 1]);
    }
  }
}

__global__ __launch_bounds__(JN_THREADS) void edges_tile_kernel(const float* __restrict__ audio, int L,
                                                                const int* __restrict__ lens, float thr, int nT,
                                                                int* __restrict__ part) {
  __shared__ int sm[2 * JN_THREADS / 64];
  const int s = blockIdx.y, t = blockIdx.x;
  const int n = utt_len(lens, s, 1, L);
  const int i0 = t * ED_TILE;  // < L <= 2^30
  if (i0 >= n) return;         // the final pass reads the pairs of live tiles only
  const float* x = audio + (size_t)s * L;
  int lo = INT_MAX, hi = -1;
#pragma unroll 4
  for (int k = 0; k < ED_TILE / JN_THREADS; ++k) {
    const int i = i0 + k * JN_THREADS + (int)threadIdx.x;
    if (i < n && fabsf(x[i]) >= thr) {  // false for a NaN
      lo = min(lo, i);
      hi = i;
    }
  }
  block_minmax(lo, hi, sm);
  if (threadIdx.x == 0) {
    int* o = part + ((size_t)s * nT + t) * 2;
    o[0] = lo;
    o[1] = hi;
  }
}

__global__ __launch_bounds__(JN_THREADS) void edges_final_kernel(const int* __restrict__ part, int L,
                                                                 const int* __restrict__ lens, int nT, int pad,
                                                                 int* __restrict__ start, int* __restrict__ end) {
  __shared__ int sm[2 * JN_THREADS / 64];
  const int s = blockIdx.x;
  const int n = utt_len(lens, s, 1, L);
  const int nt = (n + ED_TILE - 1) / ED_TILE;  // <= nT
  const int* p = part + (size_t)s * nT * 2;
  int lo = INT_MAX, hi = -1;
  for (int t = threadIdx.x; t < nt; t += JN_THREADS) {
    lo = min(lo, p[2 * t]);
    hi = max(hi, p[2 * t + 1]);
  }
  block_minmax(lo, hi, sm);
  if (threadIdx.x != 0) return;
  if (hi < 0) {
    start[s] = 0;
    end[s] = 0;
  } else {
    start[s] = clampi((long long)lo - pad, 0, n);
    end[s] = clampi((long long)hi + 1 + pad, 0, n);
  }
}

// document d's segments [lo, hi) inside [0, S]
__device__ __forceinline__ void doc_range(const int* __restrict__ doc_first, int d, int S, int& lo, int& hi) {
  lo = clampi(doc_first[d], 0, S);
  hi = clampi(doc_first[d + 1], lo, S);
}
// the kept samples [a, a + len) of segment s
__device__ __forceinline__ int seg_len(const int* __restrict__ start, const int* __restrict__ end, int s, int L,
                                       int& a) {
  a = clampi(start[s], 0, L);
  return clampi(end[s], a, L) - a;
}

__global__ __launch_bounds__(JN_THREADS) void join_plan_kernel(const int* __restrict__ doc_first,
                                                               const int* __restrict__ start,
                                                               const int* __restrict__ end,
                                                               const int* __restrict__ gap, int S, int L, int head,
                                                               int tail, int Lcap, int* __restrict__ dst,
                                                               int* __restrict__ doc_len, int* __restrict__ bad) {
  __shared__ long long sc[2][JP_CHUNK];
  const int d = blockIdx.x, tid = threadIdx.x;
  int lo, hi;
  doc_range(doc_first, d, S, lo, hi);
  long long pos = head;  // where the chunk's first segment starts: < 2^31 + 65535 * (2^30 + 2^31)
  for (int c0 = lo; c0 < hi; c0 += JP_CHUNK) {
    const int s = c0 + tid;
    long long inc = 0;  // from the start of s to the start of s + 1 (to the document's end without its tail)
    if (s < hi) {
      int a;
      const int len = seg_len(start, end, s, L, a);
      inc = len;
      if (s + 1 < hi) {
        const int nxt = seg_len(start, end, s + 1, L, a);
        inc += max(gap[s], -min(len >> 1, nxt >> 1));
      }
    }
    // inclusive scan of inc over the chunk (Hillis-Steele, double-buffered)
    int cur = 0;
    sc[0][tid] = inc;
    __syncthreads();
#pragma unroll
    for (int o = 1; o < JP_CHUNK; o <<= 1) {
      const long long v = sc[cur][tid] + (tid >= o ? sc[cur][tid - o] : 0ll);
      sc[cur ^ 1][tid] = v;
      cur ^= 1;
      __syncthreads();
    }
    const long long incl = sc[cur][tid];
    if (s < hi) {
      const long long at = pos + incl - inc;  // >= 0: head >= 0 and every inc >= 0
      dst[s] = (int)(at < Lcap ? at : Lcap);
    }
    pos += sc[cur][JP_CHUNK - 1];
    __syncthreads();  // the next chunk overwrites sc
  }
  if (tid == 0) {
    const long long n = pos + tail;
    doc_len[d] = (int)(n < Lcap ? n : Lcap);
    if (n > Lcap) *bad = 1;  // every writer writes the same value
  }
}

__global__ __launch_bounds__(JN_THREADS) void join_kernel(const float* __restrict__ seg, int S, int L,
                                                          const int* __restrict__ start,
                                                          const int* __restrict__ end,
                                                          const int* __restrict__ doc_first,
                                                          const int* __restrict__ dst,
                                                          const int* __restrict__ doc_len,
                                                          const float* __restrict__ ramp, int fade,
                                                          float* __restrict__ out, int Ld) {
#pragma clang fp contract(off)
  constexpr int K = JN_TILE / JN_THREADS;
  const int d = blockIdx.y, tid = threadIdx.x;
  const int i0 = blockIdx.x * JN_TILE;  // < Ld <= 2^30
  const int n_d = clampi(doc_len[d], 0, Ld);
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.f;
  if (i0 < n_d) {
    int lo, hi;
    doc_range(doc_first, d, S, lo, hi);
    // p = the number of segments of [lo, hi) with dst <= i0; only the last of them and the one before can cover i0
    int bl = lo, bh = hi;
    while (bl < bh) {
      const int m = bl + ((bh - bl) >> 1);
      if (dst[m] <= i0)
        bl = m + 1;
      else
        bh = m;
    }
    const int tile_end = min(i0 + JN_TILE, n_d);
    for (int s = max(bl - 2, lo); s < hi; ++s) {
      const int ds = dst[s];
      if (ds >= tile_end) break;
      int a;
      const int len = seg_len(start, end, s, L, a);
      if ((long long)ds + len <= i0) continue;
      const int F = min(fade, len >> 1);
      const float* x = seg + (size_t)s * L + a;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int i = i0 + k * JN_THREADS + tid;
        const long long jl = (long long)i - ds;
        if (i < n_d && jl >= 0 && jl < len) {
          const int j = (int)jl;
          const int jf = j < F ? j : (j >= len - F ? len - 1 - j : -1);  // the fades never meet: F <= len / 2
          float w = 1.f;
          if (jf >= 0) w = ramp[F == fade ? jf : ((2 * jf + 1) * fade) / (2 * F)];
          const float pr = w * x[j];
          acc[k] = acc[k] + pr;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = i0 + k * JN_THREADS + tid;
    if (i < Ld) out[(size_t)d * Ld + i] = acc[k];
  }
}

// ---- host side -----------------------------------------------------------------------------------------------

static int edges_shape_check(int S, int L) {
  MT_REQUIRE(S > 0 && S <= JN_MAX_ROWS && L > 0 && L <= JN_MAX_L, "audio_edges: S %d (1..%d), L %d (1..%d)", S,
             JN_MAX_ROWS, L, JN_MAX_L);
  return 0;
}

size_t audio_edges_workspace_bytes(int S, int L) {
  if (edges_shape_check(S, L) != 0) return 0;
  return (size_t)S * (((size_t)L + ED_TILE - 1) / ED_TILE) * 2 * sizeof(int);
}

int audio_edges(const float* audio, int S, int L, const int* lens, float thr, int pad, int* start, int* end, void* ws,
                size_t ws_bytes, hipStream_t st) {
  if (edges_shape_check(S, L) != 0) return -1;
  MT_REQUIRE(audio && start && end, "audio_edges: null argument");
  MT_REQUIRE(isfinite(thr) && thr >= 0.f, "audio_edges: threshold %g is not a finite magnitude", (double)thr);
  MT_REQUIRE(pad >= 0, "audio_edges: pad %d is negative", pad);
  MT_REQUIRE(ws && ws_bytes >= audio_edges_workspace_bytes(S, L) && ((uintptr_t)ws & 15) == 0,
             "audio_edges: workspace too small or not 16-byte aligned");
  const int nT = (int)(((size_t)L + ED_TILE - 1) / ED_TILE);
  hipLaunchKernelGGL(edges_tile_kernel, dim3(nT, S), dim3(JN_THREADS), 0, st, audio, L, lens, thr, nT, (int*)ws);
  MT_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(edges_final_kernel, dim3(S), dim3(JN_THREADS), 0, st, (const int*)ws, L, lens, nT, pad, start,
                     end);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

int join_plan(const int* doc_first, int D, const int* start, const int* end, const int* gap, int S, int L, int head,
              int tail, int Lcap, int* dst, int* doc_len, int* bad, hipStream_t st) {
  MT_REQUIRE(doc_first && start && end && gap && dst && doc_len && bad, "join_plan: null argument");
  MT_REQUIRE(S > 0 && S <= JN_MAX_ROWS && D > 0 && D <= JN_MAX_ROWS, "join_plan: S %d, D %d (1..%d each)", S, D,
             JN_MAX_ROWS);
  MT_REQUIRE(L > 0 && L <= JN_MAX_L, "join_plan: L %d (1..%d)", L, JN_MAX_L);
  MT_REQUIRE(head >= 0 && tail >= 0, "join_plan: head %d or tail %d is negative", head, tail);
  MT_REQUIRE(Lcap >= 1 && Lcap <= JN_MAX_L, "join_plan: Lcap %d outside 1..%d", Lcap, JN_MAX_L);
  MT_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
  hipLaunchKernelGGL(join_plan_kernel, dim3(D), dim3(JN_THREADS), 0, st, doc_first, start, end, gap, S, L, head, tail,
                     Lcap, dst, doc_len, bad);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

int join(const float* seg, int S, int L, const int* start, const int* end, const int* doc_first, int D, const int* dst,
         const int* doc_len, const float* ramp, int fade, float* out, int Ld, hipStream_t st) {
  MT_REQUIRE(seg && start && end && doc_first && dst && doc_len && out, "join: null argument");
  MT_REQUIRE(S > 0 && S <= JN_MAX_ROWS && D > 0 && D <= JN_MAX_ROWS, "join: S %d, D %d (1..%d each)", S, D,
             JN_MAX_ROWS);
  MT_REQUIRE(L > 0 && L <= JN_MAX_L && Ld > 0 && Ld <= JN_MAX_L, "join: L %d, Ld %d (1..%d each)", L, Ld, JN_MAX_L);
  MT_REQUIRE(fade >= 0 && fade <= JN_MAX_FADE, "join: fade %d outside 0..%d", fade, JN_MAX_FADE);
  MT_REQUIRE(fade == 0 || ramp, "join: fade %d without a ramp table", fade);
  hipLaunchKernelGGL(join_kernel, dim3((Ld + JN_TILE - 1) / JN_TILE, D), dim3(JN_THREADS), 0, st, seg, S, L, start,
                     end, doc_first, dst, doc_len, ramp, fade, out, Ld);
  MT_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace mt
