// Fused HiFi-GAN ResBlock1 PAIR for the 128-channel stage (stage 2 of v1), bf16, gfx950 — the 128-channel
// sibling of mt_vpair.hip:
//
//   t = conv_{k, d}(lrelu(x)) ;  y = conv_{k, 1}(lrelu(t)) + x          (hifigan/models.py:90-97)
//   (the last pair of resblock j: xs = [xs +] y [/ nk], + lrelu(xs) for the next upsampler, models.py:187-192)
//
// Per layer (mt_vconv) this pair moves x_act in, t out, t back in, x in, y and y_act out: six 128-channel
// tensors. Fused it moves x in and y out. The price is LDS: a 128-channel row is 256 bytes, so a tile is only
// 192 conv1 frames (the intermediate t is 192 x 128 channels), and conv2 keeps BN = 192 - 2 h2 of them
// (h2 = (k - 1) / 2: 190 / 186 / 182 output frames for k = 3 / 7 / 11).
//
// One persistent 512-thread workgroup per CU walks the tiles. Waves: 2 along rows (64 output channels each)
// x 4 along frames (48 frames = 3 fragments each). Per tile:
//   1. the RAW input rows (192 conv1 frames + the conv1 halo 2 h1 <= 40 rows: k <= 7 at d = 5, k = 11 at d <= 3;
//      a k = 11, d = 5 pair is not supported here and runs per layer on mt_vconv — the default vocoder fuses only
//      the k = 3 resblock on this kernel) of both 64-channel planes land
//      in LDS by global_load_lds_dwordx4 (issued during the previous tile's second conv); each lane reads its
//      residual rows out of them, then one in-place VALU pass turns them into lrelu(rows);
//   2. conv1: 128 rows x 192 frames over (chunk, tap) steps; epilogue lrelu(round(acc + b1)), zero outside
//      [0, L) -> T (two 64-channel planes in LDS);
//   3. conv2: 128 rows x 192 frames over T (frames past BN discarded); epilogue + b2 + x [+ xs, / nk] -> y
//      (+ lrelu(y)).
// A step is one (64-channel chunk, tap) pair: a 16 KiB weight slot of the mt_vconv image [2][k][128][64]
// (3-slot LDS ring, two steps in flight) and 24 MFMAs per wave. Steps run chunk-major, taps ascending, two
// K = 32 slices each: the per-output MFMA accumulation order of mt_vconv's K loop, and its rounding points
// (every stored tensor rounded to bf16 once, activated outputs lrelu'd in fp32 first), so the results are the
// same bits as the per-layer mt_vconv path.
// LDS: T planes (2 x 192 rows) | X planes (2 x XROWS = 232 rows) | weight ring | biases | the ragged tile map. Rows are 128 B
// with the 16-byte unit XOR-swizzled by (row & 6) (mt_vconv's conflict-free layout). conv2's discarded last
// fragments read up to 2 h2 rows past a T plane: into the next plane / the X planes, never outside LDS.
#include <algorithm>
#include <type_traits>

#include "mt_probe.h"
#include "mt_ts.h"
#include "mt_vpair.h"

namespace mt {

namespace {
constexpr int NT = 512, C = 128;
constexpr int FN = 3;                // 16-frame fragments per wave
constexpr int WNC = 16 * FN;         // frames per wave (4 waves along frames)
constexpr int NF1 = 4 * WNC;         // conv1 frames per tile (192)
constexpr int XROWS = NF1 + 40;      // staged input rows >= NF1 + 2 h1 (k <= 7 at d = 5; room for the ragged map)
constexpr int XPL = XROWS * 128;     // one 64-channel plane of X
constexpr int TPL = NF1 * 128;       // one 64-channel plane of T
constexpr int WSLOT = C * 128;       // one step: 128 output rows x 64 input channels (16 KiB)
constexpr int NWS = 3;
constexpr int T_OFF = 0, X_OFF = 2 * TPL, W_OFF = X_OFF + 2 * XPL, PAR_OFF = W_OFF + NWS * WSLOT;
constexpr int RAG_OFF = PAR_OFF + 2 * C * 4;
constexpr int LDS_BYTES = RAG_OFF + RAG_LDS;
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
static_assert(XROWS % 8 == 0, "X staged 8 rows per DMA instruction");
// the compile-time K loop (vpair128_kernel<EF, K>, K > 0) stages a fixed XPW row pieces per wave (8 rows of one plane
// each: 4 XPW blocks per plane, the rows past R1 zero) so that every vmcnt count is a constant; spread over the
// first XSP of conv2's steps
constexpr int XPW = 7;
#ifndef VP128_XSP
#define VP128_XSP 4
#endif
static_assert(32 * XPW <= XROWS, "fixed row staging fits the X planes");
#ifndef VP128_BUF
#define VP128_BUF 1  // 1: the compile-time kernel's LDS-DMA and the y / y2 stores through buffer resources (mt_common.h)
#endif
}  // namespace

// the compile-time K loop's schedule of vpair128_kernel<EF, K> (K > 0; registered by launch_vpair128 for the CPU replay)
template <int EF, int K>
using Vp128Sched = VpkSched<EF, 2 * (K > 0 ? K : 1), XPW, FN, (VP128_XSP < 2 * K ? VP128_XSP : 2 * (K > 0 ? K : 1)), NWS>;

// K > 0: the compile-time K loop (k = K): steps unrolled, ring slots and vmcnt counts constants (VpkSched), step
// barriers without an lgkmcnt drain except each conv's first, phantom prefetches past the workgroup's last tile
template <int EF, int K = 0, int SP = ST_PLAIN>  // SP: the y / y2 stores' policy (mt_common.h)
__global__ __launch_bounds__(NT) void vpair128_kernel(VPairArgs a) {
  static_assert(SP == ST_PLAIN || VP128_BUF, "the store policy rides on the buffer stores");
  __shared__ __attribute__((aligned(1024))) char smem[LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;  // 64-row half, 48-frame quarter
  const int g4 = lane >> 4, l16 = lane & 15, lrow = lane >> 3, lp = lane & 7;
  const int k = K > 0 ? K : a.taps, d = a.dil, L = a.L;
  const int h1 = d * (k - 1) / 2, h2 = (k - 1) / 2;
  const int BN = NF1 - 2 * h2;  // output frames per tile
  const int R1 = NF1 + 2 * h1;  // staged rows per plane
  const int nxi = (R1 + 7) / 8; // DMA instructions per plane
  PairWalk tiles;
  if (!tiles.init(a, smem + RAG_OFF, BN, tid)) return;
  const int nmine = tiles.nmine;
  pair_load_bias<C, NT>(reinterpret_cast<float*>(smem + PAR_OFF), a, tid);

  int issued = 0, xmk = 0;
  int wmk[NWS] = {};
  const int ns = 2 * k;          // steps per conv: (chunk, tap), chunk-major
  const int S = nmine * 2 * ns;  // weight steps of this workgroup
  RagTile nxt;  // the tile stage_x staged last (the next tile of the loop)
  // VP128_BUF: this lane's byte offsets within a weight piece (row 16 wave + lrow of the step's block; + 8 rows for
  // the second piece) and a row piece (row lrow of 8 of one plane); the 16-byte unit is swizzled by lrow & 6
  const int wlane = (16 * wave + lrow) * 128 + ((lp ^ (lrow & 6)) * 16);
  const int xlane = lrow * (C * 2) + ((lp ^ (lrow & 6)) * 16);
  auto stage_w = [&](int s) {  // step m of conv1 or conv2: image block (chunk m / k, tap m % k)
    const int r2 = s % (2 * ns);
    const int m = r2 < ns ? r2 : r2 - ns;
    const bf16* w = (r2 < ns ? a.w1 : a.w2) + (size_t)m * C * 64;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = 16 * wave + 8 * u + lrow;
      glds16(w + r * 64 + (lp ^ (r & 6)) * 8, smem + W_OFF + (s % NWS) * WSLOT + (16 * wave + 8 * u) * 128);
    }
    issued += 2;
    wmk[s % NWS] = issued;
  };
  // K > 0: the weights of tile step q (mod S) into ring slot `slot` (opaque offsets: with a constant LDS destination
  // the compiler tracks the DMA and waits for it before every ds_read it cannot prove disjoint)
  auto stage_w_ct = [&](auto qc, int slot) __attribute__((always_inline)) {
    constexpr int NSK = 2 * (K > 0 ? K : 1), q = decltype(qc)::value % (2 * NSK);
    constexpr int m = q < NSK ? q : q - NSK;
    const bf16* w = (q < NSK ? a.w1 : a.w2) + (size_t)m * C * 64;
    int so = W_OFF + slot * WSLOT + 16 * wave * 128;
    asm volatile("" : "+s"(so));
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if constexpr (VP128_BUF && K > 0) {
        // the step's [C][64] block as the scalar offset, the lane's row unit as the (fixed) vector offset
        const auto wr = buf_rsrc(q < NSK ? a.w1 : a.w2, (unsigned)(NSK * C * 64 * 2));
        buf_lds16(wr, (unsigned)(wlane + u * 8 * 128), (unsigned)(m * C * 64 * 2), smem + so + 8 * u * 128);
      } else {
        const int r = 16 * wave + 8 * u + lrow;
        int off = r * 64 + (lp ^ (r & 6)) * 8;
        asm volatile("" : "+v"(off));
        glds16(w + off, smem + so + 8 * u * 128);
      }
    }
  };
  const bf16* sx_xb = a.x;
  int sx_f0 = 0, sx_lv = 0;
  auto stage_x_begin = [&](int ti) {
    nxt = tiles.at(K > 0 ? min(ti, nmine - 1) : ti);  // K > 0: past the last tile a phantom copy of it (never read)
    sx_xb = a.x + (size_t)__builtin_amdgcn_readfirstlane(nxt.b) * L * C;
    sx_f0 = __builtin_amdgcn_readfirstlane(nxt.n0 - h2 - h1), sx_lv = __builtin_amdgcn_readfirstlane(nxt.lv);
  };
  auto stage_x_piece = [&](int j) {  // rows 8 blk .. 8 blk + 7 of plane p (j = 2 blk + p)
    const int p = j & 1, blk = j >> 1;
    if constexpr (VP128_BUF && K > 0) {
      // the utterance as a buffer of its sx_lv valid frames: row r = frame sx_f0 + r, plane p = channels 64 p ..;
      // offsets of frames before the utterance wrap past the range (zero padding on both sides); rows past R1 are
      // staged too and never read
      buf_lds16(buf_rsrc(sx_xb, (unsigned)sx_lv * (C * 2)), (unsigned)(xlane + (sx_f0 + 8 * blk) * C * 2 + p * 128), 0u,
                smem + X_OFF + p * XPL + blk * 1024);
      return;
    }
    const int r = 8 * blk + lrow;
    const int q = lp ^ (r & 6);
    const int f = sx_f0 + r;
    const bool ok = r < R1 && f >= 0 && f < sx_lv;
    glds16(ok ? sx_xb + (size_t)f * C + p * 64 + q * 8 : a.zero + q * 8, smem + X_OFF + p * XPL + blk * 1024);
  };
  auto stage_x = [&](int ti) {  // raw rows of tile ti, both planes: row r = frame n0 - h2 - h1 + r
    stage_x_begin(ti);
    if constexpr (K > 0) {
#pragma unroll
      for (int i = 0; i < XPW; ++i) stage_x_piece(wave + 8 * i);
    } else {
      for (int j = wave; j < 2 * nxi; j += 8) {
        stage_x_piece(j);
        ++issued;
      }
      xmk = issued;
    }
  };

  const int ha = l16 & 6;

  f32x4 acc[4][FN];
  struct Frag {
    bf16x8 A[4], B[FN];
  };
  // K-slice ks of a step: A = this wave's 4 row fragments of the slot, B = FN frame fragments at rows
  // rb + 16 fn of plane `pl`
  auto read_frag = [&](Frag& F, int ks, int slot, const char* pl, int rb0) {
    const char* pa = smem + W_OFF + slot * WSLOT + (wm * 64 + l16) * 128 + (((ks * 4 + g4) ^ ha) * 16);
#pragma unroll
    for (int f = 0; f < 4; ++f) F.A[f] = *reinterpret_cast<const bf16x8*>(pa + f * 2048);
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const int rb = rb0 + fn * 16;
      F.B[fn] = *reinterpret_cast<const bf16x8*>(pl + rb * 128 + (((ks * 4 + g4) ^ (rb & 6)) * 16));
    }
  };
  // first: the conv's first K-slice starts the accumulators from the MFMA's zero C operand
  auto mma_slice = [&](const Frag& F, auto first) {
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        acc[fm][fn] = mfma16(F.A[fm], F.B[fn], decltype(first)::value ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[fm][fn]);
    constexpr int NR = 4 + FN, NMF = 4 * FN;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
    }
    __builtin_amdgcn_sched_group_barrier(0x008, NMF - NR, 0);
  };
  // one conv over the two planes of `src` (plane stride `pst`): steps (chunk c, tap t), the lane's first B row
  // of tap t at rb0 + t * tstride; each step's second K-slice is read under its first, the next step's first
  // under its second
  Frag F0, F1;
  int s = 0;
  VP_TS_DECL
  auto conv = [&](const char* src, int pst, int rb0, int tstride, auto&& at_first_step) {
    auto step = [&](int m, auto first) {
      const bool more = m + 1 < ns;
#if defined(VPAIR_TS)
      if (s % (2 * ns) < ns) VP_TS(4); else VP_TS(7);
#endif
      wait_vmcnt(issued - wmk[(more ? s + 1 : s) % NWS]);  // this step's weights and the next step's
      lds_barrier();
      VP_TS(6);
      if (s + NWS - 1 < S) stage_w(s + NWS - 1);
      const int sl = s % NWS;
      const int c = m >= k ? 1 : 0, t = m - c * k;
      if constexpr (decltype(first)::value) {
        at_first_step();
        read_frag(F0, 0, sl, src, rb0);
      }
      read_frag(F1, 1, sl, src + c * pst, rb0 + t * tstride);
      mma_slice(F0, first);
      if (more) {
        const int c2 = m + 1 >= k ? 1 : 0, t2 = m + 1 - c2 * k;
        read_frag(F0, 0, (s + 1) % NWS, src + c2 * pst, rb0 + t2 * tstride);
      }
      mma_slice(F1, std::false_type{});
    };
    step(0, std::true_type{});
    ++s;
    for (int m = 1; m < ns; ++m, ++s) step(m, std::false_type{});
  };
  // K > 0: conv CV (0: conv1 = tile steps 0 .. NS-1, 1: conv2 = NS .. S-1) unrolled; the tile's ring slots from its
  // slot base sb (S % 3 != 0 rotates it per tile)
  using SCH = Vp128Sched<EF, K>;
  auto slot_of = [&](int sb, int q) __attribute__((always_inline)) {  // ring slot of tile step q (q may pass S)
    const int v = sb + q % NWS;
    return v >= NWS ? v - NWS : v;
  };
  // at_step(m): the step's other VMEM operations after its weight DMA (VpkSched::after_w)
  auto conv_ct = [&](auto cvc, const char* src, int pst, int rb0, int tstride, int sb, bool first_tile,
                     auto&& at_step) __attribute__((always_inline)) {
    constexpr int CV = decltype(cvc)::value, NSK = SCH::NS;
    vc_for<0, NSK>([&](auto mc) {
      constexpr int m = decltype(mc)::value, st = CV * NSK + m;
      constexpr bool more = m + 1 < NSK;
      constexpr int c = m >= K ? 1 : 0, t = m - c * K;
      constexpr int c2 = m + 1 >= K ? 1 : 0, t2 = m + 1 - c2 * K;
      if constexpr (CV == 0) VP_TS(4); else VP_TS(7);
      if constexpr (st == 0) {
        if (first_tile) vc_wait_vmcnt<SCH::wait_first0>();
        else vc_wait_vmcnt<SCH::wait(0)>();
      } else {
        vc_wait_vmcnt<SCH::wait(st)>();
      }
      if constexpr (m == 0) lds_barrier();
      else step_barrier();
      VP_TS(6);
      stage_w_ct(std::integral_constant<int, st + NWS - 1>{}, slot_of(sb, st + NWS - 1));
      const int sl = slot_of(sb, st);
      int lb = 0;  // opaque per-step row base: hoisted per-step fragment addresses would take hundreds of VGPRs
      asm volatile("" : "+v"(lb));
      at_step(mc);
      if constexpr (m == 0) read_frag(F0, 0, sl, src, rb0 + lb);
      read_frag(F1, 1, sl, src + c * pst, rb0 + lb + t * tstride);
      mma_slice(F0, std::integral_constant<bool, m == 0>{});
      if constexpr (more) read_frag(F0, 0, slot_of(sb, st + 1), src + c2 * pst, rb0 + lb + t2 * tstride);
      mma_slice(F1, std::false_type{});
    });
  };

  // ---- prologue ----
  stage_x(0);
  if constexpr (K > 0) {
    vc_for<0, SCH::PW>([&](auto qc) { stage_w_ct(qc, decltype(qc)::value); });
  } else {
#pragma unroll
    for (int p = 0; p < NWS - 1; ++p)
      if (p < S) stage_w(p);
  }
  int sb = 0;  // K > 0: ring slot of the tile's step 0

  const float* par = reinterpret_cast<const float*>(smem + PAR_OFF);
  const int ch16 = (g4 & 1) * 16 + (g4 >> 1) * 8;  // + fp * 32: this lane's 8 channels after the pair swap
  const char* xpl = smem + X_OFF + wm * XPL;        // this wave's rows' plane of X
  for (int ti = 0; ti < nmine; ++ti) {
    const int b = nxt.b, n0 = nxt.n0;  // staged by the previous stage_x (tile ti)
    const int Lt = nxt.lv;             // this utterance's frames (conv2's zero padding starts there)
    // ---- 1. the residual rows of this lane's outputs (output frame n0 + i = raw row i + h2 + h1), then the
    // in-place lrelu of the landed raw rows ----
    VP_TS(10);
    if constexpr (K > 0) {
      if (ti == 0) vc_wait_vmcnt<SCH::xwait_first>();
      else vc_wait_vmcnt<SCH::xwait>();
    } else {
      wait_vmcnt(issued - xmk);
    }
    VP_TS(0);
    lds_barrier();
    VP_TS(1);
    u32x4 rv[2][FN], yv[2][FN];  // residual x and (VE_ACCUM) old xs of this lane's outputs
#pragma unroll
    for (int fp = 0; fp < 2; ++fp)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const int r = wn * WNC + fn * 16 + l16 + h2 + h1;
        const int q = fp * 4 + (g4 & 1) * 2 + (g4 >> 1);
        rv[fp][fn] = *reinterpret_cast<const u32x4*>(xpl + r * 128 + ((q ^ (r & 6)) * 16));
      }
    lds_barrier();
    VP_TS(2);
    for (int e = tid; e < 2 * XROWS * 8; e += NT) {
      u32x4 v = *reinterpret_cast<const u32x4*>(smem + X_OFF + e * 16);
#pragma unroll
      for (int w = 0; w < 4; ++w) v[w] = lrelu_pk(v[w], a.slope);
      *reinterpret_cast<u32x4*>(smem + X_OFF + e * 16) = v;
    }
    VP_TS(3);
    // ---- 2. conv1 (published by its first step's barrier) ----
    int ymk = 0;
    auto accum_loads = [&] {
      // VE_ACCUM: the old-xs rows of this tile's outputs, loaded now and consumed after conv2 (asm, so the
      // counted wait below retires them instead of a compiler vmcnt(0) that would drain the row staging)
      if constexpr ((EF & VE_ACCUM) != 0) {
#pragma unroll
        for (int fp = 0; fp < 2; ++fp)
#pragma unroll
          for (int fn = 0; fn < FN; ++fn) {
            const int i = min(n0 + wn * WNC + fn * 16 + l16, L - 1);
            asm volatile("global_load_dwordx4 %0, %1, off"
                         : "=v"(yv[fp][fn])
                         : "v"(a.y + ((size_t)b * L + i) * C + wm * 64 + fp * 32 + ch16)
                         : "memory");
          }
        issued += 2 * FN;
        ymk = issued;
      }
    };
    if constexpr (K > 0) {
      conv_ct(std::integral_constant<int, 0>{}, smem + X_OFF, XPL, wn * WNC + l16, d, sb, ti == 0, [&](auto mc) {
        if constexpr (decltype(mc)::value == 0) accum_loads();
      });
    } else {
      conv(smem + X_OFF, XPL, wn * WNC + l16, d, accum_loads);
    }
    VP_TS(4);
    // epilogue: lrelu(round(acc + b1)) -> T row j (frame n0 - h2 + j), zero outside [0, L)
#pragma unroll
    for (int fp = 0; fp < 2; ++fp)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const int j = wn * WNC + fn * 16 + l16;
        const int f = n0 - h2 + j;
        const bool ok = f >= 0 && f < Lt;
        uint32_t o[2][2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int fm = 2 * fp + h;
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(par + wm * 64 + fm * 16 + 4 * g4);
          // lrelu(acc + b1) rounded once to bf16 (conv2's operand); zero outside [0, L)
          o[h][0] = ok ? lrelu_pk_f(f32x2{acc[fm][fn][0], acc[fm][fn][1]} + f32x2{b4[0], b4[1]}, a.slope) : 0u;
          o[h][1] = ok ? lrelu_pk_f(f32x2{acc[fm][fn][2], acc[fm][fn][3]} + f32x2{b4[2], b4[3]}, a.slope) : 0u;
        }
        const int q = fp * 4 + (g4 & 1) * 2 + (g4 >> 1);
        *reinterpret_cast<u32x4*>(smem + T_OFF + wm * TPL + j * 128 + ((q ^ (j & 6)) * 16)) = pack16(o);
      }
    VP_TS(5);
    // ---- 3. conv2 ----
    // every wave is past conv1's reads of the row planes: stage the next tile's raw rows into them (K > 0: spread
    // over conv2's first steps, a phantom copy of the last tile after it, so the counts stay constant)
    if constexpr (K > 0) {
      conv_ct(std::integral_constant<int, 1>{}, smem + T_OFF, TPL, wn * WNC + l16, 1, sb, false, [&](auto mc) {
        constexpr int m = decltype(mc)::value;
        if constexpr (m == 0) stage_x_begin(ti + 1);
        vc_for<0, XPW>([&](auto ic) {
          constexpr int i = decltype(ic)::value;
          if constexpr (i * SCH::XSP / XPW == m) stage_x_piece(wave + 8 * i);
        });
      });
      sb = slot_of(sb, SCH::S);
    } else {
      conv(smem + T_OFF, TPL, wn * WNC + l16, 1, [&] {
        if (ti + 1 < nmine) stage_x(ti + 1);
      });
    }
    VP_TS(7);
    // epilogue: + b2 + x [+ xs] [/ nk] -> y [, lrelu(y) -> y2]
    if constexpr ((EF & VE_ACCUM) != 0) {
      if constexpr (K > 0) vc_wait_vmcnt<SCH::accwait>();
      else wait_vmcnt(issued - ymk);
#pragma unroll
      for (int fp = 0; fp < 2; ++fp)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) asm volatile("" : "+v"(yv[fp][fn]));  // no use of yv before the wait
    }
    VP_TS(8);
    const size_t ybase = (size_t)__builtin_amdgcn_readfirstlane(b) * L * C;
    const auto yr = buf_rsrc(a.y + ybase, (unsigned)L * (C * 2));
    const auto y2r = buf_rsrc(((EF & VE_DUAL) ? a.y2 : a.y) + ybase, (unsigned)L * (C * 2));
#pragma unroll
    for (int fp = 0; fp < 2; ++fp)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const int i = wn * WNC + fn * 16 + l16;  // output frame n0 + i
        uint32_t rr[2][2], yy[2][2] = {}, o1[2][2], o2[2][2];  // [X|Y][dword]: x, old xs, y and its activated copy
        unpack16(rv[fp][fn], rr);  // back to the accumulator layout
        if constexpr ((EF & VE_ACCUM) != 0) unpack16(yv[fp][fn], yy);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int fm = 2 * fp + h;
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(par + C + wm * 64 + fm * 16 + 4 * g4);
          // round(acc + b2 + x [+ xs] [/ nk]) and its lrelu (res_out, mt_vconv.h), two channels per packed op
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            res_out<EF | VE_RESID>(f32x2{acc[fm][fn][2 * u], acc[fm][fn][2 * u + 1]}, f32x2{b4[2 * u], b4[2 * u + 1]}, rr[h][u],
                                   yy[h][u], a.div, a.slope, o1[h][u], o2[h][u]);
          }
        }
        const u32x4 y = pack16(o1);
        if constexpr (VP128_BUF) {
          // the utterance's [L][C] output as a buffer: frames past L fall outside it (store dropped), the tile's
          // discarded frames i >= BN get an offset past any range; every lane still stores
          const unsigned vo = i < BN ? (unsigned)(((n0 + i) * C + wm * 64 + fp * 32 + ch16) * 2) : 0x80000000u;
          buf_store16<SP>(y, yr, vo);
          if constexpr ((EF & VE_DUAL) != 0) buf_store16<SP>(pack16(o2), y2r, vo);
          continue;
        }
        const bool ok = i < BN && n0 + i < L;
        const size_t o = ((size_t)b * L + n0 + i) * C + wm * 64 + fp * 32 + ch16;
        *reinterpret_cast<u32x4*>(ok ? a.y + o : a.trash + 8 * lane) = y;
        if constexpr ((EF & VE_DUAL) != 0) *reinterpret_cast<u32x4*>(ok ? a.y2 + o : a.trash + 8 * lane) = pack16(o2);
      }
    issued += 2 * FN * ((EF & VE_DUAL) ? 2 : 1);
    VP_TS(9);
  }
  if constexpr (K > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the phantom DMA lands before the wave ends
  VP_TS(11);
  VP_TS_END(wave, lane);
}

bool vpair128_supported(int k, int d) {
  return k >= 3 && k % 2 == 1 && NF1 - (k - 1) > 0 && NF1 + d * (k - 1) <= XROWS;
}

int launch_vpair128(int ef, const VPairArgs& a, hipStream_t st) {
  ef &= ~VE_Y2ONLY;  // stores y as well (VE_Y2ONLY is an option, mt_vconv.h)
  if (pair_check("vpair128", ef, a, vpair128_supported(a.taps, a.dil))) return -1;
  // the compile-time K loop for k = 3 (mt_vpair_set_kernels bit VPK_CTK128) when its fixed row staging covers R1
  const bool ct3 = a.taps == 3 && (vpair_kernels() & VPK_CTK128) != 0 && NF1 + 2 * a.dil <= 32 * XPW;
  const bool wt = store_policy() == ST_WT;  // the store policy (mt_common.h)
  return pair_launch("vpair128", C, NF1 - (a.taps - 1), ef, a, st, PROBE_TAG_VPAIR128, [&](int G) {
    return pair_with_ef(ef, [&](auto ec) {
      constexpr int E = decltype(ec)::value;
      if (ct3) {
        (void)VpkReg<3, Vp128Sched<E, 3>, E>::reg;
        if (wt) hipLaunchKernelGGL((vpair128_kernel<E, 3, ST_WT>), dim3(G), dim3(NT), 0, st, a);
        else hipLaunchKernelGGL((vpair128_kernel<E, 3>), dim3(G), dim3(NT), 0, st, a);
      }
      else if (wt) hipLaunchKernelGGL((vpair128_kernel<E, 0, ST_WT>), dim3(G), dim3(NT), 0, st, a);
      else hipLaunchKernelGGL((vpair128_kernel<E>), dim3(G), dim3(NT), 0, st, a);
    });
  });
}

VP_TS_BINDER(vpair128_ts_bind)

}  // namespace mt
