// Implicit-GEMM Conv1d kernel for gfx950 (see mt_conv.h for the op coverage).
//
// Workgroup = 256 threads = 4 waves (wave64). Tile = BM output rows x BN output positions.
// Per K-stage (one 64-byte channel chunk = 32 bf16 / 16 f32 channels, and a group of up to
// TG taps) the workgroup stages into LDS
//   Ws[tap][BM][64B]   packed weight rows,
//   Xs[RB][64B]        the input frames the tile needs for all taps of the group (halo
//                      included), with the prologue transform applied once per element,
// then every wave issues FM x FN MFMAs per tap (bf16: v_mfma_f32_16x16x32_bf16, f32: 4 x
// v_mfma_f32_16x16x4_f32 = an exact fp32 fmaf chain). LDS rows are padded to 80 bytes so the
// 16-lane ds_read_b128 groups hit 16 distinct 4-bank slots (conflict-free).
#include "mt_conv.h"
#include "mt_probe.h"

#include <algorithm>
#include <type_traits>

namespace mt {

template <class E>
__device__ __forceinline__ float mish_e(float x) {
  if constexpr (std::is_same<E, float>::value) {
    if (x > 20.f) return x;
    const float e = expf(x);
    const float n = e * (e + 2.f);
    return x * (n / (n + 2.f));
  } else {
    return mish_f(x);
  }
}

// Tile configuration (compile time): BM x BN output tile, WAVES_M x WAVES_N waves, TG taps and
// CK bytes of input channels per K-stage (LDS rows of CK+32 bytes: the 16-row x 4-column MFMA
// fragment reads then hit 16 distinct 16-byte bank slots in every ds_read_b128 lane group, for CK
// in {64,128,256}; CK+16 rows were 2-way conflicted), SMAX = largest stride served. Static LDS: two stage buffers + tables.
template <int BM_, int BN_, int WAVES_M_, int WAVES_N_, int TG_, int CK_, int SMAX_>
struct Tile {
  static constexpr int BM = BM_, BN = BN_, WAVES_M = WAVES_M_, WAVES_N = WAVES_N_, TG = TG_, SMAX = SMAX_;
  static constexpr int CK = CK_, ROW = CK_ + 32, VPR = CK_ / 16, KS = CK_ / 64;
  static constexpr int NT = 64 * WAVES_M * WAVES_N;
  static constexpr int DMAX = 5;  // largest dilation served (HiFi-GAN v1: 1, 3, 5)
  static constexpr int RBMAX = (BN - 1) * SMAX + (TG - 1) * DMAX + 1;
  static constexpr int WS_BYTES = TG * BM * ROW;
  static constexpr int XS_BYTES = RBMAX * ROW;
  static constexpr int BUF_BYTES = WS_BYTES + XS_BYTES;
  static constexpr int TAB_BYTES = (768 + 2 * BN) * 4;
  static constexpr int LDS_BYTES = 2 * BUF_BYTES + TAB_BYTES;
  static constexpr int NWV = (TG * BM * VPR + NT - 1) / NT;  // 16-B weight vectors per thread per stage
  static constexpr int NXV = (RBMAX * VPR + NT - 1) / NT;    // 16-B input vectors per thread per stage
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// TAG only renames the symbol: TAG=1 is the op-level entry (mt_op_conv1d) used by bench.py's
// roofline leg, so its launches get their own rocprof row; the code is identical.
//
// Pipeline per K-stage s (tap group x 64-byte channel chunk), one barrier per stage:
//   issue(s+1): global loads of stage s+1 into registers (addresses clamped, no branches)
//   MFMAs of stage s from LDS buffer s&1
//   commit(s+1): prologue transform + zero padding, ds_write into buffer (s+1)&1
//   __syncthreads()
template <class E, class TL, int PF, int EF, int TAG = 0>
__global__ __launch_bounds__(TL::NT) void conv_kernel(ConvArgs a) {
  constexpr int BM = TL::BM, BN = TL::BN, WAVES_M = TL::WAVES_M, WAVES_N = TL::WAVES_N;
  constexpr int NT = TL::NT, TG = TL::TG;
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int FM = WM / 16, FN = WN / 16;
  constexpr int VN = Vec16<E>::N;                 // elements per 16 bytes
  constexpr int VPR = TL::VPR;                       // 16-B vectors per LDS row
  constexpr int CH = VPR * VN;                       // channels per K-stage
  constexpr int ROWB = TL::ROW;
  constexpr bool NEED_GN = (PF & PF_GN) || (EF & EF_GNADD);

  __shared__ __attribute__((aligned(16))) char smem[TL::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WAVES_M, wn = wave / WAVES_M;
  const int ntiles = (a.Ncols + BN - 1) / BN;
  const int b = blockIdx.x / ntiles, nt = blockIdx.x - b * ntiles;
  const int n0 = nt * BN, m0 = blockIdx.y * BM;
  // ragged batch: this utterance's valid input frames / output frames (whole block uniform)
  const int Lin = a.lens ? min(max(a.lens[b] * a.lmul, 0), a.Tin) : a.Tin;
  const int Lout = a.lens ? min(a.Tout, a.stride > 1 ? Lin / a.stride : Lin * a.ups) : a.Tout;
  if (a.lens && n0 >= Lin + (a.Ncols - a.Tin)) return;  // a tile wholly past the utterance

  float* ga = reinterpret_cast<float*>(smem + 2 * TL::BUF_BYTES);  // [256]
  float* gsh = ga + 256;                                           // [256]
  float* lnm = gsh + 256;                                          // [BN]
  float* lnr = lnm + BN;                                           // [BN]
  float* tbs = lnr + BN;                                           // [256] time-embedding bias

  if constexpr ((PF & PF_TB) != 0) {
    for (int c = tid; c < a.cin; c += NT) tbs[c] = a.tb[(size_t)b * a.tb_ld + c];
    __syncthreads();
  }

  // ---- pre-phase: GroupNorm coefficients for utterance b (merged tile partials) ----
  if constexpr (NEED_GN) {
    const int C = (PF & PF_GN) ? a.cin : a.cout;
    const int G = C >> 5;
    if (tid < 64) {
      // first wave: a power-of-two segment of lanes per group, each summing a strided subset of the group's
      // partials (all loads in flight together), then a butterfly inside the segment (fixed order)
      int lpg = 64;
      while (lpg * G > 64) lpg >>= 1;
      const int g = tid / lpg, sub = tid % lpg;
      double s1 = 0.0, s2 = 0.0;
      if (g < G) {
        const double* p = a.gn_in + (size_t)(b * G + g) * a.gn_ntiles * 2;
        for (int i = sub; i < a.gn_ntiles; i += lpg) {
          s1 += p[2 * i];
          s2 += p[2 * i + 1];
        }
      }
      for (int o = lpg >> 1; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
      }
      if (sub == 0 && g < G) {
        const double n = 32.0 * (double)a.gn_T;
        const double mean = s1 / n;
        double var = s2 / n - mean * mean;
        var = var < 0.0 ? 0.0 : var;
        lnm[g] = (float)mean;
        lnr[g] = (float)(1.0 / sqrt(var + (double)a.gn_eps));
      }
    }
    __syncthreads();
    for (int c = tid; c < C; c += NT) {
      const int g = c >> 5;
      const float sc = lnr[g] * a.gn_g[c];
      ga[c] = sc;
      gsh[c] = -sc * lnm[g] + a.gn_b[c];
    }
    __syncthreads();
  }

  // ---- pre-phase: LayerNorm row statistics of the tile's frames (k=1 GEMMs only) ----
  if constexpr (PF & PF_LN) {
    for (int r = tid; r < BN; r += NT) {
      const int f = n0 + r;
      float mean = 0.f, rstd = 0.f;
      if (f < a.Tin) {
        const float* st = a.ln_stats + ((size_t)b * a.Tin + f) * 2;
        mean = st[0];
        rstd = st[1];
      }
      lnm[r] = mean;
      lnr[r] = rstd;
    }
    __syncthreads();
  }

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const E* x0p = reinterpret_cast<const E*>(a.x0);
  const E* x1p = reinterpret_cast<const E*>(a.x1);
  const E* wp = reinterpret_cast<const E*>(a.w);
  const int c1 = a.cin - a.c0;
  const int nchunks = (a.cin_pad + CH - 1) / CH;
  const int ngroups = (a.taps + TG - 1) / TG;
  const int S = ngroups * nchunks;

  Vec16<E> xr[TL::NXV], wr[TL::NWV];

  // global -> registers for stage s (every load issued, invalid ones from a clamped address)
  auto issue = [&](int s) {
    const int gi = s / nchunks, c = s - gi * nchunks;
    const int tg0 = gi * TG, ntg = min(TG, a.taps - tg0);
    const int RB = (BN - 1) * a.stride + (ntg - 1) * a.dil + 1;
    const int fbase = n0 * a.stride - a.pad + tg0 * a.dil;
    const int cbase = c * CH;
#pragma unroll
    for (int i = 0; i < TL::NXV; ++i) {
      const int v = tid + i * NT;
      const int r = v / VPR, sl = v % VPR;
      int f = fbase + r;
      int ch = cbase + sl * VN;
      const bool ok = (v < RB * VPR) && f >= 0 && f < Lin && ch < a.cin;
      f = ok ? f : 0;
      ch = ok ? ch : 0;
      const size_t row = (size_t)b * a.Tin + f;
      const E* src = (ch < a.c0) ? x0p + row * a.c0 + ch : x1p + row * c1 + (ch - a.c0);
      xr[i] = load16(src);
    }
#pragma unroll
    for (int i = 0; i < TL::NWV; ++i) {
      const int v = tid + i * NT;
      const int rr = v / VPR, sl = v % VPR;
      const int t = rr / BM, m = rr - t * BM;
      const bool ok = (t < ntg) && (m0 + m < a.Mpad) && (cbase + sl * VN < a.cin_pad);
      const size_t off = ok ? ((size_t)(m0 + m) * a.taps + (tg0 + t)) * a.cin_pad + cbase + sl * VN : 0;
      wr[i] = load16(wp + off);
    }
  };

  // registers -> LDS buffer `buf` for stage s (prologue transform, zero padding)
  auto commit = [&](int s, int buf) {
    char* Ws = smem + buf * TL::BUF_BYTES;
    char* Xs = Ws + TL::WS_BYTES;
    const int gi = s / nchunks, c = s - gi * nchunks;
    const int tg0 = gi * TG, ntg = min(TG, a.taps - tg0);
    const int RB = (BN - 1) * a.stride + (ntg - 1) * a.dil + 1;
    const int fbase = n0 * a.stride - a.pad + tg0 * a.dil;
    const int cbase = c * CH;
#pragma unroll
    for (int i = 0; i < TL::NXV; ++i) {
      const int v = tid + i * NT;
      if (v >= RB * VPR) continue;
      const int r = v / VPR, sl = v % VPR;
      const int f = fbase + r;
      const int ch = cbase + sl * VN;
      Vec16<E> val = xr[i];
      if (f < 0 || f >= Lin || ch >= a.cin) {
        val = zero16<E>();
      } else if constexpr (PF != 0) {
        const size_t row = (size_t)b * a.Tin + f;
        float mk = 1.f, lm = 0.f, lr = 1.f;
        if constexpr ((PF & PF_MASK) != 0) mk = a.pmask[row];
        if constexpr ((PF & PF_LN) != 0) {
          lm = lnm[f - n0];
          lr = lnr[f - n0];
        }
#pragma unroll
        for (int k = 0; k < VN; ++k) {
          float x = val.get(k);
          const int cc = ch + k;
          if constexpr ((PF & PF_LN) != 0) x = (x - lm) * lr;  // gamma/beta folded into W, bias
          if constexpr ((PF & PF_GN) != 0) x = mish_e<E>(x * ga[cc] + gsh[cc]);
          if constexpr ((PF & PF_TB) != 0) x = x + tbs[cc];
          if constexpr ((PF & PF_LRELU) != 0) x = lrelu_f(x, a.slope);
          if constexpr ((PF & PF_MASK) != 0) x = x * mk;
          val.set(k, x);
        }
      }
      store16(reinterpret_cast<E*>(Xs + r * ROWB + sl * 16), val);
    }
#pragma unroll
    for (int i = 0; i < TL::NWV; ++i) {
      const int v = tid + i * NT;
      const int rr = v / VPR, sl = v % VPR;
      const int t = rr / BM, m = rr - t * BM;
      if (t >= TG) continue;
      Vec16<E> val = wr[i];
      if (t >= ntg || m0 + m >= a.Mpad || cbase + sl * VN >= a.cin_pad) val = zero16<E>();
      store16(reinterpret_cast<E*>(Ws + rr * ROWB + sl * 16), val);
    }
  };

  // MFMAs of one K-stage; the A/B fragments of step j+1 are read from LDS before the MFMAs of
  // step j are issued (steps = taps x 64-byte K slices), so LDS latency hides under the MFMAs.
  auto compute = [&](int s, int buf) {
    const char* Ws = smem + buf * TL::BUF_BYTES;
    const char* Xs = Ws + TL::WS_BYTES;
    const int gi = s / nchunks;
    const int ntg = min(TG, a.taps - gi * TG);
    const int nsteps = ntg * TL::KS;
    const char* abase = Ws + (wm * WM + (lane & 15)) * ROWB + (lane >> 4) * 16;
    const char* bbase = Xs + ((wn * WN + (lane & 15)) * a.stride) * ROWB + (lane >> 4) * 16;
    auto load_frags = [&](int j, Vec16<E>(&af)[FM], Vec16<E>(&bf)[FN]) {
      const int t = j / TL::KS, ks = j - t * TL::KS;
      const char* ap = abase + t * BM * ROWB + ks * 64;
      const char* bp = bbase + (t * a.dil) * ROWB + ks * 64;
#pragma unroll
      for (int fm = 0; fm < FM; ++fm) af[fm] = load16(reinterpret_cast<const E*>(ap + fm * 16 * ROWB));
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        bf[fn] = load16(reinterpret_cast<const E*>(bp + fn * 16 * a.stride * ROWB));
    };
    auto mma = [&](const Vec16<E>(&af)[FM], const Vec16<E>(&bf)[FN]) {
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) acc[fm][fn] = mfma16(af[fm].v, bf[fn].v, acc[fm][fn]);
    };
    Vec16<E> a0[FM], b0[FN], a1[FM], b1[FN];
    load_frags(0, a0, b0);
#pragma unroll
    for (int j = 0; j < TG * TL::KS; j += 2) {
      if (j >= nsteps) break;
      if (j + 1 < nsteps) load_frags(j + 1, a1, b1);
      mma(a0, b0);
      if (j + 1 >= nsteps) break;
      if (j + 2 < nsteps) load_frags(j + 2, a0, b0);
      mma(a1, b1);
    }
  };

  issue(0);
  commit(0, 0);
  __syncthreads();
  for (int s = 0; s < S; ++s) {
    const bool more = s + 1 < S;
    if (more) issue(s + 1);
    compute(s, s & 1);
    if (more) commit(s + 1, (s + 1) & 1);
    __syncthreads();
  }

  // ---- epilogue ----
  double g1[FM], g2[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) g1[i] = g2[i] = 0.0;

#pragma unroll
  for (int fm = 0; fm < FM; ++fm) {
    const int mr = m0 + wm * WM + fm * 16 + 4 * (lane >> 4);
    if (mr >= a.M) continue;
    const int ph = mr / a.cout;
    const int ch = mr - ph * a.cout;
    bool ok[4];
    float bias4[4], alpha4[4], ibeta4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ok[r] = (mr + r) < a.M;
      bias4[r] = ok[r] ? a.bias[mr + r] : 0.f;
      if constexpr ((EF & EF_SNAKE) != 0) {
        alpha4[r] = ok[r] ? a.snake_alpha[ch + r] : 0.f;
        ibeta4[r] = ok[r] ? a.snake_ibeta[ch + r] : 0.f;
      }
    }
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const int n = n0 + wn * WN + fn * 16 + (lane & 15);
      if (n >= a.Ncols) continue;
      const int fr = n * a.ups + ph - a.opad;
      if (fr < 0 || fr >= Lout) continue;
      const size_t orow = (size_t)b * a.Tout + fr;
      float em = 1.f;
      if constexpr ((EF & (EF_MASK | EF_GNADD | EF_FMASK)) != 0) em = a.emask[orow];
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[fm][fn][r] + bias4[r];
      if constexpr ((EF & EF_RELU) != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      }
      if constexpr ((EF & EF_SNAKE) != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sn;
          if constexpr (std::is_same<E, float>::value) sn = sinf(v[r] * alpha4[r]);
          else sn = __sinf(v[r] * alpha4[r]);
          v[r] = v[r] + ibeta4[r] * (sn * sn);
        }
      }
      if constexpr ((EF & EF_GNSTATS) != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ok[r]) {
            g1[fm] += (double)v[r];
            g2[fm] += (double)v[r] * (double)v[r];
          }
      }
      if constexpr ((EF & EF_GNADD) != 0) {
        const E* gy = reinterpret_cast<const E*>(a.gy) + orow * a.cout + ch;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ok[r]) v[r] = mish_e<E>(to_f(gy[r]) * ga[ch + r] + gsh[ch + r]) * em + v[r];
      }
      if constexpr ((EF & EF_MASK) != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = v[r] * em;
      }
      if constexpr ((EF & EF_RESID) != 0) {
        const E* rp = reinterpret_cast<const E*>(a.resid) + orow * a.ldr + ch;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ok[r]) v[r] = v[r] + to_f(rp[r]);
      }
      if constexpr ((EF & EF_ACCUM) != 0) {
        const E* yp = reinterpret_cast<const E*>(a.y) + orow * a.ldy + ch;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (ok[r]) v[r] = to_f(yp[r]) + v[r];
      }
      if constexpr ((EF & EF_DIV) != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = v[r] / a.div;
      }
      if constexpr ((EF & EF_FMASK) != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = v[r] * em;
      }
      if constexpr ((EF & EF_TANH) != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = tanhf(v[r]);
      }
      if constexpr ((EF & EF_EULER) != 0) {
        E* xz = reinterpret_cast<E*>(a.xin_z) + orow * a.ld_xin + ch;
        float* zp = a.zmaster + orow * a.cout + ch;
        const float dt = a.dt_rows ? a.dt_rows[b] : a.dt;  // orow's utterance, uniform over the tile
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (!ok[r]) continue;
          float inc = v[r] * dt;
          if (a.half_step) inc = inc * 0.5f;
          const float zn = zp[r] + inc;
          if (a.update_master) zp[r] = zn;
          xz[r] = from_f<E>(zn * em);  // the estimator-input slot is read as x * mask only
        }
      } else if constexpr ((EF & EF_OUTF32) != 0) {
        float* yp = reinterpret_cast<float*>(a.y) + orow * a.ldy + ch;
        if (ok[3] && ((a.ldy & 3) == 0)) {
          *reinterpret_cast<f32x4*>(yp) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (ok[r]) yp[r] = v[r];
        }
      } else {
        E* yp = reinterpret_cast<E*>(a.y) + orow * a.ldy + ch;
        if constexpr (std::is_same<E, float>::value) {
          if (ok[3] && ((a.ldy & 3) == 0)) {
            *reinterpret_cast<f32x4*>(yp) = f32x4{v[0], v[1], v[2], v[3]};
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (ok[r]) yp[r] = v[r];
          }
        } else {
          if (ok[3] && ((a.ldy & 3) == 0)) {
            bf16x4 o;
            o[0] = (bf16)v[0];
            o[1] = (bf16)v[1];
            o[2] = (bf16)v[2];
            o[3] = (bf16)v[3];
            *reinterpret_cast<bf16x4*>(yp) = o;
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (ok[r]) yp[r] = (bf16)v[r];
          }
        }
        if constexpr ((EF & EF_DUAL) != 0) {
          E* y2p = reinterpret_cast<E*>(a.y2) + orow * a.ldy + ch;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (ok[r]) y2p[r] = from_f<E>(lrelu_f(to_f(from_f<E>(v[r])), a.slope));
        }
      }
    }
  }

  // ---- GroupNorm partial statistics of this tile: [b][group][nt] ----
  if constexpr ((EF & EF_GNSTATS) != 0) {
    static_assert(WM >= 32, "GN stats need >= 32 rows per wave");
    __syncthreads();
    double* red = reinterpret_cast<double*>(smem);  // [NWAVES][FM][2]
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
      const double s1 = wave_sum_d(g1[fm]);
      const double s2 = wave_sum_d(g2[fm]);
      if (lane == 0) {
        red[(wave * FM + fm) * 2] = s1;
        red[(wave * FM + fm) * 2 + 1] = s2;
      }
    }
    __syncthreads();
    constexpr int LG = BM / 32;
    if (tid < LG) {
      const int wmg = (tid * 32) / WM;
      const int fmg = ((tid * 32) % WM) / 16;
      double s1 = 0.0, s2 = 0.0;
      for (int w2 = 0; w2 < WAVES_N; ++w2) {
        const int wv = wmg + w2 * WAVES_M;
        for (int q = 0; q < 2; ++q) {
          s1 += red[(wv * FM + fmg + q) * 2];
          s2 += red[(wv * FM + fmg + q) * 2 + 1];
        }
      }
      const int G = a.M >> 5;
      const int g = (m0 >> 5) + tid;
      if (g < G) {
        double* o = a.gn_out + ((size_t)(b * G + g) * ntiles + nt) * 2;
        o[0] = s1;
        o[1] = s2;
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// The decoder's last launch per evaluation: final_proj (1x1, 256 -> n_feats) of the final block's
// mish(GroupNorm(conv)) * mask, times the mask, and the ODE update z += dt * v (model.py Decoder.forward's
// final_block / final_proj, flow_matching.py solve_euler; the midpoint solver's half step). The generic
// conv_kernel<bf16, TG6, PF_GN | PF_MASK, EF_MASK | EF_EULER> stages 128 x 128 tiles through LDS with the
// GroupNorm + Mish transform in its commit phase, two K stages and no overlap: 30 us per launch at B = 32,
// 174 us at B = 256 (≈ 0.55 TB/s on a 95 MB operand). Here each lane transforms in registers exactly the
// 8-channel pieces it hands the MFMA (B operand: frame lane & 15, channels 32 ks + 8 (lane >> 4)), the
// n_feats x 256 weight image is staged in LDS once per workgroup, and nothing else goes through LDS.
// Workgroup: 4 waves x 16 frames of one utterance; grid (ceil(T / 64), B). Same operations in the same
// order as the generic kernel (GroupNorm merge, transform, bf16 rounding, K order 0..255 from a zero
// accumulator, bias, mask, update): bit-identical results.
constexpr int PJ_C = 256;
constexpr int PJ_ROW = PJ_C * 2 + 16;  // LDS row bytes: a fragment's 16 rows hit 16 distinct 16-byte bank slots

template <int MB, int SP = ST_PLAIN>  // n_feats = 16 * MB; SP: the store policy of the 16-byte z master store (mt_common.h)
__global__ __launch_bounds__(256) void proj_euler_kernel(ConvArgs a) {
  __shared__ __attribute__((aligned(16))) char wl[16 * MB * PJ_ROW];
  __shared__ float ga[PJ_C], gsh[PJ_C], lnm[8], lnr[8];
  constexpr int NWP = (16 * MB * (PJ_C / 8) + 255) / 256;  // 16-byte weight pieces per thread
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
  const int b = blockIdx.y, T = a.Tin;
  const int f = blockIdx.x * 64 + wave * 16 + (lane & 15);
  const bool fok = f < T;
  const size_t row = (size_t)b * T + (fok ? f : T - 1);
  // every global load first: the lane's 8 operand pieces, this thread's share of the weight image, the masks
  const bf16* xp = reinterpret_cast<const bf16*>(a.x0) + row * PJ_C + 8 * kq;
  Vec16<bf16> xv[PJ_C / 32];
#pragma unroll
  for (int ks = 0; ks < PJ_C / 32; ++ks) xv[ks] = load16(xp + 32 * ks);
  const bf16* wp = reinterpret_cast<const bf16*>(a.w);
  Vec16<bf16> wv[NWP];
#pragma unroll
  for (int i = 0; i < NWP; ++i) {
    const int v = min(tid + 256 * i, 16 * MB * (PJ_C / 8) - 1);
    wv[i] = load16(wp + (size_t)(v / (PJ_C / 8)) * a.cin_pad + (v % (PJ_C / 8)) * 8);
  }
  const float mk = a.pmask[row], em = a.emask[row];
  // GroupNorm coefficients of utterance b (conv_kernel's pre-phase, same merge order)
  {
    constexpr int G = PJ_C >> 5;
    if (tid < 64) {
      int lpg = 64;
      while (lpg * G > 64) lpg >>= 1;
      const int g = tid / lpg, sub = tid % lpg;
      double s1 = 0.0, s2 = 0.0;
      if (g < G) {
        const double* p = a.gn_in + (size_t)(b * G + g) * a.gn_ntiles * 2;
        for (int i = sub; i < a.gn_ntiles; i += lpg) {
          s1 += p[2 * i];
          s2 += p[2 * i + 1];
        }
      }
      for (int o = lpg >> 1; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
      }
      if (sub == 0 && g < G) {
        const double n = 32.0 * (double)a.gn_T;
        const double mean = s1 / n;
        double var = s2 / n - mean * mean;
        var = var < 0.0 ? 0.0 : var;
        lnm[g] = (float)mean;
        lnr[g] = (float)(1.0 / sqrt(var + (double)a.gn_eps));
      }
    }
    __syncthreads();
    for (int c = tid; c < PJ_C; c += 256) {
      const int g = c >> 5;
      const float sc = lnr[g] * a.gn_g[c];
      ga[c] = sc;
      gsh[c] = -sc * lnm[g] + a.gn_b[c];
    }
  }
#pragma unroll
  for (int i = 0; i < NWP; ++i) {
    const int v = tid + 256 * i;
    if (v < 16 * MB * (PJ_C / 8))
      store16(reinterpret_cast<bf16*>(wl + (v / (PJ_C / 8)) * PJ_ROW + (v % (PJ_C / 8)) * 16), wv[i]);
  }
  __syncthreads();
  // operand: mish(GroupNorm(x)) * mask, rounded to bf16 (the generic kernel's commit transform)
#pragma unroll
  for (int ks = 0; ks < PJ_C / 32; ++ks) {
    Vec16<bf16> val = xv[ks];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int cc = 32 * ks + 8 * kq + k;
      float x = val.get(k);
      x = mish_e<bf16>(x * ga[cc] + gsh[cc]);
      x = x * mk;
      val.set(k, x);
    }
    xv[ks] = val;
  }
  f32x4 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const char* abase = wl + (lane & 15) * PJ_ROW + kq * 16;
#pragma unroll
  for (int ks = 0; ks < PJ_C / 32; ++ks)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const Vec16<bf16> af = load16(reinterpret_cast<const bf16*>(abase + mb * 16 * PJ_ROW + ks * 64));
      acc[mb] = mfma16(af.v, xv[ks].v, acc[mb]);
    }
  if (!fok) return;
  // epilogue (conv_kernel's EF_MASK | EF_EULER): rows 16 mb + 4 (lane >> 4) + r of frame f
  const size_t orow = (size_t)b * a.Tout + f;
  const float dt = a.dt_rows ? a.dt_rows[b] : a.dt;  // b is the workgroup's utterance: one uniform load
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int ch = 16 * mb + 4 * kq;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = acc[mb][r] + a.bias[ch + r];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = v[r] * em;
    bf16* xz = reinterpret_cast<bf16*>(a.xin_z) + orow * a.ld_xin + ch;
    float* zp = a.zmaster + orow * a.cout + ch;
    const f32x4 z4 = *reinterpret_cast<const f32x4*>(zp);
    f32x4 zn4;
    bf16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float inc = v[r] * dt;
      if (a.half_step) inc = inc * 0.5f;
      const float zn = z4[r] + inc;
      zn4[r] = zn;
      o[r] = (bf16)(zn * em);  // the estimator-input slot is read as x * mask only
    }
    if (a.update_master) {
      if constexpr (SP != ST_PLAIN)  // the same store through the utterance's fp32 [T][80] master rows as a buffer
        buf_store16<SP>(__builtin_bit_cast(u32x4, zn4),
                        buf_rsrc(a.zmaster + (size_t)b * a.Tout * a.cout, (unsigned)a.Tout * (unsigned)a.cout * 4u),
                        (unsigned)((f * a.cout + ch) * 4));
      else
        *reinterpret_cast<f32x4*>(zp) = zn4;
    }
    *reinterpret_cast<bf16x4*>(xz) = o;  // 8 bytes per lane: plain under every policy
  }
}

bool proj_euler_supported(const ConvArgs& a) {
  return a.taps == 1 && a.stride == 1 && a.pad == 0 && a.ups == 1 && a.cin == PJ_C && a.c0 == PJ_C &&
         a.cin_pad == PJ_C && a.M == 80 && a.cout == 80 && a.Tout == a.Tin && a.Ncols == a.Tin && !a.lens &&
         a.ld_xin % 4 == 0 && a.gn_ntiles > 0;
}

int launch_proj_euler(const ConvArgs& a, hipStream_t stream) {
  MT_REQUIRE(proj_euler_supported(a), "proj_euler: geometry (1x1, 256 -> 80, no ragged lengths)");
  MT_REQUIRE(a.x0 && a.w && a.bias && a.pmask && a.emask && a.gn_in && a.gn_g && a.gn_b && a.zmaster && a.xin_z,
             "proj_euler: null pointer");
  MT_REQUIRE((reinterpret_cast<uintptr_t>(a.zmaster) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.xin_z) & 7) == 0,
             "proj_euler: z / estimator-input alignment");
  // the store policy (mt_common.h); its buffer store addresses an utterance's master rows with 32-bit byte offsets
  const bool wt = store_policy() == ST_WT && (long long)a.Tout * a.cout * 4 < (1ll << 31);
  const auto kern = wt ? proj_euler_kernel<5, ST_WT> : proj_euler_kernel<5>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((a.Tin + 63) / 64), (unsigned)a.B), dim3(256), 0, stream, a);
  MT_CHECK_HIP(hipGetLastError());
  // launch log (tests/test_gpu_decoder_kernels.py: the dedicated kernel, not the generic conv, ran): tag 0x20000
  const int rec[VCLOG_FIELDS] = {0x20000, 80, 64, 1, (a.Tin + 63) / 64 * a.B, (a.Tin + 63) / 64 * a.B, 1, 80, PJ_C,
                                 a.B, a.Tin};
  vclog_record(rec);
  return 0;
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
enum : int { CFG_BIG = 1, CFG_SMALLN = 2, CFG_64 = 4, CFG_32 = 8, CFG_16 = 16, CFG_G6 = 32, CFG_C5 = 64 };

// every tile is 8 waves (512 threads): 2 waves per SIMD at one workgroup per CU
using TConv = Tile<128, 256, 2, 4, 4, 64, 1>;    // k >= 3 convs: 4 taps x 32 bf16 channels per stage
using TConvT = Tile<128, 256, 2, 4, 2, 64, 1>;   // 2-tap polyphase ConvTranspose
using TGemm = Tile<128, 256, 2, 4, 1, 128, 1>;   // 1x1 (Linear) GEMMs: 64 bf16 channels per stage
using TSmall = Tile<128, 128, 2, 4, 2, 64, 2>;   // stride-2 conv or too few column tiles
using TG6 = Tile<128, 128, 2, 4, 1, 256, 1>;     // 1x1 GEMMs with K >= 512 or M <= 384 (decoder): 256-byte stages
using TC5 = Tile<128, 128, 2, 4, 4, 64, 1>;      // k >= 3 convs whose 128x256 grid would leave CUs idle
using T64x256 = Tile<64, 512, 1, 8, 4, 64, 1>;   // wave tile 64x64 (HiFi-GAN 64-channel stage)
using T32x256 = Tile<32, 512, 1, 8, 4, 64, 1>;   // wave tile 32x64 (32-channel stage)
using T16x256 = Tile<16, 512, 1, 8, 4, 64, 1>;   // wave tile 16x64 (conv_post, M = 1)

// tile variants for in-process A/B timing of the op-level entry (mt_op_conv1d_tile)
using V1 = Tile<128, 256, 2, 4, 4, 64, 1>;
using V2 = Tile<128, 128, 2, 4, 2, 128, 1>;
using V3 = Tile<128, 512, 2, 4, 2, 64, 1>;
using V4 = Tile<128, 256, 2, 4, 3, 64, 1>;
using V5 = Tile<128, 128, 2, 4, 4, 64, 1>;
using V6 = Tile<128, 128, 2, 4, 1, 256, 1>;
using V7 = Tile<128, 128, 2, 2, 2, 64, 1>;   // 4 waves, 77 KB: two workgroups per CU
using V8 = Tile<64, 128, 2, 2, 4, 64, 1>;    // 4 waves, 79 KB: two workgroups per CU
using V9 = Tile<64, 256, 2, 4, 2, 64, 1>;    // 8 waves, 78 KB: two workgroups per CU
using V10 = Tile<128, 128, 2, 2, 4, 64, 1>;  // 4 waves, one workgroup per CU
using V13 = Tile<64, 128, 2, 2, 1, 128, 1>;  // 4 waves, 64 KB: 1x1 GEMMs, two workgroups per CU
using V14 = Tile<64, 64, 2, 2, 1, 128, 1>;   // 4 waves, 1x1 GEMMs, small tiles
using V15 = Tile<128, 64, 2, 2, 1, 128, 1>;  // 4 waves

template <class E, class TL, int PF, int EF, int TAG = 0>
static int launch_tile(const ConvArgs& a, hipStream_t stream, int* ntiles_out) {
  const int ntg = std::min(a.taps, TL::TG);
  const int RB = (TL::BN - 1) * a.stride + (ntg - 1) * a.dil + 1;
  MT_REQUIRE(a.stride <= TL::SMAX && RB <= TL::RBMAX,
             "conv: stride %d / dilation %d exceed the tile's static bounds", a.stride, a.dil);
  const int ntiles = (a.Ncols + TL::BN - 1) / TL::BN;
  dim3 grid((unsigned)(ntiles * a.B), (unsigned)((a.M + TL::BM - 1) / TL::BM));
  hipLaunchKernelGGL((conv_kernel<E, TL, PF, EF, TAG>), grid, dim3(TL::NT), 0, stream, a);
  MT_CHECK_HIP(hipGetLastError());
  if (ntiles_out) *ntiles_out = ntiles;
  return 0;
}

static int check_args(const ConvArgs& a, int esize, int pf, int ef) {
  const int VN = 16 / esize, CH = 64 / esize;
  MT_REQUIRE(a.B > 0 && a.Tin > 0 && a.Tout > 0 && a.Ncols > 0, "conv: empty geometry");
  MT_REQUIRE(a.cin % VN == 0 && a.c0 % VN == 0 && a.c0 <= a.cin && a.c0 > 0,
             "conv: channel split %d/%d not 16-byte aligned", a.c0, a.cin);
  MT_REQUIRE(a.cin_pad % CH == 0 && a.cin_pad >= a.cin, "conv: cin_pad %d", a.cin_pad);
  MT_REQUIRE(a.Mpad >= a.M && a.M > 0 && a.cout > 0 && a.M % a.cout == 0, "conv: M %d cout %d", a.M,
             a.cout);
  MT_REQUIRE(a.taps >= 1 && a.dil >= 1 && a.stride >= 1 && a.ups >= 1, "conv: taps/dil/stride");
  MT_REQUIRE(a.x0 && a.w && a.bias && (a.y || (ef & EF_EULER)), "conv: null pointer");
  MT_REQUIRE(!(ef & EF_DUAL) || a.y2, "conv: y2 missing");
  MT_REQUIRE(a.c0 == a.cin || a.x1, "conv: second source missing");
  if (pf & PF_LN) MT_REQUIRE(a.taps == 1 && a.stride == 1 && a.pad == 0 && a.ln_stats,
                             "conv: LN prologue needs a 1x1 GEMM and row statistics");
  if (pf & PF_GN) MT_REQUIRE(a.cin <= 256 && a.cin % 32 == 0 && a.gn_in, "conv: GN prologue");
  if (ef & EF_GNADD) MT_REQUIRE(a.cout <= 256 && a.cout % 32 == 0 && a.gn_in && a.gy, "conv: GN epilogue");
  if (ef & EF_GNSTATS) MT_REQUIRE(a.M % 32 == 0 && a.gn_out && a.ups == 1, "conv: GN stats");
  if (pf & PF_MASK) MT_REQUIRE(a.pmask, "conv: pmask");
  if (ef & (EF_MASK | EF_GNADD | EF_FMASK)) MT_REQUIRE(a.emask, "conv: emask");
  if (ef & EF_RESID) MT_REQUIRE(a.resid, "conv: resid");
  if (ef & EF_EULER) MT_REQUIRE(a.zmaster && a.xin_z, "conv: euler buffers");
  if (ef & EF_SNAKE) MT_REQUIRE(a.snake_alpha && a.snake_ibeta, "conv: snake params");
  return 0;
}

template <class E, int PF, int EF, int CFGS, int TAG = 0>
static int launch_sel(const ConvArgs& a, hipStream_t stream, int* ntiles_out) {
  int rc = check_args(a, (int)sizeof(E), PF, EF);
  if (rc) return rc;
  const int M = a.M;
  if constexpr ((CFGS & CFG_16) != 0)
    if (M <= 16) return launch_tile<E, T16x256, PF, EF, TAG>(a, stream, ntiles_out);
  if constexpr ((CFGS & CFG_32) != 0)
    if (M <= 32) return launch_tile<E, T32x256, PF, EF, TAG>(a, stream, ntiles_out);
  if constexpr ((CFGS & CFG_64) != 0)
    if (M <= 64) return launch_tile<E, T64x256, PF, EF, TAG>(a, stream, ntiles_out);
  if constexpr ((CFGS & CFG_BIG) != 0) {
    const long wgs = (long)a.B * ((a.Ncols + 255) / 256) * ((M + 127) / 128);
    // choices measured in-process on the decoder's shapes (tools_ab_gemm.py, B=32, T=728)
    if constexpr ((CFGS & CFG_G6) != 0)
      if (a.stride == 1 && a.taps == 1 && (a.cin >= 512 || M <= 384))
        return launch_tile<E, TG6, PF, EF, TAG>(a, stream, ntiles_out);
    if constexpr ((CFGS & CFG_C5) != 0)
      if (a.stride == 1 && a.taps >= 3 && wgs < 192 && !a.fixed_tile)
        return launch_tile<E, TC5, PF, EF, TAG>(a, stream, ntiles_out);
    if (a.stride == 1 && (wgs >= 192 || a.fixed_tile || (CFGS & CFG_SMALLN) == 0)) {
      if (a.taps == 1) return launch_tile<E, TGemm, PF, EF, TAG>(a, stream, ntiles_out);
      if (a.taps == 2) return launch_tile<E, TConvT, PF, EF, TAG>(a, stream, ntiles_out);
      return launch_tile<E, TConv, PF, EF, TAG>(a, stream, ntiles_out);
    }
  }
  if constexpr ((CFGS & CFG_SMALLN) != 0) return launch_tile<E, TSmall, PF, EF, TAG>(a, stream, ntiles_out);
  set_error("conv: no tile configuration for M=%d (pf %d ef %d)", M, PF, EF);
  return -1;
}

// (PF, EF, tile configs) combinations used by the decoder and the vocoder.
#define MT_CONV_COMBOS(X)                                                              \
  X(PF_MASK, EF_GNSTATS, CFG_BIG | CFG_SMALLN | CFG_G6 | CFG_C5)                                     \
  X(PF_GN | PF_TB | PF_MASK, EF_GNSTATS, CFG_BIG | CFG_SMALLN | CFG_G6 | CFG_C5)                     \
  X(PF_MASK, EF_GNADD, CFG_BIG | CFG_SMALLN | CFG_G6 | CFG_C5)                                       \
  X(PF_LN, 0, CFG_BIG | CFG_SMALLN | CFG_G6 | CFG_C5)                                                \
  X(0, EF_RESID, CFG_BIG | CFG_SMALLN | CFG_64 | CFG_32 | CFG_G6 | CFG_C5)                   \
  X(PF_LN, EF_SNAKE, CFG_BIG | CFG_SMALLN | CFG_G6 | CFG_C5)                                         \
  X(PF_MASK, 0, CFG_BIG | CFG_SMALLN | CFG_G6 | CFG_C5)                                              \
  X(PF_GN | PF_MASK, EF_MASK | EF_EULER, CFG_BIG | CFG_SMALLN | CFG_G6 | CFG_C5)                     \
  X(0, 0, CFG_BIG | CFG_SMALLN | CFG_64 | CFG_32 | CFG_16)             \
  X(PF_LRELU, 0, CFG_BIG | CFG_SMALLN | CFG_64 | CFG_32 | CFG_16)      \
  X(PF_LRELU, EF_RESID, CFG_BIG | CFG_SMALLN | CFG_64 | CFG_32)            \
  X(PF_LRELU, EF_RESID | EF_ACCUM, CFG_BIG | CFG_SMALLN | CFG_64 | CFG_32) \
  X(PF_LRELU, EF_RESID | EF_ACCUM | EF_DIV,                                            \
    CFG_BIG | CFG_SMALLN | CFG_64 | CFG_32)                                \
  X(PF_LRELU, EF_RESID | EF_DIV, CFG_BIG | CFG_SMALLN | CFG_64 | CFG_32)   \
  X(PF_LRELU, EF_TANH | EF_OUTF32, CFG_16 | CFG_32)                                     \
  X(PF_LRELU, EF_DUAL, CFG_BIG | CFG_SMALLN)                                            \
  X(0, EF_RESID | EF_FMASK, CFG_BIG | CFG_SMALLN | CFG_G6)                               \
  X(0, EF_RELU, CFG_BIG | CFG_SMALLN | CFG_C5)                                           \
  X(0, EF_RELU | EF_MASK, CFG_BIG | CFG_SMALLN | CFG_C5)                                 \
  X(0, EF_MASK | EF_RESID, CFG_BIG | CFG_SMALLN | CFG_C5)                                \
  X(0, EF_MASK, CFG_BIG | CFG_SMALLN | CFG_G6)                                           \
  X(0, EF_DUAL, CFG_BIG | CFG_SMALLN)                                                    \
  X(0, EF_MASK | EF_OUTF32, CFG_16 | CFG_32)

#define MT_DEFINE_LAUNCH(PFV, EFV, CFGV)                                                    \
  template <>                                                                             \
  int launch_conv<float, (PFV), (EFV)>(const ConvArgs& a, hipStream_t s, int* nt) {        \
    return launch_sel<float, (PFV), (EFV), (CFGV)>(a, s, nt);                              \
  }                                                                                       \
  template <>                                                                             \
  int launch_conv<bf16, (PFV), (EFV)>(const ConvArgs& a, hipStream_t s, int* nt) {         \
    return launch_sel<bf16, (PFV), (EFV), (CFGV)>(a, s, nt);                               \
  }
MT_CONV_COMBOS(MT_DEFINE_LAUNCH)

template <class E, int PF>
static int launch_variant(int variant, const ConvArgs& a, hipStream_t stream) {
  int rc = check_args(a, (int)sizeof(E), PF, 0);
  if (rc) return rc;
  switch (variant) {
    case 0: return launch_tile<E, TConvT, PF, 0, 1>(a, stream, nullptr);
    case 1: return launch_tile<E, V1, PF, 0, 1>(a, stream, nullptr);
    case 2: return launch_tile<E, V2, PF, 0, 1>(a, stream, nullptr);
    case 3: return launch_tile<E, V3, PF, 0, 1>(a, stream, nullptr);
    case 4: return launch_tile<E, V4, PF, 0, 1>(a, stream, nullptr);
    case 5: return launch_tile<E, V5, PF, 0, 1>(a, stream, nullptr);
    case 6: return launch_tile<E, V6, PF, 0, 1>(a, stream, nullptr);
    case 7: return launch_tile<E, V7, PF, 0, 1>(a, stream, nullptr);
    case 8: return launch_tile<E, V8, PF, 0, 1>(a, stream, nullptr);
    case 9: return launch_tile<E, V9, PF, 0, 1>(a, stream, nullptr);
    case 10: return launch_tile<E, V10, PF, 0, 1>(a, stream, nullptr);
    case 11: return launch_tile<E, TGemm, PF, 0, 1>(a, stream, nullptr);
    case 12: return launch_tile<E, TSmall, PF, 0, 1>(a, stream, nullptr);
    case 13: return launch_tile<E, V13, PF, 0, 1>(a, stream, nullptr);
    case 14: return launch_tile<E, V14, PF, 0, 1>(a, stream, nullptr);
    case 15: return launch_tile<E, V15, PF, 0, 1>(a, stream, nullptr);
    default: set_error("conv: unknown tile variant %d", variant); return -1;
  }
}

int launch_conv_op(int dtype, int pf, const ConvArgs& a, hipStream_t stream, int variant) {
  if (variant >= 0) {
    MT_REQUIRE(pf == PF_LRELU, "conv: tile variants are compiled for the lrelu prologue only");
    return dtype == BF16 ? launch_variant<bf16, PF_LRELU>(variant, a, stream)
                         : launch_variant<float, PF_LRELU>(variant, a, stream);
  }
  constexpr int ALL = CFG_BIG | CFG_SMALLN | CFG_64 | CFG_32 | CFG_16;
  if (pf == PF_LRELU)
    return dtype == BF16 ? launch_sel<bf16, PF_LRELU, 0, ALL, 1>(a, stream, nullptr)
                         : launch_sel<float, PF_LRELU, 0, ALL, 1>(a, stream, nullptr);
  return dtype == BF16 ? launch_sel<bf16, 0, 0, ALL, 1>(a, stream, nullptr)
                       : launch_sel<float, 0, 0, ALL, 1>(a, stream, nullptr);
}

int launch_conv_dyn(int dtype, int pf, int ef, const ConvArgs& a, hipStream_t stream, int* nt) {
#define MT_DYN_CASE(PFV, EFV, CFGV)                                                        \
  if (pf == (PFV) && ef == (EFV))                                                          \
    return dtype == BF16 ? launch_conv<bf16, (PFV), (EFV)>(a, stream, nt)                   \
                         : launch_conv<float, (PFV), (EFV)>(a, stream, nt);
  MT_CONV_COMBOS(MT_DYN_CASE)
#undef MT_DYN_CASE
  set_error("conv: prologue/epilogue combination pf=%d ef=%d is not compiled in", pf, ef);
  return -1;
}

}  // namespace mt
