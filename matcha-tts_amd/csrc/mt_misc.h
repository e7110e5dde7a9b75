#pragma once
#include "mt_common.h"

namespace mt {

// solver evaluation times, passed by value to the time-embedding kernel
struct TimeSched {
  static constexpr int MAX = 128;
  float t[MAX];
};

int pack_conv(int dtype, const float* W, int kind, int cout, int cin, int k, int s, int row0, int Mrows,
              int Mpad, int taps, int cin_pad, void* out, hipStream_t st, const float* colscale = nullptr);
int rowstats(int dtype, const void* x, int rows, int C, float eps, float* stats, hipStream_t st);
int fold_bias(const float* W, const float* beta, int M, int K, float* out, hipStream_t st);
int pack_vec(const float* src, int period, int n, int op, float* out, hipStream_t st);

// scale_rows (optional, [B] in device memory): utterance b is scaled by scale_rows[b] instead of scale
int bct_to_btc(int dtype, const float* src, int B, int C, int T, float scale, void* dst, int ld, int coff,
               hipStream_t st, const float* scale_rows = nullptr);
int btc_to_bct(int dtype, const void* src, int ld, int coff, int B, int C, int T, float* dst,
               hipStream_t st);
// Seeded noise (mt_noise.hip): the value at (seeds[b], channel, frame) times temp[b] (temp NULL: 1), a pure function
// of those. noise_fill: z [B][C][T] fp32, C % 4 == 0. noise_fill_decoder: the estimator's 80 channels into both
// workspace layouts at once, zm [B][T][80] fp32 and columns 0 .. 79 of xin [B][T][ld] (element type by dtype, the
// rounding of zm's value).
int noise_fill(const long long* seeds, const float* temp, int B, int C, int T, float* z, hipStream_t st);
int noise_fill_decoder(int dtype, const long long* seeds, const float* temp, int B, int T, float* zm, void* xin,
                       int ld, hipStream_t st);
int spk_fill(int dtype, const float* spks, int B, int C, int T, void* dst, int ld, int coff, hipStream_t st);
int mask_half(const float* m0, int B, int T0, float* m1, hipStream_t st);
// dst[r][0..C) = src[r][0..C) (row strides ld_src / ld_dst, element type by dtype)
int copy_rows(int dtype, const void* src, int ld_src, int rows, int C, void* dst, int ld_dst, hipStream_t st);
// x[r][c] *= mask[r]
int mask_rows(int dtype, void* x, int rows, int C, const float* mask, hipStream_t st);

// Mel infill: the kept frames of the first `rows` utterances are set to the conditional path
// p = (1 - (1 - sigma_min) t) z0 + t x1 (p = x1 itself at t == 1) at t = t_rows[b]: the fp32 master zm [B][T][80]
// (only when update_master) and columns 0 .. 79 of the estimator input xin [B][T][ld] (element type by dtype, p * mask).
// z0, x1: fp32 [B][T][80]; keep: uint8 [B][T]; a frame is kept when keep != 0 and mask != 0, so padded frames are
// neither read nor written. one_m_sigma = 1 - sigma_min. ld % 4 == 0. One launch of infill_clamp_kernel.
int infill_clamp(int dtype, const float* z0, const float* x1, const unsigned char* keep, const float* mask,
                 const float* t_rows, float one_m_sigma, int rows, int T, int update_master, float* zm, void* xin,
                 int ld, hipStream_t st);
// launch-log tag of infill_clamp (the record's ef field, family VCLOG_CONV like proj_euler's; B = rows, L = T)
enum : int { INFILL_LOG = 0x1000000 };

// ResnetBlock1D block tail (GroupNorm(8) -> Mish [-> + time bias] -> * mask, model.py Block1D/ResnetBlock1D)
// for bf16 rows y[b][t][C] whose GroupNorm partial sums (fp64 (sum, sumsq) per (b, 32-channel group,
// part), nparts per group) a conv epilogue produced: h = (mish(y * ga[b,c] + gs[b,c]) + tb[c]) * mask[b,t]
// tb_ld: elements between utterances' time biases (0: one shared vector)
int gn_apply(const void* y, int B, int T, int C, const double* part, int nparts, const float* gamma,
             const float* beta, float eps, const float* tb, int tb_ld, const float* mask, void* h, hipStream_t st);

// t_dev (optional): the S times in device memory instead of ts
int sinus_embed(const TimeSched& ts, int S, const float* freq, int half, float* emb, hipStream_t st,
                const float* t_dev = nullptr);
int rowdot(const float* x, int ldx, const float* W, const float* bias, float* y, int ldy, int yoff, int S,
           int O, int I, int pre, int post, hipStream_t st);
// n segments of O outputs each, segment j: y[s][yoff[j] + o] = post(b[j][o] + W[j][o] . pre(x[s])), one launch
constexpr int ROWDOT_MAXSEG = 8;
struct RowdotSegs {
  const float* W[ROWDOT_MAXSEG];
  const float* b[ROWDOT_MAXSEG];
  int yoff[ROWDOT_MAXSEG];
  int n;
};
int rowdot_segs(const float* x, int ldx, const RowdotSegs& sg, float* y, int ldy, int S, int O, int I, int pre,
                int post, hipStream_t st);

// ls_dev (optional): one length scale per utterance, [B] in device memory, read in place of ls
int durations(const float* logw, const float* xmask, float ls, int B, int Tx, float* w_ceil, float* cum,
              long long* ylen, hipStream_t st, const float* ls_dev = nullptr);
// per-token scale ts [B][Tx] (optional) on top of ls_dev, or given frame counts dur_in [B][Tx] (then logw may be
// NULL); bad (optional, device int): 1 when a count is negative / not finite / fractional or a row reaches 2^24
int durations_tokens(const float* logw, const float* xmask, const float* ls_dev, const float* ts, const float* dur_in,
                     int B, int Tx, float* w_ceil, float* cum, long long* ylen, int* bad, hipStream_t st);
int alignment(const float* cum, const long long* ylen, int B, int Tx, int T, const float* mu, int C, float* attn,
              float* mu_y, float* y_mask, hipStream_t st);
// Forced aligner (mt_align.hip): direct-form log-prior + textbook MAS -> frames per token
size_t align_workspace_bytes(int B, int C, int Tx, int Ty);
int align(const float* mu, const float* y, const float* mean, const float* stdv, const int* t_xs, const int* t_ys,
          int B, int C, int Tx, int Ty, long long* durations, float* log_prior, float* paths, void* ws,
          size_t ws_bytes, hipStream_t st);
int denorm_crop(const float* z, const float* mean, const float* stdv, int B, int C, int T, int Ty, float* mel,
                hipStream_t st);

// part (optional): key-split slots (attention_part_bytes, sized for the largest T launched on it);
// with it an unpadded utterance's keys are split over several workgroups + a merge launch
// Monotonic Alignment Search (mt_mas.hip, train_standalone.py:280-325)
size_t mas_workspace_bytes(int B, int Tx, int Ty);
int maximum_path(const float* value, const int* t_xs, const int* t_ys, int B, int Tx, int Ty, float* out,
                 void* ws, size_t ws_bytes, hipStream_t st);

int launch_attention(int dtype, const void* qkv, const float* mask, void* out, int B, int T, int heads,
                     hipStream_t stream, float* part = nullptr);
size_t attention_part_bytes(int B, int T, int heads);
// query-independent attention + out-projection + residual of utterances that ALL have padded frames at this
// level (the reference's mask fill, model.py:697; mt_attn.hip): x [B][T][256] bf16 updated in place to x + attn1(x),
// row_out [B*T][4][2] the per-slab (mean, M2) of the result; wqkv / bqkv the LN-folded QKV vconv image (mq = 384
// rows) and bias, wout / bout the out-projection image and bias; part: uniform_attention_floats(B) floats.
// Three launches: masked sums of the normalised rows over uniform_part_slices(T) frame slices per utterance; per
// utterance the merge and the two GEMVs (o_b); x += o_b with the row statistics over the same slices.
constexpr int UNI_PSMAX = 32;  // most masked-sum slices per utterance (the workspace holds B x 32 x 260 floats)
int uniform_part_slices(int T);
size_t uniform_attention_floats(int B);  // workspace `part`: slice sums + one o_b ([B][256] floats)
float* uniform_attention_ovec(float* part, int B);  // the o_b inside `part`
// The caller chooses the steps. launch_uniform_ovec: the first two launches, o_b -> ovec ([B][256] floats; x is only
// read). o_b depends on the rows of x at the masked frames only, so a caller that knows them unchanged (the ODE
// solve's later evaluations) keeps ovec and skips this step. launch_uniform_apply: the third launch from a
// given ovec; a consumer that adds o_b itself (mt_ffn, FfnArgs::ovec) replaces it.
int launch_uniform_ovec(const void* x, const float* mask, int B, int T, const void* wqkv, int mq, const float* bqkv,
                        const void* wout, const float* bout, float* part, float* ovec, hipStream_t st);
int launch_uniform_apply(void* x, int B, int T, const float* ovec, float* row_out, hipStream_t st);
// launch-log tags (the record's ef field; mt_probe.h vclog_record, family VCLOG_AUX) of the three launches: part, vec,
// apply
enum : int { UNI_LOG_PART = 0x40000, UNI_LOG_VEC = 0x80000, UNI_LOG_APPLY = 0xC0000 };

// the XCD-aligned block order of the decoder's streaming kernels (mt_common.h xcd_chunk; MT_XCD_TILES=0 turns it
// and mt_vconv's XCD-major tile walk off)
int xcd_remap_enabled();
// ... for a launch streaming `bytes` of activations: only while they fit the XCDs' L2 (the decoder at B = 32: CFM
// solve 8.70 -> 8.47 ms with mt_vconv's XCD-major walk; at B = 256 the round-robin order is faster)
inline int xcd_remap_for(size_t bytes) { return xcd_remap_enabled() && bytes <= (24u << 20) ? 1 : 0; }
}  // namespace mt
