/*
 * matcha_hip.h — C ABI of the MI355X-native (gfx950) Matcha-TTS synthesis path.
 *
 * The reference (Lounes78/matcha-tts) has no native code and no FFI: its hot path is the
 * PyTorch module call surface that main.py uses. Each entry point below replaces the ATen
 * work under one of those calls (reference file:line in /root/reference):
 *
 *   mt_durations + mt_alignment  <- MatchaTTS.synthesize duration/index path  model.py:1273-1289
 *                                   (sequence_mask :42-46, generate_path :64-76)
 *   mt_cfm_solve                 <- CFM.forward / BASECFM.forward Euler|midpoint loop
 *                                   model.py:1084-1109, 1136-1145, estimator Decoder.forward :964-1048
 *   mt_decoder_step              <- one Decoder.forward (estimator) call  model.py:964-1048
 *   mt_denorm_crop               <- denormalize + crop  model.py:106-125, 1295-1298
 *   mt_vocoder_forward           <- hifigan.models.Generator.forward  hifigan/models.py:181-197
 *   mt_denoise                   <- hifigan.denoiser.Denoiser.forward hifigan/denoiser.py:62-68
 *   mt_vocoder_forward_ragged,   <- the reference pipeline's per-utterance vocoder + denoiser calls (one utterance
 *   mt_denoise_ragged               per call, mel cropped to its y_length: main.py:181-198,
 *                                   MOS_audiou_generator.ipynb:265-277) for a whole padded batch in one launch chain
 *   mt_resample, mt_audio_stats, <- the host steps after the vocoder, main.py:198-201 (`.clamp(-1, 1)`, soundfile's
 *   mt_audio_encode                 PCM16 write), plus rate conversion and level, which the reference leaves to callers
 *   mt_loudness, mt_true_peak    <- no counterpart: BS.1770 loudness and true peak of the output, for delivery levels
 *   mt_peak_envelope, mt_limit   <- no counterpart: look-ahead true-peak limiter, so that both figures are met
 *   mt_window_gather,            <- streaming delivery of the steps above (windows of the mel / the audio, the outputs
 *   mt_window_scatter,              that became final): no counterpart in the reference, which vocodes whole utterances
 *   mt_resample_range,
 *   mt_peak_envelope_range,      <- a fixed gain and the limiter chunk by chunk: ranges of mt_peak_envelope's and
 *   mt_limit_range                  mt_limit's rows, read in place from buffers that are still being filled
 *   mt_audio_edges, mt_join_plan, <- long-form synthesis: a batch of sentences joined into documents (trim, pauses,
 *   mt_join                         crossfades); no counterpart in the reference, which writes one file per sentence
 *   mt_audio_decode,             <- the recording input stage: PCM / mu-law bytes of a ragged batch to the log-mel that
 *   mt_log_mel_ragged               align, edit and the trainer take (the reference featurizes one file per CPU worker)
 *   mt_maximum_path              <- train_standalone.maximum_path train_standalone.py:280-325 (MAS)
 *   mt_durations_tokens, mt_align   duration control and a forced aligner for inference: no counterpart in the
 *                                   reference (its log-prior train_standalone.py:639-644 in direct form, textbook MAS)
 *
 * Conventions
 *  - Every pointer argument is DEVICE memory owned by the caller (PyTorch), except the
 *    host-side handles and name/shape buffers. The library never allocates device memory
 *    and keeps no global device state.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, asynchronously.
 *  - Tensors use the reference layouts at the boundary: mel/mu/z [B][80][T] fp32, masks
 *    [B][1][T] fp32 (0/1), wav [B][1][L] fp32. Internally activations are [B][T][C].
 *  - Return 0 on success; a negative value on error, with a message in mt_last_error()
 *    (thread-local).
 *  - dtype selects the arithmetic of the conv/GEMM/attention kernels: MT_DTYPE_F32 (exact fp32
 *    MFMA, parity mode) or MT_DTYPE_BF16 (bf16 MFMA, fp32 accumulate, perf mode). Norm
 *    statistics, the time-embedding MLP and the ODE state are always fp32.
 */
#ifndef MATCHA_HIP_H
#define MATCHA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MT_DTYPE_F32 0
#define MT_DTYPE_BF16 1
#define MT_SOLVER_EULER 0
#define MT_SOLVER_MIDPOINT 1

const char* mt_last_error(void);
int mt_abi_version(void);
/* Nonzero when this library is a timing-experiment build (tools/exp_build.sh), whose kernels drop work and
 * compute WRONG results: bit 0 mt_vconv (VCONV_EXP, or the VCONV_TS diagnostic build), 1 mt_rbconv (RB_EXP),
 * 2 mt_ffn (FFN_EXP), 3 the pair kernels (VPAIR_EXP). A production build returns 0; smoke() and bench.py refuse
 * anything else. */
int mt_build_experiments(void);
/* The compile-time K-loop schedules this library instantiates (mt_vconv's CT loops and mt_rbconv; test support for
 * tests/test_vcsched.py, host only): mt_sched_count() records; mt_sched_get(i, rec[11], wait, wait_first, cap) fills
 * rec = {family, NCH, TAPS, NW, NXB, TX, WPW, XPW, NST, RL, prologue wait} and the vmcnt counts the kernel waits with
 * at the top of steps s = -1 .. S-1 (entries 0 .. S; wait_first: the first tile's), returns S (negative: error). */
int mt_sched_count(void);
int mt_sched_get(int i, int* rec, int* wait, int* wait_first, int cap);

/* ---------------------------------------------------------------------------------------
 * Text encoder + duration predictor (TextEncoder.forward, model.py:517-535; Encoder :428-439,
 * RoPE MultiHeadAttention :294-364, ConvReluNorm prenet :171-208, DurationPredictor :210-229).
 * Replaces the host PyTorch encoder that MatchaTTS.synthesize (model.py:1273) calls.
 * Parameters are named relative to the TextEncoder module ("emb.weight",
 * "encoder.attn_layers.0.conv_q.weight", "proj_w.norm_1.gamma", ...); "_rope_theta" is the fp32
 * table 1/10000^(arange(0, d, 2)/d), d = int(head_dim * 0.5), of model.py:258-265.
 * forward: x int64 [B][Tx] token ids, x_lengths int64 [B], spks fp32 [B][spk_emb_dim] (n_spks > 1)
 * -> mu fp32 [B][80][Tx], logw fp32 [B][1][Tx], x_mask fp32 [B][1][Tx].
 * ------------------------------------------------------------------------------------- */
typedef struct mt_encoder mt_encoder;
int mt_encoder_create(int n_vocab, int n_channels, int filter_channels, int n_heads, int n_layers, int kernel_size,
                      int n_spks, int spk_emb_dim, int dp_filter_channels, int dp_kernel_size, int prenet, int dtype,
                      mt_encoder** out);
void mt_encoder_destroy(mt_encoder* e);
int mt_encoder_num_params(const mt_encoder* e);
int mt_encoder_param_name(const mt_encoder* e, int i, char* buf, int buflen);
int mt_encoder_param_shape(const mt_encoder* e, int i, int64_t* shape, int maxdim);
size_t mt_encoder_packed_bytes(const mt_encoder* e);
int mt_encoder_pack(const mt_encoder* e, const float* const* params, void* packed, void* stream);
size_t mt_encoder_workspace_bytes(const mt_encoder* e, int B, int Tx);
/* 96-dim heads: the self-attention core on MFMA (1, default; bf16: probabilities enter P.V as bf16; fp32: exact-fp32
 * v_mfma_f32_16x16x4_f32 throughout) or on the fp32-VALU kernel (0). */
int mt_encoder_set_mfma_attention(mt_encoder* e, int enable);
/* fp32: 1 (default) runs the prenet / attention-projection / FFN / duration-predictor convs on mt_vconv's fp32 mode
 * (LDS-DMA staging, exact-fp32 MFMA); 0 = the generic implicit-GEMM kernel (A/B, tests). Same arithmetic. */
int mt_encoder_set_vconv(mt_encoder* e, int enable);
/* fp32 encoder: 1 runs the FFN convs (model.py:375-393; TextEncoder precision "fp32x3") in mt_vconv's split-bf16 mode:
 * every fp32 operand is the sum of three bf16 parts and each fp32 product the sum of the six bf16 MFMA products whose
 * parts reach 2^-16, accumulated in fp32 (the reference's fp32 to a few ulp, at 16x the fp32 MFMA rate per product);
 * 0 (default) = exact fp32 MFMA. Not a bf16 encoder: its logw stays within 1e-5 of the fp32 reference. */
int mt_encoder_set_split(mt_encoder* e, int enable);
/* Store policy of the mt_vconv launches' 16-byte output stores: 0 plain (default), 1 write-through (sc1); same bits.
 * Any other mode is refused. */
int mt_encoder_set_store_policy(mt_encoder* e, int mode);
/* oov (nullable, device int32): set to 0, then to 1 when any id of x (padding included) lies outside [0, n_vocab):
 * nn.Embedding's IndexError (model.py:522); the caller raises at its next host sync. The embedding reads a clamped
 * row for such an id, so the launch itself stays in bounds. */
int mt_encoder_forward(const mt_encoder* e, const void* packed, const int64_t* x, const int64_t* x_lengths,
                       const float* spks, int B, int Tx, float* mu, float* logw, float* x_mask, int32_t* oov,
                       void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * U-Net estimator + CFM solver. Hyper-parameters are those of main.py:67-76
 * (channels=(256,256), attention_head_dim=64); c_cond = 2*n_feats (+ spk_emb_dim).
 * ------------------------------------------------------------------------------------- */
typedef struct mt_decoder mt_decoder;
int mt_decoder_create(int c_cond, int n_mid_blocks, int n_blocks, int num_heads, int dtype,
                      mt_decoder** out);
void mt_decoder_destroy(mt_decoder* d);
/* Reference state_dict tensors the packer needs, in canonical order, named relative to the
 * estimator (e.g. "down_blocks.0.0.block1.block.0.weight"); "_sinus_freq" is the fp32
 * frequency table exp(arange(c_cond/2) * -ln(1e4)/(c_cond/2-1)) of model.py:757-759. */
int mt_decoder_num_params(const mt_decoder* d);
int mt_decoder_param_name(const mt_decoder* d, int i, char* buf, int buflen);
int mt_decoder_param_shape(const mt_decoder* d, int i, int64_t* shape, int maxdim); /* -> ndim */
/* bf16: 1 (default) runs the ResnetBlock1D convs, the stride-1 down/up convs and the final block
 * conv on the LDS-DMA persistent conv (mt_vconv; producers keep those inputs masked, block 1's
 * GroupNorm+Mish applied by a separate pass, block 2's inside the res conv's epilogue); 2 = the same with
 * block 2's GroupNorm+Mish as a separate pass too; 0 = generic conv kernel with the GN/mask prologues.
 * Same math as mt_decoder_step / mt_cfm_solve (model.py ResnetBlock1D, Block1D, Decoder.forward). */
int mt_decoder_set_vconv(mt_decoder* d, int enable);
size_t mt_decoder_packed_bytes(const mt_decoder* d);
/* params[i]: device fp32 tensor in reference layout for parameter i. */
int mt_decoder_pack(const mt_decoder* d, const float* const* params, void* packed, void* stream);

size_t mt_cfm_workspace_bytes(const mt_decoder* d, int B, int T, int n_timesteps, int solver);
/* z_noise: randn [B,80,T] (z = z_noise*temperature, model.py:1085); mu_y [B,80,T]; mask [B,1,T];
 * spks [B,spk_dim] or NULL; z_out [B,80,T] (may alias z_noise). T must be even. */
int mt_cfm_solve(const mt_decoder* d, const void* packed, const float* z_noise, float temperature,
                 const float* mu_y, const float* mask, const float* spks, int B, int T,
                 int n_timesteps, int solver, float* z_out, void* ws, size_t ws_bytes, void* stream);

/* The same solve with the caller's bound on valid frames: max_valid = the most mask = 1 frames of any utterance
 * (model.py:1278's y_max; 0 = unknown). When max_valid < T every utterance has padded frames at full resolution
 * (and at max_valid <= T - 2 also at half resolution, mask[:, ::2]); the reference then fills every masked key
 * with +3.4e38 (model.py:697), so each utterance's attention is the same row for all queries — the uniform
 * mean of its masked V rows — and those transformer blocks skip Q / K / the per-frame softmax and
 * out-projection (a masked mean + two GEMVs per utterance). Same results as mt_cfm_solve up to rounding. */
int mt_cfm_solve_bounded(const mt_decoder* d, const void* packed, const float* z_noise, float temperature,
                         const float* mu_y, const float* mask, const float* spks, int B, int T, int max_valid,
                         int n_timesteps, int solver, float* z_out, void* ws, size_t ws_bytes, void* stream);
/* mt_cfm_solve_bounded with the noise drawn by the library instead of read from z_noise: utterance b gets the seeded
 * stream of seeds[b] (int64 [B], device; see mt_noise_fill) times temperature[b] (fp32 [B], device; NULL = 1), at
 * every frame of [0, T), padded ones included. One kernel writes the solver's fp32 state and the estimator's input
 * slot directly, so no [B,80,T] noise tensor exists; it runs before the captured graph, which is the same graph
 * mt_cfm_solve_bounded replays. Bit-identical to mt_cfm_solve_bounded on z_noise = mt_noise_fill(seeds, temperature)
 * with temperature 1, and on z_noise = mt_noise_fill(seeds, NULL) with one shared temperature. Workspace:
 * mt_cfm_workspace_bytes. */
int mt_cfm_solve_seeded(const mt_decoder* d, const void* packed, const int64_t* seeds, const float* temperature,
                        const float* mu_y, const float* mask, const float* spks, int B, int T, int max_valid,
                        int n_timesteps, int solver, float* z_out, void* ws, size_t ws_bytes, void* stream);
/* One solve with a step count and a time grid per utterance. The rows come sorted by step count: n_steps (int32 [B],
 * host, each >= 1) is non-increasing, anything else is an error; callers sort their own rows. Utterance b takes the
 * Euler / midpoint steps i = 0 .. n_steps[b] - 1 at time t[b][i] with step dt[b][i] (fp32 [B][n_steps[0]] row-major,
 * host; entries past a row's count are not read; t in [0, 1], dt in (0, 1]), or, with t and dt both NULL, the
 * reference's grid t = (float)(i / n_b), dt = (float)(1 / n_b) (model.py:1086-1104), on which a row's arithmetic is
 * that of mt_cfm_solve_bounded with n_timesteps = n_b. After its last step no launch includes the row: evaluation i
 * runs on the first rows_per_eval[i] rows (mt_cfm_rows_plan): the solve costs sum_i rows_per_eval[i] row-evaluations.
 * Exactly one of z_noise ([B,80,T]) and seeds (int64 [B], device; mt_cfm_solve_seeded's stream) is given;
 * temperature: fp32 [B], device, NULL = 1. The host arrays are consumed before the call returns. Launched directly on
 * the stream (no hipGraph, nothing cached). Workspace: mt_cfm_rows_workspace_bytes(d, B, T, n_steps[0], solver). */
size_t mt_cfm_rows_workspace_bytes(const mt_decoder* d, int B, int T, int n_max, int solver);
/* Host only (no GPU call): the number of estimator evaluations S of such a solve (n_steps[0] for Euler, twice that
 * for midpoint), with rows_per_eval[i] = the rows evaluation i runs on; negative (mt_last_error) for an empty batch,
 * a count < 1, an increasing pair or cap < S. */
int mt_cfm_rows_plan(const int32_t* n_steps, int B, int solver, int32_t* rows_per_eval, int cap);
int mt_cfm_solve_rows(const mt_decoder* d, const void* packed, const float* z_noise, const int64_t* seeds,
                      const float* temperature, const float* mu_y, const float* mask, const float* spks, int B, int T,
                      int max_valid, const int32_t* n_steps, const float* t, const float* dt, int solver, float* z_out,
                      void* ws, size_t ws_bytes, void* stream);
/* Mel infill: mt_cfm_solve_rows with some frames given. x1 (fp32 [B,80,T], device, normalized mel) and keep (uint8
 * [B,T], device, non-zero = kept); a frame is kept only where mask != 0 too, padded frames are never written. Kept
 * frames are held on the training-time conditional path p(t) = (1 - (1 - sigma_min) t) z0 + t x1 in fp32 (model.py:
 * 1147-1162), z0 the utterance's own initial noise (seeded, or z_noise times temperature), p(1) = x1 itself: before
 * evaluation 0 state and estimator input are p(t_0); after an Euler step or a midpoint second evaluation both are
 * p(t_{i+1}); after a midpoint first half the estimator input alone is p(t_i + dt_i / 2). Free frames are integrated
 * as in mt_cfm_solve_rows and see the kept ones through the estimator. One extra element-wise launch
 * (infill_clamp_kernel) per evaluation on the rows still in the batch, and one before the first. t: whole grids, fp32
 * [B][n_steps[0] + 1] row-major on the host, row b strictly increasing inside [0, 1] over its first n_steps[b] + 1
 * entries (dt_i = t[i+1] - t[i] in fp32; the clamp takes t[i+1] itself), or NULL: the reference grid (float)(i / n_b).
 * sigma_min in [0, 1). Every other argument, check and message as mt_cfm_solve_rows. Workspace:
 * mt_cfm_infill_workspace_bytes(d, B, T, n_steps[0], solver). */
size_t mt_cfm_infill_workspace_bytes(const mt_decoder* d, int B, int T, int n_max, int solver);
int mt_cfm_solve_infill(const mt_decoder* d, const void* packed, const float* z_noise, const int64_t* seeds,
                        const float* temperature, const float* mu_y, const float* mask, const float* spks,
                        const float* x1, const uint8_t* keep, float sigma_min, int B, int T, int max_valid,
                        const int32_t* n_steps, const float* t, int solver, float* z_out, void* ws, size_t ws_bytes,
                        void* stream);
/* Seeded Gaussian noise, z [B,C,T] fp32 (C % 4 == 0): z[b,c,t] depends on (seeds[b], c, t) only, not on B, T or the
 * row's position. Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) of the int64 seed's two's-complement uint64
 * on the counter (t, c / 4, 0, 0); each output word x gives u(x) = (2 (x >> 9) + 1) 2^-24; channels 4q, 4q + 1 are
 * r(u(x0)) cos(2 pi u(x1)) and r(u(x0)) sin(2 pi u(x1)), channels 4q + 2, 4q + 3 the same from x2, x3, with
 * r(u) = sqrt(-2 ln u); the value is then multiplied by temperature[b] (fp32 [B], device; NULL = 1) in fp32.
 * matcha_hip/noise.py is the same stream on the CPU. */
int mt_noise_fill(const int64_t* seeds, const float* temperature, int B, int C, int T, float* z, void* stream);
/* 1 (default): mt_cfm_solve_bounded takes the query-independent attention path where max_valid allows it;
 * 0: always the general Q.K^T path (A/B, tests) */
int mt_decoder_set_uniform_attention(mt_decoder* d, int enable);
/* 1 (default): mt_cfm_solve / mt_cfm_solve_bounded replay the evaluation chain (time embedding + every estimator
 * evaluation) as a captured hipGraph, cached per (packed, workspace, B, T, steps, solver, path flags); the caller's
 * mask is staged into the workspace first, so replays read no caller pointer. 0: direct launches. Bypassed while a
 * launch probe or the launch log is armed. Same results either way. */
int mt_decoder_set_graphs(mt_decoder* d, int enable);
/* Debug taps honoured by mt_decoder_step only: taps[i] (device fp32 [B,256,T_l], or NULL) receives a copy of
 * the block output the reference fixture records with forward hooks — 0 down_blocks[0][0] (ResnetBlock1D),
 * 1 down_blocks[0][1][0] (BasicTransformerBlock, channel-major), 2 mid_blocks[-1][1][0] (T/2), 3 up_blocks[0][2]
 * (Upsample1D, masked), 4 up_blocks[1][1][0] (model.py:984-1043). n <= 5; NULL / n = 0 clears them. */
int mt_decoder_set_taps(mt_decoder* d, float* const* taps, int n);

size_t mt_decoder_step_workspace_bytes(const mt_decoder* d, int B, int T);
/* one estimator evaluation: out = Decoder.forward(x, mask, mu_y, t, spks) [B,80,T] */
int mt_decoder_step(const mt_decoder* d, const void* packed, const float* x, const float* mu_y,
                    const float* mask, const float* spks, float t, int B, int T, float* out, void* ws,
                    size_t ws_bytes, void* stream);
/* the same with one time per utterance, t [B] fp32 in device memory (Decoder.forward with a [B] t as
 * CFM.compute_loss calls it, model.py:1147-1162) */
size_t mt_decoder_step_times_workspace_bytes(const mt_decoder* d, int B, int T);
int mt_decoder_step_times(const mt_decoder* d, const void* packed, const float* x, const float* mu_y,
                          const float* mask, const float* spks, const float* t, int B, int T, float* out,
                          void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * HiFi-GAN Generator (hifigan/models.py:148-206). Parameters are the folded weights
 * ("conv_pre.weight", "ups.0.weight", "resblocks.4.convs1.1.weight", ...) i.e. after
 * remove_weight_norm (hifigan/models.py:199-206).
 * ------------------------------------------------------------------------------------- */
typedef struct mt_vocoder mt_vocoder;
/* rb_dils: n_kernels x n_dils row-major */
int mt_vocoder_create(int resblock, int n_ups, const int* up_rates, const int* up_kernels,
                      int up_init_channel, int n_kernels, const int* rb_kernels, int n_dils,
                      const int* rb_dils, int dtype, mt_vocoder** out);
void mt_vocoder_destroy(mt_vocoder* v);
int mt_vocoder_num_params(const mt_vocoder* v);
int mt_vocoder_param_name(const mt_vocoder* v, int i, char* buf, int buflen);
int mt_vocoder_param_shape(const mt_vocoder* v, int i, int64_t* shape, int maxdim);
size_t mt_vocoder_packed_bytes(const mt_vocoder* v);
/* fused ResBlock stages for the 32/64-channel stages in bf16 (default on; bit-identical to the
 * per-layer path, which 0 selects) */
int mt_vocoder_set_fusion(mt_vocoder* v, int enable);
/* LDS-DMA persistent convs (mt_vconv) for the bf16 ResBlock1 stages with C % 64 == 0: inputs
 * pre-activated by their producers, same rounding points as the generic per-layer path. mode 1:
 * the stages the fused ResBlock kernel does not serve (C = 128, 256); mode 2 (default, measured
 * faster): also the 64-channel stage instead of the fused kernel; 0: the generic per-layer kernel. Replaces the same
 * convs as mt_vocoder_forward (hifigan/models.py:90-97, 187-192). */
int mt_vocoder_set_vconv(mt_vocoder* v, int mode);
/* bf16, vconv mode 2: ResBlock pairs (conv_{k,d} -> lrelu -> conv_{k,1} -> + x, hifigan/models.py:90-97) each as
 * ONE launch with the intermediate on chip and the input activation applied on chip. 1 (default): the 64- and
 * 32-channel stages' pairs and the 128-channel stage's k = 3 resblock; 4: every 128-channel pair too; 2: none of
 * the 128-channel stage; 0: every pair as two per-layer launches. Same bits in every mode. */
int mt_vocoder_set_pair(mt_vocoder* v, int enable);
/* Store policy of the bf16 stages' 16-byte output stores: bit i of stage_mask = stage i's launches (its upsampler and
 * its ResBlock convs / pairs) store write-through (sc1: the line leaves the XCD's L2 at once instead of at the launch
 * boundary); 0 = plain stores everywhere (default). Same bits either way. A mask naming a stage the vocoder does not
 * have is refused. */
int mt_vocoder_set_store_policy(mt_vocoder* v, int stage_mask);
int mt_vocoder_pack(const mt_vocoder* v, const float* const* params, void* packed, void* stream);
size_t mt_vocoder_workspace_bytes(const mt_vocoder* v, int B, int T);
/* mel [B,80,T] fp32 -> wav [B,1,T*prod(up_rates)] fp32 */
int mt_vocoder_forward(const mt_vocoder* v, const void* packed, const float* mel, int B, int T,
                       float* wav, void* ws, size_t ws_bytes, void* stream);
/* Ragged batch: utterance b is vocoded at its own lens[b] mel frames (int32, device; frames past it are the
 * zero padding a batch-1 call of that length sees), so wav[b][0, 256 lens[b]) equals Generator.forward on
 * mel[b:b+1, :, :lens[b]] alone; wav[b] past it is zero and columns past lens[b] are not computed. Needs the bf16
 * vconv / pair path on every stage (the defaults) and B <= 512. */
int mt_vocoder_forward_ragged(const mt_vocoder* v, const void* packed, const float* mel, int B, int T,
                              const int32_t* lens, float* wav, void* ws, size_t ws_bytes, void* stream);
/* 1 when mt_vocoder_forward_ragged runs with this handle's precision and path modes, else 0 */
int mt_vocoder_ragged_supported(const mt_vocoder* v);

/* ---------------------------------------------------------------------------------------
 * Duration -> alignment index path (bit-exact given logw).
 * ------------------------------------------------------------------------------------- */
/* w_ceil = ceil(exp(logw)*x_mask*length_scale) [B,Tx]; cum = cumsum(w_ceil) [B,Tx];
 * y_lengths = max(sum(w_ceil), 1) int64 [B]. */
int mt_durations(const float* logw, const float* x_mask, float length_scale, int B, int Tx,
                 float* w_ceil, float* cum, int64_t* y_lengths, void* stream);
/* the same with one length scale per utterance, length_scale fp32 [B] in device memory: row b has the bits of
 * mt_durations on that row with length_scale[b] */
int mt_durations_scaled(const float* logw, const float* x_mask, const float* length_scale, int B, int Tx,
                        float* w_ceil, float* cum, int64_t* y_lengths, void* stream);
/* Duration control. length_scale fp32 [B] (NULL: 1), token_scale fp32 [B,Tx] (NULL: 1), dur_in fp32 [B,Tx] (NULL).
 *   dur_in == NULL: w_ceil = ceil((((exp(logw)*x_mask)*length_scale[b])*token_scale[b,x])), in that multiply order:
 *                   with token_scale NULL or all 1 every output has the bits of mt_durations_scaled.
 *   dur_in given:   w_ceil = dur_in*x_mask (logw may be NULL); zero-frame tokens are legal, mt_alignment skips them.
 * cum and y_lengths as above. bad (device int32, may be NULL) is set to 0, then to 1 when an unmasked w_ceil is
 * negative, not finite or not a whole number, or a row's sum reaches 2^24 (that row's y_length is then 1). */
int mt_durations_tokens(const float* logw, const float* x_mask, const float* length_scale, const float* token_scale,
                        const float* dur_in, int B, int Tx, float* w_ceil, float* cum, int64_t* y_lengths,
                        int32_t* bad, void* stream);
/* attn [B,1,Tx,T] one-hot path (may be NULL); mu_y[b,c,j] = mu[b,c,token(j)] [B,C,T] (may be NULL);
 * y_mask [B,1,T] = (j < y_lengths[b]) (may be NULL) */
int mt_alignment(const float* cum, const int64_t* y_lengths, int B, int Tx, int T, const float* mu, int C,
                 float* attn, float* mu_y, float* y_mask, void* stream);
/* mel[b,c,t] = z[b,c,t]*std[c] + mean[c] for t < Ty; z [B,C,T] -> mel [B,C,Ty] */
int mt_denorm_crop(const float* z, const float* mean, const float* std, int B, int C, int T, int Ty,
                   float* mel, void* stream);

/* ---------------------------------------------------------------------------------------
 * Forced aligner (inference): the frames each token of mu [B,C,Tx] spans in the mel y [B,C,Ty].
 *   log-prior, direct form, fp32, c ascending (a cell depends on mu[b,:,x] and y[b,:,j] only):
 *     lp[b,x,j] = -0.5 * sum_c (yh[c,j] - mu[c,x])^2 - 0.5*C*log(2 pi),  yh = (y - mean)/std  (mean or std NULL: yh = y)
 *   textbook Monotonic Alignment Search (Glow-TTS maximum_path_each; NOT mt_maximum_path's recurrence) over the
 *   cells max(0, tx+y-ty) <= x < min(tx, y+1), NEG = -1e9:
 *     p[x,y] = lp[x,y] + max(x == y ? NEG : p[x,y-1], x == 0 ? (y == 0 ? 0 : NEG) : p[x-1,y-1])
 *   backtrack idx = tx-1; y = ty-1 .. 0: durations[idx] += 1; idx -= 1 when idx != 0 and
 *     (idx == y or p[idx,y-1] < p[idx-1,y-1]).
 * t_xs / t_ys int32 [B] are clamped to [0,Tx] / [0,Ty]; a row with t_ys < t_xs or t_xs <= 0 gets all-zero durations.
 * durations int64 [B,Tx] (zero past t_xs); log_prior [B,Tx,Ty] and paths [B,Tx,Ty] (one-hot) may be NULL. Tx <= 1024.
 * ------------------------------------------------------------------------------------- */
size_t mt_align_workspace_bytes(int B, int C, int Tx, int Ty);
int mt_align(const float* mu, const float* y, const float* mean, const float* std, const int32_t* t_xs,
             const int32_t* t_ys, int B, int C, int Tx, int Ty, int64_t* durations, float* log_prior, float* paths,
             void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Denoiser (hifigan/denoiser.py): STFT n_fft 1024 / hop 256 / Hann, magnitude - strength*bias,
 * clamp >= 0, iSTFT. audio [B,L] -> out [B, 256*(L/256)]; bias_spec [513].
 * ------------------------------------------------------------------------------------- */
size_t mt_denoise_workspace_bytes(int B, int L);
int mt_denoise(const float* audio, int B, int L, const float* bias_spec, float strength, float* out,
               void* ws, size_t ws_bytes, void* stream);
/* Ragged batch: row b denoised as an utterance of lens[b] * lmul samples (int32, device; its own reflect padding
 * and 1 + samples / 256 frames, as a one-utterance call); out[b] past those samples is zero. */
int mt_denoise_ragged(const float* audio, int B, int L, const int32_t* lens, int lmul, const float* bias_spec,
                      float strength, float* out, void* ws, size_t ws_bytes, void* stream);
/* |STFT| (same framing) of every frame: mag [B][1+L/256][513] (bias spectrum, denoiser.py:57-60) */
int mt_stft_magnitude(const float* audio, int B, int L, float* mag, void* stream);

/* ---------------------------------------------------------------------------------------
 * Audio output stage (matcha_hip/audio_out.py is the specification on the CPU): what main.py does on
 * the host after the vocoder (`.clamp(-1, 1)`, then soundfile), for a whole padded batch audio [B][L] fp32 whose row
 * b is valid for its first len_b samples. Every result of row b depends on that row's valid samples alone.
 * ------------------------------------------------------------------------------------- */
#define MT_NORM_NONE 0
#define MT_NORM_PEAK 1
#define MT_NORM_RMS 2
#define MT_ENC_F32 0
#define MT_ENC_PCM16 1
#define MT_ENC_MULAW 2
/* Rational resampling by up / down (coprime, each 1 .. 1024) with a zero-phase FIR h of 2 half + 1 taps:
 *   out[b][m] = sum_k h[half + m down - k up] audio[b][k],  m < out_lens[b] = ceil(len_b up / down) (64-bit),
 * one fp32 FMA chain per output over the taps of its phase, in an order that depends on m alone; zero past out_lens[b]
 * up to Lout, which is at least ceil(L up / down). len_b = lens[b] * lmul clamped to [0, L] (lens int32 [B], device;
 * NULL: L). taps_polyphase: fp32 [up][ceil((2 half + 1) / up)], entry [p][q] = h[q up + p], zero-filled (device).
 * out_lens int32 [B]. The table goes to LDS with the tile's input samples while both fit 64 KiB (every rate between
 * 8 and 48 kHz from 22,050 Hz does); beyond that the kernel reads them from global memory, same bits.
 * Workspace: mt_resample_workspace_bytes (0 and mt_last_error for a refused factor), 16-byte aligned. */
size_t mt_resample_workspace_bytes(int half, int up, int down);
int mt_resample(const float* audio, int B, int L, const int32_t* lens, int lmul, const float* taps_polyphase, int half,
                int up, int down, float* out, int Lout, int32_t* out_lens, void* ws, size_t ws_bytes, void* stream);
/* The outputs [m_lo, m_lo + cnt) of mt_resample's rows, without the others: out[b][j] (fp32 [B][cnt]) has the bits of
 * mt_resample's out[b][m_lo + j] while m_lo + j < ceil(len_b up / down) and is zero past it; out_cnt[b] (int32 [B]) =
 * that row's count of such j, clamp(ceil(len_b up / down) - m_lo, 0, cnt). Same chain, same table re-order, phase and
 * input span taken from the output's index m_lo + j in the utterance. Of audio[b] it reads only the samples between
 * the first and the last one the chains of the requested outputs touch, the last being
 * (half + (m_lo + out_cnt[b] - 1) down) / up: later samples of the row need not be written yet (streaming delivery,
 * DESIGN.md §20). m_lo >= 0, cnt >= 1, m_lo + cnt < 2^31 - 2048. Workspace as mt_resample. */
int mt_resample_range(const float* audio, int B, int L, const int32_t* lens, int lmul, const float* taps_polyphase,
                      int half, int up, int down, int m_lo, int cnt, float* out, int32_t* out_cnt, void* ws,
                      size_t ws_bytes, void* stream);
/* peak[b] = max |x| (fp32 [B]) and meansq[b] = sum x^2 / len_b (fp64 [B]; 0 for an empty row) over the first len_b =
 * lens[b] samples (int32 [B], device, clamped to [0, L]; NULL: L). The squares are summed in fp64 over tiles of 4096
 * samples counted from the row's start, then the partials in a fixed order: no atomics. */
size_t mt_audio_stats_workspace_bytes(int B, int L);
int mt_audio_stats(const float* audio, int B, int L, const int32_t* lens, float* peak, double* meansq, void* ws,
                   size_t ws_bytes, void* stream);
/* gain g_b (fp64, rounded to fp32 at the end): MT_NORM_NONE 1 (peak and meansq are not read and may be NULL);
 * MT_NORM_PEAK level / peak[b]; MT_NORM_RMS level / sqrt(meansq[b]), with limit != 0 at most 1 / peak[b]; 1 when
 * peak[b] == 0. level must be finite and positive. Then, in fp32, v = clamp(g_b x, -1, 1) and out[b][i] is
 * MT_ENC_F32 v (fp32), MT_ENC_PCM16 q = rint(32767 v), half to even (int16), MT_ENC_MULAW the G.711 mu-law byte of
 * q (uint8); past len_b (lens as in mt_audio_stats) 0, 0 and 0xFF. out: [B][L] of the encoding's type, never in
 * place. gain_out fp32 [B], may be NULL. */
int mt_audio_encode(const float* audio, int B, int L, const int32_t* lens, const float* peak, const double* meansq,
                    int normalize, double level, int limit, int encoding, void* out, float* gain_out, void* stream);
/* Programme loudness and true peak of every row (matcha_hip/loudness.py is the specification on the
 * CPU). lens as in mt_audio_stats; a row's results depend on its valid samples alone, bit for bit. Neither entry point
 * allocates on the device; every argument error is refused before any launch.
 *
 * mt_loudness: ITU-R BS.1770 gated loudness as an energy. The row is K-weighted from a zero state by the two biquads
 * coef (HOST pointer to 10 doubles: b1[0..2], a1[1..2], b2[0..2], a2[1..2], a[0] = 1; transposed direct form II) in
 * fp64, as a chunked scan along time (chunks of 32 samples, tiles of 8192, both counted from the row's start). Blocks
 * of 4 hop samples every hop samples (32 <= hop <= 2^24; 100 ms): len_b >= 4 hop gives J = (len_b - 4 hop) / hop + 1
 * blocks z_j = sum y^2 / (4 hop); 0 < len_b < 4 hop one block over the whole row, z_0 = sum y^2 / len_b; an empty row
 * none. energy[b] (fp64 [B]) = the mean of the z_j with z_j > gate_abs and z_j > 0.1 * mean{z_j > gate_abs}, summed in
 * block order; 0 when no block passes gate_abs. Loudness = -0.691 + 10 log10 energy. nblocks[b] (int32 [B]) = J.
 * z: fp64 [B][Jcap], written whole (0 from J on), or NULL; Jcap >= the block count of a row of L samples. L <= 2^30.
 * Workspace: mt_loudness_workspace_bytes (0 and mt_last_error for a refused shape), 16-byte aligned. */
size_t mt_loudness_workspace_bytes(int B, int L, int hop);
int mt_loudness(const float* audio, int B, int L, const int32_t* lens, const double* coef, int hop, double gate_abs,
                double* z, int Jcap, int32_t* nblocks, double* energy, void* ws, size_t ws_bytes, void* stream);
/* tpeak[b] (fp32 [B]) = the largest magnitude of the row oversampled four times, max_m |r[m]|, m < 4 len_b, r the
 * outputs of mt_resample at up = 4, down = 1 with the same table (taps_polyphase fp32 [4][ceil((2 half + 1) / 4)],
 * device; 1 <= half <= 1024), bit for bit: the same chain, nothing of r is written. sample_peak (fp32 [B], device,
 * mt_audio_stats' peak; may be NULL) is folded in: tpeak[b] = max(sample_peak[b], max |r|), the true peak. L < 2^29 -
 * 2048. Workspace: mt_true_peak_workspace_bytes, 16-byte aligned. */
size_t mt_true_peak_workspace_bytes(int B, int L);
int mt_true_peak(const float* audio, int B, int L, const int32_t* lens, const float* taps_polyphase, int half,
                 const float* sample_peak, float* tpeak, void* ws, size_t ws_bytes, void* stream);
/* Look-ahead true-peak limiter (matcha_hip/limiter.py is the specification on the CPU, bit for bit).
 * lens as in mt_audio_stats; a row's results depend on its valid samples alone. Neither entry point allocates on the
 * device or uses atomics; every argument error is refused before any launch. 1 <= B <= 65535, L as mt_true_peak.
 *
 * mt_peak_envelope: env[b][i] (fp32 [B][L], zero from len_b on) = max(|x[i]|, max |r[m]|, 4i - 3 <= m <= 4i + 3 inside
 * [0, 4 len_b)), r the 4x oversampled row exactly as mt_true_peak forms it (same table, same chain; nothing of r is
 * written). The maximum starts at 0 and is taken with fmaxf: a NaN counts as absent. env must not overlap audio.
 * Workspace: mt_peak_envelope_workspace_bytes (a constant), 16-byte aligned.
 *
 * mt_limit: the row's gain g = float32(double(g_in) level / sqrt(meansq[b])) with g_in = gain_in[b] (fp32 [B], device;
 * NULL: 1), formed on the device by the encoder's own gain routine; g = g_in where peak[b] == 0 or meansq[b] == 0.
 * peak (fp32 [B]) only tells whether the row is levelled at all: peak[b] == 0 leaves it untouched (s = 1). With
 * c32 = float32(ceiling) (ceiling: a linear amplitude, finite and positive, as is level):
 *   a = fl32(g env[b][i]);  r = c32 / a (IEEE fp32) where a > c32, else 1;  q[i] = floor(r 2^30), 2^30 outside the row
 *   m[j] = min q[j .. j + W - 1];  S[i] = sum_{k < W} m[i - k];  s[i] = float32(double(S[i]) / double(W 2^30))
 *   out[b][i] = fl32(fl32(g audio[b][i]) s[i]), two products rounded separately; zero from len_b on.
 * s[i] <= r[i] at every sample: no sample's envelope passes the ceiling. The gain falls over W samples before a peak
 * and recovers over W after it (1 <= W <= 2048). reduction[b] (fp32 [B]) = min_i s[i] (1 for an empty row),
 * gain_out[b] (fp32 [B]) = g. Integer minimum (van Herk / Gil-Werman blocks of W) and integer sum: the same bits in
 * any order. out must overlap neither audio nor env. Workspace: mt_limit_workspace_bytes (0 and mt_last_error for a
 * refused shape or window), 16-byte aligned. */
size_t mt_peak_envelope_workspace_bytes(void);
int mt_peak_envelope(const float* audio, int B, int L, const int32_t* lens, const float* taps_polyphase, int half,
                     float* env, void* ws, size_t ws_bytes, void* stream);
size_t mt_limit_workspace_bytes(int B, int L, int W);
int mt_limit(const float* audio, const float* env, int B, int L, const int32_t* lens, const float* peak,
             const double* meansq, const float* gain_in, double level, double ceiling, int W, float* out,
             float* reduction, float* gain_out, void* ws, size_t ws_bytes, void* stream);
/* Ranges of the two, for a stream at a gain fixed beforehand: the tile bodies of mt_peak_envelope and
 * mt_limit run from i_lo instead of from 0, on full-length buffers [B][L] read in place. lens are the rows' FINAL
 * lengths; what happens at a row's end is the whole-row kernel's. i_lo >= 0, cnt >= 1, i_lo + cnt < 2^31 - 8192; a
 * range may lie past the end of a row or of L. Every argument error is refused before any launch; no device
 * allocation, no atomics.
 *
 * mt_peak_envelope_range: writes env[b][i] for i in [i_lo, i_lo + cnt) inside [0, len_b) with the bits of
 * mt_peak_envelope, and nothing else of env (fp32 [B][L], the same buffer across calls). Of audio[b] it reads no
 * sample past min(len_b - 1, i_lo + cnt - 1 + (half + 3) / 4): later samples need not be written yet. Workspace as
 * mt_peak_envelope.
 *
 * mt_limit_range: out[b][j] (fp32 [B][cnt]) has the bits of mt_limit's out[b][i_lo + j] called with peak = 1,
 * meansq = 1, level = 1 and gain_in = gain, which makes g = gain[b] (fp32 [B], device) as it stands; zero from the
 * row's end on. out_cnt[b] (int32 [B]) = clamp(len_b - i_lo, 0, cnt). Of env[b] it reads only
 * [i_lo - (W - 1), i_lo + cnt + W - 2] inside [0, len_b), 2^30 in place of q outside the row; of audio[b] only the
 * range. reduction (fp32 [B]) is read and written: min(its value, min s over the range), from per-tile minima in the
 * workspace and a final kernel; the caller starts it at 1. out must overlap neither audio nor env. Workspace:
 * mt_limit_range_workspace_bytes (0 and mt_last_error for a refused shape or window), 16-byte aligned. */
int mt_peak_envelope_range(const float* audio, int B, int L, const int32_t* lens, const float* taps_polyphase,
                           int half, int i_lo, int cnt, float* env, void* ws, size_t ws_bytes, void* stream);
size_t mt_limit_range_workspace_bytes(int B, int cnt, int W);
int mt_limit_range(const float* audio, const float* env, int B, int L, const int32_t* lens, const float* gain,
                   double ceiling, int W, int i_lo, int cnt, float* out, int32_t* out_cnt, float* reduction, void* ws,
                   size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Streaming delivery (matcha_hip/stream_plan.py is the specification of the windows): cut one window
 * per row out of a full-length buffer, and write the part of a processed window that became final back into one.
 * Plain copies. All tables are int32 [R] in device memory, R <= 512 (one ragged launch chain); an entry that points
 * outside its buffer (negative, a row index past the batch, a range past the row) is clamped away inside the kernel:
 * such a gather reads zeros, such a scatter writes nothing, neither touches memory out of range.
 * ------------------------------------------------------------------------------------- */
/* rows[r][c][w] = src[row_src[r]][c][row_start[r] + w] for w < row_len[r], else 0. src fp32 [Bs][C][Ls], rows fp32
 * [R][C][W] (written whole). C = 80 for a mel [B][80][T] (start and len in frames), C = 1 for audio (in samples). */
int mt_window_gather(const float* src, int Bs, int C, int Ls, const int32_t* row_src, const int32_t* row_start,
                     const int32_t* row_len, int R, int W, float* rows, void* stream);
/* dst[row_dst[r]][dst_start[r] + i] = rows[r][crop_from[r] + i] for i < crop_len[r]. rows fp32 [R][W], dst fp32
 * [Bd][Ld]; the rest of dst keeps its contents. Two rows r must not write the same samples of dst. */
int mt_window_scatter(const float* rows, int R, int W, const int32_t* row_dst, const int32_t* crop_from,
                      const int32_t* dst_start, const int32_t* crop_len, float* dst, int Bd, int Ld, void* stream);

/* ---------------------------------------------------------------------------------------
 * Long-form synthesis (matcha_hip/join.py is the specification on the CPU): a batch of sentences
 * (segments, the rows of seg fp32 [S][L]) becomes D documents: trim edges per segment, the place of every segment in
 * its document, the documents written with fades and overlaps. 1 <= S, D <= 65535; L, Ld, Lcap <= 2^30. doc_first:
 * int32 [D + 1], CSR: document d owns the segments doc_first[d] .. doc_first[d + 1] - 1 in that order (none is
 * allowed). All tables are int32 in device memory, so mt_audio_edges -> mt_join_plan -> mt_join needs no host round
 * trip; the host cannot check them, and an entry that points outside its buffer (a segment range outside [0, S], an
 * edge outside [0, L], a doc_len past Ld) is clamped inside the kernels: wrong audio, never an access out of range.
 * No entry point allocates on the device, none uses atomics, every argument error is refused before any launch, and
 * a document's results depend on its own segments alone, bit for bit.
 * ------------------------------------------------------------------------------------- */
/* Trim edges of every row: sample k < n_s (n_s = lens[s] clamped to [0, L]; lens int32 [S], NULL: L) is loud when
 * |audio[s][k]| >= thr (fp32 compare; a NaN is not loud; thr finite, >= 0). first / last = the smallest / largest
 * loud k: start[s] = max(first - pad, 0), end[s] = min(last + 1 + pad, n_s) (pad >= 0, in samples); (0, 0) for a row
 * without a loud sample. One pass over tiles of 4096 samples counted from the row's start; tiles at or past n_s are
 * skipped and nothing at or past n_s is read. Integer min / max through the workspace (two ints per tile), then one
 * workgroup per row. Workspace: mt_audio_edges_workspace_bytes (0 and mt_last_error for a refused shape), 16-byte
 * aligned. start, end: int32 [S]. */
size_t mt_audio_edges_workspace_bytes(int S, int L);
int mt_audio_edges(const float* audio, int S, int L, const int32_t* lens, float thr, int pad, int32_t* start,
                   int32_t* end, void* ws, size_t ws_bytes, void* stream);
/* Placement. Per segment a_s = clamp(start[s], 0, L), e_s = clamp(end[s], a_s, L), len_s = e_s - a_s. gap[s] (int32
 * [S]) is the silence in samples between s and the next segment of its document, negative an overlap; it is ignored on
 * a document's last segment. Effective gap g_s = max(gap[s], -min(len_s / 2, len_{s+1} / 2)) (integer halves), so no
 * sample is covered by more than two segments. dst[first] = head, dst[s + 1] = dst[s] + len_s + g_s; doc_len[d] =
 * dst[last] + len_last + tail, head + tail for a document without segments (head, tail >= 0). 64-bit arithmetic;
 * *bad (int32, device) = 1 when a doc_len exceeds Lcap (1 .. 2^30), else 0, and every output is then min(., Lcap) of
 * its 64-bit value: nothing wraps. dst int32 [S] (a segment no document owns is not written), doc_len int32 [D]. One
 * workgroup per document: a segmented scan in chunks of 256 segments. */
int mt_join_plan(const int32_t* doc_first, int D, const int32_t* start, const int32_t* end, const int32_t* gap, int S,
                 int L, int head, int tail, int Lcap, int32_t* dst, int32_t* doc_len, int32_t* bad, void* stream);
/* out[d][i] (fp32 [D][Ld], written whole) = 0.0f plus, in segment order, fl32(w_s(j) seg[s][a_s + j]) for every
 * segment s of document d with 0 <= j = i - dst[s] < len_s: one fp32 product and one fp32 add per covering segment,
 * rounded separately (never a fused multiply-add); zero where nothing covers i and from min(doc_len[d], Ld) on. With
 * F_s = min(fade, len_s / 2): w_s(j) = ramp[((2 j + 1) fade) / (2 F_s)] for j < F_s, the same of j' = len_s - 1 - j
 * for j >= len_s - F_s, 1 between (with F_s == fade the index is j itself). ramp: fp32 [fade], device, the rising
 * half of a raised cosine 0.5 - 0.5 cos(pi (j + 0.5) / fade) built by the host; 0 <= fade <= 16384, NULL allowed at
 * fade == 0. Only the samples [a_s, e_s) of a segment are read. One workgroup per tile of 1024 document samples: it
 * finds its first segment by binary search in the document's range of dst (non-decreasing in a plan of mt_join_plan)
 * and walks forward. */
int mt_join(const float* seg, int S, int L, const int32_t* start, const int32_t* end, const int32_t* doc_first, int D,
            const int32_t* dst, const int32_t* doc_len, const float* ramp, int fade, float* out, int Ld, void* stream);

/* ---------------------------------------------------------------------------------------
 * Log-mel featurizer (§8f rank 4), replacing train_standalone.py:164-201 `mel_spectrogram(y, 1024, 80,
 * 22050, 256, 1024, fmin, fmax, center=False)` + `normalize(mel, mel_mean, mel_std)` (:204-210,
 * hifigan/meldataset.py:52-89): reflect pad 384 | STFT 1024/256 Hann, center=False | sqrt(|S|^2 + 1e-9) |
 * mel_basis . | log(clamp(., 1e-5)) | (. - mel_mean) / mel_std.
 * audio [B][L] fp32 (L > 384), mel_basis [80][513] fp32 (librosa slaney filters, host-computed) ->
 * mel [B][80][F] fp32, F = (L - 256) / 256 + 1.
 * ------------------------------------------------------------------------------------- */
int mt_log_mel(const float* audio, int B, int L, const float* mel_basis, float mel_mean, float mel_std, float* mel,
               void* stream);

/* ---------------------------------------------------------------------------------------
 * Recording input stage (matcha_hip/audio_in.py is the specification on the CPU): the mirror image of
 * the audio output stage, from the bytes of a ragged batch of recordings to (mel, mel_lengths) as MatchaTTS.align,
 * MatchaTTS.edit and the trainer take them: mt_audio_decode -> mt_resample (to 22,050 Hz) -> mt_audio_stats (peak
 * level) -> mt_audio_edges (trim) -> mt_log_mel_ragged. 1 <= B <= 65535. Neither entry point allocates on the device
 * or uses atomics; every argument error is refused before any launch; the tables (lens, start, end) are int32 in
 * device memory, the host cannot check them, and an entry that points outside its buffer is clamped inside the
 * kernel: wrong audio, never an access out of range. A row's results depend on its own valid samples alone, bit for
 * bit.
 * ------------------------------------------------------------------------------------- */
/* Interleaved frames -> mono fp32. raw: [B][Lcap channels] of the encoding's type (MT_ENC_F32 float, MT_ENC_PCM16
 * int16, MT_ENC_MULAW uint8), frame i of row b at raw[b][i channels + c]; 1 <= channels <= 8, Lcap >= 1, Lcap channels
 * < 2^31. len_b = lens[b] in frames (int32 [B], device, clamped to [0, Lcap]; NULL: Lcap). Per sample, in fp32:
 * MT_ENC_PCM16 q / 32768 (exact); MT_ENC_MULAW the G.711 expansion of the byte (the centre of its interval, an int16)
 * / 32768; MT_ENC_F32 the value itself, 0.0f in place of a NaN or an infinity. channels > 1: the fp32 sum in channel
 * order ((c0 + c1) + c2) ..., then one fp32 product with float(1.0 / channels). out: fp32 [B][Lcap], written whole,
 * 0.0f from len_b on; nothing of raw at or past frame len_b is read. out must not overlap raw. */
int mt_audio_decode(const void* raw, int B, int Lcap, const int32_t* lens, int encoding, int channels, float* out,
                    void* stream);
/* mt_log_mel of every row at its own edges and gain. a_b = clamp(start[b], 0, L), e_b = clamp(end[b], a_b, L), n_b =
 * e_b - a_b (start, end: int32 [B], device; start NULL: 0, end NULL: L). Row b's signal is s_b[i] = fl32(gain[b]
 * audio[b][a_b + i]), i < n_b (gain fp32 [B], device; NULL: the samples as they stand), reflected at ITS two ends 0 and
 * n_b - 1. frames[b] (int32 [B]) = 0 for n_b <= 384, else (n_b - 256) / 256 + 1. mel: fp32 [B][80][Fcap], written
 * whole: for f < frames[b] the bits mt_log_mel gives for s_b held alone in a [1][n_b] buffer (the same frame body:
 * FFT, magnitude, (p0 + p1) + p2 of the three thirds of each 513-bin dot product), `fill` for f >= frames[b]. Nothing
 * of audio[b] outside [a_b, e_b) is read. Fcap >= the frame count of a row of L samples; L >= 1, L < 2^30; mel_std
 * != 0. One workgroup per (row, 8 frames): the twiddle table is built once per workgroup and a workgroup past the
 * row's last frame only writes `fill`. */
int mt_log_mel_ragged(const float* audio, int B, int L, const int32_t* start, const int32_t* end, const float* gain,
                      const float* mel_basis, float mel_mean, float mel_std, float fill, float* mel, int Fcap,
                      int32_t* frames, void* stream);

/* ---------------------------------------------------------------------------------------
 * Training-side (§8f rank 3): Monotonic Alignment Search, replacing train_standalone.py:280-325
 * `maximum_path(neg_cent, mask)` (a device->host copy + CPU numba/Python DP in the reference) with
 * its exact recurrence as a GPU anti-diagonal wavefront. neg_cent [B][Tx][Ty] fp32, t_xs / t_ys [B]
 * int32 (the mask's token / frame counts) -> paths [B][Tx][Ty] fp32 one-hot per frame column inside
 * [0,t_x) x [0,t_y), zero elsewhere. Tx <= 1024.
 * ------------------------------------------------------------------------------------- */
size_t mt_maximum_path_workspace_bytes(int B, int Tx, int Ty);
int mt_maximum_path(const float* neg_cent, const int32_t* t_xs, const int32_t* t_ys, int B, int Tx, int Ty,
                    float* paths, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Training step (§8f rank 3): fp32 primitives the CFM training step (train_standalone.py:623-707,
 * MatchaLightningModule.forward / training_step / configure_optimizers; model.py:1147-1162 compute_loss)
 * is built from, forward and backward (matcha_hip/train.py composes them). Activations are [rows][C]
 * row-major fp32 device buffers. No reduction uses atomics (bitwise reproducible).
 * ------------------------------------------------------------------------------------- */
/* C[z] = (alpha op(A[z]) op(B[z]) + beta C[z] + bias[n]) * row_mask[z][m]; op(A) M x K, op(B) K x N; z < batch,
 * strides in elements; bias [N] and row_mask [batch][M] optional (NULL). Exact-fp32 MFMA (32x32x2 f32); a long K over
 * few output tiles is split into slices whose partials (in the caller's workspace) are summed in slice order
 * (deterministic). */
int mtt_gemm(int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda, long long sA,
             const float* B, int ldb, long long sB, float beta, float* C, int ldc, long long sC, int batch,
             const float* bias, const float* row_mask, float* ws, size_t ws_bytes, void* stream);
/* mtt_gemm with the operands rounded (RNE) to a 16-bit format before 16-bit MFMA with fp32 accumulation:
 * opfmt 0 none (= mtt_gemm), 1 fp16 (the reference Trainer's precision="16-mixed", train_standalone.py:868, under
 * which autocast runs conv1d / linear / matmul on fp16 operands), 2 bf16 ("bf16-mixed"). The output stays fp32. */
int mtt_gemm_ex(int opfmt, int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda,
                long long sA, const float* B, int ldb, long long sB, float beta, float* C, int ldc, long long sC,
                int batch, const float* bias, const float* row_mask, float* ws, size_t ws_bytes, void* stream);
/* device workspace mtt_gemm uses to split a long K over slices (0: never splits this shape); with less, it runs
 * unsplit */
size_t mtt_gemm_workspace_bytes(int M, int N, int K, int batch);
/* conv1d columns: cols[(b*Tout+o)][c*k+tap] = x[b][t][c] * mask[b][t], t = o*stride-pad+tap*dil (a torch Conv1d weight
 * [Cout][Cin][k] is then the GEMM operand as stored; mask [B][T] optional: the reference's conv(x * mask)); col2im is
 * its adjoint, dx[b][t][c] (+)= mask[b][t] * sum of the columns that read (b, t, c) */
int mtt_im2col(const float* x, const float* mask, int B, int T, int C, int k, int stride, int pad, int dil, int Tout,
               float* cols, void* stream);
int mtt_col2im(const float* dcols, const float* mask, int B, int T, int C, int k, int stride, int pad, int dil,
               int Tout, float* dx, int accumulate, void* stream);
/* out[i] (+)= op(a[i], b[((i/d0)%m0)*s0 + ((i/d1)%m1)*s1], c[i]); op: 0 alpha a + beta b, 1 alpha a b,
 * 2 mish(a), 3 c mish'(a), 4 silu(a), 5 c silu'(a), 6 relu(a), 7 c [a>0], 8 exp(a), 9 (a-b)^2, 10 sin(a),
 * 11 cos(a), 12 log(alpha + a), 13 alpha / a */
int mtt_ew(int op, size_t n, const float* a, const float* b, const float* c, float* out, float alpha, float beta,
           size_t d0, size_t m0, size_t s0, size_t d1, size_t m1, size_t s1, int accumulate, void* stream);
/* dst[r][doff+j] (+)= src[r][soff+j], r < rows, j < n (channel concat / split; lds, ldd row strides) */
int mtt_copy_cols(const float* src, int lds, int soff, float* dst, int ldd, int doff, int rows, int n, int accumulate,
                  void* stream);
/* sequence_mask (model.py:42-46, train_standalone.py:328-333): out[b][t] = t < lengths[b], fp32 [B][T] */
int mtt_seq_mask(const int64_t* lengths, int B, int T, float* out, void* stream);
/* out[s][c] (+)= sum over rows r of segment s (seg rows each) of a[r][c] (* b[r][c]); scratch >=
 * mtt_colsum_scratch_floats(rows, C, seg) floats */
size_t mtt_colsum_scratch_floats(int rows, int C, int seg);
int mtt_colsum(const float* a, const float* b, int rows, int C, int seg, float* out, int accumulate, float* scratch,
               void* stream);
/* dst[r][doff + j] = src[r / seg][j], r < rows, j < n: one vector per utterance repeated over its seg rows into a
 * column slice of [rows][ldd] (spks.unsqueeze(-1).repeat + cat, model.py:528, 977-979). Writes only that slice. */
int mtt_bcast_cols(const float* src, int n, float* dst, int ldd, int doff, int rows, int seg, void* stream);
/* out[s][j] (+)= sum over the rows r of segment s (seg rows each) of a[r*lda + soff + j], j < n: the adjoint of
 * mtt_bcast_cols, read in place from a column slice (no split copy). scratch >= mtt_segsum_cols_scratch_floats(). */
size_t mtt_segsum_cols_scratch_floats(int rows, int n, int seg);
int mtt_segsum_cols(const float* a, int lda, int soff, int n, int rows, int seg, float* out, int accumulate,
                    float* scratch, void* stream);
/* out[0] = sum_i a[i] (* b[i]); scratch >= 1024 floats */
int mtt_sum(const float* a, const float* b, size_t n, float* out, float* scratch, void* stream);
/* dropout(p) with a counter-based hash mask of (seed, index): out = a * keep / (1 - p); the backward is the same
 * call on the gradient with the same seed */
int mtt_dropout(const float* a, size_t n, float p, unsigned seed, float* out, void* stream);
/* torch.nn.GroupNorm over x [B][T][C] (model.py:764-775); backward writes dx and per-(b, c) partials of the
 * gamma / beta gradients [B][C] (reduce with mtt_colsum) */
int mtt_groupnorm_fwd(const float* x, const float* gamma, const float* beta, int B, int T, int C, int G, float eps,
                      float* y, float* mean, float* rstd, void* stream);
int mtt_groupnorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, int B,
                      int T, int C, int G, float* dx, float* dgamma_part, float* dbeta_part, void* stream);
/* LayerNorm over the C channels of each row (decoder nn.LayerNorm, encoder channel LayerNorm model.py:148-166) */
int mtt_layernorm_fwd(const float* x, const float* gamma, const float* beta, int rows, int C, float eps, float* y,
                      float* mean, float* rstd, void* stream);
int mtt_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                      int rows, int C, float* dx, void* stream);
/* SnakeBeta (model.py:580-609) on [n/C][C]; backward: dx and per-element log-alpha / log-beta gradient terms */
int mtt_snake_fwd(const float* x, const float* log_alpha, const float* log_beta, size_t n, int C, float* y,
                  void* stream);
int mtt_snake_bwd(const float* x, const float* log_alpha, const float* log_beta, const float* dy, size_t n, int C,
                  float* dx, float* galpha, float* gbeta, void* stream);
/* row softmax of scale*s [BH][Tq][Tk] with masked keys (kmask [B][Tk] == 0) or masked queries (qmask [B][Tq],
 * may be NULL) := +3.4e38 (mode 0, decoder model.py:697) or -1e4 (mode 1, encoder model.py:353) */
int mtt_softmax_fwd(const float* s, const float* kmask, const float* qmask, int BH, int H, int Tq, int Tk, float scale,
                    int mode, float* p, void* stream);
int mtt_softmax_bwd(const float* p, const float* dp, const float* kmask, const float* qmask, int BH, int H, int Tq,
                    int Tk, float scale, float* ds, void* stream);
/* RoPE in place on x [B][T][H*dh] (first d features of each head), inverse = 1 for the backward */
int mtt_rope(float* x, int B, int T, int H, int dh, int d, const float* theta, int inverse, void* stream);
int mtt_embed_fwd(const int64_t* ids, size_t ntok, const float* table, int C, float scale, float* out, void* stream);
int mtt_embed_bwd(const int64_t* ids, size_t ntok, const float* dout, int V, int C, float scale, float* dtable,
                  void* stream);
/* torch.optim.Adam step (lr, betas, eps; no weight decay) with grad scaled by *gscale (clip / world) */
int mtt_adam(float* p, const float* g, float* m, float* v, size_t n, const float* gscale, float lr, float beta1,
             float beta2, float eps, int step, void* stream);
/* clip factor for a flat gradient holding the SUM over `world` ranks: norm = sqrt(*sumsq) * inv_world (the norm of
 * the DDP-averaged gradient), out = min(1, max_norm / (norm + 1e-6)) * inv_world (torch.nn.utils.clip_grad_norm_) */
int mtt_clip_factor(const float* sumsq, float max_norm, float inv_world, float* out, float* norm_out, void* stream);
/* torch.cuda.amp.GradScaler.unscale_ ("16-mixed", train_standalone.py:868): g *= inv_scale in place, and
 * *found = the number of non-finite elements of g as stored, checked before the multiply (the per-element
 * found-inf check of torch._amp_foreach_non_finite_check_and_unscale_); scratch >= 1024 floats */
int mtt_unscale(float* g, size_t n, float inv_scale, float* found, float* scratch, void* stream);

/* ---------------------------------------------------------------------------------------
 * Op-level entry points (per-kernel parity tests)
 * ------------------------------------------------------------------------------------- */
/* y = conv(act(x)), x [B][Tin][Cin], y [B][Tout][Cout] in dtype; W fp32 reference layout
 * (Conv1d [Cout][Cin][k]; transposed: ConvTranspose1d [Cin][Cout][k]); slope < 0: no act. */
size_t mt_op_conv1d_workspace_bytes(int dtype, int cin, int cout, int k, int stride, int transposed);
int mt_op_conv1d(int dtype, const void* x, int B, int Tin, int cin, const float* W, const float* bias,
                 int cout, int k, int stride, int pad, int dil, int transposed, float slope, void* y,
                 int Tout, void* ws, size_t ws_bytes, void* stream);
/* same with a fixed tile variant (in-process A/B timing; lrelu prologue only; -1 = automatic;
 * variant + 0x1000 reuses the weights a previous call packed into ws) */
int mt_op_conv1d_tile(int variant, int dtype, const void* x, int B, int Tin, int cin, const float* W,
                      const float* bias, int cout, int k, int stride, int pad, int dil, int transposed,
                      float slope, void* y, int Tout, void* ws, size_t ws_bytes, void* stream);
/* Op-level entry of mt_vconv (tests / A-B timing): bf16 x [B][L][cin] already activated, fp32
 * W [cout][cin][k], bias [cout], padding dil*(k-1)/2 ("same"), epilogue flags ef: 1 + resid,
 * 2 accumulate into y, 4 / div, 8 y = lrelu(v), 16 also y2 = lrelu(v); lens (nullable, device int32 [B]): the
 * ragged batch, utterance b valid for its first lens[b] frames. pack = 0 reuses the weights a
 * previous call with the same ws packed (timing). One ResBlock1 conv of hifigan/models.py:90-97. */
size_t mt_op_vconv_workspace_bytes(int cin, int cout, int k);
int mt_op_vconv(const void* x, int B, int L, int cin, const float* W, const float* bias, int cout, int k, int dil,
                int ef, const void* resid, void* y, void* y2, float slope, float div, const int32_t* lens, int pack,
                void* ws, size_t ws_bytes, void* stream);
/* The HiFi-GAN wide-stage ResBlock convs (C_in = C_out in {128, 256}, k in {3, 7, 11}) run on mt_rbconv, a variant
 * of mt_vconv whose K loop is scheduled at compile time (1, the default; bit-identical results) or on the generic
 * mt_vconv kernel (0). Process-wide; returns the previous setting. */
int mt_vconv_set_rbconv(int enable);
/* The decoder's convs and the upsamplers run mt_vconv with their K loop unrolled at compile time for their
 * (C_in, taps) (1, the default; bit-identical results) or with the runtime-cursor loop (0). Process-wide; returns
 * the previous setting. */
int mt_vconv_set_ct(int enable);
/* Round-5 ResBlock pair kernels (mask; each bit-identical to the kernel it replaces): bit 0 the 64-channel k = 7 / 11
 * pairs' compile-time K loop, bit 1 the 128-channel k = 3 pairs' one. Default 3 (MT_VPAIRK=<mask> in the
 * environment); process-wide; returns the previous mask. */
int mt_vpair_set_kernels(int mask);
/* conv_post (hifigan/models.py:193-195) in the epilogue of the last stage's final ResBlock pair (1, the default: the stage
 * output xs is never stored) or as its own launch after it (0). Both run the same MFMA arithmetic (bit-identical).
 * Process-wide; returns the previous setting (MT_POSTFOLD=0 in the environment: off). */
int mt_vocoder_set_post_fold(int enable);
/* The stage 1-2 ResBlock conv1s (mt_rbconv) read the raw chain state and apply its leaky ReLU to their staged rows in
 * LDS, so the producing convs store no activated copy (1, the default; bit-identical results), or read an activated
 * copy the producers store (0). Process-wide; returns the previous setting. */
int mt_vconv_set_actin(int enable);
/* The bf16 decoder's transformer FeedForward (LayerNorm, Linear 256 -> 1024, SnakeBeta, Linear 1024 -> 256, + x) as
 * one fused launch whose 1024-wide intermediate stays on chip (3, the default; 1 / 2 other schedules of the same
 * kernel; bit-identical results) or as two mt_vconv GEMM launches (0). Process-wide; returns the previous setting. */
int mt_ffn_set(int enable);
/* ... on decoder levels of at least `frames` frames (B x T at that level; default 16384); returns the previous value */
int mt_ffn_set_min_frames(int frames);
/* Decoder kernel variants (mask; each bit-identical to the launches it replaces): bit 0 the final projection + ODE
 * update (final_proj of mish(GroupNorm) * mask, z += dt * v) on a dedicated kernel instead of the generic conv
 * kernel; bit 1 the query-independent attention's per-utterance output vector o_b (bf16 decoder, utterances with
 * padding) computed in the first estimator evaluation of a mt_cfm_solve only and kept per transformer block for the
 * later ones: it depends on the weights and on the number of masked frames, not on the ODE state, the time, mu or the
 * speaker, so recomputing it (two launches per block and evaluation) gives the same bits. Never kept across solves or
 * graph replays; single evaluations (mt_decoder_step) always compute it. Bits 2 (value 4) and 3 (value 8): the bf16
 * evaluation's streaming launches at level 0 (T frames) / level 1 (T/2 frames) store their 16-byte outputs
 * write-through (sc1) instead of plain (level 0 only while its activations fit the L2); same bits. Default 15
 * (MT_DECK=<mask> in the environment); process-wide; bits past 15 are ignored; returns the previous mask. */
int mt_decoder_set_kernels(int mask);
/* qkv [B][T][3*heads*64], mask [B][T] -> out [B][T][heads*64], reference mask semantics */
int mt_op_attention(int dtype, const void* qkv, const float* mask, void* out, int B, int T, int heads,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * Launch probe (measurement only; no reference counterpart). Arms HIP events around every
 * launch of one kernel site, on the stream the kernel is launched on, so a benchmark can time
 * that kernel inside its own timed region. Sites: 1 = fused 64-channel HiFi-GAN ResBlock stage,
 * 2 = fused 32-channel stage, 3 = every HiFi-GAN ResBlock conv launch on mt_vconv and every fused conv-pair
 * launch (mt_vpair / mt_vpair32, priced as its two convs), 4 = the
 * decoder's k >= 2 mt_vconv launches. mt_probe_stop synchronizes the recorded events and returns the
 * number of launches, their summed duration, the algorithmic FLOPs and layer-boundary bytes they did
 * (every conv reads its input once and writes its output once, + its weights), and
 * roof_ms = sum over launches of max(FLOPs / peak_flops, bytes / peak_bw) (peaks in FLOP/s, B/s).
 * mt_probe_pause(1) stops recording (launches run unprobed) until mt_probe_pause(0); mt_probe_start
 * arms the probe unpaused. A benchmark probes a sample of its timed steps this way, since each event
 * pair adds a few microseconds of idle before the launch it brackets.
 * ------------------------------------------------------------------------------------- */
#define MT_PROBE_RBFUSE_C64 1
#define MT_PROBE_RBFUSE_C32 2
#define MT_PROBE_VCONV 3
#define MT_PROBE_VCONV_DEC 4
int mt_probe_start(int site, int max_launches);
int mt_probe_pause(int paused);
/* per recorded launch: duration (ms), algorithmic FLOPs and bytes, kernel tag (0 mt_vconv, 1 mt_vpair,
 * 2 mt_vpair32, 3 mt_rbfuse); synchronizes the events; call before mt_probe_stop. Returns the count written. */
int mt_probe_detail(int cap, double* ms, double* flops, double* bytes, int* tags);
int mt_probe_stop(int* launches, double* total_ms, double* flops, double* bytes, double peak_flops, double peak_bw,
                  double* roof_ms);

/* Launch log of the persistent LDS-DMA conv (test coverage only; no reference counterpart). While
 * armed, every mt_vconv launch appends 11 int32: epilogue flags, rows per tile (BM), frames per tile
 * (BN), 1x1 pipeline flag, output tiles, grid size (tiles > grid: workgroups walk several tiles), taps,
 * output channels, input channels, utterances, frames per utterance. stop returns the record count.
 * Launches of other kernels carry a tag in the first field instead of epilogue flags: 0x20000 the decoder's final
 * projection + ODE update kernel; and, only after mt_vconv_log_select(3), 0x40000 / 0x80000 / 0xC0000 the
 * query-independent attention's masked-sum pass, its per-utterance vector (o_b) and its x += o_b pass (grid size in
 * fields 5-6, utterances and frames per utterance in the last two) and 0x400000 the fused decoder FeedForward (field 4:
 * 1 when it adds o_b itself). mt_vconv_log_select: bit 0 the conv launches (always on), bit 1 those other decoder
 * launches (off by default: readers of the conv log expect conv variants); process-wide; returns the previous mask. */
#define MT_VCONV_LOG_FIELDS 11
int mt_vconv_log_start(int capacity);
int mt_vconv_log_stop(int32_t* records, int capacity);
int mt_vconv_log_select(int families);

#ifdef __cplusplus
}
#endif
#endif /* MATCHA_HIP_H */
