/*
 * speechclip_hip.h -- C ABI of libspeechclip_hip.so: the MI355X (gfx950) kernels behind the
 * SpeechCLIP forward / contrastive hot path.
 *
 * The reference (atosystem/SpeechCLIP) has NO native boundary: every op on this path is executed
 * inside fairseq / openai-clip / torch.nn.  Each entry point below therefore
 * cites the reference call site whose arithmetic it replaces; INTEGRATION.md shows the ctypes
 * binding a reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types cross the boundary.
 *   - every pointer is a DEVICE pointer unless named host_*; the caller owns all memory
 *     (including workspaces) and has already selected the device.
 *   - `stream` is a hipStream_t passed as void*; kernels are stateless, re-entrant and launch only
 *     on that stream (safe under one-process-per-GPU and one-thread-per-GPU callers).
 *   - return 0 on success, negative on error; sc_last_error() returns a thread-local message.
 *   - bf16 tensors are raw uint16 storage ("bf16"); "f32" is IEEE float.  Rows are contiguous;
 *     leading dimensions (ld*) are in ELEMENTS.
 */
#ifndef SPEECHCLIP_HIP_H
#define SPEECHCLIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int sc_abi_version(void);
const char* sc_last_error(void);

/* ---- GEMM family (MFMA bf16, fp32 accumulate) ------------------------------------------------
 * C[M,N] = epilogue( A[M,K] . W[N,K]^T + bias[N] ) (+ residual[M,N])
 * Replaces every nn.Linear / Conv1d-as-GEMM / patch-projection on the path:
 *   fairseq q/k/v/out_proj, fc1, fc2, post_extract_proj  (speech_encoder_plus.py:52,:84-85 call sites),
 *   ConvFeatureExtractionModel layers 1-6 as implicit GEMM over a channels-last activation with
 *   overlapping rows (lda < K)                           (speech_encoder_plus.py:75),
 *   CLIP c_fc / c_proj / in_proj / out_proj / conv1      (clip_official.py:209),
 *   parallel/cascaded branch linears                    (kwClip.py:1097-1104, :877-883).
 * flags: see SC_GEMM_* below.  K must be a multiple of 64; A rows may overlap (lda < K) and the
 * caller guarantees A is readable for rows [0, M) x [0, K).
 * Batched form: grid over `batch`; batch z uses A + z*strideA, W + (z % w_mod)*strideW,
 * C + z*strideC (bias/residual follow W / C respectively: bias + (z % w_mod)*N).
 */
#define SC_ACT_NONE 0
#define SC_ACT_GELU 1       /* erf GELU (fairseq "gelu", torch F.gelu) */
#define SC_ACT_QUICKGELU 2  /* x*sigmoid(1.702x) (openai CLIP) */
#define SC_GEMM_ACT_MASK 0x3
#define SC_GEMM_OUT_F32 0x10      /* C (and residual, if given) are f32 instead of bf16 */
#define SC_GEMM_F16 0x20          /* A, W -- and C / residual unless SC_GEMM_OUT_F32 -- are IEEE half instead of bf16 (`v_mfma_f32_16x16x32_f16`, RNE on the way out).  The
                                   * frozen pre-LN encoder layers of HuBERT-large run in this format: 11 significand bits in the GEMM / attention operands, the precision the
                                   * reference runs these models at on a GPU (fp16 autocast, config/speechCLIP/model_large/coco/spchclp_p.yaml:122) */
#define SC_GEMM_RES_AFTER_ACT 0x0 /* residual is always added after the activation */

int sc_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                 const float* bias, const void* residual, int64_t ldr,
                 int64_t M, int N, int K, int flags, void* stream);
/* COMPARATOR, off unless a scratch buffer is registered here: plain GEMMs (no activation, lda >= K, M >= 8192: QKV / attention out-proj /
 * fc2 with their bias and residual) are then handed to hipBLASLt instead of the hand-written kernel, so that the two can be timed on the same
 * operands behind the same entry (bench.py `vendor_comparator`, tools/blas_compare.py).  The product path never registers one: every GEMM of
 * the hot path runs on gemm8p_pers_kernel / gemm256_kernel / gemm_bf16_kernel (all hand-written).  Caller-owned device scratch, 64 MiB is plenty; NULL switches the comparator off. */
int sc_set_gemm_workspace(void* workspace, int64_t bytes);
int sc_gemm_last_path(void);   /* instrumentation: which kernel the last sc_gemm_bf16 call ran on: 0 gemm256_kernel / gemm_bf16_kernel, 1 the vendor
                                * library (comparator), 3 gemm8p_pers_kernel (ping-pong schedule, gemm8p.hip) -- 0 and 3 are the hand-written kernels */
/* instrumentation (comparator only): which half of the comparator workspace `stream` owns: 0 / 1, -1 none yet, -2 both halves belong to other
 * streams (that stream's GEMMs run on the hand-written kernels), -3 comparator library not loaded.  The comparator ABI itself is declared once,
 * in speechclip_amd/csrc/vendor/vendor_abi.h, for both libraries. */
int sc_debug_vendor_stream_slot(void* stream);

int sc_gemm_bf16_batched(const void* A, int64_t lda, int64_t strideA, const void* W, int64_t ldw,
                         int64_t strideW, int w_mod, void* C, int64_t ldc, int64_t strideC,
                         const float* bias, int64_t M, int N, int K, int batch, int flags, void* stream);
/* Two-level batch of the same products: z = zo*inner + zi reads A at zo*strideA + zi*strideA2, W at zo*strideW + zi*strideW2, writes C at
 * zo*strideC + zi*strideC2 (elements; no bias) -- the (utterance, head) pairs of the attention backward in ONE launch per product
 * (speechclip_amd/train_hubert.py: autograd of the [3P fairseq] MultiheadAttention inside a fine-tuned layer, speech_encoder_plus.py:52). */
int sc_gemm_bf16_batched2(const void* A, int64_t lda, int64_t strideA, int64_t strideA2, const void* W, int64_t ldw, int64_t strideW, int64_t strideW2,
                          void* C, int64_t ldc, int64_t strideC, int64_t strideC2, int64_t M, int N, int K, int outer, int inner, int flags, void* stream);

/* ---- LayerNorm (wave-per-row, D <= 1024) -----------------------------------------------------
 * out[r,:] = [gelu]( (x[r,:] - mean) * rstd * gamma + beta ), gamma/beta may be NULL (no affine).
 * Replaces every nn.LayerNorm on the path: fairseq layer_norm / self_attn_layer_norm /
 * final_layer_norm / encoder.layer_norm (speech_encoder_plus.py:39-40,:52,:78), the conv-stack
 * channel LayerNorm+GELU of the `layer_norm` extractor mode (large), CLIP ln_1/ln_2/ln_post
 * (clip_official.py:209), branch norm1/norm2/final norm (TransformerModels.py:64-75,:117).
 */
#define SC_LN_IN_F32 0x1
#define SC_LN_OUT_F32 0x2
#define SC_LN_GELU 0x4
#define SC_LN_OUT_F16 0x8         /* with SC_LN_IN_F32, 16-bit output: IEEE half instead of bf16 (the operand format of SC_GEMM_F16) */
int sc_layernorm(const void* x, int64_t ld_in, const float* gamma, const float* beta, void* out, int64_t ld_out,
                 int64_t rows, int D, float eps, int flags, void* stream);

/* ---- Weighted sum of hidden states -- avssl/module/weighted_sum.py:26-45 ----------------------
 * out[m,:] (bf16) = sum_i softmax(weights)_i * h_i[m,:]; h_i = hidden + i*layer_stride (elements),
 * rows contiguous [rows, D].  SC_WS_NORMALIZE applies F.layer_norm(h_i, (D,)) (no affine) first. */
#define SC_WS_NORMALIZE 0x1
#define SC_WS_IN_F32 0x2
int sc_weighted_sum_fwd(const void* hidden, int64_t layer_stride, const float* weights, void* out, int n_layers,
                        int64_t rows, int D, int flags, float eps, void* stream);

/* ---- L2 normalise -- avssl/model/kwClip.py:1436,:1444-1454 (x / ||x||, no eps), f32 out.  SC_L2NORM_CLAMP: x / max(||x||, 1e-8), the
 * operand normalisation of F.cosine_similarity (kwClip.py:889-897) -- a zero row gives zeros, not NaN ------- */
#define SC_L2NORM_IN_F32 0x1
#define SC_L2NORM_CLAMP 0x2
int sc_l2norm_fwd(const void* x, int64_t ld_in, float* out, int64_t rows, int D, int flags, void* stream);

/* ---- `normalize_hiddenstates: true` with `normalize_type: method1 | method2` (avssl/module/speech_encoder_plus.py:572-592; "s3prl" is the per-feature
 * layer_norm inside WeightedSumLayer, SC_WS_NORMALIZE): IN PLACE on the stacked hidden states [n_layers][B][Tp][D] (bf16, or f32 when in_f32), as the
 * reference overwrites layer_results[i] before it mixes / returns them.  method 1: every frame to unit L2 norm, x / (||x|| + 1e-8); method 2: every state
 * of utterance b divided by the mean frame norm over frames t < T (all frames of the padded batch).  workspace (method 2): n_layers*B*(Tp+1) floats. */
int sc_hidden_normalize(void* hidden, int in_f32, int n_layers, int B, int Tp, int T, int D, int method, float* workspace, void* stream);

/* ---- Deterministic split-K finish for few-row, deep-K products (the CLS rows of the pooling heads, kwClip.py:1097-1104: linear2 of the branch's
 * encoder layer is 256 x 768 x 3072): sc_gemm_bf16_batched writes `nsplit` fp32 partial products [nsplit][M][N] (K chunks as the batch), this
 * sums them in fixed order and applies bias / erf-GELU / residual: out[m,n] = act(sum_s partials[s][m][n] + bias[n]) + residual[m][n].  No atomics. */
int sc_splitk_reduce_f32(const float* partials, int nsplit, int64_t M, int N, const float* bias, const float* residual, int64_t ldr, float* out, int act,
                         void* stream);

/* ---- Per-utterance wave layer-norm -- speech_encoder_plus.py:507-508 (task.cfg.normalize) -----
 * out[b,:len_b] = layer_norm(wav[b,:len_b]); out[b,len_b:] = 0.  wav/out are [B, ld] f32. */
int sc_wave_layernorm(const float* wav, float* out, const int32_t* lens, int B, int64_t ld, float eps, void* stream);   /* `out` must not alias `wav` (several blocks per utterance read the whole row) */

/* ---- Attention ---------------------------------------------------------------------------------
 * Flash-style forward, head_dim 64, per-utterance key lengths (klens[b] keys valid; NULL = T).
 * q/k/v point at the first head's columns of row 0; rows are (b*T + t) with stride ld_qkv; head h
 * is at column offset h*64.  Replaces fairseq MultiheadAttention (key_padding_mask -> -inf) inside
 * TransformerSentenceEncoderLayer (speech_encoder_plus.py:52) and CLIP's nn.MultiheadAttention
 * in ResidualAttentionBlock (clip_official.py:209; causal != 0 adds the text tower's build_attention_mask,
 * clip_official.py:249-262).  out: bf16 [B*T, H*64] rows of stride ld_out.
 * `flags`: SC_ATTN_CAUSAL (= 1, what a boolean `causal` used to pass) | SC_ATTN_F16: q / k / v / out are IEEE half instead of bf16 (the probabilities
 * are rounded to half too; scores, running maxima and sums stay fp32) -- the operand format of SC_GEMM_F16.
 * Rows past the key length (also sc_attention_fwd_dropout / sc_attention_fwd_packed): K / V rows t in [klens[b], T) that share the last 64-key tile with a valid key are
 * loaded; their scores are replaced by -inf whatever K holds, but their V rows enter the P.V MFMA with P = 0.  PRECONDITION: V is FINITE on those rows (0 x Inf / NaN would
 * reach every query row of the utterance); any finite value, and anything at all in K or in later tiles, is ignored bit for bit.  klens[b] <= 0 gives exact zeros, klens[b] > T
 * means T.  (sc_attention_hd_fwd zeroes such V rows on load and has no such precondition.) */
#define SC_ATTN_CAUSAL 0x1
#define SC_ATTN_F16 0x2
int sc_attention_fwd(const void* q, const void* k, const void* v, void* out, const int32_t* klens, int B, int H,
                     int T, int head_dim, int64_t ld_qkv, int64_t ld_out, float scale, int flags, void* stream);

/* Train-mode dropouts of the FROZEN encoder: Lightning's model.train() re-enables them while the reference trains the pooling heads
 * (avssl/module/speech_encoder_plus.py:42 F.dropout after the positional conv, :87 dropout_input; [3P fairseq] TransformerSentenceEncoderLayer
 * dropout1 / dropout2 / dropout3 and MultiheadAttention's dropout on the probabilities).  Masks are counter-based: element i of a tensor is kept iff
 * hash(seed, i) >= drop_p * 2^32, and scaled by 1 / (1 - drop_p).
 *   sc_attention_fwd_dropout: sc_attention_fwd with dropout on the attention probabilities (the softmax row sum keeps every probability).
 *   sc_dropout_bf16: out = [residual +] dropout(x) over n bf16 elements (n % 4 == 0); in place allowed. */
int sc_attention_fwd_dropout(const void* q, const void* k, const void* v, void* out, const int32_t* klens, int B, int H, int T, int head_dim,
                             int64_t ld_qkv, int64_t ld_out, float scale, int causal, float drop_p, uint32_t seed, void* stream);
int sc_dropout_bf16(const void* x, const void* residual, void* out, int64_t n, float drop_p, uint32_t seed, void* stream);
/* out = LayerNorm(residual + dropout(x)), bf16 [rows, D]: the post-LN sites of a [3P fairseq] TransformerSentenceEncoderLayer in train mode in ONE pass
 * (same mask as sc_dropout_bf16: element index = row*D + column).  Returns 1 when D is not covered (768 is): run sc_dropout_bf16 + sc_layernorm. */
int sc_dropout_add_layernorm_bf16(const void* x, const void* residual, const float* gamma, const float* beta, void* out, int64_t rows, int D, float eps,
                                  float drop_p, uint32_t seed, void* stream);

/* CLS-rows-only attention of the pooling heads (kwClip.py:1089-1099 parallel, :869-881 cascaded):
 * NQ learned query tokens attend to [NQ CLS tokens ; frames t < lens[b]].  cls_qkv: bf16 [NQ, 3*D]
 * (q|k|v of the CLS tokens); kv_x: bf16 rows (b*T+t) = [k | v] of the frames, stride ld_kv;
 * out: bf16 [B, NQ, D], D = H*head_dim. */
int sc_cls_attention_fwd(const void* cls_qkv, const void* kv_x, int64_t ld_kv, const int32_t* lens, void* out, int B, int T,
                         int NQ, int H, int head_dim, float scale, void* stream);

/* Flash-style forward for head_dim 64 / 96 / 128 (MFMA): the full-row layers of a parallel branch with n_layers >= 2 (8 heads: head_dim 96 at
 * d = 768, 128 at d = 1024) and the per-utterance CLS row of its last layer (Tq = 1).  Sequence b has Tq query rows and Tk key rows; klens[b]
 * keys are valid (NULL = Tk).  Element (b, t, h, e) of q is at q[b*q_bs + t*q_rs + h*head_dim + e], of k / v at b*kv_bs + t*kv_rs + ..., of
 * out at b*o_bs + t*o_rs + ... (elements).  bf16 q / k / v; out bf16, or fp32 with SC_ATTN_HD_OUT_F32.  fp32 scores / softmax.  drop_p > 0:
 * dropout on the probabilities with sc_attention_fwd_dropout's mask (pair index ((b*H + h)*Tk + t) * ceil(Tk / 2) + key / 2).
 * Other head dims return an error: sc_attention_fwd keeps its head_dim-64 contract. */
#define SC_ATTN_HD_OUT_F32 0x10
int sc_attention_hd_fwd(const void* q, const void* k, const void* v, void* out, const int32_t* klens, int B, int H, int Tq, int Tk,
                        int head_dim, int64_t q_bs, int64_t q_rs, int64_t kv_bs, int64_t kv_rs, int64_t o_bs, int64_t o_rs,
                        float scale, float drop_p, uint32_t seed, int flags, void* stream);

/* Full-row multi-head attention, any head_dim <= 1024 (multiple of 8), arbitrary boolean key-padding mask (uint8 [B, L], 1 = padding;
 * NULL = none): torch.nn.MultiheadAttention(batch_first) as the reference's pooling heads call it on WHOLE sequences --
 * TransformerEncoder.forward / extract_hidden_states (avssl/module/kw_modules/TransformerModels.py:77-96) and
 * MultiheadAttentionAndNorm.forward / extract_hidden_states (:119-129), reached through KW_*Branch.extract_hidden_states
 * (avssl/model/kwClip.py:828-856, :1049-1076) and feature_extractor_s3prl (:1213-1247).  Not on the hot path (which keeps the CLS rows
 * only: sc_cls_pool_fwd).  q/k/v: bf16, row (b*L + t) at stride ld_qkv, head h at column h*head_dim; out: bf16 rows of stride ld_out. */
int sc_attention_rows_fwd(const void* q, const void* k, const void* v, void* out, const uint8_t* key_padding_mask, int B, int H, int L,
                          int head_dim, int64_t ld_qkv, int64_t ld_out, float scale, void* stream);

/* Per-head attention probabilities of the same attention for the query rows [0, n_rows) of every (b, h): probs f32 [B, H, n_rows, L],
 * softmax over the non-padding keys, exactly 0 at padding -- what torch.nn.MultiheadAttention returns with need_weights=True,
 * average_attn_weights=False in MultiheadAttentionAndNorm.extract_attention_map (avssl/module/kw_modules/TransformerModels.py:130-135);
 * n_rows = keyword_num is all KW_CascadedBranch.getAttentionMap keeps (avssl/model/kwClip.py:941-949), n_rows = L the full map. */
int sc_attention_probs_fwd(const void* q, const void* k, float* probs, const uint8_t* key_padding_mask, int B, int H, int L, int head_dim,
                           int n_rows, int64_t ld_qkv, float scale, void* stream);

/* torch.topk(x, K, dim=-1) of f32 rows (row r at x + r*ld, V entries): vals f32 [rows, K] descending, idx i32 [rows, K]; ties go to the
 * lowest index.  The K nearest sub-words of every keyword: getAttentionMap (avssl/model/kwClip.py:990) and the de-tokenisation of
 * validation_epoch_end (:357-375, K = detokenized_K_neighbors). */
int sc_topk_rows_f32(const float* x, int64_t ld, int64_t rows, int V, int K, float* vals, int32_t* idx, void* stream);

/* Algebraic form of the same pooling attention (no K/V of the frames is formed): score_r(x) = x . u_r + beta_r with
 * u_r = scale * Wk_h^T Q_{q,h}, r = (q,h), R = NQ*H <= 8.  `scores` f32 [B*T, R] are the frame scores (one skinny sc_gemm_bf16 with
 * W = u, bias = beta), `cls_scores` f32 [NQ, R] those of the CLS tokens; the kernel soft-maxes over [CLS tokens ; frames t < lens[b]]
 * and writes xbar[b,r,:] = sum_keys p_r(key) x_key (bf16 [B,R,D], D <= 1024).  The caller finishes with
 * out_{q,h} = Wv_h xbar_r + bv_h (sc_gemm_bf16_batched). */
int sc_cls_pool_fwd(const void* x, int64_t ld_x, const void* cls_tok, const float* scores, const float* cls_scores,
                    const int32_t* lens, void* xbar, int B, int T, int NQ, int R, int D, void* stream);
/* The same pooling with the pooled sums kept to ~16 mantissa bits: xbar_hilo bf16 [B, R, nblk*D] = (hi | lo) or (hi | lo | hi), hi + lo = the fp32
 * sum -- the A operand of a depth-nblk*D sc_gemm_bf16[_batched] against [Wv_h | Wv_h] or [Wv_hi | Wv_hi | Wv_lo] (sc_split_hilo_bf16's convention).  The eval heads use this form (round 4): on the
 * benchmark's T = 499 batch the utterances' pooled vectors differ by ~1e-2 of their norm, and ONE bf16 rounding of them (2e-3) is visible in the
 * centred-cosine parity of the embedding (kwClip.py:1099-1104 runs this in fp32). */
int sc_cls_pool_fwd_split(const void* x, int64_t ld_x, const void* cls_tok, const float* scores, const float* cls_scores,
                          const int32_t* lens, void* xbar_hilo, int B, int T, int NQ, int R, int D, int nblk, void* stream);

/* ---- HuBERT conv layer 0 -- fairseq ConvFeatureExtractionModel block 0 (speech_encoder_plus.py:75)
 * wav f32 [B, ld] (zero padded, L valid columns), w f32 [C,10], out bf16 channels-last [B, P, C]
 * (P >= T0 rows per utterance; rows >= T0 are written as zeros).
 * sc_conv0_gn_coef: per-(b,c) GroupNorm scale/shift from the 10x10 sample autocorrelation
 * (fp64) -- the statistics are over all T0 frames of the padded batch, as in the reference.
 * sc_conv0_fwd mode 0: conv -> GroupNorm(coef) -> GELU; mode 1: conv + bias (no norm, no act); mode 2: conv + bias -> LayerNorm over the C channels of every
 * frame -> GELU (the first layer of an extractor_mode = "layer_norm" feature extractor, HuBERT-large: fairseq ConvFeatureExtractionModel [3P] via
 * speech_encoder_plus.py:75) with `coef` = gamma[C] | beta[C] | eps (2 C + 1 floats); C % 64 == 0 and P % 64 == 0. */
int64_t sc_conv0_stats_workspace_bytes(int B);
int sc_conv0_gn_coef(const float* wav, int64_t ld, const float* w, const float* gamma, const float* beta, void* workspace,
                     float* coef, int B, int C, int T0, float eps, void* stream);
int64_t sc_conv0_wfrag_workspace_bytes(int B);   /* scratch for the matrix-core form (C % 64 == 0): per-utterance weight fragments */
int sc_conv0_fwd(const float* wav, int64_t ld, int64_t L, const float* w, const float* bias, const float* coef, void* out, int B,
                 int C, int T0, int P, int mode, void* wfrag_ws, void* stream);

/* ---- HuBERT positional conv -- speech_encoder_plus.py:32-40 ------------------------------------
 * pack: zero padded frames (t >= valid[b]) and regroup x bf16 [B*Tp, D] into xg bf16
 * [B][G][Tp+Kw][D/G] (Kw/2 zero rows each side) so that group g is an overlapping-row GEMM
 * (lda = D/G, K = Kw*D/G) via sc_gemm_bf16_batched -> conv bf16 [B*G][Tp][D/G].
 * finish: out = [LayerNorm]( mask(x) + gelu(conv + bias) ); gamma NULL = no LN (layer_norm_first). */
/* sc_posconv_conv: the grouped conv itself on the matrix cores from an LDS-resident input window (no pack pass, no sliding-window
 * re-streaming): conv bf16 [B][G][Tp][D/G].  Returns 1 without doing anything when D/G is not 32/48/64 (caller: pack + batched GEMM). */
int sc_posconv_conv(const void* x, const int32_t* valid, const void* wg, void* conv, int B, int Tp, int D, int G, int Kw, void* stream);
int sc_posconv_pack(const void* x, const int32_t* valid, void* xg, int B, int Tp, int D, int G, int Kw, void* stream);
int sc_posconv_finish(const void* x, const int32_t* valid, const void* conv, const float* bias, const float* gamma, const float* beta,
                      void* out, int B, int Tp, int D, int G, int out_f32, float eps, void* stream);

/* sc_crop_pad: out[b,j] = j < lens[b] ? wav[b, starts[b]+j] : 0 -- train-mode random crop (audio_transforms.py:5-23; offsets drawn on the
 * host exactly as the reference draws them) + zero right-padding (speech_encoder_plus.py:510-518) for the whole batch in one launch. */
int sc_crop_pad(const float* wav, int64_t ld, const int32_t* starts, const int32_t* lens, float* out, int B, int Lout, void* stream);
/* sc_wave_prep: the audio side of the data hand-over for a ragged batch of raw PCM utterances in ONE call: int16 -> f32, mono mix, rational-ratio resampling
 *   to the model's rate, the train-mode crop window and zero right-padding to [B, Lout] (what `librosa.load(path, sr=16000)` in avssl/data/base_dataset.py:70-87
 *   and random_crop_max_length + re-padding in speech_encoder_plus.py:510-518 do per utterance on the host).  ARITHMETIC CONTRACT (restated in
 *   speechclip_amd/data/audio_transforms.py, whose float64 execution the tests judge against):
 *     mono f32 sample  int16: x = (float)(sum_c s_c) * (1.0f / (C * 32768)): every step exact in f32 for C in {1, 2}, so at a matching rate the output equals
 *                      np.mean(pcm.astype(np.float32) / 32768, axis=1) bit for bit.  f32: x = s (C = 1), (s_0 + s_1) * 0.5f (C = 2).
 *     ratio            L / M = dst / src reduced by their gcd; n_out = (frames * L + M - 1) / M in 64-bit integers.  L == M == 1 (table = -1, K = 0):
 *                      y[n] = x[n], no table is read.
 *     resampler        polyphase Kaiser-windowed sinc (the project's own design; no parity with soxr / librosa is claimed).  In the up-sampled domain
 *                      fc = ROLLOFF * 0.5 / max(L, M), W = Z / (2 fc), h(t) = L * 2 fc * sinc(2 fc t) * I0(beta * sqrt(1 - (t / W)^2)) / I0(beta) for
 *                      |t| <= W and 0 outside; Z = 16, beta = 8.56, ROLLOFF = 0.85 = 17 / 20, so `|t| <= W` is the integer test 17 |t| <= 320 max(L, M).
 *                      Output n: u = n * M (int64), j0 = u div L, p = u mod L; y[n] = sum_k taps[p][k] * x[j_k] over the inputs j_k with
 *                      |p + (j0 - j_k) * L| <= W in ascending j, x = 0 outside [0, frames); fp32 accumulation in that order inside one thread.
 *                      taps[p][k] = h evaluated in double on the host and rounded once to f32; K = the largest tap count of any phase (rows are zero
 *                      beyond their own count; the kernel stops at the count).
 *   packed   device bytes [packed_bytes]: the utterances back to back (any gaps allowed), each frame-interleaved, frames x C samples
 *   offsets  int64 [B]: byte offset of utterance b in `packed`, a multiple of its frame size (C * 2 or C * 4 bytes)
 *   geom     int64 [B][SC_WAVE_PREP_GEOM]: frames, C (1 | 2), fmt (SC_WAVE_PREP_I16 | SC_WAVE_PREP_F32), L, M, K, table (f32 index of the utterance's [L][K]
 *            tap table in `tables`; -1 = identity rate), start, len (the crop window in OUTPUT samples)
 *   tables   f32 [tables_len]: one [L][K] table per distinct rate; may be NULL when no utterance resamples.  L * K <= SC_WAVE_PREP_MAX_TABLE.
 *   offsets / geom / tables are passed TWICE, as host memory (`*_host`: every rule is checked there before any launch) and as the device copy of the same
 *   bytes the kernel reads.  out f32: out[b * ld + j] = y_b[start_b + j] for j < len_b and exactly 0.0f for len_b <= j < Lout (ld >= Lout).
 *   Only the crop window is computed.  Every output element is written once; one launch; no atomics, no host synchronisation, 64-bit addressing.
 *   Refused (nonzero rc + sc_last_error, nothing launched): C outside {1, 2}; unknown fmt; frames < 0; L, M <= 0 or not coprime; a window outside [0, n_out];
 *   len > Lout; an utterance outside `packed` (or a misaligned offset); a table index or extent outside `tables`; K that is not the support's tap count (or a
 *   table given at identity rate); NULL tables when an utterance resamples; a table over the cap; a decimation so steep (about M / L > 30) that one block's
 *   input span does not fit its staging buffer; ld < Lout. */
#define SC_WAVE_PREP_GEOM 9
#define SC_WAVE_PREP_I16 0
#define SC_WAVE_PREP_F32 1
#define SC_WAVE_PREP_MAX_TABLE 65536
int sc_wave_prep(const void* packed, int64_t packed_bytes, const int64_t* offsets_host, const int64_t* offsets, const int64_t* geom_host, const int64_t* geom,
                 const float* tables_host, const float* tables, int64_t tables_len, int B, float* out, int64_t ld, int64_t Lout, void* stream);

/* ---- CLIP ViT stem -- openai VisionTransformer.forward up to ln_pre (clip_official.py:209) ----- */
/* sc_image_normalize_u8: torchvision ToTensor + Normalize of CLIP's `_transform` (openai clip.py `_transform`, called through
 *   avssl/data/{flickr,coco}_dataset.py image_transform): uint8 [B,H,W,3] (host pointers: mean3 / std3) -> f32 [B,3,H,W]. */
int sc_image_normalize_u8(const void* u8_hwc, float* out_chw, int B, int H, int W, const float* mean3, const float* std3, void* stream);
/* sc_image_prep_u8: the WHOLE `_transform` on the device for a ragged batch of decoded 8-bit images: Resize(n_px, BICUBIC) -> CenterCrop(n_px) ->
 *   convert("RGB") -> ToTensor -> Normalize.  BYTE-EXACTNESS CONTRACT: the uint8 crop equals PIL's `Image.resize(..., BICUBIC)` + `crop` on every byte
 *   (Pillow's 8-bit resampler is integer arithmetic on fixed-point tables; the kernels execute the tables the host plan supplies,
 *   speechclip_amd/data/image_transforms.py), and the f32 output equals sc_image_normalize_u8 of that crop bit for bit.  Only BICUBIC on 8-bit RGB / L
 *   images is restated; other modes are resized on the host and arrive as n_px x n_px RGB images with no pass.  Only the crop window is computed.
 *   packed   device uint8 [packed_bytes]: the images back to back (any gaps allowed), each HWC with C in {1, 3}
 *   offsets  int64 [2][B]: byte offset of image b in `packed`, then byte offset of its share of `workspace` (shares back to back in batch order)
 *   geom     int32 [B][SC_IMAGE_PREP_GEOM]: w, h, C, left, top (window origin in the resized image), row0, row1 (first / last input row the window
 *            needs), passes (SC_IMAGE_PREP_HPASS | SC_IMAGE_PREP_VPASS), htab, vtab (int32 index of the axis' table in `tables`)
 *   tables   int32 [tables_len], one record per distinct size pair: in_size, out_size, ksize, bounds [out][2] = (first input pixel, taps),
 *            coef [out][ksize] (22 fractional bits); may be NULL when no image runs a pass; the tap count is not capped
 *   offsets / geom / tables are passed TWICE, as host memory (`*_host`: every rule is checked there before any launch) and as the device copy of the same
 *   bytes the kernels read.  out_chw f32 [B,3,n_px,n_px]; out_u8 (may be NULL) uint8 [B,n_px,n_px,3]; C = 1 writes its value to all three channels.
 *   workspace: sc_image_prep_workspace_bytes bytes: 0 when B == 0 or no image runs the horizontal pass; -1 for what the entry would refuse as far as this
 *   function sees it (NULL geom, B < 0, n_px <= 0, C outside {1, 3}, row1 < row0).
 *   Every output element is written once, no atomics, no host synchronisation, integer arithmetic before the final normalise, 64-bit addressing.
 *   Refused (nonzero rc + sc_last_error, nothing launched): C outside {1, 3}; n_px <= 0; a window outside the resized image; needed rows outside
 *   [0, h); bounds that leave the image; an image outside `packed`; a workspace smaller than required; NULL tables when a pass runs. */
#define SC_IMAGE_PREP_GEOM 10
#define SC_IMAGE_PREP_HPASS 1
#define SC_IMAGE_PREP_VPASS 2
int64_t sc_image_prep_workspace_bytes(const int32_t* geom_host, int B, int n_px);
int sc_image_prep_u8(const void* packed, int64_t packed_bytes, const int64_t* offsets_host, const int64_t* offsets, const int32_t* geom_host,
                     const int32_t* geom, const int32_t* tables_host, const int32_t* tables, int64_t tables_len, int B, int n_px, const float* mean3,
                     const float* std3, void* workspace, int64_t workspace_bytes, float* out_chw, void* out_u8, void* stream);
int sc_vit_patchify(const float* img, void* cols, int B, int R, int p, int Kpad, void* stream);
int sc_vit_embed(const void* patch, const float* cls, const float* pos, const float* gamma, const float* beta, float* out, int B,
                 int ntok, int D, float eps, void* stream);

/* ---- Masked InfoNCE -- avssl/module/losses.py:185-245 (any global batch size) ------------------
 * feat_a/feat_b f32 [Bg,E] (unit norm), ids int64 [Bg] or NULL, out3 = {loss, a2b term, b2a term}. */
int64_t sc_infonce_workspace_bytes(int Bg);
int sc_infonce_fwd(const float* feat_a, const float* feat_b, const int64_t* ids, void* workspace, float* out3, int Bg, int E,
                   float inv_temperature, float margin, int dcl, int a2b, int b2a, void* stream);

/* ---- Cascaded-branch extras (fp32) -- avssl/model/kwClip.py:883-909 -------------------------------
 * sc_kw_affine: eval-mode Kw_BatchNorm (kw_bn.py:122-131) as out[r,d] = x[r,d]*scale[r%K,d] + shift[r%K,d].
 * sc_cosine_scores: F.cosine_similarity of every keyword against every sub-word embedding (kwClip.py:889-898):
 *   out[r,v] = a_r . e_v / (max(|a_r|,eps) max(|e_v|,eps)), a f32 [R,E], emb f32 [V,E], out f32 [R,V].
 * sc_vq_fwd: SimpleVectorQuantizer eval path (my_vector_quantizer.py:64-165): ids in host_mask_ids get -inf,
 *   targets[r] = arg-max, stats2 = {code_perplexity, prob_perplexity}, ent_per_t[k] (K keywords; rows r = b*K + k).
 * sc_gather_rows: out[r,:] = src[idx[r],:]  (one-hot @ E, kwClip.py:909). */
int sc_kw_affine(const float* x, const float* scale, const float* shift, float* out, int64_t rows, int K, int D, void* stream);
int64_t sc_cosine_workspace_bytes(int R, int V);
int sc_cosine_scores(const float* a, const float* emb, void* workspace, float* out, int R, int V, int E, float eps, void* stream);
/* sc_cosine_refine: for score matrices produced on the MFMA path (three-term bf16 split GEMM, ~1e-5 accurate): every entry within `delta` of its
 *   row maximum is recomputed in fp32 as (a . e) / (max(|a|,eps) max(|e|,eps)), so the arg-max is decided by fp32 arithmetic (kwClip.py:889-909). */
int sc_cosine_refine(float* scores, const float* a, const float* emb, int R, int V, int E, float delta, float eps, void* stream);
/* sc_cosine_refine_masked: the same for a quantiser that masks sub-words afterwards (sc_vq_fwd's host_mask_ids, at most 8): the refined set is
 *   every UNMASKED entry within `delta` of the row's maximum over the UNMASKED columns; masked columns are neither read for the maximum nor
 *   rewritten.  Candidates are chosen from the values on entry, however many there are, and the result is bitwise repeatable.
 *   sc_cosine_refine is the n_mask = 0 case. */
int sc_cosine_refine_masked(float* scores, const float* a, const float* emb, int R, int V, int E, float delta, float eps,
                            const int32_t* host_mask_ids, int n_mask, void* stream);
int64_t sc_vq_workspace_bytes(int R, int V);
int sc_vq_fwd(const float* scores, int64_t* targets, float* stats2, float* ent_per_t, void* workspace, int R, int K, int V,
              const int32_t* host_mask_ids, int n_mask, void* stream);
int sc_gather_rows(const float* src, const int64_t* idx, float* out, int R, int E, void* stream);
/* sc_retrieval_ranks: rank[i] = number of candidates ranked ahead of row i's best candidate carrying own_ids[i] (stable descending order;
 *   m if no candidate matches): recall@K of mutualRetrieval (avssl/module/retrieval.py:45-121) is mean(rank < K), without sorting.
 *   score f32 [n, m] (ld elements per row), own_ids i64 [n], cand_ids i64 [m]. */
int sc_retrieval_ranks(const float* score, int64_t ld, const int64_t* own_ids, const int64_t* cand_ids, int32_t* rank, int n, int m, void* stream);

/* ==== Trainable tail: forward-for-training and backward of the parallel branch, the layer-mix weights,
 * L2 normalisation and the masked InfoNCE loss, Adam and gradient clipping.  All fp32 (master weights), except the frozen encoder's bf16
 * hidden states.  Replaces `loss.backward()` + `optimizer.step()` of the Lightning loop (kwClip.py:143-191 -> training_step_end;
 * trainer.gradient_clip_val, audio_encoder.optim / scheduler in config/speechCLIP/model_base/spchclp_p.yaml:96-118).
 *
 * sc_sgemm: C[M,N] = alpha op(A)[M,K] op(B)[K,N] + beta C (+ bias[N]); row-major, fp32 SIMT.  transa=1: A stored [K,M];
 *   transb=1: B stored [N,K] (nn.Linear weight).  Every dense product of the tail has only B (pairs per GPU) rows on one side. */
int sc_sgemm(int transa, int transb, int M, int N, int K, float alpha, const float* A, int64_t lda, const float* B, int64_t ldb, float beta,
             float* C, int64_t ldc, const float* bias, void* stream);
int sc_sgemm_batched(int transa, int transb, int M, int N, int K, float alpha, const float* A, int64_t lda, int64_t strideA, const float* B,
                     int64_t ldb, int64_t strideB, float beta, float* C, int64_t ldc, int64_t strideC, const float* bias, int64_t strideBias,
                     int batch, void* stream);   /* operand i of the batch at X + i*strideX: the per-head products in one launch */
/* sc_cls_pool_train_fwd: sc_cls_pool_fwd with fp32 CLS tokens / outputs, the softmax probabilities kept (p_out f32 [B,R,NQ+T]) and
 *   attention-probability dropout (nn.MultiheadAttention dropout=0.1, TransformerModels.py:62-71) from a counter-based hash RNG.
 * sc_cls_pool_bwd: two streaming passes over the frames.  In: p (from the forward), dzbar f32 [B,R,D] (gradient of the pooled sums), u f32 [R,D];
 *   hidden bf16 (f32 when hidden_f32: the pre-LN encoder's residual stream) [n_layers][B*T, D] (layer_stride elements apart) = the states the frames were mixed from (NULL / n_layers = 0: skip dalpha).
 *   Out (PARTIAL rows, B*nsplit of them -- the keys of an utterance are split over nsplit blocks; every consumer sums over rows):
 *   du f32 [B*nsplit,R,D], dcls_key f32 [B*nsplit,NQ,D] (gradient reaching the CLS tokens as KEYS), dalpha f32 [B*nsplit,n_layers]
 *   (gradient of the softmaxed mix weights, weighted_sum.py:38-43).  ds_ws / pp_ws: f32 [B,R,NQ+T] workspaces. */
int sc_cls_pool_train_fwd(const void* x, int64_t ld_x, const float* cls_tok, const float* scores, const float* cls_scores,
                          const int32_t* lens, float* p_out, float* xbar, int B, int T, int NQ, int R, int D, float drop_p, uint32_t seed,
                          void* stream);
int sc_cls_pool_bwd(const void* x, int64_t ld_x, const float* cls_tok, const void* hidden, int hidden_f32, int64_t layer_stride, int n_layers,
                    int normalize,
                    const float* p, const float* dzbar, const float* u, const int32_t* lens, float* ds_ws, float* pp_ws, float* du,
                    float* dcls_key, float* dalpha, int B, int T, int NQ, int R, int D, int nsplit, float drop_p, uint32_t seed, void* stream);
/* Row ops, fp32.  sc_layernorm_bwd: dx (= or += when accumulate_dx) and dgamma/dbeta += (NULL: skipped); stats_ws f32 [rows,2].
 * sc_gelu_f32: backward=0: y = gelu(z) (exact erf);  backward=1: y_or_dh *= gelu'(z).   sc_colsum: out[c] (=|+=) sum_r x[r,c].
 * sc_l2norm_bwd: y = x/|x| (kwClip.py:1436).  sc_dropout_f32: y = x * keep/(1-p) with keep = hash(seed, index) (in place allowed).
 * sc_mix_softmax_bwd: dw += softmax-backward of the column sums of dalpha_b [B,n]. */
int sc_layernorm_bwd(const float* x, const float* dy, const float* gamma, float* dx, float* dgamma, float* dbeta, float* stats_ws, int rows,
                     int D, float eps, int accumulate_dx, void* stream);
int sc_gelu_f32(const float* z, float* y_or_dh, int64_t n, int backward, void* stream);
int sc_colsum(const float* x, int64_t ld, int rows, int cols, float* out, int accumulate, void* stream);
int sc_l2norm_bwd(const float* x, const float* dy, float* dx, int rows, int D, void* stream);
int sc_dropout_f32(const float* x, float* y, int64_t n, float drop_p, uint32_t seed, void* stream);
int sc_add_rows_f32(const float* a, const float* b, float* out, int rows, int cols, int b_rows, float alpha, void* stream);   /* out = alpha*a + b[r % b_rows] */
int sc_mix_softmax_bwd(const float* w, const float* dalpha_b, int B, int n, float* dw, void* stream);
/* Cascaded tail, training (kwClip.py:868-916 under loss.backward(); gradients reach the keyword branch THROUGH the frozen CLIP text tower).
 * sc_attn_small_bwd: causal self-attention backward over L <= 16 live positions (clip_official.py:220-264: only SOT, K keywords, EOT matter
 *   under the causal mask), qkv bf16 [B*L, 3W] as saved by the forward, dout f32 [B*L, W] -> dqkv f32 [B*L, 3W]; head_dim 64.
 * sc_quickgelu_f32: backward=0: y = z sigmoid(1.702 z) (f32, or bf16 when out_bf16); backward=1: y_or_dh (f32) *= d/dz.
 * sc_vq_st_bwd: straight-through estimator of SimpleVectorQuantizer (my_vector_quantizer.py:133-141, hard, no gumbel):
 *   dprob_inout f32 [R,V] (d loss / d subword_prob) -> d loss / d cos_scores = p (dprob - sum p dprob) / temp, p = softmax(cos / temp) over the
 *   unmasked sub-words (masked columns get 0); rowdot[r] = sum_v dcos cos.
 * sc_cosine_bwd_finish: da = (G - rowdot a/|a|) / |a| with G = dcos @ (emb/|emb|) (one sc_sgemm): backward of F.cosine_similarity (kwClip.py:889-897).
 * sc_kw_bn_train_fwd / sc_kw_bn_bwd: Kw_BatchNorm eachKw+parallel in train mode (kw_bn.py:122-131): batch statistics over the B rows of
 *   x f32 [B,K,E]; gamma/beta/running_* are indexed e*K + k (the reference flattens (B,E,K)); running statistics updated in place with
 *   `momentum` (unbiased variance), NULL: not tracked.  mean_out / rstd_out f32 [K*E] (data order) feed the backward. */
/* sc_split_hilo_bf16: out bf16 [M, 2K] = (bf16(a) | bf16(a - bf16(a))): a @ W^T = out @ [W | W]^T keeps ~16 mantissa bits of an fp32 gradient on the
 *   bf16 MFMA GEMM (the dX products against the frozen text tower / sub-word table). */
int sc_split_hilo_bf16(const float* a, int64_t lda, void* out, int64_t M, int K, int nblk, void* stream);   /* nblk 2: (hi|lo); 3: (hi|lo|hi) */
int sc_attn_small_bwd(const void* qkv, const float* dout, float* dqkv, int B, int L, int heads, int head_dim, int causal, void* stream);
int sc_quickgelu_f32(const float* z, void* y_or_dh, int64_t n, int backward, int out_bf16, void* stream);
int sc_vq_st_bwd(const float* cos_scores, float* dprob_inout, float* rowdot, int R, int V, float temp, const int* mask_ids, int n_mask, void* stream);
int sc_cosine_bwd_finish(const float* a, const float* G, const float* rowdot, float* da, int R, int E, float eps, void* stream);
/* SimpleVectorQuantizer, the modes beside the shipped one (my_vector_quantizer.py:124-139 in train mode; csrc/vq_modes.hip):
 *   y = softmax((x + g) / T) over the unmasked sub-words, x = scores f32 [R,V], g = Gumbel noise (use_gumbel) or 0, masked columns: probability and gradient 0.
 *   soft (hard: false): subword_prob = y, keywords = y @ emb; gumbel hard: subword_prob = one-hot(arg-max(x + g)), gradient through y; gumbel soft: both from y.
 * NOISE CONTRACT (part of the ABI: the backward and any host restatement regenerate it): idx = r * V + v as uint32 (R * V >= 2^32 is refused),
 *   h = hash32(seed ^ hash32(idx + 0x9e3779b9)) with hash32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (the dropout hash),
 *   u = ((h >> 9) + 0.5) * 2^-23 (exact in fp32, in [2^-24, 1 - 2^-24]), e = -log u (the Exponential(1) draw of F.gumbel_softmax), g = -log e in [-2.82, 16.64];
 *   both logarithms are the accurate logf.  Every entry: seed_on = 0 means g = 0 (seed ignored); mask ids as in sc_vq_st_bwd (at most 8); no atomics, results
 *   bitwise identical run to run.  A row with EVERY column masked (V <= 8) has y = 0: sc_vq_probs writes a row of zeros, sc_vq_soft_embed a zero keyword row
 *   with row_max = -inf and row_den = 0, sc_vq_mode_bwd dcos = 0 and both rowdots 0, sc_vq_noisy_argmax target 0.
 * sc_vq_gumbel_noise: out f32 [R,V] = g.
 * sc_vq_noisy_argmax: targets[r] = arg-max_v (x + g) over the unmasked sub-words, the lowest index on ties.
 * sc_vq_probs: out f32 [R,V] = y (dense; for the lazy `subword_prob` and for shapes sc_vq_soft_embed does not cover).
 * sc_vq_soft_table: the sub-word table emb f32 [V,E] (E % 64 == 0) as the bf16 (hi, lo) B operand of v_mfma_f32_16x16x32_bf16, sc_vq_soft_table_bytes(V, E) bytes:
 *   table[half][vb][et][lane][j] = half(emb[32 vb + 8 (lane >> 4) + j][16 et + (lane & 15)]), hi = bf16(emb), lo = bf16(emb - hi), rows beyond V zero.
 * sc_vq_soft_embed: keywords f32 [R,E] = y @ emb without an [R,V] image of y: a pre-pass writes row_max[r] = max_v (x + g) and
 *   row_den[r] = sum_v exp((x + g - row_max) / T); the main kernel forms 128 x 32 tiles of P = exp(..) / row_den, split (hi, lo), and accumulates
 *   P_hi E_hi + P_lo E_hi + P_hi E_lo on the MFMA.  V is split over `nsplit` chunks (0 = auto: about one block per CU); P being normalised, the partial products
 *   [nsplit, R, E] in `workspace` (sc_vq_soft_embed_workspace_bytes; none for one chunk) add in a fixed order.  Returns 1 without a launch ("not covered")
 *   unless E % 64 == 0 and V >= 5.
 * sc_vq_mode_bwd: dprob_inout f32 [R,V] (d loss / d y) -> d loss / d cos = y (dprob - sum y dprob) / T in place; rowdot_cos[r] = sum_v dcos cos (for
 *   sc_cosine_bwd_finish), rowdot_z[r] = sum_v dcos (cos + g): d loss / d T = -(1 / T) sum_r rowdot_z[r].  With seed_on = 0 it returns sc_vq_st_bwd's bits. */
int sc_vq_gumbel_noise(float* out, int R, int V, uint32_t seed, void* stream);
int sc_vq_noisy_argmax(const float* scores, int64_t* targets, int R, int V, uint32_t seed, int seed_on, const int* mask_ids, int n_mask, void* stream);
int sc_vq_probs(const float* scores, float* out, int R, int V, float temp, uint32_t seed, int seed_on, const int* mask_ids, int n_mask, void* stream);
int64_t sc_vq_soft_table_bytes(int V, int E);
int sc_vq_soft_table(const float* emb, void* table, int V, int E, void* stream);
int64_t sc_vq_soft_embed_workspace_bytes(int R, int V, int E, int nsplit);
int sc_vq_soft_embed(const float* scores, const void* table, float* keywords, float* row_max, float* row_den, void* workspace, int R, int V, int E,
                     float temp, uint32_t seed, int seed_on, const int* mask_ids, int n_mask, int nsplit, void* stream);
int sc_vq_mode_bwd(const float* cos_scores, float* dprob_inout, float* rowdot_cos, float* rowdot_z, int R, int V, float temp, uint32_t seed, int seed_on,
                   const int* mask_ids, int n_mask, void* stream);
int sc_kw_bn_train_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean_out, float* rstd_out, float* running_mean,
                       float* running_var, int B, int K, int E, float momentum, float eps, void* stream);
int sc_kw_bn_bwd(const float* x, const float* dy, const float* gamma, const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta,
                 int B, int K, int E, void* stream);
/* sc_infonce_bwd: G[Bg,Bg] = d loss / d logits and dinv_out[0] = d loss / d inv_temperature (losses.py:161,:219 trainable temperature),
 *   from the workspace sc_infonce_fwd filled for the same inputs; d loss / d feat_a = inv_temperature * G . feat_b (one sc_sgemm). */
int64_t sc_infonce_bwd_workspace_bytes(int Bg);
int sc_infonce_bwd(const float* feat_a, const float* feat_b, const int64_t* ids, const void* fwd_workspace, void* bwd_workspace, float* G,
                   float* dinv_out, int Bg, int E, float inv_temperature, float margin, int dcl, int a2b, int b2a, void* stream);
/* Optimizer over ONE flat fp32 buffer holding all trainable parameters (and a same-shaped gradient buffer):
 * sc_grad_norm: out2 = {|g|_2, min(1, max_norm/(|g|_2 + 1e-6))} (torch.nn.utils.clip_grad_norm_; Lightning gradient_clip_val).
 * sc_adam_step: torch.optim.Adam semantics (L2 weight decay into the gradient, bias correction), gradient scaled by *clip_coef. */
int64_t sc_grad_norm_workspace_bytes(void);
int sc_grad_norm(const float* g, int64_t n, float max_norm, void* workspace, float* out2, void* stream);
int sc_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* clip_coef, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int step, void* stream);

/* ---- Deterministic reductions: the three order-dependent sums of the tail (split-K sc_sgemm, chunked sc_colsum, the 8 waves of
 * sc_cls_pool_bwd) with ONE writer per element and a stated order, no atomics.  Same arithmetic inside a slice / chunk / wave as the default
 * entries, same tile shapes and the same split rules, so the default entries' error bounds hold unchanged; only the order in which the
 * partial sums meet is fixed.  Every "+" and "*" below is one correctly rounded fp32 operation, never contracted into an FMA, so the
 * chains can be restated bit for bit in fp32 on a host.  Workspaces are caller-owned, must not be shared between streams, and need no
 * initialisation; their contents after the call are the partials described here.
 *
 * sc_sgemm_batched_det / sc_sgemm_det: sc_sgemm_batched / sc_sgemm.  slices = sc_sgemm_det_slices (the split-K rule of sc_sgemm_batched),
 *   workspace f32 [batch][slices][M][N] = sc_sgemm_det_workspace_bytes = slices * M * N * batch * 4.
 *   slices == 1: the call IS sc_sgemm_batched (same kernel, same bits); the workspace is not touched and may be NULL.
 *   slices  > 1: slice s stores p_s = alpha * acc_s (acc_s: the FMA chain over its K range, ascending k) to workspace[b][s]; then
 *       C = (...((t + p_0) + p_1) + ... ) + p_{slices-1},   t = beta * C (+0 when beta == 0: C is not read), then t = t + bias[n] when bias is given.
 * sc_colsum_det: sc_colsum.  chunks = sc_colsum_det_chunks (the chunk rule of sc_colsum), workspace f32 [chunks][cols] =
 *   sc_colsum_det_workspace_bytes = chunks * cols * 4.  chunks == 1: the call IS sc_colsum.  chunks > 1: chunk k stores its sum p_k (four
 *   row-interleaved partials q_0..q_3, p_k = (q_0 + q_1) + (q_2 + q_3)) to workspace[k]; then out = (...((p_0 + p_1) + p_2) ...) + p_{chunks-1},
 *   and out = that + old out when accumulate.
 * sc_cls_pool_bwd_det: sc_cls_pool_bwd, same arguments and outputs.  Wave w of a block owns keys w, w + 8 * nsplit, ... of its key split and
 *   accumulates du and dalpha over them in ascending key; the block's result is ((w_0 + w_1) + w_2) + ... + w_7 for every element of du and
 *   dalpha.  dcls_key, ds_ws and pp_ws have one writer in both entries and are bit-identical to sc_cls_pool_bwd's.  The B * nsplit partial
 *   rows are summed by the caller (sc_colsum_det / sc_sgemm_det for a fixed order). */
int sc_sgemm_det_slices(int M, int N, int K, int batch);
int64_t sc_sgemm_det_workspace_bytes(int M, int N, int K, int batch);
int sc_sgemm_batched_det(int transa, int transb, int M, int N, int K, float alpha, const float* A, int64_t lda, int64_t strideA, const float* B,
                         int64_t ldb, int64_t strideB, float beta, float* C, int64_t ldc, int64_t strideC, const float* bias, int64_t strideBias,
                         int batch, void* workspace, int64_t workspace_bytes, void* stream);
int sc_sgemm_det(int transa, int transb, int M, int N, int K, float alpha, const float* A, int64_t lda, const float* B, int64_t ldb, float beta,
                 float* C, int64_t ldc, const float* bias, void* workspace, int64_t workspace_bytes, void* stream);
int sc_colsum_det_chunks(int rows, int cols);
int64_t sc_colsum_det_workspace_bytes(int rows, int cols);
int sc_colsum_det(const float* x, int64_t ld, int rows, int cols, float* out, int accumulate, void* workspace, int64_t workspace_bytes,
                  void* stream);
int sc_cls_pool_bwd_det(const void* x, int64_t ld_x, const float* cls_tok, const void* hidden, int hidden_f32, int64_t layer_stride, int n_layers,
                        int normalize, const float* p, const float* dzbar, const float* u, const int32_t* lens, float* ds_ws, float* pp_ws,
                        float* du, float* dcls_key, float* dalpha, int B, int T, int NQ, int R, int D, int nsplit, float drop_p, uint32_t seed,
                        void* stream);

/* ---- Fine-tuning HuBERT transformer layers (speech_encoder_plus.py:416-446: `trainable` with `reinit_layers` / `unfreeze_layers`; the feature
 * extractor, positional conv and projections stay frozen as the reference freezes them in those modes).  The dense products of the backward
 * run on sc_gemm_bf16 / sc_gemm_bf16_batched (dX = dY W on transposed weight copies; dW = dY^T X as a split-K batched product over
 * transposed activations); these are the pieces around them.
 *   sc_transpose_bf16: batch of [rows, cols] -> [cols, rows_padded] (rows >= `rows` zero filled: the TN products' K must be a multiple of 64).
 *   sc_attn_softmax_bwd: per (batch z, query i): P = softmax(scale S + mask(keys >= klens[z])) and dS = scale P (dP - dO_i . O_i), from
 *     S = Q K^T and dP = dO V^T (f32 [batch, Lp, ld]); dO / O: bf16 rows (z*rows_per_batch + i) of 64 head dims; P / dS: bf16 [batch, Lp, ld].
 *   sc_gelu_bwd_bf16: du = dh gelu'(u), exact erf form.   sc_axpy_bf16: y += alpha x.
 *   sc_layernorm_bwd_bf16: dx per row + partial column sums part f32 [sc_layernorm_bwd_bf16_partials(rows), 2, D] (dgamma, dbeta rows; the
 *     caller reduces them with sc_colsum).   sc_colsum_bf16: out[c] (=|+=) sum_r x[r,c], two deterministic stages.
 *   sc_cls_pool_dz: d loss / d (mixed frames) from sc_cls_pool_bwd's workspaces: dz[b,t] = sum_r pp[b,r,NQ+t] dzbar[b,r] + ds[b,r,NQ+t] u[r]. */
int sc_transpose_bf16(const void* in, int64_t ld_in, int64_t stride_in, void* out, int64_t ld_out, int64_t stride_out, int rows, int cols,
                      int rows_padded, int batch, void* stream);

/* ---- backward of the HuBERT front end: `audio_encoder.trainable: true` with no layer lists trains the conv feature extractor, post_extract_proj,
 * layer_norm and the positional conv as well (avssl/module/speech_encoder_plus.py:399-401: freeze_model is not called; [3P fairseq]
 * HubertModel.forward_features scales the extractor's gradient by feature_grad_mult).  GEMM-shaped parts reuse sc_gemm_bf16 / sc_gemm_bf16_batched /
 * sc_posconv_conv (speechclip_amd/train_front.py); these entries are the rest:
 * Each operation is ONE kernel serving both row layouts: uniform rows (B utterances of Tp rows) are the packed layout with row_off[b] = b * Tp and
 * rows_b = Tp.  The entries below take the uniform layout; their *_packed forms (further down) take row_off and forward into the same code.
 *   sc_posconv_finish_train: training forward of the positional-conv tail (speech_encoder_plus.py:35-37): u = conv + bias regrouped from the conv slabs
 *     (utterance b = [G][rows_b][D/G] at element row_off[b] * D; uniform: [B, G, Tp, D/G]) to bf16 [rows, D], s = mask(x) + gelu(u) (bf16, the GELU taken
 *     at the bf16-rounded u; the LayerNorm after it runs as sc_layernorm) -- both kept for the backward.  D/G a multiple of 4 (8 elements per thread when
 *     it is a multiple of 8, else 4).
 *   sc_posconv_dgrad_finish: dx = mask(ds + time-reversed regroup of convT), convT = sc_posconv_conv of the time-reversed du with the in/out
 *     channel-swapped weights (the adjoint of "pad Kw/2, drop the last output" is the same conv on the reversed sequence); rows >= valid[b] are zeros.
 *   sc_reverse_rows_bf16: out[b, t, :] = in[b, T-1-t, :] (packed: inside each utterance's own rows).
 *   sc_conv0_bwd: conv layer 0 = Conv1d(1 -> C, k 10, s 5, no bias) -> GroupNorm(C groups, statistics over the T0 frames) -> GELU, from the wave:
 *     dy bf16 [B, P, C] -> part f32 [B, C, 12] = per-utterance (dw[0..9], dgamma, dbeta); sum over B for the parameter gradients.
 * Zero rows (B * Tp == 0, B == 0) return 0 without a launch. */
int sc_posconv_finish_train(const void* x, const int32_t* valid, const void* conv, const float* bias, void* u, void* s, int B, int Tp, int D, int G,
                            void* stream);
int sc_posconv_dgrad_finish(const void* convT, const void* ds, const int32_t* valid, void* dx, int B, int Tp, int D, int G, void* stream);
int sc_reverse_rows_bf16(const void* in, void* out, int B, int T, int D, void* stream);
int sc_conv0_bwd(const float* wav, int64_t ld, const float* w, const float* gamma, const float* beta, const void* dy, float* part, int B, int C, int T0,
                 int P, float eps, void* stream);
/* conv layer 0 of the LayerNorm extractor (HuBERT-large: conv + bias -> LayerNorm(C) -> GELU; the LayerNorm / GELU backward runs on the row kernels):
 * du bf16 [B, P, C] = gradient of the conv output -> part f32 [B, C, 12] = per-utterance (dw[0..9], dbias, 0). */
int sc_conv0_wgrad(const float* wav, int64_t ld, const void* du, float* part, int B, int C, int T0, int P, void* stream);
int sc_attn_softmax_bwd(const float* S, const float* dP, int64_t ld, int64_t stride, const void* dO, int64_t ld_do, const void* O, int64_t ld_o,
                        int64_t rows_per_batch, const int32_t* klens, void* P, void* dS, int L, int Lp, int batch, float scale, void* stream);
/* sc_attn_softmax_bwd for a forward that ran sc_attention_fwd_dropout with (drop_p, seed): P comes out masked and rescaled (dV = P^T dO sees the
 * dropped probabilities), dP is masked before the softmax backward; batch z = utterance b, head h of H (the forward's mask index). */
int sc_attn_softmax_bwd_dropout(const float* S, const float* dP, int64_t ld, int64_t stride, const void* dO, int64_t ld_do, const void* O, int64_t ld_o,
                                int64_t rows_per_batch, const int32_t* klens, void* P, void* dS, int L, int Lp, int batch, float scale, float drop_p,
                                uint32_t seed, int H, int h, void* stream);
/* the same for ALL heads in one launch: S / dP / P / dS are [B*H, Lp, ld] images (z = b*H + h), dO / O the [rows, H*64] matrices; drop_p = 0: plain */
int sc_attn_softmax_bwd_heads(const float* S, const float* dP, int64_t ld, int64_t stride, const void* dO, int64_t ld_do, const void* O, int64_t ld_o,
                              int64_t rows_per_batch, const int32_t* klens, void* P, void* dS, int L, int Lp, int B, int H, float scale, float drop_p,
                              uint32_t seed, void* stream);
/* Fused form of the two recompute products + sc_attn_softmax_bwd_heads for head dim 64: P / dS bf16 [B*H, Lp, Lp] straight from the packed q | k | v
 * rows (row b*L + t of stride ld_qkv, head h at column h*64), dO and O (stride ld_o); the fp32 S / dP images are never written. */
int sc_attn_bwd_probs(const void* q, const void* k, const void* v, int64_t ld_qkv, const void* dO, const void* O, int64_t ld_o, const int32_t* klens,
                      void* P, void* dS, int B, int H, int L, int Lp, float scale, float drop_p, uint32_t seed, void* stream);
/* Argument rules (a violation returns non-zero with the message in sc_last_error(); a call of size zero -- n, rows or cols <= 0 -- returns 0 and
 * touches nothing; every operand is aligned to its element size):
 *   sc_gelu_bwd_bf16       n even; u, dh, du 16-byte aligned.
 *   sc_layernorm_bwd_bf16  D a multiple of 64, at most 1024; no operand null; x, dy, dx 8-byte aligned when D % 256 == 0 (the 8-byte kernel; rows are
 *                          contiguous, so the base decides for every row); part holds sc_layernorm_bwd_bf16_partials(rows) rows of 2 D floats.
 *   sc_colsum_bf16         no operand null; cols <= 65535 * 256; ld >= cols; ws holds sc_colsum_bf16_workspace_bytes(rows, cols) bytes.
 *   sc_axpy_bf16           n even; y, x not null and 4-byte aligned (the kernel moves pairs). */
int sc_gelu_bwd_bf16(const void* u, const void* dh, void* du, int64_t n, void* stream);
int64_t sc_layernorm_bwd_bf16_partials(int64_t rows);
int sc_layernorm_bwd_bf16(const void* x, const void* dy, const float* gamma, void* dx, float* part, int64_t rows, int D, float eps, void* stream);
int64_t sc_colsum_bf16_workspace_bytes(int64_t rows, int cols);
int sc_colsum_bf16(const void* x, int64_t ld, int64_t rows, int cols, float* ws, float* out, int accumulate, void* stream);
int sc_axpy_bf16(void* y, const void* x, float alpha, int64_t n, void* stream);
int sc_cls_pool_dz(const float* pp, const float* ds, const float* dzbar, const float* u, const int32_t* lens, void* dz, int B, int T, int NQ, int R,
                   int D, int64_t ld_dz, void* stream);

/* ---- Fine-tuning the CLIP image tower (clip_official.py `image_encoder_trainable`: model.visual trains).  The ViT blocks run on the pre-LN layer
 * pieces above; these are the ViT-specific ones (train_vit.hip).
 *   sc_quickgelu_bwd_bf16: du = dh (s + 1.702 u s (1 - s)), s = sigmoid(1.702 u): bf16 in / out, fp32 arithmetic.  Any n >= 0 and any 2-byte-aligned
 *     operands; where u, dh and du share their address modulo 16 the body moves 16 bytes per lane.  du may be dh (in place).
 *   sc_vit_embed_bwd: adjoint of sc_vit_embed, x0 = LN_pre([cls | patch] + pos).  dx f32 [B*ntok, D] = d loss / d x0; patch bf16 [B*(ntok-1), D], cls f32 [D],
 *     pos f32 [ntok, D], gamma f32 [D]: the forward's inputs (the row, its mean and its rstd are recomputed; the forward saves nothing).  Outputs:
 *     dpatch bf16 [B*(ntok-1), D] = gradient of the pre-LN rows of tokens >= 1 (the dY of the patch GEMM); dpos f32 [ntok, D] = the gradient of every pre-LN
 *     row summed over the batch (row 0 is d loss / d cls); dgamma, dbeta f32 [D].  ntok >= 2, D % 4 == 0, D <= 1024; dx 16-byte, patch / dpatch 8-byte aligned
 *     (cls, pos, gamma and the f32 outputs: any 4-byte alignment, e.g. views of an optimizer's flat buffer).  Reduction order (fixed, no atomics, bitwise reproducible): block (token, batch split) adds its batch entries wave by wave in
 *     ascending order and writes one partial row triple into `workspace` (sc_vit_embed_bwd_workspace_bytes); the finish adds the splits in ascending
 *     order for dpos and all (split, token) partials as four interleaved running sums for dgamma / dbeta. */
int sc_quickgelu_bwd_bf16(const void* u, const void* dh, void* du, int64_t n, void* stream);
int64_t sc_vit_embed_bwd_workspace_bytes(int B, int ntok, int D);
int sc_vit_embed_bwd(const float* dx, const void* patch, const float* cls, const float* pos, const float* gamma, void* dpatch, float* dpos,
                     float* dgamma, float* dbeta, float* workspace, int B, int ntok, int D, float eps, void* stream);


/* ---- Padding-free (packed) batches.  The reference pads every utterance of a batch to the longest one (collate_function.py:18-30,
 * speech_encoder_plus.py:506-518, :540-556) and runs the conv stack and all transformer GEMMs on B x T_max rows; only rows below each
 * utterance's own length ever reach an output (padding mask, speech_encoder_plus.py:604-611).  Here utterance b owns rows
 * [row_off[b], row_off[b + 1]) of every transformer-level tensor (row_off: B + 1 device ints, row_off[0] = 0) and row_scale times that range at
 * conv layer 0, so all GEMMs run on sum_b rows_b rows.  The GEMM entries need no change (rows are rows); these are the per-utterance kernels:
 *   sc_conv0_fwd_packed      sc_conv0_fwd writing utterance b at rows row_scale * row_off[b] ..; `coef` = sc_conv0_gn_coef over the PADDED length
 *                            (zero samples add nothing to the GroupNorm sums, the divisor stays T0: the reference's statistics exactly)
 *   sc_posconv_conv_packed / sc_posconv_finish_packed   conv slab of utterance b = [G][rows_b][D/G] at element row_off[b] * D
 *   sc_attention_fwd_packed  fairseq MHA with key-padding mask over packed q|k|v rows (drop_p > 0: the train-mode form)
 *   sc_unpack_rows           packed -> the reference's padded [n_layers][B][T_out][row] layout: out[l][b][t] = t < rows_b - halo ? src row : 0.
 *                            The encoder passes halo = 1: the last row of every utterance is the receptive-field halo (inexact, reads the
 *                            neighbouring utterance's samples) and is not exposed; frames >= max(valid_b, feat_len_b) are zeros.
 * Whole-encoder training on packed rows (speechclip_amd/train_front.py) adds the backward's per-utterance kernels; none of them uses atomics:
 *   sc_conv0_bwd_packed / sc_conv0_wgrad_packed   the kernels of sc_conv0_bwd / sc_conv0_wgrad with dy / du read at rows row_scale * row_off[b] + t and taken
 *                            as zero for t >= row_scale * rows_b (uniform: row b * P + t, and P >= T0 makes the limit T0).  The wave stays the padded [B, ld];
 *                            the GroupNorm statistics and every sum of its backward run over all T0 frames of the padded length (frames the layout does not
 *                            materialise carry no dy but still enter the mean-subtraction terms).
 *   sc_posconv_finish_train_packed / sc_posconv_dgrad_finish_packed / sc_reverse_rows_packed_bf16   the kernels of the three uniform entries with the row's
 *                            utterance found in row_off (binary search) instead of by division, over sc_posconv_conv_packed's slab layout; with
 *                            row_off[b] = b * Tp they give the uniform entries' output bit for bit.  dx = mask(ds + conv^T du) with convT =
 *                            sc_posconv_conv_packed(reversed du, valid = rows_b, swapped weights); every row of u / s / dx / out is written.  They need
 *                            D/G (D for the reversal) a multiple of 8, B > 0, total_rows > 0 and row_off.
 *   sc_posconv_pack_gapped   out bf16 [G][slab_rows][D/G]: row lead + row_off[b] + b * gap + t of group g = row row_off[b] + t of x for t < min(lim[b], rows_b),
 *                            zeros everywhere else (slab_rows >= lead + total_rows + B * gap; every row written).  With gap = Kw a window of Kw rows never sees
 *                            two utterances, so the positional conv's dW is ONE [rows, cols] product: (x, lim = valid, lead = Kw/2) is its sliding-window
 *                            operand and (du, lim = rows_b, G = 1, lead = 0) the gradient in the same row numbering. */
int sc_conv0_fwd_packed(const float* wav, int64_t ld, int64_t L, const float* w, const float* bias, const float* coef, void* out, int B,
                        int C, int T0, const int32_t* row_off, int row_scale, int Pmax, int mode, void* wfrag_ws, void* stream);
int sc_posconv_conv_packed(const void* x, const int32_t* valid, const int32_t* row_off, const void* wg, void* conv, int B, int Tmax, int D, int G,
                           int Kw, void* stream);
int sc_posconv_finish_packed(const void* x, const int32_t* valid, const int32_t* row_off, const void* conv, const float* bias, const float* gamma,
                             const float* beta, void* out, int B, int64_t total_rows, int D, int G, int out_f32, float eps, void* stream);
int sc_conv0_bwd_packed(const float* wav, int64_t ld, const float* w, const float* gamma, const float* beta, const void* dy, float* part, int B, int C,
                        int T0, const int32_t* row_off, int row_scale, float eps, void* stream);
int sc_conv0_wgrad_packed(const float* wav, int64_t ld, const void* du, float* part, int B, int C, int T0, const int32_t* row_off, int row_scale,
                          void* stream);
int sc_posconv_finish_train_packed(const void* x, const int32_t* valid, const int32_t* row_off, const void* conv, const float* bias, void* u, void* s,
                                   int B, int64_t total_rows, int D, int G, void* stream);
int sc_posconv_dgrad_finish_packed(const void* convT, const void* ds, const int32_t* valid, const int32_t* row_off, void* dx, int B, int64_t total_rows,
                                   int D, int G, void* stream);
int sc_reverse_rows_packed_bf16(const void* in, const int32_t* row_off, void* out, int B, int64_t total_rows, int D, void* stream);
int sc_posconv_pack_gapped(const void* x, const int32_t* lim, const int32_t* row_off, void* out, int B, int64_t total_rows, int D, int G, int gap,
                           int lead, int64_t slab_rows, void* stream);
int sc_attention_fwd_packed(const void* q, const void* k, const void* v, void* out, const int32_t* klens, const int32_t* row_off, int B, int H,
                            int Tmax, int64_t total_rows, int head_dim, int64_t ld_qkv, int64_t ld_out, float scale, float drop_p, uint32_t seed,
                            int flags /* SC_ATTN_F16 or 0 */, void* stream);
int sc_unpack_rows(const void* src, int64_t src_layer_stride_bytes, const int32_t* row_off, void* out, int64_t out_layer_stride_bytes, int n_layers,
                   int B, int T_out, int row_bytes, int halo, void* stream);
/* sc_pack_rows: padded [n_layers][B][T_in][row] -> packed, the adjoint of sc_unpack_rows: out[l][row_off[b] + t] = t < min(rows_b - halo, T_in) ? in[l][b][t] : 0
 * for every row of every utterance (row_off[B] == total_rows). */
int sc_pack_rows(const void* src, int64_t src_layer_stride_bytes, const int32_t* row_off, void* out, int64_t out_layer_stride_bytes, int n_layers,
                 int B, int T_in, int64_t total_rows, int row_bytes, int halo, void* stream);

/* ---- CLIP text tower on packed rows (speech-text retrieval: ClipModel.encode_text with SC_TEXT_PACK=1, clip_official.py:211-218).  Caption b owns rows
 * [row_off[b], row_off[b + 1]) = its positions SOT .. EOT (row_off: B + 1 device int32, row_off[0] = 0, row_off[B] = total_rows): under the causal mask nothing
 * behind a caption's EOT reaches its feature, so those positions are not computed.  GEMMs and LayerNorms take the rows as they are.
 *   sc_text_embed_packed   out[row_off[b] + t][:] = tok[ids[b * ld_ids + t]][:] + pos[t][:] for t < row_off[b + 1] - row_off[b]; ids int64 [B, L] (row stride
 *                          ld_ids >= L), tok fp32 [V, W], pos fp32 [ctx, W], out fp32 [total_rows, W].  One fp32 add per element, float4 loads and stores,
 *                          nothing else is written.  PRECONDITION: every id in [0, V) and rows per caption <= min(L, ctx) (the caller checks both where it
 *                          finds the EOT positions); the kernel itself stays inside its operands (rows beyond L are not written, an id outside the table reads
 *                          the table's first / last row).  W % 4 != 0, a null operand, L > ctx, ld_ids < L or a misaligned table return an error, no launch.
 *   sc_attention_fwd_text  causal attention over packed rows, head_dim 64, bf16, operands as sc_attention_fwd_packed (head h at column h*64, ld_qkv / ld_out
 *                          multiples of 8, rows per caption <= Tmax): query t of caption b sees keys 0 .. t of caption b only.  No dropout, no SC_ATTN_F16, no klens.
 *                          Two forms.  GENERAL (any Tmax; forced by SC_ATTN_TEXT_GENERAL): sc_attention_fwd's kernel with row_off and the causal bit -- with
 *                          row_off[b] = b*T it returns sc_attention_fwd(..., SC_ATTN_CAUSAL) bit for bit.  SHORT-ROW (the default when Tmax <= 128; measured,
 *                          profiles/text_tower_bench.txt): one wave per (caption, head) unit, S = K.Q^T and P.V on v_mfma_f32_16x16x32_bf16 over the caption's
 *                          whole key range at once, fp32 scores and softmax in registers (no online rescale), every output row written once, no atomics; the
 *                          same roundings as the general form (P to bf16 before P.V, the row sum over the unrounded P, one rounding of the output).
 *                          Both forms: no row outside [row_off[b], row_off[b + 1]) is read for caption b (rows before the first and behind the last caption
 *                          may hold anything); V rows INSIDE a caption must be finite, as for sc_attention_fwd (keys behind the diagonal enter the P.V MFMA
 *                          with P = 0).  Any flag bit other than SC_ATTN_TEXT_GENERAL is refused. */
#define SC_ATTN_TEXT_GENERAL 0x100
int sc_text_embed_packed(const int64_t* ids, int64_t ld_ids, const float* tok, const float* pos, const int32_t* row_off, float* out,
                         int B, int L, int V, int ctx, int W, int64_t total_rows, void* stream);
int sc_attention_fwd_text(const void* q, const void* k, const void* v, void* out, const int32_t* row_off, int B, int H, int Tmax,
                          int64_t total_rows, int head_dim, int64_t ld_qkv, int64_t ld_out, float scale, int flags, void* stream);

/* ---- Fused attention backward over packed rows (fine-tuning on the padding-free layout), head_dim 64.  Operands as sc_attention_fwd_packed: bf16 rows,
 * head h at column h*64, utterance b at rows row_off[b] .. (row_off[B] == total_rows; rows per utterance <= Tmax), klens[b] valid keys; row_off == NULL:
 * the uniform layout row_off[b] = b*Tmax (total_rows = B*Tmax).  O / dO: the forward's output and its gradient (row stride ld_o); dq / dk / dv: row stride
 * ld_dqkv.  Flash-style: S = Q K^T and dP = dO V^T are recomputed on the MFMA in a key-tile-stationary sweep (dK, dV) and a query-tile-stationary sweep (dQ);
 * nothing of size L x L is written.  `workspace` (sc_attention_bwd_packed_workspace_bytes: 2 fp32 per (row, head)) receives the log-sum-exp and
 * delta = dO . O of a pre-pass.  No atomics: results are bitwise reproducible.  drop_p > 0: the forward ran with (drop_p, seed); its mask is regenerated
 * (P for dV is the dropped, rescaled one, dP is masked before the softmax backward: sc_attn_softmax_bwd_dropout's semantics).
 * Query rows >= klens[b] of an utterance take no part: dq = 0 there and they add nothing to dk / dv; key rows >= klens[b] get dk = dv = 0.  Every row
 * in [0, total_rows) of dq / dk / dv is written.  Rows >= klens[b] of q / k / v, O and dO may hold anything, NaN and Inf included (they are zeroed on load).
 * One kernel set (csrc/attention_bwd.hip) serves this entry and sc_attention_hd_bwd: at head_dim 64 on uniform rows without dropout the two return the same bits. */
int64_t sc_attention_bwd_packed_workspace_bytes(int64_t total_rows, int H);
int sc_attention_bwd_packed(const void* q, const void* k, const void* v, int64_t ld_qkv, const void* O, const void* dO, int64_t ld_o,
                            const int32_t* klens, const int32_t* row_off, int B, int H, int Tmax, int64_t total_rows, int head_dim, float scale,
                            float drop_p, uint32_t seed, void* dq, void* dk, void* dv, int64_t ld_dqkv, void* workspace, void* stream);

/* ---- Fused attention backward for head_dim 64 / 96 / 128: the backward of sc_attention_hd_fwd, operands addressed exactly as there (all bf16; element
 * (b, t, h, e) of q at b*q_bs + t*q_rs + h*head_dim + e, of k / v at b*kv_bs + ..., of O / dO (the forward's bf16 output and its gradient) at b*o_bs + ...,
 * of dq at b*dq_bs + ..., of dk / dv at b*dkv_bs + ...; every stride a multiple of 8 elements).  Served: Tq == Tk (self-attention rows) and Tq == 1 (the
 * CLS query of a branch's last layer); any other pair and any other head dim return an error.  The kernel set of sc_attention_bwd_packed (one set, two entries):
 * `workspace` (sc_attention_hd_bwd_workspace_bytes: 2 fp32 per (b, h, query row)) receives log-sum-exp and delta (dO . O; with drop_p > 0 the same number
 * taken before O's rounding, sum_k P_dropped dP, which sc_attention_bwd_packed does not do); a key-tile-stationary sweep
 * gives dK / dV, a query-tile-stationary sweep dQ; fp32 scores / softmax / accumulators; nothing of size Tq x Tk is written; no atomics (bitwise reproducible).
 * klens[b] is clamped to [0, Tk] (NULL = Tk).  Query row t takes part iff t < klens[b]: other query rows get dq = 0 and add nothing to dk / dv; key rows
 * >= klens[b] get dk = dv = 0; every row of dq / dk / dv is written.  K / V rows >= klens[b] and Q / dO rows that take no part may hold anything (they are
 * zeroed on load).  drop_p > 0: the forward ran with (drop_p, seed); its mask (pair index ((b*H + h)*Tk + t) * ceil(Tk / 2) + key / 2) is regenerated: P for
 * dV is the dropped, rescaled one, dP is masked before the softmax backward (sc_attn_softmax_bwd_dropout's semantics).  B == 0 or Tk == 0: returns 0, no launch. */
int64_t sc_attention_hd_bwd_workspace_bytes(int B, int H, int Tq);
int sc_attention_hd_bwd(const void* q, const void* k, const void* v, const void* O, const void* dO, const int32_t* klens,
                        int B, int H, int Tq, int Tk, int head_dim,
                        int64_t q_bs, int64_t q_rs, int64_t kv_bs, int64_t kv_rs, int64_t o_bs, int64_t o_rs,
                        void* dq, int64_t dq_bs, int64_t dq_rs, void* dk, void* dv, int64_t dkv_bs, int64_t dkv_rs,
                        float scale, float drop_p, uint32_t seed, void* workspace, void* stream);

/* ---- Gallery search: the K nearest gallery rows of every query row, fused fp32 similarity + top-K (csrc/search.hip).  No [Q, N] score image is formed:
 * the scores of a (query tile, gallery tile) pair live in MFMA accumulators, are filtered against the row's current K-th entry and only survivors reach a
 * per-row candidate list in LDS.  ARITHMETIC CONTRACT (restated on the host in tests/search_ref.py, which the tests judge against):
 *   score     s(i, j) = the fp32 chain  acc = +0.0f;  for e = 0 .. E-1 ascending:  acc = fmaf(q[i*ld_q + e], g[j*ld_g + e], acc)  -- one rounding per step, one
 *             accumulator per (i, j), never split over E and never reordered.  It is formed on v_mfma_f32_32x32x2_f32, whose result is that chain (k = 2t from
 *             lanes 0..31, k = 2t + 1 from lanes 32..63, in that order); subnormals are kept.
 *   order     pairs (s(i, j), j) are ordered by score descending, then j ascending (sc_topk_rows_f32's tie rule).  A NaN score takes no part.
 *   result    for query i the first K pairs of that order over j in [0, N): vals f32 [Q, K] = the scores, idx i64 [Q, K] = idx_base + j.  With fewer than K
 *             comparable scores the remaining slots hold -inf / -1.
 *   pure      the bits of row i of vals / idx depend on q[i, :E], g[:N, :E], K and idx_base only: not on the other queries, on i's position in the call, on
 *             n_split, on the previous contents of `workspace`, and on K only as a prefix (the result for K' < K is the first K' columns of the result for K).
 *             No global atomics; LDS counters only hand out candidate slots, and the list is always rebuilt by rank in the total order above.
 *   splits    the gallery is cut into n_split ranges of ceil(N / n_split) rows (trailing ranges may be empty), one block per (query tile, range), so that a
 *             single query against 10^6 rows still fills the chip; each block writes its K-list to `workspace` ([Q][n_split][K] i64, then the same in f32:
 *             sc_search_workspace_bytes = 12 Q n_split K bytes, 0 for one split, which writes vals / idx directly) and sc_topk_merge joins them.
 *             n_split = 0: sc_search_splits(Q, N, K) = clamp(min(ceil(512 / query_tiles), N / 256), 1, 1024) with query_tiles = ceil(Q / B) and
 *             B = 128 query rows per block when K <= 64 and Q > 64, else 64.  Both are pure host functions.
 *   reads     rows [0, Q) of q and [0, N) of g, E elements of each; nothing else.
 *   refused   (nonzero rc + sc_last_error, nothing launched) E % 4 != 0 or E outside [4, 1024]; ld_q / ld_g < E or not multiples of 4; q or g not 16-byte
 *             aligned; K outside [1, 128]; K > N; N >= 2^31; n_split outside [0, 1024]; Q < 0; a null operand; no workspace with more than one split.
 *             Q == 0 returns 0 and launches nothing.
 * sc_topk_merge: row r of vals_in f32 [Q, L] / idx_in i64 [Q, L] holds L candidates in any order; vals / idx [Q, K] receive the first K by (value
 *   descending, idx ascending).  Entries with idx < 0 or a NaN value take no part (they are how a short list is padded); missing slots hold -inf / -1.
 *   Entries of one row are expected to carry distinct idx (an exact duplicate pair is emitted once).  1 <= K <= 128, K <= L; outputs must not alias inputs. */
int sc_search_splits(int Q, int64_t N, int K);
int64_t sc_search_workspace_bytes(int Q, int64_t N, int K, int n_split);
int sc_search_topk(const float* q, int64_t ld_q, const float* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split,
                   int64_t idx_base, float* vals, int64_t* idx, void* workspace, void* stream);
int sc_topk_merge(const float* vals_in, const int64_t* idx_in, int Q, int L, int K, float* vals, int64_t* idx, void* stream);

/* ---- Gallery search, bf16 storage: sc_search_topk on rows stored in bf16 (csrc/search_bf16.hip) -- half the gallery bytes, the product on the bf16 MFMA.
 * q is bf16 [Q, E] with row stride ld_q, g is bf16 [N, E] with row stride ld_g (strides in elements); vals, idx, n_split, idx_base, `workspace`
 * (sc_search_workspace_bytes), the split rule (sc_search_splits) and the merge (sc_topk_merge) are those of sc_search_topk.  BF16 ARITHMETIC CONTRACT
 * (restated on the host in tests/search_bf16_ref.py):
 *   score     s(i, j) = sum over e of q[i*ld_q + e] * g[j*ld_g + e].  Every bf16 product is exact in fp32; the products are accumulated in fp32 by
 *             v_mfma_f32_32x32x16_bf16: one accumulator per (i, j), starting from +0.0f, E walked in ascending groups of 16, never split over blocks.  The
 *             order of the 16 additions inside one instruction is the hardware's and is NOT stated; what is stated is the bound
 *             |s(i, j) - exact sum| <= c * 2^-24 * sum over e of |q[i, e] g[j, e]|,  c = 2 E / (1 - 2 E 2^-24)  (E additions, each counted with twice the
 *             fp32 unit roundoff so that an adder that truncates is covered; derivation in tests/search_bf16_ref.py).  Sums of integers below 2^24 are
 *             exact.  Subnormal operands and subnormal products are outside the contract (the matrix pipe may flush them).
 *   order     pairs (s(i, j), j) are ordered by score descending, then j ascending (sc_topk_rows_f32's tie rule).  A NaN score takes no part.
 *   result    for query i the first K pairs of that order over j in [0, N): vals f32 [Q, K] = the scores, idx i64 [Q, K] = idx_base + j.  With fewer than K
 *             comparable scores the remaining slots hold -inf / -1.
 *   pure      the bits of row i of vals / idx depend on q[i, :E], g[:N, :E], K and idx_base only: not on the other queries, on i's position in the call, on
 *             n_split, on the previous contents of `workspace`, and on K only as a prefix (the result for K' < K is the first K' columns of the result for K).
 *             No global atomics; LDS counters only hand out candidate slots, and the list is always rebuilt by rank in the total order above.
 *   splits    as sc_search_topk: n_split ranges of ceil(N / n_split) rows, one block per (query tile, range), partial K-lists in `workspace`
 *             (12 Q n_split K bytes, none for one split), joined by sc_topk_merge; n_split = 0: sc_search_splits(Q, N, K).
 *   reads     rows [0, Q) of q and [0, N) of g, E elements of each; nothing else.
 *   refused   (nonzero rc + sc_last_error, nothing launched) E % 16 != 0 or E outside [16, 1024] (multiples of 16 only: no zero-filled k-slot ever enters a
 *             sum); ld_q / ld_g < E or not multiples of 8; q or g not 16-byte aligned; K outside [1, 128]; K > N; N >= 2^31; n_split outside [0, 1024];
 *             Q < 0; a null operand; no workspace with more than one split.  Q == 0 returns 0 and launches nothing. */
int sc_search_topk_bf16(const void* q, int64_t ld_q, const void* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split,
                        int64_t idx_base, float* vals, int64_t* idx, void* workspace, void* stream);

/* ---- Gallery search by item: the K nearest DISTINCT items of every query row, the query's own item left out (csrc/search_items.hip).  A gallery is rarely
 * one row per thing (five spoken captions per image): g_item gives every gallery row an item code, and the selection of sc_search_topk /
 * sc_search_topk_bf16 gets a predicate and a tie rule -- no new score.  sc_search_items takes fp32 rows, sc_search_items_bf16 bf16 rows; scores, strides,
 * alignment, the rules for E, K in [1, 128], n_split, idx_base and N < 2^31 are exactly those of sc_search_topk and sc_search_topk_bf16 respectively.
 * SELECTION CONTRACT (restated on the host in tests/search_items_ref.py):
 *   score      the plain entry's s(i, j) of the same format, bit for bit: fp32 rows the ascending fmaf chain of sc_search_topk, bf16 rows the contract of
 *              sc_search_topk_bf16 (the same loading, staging and MFMA code is compiled into both).
 *   eligible   eligible(i, j) means: s(i, j) is not NaN and (q_skip == NULL or q_skip[i] < 0 or g_item[j] != q_skip[i]).  g_item is int32 [N] with codes
 *              >= 0 and is required (non-null); q_skip is int32 [Q] or NULL.
 *   order      pairs (s(i, j), j) are ordered by score descending, then j ascending, as before.
 *   result     distinct == 0: the first K eligible pairs of query i in that order.  distinct != 0: the REPRESENTATIVE of an item code c is the first eligible
 *              pair, in that order, among the rows with g_item[j] == c; the result is the first K representatives in that order.
 *   outputs    vals f32 [Q, K] = the scores, idx i64 [Q, K] = idx_base + j, items i32 [Q, K] = g_item[j].  Missing slots hold -inf / -1 / -1.
 *   prefix     in both modes the result for K' < K is the first K' columns of the result for K.
 *   identities with distinct == 0 and q_skip == NULL, vals and idx equal the plain entry's bit for bit; the same holds with distinct != 0 when all codes in
 *              g_item are different.
 *   pure       as the plain entries: the bits of row i depend on q[i, :E], g[:N, :E], g_item[:N], q_skip[i], distinct, K and idx_base only -- not on the other
 *              queries, on i's position in the call, on n_split or on the previous contents of `workspace`.  No global atomics; LDS counters only hand out
 *              candidate slots; the list is rebuilt by rank among the entries that no entry of the same item code precedes.
 *   splits     the same ranges and auto rule (sc_search_splits).  Each block writes its K-list as (idx i64, vals f32, items i32) to `workspace`
 *              ([Q][n_split][K] of each, in that order: sc_search_items_workspace_bytes = 16 Q n_split K bytes, 0 for one split, which writes the outputs
 *              directly) and sc_topk_merge_items joins them.  Joining per-split lists is exact also with `distinct`: an item's representative over the
 *              whole gallery is its representative inside its split, and if it is missing from that split's K-list, K other items have representatives
 *              before it there -- and those, or better ones, come before it over the whole gallery, so the item is not among the first K.
 *   reads      rows [0, Q) of q and [0, N) of g, E elements of each; g_item[0 .. N); q_skip[0 .. Q) if given; nothing else.
 *   refused    (nonzero rc + sc_last_error naming the value, nothing launched) every refusal of the plain entry of the same format, a null g_item and a null
 *              items.  Q == 0 returns 0 and launches nothing.
 * sc_topk_merge_items: row r of vals_in f32 [Q, L] / idx_in i64 [Q, L] / items_in i32 [Q, L] holds L candidates in any order.  Entries with idx < 0 or a
 *   NaN value take no part.  distinct == 0: sc_topk_merge with the item codes carried along.  distinct != 0: only the first pair of each item code, in (value
 *   descending, idx ascending) order, survives; then the first K of the survivors; L <= 131072 (one bit per candidate in LDS).  Missing slots hold
 *   -inf / -1 / -1.  1 <= K <= 128, K <= L; outputs must not alias inputs. */
int64_t sc_search_items_workspace_bytes(int Q, int64_t N, int K, int n_split);
int sc_search_items(const float* q, int64_t ld_q, const float* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base,
                    const int32_t* g_item, const int32_t* q_skip, int distinct, float* vals, int64_t* idx, int32_t* items, void* workspace, void* stream);
int sc_search_items_bf16(const void* q, int64_t ld_q, const void* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base,
                         const int32_t* g_item, const int32_t* q_skip, int distinct, float* vals, int64_t* idx, int32_t* items, void* workspace, void* stream);
int sc_topk_merge_items(const float* vals_in, const int64_t* idx_in, const int32_t* items_in, int Q, int L, int K, int distinct, float* vals, int64_t* idx,
                        int32_t* items, void* stream);

/* ---- Gallery search by subset: sc_search_items / sc_search_items_bf16 inside a part of the gallery (csrc/search_select.hip) -- one split of an index that
 * holds several, one language, or for every query the rows of its own class.  Two conjuncts join eligible(i, j), inside the fused kernel and BEFORE the
 * top-K filter, and the scan skips the gallery tiles that nobody selected.  sc_search_select takes fp32 rows, sc_search_select_bf16 bf16 rows.  Everything
 * not named here is sc_search_items / sc_search_items_bf16 of the same format: scores bit for bit, order, distinct, q_skip, the outputs and their missing
 * slots (-inf / -1 / -1), strides, alignment, the rules for E, K, N and n_split, sc_search_splits, sc_search_items_workspace_bytes, the merge by
 * sc_topk_merge_items, and every refusal.  SUBSET CONTRACT (restated on the host in tests/search_select_ref.py):
 *   eligible   eligible(i, j) of sc_search_items, and allowed(j), and grouped(i, j).
 *   row mask   allowed(j) means: g_allow == NULL, or bit (j & 31) of g_allow[j >> 5] is set.  j is the row number inside this call (0 .. N-1), not
 *              idx_base + j.  Bits at j >= N are ignored, whatever they hold; ceil(N / 32) words are read and nothing beyond them.
 *   group      grouped(i, j) means: q_group == NULL, or q_group[i] < 0, or g_group[j] == q_group[i].  g_group is int32 [N] with codes >= 0, q_group int32
 *              [Q]; both are given or neither.
 *   identity   with g_allow, g_group and q_group all NULL the result equals sc_search_items[_bf16] bit for bit.
 *   few rows   a query with fewer than K eligible rows gets missing slots; that is not an error.
 *   dead tiles a block's range is cut into tiles of 128 rows from the range's first row; a tile none of whose rows inside the range is allowed is DEAD: the
 *              block issues no global loads of its g rows, no LDS stage and no MFMA for it, and prefetches the next LIVE tile's first chunk during the
 *              current multiply.  Ranges are ceil(N / n_split) rows and in general neither word- nor tile-aligned: the first and last word of a tile are
 *              masked to its rows.  Without g_allow every tile is live; groups skip nothing.  A block whose whole range is dead still writes its empty
 *              K-list to the workspace.  The rows of dead tiles and the rows that are not eligible may hold anything (NaN, +-inf): the result does not change.
 *   pure       as sc_search_items, with g_allow[0 .. ceil(N / 32)), g_group[:N] and q_group[i] added to what row i depends on.  No global atomics; the walk
 *              over the live tiles is wave-uniform arithmetic on the mask words (a ballot over 64 tiles), the same in every wave of the block.
 *   reads      what sc_search_items reads, except the g rows of dead tiles; g_allow[0 .. ceil(N / 32)), g_group[0 .. N) and q_group[0 .. Q) if given.
 *   refused    (nonzero rc + sc_last_error naming the value, nothing launched) every refusal of sc_search_items[_bf16], and g_group without q_group or
 *              q_group without g_group.  Q == 0 returns 0 and launches nothing.
 * sc_pack_row_mask: mask uint8 [N] -> words uint32 [ceil(N / 32)]: words[j >> 5] bit (j & 31) = mask[j] != 0; the unused high bits of the last word are
 *   written as 0; every word is written once.  N must be in [0, 2^31); N == 0 returns 0 and launches nothing; a null operand is refused. */
int sc_search_select(const float* q, int64_t ld_q, const float* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base,
                     const uint32_t* g_allow, const int32_t* g_group, const int32_t* q_group, const int32_t* g_item, const int32_t* q_skip, int distinct,
                     float* vals, int64_t* idx, int32_t* items, void* workspace, void* stream);
int sc_search_select_bf16(const void* q, int64_t ld_q, const void* g, int64_t ld_g, int Q, int64_t N, int E, int K, int n_split, int64_t idx_base,
                          const uint32_t* g_allow, const int32_t* g_group, const int32_t* q_group, const int32_t* g_item, const int32_t* q_skip, int distinct,
                          float* vals, int64_t* idx, int32_t* items, void* workspace, void* stream);
int sc_pack_row_mask(const uint8_t* mask, int64_t N, uint32_t* words, void* stream);

/* ---- Gallery search, fp32 re-score of a shortlist: the second stage of a two-stage search (csrc/search_rescore.hip).  A bf16 search (sc_search_topk_bf16 /
 * sc_search_items_bf16 on the rounded rows) shortlists R >= K rows per query; this entry scores those rows on the fp32 rows, returns the first K of them and
 * says per query whether an error bound given by the caller PROVES that the first K of the shortlist are the first K of the whole gallery.
 * q f32 [Q, E] / g f32 [N, E] with row strides ld_q / ld_g (elements); cand_idx i64 [Q, R]: the shortlist as the first stage wrote it (idx_base + j, or -1
 * for an empty slot); short_vals f32 [Q, R]: that stage's scores, descending; eps f32 [Q].  RESCORE CONTRACT (restated on the host, with the derivation of
 * eps, in tests/search_rerank_ref.py):
 *   score      for every slot with cand_idx != -1 and 0 <= cand_idx - idx_base < N, j = cand_idx - idx_base and s(i, j) = the fp32 chain of sc_search_topk:
 *              acc = +0.0f; for e ascending: acc = fmaf(q[i*ld_q + e], g[j*ld_g + e], acc) -- one accumulator, never split or reordered, subnormals kept:
 *              the bits of sc_search_topk's score of the same pair.  Any other slot is never dereferenced and takes no part.
 *   order      score descending, then j ascending; a NaN score takes no part.
 *   result     vals f32 [Q, K] / idx i64 [Q, K] (= idx_base + j): the first K slots of row i in that order; missing slots hold -inf / -1.  The slots of one
 *              row are expected to name distinct rows.
 *   certified  int32 [Q]: certified[i] = 1 iff all R slots of row i name a row in range, short_vals[i, R-1] is not NaN, and either R == N or
 *              (double)vals[i, K-1] > (double)short_vals[i, R-1] + (double)eps[i] (strict, in fp64); else 0.  What it proves: if every first-stage score is
 *              within eps[i] of the fp32 chain of the same pair, a row outside the shortlist has a first-stage score <= short_vals[i, R-1], hence a chain
 *              score <= short_vals[i, R-1] + eps[i] < vals[i, K-1]: it comes after the K returned rows, ties included.
 *   pure       row i of vals / idx / certified depends on row i of q, cand_idx, short_vals and eps, on g, K, R, N and idx_base only: not on i's position in
 *              the call and not on the other queries.  No atomics; every output element is written once.
 *   reads      rows [0, Q) of q, cand_idx, short_vals and eps; E elements of the rows of g that an in-range slot names; nothing else.
 *   refused    (nonzero rc + sc_last_error, nothing launched) E % 4 != 0 or E outside [4, 1024]; ld_q / ld_g < E or not multiples of 4; q or g not 16-byte
 *              aligned; K outside [1, 128]; R outside [K, 128]; N outside [1, 2^31); Q < 0; a null operand.  Q == 0 returns 0 and launches nothing. */
int sc_search_rescore(const float* q, int64_t ld_q, const float* g, int64_t ld_g, int Q, int64_t N, int E, const int64_t* cand_idx, const float* short_vals,
                      int R, const float* eps, int K, int64_t idx_base, float* vals, int64_t* idx, int32_t* certified, void* stream);

/* ---- Gallery search by threshold: every gallery row whose score reaches the query's threshold (csrc/search_range.hip) -- the other question a vector index
 * is asked, answered like sc_search_topk without a [Q, N] score image.  The number of hits is not known beforehand, so there are TWO PASSES over the same
 * scores: sc_search_range_count[_bf16] counts the hits of every (query, gallery range), the caller turns the counts into offsets with an exclusive scan (and
 * learns the total T), and sc_search_range_fill[_bf16] recomputes the scores and writes every hit to its place.  The plain entries take fp32 rows, the _bf16
 * entries bf16 rows; operands, strides, alignment and the rules for E are those of sc_search_topk and sc_search_topk_bf16 respectively.  thresh is f32 [Q].
 * RANGE CONTRACT (restated on the host in tests/search_range_ref.py):
 *   score     the plain entry's s(i, j) of the same format in every bit: fp32 rows the ascending fmaf chain of sc_search_topk on v_mfma_f32_32x32x2_f32,
 *             bf16 rows the contract of sc_search_topk_bf16 (the same loading, staging and MFMA code is compiled into all of them; one accumulator per
 *             (i, j), E never split).
 *   hit       pair (i, j) is a hit iff s(i, j) >= thresh[i], compared in fp32, and the row is eligible.  A NaN score or a NaN threshold hits nothing;
 *             thresh[i] = -inf hits every row whose score is not NaN; +inf hits only a score of +inf.
 *   eligible  q_skip == NULL, or q_skip[i] < 0, or g_item[j] != q_skip[i] (g_item int32 [N], q_skip int32 [Q], as sc_search_items).  With a null q_skip
 *             nothing reads g_item, which may then be null.  There is no `distinct` mode.
 *   ranges    those of sc_search_topk: n_split ranges of ceil(N / n_split) rows, trailing ranges may be empty, one block per (query tile, range);
 *             n_split = 0: sc_search_splits(Q, N, 1).  A query tile is 128 rows when Q > 64, else 64 (no list in LDS to make room for).
 *   count     counts[i*ld_counts + s] (int32) = the number of hits of query i among the rows of range s, for every i in [0, Q) and s in [0, n_split); no
 *             other element of `counts` is written, so with ld_counts > n_split several calls (the segments of an index) share one table, each writing
 *             its own band of columns.
 *   fill      the hits of (i, s), in ASCENDING j, go to vals[o] = s(i, j) / idx[o] = idx_base + j for o = offs[i*ld_offs + s] (int64), o + 1, ...  The
 *             fill pass assumes nothing about the count pass except that the caller derived `offs` from its counts with the same operands and n_split:
 *             with the exclusive scan over (i, s) in row-major order, query i's hits lie at [offs[i, 0], offs[i + 1, 0]) in ascending j.  Exactly
 *             count(i, s) elements are written per (i, s); nothing else of vals / idx is touched.
 *   pure      the hits of query i, their bits and their order depend on q[i, :E], g[:N, :E], thresh[i], the skip code and idx_base only: not on the other
 *             queries, on n_split, on i's position in the call, or on what the outputs held before.  NO ATOMICS, global or LDS: a hit's place follows
 *             from 64-bit ballots of the hit predicate (two query rows x 32 gallery columns per ballot) and their popcounts, a per-tile table of the four
 *             column groups' counts per row in LDS, and a per-row running position.
 *   reads     rows [0, Q) of q and [0, N) of g, E elements of each; thresh[0 .. Q); with q_skip: q_skip[0 .. Q) and g_item[0 .. N); fill: offs[i, s].
 *   refused   (nonzero rc + sc_last_error naming the value, nothing launched) the E, ld_q / ld_g, alignment, N >= 2^31, n_split and Q < 0 rules of the
 *             top-K entry of the same format; ld_counts / ld_offs below the split count; a null q, g, counts (count), offs, vals or idx (fill); a null
 *             thresh; a non-null q_skip with a null g_item.  Q == 0 returns 0 and launches nothing.  (A caller whose total is 0 has nothing to fill and
 *             does not call the fill pass.) */
int sc_search_range_count(const float* q, int64_t ld_q, const float* g, int64_t ld_g, int Q, int64_t N, int E, const float* thresh, int n_split,
                          const int32_t* g_item, const int32_t* q_skip, int32_t* counts, int64_t ld_counts, void* stream);
int sc_search_range_fill(const float* q, int64_t ld_q, const float* g, int64_t ld_g, int Q, int64_t N, int E, const float* thresh, int n_split,
                         const int32_t* g_item, const int32_t* q_skip, int64_t idx_base, const int64_t* offs, int64_t ld_offs, float* vals, int64_t* idx,
                         void* stream);
int sc_search_range_count_bf16(const void* q, int64_t ld_q, const void* g, int64_t ld_g, int Q, int64_t N, int E, const float* thresh, int n_split,
                               const int32_t* g_item, const int32_t* q_skip, int32_t* counts, int64_t ld_counts, void* stream);
int sc_search_range_fill_bf16(const void* q, int64_t ld_q, const void* g, int64_t ld_g, int Q, int64_t N, int E, const float* thresh, int n_split,
                              const int32_t* g_item, const int32_t* q_skip, int64_t idx_base, const int64_t* offs, int64_t ld_offs, float* vals, int64_t* idx,
                              void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SPEECHCLIP_HIP_H */
