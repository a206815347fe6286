/* C ABI of the MI355X-native image->LaTeX hot path (liblxo.so).
 *
 * The reference (LinXueyuanStdio/LaTeX_OCR) has no FFI: its numeric boundary is
 * `sess.run` inside model/img2seq.py (:169, :236, :263).  These entry points
 * are what a binding for that boundary calls; each cites the reference code it
 * replaces.  All pointers are DEVICE pointers owned by the caller, all calls
 * are asynchronous on the given hipStream_t (passed as void*), none allocates.
 * Return value: 0 = OK, negative = error (see lxo_last_error()).
 */
#ifndef LXO_H
#define LXO_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* liblxo.so is built with -fvisibility=hidden: what this header (and include/lxo_debug.h, the measurement hooks) declares is the
 * library's whole dynamic symbol table (tests/test_abi.py compares `nm -D` with the two headers) */
#pragma GCC visibility push(default)

#define LXO_F32 0
#define LXO_BF16 1

const char* lxo_last_error(void);
/* ABI version of this header.  Bumped whenever lxo_shape grows or an entry point changes (round 4: 4 -- lxo_comm_*,
 * lxo_allreduce_bucket, LXO_GNORM_FLOATS behind lxo_global_norm_scale's scale_out; round 5: 5 -- lxo_shape.deterministic,
 * lxo_chain_guard, lxo_decode_state_get / _set, lxo_decode_cell_step; a NaN *scale_dev drops an optimizer step; round 6: 6 --
 * lxo_beam_decode_attn, lxo_shape.live_B; the lxo_decoder_train_*_active calls are gone: they ran the launch-per-step kernels and were slower than the persistent chains computing every padded step).  A binding must check
 * lxo_version() == LXO_ABI_VERSION and lxo_shape_size() == sizeof(its own lxo_shape) before the first call: a caller built
 * against an older header passes a shorter struct and the library would read past its end. */
#define LXO_ABI_VERSION 6
int lxo_version(void);
int lxo_shape_size(void);

/* ---- building blocks (exposed for parity tests and for bindings that want
 *      the encoder / projections alone) ---- */

/* C[M,N] = act(alpha * A[M,K] * Bp[N,K]^T + bias) ; Bp is the K-contiguous
 * ("transposed", TF [in,out] -> [out,in]) weight copy in the compute dtype.
 * dt: compute dtype; a_f32/c_f32: A / C are float even when dt == LXO_BF16.
 * Replaces tf.layers.dense / tf.matmul call sites (attention_mechanism.py:43,79;
 * attention_cell.py:82-84).
 * Operand contract (the kernels load whole 16-byte pieces of a row and do not check):
 *  - K > 0 and K % 32 == 0 (else -2); M <= 0 or N <= 0 is an empty call (0, nothing written).
 *  - every row of A and Bp starts on a 16-byte boundary: A and Bp 16-byte aligned, lda % 8 == 0 and ldb % 8 == 0 (% 4 where
 *    the row is float); lda, ldb >= K.  Only columns 0..K of rows 0..M (0..N) are read.
 *  - C [M][ldc] in the compute dtype (float with c_f32), ldc >= N, no alignment; only columns 0..N of rows 0..M are written.
 *    accumulate != 0 adds the previous C (read in C's own type) to the result; it is defined for act == 0.
 *  - small != 0 (the recurrent steps' M <= 64 shapes): with dt == LXO_BF16 it takes float A and float C only (else -3);
 *    K % 256 == 0 and lda % 4 == 0 select the split-K skinny kernel, whose float A rows need 16-byte alignment only. */
int lxo_gemm_nt(int dt, int a_f32, int c_f32, int small, const void* A, const void* Bp, void* C,
                int M, int N, int K, int lda, int ldb, int ldc, const float* bias, int act,
                float alpha, int accumulate, void* stream);

/* C[I,J] += sum_m A[m,I] * B[m,J] (f32 output, atomics across nsplit row ranges).
 * Operand contract:
 *  - atomic != 0 adds into C; atomic == 0 stores the product over C and needs nsplit == 1 (else -2).  dt == LXO_F32 always uses one
 *    row range (a reproducible sum), whatever nsplit says.  I, J or M <= 0 is an empty call (0, nothing written).
 *  - the kernels read whole 8-column chunks of a row: lda >= round8(I) and ldb >= round8(J) (round8(x) = (x + 7) / 8 * 8), and the
 *    columns I..round8(I) of A and J..round8(J) of B must be readable memory; their values never reach C.
 *  - every row of A and B starts on a 16-byte boundary: A and B 16-byte aligned, lda % 8 == 0 and ldb % 8 == 0 (% 4 where the operand
 *    is float).  Only rows 0..M are read; C [I][ldc] float, ldc >= J, only columns 0..J of rows 0..I are written. */
int lxo_gemm_tn(int dt, int a_f32, int b_f32, const void* A, const void* B, float* C,
                int M, int I, int J, int lda, int ldb, int ldc, int nsplit, int atomic, void* stream);

/* split-K partial products of a skinny GEMM (the recurrent steps): slab[ks][M][ldc] = A[:, ks*128:+128] *
 * Bp[:, same]^T for ks < K/128, A float [M][lda], Bp compute dtype [N][ldb]; the consumer adds the slabs.
 * Operand contract: K > 0, K % 128 == 0 and lda % 4 == 0 (else -2); M <= 0 or N <= 0 is an empty call (0, nothing written); rows of
 * A and Bp on 16-byte boundaries (A, Bp 16-byte aligned, ldb % 8 == 0, % 4 for float Bp); slab_stride >= M * ldc, ldc >= N; only
 * columns 0..N of rows 0..M of each slab are written (plain stores over whatever was there). */
int lxo_gemm_slab(int dt, const void* A, const void* Bp, float* slab, int M, int N, int K, int lda, int ldb, int ldc,
                  long long slab_stride, void* stream);

/* 3x3 stride-1 convolution as an implicit GEMM on the MFMA units (the tf.layers.conv2d call
 * sites model/encoder.py:37-59): out[B,Ho,Wo,Cout] = act(conv(in[B,H,W,Cin]) + bias), NHWC,
 * in/out/wpk in the compute dtype, wpk = [Cout][9*Cin] (tap-major, channel-minor).
 * pad 1 + Ho=H,Wo=W is SAME; pad 0 + Ho=H-2,Wo=W-2 is VALID; pad 2 + Ho=H+2,Wo=W+2 is the
 * dgrad of a VALID layer.  Cin % 64 == 0 (bf16) / % 32 (f32). */
int lxo_conv3x3(int dt, const void* in, const void* wpk, const float* bias, void* out, int B, int H, int W,
                int Cin, int Ho, int Wo, int Cout, int pad, int relu, void* stream);

/* lxo_conv3x3 with the rest of the fused epilogue the encoder uses: out_pre (optional) receives
 * act(conv + bias) before `addend` (f32 [addend_rows][Cout], row = pixel index % addend_rows: the timing signal of
 * positional.py:10-65 fused into conv6) is added; relu_ref (optional, same shape as out) zeroes out where the
 * reference activation is <= 0 (the ReLU backward of the producing layer when this call is a dgrad) and
 * colsum (optional, f32 [Cout], accumulated) receives the column sums of the result (that layer's bias gradient). */
int lxo_conv3x3_ex(int dt, const void* in, const void* wpk, const float* bias, void* out, int B, int H, int W,
                   int Cin, int Ho, int Wo, int Cout, int pad, int relu, const float* addend, int addend_rows,
                   void* out_pre, const void* relu_ref, float* colsum, void* stream);

/* weight gradient of lxo_conv3x3: dw[9*Cin][Cout] (f32, HWIO flattened) += sum_pixels in (x) dout.
 * What TF autodiff derives for the tf.layers.conv2d kernels (model/img2seq.py:119-123). */
int lxo_conv3x3_wgrad(int dt, const void* in, const void* dout, float* dw, int B, int H, int W,
                      int Cin, int Ho, int Wo, int Cout, int pad, void* stream);

/* AttentionMechanism.context (model/components/attention_mechanism.py:46-94) for nv decoder rows:
 * alpha = softmax_r(sum_k beta_k tanh(att_img[r,k] + att_h[k])), ctx = sum_r alpha_r img[r,:].
 * att_img [nimg,R,E], img [nimg,R,C] compute dtype; row v uses image v / beam; alpha f32 [nv,Rp],
 * Rp = (R+7)/8*8; ctx f32 [nv, ldctx]; part = scratch of nv*32*(C+2) floats. */
int lxo_attention_fwd(int dt, const void* att_img, const void* img, const float* att_h, const float* beta,
                      float* alpha, float* part, float* ctx, int ldctx, int nv, int R, int E, int C, int beam,
                      void* stream);

/* Measurement aid (off by default, per host thread): with timing enabled every implicit-GEMM conv launch (forward,
 * data gradient, weight gradient) and every attention launch of the lxo_encoder_* / lxo_decoder_train_* calls is
 * bracketed by HIP events on the stream it is launched on, so that bench.py's roofline comes from kernel durations
 * INSIDE a real training step.  lxo_timing_enable(1) clears the records; lxo_timing_get synchronises record i and returns
 * its family ("conv_fwd", "conv_dgrad", "conv_wgrad", "attn_fwd", "attn_bwd"), name, algorithmic work (FLOPs or bytes)
 * and duration in milliseconds. */
int lxo_timing_enable(int on);
int lxo_timing_count(void);
int lxo_timing_get(int i, const char** family, const char** name, double* work, float* ms);

/* ---- the hot path proper ---- */

/* Shape of one call.  H, W are the batch-max image extents after white padding
 * (model/utils/image.py:27-44); T is the padded formula width Lmax+1
 * (model/utils/text.py:157-162); V is Vocab.n_tok (text.py:16); C/E/U/O/D are the
 * encoder width (512) and attn_cell_config {dim_e, num_units, dim_o, dim_embeddings}
 * (configs/model.json:6-12). */
typedef struct lxo_shape {
    int B, H, W, T, V;
    int C, E, U, O, D;
    int dtype;      /* LXO_F32 (parity mode) or LXO_BF16 (bf16 storage, f32 accumulate) */
    int beam;       /* decode only: beam width the workspace is sized for (>= 1); beam decode takes 2 .. min(16, V) (lxo_beam_decode and
                     * lxo_decode_begin refuse a wider beam: at time 0 only V candidates exist) */
    int max_steps;  /* decode only: step capacity (max_length_formula + 2) */
    /* training only: tf.nn.dropout keep probability on h and o (attention_cell.py:72,83; config.dropout,
     * fed at img2seq.py:166) and the seed of this step's counter-based masks; 0 or >= 1 disables */
    float keep_prob;
    int dropout_seed;
    /* beam decode only: add_div_penalty (beam_search_decoder_cell.py:258-287; configs/model.json:15-16).
     * div_gamma 0 or 1, or div_prob 0, disables; div_seed keys the Bernoulli(div_prob) draws */
    float div_gamma, div_prob;
    int div_seed;
    /* encoder variants of configs/model.json: encoder_cnn 0 = "vanilla" (pools after conv4 / conv5,
     * encoder.py:46-52), 1 = "cnn" (no pools, a (2,4) stride-2 SAME conv after conv5, encoder.py:54-56);
     * no_positional != 0 = positional_embeddings false (encoder.py:60-65 skipped) */
    int encoder_cnn;
    int no_positional;
    /* decoder step decomposition: 0 (default) = automatic: the teacher-forced recurrence of lxo_decoder_train_fwd as ONE persistent launch
     * of 8 XCD-local chains (csrc/xdec.hip) where the shape qualifies (bf16, the shipped widths U = O = C = 512, E = 256, B in
     * {8, 16, 32, 64}, an MI355X), else the fused step kernels; 2 = always the fused step kernels (full-K workgroups with the cell's
     * point-wise stages in the GEMM epilogues, csrc/rstep.hip: 9 dependent launches per training step pair); 1 = the split-K slab
     * GEMMs + separate point-wise kernels of round 1 (13 launches; also what the side-stream interleave uses) */
    int step_kernels;
    /* optional row encoder between the CNN and the decoder (north_star's "row-BiLSTM encoder"; ABSENT from the reference, whose
     * encoder.py:4 imports GRUCell / LSTMCell and never uses them -- off by default, outside the parity contract): 1 = every
     * row of the H' x W' feature map is run through a bidirectional TF-style LSTMCell (C/2 units per direction, zero initial
     * state) along W'; the concatenated outputs replace the features the attention reads.  Needs C in {256, 512}. */
    int encoder_rnn;
    /* bf16 mode only (the f32 parity mode is always run-to-run reproducible): != 0 = every reduction of the training step runs in a
     * fixed order -- the float atomics of the bf16 epilogues (conv weight gradients, the deferred all-step weight gradients, bias
     * sums, d_beta, the embedding scatter, the loss statistics) go through ordered partial slots (ws region "det_part") -- so that
     * two runs of one binary on the same inputs give bit-identical losses, gradients and weights.  Costs a few per cent of a step
     * (bench.py: secondary.deterministic_bf16); off by default.  SURVEY.md Appendix D step 8. */
    int deterministic;
    /* training only: 0 (or B) = every batch row is a sample.  0 < live_B < B: rows live_B .. B - 1 are DEAD PADDING ROWS -- a batch the
     * persistent chains do not take (the reference trains at 3, buckets and evaluates at 20: configs/training.json:6, data_generator.py:41,
     * evaluate_txt.py:42) filled up to a chain batch of 8 / 16 / 32 / 64.  The caller gives them any valid token ids and formula
     * length 0 (so no token of theirs is inside the loss mask, img2seq.py:68-71: their d(logits) and every gradient contribution is an
     * exact zero, n_words does not see them); `img` needs only live_B images.  The encoder computes the live images only (the dead
     * rows' features are zeros), the decoder steps all B rows.  Ignored with encoder_rnn. */
    int live_B;
} lxo_shape;

/* flat f32 parameter / gradient / Adam-slot buffers: variable inventory in TF
 * checkpoint order.  id in [0, lxo_param_num()). */
int lxo_param_num(void);
const char* lxo_param_name(int id);
/* the TF variable name of slot id for this shape's encoder variant (the tf.layers.conv2d scopes are numbered in
 * creation order, so "cnn" renames the last two convs); slots with count 0 in lxo_param_info are absent */
const char* lxo_param_name_for(const lxo_shape* s, int id);
long long lxo_param_total(const lxo_shape* s);
int lxo_param_info(const lxo_shape* s, int id, long long* offset, long long* count);

size_t lxo_wpack_bytes(const lxo_shape* s);
size_t lxo_workspace_bytes(const lxo_shape* s);
/* offset/size of a named workspace region (tests and bindings read activations,
 * logits, loss statistics and attention weights through this) */
int lxo_ws_region(const lxo_shape* s, const char* name, size_t* offset, size_t* bytes);
/* element type of a workspace region for this shape: LXO_F32, LXO_BF16, LXO_I32 or LXO_U8 (negative: unknown name).
 * Matters for "d_img", the hand-over between lxo_decoder_train_bwd and lxo_encoder_bwd: f32 mode = the f32 gradient w.r.t. the
 * encoder output; bf16 mode = d_y6, that gradient with conv6's ReLU mask already applied, stored as bf16 (and conv6's bias
 * gradient already accumulated) -- a caller that drives lxo_encoder_bwd on its own must write the region in THAT form. */
#define LXO_I32 2
#define LXO_U8 3
int lxo_ws_region_dtype(const lxo_shape* s, const char* name);

/* refresh the compute-dtype GEMM operand copies from the f32 master parameters
 * (call after every optimizer step / checkpoint load) */
int lxo_pack_weights(const lxo_shape* s, const float* params, void* wpack, void* stream);

/* Encoder.__call__ (model/encoder.py:17-68) + add_timing_signal_nd
 * (model/components/positional.py:10-65): u8 [B,H,W,1] -> ws region "img" [B,R,C] */
int lxo_encoder_fwd(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                    const uint8_t* img, void* stream);
/* backward of conv layers last_layer..first_layer (6..1), accumulating into grads;
 * layer 6 consumes ws region "d_img" (f32 mode: the f32 gradient w.r.t. the encoder output; bf16 mode: d_y6, i.e. that
 * gradient with conv6's ReLU mask applied, in bf16 -- the decoder's last GEMM applies the mask and sums conv6's bias
 * gradient in its epilogue, see lxo_decoder_train_bwd).  Split so a data-parallel caller can
 * all-reduce finished buckets while earlier layers still run. */
int lxo_encoder_bwd(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                    const uint8_t* img, float* grads, int last_layer, int first_layer, void* stream);
/* The same range in ONE call, for a data-parallel caller that does not want the compute stream to stop at every bucket:
 * ready_events[l] (l = 1..6; a table of 7 hipEvent_t created by the caller, NULL entries skipped) is recorded as soon as layer l's
 * weight and bias gradients are final -- on the weight-gradient side stream when one is bound (lxo_set_encoder_side_stream), else on
 * `stream` -- so a communication stream can wait for a layer's event and reduce its bucket while the earlier layers, and the
 * weight gradients beside them, still run.  Returns like lxo_encoder_bwd: `stream` ordered after the whole range. */
int lxo_encoder_bwd_ready(const lxo_shape* s, const float* params, const void* wpack, void* ws, const uint8_t* img, float* grads,
                          int last_layer, int first_layer, void* const* ready_events, void* stream);
/* The whole backward pass of a training step in one call: lxo_decoder_train_bwd followed by lxo_encoder_bwd for layers 6..1 (the two
 * halves of what one sess.run(train_op) differentiates, img2seq.py:169), with the weight-gradient side stream -- when one is bound --
 * joined ONCE, at the end, instead of once per call: the decoder's deferred weight gradients then also run beside conv6's data
 * gradient.  ready_events (optional): as for lxo_encoder_bwd_ready, plus entry 0 = every decoder gradient final (incl. y_W_o and the
 * chain-failure probe element lxo_chain_guard reads).  `stream` is ordered after everything when the call returns. */
int lxo_train_bwd(const lxo_shape* s, const float* params, const void* wpack, void* ws, const int32_t* formula, const uint8_t* img,
                  float* grads, void* const* ready_events, void* stream);

/* Optional second HIP stream for the calling host thread (NULL disables).  When set, the recurrent
 * loops of lxo_decoder_train_fwd / _bwd run the two halves of the batch on `stream` and on this side
 * stream (fork/join by events), so the launch- and latency-bound step kernels of one half overlap the
 * other half's.  The only per-thread state the library keeps. */
int lxo_set_side_stream(void* stream);
/* Optional second HIP stream for the weight gradients of the calling host thread (NULL disables; bf16 mode only,
 * ignored while lxo_timing_enable(1) records).  lxo_encoder_bwd runs the conv weight-gradient
 * kernels on it, beside the data-gradient / pool-backward chain of the main stream (three rotating gradient buffers);
 * lxo_decoder_train_bwd runs its deferred all-step weight gradients (dense dW GEMMs, LSTM bias, embeddings, initial-state
 * parameters, dW_att_img) on it, beside the d_att_img -> d_img path.  Fork / join by events inside each call: every call
 * returns with `stream` ordered after all of its work on the side stream, so gradients are final in stream order as without
 * it, and no kernel of the side stream is in flight when a later call launches a persistent chain. */
int lxo_set_encoder_side_stream(void* stream);

/* Decoder.__call__ training branch (model/decoder.py:41-57): AttentionMechanism
 * set-up (attention_mechanism.py:19-43,124-153), T steps of AttentionCell.step
 * (attention_cell.py:58-89) under teacher forcing, logits for every step. */
int lxo_decoder_train_fwd(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                          const int32_t* formula, void* stream);
/* The same for a caller that knows the formula lengths (device int32 [B], the array the loss calls take; the dead rows that fill a batch up carry
 * length 0).  Where the persistent forward chain runs, a pair (t, b) with t >= lengths[b] is DEAD: its attention workgroups stream nothing.  What
 * a dead position then holds: ws region "alpha" row (t, b) and the ctx columns of its record (ws regions "rec" / "recb", slot t + 1) are exact
 * zeros; h, c, the gates, att_h, o and the logits are what the step computes from that zero context -- finite, and a function of this call's
 * inputs only, never of what the workspace held before.  The loss, lxo_score_tokens and lxo_train_bwd read a dead position only to multiply it
 * by an exact zero.  Every live position (t < lengths[b]) holds lxo_decoder_train_fwd's value bit for bit, whatever the other rows' lengths.
 * On every other path -- the launch-per-step kernels, f32, a shape the chain does not take -- and with lengths == NULL the call IS
 * lxo_decoder_train_fwd: every padded position is computed. */
int lxo_decoder_train_fwd_live(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                               const int32_t* formula, const int32_t* lengths, void* stream);
/* loss of model/img2seq.py:68-75 and d(loss)/d(logits).  inv_ntok = 1 / (number of
 * unmasked tokens in the GLOBAL batch).  ws region "loss" = {sum CE, token count}.  Target ids outside [0, V) are
 * clamped into it (< 0 -> 0, >= V -> V - 1), as lxo_score_tokens does; d(logits) is 0 in the padding columns [V, Vp). */
int lxo_ce_loss_fwd_bwd(const lxo_shape* s, void* ws, const int32_t* formula,
                        const int32_t* lengths, float inv_ntok, void* stream);
/* The same with the GLOBAL token count read from device memory (*ntok_dev, a float): under data parallelism the count is
 * the sum over ranks of host-known integers, all-reduced on a side stream while the forward runs, so no host
 * synchronisation sits between forward and backward (img2seq.py:69-71 takes the mean over all tokens of the batch). */
int lxo_ce_loss_fwd_bwd_dev(const lxo_shape* s, void* ws, const int32_t* formula,
                            const int32_t* lengths, const float* ntok_dev, void* stream);
/* The weighted loss: token (b, t) weighs w = w_tok[b][t] * w_row[b] (device f32 [B, T] / [B]; ONE f32 product, a NULL factor is 1; at least one of the
 * two is given, else -1).  d(logits)[t * B + b][j] = (softmax_j - [j == target]) * (w * inv_norm) for t < lengths[b] -- the scale is the single f32
 * product w * inv_norm -- and 0 for t >= lengths[b] and in the padding columns [V, Vp), as in lxo_ce_loss_fwd_bwd.  A weight may be negative (a
 * transcription to train AGAINST) or 0 (a live row of weight 0 gets zeros of either sign); weights are not checked for NaN.  norm_dev (nullable,
 * device f32 [1]): 1 / norm_dev[0] replaces inv_norm, as ntok_dev does in lxo_ce_loss_fwd_bwd_dev.
 * ws region "loss" = {sum w CE, live token count (whatever the weights), sum w, sum CE (unweighted)} over the live tokens; the forward chain's error
 * word turns [0] into NaN.  The four go through the ordered per-workgroup slots of ws region "det_part" in every mode.
 * With w_tok == 1 everywhere d(logits) and "loss"[0..1] are lxo_ce_loss_fwd_bwd's bit for bit; with w_row == c, d(logits) is the one it leaves
 * for inv_ntok = c * inv_norm (the f32 product).  The rest of the training step is linear in d(logits): lxo_train_bwd after this call leaves the
 * gradient of sum w CE * inv_norm. */
int lxo_ce_loss_weighted(const lxo_shape* s, void* ws, const int32_t* formula, const int32_t* lengths,
                         const float* w_tok, const float* w_row, float inv_norm, const float* norm_dev, void* stream);
/* The label-smoothed loss (TensorFlow's softmax_cross_entropy(label_smoothing=), torch's F.cross_entropy(label_smoothing=)): the target of a live row
 * (t < lengths[b]) with clamped target y is q_j = (1 - eps) [j == y] + eps / V over j in [0, V), and with lse the row's log-sum-exp, p its soft-max and
 * w = w_tok[b][t] * w_row[b] (both nullable here: a NULL factor is 1, both NULL is smoothing alone)
 *     CE = lse - x_y,   U = lse - (sum_{j < V} x_j) / V  (= -mean_j log p_j),   L = (1 - eps) * CE + eps * U,
 *     d(logits)[t * B + b][j] = (p_j - q_j) * (w * inv_norm) for j < V;   0 in the padding columns [V, Vp) and on rows t >= lengths[b].
 * In f32 on the device: eps_v = eps / (float)V is one division, the target column subtracts (1.f - eps) + eps_v and every other column eps_v -- with
 * eps == 0 that is p - 1 and p - 0, so d(logits) and all four statistics are lxo_ce_loss_weighted's bit for bit, and without weights d(logits) and
 * "loss"[0..1] are lxo_ce_loss_fwd_bwd's.  The logit sum runs over [0, V) only: what the padding columns hold is never read into a result.
 * norm_dev (nullable, device f32 [1]): 1 / norm_dev[0] replaces inv_norm, as in lxo_ce_loss_weighted.
 * ws region "loss" = {sum w L, live token count, sum w, sum CE (plain, unweighted)} over the live tokens -- [1] and [3] are the bytes lxo_ce_loss_weighted
 * leaves -- through the ordered per-workgroup slots of ws region "det_part" in every mode: the same bytes in every run.  The forward chain's error
 * word turns [0] into NaN.  The rest of the training step is linear in d(logits): lxo_train_bwd after this call leaves the gradient of sum w L * inv_norm.
 * -1, nothing written, the reason in lxo_last_error: eps not finite or outside [0, 1); a NULL ws, formula or lengths. */
int lxo_ce_loss_smoothed(const lxo_shape* s, void* ws, const int32_t* formula, const int32_t* lengths, float eps,
                         const float* w_tok, const float* w_row, float inv_norm, const float* norm_dev, void* stream);
/* Soft targets (knowledge distillation from a teacher's top-k per position): the target of a live row is a sparse distribution the caller supplies,
 * mixed into lxo_ce_loss_smoothed's.  soft_ids int32 [B, T, k] and soft_p f32 [B, T, k] on the device -- lxo_score_alternatives' layout, B the shape's --
 * with 1 <= k <= 16; the slots of row (b, t) are read only where t < lengths[b].  eps, w_tok, w_row, inv_norm and norm_dev are lxo_ce_loss_smoothed's,
 * lambda lies in [0, 1].  Per live row, with y the clamped target, lse the log-sum-exp, p the soft-max, U = lse - (sum_{j < V} x_j) / V and CE = lse - x_y:
 *     slot i counts iff 0 <= soft_ids[i] < V; its mass is m_i = soft_p[i] when it counts, else 0 (the device does not check masses);
 *     Sigma = sum_i m_i, added in ascending i in f32;   rest = max(0, 1 - Sigma), the mass the top-k leaves out, spread uniformly over [0, V);
 *     tau_j = sum_{i: ids_i == j} m_i + rest / V   (slots that name the same token add up, in ascending i);
 *     lambda_r = 0 when Sigma == 0 (no counting slot: the row has no teacher and is lxo_ce_loss_smoothed's row), else lambda;
 *     q_j = (1 - lambda_r) [(1 - eps) [j == y] + eps / V] + lambda_r tau_j;   S = sum_j q_j = (1 - lambda_r) + lambda_r (Sigma + rest)  (1 unless the masses exceed 1);
 *     L = (1 - lambda_r) [(1 - eps) CE + eps U] + lambda_r [sum_i m_i (lse - x_{ids_i}) + rest U]   (the cross-entropy of q against p: the KL divergence
 *         plus the teacher's entropy, a constant);
 *     d(logits)[t * B + b][j] = (S p_j - q_j) * (w * inv_norm) for j < V;   0 in [V, Vp) and on rows t >= lengths[b].
 * ws region "loss" = {sum w L, live token count, sum w, sum CE (plain, unweighted)} through the ordered slots of "det_part" in every mode: the same bytes in
 * every run; [1] and [3] are the bytes lxo_ce_loss_weighted leaves for the same weights.  The forward chain's error word turns [0] into NaN.
 * IDENTITIES: a row whose slots are all -1 carries lxo_ce_loss_smoothed's d(logits) bytes (with eps == 0: lxo_ce_loss_weighted's), and with every row
 * like that the four statistics are its bytes too; lambda == 0 IS the lxo_ce_loss_smoothed call.  A live row's sum_j d(logits)_j is 0 up to rounding.
 * -1, nothing written, the reason in lxo_last_error: a NULL ws, formula, lengths, soft_ids or soft_p; k outside 1 .. 16; eps not finite or outside
 * [0, 1); lambda not finite or outside [0, 1].
 * Not here: a temperature on the student's logits, renormalising the top-k instead of spreading the rest, a confidence penalty. */
int lxo_ce_loss_soft(const lxo_shape* s, void* ws, const int32_t* formula, const int32_t* lengths,
                     float eps, float lambda, int k, const int32_t* soft_ids, const float* soft_p,
                     const float* w_tok, const float* w_row, float inv_norm, const float* norm_dev, void* stream);
/* Minimum-risk weights on the device, shape-free: rows group_off[g] .. group_off[g + 1] - 1 (device int32 [G + 1], ascending, group_off[0] == 0,
 * group_off[G] <= rows) are the candidate transcriptions of image g, seq_logp their sequence log-probs (lxo_score_tokens' seq_out) and cost their costs
 * (device f32 [rows]).  Q_c = softmax_c(alpha * seq_logp_c) over the group (maximum subtracted), R_g = sum_c Q_c cost_c,
 * w_out[c] = alpha * Q_c * (R_g - cost_c) (f32 [rows], NOT NULL), q_out[c] = Q_c (nullable), risk_out[0] = sum_g R_g (nullable), added in ascending g.
 * THE IDENTITY: with CE_c = -seq_logp_c, d(sum_c Q_c cost_c) / d(CE_c) = w_c exactly, and sum_c w_c = 0 per group -- so lxo_ce_loss_weighted with
 * w_row = w_out, no token weights and inv_norm = 1 / G leaves the gradient of the mean expected cost.
 * Rows in [group_off[G], rows) (a chain batch's dead rows) get w = q = 0; a group may have any size >= 0, one candidate gives w = 0 exactly; G == 0
 * zeroes w_out[0 .. rows).  One wave per group, fixed-order reductions, expf in both dtype modes, no atomics: the same bytes in every run.  The
 * device clamps an offset into [0, rows].  -1: a NULL w_out, seq_logp, cost or group_off, G < 0, rows < 0, alpha not finite. */
int lxo_mrt_weights(const float* seq_logp, const float* cost, const int32_t* group_off, int G, int rows, float alpha,
                    float* w_out, float* q_out, float* risk_out, void* stream);
/* Batched Levenshtein distance over int32 token rows on the device, shape-free.  Pair p (0 <= p < pairs) compares hypothesis row p with reference
 * row ref_of[p] (device int32 [pairs]; NULL: row p / per_ref, per_ref >= 1), an index the device clamps into [0, G).
 * HYPOTHESES: row p starts at element (p / hyp_block) * hyp_block_stride + (p % hyp_block) * hyp_row_stride of `hyp` and its tokens lie hyp_tok_stride
 * elements apart, T of them.  Plain rows [pairs, T]: hyp_block 1, hyp_block_stride T, hyp_tok_stride 1.  The ids [B, max_steps, n] that
 * lxo_sample_decode writes are read in place with hyp_block n, hyp_block_stride max_steps * n, hyp_row_stride 1, hyp_tok_stride n, T = the steps run.
 * REFERENCES: ref int32 [G, ref_ld], 1 <= ref_ld <= LXO_EDIT_MAX_REF.
 * A side's sequence is its first len tokens -- hyp_len [pairs] / ref_len [G], device int32, clamped into the row; NULL: T / ref_ld -- cut at the
 * first id_end (truncate_end's rule; id_end < 0: no cut), so a reference in pad_batch_formulas' layout with its lengths is passed as it is.
 * dist_out int32 [pairs] (NOT NULL): insertions + deletions + substitutions, exact.  cost_out f32 [pairs] (nullable): (float)dist /
 * (float)max(reference tokens, 1), ONE correctly rounded f32 division -- for these integers bit for bit np.float32(dist / max(len, 1)).
 * One wave per pair, integer arithmetic only: the same bytes in every run.  The hypothesis side has no limit beyond T.
 * -1: a NULL hyp, ref or dist_out; pairs, T, G, a stride or hyp_block negative, hyp_block or per_ref < 1, G < 1 with pairs > 0; ref_ld outside
 * 1 .. LXO_EDIT_MAX_REF. */
#define LXO_EDIT_MAX_REF 1024
int lxo_edit_distance(const int32_t* hyp, int hyp_block, long long hyp_block_stride, long long hyp_row_stride, long long hyp_tok_stride, int T,
                      const int32_t* hyp_len, const int32_t* ref, int G, int ref_ld, const int32_t* ref_len, const int32_t* ref_of, int per_ref,
                      int pairs, int id_end, int32_t* dist_out, float* cost_out, void* stream);
/* The counts an evaluation's text metrics are made of -- BLEU-4's clipped n-gram matches and totals, the lengths, the Levenshtein distance and exact
 * match -- per pair and summed over the pairs, on the device, shape-free.  ADDRESSING, LENGTHS, THE END CUT AND THE CLAMPING of what the device holds
 * are lxo_edit_distance's, argument for argument: the ids [B, max_steps, n] of a sampled decode are read in place, references are taken in
 * pad_batch_formulas' layout.  Pair p has hypothesis h and reference r after the cut.
 * stats_out int32 [pairs][LXO_TEXT_STATS] (nullable), row p:
 *   [0 .. 3]  match_n, n = 1 .. 4: sum over the distinct n-grams g of h of min(count_h(g), count_r(g)) -- corpus BLEU's clipped matches with one reference.
 *   [4 .. 7]  total_n = max(1, |h| - n + 1) (nltk's rule: with |h| < n the total is 1 and the matches are 0).
 *   [8] |h|   [9] |r|   [10] Levenshtein(h, r), the value lxo_edit_distance writes   [11] 1 if h == r (equal length, equal tokens), else 0.
 * corpus_io int64 [LXO_TEXT_CORPUS] (nullable): [0 .. 9] the column sums of stats [0 .. 9] over the pairs, [10] sum of the distances, [11] sum of
 *   max(|h|, |r|), [12] sum of the exact matches, [13] pairs.  accumulate = 0 overwrites, accumulate = 1 adds to what is there: an evaluation runs batch
 *   after batch into one row and copies 14 integers out at its end.  BLEU-4, the edit-distance score and exact match follow from the row alone
 *   (model/evaluation/text.py scores_from_counts).
 * Tokens are compared as int32 values and ANY value is a token (negative ids, an id of V as a sentinel): an n-gram is compared only where it lies inside
 * its sequence, by position, never against padding.  Both sides are at most LXO_EDIT_MAX_REF tokens wide.
 * THE COUNTING IDENTITY: hypothesis position i counts for order n iff k < c, with k the earlier hypothesis positions holding its n-gram and c the
 * reference positions holding it; summed over i that is sum_g min(count_h(g), count_r(g)) exactly.  One wave per pair, both sides staged in LDS, one
 * walk for the four orders; integer arithmetic only, no host synchronisation, capturable into a graph, the same bytes in every run.  With stats_out
 * the corpus row is a fixed-order reduction of the rows in a second one-workgroup launch; with stats_out NULL the waves add into corpus_io with 64-bit
 * integer atomics (behind a launch that zeroes it when accumulate = 0) -- integer sums, the same in every order.
 * pairs == 0: no kernel runs; corpus_io is zeroed when accumulate == 0 and untouched otherwise.
 * -1, with the reason in lxo_last_error and nothing written: stats_out and corpus_io both NULL; a NULL hyp or ref; pairs, T, G or a stride negative,
 * hyp_block or per_ref < 1, G < 1 with pairs > 0; T outside 0 .. LXO_EDIT_MAX_REF; ref_ld outside 1 .. LXO_EDIT_MAX_REF; accumulate not 0 or 1. */
#define LXO_TEXT_STATS  12   /* int32 per pair  */
#define LXO_TEXT_CORPUS 14   /* int64 per corpus */
int lxo_text_stats(const int32_t* hyp, int hyp_block, long long hyp_block_stride, long long hyp_row_stride, long long hyp_tok_stride, int T,
                   const int32_t* hyp_len, const int32_t* ref, int G, int ref_ld, const int32_t* ref_len, const int32_t* ref_of, int per_ref,
                   int pairs, int id_end, int32_t* stats_out, long long* corpus_io, int accumulate, void* stream);
/* The edit alignment of pairs, on the device, shape-free: WHERE a hypothesis differs from its reference -- substitution, insertion and deletion
 * counts, the token-to-token maps of both sides and the confusion pairs -- from the Levenshtein table lxo_edit_distance fills, with its path kept.
 * ADDRESSING, LENGTHS, THE END CUT AND THE CLAMPING are lxo_edit_distance's (and lxo_text_stats'), argument for argument: the ids [B, max_steps, n] of
 * a sampled decode are read in place, references are taken in pad_batch_formulas' layout.  Pair p has hypothesis h (m tokens) and reference r
 * (n tokens) after the cut; both sides are at most LXO_EDIT_MAX_REF tokens wide and ANY int32 value is a token.
 * THE DEFINITION: D[i][j] is the Levenshtein table of h[0 .. i) against r[0 .. j) (D[i][0] = i, D[0][j] = j).  The canonical alignment is the path
 * walked back from (i, j) = (m, n) until (0, 0), taking at every cell the FIRST rule that applies:
 *   1. i > 0, j > 0 and D[i][j] == D[i-1][j-1] + (h[i-1] != r[j-1]): a diagonal step -- a MATCH if the tokens are equal, else a SUBSTITUTION; i--, j--.
 *   2. else i > 0 and D[i][j] == D[i-1][j] + 1: an INSERTION (h[i-1] is a token the reference does not have); i--.
 *   3. else: a DELETION (r[j-1] is a token the hypothesis lacks); j--.
 * The rule is local -- a cell's step follows from the cell, its three predecessors and one token compare -- so it is decided while the table is filled.
 * OUTPUTS (device; each nullable, not all NULL):
 *   hyp_align int32 [pairs][T]: position i < m: the reference position it is aligned with (match or substitution), -1 for an insertion; i >= m: -2.
 *   ref_align int32 [pairs][ref_ld]: position j < n: the hypothesis position it is aligned with, -1 for a deletion; j >= n: -2.
 *   counts_out int32 [pairs][LXO_ALIGN_COUNTS]: matches M, substitutions S, insertions I, deletions D, |h|, |r|.  S + I + D is the value
 *     lxo_edit_distance writes for the pair; M + S + I = |h|; M + S + D = |r|.
 *   corpus_io int64 [LXO_ALIGN_CORPUS]: [0 .. 5] the column sums of the six counts, [6] the pairs, [7] the alignment steps left out of the
 *     confusion matrix (below; 0 without one).  accumulate = 0 overwrites, accumulate = 1 adds to what is there -- lxo_text_stats' semantics.
 *   confusion_io int64 [(V + 1) * (V + 1)], V >= 1 an argument: entry [a][b] counts the alignment steps with reference token a and hypothesis token b;
 *     the index V stands for "no token": an insertion of b goes to [V][b], a deletion of a to [a][V]; matches go on the diagonal, so a row gives a
 *     token's recall; [V][V] is never written.  A step with a token outside [0, V) is counted in the counts but not entered, and counted in
 *     corpus_io[7].  The same accumulate governs it (0: the matrix is zeroed first).
 * The waves add into corpus_io and confusion_io with 64-bit integer atomics: integer sums, the same in every order.
 * SCRATCH: device memory of lxo_edit_align_scratch_bytes(pairs, T, ref_ld) bytes -- at most pairs * T * 256: per row of the table one dword per lane
 * of the pair's wave, a strip's 2-bit steps -- passed as scratch / scratch_bytes; its content after the call means nothing.
 * One launch, one wave per pair (behind one that zeroes what is overwritten); no host synchronisation, capturable into a graph, the same bytes in
 * every run.  pairs == 0: no pair kernel runs; corpus_io and confusion_io are zeroed when accumulate == 0 and untouched otherwise.
 * -1, with the reason in lxo_last_error and nothing written: all five outputs NULL; confusion_io with V < 1; scratch NULL or scratch_bytes below the
 * size function's value when pairs > 0 and T > 0; accumulate not 0 or 1; otherwise lxo_text_stats' own cases -- a NULL hyp or ref; pairs, T, G or a
 * stride negative; hyp_block or per_ref < 1; G < 1 with pairs > 0; T outside 0 .. LXO_EDIT_MAX_REF; ref_ld outside 1 .. LXO_EDIT_MAX_REF. */
#define LXO_ALIGN_COUNTS 6   /* int32 per pair  */
#define LXO_ALIGN_CORPUS 8   /* int64 per corpus */
size_t lxo_edit_align_scratch_bytes(int pairs, int T, int ref_ld);
int lxo_edit_align(const int32_t* hyp, int hyp_block, long long hyp_block_stride, long long hyp_row_stride, long long hyp_tok_stride, int T,
                   const int32_t* hyp_len, const int32_t* ref, int G, int ref_ld, const int32_t* ref_len, const int32_t* ref_of, int per_ref,
                   int pairs, int id_end, int32_t* hyp_align, int32_t* ref_align, int32_t* counts_out, long long* corpus_io, long long* confusion_io,
                   int V, int accumulate, void* scratch, size_t scratch_bytes, void* stream);
/* WHERE IN THE IMAGE a token is, on the device, shape-free: every attention map reduced to its arg-max cell, a box in feature cells, its moments and
 * entropy, and a row's maps added up over its steps (the coverage).  The maps are read where they lie and never visit the host.
 * ADDRESSING: alpha is device f32; position (i, t), i < rows, t < steps, reads the Hp x Wp map (row-major, R = Hp * Wp cells a[y * Wp + x]) that
 * starts at element t * step_stride + r * row_stride, with r = src[t * rows + i] (device int32 [steps][rows]; NULL: r = i).  Workspace region "alpha"
 * [T][B][Rp] is read with step_stride B * Rp and row_stride Rp, the alpha_out [max_steps][rows][Rp] of a decode likewise, rows [rows][steps][R] with
 * step_stride R and row_stride steps * R; whatever lies behind a map's R cells is never read.  src is for beam search, where the token of hypothesis
 * i at step t was read off its parent's row.
 * A position has NO MAP when t >= len[i] (device int32 [rows]; NULL: never), when r lies outside [0, alpha_rows), or when the map's f32 sum is not a
 * positive finite number (all zero, a NaN or an infinity in it).  Every output of such a position is its NONE value below.  Cells are weights: a map
 * with negative cells has unspecified (in-bounds) outputs.
 * THE DEFINITION for a map a with S = sum a:
 *   peak_out int32 [rows][steps]: the arg-max cell index, the lower index on ties -- a comparison of f32 values, bit-defined.  NONE: -1.
 *   box_out int32 [rows][steps][4] = (x0, y0, x1, y1), inclusive, in feature cells: the central-mass interval of each marginal.  With
 *     px(x) = sum_y a[y * Wp + x], Cx its running sum and tail = (0.5 * (1 - mass)) * S:  x0 = min{x : Cx(x) > tail}, x1 = min{x : Cx(x) >= S - tail};
 *     y0, y1 the same from py(y) = sum_x a[y * Wp + x].  mass = 1 gives the bounding box of the support, a one-cell map gives that cell.
 *     x0 <= x1 ALWAYS: Cx is non-decreasing, and mass > 0 gives tail < S / 2 < S - tail, so Cx(x1) >= S - tail > tail and the first x whose Cx exceeds
 *     tail is no later than x1.  (Where 1 - mass rounds to 1 the two thresholds meet; the kernel then takes x1 = max(x0, x1).)
 *     WHAT THE BOX HOLDS: each marginal leaves at most tail on either side, so the box holds at least 2 * mass - 1 of S -- a union bound over
 *     the two axes, not mass itself (a diagonal map shows the difference).
 *     The kernel forms the cumulative sums in exact integer arithmetic on cells truncated to 2^-40 of S's binade, so they are exactly monotone and the
 *     same in any order; on maps whose cells are multiples of 2^-12 with S <= 2 the edges are those of exact arithmetic, elsewhere they can differ
 *     from it only where a cumulative sum lies within the cells' own f32 rounding of a threshold.  NONE: -1 four times.
 *   stats_out f32 [rows][steps][LXO_LOCATE_STATS]: [0] S (f32 sum);  [1] cx = sum x px(x) / S, [2] cy likewise;  [3] sx = sqrt(sum px(x) (x - cx)^2 / S),
 *     [4] sy likewise -- the CENTRED second moment, no cancellation;  [5] the entropy -sum (a/S) ln(a/S) in nats (0 ln 0 = 0);  [6] inside = the share
 *     of S within the box;  [7] peak_share = a[peak] / S.  f32 sums in a fixed order.  NONE: eight zeros.
 *   coverage_out f32 [rows][cov_ld], cov_ld >= R: cell r < R of row i = sum over t of a_t[r] over the row's positions that have a map, ADDED IN
 *     ASCENDING t into one f32 accumulator from 0.f -- bit-reproducible, restatable exactly in np.float32.  Cells [R, cov_ld) are not written.
 * Each output is nullable, not all four.  One launch of one wave per position (the map staged once in LDS; both marginals, the box and the inside
 * pass come from that one read) and a second small launch for the coverage; no atomics, no host synchronisation, capturable into a graph, the same
 * bytes in every run.  rows == 0 or steps == 0 launches nothing per position; the coverage of a row without steps is zeros.
 * Refusals, with the reason in lxo_last_error, nothing written and nothing launched:
 * -1: a NULL alpha; all four outputs NULL; mass outside (0, 1] or not finite; a stride, alpha_rows, rows or steps negative; coverage_out with cov_ld < R.
 * -5: Hp or Wp < 1; R above LXO_LOCATE_MAX_CELLS, the kernel's staging limit (98 x 98 = 9604, the map of an 800 x 800 input, fits); more positions
 * than a grid holds (rows * steps > 2^31 - 5). */
#define LXO_LOCATE_STATS     8      /* f32 per position */
#define LXO_LOCATE_MAX_CELLS 9728
int lxo_attention_locate(const float* alpha, long long step_stride, long long row_stride, int alpha_rows, int Hp, int Wp, int rows, int steps,
                         const int32_t* len, const int32_t* src, float mass, int32_t* peak_out, int32_t* box_out, float* stats_out,
                         float* coverage_out, int cov_ld, void* stream);
/* The candidate rows of a minimum-risk step, built on the device from a sampled decode: three launches, no host synchronisation.
 * ids int32 [B, max_steps, n] as lxo_sample_decode leaves them and steps = the steps it ran (0 <= steps <= max_steps, 1 <= n <= 16);
 * ref int32 [B, Tr] with ref_len [B] in pad_batch_formulas' layout (tokens, END, PAD; length = tokens + 1), 1 <= Tr <= LXO_EDIT_MAX_REF.
 * With R = B * (n + include_reference) and Tc = max(steps + 1, Tr), all outputs device, NOT NULL:
 * cand int32 [R, Tc]: image g's candidates are the consecutive rows group_off[g] .. group_off[g + 1] - 1 -- its reference first (include_reference;
 * its first ref_len tokens cut at END), then its DISTINCT draws in ascending draw index, each cut at its first END within `steps`: of equal draws
 * (equal length, equal tokens) the first is kept, a draw equal to the reference is dropped.  A row is its tokens, then id_end, then id_pad up to Tc.
 * cand_len int32 [R] = tokens + 1; row_image int32 [R] = g; group_off int32 [B + 1]; cost f32 [R] = lxo_edit_distance's cost_out of the row against
 * its image's reference (the same kernel), 0 exactly for the reference's own row.
 * Rows at and behind group_off[B] are DEAD: all id_pad, length 0, cost 0, row_image 0 -- lxo_mrt_weights gives them w = q = 0, the weighted loss
 * leaves a length of 0 out.  cost doubles as the launches' scratch: its content is final only after the call's last kernel.
 * -1: a NULL argument, B < 0, n outside 1 .. 16, steps outside [0, max_steps], Tr outside 1 .. LXO_EDIT_MAX_REF, id_end < 0. */
int lxo_mrt_candidates(const int32_t* ids, int B, int max_steps, int n, int steps, const int32_t* ref, int Tr, const int32_t* ref_len,
                       int id_end, int id_pad, int include_reference, int32_t* cand, int32_t* cand_len, float* cost, int32_t* group_off,
                       int32_t* row_image, void* stream);
/* Consensus (minimum-Bayes-risk choice) among n sampled transcriptions per image, on the device, shape-free: two launches, no host synchronisation,
 * no atomics, capturable into a graph.
 * DRAWS: draw i of image g starts at element g * image_stride + i * draw_stride of `ids` and its tokens lie tok_stride elements apart; its sequence
 * s_i is the first T tokens cut at the first id_end (truncate_end's rule; id_end < 0: no cut).  The ids [B, max_steps, n] that lxo_sample_decode
 * writes are read in place with image_stride max_steps * n, draw_stride 1, tok_stride n, T = the steps run; rows [B, n, T]: T * n, T, 1.
 * THE DEFINITION:
 *   dist[g][i][j] = Levenshtein(s_i, s_j): int32, exact, symmetric, 0 on the diagonal.
 *   c(i, j) = (float)dist[g][i][j] / (float)max(|s_j|, 1) with normalize = 1 -- draw j plays the reference, one f32 division as lxo_edit_distance's
 *     cost_out -- and (float)dist[g][i][j] with normalize = 0.
 *   w_j = weights[g][j], device f32 [B][n]; NULL: every weight is 1.  A weight that is negative or not finite counts as 0; an image whose weights
 *     (so read) sum to 0 gets all ones.
 *   risk[g][i] = (sum_j w_j * c(i, j)) / (sum_j w_j): f32, every product and sum rounded on its own (no fused multiply-add), both sums added in
 *     ascending j from 0.f, one final division.
 *   best[g] = the smallest i whose stored risk[g][i] is the minimum: an f32 comparison of the values written, ties go to the lower draw index.
 * With NULL weights and normalize = 0 every term and every partial sum is an integer below 2^24 (n <= 64 draws of <= 1024 tokens), so the sums are
 * exact and risk[g][i] is the correctly rounded f32 quotient (float)(sum_j dist[g][i][j]) / (float)n: exact up to that one division.  Equal draws
 * have equal rows of dist and so equal risks, bit for bit.  The distances are integer arithmetic and every float sum has a fixed order: the same
 * bytes in every run.
 * OUTPUTS (device, all NOT NULL): dist_out int32 [B][n][n] -- also the hand-over between the two launches; risk_out f32 [B][n] -- it holds the
 * draws' lengths as scratch between the launches, its content is final after the second; best_out int32 [B].
 * B == 0 launches nothing.  T == 0 or n == 1: dist and risk all 0, best 0.
 * -1, with the reason in lxo_last_error and no output written: a NULL ids, dist_out, risk_out or best_out; B < 0; n outside
 * 1 .. LXO_CONSENSUS_MAX_N; T outside 0 .. LXO_EDIT_MAX_REF; a negative stride; normalize other than 0 or 1; more than 2^31 - 16 pairs
 * B * n * (n - 1) / 2. */
#define LXO_CONSENSUS_MAX_N 64
int lxo_consensus(const int32_t* ids, long long image_stride, long long draw_stride, long long tok_stride, int B, int n, int T, int id_end,
                  const float* weights, int normalize, int32_t* dist_out, float* risk_out, int32_t* best_out, void* stream);
/* Sentence-level BLEU of pairs, on the device, shape-free: the text metric as a COST, for minimum-risk training and consensus decoding.
 * ADDRESSING, LENGTHS, THE END CUT AND THE CLAMPING are lxo_edit_distance's (and lxo_text_stats'), argument for argument.  Pair p has hypothesis h
 * and reference r after the cut.  THE DEFINITION:
 *   m_n, n = 1 .. 4: the clipped matches, sum over the distinct n-grams g of h of min(count_h(g), count_r(g)); t_n = max(1, |h| - n + 1).  Both are
 *     exactly columns 0 .. 7 of lxo_text_stats.
 *   Smoothing (Lin and Och's add-one on the higher orders only; nltk's SmoothingFunction().method2): p_1 = m_1 / t_1, p_n = (m_n + 1) / (t_n + 1)
 *     for n = 2, 3, 4.
 *   Brevity penalty: BP = 1 if |h| > |r|, else exp(1 - |r| / |h|).
 *   sBLEU = 0 if m_1 = 0 (an empty hypothesis included), else BP * exp(1/4 * sum_n ln p_n).  cost = 1 - sBLEU, in [0, 1].
 *   EQUALITY OVERRIDE: if h == r (equal length, equal tokens; two empty sequences are equal) then sBLEU = 1.f and cost = 0.f exactly, whatever
 *     the formula says -- smoothed, an identical 2-token pair has p_3 = p_4 = 1/2.  So a reference costs 0 against itself and equal hypotheses
 *     cost the same bit for bit.
 *   Arithmetic: f32, logf / expf, one division per p_n, the logs added in ascending n; model/evaluation/text.py sentence_bleu restates it in
 *     float64 on the host.  The counts are integers and exact; the floats agree with the float64 value within 1e-5.
 * OUTPUTS (device, at least one NOT NULL): counts_out int32 [pairs][LXO_BLEU_COUNTS] = m_1 .. m_4, t_1 .. t_4, |h|, |r|; bleu_out f32 [pairs] =
 * sBLEU; cost_out f32 [pairs] = 1 - sBLEU.
 * One launch, one wave per pair: both sides staged in LDS, one walk for the four orders (lxo_text_stats' counting identity), NO Levenshtein DP, an
 * equality compare, the float tail on wave-uniform values.  No host synchronisation, capturable into a graph, the same bytes in every run.
 * Both sides are at most LXO_EDIT_MAX_REF tokens wide.  pairs == 0 launches nothing.
 * -1, with the reason in lxo_last_error and nothing written: the three outputs all NULL; otherwise lxo_text_stats' own cases -- a NULL hyp or ref;
 * pairs, T, G or a stride negative; hyp_block or per_ref < 1; G < 1 with pairs > 0; T outside 0 .. LXO_EDIT_MAX_REF; ref_ld outside
 * 1 .. LXO_EDIT_MAX_REF. */
#define LXO_BLEU_COUNTS 10   /* int32 per pair */
int lxo_sentence_bleu(const int32_t* hyp, int hyp_block, long long hyp_block_stride, long long hyp_row_stride, long long hyp_tok_stride, int T,
                      const int32_t* hyp_len, const int32_t* ref, int G, int ref_ld, const int32_t* ref_len, const int32_t* ref_of, int per_ref,
                      int pairs, int id_end, int32_t* counts_out, float* bleu_out, float* cost_out, void* stream);
/* lxo_consensus under the cost 1 - sBLEU (lxo_sentence_bleu's definition): the draws are addressed and cut as lxo_consensus', the weights read
 * and the risk and the arg-min formed as there; there is no `normalize`.
 *   c(i, j) = lxo_sentence_bleu's cost of hypothesis s_i against reference s_j -- draw j plays the reference; 0.f exactly for equal draws and on
 *     the diagonal.  The cost is NOT symmetric (t_n and BP are the hypothesis'), the clipped matches are: sum_g min(count_i(g), count_j(g)).  One
 *     wave per UNORDERED pair counts them once and writes c(i, j) and c(j, i); equal draws are found by a compare and skip the count.
 *   risk[g][i] = (sum_j w_j * c(i, j)) / (sum_j w_j) and best[g] exactly as lxo_consensus states them.  Equal draws have equal rows of costs --
 *     the same integers go through the same f32 operations -- and so equal risks, bit for bit.
 * OUTPUTS (device): match_out int32 [B][n][n][4] (nullable): the clipped matches of orders 1 .. 4, symmetric; on the diagonal a draw against itself,
 * its own n-grams max(0, |s_i| - n + 1).  cost_out f32 [B][n][n] (NOT NULL), cost_out[g][i][j] = c(i, j) -- also the hand-over between the two
 * launches; risk_out f32 [B][n]; best_out int32 [B] (both NOT NULL).
 * B == 0 launches nothing.  T == 0 or n == 1: costs and risks all 0, best 0.
 * -1, with the reason in lxo_last_error and no output written: a NULL ids, cost_out, risk_out or best_out; B < 0; n outside
 * 1 .. LXO_CONSENSUS_MAX_N; T outside 0 .. LXO_EDIT_MAX_REF; a negative stride; more than 2^31 - 16 pairs B * n * (n - 1) / 2. */
int lxo_consensus_bleu(const int32_t* ids, long long image_stride, long long draw_stride, long long tok_stride, int B, int n, int T, int id_end,
                       const float* weights, int32_t* match_out, float* cost_out, float* risk_out, int32_t* best_out, void* stream);
/* THE FINISH OF A BEAM SEARCH on the device: the k hypotheses of every image back-traced from what the beam decodes leave, without a copy or a
 * synchronisation.  The search itself is not touched.
 * INPUTS (device): ids, parents int32 and scores f32 (nullable), each [B][ld_t][k] as lxo_beam_decode* write them with ld_t = max_steps; steps <= ld_t
 * is the number of valid steps -- what lies at or behind step `steps` is never read.
 * THE DEFINITION (utils/text.beam_slots' rule), with P[b][t][j] = min(max(parents[b][t][j], 0), k - 1) -- a parent outside [0, k) is clamped into
 * it, so no content can fault:
 *   slot[b][steps - 1][i] = i,  slot[b][t - 1][i] = P[b][t][slot[b][t][i]]        the beam slot at step t of the hypothesis that ends in slot i
 *   tok[b][t][i] = ids[b][t][slot[b][t][i]],  run[b][t][i] = scores[b][t][slot[b][t][i]]
 *   len_out int32 [B][k]: 1 + the first t with tok[b][t][i] == id_end, steps if there is none: the tokens through the path's first id_end.  An
 *     id_end in a slot that is not on the path does not count.  1 <= len <= steps.
 *   hyp_out int32 [B][steps][k]: tok[b][t][i] for t < len[b][i], id_end behind.  The layout of the input, so lxo_consensus, lxo_consensus_bleu,
 *     lxo_text_stats, lxo_edit_align and lxo_sentence_bleu read the hypotheses in place (image stride steps k, draw stride 1, token stride k).
 *   src_out int32 [steps][B k]: src[t][b k + i] = b k + P[b][t][slot[b][t][i]], the decoder row whose attention map produced the token (the parent's
 *     row): utils/text.beam_parent_rows transposed to the src of lxo_attention_locate.  Written for every t < steps.
 *   tok_logp_out f32 [B][steps][k]: run[t] - run[t - 1] as ONE f32 subtraction, run[-1] = 0.f, for t < len; 0.f behind.
 *   seq_logp_out f32 [B][k]: run[len - 1], the frozen score of the hypothesis.
 * Each output is nullable (not all five); the last two need scores.  One launch, one workgroup per image: the parents are staged in LDS a byte
 * each, one lane per slot walks them back there, then ids and scores are gathered and every output element is written once.  No atomics, no host
 * synchronisation, capturable into a graph, the same bytes in every run.  B == 0 launches nothing.
 * -1, with the reason in lxo_last_error, nothing written and nothing launched: a NULL ids or parents; all outputs NULL; tok_logp_out or seq_logp_out
 * without scores; B < 0; id_end < 0; ld_t < steps; B * k above 2^31 - 1.
 * -5: k outside 1 .. LXO_BEAM_MAX_K; steps outside 1 .. LXO_BEAM_MAX_STEPS (the LDS stage; the limit lxo_consensus has). */
#define LXO_BEAM_MAX_K     16
#define LXO_BEAM_MAX_STEPS 1024
int lxo_beam_finalize(const int32_t* ids, const int32_t* parents, const float* scores, int B, int ld_t, int steps, int k, int id_end,
                      int32_t* hyp_out, int32_t* len_out, int32_t* src_out, float* tok_logp_out, float* seq_logp_out, void* stream);
/* THE RERANK of a finished beam: GNMT's length and coverage normalisation applied to the k hypotheses the search returned -- the search is as the
 * reference runs it, the penalties only reorder its result.
 * INPUTS (device): len int32 [B][k] and seq_logp f32 [B][k] (finite) as lxo_beam_finalize writes them; coverage f32 [B k][cov_ld] (nullable), R <= cov_ld
 * cells read per row: the coverage_out of lxo_attention_locate given lxo_beam_finalize's src_out and len_out.  alpha, beta >= 0; cov_floor in (0, 1].
 * THE DEFINITION, per image over its slots i < k:
 *   lp_i = ((5 + max(len_i, 0)) / 6)^alpha
 *   cp_i = sum_{r < R} log(min(max(cov_i[r], cov_floor), 1)), 0 without coverage          (a NaN cell counts as cov_floor)
 *   score_out f32 [B][k] = seq_logp_i / lp_i + beta * cp_i
 *   post_out  f32 [B][k] = exp(seq_logp_i - m) / sum_j exp(seq_logp_j - m), m = max_j seq_logp_j: the softmax of the frozen scores, the weights of a
 *     consensus over the beam
 *   order_out int32 [B][k]: the slots by descending score_out -- the f32 values written -- equal scores by ascending slot (scores with a NaN:
 *     unspecified, in bounds).
 * The cells of one image are the same for all its hypotheses: cells that belong to the padding of a batch canvas are attended by none of them, each
 * adds log(cov_floor) to every cp_i of the image, and so they shift an image's scores TOGETHER -- the order within an image does not see them,
 * scores of different images are comparable only at equal padding.
 * ARITHMETIC: logf per cell, its sum over the cells in double in a fixed order; lp, the quotient, the product with beta, the sum and the softmax in
 * double, each output rounded to f32 once.  So alpha = 0 without coverage gives score_out = seq_logp BIT FOR BIT (x^0 = 1, x / 1 = x, nothing added),
 * and equal (len, seq_logp) without coverage give equal scores bit for bit.
 * Each output is nullable (not all three).  One launch, one wave per image; no atomics, no host synchronisation, graph-capturable, the same bytes
 * in every run.  B == 0 launches nothing.
 * -1: a NULL len or seq_logp; all outputs NULL; B < 0; B * k above 2^31 - 1; alpha or beta negative or not finite; cov_floor outside (0, 1]; with
 * coverage, R < 0 or cov_ld < R.  -5: k outside 1 .. LXO_BEAM_MAX_K. */
int lxo_beam_rerank(const int32_t* len, const float* seq_logp, const float* coverage, int cov_ld, int R, int B, int k, float alpha, float beta,
                    float cov_floor, float* score_out, float* post_out, int32_t* order_out, void* stream);
/* lxo_mrt_candidates with the cost chosen: cost_kind = LXO_COST_EDIT is that call bit for bit (it forwards here); with LXO_COST_BLEU the third
 * launch is lxo_sentence_bleu's kernel and cost f32 [R] = 1 - sBLEU of the row against its image's reference -- 0 exactly for the reference's own
 * row (the equality override) and for the dead rows.  Then the rows are a side of that kernel: steps + 1 <= LXO_EDIT_MAX_REF as well.
 * -1: lxo_mrt_candidates' cases; a cost_kind other than the two; with LXO_COST_BLEU, steps + 1 > LXO_EDIT_MAX_REF. */
#define LXO_COST_EDIT 0
#define LXO_COST_BLEU 1
int lxo_mrt_candidates_cost(const int32_t* ids, int B, int max_steps, int n, int steps, const int32_t* ref, int Tr, const int32_t* ref_len,
                            int id_end, int id_pad, int include_reference, int32_t* cand, int32_t* cand_len, float* cost, int32_t* group_off,
                            int32_t* row_image, int cost_kind, void* stream);
/* Teacher-forced scoring, after lxo_decoder_train_fwd with the same shape and formula: per-token log-probs, the model's top-1 token per
 * position and per-sequence sums; reads ws region "logits", writes only the caller's outputs (device, [B, T] / [B]).
 * logp_out f32 [B, T] (NOT NULL): log_softmax(logits of step t)[formula[b][t]] for t < lengths[b], 0 after.
 * top1_out int32 [B, T] (nullable): the arg-max of step t's logits (the lower id on ties, as greedy decode picks it), -1 for t >= lengths[b].
 * seq_out f32 [B] (nullable): logp_out[b][0] + ... + logp_out[b][lengths[b] - 1], added in ascending t in f32.
 * -seq_out summed over the batch is the "sum CE" lxo_ce_loss_fwd_bwd leaves, up to summation order.  Token ids outside [0, V) are clamped
 * (the caller should refuse them).  When the forward chain's error word is set every logp / seq is NaN and every top1 -1. */
int lxo_score_tokens(const lxo_shape* s, void* ws, const int32_t* formula, const int32_t* lengths,
                     float* logp_out, int32_t* top1_out, float* seq_out, void* stream);
/* Alternatives per position, after lxo_decoder_train_fwd with the same shape and formula: the model's k best tokens at every step of the
 * teacher-forced pass, the rank of the given token and the entropy of the step; reads ws region "logits" and the forward chain's error
 * word, writes only the caller's outputs (device), uses no workspace region of its own.  1 <= k <= min(16, V).
 * ORDER: value descending on the raw f32 logits, then token id ascending -- exact ties go to the lower id, as greedy decode picks.
 * ids_out int32 [B, T, k] (NOT NULL): slot j = the j-th token of step t in that order.  logp_out f32 [B, T, k] (NOT NULL): its
 * log_softmax.  rank_out int32 [B, T] (nullable): the number of tokens in front of formula[b][t] in that order (0 = it is the model's
 * top-1).  entropy_out f32 [B, T] (nullable): sum_v p_v (lse - x_v), in nats.
 * Bit identities with lxo_score_tokens on the same workspace: ids_out[b][t][0] is its top1_out[b][t]; a slot whose id is the (clamped)
 * formula token carries its logp_out[b][t], and that slot's index is rank_out[b][t].
 * allow / allow_ld: allowed-token sets as in lxo_greedy_decode_constrained (one row per sample b), or NULL / 0 for none.  A banned token
 * is a column outside the vocabulary: the log-sum-exp, the selection, the rank and the entropy run over the allowed tokens; a banned
 * formula token has rank -1; where fewer than k tokens are allowed the remaining slots are id -1, logp -inf.  Words of a set are read
 * inside [0, (V + 31) / 32) only.
 * t >= lengths[b]: ids -1, logp 0, rank -1, entropy 0.  Forward chain's error word set: ids -1, logp NaN, rank -1, entropy NaN, everywhere.
 * -1: a NULL ids_out or logp_out, k out of range, a non-NULL allow with 0 < allow_ld < (V + 31) / 32, a NULL allow with allow_ld != 0. */
int lxo_score_alternatives(const lxo_shape* s, void* ws, const int32_t* formula, const int32_t* lengths, int k,
                           const uint32_t* allow, int allow_ld, int32_t* ids_out, float* logp_out,
                           int32_t* rank_out, float* entropy_out, void* stream);
/* BPTT through the decoder (what TF autodiff does for img2seq.py:119-123);
 * accumulates decoder gradients into grads and leaves d(enc) in ws region "d_img" (bf16 mode: already masked by conv6's
 * ReLU and converted, with conv6's bias gradient added to grads; f32 mode: the plain f32 gradient). */
int lxo_decoder_train_bwd(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                          const int32_t* formula, float* grads, void* stream);
/* The same in two parts so that a data-parallel caller can start reducing gradients before the recurrence has run:
 * parts bit 0 = d_o from the logits for every step + the y_W_o gradient (final after this part);
 * parts bit 1 = BPTT, every other decoder gradient and d(enc). */
int lxo_decoder_train_bwd_part(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                               const int32_t* formula, float* grads, int parts, void* stream);

/* Health of the persistent decoder chains (lxo_shape.step_kernels == 0, bf16: lxo_decoder_train_fwd / _bwd run the recurrence as ONE
 * launch of 8 XCD-local chains that rely on the hardware placing 32 workgroups of the grid on every XCD).  A chain that does not
 * assemble within 200 ms gives up (no hang) and leaves a non-zero ERROR WORD; the call's outputs are then invalid.  The words live in
 * ws region "xdec_sync": int32 index LXO_XDEC_ERR_WORD of block 0 (forward chain) and of block 1 (backward chain), a block being
 * LXO_XDEC_BLOCK_BYTES bytes; both are cleared by every lxo_decoder_train_fwd / _bwd call, whether a chain runs in it or not.
 * The forward chain's word also turns the loss of lxo_ce_loss_fwd_bwd* into NaN.
 * lxo_chain_guard folds both words into the optimizer's scale ON THE DEVICE (no host synchronisation): scale_io[0] becomes NaN when
 * either word is set, else stays (have_scale != 0: the value lxo_global_norm_scale left) or becomes 1 (have_scale == 0);
 * lxo_adam_step / lxo_optimizer_step DROP the step (touch nothing) when *scale_dev is NaN.  Data parallel: lxo_decoder_train_bwd[_part]
 * turns the LAST element of `grads` (y_W_o's last) into NaN when a chain of this rank failed, the gradient all-reduce spreads it, and
 * lxo_chain_guard (grads != NULL) also drops the step when it reads a NaN there -- every rank drops the same steps, the replicas stay
 * identical.  status_out (device, 3 words, may be NULL) receives {forward word, backward word, 1 if the step is dropped} so that a
 * caller can copy them to the host asynchronously, switch to lxo_shape.step_kernels = 2 (the launch-per-step kernels) when one of its
 * own words is set, and take back the time step of a dropped Adam update.  Call it behind lxo_decoder_train_bwd and the gradient
 * exchange, on the stream the optimizer runs on.
 * Reference: the step this protects is model/img2seq.py:169 (one sess.run = forward, loss, gradients, update). */
#define LXO_XDEC_BLOCK_BYTES (4096 + (384 << 10))
#define LXO_XDEC_ERR_WORD 512
int lxo_chain_guard(const lxo_shape* s, void* ws, const float* grads, float* scale_io, int have_scale, uint32_t* status_out, void* stream);

/* tf.clip_by_global_norm scale (img2seq.py:119-121): scale_out[0] = clip / max(||g||, clip),
 * scale_out[1] = ||g|| ; device memory, no host sync.  clip <= 0 -> scale 1.  scale_out must hold LXO_GNORM_FLOATS floats:
 * the rest is scratch for one partial sum of squares per workgroup, which are added in workgroup order (no float atomics:
 * the norm is the same in every run). */
#define LXO_GNORM_FLOATS (2 + 1024)
int lxo_global_norm_scale(long long n, const float* grads, float clip, float* scale_out, void* stream);
/* tf.train.AdamOptimizer update (img2seq.py:101), TF epsilon placement:
 * m,v updated; theta -= lr_t * m / (sqrt(v) + eps), grads pre-multiplied by *scale_dev if given.
 * A NaN *scale_dev (lxo_chain_guard) drops the step: params, m and v are left untouched. */
int lxo_adam_step(long long n, float* params, const float* grads, float* m, float* v,
                  float lr_t, float beta1, float beta2, float eps, const float* scale_dev, void* stream);

/* the non-Adam branches of add_optimizer (img2seq.py:102-107), TF-1.12 defaults:
 * method 1 GradientDescentOptimizer, 2 AdagradOptimizer (slot = accumulator, caller initialises to 0.1),
 * 3 RMSPropOptimizer (slot = rms, caller initialises to 1; decay 0.9, momentum 0, epsilon 1e-10). */
int lxo_optimizer_step(int method, long long n, float* params, const float* grads, float* slot, float lr,
                       const float* scale_dev, void* stream);

/* dynamic_decode + GreedyDecoderCell (dynamic_decode.py:17-74, greedy_decoder_cell.py:40-66):
 * runs on the encoder output already in ws; ids_out int32 [B, max_steps] (device),
 * *steps_out = number of steps executed (<= max_iter + 1).  Host-synchronising.  Columns >= *steps_out of ids_out are
 * unspecified (the loop runs ahead of the host's all-finished check).  Where the shape qualifies (bf16, step_kernels 0,
 * U = O = C = 512, E = 256, B in {8, 16, 32, 64}, V <= 512, MI355X) the steps run as a persistent chain, up to 16 per
 * launch (csrc/xdec.hip: xdec_dec_kernel; LXO_XDEC_DEC=0 disables); a chain that fails to assemble is detected by the
 * call, which then repeats the decode on the launch-per-step kernels. */
int lxo_greedy_decode(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                      int id_end, int max_iter, int32_t* ids_out, int* steps_out, void* stream);
/* lxo_greedy_decode that also exports the attention weights of every step: alpha_out f32
 * [max_steps][B][Rp] (device), Rp = (R+7)/8*8, row r = region (y*W' + x) -- the data the reference taps with
 * its tf.py_func hook (attention_mechanism.py:96-105) for visualize_attention.py. */
int lxo_greedy_decode_attn(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                           int id_end, int max_iter, int32_t* ids_out, float* alpha_out, int* steps_out, void* stream);
/* lxo_greedy_decode(_attn) that also returns the model's probability of every token it emits: logp_out f32 [B, max_steps] (device,
 * NOT NULL), logp_out[b][t] = log_softmax(logits of step t)[ids_out[b][t]] -- the reference's DecoderOutput.logits reduced to the
 * chosen token.  A row that has emitted END goes on being decoded (as its ids do) and its later columns are the log-probs of those
 * ids: the sequence log-prob is the sum through the first END.  Columns >= *steps_out are unspecified.  alpha_out: as in
 * lxo_greedy_decode_attn, or NULL for none.  The persistent chain, where the shape qualifies, computes the log-probs in place
 * (its ids are those of lxo_greedy_decode); the launch-per-step fall-back rewrites them with the ids. */
int lxo_greedy_decode_scores(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                             int32_t* ids_out, float* logp_out, float* alpha_out, int* steps_out, void* stream);
/* Greedy decode from a given prefix.  prefix int32 [B, prefix_ld] and prefix_len int32 [B] (device, NOT NULL, prefix_ld >= 1): at a
 * step t < P_b = prefix_len[b] row b emits prefix[b][t] (fed to step t + 1 like any emitted id) and stays unfinished; from step P_b on it
 * is lxo_greedy_decode's arg-max step.  The loop ends, as there, after the first step that leaves no row unfinished or after step max_iter.
 * Contract: 0 <= P_b <= min(prefix_ld, max_iter), prefix ids in [0, V) and never id_end; rows may differ in P_b.  What the device holds
 * is read defensively (a length is clamped into that range, an id outside [0, V) reads as 0): nothing faults.  logp_out (nullable):
 * as in lxo_greedy_decode_scores; at a forced step, the log-prob of the forced id.  alpha_out (nullable): as in lxo_greedy_decode_attn
 * (the launch-per-step path).  With every P_b = 0 the outputs are those of lxo_greedy_decode(_scores). */
int lxo_greedy_decode_prefix(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                             const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                             int32_t* ids_out, float* logp_out, float* alpha_out, int* steps_out, void* stream);
/* Greedy decode under a token constraint: an ALLOWED-TOKEN SET PER IMAGE.  allow (device, NOT NULL): bit sets, bit v & 31 of word v >> 5
 * of row b set = token v may be emitted by image b; allow_ld in words: 0 = one set shared by every image, else >= (V + 31) / 32 and allow
 * is [B][allow_ld].  Bits at or beyond V are ignored.  The one rule: a banned vocabulary column behaves as a column outside the
 * vocabulary -- its logit is -inf before anything else happens in the select step.  So the arg-max runs over the allowed columns (ties:
 * the lower index) and logp_out (nullable) holds logit - logsumexp(allowed logits), the model's distribution renormalised over the set;
 * with every column allowed the outputs are those of lxo_greedy_decode_prefix / _scores.  The set is constant over the steps of a call (a set that follows the row's history: lxo_greedy_decode_grammar).
 * prefix / prefix_ld / prefix_len: as in lxo_greedy_decode_prefix, or all NULL / 0 for no prefix; a forced id is emitted as given, its
 * log-prob taken under the same renormalised distribution.  Contract: in every row id_end is allowed and at least one token is; no forced
 * prefix token is banned in its row.  The device reads defensively: a row that breaks the contract does not fault or hang (it may emit id 0
 * and an unspecified log-prob).  -1: NULL allow, allow_ld < 0 or 0 < allow_ld < (V + 31) / 32, half a prefix.  alpha_out non-NULL runs the
 * launch-per-step path.  lxo_decode_step and lxo_score_tokens take no constraint. */
int lxo_greedy_decode_constrained(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                                  const uint32_t* allow, int allow_ld,
                                  const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                                  int32_t* ids_out, float* logp_out, float* alpha_out, int* steps_out, void* stream);
/* Sampled decode: DRAWS from the model's distribution instead of its arg-max.  For a decoder row with f32 logits x[0..V) and its image's allowed
 * set A (a banned column is a column outside the vocabulary): y = x * (1 / temperature); the row's order is value descending, then column
 * ascending; C_K = its first top_k allowed columns (top_k = 0 or >= |A|: all of A); C = the shortest prefix of the order inside C_K whose
 * softmax(y over C_K) mass is >= top_p (1: all of C_K) -- temperature, then top-k, then top-p on the renormalised mass; the token is
 * argmax over C of y_v + g_v (ties: the lower column), g_v = -log(-log u_v), the Gumbel-max form of a draw from softmax(y over C).  The uniforms
 * are counter-based: mix(z) = splitmix64's step (z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) *
 * 0x94D049BB133111EB; z ^= z >> 31), key = mix(seed << 32 | b << 4 | j) for draw j of image b, u_v = ((mix(key + t * V + v) >> 41) + 0.5) * 2^-23 at
 * step t.  So draw (b, j) depends on neither n nor B nor any other row, the same seed repeats bit for bit, and top_k = 1 is the arg-max. */
typedef struct lxo_sample_opts { float temperature; int top_k; float top_p; unsigned seed; } lxo_sample_opts;
/* n = s->beam rows per image (1..16), each an independent draw of the whole sequence.
 * ids_out int32 [B, max_steps, n]; logp_out, logq_out f32, same shape, nullable: logp = x_id - logsumexp_A(x), the model's own log-prob as in
 * lxo_greedy_decode_scores / _constrained; logq = y_id - logsumexp_C(y), the log-prob under the distribution sampled from.
 * allow / prefix: ONE ROW PER IMAGE, as in the beam calls, all NULL / 0 for none.  alpha_out (nullable): f32 [max_steps][B * n][Rp].
 * The loop is lxo_greedy_decode's at n rows per image: a row is finished once it draws END at a free step (it goes on being decoded; its later
 * columns are deterministic, no more); the loop ends after the first step with no unfinished row, or at max_iter.  At a forced step the forced id is
 * emitted with its logp, logq is 0 and nothing is drawn; step t's uniforms keep the global t.  Launch per step in both dtypes.
 * -1: NULL opts / ids_out, temperature or 1 / temperature not positive and finite in f32, top_k < 0, top_p outside (0, 1], a half-given set or prefix; -5: the shape limits of the
 * other decodes (max_steps <= max_iter, beam outside 1 .. min(16, V)); all before any launch.  The device reads defensively, as the constrained
 * calls do: an empty allowed row emits 0 and nothing faults. */
int lxo_sample_decode(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                      const lxo_sample_opts* opts, const uint32_t* allow, int allow_ld,
                      const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                      int32_t* ids_out, float* logp_out, float* logq_out, float* alpha_out, int* steps_out, void* stream);
/* The select step alone, on logits the caller holds (e.g. ws region "dec_logits" after lxo_decode_cell_step): logits f32 [rows][ld] (device),
 * row r = image r / n, sample r % n, step `time`.  Writes ids / logp / logq [rows] (the last two nullable).  No finished flags.
 * -5: V < 1, ld < V, rows < 1, n outside 1 .. 16, time < 0; -1: the option and set refusals of lxo_sample_decode. */
int lxo_sample_tokens(const float* logits, int ld, int rows, int n, int V, int time, const lxo_sample_opts* opts,
                      const uint32_t* allow, int allow_ld, int32_t* ids_out, float* logp_out, float* logq_out, void* stream);
/* The same loops ONE STEP AT A TIME: the calls behind the reference's decoder-cell protocol (dynamic_decode.py:35-36,43-44:
 * decoder_cell.initialize() / .step(time, state, inputs, finished); greedy_decoder_cell.py:46-66,
 * beam_search_decoder_cell.py:113-187).  latex_ocr_amd/model/components/ wraps them in cell objects with the reference's
 * method names.  The cell state (c, h, o, running log-probs, finished flags, the ids fed back) stays in ws.
 *   lxo_decode_begin: initialize() -- attention set-up and initial states for s->beam hypotheses per image (1 = greedy).
 *   lxo_decode_step:  step(time) -- writes column `time` of ids_out int32 [B, max_steps(, beam)] (and parents_out, beam only;
 *     may be NULL), copies the per-row finished flags (int32 [B * beam], 0 / 1, after this step, before the loop's own
 *     `time >= maximum_iterations` OR) to finished_host and the number of unfinished rows to *unfinished_host (either may be
 *     NULL; with unfinished_host the call synchronises the stream). */
int lxo_decode_begin(const lxo_shape* s, const float* params, const void* wpack, void* ws, void* stream);
int lxo_decode_step(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int time,
                    int32_t* ids_out, int32_t* parents_out, int32_t* finished_host, int* unfinished_host, void* stream);
/* The AttentionState of the step-wise decode (attention_cell.py:8: AttentionState(cell_state = LSTMStateTuple(c, h), o)) as data:
 * the state that lxo_decode_step(time) / lxo_decode_cell_step(time) steps FROM (after lxo_decode_begin: time 0 = the initial state
 * of attention_cell.py:51-56; after a step at `time`: time + 1).  c, h f32 [B * beam][U], o f32 [B * beam][O], DEVICE pointers, any
 * may be NULL (skipped).  _set also takes ids_prev int32 [B * beam] = the tokens whose embeddings are the step's input
 * (greedy_decoder_cell.py:61: embedding_lookup(E, new_ids)); NULL leaves them.  With these a caller can run AttentionCell.step from
 * a state of its choosing, as the reference's cell allows (attention_cell.py:58: step(embedding, attn_cell_state)). */
int lxo_decode_state_get(const lxo_shape* s, void* ws, int time, float* c, float* h, float* o, void* stream);
int lxo_decode_state_set(const lxo_shape* s, void* ws, int time, const float* c, const float* h, const float* o,
                         const int32_t* ids_prev, void* stream);
/* AttentionCell.step alone (attention_cell.py:58-89): LSTM cell, attention context, o and logits projections for every decoder row,
 * from the state of `time` to the state of time + 1; logits f32 [B * beam][Vp] in ws region "dec_logits" (Vp = V rounded up to 32).
 * start_token != 0: the input is the learnt start token (greedy_decoder_cell.py:40-43), else the embeddings of the ids last set /
 * produced.  No arg-max, no finished flags, no beam bookkeeping: those belong to the decoder cells (lxo_decode_step). */
int lxo_decode_cell_step(const lxo_shape* s, const float* params, const void* wpack, void* ws, int time, int start_token, void* stream);
/* dynamic_decode + BeamSearchDecoderCell (beam_search_decoder_cell.py:98-250),
 * reference-faithful finalize (parents not followed): ids_out int32 [B, max_steps, beam],
 * parents_out same shape (may be NULL). */
int lxo_beam_decode(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                    int id_end, int max_iter, int32_t* ids_out, int32_t* parents_out,
                    int* steps_out, void* stream);
/* lxo_beam_decode that also exports the attention weights: alpha_out f32 [max_steps][B * beam][Rp] (device), Rp = (R+7)/8*8 --
 * entry [t][b * beam + j] = the weights decoder row j of image b attended with AT step t, i.e. of hypothesis slot j as it stood
 * BEFORE step t's top-k re-ordering: the rows the reference's tf.py_func tap sees on the merged batch x beam tensor when
 * config.decoding == "beam_search" (attention_mechanism.py:59-65,96-121; the shipped configs/model.json:13-14 decodes with beam 2).
 * The token ids_out[b][t][i] was read off row parents_out[b][t][i] of that step, so the map under which token i of step t was emitted is
 * alpha_out[t][b * beam + parents_out[b][t][i]] (time 0: every slot descends from row 0, whose k copies are identical). */
int lxo_beam_decode_attn(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                         int id_end, int max_iter, int32_t* ids_out, int32_t* parents_out, float* alpha_out,
                         int* steps_out, void* stream);
/* lxo_beam_decode(_attn) that also returns the running log-probs of the hypotheses (the beam state's log_probs,
 * beam_search_decoder_cell.py:146-187): scores_out f32 [B, max_steps, beam] (device, NOT NULL), scores_out[b][t][i] = the score with
 * which slot i was selected at step t = the log-prob of the token sequence that back-traces from (t, i) through parents_out.  The slots
 * of a step are in descending score order (top_k).  A finished hypothesis extends only with END at log-prob 0: its score is frozen.
 * With the diversity penalty on (div_gamma, div_prob) the scores include it, as the reference's state does.  Columns >= *steps_out
 * are unspecified.  alpha_out: as in lxo_beam_decode_attn, or NULL for none.  ids_out / parents_out are those of lxo_beam_decode. */
int lxo_beam_decode_scores(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                           int32_t* ids_out, int32_t* parents_out, float* scores_out, float* alpha_out, int* steps_out, void* stream);
/* Beam decode from a given prefix (prefix, prefix_ld, prefix_len per image, as in lxo_greedy_decode_prefix).  At a step t < P_b every slot j
 * of image b takes prefix[b][t] with parent j and its running log-prob grows by that id's log-prob (no diversity penalty): the k slots stay
 * identical.  Step P_b selects its top-k over slot 0 alone, as step 0 does without a prefix; later steps over all k V candidates.  The
 * diversity penalty's hash keeps the global step index.  scores_out (nullable): as in lxo_beam_decode_scores.  With every P_b = 0 the
 * outputs are those of lxo_beam_decode(_scores). */
int lxo_beam_decode_prefix(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                           const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                           int32_t* ids_out, int32_t* parents_out, float* scores_out, float* alpha_out, int* steps_out, void* stream);
/* Beam decode under a token constraint (allow / allow_ld as in lxo_greedy_decode_constrained: ONE ROW PER IMAGE, shared by its beam slots;
 * prefix as in lxo_beam_decode_prefix or all NULL / 0).  log_softmax runs over the allowed columns; a banned candidate (slot, token) scores
 * -inf and is never selected, also for a finished hypothesis (whose only live candidate stays END at 0); the diversity penalty ranks banned
 * columns last, so the rank of an allowed column is the number of allowed columns ahead of it, and its Bernoulli hash keeps the
 * (time, row, id, V) indexing.  Contract, beyond the greedy call's: every row allows at least `beam` tokens (the first free step selects k
 * candidates from slot 0 alone -- why beam > V is refused).  With every column allowed the outputs are those of lxo_beam_decode_prefix /
 * _scores. */
int lxo_beam_decode_constrained(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                                const uint32_t* allow, int allow_ld,
                                const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                                int32_t* ids_out, int32_t* parents_out, float* scores_out, float* alpha_out, int* steps_out, void* stream);

/* ---- decode under a DELIMITER GRAMMAR: hypotheses that close what they open ------------------------------------------------
 * A set that follows each decoder row's own history, on the device, inside the loop of the three decodes.  cls int8 [V] (device): 0 = a
 * plain token, +q = an opener of delimiter kind q, -q = a closer of kind q, 1 <= q <= n_kinds <= 15; many tokens may share a kind; id_end
 * must be class 0.  A row's state: a depth d in [0, D], D = max_depth <= LXO_GRAMMAR_MAX_DEPTH, and the stack of the d open kinds -- one
 * state per image (greedy), per hypothesis slot (beam), per draw (sampling).  With r = max_iter - t the steps that can still follow step t,
 * the grammar set G(state, t) of an unfinished row holds
 *   a closer of kind q   iff d > 0 and the top of the stack is q,
 *   id_end               iff d == 0,
 *   an opener            iff d < D and [budget] r >= d + 2,
 *   any other token      iff [budget] r >= d + 1,
 * the [budget] conditions only with `budget` != 0.  With the budget d <= r holds before every step, so a row always has room to close
 * everything and emit END by step max_iter; at r == d only the matching closer is left, or END at d == 0.  The effective set of step t is
 * S_t = A & G(state, t), A the static set of the row's image (allow, or everything); a finished row has S_t = A and a frozen state.
 * Everything the constrained calls do with A these calls do with S_t: arg-max, log-sum-exp, the beam's top-k and diversity rank, the
 * sampler's cut-offs and draw, the returned log-probs; forced prefix steps too.  After the select of step t emitted id in a row that is
 * still unfinished: an opener at d < D pushes its kind, a closer that matches the top pops, anything else (a mismatched closer, a closer at
 * depth 0, an opener at depth D) leaves the state as it is -- no content faults.  A beam slot continues the state of its PARENT slot.
 * Contract (checked by the caller, not by the device): A allows id_end and every closer; a prefix obeys the grammar at every forced step,
 * budget included; for beam, slot 0's effective set at the first free step holds at least `beam` tokens.  Then, with budget set, every row /
 * back-traced hypothesis / draw reaches END at or before step max_iter and its tokens up to that END are balanced and correctly nested. */
#define LXO_GRAMMAR_MAX_DEPTH 32
typedef struct lxo_grammar { const int8_t* cls; int n_kinds; int max_depth; int budget; } lxo_grammar;
/* bytes of the device scratch a grammar call needs for `rows` decoder rows (B, B * beam, B * n); 0: rows < 1 or V < 1.  Not part of ws. */
size_t lxo_grammar_scratch_bytes(int rows, int V);
/* lxo_greedy_decode_constrained / lxo_beam_decode_constrained / lxo_sample_decode under a grammar: their arguments (allow may be NULL with
 * allow_ld 0: everything) plus the grammar, depth_out (nullable: int32, laid out as ids_out, the depth of the row after each step) and scratch
 * (device, lxo_grammar_scratch_bytes of the call's decoder rows).  One small launch more per step; the greedy call runs the launch-per-step
 * path in both dtypes (the persistent chain holds no grammar).  -1, before any launch: NULL grammar / cls, n_kinds outside 1 .. 15,
 * max_depth outside 1 .. LXO_GRAMMAR_MAX_DEPTH, NULL scratch, and the set / prefix / option refusals of the calls they extend. */
int lxo_greedy_decode_grammar(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                              const uint32_t* allow, int allow_ld, const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                              const lxo_grammar* grammar, int32_t* ids_out, float* logp_out, float* alpha_out, int32_t* depth_out,
                              void* scratch, int* steps_out, void* stream);
int lxo_beam_decode_grammar(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                            const uint32_t* allow, int allow_ld, const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                            const lxo_grammar* grammar, int32_t* ids_out, int32_t* parents_out, float* scores_out, float* alpha_out,
                            int32_t* depth_out, void* scratch, int* steps_out, void* stream);
int lxo_sample_decode_grammar(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                              const lxo_sample_opts* opts, const uint32_t* allow, int allow_ld,
                              const int32_t* prefix, int prefix_ld, const int32_t* prefix_len, const lxo_grammar* grammar,
                              int32_t* ids_out, float* logp_out, float* logq_out, float* alpha_out, int32_t* depth_out, void* scratch,
                              int* steps_out, void* stream);
/* The grammar kernels alone, on ids the caller holds; the states live in scratch between calls.  rows decoder rows, rows_per_image of them
 * per image (1 .. 16, a divisor of rows); allow: one row per image.  ids == NULL: the set-up launch -- class sets, states cleared, S_0.
 * Else the step behind the select of step `time`: ids / finished int32 [rows] (device) as the select left them, parents (nullable) int32
 * [rows] = the slot inside the row's image whose state the row continues; the states before step `time` are those the previous call left
 * (set-up, or the step at time - 1).  Outputs (device, nullable): sets_out uint32 [rows][(V + 31) / 32] = S_0 / S_{time + 1} (pad bits 0),
 * depth_out int32 [rows] (step only).  -1: the grammar and set refusals above, ids without finished; -5: the shape refusals. */
int lxo_grammar_step(const lxo_grammar* grammar, int rows, int rows_per_image, int V, int id_end, const int32_t* ids, const int32_t* parents,
                     const int32_t* finished, int time, int max_iter, const uint32_t* allow, int allow_ld, uint32_t* sets_out,
                     int32_t* depth_out, void* scratch, void* stream);

/* ---- data parallel: one process per GPU, RCCL over xGMI -------------------------------------
 * The reference trains on one device (one sess.run per step, model/img2seq.py:169).  Samples are independent through encoder,
 * decoder and loss, so a data-parallel binding needs exactly two exchanges per step, both sums over ranks:
 *   (1) the number of unmasked tokens -- the loss is the mean over ALL tokens of the GLOBAL batch (img2seq.py:69-71); the summed
 *       count is what lxo_ce_loss_fwd_bwd_dev reads from device memory;
 *   (2) the gradients, in buckets as lxo_decoder_train_bwd_part / lxo_encoder_bwd(l, l) finalise them (y_W_o, the rest of the
 *       decoder, conv6 .. conv3, conv2 + conv1), on a side stream so that they overlap the rest of the backward.
 * RCCL (librccl.so) is bound with dlopen at the first lxo_comm_* call; nothing else in the library needs it.
 * Bootstrap: rank 0 calls lxo_comm_unique_id and ships the LXO_COMM_ID_BYTES bytes to the other ranks by any host channel
 * (a file, a TCP store, MPI); every rank then calls lxo_comm_init with ITS device current (hipSetDevice). */
#define LXO_COMM_ID_BYTES 128
int lxo_comm_unique_id(void* id_out /* host, LXO_COMM_ID_BYTES */);
int lxo_comm_init(const void* unique_id, int rank, int world, void** comm_out);
/* rank / world as the communicator reports them (ncclCommUserRank / ncclCommCount): what bench.py prints as rccl_ranks_seen */
int lxo_comm_info(void* comm, int* rank, int* world);
/* In-place sum over ranks of `count` elements (LXO_F32, LXO_BF16 or LXO_I32) at device pointer ptr, enqueued on side_stream
 * (a hipStream_t).  ready_event (a hipEvent_t, may be NULL): recorded by the caller on its compute stream behind the kernels
 * that finalised the bucket; the side stream waits for it before the collective.  A caller that orders buckets on the host
 * (hipEventSynchronize, then this call) passes NULL.  The caller makes its compute stream wait for side_stream before the
 * optimizer step.  Every rank must issue the same sequence of calls on a communicator. */
int lxo_allreduce_bucket(void* comm, void* ptr, long long count, int dtype, void* side_stream, void* ready_event);
int lxo_comm_destroy(void* comm);
const char* lxo_comm_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
