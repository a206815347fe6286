// extern "C" boundary of liblxo.so (see include/lxo.h).
#include "lxo.h"
#include "gemm.h"
#include "impl.h"
#include <stdio.h>
#include <string.h>

static thread_local char g_err[256] = "";
static int fail(int code, const char* what) {
    snprintf(g_err, sizeof(g_err), "%s (code %d)", what, code);
    return code < 0 ? code : -code;
}
#define CHECK_LAUNCH(expr, what) do { int rc_ = (expr); if (rc_ != 0) return fail(rc_, what); } while (0)

extern "C" const char* lxo_last_error(void) { return g_err; }
extern "C" int lxo_version(void) { return LXO_ABI_VERSION; }
extern "C" int lxo_shape_size(void) { return (int)sizeof(lxo_shape); }

extern "C" int lxo_gemm_nt(int dt, int a_f32, int c_f32, int small, const void* A, const void* Bp, void* C,
                           int M, int N, int K, int lda, int ldb, int ldc, const float* bias, int act,
                           float alpha, int accumulate, void* stream) {
    GemmNT p; memset(&p, 0, sizeof(p));
    p.A = A; p.Bp = Bp; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.bias = bias; p.act = act; p.alpha = alpha; p.accumulate = accumulate; p.addend_rows = 1;
    CHECK_LAUNCH(lxo_launch_gemm_nt(dt, a_f32, c_f32, small, p, (hipStream_t)stream), "lxo_gemm_nt");
    return 0;
}

extern "C" int lxo_gemm_tn(int dt, int a_f32, int b_f32, const void* A, const void* B, float* C,
                           int M, int I, int J, int lda, int ldb, int ldc, int nsplit, int atomic, void* stream) {
    GemmTN p; memset(&p, 0, sizeof(p));
    p.A = A; p.B = B; p.C = C; p.M = M; p.I = I; p.J = J; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.nsplit = nsplit; p.nbatch = 1; p.atomic = atomic;
    CHECK_LAUNCH(lxo_launch_gemm_tn(dt, a_f32, b_f32, p, (hipStream_t)stream), "lxo_gemm_tn");
    return 0;
}

// ---------------------------------------------------------------- plan ----
#define MAKE_PLAN(P, s) if (!(s)) return fail(-1, "null shape"); Plan P(*(s)); \
    { char m_[200]; int v_ = P.validate(m_, sizeof(m_)); if (v_) { snprintf(g_err, sizeof(g_err), "%s", m_); return v_; } }

extern "C" int lxo_param_num(void) { return P_COUNT; }
extern "C" const char* lxo_param_name_for(const lxo_shape* s, int id) { return lxo_param_name_mode(id, s ? s->encoder_cnn : 0); }
extern "C" long long lxo_param_total(const lxo_shape* s) { if (!s) return -1; Plan P(*s); return P.ptotal; }
extern "C" int lxo_param_info(const lxo_shape* s, int id, long long* offset, long long* count) {
    if (!s || id < 0 || id >= P_COUNT) return fail(-1, "lxo_param_info");
    Plan P(*s);
    if (offset) *offset = P.poff[id];
    if (count) *count = P.pcount[id];
    return 0;
}
extern "C" size_t lxo_wpack_bytes(const lxo_shape* s) { if (!s) return 0; Plan P(*s); return P.ktotal; }
extern "C" size_t lxo_workspace_bytes(const lxo_shape* s) { if (!s) return 0; Plan P(*s); return P.wtotal; }
extern "C" int lxo_ws_region(const lxo_shape* s, const char* name, size_t* offset, size_t* bytes) {
    if (!s || !name) return fail(-1, "lxo_ws_region");
    Plan P(*s);
    for (int i = 0; i < W_COUNT; ++i)
        if (strcmp(name, lxo_ws_name(i)) == 0) {
            if (offset) *offset = P.woff[i];
            if (bytes) *bytes = P.wbytes[i];
            return 0;
        }
    return fail(-1, "unknown workspace region");
}
extern "C" int lxo_ws_region_dtype(const lxo_shape* s, const char* name) {
    if (!s || !name) return fail(-1, "lxo_ws_region_dtype");
    const bool bf = s->dtype == LXO_BF16;
    static const char* const kCompute[] = {"p1", "y2", "p2", "y3", "y4", "p4", "y5", "p5", "y6", "img", "att_img", "emb_in", "dlogits",
                                           "d_att_img", "g0", "g1", "g2", "cols", "dec_emb", "dec_txe", "rxt"};
    static const char* const kBf16[] = {"recb", "gb", "dzb", "rhb", "rdzb", "att_exp", "datth_b"};
    static const char* const kI32[] = {"dec_ids", "dec_flags", "beam_par"};
    static const char* const kU8[] = {"m2", "m4", "m5"};
    for (const char* n : kCompute) if (strcmp(name, n) == 0) return bf ? LXO_BF16 : LXO_F32;
    for (const char* n : kBf16) if (strcmp(name, n) == 0) return LXO_BF16;
    for (const char* n : kI32) if (strcmp(name, n) == 0) return LXO_I32;
    for (const char* n : kU8) if (strcmp(name, n) == 0) return LXO_U8;
    // "d_img": the hand-over from the decoder backward to the encoder backward.  f32 mode: the f32 gradient w.r.t. the encoder
    // output; bf16 mode: d_y6 (that gradient with conv6's ReLU mask applied, bf16; conv6's bias gradient is already in grads)
    // -- and only where the decoder's last GEMM applies the mask (Plan::dimg_masked: bf16, E % 32 == 0, no row encoder); with the row
    // encoder, or an E the fused GEMM does not take, the region is the plain f32 gradient in bf16 mode too
    if (strcmp(name, "d_img") == 0) { Plan P(*s); return P.dimg_masked() ? LXO_BF16 : LXO_F32; }
    for (int i = 0; i < W_COUNT; ++i) if (strcmp(name, lxo_ws_name(i)) == 0) return LXO_F32;
    return fail(-1, "unknown workspace region");
}
extern "C" int lxo_pack_weights(const lxo_shape* s, const float* params, void* wpack, void* stream) {
    MAKE_PLAN(P, s);
    CHECK_LAUNCH(lxo_impl_pack_weights(P, params, wpack, (hipStream_t)stream), "lxo_pack_weights");
    return 0;
}
extern "C" int lxo_encoder_fwd(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                               const uint8_t* img, void* stream) {
    MAKE_PLAN(P, s);
    CHECK_LAUNCH(lxo_impl_encoder_fwd(P, params, wpack, ws, img, (hipStream_t)stream), "lxo_encoder_fwd");
    return 0;
}
extern "C" int lxo_encoder_bwd(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                               const uint8_t* img, float* grads, int last_layer, int first_layer, void* stream) {
    MAKE_PLAN(P, s);
    if (last_layer > 6 || first_layer < 1 || last_layer < first_layer) return fail(-1, "lxo_encoder_bwd: layer range");
    CHECK_LAUNCH(lxo_impl_encoder_bwd(P, params, wpack, ws, img, grads, last_layer, first_layer, (hipStream_t)stream), "lxo_encoder_bwd");
    return 0;
}
extern "C" int lxo_encoder_bwd_ready(const lxo_shape* s, const float* params, const void* wpack, void* ws, const uint8_t* img, float* grads,
                                     int last_layer, int first_layer, void* const* ready_events, void* stream) {
    MAKE_PLAN(P, s);
    if (last_layer > 6 || first_layer < 1 || last_layer < first_layer) return fail(-1, "lxo_encoder_bwd_ready: layer range");
    if (!ready_events) return fail(-1, "lxo_encoder_bwd_ready: null event table");
    CHECK_LAUNCH(lxo_impl_encoder_bwd(P, params, wpack, ws, img, grads, last_layer, first_layer, (hipStream_t)stream, ready_events), "lxo_encoder_bwd_ready");
    return 0;
}

#include "head_kernels.h"
extern "C" int lxo_decoder_train_fwd(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                                     const int32_t* formula, void* stream) {
    MAKE_PLAN(P, s);
    if (s->T <= 0) return fail(-1, "T must be positive");
    CHECK_LAUNCH(lxo_impl_decoder_train_fwd(P, params, wpack, ws, formula, (hipStream_t)stream), "lxo_decoder_train_fwd");
    return 0;
}
extern "C" int lxo_decoder_train_fwd_live(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                                          const int32_t* formula, const int32_t* lengths, void* stream) {
    MAKE_PLAN(P, s);
    if (s->T <= 0) return fail(-1, "T must be positive");
    CHECK_LAUNCH(lxo_impl_decoder_train_fwd(P, params, wpack, ws, formula, (hipStream_t)stream, lengths), "lxo_decoder_train_fwd_live");
    return 0;
}
extern "C" int lxo_ce_loss_fwd_bwd(const lxo_shape* s, void* ws, const int32_t* formula, const int32_t* lengths,
                                   float inv_ntok, void* stream) {
    MAKE_PLAN(P, s);
    CHECK_LAUNCH(lxo_impl_ce_loss(P, ws, formula, lengths, inv_ntok, nullptr, (hipStream_t)stream), "lxo_ce_loss_fwd_bwd");
    return 0;
}
extern "C" int lxo_ce_loss_fwd_bwd_dev(const lxo_shape* s, void* ws, const int32_t* formula, const int32_t* lengths,
                                       const float* ntok_dev, void* stream) {
    MAKE_PLAN(P, s);
    if (!ntok_dev) return fail(-1, "lxo_ce_loss_fwd_bwd_dev: null token count");
    CHECK_LAUNCH(lxo_impl_ce_loss(P, ws, formula, lengths, 0.f, ntok_dev, (hipStream_t)stream), "lxo_ce_loss_fwd_bwd_dev");
    return 0;
}
extern "C" int lxo_ce_loss_weighted(const lxo_shape* s, void* ws, const int32_t* formula, const int32_t* lengths, const float* w_tok, const float* w_row,
                                    float inv_norm, const float* norm_dev, void* stream) {
    MAKE_PLAN(P, s);
    if (!w_tok && !w_row) return fail(-1, "lxo_ce_loss_weighted: w_tok and w_row are both NULL (the unweighted loss is lxo_ce_loss_fwd_bwd)");
    CHECK_LAUNCH(lxo_impl_ce_loss(P, ws, formula, lengths, inv_norm, norm_dev, (hipStream_t)stream, w_tok, w_row), "lxo_ce_loss_weighted");
    return 0;
}
extern "C" int lxo_ce_loss_smoothed(const lxo_shape* s, void* ws, const int32_t* formula, const int32_t* lengths, float eps, const float* w_tok,
                                    const float* w_row, float inv_norm, const float* norm_dev, void* stream) {
    MAKE_PLAN(P, s);
    if (!ws || !formula || !lengths) return fail(-1, "lxo_ce_loss_smoothed: null ws, formula or lengths");
    if (!(eps - eps == 0.f) || !(eps >= 0.f && eps < 1.f)) return fail(-1, "lxo_ce_loss_smoothed: eps is not a finite number in [0, 1)");
    CHECK_LAUNCH(lxo_impl_ce_loss(P, ws, formula, lengths, inv_norm, norm_dev, (hipStream_t)stream, w_tok, w_row, &eps), "lxo_ce_loss_smoothed");
    return 0;
}
extern "C" int lxo_ce_loss_soft(const lxo_shape* s, void* ws, const int32_t* formula, const int32_t* lengths, float eps, float lambda, int k,
                                const int32_t* soft_ids, const float* soft_p, const float* w_tok, const float* w_row, float inv_norm, const float* norm_dev,
                                void* stream) {
    MAKE_PLAN(P, s);
    if (!ws || !formula || !lengths) return fail(-1, "lxo_ce_loss_soft: null ws, formula or lengths");
    if (!soft_ids || !soft_p) return fail(-1, "lxo_ce_loss_soft: null soft_ids or soft_p");
    if (k < 1 || k > 16) return fail(-1, "lxo_ce_loss_soft: k outside 1 .. 16");
    if (!(eps - eps == 0.f) || !(eps >= 0.f && eps < 1.f)) return fail(-1, "lxo_ce_loss_soft: eps is not a finite number in [0, 1)");
    if (!(lambda - lambda == 0.f) || !(lambda >= 0.f && lambda <= 1.f)) return fail(-1, "lxo_ce_loss_soft: lambda is not a finite number in [0, 1]");
    const CeSoft soft = {soft_ids, soft_p, k, lambda};
    CHECK_LAUNCH(lxo_impl_ce_loss(P, ws, formula, lengths, inv_norm, norm_dev, (hipStream_t)stream, w_tok, w_row, &eps, &soft), "lxo_ce_loss_soft");
    return 0;
}
extern "C" int lxo_mrt_weights(const float* seq_logp, const float* cost, const int32_t* group_off, int G, int rows, float alpha,
                               float* w_out, float* q_out, float* risk_out, void* stream) {
    if (!w_out || !seq_logp || !cost || !group_off) return fail(-1, "lxo_mrt_weights: null w_out, seq_logp, cost or group_off");
    if (G < 0 || rows < 0) return fail(-1, "lxo_mrt_weights: G < 0 or rows < 0");
    if (!(alpha - alpha == 0.f)) return fail(-1, "lxo_mrt_weights: alpha is not finite");
    CHECK_LAUNCH(lxo_k_mrt_weights(seq_logp, cost, group_off, G, rows, alpha, w_out, q_out, risk_out, (hipStream_t)stream), "lxo_mrt_weights");
    return 0;
}
#include "seqcost.h"
#include "attloc.h"
#include "beamfin.h"
static_assert(LXO_EDIT_MAX_REF == kEditMaxRef, "include/lxo.h and csrc/seqcost.h disagree on the reference limit");
extern "C" int lxo_edit_distance(const int32_t* hyp, int hyp_block, long long hyp_block_stride, long long hyp_row_stride, long long hyp_tok_stride, int T,
                                 const int32_t* hyp_len, const int32_t* ref, int G, int ref_ld, const int32_t* ref_len, const int32_t* ref_of,
                                 int per_ref, int pairs, int id_end, int32_t* dist_out, float* cost_out, void* stream) {
    if (!hyp || !ref || !dist_out) return fail(-1, "lxo_edit_distance: null hyp, ref or dist_out");
    if (pairs < 0 || T < 0 || G < 0 || hyp_block_stride < 0 || hyp_row_stride < 0 || hyp_tok_stride < 0)
        return fail(-1, "lxo_edit_distance: a negative count or stride");
    if (hyp_block < 1 || per_ref < 1 || (pairs > 0 && G < 1)) return fail(-1, "lxo_edit_distance: hyp_block < 1, per_ref < 1 or no reference row");
    if (ref_ld < 1 || ref_ld > LXO_EDIT_MAX_REF) return fail(-1, "lxo_edit_distance: ref_ld outside 1 .. LXO_EDIT_MAX_REF (a reference longer than the kernel's column limit)");
    const EditArgs a = {hyp, hyp_len, ref, ref_len, ref_of, nullptr, dist_out, cost_out, hyp_block_stride, hyp_row_stride, hyp_tok_stride,
                        hyp_block, T, G, ref_ld, per_ref, pairs, id_end};
    CHECK_LAUNCH(lxo_k_edit_distance(a, (hipStream_t)stream), "lxo_edit_distance");
    return 0;
}
static_assert(LXO_TEXT_STATS == kTextStats && LXO_TEXT_CORPUS == kTextCorpus, "include/lxo.h and csrc/seqcost.h disagree on the text-metric rows");
extern "C" int lxo_text_stats(const int32_t* hyp, int hyp_block, long long hyp_block_stride, long long hyp_row_stride, long long hyp_tok_stride, int T,
                              const int32_t* hyp_len, const int32_t* ref, int G, int ref_ld, const int32_t* ref_len, const int32_t* ref_of, int per_ref,
                              int pairs, int id_end, int32_t* stats_out, long long* corpus_io, int accumulate, void* stream) {
    if (!hyp || !ref) return fail(-1, "lxo_text_stats: null hyp or ref");
    if (!stats_out && !corpus_io) return fail(-1, "lxo_text_stats: stats_out and corpus_io are both NULL");
    if (pairs < 0 || T < 0 || G < 0 || hyp_block_stride < 0 || hyp_row_stride < 0 || hyp_tok_stride < 0)
        return fail(-1, "lxo_text_stats: a negative count or stride");
    if (hyp_block < 1 || per_ref < 1 || (pairs > 0 && G < 1)) return fail(-1, "lxo_text_stats: hyp_block < 1, per_ref < 1 or no reference row");
    if (T > LXO_EDIT_MAX_REF) return fail(-1, "lxo_text_stats: T outside 0 .. LXO_EDIT_MAX_REF (a hypothesis wider than the kernel's staging limit)");
    if (ref_ld < 1 || ref_ld > LXO_EDIT_MAX_REF) return fail(-1, "lxo_text_stats: ref_ld outside 1 .. LXO_EDIT_MAX_REF (a reference longer than the kernel's column limit)");
    if (accumulate != 0 && accumulate != 1) return fail(-1, "lxo_text_stats: accumulate must be 0 or 1");
    const TextArgs a = {hyp, hyp_len, ref, ref_len, ref_of, stats_out, corpus_io, hyp_block_stride, hyp_row_stride, hyp_tok_stride,
                        hyp_block, T, G, ref_ld, per_ref, pairs, id_end, accumulate};
    CHECK_LAUNCH(lxo_k_text_stats(a, (hipStream_t)stream), "lxo_text_stats");
    return 0;
}
static_assert(LXO_ALIGN_COUNTS == kAlignCounts && LXO_ALIGN_CORPUS == kAlignCorpus, "include/lxo.h and csrc/seqcost.h disagree on the alignment rows");
extern "C" size_t lxo_edit_align_scratch_bytes(int pairs, int T, int ref_ld) { return lxo_k_edit_align_scratch_bytes(pairs, T, ref_ld); }
extern "C" int lxo_edit_align(const int32_t* hyp, int hyp_block, long long hyp_block_stride, long long hyp_row_stride, long long hyp_tok_stride, int T,
                              const int32_t* hyp_len, const int32_t* ref, int G, int ref_ld, const int32_t* ref_len, const int32_t* ref_of, int per_ref,
                              int pairs, int id_end, int32_t* hyp_align, int32_t* ref_align, int32_t* counts_out, long long* corpus_io,
                              long long* confusion_io, int V, int accumulate, void* scratch, size_t scratch_bytes, void* stream) {
    if (!hyp || !ref) return fail(-1, "lxo_edit_align: null hyp or ref");
    if (!hyp_align && !ref_align && !counts_out && !corpus_io && !confusion_io) return fail(-1, "lxo_edit_align: the five outputs are all NULL");
    if (pairs < 0 || T < 0 || G < 0 || hyp_block_stride < 0 || hyp_row_stride < 0 || hyp_tok_stride < 0)
        return fail(-1, "lxo_edit_align: a negative count or stride");
    if (hyp_block < 1 || per_ref < 1 || (pairs > 0 && G < 1)) return fail(-1, "lxo_edit_align: hyp_block < 1, per_ref < 1 or no reference row");
    if (T > LXO_EDIT_MAX_REF) return fail(-1, "lxo_edit_align: T outside 0 .. LXO_EDIT_MAX_REF (a hypothesis wider than the kernel's staging limit)");
    if (ref_ld < 1 || ref_ld > LXO_EDIT_MAX_REF) return fail(-1, "lxo_edit_align: ref_ld outside 1 .. LXO_EDIT_MAX_REF (a reference longer than the kernel's column limit)");
    if (accumulate != 0 && accumulate != 1) return fail(-1, "lxo_edit_align: accumulate must be 0 or 1");
    if (confusion_io && V < 1) return fail(-1, "lxo_edit_align: a confusion matrix needs V >= 1");
    if (pairs > 0 && T > 0 && (!scratch || scratch_bytes < lxo_k_edit_align_scratch_bytes(pairs, T, ref_ld)))
        return fail(-1, "lxo_edit_align: scratch is NULL or smaller than lxo_edit_align_scratch_bytes");
    const AlignArgs a = {hyp, hyp_len, ref, ref_len, ref_of, hyp_align, ref_align, counts_out, corpus_io, confusion_io, static_cast<unsigned*>(scratch),
                         hyp_block_stride, hyp_row_stride, hyp_tok_stride, hyp_block, T, G, ref_ld, per_ref, pairs, id_end, confusion_io ? V : 1, accumulate};
    CHECK_LAUNCH(lxo_k_edit_align(a, (hipStream_t)stream), "lxo_edit_align");
    return 0;
}
static_assert(LXO_LOCATE_STATS == kLocateStats && LXO_LOCATE_MAX_CELLS == kLocateMaxCells, "include/lxo.h and csrc/attloc.h disagree on the location rows");
extern "C" int lxo_attention_locate(const float* alpha, long long step_stride, long long row_stride, int alpha_rows, int Hp, int Wp, int rows, int steps,
                                    const int32_t* len, const int32_t* src, float mass, int32_t* peak_out, int32_t* box_out, float* stats_out,
                                    float* coverage_out, int cov_ld, void* stream) {
    if (!alpha) return fail(-1, "lxo_attention_locate: null alpha");
    if (!peak_out && !box_out && !stats_out && !coverage_out) return fail(-1, "lxo_attention_locate: the four outputs are all NULL");
    if (!(mass > 0.f && mass <= 1.f)) return fail(-1, "lxo_attention_locate: mass outside (0, 1]");
    if (step_stride < 0 || row_stride < 0 || alpha_rows < 0 || rows < 0 || steps < 0) return fail(-1, "lxo_attention_locate: a negative count or stride");
    if (Hp < 1 || Wp < 1) return fail(-5, "lxo_attention_locate: Hp or Wp < 1");
    if ((long long)Hp * Wp > LXO_LOCATE_MAX_CELLS) return fail(-5, "lxo_attention_locate: Hp * Wp above LXO_LOCATE_MAX_CELLS (a map larger than the kernel's staging limit)");
    if (coverage_out && cov_ld < Hp * Wp) return fail(-1, "lxo_attention_locate: cov_ld < Hp * Wp");
    if ((long long)rows * steps > 0x7fffffffll - 4 || (long long)rows * ((Hp * Wp + 255) / 256) > 0x7fffffffll)
        return fail(-5, "lxo_attention_locate: more positions than a grid holds");
    const LocateArgs a = {alpha, len, src, peak_out, box_out, stats_out, coverage_out, step_stride, row_stride, alpha_rows, Hp, Wp, rows, steps, cov_ld, mass};
    CHECK_LAUNCH(lxo_k_attention_locate(a, (hipStream_t)stream), "lxo_attention_locate");
    return 0;
}
static_assert(LXO_BLEU_COUNTS == kBleuCounts, "include/lxo.h and csrc/seqcost.h disagree on the sentence-BLEU counts");
extern "C" int lxo_sentence_bleu(const int32_t* hyp, int hyp_block, long long hyp_block_stride, long long hyp_row_stride, long long hyp_tok_stride, int T,
                                 const int32_t* hyp_len, const int32_t* ref, int G, int ref_ld, const int32_t* ref_len, const int32_t* ref_of, int per_ref,
                                 int pairs, int id_end, int32_t* counts_out, float* bleu_out, float* cost_out, void* stream) {
    if (!hyp || !ref) return fail(-1, "lxo_sentence_bleu: null hyp or ref");
    if (!counts_out && !bleu_out && !cost_out) return fail(-1, "lxo_sentence_bleu: counts_out, bleu_out and cost_out are all NULL");
    if (pairs < 0 || T < 0 || G < 0 || hyp_block_stride < 0 || hyp_row_stride < 0 || hyp_tok_stride < 0)
        return fail(-1, "lxo_sentence_bleu: a negative count or stride");
    if (hyp_block < 1 || per_ref < 1 || (pairs > 0 && G < 1)) return fail(-1, "lxo_sentence_bleu: hyp_block < 1, per_ref < 1 or no reference row");
    if (T > LXO_EDIT_MAX_REF) return fail(-1, "lxo_sentence_bleu: T outside 0 .. LXO_EDIT_MAX_REF (a hypothesis wider than the kernel's staging limit)");
    if (ref_ld < 1 || ref_ld > LXO_EDIT_MAX_REF) return fail(-1, "lxo_sentence_bleu: ref_ld outside 1 .. LXO_EDIT_MAX_REF (a reference wider than the kernel's staging limit)");
    const BleuArgs a = {hyp, hyp_len, ref, ref_len, ref_of, nullptr, counts_out, bleu_out, cost_out, hyp_block_stride, hyp_row_stride, hyp_tok_stride,
                        hyp_block, T, G, ref_ld, per_ref, pairs, id_end};
    CHECK_LAUNCH(lxo_k_sentence_bleu(a, (hipStream_t)stream), "lxo_sentence_bleu");
    return 0;
}
extern "C" int lxo_mrt_candidates_cost(const int32_t* ids, int B, int max_steps, int n, int steps, const int32_t* ref, int Tr, const int32_t* ref_len,
                                       int id_end, int id_pad, int include_reference, int32_t* cand, int32_t* cand_len, float* cost, int32_t* group_off,
                                       int32_t* row_image, int cost_kind, void* stream) {
    if (!ids || !ref || !ref_len || !cand || !cand_len || !cost || !group_off || !row_image) return fail(-1, "lxo_mrt_candidates: a null argument");
    if (B < 0 || n < 1 || n > 16 || max_steps < 0 || steps < 0 || steps > max_steps) return fail(-1, "lxo_mrt_candidates: B < 0, n outside 1 .. 16 or steps outside [0, max_steps]");
    if (Tr < 1 || Tr > LXO_EDIT_MAX_REF) return fail(-1, "lxo_mrt_candidates: Tr outside 1 .. LXO_EDIT_MAX_REF");
    if (id_end < 0) return fail(-1, "lxo_mrt_candidates: id_end < 0");
    if (cost_kind != LXO_COST_EDIT && cost_kind != LXO_COST_BLEU) return fail(-1, "lxo_mrt_candidates_cost: cost_kind is neither LXO_COST_EDIT nor LXO_COST_BLEU");
    if (cost_kind == LXO_COST_BLEU && steps + 1 > LXO_EDIT_MAX_REF)
        return fail(-1, "lxo_mrt_candidates_cost: with LXO_COST_BLEU steps + 1 must not exceed LXO_EDIT_MAX_REF (rows wider than the kernel's staging limit)");
    const CandArgs a = {ids, ref, ref_len, cand, cand_len, cost, group_off, row_image, B, max_steps, n, steps, Tr, id_end, id_pad, include_reference ? 1 : 0};
    CHECK_LAUNCH(lxo_k_mrt_candidates(a, (hipStream_t)stream, cost_kind), "lxo_mrt_candidates");
    return 0;
}
extern "C" int lxo_mrt_candidates(const int32_t* ids, int B, int max_steps, int n, int steps, const int32_t* ref, int Tr, const int32_t* ref_len,
                                  int id_end, int id_pad, int include_reference, int32_t* cand, int32_t* cand_len, float* cost, int32_t* group_off,
                                  int32_t* row_image, void* stream) {
    return lxo_mrt_candidates_cost(ids, B, max_steps, n, steps, ref, Tr, ref_len, id_end, id_pad, include_reference, cand, cand_len, cost, group_off, row_image,
                                   LXO_COST_EDIT, stream);
}
static_assert(LXO_CONSENSUS_MAX_N == kConsensusMaxN, "include/lxo.h and csrc/seqcost.h disagree on the number of draws");
extern "C" int lxo_consensus(const int32_t* ids, long long image_stride, long long draw_stride, long long tok_stride, int B, int n, int T, int id_end,
                             const float* weights, int normalize, int32_t* dist_out, float* risk_out, int32_t* best_out, void* stream) {
    if (!ids || !dist_out || !risk_out || !best_out) return fail(-1, "lxo_consensus: null ids, dist_out, risk_out or best_out");
    if (B < 0 || image_stride < 0 || draw_stride < 0 || tok_stride < 0) return fail(-1, "lxo_consensus: B or a stride negative");
    if (n < 1 || n > LXO_CONSENSUS_MAX_N) return fail(-1, "lxo_consensus: n outside 1 .. LXO_CONSENSUS_MAX_N");
    if (T < 0 || T > LXO_EDIT_MAX_REF) return fail(-1, "lxo_consensus: T outside 0 .. LXO_EDIT_MAX_REF (draws longer than the kernel's column limit)");
    if (normalize != 0 && normalize != 1) return fail(-1, "lxo_consensus: normalize must be 0 or 1");
    if ((long long)B * n * (n - 1) / 2 > 0x7ffffff0ll) return fail(-1, "lxo_consensus: B n (n - 1) / 2 pairs exceed one launch");
    const ConsArgs a = {ids, weights, dist_out, risk_out, best_out, image_stride, draw_stride, tok_stride, B, n, T, id_end, normalize};
    CHECK_LAUNCH(lxo_k_consensus(a, (hipStream_t)stream), "lxo_consensus");
    return 0;
}
extern "C" int lxo_consensus_bleu(const int32_t* ids, long long image_stride, long long draw_stride, long long tok_stride, int B, int n, int T, int id_end,
                                  const float* weights, int32_t* match_out, float* cost_out, float* risk_out, int32_t* best_out, void* stream) {
    if (!ids || !cost_out || !risk_out || !best_out) return fail(-1, "lxo_consensus_bleu: null ids, cost_out, risk_out or best_out");
    if (B < 0 || image_stride < 0 || draw_stride < 0 || tok_stride < 0) return fail(-1, "lxo_consensus_bleu: B or a stride negative");
    if (n < 1 || n > LXO_CONSENSUS_MAX_N) return fail(-1, "lxo_consensus_bleu: n outside 1 .. LXO_CONSENSUS_MAX_N");
    if (T < 0 || T > LXO_EDIT_MAX_REF) return fail(-1, "lxo_consensus_bleu: T outside 0 .. LXO_EDIT_MAX_REF (draws wider than the kernel's staging limit)");
    if ((long long)B * n * (n - 1) / 2 > 0x7ffffff0ll) return fail(-1, "lxo_consensus_bleu: B n (n - 1) / 2 pairs exceed one launch");
    const ConsBleuArgs a = {ids, weights, match_out, cost_out, risk_out, best_out, image_stride, draw_stride, tok_stride, B, n, T, id_end};
    CHECK_LAUNCH(lxo_k_consensus_bleu(a, (hipStream_t)stream), "lxo_consensus_bleu");
    return 0;
}
static_assert(LXO_BEAM_MAX_K == kBeamFinMaxK && LXO_BEAM_MAX_STEPS == kBeamFinMaxSteps, "include/lxo.h and csrc/beamfin.h disagree on the beam limits");
extern "C" int lxo_beam_finalize(const int32_t* ids, const int32_t* parents, const float* scores, int B, int ld_t, int steps, int k, int id_end,
                                 int32_t* hyp_out, int32_t* len_out, int32_t* src_out, float* tok_logp_out, float* seq_logp_out, void* stream) {
    if (!ids || !parents) return fail(-1, "lxo_beam_finalize: null ids or parents");
    if (!hyp_out && !len_out && !src_out && !tok_logp_out && !seq_logp_out) return fail(-1, "lxo_beam_finalize: the five outputs are all NULL");
    if ((tok_logp_out || seq_logp_out) && !scores) return fail(-1, "lxo_beam_finalize: tok_logp_out or seq_logp_out without scores");
    if (B < 0 || id_end < 0) return fail(-1, "lxo_beam_finalize: B or id_end negative");
    if (k < 1 || k > LXO_BEAM_MAX_K) return fail(-5, "lxo_beam_finalize: k outside 1 .. LXO_BEAM_MAX_K");
    if (steps < 1 || steps > LXO_BEAM_MAX_STEPS) return fail(-5, "lxo_beam_finalize: steps outside 1 .. LXO_BEAM_MAX_STEPS (the kernel's LDS stage)");
    if (ld_t < steps) return fail(-1, "lxo_beam_finalize: ld_t < steps");
    if ((long long)B * k > 0x7fffffffll) return fail(-1, "lxo_beam_finalize: B * k above 2^31 - 1");
    const BeamFinArgs a = {ids, parents, scores, hyp_out, len_out, src_out, tok_logp_out, seq_logp_out, B, ld_t, steps, k, id_end};
    CHECK_LAUNCH(lxo_k_beam_finalize(a, (hipStream_t)stream), "lxo_beam_finalize");
    return 0;
}
extern "C" int lxo_beam_rerank(const int32_t* len, const float* seq_logp, const float* coverage, int cov_ld, int R, int B, int k, float alpha, float beta,
                               float cov_floor, float* score_out, float* post_out, int32_t* order_out, void* stream) {
    if (!len || !seq_logp) return fail(-1, "lxo_beam_rerank: null len or seq_logp");
    if (!score_out && !post_out && !order_out) return fail(-1, "lxo_beam_rerank: the three outputs are all NULL");
    if (B < 0) return fail(-1, "lxo_beam_rerank: B negative");
    if (k < 1 || k > LXO_BEAM_MAX_K) return fail(-5, "lxo_beam_rerank: k outside 1 .. LXO_BEAM_MAX_K");
    if ((long long)B * k > 0x7fffffffll) return fail(-1, "lxo_beam_rerank: B * k above 2^31 - 1");
    if (!(alpha >= 0.f && __builtin_isfinite(alpha)) || !(beta >= 0.f && __builtin_isfinite(beta))) return fail(-1, "lxo_beam_rerank: alpha or beta negative or not finite");
    if (!(cov_floor > 0.f && cov_floor <= 1.f)) return fail(-1, "lxo_beam_rerank: cov_floor outside (0, 1]");
    if (coverage && (R < 0 || cov_ld < R)) return fail(-1, "lxo_beam_rerank: R < 0 or cov_ld < R");
    const BeamRerankArgs a = {len, seq_logp, coverage, score_out, post_out, order_out, B, k, coverage ? R : 0, cov_ld, alpha, beta, cov_floor};
    CHECK_LAUNCH(lxo_k_beam_rerank(a, (hipStream_t)stream), "lxo_beam_rerank");
    return 0;
}
extern "C" int lxo_score_tokens(const lxo_shape* s, void* ws, const int32_t* formula, const int32_t* lengths,
                                float* logp_out, int32_t* top1_out, float* seq_out, void* stream) {
    MAKE_PLAN(P, s);
    if (s->T <= 0) return fail(-1, "T must be positive");
    if (!ws || !formula || !lengths) return fail(-1, "lxo_score_tokens: null workspace, formula or lengths");
    if (!logp_out) return fail(-1, "lxo_score_tokens: null logp_out");
    CHECK_LAUNCH(lxo_impl_score_tokens(P, ws, formula, lengths, logp_out, top1_out, seq_out, (hipStream_t)stream), "lxo_score_tokens");
    return 0;
}
extern "C" int lxo_score_alternatives(const lxo_shape* s, void* ws, const int32_t* formula, const int32_t* lengths, int k,
                                      const uint32_t* allow, int allow_ld, int32_t* ids_out, float* logp_out,
                                      int32_t* rank_out, float* entropy_out, void* stream) {
    MAKE_PLAN(P, s);
    if (s->T <= 0) return fail(-1, "T must be positive");
    if (!ws || !formula || !lengths) return fail(-1, "lxo_score_alternatives: null workspace, formula or lengths");
    if (!ids_out) return fail(-1, "lxo_score_alternatives: null ids_out");
    if (!logp_out) return fail(-1, "lxo_score_alternatives: null logp_out");
    if (k < 1 || k > 16 || k > P.s.V) return fail(-1, "lxo_score_alternatives: k outside 1 .. min(16, V)");
    if (allow && (allow_ld < 0 || (allow_ld != 0 && allow_ld < (P.s.V + 31) / 32))) return fail(-1, "lxo_score_alternatives: allow_ld must be 0 or >= (V + 31) / 32");
    if (!allow && allow_ld != 0) return fail(-1, "lxo_score_alternatives: null allow with allow_ld != 0");
    const DecAllow al = {allow, allow_ld};
    CHECK_LAUNCH(lxo_impl_score_alternatives(P, ws, formula, lengths, k, allow ? &al : nullptr, ids_out, logp_out, rank_out, entropy_out, (hipStream_t)stream),
                 "lxo_score_alternatives");
    return 0;
}
extern "C" int lxo_decoder_train_bwd(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                                     const int32_t* formula, float* grads, void* stream) {
    MAKE_PLAN(P, s);
    CHECK_LAUNCH(lxo_impl_decoder_train_bwd(P, params, wpack, ws, formula, grads, 3, (hipStream_t)stream), "lxo_decoder_train_bwd");
    return 0;
}
extern "C" int lxo_train_bwd(const lxo_shape* s, const float* params, const void* wpack, void* ws, const int32_t* formula, const uint8_t* img,
                            float* grads, void* const* ready_events, void* stream) {
    MAKE_PLAN(P, s);
    CHECK_LAUNCH(lxo_impl_decoder_train_bwd(P, params, wpack, ws, formula, grads, 3, (hipStream_t)stream, true, ready_events ? ready_events[0] : nullptr),
                 "lxo_train_bwd (decoder)");
    CHECK_LAUNCH(lxo_impl_encoder_bwd(P, params, wpack, ws, img, grads, 6, 1, (hipStream_t)stream, ready_events), "lxo_train_bwd (encoder)");
    return 0;
}
extern "C" int lxo_decoder_train_bwd_part(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                                          const int32_t* formula, float* grads, int parts, void* stream) {
    MAKE_PLAN(P, s);
    if (parts < 1 || parts > 3) return fail(-1, "lxo_decoder_train_bwd_part: parts must be 1, 2 or 3");
    CHECK_LAUNCH(lxo_impl_decoder_train_bwd(P, params, wpack, ws, formula, grads, parts, (hipStream_t)stream), "lxo_decoder_train_bwd_part");
    return 0;
}
extern "C" int lxo_global_norm_scale(long long n, const float* grads, float clip, float* scale_out, void* stream) {
    // scale_out: LXO_GNORM_FLOATS floats = {scale, norm, up to 1024 per-workgroup partial sums (added in order: no atomics)}
    CHECK_LAUNCH(lxo_k_global_norm_scale(n, grads, clip, scale_out + 2, scale_out, (hipStream_t)stream), "lxo_global_norm_scale");
    return 0;
}
extern "C" int lxo_adam_step(long long n, float* params, const float* grads, float* m, float* v,
                             float lr_t, float beta1, float beta2, float eps, const float* scale_dev, void* stream) {
    CHECK_LAUNCH(lxo_k_adam(params, grads, m, v, n, lr_t, beta1, beta2, eps, scale_dev, (hipStream_t)stream), "lxo_adam_step");
    return 0;
}
// The whole-loop decodes: one implementation per kind; the entry points differ in which outputs they take (impl.h: DecodeOuts) and demand
extern "C" int lxo_greedy_decode(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                                 int id_end, int max_iter, int32_t* ids_out, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    const DecodeOuts o = {ids_out, nullptr, nullptr, nullptr, nullptr};
    CHECK_LAUNCH(lxo_impl_greedy_decode(P, params, wpack, ws, id_end, max_iter, o, steps_out, (hipStream_t)stream), "lxo_greedy_decode");
    return 0;
}
extern "C" int lxo_greedy_decode_attn(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                                      int id_end, int max_iter, int32_t* ids_out, float* alpha_out, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    const DecodeOuts o = {ids_out, nullptr, nullptr, alpha_out, nullptr};
    CHECK_LAUNCH(lxo_impl_greedy_decode(P, params, wpack, ws, id_end, max_iter, o, steps_out, (hipStream_t)stream), "lxo_greedy_decode_attn");
    return 0;
}
extern "C" int lxo_greedy_decode_scores(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                                        int32_t* ids_out, float* logp_out, float* alpha_out, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    if (!logp_out) return fail(-1, "lxo_greedy_decode_scores: null logp_out");
    const DecodeOuts o = {ids_out, nullptr, logp_out, alpha_out, nullptr};
    CHECK_LAUNCH(lxo_impl_greedy_decode(P, params, wpack, ws, id_end, max_iter, o, steps_out, (hipStream_t)stream), "lxo_greedy_decode_scores");
    return 0;
}
// the forced prefix of the _prefix calls (head_kernels.h); false: an array is missing or prefix_ld < 1
static bool make_prefix(DecPrefix* pf, const int32_t* prefix, int prefix_ld, const int32_t* prefix_len, int max_iter) {
    *pf = DecPrefix{prefix, prefix_len, prefix_ld, prefix_ld < max_iter ? prefix_ld : max_iter};
    return prefix && prefix_len && prefix_ld >= 1;
}
extern "C" int lxo_greedy_decode_prefix(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                                        const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                                        int32_t* ids_out, float* logp_out, float* alpha_out, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    DecPrefix pf;
    if (!make_prefix(&pf, prefix, prefix_ld, prefix_len, max_iter)) return fail(-1, "lxo_greedy_decode_prefix: null prefix / prefix_len or prefix_ld < 1");
    const DecodeOuts o = {ids_out, nullptr, logp_out, alpha_out, &pf};
    CHECK_LAUNCH(lxo_impl_greedy_decode(P, params, wpack, ws, id_end, max_iter, o, steps_out, (hipStream_t)stream), "lxo_greedy_decode_prefix");
    return 0;
}
// the _constrained calls' sets (head_kernels.h) and optional prefix; what is refused, or null
static const char* make_constraint(DecAllow* al, DecPrefix* pf, bool* has_prefix, int V, const uint32_t* allow, int allow_ld,
                                   const int32_t* prefix, int prefix_ld, const int32_t* prefix_len, int max_iter) {
    *al = DecAllow{allow, allow_ld};
    if (!allow || allow_ld < 0 || (allow_ld != 0 && allow_ld < (V + 31) / 32)) return "lxo_*_decode_constrained: null allow or 0 < allow_ld < (V + 31) / 32";
    *has_prefix = prefix || prefix_len || prefix_ld != 0;
    if (*has_prefix && !make_prefix(pf, prefix, prefix_ld, prefix_len, max_iter)) return "lxo_*_decode_constrained: a prefix needs prefix, prefix_len and prefix_ld >= 1 (none: all NULL / 0)";
    return nullptr;
}
extern "C" int lxo_greedy_decode_constrained(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                                             const uint32_t* allow, int allow_ld, const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                                             int32_t* ids_out, float* logp_out, float* alpha_out, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    DecAllow al; DecPrefix pf; bool has_prefix = false;
    if (const char* why = make_constraint(&al, &pf, &has_prefix, P.s.V, allow, allow_ld, prefix, prefix_ld, prefix_len, max_iter))
        return fail(-1, why);
    const DecodeOuts o = {ids_out, nullptr, logp_out, alpha_out, has_prefix ? &pf : nullptr, &al};
    CHECK_LAUNCH(lxo_impl_greedy_decode(P, params, wpack, ws, id_end, max_iter, o, steps_out, (hipStream_t)stream), "lxo_greedy_decode_constrained");
    return 0;
}
// lxo_sample_opts as the kernels take it (head_kernels.h: DecSample); what is refused, or null
static const char* make_sample(DecSample* so, const lxo_sample_opts* opts) {
    if (!opts) return "lxo_sample_*: null opts";
    if (!(opts->temperature > 0.f) || opts->temperature > 3.0e38f || !(1.0f / opts->temperature <= 3.0e38f))      // a subnormal tau: 1 / tau overflows
        return "lxo_sample_*: temperature and 1 / temperature must be positive and finite";
    if (opts->top_k < 0) return "lxo_sample_*: top_k < 0";
    if (!(opts->top_p > 0.f && opts->top_p <= 1.f)) return "lxo_sample_*: top_p outside (0, 1]";
    *so = DecSample{1.0f / opts->temperature, opts->top_k, opts->top_p, opts->seed, 1, 0};
    return nullptr;
}
extern "C" int lxo_sample_decode(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                                 const lxo_sample_opts* opts, const uint32_t* allow, int allow_ld,
                                 const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                                 int32_t* ids_out, float* logp_out, float* logq_out, float* alpha_out, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    DecSample so; DecAllow al; DecPrefix pf; bool has_prefix = false;
    if (const char* why = make_sample(&so, opts)) return fail(-1, why);
    if (!ids_out) return fail(-1, "lxo_sample_decode: null ids_out");
    if (!allow && allow_ld != 0) return fail(-1, "lxo_sample_decode: null allow with allow_ld != 0");
    if (allow) {
        if (const char* why = make_constraint(&al, &pf, &has_prefix, P.s.V, allow, allow_ld, prefix, prefix_ld, prefix_len, max_iter)) return fail(-1, why);
    } else {
        has_prefix = prefix || prefix_len || prefix_ld != 0;
        if (has_prefix && !make_prefix(&pf, prefix, prefix_ld, prefix_len, max_iter)) return fail(-1, "lxo_sample_decode: a prefix needs prefix, prefix_len and prefix_ld >= 1 (none: all NULL / 0)");
    }
    const DecodeOuts o = {ids_out, nullptr, logp_out, alpha_out, has_prefix ? &pf : nullptr, allow ? &al : nullptr};
    CHECK_LAUNCH(lxo_impl_sample_decode(P, params, wpack, ws, id_end, max_iter, so, o, logq_out, steps_out, (hipStream_t)stream), "lxo_sample_decode");
    return 0;
}
extern "C" int lxo_sample_tokens(const float* logits, int ld, int rows, int n, int V, int time, const lxo_sample_opts* opts,
                                 const uint32_t* allow, int allow_ld, int32_t* ids_out, float* logp_out, float* logq_out, void* stream) {
    DecSample so;
    if (const char* why = make_sample(&so, opts)) return fail(-1, why);
    if (!logits || !ids_out) return fail(-1, "lxo_sample_tokens: null logits or ids_out");
    if (V < 1 || ld < V || rows < 1 || n < 1 || n > 16 || time < 0) return fail(-5, "lxo_sample_tokens: V < 1, ld < V, rows < 1, n outside 1 .. 16 or time < 0");
    if (!allow && allow_ld != 0) return fail(-1, "lxo_sample_tokens: null allow with allow_ld != 0");
    if (allow && (allow_ld < 0 || (allow_ld != 0 && allow_ld < (V + 31) / 32))) return fail(-1, "lxo_sample_tokens: allow_ld must be 0 or >= (V + 31) / 32");
    const DecAllow al = {allow, allow_ld};
    CHECK_LAUNCH(lxo_k_sample(logits, ld, V, rows, n, -1, time, so, nullptr, ids_out, logp_out, logq_out, 1, 0, nullptr, nullptr, (hipStream_t)stream,
                              nullptr, allow ? &al : nullptr), "lxo_sample_tokens");
    return 0;
}
extern "C" int lxo_decode_begin(const lxo_shape* s, const float* params, const void* wpack, void* ws, void* stream) {
    MAKE_PLAN(P, s);
    CHECK_LAUNCH(lxo_impl_decode_begin(P, params, wpack, ws, (hipStream_t)stream), "lxo_decode_begin");
    return 0;
}
extern "C" int lxo_decode_step(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int time,
                               int32_t* ids_out, int32_t* parents_out, int32_t* finished_host, int* unfinished_host, void* stream) {
    MAKE_PLAN(P, s);
    CHECK_LAUNCH(lxo_impl_decode_step(P, params, wpack, ws, id_end, time, ids_out, parents_out, finished_host, unfinished_host, (hipStream_t)stream),
                 "lxo_decode_step");
    return 0;
}
extern "C" int lxo_beam_decode(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                               int id_end, int max_iter, int32_t* ids_out, int32_t* parents_out, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    const DecodeOuts o = {ids_out, parents_out, nullptr, nullptr, nullptr};
    CHECK_LAUNCH(lxo_impl_beam_decode(P, params, wpack, ws, id_end, max_iter, o, steps_out, (hipStream_t)stream), "lxo_beam_decode");
    return 0;
}
extern "C" int lxo_beam_decode_attn(const lxo_shape* s, const float* params, const void* wpack, void* ws,
                                    int id_end, int max_iter, int32_t* ids_out, int32_t* parents_out, float* alpha_out, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    if (!alpha_out) return fail(-1, "lxo_beam_decode_attn: null alpha_out");
    const DecodeOuts o = {ids_out, parents_out, nullptr, alpha_out, nullptr};
    CHECK_LAUNCH(lxo_impl_beam_decode(P, params, wpack, ws, id_end, max_iter, o, steps_out, (hipStream_t)stream), "lxo_beam_decode_attn");
    return 0;
}
extern "C" int lxo_beam_decode_scores(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                                      int32_t* ids_out, int32_t* parents_out, float* scores_out, float* alpha_out, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    if (!scores_out) return fail(-1, "lxo_beam_decode_scores: null scores_out");
    const DecodeOuts o = {ids_out, parents_out, scores_out, alpha_out, nullptr};
    CHECK_LAUNCH(lxo_impl_beam_decode(P, params, wpack, ws, id_end, max_iter, o, steps_out, (hipStream_t)stream), "lxo_beam_decode_scores");
    return 0;
}
extern "C" int lxo_beam_decode_prefix(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                                      const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                                      int32_t* ids_out, int32_t* parents_out, float* scores_out, float* alpha_out, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    DecPrefix pf;
    if (!make_prefix(&pf, prefix, prefix_ld, prefix_len, max_iter)) return fail(-1, "lxo_beam_decode_prefix: null prefix / prefix_len or prefix_ld < 1");
    const DecodeOuts o = {ids_out, parents_out, scores_out, alpha_out, &pf};
    CHECK_LAUNCH(lxo_impl_beam_decode(P, params, wpack, ws, id_end, max_iter, o, steps_out, (hipStream_t)stream), "lxo_beam_decode_prefix");
    return 0;
}
extern "C" int lxo_beam_decode_constrained(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                                           const uint32_t* allow, int allow_ld, const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                                           int32_t* ids_out, int32_t* parents_out, float* scores_out, float* alpha_out, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    DecAllow al; DecPrefix pf; bool has_prefix = false;
    if (const char* why = make_constraint(&al, &pf, &has_prefix, P.s.V, allow, allow_ld, prefix, prefix_ld, prefix_len, max_iter))
        return fail(-1, why);
    const DecodeOuts o = {ids_out, parents_out, scores_out, alpha_out, has_prefix ? &pf : nullptr, &al};
    CHECK_LAUNCH(lxo_impl_beam_decode(P, params, wpack, ws, id_end, max_iter, o, steps_out, (hipStream_t)stream), "lxo_beam_decode_constrained");
    return 0;
}

// ---- decode under a delimiter grammar (grammar.h) ----
#include "grammar.h"
// the grammar of the _grammar calls and their optional static sets and prefix; what is refused, or null
static const char* make_grammar(DecGrammar* dg, const lxo_grammar* g, int32_t* depth_out, void* scratch) {
    if (!g || !g->cls) return "lxo_*_grammar: null grammar or cls";
    if (g->n_kinds < 1 || g->n_kinds > kGrammarMaxKinds) return "lxo_*_grammar: n_kinds outside 1 .. 15";
    if (g->max_depth < 1 || g->max_depth > LXO_GRAMMAR_MAX_DEPTH) return "lxo_*_grammar: max_depth outside 1 .. LXO_GRAMMAR_MAX_DEPTH";
    if (!scratch) return "lxo_*_grammar: null scratch";
    *dg = DecGrammar{g->cls, g->n_kinds, g->max_depth, g->budget ? 1 : 0, (unsigned*)scratch, depth_out};
    return nullptr;
}
static const char* make_grammar_constraint(DecAllow* al, DecPrefix* pf, bool* has_prefix, int V, const uint32_t* allow, int allow_ld,
                                           const int32_t* prefix, int prefix_ld, const int32_t* prefix_len, int max_iter) {
    if (!allow && allow_ld != 0) return "lxo_*_grammar: null allow with allow_ld != 0";
    if (allow) return make_constraint(al, pf, has_prefix, V, allow, allow_ld, prefix, prefix_ld, prefix_len, max_iter);
    *has_prefix = prefix || prefix_len || prefix_ld != 0;
    if (*has_prefix && !make_prefix(pf, prefix, prefix_ld, prefix_len, max_iter)) return "lxo_*_grammar: a prefix needs prefix, prefix_len and prefix_ld >= 1 (none: all NULL / 0)";
    return nullptr;
}
extern "C" size_t lxo_grammar_scratch_bytes(int rows, int V) {
    if (rows < 1 || V < 1) return 0;
    return (size_t)lxo_k_grammar_scratch_words(rows, V) * sizeof(unsigned);
}
extern "C" int lxo_greedy_decode_grammar(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                                         const uint32_t* allow, int allow_ld, const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                                         const lxo_grammar* grammar, int32_t* ids_out, float* logp_out, float* alpha_out, int32_t* depth_out,
                                         void* scratch, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    DecAllow al; DecPrefix pf; DecGrammar dg; bool has_prefix = false;
    if (const char* why = make_grammar(&dg, grammar, depth_out, scratch)) return fail(-1, why);
    if (const char* why = make_grammar_constraint(&al, &pf, &has_prefix, P.s.V, allow, allow_ld, prefix, prefix_ld, prefix_len, max_iter)) return fail(-1, why);
    const DecodeOuts o = {ids_out, nullptr, logp_out, alpha_out, has_prefix ? &pf : nullptr, allow ? &al : nullptr, &dg};
    CHECK_LAUNCH(lxo_impl_greedy_decode(P, params, wpack, ws, id_end, max_iter, o, steps_out, (hipStream_t)stream), "lxo_greedy_decode_grammar");
    return 0;
}
extern "C" int lxo_beam_decode_grammar(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                                       const uint32_t* allow, int allow_ld, const int32_t* prefix, int prefix_ld, const int32_t* prefix_len,
                                       const lxo_grammar* grammar, int32_t* ids_out, int32_t* parents_out, float* scores_out, float* alpha_out,
                                       int32_t* depth_out, void* scratch, int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    DecAllow al; DecPrefix pf; DecGrammar dg; bool has_prefix = false;
    if (const char* why = make_grammar(&dg, grammar, depth_out, scratch)) return fail(-1, why);
    if (const char* why = make_grammar_constraint(&al, &pf, &has_prefix, P.s.V, allow, allow_ld, prefix, prefix_ld, prefix_len, max_iter)) return fail(-1, why);
    const DecodeOuts o = {ids_out, parents_out, scores_out, alpha_out, has_prefix ? &pf : nullptr, allow ? &al : nullptr, &dg};
    CHECK_LAUNCH(lxo_impl_beam_decode(P, params, wpack, ws, id_end, max_iter, o, steps_out, (hipStream_t)stream), "lxo_beam_decode_grammar");
    return 0;
}
extern "C" int lxo_sample_decode_grammar(const lxo_shape* s, const float* params, const void* wpack, void* ws, int id_end, int max_iter,
                                         const lxo_sample_opts* opts, const uint32_t* allow, int allow_ld,
                                         const int32_t* prefix, int prefix_ld, const int32_t* prefix_len, const lxo_grammar* grammar,
                                         int32_t* ids_out, float* logp_out, float* logq_out, float* alpha_out, int32_t* depth_out, void* scratch,
                                         int* steps_out, void* stream) {
    MAKE_PLAN(P, s);
    DecSample so; DecAllow al; DecPrefix pf; DecGrammar dg; bool has_prefix = false;
    if (const char* why = make_sample(&so, opts)) return fail(-1, why);
    if (!ids_out) return fail(-1, "lxo_sample_decode_grammar: null ids_out");
    if (const char* why = make_grammar(&dg, grammar, depth_out, scratch)) return fail(-1, why);
    if (const char* why = make_grammar_constraint(&al, &pf, &has_prefix, P.s.V, allow, allow_ld, prefix, prefix_ld, prefix_len, max_iter)) return fail(-1, why);
    const DecodeOuts o = {ids_out, nullptr, logp_out, alpha_out, has_prefix ? &pf : nullptr, allow ? &al : nullptr, &dg};
    CHECK_LAUNCH(lxo_impl_sample_decode(P, params, wpack, ws, id_end, max_iter, so, o, logq_out, steps_out, (hipStream_t)stream), "lxo_sample_decode_grammar");
    return 0;
}
extern "C" int lxo_grammar_step(const lxo_grammar* grammar, int rows, int rows_per_image, int V, int id_end, const int32_t* ids,
                                const int32_t* parents, const int32_t* finished, int time, int max_iter, const uint32_t* allow, int allow_ld,
                                uint32_t* sets_out, int32_t* depth_out, void* scratch, void* stream) {
    DecGrammar dg;
    if (const char* why = make_grammar(&dg, grammar, depth_out, scratch)) return fail(-1, why);
    if (V < 1 || rows < 1 || rows_per_image < 1 || rows_per_image > 16 || rows % rows_per_image != 0 || time < 0 || max_iter < 0)
        return fail(-5, "lxo_grammar_step: V < 1, rows < 1, rows_per_image outside 1 .. 16 or no divisor of rows, time < 0 or max_iter < 0");
    if (!allow && allow_ld != 0) return fail(-1, "lxo_grammar_step: null allow with allow_ld != 0");
    if (allow && (allow_ld < 0 || (allow_ld != 0 && allow_ld < (V + 31) / 32))) return fail(-1, "lxo_grammar_step: allow_ld must be 0 or >= (V + 31) / 32");
    if (ids && !finished) return fail(-1, "lxo_grammar_step: ids without finished");
    const GrammarArgs a = {dg.cls, dg.n_kinds, dg.max_depth, dg.budget, allow, allow_ld, dg.scratch, rows, rows_per_image, V, id_end, max_iter};
    hipStream_t st = (hipStream_t)stream;
    if (!ids) CHECK_LAUNCH(lxo_k_grammar_setup(a, st), "lxo_grammar_step");
    else CHECK_LAUNCH(lxo_k_grammar_step(a, ids, parents, finished, time, depth_out, 1, 0, st), "lxo_grammar_step");
    if (sets_out)
        CHECK_LAUNCH((int)hipMemcpyAsync(sets_out, lxo_k_grammar_sets(a), (size_t)rows * ((V + 31) / 32) * sizeof(unsigned), hipMemcpyDeviceToDevice, st),
                     "lxo_grammar_step");
    return 0;
}

extern "C" int lxo_conv3x3(int dt, const void* in, const void* wpk, const float* bias, void* out, int B, int H, int W,
                           int Cin, int Ho, int Wo, int Cout, int pad, int relu, void* stream) {
    GemmNT g; memset(&g, 0, sizeof(g));
    g.A = in; g.Bp = wpk; g.C = out; g.conv = 1; g.H = H; g.W = W; g.Cin = Cin; g.Ho = Ho; g.Wo = Wo; g.pad = pad;
    g.M = B * Ho * Wo; g.N = Cout; g.K = 9 * Cin; g.lda = Cin; g.ldb = 9 * Cin; g.ldc = Cout;
    g.bias = bias; g.act = relu ? 1 : 0; g.alpha = 1.f; g.addend_rows = 1;
    CHECK_LAUNCH(lxo_launch_gemm_nt(dt, 0, 0, 0, g, (hipStream_t)stream), "lxo_conv3x3");
    return 0;
}
extern "C" int lxo_conv3x3_ex(int dt, const void* in, const void* wpk, const float* bias, void* out, int B, int H, int W,
                              int Cin, int Ho, int Wo, int Cout, int pad, int relu, const float* addend, int addend_rows,
                              void* out_pre, const void* relu_ref, float* colsum, void* stream) {
    GemmNT g; memset(&g, 0, sizeof(g));
    g.A = in; g.Bp = wpk; g.C = out; g.conv = 1; g.H = H; g.W = W; g.Cin = Cin; g.Ho = Ho; g.Wo = Wo; g.pad = pad;
    g.M = B * Ho * Wo; g.N = Cout; g.K = 9 * Cin; g.lda = Cin; g.ldb = 9 * Cin; g.ldc = Cout;
    g.bias = bias; g.act = relu ? 1 : 0; g.alpha = 1.f;
    g.addend = addend; g.addend_rows = addend_rows > 0 ? addend_rows : 1; g.out_pre = out_pre;
    g.relu_ref = relu_ref; g.ldr = Cout; g.colsum = colsum;
    CHECK_LAUNCH(lxo_launch_gemm_nt(dt, 0, 0, 0, g, (hipStream_t)stream), "lxo_conv3x3_ex");
    return 0;
}
extern "C" int lxo_attention_fwd(int dt, const void* att_img, const void* img, const float* att_h, const float* beta,
                                 float* alpha, float* part, float* ctx, int ldctx, int nv, int R, int E, int C, int beam,
                                 void* stream) {
    int nch = (512 + nv - 1) / nv; if (nch > 16) nch = 16;
    const int by_rows = R / 32 > 0 ? R / 32 : 1; if (nch > by_rows) nch = by_rows;
    const int need = (R + 1023) / 1024; if (nch < need) nch = need;
    Slabs none = {nullptr, 0, 0, 0};
    CHECK_LAUNCH(lxo_k_attn_fwd(dt, att_img, img, att_h, none, nullptr, beta, alpha, part, ctx, ldctx, nullptr, 0, nv, R, (R + 7) / 8 * 8, E, C, beam < 1 ? 1 : beam,
                                nch, 0, (hipStream_t)stream), "lxo_attention_fwd");
    return 0;
}

// test / micro-benchmark entry: split-K slab GEMM (see gemm.hip)
extern "C" int lxo_gemm_slab(int dt, const void* A, const void* Bp, float* slab, int M, int N, int K, int lda, int ldb, int ldc,
                             long long slab_stride, void* stream) {
    GemmNT p; memset(&p, 0, sizeof(p));
    p.A = A; p.Bp = Bp; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.alpha = 1.f; p.addend_rows = 1;
    CHECK_LAUNCH(lxo_launch_gemm_slab(dt, p, slab, slab_stride, (hipStream_t)stream), "lxo_gemm_slab");
    return 0;
}

extern "C" int lxo_conv3x3_wgrad(int dt, const void* in, const void* dout, float* dw, int B, int H, int W,
                                 int Cin, int Ho, int Wo, int Cout, int pad, void* stream) {
    GemmTN g; memset(&g, 0, sizeof(g));
    g.A = in; g.B = dout; g.C = dw; g.conv = 1; g.H = H; g.W = W; g.Cin = Cin; g.Ho = Ho; g.Wo = Wo; g.pad = pad;
    g.M = B * Ho * Wo; g.I = 9 * Cin; g.J = Cout; g.lda = Cin; g.ldb = Cout; g.ldc = Cout;
    const int tiles = cdiv(g.I, 128) * cdiv(g.J, 128);
    int ns = cdiv(1024, tiles); const int maxs = g.M / 256 > 0 ? g.M / 256 : 1; if (ns > maxs) ns = maxs;
    g.nsplit = ns < 1 ? 1 : ns; g.nbatch = 1; g.atomic = 1;
    CHECK_LAUNCH(lxo_launch_gemm_tn(dt, 0, 0, g, (hipStream_t)stream), "lxo_conv3x3_wgrad");
    return 0;
}

extern "C" int lxo_chain_guard(const lxo_shape* s, void* ws, const float* grads, float* scale_io, int have_scale, uint32_t* status_out, void* stream) {
    MAKE_PLAN(P, s);
    if (!ws || !scale_io) return fail(-1, "lxo_chain_guard: null workspace / scale");
    CHECK_LAUNCH(lxo_impl_chain_guard(P, ws, grads, scale_io, have_scale, status_out, (hipStream_t)stream), "lxo_chain_guard");
    return 0;
}
extern "C" int lxo_decode_state_get(const lxo_shape* s, void* ws, int time, float* c, float* h, float* o, void* stream) {
    MAKE_PLAN(P, s);
    if (time < 0) return fail(-5, "lxo_decode_state_get: time < 0");
    CHECK_LAUNCH(lxo_impl_decode_state_get(P, ws, time, c, h, o, (hipStream_t)stream), "lxo_decode_state_get");
    return 0;
}
extern "C" int lxo_decode_state_set(const lxo_shape* s, void* ws, int time, const float* c, const float* h, const float* o,
                                    const int32_t* ids_prev, void* stream) {
    MAKE_PLAN(P, s);
    if (time < 0) return fail(-5, "lxo_decode_state_set: time < 0");
    CHECK_LAUNCH(lxo_impl_decode_state_set(P, ws, time, c, h, o, ids_prev, (hipStream_t)stream), "lxo_decode_state_set");
    return 0;
}
extern "C" int lxo_decode_cell_step(const lxo_shape* s, const float* params, const void* wpack, void* ws, int time, int start_token, void* stream) {
    MAKE_PLAN(P, s);
    CHECK_LAUNCH(lxo_impl_decode_cell_step(P, params, wpack, ws, time, start_token, (hipStream_t)stream), "lxo_decode_cell_step");
    return 0;
}

extern "C" int lxo_set_side_stream(void* stream) {
    CHECK_LAUNCH(lxo_impl_set_side_stream((hipStream_t)stream), "lxo_set_side_stream");
    return 0;
}
extern "C" int lxo_set_encoder_side_stream(void* stream) {
    CHECK_LAUNCH(lxo_impl_set_encoder_side_stream((hipStream_t)stream), "lxo_set_encoder_side_stream");
    return 0;
}

extern "C" int lxo_optimizer_step(int method, long long n, float* params, const float* grads, float* slot, float lr,
                                  const float* scale_dev, void* stream) {
    CHECK_LAUNCH(lxo_k_simple_opt(params, grads, slot, n, lr, method, scale_dev, (hipStream_t)stream), "lxo_optimizer_step");
    return 0;
}
