// Internal entry points behind the C ABI (one per extern "C" function of lxo.h).
#pragma once
#include "plan.h"
struct DecPrefix;                     // head_kernels.h
struct DecAllow;
struct DecSample;
struct CeSoft;
const char* lxo_ws_name(int id);
int lxo_impl_pack_weights(const Plan& P, const float* prm, void* wp, hipStream_t st);
int lxo_impl_encoder_fwd(const Plan& P, const float* prm, const void* wp, void* ws, const uint8_t* img, hipStream_t st);
int lxo_impl_encoder_bwd(const Plan& P, const float* prm, const void* wp, void* ws, const uint8_t* img, float* grads,
                         int last_layer, int first_layer, hipStream_t st, void* const* ready = nullptr);
int lxo_impl_decoder_train_fwd(const Plan& P, const float* prm, const void* wp, void* ws, const int* formula, hipStream_t st, const int* lengths = nullptr);
int lxo_impl_ce_loss(const Plan& P, void* ws, const int* formula, const int* lengths, float inv_ntok, const float* ntok_dev, hipStream_t st,
                     const float* w_tok = nullptr, const float* w_row = nullptr, const float* smooth_eps = nullptr,
                     const CeSoft* soft = nullptr);
int lxo_impl_score_tokens(const Plan& P, void* ws, const int* formula, const int* lengths, float* logp_out, int* top1_out, float* seq_out, hipStream_t st);
int lxo_impl_score_alternatives(const Plan& P, void* ws, const int* formula, const int* lengths, int k, const DecAllow* allow, int* ids_out, float* logp_out,
                                int* rank_out, float* ent_out, hipStream_t st);
// parts: bit 0 = d_o from the logits + d y_W_o (final before the recurrence runs), bit 1 = BPTT + every other decoder gradient + d_img
int lxo_impl_decoder_train_bwd(const Plan& P, const float* prm, const void* wp, void* ws, const int* formula, float* grads, int parts, hipStream_t st,
                               bool defer_join = false, void* ready = nullptr);
// Where a whole-loop decode writes and what it is forced to emit (device arrays; all but ids nullable): scores = the token log-probs
// (greedy) / the running log-probs (beam), alpha = the attention maps, prefix = forced ids, allow = the images' allowed-token sets (head_kernels.h).  Greedy has no parents.
// grammar (nullable, the _grammar calls): the delimiter grammar of the call, its scratch and where the depths go (depth laid out as ids).  Under a
// grammar `allow` stays the images' STATIC sets; the select kernels read the per-row sets the grammar kernel leaves in the scratch (grammar.h)
struct DecGrammar { const signed char* cls; int n_kinds, max_depth, budget; unsigned* scratch; int* depth; };
struct DecodeOuts { int* ids; int* parents; float* scores; float* alpha; const DecPrefix* prefix; const DecAllow* allow; const DecGrammar* grammar; };
int lxo_impl_greedy_decode(const Plan& P, const float* prm, const void* wp, void* ws, int id_end, int max_iter, const DecodeOuts& out, int* steps_out, hipStream_t st);
int lxo_impl_decode_begin(const Plan& P, const float* prm, const void* wp, void* ws, hipStream_t st);
int lxo_impl_decode_step(const Plan& P, const float* prm, const void* wp, void* ws, int id_end, int time, int* ids_out, int* parents_out, int* finished_out, int* unfinished_host, hipStream_t st);
int lxo_impl_chain_guard(const Plan& P, void* ws, const float* grads, float* scale, int have_scale, unsigned* status, hipStream_t st);
int lxo_impl_decode_state_get(const Plan& P, void* ws, int time, float* c, float* h, float* o, hipStream_t st);
int lxo_impl_decode_state_set(const Plan& P, void* ws, int time, const float* c, const float* h, const float* o, const int* ids_prev, hipStream_t st);
int lxo_impl_decode_cell_step(const Plan& P, const float* prm, const void* wp, void* ws, int time, int start_token, hipStream_t st);
int lxo_impl_beam_decode(const Plan& P, const float* prm, const void* wp, void* ws, int id_end, int max_iter, const DecodeOuts& out, int* steps_out, hipStream_t st);
// n = s.beam independent draws per image; out.scores = the tokens' log-probs under the model, logq_out (nullable) under the sampled distribution
int lxo_impl_sample_decode(const Plan& P, const float* prm, const void* wp, void* ws, int id_end, int max_iter, const DecSample& opts, const DecodeOuts& out,
                           float* logq_out, int* steps_out, hipStream_t st);
int lxo_impl_set_side_stream(hipStream_t s);
int lxo_impl_set_encoder_side_stream(hipStream_t s);
// optional row-BiLSTM encoder (model_rowenc.hip): features in ws region "img" in place; backward: "d_img" (f32) in place + parameter gradients
int lxo_impl_rowenc_fwd(const Plan& P, const float* prm, const void* wp, void* ws, hipStream_t st);
int lxo_impl_rowenc_bwd(const Plan& P, const float* prm, const void* wp, void* ws, float* grads, hipStream_t st);
