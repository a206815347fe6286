// Launchers of the output head (head_kernels.hip): loss, teacher-forced scoring, greedy and beam token selection.
#pragma once
#include "decoder_kernels.h"
// ntok_dev (nullable): device scalar holding the global token count; when set the kernel uses 1 / *ntok_dev instead of inv_ntok
int lxo_k_ce_loss(int dt, const float* logits, const int* formula, const int* lengths, void* dlogits, float* loss_acc, float inv_ntok,
                  const float* ntok_dev, const unsigned* chain_err, int B, int T, int V, int Vp, DetScratch det, hipStream_t st);      // chain_err (nullable): error word of the persistent decoder chain; non-zero poisons the loss (NaN)
// teacher-forced scoring: logp_out [B][T] (logits[t * B + b][formula[b][t]] - lse), top1_out [B][T] (nullable), seq_out [B] (nullable, ordered f32
// sum); rows t >= lengths[b]: 0 / -1; chain_err set: NaN / -1.  Reads the logits only.
int lxo_k_score(int dt, const float* logits, const int* formula, const int* lengths, float* logp_out, int* top1_out, float* seq_out,
                const unsigned* chain_err, int B, int T, int V, int Vp, hipStream_t st);
// A forced decode prefix (lxo_greedy_decode_prefix / lxo_beam_decode_prefix), device arrays: row (greedy) or image (beam) r emits ids[r][t] at
// steps t < len[r]; lim = min(ld, max_iter) bounds a length (head_kernels.hip: how out-of-range values are read)
struct DecPrefix { const int* ids; const int* len; int ld; int lim; };
// Allowed-token sets (lxo_greedy_decode_constrained / lxo_beam_decode_constrained), device bit sets: bit v & 31 of word v >> 5 of row b set = image b
// may emit token v; ld words per row, 0 = one row shared by every image.  A banned column is read as a column outside the vocabulary
struct DecAllow { const unsigned* bits; int ld; };
// alternatives per position of the same logits: ids_out / logp_out [B][T][k] = the k first columns of row t * B + b (value descending, then column
// ascending) and logits[id] - lse, rank_out [B][T] (nullable) = the columns in front of the clamped target, ent_out [B][T] (nullable) = sum p (lse - x);
// allow (nullable): one row per sample b, everything then runs over its allowed columns (banned target: rank -1; no column left: -1 / -inf);
// rows t >= lengths[b]: -1 / 0 / -1 / 0; chain_err set: -1 / NaN / -1 / NaN.  1 <= k <= min(16, V), else -2.  Reads the logits only.
int lxo_k_score_alt(int dt, const float* logits, const int* formula, const int* lengths, int k, const DecAllow* allow, int* ids_out, float* logp_out,
                    int* rank_out, float* ent_out, const unsigned* chain_err, int B, int T, int V, int Vp, hipStream_t st);
int lxo_k_argmax(const float* logits, int Vp, int V, int n, int id_end, int* ids_step, int* ids_out, int max_steps, int step,
                 int* finished, int* n_unfinished, hipStream_t st, float* logp_out = nullptr,      // logp_out (nullable): [n][max_steps] log-prob of the id
                 const DecPrefix* prefix = nullptr, const DecAllow* allow = nullptr);
int lxo_k_beam_step(float* logits, int Vp, int V, int nimg, int k, int id_end, int time, float div_gamma, float div_prob, int div_seed,
                    float* scratch, float* logp, int* finished,
                    int* ids_step, int* parents_step, int* ids_out, int* par_out, int max_steps, int* n_unfinished, hipStream_t st,
                    float* scores_out = nullptr,      // scores_out (nullable): [nimg][max_steps][k] the running log-probs after the step
                    const DecPrefix* prefix = nullptr, const DecAllow* allow = nullptr);      // allow: one row per IMAGE
