// Launchers of the output head (head_kernels.hip): loss, teacher-forced scoring, greedy and beam token selection.
#pragma once
#include "decoder_kernels.h"
// ntok_dev (nullable): device scalar holding the global token count; when set the kernel uses 1 / *ntok_dev instead of inv_ntok
// weights (nullable, lxo_ce_loss_weighted): device f32 tok [B][T] and row [B], either nullable -- token (b, t) weighs tok[b][t] * row[b] (a NULL factor is 1, any
// sign); d(logits) of a live row is scaled by w * inv_ntok and loss_acc = {sum w CE, token count, sum w, sum CE}: four statistics per slot of `det`
// (512 x 4 floats, else -2).  Without weights: {sum CE, token count} and the kernels of before
struct CeWeights { const float* tok; const float* row; };
// smooth (nullable, lxo_ce_loss_smoothed): the target of a live row is q_j = (1 - eps) [j == y] + eps / V over [0, V), eps_v = eps / (float)V.  d(logits) is
// (p_j - q_j) * scale -- the target column subtracts (1.f - eps) + eps_v, every other eps_v -- and the row's loss (1 - eps) CE + eps (lse - sum_{j < V} x_j / V);
// the statistics are the four, {sum w L, token count, sum w, sum CE (plain)}, with or without weights (without: w = 1.f), through `det` as above
struct CeSmooth { float eps, eps_v; };
// soft (nullable, lxo_ce_loss_soft; include/lxo.h holds the definition): device ids / p [B][T][k], 1 <= k <= 16 (else -2), lxo_k_score_alt's layout -- slot i of a
// live row counts iff 0 <= ids[i] < V and then carries the mass p[i]; Sigma = their sum in ascending i, rest = max(0, 1 - Sigma) is spread over [0, V),
// tau_j = sum_{ids_i == j} p_i (ascending i) + rest / V, and the row's target is (1 - lambda) * (the smoothed target) + lambda * tau; a row with Sigma == 0 has no
// teacher and is lxo_ce_loss_smoothed's row.  d(logits) is (S p_j - q_j) * scale with S = sum_j q_j.  Needs `smooth` (eps may be 0); the four statistics as above
struct CeSoft { const int* ids; const float* p; int k; float lambda; };
int lxo_k_ce_loss(int dt, const float* logits, const int* formula, const int* lengths, void* dlogits, float* loss_acc, float inv_ntok,
                  const float* ntok_dev, const unsigned* chain_err, int B, int T, int V, int Vp, DetScratch det, hipStream_t st,      // chain_err (nullable): error word of the persistent decoder chain; non-zero poisons the loss (NaN)
                  const CeWeights* weights = nullptr, const CeSmooth* smooth = nullptr, const CeSoft* soft = nullptr);
// minimum-risk weights of candidate rows grouped by image (rows group_off[g] .. group_off[g + 1] - 1, G groups): Q = softmax(alpha seq_logp) over a group,
// R_g = sum Q cost, w_out = alpha Q (R_g - cost), q_out (nullable) = Q, risk_out (nullable) [1] = sum_g R_g added in ascending g; rows behind the last group: 0.
// Offsets are clamped into [0, rows] on the device.  No atomics: the same bytes in every run
int lxo_k_mrt_weights(const float* seq_logp, const float* cost, const int* group_off, int G, int rows, float alpha, float* w_out, float* q_out,
                      float* risk_out, hipStream_t st);
// teacher-forced scoring: logp_out [B][T] (logits[t * B + b][formula[b][t]] - lse), top1_out [B][T] (nullable), seq_out [B] (nullable, ordered f32
// sum); rows t >= lengths[b]: 0 / -1; chain_err set: NaN / -1.  Reads the logits only.
int lxo_k_score(int dt, const float* logits, const int* formula, const int* lengths, float* logp_out, int* top1_out, float* seq_out,
                const unsigned* chain_err, int B, int T, int V, int Vp, hipStream_t st);
// A forced decode prefix (lxo_greedy_decode_prefix / lxo_beam_decode_prefix), device arrays: row (greedy) or image (beam) r emits ids[r][t] at
// steps t < len[r]; lim = min(ld, max_iter) bounds a length (head_kernels.hip: how out-of-range values are read)
struct DecPrefix { const int* ids; const int* len; int ld; int lim; };
// Allowed-token sets (lxo_greedy_decode_constrained / lxo_beam_decode_constrained), device bit sets: bit v & 31 of word v >> 5 of row b set = image b
// may emit token v; ld words per row, 0 = one row shared by every image.  A banned column is read as a column outside the vocabulary.
// per_row != 0 (a grammar call, grammar.h): one row per DECODER ROW -- beam slot b * k + j, draw b * n + j -- instead of one per image
struct DecAllow { const unsigned* bits; int ld; int per_row; };
// alternatives per position of the same logits: ids_out / logp_out [B][T][k] = the k first columns of row t * B + b (value descending, then column
// ascending) and logits[id] - lse, rank_out [B][T] (nullable) = the columns in front of the clamped target, ent_out [B][T] (nullable) = sum p (lse - x);
// allow (nullable): one row per sample b, everything then runs over its allowed columns (banned target: rank -1; no column left: -1 / -inf);
// rows t >= lengths[b]: -1 / 0 / -1 / 0; chain_err set: -1 / NaN / -1 / NaN.  1 <= k <= min(16, V), else -2.  Reads the logits only.
int lxo_k_score_alt(int dt, const float* logits, const int* formula, const int* lengths, int k, const DecAllow* allow, int* ids_out, float* logp_out,
                    int* rank_out, float* ent_out, const unsigned* chain_err, int B, int T, int V, int Vp, hipStream_t st);
int lxo_k_argmax(const float* logits, int Vp, int V, int n, int id_end, int* ids_step, int* ids_out, int max_steps, int step,
                 int* finished, int* n_unfinished, hipStream_t st, float* logp_out = nullptr,      // logp_out (nullable): [n][max_steps] log-prob of the id
                 const DecPrefix* prefix = nullptr, const DecAllow* allow = nullptr);
// The sampled select step (lxo_sample_decode / lxo_sample_tokens).  THE DISTRIBUTION AND THE DRAW, stated here once: for a decoder row with f32
// logits x[0..V) whose image allows the set A (a banned column is a column outside the vocabulary), temperature tau > 0, top_k K >= 0 (0: off) and
// top_p p in (0, 1] (1: off):
//   1. y_v = x_v * (1 / tau) in f32;
//   2. the row's total order is alt_before's on x: value descending, then column ascending;
//   3. C_K = the first K allowed columns of that order (all of A when K = 0 or K >= |A|);
//   4. q = softmax of y over C_K; C = the shortest prefix of the order inside C_K whose q-mass is >= p (temperature, then top-k, then top-p on
//      the renormalised mass);
//   5. the token is argmax over v in C of y_v + g_v, ties to the lower column, g_v = -log(-log u_v): the Gumbel-max trick -- arg-max row steps, no
//      prefix sum over the row;
//   6. logp = x_id - logsumexp_A(x), the model's own log-prob (lxo_k_argmax's arithmetic), logq = y_id - logsumexp_C(y), the log-prob under the
//      distribution sampled from.
// The uniforms are counter-based: mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
// z ^= z >> 31 in 64 bits; key = mix(seed << 32 | b << 4 | j) for draw j (< 16) of image b; bits = mix(key + (t V + v)) >> 41 (23 bits);
// u = (bits + 0.5) 2^-23.  23 bits, not 24: bits + 0.5 is then exact in f32, u never rounds to 1 and g is always finite.  logf and expf in both
// dtype modes.  So draw (b, j) at step t depends on neither n nor B nor another row, a seed repeats bit for bit, and K = 1 is the arg-max.
// n, cb: filled in by the launcher (draws per image; the bits of a column index)
struct DecSample { float inv_tau; int top_k; float top_p; unsigned seed; int n; int cb; };
// row r of logits [rows][Vp] = draw r % n of image r / n at step `time` (the hash's and the prefix's step); ids_out / logp_out / logq_out (the last
// two nullable) [image][max_steps][n] at column ostep; ids_step (nullable) [rows]: the ids fed back; finished / n_unfinished (nullable together):
// as lxo_k_argmax keeps them.  prefix / allow: one row per IMAGE.  A forced step emits the forced id, its logp, logq 0, and draws nothing.
int lxo_k_sample(const float* logits, int Vp, int V, int rows, int n, int id_end, int time, const DecSample& opts, int* ids_step, int* ids_out,
                 float* logp_out, float* logq_out, int max_steps, int ostep, int* finished, int* n_unfinished, hipStream_t st,
                 const DecPrefix* prefix = nullptr, const DecAllow* allow = nullptr);
int lxo_k_beam_step(float* logits, int Vp, int V, int nimg, int k, int id_end, int time, float div_gamma, float div_prob, int div_seed,
                    float* scratch, float* logp, int* finished,
                    int* ids_step, int* parents_step, int* ids_out, int* par_out, int max_steps, int* n_unfinished, hipStream_t st,
                    float* scores_out = nullptr,      // scores_out (nullable): [nimg][max_steps][k] the running log-probs after the step
                    const DecPrefix* prefix = nullptr, const DecAllow* allow = nullptr);      // allow: one row per IMAGE
