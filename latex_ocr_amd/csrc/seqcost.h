// Launchers of the sequence-cost kernels (seqcost.hip): batched Levenshtein distance over token rows, and the candidate rows of a minimum-risk
// step built on the device from sampled ids and references, and the minimum-risk choice among an image's draws; the text metrics' counts and the
// sentence-level BLEU built on them, as a score and as the cost of the candidates and of the consensus.
#pragma once
#include "lxo_common.h"

// the widest reference a pair may have: 64 lanes x the widest strip of DP columns a lane owns (edit_kernel<16>)
constexpr int kEditMaxRef = 1024;

// Pair p: hypothesis row p against reference row ref_of[p] (NULL: p / per_ref), clamped into [0, G).  Hypothesis row p starts at element
// (p / hyp_block) * hb_stride + (p % hyp_block) * hr_stride of `hyp` and its tokens are ht_stride apart; its sequence is the first
// hyp_len[p] (NULL: T; clamped into [0, T]) tokens cut at the first id_end (id_end < 0: no cut).  The reference side likewise: row r of
// ref [G][ref_ld], ref_len[r] (NULL: ref_ld), the same cut.  dist (nullable) int32 [pairs], cost (nullable) f32 [pairs] =
// (float)dist / (float)max(reference tokens, 1), one IEEE division.  live (nullable, device int [1]): pairs p >= live[0] get dist = cost = 0
// and read nothing.  ref_ld > kEditMaxRef: -2.
struct EditArgs {
    const int* hyp; const int* hyp_len; const int* ref; const int* ref_len; const int* ref_of; const int* live;
    int* dist; float* cost;
    long long hb_stride, hr_stride, ht_stride;
    int hyp_block, T, G, ref_ld, per_ref, pairs, id_end;
};
int lxo_k_edit_distance(const EditArgs& a, hipStream_t st);

// The candidate rows of a minimum-risk step (lxo_mrt_candidates): ids [B][max_steps][n] of a sampled decode that ran `steps` steps, ref [B][Tr] with
// ref_len [B].  R = B (n + inc) rows of Tc = max(steps + 1, Tr) tokens; three launches, no host synchronisation: the draws' lengths and which of them
// repeat (into cost_out, as scratch), the rows, their costs through lxo_k_edit_distance.
struct CandArgs {
    const int* ids; const int* ref; const int* ref_len;
    int* cand; int* cand_len; float* cost; int* group_off; int* row_image;
    int B, max_steps, n, steps, Tr, id_end, id_pad, inc;
};
// cost_kind 0: the edit-distance cost through lxo_k_edit_distance; 1: 1 - sentence BLEU through lxo_k_sentence_bleu (then steps + 1 <= kEditMaxRef too)
int lxo_k_mrt_candidates(const CandArgs& a, hipStream_t st, int cost_kind = 0);

// The consensus among the draws of an image (lxo_consensus, include/lxo.h holds the definition): draw i of image g starts at element
// g image_stride + i draw_stride of ids, its tokens tok_stride apart, T of them, cut at the first id_end.  Two launches, no host synchronisation:
// the distances of the B n (n - 1) / 2 unordered pairs into both halves of dist [B][n][n] (and the draws' lengths into risk, as scratch), then per
// image the risks, the diagonal and the arg-min.  T > kEditMaxRef, n > kConsensusMaxN or more waves than a grid holds: -2.
constexpr int kConsensusMaxN = 64;
struct ConsArgs {
    const int* ids; const float* weights;
    int* dist; float* risk; int* best;
    long long image_stride, draw_stride, tok_stride;
    int B, n, T, id_end, normalize;
};
int lxo_k_consensus(const ConsArgs& a, hipStream_t st);

// The text metrics' counts (lxo_text_stats, include/lxo.h holds the definition): pairs addressed, cut and clamped as EditArgs', T <= kEditMaxRef as
// well.  stats (nullable) int32 [pairs][kTextStats]; corpus (nullable) int64 [kTextCorpus], overwritten or added to (accumulate).  With stats: one
// launch for the rows and a one-workgroup launch that sums them in a fixed order; without: the waves add their rows into corpus with 64-bit integer
// atomics (behind a launch that zeroes it when it is overwritten).  No host synchronisation.  T or ref_ld > kEditMaxRef: -2.
constexpr int kTextStats = 12, kTextCorpus = 14;
struct TextArgs {
    const int* hyp; const int* hyp_len; const int* ref; const int* ref_len; const int* ref_of;
    int* stats; long long* corpus;
    long long hb_stride, hr_stride, ht_stride;
    int hyp_block, T, G, ref_ld, per_ref, pairs, id_end, accumulate;
};
int lxo_k_text_stats(const TextArgs& a, hipStream_t st);

// Sentence-level BLEU of pairs (lxo_sentence_bleu, include/lxo.h holds the definition): pairs addressed, cut and clamped as TextArgs'.  counts (nullable)
// int32 [pairs][kBleuCounts], bleu (nullable) and cost (nullable) f32 [pairs]; live as EditArgs': pairs p >= live[0] read nothing and cost 0.  One launch,
// one wave per pair, no Levenshtein DP, no host synchronisation.  T or ref_ld > kEditMaxRef: -2.
constexpr int kBleuCounts = 10;
struct BleuArgs {
    const int* hyp; const int* hyp_len; const int* ref; const int* ref_len; const int* ref_of; const int* live;
    int* counts; float* bleu; float* cost;
    long long hb_stride, hr_stride, ht_stride;
    int hyp_block, T, G, ref_ld, per_ref, pairs, id_end;
};
int lxo_k_sentence_bleu(const BleuArgs& a, hipStream_t st);

// The consensus under the cost 1 - sentence BLEU (lxo_consensus_bleu): draws addressed as ConsArgs'.  Two launches: one wave per unordered pair counts the
// clipped matches once and writes both directions of cost [B][n][n] (and of match (nullable) int32 [B][n][n][4]), then per image the risks, the
// diagonal and the arg-min.  The limits and -2 of lxo_k_consensus.
struct ConsBleuArgs {
    const int* ids; const float* weights;
    int* match; float* cost; float* risk; int* best;
    long long image_stride, draw_stride, tok_stride;
    int B, n, T, id_end;
};
int lxo_k_consensus_bleu(const ConsBleuArgs& a, hipStream_t st);

// The edit alignment of pairs (lxo_edit_align, include/lxo.h holds the definition and the path rule): pairs addressed, cut and clamped as TextArgs'.
// hyp_align (nullable) int32 [pairs][T], ref_align (nullable) int32 [pairs][ref_ld], counts (nullable) int32 [pairs][kAlignCounts]; corpus (nullable)
// int64 [kAlignCorpus] and confusion (nullable) int64 [(V + 1)(V + 1)], overwritten (zeroed by a launch in front) or added to (accumulate) with 64-bit
// integer atomics.  steps: the scratch, one dword per lane per row of the table -- pair p's row i (1 .. m) at dword (p T + i - 1) 64 + lane, the 2-bit
// steps of the lane's strip of columns, column e of the strip in bits 2e, 2e + 1 (0 diagonal, 1 insertion, 2 deletion).  One wave per pair, no host
// synchronisation.  T or ref_ld > kEditMaxRef: -2.
constexpr int kAlignCounts = 6, kAlignCorpus = 8;
struct AlignArgs {
    const int* hyp; const int* hyp_len; const int* ref; const int* ref_len; const int* ref_of;
    int* hyp_align; int* ref_align; int* counts; long long* corpus; long long* confusion; unsigned* steps;
    long long hb_stride, hr_stride, ht_stride;
    int hyp_block, T, G, ref_ld, per_ref, pairs, id_end, V, accumulate;
};
inline size_t lxo_k_edit_align_scratch_bytes(int pairs, int T, int ref_ld) {
    (void)ref_ld;
    return pairs > 0 && T > 0 ? (size_t)pairs * (size_t)T * 256u : 0;
}
int lxo_k_edit_align(const AlignArgs& a, hipStream_t st);
