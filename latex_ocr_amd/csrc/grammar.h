// Launchers of the delimiter-grammar kernels (grammar.hip): a pushdown state per decoder row on the device and, from it, the row's allowed-token
// set of the next decode step.  The select kernels (head_kernels.hip) read that set as they read any allowed-token set.
#pragma once
#include "lxo_common.h"

// the deepest stack a row may hold (include/lxo.h: LXO_GRAMMAR_MAX_DEPTH) and the number of delimiter kinds (a stack entry is 4 bits)
constexpr int kGrammarMaxDepth = 32;
constexpr int kGrammarMaxKinds = 15;
// class bit sets in front of the scratch: plain, opener, END, then one per closer kind 1 .. 15; W = (V + 31) / 32 words each
constexpr int kGrammarSets = 3 + kGrammarMaxKinds;
// words of one row's state: [0] depth, [1 .. 4] the stack, entry i in bits 4 (i & 7) .. of word 1 + (i >> 3); [5 .. 7] unused
constexpr int kGrammarStateWords = 8;

// cls int8 [V] (device): 0 plain, +q opener of kind q, -q closer of kind q, 1 <= q <= n_kinds; a value outside that range and id_end read as
// plain / END.  rows decoder rows, k of them per image (greedy 1, beam: the hypothesis slots, sampling: the draws).  allow (nullable): the
// static sets, one row per IMAGE, allow_ld words apart (0: one row for all).  scratch: lxo_k_grammar_scratch_words(rows, V) words:
//   [kGrammarSets][W] class sets | [2][rows][kGrammarStateWords] states (the state BEFORE step t in buffer t & 1) | [rows][W] the sets S_t
struct GrammarArgs {
    const signed char* cls; int n_kinds, max_depth, budget;
    const unsigned* allow; int allow_ld;
    unsigned* scratch;
    int rows, k, V, id_end, max_iter;
};
long long lxo_k_grammar_scratch_words(int rows, int V);
// the sets S_t of the rows inside the scratch: [rows][(V + 31) / 32]
unsigned* lxo_k_grammar_sets(const GrammarArgs& a);
// once per call: class sets from cls, both state buffers cleared, S_0
int lxo_k_grammar_setup(const GrammarArgs& a, hipStream_t st);
// behind the select of step `time`: ids / finished [rows] as the select left them, parents (nullable) [rows]: the slot inside the row's image
// whose state the row continues (clamped into [0, k)).  Writes the state after the step, depth_out (nullable) at
// [(image * max_steps + ostep) * k + slot], and S_{time + 1}.  A finished row keeps its (parent's) state and gets S = A.
int lxo_k_grammar_step(const GrammarArgs& a, const int* ids, const int* parents, const int* finished, int time, int* depth_out, int max_steps,
                       int ostep, hipStream_t st);
