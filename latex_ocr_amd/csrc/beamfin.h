// Launchers of the beam-finish kernels (beamfin.hip): the back-trace of a beam decode's ids / parents / scores into its k hypotheses, and the rerank
// of those hypotheses under a length and a coverage penalty.  include/lxo.h (lxo_beam_finalize, lxo_beam_rerank) holds the definitions.
#pragma once
#include "lxo_common.h"

constexpr int kBeamFinMaxK = 16;        // the widest beam the decode kernels take
constexpr int kBeamFinMaxSteps = 1024;  // what the LDS stage holds: a byte per parent and a byte per slot, 2 x 16 KB at the limits

// ids / parents / scores [B][ld_t][k] (scores nullable), the first `steps` steps valid; hyp / tok_logp [B][steps][k], len / seq_logp [B][k],
// src [steps][B k]; every output nullable.  One workgroup per image, no atomics, no host synchronisation.  k or steps outside the limits: -2.
struct BeamFinArgs {
    const int* ids; const int* parents; const float* scores;
    int* hyp; int* len; int* src; float* tok_logp; float* seq_logp;
    int B, ld_t, steps, k, id_end;
};
int lxo_k_beam_finalize(const BeamFinArgs& a, hipStream_t st);

// len / seq_logp [B][k], coverage f32 [B k][cov_ld] (nullable; R cells read per row); score / post f32 [B][k], order int32 [B][k], each nullable.
// One wave per image.  k outside the limit: -2.
struct BeamRerankArgs {
    const int* len; const float* seq_logp; const float* coverage;
    float* score; float* post; int* order;
    int B, k, R, cov_ld;
    float alpha, beta, cov_floor;
};
int lxo_k_beam_rerank(const BeamRerankArgs& a, hipStream_t st);
