// The finish of a beam search on the device (lxo_beam_finalize, lxo_beam_rerank; include/lxo.h holds the definitions).
//
// FINALIZE: the beam decodes leave ids / parents / scores [B][ld_t][k]; the hypothesis that ends in slot i exists only after the parents are walked
// back from the last step (utils/text.beam_slots' rule).  That walk is a chain of `steps` dependent reads, so it must not run over global memory:
//   1. all 256 threads stage the image's parents in LDS, clamped into [0, k), a BYTE each (k <= 16): consecutive threads read consecutive words,
//      16 KB at the limits (1024 steps, k = 16);
//   2. lane i < k of the first wave walks slot i back through the stage -- one ds_read_u8 per step on the chain, its ds_write_b8 into the slot
//      table (a second byte table in LDS) off it -- while the other waves wait at the barrier;
//   3. every thread owns one slot i = tid mod kp (kp = k rounded up to a power of two) and the steps t = tid / kp + j 256 / kp: it gathers
//      ids[t][slot[t][i]] and keeps the first step that holds id_end; the minimum over a slot's threads is four shuffles inside a wave and a
//      16-word LDS row per wave across them.  No atomics;
//   4. in the same mapping every output is written, each element once, with loads that depend on the LDS tables alone: a wave's stores are one
//      run of 64 k / kp consecutive words (src: k words per step, the layout's own stride).
// Nothing at or behind step `steps` is read.
//
// RERANK: one wave per image, four images per workgroup.  The coverage penalty of hypothesis i is summed lane-strided over its R cells -- logf per
// cell, the sum in double, a butterfly across the lanes: a fixed order -- the length penalty, the softmax over the k frozen scores and the final
// combination are double arithmetic on lane i rounded once to f32 (so alpha = 0 without coverage returns seq_logp bit for bit), the order is a
// rank count over k shuffles.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage) are listed in profiles/beam_finalize.txt.
#include "beamfin.h"
#include <math.h>

namespace {

LXO_DEV double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// lg = log2(kp), kp = the power of two in [k, 2k): the slot-per-thread mapping of phases 3 and 4
__global__ __launch_bounds__(256) void beam_finalize_kernel(BeamFinArgs a, int lg) {
    __shared__ unsigned char par[kBeamFinMaxSteps * kBeamFinMaxK];
    __shared__ unsigned char slot[kBeamFinMaxSteps * kBeamFinMaxK];
    __shared__ int first[4][kBeamFinMaxK];
    const int b = blockIdx.x, tid = threadIdx.x, k = a.k, steps = a.steps, n = steps * k;
    const long long base = (long long)b * a.ld_t * k;
    const int* pp = a.parents + base;
    for (int e = tid; e < n; e += 256) par[e] = (unsigned char)min(max(pp[e], 0), k - 1);
    __syncthreads();
    if (tid < k) {
        int s = tid;
        for (int t = steps - 1; t >= 0; --t) {
            slot[t * k + tid] = (unsigned char)s;
            s = par[t * k + s];
        }
    }
    __syncthreads();
    const int kp = 1 << lg, i = tid & (kp - 1), tg = tid >> lg, G = 256 >> lg;
    const bool on = i < k;
    const int* ids = a.ids + base;
    int f = steps;                                                       // the first step of the path that holds id_end
    if (on) {
#pragma unroll 4
        for (int t = tg; t < steps; t += G)
            if (ids[t * k + slot[t * k + i]] == a.id_end) f = min(f, t);
    }
    for (int o = 32; o >= kp; o >>= 1) f = min(f, __shfl_xor(f, o));     // the lanes of one slot lie kp apart
    if ((tid & 63) < kp) first[tid >> 6][i] = f;
    __syncthreads();
    f = min(min(first[0][i], first[1][i]), min(first[2][i], first[3][i]));
    const int len = f < steps ? f + 1 : steps;
    if (!on) return;
    const float* sc = a.scores ? a.scores + base : nullptr;              // read only where an output asks for it (the entry point's check)
    const long long ob = (long long)b * n;
    const int row = b * k + i;
    for (int t = tg; t < steps; t += G) {
        const int e = t * k + i, s = slot[e];
        if (a.hyp) a.hyp[ob + e] = t < len ? ids[t * k + s] : a.id_end;
        if (a.src) a.src[(long long)t * a.B * k + row] = b * k + par[t * k + s];
        if (a.tok_logp) {
            float v = 0.f;
            if (t < len) {
                const float prev = t ? sc[(t - 1) * k + slot[e - k]] : 0.f;
                v = sc[t * k + s] - prev;
            }
            a.tok_logp[ob + e] = v;
        }
    }
    if (tg == 0) {
        if (a.len) a.len[row] = len;
        if (a.seq_logp) a.seq_logp[row] = sc[(len - 1) * k + slot[(len - 1) * k + i]];
    }
}

__global__ __launch_bounds__(256) void beam_rerank_kernel(BeamRerankArgs a) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6), k = a.k;
    if (b >= a.B) return;                                                // a whole wave
    const bool on = lane < k;
    double cp = 0.0;
    if (a.coverage) {
        for (int i = 0; i < k; ++i) {
            const float* row = a.coverage + ((long long)b * k + i) * a.cov_ld;
            double s = 0.0;
            for (int r = lane; r < a.R; r += 64) s += (double)logf(fminf(fmaxf(row[r], a.cov_floor), 1.f));      // (a NaN cell counts as the floor)
            s = wave_sum_d(s);
            if (lane == i) cp = s;
        }
    }
    const float sl = on ? a.seq_logp[b * k + lane] : -INFINITY;
    const int ln = on ? max(a.len[b * k + lane], 0) : 1;
    const double lp = pow((5.0 + (double)ln) / 6.0, (double)a.alpha);   // pow(x, 0) = 1: seq_logp / 1 is seq_logp
    const double q = (double)sl / lp;
    const float score = a.coverage ? (float)(q + (double)a.beta * cp) : (float)q;
    const float m = wave_max(sl);
    const double ex = on ? exp((double)sl - (double)m) : 0.0;
    const double Z = wave_sum_d(ex);
    int rank = 0;
    for (int j = 0; j < k; ++j) {
        const float sj = __shfl(score, j);
        rank += (sj > score || (sj == score && j < lane)) ? 1 : 0;
    }
    if (!on) return;
    if (a.score) a.score[b * k + lane] = score;
    if (a.post) a.post[b * k + lane] = (float)(ex / Z);
    if (a.order) a.order[b * k + rank] = lane;
}

}  // namespace

int lxo_k_beam_finalize(const BeamFinArgs& a, hipStream_t st) {
    if (a.k < 1 || a.k > kBeamFinMaxK || a.steps < 1 || a.steps > kBeamFinMaxSteps || a.ld_t < a.steps) return -2;
    if (a.B <= 0) return 0;
    int lg = 0;
    while ((1 << lg) < a.k) ++lg;
    hipLaunchKernelGGL(beam_finalize_kernel, dim3((unsigned)a.B), dim3(256), 0, st, a, lg);
    return (int)hipGetLastError();
}

int lxo_k_beam_rerank(const BeamRerankArgs& a, hipStream_t st) {
    if (a.k < 1 || a.k > kBeamFinMaxK) return -2;
    if (a.B <= 0) return 0;
    hipLaunchKernelGGL(beam_rerank_kernel, dim3((unsigned)cdiv(a.B, 4)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}
