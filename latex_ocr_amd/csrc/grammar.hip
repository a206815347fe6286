// Decode under a delimiter grammar: a pushdown state per decoder row -- a depth d in [0, D] and the stack of the d open kinds -- and the row's
// allowed-token set of the next step, S = A & G(state, t).  G (include/lxo.h): a closer of kind q iff d > 0 and the top is q; END iff
// d == 0; an opener iff d < D (budget: and r >= d + 2); any other token (budget:) iff r >= d + 1, r = max_iter - t the steps that can still
// follow step t.  With the budget d <= r holds before every step, so a row can always close what it opened and emit END by step max_iter.
// Integer arithmetic and plain vector loads / stores throughout; every word index stays inside [0, (V + 31) / 32).
#include "grammar.h"

namespace {

// the class of token v as the kernels read it: END first, a kind outside 1 .. n_kinds is plain
LXO_DEV int gram_cls(const signed char* cls, int v, int n_kinds, int id_end) {
    if (v == id_end) return 0;
    const int c = cls[v];
    return (c > n_kinds || c < -n_kinds) ? 0 : c;
}
// G(state, t) over one word of the class sets: close_top = the word of the closers of the stack's top (unused at d == 0)
LXO_DEV unsigned gram_mask(unsigned plain, unsigned open, unsigned end, unsigned close_top, int d, int D, int budget, int r) {
    unsigned m = d > 0 ? close_top : end;
    if (d < D && (!budget || r >= d + 2)) m |= open;
    if (!budget || r >= d + 1) m |= plain;
    return m;
}
// entry i of a stack (selects, not an indexed register array: no scratch)
LXO_DEV int gram_entry(const unsigned (&st)[4], int i) {
    const unsigned w = i < 8 ? st[0] : i < 16 ? st[1] : i < 24 ? st[2] : st[3];
    return (int)((w >> ((i & 7) * 4)) & 15u);
}
// the bits of word w that are tokens
LXO_DEV unsigned gram_valid(int w, int V) { return (w == (V >> 5)) ? ((1u << (V & 31)) - 1u) : 0xffffffffu; }
LXO_DEV unsigned gram_allow(const GrammarArgs& a, int b, int W, int w) { return a.allow ? a.allow[(long long)b * a.allow_ld + w] : 0xffffffffu; }

// Set-up: thread i = (row i / W, word i % W) forms word w of every class set from cls (row 0's threads store them), clears the row's two states
// (word 0's thread) and writes S_0[row][w] -- every row starts at depth 0
__global__ __launch_bounds__(256) void grammar_setup_kernel(GrammarArgs a, int W) {
    const long long total = (long long)a.rows * W;
    unsigned* cw = a.scratch;
    unsigned* states = cw + (long long)kGrammarSets * W;
    unsigned* sets = states + 2ll * a.rows * kGrammarStateWords;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int row = (int)(i / W), w = (int)(i - (long long)row * W);
        unsigned plain = 0u, open = 0u, end = 0u;
        for (int e = 0; e < 32; ++e) {
            const int v = 32 * w + e;
            if (v >= a.V) break;
            const int c = gram_cls(a.cls, v, a.n_kinds, a.id_end);
            if (v == a.id_end) end |= 1u << e;
            else if (c == 0) plain |= 1u << e;
            else if (c > 0) open |= 1u << e;
        }
        if (row == 0) {
            cw[w] = plain; cw[W + w] = open; cw[2 * W + w] = end;
            for (int q = 1; q <= kGrammarMaxKinds; ++q) {
                unsigned cl = 0u;
                for (int e = 0; e < 32; ++e) {
                    const int v = 32 * w + e;
                    if (v >= a.V) break;
                    if (gram_cls(a.cls, v, a.n_kinds, a.id_end) == -q) cl |= 1u << e;
                }
                cw[(long long)(2 + q) * W + w] = cl;
            }
        }
        if (w == 0)
            for (int e = 0; e < kGrammarStateWords; ++e) {
                states[(long long)row * kGrammarStateWords + e] = 0u;
                states[((long long)a.rows + row) * kGrammarStateWords + e] = 0u;
            }
        const unsigned m = gram_mask(plain, open, end, 0u, 0, a.max_depth, a.budget, a.max_iter);
        sets[i] = gram_allow(a, a.allow_ld ? row / a.k : 0, W, w) & m & gram_valid(w, a.V);
    }
}

// Step: one wave per row.  Every lane reads the (parent's) old state and forms the new depth and top; lane 0 stores the new state and the
// depth; the lanes share the row's W words of S_{time + 1}.  Old states: buffer time & 1, new: the other one -- a beam slot may read a state that
// another slot's wave replaces in the same launch, so nothing is updated in place.
__global__ __launch_bounds__(256) void grammar_step_kernel(GrammarArgs a, int W, const int* __restrict__ ids, const int* __restrict__ parents,
                                                           const int* __restrict__ finished, int time, int* __restrict__ depth_out, int max_steps, int ostep) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int b = row / a.k, j = row - b * a.k;
    const unsigned* cw = a.scratch;
    unsigned* states = a.scratch + (long long)kGrammarSets * W;
    unsigned* sets = states + 2ll * a.rows * kGrammarStateWords;
    int src = row;
    if (parents) src = b * a.k + min(max(parents[row], 0), a.k - 1);
    const unsigned* so = states + ((long long)(time & 1) * a.rows + src) * kGrammarStateWords;
    unsigned* sn = states + ((long long)((time + 1) & 1) * a.rows + row) * kGrammarStateWords;
    const int D = a.max_depth;
    int d = min(max((int)so[0], 0), D);
    unsigned st[4] = {so[1], so[2], so[3], so[4]};
    const bool fin = finished[row] != 0;
    if (!fin) {
        const int id = ids[row];
        const int c = (id >= 0 && id < a.V) ? gram_cls(a.cls, id, a.n_kinds, a.id_end) : 0;
        if (c > 0 && d < D) {
            const int sh = (d & 7) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e == (d >> 3)) st[e] = (st[e] & ~(15u << sh)) | ((unsigned)c << sh);
            ++d;
        } else if (c < 0 && d > 0 && gram_entry(st, d - 1) == -c) --d;
    }
    if (lane == 0) {
        sn[0] = (unsigned)d; sn[1] = st[0]; sn[2] = st[1]; sn[3] = st[2]; sn[4] = st[3];
        if (depth_out) depth_out[((long long)b * max_steps + ostep) * a.k + j] = d;
    }
    const int top = d > 0 ? gram_entry(st, d - 1) : 0;             // 1 .. 15 at d > 0 for every state the kernels wrote; 0 reads the END set
    const int r = a.max_iter - (time + 1);
    const int ab = a.allow_ld ? b : 0;
    for (int w = lane; w < W; w += 64) {
        unsigned m = 0xffffffffu;                                   // a finished row: the grammar is off
        if (!fin) m = gram_mask(cw[w], cw[W + w], cw[2 * W + w], cw[(long long)(2 + top) * W + w], d, D, a.budget, r);
        sets[(long long)row * W + w] = gram_allow(a, ab, W, w) & m & gram_valid(w, a.V);
    }
}

}  // namespace

long long lxo_k_grammar_scratch_words(int rows, int V) {
    const long long W = (V + 31) / 32;
    return kGrammarSets * W + 2ll * rows * kGrammarStateWords + (long long)rows * W;
}
unsigned* lxo_k_grammar_sets(const GrammarArgs& a) {
    return a.scratch + (long long)kGrammarSets * ((a.V + 31) / 32) + 2ll * a.rows * kGrammarStateWords;
}
static bool grammar_args_ok(const GrammarArgs& a) {
    return a.cls && a.scratch && a.rows >= 1 && a.k >= 1 && a.rows % a.k == 0 && a.V >= 1 && a.n_kinds >= 1 && a.n_kinds <= kGrammarMaxKinds &&
           a.max_depth >= 1 && a.max_depth <= kGrammarMaxDepth && (!a.allow || a.allow_ld == 0 || a.allow_ld >= (a.V + 31) / 32);
}
int lxo_k_grammar_setup(const GrammarArgs& a, hipStream_t st) {
    if (!grammar_args_ok(a)) return -2;
    const int W = (a.V + 31) / 32;
    const long long total = (long long)a.rows * W;
    hipLaunchKernelGGL(grammar_setup_kernel, dim3((unsigned)(total + 255 < 256ll * 1024 ? (total + 255) / 256 : 1024)), dim3(256), 0, st, a, W);
    return (int)hipGetLastError();
}
int lxo_k_grammar_step(const GrammarArgs& a, const int* ids, const int* parents, const int* finished, int time, int* depth_out, int max_steps,
                       int ostep, hipStream_t st) {
    if (!grammar_args_ok(a) || !ids || !finished || time < 0 || max_steps < 1 || ostep < 0 || ostep >= max_steps) return -2;
    hipLaunchKernelGGL(grammar_step_kernel, dim3(cdiv(a.rows, 4)), dim3(256), 0, st, a, (a.V + 31) / 32, ids, parents, finished, time, depth_out,
                       max_steps, ostep);
    return (int)hipGetLastError();
}
