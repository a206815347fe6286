// Sequence costs on the device: the batched Levenshtein distance (lxo_edit_distance) and the candidate rows of a minimum-risk step built from
// sampled ids (lxo_mrt_candidates).  Integer arithmetic throughout: exact, and the same in every order.  On top of the distances, the
// minimum-risk choice among the draws of an image (lxo_consensus): all pairwise distances, the expected cost of every draw, the arg-min.
// And the counts an evaluation's text metrics are made of (lxo_text_stats): clipped n-gram matches, lengths, distance and exact match per pair,
// summed over the pairs into a corpus row.  And that metric as a cost: the sentence-level BLEU of a pair (lxo_sentence_bleu), the consensus under
// 1 - sBLEU (lxo_consensus_bleu) and the candidate rows costed with it (lxo_mrt_candidates_cost); their float tails are f32 in one fixed order.
// And the path through the Levenshtein table (lxo_edit_align): substitution, insertion and deletion counts, the token maps of both sides, confusion pairs.
#include "seqcost.h"

namespace {

// A side's sequence: the first `len` tokens of a strided row, cut at the first id_end (truncate_end's rule; id_end < 0: no cut).  The whole
// wave calls it; every lane returns the same length.
LXO_DEV int cut_len(const int* p, long long stride, int len, int id_end, int lane) {
    if (id_end < 0) return len;
    for (int t0 = 0; t0 < len; t0 += 64) {
        const int t = t0 + lane;
        const unsigned long long hit = __ballot(t < len && p[t * stride] == id_end);
        if (hit) return t0 + (int)__builtin_ctzll(hit);
    }
    return len;
}

// ---- Levenshtein distance, one wave per pair ----
// The DP table has a row per hypothesis token and a column per reference token; lane l owns the CPL columns l CPL + 1 .. l CPL + CPL (column 0 is
// the row number).  With t[j] = min(prev[j] + 1, prev[j - 1] + (x != b[j])) -- what a cell gets from the row above -- and t[0] = i, the horizontal
// dependency cur[j] = min(t[j], cur[j - 1] + 1) unrolls to cur[j] = j + min_{k <= j} (t[k] - k): a min-plus prefix.  So a row costs one neighbour
// exchange (prev of the column left of the strip), a serial prefix-min over the strip and one exclusive prefix-min scan over the 64 lanes.
// Columns beyond the reference's n tokens compute values nobody reads (a cell depends on columns to its left only).
// m hypothesis tokens at hp (stride hts), n <= 64 CPL reference tokens at rp (stride rts) -> the distance, in every lane.
template <int CPL>
LXO_DEV int edit_wave(const int* hp, long long hts, int m, const int* rp, long long rts, int n, int lane) {
    int b[CPL], prev[CPL];
#pragma unroll
    for (int e = 0; e < CPL; ++e) {
        const int j = lane * CPL + e;
        b[e] = j < n ? rp[j * rts] : -1;
        prev[e] = j + 1;
    }
    for (int i0 = 0; i0 < m; i0 += 64) {
        const int xi = hp[(i0 + lane < m ? i0 + lane : i0) * hts];      // 64 hypothesis tokens per load, handed out lane by lane below
        const int cnt = min(64, m - i0);
        for (int k = 0; k < cnt; ++k) {
            const int x = __shfl(xi, k), i = i0 + k + 1;
            int left = __shfl_up(prev[CPL - 1], 1);
            if (lane == 0) left = i - 1;
            int s[CPL], run = 0x3fffffff;
#pragma unroll
            for (int e = 0; e < CPL; ++e) {
                const int diag = e ? prev[e - 1] : left;
                const int t = min(prev[e] + 1, diag + (x != b[e] ? 1 : 0));
                run = min(run, t - (lane * CPL + e + 1));
                s[e] = run;
            }
            int v = lane == 0 ? min(run, i) : run;                       // t[0] - 0 = i joins lane 0's strip
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(v, d);
                if (lane >= d) v = min(v, o);
            }
            int ex = __shfl_up(v, 1);
            if (lane == 0) ex = i;
#pragma unroll
            for (int e = 0; e < CPL; ++e) prev[e] = lane * CPL + e + 1 + min(s[e], ex);
        }
    }
    if (n == 0) return m;
    int r = 0;
#pragma unroll
    for (int e = 0; e < CPL; ++e) if (e == (n - 1) % CPL) r = prev[e];
    return __shfl(r, (n - 1) / CPL);
}

template <int CPL>
__global__ __launch_bounds__(256) void edit_kernel(EditArgs a) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.pairs) return;
    if (a.live && p >= a.live[0]) {
        if (lane == 0) { if (a.dist) a.dist[p] = 0; if (a.cost) a.cost[p] = 0.f; }
        return;
    }
    // what the device holds is read defensively: a reference index is clamped into [0, G), a length into its row
    const int r = min(max(a.ref_of ? a.ref_of[p] : p / a.per_ref, 0), a.G - 1);
    const int* hp = a.hyp + (long long)(p / a.hyp_block) * a.hb_stride + (long long)(p % a.hyp_block) * a.hr_stride;
    const int* rp = a.ref + (long long)r * a.ref_ld;
    const int m = cut_len(hp, a.ht_stride, a.hyp_len ? min(max(a.hyp_len[p], 0), a.T) : a.T, a.id_end, lane);
    const int n = cut_len(rp, 1, min(a.ref_len ? min(max(a.ref_len[r], 0), a.ref_ld) : a.ref_ld, 64 * CPL), a.id_end, lane);
    const int d = edit_wave<CPL>(hp, a.ht_stride, m, rp, 1, n, lane);
    if (lane == 0) {
        if (a.dist) a.dist[p] = d;
        if (a.cost) a.cost[p] = (float)d / (float)max(n, 1);
    }
}

// ---- candidate rows of a minimum-risk step ----
// Launch 1, one workgroup per image: the length of each draw and of the reference (cut at END), and which draws repeat the reference or an earlier
// draw (equal length, equal tokens).  slot[g (n + inc) + k], k = the reference (inc) then the draws: the length of a row that is kept, -1 for a
// draw that is dropped.  The slots live in cost_out until launch 3 overwrites them.
LXO_DEV const int* cand_src(const CandArgs& a, int g, int k, long long& stride) {      // k = -1: the reference
    if (k < 0) { stride = 1; return a.ref + (long long)g * a.Tr; }
    stride = a.n;
    return a.ids + (long long)g * a.max_steps * a.n + k;
}
LXO_DEV int cand_Tc(const CandArgs& a) { return max(a.steps + 1, a.Tr); }

__global__ __launch_bounds__(256) void cand_analyse_kernel(CandArgs a, int* slot) {
    __shared__ int len[17], dup[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = blockIdx.x;
    if (threadIdx.x < 16) dup[threadIdx.x] = 0;
    for (int j = wave; j < a.n; j += 4) {
        long long st;
        const int* p = cand_src(a, g, j, st);
        const int L = cut_len(p, st, a.steps, a.id_end, lane);
        if (lane == 0) len[j + 1] = L;
    }
    if (wave == 0 && a.inc) {
        // (a reference without END inside its length would not fit its row with the END behind it: cut to Tc - 1 tokens)
        const int L = min(cut_len(a.ref + (long long)g * a.Tr, 1, min(max(a.ref_len[g], 0), a.Tr), a.id_end, lane), cand_Tc(a) - 1);
        if (lane == 0) len[0] = L;
    }
    __syncthreads();
    int q = 0;
    for (int j = 0; j < a.n; ++j)
        for (int i = a.inc ? -1 : 0; i < j; ++i, ++q) {
            if ((q & 3) != wave || len[i + 1] != len[j + 1]) continue;
            long long si, sj;
            const int* pi = cand_src(a, g, i, si);
            const int* pj = cand_src(a, g, j, sj);
            const int L = len[j + 1];
            bool same = true;
            for (int t0 = 0; t0 < L && same; t0 += 64) {
                const int t = t0 + lane;
                same = __ballot(t < L && pi[t * si] != pj[t * sj]) == 0ull;
            }
            if (same && lane == 0) dup[j] = 1;
        }
    __syncthreads();
    const int k = threadIdx.x, per = a.n + a.inc;
    if (k < per) slot[(long long)g * per + k] = (a.inc && k == 0) ? len[0] : (dup[k - a.inc] ? -1 : len[k - a.inc + 1]);
}

// Launch 2, one workgroup per image: its first row = the rows kept by the images in front of it (every workgroup counts for itself: B (n + inc)
// slots), then its rows -- tokens, END, PAD up to Tc -- with their lengths (tokens + 1) and image, group_off, and its share of the dead rows
// behind the last group (all PAD, length 0, image 0; their cost is launch 3's)
__global__ __launch_bounds__(256) void cand_emit_kernel(CandArgs a, const int* slot) {
    __shared__ int red[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = blockIdx.x, per = a.n + a.inc, Tc = cand_Tc(a);
    int before = 0, all = 0;
    for (int i = threadIdx.x; i < a.B * per; i += 256) {
        const int kept = slot[i] >= 0 ? 1 : 0;
        all += kept;
        if (i < g * per) before += kept;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o); all += __shfl_xor(all, o); }
    if (lane == 0) { red[0][wave] = before; red[1][wave] = all; }
    __syncthreads();
    before = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    all = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    int r = before;
    for (int k = 0; k < per; ++k) {
        const int L = slot[(long long)g * per + k];
        if (L < 0) continue;
        long long st;
        const int* p = cand_src(a, g, k - a.inc, st);
        for (int t = threadIdx.x; t < Tc; t += 256) a.cand[(long long)r * Tc + t] = t < L ? p[t * st] : (t == L ? a.id_end : a.id_pad);
        if (threadIdx.x == 0) { a.cand_len[r] = L + 1; a.row_image[r] = g; }
        ++r;
    }
    if (threadIdx.x == 0) { a.group_off[g + 1] = r; if (g == 0) a.group_off[0] = 0; }
    for (int d = all + g; d < a.B * per; d += a.B) {
        for (int t = threadIdx.x; t < Tc; t += 256) a.cand[(long long)d * Tc + t] = a.id_pad;
        if (threadIdx.x == 0) { a.cand_len[d] = 0; a.row_image[d] = 0; }
    }
}

// ---- consensus among the draws of an image (lxo_consensus) ----
// Launch 1, one wave per unordered pair (g, i < j), image by image in the order (0,1) (0,2) .. (0,n-1) (1,2) ..: the distance of the two draws into
// dist[g][i][j] and dist[g][j][i].  Equal draws (equal length, equal tokens) skip the DP: its answer for them is 0 as well.  The waves of the pairs
// (0, j) leave the draws' lengths in risk_out [g][j] (as int32) for launch 2.
LXO_DEV const int* cons_draw(const ConsArgs& a, int g, int i) { return a.ids + (long long)g * a.image_stride + (long long)i * a.draw_stride; }
LXO_DEV const int* cons_draw(const int* ids, long long image_stride, long long draw_stride, int g, int i) {
    return ids + (long long)g * image_stride + (long long)i * draw_stride;
}

template <int CPL>
__global__ __launch_bounds__(256) void cons_pairs_kernel(ConsArgs a, int per) {
    const int lane = threadIdx.x & 63, w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.B * per) return;
    const int g = w / per;
    int q = w % per, i = 0;
    while (q >= a.n - 1 - i) { q -= a.n - 1 - i; ++i; }
    const int j = i + 1 + q;
    const int* pi = cons_draw(a, g, i);
    const int* pj = cons_draw(a, g, j);
    const int Li = cut_len(pi, a.tok_stride, a.T, a.id_end, lane), Lj = cut_len(pj, a.tok_stride, a.T, a.id_end, lane);
    bool same = Li == Lj;
    for (int t0 = 0; t0 < Li && same; t0 += 64) {
        const int t = t0 + lane;
        same = __ballot(t < Li && pi[t * a.tok_stride] != pj[t * a.tok_stride]) == 0ull;
    }
    const int d = same ? 0 : edit_wave<CPL>(pi, a.tok_stride, Li, pj, a.tok_stride, Lj, lane);
    if (lane == 0) {
        int* row = a.dist + (long long)g * a.n * a.n;
        row[i * a.n + j] = d;
        row[j * a.n + i] = d;
        if (i == 0) {
            int* len = reinterpret_cast<int*>(a.risk) + (long long)g * a.n;
            len[j] = Lj;
            if (j == 1) len[0] = Li;
        }
    }
}

// Launch 2, one wave per image, lane i = draw i: risk[g][i] = (sum_j w_j c(i, j)) / sum_j w_j with both sums added in ascending j, products and sums
// rounded one by one (no fused multiply-add: the value is the one the f32 operations of the definition give); then the arg-min over the values
// written, the lower draw on ties.  The diagonal of dist is written here.
__global__ __launch_bounds__(256) void cons_select_kernel(ConsArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + (threadIdx.x >> 6), n = a.n;
    if (g >= a.B) return;
    const bool mine = lane < n;
    float* risk = a.risk + (long long)g * n;
    int* row = a.dist + (long long)g * n * n;
    const int len = mine && n > 1 ? reinterpret_cast<const int*>(risk)[lane] : 0;      // (one draw: no pair left a length, and none is needed)
    float w = 1.f;
    if (a.weights) {
        w = mine ? a.weights[(long long)g * n + lane] : 0.f;
        if (!(w > 0.f) || !(w - w == 0.f)) w = 0.f;                                    // negative, NaN, infinite: 0
        float sum = 0.f;
        for (int j = 0; j < n; ++j) sum += __shfl(w, j);
        if (sum == 0.f) w = 1.f;
    }
    float W = 0.f, acc = 0.f;
    for (int j = 0; j < n; ++j) {
        const float wj = __shfl(w, j);
        const int Lj = __shfl(len, j);
        const int d = mine && lane != j ? row[lane * n + j] : 0;
        const float c = a.normalize ? (float)d / (float)max(Lj, 1) : (float)d;
        W += wj;
        acc += wj * c;
    }
    const float r = acc / W;
    if (mine) { risk[lane] = r; row[lane * n + lane] = 0; }
    float v = mine ? r : __int_as_float(0x7f800000);
    int best = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int ob = __shfl_xor(best, o);
        if (ov < v || (ov == v && ob < best)) { v = ov; best = ob; }
    }
    if (lane == 0) a.best[g] = best;
}

// ---- text metrics of a pair (lxo_text_stats): clipped n-gram matches for n = 1 .. 4, lengths, distance, exact match ----
// A side's tokens are staged in LDS with token t at word t + 1, so that the walks below read four tokens per aligned 16-byte broadcast.  Words
// behind the sequence are zero, and NO comparison reaches them: an n-gram is compared only where it lies inside its sequence, by position, so any
// int32 value is a token.
constexpr int kTextWords = kEditMaxRef + 12;
typedef __attribute__((ext_vector_type(4))) int i32x4;

LXO_DEV void text_stage(int* s, const int* src, long long stride, int len, int lane) {
    for (int t = lane; t < len + 12; t += 64) s[t] = (t >= 1 && t <= len) ? src[(t - 1) * stride] : 0;
}

// Four positions j0 .. j0 + 3 of a walk: x holds the tokens j0 .. j0 + 6.  CHECK: position j counts only while bound - j >= 1, and then for every
// order (ALL) or for the orders n <= bound - j.
template <bool CHECK, bool ALL>
LXO_DEV void text_group(const int (&x)[7], int j0, int bound, int t0, int t1, int t2, int t3, int (&cnt)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int room = bound - (j0 + u);
        const bool e1 = (!CHECK || room >= 1) && x[u] == t0;
        const bool e2 = e1 && (!CHECK || ALL || room >= 2) && x[u + 1] == t1;
        const bool e3 = e2 && (!CHECK || ALL || room >= 3) && x[u + 2] == t2;
        const bool e4 = e3 && (!CHECK || ALL || room >= 4) && x[u + 3] == t3;
        cnt[0] += e1; cnt[1] += e2; cnt[2] += e3; cnt[3] += e4;
    }
}

// The lane holds the window (t0 .. t3) of its hypothesis position; cnt[n - 1] += the positions j < steps of the staged sequence s whose window agrees
// with it in the first n tokens.  PREFIX: s is the hypothesis itself and only j < bound (the lane's own position) count -- their n-grams lie inside
// the hypothesis wherever the lane's does.  Otherwise s is the reference of bound tokens and order n counts at j only while j + n <= bound.  The
// first `unchecked` positions (a multiple of 4, wave-uniform, <= steps) meet these limits in every lane and order and are compared without them.
// The next group's tokens are read while the current group is compared.
template <bool PREFIX>
LXO_DEV void text_walk(const int* s, int steps, int unchecked, int bound, int t0, int t1, int t2, int t3, int (&cnt)[4]) {
    int x[7] = {s[1], s[2], s[3], 0, 0, 0, 0};
    i32x4 q = *reinterpret_cast<const i32x4*>(s + 4);
    int j0 = 0;
    for (; j0 < unchecked; j0 += 4) {
        x[3] = q[0]; x[4] = q[1]; x[5] = q[2]; x[6] = q[3];
        q = *reinterpret_cast<const i32x4*>(s + j0 + 8);
        text_group<false, PREFIX>(x, j0, bound, t0, t1, t2, t3, cnt);
        x[0] = x[4]; x[1] = x[5]; x[2] = x[6];
    }
    for (; j0 < steps; j0 += 4) {
        x[3] = q[0]; x[4] = q[1]; x[5] = q[2]; x[6] = q[3];
        q = *reinterpret_cast<const i32x4*>(s + j0 + 8);
        text_group<true, PREFIX>(x, j0, bound, t0, t1, t2, t3, cnt);
        x[0] = x[4]; x[1] = x[5]; x[2] = x[6];
    }
}

// One wave per pair.  Hypothesis position i counts for order n iff the number k of EARLIER hypothesis positions with its n-gram is below the number c
// of reference positions with it: summed over i that is sum_g min(count_h(g), count_r(g)), the clipped matches, with no table of n-grams.  Lane l of
// each 64-position chunk owns one position and walks the hypothesis prefix and the reference once for all four orders.
template <int CPL>
__global__ __launch_bounds__(256) void text_stats_kernel(TextArgs a) {
    __shared__ __attribute__((aligned(16))) int tok[4][2 * kTextWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = blockIdx.x * 4 + wave;
    if (p >= a.pairs) return;
    const int r = min(max(a.ref_of ? a.ref_of[p] : p / a.per_ref, 0), a.G - 1);
    const int* hp = a.hyp + (long long)(p / a.hyp_block) * a.hb_stride + (long long)(p % a.hyp_block) * a.hr_stride;
    const int* rp = a.ref + (long long)r * a.ref_ld;
    // (the lengths are the same in every lane: held as scalars, the walks' loop control and position limits cost no vector work)
    const int m = __builtin_amdgcn_readfirstlane(cut_len(hp, a.ht_stride, min(a.hyp_len ? min(max(a.hyp_len[p], 0), a.T) : a.T, kEditMaxRef), a.id_end, lane));
    const int n = __builtin_amdgcn_readfirstlane(cut_len(rp, 1, min(a.ref_len ? min(max(a.ref_len[r], 0), a.ref_ld) : a.ref_ld, 64 * CPL), a.id_end, lane));
    int* hs = tok[__builtin_amdgcn_readfirstlane(wave)];
    int* rs = hs + kTextWords;
    text_stage(hs, hp, a.ht_stride, m, lane);
    text_stage(rs, rp, 1, n, lane);
    __builtin_amdgcn_wave_barrier();                                    // the wave's lanes exchange through its own LDS rows (in-order LDS: no s_barrier)

    int match[4] = {0, 0, 0, 0};
    for (int i0 = 0; i0 < m; i0 += 64) {
        const int i = i0 + lane, ic = min(i, m);
        const int t0 = hs[ic + 1], t1 = hs[ic + 2], t2 = hs[ic + 3], t3 = hs[ic + 4];
        int k[4] = {0, 0, 0, 0}, c[4] = {0, 0, 0, 0};
        text_walk<true>(hs, min(i0 + 63, m - 1), i0, i, t0, t1, t2, t3, k);                     // (every j < i0 lies in front of every lane)
        text_walk<false>(rs, n, max(n - 3, 0) / 4 * 4, n, t0, t1, t2, t3, c);                   // (groups whose last position j has j + 4 <= n)
#pragma unroll
        for (int o = 0; o < 4; ++o) match[o] += (int)__builtin_popcountll(__ballot(i + o < m && k[o] < c[o]));
    }
    bool same = m == n;
    for (int t0 = 0; t0 < m && same; t0 += 64) {
        const int t = min(t0 + lane, m);
        same = __ballot(hs[t + 1] != rs[t + 1]) == 0ull;
    }
    const int d = edit_wave<CPL>(hp, a.ht_stride, m, rp, 1, n, lane);
    // lane c holds value c of the row (the rows' columns, or the corpus' with max(|h|, |r|) slipped in and the pair count at the end): one store, or one
    // atomic instruction, of the wave
    const int row[kTextCorpus] = {match[0], match[1], match[2], match[3], max(1, m), max(1, m - 1), max(1, m - 2), max(1, m - 3), m, n, d,
                                  a.stats ? (same ? 1 : 0) : max(m, n), same ? 1 : 0, p == 0 ? a.pairs : 0};
    int v = 0;
#pragma unroll
    for (int c = 0; c < kTextCorpus; ++c) if (lane == c) v = row[c];
    if (a.stats) {
        if (lane < kTextStats) a.stats[(long long)p * kTextStats + lane] = v;
    } else if (lane < kTextCorpus) {
        // no rows to reduce: 64-bit integer adds, whose sum is the same in every order
        atomicAdd(reinterpret_cast<unsigned long long*>(a.corpus) + lane, (unsigned long long)v);
    }
}

// Launch 2, one workgroup: the column sums of the rows in a fixed order (thread t takes the rows t, t + 256, ..; then the wave, then the four waves),
// written to or added into the corpus row.
__global__ __launch_bounds__(256) void text_corpus_kernel(const int* stats, int pairs, long long* corpus, int accumulate) {
    __shared__ long long part[4][kTextCorpus - 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long s[kTextCorpus - 1];
#pragma unroll
    for (int c = 0; c < kTextCorpus - 1; ++c) s[c] = 0;
    for (int p = threadIdx.x; p < pairs; p += 256) {
        const int* row = stats + (long long)p * kTextStats;
#pragma unroll
        for (int c = 0; c < 11; ++c) s[c] += row[c];
        s[11] += max(row[8], row[9]);
        s[12] += row[11];
    }
#pragma unroll
    for (int c = 0; c < kTextCorpus - 1; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[c] += __shfl_xor(s[c], o);
        if (lane == 0) part[wave][c] = s[c];
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < kTextCorpus) {
        const long long v = c == kTextCorpus - 1 ? (long long)pairs : part[0][c] + part[1][c] + part[2][c] + part[3][c];
        corpus[c] = (accumulate ? corpus[c] : 0ll) + v;
    }
}

// ---- sentence-level BLEU of a pair (lxo_sentence_bleu), and as the cost of a consensus (lxo_consensus_bleu) ----
// The steps of text_stats_kernel and cons_select_kernel that the kernels below share, as functions.  (Those two kernels keep the steps in their own
// bodies: calling the functions there moved a few of their instructions, and their code objects stay what they were.)
// The clipped matches of a staged pair, match[n - 1] += sum_g min(count_h(g), count_r(g)) for the orders n = 1 .. 4 -- text_stats_kernel's counting identity, lane l
// of each 64-position chunk owning one hypothesis position -- and whether the two staged sequences are equal (equal length, equal tokens).
LXO_DEV void text_matches(const int* hs, int m, const int* rs, int n, int lane, int (&match)[4]) {
    for (int i0 = 0; i0 < m; i0 += 64) {
        const int i = i0 + lane, ic = min(i, m);
        const int t0 = hs[ic + 1], t1 = hs[ic + 2], t2 = hs[ic + 3], t3 = hs[ic + 4];
        int k[4] = {0, 0, 0, 0}, c[4] = {0, 0, 0, 0};
        text_walk<true>(hs, min(i0 + 63, m - 1), i0, i, t0, t1, t2, t3, k);                     // (every j < i0 lies in front of every lane)
        text_walk<false>(rs, n, max(n - 3, 0) / 4 * 4, n, t0, t1, t2, t3, c);                   // (groups whose last position j has j + 4 <= n)
#pragma unroll
        for (int o = 0; o < 4; ++o) match[o] += (int)__builtin_popcountll(__ballot(i + o < m && k[o] < c[o]));
    }
}
LXO_DEV bool text_same(const int* hs, int m, const int* rs, int n, int lane) {
    bool same = m == n;
    for (int t0 = 0; t0 < m && same; t0 += 64) {
        const int t = min(t0 + lane, m);
        same = __ballot(hs[t + 1] != rs[t + 1]) == 0ull;
    }
    return same;
}

// The weight of lane i's draw as the select kernels read it: negative, NaN or infinite counts as 0, a row that sums to 0 as all ones (NULL: ones).
LXO_DEV float cons_weight(const float* weights, int g, int n, int lane, bool mine) {
    float w = 1.f;
    if (weights) {
        w = mine ? weights[(long long)g * n + lane] : 0.f;
        if (!(w > 0.f) || !(w - w == 0.f)) w = 0.f;                                    // negative, NaN, infinite: 0
        float sum = 0.f;
        for (int j = 0; j < n; ++j) sum += __shfl(w, j);
        if (sum == 0.f) w = 1.f;
    }
    return w;
}
// The lane of the smallest r among the lanes that hold a draw, the lower lane on ties; in every lane.
LXO_DEV int cons_argmin(float r, bool mine, int lane) {
    float v = mine ? r : __int_as_float(0x7f800000);
    int best = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int ob = __shfl_xor(best, o);
        if (ov < v || (ov == v && ob < best)) { v = ov; best = ob; }
    }
    return best;
}

// The score of include/lxo.h from the clipped matches of a hypothesis of m tokens against a reference of n: add-one smoothing on the orders 2 .. 4,
// the brevity penalty, 1 for an equal pair and 0 without a common unigram.  Lane-uniform values in, f32 throughout, one division per order.
LXO_DEV float sbleu(const int (&match)[4], int m, int n, bool same) {
#pragma clang fp contract(off)
    if (same) return 1.f;
    if (match[0] == 0) return 0.f;                                      // (an empty hypothesis included: below, m >= 1)
    float s = logf((float)match[0] / (float)m);
#pragma unroll
    for (int o = 1; o < 4; ++o) s += logf((float)(match[o] + 1) / (float)(max(1, m - o) + 1));
    const float bp = m > n ? 1.f : expf(1.f - (float)n / (float)m);
    return bp * expf(0.25f * s);
}

// One wave per pair, as text_stats_kernel without the DP: both sides staged, one walk for the four orders, the ballot compare, the float tail.
__global__ __launch_bounds__(256) void bleu_pairs_kernel(BleuArgs a) {
    __shared__ __attribute__((aligned(16))) int tok[4][2 * kTextWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = blockIdx.x * 4 + wave;
    if (p >= a.pairs) return;
    if (a.live && p >= a.live[0]) {                                     // a dead candidate row: nothing read, no cost
        if (lane < kBleuCounts && a.counts) a.counts[(long long)p * kBleuCounts + lane] = 0;
        if (lane == 0) { if (a.bleu) a.bleu[p] = 1.f; if (a.cost) a.cost[p] = 0.f; }
        return;
    }
    const int r = min(max(a.ref_of ? a.ref_of[p] : p / a.per_ref, 0), a.G - 1);
    const int* hp = a.hyp + (long long)(p / a.hyp_block) * a.hb_stride + (long long)(p % a.hyp_block) * a.hr_stride;
    const int* rp = a.ref + (long long)r * a.ref_ld;
    const int m = __builtin_amdgcn_readfirstlane(cut_len(hp, a.ht_stride, min(a.hyp_len ? min(max(a.hyp_len[p], 0), a.T) : a.T, kEditMaxRef), a.id_end, lane));
    const int n = __builtin_amdgcn_readfirstlane(cut_len(rp, 1, min(a.ref_len ? min(max(a.ref_len[r], 0), a.ref_ld) : a.ref_ld, kEditMaxRef), a.id_end, lane));
    int* hs = tok[__builtin_amdgcn_readfirstlane(wave)];
    int* rs = hs + kTextWords;
    text_stage(hs, hp, a.ht_stride, m, lane);
    text_stage(rs, rp, 1, n, lane);
    __builtin_amdgcn_wave_barrier();

    int match[4] = {0, 0, 0, 0};
    const bool same = text_same(hs, m, rs, n, lane);
    if (same) {
#pragma unroll
        for (int o = 0; o < 4; ++o) match[o] = max(0, m - o);           // every n-gram of h against itself
    } else {
        text_matches(hs, m, rs, n, lane, match);
    }
    const float b = sbleu(match, m, n, same);
    if (a.counts) {
        const int row[kBleuCounts] = {match[0], match[1], match[2], match[3], max(1, m), max(1, m - 1), max(1, m - 2), max(1, m - 3), m, n};
        int v = 0;
#pragma unroll
        for (int c = 0; c < kBleuCounts; ++c) if (lane == c) v = row[c];
        if (lane < kBleuCounts) a.counts[(long long)p * kBleuCounts + lane] = v;
    }
    if (lane == 0) { if (a.bleu) a.bleu[p] = b; if (a.cost) a.cost[p] = 1.f - b; }
}

// Consensus, launch 1: one wave per unordered pair (g, i < j), enumerated as cons_pairs_kernel does.  The clipped matches are symmetric in the two draws,
// so one count serves c(i, j) -- draw j the reference -- and c(j, i); only the totals and the brevity penalty change sides.  Equal draws skip the walk.
// The waves of the pairs (0, j) write the diagonal of match_out (a draw against itself: its own n-grams).
__global__ __launch_bounds__(256) void cons_bleu_pairs_kernel(ConsBleuArgs a, int per) {
    __shared__ __attribute__((aligned(16))) int tok[4][2 * kTextWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, w = blockIdx.x * 4 + wave;
    if (w >= a.B * per) return;
    const int g = w / per;
    int q = w % per, i = 0;
    while (q >= a.n - 1 - i) { q -= a.n - 1 - i; ++i; }
    const int j = i + 1 + q;
    const int* pi = cons_draw(a.ids, a.image_stride, a.draw_stride, g, i);
    const int* pj = cons_draw(a.ids, a.image_stride, a.draw_stride, g, j);
    const int Li = __builtin_amdgcn_readfirstlane(cut_len(pi, a.tok_stride, min(a.T, kEditMaxRef), a.id_end, lane));
    const int Lj = __builtin_amdgcn_readfirstlane(cut_len(pj, a.tok_stride, min(a.T, kEditMaxRef), a.id_end, lane));
    int* si = tok[__builtin_amdgcn_readfirstlane(wave)];
    int* sj = si + kTextWords;
    text_stage(si, pi, a.tok_stride, Li, lane);
    text_stage(sj, pj, a.tok_stride, Lj, lane);
    __builtin_amdgcn_wave_barrier();

    int match[4] = {0, 0, 0, 0};
    const bool same = text_same(si, Li, sj, Lj, lane);
    if (same) {
#pragma unroll
        for (int o = 0; o < 4; ++o) match[o] = max(0, Li - o);
    } else {
        text_matches(si, Li, sj, Lj, lane, match);
    }
    const float cij = 1.f - sbleu(match, Li, Lj, same), cji = 1.f - sbleu(match, Lj, Li, same);
    const long long n = a.n;
    if (lane == 0) {
        float* row = a.cost + g * n * n;
        row[i * n + j] = cij;
        row[j * n + i] = cji;
    }
    if (a.match && lane < 4) {
        int v = 0;
#pragma unroll
        for (int o = 0; o < 4; ++o) if (lane == o) v = match[o];
        int* row = a.match + g * n * n * 4;
        row[(i * n + j) * 4 + lane] = v;
        row[(j * n + i) * 4 + lane] = v;
        if (i == 0) {
            row[(j * n + j) * 4 + lane] = max(0, Lj - lane);
            if (j == 1) row[lane] = max(0, Li - lane);
        }
    }
}

// Consensus, launch 2: cons_select_kernel on the f32 cost matrix -- the same weights, ascending-j sums without fused multiply-add, arg-min and ties; the
// diagonal of the costs is written here (and with one draw, which no pair wave saw, the diagonal of match_out).
__global__ __launch_bounds__(256) void cons_bleu_select_kernel(ConsBleuArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + (threadIdx.x >> 6), n = a.n;
    if (g >= a.B) return;
    const bool mine = lane < n;
    float* row = a.cost + (long long)g * n * n;
    if (n == 1 && a.match) {
        const int L = cut_len(cons_draw(a.ids, a.image_stride, a.draw_stride, g, 0), a.tok_stride, min(a.T, kEditMaxRef), a.id_end, lane);
        if (lane < 4) a.match[(long long)g * 4 + lane] = max(0, L - lane);
    }
    const float w = cons_weight(a.weights, g, n, lane, mine);
    float W = 0.f, acc = 0.f;
    for (int j = 0; j < n; ++j) {
        const float wj = __shfl(w, j);
        const float c = mine && lane != j ? row[lane * n + j] : 0.f;
        W += wj;
        acc += wj * c;
    }
    const float r = acc / W;
    if (mine) { a.risk[(long long)g * n + lane] = r; row[lane * n + lane] = 0.f; }
    const int best = cons_argmin(r, mine, lane);
    if (lane == 0) a.best[g] = best;
}

// ---- edit alignment of a pair (lxo_edit_align): the path through the table edit_wave fills ----
// The forward phase is edit_wave's row step with the path kept: once a row's values are final a lane holds, for every cell (i, j) of its strip, the cell
// (cur), the cell above (prev) and the cell above-left (prev of the column to the left) -- what the path rule of include/lxo.h reads: 0 a diagonal step
// if cur == above-left + (x != b), else 1 an insertion if cur == above + 1, else 2 a deletion.  The 2-bit steps of the strip, column e in bits 2e, 2e + 1,
// are one dword of the lane; the 64 dwords of row i (1 .. m) are stored as one coalesced row at steps[(i - 1) 64 + lane].  Row 0 and column 0 are implied
// (deletions and insertions).  (A template of its own beside edit_wave: the kernels built on edit_wave keep their instructions.)
template <int CPL>
LXO_DEV void align_forward(const int* hp, long long hts, int m, const int* rp, int n, int lane, unsigned* steps) {
    int b[CPL], prev[CPL];
#pragma unroll
    for (int e = 0; e < CPL; ++e) {
        const int j = lane * CPL + e;
        b[e] = j < n ? rp[j] : -1;
        prev[e] = j + 1;
    }
    for (int i0 = 0; i0 < m; i0 += 64) {
        const int xi = hp[(i0 + lane < m ? i0 + lane : i0) * hts];
        const int cnt = min(64, m - i0);
        for (int k = 0; k < cnt; ++k) {
            const int x = __shfl(xi, k), i = i0 + k + 1;
            int left = __shfl_up(prev[CPL - 1], 1);
            if (lane == 0) left = i - 1;
            int s[CPL], run = 0x3fffffff;
#pragma unroll
            for (int e = 0; e < CPL; ++e) {
                const int diag = e ? prev[e - 1] : left;
                const int t = min(prev[e] + 1, diag + (x != b[e] ? 1 : 0));
                run = min(run, t - (lane * CPL + e + 1));
                s[e] = run;
            }
            int v = lane == 0 ? min(run, i) : run;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(v, d);
                if (lane >= d) v = min(v, o);
            }
            int ex = __shfl_up(v, 1);
            if (lane == 0) ex = i;
            unsigned w = 0;
            int diag = left;
#pragma unroll
            for (int e = 0; e < CPL; ++e) {
                const int cur = lane * CPL + e + 1 + min(s[e], ex);
                const unsigned step = cur == diag + (x != b[e] ? 1 : 0) ? 0u : (cur == prev[e] + 1 ? 1u : 2u);
                w |= step << (2 * e);
                diag = prev[e];
                prev[e] = cur;
            }
            steps[(long long)(i - 1) * 64 + lane] = w;
        }
    }
}

constexpr int kAlignAhead = 8;      // step rows the backtrace loads in one go, a second set in flight behind them

// The rows i, i - 1, .. of the steps, the lane's own dword of each (row numbers below 1 repeat row 1: loaded, never walked)
LXO_DEV void align_rows(unsigned (&w)[kAlignAhead], const unsigned* steps, int i, int lane) {
#pragma unroll
    for (int u = 0; u < kAlignAhead; ++u) w[u] = steps[(long long)(max(i - u, 1) - 1) * 64 + lane];
}

// One wave per pair.  (a) align_forward.  (b) The walk back from (m, n): the path is serial in (i, j), but the row it reads next is not path-dependent --
// a row is left by exactly one diagonal or insertion step -- so the rows are loaded kAlignAhead at a time, the next set while the current one is walked,
// and within a row the run of deletions left of j is resolved on the wave: every lane masks its strip to the columns <= j, a ballot finds the last lane
// with a step that is no deletion and one shuffle fetches its column and kind.  i and j stay wave-uniform scalars; a row costs no dependent load.  Both
// maps are staged in LDS as int16 with the defaults an unvisited position has (-1: inserted / deleted, -2: behind the sequence), so the walk stores the
// diagonal steps only.  (c) The maps go out coalesced, one lane per position enters its step in the confusion matrix, the counts are reduced over the wave.
template <int CPL>
__global__ __launch_bounds__(256) void align_kernel(AlignArgs a) {
    __shared__ short map[4][2 * kEditMaxRef];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = blockIdx.x * 4 + wave;
    if (p >= a.pairs) return;
    const int r = min(max(a.ref_of ? a.ref_of[p] : p / a.per_ref, 0), a.G - 1);
    const int* hp = a.hyp + (long long)(p / a.hyp_block) * a.hb_stride + (long long)(p % a.hyp_block) * a.hr_stride;
    const int* rp = a.ref + (long long)r * a.ref_ld;
    const int m = __builtin_amdgcn_readfirstlane(cut_len(hp, a.ht_stride, min(a.hyp_len ? min(max(a.hyp_len[p], 0), a.T) : a.T, kEditMaxRef), a.id_end, lane));
    const int n = __builtin_amdgcn_readfirstlane(cut_len(rp, 1, min(a.ref_len ? min(max(a.ref_len[r], 0), a.ref_ld) : a.ref_ld, 64 * CPL), a.id_end, lane));
    short* ha = map[__builtin_amdgcn_readfirstlane(wave)];
    short* ra = ha + kEditMaxRef;
    for (int t = lane; t < kEditMaxRef; t += 64) { ha[t] = t < m ? -1 : -2; ra[t] = t < n ? -1 : -2; }
    __builtin_amdgcn_wave_barrier();

    if (m > 0 && n > 0) {
        unsigned* steps = a.steps + (long long)p * a.T * 64;
        align_forward<CPL>(hp, a.ht_stride, m, rp, n, lane, steps);
        // The step rows are read back by the wave that stored them, every lane the dwords it wrote itself: nothing crosses lanes through memory.  The
        // stores must have left the wave before the first load of the walk is issued: wait for the outstanding vector-memory operations (vmcnt(0)).
        __builtin_amdgcn_s_waitcnt(0x0F70);
        int i = m, j = n;
        unsigned w[kAlignAhead], ahead[kAlignAhead];
        align_rows(w, steps, i, lane);
        while (i > 0 && j > 0) {
            align_rows(ahead, steps, i - kAlignAhead, lane);
#pragma unroll
            for (int u = 0; u < kAlignAhead; ++u) {
                if (i <= 0 || j <= 0) break;
                const int k = min(max(j - lane * CPL, 0), CPL);                          // columns of the strip at or left of j
                const unsigned keep = k >= 16 ? 0xffffffffu : (1u << (2 * k)) - 1u;
                const unsigned stay = ~(w[u] >> 1) & 0x55555555u & keep;                 // bit 2e: column e leaves the row (a diagonal step or an insertion)
                const unsigned long long any = __ballot(stay != 0u);
                if (!any) { j = 0; break; }                                              // deletions down to column 0; the rows above are insertions: the defaults
                const int L = 63 - (int)__builtin_clzll(any);
                const int e = (31 - (int)__builtin_clz(stay | 1u)) >> 1;
                const int got = __builtin_amdgcn_readfirstlane(__shfl((int)((e << 2) | ((w[u] >> (2 * e)) & 3u)), L));
                const int jj = L * CPL + (got >> 2) + 1;                                 // the columns jj + 1 .. j are deleted: the defaults
                if ((got & 3) == 0) {
                    if (lane == 0) { ha[i - 1] = (short)(jj - 1); ra[jj - 1] = (short)(i - 1); }
                    j = jj - 1;
                } else {
                    j = jj;
                }
                --i;
            }
#pragma unroll
            for (int u = 0; u < kAlignAhead; ++u) w[u] = ahead[u];
        }
    }
    __builtin_amdgcn_wave_barrier();                                    // lane 0's LDS stores, read by every lane below (in-order LDS: no s_barrier)

    const int V = a.V;
    const long long ld = (long long)V + 1;
    unsigned long long* conf = reinterpret_cast<unsigned long long*>(a.confusion);
    int cM = 0, cS = 0, cI = 0, cD = 0, out = 0;
    for (int t0 = 0; t0 < a.T; t0 += 64) {
        const int t = t0 + lane;
        if (t >= a.T) break;
        const int v = ha[t];
        if (a.hyp_align) a.hyp_align[(long long)p * a.T + t] = v;
        if (t >= m) continue;
        const int hb = hp[t * a.ht_stride], rb = v >= 0 ? rp[v] : 0;
        if (v < 0) ++cI; else if (hb == rb) ++cM; else ++cS;
        if (conf) {
            if (hb >= 0 && hb < V && rb >= 0 && rb < V) atomicAdd(conf + (v >= 0 ? rb : V) * ld + hb, 1ull);
            else ++out;
        }
    }
    for (int t0 = 0; t0 < a.ref_ld; t0 += 64) {
        const int t = t0 + lane;
        if (t >= a.ref_ld) break;
        const int v = ra[t];
        if (a.ref_align) a.ref_align[(long long)p * a.ref_ld + t] = v;
        if (t >= n || v >= 0) continue;
        ++cD;
        if (conf) {
            const int rb = rp[t];
            if (rb >= 0 && rb < V) atomicAdd(conf + rb * ld + V, 1ull);
            else ++out;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cM += __shfl_xor(cM, o); cS += __shfl_xor(cS, o); cI += __shfl_xor(cI, o); cD += __shfl_xor(cD, o); out += __shfl_xor(out, o);
    }
    // lane c holds value c of the row (the counts, then the pair count and the steps left out of the matrix): one store and one atomic instruction of the wave
    const int row[kAlignCorpus] = {cM, cS, cI, cD, m, n, p == 0 ? a.pairs : 0, out};
    int v = 0;
#pragma unroll
    for (int c = 0; c < kAlignCorpus; ++c) if (lane == c) v = row[c];
    if (a.counts && lane < kAlignCounts) a.counts[(long long)p * kAlignCounts + lane] = v;
    // 64-bit integer adds, whose sum is the same in every order
    if (a.corpus && lane < kAlignCorpus) atomicAdd(reinterpret_cast<unsigned long long*>(a.corpus) + lane, (unsigned long long)v);
}

// What a call overwrites is zeroed by a launch in front of the pair waves, which add into it: the corpus row by the first threads, the matrix grid-stride.
__global__ __launch_bounds__(256) void align_zero_kernel(long long* corpus, long long* confusion, long long cells) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (corpus && t < kAlignCorpus) corpus[t] = 0;
    if (confusion)
        for (long long c = t; c < cells; c += (long long)gridDim.x * 256) confusion[c] = 0;
}

}  // namespace

#define LAUNCH(kern, grid, ...) hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, __VA_ARGS__)

int lxo_k_edit_distance(const EditArgs& a, hipStream_t st) {
    if (a.ref_ld > kEditMaxRef) return -2;
    if (a.pairs == 0) return 0;
    const int grid = cdiv(a.pairs, 4);
    if (a.ref_ld <= 64) LAUNCH(edit_kernel<1>, grid, a);
    else if (a.ref_ld <= 128) LAUNCH(edit_kernel<2>, grid, a);
    else if (a.ref_ld <= 256) LAUNCH(edit_kernel<4>, grid, a);
    else if (a.ref_ld <= 512) LAUNCH(edit_kernel<8>, grid, a);
    else LAUNCH(edit_kernel<16>, grid, a);
    return (int)hipGetLastError();
}

int lxo_k_edit_align(const AlignArgs& a, hipStream_t st) {
    if (a.ref_ld > kEditMaxRef || a.T > kEditMaxRef) return -2;
    // what is overwritten is zeroed first: the waves add into it (a launch, as lxo_k_text_stats zeroes its row)
    if (!a.accumulate && (a.corpus || a.confusion)) {
        const long long cells = a.confusion ? ((long long)a.V + 1) * ((long long)a.V + 1) : 0;
        LAUNCH(align_zero_kernel, (int)min(max((cells + 255) / 256, 1ll), 1024ll), a.corpus, a.confusion, cells);
    }
    if (a.pairs == 0) return (int)hipGetLastError();
    const int grid = cdiv(a.pairs, 4);
    if (a.ref_ld <= 64) LAUNCH(align_kernel<1>, grid, a);
    else if (a.ref_ld <= 128) LAUNCH(align_kernel<2>, grid, a);
    else if (a.ref_ld <= 256) LAUNCH(align_kernel<4>, grid, a);
    else if (a.ref_ld <= 512) LAUNCH(align_kernel<8>, grid, a);
    else LAUNCH(align_kernel<16>, grid, a);
    return (int)hipGetLastError();
}

int lxo_k_sentence_bleu(const BleuArgs& a, hipStream_t st) {
    if (a.ref_ld > kEditMaxRef || a.T > kEditMaxRef) return -2;
    if (a.pairs == 0) return 0;
    LAUNCH(bleu_pairs_kernel, cdiv(a.pairs, 4), a);
    return (int)hipGetLastError();
}

int lxo_k_mrt_candidates(const CandArgs& a, hipStream_t st, int cost_kind) {
    if (a.Tr > kEditMaxRef || (cost_kind && a.steps + 1 > kEditMaxRef)) return -2;
    if (a.B == 0) return (int)hipMemsetAsync(a.group_off, 0, sizeof(int), st);
    int* slot = reinterpret_cast<int*>(a.cost);
    LAUNCH(cand_analyse_kernel, a.B, a, slot);
    LAUNCH(cand_emit_kernel, a.B, a, slot);
    const int Tc = a.steps + 1 > a.Tr ? a.steps + 1 : a.Tr;
    EditArgs e = {a.cand, nullptr, a.ref, a.ref_len, a.row_image, a.group_off + a.B, nullptr, a.cost, Tc, 0, 1, 1, Tc, a.B, a.Tr, 1,
                  a.B * (a.n + a.inc), a.id_end};
    if (!cost_kind) return lxo_k_edit_distance(e, st);
    const BleuArgs b = {e.hyp, e.hyp_len, e.ref, e.ref_len, e.ref_of, e.live, nullptr, nullptr, e.cost, e.hb_stride, e.hr_stride, e.ht_stride,
                        e.hyp_block, e.T, e.G, e.ref_ld, e.per_ref, e.pairs, e.id_end};
    return lxo_k_sentence_bleu(b, st);
}

int lxo_k_consensus(const ConsArgs& a, hipStream_t st) {
    if (a.T > kEditMaxRef || a.n > kConsensusMaxN) return -2;
    if (a.B == 0) return 0;
    const long long per = (long long)a.n * (a.n - 1) / 2, waves = per * a.B;
    if (waves > 0x7ffffff0ll) return -2;
    if (waves) {
        const int grid = (int)((waves + 3) / 4), p = (int)per;
        if (a.T <= 64) LAUNCH(cons_pairs_kernel<1>, grid, a, p);
        else if (a.T <= 128) LAUNCH(cons_pairs_kernel<2>, grid, a, p);
        else if (a.T <= 256) LAUNCH(cons_pairs_kernel<4>, grid, a, p);
        else if (a.T <= 512) LAUNCH(cons_pairs_kernel<8>, grid, a, p);
        else LAUNCH(cons_pairs_kernel<16>, grid, a, p);
    }
    LAUNCH(cons_select_kernel, cdiv(a.B, 4), a);
    return (int)hipGetLastError();
}

int lxo_k_consensus_bleu(const ConsBleuArgs& a, hipStream_t st) {
    if (a.T > kEditMaxRef || a.n > kConsensusMaxN) return -2;
    if (a.B == 0) return 0;
    const long long per = (long long)a.n * (a.n - 1) / 2, waves = per * a.B;
    if (waves > 0x7ffffff0ll) return -2;
    if (waves) LAUNCH(cons_bleu_pairs_kernel, (int)((waves + 3) / 4), a, (int)per);
    LAUNCH(cons_bleu_select_kernel, cdiv(a.B, 4), a);
    return (int)hipGetLastError();
}

int lxo_k_text_stats(const TextArgs& a, hipStream_t st) {
    if (a.ref_ld > kEditMaxRef || a.T > kEditMaxRef) return -2;
    // a corpus row that is overwritten without rows to reduce (no pair, or no stats: the waves add into it) is zeroed first -- the reduction over no row
    if (a.corpus && !a.accumulate && (a.pairs == 0 || !a.stats)) LAUNCH(text_corpus_kernel, 1, (const int*)nullptr, 0, a.corpus, 0);
    if (a.pairs == 0) return (int)hipGetLastError();
    const int grid = cdiv(a.pairs, 4);
    if (a.ref_ld <= 64) LAUNCH(text_stats_kernel<1>, grid, a);
    else if (a.ref_ld <= 128) LAUNCH(text_stats_kernel<2>, grid, a);
    else if (a.ref_ld <= 256) LAUNCH(text_stats_kernel<4>, grid, a);
    else if (a.ref_ld <= 512) LAUNCH(text_stats_kernel<8>, grid, a);
    else LAUNCH(text_stats_kernel<16>, grid, a);
    if (a.stats && a.corpus) LAUNCH(text_corpus_kernel, 1, a.stats, a.pairs, a.corpus, a.accumulate);
    return (int)hipGetLastError();
}
