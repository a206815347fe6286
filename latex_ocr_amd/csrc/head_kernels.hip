// The output head: every kernel that reads a row of logits and turns it into a loss (ce_loss*, weighted or not), a log-prob (score*), a choice list
// (score_alt*) or a token (argmax_kernel, beam_step*), the minimum-risk weights made from sequence log-probs (mrt_*), their launchers, and -- first --
// the row steps they are made of.
#include "head_kernels.h"
#include "drop.h"
#include "switches.h"

namespace {

// ---- row steps ----
// Every step of the head exists once, here; a kernel below only says which steps it takes and where the result goes.  A new head feature
// (a tie rule, a temperature, a length penalty, another mask) goes into these helpers, never into a kernel.

// Forced prefix (PF instantiations of the decode kernels, DecPrefix in head_kernels.h): row r emits ids[r][t] at steps t < len[r].  What
// the device holds is read defensively -- a length is clamped into [0, lim], lim = min(ld, max_iter), and an id outside [0, V) is read as
// 0 -- so that no caller error faults.
LXO_DEV int pfx_len(const DecPrefix& q, int r) { return min(max(q.len[r], 0), q.lim); }
LXO_DEV int pfx_id(const DecPrefix& q, int r, int t, int V) { const int f = q.ids[(long long)r * q.ld + t]; return (f >= 0 && f < V) ? f : 0; }
// Allowed-token sets (AL instantiations, DecAllow in head_kernels.h): a banned column is a column outside the vocabulary -- its logit is
// -inf before anything else happens in the select step.  The words of a row are read inside [0, (V + 31) / 32): nothing faults on any content.
LXO_DEV const unsigned* alw_row(const DecAllow& q, int r) { return q.bits + (long long)r * q.ld; }
// the set of decoder row `row` of image b: the image's, or under a grammar the row's own
LXO_DEV const unsigned* alw_row(const DecAllow& q, int b, int row) { return q.bits + (long long)(q.per_row ? row : b) * q.ld; }
// beam kernels: words between the sets of an image's consecutive hypothesis slots (0: they share the image's set)
LXO_DEV long long alw_slot_stride(const DecAllow& q) { return q.per_row ? q.ld : 0; }
LXO_DEV bool alw_ok(const unsigned* row, int v) { return (row[v >> 5] >> (v & 31)) & 1u; }

// Register row (Vp <= 64 * KV): 16-byte loads, a lane owns 4 consecutive columns per quarter of KV; the load is unconditional (clamped) and a
// column >= V reads as -3.0e38f
template <int KV>
LXO_DEV void row_load(const float* lg, int lane, int V, int Vp, float (&x)[KV]) {
#pragma unroll
    for (int q = 0; q < KV / 4; ++q) {
        const int j0 = 4 * (lane + 64 * q);
        const f32x4 v = *reinterpret_cast<const f32x4*>(lg + (j0 < Vp ? j0 : 0));
#pragma unroll
        for (int e = 0; e < 4; ++e) x[4 * q + e] = (j0 + e < V) ? v[e] : -3.0e38f;
    }
}
// e^x of the register-row kernels: v_exp_f32 (1 ulp) in bf16 mode, expf in f32 parity mode
template <bool FAST> LXO_DEV float row_exp(float x) { return FAST ? __expf(x) : expf(x); }
// its log-sum-exp, every lane's
template <bool FAST, int KV>
LXO_DEV float row_lse(const float (&x)[KV]) {
    float m = x[0];
#pragma unroll
    for (int e = 1; e < KV; ++e) m = fmaxf(m, x[e]);
    m = wave_max(m);
    float l = 0.f;
#pragma unroll
    for (int e = 0; e < KV; ++e) l += row_exp<FAST>(x[e] - m);
    l = wave_sum(l);
    return m + logf(l);
}

// Strided row (any V): a lane takes columns lane, lane + 64, ...; AL: the banned ones are skipped.  The wave's exp-sum around a given max ...
template <bool AL>
LXO_DEV float strided_expsum(const float* lg, int lane, int V, const unsigned* ar, float m) {
    float l = 0.f;
    for (int j = lane; j < V; j += 64) if (!AL || alw_ok(ar, j)) l += expf(lg[j] - m);
    return wave_sum(l);
}
// ... and its log-sum-exp, around its own
template <bool AL>
LXO_DEV float strided_lse(const float* lg, int lane, int V, const unsigned* ar) {
    float m = -3.0e38f;
    for (int j = lane; j < V; j += 64) if (!AL || alw_ok(ar, j)) m = fmaxf(m, lg[j]);
    m = wave_max(m);
    return m + logf(strided_expsum<AL>(lg, lane, V, ar, m));
}
// a lane's first maximum of such a row (strict >, ascending columns); a wave arg-max follows
template <bool AL>
LXO_DEV void strided_argmax(const float* lg, int lane, int V, const unsigned* ar, float& best, int& bi) {
    best = -3.0e38f; bi = 0x7fffffff;
    for (int j = lane; j < V; j += 64) { const float x = lg[j]; if ((!AL || alw_ok(ar, j)) && x > best) { best = x; bi = j; } }
}

// Lane-register row (V <= 64 * N): columns lane + 64 u, every load requested (clamped index) before anything is reduced, masked by V and AL
template <int N, bool AL>
LXO_DEV float lane_row_lse(const float* lg, int lane, int V, const unsigned* ar) {
    float x[N];
#pragma unroll
    for (int u = 0; u < N; ++u) { const int c = lane + 64 * u; x[u] = lg[c < V ? c : V - 1]; }
    float m = -3.0e38f;
#pragma unroll
    for (int u = 0; u < N; ++u) if (lane + 64 * u < V && (!AL || alw_ok(ar, lane + 64 * u))) m = fmaxf(m, x[u]);
    m = wave_max(m);
    float l = 0.f;
#pragma unroll
    for (int u = 0; u < N; ++u) if (lane + 64 * u < V && (!AL || alw_ok(ar, lane + 64 * u))) l += expf(x[u] - m);
    l = wave_sum(l);
    return m + logf(l);
}

// (value, index) arg-max over the 64 lanes of a wave -- value descending, index ascending -- every lane ends with the winner: the shuffle butterfly ...
LXO_DEV void shfl_argmax(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o); const int oi = __shfl_xor(i, o);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}
// ... and the one without LDS crossbar round trips: the four steps inside a row of 16 lanes are DPP moves, the two across rows permlane swaps
// (as bm_wave_sum_dpp of decoder_kernels.hip)
#ifdef LXO_HIPSIM
LXO_DEV void wave_argmax(float& v, int& i) { shfl_argmax(v, i); }
#else
template <int CTRL> LXO_DEV void amax_dpp(float& v, int& i) {
    const float ov = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
    const int oi = __builtin_amdgcn_update_dpp(0, i, CTRL, 0xf, 0xf, true);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
LXO_DEV void wave_argmax(float& v, int& i) {
    amax_dpp<0xB1>(v, i); amax_dpp<0x4E>(v, i); amax_dpp<0x141>(v, i); amax_dpp<0x140>(v, i);
    {
        const auto rv = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        const auto ri = __builtin_amdgcn_permlane16_swap((unsigned)i, (unsigned)i, false, false);
        const float v0 = __uint_as_float(rv[0]), v1 = __uint_as_float(rv[1]); const int i0 = (int)ri[0], i1 = (int)ri[1];
        const bool first = v0 > v1 || (v0 == v1 && i0 < i1);
        v = first ? v0 : v1; i = first ? i0 : i1;
    }
    {
        const auto rv = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        const auto ri = __builtin_amdgcn_permlane32_swap((unsigned)i, (unsigned)i, false, false);
        const float v0 = __uint_as_float(rv[0]), v1 = __uint_as_float(rv[1]); const int i0 = (int)ri[0], i1 = (int)ri[1];
        const bool first = v0 > v1 || (v0 == v1 && i0 < i1);
        v = first ? v0 : v1; i = first ? i0 : i1;
    }
}
#endif

// Alternatives (the score_alt kernels): the k first columns of a row, the target's rank and the step's entropy.  ONE total order on the raw
// f32 logits -- value descending, then column ascending -- and `alt_before` is the only place that states it.
LXO_DEV bool alt_before(float x, int c, float y, int d) { return x > y || (x == y && c < d); }      // (x, c) comes strictly before (y, d)
LXO_DEV int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// Register row: bit 4 q + e of the result = the lane's column 4 (lane + 64 q) + e counts (inside [0, V), AL: and allowed); AL: a banned column is
// masked here, right after the load, to the value a column >= V carries
template <int KV, bool AL>
LXO_DEV unsigned row_counts(int lane, int V, const unsigned* ar, float (&x)[KV]) {
    unsigned ok = 0u;
#pragma unroll
    for (int q = 0; q < KV / 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * (lane + 64 * q) + e;
            bool on = c < V;
            if constexpr (AL) { on = on && alw_ok(ar, c < V ? c : 0); if (!on) x[4 * q + e] = -3.0e38f; }
            ok |= (on ? 1u : 0u) << (4 * q + e);
        }
    return ok;
}
// a lane's first maximum among its columns that come strictly after (pv, pi) -- slot j of the selection is the maximum of what comes after slot
// j - 1, so nothing is overwritten and no taken-list is kept; (+inf, -1) in front of slot 0.  None left: (-inf, 0x7fffffff).  A wave arg-max follows
template <int KV>
LXO_DEV void row_next(const float (&x)[KV], unsigned ok, int lane, float pv, int pi, float& best, int& bi) {
    best = -INFINITY; bi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < KV / 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * (lane + 64 * q) + e;
            const float v = x[4 * q + e];
            if (((ok >> (4 * q + e)) & 1u) && alt_before(pv, pi, v, c) && v > best) { best = v; bi = c; }
        }
}
// the wave's number of counting columns in front of (xt, tgt): the target's rank
template <int KV>
LXO_DEV int row_rank(const float (&x)[KV], unsigned ok, int lane, float xt, int tgt) {
    int n = 0;
#pragma unroll
    for (int q = 0; q < KV / 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            n += (((ok >> (4 * q + e)) & 1u) && alt_before(x[4 * q + e], 4 * (lane + 64 * q) + e, xt, tgt)) ? 1 : 0;
    return wave_sum_i(n);
}
// the wave's entropy sum p (lse - x), p = e^(x - lse), over the counting columns: every term >= 0 (lse - sum p x cancels at |x| ~ 100), a lane's
// columns first, then the wave, as row_lse adds; a column that does not count is skipped, never multiplied in
template <bool FAST, int KV>
LXO_DEV float row_entropy(const float (&x)[KV], unsigned ok, float lse) {
    float h = 0.f;
#pragma unroll
    for (int e = 0; e < KV; ++e) if ((ok >> e) & 1u) h += row_exp<FAST>(x[e] - lse) * (lse - x[e]);
    return wave_sum(h);
}
// The same three steps on a strided row: a pass over the row (it sits in L2) each
template <bool AL>
LXO_DEV void strided_next(const float* lg, int lane, int V, const unsigned* ar, float pv, int pi, float& best, int& bi) {
    best = -INFINITY; bi = 0x7fffffff;
    for (int j = lane; j < V; j += 64) {
        const float v = lg[j];
        if ((!AL || alw_ok(ar, j)) && alt_before(pv, pi, v, j) && v > best) { best = v; bi = j; }
    }
}
template <bool AL>
LXO_DEV int strided_rank(const float* lg, int lane, int V, const unsigned* ar, float xt, int tgt) {
    int n = 0;
    for (int j = lane; j < V; j += 64) n += ((!AL || alw_ok(ar, j)) && alt_before(lg[j], j, xt, tgt)) ? 1 : 0;
    return wave_sum_i(n);
}
template <bool AL>
LXO_DEV float strided_entropy(const float* lg, int lane, int V, const unsigned* ar, float lse) {
    float h = 0.f;
    for (int j = lane; j < V; j += 64) if (!AL || alw_ok(ar, j)) { const float v = lg[j]; h += expf(v - lse) * (lse - v); }
    return wave_sum(h);
}

// Sampling (the sample kernels; head_kernels.h states the distribution and the draw).  The uniforms are counter-based as drop.h's mask is: smp_mix is
// splitmix64's step, a sample (image b, draw j) has ONE key and column v of step t the counter t V + v behind it -- nothing depends on n, B or a neighbour.
LXO_DEV unsigned long long smp_mix(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
LXO_DEV unsigned long long smp_key(unsigned seed, int b, int j) {
    return smp_mix(((unsigned long long)seed << 32) | ((unsigned long long)(unsigned)b << 4) | (unsigned long long)(unsigned)j);
}
// g = -log(-log u), u = (bits + 0.5) 2^-23 from 23 hash bits: bits + 0.5 is exact in f32, u < 1 always, g finite (24 bits round u to 1)
LXO_DEV float smp_gumbel(unsigned long long key, int t, int V, int v) {
    const unsigned bits = (unsigned)(smp_mix(key + ((unsigned long long)(unsigned)t * (unsigned)V + (unsigned)v)) >> 41);
    const float u = ((float)bits + 0.5f) * 1.1920928955078125e-7f;
    return -logf(-logf(u));
}
// y = x / tau as the definition states it: the f32 product, ROUNDED -- never contracted into the subtraction or addition that follows, so that every
// step sees the same y (top_k = 1: logq = y - (y + log 1) = 0 exactly)
LXO_DEV float smp_y(float x, float inv_tau) {
#pragma clang fp contract(off)
    return x * inv_tau;
}
// alt_before's order as ONE integer: (x, c) comes before (y, d) <=> alt_key(x, c) > alt_key(y, d) -- high word: the value's bits made monotone (-0 = +0,
// never 0), low word: the column complemented.  A cut-off of the order is then a key T: the columns with alt_key >= T are a prefix of the order,
// CUT_NONE the cut that keeps every column.  alt_val: the value back from a high word
constexpr unsigned long long CUT_NONE = 1ull << 32;
LXO_DEV unsigned alt_key_hi(float x) {
    unsigned u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return u ? u : 1u;
}
LXO_DEV float alt_val(unsigned kh) { return __uint_as_float((kh & 0x80000000u) ? (kh & 0x7fffffffu) : ~kh); }
LXO_DEV unsigned long long alt_key(float x, int c) { return ((unsigned long long)alt_key_hi(x) << 32) | (unsigned long long)(~(unsigned)c); }
LXO_DEV bool key_ge(unsigned kh, int c, unsigned long long T) {
    const unsigned th = (unsigned)(T >> 32), tl = (unsigned)T;
    return kh > th || (kh == th && ~(unsigned)c >= tl);
}
// The cut-offs are found by bisection on the key, most significant bit first: the largest T whose prefix still holds `need` columns (top-k) or
// `need` exp-mass (top-p).  cb = the bits a column < V takes: above them the low word of every key is ones, so those bits are set from the start
// and 32 + cb probes decide the rest -- a trip count fixed by V.  cut_bit(i): the bit probe i decides
LXO_DEV unsigned long long cut_start(int cb) { return 0xFFFFFFFFull & ~((1ull << cb) - 1ull); }
LXO_DEV unsigned long long cut_bit(int i, int cb) { return 1ull << (i < 32 ? 63 - i : cb - 1 - (i - 32)); }
// Register row, what the sample kernel keeps of it: kh = the key's high word of a counting column, 0 (behind every cut) elsewhere, and
// ex = exp(y - max y), y = x / tau, 0 elsewhere; returns max y
template <int KV>
LXO_DEV float row_tempered(const float (&x)[KV], unsigned ok, float inv_tau, unsigned (&kh)[KV], float (&ex)[KV]) {
    float m = -3.0e38f;
#pragma unroll
    for (int i = 0; i < KV; ++i) if ((ok >> i) & 1u) m = fmaxf(m, smp_y(x[i], inv_tau));
    m = wave_max(m);
#pragma unroll
    for (int i = 0; i < KV; ++i) {
        const bool on = (ok >> i) & 1u;
        kh[i] = on ? alt_key_hi(x[i]) : 0u;
        ex[i] = on ? expf(smp_y(x[i], inv_tau) - m) : 0.f;
    }
    return m;
}
// the wave's number of counting columns / their exp-mass at or in front of the cut T (a lane's columns first, then the wave: both monotone in T)
template <int KV>
LXO_DEV int row_count_ge(const unsigned (&kh)[KV], int lane, unsigned long long T) {
    int n = 0;
#pragma unroll
    for (int q = 0; q < KV / 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) n += key_ge(kh[4 * q + e], 4 * (lane + 64 * q) + e, T) ? 1 : 0;
    return wave_sum_i(n);
}
template <int KV>
LXO_DEV float row_mass_ge(const unsigned (&kh)[KV], const float (&ex)[KV], int lane, unsigned long long T) {
    float l = 0.f;
#pragma unroll
    for (int q = 0; q < KV / 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) if (key_ge(kh[4 * q + e], 4 * (lane + 64 * q) + e, T)) l += ex[4 * q + e];
    return wave_sum(l);
}
template <int KV>
LXO_DEV unsigned long long row_cut_count(const unsigned (&kh)[KV], int lane, int cb, int need) {
    unsigned long long T = cut_start(cb);
    for (int i = 0; i < 32 + cb; ++i) { const unsigned long long c = T | cut_bit(i, cb); if (row_count_ge<KV>(kh, lane, c) >= need) T = c; }
    return T;
}
template <int KV>
LXO_DEV unsigned long long row_cut_mass(const unsigned (&kh)[KV], const float (&ex)[KV], int lane, int cb, float need) {
    unsigned long long T = cut_start(cb);
    for (int i = 0; i < 32 + cb; ++i) { const unsigned long long c = T | cut_bit(i, cb); if (row_mass_ge<KV>(kh, ex, lane, c) >= need) T = c; }
    return T;
}
// a lane's first maximum of y + g over its columns inside the cut (strict >, ascending columns): the Gumbel-max draw; a wave arg-max follows
template <int KV>
LXO_DEV void row_gumbel(const unsigned (&kh)[KV], int lane, unsigned long long T, float inv_tau, unsigned long long key, int t, int V, float& best, int& bi) {
    best = -INFINITY; bi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < KV / 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * (lane + 64 * q) + e;
            if (key_ge(kh[4 * q + e], c, T)) {
                const float s = smp_y(alt_val(kh[4 * q + e]), inv_tau) + smp_gumbel(key, t, V, c);
                if (s > best) { best = s; bi = c; }
            }
        }
}
// The same steps on a strided row: a pass over the row each (a probe of a cut-off is one)
template <bool AL>
LXO_DEV float strided_tempered_max(const float* lg, int lane, int V, const unsigned* ar, float inv_tau) {
    float m = -3.0e38f;
    for (int j = lane; j < V; j += 64) if (!AL || alw_ok(ar, j)) m = fmaxf(m, smp_y(lg[j], inv_tau));
    return wave_max(m);
}
template <bool AL>
LXO_DEV int strided_count_ge(const float* lg, int lane, int V, const unsigned* ar, unsigned long long T) {
    int n = 0;
    for (int j = lane; j < V; j += 64) n += ((!AL || alw_ok(ar, j)) && alt_key(lg[j], j) >= T) ? 1 : 0;
    return wave_sum_i(n);
}
template <bool AL>
LXO_DEV float strided_mass_ge(const float* lg, int lane, int V, const unsigned* ar, float inv_tau, float m, unsigned long long T) {
    float l = 0.f;
    for (int j = lane; j < V; j += 64) { const float x = lg[j]; if ((!AL || alw_ok(ar, j)) && alt_key(x, j) >= T) l += expf(smp_y(x, inv_tau) - m); }
    return wave_sum(l);
}
template <bool AL>
LXO_DEV unsigned long long strided_cut_count(const float* lg, int lane, int V, const unsigned* ar, int cb, int need) {
    unsigned long long T = cut_start(cb);
    for (int i = 0; i < 32 + cb; ++i) { const unsigned long long c = T | cut_bit(i, cb); if (strided_count_ge<AL>(lg, lane, V, ar, c) >= need) T = c; }
    return T;
}
template <bool AL>
LXO_DEV unsigned long long strided_cut_mass(const float* lg, int lane, int V, const unsigned* ar, float inv_tau, float m, int cb, float need) {
    unsigned long long T = cut_start(cb);
    for (int i = 0; i < 32 + cb; ++i) { const unsigned long long c = T | cut_bit(i, cb); if (strided_mass_ge<AL>(lg, lane, V, ar, inv_tau, m, c) >= need) T = c; }
    return T;
}
template <bool AL>
LXO_DEV void strided_gumbel(const float* lg, int lane, int V, const unsigned* ar, unsigned long long T, float inv_tau, unsigned long long key, int t,
                            float& best, int& bi) {
    best = -INFINITY; bi = 0x7fffffff;
    for (int j = lane; j < V; j += 64) {
        const float x = lg[j];
        if ((!AL || alw_ok(ar, j)) && alt_key(x, j) >= T) {
            const float s = smp_y(x, inv_tau) + smp_gumbel(key, t, V, j);
            if (s > best) { best = s; bi = j; }
        }
    }
}
// What a sampled row leaves behind: id, logp = the model's own log-prob of it with argmax_kernel's arithmetic (-log of the exp-sum around the
// allowed maximum, plus x[id] - max where the id is not that maximum or is forced), logq = its log-prob under the distribution it was drawn from
// (0 at a forced step); outputs [image][step][draw].  finished (nullable): as argmax_kernel keeps it
struct SmpOut { int* ids_step; int* ids; float* logp; float* logq; int* finished; int* n_unfinished; int max_steps, ostep; };
template <bool AL>
LXO_DEV void smp_emit(const SmpOut& o, const float* lg, int lane, int V, const unsigned* ar, int row, int b, int j, int n, int id, bool forced, float xmax,
                      float lq, int id_end) {
    float lp = 0.f;
    if (o.logp) {
        lp = -logf(strided_expsum<AL>(lg, lane, V, ar, xmax));
        const float xi = lg[id];
        if (forced || xi != xmax) lp += xi - xmax;
    }
    if (lane == 0) {
        const long long at = ((long long)b * o.max_steps + o.ostep) * n + j;
        o.ids[at] = id;
        if (o.logp) o.logp[at] = lp;
        if (o.logq) o.logq[at] = lq;
        if (o.ids_step) o.ids_step[row] = id;
        if (o.finished) {
            const int f = o.finished[row] | (id == id_end && !forced ? 1 : 0);
            o.finished[row] = f;
            if (!f) atomicAdd(o.n_unfinished, 1);
        }
    }
}

// Row of the loss and scoring kernels: row = t * B + b reads formula[b][t] (o = its flat index), live while t < lengths[b]; the target clamped into [0, V)
struct RowTok { int t, b; long long o; bool live; };
LXO_DEV RowTok row_tok(int row, int B, int T, const int* lengths) {
    const int t = row / B, b = row - t * B;
    return {t, b, (long long)b * T + t, t < lengths[b]};
}
LXO_DEV int row_target(const int* formula, long long o, int V) {
    const int tgt = formula[o];
    return tgt < 0 ? 0 : (tgt >= V ? V - 1 : tgt);
}

// The CE kernels' way in: the persistent decoder chain (xdec.hip) flags a barrier that timed out: its logits are then garbage -- make the loss say
// so (NaN) instead of training on them silently.  Returns 1 / the token count (data parallel: the global count arrives by all-reduce in ntok_dev,
// never through the host)
LXO_DEV float ce_begin(const unsigned* chain_err, float* loss_acc, const float* ntok_dev, float inv_ntok) {
    if (chain_err && blockIdx.x == 0 && threadIdx.x == 0 && chain_err[0] != 0u) atomicAdd(&loss_acc[0], __uint_as_float(0x7fc00000u));
    return ntok_dev ? 1.0f / ntok_dev[0] : inv_ntok;
}
// ... and out: the two loss statistics (wave-uniform) are summed per workgroup first -- one atomic pair per workgroup instead of one per token (the
// tokens all hit the same two addresses); f32 parity mode (loss_part): stored, and summed in workgroup order by lxo_k_det_reduce
LXO_DEV void ce_end(float* red, float ce_sum, float n_sum, float* loss_acc, float* loss_part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave] = ce_sum; red[4 + wave] = n_sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float c = red[0] + red[1] + red[2] + red[3], n = red[4] + red[5] + red[6] + red[7];
        if (loss_part) { loss_part[2 * blockIdx.x] = c; loss_part[2 * blockIdx.x + 1] = n; }
        else if (n > 0.f) { atomicAdd(&loss_acc[0], c); atomicAdd(&loss_acc[1], n); }
    }
}

// Weights of the loss (lxo_ce_loss_weighted): the CE kernels end in a parameter pack W that is empty -- the unweighted kernels, argument for argument
// the kernels they were -- or one CeWeights (WT): token (b, t) then weighs tok[b][t] * row[b], ONE f32 product, a NULL factor is 1, any sign
LXO_DEV float ce_weight(const RowTok&) { return 1.f; }
LXO_DEV float ce_weight(const RowTok& r, const CeWeights& q) { return (q.tok ? q.tok[r.o] : 1.f) * (q.row ? q.row[r.b] : 1.f); }
// Label smoothing (lxo_ce_loss_smoothed): the pack may also END in one CeSmooth (SM), alone -- every token weighs 1.f -- or behind the CeWeights.  The
// target of a live row is then q_j = (1 - eps) [j == y] + eps / V over [0, V): ce_target is what column j subtracts from p_j, 1.f and 0.f without it
LXO_DEV float ce_weight(const RowTok&, const CeSmooth&) { return 1.f; }
LXO_DEV float ce_weight(const RowTok& r, const CeWeights& q, const CeSmooth&) { return ce_weight(r, q); }
template <typename... W> struct ce_has_smooth { static constexpr bool value = false; };
template <typename... W> struct ce_has_smooth<CeSmooth, W...> { static constexpr bool value = true; };
template <typename A, typename... W> struct ce_has_smooth<A, W...> { static constexpr bool value = ce_has_smooth<W...>::value; };
LXO_DEV CeSmooth ce_smooth() { return {0.f, 0.f}; }
LXO_DEV CeSmooth ce_smooth(const CeWeights&) { return {0.f, 0.f}; }
LXO_DEV CeSmooth ce_smooth(const CeSmooth& s) { return s; }
LXO_DEV CeSmooth ce_smooth(const CeWeights&, const CeSmooth& s) { return s; }
template <bool SM>
LXO_DEV float ce_target(bool hit, const CeSmooth& s) {
    if constexpr (SM) return hit ? (1.f - s.eps) + s.eps_v : s.eps_v;
    else return hit ? 1.f : 0.f;
}
// a live row's smoothed loss from its plain CE, its log-sum-exp and the sum of its logits over [0, V): (1 - eps) CE + eps U, U = lse - sum / V = -mean_j log p_j
LXO_DEV float ce_smoothed(const CeSmooth& s, float ce, float lse, float xsum, int V) { return (1.f - s.eps) * ce + s.eps * (lse - xsum / (float)V); }
// Soft targets (lxo_ce_loss_soft): behind the CeSmooth the pack may END in one CeSoft (SF).  The row steps it adds:
//   ce_soft_row   lanes 0 .. k - 1 load their slot (a slot that does not count: id -1, mass 0.f) and its logit, the way xt = lg[tgt] is loaded; Sigma and
//                 sum_i m_i (lse - x_i) are added in ascending i from wave-uniform reads of the slot lanes; a row past lengths[b] reads no slot
//   ce_soft_tau   a column's teacher mass before rest / V: the counting slots that name it, in ascending i -- no read-modify-write of the stored row, no
//                 atomics, so slots that share an id are as deterministic as any other
//   ce_soft_grad  S p_j - q_j, q_j = (1 - lambda_r) * ce_target + lambda_r * (tau_j + rest / V)
// A row with lambda_r = 0 (Sigma == 0: no teacher) takes none of the last two: the kernels send it, wave-uniformly, through the smoothed row's own
// statements, so its d(logits) and statistics are lxo_ce_loss_smoothed's bytes whatever the compiler contracts into an fma on either path
LXO_DEV float ce_weight(const RowTok&, const CeSmooth&, const CeSoft&) { return 1.f; }
LXO_DEV float ce_weight(const RowTok& r, const CeWeights& q, const CeSmooth&, const CeSoft&) { return ce_weight(r, q); }
LXO_DEV CeSmooth ce_smooth(const CeSmooth& s, const CeSoft&) { return s; }
LXO_DEV CeSmooth ce_smooth(const CeWeights&, const CeSmooth& s, const CeSoft&) { return s; }
template <typename... W> struct ce_has_soft { static constexpr bool value = false; };
template <> struct ce_has_soft<CeSoft> { static constexpr bool value = true; };
template <typename A, typename... W> struct ce_has_soft<A, W...> { static constexpr bool value = ce_has_soft<W...>::value; };
template <typename... W> LXO_DEV CeSoft ce_soft(const W&...) { return {nullptr, nullptr, 0, 0.f}; }
LXO_DEV CeSoft ce_soft(const CeSmooth&, const CeSoft& f) { return f; }
LXO_DEV CeSoft ce_soft(const CeWeights&, const CeSmooth&, const CeSoft& f) { return f; }
// lane i's value in every lane, i wave-uniform: a v_readlane into a scalar register, no LDS crossbar round trip
#ifdef LXO_HIPSIM
LXO_DEV int wave_bcast(int v, int i) { return __shfl(v, i); }
#else
LXO_DEV int wave_bcast(int v, int i) { return __builtin_amdgcn_readlane(v, i); }
#endif
LXO_DEV float wave_bcast(float v, int i) { return __int_as_float(wave_bcast(__float_as_int(v), i)); }
struct SoftRow {
    int id; float m;                        // lane i < k: slot i
    float lam, keep, S, rest, rest_v, dot;  // wave-uniform: lambda_r, 1 - lambda_r, sum_j q_j, rest, rest / V, sum_i m_i (lse - x_i)
};
LXO_DEV SoftRow ce_soft_row(const CeSoft& f, const RowTok& r, const float* lg, int lane, int V, float lse) {
    SoftRow s;
    s.id = -1; s.m = 0.f;
    float c = 0.f;
    if (r.live && lane < f.k) {
        const long long o = r.o * f.k + lane;
        const int v = f.ids[o];
        if (v >= 0 && v < V) { s.id = v; s.m = f.p[o]; c = s.m * (lse - lg[v]); }
    }
    float sigma = 0.f;
    s.dot = 0.f;
    for (int i = 0; i < f.k; ++i) { sigma += wave_bcast(s.m, i); s.dot += wave_bcast(c, i); }
    s.rest = fmaxf(0.f, 1.f - sigma);
    s.rest_v = s.rest / (float)V;
    s.lam = sigma == 0.f ? 0.f : f.lambda;
    s.keep = 1.f - s.lam;
    s.S = s.keep + s.lam * (sigma + s.rest);
    return s;
}
LXO_DEV float ce_soft_tau(const SoftRow& s, int k, int j) {
    float t = 0.f;
    for (int i = 0; i < k; ++i) {
        const int id_i = wave_bcast(s.id, i);
        const float m_i = wave_bcast(s.m, i);
        t += id_i == j ? m_i : 0.f;
    }
    return t;
}
// ... of the four columns j0 .. j0 + 3 of a register row's quarter q, j0 = 4 (lane + 64 q): a slot's quarter is id >> 8, wave-uniform -- a quarter no slot
// names costs a scalar compare per slot, and a slot costs its compare-select-adds in one quarter only
LXO_DEV void ce_soft_tau4(const SoftRow& s, int k, int q, int j0, float (&t)[4]) {
    t[0] = t[1] = t[2] = t[3] = 0.f;
    for (int i = 0; i < k; ++i) {
        const int id_i = wave_bcast(s.id, i);
        const float m_i = wave_bcast(s.m, i);
        if ((id_i >> 8) != q) continue;
        const int d = id_i - j0;
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] += d == e ? m_i : 0.f;
    }
}
LXO_DEV float ce_soft_grad(const SoftRow& s, float pr, float hard, float tau) { return s.S * pr - (s.keep * hard + s.lam * (tau + s.rest_v)); }
// a live row's soft loss from its smoothed loss: (1 - lambda_r) L_smoothed + lambda_r (sum_i m_i (lse - x_i) + rest U)
LXO_DEV float ce_soft_loss(const SoftRow& s, float l_smoothed, float lse, float xsum, int V) {
    return s.keep * l_smoothed + s.lam * (s.dot + s.rest * (lse - xsum / (float)V));
}
// d(logits) scale of a row: inv_ntok on a live unweighted row, the single f32 product w * inv_norm on a weighted one, 0 past lengths[b]
template <bool WT>
LXO_DEV float ce_scale(const RowTok& r, float w, float inv_ntok) {
    if constexpr (WT) return r.live ? w * inv_ntok : 0.f;
    else return r.live ? inv_ntok : 0.f;
}
// a live row's statistics: {CE, 1}, weighted {w CE, 1, w, CE}
template <bool WT>
LXO_DEV void ce_stats(float& ce_sum, float& n_sum, float& w_sum, float& u_sum, float w, float ce) {
    if constexpr (WT) { ce_sum += w * ce; w_sum += w; u_sum += ce; } else ce_sum += ce;
    n_sum += 1.0f;
}
// ... smoothed {w L, 1, w, CE}: the row's loss l in the first, its PLAIN CE in the last
LXO_DEV void ce_stats_smoothed(float& ce_sum, float& n_sum, float& w_sum, float& u_sum, float w, float l, float ce) {
    ce_sum += w * l; w_sum += w; u_sum += ce;
    n_sum += 1.0f;
}
// ce_end for the four: always through the ordered slots, 4 per workgroup, each added as ce_end adds its two
LXO_DEV void ce_end_w(float* red, float ce_sum, float n_sum, float w_sum, float u_sum, float* loss_part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave] = ce_sum; red[4 + wave] = n_sum; red[8 + wave] = w_sum; red[12 + wave] = u_sum; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const float* q = red + 4 * threadIdx.x;
        loss_part[4 * blockIdx.x + threadIdx.x] = q[0] + q[1] + q[2] + q[3];
    }
}

// Score of the beam candidate (slot, token c) from the token's raw logit x: log_softmax, a finished slot masked (0 at END, f32 lowest elsewhere),
// plus the slot's running log-prob; AL: a banned token scores -inf, also for a finished slot
template <bool AL>
LXO_DEV float cand_score(float x, float lse, int fin, float lp, int c, int id_end, const unsigned* ar) {
    float sl = x - lse;
    const float f = fin ? 1.f : 0.f;
    sl = (1.f - f) * sl + f * (c == id_end ? 0.f : -3.40282347e38f);
    float v = lp + sl;
    if constexpr (AL) { if (!alw_ok(ar, c)) v = -INFINITY; }
    return v;
}
// What slot tid of image b leaves behind at a beam step: its id and parent, v = its running log-prob after the step (state.log_probs), its finished flag
LXO_DEV void beam_emit(int b, int k, int tid, int time, int id, int par, float v, int fin, int* ids_step, int* parents_step, int* ids_out, int* par_out,
                       int max_steps, float* scores_out, float* logp, int* finished, int* n_unfinished) {
    ids_step[b * k + tid] = id;
    parents_step[b * k + tid] = par;
    ids_out[((long long)b * max_steps + time) * k + tid] = id;
    if (par_out) par_out[((long long)b * max_steps + time) * k + tid] = par;
    if (scores_out) scores_out[((long long)b * max_steps + time) * k + tid] = v;
    logp[b * k + tid] = v;
    finished[b * k + tid] = fin;
    if (!fin) atomicAdd(n_unfinished, 1);
}

// ---- loss ----
// loss of img2seq.py:68-75 + gradient; one wave per (t, b) row, rows strided over the grid, three strided passes per row
// W = CeWeights (lxo_ce_loss_weighted): the row's scale is w * inv_norm and the statistics are the four of ce_stats; everything else is the same row
// W ending in CeSmooth (lxo_ce_loss_smoothed): the sum of the logits over [0, V) rides the third pass, on the values it loads anyway -- a lane adds its
// columns in ascending order, then the wave -- and ce_target stands in place of the one-hot
// W ending in CeSoft (lxo_ce_loss_soft): the row takes its own branch below -- the instantiations without one are, statement for statement, what they were
template <typename CT, typename... W>
__global__ __launch_bounds__(256) void ce_loss_kernel(const float* __restrict__ logits, const int* __restrict__ formula,
                                                     const int* __restrict__ lengths, CT* __restrict__ dlogits,
                                                     float* __restrict__ loss_acc, float* __restrict__ loss_part, float inv_ntok, const float* __restrict__ ntok_dev,
                                                     const unsigned* __restrict__ chain_err, int B, int T, int V, int Vp, W... wt) {
    constexpr bool WT = sizeof...(W) != 0;
    constexpr bool SM = ce_has_smooth<W...>::value;
    constexpr bool SF = ce_has_soft<W...>::value;
    __shared__ float red[WT ? 16 : 8];
    inv_ntok = ce_begin(chain_err, loss_acc, ntok_dev, inv_ntok);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const CeSmooth sm = ce_smooth(wt...);
    float ce_sum = 0.f, n_sum = 0.f, w_sum = 0.f, u_sum = 0.f;
    for (int row = blockIdx.x * 4 + wave; row < T * B; row += gridDim.x * 4) {
        const RowTok r = row_tok(row, B, T, lengths);
        const float* lg = logits + (long long)row * Vp;
        CT* dl = dlogits + (long long)row * Vp;
        const int tgt = row_target(formula, r.o, V);
        const float lse = strided_lse<false>(lg, lane, V, nullptr);
        const float w = ce_weight(r, wt...);
        const float scale = ce_scale<WT>(r, w, inv_ntok);
        if constexpr (SF) {
            // the soft row: the smoothed row's steps, the teacher's mass in every column's target.  The column loop is wave-uniform (the slot reads are)
            const CeSoft sf = ce_soft(wt...);
            const SoftRow sr = ce_soft_row(sf, r, lg, lane, V, lse);
            if (sr.lam != 0.f) {                                   // (no teacher: the smoothed row below, statement for statement -- its bytes)
                float xs = 0.f;
                for (int jb = 0; jb < Vp; jb += 64) {
                    const int j = jb + lane;
                    const float tau = ce_soft_tau(sr, sf.k, j);
                    float g = 0.f;
                    if (j < V) {
                        const float xj = lg[j];
                        xs += xj;
                        g = ce_soft_grad(sr, expf(xj - lse), ce_target<true>(j == tgt, sm), tau) * scale;
                    }
                    if (j < Vp) dl[j] = from_f32<CT>(g);
                }
                xs = wave_sum(xs);
                if (r.live) {
                    const float ce = lse - lg[tgt];
                    ce_stats_smoothed(ce_sum, n_sum, w_sum, u_sum, w, ce_soft_loss(sr, ce_smoothed(sm, ce, lse, xs, V), lse, xs, V), ce);
                }
                continue;
            }
        }
        float xs = 0.f;
        for (int j = lane; j < Vp; j += 64) {
            float g = 0.f;
            if (j < V) {
                const float xj = lg[j];
                if constexpr (SM) xs += xj;
                g = (expf(xj - lse) - ce_target<SM>(j == tgt, sm)) * scale;
            }
            dl[j] = from_f32<CT>(g);
        }
        if constexpr (SM) {
            if (r.live) {
                const float ce = lse - lg[tgt];
                ce_stats_smoothed(ce_sum, n_sum, w_sum, u_sum, w, ce_smoothed(sm, ce, lse, wave_sum(xs), V), ce);
            }
        } else if (r.live) ce_stats<WT>(ce_sum, n_sum, w_sum, u_sum, w, lse - lg[tgt]);
    }
    if constexpr (WT) ce_end_w(red, ce_sum, n_sum, w_sum, u_sum, loss_part); else ce_end(red, ce_sum, n_sum, loss_acc, loss_part);
}

// The same with the row held in registers (Vp <= 64 * KV): ONE pass over the logits instead of three passes of 4-byte loads, and every row
// has its own wave from the start (the three-pass kernel: 31 us for 13 MB at the benchmark shape, a chain of dependent passes per row; this one 8).
// Smoothing costs it one more wave reduction per row, over registers it already holds.
template <typename CT, int KV, typename... W>
__global__ __launch_bounds__(256) void ce_loss_rows_kernel(const float* __restrict__ logits, const int* __restrict__ formula,
                                                          const int* __restrict__ lengths, CT* __restrict__ dlogits,
                                                          float* __restrict__ loss_acc, float* __restrict__ loss_part, float inv_ntok, const float* __restrict__ ntok_dev,
                                                          const unsigned* __restrict__ chain_err, int B, int T, int V, int Vp, W... wt) {
    constexpr bool WT = sizeof...(W) != 0;
    constexpr bool SM = ce_has_smooth<W...>::value;
    constexpr bool SF = ce_has_soft<W...>::value;
    constexpr bool BF = is_bf16<CT>::value;
    __shared__ float red[WT ? 16 : 8];
    inv_ntok = ce_begin(chain_err, loss_acc, ntok_dev, inv_ntok);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const CeSmooth sm = ce_smooth(wt...);
    float ce_sum = 0.f, n_sum = 0.f, w_sum = 0.f, u_sum = 0.f;
    for (int row = blockIdx.x * 4 + wave; row < T * B; row += gridDim.x * 4) {
        const RowTok r = row_tok(row, B, T, lengths);
        const float* lg = logits + (long long)row * Vp;
        CT* dl = dlogits + (long long)row * Vp;
        const int tgt = row_target(formula, r.o, V);
        const float xt = lg[tgt];
        float x[KV];
        row_load<KV>(lg, lane, V, Vp, x);
        const float lse = row_lse<BF, KV>(x);
        const float w = ce_weight(r, wt...);
        const float scale = ce_scale<WT>(r, w, inv_ntok);
        if constexpr (SF) {
            // the soft row: the smoothed row's steps, the teacher's mass in every column's target; still one packed store per four columns
            const CeSoft sf = ce_soft(wt...);
            const SoftRow sr = ce_soft_row(sf, r, lg, lane, V, lse);
            if (sr.lam != 0.f) {                                   // (no teacher: the smoothed row below, statement for statement -- its bytes)
#pragma unroll
                for (int q = 0; q < KV / 4; ++q) {
                    const int j0 = 4 * (lane + 64 * q);
                    float tau[4];
                    ce_soft_tau4(sr, sf.k, q, j0, tau);
                    if (j0 >= Vp) continue;
                    float g[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int j = j0 + e;
                        const float pr = row_exp<BF>(x[4 * q + e] - lse);
                        g[e] = j < V ? ce_soft_grad(sr, pr, ce_target<true>(j == tgt, sm), tau[e]) * scale : 0.f;
                    }
                    if constexpr (BF) { const u32x2 pk = {pack_bf2(g[0], g[1]), pack_bf2(g[2], g[3])}; *reinterpret_cast<u32x2*>(dl + j0) = pk; }
                    else { const f32x4 gv = {g[0], g[1], g[2], g[3]}; *reinterpret_cast<f32x4*>(dl + j0) = gv; }
                }
                float xs = 0.f;
#pragma unroll
                for (int q = 0; q < KV / 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) xs += 4 * (lane + 64 * q) + e < V ? x[4 * q + e] : 0.f;
                xs = wave_sum(xs);
                if (r.live) ce_stats_smoothed(ce_sum, n_sum, w_sum, u_sum, w, ce_soft_loss(sr, ce_smoothed(sm, lse - xt, lse, xs, V), lse, xs, V), lse - xt);
                continue;
            }
        }
#pragma unroll
        for (int q = 0; q < KV / 4; ++q) {
            const int j0 = 4 * (lane + 64 * q);
            if (j0 >= Vp) continue;
            float g[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = j0 + e;
                const float pr = row_exp<BF>(x[4 * q + e] - lse);
                g[e] = j < V ? (pr - ce_target<SM>(j == tgt, sm)) * scale : 0.f;
            }
            if constexpr (BF) { const u32x2 pk = {pack_bf2(g[0], g[1]), pack_bf2(g[2], g[3])}; *reinterpret_cast<u32x2*>(dl + j0) = pk; }
            else { const f32x4 gv = {g[0], g[1], g[2], g[3]}; *reinterpret_cast<f32x4*>(dl + j0) = gv; }
        }
        if constexpr (SM) {
            // the sum of the logits over [0, V) only (row_load's fill of the columns behind V is for the max and the exp): KV additions in a lane, six in the wave
            float xs = 0.f;
#pragma unroll
            for (int q = 0; q < KV / 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) xs += 4 * (lane + 64 * q) + e < V ? x[4 * q + e] : 0.f;
            xs = wave_sum(xs);
            if (r.live) ce_stats_smoothed(ce_sum, n_sum, w_sum, u_sum, w, ce_smoothed(sm, lse - xt, lse, xs, V), lse - xt);
        } else if (r.live) ce_stats<WT>(ce_sum, n_sum, w_sum, u_sum, w, lse - xt);
    }
    if constexpr (WT) ce_end_w(red, ce_sum, n_sum, w_sum, u_sum, loss_part); else ce_end(red, ce_sum, n_sum, loss_acc, loss_part);
}

// ---- teacher-forced scoring (lxo_score_tokens) ----
// Forward-only read-out of the training logits: logp_out[b][t] = logits[row][formula[b][t]] - lse(row) and top1_out[b][t] (nullable) =
// the row's first maximum (argmax_kernel's rule: the lower index on ties), row = t * B + b.  No d(logits), no loss statistics, no atomics.
// One wave per row with the row in registers, ce_loss_rows_kernel's row steps: -sum logp over the live tokens is that kernel's sum CE up to
// summation order.  Rows t >= lengths[b]: logp 0, top1 -1.  A failed forward chain (chain_err set): every logp NaN, every top1 -1, as the
// CE kernel turns its loss into NaN.
LXO_DEV void score_dead(bool bad, int lane, long long o, float* logp_out, int* top1_out) {
    if (lane == 0) { logp_out[o] = bad ? __uint_as_float(0x7fc00000u) : 0.f; if (top1_out) top1_out[o] = -1; }
}
template <bool BF, int KV>
__global__ __launch_bounds__(256) void score_rows_kernel(const float* __restrict__ logits, const int* __restrict__ formula,
                                                        const int* __restrict__ lengths, float* __restrict__ logp_out, int* __restrict__ top1_out,
                                                        const unsigned* __restrict__ chain_err, int B, int T, int V, int Vp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool bad = chain_err && chain_err[0] != 0u;
    for (int row = blockIdx.x * 4 + wave; row < T * B; row += gridDim.x * 4) {
        const RowTok r = row_tok(row, B, T, lengths);
        if (bad || !r.live) { score_dead(bad, lane, r.o, logp_out, top1_out); continue; }
        const float* lg = logits + (long long)row * Vp;
        const int tgt = row_target(formula, r.o, V);
        const float xt = lg[tgt];
        float x[KV];
        row_load<KV>(lg, lane, V, Vp, x);
        const float lse = row_lse<BF, KV>(x);
        float best = -3.0e38f; int bi = 0x7fffffff;
        if (top1_out) {
            // a lane's columns in ascending order (strict >: its first maximum), then the wave's (value desc, index asc)
#pragma unroll
            for (int q = 0; q < KV / 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = 4 * (lane + 64 * q) + e;
                    if (j < V && x[4 * q + e] > best) { best = x[4 * q + e]; bi = j; }
                }
            wave_argmax(best, bi);
        }
        if (lane == 0) { logp_out[r.o] = xt - lse; if (top1_out) top1_out[r.o] = bi < V ? bi : 0; }
    }
}

// The same for any Vp (the row does not fit in registers): ce_loss_kernel's strided row steps (expf in both modes), so that its sum CE is
// again -sum logp up to summation order.
__global__ __launch_bounds__(256) void score_kernel(const float* __restrict__ logits, const int* __restrict__ formula,
                                                   const int* __restrict__ lengths, float* __restrict__ logp_out, int* __restrict__ top1_out,
                                                   const unsigned* __restrict__ chain_err, int B, int T, int V, int Vp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool bad = chain_err && chain_err[0] != 0u;
    for (int row = blockIdx.x * 4 + wave; row < T * B; row += gridDim.x * 4) {
        const RowTok r = row_tok(row, B, T, lengths);
        if (bad || !r.live) { score_dead(bad, lane, r.o, logp_out, top1_out); continue; }
        const float* lg = logits + (long long)row * Vp;
        const int tgt = row_target(formula, r.o, V);
        const float lse = strided_lse<false>(lg, lane, V, nullptr);
        float best = -3.0e38f; int bi = 0x7fffffff;
        if (top1_out) {
            strided_argmax<false>(lg, lane, V, nullptr, best, bi);
            wave_argmax(best, bi);
        }
        if (lane == 0) { logp_out[r.o] = lg[tgt] - lse; if (top1_out) top1_out[r.o] = bi < V ? bi : 0; }
    }
}

// seq_out[b] = logp_out[b][0] + ... + logp_out[b][len - 1], one thread per sequence adding in ascending t: the f32 sum in np.float32's
// left-to-right order, whatever the grid of the pass before; a failed forward chain: NaN.  The loads go out 16 at a time ahead of their
// additions (one load after another, T = 101 took 21 us of dependent latency)
__global__ __launch_bounds__(256) void score_seq_kernel(const float* __restrict__ logp, const int* __restrict__ lengths, float* __restrict__ seq_out,
                                                       const unsigned* __restrict__ chain_err, int B, int T) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int n = lengths[b];
    n = n < 0 ? 0 : (n > T ? T : n);
    const float* p = logp + (long long)b * T;
    float s = 0.f;
    for (int t0 = 0; t0 < n; t0 += 16) {
        float v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = t0 + e < n ? p[t0 + e] : 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) if (t0 + e < n) s += v[e];
    }
    seq_out[b] = (chain_err && chain_err[0] != 0u) ? __uint_as_float(0x7fc00000u) : s;
}

// ---- minimum-risk weights (lxo_mrt_weights) ----
// Rows [lo, hi) are the candidates of one image: Q_c = softmax_c(alpha seq_logp_c) around the group's maximum, R = sum_c Q_c cost_c, w_c = alpha Q_c (R - cost_c)
// = d R / d CE_c with CE_c = -seq_logp_c, so the weighted loss kernel's d(logits) is the gradient of the expected cost.  One wave per group, lanes striding
// it in steps of 64; wave_max / wave_sum add in a fixed order and the exponential is expf in both dtype modes: the same bytes in every run and every mode.
// -> R (0 for an empty group); w_out NULL: nothing is written (mrt_risk_kernel adds the groups' R this way).  alpha seq_logp is smp_y's rounded product
LXO_DEV float mrt_group(const float* lp, const float* cost, int lo, int hi, float alpha, int lane, float* w_out, float* q_out) {
    float m = -3.0e38f;
    for (int c = lo + lane; c < hi; c += 64) m = fmaxf(m, smp_y(lp[c], alpha));
    m = wave_max(m);
    float l = 0.f;
    for (int c = lo + lane; c < hi; c += 64) l += expf(smp_y(lp[c], alpha) - m);
    l = wave_sum(l);
    const float inv = 1.0f / l;
    float R = 0.f;
    for (int c = lo + lane; c < hi; c += 64) R += (expf(smp_y(lp[c], alpha) - m) * inv) * cost[c];
    R = wave_sum(R);
    if (w_out)
        for (int c = lo + lane; c < hi; c += 64) {
            const float q = expf(smp_y(lp[c], alpha) - m) * inv;
            w_out[c] = alpha * q * (R - cost[c]);
            if (q_out) q_out[c] = q;
        }
    return R;
}
// what the device holds is read defensively: an offset is clamped into [0, rows] and a group never ends in front of its start
LXO_DEV void mrt_bounds(const int* off, int g, int rows, int& lo, int& hi) {
    lo = min(max(off[g], 0), rows);
    hi = max(min(max(off[g + 1], 0), rows), lo);
}
__global__ __launch_bounds__(256) void mrt_weights_kernel(const float* __restrict__ lp, const float* __restrict__ cost, const int* __restrict__ off, int G,
                                                         int rows, float alpha, float* __restrict__ w_out, float* __restrict__ q_out) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g < G) {
        int lo, hi;
        mrt_bounds(off, g, rows, lo, hi);
        mrt_group(lp, cost, lo, hi, alpha, lane, w_out, q_out);
    }
    // the rows behind the last group (the chain batch's dead rows; G == 0: every row) weigh nothing
    for (int i = min(max(off[G], 0), rows) + blockIdx.x * 256 + threadIdx.x; i < rows; i += gridDim.x * 256) { w_out[i] = 0.f; if (q_out) q_out[i] = 0.f; }
}
// risk_out[0] = R_0 + R_1 + ... in ascending g, added by one thread: ONE workgroup, its four waves take four groups at a time
__global__ __launch_bounds__(256) void mrt_risk_kernel(const float* __restrict__ lp, const float* __restrict__ cost, const int* __restrict__ off, int G,
                                                      int rows, float alpha, float* __restrict__ risk_out) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float risk = 0.f;
    for (int g0 = 0; g0 < G; g0 += 4) {
        float R = 0.f;
        if (g0 + wave < G) {
            int lo, hi;
            mrt_bounds(off, g0 + wave, rows, lo, hi);
            R = mrt_group(lp, cost, lo, hi, alpha, lane, nullptr, nullptr);
        }
        if (lane == 0) red[wave] = R;
        __syncthreads();
        if (threadIdx.x == 0) for (int e = 0; e < 4 && g0 + e < G; ++e) risk += red[e];
        __syncthreads();
    }
    if (threadIdx.x == 0) risk_out[0] = risk;
}

// ---- alternatives per position (lxo_score_alternatives) ----
// Read-out of the same logits: ids_out / logp_out [B][T][k] = the k first columns of row t * B + b in alt_before's order and their log-probs
// x[id] - lse, rank_out [B][T] (nullable) = how many columns come before the target (0: it is the top-1), ent_out [B][T] (nullable) = the
// entropy of the step.  Slot 0 is score_rows_kernel's arg-max and a slot that holds the target carries its logp_out, bit for bit (same lse
// helper, same operands).  AL: everything runs over row b's allowed columns; a banned target has rank -1, slots beyond the allowed columns
// are -1 / -inf.  Rows t >= lengths[b]: -1 / 0 / -1 / 0.  A failed forward chain: -1 / NaN / -1 / NaN.
LXO_DEV void alt_dead(bool bad, int lane, int k, long long o, int* ids_out, float* logp_out, int* rank_out, float* ent_out) {
    const float z = bad ? __uint_as_float(0x7fc00000u) : 0.f;
    if (lane < k) { ids_out[o * k + lane] = -1; logp_out[o * k + lane] = z; }
    if (lane == 0) { if (rank_out) rank_out[o] = -1; if (ent_out) ent_out[o] = z; }
}
// lane j holds slot j: (sv, si) = its logit and column, 0x7fffffff where the row had no column left
LXO_DEV void alt_emit(int lane, int k, long long o, float sv, int si, float lse, int* ids_out, float* logp_out) {
    if (lane < k) {
        const bool none = si == 0x7fffffff;
        ids_out[o * k + lane] = none ? -1 : si;
        logp_out[o * k + lane] = none ? -INFINITY : sv - lse;
    }
}
template <bool BF, int KV, bool AL>
__global__ __launch_bounds__(256) void score_alt_rows_kernel(const float* __restrict__ logits, const int* __restrict__ formula,
                                                            const int* __restrict__ lengths, int k, DecAllow al, int* __restrict__ ids_out,
                                                            float* __restrict__ logp_out, int* __restrict__ rank_out, float* __restrict__ ent_out,
                                                            const unsigned* __restrict__ chain_err, int B, int T, int V, int Vp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool bad = chain_err && chain_err[0] != 0u;
    for (int row = blockIdx.x * 4 + wave; row < T * B; row += gridDim.x * 4) {
        const RowTok r = row_tok(row, B, T, lengths);
        if (bad || !r.live) { alt_dead(bad, lane, k, r.o, ids_out, logp_out, rank_out, ent_out); continue; }
        const float* lg = logits + (long long)row * Vp;
        const unsigned* ar = nullptr;
        if constexpr (AL) ar = alw_row(al, r.b);
        const int tgt = row_target(formula, r.o, V);
        const float xt = lg[tgt];
        float x[KV];
        row_load<KV>(lg, lane, V, Vp, x);
        const unsigned ok = row_counts<KV, AL>(lane, V, ar, x);
        const float lse = row_lse<BF, KV>(x);
        float pv = INFINITY, sv = 0.f; int pi = -1, si = 0x7fffffff;
        for (int j = 0; j < k; ++j) {
            float best; int bi;
            row_next<KV>(x, ok, lane, pv, pi, best, bi);
            wave_argmax(best, bi);
            if (lane == j) { sv = best; si = bi; }
            pv = best; pi = bi;
        }
        alt_emit(lane, k, r.o, sv, si, lse, ids_out, logp_out);
        if (rank_out) {
            const int n = row_rank<KV>(x, ok, lane, xt, tgt);
            if (lane == 0) rank_out[r.o] = (AL && !alw_ok(ar, tgt)) ? -1 : n;
        }
        if (ent_out) {
            const float h = row_entropy<BF, KV>(x, ok, lse);
            if (lane == 0) ent_out[r.o] = h;
        }
    }
}
// The same for any Vp: the strided row steps, k + 4 passes over a row
template <bool AL>
__global__ __launch_bounds__(256) void score_alt_kernel(const float* __restrict__ logits, const int* __restrict__ formula,
                                                       const int* __restrict__ lengths, int k, DecAllow al, int* __restrict__ ids_out,
                                                       float* __restrict__ logp_out, int* __restrict__ rank_out, float* __restrict__ ent_out,
                                                       const unsigned* __restrict__ chain_err, int B, int T, int V, int Vp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool bad = chain_err && chain_err[0] != 0u;
    for (int row = blockIdx.x * 4 + wave; row < T * B; row += gridDim.x * 4) {
        const RowTok r = row_tok(row, B, T, lengths);
        if (bad || !r.live) { alt_dead(bad, lane, k, r.o, ids_out, logp_out, rank_out, ent_out); continue; }
        const float* lg = logits + (long long)row * Vp;
        const unsigned* ar = nullptr;
        if constexpr (AL) ar = alw_row(al, r.b);
        const int tgt = row_target(formula, r.o, V);
        const float lse = strided_lse<AL>(lg, lane, V, ar);
        float pv = INFINITY, sv = 0.f; int pi = -1, si = 0x7fffffff;
        for (int j = 0; j < k; ++j) {
            float best; int bi;
            strided_next<AL>(lg, lane, V, ar, pv, pi, best, bi);
            wave_argmax(best, bi);
            if (lane == j) { sv = best; si = bi; }
            pv = best; pi = bi;
        }
        alt_emit(lane, k, r.o, sv, si, lse, ids_out, logp_out);
        if (rank_out) {
            const int n = strided_rank<AL>(lg, lane, V, ar, lg[tgt], tgt);
            if (lane == 0) rank_out[r.o] = (AL && !alw_ok(ar, tgt)) ? -1 : n;
        }
        if (ent_out) {
            const float h = strided_entropy<AL>(lg, lane, V, ar, lse);
            if (lane == 0) ent_out[r.o] = h;
        }
    }
}

// ---- decode ----
// greedy_decoder_cell.py:58-64: id = argmax (first max), finished |= id == END; one wave per row.
// logp_out (nullable) [n][max_steps]: log_softmax(logits)[id] = logits[id] - lse, the log-sum-exp from one more pass over the row the wave has read
// PF: at a step inside its prefix a row emits the forced id f (logp: logits[f] - lse) and stays unfinished
// AL: banned columns are skipped in the max pass and in the exp-sum pass (a forced id's log-prob is taken under the same renormalised distribution)
template <bool PF, bool AL>
__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ logits, int Vp, int V, int n, int id_end,
                                                    int* __restrict__ ids_step, int* __restrict__ ids_out, int max_steps, int step,
                                                    int* __restrict__ finished, int* __restrict__ n_unfinished, float* __restrict__ logp_out,
                                                    DecPrefix pf, DecAllow al) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* lg = logits + (long long)row * Vp;
    const unsigned* ar = nullptr;
    if constexpr (AL) ar = alw_row(al, row);
    float best; int bi;
    strided_argmax<AL>(lg, lane, V, ar, best, bi);
    shfl_argmax(best, bi);
    int fi = -1;                                               // PF: the forced id of this step (-1: a free step)
    if constexpr (PF) { if (step < pfx_len(pf, row)) fi = pfx_id(pf, row, step, V); }
    float lp = 0.f;
    if (logp_out) {
        lp = -logf(strided_expsum<AL>(lg, lane, V, ar, best));      // logits[id] - (best + log l), logits[id] = best
        if constexpr (PF) { if (fi >= 0) lp += lg[fi] - best; }
    }
    if (lane == 0) {
        if (bi >= V) bi = 0;
        if constexpr (PF) { if (fi >= 0) bi = fi; }
        if (logp_out) logp_out[(long long)row * max_steps + step] = lp;
        ids_step[row] = bi;
        ids_out[(long long)row * max_steps + step] = bi;
        const int f = finished[row] | (bi == id_end && fi < 0 ? 1 : 0);
        finished[row] = f;
        if (!f) atomicAdd(n_unfinished, 1);
    }
}

// Sampled select step (head_kernels.h: the distribution and the draw): row r is draw r % n of image r / n, one wave per row as argmax_kernel; the row
// in registers (Vp <= 64 * KV).  PF / AL: one prefix and one allowed set per IMAGE.  The cut-off searches run only where top_k / top_p ask for them
// (wave-uniform branches, fixed trip counts); an empty allowed row emits 0.
template <int KV, bool PF, bool AL>
__global__ __launch_bounds__(256) void sample_rows_kernel(const float* __restrict__ logits, int Vp, int V, int rows, int id_end, int time, DecSample so,
                                                         SmpOut o, DecPrefix pf, DecAllow al) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = row / so.n, j = row - b * so.n;
    const float* lg = logits + (long long)row * Vp;
    const unsigned* ar = nullptr;
    if constexpr (AL) ar = alw_row(al, b, row);
    int fi = -1;
    if constexpr (PF) { if (time < pfx_len(pf, b)) fi = pfx_id(pf, b, time, V); }
    float x[KV];
    row_load<KV>(lg, lane, V, Vp, x);
    const unsigned ok = row_counts<KV, AL>(lane, V, ar, x);
    float xmax = x[0];
#pragma unroll
    for (int e = 1; e < KV; ++e) xmax = fmaxf(xmax, x[e]);
    xmax = wave_max(xmax);
    int id = fi; float lq = 0.f;
    if (fi < 0) {
        unsigned kh[KV]; float ex[KV];
        const float m = row_tempered<KV>(x, ok, so.inv_tau, kh, ex);
        unsigned long long T = CUT_NONE;
        if (so.top_k > 0) T = row_cut_count<KV>(kh, lane, so.cb, min(so.top_k, wave_sum_i(__builtin_popcount(ok))));
        if (so.top_p < 1.f) T = row_cut_mass<KV>(kh, ex, lane, so.cb, so.top_p * row_mass_ge<KV>(kh, ex, lane, T));
        float best; int bi;
        row_gumbel<KV>(kh, lane, T, so.inv_tau, smp_key(so.seed, b, j), time, V, best, bi);
        wave_argmax(best, bi);
        id = bi < V ? bi : 0;
        lq = smp_y(lg[id], so.inv_tau) - (m + logf(row_mass_ge<KV>(kh, ex, lane, T)));
    }
    smp_emit<AL>(o, lg, lane, V, ar, row, b, j, so.n, id, fi >= 0, xmax, lq, id_end);
}
// The same for any Vp: the strided row steps
template <bool PF, bool AL>
__global__ __launch_bounds__(256) void sample_kernel(const float* __restrict__ logits, int Vp, int V, int rows, int id_end, int time, DecSample so,
                                                    SmpOut o, DecPrefix pf, DecAllow al) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = row / so.n, j = row - b * so.n;
    const float* lg = logits + (long long)row * Vp;
    const unsigned* ar = nullptr;
    if constexpr (AL) ar = alw_row(al, b, row);
    int fi = -1;
    if constexpr (PF) { if (time < pfx_len(pf, b)) fi = pfx_id(pf, b, time, V); }
    float xmax; int xi;
    strided_argmax<AL>(lg, lane, V, ar, xmax, xi);
    xmax = wave_max(xmax);
    int id = fi; float lq = 0.f;
    if (fi < 0) {
        const float m = strided_tempered_max<AL>(lg, lane, V, ar, so.inv_tau);
        unsigned long long T = CUT_NONE;
        if (so.top_k > 0) T = strided_cut_count<AL>(lg, lane, V, ar, so.cb, min(so.top_k, strided_count_ge<AL>(lg, lane, V, ar, CUT_NONE)));
        if (so.top_p < 1.f) T = strided_cut_mass<AL>(lg, lane, V, ar, so.inv_tau, m, so.cb, so.top_p * strided_mass_ge<AL>(lg, lane, V, ar, so.inv_tau, m, T));
        float best; int bi;
        strided_gumbel<AL>(lg, lane, V, ar, T, so.inv_tau, smp_key(so.seed, b, j), time, best, bi);
        wave_argmax(best, bi);
        id = bi < V ? bi : 0;
        lq = smp_y(lg[id], so.inv_tau) - (m + logf(strided_mass_ge<AL>(lg, lane, V, ar, so.inv_tau, m, T)));
    }
    smp_emit<AL>(o, lg, lane, V, ar, row, b, j, so.n, id, fi >= 0, xmax, lq, id_end);
}

// One block per image: beam_search_decoder_cell.py:146-187.
//  log_softmax, mask finished beams (0 at END, f32 lowest elsewhere), add running log-probs,
//  top-k over k*V (beam 0 only at time 0), ids = idx % V, parents = idx / V, gather finished.
// add_div_penalty (beam_search_decoder_cell.py:258-287, Li et al. 2016): score += log(div_gamma) * rank * bernoulli(div_prob),
// rank = position of the entry in the descending sort of its hypothesis' V scores (ties: lower id first, as
// tf.nn.top_k orders them).  Bernoulli draws: the counter hash of drop_scale on (time, image, beam, id).
struct DivPen { float log_gamma; unsigned thr; unsigned seed; float* scratch; };   // log_gamma == 0 or thr == 0: off
// PF (both beam kernels): at a step t < P inside image b's prefix every slot j takes the forced id with parent j, its running log-prob grows by
// that id's log-prob, its finished flag stays, no diversity penalty -- the k slots stay identical, as in the initial state.  Step P selects
// over slot 0 alone (what time 0 does without a prefix), later steps over all k V candidates.
// AL (both beam kernels): the log-sum-exp runs over image b's allowed columns; a banned candidate (slot, token) scores -inf, also for a finished
// hypothesis, and is never selected while an allowed one is left; the diversity rank of an allowed column counts the allowed columns ahead of it.
// Under a grammar (DecAllow::per_row) every hypothesis slot j has its own set, ar + j * as; else as == 0 and the slots share the image's.
template <bool PF, bool AL>
__global__ __launch_bounds__(256) void beam_step_kernel(float* __restrict__ logits, int Vp, int V, int k, int id_end, int time, DivPen dp,
                                                       float* __restrict__ logp, int* __restrict__ finished,
                                                       int* __restrict__ ids_step, int* __restrict__ parents_step,
                                                       int* __restrict__ ids_out, int* __restrict__ par_out, int max_steps,
                                                       int* __restrict__ n_unfinished, float* __restrict__ scores_out, DecPrefix pf, DecAllow al) {
    __shared__ float lse[16];
    __shared__ float cand_v[16 * 4]; __shared__ int cand_i[16 * 4];
    __shared__ float sel_v[16]; __shared__ int sel_i[16];
    __shared__ int fin_old[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned* ar = nullptr; long long as = 0;          // AL: the set of slot j is ar + j * as
    if constexpr (AL) { ar = alw_row(al, b, b * k); as = alw_slot_stride(al); }
    // log-sum-exp per beam (one wave per beam, round-robin)
    for (int j = wave; j < k; j += 4) {
        const float s = strided_lse<AL>(logits + ((long long)b * k + j) * Vp, lane, V, ar + j * as);
        if (lane == 0) lse[j] = s;
    }
    if (tid < k) fin_old[tid] = finished[b * k + tid];
    __syncthreads();
    int t0 = 0;                                                // PF: the image's prefix length -- its beam search starts there
    if constexpr (PF) {
        t0 = pfx_len(pf, b);
        if (time < t0) {
            if (tid < k) {
                const int id = pfx_id(pf, b, time, V);
                beam_emit(b, k, tid, time, id, tid, logp[b * k + tid] + (logits[((long long)b * k + tid) * Vp + id] - lse[tid]), fin_old[tid],
                          ids_step, parents_step, ids_out, par_out, max_steps, scores_out, logp, finished, n_unfinished);
            }
            return;
        }
    }
    const int nb = time > t0 ? k : 1;
    const int total = nb * V;
    const bool div = dp.log_gamma != 0.f && dp.thr != 0u;
    float* pen = dp.scratch + (long long)b * k * Vp;
    if (div) {
        float* row0 = logits + (long long)b * k * Vp;
        for (int i = tid; i < k * V; i += 256) {            // scores of every hypothesis, in place of its logits
            const int j = i / V, c = i - j * V;
            row0[j * Vp + c] = cand_score<AL>(row0[j * Vp + c], lse[j], fin_old[j], logp[b * k + j], c, id_end, ar + j * as);
        }
        __syncthreads();
        for (int i = tid; i < k * V; i += 256) {
            const int j = i / V, c = i - j * V;
            const float* row = row0 + j * Vp;
            const float v = row[c];
            int rank = 0;
            for (int q = 0; q < V; ++q) { const float w = row[q]; rank += (w > v || (w == v && q < c)) ? 1 : 0; }
            const Drop dd = {dp.thr, 1.f, dp.seed, time, b * k + j, (int)gridDim.x * k};
            pen[j * Vp + c] = v + dp.log_gamma * (float)rank * drop_scale(dd, 3u, 0, c, V);
            if constexpr (AL) { if (!alw_ok(ar + j * as, c)) pen[j * Vp + c] = -INFINITY; }
        }
        __syncthreads();
    }
    for (int sel = 0; sel < k; ++sel) {
        float best = -INFINITY; int bi = 0x7fffffff;
        for (int i = tid; i < total; i += 256) {
            const int j = i / V, c = i - j * V;
            bool taken = false;
            for (int q = 0; q < sel; ++q) taken |= (sel_i[q] == i);
            if (taken) continue;
            const float val = div ? pen[j * Vp + c]
                                  : cand_score<AL>(logits[((long long)b * k + j) * Vp + c], lse[j], fin_old[j], logp[b * k + j], c, id_end, ar + j * as);
            if (val > best || (val == best && i < bi)) { best = val; bi = i; }
        }
        shfl_argmax(best, bi);
        if (lane == 0) { cand_v[wave] = best; cand_i[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            float bv = cand_v[0]; int bx = cand_i[0];
            for (int w = 1; w < 4; ++w)
                if (cand_v[w] > bv || (cand_v[w] == bv && cand_i[w] < bx)) { bv = cand_v[w]; bx = cand_i[w]; }
            sel_v[sel] = bv; sel_i[sel] = bx;
        }
        __syncthreads();
    }
    if (tid < k) {
        const int idx = sel_i[tid];
        const int id = idx % V, par = idx / V;
        beam_emit(b, k, tid, time, id, par, sel_v[tid], fin_old[par] | (id == id_end ? 1 : 0),
                  ids_step, parents_step, ids_out, par_out, max_steps, scores_out, logp, finished, n_unfinished);
    }
}

// The same step with every candidate score held in REGISTERS (k * V <= BS_TH * BS_NPT = 4096, k <= 64 / BS_NW, no diversity penalty): beam_step_kernel re-reads and
// re-forms all k * V scores (an integer division each) for every one of its k selections and makes two passes over a row for its
// log-sum-exp -- 31 us of a 161 us beam-5 step at B = 64, on 64 workgroups.  Here a lane loads its share of a row ONCE (max, then the
// exponentials, from registers), a thread forms its <= BS_NPT scores ONCE, and a selection is a register scan + the block-wide arg-max.
// Same row steps, same summation order inside a wave, same tie rule (lower flat index first): the ids and parents are the slow kernel's.
constexpr int BS_TH = 512, BS_NW = BS_TH / 64, BS_NPT = 4096 / BS_TH;      // 8 waves x 8 candidates per thread (it was 4 x 16: a selection round scans a thread's candidates, k rounds per step)
template <bool PF, bool AL>
__global__ __launch_bounds__(BS_TH) void beam_step_fast_kernel(const float* __restrict__ logits, int Vp, int V, int k, int id_end, int time,
                                                            float* __restrict__ logp, int* __restrict__ finished,
                                                            int* __restrict__ ids_step, int* __restrict__ parents_step,
                                                            int* __restrict__ ids_out, int* __restrict__ par_out, int max_steps,
                                                            int* __restrict__ n_unfinished, float* __restrict__ scores_out, DecPrefix pf, DecAllow al) {
    __shared__ float lse[16];
    __shared__ float sel_v[16]; __shared__ int sel_i[16];
    __shared__ int fin_old[16];
    __shared__ float lp_old[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ float wc_v[BS_NW * 16]; __shared__ int wc_i[BS_NW * 16];      // the waves' k best each
    int t0 = 0;                                                // PF: the image's prefix length (beam_step_kernel)
    if constexpr (PF) t0 = pfx_len(pf, b);
    const unsigned* ar = nullptr; long long as = 0;           // AL: the allowed-token bits of slot j are ar + j * as
    if constexpr (AL) { ar = alw_row(al, b, b * k); as = alw_slot_stride(al); }
    const int nb = time > t0 ? k : 1;
    const int total = nb * V;
    float raw[BS_NPT];                                         // raw logits of this thread's candidates (unconditional, clamped: requested before anything is waited for)
    {
        int jq = tid / V, cq = tid - jq * V;
#pragma unroll
        for (int u = 0; u < BS_NPT; ++u) {
            const int j = min(jq, k - 1), c = cq;
            cq += BS_TH;
            while (cq >= V) { cq -= V; ++jq; }
            raw[u] = logits[((long long)b * k + j) * Vp + c];
        }
    }
    // log-sum-exp per hypothesis
    if (V <= 64 * 8 && k <= BS_NW) {
        // a wave takes hypothesis `wave` (a spare wave repeats the last one), the row in registers for its two passes
        const float s = lane_row_lse<8, AL>(logits + ((long long)b * k + min(wave, k - 1)) * Vp, lane, V, ar + min(wave, k - 1) * as);
        if (lane == 0 && wave < k) lse[wave] = s;
    } else
    for (int j = wave; j < k; j += BS_NW) {                   // the general form: one wave per hypothesis, round-robin
        const float* lg = logits + ((long long)b * k + j) * Vp;
        const float s = V <= 64 * 16 ? lane_row_lse<16, AL>(lg, lane, V, ar + j * as) : strided_lse<AL>(lg, lane, V, ar + j * as);
        if (lane == 0) lse[j] = s;
    }
    if (tid < k) { fin_old[tid] = finished[b * k + tid]; lp_old[tid] = logp[b * k + tid]; }
    __syncthreads();
    if constexpr (PF) {
        if (time < t0) {
            if (tid < k) {
                const int id = pfx_id(pf, b, time, V);
                beam_emit(b, k, tid, time, id, tid, lp_old[tid] + (logits[((long long)b * k + tid) * Vp + id] - lse[tid]), fin_old[tid],
                          ids_step, parents_step, ids_out, par_out, max_steps, scores_out, logp, finished, n_unfinished);
            }
            return;
        }
    }
    // candidates of this thread: i = tid + BS_TH u -> (hypothesis, id) walked instead of divided; their raw logits were requested in front of the
    // log-sum-exp pass (raw[]: the second read of the rows no longer waits behind the first)
    float val[BS_NPT];
    {
        int jq = tid / V, cq = tid - jq * V;
#pragma unroll
        for (int u = 0; u < BS_NPT; ++u) {
            const int i = tid + BS_TH * u;
            val[u] = -INFINITY;
            const int j = jq, c = cq;
            cq += BS_TH;
            while (cq >= V) { cq -= V; ++jq; }
            if (i < total) val[u] = cand_score<AL>(raw[u], lse[j], fin_old[j], lp_old[j], c, id_end, ar + j * as);
        }
    }
    // top-k in two stages, ONE workgroup barrier between them (it was two per selection): every wave selects the k best of ITS candidates by itself
    // -- the k best of the block are among them -- then wave 0 selects the k best of the BS_NW k survivors, one per lane.  Order everywhere:
    // value descending, flat index ascending (tf.nn.top_k over the flattened [k * V] scores: the lower index of equal values first).
    {
        unsigned taken = 0u;                                   // bit u: this thread's candidate u has been selected
        for (int sel = 0; sel < k; ++sel) {
            float best = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
            for (int u = 0; u < BS_NPT; ++u) {
                const int i = tid + BS_TH * u;
                if (i < total && !((taken >> u) & 1u) && (val[u] > best || (val[u] == best && i < bi))) { best = val[u]; bi = i; }
            }
            wave_argmax(best, bi);
            if (lane == 0) { wc_v[wave * 16 + sel] = best; wc_i[wave * 16 + sel] = bi; }
#pragma unroll
            for (int u = 0; u < BS_NPT; ++u) if (tid + BS_TH * u == bi) taken |= 1u << u;
        }
    }
    __syncthreads();
    if (wave == 0) {
        const int w = lane / k, e = lane - w * k;              // survivor e of wave w (BS_NW k <= 64 lanes: the launcher's condition)
        float cv = -INFINITY; int ci = 0x7fffffff;
        if (w < BS_NW) { cv = wc_v[w * 16 + e]; ci = wc_i[w * 16 + e]; }
        for (int sel = 0; sel < k; ++sel) {
            float bv = cv; int bx = ci;
            wave_argmax(bv, bx);
            if (lane == 0) { sel_v[sel] = bv; sel_i[sel] = bx; }
            if (ci == bx) { cv = -INFINITY; ci = 0x7fffffff; }
        }
    }
    __syncthreads();
    if (tid < k) {
        const int idx = sel_i[tid];
        const int id = idx % V, par = idx / V;
        beam_emit(b, k, tid, time, id, par, sel_v[tid], fin_old[par] | (id == id_end ? 1 : 0),
                  ids_step, parents_step, ids_out, par_out, max_steps, scores_out, logp, finished, n_unfinished);
    }
}

}  // namespace

#define LAUNCH(kern, grid, ...) hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, __VA_ARGS__)
#define DONE return (int)hipGetLastError()
// the register-row kernels' KV from the padded vocabulary: ROWS(KV) with 64 * KV >= Vp
#define BY_KV(Vp, ROWS) do { if ((Vp) <= 256) ROWS(4); else if ((Vp) <= 512) ROWS(8); else ROWS(16); } while (0)

int lxo_k_ce_loss(int dt, const float* logits, const int* formula, const int* lengths, void* dlogits, float* loss_acc, float inv_ntok,
                  const float* ntok_dev, const unsigned* chain_err, int B, int T, int V, int Vp, DetScratch det, hipStream_t st, const CeWeights* weights,
                  const CeSmooth* smooth, const CeSoft* soft) {
    int g = cdiv(T * B, 4);
    float* part = (det.p && det.floats >= 1024) ? det.p : nullptr;      // loss_acc is zero on entry (lxo_impl_ce_loss)
    const bool four = weights || smooth;
    const int nst = four ? 4 : 2;                                       // statistics per workgroup slot
    if (four && !(det.p && det.floats >= 2048)) return -2;              // the four weighted / smoothed statistics go through the ordered slots only
    const CeWeights wt = weights ? *weights : CeWeights{};
    const CeSmooth sm = smooth ? *smooth : CeSmooth{};
    if (soft && (!smooth || soft->k < 1 || soft->k > 16)) return -2;    // soft targets ride behind a CeSmooth (eps may be 0), their k is lxo_k_score_alt's
    const CeSoft sf = soft ? *soft : CeSoft{};
#define CE_ARGS(CT_) logits, formula, lengths, (CT_*)dlogits, loss_acc, part, inv_ntok, ntok_dev, chain_err, B, T, V, Vp
    // CE_WT(CT, KERNEL<...): KERNEL<...> or, with weights, KERNEL<..., CeWeights>; with smoothing KERNEL<..., CeSmooth> and KERNEL<..., CeWeights, CeSmooth>;
    // with soft targets a CeSoft behind either of the last two
#define CE_WT(CT_, ...) do { \
        if (weights && soft) LAUNCH((__VA_ARGS__, CeWeights, CeSmooth, CeSoft>), g, CE_ARGS(CT_), wt, sm, sf); \
        else if (soft) LAUNCH((__VA_ARGS__, CeSmooth, CeSoft>), g, CE_ARGS(CT_), sm, sf); \
        else if (weights && smooth) LAUNCH((__VA_ARGS__, CeWeights, CeSmooth>), g, CE_ARGS(CT_), wt, sm); \
        else if (smooth) LAUNCH((__VA_ARGS__, CeSmooth>), g, CE_ARGS(CT_), sm); \
        else if (weights) LAUNCH((__VA_ARGS__, CeWeights>), g, CE_ARGS(CT_), wt); \
        else LAUNCH((__VA_ARGS__>), g, CE_ARGS(CT_)); } while (0)
    if (Vp % 4 == 0 && Vp <= 1024 && (((uintptr_t)logits | (uintptr_t)dlogits) & 15) == 0) {
        // a wave per row, the row in registers (one pass); the f32 parity mode keeps at most 512 workgroups (its ordered partial sums)
        if (g > (part ? 512 : 2048)) g = part ? 512 : 2048;
#define CE_ROWS(KV_) do { if (dt == LXO_BF16) CE_WT(bf16_t, ce_loss_rows_kernel<bf16_t, KV_); else CE_WT(float, ce_loss_rows_kernel<float, KV_); } while (0)
        BY_KV(Vp, CE_ROWS);
#undef CE_ROWS
    } else {
        if (g > 512) g = 512;
        if (dt == LXO_BF16) CE_WT(bf16_t, ce_loss_kernel<bf16_t);
        else CE_WT(float, ce_loss_kernel<float);
    }
#undef CE_WT
#undef CE_ARGS
    if (part) return lxo_k_det_reduce(part, g, nst, nst, loss_acc, st);
    DONE;
}
int lxo_k_mrt_weights(const float* seq_logp, const float* cost, const int* group_off, int G, int rows, float alpha, float* w_out, float* q_out,
                      float* risk_out, hipStream_t st) {
    LAUNCH(mrt_weights_kernel, G > 4 ? cdiv(G, 4) : 1, seq_logp, cost, group_off, G, rows, alpha, w_out, q_out);
    if (risk_out) LAUNCH(mrt_risk_kernel, 1, seq_logp, cost, group_off, G, rows, alpha, risk_out);
    DONE;
}
int lxo_k_score(int dt, const float* logits, const int* formula, const int* lengths, float* logp_out, int* top1_out, float* seq_out,
                const unsigned* chain_err, int B, int T, int V, int Vp, hipStream_t st) {
    int g = cdiv(T * B, 4);
#define SC_ARGS logits, formula, lengths, logp_out, top1_out, chain_err, B, T, V, Vp
    if (Vp % 4 == 0 && Vp <= 1024 && ((uintptr_t)logits & 15) == 0) {
        if (g > 2048) g = 2048;
#define SC_ROWS(KV_) do { if (dt == LXO_BF16) LAUNCH((score_rows_kernel<true, KV_>), g, SC_ARGS); else LAUNCH((score_rows_kernel<false, KV_>), g, SC_ARGS); } while (0)
        BY_KV(Vp, SC_ROWS);
#undef SC_ROWS
    } else {
        LAUNCH(score_kernel, g > 512 ? 512 : g, SC_ARGS);
    }
#undef SC_ARGS
    if (seq_out) LAUNCH(score_seq_kernel, cdiv(B, 256), logp_out, lengths, seq_out, chain_err, B, T);
    DONE;
}
int lxo_k_score_alt(int dt, const float* logits, const int* formula, const int* lengths, int k, const DecAllow* allow, int* ids_out, float* logp_out,
                    int* rank_out, float* ent_out, const unsigned* chain_err, int B, int T, int V, int Vp, hipStream_t st) {
    if (k < 1 || k > 16 || k > V) return -2;
    int g = cdiv(T * B, 4);
    const DecAllow al = allow ? *allow : DecAllow{};
#define SA_ARGS logits, formula, lengths, k, al, ids_out, logp_out, rank_out, ent_out, chain_err, B, T, V, Vp
    if (Vp % 4 == 0 && Vp <= 1024 && ((uintptr_t)logits & 15) == 0) {
        if (g > 2048) g = 2048;
#define SA_ROWS_AL(KV_, AL_) do { if (dt == LXO_BF16) LAUNCH((score_alt_rows_kernel<true, KV_, AL_>), g, SA_ARGS); else LAUNCH((score_alt_rows_kernel<false, KV_, AL_>), g, SA_ARGS); } while (0)
#define SA_ROWS(KV_) do { if (allow) SA_ROWS_AL(KV_, true); else SA_ROWS_AL(KV_, false); } while (0)
        BY_KV(Vp, SA_ROWS);
#undef SA_ROWS
#undef SA_ROWS_AL
    } else {
        if (g > 512) g = 512;
        if (allow) LAUNCH(score_alt_kernel<true>, g, SA_ARGS); else LAUNCH(score_alt_kernel<false>, g, SA_ARGS);
    }
#undef SA_ARGS
    DONE;
}
// The decode kernels' compile-time flags from the call's nullable arguments: KERNEL<PF, AL> with PF = a forced prefix, AL = allowed-token sets
#define DEC_VARIANT(KERNEL, grid, block, ...)                                                                         \
    do {                                                                                                               \
        if (prefix && allow) hipLaunchKernelGGL((KERNEL<true, true>), dim3(grid), dim3(block), 0, st, __VA_ARGS__);    \
        else if (prefix) hipLaunchKernelGGL((KERNEL<true, false>), dim3(grid), dim3(block), 0, st, __VA_ARGS__);       \
        else if (allow) hipLaunchKernelGGL((KERNEL<false, true>), dim3(grid), dim3(block), 0, st, __VA_ARGS__);        \
        else hipLaunchKernelGGL((KERNEL<false, false>), dim3(grid), dim3(block), 0, st, __VA_ARGS__);                  \
    } while (0)
// ... and of a register-row decode kernel KERNEL<KV, PF, AL>
#define DEC_VARIANT_KV(KERNEL, KV_, grid, block, ...)                                                                      \
    do {                                                                                                                    \
        if (prefix && allow) hipLaunchKernelGGL((KERNEL<KV_, true, true>), dim3(grid), dim3(block), 0, st, __VA_ARGS__);    \
        else if (prefix) hipLaunchKernelGGL((KERNEL<KV_, true, false>), dim3(grid), dim3(block), 0, st, __VA_ARGS__);       \
        else if (allow) hipLaunchKernelGGL((KERNEL<KV_, false, true>), dim3(grid), dim3(block), 0, st, __VA_ARGS__);        \
        else hipLaunchKernelGGL((KERNEL<KV_, false, false>), dim3(grid), dim3(block), 0, st, __VA_ARGS__);                  \
    } while (0)
int lxo_k_argmax(const float* logits, int Vp, int V, int n, int id_end, int* ids_step, int* ids_out, int max_steps, int step,
                 int* finished, int* n_unfinished, hipStream_t st, float* logp_out, const DecPrefix* prefix, const DecAllow* allow) {
    const DecPrefix pf = prefix ? *prefix : DecPrefix{};
    const DecAllow al = allow ? *allow : DecAllow{};
    DEC_VARIANT(argmax_kernel, cdiv(n, 4), 256, logits, Vp, V, n, id_end, ids_step, ids_out, max_steps, step, finished, n_unfinished, logp_out, pf, al);
    DONE;
}
int lxo_k_sample(const float* logits, int Vp, int V, int rows, int n, int id_end, int time, const DecSample& opts, int* ids_step, int* ids_out,
                 float* logp_out, float* logq_out, int max_steps, int ostep, int* finished, int* n_unfinished, hipStream_t st,
                 const DecPrefix* prefix, const DecAllow* allow) {
    if (rows < 1 || n < 1 || n > 16 || V < 1) return -2;
    DecSample so = opts;
    so.n = n;
    so.cb = 0;
    while (so.cb < 31 && (1ll << so.cb) < V) ++so.cb;
    const SmpOut o = {ids_step, ids_out, logp_out, logq_out, finished, n_unfinished, max_steps, ostep};
    const DecPrefix pf = prefix ? *prefix : DecPrefix{};
    const DecAllow al = allow ? *allow : DecAllow{};
    if (Vp % 4 == 0 && Vp <= 1024 && ((uintptr_t)logits & 15) == 0) {
#define SM_ROWS(KV_) DEC_VARIANT_KV(sample_rows_kernel, KV_, cdiv(rows, 4), 256, logits, Vp, V, rows, id_end, time, so, o, pf, al)
        BY_KV(Vp, SM_ROWS);
#undef SM_ROWS
    } else
        DEC_VARIANT(sample_kernel, cdiv(rows, 4), 256, logits, Vp, V, rows, id_end, time, so, o, pf, al);
    DONE;
}
int lxo_k_beam_step(float* logits, int Vp, int V, int nimg, int k, int id_end, int time, float div_gamma, float div_prob, int div_seed,
                    float* scratch, float* logp, int* finished,
                    int* ids_step, int* parents_step, int* ids_out, int* par_out, int max_steps, int* n_unfinished, hipStream_t st,
                    float* scores_out, const DecPrefix* prefix, const DecAllow* allow) {
    if (k > 16 || k > V) return -2;                            // k > V: at time 0 only V candidates exist -- a k-th selection would have no index
    DivPen dp = {0.f, 0u, (unsigned)div_seed, scratch};
    if (div_gamma > 0.f && div_gamma != 1.f && div_prob > 0.f) {      // the reference returns early for gamma == 1 or prob == 0
        dp.log_gamma = logf(div_gamma);
        dp.thr = div_prob >= 1.f ? 16777216u : (unsigned)(div_prob * 16777216.0f);
    }
    const int fast = lxo_switch(SW_BEAM_FAST);                 // LXO_BEAM_FAST=0: the general kernel always (A/B)
    const DecPrefix pf = prefix ? *prefix : DecPrefix{};
    const DecAllow al = allow ? *allow : DecAllow{};
    if (fast && dp.log_gamma == 0.f && (long long)k * V <= BS_TH * BS_NPT && k * BS_NW <= 64) {
        DEC_VARIANT(beam_step_fast_kernel, nimg, BS_TH, logits, Vp, V, k, id_end, time, logp, finished, ids_step, parents_step, ids_out, par_out, max_steps, n_unfinished, scores_out, pf, al);
    } else
        DEC_VARIANT(beam_step_kernel, nimg, 256, logits, Vp, V, k, id_end, time, dp, logp, finished, ids_step, parents_step, ids_out, par_out, max_steps, n_unfinished, scores_out, pf, al);
    DONE;
}
