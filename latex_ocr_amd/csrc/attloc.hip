// Where a token is in the image (lxo_attention_locate, include/lxo.h holds the definition): each attention map reduced to its arg-max cell, the
// central-mass box of its two marginals, centroid, spread, entropy, the share inside the box and the peak's share; and a row's maps added up over
// its steps into the coverage.  The maps are read where they lie, through strides: workspace region `alpha` [T][B][Rp] and the decodes' alpha_out
// [max_steps][rows][Rp] alike.
//
// One wave per position.  The map is read from memory once, lane-strided (a wave's request is one run of 256 bytes), and staged in the wave's own LDS
// row; the sum S and the arg-max come from that read.  Everything else reads the stage:
//   - THE BOX IS EXACT INTEGER ARITHMETIC.  With e = ilogb(S), cell a weighs w = trunc(max(a, 0) 2^(40 - e)): an integer below 2^41 held in a double, so
//     every sum of up to kLocateMaxCells weights is exact in any order.  The cumulative marginals are therefore exactly non-decreasing, a column of zeros adds
//     exactly nothing, both marginals have the same total Q, and the edges do not depend on how the scan associates.  What is lost is below
//     2^-40 S per cell, 2^-16 of the f32 rounding of the cells themselves.  On maps whose cells are multiples of 2^-12 summing to at most 2 nothing
//     is lost at all and the edges are those of exact arithmetic.
//   - lane x of a chunk of 64 columns adds its column's weights (consecutive lanes, consecutive LDS words); lane y adds its row's, starting at
//     column y mod Wp so that the 64 rows fall on different banks.  One inclusive scan over the lanes per chunk, two ballots for the edges.  The
//     first moments of the same weights give the centroid.
//   - a last sweep over the stage gives the centred second moments, the entropy, and the share inside the box, in f32.
// The "none" decision, the strides and every index the device holds (len, src) are read defensively; nothing outside the Hp Wp cells of a map is read.
//
// Coverage is a second launch, one thread per cell and row: the row's maps added in ascending t into one f32 accumulator, eight steps' loads in
// flight.  It takes "has a map" from what the first launch wrote (peak >= 0, else box, else stats); a call with coverage alone sums each map in
// the workgroup itself.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage) are listed in profiles/attention_locate.txt.
#include "attloc.h"
#include <math.h>

namespace {

LXO_DEV double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the map of position (i, t), NULL when it has none by its indices (the sum is the caller's to judge)
LXO_DEV const float* map_of(const LocateArgs& a, int i, int t, int len_i) {
    if (t >= len_i) return nullptr;
    const int r = a.src ? a.src[(long long)t * a.rows + i] : i;
    if (r < 0 || r >= a.alpha_rows) return nullptr;
    return a.alpha + (long long)t * a.step_stride + (long long)r * a.row_stride;
}

LXO_DEV double weight(float v, double scale) { return __builtin_trunc((double)fmaxf(v, 0.f) * scale); }

// One marginal of the staged map: n lines of m cells, line o's cell j at stage[o os + j js].  e0 = the first line whose cumulative weight exceeds
// tail, e1 = the first whose cumulative weight reaches hi, m1 = sum of o w(o).  skew: lane l starts its line at cell l mod m (the bank argument above).
LXO_DEV void marginal(const float* stage, int n, int os, int m, int js, bool skew, double scale, double tail, double hi, int lane, int& e0, int& e1, double& m1) {
    double carry = 0.0, mom = 0.0;
    e0 = e1 = -1;
    for (int o0 = 0; o0 < n; o0 += 64) {
        const int o = o0 + lane;
        double w = 0.0;
        if (o < n) {
            const float* p = stage + o * os;
            int j = skew ? lane % m : 0;
            for (int k = 0; k < m; ++k) {
                w += weight(p[j * js], scale);
                if (++j == m) j = 0;
            }
        }
        mom += w * (double)o;
        double c = w;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double up = __shfl_up(c, d);
            if (lane >= d) c += up;
        }
        c += carry;
        if (e0 < 0) {
            const unsigned long long b = __ballot(o < n && c > tail);
            if (b) e0 = o0 + (int)__builtin_ctzll(b);
        }
        if (e1 < 0) {
            const unsigned long long b = __ballot(o < n && c >= hi);
            if (b) e1 = o0 + (int)__builtin_ctzll(b);
        }
        carry = __shfl(c, 63);
    }
    // the last line's cumulative weight is Q: it exceeds tail <= Q / 2 and reaches hi <= Q, so both edges exist; the fall-back only keeps a
    // map that breaks the premise (no positive weight) inside its bounds
    if (e0 < 0) e0 = n - 1;
    if (e1 < e0) e1 = e1 < 0 ? n - 1 : e0;
    m1 = wave_sum_d(mom);
}

LXO_DEV void write_none(const LocateArgs& a, long long p) {
    if (a.peak) a.peak[p] = -1;
    if (a.box)
        for (int k = 0; k < 4; ++k) a.box[p * 4 + k] = -1;
    if (a.stats)
        for (int k = 0; k < kLocateStats; ++k) a.stats[p * kLocateStats + k] = 0.f;
}

template <int CAP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void locate_kernel(LocateArgs a) {
    __shared__ float stage_all[WAVES][CAP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long p = (long long)blockIdx.x * WAVES + wv;
    if (p >= (long long)a.rows * a.steps) return;
    const int i = (int)(p / a.steps), t = (int)(p % a.steps);
    const int Hp = a.Hp, Wp = a.Wp, R = Hp * Wp;                         // R <= CAP: the launcher's choice
    float* stage = stage_all[wv];
    const float* mp = map_of(a, i, t, a.len ? a.len[i] : a.steps);
    float S = 0.f, bv = -INFINITY;
    int bi = 0x7fffffff;
    if (mp) {
#pragma unroll 4
        for (int r = lane; r < R; r += 64) {
            const float v = mp[r];
            stage[r] = v;
            S += v;
            if (v > bv) { bv = v; bi = r; }                              // ascending r: a lane keeps its lowest arg-max
        }
        S = wave_sum(S);
    }
    if (!(mp && S > 0.f && S < INFINITY)) {                              // NaN compares false
        if (lane == 0) write_none(a, p);
        return;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    __builtin_amdgcn_wave_barrier();                                     // the stage is the wave's own (in-order LDS: no s_barrier)
    const double scale = ldexp(1.0, 40 - ilogbf(S));
    double Q = 0.0;
    for (int r = lane; r < R; r += 64) Q += weight(stage[r], scale);
    Q = wave_sum_d(Q);
    if (!(Q > 0.0)) {                                                    // negative cells ate the positive ones: no weight to place
        if (lane == 0) write_none(a, p);
        return;
    }
    const double tail = (0.5 * (1.0 - (double)a.mass)) * Q, hi = Q - tail;
    int x0, x1, y0, y1;
    double mx, my;
    marginal(stage, Wp, 1, Hp, Wp, false, scale, tail, hi, lane, x0, x1, mx);
    marginal(stage, Hp, Wp, Wp, 1, true, scale, tail, hi, lane, y0, y1, my);
    const float cx = (float)(mx / Q), cy = (float)(my / Q), inv = 1.f / S;
    float vx = 0.f, vy = 0.f, ent = 0.f, ins = 0.f;
    for (int y = 0; y < Hp; ++y) {
        const float dy = (float)y - cy;
        const bool yin = y >= y0 && y <= y1;
        for (int x = lane; x < Wp; x += 64) {
            const float v = stage[y * Wp + x], dx = (float)x - cx, q = v * inv;
            vx += v * (dx * dx);
            vy += v * (dy * dy);
            if (q > 0.f) ent -= q * logf(q);
            if (yin && x >= x0 && x <= x1) ins += v;
        }
    }
    vx = wave_sum(vx); vy = wave_sum(vy); ent = wave_sum(ent); ins = wave_sum(ins);
    if (lane == 0) {
        if (a.peak) a.peak[p] = bi;
        if (a.box) { int* b = a.box + p * 4; b[0] = x0; b[1] = y0; b[2] = x1; b[3] = y1; }
        if (a.stats) {
            float* s = a.stats + p * kLocateStats;
            s[0] = S; s[1] = cx; s[2] = cy; s[3] = sqrtf(vx * inv); s[4] = sqrtf(vy * inv); s[5] = ent; s[6] = ins * inv; s[7] = bv * inv;
        }
    }
}

// Coverage: workgroup (i, c) owns the cells c 256 .. c 256 + 255 of row i.  FLAGS: position (i, t) has a map iff flag[(i steps + t) fstride] >= fmin,
// what locate_kernel wrote.  Without: the workgroup sums the map itself, all its cells, and asks for a positive finite sum.
constexpr int kCovAhead = 8;
template <bool FLAGS>
__global__ __launch_bounds__(256) void coverage_kernel(LocateArgs a, const int* flag, int fstride, int fmin, int chunks) {
    __shared__ float part[4];
    const int i = blockIdx.x / chunks, r = (blockIdx.x % chunks) * 256 + threadIdx.x, R = a.Hp * a.Wp;
    const int len_i = a.len ? a.len[i] : a.steps;
    float acc = 0.f;
    if (FLAGS) {
        for (int t0 = 0; t0 < a.steps; t0 += kCovAhead) {
            float v[kCovAhead];
#pragma unroll
            for (int u = 0; u < kCovAhead; ++u) {
                const int t = t0 + u;
                v[u] = 0.f;                                              // acc + 0.f is acc: a position without a map adds nothing
                if (t < a.steps && r < R) {
                    const float* mp = map_of(a, i, t, len_i);
                    if (mp && flag[((long long)i * a.steps + t) * fstride] >= fmin) v[u] = mp[r];
                }
            }
#pragma unroll
            for (int u = 0; u < kCovAhead; ++u) acc += v[u];             // ascending t
        }
    } else {
        for (int t = 0; t < a.steps; ++t) {
            const float* mp = map_of(a, i, t, len_i);                    // uniform over the workgroup
            if (!mp) continue;
            float s = 0.f;
            for (int q = threadIdx.x; q < R; q += 256) s += mp[q];
            s = wave_sum(s);
            if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
            __syncthreads();
            s = (part[0] + part[1]) + (part[2] + part[3]);
            __syncthreads();
            if (s > 0.f && s < INFINITY && r < R) acc += mp[r];
        }
    }
    if (r < R) a.coverage[(long long)i * a.cov_ld + r] = acc;
}

}  // namespace

int lxo_k_attention_locate(const LocateArgs& a, hipStream_t st) {
    const long long R = (long long)a.Hp * a.Wp, pos = (long long)a.rows * a.steps;
    if (R > kLocateMaxCells || pos > 0x7fffffffll - 4) return -2;
    const bool per_pos = a.peak || a.box || a.stats;
    if (per_pos && pos > 0) {
        if (R <= 1024) hipLaunchKernelGGL((locate_kernel<1024, 4>), dim3((unsigned)cdivl(pos, 4)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((locate_kernel<kLocateMaxCells, 1>), dim3((unsigned)pos), dim3(64), 0, st, a);
    }
    if (a.coverage && a.rows > 0) {
        const int chunks = cdiv((int)R, 256);
        if ((long long)a.rows * chunks > 0x7fffffffll) return -2;
        const dim3 grid((unsigned)(a.rows * chunks));
        if (a.peak) hipLaunchKernelGGL(coverage_kernel<true>, grid, dim3(256), 0, st, a, (const int*)a.peak, 1, 0, chunks);
        else if (a.box) hipLaunchKernelGGL(coverage_kernel<true>, grid, dim3(256), 0, st, a, (const int*)a.box, 4, 0, chunks);
        else if (a.stats) hipLaunchKernelGGL(coverage_kernel<true>, grid, dim3(256), 0, st, a, reinterpret_cast<const int*>(a.stats), kLocateStats, 1, chunks);   // S > 0 as bits
        else hipLaunchKernelGGL(coverage_kernel<false>, grid, dim3(256), 0, st, a, (const int*)nullptr, 0, 0, chunks);
    }
    return (int)hipGetLastError();
}
