// Non-GEMM encoder kernels (all HBM-bound, NHWC, 8 channels = 16 B per lane):
//   conv1_pool_fwd   : u8 image -> (x-128)/128 -> 3x3 SAME conv 1->64 + bias + ReLU
//                      -> 2x2 SAME max-pool, fused so the 64-channel full-resolution
//                      activation never reaches HBM (model/encoder.py:26-34)
//   conv1_pool_bwd   : recomputes the four conv outputs of each pooled pixel to find
//                      the arg-max / ReLU mask, accumulates dW1, db1 (no dgrad: the
//                      image needs no gradient)
//   maxpool_fwd/bwd  : SAME max-pool with window == stride in {2x2, 2x1, 1x2}
//                      (encoder.py:39,47,52); bwd routes to the FIRST max of the
//                      window in (dy,dx) scan order, applies the ReLU mask of the
//                      pre-pool activation and accumulates the bias gradient
//   mask_convert     : d_y6 = d_img(f32) * (y6 > 0) -> compute dtype, + bias gradient
//   timing_signal    : positional.py:42-64 table [Hp*Wp][C] f32
#include "encoder_kernels.h"
#include "switches.h"

namespace {

template <typename CT>
__global__ __launch_bounds__(256) void conv1_pool_fwd_kernel(const uint8_t* __restrict__ img, const float* __restrict__ w,
                                                            const float* __restrict__ bias, CT* __restrict__ out,
                                                            int B, int H, int W, int Hp, int Wp) {
    const int cg = threadIdx.x & 7;            // channels cg*8 .. cg*8+7
    float wr[9][8], br[8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) wr[t][e] = w[t * 64 + cg * 8 + e];
#pragma unroll
    for (int e = 0; e < 8; ++e) br[e] = bias[cg * 8 + e];
    // A workgroup walks segments of 32 pooled pixels of one pooled row: the 4 x 66 input bytes they touch are staged
    // ONCE through LDS (normalised to float) instead of 16 predicated byte loads per thread (texture-addresser bound).
    __shared__ float sp[4][68];
    const int pl = threadIdx.x >> 3;                               // pooled pixel inside the segment
    const int segs_x = (Wp + 31) >> 5, nseg = B * Hp * segs_x;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const int row = seg / segs_x, xc = seg - row * segs_x;
        const int b = row / Hp, py = row - b * Hp;
        const int px = xc * 32 + pl;
        const uint8_t* im = img + (long long)b * H * W;
        __syncthreads();                                           // previous segment's readers are done
        for (int i = threadIdx.x; i < 4 * 66; i += 256) {
            const int dy = i / 66, dx = i - dy * 66;
            const int y = 2 * py - 1 + dy, x = 64 * xc - 1 + dx;
            sp[dy][dx] = (y >= 0 && y < H && x >= 0 && x < W) ? fmaf((float)im[y * W + x], 0.0078125f, -1.0f) : 0.f;   // (v - 128) / 128, exact
        }
        __syncthreads();
        if (px >= Wp) continue;                                    // (no barrier below this point in the iteration)
        const int pix = row * Wp + px;
        float patch[4][4];
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            const f32x2 lo = *reinterpret_cast<const f32x2*>(&sp[dy][2 * pl]), hi = *reinterpret_cast<const f32x2*>(&sp[dy][2 * pl + 2]);
            patch[dy][0] = lo[0]; patch[dy][1] = lo[1]; patch[dy][2] = hi[0]; patch[dy][3] = hi[1];
        }
        float best[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) best[e] = -3.0e38f;
#pragma unroll
        for (int qy = 0; qy < 2; ++qy)
#pragma unroll
            for (int qx = 0; qx < 2; ++qx) {
                if (2 * py + qy >= H || 2 * px + qx >= W) continue;   // SAME pool ignores padding
                // channel PAIRS on the packed-f32 FMA (v_pk_fma_f32: two lanes' worth of FMAs per issue slot)
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    f32x2 a = {br[e], br[e + 1]};
#pragma unroll
                    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) {
                            const f32x2 pp = {patch[qy + kh][qx + kw], patch[qy + kh][qx + kw]};
                            const f32x2 ww = {wr[kh * 3 + kw][e], wr[kh * 3 + kw][e + 1]};
                            a = __builtin_elementwise_fma(pp, ww, a);
                        }
                    best[e] = fmaxf(best[e], fmaxf(a[0], 0.f));
                    best[e + 1] = fmaxf(best[e + 1], fmaxf(a[1], 0.f));
                }
            }
        store8(out + (long long)pix * 64 + cg * 8, best);
    }
}

template <typename CT>
__global__ __launch_bounds__(256) void conv1_pool_bwd_kernel(const uint8_t* __restrict__ img, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const CT* __restrict__ dout,
                                                            float* __restrict__ dw, float* __restrict__ db, float* __restrict__ part,
                                                            int B, int H, int W, int Hp, int Wp) {
    __shared__ float red[4][8][80];
    const int cg = threadIdx.x & 7, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float wr[9][8], br[8], gw[9][8], gb[8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) { wr[t][e] = w[t * 64 + cg * 8 + e]; gw[t][e] = 0.f; }
#pragma unroll
    for (int e = 0; e < 8; ++e) { br[e] = bias[cg * 8 + e]; gb[e] = 0.f; }
    __shared__ float sp[4][68];
    const int pl = threadIdx.x >> 3;
    const int segs_x = (Wp + 31) >> 5, nseg = B * Hp * segs_x;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const int row = seg / segs_x, xc = seg - row * segs_x;
        const int b = row / Hp, py = row - b * Hp;
        const int px = xc * 32 + pl;
        const uint8_t* im = img + (long long)b * H * W;
        __syncthreads();
        for (int i = threadIdx.x; i < 4 * 66; i += 256) {
            const int dy = i / 66, dx = i - dy * 66;
            const int y = 2 * py - 1 + dy, x = 64 * xc - 1 + dx;
            sp[dy][dx] = (y >= 0 && y < H && x >= 0 && x < W) ? fmaf((float)im[y * W + x], 0.0078125f, -1.0f) : 0.f;
        }
        __syncthreads();
        if (px >= Wp) continue;
        const int pix = row * Wp + px;
        float patch[4][4];
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            const f32x2 lo = *reinterpret_cast<const f32x2*>(&sp[dy][2 * pl]), hi = *reinterpret_cast<const f32x2*>(&sp[dy][2 * pl + 2]);
            patch[dy][0] = lo[0]; patch[dy][1] = lo[1]; patch[dy][2] = hi[0]; patch[dy][3] = hi[1];
        }
        float g[8];
        load8(dout + (long long)pix * 64 + cg * 8, g);
        // channel PAIRS on the packed-f32 FMA; the weight gradient adds d * patch for all four pool positions with d
        // zeroed outside the winning one (4 packed FMAs instead of one FMA + three selects per tap and channel)
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            float best0 = -3.0e38f, best1 = -3.0e38f; int bq0 = 0, bq1 = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int qy = q >> 1, qx = q & 1;
                if (2 * py + qy >= H || 2 * px + qx >= W) continue;
                f32x2 a = {br[e], br[e + 1]};
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const f32x2 pp = {patch[qy + kh][qx + kw], patch[qy + kh][qx + kw]};
                        const f32x2 ww = {wr[kh * 3 + kw][e], wr[kh * 3 + kw][e + 1]};
                        a = __builtin_elementwise_fma(pp, ww, a);
                    }
                const float a0 = fmaxf(a[0], 0.f), a1 = fmaxf(a[1], 0.f);
                if (a0 > best0) { best0 = a0; bq0 = q; }
                if (a1 > best1) { best1 = a1; bq1 = q; }
            }
            const float d0 = best0 > 0.f ? g[e] : 0.f, d1 = best1 > 0.f ? g[e + 1] : 0.f;
            gb[e] += d0; gb[e + 1] += d1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int qy = q >> 1, qx = q & 1;
                const f32x2 dq = {bq0 == q ? d0 : 0.f, bq1 == q ? d1 : 0.f};
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const f32x2 pp = {patch[qy + kh][qx + kw], patch[qy + kh][qx + kw]};
                        f32x2 acc2 = {gw[kh * 3 + kw][e], gw[kh * 3 + kw][e + 1]};
                        acc2 = __builtin_elementwise_fma(pp, dq, acc2);
                        gw[kh * 3 + kw][e] = acc2[0]; gw[kh * 3 + kw][e + 1] = acc2[1];
                    }
            }
        }
    }
    // reduce over the 8 lanes-groups of a wave that share a channel group (lane bits 3..5)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = gw[t][e];
            v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
            gw[t][e] = v;
        }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float v = gb[e];
        v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
        gb[e] = v;
    }
    if (lane < 8) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int e = 0; e < 8; ++e) red[wave][cg][t * 8 + e] = gw[t][e];
#pragma unroll
        for (int e = 0; e < 8; ++e) red[wave][cg][72 + e] = gb[e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 640; i += 256) {
        const int g8 = i / 80, k = i % 80;
        const float v = red[0][g8][k] + red[1][g8][k] + red[2][g8][k] + red[3][g8][k];
        if (part) {          // f32 parity mode: this workgroup's slot [dw 576 | db 64]; lxo_k_det_reduce adds the slots in order
            if (k < 72) part[(long long)blockIdx.x * 640 + (k >> 3) * 64 + g8 * 8 + (k & 7)] = v;
            else part[(long long)blockIdx.x * 640 + 576 + g8 * 8 + (k - 72)] = v;
        }
        else if (k < 72) atomicAdd(&dw[(k >> 3) * 64 + g8 * 8 + (k & 7)], v);
        else atomicAdd(&db[g8 * 8 + (k - 72)], v);
    }
}


// ---- bf16 mode: conv1 + ReLU + 2x2 pool on the matrix cores ----
// The VALU kernels above spend 2.4 G FMAs per pass over the batch (80 us forward, 216 us backward at B = 64, 128 x 512) for a
// layer whose memory traffic is 134 MB.  Here a wave treats 8 pooled pixels = 32 full-resolution pixels as one 32 x 16 x 32
// MFMA tile:  pre[pixel][channel] = sum_tap x[pixel + tap] w[tap][channel]  with K = 9 taps padded to 16.
//   * tile row m = 4 * window + q (q = position inside the 2 x 2 pool window), so a lane's accumulator registers r, r+1, r+2,
//     r+3 ARE the four pool positions of one window: pooling is three v_max per (window, channel), no cross-lane traffic;
//   * the two MFMAs of a tile take the EVEN and the ODD channels (the column order of the weight operand is free), so lane n
//     ends up with channels 2n and 2n+1 of the same pixels: one packed 4-byte store per window, 128 contiguous bytes per wave;
//   * the image values (v - 128) / 128 are exact in bf16; the weights are rounded to bf16 like every other layer's.
// Backward recomputes the tile the same way (so the argmax is the forward's), routes d through first-max + ReLU in registers,
// and contracts  dW[tap][channel] = sum_pixel x[pixel + tap] d[pixel][channel]  with the d tile taken straight from those
// registers as the MFMA B operand (k = pixel), the shifted image rows gathered from the LDS patch as the A operand (m = tap).
typedef __attribute__((ext_vector_type(16))) float c1_v16f;
LXO_DEV c1_v16f c1_mfma(u32x4 a, u32x4 b, c1_v16f c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
constexpr int C1_SEG = 128;                       // pooled pixels per workgroup pass (4 waves x 4 tiles x 8)
constexpr int C1_PW = 2 * C1_SEG + 8;             // patch row pitch in elements (2 * 128 + 2 halo columns used)

// The patch (image rows 2py-1 .. 2py+2, columns 256*xc-1 .. 256*xc+256 as bf16 (v - 128) / 128, zero outside the image) is
// kept TWICE, the second copy shifted by one element: every (column, column + 1) pair the MFMA operands need is then one
// ALIGNED 4-byte LDS read from the copy of matching parity, already in operand order -- no 2-byte reads, no packing.
struct C1Patch { bf16_t e[4][C1_PW]; bf16_t o[4][C1_PW]; };      // o[r][j] = e[r][j + 1]
constexpr int C1_NF = (4 * (2 * C1_SEG + 2) + 255) / 256;        // patch bytes per thread
// The patch of pass i+1 is requested (into registers) before pass i computes and written to the other LDS buffer after it:
// the image round trip hides behind the MFMA work, one barrier per pass.  Loads are unconditional (clamped address).
struct C1Fetch { unsigned char v[C1_NF]; };
LXO_DEV void c1_fetch(C1Fetch& f, const uint8_t* im, int H, int W, int py, int xc) {
#pragma unroll
    for (int k = 0; k < C1_NF; ++k) {
        const int i = min((int)threadIdx.x + 256 * k, 4 * (2 * C1_SEG + 2) - 1);
        const int dy = i / (2 * C1_SEG + 2), dx = i - dy * (2 * C1_SEG + 2);
        const int y = 2 * py - 1 + dy, x = 2 * C1_SEG * xc - 1 + dx;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const unsigned char b = im[in ? y * W + x : 0];
        f.v[k] = in ? b : (unsigned char)128;                     // 128 -> (128 - 128) / 128 = 0: the zero padding
    }
}
LXO_DEV void c1_commit(C1Patch& sp, const C1Fetch& f) {
#pragma unroll
    for (int k = 0; k < C1_NF; ++k) {
        const int i = (int)threadIdx.x + 256 * k;
        if (i < 4 * (2 * C1_SEG + 2)) {
            const int dy = i / (2 * C1_SEG + 2), dx = i - dy * (2 * C1_SEG + 2);
            const bf16_t q = f2bf(fmaf((float)f.v[k], 0.0078125f, -1.0f));      // (v - 128) / 128, exact in bf16
            sp.e[dy][dx] = q;
            if (dx > 0) sp.o[dy][dx - 1] = q;
        }
    }
}
LXO_DEV unsigned c1_pair(const bf16_t* row, int col) { return *reinterpret_cast<const unsigned*>(row + col); }   // col even
// weight operand of the even (e = 0) / odd (e = 1) channels: lane n -> channel 2n + e, k = tap
LXO_DEV u32x4 c1_wop(const float* w, int lane, int e) {
    const int ch = 2 * (lane & 31) + e, h = lane >> 5;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int t = 8 * h + i; v[i] = t < 9 ? w[t * 64 + ch] : 0.f; }
    return u32x4{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
}
// image operand of the forward product: lane m = pixel 4 * window + q of the tile, k = tap (kh * 3 + kw).
// With c = 2 * (pw0 + window) + qx the taps of row r sit at columns c, c+1, c+2 of patch row qy + r.
LXO_DEV u32x4 c1_xop(const C1Patch& sp, int lane, int pw0) {
    const int m = lane & 31, h = lane >> 5, q = m & 3, qy = q >> 1, qx = q & 1;
    const bf16_t (*cp)[C1_PW] = qx ? sp.o : sp.e;                 // copy whose even columns are c, c + 2
    const int cb = 2 * (pw0 + (m >> 2));
    const unsigned p00 = c1_pair(cp[qy], cb), p02 = c1_pair(cp[qy], cb + 2);
    const unsigned p10 = c1_pair(cp[qy + 1], cb), p12 = c1_pair(cp[qy + 1], cb + 2);
    const unsigned p20 = c1_pair(cp[qy + 2], cb), p22 = c1_pair(cp[qy + 2], cb + 2);
    const u32x4 lo = {p00, (p02 & 0xffffu) | (p10 << 16), __builtin_amdgcn_alignbit(p12, p10, 16), p20};     // taps 0..7
    const u32x4 hi = {p22 & 0xffffu, 0u, 0u, 0u};                                                             // tap 8
    return h ? hi : lo;
}

__global__ __launch_bounds__(256) void conv1_pool_fwd_mfma_kernel(const uint8_t* __restrict__ img, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, bf16_t* __restrict__ out,
                                                                 int B, int H, int W, int Hp, int Wp) {
    __shared__ __attribute__((aligned(16))) C1Patch spb[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, h = lane >> 5;
    const u32x4 w0 = c1_wop(w, lane, 0), w1 = c1_wop(w, lane, 1);
    const float b0 = bias[2 * n], b1 = bias[2 * n + 1];           // added after the pool: max(v + b) = max(v) + b
    c1_v16f z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    const int segs_x = (Wp + C1_SEG - 1) / C1_SEG, nseg = B * Hp * segs_x;
    if ((int)blockIdx.x >= nseg) return;
    C1Fetch nf;
    {
        const int row = blockIdx.x / segs_x, xc = blockIdx.x - row * segs_x, b = row / Hp, py = row - b * Hp;
        c1_fetch(nf, img + (long long)b * H * W, H, W, py, xc);
        c1_commit(spb[0], nf);
    }
    __syncthreads();
    int cur = 0;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x, cur ^= 1) {
        const int row = seg / segs_x, xc = seg - row * segs_x;
        const int b = row / Hp, py = row - b * Hp;
        {
            const int ns = min(seg + (int)gridDim.x, nseg - 1);    // next pass (clamped: the last pass re-fetches its own patch)
            const int nrow = ns / segs_x, nxc = ns - nrow * segs_x, nb = nrow / Hp;
            c1_fetch(nf, img + (long long)nb * H * W, H, W, nrow - nb * Hp, nxc);
        }
        const C1Patch& sp = spb[cur];
        const bool edge = 2 * py + 1 >= H || (W & 1);              // block-uniform: some pool windows reach past the image
#pragma unroll
        for (int tile = 0; tile < 4; ++tile) {
            const int pw0 = wave * 32 + tile * 8;
            const u32x4 xa = c1_xop(sp, lane, pw0);
            c1_v16f a0 = c1_mfma(xa, w0, z), a1 = c1_mfma(xa, w1, z);
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int px = xc * C1_SEG + pw0 + 2 * g4 + h;     // this lane's window
                if (edge) {                                        // SAME pool ignores padding
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const bool ok = 2 * py + (q >> 1) < H && 2 * px + (q & 1) < W;
                        a0[4 * g4 + q] = ok ? a0[4 * g4 + q] : -3.0e38f; a1[4 * g4 + q] = ok ? a1[4 * g4 + q] : -3.0e38f;
                    }
                }
                const float m0 = fmaxf(fmaxf(a0[4 * g4], a0[4 * g4 + 1]), fmaxf(a0[4 * g4 + 2], a0[4 * g4 + 3]));
                const float m1 = fmaxf(fmaxf(a1[4 * g4], a1[4 * g4 + 1]), fmaxf(a1[4 * g4 + 2], a1[4 * g4 + 3]));
                const unsigned o = pack_bf2(fmaxf(m0 + b0, 0.f), fmaxf(m1 + b1, 0.f));
                if (px < Wp) *reinterpret_cast<unsigned*>(out + ((long long)row * Wp + px) * 64 + 2 * n) = o;
            }
        }
        c1_commit(spb[cur ^ 1], nf);                               // nobody reads that buffer during this pass
        __syncthreads();
    }
}

// first maximum of the four pool positions (scan order, as the forward's fmaxf chain keeps it), ReLU, and the routed gradient
LXO_DEV void c1_route(const c1_v16f& a, int g4, float bias, float g, float (&d)[16], float& gsum) {
    const float v0 = a[4 * g4], v1 = a[4 * g4 + 1], v2 = a[4 * g4 + 2], v3 = a[4 * g4 + 3];      // without the bias: it does not move the argmax
    const float best = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
    const float gg = best + bias > 0.f ? g : 0.f;                  // ReLU: a window whose maximum is not positive passes nothing
    const bool s0 = v0 == best, s1 = !s0 && v1 == best, s2 = !s0 && !s1 && v2 == best, s3 = !s0 && !s1 && !s2;
    d[4 * g4] = s0 ? gg : 0.f; d[4 * g4 + 1] = s1 ? gg : 0.f; d[4 * g4 + 2] = s2 ? gg : 0.f; d[4 * g4 + 3] = s3 ? gg : 0.f;
    gsum += gg;
}

__global__ __launch_bounds__(256) void conv1_pool_bwd_mfma_kernel(const uint8_t* __restrict__ img, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, const bf16_t* __restrict__ dout,
                                                                 float* __restrict__ dw, float* __restrict__ db, float* __restrict__ part,
                                                                 int B, int H, int W, int Hp, int Wp) {
    __shared__ __attribute__((aligned(16))) C1Patch spb[2];
    __shared__ float red[4][10][64];                               // per wave: 9 taps + bias, 64 channels
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 31, h = lane >> 5;
    const u32x4 w0 = c1_wop(w, lane, 0), w1 = c1_wop(w, lane, 1);
    const float b0 = bias[2 * n], b1 = bias[2 * n + 1];
    c1_v16f z, gw0, gw1;                                           // gw: dW tile [tap][channel], even / odd channels
#pragma unroll
    for (int r = 0; r < 16; ++r) { z[r] = 0.f; gw0[r] = 0.f; gw1[r] = 0.f; }
    float gb0 = 0.f, gb1 = 0.f;
    // dW product: lane m = tap (rows >= 9 are never read back), k = pixel.  Tap (kh, kw) of pixel (window, qy, qx) reads patch
    // row qy + kh, column 2 * window + qx + kw: the (qx = 0, qx = 1) pair is one aligned dword of the copy of kw's parity.
    const int tp = n < 9 ? n : 0, tkh = tp / 3, tkw = tp - 3 * tkh;
    const int tcb = 2 * (tkw >> 1);
    const int segs_x = (Wp + C1_SEG - 1) / C1_SEG, nseg = B * Hp * segs_x;
    // d_out of a pass: this lane's four windows of each of the wave's four tiles, channels 2n, 2n+1 (unconditional, clamped)
    auto fetch_g = [&](unsigned (&g)[16], int row, int xc) {
#pragma unroll
        for (int tile = 0; tile < 4; ++tile)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int px = xc * C1_SEG + wave * 32 + tile * 8 + 2 * g4 + h;
                const unsigned v = *reinterpret_cast<const unsigned*>(dout + ((long long)row * Wp + (px < Wp ? px : 0)) * 64 + 2 * n);
                g[4 * tile + g4] = px < Wp ? v : 0u;
            }
    };
    C1Fetch nf;
    unsigned gq[16], gn[16];
    if ((int)blockIdx.x < nseg) {
        const int row = blockIdx.x / segs_x, xc = blockIdx.x - row * segs_x, b = row / Hp, py = row - b * Hp;
        c1_fetch(nf, img + (long long)b * H * W, H, W, py, xc);
        fetch_g(gn, row, xc);
        c1_commit(spb[0], nf);
    }
    __syncthreads();
    int cur = 0;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x, cur ^= 1) {
        const int row = seg / segs_x, xc = seg - row * segs_x;
        const int b = row / Hp, py = row - b * Hp;
#pragma unroll
        for (int i = 0; i < 16; ++i) gq[i] = gn[i];
        {
            const int ns = min(seg + (int)gridDim.x, nseg - 1);    // next pass (clamped), requested before this pass computes
            const int nrow = ns / segs_x, nxc = ns - nrow * segs_x, nb = nrow / Hp;
            c1_fetch(nf, img + (long long)nb * H * W, H, W, nrow - nb * Hp, nxc);
            fetch_g(gn, nrow, nxc);
        }
        const C1Patch& sp = spb[cur];
        const bf16_t (*tcp)[C1_PW] = (tkw & 1) ? sp.o : sp.e;
        const bool edge = 2 * py + 1 >= H || (W & 1);
#pragma unroll
        for (int tile = 0; tile < 4; ++tile) {
            const int pw0 = wave * 32 + tile * 8;
            const u32x4 xa = c1_xop(sp, lane, pw0);
            c1_v16f a0 = c1_mfma(xa, w0, z), a1 = c1_mfma(xa, w1, z);
            if (edge) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int px = xc * C1_SEG + pw0 + 2 * g4 + h;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const bool ok = 2 * py + (q >> 1) < H && 2 * px + (q & 1) < W;
                        a0[4 * g4 + q] = ok ? a0[4 * g4 + q] : -3.0e38f; a1[4 * g4 + q] = ok ? a1[4 * g4 + q] : -3.0e38f;
                    }
                }
            }
            // dW += X^T D: k-step s covers the pixels of accumulator registers 8s .. 8s+7, i.e. tile rows
            // (i & 3) + 8 (i >> 2) + 4 h + 16 s  =  windows h + 4s (i < 4) and h + 4s + 2 (i >= 4), positions q = i & 3;
            // the two windows of a k-step are routed and contracted before the next two are touched (registers)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                float d0[16], d1[16];
#pragma unroll
                for (int g4 = 2 * s2; g4 < 2 * s2 + 2; ++g4) {
                    c1_route(a0, g4, b0, __uint_as_float(gq[4 * tile + g4] << 16), d0, gb0);
                    c1_route(a1, g4, b1, __uint_as_float(gq[4 * tile + g4] & 0xffff0000u), d1, gb1);
                }
                const u32x4 db0 = {pack_bf2(d0[8 * s2], d0[8 * s2 + 1]), pack_bf2(d0[8 * s2 + 2], d0[8 * s2 + 3]),
                                   pack_bf2(d0[8 * s2 + 4], d0[8 * s2 + 5]), pack_bf2(d0[8 * s2 + 6], d0[8 * s2 + 7])};
                const u32x4 db1 = {pack_bf2(d1[8 * s2], d1[8 * s2 + 1]), pack_bf2(d1[8 * s2 + 2], d1[8 * s2 + 3]),
                                   pack_bf2(d1[8 * s2 + 4], d1[8 * s2 + 5]), pack_bf2(d1[8 * s2 + 6], d1[8 * s2 + 7])};
                const int cb = 2 * (pw0 + h + 4 * s2) + tcb;
                const u32x4 xt = {c1_pair(tcp[tkh], cb), c1_pair(tcp[tkh + 1], cb), c1_pair(tcp[tkh], cb + 4), c1_pair(tcp[tkh + 1], cb + 4)};
                gw0 = c1_mfma(xt, db0, gw0);
                gw1 = c1_mfma(xt, db1, gw1);
            }
        }
        c1_commit(spb[cur ^ 1], nf);
        __syncthreads();
    }
    // taps live in rows (r & 3) + 8 (r >> 2) + 4 h: r = 0..3 -> taps 0..3 (h = 0) / 4..7 (h = 1), r = 4, h = 0 -> tap 8
    gb0 += __shfl_xor(gb0, 32); gb1 += __shfl_xor(gb1, 32);
#pragma unroll
    for (int r = 0; r < 4; ++r) { red[wave][4 * h + r][2 * n] = gw0[r]; red[wave][4 * h + r][2 * n + 1] = gw1[r]; }
    if (h == 0) { red[wave][8][2 * n] = gw0[4]; red[wave][8][2 * n + 1] = gw1[4]; red[wave][9][2 * n] = gb0; red[wave][9][2 * n + 1] = gb1; }
    __syncthreads();
    for (int i = threadIdx.x; i < 640; i += 256) {
        const int t = i >> 6, c = i & 63;
        const float v = red[0][t][c] + red[1][t][c] + red[2][t][c] + red[3][t][c];
        if (part) part[(long long)blockIdx.x * 640 + i] = v;       // deterministic mode: this workgroup's slot [dw 576 | db 64]; lxo_k_det_reduce adds the slots in order
        else if (t < 9) atomicAdd(&dw[t * 64 + c], v); else atomicAdd(&db[c], v);
    }
}

template <typename CT>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const CT* __restrict__ in, CT* __restrict__ out,
                                                         int B, int H, int W, int C, int ph, int pw, int Ho, int Wo) {
    const int cgs = C >> 3;
    const int total = B * Ho * Wo * cgs;          // < 2^31 for every shape the plan accepts; 32-bit index arithmetic
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int pix = i / cgs, cg = i - pix * cgs;
        const int row = pix / Wo, ox = pix - row * Wo;
        const int b = row / Ho, oy = row - b * Ho;
        float best[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) best[e] = -3.0e38f;
        for (int dy = 0; dy < ph; ++dy)
            for (int dx = 0; dx < pw; ++dx) {
                const int y = oy * ph + dy, x = ox * pw + dx;
                if (y >= H || x >= W) continue;
                float v[8];
                load8(in + (((long long)b * H + y) * W + x) * C + cg * 8, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) best[e] = fmaxf(best[e], v[e]);
            }
        store8(out + (long long)pix * C + cg * 8, best);
    }
}

// d_y = route(d_p) * (y > 0); db[c] += sum d_y.   One thread per pooled pixel x 8 channels.
template <typename CT>
__global__ __launch_bounds__(256) void maxpool_relu_bwd_kernel(const CT* __restrict__ y, const CT* __restrict__ dp,
                                                              CT* __restrict__ dyo, float* __restrict__ db,
                                                              int B, int H, int W, int C, int ph, int pw, int Ho, int Wo) {
    __shared__ float dbs[512];
    for (int i = threadIdx.x; i < C; i += 256) dbs[i] = 0.f;
    __syncthreads();
    const int cgs = C >> 3;                   // divides 256 (C in {64,128,256,512})
    const int cg = threadIdx.x % cgs;
    const int ppb = 256 / cgs;                // pooled pixels per block per iteration
    const int npix = B * Ho * Wo;
    float gb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) gb[e] = 0.f;
    for (int pix = blockIdx.x * ppb + threadIdx.x / cgs; pix < npix; pix += gridDim.x * ppb) {
        const int row = pix / Wo, ox = pix - row * Wo;
        const int b = row / Ho, oy = row - b * Ho;
        float best[8]; int bq[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { best[e] = -3.0e38f; bq[e] = 0; }
        for (int qy = 0; qy < ph; ++qy)
            for (int qx = 0; qx < pw; ++qx) {
                const int yy = oy * ph + qy, xx = ox * pw + qx;
                if (yy >= H || xx >= W) continue;
                float v[8];
                load8(y + (((long long)b * H + yy) * W + xx) * C + cg * 8, v);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (v[e] > best[e]) { best[e] = v[e]; bq[e] = qy * pw + qx; }
            }
        float g[8];
        load8(dp + (long long)pix * C + cg * 8, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) { g[e] = best[e] > 0.f ? g[e] : 0.f; gb[e] += g[e]; }
        for (int qy = 0; qy < ph; ++qy)
            for (int qx = 0; qx < pw; ++qx) {
                const int yy = oy * ph + qy, xx = ox * pw + qx;
                if (yy >= H || xx >= W) continue;
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (bq[e] == qy * pw + qx) ? g[e] : 0.f;
                store8(dyo + (((long long)b * H + yy) * W + xx) * C + cg * 8, o);
            }
    }
    if (db) {
#pragma unroll
        for (int e = 0; e < 8; ++e) atomicAdd(&dbs[cg * 8 + e], gb[e]);
        __syncthreads();
        for (int i = threadIdx.x; i < C; i += 256) atomicAdd(&db[i], dbs[i]);
    }
}

// Pool backward from the mask the fused conv + pool epilogue wrote (conv_igemm.hip, EPI 4): one byte per pooled element,
// first-max position | 4 if the maximum was positive (ReLU).  Reads d_pooled + the mask instead of re-reading the
// full-resolution activation (pool 2x2 on conv2: 369 MB instead of 603 MB); every load and store is unconditional in count.
template <int PH, int PW>
__global__ __launch_bounds__(256) void maxpool_mask_bwd_kernel(const unsigned char* __restrict__ mask, const bf16_t* __restrict__ dp,
                                                              bf16_t* __restrict__ dyo, float* __restrict__ db, float* __restrict__ db_part,
                                                              int B, int H, int W, int C, int Ho, int Wo) {
    constexpr int ph = PH, pw = PW;           // compile-time window: the position loop unrolls into straight-line selects and stores
    __shared__ float dbs[512];
    for (int i = threadIdx.x; i < C; i += 256) dbs[i] = 0.f;
    __syncthreads();
    const int cgs = C >> 3;                   // divides 256 (C in {64,128,256,512})
    const int cg = threadIdx.x % cgs;
    const int ppb = 256 / cgs;                // pooled pixels per block per iteration
    const int npix = B * Ho * Wo;
    float gb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) gb[e] = 0.f;
    // four pooled pixels per thread and iteration: their loads (unconditional, index clamped) are all requested before the first
    // store, or the loop is one dependent load -> store round trip per pixel
    constexpr int UNR = 4;
    const int stride = gridDim.x * ppb;
    for (int pix0 = blockIdx.x * ppb + threadIdx.x / cgs; pix0 < npix; pix0 += UNR * stride) {
        u32x4 g4s[UNR]; u32x2 m2s[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const long long pc = min(pix0 + u * stride, npix - 1);
            g4s[u] = *reinterpret_cast<const u32x4*>(dp + pc * C + cg * 8);
            m2s[u] = *reinterpret_cast<const u32x2*>(mask + pc * C + cg * 8);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int pix = pix0 + u * stride;
            if (pix >= npix) break;
            const u32x4 g4 = g4s[u]; const u32x2 m2 = m2s[u];
            const int row = pix / Wo, ox = pix - row * Wo;
            const int b = row / Ho, oy = row - b * Ho;
            unsigned gm[4];                                              // d_pooled with the ReLU bit applied, still packed
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const unsigned mlo = (m2[d >> 1] >> (16 * (d & 1))) & 0xffu, mhi = (m2[d >> 1] >> (16 * (d & 1) + 8)) & 0xffu;
                const unsigned lo = (mlo & 4u) ? (g4[d] & 0xffffu) : 0u, hi = (mhi & 4u) ? (g4[d] & 0xffff0000u) : 0u;
                gm[d] = lo | hi;
                gb[2 * d] += __uint_as_float(lo << 16); gb[2 * d + 1] += __uint_as_float(hi);
            }
#pragma unroll
            for (int qy = 0; qy < ph; ++qy)
#pragma unroll
                for (int qx = 0; qx < pw; ++qx) {
                    const int yy = oy * ph + qy, xx = ox * pw + qx;
                    if (yy >= H || xx >= W) continue;
                    const unsigned q = (unsigned)(qy * pw + qx);
                    u32x4 o;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const unsigned mlo = (m2[d >> 1] >> (16 * (d & 1))) & 3u, mhi = (m2[d >> 1] >> (16 * (d & 1) + 8)) & 3u;
                        o[d] = (mlo == q ? (gm[d] & 0xffffu) : 0u) | (mhi == q ? (gm[d] & 0xffff0000u) : 0u);
                    }
                    *reinterpret_cast<u32x4*>(dyo + (((long long)b * H + yy) * W + xx) * C + cg * 8) = o;
                }
        }
    }
    if (db_part) {
        // deterministic mode: no atomics, neither in LDS nor in memory -- the threads' sums of a column meet in thread order, the workgroup's
        // sums go to ITS slot [C] and lxo_k_det_reduce adds the slots in workgroup order
        __shared__ float dbo[256 * 8];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) dbo[threadIdx.x * 8 + e] = gb[e];
        __syncthreads();
        for (int i = threadIdx.x; i < C; i += 256) {
            const int g = i >> 3, e = i & 7;
            float s = 0.f;
            for (int r = 0; r < ppb; ++r) s += dbo[(r * cgs + g) * 8 + e];
            db_part[(long long)blockIdx.x * C + i] = s;
        }
    } else if (db) {
#pragma unroll
        for (int e = 0; e < 8; ++e) atomicAdd(&dbs[cg * 8 + e], gb[e]);
        __syncthreads();
        for (int i = threadIdx.x; i < C; i += 256) atomicAdd(&db[i], dbs[i]);
    }
}

// out = d(f32) * (ref > 0) in the compute dtype; db[c] += column sums.
template <typename CT>
__global__ __launch_bounds__(256) void mask_convert_kernel(const float* __restrict__ d, const CT* __restrict__ ref,
                                                          CT* __restrict__ out, float* __restrict__ db,
                                                          long long rows, int C) {
    __shared__ float dbs[512];
    for (int i = threadIdx.x; i < C; i += 256) dbs[i] = 0.f;
    __syncthreads();
    const int cgs = C >> 3;
    const int cg = threadIdx.x % cgs;
    const int rpb = 256 / cgs;
    float gb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) gb[e] = 0.f;
    for (long long r = (long long)blockIdx.x * rpb + threadIdx.x / cgs; r < rows; r += (long long)gridDim.x * rpb) {
        float g[8], v[8];
        load8(d + r * C + cg * 8, g);
        load8(ref + r * C + cg * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) { g[e] = v[e] > 0.f ? g[e] : 0.f; gb[e] += g[e]; }
        store8(out + r * C + cg * 8, g);
    }
    if (db) {
#pragma unroll
        for (int e = 0; e < 8; ++e) atomicAdd(&dbs[cg * 8 + e], gb[e]);
        __syncthreads();
        for (int i = threadIdx.x; i < C; i += 256) atomicAdd(&db[i], dbs[i]);
    }
}

// positional.py:42-64: channels [sin_h | cos_h | sin_w | cos_w], C/4 timescales each
__global__ __launch_bounds__(256) void timing_signal_kernel(float* __restrict__ pos, int Hp, int Wp, int C) {
    const int nts = C / 4;
    const float inc = logf(1.0e4f / 1.0f) / ((float)nts - 1.f);
    const long long total = (long long)Hp * Wp * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const int w = (int)((i / C) % Wp), h = (int)(i / ((long long)C * Wp));
        const int q = c / nts, k = c - q * nts;
        const float inv = expf((float)k * -inc);
        const float t = (q < 2 ? (float)h : (float)w) * inv;
        pos[i] = (q & 1) ? cosf(t) : sinf(t);
    }
}

// ---- weight packing (master f32 TF layouts -> compute-dtype GEMM operands) ----
// dst[n][coff + k] = k < K ? src[k*lds + n] : 0   for n < N, k < Kpad
template <typename CT>
__global__ __launch_bounds__(256) void pack_transpose_kernel(const float* __restrict__ src, CT* __restrict__ dst,
                                                            int K, int N, int lds, int ldd, int coff, int Kpad) {
    __shared__ float tile[32][33];
    const int k0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, n = n0 + tx;
        tile[r][tx] = (k < K && n < N) ? src[(long long)k * lds + n] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int n = n0 + r, k = k0 + tx;
        if (n < N && k < Kpad) dst[(long long)n * ldd + coff + k] = from_f32<CT>(tile[tx][r]);
    }
}
// dst[r][c] = c < Ccols ? src[r*lds + c] : 0   for r < R, c < Cpad
template <typename CT>
__global__ __launch_bounds__(256) void pack_copy_kernel(const float* __restrict__ src, CT* __restrict__ dst,
                                                       int R, int Ccols, int lds, int ldd, int Cpad) {
    const long long total = (long long)R * Cpad;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % Cpad); const long long r = i / Cpad;
        dst[r * ldd + c] = from_f32<CT>(c < Ccols ? src[r * lds + c] : 0.f);
    }
}
// conv dgrad operand: dst[ci][(a*3+b)*Cout + co] = W[((2-a)*3+(2-b))*Cin + ci][co]
template <typename CT>
__global__ __launch_bounds__(256) void pack_conv_dgrad_kernel(const float* __restrict__ w, CT* __restrict__ dst, int Cin, int Cout) {
    const long long total = (long long)Cin * 9 * Cout;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int co = (int)(i % Cout);
        const int tap = (int)((i / Cout) % 9);
        const int ci = (int)(i / ((long long)Cout * 9));
        const int a = tap / 3, b = tap - 3 * a;
        dst[i] = from_f32<CT>(w[((long long)((2 - a) * 3 + (2 - b)) * Cin + ci) * Cout + co]);
    }
}

// All weight packs of one optimizer step in ONE launch: a table of jobs, each a 32x32-tiled transpose
// (kind 0), a padded row copy (kind 1) or the flipped-tap dgrad layout (kind 2); blockIdx -> job by prefix sums.
template <typename CT>
__global__ __launch_bounds__(256) void pack_batch_kernel(PackTable tab, const float* __restrict__ prm, char* __restrict__ wpk) {
    __shared__ float tile[32][33];
    int j = 0;
    while (j + 1 < tab.n && (int)blockIdx.x >= tab.job[j + 1].first_block) ++j;
    const PackJob q = tab.job[j];
    const int lb = blockIdx.x - q.first_block;
    const float* src = prm + q.src;
    CT* dst = reinterpret_cast<CT*>(wpk + q.dst);
    if (q.kind == 0) {
        const int tiles_k = (q.Kpad + 31) / 32;
        const int k0 = (lb % tiles_k) * 32, n0 = (lb / tiles_k) * 32;
        const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
        for (int r = ty; r < 32; r += 8) {
            const int k = k0 + r, n = n0 + tx;
            tile[r][tx] = (k < q.K && n < q.N) ? src[(long long)k * q.lds + n] : 0.f;
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const int n = n0 + r, k = k0 + tx;
            if (n < q.N && k < q.Kpad) dst[(long long)n * q.ldd + q.coff + k] = from_f32<CT>(tile[tx][r]);
        }
    } else if (q.kind == 1) {
        const long long total = (long long)q.K * q.Kpad;       // rows K, padded columns Kpad, real columns N
        for (long long i = (long long)lb * 256 + threadIdx.x; i < total; i += (long long)q.nblocks * 256) {
            const int c = (int)(i % q.Kpad); const long long r = i / q.Kpad;
            dst[r * q.ldd + c] = from_f32<CT>(c < q.N ? src[r * q.lds + c] : 0.f);
        }
    } else {
        const int Cin = q.K, Cout = q.N;
        const long long total = (long long)Cin * 9 * Cout;
        for (long long i = (long long)lb * 256 + threadIdx.x; i < total; i += (long long)q.nblocks * 256) {
            const int co = (int)(i % Cout);
            const int tap = (int)((i / Cout) % 9);
            const int ci = (int)(i / ((long long)Cout * 9));
            const int a = tap / 3, b = tap - 3 * a;
            dst[i] = from_f32<CT>(src[((long long)((2 - a) * 3 + (2 - b)) * Cin + ci) * Cout + co]);
        }
    }
}


// ---- "cnn" encoder: the (2,4) stride-2 SAME convolution of encoder.py:54-56 as im2col + dense GEMM ----
// TF SAME padding for kernel (2,4), stride 2: rows pad (0 top, 0/1 bottom), columns pad (1 left, 1/2 right).
// cols[(b,oy,ox)][(kh,kw,c)] = in[b, 2oy+kh, 2ox+kw-1, c]   (zero outside)
template <typename CT>
__global__ __launch_bounds__(256) void im2col_s2_kernel(const CT* __restrict__ in, CT* __restrict__ cols, int B, int H, int W, int Ho, int Wo, int C) {
    const int c8n = C >> 3;
    const long long total = (long long)B * Ho * Wo * 8 * c8n;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c8 = (int)(i % c8n);
        const int tap = (int)((i / c8n) & 7);
        const long long m = i / (8 * c8n);
        const int ox = (int)(m % Wo), oy = (int)((m / Wo) % Ho), b = (int)(m / ((long long)Wo * Ho));
        const int iy = 2 * oy + (tap >> 2), ix = 2 * ox + (tap & 3) - 1;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (iy < H && ix >= 0 && ix < W) load8(in + (((long long)b * H + iy) * W + ix) * C + c8 * 8, v);
        store8(cols + (m * 8 + tap) * C + c8 * 8, v);
    }
}
// dy[b,y,x,c] = (y5 > 0) * sum over the <= 2 windows covering (y,x) of dcols ;  db[c] += column sums of dy
template <typename CT>
__global__ __launch_bounds__(256) void col2im_s2_relu_kernel(const CT* __restrict__ dcols, const CT* __restrict__ yref, CT* __restrict__ dy,
                                                            float* __restrict__ db, int B, int H, int W, int Ho, int Wo, int C, int ppt) {
    const int c8n = C >> 3;
    const long long npix = (long long)B * H * W;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c8 = (int)(t % c8n);
    const long long p0 = (t / c8n) * ppt;
    if (p0 >= npix) return;
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const long long p1 = p0 + ppt < npix ? p0 + ppt : npix;
    for (long long p = p0; p < p1; ++p) {
        const int x = (int)(p % W), y = (int)((p / W) % H), b = (int)(p / ((long long)W * H));
        const int oy = y >> 1, kh = y & 1;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (oy < Ho) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int kw = ((x + 1) & 1) + 2 * h;
                const int ox2 = x + 1 - kw;                 // = 2 * ox
                if (ox2 < 0 || (ox2 >> 1) >= Wo) continue;
                float v[8];
                load8(dcols + ((((long long)b * Ho + oy) * Wo + (ox2 >> 1)) * 8 + kh * 4 + kw) * C + c8 * 8, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += v[e];
            }
        }
        float r[8];
        load8(yref + p * C + c8 * 8, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) { acc[e] = r[e] > 0.f ? acc[e] : 0.f; cs[e] += acc[e]; }
        store8(dy + p * C + c8 * 8, acc);
    }
    if (!db) return;             // f32 parity mode: the caller sums the columns of dy in a fixed order instead
#pragma unroll
    for (int e = 0; e < 8; ++e) atomicAdd(&db[c8 * 8 + e], cs[e]);
}
// out[n] += sum_m a[m][n] for a compute-dtype matrix (bias gradient of the strided conv)
template <typename CT>
__global__ __launch_bounds__(256) void colsum_ct_kernel(const CT* __restrict__ a, float* __restrict__ out, long long M, int N, int rpb) {
    const int c8n = N >> 3;
    const int c8 = threadIdx.x % c8n, sub = threadIdx.x / c8n, nsub = 256 / c8n;
    const long long m0 = (long long)blockIdx.x * rpb, m1 = m0 + rpb < M ? m0 + rpb : M;
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (sub < nsub)
        for (long long m = m0 + sub; m < m1; m += nsub) {
            float v[8];
            load8(a + m * N + c8 * 8, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) cs[e] += v[e];
        }
#pragma unroll
    for (int e = 0; e < 8; ++e) atomicAdd(&out[c8 * 8 + e], cs[e]);
}

inline int grid_for(long long items, int per_block, int cap = 2048) {
    long long g = (items + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
}  // namespace

#define DISPATCH_CT(dt, FN, ...) do { if ((dt) == LXO_BF16) { FN<bf16_t>(__VA_ARGS__); } else { FN<float>(__VA_ARGS__); } } while (0)

template <typename CT> static void conv1_fwd_t(const uint8_t* img, const float* w, const float* b, void* out, int B, int H, int W, hipStream_t s) {
    const int Hp = (H + 1) / 2, Wp = (W + 1) / 2;
    hipLaunchKernelGGL((conv1_pool_fwd_kernel<CT>), dim3(grid_for((long long)B * Hp * ((Wp + 31) / 32), 1, 4096)), dim3(256), 0, s,
                       img, w, b, (CT*)out, B, H, W, Hp, Wp);
}
static int conv1_mfma() { return lxo_switch(SW_CONV1_MFMA); }       // LXO_CONV1_MFMA=0: the VALU kernels in bf16 mode too (A/B)
constexpr int kC1FwdCap = 4096, kC1BwdCap = 512, kPoolBwdCap = 2048;      // workgroup caps of the conv1 + pool kernels and the pool backward
int lxo_k_conv1_pool_fwd(int dt, const uint8_t* img, const float* w, const float* b, void* out, int B, int H, int W, hipStream_t s) {
    if (dt == LXO_BF16 && conv1_mfma()) {
        const int Hp = (H + 1) / 2, Wp = (W + 1) / 2;
        hipLaunchKernelGGL(conv1_pool_fwd_mfma_kernel, dim3(grid_for((long long)B * Hp * ((Wp + C1_SEG - 1) / C1_SEG), 1, kC1FwdCap)), dim3(256), 0, s,
                           img, w, b, (bf16_t*)out, B, H, W, Hp, Wp);
        return (int)hipGetLastError();
    }
    DISPATCH_CT(dt, conv1_fwd_t, img, w, b, out, B, H, W, s);
    return (int)hipGetLastError();
}
template <typename CT> static int conv1_bwd_t(const uint8_t* img, const float* w, const float* b, const void* dout, float* dw, float* db, int B, int H, int W, DetScratch det, hipStream_t s) {
    const int Hp = (H + 1) / 2, Wp = (W + 1) / 2;
    const int g = grid_for((long long)B * Hp * ((Wp + 31) / 32), 16, 512);
    float* part = nullptr;
    if (det.p) { if ((size_t)g * 640 > det.floats) return -6; part = det.p; }
    hipLaunchKernelGGL((conv1_pool_bwd_kernel<CT>), dim3(g), dim3(256), 0, s,
                       img, w, b, (const CT*)dout, dw, db, part, B, H, W, Hp, Wp);
    if (part) {          // the workgroups' partial sums, added in workgroup order
        if (int rc = lxo_k_det_reduce(part, g, 640, 576, dw, s)) return rc;
        return lxo_k_det_reduce(part + 576, g, 640, 64, db, s);
    }
    return 0;
}
int lxo_k_conv1_pool_bwd(int dt, const uint8_t* img, const float* w, const float* b, const void* dout, float* dw, float* db, int B, int H, int W, DetScratch det, hipStream_t s) {
    if (dt == LXO_BF16 && conv1_mfma()) {
        const int Hp = (H + 1) / 2, Wp = (W + 1) / 2;
        const int g = grid_for((long long)B * Hp * ((Wp + C1_SEG - 1) / C1_SEG), 4, kC1BwdCap);
        float* part = nullptr;                  // deterministic mode: one slot [dw 576 | db 64] per workgroup, added in workgroup order
        if (det.p) { if ((size_t)g * 640 > det.floats) return -6; part = det.p; }
        hipLaunchKernelGGL(conv1_pool_bwd_mfma_kernel, dim3(g), dim3(256), 0, s, img, w, b, (const bf16_t*)dout, dw, db, part, B, H, W, Hp, Wp);
        if (part) {
            if (int rc = lxo_k_det_reduce(part, g, 640, 576, dw, s)) return rc;
            return lxo_k_det_reduce(part + 576, g, 640, 64, db, s);
        }
        return (int)hipGetLastError();
    }
    const int rc = dt == LXO_BF16 ? conv1_bwd_t<bf16_t>(img, w, b, dout, dw, db, B, H, W, det, s) : conv1_bwd_t<float>(img, w, b, dout, dw, db, B, H, W, det, s);
    if (rc) return rc;
    return (int)hipGetLastError();
}
template <typename CT> static void pool_fwd_t(const void* in, void* out, int B, int H, int W, int C, int ph, int pw, hipStream_t s) {
    const int Ho = (H + ph - 1) / ph, Wo = (W + pw - 1) / pw;
    hipLaunchKernelGGL((maxpool_fwd_kernel<CT>), dim3(grid_for((long long)B * Ho * Wo * (C / 8), 256, 8192)), dim3(256), 0, s,
                       (const CT*)in, (CT*)out, B, H, W, C, ph, pw, Ho, Wo);
}
int lxo_k_maxpool_fwd(int dt, const void* in, void* out, int B, int H, int W, int C, int ph, int pw, hipStream_t s) {
    if (C % 8 || C > 512 || 256 % (C / 8)) return -2;
    DISPATCH_CT(dt, pool_fwd_t, in, out, B, H, W, C, ph, pw, s);
    return (int)hipGetLastError();
}
template <typename CT> static void pool_bwd_t(const void* y, const void* dp, void* dy, float* db, int B, int H, int W, int C, int ph, int pw, hipStream_t s) {
    const int Ho = (H + ph - 1) / ph, Wo = (W + pw - 1) / pw;
    const int ppb = 256 / (C / 8);
    hipLaunchKernelGGL((maxpool_relu_bwd_kernel<CT>), dim3(grid_for((long long)B * Ho * Wo, ppb * 8, 2048)), dim3(256), 0, s,
                       (const CT*)y, (const CT*)dp, (CT*)dy, db, B, H, W, C, ph, pw, Ho, Wo);
}
int lxo_k_maxpool_mask_bwd(const unsigned char* mask, const void* dp, void* dy, float* db, int B, int H, int W, int C, int ph, int pw, DetScratch det, hipStream_t s) {
    if (C % 8 || C > 512 || 256 % (C / 8)) return -2;
    const int Ho = (H + ph - 1) / ph, Wo = (W + pw - 1) / pw;
    const int ppb = 256 / (C / 8);
    // Workgroup cap (kPoolBwdCap): ALONE on the GPU 512 workgroups (two per CU, 8 rounds of four pixels per thread) run the three pools of the benchmark
    // shape in 61 / 48 / 47 us where 2048 take 82 / 72 / 72 (fewer, longer streams keep more of the DRAM traffic inside open pages; 384 / 768: 5-10 % behind 512) --
    // but inside the training step they run beside the weight-gradient kernel of the second stream, and there 2048 is the faster step: 7.418 / 7.422 ms against
    // 7.433 / 7.439 with 512 (same box, alternating processes).  The step is what counts: 2048.
    const dim3 grid(grid_for((long long)B * Ho * Wo, ppb * 8, kPoolBwdCap));
    float* db_part = nullptr;                 // deterministic mode: one slot [C] per workgroup
    if (det.p && db) { if ((size_t)grid.x * C > det.floats) return -6; db_part = det.p; }
#define MB_ARGS mask, (const bf16_t*)dp, (bf16_t*)dy, db, db_part, B, H, W, C, Ho, Wo
    if (ph == 2 && pw == 2) hipLaunchKernelGGL((maxpool_mask_bwd_kernel<2, 2>), grid, dim3(256), 0, s, MB_ARGS);
    else if (ph == 2 && pw == 1) hipLaunchKernelGGL((maxpool_mask_bwd_kernel<2, 1>), grid, dim3(256), 0, s, MB_ARGS);
    else if (ph == 1 && pw == 2) hipLaunchKernelGGL((maxpool_mask_bwd_kernel<1, 2>), grid, dim3(256), 0, s, MB_ARGS);
    else return -2;
#undef MB_ARGS
    if (db_part) return lxo_k_det_reduce(db_part, (int)grid.x, C, C, db, s);
    return (int)hipGetLastError();
}
int lxo_k_maxpool_relu_bwd(int dt, const void* y, const void* dp, void* dy, float* db, int B, int H, int W, int C, int ph, int pw, hipStream_t s) {
    if (C % 8 || C > 512 || 256 % (C / 8)) return -2;
    DISPATCH_CT(dt, pool_bwd_t, y, dp, dy, db, B, H, W, C, ph, pw, s);
    return (int)hipGetLastError();
}
template <typename CT> static void mask_convert_t(const float* d, const void* ref, void* out, float* db, long long rows, int C, hipStream_t s) {
    const int rpb = 256 / (C / 8);
    hipLaunchKernelGGL((mask_convert_kernel<CT>), dim3(grid_for(rows, rpb * 8, 2048)), dim3(256), 0, s,
                       d, (const CT*)ref, (CT*)out, db, rows, C);
}
int lxo_k_mask_convert(int dt, const float* d, const void* ref, void* out, float* db, long long rows, int C, hipStream_t s) {
    if (C % 8 || C > 512 || 256 % (C / 8)) return -2;
    DISPATCH_CT(dt, mask_convert_t, d, ref, out, db, rows, C, s);
    return (int)hipGetLastError();
}
int lxo_k_timing_signal(float* pos, int Hp, int Wp, int C, hipStream_t s) {
    hipLaunchKernelGGL(timing_signal_kernel, dim3(grid_for((long long)Hp * Wp * C, 256, 1024)), dim3(256), 0, s, pos, Hp, Wp, C);
    return (int)hipGetLastError();
}
template <typename CT> static void pack_tr_t(const float* src, void* dst, int K, int N, int lds, int ldd, int coff, int Kpad, hipStream_t s) {
    hipLaunchKernelGGL((pack_transpose_kernel<CT>), dim3(cdiv(Kpad, 32), cdiv(N, 32)), dim3(256), 0, s, src, (CT*)dst, K, N, lds, ldd, coff, Kpad);
}
int lxo_k_pack_transpose(int dt, const float* src, void* dst, int K, int N, int lds, int ldd, int coff, int Kpad, hipStream_t s) {
    DISPATCH_CT(dt, pack_tr_t, src, dst, K, N, lds, ldd, coff, Kpad, s);
    return (int)hipGetLastError();
}
template <typename CT> static void pack_cp_t(const float* src, void* dst, int R, int Ccols, int lds, int ldd, int Cpad, hipStream_t s) {
    hipLaunchKernelGGL((pack_copy_kernel<CT>), dim3(grid_for((long long)R * Cpad, 256, 2048)), dim3(256), 0, s, src, (CT*)dst, R, Ccols, lds, ldd, Cpad);
}
int lxo_k_pack_copy(int dt, const float* src, void* dst, int R, int Ccols, int lds, int ldd, int Cpad, hipStream_t s) {
    DISPATCH_CT(dt, pack_cp_t, src, dst, R, Ccols, lds, ldd, Cpad, s);
    return (int)hipGetLastError();
}
template <typename CT> static void pack_dg_t(const float* w, void* dst, int Cin, int Cout, hipStream_t s) {
    hipLaunchKernelGGL((pack_conv_dgrad_kernel<CT>), dim3(grid_for((long long)Cin * 9 * Cout, 256, 2048)), dim3(256), 0, s, w, (CT*)dst, Cin, Cout);
}
int lxo_k_pack_conv_dgrad(int dt, const float* w, void* dst, int Cin, int Cout, hipStream_t s) {
    DISPATCH_CT(dt, pack_dg_t, w, dst, Cin, Cout, s);
    return (int)hipGetLastError();
}

int lxo_k_pack_batch(int dt, const PackTable& tab, int total_blocks, const float* prm, void* wpk, hipStream_t s) {
    if (tab.n <= 0) return 0;
    if (dt == LXO_BF16) hipLaunchKernelGGL((pack_batch_kernel<bf16_t>), dim3(total_blocks), dim3(256), 0, s, tab, prm, (char*)wpk);
    else hipLaunchKernelGGL((pack_batch_kernel<float>), dim3(total_blocks), dim3(256), 0, s, tab, prm, (char*)wpk);
    return (int)hipGetLastError();
}

template <typename CT> static void im2col_s2_t(const void* in, void* cols, int B, int H, int W, int Ho, int Wo, int C, hipStream_t s) {
    hipLaunchKernelGGL((im2col_s2_kernel<CT>), dim3(grid_for((long long)B * Ho * Wo * C, 256 * 4, 8192)), dim3(256), 0, s,
                       (const CT*)in, (CT*)cols, B, H, W, Ho, Wo, C);
}
int lxo_k_im2col_s2(int dt, const void* in, void* cols, int B, int H, int W, int Ho, int Wo, int C, hipStream_t s) {
    if (C % 8) return -2;
    DISPATCH_CT(dt, im2col_s2_t, in, cols, B, H, W, Ho, Wo, C, s);
    return (int)hipGetLastError();
}
template <typename CT> static void col2im_s2_t(const void* dcols, const void* yref, void* dy, float* db, int B, int H, int W, int Ho, int Wo, int C, hipStream_t s) {
    const int ppt = 32;
    const long long threads = (((long long)B * H * W + ppt - 1) / ppt) * (C / 8);
    hipLaunchKernelGGL((col2im_s2_relu_kernel<CT>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s,
                       (const CT*)dcols, (const CT*)yref, (CT*)dy, db, B, H, W, Ho, Wo, C, ppt);
}
int lxo_k_col2im_s2_relu(int dt, const void* dcols, const void* yref, void* dy, float* db, int B, int H, int W, int Ho, int Wo, int C, hipStream_t s) {
    if (C % 8) return -2;
    DISPATCH_CT(dt, col2im_s2_t, dcols, yref, dy, db, B, H, W, Ho, Wo, C, s);
    return (int)hipGetLastError();
}
template <typename CT> static void colsum_ct_t(const void* a, float* out, long long M, int N, hipStream_t s) {
    const int rpb = 256;
    hipLaunchKernelGGL((colsum_ct_kernel<CT>), dim3((unsigned)((M + rpb - 1) / rpb)), dim3(256), 0, s, (const CT*)a, out, M, N, rpb);
}
int lxo_k_colsum_ct(int dt, const void* a, float* out, long long M, int N, hipStream_t s) {
    if (N % 8 || N > 2048 || 256 % (N / 8)) return -2;
    DISPATCH_CT(dt, colsum_ct_t, a, out, M, N, s);
    return (int)hipGetLastError();
}
