// Persistent, XCD-local decoder chain: the T teacher-forced steps of AttentionCell.step (model/components/attention_cell.py:58-89:
// LSTM cell -> dropout -> attention context (attention_mechanism.py:46-94) -> o projection) in ONE launch.
//
// Why: the launch-per-step chain (rstep.hip + the attention pair) is five dependent launches per step, each paying the 1.5 us kernel
// boundary plus a fetch of its operands into an empty CU: 39.6 us per step for ~14 us of streaming.  The samples of a
// batch are independent through the recurrence, workgroup b runs on XCD b % 8, and an XCD's L2 is the point of coherence for its own
// 32 CUs.  So the batch is cut into 8 chains of NB = B / 8 samples, chain x lives on XCD x, and the workgroups of a chain hand their
// results over THROUGH THAT L2: plain stores (the L1 is write-through), `s_waitcnt vmcnt(0)`, one flag word per workgroup in a
// 128-byte line, consumers poll the line and then read with sc1 loads (L1 bypassed).  No agent-scope fence, no atomic, nothing crosses
// the die.  tools/xcd_barrier_probe.hip (profiles/r04_xcd_barrier_probe.txt): 0.44 us per barrier idle, lost in the noise under a
// 10 MB-per-XCD stream, zero stale reads -- against 1.5 us for a kernel boundary and 4.1 us for a whole-chip barrier.
//
// One workgroup per CU (256 x 512 threads), identity = (XCD id read from the hardware, rank = ticket on the XCD's counter).
// The recurrent weights never move: workgroup `rank` keeps ITS column slice of K_LSTM_RT (16 units x 4 gates x 1024 k = 128 KB), of
// the att_h projection (8 columns x 512 k) and of the o projection (16 columns x 1024 k) in REGISTERS for the whole launch -- each of
// the 8 waves holds the MFMA B-fragments of its eighth of every contraction (88 VGPRs per lane).  Per step, four phases:
//   P1  z = zx_t + [o | h]_{t-1} K^T  -> gates, c, h, h~         every workgroup: its 16 units, all NB rows      (attention_cell.py:70-72)
//   P2  att_h = h~ W                                              every workgroup: its 8 columns                  (attention_mechanism.py:79)
//   P3  scores / online softmax / context of one (sample, chunk)  workgroup = (rank / nq, rank % nq), nq = 32 / NB (attention_mechanism.py:80-94)
//   P4  merge the chunks, alpha, ctx; o = dropout(tanh([h~ | ctx] o_W))   every workgroup: its 16 columns          (attention_cell.py:82-83)
// with an XCD barrier after each.  A workgroup whose barrier does not complete within 200 ms (a chain that lost a member: fewer than
// 32 workgroups of the grid landed on its XCD) flags an error word and stops waiting; the host checks the word after the first use
// of this path and falls back to the launch-per-step chain (engine.py).
// The backward chain (xdec_bwd_kernel, further down) runs the same steps in reverse; there a (step, sample) pair behind the sample's formula end
// is recognised by its all-zero d_ctx row and streams nothing (37 % of the pairs at the benchmark's lengths).  The forward chain is told the
// lengths where the caller has them (XDecFwd.lengths, lxo_decoder_train_fwd_live): a pair behind its row's end streams nothing in P3 either, its
// context and alpha row are exact zeros and the rest of its record is what the step makes of that zero context.  Without lengths
// (lxo_decoder_train_fwd) its record is kept -- and tested -- at padded positions too.
#include "xdec.h"
#include "drop.h"
#include "api_util.h"
#include "switches.h"

#ifdef LXO_HIPSIM
// tests/hipsim interprets one workgroup after the other: a kernel whose workgroups wait for each other cannot run there
int lxo_launch_xdec_fwd(const XDecFwd&, int, int, int, int, hipStream_t) { return -2; }
int lxo_launch_xdec_bwd(const XDecBwd&, int, int, int, int, hipStream_t) { return -2; }
int lxo_launch_xdec_dec(const XDecDec&, int, int, int, int, hipStream_t) { return -2; }
extern "C" int lxo_xdec_debug(unsigned long long*) { return 0; }
extern "C" int lxo_xdec_debug_bwd(unsigned long long*) { return 0; }
#else

HIP_DYNAMIC_SHARED(char, xdec_dyn_lds)

namespace {
constexpr int XU = 512, XO = 512, XC = 512, XE = 256;           // the shipped attn_cell_config (configs/model.json); other sizes take the launch chain
constexpr int XXH = XO + XU, XHC = XU + XC;
constexpr int OFF_H = XO, OFF_HT = XO + XU, OFF_CTX = XO + 2 * XU;
constexpr int XW = 8;                                            // waves per workgroup
// which hand-overs of the forward chain are polled from {value, tag} words instead of meeting at an XCD barrier: 1 = h~ (P1 -> P2),
// 2 = att_h (P2 -> P3), 8 = o (P4 -> the next step's P1), 4 (round 6) = the chunk partials (P3 -> P4; chains of four and eight samples).  A compile-time choice (a run-time one costs registers the chain does not have);
// `make EXTRA=-DLXO_XDEC_LLMASK=0` builds the all-barriers variant for A/B runs (LXO_LIB_PATH selects the library).
#ifndef LXO_XDEC_LLMASK
#define LXO_XDEC_LLMASK 15
#endif
constexpr int kLL = LXO_XDEC_LLMASK;
// the same for the backward chain: 1 = g_{t-1} (Q4 -> the next step's Q1), 2 = d_ctx (Q1 -> Q2), 4 (round 6) = the d_att_h chunk partials (Q2 -> Q3)
#ifndef LXO_XDEC_LLMASK_B
#define LXO_XDEC_LLMASK_B 7
#endif
constexpr int kLLB = LXO_XDEC_LLMASK_B;

// Where the forward chain requests the first two row blocks of the NEXT step's attention stream (registers xiA / xiB):
//   0  at the end of this step's chunk (round 4): they land before the XCD barrier behind P3 -- `vmcnt` counts in order, so the barrier's
//      s_waitcnt vmcnt(0) (it must cover the partial stores) also waits for them: that IS the ~2 us wait behind P3
//   1  in the NEXT step's P1, behind the workgroup barrier that follows the partial tiles (waves 2..7: they have no epilogue work) / behind
//      the epilogue's stores (waves 0, 1): the requests fly during the P1 epilogue, the h~ hand-over and P2, whose own loads are younger
//   2  at the end of P2 (behind the att_h stores): they fly during the att_h hand-over only
//   3  in P4 behind the merge of the chunk partials (its loads are the last ones P4 waits for): they fly during the o projection, P1 and P2
#ifndef LXO_XDEC_PF
#define LXO_XDEC_PF 0
#endif
constexpr int kPF = LXO_XDEC_PF;
// the same for the backward chain: 0 at the end of the chunk (Q2); 1 in Q3 behind its first workgroup barrier (the chunk partials are in
// LDS by then); 3 in Q4 behind the workgroup barrier that follows the partial tiles.  (The forward values of the coming phases -- gates, c,
// d_o(logits), o, ctx, att_h: HBM loads, ~2 us -- stay at the end of Q2 in every variant: they are consumed within the step, so they cannot
// be requested a step ahead without a second register set, and in front of the stream they measured slower in round 4.)
#ifndef LXO_XDEC_PFB
#define LXO_XDEC_PFB 0
#endif
constexpr int kPFB = LXO_XDEC_PFB;

constexpr int PST = XC + 4;                                      // floats per chunk partial: [context 512 | max | sum | pad] (16-byte rows)
// kLL & 4: the chunk partials (P3 -> P4) as polled hand-over words too: per (sample, chunk) PLW 8-byte words -- word j < 256 = channels 2j, 2j + 1 of the
// unnormalised context as a pack28 pair (below: two 28-bit floats + an 8-bit step tag, so that a 16-byte request still carries four channels),
// words 256 / 257 = {the chunk's max, step tag} / {its sum, step tag} (f32 bits).  They live in the same ws region as the plain
// partials ("att_part"); the launcher zeroes them (a tag of an earlier launch must not pass).  No XCD barrier is left in a forward step then: every
// buffer a workgroup rewrites in step t + 1 was last read in a phase that ALL workgroups have left before any of them can get there (the data
// dependence o_t -> h~_{t+1} -> att_h_{t+1} runs through every workgroup of the chain).
constexpr int PLW = 264;                                        // = XC / 2 + 8: ws region "att_part" is sized for it (plan.hip)
static_assert(PLW * 2 <= XC + 16, "plan.hip sizes att_part with C + 16 floats per partial");
constexpr int SCMAX = 2432;                                      // rows of one attention chunk (raw scores stay in LDS until P4; static LDS is 64 KB, 58.4 KB used).  2432: the largest bucket of the reference (800 x 800 -> 9604 regions, configs/data.json:28) at B = 64 is 4 chunks of 2401 rows

typedef __attribute__((ext_vector_type(4))) float v4f;
LXO_DEV v4f mfma16(u32x4 a, u32x4 b, v4f c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
// the same v_exp_f32 / v_rcp_f32 forms as the bf16 step kernels (rstep.hip)
LXO_DEV float tanh_x(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(x * 2.8853900817779268f) + 1.f); }
LXO_DEV float sigm_x(float x) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f)); }

// Loads of data ANOTHER workgroup of the chain wrote in the previous phase: buffer loads with sc1 = served by the XCD's L2, never by
// this CU's L1 (which no other CU's store refreshes).  The compiler counts them like any other load.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
LXO_DEV rsrc_t make_rsrc(const void* base, unsigned bytes) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000); }
LXO_DEV u32x4 l2_load16(rsrc_t r, unsigned byte_off) { return __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 16); }
LXO_DEV float l2_load4(rsrc_t r, unsigned byte_off) { return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)byte_off, 0, 16)); }

// Barrier of the 32 workgroups of one XCD.  flags = the XCD's 128-byte flag line; ph = phase number (strictly increasing).
// Every thread first waits for ITS stores to be acknowledged by the L2; lane-wise poll of the whole line by wave 0.
LXO_DEV void xbar(unsigned* flags, int rank, unsigned ph, unsigned* err, int* s_dead) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < 64) {
        if (tid == 0) *reinterpret_cast<volatile unsigned*>(flags + rank) = ph;
        if (!*s_dead) {
            const unsigned long long t0 = wall_clock64();
            for (;;) {
                const unsigned v = __hip_atomic_load(flags + (tid & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__ballot(v < ph) == 0ull) break;
                if (wall_clock64() - t0 > 20000000ull) {         // 200 ms of a 100 MHz clock: the chain is broken
                    if (tid == 0) { *s_dead = 1; *reinterpret_cast<volatile unsigned*>(err) = 1u; }
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
    }
    __syncthreads();
}

// Wave-wide sums WITHOUT the LDS crossbar: `__shfl_xor` compiles to ds_bpermute_b32 (an LDS-pipe round trip per butterfly step: 197 ns per
// dependent 64-lane reduction, tools/dpp_probe.hip); the four steps inside a row of 16 lanes are v_add_f32_dpp (quad_perm, row_half_mirror,
// row_mirror: the partner's value arrives as an operand modifier), the two across rows v_permlane16_swap / v_permlane32_swap (gfx950):
// 69 ns, every lane ends with the same bits.  STEP-wise so that the rows of a block can be interleaved.
template <int CTRL> LXO_DEV float dpp_add(float v) { return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true)); }
template <int STEP> LXO_DEV float xsum_step(float v) {
    if constexpr (STEP == 0) return dpp_add<0xB1>(v);            // quad_perm [1,0,3,2]
    else if constexpr (STEP == 1) return dpp_add<0x4E>(v);       // quad_perm [2,3,0,1]
    else if constexpr (STEP == 2) return dpp_add<0x141>(v);      // row_half_mirror
    else if constexpr (STEP == 3) return dpp_add<0x140>(v);      // row_mirror
    else if constexpr (STEP == 4) { const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false); return __uint_as_float(r[0]) + __uint_as_float(r[1]); }
    else { const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false); return __uint_as_float(r[0]) + __uint_as_float(r[1]); }
}
// (Measured: decoder backward 2.80 -> 2.72 ms; the forward chain, whose stream phase has the crossbar to spare, 2.42 either way -- also with
// only the two cross-row steps left on ds_bpermute.)
template <int N> LXO_DEV void xsum_rows(float (&v)[N]) {
#pragma unroll
    for (int u = 0; u < N; ++u) v[u] = xsum_step<0>(v[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) v[u] = xsum_step<1>(v[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) v[u] = xsum_step<2>(v[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) v[u] = xsum_step<3>(v[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) v[u] = xsum_step<4>(v[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) v[u] = xsum_step<5>(v[u]);
}

// Hand-over WITHOUT a barrier: the producer stores 8-byte words {value, tag} (one store, so the pair arrives together), the consumer
// polls the words it needs until every tag is the current step's.  Saves the producer's wait for its store acknowledgements, the flag
// round trip and the consumer's separate load behind the barrier (~1 us of the 1.0 + 0.5 a barrier-and-load costs inside the chain).
// ll_wait: all lanes of the wave load `N` 16-byte pieces (two words each) and repeat until all their tags match; 200 ms timeout as in xbar.
template <int N>
LXO_DEV bool ll_wait(u32x4 (&w)[N], rsrc_t r, const unsigned (&off)[N], unsigned tag, unsigned* err, int* s_dead) {
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        bool ok = true;
#pragma unroll
        for (int j = 0; j < N; ++j) { w[j] = l2_load16(r, off[j]); }
#pragma unroll
        for (int j = 0; j < N; ++j) ok = ok && w[j][1] == tag && w[j][3] == tag;
        const bool all = __ballot(!ok) == 0ull;
        const bool gave_up = !all && (*s_dead || wall_clock64() - t0 > 20000000ull);
        if (gave_up && (threadIdx.x & 63) == 0) { *s_dead = 1; *reinterpret_cast<volatile unsigned*>(err) = 3u; }
        if (all || gave_up) return all;                          // ONE way out of the loop: with two, every caller gets an if / else over them with a copy of w in each arm
    }
}

// Hand-over words for the chunk partials (round 6): TWO values of 28 bits each -- an f32 cut to 19 mantissa bits (relative error 2^-20) -- and an
// 8-bit step tag in one 8-byte word, so that a 16-byte request still carries four values (the merges that consume them are the kernels' register
// peaks and cannot afford twice the requests) without the 2^-9 of a bf16 pair: the partial contexts of a sample feed s = <ctx, d_ctx> in BPTT and
// the d_att_h partials cancel (sum_r d_e_r = 0), so bf16 pairs cost dW_att_h a factor of 5 in noise (cosine against the oracle 0.99993 at B = 64
// where this form gives 0.99996+).  Tags are 1 .. 255 (the words are zeroed per launch; the word of step t - 1 is what a step-t poll may still see).
LXO_DEV u32x2 pack28(float x0, float x1, unsigned tag8) {
    const unsigned a = (__float_as_uint(x0) + 8u) >> 4, b = (__float_as_uint(x1) + 8u) >> 4;      // round to nearest (a carry into the exponent is the right answer)
    return u32x2{(a & 0x0FFFFFFFu) | (b << 28), ((b >> 4) & 0x00FFFFFFu) | (tag8 << 24)};
}
LXO_DEV float unpack28_lo(unsigned lo) { return __uint_as_float(lo << 4); }
LXO_DEV float unpack28_hi(unsigned lo, unsigned hi) { return __uint_as_float(((lo >> 28) | (hi << 4)) << 4); }
LXO_DEV unsigned tag8_of(int t) { return (unsigned)(t % 255) + 1u; }
// ll_wait for such words: the tag is the top byte of every odd dword
template <int N>
LXO_DEV bool ll_wait8(u32x4 (&w)[N], rsrc_t r, const unsigned (&off)[N], unsigned tag8, unsigned* err, int* s_dead) {
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        bool ok = true;
#pragma unroll
        for (int j = 0; j < N; ++j) { w[j] = l2_load16(r, off[j]); }
#pragma unroll
        for (int j = 0; j < N; ++j) ok = ok && (w[j][1] >> 24) == tag8 && (w[j][3] >> 24) == tag8;
        const bool all = __ballot(!ok) == 0ull;
        const bool gave_up = !all && (*s_dead || wall_clock64() - t0 > 20000000ull);
        if (gave_up && (threadIdx.x & 63) == 0) { *s_dead = 1; *reinterpret_cast<volatile unsigned*>(err) = 3u; }
        if (all || gave_up) return all;                          // ONE way out of the loop: with two, every caller gets an if / else over them with a copy of w in each arm
    }
}

// One block of ATT_U rows per wave of the attention chunk: scores from the att_img rows (raw bf16 words in xa), online-softmax update of
// (m, l, acc) with the img rows (xi).  Rows at or beyond `an` were loaded clamped and contribute nothing.
// EXPD: xa holds E_x = e^{2x}, ah holds E_a = e^{2 att_h}, bt holds -2 beta: with r = 1 / (1 + E_x E_a), tanh = 1 - 2r and the score is
// sum_k beta_k - 2 sum_k beta_k r_k; the constant is the same for every region of the step, so the softmax does not see it and it is dropped.
template <int ATT_U, bool EXPD>
LXO_DEV void att_block(const u32x4 (&xi)[ATT_U], const u32x2 (&xa)[ATT_U], int base, int an, const float (&ah)[4], const float (&bt)[4],
                       float& m, float& l, float (&acc)[8], float* sc, int lane) {
    float pt[ATT_U];
#pragma unroll
    for (int u = 0; u < ATT_U; ++u) {
        pt[u] = 0.f;
        if (base + XW * u >= an) continue;                       // wave-uniform: a clamped row (the chunk's last block) costs its loads, not its arithmetic
        const float x0 = __uint_as_float(xa[u][0] << 16), x1 = __uint_as_float(xa[u][0] & 0xffff0000u);
        const float x2 = __uint_as_float(xa[u][1] << 16), x3 = __uint_as_float(xa[u][1] & 0xffff0000u);
        float a;
        if constexpr (EXPD) {
            a = __builtin_amdgcn_rcpf(fmaf(x0, ah[0], 1.f)) * bt[0];
            a = fmaf(__builtin_amdgcn_rcpf(fmaf(x1, ah[1], 1.f)), bt[1], a);
            a = fmaf(__builtin_amdgcn_rcpf(fmaf(x2, ah[2], 1.f)), bt[2], a);
            a = fmaf(__builtin_amdgcn_rcpf(fmaf(x3, ah[3], 1.f)), bt[3], a);
        } else {
            a = tanh_x(x0 + ah[0]) * bt[0];
            a = fmaf(tanh_x(x1 + ah[1]), bt[1], a);
            a = fmaf(tanh_x(x2 + ah[2]), bt[2], a);
            a = fmaf(tanh_x(x3 + ah[3]), bt[3], a);
        }
        pt[u] = a;
    }
    xsum_rows<ATT_U>(pt);
    float mn = m;
#pragma unroll
    for (int u = 0; u < ATT_U; ++u) if (base + XW * u < an) mn = fmaxf(mn, pt[u]);
    const float scl = __expf(m - mn);
    l *= scl;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= scl;
    m = mn;
#pragma unroll
    for (int u = 0; u < ATT_U; ++u) {
        const int r = base + XW * u;
        if (r >= an) continue;
        const bool ok = true;
        const float pw = __expf(pt[u] - m);
        l += pw;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[2 * e] = fmaf(pw, __uint_as_float(xi[u][e] << 16), acc[2 * e]);
            acc[2 * e + 1] = fmaf(pw, __uint_as_float(xi[u][e] & 0xffff0000u), acc[2 * e + 1]);
        }
        if (ok && sc && lane == 0) sc[r] = pt[u];                   // (sc == null: the decode chain keeps no raw scores)
    }
}
// the loads of one block: UNCONDITIONAL (a row index beyond the chunk is clamped to its last row), so that the compiler counts them
// and a block can stay in flight under the computation of the previous one.  Buffer loads: the row is wave-uniform, so it travels in the
// SCALAR offset and the per-lane offset is one loop-invariant register -- no address arithmetic on the vector ALU, no 64-bit address pairs.
template <int ATT_U>
LXO_DEV void att_load(u32x4 (&xi)[ATT_U], u32x2 (&xa)[ATT_U], rsrc_t rim, rsrc_t rai, int base, int an, int lane) {
#pragma unroll
    for (int u = 0; u < ATT_U; ++u) {
        const int r = max(min(base + XW * u, an - 1), 0);
        xi[u] = __builtin_amdgcn_raw_buffer_load_b128(rim, lane * 16, r * (XC * 2), 0);
        xa[u] = __builtin_amdgcn_raw_buffer_load_b64(rai, lane * 8, r * (XE * 2), 0);
    }
}

// ------------------------------------------------------------------------------------------------ what the chains share ----
// Identity of a chain workgroup: the XCD it runs on (read from the hardware), its rank there (a ticket on the XCD's counter), the first sample
// of its chain and what a thread needs to find its place in an MFMA fragment.  All three kernels take theirs from here.
struct XChain {
    int tid, lane, wave;                                         // wave: known uniform (row arithmetic on the scalar ALU)
    int r16, g4;                                                 // the lane in an MFMA fragment: (column, k group)
    unsigned xcc;
    int rank, b0;                                                // first sample of this chain
    int arow;                                                    // A-fragment row of this lane (rows >= NB repeat the last one; their products are dropped)
    unsigned* xsync; unsigned* err; int* s_dead;                 // the XCD's flag line, the launch's error word, the workgroup's "chain is broken" word
};
LXO_DEV XChain xchain_ticket(unsigned* sync, int nb, int* s_rank, int* s_dead) {
    XChain c;
    c.tid = threadIdx.x; c.lane = c.tid & 63; c.wave = __builtin_amdgcn_readfirstlane(c.tid >> 6);
    c.r16 = c.lane & 15; c.g4 = c.lane >> 4;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(c.xcc));
    c.xcc &= 7u;
    c.xsync = sync + c.xcc * 64; c.err = sync + 8 * 64; c.s_dead = s_dead;
    c.rank = 0; c.b0 = (int)c.xcc * nb; c.arow = min(c.r16, nb - 1);
    if (c.tid == 0) { *s_dead = 0; *s_rank = (int)atomicAdd(c.xsync + 32, 1u); }
    return c;
}
// behind the workgroup barrier that follows the ticket.  false: more than 32 workgroups on this XCD, not a chain (error word 2)
LXO_DEV bool xchain_rank(XChain& c, const int* s_rank) {
    c.rank = *s_rank;
    if (c.rank < 32) return true;
    if (c.tid == 0) *reinterpret_cast<volatile unsigned*>(c.err) = 2u;
    return false;
}

// Attention role of a workgroup: (sample of the chain, chunk) = (rank / NQ, rank % NQ) and the two streams of that chunk.
// The chunk is walked in blocks of XW * ATT_U rows, two blocks per loop trip (buffers A and B): block i+1 is in flight while block i is
// computed, and the FIRST block of the next step is requested before this step's last block is computed -- it lands during P4 / P1 / P2,
// so P3 starts on data that is already in registers.  An odd block count ends on an A half (no padded block: its clamped loads cost 1 / 8 of
// the benchmark chunk's requests).  Blocks are walked in alternating directions from step to step (what this step read last is what the next
// one reads first: L2 reuse).
template <int ATT_U>
struct XRole {
    int as, aq, ab;                                              // sample of the chain, chunk, sample of the batch
    int ar0, an;                                                 // the chunk's first row and row count (may be <= 0 for a trailing chunk)
    int nblk, anq;                                               // blocks; rows the streams' descriptors cover (an empty trailing chunk still issues (masked) loads: row 0 of the first sample)
    rsrc_t imq, aiq;                                             // the chunk's img rows and att_img (or e^{2 att_img}) rows
    int wave;
    // first row of this wave in block i of the walk (rv: the walk runs backwards)
    LXO_DEV int XBASE(int i, int rv) const { return wave + XW * ATT_U * (rv ? nblk - 1 - i : i); }
};
template <int NB, int ATT_U>
LXO_DEV XRole<ATT_U> xdec_role(const XChain& c, int R, const bf16_t* img, const bf16_t* ai) {
    constexpr int NQ = 32 / NB;                                  // attention chunks per sample = workgroups per sample
    XRole<ATT_U> ro;
    ro.as = c.rank / NQ; ro.aq = c.rank - ro.as * NQ;
    ro.ab = c.b0 + ro.as;
    const int rows_per = (R + NQ - 1) / NQ;
    ro.ar0 = ro.aq * rows_per;
    ro.an = min(R, ro.ar0 + rows_per) - ro.ar0;
    ro.nblk = ro.an > 0 ? (ro.an + XW * ATT_U - 1) / (XW * ATT_U) : 0;
    ro.anq = ro.an > 0 ? ro.an : 1;
    ro.imq = make_rsrc(ro.an > 0 ? img + ((long long)ro.ab * R + ro.ar0) * XC : img, (unsigned)ro.anq * XC * 2u);
    ro.aiq = make_rsrc(ro.an > 0 ? ai + ((long long)ro.ab * R + ro.ar0) * XE : ai, (unsigned)ro.anq * XE * 2u);
    ro.wave = c.wave;
    return ro;
}

// P1's contraction index [o (512) | h (512)]: k-steps 0, 1 of a wave lie in o (polled hand-over words), 2, 3 in h (plain loads)
LXO_DEV constexpr int P1K(int wave, int ks) { return ks < 2 ? wave * 64 + ks * 32 : XO + wave * 64 + (ks - 2) * 32; }

// ---- resident weights of the forward and decode chains: this wave's eighth of every contraction, as MFMA B fragments (lane = (column r16, k group g4)) ----
// K_LSTM_RT: gate i in registers, gates j, f, o in LDS (96 KB, fragment-shaped: [wave][gate][k-step][lane] x 16 B, read back by the
// lane that wrote it) -- 88 resident VGPRs left no room for the attention stream's two row blocks in flight
template <bool EXPD, class P>
LXO_DEV void xdec_resident(const P& p, const XChain& c, u32x4 (&wrt0)[4], u32x4* wl, u32x4 (*wahs)[2][64], u32x4 (&wow)[4], float (&bt)[4]) {
    const int u0 = c.rank * 16, e0 = c.rank * 8, o0 = c.rank * 16;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const u32x4 w = *reinterpret_cast<const u32x4*>(p.Wrt + (long long)(q * XU + u0 + c.r16) * p.ldrt + P1K(c.wave, ks) + c.g4 * 8);
            if (q == 0) wrt0[ks] = w; else wl[((q - 1) * 4 + ks) * 64] = w;      // wl + (gate - 1) * 4 * 64 + ks * 64
        }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(p.Wah + (long long)(e0 + (c.r16 & 7)) * p.ldah + c.wave * 64 + ks * 32 + c.g4 * 8);
        const u32x4 z = {0u, 0u, 0u, 0u};
        wahs[c.wave][ks][c.lane] = c.r16 < 8 ? w : z;            // an 8-column slice in a 16-column tile
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        wow[ks] = *reinterpret_cast<const u32x4*>(p.Wow + (long long)(o0 + c.r16) * p.ldow + c.wave * 128 + ks * 32 + c.g4 * 8);
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.beta + c.lane * 4);
    const float f = EXPD ? -2.f : 1.f;
    bt[0] = f * b4[0]; bt[1] = f * b4[1]; bt[2] = f * b4[2]; bt[3] = f * b4[3];
}

// P1's A operand: this lane's row of [o | h]_{t-1} (record slot sp).  h comes from plain loads; o, when `polled`, from the hand-over words the
// o projection of the previous step left (no barrier behind P4), tagged `tag`
template <class P>
LXO_DEV void xdec_p1_fetch(u32x4 (&a)[4], const P& p, const XChain& c, long long sp, bool polled, rsrc_t rll_o, unsigned tag) {
    const rsrc_t rp = make_rsrc(p.recb + sp * p.RECB, (unsigned)p.B * p.RECB * 2u);
#pragma unroll
    for (int ks = 2; ks < 4; ++ks) a[ks] = l2_load16(rp, (unsigned)(((c.b0 + c.arow) * p.RECB + P1K(c.wave, ks) + c.g4 * 8) * 2));
    if (polled) {
        u32x4 w[4];
        unsigned off[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) off[j] = (unsigned)(((c.b0 + c.arow) * 256 + ((P1K(c.wave, j >> 1) + c.g4 * 8) >> 1)) * 8 + (j & 1) * 16);
        ll_wait<4>(w, rll_o, off, tag, c.err, c.s_dead);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) a[ks] = u32x4{w[2 * ks][0], w[2 * ks][2], w[2 * ks + 1][0], w[2 * ks + 1][2]};
    } else {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) a[ks] = l2_load16(rp, (unsigned)(((c.b0 + c.arow) * p.RECB + P1K(c.wave, ks) + c.g4 * 8) * 2));
    }
}

// TF-1.12 LSTMCell, gate order i, j, f, o, forget_bias 1.0 (attention_cell.py:71), of one element (row erow, unit eu) of the workgroup's tile.
// g: in, the x-part of the pre-activation; out, the activated gates.  The recurrent part is the sum of the waves' partial tiles.
LXO_DEV void xdec_lstm(float (&g)[4], const float (*red)[8][64], int erow, int eu, float c_prev, float& c, float& h) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float z = g[q];
#pragma unroll
        for (int w = 0; w < XW; ++w) z += red[w][erow][q * 16 + eu];
        g[q] = (q == 1) ? tanh_x(z) : sigm_x(q == 2 ? z + 1.0f : z);
    }
    c = fmaf(g[2], c_prev, g[0] * g[1]);                         // written out: left to the compiler, WHICH product is fused changes with the code around it
    h = g[3] * tanh_x(c);
}

// P2: att_h = h~ W, this workgroup's 8 columns of all NB rows, handed to the attention workgroups as polled words (no barrier).
// POLL: h~ comes from the hand-over words P1 left, else from the record behind an XCD barrier.  ATTH: att_h is also kept (p.atth, step slot sp).
template <int NB, bool POLL, bool ATTH, class P>
LXO_DEV void xdec_p2(const P& p, const XChain& c, long long sp, long long sn, int t, rsrc_t rll_ht, unsigned* ll_ah, float (*red)[8][64], const u32x4 (*wahs)[2][64]) {
    u32x4 a[2];
    if constexpr (POLL) {
        u32x4 w[4];
        unsigned off[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) off[j] = (unsigned)(((c.b0 + c.arow) * 256 + ((c.wave * 64 + (j >> 1) * 32 + c.g4 * 8) >> 1)) * 8 + (j & 1) * 16);
        ll_wait<4>(w, rll_ht, off, (unsigned)(t + 1), c.err, c.s_dead);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) a[ks] = u32x4{w[2 * ks][0], w[2 * ks][2], w[2 * ks + 1][0], w[2 * ks + 1][2]};
    } else {
        const rsrc_t rn = make_rsrc(p.recb + sn * p.RECB, (unsigned)p.B * p.RECB * 2u);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) a[ks] = l2_load16(rn, (unsigned)(((c.b0 + c.arow) * p.RECB + OFF_HT + c.wave * 64 + ks * 32 + c.g4 * 8) * 2));
    }
    v4f acc = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) acc = mfma16(a[ks], wahs[c.wave][ks][c.lane], acc);
    if (c.g4 * 4 < NB) {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (NB >= 4 || i < NB) red[c.wave][c.g4 * 4 + i][c.r16] = acc[i];
    }
    __syncthreads();
    if (c.tid < NB * 8) {
        const int row = c.tid >> 3, e = c.tid & 7, e0 = c.rank * 8;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < XW; ++w) v += red[w][row][e];
        if constexpr (ATTH) p.atth[(sp + c.b0 + row) * XE + e0 + e] = v;
        const u32x2 wv = {__float_as_uint(v), (unsigned)(t + 1)};
        *reinterpret_cast<u32x2*>(ll_ah + ((c.b0 + row) * XE + e0 + e) * 2) = wv;      // the attention workgroups poll these words: no barrier
    }
}

// P3's att_h of this workgroup's sample, polled from P2's words (behind a barrier the tags already match: one pass).  EXPD: as E_a = e^{2 att_h}
template <bool EXPD>
LXO_DEV void xdec_att_h(float (&ah)[4], const XChain& c, int ab, rsrc_t rll_ah, unsigned tag) {
    u32x4 aw[2];
    const unsigned off[2] = {(unsigned)((ab * XE + c.lane * 4) * 8), (unsigned)((ab * XE + c.lane * 4) * 8 + 16)};
    ll_wait<2>(aw, rll_ah, off, tag, c.err, c.s_dead);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ah[j] = __uint_as_float(aw[j >> 1][(j & 1) * 2]);
        if constexpr (EXPD) ah[j] = __builtin_amdgcn_exp2f(fminf(fmaxf(ah[j] * 2.8853900817779268f, -60.f), 60.f));      // E_a
    }
}

// P3's walk over the chunk, direction rev.  Entering: block 0 in A and block 1 in B (requested at the end of the previous step's P3).  Each
// buffer is refilled right after its block is computed -- with the block two ahead, or, at the end of the chunk, with the NEXT STEP's first two
// blocks (its direction is the other one): they land during P4 / P1 / P2.  nwalk: ro.nblk, or 0 for a step that walks nothing (a dead pair
// of the forward chain: no block is computed and none is requested; what the last walk asked for stays in the buffers, unread).  A scalar
template <int ATT_U, bool EXPD>
LXO_DEV void xdec_walk(u32x4 (&xiA)[ATT_U], u32x2 (&xaA)[ATT_U], u32x4 (&xiB)[ATT_U], u32x2 (&xaB)[ATT_U], const XRole<ATT_U>& ro, int nwalk, int rev,
                       const float (&ah)[4], const float (&bt)[4], float& m, float& l, float (&acc)[8], float* sc, int lane) {
    const int nblk = ro.nblk;
    for (int it = 0; it < nwalk; it += 2) {
        att_block<ATT_U, EXPD>(xiA, xaA, ro.XBASE(it, rev), ro.an, ah, bt, m, l, acc, sc, lane);
        __builtin_amdgcn_sched_barrier(0);
        att_load<ATT_U>(xiA, xaA, ro.imq, ro.aiq, (it + 2 < nblk) ? ro.XBASE(it + 2, rev) : ro.XBASE(0, rev ^ 1), ro.anq, lane);
        __builtin_amdgcn_sched_barrier(0);
        if (it + 1 < nblk) {                                     // (an odd block count ends on an A half: B already holds the next step's block 1)
            att_block<ATT_U, EXPD>(xiB, xaB, ro.XBASE(it + 1, rev), ro.an, ah, bt, m, l, acc, sc, lane);
            __builtin_amdgcn_sched_barrier(0);
            att_load<ATT_U>(xiB, xaB, ro.imq, ro.aiq, (it + 3 < nblk) ? ro.XBASE(it + 3, rev) : ro.XBASE(1, rev ^ 1), ro.anq, lane);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// P3's end: merge the 8 waves' (max, sum, context) and publish the chunk's partial for P4 -- PP: as polled words (tags of step t), else plain
// floats in front of an XCD barrier
template <int NQ, bool PP>
LXO_DEV void xdec_p3_publish(float m, float l, const float (&acc)[8], const XChain& c, int ab, int aq, int t, float* part, float* wred, float (*redc)[XC]) {
    const int tid = c.tid, lane = c.lane, wave = c.wave, c0 = lane * 8;
    if (lane == 0) wred[wave] = m;
    __syncthreads();
    float mc = wred[0];
#pragma unroll
    for (int w = 1; w < XW; ++w) mc = fmaxf(mc, wred[w]);
    const float sw = (l > 0.f) ? __expf(m - mc) : 0.f;
    if (lane == 0) wred[XW + wave] = l * sw;
#pragma unroll
    for (int e = 0; e < 8; ++e) redc[wave][c0 + e] = acc[e] * sw;
    __syncthreads();
    if constexpr (PP) {
        unsigned* pw = reinterpret_cast<unsigned*>(part) + ((long long)ab * NQ + aq) * (PLW * 2);
        if (tid == 0) {
            float lt = 0.f;
#pragma unroll
            for (int w = 0; w < XW; ++w) lt += wred[XW + w];
            const u32x4 st4 = {__float_as_uint(mc), (unsigned)(t + 1), __float_as_uint(lt), (unsigned)(t + 1)};
            *reinterpret_cast<u32x4*>(pw + 256 * 2) = st4;
        }
        float tsum = 0.f;
#pragma unroll
        for (int w = 0; w < XW; ++w) tsum += redc[w][tid];
        const float other = __shfl_xor(tsum, 1);
        if (!(tid & 1)) *reinterpret_cast<u32x2*>(pw + (tid >> 1) * 2) = pack28(tsum, other, tag8_of(t));
    } else {
        float* pout = part + ((long long)ab * NQ + aq) * PST;
        if (tid == 0) {
            float lt = 0.f;
#pragma unroll
            for (int w = 0; w < XW; ++w) lt += wred[XW + w];
            pout[XC] = mc; pout[XC + 1] = lt;
        }
        float tsum = 0.f;
#pragma unroll
        for (int w = 0; w < XW; ++w) tsum += redc[w][tid];
        pout[tid] = tsum;
    }
}

// P4's first request: the h~ half of the o projection's A operand (waves 0..3), asked for in front of the chunk partials -- all of P4's
// requests go out up front, 16 bytes each
template <class P>
LXO_DEV void xdec_o_fetch(u32x4 (&a)[4], const P& p, const XChain& c, long long sn) {
    if (c.wave < 4) {
        const rsrc_t rn = make_rsrc(p.recb + sn * p.RECB, (unsigned)p.B * p.RECB * 2u);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) a[ks] = l2_load16(rn, (unsigned)(((c.b0 + c.arow) * p.RECB + OFF_HT + c.wave * 128 + ks * 32 + c.g4 * 8) * 2));
    }
}

// P4: merge the chunk partials of the chain's samples into ctx -- the A tile of the o projection (actx) and, for the 16 channels this
// workgroup owns, the record (slot sn).  Four groups of 128 threads split the NB samples; a thread holds 4 channels.
// SM: the samples' softmax max and 1 / sum are kept too (smax, sinv: what alpha needs), and a sample none of whose chunks reports a sum (a dead
// pair of the forward chain: every partial is zero) merges to an exact zero context instead of 0 / 0.  arrived: measurement only (null = off), stamped once the polled partials are there
template <int NB, bool PP, bool SM, class P>
LXO_DEV void xdec_p4_merge(const P& p, const XChain& c, long long sn, int t, float (*wgt)[32 / NB], float* smax, float* sinv, float (*redc)[XC],
                           bf16_t (*actx)[XC + 8], unsigned long long* arrived) {
    constexpr int NQ = 32 / NB;
    const int tid = c.tid, wave = c.wave, b0 = c.b0;
    const rsrc_t rpart = PP ? make_rsrc(reinterpret_cast<const unsigned*>(p.part) + (long long)b0 * NQ * (PLW * 2), (unsigned)(NB * NQ * PLW) * 8u)
                            : make_rsrc(p.part + (long long)b0 * NQ * PST, (unsigned)(NB * NQ * PST) * 4u);
    constexpr int SPG = NB >= 4 ? NB / 4 : 1, NG = NB / SPG;      // samples per thread group, groups that have samples
    // chains of one or two samples: the 32 / 16 chunk partials of a sample are split over the 4 / 2 thread groups (8 chunks each = two rounds of
    // four requests; one group per sample walked them in eight / four dependent rounds: P4 5.6 us of a 12.2 us step at B = 8) and the groups' sums meet in LDS
    constexpr int GPS = NB >= 4 ? 1 : 4 / NB, CPG = NQ / GPS;
    const int tg = tid >> 7, c4 = (tid & 127) * 4;
    const int gsm = tg / GPS, cb = (tg - gsm * GPS) * CPG;      // this thread group's sample (block) and first chunk
    // chunks requested at a time per sample.  Every request in flight pins four destination registers, and this merge is where the
    // kernel's register demand peaks: with 8 x 16 bytes in flight per thread the allocator kept 17 dwords of loop-invariant
    // addresses in scratch and reloaded them (behind `vmcnt(0)`) in every serial phase -- 4 in flight (2 samples x 2 chunks at
    // B = 64) costs the merge one more L2 round trip and the step 1 us less: decoder forward 2.40 -> 2.30 ms
    constexpr int QG = NB >= 4 ? 2 : 4;
    u32x4 pc[SPG][QG];
    float st_m = 0.f, st_l = 0.f;                               // wave 0: {max, sum} of (sample, chunk) = lane (lanes 32 .. 63 repeat lane 31's)
    if constexpr (PP) {
        // polled: the words of this thread's channel pair pairs ({28 bits x 2, tag} x 2 per 16 bytes) of the first chunk group, and -- wave 0 -- the
        // {max, tag, sum, tag} words of every (sample, chunk) of the chain (NB * NQ = 32 of them: lanes 32 .. 63 repeat lane 31's)
        if (wave == 0) {
            u32x4 w1[1];
            const unsigned off1[1] = {(unsigned)((min(tid, NB * NQ - 1) * PLW + 256) * 8)};
            ll_wait<1>(w1, rpart, off1, (unsigned)(t + 1), c.err, c.s_dead);
            st_m = __uint_as_float(w1[0][0]); st_l = __uint_as_float(w1[0][2]);
        }
        if (gsm < NG) {
            u32x4 wq[SPG * QG];
            unsigned offq[SPG * QG];
#pragma unroll
            for (int si = 0; si < SPG; ++si)
#pragma unroll
                for (int q = 0; q < QG; ++q) offq[si * QG + q] = (unsigned)((((gsm * SPG + si) * NQ + cb + q) * PLW + (c4 >> 1)) * 8);
            ll_wait8<SPG * QG>(wq, rpart, offq, tag8_of(t), c.err, c.s_dead);
#pragma unroll
            for (int si = 0; si < SPG; ++si)
#pragma unroll
                for (int q = 0; q < QG; ++q) pc[si][q] = wq[si * QG + q];
        }
        if (arrived && tid == 0) *arrived = wall_clock64();
    } else {
        if (gsm < NG) {
#pragma unroll
            for (int si = 0; si < SPG; ++si)
#pragma unroll
                for (int q = 0; q < QG; ++q) pc[si][q] = l2_load16(rpart, (unsigned)((((gsm * SPG + si) * NQ + cb + q) * PST + c4) * 4));
        }
        if (wave == 0) {
            const unsigned o = (unsigned)((min(tid, NB * NQ - 1) * PST + XC) * 4);
            st_m = l2_load4(rpart, o); st_l = l2_load4(rpart, o + 4);
        }
    }
    // softmax over the chunks of a sample, one lane per (sample, chunk) -- NB * NQ = 32 lanes of wave 0, log2(NQ) exchange rounds (one thread per
    // sample walked its NQ chunks three times: ~2 us of serial code per step at NQ = 32, the chains of one sample)
    if (wave == 0) {
        float mm = st_l > 0.f ? st_m : -3.0e38f;
#pragma unroll
        for (int o = NQ / 2; o > 0; o >>= 1) mm = fmaxf(mm, __shfl_xor(mm, o));
        const float w = st_l > 0.f ? __expf(st_m - mm) : 0.f;
        float ll = st_l * w;
#pragma unroll
        for (int o = NQ / 2; o > 0; o >>= 1) ll += __shfl_xor(ll, o);
        float inv = 1.0f / ll;
        if constexpr (SM) inv = ll > 0.f ? inv : 0.f;            // (a live sample's sum is >= 1: its own values are untouched)
        if (tid < NB * NQ) {
            (&wgt[0][0])[tid] = w * inv;
            if constexpr (SM) { if ((tid & (NQ - 1)) == 0) { smax[tid / NQ] = mm; sinv[tid / NQ] = inv; } }
        }
    }
    __syncthreads();
    // ctx[s][c4 .. c4+3]: A tile of the o projection; the 16 channels this workgroup owns also go to the record
    if (gsm < NG) {
#pragma unroll
        for (int si = 0; si < SPG; ++si) {
            const int sidx = gsm * SPG + si;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q0 = 0; q0 < CPG; q0 += QG) {
#pragma unroll
                for (int q = 0; q < QG; ++q) {
                    const float w = wgt[sidx][cb + q0 + q];
                    if constexpr (PP) {
                        v[0] = fmaf(unpack28_lo(pc[si][q][0]), w, v[0]); v[1] = fmaf(unpack28_hi(pc[si][q][0], pc[si][q][1]), w, v[1]);
                        v[2] = fmaf(unpack28_lo(pc[si][q][2]), w, v[2]); v[3] = fmaf(unpack28_hi(pc[si][q][2], pc[si][q][3]), w, v[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaf(__uint_as_float(pc[si][q][e]), w, v[e]);
                    }
                }
                if (q0 + QG < CPG) {                             // next group of chunks (compile-time condition: NQ, QG are constants)
                    if constexpr (PP) {
                        u32x4 wq[QG];
                        unsigned offq[QG];
#pragma unroll
                        for (int q = 0; q < QG; ++q) offq[q] = (unsigned)(((sidx * NQ + cb + q0 + QG + q) * PLW + (c4 >> 1)) * 8);
                        ll_wait8<QG>(wq, rpart, offq, tag8_of(t), c.err, c.s_dead);
#pragma unroll
                        for (int q = 0; q < QG; ++q) pc[si][q] = wq[q];
                    } else {
#pragma unroll
                        for (int q = 0; q < QG; ++q) pc[si][q] = l2_load16(rpart, (unsigned)(((sidx * NQ + cb + q0 + QG + q) * PST + c4) * 4));
                    }
                }
            }
            if constexpr (GPS > 1) {                             // the groups of a sample meet in LDS (the waves' partial-context buffer of P3 is free here)
                *reinterpret_cast<f32x4*>(&redc[tg][c4]) = f32x4{v[0], v[1], v[2], v[3]};
                __syncthreads();
                if (cb == 0) {
#pragma unroll
                    for (int g = 1; g < GPS; ++g) { const f32x4 o4 = *reinterpret_cast<const f32x4*>(&redc[tg + g][c4]); v[0] += o4[0]; v[1] += o4[1]; v[2] += o4[2]; v[3] += o4[3]; }
                }
            }
            if (GPS > 1 && cb != 0) continue;
            const u32x2 vb = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
            *reinterpret_cast<u32x2*>(&actx[sidx][c4]) = vb;
            if ((c4 >> 4) == c.rank) {
                const f32x4 vf = {v[0], v[1], v[2], v[3]};
                *reinterpret_cast<f32x4*>(p.rec + (sn + b0 + sidx) * p.REC + OFF_CTX + c4) = vf;
                *reinterpret_cast<u32x2*>(p.recb + (sn + b0 + sidx) * p.RECB + OFF_CTX + c4) = vb;
            }
        }
    }
}

// P4's end, behind the workgroup barrier that follows the merge: o = dropout(tanh([h~ | ctx] o_W)) (attention_cell.py:82-83), this workgroup's 16
// columns, into the record (slot sn) and as hand-over words for the next step's P1 (two columns per word, tag t + 1).  a: waves 0..3 come with
// their h~ fragments (xdec_o_fetch), waves 4..7 take ctx from the A tile -- of 16 rows (rows >= NB are zero) or of 8 (AROWS: the lanes of
// rows >= NB repeat the last one).  dr: the dropout of o, null = none.
template <int NB, int AROWS, class P>
LXO_DEV void xdec_o_proj(u32x4 (&a)[4], const P& p, const XChain& c, long long sn, int t, const Drop* dr, const u32x4 (&wow)[4],
                         const bf16_t (*actx)[XC + 8], float (*red)[8][64], unsigned* ll_o) {
    if (c.wave >= 4) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) a[ks] = *reinterpret_cast<const u32x4*>(&actx[AROWS == 16 ? c.r16 : c.arow][(c.wave - 4) * 128 + ks * 32 + c.g4 * 8]);
    }
    v4f acc = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) acc = mfma16(a[ks], wow[ks], acc);
    if (c.g4 * 4 < NB) {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (NB >= 4 || i < NB) red[c.wave][c.g4 * 4 + i][c.r16] = acc[i];
    }
    __syncthreads();
    if (c.tid < NB * 16) {
        const int row = c.tid >> 4, cc = c.tid & 15;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < XW; ++w) v += red[w][row][cc];
        const int bb = c.b0 + row, n = c.rank * 16 + cc;
        v = tanh_x(v);
        if (dr) v *= drop_scale(*dr, 2u, bb, n, XO);
        p.rec[(sn + bb) * p.REC + n] = v;
        const bf16_t vb = f2bf(v);
        p.recb[(sn + bb) * p.RECB + n] = vb;
        const unsigned mine = (unsigned)vb, other = (unsigned)__shfl_xor((int)mine, 1);
        if (!(cc & 1)) { const u32x2 wv = {mine | (other << 16), (unsigned)(t + 1)}; *reinterpret_cast<u32x2*>(ll_o + ((bb * 256 + (n >> 1)) * 2)) = wv; }
    }
}

// measurement aid of the forward and backward kernels (p.dbg, null = off): thread 0 stamps slot i of the launch's step-th step
#define XSTAMP(step, i) do { if (dbg && tid == 0) dbg[(step) * 16 + (i)] = wall_clock64(); } while (0)

template <int NB, int ATT_U, bool EXPD>
__global__ __launch_bounds__(512) void xdec_fwd_kernel(XDecFwd p) {
    constexpr int NQ = 32 / NB;                                  // attention chunks per sample = workgroups per sample
    constexpr bool PP = (kLL & 4) != 0;                          // polled chunk partials (chains of one or two samples too since their merge is spread over all four thread groups: no scratch)
    // cross-wave partial tiles of the GEMM phases ([wave][row][column]) and the waves' partial contexts of P3 ([wave][channel]) share 16 KB:
    // the phases that use one are a workgroup barrier away from the phases that use the other
    __shared__ __attribute__((aligned(16))) float redbuf[XW * 8 * 64];
    float (*red)[8][64] = reinterpret_cast<float (*)[8][64]>(redbuf);
    float (*redc)[XC] = reinterpret_cast<float (*)[XC]>(redbuf);
    __shared__ u32x4 wahs[XW][2][64];                            // the att_h projection's B fragments (fragment-shaped, read back by the lane that wrote them)  16 KB
    __shared__ __attribute__((aligned(16))) bf16_t actx[16][XC + 8];   // P4: merged contexts as the A tile of the o projection   16.6 KB
    __shared__ float sc[SCMAX];                                  // raw scores of this workgroup's chunk                   16 KB
    __shared__ float cst[8][16];                                 // c state of this workgroup's 16 units (lives here for all T steps)
    __shared__ float wgt[NB][NQ], smax[NB], sinv[NB];
    __shared__ float wred[2 * XW];
    __shared__ int s_rank, s_dead, s_alen;

    // A forward-chain workgroup of two and more samples must allocate all 256 VGPRs per lane (granules of 8: v254 named = 256), so that
    // 8 waves x 256 fill the CU's register file and no foreign wave fits beside it: one that did would stretch this member's phases and with
    // them every step of its chain.  A chain that cannot get a whole CU does not assemble and gives up after 200 ms (tests/test_gpu_xdec.py).
    // Exempt: the chains of one sample (225 VGPRs), the decode kernels and the backward kernels (up to 241).  They leave room for a small
    // foreign wave and run beside it; claiming the file for them would turn a shared CU, which they tolerate, into a dropped step or decode.
    if constexpr (NB >= 2) asm volatile("" ::: "v254");
    XChain c = xchain_ticket(p.sync, NB, &s_rank, &s_dead);
    const int tid = c.tid, lane = c.lane, wave = c.wave, r16 = c.r16, g4 = c.g4;
    for (int i = tid; i < 16 * (XC + 8); i += 512) (&actx[0][0])[i] = 0;     // rows >= NB of the A tile stay zero
    __syncthreads();
    if (!xchain_rank(c, &s_rank)) return;
    const int rank = c.rank, b0 = c.b0, u0 = rank * 16;
    unsigned* xsync = c.xsync; unsigned* err = c.err;
    const int B = p.B, T = p.T;

    u32x4 wrt0[4], wow[4];
    u32x4* wl = reinterpret_cast<u32x4*>(xdec_dyn_lds) + (wave * 12) * 64 + lane;
    float bt[4];
    xdec_resident<EXPD>(p, c, wrt0, wl, wahs, wow, bt);
    if (tid < NB * 16) cst[tid >> 4][tid & 15] = p.cs[(long long)(b0 + (tid >> 4)) * XU + u0 + (tid & 15)];

    const XRole<ATT_U> ro = xdec_role<NB, ATT_U>(c, p.R, p.img, EXPD ? p.att_exp : p.att_img);
    // the formula length of this workgroup's attention sample, read once per launch (no lengths: every step is live) and kept in LDS: the kernel has no
    // scalar register to spare for a value that lives through the whole step loop (it keeps 12 .. 21 of them in VGPR lanes as it is); a uniform LDS read
    // per step, asked for in front of the att_h poll, is hidden by that poll.  Step t is DEAD for the sample when t >= s_alen.  P3 makes the flag a
    // scalar (readfirstlane): the walk's trip count hangs on it and must stay on the scalar ALU
    if (tid == 0) s_alen = p.lengths ? p.lengths[ro.ab] : T;       // (read behind P1's workgroup barriers)
    Drop dr = p.dr;
    unsigned ph = 0;
    u32x4 xiA[ATT_U], xiB[ATT_U]; u32x2 xaA[ATT_U], xaB[ATT_U];
    // the first two row blocks of step `ts`'s walk (direction ts & 1) into the two buffers
    auto prefetch = [&](int ts) {
        att_load<ATT_U>(xiA, xaA, ro.imq, ro.aiq, ro.XBASE(0, ts & 1), ro.anq, lane);
        att_load<ATT_U>(xiB, xaB, ro.imq, ro.aiq, ro.XBASE(1, ts & 1), ro.anq, lane);
    };
    prefetch(0);                                                 // step 0 walks forward: its first blocks are blocks 0 and 1

    // x-part of the LSTM pre-activation of this thread's epilogue element (threads < NB * 16: row tid >> 4, unit tid & 15), one step ahead
    float pzn[4];
    {
        const int er = min(tid >> 4, NB - 1);
        const float* zr = p.zx + (long long)(b0 + er) * 4 * XU + u0 + (tid & 15);
#pragma unroll
        for (int q = 0; q < 4; ++q) pzn[q] = zr[q * XU];
    }
    unsigned* ll_ah = p.sync + kXDecSyncBytes / 4 + kLLFwdAh / 4;
    unsigned* ll_ht = p.sync + kXDecSyncBytes / 4 + kLLFwdHt / 4;
    unsigned* ll_o = p.sync + kXDecSyncBytes / 4 + kLLFwdO / 4;
    const rsrc_t rll_ah = make_rsrc(ll_ah, (unsigned)B * XE * 8u);
    const rsrc_t rll_ht = make_rsrc(ll_ht, (unsigned)B * 256u * 8u);
    const rsrc_t rll_o = make_rsrc(ll_o, (unsigned)B * 256u * 8u);
    unsigned long long* dbg = p.dbg ? p.dbg + ((long long)(c.xcc * 32 + rank) * T) * 16 : nullptr;
    for (int t = 0; t < T; ++t) {
        dr.t = t;
        XSTAMP(t, 0);
        const long long sp = (long long)t * B, sn = (long long)(t + 1) * B;       // row blocks of the previous / this state
        // =========================== P1: LSTM cell ===========================
        {
            u32x4 a[4];
            xdec_p1_fetch(a, p, c, sp, (kLL & 8) && t > 0, rll_o, (unsigned)t);
            // the x-part of this thread's epilogue element: requested one step ahead (at the start of the previous step's P3) -- zx_t was
            // written before the launch and comes from HBM, 2 us away; asked for here it was the critical path of the phase
            float g[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] = pzn[q];
            const int erow = tid >> 4, eu = tid & 15;
            v4f acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = v4f{0.f, 0.f, 0.f, 0.f};
            if (dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); XSTAMP(t, 9); }      // measurement only: when the A operand has arrived
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                acc[0] = mfma16(a[ks], wrt0[ks], acc[0]);
#pragma unroll
                for (int q = 1; q < 4; ++q) acc[q] = mfma16(a[ks], wl[((q - 1) * 4 + ks) * 64], acc[q]);
            }
            // D layout: column = r16, row = g4 * 4 + i
            if (g4 * 4 < NB) {                                    // ONE branch for the lanes that hold real rows (sixteen per-store branches otherwise)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (NB >= 4 || i < NB) red[wave][g4 * 4 + i][q * 16 + r16] = acc[q][i];
            }
            XSTAMP(t, 10);
            __syncthreads();
            XSTAMP(t, 11);
            if (kPF == 1 && t > 0 && wave >= 2) prefetch(t);      // (step 0's blocks were requested in the prologue)
            if (tid < NB * 16) {
                float cn, h;
                xdec_lstm(g, red, erow, eu, cst[erow][eu], cn, h);
                const int bb = b0 + erow, u = u0 + eu;
                const float ht = h * drop_scale(dr, 1u, bb, u, XU);          // h~ = dropout(h) (attention_cell.py:72)
                cst[erow][eu] = cn;
                float* gr = p.gates + (sp + bb) * 4 * XU + u;
#pragma unroll
                for (int q = 0; q < 4; ++q) gr[q * XU] = g[q];
                p.cs[(sn + bb) * XU + u] = cn;
                float* rr = p.rec + (sn + bb) * p.REC;
                bf16_t* rb = p.recb + (sn + bb) * p.RECB;
                rr[OFF_H + u] = h; rr[OFF_HT + u] = ht;
                const bf16_t htb = f2bf(ht);
                rb[OFF_H + u] = f2bf(h); rb[OFF_HT + u] = htb;
                // hand-over words for P2: two units per word (the even lane of a pair stores)
                const unsigned mine = (unsigned)htb, other = (unsigned)__shfl_xor((int)mine, 1);
                if (!(eu & 1)) { const u32x2 wv = {mine | (other << 16), (unsigned)(t + 1)}; *reinterpret_cast<u32x2*>(ll_ht + ((bb * 256 + (u >> 1)) * 2)) = wv; }
            }
            if (kPF == 1 && t > 0 && wave < 2) prefetch(t);
        }
        XSTAMP(t, 1);
        if (kLL & 1) __syncthreads();                       // (the partial tiles in LDS are rewritten by P2)
        else xbar(xsync, rank, ++ph, err, &s_dead);
        XSTAMP(t, 2);
        // =========================== P2: att_h = h~ W ===========================
        xdec_p2<NB, (kLL & 1) != 0, true>(p, c, sp, sn, t, rll_ht, ll_ah, red, wahs);
        if (kPF == 2 && t > 0) prefetch(t);
        XSTAMP(t, 3);
        if (!(kLL & 2)) xbar(xsync, rank, ++ph, err, &s_dead);
        XSTAMP(t, 4);
        // =========================== P3: attention chunk (scores, online softmax, context) ===========================
        {
            {   // next step's x-part (unconditional: the last step re-reads its own)
                const int er = min(tid >> 4, NB - 1);
                const float* zr = p.zx + ((long long)min(t + 1, T - 1) * B + b0 + er) * 4 * XU + u0 + (tid & 15);
#pragma unroll
                for (int q = 0; q < 4; ++q) pzn[q] = zr[q * XU];
            }
            const int alen_v = s_alen;
            float ah[4];
            xdec_att_h<EXPD>(ah, c, ro.ab, rll_ah, (unsigned)(t + 1));
            const bool live = t < __builtin_amdgcn_readfirstlane(alen_v);
            float m = -3.0e38f, l = 0.f, acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.f;
            const int rev = t & 1;
            // a dead pair walks no block and requests none (a row that is dead stays dead: the blocks its last live step asked for are never read);
            // it publishes the partial (max -3e38, sum 0, context 0) with this step's tags like any other, so every poll of the step is served
            if constexpr (kPF == 0) xdec_walk<ATT_U, EXPD>(xiA, xaA, xiB, xaB, ro, live ? ro.nblk : 0, rev, ah, bt, m, l, acc, sc, lane);
            else {
                // the chunk ends with nothing in flight (the next step's first blocks are requested elsewhere: kPF).  Peeled so that every load is
                // unconditional on its path (a load behind a branch makes hipcc wait vmcnt(0) at the join)
                const int nblk = live ? ro.nblk : 0, an = ro.an, anq = ro.anq;      // (a dead pair computes nothing; these variants still request its first blocks)
                int it = 0;
                for (; it + 3 < nblk; it += 2) {
                    att_block<ATT_U, EXPD>(xiA, xaA, ro.XBASE(it, rev), an, ah, bt, m, l, acc, sc, lane);
                    __builtin_amdgcn_sched_barrier(0);
                    att_load<ATT_U>(xiA, xaA, ro.imq, ro.aiq, ro.XBASE(it + 2, rev), anq, lane);
                    __builtin_amdgcn_sched_barrier(0);
                    att_block<ATT_U, EXPD>(xiB, xaB, ro.XBASE(it + 1, rev), an, ah, bt, m, l, acc, sc, lane);
                    __builtin_amdgcn_sched_barrier(0);
                    att_load<ATT_U>(xiB, xaB, ro.imq, ro.aiq, ro.XBASE(it + 3, rev), anq, lane);
                    __builtin_amdgcn_sched_barrier(0);
                }
                const int rem = nblk - it;                       // 0 (empty chunk) .. 3
                if (rem >= 1) att_block<ATT_U, EXPD>(xiA, xaA, ro.XBASE(it, rev), an, ah, bt, m, l, acc, sc, lane);
                if (rem == 3) { __builtin_amdgcn_sched_barrier(0); att_load<ATT_U>(xiA, xaA, ro.imq, ro.aiq, ro.XBASE(it + 2, rev), anq, lane); __builtin_amdgcn_sched_barrier(0); }
                if (rem >= 2) att_block<ATT_U, EXPD>(xiB, xaB, ro.XBASE(it + 1, rev), an, ah, bt, m, l, acc, sc, lane);
                if (rem == 3) att_block<ATT_U, EXPD>(xiA, xaA, ro.XBASE(it + 2, rev), an, ah, bt, m, l, acc, sc, lane);
            }
            xdec_p3_publish<NQ, PP>(m, l, acc, c, ro.ab, ro.aq, t, p.part, wred, redc);
        }
        XSTAMP(t, 5);
        if constexpr (!PP) xbar(xsync, rank, ++ph, err, &s_dead);
        XSTAMP(t, 6);
        // =========================== P4: merge the chunks; alpha; ctx; o projection ===========================
        {
            u32x4 a[4];
            xdec_o_fetch(a, p, c, sn);
            // (stamp 6 -> 12 = the wait for the polled partials, which used to sit at the barrier behind P3)
            xdec_p4_merge<NB, PP, true>(p, c, sn, t, wgt, smax, sinv, redc, actx, dbg ? dbg + t * 16 + 12 : nullptr);
            if (kPF == 3) prefetch(t + 1);
            // alpha of this workgroup's chunk (what the reference hands to its visualisation hook, attention_mechanism.py:96-105)
            {
                const float mm = smax[ro.as], inv = sinv[ro.as];
                float* al = p.alpha + (sp + ro.ab) * p.Rp + ro.ar0;
                // a dead pair: exact zeros (sc holds an earlier step's scores, or nothing).  A select per element: the loop as two arms of a branch
                // put 20 more scalars into VGPR lanes
                const int alen_a = s_alen;
                for (int r = tid; r < ro.an; r += 512) { const float a = __expf(sc[r] - mm) * inv; al[r] = t < alen_a ? a : 0.f; }
            }
            __syncthreads();
            xdec_o_proj<NB, 16>(a, p, c, sn, t, &dr, wow, actx, red, ll_o);
        }
        XSTAMP(t, 7);
        if (kLL & 8) __syncthreads();                       // (the partial tiles in LDS are rewritten by the next step's P1)
        else xbar(xsync, rank, ++ph, err, &s_dead);
        XSTAMP(t, 8);
    }
}

// One launch of a chain kernel: 256 workgroups (one per CU) of 512 threads, the LDS-resident part of the LSTM weights (96 KB) as dynamic LDS
template <auto KERNEL, class P>
int xdec_launch(const P& p, hipStream_t st) {
    constexpr int DYN = XW * 12 * 64 * 16;
    static bool attr_done = false;
    if (!attr_done) { HIPRC(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, DYN)); attr_done = true; }
    hipLaunchKernelGGL(KERNEL, dim3(256), dim3(512), DYN, st, p);
    return (int)hipGetLastError();
}

template <int NB>
int launch_nb(const XDecFwd& p, hipStream_t st) {
    return p.att_exp ? xdec_launch<xdec_fwd_kernel<NB, 4, true>>(p, st) : xdec_launch<xdec_fwd_kernel<NB, 4, false>>(p, st);
}

// ------------------------------------------------------------------------------------------------ greedy-decode chain ----
// xdec_fwd_kernel's phases with the decode's feedback (XDecDec in xdec.h).  Iteration s of the loop = [boundary: logits and arg-max of step
// s - 1, from the o fragments P1 polls anyway] + [step s: P1 .. P4]; iteration nsteps is the boundary alone.  LDS: the y_W_o fragments take
// the place of the raw scores (no alpha is kept), the o projection's A tile has 8 rows instead of 16.
// SC: the log-prob of every arg-max (p.logp_out).  Beside its {max, tag | index} word a workgroup hands over {s, tag << 16}, s = the sum of
// exp(v - max) over its 16 columns; the merge forms log p = -log sum_r s_r exp(m_r - M).  SC = false is the ids-only chain.
// PF: a forced prefix (p.prefix).  At a boundary inside its prefix a row takes the forced id f in place of the merged arg-max and stays
// unfinished.  With SC the workgroup owning column f (rank f / 16) hands over a third word {v_f, tag << 16} beside the other two, the merge
// forms log p = v_f - M - log sum_r s_r exp(m_r - M).  PF = false is the chain without a prefix.
LXO_DEV int xdec_plen(const XDecDec& p, int bb) { return min(max(p.prefix_len[bb], 0), p.prefix_lim); }
LXO_DEV int xdec_forced(const XDecDec& p, int bb, int step, int plen) {  // the forced id of row bb (prefix length plen) at `step`, -1: a free step
    if (step >= plen) return -1;
    const int f = p.prefix[(long long)bb * p.prefix_ld + step];
    return (f >= 0 && f < p.V) ? f : 0;
}
// AL: allowed-token sets (p.allow).  A thread (row, column) of the logits tile holds one bit, read once per launch; a banned column is masked
// exactly where a column >= V is (value -3.0e38, exp-sum term 0): no further hand-over word.  AL = false is the chain without a constraint.
template <int NB, bool SC, bool PF, bool AL>
__global__ __launch_bounds__(512) void xdec_dec_kernel(XDecDec p) {
    // 2 rows per wave and block in flight (the training chain: 4): the decode form carries more loop-invariant addresses (token table, ids,
    // arg-max words) and with 4 rows the allocator spills 55 dwords of them into the serial phases; with 2 it spills 9
    constexpr int NQ = 32 / NB, ATT_U = 2;
    constexpr bool PP = (kLL & 4) != 0;                          // polled chunk partials, as in the training chain (tags restart with every launch: the launcher zeroes the words)
    __shared__ __attribute__((aligned(16))) float redbuf[XW * 8 * 64];
    float (*red)[8][64] = reinterpret_cast<float (*)[8][64]>(redbuf);
    float (*redc)[XC] = reinterpret_cast<float (*)[XC]>(redbuf);
    __shared__ u32x4 wahs[XW][2][64];
    __shared__ u32x4 wyos[XW][2][64];                            // y_W_o B fragments: this workgroup's 16 vocabulary columns x its wave's 64 k   16 KB
    __shared__ __attribute__((aligned(16))) bf16_t actx[8][XC + 8];
    __shared__ float redl[XW][8][16];                            // logits partial tiles [wave][row][column]   4 KB
    __shared__ float cst[8][16];
    __shared__ float wgt[NB][NQ];
    __shared__ float wred[2 * XW];
    __shared__ int ids_l[8], unf_l[8];
    __shared__ int s_rank, s_dead, s_stop;

    XChain c = xchain_ticket(p.sync, NB, &s_rank, &s_dead);
    const int tid = c.tid, lane = c.lane, wave = c.wave, r16 = c.r16, g4 = c.g4;
    if (tid == 0) s_stop = 0;
    for (int i = tid; i < 8 * (XC + 8); i += 512) (&actx[0][0])[i] = 0;
    __syncthreads();
    if (!xchain_rank(c, &s_rank)) { if (tid == 0) *reinterpret_cast<volatile int*>(p.stop) = 1; return; }
    const int rank = c.rank, b0 = c.b0, u0 = rank * 16, v0 = rank * 16;
    const unsigned xcc = c.xcc;                                  // (the LXO_TEST_DEC_FAULT build names it)
    unsigned* xsync = c.xsync; unsigned* err = c.err;
    const int B = p.B, T = p.nsteps;
    // the decode is over (an earlier launch saw every row finished): a speculative launch has nothing to do.  Every workgroup reads the same
    // word, written before this kernel started.
    if (*reinterpret_cast<volatile const int*>(p.stop) != 0) return;

    u32x4 wrt0[4], wow[4];
    u32x4* wl = reinterpret_cast<u32x4*>(xdec_dyn_lds) + (wave * 12) * 64 + lane;
    float bt[4];
    xdec_resident<true>(p, c, wrt0, wl, wahs, wow, bt);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        // y_W_o rows v0 .. v0 + 15 (rows >= V: zeros, their logits are masked anyway), this wave's k range = P1's first two k-steps (o)
        const int vr = v0 + r16;
        const u32x4 y = *reinterpret_cast<const u32x4*>(p.Wyo + (long long)min(vr, p.V - 1) * p.ldyo + wave * 64 + ks * 32 + g4 * 8);
        const u32x4 z = {0u, 0u, 0u, 0u};
        wyos[wave][ks][lane] = vr < p.V ? y : z;
    }
    if (tid < NB * 16) cst[tid >> 4][tid & 15] = p.cs[((long long)(p.t0 & 1) * B + b0 + (tid >> 4)) * XU + u0 + (tid & 15)];

    const XRole<ATT_U> ro = xdec_role<NB, ATT_U>(c, p.R, p.img, p.att_exp);
    u32x4 xiA[ATT_U], xiB[ATT_U]; u32x2 xaA[ATT_U], xaB[ATT_U];
    att_load<ATT_U>(xiA, xaA, ro.imq, ro.aiq, ro.XBASE(0, p.t0 & 1), ro.anq, lane);
    att_load<ATT_U>(xiB, xaB, ro.imq, ro.aiq, ro.XBASE(1, p.t0 & 1), ro.anq, lane);

    unsigned* ll_ah = p.sync + kXDecSyncBytes / 4 + kLLFwdAh / 4;
    unsigned* ll_ht = p.sync + kXDecSyncBytes / 4 + kLLFwdHt / 4;
    unsigned* ll_o = p.sync + kXDecSyncBytes / 4 + kLLFwdO / 4;
    unsigned* ll_am = p.sync + kXDecBlockBytes / 4 + kXDecSyncBytes / 4;      // arg-max words [B][32 workgroups]: block 1's hand-over area (zeroed by the launcher)
    const rsrc_t rll_ah = make_rsrc(ll_ah, (unsigned)B * XE * 8u);
    const rsrc_t rll_ht = make_rsrc(ll_ht, (unsigned)B * 256u * 8u);
    const rsrc_t rll_o = make_rsrc(ll_o, (unsigned)B * 256u * 8u);
    const rsrc_t rll_am = make_rsrc(ll_am, (unsigned)B * 32u * 8u);
    unsigned* ll_sm = ll_am + B * 32 * 2;                        // SC: the exponential-sum words [B][32 workgroups], behind the arg-max words
    const rsrc_t rll_sm = make_rsrc(ll_sm, (unsigned)B * 32u * 8u);
    unsigned* ll_fv = ll_sm + B * 32 * 2;                        // SC && PF: the forced-logit words [B][32 workgroups], behind the sums
    const rsrc_t rll_fv = make_rsrc(ll_fv, (unsigned)B * 32u * 8u);
    unsigned ph = 0;
    // early exit (dynamic_decode.py:38-51 stops once every row has finished): workgroup 0 of a chain looks, one boundary late and without
    // waiting, at how many chains have reported a step and how many rows it left unfinished, and raises a STOP bit in its arg-max word --
    // the one word every workgroup of the chain reads, so the whole chain leaves the loop at the same boundary
    int pr_done = 0, pr_unf = 1;
    // PF: the prefix lengths of this thread's rows, read once per launch -- the merge's row (tid >> 5) and, with SC, the logits row (tid >> 4)
    int plen_m = 0, plen_l = 0;
    if constexpr (PF) {
        if (tid < NB * 32) plen_m = xdec_plen(p, b0 + (tid >> 5));
        if constexpr (SC) { if (tid < NB * 16) plen_l = xdec_plen(p, b0 + (tid >> 4)); }
    }
    // the first column this thread's logits column (tid & 15 of the workgroup's 16) may NOT take: V, or 0 for a column its row's set bans
    int vlim = p.V;
    if constexpr (AL) {
        const int vc = v0 + (tid & 15);
        if (tid < NB * 16 && vc < p.V && !((p.allow[(long long)(b0 + (tid >> 4)) * p.allow_ld + (vc >> 5)] >> (vc & 31)) & 1u)) vlim = 0;
    }
    for (int t = 0; t <= T; ++t) {
        const int tg = p.t0 + t;                                 // global step index of the step this iteration runs
        const long long sp = (long long)(tg & 1) * B, sn = (long long)((tg + 1) & 1) * B;
        // =========================== boundary (logits, arg-max of step t - 1) + P1: LSTM cell ===========================
        {
            u32x4 a[4];
            xdec_p1_fetch(a, p, c, sp, t > 0, rll_o, (unsigned)t);
            v4f acc[4], accl = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = v4f{0.f, 0.f, 0.f, 0.f};
            if (t > 0) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) accl = mfma16(a[ks], wyos[wave][ks][lane], accl);
            }
            if (t < T) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    acc[0] = mfma16(a[ks], wrt0[ks], acc[0]);
#pragma unroll
                    for (int q = 1; q < 4; ++q) acc[q] = mfma16(a[ks], wl[((q - 1) * 4 + ks) * 64], acc[q]);
                }
            }
            if (g4 * 4 < NB) {
#pragma unroll
                for (int i = 0; i < 4; ++i) if (NB >= 4 || i < NB) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) red[wave][g4 * 4 + i][q * 16 + r16] = acc[q][i];
                    redl[wave][g4 * 4 + i][r16] = accl[i];
                }
            }
            __syncthreads();
            const int erow = tid >> 4, eu = tid & 15;
            if (t > 0) {
                // logits of this workgroup's 16 vocabulary columns, rows 0 .. NB-1; arg-max inside the 16 lanes of a row (ties: the lower index)
                if (tid < NB * 16) {
                    float v = 0.f;
#pragma unroll
                    for (int w = 0; w < XW; ++w) v += redl[w][erow][eu];
                    int vi = v0 + eu;
                    const bool masked = AL ? vi >= vlim : vi >= p.V;      // a column outside the vocabulary, or a banned one
                    if (masked) v = -3.0e38f;
                    const float vc = v;
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) {
                        const float ov = __shfl_xor(v, o); const int oi = __shfl_xor(vi, o);
                        if (ov > v || (ov == v && oi < vi)) { v = ov; vi = oi; }
                    }
                    // (workgroup 0, row 0 carries the chain's STOP bit: what thread 0 probed at the previous boundary)
                    const unsigned stopbit = (rank == 0 && erow == 0 && pr_done == 8 && pr_unf == 0) ? 0x8000u : 0u;
                    if constexpr (SC) {
                        float sr = (AL ? !masked : v0 + eu < p.V) ? expf(vc - v) : 0.f;   // columns >= V (and banned ones): 0
#pragma unroll
                        for (int o = 8; o > 0; o >>= 1) sr += __shfl_xor(sr, o);
                        if (eu == 0) { const u32x2 ws = {__float_as_uint(sr), (unsigned)t << 16}; *reinterpret_cast<u32x2*>(ll_sm + ((b0 + erow) * 32 + rank) * 2) = ws; }
                        if constexpr (PF) {
                            const int fr = xdec_forced(p, b0 + erow, tg - 1, plen_l);
                            if (fr == v0 + eu) { const u32x2 wf = {__float_as_uint(vc), (unsigned)t << 16}; *reinterpret_cast<u32x2*>(ll_fv + ((b0 + erow) * 32 + rank) * 2) = wf; }
                        }
                    }
                    if (eu == 0) { const u32x2 wv = {__float_as_uint(v), ((unsigned)t << 16) | stopbit | (unsigned)vi}; *reinterpret_cast<u32x2*>(ll_am + ((b0 + erow) * 32 + rank) * 2) = wv; }
                }
                // every workgroup gathers the 32 candidates of each of its chain's rows (thread = (row, candidate)) and reduces them
                if (tid < NB * 32) {
                    const int row = tid >> 5, cr = tid & 31;
                    const unsigned off = (unsigned)(((b0 + row) * 32 + cr) * 8);
                    float v = -3.0e38f; int vi = 0x7fffffff;
                    float sr = 0.f, vf = 0.f;
                    int fr = -1;                                          // PF: the row's forced id at step tg - 1
                    if constexpr (PF) fr = xdec_forced(p, b0 + row, tg - 1, plen_m);
                    const unsigned long long c0 = wall_clock64();
                    for (;;) {
                        const u32x2 wv = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rll_am, (int)off, 0, 16));
                        bool ok = (wv[1] >> 16) == (unsigned)t;
                        if constexpr (SC) {
                            const u32x2 ws = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rll_sm, (int)off, 0, 16));
                            ok = ok && ws[1] == ((unsigned)t << 16);
                            if (ok) sr = __uint_as_float(ws[0]);
                        }
                        if constexpr (SC && PF) {
                            if (fr >= 0 && (fr >> 4) == cr) {             // the candidate thread of the owning workgroup polls its third word too
                                const u32x2 wf = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rll_fv, (int)off, 0, 16));
                                ok = ok && wf[1] == ((unsigned)t << 16);
                                if (ok) vf = __uint_as_float(wf[0]);
                            }
                        }
                        if (ok) { v = __uint_as_float(wv[0]); vi = (int)(wv[1] & 0xffffu); }      // (bit 15 of workgroup 0's row-0 word: STOP)
                        if (__ballot(!ok) == 0ull) break;
                        if (s_dead || wall_clock64() - c0 > 20000000ull) {
                            if ((tid & 63) == 0) { s_dead = 1; *reinterpret_cast<volatile unsigned*>(err) = 4u; }
                            break;
                        }
                    }
                    if (tid == 0) s_stop = (vi >> 15) & 1;               // thread 0 holds workgroup 0's row-0 word: the chain's STOP bit
                    vi &= 0x7fff;
                    const float mr = v;
#pragma unroll
                    for (int o = 16; o > 0; o >>= 1) {
                        const float ov = __shfl_xor(v, o); const int oi = __shfl_xor(vi, o);
                        if (ov > v || (ov == v && oi < vi)) { v = ov; vi = oi; }
                    }
                    if constexpr (SC) {
                        sr *= expf(mr - v);                               // rescaled to the row's max
#pragma unroll
                        for (int o = 16; o > 0; o >>= 1) sr += __shfl_xor(sr, o);
                    }
                    if constexpr (SC && PF) vf = __shfl(vf, (lane & 32) | (fr >> 4 & 31));      // from the owner's candidate thread
                    if (cr == 0) {
                        if (vi >= p.V) vi = 0;
                        if constexpr (PF) { if (fr >= 0) vi = fr; }
                        ids_l[row] = vi;
                        if (rank == 0) {                          // one workgroup per chain publishes: ids, log-probs, finished flags
                            const int bb = b0 + row;
                            p.ids_out[(long long)bb * p.max_steps + (tg - 1)] = vi;
                            if constexpr (SC) p.logp_out[(long long)bb * p.max_steps + (tg - 1)] = (PF && fr >= 0) ? (vf - v) - logf(sr) : -logf(sr);
                            p.ids_step[bb] = vi;
                            const int fo = p.finished[bb] | (vi == p.id_end && fr < 0 ? 1 : 0);
                            p.finished[bb] = fo;
                            unf_l[row] = fo ? 0 : 1;
                        }
                    }
                }
                __syncthreads();
                if (rank == 0 && tid == 0) {
                    // ONE word per step: low 16 bits = the unfinished rows of step t - 1 summed over the chains, high bits = the number of chains
                    // that have reported -- one atomic per chain and step, and the probe of the step before (consumed at the next boundary)
                    // is ONE load: a consistent snapshot of both fields
                    int cnt = 0;
#pragma unroll
                    for (int r = 0; r < NB; ++r) cnt += unf_l[r];
                    atomicAdd(p.unfinished + (t - 1), cnt | 0x10000);
                    if (t >= 2) {
                        const int w = __hip_atomic_load(p.unfinished + (t - 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        pr_done = w >> 16; pr_unf = w & 0xffff;
                    }
                }
                if (s_stop) {
                    if (rank == 0 && tid == 0) *reinterpret_cast<volatile int*>(p.stop) = 1;
                    break;
                }
            }
            if (t == T) break;
            if (tid < NB * 16) {
                // x-part of the pre-activation: the table row of the token fed at this step (the start token at step 0 of the decode)
                const int bb = b0 + erow, u = u0 + eu;
                const int id = tg == 0 ? p.V : (t == 0 ? p.ids_step[bb] : ids_l[erow]);
                const float* zr = p.tx + (long long)id * 4 * XU + u;
                float g[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) g[q] = zr[q * XU];
                float cn, h;
                xdec_lstm(g, red, erow, eu, cst[erow][eu], cn, h);
                cst[erow][eu] = cn;
                p.cs[(sn + bb) * XU + u] = cn;
                float* rr = p.rec + (sn + bb) * p.REC;
                bf16_t* rb = p.recb + (sn + bb) * p.RECB;
                rr[OFF_H + u] = h; rr[OFF_HT + u] = h;
                const bf16_t htb = f2bf(h);
                rb[OFF_H + u] = htb; rb[OFF_HT + u] = htb;
                const unsigned mine = (unsigned)htb, other = (unsigned)__shfl_xor((int)mine, 1);
                if (!(eu & 1)) { const u32x2 wv = {mine | (other << 16), (unsigned)(t + 1)}; *reinterpret_cast<u32x2*>(ll_ht + ((bb * 256 + (u >> 1)) * 2)) = wv; }
            }
        }
        __syncthreads();
        // =========================== P2: att_h = h~ W ===========================
        xdec_p2<NB, true, false>(p, c, sp, sn, t, rll_ht, ll_ah, red, wahs);
        // =========================== P3: attention chunk ===========================
        {
            float ah[4];
            xdec_att_h<true>(ah, c, ro.ab, rll_ah, (unsigned)(t + 1));
            float m = -3.0e38f, l = 0.f, acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.f;
            xdec_walk<ATT_U, true>(xiA, xaA, xiB, xaB, ro, ro.nblk, tg & 1, ah, bt, m, l, acc, nullptr, lane);      // (no raw scores: the decode keeps no alpha)
            xdec_p3_publish<NQ, PP>(m, l, acc, c, ro.ab, ro.aq, t, p.part, wred, redc);
        }
        if constexpr (!PP) xbar(xsync, rank, ++ph, err, &s_dead);
#ifdef LXO_TEST_DEC_FAULT          // diagnostic build only (never in liblxo.so): chain 3 declares itself broken in step 21 -- profiles/r05_dec_fault_fallback.txt
        if (tg == 21 && xcc == 3u && tid == 0) { s_dead = 1; *reinterpret_cast<volatile unsigned*>(err) = 9u; }
#endif
        // =========================== P4: merge the chunks; ctx; o projection ===========================
        {
            u32x4 a[4];
            xdec_o_fetch(a, p, c, sn);
            xdec_p4_merge<NB, PP, false>(p, c, sn, t, wgt, nullptr, nullptr, redc, actx, nullptr);
            __syncthreads();
            xdec_o_proj<NB, 8>(a, p, c, sn, t, nullptr, wow, actx, red, ll_o);
        }
        __syncthreads();
    }
    // a hand-over that timed out: the ids are garbage from here on; later launches of this decode return at once, the host reads the error word
    // (which the launcher leaves alone: it is cleared once per decode) and repeats the decode on the launch-per-step kernels
    if (tid == 0 && s_dead) *reinterpret_cast<volatile int*>(p.stop) = 1;
}

template <int NB, bool SC, bool PF, bool AL>
int launch_dec_sc(const XDecDec& p, hipStream_t st) { return xdec_launch<xdec_dec_kernel<NB, SC, PF, AL>>(p, st); }
template <int NB, bool PF, bool AL>
int launch_dec_pf(const XDecDec& p, hipStream_t st) { return p.logp_out ? launch_dec_sc<NB, true, PF, AL>(p, st) : launch_dec_sc<NB, false, PF, AL>(p, st); }
template <int NB, bool AL>
int launch_dec_al(const XDecDec& p, hipStream_t st) { return p.prefix ? launch_dec_pf<NB, true, AL>(p, st) : launch_dec_pf<NB, false, AL>(p, st); }
template <int NB>
int launch_dec_nb(const XDecDec& p, hipStream_t st) { return p.allow ? launch_dec_al<NB, true>(p, st) : launch_dec_al<NB, false>(p, st); }

// ------------------------------------------------------------------------------------------------ backward chain ----
// Steps T-1 .. 0 of BPTT in one launch, same chains, same identity, same barrier.  Per step:
//   Q1  [d_h~ | d_ctx] = g_t o_W^T                                   every workgroup: its 32 columns, all NB rows
//   Q2  attention stream of one (sample, chunk): d_alpha_r = <img_r, d_ctx>, d_e_r = alpha_r (d_alpha_r - s), d_att_h += d_e_r beta (1 - tanh^2)
//   Q3  d_att_h = sum of the chunks; d_h = (d_h~ + d_att_h W_att_h^T) mask + carry; LSTM cell backward -> d_z, d_c     its 16 units
//   Q4  [d_o | d_h] carries = d_z K[D:]^T; g_{t-1} = (d_o(logits) + d_o carry) mask tanh'                              its 32 columns
// Resident per wave: its eighth of K_OW (2 x 2 fragments), of K_ATT_H (1) and of K_LSTM[D:] (16 fragments: 4 in registers, 12 in LDS).
// Steps behind a sample's end (BPTT meets them first): d_o(logits) is 0 there and nothing is carried into them, so the d_ctx row Q2 receives is 512
// exact zeros.  The kernel has no length input; the sample's workgroups see it on the row itself and stream nothing in Q2 (zeros into their d_e
// columns, a zero d_att_h partial, no request for the next step either).  The protocol is untouched -- every poll, barrier and hand-over store of
// a step stays, nobody's work moves to another workgroup, a chain still waits for its slowest member; what the live samples' workgroups gain is the
// memory bandwidth the dead ones no longer take.  The forward chain leaves the same pairs silent where it is given the lengths
// (XDecFwd.lengths); whether it did makes no difference here: the test is on d_ctx, and the forward values of a dead pair only meet exact zeros.
template <int ATT_U>
LXO_DEV void attb_load(u32x4 (&xi)[ATT_U], u32x2 (&xa)[ATT_U], float (&al)[ATT_U], rsrc_t rim, rsrc_t rai, rsrc_t ral, int base, int an, int lane) {
#pragma unroll
    for (int u = 0; u < ATT_U; ++u) {
        const int r = max(min(base + XW * u, an - 1), 0);
        xi[u] = __builtin_amdgcn_raw_buffer_load_b128(rim, lane * 16, r * (XC * 2), 0);
        xa[u] = __builtin_amdgcn_raw_buffer_load_b64(rai, lane * 8, r * (XE * 2), 0);
        al[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ral, 0, r * 4, 0));
    }
}
// EXPD: xa holds E_x = e^{2x}, ah holds E_a: r = 1 / (1 + E_x E_a), 1 - tanh^2 = 4 r (1 - r)
template <int ATT_U, bool EXPD>
LXO_DEV void attb_block(const u32x4 (&xi)[ATT_U], const u32x2 (&xa)[ATT_U], const float (&al)[ATT_U], int base, int an, const float (&dc)[8],
                        const float (&ah)[4], float s, float (&acc)[4], float* de_row, int lane) {
    float pt[ATT_U];
#pragma unroll
    for (int u = 0; u < ATT_U; ++u) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a = fmaf(__uint_as_float(xi[u][e] << 16), dc[2 * e], a);
            a = fmaf(__uint_as_float(xi[u][e] & 0xffff0000u), dc[2 * e + 1], a);
        }
        pt[u] = a;
    }
    xsum_rows<ATT_U>(pt);
#pragma unroll
    for (int u = 0; u < ATT_U; ++u) {
        const int r = base + XW * u;
        if (r >= an) continue;                                           // wave-uniform: a clamped row costs its loads, not its arithmetic
        const float d = al[u] * (pt[u] - s);                            // softmax backward
        if (lane == 0) de_row[r] = d;
        const float x0 = __uint_as_float(xa[u][0] << 16), x1 = __uint_as_float(xa[u][0] & 0xffff0000u);
        const float x2 = __uint_as_float(xa[u][1] << 16), x3 = __uint_as_float(xa[u][1] & 0xffff0000u);
        if constexpr (EXPD) {
            const float d4 = 4.f * d;
            const float r0 = __builtin_amdgcn_rcpf(fmaf(x0, ah[0], 1.f)), r1 = __builtin_amdgcn_rcpf(fmaf(x1, ah[1], 1.f));
            const float r2 = __builtin_amdgcn_rcpf(fmaf(x2, ah[2], 1.f)), r3 = __builtin_amdgcn_rcpf(fmaf(x3, ah[3], 1.f));
            acc[0] = fmaf(d4, fmaf(-r0, r0, r0), acc[0]); acc[1] = fmaf(d4, fmaf(-r1, r1, r1), acc[1]);
            acc[2] = fmaf(d4, fmaf(-r2, r2, r2), acc[2]); acc[3] = fmaf(d4, fmaf(-r3, r3, r3), acc[3]);
        } else {
            const float t0 = tanh_x(x0 + ah[0]), t1 = tanh_x(x1 + ah[1]), t2 = tanh_x(x2 + ah[2]), t3 = tanh_x(x3 + ah[3]);
            acc[0] = fmaf(d, 1.f - t0 * t0, acc[0]); acc[1] = fmaf(d, 1.f - t1 * t1, acc[1]);
            acc[2] = fmaf(d, 1.f - t2 * t2, acc[2]); acc[3] = fmaf(d, 1.f - t3 * t3, acc[3]);
        }
    }
}

template <int NB, int ATT_U, bool EXPD>
__global__ __launch_bounds__(512) void xdec_bwd_kernel(XDecBwd p) {
    constexpr int NQ = 32 / NB;                                  // attention chunks per sample
    constexpr int QS = 8 / NB;                                   // Q3: thread groups (waves) that share one sample's NQ chunk partials, 4 chunks each
    __shared__ float red[XW][8][32];                             // cross-wave partial tiles: [wave][row][column]           8 KB
    __shared__ __attribute__((aligned(16))) float redc[XW][XE];  // Q2: the waves' partial d_att_h; Q3: the chunk groups' sums   8 KB
    __shared__ __attribute__((aligned(16))) bf16_t adh[16][XE + 8];   // Q3: d_att_h as the A tile of the att_h product     8.3 KB
    __shared__ float cst[8][16];                                 // d_c of this workgroup's 16 units (lives here for all T steps)
    __shared__ int s_rank, s_dead;

    XChain c = xchain_ticket(p.sync, NB, &s_rank, &s_dead);
    const int tid = c.tid, lane = c.lane, wave = c.wave, r16 = c.r16, g4 = c.g4;
    for (int i = tid; i < 16 * (XE + 8); i += 512) (&adh[0][0])[i] = 0;      // rows >= NB of the A tile stay zero
    if (tid < 128) (&cst[0][0])[tid] = 0.f;
    __syncthreads();
    if (!xchain_rank(c, &s_rank)) return;
    const int rank = c.rank, b0 = c.b0, arow = c.arow, u0 = rank * 16, n0 = rank * 32;
    const unsigned xcc = c.xcc;
    unsigned* xsync = c.xsync; unsigned* err = c.err;
    const int B = p.B, T = p.T;

    // ---- resident weights (MFMA B fragments: lane = (output column r16, k group g4)) ----
    u32x4 wow[2][2], wahb, wk0[4];
    u32x4* wl = reinterpret_cast<u32x4*>(xdec_dyn_lds) + (wave * 12) * 64 + lane;       // + (f - 4) * 64, f = nt * 8 + ks
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            wow[nt][ks] = *reinterpret_cast<const u32x4*>(p.Wow + (long long)(n0 + nt * 16 + r16) * p.ldow + wave * 64 + ks * 32 + g4 * 8);
    wahb = *reinterpret_cast<const u32x4*>(p.Wah + (long long)(u0 + r16) * p.ldah + wave * 32 + g4 * 8);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const u32x4 w = *reinterpret_cast<const u32x4*>(p.Wk + (long long)(n0 + nt * 16 + r16) * p.ldk + wave * 256 + ks * 32 + g4 * 8);
            const int f = nt * 8 + ks;
            if (f < 4) wk0[f] = w; else wl[(f - 4) * 64] = w;
        }
    float bt[4];
    { const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.beta + lane * 4); bt[0] = b4[0]; bt[1] = b4[1]; bt[2] = b4[2]; bt[3] = b4[3]; }

    // attention role of this workgroup (as in the forward chain)
    const XRole<ATT_U> ro = xdec_role<NB, ATT_U>(c, p.R, p.img, EXPD ? p.att_exp : p.att_img);
    const int ab = ro.ab, aq = ro.aq, ar0 = ro.ar0, an = ro.an, nblk = ro.nblk, anq = ro.anq;
    const rsrc_t imq = ro.imq, aiq = ro.aiq;
    Drop dr = p.dr;
    unsigned ph = 0;
    const long long al_off = an > 0 ? (long long)ab * p.Rp + ar0 : 0;     // + t * B * Rp: this chunk's alpha rows of step t
    u32x4 xiA[ATT_U], xiB[ATT_U]; u32x2 xaA[ATT_U], xaB[ATT_U]; float alA[ATT_U], alB[ATT_U];
    {
        const rsrc_t ral = make_rsrc(p.alpha + (long long)(T - 1) * B * p.Rp + al_off, (unsigned)anq * 4u);
        attb_load<ATT_U>(xiA, xaA, alA, imq, aiq, ral, ro.XBASE(0, (T - 1) & 1), anq, lane);
        attb_load<ATT_U>(xiB, xaB, alB, imq, aiq, ral, ro.XBASE(1, (T - 1) & 1), anq, lane);
    }
    // forward values the phases of a step need, requested a few phases ahead (they come from HBM): this lane's 8 channels of ctx_t and
    // 4 columns of att_h_t (Q2); gates, c_t, c_{t-1} of this thread's LSTM element (Q3); d_o(logits) and o of step t-1 (Q4)
    f32x4 cx0, cx1, ahn;
    {
        const float* cp = p.rec + ((long long)T * B + ab) * p.REC + OFF_CTX + lane * 8;
        cx0 = *reinterpret_cast<const f32x4*>(cp); cx1 = *reinterpret_cast<const f32x4*>(cp + 4);
        ahn = *reinterpret_cast<const f32x4*>(p.atth + ((long long)(T - 1) * B + ab) * XE + lane * 4);
    }
    float lg[4], lcc = 0.f, lcp = 0.f, qd = 0.f, qo = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) lg[q] = 0.f;
    const int e3r = min(tid >> 4, NB - 1), e3u = tid & 15;       // Q3 epilogue element of this thread (threads < NB * 16)
    const int e4r = min(tid >> 5, NB - 1), e4c = tid & 31;       // Q1 / Q4 epilogue element (threads < NB * 32)
    unsigned* ll_gb = p.sync + kXDecSyncBytes / 4 + kLLBwdGb / 4;
    unsigned* ll_dc = p.sync + kXDecSyncBytes / 4 + kLLBwdDctx / 4;
    const rsrc_t rll_gb = make_rsrc(ll_gb, (unsigned)B * 256u * 8u);
    const rsrc_t rll_dc = make_rsrc(ll_dc, (unsigned)B * XC * 8u);
    unsigned long long* dbg = p.dbg ? p.dbg + ((long long)(xcc * 32 + rank) * T) * 16 : nullptr;
    // forward values the phases behind Q2 of step ts need (gates, c_ts, c_{ts-1}: Q3 of step ts; d_o(logits), o of step ts - 1: Q4) and the next
    // Q2's ctx / att_h (step ts - 1)
    auto fwd_values = [&](int ts) {
        const long long sq = (long long)ts * B;
        const int tq = max(ts - 1, 0);
        const float* cp = p.rec + ((long long)(tq + 1) * B + ab) * p.REC + OFF_CTX + lane * 8;
        cx0 = *reinterpret_cast<const f32x4*>(cp); cx1 = *reinterpret_cast<const f32x4*>(cp + 4);
        ahn = *reinterpret_cast<const f32x4*>(p.atth + ((long long)tq * B + ab) * XE + lane * 4);
        const float* gr = p.gates + (sq + b0 + e3r) * 4 * XU + u0 + e3u;
#pragma unroll
        for (int q = 0; q < 4; ++q) lg[q] = gr[q * XU];
        lcc = p.cs[(sq + B + b0 + e3r) * XU + u0 + e3u];
        lcp = p.cs[(sq + b0 + e3r) * XU + u0 + e3u];
        const int nq4 = min(n0 + e4c, XO - 1);
        qd = p.dolog[((long long)tq * B + b0 + e4r) * XO + nq4];
        qo = p.rec[((long long)(tq + 1) * B + b0 + e4r) * p.REC + nq4];
    };
    // the first two row blocks of step ts's walk (direction ts & 1) and their alpha rows
    auto prefetch_b = [&](int ts) {
        const int rv = ts & 1;
        const rsrc_t ralq = make_rsrc(p.alpha + (long long)ts * B * p.Rp + al_off, (unsigned)anq * 4u);
        attb_load<ATT_U>(xiA, xaA, alA, imq, aiq, ralq, wave + XW * ATT_U * (rv ? nblk - 1 : 0), anq, lane);
        attb_load<ATT_U>(xiB, xaB, alB, imq, aiq, ralq, wave + XW * ATT_U * (rv ? nblk - 2 : 1), anq, lane);
    };
    // the stream's software pipeline across steps: a step ends with the next step's first two blocks requested (kPFB: in Q3 / Q4), EXCEPT a dead
    // step (Q2), which requests nothing and leaves the pipeline cold; the next live step requests its own first blocks (wave-uniform: a scalar)
    bool cold = false;
    for (int t = T - 1; t >= 0; --t) {
        dr.t = t;
        XSTAMP(T - 1 - t, 0);
        const long long sp = (long long)t * B;
        const rsrc_t rdh = make_rsrc(p.dhc + sp * XHC, (unsigned)B * XHC * 4u);
        // =========================== Q1: [d_h~ | d_ctx] = g o_W^T ===========================
        {
            const rsrc_t rg = make_rsrc(p.gb + sp * p.GBP, (unsigned)B * p.GBP * 2u);
            u32x4 a[2];
            if ((kLLB & 1) && t < T - 1) {
                // g_t: polled from the hand-over words Q4 of the previous step left (no barrier behind it)
                u32x4 w[4];
                unsigned off[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) off[j] = (unsigned)(((b0 + arow) * 256 + ((wave * 64 + (j >> 1) * 32 + g4 * 8) >> 1)) * 8 + (j & 1) * 16);
                ll_wait<4>(w, rll_gb, off, (unsigned)(t + 1), err, &s_dead);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) a[ks] = u32x4{w[2 * ks][0], w[2 * ks][2], w[2 * ks + 1][0], w[2 * ks + 1][2]};
            } else {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) a[ks] = l2_load16(rg, (unsigned)(((b0 + arow) * p.GBP + wave * 64 + ks * 32 + g4 * 8) * 2));
            }
            v4f acc[2] = {v4f{0.f, 0.f, 0.f, 0.f}, v4f{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) { acc[0] = mfma16(a[ks], wow[0][ks], acc[0]); acc[1] = mfma16(a[ks], wow[1][ks], acc[1]); }
            if (g4 * 4 < NB) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (NB >= 4 || i < NB) red[wave][g4 * 4 + i][nt * 16 + r16] = acc[nt][i];
            }
            __syncthreads();
            if (tid < NB * 32) {
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < XW; ++w) v += red[w][e4r][e4c];
                p.dhc[(sp + b0 + e4r) * XHC + n0 + e4c] = v;
                if ((kLLB & 2) && n0 >= XU) {                     // the d_ctx half: hand-over words for the attention workgroups
                    const u32x2 wv = {__float_as_uint(v), (unsigned)(t + 1)};
                    *reinterpret_cast<u32x2*>(ll_dc + (((b0 + e4r) * XC + (n0 - XU) + e4c) * 2)) = wv;
                }
            }
        }
        XSTAMP(T - 1 - t, 1);
        if (!(kLLB & 2)) xbar(xsync, rank, ++ph, err, &s_dead);
        XSTAMP(T - 1 - t, 2);
        // =========================== Q2: attention stream ===========================
        {
            float dc[8], ah[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
            if (kLLB & 2) {
                u32x4 w[4];
                unsigned off[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) off[j] = (unsigned)((ab * XC + lane * 8 + 2 * j) * 8);
                ll_wait<4>(w, rll_dc, off, (unsigned)(t + 1), err, &s_dead);
#pragma unroll
                for (int e = 0; e < 8; ++e) dc[e] = __uint_as_float(w[e >> 1][(e & 1) * 2]);
            } else {
                const u32x4 d0 = l2_load16(rdh, (unsigned)((ab * XHC + XU + lane * 8) * 4)), d1 = l2_load16(rdh, (unsigned)((ab * XHC + XU + lane * 8 + 4) * 4));
#pragma unroll
                for (int e = 0; e < 4; ++e) { dc[e] = __uint_as_float(d0[e]); dc[4 + e] = __uint_as_float(d1[e]); }
            }
            float s = 0.f;                                       // s = <ctx, d_ctx> = sum_r alpha_r d_alpha_r: every wave forms it by itself
#pragma unroll
            for (int e = 0; e < 4; ++e) s = fmaf(cx0[e], dc[e], fmaf(cx1[e], dc[4 + e], s));
            { float sv[1] = {s}; xsum_rows<1>(sv); s = sv[0]; }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ah[j] = ahn[j];
                if constexpr (EXPD) ah[j] = __builtin_amdgcn_exp2f(fminf(fmaxf(ah[j] * 2.8853900817779268f, -60.f), 60.f));
            }
            float* de_row = p.de + (sp + ab) * p.Rp + ar0;
            const int rev = t & 1;
            const int tn = max(t - 1, 0);
            const rsrc_t ral = make_rsrc(p.alpha + sp * p.Rp + al_off, (unsigned)anq * 4u);
            const rsrc_t raln = make_rsrc(p.alpha + (long long)tn * B * p.Rp + al_off, (unsigned)anq * 4u);
            // A step behind the sample's end: d_o(logits) is 0 there and so is everything BPTT carried into it, so d_ctx is 512 exact zeros, every d_e
            // of the row is alpha (0 - 0) and the d_att_h partial a sum of zeros.  Every wave holds the whole d_ctx row: all waves of the workgroup
            // and all workgroups of the sample decide alike.  Such a step requests and computes no block; it stores the zeros of its d_e columns
            // (datt_img_live_kernel finds a row's live range by d != 0) and goes on to the forward values, the workgroup barrier and the partial's
            // hand-over words (acc is still 0) like any other step: no poll, barrier or hand-over store is left out.
            bool nz = false;
#pragma unroll
            for (int e = 0; e < 8; ++e) nz = nz || dc[e] != 0.f;     // (a NaN is not a zero: a broken step streams as before)
            // (readfirstlane: known uniform.  Left to the compiler, the loop counter below that starts from `cold` becomes a vector register, and with
            // it every row address of the stream and the block's row tests -- measured: 14.7 us for a live step's stream against 11.9)
            const bool dead_step = __builtin_amdgcn_readfirstlane(__ballot(nz) == 0ull ? 1 : 0) != 0;
            if (dead_step) for (int i = tid; i < an; i += 512) de_row[i] = 0.f;
            if constexpr (kPFB == 0) {
            // A dead step walks no block (nb = 0) and requests nothing: the pipeline is cold behind it.  The first live step behind dead ones starts
            // one trip early (it = -2), which computes nothing and requests blocks 0 and 1 of its own walk as the kernel's prologue does for
            // t = T - 1 -- one exposed load latency per sample and launch; the loop's requests stay the only ones (a second place that writes the
            // block registers costs a second register set: the allocator does not merge the two).
            const int nb = dead_step ? 0 : nblk;
            for (int it = __builtin_amdgcn_readfirstlane((cold && nb > 0) ? -2 : 0); it < nb; it += 2) {
                const bool moreA = it + 2 < nblk, moreB = it + 3 < nblk;
                if (it >= 0) {
                    attb_block<ATT_U, EXPD>(xiA, xaA, alA, ro.XBASE(it, rev), an, dc, ah, s, acc, de_row, lane);
                    __builtin_amdgcn_sched_barrier(0);
                }
                attb_load<ATT_U>(xiA, xaA, alA, imq, aiq, moreA ? ral : raln, moreA ? ro.XBASE(it + 2, rev) : ro.XBASE(0, rev ^ 1), anq, lane);
                __builtin_amdgcn_sched_barrier(0);
                if (it + 1 < nblk) {                              // (an odd block count ends on an A half: B already holds the next step's block 1)
                    if (it >= 0) {
                        attb_block<ATT_U, EXPD>(xiB, xaB, alB, ro.XBASE(it + 1, rev), an, dc, ah, s, acc, de_row, lane);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    attb_load<ATT_U>(xiB, xaB, alB, imq, aiq, moreB ? ral : raln, moreB ? ro.XBASE(it + 3, rev) : ro.XBASE(1, rev ^ 1), anq, lane);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            cold = dead_step;
            } else if (!dead_step) {
            if (cold) { prefetch_b(t); cold = false; }          // kPFB: the first live step behind dead ones requests its own first blocks (Q3 / Q4 of a dead step request nothing)
            // the chunk ends with nothing in flight (kPFB: the next step's first blocks are requested in Q3 / Q4); peeled as in the forward chain
            int it = 0;
            for (; it + 3 < nblk; it += 2) {
                attb_block<ATT_U, EXPD>(xiA, xaA, alA, ro.XBASE(it, rev), an, dc, ah, s, acc, de_row, lane);
                __builtin_amdgcn_sched_barrier(0);
                attb_load<ATT_U>(xiA, xaA, alA, imq, aiq, ral, ro.XBASE(it + 2, rev), anq, lane);
                __builtin_amdgcn_sched_barrier(0);
                attb_block<ATT_U, EXPD>(xiB, xaB, alB, ro.XBASE(it + 1, rev), an, dc, ah, s, acc, de_row, lane);
                __builtin_amdgcn_sched_barrier(0);
                attb_load<ATT_U>(xiB, xaB, alB, imq, aiq, ral, ro.XBASE(it + 3, rev), anq, lane);
                __builtin_amdgcn_sched_barrier(0);
            }
            const int rem = nblk - it;
            if (rem >= 1) attb_block<ATT_U, EXPD>(xiA, xaA, alA, ro.XBASE(it, rev), an, dc, ah, s, acc, de_row, lane);
            if (rem == 3) { __builtin_amdgcn_sched_barrier(0); attb_load<ATT_U>(xiA, xaA, alA, imq, aiq, ral, ro.XBASE(it + 2, rev), anq, lane); __builtin_amdgcn_sched_barrier(0); }
            if (rem >= 2) attb_block<ATT_U, EXPD>(xiB, xaB, alB, ro.XBASE(it + 1, rev), an, dc, ah, s, acc, de_row, lane);
            if (rem == 3) attb_block<ATT_U, EXPD>(xiA, xaA, alA, ro.XBASE(it + 2, rev), an, dc, ah, s, acc, de_row, lane);
            } else cold = true;
            // forward values of the coming phases (unconditional, clamped indices)
            fwd_values(t);
#pragma unroll
            for (int j = 0; j < 4; ++j) redc[wave][lane * 4 + j] = acc[j] * bt[j];
            __syncthreads();
            if (tid < XE) {
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < XW; ++w) v += redc[w][tid];
                if constexpr (kLLB & 4) {
                    // polled hand-over: 128 pack28 words per (sample, chunk) -- the kilobyte the plain f32 partial took
                    const float other = __shfl_xor(v, 1);
                    if (!(tid & 1)) *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned*>(p.part) + (((long long)ab * NQ + aq) * (XE / 2) + (tid >> 1)) * 2) = pack28(v, other, tag8_of(t));
                } else p.part[((long long)ab * NQ + aq) * XE + tid] = v;
            }
        }
        XSTAMP(T - 1 - t, 3);
        // (kLLB & 4: no barrier here.  Q3 also reads d_h~ (Q1 of other workgroups) and the carried d_h (Q4 of the previous step): both were stored in front of a
        // workgroup barrier -- on gfx950 a wait for the store acknowledgements -- that their producers passed before they stored the partial / d_ctx words Q3's
        // and Q2's polls have seen; and nobody rewrites the partial words of this step before every workgroup has read them: the next Q2 needs d_ctx of
        // workgroups that are past this step's Q3.)
        if constexpr (!(kLLB & 4)) xbar(xsync, rank, ++ph, err, &s_dead);
        XSTAMP(T - 1 - t, 4);
        // =========================== Q3: d_att_h; d_h; LSTM cell backward ===========================
        {
            const rsrc_t rpart = make_rsrc(p.part + (long long)b0 * NQ * XE, (unsigned)(NB * NQ * XE) * 4u);      // (kLLB & 4: 128 pack28 words per partial = the same kilobyte)
            const rsrc_t rcar = make_rsrc(p.carry_h, (unsigned)B * XU * 4u);
            // wave `slot` sums 4 of the NQ chunk partials of sample slot / QS; the QS groups of a sample meet in LDS
            const int srow = wave / QS, sqg = wave - srow * QS;
            u32x4 pc[4];
            if constexpr (kLLB & 4) {
                unsigned off[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) off[j] = (unsigned)((((srow * NQ + sqg * 4 + j) * (XE / 2)) + lane * 2) * 8);
                ll_wait8<4>(pc, rpart, off, tag8_of(t), err, &s_dead);
                XSTAMP(T - 1 - t, 12);                                       // measurement only: the polled d_att_h partials have arrived
            } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) pc[j] = l2_load16(rpart, (unsigned)((((srow * NQ + sqg * 4 + j) * XE) + lane * 4) * 4));
            }
            const float dhm = l2_load4(rdh, (unsigned)(((b0 + e3r) * XHC + u0 + e3u) * 4));
            const float chv = l2_load4(rcar, (unsigned)(((b0 + e3r) * XU + u0 + e3u) * 4));
            {
                f32x4 v;
                if constexpr (kLLB & 4) {
                    // chunk j: words {c0 c1 tag}{c2 c3 tag}; the same association as the plain form: (p0 + p1) + (p2 + p3)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        v[2 * h] = (unpack28_lo(pc[0][2 * h]) + unpack28_lo(pc[1][2 * h])) + (unpack28_lo(pc[2][2 * h]) + unpack28_lo(pc[3][2 * h]));
                        v[2 * h + 1] = (unpack28_hi(pc[0][2 * h], pc[0][2 * h + 1]) + unpack28_hi(pc[1][2 * h], pc[1][2 * h + 1])) + (unpack28_hi(pc[2][2 * h], pc[2][2 * h + 1]) + unpack28_hi(pc[3][2 * h], pc[3][2 * h + 1]));
                    }
                } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (__uint_as_float(pc[0][e]) + __uint_as_float(pc[1][e])) + (__uint_as_float(pc[2][e]) + __uint_as_float(pc[3][e]));
                }
                *reinterpret_cast<f32x4*>(&redc[wave][lane * 4]) = v;
            }
            __syncthreads();
            if (kPFB == 1 && t > 0 && !cold) prefetch_b(t - 1);
            if (tid < NB * 64) {
                const int row = tid >> 6, k4 = (tid & 63) * 4;
                f32x4 v = *reinterpret_cast<const f32x4*>(&redc[row * QS][k4]);
#pragma unroll
                for (int g = 1; g < QS; ++g) { const f32x4 w = *reinterpret_cast<const f32x4*>(&redc[row * QS + g][k4]); v += w; }
                const u32x2 vb = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
                *reinterpret_cast<u32x2*>(&adh[row][k4]) = vb;
                if (rank == row) {                               // kept for the deferred dW_att_h product (f32 + the bf16 mirror its GEMM reads)
                    *reinterpret_cast<f32x4*>(p.datth + (sp + b0 + row) * XE + k4) = v;
                    if (p.datthb) *reinterpret_cast<u32x2*>(p.datthb + (sp + b0 + row) * XE + k4) = vb;
                }
            }
            __syncthreads();
            const u32x4 a = *reinterpret_cast<const u32x4*>(&adh[r16][wave * 32 + g4 * 8]);
            v4f acc = v4f{0.f, 0.f, 0.f, 0.f};
            acc = mfma16(a, wahb, acc);
            if (g4 * 4 < NB) {
#pragma unroll
                for (int i = 0; i < 4; ++i) if (NB >= 4 || i < NB) red[wave][g4 * 4 + i][r16] = acc[i];
            }
            __syncthreads();
            if (tid < NB * 16) {
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < XW; ++w) v += red[w][e3r][e3u];
                const int bb = b0 + e3r, u = u0 + e3u;
                // backward of the TF-1.12 LSTMCell (gates i, j, f, o) -- the same expressions as the launch chain's epilogue (rstep.hip)
                const float dh = (dhm + v) * drop_scale(dr, 1u, bb, u, XU) + (t == T - 1 ? 0.f : chv);
                const float tc = tanh_x(lcc);
                const float dcv = cst[e3r][e3u] + dh * lg[3] * (1.f - tc * tc);
                const float dzi = dcv * lg[1] * lg[0] * (1.f - lg[0]);
                const float dzj = dcv * lg[0] * (1.f - lg[1] * lg[1]);
                const float dzf = dcv * lcp * lg[2] * (1.f - lg[2]);
                const float dzo = dh * tc * lg[3] * (1.f - lg[3]);
                cst[e3r][e3u] = dcv * lg[2];
                float* dzr = p.dz + (sp + bb) * 4 * XU + u;
                dzr[0] = dzi; dzr[XU] = dzj; dzr[2 * XU] = dzf; dzr[3 * XU] = dzo;
                bf16_t* db = p.dzb + (sp + bb) * p.DZBP + u;
                db[0] = f2bf(dzi); db[XU] = f2bf(dzj); db[2 * XU] = f2bf(dzf); db[3 * XU] = f2bf(dzo);
            }
        }
        XSTAMP(T - 1 - t, 5);
        xbar(xsync, rank, ++ph, err, &s_dead);
        XSTAMP(T - 1 - t, 6);
        // =========================== Q4: carries = d_z K[D:]^T; g_{t-1} ===========================
        {
            const rsrc_t rdz = make_rsrc(p.dzb + sp * p.DZBP, (unsigned)B * p.DZBP * 2u);
            u32x4 a[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) a[ks] = l2_load16(rdz, (unsigned)(((b0 + arow) * p.DZBP + wave * 256 + ks * 32 + g4 * 8) * 2));
            v4f acc[2] = {v4f{0.f, 0.f, 0.f, 0.f}, v4f{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                acc[0] = mfma16(a[ks], ks < 4 ? wk0[ks < 4 ? ks : 0] : wl[(ks - 4) * 64], acc[0]);
                acc[1] = mfma16(a[ks], wl[(8 + ks - 4) * 64], acc[1]);
            }
            if (g4 * 4 < NB) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (NB >= 4 || i < NB) red[wave][g4 * 4 + i][nt * 16 + r16] = acc[nt][i];
            }
            __syncthreads();
            if (kPFB == 3 && t > 0 && !cold) prefetch_b(t - 1);
            if (tid < NB * 32) {
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < XW; ++w) v += red[w][e4r][e4c];
                const int bb = b0 + e4r, n = n0 + e4c;
                if (t == 0) p.dxh[(long long)bb * XXH + n] = v;              // raw carries for the initial-state gradients
                else if (n < XO) {
                    // g_{t-1} = (d_o(logits) + d_o carry) * dropout mask * (1 - tanh^2), tanh from o_{t-1}   (attention_cell.py:82-83 backward)
                    Drop dq = dr; dq.t = t - 1;
                    const float sc = drop_scale(dq, 2u, bb, n, XO);
                    const float th = (dq.thr == 0u) ? qo : qo / dq.inv_keep;   // rec holds the dropped o; where the mask is 1 tanh = o * keep
                    const float g = (qd + v) * sc * (1.f - th * th);
                    p.gall[(sp - B + bb) * XO + n] = g;
                    const bf16_t gbv = f2bf(g);
                    p.gb[(sp - B + bb) * p.GBP + n] = gbv;
                    if (kLLB & 1) {                              // hand-over words for the next step's Q1: two columns per word
                        const unsigned mine = (unsigned)gbv, other = (unsigned)__shfl_xor((int)mine, 1);
                        if (!(e4c & 1)) { const u32x2 wv = {mine | (other << 16), (unsigned)t}; *reinterpret_cast<u32x2*>(ll_gb + ((bb * 256 + (n >> 1)) * 2)) = wv; }
                    }
                } else p.carry_h[(long long)bb * XU + (n - XO)] = v;
            }
        }
        XSTAMP(T - 1 - t, 7);
        if (kLLB & 1) __syncthreads();                           // (the partial tiles in LDS are rewritten by the next step's Q1)
        else xbar(xsync, rank, ++ph, err, &s_dead);
        XSTAMP(T - 1 - t, 8);
    }
    if (tid < NB * 16) p.dcc[(long long)(b0 + e3r) * XU + u0 + e3u] = cst[e3r][e3u];
}

template <int NB>
int launch_bwd_nb(const XDecBwd& p, hipStream_t st) {
    return p.att_exp ? xdec_launch<xdec_bwd_kernel<NB, 4, true>>(p, st) : xdec_launch<xdec_bwd_kernel<NB, 4, false>>(p, st);
}
}  // namespace

// What the three launchers ask alike.  Returns NB = B / 8 (1, 2, 4 or 8), or 0: the shape does not qualify or the chain is switched off, and
// the launcher answers -2.  LXO_XDEC=0 sends everything to the launch-per-step kernels, the launcher's
// `own` switch (SW_XDEC: none) set to 0 that chain alone (A/B runs).  Only the shipped sizes run here, in chains of 1, 2, 4 or 8 samples with
// attention chunks of 1 .. rows_max rows, and the chain needs 8 XCDs x 32 CUs (MI355X).
static int xdec_gate(LxoSwitch own, int U, int O, int C, int E, int B, int R, int rows_max) {
    if (!lxo_switch(SW_XDEC) || !lxo_switch(own)) return 0;
    if (U != XU || O != XO || C != XC || E != XE) return 0;
    if (B % 8 != 0 || B > 64) return 0;
    const int nb = B / 8;
    if (nb != 1 && nb != 2 && nb != 4 && nb != 8) return 0;
    const int nq = 32 / nb, rows_per = (R + nq - 1) / nq;
    if (rows_per > rows_max || rows_per < 1) return 0;
    static int dev_ok = -1;
    if (dev_ok < 0) {
        int dev = 0; hipDeviceProp_t pr;
        dev_ok = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount == 256) ? 1 : 0;
    }
    return dev_ok ? nb : 0;
}

static thread_local unsigned long long* g_xdbg = nullptr;
extern "C" int lxo_xdec_debug(unsigned long long* buf) { g_xdbg = buf; return 0; }
int lxo_launch_xdec_fwd(const XDecFwd& p0, int U, int O, int C, int E, hipStream_t st) {
    XDecFwd p = p0;
    p.dbg = g_xdbg;
    const int nb = xdec_gate(SW_XDEC, U, O, C, E, p.B, p.R, SCMAX);       // (the raw scores of a chunk stay in LDS)
    if (!nb || p.T < 1) return -2;
    if ((long long)p.B * p.RECB * 2 >= (1LL << 31) || p.ldrt % 8 || p.ldah % 8 || p.ldow % 8 || p.RECB % 8) return -2;
    HIPRC(hipMemsetAsync(p.sync, 0, kXDecBlockBytes, st));
    if (kLL & 4) HIPRC(hipMemsetAsync(p.part, 0, (size_t)p.B * (32 / nb) * PLW * 8, st));      // the polled chunk partials: no tag of an earlier launch may pass

    // rows per wave and block (two blocks in flight).  4: the largest count whose two blocks + the resident weights fit the register file
    // without spills (5 .. 7 spill 68 .. 208 bytes per lane into the serial phases and lose more there than their fewer padded rows gain:
    // 23.9 / 28.9 / 28.3 us per step against 22.2, profiles/r04_xdec_stamps_v2.txt).
    switch (nb) {
    case 1: return launch_nb<1>(p, st);
    case 2: return launch_nb<2>(p, st);
    case 4: return launch_nb<4>(p, st);
    default: return launch_nb<8>(p, st);
    }
}
int lxo_launch_xdec_dec(const XDecDec& p, int U, int O, int C, int E, hipStream_t st) {
    const int nb = xdec_gate(SW_XDEC_DEC, U, O, C, E, p.B, p.R, 1 << 30);     // (no raw scores are kept: any chunk length)
    if (!nb || p.nsteps < 1 || p.nsteps > 16 || p.V < 1 || p.V > 512 || !p.stop) return -2;      // 32 workgroups x 16 vocabulary columns; one counter word per step and launch
    if ((long long)p.B * p.RECB * 2 >= (1LL << 31) || p.ldrt % 8 || p.ldah % 8 || p.ldow % 8 || p.ldyo % 8 || p.RECB % 8 || !p.att_exp) return -2;
    // tickets / flags and the hand-over area, but NOT the error word (int 512): an error of an earlier launch of this decode stays visible
    HIPRC(hipMemsetAsync(p.sync, 0, 8 * 64 * 4, st));
    HIPRC(hipMemsetAsync(p.sync + 8 * 64 + 1, 0, kXDecBlockBytes - (8 * 64 + 1) * 4, st));
    HIPRC(hipMemsetAsync(p.sync + kXDecBlockBytes / 4 + kXDecSyncBytes / 4, 0, (size_t)p.B * 32 * 8 * (p.logp_out ? (p.prefix ? 3 : 2) : 1), st));      // the arg-max words (block 1's hand-over area; + the exponential sums, + the forced logits)
    if (kLL & 4) HIPRC(hipMemsetAsync(p.part, 0, (size_t)p.B * (32 / nb) * PLW * 8, st));               // the polled chunk partials (tags restart with every launch)
    switch (nb) {
    case 1: return launch_dec_nb<1>(p, st);
    case 2: return launch_dec_nb<2>(p, st);
    case 4: return launch_dec_nb<4>(p, st);
    default: return launch_dec_nb<8>(p, st);
    }
}
static thread_local unsigned long long* g_xdbg_b = nullptr;
extern "C" int lxo_xdec_debug_bwd(unsigned long long* buf) { g_xdbg_b = buf; return 0; }
int lxo_launch_xdec_bwd(const XDecBwd& p0, int U, int O, int C, int E, hipStream_t st) {
    XDecBwd p = p0;
    p.dbg = g_xdbg_b;
    const int nb = xdec_gate(SW_XDEC_BWD, U, O, C, E, p.B, p.R, SCMAX);       // (the forward chain must have run the same shape)
    if (!nb || p.T < 1) return -2;
    if (p.ldow % 8 || p.ldah % 8 || p.ldk % 8 || p.GBP % 8 || p.DZBP % 8 || p.REC % 4 || (long long)p.B * p.DZBP * 2 >= (1LL << 31)) return -2;
    HIPRC(hipMemsetAsync(p.sync, 0, kXDecBlockBytes, st));
    if (kLLB & 4) HIPRC(hipMemsetAsync(p.part, 0, (size_t)p.B * (32 / nb) * XE * 4, st));      // the polled d_att_h partials (the forward chain's words lie there: no tag of theirs may pass)
    switch (nb) {
    case 1: return launch_bwd_nb<1>(p, st);
    case 2: return launch_bwd_nb<2>(p, st);
    case 4: return launch_bwd_nb<4>(p, st);
    default: return launch_bwd_nb<8>(p, st);
    }
}
#endif
