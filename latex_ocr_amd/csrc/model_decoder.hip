// Host driver of the decoder: it launches every kernel of the training forward, the BPTT and the decodes.
//   step_path()                  which kernels run a shape's recurrence -- decided once, read by every user below
//   lxo_impl_decoder_train_fwd   set-up | recurrence (persistent chain, fused loop or split-K loop) | logits
//   lxo_impl_decoder_train_bwd   logits part | recurrence (the same three) | initial states, deferred weight gradients, embedding gradient
//                                (on the weight-gradient side stream where one is bound: BwdStreams) | d_img | join
//   decode                       shared set-up, host loop and select step of the greedy, sampled, beam and step-wise calls
// Reference graph: model/decoder.py:41-72, model/components/attention_mechanism.py,
// model/components/attention_cell.py:58-89, model/img2seq.py:68-75.
#include "plan.h"
#include "impl.h"
#include "gemm.h"
#include "head_kernels.h"
#include "grammar.h"
#include "rstep.h"
#include "xdec.h"
#include "dimg.h"
#include "api_util.h"
#include "switches.h"
#include "timing.h"

namespace {
// dense C = act(A * Bp^T + bias) on the compute dtype `dt`
int nt(const Plan& P, bool a_f32, bool c_f32, bool small, const void* A, int lda, const void* Bp, int ldb, void* C, int ldc,
       int M, int N, int K, const float* bias, int act, bool accumulate, hipStream_t st) {
    GemmNT g; memset(&g, 0, sizeof(g));
    g.A = A; g.Bp = Bp; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.bias = bias; g.act = act; g.alpha = 1.f; g.accumulate = accumulate ? 1 : 0; g.addend_rows = 1;
    if (P.s.dtype == LXO_F32) { a_f32 = true; c_f32 = true; }
    return lxo_launch_gemm_nt(P.s.dtype, a_f32, c_f32, small, g, st);
}
// C[I][J] += A^T B over M rows
int tn(const Plan& P, bool a_f32, bool b_f32, const void* A, int lda, const void* B, int ldb, float* C, int ldc,
       int M, int I, int J, hipStream_t st, DetScratch det = DetScratch{nullptr, 0}) {
    GemmTN g; memset(&g, 0, sizeof(g));
    g.A = A; g.B = B; g.C = C; g.M = M; g.I = I; g.J = J; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    const int tiles = cdiv(I, 128) * cdiv(J, 128);
    int ns = cdiv(512, tiles);
    const int maxs = M / 64 > 0 ? M / 64 : 1;
    if (ns > maxs) ns = maxs;
    g.nsplit = ns < 1 ? 1 : ns; g.nbatch = 1; g.atomic = 1;
    // bf16 deterministic mode: partial tiles to the slab, added in range order (or, without a slab, one row range per output tile)
    if (P.bf && P.det()) { if (det.p) { g.det_slab = det.p; g.det_floats = det.floats; } else g.nsplit = 1; }
    if (P.s.dtype == LXO_F32) { a_f32 = true; b_f32 = true; }
    return lxo_launch_gemm_tn(P.s.dtype, a_f32, b_f32, g, st);
}
// split-K partial products slab[ks] = A[:, ks*128:+128] * Bp^T  (one memory round trip; consumers add the slabs)
int slab(const Plan& P, const float* A, int lda, const void* Bp, int ldb, float* out, int M, int N, int K, hipStream_t st) {
    GemmNT g; memset(&g, 0, sizeof(g));
    g.A = A; g.Bp = Bp; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = N; g.alpha = 1.f; g.addend_rows = 1;
    return lxo_launch_gemm_slab(P.s.dtype, g, out, (long long)M * N, st);
}
Slabs view(const float* p, int K, int M, int N) { Slabs s = {p, K / 128, (long long)M * N, N}; return s; }
const Slabs kNoSlabs = {nullptr, 0, 0, 0};
}  // namespace

// the attention kernels walk their row blocks in alternating directions from step to step (L2 reuse; LXO_ATT_ALT=0: always forward)
static bool att_alternate() { return lxo_switch(SW_ATT_ALT) != 0; }
// out[M][N] (+)= act(A[M][K] W[N][K]^T + bias) for the few-row GEMMs outside the loops (initial states, their gradients) on the
// fused step kernels (16-row tiles, one workgroup per 16 columns: 128 workgroups where gemm_skinny_kernel has 16)
static int rs_dense(const Plan& P, const float* A, int lda, const void* W, int ldw, float* out, int ldo, int M, int N, int K,
                    const float* bias, bool tanh_act, bool accumulate, hipStream_t st) {
    RStep a; memset(&a, 0, sizeof(a));
    a.M = M; a.N = N; a.K = K; a.U = P.s.U; a.O = P.s.O; a.zx_row = -1;
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.out = out; a.ldo = ldo; a.bias = bias; a.accumulate = accumulate ? 1 : 0;
    a.epi = tanh_act ? RS_TANH_O : RS_PLAIN;              // dropout descriptor zero: tanh only
    a.dr.inv_keep = 1.f;
    return lxo_launch_rstep(P.s.dtype, 0, a, st);
}

// Side stream for the half-batch interleave of the recurrent loop (set per host thread through
// lxo_set_side_stream; null = single stream).  The recurrence is a chain of ~13 short, latency-bound
// launches per step pair; the two halves of the batch are independent, so running them on two HIP
// streams lets one half's launch/latency gaps be filled by the other half's kernels.
static thread_local hipStream_t g_side = nullptr;
static thread_local hipEvent_t g_ev_fork = nullptr, g_ev_join = nullptr;
int lxo_impl_set_side_stream(hipStream_t s) {
    g_side = s;
    if (s && !g_ev_fork) {
        HIPRC(hipEventCreateWithFlags(&g_ev_fork, hipEventDisableTiming));
        HIPRC(hipEventCreateWithFlags(&g_ev_join, hipEventDisableTiming));
    }
    return 0;
}
static int fork_side(hipStream_t st) { HIPRC(hipEventRecord(g_ev_fork, st)); HIPRC(hipStreamWaitEvent(g_side, g_ev_fork, 0)); return 0; }
static int join_side(hipStream_t st) { HIPRC(hipEventRecord(g_ev_join, g_side)); HIPRC(hipStreamWaitEvent(st, g_ev_join, 0)); return 0; }

// ------------------------------------------------------------------ the step path ----
// The fused step kernels split a contraction over the 4 waves in chunks of 32 / 64 k whose count must be a power of two up to 16
// (rstep.hip: launch_nch): true for every contraction of the shipped sizes (and of any U, O, E, C in {128, 256, 512} that are
// equal); a mixed shape such as U = 128, C = 256 (K = 384) runs on round 1's split-K step kernels instead.
static bool rstep_k_ok(int K, bool bf) {
    if (K % 128) return false;
    const int kq = K / 4;
    auto pow2_16 = [](int n) { return n >= 1 && n <= 16 && (n & (n - 1)) == 0; };
    if (bf && kq % 64 == 0 && pow2_16(kq / 64)) return true;
    return kq % 32 == 0 && pow2_16(kq / 32);
}
// Which kernels run the recurrence of a shape: step_path() decides, everything below reads its answer.
//   shape      the fused launch-per-step kernels (rstep.hip) where the contraction lengths and lxo_shape.step_kernels allow them, else round 1's
//              split-K kernels.  Every decode and the few-row GEMMs outside the loops (initial states, their gradients) follow it
//   dual, loop training with a side stream bound and an even batch: the halves interleave on two streams, on the split-K kernels; otherwise loop = shape
//   mirrors    bf16 on the fused kernels: they leave bf16 mirrors of the record, g_t and d_z_t, which the GEMMs around the loops read ...
//   try_chain  ... and the persistent chain (xdec.hip) is tried first (lxo_shape.step_kernels 0): its launcher answers -2 for a shape it does
//              not take, and the caller runs the fused loop
struct StepPath {
    enum Kernels { SplitK, Fused };
    Kernels shape, loop;
    bool dual, mirrors, try_chain;
};
static StepPath step_path(const Plan& P, bool training) {
    StepPath p;
    p.shape = P.s.step_kernels == 1 ? StepPath::SplitK : StepPath::Fused;
    const int ks[7] = {P.XH, P.s.U, P.HC, P.s.O, P.s.E, 4 * P.s.U, P.s.C};     // C: the initial-state projections run on the step kernels too
    for (int k : ks) if (!rstep_k_ok(k, P.bf) || !rstep_k_ok(k, false)) p.shape = StepPath::SplitK;     // the f32-operand launches (A converted on load) use 32-k chunks
    p.dual = training && g_side != nullptr && P.s.B >= 2 && (P.s.B % 2) == 0;
    p.loop = p.dual ? StepPath::SplitK : p.shape;
    p.mirrors = P.bf && p.loop == StepPath::Fused;
    p.try_chain = p.mirrors && P.s.step_kernels == 0;
    return p;
}
// chunks of the attention backward for nr rows: the ordered modes take one per sample = one writer per d_att_h element
static int attn_bwd_chunks(const Plan& P, int nr) { return P.det() ? 1 : P.attn_chunks(nr); }

// ws region "xdec_sync" (xdec.h): the block of chain `which` and its error word
enum { kChainFwd = 0, kChainBwd = 1 };
static unsigned* chain_block(const Plan& P, void* ws, int which) { return P.ws<unsigned>(ws, W_XSYNC) + which * kXDecBlockWords; }
static unsigned* chain_err(const Plan& P, void* ws, int which) { return P.bf ? chain_block(P, ws, which) + kXDecErrWord : nullptr; }      // (f32: no chains, no word)

// The three initial-state projections (attention_cell.py:51-56), in launch order c, h, o: where the weight block starts in K_INIT_T /
// K_INIT (bytes), its width, its parameters, and `x`: the destination of the forward product or the d_pre columns of the backward ones
struct InitProj { size_t woff; int n; ParamId bias, weight; float* x; int ldx; };
struct InitProjs { InitProj p[3]; const InitProj* begin() const { return p; } const InitProj* end() const { return p + 3; } };
static InitProjs init_projs(const Plan& P, float* c, int ldc, float* h, int ldh, float* o, int ldo) {
    const size_t blk = (size_t)P.s.U * P.s.C * P.esz;
    return {{{0, P.s.U, P_BC0, P_WC0, c, ldc}, {blk, P.s.U, P_BH0, P_WH0, h, ldh}, {2 * blk, P.s.O, P_BO0, P_WO0, o, ldo}}};
}

// att_img projection + initial states (attention_mechanism.py:19-43, 124-153; attention_cell.py:51-56)
// beam = hypotheses per image (1 for training / greedy; the B * beam decoder rows v use image v / beam).
static int attention_prepare(const Plan& P, const StepPath& sp, const float* prm, const void* wp, void* ws, int beam, hipStream_t st) {
    const int B = P.s.B, C = P.s.C, E = P.s.E, U = P.s.U, O = P.s.O;
    RC(nt(P, false, false, false, P.ws<void>(ws, W_IMG), C, P.pk(wp, K_ATT_IMG_T), C, P.ws<void>(ws, W_ATT_IMG), E,
          B * P.R, E, C, nullptr, 0, false, st));
    RC(lxo_k_rowmean(P.s.dtype, P.ws<void>(ws, W_IMG), P.ws<float>(ws, W_MEAN), B, P.R, C, st));
    float* rec0 = P.ws<float>(ws, W_REC);
    const char* wt = (const char*)P.pk(wp, K_INIT_T);
    float* mean = P.ws<float>(ws, W_MEAN);
    const InitProjs state = init_projs(P, P.ws<float>(ws, W_CS), U, rec0 + O, P.REC, rec0, P.REC);
    // beam search: compute once per image into the beam scratch, then tile over the beam (beam_search_decoder_cell.py:98-109)
    float* tmp = P.ws<float>(ws, W_BEAM_TMP);
    const InitProjs out = beam <= 1 ? state : init_projs(P, tmp, U, tmp + (size_t)B * U, U, tmp + (size_t)2 * B * U, O);
    for (const InitProj& p : out) {
        if (beam <= 1 && sp.shape == StepPath::Fused) RC(rs_dense(P, mean, C, wt + p.woff, C, p.x, p.ldx, B, p.n, C, prm + P.poff[p.bias], true, false, st));
        else RC(nt(P, true, true, true, mean, C, wt + p.woff, C, p.x, p.ldx, B, p.n, C, prm + P.poff[p.bias], 2, false, st));
    }
    for (int i = 0; i < 3 && beam > 1; ++i)
        RC(lxo_k_tile_rows(out.p[i].x, out.p[i].ldx, state.p[i].x, state.p[i].ldx, B * beam, beam, out.p[i].n, st));
    return 0;
}

// The slices one step works on.  Training: step t of rows r0.. (Train::step); decode: the two alternating state slots.
// rec_prev / cs_prev = state t-1 (o final), rec_cur / cs_cur receive state t; recb_* = the bf16 mirror of the record (null in f32)
struct Step {
    const float *zx, *rec_prev, *cs_prev; float *rec_cur, *cs_cur; const bf16_t* recb_prev; bf16_t* recb_cur;
    float *gates, *atth, *alpha;                          // gates: null in decode (not kept)
    const float* dolog; float *g, *dhc, *de, *datth, *dz; bf16_t *gb, *dzb;      // the backward's (training only; mirrors null in f32)
};

// One AttentionCell.step (attention_cell.py:58-89) for rows [r0, r0+nr) of the decoder rows.  The step's slices address row r0;
// s.zx must already hold emb_t * K[0:D] + b.  Every GEMM is a split-K slab GEMM; the kernel that consumes a product adds its slabs.
static int cell_step(const Plan& P, const float* prm, const void* wp, void* ws, int r0, int nr, int beam, const Step& s, Drop dr, hipStream_t st) {
    const int C = P.s.C, E = P.s.E, U = P.s.U, O = P.s.O;
    const size_t r = (size_t)r0;
    float* s1 = P.ws<float>(ws, W_S_K1) + r * (P.XH / 128) * 4 * U;
    float* s2 = P.ws<float>(ws, W_S_K2) + r * (U / 128) * E;
    float* s4 = P.ws<float>(ws, W_S_K4) + r * (P.HC / 128) * O;
    const char* att_img = (const char*)P.ws<void>(ws, W_ATT_IMG) + (r / beam) * P.R * E * P.esz;
    const char* img = (const char*)P.ws<void>(ws, W_IMG) + (r / beam) * P.R * C * P.esz;
    float* part = P.ws<float>(ws, W_APART) + r * 32 * (C + 2);
    // z = zx + [o_prev, h_prev] K[D:]            (attention_cell.py:70-71)
    RC(slab(P, s.rec_prev, P.REC, P.pk(wp, K_LSTM_RT), P.ldRT, s1, nr, 4 * U, P.XH, st));
    RC(lxo_k_lstm_fwd(s.zx, view(s1, P.XH, nr, 4 * U), s.cs_prev, s.gates, s.cs_cur, s.rec_cur + O, s.rec_cur + P.OFF_HT, P.REC, dr, nr, U, st));
    // att_h = h~ W                                (attention_mechanism.py:79)
    RC(slab(P, s.rec_cur + P.OFF_HT, P.REC, P.pk(wp, K_ATT_H_T), P.ldAHT, s2, nr, E, U, st));
    RC(lxo_k_attn_fwd(P.s.dtype, att_img, img, nullptr, view(s2, U, nr, E), s.atth,
                      prm + P.poff[P_BETA], s.alpha, part, s.rec_cur + P.OFF_CTX, P.REC, nullptr, 0, nr, P.R, P.Rp, E, C, beam,
                      P.attn_chunks(nr), 0, st));
    // o = tanh([h, ctx] [o_W_h; o_W_c])           (attention_cell.py:82)
    RC(slab(P, s.rec_cur + P.OFF_HT, P.REC, P.pk(wp, K_OW_T), P.ldOWT, s4, nr, O, P.HC, st));
    RC(lxo_k_tanh_finalize(view(s4, P.HC, nr, O), s.rec_cur, P.REC, dr, nr, O, st));
    return 0;
}

// The same step on the fused full-K kernels (rstep.hip): 5 dependent launches instead of 7, no split-K slabs.
// bf16 mode reads the GEMM A operands from the bf16 mirror of the record (recb_*), which every producer writes next
// to its f32 value; in the f32 parity mode the mirrors are null and A is the f32 record itself.
static int cell_step_fused(const Plan& P, const float* prm, const void* wp, void* ws, int nr, int beam, const Step& s, Drop dr, hipStream_t st,
                           const int* zx_idx = nullptr, int zx_row = -1, const int* a_par = nullptr) {
    // s.zx: training = the step's rows of emb K[0:D] + b; decode = the per-token table (zx_idx picks the row of each decoder row,
    // zx_row >= 0 = one row for all: the start token)
    const int C = P.s.C, E = P.s.E, U = P.s.U, O = P.s.O;
    const bool bf = P.bf;
    const char* att_img = (const char*)P.ws<void>(ws, W_ATT_IMG);
    const char* img = (const char*)P.ws<void>(ws, W_IMG);
    float* part = P.ws<float>(ws, W_APART);
    RStep a; memset(&a, 0, sizeof(a));
    a.M = nr; a.U = U; a.O = O; a.dr = dr; a.zx_row = -1;
    // z = zx + [o_prev, h_prev] K[D:] -> gates, c, h, h~        (attention_cell.py:70-72)
    RStep k1 = a;
    k1.A = bf ? (const void*)s.recb_prev : (const void*)s.rec_prev; k1.lda = bf ? P.RECB : P.REC;
    k1.W = P.pk(wp, K_LSTM_RT); k1.ldw = P.ldRT; k1.N = 4 * U; k1.K = P.XH; k1.epi = RS_LSTM_FWD;
    k1.zx = s.zx; k1.c_prev = s.cs_prev; k1.gates = s.gates; k1.c_out = s.cs_cur;
    k1.zx_idx = zx_idx; k1.zx_vocab = P.s.V; k1.zx_row = zx_row;
    k1.a_par = a_par; k1.a_k = beam;                         // beam decode: the previous state is read through the parents (no re-ordering launch)
    k1.out = s.rec_cur + O; k1.out2 = s.rec_cur + P.OFF_HT; k1.ldo = P.REC;
    if (bf) { k1.outb = s.recb_cur + O; k1.out2b = s.recb_cur + P.OFF_HT; k1.ldob = P.RECB; }
    RC(lxo_launch_rstep(P.s.dtype, bf, k1, st));
    // att_h = h~ W                                                (attention_mechanism.py:79)
    RStep k2 = a;
    k2.A = bf ? (const void*)(s.recb_cur + P.OFF_HT) : (const void*)(s.rec_cur + P.OFF_HT); k2.lda = bf ? P.RECB : P.REC;
    k2.W = P.pk(wp, K_ATT_H_T); k2.ldw = P.ldAHT; k2.N = E; k2.K = U; k2.epi = RS_PLAIN;
    k2.out = s.atth; k2.ldo = E;
    RC(lxo_launch_rstep(P.s.dtype, bf, k2, st));
    {
    LxoTimed tm("attn_fwd", "part+combine", (double)nr * P.R * (E + C) * P.esz, st);
    RC(lxo_k_attn_fwd(P.s.dtype, att_img, img, s.atth, kNoSlabs, nullptr,
                      prm + P.poff[P_BETA], s.alpha, part, s.rec_cur + P.OFF_CTX, P.REC, bf ? s.recb_cur + P.OFF_CTX : nullptr, P.RECB, nr, P.R, P.Rp, E, C, beam,
                      P.attn_chunks(nr), att_alternate() ? (dr.t & 1) : 0, st,
                      (!s.gates && P.att_exp()) ? P.ws<void>(ws, W_ATT_EXP) : nullptr));      // decode (no gates kept), bf16: the E-domain copy the decode set-up wrote
    }
    // o = dropout(tanh([h~, ctx] [o_W_h; o_W_c]))                  (attention_cell.py:82-83)
    RStep k4 = a;
    k4.A = bf ? (const void*)(s.recb_cur + P.OFF_HT) : (const void*)(s.rec_cur + P.OFF_HT); k4.lda = bf ? P.RECB : P.REC;
    k4.W = P.pk(wp, K_OW_T); k4.ldw = P.ldOWT; k4.N = O; k4.K = P.HC; k4.epi = RS_TANH_O;
    k4.out = s.rec_cur; k4.ldo = P.REC;
    if (bf) { k4.outb = s.recb_cur; k4.ldob = P.RECB; }
    RC(lxo_launch_rstep(P.s.dtype, bf, k4, st));
    return 0;
}
// bf16 mirror of the [o | h] columns of `rows` records (initial state; beam re-ordering)
static int mirror_oh(const Plan& P, void* ws, size_t slot_rows, int rows, hipStream_t st) {
    if (!P.bf) return 0;
    return lxo_k_mirror(P.ws<float>(ws, W_REC) + slot_rows * P.REC, P.REC, P.ws<bf16_t>(ws, W_RECB) + slot_rows * P.RECB, P.RECB, rows, P.XH, st);
}
// What the forward chain and the greedy-decode chain (XDecFwd, XDecDec) share: the recurrent weights, the image side, the record and
// the forward chain's block of the sync region
template <class X>
static void xdec_common(X& x, const Plan& P, const float* prm, const void* wp, void* ws) {
    x.Wrt = (const bf16_t*)P.pk(wp, K_LSTM_RT); x.ldrt = P.ldRT;
    x.Wah = (const bf16_t*)P.pk(wp, K_ATT_H_T); x.ldah = P.ldAHT;
    x.Wow = (const bf16_t*)P.pk(wp, K_OW_T); x.ldow = P.ldOWT;
    x.beta = prm + P.poff[P_BETA];
    x.img = P.ws<bf16_t>(ws, W_IMG);
    x.att_exp = P.att_exp() ? P.ws<bf16_t>(ws, W_ATT_EXP) : nullptr;
    x.rec = P.ws<float>(ws, W_REC); x.recb = P.ws<bf16_t>(ws, W_RECB); x.cs = P.ws<float>(ws, W_CS);
    x.part = P.ws<float>(ws, W_APART); x.sync = chain_block(P, ws, kChainFwd);
    x.B = P.s.B; x.R = P.R; x.REC = P.REC; x.RECB = P.RECB;
}

// ------------------------------------------------------------------ training ----
// What the stages of one training call share, fetched once: the call's arguments, its step path and the workspace regions of the recurrence
struct Train {
    const Plan& P; const float* prm; const void* wp; void* ws; hipStream_t st;
    StepPath sp;
    float *zx, *rec, *cs, *gates, *atth, *alpha; bf16_t* recb;                       // forward: [T][B][.] per step, rec / cs [(T + 1)][B][.]
    float *dolog, *g, *dhc, *de, *datth, *dz, *dcc, *dxh; bf16_t *gb, *dzb;          // backward (the bf16 mirrors: null in f32)
    // step t of rows r0..: the rows of its inputs and of state t-1, and the rows of state t
    Step step(int t, int r0 = 0) const {
        const int B = P.s.B, U = P.s.U, O = P.s.O, E = P.s.E;
        const size_t p = (size_t)t * B + r0, c = p + B;
        Step s;
        s.zx = zx + p * 4 * U; s.rec_prev = rec + p * P.REC; s.cs_prev = cs + p * U; s.rec_cur = rec + c * P.REC; s.cs_cur = cs + c * U;
        s.recb_prev = recb ? recb + p * P.RECB : nullptr; s.recb_cur = recb ? recb + c * P.RECB : nullptr;
        s.gates = gates + p * 4 * U; s.atth = atth + p * E; s.alpha = alpha + p * P.Rp;
        s.dolog = dolog + p * O; s.g = g + p * O; s.dhc = dhc + p * P.HC; s.de = de + p * P.Rp; s.datth = datth + p * E; s.dz = dz + p * 4 * U;
        s.gb = gb ? gb + p * P.GBP : nullptr; s.dzb = dzb ? dzb + p * P.DZBP : nullptr;
        return s;
    }
};
static Train train_of(const Plan& P, const float* prm, const void* wp, void* ws, hipStream_t st) {
    Train w = {P, prm, wp, ws, st, step_path(P, true),
               P.ws<float>(ws, W_ZX), P.ws<float>(ws, W_REC), P.ws<float>(ws, W_CS), P.ws<float>(ws, W_GATES), P.ws<float>(ws, W_ATTH),
               P.ws<float>(ws, W_ALPHA), P.bf ? P.ws<bf16_t>(ws, W_RECB) : nullptr,
               P.ws<float>(ws, W_DOLOG), P.ws<float>(ws, W_G), P.ws<float>(ws, W_DHC), P.ws<float>(ws, W_DE), P.ws<float>(ws, W_DATTH),
               P.ws<float>(ws, W_DZ), P.ws<float>(ws, W_DCC), P.ws<float>(ws, W_DXH),
               P.bf ? P.ws<bf16_t>(ws, W_GB) : nullptr, P.bf ? P.ws<bf16_t>(ws, W_DZB) : nullptr};
    return w;
}

// attention, E_x, the embedding gather and zx = emb K[0:D] + b for every step at once
static int fwd_setup(const Train& w, const int* formula) {
    const Plan& P = w.P; void* ws = w.ws; hipStream_t st = w.st;
    const int B = P.s.B, T = P.s.T, U = P.s.U, D = P.s.D, V = P.s.V;
    RC(attention_prepare(P, w.sp, w.prm, w.wp, ws, 1, st));
    if (P.att_exp()) RC(lxo_k_att_exp(P.ws<void>(ws, W_ATT_IMG), P.ws<void>(ws, W_ATT_EXP), (long long)B * P.R * P.s.E, st));     // E_x = e^{2 att_img}: what the recurrence's attention kernels read
    RC(lxo_k_embed_gather(P.s.dtype, w.prm + P.poff[P_EMB], w.prm + P.poff[P_START], formula, P.ws<void>(ws, W_EMB_IN), B, T, D, P.Dp, V, st));
    return nt(P, false, true, false, P.ws<void>(ws, W_EMB_IN), P.Dp, P.pk(w.wp, K_LSTM_XT), P.Dp, w.zx, 4 * U, T * B, 4 * U, P.Dp,
              w.prm + P.poff[P_LSTM_B], 0, false, st);
}
// the whole recurrence in one launch: 8 XCD-local chains of B / 8 samples (xdec.hip).  *ran stays false where the shape does not qualify (-2).
// lengths (device, [B], nullable): the chain streams nothing for the steps behind a row's end (XDecFwd.lengths)
static int fwd_chain(const Train& w, const int* lengths, bool* ran) {
    const Plan& P = w.P; void* ws = w.ws;
    RC(mirror_oh(P, ws, 0, P.s.B, w.st));
    XDecFwd x; memset(&x, 0, sizeof(x));
    xdec_common(x, P, w.prm, w.wp, ws);
    x.att_img = P.ws<bf16_t>(ws, W_ATT_IMG);
    x.zx = w.zx; x.gates = w.gates; x.atth = w.atth; x.alpha = w.alpha;
    x.T = P.s.T; x.Rp = P.Rp;
    x.dr = P.drop(0, 0);
    x.lengths = lengths;
    LxoTimed tm("xdec_fwd", "chain", (double)P.s.T * P.s.B * P.R * (P.s.E + P.s.C) * P.esz, w.st);
    const int rc = lxo_launch_xdec_fwd(x, P.s.U, P.s.O, P.s.C, P.s.E, w.st);
    if (rc == 0) *ran = true;
    else if (rc != -2) return rc < 0 ? rc : -rc;
    return 0;
}
static int fwd_fused_loop(const Train& w) {
    const Plan& P = w.P;
    RC(mirror_oh(P, w.ws, 0, P.s.B, w.st));
    for (int t = 0; t < P.s.T; ++t) RC(cell_step_fused(P, w.prm, w.wp, w.ws, P.s.B, 1, w.step(t), P.drop(t, 0), w.st));
    return 0;
}
// round 1's kernels; under `dual` the second half of the batch runs on the side stream
static int fwd_splitk_loop(const Train& w) {
    const Plan& P = w.P;
    const int nh = w.sp.dual ? 2 : 1, hb = P.s.B / nh;
    if (w.sp.dual) RC(fork_side(w.st));
    for (int t = 0; t < P.s.T; ++t)
        for (int h = 0; h < nh; ++h)
            RC(cell_step(P, w.prm, w.wp, w.ws, h * hb, hb, 1, w.step(t, h * hb), P.drop(t, h * hb), h ? g_side : w.st));
    if (w.sp.dual) RC(join_side(w.st));
    return 0;
}
// logits_t = o_t y_W_o for every step at once  (attention_cell.py:84)
static int fwd_logits(const Train& w) {
    const Plan& P = w.P;
    const bool m = w.sp.mirrors;      // A = the bf16 mirror of o_t the step kernels wrote next to the f32 record, where there is one
    return nt(P, !m, true, false, m ? (const void*)w.step(0).recb_cur : (const void*)w.step(0).rec_cur, m ? P.RECB : P.REC, P.pk(w.wp, K_YWO_T), P.s.O,
              P.ws<float>(w.ws, W_LOGITS), P.Vp, P.s.T * P.s.B, P.s.V, P.s.O, nullptr, 0, false, w.st);
}

// All B rows run all T steps, padded ones included, as the reference does (decoder.py:57: dynamic_rnn without sequence_length; the padded
// steps are masked in the loss, img2seq.py:68-71).  One stream, but for the split-K loop's second half-batch under `dual`.
// lengths (lxo_decoder_train_fwd_live; null: none): only the persistent chain reads them -- the loops compute every position as before.
int lxo_impl_decoder_train_fwd(const Plan& P, const float* prm, const void* wp, void* ws, const int* formula, hipStream_t st, const int* lengths) {
    const Train w = train_of(P, prm, wp, ws, st);
    RC(fwd_setup(w, formula));
    bool chain = false;
    if (w.sp.try_chain) RC(fwd_chain(w, lengths, &chain));
    // no chain in this call: clear its tickets and its error word (the loss kernel and lxo_chain_guard read it; a reused workspace may hold another shape's bytes here)
    if (P.bf && !chain) HIPRC(hipMemsetAsync(chain_block(P, ws, kChainFwd), 0, kXDecSyncBytes, st));
    if (w.sp.loop == StepPath::SplitK) RC(fwd_splitk_loop(w));
    else if (!chain) RC(fwd_fused_loop(w));
    return fwd_logits(w);
}

// w_tok / w_row (lxo_ce_loss_weighted; both NULL: the unweighted loss): ws region "loss" then holds {sum w CE, token count, sum w, sum CE}
// smooth_eps (lxo_ce_loss_smoothed; NULL: one-hot targets): *smooth_eps in [0, 1) is the label smoothing, the region then {sum w L, token count, sum w,
// sum CE (plain)} with or without weights
// soft (lxo_ce_loss_soft; NULL: none; needs smooth_eps): the teacher's slots and lambda; lambda == 0 is the smoothed call, and takes it
int lxo_impl_ce_loss(const Plan& P, void* ws, const int* formula, const int* lengths, float inv_ntok, const float* ntok_dev, hipStream_t st,
                     const float* w_tok, const float* w_row, const float* smooth_eps, const CeSoft* soft) {
    HIPRC(hipMemsetAsync(P.ws<float>(ws, W_LOSS), 0, 64, st));
    const CeWeights wt = {w_tok, w_row};
    const CeSmooth sm = {smooth_eps ? *smooth_eps : 0.f, smooth_eps ? *smooth_eps / (float)P.s.V : 0.f};      // eps_v: ONE f32 division
    RC(lxo_k_ce_loss(P.s.dtype, P.ws<float>(ws, W_LOGITS), formula, lengths, P.ws<void>(ws, W_DLOGITS), P.ws<float>(ws, W_LOSS),
                     inv_ntok, ntok_dev, chain_err(P, ws, kChainFwd), P.s.B, P.s.T, P.s.V, P.Vp,
                     DetScratch{P.ws<float>(ws, W_DET), P.wbytes[W_DET] / 4}, st,      // every mode: per-workgroup partial statistics added in order (25 us; the atomic form measured 53)
                     (w_tok || w_row) ? &wt : nullptr, smooth_eps ? &sm : nullptr, (soft && soft->lambda != 0.f) ? soft : nullptr));
    return 0;
}

// teacher-forced scoring of the formula the last lxo_decoder_train_fwd ran: reads ws region "logits" (and the forward chain's error word),
// writes the caller's outputs only
int lxo_impl_score_tokens(const Plan& P, void* ws, const int* formula, const int* lengths, float* logp_out, int* top1_out, float* seq_out, hipStream_t st) {
    return lxo_k_score(P.s.dtype, P.ws<float>(ws, W_LOGITS), formula, lengths, logp_out, top1_out, seq_out,
                       chain_err(P, ws, kChainFwd), P.s.B, P.s.T, P.s.V, P.Vp, st);
}

// ... and the alternatives at every position of the same logits (no workspace region of its own)
int lxo_impl_score_alternatives(const Plan& P, void* ws, const int* formula, const int* lengths, int k, const DecAllow* allow, int* ids_out, float* logp_out,
                                int* rank_out, float* ent_out, hipStream_t st) {
    return lxo_k_score_alt(P.s.dtype, P.ws<float>(ws, W_LOGITS), formula, lengths, k, allow, ids_out, logp_out, rank_out, ent_out,
                           chain_err(P, ws, kChainFwd), P.s.B, P.s.T, P.s.V, P.Vp, st);
}

// The weight-gradient side stream of the encoder backward (model_encoder.hip: lxo_set_encoder_side_stream) also takes the decoder's
// deferred work (round 5): behind the recurrence the critical path is d_att_img (bound by the transcendental rate) -> d_img -> conv6;
// the initial-state gradients, the dense dW GEMMs, d_z's column sum and dW_att_img feed nothing downstream but d_mean, and run
// beside it.  The embedding gradient feeds nothing either, but follows d_img on the MAIN stream: from here to the end of the step the side
// stream (deferred GEMMs, then the encoder's five weight gradients) is the longer one, and the main stream stops for it before it may
// rewrite a gradient buffer (profiles/datt_img_live_steps.txt: 0.10 ms per step together with the shorter d_att_img pass, nothing alone).
// Enqueue order top to bottom, an arrow = an event recorded at its tail and waited for at its head:
//      main stream: recurrence                            side stream
//      fork ----------------------------------------->    initial states: d_pre, d_mean
//      d_att_img (masked d_img) / alpha (x) d_ctx    .--  dmean_ready
//      wait_dmean  <---------------------------------'    dW, db of the initial states; deferred dW GEMMs; d_z column sum
//      d_img's readers of d_mean
//      embedding gradient
//      datt_img_ready (masked form: recorded right behind d_att_img, before wait_dmean; plain form: d_att_img runs here, behind d_mean's readers)
//             `-------------------------------------->    wait_datt_img: dW_att_img
//      join  <----------------------------------------    (none under defer_join: lxo_impl_encoder_bwd follows on both streams and joins them once)
//      backward-chain poison
//      record_ready: a second fork ------------------>    `ready` recorded, behind both streams' work
// Without a side stream (f32, the split-K kernels, a timed run) everything runs on the main stream in this order and every operation
// but record_ready is a no-op.
hipStream_t lxo_impl_encoder_side_stream();
static thread_local hipEvent_t g_dbw_fork = nullptr, g_dbw_fork2 = nullptr, g_dbw_join = nullptr, g_dbw_init = nullptr;
struct BwdStreams {
    hipStream_t main, side;
    hipStream_t deferred() const { return side ? side : main; }      // the stream of the work nothing downstream waits for
    int fork() const {
        if (!side) return 0;
        if (!g_dbw_fork) for (hipEvent_t* e : {&g_dbw_fork, &g_dbw_fork2, &g_dbw_join, &g_dbw_init}) HIPRC(hipEventCreateWithFlags(e, hipEventDisableTiming));
        HIPRC(hipEventRecord(g_dbw_fork, main));
        HIPRC(hipStreamWaitEvent(side, g_dbw_fork, 0));
        return 0;
    }
    int dmean_ready() const { if (side) HIPRC(hipEventRecord(g_dbw_init, side)); return 0; }      // d_mean is complete: the main stream's d_img waits for THIS, not for the six small launches behind it
    int wait_dmean() const { if (side) HIPRC(hipStreamWaitEvent(main, g_dbw_init, 0)); return 0; }
    int datt_img_ready() const { if (side) HIPRC(hipEventRecord(g_dbw_fork2, main)); return 0; }
    int wait_datt_img() const { if (side) HIPRC(hipStreamWaitEvent(side, g_dbw_fork2, 0)); return 0; }      // dW_att_img needs d_att_img, nothing needs dW_att_img
    int join(bool defer) const {
        if (!side || defer) return 0;
        HIPRC(hipEventRecord(g_dbw_join, side));
        HIPRC(hipStreamWaitEvent(main, g_dbw_join, 0));
        return 0;
    }
    // `ready`: every decoder gradient (and the probe element) is final -- recorded on the side stream behind both streams' work when
    // one is in use, so that a communication stream can wait for it without the main stream stopping
    int record_ready(void* ready) const {
        if (!ready) return 0;
        if (side) { HIPRC(hipEventRecord(g_dbw_fork, main)); HIPRC(hipStreamWaitEvent(side, g_dbw_fork, 0)); }
        HIPRC(hipEventRecord((hipEvent_t)ready, deferred()));
        return 0;
    }
};

// d_o (from logits) for every step, and dy_W_o
static int bwd_logits(const Train& w, float* grads) {
    const Plan& P = w.P; hipStream_t st = w.st;
    const int B = P.s.B, TB = P.s.T * B, O = P.s.O, V = P.s.V;
    const void* dlog = P.ws<void>(w.ws, W_DLOGITS);
    RC(nt(P, false, true, false, dlog, P.Vp, P.pk(w.wp, K_YWO), P.Vp, w.dolog, O, TB, O, P.Vp, nullptr, 0, false, st));
    if (w.sp.mirrors) RC(tn(P, false, false, w.step(0).recb_cur, P.RECB, dlog, P.Vp, grads + P.poff[P_YWO], V, TB, O, V, st, P.det_scratch(w.ws)));
    else RC(tn(P, true, false, w.step(0).rec_cur, P.REC, dlog, P.Vp, grads + P.poff[P_YWO], V, TB, O, V, st));
    // a failed forward chain poisons the last gradient element (y_W_o's, final after this part): under data parallelism its all-reduce
    // carries the failure to every rank (lxo_chain_guard)
    if (P.bf) RC(lxo_k_chain_poison(chain_err(P, w.ws, kChainFwd), nullptr, grads + P.ptotal - 1, st));
    return 0;
}
// the launch-per-step kernels accumulate d_c in place and d_att_h with atomics; the backward chain writes both with plain stores
static int bwd_zero_acc(const Train& w) {
    HIPRC(hipMemsetAsync(w.dcc, 0, (size_t)w.P.s.B * w.P.s.U * 4, w.st));
    HIPRC(hipMemsetAsync(w.datth, 0, (size_t)w.P.s.T * w.P.s.B * w.P.s.E * 4, w.st));
    return 0;
}
// g_{T-1} = d_o(logits) * tanh'   (no carry yet): what the chain and the fused loop start from
static int bwd_last_g(const Train& w) {
    const Plan& P = w.P;
    const Step l = w.step(P.s.T - 1);
    return lxo_k_tanh_bwd(l.dolog, P.s.O, kNoSlabs, l.rec_cur, P.REC, l.g, P.s.O, l.gb, P.GBP, P.drop(P.s.T - 1, 0), 0, P.s.B, P.s.O, w.st);
}
// the whole recurrence in one launch (xdec.hip, the backward chain).  *ran stays false where the shape does not qualify (-2)
static int bwd_chain(const Train& w, bool* ran) {
    const Plan& P = w.P; void* ws = w.ws; const void* wp = w.wp;
    XDecBwd x; memset(&x, 0, sizeof(x));
    x.Wow = (const bf16_t*)P.pk(wp, K_OW); x.ldow = P.ldOW;
    x.Wah = (const bf16_t*)P.pk(wp, K_ATT_H); x.ldah = P.ldAH;
    x.Wk = (const bf16_t*)P.pk(wp, K_LSTM) + (size_t)P.s.D * P.ldK; x.ldk = P.ldK;
    x.beta = w.prm + P.poff[P_BETA];
    x.att_img = P.ws<bf16_t>(ws, W_ATT_IMG); x.img = P.ws<bf16_t>(ws, W_IMG);
    x.att_exp = P.att_exp() ? P.ws<bf16_t>(ws, W_ATT_EXP) : nullptr;
    x.rec = w.rec; x.REC = P.REC; x.cs = w.cs; x.gates = w.gates; x.atth = w.atth; x.alpha = w.alpha; x.Rp = P.Rp;
    x.dolog = w.dolog; x.gall = w.g; x.gb = w.gb; x.GBP = P.GBP; x.dhc = w.dhc; x.de = w.de; x.datth = w.datth; x.datthb = P.ws<bf16_t>(ws, W_DATTHB);
    x.dz = w.dz; x.dzb = w.dzb; x.DZBP = P.DZBP; x.carry_h = P.ws<float>(ws, W_CARRYH); x.dcc = w.dcc; x.dxh = w.dxh;
    x.part = P.ws<float>(ws, W_APART);                       // the forward chain's chunk partials are dead by now
    x.sync = chain_block(P, ws, kChainBwd);                  // its own block
    x.T = P.s.T; x.B = P.s.B; x.R = P.R;
    x.dr = P.drop(0, 0);
    LxoTimed tm("xdec_bwd", "chain", (double)P.s.T * P.s.B * P.R * (P.s.E + P.s.C) * P.esz, w.st);
    const int rc = lxo_launch_xdec_bwd(x, P.s.U, P.s.O, P.s.C, P.s.E, w.st);
    if (rc == 0) *ran = true;
    else if (rc != -2) return rc < 0 ? rc : -rc;
    else { RC(bwd_zero_acc(w)); HIPRC(hipMemsetAsync(x.sync, 0, kXDecSyncBytes, w.st)); }      // the shape does not qualify: no tickets, no error
    return 0;
}
// 4 dependent launches per step: [d_h~|d_ctx] GEMM, attention backward, d_att_h GEMM + LSTM backward,
// d_z K^T GEMM + the tanh' of step t-1.  All operands are final values (no split-K slabs).
static int bwd_fused_loop(const Train& w) {
    const Plan& P = w.P; void* ws = w.ws; const void* wp = w.wp; hipStream_t st = w.st;
    const int B = P.s.B, T = P.s.T, C = P.s.C, E = P.s.E, U = P.s.U, O = P.s.O;
    const bool bf = P.bf;
    float* carry_h = P.ws<float>(ws, W_CARRYH);
    const int nchb = attn_bwd_chunks(P, B);
    RStep a; memset(&a, 0, sizeof(a));
    a.U = U; a.O = O; a.zx_row = -1; a.M = B;
    for (int t = T - 1; t >= 0; --t) {
        const Step s = w.step(t);
        // [d_h~ | d_ctx] = g [o_W_h; o_W_c]^T
        RStep b1 = a;
        b1.A = bf ? (const void*)s.gb : (const void*)s.g; b1.lda = bf ? P.GBP : O;
        b1.W = P.pk(wp, K_OW); b1.ldw = P.ldOW; b1.N = P.HC; b1.K = O; b1.epi = RS_PLAIN;
        b1.out = s.dhc; b1.ldo = P.HC;
        RC(lxo_launch_rstep(P.s.dtype, bf, b1, st));
        const Slabs dc1 = {s.dhc, 1, 0, P.HC};
        {
        LxoTimed tm("attn_bwd", "part", (double)B * P.R * (E + C) * P.esz, st);
        RC(lxo_k_attn_bwd(P.s.dtype, P.ws<void>(ws, W_ATT_IMG), P.att_exp() ? P.ws<void>(ws, W_ATT_EXP) : nullptr, P.ws<void>(ws, W_IMG), s.atth, w.prm + P.poff[P_BETA],
                          s.alpha, dc1, U, nullptr, P.HC, s.rec_cur + P.OFF_CTX, P.REC,
                          s.de, s.datth, B, P.R, P.Rp, E, C, nchb, att_alternate() ? (t & 1) : 0, st));
        }
        // d_h = (d_h~(o projection) + d_att_h W_att_h^T) * mask + carry -> d_z, d_c
        RStep b3 = a;
        b3.A = s.datth; b3.lda = E;                                  // f32 (atomically accumulated), converted on load
        b3.W = P.pk(wp, K_ATT_H); b3.ldw = P.ldAH; b3.N = U; b3.K = E; b3.epi = RS_LSTM_BWD;
        b3.dhm = s.dhc; b3.lddhm = P.HC; b3.carry_h = carry_h; b3.carry_rows = (t == T - 1) ? 0 : B;
        b3.gates_in = s.gates; b3.c_prev = s.cs_prev; b3.c_cur = s.cs_cur;
        b3.dcc = w.dcc; b3.out = s.dz; b3.outb = s.dzb; b3.ldob = P.DZBP; b3.dr = P.drop(t, 0);
        RC(lxo_launch_rstep(P.s.dtype, 0, b3, st));
        // [d_o carry | d_h carry] = d_z K[D:]^T ; g_{t-1} = (d_o(logits) + d_o carry) * tanh'
        RStep b4 = a;
        b4.A = bf ? (const void*)s.dzb : (const void*)s.dz; b4.lda = bf ? P.DZBP : 4 * U;
        b4.W = (const char*)P.pk(wp, K_LSTM) + (size_t)P.s.D * P.ldK * P.esz; b4.ldw = P.ldK; b4.N = P.XH; b4.K = 4 * U; b4.epi = RS_CARRY;
        if (t == 0) { b4.first = 1; b4.out = w.dxh; b4.ldo = P.XH; }
        else {
            const Step q = w.step(t - 1);
            b4.out = q.g; b4.outb = q.gb; b4.ldob = P.GBP; b4.out2 = carry_h;
            b4.dolog = q.dolog; b4.o_prev = s.rec_prev; b4.ldoprev = P.REC;
            b4.dr = P.drop(t - 1, 0);
        }
        RC(lxo_launch_rstep(P.s.dtype, bf, b4, st));
    }
    return 0;
}
// round 1's kernels (under `dual` the second half of the batch on the side stream), then the final carries: the halves' are separate
// slab sets, gathered into one [B][XH] buffer
static int bwd_splitk_loop(const Train& w) {
    const Plan& P = w.P; void* ws = w.ws; const void* wp = w.wp;
    const int T = P.s.T, C = P.s.C, E = P.s.E, U = P.s.U, O = P.s.O;
    const int nh = w.sp.dual ? 2 : 1, hb = P.s.B / nh;
    const int nchb = attn_bwd_chunks(P, hb);
    auto sb4_of = [&](size_t r0) { return P.ws<float>(ws, W_S_B4) + r0 * (4 * U / 128) * P.XH; };
    if (w.sp.dual) RC(fork_side(w.st));
    for (int t = T - 1; t >= 0; --t) {
        for (int h = 0; h < nh; ++h) {
            // rows that also ran step t+1 receive its carries; the others end here (their later steps were skipped)
            const int crows = (t == T - 1) ? 0 : hb;
            hipStream_t sh = h ? g_side : w.st;
            const size_t r0 = (size_t)h * hb;
            const Step s = w.step(t, (int)r0);
            float* sb1 = P.ws<float>(ws, W_S_B1) + r0 * (O / 128) * P.HC;
            float* sb3 = P.ws<float>(ws, W_S_B3) + r0 * (E / 128) * U;
            float* sb4 = sb4_of(r0);
            const char* att_img = (const char*)P.ws<void>(ws, W_ATT_IMG) + r0 * P.R * E * P.esz;
            const char* img = (const char*)P.ws<void>(ws, W_IMG) + r0 * P.R * C * P.esz;
            // carry [d_o | d_h] from step t+1 = the B4 slabs of the previous iteration (none at t = T-1)
            const Slabs carry = (crows <= 0) ? kNoSlabs : view(sb4, 4 * U, crows, P.XH);
            // g = (d_o_logits + d_o_carry) * (1 - o^2)
            const Drop dr = P.drop(t, (int)r0);
            RC(lxo_k_tanh_bwd(s.dolog, O, carry, s.rec_cur, P.REC, s.g, O, nullptr, 0, dr, crows, hb, O, sh));
            // [d_h~ | d_ctx] = g [o_W_h; o_W_c]^T
            RC(slab(P, s.g, O, P.pk(wp, K_OW), P.ldOW, sb1, hb, P.HC, O, sh));
            RC(lxo_k_attn_bwd(P.s.dtype, att_img, P.att_exp() ? (const char*)P.ws<void>(ws, W_ATT_EXP) + r0 * P.R * E * P.esz : nullptr, img, s.atth, w.prm + P.poff[P_BETA],
                              s.alpha, view(sb1, O, hb, P.HC), U, s.dhc + U, P.HC, s.rec_cur + P.OFF_CTX, P.REC,
                              s.de, s.datth, hb, P.R, P.Rp, E, C, nchb, 0, sh));
            // d_h += d_att_h W_att_h^T
            RC(slab(P, s.datth, E, P.pk(wp, K_ATT_H), P.ldAH, sb3, hb, U, E, sh));
            RC(lxo_k_lstm_bwd(s.gates, s.cs_prev, s.cs_cur, view(sb1, O, hb, P.HC), view(sb3, E, hb, U), carry, O, w.dcc + r0 * U, s.dz, dr, crows, hb, U, sh));
            // [d_o carry | d_h carry] = d_z K[D:]^T
            RC(slab(P, s.dz, 4 * U, (const char*)P.pk(wp, K_LSTM) + (size_t)P.s.D * P.ldK * P.esz, P.ldK, sb4, hb, P.XH, 4 * U, sh));
        }
    }
    if (w.sp.dual) RC(join_side(w.st));
    for (int h = 0; h < nh; ++h) {
        const size_t r0 = (size_t)h * hb;
        RC(lxo_k_slab_reduce(view(sb4_of(r0), 4 * U, hb, P.XH), w.dxh + r0 * P.XH, P.XH, hb, P.XH, w.st));
    }
    return 0;
}
// initial states: d_pre, then d_mean (which d_img needs: first, and announced before the projections' own weight gradients)
static int bwd_init_states(const Train& w, float* grads, const BwdStreams& s, DetScratch det_s) {
    const Plan& P = w.P; void* ws = w.ws;
    const int B = P.s.B, C = P.s.C, U = P.s.U, O = P.s.O, W3 = 2 * U + O;
    hipStream_t sd = s.deferred();
    float* dpre = P.ws<float>(ws, W_DPRE0); float* mean = P.ws<float>(ws, W_MEAN); float* dmean = P.ws<float>(ws, W_DMEAN);
    { const Slabs one = {w.dxh, 1, 0, P.XH}; RC(lxo_k_init_bwd(w.dcc, one, w.cs, w.rec, P.REC, dpre, B, U, O, sd)); }
    const char* wi = (const char*)P.pk(w.wp, K_INIT);
    const InitProjs pr = init_projs(P, dpre, W3, dpre + U, W3, dpre + 2 * U, W3);
    for (const InitProj& p : pr) {
        const bool acc = &p != pr.p;
        if (w.sp.shape == StepPath::Fused) RC(rs_dense(P, p.x, W3, wi + p.woff, p.n, dmean, C, B, C, p.n, nullptr, false, acc, sd));
        else RC(nt(P, true, true, true, p.x, W3, wi + p.woff, p.n, dmean, C, B, C, p.n, nullptr, 0, acc, sd));
    }
    RC(s.dmean_ready());
    for (const InitProj& p : pr) RC(tn(P, true, true, mean, C, p.x, W3, grads + P.poff[p.weight], p.n, B, C, p.n, sd));
    for (const InitProj& p : pr) RC(lxo_k_colsum(p.x, W3, grads + P.poff[p.bias], B, p.n, det_s, sd));
    return 0;
}
// the deferred weight gradients over all steps: d[o_W_h; o_W_c], dW_att_h, dK in two row ranges, d_b
static int bwd_weight_grads(const Train& w, float* grads, bool bwd_chain_ran, const BwdStreams& s, DetScratch det_s) {
    const Plan& P = w.P; void* ws = w.ws; hipStream_t st = w.st, sd = s.deferred();
    const int TB = P.s.T * P.s.B, E = P.s.E, U = P.s.U, O = P.s.O, D = P.s.D;
    auto gw = [&](int pid) { return grads + P.poff[pid]; };
    // bf16 on the fused kernels: the bf16 mirrors they left (record, g_t, d_z_t) are the operands: half the bytes of the f32 originals, and
    // these reductions over T*B rows are bound by operand re-reads (every 128 x 128 tile walks all rows of both operands).  They then
    // run on the deferred stream with its ordered-partials scratch; otherwise f32 operands on the main stream
    const bool m = w.sp.mirrors, f = !m;
    const Step s0 = w.step(0);      // the operands over all T*B rows start at step 0's slices: the states 0 .. T-1 are the [o | h] inputs, the states 1 .. T hold [h~ | ctx]
    const void* rec = m ? (const void*)w.recb : (const void*)w.rec; const int ldr = m ? P.RECB : P.REC;
    const void* hc = m ? (const void*)(s0.recb_cur + P.OFF_HT) : (const void*)(s0.rec_cur + P.OFF_HT);
    const void* g = m ? (const void*)w.gb : (const void*)w.g; const int ldg = m ? P.GBP : O;
    const void* dz = m ? (const void*)w.dzb : (const void*)w.dz; const int ldz = m ? P.DZBP : 4 * U;
    hipStream_t sx = m ? sd : st;
    const DetScratch dx = m ? det_s : DetScratch{nullptr, 0};
    RC(tn(P, f, f, hc, ldr, g, ldg, gw(P_OWH), O, TB, P.HC, O, sx, dx));                                              // d[o_W_h; o_W_c]
    if (bwd_chain_ran) RC(tn(P, f, false, hc, ldr, P.ws<bf16_t>(ws, W_DATTHB), E, gw(P_ATT_H), E, TB, U, E, sx, dx));  // dW_att_h: the chain left the bf16 mirror of d_att_h
    else RC(tn(P, f, true, hc, ldr, w.datth, E, gw(P_ATT_H), E, TB, U, E, sx));
    RC(tn(P, false, f, P.ws<void>(ws, W_EMB_IN), P.Dp, dz, ldz, gw(P_LSTM_K), 4 * U, TB, D, 4 * U, sx, dx));           // dK rows 0..D
    RC(tn(P, f, f, rec, ldr, dz, ldz, gw(P_LSTM_K) + (size_t)D * 4 * U, 4 * U, TB, P.XH, 4 * U, sx, dx));              // dK rows D..
    return lxo_k_colsum(w.dz, 4 * U, gw(P_LSTM_B), TB, 4 * U, det_s, sd);
}
static int bwd_embedding(const Train& w, const int* formula, float* grads, const BwdStreams& s) {
    const Plan& P = w.P; hipStream_t sd = s.deferred();
    const int B = P.s.B, T = P.s.T, TB = T * B, U = P.s.U, D = P.s.D;
    float* demb = P.ws<float>(w.ws, W_DEMB);
    if (w.sp.loop == StepPath::Fused) {   // d_emb = d_z K[0:D]^T over all T*B rows: a tall GEMM on the step kernel (505 workgroups; the bf16 mirror of d_z halves its bytes)
        RStep e; memset(&e, 0, sizeof(e));
        e.M = TB; e.N = D; e.K = 4 * U; e.U = U; e.O = P.s.O; e.zx_row = -1; e.epi = RS_PLAIN; e.dr.inv_keep = 1.f;
        e.A = P.bf ? (const void*)w.dzb : (const void*)w.dz; e.lda = P.bf ? P.DZBP : 4 * U;
        e.W = P.pk(w.wp, K_LSTM); e.ldw = P.ldK; e.out = demb; e.ldo = D;
        RC(lxo_launch_rstep(P.s.dtype, P.bf, e, sd));
    } else
        RC(nt(P, true, true, true, w.dz, 4 * U, P.pk(w.wp, K_LSTM), P.ldK, demb, D, TB, D, 4 * U, nullptr, 0, false, w.st));
    return lxo_k_embed_scatter(demb, formula, grads + P.poff[P_EMB], grads + P.poff[P_START], B, T, D, P.s.V, P.det() ? 1 : 0, sd);
}
// d_att_img = the attention's gradient w.r.t. the projected image, all steps (+ d_beta)
static int bwd_datt_img(const Train& w, float* grads) {
    const Plan& P = w.P;
    return lxo_k_datt_img(P.s.dtype, P.ws<void>(w.ws, W_ATT_IMG), w.atth, w.prm + P.poff[P_BETA], w.de, P.ws<void>(w.ws, W_DATTIMG), grads + P.poff[P_BETA],
                          P.s.T, P.s.B, P.R, P.Rp, P.s.E, P.wbytes[W_ATTH_EXP] ? P.ws<float>(w.ws, W_ATTH_EXP) : nullptr, P.det_scratch(w.ws), w.st);
}
// d_img = sum_t alpha_t (x) d_ctx_t  (batched over samples)  + d_mean / R + d_att_img W_att_img^T, masked form:
// one batched GEMM contracts both products, adds the mean gradient and applies conv6's ReLU mask + bias-gradient sum
// in its epilogue (dimg.hip): region "d_img" receives d_y6 in the compute dtype, lxo_encoder_bwd skips its mask pass
static int bwd_dimg_masked(const Train& w, float* grads, const BwdStreams& s) {
    const Plan& P = w.P; void* ws = w.ws;
    const int B = P.s.B;
    const DetScratch det = P.det_scratch(ws);
    RC(bwd_datt_img(w, grads));
    RC(s.datt_img_ready());
    RC(s.wait_dmean());
    DimgArgs a; memset(&a, 0, sizeof(a));
    a.alpha = w.alpha; a.ld_alpha = (long long)B * P.Rp; a.Rp = P.Rp;
    a.dctx = w.dhc + P.s.U; a.ld_dctx = (long long)B * P.HC; a.HC = P.HC;
    a.datt = P.ws<bf16_t>(ws, W_DATTIMG); a.W = (const bf16_t*)P.pk(w.wp, K_ATT_IMG); a.ldw = P.s.E;
    a.dmean = P.ws<float>(ws, W_DMEAN); a.T = P.s.T; a.B = B; a.R = P.R; a.C = P.s.C; a.E = P.s.E;
    a.y6 = P.ws<bf16_t>(ws, W_Y6); a.dy6 = P.ws<bf16_t>(ws, W_DIMG); a.db = grads + P.poff[P_CONV6_B];
    if (P.det()) { a.db_part = det.p; a.db_part_floats = det.floats; }      // deterministic mode: per-workgroup slots, added in order
    return lxo_launch_dimg_fused(a, w.st);
}
// ... and the plain form: the three terms one after the other into the f32 region "d_img"
static int bwd_dimg_plain(const Train& w, float* grads, const BwdStreams& s) {
    const Plan& P = w.P; void* ws = w.ws; hipStream_t st = w.st;
    const int B = P.s.B, C = P.s.C, E = P.s.E;
    float* dimg = P.ws<float>(ws, W_DIMG);
    GemmTN g; memset(&g, 0, sizeof(g));
    g.A = w.alpha; g.B = w.dhc + P.s.U; g.C = dimg; g.M = P.s.T; g.I = P.R; g.J = C;
    g.lda = B * P.Rp; g.ldb = B * P.HC; g.ldc = C;
    g.nsplit = 1; g.nbatch = B; g.strideA = P.Rp; g.strideB = P.HC; g.strideC = (long long)P.R * C; g.atomic = 0;
    RC(lxo_launch_gemm_tn(P.s.dtype, 1, 1, g, st));
    RC(s.wait_dmean());      // before d_mean's first reader
    RC(lxo_k_add_mean_grad(dimg, P.ws<float>(ws, W_DMEAN), B, P.R, C, st));
    RC(bwd_datt_img(w, grads));
    RC(s.datt_img_ready());
    return nt(P, false, true, false, P.ws<void>(ws, W_DATTIMG), E, P.pk(w.wp, K_ATT_IMG), E, dimg, C, B * P.R, C, E, nullptr, 0, true, st);
}

// parts & 1: the logits part; parts & 2: everything else.  The recurrence runs on `st` (its split-K form under `dual` also on the
// half-batch side stream); behind it BwdStreams says which stage runs on which stream.
int lxo_impl_decoder_train_bwd(const Plan& P, const float* prm, const void* wp, void* ws, const int* formula, float* grads,
                               int parts, hipStream_t st, bool defer_join, void* ready) {
    const Train w = train_of(P, prm, wp, ws, st);
    if (parts & 1) RC(bwd_logits(w, grads));
    if (!(parts & 2)) return 0;
    bool chain = false;                                  // the backward chain ran (and left the bf16 mirror of d_att_h)
    if (!w.sp.try_chain) {
        RC(bwd_zero_acc(w));
        // no backward chain in this call: clear its tickets and error word (lxo_chain_guard / Engine.chain_status read them; the workspace
        // is reused across shapes and the region offsets move with the shape, so stale bytes there would read as a broken chain)
        if (P.bf) HIPRC(hipMemsetAsync(chain_block(P, ws, kChainBwd), 0, kXDecSyncBytes, st));
    }
    if (w.sp.loop == StepPath::SplitK) RC(bwd_splitk_loop(w));
    else {
        RC(bwd_last_g(w));
        if (w.sp.try_chain) RC(bwd_chain(w, &chain));
        if (!chain) RC(bwd_fused_loop(w));
    }
    const BwdStreams s = {st, (w.sp.mirrors && !lxo_timer_on()) ? lxo_impl_encoder_side_stream() : nullptr};
    // f32 parity mode and bf16 deterministic mode: ordered reductions (no float atomics); the side stream works in its own half of the scratch
    const DetScratch det_s = s.side ? P.det_scratch_side(ws) : P.det_scratch(ws);
    RC(s.fork());
    RC(bwd_init_states(w, grads, s, det_s));                       // deferred stream
    RC(bwd_weight_grads(w, grads, chain, s, det_s));               // deferred stream (the main one off the fused kernels)
    RC(P.dimg_masked() ? bwd_dimg_masked(w, grads, s) : bwd_dimg_plain(w, grads, s));      // main stream
    RC(bwd_embedding(w, formula, grads, BwdStreams{st, nullptr}));                          // main stream (see above)
    RC(s.wait_datt_img());
    RC(tn(P, false, false, P.ws<void>(ws, W_IMG), P.s.C, P.ws<void>(ws, W_DATTIMG), P.s.E, grads + P.poff[P_ATT_IMG], P.s.E, P.s.B * P.R, P.s.C, P.s.E,
          s.deferred(), det_s));                                   // dW_att_img, deferred stream
    RC(s.join(defer_join));
    // the backward chain's error word -> the probe element (as for the forward chain in bwd_logits; y_W_o's bucket is reduced behind this call
    // where the backward chain runs, Engine.backward)
    if (chain) RC(lxo_k_chain_poison(nullptr, chain_err(P, ws, kChainBwd), grads + P.ptotal - 1, st));
    return s.record_ready(ready);
}

// ------------------------------------------------------------------ decode ----
// What the decode calls share, fetched once per call: the selection kind, its rows and the workspace regions it works in
struct Dec {
    int k, nv;                      // hypotheses per image, decoder rows (B * k)
    bool beam;                      // select with beam_step (else arg-max): lxo_beam_decode at any k, the step-wise calls at k > 1
    int *flags, *finished;          // [0..63]: per-step unfinished counters (two slots of 32); behind them finished[nv]
    int *ids_step, *par_step;       // the ids fed back into the next step, their parent slots
    float *logp, *tmp;              // beam: running log-probs, scratch
    float *rec, *cs; bf16_t* recb;  // the two state slots (slot 0 holds the initial state, slots alternate); bf16 mirror of rec or null
    float *logits, *alpha;          // of the step that just ran
    StepPath path;                  // what every decode follows is path.shape (no half-batch interleave, and the chain is the greedy call's own question)
    bool fused() const { return path.shape == StepPath::Fused; }
};
static Dec dec_of(const Plan& P, void* ws, int k, bool beam) {
    Dec d;
    d.k = k; d.nv = P.s.B * k; d.beam = beam;
    d.flags = P.ws<int>(ws, W_DEC_FLAGS); d.finished = d.flags + 64;
    d.ids_step = P.ws<int>(ws, W_DEC_IDS); d.par_step = P.ws<int>(ws, W_BEAM_PAR);
    d.logp = P.ws<float>(ws, W_BEAM_LP); d.tmp = P.ws<float>(ws, W_BEAM_TMP);
    d.rec = P.ws<float>(ws, W_REC); d.cs = P.ws<float>(ws, W_CS);
    d.logits = P.ws<float>(ws, W_DEC_LOGITS); d.alpha = P.ws<float>(ws, W_ALPHA);
    d.path = step_path(P, false);
    d.recb = d.path.mirrors ? P.ws<bf16_t>(ws, W_RECB) : nullptr;
    return d;
}
// x-part of the LSTM pre-activation for every possible input token, once per decode call: row v = embedding_table[v] K[0:D] + b,
// row V = the start token's.  The step kernels then pick rows by the previous ids (no per-step gather + GEMM launches).
static int decode_token_table(const Plan& P, const float* prm, const void* wp, void* ws, hipStream_t st) {
    const int U = P.s.U, D = P.s.D, V = P.s.V;
    RC(lxo_k_embed_table(P.s.dtype, prm + P.poff[P_EMB], prm + P.poff[P_START], P.ws<void>(ws, W_DEC_TXE), V, D, P.Dp, st));
    RC(nt(P, false, true, false, P.ws<void>(ws, W_DEC_TXE), P.Dp, P.pk(wp, K_LSTM_XT), P.Dp, P.ws<float>(ws, W_DEC_TX), 4 * U, V + 1, 4 * U, P.Dp,
          prm + P.poff[P_LSTM_B], 0, false, st));
    return 0;
}
static int decode_common_step(const Plan& P, const float* prm, const void* wp, void* ws, const Dec& d, int time, const int* ids_prev, hipStream_t st, const int* a_par = nullptr) {
    const int U = P.s.U, O = P.s.O, D = P.s.D, V = P.s.V, nv = d.nv;
    const size_t cur = (size_t)((time + 1) & 1) * nv, prev = (size_t)(time & 1) * nv;      // the rows of the two state slots
    Step s; memset(&s, 0, sizeof(s));
    s.rec_prev = d.rec + prev * P.REC; s.cs_prev = d.cs + prev * U; s.rec_cur = d.rec + cur * P.REC; s.cs_cur = d.cs + cur * U;
    if (d.recb) { s.recb_prev = d.recb + prev * P.RECB; s.recb_cur = d.recb + cur * P.RECB; }
    s.atth = P.ws<float>(ws, W_ATTH); s.alpha = d.alpha;
    if (d.fused()) {
        s.zx = P.ws<float>(ws, W_DEC_TX);
        RC(cell_step_fused(P, prm, wp, ws, nv, d.k, s, Drop{0u, 1.f, 0u, (time + 1) & 1, 0, 0}, st,      // t = the record slot: only its parity is used (attention direction)
                           ids_prev, ids_prev ? -1 : V, ids_prev ? a_par : nullptr));
    } else {
        // next input embedding (start token at time 0), its LSTM x-part, then the cell step
        float* zx = P.ws<float>(ws, W_DEC_ZX);
        RC(lxo_k_embed_rows(P.s.dtype, prm + P.poff[P_EMB], prm + P.poff[P_START], ids_prev, P.ws<void>(ws, W_DEC_EMB), nv, D, P.Dp, V, st));
        RC(nt(P, false, true, false, P.ws<void>(ws, W_DEC_EMB), P.Dp, P.pk(wp, K_LSTM_XT), P.Dp, zx, 4 * U, nv, 4 * U, P.Dp,
              prm + P.poff[P_LSTM_B], 0, false, st));
        s.zx = zx;
        RC(cell_step(P, prm, wp, ws, 0, nv, d.k, s, Drop{0u, 1.f, 0u, 0, 0, 0}, st));
    }
    // logits = o y_W_o (attention_cell.py:84).  On the step kernel where it runs: one workgroup per 16 vocabulary columns and 16 / 64 rows
    // (128 .. 160 workgroups); the dense-GEMM tiles gave 8 (greedy, 64 rows) or 12 (beam 5, 320 rows) workgroups -- 19 us of a beam step
    if (d.fused() && V % 4 == 0) {
        RStep e; memset(&e, 0, sizeof(e));
        e.M = nv; e.N = V; e.K = O; e.U = U; e.O = O; e.zx_row = -1; e.epi = RS_PLAIN; e.dr.inv_keep = 1.f;
        e.A = P.bf ? (const void*)s.recb_cur : (const void*)s.rec_cur;
        e.lda = P.bf ? P.RECB : P.REC;
        e.W = P.pk(wp, K_YWO_T); e.ldw = O; e.out = d.logits; e.ldo = P.Vp;
        const int rc = lxo_launch_rstep(P.s.dtype, P.bf, e, st);
        if (rc != -2) return rc < 0 ? rc : -rc;
    }
    return nt(P, true, true, nv <= 64, s.rec_cur, P.REC, P.pk(wp, K_YWO_T), O, d.logits, P.Vp, nv, V, O, nullptr, 0, false, st);
}

// Host side of dynamic_decode's `while not all(finished)` (dynamic_decode.py:38-61): steps are enqueued in chunks (8 steps of launches, or
// one launch of the persistent greedy-decode chain);
// each chunk ends with an asynchronous copy of its per-step "rows still unfinished" counters into pinned host memory and
// an event.  The host enqueues chunk c + 1 BEFORE it waits for chunk c's event, so the stream never drains while the
// host looks at the flags (the round-1 loop synchronised the stream every 8 steps); if chunk c turns out to contain the
// last step, chunk c + 1 ran speculatively (its ids land beyond `steps` columns, which no caller reads).
namespace {
struct DecodePoll { int* host; hipEvent_t ev[2]; bool ok; };
thread_local DecodePoll g_poll = {nullptr, {nullptr, nullptr}, false};
int poll_init() {
    if (g_poll.ok) return 0;
    HIPRC(hipHostMalloc((void**)&g_poll.host, 2 * 64 * sizeof(int), 0));      // one-time 512-byte pinned buffer per host thread
    HIPRC(hipEventCreateWithFlags(&g_poll.ev[0], hipEventDisableTiming));
    HIPRC(hipEventCreateWithFlags(&g_poll.ev[1], hipEventDisableTiming));
    g_poll.ok = true;
    return 0;
}
}  // namespace
// `enqueue(first, n, device counters)` enqueues steps first .. first + n - 1 (n <= steps_per_enqueue); step first + c adds its unfinished
// rows to counter word c.  counter_words (<= 32) words are cleared before an enqueue and copied back behind it.
template <typename EnqueueFn>
static int decode_loop(int max_iter, int steps_per_enqueue, int counter_words, int* flags, hipStream_t st, int* steps_out, EnqueueFn enqueue) {
    RC(poll_init());
    if (steps_per_enqueue > counter_words) steps_per_enqueue = counter_words;
    int enq = 0;                 // steps enqueued so far
    int nchunks = 0;             // chunks enqueued
    int steps = -1;              // final step count once known
    auto enqueue_chunk = [&]() -> int {
        const int slot = nchunks & 1;
        int* dflags = flags + slot * 32;                      // device counters of this chunk (flags[0..63]: two slots of 32)
        HIPRC(hipMemsetAsync(dflags, 0, counter_words * sizeof(int), st));
        int n = max_iter + 1 - enq; if (n > steps_per_enqueue) n = steps_per_enqueue;
        RC(enqueue(enq, n, dflags));
        enq += n;
        HIPRC(hipMemcpyAsync(g_poll.host + slot * 64, dflags, counter_words * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPRC(hipEventRecord(g_poll.ev[slot], st));
        g_poll.host[slot * 64 + 32] = n;                      // steps in this chunk
        g_poll.host[slot * 64 + 33] = enq - n;                // first step of this chunk
        ++nchunks;
        return 0;
    };
    RC(enqueue_chunk());
    int checked = 0;
    while (steps < 0) {
        if (enq <= max_iter) RC(enqueue_chunk());             // speculative: keeps the stream busy while the host polls
        const int slot = checked & 1;
        HIPRC(hipEventSynchronize(g_poll.ev[slot]));
        const int n = g_poll.host[slot * 64 + 32], first = g_poll.host[slot * 64 + 33];
        for (int c = 0; c < n; ++c) {
            // dynamic_decode.py:38-51: stop after the first step that leaves nothing unfinished, or after step max_iter.  Low 16 bits: the
            // unfinished rows (the greedy chain keeps "chains that reported" in the high bits; a launch-per-step counter is at most
            // B * beam <= 64 * 16 rows, so the mask changes nothing there)
            if ((g_poll.host[slot * 64 + c] & 0xffff) == 0 || first + c >= max_iter) { steps = first + c + 1; break; }
        }
        ++checked;
        if (steps < 0 && checked == nchunks && enq > max_iter) steps = enq;      // cannot happen (the last step hits the bound); belt and braces
    }
    if (nchunks > checked) HIPRC(hipEventSynchronize(g_poll.ev[(nchunks - 1) & 1]));   // the speculative chunk must not outlive the call's buffers
    if (steps_out) *steps_out = steps;
    return 0;
}
// The launch-per-step decodes: 8 steps per enqueue, `step(time, its counter word)` enqueues one
template <typename StepFn>
static int decode_loop_steps(int max_iter, int* flags, hipStream_t st, int* steps_out, StepFn step) {
    return decode_loop(max_iter, 8, 8, flags, st, steps_out, [&](int first, int n, int* unfinished) -> int {
        for (int c = 0; c < n; ++c) RC(step(first + c, unfinished + c));
        return 0;
    });
}

// The shapes and arguments every decode call refuses (-5): fewer record columns than steps, a beam the kernels do not take (k > V: fewer
// first-step candidates than hypotheses), a prefix without its arrays, allowed-token sets without their words or with rows shorter than V bits
static int decode_check(const Plan& P, int k, int steps_needed, const DecPrefix* prefix, const DecAllow* allow = nullptr) {
    if (P.s.max_steps < steps_needed || k < 1 || k > 16 || k > P.s.V) return -5;
    if (prefix && (!prefix->ids || !prefix->len || prefix->ld < 1)) return -5;
    if (allow && (!allow->bits || (allow->ld != 0 && allow->ld < (P.s.V + 31) / 32))) return -5;
    return 0;
}
// Before step 0: initial state, cleared flags, and what is computed once per call.  `again` (the greedy chain's fall-back, behind a
// chain that failed): only the initial state and the finished flags are rebuilt
static int decode_setup(const Plan& P, const float* prm, const void* wp, void* ws, const Dec& d, bool again, hipStream_t st) {
    RC(attention_prepare(P, d.path, prm, wp, ws, d.k, st));
    if (!again && P.att_exp())      // bf16: E_x = e^{2 att_img}, once per call
        RC(lxo_k_att_exp(P.ws<void>(ws, W_ATT_IMG), P.ws<void>(ws, W_ATT_EXP), (long long)P.s.B * P.R * P.s.E, st));
    if (d.fused()) RC(mirror_oh(P, ws, 0, d.nv, st));
    HIPRC(hipMemsetAsync(d.flags, 0, 256 + (size_t)d.nv * 4, st));
    if (again) return 0;
    if (d.beam) HIPRC(hipMemsetAsync(d.logp, 0, (size_t)d.nv * 4, st));
    if (d.fused()) RC(decode_token_table(P, prm, wp, ws, st));
    return 0;
}
// Behind decode_common_step(time): the attention maps of the step's rows as they ran, if asked for (beam: row b * k + j = hypothesis slot j
// BEFORE this step's re-ordering -- what the reference's py_func tap sees, attention_mechanism.py:59-65,96-105), then the arg-max, or the
// beam's top-k and the re-ordering of the new state rows (+ their bf16 mirror) by parent, which feed the next LSTM GEMM.  `indirect`: no
// re-ordering, the next step reads its rows through par_step
static int decode_keep_alpha(const Plan& P, const Dec& d, int time, const DecodeOuts& o, hipStream_t st) {
    if (o.alpha) HIPRC(hipMemcpyAsync(o.alpha + (size_t)time * d.nv * P.Rp, d.alpha, (size_t)d.nv * P.Rp * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}
// A grammar call (DecodeOuts::grammar, grammar.h): the arguments of the grammar kernels and `rows`, the per-row sets the select kernels read in place of
// the images' static ones.  on == false: no grammar, the call runs what it ran before
struct DecGram { bool on; GrammarArgs a; DecAllow rows; int* depth; };
static DecGram decode_grammar(const Plan& P, const Dec& d, int id_end, int max_iter, const DecodeOuts& o) {
    DecGram g; memset(&g, 0, sizeof(g));
    if (!o.grammar) return g;
    g.on = true;
    g.a = GrammarArgs{o.grammar->cls, o.grammar->n_kinds, o.grammar->max_depth, o.grammar->budget, o.allow ? o.allow->bits : nullptr,
                      o.allow ? o.allow->ld : 0, o.grammar->scratch, d.nv, d.k, P.s.V, id_end, max_iter};
    g.rows = DecAllow{lxo_k_grammar_sets(g.a), (P.s.V + 31) / 32, 1};
    g.depth = o.grammar->depth;
    return g;
}
// the outputs as the select kernels take them: under a grammar `allow` names the per-row sets
static DecodeOuts decode_outs(const DecodeOuts& o, const DecGram& g) {
    DecodeOuts r = o;
    if (g.on) r.allow = &g.rows;
    return r;
}
// behind a select: the rows' states after step `time` and their sets of step time + 1 (beam: through the parents the select just wrote)
static int decode_grammar_step(const Plan& P, const Dec& d, const DecGram& g, int time, hipStream_t st) {
    if (!g.on) return 0;
    return lxo_k_grammar_step(g.a, d.ids_step, d.beam ? d.par_step : nullptr, d.finished, time, g.depth, P.s.max_steps, time, st);
}
static int decode_select(const Plan& P, const Dec& d, int id_end, int time, const DecodeOuts& o, int* unfinished, bool indirect, hipStream_t st,
                         const DecGram* g = nullptr) {
    const int ms = P.s.max_steps, U = P.s.U, nv = d.nv, cur = (time + 1) & 1;
    RC(decode_keep_alpha(P, d, time, o, st));
    if (!d.beam) {
        RC(lxo_k_argmax(d.logits, P.Vp, P.s.V, nv, id_end, d.ids_step, o.ids, ms, time, d.finished, unfinished, st, o.scores, o.prefix, o.allow));
        if (g) RC(decode_grammar_step(P, d, *g, time, st));
        return 0;
    }
    RC(lxo_k_beam_step(d.logits, P.Vp, P.s.V, P.s.B, d.k, id_end, time, P.s.div_gamma, P.s.div_prob, P.s.div_seed, d.tmp, d.logp, d.finished,
                       d.ids_step, d.par_step, o.ids, o.parents, ms, unfinished, st, o.scores, o.prefix, o.allow));
    if (g) RC(decode_grammar_step(P, d, *g, time, st));
    if (indirect) return 0;
    RC(lxo_k_beam_gather(d.rec + (size_t)cur * nv * P.REC, P.REC, P.XH, d.cs + (size_t)cur * nv * U, U, d.par_step, d.k,
                         d.tmp, d.tmp + (size_t)nv * P.XH, nv, d.recb ? d.recb + (size_t)cur * nv * P.RECB : nullptr, P.RECB, st));
    return 0;
}

int lxo_impl_greedy_decode(const Plan& P, const float* prm, const void* wp, void* ws, int id_end, int max_iter, const DecodeOuts& out,
                           int* steps_out, hipStream_t st) {
    const int B = P.s.B, ms = P.s.max_steps;
    const DecPrefix* prefix = out.prefix;
    RC(decode_check(P, 1, max_iter + 1, prefix, out.allow));
    const Dec d = dec_of(P, ws, 1, false);
    RC(decode_setup(P, prm, wp, ws, d, false, st));
    const DecGram g = decode_grammar(P, d, id_end, max_iter, out);
    const DecodeOuts og = decode_outs(out, g);
    if (g.on) RC(lxo_k_grammar_setup(g.a, st));
    if (d.path.try_chain && P.att_exp() && !out.alpha && !g.on) {      // the chain holds no grammar (as it holds no sampler): launch per step
        // the persistent greedy-decode chain (xdec.hip: xdec_dec_kernel): 16 steps per launch; -2 = the shape does not qualify
        XDecDec x; memset(&x, 0, sizeof(x));
        xdec_common(x, P, prm, wp, ws);
        x.Wyo = (const bf16_t*)P.pk(wp, K_YWO_T); x.ldyo = P.s.O;
        x.tx = P.ws<float>(ws, W_DEC_TX);
        x.ids_step = d.ids_step; x.ids_out = out.ids; x.logp_out = out.scores; x.finished = d.finished;
        if (prefix) { x.prefix = prefix->ids; x.prefix_len = prefix->len; x.prefix_ld = prefix->ld; x.prefix_lim = prefix->lim; }
        if (out.allow) { x.allow = out.allow->bits; x.allow_ld = out.allow->ld; }
        x.V = P.s.V; x.id_end = id_end; x.max_steps = ms;
        x.t0 = 0; x.nsteps = 1; x.unfinished = d.flags;
        x.stop = d.ids_step + B;                            // one word behind the fed-back ids (region "dec_ids" holds B x max_steps ints)
        HIPRC(hipMemsetAsync(x.stop, 0, sizeof(int), st));
        HIPRC(hipMemsetAsync(chain_err(P, ws, kChainFwd), 0, sizeof(unsigned), st));      // the error word: once per decode (the launcher leaves it alone)
        int chunk_steps = 16;                             // steps per launch (LXO_XDEC_DEC_CHUNK: 1 .. 16; read per call so that a test can vary it)
        { const int c = lxo_switch(SW_XDEC_DEC_CHUNK); if (c > 0 && c < 16) chunk_steps = c; }
        bool took = true;
        const int rc = decode_loop(max_iter, chunk_steps, 32, d.flags, st, steps_out, [&](int first, int n, int* unfinished) -> int {
            XDecDec y = x; y.t0 = first; y.nsteps = n; y.unfinished = unfinished;
            const int r = lxo_launch_xdec_dec(y, P.s.U, P.s.O, P.s.C, P.s.E, st);
            if (r == -2 && first == 0) { took = false; return -2; }
            return r;
        });
        if (took) {
            if (rc) return rc;
            // the chain's error word (a hand-over that timed out: the ids are garbage).  The call has synchronised with the stream already.
            unsigned errw = 0;
            HIPRC(hipMemcpyAsync(&errw, chain_err(P, ws, kChainFwd), sizeof(unsigned), hipMemcpyDeviceToHost, st));
            HIPRC(hipStreamSynchronize(st));
            if (errw == 0) return 0;
            // fall back to the launch-per-step kernels: the initial state and the finished flags are rebuilt first
            RC(decode_setup(P, prm, wp, ws, d, true, st));
        } else {
            HIPRC(hipStreamSynchronize(st));              // (nothing was enqueued by the refused first chunk but its counter memset)
            HIPRC(hipMemsetAsync(chain_block(P, ws, kChainFwd), 0, kXDecTicketBytes, st));      // no chain in this call: no tickets (Engine.chain_status reads them)
            HIPRC(hipMemsetAsync(d.flags, 0, 256 + (size_t)B * 4, st));
        }
    } else if (P.bf) HIPRC(hipMemsetAsync(chain_block(P, ws, kChainFwd), 0, kXDecTicketBytes, st));
    return decode_loop_steps(max_iter, d.flags, st, steps_out, [&](int time, int* unfinished) -> int {
        RC(decode_common_step(P, prm, wp, ws, d, time, time == 0 ? nullptr : d.ids_step, st));
        return decode_select(P, d, id_end, time, og, unfinished, false, st, &g);
    });
}

// Sampled decode: lxo_impl_greedy_decode's loop over n = s.beam rows per image, every row an independent draw of the whole sequence -- the beam's
// tiled set-up and decoder step, no parents, and lxo_k_sample as the select step.  Launch per step in both dtypes (the chain holds no sampler)
int lxo_impl_sample_decode(const Plan& P, const float* prm, const void* wp, void* ws, int id_end, int max_iter, const DecSample& opts,
                           const DecodeOuts& out, float* logq_out, int* steps_out, hipStream_t st) {
    const int n = P.s.beam;
    RC(decode_check(P, n, max_iter + 1, out.prefix, out.allow));
    const Dec d = dec_of(P, ws, n, false);
    RC(decode_setup(P, prm, wp, ws, d, false, st));
    const DecGram g = decode_grammar(P, d, id_end, max_iter, out);
    const DecodeOuts og = decode_outs(out, g);
    if (g.on) RC(lxo_k_grammar_setup(g.a, st));
    return decode_loop_steps(max_iter, d.flags, st, steps_out, [&](int time, int* unfinished) -> int {
        RC(decode_common_step(P, prm, wp, ws, d, time, time == 0 ? nullptr : d.ids_step, st));
        RC(decode_keep_alpha(P, d, time, out, st));
        RC(lxo_k_sample(d.logits, P.Vp, P.s.V, d.nv, n, id_end, time, opts, d.ids_step, out.ids, out.scores, logq_out, P.s.max_steps, time,
                        d.finished, unfinished, st, og.prefix, og.allow));
        return decode_grammar_step(P, d, g, time, st);
    });
}

// lxo_chain_guard: scale[0] = NaN when a chain of this step left an error word, else the clip scale / 1 (decoder_kernels.hip)
int lxo_impl_chain_guard(const Plan& P, void* ws, const float* grads, float* scale, int have_scale, unsigned* status, hipStream_t st) {
    return lxo_k_chain_guard(chain_err(P, ws, kChainFwd), chain_err(P, ws, kChainBwd), grads ? grads + P.ptotal - 1 : nullptr, scale, have_scale, status, st);
}

// ---- AttentionState of the step-wise decode (attention_cell.py:8: cell_state = LSTMStateTuple(c, h), o): the state lxo_decode_step(time) /
// lxo_decode_cell_step(time) steps FROM lives in record slot time & 1 ----
static int state_rows(const Plan& P) { return P.s.B * (P.s.beam > 1 ? P.s.beam : 1); }
int lxo_impl_decode_state_get(const Plan& P, void* ws, int time, float* c, float* h, float* o, hipStream_t st) {
    const int nv = state_rows(P), U = P.s.U, O = P.s.O, slot = time & 1;
    const float* rec = P.ws<float>(ws, W_REC) + (size_t)slot * nv * P.REC;
    const float* cs = P.ws<float>(ws, W_CS) + (size_t)slot * nv * U;
    if (c) HIPRC(hipMemcpyAsync(c, cs, (size_t)nv * U * 4, hipMemcpyDeviceToDevice, st));
    if (h) HIPRC(hipMemcpy2DAsync(h, (size_t)U * 4, rec + O, (size_t)P.REC * 4, (size_t)U * 4, nv, hipMemcpyDeviceToDevice, st));
    if (o) HIPRC(hipMemcpy2DAsync(o, (size_t)O * 4, rec, (size_t)P.REC * 4, (size_t)O * 4, nv, hipMemcpyDeviceToDevice, st));
    return 0;
}
int lxo_impl_decode_state_set(const Plan& P, void* ws, int time, const float* c, const float* h, const float* o, const int* ids_prev, hipStream_t st) {
    const int nv = state_rows(P), U = P.s.U, O = P.s.O, slot = time & 1;
    float* rec = P.ws<float>(ws, W_REC) + (size_t)slot * nv * P.REC;
    float* cs = P.ws<float>(ws, W_CS) + (size_t)slot * nv * U;
    if (c) HIPRC(hipMemcpyAsync(cs, c, (size_t)nv * U * 4, hipMemcpyDeviceToDevice, st));
    if (h) HIPRC(hipMemcpy2DAsync(rec + O, (size_t)P.REC * 4, h, (size_t)U * 4, (size_t)U * 4, nv, hipMemcpyDeviceToDevice, st));
    if (o) HIPRC(hipMemcpy2DAsync(rec, (size_t)P.REC * 4, o, (size_t)O * 4, (size_t)O * 4, nv, hipMemcpyDeviceToDevice, st));
    if ((h || o) && step_path(P, false).shape == StepPath::Fused) RC(mirror_oh(P, ws, (size_t)slot * nv, nv, st));      // the step GEMMs read the bf16 mirror of [o | h]
    if (ids_prev) HIPRC(hipMemcpyAsync(P.ws<int>(ws, W_DEC_IDS), ids_prev, (size_t)nv * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}
// AttentionCell.step alone (attention_cell.py:58-89): state slot time & 1 -> slot (time + 1) & 1, logits in ws region "dec_logits";
// no arg-max, no finished flags (those belong to the decoder cells: lxo_decode_step)
int lxo_impl_decode_cell_step(const Plan& P, const float* prm, const void* wp, void* ws, int time, int start_token, hipStream_t st) {
    const int k = P.s.beam > 1 ? P.s.beam : 1;
    if (time < 0) return -5;
    const Dec d = dec_of(P, ws, k, k > 1);
    return decode_common_step(P, prm, wp, ws, d, time, start_token ? nullptr : d.ids_step, st);
}

// ---- the decode loop one step at a time: what the reference's cell protocol (dynamic_decode.py:34-61: initialize / step /
// finalize) is bound to.  State (c, h, o, running log-probs, finished flags, previous ids) stays in the workspace. ----
int lxo_impl_decode_begin(const Plan& P, const float* prm, const void* wp, void* ws, hipStream_t st) {
    const int k = P.s.beam > 1 ? P.s.beam : 1;
    RC(decode_check(P, k, 1, nullptr));
    return decode_setup(P, prm, wp, ws, dec_of(P, ws, k, k > 1), false, st);
}

int lxo_impl_decode_step(const Plan& P, const float* prm, const void* wp, void* ws, int id_end, int time,
                         int* ids_out, int* parents_out, int* finished_out, int* unfinished_host, hipStream_t st) {
    const int k = P.s.beam > 1 ? P.s.beam : 1;
    if (time < 0 || decode_check(P, k, time + 1, nullptr)) return -5;
    const Dec d = dec_of(P, ws, k, k > 1);
    HIPRC(hipMemsetAsync(d.flags, 0, sizeof(int), st));
    RC(decode_common_step(P, prm, wp, ws, d, time, time == 0 ? nullptr : d.ids_step, st));
    // (the state rows are always re-ordered here: the callers may look at the state between steps, see lxo_impl_beam_decode)
    RC(decode_select(P, d, id_end, time, DecodeOuts{ids_out, parents_out, nullptr, nullptr, nullptr}, d.flags, false, st));
    if (finished_out) HIPRC(hipMemcpyAsync(finished_out, d.finished, (size_t)d.nv * 4, hipMemcpyDeviceToHost, st));
    if (unfinished_host) {
        HIPRC(hipMemcpyAsync(unfinished_host, d.flags, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPRC(hipStreamSynchronize(st));
    }
    return 0;
}

int lxo_impl_beam_decode(const Plan& P, const float* prm, const void* wp, void* ws, int id_end, int max_iter, const DecodeOuts& out,
                         int* steps_out, hipStream_t st) {
    RC(decode_check(P, P.s.beam, max_iter + 1, out.prefix, out.allow));
    const Dec d = dec_of(P, ws, P.s.beam, true);
    RC(decode_setup(P, prm, wp, ws, d, false, st));
    const DecGram g = decode_grammar(P, d, id_end, max_iter, out);
    const DecodeOuts og = decode_outs(out, g);
    if (g.on) RC(lxo_k_grammar_setup(g.a, st));
    // the state of a step's rows is that of their PARENT hypotheses (beam_search_decoder_cell.py:176-178).  With the fused step kernels the next LSTM launch
    // reads its [o | h] and c rows through the parents in place; the launch that re-ordered the rows (beam_permute_kernel, 5.3 us + its gap) is only left for
    // the split-K step kernels and for lxo_decode_step, whose callers may look at the state between steps (LXO_BEAM_INDIRECT=0: always re-order; A/B)
    const bool indirect = lxo_switch(SW_BEAM_INDIRECT) && d.fused();
    return decode_loop_steps(max_iter, d.flags, st, steps_out, [&](int time, int* unfinished) -> int {
        RC(decode_common_step(P, prm, wp, ws, d, time, time == 0 ? nullptr : d.ids_step, st, indirect ? d.par_step : nullptr));
        return decode_select(P, d, id_end, time, og, unfinished, indirect, st, &g);
    });
}
