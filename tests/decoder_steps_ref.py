"""float64 reference of the decoder's training step, one stage at a time, for tests/test_decoder_steps_sim.py (hipsim) and
tests/test_gpu_decoder_steps.py, and of the decode step (tests/decode_steps_walk.py: test_decode_steps_sim.py, test_gpu_decode_steps.py).  Torch float64 only (on whatever device the tensors live); never calls the library.

Every function takes the values the kernel actually READ -- a stored workspace region, a weight rounded to the compute dtype, an f32
operand rounded to bf16 where the bf16 kernels convert it on load -- and returns the exact result with

    (value, S)       a stored sum: S = the float64 sum of the absolute values of the element's terms.  Held as in
                     tests/encoder_layers_ref.py: bf16-stored 2^-8 |ref| + 2^-14 S, f32 2^-14 S (bf16 mode) / 2^-20 S (f32 mode)
    (value, bound)   a non-linear stage: first-order propagation in float64, bound(out) = sum |d out / d in| bound(in) + eps.  An input read
                     from a stored region carries bound 0; an input the stage computes itself (the GEMM part of z, the carry product)
                     carries the sum bound `absf * S`.

eps are the bars tests/test_gpu_xdec.py::test_bf16_cell_transcendentals_over_pm20 holds the exp / rcp forms to against float64:
EPS_T = 4e-7 on a gate or tanh value, EPS_CH = 2e-6 on c / h.  REL_F32 covers the few f32 roundings of a point-wise expression on
stored operands (products, one subtraction).  Gate order i, j, f, o; forget bias 1.0; the record row is [o | h | h~ | ctx]."""
import torch

from encoder_layers_ref import bf16_round, bound, ratio, REL_BF16, ABS_BF16, ABS_F32      # noqa: F401  (re-exported for the walk)
from oracle.ref_model import drop_mask

EPS_T = 4e-7
EPS_CH = 2e-6
REL_F32 = 2.0 ** -21
PACK28 = 2.0 ** -20          # csrc/xdec.hip, comment at pack28: "an f32 cut to 19 mantissa bits (relative error 2^-20)"


def f64(t):
    return t.to(torch.float64)


def mm(a, b):
    """a @ b -> (product, S = |a| @ |b|)"""
    a, b = f64(a), f64(b)
    return a @ b, a.abs() @ b.abs()


def masks(keep, seed, which, t, B, width, dev):
    """the dropout scale of step t (0 or 1 / keep) as float64 [B, width], and the 0 / 1 mask; keep outside (0, 1) = no dropout"""
    if not (0.0 < keep < 1.0):
        one = torch.ones(B, width, dtype=torch.float64, device=dev)
        return one, one
    m = (drop_mask(keep, seed, which, t, B, width, rows_total=B) > 0).to(torch.float64).to(dev)
    return m / keep, m


# ------------------------------------------------------------------------------------------------------------------------ set-up --
def rowmean(img):
    """mean over the R regions: (mean [B, C], S)"""
    x = f64(img)
    return x.mean(1), x.abs().mean(1)


def tanh_dense(a, w, b, absf):
    """tanh(a w + b) on stored a: (value, bound)"""
    pre, S = mm(a, w)
    pre, S = pre + b, S + b.abs()
    v = torch.tanh(pre)
    return v, (1 - v * v) * absf * S + EPS_T


def att_exp(att_img):
    """E_x = e^{2 x} of the stored projection, exponent clamped to 2^+-60 (att_exp_kernel).  bound: one bf16 rounding + the f32 product
    x * 2 / ln 2 in front of v_exp_f32 (half an ulp of an exponent below 2^6: 2^-19 ln 2 relative) and the exp itself (2^-22)"""
    x = f64(att_img)
    v = torch.exp2(torch.clamp(x * 2.8853900817779268, -60.0, 60.0))
    return v, (REL_BF16 + 2.0 ** -18) * v


def embed_rows(table, start, formula, T):
    """teacher-forcing inputs [T, B, D]: the start token at t = 0, table[formula[:, t - 1]] after that (ids clamped to the table)"""
    V = table.shape[0]
    ids = formula[:, :T - 1].clamp(0, V - 1).long().t()                 # [T - 1, B]
    rows = table[ids]                                                  # [T - 1, B, D]
    s = start.reshape(1, 1, -1).expand(1, formula.shape[0], -1)
    return torch.cat([s, rows], 0)


def token_table(table, start, Dp):
    """the decode's input rows, one per possible previous token: row v < V = embedding_table[v], row V = start_token, columns D..Dp zero
    (embed_table_kernel) -> [V + 1, Dp]"""
    V, D = table.shape
    t = torch.zeros(V + 1, Dp, dtype=torch.float64, device=table.device)
    t[:V, :D] = f64(table)
    t[V, :D] = f64(start).reshape(-1)
    return t


# -------------------------------------------------------------------------------------------------------------------- forward step --
def lstm_gates(zx_t, a, kr, absf):
    """z = zx_t (stored) + a K[D:]; gates [B, 4U] as stored (i, j, f, o): (gates, bound)"""
    zg, S = mm(a, kr)
    z = f64(zx_t) + zg
    bz = absf * (S + f64(zx_t).abs())
    U = z.shape[1] // 4
    i, j, f, o = torch.sigmoid(z[:, :U]), torch.tanh(z[:, U:2 * U]), torch.sigmoid(z[:, 2 * U:3 * U] + 1.0), torch.sigmoid(z[:, 3 * U:])
    g = torch.cat([i, j, f, o], 1)
    d = torch.cat([i * (1 - i), 1 - j * j, f * (1 - f), o * (1 - o)], 1)
    return g, d * bz + EPS_T


def lstm_state(gates, c_prev):
    """c = f c_prev + i j on the stored gates and c_prev: (c, bound)"""
    U = c_prev.shape[1]
    g = f64(gates)
    i, j, f = g[:, :U], g[:, U:2 * U], g[:, 2 * U:3 * U]
    c = f * f64(c_prev) + i * j
    return c, torch.full_like(c, EPS_CH)


def lstm_h(gates, c):
    """h = o tanh(c) on the stored gate and the stored c: (h, bound)"""
    U = c.shape[1]
    h = f64(gates)[:, 3 * U:] * torch.tanh(f64(c))
    return h, torch.full_like(h, EPS_CH)


def lstm_state_from(gates, b_g, c_prev):
    """the decode keeps no gates: c = f c_prev + i j from the gates the stage computes itself (lstm_gates' value and bound) and the stored
    c_prev; bound = |c_prev| b_f + |j| b_i + |i| b_j + EPS_CH: (c, bound)"""
    U = c_prev.shape[1]
    cp = f64(c_prev)
    i, j, f = gates[:, :U], gates[:, U:2 * U], gates[:, 2 * U:3 * U]
    bi, bj, bf_ = b_g[:, :U], b_g[:, U:2 * U], b_g[:, 2 * U:3 * U]
    return f * cp + i * j, cp.abs() * bf_ + j.abs() * bi + i.abs() * bj + EPS_CH


def lstm_h_from(gates, b_g, c):
    """h = o tanh(c) from the o gate the stage computes itself and the stored c; bound = |tanh c| b_o + EPS_CH: (h, bound)"""
    U = c.shape[1]
    tc = torch.tanh(f64(c))
    return gates[:, 3 * U:] * tc, tc.abs() * b_g[:, 3 * U:] + EPS_CH


def dropped(v, scale):
    """v * scale on the stored v: one f32 product with the f32 1 / keep"""
    r = f64(v) * scale
    return r, REL_F32 * r.abs()


def tanh_tau(att_x, att_h, expd):
    """tanh(x + a) per (sample, region, channel) in the form the kernel uses on the operand it reads: att_x = x [B, R, E], or -- expd -- the stored
    E_x = e^{2x}: with E_a = e^{2a} (exponent clamped to 2^+-60), r = 1 / (1 + E_x E_a), tanh = 1 - 2 r and 1 - tanh^2 = 4 r (1 - r).
    -> (tau, 1 - tau^2)"""
    a = f64(att_h)[:, None, :]
    if expd:
        ea = torch.exp2(torch.clamp(a * 2.8853900817779268, -60.0, 60.0))
        r = 1.0 / (1.0 + f64(att_x) * ea)
        return 1.0 - 2.0 * r, 4.0 * r * (1.0 - r)
    tau = torch.tanh(f64(att_x) + a)
    return tau, 1.0 - tau * tau


def attention_alpha(tau, beta, absf, extra_rel=0.0):
    """e = tau beta; alpha = softmax(e): (alpha [B, R], bound).  d alpha_r / d e_j = alpha_r (delta_rj - alpha_j)"""
    b = f64(beta).reshape(-1)
    e = tau @ b
    be = absf * (tau.abs() @ b.abs()) + EPS_T * b.abs().sum() + extra_rel * e.abs()
    al = torch.softmax(e, dim=1)
    return al, al * (be + (al * be).sum(1, keepdim=True)) + EPS_T


def context(alpha, img):
    """ctx = sum_r alpha_r img_r on the stored alpha: (ctx [B, C], S)"""
    a, x = f64(alpha), f64(img)
    return torch.einsum("br,brc->bc", a, x), torch.einsum("br,brc->bc", a.abs(), x.abs())


def context_from_att_h(att_h, S_h, att_x, expd, beta, img, absf):
    """the chain of a step that stores neither att_h nor alpha (the persistent greedy-decode chain): att_h (the float64 product, its sum
    bound delta_k = absf S_h) -> alpha -> ctx.  tanh is 1-Lipschitz, so a region's score moves by at most eps = sum_k |beta_k| delta_k and
    |d alpha_r| <= alpha_r (e^{2 eps} - 1) + attention_alpha's own bound; the context then moves by sum_r |d alpha_r| |img_r|, beside its own
    sum (absf S) and the 28-bit hand-over of the chunk partials (PACK28 S): (ctx [B, C], bound)"""
    tau, _ = tanh_tau(att_x, att_h, expd)
    al, b_al = attention_alpha(tau, beta, absf)
    eps = (f64(beta).reshape(1, -1).abs() * absf * S_h).sum(1, keepdim=True)
    d_al = al * torch.expm1(2.0 * eps) + b_al
    x = f64(img)
    ctx, S = context(al, x)
    return ctx, torch.einsum("br,brc->bc", d_al, x.abs()) + (absf + PACK28) * S


def output_o(a, w, scale, absf):
    """o = tanh(a [o_W_h; o_W_c]) * dropout scale: (o, bound)"""
    pre, S = mm(a, w)
    t = torch.tanh(pre)
    v = t * scale
    return v, scale * ((1 - t * t) * absf * S + EPS_T) + REL_F32 * v.abs()


# ------------------------------------------------------------------------------------------------------------------- backward step --
def g_step(do_log_t, carry, S_carry, o_t, scale, keep_on, keep, absf):
    """g = (d_o from the logits + the carried d_o) * dropout scale * (1 - tanh^2); tanh recovered from the stored, dropped o as o * keep
    (rstep.hip RS_CARRY / tanh_bwd_kernel: o / inv_keep).  carry = None at t = T - 1.  -> (g, bound)"""
    d = f64(do_log_t)
    S = d.abs()
    if carry is not None:
        d = d + carry
        S = S + S_carry
    th = f64(o_t) * (keep if keep_on else 1.0)
    q = 1.0 - th * th
    g = d * scale * q
    return g, scale * (q * absf * S + d.abs() * 2 * REL_F32)


def attention_bwd(alpha, img, d_ctx, ctx, absf):
    """d_alpha_r = d_ctx . img_r; s = ctx . d_ctx (the kernel reads the stored context: = sum_r alpha_r d_alpha_r);
    de = alpha (d_alpha - s): (de [B, R], bound)"""
    a, x, d, c = f64(alpha), f64(img), f64(d_ctx), f64(ctx)
    da = torch.einsum("brc,bc->br", x, d)
    Sa = torch.einsum("brc,bc->br", x.abs(), d.abs())
    s = (c * d).sum(1, keepdim=True)
    Ss = (c.abs() * d.abs()).sum(1, keepdim=True)
    de = a * (da - s)
    return de, a * absf * (Sa + Ss) + REL_F32 * de.abs()


def datt_h(de, dtau, beta, absf):
    """d_att_h_k = beta_k sum_r de_r (1 - tanh^2)_rk on the stored de: (value [B, E], bound)"""
    b = f64(beta).reshape(1, -1)
    d = f64(de)
    v = torch.einsum("br,brk->bk", d, dtau)
    S = torch.einsum("br,brk->bk", d.abs(), dtau.abs())
    return v * b, b.abs() * (absf * S + 2 * EPS_T * d.abs().sum(1, keepdim=True))


def lstm_bwd(dhm, b_dhm, v, S_v, carry_h, S_ch, scale1, gates, c_cur, c_prev, dcc, b_dcc, absf):
    """d_h = (d_h~ + d_att_h W_att_h^T) * mask_1 + carried d_h; d_c = running d_c + d_h o (1 - tanh^2 c); d_z from the stored gates, c_t and
    c_{t-1}.  dhm: d_h~ of the o projection (stored: b_dhm = 0); v, carry_h: the two products the kernel forms itself.
    -> (dz [B, 4U], bound), (d_c handed to step t - 1, bound)"""
    U = c_cur.shape[1]
    g = f64(gates)
    i, j, f, o = g[:, :U], g[:, U:2 * U], g[:, 2 * U:3 * U], g[:, 3 * U:]
    dh = (f64(dhm) + v) * scale1
    b_dh = scale1 * (b_dhm + absf * S_v)
    if carry_h is not None:
        dh = dh + carry_h
        b_dh = b_dh + absf * S_ch
    tc = torch.tanh(f64(c_cur))
    q = 1 - tc * tc
    dc = dcc + dh * o * q
    b_dc = b_dcc + (o * q).abs() * b_dh + (dh * o).abs() * 2 * EPS_T
    cp = f64(c_prev)
    ki, kj, kf, ko = j * i * (1 - i), i * (1 - j * j), cp * f * (1 - f), tc * o * (1 - o)
    dz = torch.cat([dc * ki, dc * kj, dc * kf, dh * ko], 1)
    b = torch.cat([ki.abs() * b_dc, kj.abs() * b_dc, kf.abs() * b_dc, ko.abs() * b_dh + (dh * o * (1 - o)).abs() * EPS_T], 1)
    return (dz, b + 4 * REL_F32 * dz.abs()), (dc * f, b_dc * f + REL_F32 * (dc * f).abs())


def init_bwd(dcc, dxh, c0, rec0, U, O):
    """dpre0 = [d_c0 (1 - c0^2) | d_h0 (1 - h0^2) | d_o0 (1 - o0^2)] on the stored dcc, dxh ([d_o | d_h]), cs[0] and rec[0]: (value, bound)"""
    d = torch.cat([f64(dcc), f64(dxh)[:, O:O + U], f64(dxh)[:, :O]], 1)
    s = torch.cat([f64(c0), f64(rec0)[:, O:O + U], f64(rec0)[:, :O]], 1)
    return d * (1 - s * s), 2 * REL_F32 * d.abs()


def colsum(d):
    """column sums over every leading index: (sum, S)"""
    d = f64(d).reshape(-1, d.shape[-1])
    return d.sum(0), d.abs().sum(0)


def embed_scatter(demb, formula, V):
    """d_emb [T, B, D] (stored) scattered: rows t >= 1 into embedding_table[formula[:, t - 1]] (duplicated ids sum), the t = 0 rows into
    start_token only.  -> (d_table [V, D], S), (d_start [D], S)"""
    d = f64(demb)
    T, B, D = d.shape
    ids = formula[:, :T - 1].clamp(0, V - 1).long().t().reshape(-1)
    rows = d[1:].reshape(-1, D)
    dt = torch.zeros(V, D, dtype=torch.float64, device=d.device).index_add_(0, ids, rows)
    st = torch.zeros(V, D, dtype=torch.float64, device=d.device).index_add_(0, ids, rows.abs())
    return (dt, st), (d[0].sum(0), d[0].abs().sum(0))


def datt_img(de, att_img, att_h, beta, absf, bf):
    """d_att_img[b, r, k] = beta_k sum_t de[t, b, r] (1 - tau^2), d_beta_k = sum de tau on the stored de / att_img / att_h
    (datt_img_kernel: the x form in both modes; the bf16 kernel sums d_beta as sum de - 2 sum de r with r = (1 - tau) / 2, so its terms are
    |de| (1 + 2 r)).  -> (d_att_img [B, R, E], bound without the storage rounding), (d_beta [E], S + the tanh term)"""
    b = f64(beta).reshape(1, 1, -1)
    T = de.shape[0]
    acc = Sacc = db = Sdb = 0.0
    dsum = 0.0
    for t in range(T):
        tau, dtau = tanh_tau(att_img, att_h[t], False)
        d = f64(de[t])[:, :, None]
        acc = acc + d * dtau
        Sacc = Sacc + d.abs() * dtau
        db = db + (d * tau).sum((0, 1))
        Sdb = Sdb + (d.abs() * ((2.0 - tau) if bf else tau.abs())).sum((0, 1))
        dsum = dsum + d.abs().sum((0, 1))
    bnd = b.abs() * (absf * Sacc + 2 * EPS_T * f64(de).abs().sum(0)[:, :, None])
    return (acc * b, bnd), (db, Sdb + (EPS_T / absf) * dsum)
