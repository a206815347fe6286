"""TEST INFRASTRUCTURE: walks the decoder's training step stage by stage through an adapter (the hipsim `Sim` or the GPU `Engine`) and checks
every workspace region and gradient it stores against tests/decoder_steps_ref.py applied to the operands the kernels themselves stored.

Sequence: encoder forward once; lxo_decoder_train_fwd -> the forward stages; lxo_ce_loss_fwd_bwd (d(logits) is taken as stored: the output-head
tests own it); lxo_decoder_train_bwd_part(1) -> do_log and d y_W_o; lxo_decoder_train_bwd_part(2) -> the backward stages for t = T-1 .. 0,
then the deferred gradients and what goes to the encoder.

The adapter `io` offers: bf, det, B, live_B, T, R, Rp, C, E, U, O, D, V, keep, seed, step_kernels, dual (a side stream is bound: the
half-batch interleave), chain (the persistent chains ran), dimg_bf (lxo_ws_region_dtype("d_img") is bf16), dev, params (name -> f32 tensor);
values(region, shape, kind) (float64 of the "f32" / "bf16" / "ct" = compute-dtype contents), bits(region, shape, kind) (raw 16- / 32-bit
patterns), write(region, tensor), fill(region, byte), grad(name) (float64), zero_grads(), set_formula(formula, lengths), enc_fwd(), dec_fwd(),
loss(inv_ntok), dec_bwd(parts).

Every region the walk reads is filled with 0xFF bytes (NaN) before the call that has to write it.  att_part, xdec_sync and det_part are never
filled: the chains clear and tag-poll att_part themselves.  Padding (columns R..Rp of alpha / de, V..Vp, the 128-element tails of the mirrors'
rows) is not compared."""
import numpy as np
import torch

import decoder_steps_ref as DR

POISON = 0xFF
A_ = "Decoder/AttentionCell/"
N_EMB, N_START = "Decoder/embedding_table", "Decoder/start_token"
N_ATT_IMG = A_ + "att_img/kernel"
N_INIT = [(A_ + "att_mechanism/W_c_0", A_ + "att_mechanism/b_c_0"), (A_ + "att_mechanism/W_h_0", A_ + "att_mechanism/b_h_0"),
          (A_ + "att_mechanism/W_o_0", A_ + "att_mechanism/b_o_0")]
N_K, N_KB = A_ + "rnn/lstm_cell/kernel", A_ + "rnn/lstm_cell/bias"
N_ATT_H, N_BETA = A_ + "rnn/att_mechanism/dense/kernel", A_ + "rnn/att_mechanism/att_beta"
N_OWH, N_OWC, N_YWO = A_ + "rnn/o_W_h", A_ + "rnn/o_W_c", A_ + "rnn/y_W_o"
N_CONV6_B = "Encoder/convolutional_encoder/conv2d_5/bias"


def random_decoder_params(P, seed, beta_scale=1.5):
    """the decoder's biases and the start token start at zero / a unit vector: random ones of both signs, so that a bias added twice, at the
    wrong place or not at all shows; att_beta scaled up so that the softmax over the regions is not flat (the walk checks max alpha > 3 / R)"""
    rng = np.random.default_rng(seed)
    P = dict(P)
    for k in [N_KB] + [b for _, b in N_INIT]:
        P[k] = (0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    P[N_START] = (0.3 * rng.standard_normal(P[N_START].shape)).astype(np.float32)
    P[N_BETA] = (beta_scale * rng.standard_normal(P[N_BETA].shape)).astype(np.float32)
    return P


def formulas(B, T, V, live_B, seed, first_len=None):
    """[B, T] int32 token ids and [B] lengths: lengths T - 1 and 1 in the first two rows, mixed ones after that (T among them); ids 0 and
    V - 1; ids repeated inside a row and across rows; rows from live_B on are dead (copies of live rows, length 0).
    Only a row of length T has a gradient at step T - 1, so only it carries d_o / d_h / d_c from the last step into T - 2: a batch of
    two live rows has no room for it beside 1 and T - 1, and its case may ask for first_len = T instead of T - 1."""
    rng = np.random.default_rng(seed)
    live = live_B or B
    f = rng.integers(0, V, size=(B, T)).astype(np.int32)
    ln = rng.integers(2, T + 1, size=B).astype(np.int32)
    f[0, 0], f[0, 1 % T] = 0, V - 1
    if T > 3:
        f[0, 3] = f[0, 1]                       # repeated inside a row (both feed a step: positions < T - 1)
    ln[0] = T - 1 if first_len is None else first_len
    if live > 1:
        ln[1] = 1
        f[1, 0] = f[0, 1 % T]                   # ... and across rows
    if live > 2:
        ln[2] = T
        f[2, :] = f[0, :]
        f[2, T - 1] = V - 1
    for b in range(live, B):
        f[b] = f[b % live]
        ln[b] = 0
    return f, ln


def rstep_k_ok(K, bf):
    """csrc/model_decoder.hip: rstep_k_ok"""
    if K % 128:
        return False
    kq = K // 4
    p2 = lambda n: 1 <= n <= 16 and (n & (n - 1)) == 0
    if bf and kq % 64 == 0 and p2(kq // 64):
        return True
    return kq % 32 == 0 and p2(kq // 32)


def fused_steps(step_kernels, bf, U, O, E, C):
    """csrc/model_decoder.hip: fused_steps -- the fused step kernels of rstep.hip run (else the split-K slab kernels)"""
    if step_kernels == 1:
        return False
    return all(rstep_k_ok(k, bf) and rstep_k_ok(k, False) for k in (O + U, U, U + C, O, E, 4 * U, C))


class Checks(object):
    """What a walk of this kind holds its stages with (shared with tests/decode_steps_walk.py): the operands as a GEMM of the mode reads them,
    the bounds of tests/decoder_steps_ref.py, and `worst`, which collects err / bound per check."""

    def __init__(self, io, case):
        self.io, self.case = io, case
        if io.bf:
            self.rel, self.absf = DR.REL_BF16, DR.ABS_BF16
        else:
            self.rel, self.absf = 0.0, DR.ABS_F32
        self.worst = {}

    def q(self, t):
        """an operand as a GEMM of this mode reads it: rounded to bf16 in bf16 mode (weights are packed as bf16, f32 operands are converted
        on load), as it is in the f32 mode"""
        return DR.bf16_round(t) if self.io.bf else DR.f64(t)

    def P(self, name):
        return self.io.params[name].to(self.io.dev, torch.float64)

    def W(self, name):
        return self.q(self.P(name))

    def note(self, what, r):
        self.worst[what] = max(self.worst.get(what, 0.0), r)
        assert r <= 1.0, "%s / %s: err / bound = %.3g" % (self.case, what, r)

    def held(self, what, got, ref, S, rel=None, extra=None):
        rel = self.rel if rel is None else rel
        self.note(what, DR.ratio(got, ref, DR.bound(ref, S, rel, self.absf, extra)))

    def f32_held(self, what, got, ref, S, extra=None):
        """an f32 sum: 2^-14 S in bf16 mode, 2^-20 S in the f32 mode"""
        self.held(what, got, ref, S, rel=0.0, extra=extra)

    def held_b(self, what, got, ref, bnd):
        self.note(what, DR.ratio(got, ref, bnd))

    def mirror(self, what, bits, src):
        """a bf16 mirror: bit for bit the round-to-nearest-even bf16 of its f32 neighbour (src: float64 of the stored f32 values)"""
        want = src.to(torch.float32).to(torch.bfloat16).view(torch.int16)
        bad = bits != want
        assert int(bad.sum()) == 0, "%s / %s: %d mirror elements are not the rounded f32 value, first at %s" % (
            self.case, what, int(bad.sum()), bad.nonzero()[0].tolist())
        self.worst[what] = max(self.worst.get(what, 0.0), 0.0)

    def f32(self, name, shape):
        return self.io.values(name, shape, "f32")

    def report(self):
        print("%s: worst err / bound: %s" % (self.case, ", ".join("%s %.3f" % (k, v) for k, v in self.worst.items())))


class Walk(Checks):
    """One case: forward() checks the stored record, backward() the backward record and every decoder gradient."""

    def __init__(self, io, case, formula_seed=11, first_len=None):
        Checks.__init__(self, io, case)
        self.Vp, self.Dp = (io.V + 31) // 32 * 32, (io.D + 63) // 64 * 64
        self.XH, self.HC = io.O + io.U, io.U + io.C
        self.OFF_HT, self.OFF_CTX, self.REC = io.O + io.U, io.O + 2 * io.U, io.O + 2 * io.U + io.C
        self.fused = fused_steps(io.step_kernels, io.bf, io.U, io.O, io.E, io.C) and not (io.dual and io.B >= 2 and io.B % 2 == 0)
        self.mirr = io.bf and self.fused                     # the bf16 mirrors of the record / g / d_z exist and are what the GEMMs read
        self.expd = io.bf and io.E <= 256 and (io.B * io.R * io.E) % 8 == 0      # csrc/plan.hip: Plan::att_exp
        self.keep_on = 0.0 < io.keep < 1.0
        self.formula, self.lengths = formulas(io.B, io.T, io.V, io.live_B, formula_seed, first_len)
        self.ftor = torch.from_numpy(self.formula).to(io.dev)
        io.set_formula(self.formula, self.lengths)
        self.st = {}

    # ---------------------------------------------------------------------------------------------------------------- helpers --
    def scale(self, which, t, width):
        io = self.io
        return DR.masks(io.keep, io.seed, which, t, io.B, width, io.dev)[0]

    # ---------------------------------------------------------------------------------------------------------------- forward --
    def forward(self):
        io, st = self.io, self.st
        B, T, R, Rp, C, E, U, O, D, V = io.B, io.T, io.R, io.Rp, io.C, io.E, io.U, io.O, io.D, io.V
        XH, HC, OFF_HT, OFF_CTX, REC = self.XH, self.HC, self.OFF_HT, self.OFF_CTX, self.REC
        io.enc_fwd()
        reads = ["att_img", "mean", "emb_in", "zx", "rec", "cs", "gates", "att_h", "alpha", "logits"]
        if io.bf:
            reads += ["att_exp", "recb"]
        for r in reads:
            io.fill(r, POISON)
        io.dec_fwd()
        img = io.values("img", (B, R, C), "ct")
        # ---- set-up
        ref, S = DR.mm(self.q(img), self.W(N_ATT_IMG))
        att_img = io.values("att_img", (B, R, E), "ct")
        self.held("att_img", att_img, ref, S)
        att_x_bwd = att_img                               # what the attention kernels of the recurrence read
        if self.expd:
            ref, bnd = DR.att_exp(att_img)
            att_e = io.values("att_exp", (B, R, E), "bf16")
            self.held_b("att_exp", att_e, ref, bnd)
            att_x_bwd = att_e
        ref, S = DR.rowmean(img)
        mean = self.f32("mean", (B, C))
        self.f32_held("mean", mean, ref, S)
        rec = self.f32("rec", (T + 1, B, REC))
        cs = self.f32("cs", (T + 1, B, U))
        for (wn, bn), what, got in zip(N_INIT, ("c0", "h0", "o0"), (cs[0], rec[0][:, O:O + U], rec[0][:, :O])):
            ref, bnd = DR.tanh_dense(self.q(mean), self.W(wn), self.P(bn), self.absf)
            self.held_b(what, got, ref, bnd)
        rows = DR.embed_rows(self.P(N_EMB), self.P(N_START), self.ftor, T)          # [T, B, D]
        want = torch.zeros(T, B, self.Dp, dtype=torch.float64, device=io.dev)
        want[:, :, :D] = rows
        wbits = want.to(torch.float32)
        wbits = wbits.to(torch.bfloat16).view(torch.int16) if io.bf else wbits.view(torch.int32)
        got = io.bits("emb_in", (T, B, self.Dp), "ct")
        bad = got != wbits
        assert int(bad.sum()) == 0, "%s / emb_in: %d elements are not the gathered row, first at %s" % (self.case, int(bad.sum()), bad.nonzero()[0].tolist())
        self.worst["emb_in"] = 0.0
        emb_in = io.values("emb_in", (T, B, self.Dp), "ct")
        K = self.W(N_K)
        kb = self.P(N_KB)
        ref, S = DR.mm(emb_in[:, :, :D], K[:D])
        zx = self.f32("zx", (T, B, 4 * U))
        self.f32_held("zx", zx, ref + kb, S + kb.abs())
        # ---- the T steps
        gates = self.f32("gates", (T, B, 4 * U))
        att_h = self.f32("att_h", (T, B, E))
        alpha = self.f32("alpha", (T, B, Rp))[:, :, :R]
        recb = io.values("recb", (T + 1, B, REC + 128), "bf16") if self.mirr else None
        recbits = io.bits("recb", (T + 1, B, REC + 128), "bf16") if self.mirr else None
        if self.mirr:
            self.mirror("recb [o|h] 0", recbits[0][:, :XH], rec[0][:, :XH])
        OW = torch.cat([self.W(N_OWH), self.W(N_OWC)], 0)                          # [HC, O]
        WAH, beta = self.W(N_ATT_H), self.P(N_BETA)
        amax = 0.0
        fwd_expd = self.expd and io.chain                  # the launch-per-step forward reads x (cell_step_fused passes att_exp to decode only)
        xtra = DR.PACK28 if io.chain else 0.0
        for t in range(T):
            prev, cur = rec[t], rec[t + 1]
            a = recb[t][:, :XH] if self.mirr else self.q(prev[:, :XH])
            ref, bnd = DR.lstm_gates(zx[t], a, K[D:], self.absf)
            self.held_b("gates", gates[t], ref, bnd)
            ref, bnd = DR.lstm_state(gates[t], cs[t])
            self.held_b("c", cs[t + 1], ref, bnd)
            ref, bnd = DR.lstm_h(gates[t], cs[t + 1])
            self.held_b("h", cur[:, O:O + U], ref, bnd)
            ref, bnd = DR.dropped(cur[:, O:O + U], self.scale(1, t, U))
            self.held_b("h~", cur[:, OFF_HT:OFF_HT + U], ref, bnd)
            a = recb[t + 1][:, OFF_HT:OFF_HT + U] if self.mirr else self.q(cur[:, OFF_HT:OFF_HT + U])
            ref, S = DR.mm(a, WAH)
            self.f32_held("att_h", att_h[t], ref, S)
            tau, _ = DR.tanh_tau(att_e if fwd_expd else att_img, att_h[t], fwd_expd)
            ref, bnd = DR.attention_alpha(tau, beta, self.absf)
            amax = max(amax, float(ref.max()) * R)
            self.held_b("alpha", alpha[t], ref, bnd)
            ref, S = DR.context(alpha[t], img)
            # the chains hand the chunk partials of the context over as 28-bit floats (csrc/xdec.hip:178-186, pack28: relative error 2^-20 each)
            self.f32_held("ctx", cur[:, OFF_CTX:], ref, S, extra=xtra * S)
            a = recb[t + 1][:, OFF_HT:OFF_HT + HC] if self.mirr else self.q(cur[:, OFF_HT:OFF_HT + HC])
            ref, bnd = DR.output_o(a, OW, self.scale(2, t, O), self.absf)
            self.held_b("o", cur[:, :O], ref, bnd)
            if self.mirr:
                self.mirror("recb", recbits[t + 1][:, :REC], cur)
        assert amax > 3.0, "%s: the softmax is flat (max alpha = %.2f / R): scale att_beta up" % (self.case, amax)
        a = recb[1:, :, :O] if self.mirr else self.q(rec[1:, :, :O])
        ref, S = DR.mm(a, self.W(N_YWO))
        logits = self.f32("logits", (T, B, self.Vp))[:, :, :V]
        self.f32_held("logits", logits, ref, S)
        st.update(img=img, att_img=att_img, att_x_bwd=att_x_bwd, mean=mean, rec=rec, cs=cs, recb=recb, emb_in=emb_in, gates=gates, att_h=att_h,
                  alpha=alpha, K=K, OW=OW, WAH=WAH, beta=beta)

    # --------------------------------------------------------------------------------------------------------------- backward --
    def backward(self):
        io, st = self.io, self.st
        B, T, R, Rp, C, E, U, O, D, V = io.B, io.T, io.R, io.Rp, io.C, io.E, io.U, io.O, io.D, io.V
        XH, HC, OFF_HT, OFF_CTX = self.XH, self.HC, self.OFF_HT, self.OFF_CTX
        rec, cs, recb, gates, att_h, alpha, img = st["rec"], st["cs"], st["recb"], st["gates"], st["att_h"], st["alpha"], st["img"]
        K, OW, WAH, beta = st["K"], st["OW"], st["WAH"], st["beta"]
        io.fill("dlogits", POISON)
        io.loss(1.0 / max(int(self.lengths.sum()), 1))
        dlog = io.values("dlogits", (T, B, self.Vp), "ct")[:, :, :V]
        # ---- part 1: from the logits
        io.zero_grads()
        io.fill("do_log", POISON)
        io.dec_bwd(1)
        YWO = self.W(N_YWO)
        ref, S = DR.mm(dlog, YWO.t())
        do_log = self.f32("do_log", (T, B, O))
        self.f32_held("do_log", do_log, ref, S)
        o_all = (recb[1:, :, :O] if self.mirr else self.q(rec[1:, :, :O])).reshape(T * B, O)
        ref, S = DR.mm(o_all.t(), dlog.reshape(T * B, V))
        self.f32_held("d y_W_o", io.grad(N_YWO), ref, S)
        # ---- part 2: the recurrence backwards
        reads = ["g", "dhc", "de", "datth", "dz", "dxh", "dcc", "d_emb", "dpre0", "dmean", "d_att_img", "d_img"]
        if io.bf:
            reads += ["gb", "dzb"]
        if io.chain:
            reads += ["datth_b"]
        for r in reads:
            io.fill(r, POISON)
        io.dec_bwd(2)
        g = self.f32("g", (T, B, O))
        dhc = self.f32("dhc", (T, B, HC))
        de = self.f32("de", (T, B, Rp))[:, :, :R]
        datth = self.f32("datth", (T, B, E))
        dz = self.f32("dz", (T, B, 4 * U))
        if self.mirr:
            gb = io.values("gb", (T, B, O + 128), "bf16")[:, :, :O]
            dzb = io.values("dzb", (T, B, 4 * U + 128), "bf16")[:, :, :4 * U]
            self.mirror("gb", io.bits("gb", (T, B, O + 128), "bf16")[:, :, :O], g)
            self.mirror("dzb", io.bits("dzb", (T, B, 4 * U + 128), "bf16")[:, :, :4 * U], dz)
        else:
            gb, dzb = self.q(g), self.q(dz)
        if io.chain:
            datthb = io.values("datth_b", (T, B, E), "bf16")
            self.mirror("datth_b", io.bits("datth_b", (T, B, E), "bf16"), datth)
        else:
            datthb = self.q(datth)
        xtra = DR.PACK28 if io.chain else 0.0
        dcc_ref = torch.zeros(B, U, dtype=torch.float64, device=io.dev)
        b_dcc = torch.zeros_like(dcc_ref)
        zero_bu = torch.zeros_like(dcc_ref)
        for t in range(T - 1, -1, -1):
            cur = rec[t + 1]
            carry = S_carry = None
            if t < T - 1:
                carry, S_carry = DR.mm(dzb[t + 1], K[D:].t())                      # [B, XH] = [d_o | d_h] carried from step t + 1
            ref, bnd = DR.g_step(do_log[t], None if carry is None else carry[:, :O], None if carry is None else S_carry[:, :O],
                                 cur[:, :O], self.scale(2, t, O), self.keep_on, io.keep, self.absf)
            self.held_b("g", g[t], ref, bnd)
            ref, S = DR.mm(gb[t], OW.t())                                          # [B, HC] = [d_h~ | d_ctx]
            if self.fused:
                self.f32_held("dhc", dhc[t], ref, S)
                dhm, b_dhm = dhc[t][:, :U], zero_bu
            else:                                                                   # split-K: only the d_ctx half is stored (for the deferred d_img)
                self.f32_held("dhc d_ctx", dhc[t][:, U:], ref[:, U:], S[:, U:])
                dhm, b_dhm = ref[:, :U], self.absf * S[:, :U]
            d_ctx = dhc[t][:, U:]
            ref, bnd = DR.attention_bwd(alpha[t], img, d_ctx, cur[:, OFF_CTX:], self.absf)
            self.held_b("de", de[t], ref, bnd)
            _, dtau = DR.tanh_tau(st["att_x_bwd"], att_h[t], self.expd)
            ref, bnd = DR.datt_h(de[t], dtau, beta, self.absf)
            # the backward chain hands the chunk partials of d_att_h over as 28-bit floats (csrc/xdec.hip:1473-1476)
            self.held_b("datth", datth[t], ref, bnd + xtra * self._datth_terms(de[t], dtau, beta))
            v, S_v = DR.mm(datthb[t], WAH.t())
            (ref, bnd), (dcc_ref, b_dcc) = DR.lstm_bwd(dhm, b_dhm, v, S_v, None if carry is None else carry[:, O:],
                                                       None if carry is None else S_carry[:, O:], self.scale(1, t, U), gates[t], cs[t + 1], cs[t],
                                                       dcc_ref, b_dcc, self.absf)
            self.held_b("dz", dz[t], ref, bnd)
        if io.live_B and io.live_B < B:
            # a dead row (length 0) is outside the loss mask: its d(logits) and with it every per-row gradient of the record is an exact zero.
            # (Nothing of a dead row may be NaN instead: the kernels multiply by that zero, they do not skip the row.)
            for what, t_ in (("dlogits", dlog), ("g", g), ("dhc d_ctx", dhc[:, :, U:]), ("de", de), ("datth", datth), ("dz", dz)):
                assert int((t_[:, io.live_B:] != 0).sum()) == 0, "%s: dead rows of %s are not zeros" % (self.case, what)
        dcc = self.f32("dcc", (B, U))
        self.held_b("dcc", dcc, dcc_ref, b_dcc)
        ref, S = DR.mm(dzb[0], K[D:].t())
        dxh = self.f32("dxh", (B, XH))
        self.f32_held("dxh", dxh, ref, S)
        # ---- initial state
        ref, bnd = DR.init_bwd(dcc, dxh, cs[0], rec[0], U, O)
        dpre = self.f32("dpre0", (B, 2 * U + O))
        self.held_b("dpre0", dpre, ref, bnd)
        parts = (dpre[:, :U], dpre[:, U:2 * U], dpre[:, 2 * U:])
        ref = S = 0.0
        for (wn, bn), d in zip(N_INIT, parts):
            r_, s_ = DR.mm(self.q(d), self.W(wn).t())
            ref, S = ref + r_, S + s_
            r_, s_ = DR.mm(self.q(st["mean"]).t(), self.q(d))
            self.f32_held("dW_0", io.grad(wn), r_, s_)
            r_, s_ = DR.colsum(d)
            self.f32_held("db_0", io.grad(bn), r_, s_)
        dmean = self.f32("dmean", (B, C))
        self.f32_held("dmean", dmean, ref, S)
        # ---- deferred weight gradients
        TB = T * B
        hc_all = (recb[1:, :, OFF_HT:OFF_HT + HC] if self.mirr else self.q(rec[1:, :, OFF_HT:OFF_HT + HC])).reshape(TB, HC)
        ref, S = DR.mm(hc_all.t(), gb.reshape(TB, O))
        got = torch.cat([io.grad(N_OWH), io.grad(N_OWC)], 0)
        self.f32_held("d o_W", got, ref, S)
        ref, S = DR.mm(hc_all[:, :U].t(), datthb.reshape(TB, E))
        self.f32_held("dW_att_h", io.grad(N_ATT_H), ref, S)
        xh_all = (recb[:T, :, :XH] if self.mirr else self.q(rec[:T, :, :XH])).reshape(TB, XH)
        dz_all = dzb.reshape(TB, 4 * U)
        r0, s0 = DR.mm(st["emb_in"][:, :, :D].reshape(TB, D).t(), dz_all)
        r1, s1 = DR.mm(xh_all.t(), dz_all)
        self.f32_held("dK", io.grad(N_K), torch.cat([r0, r1], 0), torch.cat([s0, s1], 0))
        ref, S = DR.colsum(dz)
        self.f32_held("d lstm bias", io.grad(N_KB), ref, S)
        ref, S = DR.mm(dzb, K[:D].t())
        demb = self.f32("d_emb", (T, B, D))
        self.f32_held("d_emb", demb, ref, S)
        (rt, stt), (rs, ss) = DR.embed_scatter(demb, self.ftor, V)
        self.f32_held("d embedding_table", io.grad(N_EMB), rt, stt)
        self.f32_held("d start_token", io.grad(N_START).reshape(-1), rs, ss)
        # ---- towards the encoder
        (ref, bnd), (db, Sdb) = DR.datt_img(de, st["att_img"], att_h, beta, self.absf, io.bf)
        datt = io.values("d_att_img", (B, R, E), "ct")
        self.held_b("d_att_img", datt, ref, bnd + self.rel * ref.abs())
        self.f32_held("d_beta", io.grad(N_BETA).reshape(-1), db, Sdb)
        ref, S = DR.mm(self.q(img).reshape(B * R, C).t(), datt.reshape(B * R, E))
        self.f32_held("dW_att_img", io.grad(N_ATT_IMG), ref, S)
        al, dc = (self.q(alpha), self.q(dhc[:, :, U:])) if io.dimg_bf else (alpha, dhc[:, :, U:])      # dimg.hip packs both to bf16 for the MFMAs
        ref = torch.einsum("tbr,tbc->brc", al, dc)
        S = torch.einsum("tbr,tbc->brc", al.abs(), dc.abs())
        r_, s_ = DR.mm(datt, self.W(N_ATT_IMG).t())
        ref = ref + dmean[:, None, :] / R + r_
        S = S + dmean.abs()[:, None, :] / R + s_
        if io.dimg_bf:
            on = io.values("y6", (B, R, C), "ct") > 0
            zero = torch.zeros((), dtype=torch.float64, device=io.dev)
            ref, S = torch.where(on, ref, zero), torch.where(on, S, zero)
            got = io.values("d_img", (B, R, C), "bf16")
            self.held("d_img", got, ref, S, rel=DR.REL_BF16)
            self.f32_held("d conv6 bias", io.grad(N_CONV6_B), ref.reshape(-1, C).sum(0), S.reshape(-1, C).sum(0))
        else:
            got = self.f32("d_img", (B, R, C))
            self.f32_held("d_img", got, ref, S)
        if io.live_B and io.live_B < B:
            assert int((got[io.live_B:] != 0).sum()) == 0, "%s: dead rows of d_img are not zeros" % self.case

    def _datth_terms(self, de_t, dtau, beta):
        return DR.f64(beta).reshape(1, -1).abs() * torch.einsum("br,brk->bk", DR.f64(de_t).abs(), dtau.abs())
