"""TEST INFRASTRUCTURE: walks the decode step stage by stage through an adapter and checks every workspace region it stores against
tests/decoder_steps_ref.py applied to the operands the kernels themselves read -- the decode-side sibling of tests/decoder_steps_walk.py,
whose parameter names, random_decoder_params, fused_steps and Checks (held / f32_held / held_b / mirror / note / report) it uses.

Sequence of DecodeWalk.run(): encoder forward once; lxo_decode_begin -> att_img, att_exp, mean, the initial states (tiled over the beam), the
token table; then per step lxo_decode_cell_step(time) from the stored state -> c, h, h~, att_h, alpha, ctx, o, the mirror, the logits and
the untouched read slot; lxo_decode_step(time) from the same state -> the select against a float64 select on the stored logits, beam_lp, the
re-ordered rows, dec_ids.  At one step the ids (0, V - 1, a repeated one, different ones inside a beam) and h / o are given through
lxo_decode_state_set.  beam_last(m) checks step m of a whole lxo_beam_decode_scores loop (the parent indirection of the fused path, or the
re-ordering launch), chain_last(m) step m of the persistent greedy-decode chain (xdec_dec_kernel) and its tail.

What xdec_dec_kernel stores at its last step: c, h, h~, ctx, o and their mirrors (csrc/xdec.hip: the LSTM phase, xdec_p4_merge, xdec_o_proj)
-- every value chain_last() holds; att_h, alpha and the logits are never stored, so ctx is held through the propagated bound of
decoder_steps_ref.context_from_att_h and the tail through the emitted id and log-prob.

The adapter `io` offers what the training adapters offer -- bf, B, R, Rp, C, E, U, O, D, V, dev, params, values(region, shape, kind),
bits(region, shape, kind), write(region, tensor), fill(region, byte, offset = 0, count = None: bytes), step_kernels -- and k (hypotheses per
image), indirect (the whole beam loop reads through the parents where the step kernels are fused), enc_fwd(), begin(), cell_step(time,
start), step(time, id_end) -> (ids, parents), set_state(time, c, h, o, ids), greedy(max_iter, scores) -> (ids, logp, steps, chain_used,
chain_err), beam(max_iter) -> (ids, parents, scores, steps).  EngineIO below is that adapter on a latex_ocr_amd Engine -- bound to the hipsim
build on the CPU or to the library on the GPU.

Every region a call must write is filled with 0xFF bytes (NaN) before that call: the slot being written, not the slot being read.  Padding
(columns R..Rp of alpha, V..Vp of dec_logits, the 128-element tails of recb rows) is not compared."""
import ctypes
import os

import numpy as np
import torch
import torch.nn.functional as F

import decoder_steps_ref as DR
import decoder_steps_walk as DW
import encoder_layers_walk as EW
from output_head_ref import logp_tol
from oracle.ref_model import _top_k_lowest_index

POISON = DW.POISON


class EngineIO(object):
    """the walk's adapter on an Engine (e.step_kernels is set by the caller before)"""

    def __init__(self, e, B, H, W, k=1, seed=3):
        from latex_ocr_amd.engine import _p
        self._p, self.e = _p, e
        self.cuda = e.device.type == "cuda"
        e.load_params(DW.random_decoder_params(EW.random_biases(e.get_params(), seed + 1), seed + 2))
        d = e.dims
        self.bf, self.B, self.k = e.dtype == 1, B, k
        self.C, self.E, self.U, self.O, self.D, self.V = d["C"], d["E"], d["U"], d["O"], d["D"], e.n_tok
        cd8 = lambda n: -(-n // 8)
        self.R = (cd8(H) - 2) * (cd8(W) - 2)
        self.Rp = (self.R + 7) // 8 * 8
        self.step_kernels = e.step_kernels
        self.indirect = not os.environ.get("LXO_BEAM_INDIRECT", "1").startswith("0")      # read as lxo_impl_beam_decode reads it
        self.dev = e.device
        self.img = torch.from_numpy(np.ascontiguousarray(EW.images("plain", B, H, W, seed))).to(self.dev)
        self.params = {n: torch.from_numpy(v) for n, v in e.get_params().items()}

    def _sync(self):
        if self.cuda:
            torch.cuda.synchronize()

    def enc_fwd(self):
        e = self.e
        e._encode_only(self.img, self.k)
        e._set_diversity(1.0, 0.0, 0)
        shp = (self.B, e.max_steps) if self.k == 1 else (self.B, e.max_steps, self.k)
        e._dec_ids = torch.zeros(*shp, dtype=torch.int32, device=self.dev)
        e._dec_par = torch.zeros(*shp, dtype=torch.int32, device=self.dev) if self.k > 1 else None
        e._dec_fin = np.zeros(self.B * self.k, dtype=np.int32)
        self._sync()

    def begin(self):
        e, _p = self.e, self._p
        e._ck(e.lib.lxo_decode_begin(e.sref(), _p(e.params), _p(e.wpack), _p(e.ws), e._stream()), "decode_begin")
        self._sync()

    def cell_step(self, time, start):
        self.e.decode_cell_step(time, start)
        self._sync()

    def step(self, time, id_end):
        ids, par, _, _ = self.e.decode_step(time, id_end)
        self._sync()
        return ids, par

    def set_state(self, time, c=None, h=None, o=None, ids=None):
        self.e.decode_set_state(time, c=c, h=h, o=o, ids=ids)
        self._sync()

    def greedy(self, max_iter, scores=True):
        out = self.e.greedy_decode(self.img, self.V - 1, max_iter=max_iter, return_scores=scores)
        ids, logp = out if scores else (out, None)
        self._sync()
        used, err = self.e.chain_status() if self.bf else (False, 0)
        return ids, logp, ids.shape[1], used, err

    def beam(self, max_iter):
        ids, par, sc = self.e.beam_decode(self.img, self.V - 1, self.k, max_iter=max_iter, return_scores=True)
        self._sync()
        return ids, par, sc, ids.shape[1]

    def _raw(self, name):
        e = self.e
        off, nb = ctypes.c_size_t(), ctypes.c_size_t()
        e._ck(e.lib.lxo_ws_region(e.sref(), name.encode(), ctypes.byref(off), ctypes.byref(nb)), "ws_region")
        return e.ws[off.value:off.value + nb.value]

    def _view(self, name, shape, dt):
        return self._raw(name).view(dt)[:int(np.prod(shape))].view(*shape)

    def _bf(self, kind):
        return kind == "bf16" or (kind == "ct" and self.bf)

    def values(self, name, shape, kind="f32"):
        return self._view(name, shape, torch.bfloat16 if self._bf(kind) else torch.float32).to(torch.float64)

    def bits(self, name, shape, kind="f32"):
        return self._view(name, shape, torch.int16 if self._bf(kind) else torch.int32).clone()

    def write(self, name, t):
        raw = t.contiguous().view(torch.uint8).reshape(-1)
        dst = self._raw(name)
        assert raw.numel() <= dst.numel()
        dst[:raw.numel()].copy_(raw)

    def fill(self, name, byte, offset=0, count=None):
        raw = self._raw(name)
        end = raw.numel() if count is None else offset + count
        assert 0 <= offset and end <= raw.numel(), (name, offset, end, raw.numel())
        raw[offset:end].fill_(byte)


def forced_ids(B, k, V):
    """ids to feed in place of the model's own: 0 and V - 1, one id repeated across rows, different ids inside one image's beam"""
    nv = B * k
    ids = np.full(nv, (V // 2) | 1, np.int32)                 # the repeated one
    if k > 1:
        ids[nv - k:] = (np.arange(k) * 7 + 3) % V            # the last image: k different ids (V - 1 among them, below)
    elif nv < 4:
        ids[:] = V - 1                                       # too few rows for a third id: V - 1 is the repeated one
    ids[0], ids[nv - 1] = 0, V - 1
    return ids


class DecodeWalk(DW.Checks):
    """One case: run(steps), beam_last(m) or chain_last(m); `worst` collects err / bound per check."""

    def __init__(self, io, case):
        DW.Checks.__init__(self, io, case)
        self.k, self.nv = io.k, io.B * io.k
        self.Vp, self.Dp = (io.V + 31) // 32 * 32, (io.D + 63) // 64 * 64
        self.XH, self.HC = io.O + io.U, io.U + io.C
        self.OFF_HT, self.OFF_CTX, self.REC = io.O + io.U, io.O + 2 * io.U, io.O + 2 * io.U + io.C
        self.RECB = self.REC + 128
        self.fused = DW.fused_steps(io.step_kernels, io.bf, io.U, io.O, io.E, io.C)
        self.mirr = io.bf and self.fused                     # the bf16 mirror of the state slots exists and is what the step GEMMs read
        self.has_exp = io.bf and io.E <= 256 and (io.B * io.R * io.E) % 8 == 0      # csrc/plan.hip: Plan::att_exp
        self.expd = self.has_exp and self.fused              # cell_step_fused passes att_exp to every decode; the split-K step reads x
        self.id_end = io.V - 1
        self.img_of = torch.arange(self.nv, device=io.dev) // self.k             # row v reads image v // k
        self.amax = 0.0
        self.st = {}

    # ---------------------------------------------------------------------------------------------------------------- helpers --
    def same(self, what, got, want):
        bad = got != want
        assert int(bad.sum()) == 0, "%s / %s: %d elements differ bit for bit, first at %s" % (self.case, what, int(bad.sum()), bad.nonzero()[0].tolist())
        self.worst[what] = max(self.worst.get(what, 0.0), 0.0)

    def slot_bits(self, s):
        """the raw contents of state slot s: rec, cs (and recb)"""
        io, nv = self.io, self.nv
        d = dict(rec=io.bits("rec", (2, nv, self.REC))[s], cs=io.bits("cs", (2, nv, io.U))[s])
        if self.mirr:
            d["recb"] = io.bits("recb", (2, nv, self.RECB), "bf16")[s][:, :self.REC]
        return d

    def slot(self, s):
        """state slot s as float64 values (+ the mirror's values and bits)"""
        io, nv = self.io, self.nv
        d = dict(rec=io.values("rec", (2, nv, self.REC))[s], cs=io.values("cs", (2, nv, io.U))[s], recb=None, recbits=None)
        if self.mirr:
            d["recb"] = io.values("recb", (2, nv, self.RECB), "bf16")[s][:, :self.REC]
            d["recbits"] = io.bits("recb", (2, nv, self.RECB), "bf16")[s][:, :self.REC]
        return d

    def fill_slot(self, s):
        io, nv = self.io, self.nv
        io.fill("rec", POISON, s * nv * self.REC * 4, nv * self.REC * 4)
        io.fill("cs", POISON, s * nv * io.U * 4, nv * io.U * 4)
        if self.mirr:
            io.fill("recb", POISON, s * nv * self.RECB * 2, nv * self.RECB * 2)

    def fill_step_outputs(self, time):
        io = self.io
        self.fill_slot((time + 1) & 1)
        for r in ["att_h", "alpha", "dec_logits"] + ([] if self.fused else ["dec_emb", "dec_zx"]):
            io.fill(r, POISON)

    def weights(self):
        if "K" not in self.st:
            self.st.update(K=self.W(DW.N_K), kb=self.P(DW.N_KB), OW=torch.cat([self.W(DW.N_OWH), self.W(DW.N_OWC)], 0), WAH=self.W(DW.N_ATT_H),
                           beta=self.P(DW.N_BETA), YWO=self.W(DW.N_YWO))
        return self.st

    # ----------------------------------------------------------------------------------------------------------------- set-up --
    def setup(self):
        io, st = self.io, self.st
        B, R, C, E, U, O, D, V, k, nv = io.B, io.R, io.C, io.E, io.U, io.O, io.D, io.V, self.k, self.nv
        io.enc_fwd()
        reads = ["att_img", "mean", "rec", "cs"] + (["att_exp"] if self.has_exp else []) + (["recb"] if self.mirr else [])
        reads += ["dec_tx", "dec_txe"] if self.fused else []
        for r in reads:
            io.fill(r, POISON)
        io.begin()
        self.check_setup()
        s0 = self.slot(0)
        for (wn, bn), what, got in zip(DW.N_INIT, ("c0", "h0", "o0"), (s0["cs"], s0["rec"][:, O:O + U], s0["rec"][:, :O])):
            ref, bnd = DR.tanh_dense(self.q(st["mean"]), self.W(wn), self.P(bn), self.absf)
            self.held_b(what, got, ref[self.img_of], bnd[self.img_of])
        b0 = self.slot_bits(0)
        first = self.img_of * k                                                     # row b k + j = row b k, bit for bit
        self.same("tiled c0", b0["cs"], b0["cs"][first])
        self.same("tiled [o|h] 0", b0["rec"][:, :self.XH], b0["rec"][first][:, :self.XH])
        if self.mirr:
            self.mirror("recb [o|h] 0", b0["recb"][:, :self.XH], s0["rec"][:, :self.XH])
        if self.fused:
            self.check_table()

    def check_setup(self):
        """att_img, att_exp and mean, as the training walk holds them"""
        io, st = self.io, self.st
        B, R, C, E = io.B, io.R, io.C, io.E
        img = io.values("img", (B, R, C), "ct")
        ref, S = DR.mm(self.q(img), self.W(DW.N_ATT_IMG))
        att_img = io.values("att_img", (B, R, E), "ct")
        self.held("att_img", att_img, ref, S)
        att_e = None
        if self.has_exp:
            ref, bnd = DR.att_exp(att_img)
            att_e = io.values("att_exp", (B, R, E), "bf16")
            self.held_b("att_exp", att_e, ref, bnd)
        ref, S = DR.rowmean(img)
        mean = self.f32("mean", (B, C))
        self.f32_held("mean", mean, ref, S)
        st.update(img=img, att_img=att_img, att_e=att_e, mean=mean)

    def check_table(self):
        io, st = self.io, self.st
        U, D, V = io.U, io.D, io.V
        w = self.weights()
        want = DR.token_table(self.P(DW.N_EMB), self.P(DW.N_START), self.Dp).to(torch.float32)
        want = want.to(torch.bfloat16).view(torch.int16) if io.bf else want.view(torch.int32)
        self.same("dec_txe", io.bits("dec_txe", (V + 1, self.Dp), "ct"), want)
        txe = io.values("dec_txe", (V + 1, self.Dp), "ct")
        ref, S = DR.mm(txe[:, :D], w["K"][:D])
        st["dec_tx"] = self.f32("dec_tx", (V + 1, 4 * U))
        self.f32_held("dec_tx", st["dec_tx"], ref + w["kb"], S + w["kb"].abs())

    # ------------------------------------------------------------------------------------------------------------- one cell step --
    def step_input(self, ids_prev):
        """zx as the LSTM kernel reads it: the table row of the previous id (row V at the start step) on the fused path; on the split-K path the
        stored dec_zx, behind dec_emb gathered bit for bit"""
        io, st = self.io, self.st
        U, D, V, nv = io.U, io.D, io.V, self.nv
        w = self.weights()
        rows = torch.full((nv,), V, dtype=torch.long, device=io.dev) if ids_prev is None else ids_prev.long().clamp(0, V - 1)
        if self.fused:
            return st["dec_tx"][rows]
        want = DR.token_table(self.P(DW.N_EMB), self.P(DW.N_START), self.Dp)[rows].to(torch.float32)
        want = want.to(torch.bfloat16).view(torch.int16) if io.bf else want.view(torch.int32)
        self.same("dec_emb", io.bits("dec_emb", (nv, self.Dp), "ct"), want)
        emb = io.values("dec_emb", (nv, self.Dp), "ct")
        ref, S = DR.mm(emb[:, :D], w["K"][:D])
        zx = self.f32("dec_zx", (nv, 4 * U))
        self.f32_held("dec_zx", zx, ref + w["kb"], S + w["kb"].abs())
        return zx

    def check_cell(self, zx, prev, cur, att_h, alpha, logits, cur_map=None):
        """One step on the operands it read.  prev / cur: dicts of slot() -- prev already in the order the rows were read in (through the parents
        where the loop reads them in place).  cur_map (the whole loop with the re-ordering launch): [o | h], c and their mirror in `cur` are
        re-ordered, row r holds the step's row cur_map[r]; h~, ctx, att_h, alpha and the logits are not."""
        io, st = self.io, self.st
        U, O, R, V = io.U, io.O, io.R, io.V
        XH, HC, OFF_HT, OFF_CTX = self.XH, self.HC, self.OFF_HT, self.OFF_CTX
        w = self.weights()
        ident = torch.arange(self.nv, device=io.dev)
        cm = ident if cur_map is None else cur_map
        rec = cur["rec"]
        a = prev["recb"][:, :XH] if self.mirr else self.q(prev["rec"][:, :XH])
        gates, b_g = DR.lstm_gates(zx, a, w["K"][io.D:], self.absf)
        ref, bnd = DR.lstm_state_from(gates, b_g, prev["cs"])
        self.held_b("c", cur["cs"], ref[cm], bnd[cm])
        ref, bnd = DR.lstm_h_from(gates[cm], b_g[cm], cur["cs"])
        self.held_b("h", rec[:, O:O + U], ref, bnd)
        hbits = rec[:, O:O + U].to(torch.float32).view(torch.int32)
        self.same("h~", rec[:, OFF_HT:OFF_HT + U].to(torch.float32).view(torch.int32)[cm], hbits)      # no dropout in decode
        if att_h is not None:
            a = cur["recb"][:, OFF_HT:OFF_HT + U] if self.mirr else self.q(rec[:, OFF_HT:OFF_HT + U])
            ref, S = DR.mm(a, w["WAH"])
            self.f32_held("att_h", att_h, ref, S)
            att_x = (st["att_e"] if self.expd else st["att_img"])[self.img_of]
            tau, _ = DR.tanh_tau(att_x, att_h, self.expd)
            ref, bnd = DR.attention_alpha(tau, w["beta"], self.absf)
            self.amax = max(self.amax, float(ref.max()) * R)
            self.held_b("alpha", alpha, ref, bnd)
            ref, S = DR.context(alpha, st["img"][self.img_of])
            self.f32_held("ctx", rec[:, OFF_CTX:], ref, S)
        a = cur["recb"][:, OFF_HT:OFF_HT + HC] if self.mirr else self.q(rec[:, OFF_HT:OFF_HT + HC])
        ref, bnd = DR.output_o(a, w["OW"], 1.0, self.absf)
        self.held_b("o", rec[:, :O], ref[cm], bnd[cm])
        if self.mirr:
            self.mirror("recb", cur["recbits"], rec)
        if logits is not None:
            a = cur["recb"][:, :O] if self.mirr else self.q(rec[:, :O])
            ref, S = DR.mm(a, w["YWO"])
            self.f32_held("dec_logits", logits[cm], ref, S)                            # (re-ordered: the rows that survived as parents)

    def cell(self, time, ids_prev):
        """lxo_decode_cell_step(time) from the stored state of slot time & 1"""
        io = self.io
        sp, sn = time & 1, (time + 1) & 1
        before = self.slot_bits(sp)
        self.fill_step_outputs(time)
        io.cell_step(time, ids_prev is None)
        zx = self.step_input(ids_prev)
        cur = self.slot(sn)
        att_h = self.f32("att_h", (self.nv, io.E))
        alpha = self.f32("alpha", (self.nv, io.Rp))[:, :io.R]
        logits = self.f32("dec_logits", (self.nv, self.Vp))[:, :io.V]
        self.check_cell(zx, self.slot(sp), cur, att_h, alpha, logits)
        after = self.slot_bits(sp)
        for n in before:
            self.same("read slot untouched (%s)" % n, after[n], before[n])
        return logits, self.slot_bits(sn)

    # ---------------------------------------------------------------------------------------------------------------- the select --
    def select_ref(self, time, logits, lp_prev, fin_prev, beam):
        """float64 select on the stored logits: -> (ids, parents, running log-probs) [B, k]; exact ties as _top_k_lowest_index takes them"""
        io, k, V = self.io, self.k, self.io.V
        lg = logits.to("cpu", torch.float64)
        if not beam:
            _, idx = _top_k_lowest_index(lg, 1)
            return idx, None, None
        step_lp = F.log_softmax(lg.reshape(io.B, k, V), dim=-1)
        one_hot = torch.full((V,), float(torch.finfo(torch.float32).min), dtype=torch.float64)
        one_hot[self.id_end] = 0.0
        fin = fin_prev.to(torch.float64)[:, :, None]
        step_lp = (1.0 - fin) * step_lp + fin * one_hot
        lp = lp_prev[:, :, None] + step_lp
        flat = lp.reshape(io.B, k * V) if time > 0 else lp[:, 0]
        vals, idx = _top_k_lowest_index(flat, k)
        return idx % V, idx // V, vals

    def select(self, time, logits, left, lp_prev, fin_prev):
        """lxo_decode_step(time) from the same untouched state: the choice, beam_lp, the re-ordered rows, dec_ids"""
        io, k, nv = self.io, self.k, self.nv
        sp, sn = time & 1, (time + 1) & 1
        before = self.slot_bits(sp)
        self.fill_step_outputs(time)
        ids, par = io.step(time, self.id_end)
        ids = torch.from_numpy(np.asarray(ids)).long().reshape(io.B, k)
        again = self.f32("dec_logits", (nv, self.Vp))[:, :io.V]
        self.same("dec_logits again", again.to(torch.float32).view(torch.int32), logits.to(torch.float32).view(torch.int32))
        r_ids, r_par, r_lp = self.select_ref(time, logits, lp_prev, fin_prev, k > 1)
        self.same("ids", ids, r_ids.reshape(io.B, k))
        got = self.slot_bits(sn)
        if k > 1:
            par = torch.from_numpy(np.asarray(par)).long().reshape(io.B, k)
            self.same("parents", par, r_par)
            lp = self.f32("beam_lp", (nv,)).reshape(io.B, k).cpu()
            self.note("beam_lp", float((lp - r_lp).abs().max()) / logp_tol(logits.cpu().numpy()))
            self.same("beam_par", io.bits("beam_par", (nv,)).reshape(io.B, k).cpu().long(), par)
            src = (self.img_of * k + par.reshape(-1).to(io.dev))
            XH = self.XH
            self.same("re-ordered [o|h]", got["rec"][:, :XH], left["rec"][src][:, :XH])
            self.same("re-ordered c", got["cs"], left["cs"][src])
            self.same("rest of the record", got["rec"][:, XH:], left["rec"][:, XH:])
            if self.mirr:
                self.same("re-ordered mirror [o|h]", got["recb"][:, :XH], left["recb"][src][:, :XH])
                self.same("rest of the mirror", got["recb"][:, XH:], left["recb"][:, XH:])
            fin = torch.gather(fin_prev, 1, par) | (ids == self.id_end)
        else:
            for n in got:
                self.same("slot unchanged (%s)" % n, got[n], left[n])
            lp, fin = lp_prev, fin_prev | (ids == self.id_end)
        self.same("dec_ids", io.bits("dec_ids", (nv,)).reshape(io.B, k).cpu().long(), ids)
        after = self.slot_bits(sp)
        for n in before:
            self.same("read slot untouched by the step (%s)" % n, after[n], before[n])
        return ids, lp.to(torch.float64), fin

    # ------------------------------------------------------------------------------------------------------- ids and state given --
    def force(self, time):
        """lxo_decode_state_set: ids of the walk's choosing, and h / o of its choosing -- the mirror of [o | h] follows"""
        io, nv = self.io, self.nv
        s = time & 1
        ids = forced_ids(io.B, self.k, io.V)
        rng = np.random.default_rng(17)
        h = rng.uniform(-0.9, 0.9, size=(nv, io.U)).astype(np.float32)
        o = rng.uniform(-0.9, 0.9, size=(nv, io.O)).astype(np.float32)
        cs_before = self.slot_bits(s)["cs"]
        if self.mirr:
            io.fill("recb", POISON, s * nv * self.RECB * 2, nv * self.RECB * 2)
        io.set_state(time, h=h, o=o, ids=ids)
        got, gb = self.slot(s), self.slot_bits(s)
        want = torch.from_numpy(np.concatenate([o, h], 1)).to(io.dev)
        self.same("set_state [o|h]", gb["rec"][:, :self.XH], want.view(torch.int32))
        self.same("set_state leaves c", gb["cs"], cs_before)
        if self.mirr:
            self.mirror("set_state recb [o|h]", gb["recb"][:, :self.XH], got["rec"][:, :self.XH])
        self.same("set_state dec_ids", io.bits("dec_ids", (nv,)).cpu(), torch.from_numpy(ids))
        return torch.from_numpy(ids).to(io.dev)

    def run(self, steps, force_at=None):
        io = self.io
        self.setup()
        lp = torch.zeros(io.B, self.k, dtype=torch.float64)
        fin = torch.zeros(io.B, self.k, dtype=torch.bool)
        ids = None
        for t in range(steps):
            ids_prev = None if t == 0 else ids.reshape(-1).to(io.dev)
            if t == force_at:
                ids_prev = self.force(t)
            logits, left = self.cell(t, ids_prev)
            ids, lp, fin = self.select(t, logits, left, lp, fin)
        self.not_flat()

    def not_flat(self):
        assert self.amax > 3.0, "%s: the softmax is flat (max alpha = %.2f / R): scale att_beta up" % (self.case, self.amax)

    # ------------------------------------------------------------------------------------------------- last step of a whole loop --
    def fill_loop(self):
        io = self.io
        io.enc_fwd()
        reads = ["att_img", "mean", "rec", "cs", "att_h", "alpha", "dec_logits"] + (["att_exp"] if self.has_exp else []) + (["recb"] if self.mirr else [])
        reads += ["dec_tx", "dec_txe"] if self.fused else ["dec_emb", "dec_zx"]
        for r in reads:
            io.fill(r, POISON)

    def beam_last(self, m):
        """step m of lxo_beam_decode_scores(max_iter = m): on the fused path row b k + j read its state at row b k + parents[b, m - 1, j] of the
        un-re-ordered slot m & 1; with the re-ordering launch (split-K, LXO_BEAM_INDIRECT=0) both slots hold re-ordered rows"""
        io, k, V = self.io, self.k, self.io.V
        assert m >= 2 and k > 1
        self.fill_loop()
        ids, par, sc, steps = io.beam(m)
        assert steps == m + 1, "%s: the loop ran %d steps, not to its bound of %d" % (self.case, steps, m + 1)
        ids, par = torch.from_numpy(np.asarray(ids)).long(), torch.from_numpy(np.asarray(par)).long()          # [B, steps, k]
        sc = torch.from_numpy(np.asarray(sc)).to(torch.float64)
        pp = par[:, m - 1]
        assert bool((pp != torch.arange(k)).any()), "%s: every parent row of step %d is the identity" % (self.case, m - 1)
        assert any(len(set(r)) < k for r in pp.tolist()), "%s: no image repeats a parent at step %d" % (self.case, m - 1)
        self.check_setup()
        if self.fused:
            self.check_table()
        prev, cur = self.slot(m & 1), self.slot((m + 1) & 1)
        cur_map = None
        if self.fused and io.indirect:
            src = self.img_of * k + pp.reshape(-1).to(io.dev)
            prev = {n: (v[src] if v is not None else None) for n, v in prev.items()}
        else:
            cur_map = self.img_of * k + par[:, m].reshape(-1).to(io.dev)
        zx = self.step_input(ids[:, m - 1].reshape(-1).to(io.dev))
        att_h = self.f32("att_h", (self.nv, io.E))
        alpha = self.f32("alpha", (self.nv, io.Rp))[:, :io.R]
        logits = self.f32("dec_logits", (self.nv, self.Vp))[:, :V]
        self.check_cell(zx, prev, cur, att_h, alpha, logits, cur_map)
        fin = torch.zeros(io.B, k, dtype=torch.bool)
        for t in range(m):
            fin = torch.gather(fin, 1, par[:, t]) | (ids[:, t] == self.id_end)
        r_ids, r_par, r_lp = self.select_ref(m, logits, sc[:, m - 1], fin, True)
        self.same("ids", ids[:, m], r_ids)
        self.same("parents", par[:, m], r_par)
        self.note("scores", float((sc[:, m] - r_lp).abs().max()) / logp_tol(logits.cpu().numpy()))
        self.not_flat()

    # ------------------------------------------------------------------------------- last step of the persistent greedy-decode chain --
    def chain_last(self, m):
        """step m of lxo_greedy_decode_scores(max_iter = m) on xdec_dec_kernel, and its tail (logits, arg-max and log-prob at the boundary
        behind the step)"""
        io, st = self.io, self.st
        U, O, V = io.U, io.O, io.V
        assert self.k == 1 and self.mirr and self.has_exp
        self.fill_loop()
        ids, logp, steps, used, err = io.greedy(m, True)
        assert used and err == 0, "%s: the chain did not run cleanly (used %s, error word %d)" % (self.case, used, err)
        assert steps == m + 1, "%s: the loop ran %d steps, not to its bound of %d" % (self.case, steps, m + 1)
        ids = torch.from_numpy(np.asarray(ids)).long().to(io.dev)
        logp = torch.from_numpy(np.asarray(logp)).to(io.dev, torch.float64)
        self.check_setup()
        self.check_table()
        w = self.weights()
        prev, cur = self.slot(m & 1), self.slot((m + 1) & 1)
        zx = self.step_input(None if m == 0 else ids[:, m - 1])
        self.check_cell(zx, prev, cur, None, None, None)
        att_h, S_h = DR.mm(cur["recb"][:, self.OFF_HT:self.OFF_HT + U], w["WAH"])
        att_x, img = st["att_e"][self.img_of], st["img"][self.img_of]
        al, _ = DR.attention_alpha(DR.tanh_tau(att_x, att_h, True)[0], w["beta"], self.absf)
        self.amax = max(self.amax, float(al.max()) * io.R)
        ref, bnd = DR.context_from_att_h(att_h, S_h, att_x, True, w["beta"], img, self.absf)
        self.held_b("ctx", cur["rec"][:, self.OFF_CTX:], ref, bnd)
        l, S = DR.mm(cur["recb"][:, :O], w["YWO"])
        b = self.absf * S
        rows = torch.arange(self.nv, device=io.dev)
        idm = ids[:, m]
        l_id, b_id = l[rows, idm], b[rows, idm]
        self.note("chain arg-max", float((((l - b).max(1).values - l_id) / b_id).max()))      # l[id] + b_id >= max_j (l_j - b_j)
        tol = b_id + b.max(1).values + logp_tol(l.cpu().numpy())
        self.note("chain logp", float(((logp[:, m] - (l_id - torch.logsumexp(l, 1))).abs() / tol).max()))
        self.not_flat()
