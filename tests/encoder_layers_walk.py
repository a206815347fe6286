"""TEST INFRASTRUCTURE: runs the encoder one layer at a time through an adapter (the hipsim `Sim` or the GPU `Engine`) and checks every
tensor it stores against tests/encoder_layers_ref.py applied to the tensors the kernels themselves stored below it.

The adapter `io` offers: bf (bool), e_det (lxo_shape.deterministic), B, Be (live images), H, W, C, cnn, positional, dev (torch device of the reference), img (u8 [Be, H, W]),
params (name -> f32 torch tensor), fwd(), bwd(layer), values(region, shape) (float64 of the compute-dtype / f32 contents),
bits(region, shape) (the raw 16- / 32-bit patterns), bytes(region, shape) (u8), write(region, tensor), fill(region, byte) (every byte of
the region), zero_grads(), grad(name) (float64).

Every region the walk reads is filled with 0xFF bytes (NaN, mask byte 0xFF) before the call that has to write it: an element a kernel
leaves unwritten -- a dead row not zeroed, a partial tile not stored -- fails its check instead of passing on a zero-initialised workspace."""
import numpy as np
import torch

from latex_ocr_amd import synthetic
from latex_ocr_amd.model.utils.image import pad_batch_images

import encoder_layers_ref as ER

# which ws region g0 / g1 / g2 holds what during the encoder backward pass (csrc/model_encoder.hip: XV / YV, XC / YC): X[l] = d_y of layer l,
# Y[l] = the gradient of layer l's input
XV, YV = (0, 0, 0, 1, 0, 2, 0), (0, 0, 2, 2, 1, 1, 1)
XC, YC = (0, 0, 1, 0, 1, 2, 0), (0, 0, 2, 2, 0, 1, 1)
PRE = "Encoder/convolutional_encoder/conv2d"


POISON = 0xFF


def random_biases(P, seed):
    """conv biases start at zero (tf.layers.conv2d): random ones of both signs, so that a bias added twice, at the wrong place or not at
    all shows, and the ReLUs cut at varying heights"""
    rng = np.random.default_rng(seed)
    P = dict(P)
    for k in P:
        if k.startswith(PRE) and k.endswith("/bias"):
            P[k] = (0.05 * rng.standard_normal(P[k].shape)).astype(np.float32)
    return P


def images(kind, B, H, W, seed):
    """u8 [B, H, W, 1]: `plain` = synthetic pages (white, 8 % ink); `ties` = pages of mixed sizes padded white to the batch maximum plus one
    constant grey page (exact ties through every pool level, with the ReLU positive over wide areas)."""
    if kind == "plain":
        imgs, _ = synthetic.make_set(B, H, W, 50, 5, 9, seed=seed)
    else:
        imgs = []
        for i in range(B - 1):
            h, w = max(17, H - (H // 5) * i), max(17, W - (W // 4) * i)
            imgs += synthetic.make_set(1, h, w, 50, 5, 9, seed=seed + i)[0]
        imgs.append(np.full((H, W, 1), 77, np.uint8))
    return np.ascontiguousarray(pad_batch_images(imgs, (H, W, 1)))


def pname(i):
    return PRE + ("" if i == 0 else "_%d" % i)


def geometry(io):
    cd2 = lambda n: (n + 1) // 2
    g = dict(H1=cd2(io.H), W1=cd2(io.W))
    g["H2"], g["W2"] = cd2(g["H1"]), cd2(g["W1"])
    g["H4"] = g["H2"] if io.cnn else cd2(g["H2"])
    g["W5"] = cd2(g["W2"])
    g["H6"] = cd2(g["H2"]) if io.cnn else g["H4"]
    g["Hp"], g["Wp"] = g["H6"] - 2, g["W5"] - 2
    return g


class Walk(object):
    """One case: forward() checks the stored activations, backward() the per-layer gradients; `worst` collects err / bound per check."""

    def __init__(self, io, case):
        self.io, self.case = io, case
        self.g = geometry(io)
        if io.bf:
            self.rel, self.absf = ER.REL_BF16, ER.ABS_BF16
        else:
            self.rel, self.absf = 0.0, ER.ABS_F32
        self.worst = {}
        self.ties = {}
        self.st = {}

    # ---------------------------------------------------------------------------------------------------------------- helpers --
    def w(self, i):
        w = self.io.params[pname(i) + "/kernel"].to(self.io.dev, torch.float64)
        return ER.bf16_round(w) if self.io.bf else w

    def b(self, i):
        return self.io.params[pname(i) + "/bias"].to(self.io.dev, torch.float64)

    def last(self):
        return 6 if self.io.cnn else 5

    def held(self, what, got, ref, S, rel=None, extra=None):
        rel = self.rel if rel is None else rel
        r = ER.ratio(got, ref, ER.bound(ref, S, rel, self.absf, extra))
        self.worst[what] = max(self.worst.get(what, 0.0), r)
        assert r <= 1.0, "%s / %s: err / bound = %.3g" % (self.case, what, r)

    def held_b(self, what, got, ref, bnd):
        r = ER.ratio(got, ref, bnd)
        self.worst[what] = max(self.worst.get(what, 0.0), r)
        assert r <= 1.0, "%s / %s: err / bound = %.3g" % (self.case, what, r)

    def f32_held(self, what, got, ref, S):
        """f32 results (weight and bias gradients): 2^-14 S in bf16 mode, 2^-20 S in the f32 parity mode."""
        self.held(what, got, ref, S, rel=0.0)

    def act(self, name, shape):
        return self.io.values(name, (self.io.Be,) + tuple(shape))

    def pool_check(self, what, pre, S, ph, pw, pooled, mask_name):
        """a fused conv + pool (bf16): pooled values and mask bytes; the f32 parity mode stores the full-resolution activation first."""
        io = self.io
        pr = ER.pool_ref(pre, S, ph, pw, self.rel, self.absf)
        if io.bf:
            p = self.act(pooled, pr["value"].shape[1:])
            self.held_b(what + " pooled", p, pr["value"], pr["bound"])
            m = io.bytes(mask_name, (io.Be,) + tuple(pr["value"].shape[1:]))
            near, ties = ER.check_mask(m, pr, "%s / %s mask" % (self.case, what))
            self.ties[what] = (near, ties)
            self.st[mask_name] = m
        else:
            y = self.act(mask_name, pre.shape[1:])                          # (f32: the un-pooled activation region)
            self.held(what, y, torch.relu(pre), S)
            v, _ = ER.windows(y, ph, pw, -float("inf"))
            p = self.act(pooled, pr["value"].shape[1:])
            assert torch.equal(p, v.max(-1)[0]), "%s / %s: pool of the stored activation" % (self.case, what)
            self.st[mask_name] = y
        return p

    # ---------------------------------------------------------------------------------------------------------------- forward --
    def forward(self):
        io, g = self.io, self.g
        reads = ["p1", "p2", "y3", "p5", "y6", "img"]
        if io.cnn:
            reads += ["y4", "y5", "cols"]
        elif io.bf:
            reads += ["m2", "p4", "m4", "m5"]
        else:
            reads += ["y2", "p4", "y4", "y5"]
        for r in reads:
            io.fill(r, POISON)
        io.fwd()
        pre, S = ER.conv1_pre(io.img, io.params[pname(0) + "/kernel"].to(io.dev), self.b(0), io.bf)
        pr = ER.pool_ref(pre, S, 2, 2, self.rel, self.absf)
        p1 = self.act("p1", (g["H1"], g["W1"], 64))
        self.held_b("L1 p1", p1, pr["value"], pr["bound"])
        pre, S = ER.conv3x3(p1, self.w(1), self.b(1), 1)
        p2 = self.pool_check("L2 p2", pre, S, 2, 2, "p2", "m2" if io.bf else "y2")
        pre, S = ER.conv3x3(p2, self.w(2), self.b(2), 1)
        y3 = self.act("y3", (g["H2"], g["W2"], 256))
        self.held("L3 y3", y3, torch.relu(pre), S)
        pre, S = ER.conv3x3(y3, self.w(3), self.b(3), 1)
        if not io.cnn:
            p4 = self.pool_check("L4 p4", pre, S, 2, 1, "p4", "m4" if io.bf else "y4")
            pre, S = ER.conv3x3(p4, self.w(4), self.b(4), 1)
            p5 = self.pool_check("L5 p5", pre, S, 1, 2, "p5", "m5" if io.bf else "y5")
        else:
            y4 = self.act("y4", (g["H2"], g["W2"], 256))
            self.held("L4 y4", y4, torch.relu(pre), S)
            pre, S = ER.conv3x3(y4, self.w(4), self.b(4), 1)
            y5 = self.act("y5", (g["H4"], g["W2"], io.C))
            self.held("L5 y5", y5, torch.relu(pre), S)
            cols = io.bits("cols", (io.Be, g["H6"], g["W5"], 8 * io.C))
            want = ER.im2col_s2(io.bits("y5", (io.Be, g["H4"], g["W2"], io.C)))
            assert torch.equal(cols, want), "%s: cols is not the bit-exact im2col of y5" % self.case
            colv = self.act("cols", (g["H6"], g["W5"], 8 * io.C))
            ref, S = ER.strided_conv(colv, self.w(5), self.b(5))
            p5 = self.act("p5", (g["H6"], g["W5"], io.C))
            self.held("L5s p5", p5, ref, S)
            self.st.update(y4=y4, y5=y5, cols=colv)
        pos = None
        if io.positional:
            from oracle.ref_model import timing_signal_2d
            pos = timing_signal_2d(g["Hp"], g["Wp"], io.C, dtype=torch.float64).to(io.dev)
        pre, S = ER.conv3x3(p5, self.w(self.last()), self.b(self.last()), 0)
        y6 = self.act("y6", (g["Hp"], g["Wp"], io.C))
        self.held("L6 y6", y6, torch.relu(pre), S)
        img = self.act("img", (g["Hp"], g["Wp"], io.C))
        ref = torch.relu(pre) + (pos[None] if pos is not None else 0.0)
        self.held("L6 img", img, ref, S + (pos.abs()[None] if pos is not None else 0.0))
        if io.Be < io.B:                     # dead padding rows: exact zeros
            for r in ("img", "y6"):
                raw = io.bits(r, (io.B, g["Hp"], g["Wp"], io.C))[io.Be:]
                assert int((raw != 0).sum()) == 0, "%s: dead rows of %s are not zeros" % (self.case, r)
        self.st.update(p1=p1, p2=p2, y3=y3, p5=p5, y6=y6)
        if not io.cnn:
            self.st["p4"] = p4

    # --------------------------------------------------------------------------------------------------------------- backward --
    def dimg(self, seed, dead_nan=False):
        """the gradient the decoder would hand over: bf16 mode d_y6 = random bf16 masked by y6 > 0 (include/lxo.h: the decoder applies
        conv6's mask), f32 mode the plain f32 gradient.  Dead rows: zeros or NaN.  Written into ws region d_img."""
        io, g = self.io, self.g
        gen = torch.Generator().manual_seed(seed)
        shape = (io.B, g["Hp"], g["Wp"], io.C)
        d = torch.randn(shape, generator=gen, dtype=torch.float64).to(io.dev)
        d[io.Be:] = float("nan") if dead_nan else 0.0
        if io.bf:
            y6 = torch.zeros(shape, dtype=torch.float64, device=io.dev)
            y6[:io.Be] = self.st["y6"]
            d = torch.where((y6 > 0) | torch.isnan(d), d, torch.zeros_like(d))
            d = ER.bf16_round(d)
        else:
            d = d.to(torch.float32).to(torch.float64)
        io.write("d_img", d.to(torch.bfloat16 if io.bf else torch.float32))
        return d[:io.Be]

    def gbuf(self, i, shape, kind="values"):
        return getattr(self.io, kind)("g%d" % i, (self.io.Be,) + tuple(shape))

    def grad_w(self, i):
        return self.io.grad(pname(i) + "/kernel")

    def grad_b(self, i):
        return self.io.grad(pname(i) + "/bias")

    def routed(self, what, i, dp_bits, mask, ph, pw, H, W, Cc):
        """d_y written by the pool backward: bit for bit the routed d_p (bf16 mask kernels) / routed by the stored activation (f32)."""
        io = self.io
        if io.bf:
            got = self.gbuf(i, (H, W, Cc), "bits")
            want = ER.route(dp_bits, mask, ph, pw, H, W)
            bad = got != want
            assert int(bad.sum()) == 0, "%s / %s: %d routed elements differ, first at %s" % (self.case, what, int(bad.sum()), bad.nonzero()[0].tolist())
            self.worst[what] = 0.0
        else:
            got = self.gbuf(i, (H, W, Cc))
            dp = dp_bits.view(torch.float32).to(torch.float64)
            want = ER.route_by_first_max(dp, mask, ph, pw)
            assert torch.equal(got, want), "%s / %s: routed gradient" % (self.case, what)
            self.worst[what] = 0.0
        return self.gbuf(i, (H, W, Cc))

    def backward(self, seed=5, dead_nan=False):
        io, g, st = self.io, self.g, self.st
        XB, YB = (XC, YC) if io.cnn else (XV, YV)
        C = io.C
        dy6 = self.dimg(seed, dead_nan)
        for i in range(3):
            io.fill("g%d" % i, POISON)
        io.zero_grads()
        L = self.last()
        # ---- layer 6
        io.bwd(6)
        if not io.bf:                      # f32: the mask of y6 and conv6's bias gradient are the encoder's (mask_convert + ordered sums)
            x6 = self.gbuf(XB[6], (g["Hp"], g["Wp"], C))
            assert torch.equal(x6, ER.relu_mask(dy6, st["y6"])), "%s: d_y6 = d_img * (y6 > 0)" % self.case
            dy6 = x6
            ref, S = ER.colsum(dy6)
            self.f32_held("L6 db", self.grad_b(L), ref, S)
        ref, S = ER.conv3x3_wgrad(st["p5"], dy6, 0)
        self.f32_held("L6 dW", self.grad_w(L), ref, S)
        dp5 = self.gbuf(YB[6], (g["H6"], g["W5"], C))
        dp5_bits = self.gbuf(YB[6], (g["H6"], g["W5"], C), "bits")
        ref, S = ER.conv3x3_dgrad(dy6, self.w(L), 0)
        self.held("L6 d_p5", dp5, ref, S)
        # ---- layer 5
        io.bwd(5)
        if not io.cnn:
            dy5 = self.routed("L5 d_y5", XB[5], dp5_bits, st["m5" if io.bf else "y5"], 1, 2, g["H4"], g["W2"], C)
        else:
            (db, Sdb), (dw, Sdw), (dc, Sdc) = ER.strided_conv_bwd(st["cols"], dp5, self.w(5))
            self.f32_held("L5s db", self.grad_b(5), db, Sdb)
            self.f32_held("L5s dW", self.grad_w(5), dw, Sdw)
            dcols = self.act("cols", (g["H6"], g["W5"], 8 * C))
            self.held("L5s d_cols", dcols, dc, Sdc)
            ref, S = ER.col2im_s2_relu(dcols, st["y5"])
            dy5 = self.gbuf(XB[5], (g["H4"], g["W2"], C))
            self.held("L5s d_y5", dy5, ref, S)
            # col2im_s2_relu sums conv5's bias gradient from its f32 values before they are rounded to bf16; the ordered pass of the
            # deterministic and f32 modes sums the stored tensor
            db5_in = ref if (io.bf and not io.e_det) else dy5
        ref, S = ER.colsum(db5_in if io.cnn else dy5)
        self.f32_held("L5 db", self.grad_b(4), ref, S)
        ref, S = ER.conv3x3_wgrad(st["y4"] if io.cnn else st["p4"], dy5, 1)
        self.f32_held("L5 dW", self.grad_w(4), ref, S)
        ref, S = ER.conv3x3_dgrad(dy5, self.w(4), 1)
        if io.cnn:                          # d_y4 = dgrad5 * (y4 > 0) (+ db4): the EPI 2 epilogue
            dy4 = self.gbuf(YB[5], (g["H2"], g["W2"], 256))
            self.held("L5 d_y4", dy4, ER.relu_mask(ref, st["y4"]), ER.relu_mask(S, st["y4"]))
        else:
            dp4 = self.gbuf(YB[5], (g["H4"], g["W2"], 256))
            dp4_bits = self.gbuf(YB[5], (g["H4"], g["W2"], 256), "bits")
            self.held("L5 d_p4", dp4, ref, S)
        # ---- layer 4
        io.bwd(4)
        if not io.cnn:
            dy4 = self.routed("L4 d_y4", XB[4], dp4_bits, st["m4" if io.bf else "y4"], 2, 1, g["H2"], g["W2"], 256)
        ref, S = ER.colsum(dy4)
        self.f32_held("L4 db", self.grad_b(3), ref, S)
        ref, S = ER.conv3x3_wgrad(st["y3"], dy4, 1)
        self.f32_held("L4 dW", self.grad_w(3), ref, S)
        ref, S = ER.conv3x3_dgrad(dy4, self.w(3), 1)
        dy3 = self.gbuf(YB[4], (g["H2"], g["W2"], 256))
        self.held("L4 d_y3", dy3, ER.relu_mask(ref, st["y3"]), ER.relu_mask(S, st["y3"]))
        ref, S = ER.colsum(dy3)
        self.f32_held("L3 db", self.grad_b(2), ref, S)
        # ---- layer 3
        io.bwd(3)
        ref, S = ER.conv3x3_wgrad(st["p2"], dy3, 1)
        self.f32_held("L3 dW", self.grad_w(2), ref, S)
        ref, S = ER.conv3x3_dgrad(dy3, self.w(2), 1)
        dp2 = self.gbuf(YB[3], (g["H2"], g["W2"], 128))
        dp2_bits = self.gbuf(YB[3], (g["H2"], g["W2"], 128), "bits")
        self.held("L3 d_p2", dp2, ref, S)
        # ---- layer 2
        io.bwd(2)
        dy2 = self.routed("L2 d_y2", XB[2], dp2_bits, st["m2" if io.bf else "y2"], 2, 2, g["H1"], g["W1"], 128)
        ref, S = ER.colsum(dy2)
        self.f32_held("L2 db", self.grad_b(1), ref, S)
        ref, S = ER.conv3x3_wgrad(st["p1"], dy2, 1)
        self.f32_held("L2 dW", self.grad_w(1), ref, S)
        ref, S = ER.conv3x3_dgrad(dy2, self.w(1), 1)
        dp1 = self.gbuf(YB[2], (g["H1"], g["W1"], 64))
        self.held("L2 d_p1", dp1, ref, S)
        # ---- layer 1
        io.bwd(1)
        (dw, Sw, aw), (db, Sb, ab) = ER.conv1_pool_bwd(io.img, io.params[pname(0) + "/kernel"].to(io.dev), self.b(0), dp1, io.bf, self.absf)
        self.held("L1 dW", self.grad_w(0), dw, Sw, rel=0.0, extra=aw)
        self.held("L1 db", self.grad_b(0), db, Sb, rel=0.0, extra=ab)
        return {k: io.grad(k).clone() for k in io.params if k.startswith("Encoder/")}

    def dead_rows_not_read(self, grads, seed=5):
        """NaN in the dead rows of d_img (live_B < B): those rows are not read -- every gradient finite and equal to the run with zeros
        there (`grads`, from backward(seed)): bit for bit where the sums are ordered, within rounding where atomics add in any order."""
        got = self.backward(seed=seed, dead_nan=True)
        ordered = not self.io.bf or self.io.e_det
        for k in grads:
            assert torch.isfinite(got[k]).all(), (self.case, k)
            if ordered:
                assert torch.equal(got[k], grads[k]), (self.case, k)
            else:
                assert (got[k] - grads[k]).abs().max() <= 1e-5 * grads[k].abs().max(), (self.case, k)

    def report(self):
        print("%s: worst err / bound: %s" % (self.case, ", ".join("%s %.3f" % (k, v) for k, v in self.worst.items())))
        if self.ties:
            print("%s: pool windows (near ties, exact ties of 2+): %s" % (self.case, ", ".join("%s %d/%d" % (k, a, b) for k, (a, b) in self.ties.items())))
