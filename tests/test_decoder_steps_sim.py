"""CPU: the decoder's training step stage by stage under the hipsim SIMT interpreter -- the launch-per-step kernels (csrc/rstep.hip,
decoder_kernels.hip, dimg.hip and the GEMM calls of model_decoder.hip), every workspace region and gradient they store against the float64
reference of tests/decoder_steps_ref.py applied to the operands the kernels stored (tests/decoder_steps_walk.py) -- the mirror of
tests/test_gpu_decoder_steps.py at small widths: C = E = U = O = 128, D = 16, V = 11, a 25 x 57 image (R = 12, Rp = 16), T = 5."""
import ctypes

import numpy as np
import torch

from simharness import Sim, lib, ptr
from simlib import bf16_to_f32
import encoder_layers_walk as EW
import decoder_steps_walk as DW

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V = 11


class SimIO(object):
    """the walk's adapter on the interpreter (see decoder_steps_walk.py)"""

    def __init__(self, B, H, W, T, bf=True, live_B=0, dims=None, keep=0.0, dseed=0, step_kernels=2, deterministic=0, dual=False, seed=0):
        self.S = S = Sim(B, H, W, T, V, dtype=1 if bf else 0, dims=dict(dims or SMALL), seed=seed)
        sh = S.shape
        sh.live_B, sh.deterministic, sh.step_kernels = live_B, deterministic, step_kernels
        if 0.0 < keep < 1.0:
            sh.keep_prob, sh.dropout_seed = keep, dseed
        S.ws = np.zeros(S.L.lxo_workspace_bytes(ctypes.byref(sh)) + 256, np.uint8)
        S.P = DW.random_decoder_params(EW.random_biases(S.P, seed + 1), seed + 2)
        S.set_params(S.P)
        d = S.dims
        self.bf, self.det, self.B, self.live_B, self.T = bf, bool(deterministic), B, live_B, T
        self.C, self.E, self.U, self.O, self.D, self.V = d["C"], d["E"], d["U"], d["O"], d["D"], V
        cd8 = lambda n: -(-n // 8)
        self.R = (cd8(H) - 2) * (cd8(W) - 2)
        self.Rp = (self.R + 7) // 8 * 8
        self.keep, self.seed, self.step_kernels, self.dual, self.chain = float(keep), dseed, step_kernels, dual, False
        self.dev = torch.device("cpu")
        self.dimg_bf = S.L.lxo_ws_region_dtype(S.sref(), b"d_img") == 1
        self.img = np.ascontiguousarray(EW.images("plain", B, H, W, seed)[:live_B or B])
        self.params = {k: torch.from_numpy(np.asarray(v, np.float32).copy()) for k, v in S.P.items()}

    def set_formula(self, f, l):
        self.f, self.l = np.ascontiguousarray(f, np.int32), np.ascontiguousarray(l, np.int32)

    def _call(self, fn):
        lib().lxo_set_side_stream(ctypes.c_void_p(1 if self.dual else 0))        # (streams are no-ops under hipsim: the half-batch code path)
        try:
            fn()
        finally:
            lib().lxo_set_side_stream(ctypes.c_void_p(0))

    def enc_fwd(self):
        S = self.S
        S.ck(S.L.lxo_encoder_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(self.img), None), "enc")

    def dec_fwd(self):
        S = self.S
        self._call(lambda: S.ck(S.L.lxo_decoder_train_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(self.f), None), "dec"))

    def loss(self, inv_ntok):
        S = self.S
        S.ck(S.L.lxo_ce_loss_fwd_bwd(S.sref(), ptr(S.ws), ptr(self.f), ptr(self.l), ctypes.c_float(inv_ntok), None), "loss")

    def dec_bwd(self, parts):
        S = self.S
        self._call(lambda: S.ck(S.L.lxo_decoder_train_bwd_part(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(self.f), ptr(S.grads), parts, None),
                                "decbwd"))

    def _raw(self, name, shape, kind):
        bf = kind == "bf16" or (kind == "ct" and self.bf)
        a = self.S.region(name, np.uint16 if bf else np.float32)
        return a[:int(np.prod(shape))].reshape(shape), bf

    def values(self, name, shape, kind="f32"):
        a, bf = self._raw(name, shape, kind)
        return torch.from_numpy(bf16_to_f32(a.copy()) if bf else a.copy()).to(torch.float64)

    def bits(self, name, shape, kind="f32"):
        a, bf = self._raw(name, shape, kind)
        return torch.from_numpy(a.copy().view(np.int16 if bf else np.int32))

    def write(self, name, t):
        a = t.contiguous().view(torch.int16).numpy() if t.dtype == torch.bfloat16 else t.contiguous().numpy()
        self.S.write_region(name, a)

    def fill(self, name, byte):
        off, nb = ctypes.c_size_t(), ctypes.c_size_t()
        self.S.ck(self.S.L.lxo_ws_region(self.S.sref(), name.encode(), ctypes.byref(off), ctypes.byref(nb)), "region")
        self.S.ws[off.value:off.value + nb.value] = byte

    def zero_grads(self):
        self.S.grads[:] = 0

    def grad(self, name):
        return torch.from_numpy(self.S.grad(name).copy()).to(torch.float64)


def run_case(case, B, T=5, H=25, W=57, seed=3, first_len=None, **kw):
    io = SimIO(B, H, W, T, seed=seed, **kw)
    walk = DW.Walk(io, case, first_len=first_len)
    walk.forward()
    walk.backward()
    walk.report()
    return walk


def test_bf16_fused_dead_row():
    """the fused step kernels (rstep.hip) in bf16: B = 3 with live_B = 2 (a dead row of length 0 behind the live ones)"""
    w = run_case("sim bf16 fused live 2/3", 3, live_B=2)
    assert w.fused and w.mirr


def test_bf16_fused_dropout():
    """the same with dropout (keep 0.8): both mask streams, forward and backward, and the tanh recovered from the dropped o.  Lengths T and 1
    (the case above has T - 1 and 1): the full row is the one whose carries leave step T - 1"""
    run_case("sim bf16 fused dropout", 3, live_B=2, keep=0.8, dseed=77, first_len=5)


def test_f32_fused():
    """the f32 parity mode on the fused step kernels: every sum held to 2^-20 S"""
    run_case("sim f32 fused", 2, bf=False)


def test_bf16_split_k_two_halves_dropout():
    """step_kernels = 1 (round 1's split-K slab kernels) with a side stream bound: the two halves of B = 4 carry row0 offsets in their masks"""
    w = run_case("sim bf16 split-K dual dropout", 4, step_kernels=1, dual=True, keep=0.8, dseed=5)
    assert not w.fused


def test_bf16_mixed_widths():
    """C = E = 256, U = O = 128: K = U + C = 384 is no power-of-two chunk count, so the shape falls to the split-K path by itself; with
    C != U != ... a transposed operand cannot pass"""
    w = run_case("sim bf16 mixed widths", 2, dims=dict(C=256, E=256, U=128, O=128, D=16))
    assert not w.fused


def test_bf16_deterministic():
    """lxo_shape.deterministic: the ordered slots in place of the atomics (one attention-backward chunk per sample, the ordered column sums)"""
    run_case("sim bf16 deterministic", 2, deterministic=1, first_len=5)
