"""-m gpu: the decoder's training step stage by stage on the GPU.  lxo_decoder_train_fwd, lxo_ce_loss_fwd_bwd, lxo_decoder_train_bwd_part(1)
and (2); every workspace region and gradient the kernels store is checked against the float64 reference of tests/decoder_steps_ref.py applied
to the operands the kernels themselves stored (tests/decoder_steps_walk.py), element by element: stored sums within 2^-14 S (bf16 mode; a
bf16-stored value 2^-8 |ref| on top) or 2^-20 S (f32 mode), non-linear stages within their first-order bound, bf16 mirrors and the gathered
embedding rows bit for bit.  The launch-per-step kernels (fused and split-K) first, then the persistent chains (csrc/xdec.hip), which
write the same record.  Default widths (C = U = O = 512, E = 256), V = 120.  Each case prints its worst err / bound per check."""
import ctypes

import numpy as np
import pytest
import torch

from latex_ocr_amd import _abi
from latex_ocr_amd.engine import Engine, _p
import encoder_layers_walk as EW
import decoder_steps_walk as DW

pytestmark = pytest.mark.gpu
V = 120


class GpuIO(object):
    """the walk's adapter on an Engine's buffers (see decoder_steps_walk.py)"""

    def __init__(self, B, H, W, T, bf=True, live_B=0, dims=None, keep=0.0, dseed=0, step_kernels=2, deterministic=False, dual=False, seed=0):
        self.e = e = Engine(V, dims=dims, dtype="bf16" if bf else "f32", device="cuda:0", seed=seed, deterministic=deterministic)
        e.step_kernels = step_kernels
        e.ensure(B, H, W, T)
        sh = e.shape
        sh.live_B = live_B
        if 0.0 < keep < 1.0:
            sh.keep_prob, sh.dropout_seed = keep, dseed
        e.load_params(DW.random_decoder_params(EW.random_biases(e.get_params(), seed + 1), seed + 2))
        e._bind_side()
        d = e.dims
        self.bf, self.det, self.B, self.live_B, self.T = bf, bool(deterministic), B, live_B, T
        self.C, self.E, self.U, self.O, self.D, self.V = d["C"], d["E"], d["U"], d["O"], d["D"], V
        cd8 = lambda n: -(-n // 8)
        self.R = (cd8(H) - 2) * (cd8(W) - 2)
        self.Rp = (self.R + 7) // 8 * 8
        self.keep, self.seed, self.step_kernels, self.dual = float(keep), dseed, step_kernels, dual
        self.chain = bf and step_kernels == 0                     # expected; dec_fwd / dec_bwd assert that the chains ran
        self.dev = torch.device("cuda:0")
        self.side = torch.cuda.Stream(self.dev) if dual else None
        self.dimg_bf = e.lib.lxo_ws_region_dtype(e.sref(), b"d_img") == _abi.LXO_BF16
        self.img = torch.from_numpy(np.ascontiguousarray(EW.images("plain", B, H, W, seed)[:live_B or B])).to(self.dev)
        self.params = {k: torch.from_numpy(v) for k, v in e.get_params().items()}

    def set_formula(self, f, l):
        self.f = torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(self.dev)
        self.l = torch.from_numpy(np.ascontiguousarray(l, np.int32)).to(self.dev)

    def _call(self, fn):
        e = self.e
        torch.cuda.synchronize()
        e._ck(e.lib.lxo_set_side_stream(ctypes.c_void_p(self.side.cuda_stream) if self.side is not None else ctypes.c_void_p(0)), "set_side_stream")
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            e._ck(e.lib.lxo_set_side_stream(ctypes.c_void_p(0)), "set_side_stream")

    def enc_fwd(self):
        e = self.e
        self._call(lambda: e._ck(e.lib.lxo_encoder_fwd(e.sref(), _p(e.params), _p(e.wpack), _p(e.ws), _p(self.img), e._stream()), "encoder_fwd"))

    def dec_fwd(self):
        e = self.e
        self._call(lambda: e._ck(e.lib.lxo_decoder_train_fwd(e.sref(), _p(e.params), _p(e.wpack), _p(e.ws), _p(self.f), e._stream()), "decoder_train_fwd"))
        if self.chain:
            used, err = e.chain_status()
            assert used and err == 0, ("forward chain", used, err)

    def loss(self, inv_ntok):
        e = self.e
        self._call(lambda: e._ck(e.lib.lxo_ce_loss_fwd_bwd(e.sref(), _p(e.ws), _p(self.f), _p(self.l), ctypes.c_float(inv_ntok), e._stream()), "ce_loss"))

    def dec_bwd(self, parts):
        e = self.e
        self._call(lambda: e._ck(e.lib.lxo_decoder_train_bwd_part(e.sref(), _p(e.params), _p(e.wpack), _p(e.ws), _p(self.f), _p(e.grads), parts,
                                                                  e._stream()), "decoder_train_bwd_part"))
        if self.chain and parts & 2:
            used, err = e.chain_status(backward=True)
            assert used and err == 0, ("backward chain", used, err)

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

    def fill(self, name, byte):
        self._raw(name).fill_(byte)

    def zero_grads(self):
        self.e.grads.zero_()

    def grad(self, name):
        o, n, s = self.e._offsets[name]
        return self.e.grads[o:o + n].view(*s).to(torch.float64)


def run_case(case, B, H, W, T, seed=3, first_len=None, **kw):
    io = GpuIO(B, H, W, T, seed=seed, **kw)
    walk = DW.Walk(io, case, first_len=first_len)
    walk.forward()
    walk.backward()
    walk.report()
    torch.cuda.synchronize()
    return walk


def test_fused_bf16_dropout_b20():
    """the fused step kernels: B = 20 (two 16-row tiles, the second partial), 40 x 150 (R = 51, Rp = 56), T = 9, dropout (0.85, 99)"""
    w = run_case("fused bf16 B20 40x150 dropout", 20, 40, 150, 9, keep=0.85, dseed=99)
    assert w.fused and w.mirr


def test_fused_f32():
    """the f32 parity mode on the fused step kernels: every sum held to 2^-20 S"""
    run_case("fused f32 B4 40x150", 4, 40, 150, 6, bf=False)


def test_fused_bf16_deterministic():
    """lxo_shape.deterministic: ordered slots in place of the atomics"""
    run_case("fused bf16 deterministic B5", 5, 40, 150, 9, deterministic=True)


def test_split_k_side_stream_dropout():
    """step_kernels = 1 with the side stream bound: the two halves of B = 6 on two streams, row0 offsets in their masks"""
    w = run_case("split-K dual B6 dropout", 6, 40, 150, 9, step_kernels=1, dual=True, keep=0.85, dseed=99)
    assert not w.fused


def test_many_regions_160x800():
    """R = 1764: both attention kernels run more than one chunk per row (at most 1024 rows fit a chunk: the floor of Plan::attn_chunks)"""
    run_case("fused bf16 B2 160x800", 2, 160, 800, 3)


def test_mixed_widths():
    """C = E = 256, U = O = 128: falls to the split-K path by itself; no two operands of a product have the same shape by accident"""
    w = run_case("mixed widths B3", 3, 40, 150, 9, dims=dict(C=256, E=256, U=128, O=128, D=16))
    assert not w.fused


def test_chain_dead_rows_dropout():
    """the persistent chains (step_kernels = 0): B = 8 with live_B = 3, 50 x 120, T = 9, dropout"""
    run_case("chain B8 live3 50x120 dropout", 8, 50, 120, 9, step_kernels=0, live_B=3, keep=0.85, dseed=99)


def test_chain_b16():
    """the persistent chains: B = 16 (two samples per XCD), 64 x 128, T = 7"""
    run_case("chain B16 64x128", 16, 64, 128, 7, step_kernels=0)
