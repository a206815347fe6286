"""-m gpu: the encoder's kernels one layer at a time on the GPU.  lxo_encoder_fwd, then lxo_encoder_bwd(l, l) for l = 6 .. 1; every tensor
the kernels store (pooled activations and their routing masks, the rotating gradient buffers, weight and bias gradients) is checked
against the float64 reference of tests/encoder_layers_ref.py applied to the tensors the kernels themselves stored below it
(tests/encoder_layers_walk.py), element by element: bf16-stored values within 2^-8 |ref| + 2^-14 S, f32 sums within 2^-14 S (S = the sum
of the absolute values of the element's terms), routed gradients bit for bit, exact ties in a pool window taken at their first position.
Each case prints its worst err / bound per check."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from latex_ocr_amd import synthetic
from latex_ocr_amd.engine import Engine, _p
import encoder_layers_walk as EW

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
V = 50


class GpuIO(object):
    """the walk's adapter on an Engine's buffers (see encoder_layers_walk.py)"""

    def __init__(self, B, H, W, img, bf=True, live_B=0, cnn=False, positional=True, deterministic=False, side=True, seed=0):
        dims = dict(cnn=cnn, positional=positional)
        self.e = e = Engine(V, dims=dims, dtype="bf16" if bf else "f32", device="cuda:0", seed=seed, deterministic=deterministic)
        e.ensure(B, H, W, 1)
        e.shape.live_B = live_B
        e.load_params(EW.random_biases(e.get_params(), seed + 1))
        e._bind_side()
        if not side:                       # the encoder without its weight-gradient stream (the engine binds one by default)
            e._ck(e.lib.lxo_set_encoder_side_stream(ctypes.c_void_p(0)), "set_encoder_side_stream")
        self.bf, self.B, self.Be, self.H, self.W, self.C = bf, B, (live_B or B), H, W, e.dims["C"]
        self.cnn, self.positional, self.dev = cnn, positional, torch.device("cuda:0")
        self.e_det = bool(deterministic)
        self.img_dev = torch.from_numpy(np.ascontiguousarray(img[:self.Be])).to(self.dev)
        self.img = self.img_dev[..., 0]
        self.params = {k: torch.from_numpy(v) for k, v in e.get_params().items()}

    def fwd(self):
        e = self.e
        e._ck(e.lib.lxo_encoder_fwd(e.sref(), _p(e.params), _p(e.wpack), _p(e.ws), _p(self.img_dev), e._stream()), "encoder_fwd")

    def bwd(self, l):
        e = self.e
        e._ck(e.lib.lxo_encoder_bwd(e.sref(), _p(e.params), _p(e.wpack), _p(e.ws), _p(self.img_dev), _p(e.grads), l, l, e._stream()),
              "encoder_bwd")

    def _raw(self, name):
        e = self.e
        off, nb = ctypes.c_size_t(), ctypes.c_size_t()
        e._ck(e.lib.lxo_ws_region(e.sref(), name.encode(), ctypes.byref(off), ctypes.byref(nb)), "ws_region")
        return e.ws[off.value:off.value + nb.value]

    def _view(self, name, shape, dt):
        return self._raw(name).view(dt)[:int(np.prod(shape))].view(*shape)

    def values(self, name, shape):
        return self._view(name, shape, torch.bfloat16 if self.bf else torch.float32).to(torch.float64)

    def bits(self, name, shape):
        return self._view(name, shape, torch.int16 if self.bf else torch.int32).clone()

    def bytes(self, name, shape):
        return self._view(name, shape, torch.uint8).clone()

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


def run_case(case, B, H, W, kind="plain", live_B=0, seed=3, nan_dead=False, **kw):
    img = EW.images(kind, B, H, W, seed)
    io = GpuIO(B, H, W, img, live_B=live_B, seed=seed, **kw)
    walk = EW.Walk(io, case)
    walk.forward()
    grads = walk.backward(seed=seed + 7)
    if nan_dead:
        walk.dead_rows_not_read(grads, seed=seed + 7)
    walk.report()
    torch.cuda.synchronize()
    return walk


def test_128x512_b16():
    """128-channel tiles (NJ = 4) in every layer with Cout >= 128; all three fused pools on NJ = 4; conv6's short tile (14 output rows in
    two 8-row tiles); EPI 1 (conv6: timing signal + out_pre) and EPI 2 (conv4's data gradient) on 128-channel tiles; conv_wgrad with nsplit > 1"""
    run_case("128x512 B16", 16, 128, 512)


def test_reference_training_batch_dead_rows():
    """the reference's training batch: 50 x 120 filled up to B = 8 with live_B = 3 -- 64-channel tiles, odd extents at every pool level
    (H 25 -> 13 -> 7, W 60 -> 30 -> 15), dead rows (zero features; NaN in their d_img rows changes nothing)"""
    run_case("50x120 B8 live3", 8, 50, 120, live_B=3, nan_dead=True)


def test_clipped_windows_37x141():
    """37 x 141: clipped pool windows in both directions and partial tiles everywhere"""
    run_case("37x141 B3", 3, 37, 141)


def test_tie_batch():
    """mixed page sizes padded white + one constant grey page: exact float64 ties through every pool level, the first position must win"""
    w = run_case("ties 64x256 B4", 4, 64, 256, kind="ties")
    assert sum(t for _, t in w.ties.values()) > 10000, w.ties


@pytest.mark.parametrize("B,H,W", [(16, 128, 512), (3, 37, 141)])
def test_deterministic(B, H, W):
    """lxo_shape.deterministic: the ordered slots (colsum_part, the weight-gradient slabs and their ordered pass, the mask kernels' and conv1's
    partials) in place of the atomics"""
    run_case("deterministic %dx%d B%d" % (H, W, B), B, H, W, deterministic=True)


def test_without_the_encoder_side_stream():
    """lxo_set_encoder_side_stream(NULL): every weight gradient on the compute stream"""
    run_case("no side stream 50x120 B3", 3, 50, 120, side=False)


def test_cnn_variant_no_positional():
    """encoder_cnn = "cnn", positional embeddings off: y4 / y5 stored, im2col_s2 (bit-exact), the strided GEMM, col2im_s2_relu"""
    run_case("cnn 64x256 B4", 4, 64, 256, cnn=True, positional=False)


@pytest.mark.parametrize("H,W", [hw for hw in synthetic.REAL_BUCKETS if hw != (800, 800)])
def test_real_buckets(H, W):
    """the reference's real bucket sizes at its training batch of 3 (800 x 800 stays with test_gpu_fullsize.py)"""
    run_case("bucket %dx%d B3" % (H, W), 3, H, W)


def test_f32_parity_mode():
    """f32: the unfused maxpool_fwd / maxpool_relu_bwd kernels, the VALU conv1 kernels, mask_convert and the ordered sums, every output held to
    2^-20 S -- a check of the harness itself; dead rows with NaN in d_img"""
    run_case("f32 50x120 B4 live3", 4, 50, 120, bf=False, live_B=3, nan_dead=True)


def test_128_channel_tiles_at_a_small_shape():
    """LXO_CONV_SMALL=0 (read once per process, so in a child): every launch on 128-channel tiles at the reference's batch shape"""
    env = dict(os.environ, LXO_CONV_SMALL="0")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_encoder_layers as T; T.run_case('NJ=4 ties 50x120 B3', 3, 50, 120, kind='ties')" % (
        HERE, os.path.dirname(HERE))
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    print(out[-3000:])
    assert r.returncode == 0, out[-3000:]
