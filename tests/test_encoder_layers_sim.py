"""CPU: the encoder's kernels one layer at a time under the hipsim SIMT interpreter, each stored tensor against the float64 reference of
tests/encoder_layers_ref.py applied to the tensors the kernels stored below it (tests/encoder_layers_walk.py) -- the mirror of
tests/test_gpu_encoder_layers.py at small widths (C = 128: the pools stay fused into the conv epilogue)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from simharness import Sim, ptr
from simlib import bf16_to_f32
import encoder_layers_walk as EW

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
HERE = os.path.dirname(os.path.abspath(__file__))


class SimIO(object):
    """the walk's adapter on the interpreter (see encoder_layers_walk.py)"""

    def __init__(self, B, H, W, img, bf=True, live_B=0, cnn=False, positional=True, deterministic=0, seed=0):
        dims = dict(SMALL, cnn=cnn, positional=positional)
        self.S = S = Sim(B, H, W, 3, 11, dtype=1 if bf else 0, dims=dims, seed=seed)
        S.shape.live_B = live_B
        S.shape.deterministic = deterministic
        S.ws = np.zeros(S.L.lxo_workspace_bytes(ctypes.byref(S.shape)) + 256, np.uint8)
        S.P = EW.random_biases(S.P, seed + 1)
        S.set_params(S.P)
        self.bf, self.B, self.Be, self.H, self.W, self.C = bf, B, (live_B or B), H, W, SMALL["C"]
        self.cnn, self.positional, self.dev = cnn, positional, torch.device("cpu")
        self.e_det = bool(deterministic)
        self.img_np = np.ascontiguousarray(img[:self.Be])
        self.img = torch.from_numpy(self.img_np[..., 0].copy())
        self.params = {k: torch.from_numpy(np.asarray(v, np.float32).copy()) for k, v in S.P.items()}

    def fwd(self):
        S = self.S
        S.ck(S.L.lxo_encoder_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(self.img_np), None), "enc")

    def bwd(self, l):
        S = self.S
        S.ck(S.L.lxo_encoder_bwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(self.img_np), ptr(S.grads), l, l, None), "encbwd")

    def _raw(self, name, shape, dt):
        a = self.S.region(name, dt)
        return a[:int(np.prod(shape))].reshape(shape)

    def values(self, name, shape):
        if self.bf:
            return torch.from_numpy(bf16_to_f32(self._raw(name, shape, np.uint16).copy())).to(torch.float64)
        return torch.from_numpy(self._raw(name, shape, np.float32).copy()).to(torch.float64)

    def bits(self, name, shape):
        return torch.from_numpy(self._raw(name, shape, np.int16 if self.bf else np.int32).copy())

    def bytes(self, name, shape):
        return torch.from_numpy(self._raw(name, shape, np.uint8).copy())

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


def run_case(case, B, H, W, kind="plain", live_B=0, seed=3, nan_dead=False, **kw):
    img = EW.images(kind, B, H, W, seed)
    io = SimIO(B, H, W, img, live_B=live_B, seed=seed, **kw)
    walk = EW.Walk(io, case)
    walk.forward()
    grads = walk.backward(seed=seed + 7)
    if nan_dead:
        walk.dead_rows_not_read(grads, seed=seed + 7)
    walk.report()
    return walk


def test_odd_extents_dead_rows_bf16():
    """25 x 57: odd extents at every pool level (H 25 -> 13 -> 7 -> 4, W 57 -> 29 -> 15 -> 8), so clipped windows in both directions and
    partial tiles everywhere; B = 3 with live_B = 2 (the dead row's features must be exact zeros, its d_img rows are not read: NaN there
    changes no gradient)."""
    run_case("sim odd 25x57 live 2/3", 3, 25, 57, live_B=2, nan_dead=True)


def test_tie_batch_bf16():
    """white padding of mixed page sizes and a constant grey page: exact float64 ties in every pool window over those areas -- the first
    position must take them, in the fused pools' masks and in conv1's recomputed routing"""
    w = run_case("sim ties 24x64", 3, 24, 64, kind="ties")
    assert sum(t for _, t in w.ties.values()) > 1000, w.ties          # the batch does what it is for


def test_deterministic_bf16():
    """lxo_shape.deterministic: the ordered slots (colsum_part of the data gradients' bias sums, the weight-gradient slabs and their
    ordered pass, the mask kernels' and conv1's partials) in place of the atomics"""
    run_case("sim deterministic 25x57", 2, 25, 57, deterministic=1)


def test_cnn_variant_bf16():
    """encoder_cnn = "cnn" without positional embeddings: y4 / y5 stored, im2col_s2 (bit-exact), the strided GEMM, col2im_s2_relu"""
    run_case("sim cnn 21x45", 2, 21, 45, cnn=True, positional=False)


def test_f32_parity_mode():
    """f32: the unfused maxpool_fwd / maxpool_relu_bwd kernels, the VALU conv1 kernels and mask_convert, every output held to 2^-20 S"""
    run_case("sim f32 21x45", 2, 21, 45, bf=False)


def test_128_channel_tiles_in_a_child_process():
    """LXO_CONV_SMALL=0 (read once per process): every launch on 128-channel tiles, so the NJ = 4 instantiations of the conv kernel
    (EPI 0 / 2 and the three fused pools) are interpreted too"""
    env = dict(os.environ, LXO_CONV_SMALL="0")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_encoder_layers_sim as T; T.run_case('sim NJ=4 ties 21x45', 2, 21, 45, kind='ties')" % (
        HERE, os.path.dirname(HERE))
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    out = r.stdout.decode()
    print(out[-3000:])
    assert r.returncode == 0, out[-3000:]
