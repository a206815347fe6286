"""CPU (hipsim): lxo_decoder_train_fwd_live off the persistent chain.  The sim interprets one workgroup after the other, so no chain runs there
(lxo_launch_xdec_fwd answers -2) and the call must BE lxo_decoder_train_fwd: the lengths pointer is ignored, every padded position is computed.
The entry point exists in the sim library (every binding resolves), and the regions the decoder writes are equal byte for byte with lengths,
without (NULL) and through the old call, in both dtypes."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi, synthetic
from latex_ocr_amd.model.utils.image import pad_batch_images
from simharness import Sim, ptr
from simlib import SIM_SO, build_sim

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
V = 11
H, W, T = 32, 48, 6
LENGTHS = np.array([6, 0, 3, 1], np.int32)          # a full row, a dead row, a row of one token
REGIONS = ("logits", "rec", "cs", "gates", "att_h", "alpha")


def _inputs(B=4, seed=5):
    imgs, _ = synthetic.make_set(B, H, W, V, 2, 4, seed=seed)
    f = np.random.default_rng(seed).integers(0, V, size=(B, T)).astype(np.int32)
    return pad_batch_images(imgs), f


def _run(dtype, how):
    img, f = _inputs()
    S = Sim(len(LENGTHS), H, W, T, V, dtype=dtype, seed=0, dims=SMALL)
    S.ck(S.L.lxo_encoder_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(img), None), "enc")
    for name in REGIONS:
        S.region(name, np.float32)[:] = np.float32(7.0)          # what the call does not write would show as equal by accident otherwise
    if how == "old":
        S.ck(S.L.lxo_decoder_train_fwd(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(f), None), "dec")
    else:
        S.ck(S.L.lxo_decoder_train_fwd_live(S.sref(), ptr(S.params), ptr(S.wpack), ptr(S.ws), ptr(f), ptr(LENGTHS) if how == "lengths" else None, None),
             "dec_live")
    return {name: S.region(name, np.float32).copy() for name in REGIONS}


def test_entry_point_is_exported_and_bound():
    build_sim()
    lib = _abi.bind(ctypes.CDLL(SIM_SO))
    assert "lxo_decoder_train_fwd_live" in _abi.ENTRY_POINTS and not lib._lxo_missing, lib._lxo_missing
    assert lib.lxo_decoder_train_fwd_live.argtypes is not None and len(lib.lxo_decoder_train_fwd_live.argtypes) == 7


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_equals_decoder_train_fwd_at_every_position(dtype):
    old = _run(dtype, "old")
    for how in ("lengths", "null"):
        new = _run(dtype, how)
        for name in REGIONS:
            assert old[name].tobytes() == new[name].tobytes(), (how, name)
    n = len(LENGTHS) * T * ((V + 31) // 32 * 32)
    assert np.isfinite(old["logits"][:n]).all() and old["logits"][:n].any()
