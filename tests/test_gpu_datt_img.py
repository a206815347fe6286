"""-m gpu: the deferred d_att_img pass (csrc/decoder_kernels.hip: atth_exp_kernel + datt_img_live_kernel; bf16, E <= 256) at the shapes where its
loop bounds and its LDS staging can go wrong.  A workgroup stages its 16 columns of d_e for all steps in LDS, every wave takes n = 1 + the last
step at which one of its 4 regions has a non-zero d and walks t < n in groups of 4 and a remainder.  Each case is a full walk of
tests/decoder_steps_walk.py (run_case of tests/test_gpu_decoder_steps.py), which holds d_att_img and d_beta -- and everything that reads them
-- to their float64 bounds, with columns R..Rp of d_e poisoned.  Default widths (C = U = O = 512, E = 256) unless a case says otherwise."""
import ctypes

import pytest

import test_gpu_decoder_steps as G

pytestmark = pytest.mark.gpu


def table_bytes(walk):
    """size of ws region "atth_exp" (e^{2 att_h}, f32 [T][B][E]): what the live-steps kernel reads in place of att_h"""
    e = walk.io.e
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    e._ck(e.lib.lxo_ws_region(e.sref(), b"atth_exp", ctypes.byref(off), ctypes.byref(nb)), "ws_region")
    return nb.value


def test_chain_r84_t7():
    """the persistent chains, B = 8, 64 x 128 (R = 84: the last 16-region workgroup has one wave with regions and three without), T = 7 (a
    group of 4 and a remainder of 3); lengths 6, 1 and mixed ones up to 7"""
    w = G.run_case("datt_img chain B8 64x128 T7", 8, 64, 128, 7, step_kernels=0)
    assert w.io.R == 84 and w.io.chain
    assert sorted(w.lengths.tolist())[0] == 1 and w.lengths[0] == 6 and w.lengths.max() == 7
    assert table_bytes(w) == 7 * 8 * 256 * 4


def test_fused_r51_full_first_row():
    """the fused step kernels, B = 3, 40 x 150 (R = 51, Rp = 56: a wave with 3 live regions beside a poisoned padding column), T = 5,
    first_len = T: row 0 has no trailing dead step, row 1 has length 1"""
    w = G.run_case("datt_img fused B3 40x150 T5", 3, 40, 150, 5, first_len=5)
    assert w.fused and (w.io.R, w.io.Rp) == (51, 56)
    assert w.lengths[0] == 5 and w.lengths[1] == 1


def test_fused_r51_deterministic():
    """the same shape with lxo_shape.deterministic: d_beta through one slot per workgroup, added in order"""
    w = G.run_case("datt_img fused deterministic B3 40x150 T5", 3, 40, 150, 5, first_len=5, deterministic=True)
    assert w.fused and w.io.det


def test_dead_rows_t2():
    """B = 8 with live_B = 3, 50 x 120, T = 2: the dead rows of the filled-up batch give n = 0 (no step walked), the live ones a range shorter
    than one group of 4"""
    w = G.run_case("datt_img B8 live3 50x120 T2", 8, 50, 120, 2, live_B=3)
    assert w.lengths[3:].max() == 0


def test_e512_keeps_the_step_masked_kernel():
    """E = 512 (> 256): no table region, datt_img_kernel as before, still within its bounds"""
    w = G.run_case("datt_img E512 B3 40x150 T5", 3, 40, 150, 5, dims=dict(C=256, E=512, U=128, O=128, D=16))
    assert table_bytes(w) == 0
