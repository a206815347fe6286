"""-m gpu: the decode step stage by stage on the GPU.  lxo_decode_begin, lxo_decode_cell_step, lxo_decode_step and lxo_decode_state_set on
the state the kernels themselves stored, the last step of a whole lxo_beam_decode_scores loop (the parent indirection, and in a child process
the re-ordering launch) and the last step of the persistent greedy-decode chain with its tail: every region checked element by element
against the float64 reference of tests/decoder_steps_ref.py applied to the operands the kernels read (tests/decode_steps_walk.py), with the
bounds of the training walk.  Default widths (C = U = O = 512, E = 256), 40 x 150 (R = 51, Rp = 56) unless noted.  Each case prints its
worst err / bound per check."""
import os
import subprocess
import sys

import pytest
import torch

from latex_ocr_amd.engine import Engine
import decode_steps_walk as XW

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def make(case, B, V=120, k=1, H=40, W=150, bf=True, dims=None, step_kernels=2, seed=3):
    e = Engine(V, dims=dims, dtype="bf16" if bf else "f32", device="cuda:0", seed=seed, beam=k, max_steps=24)
    e.step_kernels = step_kernels
    return XW.DecodeWalk(XW.EngineIO(e, B, H, W, k=k, seed=seed), case)


def done(w):
    w.report()
    torch.cuda.synchronize()
    return w


def test_greedy_bf16_fused():
    """B = 3: one partial 16-row tile, the token table, the E-domain attention, the logits on the step kernel (V = 120)"""
    w = make("greedy bf16 fused B3", 3)
    assert w.fused and w.mirr and w.expd
    w.run(3, force_at=2)
    done(w)


def test_beam5_bf16_fused_forced_ids_and_state():
    """B = 8, k = 5: 40 rows on 32-row tiles (one full, one partial), image v / k, tiled initial states, the re-ordering bit for bit; at step 2
    the ids and h / o are given through lxo_decode_state_set"""
    w = make("beam 5 bf16 fused B8, forced ids", 8, k=5)
    assert w.fused and w.mirr and w.expd
    w.run(4, force_at=2)
    done(w)


def test_beam5_dense_logits_above_64_rows():
    """B = 16, k = 5 (80 rows), V = 121: the logits on the dense GEMM with `small` off"""
    w = make("beam 5 bf16 B16 V121", 16, V=121, k=5)
    w.run(3)
    done(w)


def test_beam3_dense_logits_small():
    """B = 4, k = 3 (12 rows), V = 121: the logits on the dense GEMM at <= 64 rows"""
    w = make("beam 3 bf16 B4 V121", 4, V=121, k=3)
    w.run(3)
    done(w)


def test_beam3_f32_fused():
    """the f32 parity mode: the harness itself at 2^-20 S"""
    w = make("beam 3 f32 fused B4", 4, k=3, bf=False)
    assert w.fused and not w.mirr
    w.run(3)
    done(w)


def test_beam2_split_k():
    """step_kernels = 1: the split-K decode step (dec_emb, dec_zx, the x-domain attention kernel)"""
    w = make("beam 2 bf16 split-K B3", 3, k=2, step_kernels=1)
    assert not w.fused
    w.run(3, force_at=1)
    done(w)


def test_greedy_mixed_widths():
    """C = E = 256, U = O = 128, D = 16: falls to the split-K path by itself; no two operands of a product have the same shape"""
    w = make("greedy mixed widths B3", 3, dims=dict(C=256, E=256, U=128, O=128, D=16))
    assert not w.fused
    w.run(3)
    done(w)


def test_beam2_e512_x_domain():
    """E = 512: Plan::att_exp is off, the fused decode step runs the x-domain attention"""
    w = make("beam 2 bf16 E512 B2", 2, k=2, dims=dict(E=512))
    assert w.fused and not w.has_exp
    w.run(3)
    done(w)


def test_beam2_many_regions_160x800():
    """R = 1764: more than one attention chunk per row, with the two rows of a beam sharing an image"""
    w = make("beam 2 bf16 B2 160x800", 2, k=2, H=160, W=800)
    w.run(2)
    done(w)


def loop_case(B, m, seed, tag=""):
    w = make("beam 5 whole loop B%d m %d%s" % (B, m, tag), B, k=5, step_kernels=0, seed=seed)
    w.beam_last(m)
    return done(w)


@pytest.mark.parametrize("B,m,seed", [(3, 2, 3), (3, 3, 3), (8, 9, 4)])
def test_beam_loop_last_step_reads_through_the_parents(B, m, seed):
    """lxo_beam_decode_scores(max_iter = m), default environment: step m read [o | h], c and the table row through the parents of step m - 1,
    in place; m = 9 is a step of the second enqueue of 8.  The seeds are chosen with oracle.ref_model.beam_decode: at step m - 1 one image
    has a parent row that is not the identity and one repeats a parent (the walk asserts both on the device's own parents)"""
    w = loop_case(B, m, seed)
    assert w.fused and w.io.indirect


def test_beam_loop_last_step_with_the_reordering_launch():
    """LXO_BEAM_INDIRECT=0 (read once per process, so in a child): the gather path inside the loop"""
    env = dict(os.environ, LXO_BEAM_INDIRECT="0")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_decode_steps as T; w = T.loop_case(3, 3, 3, ' re-ordered'); "
            "assert w.fused and not w.io.indirect") % (HERE, os.path.dirname(HERE))
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    print(out[-3000:])
    assert r.returncode == 0, out[-3000:]


@pytest.mark.parametrize("B,H,W,m", [(8, 50, 120, 3), (16, 64, 128, 15), (16, 64, 128, 16)])
def test_greedy_chain_last_step(B, H, W, m):
    """the persistent greedy-decode chain (step_kernels = 0): a step in the middle of a launch (m = 3), the last step of a launch (m = 15) and the
    first step of the next (m = 16: c re-read from cs, the ids handed across launches)"""
    w = make("greedy chain B%d %dx%d m %d" % (B, H, W, m), B, H=H, W=W, step_kernels=0)
    w.chain_last(m)
    done(w)
