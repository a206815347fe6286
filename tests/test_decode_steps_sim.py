"""CPU: the decode step stage by stage under the hipsim SIMT interpreter -- lxo_decode_begin, lxo_decode_cell_step, lxo_decode_step,
lxo_decode_state_set and the last step of a whole lxo_beam_decode_scores loop, every workspace region they store against the float64
reference of tests/decoder_steps_ref.py applied to the operands the kernels read (tests/decode_steps_walk.py) -- the mirror of
tests/test_gpu_decode_steps.py at small widths: C = E = U = O = 128, D = 16, a 25 x 57 image (R = 12, Rp = 16), three steps each."""
from latex_ocr_amd.engine import Engine
from simharness import lib
import decode_steps_walk as XW

SMALL = dict(C=128, E=128, U=128, O=128, D=16)
LOOP_SEED = 6      # the whole-loop case; oracle.ref_model.beam_decode: parents [0, 0, 1] and [0, 1, 0] at step 1, END not emitted


def make(case, B, V, k=1, bf=True, dims=None, step_kernels=2, seed=3, H=25, W=57):
    e = Engine(V, dims=dict(dims or SMALL), dtype="bf16" if bf else "f32", device="cpu", seed=seed, beam=k, max_steps=8, lib=lib())
    e.step_kernels = step_kernels
    return XW.DecodeWalk(XW.EngineIO(e, B, H, W, k=k, seed=seed), case)


def test_greedy_bf16_fused():
    """V = 12: the logits come from the step kernel (V % 4 == 0)"""
    w = make("sim greedy bf16 fused", 2, 12)
    assert w.fused and w.mirr and w.expd
    w.run(3)
    w.report()


def test_beam3_bf16_fused_forced_ids_and_state():
    """V = 11: the logits come from the dense GEMM; at step 1 the ids and h / o are given through lxo_decode_state_set"""
    w = make("sim beam 3 bf16 fused, forced ids", 2, 11, k=3)
    assert w.fused and w.mirr
    w.run(3, force_at=1)
    w.report()


def test_beam2_f32_fused():
    """the f32 parity mode: every sum held to 2^-20 S"""
    w = make("sim beam 2 f32 fused", 2, 11, k=2, bf=False)
    assert w.fused and not w.mirr and not w.expd
    w.run(3)
    w.report()


def test_beam2_bf16_split_k():
    """step_kernels = 1: the split-K decode step (dec_emb gathered, dec_zx, the x-domain attention)"""
    w = make("sim beam 2 bf16 split-K", 2, 11, k=2, step_kernels=1)
    assert not w.fused and w.has_exp and not w.expd
    w.run(3, force_at=2)
    w.report()


def test_greedy_bf16_mixed_widths():
    """C = E = 256, U = O = 128: falls to the split-K path by itself"""
    w = make("sim greedy bf16 mixed widths", 2, 11, dims=dict(C=256, E=256, U=128, O=128, D=16))
    assert not w.fused
    w.run(3)
    w.report()


def test_beam3_whole_loop_last_step():
    """lxo_beam_decode_scores(max_iter = 2): step 2 read its rows through the parents of step 1 (seed chosen with the oracle so that they are
    neither the identity nor free of repeats)"""
    w = make("sim beam 3 whole loop m 2", 2, 11, k=3, seed=LOOP_SEED)
    assert w.fused and w.io.indirect
    w.beam_last(2)
    w.report()

