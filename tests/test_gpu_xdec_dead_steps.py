"""-m gpu: the backward chain (csrc/xdec.hip, xdec_bwd_kernel) behind a formula's end.  A step t at or behind a row's length has d_o(logits) = 0
and nothing carried into it, so its d_ctx is 512 exact zeros; phase Q2 of such a step streams no block: it stores the zeros of its d_e columns,
publishes a zero d_att_h partial and leaves the stream's software pipeline cold, and the row's first live step requests its own first blocks.

What must hold: exact zeros behind the end (1), the live steps of a row that had a dead prefix equal to the same row without one, bit for bit
(2: rows are independent through the recurrence, and the walk's direction is t & 1 with absolute t, so this also holds without the skip),
a second backward over one record equal to the first (3: no stale register, no flag left over), and the shapes at which the block loop takes
its other arms against the launch-per-step backward at the bars of test_gpu_xdec.py (4).  Formulas are built by hand: the lengths are the test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa

V = 120


def _regions(H, W):
    return (-(-H // 8) - 2) * (-(-W // 8) - 2)


def _images(B, H, W, seed):
    imgs, _ = synthetic.make_set(B, H, W, V, 1, 2, seed=seed)
    return pad_batch_images(imgs)


def _formulas(lengths, seed):
    """one token row per length, each row from its own stream: row b is the same in every batch that gives it the same length"""
    return [[int(x) for x in np.random.default_rng(seed * 1000 + b).integers(0, V - 3, size=n)] for b, n in enumerate(lengths)]


def _forward(img, lengths, seed, dropout=None, inv_ntok=None, eng_seed=9, deterministic=None):
    f, l = pad_batch_formulas(_formulas(lengths, seed), V - 2, V - 1)
    eng = Engine(V, dtype="bf16", seed=eng_seed, deterministic=deterministic)
    eng.forward(img, f, dropout=dropout)
    eng.loss(l, inv_ntok if inv_ntok is not None else 1.0 / int(l.sum()))
    return eng, f, l


def _fwd_snap(eng, T, R):
    torch.cuda.synchronize()
    B, Rp = int(eng.shape.B), (R + 7) // 8 * 8
    out = {"rec": eng.region("rec", "f32", (T + 1, B, 2048)), "cs": eng.region("cs", "f32", (T + 1, B, 512)),
           "alpha": eng.region("alpha", "f32", (T, B, Rp))[:, :, :R], "att_h": eng.region("att_h", "f32", (T, B, 256))}
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _bwd_snap(eng, T, R):
    torch.cuda.synchronize()
    B, Rp = int(eng.shape.B), (R + 7) // 8 * 8
    out = {"g": eng.region("g", "f32", (T, B, 512)), "dhc": eng.region("dhc", "f32", (T, B, 1024)),
           "de": eng.region("de", "f32", (T, B, Rp))[:, :, :R], "datth": eng.region("datth", "f32", (T, B, 256)),
           "dz": eng.region("dz", "f32", (T, B, 2048)), "dxh": eng.region("dxh", "f32", (B, 1024)), "dcc": eng.region("dcc", "f32", (B, 512))}
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _chains_ran(eng):
    for backward in (False, True):
        used, err = eng.chain_status(backward=backward)
        assert used and err == 0, (backward, used, err)


def _finite(snap):
    for k, v in snap.items():
        assert np.isfinite(v).all(), k


@pytest.mark.parametrize("lengths", [[24, 1, 2, 3, 1, 2, 3, 1, 24, 3, 2, 1, 12, 1, 2, 3], [6] * 16],
                         ids=["full_row_beside_rows_of_1_to_3", "equal_lengths_no_dead_step"])
def test_exact_zeros_behind_the_end(lengths):
    B, H, W = 16, 40, 150
    R = _regions(H, W)
    eng, f, l = _forward(_images(B, H, W, 11), lengths, seed=1)
    T = f.shape[1]
    eng.backward()
    s = _bwd_snap(eng, T, R)
    _chains_ran(eng)
    _finite(s)
    assert [int(x) for x in l] == [n + 1 for n in lengths]
    for b in range(B):
        n = int(l[b])
        for k in ("de", "datth", "dz", "g", "dhc"):
            assert not s[k][n:, b].any(), (k, b, n)               # (-0.0 == 0: the sign of a zero is not looked at)
            assert s[k][n - 1, b].any() and s[k][0, b].any(), (k, b, n)      # ... and the row's last live step is not among them


@pytest.mark.parametrize("n", [5, 6], ids=["n_odd", "n_even"])
@pytest.mark.parametrize("B,H,W", [(8, 64, 128), (64, 96, 256)], ids=["one_block_one_sample_per_chain", "three_blocks_eight_samples_per_chain"])
def test_live_steps_behind_a_dead_prefix_equal_the_row_without_one(B, H, W, n):
    """Sample 1 has n tokens.  In batch X other samples are much longer: BPTT reaches sample 1 through a long dead prefix and its first live step
    starts the stream cold.  In batch Z no row is longer: sample 1 is live from the kernel's prologue on.  Same images, same sample 1, no dropout,
    the same loss normaliser.  Rows are independent and the walk's direction is t & 1 in both, so sample 1's record and its BPTT agree bit for bit
    -- except the f32 g of its last step, which the two batches take from two kernels (below; measured 1.16e-10 at |g| 1.6e-3, a last bit).
    Holds with and without the skip: the parent's library passes it too.
    (8, 64 x 128: R = 84, 32 chunks of 3 rows, the last four empty, one block each; 64, 96 x 256: R = 300, 4 chunks of 75 rows, blocks A, B, A.)"""
    R = _regions(H, W)
    img = _images(B, H, W, 23)
    lx = [(21, n, 3, 17, 1, 9, 2, 13)[b % 8] for b in range(B)]
    lz = [min(v, n - (b % 3 == 2)) for b, v in enumerate(lx)]
    lz[1] = n
    assert max(lz) == n and lx[1] == n and max(lx) > 3 * n
    out = []
    for lengths in (lx, lz):
        eng, f, l = _forward(img, lengths, seed=2, inv_ntok=1.0 / 64)
        T = f.shape[1]
        fw = _fwd_snap(eng, T, R)
        eng.backward()
        bw = _bwd_snap(eng, T, R)
        _chains_ran(eng)
        _finite(fw); _finite(bw)
        out.append((fw, bw, T, f[1, :n + 1].copy()))
    (fx, bx, Tx, tx), (fz, bz, Tz, tz) = out
    assert Tx == max(lx) + 1 and Tz == n + 1 and np.array_equal(tx, tz)
    for k in ("rec", "cs"):
        assert np.array_equal(fx[k][:n + 2, 1], fz[k][:n + 2, 1]), k
    for k in ("alpha", "att_h"):
        assert np.array_equal(fx[k][:n + 1, 1], fz[k][:n + 1, 1]), k
    for k in ("de", "datth", "dz", "dhc", "g"):
        top = n if k == "g" else n + 1                            # g: slot n apart, below
        d = float(np.abs(bx[k][:top, 1] - bz[k][:top, 1]).max())
        print("B=%d n=%d %s: steps 0..%d of sample 1, X against Z: max |diff| %.3e" % (B, n, k, top - 1, d))
        assert bz[k][:top, 1].any(), k
        assert np.array_equal(bx[k][:top, 1], bz[k][:top, 1]), (k, d)
    # g_n is the one value of these that the two batches take from different kernels: in Z step n is the last one, and slot T - 1 of g is the
    # chain's INPUT (tanh_bwd_kernel: d_o (1 - o^2)); in X the chain's own Q4 of step n + 1 forms it as (d_o + carry) (1 - o^2) with a carry of
    # exact zeros.  Two compilations of one expression: th * th may or may not be contracted into the subtraction (an error of 2^-24 absolute in
    # 1 - th^2, times |d_o|), and each of the two products rounds once (2^-24 relative each).  What BPTT consumes of it, the bf16 mirror, is held
    # bit for bit by dhc[n] = g_n o_W^T above.  (The parent library shows the same last-bit difference in g_n and nothing else.)
    gx, gz = bx["g"][n, 1].astype(np.float64), bz["g"][n, 1].astype(np.float64)
    d_o = np.abs(eng.region("do_log", "f32", (Tz, B, 512))[n, 1].cpu().numpy().astype(np.float64))
    bound = 2.0 ** -23 * d_o + 2.0 ** -22 * np.abs(gz)
    print("B=%d n=%d g_n: max |diff| %.3e at max |g_n| %.3e; %d of 512 differ; largest diff / bound %.3f" % (
        B, n, np.abs(gx - gz).max(), np.abs(gz).max(), int((gx != gz).sum()), float((np.abs(gx - gz) / np.maximum(bound, 1e-300)).max())))
    assert gz.any() and (np.abs(gx - gz) <= bound).all()


def test_backward_twice_over_one_record():
    """(the ordered-reduction mode: with float atomics the encoder's weight gradients differ from run to run whatever the chain does)"""
    B, H, W = 16, 48, 160
    R = _regions(H, W)
    eng, f, l = _forward(_images(B, H, W, 31), [20, 2, 7, 1, 13, 3, 20, 5, 1, 9, 2, 16, 4, 11, 1, 6], seed=3, deterministic=True)
    T = f.shape[1]
    eng.backward()
    a, ga = _bwd_snap(eng, T, R), eng.grad_dict()
    _chains_ran(eng)
    eng.backward()
    b, gb = _bwd_snap(eng, T, R), eng.grad_dict()
    _chains_ran(eng)
    _finite(a); _finite(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k


_ARMS = [(8, 32, 128, None, "R28_over_32_chunks"), (64, 40, 150, None, "one_block_per_chunk"), (64, 96, 256, None, "three_blocks_per_chunk"),
         (32, 48, 200, (0.85, 99), "dropout"), (3, 50, 120, None, "chain_batch_8_with_dead_rows")]


@pytest.mark.parametrize("B,H,W,drop", [a[:4] for a in _ARMS], ids=[a[4] for a in _ARMS])
def test_block_loop_arms_against_launch_per_step_backward(B, H, W, drop):
    """One forward, then BPTT by the backward chain and by the launch-per-step kernels over the same record, at the bars of
    test_gpu_xdec.py::test_backward_chain_equals_launch_per_step_backward; lengths 1 .. 24, so most (step, row) pairs are dead."""
    R = _regions(H, W)
    lengths = [(1, 24, 2, 9, 3, 17, 5, 12)[b % 8] + (b // 8) % 3 for b in range(B)]
    lengths[B - 1] = 24
    eng, f, l = _forward(_images(B, H, W, 40 + B), lengths, seed=4, dropout=drop)
    T = f.shape[1]
    assert int(eng.shape.B) == (8 if B == 3 else B) and eng.live_B == B
    eng.backward()
    a, ga = _bwd_snap(eng, T, R), eng.grad_dict()
    _chains_ran(eng)
    eng.shape.step_kernels = 2                                   # the same record, the launch-per-step kernels
    eng.backward()
    b, gb = _bwd_snap(eng, T, R), eng.grad_dict()
    _finite(a); _finite(b)
    for k in a:
        d = np.abs(a[k] - b[k]).max() / max(np.abs(b[k]).max(), 1e-30)
        assert d < 2e-2, (k, d)
        assert cosine(a[k], b[k]) > 0.99999, (k, cosine(a[k], b[k]))
    for k in ga:
        assert cosine(ga[k], gb[k]) > 0.99995, (k, cosine(ga[k], gb[k]))
