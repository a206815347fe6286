"""-m gpu: the forward chain (csrc/xdec.hip, xdec_fwd_kernel) behind a formula's end.  With the lengths (lxo_decoder_train_fwd_live,
Engine.forward(lengths=)) a pair (t, b) with t >= lengths[b] is dead: P3 of its workgroups walks no block and publishes a zero partial, P4 merges an
exact zero context and writes an exact zero alpha row, and the rest of the record is what the step makes of that.

What must hold: every live position equal to the call without lengths bit for bit (1; the forward has no atomics); exact zeros in alpha and ctx and
finite values everywhere behind the end, the same bytes from a second call and over a poisoned workspace (2); a row's live positions independent of
the other rows' lengths (3); the training step (4) and the scoring (5) that use the call equal byte for byte to the ones that do not; and off the
chain the call IS the old one (6).  One chain batch per kernel instantiation (1, 2, 4, 8 samples per chain), V = 120, T = 25, lengths U{5..24}
with planted rows: length 0, 1 and T, a last chain whose samples all end by step 7, and -- row 2 being the only one of length T -- a last step
with exactly one live row in the batch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa

V, T = 120, 25
SHAPES = {8: (40, 150), 16: (64, 128), 32: (48, 200), 64: (64, 256)}
REGIONS = ("logits", "rec", "cs", "gates", "att_h", "alpha")
OFF_CTX = 1536                                                    # record columns [o | h | h~ | ctx], 512 each


def _regions(H, W):
    return (-(-H // 8) - 2) * (-(-W // 8) - 2)


def _images(B, seed=11):
    H, W = SHAPES[B]
    imgs, _ = synthetic.make_set(B, H, W, V, 1, 2, seed=seed)
    return pad_batch_images(imgs)


def _lengths(B):
    l = np.random.default_rng(100 + B).integers(5, 25, size=B).astype(np.int32)
    l[0], l[1], l[2] = 0, 1, T
    nb = B // 8
    l[B - nb:] = np.minimum(l[B - nb:], 7)                         # the last chain's samples all end long before the batch does
    assert (l == T).sum() == 1 and l.max() == T                    # step T - 1: one live row in the whole batch
    return l


def _formula(l, seed=3):
    f = np.random.default_rng(seed).integers(0, V - 3, size=(len(l), T)).astype(np.int32)
    for b, n in enumerate(l):
        f[b, n:] = V - 2
        if n > 0:
            f[b, n - 1] = V - 1
    return f


def _live_mask(l):
    return np.arange(T)[:, None] < np.asarray(l)[None, :]          # [T, B]


def _snap(eng, B):
    torch.cuda.synchronize()
    R = _regions(*SHAPES[B])
    Rp, Vp = (R + 7) // 8 * 8, (V + 31) // 32 * 32
    out = {"logits": eng.region("logits", "f32", (T, B, Vp))[:, :, :V], "rec": eng.region("rec", "f32", (T + 1, B, 2048)),
           "cs": eng.region("cs", "f32", (T + 1, B, 512)), "gates": eng.region("gates", "f32", (T, B, 2048)),
           "att_h": eng.region("att_h", "f32", (T, B, 256)), "alpha": eng.region("alpha", "f32", (T, B, Rp))[:, :, :R]}
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _steps(snap, k):
    """region k by step: the state regions keep the initial state in slot 0"""
    return snap[k][1:] if k in ("rec", "cs") else snap[k]


def _poison(eng):
    """alpha, rec and att_part hold NaN before the call.  No region had to be dropped, the old path passes the same check below; of rec, slot 0
    is left out: the initial state is [o | h], its [h~ | ctx] columns are written -- and read -- by no call, with or without lengths, so they
    keep whatever they held and would fail the comparison for either path."""
    B = int(eng.shape.B)
    for name in ("alpha", "rec", "att_part"):
        eng.region(name)[B * 2048 if name == "rec" else 0:].fill_(float("nan"))


_RUNS = {}


def _run(B, lengths=None, drop=None, twice=False):
    """One engine, one forward with the given lengths (None: the call without lengths); twice: a second forward over the poisoned workspace.
    -> (first snapshot, second snapshot or None).  Kept: the tests share the runs."""
    key = (B, None if lengths is None else tuple(int(x) for x in lengths), drop, twice)
    if key not in _RUNS:
        l = _lengths(B)
        eng = Engine(V, dtype="bf16", seed=9)
        img, f = _images(B), _formula(l)
        kw = {} if lengths is None else {"lengths": np.asarray(lengths, np.int32)}
        eng.forward(img, f, dropout=drop, **kw)
        first, second = _snap(eng, B), None
        assert eng.chain_status() == (True, 0)
        if twice:
            _poison(eng)
            eng.forward(img, f, dropout=drop, **kw)
            second = _snap(eng, B)
            assert eng.chain_status() == (True, 0)
        assert int(eng.shape.B) == B
        _RUNS[key] = (first, second)
    return _RUNS[key]


_CASES = [(8, None), (16, None), (32, None), (64, None), (16, (0.85, 99))]
_IDS = ["one_sample_per_chain", "two_samples_per_chain", "four_samples_per_chain", "eight_samples_per_chain", "two_samples_per_chain_dropout"]


@pytest.mark.parametrize("B,drop", _CASES, ids=_IDS)
def test_live_positions_are_bit_identical(B, drop):
    l = _lengths(B)
    new, _ = _run(B, l, drop, twice=drop is None)
    old, _ = _run(B, None, drop, twice=drop is None)
    live = _live_mask(l)
    assert live.any() and not live.all()
    for k in REGIONS:
        a, b = _steps(new, k), _steps(old, k)
        assert b[live].any(), k
        assert _same(a[live], b[live]), (k, int((_bits(a[live]) != _bits(b[live])).sum()))
    for k in ("rec", "cs"):
        assert _same(new[k][0], old[k][0]), k                     # the initial state


@pytest.mark.parametrize("B", [8, 16, 32, 64])
def test_dead_positions(B):
    l = _lengths(B)
    first, second = _run(B, l, None, twice=True)
    dead = ~_live_mask(l)
    assert dead[:, 0].all() and dead[T - 1].sum() == B - 1
    assert not first["alpha"][dead].any()                           # exact zeros (-0.0 == 0: the sign of a zero is not looked at)
    assert not first["rec"][1:][dead][:, OFF_CTX:].any()
    assert first["alpha"][~dead].any() and first["rec"][1:][~dead][:, OFF_CTX:].any()
    for k in REGIONS:
        assert np.isfinite(first[k]).all(), k
        assert _same(first[k], second[k]), k                        # a second call, over NaN in alpha, rec and att_part: the same bytes
    # the old path under the same poison (it holds on the parent library too: the poison list needs no exception)
    o1, o2 = _run(B, None, None, twice=True)
    for k in REGIONS:
        assert np.isfinite(o1[k]).all(), k
        assert _same(o1[k], o2[k]), k


@pytest.mark.parametrize("B", [8, 16, 32, 64])
def test_a_row_does_not_depend_on_the_other_rows_lengths(B):
    l = _lengths(B)
    a, _ = _run(B, l, None, twice=True)
    nb = B // 8
    for rows in ([1, 3, B - 1], [0, 2, 4, B - nb]):                 # (with their chain neighbours at full length)
        lz = np.full(B, T, np.int32)
        lz[rows] = l[rows]
        z, _ = _run(B, lz)
        live = _live_mask(l)[:, rows]
        for k in REGIONS:
            assert _same(_steps(a, k)[:, rows][live], _steps(z, k)[:, rows][live]), (k, rows)


def _train_batch(Bc, live_B):
    l = _lengths(Bc)[:live_B].copy()
    if live_B < Bc:
        l[live_B - 1] = T
    H, W = SHAPES[Bc]
    imgs, _ = synthetic.make_set(live_B, H, W, V, 1, 2, seed=17)
    return pad_batch_images(imgs), _formula(l, seed=5), l


def _state(eng):
    torch.cuda.synchronize()
    return {"loss": eng.region("loss")[:2].cpu().numpy().copy(), "grads": eng.grads.cpu().numpy().copy(), "params": eng.params.cpu().numpy().copy()}


@pytest.mark.parametrize("Bc,live_B", [(16, 16), (64, 64), (32, 20)], ids=["B16", "B64", "B20_in_32"])
def test_training_step(Bc, live_B):
    """two consecutive train_steps (forward with lengths) against forward() without lengths + loss + backward + optimizer_step, deterministic bf16"""
    img, f, l = _train_batch(Bc, live_B)
    n = float(l.sum())
    new, old = Engine(V, dtype="bf16", seed=4, deterministic=True), Engine(V, dtype="bf16", seed=4, deterministic=True)
    for step in range(2):
        loss = new.train_step(img, f, l, 1e-3)
        a = _state(new)
        old.forward(img, f)
        old.loss(l, 1.0 / n)
        old.backward()
        old.optimizer_step(1e-3, -1.0, guard=True)
        b = _state(old)
        assert int(new.shape.B) == Bc and new.live_B == live_B
        for e in (new, old):
            assert e.chain_status() == (True, 0) and e.chain_status(backward=True) == (True, 0) and e.chain_failures == 0
        assert np.isfinite(loss) and loss == float(b["loss"][0]) / float(b["loss"][1])
        for k in a:
            assert np.isfinite(a[k]).all() and a[k].any(), (step, k)
            assert _same(a[k], b[k]), (step, k, int((_bits(a[k]) != _bits(b[k])).sum()))


@pytest.mark.parametrize("Bc,live_B", [(16, 16), (32, 20)], ids=["B16", "B20_in_32"])
def test_scoring(Bc, live_B, monkeypatch):
    img, f, l = _train_batch(Bc, live_B)
    eng = Engine(V, dtype="bf16", seed=4)
    new = eng.score(img, f, l, return_top1=True)
    assert eng.chain_status() == (True, 0)
    plain = Engine._decoder_fwd
    calls = []
    monkeypatch.setattr(Engine, "_decoder_fwd", lambda self, st, live: (calls.append(live), plain(self, st, False))[1])      # the old entry point
    eng2 = Engine(V, dtype="bf16", seed=4)
    old = eng2.score(img, f, l, return_top1=True)
    assert eng2.chain_status() == (True, 0) and calls and all(calls)
    for a, b, name in zip(new, old, ("logp", "top1", "seq")):
        assert a.shape == b.shape and a.any(), name
        assert _same(a, b), name


@pytest.mark.parametrize("dtype,step_kernels", [("bf16", 2), ("f32", 0)], ids=["launch_per_step", "f32"])
def test_off_the_chain_the_call_is_the_old_one(dtype, step_kernels):
    B = 16
    l = _lengths(B)
    img, f = _images(B), _formula(l)
    out = []
    for kw in ({"lengths": l}, {}):
        eng = Engine(V, dtype=dtype, seed=9)
        eng.step_kernels = step_kernels
        eng.forward(img, f, **kw)
        out.append(_snap(eng, B))
        if dtype == "bf16":                                        # (f32 has no chain and no status words)
            used, err = eng.chain_status()
            assert not used and err == 0
    for k in REGIONS:
        assert np.isfinite(out[0][k]).all() and out[0][k].any(), k
        assert _same(out[0][k], out[1][k]), k
