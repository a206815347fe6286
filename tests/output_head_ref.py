"""TEST INFRASTRUCTURE: constructed logits for the decoder output head (lxo_ce_loss_fwd_bwd, lxo_score_tokens) and their float64
reference.  Shared by tests/test_output_head_sim.py (hipsim) and tests/test_gpu_output_head.py (MI355X).

Logits rows are row = t * B + b with a stride of Vp = V rounded up to 32; only columns [0, V) are the model's, [V, Vp) are padding that
no kernel may read into a result.  The kernels clamp a target id outside [0, V) into it (tgt < 0 -> 0, tgt >= V -> V - 1)."""
import numpy as np

# the smallest vocabulary a shape may have (lxo_shape: V >= 4), every row-kernel instantiation (KV = 4, 8, 16 for Vp <= 256, 512, 1024)
# and the strided kernels (Vp > 1024), both sides of each boundary, and the worst padding (33 -> Vp 64)
VOCABS = (4, 33, 256, 257, 511, 512, 513, 1000, 1024, 1025, 3000)
CASES = ("normal", "large", "dominant", "ties", "target_edges", "target_out_of_range", "dead_rows")
POISONS = ("nan", "huge")          # what fills columns [V, Vp): NaN, and +1e30 (would win every max and swamp every sum)


def vpad(V):
    return (V + 31) // 32 * 32


def make_case(case, V, B, T, seed):
    """-> (logits f32 [T * B, V], formula int32 [B, T], lengths int32 [B])"""
    rng = np.random.default_rng([seed, V, B, T, CASES.index(case)])
    n = T * B
    x = rng.standard_normal((n, V)) * 2.0
    f = rng.integers(0, V, size=(B, T))
    ln = rng.integers(1, T + 1, size=B)
    ln[0] = T                                                      # one full row
    if case == "large":
        # |x| ~ 100: an unshifted exp overflows f32 (e^89 > 3.4e38), a shifted one does not; the sign alternates by row
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]
        x = sign * 100.0 + rng.standard_normal((n, V))
    elif case == "dominant":
        # one logit 40 above the rest: p ~ 1 there, ~e^-40 elsewhere; the target is the dominant column in half of the rows
        d = rng.integers(0, V, size=n)
        x[np.arange(n), d] += 40.0
        fl = f.T.reshape(-1)                                       # row order t * B + b
        half = np.arange(n) % 2 == 0
        fl[half] = d[half]
        f = fl.reshape(T, B).T
    elif case == "ties":
        # exact f32 ties at the maximum (three columns, spread over the row), and many ties below it
        x = np.round(x * 2.0) / 2.0
        for r in range(n):
            cols = rng.choice(V, size=min(3, V), replace=False)
            x[r, cols] = x[r].max() + 1.0
    elif case == "target_edges":
        f = np.where((np.arange(B)[:, None] + np.arange(T)[None, :]) % 2 == 0, 0, V - 1)
    elif case == "target_out_of_range":
        bad = np.array([-1, -7, V, V + 5, 1 << 30, -(1 << 30)])
        f = np.where(rng.random((B, T)) < 0.5, bad[rng.integers(0, len(bad), size=(B, T))], f)
    elif case == "dead_rows":
        ln = rng.integers(0, max(T // 3, 1) + 1, size=B)
        ln[0], ln[-1] = 0, T                                       # a sample without any token, one full
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(f, np.int32), np.ascontiguousarray(ln, np.int32)


def padded(logits, Vp, poison):
    """[n, V] -> [n, Vp] with the padding columns 0 (poison None), NaN or +1e30"""
    n, V = logits.shape
    fill = {None: 0.0, "nan": np.nan, "huge": 1e30}[poison]
    out = np.full((n, Vp), fill, np.float32)
    out[:, :V] = logits
    return out


def reference(logits, formula, lengths):
    """float64 reference of the head on f32 logits [T * B, V] -> dict:
    lse [n], live [B, T], tgt (clamped) [B, T], logp [B, T] (0 on dead rows), top1 [B, T] (first maximum; -1 on dead rows),
    ce (sum over live rows of lse - x[tgt]), ntok, dlogits [n, V] = (softmax - onehot) / ntok on live rows, 0 on dead rows."""
    B, T = formula.shape
    x = logits.astype(np.float64)
    n, V = x.shape
    m = x.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]
    live = np.arange(T)[None, :] < lengths[:, None]
    tgt = np.clip(formula.astype(np.int64), 0, V - 1)
    rows = (np.arange(T)[None, :] * B + np.arange(B)[:, None])        # [B, T] -> row t * B + b
    xt = x[rows, tgt]
    logp = np.where(live, xt - lse[rows], 0.0)
    top1 = np.where(live, logits.argmax(axis=1)[rows], -1)           # on the f32 values: exact ties, the lower index first
    ntok = int(live.sum())
    live_row = np.zeros(n, bool)
    live_row[rows[live]] = True
    d = np.exp(x - lse[:, None])
    tgt_row = np.zeros(n, np.int64)
    tgt_row[rows.reshape(-1)] = tgt.reshape(-1)
    d[np.arange(n), tgt_row] -= 1.0
    d *= np.where(live_row, 1.0 / max(ntok, 1), 0.0)[:, None]
    return dict(lse=lse, live=live, tgt=tgt, logp=logp, top1=top1, ce=float(-logp[live].sum()), ntok=ntok, dlogits=d, rows=rows)


def ordered_sum(x):
    """np.float32 sum in ascending order (what score_seq_kernel promises)"""
    s = np.float32(0.0)
    for v in x:
        s = np.float32(s + np.float32(v))
    return s


def logp_tol(logits):
    """absolute bound on |logp - reference| and on the log-sum-exp behind d(logits): 1e-5 at moderate logits (tests/test_gpu_score.py's
    scale), growing with the magnitude of the row (an f32 lse of ~100 carries an ulp of 7.6e-6).  Measured on the MI355X over the whole
    matrix: 1.9e-6 at |x| <= 45 (bound 1e-5 .. 6e-5), 4.2e-6 at |x| ~ 100 (bound 1.3e-4); the CE sum 5.9e-3 over 9664 rows (bound 5e-2)."""
    return 1e-5 * max(1.0, float(np.abs(logits).max()) / 8.0)


def check(ref, logits, V, Vp, loss, dl, logp, top1, seq, bf16):
    """Assert the kernels' outputs against the reference; -> dict of the measured worst errors.
    loss = (sum CE, token count) f32, dl = d(logits) [n, Vp] as f32 (bf16 mode: the bf16 values widened), logp / top1 [B, T], seq [B]."""
    tol = logp_tol(logits)
    live = ref["live"]
    B, T = live.shape
    ntok = ref["ntok"]
    out = {}
    # token count exact, CE sum: per row within tol, summed in f32 over at most a few thousand rows
    assert float(loss[1]) == float(ntok), (loss[1], ntok)
    out["ce"] = abs(float(loss[0]) - ref["ce"])
    assert out["ce"] <= tol * max(ntok, 1) + 2e-6 * abs(ref["ce"]), (float(loss[0]), ref["ce"], out["ce"])
    # log-probs and top-1
    out["logp"] = float(np.abs(logp - ref["logp"])[live].max()) if live.any() else 0.0
    assert out["logp"] <= tol, (out["logp"], tol)
    assert (logp[~live] == 0).all() and (top1[~live] == -1).all()
    assert np.array_equal(top1, ref["top1"]), np.argwhere(top1 != ref["top1"])[:8]
    for b in range(B):
        assert seq[b].tobytes() == ordered_sum(logp[b, :ref["live"][b].sum()]).tobytes(), (b, seq[b])
    # d(logits): the padding columns exactly 0, dead rows exactly 0, live rows (softmax - onehot) / ntok
    assert (dl[:, V:Vp] == 0).all() and not np.signbit(dl[:, V:Vp]).any()
    g, r = dl[:, :V].astype(np.float64), ref["dlogits"]
    err = np.abs(g - r)
    inv = 1.0 / max(ntok, 1)
    p = np.exp(logits.astype(np.float64) - ref["lse"][:, None])
    # f32: the softmax carries the log-sum-exp's error (relative tol) and an ulp or two of exp; (p - onehot) * inv_ntok one rounding more
    # (measured: at most 0.57 of this bound; bf16: 0.99 -- the half-ulp rounding of values just above a power of two fills its share)
    bar = (2.0 * tol + 2.0 ** -21) * p * inv + 2.0 ** -22 * np.abs(r)
    if bf16:
        bar += 2.0 ** -8 * np.abs(r)              # one bf16 rounding of the exact value (half an ulp <= 2^-8 |value|)
    out["dlogits"] = float((err / np.maximum(bar, 1e-300)).max())          # worst error as a fraction of its bound
    assert (err <= bar).all(), (np.argwhere(err > bar)[:4], float(err.max()))
    dead = ~np.isin(np.arange(dl.shape[0]), ref["rows"][live])
    assert (dl[dead] == 0).all()
    return out
