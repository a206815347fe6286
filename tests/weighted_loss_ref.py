"""TEST INFRASTRUCTURE: float64 reference of the weighted loss (lxo_ce_loss_weighted) and of the minimum-risk weights (lxo_mrt_weights).
Shared by tests/test_weighted_loss_sim.py (hipsim) and tests/test_gpu_weighted_loss.py (MI355X).  The logits, their padding and the
unweighted float64 head come from tests/output_head_ref.py."""
import numpy as np

from output_head_ref import VOCABS, logp_tol, make_case, padded, reference, vpad  # noqa: F401  (re-exported for the two test files)

W_CASES = ("normal", "large", "target_out_of_range", "dead_rows")
W_MODES = ("tok", "row", "both")


def make_weights(ln, B, T, seed):
    """-> (w_tok f32 [B, T], w_row f32 [B]): mixed sign in [-2, 2]; one exact 0 on a live token and one whole zero row (a row with live
    tokens, where the case has two)"""
    rng = np.random.default_rng([seed, B, T])
    w_tok = rng.uniform(-2.0, 2.0, size=(B, T)).astype(np.float32)
    w_row = rng.uniform(-2.0, 2.0, size=B).astype(np.float32)
    live_rows = np.flatnonzero(ln > 0)
    b0 = int(live_rows[-1])                                        # (make_case: the first or the last row is full)
    w_tok[b0, int(ln[b0]) - 1] = 0.0                               # a live token that weighs nothing
    bz = int(live_rows[0]) if len(live_rows) > 1 else (b0 + 1) % B
    w_tok[bz, :] = 0.0                                             # a whole zero row, in either form of the weights
    w_row[bz] = 0.0
    return w_tok, w_row


def weighted_reference(logits, formula, lengths, w_tok, w_row, inv_norm):
    """float64 reference on f32 inputs: the dict of output_head_ref.reference plus w_eff [n] (row order t * B + b, 0 on dead rows),
    dlogits_w [n, V] = (softmax - onehot) * w_eff * inv_norm and stats = {sum w CE, ntok, sum w, sum CE} over the live tokens"""
    ref = reference(logits, formula, lengths)
    B, T = formula.shape
    w = np.ones((B, T), np.float64)
    if w_tok is not None:
        w = w * np.asarray(w_tok, np.float32).astype(np.float64)
    if w_row is not None:
        w = w * np.asarray(w_row, np.float32).astype(np.float64)[:, None]
    live, rows, ntok = ref["live"], ref["rows"], ref["ntok"]
    w_eff = np.zeros(logits.shape[0], np.float64)
    w_eff[rows[live]] = w[live]
    ce = -ref["logp"]
    ref["w"] = w
    ref["w_eff"] = w_eff
    ref["dlogits_w"] = ref["dlogits"] * max(ntok, 1) * w_eff[:, None] * float(np.float32(inv_norm))
    ref["stats"] = np.array([(w * ce)[live].sum(), float(ntok), w[live].sum(), ce[live].sum()], np.float64)
    return ref


def check_weighted(ref, logits, V, Vp, loss, dl, inv_norm, bf16):
    """Assert lxo_ce_loss_weighted's outputs (loss f32 [4], dl = d(logits) [n, Vp] widened to f32) -> dict of worst errors as fractions of their bars.
    The element bar is output_head_ref.check's with inv replaced by |w_eff| inv_norm; its 2^-22 |ref| term still holds: the two weight
    products add two f32 roundings and 3 * 2^-24 < 2^-22."""
    tol = logp_tol(logits)
    live, ntok = ref["live"], ref["ntok"]
    w = ref["w"]
    inv = float(np.float32(inv_norm))
    out = {}
    assert (dl[:, V:Vp] == 0).all()                                # the padding columns exactly 0
    dead = ~np.isin(np.arange(dl.shape[0]), ref["rows"][live])
    assert (dl[dead] == 0).all()                                   # rows past lengths[b] exactly 0
    g, r = dl[:, :V].astype(np.float64), ref["dlogits_w"]
    err = np.abs(g - r)
    p = np.exp(logits.astype(np.float64) - ref["lse"][:, None])
    bar = (2.0 * tol + 2.0 ** -21) * p * (np.abs(ref["w_eff"]) * inv)[:, None] + 2.0 ** -22 * np.abs(r)
    if bf16:
        bar += 2.0 ** -8 * np.abs(r)
    out["dlogits"] = float((err / np.maximum(bar, 1e-300)).max())
    assert (err <= bar).all(), (np.argwhere(err > bar)[:4], float(err.max()))
    st = ref["stats"]
    assert float(loss[1]) == float(ntok), (loss[1], ntok)          # the token count: exact, whatever the weights
    wmax = max(1.0, float(np.abs(w[live]).max())) if live.any() else 1.0
    for i in (0, 3):
        e, b = abs(float(loss[i]) - st[i]), tol * max(ntok, 1) * wmax + 2e-6 * abs(st[i])
        out["loss%d" % i] = e / b
        assert e <= b, (i, float(loss[i]), st[i], e, b)
    e, b = abs(float(loss[2]) - st[2]), 2.0 ** -22 * float(np.abs(w[live]).sum())
    out["loss2"] = e / max(b, 1e-300)
    assert e <= b, (float(loss[2]), st[2], e, b)
    return out


# ---------------------------------------------------------------------------------------------------------- minimum-risk weights --
MRT_SIZES = (1, 2, 5, 64, 65, 130)
MRT_TAIL = 3
MRT_ALPHAS = (0.005, 1.0)


def make_mrt_case(seed=0):
    """-> (seq_logp f32 [rows] in [-40, 0], cost f32 [rows] in [0, 2], group_off int32 [G + 1], rows = group_off[G] + MRT_TAIL)"""
    rng = np.random.default_rng([seed, 77])
    off = np.concatenate([[0], np.cumsum(MRT_SIZES)]).astype(np.int32)
    rows = int(off[-1]) + MRT_TAIL
    lp = rng.uniform(-40.0, 0.0, size=rows).astype(np.float32)
    cost = rng.uniform(0.0, 2.0, size=rows).astype(np.float32)
    return lp, cost, off, rows


def mrt_weights_ref(seq_logp, cost, group_off, alpha):
    """float64: Q = softmax(alpha seq_logp) per group, R_g = sum Q cost, w = alpha Q (R_g - cost); rows behind the last group 0.
    alpha is the f32 value the kernel receives.  -> (w [rows], q [rows], risk = sum_g R_g, R [G])"""
    lp, c = np.asarray(seq_logp, np.float32).astype(np.float64), np.asarray(cost, np.float32).astype(np.float64)
    a = float(np.float32(alpha))
    w, q = np.zeros(lp.shape[0]), np.zeros(lp.shape[0])
    R = np.zeros(len(group_off) - 1)
    for g in range(len(group_off) - 1):
        lo, hi = int(group_off[g]), int(group_off[g + 1])
        if hi <= lo:
            continue
        y = a * lp[lo:hi]
        e = np.exp(y - y.max())
        q[lo:hi] = e / e.sum()
        R[g] = (q[lo:hi] * c[lo:hi]).sum()
        w[lo:hi] = a * q[lo:hi] * (R[g] - c[lo:hi])
    return w, q, float(R.sum()), R


def check_mrt(seq_logp, cost, group_off, alpha, w, q, risk):
    """Assert lxo_mrt_weights' outputs against mrt_weights_ref -> worst errors as fractions of their bars.  eps = 2^-20 max(1, max |alpha seq_logp| / 8):
    the logp_tol style of bound on a short f32 chain (a product, a subtraction of up to |alpha seq_logp|, expf, a sum, a quotient)"""
    a = float(np.float32(alpha))
    rw, rq, rrisk, R = mrt_weights_ref(seq_logp, cost, group_off, alpha)
    c = np.asarray(cost, np.float64)
    eps = 2.0 ** -20 * max(1.0, float(np.abs(a * np.asarray(seq_logp, np.float64)).max()) / 8.0)
    out = {"w": 0.0, "q": 0.0}
    G = len(group_off) - 1
    for g in range(G):
        lo, hi = int(group_off[g]), int(group_off[g + 1])
        if hi <= lo:
            continue
        bw = eps * a * rq[lo:hi] * (np.abs(R[g] - c[lo:hi]) + np.abs(c[lo:hi]).max())
        ew = np.abs(w[lo:hi].astype(np.float64) - rw[lo:hi])
        assert (ew <= bw).all(), (g, float((ew / np.maximum(bw, 1e-300)).max()))
        out["w"] = max(out["w"], float((ew / np.maximum(bw, 1e-300)).max()))
        bq = eps * rq[lo:hi]
        eq = np.abs(q[lo:hi].astype(np.float64) - rq[lo:hi])
        assert (eq <= bq).all(), (g, float((eq / np.maximum(bq, 1e-300)).max()))
        out["q"] = max(out["q"], float((eq / np.maximum(bq, 1e-300)).max()))
        if hi - lo == 1:
            assert w[lo] == 0.0                                    # one candidate: nothing to prefer
    tail = int(group_off[G])
    assert (w[tail:] == 0).all() and (q[tail:] == 0).all()
    br = eps * float((rq * np.abs(c)).sum())
    out["risk"] = abs(float(risk) - rrisk) / max(br, 1e-300)
    assert abs(float(risk) - rrisk) <= br, (float(risk), rrisk, br)
    return out
