"""TEST INFRASTRUCTURE: float64 reference of the soft-target loss (lxo_ce_loss_soft).  Shared by tests/test_soft_loss_sim.py (hipsim),
tests/test_engine_soft_sim.py and tests/test_gpu_soft_loss.py (MI355X).  The logits, their padding, the weights and the float64 smoothed head come
from tests/smoothed_loss_ref.py and tests/weighted_loss_ref.py.

The definition (include/lxo.h).  soft_ids int32 / soft_p f32 [B, T, k], 1 <= k <= 16; the slots of row (b, t) are read only where t < lengths[b].
For a live row with clamped target y, log-sum-exp lse, soft-max p, U = lse - (sum_{j < V} x_j) / V, CE = lse - x_y, smoothing eps, mix lambda and
weight w = w_tok[b][t] * w_row[b] (a missing factor is 1):
    slot i counts iff 0 <= ids_i < V; m_i = p_i when it counts, else 0
    Sigma  = sum_i m_i, added in ascending i IN F32 (so the reference adds it that way too: it is part of the definition, not an error)
    rest   = max(0, 1 - Sigma), spread uniformly over [0, V)
    tau_j  = sum_{i: ids_i == j} m_i + rest / V
    lam_r  = 0 if Sigma == 0 (no teacher: the row is lxo_ce_loss_smoothed's) else lambda
    q_j    = (1 - lam_r) [(1 - eps) [j == y] + eps / V] + lam_r tau_j
    S      = (1 - lam_r) + lam_r (Sigma + rest)
    L      = (1 - lam_r) [(1 - eps) CE + eps U] + lam_r [sum_i m_i (lse - x_{ids_i}) + rest U]
    d(logits)_j = (S p_j - q_j) * w * inv_norm
ws region "loss" = {sum w L, live token count, sum w, sum CE (plain)}."""
import numpy as np

from smoothed_loss_ref import (POISONS, S_B, S_CASES, S_INV_NORM, S_T, S_VOCABS, logp_tol, make_case, make_weights, padded,  # noqa: F401
                               smoothed_reference, vpad)

F_VOCABS = S_VOCABS                         # 33, 500, 1000, 1025: ce_loss_rows_kernel<KV = 4, 8, 16> and the strided ce_loss_kernel
F_B, F_T = S_B, S_T                         # 48 rows
F_CASES = ("normal", "dominant", "target_out_of_range", "dead_rows")
F_K = (1, 5, 16)
F_LAMBDA = (0.5, 1.0)
F_EPS = (0.0, 0.1)
F_INV_NORM = S_INV_NORM
F_KINDS = ("topk", "dup", "holes", "hard", "edges", "one", "over")      # (a) .. (f) of the slot data; (f) is two
MASS_CAP = 1.0 + 1e-3                       # the Engine's cap on a position's counted masses


def _topk(x_row, k, rng):
    """the k best tokens of a perturbed copy of the row with their probabilities under it: what a teacher's lxo_score_alternatives returns"""
    z = x_row.astype(np.float64) + 0.5 * rng.standard_normal(x_row.shape[0])
    pz = np.exp(z - z.max())
    pz /= pz.sum()
    order = np.argsort(-z, kind="stable")[:k]
    return order.astype(np.int32), pz[order].astype(np.float32)


def _dyadic(k, over):
    """k f32 masses whose ascending f32 sum is exactly 1 (halves: every partial sum is exact), or exactly 1 + 2^-20"""
    m = np.array([2.0 ** -(i + 1) for i in range(k - 1)] + [2.0 ** -(k - 1)], np.float32)[::-1].copy()      # ascending: the small ones first
    if over:
        m[0] += np.float32(2.0 ** -20)      # k = 16: 2^-15 + 2^-20, exact in f32, and so is every partial sum
    return m


def make_slots(kind, x, f, ln, V, k, seed):
    """-> (soft_ids int32 [B, T, k], soft_p f32 [B, T, k]).  kind: one of F_KINDS for every live row, or "mix": live row number i takes
    F_KINDS[i % 7], so that taught rows, untaught rows and every edge meet in ONE call.  The slots of dead rows (t >= ln[b]) hold what must never
    be read: an id far outside the row and a NaN mass."""
    B, T = f.shape
    rng = np.random.default_rng([seed, V, k, F_KINDS.index(kind) if kind in F_KINDS else 99])
    ids = np.full((B, T, k), 123456789, np.int32)
    p = np.full((B, T, k), np.nan, np.float32)
    n_live = 0
    for t in range(T):
        for b in range(B):
            if t >= ln[b]:
                continue
            kd = F_KINDS[n_live % len(F_KINDS)] if kind == "mix" else kind
            n_live += 1
            i_, p_ = _topk(x[t * B + b], k, rng)
            if kd == "dup" and k > 1:
                i_[1] = i_[0]                                       # two slots name one token: their masses add up
            elif kd == "holes":
                if rng.random() < 0.5:
                    i_[:], p_[:] = -1, 0.25                         # a whole row of -1: no teacher (the masses there are not to be counted)
                else:
                    cut = int(rng.integers(0, k))                   # the tail from `cut` on; cut = 0 is a whole row again
                    i_[cut:] = -1
            elif kd == "hard":
                y = min(max(int(f[b, t]), 0), V - 1)
                i_[:], p_[:] = -1, 0.0
                i_[0], p_[0] = y, 1.0
            elif kd == "edges":
                i_[:], p_[:] = -1, 0.0
                if k == 1:
                    i_[0], p_[0] = (0, 0.375) if n_live % 2 else (V - 1, 0.375)
                else:
                    i_[0], p_[0], i_[k - 1], p_[k - 1] = 0, 0.375, V - 1, 0.25
            elif kd in ("one", "over"):
                i_ = rng.choice(V, size=k, replace=False).astype(np.int32)
                p_ = _dyadic(k, kd == "over")
            ids[b, t], p[b, t] = i_, p_
    return ids, p


def with_invalid_ids(ids, V, seed):
    """a copy in which some counting slots of live rows are replaced by ids outside [0, V) -- and the copy that says -1 there instead: the two
    must give the same bytes"""
    rng = np.random.default_rng([seed, V])
    bad = np.array([V, V + 7, 1 << 30, -2, -(1 << 30)], np.int32)
    hit = (rng.random(ids.shape) < 0.3) & (ids >= 0) & (ids < V)
    a, b = ids.copy(), ids.copy()
    a[hit] = bad[rng.integers(0, len(bad), size=int(hit.sum()))]
    b[hit] = -1
    return a, b


def counted_mass(ids, p, ln, V):
    """[B, T] float64: the sum of the counting masses of the live positions (0 elsewhere) -- what the Engine holds against MASS_CAP"""
    B, T, _ = ids.shape
    live = np.arange(T)[None, :] < np.asarray(ln)[:, None]
    cnt = (ids >= 0) & (ids < V) & live[:, :, None]
    return np.where(cnt, p.astype(np.float64), 0.0).sum(axis=2)


def soft_reference(logits, formula, lengths, w_tok, w_row, inv_norm, eps, lam, ids, p):
    """float64 reference on f32 inputs (eps, lam: the f32 values the kernel receives): smoothed_reference's dict plus, per logits row n = t * B + b,
    q_f [n, V], S [n], lam_r [n], sigma [n], mslot [n] (= sum_i m_i), L [B, T], dlogits_f [n, V] = (S p - q) * w_eff * inv_norm and
    stats_f = {sum w L, ntok, sum w, sum CE}."""
    ref = smoothed_reference(logits, formula, lengths, w_tok, w_row, inv_norm, eps)
    e, lm = ref["eps"], float(np.float32(lam))
    x = logits.astype(np.float64)
    n, V = x.shape
    B, T = formula.shape
    k = ids.shape[2]
    live, rows, w = ref["live"], ref["rows"], ref["w"]
    q = ref["q"].copy()                                            # the smoothed target; rows without a teacher keep it
    S, lam_r, sigma, mslot = np.ones(n), np.zeros(n), np.zeros(n), np.zeros(n)
    ce = -ref["logp"]                                              # [B, T]
    u_row = ref["lse"] - x.mean(axis=1)
    L = np.zeros((B, T), np.float64)
    for b in range(B):
        for t in range(T):
            if not live[b, t]:
                continue
            r = rows[b, t]
            l_s = (1.0 - e) * ce[b, t] + e * u_row[r]
            sg, tau, dot = np.float32(0.0), np.zeros(V), 0.0
            for i in range(k):
                j = int(ids[b, t, i])
                if 0 <= j < V:
                    m = p[b, t, i]
                    sg = np.float32(sg + m)                        # ascending i, in f32: the definition
                    tau[j] += float(m)
                    dot += float(m) * (ref["lse"][r] - x[r, j])
            sg = float(sg)
            rest = max(0.0, 1.0 - sg)
            sigma[r], mslot[r] = sg, tau.sum()
            if sg == 0.0:
                L[b, t] = l_s
                continue
            tau += rest / V
            lam_r[r] = lm
            q[r] = (1.0 - lm) * q[r] + lm * tau
            S[r] = (1.0 - lm) + lm * (sg + rest)
            L[b, t] = (1.0 - lm) * l_s + lm * (dot + rest * u_row[r])
    ref["k"], ref["lam"], ref["q_f"], ref["S"], ref["lam_r"], ref["sigma"], ref["mslot"], ref["L"] = k, lm, q, S, lam_r, sigma, mslot, L
    ref["dlogits_f"] = (S[:, None] * ref["p"] - q) * (ref["w_eff"] * float(np.float32(inv_norm)))[:, None]
    ref["stats_f"] = np.array([(w * L)[live].sum(), float(ref["ntok"]), w[live].sum(), ce[live].sum()], np.float64)
    return ref


def check_soft(ref, logits, V, Vp, loss, dl, inv_norm, bf16):
    """Assert lxo_ce_loss_soft's outputs (loss f32 [4], dl = d(logits) [n, Vp] widened to f32) -> dict of worst errors as fractions of their bars.

    ELEMENT BAR: smoothed_loss_ref.check_smoothed's with two changes.
      * the soft-max term: the device forms S * p_j, so what was (2 tol + 2^-21) p_j |w_eff| inv -- the log-sum-exp's error and an ulp or two of exp --
        is taken on S p_j, and the product adds one rounding of at most 2^-24 relative; 2^-23 S p_j stands for it;
      * the q term becomes (k + 4) * 2^-24 * q_j |w_eff| inv: up to k additions make tau_j (the first, into 0.f, is exact; the k-th is rest / V's), one
        rounding is the division rest / V, two are the smoothing's (eps / (float)V and (1.f - eps) + eps_v), one is the lambda mix.  Every addend of
        q_j is non-negative, so each rounding is relative to a partial result of at most q_j.  Sigma is NOT a source of error: the definition says it
        is the ascending f32 sum, and the reference adds it that way; 1 - Sigma is exact for Sigma in [1/2, 2] and otherwise one rounding relative to
        rest, which the count above leaves room for at k >= 1 (the first addition's).
      The 2^-22 |r| (the subtraction and the scale) and, in bf16, the 2^-8 |r| of the store stay.  The p and the q term stand beside |r|, not inside it.

    STATISTICS: [1] exact; [2] and [3] check_weighted's.  [0]: a row's L weighs the log-sum-exp-carrying terms CE, U and lse - x_{ids_i} with
    (1 - lam_r)(1 - eps), (1 - lam_r) eps + lam_r rest and lam_r m_i: (1 - lam_r) + lam_r rest <= 1 of them is check_smoothed's `tol`, the slots
    add lam_r sum_i m_i tol.  The logit sum enters through U alone, now with the weight c_U = (1 - lam_r) eps + lam_r rest where check_smoothed has
    eps: c_U 2^-19 mean_j |x_j| (that docstring counts the roundings; with eps == 0 and lambda == 1 the smoothed bar would have no such term while
    L holds rest * U).  The slot sum itself -- the products m_i (lse - x_i), their additions in ascending i, the product with rest and the lambda
    mix -- is roundings of partial results no larger than the terms of L: 2^-22 |L| per row.  Then sum_live |w| (...) + 2e-6 |ref| as there.

    STRUCTURE, exact: the padding columns 0, the dead rows 0; a live row's sum_j d(logits)_j within the sum of its element bars (S p and q both sum
    to S; the f32 Sigma inside S against the masses' exact sum inside q is k roundings of Sigma, inside the rows' q terms)."""
    tol = logp_tol(logits)
    live, ntok, w, e = ref["live"], ref["ntok"], ref["w"], ref["eps"]
    k = ref["k"]
    inv = float(np.float32(inv_norm))
    out = {}
    assert (dl[:, V:Vp] == 0).all()                                # the padding columns exactly 0
    live_rows = ref["rows"][live]
    dead = ~np.isin(np.arange(dl.shape[0]), live_rows)
    assert (dl[dead] == 0).all()                                   # rows past lengths[b] exactly 0
    g, r = dl[:, :V].astype(np.float64), ref["dlogits_f"]
    err = np.abs(g - r)
    scale = (np.abs(ref["w_eff"]) * inv)[:, None]
    sp = ref["S"][:, None] * ref["p"]
    bar = (2.0 * tol + 2.0 ** -21 + 2.0 ** -23) * sp * scale + 2.0 ** -22 * np.abs(r) + (k + 4) * 2.0 ** -24 * ref["q_f"] * scale
    if bf16:
        bar += 2.0 ** -8 * np.abs(r)
    out["dlogits"] = float((err / np.maximum(bar, 1e-300)).max())
    assert (err <= bar).all(), (np.argwhere(err > bar)[:4], float(err.max()))
    rs, rb = np.abs(g.sum(axis=1))[live_rows], bar.sum(axis=1)[live_rows]
    out["rowsum"] = float((rs / np.maximum(rb, 1e-300)).max()) if len(live_rows) else 0.0
    assert (rs <= rb).all(), (np.argwhere(rs > rb)[:4],)
    st = ref["stats_f"]
    assert float(loss[1]) == float(ntok), (loss[1], ntok)          # the token count: exact, whatever the weights
    wmax = max(1.0, float(np.abs(w[live]).max())) if live.any() else 1.0
    rows = ref["rows"]
    mean_abs = np.abs(logits.astype(np.float64)).mean(axis=1)[rows]                # [B, T]
    lam_r, rest = ref["lam_r"][rows], np.maximum(0.0, 1.0 - ref["sigma"][rows])
    c_u = (1.0 - lam_r) * e + lam_r * rest
    per_row = tol * (1.0 + lam_r * np.abs(ref["mslot"][rows])) + c_u * 2.0 ** -19 * mean_abs + 2.0 ** -22 * np.abs(ref["L"])
    b0 = float((np.abs(w) * per_row)[live].sum()) + 2e-6 * abs(st[0])
    e0 = abs(float(loss[0]) - st[0])
    out["loss0"] = e0 / max(b0, 1e-300)
    assert e0 <= b0, (float(loss[0]), st[0], e0, b0)
    e3, b3 = abs(float(loss[3]) - st[3]), tol * max(ntok, 1) * wmax + 2e-6 * abs(st[3])
    out["loss3"] = e3 / b3
    assert e3 <= b3, (float(loss[3]), st[3], e3, b3)
    e2, b2 = abs(float(loss[2]) - st[2]), 2.0 ** -22 * float(np.abs(w[live]).sum())
    out["loss2"] = e2 / max(b2, 1e-300)
    assert e2 <= b2, (float(loss[2]), st[2], e2, b2)
    return out


def soft_grads(P, img, f, l, w, norm, eps, lam, ids, p):
    """The engine-level reference, autograd through oracle/ref_model.py: loss = sum_{b,t} w[b, t] (-sum_j q[b, t, j] log_softmax_j) [t < l[b]] / norm
    with q the definition's target, built by soft_reference (it does not depend on the logits); w f32 [B, T] (ones: no weights)
    -> (loss, gradients, plain token-mean CE)"""
    import torch
    import torch.nn.functional as F
    import mrt_oracle
    from oracle import ref_model as R
    f = np.ascontiguousarray(f, np.int32)
    B, T = f.shape
    l = np.asarray(l, np.int32)
    ft = torch.from_numpy(f).long()
    mask = torch.from_numpy((np.arange(T)[None, :] < l[:, None]).astype(np.float32))
    wt = torch.from_numpy(np.asarray(w, np.float32))
    q = None

    def fn(Q):
        nonlocal q
        logits = R.decoder_train(Q, R.encoder(Q, torch.from_numpy(np.asarray(img)), True), ft)
        V = logits.shape[2]
        if q is None:
            ref = soft_reference(np.zeros((T * B, V), np.float32), f, l, None, None, 1.0, eps, lam, np.asarray(ids), np.asarray(p, np.float32))
            q = torch.from_numpy(ref["q_f"].reshape(T, B, V).transpose(1, 0, 2).copy())
        lsm = F.log_softmax(logits.double(), dim=2)
        L = -(q * lsm).sum(dim=2)
        ce = F.cross_entropy(logits.reshape(B * T, V), ft.reshape(-1), reduction="none").reshape(B, T)
        return (wt * L * mask).sum() / float(norm), float((ce * mask).sum().detach() / mask.sum())
    return mrt_oracle._grads(P, fn)
