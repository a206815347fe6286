"""TEST INFRASTRUCTURE: float64 reference of the label-smoothed loss (lxo_ce_loss_smoothed).  Shared by tests/test_smoothed_loss_sim.py (hipsim)
and tests/test_gpu_smoothed_loss.py (MI355X).  The logits, their padding and the unweighted float64 head come from tests/output_head_ref.py, the
weights and the weighted float64 head from tests/weighted_loss_ref.py.

The definition (include/lxo.h; TensorFlow's softmax_cross_entropy(label_smoothing=), torch's F.cross_entropy(label_smoothing=)): for a live row
with clamped target y, smoothing eps and weight w = w_tok[b][t] * w_row[b] (a missing factor is 1)
    q_j = (1 - eps) [j == y] + eps / V,   CE = lse - x_y,   U = lse - mean_j x_j,   L = (1 - eps) CE + eps U,
    d(logits)_j = (p_j - q_j) * w * inv_norm,
ws region "loss" = {sum w L, live token count, sum w, sum CE (plain)}."""
import numpy as np

from output_head_ref import POISONS, logp_tol, make_case, padded, reference, vpad  # noqa: F401  (re-exported for the two test files)
from weighted_loss_ref import make_weights, weighted_reference  # noqa: F401

S_VOCABS = (33, 500, 1000, 1025)           # Vp = 64, 512, 1024, 1056: ce_loss_rows_kernel<KV = 4, 8, 16> and the strided ce_loss_kernel
S_B, S_T = 8, 6                            # 48 rows: twelve workgroups of four waves
S_CASES = ("normal", "large", "dominant", "target_out_of_range", "dead_rows")
S_MODES = ("none", "tok", "row", "both")
S_EPS = (0.1, 0.9)
S_INV_NORM = 1.0 / 7.0


def mode_weights(mode, w_tok, w_row):
    return {"none": (None, None), "tok": (w_tok, None), "row": (None, w_row), "both": (w_tok, w_row)}[mode]


def smoothed_reference(logits, formula, lengths, w_tok, w_row, inv_norm, eps):
    """float64 reference on f32 inputs (eps: the f32 value the kernel receives): the dict of weighted_loss_ref.weighted_reference plus
    q [n, V] (the smoothed targets; meaningless on dead rows), dlogits_s [n, V] = (p - q) * w_eff * inv_norm and stats_s = {sum w L, ntok, sum w,
    sum CE} over the live tokens"""
    ref = weighted_reference(logits, formula, lengths, w_tok, w_row, inv_norm)
    e = float(np.float32(eps))
    x = logits.astype(np.float64)
    n, V = x.shape
    live, rows, w = ref["live"], ref["rows"], ref["w"]
    tgt_row = np.zeros(n, np.int64)
    tgt_row[rows.reshape(-1)] = ref["tgt"].reshape(-1)
    q = np.full((n, V), e / V, np.float64)
    q[np.arange(n), tgt_row] += 1.0 - e
    p = np.exp(x - ref["lse"][:, None])
    ref["eps"], ref["q"], ref["p"] = e, q, p
    ref["dlogits_s"] = (p - q) * (ref["w_eff"] * float(np.float32(inv_norm)))[:, None]
    ce = -ref["logp"]                                              # [B, T], 0 on dead rows
    u = (ref["lse"] - x.mean(axis=1))[rows]                        # [B, T]
    L = (1.0 - e) * ce + e * u
    ref["stats_s"] = np.array([(w * L)[live].sum(), float(ref["ntok"]), w[live].sum(), ce[live].sum()], np.float64)
    return ref


def check_smoothed(ref, logits, V, Vp, loss, dl, inv_norm, bf16):
    """Assert lxo_ce_loss_smoothed's outputs (loss f32 [4], dl = d(logits) [n, Vp] widened to f32) -> dict of worst errors as fractions of their bars.

    ELEMENT BAR: check_weighted's, (2 tol + 2^-21) p |w_eff| inv + 2^-22 |r| -- the soft-max carries the log-sum-exp's error and an ulp or two of
    exp; the subtraction and the scale are roundings relative to the result r -- plus 2^-22 q_j |w_eff| inv for the two f32 roundings in q_j
    (eps / (float)V, and (1.f - eps) + eps_v on the target column); bf16: 2^-8 |r| for the store.  The p and the q term stand beside |r|, not inside
    it: where p_j ~ eps / V the result cancels and |r| alone would be a bar of nothing.

    STATISTICS: [1] exact; [2] and [3] check_weighted's; [0]: a row's L = (1 - eps) CE + eps (lse - sum_j x_j / V) carries the error of lse and CE
    (tol, their weights sum to 1) and the logit sum's: in the register-row kernels a lane adds its KV <= 16 columns into 0.f (the first addition
    is exact) and the wave adds 6 times -- at most 21 roundings; in the strided kernel a lane adds ceil(V / 64) columns, 17 at the V = 1025 of
    this matrix, and the wave 6 times -- 22 roundings.  22 * 2^-24 < 2^-19, each rounding relative to a partial sum of at most sum_j |x_j|, and
    the division by V makes it mean_j |x_j|.  So [0] is within sum_live |w| (tol + eps 2^-19 mean_j |x_j|) + 2e-6 |ref| (the last: the f32
    products and the ordered sums over rows, as in check_weighted).

    STRUCTURE, exact: the padding columns 0, the dead rows 0; a live row's sum_j d(logits)_j within the sum of its element bars (p and q both sum
    to 1)."""
    tol = logp_tol(logits)
    live, ntok, w, e = ref["live"], ref["ntok"], ref["w"], ref["eps"]
    inv = float(np.float32(inv_norm))
    out = {}
    assert (dl[:, V:Vp] == 0).all()                                # the padding columns exactly 0
    live_rows = ref["rows"][live]
    dead = ~np.isin(np.arange(dl.shape[0]), live_rows)
    assert (dl[dead] == 0).all()                                   # rows past lengths[b] exactly 0
    g, r = dl[:, :V].astype(np.float64), ref["dlogits_s"]
    err = np.abs(g - r)
    scale = (np.abs(ref["w_eff"]) * inv)[:, None]
    bar = (2.0 * tol + 2.0 ** -21) * ref["p"] * scale + 2.0 ** -22 * np.abs(r) + 2.0 ** -22 * ref["q"] * scale
    if bf16:
        bar += 2.0 ** -8 * np.abs(r)
    out["dlogits"] = float((err / np.maximum(bar, 1e-300)).max())
    assert (err <= bar).all(), (np.argwhere(err > bar)[:4], float(err.max()))
    rs, rb = np.abs(g.sum(axis=1))[live_rows], bar.sum(axis=1)[live_rows]
    out["rowsum"] = float((rs / np.maximum(rb, 1e-300)).max()) if len(live_rows) else 0.0
    assert (rs <= rb).all(), (np.argwhere(rs > rb)[:4],)
    st = ref["stats_s"]
    assert float(loss[1]) == float(ntok), (loss[1], ntok)          # the token count: exact, whatever the weights
    wmax = max(1.0, float(np.abs(w[live]).max())) if live.any() else 1.0
    mean_abs = np.abs(logits.astype(np.float64)).mean(axis=1)[ref["rows"]]       # [B, T]
    b0 = float((np.abs(w) * (tol + e * 2.0 ** -19 * mean_abs))[live].sum()) + 2e-6 * abs(st[0])
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


def smoothed_grads(P, img, f, l, w, norm, eps):
    """The engine-level reference, autograd through oracle/ref_model.py: loss = sum_{b,t} w[b, t] L[b, t] [t < l[b]] / norm with L torch's
    F.cross_entropy(..., label_smoothing=eps, reduction="none"); w f32 [B, T] (ones: smoothing alone) -> (loss, gradients, plain token-mean CE)"""
    import torch
    import torch.nn.functional as F
    import mrt_oracle
    from oracle import ref_model as R
    ft = torch.from_numpy(np.asarray(f)).long()
    T = ft.shape[1]
    mask = torch.from_numpy((np.arange(T)[None, :] < np.asarray(l)[:, None]).astype(np.float32))
    wt = torch.from_numpy(np.asarray(w, np.float32))

    def fn(Q):
        logits = R.decoder_train(Q, R.encoder(Q, torch.from_numpy(np.asarray(img)), True), ft)
        B, _, V = logits.shape
        L = F.cross_entropy(logits.reshape(B * T, V), ft.reshape(-1), label_smoothing=float(eps), reduction="none").reshape(B, T)
        ce = F.cross_entropy(logits.reshape(B * T, V), ft.reshape(-1), reduction="none").reshape(B, T)
        return (wt * L * mask).sum() / float(norm), float((ce * mask).sum().detach() / mask.sum())
    return mrt_oracle._grads(P, fn)
