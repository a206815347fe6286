"""TEST INFRASTRUCTURE: float64 reference of lxo_score_alternatives -- the k best tokens per position, the rank of the given token and the
entropy of the step -- over the constructed logits of tests/output_head_ref.py (make_case, imported).  Shared by
tests/test_alternatives_sim.py (hipsim) and tests/test_gpu_alternatives.py (MI355X).

Order: value descending on the f32 logits, then column ascending (np.argsort(-x, kind="stable")).  With an allowed set a banned column is
a column outside the vocabulary: log-sum-exp, selection, rank and entropy run over the allowed columns."""
import numpy as np

from output_head_ref import logp_tol


def reference(logits, formula, lengths, k, allowed=None):
    """logits f32 [T * B, V] (row t * B + b), allowed bool [B, V] or None -> dict of [B, T(, k)] arrays:
    ids (int, -1 beyond the allowed columns and on dead rows), logp f64 (-inf / 0 there), rank (int, -1: banned target or dead row),
    ent f64 (0 on dead rows), live bool, tgt (clamped)."""
    B, T = formula.shape
    n, V = logits.shape
    live = np.arange(T)[None, :] < lengths[:, None]
    tgt = np.clip(formula.astype(np.int64), 0, V - 1)
    ids = np.full((n, k), -1, np.int64)
    logp = np.zeros((n, k))
    rank = np.full(n, -1, np.int64)
    ent = np.zeros(n)
    tgt_row = tgt.T.reshape(-1)                                            # row order t * B + b
    for lo in range(0, n, 1024):                                           # in pieces: [rows, V] float64 temporaries
        r = np.arange(lo, min(lo + 1024, n))
        ok = np.ones((len(r), V), bool) if allowed is None else np.asarray(allowed, bool)[r % B]
        x32 = np.where(ok, logits[r], -np.inf)
        order = np.argsort(-x32, axis=1, kind="stable")                    # exact ties: the lower index first; banned columns last
        x = x32.astype(np.float64)
        m = x.max(axis=1, keepdims=True)
        lse = m + np.log(np.exp(x - m).sum(axis=1, keepdims=True))
        top = order[:, :k]
        have = np.arange(k)[None, :] < ok.sum(axis=1, keepdims=True)
        ids[r] = np.where(have, top, -1)
        logp[r] = np.where(have, np.take_along_axis(x, top, 1) - lse, -np.inf)
        pos = np.empty_like(order)
        np.put_along_axis(pos, order, np.broadcast_to(np.arange(V), order.shape), 1)
        t = tgt_row[r]
        rank[r] = np.where(ok[np.arange(len(r)), t], pos[np.arange(len(r)), t], -1)
        ent[r] = np.where(ok, np.exp(x - lse) * (lse - np.where(ok, x, 0.0)), 0.0).sum(axis=1)
    def bt(a):                                                             # [T * B, ...] -> [B, T, ...]
        return np.swapaxes(a.reshape((T, B) + a.shape[1:]), 0, 1)
    ids, logp, rank, ent = bt(ids).copy(), bt(logp).copy(), bt(rank).copy(), bt(ent).copy()
    ids[~live], logp[~live], rank[~live], ent[~live] = -1, 0.0, -1, 0.0
    return dict(ids=ids, logp=logp, rank=rank, ent=ent, live=live, tgt=tgt)


def check(ref, logits, ids, logp, rank, ent):
    """Assert outputs [B, T(, k)] against reference(): ids and rank exactly (comparisons of f32 values: nothing excluded), logp within
    logp_tol, the entropy within logp_tol * (2 + H) -- each factor lse - x carries the lse's absolute error, each p carries it as a
    relative error, one more share for the exp and the summation; dead rows -1 / 0 / -1 / 0.  -> (worst |logp - ref|, worst fraction of
    the entropy bound)."""
    tol = logp_tol(logits)
    live = ref["live"]
    assert np.array_equal(ids, ref["ids"]), np.argwhere(ids != ref["ids"])[:8]
    assert np.array_equal(rank, ref["rank"]), np.argwhere(rank != ref["rank"])[:8]
    assert (ids[~live] == -1).all() and (logp[~live] == 0).all() and (rank[~live] == -1).all() and (ent[~live] == 0).all()
    got, want = logp[live], ref["logp"][live]
    none = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), none)
    e_lp = float(np.abs(got[~none] - want[~none]).max()) if (~none).any() else 0.0
    assert e_lp <= tol, (e_lp, tol)
    frac = 0.0
    if live.any():
        h = ref["ent"][live]
        frac = float((np.abs(ent[live] - h) / (tol * (2.0 + h))).max())
        assert (ent[live] >= 0).all()
    assert frac <= 1.0, frac
    return e_lp, frac


def pack_bits(allowed):
    """bool [rows, V] -> uint32 words [rows, (V + 31) / 32] (bit v & 31 of word v >> 5)"""
    rows, V = allowed.shape
    words = (V + 31) // 32
    bits = np.zeros((rows, words * 32), bool)
    bits[:, :V] = allowed
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32))
