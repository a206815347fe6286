"""TEST REFERENCE: greedy and beam decode under per-image allowed-token sets, restated from the oracle's own pieces (attention_prepare,
cell_step, _top_k_lowest_index, add_div_penalty) the way tests/prefix_ref.py is, and following it line for line except for the one rule:
a banned vocabulary column is a column outside the vocabulary -- its logit is -inf BEFORE anything else happens in the select step.  So the
arg-max and the log_softmax run over the allowed columns, a banned beam candidate scores -inf (also for a finished hypothesis), and the
diversity penalty ranks banned columns last.  Masks are applied with `where` (the reference's (1 - f) x + f y turns -inf into NaN).
With every token allowed both functions equal prefix_ref's bit for bit.  They start from encoder features `enc` [B, R, C]."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_model as R
import prefix_ref

NEG = -float("inf")


def _allow(allow, B, V):
    """bool [V] or [B, V] -> torch bool [B, V]"""
    return torch.from_numpy(np.broadcast_to(np.asarray(allow, bool), (B, V)).copy())


def _no_prefix(prefix, lengths, B):
    if prefix is None:
        return np.zeros((B, 1), np.int64), np.zeros(B, np.int64)
    return prefix_ref._prefix(prefix, lengths, B)


def greedy_constrained(P, enc, id_end, allow, max_iter, prefix=None, lengths=None):
    """-> (ids int32 [B, T'], logp float64 [B, T'], logits f32 [B, T', V] with banned columns at -inf): logp[b, t] =
    log_softmax(masked logits_t)[ids[b, t]], the model's distribution renormalised over the allowed set (the forced id inside a prefix)."""
    enc = torch.as_tensor(enc)
    img, att_img, state = R.attention_prepare(P, enc)
    B = img.shape[0]
    V = P["Decoder/embedding_table"].shape[0]
    al = _allow(allow, B, V)
    pf, ln = _no_prefix(prefix, lengths, B)
    tab = P["Decoder/embedding_table"]
    emb = P["Decoder/start_token"].reshape(1, -1).expand(B, -1)
    finished = torch.zeros(B, dtype=torch.bool)
    ids_all, lp_all, lg_all = [], [], []
    time = 0
    while not bool(finished.all()):
        logits, state = R.cell_step(P, img, att_img, emb, state)
        logits = torch.where(al, logits, torch.tensor(NEG))
        ids = torch.argmax(logits, dim=-1)
        forced = torch.from_numpy(time < ln)
        if bool(forced.any()):
            col = torch.from_numpy(pf[:, min(time, pf.shape[1] - 1)])
            ids = torch.where(forced, col, ids)
        lp_all.append(F.log_softmax(logits.double(), dim=-1).gather(1, ids[:, None])[:, 0])
        lg_all.append(logits.clone())
        emb = tab[ids]
        finished = finished | ((ids == id_end) & ~forced)
        ids_all.append(ids.to(torch.int32))
        if time >= max_iter:
            finished = torch.ones_like(finished)
        time += 1
    return torch.stack(ids_all, dim=1).numpy(), torch.stack(lp_all, dim=1).numpy(), torch.stack(lg_all, dim=1).numpy()


def beam_constrained(P, enc, id_end, beam_size, allow, max_iter, div_gamma=1.0, div_prob=0.0, div_seed=0, prefix=None, lengths=None):
    """-> (ids int32 [B, T', k], parents int32 [B, T', k], scores f32 [B, T', k]) -- scores = the running log-probs after each step."""
    enc = torch.as_tensor(enc)
    img, att_img, (c, h, o) = R.attention_prepare(P, enc)
    B, k = img.shape[0], beam_size
    V = P["Decoder/embedding_table"].shape[0]
    al = _allow(allow, B, V)[:, None, :]
    pf, ln = _no_prefix(prefix, lengths, B)
    tab = P["Decoder/embedding_table"]
    tile = lambda t: t[:, None].expand(B, k, *t.shape[1:]).reshape(B * k, *t.shape[1:])
    img_t, att_t = tile(img), tile(att_img)
    state = (tile(c), tile(h), tile(o))
    emb = P["Decoder/start_token"].reshape(1, -1).expand(B * k, -1)
    log_probs = torch.zeros(B, k)
    finished = torch.zeros(B, k, dtype=torch.bool)
    fmin = torch.finfo(torch.float32).min
    ids_all, par_all, sc_all = [], [], []
    time = 0
    while not bool(finished.all()):
        logits, new_state = R.cell_step(P, img_t, att_t, emb, state)
        logits = torch.where(al, logits.reshape(B, k, V), torch.tensor(NEG))
        step_lp = F.log_softmax(logits, dim=-1)
        one_hot = torch.full((V,), fmin); one_hot[id_end] = 0.0
        step_lp = torch.where(finished[:, :, None], one_hot.expand(B, k, V), step_lp)
        step_lp = torch.where(al, step_lp, torch.tensor(NEG))                 # banned also for a finished hypothesis
        lp = log_probs[:, :, None] + step_lp
        lp_pen = R.add_div_penalty(lp, div_gamma, div_prob, div_seed, time)
        assert not torch.isnan(lp_pen).any()
        new_probs = torch.empty(B, k); new_ids = torch.empty(B, k, dtype=torch.int64); parents = torch.empty(B, k, dtype=torch.int64)
        for b in range(B):
            if time < ln[b]:                                                  # forced: every slot takes the prefix token, parent = itself
                f = int(pf[b, time])
                new_ids[b] = f
                parents[b] = torch.arange(k)
                new_probs[b] = lp[b, :, f]
                continue
            flat = lp_pen[b].reshape(1, k * V) if time > ln[b] else lp_pen[b, 0][None]
            v, idx = R._top_k_lowest_index(flat, k)
            new_probs[b], new_ids[b], parents[b] = v[0], idx[0] % V, idx[0] // V
        forced = torch.from_numpy(time < ln)[:, None]
        emb = tab[new_ids.reshape(-1)]
        gat = lambda t: t.reshape(B, k, -1).gather(1, parents[:, :, None].expand(B, k, t.shape[-1])).reshape(B * k, -1)
        finished = finished.gather(1, parents) | ((new_ids == id_end) & ~forced)
        state = tuple(gat(s) for s in new_state)
        log_probs = new_probs
        ids_all.append(new_ids.to(torch.int32))
        par_all.append(parents.to(torch.int32))
        sc_all.append(new_probs.clone())
        if time >= max_iter:
            finished = torch.ones_like(finished)
        time += 1
    return (torch.stack(ids_all, dim=1).numpy(), torch.stack(par_all, dim=1).numpy(), torch.stack(sc_all, dim=1).numpy())


def pack_bits(allow, ld=None):
    """bool [V] or [n, V] -> the C ABI's bit sets, uint32 [n, ld]: bit v & 31 of word v >> 5 (ld defaults to (V + 31) / 32)"""
    al = np.atleast_2d(np.asarray(allow, bool))
    words = (al.shape[1] + 31) // 32
    ld = words if ld is None else ld
    out = np.zeros((al.shape[0], ld), np.uint32)
    for v in range(al.shape[1]):
        out[:, v >> 5] |= al[:, v].astype(np.uint32) << np.uint32(v & 31)
    return out
