"""TEST REFERENCE: forced-prefix greedy and beam decode restated from the oracle's own pieces (attention_prepare, cell_step,
_top_k_lowest_index, add_div_penalty).  Both follow oracle.greedy_decode / oracle.beam_decode line for line except at the forced steps:
at a step t < P_b row (image) b emits prefix[b, t] and stays unfinished; a beam's slots all take it with parent j and no diversity penalty,
and its top-k at step P_b is over slot 0 alone (what step 0 does without a prefix).  They start from encoder features `enc` [B, R, C]
(oracle.encoder's output, or the features a simulated decoder read) so that the decode alone is compared."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_model as R


def _prefix(prefix, lengths, B):
    pf = np.asarray(prefix, np.int64).reshape(B, -1)
    ln = np.asarray(lengths, np.int64).reshape(B)
    return pf, ln


def greedy_prefix(P, enc, id_end, prefix, lengths, max_iter):
    """-> (ids int32 [B, T'], logp float64 [B, T']): logp[b, t] = log_softmax(logits_t)[ids[b, t]] (the forced id inside the prefix)."""
    enc = torch.as_tensor(enc)
    img, att_img, state = R.attention_prepare(P, enc)
    B = img.shape[0]
    pf, ln = _prefix(prefix, lengths, B)
    tab = P["Decoder/embedding_table"]
    emb = P["Decoder/start_token"].reshape(1, -1).expand(B, -1)
    finished = torch.zeros(B, dtype=torch.bool)
    ids_all, lp_all = [], []
    time = 0
    while not bool(finished.all()):
        logits, state = R.cell_step(P, img, att_img, emb, state)
        ids = torch.argmax(logits, dim=-1)
        forced = torch.from_numpy(time < ln)
        if bool(forced.any()):
            col = torch.from_numpy(pf[:, min(time, pf.shape[1] - 1)])
            ids = torch.where(forced, col, ids)
        lp_all.append(F.log_softmax(logits.double(), dim=-1).gather(1, ids[:, None])[:, 0])
        emb = tab[ids]
        finished = finished | ((ids == id_end) & ~forced)
        ids_all.append(ids.to(torch.int32))
        if time >= max_iter:
            finished = torch.ones_like(finished)
        time += 1
    return torch.stack(ids_all, dim=1).numpy(), torch.stack(lp_all, dim=1).numpy()


def beam_prefix(P, enc, id_end, beam_size, prefix, lengths, max_iter, div_gamma=1.0, div_prob=0.0, div_seed=0):
    """-> (ids int32 [B, T', k], parents int32 [B, T', k], scores f32 [B, T', k]) -- scores = the running log-probs after each step."""
    enc = torch.as_tensor(enc)
    img, att_img, (c, h, o) = R.attention_prepare(P, enc)
    B, k = img.shape[0], beam_size
    pf, ln = _prefix(prefix, lengths, B)
    V = P["Decoder/embedding_table"].shape[0]
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
        step_lp = F.log_softmax(logits.reshape(B, k, V), dim=-1)
        one_hot = torch.full((V,), fmin); one_hot[id_end] = 0.0
        fin = finished.to(torch.float32)[:, :, None]
        step_lp = (1.0 - fin) * step_lp + fin * one_hot
        lp = log_probs[:, :, None] + step_lp
        lp_pen = R.add_div_penalty(lp, div_gamma, div_prob, div_seed, time)
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
