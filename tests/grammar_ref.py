"""TEST REFERENCE: greedy, beam and sampled decode under a delimiter grammar, built on the oracle's step functions the way
tests/constraint_ref.py and tests/sample_ref.py build theirs and following them line for line, except that the allowed set is no longer constant:
at step t decoder row r selects over S_t = A & Grammar.allowed_at(state_r, t, max_iter) (a finished row: A, its state frozen), and after the
select an unfinished row's state becomes Grammar.apply(state, id); a beam slot continues the state of its parent.  The Grammar is the host
model in latex_ocr_amd/grammar.py -- the tests in tests/test_grammar_host.py prove its guarantee by enumeration.
All three start from encoder features `enc` [B, R, C] and return the depths after each step beside what their models return."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_model as R
import constraint_ref
import sample_ref

NEG = -float("inf")


def _static(allow, B, V):
    return np.broadcast_to(np.ones(V, bool) if allow is None else np.asarray(allow, bool), (B, V))


def step_set(gram, A_row, state, finished, t, max_iter, id_end):
    """S_t of one decoder row"""
    return A_row.copy() if finished else (A_row & gram.allowed_at(state, t, max_iter, id_end))


def greedy_grammar(P, enc, id_end, gram, max_iter, allow=None, prefix=None, lengths=None):
    """-> (ids int32 [B, T'], logp float64 [B, T'], depth int32 [B, T'], logits f32 [B, T', V] masked with the step's sets)"""
    enc = torch.as_tensor(enc)
    img, att_img, state = R.attention_prepare(P, enc)
    B = img.shape[0]
    V = P["Decoder/embedding_table"].shape[0]
    A = _static(allow, B, V)
    pf, ln = constraint_ref._no_prefix(prefix, lengths, B)
    tab = P["Decoder/embedding_table"]
    emb = P["Decoder/start_token"].reshape(1, -1).expand(B, -1)
    finished = torch.zeros(B, dtype=torch.bool)
    stacks = [() for _ in range(B)]
    ids_all, lp_all, lg_all, dp_all = [], [], [], []
    time = 0
    while not bool(finished.all()):
        logits, state = R.cell_step(P, img, att_img, emb, state)
        al = torch.from_numpy(np.stack([step_set(gram, A[b], stacks[b], bool(finished[b]), time, max_iter, id_end) for b in range(B)]))
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
        for b in range(B):
            if not bool(finished[b]):
                stacks[b] = gram.apply(stacks[b], int(ids[b]))
        dp_all.append(np.array([len(s) for s in stacks], np.int32))
        ids_all.append(ids.to(torch.int32))
        if time >= max_iter:
            finished = torch.ones_like(finished)
        time += 1
    return (torch.stack(ids_all, dim=1).numpy(), torch.stack(lp_all, dim=1).numpy(), np.stack(dp_all, 1), torch.stack(lg_all, dim=1).numpy())


def beam_grammar(P, enc, id_end, beam_size, gram, max_iter, allow=None, prefix=None, lengths=None):
    """-> (ids, parents int32 [B, T', k], scores f32 [B, T', k], depth int32 [B, T', k]); no diversity penalty"""
    enc = torch.as_tensor(enc)
    img, att_img, (c, h, o) = R.attention_prepare(P, enc)
    B, k = img.shape[0], beam_size
    V = P["Decoder/embedding_table"].shape[0]
    A = _static(allow, B, V)
    pf, ln = constraint_ref._no_prefix(prefix, lengths, B)
    tab = P["Decoder/embedding_table"]
    tile = lambda t: t[:, None].expand(B, k, *t.shape[1:]).reshape(B * k, *t.shape[1:])
    img_t, att_t = tile(img), tile(att_img)
    state = (tile(c), tile(h), tile(o))
    emb = P["Decoder/start_token"].reshape(1, -1).expand(B * k, -1)
    log_probs = torch.zeros(B, k)
    finished = torch.zeros(B, k, dtype=torch.bool)
    stacks = [[() for _ in range(k)] for _ in range(B)]
    fmin = torch.finfo(torch.float32).min
    ids_all, par_all, sc_all, dp_all = [], [], [], []
    time = 0
    while not bool(finished.all()):
        logits, new_state = R.cell_step(P, img_t, att_t, emb, state)
        al = torch.from_numpy(np.stack([np.stack([step_set(gram, A[b], stacks[b][j], bool(finished[b, j]), time, max_iter, id_end)
                                                  for j in range(k)]) for b in range(B)]))
        logits = torch.where(al, logits.reshape(B, k, V), torch.tensor(NEG))
        step_lp = F.log_softmax(logits, dim=-1)
        one_hot = torch.full((V,), fmin); one_hot[id_end] = 0.0
        step_lp = torch.where(finished[:, :, None], one_hot.expand(B, k, V), step_lp)
        step_lp = torch.where(al, step_lp, torch.tensor(NEG))
        lp = log_probs[:, :, None] + step_lp
        new_probs = torch.empty(B, k); new_ids = torch.empty(B, k, dtype=torch.int64); parents = torch.empty(B, k, dtype=torch.int64)
        for b in range(B):
            if time < ln[b]:
                f = int(pf[b, time])
                new_ids[b] = f
                parents[b] = torch.arange(k)
                new_probs[b] = lp[b, :, f]
                continue
            flat = lp[b].reshape(1, k * V) if time > ln[b] else lp[b, 0][None]
            v, idx = R._top_k_lowest_index(flat, k)
            new_probs[b], new_ids[b], parents[b] = v[0], idx[0] % V, idx[0] // V
        forced = torch.from_numpy(time < ln)[:, None]
        emb = tab[new_ids.reshape(-1)]
        gat = lambda t: t.reshape(B, k, -1).gather(1, parents[:, :, None].expand(B, k, t.shape[-1])).reshape(B * k, -1)
        finished = finished.gather(1, parents) | ((new_ids == id_end) & ~forced)
        new_stacks = [[stacks[b][int(parents[b, j])] for j in range(k)] for b in range(B)]
        for b in range(B):
            for j in range(k):
                if not bool(finished[b, j]):
                    new_stacks[b][j] = gram.apply(new_stacks[b][j], int(new_ids[b, j]))
        stacks = new_stacks
        state = tuple(gat(s) for s in new_state)
        log_probs = new_probs
        ids_all.append(new_ids.to(torch.int32))
        par_all.append(parents.to(torch.int32))
        sc_all.append(new_probs.clone())
        dp_all.append(np.array([[len(s) for s in row] for row in stacks], np.int32))
        if time >= max_iter:
            finished = torch.ones_like(finished)
        time += 1
    return (torch.stack(ids_all, dim=1).numpy(), torch.stack(par_all, dim=1).numpy(), torch.stack(sc_all, dim=1).numpy(), np.stack(dp_all, 1))


def sample_grammar(P, enc, id_end, n, gram, max_iter, tau=1.0, top_k=0, top_p=1.0, seed=0, allow=None, prefix=None, lengths=None):
    """-> (ids int32 [B, T', n], logp, logq float64 [B, T', n], depth int32 [B, T', n], picks[t][b][j], logits f32 [T', B, n, V])"""
    enc = torch.as_tensor(enc)
    img, att_img, (c, h, o) = R.attention_prepare(P, enc)
    B = img.shape[0]
    V = P["Decoder/embedding_table"].shape[0]
    A = _static(allow, B, V)
    pf, ln = constraint_ref._no_prefix(prefix, lengths, B)
    tab = P["Decoder/embedding_table"]
    tile = lambda t: t[:, None].expand(B, n, *t.shape[1:]).reshape(B * n, *t.shape[1:])
    img_t, att_t = tile(img), tile(att_img)
    state = (tile(c), tile(h), tile(o))
    emb = P["Decoder/start_token"].reshape(1, -1).expand(B * n, -1)
    finished = np.zeros((B, n), bool)
    stacks = [[() for _ in range(n)] for _ in range(B)]
    ids_all, lp_all, lq_all, dp_all, picks, lg_all = [], [], [], [], [], []
    time = 0
    while not finished.all():
        logits, state = R.cell_step(P, img_t, att_t, emb, state)
        lg = logits.detach().numpy().reshape(B, n, V)
        step = [[sample_ref.select(lg[b, j], sample_ref.gumbel(seed, b, j, time, V), tau, top_k, top_p,
                                   step_set(gram, A[b], stacks[b][j], bool(finished[b, j]), time, max_iter, id_end),
                                   int(pf[b, time]) if time < ln[b] else -1)
                 for j in range(n)] for b in range(B)]
        ids = np.array([[q.id for q in row] for row in step], np.int64)
        forced = (time < ln)[:, None]
        finished = finished | ((ids == id_end) & ~forced)
        for b in range(B):
            for j in range(n):
                if not finished[b, j]:
                    stacks[b][j] = gram.apply(stacks[b][j], int(ids[b, j]))
        emb = tab[torch.from_numpy(ids.reshape(-1))]
        ids_all.append(ids.astype(np.int32))
        lp_all.append(np.array([[q.logp for q in row] for row in step]))
        lq_all.append(np.array([[q.logq for q in row] for row in step]))
        dp_all.append(np.array([[len(s) for s in row] for row in stacks], np.int32))
        picks.append(step); lg_all.append(lg.copy())
        if time >= max_iter:
            finished[:] = True
        time += 1
    return np.stack(ids_all, 1), np.stack(lp_all, 1), np.stack(lq_all, 1), np.stack(dp_all, 1), picks, np.stack(lg_all, 0)


def backtrace(ids, parents):
    """[T, k] ids and parents of one image -> the k hypotheses [k][T] that end in slot j of the last step"""
    T, k = ids.shape
    out = []
    for j in range(k):
        seq, slot = [], j
        for t in range(T - 1, -1, -1):
            seq.append(int(ids[t, slot]))
            slot = int(parents[t, slot])
        out.append(seq[::-1])
    return out
