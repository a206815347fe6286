"""TEST INFRASTRUCTURE: autograd references of the weighted training loss and of the minimum-risk objective through oracle/ref_model.py.
Shared by tests/test_engine_weighted_sim.py (hipsim) and tests/test_gpu_weighted_loss.py (MI355X)."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_model as R


def _token_ce(Q, img, f, positional=True):
    """CE [B, T] of every position (unmasked) through the oracle's encoder and teacher-forced decoder"""
    f = torch.from_numpy(np.asarray(f)).long()
    logits = R.decoder_train(Q, R.encoder(Q, torch.from_numpy(np.asarray(img)), positional), f)
    B, T, V = logits.shape
    return F.cross_entropy(logits.reshape(B * T, V), f.reshape(-1), reduction="none").reshape(B, T)


def _grads(P, fn):
    Q = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in P.items())
    val, aux = fn(Q)
    g = torch.autograd.grad(val, list(Q.values()), allow_unused=True)
    return float(val.detach()), OrderedDict((k, (x if x is not None else torch.zeros_like(P[k])).numpy()) for k, x in zip(Q.keys(), g)), aux


def weighted_grads(P, img, f, l, w, norm):
    """loss = sum_{b,t} w[b, t] CE[b, t] [t < l[b]] / norm and its gradients by autograd; w f32 [B, T] (the product of the token and the row weights)"""
    T = np.asarray(f).shape[1]
    mask = torch.from_numpy((np.arange(T)[None, :] < np.asarray(l)[:, None]).astype(np.float32))
    wt = torch.from_numpy(np.asarray(w, np.float32))

    def fn(Q):
        return (wt * _token_ce(Q, img, f) * mask).sum() / float(norm), None
    return _grads(P, fn)[:2]


def mrt_grads(P, img, cand, cand_lengths, group_sizes, cost, alpha):
    """THE TRUE RISK, not the surrogate: risk = (1 / G) sum_g sum_c softmax_c(alpha seq_logp)[c] cost[c], seq_logp = -sum_t CE over the
    candidate's live tokens, image g repeated for its candidates -> (risk, gradients, q [rows])"""
    gs = np.asarray(group_sizes)
    rep = np.repeat(np.arange(len(gs)), gs)
    T = np.asarray(cand).shape[1]
    mask = torch.from_numpy((np.arange(T)[None, :] < np.asarray(cand_lengths)[:, None]).astype(np.float32))
    c = torch.from_numpy(np.asarray(cost, np.float32))
    off = np.concatenate([[0], np.cumsum(gs)])

    def fn(Q):
        seq = -(_token_ce(Q, np.asarray(img)[rep], cand) * mask).sum(1)
        qs = [torch.softmax(float(alpha) * seq[off[g]:off[g + 1]], 0) for g in range(len(gs))]
        risk = sum((q * c[off[g]:off[g + 1]]).sum() for g, q in enumerate(qs)) / len(gs)
        return risk, torch.cat(qs).detach().numpy()
    return _grads(P, fn)


def cosines(got, ref):
    """[(cosine, name)] ascending"""
    def cos(a, b):
        a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
        return float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))
    return sorted((cos(got[k], ref[k]), k) for k in ref)
