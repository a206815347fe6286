"""TEST INFRASTRUCTURE: the host reference of lxo_consensus -- the project's own levenshtein and truncate_end (model/evaluation/text.py) for the
pairwise distances, the risk of include/lxo.h's definition in float64 -- with the case matrix and the checks that tests/test_consensus_sim.py
(hipsim) and tests/test_gpu_consensus.py (MI355X) share.  The distances and the arg-min are compared exactly; the risk bit for bit where the
definition makes it exact (no weights, no normalisation) and otherwise against float64 within bound(n).  The expected values are computed once
per process."""
import ctypes
import functools

import numpy as np

from latex_ocr_amd import _abi
from latex_ocr_amd.model.evaluation.text import levenshtein, truncate_end
from edit_distance_ref import Host  # noqa: F401  (the numpy side of the Host / device indirection, re-exported)

LIMIT, MAX_N = _abi.LXO_EDIT_MAX_REF, _abi.LXO_CONSENSUS_MAX_N
END = 2                                                            # where a case cuts; the others pass id_end = -1 and END is a token like 0 and 1
# T either side of the strip-width switch points of cons_pairs_kernel<CPL> (64 | 128 | 256 | 512 | 1024), the decode bound, the limit
SHORT_T = [0, 1, 63, 64, 65]
LONG_T = [128, 129, 152, 256, 257, 512, 513, LIMIT]                 # at n <= 3


def bound(n):
    """the relative distance of an f32 risk from its float64 value, derived: every term is non-negative, so nothing cancels; a term carries one rounded
    division and one rounded product, each of the two sums n rounded additions, then the final division: below 2 (n + 2) units of 2^-24"""
    return 2.0 * (n + 2) * 2.0 ** -24


def clean_weights(w, B, n):
    """the weights as the device reads them, float64 [B, n]: negative or not finite -> 0, a row that sums to 0 -> ones; None -> ones"""
    if w is None:
        return np.ones((B, n))
    w = np.asarray(w, np.float32).astype(np.float64).copy()
    w[~(np.isfinite(w) & (w > 0))] = 0.0
    w[w.sum(axis=1) == 0] = 1.0
    return w


def distances(seqs):
    """seqs [B][n] token lists -> int32 [B, n, n]"""
    B, n = len(seqs), len(seqs[0])
    dist = np.zeros((B, n, n), np.int32)
    for g in range(B):
        for i in range(n):
            for j in range(i + 1, n):
                dist[g, i, j] = dist[g, j, i] = 0 if seqs[g][i] == seqs[g][j] else levenshtein(seqs[g][i], seqs[g][j])
    return dist


def reference_risk(seqs, dist, weights, normalize):
    """the definition in float64 -> [B, n]"""
    lens = np.array([[max(len(s), 1) for s in row] for row in seqs], np.float64)
    w = clean_weights(weights, dist.shape[0], dist.shape[1])
    cost = dist / lens[:, None, :] if normalize else dist.astype(np.float64)
    return (cost * w[:, None, :]).sum(axis=2) / w.sum(axis=1)[:, None]


def _sequences(flat, strides, B, n, T, id_end):
    out = []
    for g in range(B):
        row = []
        for i in range(n):
            s = [int(flat[g * strides[0] + i * strides[1] + t * strides[2]]) for t in range(T)]
            row.append(list(truncate_end(s, id_end)) if id_end >= 0 else s)
        out.append(row)
    return out


def make_case(name, ids, T, id_end, layout="BTn", weights=None, normalize=1):
    """ids [B, T + noise, n] (layout "BTn": what a sampled decode writes, the steps behind T are noise nothing may read) or [B, n, T] ("BnT")"""
    ids = np.ascontiguousarray(ids, np.int32)
    if layout == "BTn":
        B, Tall, n = ids.shape
        strides = (Tall * n, 1, n)
    else:
        B, n, Tall = ids.shape
        assert Tall == T
        strides = (n * T, T, 1)
    flat = ids.reshape(-1)
    seqs = _sequences(flat, strides, B, n, T, id_end)
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    dist = distances(seqs)
    risk = reference_risk(seqs, dist, w, normalize)
    return dict(name=name, ids=flat if flat.size else np.zeros(1, np.int32), strides=strides, B=B, n=n, T=T, id_end=id_end, weights=w, normalize=normalize, seqs=seqs,
                dist=dist, risk=risk)


def with_options(c, weights=None, normalize=None):
    """case c under other weights / the other normalisation (the distances are shared, the risk recomputed)"""
    normalize = c["normalize"] if normalize is None else normalize
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    return dict(c, weights=w, normalize=normalize, risk=reference_risk(c["seqs"], c["dist"], w, normalize))


def _random_ids(rng, B, T, n, cut):
    """[B, T + 2, n]: without a cut the three symbols at random (every draw T tokens); with one, draws of 0 / 1 whose END lies at a random place in
    the upper half of T (the last draw of an image has none), anything behind it"""
    ids = rng.integers(0, 3, size=(B, T + 2, n))
    if cut:
        ids[:, :T] = rng.integers(0, 2, size=(B, T, n))
        for g in range(B):
            for i in range(n - 1):
                L = int(rng.integers(T // 2, T + 1))
                if L < T:
                    ids[g, L, i] = END
    return ids


@functools.lru_cache(maxsize=None)
def matrix_cases():
    """n x T x B, both normalisations, with and without a cut; the layouts"""
    rng = np.random.default_rng(23)
    out = []

    def add(B, T, n, cut, normalize, layout="BTn"):
        ids = _random_ids(rng, B, T, n, cut)
        if layout == "BnT":
            ids = ids[:, :T].transpose(0, 2, 1)
        out.append(make_case("B%d T%d n%d %s norm%d %s" % (B, T, n, "cut" if cut else "whole", normalize, layout), ids, T, END if cut else -1, layout,
                             normalize=normalize))

    k = 0
    for T in SHORT_T:
        for n, B in ((1, 5), (2, 5), (3, 1), (5, 5)):
            add(B, T, n, k % 2, (k // 2) % 2)
            k += 1
    add(5, 20, 16, 1, 1)
    add(1, 20, 16, 0, 0)
    add(1, 9, MAX_N, 0, 1)
    add(1, 9, MAX_N, 1, 0)
    for T in LONG_T:
        add(5 if T in (128, 152) else 1, T, 3 if T < LIMIT else 2, k % 2, (k // 2) % 2)
        k += 1
    add(1, LIMIT, 3, 1, 1)
    add(5, 70, 3, 1, 1, "BnT")
    add(1, 40, 5, 0, 0, "BnT")
    return out


def _rows(draws, T, n_noise=2, seed=1):
    """draws [B][n] token lists (END where they mean it) -> ids [B, T + n_noise, n], noise of 0 .. 2 behind every list"""
    rng = np.random.default_rng(seed)
    B, n = len(draws), len(draws[0])
    ids = rng.integers(0, 3, size=(B, T + n_noise, n))
    for g in range(B):
        for i, d in enumerate(draws[g]):
            ids[g, :len(d), i] = d
    return ids


@functools.lru_cache(maxsize=None)
def end_cases():
    """where END lies.  T = 8, END = 2 among draws of 0 / 1."""
    E, T = END, 8
    x = [0, 1, 1, 0, 1, 0, 0, 1]
    y = [1, 1, 0, 0, 0, 1, 0, 1]
    out = []
    # a draw that is END at once, one without END, one whose END lies behind T (in the steps that were not run), one cut inside
    ids = _rows([[[E] + x[:5], x, y, x[:3] + [E] + y[:3]]], T)
    ids[0, T, 2] = E
    out.append(make_case("END at 0, absent, behind T, inside", ids, T, E))
    out.append(make_case("all draws empty", _rows([[[E, 0, 1], [E], [E, 1]], [[E], [E, E], [E, 0]]], T), T, E))
    out.append(make_case("all draws equal", _rows([[x[:5] + [E]] * 4, [y] * 4], T, seed=2), T, E))
    # draws 1 and 2 are equal and tie for the minimum (draw 0 pays twice their distance): the lower index wins
    out.append(make_case("two equal draws tie", _rows([[x, y[:6] + [E], y[:6] + [E, 1]], [y, x[:4] + [E, 0], x[:4] + [E, 1]]], T), T, E))
    out.append(make_case("id_end = -1", _rows([[[E] + x[:5], x, y, x[:3] + [E] + y[:3]]], T), T, -1))
    return out


@functools.lru_cache(maxsize=None)
def weight_cases():
    """one set of draws (B = 3, n = 5, T = 20; draw 3 repeats draw 1) under every kind of weights, both normalisations"""
    rng = np.random.default_rng(31)
    B, T, n = 3, 20, 5
    ids = _random_ids(rng, B, T, n, True)
    ids[:, :, 3] = ids[:, :, 1]
    base = make_case("weights: none", ids, T, END)
    pos = rng.uniform(0.1, 3.0, size=(B, n)).astype(np.float32)
    zeros = pos.copy()
    zeros[0, 0] = zeros[1, 4] = zeros[2, 1] = zeros[2, 2] = 0.0
    onehot = np.zeros((B, n), np.float32)
    onehot[0, 3] = onehot[1, 0] = onehot[2, 1] = 1.0                # image 0: the weight sits on the copy, best is the first of the two
    zrow = pos.copy()
    zrow[1] = 0.0
    bad = pos.copy()
    bad[0, 2], bad[1, 1], bad[2, 0], bad[2, 4] = -1.5, np.nan, np.inf, -np.inf
    out = []
    for nm in (1, 0):
        for name, w in (("none", None), ("positive", pos), ("with zeros", zeros), ("one-hot", onehot), ("a row of zeros", zrow), ("negative, NaN, inf", bad)):
            out.append(dict(with_options(base, w, nm), name="weights: %s norm%d" % (name, nm)))
    return out


def all_cases():
    return matrix_cases() + end_cases() + weight_cases()


def run_consensus(lib, c, dev=Host, **over):
    """-> (rc, dist [B, n, n], risk [B, n], best [B]) of one lxo_consensus call on case c; the outputs start at -7.  over: arguments to replace"""
    B, n = c["B"], c["n"]
    ids, w = dev.up(c["ids"]), dev.up(c["weights"])
    dist, risk, best = dev.up(np.full((B, n, n), -7, np.int32)), dev.up(np.full((B, n), -7, np.float32)), dev.up(np.full(max(B, 1), -7, np.int32))
    a = dict(ids=dev.ptr(ids), image_stride=c["strides"][0], draw_stride=c["strides"][1], tok_stride=c["strides"][2], B=B, n=n, T=c["T"], id_end=c["id_end"],
             weights=dev.ptr(w), normalize=c["normalize"], dist=dev.ptr(dist), risk=dev.ptr(risk), best=dev.ptr(best))
    a.update(over)
    rc = lib.lxo_consensus(a["ids"], a["image_stride"], a["draw_stride"], a["tok_stride"], a["B"], a["n"], a["T"], a["id_end"], a["weights"], a["normalize"],
                           a["dist"], a["risk"], a["best"], dev.stream)
    return rc, dev.down(dist), dev.down(risk), dev.down(best)[:B]


def check_outputs(c, dist, risk, best):
    """the outputs of a call on case c against its reference"""
    B, n, name = c["B"], c["n"], c["name"]
    assert np.array_equal(dist, c["dist"]), (name, dist.tolist(), c["dist"].tolist())
    assert np.array_equal(dist, dist.transpose(0, 2, 1)) and not dist[:, np.arange(n), np.arange(n)].any(), name
    assert best.tolist() == [int(np.argmin(risk[g])) for g in range(B)], (name, best.tolist(), risk.tolist())      # a function of the bytes written
    if c["weights"] is None and not c["normalize"]:
        exact = dist.sum(axis=2).astype(np.float32) / np.float32(n)
        assert risk.tobytes() == exact.tobytes(), (name, risk.tolist(), exact.tolist())
    ref = c["risk"]
    err = np.abs(risk.astype(np.float64) - ref)
    assert (err <= bound(n) * ref).all(), (name, float((err / np.maximum(ref, 1e-300)).max()), bound(n))
    for g in range(B):
        assert ref[g, best[g]] - ref[g].min() <= bound(n) * ref[g].min(), (name, g, ref[g].tolist(), int(best[g]))


def check_case(lib, c, dev=Host):
    rc, dist, risk, best = run_consensus(lib, c, dev)
    assert rc == 0, (c["name"], lib.lxo_last_error())
    check_outputs(c, dist, risk, best)
    return dist, risk, best


# ------------------------------------------------------------------------------------------------- above the C ABI: engine and model --
def host_reference(ids, id_end, weights=None, normalize=True):
    """ids [B, T, n] -> (dist, risk float64, the sequences)"""
    seqs = [[[int(x) for x in (truncate_end(ids[b, :, j], id_end) if id_end is not None else ids[b, :, j])] for j in range(ids.shape[2])]
            for b in range(ids.shape[0])]
    dist = distances(seqs)
    return dist, reference_risk(seqs, dist, weights, normalize), seqs


def check_against_host(ids, id_end, best, risk, dist=None, weights=None, normalize=True):
    d_ref, r_ref, _ = host_reference(ids, id_end, weights, normalize)
    n = ids.shape[2]
    assert best.dtype == np.int32 and risk.dtype == np.float32 and best.shape == ids.shape[:1] and risk.shape == (ids.shape[0], n)
    if dist is not None:
        assert dist.dtype == np.int32 and np.array_equal(dist, d_ref)
    assert (np.abs(risk - r_ref) <= bound(n) * r_ref).all(), (risk, r_ref)
    assert best.tolist() == np.argmin(risk, axis=1).tolist()
    for b in range(len(best)):
        assert r_ref[b, best[b]] - r_ref[b].min() <= bound(n) * r_ref[b].min()
    return d_ref


def check_sample_batch(model, imgs, n, id_end, **kw):
    """sample_batch(consensus=True) against the engine's draws at the same arguments and the host reference -> the result"""
    plain = model.sample_batch(imgs, n, **kw)
    res = model.sample_batch(imgs, n, consensus=True, **kw)
    assert all("consensus" not in r and "risk" not in r["hypotheses"][0] for r in plain)
    # every key there was stays as it was, in the same order of hypotheses
    for r, p in zip(res, plain):
        assert set(r) == set(p) | {"consensus", "expected_cost"} and r["agreement"] == p["agreement"]
        assert [{k: v for k, v in h.items() if k != "risk"} for h in r["hypotheses"]] == p["hypotheses"]
    max_iter = getattr(model._config, "max_length_formula", 150) + 1
    dec = {k: v for k, v in kw.items() if k in ("temperature", "top_k", "top_p", "seed")}
    ids, best, risk = model.engine.sample_decode(model._get_feed_dict(imgs, dropout=1)["img"], id_end, n=n, max_iter=max_iter, return_consensus=True, **dec)
    _, r_ref, seqs = host_reference(ids, id_end)
    for b, r in enumerate(res):
        texts = [" ".join(model._vocab.id_to_tok[i] for i in s) for s in seqs[b]]
        assert r["hypotheses"][r["consensus"]]["text"] == texts[best[b]]
        assert r["expected_cost"] == r["hypotheses"][r["consensus"]]["risk"] == float(risk[b, best[b]])
        for h in r["hypotheses"]:
            j = texts.index(h["text"])                               # its first draw
            assert h["risk"] == float(risk[b, j]) and abs(h["risk"] - r_ref[b, j]) <= bound(n) * r_ref[b, j]
            assert all(float(risk[b, k]) == h["risk"] for k in range(n) if texts[k] == h["text"])      # equal draws, equal risk, bit for bit
        assert r["expected_cost"] == min(h["risk"] for h in r["hypotheses"])
    return res
