"""TEST INFRASTRUCTURE: the host reference of lxo_beam_finalize and lxo_beam_rerank -- include/lxo.h's definitions restated, the back-trace in numpy
integers and np.float32, the rerank in float64 -- with the case matrix, the derived bounds and the runners that tests/test_beam_finalize_sim.py
(hipsim) and tests/test_gpu_beam_finalize.py (MI355X) share.  Finalize is compared exactly (ints, and f32 as bytes); the rerank's scores and
posterior against float64 within bounds derived below, its order exactly against the device's own scores.  The cases are built once per process."""
import functools

import numpy as np

from latex_ocr_amd import _abi
from edit_distance_ref import Host  # noqa: F401  (the numpy side of the Host / device indirection, re-exported)

V, END = 7, 2
MAX_K, MAX_STEPS = _abi.LXO_BEAM_MAX_K, _abi.LXO_BEAM_MAX_STEPS
KS, STEPS = (1, 2, 5, 16), (1, 2, 7, 65, 152, MAX_STEPS)
PATTERNS = ("identity", "random", "permutation", "collapse")
ENDS = ("step0", "none", "offpath", "mixed")
OUTPUTS = ("hyp", "len", "src", "tok_logp", "seq_logp")


# ------------------------------------------------------------------------------------------------------------------ finalize --
def slots_of(parents, steps, k):
    """the definition: slot[b][steps - 1][i] = i, slot[b][t - 1][i] = P[b][t][slot[b][t][i]] with P the parents clamped into [0, k)"""
    P = np.clip(np.asarray(parents)[:, :steps].astype(np.int64), 0, k - 1)
    B = P.shape[0]
    slot = np.empty((B, steps, k), np.int64)
    cur = np.tile(np.arange(k), (B, 1))
    rows = np.arange(B)[:, None]
    for t in range(steps - 1, -1, -1):
        slot[:, t] = cur
        cur = P[rows, t, cur]
    return P, slot


def finalize_reference(ids, parents, scores, steps, k, id_end):
    """-> dict of the five outputs as the header defines them (tok_logp / seq_logp None without scores)"""
    ids = np.asarray(ids)
    B = ids.shape[0]
    P, slot = slots_of(parents, steps, k)
    tok = np.take_along_axis(ids[:, :steps].astype(np.int64), slot, axis=2)
    hit = tok == id_end
    ln = np.where(hit.any(axis=1), hit.argmax(axis=1) + 1, steps)                         # [B, k]
    live = np.arange(steps)[None, :, None] < ln[:, None, :]
    out = dict(hyp=np.where(live, tok, id_end).astype(np.int32), len=ln.astype(np.int32),
               src=(np.take_along_axis(P, slot, axis=2) + (np.arange(B) * k)[:, None, None]).transpose(1, 0, 2).reshape(steps, B * k).astype(np.int32),
               tok_logp=None, seq_logp=None)
    if scores is not None:
        run = np.take_along_axis(np.asarray(scores, np.float32)[:, :steps], slot, axis=2)
        prev = np.concatenate([np.zeros((B, 1, k), np.float32), run[:, :-1]], axis=1)
        out["tok_logp"] = np.where(live, run - prev, np.float32(0)).astype(np.float32)      # one f32 subtraction
        out["seq_logp"] = np.take_along_axis(run, (ln - 1)[:, None, :], axis=1)[:, 0].astype(np.float32)
    return out


def make_parents(rng, B, T, k, pattern):
    if pattern == "identity":
        return np.tile(np.arange(k, dtype=np.int32), (B, T, 1))
    if pattern == "permutation":
        return np.stack([np.stack([rng.permutation(k) for _ in range(T)]) for _ in range(B)]).astype(np.int32)
    p = rng.integers(0, k, size=(B, T, k)).astype(np.int32)
    if pattern == "collapse":
        for b in range(B):
            p[b, int(rng.integers(0, T))] = 0                       # every slot descends from slot 0 there
    return p


def make_case(name, B, k, steps, ld_t, pattern, ends, seed, bad_parent=False):
    """ids / parents / scores [B, ld_t, k]; the columns at or behind `steps` hold other valid slots and tokens (END among them), so a read behind
    `steps` shows as a wrong result"""
    rng = np.random.default_rng(seed)
    parents = make_parents(rng, B, ld_t, k, pattern)
    if ld_t > steps:
        parents[:, steps:] = rng.integers(0, k, size=(B, ld_t - steps, k))
        if pattern == "identity" and k > 1:
            parents[:, steps:] = (np.arange(k) + 1) % k             # a walk that started behind `steps` would arrive rotated
    plain = np.array([t for t in range(V) if t != END])
    ids = plain[rng.integers(0, V - 1, size=(B, ld_t, k))].astype(np.int32)
    ids[:, steps:] = rng.integers(0, V, size=(B, ld_t - steps, k))
    scores = (-np.cumsum(rng.uniform(0.01, 2.0, size=(B, ld_t, k)), axis=1) + rng.normal(0, 0.3, size=(B, ld_t, k))).astype(np.float32)
    if bad_parent:
        for b in range(B):
            parents[b, int(rng.integers(0, steps)), int(rng.integers(0, k))] = (k + 3, -2, 1 << 30, -(1 << 31))[b % 4]
    _, slot = slots_of(parents, steps, k)
    rows = np.arange(B)
    if ends == "step0":
        ids[rows, 0, slot[:, 0, 0]] = END                            # path 0 ends at once (and whatever shares its first slot)
    elif ends == "offpath":
        for b in range(B):
            for t in range(steps):
                off = np.setdiff1d(np.arange(k), slot[b, t])
                ids[b, t, off] = END                                # every slot no path goes through: none may shorten anything
    elif ends == "mixed":
        for b in range(B):
            for i in range(0, k, 2):
                t = int(rng.integers(0, steps))
                ids[b, t, slot[b, t, i]] = END
    c = dict(name=name, B=B, k=k, steps=steps, ld_t=ld_t, id_end=END, ids=ids, parents=parents, scores=scores, ends=ends, pattern=pattern)
    c["want"] = finalize_reference(ids, parents, scores, steps, k, END)
    return c


@functools.lru_cache(maxsize=None)
def matrix_cases():
    """B x k x steps x (ld_t = steps | above); the parent patterns and END placements cycle so that every pair of them occurs.  steps = 1024 runs at
    k = 16 once and at the smaller widths on one image."""
    out, n = [], 0
    for steps in STEPS:
        for k in KS:
            for B in (1, 3):
                for pad in (0, 3):
                    if steps == MAX_STEPS and (B, pad) != ((3, 3) if k == 16 else (1, 0 if k == 2 else 3)):
                        continue
                    pattern, ends = PATTERNS[n % 4], ENDS[(n // 4 + n) % 4]
                    out.append(make_case("B%d k%d steps%d ld%d %s %s" % (B, k, steps, steps + pad, pattern, ends), B, k, steps, steps + pad, pattern, ends, 100 + n))
                    n += 1
    return out


@functools.lru_cache(maxsize=None)
def special_cases():
    out = [make_case("clamp: one parent out of range per image", 4, 5, 9, 11, "random", "mixed", 7, bad_parent=True)]
    # every pattern under every END placement once more at one small shape
    for a, p in enumerate(PATTERNS):
        for e, x in enumerate(ENDS):
            out.append(make_case("pairs: %s %s" % (p, x), 2, 5, 12, 13, p, x, 300 + 4 * a + e))
    return out


def all_cases():
    return matrix_cases() + special_cases()


def preconditions(cases):
    """what the matrix claims to hold, asserted on the reference alone"""
    seen = {(c["pattern"], c["ends"]) for c in cases}
    assert seen == {(p, e) for p in PATTERNS for e in ENDS}, sorted(seen)
    off = [c for c in cases if c["ends"] == "offpath" and (c["ids"][:, :c["steps"]] == END).any()]
    assert len(off) >= 3 and all((c["want"]["len"] == c["steps"]).all() for c in off)
    mixed = [c for c in cases if c["ends"] == "mixed" and c["k"] > 1 and c["steps"] > 2]
    assert any((c["want"]["len"] < c["steps"]).any() and (c["want"]["len"] == c["steps"]).any() for c in mixed)
    assert any((c["want"]["len"] == 1).any() for c in cases if c["ends"] == "step0" and c["steps"] > 1)
    assert any(c["steps"] == MAX_STEPS and c["k"] == MAX_K for c in cases)


def run_finalize(lib, c, dev=Host, outputs=OUTPUTS, with_scores=True, **over):
    """-> (rc, dict of the outputs asked for) of one lxo_beam_finalize call on case c; the outputs start at -7.  over: arguments to replace"""
    B, k, steps = c["B"], c["k"], c["steps"]
    ids, par, sc = dev.up(c["ids"]), dev.up(c["parents"]), dev.up(c["scores"]) if with_scores else None
    shape = dict(hyp=((B, steps, k), np.int32), len=((B, k), np.int32), src=((steps, B * k), np.int32), tok_logp=((B, steps, k), np.float32),
                 seq_logp=((B, k), np.float32))
    bufs = {n: dev.up(np.full(shape[n][0], -7, shape[n][1])) if n in outputs else None for n in OUTPUTS}
    a = dict(ids=dev.ptr(ids), parents=dev.ptr(par), scores=dev.ptr(sc), B=B, ld_t=c["ld_t"], steps=steps, k=k, id_end=c["id_end"])
    a.update(over)
    rc = lib.lxo_beam_finalize(a["ids"], a["parents"], a["scores"], a["B"], a["ld_t"], a["steps"], a["k"], a["id_end"],
                               *([dev.ptr(bufs[n]) for n in OUTPUTS] + [dev.stream]))
    return rc, {n: dev.down(bufs[n]) for n in OUTPUTS if bufs[n] is not None}


def check_finalize(c, got):
    for n, g in got.items():
        w = c["want"][n]
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (c["name"], n, g.tolist()[:3], w.tolist()[:3])


def check_case(lib, c, dev=Host):
    rc, got = run_finalize(lib, c, dev)
    assert rc == 0 and len(got) == 5, (c["name"], lib.lxo_last_error())
    check_finalize(c, got)
    return got


# -------------------------------------------------------------------------------------------------------------------- rerank --
U = 2.0 ** -24                                                       # half an ulp of f32, relative


def rerank_reference(ln, seq, cov, R, alpha, beta, floor):
    """include/lxo.h's definition in float64 on the f32 inputs as the device receives them -> (score, post, cp), [B, k] each"""
    alpha, beta, floor = (float(np.float32(x)) for x in (alpha, beta, floor))
    ln, seq = np.asarray(ln, np.int64), np.asarray(seq, np.float32).astype(np.float64)
    B, k = seq.shape
    lp = ((5.0 + np.maximum(ln, 0)) / 6.0) ** alpha
    cp = np.zeros((B, k))
    if cov is not None:
        cells = np.asarray(cov, np.float32)[:, :R].astype(np.float64)
        cells = np.where(np.isnan(cells), floor, cells)
        cp = np.log(np.minimum(np.maximum(cells, floor), 1.0)).sum(axis=1).reshape(B, k)
    score = seq / lp + beta * cp
    e = np.exp(seq - seq.max(axis=1, keepdims=True))
    return score, e / e.sum(axis=1, keepdims=True), cp


def score_bound(seq, ln, cp, alpha, beta):
    """|device f32 score - float64 score|, derived from the arithmetic the header states: everything but the cells' logarithms is double arithmetic
    (relative errors near 2^-53: a slack of 2^-40 of each term's size covers pow, the quotient, the product and the sum many times over) rounded to
    f32 once (half an ulp: U |score|); the cells' logarithms are f32 logf, at most 2 ulp = 4 U relative each, all of one sign so that their sum carries
    at most that relative error, 4 U |cp|, scaled by beta."""
    seq, cp = np.abs(np.asarray(seq, np.float64)), np.abs(cp)
    beta = float(np.float32(beta))
    q = seq / ((5.0 + np.maximum(np.asarray(ln, np.float64), 0)) / 6.0) ** float(np.float32(alpha))
    return U * (q + beta * cp) + 4 * U * beta * cp + 2.0 ** -40 * (q + beta * cp)


def post_bound(post):
    """the softmax is double arithmetic on exact differences of f32 values, rounded to f32 once: U post, and the same slack"""
    return (U + 2.0 ** -40) * post


def stable_order(score):
    """descending, equal scores by ascending slot"""
    return np.argsort(-score, axis=1, kind="stable").astype(np.int32)


def make_rerank_case(name, B, k, alpha, beta, floor, seed, R=0, cov_ld=0, max_len=150):
    rng = np.random.default_rng(seed)
    ln = rng.integers(1, max_len + 1, size=(B, k)).astype(np.int32)
    seq = (-rng.uniform(0.5, 60.0, size=(B, k))).astype(np.float32)
    cov = None
    if R:
        cov = rng.uniform(0.0, 1.6, size=(B * k, cov_ld)).astype(np.float32)
        cov[rng.random(size=cov.shape) < 0.2] = 0.0                  # cells never attended: the floor
        cov[:, R:] = np.nan                                          # behind the R cells: never read
    return dict(name=name, B=B, k=k, len=ln, seq=seq, cov=cov, R=R, cov_ld=cov_ld, alpha=alpha, beta=beta, floor=floor)


@functools.lru_cache(maxsize=None)
def rerank_cases():
    out, n = [], 0
    for k in KS:
        for alpha, beta, R, ld in ((0.0, 0.0, 0, 0), (0.6, 0.0, 0, 0), (1.0, 0.2, 35, 40), (2.0, 1.0, 130, 130), (0.6, 0.05, 868, 872), (0.0, 0.3, 1, 1)):
            out.append(make_rerank_case("k%d alpha%g beta%g R%d" % (k, alpha, beta, R), 6 if R > 500 else 37, k, alpha, beta, (1e-3, 0.1, 1.0, 2.0 ** -20)[n % 4] if R else 0.5,
                                        500 + n, R, ld))
            n += 1
    return out


def run_rerank(lib, c, dev=Host, outputs=("score", "post", "order"), **over):
    """-> (rc, dict of the outputs asked for) of one lxo_beam_rerank call on case c; the outputs start at -7"""
    B, k = c["B"], c["k"]
    ln, seq, cov = dev.up(c["len"]), dev.up(c["seq"]), dev.up(c["cov"])
    dt = dict(score=np.float32, post=np.float32, order=np.int32)
    bufs = {n: dev.up(np.full((B, k), -7, dt[n])) if n in outputs else None for n in dt}
    a = dict(len=dev.ptr(ln), seq=dev.ptr(seq), cov=dev.ptr(cov), cov_ld=c["cov_ld"], R=c["R"], B=B, k=k, alpha=c["alpha"], beta=c["beta"], floor=c["floor"])
    a.update(over)
    rc = lib.lxo_beam_rerank(a["len"], a["seq"], a["cov"], a["cov_ld"], a["R"], a["B"], a["k"], a["alpha"], a["beta"], a["floor"],
                             dev.ptr(bufs["score"]), dev.ptr(bufs["post"]), dev.ptr(bufs["order"]), dev.stream)
    return rc, {n: dev.down(b) for n, b in bufs.items() if b is not None}


def check_rerank(c, got):
    """-> (largest score deviation / its bound, largest posterior deviation / its bound, images whose reference order is separated, images)"""
    ref, post, cp = rerank_reference(c["len"], c["seq"], c["cov"], c["R"], c["alpha"], c["beta"], c["floor"])
    sb, pb = score_bound(c["seq"], c["len"], cp, c["alpha"], c["beta"]), post_bound(post)
    score, order = got["score"], got["order"]
    es, ep = np.abs(score.astype(np.float64) - ref), np.abs(got["post"].astype(np.float64) - post)
    assert (es <= sb).all(), (c["name"], float((es / sb).max()))
    assert (ep <= pb).all(), (c["name"], float((ep / pb).max()))
    assert np.array_equal(order, stable_order(score)), (c["name"], order.tolist()[:3], score.tolist()[:3])      # of the device's own bytes
    ro = np.argsort(-ref, axis=1, kind="stable")
    rs, rb = np.take_along_axis(ref, ro, axis=1), np.take_along_axis(sb, ro, axis=1)
    sep = (rs[:, :-1] - rs[:, 1:] > 2 * np.maximum(rb[:, :-1], rb[:, 1:])).all(axis=1)
    assert np.array_equal(order[sep], ro[sep].astype(np.int32)), c["name"]
    return float((es / sb).max()), float((ep / np.maximum(pb, 1e-300)).max()), int(sep.sum()), len(sep)
