"""TEST INFRASTRUCTURE: the host reference of lxo_sentence_bleu, lxo_consensus_bleu and lxo_mrt_candidates_cost -- include/lxo.h's definition of
the sentence-level BLEU in float64, written from the project's own _ngrams counts (model/evaluation/text.py) and truncate_end, independent of the
kernel's counting identity -- with the case matrix and the checks that tests/test_sentence_bleu_sim.py, tests/test_consensus_bleu_sim.py (hipsim)
and tests/test_gpu_sentence_bleu.py (MI355X) share.  Integers are compared exactly, the named exact cases on their bytes, floats against float64
within BOUND / RISK_BOUND.  The expected values are computed once per process and never changed."""
import functools
import math

import numpy as np

from latex_ocr_amd import _abi
from latex_ocr_amd.model.evaluation.text import _ngrams, truncate_end
from latex_ocr_amd.model.utils.text import pad_batch_formulas
from edit_distance_ref import Host  # noqa: F401  (the numpy side of the Host / device indirection, re-exported)
from consensus_ref import clean_weights

LIMIT, MAX_N, NCNT = _abi.LXO_EDIT_MAX_REF, _abi.LXO_CONSENSUS_MAX_N, _abi.LXO_BLEU_COUNTS
END = 2
# The issue's derivation: |ln p_n| <= ln 2050; four f32 logs at <= 2 ulp and the roundings of their sum give <= 1.3e-5 on the sum, 3.3e-6 on the
# exponent; the brevity exponent adds <= 1e-7, expf 2 ulp of a value <= 1: about 4e-6 in all.  A risk is a weighted mean of such costs plus
# 64 * 2^-24 for the summation.
BOUND, RISK_BOUND, GAP = 1e-5, 2e-5, 4e-5
WIDTHS = [64, 65, 128, 129, 256, 257, 512, 513, 1024]
WAVE_HYP_LENS = [63, 64, 65, 127, 128, 129]
WORST = {}                                                         # the largest deviations seen in this process: "bleu", "risk"


def note(kind, err):
    WORST[kind] = max(WORST.get(kind, 0.0), float(err))


def counts_of(h, r):
    """m_1..4, t_1..4, |h|, |r|"""
    h, r = [int(x) for x in h], [int(x) for x in r]
    m = []
    for n in range(1, 5):
        R = _ngrams(r, n)
        m.append(sum(min(c, R[g]) for g, c in _ngrams(h, n).items()))
    return m + [max(1, len(h) - n + 1) for n in range(1, 5)] + [len(h), len(r)]


def bleu_of(h, r):
    """the definition, float64"""
    h, r = [int(x) for x in h], [int(x) for x in r]
    if h == r:
        return 1.0
    c = counts_of(h, r)
    if c[0] == 0:
        return 0.0
    s = math.log(c[0] / c[4]) + sum(math.log((c[k] + 1.0) / (c[4 + k] + 1.0)) for k in (1, 2, 3))
    bp = 1.0 if len(h) > len(r) else math.exp(1.0 - len(r) / len(h))
    return bp * math.exp(0.25 * s)


def _seq(row, length, id_end):
    row = [int(x) for x in row[:max(length, 0)]]
    return truncate_end(row, id_end) if id_end >= 0 else row


def _case(name, hyp, ref, geom=None, T=None, hyp_len=None, ref_len=None, ref_of=None, per_ref=1, pairs=None, id_end=-1):
    """geom = (hyp_block, block_stride, row_stride, tok_stride), None: plain rows [pairs, T].  Lengths and reference indices may lie outside their
    ranges: the reference clamps them as the device does (a length into [0, row], an index into [0, G))."""
    hyp, ref = np.ascontiguousarray(hyp, np.int32), np.ascontiguousarray(ref, np.int32)
    if geom is None:
        pairs, T = hyp.shape
        geom = (1, T, 0, 1)
    flat = hyp.reshape(-1)
    G, Tr = ref.shape
    cut, counts, bleu = [], [], []
    for p in range(pairs):
        start = (p // geom[0]) * geom[1] + (p % geom[0]) * geom[2]
        row = flat[start:start + max(T - 1, 0) * geom[3] + 1:geom[3]] if T else flat[:0]
        h = _seq(row, T if hyp_len is None else min(int(hyp_len[p]), T), id_end)
        g = min(max(int(ref_of[p]) if ref_of is not None else p // per_ref, 0), G - 1)
        r = _seq(ref[g], Tr if ref_len is None else min(int(ref_len[g]), Tr), id_end)
        cut.append((h, r))
        counts.append(counts_of(h, r))
        bleu.append(bleu_of(h, r))
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
    return dict(name=name, hyp=flat if flat.size else np.zeros(1, np.int32), geom=geom, T=int(T), hyp_len=i32(hyp_len), ref=ref, ref_len=i32(ref_len),
                ref_of=i32(ref_of), per_ref=per_ref, pairs=pairs, id_end=id_end, cut=cut, counts=np.asarray(counts, np.int32).reshape(pairs, NCNT),
                bleu=np.asarray(bleu, np.float64))


def _rows(seqs, width=None, fill=0):
    width = max([len(s) for s in seqs] + [1]) if width is None else width
    out = np.full((len(seqs), width), fill, np.int64)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out, [len(s) for s in seqs]


@functools.lru_cache(maxsize=None)
def pair_cases():
    rng = np.random.default_rng(41)
    out = []
    # |h| x |r| in {0 .. 5}^2 over three symbols: orders that outrun a side
    hl = [a for a in range(6) for _ in range(6)]
    rl = [b for _ in range(6) for b in range(6)]
    out.append(_case("short 6 x 6", rng.integers(0, 3, size=(36, 5)), rng.integers(0, 3, size=(36, 5)), hyp_len=hl, ref_len=rl))
    # clipping: a a a a a a against a a and the reverse; a prefix either way; no unigram in common
    x = [0, 1, 1, 2, 0, 1, 2, 2]
    h, hl = _rows([[1] * 6, [1] * 2, x[:5], x, [0, 1, 0, 1], [0] * 4])
    r, rl = _rows([[1] * 2, [1] * 6, x, x[:5], [2, 2, 2], [1] * 4])
    c = _case("clipping", h, r, hyp_len=hl, ref_len=rl)
    assert c["counts"][0, :4].tolist() == [2, 1, 0, 0] and c["counts"][1, :4].tolist() == [2, 1, 0, 0] and c["bleu"][4] == 0.0 and c["bleu"][5] == 0.0
    out.append(c)
    # equal pairs of every short length: the override (an identical 2-token pair would otherwise score below 1)
    lens = [0, 1, 2, 3, 4, 5, 64, 65, 130]
    same = rng.integers(0, 3, size=(len(lens), 130))
    c = _case("identical", same, same, hyp_len=lens, ref_len=lens)
    assert (c["bleu"] == 1.0).all()
    out.append(c)
    # wave chunks: every hypothesis length against a full-length reference of each width
    hyp = rng.integers(0, 3, size=(len(WAVE_HYP_LENS), max(WAVE_HYP_LENS)))
    hyp[::2] = hyp[::2] % 2
    for Wd in WIDTHS:
        out.append(_case("wave, ref %d" % Wd, hyp, rng.integers(0, 3 if Wd % 2 else 2, size=(1, Wd)), hyp_len=WAVE_HYP_LENS, per_ref=len(WAVE_HYP_LENS)))
    # both sides at full width, hypothesis = reference with a few tokens changed (long matches, BLEU near 1) and an unrelated one
    for Wd in (129, 513, LIMIT):
        ref = rng.integers(0, 3, size=(1, Wd))
        near = ref.repeat(2, axis=0)
        near[0, ::37] = 3
        near[1] = rng.integers(0, 3, size=Wd)
        out.append(_case("full width %d" % Wd, near, ref, per_ref=2))
    # END at position 0, as the last token, absent; lengths clamped from above and below; a reference index out of range; id_end < 0
    body = rng.integers(0, 2, size=(4, 12))
    rows = body.copy()
    rows[0, 0] = END
    rows[1, 11] = END
    rows[3, 6] = END
    both = [(i, j) for i in range(4) for j in range(4)]
    hrows, of = rows[[i for i, _ in both]], [j for _, j in both]
    out.append(_case("END, no lengths", hrows, rows, ref_of=of, id_end=END))
    out.append(_case("END, lengths clamped", hrows, rows, hyp_len=[99, -3, 12, 5] * 4, ref_len=[40, 12, -1, 9], ref_of=of, id_end=END))
    out.append(_case("ref_of out of range", hrows, rows, ref_of=[-2, 7, 4, -1] * 4, id_end=END))
    out.append(_case("id_end < 0", hrows, rows, ref_of=of, id_end=-1))
    # any int32 is a token: negative ids, 0 next to the zero-filled tail of the staged rows
    big = 0x7fffffff
    seqs_h = [[-1, 0, 1, 0, big], [big, big, 0, -1, -1], [0] * 5, [-1] * 5, [0, 0], [-1], [0, -1, 0, -1, 0, -1, 0], [0, 0, 0]]
    seqs_r = [[-1, 0, 1, 1, big], [big, 0, -1, -1], [0] * 2, [-1] * 2, [0] * 6, [-1] * 4, [-1, 0, -1, 0], [0, 0, 0, 0, 0, 0, 0]]
    h0, hl = _rows(seqs_h, 12, 0)
    r0, rl = _rows(seqs_r, 12, 0)
    out.append(_case("unusual ids, zeros behind", h0, r0, hyp_len=hl, ref_len=rl))
    h1, _ = _rows(seqs_h, 12, -1)
    r1, _ = _rows(seqs_r, 12, -1)
    out.append(_case("unusual ids, -1 behind", h1, r1, hyp_len=hl, ref_len=rl))
    # the [B, max_steps, n] layout of a sampled decode read in place, references in pad_batch_formulas' layout
    tok = np.array([0, 1])
    B, T, n = 2, 70, 3
    ids = rng.choice(tok, size=(B, T + 2, n))
    ids[0, 30, 0] = ids[0, 0, 1] = ids[1, 66, 2] = END
    refs, rl = pad_batch_formulas([list(rng.choice(tok, 33)), list(rng.choice(tok, 67))], 5, END)
    out.append(_case("strided [B, T, n]", ids, refs, geom=(n, (T + 2) * n, 1, n), T=T, ref_len=rl, per_ref=n, pairs=B * n, id_end=END))
    return out


CASE_NAMES = [c["name"] for c in pair_cases()]


def named(name):
    return pair_cases()[CASE_NAMES.index(name)]


def text_stats_args(c, dev=Host):
    """the addressing arguments lxo_text_stats and lxo_sentence_bleu share, uploaded: -> (keep-alive list, argument tuple)"""
    keep = [dev.up(c[k]) for k in ("hyp", "hyp_len", "ref", "ref_len", "ref_of")]
    g = c["geom"]
    return keep, (dev.ptr(keep[0]), g[0], g[1], g[2], g[3], c["T"], dev.ptr(keep[1]), dev.ptr(keep[2]), c["ref"].shape[0], c["ref"].shape[1],
                  dev.ptr(keep[3]), dev.ptr(keep[4]), c["per_ref"], c["pairs"], c["id_end"])


def run_bleu(lib, c, dev=Host, want=(True, True, True)):
    """-> (rc, counts, bleu, cost) of one lxo_sentence_bleu call on case c; outputs start at -7; want: which outputs are passed"""
    keep, args = text_stats_args(c, dev)
    outs = [dev.up(np.full(s, -7, t)) if w else None for w, (s, t) in zip(want, (((c["pairs"], NCNT), np.int32), (c["pairs"], np.float32), (c["pairs"], np.float32)))]
    rc = lib.lxo_sentence_bleu(*(args + tuple(dev.ptr(o) for o in outs) + (dev.stream,)))
    return (rc,) + tuple(None if o is None else dev.down(o) for o in outs)


def run_text_stats(lib, c, dev=Host):
    keep, args = text_stats_args(c, dev)
    stats = dev.up(np.full((c["pairs"], _abi.LXO_TEXT_STATS), -7, np.int32))
    rc = lib.lxo_text_stats(*(args + (dev.ptr(stats), dev.ptr(None), 0, dev.stream)))
    return rc, dev.down(stats)


def check_floats(name, bleu, cost, ref):
    """f32 bleu / cost [pairs] against the float64 scores: the exact cases on their bytes, the rest within BOUND"""
    one, zero = np.float32(1.0).tobytes(), np.float32(0.0).tobytes()
    for p, b in enumerate(ref):
        if b == 1.0 or b == 0.0:
            assert bleu[p].tobytes() == (one if b else zero) and cost[p].tobytes() == (zero if b else one), (name, p, bleu[p], cost[p], b)
    assert bleu.dtype == np.float32 and cost.dtype == np.float32
    err = max(np.abs(bleu.astype(np.float64) - ref).max(initial=0.0), np.abs(cost.astype(np.float64) - (1.0 - ref)).max(initial=0.0))
    note("bleu", err)
    print("%s: largest |bleu - float64| or |cost - float64| = %.3g (bound %.0e)" % (name, err, BOUND))
    assert err <= BOUND, (name, err)
    assert ((cost >= 0) & (cost <= 1)).all()


def check_pair_case(lib, c, dev=Host):
    rc, counts, bleu, cost = run_bleu(lib, c, dev)
    assert rc == 0, (c["name"], lib.lxo_last_error())
    bad = np.flatnonzero((counts != c["counts"]).any(1))
    assert not bad.size, (c["name"], bad[:4].tolist(), counts[bad[:4]].tolist(), c["counts"][bad[:4]].tolist())
    rc, stats = run_text_stats(lib, c, dev)
    assert rc == 0 and np.array_equal(stats[:, :NCNT], counts), c["name"]
    same = np.array([h == r for h, r in c["cut"]])
    assert np.array_equal(stats[:, 11] == 1, same) and (c["bleu"][same] == 1.0).all()
    check_floats(c["name"], bleu, cost, c["bleu"])
    return counts, bleu, cost


# ------------------------------------------------------------------------------------------------------------------ consensus --
def cost_matrix(seqs):
    """seqs [B][n] -> (cost float64 [B, n, n] with cost[g][i][j] = 1 - sBLEU(hypothesis i, reference j), match int32 [B, n, n, 4])"""
    B, n = len(seqs), len(seqs[0])
    cost, match = np.zeros((B, n, n)), np.zeros((B, n, n, 4), np.int32)
    for g in range(B):
        for i in range(n):
            for j in range(n):
                match[g, i, j] = counts_of(seqs[g][i], seqs[g][j])[:4]
                cost[g, i, j] = 1.0 - bleu_of(seqs[g][i], seqs[g][j])
    return cost, match


def risk_of(cost, weights):
    w = clean_weights(weights, cost.shape[0], cost.shape[1])
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


def make_cons(name, ids, T, id_end, layout="BTn", weights=None, ties=False):
    """ids [B, T + noise, n] ("BTn": what a sampled decode writes) or [B, n, T] ("BnT").  ties: a named equal-draw case, where two best risks may be
    equal; everywhere else the two best DISTINCT risks of every image lie more than GAP apart (asserted here, on the CPU)."""
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
    cost, match = cost_matrix(seqs)
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    c = dict(name=name, ids=flat if flat.size else np.zeros(1, np.int32), strides=strides, B=B, n=n, T=T, id_end=id_end, weights=w, seqs=seqs, cost=cost,
             match=match, ties=ties)
    return _with_risk(c)


def _with_risk(c):
    risk = risk_of(c["cost"], c["weights"])
    for g in range(c["B"]):
        d = np.unique(risk[g])
        assert len(d) < 2 or d[1] - d[0] > GAP or _equal_draws_only(c, g, risk[g], d), (c["name"], g, d[:3].tolist())
    return dict(c, risk=risk, best=np.argmin(risk, axis=1).astype(np.int32))


def _equal_draws_only(c, g, risk, d):
    """two best risks closer than GAP are allowed only where they belong to equal draws (then they are equal exactly)"""
    close = [i for i in range(c["n"]) if risk[i] - d[0] <= GAP]
    return c["ties"] and all(c["seqs"][g][i] == c["seqs"][g][close[0]] for i in close)


def with_weights(c, weights):
    return _with_risk(dict(c, weights=None if weights is None else np.ascontiguousarray(weights, np.float32)))


def _random_ids(rng, B, T, n, cut):
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
def cons_cases():
    rng = np.random.default_rng(47)
    out = []

    def add(B, T, n, cut, layout="BTn"):
        for _ in range(50):                                         # draws whose best risks are told apart by more than GAP (the assertion of make_cons)
            ids = _random_ids(rng, B, T, n, cut)
            if layout == "BnT":
                ids = ids[:, :T].transpose(0, 2, 1)
            try:
                out.append(make_cons("B%d T%d n%d %s %s" % (B, T, n, "cut" if cut else "whole", layout), ids, T, END if cut else -1, layout))
                return
            except AssertionError:
                continue
        raise AssertionError("no draws with a gap above GAP for B%d T%d n%d" % (B, T, n))

    k = 0
    for n in (1, 2, 3, 5):
        for B in (1, 3):
            for T in ((0, 9) if n == 2 else (12,)):
                add(B, T, n, k % 2)
                k += 1
    add(1, 7, MAX_N, 1)
    add(3, 7, MAX_N, 0)
    for T in (64, 65, 129, 257, 513, LIMIT):
        add(1, T, 3 if T < LIMIT else 2, k % 2)
        k += 1
    add(3, 70, 3, 1, "BnT")
    # named equal-draw cases
    E, T = END, 8
    x, y = [0, 1, 1, 0, 1, 0, 0, 1], [1, 1, 0, 0, 0, 1, 0, 1]

    def rows(draws, seed=1):
        r = np.random.default_rng(seed)
        B, n = len(draws), len(draws[0])
        ids = r.integers(0, 3, size=(B, T + 2, n))
        for g in range(B):
            for i, d in enumerate(draws[g]):
                ids[g, :len(d), i] = d
        return ids
    out.append(make_cons("all draws empty", rows([[[E, 0, 1], [E], [E, 1]], [[E], [E, E], [E, 0]]]), T, E, ties=True))
    out.append(make_cons("all draws equal", rows([[x[:5] + [E]] * 4, [y] * 4], 2), T, E, ties=True))
    out.append(make_cons("two equal draws tie", rows([[x, y[:6] + [E], y[:6] + [E, 1]], [y, x[:4] + [E, 0], x[:4] + [E, 1]]]), T, E, ties=True))
    out.append(make_cons("END at 0, absent, behind T, inside", rows([[[E] + x[:5], x, y, x[:3] + [E] + y[:3]]]), T, E))
    return out


def cons_weight_cases():
    """consensus_ref.weight_cases()' weights (one-hot, a row of zeros, negative / NaN / inf, ...) on draws of this module (B = 3, n = 5; draw 3 repeats
    draw 1)"""
    from consensus_ref import weight_cases
    rng = np.random.default_rng(53)
    seen, out = set(), []
    for _ in range(50):
        ids = _random_ids(rng, 3, 20, 5, True)
        ids[:, :, 3] = ids[:, :, 1]
        try:
            base = make_cons("weights: none", ids, 20, END, ties=True)
            out = []
            for wc in weight_cases():
                key = wc["name"].rsplit(" norm", 1)[0]
                if key not in seen:
                    out.append(dict(with_weights(base, wc["weights"]), name=key))
                    seen.add(key)
            return out
        except AssertionError:
            seen.clear()
    raise AssertionError("no draws with a gap above GAP under every weight case")


def run_cons(lib, c, dev=Host, want_match=True, **over):
    """-> (rc, match [B, n, n, 4] or None, cost [B, n, n], risk [B, n], best [B]) of one lxo_consensus_bleu call; outputs start at -7"""
    B, n = c["B"], c["n"]
    ids, w = dev.up(c["ids"]), dev.up(c["weights"])
    match = dev.up(np.full((B, n, n, 4), -7, np.int32)) if want_match else None
    cost, risk, best = dev.up(np.full((B, n, n), -7, np.float32)), dev.up(np.full((B, n), -7, np.float32)), dev.up(np.full(max(B, 1), -7, np.int32))
    a = dict(ids=dev.ptr(ids), image_stride=c["strides"][0], draw_stride=c["strides"][1], tok_stride=c["strides"][2], B=B, n=n, T=c["T"], id_end=c["id_end"],
             weights=dev.ptr(w), match=dev.ptr(match), cost=dev.ptr(cost), risk=dev.ptr(risk), best=dev.ptr(best))
    a.update(over)
    rc = lib.lxo_consensus_bleu(a["ids"], a["image_stride"], a["draw_stride"], a["tok_stride"], a["B"], a["n"], a["T"], a["id_end"], a["weights"], a["match"],
                                a["cost"], a["risk"], a["best"], dev.stream)
    return rc, None if match is None else dev.down(match), dev.down(cost), dev.down(risk), dev.down(best)[:B]


def check_cons_outputs(c, match, cost, risk, best):
    B, n, name = c["B"], c["n"], c["name"]
    if match is not None:
        assert np.array_equal(match, c["match"]), name
        assert np.array_equal(match, match.transpose(0, 2, 1, 3)), name
    d = np.arange(n)
    assert cost[:, d, d].tobytes() == np.zeros((B, n), np.float32).tobytes(), name
    for g in range(B):
        for i in range(n):
            for j in range(n):
                if c["cost"][g, i, j] in (0.0, 1.0):
                    assert cost[g, i, j].tobytes() == np.float32(c["cost"][g, i, j]).tobytes(), (name, g, i, j)
                if c["seqs"][g][i] == c["seqs"][g][j]:               # equal draws: equal rows, equal risks, bit for bit
                    assert cost[g, i].tobytes() == cost[g, j].tobytes() and risk[g, i].tobytes() == risk[g, j].tobytes(), (name, g, i, j)
    err = np.abs(cost.astype(np.float64) - c["cost"]).max(initial=0.0)
    note("bleu", err)
    rerr = np.abs(risk.astype(np.float64) - c["risk"]).max(initial=0.0)
    note("risk", rerr)
    print("%s: largest |cost - float64| = %.3g (bound %.0e), |risk - float64| = %.3g (bound %.0e)" % (name, err, BOUND, rerr, RISK_BOUND))
    assert err <= BOUND and rerr <= RISK_BOUND, (name, err, rerr)
    assert best.tolist() == [int(np.argmin(risk[g])) for g in range(B)], (name, best.tolist(), risk.tolist())      # a function of the bytes written
    for g in range(B):
        assert risk[g, c["best"][g]] - risk[g].min() <= GAP, (name, g)
    assert best.tolist() == c["best"].tolist(), (name, best.tolist(), c["best"].tolist())


def check_cons_case(lib, c, dev=Host):
    rc, match, cost, risk, best = run_cons(lib, c, dev)
    assert rc == 0, (c["name"], lib.lxo_last_error())
    check_cons_outputs(c, match, cost, risk, best)
    return match, cost, risk, best


def host_consensus(ids, id_end, weights=None):
    """ids [B, T, n] -> (cost float64 [B, n, n], risk float64 [B, n], the sequences)"""
    seqs = [[[int(x) for x in (truncate_end(ids[b, :, j], id_end) if id_end is not None else ids[b, :, j])] for j in range(ids.shape[2])]
            for b in range(ids.shape[0])]
    cost, _ = cost_matrix(seqs)
    return cost, risk_of(cost, weights), seqs
