"""TEST INFRASTRUCTURE: the host reference of lxo_text_stats -- the project's own _ngrams, levenshtein and truncate_end (model/evaluation/text.py) --
with the case matrix and the exact checks that tests/test_text_stats_sim.py (hipsim) and tests/test_gpu_text_stats.py (MI355X) share.  Everything is
compared as integers.  The expected values are computed once per process and never changed."""
import functools

import numpy as np

from latex_ocr_amd import _abi
from latex_ocr_amd.model.evaluation.text import _ngrams, levenshtein, truncate_end
from latex_ocr_amd.model.utils.text import pad_batch_formulas
from edit_distance_ref import Host, REF_LENS

LIMIT = _abi.LXO_EDIT_MAX_REF
NS, NC = _abi.LXO_TEXT_STATS, _abi.LXO_TEXT_CORPUS
END = 2                                                            # inside the alphabet where a case cuts; the others pass id_end = -1
# 4-gram windows that straddle a 64-lane chunk of hypothesis positions, one or two chunks in; the decode bound
WAVE_HYP_LENS = list(range(61, 68)) + list(range(127, 132)) + [152]
V_SENTINEL = 500                                                   # "an id of V": one past a vocabulary of 500
# the matrix by name, so that a module can parametrise over it without building it at import
CASE_NAMES = (["short"] + ["wave, ref %d" % L for L in REF_LENS] + ["limit x limit", "constructed clipping", "identical", "disjoint", "END, lengths",
              "END, no lengths", "END in the rows, no cut", "unusual ids, zeros behind", "unusual ids, -1 behind", "strided [B, T, n]", "strided [B, T, n], ref_of"])


def pair_stats(h, r):
    """the 12 integers of a pair, from the host functions"""
    h, r = [int(x) for x in h], [int(x) for x in r]
    row = []
    for n in range(1, 5):
        R = _ngrams(r, n)
        row.append(sum(min(c, R[g]) for g, c in _ngrams(h, n).items()))
    row += [max(1, len(h) - n + 1) for n in range(1, 5)]
    row += [len(h), len(r), levenshtein(h, r), 1 if h == r else 0]
    return row


def corpus_of(stats):
    """the 14 integers of a set of rows"""
    s = np.asarray(stats, np.int64).reshape(-1, NS)
    return np.concatenate([s[:, :10].sum(0), [s[:, 10].sum(), np.maximum(s[:, 8], s[:, 9]).sum(), s[:, 11].sum(), s.shape[0]]]).astype(np.int64)


def clip_profile(h, r):
    """per order n: (clipped matches, hypothesis positions whose n-gram occurs anywhere in r), and whether count_h > count_r > 0 / 0 < count_h < count_r
    occurs for some n-gram -- what the condition on the matrix is stated in"""
    out, more, fewer = [], False, False
    for n in range(1, 5):
        H, R = _ngrams(h, n), _ngrams(r, n)
        out.append((sum(min(c, R[g]) for g, c in H.items()), sum(c for g, c in H.items() if R[g] > 0)))
        more |= any(c > R[g] > 0 for g, c in H.items())
        fewer |= any(0 < c < R[g] for g, c in H.items())
    return out, more, fewer


def _seq(row, length, id_end):
    row = [int(x) for x in row[:length]]
    return truncate_end(row, id_end) if id_end >= 0 else row


def _case(name, hyp, ref, geom=None, T=None, hyp_len=None, ref_len=None, ref_of=None, per_ref=1, pairs=None, id_end=-1):
    """geom = (hyp_block, block_stride, row_stride, tok_stride), None: plain rows [pairs, T]"""
    hyp, ref = np.ascontiguousarray(hyp, np.int32), np.ascontiguousarray(ref, np.int32)
    if geom is None:
        pairs, T = hyp.shape
        geom = (1, T, 0, 1)
    flat = hyp.reshape(-1)
    stats, cut = [], []
    for p in range(pairs):
        start = (p // geom[0]) * geom[1] + (p % geom[0]) * geom[2]
        row = flat[start:start + max(T - 1, 0) * geom[3] + 1:geom[3]] if T else flat[:0]
        h = _seq(row, T if hyp_len is None else int(hyp_len[p]), id_end)
        g = int(ref_of[p]) if ref_of is not None else p // per_ref
        r = _seq(ref[g], ref.shape[1] if ref_len is None else int(ref_len[g]), id_end)
        stats.append(pair_stats(h, r))
        cut.append((h, r))
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
    stats = np.asarray(stats, np.int32).reshape(pairs, NS)
    return dict(name=name, hyp=flat, geom=geom, T=int(T), hyp_len=i32(hyp_len), ref=ref, ref_len=i32(ref_len), ref_of=i32(ref_of), per_ref=per_ref,
                pairs=pairs, id_end=id_end, stats=stats, corpus=corpus_of(stats), cut=cut)


def _rows(seqs, width=None, fill=0):
    width = max([len(s) for s in seqs] + [1]) if width is None else width
    out = np.full((len(seqs), width), fill, np.int64)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out, [len(s) for s in seqs]


@functools.lru_cache(maxsize=None)
def text_cases():
    rng = np.random.default_rng(23)
    out = []
    # short sequences over {0, 1}: the max(1, .) totals and orders longer than a side
    hl = [a for a in range(6) for _ in (0, 1, 3, 4, 5)]
    rl = [b for _ in range(6) for b in (0, 1, 3, 4, 5)]
    out.append(_case("short", rng.integers(0, 2, size=(30, 5)), rng.integers(0, 2, size=(30, 5)), hyp_len=hl, ref_len=rl))
    # wave boundaries: every hypothesis length against one reference of each length (ref_ld = that length: every CPL instantiation and switch point)
    hyp = rng.integers(0, 3, size=(len(WAVE_HYP_LENS), max(WAVE_HYP_LENS)))
    hyp[::2] = hyp[::2] % 2                                         # every other row over two symbols: more repeats
    for Lr in REF_LENS:
        ref = rng.integers(0, 3 if Lr % 2 else 2, size=(1, max(Lr, 1)))
        out.append(_case("wave, ref %d" % Lr, hyp, ref, hyp_len=WAVE_HYP_LENS, ref_len=[0] if Lr == 0 else None, per_ref=len(WAVE_HYP_LENS)))
    # the width limit on both sides
    out.append(_case("limit x limit", rng.integers(0, 3, size=(1, LIMIT)), rng.integers(0, 3, size=(1, LIMIT))))
    # constructed clipping
    the = [0] * 7
    h, hl = _rows([[1] * 7, [1] * 3, the])
    r, rl = _rows([[1] * 3, [1] * 7, [0, 1, 2, 3, 0, 4]])          # "the cat is on the mat"
    c = _case("constructed clipping", h, r, hyp_len=hl, ref_len=rl)
    assert c["stats"][0, :4].tolist() == [3, 2, 1, 0] and c["stats"][1, :4].tolist() == [3, 2, 1, 0] and c["stats"][1, 4:8].tolist() == [3, 2, 1, 1]
    assert c["stats"][2, 0] == 2 and c["stats"][2, 4] == 7
    out.append(c)
    # identical and disjoint pairs
    lens = [0, 1, 2, 3, 4, 5, 64, 65, 152]
    same = rng.integers(0, 3, size=(len(lens), 152))
    out.append(_case("identical", same, same, hyp_len=lens, ref_len=lens))
    out.append(_case("disjoint", same, same + 3, hyp_len=lens, ref_len=lens[::-1]))
    # END at position 0, absent, inside the given length, behind it -- on either side, every combination; IDENTICAL noise behind both sides' END (and
    # an identical pair of tokens in front of it), so an n-gram that ran across a cut would be counted
    noise = rng.integers(0, 2, size=24)
    def side(offset):
        rows = np.stack([noise.copy() for _ in range(4)])
        body = rng.integers(0, 2, size=(4, 24))
        rows[0, 0] = END                                            # at 0
        rows[1, :] = body[1]                                        # absent
        rows[2, :7 + offset] = body[2, :7 + offset]
        rows[2, 5 + offset:7 + offset] = [1, 0]
        rows[2, 7 + offset] = END                                   # inside
        rows[2, 12] = END                                           # the FIRST END cuts
        rows[3, :15] = body[3, :15]
        rows[3, 13:15] = [1, 0]
        rows[3, 15] = END                                           # behind the length given below
        return rows
    hs, rs = side(0), side(2)
    ln = [24, 24, 24, 10]
    both = [(i, j) for i in range(4) for j in range(4)]
    hrows, of = hs[[i for i, _ in both]], [j for _, j in both]
    out.append(_case("END, lengths", hrows, rs, hyp_len=[ln[i] for i, _ in both], ref_len=ln, ref_of=of, id_end=END))
    out.append(_case("END, no lengths", hrows, rs, ref_of=of, id_end=END))
    out.append(_case("END in the rows, no cut", hrows, rs, ref_of=of, id_end=-1))
    # unusual ids next to the ends of both sequences; rows that are all zeros or all -1 behind (and in front of) their lengths, the values a staged
    # window or a DP strip may be padded with
    big = 0x7fffffff
    seqs_h = [[-1, 0, 1, 0, big], [big, big, 0, -1, -1], [V_SENTINEL, 0, 0, 0, V_SENTINEL], [0] * 5, [-1] * 5, [0, 0], [-1], [big] * 6, [0, -1, 0, -1, 0, -1, 0]]
    seqs_r = [[-1, 0, 1, 1, big], [big, 0, -1, -1], [0, 0, V_SENTINEL], [0] * 2, [-1] * 2, [0] * 6, [-1] * 4, [big] * 3, [-1, 0, -1, 0]]
    h0, hl = _rows(seqs_h, 12, 0)
    r0, rl = _rows(seqs_r, 12, 0)
    out.append(_case("unusual ids, zeros behind", h0, r0, hyp_len=hl, ref_len=rl))
    h1, _ = _rows(seqs_h, 12, -1)
    r1, _ = _rows(seqs_r, 12, -1)
    out.append(_case("unusual ids, -1 behind", h1, r1, hyp_len=hl, ref_len=rl))
    # the [B, T, n] layout a sampled decode writes, n = 3, read in place; references in pad_batch_formulas' layout; p / per_ref and an explicit ref_of
    tok = np.array([0, 1])
    B, T, n = 2, 70, 3
    ids = rng.choice(tok, size=(B, T + 2, n))                       # (two steps the decode did not run lie behind T)
    ids[0, 30, 0] = ids[0, 0, 1] = ids[1, 66, 2] = END
    refs, rl = pad_batch_formulas([list(rng.choice(tok, 33)), list(rng.choice(tok, 67))], 5, END)
    geom = (n, (T + 2) * n, 1, n)
    out.append(_case("strided [B, T, n]", ids, refs, geom=geom, T=T, ref_len=rl, per_ref=n, pairs=B * n, id_end=END))
    out.append(_case("strided [B, T, n], ref_of", ids, refs, geom=geom, T=T, ref_len=rl, ref_of=[1, 0, 1, 0, 0, 1], pairs=B * n, id_end=END))
    _assert_clipping_is_exercised(out)
    assert [c["name"] for c in out] == CASE_NAMES
    return out


def named(name):
    return text_cases()[CASE_NAMES.index(name)]


def _assert_clipping_is_exercised(cases):
    """the condition on the matrix: for every order, at least a tenth of the pairs with |h| >= n have clipped matches strictly below the unclipped
    count; an n-gram more frequent in the hypothesis and one more frequent in the reference both occur"""
    have, below, more, fewer = [0] * 4, [0] * 4, False, False
    for c in cases:
        for h, r in c["cut"]:
            prof, m, f = clip_profile(h, r)
            more, fewer = more or m, fewer or f
            for n in range(1, 5):
                if len(h) >= n:
                    have[n - 1] += 1
                    below[n - 1] += prof[n - 1][0] < prof[n - 1][1]
    assert more and fewer
    for n in range(4):
        assert 10 * below[n] >= have[n] > 0, (n + 1, below, have)


def run_text(lib, c, dev=Host, want_stats=True, corpus=None, accumulate=0, lo=0, hi=None):
    """-> (rc, stats, corpus) of one lxo_text_stats call on the pairs [lo, hi) of case c (plain-row cases only when a sub-range is asked for).
    corpus: None for a call without it, else the int64 [14] array the call starts from."""
    hi = c["pairs"] if hi is None else hi
    hyp, hyp_len, ref_of = c["hyp"], c["hyp_len"], c["ref_of"]
    g = c["geom"]
    if (lo, hi) != (0, c["pairs"]):
        assert g[0] == 1 and g[2] == 0 and c["ref_of"] is not None
        hyp, hyp_len, ref_of = hyp[lo * g[1]:], None if hyp_len is None else hyp_len[lo:], ref_of[lo:]
    keep = [dev.up(a) for a in (hyp, hyp_len, c["ref"], c["ref_len"], ref_of)]
    stats = dev.up(np.full((hi - lo, NS), -7, np.int32)) if want_stats else None
    co = None if corpus is None else dev.up(np.asarray(corpus, np.int64).copy())
    rc = lib.lxo_text_stats(dev.ptr(keep[0]), g[0], g[1], g[2], g[3], c["T"], dev.ptr(keep[1]), dev.ptr(keep[2]), c["ref"].shape[0], c["ref"].shape[1],
                            dev.ptr(keep[3]), dev.ptr(keep[4]), c["per_ref"], hi - lo, c["id_end"], dev.ptr(stats), dev.ptr(co), accumulate, dev.stream)
    return rc, dev.down(stats) if want_stats else None, None if co is None else dev.down(co)


def check_text_case(lib, c, dev=Host):
    rc, stats, corpus = run_text(lib, c, dev, corpus=np.full(NC, -7, np.int64))
    assert rc == 0, (c["name"], lib.lxo_last_error())
    bad = np.flatnonzero((stats != c["stats"]).any(1))
    assert not bad.size, (c["name"], bad[:4].tolist(), stats[bad[:4]].tolist(), c["stats"][bad[:4]].tolist())
    assert corpus.dtype == np.int64 and corpus.tolist() == c["corpus"].tolist(), (c["name"], corpus.tolist(), c["corpus"].tolist())
    if c["name"] == "identical":
        for (h, _), row in zip(c["cut"], stats):
            assert row[10] == 0 and row[11] == 1 and all(row[n - 1] == row[3 + n] for n in range(1, 5) if len(h) >= n), row
    if c["name"] == "disjoint":
        assert not stats[:, :4].any() and not stats[:, 11].any()
    return stats, corpus
