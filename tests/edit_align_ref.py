"""TEST INFRASTRUCTURE: the host reference of lxo_edit_align -- a full Levenshtein table of plain integers walked back with the three rules of
include/lxo.h, written independently of model/evaluation/text.py's align -- with the case matrix, the runner and the exact checks that
tests/test_edit_align_sim.py (hipsim), tests/test_engine_edit_align_sim.py and tests/test_gpu_edit_align.py (MI355X) share.  Everything is compared
as integers.  The expected values are computed once per process and never changed."""
import functools

import numpy as np

from latex_ocr_amd import _abi
from latex_ocr_amd.model.evaluation.text import levenshtein, truncate_end
from latex_ocr_amd.model.utils.text import pad_batch_formulas
from edit_distance_ref import HYP_LENS, REF_LENS, Host

LIMIT = _abi.LXO_EDIT_MAX_REF
NA, NC = _abi.LXO_ALIGN_COUNTS, _abi.LXO_ALIGN_CORPUS
END = 2                                                            # inside the alphabet where a case cuts; the others pass id_end = -1
GUARD = 8                                                          # words of -7 in front of and behind every output
CASE_NAMES = (["ref %d" % L for L in REF_LENS] + ["swapped", "limit x limit", "exhaustive small", "all equal", "identical", "disjoint", "END, lengths",
              "END, no lengths", "END in the rows, no cut", "strided [B, T, n]", "strided [B, T, n], ref_of", "tokens outside [0, V)", "V = 1"])


def table(h, r):
    """D[i][j], the Levenshtein table of h[:i] against r[:j], int64 [m + 1, n + 1]; a row from the row above: t = what a cell gets from above and
    above-left, then the run from the left as a running minimum of t[k] - k"""
    m, n = len(h), len(r)
    D = np.zeros((m + 1, n + 1), np.int64)
    cols = np.arange(n + 1, dtype=np.int64)
    D[0] = cols
    ra = np.asarray(r, np.int64)
    for i in range(1, m + 1):
        t = np.empty(n + 1, np.int64)
        t[0] = i
        t[1:] = np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (ra != int(h[i - 1])))
        D[i] = cols + np.minimum.accumulate(t - cols)
    return D


def align_ref(h, r):
    """-> (hyp_align, ref_align, [M, S, I, D, |h|, |r|]): the canonical path from (m, n), at every cell the first rule that applies"""
    h, r = [int(x) for x in h], [int(x) for x in r]
    D = table(h, r).tolist()
    i, j = len(h), len(r)
    ha, ra = [-1] * i, [-1] * j
    M = S = I = Dl = 0
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + (1 if h[i - 1] != r[j - 1] else 0):
            if h[i - 1] == r[j - 1]:
                M += 1
            else:
                S += 1
            ha[i - 1], ra[j - 1] = j - 1, i - 1
            i, j = i - 1, j - 1
        elif i > 0 and D[i][j] == D[i - 1][j] + 1:
            I += 1
            i -= 1
        else:
            assert j > 0 and D[i][j] == D[i][j - 1] + 1
            Dl += 1
            j -= 1
    return ha, ra, [M, S, I, Dl, len(h), len(r)]


def check_valid(h, r, ha, ra, counts, dist=None):
    """what holds for ANY optimal alignment, whatever the tie-break: ha / ra are the maps cut to the sequences"""
    m, n = len(h), len(r)
    ha, ra = [int(x) for x in ha], [int(x) for x in ra]
    assert len(ha) == m and len(ra) == n
    assert all(-1 <= x < n for x in ha) and all(-1 <= x < m for x in ra)
    up = [x for x in ha if x >= 0]
    assert all(a < b for a, b in zip(up, up[1:])), ha
    up = [x for x in ra if x >= 0]
    assert all(a < b for a, b in zip(up, up[1:])), ra
    assert all(ra[j] == i for i, j in enumerate(ha) if j >= 0) and all(ha[i] == j for j, i in enumerate(ra) if i >= 0)
    M, S, I, Dl, lh, lr = [int(x) for x in counts]
    assert (lh, lr) == (m, n) and M + S + I == m and M + S + Dl == n
    assert M == sum(1 for i, j in enumerate(ha) if j >= 0 and h[i] == r[j]) and I == ha.count(-1) and Dl == ra.count(-1)
    assert S + I + Dl == (levenshtein(h, r) if dist is None else dist)


def confusion_of(cut, maps, V):
    """-> (int64 [(V + 1)^2], steps left out): every alignment step entered, tokens outside [0, V) left out"""
    C = np.zeros((V + 1, V + 1), np.int64)
    out = 0
    ok = lambda x: 0 <= x < V
    for (h, r), (ha, ra) in zip(cut, maps):
        for i, j in enumerate(ha):
            a = V if j < 0 else r[j]
            if ok(h[i]) and (j < 0 or ok(a)):
                C[a, h[i]] += 1
            else:
                out += 1
        for j, i in enumerate(ra):
            if i < 0:
                if ok(r[j]):
                    C[r[j], V] += 1
                else:
                    out += 1
    return C.reshape(-1), out


def corpus_of(counts, out=0):
    c = np.asarray(counts, np.int64).reshape(-1, NA)
    return np.concatenate([c.sum(0), [c.shape[0], out]]).astype(np.int64)


def _seq(row, length, id_end):
    row = [int(x) for x in row[:length]]
    return truncate_end(row, id_end) if id_end >= 0 else row


def _case(name, hyp, ref, geom=None, T=None, hyp_len=None, ref_len=None, ref_of=None, per_ref=1, pairs=None, id_end=-1, V=3):
    """geom = (hyp_block, block_stride, row_stride, tok_stride), None: plain rows [pairs, T]"""
    hyp, ref = np.ascontiguousarray(hyp, np.int32), np.ascontiguousarray(ref, np.int32)
    if geom is None:
        pairs, T = hyp.shape
        geom = (1, T, 0, 1)
    flat = hyp.reshape(-1)
    ld = ref.shape[1]
    HA, RA = np.full((pairs, T), -2, np.int32), np.full((pairs, ld), -2, np.int32)
    counts, cut, maps = [], [], []
    for p in range(pairs):
        start = (p // geom[0]) * geom[1] + (p % geom[0]) * geom[2]
        row = flat[start:start + max(T - 1, 0) * geom[3] + 1:geom[3]] if T else flat[:0]
        h = _seq(row, T if hyp_len is None else int(hyp_len[p]), id_end)
        g = int(ref_of[p]) if ref_of is not None else p // per_ref
        r = _seq(ref[g], ld if ref_len is None else int(ref_len[g]), id_end)
        ha, ra, c = align_ref(h, r)
        # (the Python levenshtein on the small pairs; the wide ones have the table's own corner, which lxo_edit_distance is held against as well)
        check_valid(h, r, ha, ra, c, dist=None if len(h) * len(r) <= 40000 else sum(c[1:4]))
        HA[p, :len(h)], RA[p, :len(r)] = ha, ra
        counts.append(c)
        cut.append((h, r))
        maps.append((ha, ra))
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
    counts = np.asarray(counts, np.int32).reshape(pairs, NA)
    conf, out = confusion_of(cut, maps, V)
    return dict(name=name, hyp=flat, geom=geom, T=int(T), hyp_len=i32(hyp_len), ref=ref, ref_len=i32(ref_len), ref_of=i32(ref_of), per_ref=per_ref,
                pairs=pairs, id_end=id_end, V=V, hyp_align=HA, ref_align=RA, counts=counts, corpus=corpus_of(counts, out), confusion=conf, cut=cut, maps=maps)


def _rows(seqs, width=None, fill=0):
    width = max([len(s) for s in seqs] + [1]) if width is None else width
    out = np.full((len(seqs), width), fill, np.int64)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out, [len(s) for s in seqs]


@functools.lru_cache(maxsize=None)
def align_cases():
    rng = np.random.default_rng(31)
    out = []
    # alphabets {0, 1, 2} and {0, 1}: ties are the rule.  Every hypothesis length against one reference of each length (ref_ld = that length: every
    # strip width and switch point)
    Tm = max(HYP_LENS)
    hyp = rng.integers(0, 3, size=(len(HYP_LENS), Tm))
    for k, Lr in enumerate(REF_LENS):
        ref = rng.integers(0, 3 if k % 2 else 2, size=(1, max(Lr, 1)))
        out.append(_case("ref %d" % Lr, hyp % 2 if k % 4 == 0 else hyp, ref, hyp_len=HYP_LENS, ref_len=[0] if Lr == 0 else None, per_ref=len(HYP_LENS)))
    # the other order: hypotheses of the reference lengths, up to the limit, against references of the hypothesis lengths; an explicit ref_of
    hyp2 = rng.integers(0, 2, size=(len(REF_LENS), LIMIT))
    ref2 = rng.integers(0, 2, size=(len(HYP_LENS), Tm))
    pairs = [(i, (i + k) % len(HYP_LENS)) for i in range(len(REF_LENS)) for k in (0, 2)]
    out.append(_case("swapped", hyp2[[i for i, _ in pairs]], ref2, hyp_len=[REF_LENS[i] for i, _ in pairs], ref_len=HYP_LENS, ref_of=[g for _, g in pairs]))
    out.append(_case("limit x limit", rng.integers(0, 3, size=(1, LIMIT)), rng.integers(0, 3, size=(1, LIMIT))))
    # all 31 x 31 pairs of sequences over {0, 1} of length 0 .. 4: every tie pattern the rule can meet
    seqs = [[(v >> k) & 1 for k in range(L)] for L in range(5) for v in range(1 << L)]
    assert len(seqs) == 31
    rows, ln = _rows(seqs, 4)
    both = [(i, j) for i in range(31) for j in range(31)]
    c = _case("exhaustive small", rows[[i for i, _ in both]], rows, hyp_len=[ln[i] for i, _ in both], ref_len=ln, ref_of=[j for _, j in both], V=2)
    assert c["pairs"] == 961
    out.append(c)
    # all tokens equal, unequal lengths: every path ties and the rule leaves the surplus at the front
    la, lb = [5, 2, 70, 64, 0, 130], [2, 5, 64, 70, 3, 1]
    c = _case("all equal", np.zeros((6, 130)), np.zeros((6, 70)), hyp_len=la, ref_len=lb)
    for p, (a, b) in enumerate(zip(la, lb)):
        assert c["hyp_align"][p, :a].tolist() == [-1] * max(a - b, 0) + list(range(max(b - a, 0), b))
        assert c["ref_align"][p, :b].tolist() == [-1] * max(b - a, 0) + list(range(max(a - b, 0), a))
    out.append(c)
    lens = [0, 1, 64, 65, 152]
    same = rng.integers(0, 3, size=(len(lens), 152))
    c = _case("identical", same, same, hyp_len=lens, ref_len=lens)
    assert c["counts"][:, 0].tolist() == lens and not c["counts"][:, 1:4].any()
    out.append(c)
    c = _case("disjoint", same, same + 3, hyp_len=lens, ref_len=lens[::-1], V=6)
    assert not c["counts"][:, 0].any()
    out.append(c)
    # END at position 0, absent, inside the given length, behind it -- on either side, every combination
    def side(offset):
        rows = rng.integers(0, 2, size=(4, 24))
        rows[0, 0] = END
        rows[2, 7 + offset] = END
        rows[2, 12] = END                                          # the FIRST END cuts
        rows[3, 15] = END                                          # behind the length given below
        return rows
    hs, rs = side(0), side(2)
    ln = [24, 24, 24, 10]
    both = [(i, j) for i in range(4) for j in range(4)]
    hrows, of = hs[[i for i, _ in both]], [j for _, j in both]
    out.append(_case("END, lengths", hrows, rs, hyp_len=[ln[i] for i, _ in both], ref_len=ln, ref_of=of, id_end=END))
    out.append(_case("END, no lengths", hrows, rs, ref_of=of, id_end=END))
    out.append(_case("END in the rows, no cut", hrows, rs, ref_of=of, id_end=-1))
    # the [B, T, n] layout a sampled decode writes, n = 3, read in place; references in pad_batch_formulas' layout; p / per_ref and an explicit ref_of
    tok = np.array([0, 1])
    B, T, n = 2, 70, 3
    ids = rng.choice(tok, size=(B, T + 2, n))                       # (two steps the decode did not run lie behind T)
    ids[0, 30, 0] = ids[0, 0, 1] = ids[1, 66, 2] = END
    refs, rl = pad_batch_formulas([list(rng.choice(tok, 33)), list(rng.choice(tok, 67))], 5, END)
    geom = (n, (T + 2) * n, 1, n)
    out.append(_case("strided [B, T, n]", ids, refs, geom=geom, T=T, ref_len=rl, per_ref=n, pairs=B * n, id_end=END))
    out.append(_case("strided [B, T, n], ref_of", ids, refs, geom=geom, T=T, ref_len=rl, ref_of=[1, 0, 1, 0, 0, 1], pairs=B * n, id_end=END))
    # tokens outside [0, V) and negative ids: counted, left out of the confusion, reported in corpus[7]
    big = 0x7fffffff
    seqs_h = [[-1, 0, 1, 0, big], [big, big, 0, -1, -1], [4, 0, 0, 0, 500], [0, 1, 2, 3], [-1] * 5, [3, 3], [4], [0, -1, 0, -1, 0, -1, 0]]
    seqs_r = [[-1, 0, 1, 1, big], [big, 0, -1, -1], [0, 0, 4], [3, 2, 1, 0, 3], [-1] * 2, [0] * 6, [4, 4], [-1, 0, -1, 0]]
    h0, hl = _rows(seqs_h, 9, -1)
    r0, rl = _rows(seqs_r, 9, 0)
    c = _case("tokens outside [0, V)", h0, r0, hyp_len=hl, ref_len=rl, V=4)
    assert c["corpus"][7] > 0 and c["confusion"].sum() == c["corpus"][:4].sum() - c["corpus"][7] > 0
    out.append(c)
    # V = 1: one token and "no token"
    c = _case("V = 1", rng.integers(0, 2, size=(6, 9)), rng.integers(0, 2, size=(6, 7)), hyp_len=[9, 0, 4, 9, 1, 7], ref_len=[7, 7, 0, 3, 7, 7], V=1)
    assert c["corpus"][7] > 0 and c["confusion"][3] == 0
    out.append(c)
    assert [c["name"] for c in out] == CASE_NAMES
    for c in out:
        assert c["confusion"][-1] == 0 and c["confusion"].sum() == c["corpus"][:4].sum() - c["corpus"][7]
    return out


def named(name):
    return align_cases()[CASE_NAMES.index(name)]


def _guarded(dev, shape, dtype, start=None):
    """an output of `shape` between GUARD words of -7 on either side: -> (buffer, words); start: what the output holds before the call"""
    size = int(np.prod(shape))
    a = np.full(size + 2 * GUARD, -7, dtype)
    if start is not None:
        a[GUARD:GUARD + size] = np.asarray(start, dtype).reshape(-1)
    return dev.up(a), size


def run_align(lib, c, dev=Host, want=("hyp_align", "ref_align", "counts"), corpus=None, confusion=None, accumulate=0, lo=0, hi=None, scratch="exact"):
    """One lxo_edit_align call on the pairs [lo, hi) of case c (a sub-range on plain rows with a ref_of only) -> (rc, dict of the outputs asked for).
    corpus / confusion: None for a call without it, else what the call starts from.  Every output lies between guard words and the scratch has the
    size the size function states with guard bytes behind it: both are checked after a call that returned 0 and after one that refused."""
    hi = c["pairs"] if hi is None else hi
    hyp, hyp_len, ref_of = c["hyp"], c["hyp_len"], c["ref_of"]
    g, T, ld, V, n = c["geom"], c["T"], c["ref"].shape[1], c["V"], hi - lo
    if (lo, hi) != (0, c["pairs"]):
        assert g[0] == 1 and g[2] == 0 and c["ref_of"] is not None
        hyp, hyp_len, ref_of = hyp[lo * g[1]:], None if hyp_len is None else hyp_len[lo:], ref_of[lo:]
    keep = [dev.up(a) for a in (hyp, hyp_len, c["ref"], c["ref_len"], ref_of)]
    shapes = {"hyp_align": ((n, T), np.int32, None), "ref_align": ((n, ld), np.int32, None), "counts": ((n, NA), np.int32, None)}
    if corpus is not None:
        shapes["corpus"] = ((NC,), np.int64, corpus)
    if confusion is not None:
        shapes["confusion"] = (((V + 1) * (V + 1),), np.int64, confusion)
    bufs = {k: _guarded(dev, *shapes[k]) for k in shapes if k in want or k in ("corpus", "confusion")}
    arg = lambda k: dev.ptr(bufs[k][0][GUARD:GUARD + bufs[k][1]]) if k in bufs and bufs[k][1] else dev.ptr(bufs[k][0][GUARD:]) if k in bufs else dev.ptr(None)
    need = int(lib.lxo_edit_align_scratch_bytes(n, T, ld))
    assert 0 <= need <= n * T * 256
    nbytes = need if scratch == "exact" else scratch
    sc = dev.up(np.full(max(nbytes, 0) + 64, 0xF9, np.uint8))
    rc = lib.lxo_edit_align(dev.ptr(keep[0]), g[0], g[1], g[2], g[3], T, dev.ptr(keep[1]), dev.ptr(keep[2]), c["ref"].shape[0], ld, dev.ptr(keep[3]),
                            dev.ptr(keep[4]), c["per_ref"], n, c["id_end"], arg("hyp_align"), arg("ref_align"), arg("counts"), arg("corpus"), arg("confusion"),
                            V, accumulate, dev.ptr(sc), max(nbytes, 0), dev.stream)
    got = {}
    for k, (buf, size) in bufs.items():
        a = dev.down(buf)
        assert (a[:GUARD] == -7).all() and (a[GUARD + size:] == -7).all(), (c["name"], k, "guard words")
        got[k] = a[GUARD:GUARD + size].reshape(shapes[k][0])
    assert (dev.down(sc)[max(nbytes, 0):] == 0xF9).all(), (c["name"], "bytes behind the scratch")
    return rc, got


def check_align_case(lib, c, dev=Host):
    """the whole case, exact: maps, counts, corpus, confusion; the validity checks on what the kernel wrote"""
    V = c["V"]
    rc, got = run_align(lib, c, dev, corpus=np.full(NC, -7, np.int64), confusion=np.full((V + 1) * (V + 1), -7, np.int64))
    assert rc == 0, (c["name"], lib.lxo_last_error())
    for k in ("hyp_align", "ref_align", "counts"):
        bad = np.flatnonzero((got[k] != c[k]).any(1))
        assert not bad.size, (c["name"], k, bad[:4].tolist(), got[k][bad[:2]].tolist(), c[k][bad[:2]].tolist())
    assert got["corpus"].dtype == np.int64 and got["corpus"].tolist() == c["corpus"].tolist(), (c["name"], got["corpus"].tolist(), c["corpus"].tolist())
    assert got["confusion"].tolist() == c["confusion"].tolist(), (c["name"], got["confusion"].tolist(), c["confusion"].tolist())
    assert got["confusion"].sum() == got["corpus"][:4].sum() - got["corpus"][7]
    for p, (h, r) in enumerate(c["cut"]):
        assert (got["hyp_align"][p, len(h):] == -2).all() and (got["ref_align"][p, len(r):] == -2).all()
        check_valid(h, r, got["hyp_align"][p, :len(h)], got["ref_align"][p, :len(r)], got["counts"][p], dist=int(c["counts"][p, 1:4].sum()))
    return got
