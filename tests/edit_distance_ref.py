"""TEST INFRASTRUCTURE: the host reference of lxo_edit_distance and lxo_mrt_candidates -- the project's own levenshtein and truncate_end
(model/evaluation/text.py) and a restatement of Img2SeqModel.mrt_batch's candidate loop -- with the case matrices and the exact checks that
tests/test_edit_distance_sim.py, tests/test_mrt_candidates_sim.py (hipsim) and tests/test_gpu_mrt_device.py (MI355X) share.  Everything is
compared exactly: ints, and cost.tobytes().  The expected values are computed once per process."""
import ctypes
import functools

import numpy as np

from latex_ocr_amd import _abi
from latex_ocr_amd.model.evaluation.text import levenshtein, truncate_end
from latex_ocr_amd.model.utils.text import pad_batch_formulas

LIMIT = _abi.LXO_EDIT_MAX_REF
# one either side of a wave's 64 lanes and of the strip-width switch points of edit_kernel<CPL> (ref_ld 64 | 128 | 256 | 512 | 1024), the decode bound, the limit
REF_LENS = [0, 1, 63, 64, 65, 127, 128, 129, 152, 255, 256, 257, 511, 512, 513, LIMIT]
HYP_LENS = [0, 1, 70, 152, 300]
END = 2                                                            # inside the 3-symbol alphabet {0, 1, 2} where a case cuts; the others pass id_end = -1


class Host(object):
    """numpy arrays handed to the hipsim library as they are"""
    stream = None

    @staticmethod
    def up(a):
        return None if a is None else np.ascontiguousarray(a)

    @staticmethod
    def ptr(a):
        return ctypes.c_void_p(0) if a is None else ctypes.c_void_p(a.ctypes.data)

    @staticmethod
    def down(a):
        return a


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
    dist, cost = [], []
    for p in range(pairs):
        start = (p // geom[0]) * geom[1] + (p % geom[0]) * geom[2]
        row = flat[start:start + max(T - 1, 0) * geom[3] + 1:geom[3]] if T else flat[:0]
        h = _seq(row, T if hyp_len is None else int(hyp_len[p]), id_end)
        g = int(ref_of[p]) if ref_of is not None else p // per_ref
        r = _seq(ref[g], ref.shape[1] if ref_len is None else int(ref_len[g]), id_end)
        d = levenshtein(h, r)
        dist.append(d)
        cost.append(np.float32(d / float(max(len(r), 1))))
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
    return dict(name=name, hyp=flat, geom=geom, T=int(T), hyp_len=i32(hyp_len), ref=ref, ref_len=i32(ref_len), ref_of=i32(ref_of), per_ref=per_ref,
                pairs=pairs, id_end=id_end, dist=np.asarray(dist, np.int32), cost=np.asarray(cost, np.float32))


@functools.lru_cache(maxsize=None)
def edit_cases():
    rng = np.random.default_rng(11)
    out = []
    Tm = max(HYP_LENS)
    hyp = rng.integers(0, 3, size=(len(HYP_LENS), Tm))
    for Lr in REF_LENS:                                             # every hypothesis length against one reference of each length
        ref = rng.integers(0, 3, size=(1, max(Lr, 1)))
        out.append(_case("ref %d" % Lr, hyp, ref, hyp_len=HYP_LENS, ref_len=[0] if Lr == 0 else None, per_ref=len(HYP_LENS)))
    # the other order: hypotheses of the reference lengths (no limit on that side) against references of the hypothesis lengths, an explicit ref_of
    hyp2 = rng.integers(0, 3, size=(len(REF_LENS), LIMIT))
    ref2 = rng.integers(0, 3, size=(len(HYP_LENS), Tm))
    pairs = [(i, (i + k) % len(HYP_LENS)) for i in range(len(REF_LENS)) for k in (0, 2)]
    out.append(_case("swapped", hyp2[[i for i, _ in pairs]], ref2, hyp_len=[REF_LENS[i] for i, _ in pairs], ref_len=HYP_LENS, ref_of=[g for _, g in pairs]))
    # identical pairs (0) and disjoint pairs (the longer length)
    lens = [0, 1, 64, 65, 152]
    same = rng.integers(0, 3, size=(len(lens), 152))
    out.append(_case("identical", same, same, hyp_len=lens, ref_len=lens))
    out.append(_case("disjoint", same, same + 3, hyp_len=lens, ref_len=lens[::-1]))
    # END at position 0, absent, inside the given length, behind it -- on either side; the lengths given and not
    tok = np.array([0, 1])
    rows = np.stack([rng.choice(tok, 20) for _ in range(4)])
    rows[0, 0] = END
    rows[2, 7] = END
    rows[2, 12] = END                                              # the FIRST END cuts
    rows[3, 15] = END
    ln = [20, 20, 20, 10]                                          # row 3: the length cuts in front of its END
    order = [1, 2, 3, 0]
    out.append(_case("END, lengths", rows, rows[order], hyp_len=ln, ref_len=[ln[i] for i in order], id_end=END))
    out.append(_case("END, no lengths", rows, rows[order], id_end=END))
    out.append(_case("END in the rows, no cut", rows, rows[order], id_end=-1))
    # the [B, T, n] layout a sampled decode writes, n = 3, read in place; references in pad_batch_formulas' layout; p / per_ref
    B, T, n = 2, 40, 3
    ids = rng.choice(tok, size=(B, T + 2, n))                       # (two steps the decode did not run lie behind T)
    ids[0, 30, 0] = ids[0, 0, 1] = ids[1, 17, 2] = END
    refs, rl = pad_batch_formulas([list(rng.choice(tok, 33)), list(rng.choice(tok, 9))], 5, END)
    out.append(_case("strided [B, T, n]", ids, refs, geom=(n, (T + 2) * n, 1, n), T=T, ref_len=rl, per_ref=n, pairs=B * n, id_end=END))
    return out


def run_edit(lib, c, dev=Host, want_cost=True):
    """-> (rc, dist, cost) of one lxo_edit_distance call on case c"""
    keep = [dev.up(c[k]) for k in ("hyp", "hyp_len", "ref", "ref_len", "ref_of")]
    dist = dev.up(np.full(c["pairs"], -7, np.int32))
    cost = dev.up(np.full(c["pairs"], -7, np.float32)) if want_cost else None
    g = c["geom"]
    rc = lib.lxo_edit_distance(dev.ptr(keep[0]), g[0], g[1], g[2], g[3], c["T"], dev.ptr(keep[1]), dev.ptr(keep[2]), c["ref"].shape[0], c["ref"].shape[1],
                               dev.ptr(keep[3]), dev.ptr(keep[4]), c["per_ref"], c["pairs"], c["id_end"], dev.ptr(dist), dev.ptr(cost), dev.stream)
    return rc, dev.down(dist), dev.down(cost) if want_cost else None


def check_edit_case(lib, c, dev=Host):
    rc, dist, cost = run_edit(lib, c, dev)
    assert rc == 0, (c["name"], lib.lxo_last_error())
    assert np.array_equal(dist, c["dist"]), (c["name"], dist.tolist(), c["dist"].tolist())
    assert cost.tobytes() == c["cost"].tobytes(), (c["name"], cost.tolist(), c["cost"].tolist())
    if c["name"] == "identical":
        assert not dist.any() and not cost.any()
    if c["name"] == "disjoint":
        assert dist.tolist() == [max(a, b) for a, b in zip(c["hyp_len"], c["ref_len"][:len(dist)])]


# ---------------------------------------------------------------------------------------------------------------- candidates --
def host_candidates(ids, refs, id_end, id_pad, include_reference):
    """Img2SeqModel.mrt_batch's loop on ids [B, steps, n] and token-id references -> (cand [rows, T], lengths, group sizes, cost f32)"""
    cands, sizes, costs = [], [], []
    for b, ref in enumerate(refs):
        ref = tuple(int(x) for x in ref)
        mine = [ref] if include_reference else []
        for j in range(ids.shape[2]):
            c = tuple(int(x) for x in truncate_end(ids[b, :, j], id_end))
            if c not in mine:
                mine.append(c)
        cands += mine
        sizes.append(len(mine))
        costs += [levenshtein(c, ref) / float(max(len(ref), 1)) for c in mine]
    f, ln = pad_batch_formulas([list(c) for c in cands], id_pad, id_end)
    return f, ln, np.asarray(sizes), np.asarray(costs, np.float32)


CAND_END, CAND_PAD = 9, 8
CAND_REFS = [[1, 2, 3], [4], [5, 6, 7, 1, 2]]


def constructed_ids():
    """ids int32 [B = 3, max_steps = 8, n = 4]: image 0: two draws equal, one equal to the reference, one with no END in the first 6 steps;
    image 1: all draws equal; image 2: two draws that are END at step 0, one of its own, one equal to the reference.  Behind a draw's END, and
    behind the steps a call passes, lies noise that nothing may read."""
    E = CAND_END
    draws = [[[1, 2, E], [1, 2, E, 3], [1, 2, 3, E], [3, 3, 1, 2, 1, 1, E]],
             [[4, 4, E]] * 4,
             [[E, 5], [E, 6, E], [5, 6, E], [5, 6, 7, 1, 2, E]]]
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 8, size=(3, 8, 4)).astype(np.int32)
    for b, ds in enumerate(draws):
        for j, d in enumerate(ds):
            ids[b, :len(d), j] = d
    return ids


def cand_calls():
    """(steps, include_reference): 6 steps -- every case of constructed_ids() as described, Tc = 7 > Tr; 2 steps -- the draws cut to two
    tokens without END (other draws fall together), Tc = Tr = 6"""
    return [(6, 1), (6, 0), (2, 1), (2, 0)]


def run_candidates(lib, ids, steps, refs, id_end, id_pad, inc, dev=Host):
    """-> (rc, cand [R, Tc], cand_len, cost, group_off, row_image) of one lxo_mrt_candidates call"""
    B, max_steps, n = ids.shape
    ref, ref_len = pad_batch_formulas([list(r) for r in refs], id_pad, id_end)
    Tr = ref.shape[1]
    R, Tc = B * (n + inc), max(steps + 1, Tr)
    keep = [dev.up(np.ascontiguousarray(ids, np.int32)), dev.up(ref), dev.up(ref_len)]
    outs = [dev.up(np.full(s, -7, t)) for s, t in (((R, Tc), np.int32), (R, np.int32), (R, np.float32), (B + 1, np.int32), (R, np.int32))]
    rc = lib.lxo_mrt_candidates(dev.ptr(keep[0]), B, max_steps, n, steps, dev.ptr(keep[1]), Tr, dev.ptr(keep[2]), id_end, id_pad, inc,
                                *([dev.ptr(o) for o in outs] + [dev.stream]))
    return (rc,) + tuple(dev.down(o) for o in outs)


def check_candidates(ids, steps, refs, id_end, id_pad, inc, cand, cand_len, cost, group_off, row_image):
    """the device's candidate rows against host_candidates, exactly -> the group sizes"""
    f, ln, sizes, costs = host_candidates(ids[:, :steps], refs, id_end, id_pad, bool(inc))
    live = int(sizes.sum())
    assert group_off.tolist() == [0] + np.cumsum(sizes).tolist(), (group_off, sizes)
    assert cand_len[:live].tolist() == ln.tolist()
    assert row_image[:live].tolist() == np.repeat(np.arange(len(sizes)), sizes).tolist()
    assert cost[:live].tobytes() == costs.tobytes(), (cost[:live], costs)
    for r in range(live):
        assert cand[r, :ln[r]].tolist() == f[r, :ln[r]].tolist(), (r, cand[r], f[r])
        assert (cand[r, ln[r]:] == id_pad).all(), (r, cand[r])
    # the dead rows behind the last group
    assert (cand[live:] == id_pad).all() and not cand_len[live:].any() and not row_image[live:].any()
    assert cost[live:].tobytes() == np.zeros(len(cost) - live, np.float32).tobytes()
    return sizes
