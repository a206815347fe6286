"""CPU (hipsim): lxo_grammar_step -- the two grammar kernels alone, on ids the test holds -- bit for bit against latex_ocr_amd.grammar.Grammar:
the sets S_0 / S_{t + 1} (every word, pad bits included) and the depths, over vocabulary sizes at the word edges, 1 to 5 rows, one and
fifteen kinds, walks that push to depth D and past it, close the wrong kind, close at depth 0, run into the budget (r == d, r == d + 1),
finish rows, and permute / duplicate beam parents; with and without the budget and a static set shared (allow_ld 0) or per image."""
import ctypes

import numpy as np
import pytest

from latex_ocr_amd import _abi
from latex_ocr_amd.grammar import Grammar
from simharness import lib
from simlib import ptr
import constraint_ref


def table(V, n_kinds):
    """token v in 1 .. V - 2: plain where v % 5 == 0, else an opener (v odd) or closer (v even) of kind ((v - 1) // 2) % n_kinds + 1"""
    c = np.zeros(V, np.int8)
    for v in range(1, V - 1):
        if v % 5:
            c[v] = (1 if v & 1 else -1) * (((v - 1) // 2) % n_kinds + 1)
    return c


class Dev(object):
    """the device side of one walk: lxo_grammar_step on numpy buffers"""

    def __init__(self, g, rows, k, V, end, max_iter, allow, ld):
        self.L = lib()
        self.g, self.rows, self.k, self.V, self.end, self.max_iter = g, rows, k, V, end, max_iter
        self.W = (V + 31) // 32
        self.cls = np.ascontiguousarray(g.cls)
        self.gs = _abi.LxoGrammar(ptr(self.cls), g.n_kinds, g.max_depth, 1 if g.budget else 0)
        nb = self.L.lxo_grammar_scratch_bytes(rows, V)
        assert nb > 0 and nb % 4 == 0
        self.scratch = np.full(nb // 4 + 8, 0xDEADBEEF, np.uint32)          # the set-up launch owes nothing to what the scratch held
        self.allow = None if allow is None else constraint_ref.pack_bits(allow, ld if ld else None)
        self.ld = ld

    def call(self, ids, parents, finished, time):
        sets = np.full((self.rows, self.W), 0xFFFFFFFF, np.uint32)
        depth = np.full(self.rows, -7, np.int32)
        rc = self.L.lxo_grammar_step(ctypes.byref(self.gs), self.rows, self.k, self.V, self.end, ptr(ids), ptr(parents), ptr(finished), time,
                                     self.max_iter, ptr(self.allow), self.ld, ptr(sets), ptr(depth), ptr(self.scratch), None)
        assert rc == 0, self.L.lxo_last_error()
        assert (self.scratch[-8:] == 0xDEADBEEF).all()                      # nothing written behind lxo_grammar_scratch_bytes
        return sets, depth


def run_walk(rng, V, rows, k, n_kinds, D, budget, max_iter, allow_mode, hits, script=None):
    end = V - 1
    g = Grammar(table(V, n_kinds), max_depth=D, budget=budget, id_end=end)
    images = rows // k
    if allow_mode == "none":
        A, allow, ld = np.ones((images, V), bool), None, 0
    else:
        A = rng.rand(1 if allow_mode == "shared" else images, V) < 0.7
        A[:, end] = True
        A[:, g.cls < 0] = True                                              # the contract: END and every closer stay allowed
        allow, ld = A, (0 if allow_mode == "shared" else (V + 31) // 32 + (1 if V == 33 else 0))      # once with rows longer than the words used
        A = np.broadcast_to(A, (images, V))
    dev = Dev(g, rows, k, V, end, max_iter, allow, ld)
    state = [() for _ in range(rows)]
    fin = np.zeros(rows, np.int32)

    def want_sets(t):
        return constraint_ref.pack_bits(np.stack([A[r // k] if fin[r] else A[r // k] & g.allowed_at(state[r], t, max_iter) for r in range(rows)]))

    sets, _ = dev.call(None, None, None, 0)
    assert np.array_equal(sets, want_sets(0)), (V, rows, "S_0")
    for t in range(max_iter + 1):
        ids = np.zeros(rows, np.int32)
        par = np.arange(rows, dtype=np.int32) % k
        if k > 1 and t > 0:
            par = rng.randint(0, k, size=rows).astype(np.int32)             # permutes and duplicates slots
            if len(set(par[:k].tolist())) < k:
                hits.add("duplicate parent")
            if (par != np.arange(rows) % k).any():
                hits.add("permuted parent")
        old, old_fin = list(state), fin.copy()
        for r in range(rows):
            src = (r // k) * k + int(par[r]) if k > 1 else r
            s = old[src]
            ok = g.allowed_at(s, t, max_iter)
            d, left = len(s), max_iter - t
            if script is not None:
                tok = script(r, t, s)
            elif rng.rand() < 0.6 and (ok & A[r // k]).any():
                tok = int(rng.choice(np.nonzero(ok & A[r // k])[0]))
            else:
                tok = int(rng.randint(0, V))
            f = int(old_fin[src]) | (1 if tok == end and rng.rand() < 0.8 else 0)      # (a forced END would leave the row unfinished)
            c = int(g.cls[tok])
            if not f:
                if c > 0 and d == D:
                    hits.add("opener at depth D")
                if c > 0 and d == D - 1:
                    hits.add("depth D reached")
                if c < 0 and d > 0 and s[-1] != -c:
                    hits.add("mismatched closer")
                if c < 0 and d == 0:
                    hits.add("closer at depth 0")
                if budget and left == d:
                    hits.add("r == d")
                if budget and left == d + 1:
                    hits.add("r == d + 1")
            else:
                hits.add("finished row")
            ids[r], fin[r] = tok, f
            state[r] = s if f else g.apply(s, tok)
        sets, depth = dev.call(ids, par if k > 1 else None, fin, t)
        assert depth.tolist() == [len(s) for s in state], (V, rows, t)
        assert np.array_equal(sets, want_sets(t + 1)), (V, rows, t)
        if V & 31:
            assert not (sets[:, -1] >> np.uint32(V & 31)).any()            # pad bits 0, also in a finished row's S = A


@pytest.mark.parametrize("n_kinds", [1, 15])
def test_grammar_step_equals_the_host_model(n_kinds):
    rng = np.random.RandomState(100 + n_kinds)
    hits = set()
    for V in (11, 32, 33, 64, 65, 500):
        for rows in (1, 2, 3, 4, 5):
            for k in sorted({1, rows}):                                     # independent rows, and one image whose `rows` slots swap parents
                for budget, D, mode in ((True, 2, "none"), (True, 3, "image"), (False, 2, "shared")):
                    run_walk(rng, V, rows, k, n_kinds, D, budget, 9, mode, hits)
    want = {"opener at depth D", "depth D reached", "mismatched closer", "closer at depth 0", "r == d", "r == d + 1", "finished row",
            "duplicate parent", "permuted parent"}
    if n_kinds == 1:
        want.discard("mismatched closer")                                   # one kind: every closer matches
    assert want <= hits, want - hits


def test_the_full_depth_and_one_past_it():
    """D = 32: a row that only opens reaches depth 32 and stays there; closing pops the kinds in reverse order, all four stack words"""
    V, D = 65, 32
    opener = lambda kind: 2 * kind - 1                                      # table(): token 2 q - 1 opens kind q, 2 q closes it
    kinds = [1, 2, 4, 6, 7, 9, 11, 12, 14]                                  # (the kinds neither of whose two tokens is a multiple of 5: plain)
    cls = table(V, 15)
    assert all(cls[opener(q)] == q and cls[opener(q) + 1] == -q for q in kinds)
    seq = [kinds[i % len(kinds)] for i in range(D)]

    def script(r, t, s):
        if t < D + 2:
            return opener(seq[t % D])                                       # steps 32 and 33: an opener at depth D
        return opener(s[-1]) + 1 if s else 0                                # then the matching closers
    hits = set()
    run_walk(np.random.RandomState(0), V, 2, 1, 15, D, False, 2 * D + 3, "none", hits, script)
    assert "opener at depth D" in hits and "depth D reached" in hits


def test_refusals_before_any_launch():
    L = lib()
    V, rows = 33, 2
    cls = table(V, 2)
    scratch = np.zeros(L.lxo_grammar_scratch_bytes(rows, V) // 4, np.uint32)
    keep = scratch.copy()
    ids = np.zeros(rows, np.int32); fin = np.zeros(rows, np.int32)
    allow = np.full((rows, 2), 0xFFFFFFFF, np.uint32)

    def call(gs=None, rows_=rows, k=1, V_=V, ids_=ids, fin_=fin, time=0, max_iter=5, allow_=None, ld=0, scratch_=scratch, g_null=False):
        gs = _abi.LxoGrammar(ptr(cls), 2, 4, 1) if gs is None else gs
        return L.lxo_grammar_step(None if g_null else ctypes.byref(gs), rows_, k, V_, V_ - 1, ptr(ids_), None, ptr(fin_), time, max_iter,
                                  ptr(allow_), ld, None, None, ptr(scratch_), None)

    assert call() == 0
    scratch[:] = keep
    for kw in (dict(g_null=True), dict(gs=_abi.LxoGrammar(None, 2, 4, 1)), dict(gs=_abi.LxoGrammar(ptr(cls), 0, 4, 1)),
               dict(gs=_abi.LxoGrammar(ptr(cls), 16, 4, 1)), dict(gs=_abi.LxoGrammar(ptr(cls), 2, 0, 1)),
               dict(gs=_abi.LxoGrammar(ptr(cls), 2, _abi.LXO_GRAMMAR_MAX_DEPTH + 1, 1)), dict(scratch_=None),
               dict(allow_=None, ld=2), dict(allow_=allow, ld=1), dict(allow_=allow, ld=-1), dict(fin_=None)):
        assert call(**kw) == -1, kw
        assert L.lxo_last_error()
    for kw in (dict(rows_=0), dict(k=0), dict(k=17, rows_=17), dict(rows_=3, k=2), dict(V_=0), dict(time=-1), dict(max_iter=-1)):
        assert call(**kw) == -5, kw
    assert np.array_equal(scratch, keep)                                    # refused: nothing ran
    assert L.lxo_grammar_scratch_bytes(0, V) == 0 and L.lxo_grammar_scratch_bytes(rows, 0) == 0
    assert L.lxo_grammar_scratch_bytes(rows, V) >= 4 * (rows * 2 + rows * 2)
