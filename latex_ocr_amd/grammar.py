"""Delimiter grammars for the decode calls (`grammar=` of Engine.greedy_decode / beam_decode / sample_decode): hypotheses that close what
they open.  The class is the host-side statement of the rules the device kernels follow (csrc/grammar.hip, include/lxo.h) and the reference
the tests replay them against.

A token has a class: 0 plain, +q an opener of delimiter kind q, -q a closer of kind q (1 <= q <= 15).  The state of a decoder row is the
stack of its open kinds, here a tuple (bottom first), `()` at the start.  With r = max_iter - t the steps that can still follow step t, an
unfinished row may emit
    a closer of kind q    iff the stack is not empty and its top is q,
    END                   iff the stack is empty,
    an opener             iff depth < max_depth and (budget) r >= depth + 2,
    any other token       iff (budget) r >= depth + 1,
so that with the budget depth <= r holds before every step and the row can always close everything and end by step max_iter.
"""
import re

import numpy as np

MAX_DEPTH = 32      # include/lxo.h LXO_GRAMMAR_MAX_DEPTH
MAX_KINDS = 15


def _vocab_maps(vocab):
    """-> (token -> id or None, V, id_end or None) of a Vocab, a token -> id dict, a token list or a vocabulary size"""
    if isinstance(vocab, (int, np.integer)):
        return None, int(vocab), None
    if isinstance(vocab, dict):
        return vocab, len(vocab), None
    if isinstance(vocab, (list, tuple)):
        return {t: i for i, t in enumerate(vocab)}, len(vocab), None
    return vocab.tok_to_id, int(vocab.n_tok), int(vocab.id_end)


class Grammar(object):
    def __init__(self, cls, max_depth=MAX_DEPTH, budget=True, id_end=None):
        cls = np.asarray(cls)
        if cls.ndim != 1 or cls.size < 1:
            raise ValueError("cls must be a non-empty vector of token classes, got shape %s" % (cls.shape,))
        if np.abs(cls.astype(np.int64)).max() > MAX_KINDS:
            raise ValueError("token classes must lie in [-%d, %d], got %d .. %d" % (MAX_KINDS, MAX_KINDS, int(cls.min()), int(cls.max())))
        if not 1 <= int(max_depth) <= MAX_DEPTH:
            raise ValueError("max_depth = %d outside 1 .. %d" % (int(max_depth), MAX_DEPTH))
        self.cls = np.ascontiguousarray(cls, dtype=np.int8)
        self.n_kinds = max(1, int(np.abs(self.cls.astype(np.int64)).max()))
        self.max_depth, self.budget = int(max_depth), bool(budget)
        self.id_end = None if id_end is None else int(id_end)
        if self.id_end is not None:
            self._check_end(self.id_end)

    def _check_end(self, id_end):
        if not 0 <= int(id_end) < self.cls.size:
            raise ValueError("id_end = %d outside [0, %d)" % (int(id_end), self.cls.size))
        if self.cls[int(id_end)] != 0:
            raise ValueError("id_end = %d must be a plain token, its class is %d" % (int(id_end), int(self.cls[int(id_end)])))

    def _end(self, id_end):
        e = self.id_end if id_end is None else int(id_end)
        if e is None:
            raise ValueError("this grammar was built without id_end: pass it")
        self._check_end(e)
        return e

    @property
    def n_tok(self):
        return int(self.cls.size)

    @classmethod
    def from_pairs(cls, vocab, pairs, max_depth=MAX_DEPTH, budget=True):
        """One delimiter kind per pair (openers, closers); each side a token string / id or a list of them.  vocab: a Vocab, a token -> id
        dict, a token list, or the vocabulary size (ids only)."""
        t2i, V, id_end = _vocab_maps(vocab)
        if not 1 <= len(pairs) <= MAX_KINDS:
            raise ValueError("%d delimiter kinds outside 1 .. %d" % (len(pairs), MAX_KINDS))
        table = np.zeros(V, np.int8)

        def ids_of(side):
            out = []
            for x in (side if isinstance(side, (list, tuple, set, frozenset)) else [side]):
                if isinstance(x, (int, np.integer)):
                    i = int(x)
                else:
                    if t2i is None or x not in t2i:
                        raise ValueError("token %r is not in the vocabulary" % (x,))
                    i = int(t2i[x])
                if not 0 <= i < V:
                    raise ValueError("token id %d outside [0, %d)" % (i, V))
                out.append(i)
            return out

        for q, (op, clo) in enumerate(pairs, 1):
            for sign, side in ((1, op), (-1, clo)):
                for i in ids_of(side):
                    if table[i] != 0:
                        raise ValueError("token id %d is given two classes" % i)
                    table[i] = sign * q
        return cls(table, max_depth, budget, id_end)

    @classmethod
    def latex(cls, vocab, max_depth=MAX_DEPTH, budget=True):
        """From the token strings: `{` / `}`; every token starting `\\left` / `\\right`; `\\begin{X}` / `\\end{X}`, one kind per X.  A kind with
        no opener or no closer in the vocabulary is dropped (its tokens stay plain)."""
        t2i, V, id_end = _vocab_maps(vocab)
        if t2i is None:
            raise ValueError("Grammar.latex needs the token strings")
        groups = {}                                                    # key -> ([opener ids], [closer ids]), in order of first appearance
        for tok, i in sorted(t2i.items(), key=lambda kv: kv[1]):
            m = re.match(r"^\\(begin|end)\{(.*)\}$", tok)
            if tok == "{" or tok == "}":
                key, side = "{", 0 if tok == "{" else 1
            elif tok.startswith("\\left"):
                key, side = "\\left", 0
            elif tok.startswith("\\right") and not tok.startswith("\\rightarrow") and not tok.startswith("\\rightharpoon") \
                    and not tok.startswith("\\rightleft"):
                key, side = "\\left", 1
            elif m:
                key, side = "\\begin{%s}" % m.group(2), 0 if m.group(1) == "begin" else 1
            else:
                continue
            if tok.startswith("\\leftarrow") or tok.startswith("\\leftrightarrow") or tok.startswith("\\leftharpoon"):
                continue
            groups.setdefault(key, ([], []))[side].append(int(i))
        pairs = [(o, c) for o, c in groups.values() if o and c]
        if not pairs:
            raise ValueError("the vocabulary holds no delimiter pair")
        if len(pairs) > MAX_KINDS:
            raise ValueError("the vocabulary holds %d delimiter kinds, more than %d" % (len(pairs), MAX_KINDS))
        return cls.from_pairs(vocab, pairs, max_depth, budget)

    # ---- the state machine ----
    def allowed_at(self, state, t, max_iter, id_end=None):
        """bool [V]: the grammar set G(state, t) of an unfinished row whose stack is `state`"""
        e = self._end(id_end)
        d, r = len(state), int(max_iter) - int(t)
        c = self.cls.astype(np.int64).copy()
        ok = np.zeros(c.size, bool)
        is_end = np.arange(c.size) == e
        if d > 0:
            ok |= (c == -state[-1]) & ~is_end
        else:
            ok |= is_end
        if d < self.max_depth and (not self.budget or r >= d + 2):
            ok |= (c > 0) & ~is_end
        if not self.budget or r >= d + 1:
            ok |= (c == 0) & ~is_end
        return ok

    def apply(self, state, tok):
        """the stack after an unfinished row emitted `tok`: an opener below max_depth pushes, a closer that matches the top pops, anything
        else -- a mismatched closer, a closer on an empty stack, an opener at max_depth -- leaves it"""
        tok = int(tok)
        c = int(self.cls[tok]) if 0 <= tok < self.cls.size else 0
        if self.id_end is not None and tok == self.id_end:
            c = 0
        if c > 0 and len(state) < self.max_depth:
            return tuple(state) + (c,)
        if c < 0 and state and state[-1] == -c:
            return tuple(state[:-1])
        return tuple(state)

    def check(self, ids, id_end=None):
        """balanced and ended: the tokens of `ids` up to its first END nest correctly, and there is an END"""
        e = self._end(id_end)
        stack = []
        for tok in np.asarray(ids).reshape(-1).tolist():
            if tok == e:
                return not stack
            c = int(self.cls[tok]) if 0 <= tok < self.cls.size else 0
            if c > 0:
                stack.append(c)
            elif c < 0:
                if not stack or stack[-1] != -c:
                    return False
                stack.pop()
        return False

    def replay(self, ids, max_iter, id_end=None, n_forced=0):
        """Walks one emitted row: -> (depths after each step, ok) with ok False if a token at a step >= n_forced lies outside its set; the row
        is frozen from its first END on (as the decode loop keeps it)"""
        e = self._end(id_end)
        state, depth, ok, done = (), [], True, False
        for t, tok in enumerate(np.asarray(ids).reshape(-1).tolist()):
            if not done:
                if t >= n_forced and not self.allowed_at(state, t, max_iter, e)[tok]:
                    ok = False
                if tok == e and t >= n_forced:
                    done = True
                else:
                    state = self.apply(state, tok)
            depth.append(len(state))
        return depth, ok
