"""Decode post-processing and text metrics (host).

`truncate_end` / `write_answers` mirror `model/evaluation/text.py:95-145` of
the reference.  The metrics (`score_files`, :12-92) use nltk / `distance` in
the reference; neither is installed, so BLEU-4 (corpus level, nltk's
brevity-penalty definition, no smoothing), Levenshtein and exact match are
restated here in pure Python.
"""
import math
import os
from collections import Counter

from ..utils.general import init_dir
from ..utils.text import load_formulas


def truncate_end(list_of_ids, id_end):
    """Cut at the first END id (reference: evaluation/text.py:95-104)."""
    out = []
    for idx in list_of_ids:
        if idx == id_end:
            break
        out.append(idx)
    return out


def write_answers(references, hypotheses, rev_vocab, dir_name, id_end):
    """ref.txt + one hyp_i.txt per hypothesis rank; ids are cut at END and
    joined with single spaces.  Reference: evaluation/text.py:107-145."""
    def ids_to_str(ids):
        return " ".join(rev_vocab[int(i)] for i in truncate_end(ids, id_end))

    def write_file(name, rows):
        with open(name, "w") as f:
            for r in rows:
                f.write(ids_to_str(r) + "\n")

    init_dir(dir_name)
    names = [dir_name + "ref.txt"]
    write_file(names[0], references)
    for i, hyp in enumerate(hypotheses):
        assert len(references) == len(hyp)
        names.append(dir_name + "hyp_{}.txt".format(i))
        write_file(names[-1], hyp)
    return names


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def exact_match_score(references, hypotheses):
    """Reference: evaluation/text.py:41-56."""
    hits = sum(1 for r, h in zip(references, hypotheses) if list(r) == list(h))
    return hits / float(max(len(hypotheses), 1))


def edit_distance(references, hypotheses):
    """1 - sum(levenshtein) / sum(max len) (reference: evaluation/text.py:75-92)."""
    d, tot = 0, 0.0
    for r, h in zip(references, hypotheses):
        d += levenshtein(r, h)
        tot += float(max(len(r), len(h)))
    return 1.0 - d / tot if tot else 1.0


def _ngrams(seq, n):
    return Counter(tuple(seq[i:i + n]) for i in range(len(seq) - n + 1))


def corpus_bleu(list_of_references, hypotheses, max_n=4):
    """nltk.translate.bleu_score.corpus_bleu(list_of_references, hypotheses, weights = uniform over 1 .. max_n), no smoothing -- the
    published algorithm of the third-party call at evaluation/text.py:70-72 (nltk is not installed here), restated: per n the clipped
    n-gram matches (a hypothesis n-gram counts at most as often as in the reference that has it most) and the hypothesis n-gram totals
    (max(1, .) per sentence, as nltk's `modified_precision` does for hypotheses shorter than n) are summed over the corpus BEFORE the
    division; brevity penalty from the summed hypothesis lengths and the summed closest reference lengths (ties -> the shorter reference).
    Held to nltk's own documented values in tests/test_host_surface.py."""
    num, den = [0] * max_n, [0] * max_n
    hyp_len = ref_len = 0
    for refs, hyp in zip(list_of_references, hypotheses):
        hyp_len += len(hyp)
        ref_len += min((len(r) for r in refs), key=lambda rl: (abs(rl - len(hyp)), rl))
        for n in range(1, max_n + 1):
            h = _ngrams(hyp, n)
            best = Counter()
            for r in refs:
                for g, c in _ngrams(r, n).items():
                    if c > best[g]:
                        best[g] = c
            num[n - 1] += sum(min(c, best[g]) for g, c in h.items())
            den[n - 1] += max(1, len(hyp) - n + 1)
    return _bleu_from_counts(num, den, hyp_len, ref_len)


def _bleu_from_counts(num, den, hyp_len, ref_len):
    """corpus_bleu's tail: the score from the summed clipped matches and totals per order and the summed lengths"""
    max_n = len(num)
    if num[0] == 0 or min(num) == 0 or min(den) == 0:
        return 0.0
    logp = sum(math.log(n / d) for n, d in zip(num, den)) / max_n
    bp = 1.0 if hyp_len > ref_len else math.exp(1 - ref_len / float(max(hyp_len, 1)))
    return bp * math.exp(logp)


def bleu_score(references, hypotheses, max_n=4):
    """Corpus BLEU-4 with uniform weights, one reference per hypothesis: the call at evaluation/text.py:57-72
    (`references = [[ref] for ref in references]`, then nltk's corpus_bleu)."""
    return corpus_bleu([[ref] for ref in references], hypotheses, max_n)


def sentence_bleu(hyp, ref):
    """Sentence-level BLEU-4 of one hypothesis against one reference, the definition of include/lxo.h (lxo_sentence_bleu) in Python floats: clipped
    matches m_n and totals t_n = max(1, |h| - n + 1) for n = 1 .. 4; add-one smoothing on the higher orders only (Lin and Och; nltk's
    SmoothingFunction().method2): p_1 = m_1 / t_1, p_n = (m_n + 1) / (t_n + 1); brevity penalty 1 for |h| > |r|, else exp(1 - |r| / |h|);
    0 without a common unigram (an empty hypothesis included); and 1 exactly for hyp == ref, whatever the smoothed formula says (two empty
    sequences included), so that a reference costs 0 against itself."""
    hyp, ref = [x for x in hyp], [x for x in ref]
    if hyp == ref:
        return 1.0
    m = []
    for n in range(1, 5):
        R = _ngrams(ref, n)
        m.append(sum(min(c, R[g]) for g, c in _ngrams(hyp, n).items()))
    if m[0] == 0:
        return 0.0
    t = [max(1, len(hyp) - n + 1) for n in range(1, 5)]
    logp = math.log(m[0] / float(t[0])) + sum(math.log((m[k] + 1) / float(t[k] + 1)) for k in (1, 2, 3))
    bp = 1.0 if len(hyp) > len(ref) else math.exp(1 - len(ref) / float(len(hyp)))
    return bp * math.exp(logp / 4)


def sentence_bleu_cost(hyp, ref):
    """1 - sentence_bleu(hyp, ref): the cost in [0, 1] that minimum-risk training and the consensus decode take with cost = "bleu"."""
    return 1.0 - sentence_bleu(hyp, ref)


def score_files(path_ref, path_hyp):
    """Reference: evaluation/text.py:12-38 (tokens split on single spaces)."""
    refs = [r.split(" ") for _, r in load_formulas(path_ref).items()]
    hyps = [h.split(" ") for _, h in load_formulas(path_hyp).items()]
    assert len(refs) == len(hyps)
    return {
        "BLEU-4": bleu_score(refs, hyps) * 100,
        "ExactMatchScore": exact_match_score(refs, hyps) * 100,
        "EditDistance": edit_distance(refs, hyps) * 100,
    }


def scores_from_counts(corpus):
    """The dict of `score_files` from the 14 integers lxo_text_stats sums over a set of pairs (include/lxo.h: corpus_io) -- clipped matches and
    totals for n = 1 .. 4, the summed hypothesis and reference lengths, the summed distances, the summed max(|h|, |r|), the exact matches and the
    number of pairs.  The expressions are those of `corpus_bleu`'s tail, `edit_distance` and `exact_match_score` on the same integers, so the
    floats equal theirs."""
    c = [int(x) for x in corpus]
    if len(c) != 14:
        raise ValueError("scores_from_counts: 14 integers expected, got %d" % len(c))
    tot = float(c[11])
    return {
        "BLEU-4": _bleu_from_counts(c[0:4], c[4:8], c[8], c[9]) * 100,
        "ExactMatchScore": c[12] / float(max(c[13], 1)) * 100,
        "EditDistance": (1.0 - c[10] / tot if tot else 1.0) * 100,
    }


def align(hyp, ref):
    """The canonical edit alignment of one hypothesis against one reference, the definition of include/lxo.h (lxo_edit_align) in plain Python -- the
    product's host path, as sentence_bleu is for its kernel.  D[i][j] is the Levenshtein table; the path is walked back from (len(hyp), len(ref)),
    at every cell the FIRST rule that applies: a diagonal step (match or substitution) if D[i][j] == D[i-1][j-1] + (h != r), else an insertion
    (a hypothesis token the reference lacks) if D[i][j] == D[i-1][j] + 1, else a deletion.  The rule is local, so the steps are noted row by row
    while the table is filled and only they are kept.
    -> (hyp_align, ref_align, counts): per hypothesis position the reference position it is aligned with or -1 (inserted), per reference position
    the hypothesis position or -1 (deleted), and [matches, substitutions, insertions, deletions, len(hyp), len(ref)]."""
    h, r = [x for x in hyp], [x for x in ref]
    m, n = len(h), len(r)
    prev = list(range(n + 1))
    steps = []
    for i in range(1, m + 1):
        cur, row, x = [i] + [0] * n, [1] * (n + 1), h[i - 1]
        for j in range(1, n + 1):
            d = prev[j - 1] + (0 if x == r[j - 1] else 1)
            cur[j] = min(d, prev[j] + 1, cur[j - 1] + 1)
            row[j] = 0 if cur[j] == d else (1 if cur[j] == prev[j] + 1 else 2)
        steps.append(row)
        prev = cur
    ha, ra = [-1] * m, [-1] * n
    counts = [0, 0, 0, 0, m, n]
    i, j = m, n
    while i > 0 and j > 0:
        s = steps[i - 1][j]
        if s == 0:
            counts[0 if h[i - 1] == r[j - 1] else 1] += 1
            ha[i - 1], ra[j - 1] = j - 1, i - 1
            i, j = i - 1, j - 1
        elif s == 1:
            i -= 1
        else:
            j -= 1
    counts[2], counts[3] = ha.count(-1), ra.count(-1)
    return ha, ra, counts


def error_report(corpus, confusion, rev_vocab, top=20):
    """The error breakdown of a set of pairs from what lxo_edit_align sums over them (include/lxo.h): corpus, its 8 integers -- matches,
    substitutions, insertions, deletions, hypothesis tokens, reference tokens, pairs, steps left out of the matrix -- and confusion, its
    (V + 1) x (V + 1) matrix, [a][b] = steps with reference token a and hypothesis token b, index V = no token.  rev_vocab maps an id to its
    token (a dict or a list; an id it lacks is shown as its number).  -> a dict:
      matches, substitutions, insertions, deletions, hyp_tokens, ref_tokens, pairs, left_out: the integers;
      SubRate, InsRate, DelRate: percent of the reference tokens (0.0 without any);
      confusions: the `top` largest off-diagonal [a][b] with a, b < V, as (ref_token, hyp_token, count);
      deleted / inserted: the `top` largest of column V / row V, as (token, count);
      recall: per reference token seen at least once, diagonal over row sum, the `top` lowest, as (token, recall, seen).
    Entries that are 0 are not listed, and ties in every ranking go to the lower ids (reference id first), so the report is one fixed object."""
    c = [int(x) for x in corpus]
    if len(c) != 8:
        raise ValueError("error_report: 8 integers expected in corpus, got %d" % len(c))
    flat = [int(x) for x in (confusion.reshape(-1) if hasattr(confusion, "reshape") else confusion)]
    V = int(round(math.sqrt(len(flat)))) - 1
    if V < 1 or (V + 1) * (V + 1) != len(flat):
        raise ValueError("error_report: confusion must hold (V + 1)^2 integers with V >= 1, got %d" % len(flat))
    C = [flat[a * (V + 1):(a + 1) * (V + 1)] for a in range(V + 1)]
    name = (lambda i: rev_vocab.get(i, str(i))) if hasattr(rev_vocab, "get") else (lambda i: rev_vocab[i] if 0 <= i < len(rev_vocab) else str(i))
    rate = lambda x: 100.0 * x / float(c[5]) if c[5] else 0.0
    pairs = sorted(((-C[a][b], a, b) for a in range(V) for b in range(V) if a != b and C[a][b]))[:top]
    deleted = sorted(((-C[a][V], a) for a in range(V) if C[a][V]))[:top]
    inserted = sorted(((-C[V][b], b) for b in range(V) if C[V][b]))[:top]
    seen = [(C[a][a] / float(sum(C[a])), a, sum(C[a])) for a in range(V) if sum(C[a])]
    return {
        "matches": c[0], "substitutions": c[1], "insertions": c[2], "deletions": c[3], "hyp_tokens": c[4], "ref_tokens": c[5], "pairs": c[6], "left_out": c[7],
        "SubRate": rate(c[1]), "InsRate": rate(c[2]), "DelRate": rate(c[3]),
        "confusions": [(name(a), name(b), -k) for k, a, b in pairs],
        "deleted": [(name(a), -k) for k, a in deleted],
        "inserted": [(name(b), -k) for k, b in inserted],
        "recall": [(name(a), q, s) for q, a, s in sorted(seen)[:top]],
    }


def format_error_report(report):
    """error_report's dict as the text evaluate_txt.py --errors writes"""
    out = ["pairs %d  reference tokens %d  hypothesis tokens %d" % (report["pairs"], report["ref_tokens"], report["hyp_tokens"]),
           "matches %d  substitutions %d  insertions %d  deletions %d  (left out of the matrix: %d)"
           % (report["matches"], report["substitutions"], report["insertions"], report["deletions"], report["left_out"]),
           "SubRate %.2f  InsRate %.2f  DelRate %.2f" % (report["SubRate"], report["InsRate"], report["DelRate"]), "", "confusions (reference -> hypothesis, count)"]
    out += ["  %s -> %s  %d" % x for x in report["confusions"]]
    out += ["", "deleted (reference tokens the hypotheses lack)"] + ["  %s  %d" % x for x in report["deleted"]]
    out += ["", "inserted (hypothesis tokens the references lack)"] + ["  %s  %d" % x for x in report["inserted"]]
    out += ["", "lowest recall (token, recall, occurrences)"] + ["  %s  %.4f  %d" % x for x in report["recall"]]
    return "\n".join(out) + "\n"
