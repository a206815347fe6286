#!/usr/bin/env python
"""Prediction driver with the shape of the reference's predict.py:38-68: restore the trained model from a results
directory and print the LaTeX hypothesis for each image path given (the reference's interactive shell and its
pdf/LaTeX->PNG cropping helpers are out of scope).  --scores adds the hypothesis' log-prob and its geometric-mean token
probability exp(log-prob / tokens) (Img2SeqModel.predict_batch(..., return_scores=True)).  --formula "<tokens>" (one image) scores
that transcription instead of decoding: its log-prob (END included), geometric-mean token probability and the first position where
the model's top-1 token differs from it (Img2SeqModel.score_batch).  --prefix "<tokens>" (one image) decodes from that prefix: the
hypothesis keeps it and the model writes the rest (Img2SeqModel.complete_batch); it combines with --scores.  --ban "<tokens>" keeps those
tokens out of every hypothesis (e.g. --ban "_UNK _PAD"), --allow-file FILE (one token per line; END is added) lets only those in; both
combine with --scores and --prefix (predict_batch / complete_batch with banned= / allowed=).  --alternatives K adds one line per position
of the hypothesis (or, with --formula, of the given transcription): the token, its log-prob, its rank among the model's choices, the
entropy of the step and the model's K best tokens there with their log-probs (predict_batch / complete_batch / score_batch with
alternatives=K: for a decode they come from a second, teacher-forced pass over the emitted tokens); with --formula it combines with
--ban / --allow-file, which then constrain the alternatives.  --sample N draws N transcriptions per image instead of decoding the best one
(Img2SeqModel.sample_batch; --temperature T, --top-k K, --top-p P and --seed S shape and repeat the draws; combines with --ban /
--allow-file): one line with the agreement (top count / N), then one line per distinct hypothesis with its count and log-prob.
--consensus (with --sample) adds the minimum-risk choice among the draws (sample_batch(consensus=True)): the head line names the hypothesis with
the least expected edit distance to the draws and that cost, every hypothesis line carries its risk, and a * marks the chosen one; --consensus-cost bleu (only with --sample N --consensus) makes that cost 1 - sentence BLEU.
--balanced decodes under the delimiter grammar of the vocabulary (latex_ocr_amd.grammar.Grammar.latex: { }, \\left / \\right, \\begin{X} / \\end{X};
--pairs "OPEN:CLOSE ..." names the pairs instead, each side a comma-separated token list): every hypothesis closes what it opens.  It
combines with everything but --formula.  Without the flag, where the vocabulary has delimiters, a line "  balanced: yes / no" behind each
printed hypothesis says whether it does.
--boxes prints, per token of the decoded hypothesis (or, with --formula, of that transcription), its box in pixels of the image (left top right
bottom, the last two exclusive) and the share of its attention inside the box, behind a head line with the coverage map's largest cell and the share
of cells never attended (Img2SeqModel.locate_batch; --mass M sets the central mass the box keeps).  It combines with --formula only.
--nbest (config.decoding = "beam_search") prints the beam's hypotheses, back-traced and reranked on the device (Img2SeqModel.nbest_batch): one line
per hypothesis in rerank order with its score, log-prob, posterior, length and beam slot.  --length-penalty A and --coverage-penalty B are GNMT's
normalisation of the finished beam (0: the order of the log-probs); --consensus marks with a * the hypothesis of least expected cost against the
others weighted with their posteriors and prints every risk (--consensus-cost bleu: 1 - sentence BLEU).  It combines with --ban / --allow-file and
--balanced."""
import argparse

import numpy as np

from latex_ocr_amd.model.img2seq import Img2SeqModel
from latex_ocr_amd.model.utils.general import Config
from latex_ocr_amd.model.utils.image import greyscale
from latex_ocr_amd.model.utils.text import Vocab


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--results", default="results/small/")
    ap.add_argument("--scores", action="store_true", help="print the log-prob and the geometric-mean token probability of each hypothesis")
    ap.add_argument("--formula", default=None, help="score this space-separated token sequence against the (single) image")
    ap.add_argument("--prefix", default=None, help="decode the (single) image from this space-separated token prefix")
    ap.add_argument("--ban", default=None, help="space-separated tokens that must not be emitted")
    ap.add_argument("--allow-file", default=None, help="file with one token per line: only these (and END) may be emitted")
    ap.add_argument("--alternatives", type=int, default=0, metavar="K", help="per position: the token's log-prob and rank, the entropy and the K best tokens")
    ap.add_argument("--sample", type=int, default=0, metavar="N", help="draw N transcriptions per image: distinct hypotheses with counts, and their agreement")
    ap.add_argument("--temperature", type=float, default=1.0, help="--sample: softmax temperature (0: the arg-max)")
    ap.add_argument("--top-k", type=int, default=0, help="--sample: draw among the K most likely tokens (0: off)")
    ap.add_argument("--top-p", type=float, default=1.0, help="--sample: draw among the smallest token set of mass >= P (1: off)")
    ap.add_argument("--seed", type=int, default=0, help="--sample: the same seed repeats the draws")
    ap.add_argument("--consensus", action="store_true", help="--sample: the hypothesis of least expected edit distance to the draws, and that cost")
    ap.add_argument("--consensus-cost", choices=("edit", "bleu"), default=None,
                    help="--sample N --consensus: the cost the consensus minimises, the edit distance (default) or 1 - sentence BLEU")
    ap.add_argument("--balanced", action="store_true", help="decode under the delimiter grammar: every hypothesis closes what it opens")
    ap.add_argument("--pairs", default=None, help='delimiter pairs "OPEN:CLOSE ..." (each side comma-separated tokens) instead of those read off the vocabulary')
    ap.add_argument("--boxes", action="store_true", help="per token: its box in the image (pixels) and the share of its attention inside it; with --formula: of that transcription")
    ap.add_argument("--mass", type=float, default=0.9, help="--boxes: the central mass of each attention marginal the box keeps, in (0, 1]")
    ap.add_argument("--nbest", action="store_true", help="beam search: every hypothesis of the beam, reranked, with score, log-prob and posterior")
    ap.add_argument("--length-penalty", type=float, default=0.0, metavar="A", help="--nbest: score = logp / ((5 + length) / 6)^A")
    ap.add_argument("--coverage-penalty", type=float, default=0.0, metavar="B", help="--nbest: score += B * sum over the feature cells of log(min(coverage, 1))")
    ap.add_argument("images", nargs="+")
    a = ap.parse_args(argv)
    if a.boxes and (a.prefix is not None or a.sample or a.alternatives or a.ban is not None or a.allow_file is not None or a.balanced or a.pairs):
        ap.error("--boxes locates a plain decode or, with --formula, that transcription; it combines with nothing else")
    if a.boxes and not 0.0 < a.mass <= 1.0:
        ap.error("--mass lies in (0, 1]")
    if a.formula is not None and len(a.images) != 1:
        ap.error("--formula scores one image")
    if a.prefix is not None and (len(a.images) != 1 or a.formula is not None):
        ap.error("--prefix completes one image and does not combine with --formula")
    if a.sample and (a.formula is not None or a.prefix is not None or a.alternatives or not 1 <= a.sample <= 16):
        ap.error("--sample takes 1 .. 16 and does not combine with --formula, --prefix or --alternatives")
    if a.nbest and (a.formula is not None or a.prefix is not None or a.sample or a.alternatives or a.boxes or a.scores):
        ap.error("--nbest lists a beam decode's hypotheses; it combines with --ban, --allow-file, --balanced and --consensus only")
    if (a.length_penalty or a.coverage_penalty) and not a.nbest:
        ap.error("--length-penalty and --coverage-penalty rerank the hypotheses of --nbest")
    if a.length_penalty < 0 or a.coverage_penalty < 0:
        ap.error("--length-penalty and --coverage-penalty are >= 0")
    if a.consensus and not (a.sample or a.nbest):
        ap.error("--consensus chooses among the draws of --sample N or the hypotheses of --nbest")
    if a.consensus_cost is not None and not ((a.sample or a.nbest) and a.consensus):
        ap.error("--consensus-cost names the cost of --sample N --consensus or --nbest --consensus")
    d = a.results
    config_vocab, config_model = Config(d + "vocab.json"), Config(d + "model.json")
    vocab = Vocab(config_vocab)
    model = Img2SeqModel(config_model, d, vocab)
    model.build_pred()
    sets = {}
    if a.ban is not None:
        sets["banned"] = a.ban.split()
    if a.allow_file is not None:
        with open(a.allow_file) as f:
            sets["allowed"] = [t for t in (line.strip() for line in f) if t] + [vocab.id_end]
    if sets and a.formula is not None and not a.alternatives:
        ap.error("--ban / --allow-file constrain a decode and do not combine with --formula (without --alternatives)")
    if a.alternatives and not 1 <= a.alternatives <= min(16, vocab.n_tok):
        ap.error("--alternatives takes 1 .. min(16, vocabulary size)")
    alt = {"alternatives": a.alternatives} if a.alternatives else {}
    from latex_ocr_amd.grammar import Grammar
    try:
        gram = Grammar.from_pairs(vocab, [tuple(side.split(",") for side in p.split(":", 1)) for p in a.pairs.split()]) if a.pairs \
            else Grammar.latex(vocab)
    except ValueError as e:
        if a.balanced or a.pairs:
            ap.error("--balanced / --pairs: %s" % e)
        gram = None                                          # a vocabulary without delimiters: nothing to report
    if a.balanced:
        if a.formula is not None:
            ap.error("--balanced constrains a decode and does not combine with --formula")
        sets["grammar"] = gram
    dec = dict(sets)                                         # the decodes' keywords; score_batch takes the token sets only
    sets.pop("grammar", None)

    def report(text):
        if gram is not None and not a.balanced:
            print("  balanced:", "yes" if gram.check([vocab.tok_to_id.get(t, vocab.id_unk) for t in text.split()] + [vocab.id_end]) else "no")

    def print_alternatives(tokens, logps, entries):
        for t, (tok, lp, e) in enumerate(zip(tokens, logps, entries)):
            print("  %3d %-12s logp %8.4f  rank %3d  entropy %.4f  | %s" % (t, tok, lp, e["rank"], e["entropy"],
                                                                          "  ".join("%s %.4f" % c for c in e["alternatives"])))

    def emitted(hyp, n):
        toks = hyp.split()
        return toks + [vocab.id_to_tok[vocab.id_end]] * (n - len(toks))
    from PIL import Image
    out = []
    for path in a.images:
        img = np.asarray(Image.open(path).convert("RGB"))
        if a.boxes:
            res = model.locate_batch([greyscale(img)], None if a.formula is None else [a.formula], mass=a.mass)[0]
            print(path, "<=" if a.formula is not None else "=>", " ".join(e["token"] for e in res["tokens"]),
                  "\tmax coverage %.3f\tuncovered %.3f" % (res["max_coverage"], res["uncovered"]))
            for t, e in enumerate(res["tokens"]):
                print("  %3d %-12s box %4d %4d %4d %4d  inside %.3f" % ((t, e["token"]) + tuple(e["box"]) + (e["inside"],)))
            out.append(res)
            continue
        if a.nbest:
            more = {"consensus": True, "consensus_cost": a.consensus_cost or "edit"} if a.consensus else {}
            try:
                res = model.nbest_batch([greyscale(img)], length_penalty=a.length_penalty, coverage_penalty=a.coverage_penalty, **dict(dec, **more))[0]
            except ValueError as e:
                ap.error("--nbest: %s" % e)
            print(path, "=>", res["hypotheses"][0]["text"], "\tscore %.4f" % res["hypotheses"][0]["score"])
            if a.consensus:
                print(path, "=> consensus:", res["hypotheses"][res["consensus"]]["text"], "\texpected cost %.4f" % res["expected_cost"])
            for k, h in enumerate(res["hypotheses"]):
                risk = "  risk %.4f" % h["risk"] if a.consensus else ""
                print("%s slot %2d  score %9.4f  logp %9.4f  post %.4f  len %3d%s  %s" % ("*" if a.consensus and k == res["consensus"] else " ", h["slot"], h["score"],
                                                                                          h["logp"], h["posterior"], h["length"], risk, h["text"]))
                report(h["text"])
            out.append(res)
            continue
        if a.formula is not None:
            res = model.score_batch([greyscale(img)], [a.formula], **dict(alt, **sets))[0]
            lp, toks, first = res[:3]
            print(path, "<=", a.formula, "\tlogp %.4f\tgeo-mean p %.4f\tfirst disagreement %d" % (lp, np.exp(lp / max(1, len(toks))), first))
            if alt:
                print_alternatives(emitted(" ".join(vocab.id_to_tok[i] for i in vocab.form_prepro(a.formula)), len(toks)), toks, res[3])
            out.append(res)
            continue
        if a.sample:
            more = {"consensus": True} if a.consensus else {}
            if a.consensus_cost not in (None, "edit"):
                more["consensus_cost"] = a.consensus_cost
            res = model.sample_batch([greyscale(img)], a.sample, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, seed=a.seed, **dict(dec, **more))[0]
            print(path, "~>", "%d draws\tagreement %.3f" % (a.sample, res["agreement"]))
            if a.consensus:
                print(path, "=> consensus:", res["hypotheses"][res["consensus"]]["text"], "\texpected cost %.4f" % res["expected_cost"])
            for k, h in enumerate(res["hypotheses"]):
                if a.consensus:
                    print("%s %3d x  logp %9.4f  risk %.4f  %s" % ("*" if k == res["consensus"] else " ", h["count"], h["logp"], h["risk"], h["text"]))
                else:
                    print("  %3d x  logp %9.4f  %s" % (h["count"], h["logp"], h["text"]))
                report(h["text"])
            out.append(res)
            continue
        if a.prefix is not None:
            res = model.complete_batch([greyscale(img)], [a.prefix], return_scores=True, **dict(alt, **dec))
            hyps, scores = res[:2]
            lp, toks = scores[0][0]
            if a.scores:
                print(path, "=>", hyps[0][0], "\tlogp %.4f\tgeo-mean p %.4f" % (lp, np.exp(lp / max(1, len(toks)))))
            else:
                print(path, "=>", hyps[0][0])
            report(hyps[0][0])
            if alt:
                print_alternatives(emitted(hyps[0][0], len(toks)), toks, res[2][0][0])
            out.append(([h[0] for h in hyps], [s[0] for s in scores]) + (([x[0] for x in res[2]],) if alt else ()) if a.scores or alt else [h[0] for h in hyps])
            continue
        if a.scores or alt:
            res = model.predict_batch([greyscale(img)], return_scores=True, **dict(alt, **dec))
            hyps, scores = [h[0] for h in res[0]], res[1]
            lp, toks = scores[0][0]
            if a.scores:
                print(path, "=>", hyps[0], "\tlogp %.4f\tgeo-mean p %.4f" % (lp, np.exp(lp / max(1, len(toks)))))
            else:
                print(path, "=>", hyps[0])
            report(hyps[0])
            if alt:
                print_alternatives(emitted(hyps[0], len(toks)), toks, res[2][0][0])
            out.append((hyps, [s[0] for s in scores]) + (([x[0] for x in res[2]],) if alt else ()))
            continue
        hyps = [h[0] for h in model.predict_batch([greyscale(img)], **dec)] if dec else model.predict(greyscale(img))
        print(path, "=>", hyps[0])
        report(hyps[0])
        out.append(hyps)
    return out


if __name__ == "__main__":
    main()
