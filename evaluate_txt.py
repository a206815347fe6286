#!/usr/bin/env python
"""Text evaluation driver with the shape of the reference's evaluate_txt.py:13-50: reload the
configs saved in the results dir, restore the latest checkpoint, decode the test set, score.  --per-sample FILE also writes the
teacher-forced score of every test sample's own label (Img2SeqModel.score_batch), one TSV line each -- index, tokens, sequence
log-prob, mean token log-prob, first position where the model's top-1 differs from the label -- lowest mean first.  --on-device takes the text
metrics from the decoded ids on the device (Img2SeqModel.score_ids) instead of re-reading the files: the same numbers, the same line.  --errors FILE aligns every decoded hypothesis with its
reference on the device (Img2SeqModel.error_analysis) and writes the error breakdown -- substitution, insertion and deletion counts and rates, the
most frequent confusions, the tokens most often dropped and inserted, the tokens of lowest recall -- to FILE as text."""
import argparse

from latex_ocr_amd.model.evaluation.text import format_error_report, score_files
from latex_ocr_amd.model.img2seq import Img2SeqModel
from latex_ocr_amd.model.utils.general import Config, minibatches
from latex_ocr_amd.model.utils.text import Vocab
from train import make_sets


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--results", default="results/small/")
    ap.add_argument("--per-sample", default=None, metavar="FILE", help="write per-sample teacher-forced scores of the labels (TSV)")
    ap.add_argument("--on-device", action="store_true", help="text metrics from the decoded ids on the device, not from the written files")
    ap.add_argument("--errors", default=None, metavar="FILE", help="write the error breakdown of the decoded hypotheses (edit alignment on the device)")
    a = ap.parse_args(argv)
    d = a.results
    config_data, config_vocab, config_model = Config(d + "data.json"), Config(d + "vocab.json"), Config(d + "model.json")
    vocab = Vocab(config_vocab)
    model = Img2SeqModel(config_model, d, vocab)
    model.build_pred()
    (test_set,) = make_sets(config_data, vocab, names=("test",))
    config_eval = Config({"dir_answers": d + "formulas_test/", "batch_size": 20})
    if a.on_device or a.errors:
        files, perplexity, (refs, hyps) = model.write_prediction(config_eval, test_set, return_ids=True)
        scores = model.score_ids(refs, hyps[0]) if a.on_device else score_files(files[0], files[1])
    else:
        files, perplexity = model.write_prediction(config_eval, test_set)
        scores = score_files(files[0], files[1])
    scores["perplexity"] = perplexity
    model.logger.info("- Test Txt: " + " || ".join("{} is {:04.2f}".format(k, v) for k, v in scores.items()))
    if a.errors:
        report = model.error_analysis(refs, hyps[0])
        with open(a.errors, "w") as f:
            f.write(format_error_report(report))
        model.logger.info("- Test Errors: " + " || ".join("{} is {:04.2f}".format(k, report[k]) for k in ("SubRate", "InsRate", "DelRate")))
    if a.per_sample:
        write_per_sample(model, vocab, test_set, a.per_sample, config_eval.batch_size)
    return scores


def write_per_sample(model, vocab, test_set, path, batch_size):
    """One line per test sample, in ascending mean token log-prob: the labels the model finds least likely first."""
    rows, i = [], 0
    for img, formula in minibatches(test_set, batch_size):
        for form, (lp, toks, first) in zip(formula, model.score_batch(img, formula)):
            rows.append((lp / len(toks), i, " ".join(vocab.id_to_tok[int(t)] for t in form), lp, first))
            i += 1
    rows.sort(key=lambda r: (r[0], r[1]))
    with open(path, "w") as f:
        for mean, idx, toks, lp, first in rows:
            f.write("%d\t%s\t%.6f\t%.6f\t%d\n" % (idx, toks, lp, mean, first))


if __name__ == "__main__":
    main()
