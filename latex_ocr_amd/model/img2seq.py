"""Img2SeqModel: the reference's model facade over the MI355X-native engine.

Mirrors `model/img2seq.py` of the reference method by method (cited); the single
`sess.run` boundary (:169, :236, :263) becomes calls into liblxo.so through
`latex_ocr_amd.engine.Engine`.  Inputs are the reference's: lists of variable-shape
uint8 [H,W,1] arrays and lists of int lists; the facade owns padding.
"""
import numpy as np

from .base import BaseModel
from .evaluation.text import levenshtein, score_files, sentence_bleu_cost, truncate_end, write_answers
from .params import dims_from_config
from .utils.general import Config, Progbar, minibatches
from .utils.image import pad_batch_images
from .utils.text import pad_batch_formulas


class Img2SeqModel(BaseModel):
    def __init__(self, config, dir_output, vocab, lib=None):
        """Reference: model/img2seq.py:23-32.  lib: a bound library to drive instead of liblxo.so (_abi.bind; the engine then runs on
        config.device, default "cpu" -- the host build of the sources under test)."""
        super(Img2SeqModel, self).__init__(config, dir_output)
        self._vocab = vocab
        self._lib = lib
        self.dist = None            # latex_ocr_amd.dist.DataParallel when launched one process per GPU (attach_dist)

    def attach_dist(self, dist):
        """Data-parallel training: every rank builds the same model, trains on its share of each
        shape bucket and all-reduces gradients; evaluation / checkpoints are written by rank 0 only."""
        self.dist = dist

    # ------------------------------------------------------------------ build --
    def _build_engine(self):
        from ..engine import Engine
        cfg = self._config
        lib = getattr(self, "_lib", None)
        dev = str(getattr(cfg, "device", ""))
        self.engine = Engine(self._vocab.n_tok, dims=dims_from_config(cfg),
                             dtype=getattr(cfg, "compute_dtype", "bf16"),
                             device=dev if dev.startswith("cuda") else ("cuda:0" if lib is None else dev or "cpu"),
                             lib=lib,
                             seed=getattr(cfg, "seed", 0),
                             beam=getattr(cfg, "beam_size", 1) if getattr(cfg, "decoding", "greedy") == "beam_search" else 1,
                             max_steps=getattr(cfg, "max_length_formula", 150) + 2)

    def build_train(self, config):
        """Reference: model/img2seq.py:34-40.  The training config's optional "label_smoothing" key (a number in [0, 1), default 0.0) makes every
        cross-entropy step minimise the smoothed loss (Engine.train_step(label_smoothing=)); it does not combine with the "mrt" key.  The optional
        "distill" key (_distill_config) makes every batch a distill_batch; it combines with "label_smoothing" and not with "mrt"."""
        from ..engine import Engine
        self._label_smoothing = Engine._check_smoothing("training config: \"label_smoothing\"", getattr(config, "label_smoothing", 0.0))
        if self._label_smoothing > 0.0 and getattr(config, "mrt", None) is not None:
            raise ValueError("training config: \"label_smoothing\" and \"mrt\" do not combine -- the minimum-risk step does not smooth its targets; "
                             "drop one of the two keys")
        mrt = getattr(config, "mrt", None)
        if mrt is not None:                                      # the cost of the minimum-risk step is refused here, not at the first batch
            self._check_cost("training config: \"mrt\": \"cost\"", mrt.get("cost", "edit") if isinstance(mrt, dict) else getattr(mrt, "cost", "edit"))
        distill = self._distill_config(getattr(config, "distill", None), mrt)
        self.logger.info("Building model...")
        self._build_engine()
        # the optional "distill": {"teacher": <model dir or list of dirs>, "k": 5, "weight": 0.5} key: the teacher(s) are restored once, here, with this
        # model's vocabulary and model config, for inference only; every training batch is then one distill_batch (it combines with "label_smoothing")
        self._distill = dict(distill, teacher=[self._load_teacher(d, i) for i, d in enumerate(distill["teacher"])]) if distill else None
        self._lr_method = config.lr_method.lower()
        self.engine.set_optimizer(self._lr_method)               # img2seq.py:95-109
        self._clip = getattr(config, "clip", -1)
        self.init_session()
        self.logger.info("- done.")

    DISTILL_KEYS = ("teacher", "k", "weight")

    def _distill_config(self, distill, mrt):
        """The training config's "distill" key before anything is built -> {"teacher": [dirs], "k", "weight"} or None"""
        if distill is None:
            return None
        if mrt is not None:
            raise ValueError("training config: \"distill\" and \"mrt\" do not combine -- the minimum-risk step takes no soft targets; drop one of the two keys")
        d = dict(distill) if isinstance(distill, dict) else {k: getattr(distill, k) for k in self.DISTILL_KEYS if hasattr(distill, k)}
        unknown = sorted(set(d) - set(self.DISTILL_KEYS))
        if unknown:
            raise ValueError("training config: unknown key(s) %s under \"distill\" (known: %s)" % (unknown, list(self.DISTILL_KEYS)))
        dirs = d.get("teacher")
        dirs = [dirs] if isinstance(dirs, str) else list(dirs or [])
        if not dirs or not all(isinstance(x, str) for x in dirs):
            raise ValueError("training config: \"distill\": \"teacher\" must be a model directory or a list of them, got %r" % (d.get("teacher"),))
        k, weight = d.get("k", 5), d.get("weight", 0.5)
        if not (isinstance(k, int) and k >= 1 and k * len(dirs) <= 16):
            raise ValueError("training config: \"distill\": k = %r with %d teacher(s): k must be >= 1 and k * teachers <= 16" % (k, len(dirs)))
        if not (isinstance(weight, (int, float)) and 0.0 <= float(weight) <= 1.0):
            raise ValueError("training config: \"distill\": \"weight\" must be a number in [0, 1], got %r" % (weight,))
        return {"teacher": dirs, "k": k, "weight": float(weight)}

    def _load_teacher(self, path, i):
        """A teacher for distill_batch: this model's vocabulary and model config, the weights of the latest checkpoint of model directory `path`
        (or of a weights directory / checkpoint file), built for inference.  A checkpoint made for another vocabulary or model config is refused."""
        import os
        t = Img2SeqModel(self._config, self._dir_output + "distill_teacher_%d/" % i, self._vocab, lib=getattr(self, "_lib", None))
        t.build_pred()
        w = os.path.join(path, "model_weights")
        ckpt = w if os.path.isdir(w) else path
        if os.path.isdir(ckpt):
            found = self.latest_checkpoint(ckpt if ckpt.endswith("/") else ckpt + "/")
            if found is None:
                raise IOError("training config: \"distill\": no checkpoint in %s" % ckpt)
            ckpt = found
        z = self._open_checkpoint(ckpt)
        for name, shp, _ in t.engine.specs:
            if name in z and tuple(np.shape(z[name])) != tuple(shp):
                raise ValueError("training config: \"distill\": teacher %s holds %s of shape %s, this model's is %s -- another vocabulary or model "
                                 "config" % (path, name, list(np.shape(z[name])), list(shp)))
        t.restore_session(ckpt)
        return t

    def build_pred(self):
        """Reference: model/img2seq.py:42-46."""
        self.logger.info("Building model...")
        self._build_engine()
        self.init_session()
        self.logger.info("- done.")

    # ------------------------------------------------------------------ feeds --
    def _get_feed_dict(self, img, formula=None, lr=None, dropout=1):
        """Reference: model/img2seq.py:125-142.  `dropout` is a KEEP probability (quirk C-5);
        every value >= 1 is the identity (the shipped configs use 1 and 127); values in (0, 1) drop h and o
        in the decoder cell (attention_cell.py:72,83) -- the encoder receives the placeholder but never uses it."""
        if not dropout > 0:
            raise ValueError("dropout is a keep probability and must be > 0, got {}".format(dropout))
        fd = {"img": pad_batch_images(img), "dropout": dropout}
        if formula is not None:
            f, l = pad_batch_formulas(formula, self._vocab.id_pad, self._vocab.id_end)
            fd["formula"], fd["formula_length"] = f, l
        if lr is not None:
            fd["lr"] = lr
        return fd

    # ------------------------------------------------------------------ train --
    def _run_train(self, config, train_set, val_set, epoch, lr_schedule):
        """Reference: model/img2seq.py:144-196.  The feed runs on the background input pipeline (pipeline.py:
        pinned staging + copy stream, `prefetch_depth` batches ahead; config.prefetch_depth = 0 restores the
        reference's synchronous feed); under data parallelism every rank takes its slice of each shape bucket."""
        from ..pipeline import Prefetcher, ShardedBuckets
        batch_size = config.batch_size
        world = self.dist.world if self.dist is not None else 1
        rank = self.dist.rank if self.dist is not None else 0
        nbatches = (len(train_set) + batch_size * world - 1) // (batch_size * world)
        keep = getattr(config, "dropout", 1)
        if not keep > 0:
            raise ValueError("dropout is a keep probability and must be > 0, got {}".format(keep))
        mrt = getattr(config, "mrt", None)
        if mrt is not None:
            if getattr(self, "_label_smoothing", 0.0) > 0.0 or getattr(config, "label_smoothing", 0.0):
                raise ValueError("training config: \"label_smoothing\" and \"mrt\" do not combine")
            return self._run_train_mrt(config, train_set, val_set, epoch, lr_schedule, mrt, keep)
        depth = int(getattr(config, "prefetch_depth", 2))
        # steps per pass are counted once per (dataset, batch size, world): another train() call with other arguments must not reuse the count
        key = (id(train_set), batch_size, world)
        cached = getattr(self, "_dp_nbatches", None)
        batches = ShardedBuckets(train_set, batch_size, world, rank, n_steps=cached[1] if cached and cached[0] == key else None) if world > 1 else None
        if batches is not None:
            nbatches = len(batches)        # steps this pass really takes (per shape bucket), what the LR schedule was scaled with
            self._dp_nbatches = (key, nbatches)   # the same set every epoch: counted once
        prog = Progbar(nbatches)
        eps = getattr(self, "_label_smoothing", 0.0)
        smooth = dict(label_smoothing=eps) if eps > 0.0 else {}
        if depth > 0:
            feed = Prefetcher(train_set, batch_size, self._vocab.id_pad, self._vocab.id_end, device=self.engine.device,
                              depth=depth, batches=batches)
            it = ((b.img, b.formula, b.lengths) for b in feed)
        else:
            def sync_feed():
                for img, formula in (batches if batches is not None else minibatches(train_set, batch_size)):
                    fd = self._get_feed_dict(img, formula=formula)
                    yield fd["img"], fd["formula"], fd["formula_length"]
            it = sync_feed()
        distill = getattr(self, "_distill", None)
        for i, (img, formula, lengths) in enumerate(it):
            if distill:
                smooth = dict(smooth, soft_targets=self._teacher_targets(distill["teacher"], distill["k"], img, formula, lengths),
                              soft_weight=distill["weight"])
            loss_eval = self.engine.train_step(img, formula, lengths, lr_schedule.lr, clip=self._clip, dist=self.dist,
                                               dropout=keep, **smooth)
            # the loss the step optimised; the perplexity of the PLAIN cross-entropy, smoothed or not: comparable between runs
            prog.update(i + 1, [("loss", loss_eval), ("perplexity", np.exp(self.engine.last_ce if smooth else loss_eval)), ("lr", lr_schedule.lr)])
            lr_schedule.update(batch_no=epoch * nbatches + i)
        self.logger.info("- Training: {}".format(prog.info))
        sub = "formulas_val/" if rank == 0 else "formulas_val_rank%d/" % rank    # every rank scores (keeps LR schedules equal)
        config_eval = Config({"dir_answers": self._dir_output + sub, "batch_size": config.batch_size})
        scores = self.evaluate(config_eval, val_set)
        score = scores["perplexity"]
        if self.dist is not None:
            # every rank scored its own copy of the validation set with atomically (order-dependently) accumulated statistics:
            # rank 0's number decides, so that score-driven decay / early stopping cannot diverge between ranks
            score = self.dist.broadcast_scalar(score)
        lr_schedule.update(score=score)
        return score

    MRT_KEYS = ("n", "alpha", "temperature", "top_k", "top_p", "on_device", "cost")

    @staticmethod
    def _check_cost(what, cost):
        """the cost a minimum-risk step or a consensus optimises: "edit" (the edit distance) or "bleu" (1 - sentence BLEU, evaluation/text.py)"""
        if not isinstance(cost, str) or cost not in ("edit", "bleu"):
            raise ValueError("%s must be \"edit\" or \"bleu\", got %r" % (what, cost))
        return cost

    def _run_train_mrt(self, config, train_set, val_set, epoch, lr_schedule, mrt, keep):
        """One epoch of minimum-risk training: the training config's optional "mrt": {"n", "alpha", "temperature", "top_k", "top_p", "on_device",
        "cost"} key makes every batch one mrt_batch instead of one cross-entropy step; the sampling seed is the step counter.  Single process; the feed is the
        synchronous one (the candidates are built from the batch's own formulas: on the host, or with "on_device": true by Engine.mrt_sample_step).
        The epoch ends as _run_train's does."""
        if self.dist is not None:
            raise NotImplementedError("minimum-risk training (the training config's \"mrt\" key) runs in a single process: the data-parallel "
                                      "mrt_step is not built -- train with one GPU, or drop the key")
        mrt = dict(mrt) if isinstance(mrt, dict) else {k: getattr(mrt, k) for k in self.MRT_KEYS if hasattr(mrt, k)}
        unknown = sorted(set(mrt) - set(self.MRT_KEYS))
        if unknown:
            raise ValueError("training config: unknown key(s) %s under \"mrt\" (known: %s)" % (unknown, list(self.MRT_KEYS)))
        batch_size = config.batch_size
        nbatches = (len(train_set) + batch_size - 1) // batch_size
        prog = Progbar(nbatches)
        for i, (img, formula) in enumerate(minibatches(train_set, batch_size)):
            out = self.mrt_batch(img, formula, lr_schedule.lr, seed=epoch * nbatches + i, dropout=keep, **mrt)
            prog.update(i + 1, [("risk", out["risk"]), ("lr", lr_schedule.lr)])
            lr_schedule.update(batch_no=epoch * nbatches + i)
        self.logger.info("- Training (minimum risk): {}".format(prog.info))
        scores = self.evaluate(Config({"dir_answers": self._dir_output + "formulas_val/", "batch_size": config.batch_size}), val_set)
        lr_schedule.update(score=scores["perplexity"])
        return scores["perplexity"]

    def mrt_batch(self, images, formulas, lr, n=5, alpha=0.005, temperature=1.0, top_k=0, top_p=1.0, seed=0, include_reference=True, dropout=1,
                  on_device=False, cost="edit"):
        """One minimum-risk training step on a batch (Engine.mrt_step): the model draws n transcriptions per image (Engine.sample_decode with
        temperature / top_k / top_p / seed); an image's candidates are its DISTINCT draws, each cut at its first END, and -- include_reference --
        its reference formula; a candidate costs levenshtein(candidate, reference) / max(len(reference), 1) (evaluation/text.py, the edit distance
        the model is evaluated with); the step then lowers the expected cost under softmax(alpha * log p(candidate | image)) over each image's
        candidates.  formulas: token-id lists or space-separated token strings, as score_batch takes them.
        on_device: the same candidates, costs and step through Engine.mrt_sample_step -- the draws are cut, compared and costed by device kernels and
        never visit the host; the default builds them here, as ever.
        cost = "bleu": a candidate costs 1 - sentence BLEU against the reference (evaluation/text.py sentence_bleu_cost on the host path,
        lxo_mrt_candidates_cost on the device path; the two agree within 1e-5) in place of the edit distance.
        -> {"risk": the mean expected cost before the update, "candidates": per image [{"text", "q": its probability among the candidates, "cost"}]}"""
        if len(images) != len(formulas):
            raise ValueError("mrt_batch: %d images but %d formulas" % (len(images), len(formulas)))
        self._check_cost("mrt_batch: cost", cost)
        prepro = self._vocab.form_prepro
        refs = [tuple(prepro(f)) if isinstance(f, str) else tuple(int(x) for x in f) for f in formulas]
        id_end = self._vocab.id_end
        img = pad_batch_images(images)
        tok = self._vocab.id_to_tok
        if on_device:
            f, ln = pad_batch_formulas([list(r) for r in refs], self._vocab.id_pad, id_end)
            risk, info = self.engine.mrt_sample_step(img, f, ln, id_end, self._vocab.id_pad, lr, alpha, n=n, temperature=temperature, top_k=top_k, top_p=top_p,
                                                     seed=seed, include_reference=include_reference,
                                                     max_iter=getattr(self._config, "max_length_formula", 150) + 1, clip=getattr(self, "_clip", -1),
                                                     dropout=dropout, **({} if cost == "edit" else {"cost": cost}))
            out, at = [], 0
            for m in info["group_sizes"]:
                out.append([{"text": " ".join(tok[int(i)] for i in info["cand"][r, :info["cand_lengths"][r] - 1]), "q": float(info["q"][r]),
                             "cost": float(info["cost"][r])} for r in range(at, at + int(m))])
                at += int(m)
            return {"risk": risk, "candidates": out}
        ids = self.engine.sample_decode(img, id_end, n=n, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                        max_iter=getattr(self._config, "max_length_formula", 150) + 1)
        cands, sizes, costs = [], [], []
        for b, ref in enumerate(refs):
            mine = [ref] if include_reference else []
            for j in range(ids.shape[2]):
                c = tuple(int(x) for x in truncate_end(ids[b, :, j], id_end))
                if c not in mine:
                    mine.append(c)
            cands += mine
            sizes.append(len(mine))
            costs += [sentence_bleu_cost(c, ref) if cost == "bleu" else levenshtein(c, ref) / float(max(len(ref), 1)) for c in mine]
        f, ln = pad_batch_formulas([list(c) for c in cands], self._vocab.id_pad, id_end)
        risk, q = self.engine.mrt_step(img, f, ln, np.asarray(sizes), np.asarray(costs, np.float32), lr, alpha,
                                       clip=getattr(self, "_clip", -1), dropout=dropout)
        out, at = [], 0
        for m in sizes:
            out.append([{"text": " ".join(tok[i] for i in cands[at + k]), "q": float(q[at + k]), "cost": float(costs[at + k])} for k in range(m)])
            at += m
        return {"risk": risk, "candidates": out}

    def _run_evaluate(self, config, test_set):
        """Reference: model/img2seq.py:198-213.  With `metrics_on_device` true in the config it is given, the text metrics come from the decoded ids
        through score_ids (the files are written all the same): the same dict."""
        if getattr(config, "metrics_on_device", False):
            files, perp, (refs, hyps) = self.write_prediction(config, test_set, return_ids=True)
            scores = self.score_ids(refs, hyps[0])
        else:
            files, perp = self.write_prediction(config, test_set)
            scores = score_files(files[0], files[1])
        scores["perplexity"] = perp
        return scores

    SCORE_IDS_BATCH = 256

    def score_ids(self, references, hypotheses, per_sample=False):
        """score_files' dict -- {"BLEU-4", "ExactMatchScore", "EditDistance"} x 100 -- from token ids, on the device: references and hypotheses are
        lists of id sequences, pair by pair, each cut at the vocabulary's END.  The pairs go through Engine.text_stats in batches of SCORE_IDS_BATCH
        with ONE accumulator on the device and one copy of its 14 integers at the end; per_sample=True also returns the int32 [N, 12] rows
        (include/lxo.h: lxo_text_stats), -> (dict, rows).
        The dict EQUALS score_files' on the files write_answers writes from the same ids, for a vocabulary whose token strings are distinct,
        non-empty and free of whitespace (then equal ids are equal strings and a line splits back into its tokens).  One quirk is kept: an empty
        sequence is written as an empty line, which score_files reads as ONE token ("".split(" ") is [""]) -- so it has length 1, and an empty
        hypothesis equals an empty reference token for token.  An empty cut sequence is therefore mapped to the single id n_tok (one past the
        vocabulary, equal to no token) on both sides before the call."""
        from .evaluation.text import scores_from_counts
        if len(references) != len(hypotheses):
            raise ValueError("score_ids: %d references but %d hypotheses" % (len(references), len(hypotheses)))
        id_end, empty = self._vocab.id_end, [self._vocab.n_tok]
        eng = self.engine
        corpus, rows = None, []                                   # (the first batch's call makes the accumulator, the others add into it)
        for at in range(0, len(references), self.SCORE_IDS_BATCH):
            sides = []
            for seqs in (hypotheses[at:at + self.SCORE_IDS_BATCH], references[at:at + self.SCORE_IDS_BATCH]):
                cut = [truncate_end([int(i) for i in s], id_end) or empty for s in seqs]
                ln = np.array([len(c) for c in cut], np.int32)
                a = np.zeros((len(cut), int(ln.max())), np.int32)
                for i, c in enumerate(cut):
                    a[i, :len(c)] = c
                sides += [a, ln]
            stats, corpus = eng._text_stats_device("score_ids", sides[0], sides[2], sides[1], sides[3], None, None, per_sample, corpus, 1)
            rows.append(stats)
        scores = scores_from_counts([0] * 14 if corpus is None else corpus.cpu().numpy())
        if not per_sample:
            return scores
        return scores, (np.concatenate([r.cpu().numpy() for r in rows]) if rows else np.zeros((0, 12), np.int32))

    def error_analysis(self, references, hypotheses, per_sample=False, top=20):
        """The error breakdown of hypotheses against references, on the device: substitution, insertion and deletion counts and rates, the most
        frequent confusions, the tokens most often dropped and inserted, the tokens of lowest recall -- evaluation/text.py error_report's dict.
        references and hypotheses are lists of id sequences, pair by pair, each cut at the vocabulary's END.  The pairs go through
        Engine.edit_align (include/lxo.h: lxo_edit_align holds the alignment's definition) in batches of SCORE_IDS_BATCH into ONE corpus row and
        ONE confusion matrix on the device, copied once at the end.  per_sample=True: -> (dict, counts, hyp_maps, ref_maps) with counts int32
        [N, 6] = matches, substitutions, insertions, deletions, |h|, |r| and the two maps as lists of lists: per hypothesis position the reference
        position it is aligned with or -1 (inserted), per reference position the hypothesis position or -1 (deleted).
        score_ids' empty-line quirk does NOT apply here: an empty sequence is empty -- it aligns with nothing, and every token of the other side is
        an insertion or a deletion."""
        from .evaluation.text import error_report
        if len(references) != len(hypotheses):
            raise ValueError("error_analysis: %d references but %d hypotheses" % (len(references), len(hypotheses)))
        id_end, V = self._vocab.id_end, self._vocab.n_tok
        eng = self.engine
        corpus = confusion = True                                  # (the first batch's call makes the two accumulators, the others add into them)
        rows, hmaps, rmaps = [], [], []
        for at in range(0, len(references), self.SCORE_IDS_BATCH):
            sides = []
            for seqs in (hypotheses[at:at + self.SCORE_IDS_BATCH], references[at:at + self.SCORE_IDS_BATCH]):
                cut = [truncate_end([int(i) for i in s], id_end) for s in seqs]
                ln = np.array([len(c) for c in cut], np.int32)
                a = np.zeros((len(cut), max(int(ln.max()), 1)), np.int32)
                for i, c in enumerate(cut):
                    a[i, :len(c)] = c
                sides += [a, ln]
            ha, ra, counts, corpus, confusion = eng._edit_align_device("error_analysis", sides[0], sides[2], sides[1], sides[3], None, None, per_sample,
                                                                       per_sample, corpus, confusion)
            if per_sample:
                rows.append(counts)
                hmaps.append((ha, sides[1]))
                rmaps.append((ra, sides[3]))
        if corpus is True:                                         # no pair
            report = error_report([0] * 8, [0] * ((V + 1) * (V + 1)), self._vocab.id_to_tok, top)
        else:
            report = error_report(corpus.cpu().numpy(), confusion.cpu().numpy(), self._vocab.id_to_tok, top)
        if not per_sample:
            return report
        cut_rows = lambda maps: [[int(x) for x in row[:n]] for t, ln in maps for row, n in zip(t.cpu().numpy(), ln)]
        counts = np.concatenate([r.cpu().numpy() for r in rows]) if rows else np.zeros((0, 6), np.int32)
        return report, counts, cut_rows(hmaps), cut_rows(rmaps)

    def _beam_kwargs(self):
        """The diversity-penalty arguments of one Engine.beam_decode call (decoder.py:67-68); the seed is the number of beam decodes so far."""
        cfg = self._config
        self._div_calls = getattr(self, "_div_calls", 0) + 1
        return dict(div_gamma=getattr(cfg, "div_gamma", 1), div_prob=getattr(cfg, "div_prob", 0), div_seed=self._div_calls)

    def _token_sets(self, n_images, banned, allowed):
        """The allowed= argument of the Engine decodes from banned / allowed token lists: token strings or ids, one list for all images or
        one list per image.  `banned` is the complement form; given both, a token must be allowed and not banned.  Unknown token strings
        raise (a whitelist that silently drops a symbol is worse than none).  -> bool [V] or [B, V], None for no constraint."""
        if banned is None and allowed is None:
            return None
        V = self._vocab.n_tok

        def ids_of(toks):
            out = []
            for t in toks:
                if isinstance(t, str):
                    if t not in self._vocab.tok_to_id:
                        raise ValueError("unknown token %r" % t)
                    out.append(self._vocab.tok_to_id[t])
                else:
                    if not 0 <= int(t) < V:
                        raise ValueError("token id %d outside [0, %d)" % (int(t), V))
                    out.append(int(t))
            return out

        def mask(toks, fill):
            toks = list(toks)
            per_image = len(toks) > 0 and all(isinstance(t, (list, tuple, np.ndarray)) for t in toks)
            if per_image and len(toks) != n_images:
                raise ValueError("%d per-image token lists for %d images" % (len(toks), n_images))
            m = np.full((n_images if per_image else 1, V), not fill, bool)
            for b, row in enumerate(toks if per_image else [toks]):
                m[b, ids_of(row)] = fill
            return m
        m = mask(allowed, True) if allowed is not None else np.ones((1, V), bool)
        if banned is not None:
            m = m & mask(banned, False)
        return m[0] if m.shape[0] == 1 else m

    def _grammar(self, grammar):
        """grammar= of predict_batch / complete_batch / sample_batch: a latex_ocr_amd.grammar.Grammar, True for Grammar.latex(vocab), or
        None / False for none -> {} or the Engine decodes' grammar keyword"""
        if grammar is None or grammar is False:
            return {}
        if grammar is True:
            from ..grammar import Grammar
            grammar = Grammar.latex(self._vocab)
        return {"grammar": grammar}

    def _decode(self, img, allowed=None):
        """pred_test.ids of the decode graph (decoder.py:60-70), shaped [B, k, T'] as after
        img2seq.py:238-241."""
        cfg = self._config
        max_iter = getattr(cfg, "max_length_formula", 150) + 1          # decoder.py:70
        if getattr(cfg, "decoding", "greedy") == "beam_search":
            ids, par = self.engine.beam_decode(img, self._vocab.id_end, cfg.beam_size, max_iter=max_iter, return_parents=True,
                                               allowed=allowed, **self._beam_kwargs())
            if getattr(cfg, "beam_backtrace", False):      # extension: follow parents (the reference never does, quirk C-1)
                from .utils.text import beam_backtrace
                ids = beam_backtrace(ids, par)
            return np.transpose(ids, [0, 2, 1])
        ids = self.engine.greedy_decode(img, self._vocab.id_end, max_iter=max_iter, allowed=allowed)
        return np.expand_dims(ids, axis=1)

    def write_prediction(self, config, test_set, return_ids=False):
        """Reference: model/img2seq.py:215-254.  perplexity is NEGATED (quirk C-2).  return_ids: -> (files, perplexity, (refs, hyps)) with the id
        sequences the files were written from, hyps[i] the hypotheses of rank i."""
        k = self._config.beam_size if getattr(self._config, "decoding", "greedy") == "beam_search" else 1
        refs, hyps = [], [[] for _ in range(k)]
        n_words, ce_words = 0, 0.0
        for img, formula in minibatches(test_set, config.batch_size):
            fd = self._get_feed_dict(img, formula=formula, dropout=1)
            ce, n = self.engine.evaluate_batch(fd["img"], fd["formula"], fd["formula_length"])
            ids_eval = self._decode(fd["img"])
            n_words += n
            ce_words += ce
            for form, preds in zip(formula, ids_eval):
                refs.append(form)
                for i, pred in enumerate(preds):
                    hyps[i].append(pred)
        files = write_answers(refs, hyps, self._vocab.id_to_tok, config.dir_answers, self._vocab.id_end)
        perp = -np.exp(ce_words / float(n_words))
        if return_ids:
            return files, perp, (refs, hyps)
        return files, perp

    def predict_batch(self, images, return_scores=False, banned=None, allowed=None, alternatives=0, grammar=None):
        """Reference: model/img2seq.py:256-276.
        return_scores: -> (hyps, scores), scores[i][b] = (sequence log-prob, [log-prob of each token up to and including the first END]) of
        hypothesis hyps[i][b]; the sequence log-prob is the sum of the token log-probs.  Greedy: the hypotheses are the default call's.
        Beam search: the hypotheses are the back-traced ones (utils/text.beam_backtrace) whatever config.beam_backtrace says -- the final
        running log-prob of slot i belongs to the token path that ends in slot i, not to the per-step columns of the reference's read-out
        (quirk C-1) -- and a token's log-prob is the difference of the running scores along that path (with the diversity penalty on, the
        penalised scores).
        banned / allowed: a token constraint (Engine greedy_decode / beam_decode with allowed=): token strings or ids, one list for all
        images or one list per image; a token outside an image's set is never emitted and the scores are renormalised over the set.
        END must stay allowed.  E.g. banned=["_UNK", "_PAD"].  Nothing is banned by default.
        alternatives = k > 0: -> (hyps, scores, alts), hyps and scores as with return_scores, alts[i][b] = one entry per emitted token of
        hyps[i][b] (the first END included), as score_batch(alternatives=k) lists them: the model's k best tokens there, the emitted
        token's rank and the step's entropy, under the same token sets.  They come from a SECOND, teacher-forced pass over the emitted
        tokens (Engine.score, one per hypothesis slot), not from the decode itself: at a near-tie the slot-0 token of that pass may
        differ from the emitted one, and in beam search the log-probs are the model's, not the (penalised) running scores the search
        ranked by.  A path that ran into the length bound without END has no entry for an END it never emitted.
        grammar: a latex_ocr_amd.grammar.Grammar, or True for Grammar.latex(vocab) (Engine decodes with grammar=): every hypothesis closes the
        delimiters it opens and ends inside the length bound.  Beam search then returns the back-traced hypotheses, as with return_scores: the
        grammar holds along a hypothesis' own path, not along the per-step columns of the reference's read-out.  The alternatives of a
        grammar call run under the static sets only."""
        sets = self._token_sets(len(images), banned, allowed)
        gk = self._grammar(grammar)
        if alternatives:
            return self._predict_scored(images, allowed=sets, alternatives=alternatives, **gk)
        if return_scores:
            return self._predict_scored(images, allowed=sets, **gk)
        if gk:
            return self._predict_scored(images, allowed=sets, **gk)[0]
        fd = self._get_feed_dict(images, dropout=1)
        ids_eval = self._decode(fd["img"], sets)
        hyps = [[] for _ in range(ids_eval.shape[1])]
        for preds in ids_eval:
            for i, pred in enumerate(preds):
                p = truncate_end(pred, self._vocab.id_end)
                hyps[i].append(" ".join(self._vocab.id_to_tok[int(idx)] for idx in p))
        return hyps

    def _alt_entries(self, alt, b, n):
        """positions [0, n) of row b of an Engine.score Alternatives as [{"rank", "entropy", "alternatives": [(token string, logp), ...]}]
        (a slot beyond a row's allowed tokens, id -1, is left out)"""
        tok = self._vocab.id_to_tok
        return [{"rank": int(alt.rank[b, t]), "entropy": float(alt.entropy[b, t]),
                 "alternatives": [(tok[int(i)], float(lp)) for i, lp in zip(alt.ids[b, t], alt.logp[b, t]) if i >= 0]} for t in range(n)]

    def _teacher_targets(self, teachers, k, img, f, ln):
        """The soft targets of a padded batch, on the device: every teacher's k best tokens per position (Engine.score_alternatives_dev) side by side
        along the last axis, their probabilities divided by the number of teachers -- lxo_ce_loss_soft adds up the slots that name the same token,
        so the target is the average of the teachers' sparse distributions -> (ids [B, T, k M], p [B, T, k M])"""
        import torch
        M = len(teachers)
        if not (M >= 1 and int(k) >= 1 and int(k) * M <= 16):
            raise ValueError("distill_batch: k = %r with %d teacher(s): k must be >= 1 and k * teachers <= 16" % (k, M))
        for t in teachers:
            if t.engine.n_tok != self.engine.n_tok:
                raise ValueError("distill_batch: a teacher's vocabulary has %d tokens, this model's %d" % (t.engine.n_tok, self.engine.n_tok))
        dev = self.engine.device
        outs = [t.engine.score_alternatives_dev(img, f, ln, int(k)) for t in teachers]
        ids = [o[0].to(dev) for o in outs]
        p = [torch.exp(o[1].to(dev)) / float(M) if M > 1 else torch.exp(o[1].to(dev)) for o in outs]
        return (ids[0], p[0]) if M == 1 else (torch.cat(ids, dim=2), torch.cat(p, dim=2))

    def distill_batch(self, images, formulas, lr, teacher, k=5, weight=0.5, dropout=1):
        """One training step against a teacher's soft targets (Engine.train_step(soft_targets=, soft_weight=weight)): teacher is an Img2SeqModel or a
        list of M of them, k * M <= 16, with this model's vocabulary size.  Each teacher scores the same padded batch teacher-forced and hands over
        its k best tokens per position with their probabilities; what they leave of 1 is spread over the vocabulary, several teachers are averaged,
        and the step minimises (1 - weight) * (the cross-entropy, smoothed if the training config says so) + weight * (the cross-entropy against the
        teachers' distribution).  The targets never visit the host.  formulas: token-id lists or space-separated token strings, as score_batch takes
        them.  -> the loss the step optimised (Engine.last_ce keeps the plain cross-entropy)."""
        if len(images) != len(formulas):
            raise ValueError("distill_batch: %d images but %d formulas" % (len(images), len(formulas)))
        teachers = list(teacher) if isinstance(teacher, (list, tuple)) else [teacher]
        prepro = self._vocab.form_prepro
        forms = [prepro(f) if isinstance(f, str) else [int(x) for x in f] for f in formulas]
        fd = self._get_feed_dict(images, formula=forms, dropout=dropout)
        img, f, ln = fd["img"], fd["formula"], fd["formula_length"]
        eps = getattr(self, "_label_smoothing", 0.0)
        return self.engine.train_step(img, f, ln, lr, clip=getattr(self, "_clip", -1), dist=self.dist, dropout=dropout,
                                      soft_targets=self._teacher_targets(teachers, k, img, f, ln), soft_weight=weight,
                                      **(dict(label_smoothing=eps) if eps > 0.0 else {}))

    def score_batch(self, images, formulas, alternatives=0, banned=None, allowed=None):
        """Teacher-forced scores of given transcriptions (Engine.score): formulas are token-id lists or space-separated token strings
        (Vocab.form_prepro: unknown tokens -> id_unk), padded as _get_feed_dict pads a training batch, so the END the reference appends is
        scored too.  -> one (sequence log-prob, [token log-probs incl. END], first position where the model's top-1 differs from the
        formula or -1) per (image, formula) pair.
        alternatives = k > 0 (Engine.score(alternatives=k)): each tuple gains a 4th element, one entry per scored position, the appended END
        included: {"rank": the given token's rank among the model's choices (0 = its top-1), "entropy": of the step, in nats,
        "alternatives": [(token string, log-prob), ... k], best first}.  banned / allowed (with alternatives only): token sets as in
        predict_batch; the alternatives, ranks and entropies then run over each image's allowed tokens (a banned given token: rank -1, fewer
        than k allowed: a shorter list), the first three elements stay the unconstrained scores."""
        if len(images) != len(formulas):
            raise ValueError("score_batch: %d images but %d formulas" % (len(images), len(formulas)))
        prepro = self._vocab.form_prepro
        forms = [prepro(f) if isinstance(f, str) else [int(x) for x in f] for f in formulas]
        fd = self._get_feed_dict(images, formula=forms, dropout=1)
        f, ln = fd["formula"], fd["formula_length"]
        res = self.engine.score(fd["img"], f, ln, return_top1=True, alternatives=int(alternatives),
                                allowed=self._token_sets(len(images), banned, allowed))
        logp, top1, seq = res[:3]
        out = []
        for b in range(len(forms)):
            n = int(ln[b])
            diff = np.flatnonzero(top1[b, :n] != f[b, :n])
            out.append((float(seq[b]), [float(x) for x in logp[b, :n]], int(diff[0]) if diff.size else -1)
                       + ((self._alt_entries(res[3], b, n),) if alternatives else ()))
        return out

    def complete_batch(self, images, prefixes, return_scores=False, banned=None, allowed=None, alternatives=0, grammar=None):
        """Decode each image from a given prefix (Engine greedy_decode / beam_decode with prefix=): the prefixes are token-id lists or
        space-separated token strings (Vocab.form_prepro, as score_batch takes them, but no END is appended), one per image; "" or []
        decodes from the start.  config.decoding chooses greedy or beam search; beam hypotheses are the back-traced ones, as
        predict_batch(return_scores=True) returns them.  -> hyps (hyps[i][b]: hypothesis i of image b, its prefix included), or
        (hyps, scores) with return_scores, scores as in predict_batch (the forced tokens' log-probs included).
        banned / allowed: as in predict_batch ("and not that token again"); a prefix token must be allowed for its image.
        alternatives = k > 0: -> (hyps, scores, alts) as in predict_batch (a second, teacher-forced pass; the forced tokens' positions included).
        grammar: as in predict_batch; the prefix itself must obey it (a ValueError otherwise)."""
        if len(images) != len(prefixes):
            raise ValueError("complete_batch: %d images but %d prefixes" % (len(images), len(prefixes)))
        prepro = self._vocab.form_prepro
        forms = [(prepro(f) if f.strip() else []) if isinstance(f, str) else [int(x) for x in f] for f in prefixes]      # "": no token
        ln = np.array([len(f) for f in forms], np.int32)
        pf = np.zeros((len(forms), max(1, int(ln.max()) if ln.size else 1)), np.int32)
        for b, f in enumerate(forms):
            pf[b, :len(f)] = f
        out = self._predict_scored(images, pf, ln, self._token_sets(len(images), banned, allowed), alternatives=alternatives, **self._grammar(grammar))
        return out if return_scores or alternatives else out[0]

    def _predict_scored(self, images, prefix=None, prefix_lengths=None, allowed=None, alternatives=0, **gk):
        fd = self._get_feed_dict(images, dropout=1)
        cfg = self._config
        max_iter = getattr(cfg, "max_length_formula", 150) + 1
        id_end = self._vocab.id_end
        if getattr(cfg, "decoding", "greedy") == "beam_search":
            from .utils.text import beam_backtrace
            ids, par, sc = self.engine.beam_decode(fd["img"], id_end, cfg.beam_size, max_iter=max_iter, return_scores=True,
                                                   prefix=prefix, prefix_lengths=prefix_lengths, allowed=allowed, **dict(self._beam_kwargs(), **gk))
            ids, run = beam_backtrace(ids, par), beam_backtrace(sc, par)          # token paths and their running log-probs
            tok = np.diff(run, axis=1, prepend=0.0)
        else:
            ids, tok = self.engine.greedy_decode(fd["img"], id_end, max_iter=max_iter, return_scores=True, prefix=prefix,
                                                 prefix_lengths=prefix_lengths, allowed=allowed, **gk)
            ids, tok = ids[:, :, None], tok[:, :, None]
        k = ids.shape[2]
        hyps, scores = [[] for _ in range(k)], [[] for _ in range(k)]
        emitted = np.zeros((ids.shape[0], k), np.int32)             # tokens of each path up to and including its first END
        for b in range(ids.shape[0]):
            for i in range(k):
                path = ids[b, :, i]
                end = np.flatnonzero(path == id_end)
                n = emitted[b, i] = int(end[0]) + 1 if end.size else len(path)
                lp = [float(x) for x in tok[b, :n, i]]
                hyps[i].append(" ".join(self._vocab.id_to_tok[int(idx)] for idx in truncate_end(path, id_end)))
                scores[i].append((float(np.sum(np.asarray(lp, dtype=np.float64))), lp))
        if not alternatives:
            return hyps, scores
        alts = []
        for i in range(k):                                           # one teacher-forced pass per hypothesis slot, over what it emitted
            T = max(1, int(emitted[:, i].max()))
            f = np.where(np.arange(T)[None, :] < emitted[:, i, None], ids[:, :T, i], id_end).astype(np.int32)
            alt = self.engine.score(fd["img"], f, emitted[:, i], alternatives=int(alternatives), allowed=allowed)[-1]
            alts.append([self._alt_entries(alt, b, int(emitted[b, i])) for b in range(ids.shape[0])])
        return hyps, scores, alts

    def sample_batch(self, images, n, temperature=1.0, top_k=0, top_p=1.0, seed=0, banned=None, allowed=None, grammar=None, consensus=False,
                     consensus_cost="edit"):
        """n sampled transcriptions per image (Engine.sample_decode), folded into their DISTINCT hypotheses: -> one dict per image,
        {"hypotheses": [{"text", "count", "logp": the model's sequence log-prob (sum of the token log-probs through END), "token_logp": [...]},
        ...] sorted by count, then log-prob, both descending, "agreement": top count / n}.  A hypothesis is a draw truncated at its first END; draws
        that agree share one entry (the log-probs of its first draw).  Agreement is a confidence: n draws that all say the same are a stronger
        accept signal than the greedy path's mean token probability, and the top entry is the vote.  banned / allowed / grammar: as in predict_batch
        (under a grammar no draw is lost to an unbalanced formula).
        consensus: the minimum-risk choice among the draws on top of the vote (Engine.sample_decode(return_consensus=True): the n draws with
        uniform weights, so a hypothesis weighs by its count): every hypothesis gains "risk", its expected edit distance (over the length of the
        other side) to the image's draws, and every image "consensus", the index into "hypotheses" of the one of least risk, and "expected_cost",
        that risk -- a confidence that still tells hypotheses apart where every draw is distinct and every count 1.  Nothing else changes.
        consensus_cost = "bleu": the risk is the expected 1 - sentence BLEU against the image's draws (Engine.consensus(cost="bleu"))."""
        self._check_cost("sample_batch: consensus_cost", consensus_cost)
        fd = self._get_feed_dict(images, dropout=1)
        max_iter = getattr(self._config, "max_length_formula", 150) + 1
        id_end = self._vocab.id_end
        res = self.engine.sample_decode(fd["img"], id_end, n=n, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, max_iter=max_iter,
                                        return_scores=True, allowed=self._token_sets(len(images), banned, allowed), return_consensus=bool(consensus),
                                        **dict(self._grammar(grammar), **({} if consensus_cost == "edit" else {"consensus_cost": consensus_cost})))
        ids, logp = res[:2]
        best, risk = res[3:] if consensus else (None, None)
        out = []
        for b in range(ids.shape[0]):
            seen, entry = {}, []
            for j in range(ids.shape[2]):
                path = ids[b, :, j]
                end = np.flatnonzero(path == id_end)
                m = int(end[0]) + 1 if end.size else len(path)
                key = tuple(int(x) for x in truncate_end(path, id_end))
                if key in seen:
                    seen[key]["count"] += 1
                    entry.append(seen[key])
                    continue
                lp = [float(x) for x in logp[b, :m, j]]
                seen[key] = {"text": " ".join(self._vocab.id_to_tok[i] for i in key), "count": 1,
                             "logp": float(np.sum(np.asarray(lp, dtype=np.float64))), "token_logp": lp}
                if consensus:
                    seen[key]["risk"] = float(risk[b, j])
                entry.append(seen[key])
            hyps = sorted(seen.values(), key=lambda h: (-h["count"], -h["logp"]))
            out.append({"hypotheses": hyps, "agreement": hyps[0]["count"] / float(ids.shape[2])})
            if consensus:
                k = [i for i, h in enumerate(hyps) if h is entry[int(best[b])]][0]
                out[-1].update(consensus=k, expected_cost=hyps[k]["risk"])
        return out

    def nbest_batch(self, images, length_penalty=0.0, coverage_penalty=0.0, consensus=False, consensus_cost="edit", banned=None, allowed=None,
                    grammar=None):
        """The beam's k hypotheses per image, finished on the device and reranked (Engine.beam_decode(return_nbest=True): the back-trace, the cut
        at END, the scores and the rerank run before anything is copied).  config.decoding must be "beam_search".  -> one dict per image,
        {"hypotheses": [{"text", "slot": the beam slot the path ends in, "length": its tokens through END, "logp": its frozen beam score,
        "token_logp": [...], "score": logp / ((5 + length) / 6)^length_penalty + coverage_penalty * sum over the feature cells of
        log(min(max(coverage, floor), 1)) (GNMT's normalisation of the finished beam; the search itself is the reference's), "posterior": the
        softmax of logp over the image's k slots}, ...] in descending score}.  length_penalty = coverage_penalty = 0: the order of logp.
        consensus: every hypothesis gains "risk", its expected cost (consensus_cost "edit": edit distance over the other side's length, "bleu":
        1 - sentence BLEU) against the k hypotheses weighted with their posteriors, and every image "consensus", the index into "hypotheses" of the
        one of least risk, and "expected_cost", that risk.  banned / allowed / grammar: as in predict_batch."""
        cfg = self._config
        if getattr(cfg, "decoding", "greedy") != "beam_search":
            raise ValueError("nbest_batch needs config.decoding = \"beam_search\", got %r" % (getattr(cfg, "decoding", "greedy"),))
        self._check_cost("nbest_batch: consensus_cost", consensus_cost)
        fd = self._get_feed_dict(images, dropout=1)
        id_end = self._vocab.id_end
        res = self.engine.beam_decode(fd["img"], id_end, cfg.beam_size, max_iter=getattr(cfg, "max_length_formula", 150) + 1, return_nbest=True,
                                      length_penalty=length_penalty, coverage_penalty=coverage_penalty, return_consensus=bool(consensus),
                                      consensus_cost=consensus_cost, allowed=self._token_sets(len(images), banned, allowed),
                                      **dict(self._beam_kwargs(), **self._grammar(grammar)))
        nb = res[1]
        best, risk = res[2:4] if consensus else (None, None)
        out = []
        for b in range(nb.hyp.shape[0]):
            hyps = []
            for i in (int(x) for x in nb.order[b]):
                n = int(nb.lengths[b, i])
                h = {"text": " ".join(self._vocab.id_to_tok[int(t)] for t in truncate_end(nb.hyp[b, :n, i], id_end)), "slot": i, "length": n,
                     "logp": float(nb.seq_logp[b, i]), "token_logp": [float(x) for x in nb.tok_logp[b, :n, i]], "score": float(nb.score[b, i]),
                     "posterior": float(nb.post[b, i])}
                if consensus:
                    h["risk"] = float(risk[b, i])
                hyps.append(h)
            out.append({"hypotheses": hyps})
            if consensus:
                j = [x["slot"] for x in hyps].index(int(best[b]))
                out[-1].update(consensus=j, expected_cost=hyps[j]["risk"])
        return out

    def locate_batch(self, images, formulas=None, mass=0.9):
        """WHERE in its image each token is (Engine.attention_locate, reduced on the device: the attention maps never visit the host).
        formulas given (token-id lists or token strings, as score_batch takes them): teacher-forced, the given transcription's tokens with the
        appended END (Engine.score(locate=True)).  Without: the tokens of what config.decoding decodes, through the first END -- greedy, or the
        back-traced best beam hypothesis (Engine greedy_decode / beam_decode with return_boxes=True).
        -> per image {"tokens": [{"token", "box": (left, top, right, bottom) in pixels of the network's input (the padded batch canvas), right
        and bottom exclusive (utils/image.feature_box_to_pixels), "centre": (x, y) and "spread": (sx, sy) in pixels (the feature cell's core is 8
        pixels wide and starts at 8 (c + 1)), "inside": the share of the map within the box, "peak_share"}, ...], "coverage": f32 [H', W'], the
        token maps added up, "max_coverage": its largest cell -- above 1 a region was attended for more than one token's worth, the mark of a
        loop -- and "uncovered": the share of its cells below 1 / R^2, R = H' W'}.  The geometry is the default encoder's; encoder_cnn = "cnn" raises."""
        from .utils.image import feature_box_to_pixels
        enc = getattr(self._config, "encoder_cnn", "vanilla")
        feature_box_to_pixels((0, 0, 0, 0), 8, 8, enc)              # refuses the geometry it does not know before anything runs
        cfg, end = self._config, self._vocab.id_end
        if formulas is not None:
            if len(images) != len(formulas):
                raise ValueError("locate_batch: %d images but %d formulas" % (len(images), len(formulas)))
            prepro = self._vocab.form_prepro
            forms = [prepro(f) if isinstance(f, str) else [int(x) for x in f] for f in formulas]
            fd = self._get_feed_dict(images, formula=forms, dropout=1)
            ids = fd["formula"]
            loc = self.engine.score(fd["img"], ids, fd["formula_length"], locate=True, mass=mass, coverage=True)[-1]
            peak, box, stats, cov = loc
        else:
            fd = self._get_feed_dict(images, dropout=1)
            max_iter = getattr(cfg, "max_length_formula", 150) + 1
            if getattr(cfg, "decoding", "greedy") == "beam_search":
                from .utils.text import beam_backtrace
                out = self.engine.beam_decode(fd["img"], end, cfg.beam_size, max_iter=max_iter, return_boxes=True, mass=mass, coverage=True,
                                              **self._beam_kwargs())
                ids = beam_backtrace(out[0], out[1])[:, :, 0]
                peak, box, stats, cov = (a[:, 0] for a in out[-1])
            else:
                ids, loc = self.engine.greedy_decode(fd["img"], end, max_iter=max_iter, return_boxes=True, mass=mass, coverage=True)
                peak, box, stats, cov = loc
        H, W = int(fd["img"].shape[1]), int(fd["img"].shape[2])
        res = []
        for b in range(len(images)):
            toks = []
            for t in np.flatnonzero(peak[b] >= 0):
                s = stats[b, t]
                toks.append({"token": self._vocab.id_to_tok[int(ids[b, t])], "box": feature_box_to_pixels(box[b, t], H, W, enc),
                             "centre": (8.0 * (float(s[1]) + 1.5), 8.0 * (float(s[2]) + 1.5)), "spread": (8.0 * float(s[3]), 8.0 * float(s[4])),
                             "inside": float(s[6]), "peak_share": float(s[7])})
            R = cov[b].size
            res.append({"tokens": toks, "coverage": cov[b], "max_coverage": float(cov[b].max()), "uncovered": float((cov[b] < 1.0 / (R * R)).mean())})
        return res

    def predict(self, img):
        """Reference: model/img2seq.py:278-285."""
        return [hyp[0] for hyp in self.predict_batch([img])]

    def predict_with_attention(self, img):
        """Best hypothesis of one image plus its per-step attention maps [T', H', W'] -- the data the reference gathers in the global
        `ctx_vector` through tf.py_func (attention_mechanism.py:96-121) for visualize_attention.py -- under WHATEVER config.decoding says
        (the shipped configs/model.json:13-14 decodes with beam_search, k = 2).
        Beam search: the reference's visualiser draws row 0 of the merged batch x beam tensor of every step (`attentionVector[0]`,
        visualize_attention.py:55), for every step the loop ran -- it ends when ALL beams have finished, so there are more slices than tokens
        in the best hypothesis (51 slices for 48 tokens at k = 2); that is what comes back here.  With the
        `beam_backtrace` extension each step's map is the one of the row the back-traced best hypothesis read its token off: walking
        back from slot 0 at the last step, the parent of the path's slot at that step (utils/text.beam_slots)."""
        fd = self._get_feed_dict([img], dropout=1)
        cfg = self._config
        max_iter = getattr(cfg, "max_length_formula", 150) + 1
        if getattr(cfg, "decoding", "greedy") == "beam_search":
            ids, par, alpha = self.engine.beam_decode(fd["img"], self._vocab.id_end, cfg.beam_size, max_iter=max_iter, return_attention=True,
                                                      **self._beam_kwargs())
            if getattr(cfg, "beam_backtrace", False):
                from .utils.text import beam_backtrace, beam_slots
                slot = beam_slots(par)[0, :, 0]
                maps = np.stack([alpha[0, t, par[0, t, slot[t]]] for t in range(alpha.shape[1])])
                ids = beam_backtrace(ids, par)
            else:
                maps = alpha[0, :, 0]
            best = ids[0, :, 0]
        else:
            ids, alpha = self.engine.greedy_decode(fd["img"], self._vocab.id_end, max_iter=max_iter, return_attention=True)
            best, maps = ids[0], alpha[0]
        p = truncate_end(best, self._vocab.id_end)
        return " ".join(self._vocab.id_to_tok[int(i)] for i in p), maps
