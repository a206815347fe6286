"""Device-side engine: owns the flat parameter / gradient / Adam buffers, the packed
compute-dtype weights and the workspace (all torch CUDA tensors -- PyTorch is the
allocator and stream provider only) and drives the C ABI of liblxo.so.

Every numeric operation happens inside liblxo.so (hand-written gfx950 kernels);
there is no eager/PyTorch compute path and no CPU fallback here.
"""
import ctypes
import math
import os
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import _abi
from .model import params as PP


# Engine.score(alternatives=k): per position the k best token ids and their log-probs, the given token's rank and the step's entropy
Alternatives = namedtuple("Alternatives", ["ids", "logp", "rank", "entropy"])
_SoftDev = namedtuple("_SoftDev", ["ids", "p", "k", "lam"])          # soft targets behind their checks: device int32 / f32 [B, T, k], lambda
Alignment = namedtuple("Alignment", ["hyp_align", "ref_align", "counts", "corpus", "confusion"])
Locations = namedtuple("Locations", ["peak", "box", "stats", "coverage"])        # Engine.attention_locate
BeamPaths = namedtuple("BeamPaths", ["hyp", "lengths", "src", "tok_logp", "seq_logp"])                     # Engine.beam_finalize
NBest = namedtuple("NBest", ["hyp", "lengths", "tok_logp", "seq_logp", "score", "post", "order"])         # Engine.beam_decode(return_nbest=True)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _cost_kind(what, cost):
    """the cost of a minimum-risk step or a consensus: "edit" (the edit distance) or "bleu" (1 - sentence BLEU) -> include/lxo.h's LXO_COST_*"""
    if not isinstance(cost, str) or cost not in ("edit", "bleu"):
        raise ValueError("%s: cost must be \"edit\" or \"bleu\", got %r" % (what, cost))
    return _abi.LXO_COST_BLEU if cost == "bleu" else _abi.LXO_COST_EDIT


# include/lxo.h: LXO_XDEC_BLOCK_BYTES (csrc/xdec.h: kXDecBlockBytes) -- ws region "xdec_sync" holds one such block per chain (forward, then
# backward): 4 KB of flag lines, tickets and the error word (word LXO_XDEC_ERR_WORD) + 384 KB of hand-over words (tests/test_abi.py keeps
# the definitions together)
XDEC_BLOCK_BYTES = _abi.LXO_XDEC_BLOCK_BYTES
XDEC_STATUS_WORDS = _abi.LXO_XDEC_ERR_WORD + 1      # the head of a block that tells how its chain went


def _chain_words(w):
    """(used, error) from the first XDEC_STATUS_WORDS int32 words of a chain's block: used = a ticket word of one of the 8 XCDs' lines is
    set (its workgroups took their tickets), error = the error word"""
    return bool(w[32:_abi.LXO_XDEC_ERR_WORD:64].any()), int(w[_abi.LXO_XDEC_ERR_WORD])


class Engine(object):
    def __init__(self, n_tok, dims=None, dtype="bf16", device="cuda:0", seed=0, beam=1, max_steps=0, lib=None, deterministic=None):
        self.lib = lib if lib is not None else _abi.load()
        self.device = torch.device(device)
        if self.device.type != "cuda" and lib is None:
            raise RuntimeError("latex_ocr_amd.Engine needs a CUDA/HIP device (no CPU fallback)")
        self.dims = dict(PP.DEFAULT_DIMS, **(dims or {}))
        self.n_tok = int(n_tok)
        self.dtype = _abi.LXO_BF16 if dtype in ("bf16", 1) else _abi.LXO_F32
        self.beam, self.max_steps = int(beam), int(max_steps)
        # decoder step decomposition (lxo_shape.step_kernels): 0 = automatic (the persistent XCD-local chain of csrc/xdec.hip where the shape
        # qualifies, else the fused step kernels), 2 = always the fused step kernels, 1 = round 1's split-K slab path
        self.step_kernels = int(os.environ.get("LXO_STEP_KERNELS", "0"))
        if self.step_kernels not in (0, 1, 2):
            raise ValueError("LXO_STEP_KERNELS must be 0, 1 or 2 (include/lxo.h: lxo_shape.step_kernels), got %d" % self.step_kernels)
        # bf16 mode only: every reduction of a training step in a fixed order (lxo_shape.deterministic): bit-identical losses, gradients and
        # weights from run to run, for a few per cent of a step.  The f32 parity mode is always deterministic.
        self.deterministic = (os.environ.get("LXO_DETERMINISTIC", "0") == "1") if deterministic is None else bool(deterministic)
        # health of the persistent decoder chains (csrc/xdec.hip): checked synchronously after the first launch that used one (forward and
        # backward separately), then every step WITHOUT a host stall: lxo_chain_guard folds the two error words into the optimizer's scale on
        # the device (a step whose chain did not assemble is dropped, not applied) and copies them into a pinned ring that the next
        # train_step reads (_chain_health_poll); a failure switches this engine to the launch-per-step kernels for good.
        self._xdec_checked = False
        self._xdec_bwd_checked = False
        self.chain_used = False
        self.chain_used_bwd = False
        self.chain_failures = 0           # steps a chain failed in (each was dropped or redone)
        self.last_ce = None               # plain token-mean CE of the last synchronised train_step (whatever loss it optimised)
        self._nochain_shapes, self._nochain_shapes_bwd = set(), set()
        self._health_ring = None
        self._health_i = 0
        self.specs = PP.param_specs(self.n_tok, self.dims)
        self.n_params = PP.n_params(self.n_tok, self.dims)
        probe = self._shape(1, 32, 32, 1)
        assert self.lib.lxo_param_total(ctypes.byref(probe)) == self.n_params
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(self.n_params, **f32)
        self.grads = torch.zeros(self.n_params, **f32)
        self.adam_m = torch.zeros(self.n_params, **f32)
        self.adam_v = torch.zeros(self.n_params, **f32)
        self.adam_t = 0
        self.scale = torch.zeros(_abi.LXO_GNORM_FLOATS, **f32)      # {scale, norm, per-workgroup partial sums} of lxo_global_norm_scale
        self.wpack = torch.zeros(self.lib.lxo_wpack_bytes(ctypes.byref(probe)) + 256, dtype=torch.uint8, device=self.device)
        self.ws = None
        self.ws_key = None
        self.shape = None
        self._offsets = OrderedDict()
        off = 0
        for name, shp, _ in self.specs:
            n = int(np.prod(shp))
            self._offsets[name] = (off, n, shp)
            off += n
        # gradient buckets for data-parallel all-reduce, in the order backward finishes them
        first_dec = self._offsets["Decoder/embedding_table"][0]
        for i in range(self.lib.lxo_param_num()):          # the C plan and this inventory must agree slot by slot
            o, c = ctypes.c_longlong(), ctypes.c_longlong()
            self._ck(self.lib.lxo_param_info(ctypes.byref(probe), i, ctypes.byref(o), ctypes.byref(c)), "param_info")
            if c.value:
                name = self.lib.lxo_param_name_for(ctypes.byref(probe), i).decode()
                assert self._offsets[name][:2] == (o.value, c.value), (name, self._offsets[name], o.value, c.value)
        c3 = self._offsets["Encoder/convolutional_encoder/conv2d_2/kernel"][0]
        c4 = self._offsets["Encoder/convolutional_encoder/conv2d_3/kernel"][0]
        c5 = self._offsets["Encoder/convolutional_encoder/conv2d_4/kernel"][0]       # (the cnn variant's strided conv belongs to layer 5's pass)
        enc_names = [k for k in self._offsets if k.startswith("Encoder/convolutional_encoder/") and k.endswith("/kernel")]
        c6 = self._offsets[enc_names[-1]][0]                                          # the VALID conv in front of the decoder
        ywo = self._offsets["Decoder/AttentionCell/rnn/y_W_o"][0]        # the last variable: final before the recurrence runs
        # (range, encoder layers whose backward makes it final): a layer's kernel is final after its own pass, its bias no later
        self.buckets = [(ywo, self.n_params), (first_dec, ywo)]
        self.enc_buckets = [((6, 6), (c6, first_dec)), ((5, 5), (c5, c6)), ((4, 4), (c4, c5)), ((3, 3), (c3, c4)), ((2, 1), (0, c3))]
        # optional second stream for the half-batch interleave of the recurrent loop (LXO_DUAL_STREAM=1).
        # Measured slower than one stream in round 1 (18.8 vs 17.3 ms/step).  Round 2 measured why (tools/loop_probe.py,
        # DESIGN.md "launch cost"): the loop is bound by the device-side dependent-launch boundary, not by the host, and
        # two half-batch chains double the boundaries while each launch keeps its fixed cost; the interleave also forces
        # the round-1 split-K step kernels.  Off by default, kept as an A/B switch.
        self.side_stream = None
        if self.device.type == "cuda" and os.environ.get("LXO_DUAL_STREAM", "0") == "1":
            self.side_stream = torch.cuda.Stream(self.device)
        # second stream for the encoder's weight-gradient kernels (LXO_ENC_OVERLAP=0 switches it off): their prologues / epilogues and
        # the memory-bound pool-backward kernels overlap the data-gradient kernels.  Slower in rounds 1-3 (the cross-stream waits delayed
        # the launch-per-step decoder); with the decoder in two persistent launches it pays: 7.99 -> 7.87 ms per step (round 5).  The
        # library ignores it in the f32 parity mode and while bench.py records per-launch times (model_encoder.hip).
        self.enc_side = None
        if self.device.type == "cuda" and os.environ.get("LXO_ENC_OVERLAP", "1") != "0":
            self.enc_side = torch.cuda.Stream(self.device)
        self.load_params(PP.init_params(self.n_tok, seed, self.dims))

    # ------------------------------------------------------------ plumbing --
    def _shape(self, B, H, W, T):
        d = self.dims
        sh = _abi.LxoShape(B, H, W, T, self.n_tok, d["C"], d["E"], d["U"], d["O"], d["D"], self.dtype,
                           self.beam, self.max_steps)
        sh.encoder_cnn = 1 if d.get("cnn") else 0                 # configs/model.json encoder_cnn (encoder.py:46-56)
        sh.no_positional = 0 if d.get("positional", True) else 1  # positional_embeddings (encoder.py:60-65)
        sh.step_kernels = self.step_kernels
        sh.encoder_rnn = 1 if d.get("row_bilstm") else 0        # optional row-BiLSTM encoder (not in the reference; off by default)
        sh.deterministic = 1 if self.deterministic else 0
        return sh

    def _stream(self):
        if self.device.type == "cuda":
            return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return ctypes.c_void_p(0)

    def _ck(self, rc, what):
        _abi.check(self.lib, rc, what)

    def ensure(self, B, H, W, T):
        """Bind a call shape; grow the workspace when a larger batch arrives."""
        shape = self._shape(B, H, W, T)
        need = self.lib.lxo_workspace_bytes(ctypes.byref(shape)) + 256
        if self.ws is None or self.ws.numel() < need:
            self.ws = None
            self.ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        self.shape = shape
        return shape

    def sref(self):
        return ctypes.byref(self.shape)

    def region(self, name, kind="f32", shape=None):
        """View of a named workspace region as a torch tensor (float32, int32 or compute dtype)."""
        off, nb = ctypes.c_size_t(), ctypes.c_size_t()
        self._ck(self.lib.lxo_ws_region(self.sref(), name.encode(), ctypes.byref(off), ctypes.byref(nb)), "ws_region")
        raw = self.ws[off.value:off.value + nb.value]
        if kind == "ct":
            t = raw.view(torch.bfloat16) if self.dtype == _abi.LXO_BF16 else raw.view(torch.float32)
        elif kind == "i32":
            t = raw.view(torch.int32)
        else:
            t = raw.view(torch.float32)
        if shape is not None:
            t = t[:int(np.prod(shape))].view(*shape)
        return t

    # ------------------------------------------------------------- params --
    def load_params(self, P):
        flat = np.concatenate([np.asarray(P[k], dtype=np.float32).reshape(-1) for k, _, _ in self.specs])
        self.params.copy_(torch.from_numpy(flat))
        self.pack()

    def get_params(self):
        flat = self.params.detach().cpu().numpy()
        return OrderedDict((k, flat[o:o + n].reshape(s).copy()) for k, (o, n, s) in self._offsets.items())

    def grad_dict(self):
        flat = self.grads.detach().cpu().numpy()
        return OrderedDict((k, flat[o:o + n].reshape(s).copy()) for k, (o, n, s) in self._offsets.items())

    def pack(self):
        shape = self.shape if self.shape is not None else self._shape(1, 32, 32, 1)
        self._ck(self.lib.lxo_pack_weights(ctypes.byref(shape), _p(self.params), _p(self.wpack), self._stream()), "pack_weights")

    def state_dict(self):
        return {"params": self.get_params(), "adam_m": self.adam_m.cpu().numpy(), "adam_v": self.adam_v.cpu().numpy(),
                "adam_t": self.adam_t}

    def load_state_dict(self, sd):
        self.load_params(sd["params"])
        if "adam_m" in sd:
            self.adam_m.copy_(torch.from_numpy(np.asarray(sd["adam_m"], np.float32)))
            self.adam_v.copy_(torch.from_numpy(np.asarray(sd["adam_v"], np.float32)))
            self.adam_t = int(sd.get("adam_t", 0))

    # -------------------------------------------------------------- inputs --
    def _to_dev(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=self.device, dtype=dtype)

    def _lengths_dev(self, lengths):
        """Formula lengths on the device WITHOUT stalling the host: a pageable host array goes through a small ring of pinned staging
        buffers and an asynchronous copy.  (A plain `.to(device)` of pageable memory blocks the host until the compute stream has
        drained -- in the middle of a step that is the whole decoder forward: the kernels behind it were then enqueued ~30 us late.)"""
        if isinstance(lengths, torch.Tensor) or self.device.type != "cuda":
            return self._to_dev(lengths, torch.int32)
        a = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        n = int(a.shape[0])
        ring = getattr(self, "_len_ring", None)
        if not ring or ring[0]["host"].numel() < n:
            cap = max(64, n)
            ring = [{"host": torch.empty(cap, dtype=torch.int32).pin_memory(), "dev": torch.empty(cap, dtype=torch.int32, device=self.device), "ev": None}
                    for _ in range(4)]
            self._len_ring, self._len_i = ring, 0
        slot = ring[self._len_i % len(ring)]
        self._len_i += 1
        if slot["ev"] is not None:
            slot["ev"].synchronize()                             # the copy that last read this staging buffer (four steps ago) is long done
        slot["host"][:n].numpy()[:] = a
        slot["dev"][:n].copy_(slot["host"][:n], non_blocking=True)
        slot["ev"] = torch.cuda.Event()
        slot["ev"].record(torch.cuda.current_stream(self.device))
        return slot["dev"][:n]

    # ---------------------------------------------------------------- steps --
    def forward(self, img, formula, dropout=None, phase_hook=None, before_decoder=None, lengths=None):
        """Encoder + teacher-forced decoder; leaves logits in the workspace.  dropout = (keep_prob, seed)
        applies tf.nn.dropout on h and o (attention_cell.py:72,83) with this step's counter-based masks;
        backward() regenerates the same masks from the bound shape.
        lengths [B] (host array or device tensor; None: every position is computed): the formula lengths, bound here as loss() would bind them
        (self._lengths).  The persistent forward chain then streams nothing for the steps behind a row's end (lxo_decoder_train_fwd_live): the
        record of such a position is not the padded step's any more -- exact zeros in alpha and ctx -- and only positions t < lengths[b] may be read."""
        B, H, W = int(img.shape[0]), int(img.shape[1]), int(img.shape[2])
        T = int(formula.shape[1])
        # a batch the persistent chains do not take (the reference trains at 3, buckets and evaluates at 20: configs/training.json:6,
        # data_generator.py:41, evaluate_txt.py:42) is filled up to the next chain batch with DEAD rows: copies of its own samples whose
        # formula length is 0 (loss() appends the zeros), so no token of theirs is inside the loss mask (img2seq.py:68-71), their d(logits)
        # and with it every gradient contribution is an exact 0, and n_words does not see them
        self.live_B = B
        drop_on = dropout is not None and 0.0 < float(dropout[0]) < 1.0
        # (with config.dropout < 1 the batch stays as it is: the counter-based masks are keyed by (step, row, batch size), and the oracle the
        # dropout tests compare with draws them for the caller's batch -- the reference ships keep-probability 1, configs/training.json:7)
        Bp = B if drop_on else self._train_chain_batch(B, H, W)
        if Bp != B:
            # (lxo_shape.live_B: the encoder computes the B live images only -- `img` stays as it is -- and leaves zero features for the dead rows)
            # (host rows are repeated on the host, before the upload; device rows by ONE index_select with a cached index: at batch 3 the arange / remainder /
            # index_select triple was 3 launches with their gaps -- ~30 us of a 1.25 ms step)
            if isinstance(formula, torch.Tensor):
                cache = self.__dict__.setdefault("_pad_rows", {})
                idx = cache.get((Bp, B, formula.device))
                if idx is None:
                    idx = cache[(Bp, B, formula.device)] = (torch.arange(Bp, device=formula.device) % B)
                formula = formula.index_select(0, idx)
            else:
                formula = np.ascontiguousarray(np.asarray(formula)[np.arange(Bp) % B])
        self.ensure(Bp, H, W, T)
        self.shape.live_B = B if Bp != B else 0
        B = Bp
        if dropout is not None and 0.0 < float(dropout[0]) < 1.0:
            self.shape.keep_prob = float(dropout[0])
            self.shape.dropout_seed = int(dropout[1]) & 0x7FFFFFFF
        self._img = self._to_dev(img, torch.uint8)
        self._formula = self._to_dev(formula, torch.int32)
        if lengths is not None:
            self._bind_lengths(lengths)                            # (behind ensure(): the dead rows are counted on the chain batch)
        st = self._stream()
        self._bind_side()
        self._ck(self.lib.lxo_encoder_fwd(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), _p(self._img), st), "encoder_fwd")
        if phase_hook:
            phase_hook("encoder_fwd")
        if before_decoder is not None:
            # data parallel: the token-count all-reduce (its own stream) must be OFF the GPU before the persistent decoder chain starts --
            # the chain wants every CU, and a collective kernel that waits for a late rank would hold some of them
            torch.cuda.current_stream(self.device).wait_event(before_decoder)
        self._decoder_fwd(st, lengths is not None)
        if (not self._xdec_checked and self.dtype == _abi.LXO_BF16 and self.step_kernels == 0 and self.device.type == "cuda"
                and (B, H, W) not in self._nochain_shapes):
            if self._check_chain():
                self._decoder_fwd(st, lengths is not None)

    def _decoder_fwd(self, st, live):
        """The teacher-forced decoder on the bound shape and formula; live: with the bound lengths (self._lengths), for a caller that reads no
        position behind a row's end"""
        if live:
            self._ck(self.lib.lxo_decoder_train_fwd_live(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), _p(self._formula),
                                                         _p(self._lengths), st), "decoder_train_fwd_live")
        else:
            self._ck(self.lib.lxo_decoder_train_fwd(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), _p(self._formula), st),
                     "decoder_train_fwd")

    def chain_status(self, backward=False):
        """(used, error) of the persistent XCD-local decoder chain (csrc/xdec.hip) in the last lxo_decoder_train_fwd (backward=True: the
        backward chain of the last lxo_decoder_train_bwd): used = its 8 x 32 workgroups took their tickets; error != 0 = a chain did not
        assemble (a barrier timed out / an XCD got the wrong number of workgroups) and the step's decoder outputs are invalid.
        Synchronises the device."""
        o = XDEC_BLOCK_BYTES // 4 if backward else 0             # the backward chain's block
        return _chain_words(self.region("xdec_sync", "i32")[o:o + XDEC_STATUS_WORDS].cpu().numpy())

    def _check_chain(self, backward=False):
        """After the first forward (backward) that RAN the persistent chain (a shape that does not qualify leaves no tickets: noted, and
        not looked at again): the chain relies on how the hardware places a 256-workgroup grid (32 per XCD, one per CU).  If it reports an
        error, this engine switches to the launch-per-step kernels for good, and the caller redoes the pass (-> the error word).  The words
        are cleared by every call, chain or not, so the error is this call's.  Later steps are watched without a host synchronisation
        (_chain_health_post / _chain_health_poll)."""
        sfx = "_bwd" if backward else ""
        used, err = self.chain_status(backward)
        setattr(self, "chain_used" + sfx, used and not err)
        if used or err:
            setattr(self, "_xdec%s_checked" % sfx, True)
        else:
            getattr(self, "_nochain_shapes" + sfx).add((self.shape.B, self.shape.H, self.shape.W))
        if err:
            self._chain_fallback("backward" if backward else "forward", err)
        return err

    def _chain_fallback(self, which, err):
        import warnings
        self.chain_failures += 1
        self.step_kernels = 2
        if self.shape is not None:
            self.shape.step_kernels = 2
        self.chain_used = self.chain_used_bwd = False
        warnings.warn("latex_ocr_amd: the persistent %s decoder chain did not assemble (error word %d: a barrier / hand-over timed out or an "
                      "XCD got the wrong number of workgroups -- CUs held by another kernel or process, a CU mask); this engine now runs the "
                      "launch-per-step decoder kernels (lxo_shape.step_kernels = 2)" % (which, err), RuntimeWarning)

    def _chains_possible(self):
        return self.dtype == _abi.LXO_BF16 and self.step_kernels == 0 and self.device.type == "cuda"

    def _chain_health_post(self, have_scale, dp=False):
        """Behind backward(), before the optimizer: lxo_chain_guard (device: scale[0] = NaN when a chain of this step failed, so the optimizer
        drops the step) + an asynchronous copy of the two error words into a pinned ring slot.  No host synchronisation.
        The NaN probe element of the gradients (a PEER's chain failed) is only looked at in a data-parallel step: a single process whose
        gradients are NaN for numeric reasons is not protected from itself -- the reference would write the NaNs into its weights too
        (img2seq.py:119-123), and a silently dropped update would hide the divergence."""
        st = self._stream()
        if self._health_ring is None:
            self._health_dev = torch.zeros(4, dtype=torch.int32, device=self.device)
            self._health_ring = [{"host": torch.zeros(4, dtype=torch.int32).pin_memory(), "ev": None} for _ in range(4)]
        self._ck(self.lib.lxo_chain_guard(self.sref(), _p(self.ws), _p(self.grads if dp else None), _p(self.scale), 1 if have_scale else 0, _p(self._health_dev), st),
                 "chain_guard")
        slot = self._health_ring[self._health_i % len(self._health_ring)]
        self._health_i += 1
        if slot["ev"] is not None:
            slot["ev"].synchronize()                 # four steps old: long done (and its words were looked at by _chain_health_poll)
            self._chain_health_look(slot)
        slot["host"].copy_(self._health_dev, non_blocking=True)
        slot["seq"] = self._health_i
        slot["ev"] = torch.cuda.Event()
        slot["ev"].record(torch.cuda.current_stream(self.device))

    def _chain_health_look(self, slot):
        ef, eb, dropped = int(slot["host"][0]), int(slot["host"][1]), int(slot["host"][2])
        slot["ev"] = None
        if dropped:
            self.dropped_steps = getattr(self, "dropped_steps", 0) + 1
            self._last_dropped_seq = slot["seq"]
            if getattr(self, "method", 0) == 0 and self.adam_t > 0:
                self.adam_t -= 1                      # the step was dropped on the device (NaN scale) on EVERY rank: its Adam time step did not happen
        if (ef or eb) and self.step_kernels == 0:
            self._chain_fallback("forward" if ef else "backward", ef or eb)
        return bool(dropped)

    def _chain_health_poll(self, wait=False):
        """Look at the error words of finished steps (wait=True: of every posted step; the caller has synchronised or accepts to).
        -> True when a failure was found (the engine has switched to the launch-per-step kernels; the failed step was dropped)."""
        bad = False
        for slot in self._health_ring or ():
            if slot["ev"] is not None and (wait or slot["ev"].query()):
                if wait:
                    slot["ev"].synchronize()
                bad = self._chain_health_look(slot) or bad
        return bad

    def _bind_side(self):
        side = ctypes.c_void_p(self.side_stream.cuda_stream) if self.side_stream is not None else ctypes.c_void_p(0)
        self._ck(self.lib.lxo_set_side_stream(side), "set_side_stream")
        es = getattr(self, "enc_side", None)
        self._ck(self.lib.lxo_set_encoder_side_stream(ctypes.c_void_p(es.cuda_stream) if es is not None else ctypes.c_void_p(0)),
                 "set_encoder_side_stream")

    def _bind_lengths(self, lengths):
        dead = int(self.shape.B) - int(getattr(self, "live_B", self.shape.B))
        if dead > 0:                                               # the dead rows forward() appended: length 0 = outside the loss mask
            if isinstance(lengths, torch.Tensor):
                zc = self.__dict__.setdefault("_pad_zeros", {})
                z = zc.get((dead, lengths.device))
                if z is None:
                    z = zc[(dead, lengths.device)] = torch.zeros(dead, dtype=torch.int32, device=lengths.device)
                lengths = torch.cat([lengths.to(torch.int32), z])
            else:
                lengths = np.concatenate([np.asarray(lengths, dtype=np.int32).reshape(-1), np.zeros(dead, np.int32)])
        self._lengths = self._lengths_dev(lengths)

    @staticmethod
    def _check_weights(who, weights, row_weights, B, T):
        """The loss weights before any launch: a host array is checked for shape and finiteness (-> f32), a device tensor for its shape only (a
        look at its values would cost a synchronisation).  B, T: the caller's batch, without the chain batch's dead rows."""
        out = []
        for name, w, shp in (("weights", weights, (B, T)), ("row_weights", row_weights, (B,))):
            if w is None or isinstance(w, torch.Tensor):
                if w is not None and tuple(w.shape) != shp:
                    raise ValueError("%s: %s must be %s, got %s" % (who, name, list(shp), list(w.shape)))
                out.append(w)
                continue
            a = np.asarray(w)
            if a.shape != shp or a.dtype.kind not in "fiu":
                raise ValueError("%s: %s must be a real array of shape %s, got %s %s" % (who, name, list(shp), a.dtype, list(a.shape)))
            a = np.ascontiguousarray(a, dtype=np.float32)
            if not np.isfinite(a).all():
                raise ValueError("%s: %s holds a NaN or an infinity (or a value beyond f32)" % (who, name))
            out.append(a)
        return out

    @staticmethod
    def _check_smoothing(who, label_smoothing):
        """The label smoothing before any launch: a real number in [0, 1) -> float"""
        try:
            eps = float(label_smoothing)
        except (TypeError, ValueError):
            raise ValueError("%s: label_smoothing must be a number in [0, 1), got %r" % (who, label_smoothing))
        if not (math.isfinite(eps) and 0.0 <= eps < 1.0 and float(np.float32(eps)) < 1.0):
            raise ValueError("%s: label_smoothing must be a finite number in [0, 1), got %r" % (who, label_smoothing))
        return eps

    def _weights_dev(self, w, dead):
        """f32 on the device, zero rows appended for the dead rows forward() added (weight 0 on a length of 0); a host array goes through pinned
        memory and an asynchronous copy, as the lengths do"""
        if isinstance(w, torch.Tensor):
            w = w.to(device=self.device, dtype=torch.float32).contiguous()
            if dead > 0:
                w = torch.cat([w, torch.zeros((dead,) + tuple(w.shape[1:]), dtype=torch.float32, device=self.device)])
            return w
        if dead > 0:
            w = np.concatenate([w, np.zeros((dead,) + w.shape[1:], np.float32)])
        t = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
        if self.device.type != "cuda":
            return t
        return t.pin_memory().to(self.device, non_blocking=True)

    def _soft_dev(self, who, soft_targets, soft_weight, B, T, lengths=None):
        """The soft targets before any launch -> _SoftDev (device ids int32 / masses f32 [B, T, k], lambda).  soft_targets: an Alternatives (its ids
        and logp: the masses are exp(logp), taken on the device, -inf is mass 0) or a pair (ids [B, T, k], p [B, T, k]), host arrays or device
        tensors.  A ValueError for a wrong shape, k outside 1 .. 16, soft_weight outside [0, 1] and -- host arrays only, a look at a device tensor
        would cost a synchronisation -- for a counted mass that is negative, NaN or infinite and for a position whose counted masses exceed
        1 + 1e-3.  A slot counts where 0 <= id < V; with host lengths only the positions t < lengths[b] are looked at, as on the device."""
        if isinstance(soft_targets, _SoftDev):
            return soft_targets
        try:
            lam = float(soft_weight)
        except (TypeError, ValueError):
            raise ValueError("%s: soft_weight must be a number in [0, 1], got %r" % (who, soft_weight))
        if not (math.isfinite(lam) and 0.0 <= lam <= 1.0):
            raise ValueError("%s: soft_weight must be a finite number in [0, 1], got %r" % (who, soft_weight))
        is_logp = isinstance(soft_targets, Alternatives)
        if is_logp:
            ids, val = soft_targets.ids, soft_targets.logp
        else:
            try:
                ids, val = soft_targets
            except (TypeError, ValueError):
                raise ValueError("%s: soft_targets must be an Alternatives or a pair (ids [B, T, k], p [B, T, k])" % who)
        shp = tuple(ids.shape)
        if len(shp) != 3 or shp[:2] != (B, T) or tuple(val.shape) != shp:
            raise ValueError("%s: soft_targets must be ids and %s of shape [B = %d, T = %d, k], got %s and %s"
                             % (who, "logp" if is_logp else "p", B, T, list(shp), list(val.shape)))
        k = int(shp[2])
        if not 1 <= k <= 16:
            raise ValueError("%s: soft_targets carry k = %d slots per position, outside 1 .. 16" % (who, k))
        if not isinstance(ids, torch.Tensor):
            ids = np.asarray(ids)
            if ids.dtype.kind not in "iu":
                raise ValueError("%s: the soft targets' ids must be integers, got %s" % (who, ids.dtype))
            ids = np.ascontiguousarray(np.clip(ids, -1, np.iinfo(np.int32).max), dtype=np.int32)
        if not isinstance(val, torch.Tensor):
            val = np.asarray(val)
            if val.dtype.kind not in "fiu":
                raise ValueError("%s: the soft targets' %s must be real numbers, got %s" % (who, "logp" if is_logp else "p", val.dtype))
            val = np.ascontiguousarray(val, dtype=np.float32)
            if not isinstance(ids, torch.Tensor):
                cnt = (ids >= 0) & (ids < self.n_tok)
                if lengths is not None and not isinstance(lengths, torch.Tensor):
                    cnt &= (np.arange(T)[None, :] < np.asarray(lengths).reshape(-1)[:B, None])[:, :, None]
                with np.errstate(over="ignore", invalid="ignore"):
                    m = np.where(cnt, np.exp(val.astype(np.float64)) if is_logp else val.astype(np.float64), 0.0)
                if not np.isfinite(m).all() or (m < 0.0).any():
                    raise ValueError("%s: soft_targets hold a mass that is negative, NaN or infinite" % who)
                tot = m.sum(axis=2)
                if tot.size and tot.max() > 1.0 + 1e-3:
                    b, t = np.unravel_index(int(tot.argmax()), tot.shape)
                    raise ValueError("%s: the counted masses of position (%d, %d) add up to %.6f, above 1 + 1e-3" % (who, b, t, float(tot[b, t])))
        ids = self._to_dev(ids, torch.int32).contiguous()
        val = self._to_dev(val, torch.float32).contiguous()
        return _SoftDev(ids, torch.exp(val) if is_logp else val, k, lam)

    def _soft_padded(self, soft, dead):
        """slot rows of id -1 (mass 0) appended for the dead rows forward() added, as _weights_dev appends weights of 0"""
        if dead <= 0:
            return soft
        tail = (dead,) + tuple(soft.ids.shape[1:])
        return soft._replace(ids=torch.cat([soft.ids, torch.full(tail, -1, dtype=torch.int32, device=soft.ids.device)]),
                             p=torch.cat([soft.p, torch.zeros(tail, dtype=torch.float32, device=soft.p.device)]))

    def loss(self, lengths, inv_ntok=None, ntok_dev=None, ntok_event=None, weights=None, row_weights=None, _padded=False, label_smoothing=0.0,
             _bound=False, soft_targets=None, soft_weight=0.5):
        """Loss statistics + d(logits).  Either inv_ntok (host float) or ntok_dev (device float32 [1] = the global token count,
        e.g. from DataParallel.sum_count_async; the compute stream waits for ntok_event, the host does not).
        weights [B, T] / row_weights [B] (host arrays or device tensors, either or both): the weighted loss lxo_ce_loss_weighted -- token (b, t)
        weighs weights[b, t] * row_weights[b], of any sign; inv_ntok / ntok_dev are then its normaliser, whatever the caller chose, and the
        statistics are the four {sum w CE, token count, sum w, sum CE}.  Without weights: {sum CE, token count}, as ever.
        label_smoothing = eps in (0, 1): the smoothed loss lxo_ce_loss_smoothed -- a live row's target is (1 - eps) one-hot + eps / V over the
        vocabulary, its loss L = (1 - eps) CE + eps (lse - mean logit) -- with or without weights; the statistics are then the four
        {sum w L, token count, sum w, sum CE (plain)}.  0.0: the calls above, as without the argument.  Outside [0, 1): a ValueError before any launch.
        soft_targets (an Alternatives, or a pair (ids, p) of [B, T, k] host arrays or device tensors; _soft_dev) with soft_weight = lambda in [0, 1]:
        the soft-target loss lxo_ce_loss_soft -- a live row's target is (1 - lambda) * (the smoothed target) + lambda * (the teacher's k masses on
        their tokens, what they leave of 1 spread over the vocabulary); a position without a counting slot keeps the smoothed target.  It combines
        with the weights, the normaliser and label_smoothing; the statistics are the four.  None: the calls above."""
        eps = self._check_smoothing("loss", label_smoothing)
        soft = None
        if soft_targets is not None:
            live = int(getattr(self, "live_B", self.shape.B))
            soft = self._soft_padded(self._soft_dev("loss", soft_targets, soft_weight, live, int(self.shape.T), lengths), int(self.shape.B) - live)
            self._loss_soft = soft                                 # alive until the next call
        if _bound:
            lengths = None                                         # (train_step: forward() has bound these lengths already -- no second upload)
        if weights is None and row_weights is None:
            if lengths is not None:
                self._bind_lengths(lengths)
            wt = wr = None
        else:
            live = int(getattr(self, "live_B", self.shape.B))
            dead = int(self.shape.B) - live
            if not _padded:                                        # (mrt_grads hands over what it built for the chain batch)
                weights, row_weights = self._check_weights("loss", weights, row_weights, live, int(self.shape.T))
                weights = self._weights_dev(weights, dead) if weights is not None else None
                row_weights = self._weights_dev(row_weights, dead) if row_weights is not None else None
            if lengths is not None:
                self._bind_lengths(lengths)
            wt, wr = self._loss_weights = (weights, row_weights)      # alive until the next call
        if ntok_dev is not None:
            if ntok_event is not None:
                torch.cuda.current_stream(self.device).wait_event(ntok_event)
            self._ntok_dev = ntok_dev          # keep alive until the kernel has been enqueued
            if ntok_dev.is_cuda:               # allocated on the count stream, read on this one: the allocator must not hand the
                ntok_dev.record_stream(torch.cuda.current_stream(self.device))   # block to a later upload before this kernel ran
        if soft is not None:
            self._ck(self.lib.lxo_ce_loss_soft(self.sref(), _p(self.ws), _p(self._formula), _p(self._lengths), ctypes.c_float(eps), ctypes.c_float(soft.lam),
                                               soft.k, _p(soft.ids), _p(soft.p), _p(wt), _p(wr),
                                               ctypes.c_float(0.0 if ntok_dev is not None else inv_ntok), _p(ntok_dev), self._stream()), "ce_loss_soft")
            return self.region("loss")[:4]
        if eps > 0.0:
            self._ck(self.lib.lxo_ce_loss_smoothed(self.sref(), _p(self.ws), _p(self._formula), _p(self._lengths), ctypes.c_float(eps), _p(wt), _p(wr),
                                                   ctypes.c_float(0.0 if ntok_dev is not None else inv_ntok), _p(ntok_dev), self._stream()),
                     "ce_loss_smoothed")
            return self.region("loss")[:4]
        if wt is not None or wr is not None:
            self._ck(self.lib.lxo_ce_loss_weighted(self.sref(), _p(self.ws), _p(self._formula), _p(self._lengths), _p(wt), _p(wr),
                                                   ctypes.c_float(0.0 if ntok_dev is not None else inv_ntok), _p(ntok_dev), self._stream()),
                     "ce_loss_weighted")
            return self.region("loss")[:4]
        if ntok_dev is not None:
            self._ck(self.lib.lxo_ce_loss_fwd_bwd_dev(self.sref(), _p(self.ws), _p(self._formula), _p(self._lengths), _p(ntok_dev),
                                                      self._stream()), "ce_loss_dev")
        else:
            self._ck(self.lib.lxo_ce_loss_fwd_bwd(self.sref(), _p(self.ws), _p(self._formula), _p(self._lengths),
                                                  ctypes.c_float(inv_ntok), self._stream()), "ce_loss")
        return self.region("loss")[:2]

    def backward(self, comm=None, phase_hook=None):
        """BPTT + encoder backward into self.grads (zeroed first).  `comm(lo, hi)` is called as soon
        as the gradient range [lo, hi) is final (data-parallel bucket all-reduce hook); phase_hook(name) after each
        part (bench.py's per-phase table)."""
        st = self._stream()
        self._bind_side()
        # the recurrence may run as the persistent backward chain (csrc/xdec.hip): it wants every CU, so no collective kernel is put
        # beside it -- y_W_o's all-reduce then follows the recurrence instead of overlapping it
        chain = (self.dtype == _abi.LXO_BF16 and self.shape.step_kernels == 0 and self.device.type == "cuda")

        def decoder_bwd(defer_b0):
            self.grads.zero_()
            if comm:
                # y_W_o's gradient needs only d(logits): reduce it while the recurrence runs
                self._ck(self.lib.lxo_decoder_train_bwd_part(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), _p(self._formula),
                                                             _p(self.grads), 1, st), "decoder_train_bwd_part")
                if not defer_b0:
                    comm(*self.buckets[0])
                self._ck(self.lib.lxo_decoder_train_bwd_part(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), _p(self._formula),
                                                             _p(self.grads), 2, st), "decoder_train_bwd_part")
            else:
                self._ck(self.lib.lxo_decoder_train_bwd(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), _p(self._formula),
                                                        _p(self.grads), st), "decoder_train_bwd")

        # After the first backward of this shape has been looked at (below), the whole pass is ONE call: lxo_train_bwd joins the weight-gradient
        # side stream once, at the end (the decoder's deferred weight gradients then also run beside conv6's data gradient), and records
        # an event per gradient bucket for the data-parallel exchange.  bench.py's instrumented step (phase_hook) keeps the two calls.
        key = (self.shape.B, self.shape.H, self.shape.W)
        looked = self._xdec_bwd_checked or key in self._nochain_shapes_bwd or not chain
        ready_ok = comm is None or (getattr(comm, "takes_ready", False) and chain)      # (no chain: y_W_o's bucket goes out while the recurrence runs)
        if (self.device.type == "cuda" and looked and ready_ok and phase_hook is None
                and os.environ.get("LXO_TRAIN_BWD_FUSED", "1") != "0"):
            self.grads.zero_()
            table = None
            if comm:
                evs = self._enc_ready_events()
                table = (ctypes.c_void_p * 7)(*[ctypes.c_void_p(e.cuda_event) if e is not None else None for e in evs])
            self._ck(self.lib.lxo_train_bwd(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), _p(self._formula), _p(self._img),
                                            _p(self.grads), table, st), "train_bwd")
            if comm:
                comm(*self.buckets[0], ready=evs[0])
                comm(*self.buckets[1], ready=evs[0])
                for (hi, lo), rng in self.enc_buckets:
                    comm(*rng, ready=evs[lo])
            return
        decoder_bwd(chain)
        if chain and not self._xdec_bwd_checked and (self.shape.B, self.shape.H, self.shape.W) not in self._nochain_shapes_bwd:
            if self._check_chain(backward=True):      # as for the forward chain, after the first backward that RAN it
                chain = False
                decoder_bwd(False)
        if comm:
            if chain:
                comm(*self.buckets[0])
            comm(*self.buckets[1])
        if phase_hook:
            phase_hook("decoder_bwd")
        if comm and getattr(comm, "takes_ready", False) and self.device.type == "cuda":
            # ONE call for the six layers; the library records an event per layer when its gradients are final (on the weight-gradient
            # side stream when one is bound) and the communication side waits for THAT: the compute stream does not stop at the buckets
            evs = self._enc_ready_events()
            table = (ctypes.c_void_p * 7)(*[ctypes.c_void_p(e.cuda_event) if e is not None else None for e in evs])
            self._ck(self.lib.lxo_encoder_bwd_ready(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), _p(self._img), _p(self.grads),
                                                    6, 1, table, st), "encoder_bwd_ready")
            for (hi, lo), rng in self.enc_buckets:
                comm(*rng, ready=evs[lo])
        elif comm:
            # one all-reduce per encoder layer as its gradients become final: only conv2 + conv1 (0.3 MB) are left for the end
            for (hi, lo), rng in self.enc_buckets:
                self._ck(self.lib.lxo_encoder_bwd(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), _p(self._img), _p(self.grads),
                                                  hi, lo, st), "encoder_bwd")
                comm(*rng)
        else:
            self._ck(self.lib.lxo_encoder_bwd(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), _p(self._img), _p(self.grads),
                                              6, 1, st), "encoder_bwd")

    def _enc_ready_events(self):
        """events[l] for the layers that close a gradient bucket (enc_buckets: 6, 5, 4, 3 and 1) and [0] for the decoder's parameters; recorded
        once here so that their handles exist, re-recorded by lxo_encoder_bwd_ready / lxo_train_bwd every step"""
        if getattr(self, "_enc_ready", None) is None:
            cur = torch.cuda.current_stream(self.device)
            evs = [None] * 7
            for lo in [0] + [lo for (hi, lo), _ in self.enc_buckets]:      # 0: the decoder's parameters (lxo_train_bwd)
                evs[lo] = torch.cuda.Event()
                evs[lo].record(cur)
            self._enc_ready = evs
        return self._enc_ready

    METHODS = {"adam": 0, "sgd": 1, "adagrad": 2, "rmsprop": 3}

    def set_optimizer(self, lr_method):
        """img2seq.py:95-109: 'adam' | 'adagrad' | 'sgd' | 'rmsprop' (TF-1.12 default hyper-parameters)."""
        m = lr_method.lower()
        if m not in self.METHODS:
            raise NotImplementedError("Unknown method {}".format(lr_method))
        self.method = self.METHODS[m]
        if self.method == 2:
            self.adam_v.fill_(0.1)        # Adagrad initial_accumulator_value
        elif self.method == 3:
            self.adam_v.fill_(1.0)        # RMSProp rms slot starts at ones

    def optimizer_step(self, lr, clip=-1.0, beta1=0.9, beta2=0.999, eps=1e-8, guard=False, dp=False):
        """guard: fold the decoder chains' error words into the scale first (train_step does; a failed step is then dropped on the device).
        dp: a data-parallel step -- the guard then runs on EVERY bf16 rank whatever this rank's own step_kernels: a rank that already fell
        back to the launch-per-step kernels must still drop the step a PEER's chain failed in (the peer's NaN probe element arrives through
        the all-reduce), or the replicas part (its own error words are cleared by the no-chain paths, so the check is harmless there)."""
        st = self._stream()
        possible = self._chains_possible() or (dp and self.dtype == _abi.LXO_BF16 and self.device.type == "cuda")
        guard = guard and possible and self.ws is not None and self.shape is not None
        if getattr(self, "method", 0) != 0:
            scale = None
            if clip is not None and clip > 0:
                self._ck(self.lib.lxo_global_norm_scale(self.n_params, _p(self.grads), ctypes.c_float(clip), _p(self.scale), st), "clip")
                scale = self.scale
            if guard:
                self._chain_health_post(scale is not None, dp)
                scale = self.scale
            self._ck(self.lib.lxo_optimizer_step(self.method, self.n_params, _p(self.params), _p(self.grads), _p(self.adam_v),
                                                 ctypes.c_float(float(lr)), _p(scale), st), "optimizer_step")
            self.pack()
            return
        self.adam_t += 1
        lr_t = float(lr) * math.sqrt(1.0 - beta2 ** self.adam_t) / (1.0 - beta1 ** self.adam_t)
        scale = None
        if clip is not None and clip > 0:
            self._ck(self.lib.lxo_global_norm_scale(self.n_params, _p(self.grads), ctypes.c_float(clip), _p(self.scale), st), "clip")
            scale = self.scale
        if guard:
            self._chain_health_post(scale is not None, dp)
            scale = self.scale
        self._ck(self.lib.lxo_adam_step(self.n_params, _p(self.params), _p(self.grads), _p(self.adam_m), _p(self.adam_v),
                                        ctypes.c_float(lr_t), ctypes.c_float(beta1), ctypes.c_float(beta2), ctypes.c_float(eps),
                                        _p(scale), st), "adam")
        self.pack()

    def train_step(self, img, formula, lengths, lr, clip=-1.0, dist=None, sync_loss=True, dropout=1.0, dropout_seed=None,
                   weights=None, row_weights=None, norm=None, label_smoothing=0.0, soft_targets=None, soft_weight=0.5):
        """One optimisation step of img2seq.py:_run_train's body.  Returns the batch loss
        (token mean over the global batch) or None when sync_loss is False.  dropout = config.dropout
        (keep probability, img2seq.py:166); masks are keyed by (dropout_seed or a per-engine step counter).
        weights [B, T] / row_weights [B] (host arrays or device tensors): the step minimises sum_{b,t} weights[b, t] row_weights[b] CE[b, t] / norm
        (loss()); norm = None: the global token count, as without weights (data parallel: the device-side count); norm = a float: the caller's
        own normaliser, the GLOBAL one under dist.  Returns that weighted loss.
        label_smoothing in (0, 1): the step minimises the smoothed loss (loss()), weighted or not, and returns it; 0.0: the step without the argument.
        soft_targets / soft_weight (loss(): a teacher's top-k per position and lambda): the step minimises the soft-target loss, with or without
        weights and smoothing, and returns it; the checks of _soft_dev run before any launch.  None: the step without the argument.
        Either way a synchronised step leaves the PLAIN token-mean CE of the batch in self.last_ce (under dist: of the global batch), what a
        perplexity is made of."""
        eps = self._check_smoothing("train_step", label_smoothing)
        weighted = weights is not None or row_weights is not None
        if weighted:
            weights, row_weights = self._check_weights("train_step", weights, row_weights, int(img.shape[0]), int(formula.shape[1]))
        if norm is not None and not (math.isfinite(float(norm)) and float(norm) != 0.0):
            raise ValueError("train_step: norm must be a finite non-zero number, got %r" % (norm,))
        wkw = dict(weights=weights, row_weights=row_weights) if weighted else {}
        if eps > 0.0:
            wkw["label_smoothing"] = eps
        if soft_targets is not None:
            wkw["soft_targets"] = self._soft_dev("train_step", soft_targets, soft_weight, int(img.shape[0]), int(formula.shape[1]), lengths)
        drop = None
        if dropout is not None and 0.0 < float(dropout) < 1.0:
            self.drop_step = getattr(self, "drop_step", 0) + 1
            world, rank = (dist.world, dist.rank) if dist is not None else (1, 0)
            drop = (float(dropout), dropout_seed if dropout_seed is not None else self.drop_step * world + rank)
        n_local = int(np.asarray(lengths).sum()) if not isinstance(lengths, torch.Tensor) else int(lengths.sum().item())
        if self._health_ring is not None and dist is None:
            # error words of the steps the device has finished meanwhile (no stall).  Not under data parallelism: WHEN the host notices a
            # finished step differs from rank to rank, and the Adam time step a dropped update gives back enters lr_t -- there every rank
            # looks at a step's words at the same distance (the ring slot's reuse, four steps later, or a synchronising caller's wait)
            self._chain_health_poll()
        if dist is not None and norm is None:
            # the global token count travels rank -> device -> all-reduce -> loss kernel; no host sync inside the step
            ntok, ev = dist.sum_count_async(n_local)
            self.forward(img, formula, dropout=drop, before_decoder=ev, lengths=lengths)
            stats = self.loss(lengths, ntok_dev=ntok, ntok_event=ev, _bound=True, **wkw)
        else:
            self.forward(img, formula, dropout=drop, lengths=lengths)
            stats = self.loss(lengths, 1.0 / (float(n_local) if norm is None else float(norm)), _bound=True, **wkw)
        self.backward(comm=dist.reduce_range_fn(self.grads) if dist is not None else None)
        if dist is not None:
            dist.finish()
        self.optimizer_step(lr, clip, guard=True, dp=dist is not None)
        if not sync_loss:
            return None
        if dist is not None:
            s = stats.clone()
            dist.all_reduce(s)
            s = s.cpu().numpy()
        else:
            s = stats.cpu().numpy()
        if (self._health_ring is not None and self._chain_health_poll(wait=True) and getattr(self, "_last_dropped_seq", -1) == self._health_i
                and dist is None and not getattr(self, "_redoing", False)):
            # the host is synchronised here anyway: a chain failed in THIS step, the device dropped its update, the engine has switched to the
            # launch-per-step kernels -- run the step again so that the caller gets the loss and the update it asked for
            self._redoing = True
            try:
                return self.train_step(img, formula, lengths, lr, clip=clip, dist=None, sync_loss=True, dropout=dropout,
                                       dropout_seed=drop[1] if drop is not None else None, norm=norm, **wkw)
            finally:
                self._redoing = False
        self.last_ce = float(s[3 if len(s) == 4 else 0]) / max(float(s[1]), 1.0)
        return float(s[0]) / (float(s[1]) if norm is None else float(norm))

    def mrt_grads(self, img, cand, cand_lengths, group_sizes, cost, alpha, dropout=None):
        """Forward and backward of one minimum-risk step, into self.grads: the gradient of (1 / G) sum_g sum_c Q_c cost_c, Q = softmax over image g's
        candidates of alpha * log p(candidate | image) -- the mean expected cost under the model's own, sharpened, distribution over the candidates.
        img [G, H, W]; cand [rows, T] int32 (pad_batch_formulas' padding) and cand_lengths / cost [rows]: image g's candidates are the
        group_sizes[g] consecutive rows behind those of image g - 1.  Image g is repeated for each of its candidates (the encoder runs per
        row), then: forward, lxo_score_tokens (sequence log-probs, device), lxo_mrt_weights (w_c = alpha Q_c (R_g - cost_c) = d R_g / d CE_c,
        device), the weighted loss with row_weights = w and normaliser G, backward.  No host synchronisation in between.
        -> device tensors (risk [1] = sum_g R_g, q [rows], w [rows])."""
        cand_h = cand.detach().cpu().numpy() if isinstance(cand, torch.Tensor) else np.asarray(cand)
        ln = np.ascontiguousarray(np.asarray(cand_lengths), dtype=np.int64).reshape(-1)
        gs = np.ascontiguousarray(np.asarray(group_sizes), dtype=np.int64).reshape(-1)
        c = np.asarray(cost, dtype=np.float64).reshape(-1)
        G, rows = int(img.shape[0]), int(cand_h.shape[0])
        if cand_h.ndim != 2 or ln.shape[0] != rows or c.shape[0] != rows or gs.shape[0] != G:
            raise ValueError("mrt_step: cand must be [rows, T], cand_lengths and cost [rows] and group_sizes [G = %d images], got %s, %s, %s and %s"
                             % (G, list(cand_h.shape), list(ln.shape), list(c.shape), list(gs.shape)))
        if G < 1 or (gs < 1).any():
            raise ValueError("mrt_step: every image needs at least one candidate, got group sizes %s" % gs.tolist())
        if int(gs.sum()) != rows:
            raise ValueError("mrt_step: the group sizes add up to %d, cand has %d rows" % (int(gs.sum()), rows))
        if ln.size and (ln.min() < 0 or ln.max() > cand_h.shape[1]):
            raise ValueError("mrt_step: cand_lengths must lie in [0, T = %d], got %d .. %d" % (cand_h.shape[1], int(ln.min()), int(ln.max())))
        with np.errstate(over="ignore"):
            c32 = c.astype(np.float32)
        if not np.isfinite(c32).all():
            raise ValueError("mrt_step: cost holds a NaN or an infinity (or a value beyond f32)")
        if not (math.isfinite(float(alpha)) and float(alpha) > 0.0 and math.isfinite(float(np.float32(alpha)))):
            raise ValueError("mrt_step: alpha must be positive and finite, got %r" % (alpha,))
        rep = np.repeat(np.arange(G), gs)
        if isinstance(img, torch.Tensor):
            img = img.index_select(0, torch.from_numpy(rep).to(img.device))
        else:
            img = np.ascontiguousarray(np.asarray(img)[rep])
        # ONE upload, in front of the forward (a pageable copy behind it would wait for it): cost (f32) | the group offsets (int32).  The chain batch's
        # dead rows lie behind the last group: lxo_mrt_weights reads no cost of theirs.  One device buffer: seq | w | risk | q | logp
        host = np.zeros(rows + G + 1, np.int32)
        host[:rows].view(np.float32)[:] = c32
        host[rows + 1:] = np.cumsum(gs)
        up = self._to_dev(host, torch.int32)
        return self._mrt_grads_dev(img, np.ascontiguousarray(cand_h, dtype=np.int32), ln.astype(np.int32), up[:rows].view(torch.float32), up[rows:], G, rows,
                                   alpha, dropout, keep=up)

    def _mrt_grads_dev(self, img, cand, cand_lengths, cost, group_off, G, rows, alpha, dropout, keep=None):
        """mrt_grads behind its checks: img [rows, H, W] (one image per candidate row), cand [rows, T] and cand_lengths [rows] as host arrays or device
        tensors, cost f32 [rows] and group_off int32 [G + 1] on the device.  Rows at and behind group_off[G] (and the chain batch's own dead rows) carry
        length 0 and get w = q = 0."""
        self.forward(img, cand, dropout=dropout)
        Bp = int(self.shape.B)
        self._bind_lengths(cand_lengths)
        buf = torch.empty(3 * Bp + 1 + Bp * int(self.shape.T), dtype=torch.float32, device=self.device)
        seq, w, out, logp = buf[:Bp], buf[Bp:2 * Bp], buf[2 * Bp:3 * Bp + 1], buf[3 * Bp + 1:]
        st = self._stream()
        self._ck(self.lib.lxo_score_tokens(self.sref(), _p(self.ws), _p(self._formula), _p(self._lengths), _p(logp), None, _p(seq), st), "score_tokens")
        self._ck(self.lib.lxo_mrt_weights(_p(seq), _p(cost), _p(group_off), G, Bp, ctypes.c_float(float(alpha)), _p(w), _p(out[1:]), _p(out[:1]), st),
                 "mrt_weights")
        self.loss(None, 1.0 / float(G), row_weights=w, _padded=True)
        self.backward()
        self._mrt_keep = (keep, cost, group_off, buf)
        return out[:1], out[1:1 + rows], w[:rows]

    def mrt_step(self, img, cand, cand_lengths, group_sizes, cost, lr, alpha, clip=-1.0, dropout=1.0):
        """One minimum-risk training step (mrt_grads + the optimizer; single process): -> (risk / G = the mean expected cost BEFORE the update,
        q f32 [rows] = each candidate's probability among its image's candidates).  The host synchronises once, for that copy at the end; the
        chain guard and the redo of a step a chain failed in are train_step's."""
        drop = None
        if dropout is not None and 0.0 < float(dropout) < 1.0:
            self.drop_step = getattr(self, "drop_step", 0) + 1
            drop = (float(dropout), self.drop_step)
        if self._health_ring is not None:
            self._chain_health_poll()
        risk, q, _ = self.mrt_grads(img, cand, cand_lengths, group_sizes, cost, alpha, dropout=drop)
        self.optimizer_step(lr, clip, guard=True)
        h = torch.cat([risk, q]).cpu().numpy()
        if (self._health_ring is not None and self._chain_health_poll(wait=True) and getattr(self, "_last_dropped_seq", -1) == self._health_i
                and not getattr(self, "_redoing", False)):
            self._redoing = True                                   # as train_step: the step a chain failed in was dropped on the device; again, on the launch-per-step kernels
            if drop is not None:
                self.drop_step -= 1                                # ... under the same dropout masks
            try:
                return self.mrt_step(img, cand, cand_lengths, group_sizes, cost, lr, alpha, clip=clip, dropout=dropout)
            finally:
                self._redoing = False
        return float(h[0]) / int(img.shape[0]), h[1:].copy()

    def mrt_sample_step(self, img, ref, ref_lengths, id_end, id_pad, lr, alpha, n=5, temperature=1.0, top_k=0, top_p=1.0, seed=0, include_reference=True,
                        max_iter=151, clip=-1.0, dropout=1.0, cost="edit"):
        """One minimum-risk training step from pixels, the candidates never leaving the device: the sampled decode (sample_decode's draws at the same
        arguments, its ids kept on the device), lxo_mrt_candidates (each image's reference -- include_reference -- and its distinct draws as padded rows
        with their edit-distance costs, as Img2SeqModel.mrt_batch builds them on the host, in the same order), ONE index_select of the images by the
        rows' image, then mrt_step's sequence on those R = B (n + include_reference) rows -- forward, lxo_score_tokens, lxo_mrt_weights, the weighted
        loss with row_weights = w and normaliser B, backward, the guarded optimizer step -- with lengths, group offsets and costs read from the device.
        The rows the duplicates leave empty are dead: length 0, w = q = 0.
        ref int32 [B, Tr] and ref_lengths [B] in pad_batch_formulas' layout (host arrays or device tensors).
        -> (risk / B = the mean expected cost BEFORE the update, info): info holds host arrays, dead rows stripped -- "cand" int32 [rows, Tc],
        "cand_lengths" [rows], "group_sizes" [B], "cost" f32 [rows], "q" f32 [rows].
        The host sees the decode loop's step count (as in every decode) and makes one copy at the end; because of that count the call cannot be
        captured into a graph.  A step a chain failed in is redone on the same device candidates, not on a fresh draw.  Single process: there is no
        data-parallel form.
        cost = "bleu": the rows cost 1 - sentence BLEU against their image's reference (lxo_mrt_candidates_cost with LXO_COST_BLEU; sentence_bleu's
        definition) in place of the edit distance; the reference's own row still costs 0 exactly.  Then max_iter is bounded by the kernel's width."""
        kind = _cost_kind("mrt_sample_step", cost)
        if kind == _abi.LXO_COST_BLEU and int(max_iter) > _abi.LXO_EDIT_MAX_REF - 1:
            raise ValueError("mrt_sample_step: cost = \"bleu\" takes rows of at most %d tokens, max_iter = %d" % (_abi.LXO_EDIT_MAX_REF - 1, int(max_iter)))
        B = int(img.shape[0])
        ref_d, rl_d = self._to_dev(ref, torch.int32), self._to_dev(ref_lengths, torch.int32).reshape(-1)
        if ref_d.dim() != 2 or int(ref_d.shape[0]) != B or int(rl_d.shape[0]) != B or int(ref_d.shape[1]) < 1:
            raise ValueError("mrt_sample_step: ref must be [B, Tr >= 1] and ref_lengths [B] for B = %d images, got %s and %s"
                             % (B, list(ref_d.shape), list(rl_d.shape)))
        Tr = int(ref_d.shape[1])
        if Tr > _abi.LXO_EDIT_MAX_REF:
            raise ValueError("mrt_sample_step: references of %d tokens exceed the edit-distance kernel's limit of %d" % (Tr, _abi.LXO_EDIT_MAX_REF))
        if not (0 <= int(id_end) < self.n_tok and 0 <= int(id_pad) < self.n_tok):
            raise ValueError("mrt_sample_step: id_end = %d and id_pad = %d must lie in [0, %d)" % (int(id_end), int(id_pad), self.n_tok))
        if not (math.isfinite(float(alpha)) and float(alpha) > 0.0 and math.isfinite(float(np.float32(alpha)))):
            raise ValueError("mrt_sample_step: alpha must be positive and finite, got %r" % (alpha,))
        drop = None
        if dropout is not None and 0.0 < float(dropout) < 1.0:
            self.drop_step = getattr(self, "drop_step", 0) + 1
            drop = (float(dropout), self.drop_step)
        if self._health_ring is not None:
            self._chain_health_poll()
        img_d = self._to_dev(img, torch.uint8)
        ids, _, _, _, steps, _ = self._sample_device(img_d, id_end, n, temperature, top_k, top_p, seed, max_iter)
        n, inc = int(n), 1 if include_reference else 0
        R, Tc = B * (n + inc), max(steps + 1, Tr)
        # ONE device buffer for what the candidate kernels write: cand [R, Tc] | cand_len [R] | cost f32 [R] | group_off [B + 1] | row_image [R]
        cbuf = torch.empty(R * Tc + 3 * R + B + 1, dtype=torch.int32, device=self.device)
        o = np.cumsum([0, R * Tc, R, R, B + 1, R])
        cand, cand_len, cost, group_off, row_image = [cbuf[o[i]:o[i + 1]] for i in range(5)]
        cargs = (_p(ids), B, int(ids.shape[1]), n, steps, _p(ref_d), Tr, _p(rl_d), int(id_end), int(id_pad), inc,
                 _p(cand), _p(cand_len), _p(cost.view(torch.float32)), _p(group_off), _p(row_image))
        if kind == _abi.LXO_COST_EDIT:
            self._ck(self.lib.lxo_mrt_candidates(*(cargs + (self._stream(),))), "mrt_candidates")
        else:
            self._ck(self.lib.lxo_mrt_candidates_cost(*(cargs + (kind, self._stream()))), "mrt_candidates")
        rows_img = img_d.index_select(0, row_image.to(torch.int64))
        redone = False
        while True:
            risk, q, _ = self._mrt_grads_dev(rows_img, cand.view(R, Tc), cand_len, cost.view(torch.float32), group_off, B, R, alpha, drop, keep=cbuf)
            self.optimizer_step(lr, clip, guard=True)
            h = torch.cat([cbuf, risk.view(torch.int32), q.view(torch.int32)]).cpu().numpy()
            if (self._health_ring is not None and self._chain_health_poll(wait=True) and getattr(self, "_last_dropped_seq", -1) == self._health_i
                    and not redone):
                redone = True                                      # as mrt_step: dropped on the device; again on the launch-per-step kernels, same candidates and masks
                continue
            break
        off = h[o[3]:o[4]]
        live = int(off[B])
        info = {"cand": h[:R * Tc].reshape(R, Tc)[:live].copy(), "cand_lengths": h[o[1]:o[2]][:live].copy(), "group_sizes": np.diff(off).astype(np.int32),
                "cost": h[o[2]:o[3]].view(np.float32)[:live].copy(), "q": h[o[5] + 1:].view(np.float32)[:live].copy()}
        return float(h[o[5]:o[5] + 1].view(np.float32)[0]) / B, info

    def edit_distance(self, hyp, ref, hyp_lengths=None, ref_lengths=None, id_end=None, ref_index=None, return_cost=False):
        """Batched Levenshtein distance on the device (lxo_edit_distance): hyp [pairs, T] and ref [G, Tr] token ids, host arrays or device tensors.
        Pair p compares hyp[p] with ref[ref_index[p]]; without ref_index, pairs must be a multiple of G and hypothesis p belongs to reference
        p // (pairs // G) (G = pairs: row by row).  A side's sequence is its first *_lengths tokens (None: the whole row) cut at the first id_end
        (None: no cut) -- pad_batch_formulas' rows and lengths are taken as they are.  -> int32 [pairs], with return_cost also f32 [pairs] =
        distance / max(reference tokens, 1), bit for bit np.float32 of the host's quotient.  A ValueError before any launch for a shape mismatch, a
        reference row longer than the kernel's limit (LXO_EDIT_MAX_REF), or an index outside [0, G) in a host ref_index."""
        h, r = self._to_dev(hyp, torch.int32), self._to_dev(ref, torch.int32)
        if h.dim() != 2 or r.dim() != 2:
            raise ValueError("edit_distance: hyp must be [pairs, T] and ref [G, Tr], got %s and %s" % (list(h.shape), list(r.shape)))
        pairs, T, G, Tr = int(h.shape[0]), int(h.shape[1]), int(r.shape[0]), int(r.shape[1])
        if Tr > _abi.LXO_EDIT_MAX_REF:
            raise ValueError("edit_distance: reference rows of %d tokens exceed the kernel's limit of %d (the hypothesis side has none)" % (Tr, _abi.LXO_EDIT_MAX_REF))
        if pairs > 0 and G < 1:
            raise ValueError("edit_distance: %d hypotheses but no reference" % pairs)
        hl = rl = ri = None
        if hyp_lengths is not None:
            hl = self._to_dev(hyp_lengths, torch.int32)
            if tuple(hl.shape) != (pairs,):
                raise ValueError("edit_distance: hyp_lengths must be [pairs = %d], got %s" % (pairs, list(hl.shape)))
        if ref_lengths is not None:
            rl = self._to_dev(ref_lengths, torch.int32)
            if tuple(rl.shape) != (G,):
                raise ValueError("edit_distance: ref_lengths must be [G = %d], got %s" % (G, list(rl.shape)))
        per_ref = 1
        if ref_index is not None:
            if not isinstance(ref_index, torch.Tensor):
                a = np.asarray(ref_index)
                if a.shape == (pairs,) and a.size and (a.min() < 0 or a.max() >= G):
                    raise ValueError("edit_distance: ref_index must lie in [0, G = %d), got %d .. %d" % (G, int(a.min()), int(a.max())))
            ri = self._to_dev(ref_index, torch.int32)
            if tuple(ri.shape) != (pairs,):
                raise ValueError("edit_distance: ref_index must be [pairs = %d], got %s" % (pairs, list(ri.shape)))
        elif pairs:
            if pairs % G:
                raise ValueError("edit_distance: without ref_index the %d hypotheses must be a multiple of the %d references" % (pairs, G))
            per_ref = pairs // G
        if pairs == 0:
            return (np.zeros(0, np.int32), np.zeros(0, np.float32)) if return_cost else np.zeros(0, np.int32)
        dist = torch.empty(pairs, dtype=torch.int32, device=self.device)
        cost = torch.empty(pairs, dtype=torch.float32, device=self.device) if return_cost else None
        if T == 0:                                                 # hypotheses without a column: a row to point at, none of it read
            h = torch.zeros(pairs, 1, dtype=torch.int32, device=self.device)
        if Tr == 0:                                                # references without a column: every distance is the hypothesis' length
            r, Tr = torch.zeros(max(G, 1), 1, dtype=torch.int32, device=self.device), 1
            rl = torch.zeros(max(G, 1), dtype=torch.int32, device=self.device)
        self._ck(self.lib.lxo_edit_distance(_p(h), 1, T, 0, 1, T, _p(hl), _p(r), G, Tr, _p(rl), _p(ri), per_ref, pairs, -1 if id_end is None else int(id_end),
                                            _p(dist), _p(cost), self._stream()), "edit_distance")
        return (dist.cpu().numpy(), cost.cpu().numpy()) if return_cost else dist.cpu().numpy()

    def text_stats(self, hyp, ref, hyp_lengths=None, ref_lengths=None, id_end=None, ref_index=None, corpus=None):
        """The counts the text metrics are made of, per pair, on the device (lxo_text_stats): -> int32 [pairs, 12] = the clipped n-gram matches for
        n = 1 .. 4, the totals max(1, |h| - n + 1), |h|, |r|, the Levenshtein distance and 1 for h == r (include/lxo.h holds the definition).
        hyp [pairs, T] and ref [G, Tr] token ids, lengths, id_end and ref_index as edit_distance takes them, host arrays or device tensors; a device
        int32 tensor is read in place through its own strides, and hyp may also be the [B, T, n] ids of sample_decode (a view such as
        x.permute(0, 2, 1) of rows [B, n, T] included): pair b * n + j is draw j of image b.  corpus: a device int64 [14] tensor the call ADDS its
        column sums into and leaves on the device (model/evaluation/text.py scores_from_counts reads such a row), so an evaluation accumulates
        batch after batch and copies 14 integers out at its end.  A ValueError before any launch as edit_distance's, and for a hypothesis or
        reference wider than the kernel's limit (LXO_EDIT_MAX_REF) or a corpus that is not a device int64 [14] tensor."""
        stats, _ = self._text_stats_device("text_stats", hyp, ref, hyp_lengths, ref_lengths, id_end, ref_index, True, corpus, 1)
        return stats.cpu().numpy()

    def text_metrics(self, hyp, ref, hyp_lengths=None, ref_lengths=None, id_end=None, ref_index=None):
        """{"BLEU-4", "ExactMatchScore", "EditDistance"} x 100 -- score_files' dict -- of the pairs of one text_stats call, from its corpus row alone:
        one launch sequence, one copy of 14 integers, the floats of the host bleu_score / exact_match_score / edit_distance on the cut sequences."""
        from .model.evaluation.text import scores_from_counts
        _, corpus = self._text_stats_device("text_metrics", hyp, ref, hyp_lengths, ref_lengths, id_end, ref_index, False, None, 0)
        return scores_from_counts(corpus.cpu().numpy())

    def _pair_args(self, what, hyp, ref, hyp_lengths, ref_lengths, ref_index):
        """The pairs of text_stats / sentence_bleu on the device, checked: -> (h, block, geom, T, hl, r, G, Tr, rl, ri, per_ref, pairs), the arguments
        of lxo_text_stats' addressing in its order (sides without a column not yet replaced: _pair_fill)."""
        h = hyp if isinstance(hyp, torch.Tensor) and hyp.device == self.device and hyp.dtype == torch.int32 else self._to_dev(hyp, torch.int32)
        r = self._to_dev(ref, torch.int32)
        if h.dim() not in (2, 3) or r.dim() != 2:
            raise ValueError("%s: hyp must be [pairs, T] or [B, T, n] and ref [G, Tr], got %s and %s" % (what, list(h.shape), list(r.shape)))
        T, G, Tr = int(h.shape[1]), int(r.shape[0]), int(r.shape[1])
        if h.dim() == 3:
            block, pairs, geom = int(h.shape[2]), int(h.shape[0]) * int(h.shape[2]), (int(h.stride(0)), int(h.stride(2)), int(h.stride(1)))
        else:
            block, pairs, geom = 1, int(h.shape[0]), (int(h.stride(0)), 0, int(h.stride(1)))
        if T > _abi.LXO_EDIT_MAX_REF or Tr > _abi.LXO_EDIT_MAX_REF:
            raise ValueError("%s: rows of %d (hypotheses) and %d (references) tokens exceed the kernel's limit of %d" % (what, T, Tr, _abi.LXO_EDIT_MAX_REF))
        if pairs > 0 and G < 1:
            raise ValueError("%s: %d hypotheses but no reference" % (what, pairs))
        hl = rl = ri = None
        if hyp_lengths is not None:
            hl = self._to_dev(hyp_lengths, torch.int32)
            if tuple(hl.shape) != (pairs,):
                raise ValueError("%s: hyp_lengths must be [pairs = %d], got %s" % (what, pairs, list(hl.shape)))
        if ref_lengths is not None:
            rl = self._to_dev(ref_lengths, torch.int32)
            if tuple(rl.shape) != (G,):
                raise ValueError("%s: ref_lengths must be [G = %d], got %s" % (what, G, list(rl.shape)))
        per_ref = 1
        if ref_index is not None:
            if not isinstance(ref_index, torch.Tensor):
                a = np.asarray(ref_index)
                if a.shape == (pairs,) and a.size and (a.min() < 0 or a.max() >= G):
                    raise ValueError("%s: ref_index must lie in [0, G = %d), got %d .. %d" % (what, G, int(a.min()), int(a.max())))
            ri = self._to_dev(ref_index, torch.int32)
            if tuple(ri.shape) != (pairs,):
                raise ValueError("%s: ref_index must be [pairs = %d], got %s" % (what, pairs, list(ri.shape)))
        elif pairs:
            if pairs % G:
                raise ValueError("%s: without ref_index the %d hypotheses must be a multiple of the %d references" % (what, pairs, G))
            per_ref = pairs // G
        return h, block, geom, T, hl, r, G, Tr, rl, ri, per_ref, pairs

    def _pair_fill(self, h, T, r, G, Tr, rl):
        """a side without a column gets a word to point at: -> (h, r, Tr, rl)"""
        if T == 0:                                                 # hypotheses without a column: a word to point at, none of it read
            h = torch.zeros(1, dtype=torch.int32, device=self.device)
        if Tr == 0:                                                # references without a column: every reference is empty
            r, Tr = torch.zeros(max(G, 1), 1, dtype=torch.int32, device=self.device), 1
            rl = torch.zeros(max(G, 1), dtype=torch.int32, device=self.device)
        return h, r, Tr, rl

    def _text_stats_device(self, what, hyp, ref, hyp_lengths, ref_lengths, id_end, ref_index, want_stats, corpus, accumulate):
        """text_stats' checks and its call: -> (stats int32 [pairs, 12] or None, corpus int64 [14]), both left on the device.  corpus None: a fresh row."""
        h, block, geom, T, hl, r, G, Tr, rl, ri, per_ref, pairs = self._pair_args(what, hyp, ref, hyp_lengths, ref_lengths, ref_index)
        if corpus is None:
            corpus = torch.zeros(_abi.LXO_TEXT_CORPUS, dtype=torch.int64, device=self.device)
        elif (not isinstance(corpus, torch.Tensor) or corpus.device != self.device or corpus.dtype != torch.int64 or tuple(corpus.shape) != (_abi.LXO_TEXT_CORPUS,)
              or not corpus.is_contiguous()):
            raise ValueError("%s: corpus must be a contiguous int64 [%d] tensor on %s" % (what, _abi.LXO_TEXT_CORPUS, self.device))
        stats = torch.empty(pairs, _abi.LXO_TEXT_STATS, dtype=torch.int32, device=self.device) if want_stats else None
        if pairs == 0:                                             # nothing to count: the rows are empty, the corpus stays as it is
            return stats, corpus
        h, r, Tr, rl = self._pair_fill(h, T, r, G, Tr, rl)
        self._ck(self.lib.lxo_text_stats(_p(h), block, geom[0], geom[1], geom[2], T, _p(hl), _p(r), G, Tr, _p(rl), _p(ri), per_ref, pairs,
                                         -1 if id_end is None else int(id_end), _p(stats), _p(corpus), int(accumulate), self._stream()), what)
        return stats, corpus

    def edit_align(self, hyp, ref, hyp_lengths=None, ref_lengths=None, id_end=None, ref_index=None, corpus=None, confusion=None, return_maps=True):
        """The edit alignment of every pair on the device (lxo_edit_align; include/lxo.h holds the definition and the path rule): WHERE a hypothesis
        differs from its reference.  -> Alignment(hyp_align, ref_align, counts, corpus, confusion): hyp_align int32 [pairs, T] = per hypothesis
        position the reference position it is aligned with, -1 for an inserted token, -2 behind the sequence; ref_align int32 [pairs, Tr] likewise
        with -1 for a deleted token (both None with return_maps=False); counts int32 [pairs, 6] = matches, substitutions, insertions, deletions,
        |h|, |r| -- host arrays.  hyp, ref, the lengths, id_end and ref_index as text_stats takes them: host arrays, device tensors, strided views
        and the [B, T, n] ids of sample_decode read in place.
        corpus: a device int64 [8] tensor the call ADDS into (the column sums of the counts, the pairs, the steps left out of the matrix), or True
        for a fresh one; confusion: a device int64 [V + 1, V + 1] tensor the call adds its alignment steps into -- [a][b] = reference token a
        against hypothesis token b, index V = no token -- or True for a fresh one over this engine's vocabulary.  Both come back in the result,
        left on the device (None when not asked for): an evaluation accumulates batch after batch and copies once
        (model/evaluation/text.py error_report reads them).  A ValueError before any launch as text_stats', and for a corpus or confusion of another
        kind."""
        ha, ra, counts, corpus, confusion = self._edit_align_device("edit_align", hyp, ref, hyp_lengths, ref_lengths, id_end, ref_index, return_maps, True,
                                                                    corpus, confusion)
        host = lambda t: None if t is None else t.cpu().numpy()
        return Alignment(host(ha), host(ra), host(counts), corpus, confusion)

    def _edit_align_device(self, what, hyp, ref, hyp_lengths, ref_lengths, id_end, ref_index, want_maps, want_counts, corpus, confusion):
        """edit_align's checks and its call: -> (hyp_align, ref_align, counts, corpus, confusion), all left on the device, None where not asked for.
        corpus / confusion: None, True (a fresh zeroed tensor) or the tensor to add into.  The scratch is one cached tensor that grows."""
        h, block, geom, T, hl, r, G, Tr, rl, ri, per_ref, pairs = self._pair_args(what, hyp, ref, hyp_lengths, ref_lengths, ref_index)
        if corpus is True:
            corpus = torch.zeros(_abi.LXO_ALIGN_CORPUS, dtype=torch.int64, device=self.device)
        elif corpus is not None and (not isinstance(corpus, torch.Tensor) or corpus.device != self.device or corpus.dtype != torch.int64
                                     or tuple(corpus.shape) != (_abi.LXO_ALIGN_CORPUS,) or not corpus.is_contiguous()):
            raise ValueError("%s: corpus must be True or a contiguous int64 [%d] tensor on %s" % (what, _abi.LXO_ALIGN_CORPUS, self.device))
        if confusion is True:
            confusion = torch.zeros(self.n_tok + 1, self.n_tok + 1, dtype=torch.int64, device=self.device)
        elif confusion is not None and (not isinstance(confusion, torch.Tensor) or confusion.device != self.device or confusion.dtype != torch.int64
                                        or confusion.dim() != 2 or confusion.shape[0] != confusion.shape[1] or confusion.shape[0] < 2
                                        or not confusion.is_contiguous()):
            raise ValueError("%s: confusion must be True or a contiguous square int64 [V + 1, V + 1] tensor on %s, V >= 1" % (what, self.device))
        ha = torch.empty(pairs, T, dtype=torch.int32, device=self.device) if want_maps else None
        ra = torch.empty(pairs, Tr, dtype=torch.int32, device=self.device) if want_maps else None
        counts = torch.empty(pairs, _abi.LXO_ALIGN_COUNTS, dtype=torch.int32, device=self.device) if want_counts or (corpus is None and confusion is None) else None
        if pairs == 0:                                             # nothing to align: the rows are empty, the sums stay as they are
            return ha, ra, counts, corpus, confusion
        if Tr == 0 and ra is not None:                             # (the call below sees references of one unread column)
            ra_call = torch.empty(pairs, 1, dtype=torch.int32, device=self.device)
        else:
            ra_call = ra
        h, r, Tr, rl = self._pair_fill(h, T, r, G, Tr, rl)
        need = int(self.lib.lxo_edit_align_scratch_bytes(pairs, T, Tr))
        if getattr(self, "_align_scratch", None) is None or self._align_scratch.numel() < need:
            self._align_scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        self._ck(self.lib.lxo_edit_align(_p(h), block, geom[0], geom[1], geom[2], T, _p(hl), _p(r), G, Tr, _p(rl), _p(ri), per_ref, pairs,
                                         -1 if id_end is None else int(id_end), _p(ha) if T else None, _p(ra_call), _p(counts), _p(corpus), _p(confusion),
                                         int(confusion.shape[0]) - 1 if confusion is not None else 1, 1, _p(self._align_scratch), self._align_scratch.numel(),
                                         self._stream()), what)
        return ha, ra, counts, corpus, confusion

    def attention_locate(self, alpha, lengths=None, src=None, mass=0.9, coverage=False):
        """WHERE in the image each token is (lxo_attention_locate; include/lxo.h holds the definition): every attention map reduced on the device
        to its arg-max cell, the central-mass box of its marginals and eight statistics.  alpha: the maps [rows, steps, H', W'] f32, a host array
        or a device tensor -- a strided view (a decode's [max_steps, rows, Rp] buffer permuted, a slice) is read in place as long as each map's
        H' W' cells are contiguous.  lengths [rows] (None: every step): positions t >= lengths[i] have no map.  src int32 [steps, rows2] (None:
        row i reads its own maps): position (i, t) reads alpha[src[t, i], t]; an index outside [0, rows) gives no map.  mass in (0, 1]: the box
        leaves (1 - mass) / 2 of each marginal outside on either side.
        -> Locations(peak int32 [rows, steps] (-1: no map), box int32 [rows, steps, 4] = x0, y0, x1, y1 inclusive in feature cells (-1),
        stats f32 [rows, steps, 8] = S, cx, cy, sx, sy, entropy, inside, peak_share (0), coverage f32 [rows, H', W'] = the row's maps added
        in ascending step (None without coverage=True)), host arrays.  attention_locate_dev leaves them on the device."""
        return Locations(*[None if a is None else a.cpu().numpy() for a in self.attention_locate_dev(alpha, lengths, src, mass, coverage)])

    def attention_locate_dev(self, alpha, lengths=None, src=None, mass=0.9, coverage=False):
        """attention_locate with its outputs left on the device"""
        a = alpha.to(self.device) if isinstance(alpha, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(alpha, dtype=np.float32)).to(self.device)
        if a.dim() != 4 or a.dtype != torch.float32:
            raise ValueError("attention_locate: alpha must be f32 [rows, steps, H', W'], got %s %s" % (a.dtype, tuple(a.shape)))
        AR, steps, Hp, Wp = (int(v) for v in a.shape)
        if Hp < 1 or Wp < 1 or Hp * Wp > _abi.LXO_LOCATE_MAX_CELLS:
            raise ValueError("attention_locate: a map of %d x %d cells; 1 .. %d cells are taken" % (Hp, Wp, _abi.LXO_LOCATE_MAX_CELLS))
        if (Wp > 1 and a.stride(3) != 1) or (Hp > 1 and a.stride(2) != Wp):
            a = a.contiguous()                                     # a map's cells must lie together; rows and steps may be strided
        rows = AR
        if src is not None:
            src = self._to_dev(src, torch.int32)
            if src.dim() != 2 or int(src.shape[0]) != steps:
                raise ValueError("attention_locate: src must be int32 [steps = %d, rows], got %s" % (steps, tuple(src.shape)))
            src, rows = src.contiguous(), int(src.shape[1])
        if lengths is not None:
            lengths = self._to_dev(lengths, torch.int32).reshape(-1).contiguous()
            if int(lengths.shape[0]) != rows:
                raise ValueError("attention_locate: lengths must be [rows = %d], got %s" % (rows, tuple(lengths.shape)))
        return self._locate(a, a.stride(1) if steps > 1 else 0, a.stride(0) if AR > 1 else 0, AR, Hp, Wp, rows, steps, lengths, src, mass, coverage)

    def _locate(self, alpha, step_stride, row_stride, alpha_rows, Hp, Wp, rows, steps, len_dev, src_dev, mass, coverage, per_position=True):
        """The lxo_attention_locate call on maps where they lie (strides in floats): -> Locations of device tensors.  per_position=False: the
        coverage alone (peak, box and stats None)"""
        mass = float(mass)
        if not 0.0 < mass <= 1.0:
            raise ValueError("mass must lie in (0, 1], got %r" % mass)
        peak = torch.empty(rows, steps, dtype=torch.int32, device=self.device) if per_position else None
        box = torch.empty(rows, steps, 4, dtype=torch.int32, device=self.device) if per_position else None
        stats = torch.empty(rows, steps, _abi.LXO_LOCATE_STATS, dtype=torch.float32, device=self.device) if per_position else None
        cov = torch.empty(rows, Hp, Wp, dtype=torch.float32, device=self.device) if coverage else None
        self._ck(self.lib.lxo_attention_locate(_p(alpha), int(step_stride), int(row_stride), int(alpha_rows), Hp, Wp, rows, steps, _p(len_dev), _p(src_dev),
                                               mass, _p(peak), _p(box), _p(stats), _p(cov), Hp * Wp, self._stream()), "attention_locate")
        return Locations(peak, box, stats, cov)

    def _end_lengths(self, ids, id_end):
        """ids [rows, steps] (device) -> int32 [rows]: the steps through each row's first id_end, all of them without one"""
        if int(ids.shape[1]) == 0:
            return torch.zeros(int(ids.shape[0]), dtype=torch.int32, device=self.device)
        hit = ids == int(id_end)
        first = hit.to(torch.int32).argmax(1).to(torch.int32) + 1
        return torch.where(hit.any(1), first, torch.full_like(first, int(ids.shape[1]))).contiguous()

    def beam_finalize(self, ids, parents, scores=None, id_end=None, steps=None):
        """The hypotheses of a beam decode, back-traced on the device (lxo_beam_finalize; include/lxo.h holds the definition).  ids, parents
        int32 and scores f32 (optional) [B, T, k]: what beam_decode returns, as host arrays, or device tensors of its buffers -- a slice
        buf[:, :n] of a [B, max_steps, k] buffer is read in place.  steps (None: T): the valid steps; what lies behind is not read.
        -> BeamPaths(hyp int32 [B, steps, k]: hyp[b, :, i] = the token path that ends in slot i, id_end behind its first id_end
        (utils/text.beam_backtrace, cut); lengths int32 [B, k]: its tokens through the first id_end; src int32 [steps, B k]: the decoder row each
        token was read off (utils/text.beam_parent_rows transposed: attention_locate's src); tok_logp f32 [B, steps, k]: the differences of the
        running scores along the path, 0 behind its end; seq_logp f32 [B, k]: its frozen score -- the last two None without scores), host arrays.
        A ValueError before any launch for a wrong rank or shape, k outside 1 .. 16, steps outside 1 .. min(T, 1024), and for HOST parents
        outside [0, k) (on the device such a parent is clamped into the range).  beam_finalize_dev leaves the outputs on the device."""
        return BeamPaths(*[None if a is None else a.cpu().numpy() for a in self.beam_finalize_dev(ids, parents, scores, id_end, steps)])

    def beam_finalize_dev(self, ids, parents, scores=None, id_end=None, steps=None):
        """beam_finalize with its outputs left on the device"""
        if id_end is None or int(id_end) < 0:
            raise ValueError("beam_finalize: id_end must be a token id >= 0, got %r" % (id_end,))
        shp = tuple(int(v) for v in ids.shape)
        for name, a in (("parents", parents), ("scores", scores)):
            if a is not None and tuple(int(v) for v in a.shape) != shp:
                raise ValueError("beam_finalize: %s must have the shape of ids %s, got %s" % (name, list(shp), list(a.shape)))
        if len(shp) != 3:
            raise ValueError("beam_finalize: ids must be [B, T, k], got %s" % list(shp))
        B, T, k = shp
        if not 1 <= k <= _abi.LXO_BEAM_MAX_K:
            raise ValueError("beam_finalize: k = %d outside 1 .. %d" % (k, _abi.LXO_BEAM_MAX_K))
        steps = T if steps is None else int(steps)
        if not 1 <= steps <= min(T, _abi.LXO_BEAM_MAX_STEPS):
            raise ValueError("beam_finalize: steps = %d outside 1 .. min(T = %d, %d)" % (steps, T, _abi.LXO_BEAM_MAX_STEPS))
        if not isinstance(parents, torch.Tensor):
            p = np.asarray(parents)[:, :steps]
            if p.size and (p.min() < 0 or p.max() >= k):
                raise ValueError("beam_finalize: a parent outside [0, k = %d)" % k)
        t = [None if a is None else (a if isinstance(a, torch.Tensor) and a.device == self.device and a.dtype == dt else self._to_dev(a, dt))
             for a, dt in ((ids, torch.int32), (parents, torch.int32), (scores, torch.float32))]
        # a [B, ld_t, k] buffer seen through buf[:, :T]: rows of k words, ld_t rows per image; anything else is copied
        lds = {(x.stride(0) // k if B > 1 else T) if (k == 1 or x.stride(2) == 1) and (T == 1 or x.stride(1) == k) and (B == 1 or x.stride(0) % k == 0) else -1
               for x in t if x is not None}
        ld = lds.pop() if len(lds) == 1 else -1
        if ld < T:
            t, ld = [None if x is None else x.contiguous() for x in t], T
        return self._beam_finalize(t[0], t[1], t[2], B, ld, steps, k, int(id_end))

    def _beam_finalize(self, ids, par, sc, B, ld_t, steps, k, id_end):
        """The lxo_beam_finalize call on device buffers [B][ld_t][k]: -> BeamPaths of device tensors"""
        hyp = torch.empty(B, steps, k, dtype=torch.int32, device=self.device)
        ln = torch.empty(B, k, dtype=torch.int32, device=self.device)
        src = torch.empty(steps, B * k, dtype=torch.int32, device=self.device)
        tok = torch.empty(B, steps, k, dtype=torch.float32, device=self.device) if sc is not None else None
        seq = torch.empty(B, k, dtype=torch.float32, device=self.device) if sc is not None else None
        self._ck(self.lib.lxo_beam_finalize(_p(ids), _p(par), _p(sc), B, ld_t, steps, k, id_end, _p(hyp), _p(ln), _p(src), _p(tok), _p(seq), self._stream()),
                 "beam_finalize")
        return BeamPaths(hyp, ln, src, tok, seq)

    def _beam_rerank(self, lengths, seq_logp, coverage, alpha, beta, cov_floor):
        """The lxo_beam_rerank call: lengths / seq_logp [B, k] and coverage [B k, R...] (None) on the device -> (score, post, order) [B, k], on the device"""
        B, k = (int(v) for v in seq_logp.shape)
        score = torch.empty(B, k, dtype=torch.float32, device=self.device)
        post = torch.empty(B, k, dtype=torch.float32, device=self.device)
        order = torch.empty(B, k, dtype=torch.int32, device=self.device)
        R = 0 if coverage is None else int(coverage[0].numel())
        self._ck(self.lib.lxo_beam_rerank(_p(lengths), _p(seq_logp), _p(coverage), R, R, B, k, float(alpha), float(beta), float(cov_floor),
                                          _p(score), _p(post), _p(order), self._stream()), "beam_rerank")
        return score, post, order

    def sentence_bleu(self, hyp, ref, hyp_lengths=None, ref_lengths=None, id_end=None, ref_index=None, return_counts=False):
        """Sentence-level BLEU-4 per pair on the device (lxo_sentence_bleu; include/lxo.h holds the definition: add-one smoothing on the orders
        2 .. 4, 1 exactly for an equal pair, 0 without a common unigram): -> f32 [pairs], and with return_counts also int32 [pairs, 10] = the
        clipped matches and the totals for n = 1 .. 4, |h|, |r| -- columns 0 .. 9 of text_stats.  hyp, ref, the lengths, id_end and ref_index as
        text_stats takes them: host arrays, device tensors, strided views and the [B, T, n] ids of sample_decode read in place.  The cost of
        mrt_sample_step(cost="bleu") and consensus(cost="bleu") is 1 - this.  A ValueError before any launch as text_stats'."""
        h, block, geom, T, hl, r, G, Tr, rl, ri, per_ref, pairs = self._pair_args("sentence_bleu", hyp, ref, hyp_lengths, ref_lengths, ref_index)
        bleu = torch.empty(pairs, dtype=torch.float32, device=self.device)
        counts = torch.empty(pairs, _abi.LXO_BLEU_COUNTS, dtype=torch.int32, device=self.device) if return_counts else None
        if pairs:
            h, r, Tr, rl = self._pair_fill(h, T, r, G, Tr, rl)
            self._ck(self.lib.lxo_sentence_bleu(_p(h), block, geom[0], geom[1], geom[2], T, _p(hl), _p(r), G, Tr, _p(rl), _p(ri), per_ref, pairs,
                                                -1 if id_end is None else int(id_end), _p(counts), _p(bleu), None, self._stream()), "sentence_bleu")
        return (bleu.cpu().numpy(), counts.cpu().numpy()) if return_counts else bleu.cpu().numpy()

    def consensus(self, ids, id_end, weights=None, normalize=True, return_dist=False, cost="edit"):
        """The minimum-risk choice among n transcriptions per image (lxo_consensus): ids [B, T, n] token ids -- what sample_decode returns -- as a
        host array or a device int32 tensor, whose own strides are passed through (a view such as x.permute(0, 2, 1) of rows [B, n, T] is read in
        place).  Draw i of an image is its column cut at the first id_end (None: no cut); risk[b, i] is its expected edit distance to the image's
        draws, sum_j w_j c(i, j) / sum_j w_j with c = distance / max(tokens of draw j, 1) (normalize) or the distance itself, and best[b] the draw of
        least risk, the lower index on ties.  weights [B, n] (None: uniform).  -> (best int32 [B], risk f32 [B, n]) and with return_dist also the
        distances int32 [B, n, n].  A ValueError before any launch for a wrong rank, n outside 1 .. 64, T above the kernel's limit, weights of
        another shape, and host weights that are negative, not finite or sum to 0 in a row (on the device such an entry counts as 0 and such a row
        as all ones).
        cost = "bleu": the cost of a pair is 1 - sentence BLEU of draw i against draw j as the reference (lxo_consensus_bleu; sentence_bleu's
        definition), there is no normalisation -- normalize must be left at its default -- and return_dist returns the f32 cost matrix [B, n, n],
        cost[b, i, j] = c(i, j).  Any other cost than "edit" or "bleu" is a ValueError."""
        _cost_kind("consensus", cost)
        if cost == "bleu" and normalize is not True:
            raise ValueError("consensus: cost = \"bleu\" has no normalisation; leave normalize at its default")
        if isinstance(ids, torch.Tensor) and ids.device == self.device and ids.dtype == torch.int32:
            t = ids
        else:
            t = self._to_dev(ids, torch.int32)
        best, risk, dist = self._consensus_device(t, id_end, weights, normalize, cost)
        out = (best.cpu().numpy(), risk.cpu().numpy())
        return out + (dist.cpu().numpy(),) if return_dist else out

    def _consensus_device(self, ids, id_end, weights=None, normalize=True, cost="edit"):
        """consensus' checks and its call on a device int32 tensor [B, T, n] of any strides: -> (best, risk, dist), left on the device; with
        cost = "bleu" dist is the f32 cost matrix"""
        if ids.dim() != 3:
            raise ValueError("consensus: ids must be [B, T, n], got %s" % list(ids.shape))
        B, T, n = (int(x) for x in ids.shape)
        if not 1 <= n <= _abi.LXO_CONSENSUS_MAX_N:
            raise ValueError("consensus: n = %d draws per image outside 1 .. %d" % (n, _abi.LXO_CONSENSUS_MAX_N))
        if T > _abi.LXO_EDIT_MAX_REF:
            raise ValueError("consensus: draws of %d tokens exceed the edit-distance kernel's limit of %d" % (T, _abi.LXO_EDIT_MAX_REF))
        w = None
        if weights is not None:
            if not isinstance(weights, torch.Tensor):
                a = np.asarray(weights, np.float64)
                if a.shape == (B, n) and (not np.isfinite(a).all() or (a < 0).any() or (a.sum(axis=1) == 0).any()):
                    raise ValueError("consensus: weights must be finite, >= 0 and not all 0 for an image")
            w = self._to_dev(weights, torch.float32)
            if tuple(w.shape) != (B, n):
                raise ValueError("consensus: weights must be [B = %d, n = %d], got %s" % (B, n, list(w.shape)))
        dist = torch.empty(B, n, n, dtype=torch.float32 if cost == "bleu" else torch.int32, device=self.device)
        risk = torch.empty(B, n, dtype=torch.float32, device=self.device)
        best = torch.empty(B, dtype=torch.int32, device=self.device)
        src = ids if T else torch.zeros(1, dtype=torch.int32, device=self.device)          # (no token: a word to point at, none of it read)
        if B and cost == "bleu":
            self._ck(self.lib.lxo_consensus_bleu(_p(src), int(ids.stride(0)), int(ids.stride(2)), int(ids.stride(1)), B, n, T, -1 if id_end is None else int(id_end),
                                                 _p(w), None, _p(dist), _p(risk), _p(best), self._stream()), "consensus")
        elif B:
            self._ck(self.lib.lxo_consensus(_p(src), int(ids.stride(0)), int(ids.stride(2)), int(ids.stride(1)), B, n, T, -1 if id_end is None else int(id_end),
                                            _p(w), 1 if normalize else 0, _p(dist), _p(risk), _p(best), self._stream()), "consensus")
        return best, risk, dist

    def evaluate_batch(self, img, formula, lengths):
        """(sum CE, n_words) of img2seq.py:74-75 for one batch (teacher forced)."""
        self.forward(img, formula)
        n = int(np.asarray(lengths).sum())
        s = self.loss(lengths, 1.0 / max(n, 1)).cpu().numpy()
        return float(s[0]), n

    def score(self, img, formula, lengths, return_top1=False, alternatives=0, allowed=None, locate=False, mass=0.9, coverage=False, return_attention=False):
        """Teacher-forced scoring of given formulas (lxo_score_tokens): -> (logp f32 [B, T], seq f32 [B]) or (logp, top1 int32 [B, T], seq),
        host arrays.  logp[b, t] = log_softmax(logits of step t)[formula[b, t]] for t < lengths[b], 0 after; top1[b, t] = the model's
        arg-max at step t (lower id on ties, the greedy rule), -1 after; seq[b] = the f32 sum of logp[b, :lengths[b]] in ascending t
        (-sum(seq) = evaluate_batch's CE sum up to summation order).  The forward is forward(img, formula) without dropout -- the chain
        batch padding comes with it -- and a batch above 64 is scored in consecutive pieces of at most 64 rows, so each piece can take
        the persistent chain.  Touches no gradient, loss statistic or optimizer state.
        alternatives = k > 0 (lxo_score_alternatives, 1 <= k <= min(16, V)): the tuple gains a last element Alternatives(ids int32 [B, T, k],
        logp f32 [B, T, k], rank int32 [B, T], entropy f32 [B, T]) -- the model's k best tokens at every position (value descending, the lower
        id on ties) with their log-probs, the rank of the given token (0 = the model's top-1) and the entropy of the step in nats; positions
        t >= lengths[b]: -1 / 0 / -1 / 0.  allowed (with alternatives only): a boolean / 0-1 array [V] or [B, V] as the decode calls take it;
        the alternatives then run over each row's allowed tokens (renormalised log-probs, rank -1 for a banned given token, id -1 / logp -inf
        where fewer than k are allowed) while logp / top1 / seq stay the unconstrained values.
        locate=True: the tuple gains the Locations (attention_locate) of the given formula -- peak [B, T], box [B, T, 4], stats [B, T, 8] and, with
        coverage=True, coverage [B, H', W'] -- computed from workspace region `alpha` of each piece's forward before anything is copied: the maps
        themselves stay on the device.  Positions t >= lengths[b] have no map (-1 / -1 / 0).  mass: the box's central mass, in (0, 1].
        return_attention=True: the maps themselves, f32 [B, T, H', W'], as the last element (what lies at t >= lengths[b] means nothing)."""
        if locate and not 0.0 < float(mass) <= 1.0:
            raise ValueError("score: mass must lie in (0, 1], got %r" % (mass,))
        if coverage and not locate:
            raise ValueError("score: coverage=True needs locate=True")
        f = formula.detach().cpu().numpy() if isinstance(formula, torch.Tensor) else np.asarray(formula)
        ln = lengths.detach().cpu().numpy() if isinstance(lengths, torch.Tensor) else np.asarray(lengths)
        f = np.ascontiguousarray(f, dtype=np.int64)
        ln = np.ascontiguousarray(ln, dtype=np.int64).reshape(-1)
        B = int(img.shape[0])
        if f.ndim != 2 or f.shape[0] != B or ln.shape[0] != B:
            raise ValueError("score: formula must be [B, T] and lengths [B] for B = %d images, got %s and %s" % (B, f.shape, ln.shape))
        if f.size and (f.min() < 0 or f.max() >= self.n_tok):
            raise ValueError("score: token ids must lie in [0, %d), got %d .. %d" % (self.n_tok, int(f.min()), int(f.max())))
        if ln.size and (ln.min() < 0 or ln.max() > f.shape[1]):
            raise ValueError("score: lengths must lie in [0, T = %d], got %d .. %d" % (f.shape[1], int(ln.min()), int(ln.max())))
        f, ln = f.astype(np.int32), ln.astype(np.int32)
        k = int(alternatives)
        if k == 0 and allowed is not None:
            raise ValueError("score: allowed= constrains the alternatives only and needs alternatives > 0")
        if k != 0 and not 1 <= k <= min(16, self.n_tok):
            raise ValueError("score: alternatives must lie in 1 .. min(16, V = %d), got %d" % (self.n_tok, k))
        al = self._allow_host(allowed, B, None, 1) if allowed is not None else None
        loc = (float(mass), bool(coverage)) if locate else None
        parts = [self._score_piece(img[i:i + 64], f[i:i + 64], ln[i:i + 64], return_top1, k,
                                   al if al is None or al.shape[0] == 1 else al[i:i + 64], loc, return_attention) for i in range(0, B, 64)]
        logp, seq = np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts])
        out = (logp, np.concatenate([p[1] for p in parts]), seq) if return_top1 else (logp, seq)
        if k:
            out += (Alternatives(*[np.concatenate([p[3][j] for p in parts]) for j in range(4)]),)
        if locate:
            out += (Locations(*[None if parts[0][4][j] is None else np.concatenate([p[4][j] for p in parts]) for j in range(4)]),)
        if return_attention:
            out += (np.concatenate([p[5] for p in parts]),)
        return out

    def _score_piece(self, img, formula, lengths, top1_on, k=0, al=None, loc=None, want_maps=False):
        """-> (logp, top1 or None, seq, the four alternatives arrays or None, the Locations' four host arrays or None, the maps or None)"""
        while True:
            self.forward(img, formula, lengths=np.asarray(lengths, dtype=np.int32).reshape(-1))      # (scoring reads t < lengths[b] only)
            B, T = int(self.shape.B), int(self.shape.T)
            live, n = int(self.live_B), B * T
            ln_dev = self._lengths                                  # zero-filled for the dead rows forward() appended: length 0, logp 0 / top1 -1
            chain = self._chains_possible()
            # ONE device buffer and one copy to the host: logp | top1 | seq | the forward chain's sync words (chain_status's slice)
            # (with alternatives: + ids [n, k] | their logp [n, k] | rank | entropy in front of the sync words)
            na = 2 * n + B                                          # where the alternatives start
            ns = na + (2 * n * k + 2 * n if k else 0)               # ... and the sync words
            buf = torch.empty(ns + (XDEC_STATUS_WORDS if chain else 0), dtype=torch.int32, device=self.device)
            logp, top1, seq = buf[:n].view(torch.float32), buf[n:2 * n] if top1_on else None, buf[2 * n:2 * n + B].view(torch.float32)
            self._ck(self.lib.lxo_score_tokens(self.sref(), _p(self.ws), _p(self._formula), _p(ln_dev), _p(logp), _p(top1), _p(seq),
                                               self._stream()), "score_tokens")
            if k:
                alw = self._allow_args(al, live, B) if al is not None else (None, 0)
                self._ck(self.lib.lxo_score_alternatives(self.sref(), _p(self.ws), _p(self._formula), _p(ln_dev), k, _p(alw[0]), alw[1],
                                                         _p(buf[na:na + n * k]), _p(buf[na + n * k:na + 2 * n * k].view(torch.float32)),
                                                         _p(buf[na + 2 * n * k:na + 2 * n * k + n]), _p(buf[na + 2 * n * k + n:ns].view(torch.float32)),
                                                         self._stream()), "score_alternatives")
            where = maps = None
            if loc is not None or want_maps:
                # region `alpha` [T][B][Rp] read where it lies; the dead fill-up rows lie behind the live ones and are simply not asked for
                from .model.utils.image import encoder_out_hw
                Hp, Wp = encoder_out_hw(int(img.shape[1]), int(img.shape[2]))
                Rp = (Hp * Wp + 7) // 8 * 8
                alpha = self.region("alpha", "f32", (T, B, Rp))
                if loc is not None:
                    where = self._locate(alpha, B * Rp, Rp, B, Hp, Wp, live, T, ln_dev, None, loc[0], loc[1])
                if want_maps:
                    maps = alpha[:, :live, :Hp * Wp].permute(1, 0, 2).reshape(live, T, Hp, Wp)
            if chain:
                buf[ns:].copy_(self.region("xdec_sync", "i32")[:XDEC_STATUS_WORDS])
            h = buf.cpu().numpy()
            out = (h[:n].view(np.float32).reshape(B, T)[:live].copy(), h[n:2 * n].reshape(B, T)[:live].copy() if top1_on else None,
                   h[2 * n:2 * n + B].view(np.float32)[:live].copy())
            if k:
                a = h[na:ns]
                out += ((a[:n * k].reshape(B, T, k)[:live].copy(), a[n * k:2 * n * k].view(np.float32).reshape(B, T, k)[:live].copy(),
                         a[2 * n * k:2 * n * k + n].reshape(B, T)[:live].copy(), a[2 * n * k + n:].view(np.float32).reshape(B, T)[:live].copy()),)
            else:
                out += (None,)
            out += (None if where is None else tuple(None if a is None else a.cpu().numpy() for a in where), None if maps is None else maps.cpu().numpy())
            if chain:
                # a chain that did not assemble (forward() checks the first one itself): the launch-per-step kernels from now on, and
                # this piece again
                used, err = _chain_words(h[ns:])
                self.chain_used = used and not err
                if err:
                    self._chain_fallback("forward", err)
                    continue
            return out

    def score_alternatives_dev(self, img, formula, lengths, k):
        """score(alternatives=k)'s ids int32 [B, T, k] and log-probs f32 [B, T, k] as DEVICE tensors, for a consumer on the device (a student's
        train_step(soft_targets=)): the same forward and lxo_score_alternatives, in pieces of at most 64 rows, but no copy to the host and so no look
        at a later chain's error word -- a failed forward chain leaves NaN log-probs, and the loss made of them says so.  Positions
        t >= lengths[b]: -1 / 0."""
        k = int(k)
        if not 1 <= k <= min(16, self.n_tok):
            raise ValueError("score_alternatives_dev: k must lie in 1 .. min(16, V = %d), got %d" % (self.n_tok, k))
        ids_all, logp_all = [], []
        for i in range(0, int(img.shape[0]), 64):
            ln = lengths[i:i + 64]
            self.forward(img[i:i + 64], formula[i:i + 64], lengths=ln if isinstance(ln, torch.Tensor) else np.asarray(ln, dtype=np.int32).reshape(-1))
            B, T, live = int(self.shape.B), int(self.shape.T), int(self.live_B)
            ids = torch.empty(B, T, k, dtype=torch.int32, device=self.device)
            logp = torch.empty(B, T, k, dtype=torch.float32, device=self.device)
            self._ck(self.lib.lxo_score_alternatives(self.sref(), _p(self.ws), _p(self._formula), _p(self._lengths), k, None, 0, _p(ids), _p(logp),
                                                     None, None, self._stream()), "score_alternatives")
            ids_all.append(ids[:live])
            logp_all.append(logp[:live])
        return (ids_all[0], logp_all[0]) if len(ids_all) == 1 else (torch.cat(ids_all), torch.cat(logp_all))

    # --------------------------------------------------------------- decode --
    def _encode_only(self, img, beam):
        B, H, W = int(img.shape[0]), int(img.shape[1]), int(img.shape[2])
        if beam != self.beam:
            self.beam, self.ws = beam, None
        if self.max_steps <= 0:
            self.max_steps, self.ws = 152, None
        self.ensure(B, H, W, 1)
        self._img = self._to_dev(img, torch.uint8)
        self._ck(self.lib.lxo_encoder_fwd(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), _p(self._img), self._stream()),
                 "encoder_fwd")
        return B

    def _chain_fill_up(self, B, *switches):
        """Would a persistent chain (csrc/xdec.hip) run for B rows once they are filled up to 8, 16, 32 or 64?  The conditions the training and
        the greedy-decode chain share; `switches`: the environment variables that turn that chain or its fill-up off with "0" (beside LXO_XDEC)."""
        d = self.dims
        return (self._chains_possible() and B < 64 and B not in (8, 16, 32)
                and d["C"] == 512 and d["U"] == 512 and d["O"] == 512 and d["E"] == 256
                and not any(os.environ.get(v, "1") == "0" for v in ("LXO_XDEC",) + switches))

    def _train_chain_batch(self, B, H=None, W=None):
        """The batch the persistent training chains (csrc/xdec.hip: xdec_fwd_kernel / xdec_bwd_kernel) take for B samples -- 8, 16, 32 or 64 --
        or B itself where they would not run anyway (mirrors lxo_launch_xdec_fwd's conditions).  LXO_TRAIN_PAD=0 / Engine.pad_train = False
        switch the padding off (the launch-per-step kernels then take the batch as it is)."""
        d = self.dims
        if not self._chain_fill_up(B, "LXO_TRAIN_PAD") or not getattr(self, "pad_train", True) or d.get("row_bilstm"):
            return B
        Bp = next(n for n in (8, 16, 32, 64) if B < n)
        if H is not None and not d.get("cnn"):
            from .model.utils.image import encoder_out_hw
            Hp, Wp = encoder_out_hw(int(H), int(W))
            nq = 32 // (Bp // 8)                                    # attention chunks per sample; a chunk's raw scores stay in LDS (xdec.hip: SCMAX rows)
            if (Hp * Wp + nq - 1) // nq > 2432:
                return B
        return Bp

    def _decode_chain_batch(self, B):
        """The batch the persistent greedy-decode chain (csrc/xdec.hip: xdec_dec_kernel) takes for B images -- 8, 16, 32 or 64 -- or B itself where
        the chain would not run anyway (mirrors lxo_launch_xdec_dec's conditions).  LXO_DECODE_PAD=0 switches the padding off."""
        if not self._chain_fill_up(B, "LXO_DECODE_PAD", "LXO_XDEC_DEC") or self.n_tok > 512:
            return B
        return next(n for n in (8, 16, 32, 64) if B < n)

    def _allow_host(self, allowed, B0, id_end, beam_size):
        """Checks allowed-token sets before any launch: -> bool [1 or B0, V].  allowed: boolean / 0-1 array [V] (one set for the batch) or
        [B, V]; in every row END is allowed and at least max(1, beam_size) tokens are (a beam's first free step selects k candidates)."""
        al = allowed.detach().cpu().numpy() if isinstance(allowed, torch.Tensor) else np.asarray(allowed)
        if al.ndim == 1:
            al = al[None]
        if al.ndim != 2 or al.shape[1] != self.n_tok or al.shape[0] not in (1, B0):
            raise ValueError("allowed must be [V] or [B, V] for B = %d images and V = %d tokens, got shape %s" % (B0, self.n_tok, np.shape(allowed)))
        al = al.astype(bool)
        if id_end is not None:                                     # (Engine.score: no decode, nothing has to end)
            if not 0 <= int(id_end) < self.n_tok:
                raise ValueError("id_end = %d outside [0, %d)" % (int(id_end), self.n_tok))
            if not al[:, int(id_end)].all():
                raise ValueError("allowed rows %s ban id_end = %d" % (np.nonzero(~al[:, int(id_end)])[0].tolist(), int(id_end)))
        need = max(1, int(beam_size))
        if (al.sum(1) < need).any():
            raise ValueError("allowed rows %s allow fewer than max(1, beam_size) = %d tokens" % (np.nonzero(al.sum(1) < need)[0].tolist(), need))
        return al

    def _allow_args(self, al, B0, Bp):
        """Stages checked sets as device bit sets (lxo.h: bit v & 31 of word v >> 5): -> (uint32 words [rows, ld] as an int32 tensor, allow_ld);
        one shared row goes as allow_ld = 0, else row r of a filled-up batch copies row r % B0."""
        words = (self.n_tok + 31) // 32
        bits = np.zeros((al.shape[0], words * 32), bool)
        bits[:, :self.n_tok] = al
        w = np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)
        if al.shape[0] == 1:
            return self._to_dev(w, torch.int32), 0
        return self._to_dev(np.ascontiguousarray(w[np.arange(Bp) % B0]), torch.int32), words

    def _prefix_args(self, prefix, prefix_lengths, B0, Bp, id_end, max_iter, al=None):
        """Checks a forced decode prefix before any launch and stages it on the device: -> (prefix int32 [Bp, ld], ld, lengths int32 [Bp]).
        prefix: ids [B0, T] (None lengths: every row T long); rows >= B0 of a filled-up batch copy row index % B0, as their images do.
        al: the call's allowed-token sets (_allow_host) -- a forced token must be allowed in its row."""
        pf = prefix.detach().cpu().numpy() if isinstance(prefix, torch.Tensor) else np.asarray(prefix)
        pf = np.ascontiguousarray(pf, dtype=np.int64)
        if pf.ndim != 2 or pf.shape[0] != B0:
            raise ValueError("prefix must be [B, T] for B = %d images, got shape %s" % (B0, pf.shape))
        T = int(pf.shape[1])
        if prefix_lengths is None:
            ln = np.full(B0, T, np.int64)
        else:
            ln = prefix_lengths.detach().cpu().numpy() if isinstance(prefix_lengths, torch.Tensor) else np.asarray(prefix_lengths)
            ln = np.ascontiguousarray(ln, dtype=np.int64)
            if ln.shape != (B0,):
                raise ValueError("prefix_lengths must be [B] for B = %d images, got shape %s" % (B0, ln.shape))
        lim = min(T, int(max_iter))
        if ln.size and (ln.min() < 0 or ln.max() > lim):
            raise ValueError("prefix lengths must lie in [0, min(T_prefix, max_iter) = %d], got %d .. %d" % (lim, int(ln.min()), int(ln.max())))
        live = np.arange(T)[None, :] < ln[:, None]                  # the positions each row forces
        if live.any():
            v = pf[live]
            if v.min() < 0 or v.max() >= self.n_tok:
                raise ValueError("prefix ids must lie in [0, %d), got %d .. %d" % (self.n_tok, int(v.min()), int(v.max())))
            if (v == int(id_end)).any():
                rows = sorted(set(np.nonzero(live & (pf == int(id_end)))[0].tolist()))
                raise ValueError("prefix rows %s contain id_end = %d" % (rows, int(id_end)))
            if al is not None:
                r, t = np.nonzero(live)
                bad = ~al[r % al.shape[0], pf[r, t]]
                if bad.any():
                    raise ValueError("prefix rows %s force a token their allowed set bans" % sorted(set(r[bad].tolist())))
        pf = np.where(live, pf, 0)
        if T == 0:
            pf = np.zeros((B0, 1), np.int64)
        rows = np.arange(Bp) % B0
        return (self._to_dev(np.ascontiguousarray(pf[rows], dtype=np.int32), torch.int32), int(pf.shape[1]),
                self._to_dev(np.ascontiguousarray(ln[rows], dtype=np.int32), torch.int32))

    def _grammar_host(self, grammar, id_end, max_iter, B0, al, prefix, prefix_lengths, beam_size):
        """Checks a grammar call's contract before any launch (include/lxo.h): -> the Grammar bound to id_end.  END is a plain token; the static
        sets allow every closer; a prefix obeys the grammar at every forced step, budget included; the effective set of the first free step
        holds at least max(1, beam_size) tokens.  al / prefix: as _allow_host / _prefix_args have checked them."""
        from .grammar import Grammar
        if not isinstance(grammar, Grammar):
            raise ValueError("grammar must be a latex_ocr_amd.grammar.Grammar, got %r" % type(grammar).__name__)
        if grammar.n_tok != self.n_tok:
            raise ValueError("the grammar classifies %d tokens, the vocabulary has %d" % (grammar.n_tok, self.n_tok))
        if int(max_iter) < 0:
            raise ValueError("max_iter = %d < 0" % int(max_iter))
        g = grammar if grammar.id_end == int(id_end) else Grammar(grammar.cls, grammar.max_depth, grammar.budget, int(id_end))
        g._check_end(id_end)
        closers = g.cls < 0
        if al is not None and not al[:, closers].all():
            raise ValueError("allowed rows %s ban a closer of the grammar" % np.nonzero(~al[:, closers].all(1))[0].tolist())
        pf = ln = None
        if prefix is not None:
            pf = np.asarray(prefix.detach().cpu().numpy() if isinstance(prefix, torch.Tensor) else prefix, dtype=np.int64)
            ln = np.full(B0, pf.shape[1], np.int64) if prefix_lengths is None else np.asarray(
                prefix_lengths.detach().cpu().numpy() if isinstance(prefix_lengths, torch.Tensor) else prefix_lengths, dtype=np.int64)
        need = max(1, int(beam_size))
        for b in range(B0):
            state, P = (), int(ln[b]) if pf is not None else 0
            for t in range(P):
                tok = int(pf[b, t])
                if not g.allowed_at(state, t, max_iter)[tok]:
                    raise ValueError("prefix row %d breaks the grammar at step %d: token %d at depth %d with %d steps left"
                                     % (b, t, tok, len(state), int(max_iter) - t))
                state = g.apply(state, tok)
            S = g.allowed_at(state, P, max_iter)
            if al is not None:
                S = S & al[b % al.shape[0]]
            if S.sum() < need:
                raise ValueError("row %d: the grammar leaves %d tokens at its first free step %d, fewer than max(1, beam_size) = %d"
                                 % (b, int(S.sum()), P, need))
        return g

    def _grammar_args(self, g, rows, like):
        """Stages a checked grammar: -> (lxo_grammar, depth int32 shaped like the ids tensor `like`, scratch, the class table kept alive)"""
        cls = self._to_dev(g.cls, torch.int8)
        nbytes = int(self.lib.lxo_grammar_scratch_bytes(int(rows), self.n_tok))
        scratch = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=self.device)
        depth = torch.zeros_like(like)
        return _abi.LxoGrammar(_p(cls), g.n_kinds, g.max_depth, 1 if g.budget else 0), depth, scratch, cls

    def _alpha_buf(self, rows, img):
        """-> (the attention-map output buffer f32 [max_steps, rows, R padded to 8], R, H', W') of a decode over the features of `img`"""
        from .model.utils.image import encoder_out_hw
        Hp, Wp = encoder_out_hw(int(img.shape[1]), int(img.shape[2]))
        R = Hp * Wp
        return torch.zeros(self.max_steps, rows, (R + 7) // 8 * 8, dtype=torch.float32, device=self.device), R, Hp, Wp

    def _run_decode(self, pick, id_end, max_iter):
        """Calls the whole-loop entry point `pick` = (function, name, its prefix / output arguments); -> the number of steps it ran."""
        fn, what, args = pick
        steps = ctypes.c_int(0)
        self._ck(fn(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), int(id_end), int(max_iter), *args, ctypes.byref(steps),
                    self._stream()), what)
        return steps.value

    def _greedy_entry(self, pfx, ids, logp, alpha, alw=None, gram=None):
        """The entry point for the outputs that are present: _scores refuses a null logp_out, _prefix a null prefix, _constrained a null set;
        the plain call is bench.py's.  gram (_grammar_args): the _grammar call, which takes every other argument as nullable."""
        L = self.lib
        if gram is not None:
            pa = (_p(pfx[0]), pfx[1], _p(pfx[2])) if pfx is not None else (None, 0, None)
            aa = (_p(alw[0]), alw[1]) if alw is not None else (None, 0)
            return L.lxo_greedy_decode_grammar, "greedy_decode_grammar", aa + pa + (ctypes.byref(gram[0]), _p(ids), _p(logp), _p(alpha), _p(gram[1]), _p(gram[2]))
        if alw is not None:
            pa = (_p(pfx[0]), pfx[1], _p(pfx[2])) if pfx is not None else (None, 0, None)
            return L.lxo_greedy_decode_constrained, "greedy_decode_constrained", (_p(alw[0]), alw[1]) + pa + (_p(ids), _p(logp), _p(alpha))
        if pfx is not None:
            return L.lxo_greedy_decode_prefix, "greedy_decode_prefix", (_p(pfx[0]), pfx[1], _p(pfx[2]), _p(ids), _p(logp), _p(alpha))
        if logp is not None:
            return L.lxo_greedy_decode_scores, "greedy_decode_scores", (_p(ids), _p(logp), _p(alpha))
        if alpha is not None:
            return L.lxo_greedy_decode_attn, "greedy_decode_attn", (_p(ids), _p(alpha))
        return L.lxo_greedy_decode, "greedy_decode", (_p(ids),)

    def greedy_decode(self, img, id_end, max_iter=151, return_attention=False, return_scores=False, prefix=None, prefix_lengths=None, allowed=None,
                      grammar=None, return_depth=False, return_boxes=False, mass=0.9, coverage=False):
        """ids int32 [B, T'] as pred_test.ids of the greedy graph (decoder.py:64,70).  With return_attention also the
        attention maps alpha f32 [B, T', H', W'] (what the reference collects through its py_func hook,
        attention_mechanism.py:96-105, for visualize_attention.py).
        return_scores: -> (ids, logp) or (ids, alpha, logp), logp f32 [B, T'] = log_softmax(logits)[ids] of every step
        (lxo_greedy_decode_scores); the sequence log-prob of a row is the sum through its first END.
        A batch the persistent decode chain does not take (B not in {8, 16, 32, 64}) is filled up to the next such size with COPIES of its own
        images (rows are independent and a copy finishes with its original, so neither the ids of the real rows nor the step count change):
        20 images decode in 26 us per step on the chain where the launch-per-step kernels take 44.
        prefix / prefix_lengths: decode from a given prefix (lxo_greedy_decode_prefix): ids [B, T_prefix] and lengths [B] (None: T_prefix
        each); row b emits prefix[b, :P_b] first -- its logp there is the model's log-prob of the forced tokens -- and decodes on from there.
        A ValueError before any launch for a shape mismatch, an id outside [0, V), id_end inside a prefix, or a length outside
        [0, min(T_prefix, max_iter)].
        allowed: a token constraint (lxo_greedy_decode_constrained): a boolean / 0-1 array [V] (one set for the batch) or [B, V]; a token
        outside its image's set is never emitted -- the arg-max runs over the allowed columns and logp is renormalised over them (logit -
        logsumexp of the allowed logits).  Combines with the other arguments.  A ValueError before any launch for a wrong shape, END banned
        in a row, no token allowed in a row, or a forced prefix token banned in its row.
        grammar: a latex_ocr_amd.grammar.Grammar (lxo_greedy_decode_grammar): every step's set is `allowed` cut to what the row's own history
        leaves open -- no closer without its opener, no END while something is open and, with the grammar's budget, always room to close
        everything by max_iter -- so every row ends balanced.  Combines with the other arguments; runs the launch-per-step kernels (the
        persistent chain holds no grammar).  return_depth (with grammar): one more output, last: depth int32 [B, T'], the row's open
        delimiters after each step.  A ValueError before any launch for a grammar of another vocabulary size, END not plain, a closer that
        `allowed` bans, a prefix that breaks the grammar.
        return_boxes: one more output, last: the Locations (attention_locate: peak [B, T'], box [B, T', 4], stats [B, T', 8], with coverage=True
        coverage [B, H', W']) of every emitted token, reduced on the device from the alpha_out buffer; a row's steps behind its first END have no
        map.  Like return_attention this selects the launch-per-step path (the persistent chain exports no maps); the maps are copied to the host
        only with return_attention."""
        if return_depth and grammar is None:
            raise ValueError("return_depth needs grammar=")
        if return_boxes and not 0.0 < float(mass) <= 1.0:
            raise ValueError("mass must lie in (0, 1], got %r" % (mass,))
        if self.max_steps < max_iter + 1:
            self.max_steps, self.ws = max_iter + 1, None
        B0 = int(img.shape[0])
        want_maps, return_attention = return_attention, return_attention or return_boxes
        Bp = B0 if return_attention or grammar is not None else self._decode_chain_batch(B0)
        al = self._allow_host(allowed, B0, id_end, 1) if allowed is not None else None
        pfx = self._prefix_args(prefix, prefix_lengths, B0, Bp, id_end, max_iter, al) if prefix is not None else None
        g = self._grammar_host(grammar, id_end, max_iter, B0, al, prefix, prefix_lengths, 1) if grammar is not None else None
        alw = self._allow_args(al, B0, Bp) if al is not None else None
        if Bp != B0:
            img = self._to_dev(img, torch.uint8)
            img = img[torch.arange(Bp, device=img.device) % B0]
        B = self._encode_only(img, 1)
        ids = torch.zeros(B, self.max_steps, dtype=torch.int32, device=self.device)
        logp = torch.zeros(B, self.max_steps, dtype=torch.float32, device=self.device) if return_scores else None
        alpha, R, Hp, Wp = self._alpha_buf(B, img) if return_attention else (None, 0, 0, 0)
        gram = self._grammar_args(g, B, ids) if g is not None else None
        n = self._run_decode(self._greedy_entry(pfx, ids, logp, alpha, alw, gram), id_end, max_iter)
        out = [ids[:B0, :n]]
        if want_maps:
            out.append(alpha[:n, :B0, :R].permute(1, 0, 2).reshape(B0, n, Hp, Wp))
        if return_scores:
            out.append(logp[:B0, :n])
        if return_depth:
            out.append(gram[1][:B0, :n])
        if return_boxes:
            where = self._locate(alpha, B * alpha.shape[2], alpha.shape[2], B, Hp, Wp, B0, n, self._end_lengths(ids[:B0, :n], id_end), None, mass, coverage)
        out = tuple(a.cpu().numpy() for a in out)
        if return_boxes:
            out += (Locations(*[None if a is None else a.cpu().numpy() for a in where]),)
        return out if len(out) > 1 else out[0]

    def _check_beam(self, beam_size):
        """a beam wider than the vocabulary has no k-th candidate at time 0 (tf.nn.top_k raises there too); the kernels take k <= 16"""
        k = int(beam_size)
        if k > self.n_tok:
            raise ValueError("beam width %d exceeds the vocabulary size %d" % (k, self.n_tok))
        if k > 16:
            raise ValueError("beam width %d exceeds 16, the widest beam the decode kernels take" % k)

    def _set_diversity(self, div_gamma, div_prob, div_seed):
        """add_div_penalty of beam_search_decoder_cell.py:258-287 for the bound shape (off at gamma 1 / probability 0)"""
        self.shape.div_gamma, self.shape.div_prob = float(div_gamma or 0.0), float(div_prob or 0.0)
        self.shape.div_seed = int(div_seed) & 0x7FFFFFFF

    # one step at a time: what model/components (the reference's decoder-cell protocol) drives
    def decode_begin(self, img, beam_size=1, max_steps=152, div_gamma=1.0, div_prob=0.0, div_seed=0):
        """initialize(): encoder + attention set-up + initial states for beam_size hypotheses per image."""
        self._check_beam(beam_size)
        if self.max_steps < max_steps:
            self.max_steps, self.ws = int(max_steps), None
        B = self._encode_only(img, int(beam_size))
        self._set_diversity(div_gamma, div_prob, div_seed)
        k = max(1, int(beam_size))
        shp = (B, self.max_steps) if k == 1 else (B, self.max_steps, k)
        self._dec_ids = torch.zeros(*shp, dtype=torch.int32, device=self.device)
        self._dec_par = torch.zeros(*shp, dtype=torch.int32, device=self.device) if k > 1 else None
        self._dec_fin = np.zeros(B * k, dtype=np.int32)
        self._ck(self.lib.lxo_decode_begin(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), self._stream()), "decode_begin")
        return B

    def decode_step(self, time, id_end):
        """step(time): -> (ids [B] or [B, k], parents or None, finished bool [B(, k)], logits f32 [B(, k), V])."""
        un = ctypes.c_int(0)
        self._ck(self.lib.lxo_decode_step(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), int(id_end), int(time),
                                          _p(self._dec_ids), _p(self._dec_par), self._dec_fin.ctypes.data_as(ctypes.c_void_p),
                                          ctypes.byref(un), self._stream()), "decode_step")
        ids = self._dec_ids[:, time].cpu().numpy()
        par = self._dec_par[:, time].cpu().numpy() if self._dec_par is not None else None
        fin = self._dec_fin.astype(bool).reshape(ids.shape)
        Vp = (self.n_tok + 31) // 32 * 32
        logits = self.region("dec_logits", "f32", (ids.size, Vp))[:, :self.n_tok].cpu().numpy().reshape(ids.shape + (self.n_tok,))
        return ids, par, fin, logits

    # the AttentionState as data, and AttentionCell.step alone (model/components/attention_cell.py drives these)
    def _dec_rows(self):
        return int(self.shape.B) * max(1, int(self.beam))

    def decode_get_state(self, time):
        """-> (c [rows, U], h [rows, U], o [rows, O]) float32 host arrays: the state that step `time` starts from."""
        n, U, O = self._dec_rows(), self.dims["U"], self.dims["O"]
        c = torch.empty(n, U, dtype=torch.float32, device=self.device)
        h = torch.empty(n, U, dtype=torch.float32, device=self.device)
        o = torch.empty(n, O, dtype=torch.float32, device=self.device)
        self._ck(self.lib.lxo_decode_state_get(self.sref(), _p(self.ws), int(time), _p(c), _p(h), _p(o), self._stream()), "decode_state_get")
        return c.cpu().numpy(), h.cpu().numpy(), o.cpu().numpy()

    def decode_set_state(self, time, c=None, h=None, o=None, ids=None):
        """Overwrite (parts of) the state that step `time` starts from, and / or the token ids fed with it."""
        n, U, O = self._dec_rows(), self.dims["U"], self.dims["O"]
        dev = []
        for a, shp, dt in ((c, (n, U), torch.float32), (h, (n, U), torch.float32), (o, (n, O), torch.float32), (ids, (n,), torch.int32)):
            if a is None:
                dev.append(None)
                continue
            a = np.ascontiguousarray(a)
            if tuple(a.shape) != shp:
                raise ValueError("decode_set_state: expected shape %s, got %s" % (shp, a.shape))
            dev.append(self._to_dev(a, dt))
        self._ck(self.lib.lxo_decode_state_set(self.sref(), _p(self.ws), int(time), _p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]),
                                               self._stream()), "decode_state_set")
        torch.cuda.current_stream(self.device).synchronize() if self.device.type == "cuda" else None     # the staging tensors die with this frame

    def decode_cell_step(self, time, start_token):
        """AttentionCell.step alone: state of `time` -> state of time + 1; -> logits float32 [rows, V]."""
        self._ck(self.lib.lxo_decode_cell_step(self.sref(), _p(self.params), _p(self.wpack), _p(self.ws), int(time), 1 if start_token else 0,
                                               self._stream()), "decode_cell_step")
        Vp = (self.n_tok + 31) // 32 * 32
        return self.region("dec_logits", "f32", (self._dec_rows(), Vp))[:, :self.n_tok].cpu().numpy()

    def _beam_entry(self, pfx, ids, par, sc, alpha, alw=None, gram=None):
        """The entry point for the outputs that are present (as _greedy_entry; _attn refuses a null alpha_out too)."""
        L = self.lib
        if gram is not None:
            pa = (_p(pfx[0]), pfx[1], _p(pfx[2])) if pfx is not None else (None, 0, None)
            aa = (_p(alw[0]), alw[1]) if alw is not None else (None, 0)
            return L.lxo_beam_decode_grammar, "beam_decode_grammar", aa + pa + (ctypes.byref(gram[0]), _p(ids), _p(par), _p(sc), _p(alpha), _p(gram[1]), _p(gram[2]))
        if alw is not None:
            pa = (_p(pfx[0]), pfx[1], _p(pfx[2])) if pfx is not None else (None, 0, None)
            return L.lxo_beam_decode_constrained, "beam_decode_constrained", (_p(alw[0]), alw[1]) + pa + (_p(ids), _p(par), _p(sc), _p(alpha))
        if pfx is not None:
            return L.lxo_beam_decode_prefix, "beam_decode_prefix", (_p(pfx[0]), pfx[1], _p(pfx[2]), _p(ids), _p(par), _p(sc), _p(alpha))
        if sc is not None:
            return L.lxo_beam_decode_scores, "beam_decode_scores", (_p(ids), _p(par), _p(sc), _p(alpha))
        if alpha is not None:
            return L.lxo_beam_decode_attn, "beam_decode_attn", (_p(ids), _p(par), _p(alpha))
        return L.lxo_beam_decode, "beam_decode", (_p(ids), _p(par))

    def beam_decode(self, img, id_end, beam_size, max_iter=151, return_parents=False, div_gamma=1.0, div_prob=0.0, div_seed=0, return_attention=False,
                    return_scores=False, prefix=None, prefix_lengths=None, allowed=None, grammar=None, return_depth=False, return_boxes=False, mass=0.9,
                    coverage=False, return_nbest=False, length_penalty=0.0, coverage_penalty=0.0, cov_floor=0.01, return_consensus=False,
                    consensus_cost="edit"):
        """ids int32 [B, T', k] as pred_test.ids of the beam graph before the transpose at img2seq.py:241.
        div_gamma / div_prob: add_div_penalty of beam_search_decoder_cell.py:258-287 (off at 1 / 0, the shipped values).
        return_attention: -> (ids, parents, alpha f32 [B, T', k, H', W']): alpha[b, t, j] = the map decoder row j of image b attended with at
        step t (lxo_beam_decode_attn; the rows the reference's py_func tap sees under config.decoding = "beam_search").
        return_scores: -> (ids, parents, scores) or (ids, parents, alpha, scores), scores f32 [B, T', k] = the running log-prob of slot k after
        step t (the beam state's log_probs; lxo_beam_decode_scores): the log-prob of the sequence that back-traces from (t, k).
        prefix / prefix_lengths: per image, as in greedy_decode (lxo_beam_decode_prefix): every slot takes the forced tokens, the beam search
        starts after them.
        allowed: per image, as in greedy_decode (lxo_beam_decode_constrained): log_softmax over the allowed columns, a banned candidate is
        never selected, the diversity penalty ranks among the allowed columns.  Every row must allow at least beam_size tokens.
        grammar / return_depth: as in greedy_decode (lxo_beam_decode_grammar), one state per hypothesis slot, continued from the slot's parent:
        every back-traced hypothesis ends balanced.  depth int32 [B, T', k] (last output; the parents are returned with it).  The first free
        step must leave at least beam_size tokens.
        return_boxes: one more output, last (the parents are returned with it): the Locations of the BACK-TRACED hypotheses -- peak [B, k, T'],
        box [B, k, T', 4], stats [B, k, T', 8], coverage [B, k, H', W'] with coverage=True; entry [b, i] belongs to the hypothesis that ends in
        slot i (utils/text.beam_backtrace's out[b, :, i]).  Its token at step t was read off the row of its parent, so position (b k + i, t)
        reads the map of row b k + parents[b, t, slots[b, t, i]] (beam_slots' rule); that src array is built ON THE HOST from the copied parents
        and the reduction then runs on the device on the alpha_out buffer.  Steps behind a hypothesis' first END have no map.
        return_nbest: the beam FINISHED ON THE DEVICE (lxo_beam_finalize, lxo_beam_rerank) before anything is copied; the outputs above are what
        they are without the flag, and one NBest follows them: hyp int32 [B, T', k] (hyp[b, :, i] = the back-traced path that ends in slot i, END
        behind its first END), lengths int32 [B, k], tok_logp f32 [B, T', k] and seq_logp f32 [B, k] (the path's token log-probs and its frozen
        score), score f32 [B, k] = seq_logp / ((5 + length) / 6)^length_penalty + coverage_penalty * sum_cells log(min(max(coverage, cov_floor), 1))
        (GNMT's normalisation, applied to the k hypotheses the search returned -- the search itself is the reference's), post f32 [B, k] = the
        softmax of seq_logp over the image's slots, order int32 [B, k] = the slots by descending score.  length_penalty = coverage_penalty = 0:
        score is seq_logp.  coverage_penalty > 0 exports the attention maps and sums each hypothesis' coverage (attention_locate's) with the src
        and lengths built on the device; the cells of the batch canvas' padding shift an image's scores together.  With return_nbest,
        return_boxes takes that device-built src too.
        return_consensus (with return_nbest): best int32 [B] and risk f32 [B, k] follow the NBest: the minimum-risk choice among the k
        hypotheses (consensus(); consensus_cost "edit" or "bleu"), read from hyp in place with post as the weights.  The Locations of
        return_boxes stay the very last output."""
        self._check_beam(beam_size)
        if return_depth and grammar is None:
            raise ValueError("return_depth needs grammar=")
        if return_boxes and not 0.0 < float(mass) <= 1.0:
            raise ValueError("mass must lie in (0, 1], got %r" % (mass,))
        if return_nbest:
            _cost_kind("beam_decode: consensus_cost", consensus_cost)
            lp, cpw, fl = float(length_penalty), float(coverage_penalty), float(cov_floor)
            if not (0.0 <= lp < float("inf") and 0.0 <= cpw < float("inf")):
                raise ValueError("beam_decode: length_penalty and coverage_penalty must be finite and >= 0, got %r, %r" % (length_penalty, coverage_penalty))
            if not 0.0 < fl <= 1.0:
                raise ValueError("beam_decode: cov_floor must lie in (0, 1], got %r" % (cov_floor,))
            if max_iter > _abi.LXO_BEAM_MAX_STEPS:
                raise ValueError("beam_decode: return_nbest takes at most %d steps, got max_iter = %d" % (_abi.LXO_BEAM_MAX_STEPS, max_iter))
        elif return_consensus or float(length_penalty) != 0.0 or float(coverage_penalty) != 0.0:
            raise ValueError("beam_decode: length_penalty, coverage_penalty and return_consensus need return_nbest=True")
        with_parents = return_parents or return_attention or return_boxes or return_scores or return_depth
        want_maps, want_scores = return_attention, return_scores
        return_attention = return_attention or return_boxes or (return_nbest and cpw > 0.0)
        return_scores = return_scores or return_nbest
        if self.max_steps < max_iter + 1:
            self.max_steps, self.ws = max_iter + 1, None
        B0 = int(img.shape[0])
        al = self._allow_host(allowed, B0, id_end, beam_size) if allowed is not None else None
        pfx = self._prefix_args(prefix, prefix_lengths, B0, B0, id_end, max_iter, al) if prefix is not None else None
        g = self._grammar_host(grammar, id_end, max_iter, B0, al, prefix, prefix_lengths, beam_size) if grammar is not None else None
        alw = self._allow_args(al, B0, B0) if al is not None else None
        B = self._encode_only(img, int(beam_size))
        self._set_diversity(div_gamma, div_prob, div_seed)
        ids = torch.zeros(B, self.max_steps, beam_size, dtype=torch.int32, device=self.device)
        par = torch.zeros(B, self.max_steps, beam_size, dtype=torch.int32, device=self.device)
        sc = torch.zeros(B, self.max_steps, beam_size, dtype=torch.float32, device=self.device) if return_scores else None
        alpha, R, Hp, Wp = self._alpha_buf(B * beam_size, img) if return_attention else (None, 0, 0, 0)
        gram = self._grammar_args(g, B * int(beam_size), ids) if g is not None else None
        n = self._run_decode(self._beam_entry(pfx, ids, par, sc, alpha, alw, gram), id_end, max_iter)
        out = [ids[:, :n]]
        if with_parents:
            out.append(par[:, :n])
        if want_maps:
            out.append(alpha[:n, :, :R].reshape(n, B, beam_size, Hp, Wp).permute(1, 0, 2, 3, 4).contiguous())
        if want_scores:
            out.append(sc[:, :n])
        if return_depth:
            out.append(gram[1][:, :n])
        if return_nbest:
            return self._beam_nbest(out, ids, par, sc, alpha, (B, int(beam_size), n, Hp, Wp), id_end, lp, cpw, fl, return_consensus, consensus_cost,
                                    (mass, coverage) if return_boxes else None)
        out = tuple(a.cpu().numpy() for a in out)
        if return_boxes:
            from .model.utils.text import beam_backtrace, beam_parent_rows
            k = int(beam_size)
            hyp, src = beam_backtrace(out[0], out[1]), beam_parent_rows(out[1])          # [B, n, k] both
            hit = hyp == int(id_end)
            ln = np.where(hit.any(1), hit.argmax(1) + 1, n).astype(np.int32)             # [B, k]
            where = self._locate(alpha, B * k * alpha.shape[2], alpha.shape[2], B * k, Hp, Wp, B * k, n, self._to_dev(ln.reshape(-1), torch.int32),
                                 self._to_dev(np.ascontiguousarray(src.transpose(1, 0, 2).reshape(n, B * k)), torch.int32), mass, coverage)
            out += (Locations(*[None if a is None else a.cpu().numpy().reshape((B, k) + tuple(a.shape[1:])) for a in where]),)
        return out if len(out) > 1 else out[0]

    def _beam_nbest(self, lead, ids, par, sc, alpha, geo, id_end, length_penalty, coverage_penalty, cov_floor, consensus, consensus_cost, boxes):
        """beam_decode's finish on the device: lead (device tensors) + NBest (+ best, risk) (+ Locations), host arrays.  Everything is enqueued
        before the first copy."""
        B, k, n, Hp, Wp = geo
        fin = self._beam_finalize(ids, par, sc, B, int(ids.shape[1]), n, k, int(id_end))
        where = cov = None
        if boxes is not None or coverage_penalty > 0.0:
            Rp = int(alpha.shape[2])
            where = self._locate(alpha, B * k * Rp, Rp, B * k, Hp, Wp, B * k, n, fin.lengths.reshape(-1), fin.src, boxes[0] if boxes is not None else 0.9,
                                 coverage_penalty > 0.0 or boxes[1], per_position=boxes is not None)
            cov = where.coverage if coverage_penalty > 0.0 else None
        score, post, order = self._beam_rerank(fin.lengths, fin.seq_logp, cov, length_penalty, coverage_penalty, cov_floor)
        tail = list(self._consensus_device(fin.hyp, id_end, post, True, consensus_cost)[:2]) if consensus else []
        out = tuple(a.cpu().numpy() for a in lead)
        out += (NBest(*[a.cpu().numpy() for a in (fin.hyp, fin.lengths, fin.tok_logp, fin.seq_logp, score, post, order)]),)
        out += tuple(a.cpu().numpy() for a in tail)
        if boxes is not None:
            loc = Locations(where.peak, where.box, where.stats, where.coverage if boxes[1] else None)
            out += (Locations(*[None if a is None else a.cpu().numpy().reshape((B, k) + tuple(a.shape[1:])) for a in loc]),)
        return out

    def _sample_opts(self, n, temperature, top_k, top_p, seed):
        """Checks the sampling options before any launch: -> lxo_sample_opts.  temperature = 0 means top_k = 1 (the arg-max)."""
        n, top_k = int(n), int(top_k)
        temperature, top_p = float(temperature), float(top_p)
        if not 1 <= n <= 16:
            raise ValueError("n = %d draws per image outside 1 .. 16" % n)
        if not (temperature >= 0.0 and np.isfinite(temperature)):
            raise ValueError("temperature must be finite and >= 0, got %r" % temperature)
        if top_k < 0:
            raise ValueError("top_k must be >= 0 (0: off), got %d" % top_k)
        if not 0.0 < top_p <= 1.0:
            raise ValueError("top_p must lie in (0, 1] (1: off), got %r" % top_p)
        if temperature == 0.0:
            temperature, top_k = 1.0, 1
        with np.errstate(over="ignore", divide="ignore"):
            t32 = np.float32(temperature)
            if not (t32 > 0 and np.isfinite(t32) and np.isfinite(np.float32(1.0) / t32)):      # what the C call refuses, before the encoder runs
                raise ValueError("temperature %r and its reciprocal must be finite and positive in float32 (0 itself means top_k = 1)" % temperature)
        return _abi.LxoSampleOpts(temperature, top_k, top_p, int(seed) & 0xFFFFFFFF)

    def sample_decode(self, img, id_end, n=1, temperature=1.0, top_k=0, top_p=1.0, seed=0, max_iter=151, return_scores=False, return_attention=False,
                      prefix=None, prefix_lengths=None, allowed=None, grammar=None, return_depth=False, return_consensus=False, consensus_normalize=True, consensus_cost="edit",
                      return_boxes=False, mass=0.9, coverage=False):
        """n independent DRAWS of the whole sequence per image (lxo_sample_decode): ids int32 [B, T', n].  Every step draws from the model's
        distribution at `temperature`, cut to the top_k most likely tokens (0: off) and then to the smallest set of renormalised mass >= top_p
        (1: off); temperature = 0 means top_k = 1, the arg-max.  Draw (b, j) depends only on seed, b, j and the step: the same seed repeats bit for
        bit, and neither n nor the batch changes a draw.  Launch per step in both dtypes (no chain, so no fill-up of the batch).
        return_scores: -> (ids, logp, logq) or (ids, alpha, logp, logq), f32 [B, T', n]: logp = the model's own log-prob of the token (as
        greedy_decode's, renormalised over `allowed`), logq = its log-prob under the distribution it was drawn from (0 at a forced step); the
        sequence log-prob of a draw is the sum through its first END.  return_attention: alpha f32 [B, T', n, H', W'].
        prefix / prefix_lengths / allowed: per image, as in greedy_decode.  A ValueError before any launch for what greedy_decode refuses, n outside
        1 .. min(16, V), temperature < 0 or not finite, top_k < 0, top_p outside (0, 1].
        grammar / return_depth: as in greedy_decode (lxo_sample_decode_grammar), one state per draw: the cut-offs and the draw run over the
        step's effective set, so every draw ends balanced.  depth int32 [B, T', n] (last output).
        return_consensus: the minimum-risk choice among each image's draws (consensus(), uniform weights, consensus_normalize its normalize),
        computed on the ids where the decode left them on the device: best int32 [B] and risk f32 [B, n] are appended as the last two outputs.
        consensus_cost: consensus()'s cost, "edit" or "bleu" (with "bleu" consensus_normalize must be left at its default).
        return_boxes: the very last output: the Locations of every draw -- peak [B, n, T'], box [B, n, T', 4], stats [B, n, T', 8], coverage
        [B, n, H', W'] with coverage=True -- reduced on the device from the alpha_out buffer; steps behind a draw's first END have no map."""
        if return_depth and grammar is None:
            raise ValueError("return_depth needs grammar=")
        if return_boxes and not 0.0 < float(mass) <= 1.0:
            raise ValueError("mass must lie in (0, 1], got %r" % (mass,))
        want_maps, return_attention = return_attention, return_attention or return_boxes
        _cost_kind("sample_decode: consensus_cost", consensus_cost)
        if consensus_cost == "bleu" and consensus_normalize is not True:
            raise ValueError("sample_decode: consensus_cost = \"bleu\" has no normalisation; leave consensus_normalize at its default")
        if return_consensus and int(max_iter) > _abi.LXO_EDIT_MAX_REF:
            raise ValueError("return_consensus: max_iter = %d exceeds the edit-distance kernel's limit of %d tokens" % (int(max_iter), _abi.LXO_EDIT_MAX_REF))
        box = []
        ids, logp, logq, alpha, steps, geo = self._sample_device(img, id_end, n, temperature, top_k, top_p, seed, max_iter, return_scores, return_attention,
                                                                 prefix, prefix_lengths, allowed, grammar, box)
        B, n, R, Hp, Wp = geo
        out = [ids[:, :steps]]
        if want_maps:
            out.append(alpha[:steps, :, :R].reshape(steps, B, n, Hp, Wp).permute(1, 0, 2, 3, 4).contiguous())
        if return_scores:
            out += [logp[:, :steps], logq[:, :steps]]
        if return_depth:
            out.append(box[0][:, :steps])
        if return_consensus:
            out += self._consensus_device(ids[:, :steps], id_end, None, consensus_normalize, consensus_cost)[:2]
        if return_boxes:
            ln = self._end_lengths(ids[:, :steps].permute(0, 2, 1).reshape(B * n, steps), id_end)
            where = self._locate(alpha, B * n * alpha.shape[2], alpha.shape[2], B * n, Hp, Wp, B * n, steps, ln, None, mass, coverage)
        out = tuple(a.cpu().numpy() for a in out)
        if return_boxes:
            out += (Locations(*[None if a is None else a.cpu().numpy().reshape((B, n) + tuple(a.shape[1:])) for a in where]),)
        return out if len(out) > 1 else out[0]

    def _sample_device(self, img, id_end, n, temperature, top_k, top_p, seed, max_iter, return_scores=False, return_attention=False,
                       prefix=None, prefix_lengths=None, allowed=None, grammar=None, depth_box=None):
        """sample_decode's checks and its lxo_sample_decode call, the outputs left on the device: -> (ids int32 [B, max_steps, n], logp, logq, alpha
        (None where not asked for), the steps the loop ran -- the one number the host learns -- and (B, n, R, H', W') for the attention maps).
        grammar: lxo_sample_decode_grammar instead; its depth tensor int32 [B, max_steps, n] is appended to the list depth_box"""
        so = self._sample_opts(n, temperature, top_k, top_p, seed)
        n = int(n)
        if n > self.n_tok:                                             # the decode calls' shape limit (rows per image <= V); the select step alone has none
            raise ValueError("n = %d draws per image exceed the vocabulary size %d" % (n, self.n_tok))
        if self.max_steps < max_iter + 1:
            self.max_steps, self.ws = max_iter + 1, None
        B0 = int(img.shape[0])
        al = self._allow_host(allowed, B0, id_end, 1) if allowed is not None else None
        pfx = self._prefix_args(prefix, prefix_lengths, B0, B0, id_end, max_iter, al) if prefix is not None else None
        g = self._grammar_host(grammar, id_end, max_iter, B0, al, prefix, prefix_lengths, 1) if grammar is not None else None
        alw = self._allow_args(al, B0, B0) if al is not None else (None, 0)
        B = self._encode_only(img, n)
        ids = torch.zeros(B, self.max_steps, n, dtype=torch.int32, device=self.device)
        logp = torch.zeros(B, self.max_steps, n, dtype=torch.float32, device=self.device) if return_scores else None
        logq = torch.zeros(B, self.max_steps, n, dtype=torch.float32, device=self.device) if return_scores else None
        alpha, R, Hp, Wp = self._alpha_buf(B * n, img) if return_attention else (None, 0, 0, 0)
        pa = (_p(pfx[0]), pfx[1], _p(pfx[2])) if pfx is not None else (None, 0, None)
        if g is not None:
            gram = self._grammar_args(g, B * n, ids)
            if depth_box is not None:
                depth_box.append(gram[1])
            steps = self._run_decode((self.lib.lxo_sample_decode_grammar, "sample_decode_grammar",
                                      (ctypes.byref(so), _p(alw[0]), alw[1]) + pa + (ctypes.byref(gram[0]), _p(ids), _p(logp), _p(logq), _p(alpha),
                                                                                      _p(gram[1]), _p(gram[2]))), id_end, max_iter)
            return ids, logp, logq, alpha, steps, (B, n, R, Hp, Wp)
        steps = self._run_decode((self.lib.lxo_sample_decode, "sample_decode",
                                  (ctypes.byref(so), _p(alw[0]), alw[1]) + pa + (_p(ids), _p(logp), _p(logq), _p(alpha))), id_end, max_iter)
        return ids, logp, logq, alpha, steps, (B, n, R, Hp, Wp)

    def sample_tokens(self, logits, n=1, time=0, temperature=1.0, top_k=0, top_p=1.0, seed=0, allowed=None):
        """The sampled select step alone (lxo_sample_tokens) on logits [rows, V] the caller holds (host array or tensor): row r is draw r % n of
        image r // n at step `time`.  -> (ids int32 [rows], logp f32 [rows], logq f32 [rows]).  allowed: [V] or [images, V], images = ceil(rows / n).
        A float32 device tensor with unit column stride is read in place, whatever its row stride (a view of padded rows)."""
        so = self._sample_opts(n, temperature, top_k, top_p, seed)
        in_place = isinstance(logits, torch.Tensor) and logits.device == self.device and logits.dtype == torch.float32 and logits.dim() == 2 and \
            logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1]
        lg = logits if in_place else self._to_dev(logits, torch.float32)
        if lg.dim() != 2 or lg.shape[1] != self.n_tok or lg.shape[0] < 1:
            raise ValueError("logits must be [rows >= 1, V = %d], got shape %s" % (self.n_tok, tuple(lg.shape)))
        if int(time) < 0:
            raise ValueError("time must be >= 0, got %d" % int(time))
        rows, images = int(lg.shape[0]), (int(lg.shape[0]) + int(n) - 1) // int(n)
        alw = self._allow_args(self._allow_host(allowed, images, None, 0), images, images) if allowed is not None else (None, 0)
        ids = torch.zeros(rows, dtype=torch.int32, device=self.device)
        logp = torch.zeros(rows, dtype=torch.float32, device=self.device)
        logq = torch.zeros(rows, dtype=torch.float32, device=self.device)
        self._ck(self.lib.lxo_sample_tokens(_p(lg), int(lg.stride(0)), rows, int(n), self.n_tok, int(time), ctypes.byref(so), _p(alw[0]), alw[1],
                                            _p(ids), _p(logp), _p(logq), self._stream()), "sample_tokens")
        return ids.cpu().numpy(), logp.cpu().numpy(), logq.cpu().numpy()
