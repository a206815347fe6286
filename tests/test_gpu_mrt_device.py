"""-m gpu: minimum-risk training without the host, on the MI355X.

1. lxo_edit_distance on the case matrix of tests/edit_distance_ref.py and lxo_mrt_candidates on its constructed ids, exactly as the hipsim files.
2. Engine.mrt_sample_step in f32 (B = 2, 32 x 128, V = 50, n = 3): the candidates of the host path at the same seed, exactly; q and risk against the
   autograd oracle (tests/mrt_oracle.py) at 1e-5.
3. The same in bf16 with deterministic=True and the reference included: R = 8 rows, the chain batch -- both persistent chains run, the candidates
   equal the host construction from sample_decode, a second fresh engine returns the same q and risk bytes.  The difference to the host-path
   mrt_step on the same candidates is printed, not asserted (no bar for it exists yet; profiles/mrt_on_device.txt records it)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import *  # noqa
from latex_ocr_amd import _abi
from latex_ocr_amd.engine import _p
import mrt_oracle
from edit_distance_ref import (CAND_END, CAND_PAD, CAND_REFS, cand_calls, check_candidates, check_edit_case, constructed_ids, edit_cases, host_candidates,
                               run_candidates)

H, W, V = 32, 128, 50
ID_END, ID_PAD = V - 1, V - 2


class Dev(object):
    """numpy <-> the GPU for the shared runners of tests/edit_distance_ref.py"""
    stream = None

    @staticmethod
    def up(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def ptr(a):
        return _p(a)

    @staticmethod
    def down(a):
        return a.cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


# ------------------------------------------------------------------------------------------------------------------ 1. the kernels --
def test_edit_distance_matrix(lib):
    for c in edit_cases():
        check_edit_case(lib, c, Dev)


@pytest.mark.parametrize("steps,inc", cand_calls())
def test_candidates_on_constructed_ids(lib, steps, inc):
    ids = constructed_ids()
    out = run_candidates(lib, ids, steps, CAND_REFS, CAND_END, CAND_PAD, inc, Dev)
    assert out[0] == 0, lib.lxo_last_error()
    check_candidates(ids, steps, CAND_REFS, CAND_END, CAND_PAD, inc, *out[1:])


# ------------------------------------------------------------------------------------------------------- 2. / 3. the step end to end --
N, ALPHA, MAX_ITER = 3, 1.0, 6
SAMPLING = dict(temperature=0.5, top_k=2, seed=7)                   # few likely tokens per step: draws repeat


def _inputs():
    imgs, forms = synthetic.make_set(2, H, W, V, 3, 5, seed=13)
    ref, rl = pad_batch_formulas(forms, ID_PAD, ID_END)
    return pad_batch_images(imgs), [list(f) for f in forms], ref, rl


def _host_rows(eng, img, refs, inc=True):
    ids = eng.sample_decode(img, ID_END, n=N, max_iter=MAX_ITER, **SAMPLING)
    return host_candidates(ids, refs, ID_END, ID_PAD, inc)


def _same_rows(info, f, ln, sizes, costs):
    assert info["group_sizes"].tolist() == sizes.tolist() and info["cand_lengths"].tolist() == ln.tolist()
    assert info["cost"].tobytes() == costs.tobytes()
    for r in range(len(ln)):
        assert info["cand"][r, :ln[r]].tolist() == f[r, :ln[r]].tolist() and (info["cand"][r, ln[r]:] == ID_PAD).all(), r


def test_mrt_sample_step_f32_against_the_host_path_and_the_oracle():
    img, refs, ref, rl = _inputs()
    eng = Engine(V, dtype="f32", seed=3)
    f, ln, sizes, costs = _host_rows(eng, img, refs)
    P = oracle_params(eng)
    risk_ref, _, q_ref = mrt_oracle.mrt_grads(P, img, f, ln, sizes, costs, ALPHA)
    risk, info = eng.mrt_sample_step(img, ref, rl, ID_END, ID_PAD, 0.0, ALPHA, n=N, max_iter=MAX_ITER, **SAMPLING)
    _same_rows(info, f, ln, sizes, costs)
    print("f32: group sizes %s, risk %.7f oracle %.7f, q max err %.2e" % (sizes.tolist(), risk, risk_ref, np.abs(info["q"] - q_ref).max()))
    assert abs(risk - risk_ref) <= 1e-5 and np.abs(info["q"] - q_ref).max() <= 1e-5


def test_mrt_sample_step_bf16_on_the_chains():
    img, refs, ref, rl = _inputs()
    out = []
    for _ in range(2):
        eng = Engine(V, dtype="bf16", seed=3, deterministic=True)
        f, ln, sizes, costs = _host_rows(eng, img, refs)
        risk, info = eng.mrt_sample_step(img, ref, rl, ID_END, ID_PAD, 0.0, ALPHA, n=N, max_iter=MAX_ITER, **SAMPLING)
        assert int(eng.shape.B) == 8 == 2 * (N + 1)                 # R = 8: the chain batch, dead rows included
        print("bf16: chain_used %s chain_used_bwd %s, group sizes %s, risk %.6f" % (eng.chain_used, eng.chain_used_bwd, sizes.tolist(), risk))
        assert eng.chain_used and eng.chain_used_bwd
        _same_rows(info, f, ln, sizes, costs)
        out.append((np.float32(risk).tobytes(), info["q"].tobytes()))
    assert out[0] == out[1]                                         # deterministic mode: the same q and risk bytes from a second engine
    # the host-path step on the same candidates, printed only: the two paths differ in the padded width Tc and in the dead rows of the batch
    eng = Engine(V, dtype="bf16", seed=3, deterministic=True)
    risk_h, q_h = eng.mrt_step(img, f, ln, sizes, costs, 0.0, ALPHA)
    print("bf16 device path against the host-path mrt_step on the same candidates: |risk - risk_host| %.3e, max |q - q_host| %.3e"
          % (abs(risk - risk_h), np.abs(info["q"] - q_h).max()))
