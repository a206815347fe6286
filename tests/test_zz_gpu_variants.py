"""-m gpu: differential tests of the kernel generations that sit behind A/B switches.  Each pair computes the same
mathematics with different kernels, so they must agree far more tightly than either agrees with the f32 oracle:

* fused conv + max pool epilogue with the one-byte routing mask (default)  vs  separate pool kernels that re-read the
  activation (LXO_POOL_FUSED=0): the same bf16 values are pooled and routed; only the order of f32 atomics differs
  (whose rounding noise the bf16 mirrors downstream amplify to ~1e-3 of a gradient's largest element);
* conv1 + pool on the matrix cores (default)  vs  the VALU kernels with f32 weights (LXO_CONV1_MFMA=0): differs by the
  bf16 rounding of 576 weights;
* attention row blocks walked in alternating directions (default)  vs  always forward (LXO_ATT_ALT=0): summation order;
* dense weight-gradient GEMMs with LDS-DMA tiles + transposing reads (default)  vs  the register-packing kernel
  (LXO_GEMM_TN_TR=0): summation order;
* dense projections (att_img, logits, d_o) with LDS-DMA staging (default)  vs  the register-staged kernel
  (LXO_GEMM_NT_DMA=0): the same products in the same order per output element;
* fused recurrent-step kernels (default)  vs  round 1's split-K kernels (step_kernels = 1);
* the two-workgroup conv kernel with fused pools (default)  vs  the general halo conv kernel + separate pools (LXO_CONV_2WG=0: the
  kernel that shapes outside the model's -- Cout % 64 != 0, tensors of 2 GB and more -- run on);
* 64-channel conv tiles for launches too small to give every CU a 128-channel tile (default)  vs  128-channel tiles always (LXO_CONV_SMALL=0);
* the stream switches: LXO_DUAL_STREAM=1 (off by default: measured slower) and LXO_ENC_OVERLAP=0 (the weight gradients -- the encoder's and the
  decoder's deferred ones -- on the compute stream instead of beside it on a second stream, the default since round 5).
Odd image sizes exercise the clipped pool windows of both generations."""
import os, subprocess, sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _run(tmp, name, env, h, w, b, dtype="bf16"):
    out = os.path.join(str(tmp), name + ".npz")
    e = dict(os.environ); e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "variant_dump.py"), out, str(h), str(w), str(b), dtype], env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    return dict(np.load(out))


def _compare(a, b, loss_rel, min_cos, max_rel):
    la, lb = a["stats"][0] / a["stats"][1], b["stats"][0] / b["stats"][1]
    assert a["stats"][1] == b["stats"][1]
    assert abs(la - lb) <= loss_rel * abs(lb), (la, lb)
    worst = (1.0, None, 0.0)
    for k in a:
        if k == "stats":
            continue
        x, y = a[k].reshape(-1).astype(np.float64), b[k].reshape(-1).astype(np.float64)
        c = float(x @ y) / (np.linalg.norm(x) * np.linalg.norm(y) + 1e-300)
        r = float(np.abs(x - y).max() / (np.abs(y).max() + 1e-300))
        if c < worst[0]:
            worst = (c, k, r)
        assert c > min_cos and r < max_rel, (k, c, r)
    return worst


@pytest.mark.parametrize("h,w", [(64, 256), (50, 150)])
def test_kernel_generations_agree(tmp_path, h, w):
    base = _run(tmp_path, "default", {}, h, w, 4)
    for name, env, bars in (
            ("pool_separate", {"LXO_POOL_FUSED": "0"}, (1e-5, 0.99999, 1e-2)),
            ("conv1_valu", {"LXO_CONV1_MFMA": "0"}, (1e-3, 0.999, 5e-2)),
            ("att_forward_only", {"LXO_ATT_ALT": "0"}, (1e-5, 0.99999, 1e-2)),
            ("tn_packing_kernel", {"LXO_GEMM_TN_TR": "0"}, (1e-5, 0.99999, 1e-2)),
            ("nt_register_staged", {"LXO_GEMM_NT_DMA": "0"}, (1e-5, 0.99999, 1e-2)),
            ("split_k_steps", {"LXO_STEP_KERNELS": "1"}, (1e-4, 0.9995, 5e-2)),
            ("fused_step_launches", {"LXO_STEP_KERNELS": "2"}, (1e-4, 0.9995, 5e-2)),
            # the general halo conv kernel (what Cout % 64 != 0 or a tensor of 2 GB and more runs on) for every layer; no fused pools there
            ("general_halo_conv", {"LXO_CONV_2WG": "0"}, (1e-4, 0.9995, 5e-2)),
            # 128-channel conv tiles for every launch (the default gives a launch of fewer than 256 such tiles -- this batch of 4 -- 64-channel tiles): the
            # same products in the same order per output element; only the bias-gradient atomics group differently
            ("conv_128_channel_tiles", {"LXO_CONV_SMALL": "0"}, (1e-5, 0.99999, 1e-2)),
            # the stream switches: half-batch chains on two streams (on the split-K step kernels; off by default), and every weight gradient on
            # the compute stream instead of the second stream (the same kernels, other order of the f32 atomics)
            ("two_half_batch_chains", {"LXO_DUAL_STREAM": "1"}, (1e-4, 0.9995, 5e-2)),
            ("wgrad_on_the_compute_stream", {"LXO_ENC_OVERLAP": "0"}, (1e-5, 0.99999, 1e-2))):
        other = _run(tmp_path, name, env, h, w, 4)
        worst = _compare(base, other, *bars)
        print("%dx%d default vs %s: worst cosine %.8f (%s, max rel %.2e)" % (h, w, name, worst[0], worst[1], worst[2]))


def test_step_kernel_row_tiles_agree(tmp_path):
    """The fused step kernels with 16-row tiles (default where 32-row tiles would leave CUs idle) vs 32 / 64-row tiles
    (LXO_RSTEP_MT16=0) at a batch that takes the 16-row path (40 rows).  Every output element of a step kernel is the same
    contraction in the same order whatever the row tile, so:
    * in the f32 parity mode -- whose reductions are all ordered (no float atomics) -- the loss statistics
      and all 28 gradients are BIT-IDENTICAL between the two tilings;
    * in bf16 mode the step kernels still agree exactly, but the loss sum and several gradients are accumulated with f32 atomics whose
      order differs from run to run of ONE binary (the round-3 driver run measured 1.06e-6 on the loss of this very pair), so the bars
      are those of the other pairs (1e-5 ~ 20 ulp of the loss)."""
    base = _run(tmp_path, "f32_default", {}, 32, 128, 40, "f32")
    other = _run(tmp_path, "f32_mt32", {"LXO_RSTEP_MT16": "0"}, 32, 128, 40, "f32")
    assert sorted(base) == sorted(other)
    diff = [k for k in base if not np.array_equal(base[k], other[k])]
    assert not diff, "f32 parity mode: 16-row vs 32-row tiles differ in %s" % diff
    base = _run(tmp_path, "default", {}, 32, 128, 40)
    other = _run(tmp_path, "mt32", {"LXO_RSTEP_MT16": "0"}, 32, 128, 40)
    worst = _compare(base, other, 1e-5, 0.99999, 1e-2)
    print("16-row vs 32-row step tiles: f32 bit-identical; bf16 worst cosine %.8f (%s, max rel %.2e)" % worst)


_BEAM_SNIPPET = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r)
from latex_ocr_amd import synthetic
from latex_ocr_amd.engine import Engine
from latex_ocr_amd.model.utils.image import pad_batch_images
imgs, _ = synthetic.make_set(6, 40, 160, 60, 3, 9, seed=21)
img = pad_batch_images(imgs)
out = {}
for dt in ("f32", "bf16"):
    eng = Engine(60, dtype=dt, beam=3, max_steps=24, seed=4)
    ids, par = eng.beam_decode(img, 59, 3, max_iter=20, return_parents=True)[:2]
    out[dt + "_ids"] = np.asarray(ids); out[dt + "_par"] = np.asarray(par)
np.savez(sys.argv[1], **out)
'''


def test_beam_parents_read_in_place_equal_the_reordering_launch(tmp_path):
    """Beam decode on the fused step kernels reads a step's previous state THROUGH the parents (rstep.h: a_par) where it used to re-order the rows with a
    launch of its own (beam_search_decoder_cell.py:176-178); LXO_BEAM_INDIRECT=0 brings the launch back.  Same arithmetic on the same rows: ids and parents
    must be identical, in the f32 parity mode and in bf16."""
    outs = []
    for name, env in (("inplace", {}), ("reorder", {"LXO_BEAM_INDIRECT": "0"})):
        out = os.path.join(str(tmp_path), name + ".npz")
        e = dict(os.environ); e.update(env)
        r = subprocess.run([sys.executable, "-c", _BEAM_SNIPPET % os.path.dirname(HERE), out], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0, r.stdout.decode()[-2000:]
        outs.append(dict(np.load(out)))
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
