"""The forward chain with and without the formula lengths (lxo_decoder_train_fwd_live against lxo_decoder_train_fwd): per-phase durations from
the in-kernel 100 MHz timestamps (lxo_xdec_debug), B=64, 128x512, V=500, lengths U{30..100} (bench.py's array), T=101.
With lengths the phase means mix live and silent workgroups (a silent workgroup's P3 is short and its wait for the partials, inside P4, is the
live workgroups' stream): step_us is the figure to compare.  bench.py's chain_phases keeps measuring the call without lengths."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from latex_ocr_amd import synthetic
from latex_ocr_amd.engine import Engine, _p
from latex_ocr_amd.model.utils.image import pad_batch_images
from latex_ocr_amd.model.utils.text import pad_batch_formulas

B, H, W, V = [int(x) for x in os.environ.get("XS_SHAPE", "64,128,512").split(",")] + [500]
LLO, LHI = [int(x) for x in os.environ.get("XS_LEN", "30,101").split(",")]
imgs, forms = synthetic.make_set(B, H, W, V, LLO, LHI, seed=1234)
img = pad_batch_images(imgs)
f, l = pad_batch_formulas(forms, V - 2, V - 1)
T = f.shape[1]
eng = Engine(V, dtype="bf16", seed=0)
for _ in range(int(os.environ.get("XS_WARM", "25"))):              # the clock the chip holds under the training step, as bench.py's chain_phases
    eng.train_step(img, f, l, 1e-3, sync_loss=False)
eng.forward(img, f, lengths=l)
torch.cuda.synchronize()
print("shape B=%d %dx%d T=%d, live share of the (step, sample) pairs %.4f, chain status %s" % (B, H, W, T, float(l.sum()) / (T * B), eng.chain_status()))
eng.lib.lxo_xdec_debug.argtypes = [ctypes.c_void_p]
names = ["P1 lstm", "barrier 1", "P2 att_h", "barrier 2", "P3 attention", "barrier 3", "P4 merge + o", "barrier 4"]
for live in (False, True, False, True):
    buf = torch.zeros(256 * T * 16, dtype=torch.int64, device="cuda")
    eng.lib.lxo_xdec_debug(ctypes.c_void_p(buf.data_ptr()))
    for _ in range(2):
        eng._decoder_fwd(eng._stream(), live)
    torch.cuda.synchronize()
    eng.lib.lxo_xdec_debug(ctypes.c_void_p(0))
    s = buf.cpu().numpy().reshape(256, T, 16).astype(np.float64) * 0.01      # us
    d = s[:, 2:, 1:9] - s[:, 2:, 0:8]                                          # [wg][t][phase]
    pw = s[:, 2:, 12] - s[:, 2:, 6]
    print("%-16s step_us %.3f   chain_ms_per_launch %.4f   partials_poll_wait %.3f   status %s" % (
        "with lengths" if live else "without lengths", (s[:, 2:, 8] - s[:, 2:, 0]).mean(), (s[:, T - 1, 8].max() - s[:, 0, 0].min()) * 1e-3,
        pw[pw > 0].mean() if (pw > 0).any() else 0.0, eng.chain_status()))
    print("    " + "   ".join("%s %.3f" % (n, d[:, :, i].mean()) for i, n in enumerate(names)))
