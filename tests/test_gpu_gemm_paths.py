"""-m gpu: every dispatch path of lxo_gemm_nt, lxo_gemm_tn and lxo_gemm_slab on the GPU, element by element against the float64 reference
of tests/gemm_ref.py: odd extents, pitches larger than the extents, offset operand pointers, every epilogue branch, split ranges with and
without rows, NaN in everything the kernel must not read and a sentinel in everything it must not write.  One test per family over its
table with the default switches; one child process with LXO_GEMM_NT_DMA=0 LXO_GEMM_TN_TR=0 (the switches are read once per process) runs
the tables of the two switched kernels again, so both arms of both switches are held to the same bars.  Each test prints the worst
err / bound per kernel."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


class GpuAdapter(object):
    """the buffers of a case as torch tensors on cuda:0"""

    def __init__(self):
        from latex_ocr_amd import _abi
        self.L = _abi.load()

    def run(self, c, bufs):
        t = {k: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).to("cuda:0") for k, v in bufs.items() if v is not None}
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = G.invoke(self.L, c, t["A"].data_ptr(), t["B"].data_ptr(), t["C"].data_ptr(), t["bias"].data_ptr() if "bias" in t else 0, st)
        torch.cuda.synchronize()
        return rc, t["C"].cpu().numpy()


@pytest.mark.parametrize("fam", G.FAMILIES)
def test_family(fam):
    fails, worst, _ = G.run_table(GpuAdapter(), fam)
    assert not fails, "\n".join(fails)
    assert worst


def switched_tables(sw):
    """the NT DMA and tn_tr tables under the switches of this process -> the crc of each table's output bits; raises where a case fails"""
    crcs = {}
    for fam in G.SWITCHED:
        fails, _, crcs[fam] = G.run_table(GpuAdapter(), fam, sw=sw)
        assert not fails, "\n".join(fails)
    return crcs


def child_main():
    for fam, crc in switched_tables(G.ARMS_OFF).items():
        print("CRC %s %08x" % (fam, crc))


def test_switch_arms_off_in_a_child_process():
    """LXO_GEMM_NT_DMA=0 LXO_GEMM_TN_TR=0: the register-staged NT kernel and the packing TN kernel on the tables of the kernels they stand in
    for.  Prints whether the two NT arms gave the same bits (the TN arms add with atomics in another order)."""
    here = switched_tables(G.DEFAULT_SWITCHES)
    env = dict(os.environ, LXO_GEMM_NT_DMA="0", LXO_GEMM_TN_TR="0")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_gemm_paths as T; T.child_main()" % (HERE, os.path.dirname(HERE))
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode()
    print(out[-4000:])
    assert r.returncode == 0, out[-4000:]
    there = {ln.split()[1]: int(ln.split()[2], 16) for ln in out.splitlines() if ln.startswith("CRC ")}
    assert set(there) == set(G.SWITCHED)
    assert "nt<bf16,A=bf16,C=bf16,BK=64>" in out and "tn<bf16,A=bf16,B=bf16>" in out          # where the mirror sends these tables with the arms off
    print("NT arms (LDS-DMA against register-staged) bit-identical over the table: %s" % (here["nt_dma"] == there["nt_dma"]))
