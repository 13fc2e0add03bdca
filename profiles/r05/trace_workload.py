"""Kernel-trace workload: 4096 signals (16 x 16, K = 4 forward), cfg5's search options; 1 warm-up + 5 calls of
ops.peak_search and, where the checkout has it, of ops.peak_top.  Usage, once per checkout (parent commit, this commit):
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/r05/trace_workload.py <checkout root>
The per-dispatch times of spectrum_kernel, peaks_kernel and estimate_kernel are in OUT/*/*_kernel_trace.csv."""
import os, sys
import numpy as np, torch
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import admm_net_amd as A
from admm_net_amd import ops, synth, _lib
print("library:", _lib.LIB_PATH)
dev = torch.device("cuda:0")
Nb = Nd = 16
opts = {"xstep": 1.0 / 65, "ystep": 1.0 / 32, "iter": 2}
torch.manual_seed(0)
m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=4).eval()
ty, tb, ts, _ = synth.make_batch_device(4096, Nb, Nd, seed=20260104, device=dev)
phi = m(ty, tb, ts)
torch.cuda.synchronize()
for i in range(6):
    ops.peak_search(phi, 16, 16, opts, max_peaks=256)
    torch.cuda.synchronize()
if hasattr(ops, "peak_top"):
    for i in range(6):
        ops.peak_top(phi, 16, 16, opts, top=3)
        torch.cuda.synchronize()
print("done")
