"""End to end at cfg5 size (K = 32, 16 x 16, 65 536 signals, cfg5's search options), same phi: the host route to the top-3
rows, peak_search.batched_peak_search(phi, 16, 16, opts, top=3), against ops.peak_top(phi, 16, 16, opts, top=3) plus the
copy of its result to the host.  One warm-up, five alternating rounds, torch.cuda.synchronize around each; prints every
time, the medians, their ratio and whether the two routes returned the same bits.  Usage: python profiles/r05/e2e_top_peaks.py"""
import os, sys, time, statistics
import numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import admm_net_amd as A
from admm_net_amd import ops, peak_search, synth
dev = torch.device("cuda:0")
Nb = Nd = 16
B = 65536
opts = {"xstep": 1.0 / 65, "ystep": 1.0 / 32, "iter": 2}
torch.manual_seed(0)
m = A.PhiEstADMMNet(M=Nb, N=Nd, num_layers=32).eval()
ty, tb, ts, _ = synth.make_batch_device(B, Nb, Nd, seed=20260104, device=dev)
phi = m(ty, tb, ts)
torch.cuda.synchronize()
del m
def route_a():
    return peak_search.batched_peak_search(phi, 16, 16, opts, top=3)
def route_b():
    rows, cnt = ops.peak_top(phi, 16, 16, opts, top=3)
    return rows.cpu(), cnt.cpu()
def timed(fn):
    torch.cuda.synchronize(); t = time.perf_counter(); r = fn(); torch.cuda.synchronize(); return time.perf_counter() - t, r
ta, tb_ = [], []
_, ra = timed(route_a); _, rb = timed(route_b)            # warm-up
print("warm-up done", flush=True)
for i in range(5):
    t, ra = timed(route_a); ta.append(t)
    t, rb = timed(route_b); tb_.append(t)
    print(f"round {i}: host route {ta[-1]:.4f} s, peak_top + copy {tb_[-1]:.6f} s", flush=True)
same = all(np.array_equal(np.asarray(ra[i]).view(np.int64), rb[0][i, :len(ra[i])].numpy().view(np.int64)) for i in range(B))
print("results equal bit for bit:", same, " max count", int(rb[1].max()))
ma, mb = statistics.median(ta), statistics.median(tb_)
print(f"MEDIAN host route {ma:.4f} s ; peak_top + copy {mb:.6f} s ; ratio {ma / mb:.1f}")
print("all a:", ta, "all b:", tb_)
