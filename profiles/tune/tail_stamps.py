"""Where the epilogue of the tile-wave k_forward_backward spends its time, per workgroup (instrumented build: python -m
nfst_amd.build --variant prof -DNFST_PROF; run with NFST_TUNING=1 NFST_LIB=.../libnfst_hip_prof.so).  Stamps (100 MHz, 16
slots per workgroup): 4 after the barrier, 8 a helper wave has issued the stores of its preloaded arc groups, 9 wave 0 has
issued its row outputs, 10 wave 0 has issued the remainder loop, 7 every store of the workgroup has left the CU.
python profiles/tune/tail_stamps.py [lattices] [rotate] [--all]: `rotate` distinct resident batches take turns (cold launches,
as bench.py); --all prints every workgroup, otherwise the 16 last finishers."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from nfst_amd import ops, synth, _lib
from nfst_amd.lattice import LatticeBatch
args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if len(args) > 0 else 256
rot = int(args[1]) if len(args) > 1 else 4
S = 16
dev = torch.device("cuda")
lats = [LatticeBatch.from_synth(synth.bench_batch(B, first_seed=1234 + 100000 * r), device=dev) for r in range(rot)]
theta = torch.from_numpy(synth.label_scores(1, 256)).to(dev)
outs = [None] * rot
for it in range(10 * rot + 1):  # the last launch is batch 0 again, after the others have passed through the caches
    r = it % rot
    outs[r] = ops.forward_backward(lats[r], theta, out=outs[r])
torch.cuda.synchronize()
raw = C.CDLL(_lib.LIB_PATH)
buf = np.zeros(B * S, np.uint64)
assert raw.nfst_prof_read(buf.ctypes.data_as(C.c_void_p), B * S) == 0
t = buf.reshape(B, S).astype(np.int64)
rel = (t - t[:, 0].min()) / 100.0  # us since the first workgroup's entry
lat = lats[0]
arcs = lat.meta_host[:, _lib.META_N_ARCS]
tiles = np.maximum(lat.meta_host[:, _lib.META_BWD_TILES], lat.meta_host[:, _lib.META_FWD_TILES])
# the five intervals of the epilogue
cols = ["barrier>pre", "pre>rows", "rows>rest", "rest>drained", "barrier>end"]
iv = np.stack([t[:, 8] - t[:, 4], t[:, 9] - t[:, 8], t[:, 10] - t[:, 9], t[:, 7] - t[:, 10], t[:, 7] - t[:, 4]], 1) / 100.0
last = np.argsort(rel[:, 7])[-16:]
print(f"B={B}, {rot} batches rotating; us.  preloaded-groups stamp: wave 10; rows / remainder stamps: wave 0 (it may pass the rows")
print("before wave 10 is through its groups: a negative pre>rows is that overlap); launch = last end %.2f, barrier window %.2f .. %.2f" %
      (rel[:, 7].max(), rel[:, 4].min(), rel[:, 4].max()))
print("lattices beyond 21,504 arcs: %d, beyond 24,576: %d, largest %d" % ((arcs > 21504).sum(), (arcs > 24576).sum(), arcs.max()))
print("%5s %6s %5s %8s %8s " % ("wg", "arcs", "tiles", "barrier", "end") + " ".join("%12s" % c for c in cols))
for b in (range(B) if "--all" in sys.argv else last):
    print("%5d %6d %5d %8.2f %8.2f " % (b, arcs[b], tiles[b], rel[b, 4], rel[b, 7]) + " ".join("%12.2f" % x for x in iv[b]))
print("median, all workgroups      " + " " * 8 + " ".join("%12.2f" % x for x in np.median(iv, 0)))
print("median, 16 last finishers   " + " " * 8 + " ".join("%12.2f" % x for x in np.median(iv[last], 0)))
big = arcs > 21504
if big.any() and (~big).any():
    print("median barrier>end: lattices beyond 21,504 arcs %.2f, the others %.2f" % (np.median(iv[big, 4]), np.median(iv[~big, 4])))
