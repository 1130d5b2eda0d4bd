"""ns per tile of the beta sweep where its wave has a SIMD to itself (k_backward: sweep wave 0, tile waves 1, 2, 3, 5) and
where it shares one with two tile waves (k_forward_backward), and how often that sweep found a tile not decoded yet
(entries of tile_sweep2's wait_group per workgroup).  Instrumented build: python -m nfst_amd.build --variant prof -DNFST_PROF;
run with NFST_TUNING=1 NFST_LIB=.../libnfst_hip_prof.so.  Stamps (100 MHz) per workgroup, in both kernels: 0 entry, 5 the beta
sweep has its first decoded tile, 2 beta swept, 11 the count.

    python profiles/tune/tile_time.py [lattices] [rotate] [--json OUT.json --tag TAG]

`rotate` distinct resident batches take turns (cold launches, as bench.py); the stamps read are those of the last launch of
batch 0.  Per kernel: (swept - first tile) / beta tiles over the workgroups -- all of them, and the ones whose program is
within 10 % of the longest (the chain that decides the launch) -- and the count's sum, its maximum and the workgroups that
waited at all."""
import ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from nfst_amd import ops, synth, _lib
from nfst_amd.lattice import LatticeBatch

pos = [a for a in sys.argv[1:] if not a.startswith("--")]
opt = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None
for k in ("--json", "--tag"):
    if opt(k) in pos:
        pos.remove(opt(k))
B = int(pos[0]) if pos else 256
rot = int(pos[1]) if len(pos) > 1 else 4
dev = torch.device("cuda")
lats = [LatticeBatch.from_synth(synth.bench_batch(B, first_seed=1234 + 100000 * r), device=dev) for r in range(rot)]
theta = torch.from_numpy(synth.label_scores(1, 256)).to(dev)
raw = C.CDLL(_lib.LIB_PATH)
S = 16  # stamp slots per workgroup (kProfSlots, tile_pipeline.h)
tiles = lats[0].meta_host[:, _lib.META_BWD_TILES].astype(np.int64)
long_ = tiles >= 0.9 * tiles.max()


def stamps(launch):
    for it in range(10 * rot + 1):  # the last launch is batch 0 again, after the others have passed through the caches
        launch(it % rot)
    torch.cuda.synchronize()
    buf = np.zeros(B * S, np.uint64)
    assert raw.nfst_prof_read(buf.ctypes.data_as(C.c_void_p), B * S) == 0
    return buf.reshape(B, S).astype(np.int64)


def report(name, t):
    ns = (t[:, 2] - t[:, 5]) * 10.0 / tiles
    waits = t[:, 11]
    r = {"ns_per_tile_median": float(np.median(ns)), "ns_per_tile_min": float(ns.min()), "ns_per_tile_max": float(ns.max()),
         "ns_per_tile_long_programs_median": float(np.median(ns[long_])), "long_programs": int(long_.sum()),
         "sweep_us_longest_program": float((t[:, 2] - t[:, 5])[tiles.argmax()] / 100.0),
         "first_tile_us_after_entry_median": float(np.median(t[:, 5] - t[:, 0]) / 100.0),
         "wait_group_entries_sum": int(waits.sum()), "wait_group_entries_max": int(waits.max()),
         "workgroups_that_waited": int((waits > 0).sum()), "wait_group_entries_long_programs_median": float(np.median(waits[long_]))}
    print(name, json.dumps(r))
    return r


outs = [None] * rot
def fb(r):
    outs[r] = ops.forward_backward(lats[r], theta, out=outs[r])
res = {"lattices": B, "rotate": rot, "beta_tiles": {"min": int(tiles.min()), "median": float(np.median(tiles)), "max": int(tiles.max())},
       "k_backward": report("k_backward", stamps(lambda r: ops.backward(lats[r], theta))),
       "k_forward_backward": report("k_forward_backward", stamps(fb))}
if opt("--json"):
    path = opt("--json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc.setdefault("tile_time", {})[opt("--tag") or "new"] = res
    json.dump(doc, open(path, "w"), indent=1)
