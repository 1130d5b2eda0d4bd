"""The k best paths under position-dependent scores (nfst_positional_kbest) next to the 1-best
ops.positional_viterbi and the arc-only ops.k_best of the same batch, in the same run.  Writes
profiles/positional_kbest.json:

  positional_viterbi        ops.positional_viterbi (best path under pos_scores)
  k_best_k{K}               ops.k_best_terms at K = 1, 5, 20, 64 (no position scores, no length budget)
  positional_k_best_k{K}    ops.positional_k_best_terms at the same K: the two launches and the workspace allocation
  ws_bytes_k{K}             nfst_positional_kbest_ws_bytes: every list of every position

on the BASELINE batch (synth.bench_batch(256)) at T = 140 and on 64 SNIPS-shaped lattices at T = 748 (the batches'
depths); every lattice has its own random pos_scores [B, T, V].

Cold, as profiles/bench_kbest.py measures: ROTATE copies of the batch and of pos_scores are resident and take turns, so
that no launch finds the data of the previous one in the caches.  Every call is timed with CUDA events around it (GPU
time, incl. gaps between its launches) and host wall time to the end of a synchronise after it; medians of ITERS calls."""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfst_amd import _lib, ops, synth  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402

ITERS = int(os.environ.get("ITERS", "10"))
ROTATE = int(os.environ.get("ROTATE", "4"))
KS = tuple(int(k) for k in os.environ.get("KS", "1,5,20,64").split(","))
dev = torch.device("cuda")


def timed(fns, iters=ITERS):
    """fns: one callable per resident copy; call k runs fns[k % len(fns)]."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    ev, wall = [], []
    for k in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        fns[k % len(fns)]()
        e.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(s.elapsed_time(e))
    return {"event_ms": round(statistics.median(ev), 4), "wall_ms": round(statistics.median(wall), 4)}


def measure(name, lats, theta_np, T):
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0 = copies[0]
    B, V = lat0.n_lattices, lat0.vocab
    assert T == int(lat0.depth.max())
    theta = torch.from_numpy(theta_np).to(dev)
    poss = [torch.randn(B, T, V, device=dev, generator=torch.Generator(dev).manual_seed(k)) for k in range(ROTATE)]
    r = {"lattices": B, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows), "T": T, "rotate": ROTATE}
    r["positional_viterbi"] = timed([lambda lat=lat, pos=pos: ops.positional_viterbi(lat, theta, pos) for lat, pos in zip(copies, poss)])
    print(name, "positional_viterbi", json.dumps(r["positional_viterbi"]), flush=True)
    for k in KS:
        r[f"ws_bytes_k{k}"] = int(_lib.lib.nfst_positional_kbest_ws_bytes(C.byref(lat0.c_struct()), T, k))
        r[f"k_best_k{k}"] = timed([lambda lat=lat: ops.k_best_terms(lat, theta, k) for lat in copies])
        r[f"positional_k_best_k{k}"] = timed([lambda lat=lat, pos=pos: ops.positional_k_best_terms(lat, theta, k, pos)
                                              for lat, pos in zip(copies, poss)])
        r[f"ratio_k{k}_over_positional_viterbi"] = round(r[f"positional_k_best_k{k}"]["event_ms"] / r["positional_viterbi"]["event_ms"], 2)
        r[f"ratio_k{k}_over_k_best"] = round(r[f"positional_k_best_k{k}"]["event_ms"] / r[f"k_best_k{k}"]["event_ms"], 2)
        print(name, f"k{k}", json.dumps({key: v for key, v in r.items() if key.endswith(f"_k{k}") or f"_k{k}_" in key}), flush=True)
    # a sanity check of the measurement, not a test: entry 0 is the 1-best path
    v = ops.positional_viterbi(copies[0], theta, poss[0])
    kb = ops.positional_k_best_terms(copies[0], theta, KS[0], poss[0])
    r["entry0_is_positional_viterbi"] = bool(torch.equal(v.best, kb.best[:, 0]) and torch.equal(v.path_arcs, kb.arcs[:, 0]))
    return r


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "positional_kbest.json"))
    out["baseline_b256"] = measure("baseline_b256", synth.bench_batch(256), synth.label_scores(1, 256), 140)
    with open(path, "w") as f:  # (written after each batch: the second one is the long one)
        json.dump(out, f, indent=1)
    out["snips_b64"] = measure("snips_b64", synth.snips_shaped_batch(64, vocab=250), synth.label_scores(64, 250, mean=-1.5, std=0.8), 748)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
