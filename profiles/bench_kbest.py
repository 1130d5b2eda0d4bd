"""The k best paths (nfst_kbest) next to the 1-best Viterbi of the same batch.  Writes
profiles/kbest.json:

  viterbi          ops.viterbi (best path, labels, arcs)
  k_best_k{K}      ops.k_best at K = 1, 5, 20, 64 (forward only: the three kernels, the workspace allocation and the
                   status read-back that checks the path lengths)
  k_best_k20_fwd_bwd  ops.k_best(theta, 20).best summed, backward (the index_add over the returned arcs)

on the BASELINE batch (synth.bench_batch(256)), on 64 SNIPS-shaped lattices and, the decoder's case, on one
SNIPS-shaped lattice and one edit lattice alone.

Cold, as bench.py measures: ROTATE copies of the batch are resident and take turns, so that no launch finds the data of
the previous one in the caches.  Every call is timed with CUDA events around it (GPU time, incl. gaps between its
launches) and host wall time to the end of a synchronise after it; medians of ITERS calls.  The kernels alone:
rocprofv3 --kernel-trace --stats of the same command (profiles/kbest_kernel_stats.csv; see profiles/README.md)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfst_amd import ops, synth  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402

ITERS = int(os.environ.get("ITERS", "20"))
ROTATE = int(os.environ.get("ROTATE", "4"))
KS = (1, 5, 20, 64)
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


def measure(name, lats, theta_np):
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0 = copies[0]
    theta = torch.from_numpy(theta_np).to(dev)
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows),
         "max_depth": int(lat0.depth.max()), "rotate": ROTATE}

    def vit(lat):
        return lambda: ops.viterbi(lat, theta)

    def kb(lat, k):
        return lambda: ops.k_best(lat, theta, k)

    def kb_bwd(lat):
        def f():
            t = theta.clone().requires_grad_()
            b = ops.k_best(lat, t, 20).best
            b[torch.isfinite(b)].sum().backward()
        return f

    r["viterbi"] = timed([vit(lat) for lat in copies])
    for k in KS:
        r[f"k_best_k{k}"] = timed([kb(lat, k) for lat in copies])
    r["k_best_k20_fwd_bwd"] = timed([kb_bwd(lat) for lat in copies])
    for k in KS:
        r[f"ratio_k{k}_over_viterbi"] = round(r[f"k_best_k{k}"]["event_ms"] / r["viterbi"]["event_ms"], 3)
    print(name, json.dumps(r), flush=True)
    return r


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    out["baseline_b256"] = measure("baseline_b256", synth.bench_batch(256), synth.label_scores(1, 256))
    snips_theta = synth.label_scores(64, 250, mean=-1.5, std=0.8)
    out["snips_b64"] = measure("snips_b64", synth.snips_shaped_batch(64, vocab=250), snips_theta)
    out["snips_b1"] = measure("snips_b1", synth.snips_shaped_batch(1, vocab=250), snips_theta)
    out["edit_b1"] = measure("edit_b1", [synth.edit_lattice(list(range(10, 40)), list(range(40, 66)), vocab=250, seed=5)],
                             snips_theta)
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "kbest.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
