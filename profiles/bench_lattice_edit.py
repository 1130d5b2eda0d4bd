"""The edit distance between a reference and a whole lattice (nfst_lattice_edit) next to what a
user had before it.  Writes profiles/lattice_edit.json, per batch:

  lattice_edit          ops.lattice_edit_distance with theta (the three kernels, the workspace allocation and the status
                        read-back)
  lattice_edit_unscored the same without scores
  ws_bytes              nfst_lattice_edit_ws_bytes at the batch's R
  kbest64_min           alternative (a): ops.k_best(k = 64) + ops.edit_distance + min, an upper bound only
  kbest64_bound_exceeds the share of lattices where that bound is above the true distance
  numpy_16              alternative (b): the NumPy restatement (tests/lattice_edit_ref.py) on the host, first 16 lattices
  kernels               k_kbest_levels / k_lattice_edit_sweep / k_lattice_edit_walk alone: average us per launch from
                        ``rocprofv3 --kernel-trace --stats`` of ``BATCH=<name> python profiles/bench_lattice_edit.py
                        trace`` (a run of its own per batch), merged by ``python profiles/bench_lattice_edit.py merge
                        <name> <kernel_stats.csv>``

on the BASELINE batch (synth.bench_batch(256)) and on 64 SNIPS-shaped lattices.  The reference of a lattice is one path
drawn by swor.sample(k = 1) with 10 % of its tokens replaced.

Cold, as bench.py measures: ROTATE copies of the batch are resident and take turns.  Every call is timed with CUDA events
around it and host wall time to the end of a synchronise after it; medians of ITERS calls (of 3 for the alternatives)."""
import csv
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfst_amd import _lib, ops, swor, synth  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402

ITERS = int(os.environ.get("ITERS", "20"))
ROTATE = int(os.environ.get("ROTATE", "4"))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "lattice_edit.json"))
KERNELS = ("k_kbest_levels", "k_lattice_edit_sweep", "k_lattice_edit_walk")


def batches():
    return {"baseline_b256": (synth.bench_batch(256), synth.label_scores(1, 256)),
            "snips_b64": (synth.snips_shaped_batch(64, vocab=250), synth.label_scores(64, 250, mean=-1.5, std=0.8))}


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


def references(lat, theta, vocab):
    """(ref [B, R] int32, lengths [B]): one drawn path per lattice, 10 % of its tokens replaced."""
    r = swor.sample(lat, theta, 1, seed=7)
    ref, n = r.paths[:, 0].cpu().numpy().copy(), r.lengths[:, 0].cpu().numpy()
    rng = np.random.default_rng(11)
    for b in range(len(n)):
        swap = rng.random(int(n[b])) < 0.1
        ref[b, :n[b]][swap] = rng.integers(synth.N_SPECIAL, vocab, size=int(swap.sum()))
    dev = lat.device
    ref = np.ascontiguousarray(ref[:, :max(1, int(n.max()))])  # (R = the longest reference: the workspace grows with R)
    return torch.from_numpy(ref).to(dev), torch.from_numpy(n.astype(np.int32)).to(dev)


def setup(name):
    lats, theta_np = batches()[name]
    dev = torch.device("cuda")
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    theta = torch.from_numpy(theta_np).to(dev)
    ref, n = references(copies[0], theta, len(theta_np))
    return lats, theta_np, copies, theta, ref, n


def measure(name):
    lats, theta_np, copies, theta, ref, n = setup(name)
    lat0 = copies[0]
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows), "max_depth": int(lat0.depth.max()),
         "R": int(ref.shape[1]), "ref_len_mean": round(float(n.float().mean()), 1), "ref_len_max": int(n.max()), "rotate": ROTATE,
         "ws_bytes": int(_lib.lib.nfst_lattice_edit_ws_bytes(ctypes.byref(lat0.c_struct()), int(ref.shape[1])))}

    def alt(lat):
        kb = ops.k_best(lat, theta, 64)
        d = ops.edit_distance(kb.paths, kb.lengths, ref, n)
        live = torch.arange(64, device=d.device)[None, :] < kb.n_paths[:, None]
        return torch.where(live, d, torch.full_like(d, 1 << 20)).min(dim=1).values

    r["lattice_edit"] = timed([lambda lat=lat: ops.lattice_edit_distance(lat, ref, n, theta) for lat in copies])
    r["lattice_edit_unscored"] = timed([lambda lat=lat: ops.lattice_edit_distance(lat, ref, n) for lat in copies])
    r["kbest64_min"] = timed([lambda lat=lat: alt(lat) for lat in copies], iters=3)
    exact = ops.lattice_edit_distance(lat0, ref, n, theta)
    r["distance_mean"] = round(float(exact.distance.float().mean()), 2)
    r["kbest64_bound_exceeds"] = round(float((alt(lat0) > exact.distance).float().mean()), 4)
    from tests import lattice_edit_ref as LR  # noqa: E402

    ref_np, n_np = ref.cpu().numpy(), n.cpu().numpy()
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = LR.of_batch(lats[:16], [ref_np[b, :n_np[b]] for b in range(16)], theta_np)
        host.append((time.perf_counter() - t0) * 1e3)
    r["numpy_16"] = {"wall_ms": round(statistics.median(host), 1)}
    assert [g["distance"] for g in got] == exact.distance[:16].tolist()  # (the op and the restatement agree)
    print(name, json.dumps(r), flush=True)
    return r


def trace(name):
    """The op alone, ITERS cold calls behind one warm-up per copy: the command rocprofv3 traces."""
    _, _, copies, theta, ref, n = setup(name)
    timed([lambda lat=lat: ops.lattice_edit_distance(lat, ref, n, theta) for lat in copies])


def merge(name, stats_csv):
    with open(OUT) as f:
        out = json.load(f)
    k = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            for kn in KERNELS:
                if kn + "(" in row["Name"] or kn + "<true>(" in row["Name"]:
                    k[kn] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 1),
                             "min_us": round(float(row["MinNs"]) / 1e3, 1), "max_us": round(float(row["MaxNs"]) / 1e3, 1)}
    out[name]["kernels"] = k
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        return trace(os.environ["BATCH"])
    if len(sys.argv) > 1 and sys.argv[1] == "merge":
        return merge(sys.argv[2], sys.argv[3])
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    for name in batches():
        out[name] = measure(name)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
