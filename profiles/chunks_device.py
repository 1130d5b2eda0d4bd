"""Chunked programs cut on the device (nfst_pack_chunks_device_*, chunk_pack_kernels.h) on SNIPS-shaped batches
(BASELINE configs[2]: deep, narrow tagging machines), B = 8 and 64.  Writes profiles/chunks_device.json:

  pack            from_arcs_device without / with chunks=True: the device packer alone, and with the cutter behind it (the
                  difference is what the cut adds to the call: its two launches, the read-back of the plan and the layout)
  set_masks       LatticeScorer.set_masks on collated dense tables already on the GPU (the reference's trainer,
                  lightning.py:417), chunks off / on
  step            a trainer-shaped step: set_masks -> compute_log_beta -> log_z().sum().backward(), chunks off / on

Every call is timed with CUDA events around it and a synchronise after it (median of ITERS calls; host wall time beside).
The kernels of the cutter alone: ``--kernels`` runs the cut a few times for rocprofv3 --kernel-trace --stats (a run of its
own, see profiles/README.md)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfst_amd import synth  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402
from nfst_amd.scorers import LatticeScorer  # noqa: E402

ITERS = int(os.environ.get("ITERS", "20"))
V = 250
dev = torch.device("cuda")


def timed(fn, iters=ITERS):
    fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(s.elapsed_time(e))
    return {"event_ms": round(statistics.median(ev), 4), "wall_ms": round(statistics.median(wall), 4)}


def batch(B):
    lats = synth.snips_shaped_batch(B, vocab=V)
    arcs = synth.batch_arcs(lats)
    em, tr = synth.collate_dense([l.dense() for l in lats])
    return lats, arcs, torch.from_numpy(em).to(dev), torch.from_numpy(tr).to(dev)


def main():
    if "--kernels" in sys.argv:
        for B in (8, 64):
            _, (n_rows, arc_off, src, label, dst, _), _, _ = batch(B)
            src_d, label_d, dst_d = (torch.from_numpy(x).to(dev) for x in (src, label, dst))
            for _ in range(10):
                LatticeBatch.from_arcs_device(n_rows, arc_off, src_d, label_d, dst_d, V, device=dev, chunks=True)
            torch.cuda.synchronize()
        return
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS, "vocab": V}
    theta0 = synth.label_scores(64, V, mean=-1.5, std=0.8)
    for B in (8, 64):
        lats, (n_rows, arc_off, src, label, dst, _), em_d, tr_d = batch(B)
        src_d, label_d, dst_d = (torch.from_numpy(x).to(dev) for x in (src, label, dst))
        r = {"lattices": B, "rows": int(em_d.shape[1]), "arcs": int(arc_off[-1])}
        for name, ck in (("off", False), ("on", True)):
            r[f"pack_chunks_{name}"] = timed(lambda: LatticeBatch.from_arcs_device(n_rows, arc_off, src_d, label_d, dst_d, V, device=dev, chunks=ck))
        r["cut_added_ms"] = round(r["pack_chunks_on"]["event_ms"] - r["pack_chunks_off"]["event_ms"], 4)
        for name, ck in (("off", False), ("on", True)):
            model = LatticeScorer(V, theta=theta0, chunks=ck).to(dev)
            r[f"set_masks_chunks_{name}"] = timed(lambda: model.set_masks(em_d, tr_d))
            r[f"flavour_chunks_{name}"] = "chunked" if model.lattice.chunks is not None else "general"

            def step():
                model.set_masks(em_d, tr_d)
                model.compute_log_beta()
                model.log_z().sum().backward()
                model.theta.grad = None
            r[f"step_chunks_{name}"] = timed(step)
        r["step_speedup_on_vs_off"] = round(r["step_chunks_off"]["event_ms"] / r["step_chunks_on"]["event_ms"], 3)
        out[f"snips_b{B}"] = r
        print(json.dumps(r), flush=True)
    with open(os.path.join(ROOT, "profiles", "chunks_device.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
