"""Arc slack and beam pruning (nfst_arc_slack) next to the 1-best Viterbi and the
forward-backward of the same batch.  Writes profiles/slack.json:

  viterbi            ops.viterbi (best path, labels, arcs)
  forward_backward   ops.forward_backward (log Z and arc posteriors)
  arc_slack          ops.arc_slack with a beam (slack, keep, n_kept: the kernel and the allocation of its outputs)
  prune              ops.prune end to end at the ~10 % beam: arc_slack, the read-back of n_kept, the device packer
  keep50 / keep10    per lattice, the beam at the median / the 10 % quantile of its finite slacks: arcs kept, and
                     ops.forward_backward on the pruned batch

on the BASELINE batch (synth.bench_batch(256)), on 64 SNIPS-shaped lattices and on one SNIPS-shaped lattice.

Cold, as bench.py measures: ROTATE copies of the batch are resident and take turns, so that no launch finds the data of
the previous one in the caches.  Every call is timed with CUDA events around it (GPU time, incl. gaps between its
launches) and host wall time to the end of a synchronise after it; medians of ITERS calls.  The kernels alone:
rocprofv3 --kernel-trace --stats of the same command (profiles/slack_kernel_stats.csv; see profiles/README.md)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nfst_amd import ops, synth  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402

ITERS = int(os.environ.get("ITERS", "20"))
ROTATE = int(os.environ.get("ROTATE", "4"))
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


def quantile_beams(lat, slack, q):
    """[B] float32: per lattice, the q-quantile of its finite slacks."""
    s = slack.cpu().numpy()
    out = np.zeros(lat.n_lattices, np.float32)
    for b in range(lat.n_lattices):
        x = s[lat.arc_off[b]:lat.arc_off[b] + lat.n_arcs[b]]
        out[b] = np.quantile(x[np.isfinite(x)], q)
    return torch.from_numpy(out).to(dev)


def measure(name, lats, theta_np):
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0 = copies[0]
    theta = torch.from_numpy(theta_np).to(dev)
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows),
         "max_depth": int(lat0.depth.max()), "max_tiles": int(lat0.max_tiles), "rotate": ROTATE}
    slack = ops.arc_slack(lat0, theta).slack
    beams = {"keep50": quantile_beams(lat0, slack, 0.5), "keep10": quantile_beams(lat0, slack, 0.1)}
    r["viterbi"] = timed([lambda lat=lat: ops.viterbi(lat, theta) for lat in copies])
    r["forward_backward"] = timed([lambda lat=lat: ops.forward_backward(lat, theta, want_alpha_beta=False) for lat in copies])
    r["arc_slack"] = timed([lambda lat=lat: ops.arc_slack(lat, theta, beam=beams["keep10"]) for lat in copies])
    r["prune"] = timed([lambda lat=lat: ops.prune(lat, theta, beams["keep10"]) for lat in copies])
    for tag, beam in beams.items():
        pruned = [ops.prune(lat, theta, beam) for lat in copies]
        p0 = pruned[0]
        r[tag] = {"arcs_kept": int(p0.lat.total_arcs), "fraction": round(p0.lat.total_arcs / lat0.total_arcs, 4),
                  "max_tiles": int(p0.lat.max_tiles),
                  "forward_backward": timed([lambda p=p: ops.forward_backward(p.lat, theta, want_alpha_beta=False) for p in pruned])}
    r["ratio_arc_slack_over_viterbi"] = round(r["arc_slack"]["event_ms"] / r["viterbi"]["event_ms"], 3)
    r["ratio_arc_slack_over_forward_backward"] = round(r["arc_slack"]["event_ms"] / r["forward_backward"]["event_ms"], 3)
    print(name, json.dumps(r), flush=True)
    return r


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    out["baseline_b256"] = measure("baseline_b256", synth.bench_batch(256), synth.label_scores(1, 256))
    snips_theta = synth.label_scores(64, 250, mean=-1.5, std=0.8)
    out["snips_b64"] = measure("snips_b64", synth.snips_shaped_batch(64, vocab=250), snips_theta)
    out["snips_b1"] = measure("snips_b1", synth.snips_shaped_batch(1, vocab=250), snips_theta)
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "slack.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
