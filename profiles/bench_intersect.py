"""The product of a batch with a constraint automaton (nfst_intersect_count / _write) next to
ops.prune and one forward-backward step of the same batch.  Writes profiles/intersect.json:

  forward_backward   ops.forward_backward (log Z and arc posteriors) on the input batch
  prune              ops.prune end to end at the beam that keeps ~10 % of the arcs (arc_slack, read-back, device packer)
  per automaton (parity of the labels 3 .. V/2, at most three arcs with label 5):
    intersect          ops.intersect end to end: both launches, the read-back of the counts, the device packer
    count              nfst_intersect_count alone on preallocated buffers (k_kbest_levels + k_intersect_count)
    write              nfst_intersect_write alone on preallocated buffers (k_intersect_write)
    product            rows, arcs and tiles of the product, and ops.forward_backward on it

on the BASELINE batch (synth.bench_batch(256)) and on 64 SNIPS-shaped lattices.

Cold, as bench.py and profiles/bench_slack.py measure: ROTATE copies of the batch are resident and take turns, so that
no launch finds the data of the previous one in the caches.  Every call is timed with CUDA events around it (GPU time,
incl. gaps between its launches) and host wall time to the end of a synchronise after it; medians of ITERS calls.  The
kernels one by one: rocprofv3 --kernel-trace --stats of the same command (see profiles/README.md)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_slack import ROTATE, ITERS, dev, quantile_beams, timed  # noqa: E402
from nfst_amd import ops, synth  # noqa: E402
from nfst_amd._lib import check, lib  # noqa: E402
from nfst_amd.constraints import ConstraintDFA  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402


def raw_calls(lat, dfa):
    """(count, write): the two C entry points on buffers allocated once, sized by a first count."""
    B = lat.n_lattices
    delta_t, fin = dfa.to(dev)
    bs = C.byref(lat.c_struct())
    ws_bytes = int(lib.nfst_intersect_ws_bytes(bs, dfa.n_states))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    cs = torch.zeros(3 * B, dtype=torch.int32, device=dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def count():
        check(lib.nfst_intersect_count(bs, delta_t.data_ptr(), 0, fin.data_ptr(), 0, dfa.n_states, ws.data_ptr(), ws_bytes,
                                       cs.data_ptr(), cs[2 * B:].data_ptr(), stream()), "nfst_intersect_count")

    count()
    cnt = cs.cpu().numpy()[:2 * B].reshape(B, 2).astype(np.int64)
    off = np.zeros((2, B + 1), np.int64)
    np.cumsum(cnt[:, 0], out=off[0, 1:])
    np.cumsum(cnt[:, 1], out=off[1, 1:])
    R, A = int(off[0, -1]), int(off[1, -1])
    off_d = torch.from_numpy(off).to(dev)
    i32 = [torch.empty(A, dtype=torch.int32, device=dev) for _ in range(4)]
    arc_map = torch.empty(A, dtype=torch.int64, device=dev)
    rows = [torch.empty(R, dtype=torch.int32, device=dev) for _ in range(2)]

    def write():
        check(lib.nfst_intersect_write(bs, delta_t.data_ptr(), 0, dfa.n_states, ws.data_ptr(), ws_bytes, off_d[0].data_ptr(),
                                       off_d[1].data_ptr(), i32[0].data_ptr(), i32[1].data_ptr(), i32[2].data_ptr(), arc_map.data_ptr(),
                                       i32[3].data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), stream()), "nfst_intersect_write")

    return count, write, (lat, delta_t, fin, ws, cs, off_d, i32, arc_map, rows)


def measure(name, lats, theta_np):
    V = lats[0].vocab
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0 = copies[0]
    theta = torch.from_numpy(theta_np).to(dev)
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows),
         "max_depth": int(lat0.depth.max()), "max_tiles": int(lat0.max_tiles), "rotate": ROTATE}
    r["forward_backward"] = timed([lambda lat=lat: ops.forward_backward(lat, theta, want_alpha_beta=False) for lat in copies])
    beam = quantile_beams(lat0, ops.arc_slack(lat0, theta).slack, 0.1)
    r["prune"] = timed([lambda lat=lat: ops.prune(lat, theta, beam) for lat in copies])
    automata = {"parity": ConstraintDFA.parity(V, range(3, V // 2)), "count_at_most_3": ConstraintDFA.count_at_most(V, [5], 3)}
    for tag, dfa in automata.items():
        x = {"automaton_states": dfa.n_states}
        x["intersect"] = timed([lambda lat=lat: ops.intersect(lat, dfa) for lat in copies])
        raws = [raw_calls(lat, dfa) for lat in copies]
        x["count"] = timed([c for c, _, _ in raws])
        x["write"] = timed([w for _, w, _ in raws])
        prods = [ops.intersect(lat, dfa).lattice for lat in copies]
        p0 = prods[0]
        x["product"] = {"rows": int(p0.total_rows), "arcs": int(p0.total_arcs), "max_rows": int(p0.n_rows.max()),
                        "max_tiles": int(p0.max_tiles),
                        "forward_backward": timed([lambda p=p: ops.forward_backward(p, theta, want_alpha_beta=False) for p in prods])}
        x["ratio_intersect_over_forward_backward"] = round(x["intersect"]["event_ms"] / r["forward_backward"]["event_ms"], 2)
        x["ratio_intersect_over_prune"] = round(x["intersect"]["event_ms"] / r["prune"]["event_ms"], 3)
        r[tag] = x
    print(name, json.dumps(r), flush=True)
    return r


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    out["baseline_b256"] = measure("baseline_b256", synth.bench_batch(256), synth.label_scores(1, 256))
    out["snips_b64"] = measure("snips_b64", synth.snips_shaped_batch(64, vocab=250), synth.label_scores(64, 250, mean=-1.5, std=0.8))
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "intersect.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
