"""The product of a batch with a sparse automaton of up to 4096 states (nfst_intersect_wide_count / _write, DESIGN.md
section 4.19) next to the 64-state route (section 4.8) in the same run.  Writes profiles/intersect_wide.json:

  q64                one automaton declared with 64 states through BOTH routes: at most two arcs with label 5, its three counts on the
                     states 0, 31 and 62, the other states without a transition (three pairs per lattice state keep every
                     product of the BASELINE batch, of up to 2201 rows each, under the limit of 8192 rows; a counter that
                     uses all 64 states does not):
    narrow / wide      intersect  ops.intersect end to end: both launches, the read-back of the counts, the device packer
                       count      the count entry point alone on preallocated buffers (k_kbest_levels + the count kernel)
                       write      the write entry point alone on preallocated buffers
    ratio_*            wide over narrow, event time
  sequence           per lattice the exact string of a path drawn from it (WideDFA.sequence, ragged): intersect, count, write
  marked_sequence    per lattice "the labels after label 4 spell those of the drawn path" (WideDFA.marked_sequence)

on the BASELINE batch (synth.bench_batch(256)) and on 64 SNIPS-shaped lattices, whose random labels carry few marks
(W = 1).  The numerator case itself, W > 1:

  numerator_y40      64 denominator lattices x o T (the edit grid of tests/intersect_wide_ref.edit_denominator: |x| = 12, any
                     of four output symbols after the output mark, at most 40 of them; 3467 rows each) with one
                     marked_sequence(y) per lattice, |y| = 40: 82 states, W = 2; intersect, count, write, and
                     ops.constraint_log_prob (the product, its log Z and the denominator's)
  numerator_y140     the same at |x| = 4, |y| = 140 (the longest path the BASELINE batch draws): 4211 rows, 282 states, W = 5

A workload whose largest automaton
has more than 4096 states is recorded as skipped, with that size, one that the library refuses (a product beyond the row
limit, an empty product) as refused, with the message.

Cold, as profiles/bench_intersect.py measures: ROTATE copies of the batch are resident and take turns.  Every call is
timed with CUDA events around it and host wall time to the end of a synchronise after it; medians of ITERS calls."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_intersect import raw_calls as narrow_raw_calls  # noqa: E402
from bench_slack import ROTATE, ITERS, dev, timed  # noqa: E402
from nfst_amd import ops, synth  # noqa: E402
from nfst_amd._lib import NfstError, check, lib  # noqa: E402
from nfst_amd.constraints import MAX_WIDE_STATES, ConstraintDFA, WideDFA  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402

MARKER = 4


def wide_raw_calls(lat, dfa):
    """(count, write): the two C entry points on buffers allocated once, sized by a first count."""
    B = lat.n_lattices
    head = [t.data_ptr() for t in dfa.to(dev)] + [1 if dfa.n_lattices is None else B, dfa.n_states]
    bs = C.byref(lat.c_struct())
    ws_bytes = int(lib.nfst_intersect_wide_ws_bytes(bs, dfa.n_states))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    cs = torch.zeros(3 * B, dtype=torch.int32, device=dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def count():
        check(lib.nfst_intersect_wide_count(bs, *head, ws.data_ptr(), ws_bytes, cs.data_ptr(), cs[2 * B:].data_ptr(), stream()),
              "nfst_intersect_wide_count")

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
        check(lib.nfst_intersect_wide_write(bs, *head, ws.data_ptr(), ws_bytes, off_d[0].data_ptr(), off_d[1].data_ptr(),
                                            i32[0].data_ptr(), i32[1].data_ptr(), i32[2].data_ptr(), arc_map.data_ptr(), i32[3].data_ptr(),
                                            rows[0].data_ptr(), rows[1].data_ptr(), stream()), "nfst_intersect_wide_write")

    return count, write, (lat, dfa, ws, cs, off_d, i32, arc_map, rows, ws_bytes)


def route(copies, dfa, raw):
    x = {"intersect": timed([lambda lat=lat: ops.intersect(lat, dfa) for lat in copies])}
    raws = [raw(lat, dfa) for lat in copies]
    x["count"] = timed([c for c, _, _ in raws])
    x["write"] = timed([w for _, w, _ in raws])
    return x


def measure(name, lats, theta_np):
    V = lats[0].vocab
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0 = copies[0]
    theta = torch.from_numpy(theta_np).to(dev)
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows),
         "max_depth": int(lat0.depth.max()), "rotate": ROTATE}
    delta = np.full((64, V), -1, np.int64)
    for c in range(3):
        delta[31 * c] = 31 * c
        delta[31 * c, 5] = 31 * (c + 1) if c < 2 else -1
    narrow = ConstraintDFA(delta, np.ones(64))
    wide = WideDFA.from_constraint(narrow)
    p = ops.intersect(lat0, wide).lattice
    q = {"automaton_states": 64, "exceptions": int(wide.exc_label.size), "product_rows": int(p.total_rows), "product_arcs": int(p.total_arcs),
         "narrow": route(copies, narrow, narrow_raw_calls), "wide": route(copies, wide, wide_raw_calls)}
    for k in ("intersect", "count", "write"):
        q["ratio_wide_over_narrow_" + k] = round(q["wide"][k]["event_ms"] / q["narrow"][k]["event_ms"], 2)
    r["q64"] = q
    # one drawn path per lattice
    s = ops.sample_paths(lat0, theta, 1, seed=7)
    paths, lens = s.paths.cpu().numpy()[:, 0], s.lengths.cpu().numpy()[:, 0]
    r["drawn_path_labels"] = {"mean": float(lens.mean()), "max": int(lens.max())}
    marked = [[int(paths[b, t + 1]) for t in range(lens[b] - 1) if paths[b, t] == MARKER] for b in range(len(lats))]
    r["drawn_path_marks"] = {"mean": float(np.mean([len(m) for m in marked])), "max": max(len(m) for m in marked)}
    builders = {"sequence": (int(lens.max()) + 1, lambda: WideDFA.stack([WideDFA.sequence(V, paths[b, :lens[b]]) for b in range(len(lats))])),
                "marked_sequence": (2 * (max(len(m) for m in marked) + 1),
                                    lambda: WideDFA.stack([WideDFA.marked_sequence(V, MARKER, m) for m in marked]))}
    for tag, (need, build) in builders.items():
        if need > MAX_WIDE_STATES:
            r[tag] = {"skipped": f"the largest automaton needs {need} states"}
            continue
        dfa = build()
        try:
            p = ops.intersect(lat0, dfa).lattice
        except (NfstError, ValueError) as e:
            r[tag] = {"automaton_states_max": dfa.n_states, "refused": str(e)}
            continue
        x = {"automaton_states_max": dfa.n_states, "words": (dfa.n_states + 63) // 64, "exceptions": int(dfa.exc_label.size),
             "product_rows": int(p.total_rows), "product_arcs": int(p.total_arcs),
             "workspace_bytes": int(lib.nfst_intersect_wide_ws_bytes(C.byref(lat0.c_struct()), dfa.n_states))}
        x.update(route(copies, dfa, wide_raw_calls))
        r[tag] = x
    print(name, json.dumps(r), flush=True)
    return r


def measure_numerator(name, x_len, n_out, n_lattices=64, V=64):
    from tests.intersect_wide_ref import edit_denominator

    rng = np.random.default_rng(n_out)
    symbols = (20, 21, 22, 23)
    lats = [edit_denominator([10 + int(c) for c in rng.integers(0, 6, x_len)], symbols, n_out, V) for _ in range(n_lattices)]
    dfa = WideDFA.stack([WideDFA.marked_sequence(V, MARKER, [symbols[int(c)] for c in rng.integers(0, 4, n_out)]) for _ in lats])
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0 = copies[0]
    theta = torch.from_numpy(synth.label_scores(8, V, mean=-0.5, std=0.5)).to(dev)
    p = ops.intersect(lat0, dfa).lattice
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows), "max_depth": int(lat0.depth.max()),
         "rotate": ROTATE, "automaton_states_max": dfa.n_states, "words": (dfa.n_states + 63) // 64, "exceptions": int(dfa.exc_label.size),
         "product_rows": int(p.total_rows), "product_arcs": int(p.total_arcs),
         "workspace_bytes": int(lib.nfst_intersect_wide_ws_bytes(C.byref(lat0.c_struct()), dfa.n_states))}
    r.update(route(copies, dfa, wide_raw_calls))
    r["constraint_log_prob"] = timed([lambda lat=lat: ops.constraint_log_prob(lat, theta, dfa) for lat in copies])
    r["log_z_of_the_denominator"] = timed([lambda lat=lat: ops.log_z(lat, theta) for lat in copies])
    print(name, json.dumps(r), flush=True)
    return r


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    out["numerator_y40"] = measure_numerator("numerator_y40", 12, 40)
    out["numerator_y140"] = measure_numerator("numerator_y140", 4, 140)
    out["baseline_b256"] = measure("baseline_b256", synth.bench_batch(256), synth.label_scores(1, 256))
    out["snips_b64"] = measure("snips_b64", synth.snips_shaped_batch(64, vocab=250), synth.label_scores(64, 250, mean=-1.5, std=0.8))
    path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "intersect_wide.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
