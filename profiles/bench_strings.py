"""Output strings (nfst_merge_paths and nfst_string_logprob, DESIGN.md sections 4.20 and 4.21) next to what a user had
before them.  Writes profiles/strings.json, per workload:

  merge_paths_k{16,64,256}   ops.merge_paths on K rows per lattice (the 64 best paths, repeated or cut to K) with the
                             workload's tape, the status read-back included
  string_log_prob_m{1,20,64} ops.string_log_prob on the first M strings of decoders.decode_strings(k = 64): the level pass,
                             the sweep (in slices under 1 GiB of workspace), the status read-back
  constraint_loop_m{..}      alternative (a): one ops.constraint_log_prob per candidate, the lattices' automata stacked
                             (intersect, pack, two log Z each; float32); "failed": the calls that raised, which is what a
                             product beyond NFST_MAX_ROWS or a string that a lattice does not spell does
  numpy_16                   alternative (b): the NumPy restatement (tests/strings_ref.py), one candidate, first 16 lattices
  decode_strings_k64         decoders.decode_strings(k = 64) end to end

on the BASELINE batch (synth.bench_batch(256)) with keep = every second label, and on 64 edit grids (the denominator
lattices of tests/intersect_wide_ref.py) with the output mark.

Cold, as bench.py measures: ROTATE copies of the batch are resident and take turns.  Every call is timed with CUDA events
around it and host wall time to the end of a synchronise after it; medians of ITERS calls (of 3 for the alternatives)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nfst_amd import _lib, decoders, ops, synth  # noqa: E402
from nfst_amd.constraints import WideDFA  # noqa: E402
from nfst_amd.lattice import LatticeBatch  # noqa: E402

ITERS = int(os.environ.get("ITERS", "20"))
ROTATE = int(os.environ.get("ROTATE", "4"))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "strings.json"))
ONLY = os.environ.get("WORKLOAD", "")
MARK = 4


def grids(n=64):
    from tests import intersect_wide_ref as IW

    rng = np.random.default_rng(5)
    return [IW.edit_denominator([int(t) for t in rng.integers(6, 8, size=int(rng.integers(3, 7)))], [8, 9, 10], int(rng.integers(3, 6)), vocab=12)
            for _ in range(n)]


def workloads():
    return {"baseline_b256_keep": (lambda: synth.bench_batch(256), synth.label_scores(1, 256), dict(keep=set(range(3, 256, 2)))),
            "grids_b64_marker": (grids, synth.label_scores(1, 12, mean=-1.0, std=0.5), dict(marker=MARK))}


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


def constraint_loop(lat, theta, strings, lengths, tape, vocab):
    """Alternative (a): log p of every candidate through the product route; returns the number of calls that raised."""
    rows, n = strings.cpu().numpy(), lengths.cpu().numpy()
    failed = 0
    for m in range(rows.shape[1]):
        ys = [rows[b, m, :n[b, m]].tolist() for b in range(rows.shape[0])]
        try:
            if "marker" in tape:
                dfa = WideDFA.stack([WideDFA.marked_sequence(vocab, tape["marker"], y) for y in ys])
            else:
                dfa = WideDFA.stack([WideDFA.projected_sequence(vocab, tape["keep"], y) for y in ys])
            ops.constraint_log_prob(lat, theta, dfa)
        except (_lib.NfstError, ValueError, RuntimeError):
            failed += 1
    return failed


def measure(name):
    make, theta_np, tape = workloads()[name]
    lats = make()
    dev = torch.device("cuda")
    copies = [LatticeBatch.from_synth(lats, device=dev) for _ in range(ROTATE)]
    lat0, vocab = copies[0], len(theta_np)
    theta = torch.from_numpy(theta_np).to(dev)
    dec = decoders.decode_strings(lat0, theta, 64, **tape)
    r = {"lattices": lat0.n_lattices, "arcs": int(lat0.total_arcs), "rows": int(lat0.total_rows), "max_depth": int(lat0.depth.max()),
         "tape": sorted(tape)[0], "rotate": ROTATE, "strings_of_64_paths_mean": round(float(dec.n_strings.float().mean()), 1),
         "string_len_max": int(dec.lengths.max())}
    kb = ops.k_best(lat0, theta, 64)
    for K in (16, 64, 256):
        reps = (K + 63) // 64
        paths, lens = kb.paths.repeat(1, reps, 1)[:, :K].contiguous(), kb.lengths.repeat(1, reps)[:, :K].contiguous()
        w = kb.best.double().repeat(1, reps)[:, :K].contiguous()
        r[f"merge_paths_k{K}"] = timed([lambda: ops.merge_paths(paths, lens, w, vocab=vocab, **tape)])
    N = max(1, int(dec.lengths.max()))
    for M in (1, 20, 64):
        ys, n = dec.strings[:, :M, :N].contiguous(), dec.lengths[:, :M].contiguous()
        r[f"string_log_prob_m{M}"] = timed([lambda lat=lat: ops.string_log_prob(lat, theta, ys, n, **tape) for lat in copies])
        fails = []
        alt = timed([lambda lat=lat: fails.append(constraint_loop(lat, theta, ys, n, tape, vocab)) for lat in copies[:1]], iters=3)
        r[f"constraint_loop_m{M}"] = {**alt, "failed": int(fails[-1]), "calls": M}
        print(name, M, json.dumps(r[f"string_log_prob_m{M}"]), json.dumps(r[f"constraint_loop_m{M}"]), flush=True)
    r["decode_strings_k64"] = timed([lambda lat=lat: decoders.decode_strings(lat, theta, 64, **tape) for lat in copies])
    from tests import strings_ref as SR  # noqa: E402

    rows, n_np = dec.strings.cpu().numpy(), dec.lengths.cpu().numpy()
    cands = [[rows[b, 0, :n_np[b, 0]].tolist()] for b in range(16)]
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        num, z = SR.of_batch(lats[:16], theta_np, cands, **tape)
        host.append((time.perf_counter() - t0) * 1e3)
    r["numpy_16"] = {"wall_ms": round(statistics.median(host), 1), "candidates": 1}
    got = ops.string_log_prob(lat0, theta, dec.strings[:, :1], dec.lengths[:, :1], **tape)
    r["max_abs_error_vs_numpy_16"] = float(np.abs(got.log_num[:16, 0].cpu().numpy() - num[:, 0]).max())
    assert r["max_abs_error_vs_numpy_16"] <= 1e-9  # (the op and the restatement agree; the strings are spelled: finite)
    print(name, json.dumps(r), flush=True)
    return r


def main():
    out = {"device": torch.cuda.get_device_name(0), "iters": ITERS}
    if os.path.exists(OUT) and ONLY:
        with open(OUT) as f:
            out = json.load(f)
    for name in workloads():
        if not ONLY or ONLY == name:
            out[name] = measure(name)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
